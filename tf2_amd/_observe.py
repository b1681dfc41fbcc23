"""What the activation observers share on the Python side (audit.py, fidelity.py, caq.py; csrc/act_rows.h is the native counterpart):
the walk over a plan that lays out a store, the checks of reference tensors, the handle and device classes of the two observers that
read a keep_all step -- and `capture_graph`, the one way a step of this package becomes a HIP graph."""
from __future__ import annotations

from typing import List

import numpy as np

from . import _lib


def capture_graph(step, device, warmup=None):
    """`step()` captured into a HIP graph on a side stream of `device`; returns the torch.cuda.CUDAGraph (keep it alive, call its
    replay).  warmup: what runs once outside the capture in place of step() -- lazy set-up must not be captured, and an observer puts
    its store back there (`keeping`)."""
    import torch
    (warmup or step)()
    torch.cuda.synchronize(device)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            step()
    torch.cuda.current_stream(device).wait_stream(side)
    return g


def keeping(store, step):
    """A warm-up for capture_graph: step() with the device tensor `store` put back afterwards"""
    def run():
        keep = store.clone()
        step()
        store.copy_(keep)
    return run


def store_rows(plan, image_chw) -> List[dict]:
    """[{layer, C, H, W, first}] of a store: the input's channels ("row -1") first, then the plan's rows in order; first: the row's first
    record, its channels' records contiguous from there; an end-pool row is 1 x 1"""
    c, h, w = (int(v) for v in image_chw)
    rows, at = [dict(layer=-1, C=c, H=h, W=w, first=0)], c
    for L in plan:
        rows.append(dict(layer=L.index, C=int(L.N), H=1 if L.endpool else int(L.PH), W=1 if L.endpool else int(L.PW), first=at))
        at += int(L.N)
    return rows


def described_rows(plan, image_chw, slots: int) -> List[dict]:
    """What tf2_audit_describe / tf2_fid_describe report, from the plan alone (n_doubled is the packed image's business: None here)"""
    return [dict(layer=r["layer"], C=r["C"], H=r["H"], W=r["W"], offset=r["first"] * slots * 8, n_doubled=0 if r["layer"] < 0 else None)
            for r in store_rows(plan, image_chw)]


def listed(x, n=None) -> list:
    """A sequence as a list; a dict {row: value} as the list over rows 0 .. n - 1 (n None: up to its last key), None where a row is missing"""
    if isinstance(x, dict):
        keys = sorted(k for k in x if k >= 0)
        n = (keys[-1] + 1 if keys else 0) if n is None else n
        return [x.get(l) for l in range(n)]
    return list(x)


def checked_refs(rows, tensors, batch: int, device):
    """The host array of device pointers an observer's entry point reads at enqueue, one per row of `rows` ({C, H, W} or {C, HW}); tensors:
    a list in the rows' order or a dict {index: tensor}, each a contiguous float32 tensor [batch, C, H, W] ([batch, C] where H W = 1) on
    `device`, checked against its row; None or missing: a null pointer"""
    import ctypes as C
    import torch
    tensors = listed(tensors, len(rows))
    assert len(tensors) == len(rows), (len(tensors), len(rows))
    arr = (C.c_void_p * len(rows))()
    for i, (r, t) in enumerate(zip(rows, tensors)):
        if t is None:
            arr[i] = None
            continue
        _lib.expect(t, torch.float32, device=device)
        hw = r["HW"] if "HW" in r else r["H"] * r["W"]
        assert t.shape[0] == batch and t.shape[1] == r["C"] and t.numel() == batch * r["C"] * hw, (r, tuple(t.shape))
        arr[i] = t.data_ptr()
    return arr


class Handle:
    """tf2_<PREFIX>_create on a packed NetWork (no device needed): rows(), store_size.  A subclass names PREFIX ("audit" / "fid") and
    SLOTS, the int64 words of a record."""
    PREFIX = SLOTS = None

    def _fn(self, name: str):
        return getattr(_lib.lib(), f"tf2_{self.PREFIX}_{name}")

    def __init__(self, network):
        import ctypes as C
        self.net = network
        h = C.c_void_p()
        _lib.check(self._fn("create")(network._h, C.byref(h)))
        self._h = h
        self.store_size = int(self._fn("store_size")(h))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:                  # (None: the interpreter is shutting down)
            self._fn("destroy")(h)
            self._h = None

    def rows(self) -> List[dict]:
        """[{layer, C, H, W, offset (bytes), n_doubled}], row -1 first (tf2_<PREFIX>_describe)"""
        import ctypes as C
        cap = self.net.num_layer + 1
        arr = (_lib.AuditRow * cap)()
        n = C.c_int(0)
        _lib.check(self._fn("describe")(self._h, arr, cap, C.byref(n)))
        return [dict(layer=r.layer, C=r.C, H=r.H, W=r.W, offset=int(r.store_offset), n_doubled=r.n_doubled) for r in arr[:n.value]]


class DeviceObserver:
    """In front of a Handle subclass: the observer of a bound NetWork at one batch size.  Owns the keep_all workspace (_ws), the logits
    (_logits) and the int64 store (store_dev) as torch tensors; store=: the store tensor of another observer of the same network."""

    def __init__(self, network, batch: int, store=None):
        import torch
        super().__init__(network)
        self.batch = int(batch)
        dev = network.device
        ws = int(self._fn("workspace_size")(self._h, self.batch))
        self._ws = torch.empty(max(ws, 256), dtype=torch.uint8, device=dev)
        nbytes = int(_lib.lib().tf2_net_logits_size(network._h, self.batch))
        n_out = network.plan[-1].N
        self._logits = torch.empty((self.batch, n_out) if nbytes == self.batch * n_out else (self.batch, nbytes // (self.batch * n_out), n_out),
                                   dtype=torch.int8, device=dev)
        if store is None:
            self.store_dev = torch.empty(self.store_size // 8, dtype=torch.int64, device=dev)
            self.reset()
        else:
            assert store.dtype == torch.int64 and store.numel() * 8 >= self.store_size and store.device == dev
            self.store_dev = store

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.net.device).cuda_stream

    def reset(self) -> None:
        _lib.check(self._fn("store_init")(self._h, self.store_dev.data_ptr(), self.store_dev.numel() * 8, self._stream()))

    def _check_images(self, images, typed: bool = True) -> None:
        import torch
        assert images.is_contiguous() and images.device == self.net.device and (not typed or images.dtype in (torch.float32, torch.int8))
        assert images.shape[0] == self.batch, (images.shape, self.batch)

    def _capture(self, step, warm):
        g = capture_graph(step, self.net.device, keeping(self.store_dev, warm))
        self._graph = g
        return g.replay

    def store(self) -> np.ndarray:
        return self.store_dev.cpu().numpy()[:self.store_size // 8].reshape(-1, self.SLOTS).copy()
