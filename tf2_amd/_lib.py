"""ctypes binding of the C-ABI library (include/tf2_amd.h).

The product path FAILS LOUDLY when the HIP extension is missing: there is no CPU
fallback anywhere in tf2_amd (the CPU restatement lives in oracle/ and is test
infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# The library leaves the HIP runtime's hardware-queue count to the process environment: streams of one process share its
# queues, so batches in flight on several streams still run, with less overlap when there are fewer queues than streams
# (INTEGRATION.md "Deployment preconditions").
# TF2_AMD_LIB: another build of the same sources (the tools' -DTF2_PROBES / -DTF2_CHECK_DMA libraries); never a fallback, and refused
# unless the process also sets TF2_AMD_TOOL_LIB=1 (lib() below: a tool build can leave work out of a step)
LIB_PATH = os.environ.get("TF2_AMD_LIB") or os.path.join(_HERE, "libtf2amd.so")


class Tf2Error(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"tf2_amd status {status}: {msg}")
        self.status = status


class LayerDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "src", "q_in_row", "C", "H", "W", "N", "k", "stride", "pad_h", "pad_w", "dil", "OH", "OW",
        "bias_en", "bn_en", "relu", "ipool", "pool_en", "pool_S", "pool_st", "pool_pad", "PH", "PW",
        "add_src", "add_relu", "endpool", "endpool_mult", "concat", "n_start", "model_C", "model_k")]


class RunOpts(C.Structure):
    """tf2_run_opts (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("images_are_q", C.c_int32), ("concurrency", C.c_int32), ("mark_after_layer", C.c_int32),
                ("mark_event", C.c_void_p)]


class LaunchInfo(C.Structure):
    """tf2_launch_info (include/tf2_amd.h)."""
    _fields_ = [("layer", C.c_int32), ("grid", C.c_int32), ("block", C.c_int32), ("lds_bytes", C.c_int32), ("vgprs", C.c_int32),
                ("kernel", C.c_char * 96)]


class TensorInfo(C.Structure):
    """tf2_tensor_info (include/tf2_amd.h)."""
    _fields_ = [("offset", C.c_int64), ("bytes", C.c_int64), ("first_row", C.c_int32), ("last_row", C.c_int32)]


class RowTensors(C.Structure):
    """tf2_row_tensors (include/tf2_amd.h)."""
    _fields_ = [("in_tensor", C.c_int32), ("out_tensor", C.c_int32), ("conv_tensor", C.c_int32), ("res_tensor", C.c_int32)]


class SsdDesc(C.Structure):
    """tf2_ssd_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("num_classes", C.c_int32), ("top_k", C.c_int32), ("conf_thresh", C.c_float),
                ("nms_thresh", C.c_float), ("variance", C.c_float * 2), ("n_sources", C.c_int32), ("loc_row", C.c_int32 * 8),
                ("conf_row", C.c_int32 * 8), ("priors", C.c_void_p), ("n_priors", C.c_int32)]


class ImageSrc(C.Structure):
    """tf2_image_src (include/tf2_amd.h): one per image, in device memory."""
    _fields_ = [("offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("row_pitch", C.c_int32), ("resize_h", C.c_int32),
                ("resize_w", C.c_int32), ("crop_y", C.c_int32), ("crop_x", C.c_int32), ("reserved", C.c_int32)]


class PreprocessDesc(C.Structure):
    """tf2_preprocess_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("pixel_bytes", C.c_int32), ("src_channel", C.c_int32 * 3), ("round_resized", C.c_int32),
                ("mean", C.c_float * 3), ("scale", C.c_float * 3)]


class Roi(C.Structure):
    """tf2_roi (include/tf2_amd.h): one slot of the ROI table, in device memory."""
    _fields_ = [("image", C.c_int32), ("cls", C.c_int32), ("rank", C.c_int32), ("score", C.c_float), ("x0", C.c_float),
                ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float)]


class RoiDesc(C.Structure):
    """tf2_roi_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("num_classes", C.c_int32), ("top_k", C.c_int32), ("class_mask", C.c_uint32 * 8),
                ("min_score", C.c_float), ("max_rois", C.c_int32), ("expand_w", C.c_float), ("expand_h", C.c_float),
                ("square", C.c_int32), ("clip", C.c_int32)]


class RoiXform(C.Structure):
    """tf2_roi_xform (include/tf2_amd.h): one slot of the transform table, in device memory."""
    _fields_ = [("image", C.c_int32), ("reserved", C.c_int32), ("m", C.c_double * 6)]


class RoiFitDesc(C.Structure):
    """tf2_roi_fit_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("n_points", C.c_int32), ("tpl", (C.c_float * 2) * 16), ("space", C.c_int32)]


class YccSrc(C.Structure):
    """tf2_ycc_src (include/tf2_amd.h): the planes of one image, in device memory."""
    _fields_ = [("off_y", C.c_int64), ("off_cb", C.c_int64), ("off_cr", C.c_int64), ("pitch_y", C.c_int32), ("pitch_c", C.c_int32)]


class YccDesc(C.Structure):
    """tf2_ycc_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("layout", C.c_int32), ("sub_x", C.c_int32), ("sub_y", C.c_int32), ("upsample", C.c_int32),
                ("matrix", C.c_int32), ("pixel_bytes", C.c_int32), ("dst_channel", C.c_int32 * 3), ("alpha", C.c_int32),
                ("blocks_per_image", C.c_int32)]


class JpegInfo(C.Structure):
    """tf2_jpeg_info (include/tf2_amd.h): what tf2_jpeg_parse reads from a file's headers."""
    _fields_ = [("status", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("components", C.c_int32), ("sub_x", C.c_int32),
                ("sub_y", C.c_int32), ("restart_interval", C.c_int32), ("upsample", C.c_int32), ("bw", C.c_int32 * 3),
                ("bh", C.c_int32 * 3), ("ph", C.c_int32 * 3), ("pw", C.c_int32 * 3), ("total_blocks", C.c_int64),
                ("scan_offset", C.c_int64), ("quant", (C.c_uint16 * 64) * 3)]


class JpegSrc(C.Structure):
    """tf2_jpeg_src (include/tf2_amd.h): the coefficient blocks of one image, in device memory."""
    _fields_ = [("block_off", C.c_int64 * 3), ("bw", C.c_int32 * 3), ("bh", C.c_int32 * 3)]


class JpegScanTab(C.Structure):
    _fields_ = [("dc_counts", C.c_uint8 * 16), ("dc_vals", C.c_uint8 * 256), ("ac_counts", C.c_uint8 * 16), ("ac_vals", C.c_uint8 * 256)]


class JpegScan(C.Structure):
    """tf2_jpeg_scan (include/tf2_amd.h): where a file's entropy-coded bytes lie and its Huffman tables, in device memory."""
    _fields_ = [("byte_off", C.c_int64), ("byte_len", C.c_int64), ("components", C.c_int32), ("sub_x", C.c_int32), ("sub_y", C.c_int32),
                ("restart_interval", C.c_int32), ("tab", JpegScanTab * 3)]


class JpegHuffDesc(C.Structure):
    """tf2_jpeg_huff_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("layout", C.c_int32), ("sub_x", C.c_int32), ("sub_y", C.c_int32), ("subseq_bytes", C.c_int32)]


class JpegDesc(C.Structure):
    """tf2_jpeg_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("layout", C.c_int32), ("sub_x", C.c_int32), ("sub_y", C.c_int32), ("blocks_per_image", C.c_int32)]


class EmbDesc(C.Structure):
    """tf2_emb_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("top_k", C.c_int32)]


class ClsDesc(C.Structure):
    """tf2_cls_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("top_k", C.c_int32)]


class AuditRow(C.Structure):
    """tf2_audit_row (include/tf2_amd.h)."""
    _fields_ = [("layer", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("store_offset", C.c_int64),
                ("n_doubled", C.c_int32), ("reserved", C.c_int32)]


class CaqRow(C.Structure):
    """tf2_caq_row (include/tf2_amd.h): a row of dense float32 [batch][C][HW] and its first record."""
    _fields_ = [("C", C.c_int32), ("HW", C.c_int32), ("first_record", C.c_int64)]


class InqSeg(C.Structure):
    """tf2_inq_seg (include/tf2_amd.h): a tensor of the flat weight buffer, in elements."""
    _fields_ = [("offset", C.c_int64), ("count", C.c_int64)]


class DnscpConv(C.Structure):
    """tf2_dnscp_conv (include/tf2_amd.h): a conv [N][C][kk] of the flat weight buffer, in elements."""
    _fields_ = [("offset", C.c_int64), ("N", C.c_int32), ("C", C.c_int32), ("kk", C.c_int32), ("flags", C.c_int32),
                ("keep_offset", C.c_int64), ("t_lo", C.c_double), ("t_hi", C.c_double)]


class DnscpSeg(C.Structure):
    """tf2_dnscp_seg (include/tf2_amd.h): a tensor of the pruned stream and where it comes from."""
    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("n_src", C.c_int32), ("c_src", C.c_int32), ("n_out", C.c_int32),
                ("c_out", C.c_int32), ("kk", C.c_int32), ("reserved", C.c_int32), ("n_idx", C.c_int64), ("c_idx", C.c_int64)]


class DetEvalDesc(C.Structure):
    """tf2_det_eval_desc (include/tf2_amd.h)."""
    _fields_ = [("size", C.c_uint32), ("num_classes", C.c_int32), ("top_k", C.c_int32), ("max_gt", C.c_int32),
                ("capacity", C.c_int32), ("iou_thresh", C.c_float)]


class DetEvalClass(C.Structure):
    """tf2_det_eval_class (include/tf2_amd.h)."""
    _fields_ = [("ap", C.c_double), ("npos", C.c_int64), ("tp", C.c_int64), ("fp", C.c_int64)]


class NetDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_layers", "n_conv", "n_q_rows", "max_out_channel", "image_c", "image_h", "image_w",
        "conv1_rewrite", "n_concat")]


def build(force: bool = False) -> str:
    """Compile tf2_amd/libtf2amd.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if f.endswith((".hip", ".cpp", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "tf2_amd.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", src_dir])
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension was not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C tf2_amd/csrc`). tf2_amd has no CPU fallback by design.")
    # The HIP runtime of the process must be ONE: PyTorch-ROCm ships its own libamdhip64, and libtf2amd.so loaded BEFORE torch binds the
    # system copy under /opt/rocm instead -- a later torch import then brings the second runtime, and the library's first launch reports
    # "no ROCm-capable device is detected" (seen with build() + smoke() in one process, round 6).  Loading torch first makes the
    # dynamic loader resolve libtf2amd.so's HIP symbols against the runtime torch loaded.  (Hosts without torch -- the C++ shim of
    # INTEGRATION.md section 3 -- link one runtime anyway.)
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    L.tf2_build_kind.restype = C.c_int
    kind = L.tf2_build_kind()
    if kind != 0 and os.environ.get("TF2_AMD_TOOL_LIB") != "1":
        raise ImportError(f"{LIB_PATH} is a TOOL build of the library (tf2_build_kind() = {kind}: 1 timing probes, 2 DMA check), not the "
                          "product; tools that want it set TF2_AMD_TOOL_LIB=1 next to TF2_AMD_LIB")
    vp, sz, i32p, i8p, u8p, fp = C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int8), C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    L.tf2_last_error.restype = C.c_char_p
    L.tf2_abi_version.restype = C.c_int
    L.tf2_has_device_code.restype = C.c_int
    L.tf2_get_real.restype = C.c_uint8
    L.tf2_get_real.argtypes = [C.c_float, C.c_int8]
    L.tf2_net_create.argtypes = [C.POINTER(NetDesc), C.POINTER(LayerDesc), C.POINTER(vp)]
    L.tf2_net_destroy.argtypes = [vp]
    L.tf2_net_destroy.restype = None
    L.tf2_quantization.argtypes = [vp, C.c_char_p, sz, vp, sz, i32p]
    L.tf2_net_set_q.argtypes = [vp, vp, sz]
    L.tf2_net_load_model.argtypes = [vp, vp, sz]
    L.tf2_model4bit_decode.argtypes = [vp, sz, vp, sz, vp]
    L.tf2_net_load_model_4bit.argtypes = [vp, vp, sz]
    L.tf2_net_get_codes.argtypes = [vp, C.c_int, vp, sz, C.POINTER(sz)]
    L.tf2_net_get_bias_bn.argtypes = [vp, C.c_int, vp, vp, vp, sz]
    L.tf2_net_pack.argtypes = [vp, C.c_int]
    L.tf2_net_packed_size.argtypes = [vp]
    L.tf2_net_packed_size.restype = sz
    L.tf2_net_packed_copy.argtypes = [vp, vp, sz]
    L.tf2_net_packed_adopt.argtypes = [vp, vp, sz]
    L.tf2_net_bind_device.argtypes = [vp, vp, sz]
    L.tf2_net_workspace_size.argtypes = [vp, C.c_int, C.c_int]
    L.tf2_net_workspace_size.restype = sz
    L.tf2_net_logits_size.argtypes = [vp, C.c_int]
    L.tf2_net_logits_size.restype = sz
    L.tf2_net_reload_options.argtypes = [vp]
    L.tf2_net_run.argtypes = [vp, vp, C.c_int, vp, sz, vp, vp]
    L.tf2_net_run_q.argtypes = [vp, vp, C.c_int, vp, sz, vp, vp]
    L.tf2_net_run_ex.argtypes = [vp, vp, C.c_int, vp, sz, vp, vp, C.POINTER(RunOpts)]
    L.tf2_net_run_stats.argtypes = [vp, vp]
    L.tf2_net_poll_error.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    L.tf2_net_describe_launches.argtypes = [vp, C.c_int, C.c_int, C.POINTER(LaunchInfo), C.c_int, C.POINTER(C.c_int)]
    L.tf2_net_describe_workspace.argtypes = [vp, C.c_int, C.c_int, C.POINTER(TensorInfo), C.c_int, C.POINTER(C.c_int), C.POINTER(RowTensors), C.c_int]
    L.tf2_net_read_layer.argtypes = [vp, C.c_int, C.c_int, vp, vp, sz, vp]
    L.tf2_net_profile.argtypes = [vp, C.c_int]
    L.tf2_net_profile_read.argtypes = [vp, vp, vp, vp, C.c_int]
    L.tf2_net_profile_loop_read.argtypes = [vp, vp, vp]
    L.tf2_topk.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    L.tf2_ssd_create.argtypes = [vp, C.POINTER(SsdDesc), C.POINTER(vp)]
    L.tf2_ssd_destroy.argtypes = [vp]
    L.tf2_ssd_destroy.restype = None
    L.tf2_ssd_workspace_size.argtypes = [vp, C.c_int]
    L.tf2_ssd_workspace_size.restype = sz
    L.tf2_ssd_detect_scratch_size.argtypes = [vp, C.c_int]
    L.tf2_ssd_detect_scratch_size.restype = sz
    L.tf2_ssd_run.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.tf2_ssd_detect.argtypes = [vp, vp, vp, C.c_int, vp, sz, vp, vp, vp]
    L.tf2_preprocess.argtypes = [vp, C.POINTER(PreprocessDesc), vp, sz, vp, C.c_int, C.c_int, vp, vp, vp]
    L.tf2_preprocess_aa.argtypes = L.tf2_preprocess.argtypes
    L.tf2_roi_select.argtypes = [C.POINTER(RoiDesc), vp, vp, vp, C.c_int, vp, vp, vp]
    L.tf2_roi_crop.argtypes = [vp, C.POINTER(PreprocessDesc), vp, sz, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp]
    L.tf2_roi_crop_aa.argtypes = L.tf2_roi_crop.argtypes
    L.tf2_roi_fit.argtypes = [C.POINTER(RoiFitDesc), vp, vp, C.c_int, vp, vp, vp]
    L.tf2_roi_warp.argtypes = L.tf2_roi_crop.argtypes
    L.tf2_ycc_to_rgb.argtypes = [C.POINTER(YccDesc), vp, sz, vp, vp, sz, vp, C.c_int, vp, vp]
    L.tf2_jpeg_parse.argtypes = [vp, sz, C.POINTER(JpegInfo)]
    L.tf2_jpeg_entropy.argtypes = [vp, sz, C.POINTER(JpegInfo), vp, sz, i32p]
    L.tf2_jpeg_idct.argtypes = [C.POINTER(JpegDesc), vp, sz, vp, vp, vp, sz, vp, vp, C.c_int, vp, vp]
    L.tf2_jpeg_scan_fill.argtypes = [vp, sz, C.POINTER(JpegInfo), C.c_int64, C.POINTER(JpegScan)]
    L.tf2_jpeg_huff_work_bytes.argtypes = [C.POINTER(JpegHuffDesc), C.c_int, sz]
    L.tf2_jpeg_huff_work_bytes.restype = sz
    L.tf2_jpeg_huff.argtypes = [C.POINTER(JpegHuffDesc), vp, sz, vp, vp, vp, sz, vp, sz, C.c_int, vp, vp]
    L.tf2_cls_create.argtypes = [vp, C.POINTER(ClsDesc), C.POINTER(vp)]
    L.tf2_cls_destroy.argtypes = [vp]
    L.tf2_cls_destroy.restype = None
    L.tf2_cls_run.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tf2_emb_create.argtypes = [vp, C.POINTER(EmbDesc), C.POINTER(vp)]
    L.tf2_emb_destroy.argtypes = [vp]
    L.tf2_emb_destroy.restype = None
    L.tf2_emb_scratch_size.argtypes = [vp, C.c_int, C.c_int]
    L.tf2_emb_scratch_size.restype = sz
    L.tf2_emb_embed.argtypes = [vp, vp, C.c_int, vp, vp]
    L.tf2_emb_match.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.tf2_emb_roc_hist.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]
    L.tf2_emb_roc_pairs.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp]
    L.tf2_det_eval_create.argtypes = [C.POINTER(DetEvalDesc), C.POINTER(vp)]
    L.tf2_det_eval_destroy.argtypes = [vp]
    L.tf2_det_eval_destroy.restype = None
    L.tf2_det_eval_store_size.argtypes = [vp]
    L.tf2_det_eval_store_size.restype = sz
    L.tf2_det_eval_store_init.argtypes = [vp, vp, sz, vp]
    L.tf2_det_eval_run.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, sz, vp, vp, vp]
    L.tf2_det_eval_summarise.argtypes = [vp, vp, sz, C.c_int, C.POINTER(DetEvalClass), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.tf2_audit_create.argtypes = [vp, C.POINTER(vp)]
    L.tf2_audit_destroy.argtypes = [vp]
    L.tf2_audit_destroy.restype = None
    L.tf2_audit_store_size.argtypes = [vp]
    L.tf2_audit_store_size.restype = sz
    L.tf2_audit_describe.argtypes = [vp, C.POINTER(AuditRow), C.c_int, C.POINTER(C.c_int)]
    L.tf2_audit_store_init.argtypes = [vp, vp, sz, vp]
    L.tf2_audit_workspace_size.argtypes = [vp, C.c_int]
    L.tf2_audit_workspace_size.restype = sz
    L.tf2_audit_run.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz, vp, vp, sz, vp]
    L.tf2_audit_kept.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz, vp, sz, vp]
    L.tf2_fid_create.argtypes = [vp, C.POINTER(vp)]
    L.tf2_fid_destroy.argtypes = [vp]
    L.tf2_fid_destroy.restype = None
    L.tf2_fid_store_size.argtypes = [vp]
    L.tf2_fid_store_size.restype = sz
    L.tf2_fid_describe.argtypes = [vp, C.POINTER(AuditRow), C.c_int, C.POINTER(C.c_int)]
    L.tf2_fid_scales.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    L.tf2_fid_store_init.argtypes = [vp, vp, sz, vp]
    L.tf2_fid_workspace_size.argtypes = [vp, C.c_int]
    L.tf2_fid_workspace_size.restype = sz
    L.tf2_fid_run.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz, vp, C.POINTER(vp), vp, vp, sz, vp]
    L.tf2_fid_kept.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz, C.POINTER(vp), vp, vp, sz, vp]
    L.tf2_caq_range_store_size.argtypes = [C.c_int64]
    L.tf2_caq_range_store_size.restype = sz
    L.tf2_caq_error_store_size.argtypes = [C.c_int64]
    L.tf2_caq_error_store_size.restype = sz
    L.tf2_caq_store_init.argtypes = [vp, sz, vp]
    L.tf2_caq_range.argtypes = [C.POINTER(CaqRow), C.POINTER(vp), C.c_int, C.c_int, vp, sz, vp]
    L.tf2_caq_error.argtypes = [C.POINTER(CaqRow), C.POINTER(vp), C.c_int, C.c_int, vp, vp, sz, vp]
    L.tf2_inq_scratch_size.argtypes = [C.c_int]
    L.tf2_inq_scratch_size.restype = sz
    L.tf2_inq_state_size.argtypes = [C.c_int]
    L.tf2_inq_state_size.restype = sz
    L.tf2_inq_step.argtypes = [vp, vp, C.c_int64, C.POINTER(InqSeg), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, vp, vp, vp, sz, vp]
    L.tf2_dnscp_state_size.argtypes = [C.c_int]
    L.tf2_dnscp_state_size.restype = sz
    L.tf2_dnscp_scratch_size.argtypes = [C.c_int]
    L.tf2_dnscp_scratch_size.restype = sz
    L.tf2_dnscp_stats.argtypes = [vp, C.c_int64, C.POINTER(DnscpConv), C.c_int, vp, C.c_int64, vp, vp, vp, sz, vp]
    L.tf2_dnscp_step.argtypes = [vp, vp, C.c_int64, C.POINTER(DnscpConv), C.c_int, vp, C.c_int64, vp, vp, vp, sz, vp]
    L.tf2_dnscp_compact.argtypes = [vp, C.c_int64, vp, C.c_int64, C.POINTER(DnscpSeg), C.c_int, vp, C.c_int64, vp]
    _lib = L
    return L


EXPORTED = [
    "tf2_last_error", "tf2_abi_version", "tf2_has_device_code", "tf2_build_kind", "tf2_get_real", "tf2_quantization",
    "tf2_net_create", "tf2_net_destroy", "tf2_net_set_q", "tf2_net_load_model", "tf2_model4bit_decode", "tf2_net_load_model_4bit", "tf2_net_get_codes",
    "tf2_net_get_bias_bn", "tf2_net_pack", "tf2_net_packed_size", "tf2_net_packed_copy",
    "tf2_net_packed_adopt", "tf2_net_bind_device", "tf2_net_workspace_size", "tf2_net_logits_size", "tf2_net_reload_options", "tf2_net_run",
    "tf2_net_run_q", "tf2_net_run_ex", "tf2_net_run_stats", "tf2_net_poll_error", "tf2_net_describe_launches", "tf2_net_describe_workspace", "tf2_net_read_layer", "tf2_net_profile", "tf2_net_profile_read", "tf2_net_profile_loop_read", "tf2_topk",
    "tf2_ssd_create", "tf2_ssd_destroy", "tf2_ssd_workspace_size", "tf2_ssd_detect_scratch_size", "tf2_ssd_run", "tf2_ssd_detect",
    "tf2_preprocess", "tf2_preprocess_aa", "tf2_roi_select", "tf2_roi_crop", "tf2_roi_crop_aa", "tf2_roi_fit", "tf2_roi_warp", "tf2_ycc_to_rgb", "tf2_jpeg_parse", "tf2_jpeg_entropy", "tf2_jpeg_idct", "tf2_jpeg_scan_fill", "tf2_jpeg_huff_work_bytes", "tf2_jpeg_huff", "tf2_cls_create", "tf2_cls_destroy", "tf2_cls_run",
    "tf2_det_eval_create", "tf2_det_eval_destroy", "tf2_det_eval_store_size", "tf2_det_eval_store_init", "tf2_det_eval_run",
    "tf2_det_eval_summarise",
    "tf2_emb_create", "tf2_emb_destroy", "tf2_emb_scratch_size", "tf2_emb_embed", "tf2_emb_match",
    "tf2_emb_roc_hist", "tf2_emb_roc_pairs",
    "tf2_audit_create", "tf2_audit_destroy", "tf2_audit_store_size", "tf2_audit_describe", "tf2_audit_store_init",
    "tf2_audit_workspace_size", "tf2_audit_run", "tf2_audit_kept",
    "tf2_fid_create", "tf2_fid_destroy", "tf2_fid_store_size", "tf2_fid_describe", "tf2_fid_scales", "tf2_fid_store_init",
    "tf2_fid_workspace_size", "tf2_fid_run", "tf2_fid_kept",
    "tf2_caq_range_store_size", "tf2_caq_error_store_size", "tf2_caq_store_init", "tf2_caq_range", "tf2_caq_error",
    "tf2_inq_scratch_size", "tf2_inq_state_size", "tf2_inq_step",
    "tf2_dnscp_state_size", "tf2_dnscp_scratch_size", "tf2_dnscp_stats", "tf2_dnscp_step", "tf2_dnscp_compact"]


def parse_opts(text: str) -> dict:
    """TF2_AMD_OPTS text -> {name: value} exactly as csrc/opts.cpp reads it: items separated by ',', ';' or ' ', a bare name means
    name=1.  (An empty value, 'name=', is an error on the C side; it is kept here so that the library reports it.)"""
    cur = {}
    for item in re.split(r"[,; ]", text or ""):
        if not item:
            continue
        name, eq, val = item.partition("=")
        cur[name] = val if eq else "1"
    return cur


def set_opts(**kw) -> None:
    """Tools: set / change / remove (value None) options of TF2_AMD_OPTS (csrc/opts.h) in this process's environment, cumulatively, and
    admit the test-only ones (TF2_AMD_TEST=1).  Takes effect at the next tf2_net_create / NetWork.reload_options()."""
    cur = parse_opts(os.environ.get("TF2_AMD_OPTS", ""))
    for k, v in kw.items():
        if v is None:
            cur.pop(k, None)
        else:
            cur[k] = str(v)
    os.environ["TF2_AMD_TEST"] = "1"
    os.environ["TF2_AMD_OPTS"] = ",".join(f"{k}={v}" for k, v in cur.items())


def check(status: int) -> None:
    if status != 0:
        raise Tf2Error(status, lib().tf2_last_error().decode("utf-8", "replace"))


def expect(t, dtype, shape=None, device=None, cols=None, ndim=None):
    """A device tensor an entry point is about to hand to the library: `dtype`, contiguous, on `device` (None: any GPU -- the call's
    first tensor, whose device the others are held to), with exactly `shape`, or two-dimensional with `cols` columns, or of `ndim`
    dimensions.  AssertionError naming what it got; returns the tensor's device."""
    ok = t.dtype == dtype and t.is_contiguous() and (t.device.type == "cuda" if device is None else t.device == device)
    ok = ok and (shape is None or tuple(t.shape) == tuple(shape)) and (cols is None or (t.dim() == 2 and t.shape[1] == cols))
    want = tuple(shape) if shape is not None else f"[n, {cols}]" if cols is not None else f"{ndim}-d" if ndim is not None else ""
    assert ok and (ndim is None or t.dim() == ndim), f"expected {dtype} {want} contiguous on {device or 'a GPU'}, got {t.dtype} " \
        f"{tuple(t.shape)} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}"
    return t.device
