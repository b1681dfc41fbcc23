"""roi_warp.hip's kernels compile without scratch: the listing of the shipped source with the shipped flags (Makefile target `isa`)
has a private segment of 0 for tf2_roi_fit's kernel and for the four instantiations of tf2_roi_warp's."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vmcnt_check  # noqa: E402


def test_roi_warp_kernels_use_no_private_segment():
    seg, lds, txt = vmcnt_check.kernel_segments("roi_warp")
    assert sum("roi_fit_kernel" in k for k in seg) == 1 and sum("roi_warp_kernel" in k for k in seg) == 4, seg   # int8 / float32 x vector / scalar stores
    assert len(seg) == 5 and all(v == 0 for v in seg.values()), seg
