"""Cross-check of the oracle against the reference's compiled host functions and PE arithmetic, through the committed
golden vectors tests/golden/ref_oracle_vs_ref.npz: seeded fuzz inputs and what oracle/_ref/libtf2ref_resnet50.so and
oracle/_ref/libtf2ref_pe.so (built by oracle/Makefile from the reference sources) returned for them (oracle/gen_golden.py
gen_oracle_vs_ref)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O


@pytest.fixture(scope="module")
def R(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_oracle_vs_ref.npz"))


def test_get_real_fuzz(R):
    vals, exps, want = R["get_real_w"], R["get_real_e"], R["get_real_out"]
    assert vals.size == exps.size == want.size == 6000
    for v, e, r in zip(vals, exps, want):
        assert O.get_real(v, int(e)) == int(r), (float(v), int(e))


def test_filter_trans_fuzz(R):
    planes, wants = R["filter_trans_in"], R["filter_trans_out"]
    assert planes.shape == (50, 49) and wants.shape == (50, 81)
    for plane, want in zip(planes, wants):
        plane = np.ascontiguousarray(plane)
        got = np.zeros(81, np.uint8)
        O.lib().tf2o_filter_trans(plane.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p))
        np.testing.assert_array_equal(got, want)


def test_feature_trans_fuzz(R):
    plane = np.ascontiguousarray(R["feature_trans_in"], dtype=np.float32)
    want = R["feature_trans_out"]
    assert plane.size == 224 * 224 and want.shape == (9, 114, 114)
    got = np.empty((9, 114, 114), np.float32)
    O.lib().tf2o_feature_trans(plane.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p))
    np.testing.assert_array_equal(got, want)


# ---- the device code's PE arithmetic (pe.cl:27-49), compiled in place as C (oracle/ref_pe_probe.c, oracle/Makefile `ref`) ----


def test_pe_mul_every_feature_and_code(R):
    """tf2o_mul == the reference's own MUL (pe.cl:27-40) on ALL 256 x 256 (feature, filter code) pairs: the zero flag (bit 6), the sign flag
    with the -128 quirk ((int8)(-x) keeps -128), five-bit shifts up to 31 with the int32 wrap of `feature << filter`."""
    pe_mul = R["pe_mul"]                                     # [x + 128][code]
    assert pe_mul.shape == (256, 256)
    for x in range(-128, 128):
        for code in range(256):
            assert O.mul(x, code) == pe_mul[x + 128, code], (x, hex(code))
    assert pe_mul[0, 0x83] == -1024 == pe_mul[0, 0x03] and pe_mul[255, 0x14] == 133169152


def test_pe_dot_product_and_conv_core(R):
    """The reference's DotProduct (pe.cl:42-49: C_VECTOR = 16 MULs summed in an int, i.e. mod 2^32) against the oracle's convolution core on
    the same 16 channels (a 1x1 layer of one output channel, bias 0): random vectors, and vectors built to overflow int32 (shift 31 / 30
    codes on +-127 / -128 features)."""
    assert int(R["pe_c_vector"]) == 16
    xs, cs, refs = R["pe_dot_x"], R["pe_dot_codes"], R["pe_dot_out"]
    assert xs.shape == cs.shape == (3000, 16) and refs.shape == (3000,)
    for trial, (x, codes, ref) in enumerate(zip(xs, cs, refs)):
        ref = int(ref)
        acc = O.conv(x.reshape(16, 1, 1), codes.reshape(1, 16, 1, 1), np.zeros(1, np.int32))
        assert int(acc.reshape(-1)[0]) == ref, (trial, x.tolist(), codes.tolist())
