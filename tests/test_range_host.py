"""CPU check of the DEVICE header orp_range.hpp: the range rule of the fp16-pieces contractions (one power of two per operand
tensor puts its largest magnitude into [2^14, 2^15); the accumulator is scaled back by 2^-(kx + kw)).  g++ compiles the same
inline functions hipcc compiles for gfx950; the `-m gpu` twin is tests/test_gpu_fp16_pieces_range.py, which runs the kernels
that use them against float64 at the same edges (non-finite elements, tiny and huge operands)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "range_host.cpp")

FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.finfo(np.float32).tiny)                      # 2^-126, the smallest normal
SUB = float(np.float32(2.0 ** -149))                        # the smallest subnormal


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("range_host") / "librange_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.host_range_bits.restype = ctypes.c_uint32
    L.host_range_bits.argtypes = [ctypes.c_float]
    L.host_range_bound_bits.restype = ctypes.c_uint32
    L.host_range_bound_bits.argtypes = [ctypes.c_float]
    L.host_range_exp.restype = ctypes.c_int
    L.host_range_exp.argtypes = [ctypes.c_uint32]
    L.host_range_scale.restype = ctypes.c_float
    L.host_range_scale.argtypes = [ctypes.c_int]
    L.host_range_exp_of.restype = ctypes.c_int
    L.host_range_exp_of.argtypes = [ctypes.c_float]
    L.host_range_unscale.restype = ctypes.c_float
    L.host_range_unscale.argtypes = [ctypes.c_float, ctypes.c_int]
    L.host_range_rule_violations.restype = ctypes.c_long
    L.host_range_rule_violations.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return L


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_rule_for_every_exponent_both_signs(harness):
    """Every float bit pattern with a stride of 97 (all 256 exponent fields, both signs, subnormals, Inf and the NaN payloads):
    range word = |v| (0 for Inf / NaN), k in [-126, 127], and 2^k |v| in [2^14, 2^15) wherever that power of two is a normal
    float -- below 2^-113 the clamp k = 127 leaves it under 2^14."""
    first = ctypes.c_uint32(0)
    bad = harness.host_range_rule_violations(0, 0xffffffff, 97, ctypes.byref(first))
    assert bad == 0, "first violation at bits 0x%08x" % first.value


def test_rule_at_every_exponent_edge(harness):
    """The first and last mantissa of every exponent field, exhaustively."""
    first = ctypes.c_uint32(0)
    for e in range(256):
        for sign in (0, 0x80000000):
            for m in (0, 1, 0x400000, 0x7ffffe, 0x7fffff):
                b = sign | (e << 23) | m
                assert harness.host_range_rule_violations(b, b, 1, ctypes.byref(first)) == 0, hex(b)


def test_named_values(harness):
    nan_neg = np.array([0xffc00000], np.uint32).view(np.float32)[0]
    for v in (0.0, -0.0, float("inf"), float("-inf"), float("nan"), float(nan_neg)):
        assert harness.host_range_bits(v) == 0
    assert harness.host_range_exp(0) == 0
    for word in (0x7f800000, 0x7fc00000, 0xffc00000, 0xff800000):      # non-finite words: no producer leaves one; scale 1
        assert harness.host_range_exp(word) == 0
    assert harness.host_range_bits(-3.5) == _bits(3.5)
    assert harness.host_range_exp(_bits(FLT_MAX)) == 14 - 127               # the largest finite float: 2^-113, no clamp
    assert harness.host_range_exp(_bits(1.0)) == 14
    assert harness.host_range_exp(_bits(32767.0)) == 0
    assert harness.host_range_exp(_bits(2.0 ** -113)) == 127                # the smallest unclamped maximum
    assert harness.host_range_exp(_bits(2.0 ** -114)) == 127                # (clamped from here on down)
    for v in (TINY, SUB, 2.0 ** -130):
        assert harness.host_range_exp(_bits(v)) == 127
    for k in (-126, -113, -1, 0, 1, 100, 127):
        s = harness.host_range_scale(k)
        assert s == 2.0 ** k and harness.host_range_exp_of(s) == k


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_unscale_is_one_rounding_where_the_old_reciprocal_overflowed(harness):
    """x max ~ 2^-80 and w ~ 2^-40 give kx + kw = 94 + 54 = 148: 1 / (2^94 2^54) is 0 in float, the product result (~1e-34) a
    normal float.  ldexp(acc, -148) is the correctly rounded acc x 2^-148, also into the subnormal range."""
    kx = harness.host_range_exp(_bits(2.0 ** -80))
    kw = harness.host_range_exp(_bits(2.0 ** -40))
    assert (kx, kw) == (94, 54)
    assert np.float32(1.0) / (np.float32(2.0 ** kx) * np.float32(2.0 ** kw)) == 0.0          # what the old back-scale did
    rng = np.random.RandomState(3)
    for acc in list(rng.uniform(-2 ** 30, 2 ** 30, 200).astype(np.float32)) + [np.float32(2.0 ** 29 * 1.75), np.float32(-3.0)]:
        for k in (0, 20, 148, 200, 254, -20, -226):
            got = harness.host_range_unscale(float(acc), k)
            want = np.float32(np.ldexp(np.float64(acc), -k))                 # exact in double, one rounding to float
            assert np.float32(got).view(np.uint32) == want.view(np.uint32), (float(acc), k)
    # inside the old clamp, bits equal to the power-of-two multiply it replaces
    for acc in rng.normal(size=200).astype(np.float32):
        for kx, kw in ((14, 14), (100, -60), (-100, 27), (60, 60)):
            osc = np.float32(1.0) / (np.float32(2.0 ** kx) * np.float32(2.0 ** kw))
            assert np.float32(harness.host_range_unscale(float(acc), kx + kw)).view(np.uint32) == (acc * osc).view(np.uint32)


def test_bound_bits(harness):
    """The GroupNorm bound: a hair above a finite bound, 0 for a NaN / Inf bound (a negative NaN's bits would win every
    atomicMax), FLT_MAX when the hair overflows."""
    assert harness.host_range_bound_bits(2.0) == _bits(np.float32(2.0) * np.float32(1.0001))
    assert harness.host_range_bound_bits(0.0) == 0
    for v in (float("nan"), float("inf"), float("-inf"), float(np.array([0xffc00000], np.uint32).view(np.float32)[0])):
        assert harness.host_range_bound_bits(v) == 0
    assert harness.host_range_bound_bits(FLT_MAX) == _bits(FLT_MAX)
