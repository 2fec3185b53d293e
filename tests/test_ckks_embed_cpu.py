"""The CKKS encoder at N = 2^14 .. 2^16 without a device: the table of fhe_ckks_embed_twiddles against
`longdouble` and against fhe_ckks_twiddles, every rejection of the fhe_ckks_embed_* entry points that is answered before a
device is touched, the workspace rule, and the proofs of the case lists of tests/_ckks_embed_cases.py that
tests/test_ckks_embed_gpu.py compares the device with exactly."""
import os
import re

import numpy as np
import pytest

import _ckks_embed_cases as EC
import _ckks_numpy as K

INVALID, NULL = -9, -4


# ---- twiddles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1 << 14, 1 << 16])
def test_table_is_the_longdouble_table_rounded(pkg, n):
    got = pkg.binding.ckks_embed_twiddles(n)
    c, s = EC.roots_ld(n)
    assert np.array_equal(got.real, c.astype(np.float64)) and np.array_equal(got.imag, s.astype(np.float64))
    assert got[0] == 1 and got[n // 2] == 1j


@pytest.mark.parametrize("n", [2, 1 << 13])
def test_table_is_the_one_pass_table(pkg, n):
    a, b = pkg.binding.ckks_embed_twiddles(n), pkg.binding.ckks_twiddles(n)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_twiddle_rejections(pkg):
    L = pkg.load_library()
    buf = np.empty(16, dtype=np.complex128)
    for n in (0, 1, 3, 24, 1 << 17):
        assert L.fhe_ckks_embed_twiddles(n, buf.ctypes.data) == INVALID
    assert L.fhe_ckks_embed_twiddles(8, None) == NULL
    assert L.fhe_ckks_twiddles(1 << 14, buf.ctypes.data) == INVALID        # the one-pass entry point keeps its bound


# ---- the interface ------------------------------------------------------------------------------------------------------------
ENTRY = ("fhe_ckks_embed_twiddles", "fhe_ckks_embed_encode_dev", "fhe_ckks_embed_decode_dev")
A, B_, D = 1 << 30, 2 << 30, 3 << 30                                       # fake device addresses: every check below fails first


def test_header_binding_and_design_name_the_entry_points(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fhe_ntt.h")) as f:
        h = f.read()
    for name in ENTRY:
        assert re.search(r"\bint\s+" + name + r"\(", h) and name in pkg.binding.EXPORTS
    assert re.search(r"\bsize_t\s+fhe_ckks_embed_workspace_bytes\(", h) and "fhe_ckks_embed_workspace_bytes" in pkg.binding.EXPORTS
    with open(os.path.join(root, "DESIGN.md")) as f:
        assert re.search(r"^## 31\b", f.read(), re.M)


@pytest.mark.parametrize("n", [16, 1 << 14, 1 << 16])
def test_encoder_rejections_that_need_no_device(pkg, n):
    """the checks of fhe_ckks_encode_dev / _decode_dev in their order, at a one-pass and at two two-pass sizes"""
    L = pkg.load_library()
    h = n // 2
    enc = lambda **kw: L.fhe_ckks_embed_encode_dev(kw.get("n", n), kw.get("delta", 64.0), kw.get("tw", A), kw.get("z", B_), kw.get("stride", h), kw.get("out", D),
                                                   kw.get("batch", 2), None)
    dec = lambda **kw: L.fhe_ckks_embed_decode_dev(kw.get("n", n), kw.get("delta", 64.0), kw.get("tw", A), kw.get("p", B_), kw.get("out", D), kw.get("batch", 2), None)
    for f in (enc, dec):
        for bad in (0, 1, 3, 24, 1 << 17, 1 << 19):
            assert f(n=bad) == INVALID, bad
        for delta in (0.0, -1.0, float("inf"), float("nan")):
            assert f(delta=delta) == INVALID, delta
        assert f(tw=None) == NULL and f(out=None) == NULL and f(tw=A + 4) == INVALID and f(out=D + 4) == INVALID
        assert f(batch=1 << 58) == INVALID
        assert f(out=A) == INVALID and f(out=A - 8) == INVALID and f(out=B_) == INVALID     # the table and the input
        assert b"overlaps" in L.fhe_last_error()
        assert f(batch=0, tw=None, out=None) == 0 and f(batch=0, n=3) == INVALID and f(batch=0, n=1 << 17) == INVALID
    assert enc(z=None) == NULL and dec(p=None) == NULL and enc(z=B_ + 4) == INVALID
    assert enc(stride=h - 1) == INVALID and enc(stride=1 << 60) == INVALID
    assert enc(stride=0, z=D + 8 * n) == INVALID and enc(stride=0, z=D - 8) == INVALID
    # the one-pass entry points keep refusing the two-pass sizes
    assert L.fhe_ckks_encode_dev(1 << 14, 64.0, A, B_, 1 << 13, D, 2, None) == INVALID
    assert L.fhe_ckks_decode_dev(1 << 14, 64.0, A, B_, D, 2, None) == INVALID


def test_workspace_bytes(pkg):
    """0 for a refused shape and where no workspace is taken; otherwise the chunk's [n/2] complex rows, the chunk being
    2^21 words of polynomials as in the other CKKS calls"""
    W = pkg.binding.ckks_embed_workspace_bytes
    for n in (0, 1, 3, 24, 1 << 17, 2, 512, 1 << 13):
        assert W(n, 5) == 0, n
    for n in (1 << 14, 1 << 15, 1 << 16):
        chunk = (1 << 21) // n
        assert W(n, 0) == 0 and W(n, 1 << 58) == 0
        assert W(n, 1) == 8 * n and W(n, 3) == 3 * 8 * n
        assert W(n, chunk) == W(n, chunk + 1) == W(n, 10 * chunk) == 8 * n * chunk == 1 << 24


# ---- the restatement on the cached table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1 << 14, 1 << 16])
def test_cached_forms_are_the_restatement(n):
    """bit for bit, at the smallest and the largest size"""
    p, z = EC.exact_case(n)
    assert np.array_equal(z, K.decode(p, EC.DELTA)) and np.array_equal(EC.encode_pre(z, EC.DELTA), K.encode_pre(z, EC.DELTA))
    zr, want = EC.random_case(n)
    assert np.array_equal(want, K.encode(zr, EC.DELTA))


# ---- the case lists of the GPU module -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EC.SIZES)
def test_exact_construction_cases(n):
    """|encode_pre(z) - p| + E_enc(z) < 1/2 in every coefficient: a transform within E_enc of the restatement's rounds to p"""
    p, z = EC.exact_case(n)
    off = np.abs(EC.encode_pre(z, EC.DELTA) - p).max(axis=1)
    e = K.e_enc(z, EC.DELTA)
    print(f"\nN = {n}: pre-rounding value within {off.max():.3e} of p, E_enc {e.max():.3e}")
    assert (off + e < 0.5).all()


@pytest.mark.parametrize("n", EC.SIZES)
def test_random_cases_stay_away_from_half_integers(n):
    """every pre-rounding value is farther than E_enc from a half-integer: the restatement's rounding is the expected output"""
    z, want = EC.random_case(n)
    pre = EC.encode_pre(z, EC.DELTA)
    margin = np.abs(pre - np.floor(pre) - 0.5).min(axis=1)
    e = K.e_enc(z, EC.DELTA)
    print(f"\nN = {n}: nearest half-integer at {margin.min():.3e}, E_enc {e.max():.3e}")
    assert (margin > e).all() and np.array_equal(want, K.round_away(pre))
