"""CKKS of DESIGN.md §21 without a device: the twiddle table against `longdouble`, the restatement of tests/_ckks_numpy.py
against itself (dense against FFT form, encode after decode), the proofs of the case lists that tests/test_ckks_gpu.py
compares the device with exactly, the reference's functional tests (ckks/src/lib.rs:126-304) through the restated scheme on
fixed seeds, and every rejection that is answered before a device is touched."""
import os
import re

import numpy as np
import pytest

import _ckks_numpy as K
import _client_numpy as C
from conftest import Q16, Q61

LD = np.longdouble
TAB = C.cdt_table(3.2)
INVALID, NULL = -9, -4


# ---- twiddles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 64, 8192])
def test_twiddles_are_within_one_ulp_of_longdouble(pkg, n):
    got = pkg.binding.ckks_twiddles(n)
    c, s = K.root_powers_ld(n, n)
    for g, w in ((got.real, c), (got.imag, s)):
        assert (np.abs(g.astype(LD) - w) <= np.spacing(np.abs(g)).astype(LD)).all()
    assert got[0] == 1 and got[n // 2] == 1j                           # exact at the axes


def test_twiddle_rejections(pkg):
    L = pkg.load_library()
    buf = np.empty(16, dtype=np.complex128)
    for n in (0, 1, 3, 24, 1 << 14):
        assert L.fhe_ckks_twiddles(n, buf.ctypes.data) == INVALID
    assert L.fhe_ckks_twiddles(8, None) == NULL


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_dense_and_fft_forms_agree_at_512():
    p = np.random.default_rng(5).integers(-(1 << 40), 1 << 40, (3, 512), dtype=np.int64)
    delta = 1024.0
    dense, fft = K.decode(p, delta), K.decode_fft(p, delta)
    worst = np.abs(dense - fft).max(axis=1)
    print(f"\ndense against FFT decode at N = 512: {worst.max():.3e} against E_dec {K.e_dec(p, delta).min():.3e}")
    assert (worst <= K.e_dec(p, delta)).all()
    z = K.random_case(512, 6, 2)
    a_dense = K.encode_pre_dense_ld(z, delta).astype(np.float64)
    c, s = K.root_powers_ld(512, 512)
    a_fft = (np.fft.fft(K.hermitian(z, delta), axis=-1) * (c.astype(np.float64) - 1j * s.astype(np.float64))).real / 512
    assert (np.abs(a_dense - a_fft).max(axis=1) <= K.e_enc(z, delta)).all()


@pytest.mark.parametrize("n", [2, 16, 512, 4096])
def test_encode_after_decode_is_the_identity_on_integer_polynomials(n):
    p = np.random.default_rng(n).integers(-1000, 1000, (2, n), dtype=np.int64)
    assert np.array_equal(K.encode(K.decode(p, 64.0), 64.0), p)


# ---- the case lists of the GPU module -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,b,ld", K.EXACT_CASES)
def test_exact_construction_cases(n, seed, b, ld):
    """the restatement's own pre-rounding values lie within 2^-8 of p: far outside E_enc, far inside 1/2, so the encoder
    must return p exactly"""
    delta = float(1 << ld)
    p = K.exact_case(n, seed, b)
    z = K.exact_case_slots(p, delta)
    worst = np.abs(K.encode_pre(z, delta) - p).max()
    print(f"\nN = {n}: pre-rounding value within {worst:.3e} of p, E_enc {K.e_enc(z, delta).max():.3e}")
    assert worst < 2.0 ** -8 and K.e_enc(z, delta).max() < 2.0 ** -8


def _half_margin(z, delta):
    pre = K.encode_pre(z, delta)
    return np.abs(pre - np.floor(pre) - 0.5).min(), max(2.0 ** -20, 4 * K.e_enc(z, delta).max())


@pytest.mark.parametrize("n,seed,rows,ld", K.RANDOM_CASES)
def test_random_cases_stay_away_from_half_integers(n, seed, rows, ld):
    """every pre-rounding value is at least max(2^-20, 4 E_enc) from a half-integer: no coefficient is exempt"""
    got, need = _half_margin(K.random_case(n, seed, rows), float(1 << ld))
    print(f"\nN = {n}: nearest half-integer at {got:.3e}, needed {need:.3e}")
    assert got >= need


@pytest.mark.parametrize("name", ["encrypt_32", "encode_16", "add_16", "sub_16", "mul_plain_32_q61"])
def test_functional_slots_stay_away_from_half_integers(name):
    """so the device's encoding of these slots is the restatement's, word for word"""
    case = K.FUNCTIONAL[name]
    for k in range(2):
        got, need = _half_margin(K.case_slots(case, k), case["delta"])
        assert got >= need


# ---- the reference's functional tests through the restated scheme ----------------------------------------------------------------
def _keys(case):
    s = K.secret_key(case["seed"], 0, case["n"])
    return s, K.public_key(case["seed"], K.PK_BASE, s, case["q"], TAB)


def _rounded(z):
    return K.round_away(z.real) + 1j * K.round_away(z.imag)


def test_encrypt_decrypt_of_scaled_messages():
    """lib.rs:126-161: q = 65537, n = 32, t = 50, Delta = 512"""
    case = K.FUNCTIONAL["encrypt_32"]
    s, pk = _keys(case)
    raw = K.case_raw_message(case)
    c0, c1 = K.encrypt(case["seed"], 0, pk[0], pk[1], raw * 512, len(raw), case["q"], TAB)
    d = K.decrypt(s, c0, c1, case["q"])
    print(f"\nencrypt_32: worst |noise| / Delta {np.abs(d - raw * 512).max() / 512:.4f} against 1/2")
    assert np.array_equal(K.round_away(d / 512.0), raw)


@pytest.mark.parametrize("name", ["encode_16", "encode_4096_q61"])
def test_encode_encrypt_decrypt_decode(name):
    """lib.rs:163-210 (n = 16, t = 8, Delta = 512) and the same at the 61-bit modulus, n = 4096, Delta = 2^30"""
    case = K.FUNCTIONAL[name]
    s, pk = _keys(case)
    z = K.case_slots(case, 0)
    m = K.encode(z, case["delta"])
    assert np.array_equal(_rounded(K.decode(m, case["delta"])), z)
    c0, c1 = K.encrypt(case["seed"], 0, pk[0], pk[1], m, len(m), case["q"], TAB)
    got = K.decode(K.decrypt(s, c0, c1, case["q"]), case["delta"])
    print(f"\n{name}: worst decoded error {np.abs(got - z).max():.4f} against 1/2")
    assert np.array_equal(_rounded(got), z)


@pytest.mark.parametrize("name", ["add_16", "sub_16", "add_4096_q61", "sub_4096_q61"])
def test_add_and_sub(name):
    """lib.rs:212-304 (n = 16, Delta = 1024, t = 8 and 2) and at the 61-bit modulus; sub expects z0 - z1"""
    case = K.FUNCTIONAL[name]
    s, pk = _keys(case)
    q, rows = case["q"], case["rows"]
    z0, z1 = K.case_slots(case, 0), K.case_slots(case, 1)
    ca = K.encrypt(case["seed"], 0, pk[0], pk[1], K.encode(z0, case["delta"]), rows, q, TAB)
    cb = K.encrypt(case["seed"], rows, pk[0], pk[1], K.encode(z1, case["delta"]), rows, q, TAB)
    c, want = (K.add(ca, cb, q), z0 + z1) if name.startswith("add") else (K.sub(ca, cb, q), z0 - z1)
    got = K.decode(K.decrypt(s, c[0], c[1], q), case["delta"])
    print(f"\n{name}: worst decoded error {np.abs(got - want).max():.4f} against 1/2")
    assert np.array_equal(_rounded(got), want)


def test_mul_plain():
    """ct(z0) times the encoding of z1 at the 61-bit modulus, n = 32, Delta = 2^20: decoded with scale Delta^2 it is z0 z1"""
    case = K.FUNCTIONAL["mul_plain_32_q61"]
    s, pk = _keys(case)
    q, d = case["q"], case["delta"]
    z0, z1 = K.case_slots(case, 0), K.case_slots(case, 1)
    c0, c1 = K.encrypt(case["seed"], 0, pk[0], pk[1], K.encode(z0, d), 1, q, TAB)
    p0, p1 = K.mul_plain((c0[0], c1[0]), K.encode(z1, d)[0], q)
    got = K.decode(K.decrypt(s, p0, p1, q), d * d)
    print(f"\nmul_plain: worst decoded error {np.abs(got - z0 * z1).max():.6f} against 1/2")
    assert np.array_equal(_rounded(got), z0 * z1)


def test_secret_is_ternary_and_purposes_are_new():
    s = K.secret_key(bytes(range(32)), 0, 4096)
    assert set(np.unique(s)) == {-1, 0, 1} and abs(int((s == 0).sum()) - 2048) < 200
    import _bfv_client_numpy as BC

    ours = {K.CKKS_MASK, K.CKKS_ERR, K.CKKS_KEY, K.CKKS_EPH}
    assert ours == {0x21, 0x22, 0x23, 0x24} and not ours & {C.MASK, C.ERR, C.KEY, BC.BFV_MASK, BC.BFV_ERR, BC.BFV_KEY, BC.BFV_EPH}


# ---- the interface ------------------------------------------------------------------------------------------------------------
ENTRY = ("fhe_ckks_twiddles", "fhe_ckks_encode_dev", "fhe_ckks_decode_dev", "fhe_ckks_secret_key_dev", "fhe_ckks_public_key_dev", "fhe_ckks_encrypt_dev",
         "fhe_ckks_decrypt_dev")


def test_header_binding_and_design_name_the_entry_points(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fhe_ntt.h")) as f:
        h = f.read()
    for name in ENTRY:
        assert re.search(r"\bint\s+" + name + r"\(", h) and name in pkg.binding.EXPORTS
    assert "ckks_client.hip" in pkg.binding.SOURCES and "bfv_client_kernels.hpp" in pkg.binding.HEADERS
    with open(os.path.join(root, "DESIGN.md")) as f:
        assert re.search(r"^## 21\b", f.read(), re.M)
    B = pkg.binding
    assert (B.FHE_STREAM_CKKS_MASK, B.FHE_STREAM_CKKS_ERR, B.FHE_STREAM_CKKS_KEY, B.FHE_STREAM_CKKS_EPH) == (0x21, 0x22, 0x23, 0x24)
    for name, val in (("MASK", 0x21), ("ERR", 0x22), ("KEY", 0x23), ("EPH", 0x24)):
        assert re.search(r"#define FHE_STREAM_CKKS_%s 0x%xu" % (name, val), h)
    from fhe_study_amd import ckks

    assert ckks.ClientKey.PK_BASE == K.PK_BASE and ckks.Param(pkg.RingParam(Q16, 16)).ring.n == 16


SEED = bytes(range(32))
A, B_, C_, D = 1 << 20, 2 << 20, 3 << 20, 4 << 20                              # fake device addresses: every check below fails first


def test_the_tfhe_stream_entry_point_rejects_the_ckks_purposes(pkg):
    L = pkg.load_library()
    for purpose in (0x21, 0x22, 0x23, 0x24):
        assert L.fhe_tfhe_stream_words_dev(SEED, purpose, 0, 8, 0, D, 1, None) == INVALID


def test_encoder_rejections_that_need_no_device(pkg):
    L = pkg.load_library()
    enc = lambda **kw: L.fhe_ckks_encode_dev(kw.get("n", 16), kw.get("delta", 64.0), kw.get("tw", A), kw.get("z", B_), kw.get("stride", 8), kw.get("out", D),
                                             kw.get("batch", 2), None)
    dec = lambda **kw: L.fhe_ckks_decode_dev(kw.get("n", 16), kw.get("delta", 64.0), kw.get("tw", A), kw.get("p", B_), kw.get("out", D), kw.get("batch", 2), None)
    for f in (enc, dec):
        for n in (0, 1, 3, 24, 1 << 14, 1 << 19):
            assert f(n=n) == INVALID, n
        for delta in (0.0, -1.0, float("inf"), float("nan")):
            assert f(delta=delta) == INVALID, delta
        assert f(tw=None) == NULL and f(out=None) == NULL and f(tw=A + 4) == INVALID and f(out=D + 4) == INVALID
        assert f(batch=1 << 58) == INVALID
        assert f(out=A) == INVALID and f(out=A - 8) == INVALID and f(out=B_) == INVALID     # the table and the input
        assert b"overlaps" in L.fhe_last_error()
        assert f(batch=0, tw=None, out=None) == 0 and f(batch=0, n=3) == INVALID
    assert enc(z=None) == NULL and dec(p=None) == NULL and enc(z=B_ + 4) == INVALID
    assert enc(stride=7) == INVALID and enc(stride=1 << 60) == INVALID
    assert enc(stride=0, z=D + 8 * 16) == INVALID and enc(stride=0, z=D - 8) == INVALID


def test_scheme_rejections_that_need_no_device(pkg):
    L = pkg.load_library()
    plan, m = pkg.Plan(Q16, 16), len(TAB)

    def enc(**kw):
        a = dict(plan=plan.handle, seed=SEED, first_row=0, pk=A, msg=B_, stride=16, cdt=C_, m=m, out=D, batch=2)
        a.update(kw)
        return L.fhe_ckks_encrypt_dev(a["plan"], a["seed"], a["first_row"], a["pk"], a["msg"], a["stride"], a["cdt"], a["m"], a["out"], a["batch"], None)

    assert enc(plan=None) == NULL and enc(seed=None) == NULL and enc(pk=None) == NULL and enc(out=None) == NULL and enc(cdt=None) == NULL
    assert enc(m=1025) == INVALID and enc(plan=pkg.Plan(17, 8).handle, m=17) == INVALID and enc(cdt=C_ + 4) == INVALID
    assert enc(stride=15) == INVALID and enc(first_row=(1 << 63) - 1) == INVALID and enc(first_row=1 << 63, batch=1) == INVALID
    assert enc(batch=1 << 56) == INVALID and enc(stride=1 << 60) == INVALID and enc(out=D + 4) == INVALID and enc(msg=B_ + 4) == INVALID
    for kw in (dict(out=A), dict(out=A - 8), dict(out=B_ - 8), dict(out=C_ - 8 * 63), dict(msg=D + 8 * 32, stride=0)):
        assert enc(**kw) == INVALID and b"overlaps" in L.fhe_last_error(), kw
    assert enc(batch=0, pk=None, out=None, msg=None) == 0 and enc(batch=0, m=1025) == INVALID
    assert L.fhe_ckks_secret_key_dev(None, SEED, 0, A, None) == NULL and L.fhe_ckks_secret_key_dev(plan.handle, None, 0, A, None) == NULL
    assert L.fhe_ckks_secret_key_dev(plan.handle, SEED, 0, None, None) == NULL and L.fhe_ckks_secret_key_dev(plan.handle, SEED, 0, A + 4, None) == INVALID
    pkc = lambda **kw: L.fhe_ckks_public_key_dev(kw.get("plan", plan.handle), kw.get("seed", SEED), kw.get("row", 0), kw.get("s", A), kw.get("cdt", C_),
                                                 kw.get("m", m), kw.get("pk", D), None)
    assert pkc(plan=None) == NULL and pkc(seed=None) == NULL and pkc(s=None) == NULL and pkc(pk=None) == NULL
    assert pkc(m=1025) == INVALID and pkc(row=1 << 63) == INVALID and pkc(pk=D + 4) == INVALID and pkc(pk=A - 8) == INVALID and pkc(pk=C_) == INVALID
    dec = lambda **kw: L.fhe_ckks_decrypt_dev(kw.get("plan", plan.handle), kw.get("s", A), kw.get("ct", B_), kw.get("out", D), kw.get("batch", 2), None)
    assert dec(plan=None) == NULL and dec(s=None) == NULL and dec(ct=None) == NULL and dec(out=None) == NULL
    assert dec(batch=1 << 56) == INVALID and dec(out=D + 4) == INVALID and dec(out=B_) == INVALID and dec(out=B_ + 8 * 63) == INVALID and dec(out=A - 8) == INVALID
    assert dec(batch=0, s=None, ct=None, out=None) == 0
