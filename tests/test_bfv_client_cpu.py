"""The BFV client side of DESIGN.md §20 without a device: the uniform map, the ephemeral u and the exact product of
tests/_bfv_client_numpy.py against their definitions, the restated scheme on the reference's own property tests
(bfv/src/lib.rs:281-377, 557-601) at the reference's parameters with fixed seeds (the GPU functional tests of
tests/test_bfv_client_gpu.py use the same seeds, rows and messages, and the device words equal the restatement's, so their
outcome is decided here), the exact relinearisation key against MiniBFV.rlk_key's arithmetic, and every rejection of the
entry points that is answered before a device is touched."""
import os
import re

import numpy as np
import pytest

import _bfv_client_numpy as BC
import _bfv_numpy as BN
import _client_numpy as C
from conftest import Q16, Q61

U64 = np.uint64
Q62 = 9223372036844421121                                                      # the NTT-friendly prime above 2^62 of tests/test_glue_rows.py
TAB = C.cdt_table(3.2)
INVALID, NULL, BAD_N = -9, -4, -1


# ---- samples ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [Q16, Q61, Q62, (1 << 63) - 25, 2])
def test_uniform_map_is_the_big_integer_formula(Q):
    """in range, and the kernels' two-multiplication form equals floor(w Q / 2^128) at w = 0, 2^128 - 1, the words around a
    carry out of the low product, and random words (seed 20)"""
    rng = np.random.default_rng(20)
    top = (1 << 64) - 1
    words = [(0, 0), (top, top), (top, 0), (0, top), (1, top), (top, 1), (top - 1, top)]
    words += [(int(a), int(b)) for a, b in rng.integers(0, 1 << 64, (2000, 2), dtype=np.uint64, endpoint=False)]
    for w0, w1 in words:
        v = BC.uniform_word(w0, w1, Q)
        assert 0 <= v < Q and v == BC.uniform_word_device(w0, w1, Q)
    assert BC.uniform_word(0, 0, Q) == 0 and BC.uniform_word(top, top, Q) == Q - 1


def test_uniform_rows_are_uniform_modulo_a_small_modulus():
    """4096 coefficients modulo 16 of MASK row 5 under the seed 0, 1, .., 31: Pearson's chi-square on 15 degrees of freedom
    stays below 50, the 1 - 1e-5 quantile (44.3 is the 1 - 1e-4 quantile): deterministic, and a biased map (a mod of the low
    word, a dropped high word) fails by orders of magnitude.  Word i of a row depends on i only: a shorter row is a prefix."""
    seed = bytes(range(32))
    a = BC.uniform_row(seed, 5, 4096, 16)
    counts = np.bincount(a.astype(np.int64), minlength=16)
    chi2 = float(((counts - 256.0) ** 2 / 256.0).sum())
    print(f"\nchi-square of 4096 coefficients modulo 16: {chi2:.2f} (bound 50)")
    assert len(counts) == 16 and chi2 < 50
    assert np.array_equal(BC.uniform_row(seed, 5, 64, 16), a[:64])
    assert not np.array_equal(BC.uniform_row(seed, 6, 64, 16), a[:64])


def test_ephemeral_is_minus_one_zero_one_with_the_counts_of_the_bits():
    seed = bytes(range(1, 33))
    w = C.stream_words(seed, BC.BFV_EPH, 3, 4096, 2)
    u = BC.ephemeral(seed, 3, 4096, 2)
    b0, b1 = (w & U64(1)).astype(bool), ((w >> U64(1)) & U64(1)).astype(bool)
    assert set(np.unique(u)) == {-1, 0, 1}
    assert (u == 1).sum() == (b0 & ~b1).sum() and (u == -1).sum() == (~b0 & b1).sum() and (u == 0).sum() == (b0 == b1).sum()
    # 8192 draws of probability 1/4: within 6 standard deviations (39 each) of 2048
    assert abs(int((u == 1).sum()) - 2048) < 240 and abs(int((u == -1).sum()) - 2048) < 240
    assert np.array_equal(BC.ephemeral_of_words(np.array([0, 1, 2, 3, 4, 5], dtype=U64)), [0, 1, -1, 0, 0, 1])
    s = BC.secret_key(seed, 0, 200)
    assert set(s) == {0, 1} and np.array_equal(s, C.stream_words(seed, BC.BFV_KEY, 0, 200, 1)[0] & U64(1))


def test_purposes_do_not_meet_the_tfhe_rows():
    assert {BC.BFV_MASK, BC.BFV_ERR, BC.BFV_KEY, BC.BFV_EPH} == {0x11, 0x12, 0x13, 0x14}
    assert not {BC.BFV_MASK, BC.BFV_ERR, BC.BFV_KEY, BC.BFV_EPH} & {C.MASK, C.ERR, C.KEY}


@pytest.mark.parametrize("Q,n,rows", [(Q16, 16, 1), (Q16, 32, 5), (Q61, 16, 5), (Q62, 64, 3), (Q16 ** 3, 32, 1), (Q16 ** 3, 16, 4)])
def test_the_restated_product_is_the_schoolbook_product(Q, n, rows):
    """both routes of BC.negacyclic (np.convolve for up to two rows, the float64 matrix product for a batch), with the large
    operand as the batch and as the shared one, against the term-by-term definition"""
    rng = np.random.default_rng(n + rows)
    a = rng.integers(0, Q, (rows, n), dtype=np.uint64)
    s = rng.integers(-1, 2, n)
    got = BC.negacyclic(a, s, Q)
    u = rng.integers(-1, 2, (rows, n))
    got2 = BC.negacyclic(u, a[0], Q)
    for r in range(rows):
        assert np.array_equal(got[r], BC.negacyclic_schoolbook(a[r], s, Q))
        assert np.array_equal(got2[r], BC.negacyclic_schoolbook(u[r], a[0], Q))


# ---- the scheme on the reference's property tests ------------------------------------------------------------------------------
def _keys(case):
    seed, q, n, t, p = case["seed"], case["q"], case["n"], case["t"], case["p"]
    s = BC.secret_key(seed, 0, n)
    pk = BC.public_key(seed, BC.PK_BASE, s, q, TAB)
    return seed, q, n, t, p, s, pk


def _margin(label, s, c, m, q, t):
    worst = max(abs(int(v)) for v in BC.noise(s, c[0], c[1], m, q, t).reshape(-1))
    print(f"\n{label}: worst |noise| {worst} against q / (2 t) = {q / (2 * t):.1f}")
    return worst


@pytest.mark.parametrize("name", ["encrypt_512", "encrypt_4096_q61"])
def test_encrypt_decrypt(name):
    """lib.rs:281-307 (q = 65537, n = 512, t = 32), 64 messages under one key; and the same at n = 4096 with the 61-bit modulus"""
    case = BC.CASES[name]
    seed, q, n, t, p, s, pk = _keys(case)
    m = BC.case_messages(case, 0)
    c0, c1, _ = BC.encrypt(seed, 0, pk[0], pk[1], m, len(m), q, t, TAB)
    _margin(name, s, (c0, c1), m, q, t)
    assert np.array_equal(BC.decrypt(s, c0, c1, q, t), m)


def test_addition():
    """lib.rs:309-340 at n = 128, t = 32: 32 pairs"""
    case = BC.CASES["add_128"]
    seed, q, n, t, p, s, pk = _keys(case)
    m1, m2 = BC.case_messages(case, 0), BC.case_messages(case, 1)
    ca = BC.encrypt(seed, 0, pk[0], pk[1], m1, len(m1), q, t, TAB)[:2]
    cb = BC.encrypt(seed, len(m1), pk[0], pk[1], m2, len(m2), q, t, TAB)[:2]
    c = BC.add(ca, cb, q)
    _margin("ct + ct", s, c, (m1 + m2) % U64(t), q, t)
    assert np.array_equal(BC.decrypt(s, c[0], c[1], q, t), (m1 + m2) % U64(t))


def _plain_product(m1, m2, n, t):
    return BC.negacyclic_schoolbook(m1, m2, t)


@pytest.mark.parametrize("name", ["const_16_t8", "mul_16_t2"])
def test_constants_and_the_relinearised_product(name):
    """lib.rs:342-377 (add_const, mul_const at n = 16, t = 8, p = q^2; repeated at t = 2) and lib.rs:557-601 (ct x ct with
    relinearisation at t = 2, the only t at which the reference claims it: at t = 8 its noise passes q / 2t), with
    tests/_bfv_numpy.mul as the product; every row of the case's batch"""
    case = BC.CASES[name]
    seed, q, n, t, p, s, pk = _keys(case)
    pq = p * q
    rlk = BC.relin_key(seed, BC.RLK_BASE, s, q, pq, TAB)
    m1, m2 = BC.case_messages(case, 0), BC.case_messages(case, 1)
    rows = len(m1)
    c0, c1, _ = BC.encrypt(seed, 0, pk[0], pk[1], m1, rows, q, t, TAB)
    d0, d1, _ = BC.encrypt(seed, rows, pk[0], pk[1], m2, rows, q, t, TAB)
    worst = 0
    for r in range(rows):
        want_add, want_mul = (m1[r] + m2[r]) % U64(t), _plain_product(m1[r], m2[r], n, t)
        a = BC.add_const((c0[r], c1[r]), m2[r], q, t)
        assert np.array_equal(BC.decrypt(s, a[0], a[1], q, t), want_add)
        k0, k1 = BC.const_ciphertext(m2[r], q, t)
        o0, o1 = BN.mul(q, n, t, pq, rlk[0], rlk[1], c0[r], c1[r], k0, k1)
        mc = (np.array(o0, dtype=U64), np.array(o1, dtype=U64))
        assert np.array_equal(BC.decrypt(s, mc[0], mc[1], q, t), want_mul)
        worst = max(worst, max(abs(int(v)) for v in BC.noise(s, mc[0], mc[1], want_mul, q, t)))
        if t == 2:                                                     # ct x ct: the reference claims it at t = 2 only (lib.rs:557-601)
            o0, o1 = BN.mul(q, n, t, pq, rlk[0], rlk[1], c0[r], c1[r], d0[r], d1[r])
            mm = (np.array(o0, dtype=U64), np.array(o1, dtype=U64))
            assert np.array_equal(BC.decrypt(s, mm[0], mm[1], q, t), want_mul)
            worst = max(worst, max(abs(int(v)) for v in BC.noise(s, mm[0], mm[1], want_mul, q, t)))
    print(f"\n{name}: worst |noise| after a product {worst} against q / (2 t) = {q / (2 * t):.1f}")


def test_exact_rlk_is_minibfv_rlk_key_where_the_f64_route_is_exact():
    """n = 16, q = 65537, p = q^2: MiniBFV.rlk_key (tests/test_next_rows.py: tmp_naive_mul -> from_vec_i64, through f64) drawn
    from a generator that hands it the restatement's a and e gives the exact key: every integer sum is below 16 2^51 < 2^53
    for this seed, which the case asserts (every coefficient of the integer product a s) before the equality"""
    from test_next_rows import MiniBFV, _conv

    q, n = Q16, 16
    pq = q ** 3
    seed = BC.CASES["mul_16_t2"]["seed"]
    s = BC.secret_key(seed, 0, n)
    a = BC.uniform_row(seed, BC.RLK_BASE, n, pq)
    e = BC.errors(seed, 2 * BC.RLK_BASE, n, 1, TAB)[0]

    class Feed:
        def __init__(self):
            self.e = [float(x) for x in e]

        def integers(self, lo, hi, count):
            assert (lo, hi, count) == (0, pq, n)
            return a

        def normal(self, mu, sigma):
            return self.e.pop(0)

    assert max(abs(x) for x in _conv([int(x) for x in a], [int(x) for x in s])) < 1 << 53
    r0, r1 = MiniBFV(q, n, 2, q * q, Feed()).rlk_key([int(x) for x in s])
    k0, k1 = BC.relin_key(seed, BC.RLK_BASE, s, q, pq, TAB)
    assert [int(x) for x in k0] == r0 and [int(x) for x in k1] == [int(x) for x in r1]
    assert np.array_equal(k0, BC.relin_key_from(a, s, e, q, pq)[0])


def test_exact_rlk_against_python_integers_past_2_pow_53():
    """n = 64, pq = q^3: with a = pq - 1 everywhere and s all ones, |a s| reaches 64 2^51 = 2^57 > 2^53, where the reference's
    f64 route rounds; the restatement still equals the definition in Python integers"""
    q, n = Q16, 64
    pq = q ** 3
    a = np.full(n, pq - 1, dtype=U64)
    s = np.ones(n, dtype=U64)
    e = np.arange(n, dtype=np.int64) - 32
    k0, _ = BC.relin_key_from(a, s, e, q, pq)
    a_s = BC.negacyclic_schoolbook(a, s, pq)
    ss = BC.negacyclic_schoolbook(s, s, pq)
    want = [(-(int(x) + int(y)) + (pq // q) * int(z)) % pq for x, y, z in zip(a_s, e, ss)]
    assert [int(x) for x in k0] == want


# ---- the interface ------------------------------------------------------------------------------------------------------------
ENTRY = ("fhe_bfv_secret_key_dev", "fhe_bfv_public_key_dev", "fhe_bfv_relin_key_dev", "fhe_bfv_encrypt_dev", "fhe_bfv_decrypt_dev")


def test_header_binding_and_design_name_the_entry_points(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fhe_ntt.h")) as f:
        h = f.read()
    for name in ENTRY:
        assert re.search(r"\bint\s+" + name + r"\(", h) and name in pkg.binding.EXPORTS
    assert "bfv_client.hip" in pkg.binding.SOURCES and "chacha_stream.hpp" in pkg.binding.HEADERS
    with open(os.path.join(root, "DESIGN.md")) as f:
        assert re.search(r"^## 20\b", f.read(), re.M)
    B = pkg.binding
    assert (B.FHE_STREAM_BFV_MASK, B.FHE_STREAM_BFV_ERR, B.FHE_STREAM_BFV_KEY, B.FHE_STREAM_BFV_EPH) == (0x11, 0x12, 0x13, 0x14)
    for name, val in (("MASK", 0x11), ("ERR", 0x12), ("KEY", 0x13), ("EPH", 0x14)):
        assert re.search(r"#define FHE_STREAM_BFV_%s 0x%xu" % (name, val), h)


def test_rows_of_the_python_builders_do_not_meet(pkg):
    from fhe_study_amd import bfv

    K = bfv.ClientKey
    assert K.ENCRYPT_ROWS == 1 << 56 and K.PK_BASE == 1 << 56 == BC.PK_BASE and K.RLK_BASE == 2 << 56 == BC.RLK_BASE
    # a key row r draws its error from ERR row 2 r; encryption rows below 2^56 use ERR rows below 2^57
    assert 2 * K.PK_BASE >= 2 * K.ENCRYPT_ROWS and 2 * K.RLK_BASE >= 2 * (K.PK_BASE + (1 << 16)) and 2 * (K.RLK_BASE + (1 << 16)) < 1 << 63
    p = bfv.Param(pkg.RingParam(Q16, 16), 8, Q16 * Q16)
    assert p.pt() == pkg.RingParam(8, 16)


SEED = bytes(range(32))
A, B_, C_, D = 1 << 20, 2 << 20, 3 << 20, 4 << 20                              # fake device addresses: every check below fails first


def _enc(L, plan, **kw):
    a = dict(t=32, seed=SEED, first_row=0, pk=A, msg=B_, stride=plan.n, cdt=C_, m=len(TAB), out=D, batch=2)
    a.update(kw)
    return L.fhe_bfv_encrypt_dev(None if a.get("no_plan") else plan.handle, a["t"], a["seed"], a["first_row"], a["pk"], a["msg"], a["stride"], a["cdt"],
                                 a["m"], a["out"], a["batch"], None)


def test_encrypt_rejections_that_need_no_device(pkg):
    L = pkg.load_library()
    plan = pkg.Plan(Q16, 16)
    assert _enc(L, plan, no_plan=1) == NULL and _enc(L, plan, seed=None) == NULL
    for t in (0, 1, Q16, Q16 + 1, 1 << 63):
        assert _enc(L, plan, t=t) == INVALID, t
    assert b"2 <= t < q" in L.fhe_last_error()
    assert _enc(L, plan, m=1025) == INVALID and _enc(L, pkg.Plan(17, 8), m=17, t=2) == INVALID
    assert b"below the modulus" in L.fhe_last_error()
    assert _enc(L, plan, cdt=None) == NULL and _enc(L, plan, cdt=C_ + 4) == INVALID
    assert _enc(L, plan, stride=15) == INVALID
    assert _enc(L, plan, first_row=(1 << 63) - 1) == INVALID and _enc(L, plan, first_row=1 << 63, batch=1) == INVALID
    assert _enc(L, plan, first_row=(1 << 64) - 1) == INVALID
    assert b"passes 2^63" in L.fhe_last_error()
    assert _enc(L, plan, batch=1 << 56) == INVALID and _enc(L, plan, stride=1 << 60) == INVALID
    assert b"too large" in L.fhe_last_error()
    assert _enc(L, plan, pk=None) == NULL and _enc(L, plan, out=None) == NULL
    assert _enc(L, plan, out=D + 4) == INVALID and _enc(L, plan, msg=B_ + 4) == INVALID
    for kw in (dict(out=A), dict(out=A - 8), dict(out=B_ - 8), dict(out=C_ - 8 * 63), dict(msg=D + 8 * 32, stride=0)):
        assert _enc(L, plan, **kw) == INVALID, kw
        assert b"overlaps" in L.fhe_last_error()
    assert _enc(L, plan, batch=0, pk=None, out=None, msg=None) == 0                    # the empty batch is a no-op
    assert _enc(L, plan, batch=0, t=1) == INVALID                                      # but its parameters are still checked


def test_key_and_decrypt_rejections_that_need_no_device(pkg):
    L = pkg.load_library()
    plan = pkg.Plan(Q16, 16)
    m = len(TAB)
    assert L.fhe_bfv_secret_key_dev(3, SEED, 0, A, None) == BAD_N and L.fhe_bfv_secret_key_dev(16, None, 0, A, None) == NULL
    assert L.fhe_bfv_secret_key_dev(16, SEED, 0, None, None) == NULL and L.fhe_bfv_secret_key_dev(16, SEED, 0, A + 4, None) == INVALID
    pkc = lambda **kw: L.fhe_bfv_public_key_dev(kw.get("plan", plan.handle), kw.get("seed", SEED), kw.get("row", 0), kw.get("s", A), kw.get("cdt", C_),
                                                kw.get("m", m), kw.get("pk", D), None)
    assert pkc(plan=None) == NULL and pkc(seed=None) == NULL and pkc(s=None) == NULL and pkc(pk=None) == NULL
    assert pkc(m=1025) == INVALID and pkc(row=1 << 63) == INVALID and pkc(pk=D + 4) == INVALID
    assert pkc(pk=A - 8) == INVALID and pkc(pk=C_) == INVALID and pkc(plan=pkg.Plan(17, 8).handle, m=17) == INVALID
    q = Q16
    rlk = lambda **kw: L.fhe_bfv_relin_key_dev(kw.get("q", q), kw.get("n", 16), kw.get("pq", q ** 3), kw.get("seed", SEED), kw.get("row", 0),
                                               kw.get("s", A), kw.get("cdt", C_), kw.get("m", m), kw.get("rlk", D), None)
    assert rlk(n=24) == BAD_N and rlk(seed=None) == NULL and rlk(s=None) == NULL and rlk(rlk=None) == NULL
    assert rlk(pq=q ** 3 + 1) == INVALID and rlk(pq=q - 1) == INVALID and rlk(q=0) == INVALID
    assert b"multiple of q" in L.fhe_last_error()
    assert rlk(n=32768) == INVALID                                                   # q^3 = 2^48 (1 + 2^-16)^3: n pq just above 2^63
    assert b"n pq < 2^63" in L.fhe_last_error()
    assert rlk(q=3, pq=9, m=9) == INVALID and rlk(m=1025) == INVALID and rlk(row=1 << 63) == INVALID
    assert rlk(rlk=A) == INVALID and rlk(rlk=D + 4) == INVALID
    dec = lambda **kw: L.fhe_bfv_decrypt_dev(kw.get("plan", plan.handle), kw.get("t", 32), kw.get("s", A), kw.get("ct", B_), kw.get("out", D),
                                             kw.get("batch", 2), None)
    assert dec(plan=None) == NULL and dec(s=None) == NULL and dec(ct=None) == NULL and dec(out=None) == NULL
    for t in (0, 1, Q16, 1 << 63):
        assert dec(t=t) == INVALID
    assert dec(batch=1 << 56) == INVALID and dec(out=D + 4) == INVALID
    assert dec(out=B_) == INVALID and dec(out=B_ + 8 * 63) == INVALID and dec(out=A - 8) == INVALID
    assert dec(batch=0, s=None, ct=None, out=None) == 0
