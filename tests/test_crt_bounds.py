"""The CRT-lifted products at the edges of their admission rules.

BFV's tensor and relinearisation (csrc/bfv32.hip, csrc/zring.hip) and TFHE's external product and base-2 key switch
(csrc/digit32.hip, csrc/digit_mac.hip, zring's one-prime form) are bit-exact only while an integer stays below a CRT
modulus: the product of the primes for the non-negative linear convolutions, half of it for the centred lifts.  Each
host rule that admits a shape to a form was argued on paper; uniform random inputs land about two bits below the worst
case, so a rule one bit too loose, or a lift wrong in its top bit, would leave the rest of the suite green.

CPU part: every rule restated in exact Python integers, its worst-case integer checked against the modulus over a grid
of shapes, and the library's choices (as the ABI shows them without a device) checked against the restatement one step
either side of every edge.  GPU part: constant-extreme inputs (every product term at its maximum) plus one random row
per case, word for word against the oracle, with the kernel timer showing which path ran.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import Q61, ROOT

# the 27-bit primes of the two / three-prime forms (csrc/digit32.hpp:13-15)
PA, PB, PC = 0x0A3C8001, 0x0A320001, 0x0A318001
# the 61-bit CRT primes of zring's K-prime forms (csrc/zring.hip:40-44)
P61 = (2305843009211596801, 2305843009196916737, 2305843009146585089)
EXT32 = os.environ.get("FHE_EXT32", "1")[:1] != "0"          # fhe_ext32_enabled (zring.hip)
U64 = 1 << 64
M32 = (1 << 32) - 1


def bits(x):                                    # bits_of / bits_of64
    return int(x).bit_length()


def clog2(x):                                   # ceil_log2 (zring.hip:482)
    return 0 if x <= 1 else bits(x - 1)


def primes_for_bits(b, signed):                 # zring.hip primes_for_bits
    need = b + (1 if signed else 0)
    return 1 if need <= 60 else 2 if need <= 121 else 3 if need <= 182 else 0


def crt_product(k):
    out = 1
    for p in P61[:k]:
        out *= p
    return out


# ---- BFV ------------------------------------------------------------------------------------------------------------------

def bfv32_tensor_ok(q, n):
    """bfv32.hip:494-496: 1024 <= n <= 8192, 2 bits(q-1) + bits(n-1) + 1 <= 54"""
    if n < 1024 or n > 8192 or n & (n - 1) or q < 2:
        return False
    return 2 * bits(q - 1) + bits(n - 1) + 1 <= 54


def bfv32_ok(q, n, pq):
    """bfv32.hip:493-499 (bfv32_shape_supported): the tensor's rule and, for pq != 0, bits(q-1) + bits(pq-1) + bits(n-1) <= 82"""
    if not bfv32_tensor_ok(q, n):
        return False
    return not pq or (pq >= q and bits(q - 1) + bits(pq - 1) + bits(n - 1) <= 82)


def relin_split_bits(q, n, pq):
    """zring.hip:692-695: the key split at h = ceil(bits(pq-1) / 2) when bits(q-1) + h + log n <= 60"""
    h = (bits(pq - 1) + 1) // 2
    return h if h >= 1 and bits(q - 1) + h + clog2(n) <= 60 else 0


def relin_form(q, n, pq):
    """('bfv32' | 'split' | 'crt', K) as fhe_bfv_relinearize_dev picks it"""
    if EXT32 and bfv32_ok(q, n, pq):
        return "bfv32", 3
    if relin_split_bits(q, n, pq):
        return "split", 1
    return "crt", primes_for_bits(bits(q - 1) + bits(pq - 1) + clog2(n), False)


def rlk_words(q, n, pq):
    """fhe_bfv_rlk_prepared_words (zring.hip:704-710) restated: 6n (three 27-bit primes), 8n (split key), 4Kn (K primes)"""
    if n < 2 or n & (n - 1) or n > 1 << 19 or q < 2 or q >> 63 or pq < q or pq >> 63:
        return 0
    form, K = relin_form(q, n, pq)
    if form == "bfv32":
        return 6 * n
    if form == "split":
        return 8 * n
    return 4 * K * n if 1 <= K <= 3 else 0


def check_relin_bound(q, n, pq):
    """the worst-case integer of the form the library takes is below its modulus"""
    form, K = relin_form(q, n, pq)
    worst = n * (q - 1) * (pq - 1)                                  # c2 = q-1 against rlk = pq-1, n terms, non-negative
    if form == "bfv32":
        assert worst < PA * PB * PC, (q, n, pq)
    elif form == "split":
        h = relin_split_bits(q, n, pq)
        lo, hi = (1 << h) - 1, (pq - 1) >> h
        assert hi < 1 << h
        assert n * (q - 1) * max(lo, hi) < P61[0], (q, n, pq)
    elif 1 <= K <= 3:
        assert worst < crt_product(K), (q, n, pq)


def tensor_form(q, n):
    if EXT32 and bfv32_tensor_ok(q, n):
        return "bfv32", 2
    return "crt", primes_for_bits(2 * bits(q - 1) + clog2(n) + 1, False)     # zring.hip fhe_bfv_tensor_dev


def check_tensor_bound(q, n):
    form, K = tensor_form(q, n)
    worst = 2 * n * (q - 1) ** 2                                    # c1 = a0 b1 + a1 b0 at coefficient n - 1
    assert worst < (PA * PB if form == "bfv32" else crt_product(K)), (q, n)


def q_top(n):
    """the largest q the bfv32 tensor admits at n: bits(q-1) = (53 - bits(n-1)) // 2"""
    return 1 << ((54 - bits(n - 1) - 1) // 2)


def epilogue_gates(q, n, t):
    """zring.hip bfv32_tensor: (small_f64, rdenf) for the tensor's epilogue (the defaults: FHE_BFV_SMALL_F64 /
    FHE_BFV_FAST_DIV unset)"""
    vmax = 2 * n * (q - 1) ** 2
    small = q < 1 << 30 and vmax * t // q < 1 << 50
    rden = vmax * t // q < 1 << 52 and q & 1 == 1 and q < 1 << 48
    return small, rden


def epilogue_ts(q, n):
    """t = 2 (both gates on), the smallest t past the small_f64 gate (rdenf still on) and the smallest past rdenf's"""
    vmax = 2 * n * (q - 1) ** 2
    return 2, -(-(q << 50) // vmax), -(-(q << 52) // vmax)


BFV_N = (1024, 2048, 4096, 8192)


def _bfv_grid():
    q_edges = sorted({q_top(n) + d for n in BFV_N for d in (-2, -1, 0, 1, 2)})
    for n in (512,) + BFV_N + (16384, 1 << 19, 1 << 20):
        for q in sorted(set(q_edges) | {2, 3, 12289, 65537, 131071, 786433, (1 << 30) + 3, (1 << 62) + 1}):
            pqs = {q, q * q, q ** 3, (1 << 63) - 1, 1 << 63}
            b82 = 82 - bits(q - 1) - bits(n - 1)                    # bfv32's relinearisation edge: bits(pq-1) <= b82
            hmax = 60 - bits(q - 1) - clog2(n)                      # the split's edge: bits(pq-1) <= 2 hmax
            b121 = 121 - bits(q - 1) - clog2(n)                     # two / three 61-bit primes
            b60 = 60 - bits(q - 1) - clog2(n)
            for b in (b82, 2 * hmax, b121, b60):
                if 1 <= b <= 64:
                    pqs |= {(1 << b) - 1, 1 << b, (1 << b) + 1, (1 << (b - 1)) + 1}
            for pq in sorted(pqs):
                yield q, n, pq


def test_bfv_rules_bound_every_admitted_integer_and_the_library_agrees(pkg):
    """Every (q, n, pq) of the grid — each n of bfv32 and either side, q and pq one step either side of every edge:
    the form fhe_bfv_rlk_prepared_words reports is the restatement's, and that form's worst-case integer is below its
    modulus.  (A rule loosened by one bit in bfv32_shape_supported changes the reported words at the edge.)"""
    L = pkg.load_library()
    seen = {"bfv32": 0, "split": 0, "crt": 0}
    edges = 0
    for q, n, pq in _bfv_grid():
        want = rlk_words(q, n, pq)
        got = L.fhe_bfv_rlk_prepared_words(q, n, pq)
        assert got == want, (q, n, pq, got, want)
        if want:
            check_relin_bound(q, n, pq)
            seen[relin_form(q, n, pq)[0]] += 1
            if bits(q - 1) + bits(pq - 1) + bits(n - 1) in (82, 83) and bfv32_tensor_ok(q, n):
                edges += 1
        if n <= 1 << 19 and 2 <= q < 1 << 63:
            check_tensor_bound(q, n)
    assert all(seen.values()) or not EXT32, seen
    assert edges >= 2 * len(BFV_N)
    # the edges are where the table of the issue says: q <= 2^21, 2^21, 2^20, 2^20
    assert [q_top(n) for n in BFV_N] == [1 << 21, 1 << 21, 1 << 20, 1 << 20]
    for n in BFV_N:
        assert bfv32_tensor_ok(q_top(n), n) and not bfv32_tensor_ok(q_top(n) + 1, n)
    # the largest tensor integer reaches past 2^53 (where (double) v rounds) at n = 2048 and 8192 only
    assert [2 * n * (q_top(n) - 1) ** 2 >= 1 << 53 for n in BFV_N] == [False, True, False, True]


def test_bfv_relinearisation_edge_cases_are_where_the_gpu_tests_put_them():
    """The relinearisation cases of the GPU test, on paper: 17 + 52 + 13 = 82 bits at 2^81.99997 on three 27-bit primes,
    the next pq up on the split key, and a two-prime case."""
    q, n = (1 << 17) - 1, 8192
    pq = q * ((1 << 35) - 1)
    assert bits(q - 1) + bits(pq - 1) + bits(n - 1) == 82 and bfv32_ok(q, n, pq)
    worst = n * (q - 1) * (pq - 1)
    assert 81.9999 < np.log2(float(worst)) < 82 and worst < PA * PB * PC
    pq83 = q * ((1 << 36) - 1)
    assert bits(pq83 - 1) == 53 and not bfv32_ok(q, n, pq83) and relin_split_bits(q, n, pq83) == 27
    assert n * (q - 1) * (pq83 - 1) > PA * PB * PC                  # on the three-prime form it would wrap
    q2, pq2 = (1 << 20) - 1, ((1 << 20) - 1) * ((1 << 42) - 1)
    assert bfv32_tensor_ok(q2, n) and not bfv32_ok(q2, n, pq2) and not relin_split_bits(q2, n, pq2)
    assert primes_for_bits(bits(q2 - 1) + bits(pq2 - 1) + clog2(n), False) == 2
    # each epilogue form of the tensor is reached by one of the t of epilogue_ts
    for n in BFV_N:
        for q in (q_top(n), q_top(n) - 1):
            forms = [epilogue_gates(q, n, t) for t in epilogue_ts(q, n)]
            assert forms[0][0] and not forms[1][0] and not forms[2][0] and not forms[2][1]
            assert forms[1][1] == (q & 1 == 1) and forms[0][1] == (q & 1 == 1)


def test_oracle_relinearize_composes_to_the_multiply(oracle):
    """Oracle.bfv_relinearize after Oracle.bfv_tensor is Oracle.bfv_mul (bfv/src/lib.rs:87-90)"""
    q, n, t = 65537, 16, 2
    pq = q ** 3
    rng = np.random.default_rng(16)
    ab = rng.integers(0, q, (4, 3, n), dtype=np.uint64)
    rlk = rng.integers(0, pq, (2, n), dtype=np.uint64)
    c = oracle.bfv_tensor(q, n, t, *ab)
    o = oracle.bfv_relinearize(q, n, pq, rlk[0], rlk[1], *c)
    w = oracle.bfv_mul(q, n, t, pq, rlk[0], rlk[1], *ab)
    assert np.array_equal(o[0], w[0]) and np.array_equal(o[1], w[1])


# ---- TFHE -----------------------------------------------------------------------------------------------------------------

def ext32_ok(n, k, l):
    """digit32.hip:510-514 (ext32_shape_supported)"""
    return k == 1 and 1 <= l <= 64 and 256 <= n <= 4096 and not n & (n - 1) and (k + 1) * l * n <= 1 << 21


def ks32_ok(q, n, k, l):
    """digit32.hip:516-520 (ks32_shape_supported) and glue.hip ks32_usable: base 2, q < 2^61"""
    return EXT32 and q >> 61 == 0 and k == 1 and 1 <= l <= 64 and 256 <= n <= 4096 and not n & (n - 1) and k * l * n <= 1 << 21


def one_prime_form(n, k, l):
    """zring.hip:974-976: (k+1) l n <= 2^26 and a single-pass size (16 <= n <= 2^13)"""
    return (k + 1) * l * n <= 1 << 26 and 16 <= n <= 1 << 13


def ext_form(n, k, l):
    if EXT32 and ext32_ok(n, k, l):
        return "ext32", 2
    if one_prime_form(n, k, l):
        return "one-prime", 1
    return "crt", primes_for_bits(64 + clog2(n) + clog2((k + 1) * l), True)   # zring.hip fhe_tggsw_external_product_dev


def tggsw_words(n, k, l):
    """fhe_tggsw_prepared_words (zring.hip:982-986) restated"""
    if n < 2 or n & (n - 1) or not 1 <= l <= 64 or not 1 <= k <= 64 or not one_prime_form(n, k, l):
        return 0
    return 2 * (k + 1) * l * (k + 1) * n


def check_ext_bound(n, k, l):
    """centred lifts: |sum| < modulus / 2.  The split forms sum T n products of a 32-bit key half and a 0/1 digit;
    the K-prime form sums T n products of a whole 64-bit word and a digit."""
    T = (k + 1) * l
    form, K = ext_form(n, k, l)
    if form == "ext32":
        assert 2 * T * n * M32 < PA * PB, (n, k, l)
    elif form == "one-prime":
        assert 2 * T * n * M32 < P61[0], (n, k, l)
    else:
        assert 1 <= K <= 3 and 2 * T * n * (U64 - 1) < crt_product(K), (n, k, l)


def test_tfhe_rules_bound_every_admitted_integer_and_the_library_agrees(pkg):
    """Every n = 2^1 .. 2^20 and k, l = 0 .. 65: fhe_tggsw_prepared_words is the restatement's (0 for the 61-bit
    K-prime form or an unsupported shape), and every admitted shape's worst half-sum is below half its modulus."""
    L = pkg.load_library()
    forms = set()
    for e in range(1, 21):
        n = 1 << e
        for k in range(0, 66):
            for l in range(0, 66):
                assert L.fhe_tggsw_prepared_words(n, k, l) == tggsw_words(n, k, l), (n, k, l)
                if 1 <= k <= 64 and 1 <= l <= 64 and n <= 1 << 19:
                    check_ext_bound(n, k, l)
                    forms.add(ext_form(n, k, l)[0])
    assert forms == ({"ext32", "one-prime", "crt"} if EXT32 else {"one-prime", "crt"})
    # the ext32 rule's 2^21 never binds inside its k = 1, n <= 4096, l <= 64 box: the largest T n there is 2^19
    assert max(2 * l * n for n in (256, 512, 1024, 2048, 4096) for l in range(1, 65)) == 1 << 19


def test_key_switch_rule_bounds_every_admitted_integer_and_the_library_agrees(pkg):
    """fhe_glwe_ksk_prepared_words doubles exactly where the base-2 key switch takes the two 27-bit primes
    (k = 1, 2^8 <= n <= 2^12, k l n <= 2^21, q < 2^61), and there |sum| < k l n (2^32 - 1) < pA pB / 2."""
    L = pkg.load_library()
    for q in (Q61, 65537, 9223372036844421121):
        for e in range(4, 15):
            n = 1 << e
            plan = pkg.Plan(q, n)
            for k in (1, 2, 3):
                for l in range(1, 65):
                    rows = k * l * (k + 1) * n
                    ks = ks32_ok(q, n, k, l)
                    assert L.fhe_glwe_ksk_prepared_words(plan.handle, k, 2, l) == (2 if ks else 1) * rows, (q, n, k, l)
                    if ks:
                        assert 2 * k * l * n * M32 < PA * PB


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def need_gpu(pkg):
    assert pkg.binding.device_count() >= 1, "no HIP device: -m gpu tests need a real MI355X"


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64).copy()).cuda()


def _ran(B, fn):
    """the kernel-timer names of what fn() launched"""
    import torch

    torch.cuda.synchronize()
    B.kernel_timing_reset()
    B.kernel_timing_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return set(B.kernel_timing_read())
    finally:
        B.kernel_timing_enable(False)


def _has(names, prefix):
    return any(nm.startswith(prefix) for nm in names)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BFV_N)
def test_bfv_tensor_at_the_edge_of_the_two_prime_rule(pkg, oracle, need_gpu, n):
    """fhe_bfv_tensor_dev with a0 = a1 = b0 = b1 = q - 1 (c1 reaches 2 n (q-1)^2 at coefficient n - 1) plus one random
    row, at the largest admitted q, an odd q just below it and the smallest rejected q (zring's path), each with t = 2,
    t past the small_f64 gate and t past the rdenf gate: the oracle's words, on the path the rule names."""
    L, B = pkg.load_library(), pkg.binding
    lg2 = (2 * n).bit_length() - 1
    top = q_top(n)
    for q in (top, top - 1, top + 1):
        admitted = bfv32_tensor_ok(q, n)
        assert admitted == (q != top + 1)
        vmax = 2 * n * (q - 1) ** 2
        if admitted:
            check_tensor_bound(q, n)
            if q == top:                                        # (double) v and t v round from here on
                assert (vmax >= 1 << 53) == (n in (2048, 8192))
        rng = np.random.default_rng(q + n)
        ab = np.empty((4, 2, n), dtype=np.uint64)
        ab[:, 0] = q - 1
        ab[:, 1] = rng.integers(0, q, (4, n), dtype=np.uint64)
        dab = _dev(ab)
        for t in epilogue_ts(q, n):
            out = _dev(np.zeros((3, 2, n), dtype=np.uint64))
            names = _ran(B, lambda: B._check(L.fhe_bfv_tensor_dev(q, n, t, dab.data_ptr(), out.data_ptr(), 2, None)))
            if EXT32 and admitted:
                assert f"bfv32_tensor_inverse_{lg2}" in names and not _has(names, "zr_"), (q, t, names)
            else:
                assert _has(names, "zr_") and not _has(names, "bfv32_"), (q, t, names)
            want = oracle.bfv_tensor(q, n, t, *ab)
            got = _u64(out)
            for w in range(3):
                assert np.array_equal(got[w], want[w]), (q, n, t, "c%d" % w, epilogue_gates(q, n, t))


RELIN_CASES = [
    # q, p, n
    ((1 << 17) - 1, (1 << 35) - 1, 8192),       # 17 + 52 + 13 = 82 bits: three 27-bit primes, worst 2^81.99997 of 2^82.055
    ((1 << 17) - 1, (1 << 36) - 1, 8192),       # 83 bits: the split key on one 61-bit prime
    ((1 << 20) - 1, (1 << 42) - 1, 8192),       # 95 bits, no split (20 + 31 + 13 > 60): two 61-bit primes
    ((1 << 17) - 1, 1 << 35, 8192),             # p a power of two: the IEEE division of the epilogue
    ((1 << 17) - 1, 1 << 13, 8192),             # p < 2^14: the general Zq::from_f64 as well
]


@pytest.mark.gpu
@pytest.mark.parametrize("q,p,n", RELIN_CASES)
def test_bfv_relinearisation_fed_directly_at_the_edge(pkg, oracle, need_gpu, q, p, n):
    """fhe_bfv_relinearize_dev and fhe_bfv_rlk_prepare_dev + fhe_bfv_relinearize_prepared_dev with c2 = q - 1 against
    rlk = pq - 1 (every term of c2 * rlk at its maximum) and c0 = c1 = q - 1, plus one random row: the oracle's
    relinearize_204, on the path the rule names."""
    L, B = pkg.load_library(), pkg.binding
    import torch

    pq = p * q
    form, K = relin_form(q, n, pq)
    check_relin_bound(q, n, pq)
    rng = np.random.default_rng(p + n)
    c = np.empty((3, 2, n), dtype=np.uint64)
    c[:, 0] = q - 1
    c[:, 1] = rng.integers(0, q, (3, n), dtype=np.uint64)
    rlk = np.full((2, n), pq - 1, dtype=np.uint64)
    dc, drlk = _dev(c), _dev(rlk)
    want = oracle.bfv_relinearize(q, n, pq, rlk[0], rlk[1], c[0], c[1], c[2])
    words = L.fhe_bfv_rlk_prepared_words(q, n, pq)
    assert words == rlk_words(q, n, pq)
    lg2 = (2 * n).bit_length() - 1
    marker = {"bfv32": f"bfv32_relin_inverse_{lg2}", "split": "zr_split_mdr_0", "crt": f"zr_crt_mdr_{K}"}[form]
    out = torch.empty((2, 2, n), dtype=torch.int64, device="cuda")
    names = _ran(B, lambda: B._check(L.fhe_bfv_relinearize_dev(q, n, pq, drlk.data_ptr(), dc.data_ptr(), out.data_ptr(), 2, None)))
    assert marker in names, (form, names)
    assert form == "bfv32" or not _has(names, "bfv32_"), names
    got = _u64(out)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (q, p, n, form)
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    out2 = torch.empty_like(out)

    def prepared():
        B._check(L.fhe_bfv_rlk_prepare_dev(q, n, pq, drlk.data_ptr(), prep.data_ptr(), None))
        B._check(L.fhe_bfv_relinearize_prepared_dev(q, n, pq, prep.data_ptr(), dc.data_ptr(), out2.data_ptr(), 2, None))
    names = _ran(B, prepared)
    assert marker in names, (form, names)
    assert torch.equal(out2, out)


def _minus_one_key_product(n, k, l, tglwe):
    """TGGSW x TGLWE for a key of words 2^64 - 1 (= -1): every (i, d, c) term is the negacyclic product of -1 ... -1
    with the 0/1 digit polynomial x, whose coefficient j is sum(x) - 2 (x_0 + ... + x_j).  The same for every c."""
    x = ((tglwe.reshape(k + 1, 1, n) >> np.arange(l - 1, -1, -1, dtype=np.uint64).reshape(1, l, 1)) & np.uint64(1)).astype(np.int64)
    s = (x.sum(axis=2, keepdims=True) - 2 * np.cumsum(x, axis=2)).sum(axis=(0, 1))
    return np.broadcast_to(s.view(np.uint64), (k + 1, n))


EXT_CASES = [
    # n, k, l
    (256, 1, 64),       # the closed forms against the oracle's schoolbook (two 27-bit primes)
    (4096, 1, 64),      # the largest two-27-bit-prime shape: half-sums reach 128 * 4096 * (2^32 - 1)
    (8192, 15, 64),     # one-prime form, T n = 2^23: half-sums reach 2^55 (of P1 / 2 = 2^60)
    (16384, 1, 64),     # beyond the one-prime form (not a single-pass size): two 61-bit primes, whole words
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,l", EXT_CASES)
def test_external_product_with_every_digit_one_against_a_minus_one_key(pkg, oracle, need_gpu, n, k, l):
    """TGGSW of words 2^64 - 1 x TGLWE of words 2^64 - 1: every digit is 1, and coefficient j of every output row is
    T (n - 2 - 2j) mod 2^64 (T = (k+1) l) — the half-sums reach -T (n-2) (2^32 - 1) at j = 0 and T n (2^32 - 1) at
    j = n - 1.  Plus one random TGLWE.  Unprepared and (where the shape has one) prepared key; the path the rule names."""
    L, B = pkg.load_library(), pkg.binding
    import torch

    T = (k + 1) * l
    form, K = ext_form(n, k, l)
    check_ext_bound(n, k, l)
    rng = np.random.default_rng(n + k + l)
    ct = np.empty((2, k + 1, n), dtype=np.uint64)
    ct[0] = U64 - 1
    ct[1] = rng.integers(0, U64, (k + 1, n), dtype=np.uint64)
    j = np.arange(n, dtype=np.int64)
    closed = np.broadcast_to((T * (n - 2 - 2 * j)).view(np.uint64), (k + 1, n))
    want = np.stack([closed, _minus_one_key_product(n, k, l, ct[1])])
    assert np.array_equal(_minus_one_key_product(n, k, l, ct[0]), closed)
    if n <= 4096:                                               # the oracle's schoolbook: both rows at 256, one product at 4096
        g_host = np.full((k + 1, l, k + 1, n), U64 - 1, dtype=np.uint64)
        rows = [0, 1] if n <= 256 else [1]
        assert np.array_equal(oracle.external_product(n, k, l, g_host, ct[rows]), want[rows])
    g = torch.full((k + 1, l, k + 1, n), -1, dtype=torch.int64, device="cuda")
    dct = _dev(ct)
    out = torch.empty_like(dct)
    names = _ran(B, lambda: B._check(L.fhe_tggsw_external_product_dev(n, k, l, g.data_ptr(), dct.data_ptr(), out.data_ptr(), 2, None)))
    lg = n.bit_length() - 1
    if form == "ext32":
        assert f"digit_tail32_{lg}" in names, names
    elif form == "one-prime":
        assert not _has(names, "digit_tail32") and (_has(names, "digit_tail_torus") or "zr_combine32_0" in names), names
    else:
        assert f"zr_crt_{K}" in names and not _has(names, "digit_tail"), names      # (the timer's tag: the primes used)
    assert np.array_equal(_u64(out), want), (n, k, l, form)
    words = L.fhe_tggsw_prepared_words(n, k, l)
    assert words == tggsw_words(n, k, l)
    if words:
        prep = torch.empty(words, dtype=torch.int64, device="cuda")
        out2 = torch.empty_like(out)

        def prepared():
            B._check(L.fhe_tggsw_prepare_dev(n, k, l, g.data_ptr(), prep.data_ptr(), None))
            B._check(L.fhe_tggsw_external_product_prepared_dev(n, k, l, prep.data_ptr(), dct.data_ptr(), out2.data_ptr(), 2, None))
        names2 = _ran(B, prepared)
        assert (f"digit_tail32_{lg}" in names2) == (form == "ext32"), names2
        assert torch.equal(out2, out)


KS_CASES = [(Q61, 4096, 1, 64), (Q61, 8192, 1, 64)]            # the two-27-bit-prime form at its largest n, the 61-bit one


@pytest.mark.gpu
@pytest.mark.parametrize("q,n,k,l", KS_CASES)
def test_base2_key_switch_with_every_digit_one_against_a_minus_one_key(pkg, oracle, need_gpu, q, n, k, l):
    """GLWE::key_switch (glwe.rs:126-137), base 2, with ksk = q - 1 and ciphertext words q - 1 (l = 64: Zq::decompose
    saturates, every digit is 1): out[c][j] = (c < k ? 0 : q - 1) - k l (n - 2 - 2j) mod q, the key halves' sums at
    k l n (2^32 - 1).  Plus one random row; key in coefficients and prepared; the path the rule names."""
    L, B = pkg.load_library(), pkg.binding
    import torch

    plan = pkg.Plan(q, n)
    rng = np.random.default_rng(n + l)
    glwe = np.empty((2, k + 1, n), dtype=np.uint64)
    glwe[0] = q - 1
    glwe[1] = rng.integers(0, q, (k + 1, n), dtype=np.uint64)
    ksk = np.full((k, l, k + 1, n), q - 1, dtype=np.uint64)
    want = np.empty_like(glwe)
    for i in range(2):
        oracle.glue("key_switch", q, n, k, 2, l, glwe[i], ksk, want[i])
    rhs = [(k * l * (n - 2 - 2 * j)) % q for j in range(n)]
    closed = [[(0 - r) % q for r in rhs]] * k + [[(q - 1 - r) % q for r in rhs]]
    assert np.array_equal(want[0], np.array(closed, dtype=np.uint64))
    dglwe, dksk = _dev(glwe), _dev(ksk)
    out = torch.empty_like(dglwe)
    names = _ran(B, lambda: B._check(L.fhe_glwe_key_switch_dev(plan.handle, k, 2, l, dglwe.data_ptr(), dksk.data_ptr(), out.data_ptr(), 2, 0, None)))
    lg = n.bit_length() - 1
    assert (f"digit_tail32_ks_{lg}" in names) == ks32_ok(q, n, k, l), names
    assert ks32_ok(q, n, k, l) or _has(names, "digit_tail_ks") or _has(names, "ks_tail"), names
    assert np.array_equal(_u64(out), want), (q, n, k, l)
    words = L.fhe_glwe_ksk_prepared_words(plan.handle, k, 2, l)
    assert words == (2 if ks32_ok(q, n, k, l) else 1) * ksk.size
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    out2 = torch.empty_like(out)

    def prepared():
        B._check(L.fhe_glwe_ksk_prepare_dev(plan.handle, k, 2, l, dksk.data_ptr(), prep.data_ptr(), None))
        B._check(L.fhe_glwe_key_switch_prepared_dev(plan.handle, k, 2, l, dglwe.data_ptr(), prep.data_ptr(), out2.data_ptr(), 2, None))
    names2 = _ran(B, prepared)
    assert (f"digit_tail32_ks_{lg}" in names2) == ks32_ok(q, n, k, l), names2
    assert torch.equal(out2, out)


_DIGEST_SCRIPT = r"""
import hashlib, sys
sys.path.insert(0, %r)
import numpy as np, torch
import fhe_study_amd as pkg
L, B = pkg.load_library(), pkg.binding
h = hashlib.sha256()
B.kernel_timing_reset(); B.kernel_timing_enable(True)
def full(shape, v):
    v = int(v) %% (1 << 64)
    return torch.full(shape, v - (1 << 64) if v >> 63 else v, dtype=torch.int64, device="cuda")
def take(t):
    torch.cuda.synchronize()
    h.update(t.cpu().numpy().tobytes())
for n in (1024, 2048, 4096, 8192):
    q = 1 << ((53 - (n - 1).bit_length()) // 2)
    for qq in (q, q - 1, q + 1):
        vmax = 2 * n * (qq - 1) ** 2
        for t in (2, -(-(qq << 50) // vmax), -(-(qq << 52) // vmax)):
            ab, c = full((4, 1, n), qq - 1), torch.empty((3, 1, n), dtype=torch.int64, device="cuda")
            B._check(L.fhe_bfv_tensor_dev(qq, n, t, ab.data_ptr(), c.data_ptr(), 1, None)); take(c)
for q, p in (((1 << 17) - 1, (1 << 35) - 1), ((1 << 17) - 1, (1 << 36) - 1), ((1 << 20) - 1, (1 << 42) - 1),
             ((1 << 17) - 1, 1 << 35), ((1 << 17) - 1, 1 << 13)):
    n, pq = 8192, p * q
    c, rlk, o = full((3, 1, n), q - 1), full((2, n), pq - 1), torch.empty((2, 1, n), dtype=torch.int64, device="cuda")
    B._check(L.fhe_bfv_relinearize_dev(q, n, pq, rlk.data_ptr(), c.data_ptr(), o.data_ptr(), 1, None)); take(o)
for n, k, l in ((4096, 1, 64), (8192, 15, 64), (16384, 1, 64)):
    g, ct = full((k + 1, l, k + 1, n), -1), full((1, k + 1, n), -1)
    o = torch.empty_like(ct)
    B._check(L.fhe_tggsw_external_product_dev(n, k, l, g.data_ptr(), ct.data_ptr(), o.data_ptr(), 1, None)); take(o)
for q, n, k, l in ((%d, 4096, 1, 64), (%d, 8192, 1, 64)):
    plan = pkg.Plan(q, n)
    ct, ksk = full((1, k + 1, n), q - 1), full((k, l, k + 1, n), q - 1)
    o = torch.empty_like(ct)
    B._check(L.fhe_glwe_key_switch_dev(plan.handle, k, 2, l, ct.data_ptr(), ksk.data_ptr(), o.data_ptr(), 1, 0, None)); take(o)
names = sorted(B.kernel_timing_read())
print("kernels", " ".join(names))
print("digest", h.hexdigest())
""" % (ROOT, Q61, Q61)


@pytest.mark.gpu
def test_extreme_inputs_same_words_without_the_27_bit_forms(pkg, need_gpu):
    """The extreme inputs of the tests above, in fresh processes with FHE_EXT32=0 (every product on zring's 61-bit
    forms) and with the default: identical digests; the default ran the 27-bit kernels and FHE_EXT32=0 none of them."""
    outs = {}
    for name, ext in (("default", "1"), ("ext32-off", "0")):
        env = dict(os.environ, FHE_EXT32=ext)
        r = subprocess.run([sys.executable, "-c", _DIGEST_SCRIPT], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, name + r.stdout + r.stderr
        lines = dict(l.split(" ", 1) for l in r.stdout.splitlines() if l.startswith(("digest", "kernels")))
        outs[name] = lines
    k_on, k_off = outs["default"]["kernels"].split(), outs["ext32-off"]["kernels"].split()
    for prefix in ("bfv32_tensor_inverse", "bfv32_relin_inverse", "digit_tail32_", "digit_tail32_ks"):
        assert any(s.startswith(prefix) for s in k_on), (prefix, k_on)
    assert not any(s.startswith(("bfv32_", "digit_tail32", "digit_mac32", "ntt32_")) for s in k_off), k_off
    assert outs["default"]["digest"] == outs["ext32-off"]["digest"]
