"""The signed base-2^b gadget of DESIGN.md §11 without a device: the numpy restatement (tests/_gadget_numpy.py) against
Python integers, a noise-free gadget bootstrap on the CPU, the admission rule at its edges, and the argument checks of
the new entry points."""
import numpy as np
import pytest

import _gadget_numpy as G
import _tfhe_numpy as R

SHAPES = [(1, 64), (2, 32), (4, 4), (4, 16), (8, 3), (8, 8), (10, 2), (10, 3), (13, 4), (16, 4), (32, 2), (64, 1), (7, 9), (3, 5)]


def _edge_words(b, l):
    s = 64 - b * l
    B = sum((1 << (b - 1)) << (b * i) for i in range(l))
    words = [0, 1, (1 << 64) - 1, 1 << 63, (1 << 63) - 1, ((1 << (b * l)) - B) % (1 << (b * l)) << s]   # the last: all -2^(b-1)
    if s:
        words += [(1 << (s - 1)) - 1, 1 << (s - 1), (1 << (s - 1)) + 1, (1 << 64) - (1 << (s - 1)), (1 << 64) - (1 << (s - 1)) - 1]
    return words


@pytest.mark.parametrize("b,l", SHAPES)
def test_decomposition_recomposes_rounds_and_stays_in_range(b, l):
    s = 64 - b * l
    g = G.gvalues(b, l)
    rng = np.random.default_rng(b * 100 + l)
    words = _edge_words(b, l) + [int(x) for x in rng.integers(0, 1 << 64, 300, dtype=np.uint64, endpoint=False)]
    got = G.decompose(np.array(words, dtype=np.uint64), b, l)
    for w, row in zip(words, got):
        xt, digits = G.decompose_exact(w, b, l)
        assert [int(x) for x in row] == digits
        assert all(-(1 << (b - 1)) <= x < (1 << (b - 1)) for x in digits)
        rec = sum(x * gd for x, gd in zip(digits, g)) % (1 << 64)
        assert rec == (xt << s) % (1 << 64)
        err = (w - rec) % (1 << 64)
        err = err - (1 << 64) if err >= 1 << 63 else err                  # centred
        assert abs(err) <= (1 << (s - 1) if s else 0)
        assert xt == (((w + (1 << (s - 1))) >> s) if s else w) % (1 << (b * l))     # round half up
    # the all-(-2^(b-1)) word
    w = _edge_words(b, l)[5]
    assert G.decompose_exact(w, b, l)[1] == [-(1 << (b - 1))] * l


def test_gadget_product_restatement_is_the_message_times_the_rounded_word():
    """noise-free gadget TGGSW of m = 1 under a key s: the product decrypts to the rounded phase of the input"""
    from oracle import load_oracle

    O = load_oracle()
    n, b, l = 16, 8, 3
    rng = np.random.default_rng(3)
    s = rng.integers(0, 2, n, dtype=np.uint64)
    mul = lambda a, x: O.tn_mul(n, a, np.ascontiguousarray(x))
    key = G.tggsw_bits(rng, mul, n, b, l, s, [1], 0)[0]
    ct = rng.integers(0, 1 << 64, (2, 2, n), dtype=np.uint64, endpoint=False)
    out = G.external_product(key, ct, b)
    phase = lambda c: c[:, 1] - O.tn_mul(n, np.ascontiguousarray(c[:, 0]), np.broadcast_to(s, (len(c), n)).copy())
    diff = (phase(out) - phase(ct)).view(np.int64)
    assert np.all(np.abs(diff) <= (n + 1) << (64 - b * l - 1))           # |a - a~| s + |b - b~| per coefficient
    # the product is linear in the digits: Toeplitz product against the oracle's schoolbook
    x = rng.integers(0, 1 << 64, (3, n), dtype=np.uint64, endpoint=False)
    assert np.array_equal(G.negacyclic(key[0, 0, 0], x), O.tn_mul(n, x, np.broadcast_to(key[0, 0, 0], (3, n)).copy()))


@pytest.mark.parametrize("n", [256, 512])
def test_row_product_restatement_equals_the_toeplitz_one(oracle, n):
    """G.external_product_rows (digit rows against key rows through the oracle's schoolbook tn_mul) word for word against
    G.external_product (the u64 Toeplitz matmul), at every (b, l) of SHAPES that the rule admits, with the edge words in
    the first row, a row whose digits are all -2^(b-1), and a key with a band of 2^64 - 1"""
    mul = lambda x, y: oracle.tn_mul(n, x, y)
    ran = []
    for b, l in SHAPES:
        if not admitted(n, 1, b, l):
            continue
        ran.append((b, l))
        rng = np.random.default_rng(n + 100 * b + l)
        key = rng.integers(0, 1 << 64, (2, l, 2, n), dtype=np.uint64, endpoint=False)
        key[1, l - 1, :, : n // 4] = np.uint64((1 << 64) - 1)
        ct = rng.integers(0, 1 << 64, (3, 2, n), dtype=np.uint64, endpoint=False)
        edges = _edge_words(b, l)
        ct[0, 0, : len(edges)] = edges
        ct[0, 1, n - len(edges):] = edges
        ct[1] = np.uint64(edges[5])
        assert np.array_equal(G.external_product_rows(mul, key, ct, b), G.external_product(key, ct, b)), (b, l)
    assert {(1, 64), (2, 32), (4, 16), (8, 8), (8, 3), (10, 2), (7, 9), (3, 5)} <= set(ran)      # (13, 4) and wider are refused


@pytest.mark.parametrize("b,l,ks_b,ks_l", [(8, 3, 4, 4), (10, 2, 2, 10)])
def test_noise_free_cpu_gadget_bootstrap(oracle, b, l, ks_b, ks_l):
    """N = 256, k = 1, n_lwe = 8, t = 16 with a bit of padding: every m in [0, 8) bootstraps to f(m)"""
    n, k, n_lwe, t = 256, 1, 8, 16
    rng = np.random.default_rng(2025 + b)
    s_glwe = rng.integers(0, 2, n, dtype=np.uint64)
    s_lwe = rng.integers(0, 2, n_lwe, dtype=np.uint64)
    mul = lambda a, x: oracle.tn_mul(n, a, np.ascontiguousarray(x))
    bsk = G.tggsw_bits(rng, mul, n, b, l, s_glwe, s_lwe, 0)
    ks = G.ksk(rng, s_glwe, s_lwe, ks_b, ks_l, 0)
    f = lambda m: (5 * m + 1) % 8
    table = R.test_vector(n, t, f)
    delta = ((1 << 64) - 1) // t
    lwe = R.lwe_encrypt(rng, s_lwe, [m * delta for m in range(8)], 0)
    out = G.bootstrap(n, k, b, l, bsk, table, ks_b, ks_l, ks, lwe)
    assert out.shape == (8, n_lwe + 1)
    assert list(R.lwe_decode(out, s_lwe, t)) == [f(m) for m in range(8)]


# ---- the admission rule, restated from digit32.hip ext32_gadget_supported: k = 1, 2^8 <= n <= 2^12, 1 <= b, b l <= 64,
# and 2 (k+1) l n (2^32 - 1) 2^(b-1) < pA pB (digit32.hpp kExt32PrimeA, kExt32PrimeB: the centred lift of an odd P)
PA, PB = 0x0A3C8001, 0x0A320001


def admitted(n, k, b, l):
    if k != 1 or l < 1 or b < 1 or b * l > 64 or n < 256 or n > 4096 or n & (n - 1):
        return False
    return 2 * (k + 1) * l * n * ((1 << 32) - 1) * (1 << (b - 1)) < PA * PB


@pytest.mark.parametrize("n,l,b_max,bound", [(1024, 2, 10, (1 << 53) - (1 << 21)), (1024, 3, 10, None), (4096, 2, 8, (1 << 53) - (1 << 21))])
def test_admission_edges(pkg, n, l, b_max, bound):
    L = pkg.load_library()
    assert admitted(n, 1, b_max, l) and not admitted(n, 1, b_max + 1, l)
    worst = 2 * l * n * ((1 << 32) - 1) * (1 << (b_max - 1))
    if bound is not None:
        assert worst == bound
    assert worst < PA * PB // 2 < 2 * worst
    want = 2 * 2 * l * 2 * n
    assert L.fhe_tggsw_gadget_prepared_words(n, 1, b_max, l) == want
    assert L.fhe_tggsw_gadget_prepared_words(n, 1, b_max + 1, l) == 0
    assert L.fhe_tfhe_gadget_bsk_prepared_words(n, 1, b_max, l, 630) == 630 * want
    assert L.fhe_tfhe_gadget_bsk_prepared_words(n, 1, b_max + 1, l, 630) == 0


def test_admission_rule_matches_the_library_on_a_grid(pkg):
    L = pkg.load_library()
    for n in (128, 256, 512, 1000, 1024, 2048, 4096, 8192):
        for k in (1, 2):
            for l in (1, 2, 3, 4, 8, 32, 64, 65):
                for b in range(0, 18):
                    got = L.fhe_tggsw_gadget_prepared_words(n, k, b, l)
                    assert (got != 0) == admitted(n, k, b, l), (n, k, b, l)


def test_gadget_entry_points_validate_before_touching_the_gpu(pkg):
    L, B = pkg.load_library(), pkg.binding
    d = 16                                     # any non-NULL, 16-byte aligned fake device address: validation must fail first
    far = 1 << 40
    # the beta = 2 key switch still refuses any other base
    assert L.fhe_tlwe_key_switch_dev(1024, 630, 4, 32, d, d, d, 1, None) == B.FHE_E_INVALID
    # decomposition
    assert L.fhe_tn_gadget_decompose_dev(1000, 8, 3, d, d, 1, None) == B.FHE_E_BAD_N
    assert L.fhe_tn_gadget_decompose_dev(1024, 0, 3, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tn_gadget_decompose_dev(1024, 8, 9, d, d, 1, None) == B.FHE_E_INVALID     # b l = 72
    assert L.fhe_tn_gadget_decompose_dev(1024, 8, 0, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tn_gadget_decompose_dev(1024, 8, 3, None, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tn_gadget_decompose_dev(1024, 8, 3, far, far + 8, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tn_gadget_decompose_dev(1024, 8, 3, None, None, 0, None) == B.FHE_OK
    # preparation and product: the admission rule, NULL, overlap
    assert L.fhe_tggsw_gadget_prepare_dev(1024, 1, 11, 2, d, d, None) == B.FHE_E_INVALID
    assert b"log_beta" in L.fhe_last_error()
    assert L.fhe_tggsw_gadget_prepare_dev(1024, 2, 8, 3, d, d, None) == B.FHE_E_INVALID
    assert L.fhe_tggsw_gadget_prepare_dev(1000, 1, 8, 3, d, d, None) == B.FHE_E_BAD_N
    assert L.fhe_tggsw_gadget_prepare_dev(1024, 1, 8, 3, None, d, None) == B.FHE_E_NULL
    assert L.fhe_tggsw_gadget_prepare_dev(1024, 1, 8, 3, far, far + 4096, None) == B.FHE_E_INVALID
    assert L.fhe_tggsw_gadget_external_product_dev(1024, 1, 11, 2, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tggsw_gadget_external_product_dev(1024, 1, 8, 0, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tggsw_gadget_external_product_dev(1024, 1, 8, 3, d, None, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tggsw_gadget_external_product_dev(1024, 1, 8, 3, far, far + (1 << 30), far + (1 << 30) + 64, 1, None) == B.FHE_E_INVALID
    assert b"overlap" in L.fhe_last_error()
    assert L.fhe_tggsw_gadget_external_product_dev(1024, 1, 8, 3, None, None, None, 0, None) == B.FHE_OK
    # bootstrapping key, blind rotation
    assert L.fhe_tfhe_gadget_bsk_prepared_words(1024, 1, 8, 3, 0) == 0
    assert L.fhe_tfhe_gadget_bsk_prepare_dev(1024, 1, 8, 3, 0, d, d, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_bsk_prepare_dev(1024, 1, 8, 3, 8, None, d, None) == B.FHE_E_NULL
    assert L.fhe_tfhe_gadget_bsk_prepare_dev(1024, 1, 8, 3, 8, far, far + 4096, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_blind_rotation_dev(1024, 1, 8, 3, 0, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert b"n_lwe" in L.fhe_last_error()
    assert L.fhe_tfhe_gadget_blind_rotation_dev(1024, 1, 11, 3, 8, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_blind_rotation_dev(16384, 1, 8, 3, 8, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_blind_rotation_dev(1000, 1, 8, 3, 8, d, d, d, d, 1, None) == B.FHE_E_BAD_N
    assert L.fhe_tfhe_gadget_blind_rotation_dev(1024, 1, 8, 3, 8, None, d, d, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tfhe_gadget_blind_rotation_dev(1024, 1, 8, 3, 8, far, far + (1 << 30), far + (1 << 31), far + (1 << 31) + 64, 1,
                                                None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_blind_rotation_dev(1024, 1, 8, 3, 8, None, None, None, None, 0, None) == B.FHE_OK
    # key switch: 1 <= b <= 32, b l <= 64
    assert L.fhe_tlwe_gadget_key_switch_dev(1024, 630, 0, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_gadget_key_switch_dev(1024, 630, 33, 1, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_gadget_key_switch_dev(1024, 630, 4, 17, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_gadget_key_switch_dev(1024, 630, 4, 0, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_gadget_key_switch_dev(0, 630, 4, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_gadget_key_switch_dev(1024, 630, 4, 4, d, None, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tlwe_gadget_key_switch_dev(1024, 630, 4, 4, far, far + (1 << 32), far + (1 << 32) + 8, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_gadget_key_switch_dev(1024, 630, 4, 4, None, None, None, 0, None) == B.FHE_OK
    # bootstrap: both sets of checks
    assert L.fhe_tfhe_gadget_bootstrap_dev(1024, 1, 8, 3, 630, d, d, 4, 17, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_bootstrap_dev(1024, 1, 8, 3, 630, d, d, 33, 1, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_bootstrap_dev(1024, 1, 11, 3, 630, d, d, 4, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_bootstrap_dev(1024, 1, 8, 3, 0, d, d, 4, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_bootstrap_dev(1024, 1, 8, 3, 630, d, d, 4, 4, None, d, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tfhe_gadget_bootstrap_dev(1024, 1, 8, 3, 630, far, far + (1 << 32), 4, 4, far + (1 << 33), far + (1 << 36),
                                           far + (1 << 36) + 8, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_gadget_bootstrap_dev(1024, 1, 8, 3, 630, None, None, 4, 4, None, None, None, 0, None) == B.FHE_OK
