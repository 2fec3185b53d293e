"""Circuit bootstrapping of DESIGN.md §12 without a device: the numpy restatement (tests/_cb_numpy.py) with noise-free
keys — the PFKS computes f_r of the phase within its rounding bound, a circuit bootstrap at N = 256 gives a TGGSW of the
bit, and a CMux with it selects — and the argument checks and word counts of the new entry points."""
import numpy as np
import pytest

import _cb_numpy as CB
import _gadget_numpy as G
import _tfhe_numpy as R


@pytest.mark.parametrize("b,l", [(8, 4), (4, 4), (1, 64), (16, 4), (32, 2), (3, 7)])
def test_noise_free_pfks_is_f_of_the_phase_within_the_rounding_bound(oracle, b, l):
    n = 256
    rng = np.random.default_rng(700 + b * 10 + l)
    mul = lambda a, x: oracle.tn_mul(n, a, np.ascontiguousarray(x))
    s = rng.integers(0, 2, n, dtype=np.uint64)
    key = CB.pfksk(rng, mul, n, s, b, l, 0)
    assert key.shape == (2, n + 1, l, 2, n)
    c = rng.integers(0, 1 << 64, (3, n + 1), dtype=np.uint64, endpoint=False)
    out = CB.private_key_switch(key, c, b, l)                                # [3][2 functions][2][n]
    ph = CB.tlwe_phase(c, s)
    p1 = CB.tglwe_phase(mul, out[:, 1], s)                                   # f_1(x) = x: the phase at coefficient 0
    p0 = CB.tglwe_phase(mul, out[:, 0], s)                                   # f_0(x) = -s x
    sh = 64 - b * l
    bound = (n + 1) * ((1 << (sh - 1)) if sh else 0)                         # sum_j |c_j - c~_j| |K~_j|
    assert np.all(p1[:, 1:] == 0)
    err = CB.centred(p1[:, 0] - ph)
    assert np.all(np.abs(err.astype(object)) <= bound)
    if sh == 0:
        assert np.all(err == 0)
    # f_0 of the same rounded phase, exactly: -s (phase + err)
    assert np.array_equal(p0, (np.uint64(0) - s)[None, :] * p1[:, :1])


def test_pfks_restatement_is_a_sum_of_digit_rows():
    """the GEMM form against the definition's double sum, one word at a time"""
    n, b, l = 256, 8, 4
    rng = np.random.default_rng(5)
    key = rng.integers(0, 1 << 64, (2, n + 1, l, 2, n), dtype=np.uint64, endpoint=False)
    c = rng.integers(0, 1 << 64, (2, n + 1), dtype=np.uint64, endpoint=False)
    got = CB.private_key_switch(key, c, b, l)
    for m in range(2):
        want = np.zeros((2, 2, n), dtype=np.uint64)
        for j in range(n + 1):
            _, digits = G.decompose_exact(int(c[m, j]), b, l)
            for d in range(l):
                want += np.uint64(digits[d] % (1 << 64)) * key[:, j, d]
        assert np.array_equal(got[m], want)


def test_noise_free_circuit_bootstrap_gives_a_tggsw_of_the_bit_and_its_cmux_selects(oracle):
    """N = 256, n_lwe = 8, BSK (10, 3), CB (6, 2), PFKS (8, 4), noise-free keys: row (1, d) has phase mu g_d and row (0, d)
    -s mu g_d within the bound; a CMux with the TGGSW picks c1 for mu = 1 and c0 for mu = 0"""
    n, n_lwe, b, l, cb_b, cb_l, pf_b, pf_l = 256, 8, 10, 3, 6, 2, 8, 4
    rng = np.random.default_rng(12)
    mul = lambda a, x: oracle.tn_mul(n, a, np.ascontiguousarray(x))
    s = rng.integers(0, 2, n, dtype=np.uint64)
    s_lwe = rng.integers(0, 2, n_lwe, dtype=np.uint64)
    bsk = G.tggsw_bits(rng, mul, n, b, l, s, s_lwe, 0)
    pf = CB.pfksk(rng, mul, n, s, pf_b, pf_l, 0)
    mus = [0, 1, 1, 0]
    lwe = R.lwe_encrypt(rng, s_lwe, [m << 63 for m in mus], 0)
    tg = CB.circuit_bootstrap(n, b, l, bsk, cb_b, cb_l, pf_b, pf_l, pf, lwe)
    assert tg.shape == (4, 2, cb_l, 2, n)
    g = G.gvalues(cb_b, cb_l)
    # blind rotation: n_lwe CMux steps, each off by its rounding (N + 1) 2^(s-1); then the PFKS rounding (N + 1) 2^(s_p - 1)
    bound = n_lwe * (n + 1) * (1 << (64 - b * l - 1)) + (n + 1) * (1 << (64 - pf_b * pf_l - 1))
    worst = 0
    for i, mu in enumerate(mus):
        for d in range(cb_l):
            want1 = np.zeros(n, dtype=np.uint64)
            want1[0] = np.uint64(mu * g[d])
            e1 = CB.centred(CB.tglwe_phase(mul, tg[i, 1, d], s) - want1).astype(object)
            e0 = CB.centred(CB.tglwe_phase(mul, tg[i, 0, d], s) - (np.uint64(0) - s) * np.uint64(mu * g[d])).astype(object)
            worst = max(worst, max(abs(x) for x in e1), max(abs(x) for x in e0))
    assert worst <= bound < CB.alpha(cb_b, cb_l - 1)
    # the CMux: t = 16, messages m 2^60
    msgs = np.array([[3, 11], [5, 2], [7, 7], [1, 14]])
    c0 = np.zeros((4, 2, n), dtype=np.uint64)
    c1 = np.zeros((4, 2, n), dtype=np.uint64)
    for i in range(4):
        for ct, m in ((c0, msgs[i, 0]), (c1, msgs[i, 1])):
            a = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)
            v = np.zeros(n, dtype=np.uint64)
            v[0] = np.uint64(int(m) << 60)
            ct[i, 0] = a
            ct[i, 1] = mul(a[None], s[None].copy())[0] + v
    out = CB.cmux(tg, np.arange(4), c0, c1, cb_b)
    ph = CB.tglwe_phase(mul, out, s)
    got = [int(((int(x) + (1 << 59)) >> 60) % 16) for x in ph[:, 0]]
    assert got == [int(msgs[i, mus[i]]) for i in range(4)]
    # an index past the keys selects nothing
    assert np.array_equal(CB.cmux(tg, [4, 9], c0[:2], c1[:2], cb_b), c0[:2])


def test_word_counts_follow_the_rules(pkg):
    L = pkg.load_library()
    assert L.fhe_tfhe_pfksk_words(1024, 1, 8, 4) == 2 * 1025 * 4 * 2 * 1024        # 134 MB
    assert L.fhe_tfhe_pfksk_words(256, 1, 1, 64) == 2 * 257 * 64 * 2 * 256
    assert L.fhe_tfhe_pfksk_words(4096, 1, 32, 2) == 2 * 4097 * 2 * 2 * 4096
    for shape in [(1024, 1, 0, 4), (1024, 1, 33, 1), (1024, 1, 8, 9), (1024, 1, 8, 0), (1024, 2, 8, 4), (1024, 0, 8, 4),
                  (128, 1, 8, 4), (8192, 1, 8, 4), (1000, 1, 8, 4)]:
        assert L.fhe_tfhe_pfksk_words(*shape) == 0, shape


def test_circuit_bootstrap_entry_points_validate_before_touching_the_gpu(pkg):
    L, B = pkg.load_library(), pkg.binding
    d = 16                                     # any non-NULL, 16-byte aligned fake device address: validation must fail first
    far = 1 << 40
    # PFKS: k = 1, 256 <= n <= 4096, 1 <= b <= 32, b l <= 64
    pk = L.fhe_tlwe_gadget_private_key_switch_dev
    assert pk(1024, 1, 33, 1, d, d, d, 1, None) == B.FHE_E_INVALID
    assert pk(1024, 1, 0, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert pk(1024, 1, 8, 9, d, d, d, 1, None) == B.FHE_E_INVALID                 # b l = 72
    assert pk(1024, 1, 8, 0, d, d, d, 1, None) == B.FHE_E_INVALID
    assert pk(1024, 2, 8, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert pk(8192, 1, 8, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert pk(128, 1, 8, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert pk(1000, 1, 8, 4, d, d, d, 1, None) == B.FHE_E_BAD_N
    assert pk(1024, 1, 8, 4, None, d, d, 1, None) == B.FHE_E_NULL
    assert pk(1024, 1, 8, 4, d, d, 24, 1, None) == B.FHE_E_INVALID               # misaligned
    assert pk(1024, 1, 8, 4, far, far + (1 << 30), far + (1 << 30) + 64, 1, None) == B.FHE_E_INVALID
    assert b"overlap" in L.fhe_last_error()
    assert pk(1024, 1, 8, 4, far, far + (1 << 30), far + 64, 1, None) == B.FHE_E_INVALID   # d_out inside the key
    assert pk(1024, 1, 8, 4, None, None, None, 0, None) == B.FHE_OK
    # preparation of many
    pm = L.fhe_tggsw_gadget_prepare_many_dev
    assert pm(1024, 1, 11, 2, 4, d, d, None) == B.FHE_E_INVALID
    assert b"log_beta" in L.fhe_last_error()
    assert pm(1000, 1, 6, 2, 4, d, d, None) == B.FHE_E_BAD_N
    assert pm(1024, 1, 6, 2, 4, None, d, None) == B.FHE_E_NULL
    assert pm(1024, 1, 6, 2, 4, far, far + 4096, None) == B.FHE_E_INVALID
    assert pm(1024, 1, 6, 2, 1 << 60, d, d, None) == B.FHE_E_INVALID
    assert pm(1024, 1, 6, 2, 0, None, None, None) == B.FHE_OK
    # CMux with a selector per ciphertext
    cm = L.fhe_tggsw_gadget_cmux_dev
    assert cm(1024, 1, 11, 2, 4, d, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert cm(4096, 1, 9, 2, 4, d, d, d, d, d, 1, None) == B.FHE_E_INVALID       # one step past N = 4096, l = 2: b <= 8
    assert cm(1024, 1, 6, 0, 4, d, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert cm(1024, 1, 6, 2, 0, d, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert b"count" in L.fhe_last_error()
    assert cm(1024, 1, 6, 2, 1 << 32, d, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert cm(1000, 1, 6, 2, 4, d, d, d, d, d, 1, None) == B.FHE_E_BAD_N
    for i in range(5):
        args = [d] * 5
        args[i] = None
        assert cm(1024, 1, 6, 2, 4, *args, 1, None) == B.FHE_E_NULL
    ct = 2 * 1024 * 8
    base = [far, far + (1 << 30), far + (1 << 31), far + (1 << 32), far + (1 << 33)]   # prepared, idx, c0, c1, out
    for i, at in enumerate([far + 64, far + (1 << 30), far + (1 << 31) + ct - 16, far + (1 << 32) + 64]):
        args = list(base)
        args[4] = at
        assert cm(1024, 1, 6, 2, 4, *args, 1, None) == B.FHE_E_INVALID, i
        assert b"overlap" in L.fhe_last_error()
    assert cm(1024, 1, 6, 2, 4, None, None, None, None, None, 0, None) == B.FHE_OK
    # circuit bootstrap: BSK, CB and PFKS shapes each checked, and cb_b cb_l <= 63
    cb = L.fhe_tfhe_circuit_bootstrap_dev
    ok = (1024, 1, 10, 3, 630, d, 6, 2, 8, 4, d, d, d, 1, None)
    bad = [(2, 11), (3, 4), (4, 0), (6, 11), (7, 0), (8, 33), (9, 9), (8, 0), (1, 2), (0, 1000)]
    for pos, v in bad:
        args = list(ok)
        args[pos] = v
        rc = cb(*args)
        assert rc in (B.FHE_E_INVALID, B.FHE_E_BAD_N), (pos, v)
    assert cb(1024, 1, 10, 3, 0, d, 6, 2, 8, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert b"n_lwe" in L.fhe_last_error()
    # cb (8, 8) is an admitted product at N = 256 but alpha_7 = 2^-1: refused
    assert L.fhe_tggsw_gadget_prepared_words(256, 1, 8, 8) > 0
    assert cb(256, 1, 10, 3, 8, d, 8, 8, 8, 4, d, d, d, 1, None) == B.FHE_E_INVALID
    assert b"63" in L.fhe_last_error()
    for i in (5, 10, 11, 12):
        args = list(ok)
        args[i] = None
        assert cb(*args) == B.FHE_E_NULL, i
    nl, w = 630, L.fhe_tggsw_gadget_prepared_words(1024, 1, 10, 3)
    bsk_b, pf_b = nl * w * 8, L.fhe_tfhe_pfksk_words(1024, 1, 8, 4) * 8
    k_at, pf_at, lwe_at = far, far + (1 << 36), far + (1 << 37)
    for out in (k_at + bsk_b - 16, pf_at + 64, lwe_at + 16):
        assert cb(1024, 1, 10, 3, nl, k_at, 6, 2, 8, 4, pf_at, lwe_at, out, 1, None) == B.FHE_E_INVALID
        assert b"overlap" in L.fhe_last_error()
    assert pf_b < (1 << 37) - (1 << 36)
    assert cb(1024, 1, 10, 3, 630, None, 6, 2, 8, 4, None, None, None, 0, None) == B.FHE_OK


def test_python_surface_refuses_bad_shapes(pkg):
    from fhe_study_amd import tfhe

    with pytest.raises(ValueError):
        tfhe.PreparedTGGSWs(np.zeros((2, 2, 2, 3, 256), dtype=np.uint64), 6)
    with pytest.raises(ValueError):
        tfhe.CircuitBootstrappingKey(type("K", (), {"log_beta": None})(), None, 6, 2, 8, 4)
