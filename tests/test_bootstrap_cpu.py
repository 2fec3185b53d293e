"""TFHE bootstrapping without a device: the numpy restatement of DESIGN.md §10 (tests/_tfhe_numpy.py) pinned against
the reference's pieces and exact integer arithmetic, a noise-free bootstrap on the CPU, and the argument checks of the
new entry points."""
import numpy as np
import pytest

import _tfhe_numpy as R


def _rand(rng, shape):
    return rng.integers(0, 1 << 64, shape, dtype=np.uint64, endpoint=False)


@pytest.mark.parametrize("n", [16, 256])
def test_rot_matches_left_rotate_and_composes(n):
    rng = np.random.default_rng(n)
    x = _rand(rng, (2, n))
    for e in (0, 1, n // 2, n - 1):
        assert np.array_equal(R.rot(x, e), R.left_rotate(x, e))
    assert np.array_equal(R.rot(x, n), np.uint64(0) - x)
    assert np.array_equal(R.rot(x, 0), x)
    for e1, e2 in ((0, 2 * n - 1), (n - 1, n + 1), (3, 5), (2 * n - 1, 2 * n - 1), (n, n), (7, n - 3)):
        assert np.array_equal(R.rot(R.rot(x, e1), e2), R.rot(x, (e1 + e2) % (2 * n)))


@pytest.mark.parametrize("n", [16, 256, 1024, 4096])
def test_mod_switch_rounds_at_the_edges(n):
    L = n.bit_length() - 1
    half, q = 1 << (62 - L), 1 << (63 - L)       # half a slot, one slot of 2N
    words = [0, 1, half - 1, half, half + 1, q - 1, q, q + half - 1, q + half, q + half + 1,
             (1 << 63) - half - 1, (1 << 63) - half, 1 << 63, (1 << 64) - half - 1, (1 << 64) - half, (1 << 64) - 1]
    got = R.mod_switch(np.array(words, dtype=np.uint64), n)
    want = [R.mod_switch_exact(w, n) for w in words]
    assert [int(g) for g in got] == want
    assert want[0] == 0 and want[3] == 1 and want[2] == 0 and want[-1] == 0 and want[-2] == 0
    rng = np.random.default_rng(L)
    w = _rand(rng, 4000)
    assert [int(g) for g in R.mod_switch(w, n)] == [R.mod_switch_exact(int(x), n) for x in w]


def test_sample_extraction_and_key_switch_restatements():
    """sample extraction at h of a TGLWE decrypts to coefficient h of its phase; the key switch keeps the phase"""
    rng = np.random.default_rng(5)
    n = 16
    s = rng.integers(0, 2, n, dtype=np.uint64)
    a = _rand(rng, (3, n))
    b = _rand(rng, (3, n))
    from oracle import load_oracle

    O = load_oracle()
    phase = b - O.tn_mul(n, a, np.broadcast_to(s, (3, n)).copy())
    ct = np.stack([a, b], axis=1)
    for h in (0, 1, n - 1):
        tl = R.sample_extraction(ct, h)
        assert np.array_equal(tl[:, -1] - tl[:, :-1] @ s, phase[:, h])
    s_out = rng.integers(0, 2, 5, dtype=np.uint64)
    k = R.ksk(rng, s, s_out, 64, 0)
    tl = R.sample_extraction(ct, 3)
    out = R.key_switch(k, tl, 64)
    diff = (out[:, -1] - out[:, :-1] @ s_out) - phase[:, 3]
    assert all(abs(int(np.int64(x))) < 64 * n for x in diff.view(np.int64))        # gadget u64::MAX / 2^d, not 2^(64-d)


def test_noise_free_cpu_bootstrap(oracle):
    """N = 256, k = 1, l = 64, n_lwe = 8, t = 16 with a bit of padding: every m in [0, 8) bootstraps to f(m)"""
    n, k, l, n_lwe, t = 256, 1, 64, 8, 16
    rng = np.random.default_rng(2024)
    s_glwe = rng.integers(0, 2, n, dtype=np.uint64)
    s_lwe = rng.integers(0, 2, n_lwe, dtype=np.uint64)
    mul = lambda a, b: oracle.tn_mul(n, a, np.ascontiguousarray(b))
    bsk = R.tggsw_bits(rng, mul, n, l, s_glwe, s_lwe, 0)
    ks = R.ksk(rng, s_glwe, s_lwe, 64, 0)
    f = lambda m: (3 * m + 5) % 8
    table = R.test_vector(n, t, f)
    delta = ((1 << 64) - 1) // t
    msgs = np.arange(8)
    lwe = R.lwe_encrypt(rng, s_lwe, [m * delta for m in msgs], 0)
    ext = lambda j, d: oracle.external_product(n, k, l, bsk[j], d)
    out = R.bootstrap(ext, n, k, l, bsk, table, ks, 64, lwe)
    assert out.shape == (8, n_lwe + 1)
    assert list(R.lwe_decode(out, s_lwe, t)) == [f(m) for m in msgs]
    # the blind rotation alone decrypts to X^-phi v under the GLWE key
    acc = R.blind_rotation(ext, n, k, l, bsk, table, lwe[:2])
    ph = acc[:, 1] - oracle.tn_mul(n, acc[:, 0], np.broadcast_to(s_glwe, (2, n)).copy())
    assert [int(round(float(int(x)) * t / 2.0 ** 64)) % t for x in ph[:, 0]] == [f(0), f(1)]


def test_bootstrap_entry_points_validate_before_touching_the_gpu(pkg):
    """argument errors of the TFHE bootstrapping entry points are reported without a device"""
    L, B = pkg.load_library(), pkg.binding
    d = 16                                     # any non-NULL, 16-byte aligned fake device address: validation must fail first
    far = 1 << 40
    # sizes without a device
    words = L.fhe_tggsw_prepared_words(1024, 1, 64)
    assert words > 0 and L.fhe_tfhe_bsk_prepared_words(1024, 1, 64, 630) == 630 * words
    assert L.fhe_tfhe_bsk_prepared_words(1024, 1, 64, 0) == 0
    assert L.fhe_tfhe_bsk_prepared_words(16384, 1, 64, 10) == 0            # no prepared TGGSW form
    assert L.fhe_tfhe_bsk_prepared_words(1024, 1, 65, 10) == 0
    # blind rotation / preparation: l, n, n_lwe, NULL, overlap
    assert L.fhe_tfhe_blind_rotation_dev(1024, 1, 0, 8, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_blind_rotation_dev(1024, 1, 65, 8, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_blind_rotation_dev(1000, 1, 64, 8, d, d, d, d, 1, None) == B.FHE_E_BAD_N
    assert L.fhe_tfhe_blind_rotation_dev(1024, 1, 64, 0, d, d, d, d, 1, None) == B.FHE_E_INVALID
    assert b"n_lwe" in L.fhe_last_error()
    assert L.fhe_tfhe_blind_rotation_dev(16384, 1, 64, 8, d, d, d, d, 1, None) == B.FHE_E_INVALID   # no prepared form
    assert L.fhe_tfhe_blind_rotation_dev(1024, 1, 64, 8, None, d, d, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tfhe_blind_rotation_dev(1024, 1, 64, 8, far, far + (1 << 30), far + (1 << 31), far + (1 << 31) + 64, 1, None) == B.FHE_E_INVALID
    assert b"overlap" in L.fhe_last_error()
    assert L.fhe_tfhe_blind_rotation_dev(1024, 1, 64, 8, None, None, None, None, 0, None) == B.FHE_OK     # empty batch
    assert L.fhe_tfhe_bsk_prepare_dev(1024, 1, 65, 8, d, d, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_bsk_prepare_dev(1024, 1, 64, 0, d, d, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_bsk_prepare_dev(1024, 1, 64, 8, None, d, None) == B.FHE_E_NULL
    assert L.fhe_tfhe_bsk_prepare_dev(1024, 1, 64, 8, far, far + 4096, None) == B.FHE_E_INVALID            # overlapping
    # sample extraction: h < n
    assert L.fhe_tglwe_sample_extraction_dev(256, 1, 256, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tglwe_sample_extraction_dev(255, 1, 0, d, d, 1, None) == B.FHE_E_BAD_N
    assert L.fhe_tglwe_sample_extraction_dev(256, 1, 255, None, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tglwe_sample_extraction_dev(256, 1, 0, far, far + 8, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tglwe_sample_extraction_dev(256, 1, 0, None, None, 0, None) == B.FHE_OK
    # key switch: beta = 2 only, 1 <= l <= 64
    assert L.fhe_tlwe_key_switch_dev(1024, 630, 4, 32, d, d, d, 1, None) == B.FHE_E_INVALID
    assert b"beta" in L.fhe_last_error()
    assert L.fhe_tlwe_key_switch_dev(1024, 630, 2, 0, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_key_switch_dev(1024, 630, 2, 65, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_key_switch_dev(0, 630, 2, 64, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_key_switch_dev(1024, 630, 2, 64, d, None, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tlwe_key_switch_dev(1024, 630, 2, 64, far, far + (1 << 32), far + (1 << 32) + 8, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tlwe_key_switch_dev(1024, 630, 2, 64, None, None, None, 0, None) == B.FHE_OK
    # bootstrap: both sets of checks
    assert L.fhe_tfhe_bootstrap_dev(1024, 1, 64, 630, d, d, 65, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_bootstrap_dev(1024, 1, 0, 630, d, d, 64, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_bootstrap_dev(1024, 1, 64, 0, d, d, 64, d, d, d, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_bootstrap_dev(1024, 1, 64, 630, d, d, 64, None, d, d, 1, None) == B.FHE_E_NULL
    assert L.fhe_tfhe_bootstrap_dev(1024, 1, 64, 630, far, far + (1 << 32), 64, far + (1 << 33), far + (1 << 36), far + (1 << 36) + 8, 1, None) == B.FHE_E_INVALID
    assert L.fhe_tfhe_bootstrap_dev(1024, 1, 64, 630, None, None, 64, None, None, None, 0, None) == B.FHE_OK
