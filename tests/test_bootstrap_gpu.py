"""TFHE bootstrapping on the device (tfhe_boot.hip, the CMux modes of digit32.hip): word-exact against the numpy
restatement of DESIGN.md §10 (tests/_tfhe_numpy.py), and a functional bootstrap with real keys."""
import numpy as np
import pytest

import _tfhe_numpy as R

pytestmark = pytest.mark.gpu


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _rand_dev(shape, seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, dtype=torch.int64, device="cuda", generator=g)


def _edge_lwe(rng, batch, n_lwe, n):
    """random ciphertexts; the first two carry the edge words: a~ in {0, N, 2N-1}, b~ = 0"""
    L = n.bit_length() - 1
    lwe = rng.integers(0, 1 << 64, (batch, n_lwe + 1), dtype=np.uint64, endpoint=False)
    edges = [0, 1 << 63, (2 * n - 1) << (63 - L), (1 << 64) - 1, (1 << (62 - L)) - 1, 1 << (62 - L)]
    for i in range(n_lwe):
        lwe[0, i] = edges[i % len(edges)]
    lwe[0, n_lwe] = (1 << 64) - 1                                    # rounds to 2N = 0
    lwe[1, n_lwe] = 0
    return lwe


def _prepare(L, B, n, k, l, n_lwe, bsk):
    import torch

    words = L.fhe_tfhe_bsk_prepared_words(n, k, l, n_lwe)
    assert words == n_lwe * L.fhe_tggsw_prepared_words(n, k, l) > 0
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    B._check(L.fhe_tfhe_bsk_prepare_dev(n, k, l, n_lwe, bsk.data_ptr(), prep.data_ptr(), None))
    return prep


@pytest.mark.parametrize("n,k,l,n_lwe,batch", [(256, 1, 64, 8, 5), (256, 1, 20, 8, 5),
                                               (1024, 1, 64, 4, 3), (1024, 1, 20, 4, 3),
                                               (256, 2, 20, 3, 4)])          # k = 2: the composed step
def test_blind_rotation_word_exact(pkg, oracle, n, k, l, n_lwe, batch):
    import torch

    L, B = pkg.load_library(), pkg.binding
    rng = np.random.default_rng(n * 100 + l + k)
    bsk = _rand_dev((n_lwe, k + 1, l, k + 1, n), n + l + k)
    table = rng.integers(0, 1 << 64, (k + 1, n), dtype=np.uint64, endpoint=False)
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    prep = _prepare(L, B, n, k, l, n_lwe, bsk)
    out = torch.empty((batch, k + 1, n), dtype=torch.int64, device="cuda")
    dt, dl = _dev(table), _dev(lwe)                                   # held: a freed temporary's block is reused at once
    B._check(L.fhe_tfhe_blind_rotation_dev(n, k, l, n_lwe, prep.data_ptr(), dt.data_ptr(), dl.data_ptr(), out.data_ptr(), batch, None))
    hb = _u64(bsk)
    ms = R.mod_switch(lwe, n)
    assert {0, n, 2 * n - 1} <= {int(x) for x in ms[0, :n_lwe]}
    assert int(ms[0, n_lwe]) == 0 and int(ms[1, n_lwe]) == 0
    want = R.blind_rotation(lambda j, d: oracle.external_product(n, k, l, hb[j], d), n, k, l, hb, table, lwe)
    assert np.array_equal(_u64(out), want)


@pytest.mark.parametrize("batch", [64, 37])
def test_blind_rotation_full_shape_matches_the_prepared_product_loop(pkg, batch):
    """N = 1024, k = 1, l = 64, n_lwe = 630: the fused CMux steps give the words of a host loop over
    fhe_tggsw_external_product_prepared_dev and numpy rotations"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, k, l, n_lwe = 1024, 1, 64, 630
    rng = np.random.default_rng(batch)
    bsk = _rand_dev((n_lwe, k + 1, l, k + 1, n), 7)
    prep = _prepare(L, B, n, k, l, n_lwe, bsk)
    del bsk
    table = rng.integers(0, 1 << 64, (k + 1, n), dtype=np.uint64, endpoint=False)
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    out = torch.empty((batch, k + 1, n), dtype=torch.int64, device="cuda")
    dt, dl = _dev(table), _dev(lwe)                                   # held: a freed temporary's block is reused at once
    B._check(L.fhe_tfhe_blind_rotation_dev(n, k, l, n_lwe, prep.data_ptr(), dt.data_ptr(), dl.data_ptr(), out.data_ptr(), batch, None))
    words = L.fhe_tggsw_prepared_words(n, k, l)
    res = torch.empty((batch, k + 1, n), dtype=torch.int64, device="cuda")

    def ext(j, d):
        dd = _dev(d)
        B._check(L.fhe_tggsw_external_product_prepared_dev(n, k, l, prep.data_ptr() + j * words * 8, dd.data_ptr(), res.data_ptr(),
                                                           batch, None))
        return _u64(res)

    want = R.blind_rotation(ext, n, k, l, None, table, lwe)
    assert np.array_equal(_u64(out), want)


@pytest.mark.parametrize("n,k", [(1024, 1), (256, 2)])
def test_sample_extraction_word_exact(pkg, n, k):
    import torch

    L, B = pkg.load_library(), pkg.binding
    rng = np.random.default_rng(n + k)
    batch = 7
    x = rng.integers(0, 1 << 64, (batch, k + 1, n), dtype=np.uint64, endpoint=False)
    dx = _dev(x)
    for h in (0, 1, n - 1):
        out = torch.empty((batch, k * n + 1), dtype=torch.int64, device="cuda")
        B._check(L.fhe_tglwe_sample_extraction_dev(n, k, h, dx.data_ptr(), out.data_ptr(), batch, None))
        assert np.array_equal(_u64(out), R.sample_extraction(x, h))


@pytest.mark.parametrize("n_in,n_out,l,batch", [(1024, 630, 64, 37), (512, 100, 20, 5), (512, 100, 20, 70)])
def test_key_switch_word_exact(pkg, n_in, n_out, l, batch):
    import torch

    L, B = pkg.load_library(), pkg.binding
    rng = np.random.default_rng(n_in + n_out + l + batch)
    ksk = rng.integers(0, 1 << 64, (n_in, l, n_out + 1), dtype=np.uint64, endpoint=False)
    x = rng.integers(0, 1 << 64, (batch, n_in + 1), dtype=np.uint64, endpoint=False)
    x[0, :4] = [0, (1 << 64) - 1, 1 << 63, 1]
    out = torch.empty((batch, n_out + 1), dtype=torch.int64, device="cuda")
    dk, dx = _dev(ksk), _dev(x)
    B._check(L.fhe_tlwe_key_switch_dev(n_in, n_out, 2, l, dk.data_ptr(), dx.data_ptr(), out.data_ptr(), batch, None))
    assert np.array_equal(_u64(out), R.key_switch(ksk, x, l))


def test_functional_bootstrap_with_real_keys(pkg):
    """binary keys, sigma = 3.2 errors; N = 1024, k = 1, l = 64, n_lwe = 630, KSK 1024 -> 630 with l = 64; t = 16 with a
    bit of padding: every m in [0, 8) bootstraps to f(m) under the input LWE key, and bootstrapping again gives f(f(m))"""
    import torch

    from fhe_study_amd import tfhe

    L, B = pkg.load_library(), pkg.binding
    n, k, l, n_lwe, t, sigma = 1024, 1, 64, 630, 16, 3.2
    rng = np.random.default_rng(42)
    s_glwe = rng.integers(0, 2, n, dtype=np.uint64)
    s_lwe = rng.integers(0, 2, n_lwe, dtype=np.uint64)
    mul = lambda a, b: B.tn_mul(n, a, np.ascontiguousarray(b))
    bsk = torch.empty((n_lwe, k + 1, l, k + 1, n), dtype=torch.int64, device="cuda")
    for j0 in range(0, n_lwe, 70):
        j1 = min(n_lwe, j0 + 70)
        bsk[j0:j1] = _dev(R.tggsw_bits(rng, mul, n, l, s_glwe, s_lwe[j0:j1], sigma))
    ksk = R.ksk(rng, s_glwe, s_lwe, 64, sigma)
    key = tfhe.BootstrappingKey(n, k, l, n_lwe, bsk, ksk, ks_l=64)
    del bsk
    delta = ((1 << 64) - 1) // t
    msgs = np.repeat(np.arange(8), 4)
    lwe = R.lwe_encrypt(rng, s_lwe, [int(m) * delta for m in msgs], sigma)
    assert list(R.lwe_decode(lwe, s_lwe, t)) == list(msgs)
    for f in (lambda m: m, lambda m: (m * m + 3) % 8):
        table = R.test_vector(n, t, f)
        out = tfhe.bootstrapping(key, tfhe.TGLWE(table[:1], table[1]), tfhe.TLWE(lwe))
        assert list(R.lwe_decode(out.words, s_lwe, t)) == [f(int(m)) for m in msgs]
        again = tfhe.bootstrapping(key, tfhe.TGLWE(table[:1], table[1]), out)
        assert list(R.lwe_decode(again.words, s_lwe, t)) == [f(f(int(m))) for m in msgs]
    # the pieces through the public classes: blind rotation, sample extraction, key switch compose to the same words
    table = R.test_vector(n, t, lambda m: m)
    acc = tfhe.blind_rotation(tfhe.TLWE(lwe), key, tfhe.TGLWE(table[:1], table[1]))
    ext = acc.sample_extraction(0)
    ks = ext.key_switch(key.ksk, key.ks_l)
    full = tfhe.bootstrapping(key, tfhe.TGLWE(table[:1], table[1]), tfhe.TLWE(lwe))
    assert np.array_equal(ks.words, full.words)
    assert np.array_equal(acc.left_rotate(5).packed(), np.stack([R.left_rotate(acc.packed()[b], 5) for b in range(len(msgs))]))
