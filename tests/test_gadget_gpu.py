"""The signed base-2^b gadget on the device (tfhe_boot.hip, the gadget modes of digit32.hip): word-exact against the
numpy restatement of DESIGN.md §11 (tests/_gadget_numpy.py), at and inside the admission edges, and a functional
bootstrap with real keys."""
import numpy as np
import pytest

import _gadget_numpy as G
import _tfhe_numpy as R
from test_bootstrap_gpu import _dev, _edge_lwe, _rand_dev, _u64
from test_gadget_cpu import _edge_words, admitted

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("b,l", [(8, 3), (10, 2), (4, 4), (1, 64), (16, 4), (32, 2), (64, 1), (7, 9)])
def test_device_decomposition_matches_the_restatement(pkg, b, l):
    from fhe_study_amd import tfhe

    n, rows = 256, 3
    rng = np.random.default_rng(b + 100 * l)
    w = rng.integers(0, 1 << 64, (rows, n), dtype=np.uint64, endpoint=False)
    edges = _edge_words(b, l)
    w[0, : len(edges)] = edges
    got = tfhe.gadget_decompose(w, b, l)                                  # [rows][l][n]
    assert got.shape == (rows, l, n) and got.dtype == np.int64
    assert np.array_equal(got, np.moveaxis(G.decompose(w, b, l), -1, -2))


def _product(pkg, n, b, l, key, ct):
    import torch

    L, B = pkg.load_library(), pkg.binding
    words = L.fhe_tggsw_gadget_prepared_words(n, 1, b, l)
    assert words == 2 * 2 * l * 2 * n
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    dk, dc = _dev(key), _dev(ct)
    B._check(L.fhe_tggsw_gadget_prepare_dev(n, 1, b, l, dk.data_ptr(), prep.data_ptr(), None))
    out = torch.empty(ct.shape, dtype=torch.int64, device="cuda")
    B._check(L.fhe_tggsw_gadget_external_product_dev(n, 1, b, l, prep.data_ptr(), dc.data_ptr(), out.data_ptr(), ct.shape[0], None))
    return _u64(out)


@pytest.mark.parametrize("n,b,l,batch", [(256, 8, 3, 5), (256, 12, 2, 3), (1024, 10, 2, 3), (1024, 10, 3, 3), (1024, 8, 3, 4),
                                         (1024, 4, 4, 2), (1024, 1, 1, 2), (4096, 8, 2, 2), (4096, 5, 3, 1)])
def test_gadget_external_product_word_exact(pkg, n, b, l, batch):
    assert admitted(n, 1, b, l)
    rng = np.random.default_rng(n + b * 10 + l)
    key = rng.integers(0, 1 << 64, (2, l, 2, n), dtype=np.uint64, endpoint=False)
    ct = rng.integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    ct[0, 0, : len(_edge_words(b, l))] = _edge_words(b, l)
    assert np.array_equal(_product(pkg, n, b, l, key, ct), G.external_product(key, ct, b))


@pytest.mark.parametrize("n,b,l", [(1024, 10, 2), (1024, 10, 3), (4096, 8, 2)])
def test_gadget_external_product_worst_case_at_the_edge(pkg, n, b, l):
    """every key word 2^64 - 1 (both halves 2^32 - 1), every digit -2^(b-1): coefficient N-1 of each half-sum reaches
    (k+1) l N (2^32 - 1) 2^(b-1), the admission rule's bound"""
    from fhe_study_amd import tfhe

    key = np.full((2, l, 2, n), (1 << 64) - 1, dtype=np.uint64)
    ct = np.full((2, 2, n), _edge_words(b, l)[5], dtype=np.uint64)
    assert np.all(G.decompose(ct[0, 0, :1], b, l) == -(1 << (b - 1)))
    want = G.external_product(key, ct, b)
    # coefficient N-1 has no wrapped terms: 2 l N products (-1) (-2^(b-1)) = 2^(b-1) each
    assert np.all(want[:, :, n - 1] == np.uint64(2 * l * n * (1 << (b - 1))))
    assert np.array_equal(_product(pkg, n, b, l, key, ct), want)
    got = tfhe.gadget_external_product(tfhe.TGGSW(key), tfhe.TGLWE(ct[:, :1], ct[:, 1]), b)
    assert np.array_equal(got.packed(), want)


def _prepare_bsk(pkg, n, b, l, n_lwe, bsk):
    import torch

    L, B = pkg.load_library(), pkg.binding
    words = L.fhe_tfhe_gadget_bsk_prepared_words(n, 1, b, l, n_lwe)
    assert words == n_lwe * L.fhe_tggsw_gadget_prepared_words(n, 1, b, l) > 0
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    B._check(L.fhe_tfhe_gadget_bsk_prepare_dev(n, 1, b, l, n_lwe, bsk.data_ptr(), prep.data_ptr(), None))
    return prep


@pytest.mark.parametrize("n,b,l,n_lwe,batch", [(256, 8, 3, 8, 5), (256, 12, 2, 6, 3), (1024, 10, 2, 4, 3), (1024, 8, 3, 3, 2)])
def test_gadget_blind_rotation_word_exact(pkg, n, b, l, n_lwe, batch):
    import torch

    L, B = pkg.load_library(), pkg.binding
    rng = np.random.default_rng(n + b + l)
    bsk = _rand_dev((n_lwe, 2, l, 2, n), n + 7 * b + l)
    table = rng.integers(0, 1 << 64, (2, n), dtype=np.uint64, endpoint=False)
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, bsk)
    out = torch.empty((batch, 2, n), dtype=torch.int64, device="cuda")
    dt, dl = _dev(table), _dev(lwe)
    B._check(L.fhe_tfhe_gadget_blind_rotation_dev(n, 1, b, l, n_lwe, prep.data_ptr(), dt.data_ptr(), dl.data_ptr(), out.data_ptr(),
                                                  batch, None))
    ms = R.mod_switch(lwe, n)
    assert {0, n, 2 * n - 1} <= {int(x) for x in ms[0, :n_lwe]}
    assert np.array_equal(_u64(out), G.blind_rotation(n, 1, b, l, _u64(bsk), table, lwe))


@pytest.mark.parametrize("batch", [64, 37])
def test_gadget_blind_rotation_full_shape_matches_the_product_loop(pkg, batch):
    """N = 1024, k = 1, (b, l) = (8, 3), n_lwe = 630: the fused gadget CMux steps give the words of a host loop over
    fhe_tggsw_gadget_external_product_dev and numpy rotations"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, b, l, n_lwe = 1024, 8, 3, 630
    rng = np.random.default_rng(batch)
    bsk = _rand_dev((n_lwe, 2, l, 2, n), 11)
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, bsk)
    del bsk
    table = rng.integers(0, 1 << 64, (2, n), dtype=np.uint64, endpoint=False)
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    out = torch.empty((batch, 2, n), dtype=torch.int64, device="cuda")
    dt, dl = _dev(table), _dev(lwe)
    B._check(L.fhe_tfhe_gadget_blind_rotation_dev(n, 1, b, l, n_lwe, prep.data_ptr(), dt.data_ptr(), dl.data_ptr(), out.data_ptr(),
                                                  batch, None))
    words = L.fhe_tggsw_gadget_prepared_words(n, 1, b, l)
    res = torch.empty((batch, 2, n), dtype=torch.int64, device="cuda")

    def ext(j, d):
        dd = _dev(d)
        B._check(L.fhe_tggsw_gadget_external_product_dev(n, 1, b, l, prep.data_ptr() + j * words * 8, dd.data_ptr(), res.data_ptr(),
                                                         batch, None))
        return _u64(res)

    want = R.blind_rotation(ext, n, 1, l, None, table, lwe)
    assert np.array_equal(_u64(out), want)


@pytest.mark.parametrize("n_in,n_out,b,l,batch", [(1024, 630, 4, 4, 37), (512, 100, 2, 10, 5), (512, 100, 2, 10, 70),
                                                  (512, 100, 16, 4, 33), (256, 50, 32, 2, 3), (256, 50, 1, 64, 3)])
def test_gadget_key_switch_word_exact(pkg, n_in, n_out, b, l, batch):
    import torch

    L, B = pkg.load_library(), pkg.binding
    rng = np.random.default_rng(n_in + n_out + b + l + batch)
    ksk = rng.integers(0, 1 << 64, (n_in, l, n_out + 1), dtype=np.uint64, endpoint=False)
    x = rng.integers(0, 1 << 64, (batch, n_in + 1), dtype=np.uint64, endpoint=False)
    edges = _edge_words(b, l)
    x[0, : len(edges)] = edges
    out = torch.empty((batch, n_out + 1), dtype=torch.int64, device="cuda")
    dk, dx = _dev(ksk), _dev(x)
    B._check(L.fhe_tlwe_gadget_key_switch_dev(n_in, n_out, b, l, dk.data_ptr(), dx.data_ptr(), out.data_ptr(), batch, None))
    assert np.array_equal(_u64(out), G.key_switch(ksk, x, b, l))


def test_functional_gadget_bootstrap_with_real_keys(pkg):
    """binary keys, sigma = 3.2; N = 1024, k = 1, n_lwe = 630, BSK (b, l) = (8, 3), KSK 1024 -> 630 with (4, 4); t = 16
    with a bit of padding: every m in [0, 8) bootstraps to f(m), and bootstrapping again gives f(f(m))"""
    from fhe_study_amd import tfhe

    B = pkg.binding
    n, k, b, l, n_lwe, ks_b, ks_l, t, sigma = 1024, 1, 8, 3, 630, 4, 4, 16, 3.2
    rng = np.random.default_rng(43)
    s_glwe = rng.integers(0, 2, n, dtype=np.uint64)
    s_lwe = rng.integers(0, 2, n_lwe, dtype=np.uint64)
    mul = lambda a, x: B.tn_mul(n, a, np.ascontiguousarray(x))
    bsk = G.tggsw_bits(rng, mul, n, b, l, s_glwe, s_lwe, sigma)
    ksk = G.ksk(rng, s_glwe, s_lwe, ks_b, ks_l, sigma)
    key = tfhe.BootstrappingKey(n, k, l, n_lwe, bsk, ksk, ks_l=ks_l, log_beta=b, ks_log_beta=ks_b)
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
    # the public pieces compose to the words of the full call
    table = R.test_vector(n, t, lambda m: m)
    acc = tfhe.blind_rotation(tfhe.TLWE(lwe), key, tfhe.TGLWE(table[:1], table[1]))
    ks = acc.sample_extraction(0).key_switch(key.ksk, key.ks_l, log_beta=key.ks_log_beta)
    full = tfhe.bootstrapping(key, tfhe.TGLWE(table[:1], table[1]), tfhe.TLWE(lwe))
    assert np.array_equal(ks.words, full.words)
    with pytest.raises(ValueError):
        tfhe.BootstrappingKey(n, k, l, n_lwe, bsk[:1], ksk, ks_l=ks_l, log_beta=b)
