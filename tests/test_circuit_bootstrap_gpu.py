"""Circuit bootstrapping on the device: the private functional key switch, the CMux with a selector per
ciphertext (SRC32_GSEL) and the circuit bootstrap, word-exact against the numpy restatement (tests/_cb_numpy.py) or a
host loop over the existing entry points; and a functional 3-bit lookup table with real keys through circuit bootstrap,
a CMux tree, sample extraction, key switch and one more bootstrap."""
import numpy as np
import pytest

import _cb_numpy as CB
import _gadget_numpy as G
import _tfhe_numpy as R
from test_bootstrap_gpu import _dev, _edge_lwe, _rand_dev, _u64
from test_gadget_cpu import _edge_words

pytestmark = pytest.mark.gpu


def _pfks_dev(pkg, n, b, l, key, c):
    import torch

    L, B = pkg.load_library(), pkg.binding
    out = torch.empty((c.shape[0], 2, 2, n), dtype=torch.int64, device="cuda")
    dk = key if isinstance(key, torch.Tensor) else _dev(key)
    dc = _dev(c)
    B._check(L.fhe_tlwe_gadget_private_key_switch_dev(n, 1, b, l, dk.data_ptr(), dc.data_ptr(), out.data_ptr(), c.shape[0], None))
    return _u64(out)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n,b,l,batch", [(1024, 8, 4, 37), (1024, 4, 4, 5), (256, 1, 64, 33), (256, 8, 8, 3), (256, 16, 4, 70),
                                         (512, 32, 2, 3), (256, 3, 7, 1)])
def test_pfks_word_exact(pkg, n, b, l, batch):
    """random key words with a band of 2^64 - 1, random inputs with the gadget's edge words (every digit -2^(b-1) among
    them); batches that are not multiples of the 32-ciphertext tile"""
    L = pkg.load_library()
    assert L.fhe_tfhe_pfksk_words(n, 1, b, l) == 2 * (n + 1) * l * 2 * n
    rng = np.random.default_rng(n + 10 * b + l)
    key = rng.integers(0, 1 << 64, (2, n + 1, l, 2, n), dtype=np.uint64, endpoint=False)
    key[:, :3] = np.uint64((1 << 64) - 1)
    key[1, n] = np.uint64((1 << 64) - 1)
    c = rng.integers(0, 1 << 64, (batch, n + 1), dtype=np.uint64, endpoint=False)
    edges = _edge_words(b, l)
    c[0, : len(edges)] = edges
    c[-1, :] = edges[5]                                                   # every digit -2^(b-1)
    assert np.all(G.decompose(c[-1, :1], b, l) == -(1 << (b - 1)))
    assert np.array_equal(_pfks_dev(pkg, n, b, l, key, c), CB.private_key_switch(key, c, b, l))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("b,l", [(8, 4), (1, 64)])
def test_pfks_worst_case_words(pkg, b, l):
    """every key word 2^64 - 1, every digit -2^(b-1): each output word is 2^(b-1) (n + 1) l mod 2^64"""
    n = 256
    key = np.full((2, n + 1, l, 2, n), (1 << 64) - 1, dtype=np.uint64)
    c = np.full((2, n + 1), _edge_words(b, l)[5], dtype=np.uint64)
    got = _pfks_dev(pkg, n, b, l, key, c)
    assert np.all(got == np.uint64(((1 << (b - 1)) * (n + 1) * l) % (1 << 64)))


def _prepare_many(pkg, n, b, l, rows):
    import torch

    L, B = pkg.load_library(), pkg.binding
    w = L.fhe_tggsw_gadget_prepared_words(n, 1, b, l)
    prep = torch.empty(len(rows) * w, dtype=torch.int64, device="cuda")
    dr = rows if isinstance(rows, torch.Tensor) else _dev(rows)
    B._check(L.fhe_tggsw_gadget_prepare_many_dev(n, 1, b, l, len(rows), dr.data_ptr(), prep.data_ptr(), None))
    return prep, w


def _cmux_dev(pkg, n, b, l, prep, count, idx, c0, c1):
    import torch

    L, B = pkg.load_library(), pkg.binding
    out = torch.empty(c0.shape, dtype=torch.int64, device="cuda")
    di = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.uint32).view(np.int32)).cuda()
    d0, d1 = _dev(c0), _dev(c1)
    B._check(L.fhe_tggsw_gadget_cmux_dev(n, 1, b, l, count, prep.data_ptr(), di.data_ptr(), d0.data_ptr(), d1.data_ptr(), out.data_ptr(),
                                         c0.shape[0], None))
    return _u64(out)


def _ext_dev(pkg, n, b, l, d_prep, x):
    import torch

    L, B = pkg.load_library(), pkg.binding
    out = torch.empty(x.shape, dtype=torch.int64, device="cuda")
    dx = _dev(x)
    B._check(L.fhe_tggsw_gadget_external_product_dev(n, 1, b, l, d_prep, dx.data_ptr(), out.data_ptr(), x.shape[0], None))
    return _u64(out)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n,b,l,batch", [(256, 8, 3, 5), (1024, 6, 2, 7), (1024, 10, 3, 4), (4096, 8, 2, 3)])
def test_cmux_word_exact_against_the_restatement(pkg, n, b, l, batch):
    """three random TGGSWs, shuffled and repeated selectors, one past the end (selects c0)"""
    count = 3
    rng = np.random.default_rng(n + b + l + batch)
    keys = rng.integers(0, 1 << 64, (count, 2, l, 2, n), dtype=np.uint64, endpoint=False)
    c0 = rng.integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    c1 = rng.integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    c1[0, 0, : len(_edge_words(b, l))] = _edge_words(b, l)
    idx = rng.permutation(np.arange(batch) % (count + 1)).astype(np.uint32)
    idx[0] = 2
    prep, _ = _prepare_many(pkg, n, b, l, keys)
    got = _cmux_dev(pkg, n, b, l, prep, count, idx, c0, c1)
    assert np.array_equal(got, CB.cmux(keys, idx, c0, c1, b))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n,b,l,batch", [(1024, 10, 3, 1024), (1024, 10, 3, 1025), (1024, 6, 2, 1100), (2048, 8, 2, 256),
                                         (2048, 8, 2, 257), (256, 8, 3, 37)])
def test_cmux_equals_c0_plus_the_shared_key_product(pkg, n, b, l, batch):
    """constant idx: c0 + fhe_tggsw_gadget_external_product_dev(c1 - c0) word for word; shuffled idx: the same per key.
    The batches straddle ext32_gadget_split's slot threshold (N = 1024, T = 6: two parts up to 1024; N = 2048: up to 256)."""
    count = 4
    rng = np.random.default_rng(batch + n)
    keys = _rand_dev((count, 2, l, 2, n), batch + 3)
    prep, w = _prepare_many(pkg, n, b, l, keys)
    c0 = rng.integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    c1 = rng.integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    d = c1 - c0
    for sel in (2, 0):
        got = _cmux_dev(pkg, n, b, l, prep, count, np.full(batch, sel), c0, c1)
        assert np.array_equal(got, c0 + _ext_dev(pkg, n, b, l, prep.data_ptr() + sel * w * 8, d))
    idx = rng.integers(0, count, batch).astype(np.uint32)
    got = _cmux_dev(pkg, n, b, l, prep, count, idx, c0, c1)
    for s in range(count):
        m = idx == s
        if m.any():
            assert np.array_equal(got[m], c0[m] + _ext_dev(pkg, n, b, l, prep.data_ptr() + s * w * 8, np.ascontiguousarray(d[m])))


def _cb_dev(pkg, n, b, l, n_lwe, prep, cb_b, cb_l, pf_b, pf_l, pfksk, lwe):
    import torch

    L, B = pkg.load_library(), pkg.binding
    out = torch.empty((lwe.shape[0], 2, cb_l, 2, n), dtype=torch.int64, device="cuda")
    dk = pfksk if isinstance(pfksk, torch.Tensor) else _dev(pfksk)
    dl = _dev(lwe)
    B._check(L.fhe_tfhe_circuit_bootstrap_dev(n, 1, b, l, n_lwe, prep.data_ptr(), cb_b, cb_l, pf_b, pf_l, dk.data_ptr(), dl.data_ptr(),
                                              out.data_ptr(), lwe.shape[0], None))
    return _u64(out)


def _prepare_bsk(pkg, n, b, l, n_lwe, bsk):
    import torch

    L, B = pkg.load_library(), pkg.binding
    prep = torch.empty(L.fhe_tfhe_gadget_bsk_prepared_words(n, 1, b, l, n_lwe), dtype=torch.int64, device="cuda")
    B._check(L.fhe_tfhe_gadget_bsk_prepare_dev(n, 1, b, l, n_lwe, bsk.data_ptr(), prep.data_ptr(), None))
    return prep


@pytest.mark.timeout(600)
@pytest.mark.parametrize("b,l,cb_b,cb_l,pf_b,pf_l,batch", [(10, 3, 6, 2, 8, 4, 5), (8, 3, 4, 3, 4, 8, 3)])
def test_circuit_bootstrap_word_exact_at_256(pkg, b, l, cb_b, cb_l, pf_b, pf_l, batch):
    n, n_lwe = 256, 8
    rng = np.random.default_rng(b + cb_b + pf_b)
    bsk = _rand_dev((n_lwe, 2, l, 2, n), 21 + b)
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, bsk)
    pfksk = rng.integers(0, 1 << 64, (2, n + 1, pf_l, 2, n), dtype=np.uint64, endpoint=False)
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    got = _cb_dev(pkg, n, b, l, n_lwe, prep, cb_b, cb_l, pf_b, pf_l, pfksk, lwe)
    assert np.array_equal(got, CB.circuit_bootstrap(n, b, l, _u64(bsk), cb_b, cb_l, pf_b, pf_l, pfksk, lwe))


@pytest.mark.timeout(900)
def test_circuit_bootstrap_full_shape_matches_the_entry_point_loop(pkg):
    """N = 1024, n_lwe = 630, BSK (10, 3), CB (6, 2), PFKS (8, 4): the fused launch (one blind rotation over batch l_cb
    rows) gives the words of a host loop over fhe_tfhe_gadget_blind_rotation_dev, fhe_tglwe_sample_extraction_dev and
    the PFKS, level by level"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, b, l, n_lwe, cb_b, cb_l, pf_b, pf_l, batch = 1024, 10, 3, 630, 6, 2, 8, 4, 3
    rng = np.random.default_rng(77)
    bsk = _rand_dev((n_lwe, 2, l, 2, n), 5)
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, bsk)
    del bsk
    pfksk = _rand_dev((2, n + 1, pf_l, 2, n), 6)
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    got = _cb_dev(pkg, n, b, l, n_lwe, prep, cb_b, cb_l, pf_b, pf_l, pfksk, lwe)
    shifted = lwe.copy()
    shifted[:, -1] += np.uint64(1 << 62)
    acc = torch.empty((batch, 2, n), dtype=torch.int64, device="cuda")
    ext = torch.empty((batch, n + 1), dtype=torch.int64, device="cuda")
    dl = _dev(shifted)
    for d in range(cb_l):
        table = np.zeros((2, n), dtype=np.uint64)
        table[1] = np.uint64(CB.alpha(cb_b, d))
        dt = _dev(table)
        B._check(L.fhe_tfhe_gadget_blind_rotation_dev(n, 1, b, l, n_lwe, prep.data_ptr(), dt.data_ptr(), dl.data_ptr(), acc.data_ptr(), batch,
                                                      None))
        B._check(L.fhe_tglwe_sample_extraction_dev(n, 1, 0, acc.data_ptr(), ext.data_ptr(), batch, None))
        t = np.uint64(0) - _u64(ext)
        t[:, -1] += np.uint64(CB.alpha(cb_b, d))
        assert np.array_equal(got[:, :, d], _pfks_dev(pkg, n, pf_b, pf_l, pfksk, t))


@pytest.mark.timeout(1200)
def test_functional_lookup_table_through_circuit_bootstrap_and_a_cmux_tree(pkg):
    """binary keys, sigma = 3.2; N = 1024, n_lwe = 630, BSK (10, 3), CB (6, 2), PFKS (8, 4), KSK 1024 -> 630 with (4, 4);
    t = 16 with padding.  The three bits of x in [0, 8) are LWE encryptions of bit 2^63; circuit bootstrap -> cmux_tree over
    a table of 8 trivial TGLWEs -> sample extraction -> key switch decrypts to table[x], and bootstraps once more"""
    from fhe_study_amd import tfhe

    B = pkg.binding
    n, k, b, l, n_lwe, cb_b, cb_l, pf_b, pf_l, ks_b, ks_l, t, sigma = 1024, 1, 10, 3, 630, 6, 2, 8, 4, 4, 4, 16, 3.2
    rng = np.random.default_rng(2026)
    s_glwe = rng.integers(0, 2, n, dtype=np.uint64)
    s_lwe = rng.integers(0, 2, n_lwe, dtype=np.uint64)
    mul = lambda a, x: B.tn_mul(n, a, np.ascontiguousarray(x))
    bsk = G.tggsw_bits(rng, mul, n, b, l, s_glwe, s_lwe, sigma)
    ksk = G.ksk(rng, s_glwe, s_lwe, ks_b, ks_l, sigma)
    btk = tfhe.BootstrappingKey(n, k, l, n_lwe, bsk, ksk, ks_l=ks_l, log_beta=b, ks_log_beta=ks_b)
    del bsk
    cbk = tfhe.CircuitBootstrappingKey(btk, CB.pfksk(rng, mul, n, s_glwe, pf_b, pf_l, sigma), cb_b, cb_l, pf_b, pf_l)
    f = lambda x: (3 * x + 5) % 8
    delta = ((1 << 64) - 1) // t
    table = np.zeros((8, 2, n), dtype=np.uint64)
    table[:, 1, 0] = [f(x) * delta for x in range(8)]
    reps = 3
    xs = np.repeat(np.arange(8), reps)
    bits = np.array([[(x >> i) & 1 for i in range(3)] for x in xs])          # [24][3], bit 0 the least significant
    lwe = R.lwe_encrypt(rng, s_lwe, [int(v) << 63 for v in bits.reshape(-1)], sigma)
    tg = tfhe.circuit_bootstrap(cbk, tfhe.TLWE(lwe), device=True)             # [72][2][cb_l][2][n]
    sel = tfhe.PreparedTGGSWs(tg, cb_b)
    out = tfhe.cmux_tree(sel, np.arange(len(xs) * 3).reshape(len(xs), 3), table)
    ext = out.sample_extraction(0)
    # the GLWE phase before the key switch, and after it under the LWE key
    e_glwe = CB.centred(CB.tlwe_phase(ext.words, s_glwe) - np.array([f(int(x)) * delta for x in xs], dtype=np.uint64)).astype(object)
    res = ext.key_switch(btk.ksk, ks_l, log_beta=ks_b)
    e_lwe = CB.centred(CB.tlwe_phase(res.words, s_lwe) - np.array([f(int(x)) * delta for x in xs], dtype=np.uint64)).astype(object)
    print(f"\ncmux tree of depth 3: worst |error| log2 {np.log2(float(max(abs(e) for e in e_glwe))):.1f} under s, "
          f"{np.log2(float(max(abs(e) for e in e_lwe))):.1f} after the (4, 4) key switch; margin log2 {np.log2(delta / 2):.1f}")
    assert list(R.lwe_decode(res.words, s_lwe, t)) == [f(int(x)) for x in xs]
    g = lambda m: (m * m + 1) % 8
    tv = R.test_vector(n, t, g)
    again = tfhe.bootstrapping(btk, tfhe.TGLWE(tv[:1], tv[1]), res)
    assert list(R.lwe_decode(again.words, s_lwe, t)) == [g(f(int(x))) for x in xs]
    # the Python surface composes to the same words as the entry points
    one = tfhe.cmux(sel, np.arange(3) * 3, tfhe.TGLWE(table[:3, :1], table[:3, 1]), tfhe.TGLWE(table[3:6, :1], table[3:6, 1]))
    want = CB.cmux(np.stack([tg[i].cpu().numpy().view(np.uint64) for i in (0, 3, 6)]), [0, 1, 2], table[:3], table[3:6], cb_b)
    assert np.array_equal(one.packed(), want)
