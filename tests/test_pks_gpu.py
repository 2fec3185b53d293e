"""The packing key switch, the box expansion, the bootstrap with a test vector per row and two-digit tree lookups on the
device: fhe_tlwe_gadget_packing_key_switch_dev and fhe_tglwe_box_expand_dev word for word against the numpy
twin (tests/_pks_numpy.py), fhe_tfhe_gadget_bootstrap_rows_dev against the existing single-table calls, the rejections,
and tree_lookup with real keys."""
import numpy as np
import pytest

import _cb_numpy as CB
import _gadget_numpy as G
import _gates_numpy as GN
import _lut_numpy as LN
import _pks_numpy as PK
import _tfhe_numpy as R
from test_bootstrap_gpu import _dev, _edge_lwe, _rand_dev, _u64

pytestmark = pytest.mark.gpu

TG = 16                                                                         # tlwe_packing_ks_kernel's group tile (PK_TG)


def _pks_dev(pkg, n, n_in, b, l, key, flat, gstride, istride, count, log_stride, groups):
    import torch

    L, B = pkg.load_library(), pkg.binding
    out = torch.empty((groups, 2, n), dtype=torch.int64, device="cuda")
    dk, dx = _dev(key), _dev(flat)
    B._check(L.fhe_tlwe_gadget_packing_key_switch_dev(n, 1, n_in, b, l, dk.data_ptr(), dx.data_ptr(), gstride, istride, count, log_stride,
                                                      out.data_ptr(), groups, None))
    return _u64(out)


@pytest.mark.parametrize("n,n_in,b,l,count,log_stride,groups,function_major", [
    (256, 8, 1, 3, 1, 0, 1, False),
    (256, 8, 8, 4, 16, 4, TG, True),                                            # count stride = N: every rotation but the first wraps
    (256, 8, 32, 2, 256, 0, TG + 1, False),                                     # stride 1, count = N; s_p = 0
    (256, 8, 16, 4, 3, 6, 70, True),                                            # a partial pack, stride = the column tile; s_p = 0
    (256, 8, 8, 4, 4, 6, 70, False),
    (256, 8, 1, 3, 2, 7, TG + 1, True),                                         # stride > the column tile
    (1024, 630, 8, 4, 8, 7, 37, True)])                                         # the production key shape, partial tiles
def test_packing_key_switch_word_exact(pkg, n, n_in, b, l, count, log_stride, groups, function_major):
    """random key words; inputs from _edge_lwe (fields of all ones and of zero occur); a contiguous [groups][count][n_in + 1]
    block, or §15's function-major [count][groups][n_in + 1] read through the strides"""
    rng = np.random.default_rng(n + n_in + 10 * b + count + groups)
    key = rng.integers(0, 1 << 64, (n_in, l, 2, n), dtype=np.uint64, endpoint=False)
    rows = _edge_lwe(rng, max(groups * count, 2), n_in, n)[: groups * count].reshape(groups, count, n_in + 1)   # _edge_lwe pins two rows
    row = n_in + 1
    if function_major:
        flat, gs, is_ = np.ascontiguousarray(rows.transpose(1, 0, 2)), row, groups * row
    else:
        flat, gs, is_ = rows, count * row, row
    got = _pks_dev(pkg, n, n_in, b, l, key, flat, gs, is_, count, log_stride, groups)
    want = PK.packing_key_switch(key, rows, b, l, count, log_stride)
    assert want.any() and np.array_equal(got, want)


def test_packing_key_switch_with_padded_strides(pkg):
    """strides larger than the rows need: ciphertexts 3 words apart from dense, groups a further 5"""
    n, n_in, b, l, count, log_stride, groups = 256, 8, 8, 4, 4, 6, 5
    rng = np.random.default_rng(99)
    key = rng.integers(0, 1 << 64, (n_in, l, 2, n), dtype=np.uint64, endpoint=False)
    is_, gs = n_in + 1 + 3, count * (n_in + 1 + 3) + 5
    flat = rng.integers(0, 1 << 64, groups * gs, dtype=np.uint64, endpoint=False)
    rows = np.stack([np.stack([flat[g * gs + i * is_: g * gs + i * is_ + n_in + 1] for i in range(count)]) for g in range(groups)])
    got = _pks_dev(pkg, n, n_in, b, l, key, flat, gs, is_, count, log_stride, groups)
    assert np.array_equal(got, PK.packing_key_switch(key, rows, b, l, count, log_stride))


@pytest.mark.parametrize("n,t,batch", [(256, 1, 1), (256, 4, 70), (256, 7, 1), (256, 8, 70), (256, 1, 70), (4096, 4, 3)])
def test_box_expansion_word_exact(pkg, n, t, batch):
    import torch

    L, B = pkg.load_library(), pkg.binding
    x = np.random.default_rng(n + t + batch).integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    dx = _dev(x)
    out = torch.empty((batch, 2, n), dtype=torch.int64, device="cuda")
    B._check(L.fhe_tglwe_box_expand_dev(n, 1, t, dx.data_ptr(), out.data_ptr(), batch, None))
    assert np.array_equal(_u64(out), PK.box_expand(x, t))
    assert np.array_equal(_u64(dx), x)


# ---- the bootstrap with a test vector per row ---------------------------------------------------------------------------------
def _prepare_bsk(pkg, n, b, l, n_lwe, bsk):
    import torch

    L, B = pkg.load_library(), pkg.binding
    prep = torch.empty(L.fhe_tfhe_gadget_bsk_prepared_words(n, 1, b, l, n_lwe), dtype=torch.int64, device="cuda")
    B._check(L.fhe_tfhe_gadget_bsk_prepare_dev(n, 1, b, l, n_lwe, bsk.data_ptr(), prep.data_ptr(), None))
    return prep


def _rows_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, tables, lwe):
    import torch

    L, B = pkg.load_library(), pkg.binding
    out = torch.empty((lwe.shape[0], n_lwe + 1), dtype=torch.int64, device="cuda")
    dt, dl = _dev(tables), _dev(lwe)
    B._check(L.fhe_tfhe_gadget_bootstrap_rows_dev(n, 1, b, l, n_lwe, prep.data_ptr(), dt.data_ptr(), ks_b, ks_l, ksk.data_ptr(), dl.data_ptr(),
                                                  out.data_ptr(), lwe.shape[0], None))
    return _u64(out)


def _bootstrap_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, table, lwe):
    import torch

    L, B = pkg.load_library(), pkg.binding
    out = torch.empty((lwe.shape[0], n_lwe + 1), dtype=torch.int64, device="cuda")
    dt, dl = _dev(table), _dev(lwe)
    B._check(L.fhe_tfhe_gadget_bootstrap_dev(n, 1, b, l, n_lwe, prep.data_ptr(), dt.data_ptr(), ks_b, ks_l, ksk.data_ptr(), dl.data_ptr(),
                                             out.data_ptr(), lwe.shape[0], None))
    return _u64(out)


def test_bootstrap_rows_with_one_trivial_table_is_the_gadget_bootstrap(pkg):
    n, n_lwe, b, l, ks_b, ks_l, batch = 256, 8, 8, 3, 4, 4, 70
    rng = np.random.default_rng(161)
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, _rand_dev((n_lwe, 2, l, 2, n), 161))
    ksk = _rand_dev((n, ks_l, n_lwe + 1), 162)
    table = LN.expand(rng.integers(0, 1 << 64, 16, dtype=np.uint64, endpoint=False), n)
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    got = _rows_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, np.broadcast_to(table, (batch, 2, n)), lwe)
    want = _bootstrap_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, table, lwe)
    assert want.any() and np.array_equal(got, want)


def test_bootstrap_rows_with_a_random_tglwe_per_row_is_each_row_bootstrapped_alone(pkg):
    """fhe_tfhe_gadget_blind_rotation_dev rotates every component of its table (tfhe_br_init_kernel reads row r >> L of it),
    so a full random TGLWE, mask included, is a valid single-table reference: blind rotation, extraction at 0, key switch"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, n_lwe, b, l, ks_b, ks_l, batch = 256, 8, 8, 3, 4, 4, 5
    rng = np.random.default_rng(163)
    hbsk = rng.integers(0, 1 << 64, (n_lwe, 2, l, 2, n), dtype=np.uint64, endpoint=False)
    hksk = rng.integers(0, 1 << 64, (n, ks_l, n_lwe + 1), dtype=np.uint64, endpoint=False)
    prep, ksk = _prepare_bsk(pkg, n, b, l, n_lwe, _dev(hbsk)), _dev(hksk)
    tables = rng.integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    got = _rows_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, tables, lwe)
    for r in range(batch):
        dt, dl = _dev(tables[r]), _dev(lwe[r:r + 1])
        acc = torch.empty((1, 2, n), dtype=torch.int64, device="cuda")
        ext = torch.empty((1, n + 1), dtype=torch.int64, device="cuda")
        out = torch.empty((1, n_lwe + 1), dtype=torch.int64, device="cuda")
        B._check(L.fhe_tfhe_gadget_blind_rotation_dev(n, 1, b, l, n_lwe, prep.data_ptr(), dt.data_ptr(), dl.data_ptr(), acc.data_ptr(), 1, None))
        B._check(L.fhe_tglwe_sample_extraction_dev(n, 1, 0, acc.data_ptr(), ext.data_ptr(), 1, None))
        B._check(L.fhe_tlwe_gadget_key_switch_dev(n, n_lwe, ks_b, ks_l, ksk.data_ptr(), ext.data_ptr(), out.data_ptr(), 1, None))
        assert np.array_equal(got[r], _u64(out)[0]), r
    # and the numpy twin, independent of the device path, on the first two rows (the mod-switch edges)
    assert np.array_equal(got[:2], PK.bootstrap_rows(n, b, l, hbsk, tables[:2], ks_b, ks_l, hksk, lwe[:2]))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("batch", [1024, 1025])
def test_bootstrap_rows_across_the_gadget_split_threshold(pkg, batch):
    """N = 1024, BSK (8, 3): ext32_gadget_split runs two parts up to batch 1024 and one above.  Two distinct random TGLWEs
    dealt over the rows; each subset equals fhe_tfhe_gadget_bootstrap_dev on those rows with that table."""
    n, n_lwe, b, l, ks_b, ks_l = 1024, 16, 8, 3, 4, 4
    rng = np.random.default_rng(164 + batch)
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, _rand_dev((n_lwe, 2, l, 2, n), 164))
    ksk = _rand_dev((n, ks_l, n_lwe + 1), 165)
    two = rng.integers(0, 1 << 64, (2, 2, n), dtype=np.uint64, endpoint=False)
    pick = rng.integers(0, 2, batch)
    pick[:2], pick[-1] = (0, 1), 1
    lwe = _edge_lwe(rng, batch, n_lwe, n)
    got = _rows_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, two[pick], lwe)
    for i in range(2):
        want = _bootstrap_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, two[i], lwe[pick == i])
        assert want.any() and np.array_equal(got[pick == i], want), i


def test_rejections_return_invalid_and_launch_nothing(pkg):
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, n_in, b, l, count, ls, groups = 256, 8, 8, 4, 4, 6, 3
    key = torch.zeros((n_in, l, 2, n), dtype=torch.int64, device="cuda")
    src = torch.zeros((groups + 1, count, n_in + 1), dtype=torch.int64, device="cuda")
    out = torch.full((groups + 1, 2, n), 0x5A5A, dtype=torch.int64, device="cuda")
    row = n_in + 1

    def pks(n=n, k=1, n_in=n_in, b=b, l=l, d_key=key.data_ptr(), d_in=src.data_ptr(), gs=count * row, is_=row, count=count, ls=ls,
            d_out=out.data_ptr(), groups=groups):
        return L.fhe_tlwe_gadget_packing_key_switch_dev(n, k, n_in, b, l, d_key, d_in, gs, is_, count, ls, d_out, groups, None)

    n_lwe, bb, bl, ks_b, ks_l, batch = 8, 8, 3, 4, 4, 3
    prep = torch.zeros(L.fhe_tfhe_gadget_bsk_prepared_words(n, 1, bb, bl, n_lwe), dtype=torch.int64, device="cuda")
    ksk = torch.zeros((n, ks_l, n_lwe + 1), dtype=torch.int64, device="cuda")
    tables = torch.zeros((batch, 2, n), dtype=torch.int64, device="cuda")
    lwe = torch.zeros((batch, n_lwe + 1), dtype=torch.int64, device="cuda")
    bout = torch.full((batch, n_lwe + 1), 0x5A5A, dtype=torch.int64, device="cuda")

    def rows(n=n, k=1, b=bb, l=bl, n_lwe=n_lwe, ks_b=ks_b, ks_l=ks_l, d_tables=tables.data_ptr(), d_out=bout.data_ptr()):
        return L.fhe_tfhe_gadget_bootstrap_rows_dev(n, k, b, l, n_lwe, prep.data_ptr(), d_tables, ks_b, ks_l, ksk.data_ptr(), lwe.data_ptr(), d_out,
                                                    batch, None)

    B.kernel_timing_reset()
    B.kernel_timing_enable(True)                                                # every launch of the library is recorded by name
    try:
        for shape in ((n, 2, n_in, b, l), (128, 1, n_in, b, l), (8192, 1, n_in, b, l), (n, 1, n_in, 33, 1), (n, 1, n_in, 13, 5)):
            assert L.fhe_tfhe_pksk_words(*shape) == 0, shape
        for kw in (dict(groups=0), dict(count=0), dict(count=5), dict(count=1, ls=9), dict(ls=9), dict(gs=n_in), dict(is_=n_in), dict(k=2), dict(n=128),
                   dict(n=8192), dict(b=33, l=1), dict(b=13, l=5), dict(groups=1 << 40), dict(gs=1 << 62),
                   dict(d_out=key.data_ptr() + 64), dict(d_out=src.data_ptr() + 16), dict(d_out=src.data_ptr() + groups * count * row * 8 - 16)):
            assert pks(**kw) == B.FHE_E_INVALID, kw
            assert b"fhe_tlwe_gadget_packing_key_switch_dev" in L.fhe_last_error()
        be = L.fhe_tglwe_box_expand_dev
        for args in ((n, 1, 0), (n, 1, 9), (n, 2, 3), (128, 1, 3), (8192, 1, 3)):
            assert be(*args, tables.data_ptr(), out.data_ptr(), batch, None) == B.FHE_E_INVALID, args
        assert be(n, 1, 3, tables.data_ptr(), tables.data_ptr() + 2 * n * 8, batch, None) == B.FHE_E_INVALID
        for kw in (dict(k=2), dict(n=128), dict(b=33, l=1), dict(n_lwe=0), dict(ks_b=33), dict(ks_l=0), dict(d_out=tables.data_ptr() + 64),
                   dict(d_out=lwe.data_ptr()), dict(d_out=ksk.data_ptr() + 32)):
            assert rows(**kw) == B.FHE_E_INVALID, kw
            assert b"fhe_tfhe_gadget_bootstrap_rows_dev" in L.fhe_last_error()
        torch.cuda.synchronize()
        assert B.kernel_timing_read() == {}                                     # nothing was launched
        assert (_u64(out) == 0x5A5A).all() and (_u64(bout) == 0x5A5A).all()     # and nothing written
        assert pks() == B.FHE_OK and rows() == B.FHE_OK
        assert be(n, 1, 8, tables.data_ptr(), out.data_ptr(), batch, None) == B.FHE_OK          # t = L is admitted
        torch.cuda.synchronize()
        assert {"tlwe_packing_ks_8", "tglwe_box_expand_8", "tfhe_br_rows_init_8"} <= set(B.kernel_timing_read())
    finally:
        B.kernel_timing_enable(False)
        B.kernel_timing_reset()
    assert not _u64(out)[:groups].any() and (_u64(out)[groups:] == 0x5A5A).all()   # zero key and inputs: zero rows, and only `groups` of them
    assert not _u64(bout).any()


# ---- real keys: the parameters and key recipe of test_lut_gpu.py, and a packing key (8, 4) from the LWE key -------------------------
N, NL, BSK, KSK, PKS, SIGMA = 1024, 630, (10, 3), (4, 4), (8, 4), 3.2


@pytest.fixture(scope="module")
def keys(pkg):
    from fhe_study_amd import tfhe

    B = pkg.binding
    rng = np.random.default_rng(1616)
    s_glwe = rng.integers(0, 2, N, dtype=np.uint64)
    s_lwe = rng.integers(0, 2, NL, dtype=np.uint64)
    mul = lambda a, x: B.tn_mul(N, a, np.ascontiguousarray(x))
    bsk = G.tggsw_bits(rng, mul, N, BSK[0], BSK[1], s_glwe, s_lwe, SIGMA)
    ksk = G.ksk(rng, s_glwe, s_lwe, KSK[0], KSK[1], SIGMA)
    btk = tfhe.BootstrappingKey(N, 1, BSK[1], NL, bsk, ksk, ks_l=KSK[1], log_beta=BSK[0], ks_log_beta=KSK[0])
    pk = tfhe.PackingKeySwitchKey(PK.pksk(rng, mul, N, s_lwe, s_glwe, PKS[0], PKS[1], SIGMA), PKS[0], PKS[1])
    return btk, pk, s_lwe, s_glwe, mul, rng


def _encrypt(rng, s, values, t):
    return R.lwe_encrypt(rng, s, [LN.encode(v, t) for v in np.asarray(values).reshape(-1)], SIGMA)


def _log2_worst(e):
    return float(np.log2(float(max(max(abs(int(x)) for x in np.asarray(e, dtype=object).reshape(-1)), 1))))


def _level_errors(tfhe, btk, pk, s_lwe, s_glwe, mul, t, tabs, which, x, y):
    """the steps of tree_lookup one by one through the thin wrappers (nu = 0), for the errors of each level: level-1 outputs
    against table2d[j][y], the packed coefficients q box against the same words, the result against table2d[x][y]"""
    P, batch = 1 << t, x.words.shape[0]
    desc = [(int(which[g]) * P + j, g, tfhe.LUT_NONE, 1, 0, 0) for g in range(batch) for j in range(P)]
    lvl1 = tfhe.lut_bootstrap(btk, t, tabs.reshape(-1, P), desc, y.words)
    want1 = np.array([tabs[which[g], j, y_] for g, y_ in enumerate(y.values) for j in range(P)], dtype=np.uint64)
    e1 = LN.phase_error(lvl1.words, s_lwe, want1)
    packed = tfhe.packing_key_switch(pk, tfhe.TLWE(lvl1.words.reshape(batch, P, NL + 1)), 10 - t)
    ph = CB.tglwe_phase(mul, packed.packed(), s_glwe)
    e2 = CB.centred(ph[:, np.arange(P) << (10 - t)].reshape(-1) - want1).astype(object)
    rest = np.ones(N, dtype=bool)
    rest[np.arange(P) << (10 - t)] = False
    e2_rest = CB.centred(ph[:, rest]).astype(object)
    tv = tfhe.box_expand(packed, t)
    out = tfhe.bootstrap_rows(btk, tv, x)
    return lvl1, e1, e2, e2_rest, out


class _Batch:
    """TLWE words with the values they encrypt, so that the helpers above can name the expected words"""

    def __init__(self, tfhe, rng, s, values, t):
        self.values = np.asarray(values)
        self.words = _encrypt(rng, s, self.values, t)


@pytest.mark.timeout(1200)
def test_tree_lookup_product_and_comparison_over_all_64_pairs(pkg, keys):
    """t = 3, nu = 0, one tree_lookup of batch 128: all 64 pairs (x, y) through (x y) mod 8 and through [x < y] with a gate bit
    +-2^61 as the output.  Every output decrypts to the expected value with |phase error| < Delta / 2 = 2^59 (the decoding
    condition); the products still decode after one more identity lookup."""
    from fhe_study_amd import tfhe

    btk, pk, s_lwe, s_glwe, mul, rng = keys
    t, P = 3, 8
    half_box = 1 << 59
    prod = np.array([[int(LN.encode(x * y % P, t)) for y in range(P)] for x in range(P)], dtype=np.uint64)
    less = np.array([[int(GN.bit_phase(int(x < y))) % (1 << 64) for y in range(P)] for x in range(P)], dtype=np.uint64)
    tabs = np.stack([prod, less])
    xv, yv = np.tile(np.repeat(np.arange(P), P), 2), np.tile(np.tile(np.arange(P), P), 2)
    which = np.repeat([0, 1], P * P)
    x, y = _Batch(tfhe, rng, s_lwe, xv, t), _Batch(tfhe, rng, s_lwe, yv, t)
    out = tfhe.tree_lookup(btk, pk, t, tabs, tfhe.TLWE(x.words), tfhe.TLWE(y.words), which=which)
    assert out.words.shape == (128, NL + 1)
    want = tabs[which, xv, yv]
    e = LN.phase_error(out.words, s_lwe, want)
    assert list(LN.decode(LN.phases(out.words[:64], s_lwe), t)) == [int(a * b % P) for a, b in zip(xv[:64], yv[:64])]
    assert list(GN.decode(out.words[64:], s_lwe)) == [int(a < b) for a, b in zip(xv[64:], yv[64:])]
    # the same steps through the thin wrappers give the same words, and the errors level by level
    lvl1, e1, e2, e2_rest, out_steps = _level_errors(tfhe, btk, pk, s_lwe, s_glwe, mul, t, tabs, which, tfhe.TLWE(x.words), y)
    assert np.array_equal(out_steps.words, out.words)
    # once more through an identity lookup: the products still decode
    ident = tfhe.make_lut(lambda v: v, t)
    again = tfhe.lut_bootstrap(btk, t, [ident], [(0, i, tfhe.LUT_NONE, 1, 0, 0) for i in range(64)], out.words[:64])
    e3 = LN.phase_error(again.words, s_lwe, want[:64])
    assert list(LN.decode(LN.phases(again.words, s_lwe), t)) == [int(a * b % P) for a, b in zip(xv[:64], yv[:64])]
    print(f"\nworst |error| log2, t = 3, nu = 0: level-1 outputs {_log2_worst(e1):.1f}, packed coefficients q box {_log2_worst(e2):.1f}, "
          f"other packed coefficients {_log2_worst(e2_rest):.1f}, tree_lookup outputs {_log2_worst(e):.1f}, after an identity lookup "
          f"{_log2_worst(e3):.1f} (margin: half a box, 2^59)")
    assert max(abs(int(v)) for v in list(e) + list(e3)) < half_box


@pytest.mark.timeout(1200)
def test_tree_lookup_with_level_one_from_the_many_bootstrap(pkg, keys):
    """t = 2, nu = 2: all 16 pairs through (x y) mod 4, twice; level 1 is one fhe_tfhe_lut_many_bootstrap_dev whose
    function-major output the packing key switch reads through its strides.  The decoding condition, |error| < 2^60."""
    from fhe_study_amd import tfhe

    btk, pk, s_lwe, s_glwe, mul, rng = keys
    t, P = 2, 4
    prod = np.array([[int(LN.encode(x * y % P, t)) for y in range(P)] for x in range(P)], dtype=np.uint64)
    xv, yv = np.tile(np.repeat(np.arange(P), P), 2), np.tile(np.tile(np.arange(P), P), 2)
    x, y = _encrypt(rng, s_lwe, xv, t), _encrypt(rng, s_lwe, yv, t)
    out = tfhe.tree_lookup(btk, pk, t, prod, tfhe.TLWE(x), tfhe.TLWE(y), nu=t)
    e = LN.phase_error(out.words, s_lwe, prod[xv, yv])
    print(f"\nworst |error| log2, t = 2, nu = 2: tree_lookup outputs {_log2_worst(e):.1f} (margin: half a box, 2^60)")
    assert list(LN.decode(LN.phases(out.words, s_lwe), t)) == [int(a * b % P) for a, b in zip(xv, yv)]
    assert max(abs(int(v)) for v in e) < 1 << 60
