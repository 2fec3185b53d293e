"""Several lookup tables from one blind rotation on the device: fhe_tfhe_lut_many_bootstrap_dev with nu = 0
against fhe_tfhe_lut_bootstrap_dev; word for word against the existing device chain (gadget blind rotation of the
pre-rounded rows with the interleaved test vector, sample extraction at every h, gadget key switch); one anchor computed
entirely in numpy; outputs inside the pool and the overlap rejections; then lookups and the t = 3 radix adder with real
keys, with and without sharing."""
import numpy as np
import pytest

import _gadget_numpy as G
import _lut_numpy as LN
import _lutmany_numpy as LM
import _tfhe_numpy as R
from test_bootstrap_gpu import _dev, _edge_lwe, _rand_dev, _u64
from test_lut_gpu import _desc_dev, _lut_dev, _prepare_bsk, _random_desc

pytestmark = pytest.mark.gpu


def _many_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, t, nu, luts, pool, desc):
    import torch

    L, B = pkg.load_library(), pkg.binding
    out = torch.empty((1 << nu, len(desc), n_lwe + 1), dtype=torch.int64, device="cuda")
    dp, dd, dl = _dev(pool), _desc_dev(desc), _dev(luts)
    B._check(L.fhe_tfhe_lut_many_bootstrap_dev(n, 1, b, l, n_lwe, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), t, nu, dl.data_ptr(), len(luts),
                                               dp.data_ptr(), pool.shape[0], dd.data_ptr(), out.data_ptr(), len(desc), None))
    return _u64(out)


def _chain_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, table, lwe, F):
    """the existing calls: gadget blind rotation with `table` [2][n], extraction at h = 0 .. F - 1, gadget key switch
    -> [F][rows][n_lwe + 1]"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    rows = lwe.shape[0]
    acc = torch.empty((rows, 2, n), dtype=torch.int64, device="cuda")
    ext = torch.empty((rows, n + 1), dtype=torch.int64, device="cuda")
    outs = [torch.empty((rows, n_lwe + 1), dtype=torch.int64, device="cuda") for _ in range(F)]     # each its own allocation: 16-byte aligned
    dt, dl = _dev(table), _dev(lwe)
    B._check(L.fhe_tfhe_gadget_blind_rotation_dev(n, 1, b, l, n_lwe, prep.data_ptr(), dt.data_ptr(), dl.data_ptr(), acc.data_ptr(), rows, None))
    for h in range(F):
        B._check(L.fhe_tglwe_sample_extraction_dev(n, 1, h, acc.data_ptr(), ext.data_ptr(), rows, None))
        B._check(L.fhe_tlwe_gadget_key_switch_dev(n, n_lwe, ks_b, ks_l, ksk.data_ptr(), ext.data_ptr(), outs[h].data_ptr(), rows, None))
    return np.stack([_u64(o) for o in outs])


def _many_desc(rng, batch, wires, lut_count, t, nu):
    """_random_desc with lut drawn from [0, lut_count - F]; its out-of-range table rows name lut_count - F + 1 and
    0xFFFFFFFF; one more row names lut_count - 1.  All three are invalid for F > 1."""
    F = 1 << nu
    d = _random_desc(rng, batch, wires, lut_count - F + 1, t)
    d[9 if batch > 9 else 2] = (lut_count - 1, 0, 1, 1, 1, 0)
    return d


def test_nu_0_equals_the_lut_bootstrap_word_for_word(pkg):
    n, n_lwe, b, l, t, batch = 256, 8, 8, 3, 4, 70
    ks_b, ks_l, lut_count, wires = 4, 4, 5, 23
    rng = np.random.default_rng(n + n_lwe + batch + t)                          # §14's mixed descriptors at this shape
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, _rand_dev((n_lwe, 2, l, 2, n), 11 + batch))
    ksk = _rand_dev((n, ks_l, n_lwe + 1), 12 + batch)
    luts = rng.integers(0, 1 << 64, (lut_count, 1 << t), dtype=np.uint64, endpoint=False)
    pool = _edge_lwe(rng, wires, n_lwe, n)
    desc = _random_desc(rng, batch, wires, lut_count, t)
    want = _lut_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, t, luts, pool, desc)
    got = _many_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, t, 0, luts, pool, desc)
    ok = LN.valid(desc, wires, lut_count)
    assert got.shape == (1, batch, n_lwe + 1) and ok.any() and not ok.all() and want[ok].any()
    assert np.array_equal(got[0], want)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n,n_lwe,b,l,t,nu,batch", [(256, 8, 8, 3, 4, 1, 70), (256, 8, 8, 3, 4, 4, 9), (256, 8, 8, 3, 7, 1, 5),
                                                    (1024, 16, 8, 3, 4, 2, 1024), (1024, 16, 8, 3, 4, 2, 1025), (1024, 630, 10, 3, 3, 1, 37)])
def test_many_bootstrap_word_exact_against_the_device_chain(pkg, n, n_lwe, b, l, t, nu, batch):
    """per distinct valid first table: the existing gadget blind rotation with expand_many(luts[lut : lut + F]) on the
    pre-rounded combined rows, extraction at each h, the gadget key switch.  (256, t = 4, nu = 4): nu = L - t, F = box;
    (256, t = 7, nu = 1): box = 2, half = 1; N = 1024 with BSK (8, 3): the step split at batch 1024, the key switch over
    4 batch rows; (1024, 630, (10, 3)): a partial key-switch tile at the production key shape."""
    ks_b, ks_l, wires = 4, 4, 23
    F = 1 << nu
    lut_count = F + 4                                                           # first tables 0 .. 4 are valid
    rng = np.random.default_rng(n + n_lwe + batch + t + 100 * nu)
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, _rand_dev((n_lwe, 2, l, 2, n), 11 + batch))
    ksk = _rand_dev((n, ks_l, n_lwe + 1), 12 + batch)
    luts = rng.integers(0, 1 << 64, (lut_count, 1 << t), dtype=np.uint64, endpoint=False)
    pool = _edge_lwe(rng, wires, n_lwe, n)
    desc = _many_desc(rng, batch, wires, lut_count, t, nu)
    got = _many_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, t, nu, luts, pool, desc)
    ok = LM.valid_many(desc, wires, lut_count, nu)
    bad_lut = desc[:, 0].astype(np.int64) + F > lut_count
    assert {lut_count - F + 1, lut_count - 1, 0xFFFFFFFF} <= {int(x) for x in desc[bad_lut, 0]} and not ok[bad_lut].any()
    rows = LM.prerounded(LM.combine_many(pool, desc, lut_count, nu), n, nu)
    want = np.zeros_like(got)
    for i in sorted({int(x) for x in desc[ok, 0]}):
        sel = ok & (desc[:, 0] == i)
        want[:, sel] = _chain_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, LM.expand_many(luts[i:i + F], n), rows[sel], F)
    assert got.shape == (F, batch, n_lwe + 1) and ok.any() and not ok.all()
    assert not got[:, ~ok].any()                                                # invalid rows: zero in all F slices
    assert all(want[h][ok].any() for h in range(F))
    assert np.array_equal(got, want)


@pytest.mark.timeout(600)
def test_many_bootstrap_equals_the_numpy_twin(pkg):
    """independent of the device path: every word from tests/_lutmany_numpy.bootstrap_rows_many"""
    n, n_lwe, b, l, ks_b, ks_l, t, nu, batch, lut_count, wires = 256, 8, 8, 3, 4, 4, 4, 1, 6, 3, 5
    rng = np.random.default_rng(78)
    bsk = rng.integers(0, 1 << 64, (n_lwe, 2, l, 2, n), dtype=np.uint64, endpoint=False)
    ksk = rng.integers(0, 1 << 64, (n, ks_l, n_lwe + 1), dtype=np.uint64, endpoint=False)
    luts = rng.integers(0, 1 << 64, (lut_count, 1 << t), dtype=np.uint64, endpoint=False)
    pool = _edge_lwe(rng, wires, n_lwe, n)
    desc = (np.array([(0, 0, 1, 1, 1, 0), (1, 2, 3, -2, 3, 5 << 27), (1, 4, 0xFFFFFFFF, 4, 0, 0), (2, 0, 1, 1, 1, 0), (0, wires, 1, 1, 1, 0),
                      (0, 3, 4, 1, -1, 1 << 31)], dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)
    assert len(desc) == batch
    got = _many_dev(pkg, n, b, l, n_lwe, _prepare_bsk(pkg, n, b, l, n_lwe, _dev(bsk)), ks_b, ks_l, _dev(ksk), t, nu, luts, pool, desc)
    want = LM.bootstrap_rows_many(n, b, l, bsk, ks_b, ks_l, ksk, luts, pool, desc, nu)
    assert not want[:, 3].any() and not want[:, 4].any() and want[0, 0].any() and want[1, 0].any()      # row 3: lut + F > lut_count
    assert np.array_equal(got, want)


@pytest.mark.timeout(600)
def test_outputs_inside_the_pool_and_overlaps(pkg):
    """the evaluator's layout: d_out [F][batch] is a slice of the pool after the rows the descriptors read and gives the
    words of a separate buffer; any of the F slices reaching into the tables, a key or the descriptors is FHE_E_INVALID.
    (The call cannot see which pool rows the descriptors read without reading device memory: keeping d_out off those rows
    is the caller's part, as in §13/§14.)"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, n_lwe, b, l, ks_b, ks_l, t, nu, wires, batch, lut_count = 256, 8, 8, 3, 4, 4, 4, 2, 10, 20, 7    # 10 rows of 9 words: d_out 16-byte aligned
    F = 1 << nu
    rng = np.random.default_rng(5)
    prep = _prepare_bsk(pkg, n, b, l, n_lwe, _rand_dev((n_lwe, 2, l, 2, n), 5))
    ksk = _rand_dev((n, ks_l, n_lwe + 1), 6)
    luts = rng.integers(0, 1 << 64, (lut_count, 1 << t), dtype=np.uint64, endpoint=False)
    pool = _edge_lwe(rng, wires, n_lwe, n)
    desc = _many_desc(rng, batch, wires, lut_count, t, nu)
    dd, dl = _desc_dev(desc), _dev(luts)
    dp = torch.zeros((wires + F * batch + 1, n_lwe + 1), dtype=torch.int64, device="cuda")
    dp[:wires] = _dev(pool)
    dp[-1] = 0x5A5A

    def call(out_ptr, desc_ptr=dd.data_ptr(), lut_ptr=dl.data_ptr(), bsk_ptr=prep.data_ptr(), ksk_ptr=ksk.data_ptr()):
        return L.fhe_tfhe_lut_many_bootstrap_dev(n, 1, b, l, n_lwe, bsk_ptr, ks_b, ks_l, ksk_ptr, t, nu, lut_ptr, lut_count, dp.data_ptr(), wires,
                                                 desc_ptr, out_ptr, batch, None)

    B._check(call(dp[wires:].data_ptr()))
    want = _many_dev(pkg, n, b, l, n_lwe, prep, ks_b, ks_l, ksk, t, nu, luts, pool, desc)
    got = _u64(dp)
    assert np.array_equal(got[:wires], pool) and want.any() and (got[-1] == 0x5A5A).all()
    assert np.array_equal(got[wires:-1].reshape(F, batch, n_lwe + 1), want)
    # overlaps: a buffer placed so that only the last of the F slices of d_out reaches into it
    row = (n_lwe + 1) * 8
    big = torch.zeros(2 * F * batch * (n_lwe + 1) + 64, dtype=torch.int64, device="cuda")
    out_ptr = big.data_ptr()
    inside = out_ptr + (F - 1) * batch * row + 16 * row                        # inside slice F - 1, 16-byte aligned
    assert inside % 16 == 0 and inside < out_ptr + F * batch * row
    for kw in (dict(desc_ptr=inside), dict(lut_ptr=inside), dict(bsk_ptr=inside), dict(ksk_ptr=inside)):
        assert call(out_ptr, **kw) == B.FHE_E_INVALID, kw
        assert b"overlap" in L.fhe_last_error() and b"fhe_tfhe_lut_many_bootstrap_dev" in L.fhe_last_error()
    torch.cuda.synchronize()
    assert not _u64(big).any()                                                  # nothing was written


def test_rejections_return_invalid_and_launch_nothing(pkg):
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, n_lwe, b, l, ks_b, ks_l, t, wires, batch, lut_count = 256, 8, 8, 3, 4, 4, 4, 4, 3, 4
    prep = torch.zeros(L.fhe_tfhe_gadget_bsk_prepared_words(n, 1, b, l, n_lwe), dtype=torch.int64, device="cuda")
    ksk = torch.zeros((n, ks_l, n_lwe + 1), dtype=torch.int64, device="cuda")
    luts = torch.zeros((lut_count, 1 << 8), dtype=torch.int64, device="cuda")
    pool = torch.zeros((wires, n_lwe + 1), dtype=torch.int64, device="cuda")
    desc = _desc_dev(np.zeros((batch + 1, 6), dtype=np.uint32))
    out = torch.full((4 * batch + 1, n_lwe + 1), 0x5A5A, dtype=torch.int64, device="cuda")

    def call(n=n, k=1, b=b, l=l, t=t, nu=2, lut_count=lut_count, wires=wires, batch=batch):
        return L.fhe_tfhe_lut_many_bootstrap_dev(n, k, b, l, n_lwe, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), t, nu, luts.data_ptr(), lut_count,
                                                 pool.data_ptr(), wires, desc.data_ptr(), out.data_ptr(), batch, None)

    B.kernel_timing_reset()
    B.kernel_timing_enable(True)                                                # every launch of the library is recorded by name
    try:
        for kw in (dict(t=0), dict(t=9), dict(nu=5), dict(t=5, nu=4), dict(t=8, nu=1), dict(lut_count=0), dict(k=2), dict(b=33, l=1),
                   dict(wires=0), dict(batch=0), dict(n=128)):
            assert call(**kw) == B.FHE_E_INVALID, kw
            assert b"fhe_tfhe_lut_many_bootstrap_dev" in L.fhe_last_error()
        torch.cuda.synchronize()
        assert B.kernel_timing_read() == {}                                     # nothing was launched
        assert (_u64(out) == 0x5A5A).all()                                      # and nothing written
        assert call(t=6, nu=2) == B.FHE_OK                                      # nu = L - t is admitted
        torch.cuda.synchronize()
        names = B.kernel_timing_read()
        assert "tfhe_lut_many_init_8" in names and "tfhe_many_extract_8" in names and "tfhe_lut_init_8" not in names
        assert names["tlwe_gadget_key_switch_0"][1] == 1                  # one key switch over the F batch rows
    finally:
        B.kernel_timing_enable(False)
        B.kernel_timing_reset()
    assert not _u64(out)[:4 * batch].any() and (_u64(out)[4 * batch:] == 0x5A5A).all()      # zero keys and tables: zero rows


# ---- real keys: the parameters and key recipe of test_lut_gpu.py --------------------------------------------------------------
N, NL, BSK, KSK, SIGMA = 1024, 630, (10, 3), (4, 4), 3.2


@pytest.fixture(scope="module")
def keys(pkg):
    from fhe_study_amd import tfhe

    B = pkg.binding
    rng = np.random.default_rng(1515)
    s_glwe = rng.integers(0, 2, N, dtype=np.uint64)
    s_lwe = rng.integers(0, 2, NL, dtype=np.uint64)
    mul = lambda a, x: B.tn_mul(N, a, np.ascontiguousarray(x))
    bsk = G.tggsw_bits(rng, mul, N, BSK[0], BSK[1], s_glwe, s_lwe, SIGMA)
    ksk = G.ksk(rng, s_glwe, s_lwe, KSK[0], KSK[1], SIGMA)
    btk = tfhe.BootstrappingKey(N, 1, BSK[1], NL, bsk, ksk, ks_l=KSK[1], log_beta=BSK[0], ks_log_beta=KSK[0])
    return btk, s_lwe, rng


def _encrypt(rng, s, values, t):
    return R.lwe_encrypt(rng, s, [LN.encode(v, t) for v in np.asarray(values).reshape(-1)], SIGMA)


def _worst(e):
    return float(np.log2(float(max(max(abs(x) for x in np.asarray(e, dtype=object).reshape(-1)), 1))))


@pytest.mark.timeout(1200)
def test_lookups_with_real_keys_at_t3_nu1_and_t2_nu2(pkg, keys):
    """(t, nu) = (3, 1): in one call all 8 values through the groups (x mod 4, x div 4) and (identity, x^2 mod 8);
    (t, nu) = (2, 2): all 4 values through a group of four tables.  Every row decrypts to the expected value and every
    output |phase error| is below Delta / 2 (the decoding condition).  Observed worst |phase error|:
    see the table there."""
    from fhe_study_amd import tfhe

    btk, s, rng = keys
    for t, nu, groups in ((3, 1, [[lambda v: v % 4, lambda v: v // 4], [lambda v: v, lambda v: v * v % 8]]),
                          (2, 2, [[lambda v: v, lambda v: (v + 1) % 4, lambda v: v * v % 4, lambda v: 3 - v]])):
        P, F = 1 << t, 1 << nu
        fs = [f for g in groups for f in g]
        luts = [tfhe.make_lut(f, t) for f in fs]
        pool = _encrypt(rng, s, np.arange(P), t)
        desc = [(F * gi, x, tfhe.LUT_NONE, 1, 0, 0) for gi in range(len(groups)) for x in range(P)]
        out = tfhe.lut_many_bootstrap(btk, t, nu, luts, desc, pool)
        assert out.words.shape == (F, len(desc), NL + 1)
        worst = 0.0
        for h in range(F):
            want_vals = [groups[gi][h](x) for gi in range(len(groups)) for x in range(P)]
            want = np.array([LN.encode(v, t) for v in want_vals], dtype=np.uint64)
            assert list(LN.decode(LN.phases(out.words[h], s), t)) == want_vals, (t, nu, h)
            worst = max(worst, _worst(LN.phase_error(out.words[h], s, want)))
        print(f"\n(t, nu) = ({t}, {nu}): worst |phase error| log2 {worst:.1f} (margin: half a box, 2^{62 - t})")
        assert worst < 62 - t


def _adder_pairs():
    edge = [(x, y) for x in (0, 1, 85, 255) for y in (0, 1, 85, 255)]
    rnd = np.random.default_rng(2024).integers(0, 256, (240, 2))
    p = np.array(edge + [tuple(r) for r in rnd])
    return p[:, 0], p[:, 1]


@pytest.mark.timeout(1200)
def test_t3_radix_adder_over_256_pairs_with_and_without_sharing(pkg, keys):
    """the 4-digit base-4 adder in t = 3 over §14's 256 pairs, once with evaluate(share=1) (one nu = 1 call per digit) and
    once with share=0 (one call of twice the rows per digit): both give a + b, carry-out digit included, with every output
    |phase error| below Delta / 2 = 2^59"""
    from fhe_study_amd import tfhe

    btk, s, rng = keys
    D, t = 4, 3
    xs, ys = _adder_pairs()
    ins = [tfhe.TLWE(_encrypt(rng, s, (xs >> (2 * i)) & 3, t)) for i in range(D)] + \
          [tfhe.TLWE(_encrypt(rng, s, (ys >> (2 * i)) & 3, t)) for i in range(D)]
    c = LM.radix_adder(tfhe.LutCircuit(), D, t)
    want = [((xs + ys) >> (2 * i)) & 3 for i in range(D + 1)]
    for share in (1, 0):
        outs = c.evaluate(btk, ins, t, share=share)
        assert len(outs) == D + 1 and outs[0].words.shape == (256, NL + 1)
        digits = [LN.decode(LN.phases(o.words, s), t) for o in outs]
        worst = max(_worst(LN.phase_error(o.words, s, np.array([LN.encode(v, t) for v in wv], dtype=np.uint64))) for o, wv in zip(outs, want))
        print(f"\nshare = {share}: worst |phase error| log2 over the adder's outputs {worst:.1f} (margin: half a box, 2^59)")
        assert all(d.max() < 4 for d in digits), share
        assert np.array_equal(sum(d << (2 * i) for i, d in enumerate(digits)), xs + ys), share
        assert worst < 59, share


@pytest.mark.timeout(600)
@pytest.mark.parametrize("batch", [1, 3])
def test_lut_circuit_with_sharing_equals_the_node_by_node_evaluation(pkg, batch):
    """toy keys (random words: exactness needs no real keys), an odd batch (a padded, invalid row per wire) and a netlist
    with classes of 3 and 5 lookups, a second level and a lin: evaluate(share=2) gives, word for word, what the node-by-node
    evaluation through tfhe.lut_many_bootstrap (nu of the wire's chunk, the wire's function) and tfhe.lincomb gives"""
    from fhe_study_amd import tfhe

    n, n_lwe, b, l, ks_b, ks_l, t, share = 256, 8, 8, 3, 4, 4, 3, 2
    rng = np.random.default_rng(700 + batch)
    bsk = rng.integers(0, 1 << 64, (n_lwe, 2, l, 2, n), dtype=np.uint64, endpoint=False)
    ksk = rng.integers(0, 1 << 64, (n, ks_l, n_lwe + 1), dtype=np.uint64, endpoint=False)
    btk = tfhe.BootstrappingKey(n, 1, l, n_lwe, bsk, ksk, ks_l=ks_l, log_beta=b, ks_log_beta=ks_b)
    c = tfhe.LutCircuit()
    x, y = c.input(), c.input()
    tabs = [rng.integers(0, 1 << 64, 1 << t, dtype=np.uint64, endpoint=False) for _ in range(9)]
    three = [c.lut(tabs[j], x, 1, y, -2, const=1) for j in range(3)]
    five = [c.lut(tabs[3 + j], y, 3) for j in range(5)]
    single = c.lut(tabs[8], x, 1, y, 1)
    m = c.lin(three[2], 1, five[4], -1, const=2)
    second = [c.lut(tabs[j], m, 1, single, 1) for j in (0, 1)]
    for w_ in three + five + [single, m] + second:
        c.output(w_)
    p = c.plan(share=share)
    assert [{mm["nu"]: mm["chunks"] for mm in lv["many"]} for lv in p.levels] == [{2: 2}, {1: 1}] and p.levels[0]["luts"][1] == 2
    ins = [tfhe.TLWE(_edge_lwe(rng, max(batch, 2), n_lwe, n)[:batch]) for _ in range(2)]
    got = c.evaluate(btk, ins, t, share=share)
    # node by node: a wire's chunk is found from the plan (its class's members, in chunks of 2^share)
    i = np.arange(batch)
    vals, it = [], iter(ins)
    for w_, (kind, args) in enumerate(c._nodes):
        if kind == "input":
            vals.append(next(it))
            continue
        xw, sx, yw, sy, const = args[1:] if kind == "lut" else args
        zero = np.zeros((batch, n_lwe + 1), dtype=np.uint64)
        pool = np.concatenate([vals[xw].words if xw is not None else zero, vals[yw].words if yw is not None else zero])
        desc = np.stack([np.zeros(batch, dtype=np.int64), i if xw is not None else np.full(batch, tfhe.LUT_NONE),
                         i + batch if yw is not None else np.full(batch, tfhe.LUT_NONE), np.full(batch, sx), np.full(batch, sy),
                         np.full(batch, int(tfhe.encode_int(const, t)) >> 32)], axis=1)
        if kind == "lin":
            vals.append(tfhe.lincomb(desc, pool))
            continue
        mates = [v for v, (k2, a2) in enumerate(c._nodes) if k2 == "lut" and a2[1:] == args[1:]]
        pos = mates.index(w_)
        chunk = mates[pos - pos % (1 << share): pos - pos % (1 << share) + (1 << share)]
        nu = (len(chunk) - 1).bit_length()
        ids = [c._nodes[v][1][0] for v in chunk]
        ids += [ids[0]] * ((1 << nu) - len(ids))
        out = tfhe.lut_many_bootstrap(btk, t, nu, [c.tables[j] for j in ids], desc, pool)
        vals.append(tfhe.TLWE(out.words[chunk.index(w_)]))
    assert len(got) == len(c._outputs)
    for o, w_ in zip(got, c._outputs):
        assert o.words.shape == (batch, n_lwe + 1)
        assert np.array_equal(o.words, vals[w_].words), w_
    assert got[0].words.any()
