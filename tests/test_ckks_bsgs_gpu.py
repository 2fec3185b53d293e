"""The baby-step giant-step linear transform with hoisted giant steps on the device (ckks_eval.hip):
fhe_ckks_rns_bsgs_dev word for word against tests/_ckks_bsgs_numpy.py (tolerance zero) on the case list
tests/test_ckks_bsgs_cpu.py proved; edge residues; the launch counts (and diag_sum's and rotate_many's beside them); the
functional case through ckks.RnsClientKey with its bound; the Python surface; every rejection with its output untouched."""
import numpy as np
import pytest

import _ckks_bsgs_numpy as BN
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_linear_numpy as LN
import _ckks_numpy as K
import _client_numpy as C
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
FILL = 0x5A5A5A5A5A5A5A5A


def _refused():
    return pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ")


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _plans(pkg, mods, n):
    return [pkg.Plan(q, n) for q in mods]


def _ptrs(d_keys):
    return [None if x is None else x.data_ptr() for x in d_keys]


def _bsgs(pkg, plans, sp, d_baby, baby_gs, d_giant, giant_gs, kl, d_pts, d_ct):
    out = _empty(tuple(d_ct.shape))
    pkg.binding.ckks_rns_bsgs_dev(plans, sp, _ptrs(d_baby), baby_gs, _ptrs(d_giant), giant_gs, kl, d_pts.data_ptr(), d_ct.data_ptr(), out.data_ptr(), d_ct.shape[2])
    return _u64(out)


def _keys_dev(keys):
    return [None if x is None else _dev(x) for x in keys]


def _check_case(pkg, mods, P, plans, sp, n, batch, baby_gs, giant_gs, case):
    """the call at k limbs and, with the same full-chain keys, one level down"""
    k = len(mods)
    ct, baby, giant, pts = case
    d_ct, d_baby, d_giant = _dev(ct), _keys_dev(baby), _keys_dev(giant)
    got = _bsgs(pkg, plans, sp, d_baby, baby_gs, d_giant, giant_gs, k, _dev(pts), d_ct)
    assert np.array_equal(got, BN.bsgs(mods, P, baby, baby_gs, giant, giant_gs, pts, ct)), (n, k, batch, baby_gs, giant_gs)
    if k > 1:
        low_pts = BN.lower(pts, k)
        low = _bsgs(pkg, plans[:-1], sp, d_baby, baby_gs, d_giant, giant_gs, k, _dev(low_pts), _dev(ct[:-1]))
        assert np.array_equal(low, BN.bsgs(mods[:-1], P, baby, baby_gs, giant, giant_gs, low_pts, ct[:-1])), (n, k, batch, baby_gs, giant_gs, "low")
    assert np.array_equal(_u64(d_ct), ct)                                    # the input is only read


# ---- word for word -------------------------------------------------------------------------------------------------------------------
def test_first_case_word_for_word(pkg):
    n, k, batch, spec = BN.WORD_CASES[0]
    mods, P = E.case_chain(n, k, spec)
    baby_gs, giant_gs = BN.reduced(BN.SWEEP[0], n), [5 % (2 * n)]
    _check_case(pkg, mods, P, _plans(pkg, mods, n), pkg.Plan(P, n), n, batch, baby_gs, giant_gs, BN.random_case(mods, P, n, batch, baby_gs, giant_gs, 1))


@pytest.mark.parametrize("n,k,batch,spec", BN.WORD_CASES)
def test_sweep_word_for_word(pkg, n, k, batch, spec):
    mods, P = E.case_chain(n, k, spec)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    lists = [(BN.reduced(BN.SWEEP[0], n), BN.reduced(BN.SWEEP[1], n))] + BN.element_cases(n)
    for t, (baby_gs, giant_gs) in enumerate(lists):
        _check_case(pkg, mods, P, plans, sp, n, batch, baby_gs, giant_gs, BN.random_case(mods, P, n, batch, baby_gs, giant_gs, 900 * n + 10 * k + t))


def test_wide_chain_word_for_word(pkg):
    n, k, batch, spec = BN.WIDE_CASE
    mods, P = E.case_chain(n, k, spec)
    assert mods[0] >= 1 << 62 and P >= 1 << 62
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    for t, (baby_gs, giant_gs) in enumerate([BN.SWEEP, ([1, 5, 2 * n - 1], [5, 2 * n - 1, 5])]):
        _check_case(pkg, mods, P, plans, sp, n, batch, baby_gs, giant_gs, BN.random_case(mods, P, n, batch, baby_gs, giant_gs, 31 + t))


def test_over_several_chunks_and_past_the_grid_cap(pkg):
    n, k, batch, spec = BN.BIG_CASE
    mods, P = E.case_chain(n, k, spec)
    baby_gs, giant_gs = BN.SWEEP
    _check_case(pkg, mods, P, _plans(pkg, mods, n), pkg.Plan(P, n), n, batch, baby_gs, giant_gs, BN.random_case(mods, P, n, batch, baby_gs, giant_gs, 77))


@pytest.mark.parametrize("spec", [(58, 40), "wide"])
def test_edge_residues(pkg, spec):
    """every word q - 1, P included, in the ciphertext, the keys and the plaintexts: the fold rule's worst case, below 2^62 and
    on the chain whose first limb and special prime are >= 2^62, at three giants and seventeen babies"""
    n, batch = 16, 2
    k = 8 if spec == "wide" else 3
    mods, P = E.case_chain(n, k, spec)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    baby_gs, giant_gs = BN.element_cases(n)[3][0], [5, 1, 25]
    _check_case(pkg, mods, P, plans, sp, n, batch, baby_gs, giant_gs, BN.edge_case(mods, P, n, batch, baby_gs, giant_gs))


def test_anchors_to_existing_entry_points(pkg):
    """every giant the identity: fhe_ckks_rns_diag_sum_dev with one output over the giants x babies elements; one giant over the
    identity baby at m = 1: fhe_ckks_rns_galois_dev"""
    B = pkg.binding
    n, k, batch = 16, 3, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    baby_gs, giant_gs = [1, 5, 2 * n - 1], [1, 1, 1]
    ct, baby, giant, pts = BN.random_case(mods, P, n, batch, baby_gs, giant_gs, 12)
    d_ct, d_baby, d_pts = _dev(ct), _keys_dev(baby), _dev(pts)
    one_out = _empty((1,) + ct.shape)
    B.ckks_rns_diag_sum_dev(plans, sp, _ptrs(d_baby * 3), baby_gs * 3, k, d_pts.data_ptr(), 1, d_ct.data_ptr(), one_out.data_ptr(), batch)
    assert np.array_equal(_bsgs(pkg, plans, sp, d_baby, baby_gs, [None] * 3, giant_gs, k, d_pts, d_ct), _u64(one_out)[0])
    one = _dev(np.ones((1, 1, k + 1, n), dtype=U64))
    for h in (5, 2 * n - 1):
        d_gk = _dev(LN.random_keys(mods, P, n, [h], 5)[0])
        rot = _empty((1,) + ct.shape)
        B.ckks_rns_galois_dev(plans, sp, [d_gk.data_ptr()], [h], k, d_ct.data_ptr(), rot.data_ptr(), batch)
        assert np.array_equal(_bsgs(pkg, plans, sp, [None], [1], [d_gk], [h], k, one, d_ct), _u64(rot)[0]), h


# ---- the launch counts of §30 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_launch_counts(pkg, k):
    import torch

    B = pkg.binding
    n, batch = 64, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    a = _dev(E.case_ct(mods, n, batch, 2, 9))
    R = BN.GROUP + 1
    keys = [_dev(np.random.default_rng(10 + r).integers(0, 1 << 39, (k, k + 1, 2, n), dtype=np.uint64)) for r in range(3)]
    d_pts = _dev(np.random.default_rng(3).integers(0, 1 << 39, (3, R, k + 1, n), dtype=np.uint64))
    out = _empty((3, k, 2, batch, n))
    labels = ("tensor", "lift", "keymac", "divround", "galois", "diagmac", "giantmac")

    def counts(fn):
        torch.cuda.synchronize()
        B.kernel_timing_enable(True)
        B.kernel_timing_reset()
        try:
            fn()
            torch.cuda.synchronize()
            got = B.kernel_timing_read(256)
        finally:
            B.kernel_timing_enable(False)
        return {lab: sum(c for name, (_, c) in got.items() if name.startswith("ckks_rns_" + lab)) for lab in labels}

    def ptrs(gs):
        return [None if g == 1 else keys[g % 3].data_ptr() for g in gs]
    long = BN.element_cases(n)[3][0]
    for baby_gs in ([1], [5], [1, 5, 25], long[:BN.GROUP], long, [1] * R):
        for giant_gs in ([1], [25], [1, 25], [25, 1, 5], [1, 1, 1]):
            pt = d_pts[:len(giant_gs), :len(baby_gs)].contiguous()
            got = counts(lambda: B.ckks_rns_bsgs_dev(plans, sp, ptrs(baby_gs), baby_gs, ptrs(giant_gs), giant_gs, k, pt.data_ptr(), a.data_ptr(), out[0].data_ptr(), batch))
            assert got == dict(BN.launch_counts(k, baby_gs, giant_gs, 1), tensor=0, galois=0), (k, baby_gs, giant_gs)
    # §23's and §24's counts are as they were
    gs = [5, 25, 2 * n - 1]
    pt = d_pts[:3, :3].contiguous()
    got = counts(lambda: B.ckks_rns_diag_sum_dev(plans, sp, ptrs(gs), gs, k, pt.data_ptr(), 3, a.data_ptr(), out.data_ptr(), batch))
    assert got == dict(LN.launch_counts(k, 3, 3, 1), tensor=0, galois=0, giantmac=0)
    got = counts(lambda: B.ckks_rns_galois_dev(plans, sp, ptrs(gs), gs, k, a.data_ptr(), out.data_ptr(), batch))
    assert got == dict(tensor=0, lift=k + 3, keymac=3 * (k + 1), divround=3 * k, galois=0, diagmac=0, giantmac=0)


# ---- the functional case and the Python surface --------------------------------------------------------------------------------------------
def test_dense_matrix_through_the_client_key(pkg, tab):
    """n = 32, L = 2, Delta = 2^40, a dense matrix of Gaussian integers in [-3, 3]: the words of the restatement under the restated
    keys; after the rescale the slots within the bound and equal to the exact rounded product; within the two noise bounds of
    linear_transform after decryption"""
    ck = pkg.ckks
    case = LN.FUNCTIONAL["n32"]
    n = case["n"]
    N = n // 2
    M = LN.matrices(N, case["rng"])["dense"]
    mods, P = E.chain(n, case["b0"], case["bd"], case["L"])
    k = len(mods)
    delta, dpt = LN.functional_scales(n, mods, case["bd"], N)
    assert delta == 2.0 ** 40
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(case["seed"], param, delta)
    z = E.functional_slots(case, 1)
    w = G.to_rotation_order(z)
    ct = key.encrypt(key.public_key(0), K.encode(z, delta))
    lt = ck.LinearTransform.from_matrix(param, key.encoder, M, k - 1, dpt)
    steps = lt.required_steps()
    keys = {st: key.rotation_key(st, slot) for slot, st in enumerate(steps)}
    res = ct.linear_transform_hoisted(lt, keys)
    assert res.level == k - 1 and res.scale == delta * dpt and res.batch == ct.batch
    # the words
    s = K.secret_key(case["seed"], 0, n)
    gk = {st: G.galois_key(case["seed"], G.GK_BASE + 64 * slot, s, mods, P, tab, G.galois_element(n, st)) for slot, st in enumerate(steps)}
    pts = _u64(lt.pts.d_pts)
    giant_gs = [G.galois_element(n, lt.n1 * j) for j in lt.giant]
    want = BN.bsgs(mods, P, [gk[i] if i else None for i in lt.baby], lt.pts.gs, [gk[lt.n1 * j] if j else None for j in lt.giant], giant_gs, pts, _u64(ct.d))
    assert np.array_equal(_u64(res.d), want)
    # against linear_transform, after decryption at limb 0
    coef = K.centre(E.inv(P, n, pts[..., -1, :]), P)
    norm1 = [[float(np.abs(coef[a, b]).sum()) for b in range(len(lt.baby))] for a in range(len(lt.giant))]
    sw1 = [[norm1[a][b] for b, i in enumerate(lt.baby) if i] for a in range(len(lt.giant))]
    gsw = [j != 0 for j in lt.giant]
    composed = ct.linear_transform(lt, keys)
    diff = (key.decrypt(res).astype(object) - key.decrypt(composed).astype(object)) % mods[0]     # both are exact modulo q_0
    apart = np.abs(np.where(diff > mods[0] // 2, diff - mods[0], diff)).max()
    both = BN.bsgs_noise(n, k, sw1, gsw) + BN.composed_noise(n, k, sw1, gsw)
    # the slots
    out = res.rescale()
    assert out.level == k - 2 and out.scale == delta
    d = key.decrypt(out)
    got = G.to_rotation_order(key.decrypt_and_decode(out))
    exact = w @ M.T
    rows = LN.bsgs_diagonals(M)[3]
    rmax = [[float(np.abs(rows[a, b]).max()) for b in range(len(lt.baby))] for a in range(len(lt.giant))]
    bound = BN.functional_bound(n, k, delta, dpt, mods[-1], lt.baby, lt.giant, norm1, rmax) + float(K.e_dec(d, delta).max())
    err = float(np.abs(got - exact).max())
    print(f"n={n}: {len(lt.baby)} baby x {len(lt.giant)} giant steps, worst slot error {err:.3e}, derived bound {bound:.3e}; against linear_transform "
          f"{float(apart):.3e} coefficient units, the two bounds {both:.3e}")
    assert float(apart) <= both
    assert err <= bound and err < 0.5
    assert np.array_equal(np.round(got.real), exact.real) and np.array_equal(np.round(got.imag), exact.imag)


def test_python_surface(pkg):
    ck = pkg.ckks
    case = LN.FUNCTIONAL["n32"]
    n = case["n"]
    mods, P = E.chain(n, case["b0"], case["bd"], case["L"])
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(case["seed"], param, 2.0 ** 30)
    ct = key.encrypt(key.public_key(0), K.encode(E.functional_slots(case, 1), 2.0 ** 30))
    M = LN.matrices(n // 2, 5)["banded"]
    lt = ck.LinearTransform.from_matrix(param, key.encoder, M, 2, 2.0 ** 20, 2)
    assert lt.required_steps() == [1, 2, 14]
    keys = {st: key.rotation_key(st, st) for st in (1, 2)}
    with pytest.raises(KeyError, match="14"):
        ct.linear_transform_hoisted(lt, keys)
    keys[14] = key.rotation_key(14, 14)
    before = _u64(ct.d).copy()
    res = ct.linear_transform_hoisted(lt, keys)
    assert res.level == 2 and res.scale == 2.0 ** 50 and res.batch == ct.batch and np.array_equal(_u64(ct.d), before)
    with _refused():
        ct.at_level(1).linear_transform_hoisted(lt, keys)                    # the plaintexts are at another level
    other = ck.RnsParam(n, mods[:2], P)
    with _refused():
        ct.linear_transform_hoisted(lt, {**keys, 2: ck.RnsGaloisKey(other, keys[2].g, keys[2].d_gk)})
    with pytest.raises(ValueError):
        ct.linear_transform_hoisted(lt, {**keys, 2: keys[14]})         # the key of another step


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_output_untouched(pkg):
    B = pkg.binding
    n, k = 16, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    a = _dev(E.case_ct(mods, n, 2, 2, 5))
    key = _dev(E.case_ct(mods, n, 4, 2, 7))
    pts = _dev(LN.random_pts(mods, P, n, 2, 2, 9))
    o = _empty((k, 2, 2, n))
    A, R, PT, O = (x.data_ptr() for x in (a, key, pts, o))
    ct_bytes, pt_bytes = k * 2 * 2 * n * 8, 2 * 2 * (k + 1) * n * 8
    f = B.ckks_rns_bsgs_dev
    good = (plans, sp, [R, R], [5, 25], [R, R], [5, 25], k, PT, A, O, 2)

    def but(**kw):
        names = ("plans", "sp", "bk", "bg", "gk", "gg", "kl", "pt", "a", "o", "batch")
        return tuple(kw.get(name, v) for name, v in zip(names, good))
    bad = [(B.FHE_E_INVALID, but(**{role: [5, g]})) for role in ("bg", "gg") for g in (4, 0, 2 * n, 2 * n + 1)] + [
        (B.FHE_E_INVALID, but(bk=[R] * 257, bg=[5] * 257)),
        (B.FHE_E_INVALID, but(bk=[], bg=[])),
        (B.FHE_E_INVALID, but(gk=[R] * 65, gg=[5] * 65)),
        (B.FHE_E_INVALID, but(gk=[], gg=[])),
        (B.FHE_E_INVALID, but(kl=k - 1)),
        (B.FHE_E_INVALID, but(kl=9)),
        (B.FHE_E_INVALID, but(a=O + 8)),                                     # the input inside the output
        (B.FHE_E_INVALID, but(bk=[R, O + ct_bytes - 8])),                    # a baby key at the output's last word
        (B.FHE_E_INVALID, but(gk=[O - 8 * k * (k + 1) * 2 * n + 8, R])),     # a giant key ending in its first
        (B.FHE_E_INVALID, but(pt=O + ct_bytes - 8)),                         # the plaintexts at the output's last word
        (B.FHE_E_INVALID, but(pt=O - pt_bytes + 8)),                         # ... ending in its first
        (B.FHE_E_INVALID, but(pt=PT + 4)),
        (B.FHE_E_INVALID, but(a=A + 4)),
        (B.FHE_E_INVALID, but(o=O + 4)),
        (B.FHE_E_INVALID, but(bk=[R + 4, R])),
        (B.FHE_E_INVALID, but(gk=[R, R + 4])),
        (B.FHE_E_INVALID, but(sp=plans[0])),
        (B.FHE_E_INVALID, but(sp=pkg.Plan(65537, n))),
        (B.FHE_E_INVALID, but(plans=[plans[0], plans[1], plans[0]])),
        (B.FHE_E_PARAM_MISMATCH, but(plans=[plans[0], plans[1], other])),
        (B.FHE_E_NULL, but(bk=[R, None])),                                   # an element other than 1 needs its key: a baby
        (B.FHE_E_NULL, but(gk=[None, R])),                                   # ... a giant
        (B.FHE_E_NULL, but(bk=None, bg=[1, 25])),
        (B.FHE_E_NULL, but(gk=None, gg=[1, 25])),
        (B.FHE_E_NULL, but(pt=None)),
        (B.FHE_E_NULL, but(a=None)),
        (B.FHE_E_NULL, but(o=None)),
        (B.FHE_E_NULL, but(sp=None)),
    ]
    for code, args in bad:
        with _refused() as e:
            f(*args)
        assert e.value.code == code, args
    f(*but(batch=0))                                                         # batch = 0 writes nothing
    assert (_u64(o) == U64(FILL)).all()
    # the identity's key entry is not read in either role: NULL, or a pointer inside the output
    f(*but(bk=[None, R], bg=[1, 5], gk=[R, None], gg=[25, 1]))
    want = _u64(o).copy()
    f(*but(bk=[O + 8, R], bg=[1, 5], gk=[R, O + 16], gg=[25, 1]))
    assert np.array_equal(_u64(o), want) and not (want == U64(FILL)).any()
    f(*but(bk=None, bg=[1, 1], gk=None, gg=[1, 1]))                          # every element the identity: no key list at all
    assert not (_u64(o) == U64(FILL)).any()
