"""Plaintext linear transforms of the CKKS evaluator on the device (ckks_eval.hip): the double-hoisted diagonal sum
word for word against tests/_ckks_linear_numpy.py (tolerance zero) on the case list tests/test_ckks_linear_cpu.py proved; its
anchors to fhe_ckks_rns_galois_dev and pointwise_mul_dev; edge residues at the largest count; the launch counts; the functional
case through ckks.RnsClientKey with its bound; the Python surface; every rejection with its outputs untouched."""
import numpy as np
import pytest

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


def _diag(pkg, plans, sp, d_gks, gs, kl, d_pts, outputs, d_ct):
    k, _, batch, n = d_ct.shape
    out = _empty((outputs, k, 2, batch, n))
    pkg.binding.ckks_rns_diag_sum_dev(plans, sp, [None if x is None else x.data_ptr() for x in d_gks], gs, kl, d_pts.data_ptr(), outputs, d_ct.data_ptr(),
                                      out.data_ptr(), batch)
    return _u64(out)


def _keys_dev(keys):
    return [None if x is None else _dev(x) for x in keys]


# ---- the sweep, word for word -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch,spec", LN.WORD_CASES)
def test_diag_sum_word_for_word(pkg, n, k, batch, spec):
    mods, P = E.case_chain(n, k, spec)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    ct = E.case_ct(mods, n, batch, 2, 500 * n + k)
    d_ct = _dev(ct)
    top = max(LN.OUTPUTS)
    for t, gs in enumerate(LN.element_lists(n)):
        keys = LN.random_keys(mods, P, n, gs, 40 * n + t)
        pts = LN.random_pts(mods, P, n, top, len(gs), 41 * n + t)
        want = LN.diag_sum(mods, P, keys, gs, pts, ct)
        d_keys = _keys_dev(keys)
        for outputs in LN.OUTPUTS:                                            # the outputs are independent: the first o of the largest call
            got = _diag(pkg, plans, sp, d_keys, gs, k, _dev(pts[:outputs]), outputs, d_ct)
            assert np.array_equal(got, want[:outputs]), (gs, outputs)
        if k > 1:                                                            # the key of the whole chain serves the level below
            low_pts = np.ascontiguousarray(np.delete(pts[:2], k - 1, axis=2))
            low = _diag(pkg, plans[:-1], sp, d_keys, gs, k, _dev(low_pts), 2, _dev(ct[:-1]))
            assert np.array_equal(low, LN.diag_sum(mods[:-1], P, keys, gs, low_pts, ct[:-1])), gs
    assert np.array_equal(_u64(d_ct), ct)                                    # the input is only read


def test_diag_sum_over_several_chunks_and_past_the_grid_cap(pkg):
    n, k, batch, spec = LN.BIG_CASE
    mods, P = E.case_chain(n, k, spec)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    gs = LN.big_elements(n)
    ct = E.case_ct(mods, n, batch, 2, 77)
    keys, pts = LN.random_keys(mods, P, n, gs, 78), LN.random_pts(mods, P, n, 1, len(gs), 79)
    d_keys = _keys_dev(keys)
    assert np.array_equal(_diag(pkg, plans, sp, d_keys, gs, k, _dev(pts), 1, _dev(ct)), LN.diag_sum(mods, P, keys, gs, pts, ct))
    low_pts = np.ascontiguousarray(np.delete(pts, k - 1, axis=2))
    low = _diag(pkg, plans[:-1], sp, d_keys, gs, k, _dev(low_pts), 1, _dev(ct[:-1]))
    assert np.array_equal(low, LN.diag_sum(mods[:-1], P, keys, gs, low_pts, ct[:-1]))


# ---- anchors to existing entry points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch", [(2, 1, 1), (16, 3, 3), (64, 2, 3), (16, 8, 3)])
def test_anchors_to_existing_entry_points(pkg, n, k, batch):
    B = pkg.binding
    mods, P = E.case_chain(n, k, "wide" if k == 8 else (58, 40))
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    ct = E.case_ct(mods, n, batch, 2, 23 * n + k)
    d_ct = _dev(ct)
    one = np.ones((1, 1, k + 1, n), dtype=U64)
    for g in (2 * n - 1, 5 % (2 * n)):
        if g == 1:
            continue
        d_gk = _dev(LN.random_keys(mods, P, n, [g], 5)[0])
        rot = _empty((1, k, 2, batch, n))
        B.ckks_rns_galois_dev(plans, sp, [d_gk.data_ptr()], [g], k, d_ct.data_ptr(), rot.data_ptr(), batch)
        assert np.array_equal(_diag(pkg, plans, sp, [d_gk], [g], k, _dev(one), 1, d_ct), _u64(rot)), g   # m = 1: the rotation itself
    # every g = 1: the plain products, per limb and component, no key anywhere
    pts = LN.random_pts(mods, P, n, 2, 3, 6)
    d_pts = _dev(pts)
    want = np.zeros((2,) + ct.shape, dtype=U64)
    tmp = _empty((batch, n))
    for o in range(2):
        for i, p in enumerate(plans):
            for c in range(2):
                for r in range(3):
                    for b in range(batch):
                        p.pointwise_mul_dev(d_ct[i, c, b].data_ptr(), d_pts[o, r, i].data_ptr(), tmp[b].data_ptr(), 1)
                    want[o, i, c] = E.padd(mods[i], want[o, i, c], _u64(tmp))
    B_got = _empty((2,) + ct.shape)
    B.ckks_rns_diag_sum_dev(plans, sp, None, [1, 1, 1], k, d_pts.data_ptr(), 2, d_ct.data_ptr(), B_got.data_ptr(), batch)
    assert np.array_equal(_u64(B_got), want)
    # outputs = 2 equals two outputs = 1 calls
    gs = [1, 5 % (2 * n), 2 * n - 1]
    d_keys = _keys_dev(LN.random_keys(mods, P, n, gs, 8))
    both = _diag(pkg, plans, sp, d_keys, gs, k, d_pts, 2, d_ct)
    for o in range(2):
        assert np.array_equal(both[o], _diag(pkg, plans, sp, d_keys, gs, k, _dev(pts[o:o + 1]), 1, d_ct)[0])


def test_edge_residues_at_the_largest_count(pkg):
    """words 0, 1, q - 1, floor(q/2), floor(q/2) + 1 in every limb, P included, in the plaintexts, the keys and the ciphertext, with
    256 elements on the chain whose first limb and special prime are >= 2^62: the fold rule's worst case is q - 1 everywhere"""
    n, k, batch = 16, 8, 2
    mods, P = E.wide_chain(n)
    assert mods[0] >= 1 << 62 and P >= 1 << 62
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    count = G.MAX_COUNT
    gs = [1 if r % 7 == 3 else (5, 2 * n - 1, 25)[r % 3] for r in range(count)]

    def edge(q, shape, shift):
        vals = np.array([q - 1, q - 1, 0, 1, q // 2, q // 2 + 1, q - 1, q - 1], dtype=U64)
        return vals[(np.arange(int(np.prod(shape))) + shift) % len(vals)].reshape(shape)
    allm = list(mods) + [P]
    ct = np.stack([edge(q, (2, batch, n), i) for i, q in enumerate(mods)])
    ct[:, :, 0] = np.stack([np.full((2, n), q - 1, dtype=U64) for q in mods])            # one ciphertext of q - 1 throughout
    key = np.stack([np.stack([edge(q, (2, n), j) for q in allm]) for j in range(k)])
    full = np.stack([np.stack([np.full((2, n), q - 1, dtype=U64) for q in allm]) for j in range(k)])
    keys = [None if g == 1 else (full if r % 2 else key) for r, g in enumerate(gs)]
    pts = np.stack([np.stack([edge(q, (n,), r) if r % 3 else np.full(n, q - 1, dtype=U64) for q in allm]) for r in range(count)])[None]
    d_key, d_full = _dev(key), _dev(full)
    d_keys = [None if x is None else (d_full if x is full else d_key) for x in keys]
    got = _diag(pkg, plans, sp, d_keys, gs, k, _dev(pts), 1, _dev(ct))
    assert np.array_equal(got, LN.diag_sum(mods, P, keys, gs, pts, ct))


# ---- the launch counts of §24 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_launch_counts(pkg, k):
    import torch

    B = pkg.binding
    n, batch = 64, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    a = _dev(E.case_ct(mods, n, batch, 2, 9))
    R = LN.GROUP + 1
    gs = [5, 25, 2 * n - 1] * 6
    keys = [_dev(np.random.default_rng(10 + r).integers(0, 1 << 39, (k, k + 1, 2, n), dtype=np.uint64)) for r in range(3)] * 6
    d_pts = _dev(np.random.default_rng(3).integers(0, 1 << 39, (3, R, k + 1, n), dtype=np.uint64))
    out = _empty((3, k, 2, batch, n))
    labels = ("tensor", "lift", "keymac", "divround", "galois", "diagmac")

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

    def ptrs(c):
        return [x.data_ptr() for x in keys[:c]]
    for count in (1, 3, LN.GROUP, R):
        for outputs in (1, 2, 3):
            pt = d_pts[:outputs, :count].contiguous()
            got = counts(lambda: B.ckks_rns_diag_sum_dev(plans, sp, ptrs(count), gs[:count], k, pt.data_ptr(), outputs, a.data_ptr(), out.data_ptr(), batch))
            assert got == dict(LN.launch_counts(k, count, outputs, 1), tensor=0, galois=0), (k, count, outputs)
    pt = d_pts[:3, :R].contiguous()
    got = counts(lambda: B.ckks_rns_diag_sum_dev(plans, sp, None, [1] * R, k, pt.data_ptr(), 3, a.data_ptr(), out.data_ptr(), batch))
    assert got == dict(LN.launch_counts(k, R, 3, 1, switched=False), tensor=0, galois=0)   # the identity alone: no digit, transform or modulus-down
    # §22's and §23's counts are as they were
    got = counts(lambda: B.ckks_rns_mul_dev(plans, sp, keys[0].data_ptr(), k, a.data_ptr(), a.data_ptr(), out[0].data_ptr(), batch))
    assert got == dict(tensor=k, lift=k + 1, keymac=k + 1, divround=k, galois=0, diagmac=0)
    got = counts(lambda: B.ckks_rns_galois_dev(plans, sp, ptrs(3), gs[:3], k, a.data_ptr(), out.data_ptr(), batch))
    assert got == dict(tensor=0, lift=k + 3, keymac=3 * (k + 1), divround=3 * k, galois=0, diagmac=0)


# ---- the functional case and the Python surface --------------------------------------------------------------------------------------------
def _pt_coeffs(P, n, d_pts):
    """the centred integer coefficients of the plaintexts, from their limb under P, and the check that every chain limb holds
    the residues of the same polynomial"""
    pts = _u64(d_pts)
    coef = K.centre(E.inv(P, n, pts[..., -1, :]), P)
    return pts, coef


def _functional(pkg, tab, case, M, n1, terms, restate):
    ck = pkg.ckks
    n = case["n"]
    mods, P = E.chain(n, case["b0"], case["bd"], case["L"])
    k = len(mods)
    delta, dpt = LN.functional_scales(n, mods, case["bd"], terms)
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(case["seed"], param, delta)
    z = E.functional_slots(case, 1)
    w = G.to_rotation_order(z)
    ct = key.encrypt(key.public_key(0), K.encode(z, delta))
    lt = ck.LinearTransform.from_matrix(param, key.encoder, M, k - 1, dpt, n1)
    bn1, baby, giant, rows = LN.bsgs_diagonals(M, n1)
    assert (lt.n1, lt.baby, lt.giant) == (bn1, baby, giant) and lt.required_steps() == LN.required_steps(bn1, baby, giant)
    assert lt.level == k - 1 and lt.scale == dpt and lt.pts.gs == [G.galois_element(n, i) for i in baby]
    keys = {st: key.rotation_key(st, slot) for slot, st in enumerate(lt.required_steps())}
    pts, coef = _pt_coeffs(P, n, lt.pts.d_pts)
    for i, q in enumerate(mods):                                             # every limb holds the residues of one polynomial
        assert np.array_equal(pts[..., i, :], E.fwd(q, n, E.residues(coef, q)))
    res = ct.linear_transform(lt, keys)
    assert res.level == k - 1 and res.scale == delta * dpt and res.batch == ct.batch
    if restate:                                                              # the words: one diagonal sum, then the giant steps' rotations
        s = K.secret_key(case["seed"], 0, n)
        gks = [None if i == 0 else G.galois_key(case["seed"], G.GK_BASE + 64 * lt.required_steps().index(i), s, mods, P, tab, G.galois_element(n, i)) for i in baby]
        inner = LN.diag_sum(mods, P, gks, lt.pts.gs, pts, _u64(ct.d))
        got_inner = ct.diag_sum(lt.pts, [keys[i] if i else None for i in baby])
        acc = None
        for a, j in enumerate(giant):
            assert np.array_equal(_u64(got_inner[a].d), inner[a])
            part = inner[a]
            if j:
                g = G.galois_element(n, bn1 * j)
                gk = G.galois_key(case["seed"], G.GK_BASE + 64 * lt.required_steps().index(bn1 * j), s, mods, P, tab, g)
                part = G.apply_galois(mods, P, gk, part, g)
            acc = part if acc is None else G.ct_add(mods, acc, part)
        assert np.array_equal(_u64(res.d), acc)
    out = res.rescale()
    assert out.level == k - 2 and out.scale == delta * dpt / mods[-1] == delta
    d = key.decrypt(out)
    got = G.to_rotation_order(key.decrypt_and_decode(out))
    want = w @ M.T
    norm1 = [[float(np.abs(coef[a, b]).sum()) for b in range(len(baby))] for a in range(len(giant))]
    rmax = [[float(np.abs(rows[a, b]).max()) for b in range(len(baby))] for a in range(len(giant))]
    bound = LN.functional_bound(n, k, delta, dpt, mods[-1], baby, giant, norm1, rmax) + float(K.e_dec(d, delta).max())
    err = float(np.abs(got - want).max())
    print(f"n={n}: Delta = 2^{int(np.log2(delta))}, {len(baby)} baby x {len(giant)} giant steps, worst slot error {err:.3e}, derived bound {bound:.3e}")
    return err, bound, got, want


@pytest.mark.parametrize("name", list(LN.FUNCTIONAL))
def test_dense_matrix_through_the_client_key(pkg, tab, name):
    case = LN.FUNCTIONAL[name]
    N = case["n"] // 2
    M = LN.matrices(N, case["rng"])["dense"]
    err, bound, got, want = _functional(pkg, tab, case, M, None, N, True)
    assert err <= bound and err < 0.5
    assert np.array_equal(np.round(got.real), want.real) and np.array_equal(np.round(got.imag), want.imag)


def test_banded_matrix_at_4096(pkg, tab):
    case = dict(E.FUNCTIONAL_GPU["n4096"], seed=bytes((b + 53) % 256 for b in E.FUNCTIONAL_GPU["n4096"]["seed"]))
    M = LN.matrices(case["n"] // 2, case["rng"])["banded"]
    err, bound, got, want = _functional(pkg, tab, case, M, 2, 5, False)
    # the worst-case bound passes 1/2 here, as §22's and §23's do at this size: it charges every coefficient its maximum
    assert err <= bound and err < 0.5
    assert np.array_equal(np.round(got.real), want.real) and np.array_equal(np.round(got.imag), want.imag)


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
    assert lt.required_steps() == [1, 2, 14] and (lt.baby, lt.giant) == ([0, 1], [0, 1, 7])
    keys = {st: key.rotation_key(st, st) for st in (1, 2)}
    with pytest.raises(KeyError, match="14"):
        ct.linear_transform(lt, keys)
    keys[14] = key.rotation_key(14, 14)
    res = ct.linear_transform(lt, keys)
    assert res.level == 2 and res.scale == 2.0 ** 50 and res.batch == ct.batch
    # plaintext sets: shapes, elements, scale and level bookkeeping, with and without a client key
    rows = np.ones((2, 3, n // 2), dtype=np.complex128)
    pts = key.encode_diagonals(rows, [0, 1, 2], 1, 2.0 ** 20)
    free = ck.encode_diagonals(param, key.encoder, rows, [0, 1, 2], 1, 2.0 ** 20)
    assert pts.outputs == 2 and pts.gs == [1, 5, 25] and pts.level == 1 and pts.scale == 2.0 ** 20 and tuple(pts.d_pts.shape) == (2, 3, 3, n)
    assert np.array_equal(_u64(pts.d_pts), _u64(free.d_pts))
    low = ct.at_level(1)
    outs = low.diag_sum(pts, [None, keys[1], keys[2]])
    assert len(outs) == 2 and all(o.level == 1 and o.scale == 2.0 ** 50 for o in outs)
    assert np.array_equal(_u64(outs[0].d), _u64(outs[1].d))                  # the two outputs have the same plaintexts
    with _refused():
        ct.diag_sum(pts, [None, keys[1], keys[2]])                           # the plaintexts are at another level
    other = ck.RnsParam(n, mods[:2], P)
    with _refused():
        low.diag_sum(ck.RnsPlaintextSet(other, 1, pts.d_pts, 1.0, pts.gs), [None, keys[1], keys[2]])
    with _refused():
        low.diag_sum(pts, [None, ck.RnsGaloisKey(other, 5, keys[1].d_gk), keys[2]])
    with pytest.raises(ValueError):
        low.diag_sum(pts, [None, keys[2], keys[1]])                          # keys of other elements
    with pytest.raises(ValueError):
        low.diag_sum(pts, [None, None, keys[2]])
    with pytest.raises(ValueError):
        low.diag_sum(pts, [None, keys[1]])
    with pytest.raises(ValueError):
        ck.RnsPlaintextSet(param, 1, pts.d_pts, 1.0, [1, 4, 25])
    with pytest.raises(ValueError):
        key.encode_diagonals(rows, [0, 1], 1, 2.0 ** 20)
    with pytest.raises(ValueError):
        key.encode_diagonals(rows, [0, 1, 2], 3, 2.0 ** 20)
    with pytest.raises(ValueError):
        ck.LinearTransform.from_matrix(param, key.encoder, np.eye(4), 2, 2.0 ** 20)


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_outputs_untouched(pkg):
    B = pkg.binding
    n, k = 16, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    a = _dev(E.case_ct(mods, n, 2, 2, 5))
    key = _dev(E.case_ct(mods, n, 4, 2, 7))
    pts = _dev(LN.random_pts(mods, P, n, 2, 2, 9))
    o2 = _empty((2, k, 2, 2, n))
    A, R, PT, O2 = (x.data_ptr() for x in (a, key, pts, o2))
    ct_bytes, pt_bytes = k * 2 * 2 * n * 8, 2 * 2 * (k + 1) * n * 8
    f = B.ckks_rns_diag_sum_dev
    bad = [
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 4], k, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R, R], [0, 5], k, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 2 * n], k, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 2 * n + 1], k, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R] * 257, [5] * 257, k, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 25], k, PT, 0, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 25], k, PT, B.FHE_CKKS_DIAG_MAX_OUTPUTS + 1, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 25], k - 1, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 25], 9, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 25], k, PT, 2, O2 + ct_bytes, O2, 2)),             # the input inside the second output
        (B.FHE_E_INVALID, (plans, sp, [R, O2 + 2 * ct_bytes - 8], [5, 25], k, PT, 2, A, O2, 2)),     # the second key at the output's last word
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 25], k, O2 + 2 * ct_bytes - 8, 2, A, O2, 2)),      # the plaintexts at the output's last word
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 25], k, O2 - pt_bytes + 8, 2, A, O2, 2)),          # ... ending in its first
        (B.FHE_E_INVALID, (plans, sp, [R, R], [5, 25], k, PT + 4, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, plans[0], [R, R], [5, 25], k, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, (plans, pkg.Plan(65537, n), [R, R], [5, 25], k, PT, 2, A, O2, 2)),
        (B.FHE_E_INVALID, ([plans[0], plans[1], plans[0]], sp, [R, R], [5, 25], k, PT, 2, A, O2, 2)),
        (B.FHE_E_PARAM_MISMATCH, ([plans[0], plans[1], other], sp, [R, R], [5, 25], k, PT, 2, A, O2, 2)),
        (B.FHE_E_NULL, (plans, sp, [R, None], [5, 25], k, PT, 2, A, O2, 2)),                         # an element other than 1 needs its key
        (B.FHE_E_NULL, (plans, sp, None, [1, 25], k, PT, 2, A, O2, 2)),
        (B.FHE_E_NULL, (plans, sp, [R, R], [5, 25], k, None, 2, A, O2, 2)),
        (B.FHE_E_NULL, (plans, sp, [R, R], [5, 25], k, PT, 2, None, O2, 2)),
        (B.FHE_E_NULL, (plans, None, [R, R], [5, 25], k, PT, 2, A, O2, 2)),
    ]
    for code, args in bad:
        with _refused() as e:
            f(*args)
        assert e.value.code == code, args
    f(plans, sp, [R, R], [5, 25], k, PT, 2, A, O2, 0)                        # batch = 0 and count = 0 write nothing
    f(plans, sp, [], [], k, PT, 2, A, O2, 2)
    assert (_u64(o2) == U64(FILL)).all()
    # the identity's key entry is not read: NULL, or a pointer inside the output
    f(plans, sp, [None, R], [1, 5], k, PT, 2, A, O2, 2)
    want = _u64(o2).copy()
    f(plans, sp, [O2 + 8, R], [1, 5], k, PT, 2, A, O2, 2)
    assert np.array_equal(_u64(o2), want) and not (want == U64(FILL)).any()
