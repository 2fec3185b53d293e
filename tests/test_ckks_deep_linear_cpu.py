"""The plaintext linear transforms on the deep CKKS chain without a device: the restated diagonal sum
(tests/_ckks_deep_linear_numpy.py) at alpha = 1 against §24's restatement word for word; against the exact sum after decryption and
against the composition of §36's rotations and plaintext products, within §37's noise bound, with a real ternary secret and the
table's errors; the boundary; the size query; the rejections the Python classes make before any device call."""
import os
import re

import numpy as np
import pytest

import _ckks_deep_linear_numpy as DL
import _ckks_deep_numpy as D
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_linear_numpy as LN
import _ckks_numpy as K
import _client_numpy as C

U64, I64 = np.uint64, np.int64
SEED = bytes((17 * i + 5) % 256 for i in range(32))


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _centred(x, Q):
    x = x % Q
    return np.where(x > Q // 2, x - Q, x)


# ---- alpha = 1 is §24 word for word -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_alpha_one_is_the_single_digit_restatement(k):
    n = 8
    mods, P = E.chain(n, 58, 40, k - 1)
    ct = E.case_ct(mods, n, 2, 2, 30 + k)
    for t, gs in enumerate(DL.element_lists(n)):
        keys = LN.random_keys(mods, P, n, gs, 50 + t)
        pts = LN.random_pts(mods, P, n, 3, len(gs), 60 + t)
        assert np.array_equal(DL.diag_sum(mods, [P], keys, gs, pts, ct), LN.diag_sum(mods, P, keys, gs, pts, ct)), gs
    assert DL.slabs(k, 1, 2) == k * k + 3 * k + 2 * (k + 1) * 2              # §24's SwitchBufs::words
    with pytest.raises(ValueError):
        DL.diag_sum(mods, [P], [None], [4], np.ones((1, 1, k + 1, n), dtype=U64), ct)


# ---- the definition and the noise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,alpha", [(5, 2), (9, 3)])
def test_restatement_is_the_sum_of_rotated_products_within_the_bound(tab, L, alpha):
    """A real ternary secret, public key, Galois keys and the table's errors at n = 8.  The restated sum against the exact
    sum_r m_r sigma_{g_r}(dec(ct)) is under linear_noise, the composition sum_r m_r (.) apply_galois(ct) under sum_r |m_r|_1
    switch_noise_bound.  Against each other the two differ by their roundings alone: with E_r = sum_j sigma(x_j) e_{r,j} the sum's
    error is (sum_r m_r E_r - y) / P and the composition's sum_r m_r (E_r - y_r) / P, every y a pair y0 + y1 s of centred residues
    modulo P, so the key errors cancel and |difference|_inf <= (n + 1) / 2 (1 + sum_r |m_r|_1).  The measured figures are printed."""
    n = 8
    mods, sps = D.case_chain(n, L, alpha)
    P = D.product(sps)
    s = K.secret_key(SEED, 0, n)
    assert np.abs(s).max() <= 1
    pk = E.public_key(SEED, E.PK_BASE, s, mods, tab)
    rng = np.random.default_rng(10 * L + alpha)
    msg = rng.integers(-(1 << 30), 1 << 30, (2, n), dtype=np.int64)
    ct = E.encrypt(SEED, 0, pk, msg, 2, mods, tab)
    gs = [1, 5, 2 * n - 1, 5]
    gks = [None if g == 1 else D.switch_key(SEED, G.GK_BASE + 64 * r, s, mods, sps, tab, g) for r, g in enumerate(gs)]
    m = rng.integers(-64, 65, (2, len(gs), n), dtype=np.int64)               # two outputs
    pts = DL.plaintext_evals(mods, sps, m)
    assert pts.shape == (2, len(gs), L + alpha, n)
    out = DL.diag_sum(mods, sps, gks, gs, pts, ct)
    before, Q = E.phase_int(mods, n, s, ct)
    ratio = max(D.product(mods[i] for i in g) for g in D.groups(L, alpha)) / P
    assert ratio <= 1
    for o in range(2):
        after, _ = E.phase_int(mods, n, s, out[o])
        exact = sum(E.negacyclic_int(G.galois_int(before, g), m[o, r]) for r, g in enumerate(gs))
        norms = [int(np.abs(m[o, r]).sum()) for r, g in enumerate(gs) if g != 1]
        bound = DL.linear_noise(n, L, alpha, ratio, norms)
        worst = int(np.abs(_centred(after - exact, Q)).max())
        comp = None
        for r, g in enumerate(gs):
            part = E.mul_plain(mods, n, ct if g == 1 else D.apply_galois(mods, sps, gks[r], ct, g), m[o, r])
            comp = part if comp is None else DL.ct_add(mods, comp, part)
        composed, _ = E.phase_int(mods, n, s, comp)
        comp_bound = sum(norms) * D.switch_noise_bound(n, L, alpha, ratio)
        comp_err = int(np.abs(_centred(composed - exact, Q)).max())
        apart = int(np.abs(_centred(after - composed, Q)).max())
        print(f"L={L} alpha={alpha} output {o}: |dec(out) - exact|_inf = {worst} (linear_noise {bound}), the composition's {comp_err} (its bound {comp_bound}), "
              f"apart {apart} (the roundings allow {(n + 1) / 2 * (1 + sum(norms))})")
        assert worst <= bound and comp_err <= comp_bound and apart <= (n + 1) / 2 * (1 + sum(norms))
    # one rounding an output, not one an element: the bound's rounding term does not grow with the count
    assert DL.linear_noise(n, L, alpha, ratio, []) == (n + 1) / 2
    assert DL.linear_noise(n, L, 1, 1.0, [1]) == (n + 1) / 2 + L * n * E.B_ERR / 2 == LN.linear_noise(n, L, [1])   # §24's at alpha = 1, Q_j = P


def test_restatement_anchors():
    n, L, alpha = 8, 5, 2
    mods, sps = D.case_chain(n, L, alpha)
    for l in (5, 4):
        lm = mods[:l]
        ct = E.case_ct(lm, n, 2, 2, 7 + l)
        one = np.ones((1, 1, l + alpha, n), dtype=U64)
        for g in (5, 2 * n - 1, 1):
            gk = DL.random_keys(lm, sps, n, [5], 11 + g, key_mods=mods)[0]   # the key of the whole chain serves the level below
            want = ct[None] if g == 1 else D.apply_galois(lm, sps, gk, ct, g)[None]
            assert np.array_equal(DL.diag_sum(lm, sps, [gk], [g], one, ct), want), (l, g)
        pts = DL.random_pts(lm, sps, n, 2, 3, 7)
        got = DL.diag_sum(lm, sps, [None] * 3, [1, 1, 1], pts, ct)           # every element the identity: the plain products, summed
        for o in range(2):
            for i, q in enumerate(lm):
                tot = sum(pts[o, r, i].astype(object) for r in range(3)) % q
                assert np.array_equal(got[o, i], E.pmul(q, ct[i], tot.astype(U64)))
        gs = [1, 5, 2 * n - 1]
        keys = DL.random_keys(lm, sps, n, gs, 9, key_mods=mods)
        a = DL.diag_sum(lm, sps, keys, gs, pts, ct)
        b = DL.diag_sum(lm, sps, keys[::-1], gs[::-1], np.ascontiguousarray(pts[:, ::-1]), ct)
        assert np.array_equal(a, b) and np.array_equal(a[1:], DL.diag_sum(lm, sps, keys, gs, pts[1:], ct))


# ---- the boundary and the size query ---------------------------------------------------------------------------------------------------------
SIZES = [(8, 5, 2, 3, 3, 1), (8, 5, 2, 3, 3, 2), (8, 5, 2, 3, 17, 3), (8, 32, 8, 1, 1, 64), (8, 32, 1, 5, 256, 2), (8192, 4, 2, 400, 3, 2), (2048, 12, 4, 700, 16, 1),
         (2, 1, 1, 1, 1, 1), (1 << 15, 24, 3, 8, 32, 1)]
REFUSED = [(8, 33, 1, 1, 1, 1), (8, 0, 1, 1, 1, 1), (8, 4, 9, 1, 1, 1), (8, 4, 0, 1, 1, 1), (8, 4, 1, 0, 1, 1), (12, 4, 1, 1, 1, 1), (1, 4, 1, 1, 1, 1),
           (8, 4, 1, 1, 0, 1), (8, 4, 1, 1, 257, 1), (8, 4, 1, 1, 1, 0), (8, 4, 1, 1, 1, 65)]


def test_boundary(pkg):
    from conftest import ROOT

    B = pkg.binding
    h = open(os.path.join(ROOT, "include", "fhe_ntt.h")).read()
    lib = pkg.load_library()
    assert re.search(r"\bint\s+fhe_ckks_deep_diag_sum_dev\(", h) and re.search(r"\bsize_t\s+fhe_ckks_deep_diag_workspace_bytes\(", h)
    for name in ("fhe_ckks_deep_diag_sum_dev", "fhe_ckks_deep_diag_workspace_bytes"):
        assert name in B.EXPORTS and hasattr(lib, name)
    assert (B.FHE_CKKS_GALOIS_MAX_COUNT, B.FHE_CKKS_DIAG_MAX_OUTPUTS) == (DL.MAX_COUNT, DL.MAX_OUTPUTS)


def test_size_query_is_the_restated_formula(pkg):
    """it needs no device"""
    B = pkg.binding
    for n, l, a, b, count, outputs in SIZES:
        assert B.ckks_deep_diag_workspace_bytes(n, l, a, b, count, outputs) == DL.workspace_bytes(n, l, a, b, count, outputs) > 0
    for n, l, a, b, count, outputs in REFUSED:
        assert B.ckks_deep_diag_workspace_bytes(n, l, a, b, count, outputs) == DL.workspace_bytes(n, l, a, b, count, outputs) == 0
    # the slab count as the header states it, and the chunk rule over it
    assert DL.slabs(5, 2, 1) == 5 + (7 * 3 - 5) + 2 * 7 + 10 and DL.slabs(5, 2, 3) == DL.slabs(5, 2, 2) == DL.slabs(5, 2, 1) + 14
    assert DL.chunk_rows(8192, 4, 2, 400, 2) == (1 << 21) // 8192 // DL.slabs(4, 2, 2) == 5
    assert DL.launch_counts(5, 2, 17, 3) == dict(extend=3 + 3, diagmac=7 * 2 * 2, keymac=0, divround=15)
    assert DL.launch_counts(5, 2, 17, 3, switched=False) == dict(extend=0, diagmac=5 * 2 * 2, keymac=0, divround=0)


# ---- the Python classes' own rejections, made before any device call ---------------------------------------------------------------------------
def test_python_side_rejections(pkg):
    import torch

    ck = pkg.ckks
    B = pkg.binding
    n, L, alpha = 8, 5, 2
    mods, sps = D.case_chain(n, L, alpha)
    param = ck.DeepParam(n, mods, sps)
    other = ck.DeepParam(n, mods[:4], sps)
    gs = [1, 5, 2 * n - 1]
    level = 3

    def pts_of(limbs, lvl=level, p=param, kind=ck.DeepPlaintextSet, els=gs):
        return kind(p, lvl, torch.zeros((2, len(els), limbs, n), dtype=torch.int64), 2.0 ** 20, els)
    pts = pts_of(level + 1 + alpha)
    assert pts.outputs == 2 and isinstance(pts, ck.RnsPlaintextSet)
    for limbs in (level + 2, level + alpha, level + 2 + alpha):              # the deep set asks the param for its special count
        with pytest.raises(ValueError, match=r"level \+ 1 \+ alpha"):
            pts_of(limbs)
    with pytest.raises(ValueError):
        ck.DeepPlaintextSet(param, level, torch.zeros((2, 2, level + 1 + alpha, n), dtype=torch.int64), 1.0, gs)   # count is not len(gs)
    with pytest.raises(ValueError):
        pts_of(level + 1 + alpha, els=[1, 4, 5])
    rp = ck.RnsParam(n, mods, sps[0])                                        # RnsPlaintextSet's own check is as it was
    with pytest.raises(ValueError, match=r"level \+ 2"):
        pts_of(level + 1 + alpha, p=rp, kind=ck.RnsPlaintextSet)
    assert pts_of(level + 2, p=rp, kind=ck.RnsPlaintextSet).outputs == 2
    ct = ck.DeepCiphertext(param, torch.zeros((level + 1, 2, 1, n), dtype=torch.int64), level, 2.0 ** 30)
    keys = [None, ck.RnsGaloisKey(param, 5, None), ck.RnsGaloisKey(param, 2 * n - 1, None)]
    with pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ") as e:                                     # the level
        ct.diag_sum(pts_of(level + alpha, lvl=level - 1), keys)
    assert e.value.code == B.FHE_E_PARAM_MISMATCH
    with pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ") as e:                                     # another chain's plaintexts, another chain's key
        ct.diag_sum(pts_of(level + 1 + alpha, p=other), keys)
    assert e.value.code == B.FHE_E_PARAM_MISMATCH
    with pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ") as e:
        ct.diag_sum(pts, keys[:2] + [ck.RnsGaloisKey(other, 2 * n - 1, None)])
    assert e.value.code == B.FHE_E_PARAM_MISMATCH
    with pytest.raises(ValueError, match="is of g=5"):                       # the key of another element
        ct.diag_sum(pts, [None, keys[1], keys[1]])
    with pytest.raises(ValueError, match="has no key"):                      # a missing key
        ct.diag_sum(pts, [None, None, keys[2]])
    with pytest.raises(ValueError, match="2 keys for 3"):
        ct.diag_sum(pts, keys[:2])
    with pytest.raises(ValueError, match="DeepPlaintextSet"):                # a plain RnsPlaintextSet on the deep param
        ct.diag_sum(ck.RnsPlaintextSet(param, level, torch.zeros((2, 3, level + 2, n), dtype=torch.int64), 1.0, gs), keys)
    # what stays with §36: the rest of _not_yet
    for name in ("linear_transform_hoisted", "mul_const", "add_const", "eval_chebyshev"):
        with pytest.raises(NotImplementedError):
            getattr(ct, name)(1.0)
    assert ck.DeepCiphertext.linear_transform is ck.RnsCiphertext.linear_transform
    assert ck.DeepClientKey.encode_diagonals is ck.RnsClientKey.encode_diagonals
