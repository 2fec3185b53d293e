"""The plaintext linear transforms of the CKKS evaluator without a device: the restated diagonal sum against the
exact product after decryption and against the composition of §23's rotations and §22's plaintext products, within
linear_noise; its word-for-word anchors; the baby-step giant-step bookkeeping against M @ w; the proofs of the GPU module's
case list; the rejections that need no device; the Python surface that needs none."""
import numpy as np
import pytest

import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_linear_numpy as LN
import _ckks_numpy as K
import _client_numpy as C

U64, I64 = np.uint64, np.int64


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _centred(x, Q):
    x = x % Q
    return np.where(x > Q // 2, x - Q, x)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 16, 64])
@pytest.mark.parametrize("k", [2, 3])
def test_restatement_is_the_sum_of_rotated_products_after_decryption(tab, n, k):
    """Worst case the composition's own noise, sum_r |m_r|_1 relin_noise, adds to linear_noise; both measured errors are a small
    fraction of their bounds (printed), so their difference stays within linear_noise alone, which is what is asserted."""
    mods, P = E.chain(n, 58, 40, k - 1)
    s = K.secret_key(LN.SEED, 0, n)
    pk = E.public_key(LN.SEED, E.PK_BASE, s, mods, tab)
    rng = np.random.default_rng(n + k)
    msg = rng.integers(-(1 << 30), 1 << 30, (2, n), dtype=np.int64)
    ct = E.encrypt(LN.SEED, 0, pk, msg, 2, mods, tab)
    gs = [1, 5 % (2 * n), 2 * n - 1, 5 % (2 * n)]
    gks = [None if g == 1 else G.galois_key(LN.SEED, G.GK_BASE + 64 * r, s, mods, P, tab, g) for r, g in enumerate(gs)]
    m = rng.integers(-64, 65, (2, len(gs), n), dtype=np.int64)              # two outputs
    pts = LN.plaintext_evals(mods, P, m)
    out = LN.diag_sum(mods, P, gks, gs, pts, ct)
    before, Q = E.phase_int(mods, n, s, ct)
    for o in range(2):
        after, _ = E.phase_int(mods, n, s, out[o])
        exact = sum(E.negacyclic_int(G.galois_int(before, g), m[o, r]) for r, g in enumerate(gs))
        bound = LN.linear_noise(n, k, [int(np.abs(m[o, r]).sum()) for r, g in enumerate(gs) if g != 1])
        worst = int(np.abs(_centred(after - exact, Q)).max())
        comp = None
        for r, g in enumerate(gs):
            part = E.mul_plain(mods, n, ct if g == 1 else G.apply_galois(mods, P, gks[r], ct, g), m[o, r])
            comp = part if comp is None else G.ct_add(mods, comp, part)
        composed, _ = E.phase_int(mods, n, s, comp)
        apart = int(np.abs(_centred(after - composed, Q)).max())
        print(f"n={n} k={k} output {o}: |dec(out) - exact|_inf = {worst}, against the composition {apart}, linear_noise {bound}")
        assert worst <= bound and apart <= bound


def test_restatement_word_for_word_anchors():
    for n, k in ((16, 3), (64, 2), (4, 1)):
        mods, P = E.chain(n, 58, 40, k - 1)
        ct = E.case_ct(mods, n, 2, 2, 3 * n + k)
        one = np.ones((1, 1, k + 1, n), dtype=U64)
        for g in G.case_elements(n):
            gk = LN.random_keys(mods, P, n, [5], n + g)[0]                  # any words: g = 1 switches through a key in §23, here it takes none
            want = ct[None] if g == 1 else G.apply_galois(mods, P, gk, ct, g)[None]
            assert np.array_equal(LN.diag_sum(mods, P, [gk], [g], one, ct), want), (n, k, g)
        # every element the identity: the plain products, summed
        pts = LN.random_pts(mods, P, n, 2, 3, 7)
        got = LN.diag_sum(mods, P, [None] * 3, [1, 1, 1], pts, ct)
        for o in range(2):
            for i, q in enumerate(mods):
                tot = sum(pts[o, r, i].astype(object) for r in range(3)) % q
                assert np.array_equal(got[o, i], E.pmul(q, ct[i], tot.astype(U64)))
        # the sum does not depend on the order of the elements, and the outputs are independent
        gs = [1, 5 % (2 * n), 2 * n - 1]
        keys = LN.random_keys(mods, P, n, gs, 9)
        a = LN.diag_sum(mods, P, keys, gs, pts, ct)
        b = LN.diag_sum(mods, P, keys[::-1], gs[::-1], np.ascontiguousarray(pts[:, ::-1]), ct)
        assert np.array_equal(a, b) and np.array_equal(a[1:], LN.diag_sum(mods, P, keys, gs, pts[1:], ct))
    with pytest.raises(ValueError):
        LN.diag_sum(mods, P, [None], [4], np.ones((1, 1, k + 1, n), dtype=U64), ct)


# ---- baby-step giant-step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 32])
def test_bsgs_bookkeeping_is_the_matrix_product(pkg, N):
    ck = pkg.ckks
    rng = np.random.default_rng(N)
    w = rng.integers(-8, 8, (3, N)) + 1j * rng.integers(-8, 8, (3, N))
    for name, M in LN.matrices(N, 100 + N).items():
        kept = len([t for t in range(N) if np.any(M[np.arange(N), (np.arange(N) + t) % N] != 0)])
        assert kept == {"dense": N, "banded": 5, "single": 1}[name]
        for n1 in [None] + list(range(1, N + 1)):                           # every n1, dividing the diagonal count or not
            got = ck.bsgs_diagonals(M, n1)
            ref = LN.bsgs_diagonals(M, n1)
            assert got[:3] == ref[:3] and np.array_equal(got[3], ref[3]), (name, n1)
            n1_, baby, giant, rows = got
            assert len(baby) <= n1_ and all(0 <= i < n1_ for i in baby) and all(n1_ * j < N for j in giant)
            assert np.count_nonzero(np.abs(rows).sum(axis=-1)) == kept       # only the non-zero diagonals are kept
            assert np.abs(LN.bsgs_apply(n1_, baby, giant, rows, w) - w @ M.T).max() < 1e-9, (name, n1)
            steps = LN.required_steps(n1_, baby, giant)
            assert 0 not in steps and all(0 < st < N for st in steps)
    assert ck.bsgs_diagonals(np.zeros((N, N)))[1:3] == ([0], [0])             # the zero matrix keeps its (zero) main diagonal
    with pytest.raises(ValueError):
        ck.bsgs_diagonals(np.zeros((N, N + 1)))
    with pytest.raises(ValueError):
        ck.bsgs_diagonals(np.eye(N), 0)


# ---- the GPU module's case list ------------------------------------------------------------------------------------------------------------
def test_case_list_covers_every_path(pkg):
    B = pkg.binding
    cases = {(n, k, b) for n, k, b, _ in LN.WORD_CASES}
    assert cases >= {(2, 1, 1), (16, 8, 3)} | {(n, k, b) for n in (4, 16, 64) for k in (1, 2, 3) for b in (1, 3)}
    assert LN.BIG_CASE == (4096, 2, 257, (58, 40)) and len(LN.big_elements(4096)) == 3
    # the new kernel's launches: within the grid cap, and past it (a second grid-stride pass)
    counts = set()
    for n, k, b, _ in LN.WORD_CASES + [LN.BIG_CASE]:
        counts |= LN.launch_elements(n, k, b)
    print(f"diagmac: launches of {min(counts)} .. {max(counts)} elements")
    assert min(counts) < E.GRID_CAP < max(counts)
    # more than one chunk: (4096, 2, 257) runs in 128 + 128 + 1, and in one chunk of 257 at one limb, past the cap
    assert E.chunk_rows(4096, 2, 257) == 128 and E.chunk_rows(4096, 1, 257) == 257 and 257 * 4096 > E.GRID_CAP
    # a limb >= 2^62 (the accumulators' other fold), the special prime too, at k = 8
    wide, wp = E.wide_chain(16)
    assert any(spec == "wide" and k == 8 for _, k, _, spec in LN.WORD_CASES) and wide[0] >= 1 << 62 and wp >= 1 << 62
    # count on both sides of the by-value group, outputs on both sides of the in-register cap; the identity alone, with others, a repeat
    for n in {n for n, _, _, _ in LN.WORD_CASES}:
        lists = LN.element_lists(n)
        assert all(g % 2 == 1 and 0 < g < 2 * n for gs in lists for g in gs)
        assert min(len(gs) for gs in lists) == 1 and max(len(gs) for gs in lists) == LN.GROUP + 1
        assert [1] in lists and any(1 in gs and any(g != 1 for g in gs) for gs in lists)
        assert any(len(set(gs)) < len(gs) for gs in lists)
        assert n < 4 or (lists[-1][LN.GROUP] != 1 and 1 in lists[-1][:LN.GROUP])     # the second group switches a key too
    assert min(LN.OUTPUTS) <= LN.OUT_CAP < max(LN.OUTPUTS) and 2 in LN.OUTPUTS
    assert G.MAX_COUNT == B.FHE_CKKS_GALOIS_MAX_COUNT == 256 and G.MAX_COUNT > LN.GROUP and B.FHE_CKKS_DIAG_MAX_OUTPUTS == LN.MAX_OUTPUTS
    # the workspace: count does not enter, the outputs up to the cap do; §22's and §23's values are as they were
    for n, k, b, count, outputs in ((4096, 2, 257, 1, 1), (4096, 2, 257, 256, 1), (4096, 2, 257, 3, 2), (4096, 2, 257, 3, 64), (16, 8, 3, 17, 3), (2, 1, 1, 1, 1)):
        assert B.ckks_rns_diag_workspace_bytes(n, k, b, count, outputs) == LN.workspace_bytes(n, k, b, outputs)
    for args in ((4096, 2, 257, 0, 1), (4096, 2, 257, 257, 1), (4096, 2, 257, 1, 0), (4096, 2, 257, 1, 65), (12, 2, 1, 1, 1), (16, 9, 1, 1, 1), (16, 2, 0, 1, 1)):
        assert B.ckks_rns_diag_workspace_bytes(*args) == 0
    assert B.ckks_rns_workspace_bytes(4096, 2, 257) == (4 + 16 + 2) * 128 * 4096 * 8
    assert B.ckks_rns_galois_workspace_bytes(4096, 2, 257, 8) == G.workspace_bytes(4096, 2, 257)
    # §24's launch formula
    assert LN.launch_counts(3, 17, 3, 2) == dict(lift=2 * 6, diagmac=2 * 2 * 2 * 4, keymac=0, divround=2 * 9)
    assert LN.launch_counts(3, 17, 3, 2, switched=False) == dict(lift=0, diagmac=2 * 2 * 2 * 3, keymac=0, divround=0)


# ---- rejections that need no device ----------------------------------------------------------------------------------------------------------
def test_rejections_without_a_device(pkg):
    B = pkg.binding
    n = 16
    mods, P = E.chain(n, 58, 40, 2)
    plans, sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    buf, key, pt, out = 0x10000, 0x40000, 0x80000, 0x400000

    def code(*a, **kw):
        with pytest.raises(B.FheError) as e:
            B.ckks_rns_diag_sum_dev(*a, **kw)
        return e.value.code

    for g in (4, 0, 2 * n, 2 * n + 1, 1 << 40):
        assert code(plans, sp, [key], [g], 3, pt, 1, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key, key], [5, 2 * n], 3, pt, 1, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key] * 257, [5] * 257, 3, pt, 1, buf, out, 1) == B.FHE_E_INVALID         # count above the cap
    assert code(plans, sp, [key], [5], 3, pt, 0, buf, out, 1) == B.FHE_E_INVALID                     # outputs = 0, and above its cap
    assert code(plans, sp, [key], [5], 3, pt, B.FHE_CKKS_DIAG_MAX_OUTPUTS + 1, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key], [5], 2, pt, 1, buf, out, 1) == B.FHE_E_INVALID                     # key_limbs < limbs
    assert code(plans, sp, [key], [5], 9, pt, 1, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key], [5], 3, pt, 1, out, out, 1) == B.FHE_E_INVALID                     # the output overlaps the input
    assert code(plans, sp, [key], [5], 3, pt, 1, buf, key, 1) == B.FHE_E_INVALID                     # ... a key
    assert code(plans, sp, [key], [5], 3, out + 8, 1, buf, out, 1) == B.FHE_E_INVALID                # ... the plaintexts
    assert code(plans, sp, [key, out + 8 * 2 * 3 * n * 2 - 8], [5, 25], 3, pt, 2, buf, out, 1) == B.FHE_E_INVALID   # the second key in the second output
    assert code(plans, sp, [key], [5], 3, pt + 4, 1, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key, None], [5, 25], 3, pt, 1, buf, out, 1) == B.FHE_E_NULL              # g != 1 needs its key
    assert code(plans, sp, None, [5], 3, pt, 1, buf, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, [key], None, 3, pt, 1, buf, out, 1, count=1) == B.FHE_E_NULL
    assert code(plans, sp, [key], [5], 3, None, 1, buf, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, [key], [5], 3, pt, 1, None, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, [key], [5], 3, pt, 1, buf, None, 1) == B.FHE_E_NULL
    assert code(plans, None, [key], [5], 3, pt, 1, buf, out, 1) == B.FHE_E_NULL
    assert code([plans[0], other], sp, [key], [5], 3, pt, 1, buf, out, 1) == B.FHE_E_PARAM_MISMATCH
    assert code(plans, plans[0], [key], [5], 3, pt, 1, buf, out, 1) == B.FHE_E_INVALID
    # the identity's key is not looked at: an entry inside the output is no overlap, and the next element's rejection is reached
    assert code(plans, sp, [out, key], [1, 4], 3, pt, 1, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [None, None], [1, 5], 3, pt, 1, buf, out, 1) == B.FHE_E_NULL
    # batch = 0 or count = 0 is a no-op, whatever the buffers
    f = B.ckks_rns_diag_sum_dev
    f(plans, sp, None, None, 3, None, 1, None, None, 0, count=0)
    f(plans, sp, [None], [4], 3, None, 1, None, None, 0)
    f(plans, sp, [], [], 3, None, 1, None, None, 5)


# ---- the Python surface that needs no device -----------------------------------------------------------------------------------------------
def test_python_surface_without_a_device(pkg):
    ck = pkg.ckks
    n = 16
    param = ck.RnsParam(n, *E.chain(n, 58, 40, 1))
    assert callable(ck.RnsCiphertext.diag_sum) and callable(ck.RnsCiphertext.linear_transform) and callable(ck.RnsClientKey.encode_diagonals)
    pts = ck.RnsPlaintextSet(param, 1, None, 2.0 ** 20, [1, 5, 25])
    assert pts.gs == [1, 5, 25] and pts.level == 1 and pts.scale == 2.0 ** 20
    for g in (0, 2, 32, 33):
        with pytest.raises(ValueError):
            ck.RnsPlaintextSet(param, 1, None, 1.0, [1, g])
    M = LN.matrices(n // 2, 3)["banded"]
    n1, baby, giant, _ = ck.bsgs_diagonals(M, 2)
    lt = ck.LinearTransform(param, n1, baby, giant, pts)
    assert lt.required_steps() == LN.required_steps(n1, baby, giant) == [1, 2, 6] and lt.level == 1 and lt.scale == 2.0 ** 20
    ct = ck.RnsCiphertext(param, None, 1, 2.0 ** 30)
    with pytest.raises(KeyError, match="2"):
        ct.linear_transform(lt, {1: None, 6: None})                         # the missing step is named before anything runs
