"""The baby-step giant-step linear transform with hoisted giant steps without a device: the restatement against the
exact product after decryption within bsgs_noise and against the restated composition (RnsCiphertext.linear_transform) within
the sum of the two bounds; its word-for-word anchors; the fold order of the accumulate kernel replayed at words q - 1; the
proofs of the GPU module's case list; the rejections and the surface that need no device."""
import numpy as np
import pytest

import _ckks_bsgs_numpy as BN
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
def test_restatement_is_the_exact_product_after_decryption(tab, n, k):
    mods, P = E.chain(n, 58, 40, k - 1)
    s = K.secret_key(BN.SEED, 0, n)
    pk = E.public_key(BN.SEED, E.PK_BASE, s, mods, tab)
    rng = np.random.default_rng(7 * n + k)
    msg = rng.integers(-(1 << 30), 1 << 30, (2, n), dtype=np.int64)
    ct = E.encrypt(BN.SEED, 0, pk, msg, 2, mods, tab)
    baby_gs, giant_gs = [1, 5 % (2 * n), 2 * n - 1], [1, 5 % (2 * n), 2 * n - 1]
    baby = [None if g == 1 else G.galois_key(BN.SEED, G.GK_BASE + 64 * r, s, mods, P, tab, g) for r, g in enumerate(baby_gs)]
    giant = [None if g == 1 else G.galois_key(BN.SEED, G.GK_BASE + 64 * (8 + r), s, mods, P, tab, g) for r, g in enumerate(giant_gs)]
    m = rng.integers(-64, 65, (len(giant_gs), len(baby_gs), n), dtype=np.int64)
    pts = LN.plaintext_evals(mods, P, m)
    out = BN.bsgs(mods, P, baby, baby_gs, giant, giant_gs, pts, ct)
    before, Q = E.phase_int(mods, n, s, ct)
    after, _ = E.phase_int(mods, n, s, out)
    exact = sum(G.galois_int(sum(E.negacyclic_int(G.galois_int(before, g), m[a, b]) for b, g in enumerate(baby_gs)), h) for a, h in enumerate(giant_gs))
    norms1 = [[int(np.abs(m[a, b]).sum()) for b, g in enumerate(baby_gs) if g != 1] for a in range(len(giant_gs))]
    sw = [h != 1 for h in giant_gs]
    bound, cbound = BN.bsgs_noise(n, k, norms1, sw), BN.composed_noise(n, k, norms1, sw)
    worst = int(np.abs(_centred(after - exact, Q)).max())
    comp, _ = E.phase_int(mods, n, s, BN.composed(mods, P, baby, baby_gs, giant, giant_gs, pts, ct))
    apart = int(np.abs(_centred(after - comp, Q)).max())
    print(f"n={n} k={k}: |dec(out) - exact|_inf = {worst} (bsgs_noise {bound}), against the composition {apart} (its bound {cbound})")
    assert worst <= bound and apart <= bound + cbound
    assert int(np.abs(_centred(comp - exact, Q)).max()) <= cbound            # the composition's bound is one


def test_word_for_word_anchors():
    for n, k in ((16, 3), (64, 2), (4, 1)):
        mods, P = E.chain(n, 58, 40, k - 1)
        m2 = 2 * n
        # every giant the identity: diag_sum with ONE output over the A B elements, hence the sum of the outputs before one division
        baby_gs, giant_gs = [1, 5 % m2, m2 - 1], [1, 1, 1]
        ct, baby, giant, pts = BN.random_case(mods, P, n, 2, baby_gs, giant_gs, 3 * n + k)
        got = BN.bsgs(mods, P, baby, baby_gs, giant, giant_gs, pts, ct)
        flat = pts.reshape((1, 9) + pts.shape[2:])
        assert np.array_equal(got, LN.diag_sum(mods, P, baby * 3, baby_gs * 3, flat, ct)[0])
        # ... and every baby too: the plain products, summed
        ones = BN.bsgs(mods, P, [None] * 3, [1, 1, 1], [None] * 3, [1, 1, 1], pts, ct)
        for i, q in enumerate(mods):
            tot = sum(pts[a, b, i].astype(object) for a in range(3) for b in range(3)) % q
            assert np.array_equal(ones[i], E.pmul(q, ct[i], tot.astype(U64)))
        # one giant h, one identity baby, m = 1: w = c1 exactly (U_P = 0 leaves nothing to round), so the result is apply_galois
        one = np.ones((1, 1, k + 1, n), dtype=U64)
        for h in G.case_elements(n):
            gk = LN.random_keys(mods, P, n, [5], n + h)[0]
            if h != 1:
                U = BN.baby_sums(mods, P, [None], [1], one, ct)[0]
                assert not U[-1].any() and np.array_equal(BN.giant_w(mods, P, U), ct[:, 1])
            want = ct if h == 1 else G.apply_galois(mods, P, gk, ct, h)
            assert np.array_equal(BN.bsgs(mods, P, [None], [1], [gk], [h], one, ct), want), (n, k, h)
        # the order of the giants, in the sum and in the lists, does not change a word
        giant_gs = [5 % m2, 1, m2 - 1, 5 % m2]
        ct, baby, giant, pts = BN.random_case(mods, P, n, 2, baby_gs, giant_gs, 5 * n + k)
        a = BN.bsgs(mods, P, baby, baby_gs, giant, giant_gs, pts, ct)
        assert np.array_equal(a, BN.bsgs(mods, P, baby, baby_gs, giant, giant_gs, pts, ct, order=[3, 1, 0, 2]))
        assert np.array_equal(a, BN.bsgs(mods, P, baby, baby_gs, giant[::-1], giant_gs[::-1], np.ascontiguousarray(pts[::-1]), ct))
    with pytest.raises(ValueError):
        BN.bsgs(mods, P, [None], [1], [None], [4], np.ones((1, 1, k + 1, n), dtype=U64), ct)
    with pytest.raises(ValueError):
        BN.bsgs(mods, P, [None], [2 * n], [None], [1], np.ones((1, 1, k + 1, n), dtype=U64), ct)


# ---- the fold order of the accumulate kernel ---------------------------------------------------------------------------------------------
def test_fold_order_at_the_largest_words():
    narrow, pn = E.chain(16, 58, 40, 7)
    wide, pw = E.wide_chain(16)
    assert max(narrow + [pn]) < 1 << 62 <= max(wide[0], pw) < 1 << 63
    for q in narrow + [pn] + wide + [pw]:
        for k in range(1, 9):
            for carry in (False, True):
                peak, word = BN.giantmac_fold_replay(q, k, carry)
                assert peak < 1 << 128, (q, k, carry)
                assert word == ((2 if carry else 1) * (q - 1) + k * (q - 1) ** 2) % q
    # without the folds a limb >= 2^62 would pass 128 bits at five digits: the rule is needed, and q < 2^62 needs none at k <= 8
    q = wide[0]
    assert 2 * (q - 1) + 5 * (q - 1) ** 2 >= 1 << 128 and 2 * ((1 << 62) - 1) + 8 * ((1 << 62) - 1) ** 2 < 1 << 128


# ---- the GPU module's case list ------------------------------------------------------------------------------------------------------------
def test_case_list_covers_every_path(pkg):
    B = pkg.binding
    cases = {(n, k, b) for n, k, b, _ in BN.WORD_CASES}
    assert cases == {(n, k, b) for n in (4, 16, 64) for k in (1, 2, 3) for b in (1, 3)}
    assert BN.BIG_CASE == (4096, 2, 257, (58, 40)) and BN.WIDE_CASE == (16, 8, 3, "wide") and BN.SWEEP == ([1, 5], [1, 25])
    # the new kernel's launches: within the grid cap, and past it (a second grid-stride pass)
    counts = set()
    for n, k, b, _ in BN.WORD_CASES + [BN.WIDE_CASE, BN.BIG_CASE]:
        counts |= BN.launch_elements(n, k, b)
    print(f"giantmac: launches of {min(counts)} .. {max(counts)} elements")
    assert min(counts) < E.GRID_CAP < max(counts)
    # more than one chunk: (4096, 2, 257) runs in 128 + 128 + 1, and in one chunk of 257 at one limb, past the cap
    assert E.chunk_rows(4096, 2, 257) == 128 and E.chunk_rows(4096, 1, 257) == 257 and 257 * 4096 > E.GRID_CAP
    # a limb >= 2^62 (the accumulators' other fold), the special prime too
    wide, wp = E.wide_chain(16)
    assert wide[0] >= 1 << 62 and wp >= 1 << 62
    for n in sorted({n for n, _, _, _ in BN.WORD_CASES}):
        lists = [(BN.reduced(BN.SWEEP[0], n), BN.reduced(BN.SWEEP[1], n))] + BN.element_cases(n)
        assert all(g % 2 == 1 and 0 < g < 2 * n for bs, gs in lists for g in bs + gs)
        # giants 1, 2, 3 around the pair; babies 1, 16, 17 around the group
        assert {len(gs) for _, gs in lists} >= {1, BN.PAIR, BN.PAIR + 1} and {len(bs) for bs, _ in lists} >= {1, BN.GROUP, BN.GROUP + 1}
        assert any(len(set(gs)) < len(gs) == 3 and any(g != 1 for g in gs) for _, gs in lists)      # three giants with one repeated
        # identity and non-identity in both roles, alone and mixed; the identity throughout
        assert any(gs == [1] for _, gs in lists) and any(len(gs) == 1 and gs[0] != 1 for _, gs in lists)
        assert any(1 in bs and any(g != 1 for g in bs) for bs, _ in lists) and any(all(g != 1 for g in bs) for bs, _ in lists)
        assert any(all(g == 1 for g in bs + gs) for bs, gs in lists) and any(all(g == 1 for g in bs) and any(g != 1 for g in gs) for bs, gs in lists)
        long = next(bs for bs, _ in lists if len(bs) == BN.GROUP + 1)
        assert n < 4 or (long[BN.GROUP] != 1 and 1 in long[:BN.GROUP])         # the second group switches a key too
    assert BN.MAX_BABIES == B.FHE_CKKS_GALOIS_MAX_COUNT == 256 and BN.MAX_GIANTS == B.FHE_CKKS_DIAG_MAX_OUTPUTS == 64
    # the workspace: neither count enters; the other entry points' values are as they were
    assert [BN.workspace_slabs(k) for k in (1, 2, 3, 8)] == [2 * k * k + 11 * k + 6 for k in (1, 2, 3, 8)]
    for n, k, b, babies, giants in ((4096, 2, 257, 1, 1), (4096, 2, 257, 256, 64), (4096, 3, 1024, 4, 4), (16, 8, 3, 17, 3), (2, 1, 1, 1, 1)):
        assert B.ckks_rns_bsgs_workspace_bytes(n, k, b, babies, giants) == BN.workspace_bytes(n, k, b)
    for args in ((4096, 2, 257, 0, 1), (4096, 2, 257, 257, 1), (4096, 2, 257, 1, 0), (4096, 2, 257, 1, 65), (12, 2, 1, 1, 1), (16, 9, 1, 1, 1), (16, 2, 0, 1, 1)):
        assert B.ckks_rns_bsgs_workspace_bytes(*args) == 0
    assert B.ckks_rns_diag_workspace_bytes(4096, 2, 257, 3, 2) == LN.workspace_bytes(4096, 2, 257, 2)
    assert B.ckks_rns_galois_workspace_bytes(4096, 2, 257, 8) == G.workspace_bytes(4096, 2, 257)
    # §30's launch formula and the modulus-downs it saves
    assert BN.launch_counts(3, [1, 5] * 9, [1, 25, 5], 2) == dict(lift=2 * (3 + 2 * 4 + 1), diagmac=2 * 2 * 2 * 4, giantmac=2 * 3 * 4, keymac=0, divround=2 * (2 * 3 + 3))
    assert BN.launch_counts(3, [1, 1], [1, 25], 1) == dict(lift=0 + 4 + 1, diagmac=4, giantmac=8, keymac=0, divround=6)
    assert BN.launch_counts(3, [1] * 17, [1, 1, 1], 2) == dict(lift=0, diagmac=2 * 4 * 3, giantmac=0, keymac=0, divround=0)
    assert BN.moddowns([1, 5, 25, 125]) == (3 + 2, 2 * 4 + 2 * 3)


# ---- rejections that need no device ----------------------------------------------------------------------------------------------------------
def test_abi_is_present(pkg):
    B = pkg.binding
    lib = pkg.load_library()
    assert hasattr(lib, "fhe_ckks_rns_bsgs_dev") and hasattr(lib, "fhe_ckks_rns_bsgs_workspace_bytes")
    assert {"fhe_ckks_rns_bsgs_dev", "fhe_ckks_rns_bsgs_workspace_bytes"} <= set(B.EXPORTS)
    assert callable(B.ckks_rns_bsgs_dev) and callable(B.ckks_rns_bsgs_workspace_bytes)


def test_rejections_without_a_device(pkg):
    B = pkg.binding
    n = 16
    mods, P = E.chain(n, 58, 40, 2)
    plans, sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    buf, key, pt, out = 0x10000, 0x40000, 0x80000, 0x400000
    ct_bytes = 3 * 2 * n * 8

    def code(*a, **kw):
        with pytest.raises(B.FheError) as e:
            B.ckks_rns_bsgs_dev(*a, **kw)
        return e.value.code

    for g in (4, 0, 2 * n, 2 * n + 1, 1 << 40):                              # an element, in either role
        assert code(plans, sp, [key], [g], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID
        assert code(plans, sp, [key], [5], [key], [g], 3, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key, key], [5, 2 * n], [None], [1], 3, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [], [], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID                    # babies = 0, and above the cap
    assert code(plans, sp, [key] * 257, [5] * 257, [key], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key], [5], [], [], 3, pt, buf, out, 1) == B.FHE_E_INVALID                    # giants = 0, and above its cap
    assert code(plans, sp, [key], [5], [key] * 65, [5] * 65, 3, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key], [5], [key], [5], 3, pt, buf, out, 0, babies=0) == B.FHE_E_INVALID      # the counts come before batch = 0
    assert code(plans, sp, [key], [5], [key], [5], 2, pt, buf, out, 1) == B.FHE_E_INVALID                # key_limbs < limbs
    assert code(plans, sp, [key], [5], [key], [5], 9, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key], [5], [key], [5], 3, pt, out, out, 1) == B.FHE_E_INVALID                # the output overlaps the input
    assert code(plans, sp, [out + ct_bytes - 8], [5], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID   # ... a baby key, at its last word
    assert code(plans, sp, [key], [5], [key, out + 8], [5, 25], 3, pt, buf, out, 1) == B.FHE_E_INVALID   # ... a giant key
    assert code(plans, sp, [key], [5], [key], [5], 3, out + 8, buf, out, 1) == B.FHE_E_INVALID           # ... the plaintexts
    assert code(plans, sp, [key] * 2, [5, 25], [key] * 2, [5, 25], 3, out - 2 * 2 * 4 * n * 8 + 8, buf, out, 1) == B.FHE_E_INVALID   # ... their last word
    assert code(plans, sp, [key], [5], [key], [5], 3, pt + 4, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key], [5], [key], [5], 3, pt, buf + 4, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key + 4], [5], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key], [5], [key + 4], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [key, None], [5, 25], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_NULL         # an element other than 1 needs its key: a baby
    assert code(plans, sp, [key], [5], [None, key], [25, 5], 3, pt, buf, out, 1) == B.FHE_E_NULL         # ... a giant
    assert code(plans, sp, None, [5], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, [key], [5], None, [1, 5], 3, pt, buf, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, [key], None, [key], [5], 3, pt, buf, out, 1, babies=1) == B.FHE_E_NULL
    assert code(plans, sp, [key], [5], [key], None, 3, pt, buf, out, 1, giants=1) == B.FHE_E_NULL
    assert code(plans, sp, [key], [5], [key], [5], 3, None, buf, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, [key], [5], [key], [5], 3, pt, None, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, [key], [5], [key], [5], 3, pt, buf, None, 1) == B.FHE_E_NULL
    assert code(plans, None, [key], [5], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_NULL
    assert code([plans[0], other], sp, [key], [5], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_PARAM_MISMATCH
    assert code(plans, plans[0], [key], [5], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code([plans[0], plans[1], plans[0]], sp, [key], [5], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID
    # the identity's key is not looked at, in either role: an entry inside the output is no overlap, and the next rejection is reached
    assert code(plans, sp, [out, key], [1, 4], [key], [5], 3, pt, buf, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, [out], [1], [out, None], [1, 5], 3, pt, buf, out, 1) == B.FHE_E_NULL
    # batch = 0 is a no-op, whatever the buffers
    B.ckks_rns_bsgs_dev(plans, sp, None, None, None, None, 3, None, None, None, 0, babies=1, giants=1)
    B.ckks_rns_bsgs_dev(plans, sp, [None], [4], [None], [4], 3, None, None, None, 0)


# ---- the Python surface that needs no device -----------------------------------------------------------------------------------------------
def test_python_surface_without_a_device(pkg):
    ck = pkg.ckks
    n = 16
    param = ck.RnsParam(n, *E.chain(n, 58, 40, 1))
    assert callable(ck.RnsCiphertext.linear_transform_hoisted)
    pts = ck.RnsPlaintextSet(param, 1, None, 2.0 ** 20, [1, 5])
    M = LN.matrices(n // 2, 3)["banded"]
    n1, baby, giant, _ = ck.bsgs_diagonals(M, 2)
    lt = ck.LinearTransform(param, n1, baby, giant, pts)
    assert lt.required_steps() == [1, 2, 6]
    ct = ck.RnsCiphertext(param, None, 1, 2.0 ** 30)
    with pytest.raises(KeyError, match="2"):
        ct.linear_transform_hoisted(lt, {1: None, 6: None})                  # the missing step is named before anything runs
    with pytest.raises(KeyError, match="1"):
        ct.linear_transform_hoisted(lt, {})
