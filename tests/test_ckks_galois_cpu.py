"""The Galois automorphisms of the CKKS evaluator without a device: the index permutation against the schoolbook
substitution through the transforms, its group law and block property, the hoisting identity, the key-switch error by CRT
recombination against §22's noise term, the rotation order of the slots, the consistency of the key's limbs, the row ranges,
the functional case against its derived bound, the proofs of the GPU module's case list, and the rejections that need no
device."""
import numpy as np
import pytest

import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_numpy as K
import _client_numpy as C

U64, I64 = np.uint64, np.int64


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


@pytest.fixture(scope="module")
def runs(tab):
    return {name: G.functional_run(case, tab) for name, case in G.FUNCTIONAL.items()}


def _odd(n):
    return range(1, 2 * n, 2)


# ---- the permutation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 8, 64, 1024])
def test_permutation_is_the_substitution_through_the_transforms(n):
    mods, P = E.chain(n, 58, 40, 1)
    gs = list(_odd(n)) if n <= 8 else [1, 5, 25, pow(5, n // 2 - 1, 2 * n), 2 * n - 1, 2 * n - 5, 3, n + 1]
    for q in (mods[0], mods[1], P):
        a = np.random.default_rng(n + q % 97).integers(0, q, (2, n), dtype=np.uint64)
        A = E.fwd(q, n, a)
        for g in gs:
            assert np.array_equal(E.fwd(q, n, G.galois_coeffs(q, a, g)), G.galois_evals(A, g)), (n, q, g)
    # the same permutation for every q, and the identity at g = 1
    assert np.array_equal(G.galois_perm(n, 1), np.arange(n))


@pytest.mark.parametrize("n", [2, 4, 16, 64, 256])
def test_permutations_compose_as_the_elements_multiply(n):
    gs = list(_odd(n)) if n <= 16 else [1, 5, 25, 2 * n - 1, 2 * n - 5, 3, n + 1, pow(5, n // 2 - 1, 2 * n)]
    for g in gs:
        pg = G.galois_perm(n, g)
        assert np.array_equal(np.sort(pg), np.arange(n))
        for h in gs:
            # sigma_h(sigma_g(a))^ = (a^[pi_g])[pi_h] = a^[pi_g[pi_h]]: the index arrays compose in this order
            assert np.array_equal(pg[G.galois_perm(n, h)], G.galois_perm(n, g * h % (2 * n))), (n, g, h)


@pytest.mark.parametrize("n", [64, 256, 4096])
def test_aligned_blocks_map_onto_aligned_blocks(n):
    for g in (5, 25, 2 * n - 1, 2 * n - 5, 3, pow(5, n // 2 - 1, 2 * n)):
        p = G.galois_perm(n, g)
        for t in (1, 3, 6):
            blocks = (p >> t).reshape(-1, 1 << t)
            assert (blocks == blocks[:, :1]).all(), (n, g, t)              # a wave of 64 outputs reads one aligned block of 64 words


def test_hoisting_identity_digits_commute_with_the_permutation():
    for n, k in ((16, 3), (64, 2)):
        mods, P = E.chain(n, 58, 40, k - 1)
        c1 = E.case_ct(mods, n, 2, 1, 31 + n)[:, 0]
        # rows whose coefficients sit at the centring's edge: the lift is odd, so the identity holds there too
        for j, q in enumerate(mods):
            c1[j, 0] = E.fwd(q, n, np.array([q // 2, q // 2 + 1] * (n // 2), dtype=U64))
        D = G.digits(mods, P, c1)
        for g in G.case_elements(n):
            assert np.array_equal(G.digits(mods, P, G.galois_evals(c1, g)), G.galois_evals(D, g)), (n, g)


# ---- the key switch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 16, 64])
def test_key_switch_error_by_crt(tab, n):
    k = 3
    mods, P = E.chain(n, 58, 40, k - 1)
    s = K.secret_key(G.SEED, 0, n)
    pk = E.public_key(G.SEED, E.PK_BASE, s, mods, tab)
    m = np.random.default_rng(n).integers(-(1 << 30), 1 << 30, (2, n), dtype=np.int64)
    ct = E.encrypt(G.SEED, 0, pk, m, 2, mods, tab)
    for t, g in enumerate(G.case_elements(n)):
        gk = G.galois_key(G.SEED, G.GK_BASE + 64 * t, s, mods, P, tab, g)
        for lv in (k, k - 1):                                               # the key of the whole chain serves the lower level
            ml = mods[:lv]
            before, Q = E.phase_int(ml, n, s, ct[:lv])
            after, _ = E.phase_int(ml, n, s, G.apply_galois(ml, P, gk, ct[:lv], g))
            diff = (after - G.galois_int(before, g)) % Q
            diff = np.where(diff > Q // 2, diff - Q, diff)
            worst = int(np.abs(diff).max())
            print(f"n={n} g={g} k={lv}: |c0' + c1' s - sigma_g(c0 + c1 s)|_inf = {worst}, bound {E.relin_noise(n, lv)}")
            assert worst <= E.relin_noise(n, lv)


def test_limbs_of_the_key_are_residues_of_one_key(tab):
    n, k, g = 16, 3, 5
    mods, P = E.chain(n, 58, 40, k - 1)
    s = K.secret_key(G.SEED, 0, n)
    gk = G.galois_key(G.SEED, G.GK_BASE + 64 * 7, s, mods, P, tab, g)
    sg = G.galois_int(np.array(s, dtype=object), g)
    allm = mods + [P]
    for j in range(k):
        errs = []
        for i, q in enumerate(allm):
            ph = E.inv(q, n, E.padd(q, gk[j, i, 0], E.pmul(q, gk[j, i, 1], E.fwd(q, n, E.residues(s, q))))).astype(object)
            if i == j:
                ph = (ph - (P % q) * sg) % q
            errs.append(np.where(ph > q // 2, ph - q, ph))
        assert all(np.array_equal(errs[0], x) for x in errs) and int(np.abs(errs[0]).max()) <= E.B_ERR
    # and the rows are those of the public key: the mask column is the MASK row's
    assert np.array_equal(gk[1, 2, 1], E.fwd(mods[2], n, K.uniform_row(G.SEED, G.GK_BASE + 64 * 7 + 1, n, mods[2])))


def test_row_ranges_are_disjoint():
    assert G.GK_BASE == 3 << 56
    top = G.GK_BASE + 64 * ((1 << 16) - 1) + 63
    for purpose, ranges in G.row_ranges().items():
        for a in range(len(ranges)):
            for b in range(a):
                assert ranges[a][0] >= ranges[b][1] or ranges[b][0] >= ranges[a][1], (purpose, ranges[a], ranges[b])
    mask, err = G.row_ranges()["MASK"][-1], G.row_ranges()["ERR"][-1]
    assert mask[0] <= G.GK_BASE and top < mask[1] and err[0] <= 2 * G.GK_BASE and 2 * top < err[1] and 2 * top + 1 < 1 << 63


# ---- slots ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 16, 64])
def test_rotation_order_rolls_and_conjugation_conjugates(n):
    idx, conj = G.rotation_order(n)
    assert np.array_equal(np.sort(idx), np.arange(n // 2))                 # every slot once
    rng = np.random.default_rng(n)
    z = rng.integers(-8, 8, (2, n // 2)) + 1j * rng.integers(-8, 8, (2, n // 2))
    assert np.array_equal(G.from_rotation_order(G.to_rotation_order(z)), z)
    delta = float(1 << 30)
    m = K.encode(z, delta)
    w = G.to_rotation_order(z)
    for step in (0, 1, 2, n // 2 - 1, n // 2 + 1, -1):
        got = K.decode(G.galois_int(m, G.galois_element(n, step)), delta)
        assert np.abs(G.to_rotation_order(got) - np.roll(w, -step, axis=-1)).max() < 1e-6, (n, step)
    got = K.decode(G.galois_int(m, G.conjugation_element(n)), delta)
    assert np.abs(got - np.conj(z)).max() < 1e-6
    assert np.abs(G.to_rotation_order(got) - np.conj(w)).max() < 1e-6


def test_python_helpers_are_the_restatements(pkg):
    ck = pkg.ckks
    for n in (2, 4, 16, 4096):
        for step in (0, 1, 3, n // 2, -1):
            assert ck.galois_element(n, step) == G.galois_element(n, step)
        assert ck.conjugation_element(n) == 2 * n - 1
        a, b = ck.rotation_order(n), G.rotation_order(n)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    z = np.random.default_rng(3).normal(size=(3, 8)) + 1j * np.random.default_rng(4).normal(size=(3, 8))
    assert np.array_equal(ck.to_rotation_order(z), G.to_rotation_order(z)) and np.array_equal(ck.from_rotation_order(ck.to_rotation_order(z)), z)
    assert ck.RnsClientKey.GK_BASE == G.GK_BASE and pkg.binding.FHE_CKKS_GALOIS_MAX_COUNT == G.MAX_COUNT
    param = ck.RnsParam(16, *E.chain(16, 58, 40, 1))
    for g in (0, 2, 32, 33):
        with pytest.raises(ValueError):
            ck.RnsGaloisKey(param, g, None)
    assert ck.RnsGaloisKey(param, 5, None).is_rotation and not ck.RnsGaloisKey(param, 5, None).is_conjugation
    assert ck.RnsGaloisKey(param, 31, None).is_conjugation and not ck.RnsGaloisKey(param, 31, None).is_rotation
    assert not ck.RnsGaloisKey(param, 3, None).is_rotation                 # 3 = -5^t: a rotation and the conjugation


# ---- the functional case ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.FUNCTIONAL))
def test_sum_of_all_slots_and_its_real_part(runs, name):
    r, case = runs[name], G.FUNCTIONAL[name]
    n = case["n"]
    assert len(r["mods"]) == 3 and len(r["gs"]) == (n // 2).bit_length()
    assert r["delta"] * n * E.ZMAX < r["mods"][0] / 4 and (r["delta"] == 2.0 ** case["bd"] or 2 * r["delta"] * n * E.ZMAX >= r["mods"][0] / 4)
    bound = r["bound"] + r["edec"]
    print(f"{name}: Delta = 2^{int(np.log2(r['delta']))}, worst slot error {r['err']:.3e}, derived bound {bound:.3e}")
    assert bound < 0.5 and r["err"] <= bound
    assert np.array_equal(np.round(r["w"].real), r["want"].real) and np.abs(r["w"].imag).max() <= bound
    assert np.abs(r["d"]).max() < r["mods"][0] // 2                         # decryption's contract at limb 0
    # the first rotation alone moves the slots by one place in the rotation order
    first = K.decode(E.decrypt(r["mods"], n, r["s"], G.apply_galois(r["mods"], r["P"], r["gks"][0], r["ct"], r["gs"][0])), r["delta"])
    assert np.abs(G.to_rotation_order(first) - np.roll(G.to_rotation_order(r["z"]), -1, axis=-1)).max() < 1e-3


def test_functional_delta_at_the_large_size():
    mods, _ = E.chain(4096, 58, 40, 2)
    assert G.functional_delta(4096, mods, 40) == 2.0 ** 40
    assert len(G.functional_steps(4096)) == 12


# ---- the GPU module's case list ------------------------------------------------------------------------------------------------------------
def test_case_list_covers_every_path(pkg):
    cases = {(n, k, b) for n, k, b, _ in G.WORD_CASES}
    assert cases >= {(2, 1, 1), (16, 8, 3), (256, 8, 3), (4096, 2, 257)} | {(n, k, b) for n in (4, 16, 64) for k in (1, 2, 3) for b in (1, 3)}
    for n in {n for n, _, _, _ in G.WORD_CASES}:
        gs = G.case_elements(n)
        assert len(set(gs)) == len(gs) and all(g % 2 == 1 and 0 < g < 2 * n for g in gs)
        assert 2 * n - 1 in gs and (n < 256 and 1 in gs or 5 in gs)
    assert G.case_elements(64) == [1, 5, pow(5, 31, 128), 127, 123] and G.case_elements(2) == [1, 3]
    # the grid cap, per new kernel: some launch takes one pass (at most 2^20 elements) and some launch a second one.  The
    # diagonal-term kernel runs over n <= 2^19 elements: it can never need a second pass.
    per_kernel = {}
    for n, k, b, _ in G.WORD_CASES:
        for name, counts in G.launch_elements(n, k, b).items():
            per_kernel.setdefault(name, set()).update(counts)
    assert set(per_kernel) == {"galois", "keymac_galois", "divround_galois"}
    for name, counts in per_kernel.items():
        print(f"{name}: launches of {min(counts)} .. {max(counts)} elements")
        assert min(counts) < E.GRID_CAP < max(counts), name
    # more than one chunk: (4096, 2, 257) switches keys in 128 + 128 + 1, and in one chunk of 257 at one limb
    assert E.chunk_rows(4096, 2, 257) == 128 and E.chunk_rows(4096, 1, 257) == 257
    assert all(b <= E.chunk_rows(n, k, b) for n, k, b, _ in G.WORD_CASES if n < 4096)
    # a limb >= 2^62 (the accumulator's other fold) with k = 8
    assert any(spec == "wide" and k == 8 and E.wide_chain(n)[0][0] >= 1 << 62 for n, k, _, spec in G.WORD_CASES)
    B = pkg.binding
    for n, k, b, count in ((4096, 2, 257, 1), (4096, 2, 257, 8), (16, 8, 3, 3), (2, 1, 1, 256)):
        assert B.ckks_rns_galois_workspace_bytes(n, k, b, count) == G.workspace_bytes(n, k, b)
    assert B.ckks_rns_galois_workspace_bytes(4096, 2, 257, 0) == 0 and B.ckks_rns_galois_workspace_bytes(4096, 2, 257, 257) == 0
    assert B.ckks_rns_galois_workspace_bytes(12, 2, 1, 1) == 0 and B.ckks_rns_galois_workspace_bytes(16, 9, 1, 1) == 0
    # §22's values are as they were
    assert B.ckks_rns_workspace_bytes(4096, 2, 257) == (4 + 16 + 2) * 128 * 4096 * 8


# ---- rejections that need no device ----------------------------------------------------------------------------------------------------------
def test_rejections_without_a_device(pkg):
    B = pkg.binding
    n = 16
    mods, P = E.chain(n, 58, 40, 2)
    plans, sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    buf = 0x10000

    def code(fn, *a, **kw):
        with pytest.raises(B.FheError) as e:
            fn(*a, **kw)
        return e.value.code

    ev = B.ckks_galois_evals_dev
    assert code(ev, None, 5, buf, buf * 2, 1) == B.FHE_E_NULL
    for g in (0, 2, 2 * n, 2 * n + 1, 1 << 40):
        assert code(ev, plans[0], g, buf, buf * 2, 1) == B.FHE_E_INVALID
    assert code(ev, plans[0], 5, None, buf * 2, 1) == B.FHE_E_NULL
    assert code(ev, plans[0], 5, buf, buf + 8 * n * 2, 3) == B.FHE_E_INVALID        # the output overlaps the input
    assert code(ev, plans[0], 5, buf, buf, 1) == B.FHE_E_INVALID
    assert code(ev, plans[0], 5, buf + 4, buf * 2, 1) == B.FHE_E_INVALID
    ev(plans[0], 5, None, None, 0)
    gk = B.ckks_rns_galois_key_dev
    for g in (0, 4, 2 * n):
        assert code(gk, plans, sp, bytes(32), 0, g, buf, None, 0, buf * 64) == B.FHE_E_INVALID
    assert code(gk, plans, None, bytes(32), 0, 5, buf, None, 0, buf * 64) == B.FHE_E_NULL
    assert code(gk, plans, sp, bytes(32), (1 << 63) - 2, 5, buf, None, 0, buf * 64) == B.FHE_E_INVALID
    assert code(gk, plans, sp, bytes(32), 0, 5, buf, None, 5, buf * 64) == B.FHE_E_NULL
    assert code(gk, [plans[0], other], sp, bytes(32), 0, 5, buf, None, 0, buf * 64) == B.FHE_E_PARAM_MISMATCH
    ap = B.ckks_rns_galois_dev
    key, out = buf * 4, buf * 64
    assert code(ap, plans, sp, [key], [4], 3, buf, out, 1) == B.FHE_E_INVALID
    assert code(ap, plans, sp, [key], [0], 3, buf, out, 1) == B.FHE_E_INVALID
    assert code(ap, plans, sp, [key], [2 * n + 1], 3, buf, out, 1) == B.FHE_E_INVALID
    assert code(ap, plans, sp, [key, key], [5, 2 * n], 3, buf, out, 1) == B.FHE_E_INVALID
    assert code(ap, plans, sp, [key] * 257, [5] * 257, 3, buf, out, 1) == B.FHE_E_INVALID           # count above the cap
    assert code(ap, plans, sp, [key], [5], 2, buf, out, 1) == B.FHE_E_INVALID                       # key_limbs < limbs
    assert code(ap, plans, sp, [key], [5], 9, buf, out, 1) == B.FHE_E_INVALID
    assert code(ap, plans, sp, [key], [5], 3, out, out, 1) == B.FHE_E_INVALID                       # the output overlaps the input
    assert code(ap, plans, sp, [key], [5], 3, buf, key, 1) == B.FHE_E_INVALID                       # ... a key
    assert code(ap, plans, sp, [key, out + 8 * 2 * 3 * n * 2 - 8], [5, 25], 3, buf, out, 1) == B.FHE_E_INVALID   # ... the second output, the second key
    assert code(ap, plans, sp, [key, None], [5, 25], 3, buf, out, 1) == B.FHE_E_NULL
    assert code(ap, plans, sp, None, [5], 3, buf, out, 1) == B.FHE_E_NULL
    assert code(ap, plans, sp, [key], None, 3, buf, out, 1, count=1) == B.FHE_E_NULL
    assert code(ap, plans, sp, [key], [5], 3, None, out, 1) == B.FHE_E_NULL
    assert code(ap, plans, None, [key], [5], 3, buf, out, 1) == B.FHE_E_NULL
    assert code(ap, [plans[0], other], sp, [key], [5], 3, buf, out, 1) == B.FHE_E_PARAM_MISMATCH
    assert code(ap, plans, plans[0], [key], [5], 3, buf, out, 1) == B.FHE_E_INVALID
    # batch = 0 or count = 0 is a no-op, whatever the buffers
    ap(plans, sp, None, None, 3, None, None, 0, count=0)
    ap(plans, sp, [None], [4], 3, None, None, 0)
    ap(plans, sp, [], [], 3, None, None, 5)
