"""The CKKS evaluator on an RNS chain without a device: the restatement's transforms against the oracle, the
algebra of relinearisation and rescaling by CRT recombination against §22's noise terms, the consistency of the per-limb
keys and encryptions, the functional test of the reference's style against the derived bound, the proofs of the GPU
module's case lists, and the rejections that need no device."""
import numpy as np
import pytest

import _ckks_eval_numpy as E
import _ckks_numpy as K
import _client_numpy as C

U64, I64 = np.uint64, np.int64


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


@pytest.fixture(scope="module")
def runs(tab):
    return {name: E.functional_run(case, tab) for name, case in E.FUNCTIONAL.items()}


def test_the_prime_rule_gives_the_issue_cross_check(tab):
    assert len(tab) == E.B_ERR
    mods, P = E.chain(32, 58, 40, 2)
    assert mods == [0x3ffffffffffffc1, 0xfffffff941, 0xfffffff6c1] and P == 0x7fffffffffff801
    for q in mods + [P]:
        assert E.is_prime(q) and q % 64 == 1
    assert [x for x in range(60) if E.is_prime(x)] == [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59]
    assert not E.is_prime(3215031751) and not E.is_prime(341550071728321)      # strong pseudoprimes to 2, 3, 5, 7 (and up to 17)


@pytest.mark.parametrize("q", [65537, 0xfffffff941, 0x3ffffffffffffc1, E.primes_below(63, 32, 1)[0]])
def test_schoolbook_transform_is_the_oracles(q):
    n = 32
    a = np.random.default_rng(5).integers(0, q, (3, n), dtype=np.uint64)
    b = np.random.default_rng(6).integers(0, q, (3, n), dtype=np.uint64)
    O = E.oracle()
    A = E.fwd(q, n, a)
    assert np.array_equal(A, O.ntt(q, n, a).reshape(3, n)) and np.array_equal(E.inv(q, n, A), a)
    assert np.array_equal(E.polymul(q, n, a, b), O.naive_negacyclic_mul(q, n, a, b).reshape(3, n))
    big = np.random.default_rng(7).integers(0, q, 1 << 15, dtype=np.uint64)
    assert np.array_equal(E.pmul(q, big, big[::-1]), ((big.astype(object) * big[::-1].astype(object)) % q).astype(U64))


def test_lift_centres_at_half():
    qj, qi = 0xfffffff941, 65537
    x = np.array([0, 1, qj // 2, qj // 2 + 1, qj - 1], dtype=U64)
    want = [0, 1, (qj // 2) % qi, (qj // 2 + 1 - qj) % qi, qi - 1]
    assert E.lift(x, qj, qi).tolist() == want
    assert E.residues(np.array([-1, -(1 << 63), (1 << 63) - 1], dtype=I64), qi).tolist() == [qi - 1, (-(1 << 63)) % qi, ((1 << 63) - 1) % qi]


# ---- check 2: the limbs are residues of one integer ciphertext ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.FUNCTIONAL))
def test_limbs_are_residues_of_one_ciphertext(runs, name):
    r, case = runs[name], E.FUNCTIONAL[name]
    n, mods = case["n"], r["mods"]
    for ct, m in ((r["ct1"], r["m1"]), (r["ct2"], r["m2"])):
        ph, Q = E.phase_int(mods, n, r["s"], ct)
        e = ph - m.astype(object)
        worst = int(np.abs(e).max())
        print(f"{name}: fresh |e|_inf = {worst}, bound {E.fresh_noise(n)}")
        assert worst <= E.fresh_noise(n)
        for i, q in enumerate(mods):                                       # and every limb's phase is that integer's residue
            assert np.array_equal(E.phase_limb(q, n, r["s"], ct[i]).astype(object), ph % q)
    # the key rows: pk0 + pk1 s = e, rlk0 + rlk1 s = e_j + [i = j] P s^2, the same small e_j in every limb
    s, allm = r["s"], mods + [r["P"]]
    s2 = E.negacyclic_int(np.array(s, dtype=object), s)
    for j in range(len(mods)):
        errs = []
        for i, q in enumerate(allm):
            ph = E.inv(q, n, E.padd(q, r["rlk"][j, i, 0], E.pmul(q, r["rlk"][j, i, 1], E.fwd(q, n, E.residues(s, q))))).astype(object)
            if i == j:
                ph = (ph - (r["P"] % q) * s2) % q
            errs.append(np.where(ph > q // 2, ph - q, ph))
        assert all(np.array_equal(errs[0], x) for x in errs) and int(np.abs(errs[0]).max()) <= E.B_ERR


# ---- check 1: the algebra by CRT ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.FUNCTIONAL))
def test_relinearise_and_rescale_by_crt(runs, name):
    r, case = runs[name], E.FUNCTIONAL[name]
    n, mods, s = case["n"], r["mods"], r["s"]
    for lv, (a, b) in ((len(mods), (r["ct1"], r["ct2"])), (len(mods) - 1, (r["prod"], r["prod"]))):
        m = mods[:lv]
        d = E.tensor(m, a[:lv], b[:lv])
        want, Q = E.phase_int(m, n, s, d)
        c = E.relinearize(m, r["P"], r["rlk"], d)
        got, _ = E.phase_int(m, n, s, c)
        diff = (got - want) % Q
        diff = np.where(diff > Q // 2, diff - Q, diff)
        worst = int(np.abs(diff).max())
        print(f"{name} k={lv}: relinearisation |e|_inf = {worst}, bound {E.relin_noise(n, lv)}")
        assert worst <= E.relin_noise(n, lv)
        c2 = E.rescale(m, c)
        got2, _ = E.phase_int(m[:-1], n, s, c2)
        num = got * 2 - got2 * (2 * m[-1])                                  # 2 (x - q x'), |.| <= (n + 1) q
        worst2 = int(np.abs(num).max())
        print(f"{name} k={lv}: rescale |x / q - x'|_inf = {worst2 / (2 * m[-1]):.3f}, bound {E.rescale_noise(n)}")
        assert worst2 <= 2 * m[-1] * E.rescale_noise(n)


# ---- check 3: the functional test ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.FUNCTIONAL))
def test_product_then_square_rounds_to_the_exact_slots(runs, name):
    r = runs[name]
    for i, (err, w, want) in enumerate(((r["err1"], r["w1"], r["z1"] * r["z2"]), (r["err2"], r["w2"], (r["z1"] * r["z2"]) ** 2))):
        bound = r["bounds"][i] + r["edec"][i]
        print(f"{name}: stage {i + 1} worst slot error {err:.3e}, derived bound {bound:.3e}")
        assert bound < 0.5                                                  # the bound holds with the restatement alone ...
        assert err <= bound and err < 0.5
        assert np.array_equal(np.round(w.real), want.real) and np.array_equal(np.round(w.imag), want.imag)
    assert np.abs(r["d2"]).max() < r["mods"][0] // 2                        # decryption's contract at limb 0


def test_plain_operands_and_additions(runs, tab):
    r, case = runs["n32"], E.FUNCTIONAL["n32"]
    n, mods, s, delta = case["n"], r["mods"], r["s"], r["delta"]
    z3 = E.functional_slots(case, 3)
    m3 = K.encode(z3, delta)
    got = K.decode(E.decrypt(mods, n, s, E.add_plain(mods, n, r["ct1"], m3)), delta)
    assert np.abs(got - (r["z1"] + z3)).max() < 1e-6
    c = E.rescale(mods, E.mul_plain(mods, n, r["ct1"], m3))
    got = K.decode(E.decrypt(mods, n, s, c), delta * delta / mods[-1])
    assert np.abs(got - r["z1"] * z3).max() < 1e-6


# ---- check 4: the GPU module's case lists ---------------------------------------------------------------------------------------------
def test_case_lists_cover_every_path(pkg):
    ks = {k for _, k, _, _ in E.WORD_CASES}
    assert {1, 2, 3, 8} <= ks
    assert {(n, k) for n, k, _, _ in E.WORD_CASES} >= {(n, k) for n in (4, 16, 64) for k in (1, 2, 3)} | {(16, 8), (256, 8), (1024, 3), (4096, 2), (4096, 1)}
    for n, k in {(n, k) for n, k, _, _ in E.WORD_CASES}:
        batches = {b for nn, kk, b, _ in E.WORD_CASES if (nn, kk) == (n, k)}
        assert 1 in batches or n >= 256
        assert any(b % 2 == 1 and b > 1 for b in batches)
    # every arithmetic kind the plans distinguish is a limb of the wide chain at n = 256, with one q >= 2^62 and one below 2^30
    for n in (16, 256):
        mods, P = E.wide_chain(n)
        assert len(set(mods + [P])) == 9 and P >= max(mods) and P < 1 << 63
        assert mods[0] >= 1 << 62 and min(mods) < 1 << 30 and any(q % (1 << 32) == 1 for q in mods)
    kinds = [pkg.Plan(q, 256).arithmetic() for q in E.wide_chain(256)[0]]
    print("arithmetic kinds of the wide chain at n = 256:", kinds)
    assert set(kinds) == E.ARITH_KINDS
    assert (256, 8, "wide") in {(n, k, spec) for n, k, _, spec in E.WORD_CASES}
    # the grid cap, per kernel and per launch: some launch takes one pass (at most 2^20 elements) and some launch a second one
    per_kernel = {}
    for n, k, b, _ in E.WORD_CASES:
        for name, counts in E.launch_elements(n, k, b).items():
            per_kernel.setdefault(name, set()).update(counts)
    for name, counts in per_kernel.items():
        print(f"{name}: launches of {min(counts)} .. {max(counts)} elements")
        assert min(counts) < E.GRID_CAP < max(counts), name
    # chunk edges: (4096, 2, 257) relinearises in 128 + 128 + 1 and rescales in 256 + 1; (4096, 1, 301) is one chunk of 301
    assert E.chunk_rows(4096, 2, 257) == 128 and E.chunk_rows(4096, 2, 257, rescale=True) == 256 and E.chunk_rows(4096, 1, 301) == 301
    assert all(b <= E.chunk_rows(n, k, b) for n, k, b, _ in E.WORD_CASES if n < 4096)
    assert pkg.binding.ckks_rns_workspace_bytes(4096, 2, 257) == (4 + 16 + 2) * 128 * 4096 * 8
    assert pkg.binding.ckks_rns_workspace_bytes(4096, 8, 300) == max((64 + 64 + 2) * 8, 2 * 8 * 64) * 4096 * 8
    # the accumulator's fold boundary: a limb >= 2^62 folds before digits 2, 4, 6: k = 1, 2 (no fold), 3 (one) and 8 (three) on that limb
    assert {k for n, k, _, spec in E.WORD_CASES if spec == "wide"} == {8}


# ---- check 5: rejections that need no device ------------------------------------------------------------------------------------------
def test_rejections_without_a_device(pkg):
    B = pkg.binding
    mods, P = E.chain(16, 58, 40, 2)
    plans, sp = [pkg.Plan(q, 16) for q in mods], pkg.Plan(P, 16)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    buf = 0x1000

    def code(fn, *a, **kw):
        with pytest.raises(B.FheError) as e:
            fn(*a, **kw)
        return e.value.code

    assert code(B.ckks_rns_tensor_dev, plans, buf, buf * 2, buf * 64, 1, limbs=0) == B.FHE_E_INVALID
    assert code(B.ckks_rns_tensor_dev, plans * 3, buf, buf * 2, buf * 64, 1) == B.FHE_E_INVALID          # 9 limbs
    assert code(B.ckks_rns_tensor_dev, [plans[0], None], buf, buf * 2, buf * 64, 1) == B.FHE_E_NULL
    assert code(B.ckks_rns_tensor_dev, [plans[0], other], buf, buf * 2, buf * 64, 1) == B.FHE_E_PARAM_MISMATCH
    assert code(B.ckks_rns_tensor_dev, [plans[0], plans[1], plans[0]], buf, buf * 2, buf * 64, 1) == B.FHE_E_INVALID
    assert code(B.ckks_rns_tensor_dev, plans, None, buf * 2, buf * 64, 1) == B.FHE_E_NULL
    assert code(B.ckks_rns_tensor_dev, plans, buf, buf * 2, buf, 1) == B.FHE_E_INVALID                     # the output overlaps a
    assert code(B.ckks_rns_tensor_dev, plans, buf + 4, buf * 2, buf * 64, 1) == B.FHE_E_INVALID            # alignment
    assert code(B.ckks_rns_mul_dev, plans, None, buf, 3, buf * 2, buf * 4, buf * 64, 1) == B.FHE_E_NULL
    assert code(B.ckks_rns_mul_dev, plans, plans[0], buf, 3, buf * 2, buf * 4, buf * 64, 1) == B.FHE_E_INVALID   # P repeats q_0
    assert code(B.ckks_rns_mul_dev, plans, pkg.Plan(mods[1], 16), buf, 3, buf * 2, buf * 4, buf * 64, 1) == B.FHE_E_INVALID
    assert code(B.ckks_rns_mul_dev, [plans[1], plans[2]], plans[0], buf, 1, buf * 2, buf * 4, buf * 64, 1) == B.FHE_E_INVALID   # key_limbs < limbs
    assert code(B.ckks_rns_relinearize_dev, plans, pkg.Plan(65537, 16), buf, 3, buf * 2, buf * 64, 1) == B.FHE_E_INVALID       # P < max q
    assert code(B.ckks_rns_rescale_dev, plans[:1], buf, buf * 64, 1) == B.FHE_E_INVALID
    assert code(B.ckks_rns_rescale_dev, plans, buf, buf, 1) == B.FHE_E_INVALID
    assert code(B.ckks_rns_from_i64_dev, plans, None, buf, 1) == B.FHE_E_NULL
    assert code(B.ckks_rns_relin_key_dev, plans, sp, bytes(32), (1 << 63) - 2, buf, None, 0, buf * 64) == B.FHE_E_INVALID
    assert code(B.ckks_rns_relin_key_dev, plans, sp, bytes(32), 0, buf, None, 5, buf * 64) == B.FHE_E_NULL   # a table of 5 entries at NULL
    # batch = 0 is a no-op, whatever the buffers
    B.ckks_rns_tensor_dev(plans, None, None, None, 0)
    B.ckks_rns_rescale_dev(plans, None, None, 0)
    assert B.ckks_rns_workspace_bytes(16, 0, 1) == 0 and B.ckks_rns_workspace_bytes(12, 2, 1) == 0
    with pytest.raises(ValueError):
        pkg.ckks.RnsParam(16, mods, mods[1])
    with pytest.raises(ValueError):
        pkg.ckks.RnsParam(16, mods, 65537)
