"""The CKKS polynomial evaluation without a device: the planner against chebval, its structure against an
independent recurrence, the scale rule, the accumulators' overflow argument on edge residues in exact integers, the proofs of
the GPU module's case list, the whole pipeline on the restatement within a bound composed from §22's noise terms, and every
rejection of the C entry point with fake addresses."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as Ch

import _ckks_eval_numpy as E
import _ckks_numpy as K
import _ckks_poly_numpy as PN
import _client_numpy as C

U64 = np.uint64
SIM_TOL = 2.0 ** -40            # 29 times the worst |simulate - chebval| measured here (3.1e-14, at degree 63): float64 noise


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _y(x, iv):
    return (2 * x - iv[0] - iv[1]) / (iv[1] - iv[0])


# ---- the planner -----------------------------------------------------------------------------------------------------------------------
def test_simulate_is_chebval(pkg):
    ck = pkg.ckks
    rng = np.random.default_rng(27)
    worst = 0.0
    for d in list(range(1, 32)) + [63]:
        c = rng.uniform(-1, 1, d + 1)
        for iv in ((-1.0, 1.0), (-4.0, 4.0)):
            x = np.linspace(iv[0], iv[1], 64)
            err = float(np.abs(ck.ChebyshevPlan.build(c, iv).simulate(x) - Ch.chebval(_y(x, iv), c)).max())
            worst = max(worst, err)
            assert err <= SIM_TOL, (d, iv, err)
    print(f"worst |simulate - chebval| = {worst:.3e}")


def test_plan_structure_and_determinism(pkg):
    ck = pkg.ckks
    rng = np.random.default_rng(28)
    assert PN.product_count(7) == 4 and PN.product_count(15) == 7       # the issue's two numbers, from the recurrence
    for d in list(range(1, 32)) + [63]:
        c = rng.uniform(-1, 1, d + 1)
        m = d.bit_length()
        for iv in ((-1.0, 1.0), (-4.0, 4.0)):
            plan = ck.ChebyshevPlan.build(c, iv)
            mapped = iv != (-1.0, 1.0)
            assert plan.products == PN.product_count(d) == sum(op[0] == "mul" for op in plan.ops), d
            assert plan.levels == PN.level_count(d, mapped) <= m + 1 + mapped, d
            assert plan.n1 == 1 << ((m + 1) // 2) and plan.babies == list(range(1, plan.n1))
            assert {op[0] for op in plan.ops} <= {"lincomb", "mul", "rescale"}
            assert plan.drop[plan.result] == plan.levels and plan.scale[plan.result] == (1, ())   # the input's scale, symbolically
            again = ck.ChebyshevPlan.build(c.copy(), iv)
            assert repr(again.ops) == repr(plan.ops) and again.result == plan.result
            # all leaves of one level share one call: no two lincombs over babies alone sit at one level
            babies = {w for op in plan.ops if op[0] == "rescale" for w in [op[1]]} | {0}
            leaf_levels = [op[6] for op in plan.ops if op[0] == "lincomb" and len(op[2]) + len(op[1]) > 2 and set(op[2]) <= babies and op[3][0] != [2.0, -1.0]]
            assert len(leaf_levels) == len(set(leaf_levels)), d
    plan = ck.ChebyshevPlan.build(rng.uniform(-1, 1, 16))
    assert max(len(op[1]) for op in plan.ops if op[0] == "lincomb") == 2     # degree 15: two of its four leaves sit at one level
    with pytest.raises(ValueError):
        ck.ChebyshevPlan.build([1.0])
    with pytest.raises(ValueError):
        ck.ChebyshevPlan.build([1.0, 1j])
    with pytest.raises(ValueError):
        ck.ChebyshevPlan.build([1.0, 2.0], (1, 1))


def test_scale_rule_makes_every_addition_exact(pkg):
    """symbolically: a lincomb with more than one output or whose inputs include an unrescaled product has that product's scale
    as its target, and the weight of every input whose symbolic scale is the target is its coefficient exactly"""
    ck = pkg.ckks
    rng = np.random.default_rng(29)
    mods, _ = E.chain(32, 58, 40, 7)
    for d in (3, 7, 12, 15, 31):
        for iv in ((-1.0, 1.0), (-4.0, 4.0)):
            plan = ck.ChebyshevPlan.build(rng.uniform(-1, 1, d + 1), iv)
            made_by = {}
            for op in plan.ops:
                for w in (op[1] if op[0] == "lincomb" else [op[1]]):
                    made_by[w] = op[0]
            sums = 0
            for op in plan.ops:
                if op[0] != "lincomb":
                    continue
                _, outs, ins, co, consts, syms, drop = op
                assert all(plan.drop[i] <= drop for i in ins) and all(plan.drop[w] == drop and plan.scale[w] == sym for w, sym in zip(outs, syms))
                if len(outs) > 1:                                         # a shared leaf call: nothing below applies to it
                    continue
                sym = syms[0]
                prods = [i for i in ins if made_by.get(i) == "mul"]
                for i in prods:
                    assert plan.scale[i] == sym                           # the sum lands on the product's scale
                if prods and len(ins) == 2 and co == [[1.0, 1.0]]:        # q T_g + r: r was evaluated to that very scale
                    assert plan.scale[ins[1]] == sym
                    sums += 1
                # numerically the weights of same-scale inputs are the coefficients
                S = ck.ChebyshevPlan.scale_value(sym, 2.0 ** 40, mods, 7)
                assert S == PN.scale_value(sym, 2.0 ** 40, mods, 7)
                for r, i in enumerate(ins):
                    if plan.scale[i] == sym:
                        si = PN.scale_value(plan.scale[i], 2.0 ** 40, mods, 7)
                        assert all(round(row[r] * S / si) == row[r] for row in co if float(row[r]).is_integer())
            assert sums == PN.product_count(d) - (plan.n1 - 2) - len(plan.giants)


# ---- the kernel's overflow argument, in exact integers -----------------------------------------------------------------------------------
def _accumulate(q, xs, ws, k0, group=PN.GROUP):
    """the kernel's order of operations on Python integers, asserting the 128-bit bound it claims at every step"""
    chunk = PN.CHUNK63 if q >> 62 else PN.CHUNK
    word = None
    for r0 in range(0, len(xs), group):
        v = k0 if word is None else word                                     # the constant, or the carried canonical word
        assert v < q
        for r in range(min(group, len(xs) - r0)):
            if r and r % chunk == 0:
                v %= q
            v += ws[r0 + r] * xs[r0 + r]
            assert v < 1 << 128, (q, r0, r)
        word = v % q
    return word


@pytest.mark.parametrize("count", PN.OVERFLOW_COUNTS)
def test_overflow_proof_on_edge_residues(count):
    wide, _ = E.wide_chain(16)
    q61 = E.primes_below(61, 16, 1)[0]
    assert wide[0] >= 1 << 62 and (1 << 60) < q61 < (1 << 61)
    for q in (q61, E.primes_below(62, 16, 1)[0], wide[0]):
        xs, ws = [q - 1] * count, [q - 1] * count
        want = (sum(w * x for w, x in zip(ws, xs)) + q - 1) % q
        assert _accumulate(q, xs, ws, q - 1) == want
        ct = np.full((1, 2, 1, 4), q - 1, dtype=U64)
        got = PN.lincomb([q], [ct] * count, [[[q - 1]] * count], [[q - 1]])
        assert (got[0, 0, 0] == U64(want)).all() and (got[0, 0, 1] == U64((want - (q - 1)) % q)).all()


# ---- the GPU module's case list ------------------------------------------------------------------------------------------------------------
def test_case_list_covers_every_path(pkg):
    B = pkg.binding
    assert (B.FHE_CKKS_LINCOMB_MAX_COUNT, B.FHE_CKKS_LINCOMB_MAX_OUTPUTS) == (PN.MAX_COUNT, PN.MAX_OUTPUTS) == (64, 16)
    assert {(n, k) for n, k, _, _ in PN.WORD_CASES} >= {(n, k) for n in (4, 16, 64) for k in (1, 2, 3)} | {(16, 8), (256, 8)}
    assert {b for _, _, b, _ in PN.WORD_CASES} == {1, 3}
    assert set(PN.COUNTS) == {1, 2, 3, 8, 9, 16, 17, 33} and set(PN.OUTPUTS) == {1, 2, 3, 5}
    for n, k, _, spec in PN.WORD_CASES:
        cases = PN.sweep(n, k)
        assert {c for c, _, _ in cases} == set(PN.COUNTS) and {o for _, o, _ in cases} == set(PN.OUTPUTS)
        assert {kk for _, _, kk in cases} == {True, False}
        # each NOUT split: a launch of 1, 2, 3 and 4 outputs, and a call of more than one launch
        launches = {min(PN.OUT_CAP, o - o0) for _, o, _ in cases for o0 in range(0, o, PN.OUT_CAP)}
        assert launches == {1, 2, 3, 4} and any(o > PN.OUT_CAP for _, o, _ in cases)
        # the carry path: one group, exactly one group, two groups, three groups; with several outputs too
        assert {-(-c // PN.GROUP) for c, _, _ in cases} == {1, 2, 3} and PN.GROUP in PN.COUNTS and PN.GROUP + 1 in PN.COUNTS
        assert any(c > PN.GROUP and o > 1 for c, o, _ in cases)
        # both fold rules' boundaries inside one group
        assert {PN.CHUNK, PN.CHUNK + 1, PN.CHUNK63, PN.CHUNK63 + 1} <= set(PN.COUNTS)
        if spec == "wide":
            mods, _ = E.case_chain(n, k, spec)
            assert mods[0] >= 1 << 62 and any(q < 1 << 62 for q in mods)
    wide = [(n, k) for n, k, _, spec in PN.WORD_CASES if spec == "wide"]
    assert (16, 8) in wide and (256, 8) in wide
    # a launch within the grid and one that needs a second grid-stride pass
    sizes = {2 * b * n for n, _, b, _ in PN.WORD_CASES}
    n, k, b, _ = PN.BIG_CASE
    assert (n, k, b) == (4096, 1, 301) and max(sizes) < E.GRID_CAP < 2 * b * n
    assert PN.launch_counts(3, 17, 5) == 2 * 3 * 2 and PN.launch_counts(1, 16, 4) == 1 and PN.launch_counts(8, 64, 16) == 4 * 8 * 4


# ---- the whole pipeline on the restatement ---------------------------------------------------------------------------------------------------
def functional_run(pkg, tab, case):
    """encrypt, replay the plan, decrypt and decode, all in the restatement -> everything the GPU module compares against"""
    ck = pkg.ckks
    n, rows = case["n"], case["rows"]
    mods, P = E.chain(n, 58, 40, 7)
    s = K.secret_key(PN.SEED, 0, n)
    pk = E.public_key(PN.SEED, E.PK_BASE, s, mods, tab)
    rlk = E.relin_key(PN.SEED, E.RLK_BASE, s, mods, P, tab)
    z = PN.functional_slots(case)
    ct = E.encrypt(PN.SEED, 0, pk, K.encode(z, PN.DELTA), rows, mods, tab)
    coeffs = PN.functional_coeffs(case)
    plan = ck.ChebyshevPlan.build(coeffs, case["interval"])
    wires = PN.replay(plan, ct, PN.DELTA, 7, mods, P, rlk)
    res, level, scale = wires[plan.result]
    d = E.decrypt(mods[:level + 1], n, s, res)
    got = K.decode(d, scale)
    want = Ch.chebval(_y(z.real, case["interval"]), coeffs)
    xmax = max(abs(case["interval"][0]), abs(case["interval"][1]))
    bound, bscale = PN.poly_bounds(plan, n, mods, 7, PN.DELTA, xmax)
    assert bscale == scale
    return dict(mods=mods, P=P, s=s, pk=pk, rlk=rlk, z=z, ct=ct, coeffs=coeffs, plan=plan, wires=wires, res=res, level=level, scale=scale,
                got=got, want=want, err=float(np.abs(got - want).max()), bound=bound + float(K.e_dec(d, scale).max()))


@pytest.mark.parametrize("name", list(PN.FUNCTIONAL))
def test_pipeline_accuracy_on_the_restatement(pkg, tab, name):
    """measured (this test prints them): deg7 at n = 16 on [-1, 1]: error 4.8e-10, bound 9.3e-06; logistic15 at n = 32 on [-4, 4]: error
    9.8e-11, bound 9.2e-06"""
    case = PN.FUNCTIONAL[name]
    run = functional_run(pkg, tab, case)
    assert run["level"] == 7 - run["plan"].levels
    print(f"{name}: n={case['n']} degree {case['degree']} on {case['interval']}: worst slot error {run['err']:.3e}, derived bound {run['bound']:.3e}")
    assert run["bound"] < 2.0 ** -10                                         # the test cannot pass on garbage
    assert run["err"] <= run["bound"]
    if case["degree"] == 15:                                                 # and the fit is the logistic function to what degree 15 gives
        assert np.abs(run["want"] - PN.logistic(run["z"].real)).max() < 1e-3


# ---- rejections that need no device -----------------------------------------------------------------------------------------------------------
def test_rejections_without_a_device(pkg):
    B = pkg.binding
    n = 16
    mods, _ = E.chain(n, 58, 40, 2)
    plans = [pkg.Plan(q, n) for q in mods]
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    a, b, out = 0x10000, 0x40000, 0x400000
    ct_bytes = 3 * 2 * n * 8
    one = [1, 1, 1]

    def code(*args, **kw):
        with pytest.raises(B.FheError) as e:
            B.ckks_rns_lincomb_dev(*args, **kw)
        return e.value.code

    assert code(None, [a], one, None, 1, out, 1, limbs=3) == B.FHE_E_NULL
    assert code([plans[0], None, plans[2]], [a], one, None, 1, out, 1) == B.FHE_E_NULL
    assert code(plans, None, one, None, 1, out, 1, count=1) == B.FHE_E_NULL
    assert code(plans, [a], None, None, 1, out, 1) == B.FHE_E_NULL
    assert code(plans, [a, None], one * 2, None, 1, out, 1) == B.FHE_E_NULL
    assert code(plans, [a], one, None, 1, None, 1) == B.FHE_E_NULL
    assert code([plans[0], other], [a], one[:2], None, 1, out, 1) == B.FHE_E_PARAM_MISMATCH
    assert code([plans[0], plans[1], plans[0]], [a], one, None, 1, out, 1) == B.FHE_E_INVALID          # repeated moduli
    assert code([], [a], [], None, 1, out, 1) == B.FHE_E_INVALID                                       # limbs = 0, and 9
    assert code(plans * 3, [a], one * 3, None, 1, out, 1) == B.FHE_E_INVALID
    assert code(plans, [], [], None, 1, out, 1) == B.FHE_E_INVALID                                     # count = 0, and 65
    assert code(plans, [a] * 65, one * 65, None, 1, out, 1) == B.FHE_E_INVALID
    assert code(plans, [a], one, None, 0, out, 1) == B.FHE_E_INVALID                                   # outputs = 0, and 17
    assert code(plans, [a], one * 17, None, 17, out, 1) == B.FHE_E_INVALID
    for i, q in enumerate(mods):                                                                       # a weight, a constant at its modulus
        w = list(one)
        w[i] = q
        assert code(plans, [a], w, None, 1, out, 1) == B.FHE_E_INVALID
        assert code(plans, [a], one, w, 1, out, 1) == B.FHE_E_INVALID
    assert code(plans, [a, b], one * 4, [0] * 3 + [0, 0, mods[2]], 2, out, 1) == B.FHE_E_INVALID       # ... of the second output
    assert code(plans, [out], one, None, 1, out, 1) == B.FHE_E_INVALID                                 # the output overlaps an input
    assert code(plans, [a, out + 2 * ct_bytes - 8], one * 4, None, 2, out, 1) == B.FHE_E_INVALID       # ... the second, in the second output's last word
    assert code(plans, [a, out - ct_bytes + 8], one * 2, None, 1, out, 1) == B.FHE_E_INVALID           # ... ending in its first
    assert code(plans, [a + 4], one, None, 1, out, 1) == B.FHE_E_INVALID
    assert code(plans, [a], one, None, 1, out + 4, 1) == B.FHE_E_INVALID
    # batch = 0 is a no-op, whatever the buffers
    B.ckks_rns_lincomb_dev(plans, [None], one, None, 1, None, 0)
    B.ckks_rns_lincomb_dev(plans, [out], one, one, 1, out, 0)


# ---- the Python surface that needs no device -----------------------------------------------------------------------------------------------
def test_python_surface_without_a_device(pkg):
    ck = pkg.ckks
    n = 16
    mods, P = E.chain(n, 58, 40, 2)
    param = ck.RnsParam(n, mods, P)

    class Rows:                                                               # the shape of a device tensor, without one
        shape = (3, 2, 2, n)
    ct = ck.RnsCiphertext(param, Rows(), 2, 2.0 ** 40)
    for bad in ([1j], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            ck.lincomb([ct], bad)
    with pytest.raises(ValueError, match="constant polynomial"):
        ck.lincomb([ct], [1.0], consts=[1j])
    with pytest.raises(ValueError):
        ck.lincomb([ct], [1.0, 2.0])
    with pytest.raises(ValueError):
        ck.lincomb([ct], [1.0], consts=[1.0, 2.0])
    with pytest.raises(ValueError):
        ck.lincomb([], [])
    with pytest.raises(ValueError):
        ck.lincomb([ct], [1.0], level=3)
    with pytest.raises(pkg.binding.FheError):
        ck.lincomb([ct, ck.RnsCiphertext(ck.RnsParam(n, mods[:2], P), Rows(), 1, 1.0)], [1.0, 1.0])
    plan = ck.ChebyshevPlan.build(np.ones(8))
    assert plan.levels == 4
    with pytest.raises(ValueError, match="4 levels"):                        # refused before anything runs
        ct.eval_chebyshev(plan, None)
    with pytest.raises(ValueError, match="5 levels"):
        ct.eval_chebyshev(np.ones(8), None, interval=(-4, 4))
    c = ck.chebyshev_fit(PN.logistic, 15, (-4.0, 4.0))
    assert np.array_equal(c, PN.chebyshev_fit(PN.logistic, 15, (-4.0, 4.0)))
    x = np.linspace(-4, 4, 101)
    assert np.abs(Ch.chebval(x / 4, c) - PN.logistic(x)).max() < 1e-3
