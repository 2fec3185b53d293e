"""The CKKS polynomial evaluation on the device (ckks_eval.hip): fhe_ckks_rns_lincomb_dev word for word against
tests/_ckks_poly_numpy.py (tolerance zero) on the case list tests/test_ckks_poly_cpu.py proved; inputs at a higher level, a
repeated pointer, edge residues, a launch past the grid cap; the inputs untouched; every rejection with its outputs untouched;
the launch counts; the Python surface; eval_chebyshev through ckks.RnsClientKey word for word against the replay of its plan
and within the CPU module's bound; the level refusal."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as Ch

import _ckks_eval_numpy as E
import _ckks_linear_numpy as LN
import _ckks_numpy as K
import _ckks_poly_numpy as PN
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A


def _refused():
    return pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ")


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


def _plans(pkg, mods, n):
    return [pkg.Plan(q, n) for q in mods]


def _lincomb(pkg, plans, d_cts, w, k, batch, n):
    outputs = len(w)
    out = _empty((outputs, len(plans), 2, batch, n))
    pkg.binding.ckks_rns_lincomb_dev(plans, [x.data_ptr() for x in d_cts], PN.flat(w), PN.flat(k), outputs, out.data_ptr(), batch)
    return _u64(out)


# ---- the sweep, word for word -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch,spec", PN.WORD_CASES)
def test_lincomb_word_for_word(pkg, n, k, batch, spec):
    mods, _ = E.case_chain(n, k, spec)
    plans = _plans(pkg, mods, n)
    top = max(PN.COUNTS)
    cts = [E.case_ct(mods, n, batch, 2, 900 * n + 7 * k + r) for r in range(top)]
    d_cts = [_dev(x) for x in cts]
    for count, outputs, consts in PN.sweep(n, k):
        w, kk = PN.random_weights(mods, outputs, count, 31 * count + outputs, consts)
        got = _lincomb(pkg, plans, d_cts[:count], w, kk, batch, n)
        assert np.array_equal(got, PN.lincomb(mods, cts[:count], w, kk)), (count, outputs, consts)
    for x, d in zip(cts, d_cts):                                             # the inputs are only read
        assert np.array_equal(_u64(d), x)


def test_higher_level_inputs_a_repeated_pointer_and_edge_residues(pkg):
    n, batch = 16, 3
    mods, _ = E.wide_chain(n)
    assert mods[0] >= 1 << 62
    plans = _plans(pkg, mods, n)
    full = [E.case_ct(mods, n, batch, 2, 60 + r) for r in range(3)]
    d_full = [_dev(x) for x in full]
    for k in (1, 3, 8):                                                      # inputs of 8 limbs read at k: truncation costs nothing
        w, kk = PN.random_weights(mods[:k], 2, 3, 70 + k)
        assert np.array_equal(_lincomb(pkg, plans[:k], d_full, w, kk, batch, n), PN.lincomb(mods[:k], full, w, kk)), k
    w, kk = PN.random_weights(mods, 3, 4, 80)                                # the same pointer twice, and three times
    order = [0, 1, 0, 0]
    got = _lincomb(pkg, plans, [d_full[i] for i in order], w, kk, batch, n)
    assert np.array_equal(got, PN.lincomb(mods, [full[i] for i in order], w, kk))
    for count in (PN.GROUP + 1, PN.MAX_COUNT):                               # q - 1 everywhere: the fold rules' worst case, both kinds of limb
        edge = [PN.edge_ct(mods, batch, n, r) for r in range(2)]
        d_edge = [_dev(x) for x in edge]
        w = [[[q - 1 for q in mods] for _ in range(count)] for _ in range(2)]
        kk = [[q - 1 for q in mods] for _ in range(2)]
        got = _lincomb(pkg, plans, [d_edge[r % 2] for r in range(count)], w, kk, batch, n)
        assert np.array_equal(got, PN.lincomb(mods, [edge[r % 2] for r in range(count)], w, kk)), count


def test_a_launch_past_the_grid_cap(pkg):
    n, k, batch, spec = PN.BIG_CASE
    mods, _ = E.case_chain(n, k, spec)
    plans = _plans(pkg, mods, n)
    cts = [E.case_ct(mods, n, batch, 2, 90 + r) for r in range(2)]
    w, kk = PN.random_weights(mods, 2, 2, 91)
    got = _lincomb(pkg, plans, [_dev(x) for x in cts], w, kk, batch, n)
    q = mods[0]                                                              # the oracle's products: Python integers are too slow at this size
    for o in range(2):
        want = E.padd(q, E.pmul(q, cts[0][0], U64(w[o][0][0])), E.pmul(q, cts[1][0], U64(w[o][1][0])))
        want[0] = E.padd(q, want[0], U64(kk[o][0]))
        assert np.array_equal(got[o, 0], want), o


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_outputs_untouched(pkg):
    B = pkg.binding
    n, k = 16, 3
    mods, _ = E.chain(n, 58, 40, k - 1)
    plans = _plans(pkg, mods, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    a = _dev(E.case_ct(mods, n, 2, 2, 5))
    o2 = _empty((2, k, 2, 2, n))
    A, O2 = a.data_ptr(), o2.data_ptr()
    ct_bytes = k * 2 * 2 * n * 8
    one, f = [1] * k, B.ckks_rns_lincomb_dev
    bad = [
        (B.FHE_E_NULL, (plans, [A, None], one * 4, None, 2, O2, 2)),
        (B.FHE_E_NULL, (plans, [A, A], None, None, 2, O2, 2)),
        (B.FHE_E_NULL, ([plans[0], None, plans[2]], [A, A], one * 4, None, 2, O2, 2)),
        (B.FHE_E_PARAM_MISMATCH, ([plans[0], plans[1], other], [A, A], one * 4, None, 2, O2, 2)),
        (B.FHE_E_INVALID, ([plans[0], plans[1], plans[0]], [A, A], one * 4, None, 2, O2, 2)),
        (B.FHE_E_INVALID, (plans, [A] * 65, one * 130, None, 2, O2, 2)),
        (B.FHE_E_INVALID, (plans, [A, A], one * 4, None, 0, O2, 2)),
        (B.FHE_E_INVALID, (plans, [A], one * 17, None, 17, O2, 2)),
        (B.FHE_E_INVALID, (plans, [A, A], one + [mods[0], 1, 1], None, 1, O2, 2)),
        (B.FHE_E_INVALID, (plans, [A, A], one * 4, one + [1, 1, mods[2]], 2, O2, 2)),
        (B.FHE_E_INVALID, (plans, [A, O2 + 2 * ct_bytes - 8], one * 4, None, 2, O2, 2)),      # an input at the output's last word
        (B.FHE_E_INVALID, (plans, [O2 - ct_bytes + 8, A], one * 4, None, 2, O2, 2)),          # ... ending in its first
        (B.FHE_E_INVALID, (plans, [A + 4, A], one * 4, None, 2, O2, 2)),
    ]
    for code, args in bad:
        with _refused() as e:
            f(*args)
        assert e.value.code == code, args
    f(plans, [A, A], one * 4, None, 2, O2, 0)                                # batch = 0 writes nothing
    assert (_u64(o2) == U64(FILL)).all()
    f(plans, [A, A], one * 4, None, 2, O2, 2)                                # and the accepted call writes every word: a + a
    assert np.array_equal(_u64(o2)[0], np.stack([E.padd(q, _u64(a)[i], _u64(a)[i]) for i, q in enumerate(mods)]))


# ---- the launch counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_launch_counts(pkg, k):
    import torch

    B = pkg.binding
    n, batch = 64, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    a = _dev(E.case_ct(mods, n, batch, 2, 9))
    out = _empty((5, k, 2, batch, n))
    labels = ("tensor", "lift", "keymac", "divround", "galois", "diagmac", "lincomb")

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

    zero = dict.fromkeys(labels, 0)
    for count in (1, PN.GROUP, PN.GROUP + 1, 33):
        for outputs in (1, 4, 5):
            got = counts(lambda: B.ckks_rns_lincomb_dev(plans, [a.data_ptr()] * count, [1] * (outputs * count * k), None, outputs, out.data_ptr(), batch))
            assert got == dict(zero, lincomb=PN.launch_counts(k, count, outputs)), (k, count, outputs)
    # §22's and §24's counts are as they were
    key = _dev(np.random.default_rng(10).integers(0, 1 << 39, (k, k + 1, 2, n), dtype=np.uint64))
    got = counts(lambda: B.ckks_rns_mul_dev(plans, sp, key.data_ptr(), k, a.data_ptr(), a.data_ptr(), out[0].data_ptr(), batch))
    assert got == dict(zero, tensor=k, lift=k + 1, keymac=k + 1, divround=k)
    if k > 1:
        got = counts(lambda: B.ckks_rns_rescale_dev(plans, a.data_ptr(), out[0].data_ptr(), batch))
        assert got == dict(zero, lift=1, divround=k - 1)
    d_pts = _dev(np.random.default_rng(3).integers(0, 1 << 39, (2, 3, k + 1, n), dtype=np.uint64))
    got = counts(lambda: B.ckks_rns_diag_sum_dev(plans, sp, [key.data_ptr()] * 3, [5, 25, 2 * n - 1], k, d_pts.data_ptr(), 2, a.data_ptr(), out.data_ptr(), batch))
    assert got == dict(zero, **LN.launch_counts(k, 3, 2, 1))


# ---- the Python surface and eval_chebyshev ---------------------------------------------------------------------------------------------------
def _setup(pkg, n, rows, rng):
    ck = pkg.ckks
    mods, P = E.chain(n, 58, 40, 7)
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(PN.SEED, param, PN.DELTA)
    return ck, mods, P, param, key


def test_python_surface(pkg):
    ck, mods, P, param, key = _setup(pkg, 16, 2, 1)
    n = 16
    z = np.random.default_rng(5).uniform(-1, 1, (2, n // 2)).astype(np.complex128)
    pk = key.public_key(0)
    x, y = key.encode_and_encrypt(pk, z), key.encode_and_encrypt(pk, 0.5 * z)
    xw, yw = _u64(x.d), _u64(y.d)

    def want(cts, scales, coeffs, consts, S, level):
        w, k, _, _ = PN.weights(coeffs, consts, S, scales, mods[:level + 1])
        return PN.lincomb(mods[:level + 1], cts, w, k)

    # integers at the largest input scale; real coefficients at a target scale; a level below the inputs'
    outs = ck.lincomb([x, y], [[2, -1], [0, 3]], consts=[0.25, -1.5])
    assert [(o.level, o.scale) for o in outs] == [(7, PN.DELTA)] * 2
    assert np.array_equal(np.stack([_u64(o.d) for o in outs]), want([xw, yw], [PN.DELTA] * 2, [[2, -1], [0, 3]], [0.25, -1.5], PN.DELTA, 7))
    S = PN.DELTA * mods[5]
    low = ck.lincomb([x, y.at_level(6)], [0.3, -0.7], consts=[0.1], scale=S, level=5)[0]
    assert (low.level, low.scale, low.batch) == (5, S, 2)
    assert np.array_equal(_u64(low.d), want([xw, yw], [PN.DELTA] * 2, [[0.3, -0.7]], [0.1], S, 5)[0])
    dec = key.decrypt_and_decode(low.rescale())
    assert np.abs(dec - (0.3 * z - 0.35 * z + 0.1)).max() < 1e-6
    # a target per output
    two = ck.lincomb([x], [[1.0], [0.5]], scale=[PN.DELTA, S], level=5)
    assert [t.scale for t in two] == [PN.DELTA, S]
    assert np.array_equal(_u64(two[1].d), want([xw], [PN.DELTA], [[0.5]], None, S, 5)[0])
    # the thin forms
    assert np.array_equal(_u64((-x).d), want([xw], [PN.DELTA], [[-1]], None, PN.DELTA, 7)[0]) and (-x).scale == x.scale
    assert np.array_equal(_u64(x.add_const(0.75).d), want([xw], [PN.DELTA], [[1]], [0.75], PN.DELTA, 7)[0])
    assert np.array_equal(_u64(x.mul_const(3).d), want([xw], [PN.DELTA], [[3]], None, PN.DELTA, 7)[0])
    h = x.mul_const(0.37, scale=PN.DELTA * mods[7])
    assert h.scale == PN.DELTA * mods[7] and np.array_equal(_u64(h.d), want([xw], [PN.DELTA], [[0.37]], None, PN.DELTA * mods[7], 7)[0])
    assert np.abs(key.decrypt_and_decode(x.add_const(0.75)) - (z + 0.75)).max() < 1e-6
    # T_2 = 2 x^2 - 1 and 2 T_a T_b - T_c on the unrescaled product: no level is used by the sum
    rlk = key.relin_key(0)
    prod = x.mul(x, rlk)
    t2 = ck.lincomb([prod], [2], consts=[-1], scale=prod.scale)[0]
    assert (t2.level, t2.scale) == (7, prod.scale)
    t2 = t2.rescale()
    prod3 = t2.mul(x, rlk)
    t3 = ck.lincomb([prod3, x], [2, -1], scale=prod3.scale)[0]
    assert (t3.level, t3.scale) == (6, prod3.scale)
    w3, _, big, _ = PN.weights([[2, -1]], None, prod3.scale, [prod3.scale, x.scale], mods[:7])
    assert big[0][0] == 2 and np.array_equal(_u64(t3.d), PN.lincomb(mods[:7], [_u64(prod3.d), xw], w3)[0])
    zr = z.real
    assert np.abs(key.decrypt_and_decode(t3.rescale()) - (4 * zr ** 3 - 3 * zr)).max() < 1e-6
    with pytest.raises(ValueError):                                          # the scales differ: + refuses what lincomb does
        prod3 + x
    with _refused():
        ck.lincomb([x, ck.RnsCiphertext(ck.RnsParam(n, mods[:2], P), x.d, 1, 1.0)], [1, 1])
    with pytest.raises(ValueError, match="constant polynomial"):
        ck.lincomb([x], [1j])


@pytest.mark.parametrize("name", list(PN.FUNCTIONAL))
def test_eval_chebyshev_is_the_replay_of_its_plan(pkg, name):
    case = PN.FUNCTIONAL[name]
    n = case["n"]
    ck, mods, P, param, key = _setup(pkg, n, case["rows"], 2)
    z, coeffs = PN.functional_slots(case), PN.functional_coeffs(case)
    ct = key.encode_and_encrypt(key.public_key(0), z)
    rlk = key.relin_key(0)
    plan = ck.ChebyshevPlan.build(coeffs, case["interval"])
    res = ct.eval_chebyshev(plan, rlk)
    wires = PN.replay(plan, _u64(ct.d), ct.scale, 7, mods, P, _u64(rlk.d_rlk))
    words, level, scale = wires[plan.result]
    assert (res.level, res.scale) == (level, scale) == (7 - plan.levels, scale)
    assert np.array_equal(_u64(res.d), words)                                # tolerance zero
    again = ct.eval_chebyshev(coeffs, rlk, interval=case["interval"])        # from the coefficients: the same plan, the same words
    assert np.array_equal(_u64(again.d), words)
    d = key.decrypt(res)
    got = K.decode(d, scale)
    assert np.array_equal(key.decrypt_and_decode(res), key.encoder.decode(d, scale))
    a, b = case["interval"]
    want = Ch.chebval((2 * z.real - a - b) / (b - a), coeffs)
    bound = PN.poly_bounds(plan, n, mods, 7, PN.DELTA, max(abs(a), abs(b)))[0] + float(K.e_dec(d, scale).max())
    err = float(np.abs(got - want).max())
    print(f"{name}: n={n} degree {case['degree']}: worst slot error {err:.3e}, derived bound {bound:.3e}")
    assert err <= bound < 2.0 ** -10


def test_too_few_levels_are_refused_before_any_launch(pkg):
    import torch

    ck, mods, P, param, key = _setup(pkg, 16, 2, 3)
    B = pkg.binding
    ct = key.encode_and_encrypt(key.public_key(0), np.zeros((1, 8), dtype=np.complex128))
    plan = ck.ChebyshevPlan.build(np.ones(8))
    torch.cuda.synchronize()
    B.kernel_timing_enable(True)
    B.kernel_timing_reset()
    try:
        with pytest.raises(ValueError, match="4 levels"):
            ck.RnsCiphertext(param, ct.d[:4].contiguous(), 3, ct.scale).eval_chebyshev(plan, None)
        torch.cuda.synchronize()
        got = B.kernel_timing_read(256)
    finally:
        B.kernel_timing_enable(False)
    assert not any(name.startswith("ckks_rns_") for name in got)
    assert ck.RnsCiphertext(param, ct.d[:5].contiguous(), 4, ct.scale).eval_chebyshev(plan, key.relin_key(1)).level == 0
