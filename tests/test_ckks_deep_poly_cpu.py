"""Scalar sums, inner products and Chebyshev plans on the deep CKKS chain without a device: the restated dot
(tests/_ckks_deep_poly_numpy.py) at alpha = 1 equals §29's word for word; relin(sum_r w_r a_r (x) b_r) is off sum_r w_r dec(a_r)
dec(b_r) by ONE switch error under §36's bound, whatever the count; the kernels' order of operations stays under the 128-bit
bound they claim on bound-reaching words; the launch formulas against the partition; the rejections of both entry points with
fake addresses and of the Python surface; the NotImplementedErrors that stay; the plan runner against plan.simulate; the host
partition's own program."""
import os
import re
import subprocess

import numpy as np
import pytest

import _ckks_deep_numpy as D
import _ckks_deep_poly_numpy as DP
import _ckks_dot_numpy as DT
import _ckks_eval_numpy as E
import _ckks_numpy as K
import _ckks_poly_numpy as PN
import _client_numpy as C

U64 = np.uint64
SEED = bytes((7 * i + 39) % 256 for i in range(32))


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


# ---- alpha = 1 is §29 word for word; the scalar sum is §27's ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch,count", [(4, 1, 1, 1), (16, 3, 3, 5), (8, 8, 2, 17)])
def test_alpha_one_dot_is_the_single_digit_restatement(tab, n, k, batch, count):
    mods, P = E.chain(n, 58, 40, k - 1)
    s = K.secret_key(SEED, 0, n)
    rlk = E.relin_key(SEED, E.RLK_BASE, s, mods, P, tab)
    cts = [E.case_ct(mods, n, batch, 2, 100 * n + r) for r in range(count + 1)]
    pairs = [(cts[r], cts[r + 1]) for r in range(count - 1)] + [(cts[0], cts[0])]       # a square among them, operands repeated
    for w in (None, DP.random_dot_weights(mods, count, 7)):
        assert np.array_equal(DP.tensor_sum(mods, pairs, w), DT.tensor_sum(mods, pairs, w))
        assert np.array_equal(DP.dot(mods, [P], rlk, pairs, w), DT.dot(mods, P, rlk, pairs, w))
        assert np.array_equal(DP.dot(mods, [P], rlk, pairs, w), E.relinearize(mods, P, rlk, DP.tensor_sum(mods, pairs, w)))
    w, kk = DP.random_lin_weights(mods, 3, count + 1, 8)
    assert np.array_equal(DP.lincomb(mods, cts, w, kk), PN.lincomb(mods, cts, w, kk))
    assert np.array_equal(DP.dot(mods, [P], rlk, pairs[:1]), D.mul(mods, [P], rlk, *pairs[0]))   # one pair, no weight: the product


# ---- the noise statement ------------------------------------------------------------------------------------------------------------------
def _phase_product(mods, n, s, a, b):
    """dec(a) dec(b) over the integers, one row: the negacyclic product of the centred phases"""
    pa, _ = E.phase_int(mods, n, s, a)
    pb, _ = E.phase_int(mods, n, s, b)
    return E.negacyclic_int(pa, [int(x) for x in pb[0]])


@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("L,alpha", [(5, 2), (9, 3)])
def test_a_dot_carries_one_switch_error_whatever_the_count(tab, L, alpha, count):
    """a real ternary secret, public key, relinearisation key and table errors at n = 8"""
    n = 8
    mods, specials = D.case_chain(n, L, alpha)
    s = K.secret_key(SEED, 0, n)
    assert np.abs(s).max() <= 1
    pk = E.public_key(SEED, E.PK_BASE, s, mods, tab)
    rlk = D.switch_key(SEED, E.RLK_BASE, s, mods, specials, tab)
    rng = np.random.default_rng(39 + L)
    cts = [E.encrypt(SEED, r, pk, rng.integers(-1 << 30, 1 << 30, (1, n)), 1, mods, tab) for r in range(2 * count)]
    pairs = [(cts[2 * r], cts[2 * r + 1]) for r in range(count)]
    bound = D.switch_noise_bound(n, L, alpha, max(D.product(mods[i] for i in g) for g in D.groups(L, alpha)) / D.product(specials))
    for big in (None, [3, -2, 1, 5, -7][:count]):
        w = None if big is None else [[x % q for q in mods] for x in big]
        got, Q = E.phase_int(mods, n, s, DP.dot(mods, specials, rlk, pairs, w))
        want = sum((1 if big is None else big[r]) * _phase_product(mods, n, s, a, b) for r, (a, b) in enumerate(pairs))
        eps = (got - want) % Q
        eps = np.where(eps > Q // 2, eps - Q, eps)
        print(f"L={L} alpha={alpha} count={count} weighted={big is not None}: |eps| = {int(np.abs(eps).max())}, bound {bound}")
        assert int(np.abs(eps).max()) <= bound


# ---- the accumulators' overflow argument on bound-reaching words ----------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 8, 9, 16, 17, 64])
def test_accumulators_stay_under_their_bound_at_the_edges(count):
    """every word and weight q - 1 for the largest admissible prime, at the full fold period: the bound the kernels' comments
    claim is asserted inside accumulate_*, and the words are the definition's"""
    q = E.primes_below(62, 8, 1)[0]
    assert q < 1 << 62 and (1 << 62) - q < 1 << 10
    top = q - 1
    assert DP.accumulate_lincomb(q, [top] * count, [top] * count, top) == (top + count * top * top) % q
    words = [(top, top, top, top)] * min(count, DP.DOT_MAX_COUNT)
    for ws in (None, [top] * len(words)):
        wv = 1 if ws is None else top
        assert DP.accumulate_tensorsum(q, words, ws) == tuple(m * len(words) * wv * top * top % q for m in (1, 2, 1))
    # a longer period breaks the bound: the test can tell the periods apart
    with pytest.raises(AssertionError):
        DP.accumulate_lincomb(q, [top] * 17, [top] * 17, top, group=64, period=17)
    with pytest.raises(AssertionError):
        DP.accumulate_tensorsum(q, [(top, top, top, top)] * 9, None, period=9)


# ---- the launches -----------------------------------------------------------------------------------------------------------------------------
def test_launch_formulas_against_the_partition():
    for limbs in (1, 7, 8, 9, 16, 17, 24, 32):
        for outputs in (1, 4, 5, 16):
            for count in (1, 8, 9, 15, 17, 64):
                part = DP.lincomb_partition(limbs, outputs, count)
                assert len(part) == DP.lincomb_launches(limbs, outputs, count) == -(-limbs // 8) * -(-outputs // 4) * -(-count // 8)
                seen = set()
                for o0, no, i0, nl, r0, nr in part:
                    assert 1 <= no <= DP.OUT_CAP and 1 <= nl <= DP.SLICE and 1 <= nr <= DP.LIN_INPUTS
                    cells = {(o, i, r) for o in range(o0, o0 + no) for i in range(i0, i0 + nl) for r in range(r0, r0 + nr)}
                    assert not cells & seen
                    seen |= cells
                assert len(seen) == limbs * outputs * count
        for count in (1, 4, 16, 17, 64):
            assert DP.tensorsum_launches(limbs, count) == -(-limbs // 8) * -(-count // 16)
    assert DP.lincomb_launches(24, 4, 15) == 6 and DP.tensorsum_launches(24, 16) == 3 and DP.tensorsum_launches(32, 64) == 16
    assert DP.dot_launch_counts(24, 3, 16) == dict(tensorsum=3, tensor=0, extend=9, keymac=27, divround=24)


def test_host_partition_against_its_definition(pkg):
    """csrc/rns_tables.hpp's deep_lincomb_each / deep_lincomb_words / deep_tensorsum_each / deep_tensorsum_words against their
    definitions: fhe-study_amd/host/test_deep_poly.cpp, which needs neither the library nor a GPU"""
    from conftest import ROOT

    host = os.path.join(ROOT, "fhe-study_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_deep_poly"])
    r = subprocess.run([os.path.join(host, "test_deep_poly")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all deep poly partition tests passed" in r.stdout


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------------
def test_boundary(pkg):
    from conftest import ROOT

    B = pkg.binding
    h = open(os.path.join(ROOT, "include", "fhe_ntt.h")).read()
    lib = pkg.load_library()
    for name in ("fhe_ckks_deep_lincomb_dev", "fhe_ckks_deep_dot_dev"):
        assert re.search(r"\bint\s+" + name + r"\(", h) and name in B.EXPORTS and hasattr(lib, name)
    assert callable(B.ckks_deep_lincomb_dev) and callable(B.ckks_deep_dot_dev) and callable(pkg.ckks.eval_chebyshev)
    assert (B.FHE_CKKS_LINCOMB_MAX_COUNT, B.FHE_CKKS_LINCOMB_MAX_OUTPUTS, B.FHE_CKKS_DOT_MAX_COUNT) == (DP.MAX_COUNT, DP.MAX_OUTPUTS, DP.DOT_MAX_COUNT)
    mk = open(os.path.join(ROOT, "fhe-study_amd", "host", "Makefile")).read()
    assert "san_deep_poly:" in mk and "test_deep_poly:" in mk
    # the dot takes mul's workspace: the size query is what it was
    for n, l, a, b in ((8, 32, 8, 1), (8192, 12, 4, 2), (4096, 8, 1, 1024), (64, 17, 8, 3), (2, 1, 1, 1)):
        assert B.ckks_deep_workspace_bytes(n, l, a, b) == D.workspace_bytes(n, l, a, b) > 0


# ---- rejections that need no device ---------------------------------------------------------------------------------------------------------------
def test_lincomb_rejections_without_a_device(pkg):
    B = pkg.binding
    n, L = 16, 9
    mods = E.primes_below(40, n, L)
    plans = [pkg.Plan(q, n) for q in mods]
    other = pkg.Plan(E.primes_below(40, 32, 1)[0], 32)
    wide = pkg.Plan(E.primes_below(63, n, 1)[0], n)
    a, b, out = 0x10000, 0x40000, 0x400000
    ct_bytes = L * 2 * n * 8
    one = [1] * L

    def code(*args, **kw):
        with pytest.raises(B.FheError) as e:
            B.ckks_deep_lincomb_dev(*args, **kw)
        return e.value.code

    assert code(None, [a], one, None, 1, out, 1, limbs=L) == B.FHE_E_NULL
    assert code(plans[:4] + [None] + plans[5:], [a], one, None, 1, out, 1) == B.FHE_E_NULL
    assert code(plans, None, one, None, 1, out, 1, count=1) == B.FHE_E_NULL
    assert code(plans, [a], None, None, 1, out, 1) == B.FHE_E_NULL
    assert code(plans, [a, None], one * 2, None, 1, out, 1) == B.FHE_E_NULL
    assert code(plans, [a], one, None, 1, None, 1) == B.FHE_E_NULL
    assert code(plans[:8] + [other], [a], one, None, 1, out, 1) == B.FHE_E_PARAM_MISMATCH
    assert code(plans[:8] + plans[:1], [a], one, None, 1, out, 1) == B.FHE_E_INVALID                   # a repeated prime
    assert code(plans[:8] + [wide], [a], one, None, 1, out, 1) == B.FHE_E_INVALID                      # a prime of 2^62 or more
    assert code([], [a], [], None, 1, out, 1) == B.FHE_E_INVALID                                       # limbs = 0, and 33
    assert code(plans * 4, [a], one * 4, None, 1, out, 1, limbs=33) == B.FHE_E_INVALID
    assert code(plans, [], [], None, 1, out, 1) == B.FHE_E_INVALID                                     # count = 0, and 65
    assert code(plans, [a] * 65, one * 65, None, 1, out, 1) == B.FHE_E_INVALID
    assert code(plans, [a], one, None, 0, out, 1) == B.FHE_E_INVALID                                   # outputs = 0, and 17
    assert code(plans, [a], one * 17, None, 17, out, 1) == B.FHE_E_INVALID
    for i in (0, 7, 8):                                                                                # a weight, a constant at its modulus: both slices
        w = list(one)
        w[i] = mods[i]
        assert code(plans, [a], w, None, 1, out, 1) == B.FHE_E_INVALID
        assert code(plans, [a], one, w, 1, out, 1) == B.FHE_E_INVALID
    assert code(plans, [a, b], one * 4, [0] * L + [0] * (L - 1) + [mods[-1]], 2, out, 1) == B.FHE_E_INVALID
    assert code(plans, [out], one, None, 1, out, 1) == B.FHE_E_INVALID                                 # the output overlaps an input
    assert code(plans, [a, out + 2 * ct_bytes - 8], one * 4, None, 2, out, 1) == B.FHE_E_INVALID
    assert code(plans, [a, out - ct_bytes + 8], one * 2, None, 1, out, 1) == B.FHE_E_INVALID
    assert code(plans, [a + 4], one, None, 1, out, 1) == B.FHE_E_INVALID
    assert code(plans, [a], one, None, 1, out + 4, 1) == B.FHE_E_INVALID
    assert code(plans, [a], one, None, 1, out, 1 << 58) == B.FHE_E_INVALID                             # batch too large
    # batch = 0 is a no-op after the host checks, whatever the buffers
    B.ckks_deep_lincomb_dev(plans, [None], one, None, 1, None, 0)
    B.ckks_deep_lincomb_dev(plans, [out], one, one, 1, out, 0)
    assert code(plans, [out], [mods[0]] + one[1:], None, 1, out, 0) == B.FHE_E_INVALID


def test_dot_rejections_without_a_device(pkg):
    B = pkg.binding
    n, L, alpha = 16, 9, 3
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = [pkg.Plan(q, n) for q in mods], [pkg.Plan(p, n) for p in sps]
    other = pkg.Plan(E.primes_below(40, 32, 1)[0], 32)
    wide = pkg.Plan(E.primes_below(63, n, 1)[0], n)
    low = [pkg.Plan(p, n) for p in E.primes_below(39, n, alpha)]
    key, a, b, out = 0x10000, 0x100000, 0x200000, 0x400000
    ct_bytes = L * 2 * n * 8
    key_bytes = D.dnum(L, alpha) * (L + alpha) * 2 * n * 8

    def code(plans=plans, sp=sp, key=key, kl=L, xs=(a,), ys=(b,), w=None, out=out, batch=1, **kw):
        with pytest.raises(B.FheError) as e:
            B.ckks_deep_dot_dev(plans, sp, key, kl, None if xs is None else list(xs), None if ys is None else list(ys), w, out, batch, **kw)
        return e.value.code

    assert code(plans=None, limbs=L) == B.FHE_E_NULL and code(plans=plans[:3] + [None] + plans[4:]) == B.FHE_E_NULL
    assert code(sp=None, alpha=alpha) == B.FHE_E_NULL and code(sp=[sp[0], None, sp[2]]) == B.FHE_E_NULL
    assert code(plans=[], xs=(a,)) == B.FHE_E_INVALID and code(plans=plans * 4, limbs=33) == B.FHE_E_INVALID
    assert code(alpha=0) == B.FHE_E_INVALID and code(sp=sp * 3, alpha=9) == B.FHE_E_INVALID
    assert code(plans=plans[:8] + [other]) == B.FHE_E_PARAM_MISMATCH and code(sp=sp[:2] + [other]) == B.FHE_E_PARAM_MISMATCH
    assert code(plans=plans[:8] + plans[:1]) == B.FHE_E_INVALID and code(sp=sp[:2] + plans[:1]) == B.FHE_E_INVALID
    assert code(plans=plans[:8] + [wide]) == B.FHE_E_INVALID and code(sp=sp[:2] + [wide]) == B.FHE_E_INVALID
    assert code(sp=low) == B.FHE_E_INVALID                                                             # a missed admission
    assert code(kl=L - 1) == B.FHE_E_INVALID and code(kl=33) == B.FHE_E_INVALID
    assert code(xs=(), ys=()) == B.FHE_E_INVALID and code(xs=(a,) * 65, ys=(b,) * 65) == B.FHE_E_INVALID
    assert code(xs=None, count=1) == B.FHE_E_NULL and code(ys=None) == B.FHE_E_NULL
    for i in (0, 7, 8):
        w = [1] * L
        w[i] = mods[i]
        assert code(w=w) == B.FHE_E_INVALID
    assert code(xs=(a, a), ys=(b, b), w=[1] * L + [1] * (L - 1) + [mods[-1]]) == B.FHE_E_INVALID
    assert code(batch=1 << 58) == B.FHE_E_INVALID
    assert code(key=None) == B.FHE_E_NULL and code(out=None) == B.FHE_E_NULL
    assert code(key=key + 4) == B.FHE_E_INVALID and code(out=out + 4) == B.FHE_E_INVALID
    assert code(out=key) == B.FHE_E_INVALID and code(out=key + key_bytes - 8) == B.FHE_E_INVALID
    assert code(xs=(a, None), ys=(b, b)) == B.FHE_E_NULL and code(xs=(a, a), ys=(b, None)) == B.FHE_E_NULL
    assert code(xs=(a + 4,)) == B.FHE_E_INVALID and code(ys=(b + 4,)) == B.FHE_E_INVALID
    assert code(xs=(out,)) == B.FHE_E_INVALID and code(ys=(out + ct_bytes - 8,)) == B.FHE_E_INVALID
    assert code(xs=(a, out - ct_bytes + 8), ys=(b, b)) == B.FHE_E_INVALID
    # batch = 0 is a no-op after the host checks
    B.ckks_deep_dot_dev(plans, sp, None, L, [None], [None], None, None, 0)
    assert code(w=[mods[0]] + [1] * (L - 1), batch=0) == B.FHE_E_INVALID


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------------
def test_python_surface_without_a_device(pkg):
    ck = pkg.ckks
    n, L, alpha = 16, 9, 3
    mods, sps = D.case_chain(n, L, alpha)
    param = ck.DeepParam(n, mods, sps)

    class Rows:                                                               # the shape of a device tensor, without one
        shape = (L, 2, 2, n)
    ct = ck.DeepCiphertext(param, Rows(), L - 1, 2.0 ** 40)
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
        ck.lincomb([ct], [1.0], level=L)
    with pytest.raises(ValueError):
        ck.lincomb([ct], [1.0], scale=0.0)
    # mixing the deep chain with the plain one, or two deep chains, is the existing mismatch
    rns = ck.RnsCiphertext(ck.RnsParam(n, mods[:3], sps[0]), Rows(), 2, 2.0 ** 40)
    short = ck.DeepCiphertext(ck.DeepParam(n, mods[:4], sps), Rows(), 3, 2.0 ** 40)
    rlk = ck.RnsRelinKey(param, None)
    for mixed in ([ct, rns], [rns, ct], [ct, short]):
        with pytest.raises(pkg.binding.FheError) as e:
            ck.lincomb(mixed, [1.0, 1.0])
        assert e.value.code == pkg.binding.FHE_E_PARAM_MISMATCH
        with pytest.raises(pkg.binding.FheError) as e:
            ck.dot(mixed[:1], mixed[1:], rlk)
        assert e.value.code == pkg.binding.FHE_E_PARAM_MISMATCH
    with pytest.raises(pkg.binding.FheError) as e:
        ck.dot([ct], [ct], ck.RnsRelinKey(short.param, None))
    assert e.value.code == pkg.binding.FHE_E_PARAM_MISMATCH
    with pytest.raises(ValueError):
        ck.dot([], [], rlk)
    with pytest.raises(ValueError):
        ck.dot([ct], [ct, ct], rlk)
    with pytest.raises(ValueError):
        ck.dot([ct], [ct], rlk, coeffs=[1.0, 2.0])
    with pytest.raises(ValueError):
        ck.dot([ct], [ct], rlk, level=L)
    plan = ck.ChebyshevPlan.build(np.ones(16), (-4, 4))
    with pytest.raises(ValueError, match=f"{plan.levels} levels"):            # refused before anything runs
        ck.eval_chebyshev(ck.DeepCiphertext(param, Rows(), 2, 2.0 ** 40), plan, rlk)
    with pytest.raises(ValueError, match="levels"):
        ck.eval_chebyshev(ck.DeepCiphertext(param, Rows(), 1, 2.0 ** 40), np.ones(8), rlk)
    # the method sugar keeps raising, as the tests of §36 and §37 assert; __neg__ is as it was
    for call in (lambda: ct.mul_const(2.0), lambda: ct.add_const(1.0), lambda: ct.eval_chebyshev(np.ones(4), rlk), lambda: ct.linear_transform_hoisted(None, None)):
        with pytest.raises(NotImplementedError):
            call()
    assert ck.DeepCiphertext.__neg__ is not ck.RnsCiphertext.__neg__
    assert "NotImplementedError" in ck.DeepCiphertext.__doc__


# ---- the plan runner ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", [(-1.0, 1.0), (-2.0, 2.0)])
def test_plan_runner_against_simulate_on_small_integers(pkg, interval):
    """A noiseless ciphertext (c0 the constant polynomial round(Delta x), c1 = 0) of the integers x in the interval, integer
    Chebyshev coefficients of degree 7, n = 8 on a chain of 7 limbs: c1 = 0 makes every d2 zero, so the key switch adds nothing
    and the words are the plan's arithmetic alone.  Every lincomb weight and every rescale rounds once, by at most 1/2 a unit of
    a scale of about 2^40, times coefficients below 2^5 over fewer than 2^6 operations: under 2^-28 in all."""
    ck = pkg.ckks
    n, L, alpha, delta = 8, 7, 2, 2.0 ** 40
    mods, sps = D.e2e_chain(n, L, alpha)
    coeffs = [3, -2, 1, 4, -1, 2, -3, 1]
    plan = ck.ChebyshevPlan.build(coeffs, interval)
    assert plan.levels <= L - 1
    xs = np.arange(int(interval[0]), int(interval[1]) + 1)
    rlk = np.zeros((D.dnum(L, alpha), L + alpha, 2, n), dtype=U64)             # never meets a non-zero digit
    ct = np.zeros((L, 2, len(xs), n), dtype=U64)
    for i, q in enumerate(mods):
        ct[i, 0] = np.array([[int(round(delta * x)) % q] * n for x in xs], dtype=U64)   # a constant polynomial: every eval the constant
    w = DP.replay(plan, ct, delta, L - 1, mods, sps, rlk)
    words, level, scale = w[plan.result]
    assert level == L - 1 - plan.levels and abs(scale - delta) <= 1e-9 * delta
    assert not words[:, 1].any()
    got = K.centre(E.inv(mods[0], n, words[0, 0]), mods[0])
    assert not got[:, 1:].any()                                              # still constant polynomials
    err = np.abs(got[:, 0] / scale - plan.simulate(xs.astype(np.float64)))
    print(f"interval {interval}: |replay - simulate| = {float(err.max()):.3e}")
    assert float(err.max()) <= 2.0 ** -28
