"""BFV inner products, scalar sums and linear transforms on the RNS chain without a device: the route of
fhe_bfv_rns_dot_dev restated in Python integers (tests/_bfv_dot_numpy.py) against the integer definition, the admission
B > t n Q W + 1 one either side of its boundary, RnsParam.max_dot_weight, the diagonal and baby-step giant-step identities on
2 x n/2 slots in plain numpy, the residues lincomb hands the device, and the stand-alone program of the admission arithmetic."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _bfv_dot_numpy as D
import _bfv_rns_numpy as R
import _ckks_eval_numpy as E

T = 65537
N = 4                            # the route is per coefficient: the ring only has to make the negacyclic sums wrap


def _pairs(kind, rng, Q, n, count, w):
    if kind == "random":
        return [D.random_pair(rng, Q, n) for _ in range(count)]
    if kind in ("top", "bottom"):    # D reaches +W n Q^2 / 2 (bottom: -W n Q^2 / 2) to the rounding of floor(Q / 2)
        sign = 1 if kind == "top" else -1
        return [D.bound_pair(Q, n, sign * (1 if w is None or w[r] > 0 else -1)) for r in range(count)]
    raise AssertionError(kind)


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("count", [1, 2, 5, 9])
def test_route_equals_definition(k, count):
    """per pair: extend, tensor modulo every prime of Q u B, weighted accumulate into canonical words; then §33's scale once"""
    mods, aux, _ = R.chain(N, k)
    Q = R.prod(mods)
    rng = random.Random(100 * k + count)
    signed = D.signed_weights(count, T, count)
    for w in (None, [1] * count, signed):
        W = D.weight_sum(count, w)
        assert D.admitted(mods, aux, T, N, W)
        for kind in ("random", "top", "bottom"):
            pairs = _pairs(kind, rng, Q, N, count, w)
            Dint = D.sum_int(pairs, w)
            assert all(abs(x) <= W * N * Q * Q // 2 for comp in Dint for x in comp)
            if kind != "random":                                     # the bound is reached: 2 n floor(Q / 2)^2 a unit of weight
                assert Dint[1][N - 1] == (1 if kind == "top" else -1) * W * 2 * N * (Q // 2) ** 2
            got = D.route_dot(mods, aux, T, pairs, w)
            for i, q in enumerate(mods):
                for c in range(3):
                    assert got[i][c] == [R.scale_round(x, T, Q) % q for x in Dint[c]], (kind, w, i, c)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_route_where_the_sum_vanishes(k):
    mods, aux, _ = R.chain(N, k)
    Q = R.prod(mods)
    rng = random.Random(k)
    p, z = D.random_pair(rng, Q, N), tuple([0] * N for _ in range(4))
    for pairs, w in (([z], None), ([p, p], [1, -1]), ([p, p, p], [T // 2, -(T // 2 - 1), -1]), ([D.bound_pair(Q, N, 1), D.bound_pair(Q, N, -1)], None)):
        assert D.sum_int(pairs, w) == [[0] * N] * 3
        got = D.route_dot(mods, aux, T, pairs, w)
        assert all(got[i][c] == [0] * N for i in range(k) for c in range(3))


@pytest.mark.parametrize("k", [1, 2, 4])
def test_scale_once_on_multiples_of_q(k):
    """D = m Q + {0, 1, floor(Q / 2), floor(Q / 2) + 1} and their negatives, up to the bound W n Q^2 / 2 of W = 64 weights of
    t / 2: the one rounding of the summed tensor"""
    mods, aux, _ = R.chain(N, k)
    Q = R.prod(mods)
    W = 64 * (T // 2)
    assert D.admitted(mods, aux, T, N, W) and W <= D.max_weight(mods, aux, T, N)
    top = W * N * Q * Q // 2
    rng = random.Random(7 + k)
    ms = [0, 1, 2, top // Q - 1] + [rng.randrange(top // Q) for _ in range(8)]
    for m in ms:
        for off in (0, 1, Q // 2, Q // 2 + 1):
            for d in (m * Q + off, -(m * Q + off)):
                assert abs(d) <= top
                got = D.route_scale_residues(mods, aux, T, [d % q for q in mods], [d % b for b in aux])
                assert got == [R.scale_round(d, T, Q) % q for q in mods], (m, off, d < 0)
    for d in (top, -top):
        got = D.route_scale_residues(mods, aux, T, [d % q for q in mods], [d % b for b in aux])
        assert got == [R.scale_round(d, T, Q) % q for q in mods]


def _edge_base(n=64, k=2, boundary=7):
    """a chain and a t for which the largest admitted W is exactly `boundary`: t = floor(floor((B - 2) / (n Q)) / boundary)"""
    mods, aux, P = R.chain(n, k, bq=40, bb=41)
    t = (R.prod(aux) - 2) // (n * R.prod(mods)) // boundary
    return mods, aux, P, t


def test_admission_one_either_side(pkg):
    n, k = 64, 2
    mods, aux, P, t = _edge_base(n, k, 7)
    wb = D.max_weight(mods, aux, t, n)
    assert wb == 7 and 2 <= wb <= D.MAX_COUNT
    assert D.admitted(mods, aux, t, n, wb) and not D.admitted(mods, aux, t, n, wb + 1)
    assert R.admitted(mods, aux, t, n)                               # the base admits `mul`
    bfv = pkg.bfv
    param = bfv.RnsParam(n, mods, aux, P, t)
    assert param.max_dot_weight == wb
    assert bfv.dot_weights(param, 7) == (None, 7)
    assert bfv.dot_weights(param, 2, [3, -4]) == ([3, -4], 7)
    assert bfv.dot_weights(param, 2, [3, t - 4]) == ([3, -4], 7)     # centred modulo t
    assert bfv.dot_weights(param, 3, [1, 1, 1]) == (None, 3)
    for count, w in ((8, None), (2, [4, -4]), (8, [1] * 8)):
        with pytest.raises(ValueError) as e:
            bfv.dot_weights(param, count, w)
        assert "W = 8" in str(e.value) and "at most W = 7" in str(e.value)
    with pytest.raises(ValueError):
        bfv.dot_weights(param, 2, [1, t])                            # zero modulo t
    with pytest.raises(ValueError):
        bfv.dot_weights(param, 2, [1])


@pytest.mark.parametrize("n,k,t", [(64, 2, 257), (8192, 3, 65537), (2, 1, 5), (2048, 4, 65537)])
def test_max_dot_weight(pkg, n, k, t):
    mods, aux, P = R.chain(n, k)
    param = pkg.bfv.RnsParam(n, mods, aux, P, t)
    W = param.max_dot_weight
    assert W == D.max_weight(mods, aux, t, n) == (param.B - 2) // (t * n * param.Q) >= 1
    assert param.B > t * n * param.Q * W + 1 and not param.B > t * n * param.Q * (W + 1) + 1


# ---- diagonals and baby-step giant-step on 2 x n/2 slots -------------------------------------------------------------------------------
def _matrices(rng, N, t):
    dense = rng.integers(0, t, (2, N, N))
    return {
        "dense": dense,                                              # two different row matrices
        "one": rng.integers(0, t, (N, N)),                           # one matrix for both rows
        "banded": np.stack([D.banded(rng, N, t, 3), D.banded(rng, N, t, 2)]),
        "single": np.stack([D.single_diagonal(rng, N, t, 5 % N), D.single_diagonal(rng, N, t, 5 % N)]),
        "single_and_zero": np.stack([D.single_diagonal(rng, N, t, N - 1), np.zeros((N, N), dtype=np.int64)]),
        "negative": dense - t,                                       # entries outside [0, t) are taken modulo t
    }


@pytest.mark.parametrize("n,t", [(16, 97), (64, 257)])
def test_diagonal_and_bsgs_identities(pkg, n, t):
    N = n // 2
    rng = np.random.default_rng(n)
    x = rng.integers(0, t, (2, N))
    for name, M in _matrices(rng, N, t).items():
        M2 = np.stack([M, M]) if M.ndim == 2 else M
        want = D.matvec(M2, x, t)
        assert np.array_equal(D.diag_apply(M2, x, t), want), name
        diag = D.diagonals(M2, t)
        kept = [d for d in range(N) if np.any(diag[d] != 0)]
        for n1 in (1, 4, N):
            got_n1, baby, giant, rows = pkg.bfv.bsgs_diagonals(M, t, n1)
            assert got_n1 == n1 and rows.shape == (len(giant), len(baby), 2, N) and rows.min() >= 0 and rows.max() < t
            assert baby == sorted({d % n1 for d in kept}) and giant == sorted({d // n1 for d in kept}), name
            for a, j in enumerate(giant):
                for b, i in enumerate(baby):
                    d = n1 * j + i
                    expect = np.roll(diag[d], n1 * j, axis=1) if d in kept else np.zeros((2, N), dtype=np.int64)
                    assert np.array_equal(rows[a][b], expect), (name, n1, d)
            assert np.array_equal(D.bsgs_apply(n1, baby, giant, rows, x, t), want), (name, n1)
        n1, baby, giant, rows = pkg.bfv.bsgs_diagonals(M, t)
        assert n1 == int(np.ceil(np.sqrt(len(kept)))) and np.array_equal(D.bsgs_apply(n1, baby, giant, rows, x, t), want)
    n1, baby, giant, rows = pkg.bfv.bsgs_diagonals(np.zeros((N, N), dtype=np.int64), t)
    assert (baby, giant) == ([0], [0]) and not rows.any()
    for bad in (np.zeros((3, N, N)), np.zeros((N, N + 1)), np.zeros((N,))):
        with pytest.raises(ValueError):
            pkg.bfv.bsgs_diagonals(bad, t)
    with pytest.raises(ValueError):
        pkg.bfv.bsgs_diagonals(np.eye(N, dtype=np.int64), t, N + 1)


def test_lincomb_residues(pkg):
    bfv = pkg.bfv
    n, k, t = 64, 2, 257
    mods, aux, P = R.chain(n, k, bq=50, bb=61, bp=51)
    param = bfv.RnsParam(n, mods, aux, P, t)
    delta = R.prod(mods) // t
    weights = [[1, -1, 128, 129], [0, t, t + 3, -(10 ** 30)]]
    consts = [5, -5 + 3 * t]
    w, kk = bfv.lincomb_residues(param, weights, consts)
    cw = [[1, -1, 128, -128], [0, 0, 3, D.centred(-(10 ** 30), t)]]
    assert [[D.centred(x, t) for x in row] for row in weights] == cw and bfv.centred(129, t) == -128 and bfv.centred(128, t) == 128
    assert w == [x % q for row in cw for x in row for q in mods] and all(0 <= x < q for x, q in zip(w, list(mods) * 8))
    assert kk == [delta * c % q for c in (5, -5) for q in mods]
    assert bfv.lincomb_residues(param, weights)[1] is None
    # a constant's encoding is that of the constant polynomial: floor(Q / t) c in coefficient 0 alone is what encrypt scales, and
    # the residues are the scale_msg words of m = c mod t up to the multiple floor(Q / t) t of Q - (Q mod t)
    sm = R.scale_msg(mods, t, np.array([[5, t - 5]], dtype=np.uint64))
    for i, q in enumerate(mods):
        assert int(sm[i, 0, 0]) % q == kk[i] and (int(sm[i, 0, 1]) - delta * t) % q == kk[k + i]


def test_sources_exports_and_header(pkg):
    from conftest import ROOT

    B = pkg.binding
    assert "fhe_bfv_rns_dot_dev" in B.EXPORTS and B.FHE_BFV_DOT_MAX_COUNT == D.MAX_COUNT == 64
    h = open(os.path.join(ROOT, "include", "fhe_ntt.h")).read()
    assert re.search(r"\bint\s+fhe_bfv_rns_dot_dev\(", h) and re.search(r"#define\s+FHE_BFV_DOT_MAX_COUNT\s+64\b", h)
    assert hasattr(pkg.load_library(), "fhe_bfv_rns_dot_dev")
    src = open(os.path.join(ROOT, "fhe-study_amd", "csrc", "bfv_rns.hip")).read()
    assert "bfv_rns_tensorsum_kernel" in src and "MacAcc" in src
    for name in ("dot", "lincomb", "encode_diagonals", "LinearTransform", "bsgs_diagonals"):
        assert hasattr(pkg.bfv, name)
    for name in ("square", "mul_const", "diag_sum", "linear_transform"):
        assert hasattr(pkg.bfv.RnsCiphertext, name)
    assert hasattr(pkg.bfv.RnsClientKey, "encode_diagonals") and hasattr(pkg.bfv.LinearTransform, "required_steps")


def test_rejections_that_need_no_device(pkg):
    """the chain, the count, the weights and the admission are checked on the host before the device is looked at"""
    B = pkg.binding
    n, k = 64, 2
    mods, aux, P, t = _edge_base(n, k, 7)
    plans, ap, sp = [pkg.Plan(q, n) for q in mods], [pkg.Plan(b, n) for b in aux], pkg.Plan(P, n)
    d = 4096                     # a non-NULL, aligned fake device address: every call below is refused before it could be read

    def refused(code, as_, bs, w, **kw):
        with pytest.raises(B.FheError) as e:
            B.bfv_rns_dot_dev(kw.get("plans", plans), kw.get("aux", ap), kw.get("special", sp), kw.get("t", t), d, as_, bs, w, d + (1 << 30), 1, count=kw.get("count"), limbs=kw.get("limbs"))
        assert e.value.code == code, e.value

    refused(B.FHE_E_INVALID, [d], [d], None, count=0)
    refused(B.FHE_E_INVALID, [d] * 65, [d] * 65, None)
    refused(B.FHE_E_NULL, None, [d], None, count=1)
    refused(B.FHE_E_NULL, [d], None, None, count=1)
    refused(B.FHE_E_INVALID, [d, d], [d, d], [1, 0])                 # a zero weight
    refused(B.FHE_E_INVALID, [d, d], [d, d], [1, 1 << 61])           # 2^61 and above in absolute value
    refused(B.FHE_E_INVALID, [d, d], [d, d], [1, -(1 << 61)])
    refused(B.FHE_E_INVALID, [d, d], [d, d], [1, -(1 << 63)])
    refused(B.FHE_E_INVALID, [d] * 8, [d] * 8, None)                 # W = 8 past the boundary 7
    refused(B.FHE_E_INVALID, [d, d], [d, d], [4, -4])
    refused(B.FHE_E_INVALID, [d], [d], [-8])
    refused(B.FHE_E_INVALID, [d], [d], None, t=8 * t)                # a base that does not admit a single product
    refused(B.FHE_E_NULL, [d], [d], None, aux=None)
    refused(B.FHE_E_NULL, [d], [d], None, special=None)
    refused(B.FHE_E_NULL, [d], [d], None, plans=None, limbs=k)
    refused(B.FHE_E_INVALID, [d], [d], None, aux=[ap[0], ap[0], ap[1]])
    refused(B.FHE_E_INVALID, [d], [d], None, special=pkg.Plan(E.primes_below(30, n, 1)[0], n))
    refused(B.FHE_E_INVALID, [d], [d], None, t=1)
    refused(B.FHE_E_PARAM_MISMATCH, [d], [d], None, special=pkg.Plan(E.primes_below(62, 128, 1)[0], 128))
    # batch = 0 returns after those checks: W = 7 and [3, -4] pass, one more does not
    B.bfv_rns_dot_dev(plans, ap, sp, t, None, [None] * 7, [None] * 7, None, None, 0)
    B.bfv_rns_dot_dev(plans, ap, sp, t, None, [None, None], [None, None], [3, -4], None, 0)
    with pytest.raises(B.FheError) as e:
        B.bfv_rns_dot_dev(plans, ap, sp, t, None, [None] * 8, [None] * 8, None, None, 0)
    assert e.value.code == B.FHE_E_INVALID and "t n Q W + 1" in str(e.value)


def test_admission_arithmetic_program(pkg):
    """fhe-study_amd/host/test_bfv_admit.cpp: bfv_admits and big_mul128 of csrc/rns_tables.hpp against a boundary computed by
    divisions, at W in {1, boundary, boundary + 1, 64 (2^61 - 1)}; a stand-alone program that needs neither the library nor a
    GPU, and the same program under AddressSanitizer and UndefinedBehaviorSanitizer where the ROCm clang++ is installed"""
    from conftest import ROOT

    host = os.path.join(ROOT, "fhe-study_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_bfv_admit"])
    r = subprocess.run([os.path.join(host, "test_bfv_admit")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all bfv admission tests passed" in r.stdout, r.stdout + r.stderr
    if os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        r = subprocess.run(["make", "-s", "-C", host, "san_admit"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "all bfv admission tests passed" in r.stdout, r.stdout + r.stderr
