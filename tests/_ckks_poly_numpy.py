"""Restatement of the CKKS polynomial evaluation as DESIGN.md §27 defines it, on tests/_ckks_eval_numpy.py (the chain, ct x ct, the
rescale).  Nothing here calls the library under test; a ChebyshevPlan's op list is data that `replay` interprets.

    lincomb     out_o[i][c][e] = (sum_r w[o][r][i] ct_r[i][c][e] + [c = 0] k[o][i]) mod q_i over limbs i < k; the inputs may hold more
                limbs, which are not read; the same input may appear twice; w, k canonical residues
    weights     w[o][r] = round(coeff[o][r] S_o / scale_r) as a Python integer (the float64 product and quotient in this order), k[o] =
                round(const[o] S_o), both reduced per limb; S_o = the output's target scale, the largest input scale where none is given
    plan ops    ("lincomb", outs, ins, coeffs, consts, [(p, e) per output], drop), ("mul", out, a, b), ("rescale", out, a); a symbolic scale
                (p, e) is s^p prod_j q_(l-j)^e[j], factors taken in that order
    replay      mul: the level is the lower one, the scale the float product; rescale: scale / q_level; lincomb: the level l - drop,
                the scale S
    noise       a wire carries (scale, V, N): |slot| <= V for the exact value and |sigma(c0 + c1 s) - scale value|_inf <= N
"""
import numpy as np

import _ckks_eval_numpy as E

U64 = np.uint64
GROUP = 16                      # kLinGroup: inputs of one launch, by value
OUT_CAP = 4                     # kLinOutputs: outputs whose accumulators one launch keeps in registers
MAX_COUNT, MAX_OUTPUTS = 64, 16
CHUNK, CHUNK63 = 8, 2           # kMacChunk, kMacChunk63: terms between two folds


def lincomb(mods, cts, w, k=None):
    """cts: list of u64 [>= limbs][2][batch][n]; w [outputs][count][limbs] and k [outputs][limbs] Python integers below q_i
    -> u64 [outputs][limbs][2][batch][n], in exact integers per limb"""
    outs = []
    for o in range(len(w)):
        limbs = []
        for i, q in enumerate(mods):
            acc = np.zeros(cts[0][i].shape, dtype=object)
            for r, ct in enumerate(cts):
                assert 0 <= w[o][r][i] < q
                acc = acc + ct[i].astype(object) * int(w[o][r][i])
            if k is not None:
                assert 0 <= k[o][i] < q
                acc[0] = acc[0] + int(k[o][i])
            limbs.append((acc % q).astype(U64))
        outs.append(np.stack(limbs))
    return np.stack(outs)


def weights(coeffs, consts, S, scales, mods):
    """the rule of ckks.lincomb -> (w [outputs][count][limbs], k [outputs][limbs] or None, the integers before reduction)"""
    S = S if isinstance(S, list) else [S] * len(coeffs)
    big = [[round(float(c) * S[o] / s) for c, s in zip(row, scales)] for o, row in enumerate(coeffs)]
    kbig = None if consts is None else [round(float(c) * S[o]) for o, c in enumerate(consts)]
    w = [[[x % q for q in mods] for x in row] for row in big]
    k = None if kbig is None else [[x % q for q in mods] for x in kbig]
    return w, k, big, kbig


def flat(x):
    return None if x is None else [int(v) for v in np.asarray(x, dtype=object).reshape(-1)]


def scale_value(sym, s, mods, level):
    p, e = sym
    v = 1.0
    for _ in range(abs(p)):
        v = v * s if p > 0 else v / s
    for j, x in enumerate(e):
        for _ in range(abs(x)):
            v = v * mods[level - j] if x > 0 else v / mods[level - j]
    return v


def replay(plan, ct, scale, level, mods, P, rlk, noise=None, n=None):
    """the op list on the restatements -> {wire: (words [k][2][batch][n], level, scale)}.  noise = (V, N) of the input: the wires
    then also carry the bounds, -> {wire: (.., V, N)} (see poly_bounds)"""
    w = {0: (None if ct is None else ct[:level + 1], level, float(scale)) + (tuple(noise) if noise else ())}
    for op in plan.ops:
        if op[0] == "lincomb":
            _, outs, ins, co, consts, syms, drop = op
            S, lv = [scale_value(sym, float(scale), mods, level) for sym in syms], level - drop
            assert all(w[i][1] >= lv for i in ins)
            ww, kk, big, kbig = weights(co, consts, S, [w[i][2] for i in ins], mods[:lv + 1])
            res = lincomb(mods[:lv + 1], [w[i][0] for i in ins], ww, kk) if ct is not None else [None] * len(outs)
            for o, wire in enumerate(outs):
                extra = ()
                if noise:
                    V = sum(abs(co[o][r]) * w[i][3] for r, i in enumerate(ins)) + (abs(consts[o]) if consts else 0.0)
                    # the weight is a S / s_r + delta, |delta| <= |w - fl(a S / s_r)| + |w| 2^-50 (the rounding to an integer as it
                    # fell, at most 1/2, and the float product and quotient): the input's noise times |w|, delta times the input's
                    # scaled value; the constant likewise
                    N = 0.0
                    for r, i in enumerate(ins):
                        delta = abs(big[o][r] - float(co[o][r]) * S[o] / w[i][2]) + abs(big[o][r]) * 2.0 ** -50
                        N += abs(big[o][r]) * w[i][4] + delta * w[i][2] * w[i][3]
                    if consts:
                        N += abs(kbig[o] - float(consts[o]) * S[o]) + abs(kbig[o]) * 2.0 ** -50
                    extra = (V, N)
                w[wire] = (res[o], lv, S[o]) + extra
        elif op[0] == "mul":
            a, b = w[op[2]], w[op[3]]
            lv = min(a[1], b[1])
            res = E.mul(mods[:lv + 1], P, rlk, a[0][:lv + 1], b[0][:lv + 1]) if ct is not None else None
            extra = ()
            if noise:                                             # §22: slot-wise products; the float product of the scales is off by 2^-53
                s = a[2] * b[2]
                extra = (a[3] * b[3], a[2] * a[3] * b[4] + b[2] * b[3] * a[4] + a[4] * b[4] + n * E.relin_noise(n, lv + 1) + s * a[3] * b[3] * 2.0 ** -52)
            w[op[1]] = (res, lv, a[2] * b[2]) + extra
        else:
            a = w[op[2]]
            res = E.rescale(mods[:a[1] + 1], a[0]) if ct is not None else None
            extra = (a[3], a[4] / mods[a[1]] + n * E.rescale_noise(n) + a[2] / mods[a[1]] * a[3] * 2.0 ** -52) if noise else ()
            w[op[1]] = (res, a[1] - 1, a[2] / mods[a[1]]) + extra
    return w


def poly_bounds(plan, n, mods, level, scale, xmax):
    """worst-case slot error of eval_chebyshev on a fresh encryption of slots |x| <= xmax, composed from §22's terms along the op
    list: the input's slot noise is n (fresh_noise + 1/2 + 2^-10) (the encoder's rounding included; a slot is bounded by the
    1-norm of the coefficients), and the rules of `replay`.  -> (bound on |decoded - exact|, the result's scale)"""
    N0 = n * (E.fresh_noise(n) + 0.5 + 2.0 ** -10)
    w = replay(plan, None, scale, level, mods, None, None, noise=(float(xmax), N0), n=n)
    _, _, s, _, N = w[plan.result]
    return N / s, s


def launch_counts(k, count, outputs):
    """§27's formula: launches of one fhe_ckks_rns_lincomb_dev call"""
    return -(-outputs // OUT_CAP) * k * -(-count // GROUP)


def product_count(d):
    """ct x ct products of the rule, by its own recurrence: the babies T_2 .. T_(n1-1) and the giants one each, and one per
    division p = q T_g + r, on degrees alone (deg q = deg p - g; deg r = g - 1 at most and taken as that: dense coefficients)"""
    m = d.bit_length()
    n1 = 1 << ((m + 1) // 2)
    giants = [n1 << t for t in range(m) if (n1 << t) <= d]

    def divs(deg):
        if deg < n1:
            return 0
        g = max(x for x in giants if x <= deg)
        return 1 + divs(deg - g) + divs(g - 1)
    return max(n1 - 2, 0) + len(giants) + divs(d)


def level_count(d, interval_map=False):
    """levels of the rule: drop(T_i) = ceil(log2 i) (+ 1 behind the interval map); need(p) = the drop of its unrescaled value"""
    m = d.bit_length()
    n1 = 1 << ((m + 1) // 2)
    giants = [n1 << t for t in range(m) if (n1 << t) <= d]
    base = 1 if interval_map else 0

    def drop(i):
        return base + (i - 1).bit_length()

    def need(deg):
        if deg < n1:
            return drop(max(deg, 1))
        g = max(x for x in giants if x <= deg)
        return max(need(deg - g) + 1, drop(g), need(g - 1))
    return need(d) + 1


# ---- the case lists that tests/test_ckks_poly_cpu.py proves and tests/test_ckks_poly_gpu.py runs --------------------------------------
COUNTS = (1, 2, 3, 8, 9, 16, 17, 33)
OUTPUTS = (1, 2, 3, 5)
# (n, k, batch, chain): every case runs every count with one output and constants, and count 3 and 17 with every output count
WORD_CASES = ([(n, k, b, (58, 40)) for n in (4, 16, 64) for k in (1, 2, 3) for b in ((1, 3) if n == 16 else (1,) if n == 4 else (3,))]
              + [(16, 8, 1, "wide"), (256, 8, 3, "wide")])
BIG_CASE = (4096, 1, 301, (58, 40))
OVERFLOW_COUNTS = (1, 2, 3, 8, 9, 16, 17, 64)


def sweep(n, k):
    """(count, outputs, with constants) of a word-for-word case"""
    out = [(c, 1, c % 2 == 1) for c in COUNTS]
    out += [(c, o, o % 2 == 0) for c in (3, 17) for o in OUTPUTS if o > 1]
    return out


def random_weights(mods, outputs, count, rng, consts=True):
    r = np.random.default_rng(rng)
    w = [[[int(r.integers(0, q)) for q in mods] for _ in range(count)] for _ in range(outputs)]
    k = [[int(r.integers(0, q)) for q in mods] for _ in range(outputs)] if consts else None
    return w, k


def edge_ct(mods, batch, n, shift):
    """words q - 1, 0, 1, floor(q/2), floor(q/2) + 1 in every limb, the first row q - 1 throughout"""
    out = []
    for i, q in enumerate(mods):
        vals = np.array([q - 1, q - 1, 0, 1, q // 2, q // 2 + 1, q - 1, q - 1], dtype=U64)
        x = vals[(np.arange(2 * batch * n) + shift + i) % len(vals)].reshape(2, batch, n)
        x[:, 0] = q - 1
        out.append(x)
    return np.stack(out)


# ---- the functional cases: (n, degree, interval) on §22's (58, 40) chain of 8 limbs, Delta = 2^40 --------------------------------------
SEED = bytes((13 * i + 3) % 256 for i in range(32))
DELTA = 2.0 ** 40
FUNCTIONAL = {
    "deg7": dict(n=16, degree=7, interval=(-1.0, 1.0), rows=2, rng=2701),
    "logistic15": dict(n=32, degree=15, interval=(-4.0, 4.0), rows=2, rng=2702),
}


def logistic(x):
    return 1.0 / (1.0 + np.exp(-x))


def chebyshev_fit(f, degree, interval):
    """interpolation at the Chebyshev nodes, restated"""
    a, b = interval
    N = degree + 1
    t = np.cos(np.pi * (np.arange(N) + 0.5) / N)
    fx = f((b - a) / 2 * t + (a + b) / 2)
    c = np.array([2.0 / N * np.sum(fx * np.cos(np.pi * i * (np.arange(N) + 0.5) / N)) for i in range(N)])
    c[0] /= 2
    return c


def functional_coeffs(case):
    if case["degree"] == 15:
        return chebyshev_fit(logistic, 15, case["interval"])
    return np.random.default_rng(case["rng"]).uniform(-1, 1, case["degree"] + 1)


def functional_slots(case):
    """real slots in the interval"""
    a, b = case["interval"]
    return np.random.default_rng(case["rng"] + 1).uniform(a, b, (case["rows"], case["n"] // 2)).astype(np.complex128)
