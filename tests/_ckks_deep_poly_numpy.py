"""Restatement of the scalar sums, inner products and Chebyshev plans on the deep CKKS chain as DESIGN.md §39 defines them, in Python
integers, on tests/_ckks_deep_numpy.py (the grouped-digit relinearisation, the rescale) and tests/_ckks_eval_numpy.py (the
transforms).  Nothing here calls the library under test; a ChebyshevPlan's op list is data that `replay` interprets.

    lincomb     out_o[i][c][e] = (sum_r w[o][r][i] ct_r[i][c][e] + [c = 0] k[o][i]) mod q_i over limbs i < l; the inputs may hold more
                limbs, which are not read; the same input may appear twice; w, k canonical residues
    tensor sum  d[i] = sum_r w[r][i] tensor(a_r, b_r)[i] mod q_i, three components; a_r may be b_r; w None: ones
    dot         _ckks_deep_numpy.relinearize(tensor sum): ONE grouped-digit key switch whatever the number of pairs
    kernels     a launch covers a slice of up to SLICE = 8 limbs; a scalar sum up to LIN_INPUTS = 8 inputs into up to OUT_CAP = 4
                outputs, folding before input r > 0 of a launch with 8 | r; a summed tensor up to DOT_PAIRS = 16 pairs, folding
                before pair r > 0 with 4 | r; later groups start from the canonical words the former stored; every q < 2^62
    launches    lincomb: ceil(l / 8) ceil(outputs / 4) ceil(count / 8); a chunk of a dot: ceil(l / 8) ceil(count / 16), and then
                those of the relinearisation
    noise       relin(sum_r w_r a_r (x) b_r) is off sum_r w_r dec(a_r) dec(b_r) by ONE switch error (§36's bound), whatever the count
"""
import numpy as np

import _ckks_deep_numpy as D
import _ckks_eval_numpy as E

U64 = np.uint64
SLICE, LIN_INPUTS, OUT_CAP, DOT_PAIRS = 8, 8, 4, 16
MAX_COUNT, MAX_OUTPUTS, DOT_MAX_COUNT = 64, 16, 64
CHUNK = 8                       # kMacChunk: terms between two folds; every modulus is below 2^62


def _ceil(a, b):
    return -(-a // b)


# ---- the definitions, per limb, in exact integers ---------------------------------------------------------------------------------------
def lincomb(mods, cts, w, k=None):
    """cts: list of u64 [>= limbs][2][batch][n]; w [outputs][count][limbs] and k [outputs][limbs] Python integers below q_i
    -> u64 [outputs][limbs][2][batch][n]"""
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


def tensor_sum(mods, pairs, w=None):
    """pairs: list of (a, b), u64 [>= limbs][2][batch][n]; w [count][limbs] Python integers below q_i, or None -> u64
    [limbs][3][batch][n].  Exact integers per limb up to 2^14 words, modular products above that (the same words: every sum is
    exact modulo q_i)"""
    out = []
    for i, q in enumerate(mods):
        big = pairs[0][0][i, 0].size > 1 << 14
        acc = [np.zeros(pairs[0][0][i, 0].shape, dtype=U64 if big else object) for _ in range(3)]
        for r, (a, b) in enumerate(pairs):
            wr = 1 if w is None else int(w[r][i])
            assert 0 <= wr < q
            if big:
                a0, a1 = (E.pmul(q, a[i, c], U64(wr)) for c in range(2))
                terms = (E.pmul(q, a0, b[i, 0]), E.padd(q, E.pmul(q, a0, b[i, 1]), E.pmul(q, a1, b[i, 0])), E.pmul(q, a1, b[i, 1]))
                acc = [E.padd(q, x, t) for x, t in zip(acc, terms)]
            else:
                a0, a1, b0, b1 = (x.astype(object) for x in (a[i, 0], a[i, 1], b[i, 0], b[i, 1]))
                acc = [acc[0] + wr * a0 * b0, acc[1] + wr * (a0 * b1 + a1 * b0), acc[2] + wr * a1 * b1]
        out.append(np.stack([x if big else (x % q).astype(U64) for x in acc]))
    return np.stack(out)


def dot(mods, specials, key, pairs, w=None):
    """-> u64 [limbs][2][batch][n]; key may be that of a longer chain"""
    return D.relinearize(mods, specials, key, tensor_sum(mods, pairs, w))


# ---- the kernels' order of operations for one word, asserting the 128-bit bound they claim ---------------------------------------------
def accumulate_lincomb(q, words, ws, k, group=LIN_INPUTS, period=CHUNK):
    assert q < 1 << 62
    v = None
    for r0 in range(0, len(words), group):
        acc = k if v is None else v                                          # the constant, or the carried canonical word
        assert acc < q
        for r in range(min(group, len(words) - r0)):
            if r and r % period == 0:
                acc %= q
            assert ws[r0 + r] < q and words[r0 + r] < q
            acc += ws[r0 + r] * words[r0 + r]
            assert acc < (1 << 127) + (1 << 62), (q, r0, r)
        v = acc % q
    return v


def accumulate_tensorsum(q, words, ws, group=DOT_PAIRS, period=CHUNK // 2):
    """words: [(a0, a1, b0, b1)] per pair, ws: the weights or None -> (d0, d1, d2) canonical"""
    assert q < 1 << 62
    d = None
    for p0 in range(0, len(words), group):
        v = [0, 0, 0] if d is None else list(d)
        for r in range(min(group, len(words) - p0)):
            if r and r % period == 0:
                v = [x % q for x in v]
            a0, a1, b0, b1 = words[p0 + r]
            if ws is not None:                                               # the weight is folded into a first: canonical again
                assert ws[p0 + r] < q
                a0, a1 = ws[p0 + r] * a0 % q, ws[p0 + r] * a1 % q
            v[0] += a0 * b0
            v[1] += a0 * b1 + a1 * b0
            v[2] += a1 * b1
            assert max(v) < (1 << 127) + (1 << 62), (q, p0, r)
        d = [x % q for x in v]
    return tuple(d)


# ---- the launches ------------------------------------------------------------------------------------------------------------------------
def lincomb_launches(limbs, outputs, count):
    return _ceil(limbs, SLICE) * _ceil(outputs, OUT_CAP) * _ceil(count, LIN_INPUTS)


def tensorsum_launches(limbs, count):
    return _ceil(limbs, SLICE) * _ceil(count, DOT_PAIRS)


def lincomb_partition(limbs, outputs, count):
    """the launches in the order they are issued -> [(o0, no, i0, nl, r0, nr)]: every (output, limb, input) lies in exactly one"""
    return [(o0, min(OUT_CAP, outputs - o0), i0, min(SLICE, limbs - i0), r0, min(LIN_INPUTS, count - r0))
            for o0 in range(0, outputs, OUT_CAP) for i0 in range(0, limbs, SLICE) for r0 in range(0, count, LIN_INPUTS)]


def dot_launch_counts(limbs, alpha, count):
    """one chunk of a dot, by label: the summed tensor, then relin_rows' (§36): an extension a digit group and the modulus-down,
    a key sum a target, a divide-and-round a limb"""
    return dict(tensorsum=tensorsum_launches(limbs, count), tensor=0, extend=D.dnum(limbs, alpha) + 1, keymac=limbs + alpha, divround=limbs)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
def lin_weights(coeffs, consts, S, scales, mods):
    """the rule of ckks.lincomb -> (w [outputs][count][limbs], k [outputs][limbs] or None)"""
    S = S if isinstance(S, list) else [S] * len(coeffs)
    big = [[round(float(c) * S[o] / s) for c, s in zip(row, scales)] for o, row in enumerate(coeffs)]
    kbig = None if consts is None else [round(float(c) * S[o]) for o, c in enumerate(consts)]
    return [[[x % q for q in mods] for x in row] for row in big], None if kbig is None else [[x % q for q in mods] for x in kbig]


def dot_weights(coeffs, S, scales, mods):
    big = [round(float(c) * S / s) for c, s in zip(coeffs, scales)]
    return None if all(x == 1 for x in big) else [[x % q for q in mods] for x in big]


def flat(x):
    return None if x is None else [int(v) for v in np.asarray(x, dtype=object).reshape(-1)]


def random_lin_weights(mods, outputs, count, rng, consts=True):
    r = np.random.default_rng(rng)
    w = [[[int(r.integers(0, q)) for q in mods] for _ in range(count)] for _ in range(outputs)]
    return w, ([[int(r.integers(0, q)) for q in mods] for _ in range(outputs)] if consts else None)


def random_dot_weights(mods, count, rng):
    r = np.random.default_rng(rng)
    return [[int(r.integers(0, q)) for q in mods] for _ in range(count)]


def top_ct(mods, batch, n):
    """every word q - 1"""
    return np.stack([np.full((2, batch, n), q - 1, dtype=U64) for q in mods])


# ---- a ChebyshevPlan's ops on the restatements ------------------------------------------------------------------------------------------
def scale_value(sym, s, mods, level):
    p, e = sym
    v = 1.0
    for _ in range(abs(p)):
        v = v * s if p > 0 else v / s
    for j, x in enumerate(e):
        for _ in range(abs(x)):
            v = v * mods[level - j] if x > 0 else v / mods[level - j]
    return v


def replay(plan, ct, scale, level, mods, specials, rlk):
    """the op list -> {wire: (words [l][2][batch][n], level, scale)}: lincomb at level - drop with the target scales, mul at the
    lower level with the float product of the scales (not rescaled), rescale by the top prime"""
    w = {0: (ct[:level + 1], level, float(scale))}
    for op in plan.ops:
        if op[0] == "lincomb":
            _, outs, ins, co, consts, syms, drop = op
            S, lv = [scale_value(sym, float(scale), mods, level) for sym in syms], level - drop
            assert all(w[i][1] >= lv for i in ins)
            ww, kk = lin_weights(co, consts, S, [w[i][2] for i in ins], mods[:lv + 1])
            res = lincomb(mods[:lv + 1], [w[i][0] for i in ins], ww, kk)
            for o, wire in enumerate(outs):
                w[wire] = (res[o], lv, S[o])
        elif op[0] == "mul":
            a, b = w[op[2]], w[op[3]]
            lv = min(a[1], b[1])
            w[op[1]] = (D.mul(mods[:lv + 1], specials, rlk, a[0][:lv + 1], b[0][:lv + 1]), lv, a[2] * b[2])
        else:
            a = w[op[2]]
            w[op[1]] = (D.rescale(mods[:a[1] + 1], a[0]), a[1] - 1, a[2] / mods[a[1]])
    return w


def logistic(x):
    return 1.0 / (1.0 + np.exp(-x))


# ---- the case lists of tests/test_ckks_deep_poly_gpu.py ------------------------------------------------------------------------------------
SHAPES = [(5, 2, 5), (5, 2, 4), (9, 3, 7), (17, 8, 17), (3, 8, 3)]            # (L, alpha, l)
SLICE_EDGES = (8, 9, 16, 17)                                                 # l either side of every limb-slice edge
LIN_COUNTS = (1, 8, 9, 17, 64)
LIN_OUTPUTS = (1, 4, 5, 16)
DOT_COUNTS = (1, 4, 5, 16, 17, 64)
