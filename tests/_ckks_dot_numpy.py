"""Restatement of the CKKS inner product as DESIGN.md §29 defines it, on tests/_ckks_eval_numpy.py (the chain, the tensor, the
relinearisation, the rescale).  Nothing here calls the library under test.

    tensor sum  d[i] = sum_r w[r][i] tensor(a_r, b_r)[i] mod q_i over limbs i < k, three components; the operands may hold more
                limbs, which are not read; a_r may be b_r and an operand may appear in several pairs; w canonical residues, None: ones
    dot         relinearize(tensor sum): ONE key switch whatever the number of pairs
    weights     w[r] = round(coeff[r] S / (scale(a_r) scale(b_r))) as a Python integer (the float64 product and quotient in this
                order), reduced per limb; S the target scale, the largest pair scale where none is given; None where all are 1
    kernel      one limb, up to GROUP pairs a launch, later groups carried from the canonical words the former one stored; the
                weight is folded into a_r first (w a_r0 mod q, w a_r1 mod q); d0 and d2 take one term a pair, d1 two; all three
                fold before pair r > 0 of a group where r is a multiple of CHUNK / 2 (q < 2^62) or CHUNK63 / 2 (q >= 2^62)
    noise       a ciphertext carries (scale, V, N): |slot| <= V for the exact value and |sigma(c0 + c1 s) - scale value|_inf <= N
"""
import numpy as np

import _ckks_eval_numpy as E
import _ckks_numpy as K

U64 = np.uint64
GROUP = 16                      # kDotGroup: pairs of one launch, by value
MAX_COUNT = 64                  # FHE_CKKS_DOT_MAX_COUNT
CHUNK, CHUNK63 = 8, 2           # kMacChunk, kMacChunk63: terms between two folds


def fold_period(q):
    """pairs between two folds: d1 takes two terms a pair"""
    return (CHUNK63 if q >> 62 else CHUNK) // 2


def tensor_sum(mods, pairs, w=None):
    """pairs: list of (a, b), u64 [>= limbs][2][batch][n]; w [count][limbs] Python integers below q_i, or None -> u64
    [limbs][3][batch][n].  Exact integers per limb up to 2^14 words, the oracle's modular products above that (the same words:
    every sum is exact modulo q_i)"""
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


def dot(mods, P, rlk, pairs, w=None):
    """-> u64 [limbs][2][batch][n]: the relinearisation of the summed tensor; rlk may be the key of a longer chain"""
    return E.relinearize(mods, P, rlk, tensor_sum(mods, pairs, w))


def accumulate(q, words, ws, group=GROUP):
    """the kernel's order of operations for one word on Python integers, asserting the 128-bit bound it claims at every step.
    words: [(a0, a1, b0, b1)] per pair, ws: the weights or None -> (d0, d1, d2) canonical"""
    period = fold_period(q)
    d = None
    for p0 in range(0, len(words), group):
        v = [0, 0, 0] if d is None else list(d)                              # zero, or the carried canonical words
        assert all(x < q for x in v)
        for r in range(min(group, len(words) - p0)):
            if r and r % period == 0:
                v = [x % q for x in v]
            a0, a1, b0, b1 = words[p0 + r]
            if ws is not None:                                               # the weight is folded into a first: canonical again
                a0, a1 = ws[p0 + r] * a0 % q, ws[p0 + r] * a1 % q
                assert ws[p0 + r] < q
            assert max(a0, a1, b0, b1) < q
            v[0] += a0 * b0
            v[1] += a0 * b1
            assert v[1] < 1 << 128, (q, p0, r)                               # between d1's two terms too
            v[1] += a1 * b0
            v[2] += a1 * b1
            assert max(v) < 1 << 128, (q, p0, r)
        d = [x % q for x in v]
    return tuple(d)


def weights(coeffs, S, scales, mods):
    """the rule of ckks.dot -> (w [count][limbs] or None where every integer is 1, the integers before reduction)"""
    big = [round(float(c) * S / s) for c, s in zip(coeffs, scales)]
    return (None if all(x == 1 for x in big) else [[x % q for q in mods] for x in big]), big


def flat(w):
    return None if w is None else [int(x) for row in w for x in row]


def launch_counts(k, count):
    """§29's formula: ckks_rns_tensorsum launches of one chunk"""
    return k * -(-count // GROUP)


# ---- the case lists that tests/test_ckks_dot_cpu.py proves and tests/test_ckks_dot_gpu.py runs ----------------------------------------
COUNTS = (1, 2, 3, GROUP, GROUP + 1, 2 * GROUP + 1)
# (n, k, batch, chain): every case runs every count, with and without weights
WORD_CASES = ([(n, k, b, (58, 40)) for n in (4, 16, 64) for k in (1, 2, 3) for b in ((1, 3) if n == 16 else (1,) if n == 4 else (3,))]
              + [(16, 8, 1, "wide"), (256, 8, 3, "wide")])
TWO_CHUNKS = (4096, 3, 57, (58, 40))
PAST_THE_GRID = (4096, 1, 301, (58, 40))
OVERFLOW_COUNTS = (1, 2, GROUP, GROUP + 1, MAX_COUNT)


def sweep():
    """(count, weighted) of a word-for-word case"""
    return [(c, wt) for c in COUNTS for wt in (False, True)]


def random_weights(mods, count, rng):
    r = np.random.default_rng(rng)
    return [[int(r.integers(0, q)) for q in mods] for _ in range(count)]


# ---- the noise bound, from tests/_ckks_eval_numpy.py's terms ---------------------------------------------------------------------------
def fresh(n, vmax):
    """(V, N) of a fresh encryption of slots |z| <= vmax: the encoder's rounding included, a slot bounded by the 1-norm"""
    return float(vmax), n * (E.fresh_noise(n) + 0.5 + 2.0 ** -10)


def pair_noise(sa, a, sb, b):
    """slot noise of the unrelinearised product of (scale, (V, N)) a and b: (s_a z_a + e_a)(s_b z_b + e_b) slot-wise, and the float
    product of the scales, off by 2^-53; the tensor itself is exact (d0 + d1 s + d2 s^2 is the product of the phases)"""
    return sa * a[0] * b[1] + sb * b[0] * a[1] + a[1] * b[1] + sa * sb * a[0] * b[0] * 2.0 ** -52


def dot_bounds(n, mods, pairs, coeffs, S, fused=True):
    """worst-case slot error of rescale(dot) on the top limb of `mods`, composed from §22's terms.  pairs: [((s_a, (V_a, N_a)),
    (s_b, (V_b, N_b)))].  Pair r enters with the integer weight w_r = a S / s_r + delta: its noise times |w_r|, delta times its
    scaled value (|delta| <= the rounding as it fell plus the float product and quotient, |w| 2^-50).
    fused: ONE n relin_noise(n, k) on the sum.  Otherwise the composed form, a mul per pair and a lincomb: count of them, each
    multiplied by its weight.  Then one rescale.  -> (bound on |decoded - exact| before the decoder's own E_dec, the final scale,
    the part of that bound which the relinearisations contribute)"""
    k = len(mods)
    relin = n * E.relin_noise(n, k)
    N, V, R = 0.0, 0.0, (relin if fused else 0.0)
    for c, ((sa, a), (sb, b)) in zip(coeffs, pairs):
        s = sa * sb
        big = round(float(c) * S / s)
        delta = abs(big - float(c) * S / s) + abs(big) * 2.0 ** -50
        N += abs(big) * pair_noise(sa, a, sb, b) + delta * s * a[0] * b[0]
        R += 0.0 if fused else abs(big) * relin
        V += abs(float(c)) * a[0] * b[0]
    q = mods[-1]
    N = (N + R) / q + n * E.rescale_noise(n) + S / q * V * 2.0 ** -52
    return N / (S / q), S / q, R / S


# ---- the functional cases: n = 16 on §22's (58, 40) chain of 3 limbs; one rescale brings every target scale to about 2^40 ---------------
SEED = bytes((17 * i + 9) % 256 for i in range(32))
ZMAX = 2.0 ** 0.5
FUNCTIONAL = {
    "ones": dict(n=16, rows=2, delta=2.0 ** 40, coeffs=None, count=2, up=1.0, rng=2901),              # w = None: the unweighted kernel
    "integers": dict(n=16, rows=2, delta=2.0 ** 40, coeffs=[1, -2, 3], count=3, up=1.0, rng=2902),    # exact integer weights
    "reals": dict(n=16, rows=2, delta=2.0 ** 30, coeffs=[0.3, -0.7, 1.1, 0.25], count=4, up=2.0 ** 20, rng=2903),   # S = delta^2 2^20
}


def functional_slots(case, r, which):
    g = np.random.default_rng(case["rng"] + 10 * r + which)
    shape = (case["rows"], case["n"] // 2)
    return g.uniform(-1, 1, shape) + 1j * g.uniform(-1, 1, shape)


def functional_target(case):
    """(coeffs, S or None as ckks.dot takes it, S as a number)"""
    coeffs = [1.0] * case["count"] if case["coeffs"] is None else case["coeffs"]
    S = case["delta"] ** 2 * case["up"]
    return coeffs, (None if case["up"] == 1.0 else S), S


def functional_run(case, tab):
    """encrypt, dot, rescale, decrypt and decode, all in the restatement, and the composed form (a mul per pair, their weighted sum)
    on the same ciphertexts -> everything the GPU module compares against"""
    n, rows, delta, count = case["n"], case["rows"], case["delta"], case["count"]
    mods, P = E.chain(n, 58, 40, 2)
    s = K.secret_key(SEED, 0, n)
    pk = E.public_key(SEED, E.PK_BASE, s, mods, tab)
    rlk = E.relin_key(SEED, E.RLK_BASE, s, mods, P, tab)
    zs = [(functional_slots(case, r, 0), functional_slots(case, r, 1)) for r in range(count)]
    cts = [tuple(E.encrypt(SEED, (2 * r + j) * rows, pk, K.encode(z, delta), rows, mods, tab) for j, z in enumerate(pair)) for r, pair in enumerate(zs)]
    coeffs, _, S = functional_target(case)
    w, big = weights(coeffs, S, [delta * delta] * count, mods)
    res = E.rescale(mods, dot(mods, P, rlk, cts, w))
    scale = S / mods[-1]
    d = E.decrypt(mods[:-1], n, s, res)
    got = K.decode(d, scale)
    want = sum(c * x * y for c, (x, y) in zip(coeffs, zs))
    wire = (delta, fresh(n, ZMAX))
    bound, bscale, relin = dot_bounds(n, mods, [(wire, wire)] * count, coeffs, S)
    composed, _, relin_composed = dot_bounds(n, mods, [(wire, wire)] * count, coeffs, S, fused=False)
    assert bscale == scale
    # the composed form's words: they differ from the fused ones by design (count relinearisations, each with its own noise)
    acc = [np.zeros(res.shape[1:], dtype=object) for _ in mods]
    for r, (a, b) in enumerate(cts):
        p = E.mul(mods, P, rlk, a, b)
        acc = [x + p[i].astype(object) * (big[r] % q) for i, (x, q) in enumerate(zip(acc, mods))]
    comp = E.rescale(mods, np.stack([(x % q).astype(U64) for x, q in zip(acc, mods)]))
    dc = E.decrypt(mods[:-1], n, s, comp)
    edec = float(K.e_dec(d, scale).max())
    return dict(mods=mods, P=P, s=s, zs=zs, cts=cts, coeffs=coeffs, S=S, w=w, big=big, res=res, scale=scale, got=got, want=want, comp=comp,
                err=float(np.abs(got - want).max()), err_composed=float(np.abs(K.decode(dc, scale) - want).max()), bound=bound + edec,
                bound_composed=composed + float(K.e_dec(dc, scale).max()), raw_bounds=(bound, composed), relin=(relin, relin_composed))
