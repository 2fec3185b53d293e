"""Case lists and helpers of the sweep of BFV on the RNS chain (bfv_rns.hip): tests/test_bfv_rns_shapes_cpu.py
proves them, tests/test_bfv_rns_shapes_gpu.py runs them.  Nothing here calls the library under test; the restatements are the
existing ones (tests/_bfv_rns_numpy.py, tests/_bfv_dot_numpy.py, tests/_ckks_eval_numpy.py).

    A  client     fhe_bfv_rns_decrypt_dev on phases known by construction (c0 = evals(v) - c1 (.) s^), every rounding edge planted,
                  at every k, the auxiliary prime at its floor 2 t + 3, t = 2, t even, t = 2^60 - 1, and across the decrypt's own
                  chunk at (2^16, 3, 11); fhe_bfv_rns_scale_msg_dev on any 64-bit word, t up to Q and to 2^64
    B  extension  sources and targets of mixed size in one call (3 .. 62 bits, both orders), the integers that differ from
                  floor(M / 2) in one mixed-radix digit, a count past one trip of the grid-stride loop
    C  products   k = 3, primes just below 2^62, a mixed chain, the two-pass sizes 2^14 and 2^16 (the ragged tail and the chunk
                  clamp) against a sparse-times-dense product over Z, buffers one word past a 16-byte boundary, slot 13 reused
"""
import random

import numpy as np

import _bfv_rns_numpy as R
import _ckks_eval_numpy as E

U64, I64 = np.uint64, np.int64
T = 65537


def evals_of(mods, n, rows):
    """rows x n Python integers -> evals [k][rows][n]: R.to_evals with the residues taken on object arrays"""
    x = np.array(rows, dtype=object).reshape(len(rows), n)
    return np.stack([E.fwd(q, n, (x % q).astype(U64)) for q in mods])


def small_chain(n, k):
    """primes just above 2^30 (the transforms' 64-bit kind, short integers in the restatement), the base a bit longer"""
    return R.chain(n, k, bq=31, bb=32, bp=33)


# ---- A: the client kernels ---------------------------------------------------------------------------------------------------------
DECRYPT_SHAPES = [(n, k) for n in (2, 64, 2048) for k in (1, 2, 3, 4)] + [(1 << 14, 3)]
T60 = (1 << 60) - 1


def prime_below(x):
    c = (x - 1) | 1
    while not E.is_prime(c):
        c -= 2
    return c


B0_T60 = prime_below(1 << 62)


def decrypt_params(k):
    """(t, b_0): b_0 = 2 t + 3, one above the floor, for t = 257, 65537, 2 and the even 2^16; t = 2^60 - 1, the ceiling, at k = 2"""
    out = [(257, 517), (65537, 131077), (2, 7), (1 << 16, (1 << 17) + 3)]
    return out + [(T60, B0_T60)] if k == 2 else out


def quotient_targets(t):
    return [("0", 0), ("+1", 1), ("-1", -1), ("+t/2", t // 2), ("-t/2", -(t // 2)), ("+t", t), ("-t", -t), ("t/2+1", t // 2 + 1)]


def reachable_targets(t):
    """a phase centred in Q has t v + floor(Q / 2) in [-(t - 1) (Q - 1) / 2, (t + 1) (Q - 1) / 2], so its quotient by Q lies in
    [-floor(t / 2), floor(t / 2)] whatever Q is: the targets t, -t and floor(t / 2) + 1 have no phase"""
    return {name for name, m in quotient_targets(t) if -(t // 2) <= m <= t // 2}


def planted_phases(Q, t):
    """-> [(class, v)]: 0, the ends of (-Q/2, Q/2] and their neighbours, and for every target quotient m the smallest and the
    largest v with floor((t v + floor(Q / 2)) / Q) = m; those outside (-Q/2, Q/2] are dropped"""
    h = Q // 2
    out = [("zero", 0), ("+half", h), ("-half", -h), ("+half-1", h - 1), ("-half+1", 1 - h)]
    for name, m in quotient_targets(t):
        lo = -((h - m * Q) // t)                                     # ceil((m Q - floor(Q / 2)) / t)
        hi = -((h - (m + 1) * Q) // t) - 1                           # the v just below the next boundary
        out += [(name + ":min", lo), (name + ":max", hi)]
    return [(c, v) for c, v in out if -h <= v <= h]


def decrypt_batch(n, planted):
    return 3 if n == 64 else 2 if n > 64 else -(-planted // n) + 1


def phase_rows(Q, t, n, batch, seed):
    """batch x n phases centred in Q: the planted ones at the head of every row, uniform ones behind them; where a row is
    shorter than the planted list (n = 2) the list runs on over the rows"""
    rng, h = random.Random(seed), Q // 2
    planted = [v for _, v in planted_phases(Q, t)]
    if len(planted) <= n:
        return [planted + [rng.randrange(-h, h + 1) for _ in range(n - len(planted))] for _ in range(batch)]
    assert batch * n >= len(planted)
    flat = planted + [rng.randrange(-h, h + 1) for _ in range(batch * n - len(planted))]
    return [flat[r * n:(r + 1) * n] for r in range(batch)]


def ct_of_phase(mods, n, rows, seed):
    """-> (s^ [k][n] uniform words, ct [k][2][batch][n] evals) with c1 uniform and c0 = evals(v) - c1 (.) s^ per limb: the
    phase c0 + c1 s is `rows` by construction"""
    r = np.random.default_rng(seed)
    k, batch = len(mods), len(rows)
    ve = evals_of(mods, n, rows)
    s = np.stack([r.integers(0, q, n, dtype=np.uint64) for q in mods])
    ct = np.empty((k, 2, batch, n), dtype=U64)
    for i, q in enumerate(mods):
        ct[i, 1] = r.integers(0, q, (batch, n), dtype=np.uint64)
        ct[i, 0] = E.psub(q, ve[i], E.pmul(q, ct[i, 1], s[i]))
    return s, ct


DECRYPT_CHUNK = (1 << 16, 3, 11, 257, 517)                            # n, k, batch, t, b_0: chunks of 10 + 1 rows


def scale_msg_moduli(k, Q):
    """the values of t: 2, 65537; Q - 1 and Q at k = 1 (delta = 1); just below 2^64 at k = 2"""
    return [2, T] + ([Q - 1, Q] if k == 1 else []) + ([(1 << 64) - 59] if k == 2 else [])


def messages(t, batch, n, seed):
    """[batch][n] words: 0, t - 1, values at and above t up to 2^64 - 1 first, uniform 64-bit words behind them"""
    top = (1 << 64) - 1
    planted = [0, t - 1, min(t, top), min(t + 1, top), 1 << 63, top]
    r = np.random.default_rng(seed).integers(0, top, batch * n, dtype=np.uint64, endpoint=True)
    r[:min(len(planted), batch * n)] = planted[:batch * n]
    return r.reshape(batch, n)


# ---- B: the extension ---------------------------------------------------------------------------------------------------------------
P20, P37, P62 = E.primes_below(20, 8, 4), E.primes_below(37, 8, 4), E.primes_below(62, 8, 4)
# s -> (sources, targets), small before large; "down" reverses both.  The targets 3 (below every source at s = 2 and 3, equal to
# a source at s = 5 and 9) and 11 are not of the form 1 + 16 c: the extension takes any odd modulus from 3 on.
EXT_BASES = {
    2: ([7, P62[0]], [3, 5, P20[2], P37[2], P62[2]]),
    3: ([5, P37[0], P62[0]], [3, 7, P20[2], P62[2]]),
    5: ([3, 7, P20[0], P37[0], P62[0]], [3, 5, 11, P20[2], P20[3], P37[2], P37[3], P62[2], P62[3]]),
    9: ([3, 5, 7, P20[0], P20[1], P37[0], P37[1], P62[0], P62[1]], [3, P62[2]]),
}
EXT_ORDERS = ("up", "down")
EXT_COUNT = 257
STRIDE = ([3, P62[0]], [5, P37[2]], 4096 * 256 + 3)                   # M < 2^64; fhe_ew_grid caps at 4096 blocks of 256


def ext_base(s, order):
    src, dst = EXT_BASES[s]
    return (src, dst) if order == "up" else (src[::-1], dst[::-1])


def planted_integers(src):
    """integers in [0, M): 0, M - 1, floor(M / 2) and its successor; for every position i the integers whose digits are those
    of floor(M / 2) above i and one more or one less at i, with the digits below i those of floor(M / 2), all zero and all
    m_j - 1 (so that digit 0 alone points the wrong way); every digit m_j - 1; and a single non-zero digit"""
    s, h = len(src), R.half_digits(src)
    w = [R.prod(src[:i]) for i in range(s)]

    def val(d):
        assert all(0 <= x < m for x, m in zip(d, src))
        return sum(x * y for x, y in zip(d, w))

    M = R.prod(src)
    out = [0, M - 1, M // 2, M // 2 + 1]
    for i in range(s):
        for step in (1, -1):
            if 0 <= h[i] + step < src[i]:
                for low in (h[:i], [0] * i, [m - 1 for m in src[:i]]):
                    out.append(val(list(low) + [h[i] + step] + h[i + 1:]))
    out.append(val([m - 1 for m in src]))
    for j in range(s):
        for dj in sorted({1, h[j], src[j] - 1} - {0}):
            out.append(val([0] * j + [dj] + [0] * (s - j - 1)))
    assert all(0 <= x < M for x in out)
    return list(dict.fromkeys(out))


def ext_integers(src, count, seed):
    rng, M = random.Random(seed), R.prod(src)
    xs = planted_integers(src)
    assert len(xs) <= count
    return xs + [rng.randrange(M) for _ in range(count - len(xs))]


def ext_want(src, dst, xs, centred):
    M = R.prod(src)
    return np.array([[(R.centre(x, M) if centred else x) % p for x in xs] for p in dst], dtype=U64)


# ---- C: the products -------------------------------------------------------------------------------------------------------------------
K3 = [(n, batch) for n in (8, 64, 2048) for batch in (1, 3)]


def k3_dots(n, batch):
    """(count, mode): unweighted, signed weights, and five pairs, which repeat an operand of the pool of four"""
    if n <= 64:
        return [(2, "null"), (5, "signed"), (3, "ones")]
    return [(5, "signed")] if batch == 1 else [(2, "null")]


def limit_chain(n, k):
    """chain, base and special prime all just below 2^62: the largest is P (it must not be below a chain prime)"""
    ps = E.primes_below(62, n, 2 * k + 2)
    return ps[k + 2:], ps[1:k + 2], ps[0]


def mixed_chain(n):
    """k = 2: a 30-bit and a 61-bit chain prime, a base of 30, 61 and 62 bits"""
    p30, p61, p62 = E.primes_below(30, n, 2), E.primes_below(61, n, 2), E.primes_below(62, n, 2)
    return [p30[0], p61[0]], [p30[1], p61[1], p62[1]], p62[0]


TWO_PASS = [(1 << 14, 3, 3, [2, 1]), (1 << 16, 3, 2, [1, 1])]         # n, k, batch, the rows of its chunks
T_BIG = 257
DOT_WEIGHTS = [3, -2]


def chunks_of(batch, cb):
    return [min(cb, batch - r0) for r0 in range(0, batch, cb)]


def sparse_poly(Q, n, sign, rng):
    """four non-zero coefficients: +-floor(Q / 2) at 0, 1 and n - 1, a uniform one at n / 2"""
    h = Q // 2
    return {0: sign * h, 1: -sign * h, n // 2: rng.randrange(-h, h + 1), n - 1: sign * h}


def dense_of(sp, n):
    out = [0] * n
    for i, x in sp.items():
        out[i] = x
    return out


def sparse_negacyclic(sp, b):
    """sp {index: value} times the dense b (an object array) modulo X^n + 1, over Z: O(len(sp) n)"""
    n = len(b)
    c = np.zeros(n, dtype=object)
    for i, x in sp.items():
        if i == 0:
            c += x * b
        else:
            c[i:] += x * b[:n - i]
            c[:i] -= x * b[n - i:]
    return c


def sparse_tensor(a, b):
    """a = (a0, a1) sparse, b = (b0, b1) dense object arrays -> (d0, d1, d2) over Z"""
    return sparse_negacyclic(a[0], b[0]), sparse_negacyclic(a[0], b[1]) + sparse_negacyclic(a[1], b[0]), sparse_negacyclic(a[1], b[1])


class BigCase:
    """One two-pass shape: per row two sparse ciphertexts a, a2 and a dense b, by their coefficients; their evals; the scaled
    tensor of (a, b) and of DOT_WEIGHTS . ((a, b), (a2, b)) as evals, from the sparse product over Z"""

    def __init__(self, n, k, batch, seed):
        self.n, self.k, self.batch, self.t = n, k, batch, T_BIG
        self.mods, self.aux, self.P = small_chain(n, k)
        Q, h = R.prod(self.mods), R.prod(self.mods) // 2
        rng, r = random.Random(seed), np.random.default_rng(seed)
        self.sp = [[[sparse_poly(Q, n, (-1) ** (c + row + o), rng) for c in range(2)] for row in range(batch)] for o in range(2)]
        hi = r.integers(0, 1 << 62, (batch, 2, n)).astype(object) * (1 << 62) + r.integers(0, 1 << 62, (batch, 2, n)).astype(object)
        self.dense = hi % Q - h                                      # uniform in [-floor(Q / 2), floor(Q / 2)]
        self.a, self.a2 = (np.stack([evals_of(self.mods, n, [dense_of(self.sp[o][row][c], n) for row in range(batch)]) for c in range(2)], axis=1)
                           for o in range(2))
        self.b = np.stack([evals_of(self.mods, n, list(self.dense[:, c])) for c in range(2)], axis=1)

    def tensor(self, w=None):
        """round(t D / Q) as evals [k][3][batch][n]: D the tensor of (a, b), or w[0] (a, b) + w[1] (a2, b)"""
        Q, t = R.prod(self.mods), self.t
        comps = [[], [], []]
        for row in range(self.batch):
            d = sparse_tensor(self.sp[0][row], self.dense[row])
            if w is not None:
                d2 = sparse_tensor(self.sp[1][row], self.dense[row])
                d = [w[0] * x + w[1] * y for x, y in zip(d, d2)]
            for c in range(3):
                comps[c].append((t * d[c] + Q // 2) // Q)
        return np.stack([evals_of(self.mods, self.n, comps[c]) for c in range(3)], axis=1)


ALIGN_SHAPES = [(64, 2, 3), (8192, 4, 5)]
ALIGN_MODES = ("a", "b", "ab", "all")                                # which buffers sit one word past a 16-byte boundary


def align_chain(n, k):
    return (R.chain(n, k), T) if n == 64 else (R.chain(n, k, bq=21, bb=30, bp=31), 257)


REUSE = dict(n=1024, k=2, decrypt_batch=2, mul_batch=3)               # slot 13: k cb n words, then 7 (2k + 1) cb n
