"""Case lists, planted rows and replays of the deep CKKS chain's sweep: tests/test_ckks_deep_shapes_cpu.py proves
them, tests/test_ckks_deep_shapes_gpu.py runs them.  Nothing here calls the library under test; the restatements are the existing
ones (tests/_ckks_deep_numpy.py, tests/_ckks_deep_linear_numpy.py, tests/_ckks_eval_numpy.py).

    A  widths     every prime just below 2^62 at four shapes, uniform words and the bound-reaching rows; the fold schedules of
                  the two sum kernels replayed; chains of 30, 37, 61 and 62-bit primes in both orders inside a group; one integer
                  per digit position either side of floor(M / 2), on the digit groups and on t modulo P
    B  ladder     every n = 2^1 .. 2^16 that §36 / §37 left out, at (L, alpha, l) = (5, 2, 4)
    C  counts     diag_sum at 32, 33 and 256 elements, 4 and 64 outputs; galois_dev at 256
    D  chunks     the clamps of the key switch, the diagonal sum and the rescale; the rescale's chunk crossed; slot 14 reused
    E  alignment  every entry point with the inputs, the outputs or both one word past a 16-byte boundary
"""
import functools

import numpy as np

import _ckks_deep_linear_numpy as DL
import _ckks_deep_numpy as D
import _ckks_eval_numpy as E

U64 = np.uint64
WORD = 1 << 128

# ---- A1: every prime just below 2^62 ---------------------------------------------------------------------------------------------
LIMIT_SHAPES = [(32, 1, 32), (17, 8, 17), (9, 3, 7), (5, 2, 4)]             # (L, alpha, l)
WIDTH_NS, WIDTH_BATCHES = (8, 64), (1, 3)
DIAG_COUNTS, DIAG_OUTPUTS = (3, 17), 2


@functools.lru_cache(None)
def limit_chain(n, L, alpha):
    """the first alpha primes below 2^62 are the special primes, the next L the chain: every special prime is above every chain
    prime, so P is above every group's product"""
    ps = E.primes_below(62, n, alpha + L)
    return ps[alpha:], ps[:alpha]


def pool_elements(n):
    """the three elements whose keys a diagonal sum draws on: two rotations and the conjugation, reduced modulo 2n"""
    return [5 % (2 * n), 2 * n - 1, 25 % (2 * n)]


def diag_elements(n, count, identity=(1,)):
    """`count` elements from the pool in turn, the identity at the places `identity`"""
    pool = pool_elements(n)
    return [1 if r in identity else pool[r % 3] for r in range(count)]


def pool_keys(mods, specials, n, rng, key_mods=None, fill=None):
    """{g: key} over the pool: canonical uniform words (fill None) or m_i - 1 throughout"""
    km = list(mods if key_mods is None else key_mods) + list(specials)
    ng = D.dnum(len(km) - len(specials), len(specials))
    r = np.random.default_rng(rng)
    out = {}
    for g in pool_elements(n):
        if g != 1 and g not in out:
            out[g] = np.stack([np.stack([r.integers(0, q, (2, n), dtype=np.uint64) if fill is None else np.full((2, n), q - 1, dtype=U64) for q in km])
                               for _ in range(ng)])
    return out


def keys_of(pool, gs):
    return [None if g == 1 else pool[g] for g in gs]


def top_key(key_mods, specials, n):
    """a switching key whose every word is m_i - 1"""
    km = list(key_mods) + list(specials)
    return np.stack([np.stack([np.full((2, n), q - 1, dtype=U64) for q in km]) for _ in range(D.dnum(len(key_mods), len(specials)))])


def top_pts(mods, specials, n, outputs, count):
    return np.stack([np.full((outputs, count, n), q - 1, dtype=U64) for q in list(mods) + list(specials)], axis=2)


def uniform_key(key_mods, specials, n, rng):
    r = np.random.default_rng(rng)
    km = list(key_mods) + list(specials)
    return np.stack([np.stack([r.integers(0, q, (2, n), dtype=np.uint64) for q in km]) for _ in range(D.dnum(len(key_mods), len(specials)))])


def minus_one_ct(mods, n, batch, comps, rng, comp):
    """uniform words with component `comp` of batch row 0 the constant polynomial -1: every eval q_i - 1"""
    ct = E.case_ct(mods, n, batch, comps, rng)
    for i, q in enumerate(mods):
        ct[i, comp, 0] = q - 1
    return ct


def minus_one_pair(mods, n, batch, rng):
    """(a, b) whose tensor has d2 = -1 in batch row 0: a1 the constant 1, b1 the constant -1"""
    a, b = E.case_ct(mods, n, batch, 2, rng), minus_one_ct(mods, n, batch, 2, rng + 1, 1)
    a[:, 1, 0] = 1
    return a, b


def galois_many(mods, specials, keys, gs, ct, Dg=None):
    """D.apply_galois for every element of gs from ONE set of digits of the unpermuted c1 (the hoisting of §36: the digits of
    sigma_g(c1) are the digits of c1 read at pi_g), which the CPU module holds against D.apply_galois -> [count][l][2][batch][n]"""
    import _ckks_galois_numpy as G

    Dg = D.digits(mods, specials, ct[:, 1]) if Dg is None else Dg
    done, out = {}, []
    for key, g in zip(keys, gs):
        if (id(key), g) not in done:
            perm = G.galois_perm(ct.shape[-1], g)
            add = np.stack([ct[:, 0][..., perm], np.zeros_like(ct[:, 0])], axis=1)
            done[id(key), g] = D.mod_down(mods, specials, DL.key_sums(mods, specials, key, g, Dg), add=add)
        out.append(done[id(key), g])
    return out


# ---- A2: the fold schedules, replayed on words m - 1 with the largest carry-over a fold can leave ---------------------------------------
def eighth(j):
    return j % 8 == 0


def keymac_peak(q, k, fold=eighth):
    """the largest value an accumulator of ckks_deep_keymac_kernel holds over k digits: every term (q - 1)^2, a fold before digit
    j > 0 where fold(j), leaving at most q - 1"""
    acc = peak = 0
    for j in range(k):
        if j and fold(j):
            acc = q - 1
        acc += (q - 1) ** 2
        peak = max(peak, acc)
    return peak


def diagmac_peaks(q, k, count, inner=eighth, outer=eighth, addend=True, carry_launches=True):
    """-> (inner, outer): the largest values of a0 / a1 and of u_o in ckks_deep_diagmac_kernel.  Inner: the addend's term, then k
    digits.  Outer: groups of 16 elements, a group after the first starting from the canonical word CARRY read"""
    t = (q - 1) ** 2
    acc = peak_in = t if addend else 0
    for j in range(k):
        if j and inner(j):
            acc = q - 1
        acc += t
        peak_in = max(peak_in, acc)
    peak_out = 0
    for e0 in range(0, count, DL.GROUP):
        u = q - 1 if e0 and carry_launches else 0
        for r in range(min(DL.GROUP, count - e0)):
            if r and outer(r):
                u = q - 1
            u += t
            peak_out = max(peak_out, u)
    return peak_in, peak_out


def extend_peak(src, W):
    """the largest 128-bit sum of ckks_deep_extend_kernel: digits m_j - 1 against the weights W[j] of one target"""
    return sum((m - 1) * w for m, w in zip(src, W))


# ---- A3: mixed widths ----------------------------------------------------------------------------------------------------------------
MIXED_ALPHAS = (2, 4, 8)
MIXED_ORDERS = ("up", "down")                                               # small before large, large before small inside a group
DOWN_ALPHAS = (2, 3, 8)                                                      # the modulus-down's plants: t modulo P


@functools.lru_cache(None)
def mixed_chain(n, alpha, order):
    """L = 2 alpha + 1 limbs: two full groups and one limb over.  A group is 30, 62, 37, 61, 30, 62, 37, 61 bits cut to alpha
    ("up"), or that reversed ("down": a prime just under 2^62 or 2^61 before the 30-bit one).  The special primes are the first
    alpha below 2^62, above every chain prime"""
    L = 2 * alpha + 1
    pools = {30: E.primes_below(30, n, L), 37: E.primes_below(37, n, L), 61: E.primes_below(61, n, L), 62: E.primes_below(62, n, alpha + L)[alpha:]}
    sps = E.primes_below(62, n, alpha)
    mods = []
    for j in range(0, L, alpha):
        bits = [30, (62, 61, 37)[j // alpha % 3]] if alpha == 2 else ([30, 62, 37, 61] * 2)[:alpha]   # alpha = 2: the neighbour changes by group
        grp = [pools[b].pop(0) for b in bits]
        mods += grp if order == "up" else grp[::-1]
    return mods[:L], sps


def half_digits(src):
    h, out = D.product(src) // 2, []
    for m in src:
        out.append(h % m)
        h //= m
    return out


def from_digits(src, a):
    x, w = 0, 1
    for m, d in zip(src, a):
        assert 0 <= d < m
        x, w = x + d * w, w * m
    return x


def depth_integers(src):
    """[(decided at digit, above floor(M / 2)?, x in [0, M))]: for every position i the integers whose mixed-radix digits are those
    of floor(M / 2) above i, one more or one less at i, and below i those of floor(M / 2), all zero, or all m_j - 1"""
    src = [int(m) for m in src]
    h = half_digits(src)
    out = []
    for i in range(len(src)):
        for step in (1, -1):
            if not 0 <= h[i] + step < src[i]:
                continue
            for low in (h[:i], [0] * i, [m - 1 for m in src[:i]]):
                out.append((i, step > 0, from_digits(src, list(low) + [h[i] + step] + h[i + 1:])))
    return out


def planted_integers(src):
    """the edge integers of §36's test, then depth_integers -> [x in [0, M)]"""
    M = D.product(src)
    return [0, 1, M // 2, M // 2 + 1, M - 1, M // 2 - 1, M // 3, 2] + [x for _, _, x in depth_integers(src)]


def planted_rows(mods, alpha, n):
    """d2 [L][batch][n] evals whose group integers run through planted_integers(group) coefficient by coefficient, the rest
    uniform; batch as many rows as the longest list needs"""
    L = len(mods)
    lists = [planted_integers([mods[i] for i in grp]) for grp in D.groups(L, alpha)]
    batch = -(-max(len(x) for x in lists) // n)
    r = np.random.default_rng(L * n + alpha)
    coef = np.stack([r.integers(0, q, (batch, n), dtype=np.uint64) for q in mods])
    for grp, xs in zip(D.groups(L, alpha), lists):
        for i in grp:
            flat = coef[i].reshape(-1)
            flat[:len(xs)] = np.array([x % mods[i] for x in xs], dtype=U64)
    return np.stack([E.fwd(q, n, coef[i]) for i, q in enumerate(mods)]), coef


def down_case(n, alpha, L=4):
    """the modulus-down's plants: zero "keys" with one chosen column (§36's construction).  Group 0's integer is the constant 1,
    so t modulo p_m is key[0][L + m][c] itself; the planted integers of the special primes go 2n a call, n a component.
    -> (mods, specials, d, [key])"""
    mods, sps = limit_chain(n, L, alpha)
    ys = planted_integers(sps)
    ys += [ys[0]] * (-len(ys) % (2 * n))
    one = np.zeros(n, dtype=U64)
    one[0] = 1
    d = np.zeros((L, 3, 1, n), dtype=U64)
    for i in range(min(alpha, L)):
        d[i, 2, 0] = E.fwd(mods[i], n, one)
    keys = []
    for t in range(0, len(ys), 2 * n):
        key = np.zeros((D.dnum(L, alpha), L + alpha, 2, n), dtype=U64)
        for m, p in enumerate(sps):
            for c in range(2):
                key[0, L + m, c] = E.fwd(p, n, np.array([y % p for y in ys[t + c * n:t + (c + 1) * n]], dtype=U64))
        keys.append(key)
    return mods, sps, d, keys, ys


# ---- B: the ring ladder ------------------------------------------------------------------------------------------------------------------
LADDER_SHAPE = (5, 2, 4)
RAN_BEFORE = (2, 8, 64, 2048)                                                # the n of §36's and §37's word-for-word sweeps
LADDER = [(1 << L, 3 if L <= 13 else 2) for L in range(1, 17) if 1 << L not in RAN_BEFORE]
KEY_CUT = 1 << 13                                                            # the keys are the samplers' up to here, uniform words above
LADDER_DIAG, LADDER_OUTPUTS = [1, 5, 5], 2

# ---- C: counts ------------------------------------------------------------------------------------------------------------------------
COUNT_SHAPES = [(5, 2, 5), (3, 8, 3)]
COUNT_N, COUNT_BATCH = 8, 2
# (count, outputs, the places of the identity): first, 16th, 17th and last; elements 32 .. 47 of 256 are a whole group of identities
COUNT_CASES = [(32, 4, (0, 15, 31)), (33, 4, (0, 15, 16, 32)), (33, DL.MAX_OUTPUTS, (16,)), (256, 4, (0, 15, 16, 255) + tuple(range(32, 48))),
               (256, 1, ())]
LAUNCH_CASE = (33, 4)

# ---- D: chunks, clamps, workspace --------------------------------------------------------------------------------------------------------
CLAMP = (1 << 14, 2, 11, 2)                                                  # n, alpha, limbs, batch: 159 and 152 slabs, 128 a chunk
RESCALE_CROSSED = (1 << 14, 16, 5)                                           # n, limbs, batch: chunks of 4 + 1
RESCALE_CLAMPED = (1 << 16, 17, 2)                                           # 32 // 34 = 0


def rescale_chunk(n, limbs, batch):
    return min(batch, max(1, (D.CHUNK_WORDS // n) // (2 * limbs)))


def chunks_of(batch, cb):
    return [min(cb, batch - r) for r in range(0, batch, cb)]


REUSE = dict(n=1024, shape=(5, 2, 5), rescale_batch=1, mul_batch=3, diag_batch=2)

# ---- E: alignment --------------------------------------------------------------------------------------------------------------------------
ALIGN_SHAPES = [(64, (9, 3, 7), 3), (8192, (12, 4, 12), 2)]
ALIGN_MODES = ("all", "inputs", "outputs")
ENTRIES = ("relin_key", "galois_key", "relinearize", "mul", "galois", "diag_sum", "rescale")
