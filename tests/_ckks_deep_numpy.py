"""Restatement of CKKS on a deep RNS chain as DESIGN.md §36 defines it: the hybrid key switch with grouped digits and several
special primes, on tests/_ckks_eval_numpy.py's transforms, samplers and chain.  Nothing here calls the library under test.

    chain       primes q_0 .. q_{L-1} (1 <= L <= 32), special primes p_0 .. p_{alpha-1} (1 <= alpha <= 8, P their product), all
                distinct, 1 mod 2n, below 2^62
    groups      G_j(l) = limbs [j alpha, min((j + 1) alpha, l)), j alpha < l; dnum = ceil(L / alpha); Q_j(l) the group's product
    admission   P >= Q_j(L) for every j
    key         [dnum][L + alpha][2][n] evals: key[j][i] = (-a_ji s + e_j + [i in G_j(L)] (P mod q_i) s', a_ji), row first_row + j
    switch      x_j the centred integer of d's residues over G_j(l); D_ji = x_j mod m_i (i in G_j: d's own evals);
                t_i = sum_j D_ji (.) key[j][col(i)]; y the centred integer of t modulo P; r_i = (t_i - y) P^-1 mod q_i
    garner      the route of the kernel: mixed-radix digits of the group's residues, the centring by comparing them with the digits
                of floor(M / 2), one sum of digit times weight per target
"""
import numpy as np

import _ckks_eval_numpy as E
import _ckks_galois_numpy as G

U64, I64 = np.uint64, np.int64
MAX_LIMBS, MAX_SPECIALS = 32, 8
MOD_LIMIT = 1 << 62
CHUNK_WORDS = 1 << 21


# ---- groups, admission -------------------------------------------------------------------------------------------------------------
def dnum(limbs, alpha):
    return -(-limbs // alpha)


def groups(limbs, alpha):
    """-> [range of limbs of G_j(limbs)]"""
    return [range(j, min(j + alpha, limbs)) for j in range(0, limbs, alpha)]


def product(ms):
    out = 1
    for m in ms:
        out *= int(m)
    return out


def admits(mods, specials):
    P = product(specials)
    return all(P >= product(mods[i] for i in g) for g in groups(len(mods), len(specials)))


def check_chain(n, mods, specials):
    """the rejections of DeepParam and of the C ABI's chain check, as ValueError"""
    if not 1 <= len(mods) <= MAX_LIMBS:
        raise ValueError("the chain has 1 to 32 primes")
    if not 1 <= len(specials) <= MAX_SPECIALS:
        raise ValueError("there are 1 to 8 special primes")
    allp = list(mods) + list(specials)
    if len(set(allp)) != len(allp):
        raise ValueError("the primes must be distinct")
    if any(p >= MOD_LIMIT for p in allp):
        raise ValueError("every prime is below 2^62")
    if any(p % (2 * n) != 1 for p in allp):
        raise ValueError("every prime is 1 modulo 2n")
    if not admits(mods, specials):
        raise ValueError("P must not be below the product of a digit group")


# ---- the extension: the definition and the kernel's route ----------------------------------------------------------------------------
def centred_int(src, res):
    """res [s][...] canonical residues -> object array of the integers in (-M / 2, M / 2]"""
    return E.crt_centred(list(src), list(res))[0]


def extend_crt(src, res, dst):
    """the definition: the centred integer modulo every target -> u64 [t][...]"""
    x = centred_int(src, res)
    return np.stack([(x % int(p)).astype(U64) for p in dst])


def garner_tables(src, dst):
    s = len(src)
    inv = [[pow(src[j], -1, src[i]) if j < i else 0 for i in range(s)] for j in range(s)]
    h, half = product(src) // 2, []
    for m in src:
        half.append(h % m)
        h //= m
    W = [[product(src[:j]) % p for p in dst] for j in range(s)]
    return inv, half, W, [product(src) % p for p in dst]


def extend_garner(src, res, dst):
    """the kernel's route on Python integers -> u64 [t][...]"""
    src, dst = [int(m) for m in src], [int(p) for p in dst]
    inv, half, W, pM = garner_tables(src, dst)
    x = [E._obj(r) for r in res]
    a = []
    for i, q in enumerate(src):
        v = x[i]
        for j in range(i):
            v = ((v + q - a[j] % q) * inv[j][i]) % q
        a.append(v)
    gt = np.zeros(x[0].shape, dtype=bool)
    eq = np.ones(x[0].shape, dtype=bool)
    for i in reversed(range(len(src))):
        diff = a[i] != half[i]
        gt = np.where(eq & diff, a[i] > half[i], gt)
        eq = eq & ~diff
    out = []
    for t, p in enumerate(dst):
        v = sum(a[j] * W[j][t] for j in range(len(src))) % p
        out.append(np.where(gt, (v + p - pM[t]) % p, v).astype(U64))
    return np.stack(out)


# ---- keys ----------------------------------------------------------------------------------------------------------------------------
def switch_key(seed, first_row, s, mods, specials, cdt, g=None):
    """-> evals [dnum][L + alpha][2][n]; g None: the relinearisation key (s' = s^2), else the Galois key of sigma_g"""
    n, L, alpha = len(s), len(mods), len(specials)
    P = product(specials)
    out = np.zeros((dnum(L, alpha), L + alpha, 2, n), dtype=U64)
    for j, grp in enumerate(groups(L, alpha)):
        for i, q in enumerate(list(mods) + list(specials)):
            ev = E.fwd(q, n, np.stack(E.public_key_coeffs(seed, first_row + j, s, q, cdt)))
            if i in grp:
                se = E.fwd(q, n, E.residues(s, q))
                sp = E.pmul(q, se, se) if g is None else G.galois_evals(se, g)
                ev[0] = E.padd(q, ev[0], E.pmul(q, U64(P % q), sp))
            out[j, i] = ev
    return out


# ---- the key switch --------------------------------------------------------------------------------------------------------------------
def digits(mods, specials, d2):
    """D [l + alpha][groups][batch][n] evals for d2 [l][batch][n]: target i first, digit group j second"""
    l, alpha, n = len(mods), len(specials), d2.shape[-1]
    targets = list(mods) + list(specials)
    coef = [E.inv(q, n, d2[i]) for i, q in enumerate(mods)]
    D = [[None] * dnum(l, alpha) for _ in targets]
    for j, grp in enumerate(groups(l, alpha)):
        x = centred_int([mods[i] for i in grp], [coef[i] for i in grp])
        for i, m in enumerate(targets):
            D[i][j] = d2[i] if i in grp else E.fwd(m, n, (x % int(m)).astype(U64))
    return np.stack([np.stack(row) for row in D])


def key_switch_sums(mods, specials, key, d2, D=None):
    """t [l + alpha][2][batch][n] evals; key may be that of a longer chain (its columns L + m are the special primes')"""
    l, alpha = len(mods), len(specials)
    kl = key.shape[1] - alpha
    D = digits(mods, specials, d2) if D is None else D
    t = []
    for i, m in enumerate(list(mods) + list(specials)):
        col = i if i < l else kl + (i - l)
        acc = np.zeros((2,) + d2.shape[1:], dtype=U64)
        for j in range(D.shape[1]):
            for c in range(2):
                acc[c] = E.padd(m, acc[c], E.pmul(m, D[i, j], key[j, col, c]))
        t.append(acc)
    return t


def mod_down(mods, specials, t, add=None):
    """r_i = (t_i - y) P^-1 (+ add_i) mod q_i, y the centred integer of t modulo P in coefficients -> [l][2][batch][n]"""
    l, n = len(mods), t[0].shape[-1]
    P = product(specials)
    y = centred_int(specials, [E.inv(p, n, t[l + m]) for m, p in enumerate(specials)])
    out = []
    for i, q in enumerate(mods):
        r = E.pmul(q, E.psub(q, t[i], E.fwd(q, n, (y % int(q)).astype(U64))), U64(pow(P, -1, q)))
        out.append(r if add is None else E.padd(q, r, add[i]))
    return np.stack(out)


def relinearize(mods, specials, key, d):
    """d [l][3][batch][n] -> [l][2][batch][n]"""
    return mod_down(mods, specials, key_switch_sums(mods, specials, key, d[:, 2]), add=d[:, :2])


def mul(mods, specials, key, a, b):
    return relinearize(mods, specials, key, E.tensor(mods, a, b))


def apply_galois(mods, specials, gk, ct, g):
    p = G.galois_evals(ct, g)
    return relinearize(mods, specials, gk, np.stack([p[:, 0], np.zeros_like(p[:, 0]), p[:, 1]], axis=1))


def rescale(mods, c):
    return E.rescale(mods, c)


# ---- the workspace and the chunk (include/fhe_ntt.h) ---------------------------------------------------------------------------------
def slabs(limbs, alpha):
    """slabs of one ciphertext of a chunk: the tensor 3l, C l, D (l + alpha) ng - l, T 2 (l + alpha), E 2l"""
    return (limbs + alpha) * dnum(limbs, alpha) + 7 * limbs + 2 * alpha


def chunk_rows(n, limbs, alpha, batch):
    return min(batch, max(1, (CHUNK_WORDS // n) // slabs(limbs, alpha)))


def workspace_bytes(n, limbs, alpha, batch):
    if not (n >= 2 and n & (n - 1) == 0 and n <= 1 << 19 and 1 <= limbs <= MAX_LIMBS and 1 <= alpha <= MAX_SPECIALS and batch):
        return 0
    res = min(batch, max(1, (CHUNK_WORDS // n) // (2 * limbs)))
    return 8 * max(slabs(limbs, alpha) * n * chunk_rows(n, limbs, alpha, batch), 2 * limbs * n * res)


# ---- the noise of one key switch (§36) ------------------------------------------------------------------------------------------------
def switch_noise_bound(n, limbs, alpha, qj_over_p, b_err=E.B_ERR):
    """|r0 + r1 s - d s'|_inf <= dnum n B max_j Q_j / (2 P) + (n + 1) / 2: every digit |x_j| <= Q_j / 2 meets an error row
    |e_j| <= B in a negacyclic product of n terms, divided by P; the rounding y0 + y1 s of the division adds (1 + n) / 2"""
    return dnum(limbs, alpha) * n * b_err * qj_over_p / 2 + (n + 1) / 2


# ---- chains for the tests ---------------------------------------------------------------------------------------------------------------
def case_chain(n, L, alpha, bq=40, bp=None):
    """L chain primes below 2^bq and alpha special primes below 2^bp (default: one bit more, so that P >= every group's product)"""
    bp = bq + 1 if bp is None else bp
    return E.primes_below(bq, n, L), E.primes_below(bp, n, alpha)


def e2e_chain(n, L, alpha):
    """q_0 and the special primes near 2^55, the scale primes near 2^40"""
    big = E.primes_below(55, n, 1 + alpha)
    return [big[0]] + E.primes_below(40, n, L - 1), big[1:]
