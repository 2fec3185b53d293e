"""Restatement of the BFV inner product, scalar sums and linear transforms on the RNS chain as DESIGN.md §34 defines them, in
Python integers and plain numpy.  The inner product sits on its definition (D = sum_r w_r d^(r) over Z, one scale_round); the
route the device takes (per pair: centred extension, the tensor modulo every prime of Q u B, the weighted accumulation into
canonical words; then steps 3 and 4 of §33 once) is restated beside it so that tests/test_bfv_dot_cpu.py can prove the two
equal.  The pieces of §33 are those of tests/_bfv_rns_numpy.py.  Nothing here calls the library under test."""
import numpy as np

import _bfv_rns_numpy as R
import _ckks_eval_numpy as E

U64, I64 = np.uint64, np.int64
MAX_COUNT = 64
FOLD_PAIRS = 4                  # kMacChunk / 2 of ckks_rns_tensorsum_kernel: what count = 5 crosses


def admitted(mods, aux, t, n, W):
    return R.prod(aux) > t * n * R.prod(mods) * W + 1


def max_weight(mods, aux, t, n):
    return (R.prod(aux) - 2) // (t * n * R.prod(mods))


def centred(x, t):
    x = int(x) % t
    return x - t if x > t // 2 else x


def weight_sum(count, w):
    return count if w is None else sum(abs(int(x)) for x in w)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def tensor_int(a0, a1, b0, b1):
    """the negacyclic tensor over Z of one pair of ciphertexts given by their coefficient lists"""
    d1 = [x + y for x, y in zip(R.negacyclic(a0, b1), R.negacyclic(a1, b0))]
    return R.negacyclic(a0, b0), d1, R.negacyclic(a1, b1)


def sum_int(pairs, w):
    """pairs [(a0, a1, b0, b1)] coefficient lists, w integers or None -> D = sum_r w_r d^(r), three coefficient lists"""
    n = len(pairs[0][0])
    D = [[0] * n for _ in range(3)]
    for r, p in enumerate(pairs):
        wr = 1 if w is None else int(w[r])
        for c, d in enumerate(tensor_int(*p)):
            D[c] = [x + wr * y for x, y in zip(D[c], d)]
    return D


def dot_tensor(mods, t, pairs, w):
    """pairs [(a, b)] of evals [k][2][batch][n], w signed integers or None -> round(t sum_r w_r d^(r) / Q) as evals [k][3][batch][n],
    from the definition"""
    k, _, batch, n = pairs[0][0].shape
    Q = R.prod(mods)
    co = [[[R.coeffs_centred(mods, n, x[:, c]) for c in range(2)] for x in pair] for pair in pairs]
    comps = [[], [], []]
    for row in range(batch):
        D = sum_int([(a[0][row], a[1][row], b[0][row], b[1][row]) for a, b in co], w)
        for c in range(3):
            comps[c].append([R.scale_round(x, t, Q) for x in D[c]])
    out = np.empty((k, 3, batch, n), dtype=U64)
    for c in range(3):
        out[:, c] = R.to_evals(mods, n, comps[c])
    return out


def dot(mods, P, t, rlk, pairs, w):
    return E.relinearize(mods, P, rlk, dot_tensor(mods, t, pairs, w))


# ---- the route of the device, restated --------------------------------------------------------------------------------------------
def negacyclic_mod(a, b, p):
    return [x % p for x in R.negacyclic([x % p for x in a], [x % p for x in b])]


def route_accumulate(mods, aux, pairs, w):
    """per pair: the operands' residues modulo Q (what the caller's ciphertexts hold), extended centred to B by Garner's digits;
    the tensor modulo every prime of Q u B; the weight's canonical residue folded into a0 and a1; the three sums carried as
    canonical words from pair to pair -> D's residues [2k + 1][3][n]"""
    primes = list(mods) + list(aux)
    n = len(pairs[0][0])
    D = [[[0] * n for _ in range(3)] for _ in primes]
    for r, ops in enumerate(pairs):
        wr = 1 if w is None else int(w[r])
        res = []                                                     # [operand][prime][n]
        for op in ops:
            ext = [R.garner_extend(mods, aux, [x % q for q in mods], True) for x in op]
            res.append([[x % q for x in op] for q in mods] + [[e[j] for e in ext] for j in range(len(aux))])
        for l, p in enumerate(primes):
            wp = wr % p                                              # a negative weight as its canonical residue
            a0, a1 = [wp * x % p for x in res[0][l]], [wp * x % p for x in res[1][l]]
            b0, b1 = res[2][l], res[3][l]
            d = (negacyclic_mod(a0, b0, p), [(x + y) % p for x, y in zip(negacyclic_mod(a0, b1, p), negacyclic_mod(a1, b0, p))], negacyclic_mod(a1, b1, p))
            for c in range(3):
                D[l][c] = [(x + y) % p for x, y in zip(D[l][c], d[c])]
    return D


def route_scale_residues(mods, aux, t, dq, db):
    """steps 3 and 4 of §33 on one integer given by its residues dq modulo Q's primes and db modulo B's"""
    Q = R.prod(mods)
    uq = [(t * x + Q // 2) % q for x, q in zip(dq, mods)]
    ub = [(t * x + Q // 2) % b for x, b in zip(db, aux)]
    r = R.garner_extend(mods, aux, uq, False)
    y = [(ub[j] - r[j]) * pow(Q, -1, b) % b for j, b in enumerate(aux)]
    return R.garner_extend(aux, mods, y, True)


def route_dot(mods, aux, t, pairs, w):
    """the whole route on coefficient lists -> [k][3][n] residues of round(t D / Q)"""
    k, n = len(mods), len(pairs[0][0])
    D = route_accumulate(mods, aux, pairs, w)
    out = [[[0] * n for _ in range(3)] for _ in mods]
    for c in range(3):
        for e in range(n):
            y = route_scale_residues(mods, aux, t, [D[i][c][e] for i in range(k)], [D[k + j][c][e] for j in range(k + 1)])
            for i in range(k):
                out[i][c][e] = y[i]
    return out


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def bound_pair(Q, n, sign):
    """a pair whose d1 reaches sign n Q^2 / 2 (to the rounding of floor(Q / 2)) in its top coefficient: all four polynomials
    constant +-floor(Q / 2) in every coefficient"""
    h = Q // 2
    return [h] * n, [h] * n, [sign * h] * n, [sign * h] * n


def random_pair(rng, Q, n):
    return tuple([rng.randrange(-(Q // 2), Q // 2 + 1) for _ in range(n)] for _ in range(4))


def signed_weights(count, t, seed):
    """mixed signs, centred modulo t, none zero: +-1, +-2, the extremes +-floor(t / 2), and values between"""
    import random

    rng = random.Random(seed)
    pool = [1, -1, 2, -2, t // 2, -(t // 2 - 1), 3, -5]
    return [pool[i] if i < len(pool) else rng.choice([-1, 1]) * rng.randrange(1, t // 2) for i in range(count)]


# ---- diagonals and baby-step giant-step over Z_t, on 2 x n/2 slots -------------------------------------------------------------------
def matvec(M, x, t):
    """M [2][N][N], x [2][N] -> out[r] = M[r] x[r] mod t, in Python integers"""
    M, x = np.asarray(M).astype(object), np.asarray(x).astype(object)
    return np.stack([(M[r] @ x[r]) % t for r in range(2)]).astype(I64)


def diagonals(M, t):
    """-> {d: [2][N]} with diag_d[r][c] = M[r][c][(c + d) mod N] mod t"""
    M = np.mod(np.asarray(M).astype(object), t).astype(I64)
    N = M.shape[1]
    c = np.arange(N)
    return {d: M[:, c, (c + d) % N] for d in range(N)}


def diag_apply(M, x, t):
    """sum_d diag_d * roll(x, -d) mod t: what RnsCiphertext.diag_sum computes from one output of all N diagonals"""
    acc = np.zeros(np.asarray(x).shape, dtype=object)
    for d, dg in diagonals(M, t).items():
        acc = (acc + dg.astype(object) * np.roll(np.asarray(x).astype(object), -d, axis=1)) % t
    return acc.astype(I64)


def bsgs_apply(n1, baby, giant, rows, x, t):
    """sum_a roll(sum_b rows[a][b] * roll(x, -baby[b]), -n1 giant[a]) mod t"""
    x = np.asarray(x).astype(object)
    acc = np.zeros(x.shape, dtype=object)
    for a, j in enumerate(giant):
        inner = np.zeros(x.shape, dtype=object)
        for b, i in enumerate(baby):
            inner = (inner + np.asarray(rows[a][b]).astype(object) * np.roll(x, -i, axis=1)) % t
        acc = (acc + np.roll(inner, -n1 * j, axis=1)) % t
    return acc.astype(I64)


def banded(rng, N, t, width):
    M = np.zeros((N, N), dtype=I64)
    c = np.arange(N)
    for d in range(width):
        M[c, (c + d) % N] = rng.integers(1, t, N)
    return M


def single_diagonal(rng, N, t, d):
    M = np.zeros((N, N), dtype=I64)
    c = np.arange(N)
    M[c, (c + d) % N] = rng.integers(1, t, N)
    return M
