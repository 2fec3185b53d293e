"""Restatement of BFV on an RNS modulus chain as DESIGN.md §33 defines it, in Python integers: the exact basis extension, the
scaled tensor floor((t d + floor(Q / 2)) / Q), message scaling, decryption and the batch encoder sit directly on their
definitions (the CRT, the product over Z, the quotient); the route the device takes (Garner's digits, steps 1 - 4) is restated
beside them so that tests/test_bfv_rns_cpu.py can prove the two equal.  The transforms, the keys and the relinearisation are
those of tests/_ckks_eval_numpy.py.  Nothing here calls the library under test."""
import numpy as np

import _ckks_eval_numpy as E

U64, I64 = np.uint64, np.int64
CHUNK_WORDS = 1 << 21


def prod(ms):
    out = 1
    for m in ms:
        out *= int(m)
    return out


def chain(n, k, bq=59, bb=61, bp=62):
    """-> (q_0 .. q_{k-1}, b_0 .. b_k, P): distinct primes 1 modulo 2n, the chain just below 2^bq, the auxiliary base below 2^bb,
    the special prime below 2^bp"""
    return E.primes_below(bq, n, k), E.primes_below(bb, n, k + 1), E.primes_below(bp, n, 1)[0]


def admitted(mods, aux, t, n):
    return prod(aux) > t * n * prod(mods) + 1


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def crt(mods, res):
    """the integer in [0, M) with residues res[i] modulo mods[i]"""
    M = prod(mods)
    return sum(int(r) * (M // m) * pow(M // m, -1, m) for r, m in zip(res, mods)) % M


def centre(x, M):
    return x - M if x > M // 2 else x


def extend(src, dst, res, centred):
    """res [len(src)][count] -> [len(dst)][count] uint64: the residues of the same integers, taken in [0, M) or in (-M/2, M/2]"""
    M = prod(src)
    res = np.asarray(res, dtype=U64)
    out = np.empty((len(dst), res.shape[1]), dtype=U64)
    for e in range(res.shape[1]):
        x = crt(src, res[:, e])
        if centred:
            x = centre(x, M)
        for j, p in enumerate(dst):
            out[j, e] = x % p
    return out


def scale_round(d, t, Q):
    """floor((t d + floor(Q / 2)) / Q): t d / Q rounded to nearest, Q odd"""
    return (t * d + Q // 2) // Q


def negacyclic(a, b):
    """the product of two integer polynomials modulo X^n + 1, over Z: schoolbook for small n, otherwise one product of
    integers with the coefficients |c| < 2^(S - 1) packed S bits apart"""
    n = len(a)
    a, b = [int(x) for x in a], [int(x) for x in b]
    if n <= 64:
        c = [0] * n
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                if i + j < n:
                    c[i + j] += x * y
                else:
                    c[i + j - n] -= x * y
        return c
    bound = n * max(map(abs, a), default=0) * max(map(abs, b), default=0)
    S = 8 * ((bound.bit_length() + 2 + 7) // 8)
    beta, ones = 1 << (S - 1), ((1 << (2 * n * S)) - 1) // ((1 << S) - 1)

    def pack(x):
        return int.from_bytes(b"".join((v + beta).to_bytes(S // 8, "little") for v in x), "little") - beta * (((1 << (n * S)) - 1) // ((1 << S) - 1))

    raw = (pack(a) * pack(b) + beta * ones).to_bytes(2 * n * S // 8 + 1, "little")
    full = [int.from_bytes(raw[i * S // 8:(i + 1) * S // 8], "little") - beta for i in range(2 * n)]
    return [full[i] - full[i + n] for i in range(n)]


def coeffs_centred(mods, n, ev):
    """evals [k][rows][n] -> rows x n Python integers centred in Q"""
    Q = prod(mods)
    co = np.stack([E.inv(q, n, ev[i]) for i, q in enumerate(mods)])
    return [[centre(crt(mods, co[:, r, e]), Q) for e in range(n)] for r in range(co.shape[1])]


def to_evals(mods, n, rows):
    """rows x n Python integers -> evals [k][rows][n]"""
    return np.stack([E.fwd(q, n, np.array([[x % q for x in row] for row in rows], dtype=U64)) for q in mods])


def tensor(mods, t, a, b):
    """a, b [k][2][batch][n] evals -> the scaled tensor [k][3][batch][n] evals, from the definition"""
    k, _, batch, n = a.shape
    Q = prod(mods)
    ac = [coeffs_centred(mods, n, a[:, c]) for c in range(2)]
    bc = [coeffs_centred(mods, n, b[:, c]) for c in range(2)]
    out = np.empty((k, 3, batch, n), dtype=U64)
    comps = [[], [], []]
    for r in range(batch):
        d0 = negacyclic(ac[0][r], bc[0][r])
        d1 = [x + y for x, y in zip(negacyclic(ac[0][r], bc[1][r]), negacyclic(ac[1][r], bc[0][r]))]
        d2 = negacyclic(ac[1][r], bc[1][r])
        for c, d in enumerate((d0, d1, d2)):
            comps[c].append([scale_round(x, t, Q) for x in d])
    for c in range(3):
        out[:, c] = to_evals(mods, n, comps[c])
    return out


def mul(mods, P, t, rlk, a, b):
    return E.relinearize(mods, P, rlk, tensor(mods, t, a, b))


def scale_msg(mods, t, m):
    """m [batch][n] in [0, t) -> int64 [k][batch][n]: floor(Q / t) m mod q_i, centred"""
    delta = prod(mods) // t
    m = np.asarray(m, dtype=U64)
    out = np.empty((len(mods),) + m.shape, dtype=I64)
    for i, q in enumerate(mods):
        w = (m.astype(object) * (delta % q)) % q
        out[i] = np.where(w > q // 2, w - q, w).astype(I64)
    return out


def phase(mods, n, s, ct):
    """ct [k][2][batch][n] evals, s signed [n] -> the phase c0 + c1 s as batch x n Python integers centred in Q"""
    se = E.secret_evals(mods, n, s)
    return coeffs_centred(mods, n, np.stack([E.padd(q, ct[i, 0], E.pmul(q, ct[i, 1], se[i])) for i, q in enumerate(mods)]))


def decrypt_phase(mods, t, v):
    Q = prod(mods)
    return np.array([[scale_round(x, t, Q) % t for x in row] for row in v], dtype=U64)


def decrypt(mods, n, t, s, ct):
    return decrypt_phase(mods, t, phase(mods, n, s, ct))


def noise_budget(mods, t, v):
    Q = prod(mods)
    worst = max(abs(t * x - Q * scale_round(x, t, Q)) for row in v for x in row)
    if worst == 0:
        return Q.bit_length() - 1
    return max((Q // (2 * worst)).bit_length() - 1, 0) - 1


# ---- the route of the device, restated (Garner's digits; steps 3 and 4) ---------------------------------------------------------------
def garner_digits(src, res):
    """the mixed-radix digits a_0 .. a_{s-1} of the integer in [0, M) with residues res: x = a_0 + a_1 m_0 + a_2 m_0 m_1 + ..."""
    a = []
    for i, m in enumerate(src):
        v = int(res[i])
        for j in range(i):
            v = (v - a[j]) * pow(src[j], -1, m) % m
        a.append(v)
    return a


def half_digits(src):
    h, out = prod(src) // 2, []
    for m in src:
        out.append(h % m)
        h //= m
    return out


def garner_extend(src, dst, res, centred):
    """one element: residues res modulo src -> residues modulo dst, by the digits, the comparison from the top against the
    digits of floor(M / 2), and the sum of digit times prefix product per target"""
    a, h = garner_digits(src, res), half_digits(src)
    neg = False
    for i in reversed(range(len(src))):
        if a[i] != h[i]:
            neg = a[i] > h[i]
            break
    out = []
    for p in dst:
        w, acc = 1, 0
        for j, m in enumerate(src):
            acc += a[j] * w
            w = w * m % p
        out.append((acc - (w if centred and neg else 0)) % p)
    return out


def route_scale_round(mods, aux, t, d):
    """steps 3 and 4 on one integer d given by its residues modulo Q u B -> floor((t d + floor(Q / 2)) / Q) mod q_i"""
    Q = prod(mods)
    uq = [(t * (d % q) + Q // 2) % q for q in mods]
    ub = [(t * (d % b) + Q // 2) % b for b in aux]
    r = garner_extend(mods, aux, uq, False)
    y = [(ub[j] - r[j]) * pow(Q, -1, b) % b for j, b in enumerate(aux)]
    return garner_extend(aux, mods, y, True)


def route_decrypt(mods, b0, t, v):
    """the decryption route on one phase v given by its residues modulo Q: v extended centred to b_0, step 3 with b_0 alone"""
    Q = prod(mods)
    vq = [v % q for q in mods]
    vb = garner_extend(mods, [b0], vq, True)[0]
    uq = [(t * x + Q // 2) % q for x, q in zip(vq, mods)]
    r = garner_extend(mods, [b0], uq, False)[0]
    y = ((t * vb + Q // 2) - r) * pow(Q, -1, b0) % b0
    return centre(y, b0) % t


# ---- the batch encoder ---------------------------------------------------------------------------------------------------------------
def brv(x, L):
    return int(format(x, f"0{L}b")[::-1], 2) if L else 0


def slot_index(n):
    """[2][n/2]: slot (r, c) is the engine's index brv(((+-5^c mod 2n) - 1) / 2)"""
    L = n.bit_length() - 1
    idx = np.empty((2, n // 2), dtype=I64)
    for c in range(n // 2):
        e = pow(5, c, 2 * n)
        idx[0, c], idx[1, c] = brv((e - 1) // 2, L), brv((2 * n - e - 1) // 2, L)
    return idx


def encode(n, t, slots):
    """slots [2][n/2] modulo t -> coefficients [n]"""
    ev = np.zeros(n, dtype=U64)
    ev[slot_index(n).reshape(-1)] = np.mod(np.asarray(slots, dtype=I64), t).astype(U64).reshape(-1)
    return E.inv(t, n, ev[None])[0]


def decode(n, t, m):
    return E.fwd(t, n, np.asarray(m, dtype=U64)[None])[0][slot_index(n).reshape(-1)].reshape(2, n // 2)


def galois_coeffs(n, t, m, g):
    """m(X) -> m(X^g) modulo X^n + 1 and t"""
    out = np.zeros(n, dtype=object)
    for j, x in enumerate(m):
        e = j * g % (2 * n)
        out[e % n] = (out[e % n] + (int(x) if e < n else -int(x))) % t
    return out.astype(U64)


def chunk_rows(n, k, batch):
    return min(batch, max(1, (CHUNK_WORDS // n) // (7 * (2 * k + 1))))


def decrypt_chunk_rows(n, k, batch):
    """ciphertexts of a chunk of the decryption: k slabs of phase a ciphertext, 2^21 / (k n), at least one"""
    return min(batch, max(1, (CHUNK_WORDS // n) // k))
