"""A plain restatement of rows N3 / N4 of the reference (the gfhe surfaces over R_q and the element-wise glue) in
Python integers and floats, with no NTT: the reference of tests/test_rq_rows_gpu.py for n <= 256, and the check of
oracle.glue(...) (tests/test_rq_rows_cpu.py), which is the reference above that.

  Zq::decompose            arith/src/zq.rs:141-207      decompose
  Rq::decompose            arith/src/ring_nq.rs:67-78   rq_decompose          -> [l][n]
  Rq * Rq                  negacyclic schoolbook        rq_mul_schoolbook, rq_mul (the same sums, packed)
  TR . TR                  tuple_ring.rs:117-134        tr_dot
  TR x R, GLWE x R         tuple_ring.rs:137-155        tr_mul_r
  GLev x Vec<R>            gfhe/src/glev.rs:68-80       glev_mul
  GLWE::key_switch         gfhe/src/glwe.rs:126-137     key_switch
  f64 rows                 zq.rs:32-39,134-139, ring_nq.rs:82-113,282-306

Python's float(int) is the round-to-nearest-even conversion of Rust's `as f64`, and `*`, `/` on floats are the single
IEEE operations the Rust performs; `round` (half away from zero) and the saturating casts are written out here."""
import math

import numpy as np

U64 = 1 << 64
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- Zq::decompose ---------------------------------------------------------------------------------------------------

def decompose(q, v, beta, l):
    """Zq::decompose(beta, l) of the canonical word v -> l digits, most significant first"""
    if beta == 2:
        if v >= (1 << (l & 63)):                                   # zq.rs:176: `1 << l as u64`; --release wraps the amount at 64
            return [1 % q] * l
        return [((v >> i) & 1) % q for i in range(l - 1, -1, -1)]
    bl = (beta ** l) & 0xFFFFFFFF                                  # beta.pow(l) in u32 (the ABI rejects an overflow)
    if v >= bl:                                                    # zq.rs:152-160: every digit beta - 1
        return [beta - 1] * l
    out, rem = [], v
    for i in range(1, l + 1):
        den = q // (beta ** i)
        x = rem // den
        out.append(x % q)
        if x != 0:
            rem %= den
    return out


def rq_decompose(q, a, beta, l):
    """a: n words -> [l][n] (Rq::decompose: per coefficient, transposed)"""
    cols = [decompose(q, int(v), beta, l) for v in a]
    return [[cols[j][d] for j in range(len(cols))] for d in range(l)]


# ---- products -----------------------------------------------------------------------------------------------------------

def rq_mul_schoolbook(q, a, b):
    """a b mod (X^n + 1, q), term by term: the definition"""
    n = len(a)
    a, b = [int(x) for x in a], [int(x) for x in b]
    r = [0] * n
    for i in range(n):
        for j in range(n):
            if i + j < n:
                r[i + j] += a[i] * b[j]
            else:
                r[i + j - n] -= a[i] * b[j]
    return [x % q for x in r]


_SLOT = 24      # bytes per coefficient of a packed polynomial: a coefficient of the product is below n 2^128 < 2^192


def _pack(a):
    w = np.zeros((len(a), _SLOT // 8), dtype="<u8")
    w[:, 0] = np.asarray(a, dtype=np.uint64)
    return int.from_bytes(w.tobytes(), "little")


def rq_mul(q, a, b):
    """the same product with the 2n - 1 schoolbook sums formed by ONE multiplication of Python integers: A(2^192) B(2^192)
    holds sum_{i+j=m} a_i b_j in slot m, with no carry between slots (tests pin it against rq_mul_schoolbook)"""
    n = len(a)
    prod = (_pack(a) * _pack(b)).to_bytes(2 * n * _SLOT, "little")
    w = np.frombuffer(prod, dtype="<u8").reshape(2 * n, 3).astype(object)
    full = w[:, 0] + (w[:, 1] << 64) + (w[:, 2] << 128)
    return [int(x) % q for x in (full[:n] - full[n:])]


def _add(q, x, y):
    return [(s + t) % q for s, t in zip(x, y)]


def tr_dot(q, a, b):
    """a, b: [k][n] -> sum_i a[i] b[i]"""
    out = [0] * len(a[0])
    for x, y in zip(a, b):
        out = _add(q, out, rq_mul(q, x, y))
    return out


def tr_mul_r(q, a, p):
    """a: [rows][n], p: [n] -> [rows][n]"""
    return [rq_mul(q, x, p) for x in a]


def glev_mul(q, glev, v):
    """glev: [l][k+1][n], v: [l][n] -> [k+1][n]: out[c] = sum_d glev[d][c] v[d]"""
    k1, n = len(glev[0]), len(v[0])
    out = [[0] * n for _ in range(k1)]
    for d in range(len(v)):
        for c in range(k1):
            out[c] = _add(q, out[c], rq_mul(q, glev[d][c], v[d]))
    return out


def key_switch(q, k, beta, l, glwe, ksk):
    """glwe: [k+1][n] = (a_0 .. a_{k-1}, b); ksk: [k][l][k+1][n] -> (0, b) - sum_i ksk[i] x decompose(a_i)"""
    n = len(glwe[0])
    rhs = [[0] * n for _ in range(k + 1)]
    for i in range(k):
        part = glev_mul(q, ksk[i], rq_decompose(q, glwe[i], beta, l))
        rhs = [_add(q, r, p) for r, p in zip(rhs, part)]
    return [[((int(glwe[k][j]) if c == k else 0) - rhs[c][j]) % q for j in range(n)] for c in range(k + 1)]


# ---- f64 rows -------------------------------------------------------------------------------------------------------------

def rust_round(x):
    """f64::round: to the nearest integer, halves away from zero; NaN and infinities pass through"""
    if x != x or x in (math.inf, -math.inf):
        return x
    t = float(math.trunc(x))                                       # exact: |x| >= 2^52 is already an integer
    return t + math.copysign(1.0, x) if abs(x - t) >= 0.5 else t   # x - t is exact (same binade or smaller)


def as_i64(x):
    """Rust `f64 as i64`: NaN -> 0, saturating"""
    if x != x:
        return 0
    if x >= 9223372036854775808.0:
        return I64_MAX
    if x <= -9223372036854775808.0:
        return I64_MIN
    return int(x)


def as_u64(x):
    """Rust `f64 as u64`: NaN and negatives -> 0, saturating"""
    if x != x or x <= 0.0:
        return 0
    if x >= 18446744073709551616.0:
        return U64 - 1
    return int(x)


def zq_from_f64(q, e):
    """Zq::from_f64, zq.rs:32-39: ((e % q) + q) % q with Rust's truncated remainder is Python's e % q"""
    return as_i64(rust_round(e)) % q


def mod_switch(q, p, v):
    return as_u64(rust_round((float(v) * float(p)) / float(q))) % p


def mul_div_round(q, num, den, v):
    return zq_from_f64(q, rust_round((float(num) * float(v)) / float(den)))


def mul_by_f64(q, s, v):
    return zq_from_f64(q, float(v) * s)


def div_round(q, s, v):
    return zq_from_f64(q, rust_round(float(v) / float(s)))


def remodule(p, v):
    return v % p
