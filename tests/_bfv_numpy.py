"""A plain restatement of row N1 of the reference (the BFV product either side of the NTT path) in Python integers and
floats, with no NTT: the reference of tests/test_bfv_shapes_gpu.py for n <= 64 (where it is fast enough), and the
check of oracle.bfv_tensor / bfv_relinearize / bfv_mul (tests/test_bfv_shapes_cpu.py), which are the reference above that.

  R * R                    arith/src/ring_n.rs:307-320    naive_mul             -> 2n - 1 words of i64
  mul_div_round            arith/src/ring_n.rs:130-138    mul_div_round_fold    -> n words of Z_q
    Rq::from_vec_f64         ring_nq.rs:160-163             (Zq::from_f64 per term, zq.rs:32-39)
    the X^n + 1 fold         ring_nq.rs:132-141             (Zq::sub, zq.rs:259-276)
  RLWE::tensor             bfv/src/lib.rs:59-85           tensor                -> (c0, c1, c2)
  relinearize_204          bfv/src/lib.rs:251-271         relinearize           -> (o0, o1)
  RLWE::mul                bfv/src/lib.rs:87-90           mul

Words are read `as i64` (Rq::to_r, ring_n.rs:72-79); the sums of naive_mul are exact (i128 in the reference) and each
is then truncated `as i64`, which the 61-bit case depends on.  The f64 steps are those of tests/_rq_rows_numpy.py, each
one IEEE operation as in the Rust."""
from _rq_rows_numpy import U64, mul_div_round

M64 = U64 - 1


def to_i64(x):
    """the low 64 bits of x, reinterpreted signed"""
    x = int(x) & M64
    return x - U64 if x >> 63 else x


def naive_mul_exact(n, a, b):
    """the 2n - 1 sums over Z of the words of a and b read as i64"""
    a, b = [to_i64(x) for x in a], [to_i64(x) for x in b]
    assert len(a) == n == len(b)
    res = [0] * (2 * n - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                res[i + j] += x * y
    return res


def naive_mul(n, a, b):
    """naive_mul: each exact sum truncated `as i64`"""
    return [to_i64(x) for x in naive_mul_exact(n, a, b)]


def mul_div_round_fold(q, n, v, num, den):
    """v: up to 2n - 1 words of i64 -> n words: z[i] = Zq::from_f64(round(num v[i] / den)), then z[i - n] -= z[i]"""
    z = [mul_div_round(q, num, den, to_i64(x)) for x in v]
    out = (z[:n] + [0] * n)[:n]
    for i in range(n, len(z)):
        out[i - n] = (out[i - n] - z[i]) % q
    return out


def tensor(q, n, t, a0, a1, b0, b1):
    """c0 = a0 b0, c1 = a0 b1 + a1 b0 (the two products added as wrapping i64 BEFORE the scaling), c2 = a1 b1; each t / q"""
    c0 = mul_div_round_fold(q, n, naive_mul(n, a0, b0), t, q)
    l, r = naive_mul(n, a0, b1), naive_mul(n, a1, b0)
    c1 = mul_div_round_fold(q, n, [to_i64(x + y) for x, y in zip(l, r)], t, q)
    c2 = mul_div_round_fold(q, n, naive_mul(n, a1, b1), t, q)
    return c0, c1, c2


def relinearize(q, n, pq, rlk0, rlk1, c0, c1, c2):
    """(c0 + round(c2 rlk0 / p), c1 + round(c2 rlk1 / p)) with p = pq // q and Zq::add"""
    p = pq // q
    r0 = mul_div_round_fold(q, n, naive_mul(n, c2, rlk0), 1, p)
    r1 = mul_div_round_fold(q, n, naive_mul(n, c2, rlk1), 1, p)
    return [(int(x) + y) % q for x, y in zip(c0, r0)], [(int(x) + y) % q for x, y in zip(c1, r1)]


def mul(q, n, t, pq, rlk0, rlk1, a0, a1, b0, b1):
    return relinearize(q, n, pq, rlk0, rlk1, *tensor(q, n, t, a0, a1, b0, b1))
