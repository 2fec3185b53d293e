"""Restatement of the BFV client side of DESIGN.md §20 on top of tests/_client_numpy.py's ChaCha20: the four BFV purposes of
the stream, the uniform map, the secret key, the ephemeral u, the errors, and the scheme of bfv/src/lib.rs:118-225 (public
key, relinearisation key, encrypt, decrypt, add_const / mul_const) with exact modular arithmetic in Python integers.
Nothing here calls the library under test.

Every product of the scheme has one operand with coefficients in {-1, 0, 1} (s, u) or is s s, so `negacyclic` forms it
exactly with numpy: the large operand is cut into 21-bit limbs, a limb times a small operand sums to below n 2^21 <= 2^40, which
int64 (np.convolve, a few rows) and float64 (one matrix product against the negacyclic matrix of the shared operand, a batch)
both hold exactly; the limbs are recombined modulo Q by doubling.  tests/test_bfv_client_cpu.py pins both routes against the
term-by-term definition."""
import numpy as np

import _client_numpy as C
from _rq_rows_numpy import mul_div_round

BFV_MASK, BFV_ERR, BFV_KEY, BFV_EPH = 0x11, 0x12, 0x13, 0x14
U64, I64 = np.uint64, np.int64
LIMB = 21


# ---- samples ------------------------------------------------------------------------------------------------------------------
def uniform_word(w0, w1, Q):
    """floor((w1 2^64 + w0) Q / 2^128): the definition, in big integers"""
    return ((int(w1) << 64 | int(w0)) * int(Q)) >> 128


def uniform_word_device(w0, w1, Q):
    """the same as the kernels form it: ((u128) w1 Q + mulhi64(w0, Q)) >> 64"""
    return (int(w1) * int(Q) + ((int(w0) * int(Q)) >> 64)) >> 64


def uniform_row(seed, row, n, Q):
    """[n] u64: coefficient i from MASK words 2i and 2i + 1 of the row"""
    w = C.stream_words(seed, BFV_MASK, row, 2 * n, 1)[0]
    return np.array([uniform_word(w[2 * i], w[2 * i + 1], Q) for i in range(n)], dtype=U64)


def secret_key(seed, key_row, n):
    return C.stream_words(seed, BFV_KEY, key_row, n, 1)[0] & U64(1)


def ephemeral_of_words(w):
    """stream words -> u in {-1, 0, 1} (int64): (w & 1) - ((w >> 1) & 1)"""
    w = np.asarray(w, dtype=U64)
    return (w & U64(1)).astype(I64) - ((w >> U64(1)) & U64(1)).astype(I64)


def ephemeral(seed, first_row, n, rows):
    """[rows][n] int64 in {-1, 0, 1}: u of encryption rows first_row .."""
    return ephemeral_of_words(C.stream_words(seed, BFV_EPH, first_row, n, rows))


def errors(seed, first_err_row, n, rows, cdt):
    """[rows][n] int64: the signed errors of ERR rows first_err_row .. (cdt_error at log_scale 0)"""
    return C.errors(cdt, C.stream_words(seed, BFV_ERR, first_err_row, n, rows), 0).view(I64)


# ---- the product ----------------------------------------------------------------------------------------------------------------
def negacyclic_schoolbook(a, b, Q):
    """a b mod (X^n + 1, Q) term by term in Python integers (a, b: signed or unsigned integers): the definition"""
    n = len(a)
    a, b = [int(x) for x in a], [int(x) for x in b]
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                k = i + j
                if k < n:
                    out[k] += x * y
                else:
                    out[k - n] -= x * y
    return np.array([v % Q for v in out], dtype=U64)


def _limbs(x):
    """non-negative words below 2^63 -> their 21-bit limbs (int64), least significant first; small signed values -> [x]"""
    x = np.asarray(x)
    if x.dtype != U64:
        assert np.abs(x).max(initial=0) <= 1
        return [x.astype(I64)]
    top = int(x.max(initial=0))
    assert top < 1 << 63
    return [((x >> U64(LIMB * k)) & U64((1 << LIMB) - 1)).astype(I64) for k in range(max(1, -(-top.bit_length() // LIMB)))]


def _negmat(v):
    """M with (M x)_i = sum_j v[(i - j) mod n] x_j sign(i >= j): the negacyclic product by v as a float64 matrix"""
    n = len(v)
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    return np.where(i >= j, 1.0, -1.0) * np.asarray(v, dtype=np.float64)[(i - j) % n]


def _mod_words(x, Q):
    """int64 values -> their residues modulo Q < 2^63 as u64"""
    assert 0 < Q < 1 << 63
    return np.mod(x, I64(Q)).astype(U64)


def negacyclic(batch, shared, Q):
    """batch [rows][n] (or [n]) times shared [n] modulo (X^n + 1, Q) -> u64 [rows][n].  Operands are u64 words below 2^63, or
    integer arrays of another dtype with values in {-1, 0, 1}; at most one of the two is of the first kind."""
    batch = np.asarray(batch)
    one = batch.ndim == 1
    batch = batch.reshape(-1, batch.shape[-1])
    rows, n = batch.shape
    lb, ls = _limbs(batch), _limbs(shared)
    assert batch.dtype != U64 or np.asarray(shared).dtype != U64, "one operand must be small"
    assert n << LIMB < 1 << 53
    parts = []                                                       # the integer product, limb by limb
    for bl in lb:
        for sl in ls:
            if rows <= 2:
                full = np.stack([np.convolve(r, sl) for r in bl])
                p = full[:, :n].copy()
                p[:, :n - 1] -= full[:, n:]
            else:
                p = np.rint(bl.astype(np.float64) @ _negmat(sl).T).astype(I64)
            parts.append(p)
    Qw = U64(Q)
    acc = _mod_words(parts[-1], Q)
    for p in reversed(parts[:-1]):
        for _ in range(LIMB):
            acc = acc + acc
            acc = np.where(acc >= Qw, acc - Qw, acc)
        acc = acc + _mod_words(p, Q)
        acc = np.where(acc >= Qw, acc - Qw, acc)
    return acc[0] if one else acc


def _residues(x, Q):
    """signed int64 values (|x| < Q) -> residues in [0, Q)"""
    return _mod_words(np.asarray(x, dtype=I64), Q)


def _add(a, b, Q):
    r = np.asarray(a, dtype=U64) + np.asarray(b, dtype=U64)          # both below Q < 2^63: no wrap
    return np.where(r >= U64(Q), r - U64(Q), r)


def _signed(s):
    return (np.asarray(s, dtype=U64) & U64(1)).astype(I64)


# ---- the scheme (bfv/src/lib.rs:118-225) ------------------------------------------------------------------------------------------
def public_key(seed, row, s, q, cdt, mul=negacyclic):
    """-> (pk0, pk1) = (-a s + e, a) mod q: a = uniform MASK row `row`, e from ERR row 2 row"""
    n = len(s)
    a = uniform_row(seed, row, n, q)
    e = _residues(errors(seed, 2 * row, n, 1, cdt)[0], q)
    a_s = mul(a, _signed(s), q)
    return _add((U64(q) - a_s) % U64(q), e, q), a


def relin_key_from(a, s, e, q, pq, mul=negacyclic):
    """(-(a s + e) + p s^2, a) mod pq from its samples, exactly: a [n] below pq, s bits, e signed"""
    p = pq // q
    sb = _signed(s)
    a_s = mul(np.asarray(a, dtype=U64), sb, pq)
    ss = mul(sb, sb, q)                                       # p (s^2 mod q) = p s^2 mod pq, and it is below pq
    x = _add(a_s, _residues(e, pq), pq)
    return _add((U64(pq) - x) % U64(pq), U64(p) * ss, pq), np.asarray(a, dtype=U64)


def relin_key(seed, row, s, q, pq, cdt, mul=negacyclic):
    n = len(s)
    return relin_key_from(uniform_row(seed, row, n, pq), s, errors(seed, 2 * row, n, 1, cdt)[0], q, pq, mul)


def _delta_m(m, q, t):
    """Delta (m mod q) mod q per word, in Python integers"""
    return ((np.asarray(m, dtype=U64).astype(object) % q) * (q // t) % q).astype(U64)


def encrypt(seed, first_row, pk0, pk1, msg, rows, q, t, cdt, mul=negacyclic):
    """-> (c0, c1, noise samples (u, e1, e2)) each [rows][n]; msg None, [n] (one for every row) or [rows][n], any u64 words"""
    n = len(pk0)
    u = ephemeral(seed, first_row, n, rows)
    e = errors(seed, 2 * first_row, n, 2 * rows, cdt).reshape(rows, 2, n)
    e1, e2 = e[:, 0], e[:, 1]
    if msg is None:
        dm = np.zeros((rows, n), dtype=U64)
    else:
        dm = np.broadcast_to(_delta_m(msg, q, t), (rows, n))
    c0 = _add(_add(mul(u, pk0, q), _residues(e1, q), q), dm, q)
    c1 = _add(mul(u, pk1, q), _residues(e2, q), q)
    return c0, c1, (u, e1, e2)


def phase(s, c0, c1, q, mul=negacyclic):
    """c0 + c1 s mod q"""
    return _add(c0, mul(np.asarray(c1, dtype=U64), _signed(s), q), q)


def scale_round(cs, q, t):
    """Zq::from_f64(q, round(t cs / q)) reduced mod t, per word, with the reference's f64 steps"""
    flat = [mul_div_round(q, t, q, int(v)) % t for v in np.asarray(cs).reshape(-1)]
    return np.array(flat, dtype=U64).reshape(np.asarray(cs).shape)


def decrypt(s, c0, c1, q, t, mul=negacyclic):
    return scale_round(phase(s, c0, c1, q, mul), q, t)


def noise(s, c0, c1, m, q, t, mul=negacyclic):
    """the centred c0 + c1 s - Delta m as int64: what must stay inside q / (2 t) (minus the r_t(q) term) for decryption"""
    d = (phase(s, c0, c1, q, mul).astype(object) - (q // t) * (np.asarray(m, dtype=U64) % U64(t)).astype(object)) % q
    return np.array([int(v) - q if int(v) > q // 2 else int(v) for v in d.reshape(-1)], dtype=object).reshape(d.shape)


def add(ca, cb, q):
    return _add(ca[0], cb[0], q), _add(ca[1], cb[1], q)


def add_const(c, m, q, t):
    """lib.rs:180-188: (c0 + Delta m, c1)"""
    return _add(c[0], _delta_m(m, q, t), q), np.asarray(c[1], dtype=U64)


def const_ciphertext(m, q, t):
    """lib.rs:198: the noiseless (Delta m, 0) that mul_const multiplies by"""
    return _delta_m(m, q, t), np.zeros(len(m), dtype=U64)


# ---- the functional cases that tests/test_bfv_client_cpu.py proves and tests/test_bfv_client_gpu.py repeats on the device -------
# rows as bfv.ClientKey deals them: the secret is KEY row 0, public_key(0) is row PK_BASE, relin_key(0) row RLK_BASE,
# encryptions take rows 0, 1, .. in call order.  Message set k of a case: default_rng(case["rng"] + k).integers(0, t, (rows, n)).
PK_BASE, RLK_BASE = 1 << 56, 2 << 56
_Q16, _Q61 = 65537, 2305843009211596801


def _seed(k):
    return bytes((k * 37 + 11 * i + 5) % 256 for i in range(32))


CASES = {
    "encrypt_512": dict(seed=_seed(1), q=_Q16, n=512, t=32, p=0, rows=64, rng=101),
    "encrypt_4096_q61": dict(seed=_seed(2), q=_Q61, n=4096, t=32, p=0, rows=4, rng=102),
    "add_128": dict(seed=_seed(3), q=_Q16, n=128, t=32, p=0, rows=32, rng=103),
    "const_16_t8": dict(seed=_seed(4), q=_Q16, n=16, t=8, p=_Q16 * _Q16, rows=8, rng=104),
    "mul_16_t2": dict(seed=_seed(5), q=_Q16, n=16, t=2, p=_Q16 * _Q16, rows=8, rng=105),
}


def case_messages(case, k):
    return np.random.default_rng(case["rng"] + k).integers(0, case["t"], (case["rows"], case["n"]), dtype=np.uint64)
