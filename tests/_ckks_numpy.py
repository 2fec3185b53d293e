"""Restatement of CKKS as DESIGN.md §21 defines it, on tests/_client_numpy.py's ChaCha20 and tests/_bfv_client_numpy.py's
samplers and exact products: the four CKKS purposes of the stream, the canonical embedding of ckks/src/encoder.rs (a dense
`longdouble` Vandermonde product for N <= 512, `numpy.fft` on the twisted vector above that), the error bounds E_dec and
E_enc, and the scheme of ckks/src/lib.rs:46-118 with exact modular arithmetic.  Nothing here calls the library under test.

    embedding  w = exp(i pi / N); slot i < N/2 is the polynomial at w^(2i+1); slots N-1-i are the conjugates
    decode     z_i = (1/Delta) sum_j p_j w^((2i+1) j)
    encode     a_j = (1/N) Re(w^-j sum_i h_i w^(-2ij)), h the Hermitian extension of Delta z; coefficient = round half away
"""
import numpy as np

import _bfv_client_numpy as BC
import _client_numpy as C

CKKS_MASK, CKKS_ERR, CKKS_KEY, CKKS_EPH = 0x21, 0x22, 0x23, 0x24
U64, I64, LD = np.uint64, np.int64, np.longdouble
U = 2.0 ** -53                                                         # the unit roundoff of f64
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)              # pi to the 64 bits of an x87 long double


# ---- the embedding ------------------------------------------------------------------------------------------------------------
def root_powers_ld(n, count=None):
    """w^k = exp(i pi k / n), k < count (default 2n), as (cos, sin) longdouble arrays; the argument handed to cos / sin is
    reduced to [0, pi/4] in integers, so every entry is good to the last bits of a long double"""
    count = 2 * n if count is None else count
    c, s = np.empty(count, dtype=LD), np.empty(count, dtype=LD)
    for k in range(count):
        m = k % (2 * n)
        neg_s = m >= n                                                  # w^(k + n) = -w^k
        m -= n if neg_s else 0
        neg_c = neg_s
        if 2 * m > n:                                                   # cos(pi - x) = -cos x
            m, neg_c = n - m, not neg_c
        if 4 * m <= n:
            a = PI_LD * LD(m) / LD(n)
            cc, ss = np.cos(a), np.sin(a)
        else:
            a = PI_LD * LD(n - 2 * m) / LD(2 * n)
            cc, ss = np.sin(a), np.cos(a)
        c[k], s[k] = (-cc if neg_c else cc), (-ss if neg_s else ss)
    return c, s


def _vandermonde_ld(n):
    """(cos, sin) of w^((2i+1) j), i < n/2 rows, j < n columns"""
    c, s = root_powers_ld(n)
    e = (np.outer(2 * np.arange(n // 2) + 1, np.arange(n))) % (2 * n)
    return c[e], s[e]


def decode_dense_ld(p, delta):
    """-> (re, im) longdouble [rows][n/2]: the definition, term by term in longdouble"""
    p = np.atleast_2d(np.asarray(p))
    vc, vs = _vandermonde_ld(p.shape[-1])
    pl = p.astype(np.float64).astype(LD)                                # signed words taken to f64 first, as the reference does
    return (pl @ vc.T) / LD(delta), (pl @ vs.T) / LD(delta)


def decode(p, delta):
    """[rows][n] signed words -> complex128 [rows][n/2]; dense longdouble for n <= 512, numpy.fft on the twisted vector above"""
    p = np.atleast_2d(np.asarray(p))
    n = p.shape[-1]
    if n <= 512:
        re, im = decode_dense_ld(p, delta)
        return re.astype(np.float64) + 1j * im.astype(np.float64)
    return decode_fft(p, delta)


def decode_fft(p, delta):
    """z_i = sum_j (p_j w^j) exp(2 pi i ij / n) = n ifft(p w^j)[i], i < n/2"""
    p = np.atleast_2d(np.asarray(p))
    n = p.shape[-1]
    c, s = root_powers_ld(n, n)
    tw = c.astype(np.float64) + 1j * s.astype(np.float64)
    return (np.fft.ifft(p.astype(np.float64) * tw, axis=-1) * n)[:, :n // 2] / delta


def hermitian(z, delta):
    """h = Delta pi^-1(z): [rows][n/2] -> [rows][n] with h[n-1-i] = conj(h[i])"""
    z = np.atleast_2d(np.asarray(z, dtype=np.complex128))
    h = delta * z
    return np.concatenate([h, np.conj(h[:, ::-1])], axis=1)


def encode_pre_dense_ld(z, delta):
    """the exact a_j (before rounding) as longdouble [rows][n]: (1/n) sum_i Re(h_i conj(w^((2i+1) j))) over all n slots =
    (2/n) sum_{i < n/2} (Re h_i cos - ... ) by the Hermitian symmetry"""
    z = np.atleast_2d(np.asarray(z, dtype=np.complex128))
    n = 2 * z.shape[-1]
    vc, vs = _vandermonde_ld(n)
    hr, hi = (delta * z.real).astype(LD), (delta * z.imag).astype(LD)   # h = Delta z rounded to f64, as the reference forms it
    return (hr @ vc + hi @ vs) * LD(2) / LD(n)


def encode_pre(z, delta):
    """the pre-rounding a_j as float64 [rows][n]: dense longdouble for n <= 512, numpy.fft above:
    a_j = Re(w^-j fft(h)[j]) / n"""
    z = np.atleast_2d(np.asarray(z, dtype=np.complex128))
    n = 2 * z.shape[-1]
    if n <= 512:
        return encode_pre_dense_ld(z, delta).astype(np.float64)
    c, s = root_powers_ld(n, n)
    tw = c.astype(np.float64) - 1j * s.astype(np.float64)
    return (np.fft.fft(hermitian(z, delta), axis=-1) * tw).real / n


def round_away(a):
    """round half away from zero -> int64 (Rust's f64::round, then `as i64`)"""
    a = np.asarray(a, dtype=np.float64)
    return (np.sign(a) * np.floor(np.abs(a) + 0.5)).astype(I64)


def encode(z, delta):
    return round_away(encode_pre(z, delta))


def e_dec(p, delta):
    """E_dec = 16 u log2(2N) sqrt(N) ||p||_2 / Delta per row"""
    p = np.atleast_2d(np.asarray(p)).astype(np.float64)
    n = p.shape[-1]
    return 16 * U * np.log2(2 * n) * np.sqrt(n) * np.linalg.norm(p, axis=-1) / delta


def e_enc(z, delta):
    """E_enc = 16 u log2(2N) ||h||_2 / sqrt(N) per row"""
    h = hermitian(z, delta)
    n = h.shape[-1]
    return 16 * U * np.log2(2 * n) * np.linalg.norm(h, axis=-1) / np.sqrt(n)


# ---- samples ------------------------------------------------------------------------------------------------------------------
def ternary(seed, purpose, first_row, n, rows):
    """[rows][n] int64 in {-1, 0, 1}: (w AND 1) - ((w >> 1) AND 1) of the rows' stream words"""
    return BC.ephemeral_of_words(C.stream_words(seed, purpose, first_row, n, rows))


def secret_key(seed, key_row, n):
    return ternary(seed, CKKS_KEY, key_row, n, 1)[0]


def uniform_row(seed, row, n, q):
    w = C.stream_words(seed, CKKS_MASK, row, 2 * n, 1)[0]
    return np.array([BC.uniform_word(w[2 * i], w[2 * i + 1], q) for i in range(n)], dtype=U64)


def errors(seed, first_err_row, n, rows, cdt):
    return C.errors(cdt, C.stream_words(seed, CKKS_ERR, first_err_row, n, rows), 0).view(I64)


# ---- the scheme (ckks/src/lib.rs:46-118), exact ------------------------------------------------------------------------------------
def msg_mod(m, q):
    """signed words -> residues"""
    return np.mod(np.asarray(m, dtype=I64), I64(q)).astype(U64)


def public_key(seed, row, s, q, cdt):
    """(pk0, pk1) = (-a s + e, a): a the uniform MASK row `row`, e from ERR row 2 row; s ternary int64"""
    n = len(s)
    a = uniform_row(seed, row, n, q)
    e = BC._residues(errors(seed, 2 * row, n, 1, cdt)[0], q)
    a_s = BC.negacyclic(a, np.asarray(s, dtype=I64), q)
    return BC._add((U64(q) - a_s) % U64(q), e, q), a


def encrypt(seed, first_row, pk0, pk1, msg, rows, q, cdt):
    """-> (c0, c1) each [rows][n]; msg None, [n] or [rows][n] signed words"""
    n = len(pk0)
    v = ternary(seed, CKKS_EPH, first_row, n, rows)
    e = errors(seed, 2 * first_row, n, 2 * rows, cdt).reshape(rows, 2, n)
    mm = np.zeros((rows, n), dtype=U64) if msg is None else np.broadcast_to(msg_mod(msg, q), (rows, n))
    c0 = BC._add(BC._add(BC.negacyclic(v, pk0, q), BC._residues(e[:, 0], q), q), mm, q)
    c1 = BC._add(BC.negacyclic(v, pk1, q), BC._residues(e[:, 1], q), q)
    return c0, c1


def centre(d, q):
    d = np.asarray(d, dtype=U64)
    return np.where(d > U64(q // 2), d.astype(I64) - I64(q), d.astype(I64))


def decrypt(s, c0, c1, q):
    """c0 + c1 s mod q, centred -> int64"""
    c1 = np.asarray(c1, dtype=U64)
    return centre(BC._add(c0, BC.negacyclic(c1, np.asarray(s, dtype=I64), q), q), q)


def add(ca, cb, q):
    return BC._add(ca[0], cb[0], q), BC._add(ca[1], cb[1], q)


def sub(ca, cb, q):
    """both components are subtracted (the reference adds the second one, lib.rs:117: not reproduced)"""
    neg = lambda x: (U64(q) - np.asarray(x, dtype=U64)) % U64(q)
    return BC._add(ca[0], neg(cb[0]), q), BC._add(ca[1], neg(cb[1]), q)


def mul_plain(c, m, q):
    """both components of one ciphertext [n] times the plaintext polynomial m (signed words), term by term"""
    mm = msg_mod(m, q)
    return BC.negacyclic_schoolbook(c[0], mm, q), BC.negacyclic_schoolbook(c[1], mm, q)


# ---- the case lists that tests/test_ckks_cpu.py proves and tests/test_ckks_gpu.py runs on the device --------------------------
_Q16, _Q61 = 65537, 2305843009211596801
PK_BASE = 1 << 56
SIZES = [2, 4, 8, 16, 32, 64, 128, 256, 512, 4096, 8192]


def _seed(k):
    return bytes((k * 29 + 13 * i + 7) % 256 for i in range(32))


# exact-construction cases (N, rng seed, B, log2 Delta): p uniform in (-2^B, 2^B), z = f64(sigma(p) / Delta) from the dense
# longdouble form; the encoder must give p back exactly
EXACT_CASES = [(n, 700 + i, 20, 10) for i, n in enumerate(SIZES)]
# random-z cases (N, rng seed, rows, log2 Delta): z uniform in the square |re|, |im| < 8; the restatement's rounding is the
# expected output because no pre-rounding value is near a half-integer (proved by the CPU module)
RANDOM_CASES = [(2, 811, 3, 10), (16, 812, 3, 10), (32, 813, 3, 10), (512, 814, 3, 10), (4096, 815, 3, 10), (8192, 816, 3, 10)]


def exact_case(n, seed, b):
    return np.random.default_rng(seed).integers(-(1 << b) + 1, 1 << b, (3, n), dtype=np.int64)


def exact_case_slots(p, delta):
    """dense longdouble for N <= 512, the FFT form above that (what is proved is that encode_pre of these slots is near p)"""
    return decode(p, delta)


def random_case(n, seed, rows):
    r = np.random.default_rng(seed)
    return r.uniform(-8, 8, (rows, n // 2)) + 1j * r.uniform(-8, 8, (rows, n // 2))


# functional cases: the reference's four tests (lib.rs:126-304) at its parameters, the same at the 61-bit modulus, and
# mul_plain; z has integer parts in [0, t) as the reference's C::rand(t)
FUNCTIONAL = {
    "encrypt_32": dict(seed=_seed(1), q=_Q16, n=32, t=50, delta=512.0, rows=8, rng=901),
    "encode_16": dict(seed=_seed(2), q=_Q16, n=16, t=8, delta=512.0, rows=8, rng=902),
    "add_16": dict(seed=_seed(3), q=_Q16, n=16, t=8, delta=1024.0, rows=8, rng=903),
    "sub_16": dict(seed=_seed(4), q=_Q16, n=16, t=2, delta=1024.0, rows=8, rng=904),
    "encode_4096_q61": dict(seed=_seed(5), q=_Q61, n=4096, t=8, delta=float(1 << 30), rows=2, rng=905),
    "add_4096_q61": dict(seed=_seed(6), q=_Q61, n=4096, t=8, delta=float(1 << 30), rows=2, rng=906),
    "sub_4096_q61": dict(seed=_seed(7), q=_Q61, n=4096, t=2, delta=float(1 << 30), rows=2, rng=907),
    "mul_plain_32_q61": dict(seed=_seed(8), q=_Q61, n=32, t=8, delta=float(1 << 20), rows=1, rng=908),
}


def case_slots(case, k):
    r = np.random.default_rng(case["rng"] + 10 * k)
    shape = (case["rows"], case["n"] // 2)
    return r.integers(0, case["t"], shape).astype(np.float64) + 1j * r.integers(0, case["t"], shape).astype(np.float64)


def case_raw_message(case):
    """test_encrypt_decrypt's m_raw: coefficients in [0, t)"""
    return np.random.default_rng(case["rng"]).integers(0, case["t"], (case["rows"], case["n"]), dtype=np.int64)
