"""numpy restatement of the client side of DESIGN.md §17: a vectorised ChaCha20 block function (RFC 8439), the stream layout
(rows, purposes, words), the table-inversion error sampler, LWE and TGLWE samples and their phases, and the messages that
the evaluation keys encrypt.  Words are u64 and wrap mod 2^64; nothing here calls the library under test."""
from fractions import Fraction

import numpy as np

import _gadget_numpy as G
import _tfhe_numpy as R

U32, U64 = np.uint32, np.uint64
MASK, ERR, KEY = 1, 2, 3
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)             # "expand 32-byte k"


def _rotl(x, r):
    return (x << U32(r)) | (x >> U32(32 - r))


def _qr(x, a, b, c, d):
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_blocks(key, counter, nonce):
    """key: 32 bytes; counter [m] and nonce [m][3] u32 words -> [m][16] u32 output words of the m blocks (RFC 8439 §2.3)"""
    k = np.frombuffer(bytes(key), dtype="<u4")
    assert len(k) == 8
    counter = np.atleast_1d(np.asarray(counter, dtype=np.uint64)).astype(U32)
    nonce = np.asarray(nonce, dtype=np.uint64).astype(U32).reshape(len(counter), 3)
    m = len(counter)
    init = [np.full(m, v, dtype=U32) for v in SIGMA] + [np.full(m, v, dtype=U32) for v in k] + [counter] + [nonce[:, i].copy() for i in range(3)]
    x = [v.copy() for v in init]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
            _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
        return np.stack([a + b for a, b in zip(x, init)], axis=1)


def keystream(key, counter, nonce12, nbytes):
    """the RFC's serialised key stream from block `counter` on: what `openssl enc -chacha20` XORs in"""
    blocks = (nbytes + 63) // 64
    n = np.frombuffer(bytes(nonce12), dtype="<u4")
    out = chacha20_blocks(key, counter + np.arange(blocks), np.tile(n, (blocks, 1)))
    return out.astype("<u4").tobytes()[:nbytes]


def stream_words(seed, purpose, first_row, row_words, rows):
    """[rows][row_words] u64: stream word i of row first_row + r is word i mod 8 of block i div 8 (counter = block, nonce =
    (purpose, row lo, row hi)); word j of a block = u32 word 2j | u32 word 2j + 1 << 32"""
    blocks = (row_words + 7) // 8
    assert blocks <= 1 << 32
    ridx = [(first_row + r) % (1 << 64) for r in range(rows)]
    nonce = np.array([[purpose, x & 0xFFFFFFFF, x >> 32] for x in ridx for _ in range(blocks)], dtype=np.uint64)
    out = chacha20_blocks(seed, np.tile(np.arange(blocks), rows), nonce).astype(U64)
    words = out[:, 0::2] | (out[:, 1::2] << U64(32))                       # [rows blocks][8]
    return words.reshape(rows, blocks * 8)[:, :row_words]


def key_bits(seed, row, n):
    return stream_words(seed, KEY, row, n, 1)[0] & U64(1)


def cdt_table(sigma):
    """strictly increasing thresholds below 2^63: entry i = round(2^63 P(magnitude <= i)), P(0) ~ rho(0), P(j) ~ 2 rho(j),
    j <= ceil(12 sigma); the tail that no longer differs at 2^-63 is cut"""
    import decimal

    if sigma == 0:
        return np.zeros(0, dtype=np.uint64)
    top = int(np.ceil(12 * sigma))
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        rho = [Fraction((-(decimal.Decimal(j) ** 2) / (2 * decimal.Decimal(float(sigma)) ** 2)).exp()) for j in range(top + 1)]
    wts = [rho[0]] + [2 * r for r in rho[1:]]
    total, run, out = sum(wts), Fraction(0), []
    for wgt in wts[:-1]:
        run += wgt
        thr = round(run / total * (1 << 63))
        if thr >= 1 << 63 or (out and thr <= out[-1]):
            break
        out.append(thr)
    return np.array(out, dtype=np.uint64)


def cdt_moments(cdt):
    """(mean, variance) of the signed error, in exact rationals, from what the sampler below returns: the stream words u with
    u >> 1 in [cdt[j-1], cdt[j]) (cdt[-1] = 0, cdt[m] = 2^63) and sign bit s are (cdt[j] - cdt[j-1]) of the 2^64 words; the
    value of each such class is errors() of its first and of its last word, which must agree"""
    t = [0] + [int(x) for x in cdt] + [1 << 63]
    mean = var = Fraction(0)
    for j in range(len(t) - 1):
        for sign in (0, 1):
            lo, hi = errors(cdt, np.array([(t[j] << 1) | sign, ((t[j + 1] - 1) << 1) | sign], dtype=U64), 0).view(np.int64)
            assert lo == hi
            p = Fraction(t[j + 1] - t[j], 1 << 64)
            mean += p * int(lo)
            var += p * int(lo) ** 2
    return mean, var - mean ** 2


def errors(cdt, u, log_scale):
    """stream words u -> error words: magnitude #{i : cdt[i] <= u >> 1}, negative when u & 1, << log_scale (wrapping)"""
    u = R.u64(u)
    if len(cdt) == 0:
        return np.zeros(u.shape, dtype=np.uint64)
    mag = np.searchsorted(R.u64(cdt), u >> U64(1), side="right").astype(U64)
    return (np.where(u & U64(1), U64(0) - mag, mag).astype(U64) << U64(log_scale)).astype(U64)


def lwe_encrypt(seed, first_row, s, mu, cdt, log_scale):
    """-> ([batch][n + 1], the error words [batch]): row r = [mask words of row first_row + r, <a, s> + mu_r + e_r]"""
    s, mu = R.u64(s) & U64(1), R.u64(mu)
    a = stream_words(seed, MASK, first_row, len(s), len(mu))
    e = errors(cdt, stream_words(seed, ERR, first_row, 1, len(mu))[:, 0], log_scale)
    return np.concatenate([a, (a @ s + mu + e)[:, None]], axis=1), e


def tglwe_encrypt(seed, first_row, S, msg, rows, cdt, log_scale):
    """msg None, [N] (broadcast) or [rows][N] -> ([rows][2][N], the error words [rows][N])"""
    S = R.u64(S) & U64(1)
    n = len(S)
    a = stream_words(seed, MASK, first_row, n, rows)
    e = errors(cdt, stream_words(seed, ERR, first_row, n, rows), log_scale)
    m = np.zeros((rows, n), dtype=U64) if msg is None else np.broadcast_to(R.u64(msg), (rows, n))
    return np.stack([a, G.negacyclic(S, a) + m + e], axis=1), e


def lwe_phase(c, s):
    c = R.u64(c)
    return c[..., -1] - c[..., :-1] @ (R.u64(s) & U64(1))


def tglwe_phase(c, S):
    c = R.u64(c)
    return c[..., 1, :] - G.negacyclic(R.u64(S) & U64(1), c[..., 0, :])


# ---- what the evaluation keys encrypt, one message per sample in the key's layout ------------------
def gwords(b, l):
    return np.array([x % (1 << 64) for x in G.gvalues(b, l)], dtype=np.uint64)


def bsk_messages(s_glwe, s_lwe, b, l):
    """[n_lwe][2][l][N]: TGLev 0 of bit i holds -S bit_i g_d, TGLev 1 the constant bit_i g_d"""
    S, bits, g = R.u64(s_glwe), R.u64(s_lwe), gwords(b, l)
    mu = np.zeros((len(bits), 2, l, len(S)), dtype=U64)
    bg = bits[:, None] * g[None, :]
    mu[:, 0] = U64(0) - bg[:, :, None] * S[None, None, :]
    mu[:, 1, :, 0] = bg
    return mu


def ksk_messages(s_in, b, l):
    """[n_in][l]: s_in[i] g_d"""
    return R.u64(s_in)[:, None] * gwords(b, l)[None, :]


def pfksk_messages(s_glwe, b, l):
    """[2][N + 1][l][N]: K~ = (-S, 1); function 0 holds -S K~_j g_d, function 1 the constant K~_j g_d"""
    S, g = R.u64(s_glwe), gwords(b, l)
    kt = np.concatenate([U64(0) - S, np.array([1], dtype=U64)])
    sc = kt[:, None] * g[None, :]
    mu = np.zeros((2, len(S) + 1, l, len(S)), dtype=U64)
    mu[0] = (U64(0) - sc)[:, :, None] * S[None, None, :]
    mu[1, :, :, 0] = sc
    return mu


def pksk_messages(s_in, n, b, l):
    """[n_in][l][N]: the constant polynomial s_in[j] g_d"""
    mu = np.zeros((len(s_in), l, n), dtype=U64)
    mu[:, :, 0] = ksk_messages(s_in, b, l)
    return mu
