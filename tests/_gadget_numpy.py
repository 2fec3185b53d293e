"""numpy restatement of the signed base-2^b gadget of DESIGN.md §11: the decomposition, the gadget external product,
blind rotation, LWE key switch and bootstrap, and gadget key generation for the tests.  Words are u64 and wrap mod
2^64; digits are int64.  The rotation, mod switch and sample extraction are §10's (tests/_tfhe_numpy.py)."""
import numpy as np

import _tfhe_numpy as R

U64 = np.uint64


def gvalues(b, l):
    """g_d = 2^(64 - b(d+1)), level 0 the most significant"""
    return [1 << (64 - b * (d + 1)) for d in range(l)]


def decompose(w, b, l):
    """words [..] -> digits [.., l] (int64): round half up to the top b l bits, then balanced digits without a carry
    chain (y = x~ + B mod 2^(b l), digit_d = field d of y - 2^(b-1))"""
    assert 1 <= b and 1 <= l and b * l <= 64
    w = np.atleast_1d(R.u64(w))
    s = 64 - b * l
    xt = w if s == 0 else ((w >> U64(s - 1)) + U64(1)) >> U64(1)
    B = sum((1 << (b - 1)) << (b * i) for i in range(l))
    y = xt + U64(B % (1 << 64))
    if b * l < 64:
        y = y & U64((1 << (b * l)) - 1)
    mask = U64((1 << b) - 1) if b < 64 else U64((1 << 64) - 1)
    half = 1 << (b - 1)
    return np.stack([(((y >> U64(b * (l - 1 - d))) & mask) - U64(half)).view(np.int64) for d in range(l)], axis=-1)


def decompose_exact(w, b, l):
    """the same with Python integers: (x~, digits), x~ the rounded top b l bits"""
    s = 64 - b * l
    xt = w if s == 0 else ((w >> (s - 1)) + 1) >> 1
    xt %= 1 << (b * l)
    B = sum((1 << (b - 1)) << (b * i) for i in range(l))
    y = (xt + B) % (1 << (b * l))
    return xt, [((y >> (b * (l - 1 - d))) & ((1 << b) - 1)) - (1 << (b - 1)) for d in range(l)]


def negacyclic(x, rows):
    """rows [.., n] times the fixed x [n] in Z_{2^64}[X]/(X^n+1), all u64: a Toeplitz matmul in uint64 (wrapping)"""
    x = R.u64(x)
    n = x.shape[-1]
    d = np.arange(n)[:, None] - np.arange(n)[None, :]                   # out[i] = sum_j x[i - j] rows[j], negated on wrap
    m = np.where(d >= 0, x[d % n], U64(0) - x[d % n]).astype(np.uint64)
    return R.u64(rows) @ m.T


def external_product(key, ct, b):
    """key [(k+1)][l][(k+1)][n] (level d encrypts m g_d), ct [batch][(k+1)][n] -> [batch][(k+1)][n]:
    sum_i sum_d digit_d(ct_i) (x) key[i][d]"""
    key, ct = R.u64(key), R.u64(ct)
    k1, l, _, n = key.shape
    dig = decompose(ct, b, l)                                          # [batch][k1][n][l]
    out = np.zeros(ct.shape, dtype=np.uint64)
    for i in range(k1):
        for d in range(l):
            dv = dig[:, i, :, d].view(np.uint64)                       # [batch][n]
            for c in range(k1):
                out[:, c, :] += negacyclic(key[i, d, c], dv)
    return out


def external_product_rows(mul, key, ct, b):
    """the same product from digit rows against key rows: mul(x [r][n], y [r][n]) -> the r negacyclic products mod 2^64
    (the C oracle's schoolbook tn_mul), a digit entering as int64.view(uint64).  One product per (ciphertext, i, d, c);
    nothing here calls the library under test."""
    key, ct = R.u64(key), R.u64(ct)
    k1, l, _, n = key.shape
    batch = ct.shape[0]
    dig = np.moveaxis(decompose(ct, b, l), -1, -2).view(np.uint64)      # [batch][k1][l][n]
    x = np.broadcast_to(dig[:, :, :, None, :], (batch, k1, l, k1, n)).reshape(-1, n)
    y = np.broadcast_to(key[None], (batch, k1, l, k1, n)).reshape(-1, n)
    prod = R.u64(mul(np.ascontiguousarray(x), np.ascontiguousarray(y))).reshape(batch, k1 * l, k1, n)
    return prod.sum(axis=1, dtype=np.uint64)                            # wraps mod 2^64


def blind_rotation(n, k, b, l, bsk, table, lwe):
    bsk = R.u64(bsk)
    return R.blind_rotation(lambda j, d: external_product(bsk[j], d, b), n, k, l, bsk, table, lwe)


def key_switch(ksk, lwe, b, l):
    """ksk [n_in][l][n_out+1] (level d: TLev of s_in[i] g_d) -> (0 .. 0, b) - sum_i sum_d digit_d(a_i) ksk[i][d]"""
    ksk, lwe = R.u64(ksk), R.u64(lwe)
    n_in = lwe.shape[1] - 1
    dig = decompose(lwe[:, :n_in], b, l).view(np.uint64)                  # [batch][n_in][l]
    out = np.zeros((lwe.shape[0], ksk.shape[2]), dtype=np.uint64)
    out[:, -1] = lwe[:, n_in]
    for d in range(l):
        out -= dig[:, :, d] @ ksk[:, d, :]
    return out


def bootstrap(n, k, b, l, bsk, table, ks_b, ks_l, ksk, lwe):
    return key_switch(ksk, R.sample_extraction(blind_rotation(n, k, b, l, bsk, table, lwe), 0), ks_b, ks_l)


# ---- keys: as _tfhe_numpy's, with g_d = 2^(64 - b(d+1)) ----------------------------------------------------------------
def tggsw_bits(rng, mul, n, b, l, s, bits, sigma):
    """k = 1: one gadget TGGSW per bit m under the GLWE key s [n]: rows[(2)][l][(2)][n]; TGLev 0 encrypts -s m g_d,
    TGLev 1 m g_d.  mul(a [r][n], b [r][n]) -> the negacyclic products."""
    bits = np.asarray(bits)
    nb = len(bits)
    g = np.array([x % (1 << 64) for x in gvalues(b, l)], dtype=np.uint64)
    a = rng.integers(0, 1 << 64, (nb, 2, l, n), dtype=np.uint64, endpoint=False)
    a_s = mul(a.reshape(-1, n), np.broadcast_to(R.u64(s), (nb * 2 * l, n))).reshape(nb, 2, l, n)
    e = R.errors(rng, (nb, 2, l, n), sigma)
    mu = np.zeros((nb, 2, l, n), dtype=np.uint64)
    neg_s = U64(0) - R.u64(s)
    for i in range(nb):
        if bits[i]:
            mu[i, 0] = g[:, None] * neg_s[None, :]
            mu[i, 1, :, 0] = g
    rows = np.empty((nb, 2, l, 2, n), dtype=np.uint64)
    rows[:, :, :, 0, :] = a
    rows[:, :, :, 1, :] = a_s + mu + e
    return rows


def ksk(rng, s_in, s_out, b, l, sigma):
    """TLev of every input key bit under s_out with g_d = 2^(64 - b(d+1)): [n_in][l][n_out+1]"""
    s_in, s_out = R.u64(s_in), R.u64(s_out)
    n_in, n_out = len(s_in), len(s_out)
    g = np.array(gvalues(b, l), dtype=np.uint64)
    a = rng.integers(0, 1 << 64, (n_in, l, n_out), dtype=np.uint64, endpoint=False)
    out = np.empty((n_in, l, n_out + 1), dtype=np.uint64)
    out[:, :, :n_out] = a
    out[:, :, n_out] = a @ s_out + s_in[:, None] * g[None, :] + R.errors(rng, (n_in, l), sigma)
    return out
