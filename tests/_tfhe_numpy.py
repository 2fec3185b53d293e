"""numpy restatement of TFHE bootstrapping as DESIGN.md §10 defines it (steps 1-6), and host key generation for
the tests.  Words are u64 and wrap mod 2^64.  The external product is supplied by the caller (the C oracle's
schoolbook, or the library's prepared product), so that everything else here is checked against it."""
import numpy as np

U64 = np.uint64


def u64(x):
    return np.asarray(x).astype(np.uint64)


# 1. mod switch to 2N, rounding: round(w 2N / 2^64) mod 2N
def mod_switch(w, n):
    L = int(n).bit_length() - 1
    w = u64(w)
    return (((w >> U64(62 - L)) + U64(1)) >> U64(1)) & U64(2 * n - 1)


def mod_switch_exact(w, n):
    """the same with Python integers: round half up"""
    return ((int(w) * 2 * n + (1 << 63)) >> 64) % (2 * n)


# 2. rot(x, e) = X^-e x in T64[X]/(X^N+1), e in [0, 2N)
def rot(x, e):
    x = u64(x)
    n = x.shape[-1]
    j = np.arange(n) + int(e)
    v = x[..., j % n]
    return np.where((j // n) % 2 == 1, U64(0) - v, v).astype(np.uint64)


def left_rotate(x, h):
    """Tn::left_rotate (ring_torus.rs:118-132): c[h..n], then -c[0..h]"""
    x = u64(x)
    n = x.shape[-1]
    h = h % n
    return np.concatenate([x[..., h:], (U64(0) - x[..., :h])], axis=-1).astype(np.uint64)


# 3. blind rotation.  bsk: [n_lwe][(k+1)][l][(k+1)][n]; table [(k+1)][n]; lwe [batch][n_lwe+1]
def blind_rotation(ext, n, k, l, bsk, table, lwe):
    """ext(j, tglwe [batch][(k+1)][n]) -> BSK_j x tglwe"""
    lwe = u64(lwe)
    n_lwe = lwe.shape[1] - 1
    ms = mod_switch(lwe, n).astype(np.int64)
    acc = np.stack([rot(table, ms[b, n_lwe]) for b in range(lwe.shape[0])])
    for j in range(n_lwe):
        d = np.stack([rot(acc[b], (2 * n - ms[b, j]) % (2 * n)) for b in range(lwe.shape[0])]) - acc
        acc = acc + ext(j, d)
    return acc


# 4. sample extraction (tglwe.rs:89-115): [batch][(k+1)][n] -> [batch][k n + 1]
def sample_extraction(tglwe, h):
    tglwe = u64(tglwe)
    batch, k1, n = tglwe.shape
    j = np.arange(n)
    out = np.empty((batch, (k1 - 1) * n + 1), dtype=np.uint64)
    for c in range(k1 - 1):
        a = tglwe[:, c, :]
        lo = a[:, (h - j) % n]
        out[:, c * n:(c + 1) * n] = np.where(j <= h, lo, U64(0) - lo)
    out[:, -1] = tglwe[:, k1 - 1, h]
    return out


# 5. LWE key switch (tlwe.rs:101-111), beta = 2: ksk [n_in][l][n_out+1]
def key_switch(ksk, lwe, l):
    ksk, lwe = u64(ksk), u64(lwe)
    n_in = lwe.shape[1] - 1
    out = np.zeros((lwe.shape[0], ksk.shape[2]), dtype=np.uint64)
    out[:, -1] = lwe[:, n_in]
    for d in range(l):
        bits = (lwe[:, :n_in] >> U64(l - 1 - d)) & U64(1)
        out -= bits @ ksk[:, d, :]
    return out


# 6. bootstrapping: 3 -> 4 (h = 0) -> 5
def bootstrap(ext, n, k, l, bsk, table, ksk, ks_l, lwe):
    return key_switch(ksk, sample_extraction(blind_rotation(ext, n, k, l, bsk, table, lwe), 0), ks_l)


# ---- keys and messages (host-side scheme logic, as gfhe/src/glwe.rs:140-154 and tfhe/src/tlev.rs) -------------------
def gadget(l):
    """level d (0-based) of a TLev / TGLev scales the message by u64::MAX / 2^(d+1) (2^64 -> 1 at d = 63)"""
    return [((1 << 64) - 1) // (1 << (d + 1)) if d < 63 else 1 for d in range(l)]


def errors(rng, shape, sigma):
    if sigma == 0:
        return np.zeros(shape, dtype=np.uint64)
    return np.round(rng.normal(0.0, sigma, shape)).astype(np.int64).astype(np.uint64)


def tggsw_bits(rng, mul, n, l, s, bits, sigma):
    """k = 1: one TGGSW per bit m under the GLWE key s [n]: rows[(2)][l][(2)][n]; TGLev 0 encrypts -s m, TGLev 1 m
    (tggsw.rs:17-33).  mul(a [r][n], b [r][n]) -> the negacyclic products."""
    bits = np.asarray(bits)
    nb = len(bits)
    g = np.array(gadget(l), dtype=np.uint64)
    a = rng.integers(0, 1 << 64, (nb, 2, l, n), dtype=np.uint64, endpoint=False)
    a_s = mul(a.reshape(-1, n), np.broadcast_to(u64(s), (nb * 2 * l, n))).reshape(nb, 2, l, n)
    e = errors(rng, (nb, 2, l, n), sigma)
    mu = np.zeros((nb, 2, l, n), dtype=np.uint64)
    neg_s = U64(0) - u64(s)
    for i in range(nb):
        if bits[i]:
            mu[i, 0] = g[:, None] * neg_s[None, :]
            mu[i, 1, :, 0] = g
    rows = np.empty((nb, 2, l, 2, n), dtype=np.uint64)
    rows[:, :, :, 0, :] = a
    rows[:, :, :, 1, :] = a_s + mu + e
    return rows


def ksk(rng, s_in, s_out, l, sigma):
    """TLev of every input key bit under s_out: [n_in][l][n_out+1]"""
    s_in, s_out = u64(s_in), u64(s_out)
    n_in, n_out = len(s_in), len(s_out)
    g = np.array(gadget(l), dtype=np.uint64)
    a = rng.integers(0, 1 << 64, (n_in, l, n_out), dtype=np.uint64, endpoint=False)
    out = np.empty((n_in, l, n_out + 1), dtype=np.uint64)
    out[:, :, :n_out] = a
    out[:, :, n_out] = a @ s_out + s_in[:, None] * g[None, :] + errors(rng, (n_in, l), sigma)
    return out


def lwe_encrypt(rng, s, mu, sigma):
    s = u64(s)
    mu = u64(mu)
    a = rng.integers(0, 1 << 64, (len(mu), len(s)), dtype=np.uint64, endpoint=False)
    return np.concatenate([a, (a @ s + mu + errors(rng, len(mu), sigma))[:, None]], axis=1)


def lwe_decode(lwe, s, t):
    """TLWE::decrypt then TLWE::decode: round(t p / u64::MAX) in f64, mod t"""
    lwe, s = u64(lwe), u64(s)
    p = lwe[:, -1] - lwe[:, :-1] @ s
    return np.array([int(round(float(t) * float(int(x)) / float((1 << 64) - 1))) % t for x in p])


def test_vector(n, t, f):
    """trivial TGLWE (0, v), k = 1: coefficient i holds f(round(i / box)) Delta, box = 2N / t; the top half-box holds
    -f(0) Delta, where a phase just below 0 lands (X^-e v with e >= N is -v)"""
    delta = ((1 << 64) - 1) // t
    box = 2 * n // t
    v = np.empty(n, dtype=np.uint64)
    for i in range(n):
        m = (i + box // 2) // box
        v[i] = (f(m) * delta) % (1 << 64) if m < t // 2 else ((1 << 64) - f(0) * delta) % (1 << 64)
    return np.stack([np.zeros(n, dtype=np.uint64), v])
