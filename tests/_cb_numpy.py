"""numpy restatement of circuit bootstrapping as DESIGN.md §12 defines it: the private functional key switch (PFKS),
the circuit bootstrap, the CMux with a selector per ciphertext and vertical packing, and PFKSK generation for the
tests.  k = 1; words are u64 and wrap mod 2^64.  Built on tests/_gadget_numpy.py (§11) and tests/_tfhe_numpy.py (§10)."""
import numpy as np

import _gadget_numpy as G
import _tfhe_numpy as R

U64 = np.uint64


def private_key_switch(pfksk, c, b, l):
    """pfksk [(k+1)][kN+1][l][(k+1)][n], c [batch][kN+1] -> [batch][(k+1) functions][(k+1)][n]:
    out_r = sum_{j <= kN} sum_d digit_d(c_j) pfksk[r][j][d]"""
    pfksk, c = R.u64(pfksk), R.u64(c)
    k1, rows, n = pfksk.shape[0], pfksk.shape[1] * pfksk.shape[2], pfksk.shape[-1]
    dig = G.decompose(c, b, l).view(np.uint64).reshape(c.shape[0], rows)      # [batch][(kN+1) l], digit-major per word
    return np.stack([dig @ pfksk[r].reshape(rows, k1 * n) for r in range(k1)], axis=1).reshape(c.shape[0], k1, k1, n)


def alpha(cb_b, d):
    """alpha_d = g_d(b_cb) / 2"""
    return 1 << (63 - cb_b * (d + 1))


def circuit_bootstrap(n, b, l, bsk, cb_b, cb_l, pf_b, pf_l, pfksk, lwe):
    """lwe [batch][n_lwe+1] of mu 2^63 -> raw gadget TGGSWs [batch][(k+1)][cb_l][(k+1)][n]: for each level d, the gadget
    blind rotation of c + (0 .. 0, 2^62) with the trivial table of body alpha_d, sample extraction at 0, T_d = (0 .. 0,
    alpha_d) - E, row (r, d) = PFKS_r(T_d)"""
    lwe = R.u64(lwe).copy()
    lwe[:, -1] += U64(1 << 62)
    out = np.empty((lwe.shape[0], 2, cb_l, 2, n), dtype=np.uint64)
    for d in range(cb_l):
        out[:, :, d] = private_key_switch(pfksk, cb_rows_t(n, b, l, bsk, cb_b, d, lwe), pf_b, pf_l)
    return out


def cb_rows_t(n, b, l, bsk, cb_b, d, lwe_shifted):
    """T_d for every input (lwe already carries the + 2^62): [batch][kN+1]"""
    table = np.zeros((2, n), dtype=np.uint64)
    table[1, :] = U64(alpha(cb_b, d))
    e = R.sample_extraction(G.blind_rotation(n, 1, b, l, bsk, table, lwe_shifted), 0)
    t = (U64(0) - e).astype(np.uint64)
    t[:, -1] += U64(alpha(cb_b, d))
    return t


def cmux(keys, idx, c0, c1, b):
    """out_j = c0_j + keys[idx_j] [x] (c1_j - c0_j); keys [count][(k+1)][l][(k+1)][n]; an idx_j >= count gives c0_j"""
    keys, c0, c1 = R.u64(keys), R.u64(c0), R.u64(c1)
    out = c0.copy()
    for j, s in enumerate(idx):
        if s < len(keys):
            out[j] += G.external_product(keys[s], (c1[j] - c0[j])[None], b)[0]
    return out


def cmux_tree(keys, bits_idx, table, b):
    """vertical packing: table [2^m][(k+1)][n], bits_idx [batch][m] (bit 0 the least significant) -> [batch][(k+1)][n]"""
    table = R.u64(table)
    bits_idx = np.atleast_2d(bits_idx)
    batch, m = bits_idx.shape
    cur = np.broadcast_to(table, (batch,) + table.shape).copy()
    for i in range(m):
        half = cur.shape[1] // 2
        c0, c1 = cur[:, 0::2].reshape(-1, *table.shape[1:]), cur[:, 1::2].reshape(-1, *table.shape[1:])
        idx = np.repeat(bits_idx[:, i], half)
        cur = cmux(keys, idx, c0, c1, b).reshape(batch, half, *table.shape[1:])
    return cur[:, 0]


# ---- keys ----------------------------------------------------------------------------------------------------------
def pfksk(rng, mul, n, s, b, l, sigma):
    """k = 1: [(2)][n+1][l][(2)][n] under the GLWE key s [n]; K~ = (-s_0 .. -s_{n-1}, 1) (the extracted key of s, negated,
    then 1 for the body); entry [r][j][d] encrypts f_r(K~_j) g_d with f_0(x) = -s x, f_1(x) = x.
    mul(a [r][n], b [r][n]) -> the negacyclic products."""
    s = R.u64(s)
    kt = np.concatenate([U64(0) - s, np.array([1], dtype=np.uint64)])          # K~, n + 1 scalars
    g = np.array(G.gvalues(b, l), dtype=np.uint64)
    a = rng.integers(0, 1 << 64, (2, n + 1, l, n), dtype=np.uint64, endpoint=False)
    a_s = mul(a.reshape(-1, n), np.broadcast_to(s, (2 * (n + 1) * l, n))).reshape(2, n + 1, l, n)
    mu = np.zeros((2, n + 1, l, n), dtype=np.uint64)
    sc = kt[:, None] * g[None, :]                                               # K~_j g_d, [n+1][l]
    mu[0] = (U64(0) - sc)[:, :, None] * s[None, None, :]                        # -s K~_j g_d
    mu[1, :, :, 0] = sc
    out = np.empty((2, n + 1, l, 2, n), dtype=np.uint64)
    out[:, :, :, 0, :] = a
    out[:, :, :, 1, :] = a_s + mu + R.errors(rng, (2, n + 1, l, n), sigma)
    return out


def tglwe_phase(mul, ct, s):
    """ct [..][(2)][n] -> b - a s, [..][n]"""
    ct = R.u64(ct)
    n = ct.shape[-1]
    a = ct[..., 0, :].reshape(-1, n)
    return (ct[..., 1, :].reshape(-1, n) - mul(np.ascontiguousarray(a), np.broadcast_to(R.u64(s), a.shape).copy())).reshape(ct.shape[:-2] + (n,))


def tlwe_phase(c, s):
    c, s = R.u64(c), R.u64(s)
    return c[..., -1] - c[..., :-1] @ s


def centred(x):
    return R.u64(x).view(np.int64)
