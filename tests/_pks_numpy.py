"""numpy restatement of DESIGN.md §16: the packing key switch (the public functional key switch TLWE -> TGLWE with `count`
ciphertexts packed at a stride), the box expansion that turns a packed TGLWE into §14's test vector, the bootstrap with a
test vector per row, packing key generation for the tests, and the ideal two-digit tree lookup.  k = 1; words are u64 and
wrap mod 2^64.  Built on tests/_gadget_numpy.py (§11), tests/_tfhe_numpy.py (§10) and tests/_lut_numpy.py (§14)."""
import numpy as np

import _gadget_numpy as G
import _lut_numpy as LN
import _tfhe_numpy as R

U64 = np.uint64


def digits_times_key(dig, key):
    """dig [m][q] int64 digits, key [q][c] u64 words -> dig @ key mod 2^64.  Where every partial sum stays below 2^53 the key
    is cut into four 16-bit limbs and each limb product is an exact float64 matrix product; otherwise numpy's wrapping
    uint64 product (slow, but the digits are then too wide for the limbs)"""
    dig, key = np.asarray(dig, dtype=np.int64), R.u64(key)
    if dig.size and int(np.abs(dig).max()) * 0xFFFF * dig.shape[1] >= 1 << 53:
        return dig.view(np.uint64) @ key
    out = np.zeros((dig.shape[0], key.shape[1]), dtype=np.uint64)
    df = dig.astype(np.float64)
    for m in range(4):
        limb = ((key >> U64(16 * m)) & U64(0xFFFF)).astype(np.float64)
        out += (df @ limb).astype(np.int64).view(np.uint64) << U64(16 * m)
    return out


def packing_key_switch(pksk, rows, b, l, count, log_stride):
    """pksk [n_in][l][2][n], rows [groups][count][n_in+1] -> [groups][2][n], word for word:
    out_g[r][c] = [r = 1] sum_i b_{g,i} [c = i stride] - sum_i sum_j sum_d sg(i, c) digit_d(a_{g,i,j}) pksk[j][d][r][(c - i stride) mod n],
    sg(i, c) = -1 when c < i stride, else +1"""
    pksk, rows = R.u64(pksk), R.u64(rows)
    n_in, _, k1, n = pksk.shape
    groups = rows.shape[0]
    assert rows.shape == (groups, count, n_in + 1) and pksk.shape[1] == l and 1 <= count and (count << log_stride) <= n
    stride = 1 << log_stride
    key = pksk.reshape(n_in * l, k1 * n)                                      # row (j, d), digit-major per word as the digits below
    c = np.arange(n)
    out = np.zeros((groups, k1, n), dtype=np.uint64)
    for i in range(count):
        dig = G.decompose(rows[:, i, :n_in], b, l).reshape(groups, n_in * l)
        col = (c - i * stride) % n
        sg = np.where(c < i * stride, U64((1 << 64) - 1), U64(1)).astype(np.uint64)              # -1 and +1 as words
        out -= digits_times_key(dig, key).reshape(groups, k1, n)[:, :, col] * sg[None, None, :]
        out[:, k1 - 1, i * stride] += rows[:, i, n_in]
    return out


def box_expand(ct, t):
    """ct [..][n] -> out[i] = sum_{u < box} in~[i + half - u], in~ the negacyclic extension (in~[j + n] = -in~[j]), box = n >> t,
    half = box / 2 (0 when box = 1), on every row"""
    ct = R.u64(ct)
    n = ct.shape[-1]
    L = int(n).bit_length() - 1
    assert 1 << L == n and 1 <= t <= L
    box = n >> t
    half = box // 2
    ext = np.concatenate([U64(0) - ct, ct, U64(0) - ct], axis=-1)            # in~[j] at index j + n, -n <= j < 2n
    i = np.arange(n)
    out = np.zeros(ct.shape, dtype=np.uint64)
    for u in range(box):
        out += ext[..., i + half - u + n]
    return out


def bootstrap_rows(n, b, l, bsk, tables, ks_b, ks_l, ksk, lwe):
    """tables [batch][2][n] (full TGLWEs), lwe [batch][n_lwe+1]: row r is the gadget bootstrap of lwe[r] with the test
    vector tables[r] (blind rotation over both components, extraction at 0, gadget key switch)"""
    tables, lwe = R.u64(tables), R.u64(lwe)
    acc = np.concatenate([G.blind_rotation(n, 1, b, l, bsk, tables[r], lwe[r:r + 1]) for r in range(lwe.shape[0])])
    return G.key_switch(ksk, R.sample_extraction(acc, 0), ks_b, ks_l)


def pksk(rng, mul, n, s_in, s, b, l, sigma):
    """k = 1: [n_in][l][2][n] under the GLWE key s [n]; entry [j][d] encrypts the constant polynomial s_in[j] g_d.
    mul(a [r][n], b [r][n]) -> the negacyclic products."""
    s_in, s = R.u64(s_in), R.u64(s)
    n_in = len(s_in)
    g = np.array(G.gvalues(b, l), dtype=np.uint64)
    a = rng.integers(0, 1 << 64, (n_in, l, n), dtype=np.uint64, endpoint=False)
    a_s = R.u64(mul(a.reshape(-1, n), np.broadcast_to(s, (n_in * l, n)))).reshape(n_in, l, n)
    mu = np.zeros((n_in, l, n), dtype=np.uint64)
    mu[:, :, 0] = s_in[:, None] * g[None, :]
    out = np.empty((n_in, l, 2, n), dtype=np.uint64)
    out[:, :, 0, :] = a
    out[:, :, 1, :] = a_s + mu + R.errors(rng, (n_in, l, n), sigma)
    return out


def pack_plain(words, n, log_stride):
    """words [..][count] -> the trivial TGLWEs [..][2][n] (mask 0) with words[i] at coefficient i 2^log_stride"""
    words = R.u64(words)
    out = np.zeros(words.shape[:-1] + (2, n), dtype=np.uint64)
    out[..., 1, (np.arange(words.shape[-1]) << log_stride)] = words
    return out


def ideal_tree_lookup(table2d, x_phase, y_phase, n):
    """what tree_lookup gives for these phases, noise aside: m_j = ideal lookup of y in table2d[j]; the m_j packed at stride
    box and expanded are the test vector of the table j -> m_j; its ideal lookup at x"""
    table2d = R.u64(table2d)
    P = table2d.shape[0]
    t, L = P.bit_length() - 1, int(n).bit_length() - 1
    x_phase, y_phase = np.atleast_1d(R.u64(x_phase)), np.atleast_1d(R.u64(y_phase))
    m = np.stack([LN.ideal_lookup(table2d[j], y_phase, n) for j in range(P)], axis=1)        # [batch][P]
    tv = box_expand(pack_plain(m, n, L - t), t)
    return np.array([R.rot(tv[r, 1], int(e))[0] for r, e in enumerate(R.mod_switch(x_phase, n))], dtype=np.uint64)
