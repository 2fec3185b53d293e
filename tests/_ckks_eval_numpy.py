"""Restatement of the CKKS evaluator on an RNS modulus chain as DESIGN.md §22 defines it, on tests/_ckks_numpy.py's samplers
and encoder.  Nothing here calls the library under test.  Transforms and products are schoolbook arithmetic on Python integers
for n <= 64 (evaluation at the engine's points r_i = the transform of the monomial X, read once from the oracle) and the
oracle's `ntt` / `intt` / `pointwise_mul` above that.

    chain       primes q_0 .. q_L (1 <= L + 1 <= 8), a special prime P >= max q_i, all distinct, all 1 mod 2n; level l = limbs
                0 .. l, k = l + 1
    ciphertext  u64 [limb][2][batch][n], evaluation domain in the engine's order, canonical; dropping the top limb truncates
    secret      one ternary row (KEY row 0) as residues under every prime
    pk, fresh   K.public_key / K.encrypt per limb with the same seed and rows: residues of one integer ciphertext
    rlk         [j][i][2][n] evals, j <= L, i in {0 .. L, P}: (-a_ji s + e_j + [i = j] (P mod q_j) s^2, a_ji) mod q_i, the
                public key of row RLK_BASE + 64 slot + j under prime i plus the diagonal term
    tensor      per limb d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1
    lift        x mod q_j in coefficients, centred (x - q_j where x > floor(q_j / 2)), reduced modulo q_i
    relinearise inverse d2 per limb; digit j lifted to every limb i != j of {0 .. l, P}; forward; t_i = sum_j D_ji (.) rlk[j][i];
                r_i = (t_i - lift(t_P)) P^-1 mod q_i; out = (d0 + r0, d1 + r1)
    rescale     c'_i = (c_i - lift(c_l)) q_l^-1 mod q_i, i < l; level l - 1, scale / q_l; refused at level 0
    decrypt     limb 0: c0 + c1 s mod q_0 centred; exact while |m + e| < q_0 / 2
    test primes "the primes below 2^b": 2^b + 1 - 2n downward in steps of 2n, deterministic Miller-Rabin; q_0 the first below
                2^b0, q_1 .. the first below 2^bD, P the first below 2^(b0 + 1)
"""
import numpy as np

import _ckks_numpy as K

U64, I64 = np.uint64, np.int64
RLK_BASE = 2 << 56
PK_BASE = 1 << 56
B_ERR = 29                     # the largest magnitude of tfhe.cdt_table(3.2): its number of thresholds
GRID_CAP = 1 << 20             # threads of an element-wise launch: 4096 blocks of 256, one element per thread and pass
CHUNK_WORDS = 1 << 21          # a chunk is CHUNK_WORDS / (n k^2) ciphertexts, at least one


# ---- primes -------------------------------------------------------------------------------------------------------------------
def is_prime(x):
    """deterministic Miller-Rabin for x < 2^64 (the first twelve primes as bases)"""
    if x < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if x % p == 0:
            return x == p
    d, r = x - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in small:
        y = pow(a, d, x)
        if y in (1, x - 1):
            continue
        for _ in range(r - 1):
            y = y * y % x
            if y == x - 1:
                break
        else:
            return False
    return True


def primes_below(b, n, count):
    out, c = [], (1 << b) + 1 - 2 * n
    while len(out) < count:
        if is_prime(c):
            out.append(c)
        c -= 2 * n
    return out


def chain(n, b0, bd, L):
    """-> ([q_0 .. q_L], P)"""
    return primes_below(b0, n, 1) + primes_below(bd, n, L), primes_below(b0 + 1, n, 1)[0]


# ---- transforms and element-wise arithmetic --------------------------------------------------------------------------------------
_O, _PTS = [], {}


def oracle():
    if not _O:
        from oracle import load_oracle
        _O.append(load_oracle())
    return _O[0]


def points(q, n):
    """(V, Vinv) as object matrices: V[i][j] = r_i^j, Vinv[j][i] = r_i^-j / n, r_i the engine's i-th evaluation point"""
    if (q, n) not in _PTS:
        x = np.zeros(n, dtype=U64)
        x[1] = 1
        r = [int(v) for v in oracle().ntt(q, n, x)]
        ninv = pow(n, -1, q)
        V = np.array([[pow(ri, j, q) for j in range(n)] for ri in r], dtype=object)
        Vi = np.array([[pow(ri, -j, q) * ninv % q for ri in r] for j in range(n)], dtype=object)
        _PTS[(q, n)] = (V, Vi)
    return _PTS[(q, n)]


def _obj(a):
    return np.asarray(a, dtype=U64).astype(object)


def fwd(q, n, a):
    a = np.ascontiguousarray(a, dtype=U64)
    if n <= 64:
        return ((_obj(a) @ points(q, n)[0].T) % q).astype(U64)
    return oracle().ntt(q, n, a).reshape(a.shape)


def inv(q, n, a):
    a = np.ascontiguousarray(a, dtype=U64)
    if n <= 64:
        return ((_obj(a) @ points(q, n)[1].T) % q).astype(U64)
    return oracle().intt(q, n, a).reshape(a.shape)


def pmul(q, a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=U64), np.asarray(b, dtype=U64))
    if a.size <= 1 << 14:
        return ((_obj(a) * _obj(b)) % q).astype(U64)
    return oracle().pointwise_mul(q, np.ascontiguousarray(a), np.ascontiguousarray(b)).reshape(a.shape)


def padd(q, a, b):
    return (np.asarray(a, dtype=U64) + np.asarray(b, dtype=U64)) % U64(q)


def psub(q, a, b):
    return (np.asarray(a, dtype=U64) + (U64(q) - np.asarray(b, dtype=U64))) % U64(q)


def polymul(q, n, a, b):
    return inv(q, n, pmul(q, fwd(q, n, a), fwd(q, n, b)))


def residues(x, q):
    """signed words -> canonical residues"""
    return np.mod(np.asarray(x, dtype=I64), I64(q)).astype(U64)


def lift(x, qj, qi):
    x = np.asarray(x, dtype=U64)
    c = np.where(x > U64(qj // 2), x.astype(I64) - I64(qj), x.astype(I64))
    return np.mod(c, I64(qi)).astype(U64)


# ---- the scheme ---------------------------------------------------------------------------------------------------------------
def from_i64(mods, n, m):
    """signed rows [batch][n] -> evals [limbs][batch][n]"""
    return np.stack([fwd(q, n, residues(m, q)) for q in mods])


def secret_evals(mods, n, s):
    return [fwd(q, n, residues(s, q)) for q in mods]


def public_key_coeffs(seed, row, s, q, cdt):
    n = len(s)
    a = K.uniform_row(seed, row, n, q)
    e = residues(K.errors(seed, 2 * row, n, 1, cdt)[0], q)
    return psub(q, e, polymul(q, n, a, residues(s, q))), a


def public_key(seed, row, s, mods, cdt):
    """-> evals [limbs][2][n]"""
    n = len(s)
    return np.stack([fwd(q, n, np.stack(public_key_coeffs(seed, row, s, q, cdt))) for q in mods])


def relin_key(seed, first_row, s, mods, P, cdt):
    """-> evals [limbs][limbs + 1][2][n]"""
    n, k = len(s), len(mods)
    out = np.zeros((k, k + 1, 2, n), dtype=U64)
    for j in range(k):
        for i, q in enumerate(list(mods) + [P]):
            ev = fwd(q, n, np.stack(public_key_coeffs(seed, first_row + j, s, q, cdt)))
            if i == j:
                se = fwd(q, n, residues(s, q))
                ev[0] = padd(q, ev[0], pmul(q, U64(P % q), pmul(q, se, se)))
            out[j, i] = ev
    return out


def encrypt(seed, first_row, pk, msg, rows, mods, cdt):
    """pk evals [limbs][2][n]; msg signed [rows][n] -> evals [limbs][2][rows][n]"""
    n = pk.shape[-1]
    v = K.ternary(seed, K.CKKS_EPH, first_row, n, rows)
    e = K.errors(seed, 2 * first_row, n, 2 * rows, cdt).reshape(rows, 2, n)
    out = []
    for i, q in enumerate(mods):
        ve = fwd(q, n, residues(v, q))
        c0 = padd(q, padd(q, pmul(q, ve, pk[i, 0]), fwd(q, n, residues(e[:, 0], q))), fwd(q, n, residues(msg, q)))
        c1 = padd(q, pmul(q, ve, pk[i, 1]), fwd(q, n, residues(e[:, 1], q)))
        out.append(np.stack([c0, c1]))
    return np.stack(out)


def phase_limb(q, n, s, c):
    """c [2][batch][n] evals -> c0 + c1 s mod q in coefficients"""
    return inv(q, n, padd(q, c[0], pmul(q, c[1], fwd(q, n, residues(s, q)))))


def decrypt(mods, n, s, ct):
    return K.centre(phase_limb(mods[0], n, s, ct[0]), mods[0])


def tensor(mods, a, b):
    """[k][2][batch][n] x 2 -> [k][3][batch][n]"""
    return np.stack([np.stack([pmul(q, a[i, 0], b[i, 0]), padd(q, pmul(q, a[i, 0], b[i, 1]), pmul(q, a[i, 1], b[i, 0])), pmul(q, a[i, 1], b[i, 1])])
                     for i, q in enumerate(mods)])


def key_switch_sums(mods, P, rlk, d2):
    """t [k + 1][2][batch][n] evals: t_i = sum_j D_ji (.) rlk[j][i] over the limbs {0 .. k - 1, P}"""
    k, n, kl = len(mods), d2.shape[-1], rlk.shape[0]
    coef = [inv(q, n, d2[j]) for j, q in enumerate(mods)]
    t = []
    for i, q in enumerate(list(mods) + [P]):
        col = i if i < k else kl
        acc = np.zeros((2,) + d2.shape[1:], dtype=U64)
        for j in range(k):
            D = d2[j] if i == j else fwd(q, n, lift(coef[j], mods[j], q))
            for c in range(2):
                acc[c] = padd(q, acc[c], pmul(q, D, rlk[j, col, c]))
        t.append(acc)
    return t


def div_round(mods, n, x, top_q, top, add=None):
    """per limb i: (x_i - lift(inverse transform of top)) top_q^-1 (+ add_i); x_i, top [2][batch][n] evals"""
    tc = inv(top_q, n, top)
    out = []
    for i, q in enumerate(mods):
        r = pmul(q, psub(q, x[i], fwd(q, n, lift(tc, top_q, q))), U64(pow(top_q, -1, q)))
        out.append(r if add is None else padd(q, r, add[i]))
    return np.stack(out)


def relinearize(mods, P, rlk, d):
    """d [k][3][batch][n] -> [k][2][batch][n]; rlk may be the key of a longer chain"""
    t = key_switch_sums(mods, P, rlk, d[:, 2])
    return div_round(mods, d.shape[-1], t[:-1], P, t[-1], add=d[:, :2])


def mul(mods, P, rlk, a, b):
    return relinearize(mods, P, rlk, tensor(mods, a, b))


def rescale(mods, c):
    """[k][2][batch][n] -> [k - 1][2][batch][n]"""
    if len(mods) < 2:
        raise ValueError("a ciphertext at level 0 cannot be rescaled")
    return div_round(mods[:-1], c.shape[-1], c[:-1], mods[-1], c[-1])


def add_plain(mods, n, c, m):
    out = c.copy()
    pt = from_i64(mods, n, m)
    for i, q in enumerate(mods):
        out[i, 0] = padd(q, c[i, 0], pt[i])
    return out


def mul_plain(mods, n, c, m):
    pt = from_i64(mods, n, m)
    return np.stack([np.stack([pmul(q, c[i, 0], pt[i]), pmul(q, c[i, 1], pt[i])]) for i, q in enumerate(mods)])


# ---- exact integers behind the residues -------------------------------------------------------------------------------------------
def crt_centred(mods, res):
    """res [k][...] residues -> object array of the centred integers modulo Q = prod mods"""
    Q = 1
    for q in mods:
        Q *= q
    acc = np.zeros(np.asarray(res[0]).shape, dtype=object)
    for q, r in zip(mods, res):
        Qi = Q // q
        acc = (acc + _obj(r) * (Qi * pow(Qi, -1, q))) % Q
    return np.where(acc > Q // 2, acc - Q, acc), Q


def negacyclic_int(a, s):
    """object [..][n] times a small signed row s [n] over the integers, schoolbook"""
    n = len(s)
    out = np.zeros(a.shape, dtype=object)
    for j in range(n):
        if int(s[j]) == 0:
            continue
        rolled = np.concatenate([-a[..., n - j:], a[..., :n - j]], axis=-1) if j else a
        out = out + rolled * int(s[j])
    return out


def phase_int(mods, n, s, comps):
    """comps [k][C][batch][n] evals (C = 2 or 3) -> the centred integer c0 + c1 s (+ c2 s^2) modulo Q, and Q"""
    total = None
    for c in range(comps.shape[1]):
        x, Q = crt_centred(mods, [inv(q, n, comps[i, c]) for i, q in enumerate(mods)])
        for _ in range(c):
            x = negacyclic_int(x, s)
        total = x if total is None else total + x
    total = total % Q
    return np.where(total > Q // 2, total - Q, total), Q


# ---- the noise terms of §22 (worst case, infinity norms of coefficients; a slot is bounded by the 1-norm <= n |.|_inf) ----------
def fresh_noise(n):
    """|e|_inf of c0 + c1 s - m for a fresh encryption: v e_pk + e0 + e1 s with ternary v, s"""
    return (2 * n + 1) * B_ERR


def relin_noise(n, k):
    """|c0 + c1 s - (d0 + d1 s + d2 s^2)|_inf <= k n B / 2 (sum_j D_j e_j / P, |D_j| <= q_j / 2 <= P / 2) + (n + 1) / 2 (the rounding)"""
    return k * n * B_ERR / 2 + (n + 1) / 2


def rescale_noise(n):
    """|c0' + c1' s - (c0 + c1 s) / q_l|_inf <= (n + 1) / 2"""
    return (n + 1) / 2


def functional_bounds(n, mods, delta, zmax):
    """slot-error bounds (err1, err2) of: one product of two fresh ciphertexts plus rescale, then the square of that result
    plus rescale.  Slot noise of a ciphertext = |sigma(c0 + c1 s) - scale z|_inf; products multiply slot-wise."""
    k = len(mods)
    f = n * (fresh_noise(n) + 0.5 + 2.0 ** -10)          # the encoder's rounding (and its f64 error, far below 2^-10) included
    n1 = 2 * delta * zmax * f + f * f + n * relin_noise(n, k)
    n1 = n1 / mods[k - 1] + n * rescale_noise(n)
    s1 = delta * delta / mods[k - 1]
    w = zmax * zmax
    n2 = 2 * s1 * w * n1 + n1 * n1 + n * relin_noise(n, k - 1)
    n2 = n2 / mods[k - 2] + n * rescale_noise(n)
    s2 = s1 * s1 / mods[k - 2]
    return n1 / s1, n2 / s2


# ---- the case lists that tests/test_ckks_eval_cpu.py proves and tests/test_ckks_eval_gpu.py runs ------------------------------------
def _seed(k):
    return bytes((k * 31 + 11 * i + 5) % 256 for i in range(32))


ARITH_KINDS = {0, 1, 2, 3, 4, 5}          # FHE_ARITH_SHOUP62, SHOUP61, PMERSENNE, WORD32, STRICT63, MONTGOMERY (include/fhe_ntt.h)


def montgomery_prime(b):
    """the first prime = 1 (mod 2^32) below 2^b"""
    c = (1 << b) - (1 << 32) + 1
    while not is_prime(c):
        c -= 1 << 32
    return c


def wide_chain(n):
    """eight limbs, the first one >= 2^62, two below 2^30, one = 1 (mod 2^32); P the next prime below 2^63.  At n >= 256 (where
    a modulus below 2^30 has its 32-bit form) they are of every arithmetic kind the plans distinguish (proved by the CPU module)"""
    top = primes_below(63, n, 2)
    return [top[1], 2305843009211596801, 65537, primes_below(62, n, 1)[0], montgomery_prime(60), primes_below(58, n, 1)[0],
            primes_below(40, n, 1)[0], primes_below(29, n, 1)[0]], top[0]


# (n, k, batch, chain): word-for-word cases; chain = (b0, bD) by the rule above, or "wide"
WORD_CASES = ([(n, k, b, (58, 40)) for n in (4, 16, 64) for k in (1, 2, 3) for b in (1, 3)]
              + [(16, 8, 1, "wide"), (16, 8, 3, "wide"), (256, 8, 3, "wide"), (1024, 3, 3, (58, 40)), (4096, 2, 257, (58, 40)), (4096, 1, 301, (58, 40))])


def chunk_rows(n, k, batch, rescale=False):
    """ciphertexts of a chunk: 2^21 / (n k^2), and 2^21 / (n k) for a rescale, at least one"""
    return min(batch, max(1, CHUNK_WORDS // (n * (k if rescale else k * k))))


def launch_elements(n, k, batch):
    """kernel -> the element counts of its launches when a word-for-word case runs every entry point (the chunks' last, shorter
    one included): tensor_dev whole, mul's tensor per chunk; from_i64 whole (the output is aligned); relinearisation's digit lifts
    and key sums a slab, its t_P lift and divide-and-round two; a rescale's lift and divide-and-round two slabs of its own chunk"""
    def chunks(rows):
        return {rows * n, (batch % rows or rows) * n}
    rel = chunks(chunk_rows(n, k, batch))
    out = {"tensor": {batch * n} | rel, "lift_signed": {batch * n}, "lift": rel | {2 * c for c in rel}, "keymac": set(rel), "divround": {2 * c for c in rel}}
    if k > 1:
        res = {2 * c for c in chunks(chunk_rows(n, k, batch, rescale=True))}
        low = chunks(chunk_rows(n, k - 1, batch))                        # the lower-level relinearisation with the same key
        out["lift"] |= res | low | {2 * c for c in low}
        out["divround"] |= res | {2 * c for c in low}
        out["keymac"] |= low
    return out


def case_chain(n, k, spec):
    if spec == "wide":
        mods, P = wide_chain(n)
        return mods[:k], P
    return chain(n, spec[0], spec[1], k - 1)


def case_ct(mods, n, batch, comps, rng):
    r = np.random.default_rng(rng)
    return np.stack([r.integers(0, q, (comps, batch, n), dtype=np.uint64) for q in mods])


# functional cases of check 3: (n, b0, bD, L), Gaussian-integer slots in [0, 8), Delta = functional_delta
FUNCTIONAL = {
    "n32": dict(seed=_seed(1), n=32, b0=58, bd=40, L=2, rows=4, rng=1201),
    "n16": dict(seed=_seed(2), n=16, b0=40, bd=30, L=2, rows=4, rng=1202),
}
FUNCTIONAL_GPU = dict(FUNCTIONAL, n4096=dict(seed=_seed(3), n=4096, b0=58, bd=40, L=2, rows=2, rng=1203))
ZMAX = 7 * 2 ** 0.5


def functional_delta(mods, bd):
    """Delta = 2^bD where decryption's contract at limb 0 allows it, else the largest power of two that does: after the two
    rescales the scale is s2 = Delta^4 / (q_L^2 q_(L-1)), a coefficient of the encoding of slots of magnitude at most ZMAX^4
    (the square of a product) is at most s2 ZMAX^4, and that must stay below q_0 / 4 (half of the contract's q_0 / 2 is left
    to the noise)"""
    delta = float(1 << bd)
    while delta ** 4 / (mods[-1] ** 2 * mods[-2]) * ZMAX ** 4 >= mods[0] / 4:
        delta /= 2
    return delta


def functional_slots(case, which):
    r = np.random.default_rng(case["rng"] + 10 * which)
    shape = (case["rows"], case["n"] // 2)
    return r.integers(0, 8, shape).astype(np.float64) + 1j * r.integers(0, 8, shape).astype(np.float64)


def functional_run(case, cdt):
    """the whole of check 3 in the restatement -> every intermediate ciphertext, the decoded slots, the worst slot errors, the
    decoder's own f64 bound E_dec and the noise bounds: a decoded slot is within bounds[i] + edec[i] of the product"""
    n, rows = case["n"], case["rows"]
    mods, P = chain(n, case["b0"], case["bd"], case["L"])
    delta = functional_delta(mods, case["bd"])
    s = K.secret_key(case["seed"], 0, n)
    pk = public_key(case["seed"], PK_BASE, s, mods, cdt)
    rlk = relin_key(case["seed"], RLK_BASE, s, mods, P, cdt)
    z1, z2 = functional_slots(case, 1), functional_slots(case, 2)
    m1, m2 = K.encode(z1, delta), K.encode(z2, delta)
    ct1 = encrypt(case["seed"], 0, pk, m1, rows, mods, cdt)
    ct2 = encrypt(case["seed"], rows, pk, m2, rows, mods, cdt)
    prod = rescale(mods, mul(mods, P, rlk, ct1, ct2))
    s1 = delta * delta / mods[-1]
    sq = rescale(mods[:-1], mul(mods[:-1], P, rlk, prod, prod))
    s2 = s1 * s1 / mods[-2]
    d1, d2 = decrypt(mods, n, s, prod), decrypt(mods, n, s, sq)
    w1, w2 = K.decode(d1, s1), K.decode(d2, s2)
    e1, e2 = float(np.abs(w1 - z1 * z2).max()), float(np.abs(w2 - (z1 * z2) ** 2).max())
    return dict(mods=mods, P=P, delta=delta, s=s, pk=pk, rlk=rlk, m1=m1, m2=m2, ct1=ct1, ct2=ct2, prod=prod, sq=sq, s1=s1, s2=s2, d1=d1, d2=d2, w1=w1, w2=w2,
                z1=z1, z2=z2, err1=e1, err2=e2, edec=(float(K.e_dec(d1, s1).max()), float(K.e_dec(d2, s2).max())),
                bounds=functional_bounds(n, mods, delta, ZMAX))
