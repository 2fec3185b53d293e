"""Restatement of the Galois automorphisms of the CKKS evaluator as DESIGN.md §23 defines them, on tests/_ckks_eval_numpy.py
(the chain, the transforms, relinearisation's six steps) and tests/_ckks_numpy.py (samplers, encoder).  Nothing here calls the
library under test.

    sigma_g     a(X) -> a(X^g) in Z[X]/(X^n + 1), g odd, 1 <= g < 2n; rotation by `step`: g = 5^(step mod n/2) mod 2n;
                conjugation: g = 2n - 1
    evals       index i of the engine's order holds the value at psi^(2 brv_L(i) + 1), so sigma_g(a)^[i] = a^[pi_g(i)],
                pi_g(i) = brv_L((((2 brv_L(i) + 1) g mod 2n) - 1) / 2); pi_g does not depend on q
    gk_g        [j][i][2][n] evals: (-a_ji s + e_j + [i = j] (P mod q_j) sigma_g(s), a_ji) mod q_i, rows GK_BASE + 64 slot + j
    apply       d0 = pi_g(c0), d1 = 0, d2 = pi_g(c1) per limb, then §22's steps (1)-(6) with gk_g for rlk: (pi_g(c0) + r0, r1)
    slots       the encoder keeps slot i at w^(2i+1); the rotation order is u_t = 5^t mod 2n, w[t] = z[(u_t - 1)/2] where
                u_t < n, else conj(z[(2n - u_t - 1)/2]); rotation by `step` is np.roll(w, -step), conjugation conj(z)
"""
import numpy as np

import _ckks_eval_numpy as E
import _ckks_numpy as K

U64, I64 = np.uint64, np.int64
GK_BASE = 3 << 56
MAX_COUNT = 256                 # FHE_CKKS_GALOIS_MAX_COUNT


# ---- the automorphism -----------------------------------------------------------------------------------------------------------
def brv(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def galois_element(n, step):
    return pow(5, step % max(n // 2, 1), 2 * n)


def conjugation_element(n):
    return 2 * n - 1


def check_element(n, g):
    if g % 2 == 0 or not 0 < g < 2 * n:
        raise ValueError(f"g={g} must be odd and in [1, 2n)")


def galois_perm(n, g):
    """pi_g as an index array: sigma_g(a)^ = a^[pi_g]"""
    check_element(n, g)
    L = n.bit_length() - 1
    return np.array([brv((((2 * brv(i, L) + 1) * g) % (2 * n) - 1) // 2, L) for i in range(n)], dtype=np.int64)


def galois_evals(a, g):
    a = np.asarray(a)
    return a[..., galois_perm(a.shape[-1], g)]


def galois_coeff_map(n, g):
    """(position, sign): coefficient j of a lands at position[j] of sigma_g(a) with sign[j]: X^(jg) = +-X^(jg mod n)"""
    e = (np.arange(n, dtype=np.int64) * g) % (2 * n)
    return e % n, np.where(e >= n, -1, 1)


def galois_coeffs(q, a, g):
    """the schoolbook substitution X -> X^g on canonical residues [..][n]"""
    a = np.asarray(a, dtype=U64)
    pos, sign = galois_coeff_map(a.shape[-1], g)
    out = np.zeros_like(a)
    out[..., pos] = np.where(sign < 0, (U64(q) - a) % U64(q), a)
    return out


def galois_int(a, g):
    """the same on signed or object integers"""
    a = np.asarray(a)
    pos, sign = galois_coeff_map(a.shape[-1], g)
    out = np.zeros_like(a)
    out[..., pos] = a * sign
    return out


# ---- the key and its application ----------------------------------------------------------------------------------------------------
def galois_key(seed, first_row, s, mods, P, cdt, g):
    """-> evals [limbs][limbs + 1][2][n]"""
    n, k = len(s), len(mods)
    check_element(n, g)
    out = np.zeros((k, k + 1, 2, n), dtype=U64)
    for j in range(k):
        for i, q in enumerate(list(mods) + [P]):
            ev = E.fwd(q, n, np.stack(E.public_key_coeffs(seed, first_row + j, s, q, cdt)))
            if i == j:
                se = galois_evals(E.fwd(q, n, E.residues(s, q)), g)
                ev[0] = E.padd(q, ev[0], E.pmul(q, U64(P % q), se))
            out[j, i] = ev
    return out


def apply_galois(mods, P, gk, ct, g):
    """ct [k][2][batch][n] -> [k][2][batch][n], by the definition: relinearisation of (pi_g(c0), 0, pi_g(c1)) against gk"""
    p = galois_evals(ct, g)
    d = np.stack([p[:, 0], np.zeros_like(p[:, 0]), p[:, 1]], axis=1)
    return E.relinearize(mods, P, gk, d)


def digits(mods, P, c1):
    """[k + 1][k][batch][n]: D_ji of §22 for d2 = c1 [k][batch][n], target i in {0 .. k - 1, P} first, digit j second"""
    k, n = len(mods), c1.shape[-1]
    coef = [E.inv(q, n, c1[j]) for j, q in enumerate(mods)]
    return np.stack([np.stack([c1[j] if i == j else E.fwd(q, n, E.lift(coef[j], mods[j], q)) for j in range(k)]) for i, q in enumerate(list(mods) + [P])])


# ---- slots ------------------------------------------------------------------------------------------------------------------------
def rotation_order(n):
    u = np.array([pow(5, t, 2 * n) for t in range(n // 2)], dtype=np.int64)
    conj = u >= n
    return np.where(conj, (2 * n - u - 1) // 2, (u - 1) // 2), conj


def to_rotation_order(z):
    z = np.asarray(z, dtype=np.complex128)
    idx, conj = rotation_order(2 * z.shape[-1])
    return np.where(conj, np.conj(z[..., idx]), z[..., idx])


def from_rotation_order(w):
    w = np.asarray(w, dtype=np.complex128)
    idx, conj = rotation_order(2 * w.shape[-1])
    z = np.empty_like(w)
    z[..., idx] = np.where(conj, np.conj(w), w)
    return z


# ---- rows -------------------------------------------------------------------------------------------------------------------------
def row_ranges():
    """purpose -> the half-open row ranges of §21, §22 and §23, in the order (§21 ..., §22, §23)"""
    b = 1 << 56
    return {"MASK": [(b, b + (1 << 16)), (2 * b, 2 * b + (1 << 22)), (3 * b, 3 * b + (1 << 22))],
            "ERR": [(0, 2 * b), (2 * b, 2 * b + (1 << 17)), (4 * b, 4 * b + (1 << 23)), (6 * b, 6 * b + (1 << 23))]}


# ---- the case lists that tests/test_ckks_galois_cpu.py proves and tests/test_ckks_galois_gpu.py runs ------------------------------------
SEED = bytes((7 * i + 3) % 256 for i in range(32))
# (n, k, batch, chain)
WORD_CASES = ([(2, 1, 1, (58, 40))] + [(n, k, b, (58, 40)) for n in (4, 16, 64) for k in (1, 2, 3) for b in (1, 3)]
              + [(16, 8, 3, "wide"), (256, 8, 3, "wide"), (4096, 2, 257, (58, 40))])


def case_elements(n):
    if n >= 256:
        return [5, 2 * n - 1]
    out = []
    for g in (1, 5 % (2 * n), pow(5, max(n // 2 - 1, 0), 2 * n), 2 * n - 1, (2 * n - 5) % (2 * n)):
        if g not in out:
            out.append(g)
    return out


def launch_elements(n, k, batch):
    """kernel -> the element counts of its launches when a word-for-word case runs: the bare automorphism over each limb's slab
    of 2 batch rows; the key sums a slab of a chunk and the divide-and-round two, at k limbs and (the full-chain key) at k - 1"""
    def chunks(kk):
        rows = E.chunk_rows(n, kk, batch)
        return {rows * n, (batch % rows or rows) * n}
    sl = chunks(k) | (chunks(k - 1) if k > 1 else set())
    return {"galois": {2 * batch * n}, "keymac_galois": sl, "divround_galois": {2 * c for c in sl}}


def workspace_bytes(n, k, batch):
    return (k * k + 5 * k + 2) * n * E.chunk_rows(n, k, batch) * 8


# ---- the functional case: the sum of all slots and its real part --------------------------------------------------------------------
FUNCTIONAL = {name: dict(case, seed=bytes((b + 101) % 256 for b in case["seed"])) for name, case in E.FUNCTIONAL.items()}
FUNCTIONAL_GPU = dict(FUNCTIONAL, n4096=dict(E.FUNCTIONAL_GPU["n4096"], seed=bytes((b + 101) % 256 for b in E.FUNCTIONAL_GPU["n4096"]["seed"])))


def functional_delta(n, mods, bd):
    """the largest power of two <= 2^bD with Delta n ZMAX < q_0 / 4: a coefficient of the encoding of slots of magnitude at most
    S is at most Delta S, the running sums reach n ZMAX (n/2 slots, doubled by the conjugate), and decryption's contract at limb
    0 is q_0 / 2, half of which is left to the noise"""
    delta = float(1 << bd)
    while delta * n * E.ZMAX >= mods[0] / 4:
        delta /= 2
    return delta


def functional_steps(n):
    """the Galois elements of the procedure, in order: rotations by 2^t, t < log2(n/2), then the conjugation"""
    return [galois_element(n, 1 << t) for t in range((n // 2).bit_length() - 1)] + [conjugation_element(n)]


def functional_bound(n, k, steps, delta):
    """N_0 = n (fresh + 1/2 + 2^-10); N <- 2 N + n relin_noise(n, k) per step: acc + sigma(acc) doubles the slot noise and the key
    switch adds its own (a slot is bounded by the 1-norm <= n |.|_inf) -> the slot-error bound N / Delta"""
    N = n * (E.fresh_noise(n) + 0.5 + 2.0 ** -10)
    for _ in range(steps):
        N = 2 * N + n * E.relin_noise(n, k)
    return N / delta


def ct_add(mods, a, b):
    return np.stack([E.padd(q, a[i], b[i]) for i, q in enumerate(mods)])


def functional_setup(case, cdt):
    n, rows = case["n"], case["rows"]
    mods, P = E.chain(n, case["b0"], case["bd"], case["L"])
    delta = functional_delta(n, mods, case["bd"])
    s = K.secret_key(case["seed"], 0, n)
    pk = E.public_key(case["seed"], E.PK_BASE, s, mods, cdt)
    z = E.functional_slots(case, 1)
    m = K.encode(z, delta)
    ct = E.encrypt(case["seed"], 0, pk, m, rows, mods, cdt)
    want = np.repeat(2 * z.real.sum(axis=-1, keepdims=True), n // 2, axis=-1).astype(np.complex128)
    return dict(mods=mods, P=P, delta=delta, s=s, pk=pk, z=z, m=m, ct=ct, want=want, gs=functional_steps(n),
                bound=functional_bound(n, len(mods), len(functional_steps(n)), delta))


def functional_run(case, cdt):
    """the whole procedure in the restatement: key slot t for step t"""
    r = functional_setup(case, cdt)
    mods, P, n = r["mods"], r["P"], case["n"]
    acc, gks, accs = r["ct"], [], []
    for t, g in enumerate(r["gs"]):
        gk = galois_key(case["seed"], GK_BASE + 64 * t, r["s"], mods, P, cdt, g)
        acc = ct_add(mods, acc, apply_galois(mods, P, gk, acc, g))
        gks.append(gk)
        accs.append(acc)
    d = E.decrypt(mods, n, r["s"], acc)
    w = K.decode(d, r["delta"])
    return dict(r, gks=gks, accs=accs, d=d, w=w, err=float(np.abs(w - r["want"]).max()), edec=float(K.e_dec(d, r["delta"]).max()))
