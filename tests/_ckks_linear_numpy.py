"""Restatement of the plaintext linear transforms of the CKKS evaluator as DESIGN.md §24 defines them, on
tests/_ckks_galois_numpy.py (the permutation, the digits) and tests/_ckks_eval_numpy.py (the chain, the transforms, the
divide-and-round).  Nothing here calls the library under test.

    inputs      ct [k][2][batch][n] evals at level k - 1; count Galois elements g_r, odd, in [1, 2n), repeats allowed; for g_r != 1
                the key gk_r [kl][kl + 1][2][n] of §23 (kl >= k), for g_r = 1 no key (None); plaintexts pts [outputs][count][k + 1][n],
                canonical evals under the k chain primes and, as limb k, under P, shared by the batch
    digits      D_{j,i} of §23 from the unpermuted c1, once per call
    key sums    t^(r)_{i,c}[x] = sum_j D_{j,i}[pi_{g_r}(x)] gk_r[j][i][c][x] mod q_i, i in {0 .. k - 1, P}
    weighted    U_{o,i,c} = sum_{r : g_r != 1} m_{o,r,i} t^(r)_{i,c} mod q_i
    down        R_{o,i,c} = (U_{o,i,c} - fwd_i(lift(inv_P(U_{o,P,c})))) P^-1 mod q_i: ONE modulus-down per output
    out         out_{o,i,0} = R_{o,i,0} + sum_r m_{o,r,i} c0_i[pi_{g_r}];  out_{o,i,1} = R_{o,i,1} + sum_{r : g_r = 1} m_{o,r,i} c1_i
                every g_r = 1: no digit, transform or modulus-down; U = 0 gives R = 0, so the two forms agree
    noise       |dec(out) - sum_r m_r sigma_{g_r}(dec(ct))|_inf <= (n + 1)/2 + sum_{r : g_r != 1} |m_r|_1 k n B / 2 (linear_noise)
    BSGS        d_t[s] = M[s][(s + t) mod N], N = n/2, on the rotation order; non-zero diagonals only; t = n1 j + i; the inner
                sum of giant step j uses roll(d_{n1 j + i}, +n1 j), and M w = sum_j roll(inner_j, -n1 j)
"""
import numpy as np

import _ckks_eval_numpy as E
import _ckks_galois_numpy as G

U64, I64 = np.uint64, np.int64
GROUP = 16                      # kDiagGroup: elements of one launch, by value
OUT_CAP = 2                     # kDiagOutputs: outputs whose accumulators one launch keeps in registers
MAX_OUTPUTS = 64                # FHE_CKKS_DIAG_MAX_OUTPUTS


# ---- the diagonal sum -----------------------------------------------------------------------------------------------------------
def key_sums(mods, P, gk, g, D):
    """t [k + 1][2][batch][n] for one element: D [k + 1][k][batch][n] read at pi_g, the key row at the index itself"""
    k, n, kl = len(mods), D.shape[-1], gk.shape[0]
    perm = G.galois_perm(n, g)
    t = []
    for i, q in enumerate(list(mods) + [P]):
        acc = np.zeros((2,) + D.shape[2:], dtype=U64)
        for j in range(k):
            for c in range(2):
                acc[c] = E.padd(q, acc[c], E.pmul(q, D[i, j][..., perm], gk[j, i if i < k else kl, c]))
        t.append(acc)
    return t


def diag_sum(mods, P, gks, gs, pts, ct):
    """-> [outputs][k][2][batch][n], by the definition above"""
    k, n = len(mods), ct.shape[-1]
    for g in gs:
        G.check_element(n, g)
    outputs = pts.shape[0]
    assert pts.shape[1:] == (len(gs), k + 1, n) and ct.shape[0] == k
    perms = [G.galois_perm(n, g) for g in gs]
    switched = [r for r, g in enumerate(gs) if g != 1]
    if switched:
        D = G.digits(mods, P, ct[:, 1])
        ts = {r: key_sums(mods, P, gks[r], gs[r], D) for r in switched}
    out = []
    for o in range(outputs):
        if switched:
            U = []
            for i, q in enumerate(list(mods) + [P]):
                acc = np.zeros((2,) + ct.shape[2:], dtype=U64)
                for r in switched:
                    for c in range(2):
                        acc[c] = E.padd(q, acc[c], E.pmul(q, pts[o, r, i], ts[r][i][c]))
                U.append(acc)
            R = E.div_round(mods, n, U[:-1], P, U[-1])
        else:
            R = np.zeros_like(ct)
        for i, q in enumerate(mods):
            for r, g in enumerate(gs):
                R[i, 0] = E.padd(q, R[i, 0], E.pmul(q, pts[o, r, i], ct[i, 0][..., perms[r]]))
                if g == 1:
                    R[i, 1] = E.padd(q, R[i, 1], E.pmul(q, pts[o, r, i], ct[i, 1]))
        out.append(R)
    return np.stack(out)


def plaintext_evals(mods, P, m):
    """signed rows [..][n] -> canonical evals [..][k + 1][n], limb k under P"""
    m = np.asarray(m, dtype=I64)
    n = m.shape[-1]
    return np.stack([E.fwd(q, n, E.residues(m, q)) for q in list(mods) + [P]], axis=-2)


def linear_noise(n, k, norms1):
    """|dec(out) - sum_r m_r sigma_{g_r}(dec(ct))|_inf.  Modulo Q P, U_0 + U_1 s = sum_r m_r (sum_j sigma(D_j) e_{r,j}) + P sum_r m_r
    sigma(c1 s) over the elements with a key; |sum_j sigma(D_j) e_{r,j}|_inf <= k n (P / 2) B as in §22, a product by m_r grows it by
    at most |m_r|_1 (the 1-norm of its centred coefficients), and the division by P rounds once for the whole sum:
    (n + 1)/2.  norms1: |m_r|_1 of the elements with g_r != 1; the addends m_r pi(c0) (and m_r c1 for the identity) are exact."""
    return (n + 1) / 2 + sum(norms1) * k * n * E.B_ERR / 2


# ---- baby-step giant-step ---------------------------------------------------------------------------------------------------------
def bsgs_diagonals(M, n1=None):
    """-> (n1, baby, giant, rows [len(giant)][len(baby)][N])"""
    M = np.asarray(M, dtype=np.complex128)
    N = M.shape[0]
    diag = {t: np.array([M[s, (s + t) % N] for s in range(N)]) for t in range(N)}
    kept = [t for t in range(N) if np.any(diag[t] != 0)] or [0]
    if n1 is None:
        n1 = int(np.ceil(np.sqrt(len(kept))))
    baby, giant = sorted({t % n1 for t in kept}), sorted({t // n1 for t in kept})
    rows = np.zeros((len(giant), len(baby), N), dtype=np.complex128)
    for t in kept:
        rows[giant.index(t // n1), baby.index(t % n1)] = np.roll(diag[t], n1 * (t // n1))
    return n1, baby, giant, rows


def bsgs_apply(n1, baby, giant, rows, w):
    """the sum the device takes, in floating point on the rotation order: w [..][N]"""
    acc = 0
    for a, j in enumerate(giant):
        inner = sum(rows[a, b] * np.roll(w, -i, axis=-1) for b, i in enumerate(baby))
        acc = acc + np.roll(inner, -n1 * j, axis=-1)
    return acc


def required_steps(n1, baby, giant):
    return sorted({i for i in baby if i} | {n1 * j for j in giant if j})


def matrices(N, rng):
    """name -> the test matrices at N slots: small Gaussian integers, dense, banded (five diagonals, wrapping) and one diagonal"""
    r = np.random.default_rng(rng)
    dense = r.integers(-3, 4, (N, N)) + 1j * r.integers(-3, 4, (N, N))
    s = np.arange(N)
    band = np.zeros((N, N), dtype=np.complex128)
    for t in (0, 1, 2, 3, N - 1):
        band[s, (s + t) % N] = dense[s, (s + t) % N]
    single = np.zeros((N, N), dtype=np.complex128)
    single[s, (s + 3) % N] = dense[s, (s + 3) % N] + (dense[s, (s + 3) % N] == 0)
    return {"dense": dense.astype(np.complex128), "banded": band, "single": single}


# ---- the case lists that tests/test_ckks_linear_cpu.py proves and tests/test_ckks_linear_gpu.py runs ----------------------------------
SEED = bytes((11 * i + 7) % 256 for i in range(32))
# (n, k, batch, chain)
WORD_CASES = ([(2, 1, 1, (58, 40))] + [(n, k, b, (58, 40)) for n in (4, 16, 64) for k in (1, 2, 3) for b in (1, 3)] + [(16, 8, 3, "wide")])
BIG_CASE = (4096, 2, 257, (58, 40))
OUTPUTS = (1, 2, OUT_CAP + 1)


def element_lists(n):
    """the element lists of the sweep, reduced modulo 2n: one element, the identity alone, a mix with the identity, a repeat, and
    a list one longer than the by-value group"""
    m = 2 * n
    long = [1 if t % 4 == 1 else (5 ** (t % 3)) % m for t in range(GROUP + 1)]
    return [[5 % m], [1], [1, 5 % m, m - 1], [5 % m, 5 % m, 25 % m], long]


def big_elements(n):
    return [1, 5, 2 * n - 1]


def launch_elements(n, k, batch):
    """the element counts of the diagmac launches of a word-for-word case: a slab of a chunk, at k limbs and (the full-chain
    key) at k - 1"""
    def chunks(kk):
        rows = E.chunk_rows(n, kk, batch)
        return {rows * n, (batch % rows or rows) * n}
    return chunks(k) | (chunks(k - 1) if k > 1 else set())


def workspace_bytes(n, k, batch, outputs):
    return (k * k + 3 * k + 2 * (k + 1) * min(outputs, OUT_CAP)) * n * E.chunk_rows(n, k, batch) * 8


def launch_counts(k, count, outputs, chunks, switched=True):
    """§24's formula: kernel-timer label -> launches of one fhe_ckks_rns_diag_sum_dev call"""
    groups, ogroups = -(-count // GROUP), -(-outputs // OUT_CAP)
    if not switched:
        return dict(lift=0, diagmac=chunks * ogroups * groups * k, keymac=0, divround=0)
    return dict(lift=chunks * (k + outputs), diagmac=chunks * ogroups * groups * (k + 1), keymac=0, divround=chunks * outputs * k)


def random_keys(mods, P, n, gs, rng):
    """canonical random words in the shape of a key per element, None for the identity: the words of the sum do not depend on
    the key being one"""
    r = np.random.default_rng(rng)
    k = len(mods)
    return [None if g == 1 else np.stack([np.stack([r.integers(0, q, (2, n), dtype=np.uint64) for q in list(mods) + [P]]) for _ in range(k)]) for g in gs]


def random_pts(mods, P, n, outputs, count, rng):
    r = np.random.default_rng(rng)
    return np.stack([r.integers(0, q, (outputs, count, n), dtype=np.uint64) for q in list(mods) + [P]], axis=2)


# ---- the functional case: a dense complex matrix times encrypted slots ------------------------------------------------------------------
FUNCTIONAL = {name: dict(case, seed=bytes((b + 53) % 256 for b in case["seed"])) for name, case in E.FUNCTIONAL.items()}
MMAX, WMAX = 3 * 2 ** 0.5, 7 * 2 ** 0.5      # matrix entries are Gaussian integers in [-3, 3], slots in [0, 8)


def functional_scales(n, mods, bd, terms):
    """(Delta of the ciphertext, Delta_pt = q_top): after the rescale the scale is Delta again, a result slot is at most
    terms MMAX WMAX (terms: the most non-zero entries of a row of M), and Delta n terms MMAX WMAX stays below q_0 / 4 (a
    coefficient is bounded by the slots' sum, n/2 slots and their conjugates)"""
    delta = float(1 << bd)
    while delta * n * terms * MMAX * WMAX >= mods[0] / 4:
        delta /= 2
    return delta, float(mods[-1])


def functional_bound(n, k, delta, dpt, q_top, baby, giant, rows_norm1, rows_max):
    """slot-error bound of linear_transform then rescale.  N_ct = n (fresh_noise + 1/2 + 2^-10), the slot noise of the input (a slot
    is bounded by the 1-norm <= n |.|_inf).  An inner sum of giant step j: sum_i (|d|_max Delta_pt N_ct + WMAX Delta n/2 (1/2 +
    2^-10) (the encoder's rounding of a diagonal, as slot noise n (1/2 + 2^-10), times the slot of the ciphertext)) + n
    linear_noise; its rotation adds n relin_noise; the rescale divides by q_top and adds n rescale_noise."""
    enc = n * (0.5 + 2.0 ** -10)
    n_ct = n * (E.fresh_noise(n) + 0.5 + 2.0 ** -10)
    total = 0.0
    for a, j in enumerate(giant):
        inner = sum(rows_max[a][b] * dpt * n_ct + enc * (WMAX * delta + n_ct) for b in range(len(baby)))
        inner += n * linear_noise(n, k, [rows_norm1[a][b] for b, i in enumerate(baby) if i])
        total += inner + (n * E.relin_noise(n, k) if j else 0)
    return (total / q_top + n * E.rescale_noise(n)) / (delta * dpt / q_top)
