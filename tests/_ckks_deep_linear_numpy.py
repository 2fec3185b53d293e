"""Restatement of the plaintext linear transforms on the deep CKKS chain as DESIGN.md §37 defines them, in Python integers on
tests/_ckks_deep_numpy.py (the grouped digits, the key sums' columns, the modulus-down by P) and tests/_ckks_linear_numpy.py (the
baby-step giant-step bookkeeping, the test matrices).  Nothing here calls the library under test.

    inputs      ct [l][2][batch][n] evals; count Galois elements g_r, odd, in [1, 2n), repeats allowed; for g_r != 1 the key
                gk_r [dnum][kl + alpha][2][n] of §36 (kl >= l), for g_r = 1 no key (None); plaintexts pts [outputs][count][l + alpha][n],
                canonical evals under the l chain primes and then under p_0 .. p_{alpha-1}, shared by the batch
    digits      D_{j,i} of §36 from the unpermuted c1, once per call
    key sums    t^(r)_{i,c}[x] = sum_j D_{j,i}[pi_{g_r}(x)] gk_r[j][col(i)][c][x] mod m_i, i over {q_0 .. q_{l-1}, p_0 .. p_{alpha-1}}
    weighted    U_{o,i,c} = sum_{r : g_r != 1} m_{o,r,i} t^(r)_{i,c} mod m_i
    down        R_{o,i,c} = (U_{o,i,c} - y) P^-1 mod q_i, y the centred integer of U modulo P: ONE modulus-down per output
    out         out_{o,i,0} = R_{o,i,0} + sum_r m_{o,r,i} c0_i[pi_{g_r}];  out_{o,i,1} = R_{o,i,1} + sum_{r : g_r = 1} m_{o,r,i} c1_i
The device carries the addends through the division as (P mod q_i) ct; (u + P a - y) P^-1 = (u - y) P^-1 + a exactly modulo q_i,
and P a vanishes modulo every special prime, so y and the words are the same.  This module adds them after the division.
"""
import numpy as np

import _ckks_deep_numpy as D
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_linear_numpy as LN

U64, I64 = np.uint64, np.int64
GROUP = 16                      # kDeepDiagGroup: elements of one launch, by value
OUT_CAP = 2                     # kDeepDiagOutputs: outputs whose accumulators one launch keeps in registers
MAX_OUTPUTS = 64                # FHE_CKKS_DIAG_MAX_OUTPUTS
MAX_COUNT = 256                 # FHE_CKKS_GALOIS_MAX_COUNT


# ---- the diagonal sum -----------------------------------------------------------------------------------------------------------
def key_sums(mods, specials, gk, g, Dg):
    """t [l + alpha][2][batch][n] for one element: the digits Dg [l + alpha][ng][batch][n] read at pi_g, the key at the index itself"""
    n = Dg.shape[-1]
    perm = G.galois_perm(n, g)
    return D.key_switch_sums(mods, specials, gk, Dg[:len(mods), 0], D=Dg[..., perm])   # the second operand only gives the shape


def diag_sum(mods, specials, gks, gs, pts, ct):
    """-> [outputs][l][2][batch][n], by the definition above"""
    l, alpha, n = len(mods), len(specials), ct.shape[-1]
    for g in gs:
        G.check_element(n, g)
    outputs = pts.shape[0]
    assert pts.shape[1:] == (len(gs), l + alpha, n) and ct.shape[0] == l
    perms = [G.galois_perm(n, g) for g in gs]
    switched = [r for r, g in enumerate(gs) if g != 1]
    targets = list(mods) + list(specials)
    if switched:
        Dg = D.digits(mods, specials, ct[:, 1])
        once = {}                                                    # a key object that recurs with its element: its sums once
        for r in switched:
            if (id(gks[r]), gs[r]) not in once:
                once[id(gks[r]), gs[r]] = key_sums(mods, specials, gks[r], gs[r], Dg)
        ts = {r: once[id(gks[r]), gs[r]] for r in switched}
    out = []
    for o in range(outputs):
        if switched:
            U = []
            for i, q in enumerate(targets):
                acc = np.zeros((2,) + ct.shape[2:], dtype=U64)
                for r in switched:
                    for c in range(2):
                        acc[c] = E.padd(q, acc[c], E.pmul(q, pts[o, r, i], ts[r][i][c]))
                U.append(acc)
            R = D.mod_down(mods, specials, U)
        else:
            R = np.zeros_like(ct)
        for i, q in enumerate(mods):
            for r, g in enumerate(gs):
                R[i, 0] = E.padd(q, R[i, 0], E.pmul(q, pts[o, r, i], ct[i, 0][..., perms[r]]))
                if g == 1:
                    R[i, 1] = E.padd(q, R[i, 1], E.pmul(q, pts[o, r, i], ct[i, 1]))
        out.append(R)
    return np.stack(out)


def plaintext_evals(mods, specials, m):
    """signed rows [..][n] -> canonical evals [..][l + alpha][n], the special primes' limbs last and in order"""
    m = np.asarray(m, dtype=I64)
    n = m.shape[-1]
    return np.stack([E.fwd(q, n, E.residues(m, q)) for q in list(mods) + list(specials)], axis=-2)


def ct_add(mods, a, b):
    return np.stack([E.padd(q, a[i], b[i]) for i, q in enumerate(mods)])


def linear_transform(mods, specials, n1, baby, giant, pts, gks, ct):
    """ckks.RnsCiphertext.linear_transform: one diagonal sum whose outputs are the giant steps' inner sums, then sigma_{5^(n1 j)}
    and + per non-zero giant step.  gks: step -> key.  -> (the inner sums, the result)"""
    n = ct.shape[-1]
    inner = diag_sum(mods, specials, [gks[i] if i else None for i in baby], [G.galois_element(n, i) for i in baby], pts, ct)
    acc = None
    for a, j in enumerate(giant):
        part = inner[a]
        if j:
            part = D.apply_galois(mods, specials, gks[n1 * j], part, G.galois_element(n, n1 * j))
        acc = part if acc is None else ct_add(mods, acc, part)
    return inner, acc


# ---- the noise of one diagonal sum (§37) ----------------------------------------------------------------------------------------------
def linear_noise(n, limbs, alpha, qj_over_p, norms1, b_err=E.B_ERR):
    """|dec(out) - sum_r m_r sigma_{g_r}(dec(ct))|_inf.  Modulo Q P, U_0 + U_1 s = sum_r m_r (sum_j sigma_{g_r}(x_j) e_{r,j}) + P sum_r
    m_r sigma_{g_r}(c1 s) over the elements with a key.  As in §36, |sum_j sigma(x_j) e_{r,j}|_inf <= dnum n (max_j Q_j / 2) B; the
    product by m_r grows it by at most |m_r|_1 (the 1-norm of its centred coefficients); the division by P turns max_j Q_j / 2 into
    max_j Q_j / (2 P) and rounds ONCE for the whole sum, y0 + y1 s with |y| <= 1/2: (n + 1) / 2.  norms1: |m_r|_1 of the elements
    with g_r != 1; the addends m_r pi(c0) (and m_r c1 for the identity) are exact."""
    return (n + 1) / 2 + sum(norms1) * D.dnum(limbs, alpha) * n * b_err * qj_over_p / 2


# ---- the workspace and the launch counts (include/fhe_ntt.h, §37) ----------------------------------------------------------------------
def slabs(limbs, alpha, outputs):
    """slabs of one ciphertext of a chunk: C l, D (l + alpha) ng - l, min(outputs, OUT_CAP) sets U of 2 (l + alpha), E 2l"""
    return limbs + ((limbs + alpha) * D.dnum(limbs, alpha) - limbs) + 2 * (limbs + alpha) * min(outputs, OUT_CAP) + 2 * limbs


def chunk_rows(n, limbs, alpha, batch, outputs):
    return min(batch, max(1, (D.CHUNK_WORDS // n) // slabs(limbs, alpha, outputs)))


def workspace_bytes(n, limbs, alpha, batch, count, outputs):
    if not (n >= 2 and n & (n - 1) == 0 and n <= 1 << 19 and 1 <= limbs <= D.MAX_LIMBS and 1 <= alpha <= D.MAX_SPECIALS and batch
            and 1 <= count <= MAX_COUNT and 1 <= outputs <= MAX_OUTPUTS):
        return 0
    return 8 * slabs(limbs, alpha, outputs) * n * chunk_rows(n, limbs, alpha, batch, outputs)


def launch_counts(limbs, alpha, count, outputs, chunks=1, switched=True):
    """kernel-timer label -> launches of one fhe_ckks_deep_diag_sum_dev call.  Every element the identity: one pass over the whole
    batch, whatever the chunk, over the chain limbs only."""
    groups, ogroups = -(-count // GROUP), -(-outputs // OUT_CAP)
    if not switched:
        return dict(extend=0, diagmac=limbs * ogroups * groups, keymac=0, divround=0)
    return dict(extend=chunks * (D.dnum(limbs, alpha) + outputs), diagmac=chunks * (limbs + alpha) * ogroups * groups, keymac=0, divround=chunks * outputs * limbs)


# ---- random operands: word equality needs no real keys ---------------------------------------------------------------------------------
def random_keys(mods, specials, n, gs, rng, key_limbs=None, key_mods=None):
    """canonical random words in the shape of a key per element, None for the identity.  key_mods: the chain the key was made
    for (default: mods)"""
    r = np.random.default_rng(rng)
    km = list(mods if key_mods is None else key_mods)
    ng = D.dnum(len(km), len(specials))
    return [None if g == 1 else np.stack([np.stack([r.integers(0, q, (2, n), dtype=np.uint64) for q in km + list(specials)]) for _ in range(ng)]) for g in gs]


def random_pts(mods, specials, n, outputs, count, rng):
    r = np.random.default_rng(rng)
    return np.stack([r.integers(0, q, (outputs, count, n), dtype=np.uint64) for q in list(mods) + list(specials)], axis=2)


def element_lists(n):
    """the element lists of the sweep, reduced modulo 2n: the identity first, last and alone, a repeated element, the conjugation,
    a full group of 16 and one more (one CARRY launch)"""
    m = 2 * n
    full = [1 if t % 5 == 2 else (5, m - 1, 25)[t % 3] % m for t in range(GROUP)]
    return [[1], [5 % m], [1, 5 % m, m - 1], [5 % m, 5 % m, 1], full, full + [25 % m]]


bsgs_diagonals, matrices = LN.bsgs_diagonals, LN.matrices
