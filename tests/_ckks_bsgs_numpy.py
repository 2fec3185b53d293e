"""Restatement of the baby-step giant-step linear transform with hoisted giant steps as DESIGN.md §30 defines it, on
tests/_ckks_linear_numpy.py (the key sums), tests/_ckks_galois_numpy.py (the permutation, the digits) and
tests/_ckks_eval_numpy.py (the chain, the transforms, the divide-and-round).  Nothing here calls the library under test.

    inputs      ct [k][2][batch][n] evals at level k - 1; baby elements g_b (b < B) and giant elements h_a (a < A), odd, in
                [1, 2n), repeats allowed, 1 the identity, which takes no key (None); the keys of §23's shape for the others;
                plaintexts pts [A][B][k + 1][n], canonical evals under the k chain primes and, as limb k, under P
    baby sums   U_{a,i,c} = sum_b m_{a,b,i} (t^(b)_{i,c} + (P mod q_i) A^(b)_{i,c}) mod q_i, i in {0 .. k - 1, P}: t^(b) the key sums of
                §24 for g_b (zero for g_b = 1), from the digits of c1 made once; the addends A^(b)_{i,0} = c0_i[pi_{g_b}] and
                A^(b)_{i,1} = c1_i for g_b = 1, zero otherwise; modulo P the addends vanish.  This is §24's U' before its division
    giants      V = 0 in the basis Q P.  h_a = 1: V += U_a.  Otherwise
                    w_{a,i} = (U_{a,i,1} - fwd_i(lift(inv_P(U_{a,P,1})))) P^-1 mod q_i     the modulus-down of component 1 alone
                    D^(a) = the §23 digits of w_a
                    S_{a,i,c}[x] = sum_j D^(a)_{j,i}[pi_{h_a}(x)] gk_{h_a}[j][i][c][x]
                    V_{i,0} += S_{a,i,0} + U_{a,i,0}[pi_{h_a}],  V_{i,1} += S_{a,i,1}               on every i, P included
    out         out_{i,c} = (V_{i,c} - fwd_i(lift(inv_P(V_{P,c})))) P^-1 mod q_i: ONE modulus-down of both components
    degenerate  every h_a = 1: V = sum_a U_a, so out is the sum of diag_sum's outputs taken before their division, rounded once; it
                is, word for word, diag_sum with ONE output over the A B elements (g_b repeated A times, plaintext m_{a,b} for
                element a B + b).  Every g_b = 1 and h_a = 1 as well: U_{a,i} = (P mod q_i) sum_b m_{a,b,i} ct_i and U_{a,P} = 0, the
                division is exact, out_i = sum_{a,b} m_{a,b,i} ct_i: no digit, transform or modulus-down is needed
    anchor      one giant h != 1, one baby g = 1, m = 1 on every limb: U_i = (P mod q_i) ct_i, U_P = 0, so w = c1 exactly (the
                rounding of w has nothing to round) and out = §23's apply_galois(ct, h), word for word
    noise       bsgs_noise below
"""
import numpy as np

import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_linear_numpy as LN

U64, I64 = np.uint64, np.int64
GROUP = LN.GROUP                # kDiagGroup: baby elements of one diagmac launch
PAIR = LN.OUT_CAP               # kDiagOutputs: giant steps whose inner sums one diagmac launch keeps in registers
MAX_BABIES = G.MAX_COUNT        # FHE_CKKS_GALOIS_MAX_COUNT
MAX_GIANTS = LN.MAX_OUTPUTS     # FHE_CKKS_DIAG_MAX_OUTPUTS


# ---- the definition -------------------------------------------------------------------------------------------------------------
def baby_sums(mods, P, gks, gs, pts, ct):
    """-> U [A][k + 1] of [2][batch][n]: step 1"""
    k, n = len(mods), ct.shape[-1]
    A = pts.shape[0]
    assert pts.shape[1:] == (len(gs), k + 1, n) and ct.shape[0] == k
    perms = [G.galois_perm(n, g) for g in gs]
    switched = [b for b, g in enumerate(gs) if g != 1]
    ts = {}
    if switched:
        D = G.digits(mods, P, ct[:, 1])
        ts = {b: LN.key_sums(mods, P, gks[b], gs[b], D) for b in switched}
    U = []
    for a in range(A):
        row = []
        for i, q in enumerate(list(mods) + [P]):
            acc = np.zeros((2,) + ct.shape[2:], dtype=U64)
            for b, g in enumerate(gs):
                term = ts[b][i].copy() if g != 1 else np.zeros_like(acc)
                if i < k:
                    term[0] = E.padd(q, term[0], E.pmul(q, U64(P % q), ct[i, 0][..., perms[b]]))
                    if g == 1:
                        term[1] = E.padd(q, term[1], E.pmul(q, U64(P % q), ct[i, 1]))
                for c in range(2):
                    acc[c] = E.padd(q, acc[c], E.pmul(q, pts[a, b, i], term[c]))
            row.append(acc)
        U.append(row)
    return U


def giant_w(mods, P, Ua):
    """w_a [k][batch][n]: the modulus-down by P of component 1 of U_a alone"""
    n = Ua[0].shape[-1]
    return E.div_round(mods, n, [u[1:2] for u in Ua[:-1]], P, Ua[-1][1:2])[:, 0]


def bsgs(mods, P, baby_gks, baby_gs, giant_gks, giant_gs, pts, ct, order=None):
    """-> [k][2][batch][n], by the definition above; order: the order in which the giant steps are added (any permutation)"""
    k, n = len(mods), ct.shape[-1]
    for g in list(baby_gs) + list(giant_gs):
        G.check_element(n, g)
    assert pts.shape[0] == len(giant_gs) and len(giant_gs) >= 1 and len(baby_gs) >= 1
    allm = list(mods) + [P]
    U = baby_sums(mods, P, baby_gks, baby_gs, pts, ct)
    V = [np.zeros((2,) + ct.shape[2:], dtype=U64) for _ in allm]
    for a in (range(len(giant_gs)) if order is None else order):
        h = giant_gs[a]
        if h == 1:
            for i, q in enumerate(allm):
                V[i] = E.padd(q, V[i], U[a][i])
            continue
        perm = G.galois_perm(n, h)
        S = LN.key_sums(mods, P, giant_gks[a], h, G.digits(mods, P, giant_w(mods, P, U[a])))
        for i, q in enumerate(allm):
            V[i][0] = E.padd(q, V[i][0], E.padd(q, S[i][0], U[a][i][0][..., perm]))
            V[i][1] = E.padd(q, V[i][1], S[i][1])
    return E.div_round(mods, n, V[:-1], P, V[-1])


def bsgs_noise(n, k, norms1, giant_switched):
    """|dec(out) - sum_a sigma_{h_a}(sum_b m_{a,b} sigma_{g_b}(dec(ct)))|_inf.  Modulo Q P, with X_a the exact inner sum,
        U_{a,0} + U_{a,1} s = P X_a + E_a,  E_a = sum_{b : g_b != 1} m_{a,b} (sum_j sigma(D_j) e_{b,j}),  |E_a|_inf <= sum_b |m_{a,b}|_1 k n (P / 2) B
    as in linear_noise.  A giant with a key divides component 1 alone: P w_a = U_{a,1} - [U_{a,1}]_P, so w_a = U_{a,1} / P - rho_a with
    |rho_a|_inf <= 1/2, and its key switch gives S_0 + S_1 s = P sigma_h(w_a) sigma_h(s) + E'_a, |E'_a|_inf <= k n (P / 2) B.  Its
    share of V is therefore sigma_h(U_{a,0}) + S_0 + S_1 s = P sigma_h(X_a) + sigma_h(E_a) + E'_a - P sigma_h(rho_a s): the rounding of w_a
    is multiplied by the key's secret sigma_h(s), ternary, so |rho_a s|_inf <= n / 2.  The final division rounds both components
    once: (n + 1) / 2.  Hence
        (n + 1) / 2  +  sum_{a : h_a != 1} (n / 2 + k n B / 2)  +  sum_a sum_{b : g_b != 1} |m_{a,b}|_1 k n B / 2.
    norms1 [A][..]: per giant step the 1-norms of the centred coefficients of the plaintexts of its babies with g_b != 1;
    giant_switched [A]: h_a != 1."""
    total = (n + 1) / 2
    for row, sw in zip(norms1, giant_switched):
        total += sum(row) * k * n * E.B_ERR / 2 + ((n / 2 + k * n * E.B_ERR / 2) if sw else 0)
    return total


def composed_noise(n, k, norms1, giant_switched):
    """the bound of the composition §24 runs: linear_noise per inner sum and relin_noise (§22) per rotated one"""
    return sum(LN.linear_noise(n, k, row) + (E.relin_noise(n, k) if sw else 0) for row, sw in zip(norms1, giant_switched))


def composed(mods, P, baby_gks, baby_gs, giant_gks, giant_gs, pts, ct):
    """RnsCiphertext.linear_transform restated: one diag_sum, apply_galois per giant with a key, adds"""
    inner = LN.diag_sum(mods, P, baby_gks, baby_gs, pts, ct)
    acc = None
    for a, h in enumerate(giant_gs):
        part = inner[a] if h == 1 else G.apply_galois(mods, P, giant_gks[a], inner[a], h)
        acc = part if acc is None else G.ct_add(mods, acc, part)
    return acc


# ---- the fold order of ckks_rns_giantmac_kernel -------------------------------------------------------------------------------------
def giantmac_fold_replay(q, k, carry):
    """The 128-bit accumulator of component 0 of the kernel at words q - 1 everywhere: on entry u + (v if carry), then k digit
    terms (q - 1)^2 with key_sum's folds at held = 1 (q >= 2^62: before every digit of odd index; otherwise none), and the
    last fold.  -> (the largest value the accumulator held, the word it stores)"""
    wide = q >> 62 != 0
    acc = (q - 1) * (2 if carry else 1)
    peak = acc
    for j in range(k):
        if wide and j and (1 + j) % 2 == 0:
            acc %= q
        acc += (q - 1) * (q - 1)
        peak = max(peak, acc)
    return peak, acc % q


# ---- the device's bookkeeping -------------------------------------------------------------------------------------------------------
def workspace_slabs(k):
    """slabs (ciphertexts of a chunk x n words) of the workspace: the ciphertext's C k, D k^2 and E 2k, the two U sets and V at
    2 (k + 1) each, and for a giant step C k, D k^2 and w k"""
    return (k * k + 3 * k + 2 * (k + 1) * (PAIR + 1)) + (k * k + 2 * k)


def workspace_bytes(n, k, batch):
    return workspace_slabs(k) * n * E.chunk_rows(n, k, batch) * 8


def launch_counts(k, baby_gs, giant_gs, chunks):
    """§30's formula: kernel-timer label -> launches of one fhe_ckks_rns_bsgs_dev call"""
    B, A = len(baby_gs), len(giant_gs)
    sb, sa = sum(g != 1 for g in baby_gs), sum(h != 1 for h in giant_gs)
    if sb == 0 and sa == 0:
        return dict(lift=0, diagmac=chunks * -(-(A * B) // GROUP) * k, giantmac=0, keymac=0, divround=0)
    return dict(lift=chunks * ((k if sb else 0) + sa * (1 + k) + 1), diagmac=chunks * -(-A // PAIR) * -(-B // GROUP) * (k + 1), giantmac=chunks * A * (k + 1), keymac=0,
                divround=chunks * (sa * k + k))


def moddowns(giant_gs):
    """component modulus-downs of (this form, the composed form): one per giant with a key and two at the end, against two per
    inner sum and two per rotation"""
    sa = sum(h != 1 for h in giant_gs)
    return sa + 2, 2 * len(giant_gs) + 2 * sa


# ---- the case lists that tests/test_ckks_bsgs_cpu.py proves and tests/test_ckks_bsgs_gpu.py runs ------------------------------------
SEED = bytes((13 * i + 5) % 256 for i in range(32))
# (n, k, batch, chain)
WORD_CASES = [(n, k, b, (58, 40)) for n in (4, 16, 64) for k in (1, 2, 3) for b in (1, 3)]
WIDE_CASE = (16, 8, 3, "wide")
BIG_CASE = (4096, 2, 257, (58, 40))
SWEEP = ([1, 5], [1, 25])                        # the sweep's babies and giants, reduced modulo 2n


def reduced(gs, n):
    return [g % (2 * n) for g in gs]


def element_cases(n):
    """(babies, giants) beside the sweep's: a giant with a key alone, the identity alone, three giants with one repeated
    (one more than a pair), 17 babies (one more than a group, the seventeenth with a key), 16 babies, one baby with a key, and
    the identity in both roles"""
    m = 2 * n
    long = [1 if t % 4 == 1 else (5 ** (t % 3)) % m for t in range(GROUP + 1)]
    return [([1, 5 % m], [5 % m]), ([1, 5 % m], [1]), ([1, 5 % m], [5 % m, m - 1, 5 % m]), (long, [1, 25 % m]), (long[:GROUP], [25 % m, 1]), ([5 % m], [1, 25 % m]),
            ([1], [1, 1, 1]), ([1, 1], [5 % m])]


def launch_elements(n, k, batch):
    """the element counts of the giantmac launches of a word-for-word case: a slab of a chunk, at k limbs and (the full-chain
    key) at k - 1"""
    return LN.launch_elements(n, k, batch)


def random_case(mods, P, n, batch, baby_gs, giant_gs, rng):
    """canonical random words for the ciphertext, the keys and the plaintexts: the words of the sum do not depend on the keys
    being keys"""
    ct = E.case_ct(mods, n, batch, 2, rng)
    return (ct, LN.random_keys(mods, P, n, baby_gs, rng + 1), LN.random_keys(mods, P, n, giant_gs, rng + 2),
            LN.random_pts(mods, P, n, len(giant_gs), len(baby_gs), rng + 3))


def edge_case(mods, P, n, batch, baby_gs, giant_gs):
    """every word q - 1, in the ciphertext, the keys and the plaintexts"""
    allm = list(mods) + [P]
    k = len(mods)
    ct = np.stack([np.full((2, batch, n), q - 1, dtype=U64) for q in mods])
    key = np.stack([np.stack([np.full((2, n), q - 1, dtype=U64) for q in allm]) for _ in range(k)])
    pts = np.stack([np.full((len(giant_gs), len(baby_gs), n), q - 1, dtype=U64) for q in allm], axis=2)
    return ct, [None if g == 1 else key for g in baby_gs], [None if h == 1 else key for h in giant_gs], pts


def functional_bound(n, k, delta, dpt, q_top, baby, giant, rows_norm1, rows_max):
    """slot-error bound of linear_transform_hoisted then rescale, as LN.functional_bound: per diagonal the ciphertext's slot noise
    N_ct times the diagonal and the encoder's rounding of the diagonal times the ciphertext's slot; then n bsgs_noise for the
    whole call in the place of n linear_noise per inner sum and n relin_noise per rotation; the rescale divides by q_top and
    adds n rescale_noise."""
    enc = n * (0.5 + 2.0 ** -10)
    n_ct = n * (E.fresh_noise(n) + 0.5 + 2.0 ** -10)
    total = sum(rows_max[a][b] * dpt * n_ct + enc * (LN.WMAX * delta + n_ct) for a in range(len(giant)) for b in range(len(baby)))
    total += n * bsgs_noise(n, k, [[rows_norm1[a][b] for b, i in enumerate(baby) if i] for a in range(len(giant))], [j != 0 for j in giant])
    return (total / q_top + n * E.rescale_noise(n)) / (delta * dpt / q_top)


def lower(pts, k):
    """the plaintexts one level down: limb k - 1 leaves, the special prime's stays"""
    return np.ascontiguousarray(np.delete(pts, k - 1, axis=2))
