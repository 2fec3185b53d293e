// bfv_rns.hip — BFV on an RNS modulus chain: the exact basis extension, the scale-invariant product
// d -> round(t d / Q) over a second basis, and the client's message scaling and decryption.
//
//   chain      primes q_0 .. q_{k-1} (1 <= k <= 4, Q their product), the auxiliary base b_0 .. b_k (B their product), the special
//              prime P of the key switch, the plaintext modulus t; every prime distinct, below 2^62, one plan each, same n
//   admission  B > t n Q + 1: with operands centred in Q a tensor coefficient d has |d| <= n Q^2 / 2, so t d + floor(Q / 2)
//              lies inside (-Q B / 2, Q B / 2) and its quotient by Q inside (-B / 2, B / 2)
//   ciphertext [limb][2][batch][n] evals over all k limbs, the layout of ckks_eval.hip: BFV has no levels
//   extension  the residues of an integer x modulo m_0 .. m_{s-1} -> its residues modulo other primes, exactly, for x in [0, M)
//              or centred in (-M / 2, M / 2]: Garner's mixed-radix digits, a 128-bit sum per target (rns_tables.hpp)
//   product    out = floor((t d + floor(Q / 2)) / Q) mod q_i, d the negacyclic tensor over Z of the centred operands:
//              (1) operands to coefficients per limb, extended centred from Q to B, transformed in the k + 1 limbs of B (the
//                  evals modulo Q are the operands themselves);  (2) the tensor kernel per limb of Q u B, inverse transforms;
//              (3) u = t d + floor(Q / 2) in every limb, r = u mod Q extended (not centred) to B, y_j = (u_j - r_j) Q^-1 mod b_j:
//                  the quotient exactly;  (4) y extended centred from B to Q; forward transforms -> [k][3][batch][n]
//              (3) and (4) are one kernel, in place on the tensor's Q limbs; relinearisation is ckks_eval.hip's
//   dot        sum_r w_r d^(r) over pairs before the one division by Q: step (1) per pair, then ONE launch of
//              bfv_rns_tensorsum_kernel adds the pair's weighted tensor into all 2k + 1 limbs; steps (2, inverse) .. (4) and the
//              relinearisation once.  Admission B > t n Q W + 1, W the sum of the absolute weights
//   decrypt    v = c0 + c1 s per limb, centred in Q; m = floor((t v + floor(Q / 2)) / Q) mod t by (3) with b_0 alone (b_0 > 2 t + 2)
//
// All kernels are grid-stride and element-wise on fhe_ew_grid, bounds-checked against their element count, plain C++ with
// vector stores and no scratch: the tables arrive by value and are indexed by unrolled constants only.  The transforms run on
// the workspace (slot 13), one call per limb and direction over everything of that limb that is ready; a chunk is
// 2^21 / (7 (2k + 1) n) ciphertexts, at least one: 4 (2k + 1) slabs of operands and 3 (2k + 1) of tensor a ciphertext.
#include "bfv_client_kernels.hpp"
#include "rns_ext_device.hpp"
#include "rns_tables.hpp"

using fhe::u32;
using fhe::u64;

namespace fhe {

constexpr u32 kBfvMaxLimbs = 4, kBfvMaxAux = kBfvMaxLimbs + 1;

// the integer of digits a (less M where `neg`) modulo target t: sum_j a_j W[j][t], at most nine terms below 2^124, reduced once
template <u32 S, u32 T>
__device__ __forceinline__ u64 ext_target(const u64 (&a)[S], bool neg, u32 t, const ExtArgs<S, T> &e) {
    unsigned __int128 acc = 0;
#pragma unroll
    for (u32 j = 0; j < S; j++)
        if (j < e.s) acc += (unsigned __int128)a[j] * e.W[j][t];
    const u64 q = e.pq[t];
    u64 v = ext_csub(ext_red((u64)acc, q, e.ponep[t]) + ext_mul((u64)(acc >> 64), e.pr64[t], e.pr64p[t], q), q);
    if (neg) v = ext_csub(v + q - e.pM[t], q);
    return v;
}

// out[t out_ls + i] = the integer with residues in[j in_ls + i] modulo the sources, modulo target t; CENTRED: the integer is
// taken in (-M / 2, M / 2], otherwise in [0, M)
template <bool CENTRED>
__global__ __launch_bounds__(256) void rns_extend_kernel(const u64 *__restrict__ in, u64 in_ls, u64 *__restrict__ out, u64 out_ls, u64 count,
                                                         ExtArgs<kExtMax, kExtMax> e) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        u64 x[kExtMax], a[kExtMax];
#pragma unroll
        for (u32 j = 0; j < kExtMax; j++) x[j] = j < e.s ? in[j * in_ls + i] : 0ull;
        const bool gt = ext_digits(x, a, e);
#pragma unroll
        for (u32 t = 0; t < kExtMax; t++)
            if (t < e.t) out[t * out_ls + i] = ext_target(a, CENTRED && gt, t, e);
    }
}

// t x + floor(Q / 2) in one limb: {tw, twp} = t mod p and its companion, h = floor(Q / 2) mod p
struct ScaleLimb {
    u64 tw, twp, h;
};
struct ScaleArgs {
    ExtArgs<kBfvMaxLimbs, kBfvMaxAux> qb;   // Q -> B, not centred
    ExtArgs<kBfvMaxAux, kBfvMaxLimbs> bq;   // B -> Q, centred
    ScaleLimb lq[kBfvMaxLimbs], lb[kBfvMaxAux];
    u64 qinv[kBfvMaxAux], qinvp[kBfvMaxAux];   // Q^-1 mod b_j and its companion
};

// Steps (3) and (4) on `count` tensor coefficients: d [2k + 1][ls], limbs 0 .. k - 1 modulo q_i, k .. 2k modulo b_j; the k limbs
// of Q are overwritten by floor((t d + floor(Q / 2)) / Q) mod q_i.  A thread reads its 2k + 1 words before it writes.
__global__ __launch_bounds__(256) void bfv_rns_scale_kernel(u64 *d, u64 ls, u64 count, ScaleArgs s) {
    const u64 stride = (u64)gridDim.x * 256;
    const u32 k = s.qb.s;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        u64 u[kBfvMaxLimbs], ua[kBfvMaxLimbs], y[kBfvMaxAux], ya[kBfvMaxAux];
#pragma unroll
        for (u32 j = 0; j < kBfvMaxLimbs; j++) u[j] = j < k ? ext_csub(ext_mul(d[j * ls + i], s.lq[j].tw, s.lq[j].twp, s.qb.mq[j]) + s.lq[j].h, s.qb.mq[j]) : 0ull;
        ext_digits(u, ua, s.qb);                                     // r = u mod Q, in [0, Q)
#pragma unroll
        for (u32 j = 0; j < kBfvMaxAux; j++) {
            y[j] = 0;
            if (j <= k) {
                const u64 b = s.bq.mq[j];
                const u64 ub = ext_csub(ext_mul(d[(k + j) * ls + i], s.lb[j].tw, s.lb[j].twp, b) + s.lb[j].h, b);
                y[j] = ext_mul(ub + b - ext_target(ua, false, j, s.qb), s.qinv[j], s.qinvp[j], b);
            }
        }
        const bool gt = ext_digits(y, ya, s.bq);
#pragma unroll
        for (u32 j = 0; j < kBfvMaxLimbs; j++)
            if (j < k) d[j * ls + i] = ext_target(ya, gt, j, s.bq);
    }
}

struct DecryptArgs {
    ExtArgs<kBfvMaxLimbs, 1> qb;            // Q -> {b_0}
    ScaleLimb lq[kBfvMaxLimbs], lb;
    u64 qinv, qinvp;                        // Q^-1 mod b_0
    u64 t, t_onep;
};

// out[i] = floor((t v + floor(Q / 2)) / Q) mod t for the phase v centred in Q, its residues v [k][ls] in coefficients: v is
// extended centred to b_0, then step (3) with b_0 alone gives the quotient modulo b_0, which is centred (|quotient| <= t / 2 + 1
// < b_0 / 2) and reduced modulo t
__global__ __launch_bounds__(256) void bfv_rns_decrypt_kernel(const u64 *__restrict__ v, u64 ls, u64 *__restrict__ out, u64 count, DecryptArgs s) {
    const u64 stride = (u64)gridDim.x * 256;
    const u32 k = s.qb.s;
    const u64 b = s.qb.pq[0];
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        u64 x[kBfvMaxLimbs], xa[kBfvMaxLimbs], u[kBfvMaxLimbs], ua[kBfvMaxLimbs];
#pragma unroll
        for (u32 j = 0; j < kBfvMaxLimbs; j++) x[j] = j < k ? v[j * ls + i] : 0ull;
        const bool neg = ext_digits(x, xa, s.qb);
        const u64 vb = ext_target(xa, neg, 0, s.qb);
#pragma unroll
        for (u32 j = 0; j < kBfvMaxLimbs; j++) u[j] = j < k ? ext_csub(ext_mul(x[j], s.lq[j].tw, s.lq[j].twp, s.qb.mq[j]) + s.lq[j].h, s.qb.mq[j]) : 0ull;
        ext_digits(u, ua, s.qb);
        const u64 ub = ext_csub(ext_mul(vb, s.lb.tw, s.lb.twp, b) + s.lb.h, b);
        const u64 y = ext_mul(ub + b - ext_target(ua, false, 0, s.qb), s.qinv, s.qinvp, b);
        const bool yneg = y > (b >> 1);
        const u64 m = ext_red(yneg ? b - y : y, s.t, s.t_onep);
        out[i] = (yneg && m) ? s.t - m : m;
    }
}

// v^ = c0^ + c1^ (.) s^ over `count` words of one limb's rows of n = 2^L evals; s^ [n] is shared by the rows
__global__ __launch_bounds__(256) void bfv_rns_phase_kernel(const u64 *__restrict__ c0, const u64 *__restrict__ c1, const u64 *__restrict__ s, u64 *__restrict__ out,
                                                            u64 count, u32 L, Mod m) {
    const u64 stride = (u64)gridDim.x * 256, n = 1ull << L;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) out[i] = add63(c0[i], bfv_mulmod(c1[i], s[i & (n - 1)], m), m);
}

struct MsgArgs {
    u64 q[kBfvMaxLimbs], dw[kBfvMaxLimbs], dwp[kBfvMaxLimbs];   // q_i, floor(Q / t) mod q_i and its companion
    u32 k;
};
// out[j ls + i] = floor(Q / t) m[i] mod q_j, centred, as a signed word
__global__ __launch_bounds__(256) void bfv_rns_scale_msg_kernel(const u64 *__restrict__ msg, u64 *__restrict__ out, u64 ls, u64 count, MsgArgs a) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 x = msg[i];
#pragma unroll
        for (u32 j = 0; j < kBfvMaxLimbs; j++) {
            if (j < a.k) {
                const u64 w = ext_mul(x, a.dw[j], a.dwp[j], a.q[j]);
                out[j * ls + i] = w > (a.q[j] >> 1) ? w - a.q[j] : w;
            }
        }
    }
}

// ---- inner products: the weighted sum of the pairs' tensors before the one division by Q ------------------------
constexpr u32 kBfvAllLimbs = kBfvMaxLimbs + kBfvMaxAux;

// one limb of Q u B for one pair: its modulus, the weight's canonical residue (not read unless WEIGHTED) and the pair's operands,
// two components `cs` words apart each: the caller's ciphertexts for a limb of Q, the extended operands X for a limb of B
struct TensorSumLimb {
    Mod m;
    u64 w;
    const u64 *a, *b;
    u64 cs;
};
// Indexed by blockIdx.y, which is uniform: scalar loads from the kernel-argument segment, as DotGroup of ckks_eval.hip.
struct TensorSumArgs {
    TensorSumLimb l[kBfvAllLimbs];
};

// One pair into all 2k + 1 limbs of the summed tensor D [2k + 1][3][count] in ONE launch: blockIdx.y is the limb, `count` the words
// of a component, and per limb
//   d0[e] (+)= w a0[e] b0[e],  d1[e] (+)= w (a0[e] b1[e] + a1[e] b0[e]),  d2[e] (+)= w a1[e] b1[e]
// CARRY: the sums start from the canonical words the pairs before left in D; otherwise from zero.  WEIGHTED = false: w = 1.
// Overflow: every prime is below 2^62 (check_bfv_chain), so only MacAcc's narrow fold applies.  The weight is folded into a0 and
// a1 first (ckks_rns_tensorsum_kernel), so a term is a product of two canonical words, below 2^124; an accumulator holds a
// canonical carry-over and at most two terms: below 2^62 + 2^125.  Operands are only read; D is none of them (the workspace).
template <bool WEIGHTED, bool CARRY>
__global__ __launch_bounds__(256) void bfv_rns_tensorsum_kernel(u64 *__restrict__ D, u64 count, TensorSumArgs args) {
    const TensorSumLimb &l = args.l[blockIdx.y];
    const Mod m = l.m;
    const u64 *__restrict__ a = l.a, *__restrict__ b = l.b;
    const u64 cs = l.cs, w = l.w;
    u64 *__restrict__ out = D + 3ull * blockIdx.y * count;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        MacAcc d0, d1, d2;
        if (CARRY) {
            d0.v = out[i];
            d1.v = out[count + i];
            d2.v = out[2 * count + i];
        }
        u64 a0 = a[i], a1 = a[cs + i];
        const u64 b0 = b[i], b1 = b[cs + i];
        if (WEIGHTED) {
            a0 = mul_mod_var(w, a0, m);
            a1 = mul_mod_var(w, a1, m);
        }
        d0.mac(a0, b0);
        d1.mac(a0, b1);
        d1.mac(a1, b0);
        d2.mac(a1, b1);
        out[i] = d0.fold(m);
        out[count + i] = d1.fold(m);
        out[2 * count + i] = d2.fold(m);
    }
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

constexpr int kBfvRnsSlot = 13;   // fhe_workspace_get slot (12 is the CKKS evaluator's, which the relinearisation takes)

struct BfvChain {
    unsigned k = 0;
    u64 n = 0, t = 0;
    u32 L = 0;
    const fhe_ntt_plan *q[fhe::kBfvMaxLimbs] = {}, *b[fhe::kBfvMaxAux] = {};
    u64 qm[fhe::kBfvMaxLimbs] = {}, bm[fhe::kBfvMaxAux] = {};
};

int check_plans(const fhe_ntt_plan *const *plans, unsigned limbs, const char *who) {
    if (!plans) return fhe_fail(FHE_E_NULL, "%s: plans is NULL", who);
    if (limbs < 1 || limbs > fhe::kBfvMaxLimbs) return fhe_fail(FHE_E_INVALID, "%s: limbs=%u must be in [1, 4]", who, limbs);
    for (unsigned i = 0; i < limbs; i++)
        if (!plans[i]) return fhe_fail(FHE_E_NULL, "%s: plan %u is NULL", who, i);
    return FHE_OK;
}

// the chain primes, and with `aux` the auxiliary base of limbs + 1 primes and the admission B > t n Q + 1; `special` (may be
// NULL) only joins the test for repeated primes: the relinearisation checks the rest of it
int check_bfv_chain(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *aux, const fhe_ntt_plan *special, u64 t, BfvChain *c, const char *who) {
    int rc = check_plans(plans, limbs, who);
    if (rc != FHE_OK) return rc;
    if (aux)
        for (unsigned j = 0; j <= limbs; j++)
            if (!aux[j]) return fhe_fail(FHE_E_NULL, "%s: auxiliary plan %u is NULL", who, j);
    c->k = limbs;
    c->n = plans[0]->n;
    c->L = plans[0]->log_n;
    c->t = t;
    std::vector<const fhe_ntt_plan *> all;
    for (unsigned i = 0; i < limbs; i++) all.push_back(c->q[i] = plans[i]);
    for (unsigned j = 0; aux && j <= limbs; j++) all.push_back(c->b[j] = aux[j]);
    if (special) all.push_back(special);
    for (size_t i = 0; i < all.size(); i++) {
        if (all[i]->n != c->n) return fhe_fail(FHE_E_PARAM_MISMATCH, "%s: plan %zu has n=%llu, plan 0 n=%llu", who, i, (unsigned long long)all[i]->n, (unsigned long long)c->n);
        if (all[i]->q >= fhe::kExtModLimit) return fhe_fail(FHE_E_INVALID, "%s: modulus %llu is not below 2^62", who, (unsigned long long)all[i]->q);
        for (size_t j = 0; j < i; j++)
            if (all[i]->q == all[j]->q) return fhe_fail(FHE_E_INVALID, "%s: modulus %llu is repeated", who, (unsigned long long)all[i]->q);
    }
    if (c->n < 2) return fhe_fail(FHE_E_BAD_N, "%s: n must be at least 2", who);
    if (t < 2) return fhe_fail(FHE_E_INVALID, "%s: t=%llu must be at least 2", who, (unsigned long long)t);
    for (unsigned i = 0; i < limbs; i++) c->qm[i] = plans[i]->q;
    if (aux) {
        for (unsigned j = 0; j <= limbs; j++) c->bm[j] = aux[j]->q;
        if (!fhe::host::bfv_admits(c->bm, limbs + 1, c->qm, limbs, t, c->n, 1)) return fhe_fail(FHE_E_INVALID, "%s: the auxiliary base must exceed t n Q + 1", who);
    }
    return FHE_OK;
}

// t mod p with its companion and floor(Q / 2) mod p
fhe::ScaleLimb scale_limb(u64 t, const fhe::host::Big &half_q, u64 p) {
    const u64 tw = t % p;
    return fhe::ScaleLimb{tw, fhe::host::shoup(tw, p), half_q.mod(p)};
}
bool q_inverse(const BfvChain &c, u64 b, u64 *inv, u64 *invp) {
    if (!fhe::host::inv_mod_any(fhe::host::big_product(c.qm, c.k).mod(b), b, inv)) return false;
    *invp = fhe::host::shoup(*inv, b);
    return true;
}

int scale_args(const BfvChain &c, fhe::ScaleArgs *s, const char *who) {
    const unsigned k = c.k;
    if (!fhe::host::ext_tables(c.qm, k, c.bm, k + 1, &s->qb) || !fhe::host::ext_tables(c.bm, k + 1, c.qm, k, &s->bq))
        return fhe_fail(FHE_E_INVALID, "%s: the moduli are not pairwise coprime", who);
    fhe::host::Big half = fhe::host::big_product(c.qm, k);
    half.divmod(2);
    for (unsigned i = 0; i < k; i++) s->lq[i] = scale_limb(c.t, half, c.qm[i]);
    for (unsigned j = 0; j <= k; j++) {
        s->lb[j] = scale_limb(c.t, half, c.bm[j]);
        if (!q_inverse(c, c.bm[j], &s->qinv[j], &s->qinvp[j])) return fhe_fail(FHE_E_INVALID, "%s: Q has no inverse modulo an auxiliary prime", who);
    }
    return FHE_OK;
}

// ciphertexts of a chunk: 2^21 / (7 (2k + 1) n), at least one; never above the key switch's own chunk (7 (2k + 1) >= k^2)
u64 bfv_chunk_rows(unsigned k, u32 L, u64 batch) { return std::min<u64>(batch, std::max<u64>(1, (kChunkWords >> L) / (7ull * (2 * k + 1)))); }
u64 bfv_words_per_row(unsigned k, u64 n) { return 7ull * (2 * k + 1) * n; }

template <unsigned S, unsigned T>
int extend_launch(bool centred, const u64 *in, u64 in_ls, u64 *out, u64 out_ls, u64 count, const fhe::ExtArgs<S, T> &e, u32 L, hipStream_t st) {
    fhe::ExtArgs<fhe::kExtMax, fhe::kExtMax> w{};                   // the one kernel takes the widest tables
    w.s = e.s;
    w.t = e.t;
    for (unsigned i = 0; i < S; i++) {
        w.mq[i] = e.mq[i];
        w.monep[i] = e.monep[i];
        w.half[i] = e.half[i];
        for (unsigned j = 0; j < S; j++) w.inv[j][i] = e.inv[j][i], w.invp[j][i] = e.invp[j][i];
        for (unsigned k = 0; k < T; k++) w.W[i][k] = e.W[i][k];
    }
    for (unsigned k = 0; k < T; k++) w.pq[k] = e.pq[k], w.ponep[k] = e.ponep[k], w.pr64[k] = e.pr64[k], w.pr64p[k] = e.pr64p[k], w.pM[k] = e.pM[k];
    return centred ? launch_named("rns_extend", "rns_extend_kernel", (int)L, st, fhe::rns_extend_kernel<true>, fhe_ew_grid(count), 256, in, in_ls, out, out_ls, count, w)
                   : launch_named("rns_extend", "rns_extend_kernel", (int)L, st, fhe::rns_extend_kernel<false>, fhe_ew_grid(count), 256, in, in_ls, out, out_ls, count, w);
}

// `polys` rows of evals, which the ABI aligns to 8 bytes, as coefficients in the workspace rows dst
int inverse_into(const fhe_ntt_plan *p, const u64 *src, u64 *dst, u64 polys, hipStream_t st) {
    const int rc = aligned_rows(src, dst, polys * p->n, st, &src);
    return rc != FHE_OK ? rc : fhe_ntt_inverse_dev(p, src, dst, polys, st);
}

// The workspace rows of a chunk of cr ciphertexts, slab = cr n words: X [2k + 1][4][slab] (the operands' coefficients, a0 a1 b0 b1
// per limb; the limbs of B then transformed), D = W + 4 (2k + 1) slab words, [2k + 1][3][slab] (the tensor).
//
// Step (1) for rows r0 .. r0 + cr of a, b [k][2][batch][n]: their coefficients per limb of Q, the centred extension to B and the
// forward transforms there -> the evals modulo b_j in the limbs k .. 2k of X
int extend_operand_rows(const BfvChain &c, const fhe::ScaleArgs &s, const u64 *a, const u64 *b, u64 batch, u64 r0, u64 cr, u64 *W, hipStream_t st) {
    const unsigned k = c.k;
    const u64 n = c.n, slab = cr * n;
    u64 *X = W;
    int rc;
    for (unsigned i = 0; i < k; i++) {                               // coefficients of the operands, limb by limb
        const u64 *op[2] = {a + ((u64)i * 2 * batch + r0) * n, b + ((u64)i * 2 * batch + r0) * n};
        for (unsigned o = 0; o < 2; o++) {
            u64 *dst = X + ((u64)i * 4 + 2 * o) * slab;
            if (cr == batch) {
                if ((rc = inverse_into(c.q[i], op[o], dst, 2 * cr, st)) != FHE_OK) return rc;
            } else {
                if ((rc = inverse_into(c.q[i], op[o], dst, cr, st)) != FHE_OK) return rc;
                if ((rc = inverse_into(c.q[i], op[o] + batch * n, dst + slab, cr, st)) != FHE_OK) return rc;
            }
        }
    }
    if ((rc = extend_launch(true, X, 4 * slab, X + 4ull * k * slab, 4 * slab, 4 * slab, s.qb, c.L, st)) != FHE_OK) return rc;
    for (unsigned j = 0; j <= k; j++) {
        u64 *xb = X + 4ull * (k + j) * slab;
        if ((rc = fhe_ntt_forward_dev(c.b[j], xb, xb, 4 * cr, st)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

// Steps (2, the inverse transforms), (3) and (4) on the chunk's tensor D, evals in all 2k + 1 limbs -> the scaled tensor as evals
// in the Q limbs of D, [k][3][cr][n]
int scale_tensor_rows(const BfvChain &c, const fhe::ScaleArgs &s, u64 cr, u64 *W, hipStream_t st) {
    const unsigned k = c.k, all = 2 * k + 1;
    const u64 slab = cr * c.n;
    u64 *D = W + 4ull * all * slab;
    int rc;
    for (unsigned l = 0; l < all; l++) {
        u64 *dl = D + 3ull * l * slab;
        if ((rc = fhe_ntt_inverse_dev(l < k ? c.q[l] : c.b[l - k], dl, dl, 3 * cr, st)) != FHE_OK) return rc;
    }
    if ((rc = launch("bfv_rns_scale", (int)c.L, st, fhe::bfv_rns_scale_kernel, fhe_ew_grid(3 * slab), 256, D, 3 * slab, 3 * slab, s)) != FHE_OK) return rc;   // (3), (4)
    for (unsigned i = 0; i < k; i++) {
        u64 *dl = D + 3ull * i * slab;
        if ((rc = fhe_ntt_forward_dev(c.q[i], dl, dl, 3 * cr, st)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

// Rows r0 .. r0 + cr of a, b [k][2][batch][n] -> the scaled tensor of the chunk as evals in the Q limbs of D, [k][3][cr][n]
int scaled_tensor_rows(const BfvChain &c, const fhe::ScaleArgs &s, const u64 *a, const u64 *b, u64 batch, u64 r0, u64 cr, u64 *W, hipStream_t st) {
    const unsigned k = c.k, all = 2 * k + 1;
    const u64 n = c.n, slab = cr * n;
    u64 *X = W, *D = W + 4ull * all * slab;
    int rc;
    if ((rc = extend_operand_rows(c, s, a, b, batch, r0, cr, W, st)) != FHE_OK) return rc;
    for (unsigned i = 0; i < k; i++)                                 // (2) the tensor per limb: modulo Q from the operands' own evals
        if ((rc = fhe_rns_tensor_limb(c.q[i], a + ((u64)i * 2 * batch + r0) * n, batch * n, b + ((u64)i * 2 * batch + r0) * n, batch * n, D + 3ull * i * slab, slab, slab,
                                      st)) != FHE_OK)
            return rc;
    for (unsigned j = 0; j <= k; j++) {
        const u64 *xb = X + 4ull * (k + j) * slab;
        if ((rc = fhe_rns_tensor_limb(c.b[j], xb, slab, xb + 2 * slab, slab, D + 3ull * (k + j) * slab, slab, slab, st)) != FHE_OK) return rc;
    }
    return scale_tensor_rows(c, s, cr, W, st);
}

// The weighted sum of the tensors of `count` pairs over rows r0 .. r0 + cr, scaled once -> as scaled_tensor_rows.  Per pair step
// (1) into X, then ONE launch adds its tensor into all 2k + 1 limbs of D; wres [count][2k + 1] the weights' canonical residues
// (Q's primes, then B's), NULL where every weight is 1.
int scaled_tensorsum_rows(const BfvChain &c, const fhe::ScaleArgs &s, const void *const *d_as, const void *const *d_bs, unsigned count, const u64 *wres, u64 batch,
                          u64 r0, u64 cr, u64 *W, hipStream_t st) {
    const unsigned k = c.k, all = 2 * k + 1;
    const u64 n = c.n, slab = cr * n;
    u64 *X = W, *D = W + 4ull * all * slab;
    for (unsigned r = 0; r < count; r++) {
        const u64 *a = (const u64 *)d_as[r], *b = (const u64 *)d_bs[r];
        int rc = extend_operand_rows(c, s, a, b, batch, r0, cr, W, st);
        if (rc != FHE_OK) return rc;
        fhe::TensorSumArgs args{};
        for (unsigned l = 0; l < all; l++) {
            fhe::TensorSumLimb &t = args.l[l];
            t.m = (l < k ? c.q[l] : c.b[l - k])->mod;
            t.w = wres ? wres[(u64)r * all + l] : 1;
            if (l < k) {
                t.a = a + ((u64)l * 2 * batch + r0) * n;
                t.b = b + ((u64)l * 2 * batch + r0) * n;
                t.cs = batch * n;
            } else {
                t.a = X + 4ull * l * slab;
                t.b = t.a + 2 * slab;
                t.cs = slab;
            }
        }
        const bool carry = r > 0;
        auto kernel = wres ? (carry ? fhe::bfv_rns_tensorsum_kernel<true, true> : fhe::bfv_rns_tensorsum_kernel<true, false>)
                           : (carry ? fhe::bfv_rns_tensorsum_kernel<false, true> : fhe::bfv_rns_tensorsum_kernel<false, false>);
        const hipError_t e = fhe::launch_grid(kernel, "bfv_rns_tensorsum", (int)c.L, dim3(fhe_ew_grid(slab), all), 256, 0, st, D, slab, args);
        if (e != hipSuccess) return fhe_hip_fail(e, "bfv_rns_tensorsum_kernel");
    }
    return scale_tensor_rows(c, s, cr, W, st);
}

int check_product_args(const BfvChain &c, const void *d_rlk, const void *d_a, const void *d_b, void *d_out, unsigned out_comps, size_t batch, const char *who) {
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 3ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_a || !d_b || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_a) || misaligned8(d_b) || misaligned8(d_out) || misaligned8(d_rlk)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8, rlk_bytes = (u64)c.k * (c.k + 1) * 2 * n * 8;
    if (overlaps_any(d_out, (u64)out_comps * c.k * batch * n * 8, {{d_a, ct_bytes}, {d_b, ct_bytes}, {d_rlk, rlk_bytes}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an operand or the key", who);
    return FHE_OK;
}

}  // namespace

extern "C" int fhe_rns_extend_dev(const uint64_t *src_mods, unsigned src, const uint64_t *dst_mods, unsigned dst, int centred, const void *d_in, void *d_out,
                                  size_t count, void *hip_stream) {
    const char *who = "fhe_rns_extend_dev";
    if (!src_mods || !dst_mods) return fhe_fail(FHE_E_NULL, "%s: NULL moduli", who);
    if (src < 1 || src > fhe::kExtMax || dst < 1 || dst > fhe::kExtMax) return fhe_fail(FHE_E_INVALID, "%s: %u source and %u target moduli, 1 to 9 each", who, src, dst);
    u64 sm[fhe::kExtMax], dm[fhe::kExtMax];
    for (unsigned i = 0; i < src; i++) sm[i] = src_mods[i];
    for (unsigned i = 0; i < dst; i++) dm[i] = dst_mods[i];
    for (unsigned side = 0; side < 2; side++) {
        const u64 *m = side ? dm : sm;
        for (unsigned i = 0; i < (side ? dst : src); i++) {
            if (m[i] < 3 || (m[i] & 1) == 0 || m[i] >= fhe::kExtModLimit)
                return fhe_fail(FHE_E_INVALID, "%s: modulus %llu must be odd, at least 3 and below 2^62", who, (unsigned long long)m[i]);
            for (unsigned j = 0; j < i; j++)
                if (m[j] == m[i]) return fhe_fail(FHE_E_INVALID, "%s: modulus %llu is repeated", who, (unsigned long long)m[i]);
        }
    }
    fhe::ExtArgs<fhe::kExtMax, fhe::kExtMax> e;
    if (!fhe::host::ext_tables(sm, src, dm, dst, &e)) return fhe_fail(FHE_E_INVALID, "%s: the source moduli are not pairwise coprime", who);
    if (count == 0) return FHE_OK;
    if (!mul_fits((u64)count, (u64)fhe::kExtMax, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: count too large", who);
    if (!d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_out, (u64)dst * count * 8, {{d_in, (u64)src * count * 8}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps d_in", who);
    int dev, rc = fhe_current_device(&dev);
    if (rc != FHE_OK) return rc;
    return extend_launch(centred != 0, (const u64 *)d_in, (u64)count, (u64 *)d_out, (u64)count, (u64)count, e, 0, (hipStream_t)hip_stream);
}

extern "C" size_t fhe_bfv_rns_workspace_bytes(uint64_t n, unsigned limbs, size_t batch) {
    if (n < 2 || (n & (n - 1)) != 0 || n > (1ull << 19) || limbs < 1 || limbs > fhe::kBfvMaxLimbs || batch == 0) return 0;
    const u64 cb = bfv_chunk_rows(limbs, log2_of(n), batch);
    return (size_t)(bfv_words_per_row(limbs, n) * cb * 8) + fhe_ckks_rns_galois_workspace_bytes(n, limbs, (size_t)cb, 1);
}

extern "C" int fhe_bfv_rns_tensor_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *aux, uint64_t t, const void *d_a, const void *d_b,
                                      void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_bfv_rns_tensor_dev";
    if (!aux) return fhe_fail(FHE_E_NULL, "%s: aux is NULL", who);
    BfvChain c;
    int rc = check_bfv_chain(plans, limbs, aux, nullptr, t, &c, who);
    if (rc != FHE_OK) return rc;
    fhe::ScaleArgs s;
    if ((rc = scale_args(c, &s, who)) != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if ((rc = check_product_args(c, nullptr, d_a, d_b, d_out, 3, batch, who)) != FHE_OK) return rc;
    REQUIRE_ALIGNED(d_out);
    hipStream_t st = (hipStream_t)hip_stream;
    const u64 n = c.n, cb = bfv_chunk_rows(c.k, c.L, batch);
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kBfvRnsSlot, (size_t)(bfv_words_per_row(c.k, n) * cb * 8), st, &w)) != FHE_OK) return rc;
    for (u64 r0 = 0; r0 < batch; r0 += cb) {
        const u64 cr = std::min<u64>(cb, batch - r0), slab = cr * n;
        if ((rc = scaled_tensor_rows(c, s, (const u64 *)d_a, (const u64 *)d_b, batch, r0, cr, (u64 *)w, st)) != FHE_OK) return rc;
        const u64 *D = (const u64 *)w + 4ull * (2 * c.k + 1) * slab;
        for (unsigned i = 0; i < c.k; i++)
            for (unsigned comp = 0; comp < 3; comp++)
                HIP_TRY(hipMemcpyAsync((u64 *)d_out + (((u64)i * 3 + comp) * batch + r0) * n, D + ((u64)i * 3 + comp) * slab, slab * 8, hipMemcpyDeviceToDevice, st));
    }
    return FHE_OK;
}

extern "C" int fhe_bfv_rns_mul_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *aux, const fhe_ntt_plan *special, uint64_t t,
                                   const void *d_rlk, const void *d_a, const void *d_b, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_bfv_rns_mul_dev";
    if (!aux) return fhe_fail(FHE_E_NULL, "%s: aux is NULL", who);
    if (!special) return fhe_fail(FHE_E_NULL, "%s: the special prime's plan is NULL", who);
    BfvChain c;
    int rc = check_bfv_chain(plans, limbs, aux, special, t, &c, who);
    if (rc != FHE_OK) return rc;
    for (unsigned i = 0; i < c.k; i++)
        if (special->q < c.qm[i]) return fhe_fail(FHE_E_INVALID, "%s: the special prime must not be below a chain prime", who);
    fhe::ScaleArgs s;
    if ((rc = scale_args(c, &s, who)) != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_rlk) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if ((rc = check_product_args(c, d_rlk, d_a, d_b, d_out, 2, batch, who)) != FHE_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const u64 n = c.n, cb = bfv_chunk_rows(c.k, c.L, batch);
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kBfvRnsSlot, (size_t)(bfv_words_per_row(c.k, n) * cb * 8), st, &w)) != FHE_OK) return rc;
    for (u64 r0 = 0; r0 < batch; r0 += cb) {
        const u64 cr = std::min<u64>(cb, batch - r0);
        if ((rc = scaled_tensor_rows(c, s, (const u64 *)d_a, (const u64 *)d_b, batch, r0, cr, (u64 *)w, st)) != FHE_OK) return rc;
        const u64 *D = (const u64 *)w + 4ull * (2 * c.k + 1) * cr * n;   // the chunk's tensor stays in the workspace
        if ((rc = fhe_rns_relin_rows(plans, limbs, special, (const u64 *)d_rlk, D, cr, (u64 *)d_out, batch, r0, st)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

extern "C" int fhe_bfv_rns_dot_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *aux, const fhe_ntt_plan *special, uint64_t t,
                                   const void *d_rlk, const void *const *d_as, const void *const *d_bs, unsigned count, const int64_t *w, void *d_out, size_t batch,
                                   void *hip_stream) {
    const char *who = "fhe_bfv_rns_dot_dev";
    if (!aux) return fhe_fail(FHE_E_NULL, "%s: aux is NULL", who);
    if (!special) return fhe_fail(FHE_E_NULL, "%s: the special prime's plan is NULL", who);
    BfvChain c;
    int rc = check_bfv_chain(plans, limbs, aux, special, t, &c, who);
    if (rc != FHE_OK) return rc;
    for (unsigned i = 0; i < c.k; i++)
        if (special->q < c.qm[i]) return fhe_fail(FHE_E_INVALID, "%s: the special prime must not be below a chain prime", who);
    if (count < 1 || count > FHE_BFV_DOT_MAX_COUNT) return fhe_fail(FHE_E_INVALID, "%s: count=%u must be in [1, %d]", who, count, FHE_BFV_DOT_MAX_COUNT);
    if (!d_as || !d_bs) return fhe_fail(FHE_E_NULL, "%s: NULL host array", who);
    const unsigned all = 2 * c.k + 1;
    fhe::u128 W = count;                                             // the sum of the absolute weights
    std::vector<u64> wres;                                           // [count][2k + 1] canonical residues, empty where w is NULL
    if (w) {
        W = 0;
        wres.resize((size_t)count * all);
        for (unsigned r = 0; r < count; r++) {
            const u64 mag = w[r] < 0 ? 0 - (u64)w[r] : (u64)w[r];
            if (mag == 0) return fhe_fail(FHE_E_INVALID, "%s: weight %u is zero", who, r);
            if (mag >= (1ull << 61)) return fhe_fail(FHE_E_INVALID, "%s: weight %u is not below 2^61 in absolute value", who, r);
            W += mag;
            for (unsigned l = 0; l < all; l++) {
                const u64 p = l < c.k ? c.qm[l] : c.bm[l - c.k], res = mag % p;
                wres[(size_t)r * all + l] = (w[r] < 0 && res) ? p - res : res;
            }
        }
    }
    if (!fhe::host::bfv_admits(c.bm, c.k + 1, c.qm, c.k, t, c.n, W))
        return fhe_fail(FHE_E_INVALID, "%s: the auxiliary base must exceed t n Q W + 1, W the sum of the absolute weights", who);
    fhe::ScaleArgs s;
    if ((rc = scale_args(c, &s, who)) != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 3ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_rlk || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_rlk) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8, rlk_bytes = (u64)c.k * (c.k + 1) * 2 * n * 8;
    if (overlaps_any(d_out, ct_bytes, {{d_rlk, rlk_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key", who);
    for (unsigned r = 0; r < count; r++) {
        if (!d_as[r] || !d_bs[r]) return fhe_fail(FHE_E_NULL, "%s: an operand of pair %u is NULL", who, r);
        if (misaligned8(d_as[r]) || misaligned8(d_bs[r])) return fhe_fail(FHE_E_INVALID, "%s: the operands of pair %u must be 8-byte aligned", who, r);
        if (overlaps_any(d_out, ct_bytes, {{d_as[r], ct_bytes}, {d_bs[r], ct_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an operand of pair %u", who, r);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const u64 cb = bfv_chunk_rows(c.k, c.L, batch);
    void *ws = nullptr;
    if ((rc = fhe_workspace_get(kBfvRnsSlot, (size_t)(bfv_words_per_row(c.k, n) * cb * 8), st, &ws)) != FHE_OK) return rc;
    for (u64 r0 = 0; r0 < batch; r0 += cb) {
        const u64 cr = std::min<u64>(cb, batch - r0);
        if ((rc = scaled_tensorsum_rows(c, s, d_as, d_bs, count, wres.empty() ? nullptr : wres.data(), batch, r0, cr, (u64 *)ws, st)) != FHE_OK) return rc;
        const u64 *D = (const u64 *)ws + 4ull * (2 * c.k + 1) * cr * n;   // the chunk's summed tensor stays in the workspace
        if ((rc = fhe_rns_relin_rows(plans, limbs, special, (const u64 *)d_rlk, D, cr, (u64 *)d_out, batch, r0, st)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

extern "C" int fhe_bfv_rns_scale_msg_dev(const fhe_ntt_plan *const *plans, unsigned limbs, uint64_t t, const void *d_msg, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_bfv_rns_scale_msg_dev";
    BfvChain c;
    int rc = check_bfv_chain(plans, limbs, nullptr, nullptr, t, &c, who);
    if (rc != FHE_OK) return rc;
    fhe::host::Big delta = fhe::host::big_product(c.qm, c.k);
    delta.divmod(t);                                                 // floor(Q / t)
    if (delta.w.empty()) return fhe_fail(FHE_E_INVALID, "%s: t must not exceed Q", who);
    if (batch == 0) return FHE_OK;
    const u64 n = c.n, count = (u64)batch * n;
    if (!mul_fits((u64)batch, (u64)c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_msg || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_msg) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_out, (u64)c.k * count * 8, {{d_msg, count * 8}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the messages", who);
    int dev;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    fhe::MsgArgs a{};
    a.k = c.k;
    for (unsigned i = 0; i < c.k; i++) {
        a.q[i] = c.qm[i];
        a.dw[i] = delta.mod(c.qm[i]);
        a.dwp[i] = fhe::host::shoup(a.dw[i], c.qm[i]);
    }
    return launch("bfv_rns_scale_msg", (int)c.L, (hipStream_t)hip_stream, fhe::bfv_rns_scale_msg_kernel, fhe_ew_grid(count), 256, d_msg, d_out, count, count, a);
}

extern "C" int fhe_bfv_rns_decrypt_dev(const fhe_ntt_plan *const *plans, unsigned limbs, uint64_t aux, uint64_t t, const void *d_s_evals, const void *d_ct, void *d_out,
                                       size_t batch, void *hip_stream) {
    const char *who = "fhe_bfv_rns_decrypt_dev";
    const u64 aux0 = aux;
    BfvChain c;
    int rc = check_bfv_chain(plans, limbs, nullptr, nullptr, t, &c, who);
    if (rc != FHE_OK) return rc;
    if (aux0 >= fhe::kExtModLimit || (aux0 & 1) == 0 || t >= (1ull << 60) || aux0 <= 2 * t + 2)
        return fhe_fail(FHE_E_INVALID, "%s: the auxiliary prime %llu must be odd, above 2 t + 2 and below 2^62", who, (unsigned long long)aux0);
    fhe::DecryptArgs s{};
    if (!fhe::host::ext_tables(c.qm, c.k, &aux0, 1, &s.qb) || !q_inverse(c, aux0, &s.qinv, &s.qinvp))
        return fhe_fail(FHE_E_INVALID, "%s: the moduli are not pairwise coprime", who);
    fhe::host::Big half = fhe::host::big_product(c.qm, c.k);
    half.divmod(2);
    for (unsigned i = 0; i < c.k; i++) s.lq[i] = scale_limb(t, half, c.qm[i]);
    s.lb = scale_limb(t, half, aux0);
    s.t = t;
    s.t_onep = (u64)((((unsigned __int128)1) << 64) / t);
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 2ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_s_evals || !d_ct || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_s_evals) || misaligned8(d_ct) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_out, (u64)batch * n * 8, {{d_s_evals, (u64)c.k * n * 8}, {d_ct, 2ull * c.k * batch * n * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key or the ciphertexts", who);
    hipStream_t st = (hipStream_t)hip_stream;
    const u64 cb = std::min<u64>(batch, std::max<u64>(1, (kChunkWords >> c.L) / c.k));
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kBfvRnsSlot, (size_t)((u64)c.k * cb * n * 8), st, &w)) != FHE_OK) return rc;
    u64 *V = (u64 *)w;
    for (u64 r0 = 0; r0 < batch; r0 += cb) {
        const u64 cr = std::min<u64>(cb, batch - r0), slab = cr * n;
        for (unsigned i = 0; i < c.k; i++) {
            const u64 *c0 = (const u64 *)d_ct + ((u64)i * 2 * batch + r0) * n;
            if ((rc = launch("bfv_rns_phase", (int)c.L, st, fhe::bfv_rns_phase_kernel, fhe_ew_grid(slab), 256, c0, c0 + (u64)batch * n, (const u64 *)d_s_evals + (u64)i * n,
                             V + i * slab, slab, c.L, c.q[i]->mod)) != FHE_OK)
                return rc;
            if ((rc = fhe_ntt_inverse_dev(c.q[i], V + i * slab, V + i * slab, cr, st)) != FHE_OK) return rc;
        }
        if ((rc = launch("bfv_rns_decrypt", (int)c.L, st, fhe::bfv_rns_decrypt_kernel, fhe_ew_grid(slab), 256, V, slab, (u64 *)d_out + r0 * n, slab, s)) != FHE_OK) return rc;
    }
    return FHE_OK;
}
