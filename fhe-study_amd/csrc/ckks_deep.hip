// ckks_deep.hip — CKKS on a deep RNS chain: the hybrid key switch with grouped digits and several special
// primes, for chains of up to 32 limbs.  ckks_eval.hip (§22) keeps one digit per limb and one special prime, at most 8 limbs;
// this unit is the same route with the digits grouped, and at alpha = 1 it writes the same words.
//
//   chain      primes q_0 .. q_{L-1} (1 <= L <= 32) and special primes p_0 .. p_{alpha-1} (1 <= alpha <= 8, P their product), all
//              distinct, below 2^62, one plan each, same n
//   groups     digit group j holds limbs [j alpha, min((j + 1) alpha, l)) of the l limbs in use, G_j(l); dnum = ceil(L / alpha);
//              Q_j(l) the product of the group's primes.  Admission: P >= Q_j(L) for every j, exact (rns_tables.hpp: deep_admits)
//   key        [dnum][L + alpha][2][n] evals, column i < L modulo q_i, column L + m modulo p_m:
//              key[j][i] = (-a_ji s + e_j + [i in G_j(L)] (P mod q_i) s', a_ji), s' = s^2 or sigma_g(s); row first_row + j
//   switch     of d at l limbs: x_j the integer of the residues d mod q_i, i in G_j(l), centred in (-Q_j / 2, Q_j / 2];
//              D_ji = x_j mod m_i for every m_i of {q_0 .. q_{l-1}, p_0 .. p_{alpha-1}} (i in G_j: d's own limb, never lifted);
//              t_i = sum_j D_ji (.) key[j][col(i)]; y the centred integer of t modulo P; r_i = (t_i - y) P^-1 mod q_i
//   rescale    c'_i = (c_i - lift(c_top)) q_top^-1 mod q_i, §22's, for l up to 32
//   diag sum   out_o = sum_r m_{o,r} (.) sigma_{g_r}(ct) (§37): the digits of c1 once, the key sums of all elements weighted and
//              added in the basis Q P with the addends as (P mod q_i) ct, one modulus-down by P an output
//
// The kernels are grid-stride and element-wise on fhe_ew_grid, bounds-checked against their element count, plain C++ with
// vector stores and no scratch.  The tensor, the divide-and-round and the key's diagonal term are ckks_eval.hip's kernels,
// launched from that unit (capi_internal.hpp); the transforms are fhe_ntt_forward_dev / fhe_ntt_inverse_dev on the workspace
// (slot 14), one call per limb and direction over everything of that limb that is ready.
#include <map>

#include "bfv_client_kernels.hpp"
#include "rns_ext_device.hpp"
#include "rns_tables.hpp"

using fhe::Mod;
using fhe::u32;
using fhe::u64;

namespace fhe {

// dst[tab[t].off unit + i] = the integer with the canonical residues src[j src_ls + i] modulo the sources, centred in
// (-M / 2, M / 2], modulo target t, for every target: Garner's digits once, in registers, then one sum per target.  The
// source words are read once.  The targets (up to 39, 112 bytes each) pass the kernel-argument segment, so they lie in a
// device table; t is the loop counter, uniform over the wave, so an entry is read with scalar loads.
// Overflow: a digit is below its modulus and a weight below the target, both below 2^62, so a term is below 2^124 and the at
// most eight of a target below 2^127: one 128-bit accumulator, reduced once (the low word by ext_red, the high word times
// 2^64 mod q by ext_mul, each below q < 2^62, their sum below 2^63).
__global__ __launch_bounds__(256) void ckks_deep_extend_kernel(const u64 *__restrict__ src, u64 src_ls, u64 *__restrict__ dst, u64 unit, u64 count, DeepSrc e,
                                                               const DeepTarget *__restrict__ tab, u32 targets) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        u64 x[kDeepMaxSpecials], a[kDeepMaxSpecials];
#pragma unroll
        for (u32 j = 0; j < kDeepMaxSpecials; j++) x[j] = j < e.s ? src[j * src_ls + i] : 0ull;
        const bool gt = ext_digits(x, a, e);
        for (u32 t = 0; t < targets; t++) {
            const DeepTarget &d = tab[t];
            u128 acc = 0;
#pragma unroll
            for (u32 j = 0; j < kDeepMaxSpecials; j++)
                if (j < e.s) acc += (u128)a[j] * d.W[j];
            const u64 q = d.q;
            u64 v = ext_csub(ext_red((u64)acc, q, d.onep) + ext_mul((u64)(acc >> 64), d.r64, d.r64p, q), q);
            if (gt) v = ext_csub(v + q - d.pM, q);
            dst[d.off * unit + i] = v;
        }
    }
}

// One target limb of the key switch, ckks_rns_keymac_kernel's semantics with up to 32 digit groups:
// out[c][i] = sum_{j < k} D_j[s] key[j][c][i mod n], c = 0, 1, `count` words a component.  Digit j is own[s] for j = own_j (the
// limb's own group, read from the input's evals; `own` is not read for a special prime, whose own_j is k) and
// dig[(j - (j > own_j)) dig_stride + s] otherwise; its key row is key + j key_stride, [2][n], shared by the batch.
// GATHER (a Galois key switch): s is pi_g of the index within the row; the key is read at the index itself.
// Overflow: every modulus is below 2^62 and the operands are canonical, so a term is below 2^124.  The accumulators fold before
// digit j > 0 where j is a multiple of kMacChunk = 8: between two folds they hold a canonical carry-over below 2^62 and at most
// eight terms, less than 2^127 + 2^62 < 2^128 (MacAcc::fold).  32 digits are four such runs.
template <bool GATHER>
__global__ __launch_bounds__(256) void ckks_deep_keymac_kernel(const u64 *__restrict__ dig, u64 dig_stride, const u64 *__restrict__ own, u32 own_j,
                                                               const u64 *__restrict__ key, u64 key_stride, u64 *__restrict__ out, u32 k, u32 L, u64 count, u32 g,
                                                               Mod m) {
    const u64 stride = (u64)gridDim.x * 256, n = 1ull << L;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 x = i & (n - 1), s = GATHER ? i - x + galois_index((u32)x, g, L) : i;
        MacAcc a0, a1;
        for (u32 j = 0; j < k; j++) {
            if (j && j % kMacChunk == 0) {
                a0.fold(m);
                a1.fold(m);
            }
            const u64 d = j == own_j ? own[s] : dig[(u64)(j - (j > own_j ? 1u : 0u)) * dig_stride + s];
            const u64 *__restrict__ kp = key + (u64)j * key_stride + x;
            a0.mac(d, kp[0]);
            a1.mac(d, kp[n]);
        }
        out[i] = a0.fold(m);
        out[count + i] = a1.fold(m);
    }
}

// ---- plaintext linear transforms on the deep chain: the double-hoisted diagonal sum ----------------------------
constexpr u32 kDeepDiagGroup = 16;    // elements of one launch, passed by value
constexpr u32 kDeepDiagOutputs = 2;   // outputs whose accumulators one launch keeps in registers: no scratch, 8 waves a SIMD (§37)

// The elements of one launch for one target.  Indexed by the loop counter, which is uniform: the reads are scalar loads from
// the kernel-argument segment, not scratch.
struct DeepDiagGroup {
    const u64 *key[kDeepDiagGroup];   // element r's key rows of this target's column: digit j at + j key_stride, [2][n]; not read where g = 1
    const u64 *pt[kDeepDiagGroup];    // m_{o, r, i} [n] of the launch's first output; output o at + o pt_os
    u32 g[kDeepDiagGroup];
    u32 count;
};

// One target i of {q_0 .. q_{l-1}, p_0 .. p_{alpha-1}} of out_o = sum_r m_{o,r} (.) sigma_{g_r}(ct) in the extended basis, the
// grouped-digit form of ckks_rns_diagmac_kernel (§24): NOUT outputs and the elements of `grp`, over `count` words a component
// (rows of n = 2^L):
//   u_o[c][e] (+)= sum_r m_{o,r,i}[x] (t^(r)_c[e] + pmod ct_c[pi_{g_r}(e)] [c = 0 or g_r = 1]),  x = e mod n
//   t^(r)_c[e]   = sum_{j < k} D_j[pi_{g_r}(e)] key_r[j][c][x]                                    (zero for g_r = 1)
// D_j are ckks_deep_keymac_kernel's digits: `ct`'s second component for j = own_j, dig[(j - (j > own_j)) dig_stride + .]
// otherwise.  `ct` is limb i's two components, ct_cs words apart, and NULL for a special prime, where the addend vanishes, no
// digit is the target's own (own_j = k) and the identity is skipped.  With pmod = P mod q_i the addend rides through the
// division by P: (u + P a - E) P^-1 = (u - E) P^-1 + a.  With pmod = 1 and no element but the identity, u is the finished sum
// and `out` the output ciphertext.
// CARRY: u starts from the canonical words a former group of 16 left in `out`; otherwise from zero.
// Overflow.  Every modulus is below 2^62 (the deep chain refuses others, so there is no 2^62 <= q < 2^63 branch) and the operands
// are canonical, so a term is below 2^124.  Inner key sum: the accumulators hold the addend's one term, then take one term a
// digit and fold before every digit j > 0 where j is a multiple of kMacChunk = 8.  The first run is the addend and eight terms,
// 9 2^124 < 2^128; a later one a canonical carry-over below 2^62 and at most eight terms, less than 2^127 + 2^62 (MacAcc::fold).
// 32 digits are four runs.  Outer sum: u_o takes one term m t < 2^124 an element and folds before element r > 0 of the group
// where r is a multiple of 8: a carry-over below 2^62 (the last fold or the word CARRY read, both canonical) and at most eight
// terms.  An element that is skipped adds no term.  So any count holds: 256 elements are 16 groups, each folded to canonical
// words before it is stored.
template <u32 NOUT, bool CARRY>
__global__ __launch_bounds__(256) void ckks_deep_diagmac_kernel(const u64 *__restrict__ dig, u64 dig_stride, const u64 *__restrict__ ct, u64 ct_cs, u32 own_j,
                                                                u64 key_stride, u64 pt_os, u64 *__restrict__ out, u64 out_cs, u64 out_os, u32 k, u32 L, u64 count,
                                                                u64 pmod, DeepDiagGroup grp, Mod m) {
    const u64 stride = (u64)gridDim.x * 256, n = 1ull << L;
    const u64 *__restrict__ own = ct ? ct + ct_cs : nullptr;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 x = i & (n - 1);
        MacAcc u[NOUT][2];
        if (CARRY) {
#pragma unroll
            for (u32 o = 0; o < NOUT; o++) {
                u[o][0].v = out[o * out_os + i];
                u[o][1].v = out[o * out_os + out_cs + i];
            }
        }
        for (u32 r = 0; r < grp.count; r++) {
            if (r && r % kMacChunk == 0) {
#pragma unroll
                for (u32 o = 0; o < NOUT; o++) u[o][0].fold(m), u[o][1].fold(m);
            }
            const u32 g = grp.g[r];
            if (g == 1 && !ct) continue;                             // the identity contributes nothing modulo a special prime
            const u64 s = i - x + galois_index((u32)x, g, L);
            MacAcc a0, a1;
            if (ct) {
                a0.mac(ct[s], pmod);
                if (g == 1) a1.mac(ct[ct_cs + s], pmod);
            }
            if (g != 1) {
                const u64 *__restrict__ key = grp.key[r];
                for (u32 j = 0; j < k; j++) {
                    if (j && j % kMacChunk == 0) {
                        a0.fold(m);
                        a1.fold(m);
                    }
                    const u64 d = j == own_j ? own[s] : dig[(u64)(j - (j > own_j ? 1u : 0u)) * dig_stride + s];
                    const u64 *__restrict__ kp = key + (u64)j * key_stride + x;
                    a0.mac(d, kp[0]);
                    a1.mac(d, kp[n]);
                }
            }
            const u64 t0 = a0.fold(m), t1 = a1.fold(m);
            const u64 *__restrict__ pr = grp.pt[r] + x;
#pragma unroll
            for (u32 o = 0; o < NOUT; o++) {
                const u64 w = pr[o * pt_os];
                u[o][0].mac(w, t0);
                u[o][1].mac(w, t1);
            }
        }
#pragma unroll
        for (u32 o = 0; o < NOUT; o++) {
            out[o * out_os + i] = u[o][0].fold(m);
            out[o * out_os + out_cs + i] = u[o][1].fold(m);
        }
    }
}

// ---- polynomial evaluation on the deep chain: scalar sums and summed tensors over a slice of limbs a launch ----
// The per-limb kernels of ckks_eval.hip (§27, §29) launch once a limb; at 24 to 32 limbs and the small batches of the deep chain
// that is 24 to 32 launches of a few megabytes.  Here blockIdx.y is the limb within a slice of up to kDeepPolyLimbs = 8, and the
// slice's moduli, weights and constants pass by value, as bfv_rns_tensorsum_kernel's: they are indexed by blockIdx.y and by the
// loop counter, both uniform over the wave, so they are scalar loads from the kernel-argument segment.  Every modulus is below
// 2^62 (check_deep), so only MacAcc's narrow fold applies: there is no 2^62 <= q < 2^63 branch.
struct DeepLinArgs {
    Mod m[kDeepPolyLimbs];              // the slice's moduli
    DeepLinWords s;                     // w[l][o][r], k[l][o], canonical; k is not used where CARRY
    const u64 *ct[kDeepLinInputs];      // input r at the slice's first limb; limb l at + l limb_words
    u32 count;                          // inputs of this launch, 1 .. kDeepLinInputs
};
struct DeepDotArgs {
    Mod m[kDeepPolyLimbs];
    DeepDotWords s;                     // w[l][r], canonical; not read unless WEIGHTED
    const u64 *a[kDeepDotPairs], *b[kDeepDotPairs];   // pair r's operands at the slice's first limb and the chunk's first row; limb l at + l ls
    u32 count;                          // pairs of this launch, 1 .. kDeepDotPairs
};
// the kernel-argument segment that §36 keeps its by-value tables within; the scalars beside the struct are at most 64 bytes
static_assert(sizeof(DeepLinArgs) + 64 <= 4096 && sizeof(DeepDotArgs) + 64 <= 4096, "the slice's arguments pass by value within 4 KiB");

// Limb blockIdx.y of the slice of out_o = sum_r w[o][r] ct_r + (k[o], 0), ckks_rns_lincomb_kernel's semantics (§27) for NOUT
// outputs and the inputs of `a`: over the limb_words = 2 half words of a limb, component 0 first,
//   out[o out_os + l limb_words + e] (+)= sum_r w[l][o][r] ct_r[l limb_words + e] + [e < half] k[l][o].
// Every input has the layout [limb][2][batch][n], so a limb's words are limb_words apart in the inputs and in every output.
// CARRY: the sum starts from the canonical words a former group of inputs left in `out`; otherwise from the constant.
// Launches of one call: ceil(limbs / 8) ceil(outputs / 4) ceil(count / 8) (rns_tables.hpp: deep_lincomb_launches).
// Overflow.  Operands are canonical and every modulus is below 2^62, so a term is below 2^124.  The accumulator starts from a
// canonical word (the constant or the carried word) and folds before input r > 0 where r is a multiple of kMacChunk = 8: between
// two folds it holds a canonical carry-over below 2^62 and at most eight terms, less than 2^127 + 2^62 (MacAcc::fold).  A launch
// of kDeepLinInputs = 8 inputs is one such run, folded to canonical words before it is stored, so any count holds.
template <u32 NOUT, bool CARRY>
__global__ __launch_bounds__(256) void ckks_deep_lincomb_kernel(u64 *__restrict__ out, u64 out_os, u64 limb_words, u64 half, DeepLinArgs a) {
    const u32 l = blockIdx.y;
    const Mod m = a.m[l];
    const u64 base = (u64)l * limb_words, stride = (u64)gridDim.x * 256;
    u64 kk[NOUT];
#pragma unroll
    for (u32 o = 0; o < NOUT; o++) kk[o] = a.s.k[l][o];
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < limb_words; i += stride) {
        MacAcc u[NOUT];
#pragma unroll
        for (u32 o = 0; o < NOUT; o++) u[o].v = CARRY ? out[o * out_os + base + i] : (i < half ? kk[o] : 0ull);
        for (u32 r = 0; r < a.count; r++) {
            if (r && r % kMacChunk == 0) {
#pragma unroll
                for (u32 o = 0; o < NOUT; o++) u[o].fold(m);
            }
            const u64 x = a.ct[r][base + i];
#pragma unroll
            for (u32 o = 0; o < NOUT; o++) u[o].mac(a.s.w[l][o][r], x);
        }
#pragma unroll
        for (u32 o = 0; o < NOUT; o++) out[o * out_os + base + i] = u[o].fold(m);
    }
}

// Limb blockIdx.y of the slice of the summed tensor of the pairs of `a`, ckks_rns_tensorsum_kernel's semantics (§29), over
// `count` words a component; out is the slice's first limb of the chunk's tensor [limbs][3][count], canonical:
//   d0[e] (+)= sum_r w_r a_r0[e] b_r0[e],  d1[e] (+)= sum_r w_r (a_r0[e] b_r1[e] + a_r1[e] b_r0[e]),  d2[e] (+)= sum_r w_r a_r1[e] b_r1[e]
// An operand's limbs are ls words apart and its two components cs.  a_r and b_r may be the same pointer (a square) and a pointer
// may repeat across pairs: the operands are only read, and `out` (the workspace's tensor slot) is none of them.  WEIGHTED = false:
// w_r = 1, no multiplication.  CARRY: the sums start from the canonical words a former group left in `out`; otherwise from zero.
// Launches of one chunk: ceil(limbs / 8) ceil(count / 16) (rns_tables.hpp: deep_tensorsum_launches).
// Overflow.  The weight is folded into a_r first (w a_r0 and w a_r1 reduced to canonical words before they meet b: w a b < q^3 has
// no room in 128 bits), so a term is below 2^124 whether weighted or not.  d0 and d2 take one term a pair, d1 two, so d1 sets
// the period: all three fold before pair r > 0 where r is a multiple of kMacChunk / 2 = 4, and between two folds hold a canonical
// carry-over below 2^62 and at most eight terms, less than 2^127 + 2^62.  16 pairs are four runs; any count holds.
template <bool WEIGHTED, bool CARRY>
__global__ __launch_bounds__(256) void ckks_deep_tensorsum_kernel(u64 *__restrict__ out, u64 count, u64 ls, u64 cs, DeepDotArgs a) {
    const u32 l = blockIdx.y;
    const Mod m = a.m[l];
    const u64 in = (u64)l * ls, stride = (u64)gridDim.x * 256;
    out += 3ull * l * count;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        MacAcc d0, d1, d2;
        if (CARRY) {
            d0.v = out[i];
            d1.v = out[count + i];
            d2.v = out[2 * count + i];
        }
        for (u32 r = 0; r < a.count; r++) {
            if (r && r % (kMacChunk / 2) == 0) d0.fold(m), d1.fold(m), d2.fold(m);
            const u64 *pa = a.a[r] + in, *pb = a.b[r] + in;
            u64 a0 = pa[i], a1 = pa[cs + i];
            const u64 b0 = pb[i], b1 = pb[cs + i];
            if (WEIGHTED) {
                const u64 w = a.s.w[l][r];
                a0 = mul_mod_var(w, a0, m);
                a1 = mul_mod_var(w, a1, m);
            }
            d0.mac(a0, b0);
            d1.mac(a0, b1);
            d1.mac(a1, b0);
            d2.mac(a1, b1);
        }
        out[i] = d0.fold(m);
        out[count + i] = d1.fold(m);
        out[2 * count + i] = d2.fold(m);
    }
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

constexpr int kCkksDeepSlot = 14;   // fhe_workspace_get slot (12 and 13 are ckks_eval.hip's and bfv_rns.hip's)

struct Deep {
    unsigned k = 0, alpha = 0, ng = 0;                 // limbs in use, special primes, digit groups of the k limbs
    u64 n = 0;
    u32 L = 0;
    const fhe_ntt_plan *p[fhe::kDeepMaxTargets] = {};   // the chain's plans, then p[k + m] of special prime m
    unsigned group_of(unsigned i) const { return i < k ? i / alpha : ng; }   // a special prime is in no group
    // slabs in front of target i's lifted digits: limb i < k holds the ng - 1 digits of the other groups, a special prime all ng
    u64 D_off(unsigned i) const { return i < k ? (u64)i * (ng - 1) : (u64)k * (ng - 1) + (u64)(i - k) * ng; }
};

// slabs (cr n words) of one ciphertext of a chunk: the tensor 3k, C k, D (k + alpha) ng - k, T 2 (k + alpha), E 2k
u64 deep_slabs(unsigned k, unsigned alpha) { return (u64)(k + alpha) * fhe::host::deep_groups(k, alpha) + 7ull * k + 2ull * alpha; }
u64 slab_chunk(u64 n, u64 slabs, u64 batch) { return std::min<u64>(batch, std::max<u64>(1, (kChunkWords / n) / slabs)); }
u64 deep_chunk(u64 n, unsigned k, unsigned alpha, u64 batch) { return slab_chunk(n, deep_slabs(k, alpha), batch); }
u64 rescale_chunk(u64 n, unsigned k, u64 batch) { return std::min<u64>(batch, std::max<u64>(1, (kChunkWords / n) / (2ull * k))); }

// plans[0 .. limbs) and, where the entry point takes them, specials[0 .. alpha): FHE_E_NULL, then the counts, the ring, the
// repeated moduli, the 2^62 bound, the admission P >= Q_j
int check_deep(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, bool want_special, Deep *c, const char *who) {
    if (!plans) return fhe_fail(FHE_E_NULL, "%s: plans is NULL", who);
    if (limbs < 1 || limbs > fhe::kDeepMaxLimbs) return fhe_fail(FHE_E_INVALID, "%s: limbs=%u must be in [1, 32]", who, limbs);
    for (unsigned i = 0; i < limbs; i++)
        if (!plans[i]) return fhe_fail(FHE_E_NULL, "%s: plan %u is NULL", who, i);
    if (want_special) {
        if (!specials) return fhe_fail(FHE_E_NULL, "%s: specials is NULL", who);
        if (alpha < 1 || alpha > fhe::kDeepMaxSpecials) return fhe_fail(FHE_E_INVALID, "%s: alpha=%u must be in [1, 8]", who, alpha);
        for (unsigned m = 0; m < alpha; m++)
            if (!specials[m]) return fhe_fail(FHE_E_NULL, "%s: special plan %u is NULL", who, m);
    }
    c->k = limbs;
    c->alpha = want_special ? alpha : 1;
    c->ng = fhe::host::deep_groups(limbs, c->alpha);
    c->n = plans[0]->n;
    c->L = plans[0]->log_n;
    const unsigned all = limbs + (want_special ? alpha : 0u);
    for (unsigned i = 0; i < all; i++) c->p[i] = i < limbs ? plans[i] : specials[i - limbs];
    for (unsigned i = 1; i < all; i++)
        if (c->p[i]->n != c->n) return fhe_fail(FHE_E_PARAM_MISMATCH, "%s: plan %u has n=%llu, plan 0 n=%llu", who, i, (unsigned long long)c->p[i]->n, (unsigned long long)c->n);
    if (c->n < 2) return fhe_fail(FHE_E_BAD_N, "%s: n must be at least 2", who);
    for (unsigned i = 0; i < all; i++)
        for (unsigned j = 0; j < i; j++)
            if (c->p[i]->q == c->p[j]->q) return fhe_fail(FHE_E_INVALID, "%s: modulus %llu is repeated in the chain", who, (unsigned long long)c->p[i]->q);
    for (unsigned i = 0; i < all; i++)
        if (c->p[i]->q >= fhe::kExtModLimit) return fhe_fail(FHE_E_INVALID, "%s: modulus %llu is not below 2^62", who, (unsigned long long)c->p[i]->q);
    if (want_special) {
        u64 q[fhe::kDeepMaxTargets];
        for (unsigned i = 0; i < all; i++) q[i] = c->p[i]->q;
        if (!fhe::host::deep_admits(q, limbs, q + limbs, alpha))
            return fhe_fail(FHE_E_INVALID, "%s: the product of the special primes must not be below the product of a digit group", who);
    }
    return FHE_OK;
}

int check_key_limbs(const Deep &c, unsigned key_limbs, const char *who) {
    if (key_limbs < c.k || key_limbs > fhe::kDeepMaxLimbs)
        return fhe_fail(FHE_E_INVALID, "%s: key_limbs=%u must be at least limbs=%u and at most 32", who, key_limbs, c.k);
    return FHE_OK;
}
u64 key_words(unsigned key_limbs, unsigned alpha, u64 n) { return (u64)fhe::host::deep_groups(key_limbs, alpha) * (key_limbs + alpha) * 2 * n; }

int check_galois_element(uint64_t g, u64 n, int r, const char *who) {
    if ((g & 1) != 0 && g < 2 * n) return FHE_OK;
    char name[16] = "g";
    if (r >= 0) snprintf(name, sizeof name, "g[%d]", r);
    return fhe_fail(FHE_E_INVALID, "%s: %s=%llu must be odd and below 2n", who, name, (unsigned long long)g);
}

// One launch of the extension kernel: its sources by value and its targets' place in the table
struct ExtLaunch {
    fhe::DeepSrc src;
    unsigned first, targets;
};
// The tables of one chain on one device: they depend on the chain and not on the chunk, since a target's place is kept in
// slabs.  Built on the host and uploaded (blocking) on the chain's first call, then kept until fhe_ntt_shutdown().
// ext[j], j < ng: digit group j -> every limb outside it, in D; ext.back(): the modulus-down.
struct DeepTables {
    std::vector<fhe::DeepTarget> tab;
    std::vector<ExtLaunch> ext;
    fhe::DeepTarget *dev = nullptr;
    int add(const u64 *src, unsigned s, const u64 *dst, const u64 *off, unsigned t, const char *who) {
        ExtLaunch l{};
        l.first = (unsigned)tab.size();
        l.targets = t;
        tab.resize(tab.size() + t);
        if (!fhe::host::deep_ext_tables(src, s, dst, off, t, &l.src, tab.data() + l.first)) return fhe_fail(FHE_E_INVALID, "%s: the moduli are not pairwise coprime odd numbers", who);
        ext.push_back(l);
        return FHE_OK;
    }
    int upload() {
        if (tab.empty()) return FHE_OK;
        FheTableUpload up;
        dev = up.up(tab.data(), tab.size());
        if (!dev) return fhe_hip_fail(up.err, "the extension tables of the deep chain");
        up.owned.clear();                                            // kept: fhe_deep_free_all frees it
        return FHE_OK;
    }
};
std::mutex g_deep_lock;
std::map<std::vector<u64>, DeepTables> g_deep;   // key: device, kind (0 key switch, 1 rescale), limbs, alpha, the moduli

// the tables of c (a rescale: of its top limb's modulus-down) on the current device; *out stays valid until fhe_ntt_shutdown()
template <class Build>
int tables_get(const Deep &c, bool rescale, const DeepTables **out, Build build) {
    int dev, rc;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    const unsigned all = c.k + (rescale ? 0u : c.alpha);
    std::vector<u64> key{(u64)dev, rescale ? 1ull : 0ull, c.k, c.alpha};
    for (unsigned i = 0; i < all; i++) key.push_back(c.p[i]->q);
    std::lock_guard<std::mutex> lk(g_deep_lock);
    auto it = g_deep.find(key);
    if (it == g_deep.end()) {
        DeepTables t;
        if ((rc = build(&t)) != FHE_OK || (rc = t.upload()) != FHE_OK) return rc;
        it = g_deep.emplace(std::move(key), std::move(t)).first;
    }
    *out = &it->second;
    return FHE_OK;
}

int switch_tables(const Deep &c, DeepTables *t, const char *who) {
    u64 q[fhe::kDeepMaxTargets], dst[fhe::kDeepMaxTargets], off[fhe::kDeepMaxTargets];
    const unsigned all = c.k + c.alpha;
    for (unsigned i = 0; i < all; i++) q[i] = c.p[i]->q;
    int rc;
    for (unsigned j = 0; j < c.ng; j++) {
        unsigned cnt = 0;
        for (unsigned i = 0; i < all; i++) {
            const unsigned gi = c.group_of(i);
            if (gi == j) continue;
            dst[cnt] = q[i];
            off[cnt++] = c.D_off(i) + (j - (j > gi ? 1u : 0u));
        }
        if ((rc = t->add(q + j * c.alpha, std::min(c.alpha, c.k - j * c.alpha), dst, off, cnt, who)) != FHE_OK) return rc;
    }
    for (unsigned i = 0; i < c.k; i++) off[i] = 2ull * i;
    return t->add(q + c.k, c.alpha, q, off, c.k, who);
}

int extend_launch(const Deep &c, const DeepTables &t, unsigned which, const u64 *src, u64 src_ls, u64 *dst, u64 unit, u64 count, hipStream_t st) {
    const ExtLaunch &l = t.ext[which];
    if (l.targets == 0) return FHE_OK;
    return launch("ckks_deep_extend", (int)c.L, st, fhe::ckks_deep_extend_kernel, fhe_ew_grid(count), 256, src, src_ls, dst, unit, count, l.src, t.dev + l.first, l.targets);
}

// The workspace of one key switch over cr ciphertexts (slab = cr n words): Dt the chunk's tensor, C the k
// limbs in coefficients, D the lifted digits as evals by target, T the k + alpha key sums of two components, E the lifted t_P
struct DeepBufs {
    u64 *Dt, *C, *D, *T, *E;
    u64 slab;
    DeepBufs(u64 *W, const Deep &c, u64 slab_)
        : Dt(W), C(Dt + 3ull * c.k * slab_), D(C + (u64)c.k * slab_), T(D + ((u64)(c.k + c.alpha) * c.ng - c.k) * slab_), E(T + 2ull * (c.k + c.alpha) * slab_), slab(slab_) {}
    DeepBufs(u64 *C_, u64 *D_, u64 *T_, u64 *E_, u64 slab_) : Dt(nullptr), C(C_), D(D_), T(T_), E(E_), slab(slab_) {}   // a diagonal sum: no tensor, T one of its sets
};

// `polys` rows of evals, which the ABI aligns to 8 bytes, as coefficients in the workspace rows dst
int inverse_into(const fhe_ntt_plan *p, const u64 *src, u64 *dst, u64 polys, hipStream_t st) {
    const int rc = aligned_rows(src, dst, polys * p->n, st, &src);
    return rc != FHE_OK ? rc : fhe_ntt_inverse_dev(p, src, dst, polys, st);
}

// step 1: limb i = src(i) (cr rows of evals modulo q_i) in coefficients; each group extended to every limb outside it; forward
template <class Src>
int digit_rows(const Deep &c, const DeepTables &t, Src src, const DeepBufs &b, u64 cr, hipStream_t st) {
    int rc;
    for (unsigned i = 0; i < c.k; i++)
        if ((rc = inverse_into(c.p[i], src(i), b.C + i * b.slab, cr, st)) != FHE_OK) return rc;
    for (unsigned j = 0; j < c.ng; j++)
        if ((rc = extend_launch(c, t, j, b.C + (u64)j * c.alpha * b.slab, b.slab, b.D, b.slab, b.slab, st)) != FHE_OK) return rc;
    for (unsigned i = 0; i < c.k + c.alpha; i++) {
        const u64 polys = (u64)(i < c.k ? c.ng - 1 : c.ng) * cr;
        u64 *rows = b.D + c.D_off(i) * b.slab;
        if (polys && (rc = fhe_ntt_forward_dev(c.p[i], rows, rows, polys, st)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

// step 2: T_i = sum_j D_ji (.) key[j][col(i)] for every i of {0 .. k - 1, p_0 ..}; own(i) is limb i's own evals.  g != 0: a Galois
// key switch, the digits read at pi_g
template <class Own>
int keymac_rows(const Deep &c, const u64 *key, unsigned key_limbs, Own own, const DeepBufs &b, u32 g, hipStream_t st) {
    const u64 n = c.n, key_stride = (u64)(key_limbs + c.alpha) * 2 * n;
    for (unsigned i = 0; i < c.k + c.alpha; i++) {
        const u64 *col = key + (u64)(i < c.k ? i : key_limbs + (i - c.k)) * 2 * n;
        const int rc = launch(g ? "ckks_deep_keymac_galois" : "ckks_deep_keymac", (int)c.L, st, g ? fhe::ckks_deep_keymac_kernel<true> : fhe::ckks_deep_keymac_kernel<false>,
                              fhe_ew_grid(b.slab), 256, (const u64 *)b.D + c.D_off(i) * b.slab, b.slab, i < c.k ? own(i) : nullptr, c.group_of(i), col, key_stride,
                              b.T + 2ull * i * b.slab, c.ng, c.L, b.slab, g, c.p[i]->mod);
        if (rc != FHE_OK) return rc;
    }
    return FHE_OK;
}

// the rows of limb i of a ciphertext-shaped operand: limbs ls words apart, the two components cs words apart; p NULL for none
template <class T>
struct LimbRows {
    T *p;
    u64 ls, cs;
    T *of(unsigned i) const { return p ? p + (u64)i * ls : nullptr; }
};

// The tail of a modulus-down: X the dropped residues in coefficients (sources src_ls apart, two components of `slab` words
// each, contiguous), extended by launch `which` to the `keep` remaining limbs in E (2 slabs each) and transformed;
// out_i = (x_i - E_i) inv[i] (+ add_i) mod q_i.  g != 0: the addend is pi_g of add's first component, for the first only.
int moddown_rows(const Deep &c, const DeepTables &t, unsigned which, unsigned keep, const u64 *X, u64 src_ls, u64 *E, u64 slab, LimbRows<const u64> x,
                 LimbRows<const u64> add, LimbRows<u64> out, const u64 *inv, u32 g, hipStream_t st) {
    int rc;
    if ((rc = extend_launch(c, t, which, X, src_ls, E, slab, 2 * slab, st)) != FHE_OK) return rc;
    for (unsigned i = 0; i < keep; i++)
        if ((rc = fhe_ntt_forward_dev(c.p[i], E + 2ull * i * slab, E + 2ull * i * slab, 2 * (slab >> c.L), st)) != FHE_OK) return rc;
    for (unsigned i = 0; i < keep; i++)
        if ((rc = fhe_rns_divround_limb(c.p[i], x.of(i), x.cs, E + 2ull * i * slab, slab, add.of(i), add.cs, out.of(i), out.cs, slab, inv[i], g, st)) != FHE_OK) return rc;
    return FHE_OK;
}

// step 3: t modulo the special primes in coefficients, in place, and the modulus-down by P of the k limbs
int special_down(const Deep &c, const DeepTables &t, const DeepBufs &b, LimbRows<const u64> add, LimbRows<u64> out, const u64 *pinv, u32 g, hipStream_t st) {
    u64 *TP = b.T + 2ull * c.k * b.slab;
    for (unsigned m = 0; m < c.alpha; m++) {
        const int rc = fhe_ntt_inverse_dev(c.p[c.k + m], TP + 2ull * m * b.slab, TP + 2ull * m * b.slab, 2 * (b.slab >> c.L), st);
        if (rc != FHE_OK) return rc;
    }
    return moddown_rows(c, t, c.ng, c.k, TP, 2 * b.slab, b.E, b.slab, {b.T, 2 * b.slab, b.slab}, add, out, pinv, g, st);
}

// rows d_r0 .. d_r0 + cr of d [k][3][d_rows][n] -> rows o_r0 .. of out [k][2][o_rows][n]
int relin_rows(const Deep &c, const DeepTables &t, const u64 *rlk, unsigned key_limbs, const u64 *pinv, const u64 *d, u64 d_rows, u64 d_r0, u64 *out, u64 o_rows, u64 o_r0,
               const DeepBufs &b, u64 cr, hipStream_t st) {
    const u64 n = c.n;
    auto d2 = [&](unsigned limb) { return d + (((u64)limb * 3 + 2) * d_rows + d_r0) * n; };
    int rc;
    if ((rc = digit_rows(c, t, d2, b, cr, st)) != FHE_OK) return rc;
    if ((rc = keymac_rows(c, rlk, key_limbs, d2, b, 0u, st)) != FHE_OK) return rc;
    return special_down(c, t, b, {d + d_r0 * n, 3 * d_rows * n, d_rows * n}, {out + o_r0 * n, 2 * o_rows * n, o_rows * n}, pinv, 0u, st);
}

// The frame of a key-switch call: the chain's tables, the workspace of `slabs` slabs a ciphertext, the inverses of P, and
// body(r0, cr, tables, W, pinv) over the batch in chunks
template <class Body>
int switch_call(const Deep &c, u64 batch, u64 slabs, hipStream_t st, const char *who, Body body) {
    const DeepTables *t = nullptr;
    int rc = tables_get(c, false, &t, [&](DeepTables *b) { return switch_tables(c, b, who); });
    if (rc != FHE_OK) return rc;
    const u64 cb = slab_chunk(c.n, slabs, batch);
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kCkksDeepSlot, (size_t)(slabs * cb * c.n * 8), st, &w)) != FHE_OK) return rc;
    u64 pinv[fhe::kDeepMaxLimbs];
    for (unsigned i = 0; i < c.k; i++) {
        const u64 q = c.p[i]->q;
        u64 pm = 1;
        for (unsigned m = 0; m < c.alpha; m++) pm = fhe::host::mulmod(pm, c.p[c.k + m]->q % q, q);
        pinv[i] = fhe::host::inv_mod(q, pm);
    }
    for (u64 r0 = 0; r0 < batch; r0 += cb) {
        const u64 cr = std::min<u64>(cb, batch - r0);
        if ((rc = body(r0, cr, *t, (u64 *)w, pinv)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

// a switching key [dnum][limbs + alpha][2][n]: the public key of row first_row + j under every prime plus, in the columns of
// group j, the diagonal term (P mod q_i) x, x = s^2 for the relinearisation key and sigma_g(s) for a Galois key
int switch_key(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, const uint8_t *seed, uint64_t first_row, uint64_t g,
               bool galois, const void *d_s, const void *d_cdt, unsigned m, void *d_key, void *hip_stream, const char *who) {
    Deep c;
    int rc = check_deep(plans, limbs, specials, alpha, true, &c, who);
    if (rc != FHE_OK) return rc;
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    const u64 n = c.n;
    const unsigned k = c.k, cols = k + alpha;
    if (galois && (rc = check_galois_element(g, n, -1, who)) != FHE_OK) return rc;
    u64 qmin = c.p[0]->q;
    for (unsigned i = 1; i < k; i++) qmin = std::min<u64>(qmin, c.p[i]->q);
    if ((rc = check_cdt_shape(d_cdt, m, qmin, who)) != FHE_OK) return rc;
    if (first_row >= kRowLimit - c.ng) return fhe_fail(FHE_E_INVALID, "%s: first_row + dnum passes 2^63", who);
    if (!d_s || !d_key) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_s) || misaligned8(d_key)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_key, key_words(k, alpha, n) * 8, {{d_s, (u64)cols * n * 8}, {d_cdt, (u64)m * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: the key overlaps the secret or the error table", who);
    hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = check_cdt_words(d_cdt, m, st, who)) != FHE_OK) return rc;
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kCkksDeepSlot, (size_t)(4 * n * 8), st, &w)) != FHE_OK) return rc;
    u64 *PK = (u64 *)w, *S = PK + 2 * n, *SE = S + n;            // one key row, the limb's secret (16-byte aligned) and its evals
    for (unsigned j = 0; j < c.ng; j++) {
        for (unsigned i = 0; i < cols; i++) {
            const fhe_ntt_plan *p = c.p[i];
            HIP_TRY(hipMemcpyAsync(S, (const u64 *)d_s + (u64)i * n, n * 8, hipMemcpyDeviceToDevice, st));
            if ((rc = fhe_ckks_public_key_dev(p, seed, first_row + j, S, d_cdt, m, PK, st)) != FHE_OK) return rc;
            if ((rc = fhe_ntt_forward_dev(p, PK, PK, 2, st)) != FHE_OK) return rc;
            if (c.group_of(i) == j) {
                u64 pm = 1;
                for (unsigned s = 0; s < alpha; s++) pm = fhe::host::mulmod(pm, c.p[k + s]->q % p->q, p->q);
                if ((rc = fhe_ntt_forward_dev(p, S, SE, 1, st)) != FHE_OK) return rc;
                if ((rc = fhe_rns_keyterm_limb(p, PK, SE, pm, (u32)g, galois, st)) != FHE_OK) return rc;
            }
            HIP_TRY(hipMemcpyAsync((u64 *)d_key + ((u64)j * cols + i) * 2 * n, PK, 2 * n * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    return FHE_OK;
}

// the checks every key-switching entry point shares behind its chain: the batch, the ring's word limit
bool shape_of(uint64_t n, unsigned limbs, unsigned alpha, size_t batch) {
    return n >= 2 && (n & (n - 1)) == 0 && n <= (1ull << 19) && limbs >= 1 && limbs <= fhe::kDeepMaxLimbs && alpha >= 1 && alpha <= fhe::kDeepMaxSpecials && batch != 0;
}

}  // namespace

void fhe_deep_free_all() {
    std::lock_guard<std::mutex> lk(g_deep_lock);
    for (auto &kv : g_deep)
        if (kv.second.dev) (void)hipFree(kv.second.dev);
    g_deep.clear();
}

extern "C" size_t fhe_ckks_deep_workspace_bytes(uint64_t n, unsigned limbs, unsigned alpha, size_t batch) {
    if (!shape_of(n, limbs, alpha, batch)) return 0;
    return (size_t)(std::max<u64>(deep_slabs(limbs, alpha) * n * deep_chunk(n, limbs, alpha, batch), 2ull * limbs * n * rescale_chunk(n, limbs, batch)) * 8);
}

extern "C" int fhe_ckks_deep_relin_key_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, const uint8_t *seed,
                                           uint64_t first_row, const void *d_s, const void *d_cdt, unsigned m, void *d_key, void *hip_stream) {
    return switch_key(plans, limbs, specials, alpha, seed, first_row, 0, false, d_s, d_cdt, m, d_key, hip_stream, "fhe_ckks_deep_relin_key_dev");
}

extern "C" int fhe_ckks_deep_galois_key_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, const uint8_t *seed,
                                            uint64_t first_row, uint64_t g, const void *d_s, const void *d_cdt, unsigned m, void *d_key, void *hip_stream) {
    return switch_key(plans, limbs, specials, alpha, seed, first_row, g, true, d_s, d_cdt, m, d_key, hip_stream, "fhe_ckks_deep_galois_key_dev");
}

extern "C" int fhe_ckks_deep_relinearize_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, const void *d_key,
                                             unsigned key_limbs, const void *d_d, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_deep_relinearize_dev";
    Deep c;
    int rc = check_deep(plans, limbs, specials, alpha, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 3ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_key || !d_d || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_key) || misaligned8(d_d) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_out, 2ull * c.k * batch * n * 8, {{d_d, 3ull * c.k * batch * n * 8}, {d_key, key_words(key_limbs, alpha, n) * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the tensor or the key", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return switch_call(c, batch, deep_slabs(c.k, c.alpha), st, who, [&](u64 r0, u64 cr, const DeepTables &t, u64 *W, const u64 *pinv) {
        return relin_rows(c, t, (const u64 *)d_key, key_limbs, pinv, (const u64 *)d_d, batch, r0, (u64 *)d_out, batch, r0, DeepBufs(W, c, cr * n), cr, st);
    });
}

extern "C" int fhe_ckks_deep_mul_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, const void *d_key,
                                     unsigned key_limbs, const void *d_a, const void *d_b, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_deep_mul_dev";
    Deep c;
    int rc = check_deep(plans, limbs, specials, alpha, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 3ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_key || !d_a || !d_b || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_key) || misaligned8(d_a) || misaligned8(d_b) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8;
    if (overlaps_any(d_out, ct_bytes, {{d_a, ct_bytes}, {d_b, ct_bytes}, {d_key, key_words(key_limbs, alpha, n) * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an operand or the key", who);
    hipStream_t st = (hipStream_t)hip_stream;
    const u64 *a = (const u64 *)d_a, *bb = (const u64 *)d_b;
    return switch_call(c, batch, deep_slabs(c.k, c.alpha), st, who, [&](u64 r0, u64 cr, const DeepTables &t, u64 *W, const u64 *pinv) {
        const u64 slab = cr * n;
        const DeepBufs b(W, c, slab);
        for (unsigned i = 0; i < c.k; i++) {
            const int rc = fhe_rns_tensor_limb(c.p[i], a + ((u64)i * 2 * batch + r0) * n, batch * n, bb + ((u64)i * 2 * batch + r0) * n, batch * n, b.Dt + (u64)i * 3 * slab,
                                               slab, slab, st);
            if (rc != FHE_OK) return rc;
        }
        return relin_rows(c, t, (const u64 *)d_key, key_limbs, pinv, b.Dt, cr, 0, (u64 *)d_out, batch, r0, b, cr, st);
    });
}

extern "C" int fhe_ckks_deep_galois_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, const void *const *d_gks,
                                        const uint64_t *gs, unsigned count, unsigned key_limbs, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_deep_galois_dev";
    Deep c;
    int rc = check_deep(plans, limbs, specials, alpha, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (count > FHE_CKKS_GALOIS_MAX_COUNT) return fhe_fail(FHE_E_INVALID, "%s: count=%u passes %d", who, count, FHE_CKKS_GALOIS_MAX_COUNT);
    if (batch == 0 || count == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 2ull * c.k * n * count, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_gks || !gs || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8, gk_bytes = key_words(key_limbs, alpha, n) * 8;
    for (unsigned r = 0; r < count; r++) {
        if (!d_gks[r]) return fhe_fail(FHE_E_NULL, "%s: key %u is NULL", who, r);
        if (misaligned8(d_gks[r])) return fhe_fail(FHE_E_INVALID, "%s: key %u must be 8-byte aligned", who, r);
        if ((rc = check_galois_element(gs[r], n, (int)r, who)) != FHE_OK) return rc;
        if (overlaps_any(d_out, ct_bytes * count, {{d_gks[r], gk_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps key %u", who, r);
    }
    if (overlaps_any(d_out, ct_bytes * count, {{d_in, ct_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the ciphertexts", who);
    hipStream_t st = (hipStream_t)hip_stream;
    // the digits are those of the unpermuted c1, made once a chunk; every g then takes its key sums with the digits read at pi_g,
    // the divide-and-round by P, and pi_g(c0) gathered in that last kernel (§23)
    return switch_call(c, batch, deep_slabs(c.k, c.alpha), st, who, [&](u64 r0, u64 cr, const DeepTables &t, u64 *W, const u64 *pinv) {
        const DeepBufs b(W, c, cr * n);
        const LimbRows<const u64> ct{(const u64 *)d_in + r0 * n, 2 * batch * n, batch * n};
        auto c1 = [&](unsigned limb) { return ct.of(limb) + ct.cs; };
        int rc;
        if ((rc = digit_rows(c, t, c1, b, cr, st)) != FHE_OK) return rc;
        for (unsigned r = 0; r < count; r++) {
            const u32 g = (u32)gs[r];
            if ((rc = keymac_rows(c, (const u64 *)d_gks[r], key_limbs, c1, b, g, st)) != FHE_OK) return rc;
            if ((rc = special_down(c, t, b, ct, {(u64 *)d_out + r * 2ull * c.k * batch * n + r0 * n, ct.ls, ct.cs}, pinv, g, st)) != FHE_OK) return rc;
        }
        return FHE_OK;
    });
}

// ---- plaintext linear transforms: the double-hoisted diagonal sum ---------------------------------------------------
namespace {

// slabs of one ciphertext of a chunk of a diagonal sum: C k, D (k + alpha) ng - k, min(outputs, kDeepDiagOutputs) sets U of
// 2 (k + alpha), E 2k
u64 diag_slabs(unsigned k, unsigned alpha, unsigned outputs) {
    return (u64)(k + alpha) * fhe::host::deep_groups(k, alpha) + 2ull * (k + alpha) * std::min<unsigned>(outputs, fhe::kDeepDiagOutputs) + 2ull * k;
}

template <class... A>
int deep_diagmac_launch(unsigned nout, bool carry, int L, hipStream_t st, unsigned grid, A... a) {
    const char *lab = "ckks_deep_diagmac";
#define FHE_DEEP_DIAG_CASE(N) \
    case N: return carry ? launch(lab, L, st, fhe::ckks_deep_diagmac_kernel<N, true>, grid, 256, a...) : launch(lab, L, st, fhe::ckks_deep_diagmac_kernel<N, false>, grid, 256, a...)
    switch (nout) {
        FHE_DEEP_DIAG_CASE(1);
        FHE_DEEP_DIAG_CASE(2);
    }
#undef FHE_DEEP_DIAG_CASE
    static_assert(fhe::kDeepDiagOutputs == 2, "one case per accumulator count");
    return fhe_fail(FHE_E_INVALID, "ckks_deep_diagmac: %u outputs in one launch", nout);
}

// The diagmac launches of outputs o0 .. o0 + nout of a diagonal sum over `slab` words a component of `ct`, in groups of
// kDeepDiagGroup elements.  U != NULL: the sums of §37 in the basis Q P, over the k + alpha targets, into the sets 0 .. nout - 1 at
// U (D the lifted digits).  Otherwise (no element but 1) the finished sums over the k chain limbs, into the rows out0 of output
// o0, the outputs o_words apart.
int deep_diagmac_rows(const Deep &c, const u64 *const *gks, const uint64_t *gs, unsigned count, unsigned key_limbs, const u64 *pts, unsigned o0, unsigned nout,
                      const u64 *D, u64 *U, u64 slab, LimbRows<const u64> ct, LimbRows<u64> out0, u64 o_words, hipStream_t st) {
    const unsigned k = c.k, all = k + c.alpha;
    const u64 n = c.n, pt_os = (u64)count * all * n, set = 2ull * all * slab;
    for (unsigned i = 0; i < (U ? all : k); i++) {
        u64 pmod = 1;
        if (U && i < k)
            for (unsigned m = 0; m < c.alpha; m++) pmod = fhe::host::mulmod(pmod, c.p[k + m]->q % c.p[i]->q, c.p[i]->q);
        for (unsigned e0 = 0; e0 < count; e0 += fhe::kDeepDiagGroup) {
            fhe::DeepDiagGroup grp{};
            grp.count = std::min<unsigned>(fhe::kDeepDiagGroup, count - e0);
            for (unsigned r = 0; r < grp.count; r++) {
                grp.g[r] = (u32)gs[e0 + r];
                grp.key[r] = grp.g[r] == 1 ? nullptr : gks[e0 + r] + (u64)(i < k ? i : key_limbs + (i - k)) * 2 * n;
                grp.pt[r] = pts + (((u64)o0 * count + e0 + r) * all + i) * n;
            }
            const int rc = deep_diagmac_launch(nout, e0 > 0, (int)c.L, st, fhe_ew_grid(slab), U ? D + c.D_off(i) * slab : nullptr, slab, i < k ? ct.of(i) : nullptr, ct.cs,
                                               c.group_of(i), (u64)(key_limbs + c.alpha) * 2 * n, pt_os, U ? U + 2ull * i * slab : out0.of(i), U ? slab : out0.cs,
                                               U ? set : o_words, c.ng, c.L, slab, i < k ? pmod : 0ull, grp, c.p[i]->mod);
            if (rc != FHE_OK) return rc;
        }
    }
    return FHE_OK;
}

}  // namespace

extern "C" size_t fhe_ckks_deep_diag_workspace_bytes(uint64_t n, unsigned limbs, unsigned alpha, size_t batch, unsigned count, unsigned outputs) {
    if (!shape_of(n, limbs, alpha, batch) || count == 0 || count > FHE_CKKS_GALOIS_MAX_COUNT || outputs == 0 || outputs > FHE_CKKS_DIAG_MAX_OUTPUTS) return 0;
    const u64 slabs = diag_slabs(limbs, alpha, outputs);
    return (size_t)(slabs * n * slab_chunk(n, slabs, batch) * 8);
}

extern "C" int fhe_ckks_deep_diag_sum_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, const void *const *d_gks,
                                          const uint64_t *gs, unsigned count, unsigned key_limbs, const void *d_pts, unsigned outputs, const void *d_in, void *d_out,
                                          size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_deep_diag_sum_dev";
    Deep c;
    int rc = check_deep(plans, limbs, specials, alpha, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (count > FHE_CKKS_GALOIS_MAX_COUNT) return fhe_fail(FHE_E_INVALID, "%s: count=%u passes %d", who, count, FHE_CKKS_GALOIS_MAX_COUNT);
    if (outputs < 1 || outputs > FHE_CKKS_DIAG_MAX_OUTPUTS) return fhe_fail(FHE_E_INVALID, "%s: outputs=%u must be in [1, %d]", who, outputs, FHE_CKKS_DIAG_MAX_OUTPUTS);
    if (batch == 0 || count == 0) return FHE_OK;
    const u64 n = c.n;
    const unsigned k = c.k;
    if (!mul_fits((u64)batch, 2ull * k * n * outputs, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!gs || !d_pts || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_pts) || misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * k * batch * n * 8, out_bytes = ct_bytes * outputs, gk_bytes = key_words(key_limbs, alpha, n) * 8;
    bool switched = false;
    for (unsigned r = 0; r < count; r++) {                           // g = 1 takes no key: the element is looked at before its key
        if ((rc = check_galois_element(gs[r], n, (int)r, who)) != FHE_OK) return rc;
        if (gs[r] == 1) continue;
        switched = true;
        if (!d_gks || !d_gks[r]) return fhe_fail(FHE_E_NULL, "%s: key %u is NULL", who, r);
        if (misaligned8(d_gks[r])) return fhe_fail(FHE_E_INVALID, "%s: key %u must be 8-byte aligned", who, r);
        if (overlaps_any(d_out, out_bytes, {{d_gks[r], gk_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps key %u", who, r);
    }
    if (overlaps_any(d_out, out_bytes, {{d_in, ct_bytes}, {d_pts, (u64)outputs * count * (k + alpha) * n * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the ciphertexts or the plaintexts", who);
    hipStream_t st = (hipStream_t)hip_stream;
    const u64 *const *gks = (const u64 *const *)d_gks;
    const u64 *pts = (const u64 *)d_pts;
    const u64 o_words = 2ull * k * batch * n;
    if (!switched) {
        // no element but the identity: the sums are finished modulo the chain primes, element-wise over the whole batch; no
        // digit, no transform, no modulus-down and no workspace
        int dev;                                                     // not used: the call is here to refuse, as the workspace would, where there is no device
        if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
        for (unsigned o0 = 0; o0 < outputs; o0 += fhe::kDeepDiagOutputs) {
            const unsigned nout = std::min<unsigned>(fhe::kDeepDiagOutputs, outputs - o0);
            if ((rc = deep_diagmac_rows(c, gks, gs, count, key_limbs, pts, o0, nout, nullptr, nullptr, batch * n, {(const u64 *)d_in, 2 * batch * n, batch * n},
                                        {(u64 *)d_out + o0 * o_words, 2 * batch * n, batch * n}, o_words, st)) != FHE_OK)
                return rc;
        }
        return FHE_OK;
    }
    // the digits are those of the unpermuted c1, made once a chunk; per launch of up to kDeepDiagOutputs outputs, U over the
    // k + alpha targets; per output one modulus-down of its U, with no addend: it rode through as (P mod q_i) ct
    const unsigned sets = std::min<unsigned>(outputs, fhe::kDeepDiagOutputs);
    return switch_call(c, batch, diag_slabs(k, alpha, outputs), st, who, [&](u64 r0, u64 cr, const DeepTables &t, u64 *W, const u64 *pinv) {
        const u64 slab = cr * n, set = 2ull * (k + alpha) * slab;
        u64 *C = W, *D = C + (u64)k * slab, *U = D + ((u64)(k + alpha) * c.ng - k) * slab, *E = U + sets * set;
        const LimbRows<const u64> ct{(const u64 *)d_in + r0 * n, 2 * batch * n, batch * n};
        auto c1 = [&](unsigned limb) { return ct.of(limb) + ct.cs; };
        int rc;
        if ((rc = digit_rows(c, t, c1, DeepBufs(C, D, U, E, slab), cr, st)) != FHE_OK) return rc;
        for (unsigned o0 = 0; o0 < outputs; o0 += fhe::kDeepDiagOutputs) {
            const unsigned nout = std::min<unsigned>(fhe::kDeepDiagOutputs, outputs - o0);
            if ((rc = deep_diagmac_rows(c, gks, gs, count, key_limbs, pts, o0, nout, D, U, slab, ct, {}, 0, st)) != FHE_OK) return rc;
            for (unsigned o = 0; o < nout; o++)
                if ((rc = special_down(c, t, DeepBufs(C, D, U + o * set, E, slab), {}, {(u64 *)d_out + (o0 + o) * o_words + r0 * n, ct.ls, ct.cs}, pinv, 0u, st)) != FHE_OK)
                    return rc;
        }
        return FHE_OK;
    });
}

extern "C" int fhe_ckks_deep_rescale_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_deep_rescale_dev";
    Deep c;
    int rc = check_deep(plans, limbs, nullptr, 0, false, &c, who);
    if (rc != FHE_OK) return rc;
    if (limbs < 2) return fhe_fail(FHE_E_INVALID, "%s: a ciphertext of one limb cannot be rescaled", who);
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    const unsigned k = c.k, top = k - 1;
    if (!mul_fits((u64)batch, 2ull * k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_out, 2ull * top * batch * n * 8, {{d_in, 2ull * k * batch * n * 8}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the ciphertexts", who);
    hipStream_t st = (hipStream_t)hip_stream;
    u64 q[fhe::kDeepMaxLimbs], off[fhe::kDeepMaxLimbs], qinv[fhe::kDeepMaxLimbs];
    for (unsigned i = 0; i < k; i++) {
        q[i] = c.p[i]->q;
        off[i] = 2ull * i;
    }
    const DeepTables *t = nullptr;
    if ((rc = tables_get(c, true, &t, [&](DeepTables *b) { return b->add(q + top, 1, q, off, top, who); })) != FHE_OK) return rc;
    for (unsigned i = 0; i < top; i++) qinv[i] = fhe::host::inv_mod(q[i], q[top] % q[i]);
    const u64 cb = rescale_chunk(n, k, batch);
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kCkksDeepSlot, (size_t)(2ull * k * cb * n * 8), st, &w)) != FHE_OK) return rc;
    const LimbRows<const u64> in{(const u64 *)d_in, 2 * batch * n, batch * n};
    for (u64 r0 = 0; r0 < batch; r0 += cb) {
        const u64 cr = std::min<u64>(cb, batch - r0), slab = cr * n;
        u64 *C = (u64 *)w, *E = C + 2 * slab;
        const u64 *t0 = in.of(top) + r0 * n;                         // the top limb's two components, batch n apart
        if ((rc = inverse_into(c.p[top], t0, C, cr, st)) != FHE_OK) return rc;
        if ((rc = inverse_into(c.p[top], t0 + in.cs, C + slab, cr, st)) != FHE_OK) return rc;
        if ((rc = moddown_rows(c, *t, 0, top, C, 0, E, slab, {in.p + r0 * n, in.ls, in.cs}, {}, {(u64 *)d_out + r0 * n, 2 * batch * n, batch * n}, qinv, 0u, st)) != FHE_OK)
            return rc;
    }
    return FHE_OK;
}

// ---- polynomial evaluation: scalar sums and inner products ---------------------------------------------------------
namespace {

template <class... A>
int deep_lincomb_launch(unsigned nout, bool carry, int L, hipStream_t st, dim3 grid, const A &...a) {
    const char *lab = "ckks_deep_lincomb";
    hipError_t e = hipErrorInvalidValue;
#define FHE_DEEP_LIN_CASE(N) \
    case N: e = carry ? fhe::launch_grid(fhe::ckks_deep_lincomb_kernel<N, true>, lab, L, grid, 256, 0, st, a...) : fhe::launch_grid(fhe::ckks_deep_lincomb_kernel<N, false>, lab, L, grid, 256, 0, st, a...); break
    switch (nout) {
        FHE_DEEP_LIN_CASE(1);
        FHE_DEEP_LIN_CASE(2);
        FHE_DEEP_LIN_CASE(3);
        FHE_DEEP_LIN_CASE(4);
        default: return fhe_fail(FHE_E_INVALID, "ckks_deep_lincomb: %u outputs in one launch", nout);
    }
#undef FHE_DEEP_LIN_CASE
    static_assert(fhe::kDeepLinOutputs == 4, "one case per accumulator count");
    return e == hipSuccess ? FHE_OK : fhe_hip_fail(e, "ckks_deep_lincomb_kernel");
}

// rows r0 .. r0 + cr of the `count` pairs -> their summed tensor in Dt [k][3][cr][n]: per slice of limbs, groups of kDeepDotPairs
// pairs, every group after the first carried; w [count][k] or NULL (every weight 1)
int deep_tensorsum_rows(const Deep &c, const void *const *d_as, const void *const *d_bs, unsigned count, const uint64_t *w, u64 batch, u64 r0, u64 *Dt, u64 cr,
                        hipStream_t st) {
    const u64 n = c.n, slab = cr * n;
    return fhe::host::deep_tensorsum_each(c.k, count, [&](unsigned i0, unsigned nl, unsigned p0, unsigned np) {
        fhe::DeepDotArgs a{};
        for (unsigned l = 0; l < nl; l++) a.m[l] = c.p[i0 + l]->mod;
        fhe::host::deep_tensorsum_words((const u64 *)w, c.k, i0, nl, p0, np, &a.s);
        for (unsigned r = 0; r < np; r++) {
            a.a[r] = (const u64 *)d_as[p0 + r] + ((u64)i0 * 2 * batch + r0) * n;
            a.b[r] = (const u64 *)d_bs[p0 + r] + ((u64)i0 * 2 * batch + r0) * n;
        }
        a.count = np;
        const bool carry = p0 > 0;
        auto kernel = w ? (carry ? fhe::ckks_deep_tensorsum_kernel<true, true> : fhe::ckks_deep_tensorsum_kernel<true, false>)
                        : (carry ? fhe::ckks_deep_tensorsum_kernel<false, true> : fhe::ckks_deep_tensorsum_kernel<false, false>);
        const hipError_t e = fhe::launch_grid(kernel, "ckks_deep_tensorsum", (int)c.L, dim3(fhe_ew_grid(slab), nl), 256, 0, st, Dt + (u64)i0 * 3 * slab, slab, 2 * batch * n,
                                              batch * n, a);
        return e == hipSuccess ? (int)FHE_OK : fhe_hip_fail(e, "ckks_deep_tensorsum_kernel");
    });
}

}  // namespace

extern "C" int fhe_ckks_deep_lincomb_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *const *d_cts, unsigned count, const uint64_t *w,
                                         const uint64_t *k, unsigned outputs, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_deep_lincomb_dev";
    Deep c;
    int rc = check_deep(plans, limbs, nullptr, 0, false, &c, who);
    if (rc != FHE_OK) return rc;
    if (count < 1 || count > FHE_CKKS_LINCOMB_MAX_COUNT) return fhe_fail(FHE_E_INVALID, "%s: count=%u must be in [1, %d]", who, count, FHE_CKKS_LINCOMB_MAX_COUNT);
    if (outputs < 1 || outputs > FHE_CKKS_LINCOMB_MAX_OUTPUTS)
        return fhe_fail(FHE_E_INVALID, "%s: outputs=%u must be in [1, %d]", who, outputs, FHE_CKKS_LINCOMB_MAX_OUTPUTS);
    if (!d_cts || !w) return fhe_fail(FHE_E_NULL, "%s: NULL host array", who);
    for (unsigned o = 0; o < outputs; o++)
        for (unsigned i = 0; i < c.k; i++) {
            for (unsigned r = 0; r < count; r++)
                if (w[((u64)o * count + r) * c.k + i] >= c.p[i]->q) return fhe_fail(FHE_E_INVALID, "%s: weight [%u][%u][%u] is not below its modulus", who, o, r, i);
            if (k && k[(u64)o * c.k + i] >= c.p[i]->q) return fhe_fail(FHE_E_INVALID, "%s: constant [%u][%u] is not below its modulus", who, o, i);
        }
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 2ull * c.k * n * outputs, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 limb_words = 2ull * batch * n, ct_bytes = c.k * limb_words * 8;
    for (unsigned r = 0; r < count; r++) {
        if (!d_cts[r]) return fhe_fail(FHE_E_NULL, "%s: input %u is NULL", who, r);
        if (misaligned8(d_cts[r])) return fhe_fail(FHE_E_INVALID, "%s: input %u must be 8-byte aligned", who, r);
        if (overlaps_any(d_out, ct_bytes * outputs, {{d_cts[r], ct_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps input %u", who, r);
    }
    int dev;                                                         // not used: the call is here to refuse, as a workspace would, where there is no device
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    // no workspace and no chunk: the sum is element-wise over the whole batch
    return fhe::host::deep_lincomb_each(c.k, outputs, count, [&](unsigned o0, unsigned no, unsigned i0, unsigned nl, unsigned r0, unsigned nr) {
        fhe::DeepLinArgs a{};
        for (unsigned l = 0; l < nl; l++) a.m[l] = c.p[i0 + l]->mod;
        fhe::host::deep_lincomb_words((const u64 *)w, (const u64 *)k, c.k, count, o0, no, i0, nl, r0, nr, &a.s);
        for (unsigned r = 0; r < nr; r++) a.ct[r] = (const u64 *)d_cts[r0 + r] + (u64)i0 * limb_words;
        a.count = nr;
        return deep_lincomb_launch(no, r0 > 0, (int)c.L, st, dim3(fhe_ew_grid(limb_words), nl), (u64 *)d_out + ((u64)o0 * c.k + i0) * limb_words, c.k * limb_words,
                                   limb_words, limb_words / 2, a);
    });
}

extern "C" int fhe_ckks_deep_dot_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *const *specials, unsigned alpha, const void *d_key,
                                     unsigned key_limbs, const void *const *d_as, const void *const *d_bs, unsigned count, const uint64_t *w, void *d_out, size_t batch,
                                     void *hip_stream) {
    const char *who = "fhe_ckks_deep_dot_dev";
    Deep c;
    int rc = check_deep(plans, limbs, specials, alpha, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (count < 1 || count > FHE_CKKS_DOT_MAX_COUNT) return fhe_fail(FHE_E_INVALID, "%s: count=%u must be in [1, %d]", who, count, FHE_CKKS_DOT_MAX_COUNT);
    if (!d_as || !d_bs) return fhe_fail(FHE_E_NULL, "%s: NULL host array", who);
    for (unsigned r = 0; w && r < count; r++)
        for (unsigned i = 0; i < c.k; i++)
            if (w[(u64)r * c.k + i] >= c.p[i]->q) return fhe_fail(FHE_E_INVALID, "%s: weight [%u][%u] is not below its modulus", who, r, i);
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 3ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_key || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_key) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8;
    if (overlaps_any(d_out, ct_bytes, {{d_key, key_words(key_limbs, alpha, n) * 8}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key", who);
    for (unsigned r = 0; r < count; r++) {
        if (!d_as[r] || !d_bs[r]) return fhe_fail(FHE_E_NULL, "%s: an operand of pair %u is NULL", who, r);
        if (misaligned8(d_as[r]) || misaligned8(d_bs[r])) return fhe_fail(FHE_E_INVALID, "%s: the operands of pair %u must be 8-byte aligned", who, r);
        if (overlaps_any(d_out, ct_bytes, {{d_as[r], ct_bytes}, {d_bs[r], ct_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an operand of pair %u", who, r);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    // mul's chunk and workspace: the chunk's summed tensor where fhe_ckks_deep_mul_dev stages its tensor, then ONE relinearisation
    return switch_call(c, batch, deep_slabs(c.k, c.alpha), st, who, [&](u64 r0, u64 cr, const DeepTables &t, u64 *W, const u64 *pinv) {
        const DeepBufs b(W, c, cr * n);
        const int rc = deep_tensorsum_rows(c, d_as, d_bs, count, w, batch, r0, b.Dt, cr, st);
        return rc != FHE_OK ? rc : relin_rows(c, t, (const u64 *)d_key, key_limbs, pinv, b.Dt, cr, 0, (u64 *)d_out, batch, r0, b, cr, st);
    });
}
