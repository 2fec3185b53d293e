// ckks_eval.hip — the CKKS evaluator on an RNS modulus chain: the eval-domain tensor, the basis lift between
// limbs, the key-switch accumulation against a hybrid relinearisation key with one special prime, and the divide-and-round
// that drops a limb (the special prime after a key switch, the top limb in a rescale).
//
//   chain      primes q_0 .. q_L (1 <= L + 1 <= 8) and one special prime P >= max q_i, all distinct, one plan each, same n
//   ciphertext [limb][2][batch][n] evals (the engine's bit-reversed order), canonical; level l = limbs 0 .. l, k = l + 1
//   tensor     per limb: d0 = a0 b0, d1 = a0 b1 + a1 b0 (one reduction of the 128-bit sum), d2 = a1 b1: [limb][3][batch][n]
//   lift       a coefficient-domain residue x mod q_j, centred (x - q_j where x > floor(q_j / 2)), reduced modulo q_i
//   rlk        [j][i][2][n] evals, j <= L, i in {0 .. L, P}: (-a_ji s + e_j + [i = j] (P mod q_j) s^2, a_ji) mod q_i
//   relin      inverse d2 per limb; lift digit j to every limb i != j of {0 .. l, P}; forward; t_i = sum_j D_ji (.) rlk[j][i];
//              r_i = (t_i - lift(t_P)) P^-1 mod q_i; out = (d0 + r0, d1 + r1)
//   rescale    c'_i = (c_i - lift(c_l)) q_l^-1 mod q_i for i < l, both components
//   galois      sigma_g: a(X) -> a(X^g), g odd; in evals an index permutation, sigma_g(a)^[x] = a^[pi_g(x)].  gk_g is
//              rlk with sigma_g(s) for s^2; apply = the key switch of pi_g(c1) plus pi_g(c0).  The digits are those of the
//              unpermuted c1, computed once for any number of g (the automorphism commutes with the transforms and the odd,
//              coefficient-wise lift), and pi_g is folded into the key sums' and the divide-and-round's reads
//   diag sum    out_o = sum_r m_{o,r} (.) sigma_{g_r}(ct) for plaintexts known modulo P as well: the key sums of all
//              elements are weighted and added in the basis Q P by one fused kernel, and each output takes one division by P
//   bsgs        out = sum_a sigma_{h_a}(sum_b m_{a,b} (.) sigma_{g_b}(ct)): the inner sums stay in the basis Q P; a giant
//              step divides only its second component by P, switches it against gk_{h_a} in Q P and adds the permuted first
//              component as it is; one division by P of the sum over the giant steps finishes
//   lincomb     out_o = sum_r w[o][r] ct_r + (k[o], 0) per limb, the inputs read once for up to four outputs
//   dot         relin(sum_r w_r tensor(a_r, b_r)): the tensors of all pairs summed by one fused kernel into the
//              slot ct x ct stages its tensor in, then relin as it is: one key switch whatever the number of pairs
//
// All kernels are grid-stride and element-wise on fhe_ew_grid, bounds-checked against their element count, plain C++ with
// vector stores and no scratch.  The transforms are fhe_ntt_forward_dev / fhe_ntt_inverse_dev on the workspace (slot 12),
// one call per limb and direction over everything of that limb that is ready; a chunk is 2^21 / (n k^2) ciphertexts
// (2^21 / (n k) for a rescale, which stages 2k slabs a ciphertext).
//
// One of each: key_sum is the digit-times-key sum of both accumulating kernels; moddown_rows the modulus-down
// of every key switch and of the rescale (lift, forward and divide-and-round per remaining limb); SwitchBufs the layout and
// the size of a key switch's workspace; switch_call the chunking, workspace and inverses of P of every key-switch entry point.
#include "bfv_client_kernels.hpp"
#include "rns_ext_device.hpp"

using fhe::Mod;
using fhe::u32;
using fhe::u64;

namespace fhe {

constexpr u32 kRnsMaxLimbs = 8, kRnsMaxTargets = kRnsMaxLimbs + 1;

// what reduce_any needs of every target of a lift, by value: indexed by unrolled constants only, so it stays in SGPRs
struct LiftArgs {
    u64 q[kRnsMaxTargets], onep[kRnsMaxTargets];
    u64 off[kRnsMaxTargets];   // first word of target t's residues in dst
    u32 targets;
};

// dst[off[t] + i] = lift of src[i] modulo q[t] for every target t, the source read once.  SIGNED: src holds signed 64-bit
// words (a plaintext row); otherwise canonical residues modulo qs, centred first.  The magnitude is reduced by
// reduce_any's multiplication (x - mulhi(x, floor(2^64 / q)) q lies in [0, 2q) for any 64-bit x), then negated.
template <bool SIGNED>
__global__ __launch_bounds__(256) void ckks_rns_lift_kernel(const u64 *__restrict__ src, u64 *__restrict__ dst, u64 count, u64 qs, LiftArgs a) {
    const u64 stride = (u64)gridDim.x * 256, half = qs >> 1;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 x = src[i];
        const bool neg = SIGNED ? (long long)x < 0 : x > half;
        const u64 mag = SIGNED ? (neg ? 0ull - x : x) : (neg ? qs - x : x);
#pragma unroll
        for (u32 t = 0; t < kRnsMaxTargets; t++) {
            if (t < a.targets) {
                const u64 q = a.q[t];
                u64 r = mag - __umul64hi(mag, a.onep[t]) * q;
                r = r >= q ? r - q : r;
                dst[a.off[t] + i] = (neg && r) ? q - r : r;
            }
        }
    }
}

// the bare automorphism on `count` words of rows of n = 2^L evals: out[r n + x] = in[r n + pi_g(x)]; count is a multiple of n
__global__ __launch_bounds__(256) void ckks_rns_galois_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, u64 count, u32 g, u32 L) {
    const u64 stride = (u64)gridDim.x * 256, n = 1ull << L;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 x = i & (n - 1);
        out[i] = in[i - x + galois_index((u32)x, g, L)];
    }
}

// one limb of the tensor: a, b two components `*_cs` words apart, out three components o_cs apart, `count` words each
__global__ __launch_bounds__(256) void ckks_rns_tensor_kernel(const u64 *__restrict__ a, u64 a_cs, const u64 *__restrict__ b, u64 b_cs, u64 *__restrict__ out,
                                                              u64 o_cs, u64 count, Mod m) {
    const u64 stride = (u64)gridDim.x * 256;
    const bool wide = (m.q >> 62) != 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 a0 = a[i], a1 = a[a_cs + i], b0 = b[i], b1 = b[b_cs + i];
        const u128 s = (u128)a0 * b1 + (u128)a1 * b0;                 // two terms below q^2 < 2^126: below 2^127
        out[i] = bfv_mulmod(a0, b0, m);
        out[o_cs + i] = wide ? reduce128_63((u64)(s >> 64), (u64)s, m) : reduce128((u64)(s >> 64), (u64)s, m);
        out[2 * o_cs + i] = bfv_mulmod(a1, b1, m);
    }
}

// The key sum of one word: a_c += sum_{j < k} D_j[s] key[j][c], c = 0, 1.  Digit j is own[s] for j = own_j (the limb's own
// evals, never lifted; `own` is not read for the special prime, whose own_j is k) and dig[(j - (j > own_j)) dig_stride + s]
// otherwise; its key words are key[j key_stride + x] and key[j key_stride + x + n], x the word's column.
// Overflow: operands are canonical, so a term is below q^2, and the accumulators hold `held` <= 1 such terms on entry.
// q < 2^62: 1 + k <= 9 terms below 2^124 stay below 2^128 and the caller folds once, after the sum.  q >= 2^62 (`wide`): a
// term is below 2^126, so the accumulators fold before every digit that would be their third term since the last fold
// (kMacChunk63 = 2; before even j >= 2 where held = 0, before odd j where held = 1): they then hold a canonical carry-over
// below 2^63 and at most two terms, less than 2^127 + 2^63 < 2^128.
__device__ __forceinline__ void key_sum(MacAcc &a0, MacAcc &a1, u32 held, const u64 *__restrict__ dig, u64 dig_stride, const u64 *__restrict__ own, u32 own_j,
                                        const u64 *__restrict__ key, u64 key_stride, u64 n, u64 x, u64 s, u32 k, bool wide, const Mod &m) {
    for (u32 j = 0; j < k; j++) {
        if (wide && j && (held + j) % kMacChunk63 == 0) {                // held <= 1: nothing to fold before digit 0
            a0.fold63(m);
            a1.fold63(m);
        }
        const u64 d = j == own_j ? own[s] : dig[(u64)(j - (j > own_j ? 1u : 0u)) * dig_stride + s];
        const u64 *__restrict__ kp = key + (u64)j * key_stride + x;
        a0.mac(d, kp[0]);
        a1.mac(d, kp[n]);
    }
}

// One target limb of the key switch: out[c][i] = sum_{j < k} D_j[i] key[j][c][i mod n], c = 0, 1, `count` words a component;
// the key row of digit j is key + j key_stride, [2][n], shared by the batch.
// GATHER (a Galois key switch, §23): the digits and `own` are read at pi_g of the index within the row, the key row at the
// index itself; g is not read otherwise.
template <bool GATHER>
__global__ __launch_bounds__(256) void ckks_rns_keymac_kernel(const u64 *__restrict__ dig, u64 dig_stride, const u64 *__restrict__ own, u32 own_j,
                                                              const u64 *__restrict__ key, u64 key_stride, u64 *__restrict__ out, u32 k, u32 L, u64 count,
                                                              u32 g, Mod m) {
    const u64 stride = (u64)gridDim.x * 256, n = 1ull << L;
    const bool wide = (m.q >> 62) != 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 x = i & (n - 1), s = GATHER ? i - x + galois_index((u32)x, g, L) : i;
        MacAcc a0, a1;
        key_sum(a0, a1, 0, dig, dig_stride, own, own_j, key, key_stride, n, x, s, k, wide, m);
        out[i] = wide ? a0.fold63(m) : a0.fold(m);
        out[count + i] = wide ? a1.fold63(m) : a1.fold(m);
    }
}

// out = (x - t) inv (+ add) mod q over two components of `count` words, each operand's components `*_cs` words apart.  The
// addend is optional, goes to both components and is read at the index itself; g and L, which follow m so that this form's
// arguments lie where they always did, are not read.
// GATHER (the divide-and-round of a Galois key switch, rows of n = 2^L): the addend is pi_g(c0) of the input ciphertext,
// gathered here; it goes to the first component only, and add_cs is not read.
template <bool GATHER>
__global__ __launch_bounds__(256) void ckks_rns_divround_kernel(const u64 *__restrict__ x, u64 x_cs, const u64 *__restrict__ t, u64 t_cs,
                                                                const u64 *__restrict__ add, u64 add_cs, u64 *__restrict__ out, u64 out_cs, u64 count, u64 inv,
                                                                Mod m, u32 g, u32 L) {
    const u64 stride = (u64)gridDim.x * 256, n = 1ull << L;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < 2 * count; i += stride) {
        const u64 c = i >= count ? 1u : 0u, e = i - c * count;
        u64 v = bfv_mulmod(sub63(x[c * x_cs + e], t[c * t_cs + e], m), inv, m);
        if (GATHER && c == 0) {
            const u64 xx = e & (n - 1);
            v = add63(v, add[e - xx + galois_index((u32)xx, g, L)], m);
        } else if (!GATHER && add) {
            v = add63(v, add[c * add_cs + e], m);
        }
        out[c * out_cs + e] = v;
    }
}

// ---- plaintext linear transforms: the double-hoisted diagonal sum -------------------------------------------
constexpr u32 kDiagGroup = 16;     // elements of one launch, passed by value
constexpr u32 kDiagOutputs = 2;    // outputs whose accumulators one launch keeps in registers: 8 waves a SIMD still (§24)

// The elements of one launch for one target limb.  Indexed by the loop counter, which is uniform: the reads are scalar loads
// from the kernel-argument segment, not scratch.
struct DiagGroup {
    const u64 *key[kDiagGroup];    // element r's key rows of this target: digit j at + j key_stride, [2][n]; not read where g = 1
    const u64 *pt[kDiagGroup];     // m_{o, r, i} [n] of the launch's first output; output o at + o pt_os
    u32 g[kDiagGroup];
    u32 count;
};

// One target limb i of out_o = sum_r m_{o,r} (.) sigma_{g_r}(ct) in the extended basis, for NOUT outputs and the elements of
// `grp`, over `count` words a component (rows of n = 2^L):
//   u_o[c][e] (+)= sum_r m_{o,r,i}[x] (t^(r)_c[e] + pmod ct_c[pi_{g_r}(e)] [c = 0 or g_r = 1]),  x = e mod n
// t^(r) is ckks_rns_keymac_kernel<true>'s key sum for g_r (zero for g_r = 1: the identity takes no key).  `ct` is limb i's two
// components, ct_cs words apart, and NULL for the special prime, where the addend vanishes; limb i's own digit is ct's
// second component.  With pmod = P mod q_i the addend rides through the division by P: (u + P a - E) P^-1 = (u - E) P^-1 + a.
// With pmod = 1 and no element but the identity, u is the finished sum and `out` the output ciphertext.
// CARRY: u starts from the canonical words a former group left in `out`; otherwise from zero.
// Overflow.  Operands are canonical, so a term is below q^2.  Key sum: the addend's term, then key_sum with that one term held.
// Outer sum: u_o takes one term m t < q^2 an element; it folds before element r > 0 of the group where r is a multiple of
// kMacChunk (q < 2^62: a carry-over below 2^62 and eight terms below 2^124, less than 2^127 + 2^62) or of kMacChunk63
// (q >= 2^62: a carry-over below 2^63 and two terms below 2^126).  The carry-over is the last fold or the word CARRY read,
// both canonical; an element that is skipped (the identity modulo P) adds no term.  So any count holds: 256 elements are
// 16 groups, each folded to canonical words before it is stored.
template <u32 NOUT, bool CARRY>
__global__ __launch_bounds__(256) void ckks_rns_diagmac_kernel(const u64 *__restrict__ dig, u64 dig_stride, const u64 *__restrict__ ct, u64 ct_cs, u32 own_j,
                                                               u64 key_stride, u64 pt_os, u64 *__restrict__ out, u64 out_cs, u64 out_os, u32 k, u32 L, u64 count,
                                                               u64 pmod, DiagGroup grp, Mod m) {
    const u64 stride = (u64)gridDim.x * 256, n = 1ull << L;
    const bool wide = (m.q >> 62) != 0;
    const u32 chunk = wide ? kMacChunk63 : kMacChunk;
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
            if (r && r % chunk == 0) {
#pragma unroll
                for (u32 o = 0; o < NOUT; o++) {
                    if (wide) u[o][0].fold63(m), u[o][1].fold63(m);
                    else u[o][0].fold(m), u[o][1].fold(m);
                }
            }
            const u32 g = grp.g[r];
            if (g == 1 && !ct) continue;                             // the identity contributes nothing modulo P
            const u64 s = i - x + galois_index((u32)x, g, L);
            MacAcc a0, a1;
            if (ct) {
                a0.mac(ct[s], pmod);
                if (g == 1) a1.mac(ct[ct_cs + s], pmod);
            }
            if (g != 1) key_sum(a0, a1, 1, dig, dig_stride, own, own_j, grp.key[r], key_stride, n, x, s, k, wide, m);
            const u64 t0 = wide ? a0.fold63(m) : a0.fold(m), t1 = wide ? a1.fold63(m) : a1.fold(m);
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
            out[o * out_os + i] = wide ? u[o][0].fold63(m) : u[o][0].fold(m);
            out[o * out_os + out_cs + i] = wide ? u[o][1].fold63(m) : u[o][1].fold(m);
        }
    }
}

// ---- plaintext linear transforms: the hoisted giant steps -----------------------------------------------------------
// One target limb i of a giant step h of the baby-step giant-step sum, in the extended basis, over `count` words a component
// (rows of n = 2^L).  u is U_{a,i}, the inner sum of the giant step as ckks_rns_diagmac_kernel left it (canonical, its two
// components u_cs words apart); v is V_i, the sum over the giant steps (components v_cs apart).
//   SWITCH:  v[0][e] (+)= u[0][pi_h(e)] + sum_j D_j[pi_h(e)] key[j][0][x],  v[1][e] (+)= sum_j D_j[pi_h(e)] key[j][1][x],  x = e mod n
//            D the digits of w_a, the second component of U_a divided by P: `dig`, `own`, `own_j`, `key` are key_sum's.  The first
//            component of U_a is not divided: it is permuted and added as it is, so u's second component is not read.
//   otherwise (h = 1, the identity): v[c][e] (+)= u[c][e] for both components; no digit or key is read.
// CARRY: v holds the canonical words of the former giant steps and is added to; otherwise it is written (the call's first step).
// Overflow.  Every word read is canonical.  The identity adds two words below q < 2^63 in 64 bits (add63).  SWITCH: on entry
// the accumulators hold u[0][pi_h(e)] + v[0][e] < 2q, and v[1][e] < q: each is below q^2 (q >= 5), so each stands for the one
// term that key_sum allows on entry (held = 1).  q < 2^62: that and k <= 8 terms below 2^124 are below 9 2^124 < 2^128, folded
// once at the end.  2^62 <= q < 2^63: key_sum folds before every digit of odd index, so the accumulators hold the entry words
// (below 2^64) and digit 0's term, or a canonical carry-over below 2^63 and two terms below 2^126: less than 2^127 + 2^64.
template <bool SWITCH, bool CARRY>
__global__ __launch_bounds__(256) void ckks_rns_giantmac_kernel(const u64 *__restrict__ dig, u64 dig_stride, const u64 *__restrict__ own, u32 own_j,
                                                                const u64 *__restrict__ key, u64 key_stride, const u64 *__restrict__ u, u64 u_cs,
                                                                u64 *__restrict__ v, u64 v_cs, u32 k, u32 L, u64 count, u32 g, Mod m) {
    const u64 stride = (u64)gridDim.x * 256, n = 1ull << L;
    const bool wide = (m.q >> 62) != 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        if (!SWITCH) {
            const u64 u0 = u[i], u1 = u[u_cs + i];
            v[i] = CARRY ? add63(v[i], u0, m) : u0;
            v[v_cs + i] = CARRY ? add63(v[v_cs + i], u1, m) : u1;
        } else {
            const u64 x = i & (n - 1), s = i - x + galois_index((u32)x, g, L);
            MacAcc a0, a1;
            a0.v = u[s];
            if (CARRY) {
                a0.v += v[i];
                a1.v = v[v_cs + i];
            }
            key_sum(a0, a1, 1, dig, dig_stride, own, own_j, key, key_stride, n, x, s, k, wide, m);
            v[i] = wide ? a0.fold63(m) : a0.fold(m);
            v[v_cs + i] = wide ? a1.fold63(m) : a1.fold(m);
        }
    }
}

// ---- polynomial evaluation: fused sums by public scalars ------------------------------------------------------------
constexpr u32 kLinGroup = 16;     // inputs of one launch, passed by value
constexpr u32 kLinOutputs = 4;     // outputs whose accumulators one launch keeps in registers: 8 waves a SIMD still (§27)

// The inputs of one launch for one limb.  Indexed by the loop counter, which is uniform: scalar loads from the kernel-argument
// segment, as DiagGroup.
struct LinGroup {
    const u64 *ct[kLinGroup];          // input r's limb: its two components, contiguous, 2 count words
    u64 w[kLinOutputs][kLinGroup];     // w[o][r] of this limb for the launch's outputs, canonical
    u64 k[kLinOutputs];                // k[o] of this limb, canonical; not read where CARRY (the first group has added it)
    u32 count;
};

// One limb of out_o = sum_r w[o][r] ct_r + (k[o], 0) for NOUT outputs and the inputs of `grp`, over the 2 count words of a limb
// (component 0 first): out[o out_os + e] (+)= sum_r w[o][r] ct_r[e] + [e < count] k[o].  A constant polynomial has every eval
// equal to the constant, so k goes to every word of component 0.  Every input word is read once, for all NOUT outputs.
// CARRY: the sum starts from the canonical words a former group left in `out`; otherwise from the constant.
// Overflow.  Operands are canonical, so a term is below q^2, and the accumulator starts from a canonical word (the constant or
// the carried word, below q).  It folds before input r > 0 of the group where r is a multiple of kMacChunk (q < 2^62: a
// carry-over below 2^62 and eight terms below 2^124, less than 2^127 + 2^62) or of kMacChunk63 (q >= 2^62: a carry-over below
// 2^63 and two terms below 2^126, less than 2^127 + 2^63); a fold leaves a canonical word.  So any count holds: 64 inputs are
// four groups, each folded to canonical words before it is stored.
template <u32 NOUT, bool CARRY>
__global__ __launch_bounds__(256) void ckks_rns_lincomb_kernel(u64 *__restrict__ out, u64 out_os, u64 count, LinGroup grp, Mod m) {
    const u64 stride = (u64)gridDim.x * 256;
    const bool wide = (m.q >> 62) != 0;
    const u32 chunk = wide ? kMacChunk63 : kMacChunk;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < 2 * count; i += stride) {
        MacAcc u[NOUT];
#pragma unroll
        for (u32 o = 0; o < NOUT; o++) u[o].v = CARRY ? out[o * out_os + i] : (i < count ? grp.k[o] : 0ull);
        for (u32 r = 0; r < grp.count; r++) {
            if (r && r % chunk == 0) {
#pragma unroll
                for (u32 o = 0; o < NOUT; o++) {
                    if (wide) u[o].fold63(m);
                    else u[o].fold(m);
                }
            }
            const u64 x = grp.ct[r][i];
#pragma unroll
            for (u32 o = 0; o < NOUT; o++) u[o].mac(grp.w[o][r], x);
        }
#pragma unroll
        for (u32 o = 0; o < NOUT; o++) out[o * out_os + i] = wide ? u[o].fold63(m) : u[o].fold(m);
    }
}

// ---- inner products: the summed tensor of ct x ct pairs, relinearised once -------------------------------------------
constexpr u32 kDotGroup = 16;      // pairs of one launch, passed by value; the registers do not depend on it (§29)

// The pairs of one launch for one limb.  Indexed by the loop counter, which is uniform: scalar loads from the kernel-argument
// segment, as LinGroup.
struct DotGroup {
    const u64 *a[kDotGroup], *b[kDotGroup];   // pair r's operands, this limb: two components `cs` words apart each
    u64 w[kDotGroup];                         // w_r of this limb, canonical; not read unless WEIGHTED
    u64 cs;                                   // every operand is a ciphertext of the call's batch: one component stride
    u32 count;
};

// One limb of the summed tensor of the pairs of `grp`, over `count` words a component; out is three components o_cs words apart,
// the layout ckks_rns_tensor_kernel writes, canonical:
//   d0[e] (+)= sum_r w_r a_r0[e] b_r0[e],  d1[e] (+)= sum_r w_r (a_r0[e] b_r1[e] + a_r1[e] b_r0[e]),  d2[e] (+)= sum_r w_r a_r1[e] b_r1[e]
// Every operand word is read once.  a_r and b_r may be the same pointer (a square) and a pointer may repeat across pairs: the
// operands are only read, and `out` (the workspace's tensor slot) is none of them.  WEIGHTED = false: w_r = 1, no multiplication.
// CARRY: the three sums start from the canonical words a former group left in `out`; otherwise from zero.
// Overflow.  Operands are canonical, so a product of two of them is below q^2.  The weight is folded into a_r first: w a_r0 and
// w a_r1 are reduced to canonical words (bfv_mulmod) before they meet b, since w a b < q^3 has no room in 128 bits; a term is
// then below q^2 whether weighted or not.  d0 and d2 take one term a pair, d1 takes two, so d1 sets the period and all three
// fold with it.  Between two folds an accumulator holds a canonical carry-over (zero, the last fold, or the word CARRY read:
// below q) and the terms of T pairs, at most (q - 1) + 2 T (q - 1)^2:
//   q < 2^62:         a term is below 2^124; T = kMacChunk / 2 = 4 pairs are eight terms, below 2^127 + 2^62 (MacAcc::fold)
//   2^62 <= q < 2^63: a term is below 2^126; T = kMacChunk63 / 2 = 1 pair is two terms, below 2^127 + 2^63 (MacAcc::fold63)
// (2 T <= 15 and 2 T <= 3 are what 128 bits allow: 7 pairs and 1; 4 keeps to kMacChunk's eight terms.)  So the accumulators
// fold before pair r > 0 of the group where r is a multiple of T, and once more before they are stored; any count holds: 64
// pairs are four groups, each folded to canonical words before it is stored.
template <bool WEIGHTED, bool CARRY>
__global__ __launch_bounds__(256) void ckks_rns_tensorsum_kernel(u64 *__restrict__ out, u64 o_cs, u64 count, DotGroup grp, Mod m) {
    const u64 stride = (u64)gridDim.x * 256;
    const bool wide = (m.q >> 62) != 0;
    const u32 pairs = (wide ? kMacChunk63 : kMacChunk) / 2;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        MacAcc d0, d1, d2;
        if (CARRY) {
            d0.v = out[i];
            d1.v = out[o_cs + i];
            d2.v = out[2 * o_cs + i];
        }
        for (u32 r = 0; r < grp.count; r++) {
            if (r && r % pairs == 0) {
                if (wide) d0.fold63(m), d1.fold63(m), d2.fold63(m);
                else d0.fold(m), d1.fold(m), d2.fold(m);
            }
            const u64 *a = grp.a[r], *b = grp.b[r];
            u64 a0 = a[i], a1 = a[grp.cs + i];
            const u64 b0 = b[i], b1 = b[grp.cs + i];
            if (WEIGHTED) {
                a0 = bfv_mulmod(grp.w[r], a0, m);
                a1 = bfv_mulmod(grp.w[r], a1, m);
            }
            d0.mac(a0, b0);
            d1.mac(a0, b1);
            d1.mac(a1, b0);
            d2.mac(a1, b1);
        }
        out[i] = wide ? d0.fold63(m) : d0.fold(m);
        out[o_cs + i] = wide ? d1.fold63(m) : d1.fold(m);
        out[2 * o_cs + i] = wide ? d2.fold63(m) : d2.fold(m);
    }
}

// the diagonal term of a switching key, in evals (n = 2^L, c = P mod q_j): pk0 += c s^2 for the relinearisation key, g not
// read; GALOIS: pk0 += c sigma_g(s)^, the secret's evals gathered by pi_g
template <bool GALOIS>
__global__ __launch_bounds__(256) void ckks_rns_keyterm_kernel(u64 *__restrict__ pk0, const u64 *__restrict__ s_evals, u64 c, u32 g, u32 L, Mod m) {
    const u64 n = 1ull << L;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u64 s = s_evals[GALOIS ? galois_index((u32)i, g, L) : i];
        pk0[i] = add63(pk0[i], bfv_mulmod(c, GALOIS ? s : bfv_mulmod(s, s, m), m), m);
    }
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

constexpr int kCkksEvalSlot = 12;   // fhe_workspace_get slot (11 is the CKKS client's)

struct Chain {
    unsigned k = 0;                                  // limbs in use
    u64 n = 0;
    u32 L = 0;
    const fhe_ntt_plan *p[fhe::kRnsMaxTargets] = {};   // p[k] is the special prime's plan where the call has one
};

// the chain of a *_workspace_bytes query, which has sizes and no plans; false where one of them is out of range
bool chain_of(uint64_t n, unsigned limbs, size_t batch, Chain *c) {
    if (n < 2 || (n & (n - 1)) != 0 || n > (1ull << 19) || limbs < 1 || limbs > fhe::kRnsMaxLimbs || batch == 0) return false;
    c->k = limbs;
    c->n = n;
    c->L = log2_of(n);
    return true;
}

// plans[0 .. limbs) and, where the entry point takes one, the special prime: FHE_E_NULL, then the limb count, the ring, the
// repeated moduli, P >= max q_i
int check_chain(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, bool want_special, Chain *c, const char *who) {
    if (!plans) return fhe_fail(FHE_E_NULL, "%s: plans is NULL", who);
    if (limbs < 1 || limbs > fhe::kRnsMaxLimbs) return fhe_fail(FHE_E_INVALID, "%s: limbs=%u must be in [1, 8]", who, limbs);
    for (unsigned i = 0; i < limbs; i++)
        if (!plans[i]) return fhe_fail(FHE_E_NULL, "%s: plan %u is NULL", who, i);
    if (want_special && !special) return fhe_fail(FHE_E_NULL, "%s: the special prime's plan is NULL", who);
    c->k = limbs;
    c->n = plans[0]->n;
    c->L = plans[0]->log_n;
    for (unsigned i = 0; i < limbs; i++) c->p[i] = plans[i];
    const unsigned all = limbs + (want_special ? 1u : 0u);
    if (want_special) c->p[limbs] = special;
    for (unsigned i = 1; i < all; i++)
        if (c->p[i]->n != c->n) return fhe_fail(FHE_E_PARAM_MISMATCH, "%s: plan %u has n=%llu, plan 0 n=%llu", who, i, (unsigned long long)c->p[i]->n, (unsigned long long)c->n);
    if (c->n < 2) return fhe_fail(FHE_E_BAD_N, "%s: n must be at least 2", who);
    for (unsigned i = 0; i < all; i++)
        for (unsigned j = 0; j < i; j++)
            if (c->p[i]->q == c->p[j]->q) return fhe_fail(FHE_E_INVALID, "%s: modulus %llu is repeated in the chain", who, (unsigned long long)c->p[i]->q);
    if (want_special)
        for (unsigned i = 0; i < limbs; i++)
            if (special->q < c->p[i]->q) return fhe_fail(FHE_E_INVALID, "%s: the special prime must not be below a chain prime", who);
    return FHE_OK;
}

// ciphertexts of a chunk: 2^21 / (n k^2), at least one
u64 chunk_rows(const Chain &c, u64 batch) { return std::min<u64>(batch, std::max<u64>(1, (kChunkWords >> c.L) / ((u64)c.k * c.k))); }
// a rescale stages 2k slabs a ciphertext, not k^2 + 8k + 2: its chunk is 2^21 / (n k) ciphertexts, at least one
u64 rescale_chunk_rows(const Chain &c, u64 batch) { return std::min<u64>(batch, std::max<u64>(1, (kChunkWords >> c.L) / (u64)c.k)); }

// body(r0, cr) over the batch in chunks of cb ciphertexts
template <class Body>
int for_chunks(u64 batch, u64 cb, Body body) {
    for (u64 r0 = 0; r0 < batch; r0 += cb) {
        const int rc = body(r0, std::min<u64>(cb, batch - r0));
        if (rc != FHE_OK) return rc;
    }
    return FHE_OK;
}

int lift_launch(bool is_signed, const u64 *src, u64 *dst, u64 count, u64 qs, const fhe::LiftArgs &a, u32 L, hipStream_t st) {
    if (a.targets == 0) return FHE_OK;
    return is_signed ? launch_named("ckks_rns_lift", "ckks_rns_lift_kernel", (int)L, st, fhe::ckks_rns_lift_kernel<true>, fhe_ew_grid(count), 256, src, dst, count, qs, a)
                     : launch_named("ckks_rns_lift", "ckks_rns_lift_kernel", (int)L, st, fhe::ckks_rns_lift_kernel<false>, fhe_ew_grid(count), 256, src, dst, count, qs, a);
}
void lift_target(fhe::LiftArgs *a, const fhe_ntt_plan *p, u64 off) {
    a->q[a->targets] = p->q;
    a->onep[a->targets] = p->mod.onep;
    a->off[a->targets] = off;
    a->targets++;
}

// `polys` rows of evals, which the ABI aligns to 8 bytes, as coefficients in the workspace rows dst
int inverse_into(const fhe_ntt_plan *p, const u64 *src, u64 *dst, u64 polys, hipStream_t st) {
    const int rc = aligned_rows(src, dst, polys * p->n, st, &src);
    return rc != FHE_OK ? rc : fhe_ntt_inverse_dev(p, src, dst, polys, st);
}

int tensor_rows(const Chain &c, const u64 *a, const u64 *b, u64 batch, u64 r0, u64 *out, u64 o_rows, u64 o_r0, u64 cr, hipStream_t st) {
    const u64 n = c.n;
    for (unsigned i = 0; i < c.k; i++) {
        const int rc = launch("ckks_rns_tensor", (int)c.L, st, fhe::ckks_rns_tensor_kernel, fhe_ew_grid(cr * n), 256, a + ((u64)i * 2 * batch + r0) * n, batch * n,
                              b + ((u64)i * 2 * batch + r0) * n, batch * n, out + ((u64)i * 3 * o_rows + o_r0) * n, o_rows * n, cr * n, c.p[i]->mod);
        if (rc != FHE_OK) return rc;
    }
    return FHE_OK;
}

// The workspace of one key switch over cr ciphertexts (slab = cr n words): C the k digits in coefficients, D their lifts as
// evals (limb i < k holds the k - 1 digits j != i, P all k), `sets` sets T of the k + 1 key sums of two components (one
// for a relinearisation or a Galois element, one per output of a diagonal launch), E the lifted t_P of one set at a time
struct SwitchBufs {
    u64 *C, *D, *T, *E;
    u64 slab, set;                                                   // words of one T set: 2 (k + 1) slabs
    unsigned k;
    static u64 words(unsigned k, unsigned sets) { return (u64)k * k + 3ull * k + 2ull * (k + 1) * sets; }   // in slabs: C k, D k^2, E 2k, T
    SwitchBufs(u64 *W, unsigned k_, unsigned sets, u64 slab_)
        : C(W), D(C + k_ * slab_), T(D + (u64)k_ * k_ * slab_), E(T + 2ull * (k_ + 1) * slab_ * sets), slab(slab_), set(2ull * (k_ + 1) * slab_), k(k_) {}
    u64 *D_of(unsigned i) const { return D + (u64)i * (k - 1) * slab; }
    u64 *T_of(unsigned o) const { return T + o * set; }
    u64 *TP(unsigned o) const { return T_of(o) + 2ull * k * slab; }
};
// words of workspace per ciphertext of a chunk.  A Galois key switch shares the digits among its elements and a diagonal sum
// adds the elements in registers, so their count does not enter; ct x ct stages the tensor's 3k slabs in front (and the
// relinearisation of a given tensor asks for as much)
u64 galois_words_per_row(const Chain &c) { return SwitchBufs::words(c.k, 1) * c.n; }
u64 words_per_row(const Chain &c) { return galois_words_per_row(c) + 3ull * c.k * c.n; }
u64 diag_words_per_row(const Chain &c, unsigned outputs) { return SwitchBufs::words(c.k, std::min<unsigned>(outputs, fhe::kDiagOutputs)) * c.n; }

// steps (1)-(3) of §22: digit j = src(j) (cr rows of evals modulo q_j) in coefficients, lifted to every limb i != j of
// {0 .. k - 1, P} and transformed
template <class Src>
int digit_rows(const Chain &c, Src src, const SwitchBufs &b, u64 cr, hipStream_t st) {
    const unsigned k = c.k;
    int rc;
    for (unsigned j = 0; j < k; j++)
        if ((rc = inverse_into(c.p[j], src(j), b.C + j * b.slab, cr, st)) != FHE_OK) return rc;
    for (unsigned j = 0; j < k; j++) {
        fhe::LiftArgs a{};
        for (unsigned i = 0; i <= k; i++)
            if (i != j) lift_target(&a, c.p[i], (u64)(b.D_of(i) - b.D) + (u64)(i < k && j > i ? j - 1 : j) * b.slab);
        if ((rc = lift_launch(false, b.C + j * b.slab, b.D, b.slab, c.p[j]->q, a, c.L, st)) != FHE_OK) return rc;
    }
    for (unsigned i = 0; i <= k; i++) {
        const u64 polys = (u64)(i < k ? k - 1 : k) * cr;
        if (polys && (rc = fhe_ntt_forward_dev(c.p[i], b.D_of(i), b.D_of(i), polys, st)) != FHE_OK) return rc;
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

// The modulus-down by the prime of plan `drop`, which leaves limbs 0 .. drop - 1 (the special prime after a key switch, the
// top limb in a rescale).  X holds the dropped limb's two components in coefficients, `slab` words each; they are lifted to
// every remaining limb and transformed in E (2 drop slabs), and out_i = (x_i - E_i) inv[i] (+ add_i) mod q_i.  g != 0: the
// modulus-down of a Galois key switch, whose addend is pi_g of add's first component, for the first component only.
int moddown_rows(const Chain &c, unsigned drop, const u64 *X, u64 *E, u64 slab, LimbRows<const u64> x, LimbRows<const u64> add, LimbRows<u64> out, const u64 *inv,
                 u32 g, hipStream_t st) {
    int rc;
    fhe::LiftArgs a{};
    for (unsigned i = 0; i < drop; i++) lift_target(&a, c.p[i], 2ull * i * slab);
    if ((rc = lift_launch(false, X, E, 2 * slab, c.p[drop]->q, a, c.L, st)) != FHE_OK) return rc;
    for (unsigned i = 0; i < drop; i++)
        if ((rc = fhe_ntt_forward_dev(c.p[i], E + a.off[i], E + a.off[i], 2 * (slab >> c.L), st)) != FHE_OK) return rc;
    for (unsigned i = 0; i < drop; i++)
        if ((rc = launch(g ? "ckks_rns_divround_galois" : "ckks_rns_divround", (int)c.L, st, g ? fhe::ckks_rns_divround_kernel<true> : fhe::ckks_rns_divround_kernel<false>,
                         fhe_ew_grid(2 * slab), 256, x.of(i), x.cs, E + a.off[i], slab, add.of(i), add.cs, out.of(i), out.cs, slab, inv[i], c.p[i]->mod, g, c.L)) != FHE_OK)
            return rc;
    return FHE_OK;
}

// step (4): T = sum_j D_ji (.) key[j][i], i in {0 .. k - 1, P}; own(i) is limb i's own digit in evals.  g != 0: a Galois key
// switch, the digits read at pi_g
template <class Own>
int keymac_rows(const Chain &c, const u64 *key, unsigned key_limbs, Own own, const SwitchBufs &b, u32 g, hipStream_t st) {
    const unsigned k = c.k;
    const u64 n = c.n;
    for (unsigned i = 0; i <= k; i++) {
        const u64 *col = key + (u64)(i < k ? i : key_limbs) * 2 * n;
        const int rc = launch(g ? "ckks_rns_keymac_galois" : "ckks_rns_keymac", (int)c.L, st, g ? fhe::ckks_rns_keymac_kernel<true> : fhe::ckks_rns_keymac_kernel<false>,
                              fhe_ew_grid(b.slab), 256, b.D_of(i), b.slab, i < k ? own(i) : nullptr, i, col, (u64)(key_limbs + 1) * 2 * n, b.T + 2ull * i * b.slab, k, c.L,
                              b.slab, g, c.p[i]->mod);
        if (rc != FHE_OK) return rc;
    }
    return FHE_OK;
}

// step (5) on set o of T: t_P in coefficients, in place, and the modulus-down by P of the set's k limbs
int special_down(const Chain &c, const SwitchBufs &b, unsigned o, LimbRows<const u64> add, LimbRows<u64> out, const u64 *pinv, u32 g, hipStream_t st) {
    const int rc = fhe_ntt_inverse_dev(c.p[c.k], b.TP(o), b.TP(o), 2 * (b.slab >> c.L), st);
    return rc != FHE_OK ? rc : moddown_rows(c, c.k, b.TP(o), b.E, b.slab, {b.T_of(o), 2 * b.slab, b.slab}, add, out, pinv, g, st);
}

// rows d_r0 .. d_r0 + cr of d [k][3][d_rows][n] -> rows o_r0 .. of out [k][2][o_rows][n]; W holds SwitchBufs::words(k, 1) slabs
int relin_rows(const Chain &c, const u64 *rlk, unsigned key_limbs, const u64 *pinv, const u64 *d, u64 d_rows, u64 d_r0, u64 *out, u64 o_rows, u64 o_r0, u64 cr,
               u64 *W, hipStream_t st) {
    const u64 n = c.n;
    const SwitchBufs b(W, c.k, 1, cr * n);
    auto d2 = [&](unsigned limb) { return d + (((u64)limb * 3 + 2) * d_rows + d_r0) * n; };
    int rc;
    if ((rc = digit_rows(c, d2, b, cr, st)) != FHE_OK) return rc;
    if ((rc = keymac_rows(c, rlk, key_limbs, d2, b, 0u, st)) != FHE_OK) return rc;
    return special_down(c, b, 0, {d + d_r0 * n, 3 * d_rows * n, d_rows * n}, {out + o_r0 * n, 2 * o_rows * n, o_rows * n}, pinv, 0u, st);
}

// §23: rows r0 .. r0 + cr of in [k][2][batch][n] under each of `count` Galois elements -> the same rows of out
// [count][k][2][batch][n].  The digits are those of the unpermuted c1, made once; every g then takes its key sums with the
// digits read at pi_g, the divide-and-round by P, and pi_g(c0) gathered in that last kernel.  W as for relin_rows.
int galois_rows(const Chain &c, const u64 *const *gks, const uint64_t *gs, unsigned count, unsigned key_limbs, const u64 *pinv, const u64 *in, u64 *out, u64 batch,
                u64 r0, u64 cr, u64 *W, hipStream_t st) {
    const u64 n = c.n, o_words = 2ull * c.k * batch * n;
    const SwitchBufs b(W, c.k, 1, cr * n);
    const LimbRows<const u64> ct{in + r0 * n, 2 * batch * n, batch * n};
    auto c1 = [&](unsigned limb) { return ct.of(limb) + ct.cs; };
    int rc;
    if ((rc = digit_rows(c, c1, b, cr, st)) != FHE_OK) return rc;
    for (unsigned r = 0; r < count; r++) {
        const u32 g = (u32)gs[r];
        if ((rc = keymac_rows(c, gks[r], key_limbs, c1, b, g, st)) != FHE_OK) return rc;
        if ((rc = special_down(c, b, 0, ct, {out + r * o_words + r0 * n, ct.ls, ct.cs}, pinv, g, st)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

int check_key_limbs(const Chain &c, unsigned key_limbs, const char *who) {
    if (key_limbs < c.k || key_limbs > fhe::kRnsMaxLimbs)
        return fhe_fail(FHE_E_INVALID, "%s: key_limbs=%u must be at least limbs=%u and at most 8", who, key_limbs, c.k);
    return FHE_OK;
}

// r < 0: the call's one element g; otherwise element r of its list
int check_galois_element(uint64_t g, u64 n, int r, const char *who) {
    if ((g & 1) != 0 && g < 2 * n) return FHE_OK;
    char name[16] = "g";
    if (r >= 0) snprintf(name, sizeof name, "g[%d]", r);
    return fhe_fail(FHE_E_INVALID, "%s: %s=%llu must be odd and below 2n", who, name, (unsigned long long)g);
}

// The `count` elements and keys [key_limbs][key_limbs + 1][2][n] of a call that writes out_bytes at d_out: every key present,
// aligned and clear of the output, every element odd and below 2n.  skip_identity (a diagonal sum): g = 1 takes no key and
// its entry is not read, so the element is looked at before its key; *switched says whether any key is read at all.
int check_switch_keys(const void *const *d_gks, const uint64_t *gs, unsigned count, bool skip_identity, u64 n, unsigned key_limbs, const void *d_out, u64 out_bytes,
                      bool *switched, const char *who) {
    const u64 gk_bytes = (u64)key_limbs * (key_limbs + 1) * 2 * n * 8;
    int rc;
    for (unsigned r = 0; r < count; r++) {
        if (skip_identity && (rc = check_galois_element(gs[r], n, (int)r, who)) != FHE_OK) return rc;
        if (skip_identity && gs[r] == 1) continue;
        *switched = true;
        if (!d_gks || !d_gks[r]) return fhe_fail(FHE_E_NULL, "%s: key %u is NULL", who, r);
        if (misaligned8(d_gks[r])) return fhe_fail(FHE_E_INVALID, "%s: key %u must be 8-byte aligned", who, r);
        if (!skip_identity && (rc = check_galois_element(gs[r], n, (int)r, who)) != FHE_OK) return rc;
        if (overlaps_any(d_out, out_bytes, {{d_gks[r], gk_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps key %u", who, r);
    }
    return FHE_OK;
}

// The frame of a key-switch call: chunks of chunk_rows ciphertexts, `words` words of workspace a ciphertext in `slot` (none:
// the call only needs a device), the inverses of P, and body(r0, cr, W, pinv) per chunk
template <class Body>
int switch_call_in(int slot, const Chain &c, u64 batch, u64 words, hipStream_t st, Body body) {
    const u64 cb = chunk_rows(c, batch);
    void *w = nullptr;
    int rc, dev;
    if ((rc = words ? fhe_workspace_get(slot, (size_t)(words * cb * 8), st, &w) : fhe_current_device(&dev)) != FHE_OK) return rc;
    u64 pinv[fhe::kRnsMaxLimbs];
    for (unsigned i = 0; i < c.k; i++) pinv[i] = fhe::host::inv_mod(c.p[i]->q, c.p[c.k]->q);
    return for_chunks(batch, cb, [&](u64 r0, u64 cr) { return body(r0, cr, (u64 *)w, pinv); });
}
template <class Body>
int switch_call(const Chain &c, u64 batch, u64 words, hipStream_t st, Body body) {
    return switch_call_in(kCkksEvalSlot, c, batch, words, st, body);
}

}  // namespace

extern "C" size_t fhe_ckks_rns_workspace_bytes(uint64_t n, unsigned limbs, size_t batch) {
    Chain c;
    if (!chain_of(n, limbs, batch, &c)) return 0;
    return (size_t)(std::max<u64>(words_per_row(c) * chunk_rows(c, batch), 2ull * limbs * n * rescale_chunk_rows(c, batch)) * 8);
}

extern "C" int fhe_ckks_rns_from_i64_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_rns_from_i64_dev";
    Chain c;
    int rc = check_chain(plans, limbs, nullptr, false, &c, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, (u64)c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_out, (u64)c.k * batch * n * 8, {{d_in, (u64)batch * n * 8}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the rows", who);
    int dev;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    u64 *out = (u64 *)d_out;
    const bool direct = !fhe_misaligned(d_out);                      // residues land in d_out and are transformed in place
    const u64 cb = direct ? (u64)batch : chunk_rows(c, batch);
    u64 *W = nullptr;
    if (!direct) {
        void *w = nullptr;
        if ((rc = fhe_workspace_get(kCkksEvalSlot, (size_t)((u64)c.k * cb * n * 8), st, &w)) != FHE_OK) return rc;
        W = (u64 *)w;
    }
    for (u64 r0 = 0; r0 < batch; r0 += cb) {
        const u64 cr = std::min<u64>(cb, batch - r0);
        fhe::LiftArgs a{};
        for (unsigned i = 0; i < c.k; i++) lift_target(&a, c.p[i], direct ? (u64)i * batch * n : (u64)i * cr * n);
        u64 *dst = direct ? out : W;
        if ((rc = lift_launch(true, (const u64 *)d_in + r0 * n, dst, cr * n, 0, a, c.L, st)) != FHE_OK) return rc;
        for (unsigned i = 0; i < c.k; i++) {
            u64 *row = dst + a.off[i];
            if ((rc = fhe_ntt_forward_dev(c.p[i], row, row, cr, st)) != FHE_OK) return rc;
            if (!direct) HIP_TRY(hipMemcpyAsync(out + ((u64)i * batch + r0) * n, row, cr * n * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    return FHE_OK;
}

namespace {

// a hybrid switching key [limbs][limbs + 1][2][n]: the public key of row first_row + j under every prime plus the diagonal
// term (P mod q_j) x, x = s^2 for the relinearisation key (g = 0) and sigma_g(s) for a Galois key
int switch_key(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const uint8_t *seed, uint64_t first_row, uint64_t g, bool galois,
               const void *d_s, const void *d_cdt, unsigned m, void *d_key, void *hip_stream, const char *who) {
    Chain c;
    int rc = check_chain(plans, limbs, special, true, &c, who);
    if (rc != FHE_OK) return rc;
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    const u64 n = c.n;
    const unsigned k = c.k, cols = k + 1;
    if (galois && (rc = check_galois_element(g, n, -1, who)) != FHE_OK) return rc;
    u64 qmin = c.p[0]->q;
    for (unsigned i = 1; i < k; i++) qmin = std::min<u64>(qmin, c.p[i]->q);
    if ((rc = check_cdt_shape(d_cdt, m, qmin, who)) != FHE_OK) return rc;
    if (first_row >= kRowLimit - k) return fhe_fail(FHE_E_INVALID, "%s: first_row + limbs passes 2^63", who);
    if (!d_s || !d_key) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_s) || misaligned8(d_key)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 key_words = (u64)k * cols * 2 * n;
    if (overlaps_any(d_key, key_words * 8, {{d_s, (u64)cols * n * 8}, {d_cdt, (u64)m * 8}})) return fhe_fail(FHE_E_INVALID, "%s: the key overlaps the secret or the error table", who);
    hipStream_t st = (hipStream_t)hip_stream;
    if ((rc = check_cdt_words(d_cdt, m, st, who)) != FHE_OK) return rc;
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kCkksEvalSlot, (size_t)(4 * n * 8), st, &w)) != FHE_OK) return rc;
    u64 *PK = (u64 *)w, *S = PK + 2 * n, *SE = S + n;            // one key row, the limb's secret (16-byte aligned) and its evals
    for (unsigned j = 0; j < k; j++) {
        for (unsigned i = 0; i < cols; i++) {
            const fhe_ntt_plan *p = c.p[i];
            HIP_TRY(hipMemcpyAsync(S, (const u64 *)d_s + (u64)i * n, n * 8, hipMemcpyDeviceToDevice, st));
            if ((rc = fhe_ckks_public_key_dev(p, seed, first_row + j, S, d_cdt, m, PK, st)) != FHE_OK) return rc;
            if ((rc = fhe_ntt_forward_dev(p, PK, PK, 2, st)) != FHE_OK) return rc;
            if (i == j) {
                if ((rc = fhe_ntt_forward_dev(p, S, SE, 1, st)) != FHE_OK) return rc;
                if ((rc = launch(galois ? "ckks_rns_keyterm_galois" : "ckks_rns_keyterm", (int)c.L, st, galois ? fhe::ckks_rns_keyterm_kernel<true> : fhe::ckks_rns_keyterm_kernel<false>,
                                 fhe_ew_grid(n), 256, PK, SE, special->q % p->q, (u32)g, c.L, p->mod)) != FHE_OK)
                    return rc;
            }
            HIP_TRY(hipMemcpyAsync((u64 *)d_key + ((u64)j * cols + i) * 2 * n, PK, 2 * n * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    return FHE_OK;
}

}  // namespace

extern "C" int fhe_ckks_rns_relin_key_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const uint8_t *seed, uint64_t first_row,
                                          const void *d_s, const void *d_cdt, unsigned m, void *d_rlk, void *hip_stream) {
    return switch_key(plans, limbs, special, seed, first_row, 0, false, d_s, d_cdt, m, d_rlk, hip_stream, "fhe_ckks_rns_relin_key_dev");
}

extern "C" int fhe_ckks_rns_galois_key_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const uint8_t *seed, uint64_t first_row,
                                           uint64_t g, const void *d_s, const void *d_cdt, unsigned m, void *d_gk, void *hip_stream) {
    return switch_key(plans, limbs, special, seed, first_row, g, true, d_s, d_cdt, m, d_gk, hip_stream, "fhe_ckks_rns_galois_key_dev");
}

extern "C" int fhe_ckks_rns_tensor_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *d_a, const void *d_b, void *d_out, size_t batch,
                                       void *hip_stream) {
    const char *who = "fhe_ckks_rns_tensor_dev";
    Chain c;
    int rc = check_chain(plans, limbs, nullptr, false, &c, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 3ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_a || !d_b || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_a) || misaligned8(d_b) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 in_bytes = 2ull * c.k * batch * n * 8;
    if (overlaps_any(d_out, 3ull * c.k * batch * n * 8, {{d_a, in_bytes}, {d_b, in_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an operand", who);
    int dev;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    return tensor_rows(c, (const u64 *)d_a, (const u64 *)d_b, batch, 0, (u64 *)d_out, batch, 0, batch, (hipStream_t)hip_stream);
}

extern "C" int fhe_ckks_rns_relinearize_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const void *d_rlk, unsigned key_limbs,
                                            const void *d_d, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_rns_relinearize_dev";
    Chain c;
    int rc = check_chain(plans, limbs, special, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 3ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_rlk || !d_d || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_rlk) || misaligned8(d_d) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 rlk_bytes = (u64)key_limbs * (key_limbs + 1) * 2 * n * 8;
    if (overlaps_any(d_out, 2ull * c.k * batch * n * 8, {{d_d, 3ull * c.k * batch * n * 8}, {d_rlk, rlk_bytes}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the tensor or the key", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return switch_call(c, batch, words_per_row(c), st, [&](u64 r0, u64 cr, u64 *W, const u64 *pinv) {
        return relin_rows(c, (const u64 *)d_rlk, key_limbs, pinv, (const u64 *)d_d, batch, r0, (u64 *)d_out, batch, r0, cr, W, st);
    });
}

// ---- what bfv_rns.hip runs of this unit (capi_internal.hpp): a kernel is launched from the unit that defines it ----
// one limb of the tensor, ckks_rns_tensor_kernel as tensor_rows launches it
int fhe_rns_tensor_limb(const fhe_ntt_plan *p, const u64 *a, u64 a_cs, const u64 *b, u64 b_cs, u64 *out, u64 o_cs, u64 count, hipStream_t st) {
    return launch("ckks_rns_tensor", (int)p->log_n, st, fhe::ckks_rns_tensor_kernel, fhe_ew_grid(count), 256, a, a_cs, b, b_cs, out, o_cs, count, p->mod);
}
// relin_rows on a chunk's tensor d [limbs][3][cr][n] that the caller keeps: -> rows r0 .. r0 + cr of out [limbs][2][batch][n],
// against a key of `limbs` digits; the key switch's buffers come from this unit's workspace slot
int fhe_rns_relin_rows(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const u64 *rlk, const u64 *d, u64 cr, u64 *out, u64 batch,
                       u64 r0, hipStream_t st) {
    Chain c;
    int rc = check_chain(plans, limbs, special, true, &c, "fhe_rns_relin_rows");
    if (rc != FHE_OK) return rc;
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kCkksEvalSlot, (size_t)(galois_words_per_row(c) * cr * 8), st, &w)) != FHE_OK) return rc;
    u64 pinv[fhe::kRnsMaxLimbs];
    for (unsigned i = 0; i < c.k; i++) pinv[i] = fhe::host::inv_mod(c.p[i]->q, c.p[c.k]->q);
    return relin_rows(c, rlk, limbs, pinv, d, cr, 0, out, batch, r0, cr, (u64 *)w, st);
}

// ---- what ckks_deep.hip runs of this unit ----
// one limb of a divide-and-round, ckks_rns_divround_kernel as moddown_rows launches it: g != 0 gathers add's first component
int fhe_rns_divround_limb(const fhe_ntt_plan *p, const u64 *x, u64 x_cs, const u64 *t, u64 t_cs, const u64 *add, u64 add_cs, u64 *out, u64 out_cs, u64 count, u64 inv,
                          u32 g, hipStream_t st) {
    return launch(g ? "ckks_rns_divround_galois" : "ckks_rns_divround", (int)p->log_n, st, g ? fhe::ckks_rns_divround_kernel<true> : fhe::ckks_rns_divround_kernel<false>,
                  fhe_ew_grid(2 * count), 256, x, x_cs, t, t_cs, add, add_cs, out, out_cs, count, inv, p->mod, g, p->log_n);
}
// the diagonal term of one key row, ckks_rns_keyterm_kernel as switch_key launches it: pk0 += c s^2, or c sigma_g(s) where galois
int fhe_rns_keyterm_limb(const fhe_ntt_plan *p, u64 *pk0, const u64 *s_evals, u64 c, u32 g, bool galois, hipStream_t st) {
    return launch(galois ? "ckks_rns_keyterm_galois" : "ckks_rns_keyterm", (int)p->log_n, st, galois ? fhe::ckks_rns_keyterm_kernel<true> : fhe::ckks_rns_keyterm_kernel<false>,
                  fhe_ew_grid(p->n), 256, pk0, s_evals, c, g, p->log_n, p->mod);
}

extern "C" int fhe_ckks_rns_mul_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const void *d_rlk, unsigned key_limbs,
                                    const void *d_a, const void *d_b, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_rns_mul_dev";
    Chain c;
    int rc = check_chain(plans, limbs, special, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 3ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_rlk || !d_a || !d_b || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_rlk) || misaligned8(d_a) || misaligned8(d_b) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8, rlk_bytes = (u64)key_limbs * (key_limbs + 1) * 2 * n * 8;
    if (overlaps_any(d_out, ct_bytes, {{d_a, ct_bytes}, {d_b, ct_bytes}, {d_rlk, rlk_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an operand or the key", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return switch_call(c, batch, words_per_row(c), st, [&](u64 r0, u64 cr, u64 *Dt, const u64 *pinv) {   // Dt: the chunk's tensor, then relin_rows' buffers
        const int rc = tensor_rows(c, (const u64 *)d_a, (const u64 *)d_b, batch, r0, Dt, cr, 0, cr, st);
        return rc != FHE_OK ? rc : relin_rows(c, (const u64 *)d_rlk, key_limbs, pinv, Dt, cr, 0, (u64 *)d_out, batch, r0, cr, Dt + 3ull * c.k * cr * n, st);
    });
}

extern "C" int fhe_ckks_rns_rescale_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_rns_rescale_dev";
    Chain c;
    int rc = check_chain(plans, limbs, nullptr, false, &c, who);
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
    const u64 cb = rescale_chunk_rows(c, batch);
    void *w = nullptr;
    if ((rc = fhe_workspace_get(kCkksEvalSlot, (size_t)(2ull * k * cb * n * 8), st, &w)) != FHE_OK) return rc;
    u64 qinv[fhe::kRnsMaxLimbs];
    for (unsigned i = 0; i < top; i++) qinv[i] = fhe::host::inv_mod(c.p[i]->q, c.p[top]->q);
    const LimbRows<const u64> in{(const u64 *)d_in, 2 * batch * n, batch * n};
    return for_chunks(batch, cb, [&](u64 r0, u64 cr) {
        const u64 slab = cr * n;
        u64 *C = (u64 *)w, *E = C + 2 * slab;
        const u64 *t0 = in.of(top) + r0 * n;                         // the top limb's two components, batch n apart
        int rc;
        if (cr == batch) {
            if ((rc = inverse_into(c.p[top], t0, C, 2 * cr, st)) != FHE_OK) return rc;
        } else {
            if ((rc = inverse_into(c.p[top], t0, C, cr, st)) != FHE_OK) return rc;
            if ((rc = inverse_into(c.p[top], t0 + in.cs, C + slab, cr, st)) != FHE_OK) return rc;
        }
        return moddown_rows(c, top, C, E, slab, {in.p + r0 * n, in.ls, in.cs}, {}, {(u64 *)d_out + r0 * n, in.ls, in.cs}, qinv, 0u, st);
    });
}

// ---- Galois automorphisms: slot rotations and conjugation ---------------------------------------------------------
extern "C" int fhe_ckks_galois_evals_dev(const fhe_ntt_plan *plan, uint64_t g, const void *d_in, void *d_out, size_t polys, void *hip_stream) {
    const char *who = "fhe_ckks_galois_evals_dev";
    if (!plan) return fhe_fail(FHE_E_NULL, "%s: plan is NULL", who);
    const u64 n = plan->n;
    if (n < 2) return fhe_fail(FHE_E_BAD_N, "%s: n must be at least 2", who);
    int rc = check_galois_element(g, n, -1, who);
    if (rc != FHE_OK) return rc;
    if (polys == 0) return FHE_OK;
    if (!mul_fits((u64)polys, n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: polys too large", who);
    if (!d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 words = (u64)polys * n;
    if (overlaps_any(d_out, words * 8, {{d_in, words * 8}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps d_in (the permutation is not in place)", who);
    int dev;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    return launch("ckks_rns_galois", (int)plan->log_n, (hipStream_t)hip_stream, fhe::ckks_rns_galois_kernel, fhe_ew_grid(words), 256, (const u64 *)d_in, (u64 *)d_out, words,
                  (u32)g, plan->log_n);
}

extern "C" size_t fhe_ckks_rns_galois_workspace_bytes(uint64_t n, unsigned limbs, size_t batch, unsigned count) {
    Chain c;
    if (!chain_of(n, limbs, batch, &c) || count == 0 || count > FHE_CKKS_GALOIS_MAX_COUNT) return 0;
    return (size_t)(galois_words_per_row(c) * chunk_rows(c, batch) * 8);
}

extern "C" int fhe_ckks_rns_galois_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const void *const *d_gks, const uint64_t *gs,
                                       unsigned count, unsigned key_limbs, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_rns_galois_dev";
    Chain c;
    int rc = check_chain(plans, limbs, special, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (count > FHE_CKKS_GALOIS_MAX_COUNT) return fhe_fail(FHE_E_INVALID, "%s: count=%u passes %d", who, count, FHE_CKKS_GALOIS_MAX_COUNT);
    if (batch == 0 || count == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 2ull * c.k * n * count, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_gks || !gs || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8;
    bool switched;
    if ((rc = check_switch_keys(d_gks, gs, count, false, n, key_limbs, d_out, ct_bytes * count, &switched, who)) != FHE_OK) return rc;
    if (overlaps_any(d_out, ct_bytes * count, {{d_in, ct_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the ciphertexts", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return switch_call(c, batch, galois_words_per_row(c), st, [&](u64 r0, u64 cr, u64 *W, const u64 *pinv) {
        return galois_rows(c, (const u64 *const *)d_gks, gs, count, key_limbs, pinv, (const u64 *)d_in, (u64 *)d_out, batch, r0, cr, W, st);
    });
}

// ---- plaintext linear transforms: the double-hoisted diagonal sum ---------------------------------------------------
namespace {

template <class... A>
int diagmac_launch(unsigned nout, bool carry, int L, hipStream_t st, unsigned grid, A... a) {
    const char *lab = "ckks_rns_diagmac";
#define FHE_DIAG_CASE(N) \
    case N: return carry ? launch(lab, L, st, fhe::ckks_rns_diagmac_kernel<N, true>, grid, 256, a...) : launch(lab, L, st, fhe::ckks_rns_diagmac_kernel<N, false>, grid, 256, a...)
    switch (nout) {
        FHE_DIAG_CASE(1);
        FHE_DIAG_CASE(2);
    }
#undef FHE_DIAG_CASE
    static_assert(fhe::kDiagOutputs == 2, "one case per accumulator count");
    return fhe_fail(FHE_E_INVALID, "ckks_rns_diagmac: %u outputs in one launch", nout);
}

// The diagmac launches of outputs o0 .. o0 + nout of a diagonal sum over the rows of `ct`, in groups of kDiagGroup elements.
// `extended`: the sums U' of §24 in the basis Q P, over the k + 1 targets, into the sets 0 .. nout - 1 of b's T (the digits are
// read only for an element other than 1).  Otherwise the finished sums over the k chain limbs, into the rows out0 of output o0,
// the outputs o_words apart.
int diagmac_rows(const Chain &c, const u64 *const *gks, const uint64_t *gs, unsigned count, unsigned key_limbs, const u64 *pts, unsigned o0, unsigned nout,
                 bool extended, const SwitchBufs &b, LimbRows<const u64> ct, LimbRows<u64> out0, u64 o_words, hipStream_t st) {
    const u64 n = c.n, slab = b.slab, pt_os = (u64)count * (c.k + 1) * n;
    const unsigned k = c.k;
    for (unsigned i = 0; i < (extended ? k + 1 : k); i++) {
        for (unsigned e0 = 0; e0 < count; e0 += fhe::kDiagGroup) {
            fhe::DiagGroup grp{};
            grp.count = std::min<unsigned>(fhe::kDiagGroup, count - e0);
            for (unsigned r = 0; r < grp.count; r++) {
                grp.g[r] = (u32)gs[e0 + r];
                grp.key[r] = grp.g[r] == 1 ? nullptr : gks[e0 + r] + (u64)(i < k ? i : key_limbs) * 2 * n;
                grp.pt[r] = pts + (((u64)o0 * count + e0 + r) * (k + 1) + i) * n;
            }
            u64 *dst = extended ? b.T + 2ull * i * slab : out0.of(i);
            const u64 pmod = !extended ? 1 : i < k ? c.p[k]->q % c.p[i]->q : 0;
            const int rc = diagmac_launch(nout, e0 > 0, (int)c.L, st, fhe_ew_grid(slab), extended ? b.D_of(i) : nullptr, slab, i < k ? ct.of(i) : nullptr, ct.cs, i,
                                          (u64)(key_limbs + 1) * 2 * n, pt_os, dst, extended ? slab : ct.cs, extended ? b.set : o_words, k, c.L, slab, pmod, grp,
                                          c.p[i]->mod);
            if (rc != FHE_OK) return rc;
        }
    }
    return FHE_OK;
}

// §24: rows r0 .. r0 + cr of in [k][2][batch][n] -> the same rows of out [outputs][k][2][batch][n], out_o = sum_r m_{o,r} (.)
// sigma_{g_r}(in).  `switched` (some g != 1): the digits of c1 once; per launch of up to kDiagOutputs outputs, U over the k + 1
// targets in groups of kDiagGroup elements; per output one modulus-down of U.  Otherwise the sums land in `out` and W is not used.
int diag_rows(const Chain &c, const u64 *const *gks, const uint64_t *gs, unsigned count, unsigned key_limbs, const u64 *pts, unsigned outputs, bool switched,
              const u64 *pinv, const u64 *in, u64 *out, u64 batch, u64 r0, u64 cr, u64 *W, hipStream_t st) {
    const u64 n = c.n, slab = cr * n;
    const unsigned k = c.k;
    const SwitchBufs b(W, k, std::min<unsigned>(outputs, fhe::kDiagOutputs), slab);   // set o of T is the U of a launch's output o
    const u64 o_words = 2ull * k * batch * n;
    const LimbRows<const u64> ct{in + r0 * n, 2 * batch * n, batch * n};
    auto out_rows = [&](unsigned o) { return LimbRows<u64>{out + o * o_words + r0 * n, ct.ls, ct.cs}; };
    int rc;
    if (switched && (rc = digit_rows(c, [&](unsigned limb) { return ct.of(limb) + ct.cs; }, b, cr, st)) != FHE_OK) return rc;
    for (unsigned o0 = 0; o0 < outputs; o0 += fhe::kDiagOutputs) {
        const unsigned nout = std::min<unsigned>(fhe::kDiagOutputs, outputs - o0);
        if ((rc = diagmac_rows(c, gks, gs, count, key_limbs, pts, o0, nout, switched, b, ct, out_rows(o0), o_words, st)) != FHE_OK) return rc;
        for (unsigned o = 0; switched && o < nout; o++)
            if ((rc = special_down(c, b, o, {}, out_rows(o0 + o), pinv, 0u, st)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

}  // namespace

extern "C" size_t fhe_ckks_rns_diag_workspace_bytes(uint64_t n, unsigned limbs, size_t batch, unsigned count, unsigned outputs) {
    Chain c;
    if (!chain_of(n, limbs, batch, &c) || count == 0 || count > FHE_CKKS_GALOIS_MAX_COUNT || outputs == 0 || outputs > FHE_CKKS_DIAG_MAX_OUTPUTS) return 0;
    return (size_t)(diag_words_per_row(c, outputs) * chunk_rows(c, batch) * 8);
}

extern "C" int fhe_ckks_rns_diag_sum_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const void *const *d_gks, const uint64_t *gs,
                                         unsigned count, unsigned key_limbs, const void *d_pts, unsigned outputs, const void *d_in, void *d_out, size_t batch,
                                         void *hip_stream) {
    const char *who = "fhe_ckks_rns_diag_sum_dev";
    Chain c;
    int rc = check_chain(plans, limbs, special, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (count > FHE_CKKS_GALOIS_MAX_COUNT) return fhe_fail(FHE_E_INVALID, "%s: count=%u passes %d", who, count, FHE_CKKS_GALOIS_MAX_COUNT);
    if (outputs < 1 || outputs > FHE_CKKS_DIAG_MAX_OUTPUTS) return fhe_fail(FHE_E_INVALID, "%s: outputs=%u must be in [1, %d]", who, outputs, FHE_CKKS_DIAG_MAX_OUTPUTS);
    if (batch == 0 || count == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 2ull * c.k * n * outputs, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!gs || !d_pts || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_pts) || misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8, out_bytes = ct_bytes * outputs;
    bool switched = false;
    if ((rc = check_switch_keys(d_gks, gs, count, true, n, key_limbs, d_out, out_bytes, &switched, who)) != FHE_OK) return rc;
    if (overlaps_any(d_out, out_bytes, {{d_in, ct_bytes}, {d_pts, (u64)outputs * count * (c.k + 1) * n * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the ciphertexts or the plaintexts", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return switch_call(c, batch, switched ? diag_words_per_row(c, outputs) : 0, st, [&](u64 r0, u64 cr, u64 *W, const u64 *pinv) {
        return diag_rows(c, (const u64 *const *)d_gks, gs, count, key_limbs, (const u64 *)d_pts, outputs, switched, pinv, (const u64 *)d_in, (u64 *)d_out, batch, r0, cr, W, st);
    });
}

// ---- plaintext linear transforms: the hoisted giant steps -----------------------------------------------------------
namespace {

constexpr int kCkksBsgsSlot = 13;   // fhe_workspace_get slot of fhe_ckks_rns_bsgs_dev (12 is the other entry points')

// The modulus-down by P of ONE component, the special prime's side of moddown_rows over one slab: X holds the component's
// residues modulo P in coefficients; they are lifted to the k chain limbs and transformed in E (k slabs), and
// out_i = (x_i - E_i) pinv[i] mod q_i.  The divide-and-round kernel takes two components: the slab goes to it as two halves.
int moddown_one(const Chain &c, const u64 *X, u64 *E, u64 slab, LimbRows<const u64> x, LimbRows<u64> out, const u64 *pinv, hipStream_t st) {
    int rc;
    fhe::LiftArgs a{};
    for (unsigned i = 0; i < c.k; i++) lift_target(&a, c.p[i], (u64)i * slab);
    if ((rc = lift_launch(false, X, E, slab, c.p[c.k]->q, a, c.L, st)) != FHE_OK) return rc;
    for (unsigned i = 0; i < c.k; i++)
        if ((rc = fhe_ntt_forward_dev(c.p[i], E + a.off[i], E + a.off[i], slab >> c.L, st)) != FHE_OK) return rc;
    const u64 half = slab / 2;                                       // n >= 2 divides the slab
    for (unsigned i = 0; i < c.k; i++)
        if ((rc = launch("ckks_rns_divround", (int)c.L, st, fhe::ckks_rns_divround_kernel<false>, fhe_ew_grid(slab), 256, x.of(i), half, (const u64 *)E + a.off[i], half,
                         (const u64 *)nullptr, (u64)0, out.of(i), half, half, pinv[i], c.p[i]->mod, 0u, c.L)) != FHE_OK)
            return rc;
    return FHE_OK;
}

// words of workspace per ciphertext of a chunk: the key switch of the ciphertext with kDiagOutputs sets U and the set V, and
// the digits of one giant step (its C and D) with w_a in the place of its E
u64 bsgs_words_per_row(const Chain &c) { return (SwitchBufs::words(c.k, fhe::kDiagOutputs + 1) + SwitchBufs::words(c.k, 0) - c.k) * c.n; }

// §30: rows r0 .. r0 + cr of in [k][2][batch][n] -> the same rows of out [k][2][batch][n], some element other than 1.  The
// digits of c1 once (where a baby step has a key); per pair of giant steps their inner sums U in the basis Q P; per giant step
// with a key the division by P of U's second component alone, its digits, and one accumulate launch per target into V (the
// identity: the accumulate alone); one modulus-down of V.
int bsgs_rows(const Chain &c, const u64 *const *bks, const uint64_t *bgs, unsigned babies, bool baby_switched, const u64 *const *gks, const uint64_t *ggs,
              unsigned giants, unsigned key_limbs, const u64 *pts, const u64 *pinv, const u64 *in, u64 *out, u64 batch, u64 r0, u64 cr, u64 *W, hipStream_t st) {
    const u64 n = c.n, slab = cr * n, key_stride = (u64)(key_limbs + 1) * 2 * n;
    const unsigned k = c.k, vset = fhe::kDiagOutputs;
    const SwitchBufs b(W, k, vset + 1, slab);                        // sets 0 .. vset - 1: the U of a launch's giant steps; set vset: V
    const SwitchBufs gb(b.E + 2ull * k * slab, k, 0, slab);          // the digits of w_a: they leave the ciphertext's in place
    u64 *w = gb.E;                                                   // w_a [k] slabs of evals, limb i's own digit
    const LimbRows<const u64> ct{in + r0 * n, 2 * batch * n, batch * n};
    int rc;
    if (baby_switched && (rc = digit_rows(c, [&](unsigned limb) { return ct.of(limb) + ct.cs; }, b, cr, st)) != FHE_OK) return rc;
    for (unsigned a0 = 0; a0 < giants; a0 += fhe::kDiagOutputs) {
        const unsigned nout = std::min<unsigned>(fhe::kDiagOutputs, giants - a0);
        if ((rc = diagmac_rows(c, bks, bgs, babies, key_limbs, pts, a0, nout, true, b, ct, {}, 0, st)) != FHE_OK) return rc;
        for (unsigned o = 0; o < nout; o++) {
            const unsigned a = a0 + o;
            const u32 h = (u32)ggs[a];
            if (h != 1) {
                u64 *up1 = b.TP(o) + slab;                           // U_{a,P,1}: in coefficients, in place; nothing else reads it
                if ((rc = fhe_ntt_inverse_dev(c.p[k], up1, up1, cr, st)) != FHE_OK) return rc;
                if ((rc = moddown_one(c, up1, b.E, slab, {b.T_of(o) + slab, 2 * slab, slab}, {w, slab, slab}, pinv, st)) != FHE_OK) return rc;
                if ((rc = digit_rows(c, [&](unsigned limb) { return (const u64 *)w + limb * slab; }, gb, cr, st)) != FHE_OK) return rc;
            }
            for (unsigned i = 0; i <= k; i++) {
                const bool carry = a > 0;
                auto kernel = h != 1 ? (carry ? fhe::ckks_rns_giantmac_kernel<true, true> : fhe::ckks_rns_giantmac_kernel<true, false>)
                                     : (carry ? fhe::ckks_rns_giantmac_kernel<false, true> : fhe::ckks_rns_giantmac_kernel<false, false>);
                const u64 *col = h != 1 ? gks[a] + (u64)(i < k ? i : key_limbs) * 2 * n : nullptr;
                if ((rc = launch("ckks_rns_giantmac", (int)c.L, st, kernel, fhe_ew_grid(slab), 256, (const u64 *)gb.D_of(i), slab, i < k ? (const u64 *)w + i * slab : nullptr, i,
                                 col, key_stride, (const u64 *)b.T_of(o) + 2ull * i * slab, slab, b.T_of(vset) + 2ull * i * slab, slab, k, c.L, slab, h, c.p[i]->mod)) != FHE_OK)
                    return rc;
            }
        }
    }
    return special_down(c, b, vset, {}, {out + r0 * n, ct.ls, ct.cs}, pinv, 0u, st);
}

bool bsgs_counts_ok(unsigned babies, unsigned giants) {
    return babies >= 1 && babies <= FHE_CKKS_GALOIS_MAX_COUNT && giants >= 1 && giants <= FHE_CKKS_DIAG_MAX_OUTPUTS;
}

}  // namespace

extern "C" size_t fhe_ckks_rns_bsgs_workspace_bytes(uint64_t n, unsigned limbs, size_t batch, unsigned babies, unsigned giants) {
    Chain c;
    if (!chain_of(n, limbs, batch, &c) || !bsgs_counts_ok(babies, giants)) return 0;
    return (size_t)(bsgs_words_per_row(c) * chunk_rows(c, batch) * 8);
}

extern "C" int fhe_ckks_rns_bsgs_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const void *const *d_baby_gks,
                                     const uint64_t *baby_gs, unsigned babies, const void *const *d_giant_gks, const uint64_t *giant_gs, unsigned giants,
                                     unsigned key_limbs, const void *d_pts, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_rns_bsgs_dev";
    Chain c;
    int rc = check_chain(plans, limbs, special, true, &c, who);
    if (rc != FHE_OK) return rc;
    if ((rc = check_key_limbs(c, key_limbs, who)) != FHE_OK) return rc;
    if (babies < 1 || babies > FHE_CKKS_GALOIS_MAX_COUNT) return fhe_fail(FHE_E_INVALID, "%s: babies=%u must be in [1, %d]", who, babies, FHE_CKKS_GALOIS_MAX_COUNT);
    if (giants < 1 || giants > FHE_CKKS_DIAG_MAX_OUTPUTS) return fhe_fail(FHE_E_INVALID, "%s: giants=%u must be in [1, %d]", who, giants, FHE_CKKS_DIAG_MAX_OUTPUTS);
    if (batch == 0) return FHE_OK;
    const u64 n = c.n;
    if (!mul_fits((u64)batch, 2ull * c.k * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!baby_gs || !giant_gs || !d_pts || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_pts) || misaligned8(d_in) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8;
    bool baby_switched = false, giant_switched = false;
    if ((rc = check_switch_keys(d_baby_gks, baby_gs, babies, true, n, key_limbs, d_out, ct_bytes, &baby_switched, "fhe_ckks_rns_bsgs_dev, baby steps")) != FHE_OK) return rc;
    if ((rc = check_switch_keys(d_giant_gks, giant_gs, giants, true, n, key_limbs, d_out, ct_bytes, &giant_switched, "fhe_ckks_rns_bsgs_dev, giant steps")) != FHE_OK) return rc;
    if (overlaps_any(d_out, ct_bytes, {{d_in, ct_bytes}, {d_pts, (u64)giants * babies * (c.k + 1) * n * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the ciphertexts or the plaintexts", who);
    hipStream_t st = (hipStream_t)hip_stream;
    if (!baby_switched && !giant_switched) {
        // every element the identity: the plain sum over all giants x babies products, as a diagonal sum of one output
        const std::vector<uint64_t> ones((size_t)giants * babies, 1);
        return switch_call_in(kCkksBsgsSlot, c, batch, 0, st, [&](u64 r0, u64 cr, u64 *W, const u64 *pinv) {
            return diag_rows(c, nullptr, ones.data(), giants * babies, key_limbs, (const u64 *)d_pts, 1, false, pinv, (const u64 *)d_in, (u64 *)d_out, batch, r0, cr, W, st);
        });
    }
    return switch_call_in(kCkksBsgsSlot, c, batch, bsgs_words_per_row(c), st, [&](u64 r0, u64 cr, u64 *W, const u64 *pinv) {
        return bsgs_rows(c, (const u64 *const *)d_baby_gks, baby_gs, babies, baby_switched, (const u64 *const *)d_giant_gks, giant_gs, giants, key_limbs,
                         (const u64 *)d_pts, pinv, (const u64 *)d_in, (u64 *)d_out, batch, r0, cr, W, st);
    });
}

// ---- polynomial evaluation: fused sums by public scalars ------------------------------------------------------------
namespace {

template <class... A>
int lincomb_launch(unsigned nout, bool carry, int L, hipStream_t st, unsigned grid, A... a) {
    const char *lab = "ckks_rns_lincomb";
#define FHE_LIN_CASE(N) \
    case N: return carry ? launch(lab, L, st, fhe::ckks_rns_lincomb_kernel<N, true>, grid, 256, a...) : launch(lab, L, st, fhe::ckks_rns_lincomb_kernel<N, false>, grid, 256, a...)
    switch (nout) {
        FHE_LIN_CASE(1);
        FHE_LIN_CASE(2);
        FHE_LIN_CASE(3);
        FHE_LIN_CASE(4);
    }
#undef FHE_LIN_CASE
    static_assert(fhe::kLinOutputs == 4, "one case per accumulator count");
    return fhe_fail(FHE_E_INVALID, "ckks_rns_lincomb: %u outputs in one launch", nout);
}

}  // namespace

extern "C" int fhe_ckks_rns_lincomb_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const void *const *d_cts, unsigned count, const uint64_t *w,
                                        const uint64_t *k, unsigned outputs, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_rns_lincomb_dev";
    Chain c;
    int rc = check_chain(plans, limbs, nullptr, false, &c, who);
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
    int dev;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    for (unsigned o0 = 0; o0 < outputs; o0 += fhe::kLinOutputs) {
        const unsigned nout = std::min<unsigned>(fhe::kLinOutputs, outputs - o0);
        for (unsigned i = 0; i < c.k; i++) {
            for (unsigned r0 = 0; r0 < count; r0 += fhe::kLinGroup) {
                fhe::LinGroup grp{};
                grp.count = std::min<unsigned>(fhe::kLinGroup, count - r0);
                for (unsigned r = 0; r < grp.count; r++) grp.ct[r] = (const u64 *)d_cts[r0 + r] + i * limb_words;
                for (unsigned o = 0; o < nout; o++) {
                    for (unsigned r = 0; r < grp.count; r++) grp.w[o][r] = w[((u64)(o0 + o) * count + r0 + r) * c.k + i];
                    grp.k[o] = k ? k[(u64)(o0 + o) * c.k + i] : 0;
                }
                if ((rc = lincomb_launch(nout, r0 > 0, (int)c.L, st, fhe_ew_grid(limb_words), (u64 *)d_out + ((u64)o0 * c.k + i) * limb_words, c.k * limb_words,
                                         limb_words / 2, grp, c.p[i]->mod)) != FHE_OK)
                    return rc;
            }
        }
    }
    return FHE_OK;
}

// ---- inner products: the summed tensor of ct x ct pairs, relinearised once -------------------------------------------
namespace {

// rows r0 .. r0 + cr of the `count` pairs -> their summed tensor in Dt [k][3][cr][n]: per limb, groups of kDotGroup pairs, every
// group after the first carried; w [count][k] or NULL (every weight 1)
int tensorsum_rows(const Chain &c, const void *const *d_as, const void *const *d_bs, unsigned count, const uint64_t *w, u64 batch, u64 r0, u64 *Dt, u64 cr,
                   hipStream_t st) {
    const u64 n = c.n, slab = cr * n;
    for (unsigned i = 0; i < c.k; i++) {
        for (unsigned p0 = 0; p0 < count; p0 += fhe::kDotGroup) {
            fhe::DotGroup grp{};
            grp.count = std::min<unsigned>(fhe::kDotGroup, count - p0);
            grp.cs = batch * n;
            for (unsigned r = 0; r < grp.count; r++) {
                grp.a[r] = (const u64 *)d_as[p0 + r] + ((u64)i * 2 * batch + r0) * n;
                grp.b[r] = (const u64 *)d_bs[p0 + r] + ((u64)i * 2 * batch + r0) * n;
                grp.w[r] = w ? w[(u64)(p0 + r) * c.k + i] : 1;
            }
            const bool carry = p0 > 0;
            auto kernel = w ? (carry ? fhe::ckks_rns_tensorsum_kernel<true, true> : fhe::ckks_rns_tensorsum_kernel<true, false>)
                            : (carry ? fhe::ckks_rns_tensorsum_kernel<false, true> : fhe::ckks_rns_tensorsum_kernel<false, false>);
            const int rc = launch("ckks_rns_tensorsum", (int)c.L, st, kernel, fhe_ew_grid(slab), 256, Dt + (u64)i * 3 * slab, slab, slab, grp, c.p[i]->mod);
            if (rc != FHE_OK) return rc;
        }
    }
    return FHE_OK;
}

}  // namespace

extern "C" int fhe_ckks_rns_dot_dev(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const void *d_rlk, unsigned key_limbs,
                                    const void *const *d_as, const void *const *d_bs, unsigned count, const uint64_t *w, void *d_out, size_t batch,
                                    void *hip_stream) {
    const char *who = "fhe_ckks_rns_dot_dev";
    Chain c;
    int rc = check_chain(plans, limbs, special, true, &c, who);
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
    if (!d_rlk || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_rlk) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 ct_bytes = 2ull * c.k * batch * n * 8, rlk_bytes = (u64)key_limbs * (key_limbs + 1) * 2 * n * 8;
    if (overlaps_any(d_out, ct_bytes, {{d_rlk, rlk_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key", who);
    for (unsigned r = 0; r < count; r++) {
        if (!d_as[r] || !d_bs[r]) return fhe_fail(FHE_E_NULL, "%s: an operand of pair %u is NULL", who, r);
        if (misaligned8(d_as[r]) || misaligned8(d_bs[r])) return fhe_fail(FHE_E_INVALID, "%s: the operands of pair %u must be 8-byte aligned", who, r);
        if (overlaps_any(d_out, ct_bytes, {{d_as[r], ct_bytes}, {d_bs[r], ct_bytes}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an operand of pair %u", who, r);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    return switch_call(c, batch, words_per_row(c), st, [&](u64 r0, u64 cr, u64 *Dt, const u64 *pinv) {   // Dt: the chunk's summed tensor, then relin_rows' buffers
        const int rc = tensorsum_rows(c, d_as, d_bs, count, w, batch, r0, Dt, cr, st);
        return rc != FHE_OK ? rc : relin_rows(c, (const u64 *)d_rlk, key_limbs, pinv, Dt, cr, 0, (u64 *)d_out, batch, r0, cr, Dt + 3ull * c.k * cr * n, st);
    });
}
