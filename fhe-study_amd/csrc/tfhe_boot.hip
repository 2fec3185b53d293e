// tfhe_boot.hip — TFHE bootstrapping on the device: blind rotation, sample extraction, LWE key switch
// (tfhe/src/tlwe.rs:101-161, tglwe.rs:89-118; the definitions are DESIGN.md §10's, since the reference's
// blind rotation never runs).
//
//   N = ring degree = 2^L, k = GLWE rank, all words u64 wrapping mod 2^64.
//   mod switch   w -> round(w 2N / 2^64) mod 2N = (((w >> (62 - L)) + 1) >> 1) & (2N - 1)
//   rot(x, e)    X^-e x in T64[X]/(X^N+1), e < 2N: coefficient i is (-1)^floor((i+e)/N) x[(i+e) mod N]
//   blind rot.   ACC_0 = rot(v, b~);  ACC_{j+1} = ACC_j + BSK_j [x] (rot(ACC_j, (2N - a~_j) mod 2N) - ACC_j)
//
// One step of the blind rotation where the 27-bit form applies (k = 1, 2^8 <= N <= 2^12, digit32.hip) is the external
// product's own kernel pair in its CMux modes: digit_mac32_kernel<SRC32_CMUX> forms rot(ACC, e_b) - ACC as it loads the
// digits, digit_tail32_kernel<EPI32_CMUX> adds the lift to ACC in place.  2 n_lwe + 1 launches per blind rotation.
// Other shapes with a prepared key compose rotate-difference, fhe_tggsw_external_product_prepared_dev and an add.
//
// The base-2^b gadget has entry points of its own (fhe_*_gadget_*): the same kernel pair in its gadget
// modes (SRC32_GADGET, SRC32_GCMUX), a key switch by signed digits, and an element-wise decomposition.
//
// Circuit bootstrapping: a private functional key switch TLWE -> TGLWE (all k+1 functions in one pass), a
// CMux whose TGGSW is chosen per ciphertext (SRC32_GSEL, EPI32_SEL), and the glue that runs the l_cb blind rotations of a
// batch as one gadget blind rotation over batch l_cb rows and turns them into TGGSW rows.
//
// Boolean gates: one blind rotation over a batch of mixed gates, since every gate shares the test vector;
// an init kernel forms each row's combination alpha c_x + beta c_y + o from the pool as it writes ACC_0 and the shifts.
//
// Small integers: the test vector is read only by the init kernel, so a batch in which every row names its
// own lookup table ([P] torus words, P = 2^t) and its own combination sx c_x + sy c_y + o shares one blind rotation too.
//   t = t_bits, 1 <= t <= L, Delta = 2^(63 - t): a value x in [0, P) is a TLWE of phase x Delta + e, the top bit padding (0)
//   table T -> v_T = (mask 0, body v), box = N / P, half = box / 2: v[i] = T[m] for m = (i + half) >> (L - t) < P, else -T[0]
//   a phase within half a box of x Delta gives T[x] at coefficient 0; with the padding bit set it gives -T[x - P] (negacyclic)
//   descriptor row [6] u32 (lut, x, y, sx, sy, o_hi), sx, sy int32; a scale of 0 reads nothing; a non-zero scale with an
//   index >= wires, or (bootstrap only) lut >= lut_count, makes the row invalid: nothing read, an all-zero output row
//
// Several tables from one blind rotation (the many-output bootstrap of ePrint 2021/729): nu = 0 .. min(L - t, 4),
// F = 2^nu.  The mod switch rounds to multiples of F, ms_nu(w) = ((((w >> (62 - L + nu)) + 1) >> 1) << nu) & (2N - 1), on the
// body and on every mask word; a row's lut word names the first of F consecutive tables, interleaved in the test vector:
//   v[i] = T_h[q], h = i mod F, q = (i - h + half) >> (L - t), and 0 - T_h[0] where q = P (never at nu = L - t)
// so after the one rotation coefficient h holds T_h[x] (0 - T_h[x - P] with the padding bit set).  A row is also invalid if
// lut + F > lut_count; all F of its output rows are zero.  Output [F][batch][n_lwe + 1]: function h of row m is row h batch + m.
//
// How the file is put together.  Device side: every blind rotation starts from ACC_0[m] = rot(v_m, b~_m) and shift[m][j] =
// (2N - a~_{m,j}) mod 2N, written by one element-wise body (br_init_body) over a row source that says what names row m (its
// index or its decoded descriptor), whether it is valid, what its LWE word j is and what coefficient i of its test vector is: TableRows (one table or one a row; tfhe_br_init_kernel),
// CbLevels (§12), GateRows<MUX> (§13), LutRows (§14).  Each kernel is a thin instantiation; tfhe_lut_many_init_kernel (§15)
// keeps its organisation by row and shares lut_row_ok / lut_word / lut_coeff with LutRows.  nega_sign / nega_read and rot_shift
// are the negacyclic read and the shift wherever they occur.  The LWE key switch is one tile (tlwe_ks_kernel) over a digit
// policy: BitDigit (beta = 2) and SignedDigit (§11).  extract0_word is the sample extraction at h = 0 that tfhe_cb_extract_kernel
// and tfhe_mux_extract_kernel combine; tfhe_many_extract_kernel scatters (one read, F stores) and states the rule itself.
// Host side: launch() (capi_internal.hpp) is a timed launch with its check; ks_grid, bsk_bytes, ksk_bytes and overlaps_any
// (capi_internal.hpp) are the limits and extents every entry point uses.  A gadget bootstrap is a BootShape (a BrShape and the key switch's gadget) and three stages: check_boot, boot_workspace (slots 7, 8,
// 5), and after the entry point's own init launch finish_boot (CMux steps, the extraction it names, key switch).
#include <algorithm>
#include <cstdio>

#include "capi_internal.hpp"
#include "digit32.hpp"

using fhe::u32;
using fhe::u64;

namespace fhe {

// ms_nu(w) = round(w / 2^(63 - L + nu)) 2^nu mod 2N: the mod switch with its nu low bits forced to 0, so a row's
// accumulator is rotated by a multiple of F = 2^nu and coefficients 0 .. F - 1 of the result all come from the box the
// phase fell into.  nu = 0 is the plain mod switch.
__device__ __forceinline__ u32 mod_switch_nu(u64 w, u32 L, u32 nu) {
    return (u32)(((((w >> (62u - L + nu)) + 1u) >> 1) << nu) & ((2ull << L) - 1u));
}
__device__ __forceinline__ u32 mod_switch_2n(u64 w, u32 L) { return mod_switch_nu(w, L, 0); }
// the CMux step's exponent for the mask word w: (2N - ms_nu(w)) mod 2N
__device__ __forceinline__ u32 rot_shift(u64 w, u32 L, u32 nu = 0) {
    return (u32)(((2ull << L) - mod_switch_nu(w, L, nu)) & ((2ull << L) - 1));
}
// the negacyclic extension at index j in [0, 2N): x is the word at j mod N, negated in the second half
__device__ __forceinline__ u64 nega_sign(u64 x, u64 j, u32 L) { return ((j >> L) & 1u) ? 0ull - x : x; }
__device__ __forceinline__ u64 nega_read(const u64 *__restrict__ row, u64 j, u32 L) { return nega_sign(row[j & ((1ull << L) - 1)], j, L); }

// ---- the init of a blind rotation ----------------------------------------------------------------------------------------
// ACC_0[m] = rot(v_m, b~_m) and shift[m][j] = (2N - a~_{m,j}) mod 2N, one grid-stride pass over both; an invalid row gets
// zeros and zero shifts and reads nothing.  A row source Src says where row m comes from:
//   row(m)            what names row m: its index, or its decoded descriptor
//   valid(row)        is the row valid?
//   word(row, j)      LWE word j of the row, j = n_lwe the body
//   coeff(row, c, i)  coefficient i of component c of its test vector v_m (never formed in memory)
//   BODY_ONLY         v_m has zero mask components: they are written without reading anything
//   DESCRIPTOR        row(m) reads a descriptor: it is decoded, and valid() asked, once per element ahead of the split
template <class Src>
__device__ __forceinline__ void br_init_body(const Src s, u64 *__restrict__ acc, u32 *__restrict__ shift, u32 n_lwe, u32 k1, u32 L, u64 rows) {
    const u64 N = 1ull << L, k1N = (u64)k1 * N, na = rows * k1N, total = na + rows * n_lwe;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 md = Src::DESCRIPTOR ? (i < na ? i / k1N : (i - na) / n_lwe) : 0;      // a descriptor is decoded once, ahead of the split
        const auto rd = s.row(md);
        const bool ok = Src::DESCRIPTOR ? s.valid(rd) : true;
        if (i < na) {
            const u64 m = Src::DESCRIPTOR ? md : i / k1N, r = i - m * k1N, c = r >> L;
            const auto row = Src::DESCRIPTOR ? rd : s.row(m);
            if ((Src::BODY_ONLY && c + 1 < k1) || !ok) {
                acc[i] = 0;
            } else {
                const u64 j = (r & (N - 1)) + mod_switch_2n(s.word(row, n_lwe), L);
                acc[i] = nega_sign(s.coeff(row, c, j & (N - 1)), j, L);
            }
        } else {
            const u64 q = i - na, m = Src::DESCRIPTOR ? md : q / n_lwe;
            shift[q] = ok ? rot_shift(s.word(Src::DESCRIPTOR ? rd : s.row(m), (u32)(q - m * n_lwe)), L) : 0u;
        }
    }
}

// rows of lwe [rows][n_lwe + 1]; the test vector of row m is the TGLWE at table + m tstride (all k + 1 components, mask
// rows included): tstride = 0 is one table for the batch, tstride = (k+1) N a table per row
struct TableRows {
    const u64 *__restrict__ lwe, *__restrict__ table;
    u64 tstride;
    u32 n_lwe, L;
    static constexpr bool BODY_ONLY = false, DESCRIPTOR = false;
    __device__ __forceinline__ u64 row(u64 m) const { return m; }
    __device__ __forceinline__ bool valid(u64) const { return true; }
    __device__ __forceinline__ u64 word(u64 m, u32 j) const { return lwe[m * (n_lwe + 1ull) + j]; }
    __device__ __forceinline__ u64 coeff(u64 m, u64 c, u64 i) const { return table[m * tstride + (c << L) + i]; }
};
__global__ __launch_bounds__(256) void tfhe_br_init_kernel(const u64 *__restrict__ lwe, const u64 *__restrict__ table, u64 tstride,
                                                           u64 *__restrict__ acc, u32 *__restrict__ shift, u32 n_lwe, u32 k1, u32 L, u64 batch) {
    br_init_body(TableRows{lwe, table, tstride, n_lwe, L}, acc, shift, n_lwe, k1, L, batch);
}

// the composed step (shapes outside the 27-bit form): d[b] = rot(acc[b], e_b) - acc[b], e_b = shift[b * stride]
__global__ __launch_bounds__(256) void tfhe_rotdiff_kernel(const u64 *__restrict__ acc, const u32 *__restrict__ shift, u64 stride_s,
                                                           u64 *__restrict__ d, u32 k1, u32 L, u64 batch) {
    const u64 N = 1ull << L, k1N = (u64)k1 * N, total = batch * k1N;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 b = i / k1N, r = i - b * k1N;
        const u64 j = (r & (N - 1)) + shift[b * stride_s];
        d[i] = nega_read(acc + b * k1N + (r >> L) * N, j, L) - acc[i];
    }
}
__global__ __launch_bounds__(256) void tfhe_add_kernel(u64 *__restrict__ acc, const u64 *__restrict__ p, u64 count) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) acc[i] += p[i];
}

// TGLWE::sample_extraction (tglwe.rs:89-115): out[b][c N + j] = j <= h ? a_c[h - j] : -a_c[N + h - j];  out[b][k N] = b[h]
__global__ __launch_bounds__(256) void tglwe_sample_extract_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, u32 k, u32 L, u32 h,
                                                                   u64 batch) {
    const u64 N = 1ull << L, kN = (u64)k * N, per = kN + 1, total = batch * per;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 b = i / per, r = i - b * per;
        const u64 *src = in + b * (kN + N);
        if (r == kN) {
            out[i] = src[kN + h];
        } else {
            const u64 c = r >> L, j = r & (N - 1);
            out[i] = j <= h ? src[c * N + h - j] : 0ull - src[c * N + N + h - j];
        }
    }
}

// word r of the extraction at h = 0: a_c[0] at r = c N, -a_c[N - j] at r = c N + j, and b[0] + body_add at r = k N, with
// read(at) the word at index `at` of the TGLWE (or the sum of that word over several), under one decision
template <class Read>
__device__ __forceinline__ u64 extract0_word(u64 r, u64 kN, u32 L, u64 body_add, Read read) {
    if (r == kN) return read(kN) + body_add;
    const u64 N = 1ull << L, c = r >> L, j = r & (N - 1);
    return j == 0 ? read(c * N) : 0ull - read(c * N + N - j);
}

// TLWE key switch:  out[b] = (0 .. 0, b_b) - sum_i sum_{d<l} digit_d(a_{b,i}) ksk[i][d]
// A workgroup owns KS_TB ciphertexts and KS_TH output columns: every KSK word it reads serves all KS_TB ciphertexts (the
// key is n_in l (n_out + 1) words, 331 MB at n_in = 1024, l = 64, n_out = 630).  The ciphertext words are uniform across
// the workgroup, so the digit of a (ciphertext, level) is one operation per lane.  A digit policy says what a digit is:
//   prepare(w)        the word as the digits are taken from it
//   term(w, d, kv)    digit_d(w) kv, w prepared
constexpr int KS_TB = 32, KS_TH = 64;
template <class Digit>
__global__ __launch_bounds__(KS_TH) void tlwe_ks_kernel(const u64 *__restrict__ ksk, const u64 *__restrict__ in, u64 *__restrict__ out, u32 n_in,
                                                        u32 n_out, u32 l, u64 batch, u32 cblocks, const Digit dg) {
    const u64 tile = blockIdx.x / cblocks;
    const u32 o = (blockIdx.x - (u32)tile * cblocks) * KS_TH + threadIdx.x;
    const u64 b0 = tile * KS_TB, row = (u64)n_out + 1, irow = (u64)n_in + 1;
    const u32 live = (u32)min((u64)KS_TB, batch - b0);
    const bool on = o <= n_out;
    const u64 *__restrict__ kc = ksk + (on ? o : n_out);        // idle lanes read a valid column and store nothing
    const u64 *__restrict__ src = in + b0 * irow;
    u64 acc[KS_TB];
#pragma unroll
    for (int t = 0; t < KS_TB; t++) acc[t] = 0;
    for (u32 i = 0; i < n_in; i++) {
        u64 w[KS_TB];
#pragma unroll
        for (int t = 0; t < KS_TB; t++) w[t] = dg.prepare((u32)t < live ? src[t * irow + i] : 0ull);
        const u64 *__restrict__ kr = kc + (u64)i * l * row;
        for (u32 d = 0; d < l; d++) {
            const u64 kv = kr[(u64)d * row];
#pragma unroll
            for (int t = 0; t < KS_TB; t++) acc[t] += dg.term(w[t], d, kv);
        }
    }
    if (!on) return;
#pragma unroll
    for (int t = 0; t < KS_TB; t++)
        if ((u32)t < live) out[(b0 + t) * row + o] = (o == n_out ? src[t * irow + n_in] : 0ull) - acc[t];
}

// TLWE::key_switch (tlwe.rs:101-111), beta = 2: digit_d(w) = bit l - 1 - d of w, a select of the key word
struct BitDigit {
    u32 l;
    __device__ __forceinline__ u64 prepare(u64 w) const { return w; }
    __device__ __forceinline__ u64 term(u64 w, u32 d, u64 kv) const { return ((w >> (l - 1u - d)) & 1u) ? kv : 0ull; }
};

// ---- the base-2^b gadget ----------------------------------------------------------------------------
// digit_d(w) = ((w + cadd) >> (64 - b (d+1))) & (2^b - 1)) - 2^(b-1), cadd = gadget_cadd(b, l); 1 <= b <= 64, b l <= 64
__device__ __forceinline__ u64 gadget_digit(u64 w, u64 cadd, u32 b, u32 d) {
    const u64 mask = ~0ull >> (64u - b), half = 1ull << (b - 1u);
    return ((w + cadd) >> (64u - b * (d + 1u)) & mask) - half;        // the signed digit as a wrapping u64
}

// [rows][n] words -> [rows][l][n] signed digits (i64 words)
__global__ __launch_bounds__(256) void tn_gadget_decompose_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, u32 L, u32 b, u32 l,
                                                                  u64 cadd, u64 rows) {
    const u64 N = 1ull << L, per = (u64)l << L, total = rows * per;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 r = i / per, q = i - r * per;
        const u32 d = (u32)(q >> L);
        out[i] = gadget_digit(in[(r << L) + (q & (N - 1))], cadd, b, d);
    }
}

// the key switch by signed digits: the word carries cadd, every product is a wrapping multiply by the signed digit
struct SignedDigit {
    u32 lb;
    u64 cadd;
    __device__ __forceinline__ u64 prepare(u64 w) const { return w + cadd; }
    __device__ __forceinline__ u64 term(u64 w, u32 d, u64 kv) const {
        const u64 mask = ~0ull >> (64u - lb), half = 1ull << (lb - 1u);
        return ((w >> (64u - lb * (d + 1u)) & mask) - half) * kv;
    }
};

// ---- circuit bootstrapping ---------------------------------------------------------------------------
// Private functional key switch, k = 1: out[m][r] = sum_{j <= kN} sum_{d < l} digit_d(c_m[j]) pfksk[r][j][d], r <= k, with
// c_m[kN] the body; key [(k+1)][kN+1][l][cols], cols = (k+1) N, output row (m / group, r, m % group) of [..][(k+1)][group][cols].
// A wrapping u64 GEMM tiled as tlwe_ks_kernel: a workgroup owns PF_TB ciphertexts and PF_TH columns of every
// function, so each key word is read once per tile and each digit (an SGPR: the ciphertext words are uniform) is extracted
// once per wave for all the functions.  digit = f - 2^(b-1) with the field f in [0, 2^b): sum digit key = sum f key -
// 2^(b-1) sum key, so a term is one v_mad_u64_u32 and one 32-bit multiply of the high half, and sum key is per column.
constexpr int PF_TB = 32, PF_TH = 64, PF_K1 = 2;
__global__ __launch_bounds__(PF_TH) void tlwe_private_ks_kernel(const u64 *__restrict__ key, const u64 *__restrict__ in, u64 *__restrict__ out,
                                                                u32 n_in, u32 cols, u32 lb, u32 l, u64 cadd, u64 batch, u32 group, u32 cblocks) {
    const u64 tile = blockIdx.x / cblocks;
    const u32 o = (blockIdx.x - (u32)tile * cblocks) * PF_TH + threadIdx.x;
    const u64 b0 = tile * PF_TB, irow = (u64)n_in + 1, fstride = irow * l * cols;   // fstride: one function's key
    const u32 live = (u32)min((u64)PF_TB, batch - b0);
    const bool on = o < cols;
    const u64 *__restrict__ kc = key + (on ? o : cols - 1);        // idle lanes read a valid column and store nothing
    const u64 *__restrict__ src = in + b0 * irow;
    const u32 sh0 = 64u - lb, mask = (u32)(~0ull >> (64u - lb));
    u64 acc[PF_K1][PF_TB], ksum[PF_K1];
#pragma unroll
    for (int r = 0; r < PF_K1; r++) {
        ksum[r] = 0;
#pragma unroll
        for (int t = 0; t < PF_TB; t++) acc[r][t] = 0;
    }
    for (u32 j = 0; j <= n_in; j++) {
        u64 w[PF_TB];
#pragma unroll
        for (int t = 0; t < PF_TB; t++) w[t] = ((u32)t < live ? src[t * irow + j] : 0ull) + cadd;
        const u64 *__restrict__ kr = kc + (u64)j * l * cols;
        for (u32 d = 0; d < l; d++) {
            u64 kv[PF_K1];
#pragma unroll
            for (int r = 0; r < PF_K1; r++) kv[r] = kr[r * fstride + (u64)d * cols];
            const u32 sh = sh0 - lb * d;
#pragma unroll
            for (int r = 0; r < PF_K1; r++) ksum[r] += kv[r];
#pragma unroll
            for (int t = 0; t < PF_TB; t++) {
                const u64 f = (u32)(w[t] >> sh) & mask;
#pragma unroll
                for (int r = 0; r < PF_K1; r++) acc[r][t] += f * kv[r];
            }
        }
    }
    if (!on) return;
    const u64 half = 1ull << (lb - 1u);
#pragma unroll
    for (int t = 0; t < PF_TB; t++) {
        if ((u32)t >= live) continue;
        const u64 m = b0 + t, bb = m / group, dd = m - bb * group;
#pragma unroll
        for (int r = 0; r < PF_K1; r++) out[((bb * PF_K1 + r) * group + dd) * cols + o] = acc[r][t] - half * ksum[r];
    }
}

// alpha_d = g_d(b_cb) / 2 = 2^(63 - b_cb (d+1)): the body of level d's trivial table (b_cb l_cb <= 63)
__device__ __forceinline__ u64 cb_alpha(u32 cb_b, u32 d) { return 1ull << (63u - cb_b * (d + 1u)); }

// row m = b G + d (G = l_cb) is c_b + (0 .. 0, 2^62) under v_d, the trivial table whose body is alpha_d in every coefficient
struct CbLevels {
    const u64 *__restrict__ lwe;
    u32 n_lwe, G, cb_b;
    static constexpr bool BODY_ONLY = true, DESCRIPTOR = false;
    __device__ __forceinline__ u64 row(u64 m) const { return m; }
    __device__ __forceinline__ bool valid(u64) const { return true; }
    __device__ __forceinline__ u64 word(u64 m, u32 j) const { return lwe[m / G * (n_lwe + 1ull) + j] + (j == n_lwe ? 1ull << 62 : 0ull); }
    __device__ __forceinline__ u64 coeff(u64 m, u64, u64) const { return cb_alpha(cb_b, (u32)(m % G)); }
};
__global__ __launch_bounds__(256) void tfhe_cb_init_kernel(const u64 *__restrict__ lwe, u64 *__restrict__ acc, u32 *__restrict__ shift,
                                                           u32 n_lwe, u32 k1, u32 L, u32 G, u32 cb_b, u64 rows) {
    br_init_body(CbLevels{lwe, n_lwe, G, cb_b}, acc, shift, n_lwe, k1, L, rows);
}

// T[m] = (0 .. 0, alpha_d) - E, E the extraction of ACC[m] at h = 0, d = m mod G
__global__ __launch_bounds__(256) void tfhe_cb_extract_kernel(const u64 *__restrict__ acc, u64 *__restrict__ out, u32 k, u32 L, u32 G,
                                                              u32 cb_b, u64 rows) {
    const u64 N = 1ull << L, kN = (u64)k * N, per = kN + 1, total = rows * per;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 m = i / per, r = i - m * per;
        const u64 *src = acc + m * (kN + N);
        out[i] = 0ull - extract0_word(r, kN, L, 0ull - cb_alpha(cb_b, (u32)(m % G)), [&](u64 at) { return src[at]; });
    }
}

// ---- boolean gates ------------------------------------------------------------------------------------
// bits are phases +-mu, mu = 2^61; op (alpha, beta, o / mu) in FHE_GATE_* order: AND NAND OR NOR XOR XNOR ANDNY ANDYN ORNY ORYN
constexpr u64 GATE_MU = 1ull << 61;
constexpr u32 GATE_COUNT = 10, GATE_AND = 0, GATE_ANDNY = 6;
__constant__ signed char gate_alpha[GATE_COUNT] = {1, -1, 1, -1, 2, -2, -1, 1, -1, 1};
__constant__ signed char gate_beta[GATE_COUNT] = {1, -1, 1, -1, 2, -2, 1, -1, 1, -1};
__constant__ signed char gate_o[GATE_COUNT] = {-1, 1, 1, -1, 2, -2, -1, -1, 1, 1};

// word j (j = n_lwe: the body) of alpha c_x + beta c_y + (0 .. 0, o); an op >= GATE_COUNT or an index >= wires gives 0 and
// reads nothing
__device__ __forceinline__ u64 gate_word(const u64 *__restrict__ pool, u64 wires, u32 n_lwe, u32 op, u32 x, u32 y, u32 j) {
    if (op >= GATE_COUNT || x >= wires || y >= wires) return 0;
    const u64 row = n_lwe + 1ull;
    const u64 w = (u64)(long long)gate_alpha[op] * pool[x * row + j] + (u64)(long long)gate_beta[op] * pool[y * row + j];
    return j == n_lwe ? w + (u64)(long long)gate_o[op] * GATE_MU : w;
}

// the combined rows under v = (mask 0, body mu).  MUX = false: row m is gate m, desc[m] = (op, x, y).  MUX = true: desc[b] =
// (s, a, c), row 2b is AND(s, a), row 2b + 1 ANDNY(s, c).  The combined TLWE exists only in registers.
template <bool MUX>
struct GateRows {
    const u64 *__restrict__ pool;
    u64 wires;
    const u32 *__restrict__ desc;
    u32 n_lwe;
    static constexpr bool BODY_ONLY = true, DESCRIPTOR = true;
    struct Row { u32 op, x, y; };
    __device__ __forceinline__ Row row(u64 m) const {
        if (MUX) {
            const u32 *d = desc + (m >> 1) * 3;
            return {(m & 1) ? GATE_ANDNY : GATE_AND, d[0], d[1 + (m & 1)]};
        }
        const u32 *d = desc + m * 3;
        return {d[0], d[1], d[2]};
    }
    __device__ __forceinline__ bool valid(Row) const { return true; }          // gate_word is 0 where the row names nothing
    __device__ __forceinline__ u64 word(Row g, u32 j) const { return gate_word(pool, wires, n_lwe, g.op, g.x, g.y, j); }
    __device__ __forceinline__ u64 coeff(Row, u64, u64) const { return GATE_MU; }
};
template <bool MUX>
__global__ __launch_bounds__(256) void tfhe_gate_init_kernel(const u64 *__restrict__ pool, u64 wires, const u32 *__restrict__ desc,
                                                             u64 *__restrict__ acc, u32 *__restrict__ shift, u32 n_lwe, u32 k1, u32 L, u64 rows) {
    br_init_body(GateRows<MUX>{pool, wires, desc, n_lwe}, acc, shift, n_lwe, k1, L, rows);
}

// out[b] = E[2b] + E[2b + 1] + (0 .. 0, mu), E the extraction of ACC at h = 0
__global__ __launch_bounds__(256) void tfhe_mux_extract_kernel(const u64 *__restrict__ acc, u64 *__restrict__ out, u32 k, u32 L, u64 batch) {
    const u64 N = 1ull << L, kN = (u64)k * N, per = kN + 1, total = batch * per;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 b = i / per, r = i - b * per;
        const u64 *s0 = acc + 2 * b * (kN + N);
        out[i] = extract0_word(r, kN, L, GATE_MU, [&](u64 at) { return s0[at] + s0[kN + N + at]; });
    }
}

// ---- small integers: a lookup table per row -----------------------------------------------------------
// descriptor row (lut, x, y, sx, sy, o_hi), sx and sy int32: c = sx pool[x] + sy pool[y] + (0 .. 0, o_hi 2^32).  An operand
// whose scale is 0 is never read; one with a non-zero scale and an index >= wires makes the row invalid.
constexpr u32 LUT_DESC = 6;
__device__ __forceinline__ bool lut_row_valid(const u32 *__restrict__ d, u64 wires) {
    return (d[3] == 0 || d[1] < wires) && (d[4] == 0 || d[2] < wires);
}
// word j (j = n_lwe: the body) of the combined input of a valid row
__device__ __forceinline__ u64 lut_word(const u64 *__restrict__ pool, const u32 *__restrict__ d, u32 n_lwe, u32 j) {
    const u64 row = n_lwe + 1ull;
    u64 w = j == n_lwe ? (u64)d[5] << 32 : 0ull;
    if (d[3]) w += (u64)(long long)(int)d[3] * pool[d[1] * row + j];
    if (d[4]) w += (u64)(long long)(int)d[4] * pool[d[2] * row + j];
    return w;
}

// out[m] = the combined input of descriptor row m (the lut word is not looked at); an invalid row gives zeros
__global__ __launch_bounds__(256) void tlwe_lincomb_kernel(const u64 *__restrict__ pool, u64 wires, const u32 *__restrict__ desc,
                                                           u64 *__restrict__ out, u32 n_lwe, u64 rows) {
    const u64 row = n_lwe + 1ull, total = rows * row;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 m = i / row;
        const u32 *d = desc + m * LUT_DESC;
        out[i] = lut_row_valid(d, wires) ? lut_word(pool, d, n_lwe, (u32)(i - m * row)) : 0ull;
    }
}

// a row whose lut word names the first of F consecutive tables is valid under lut_row_valid and lut + F <= lut_count (64-bit)
__device__ __forceinline__ bool lut_row_ok(const u32 *__restrict__ d, u64 wires, u64 lut_count, u64 F) {
    return (u64)d[0] + F <= lut_count && lut_row_valid(d, wires);
}
// coefficient i of the body of the test vector that interleaves tables lut .. lut + F - 1 ([P] torus words each, P = 2^t,
// F = 2^nu): T_h[q] with h = i mod F, q = (i - h + half) >> (L - t), half = N / 2P, and 0 - T_h[0] in the top half box (q = P)
__device__ __forceinline__ u64 lut_coeff(const u64 *__restrict__ luts, u32 lut, u32 t, u32 nu, u32 L, u64 i) {
    const u64 P = 1ull << t, half = ((1ull << L) >> t) >> 1, h = i & ((1ull << nu) - 1);
    const u64 q = (i - h + half) >> (L - t);
    const u64 *T = luts + (((u64)lut + h) << t);
    return q < P ? T[q] : 0ull - T[0];
}

// descriptor rows under v_T = (mask 0, body lut_coeff), T = luts[desc[m][0]], one table a row (F = 1)
struct LutRows {
    const u64 *__restrict__ pool;
    u64 wires;
    const u32 *__restrict__ desc;
    const u64 *__restrict__ luts;
    u64 lut_count;
    u32 t, n_lwe, L;
    static constexpr bool BODY_ONLY = true, DESCRIPTOR = true;
    __device__ __forceinline__ const u32 *row(u64 m) const { return desc + m * LUT_DESC; }
    __device__ __forceinline__ bool valid(const u32 *d) const { return lut_row_ok(d, wires, lut_count, 1); }
    __device__ __forceinline__ u64 word(const u32 *d, u32 j) const { return lut_word(pool, d, n_lwe, j); }
    __device__ __forceinline__ u64 coeff(const u32 *d, u64, u64 i) const { return lut_coeff(luts, d[0], t, 0, L, i); }
};
__global__ __launch_bounds__(256) void tfhe_lut_init_kernel(const u64 *__restrict__ pool, u64 wires, const u32 *__restrict__ desc,
                                                            const u64 *__restrict__ luts, u64 lut_count, u32 t, u64 *__restrict__ acc,
                                                            u32 *__restrict__ shift, u32 n_lwe, u32 k1, u32 L, u64 rows) {
    br_init_body(LutRows{pool, wires, desc, luts, lut_count, t, n_lwe, L}, acc, shift, n_lwe, k1, L, rows);
}

// ---- small integers: several tables from one blind rotation ---------------------------------------------
// LutRows at F = 2^nu tables a row and the mod switch ms_nu, organised by row: a workgroup takes a row (grid-stride over rows), so the
// descriptor, the validity, the combined body and b~ are workgroup-uniform and formed once per row; its lanes then write the
// row's k1 N accumulator words two at a time (16-byte stores) and its n_lwe shifts, both coalesced.  An invalid row
// (lut_row_ok) reads no pool or table word and writes zeros and zero shifts.
__global__ __launch_bounds__(256) void tfhe_lut_many_init_kernel(const u64 *__restrict__ pool, u64 wires, const u32 *__restrict__ desc,
                                                                 const u64 *__restrict__ luts, u64 lut_count, u32 t, u32 nu,
                                                                 u64 *__restrict__ acc, u32 *__restrict__ shift, u32 n_lwe, u32 k1, u32 L,
                                                                 u64 rows) {
    const u64 N = 1ull << L, k1N = (u64)k1 * N, body0 = k1N - N;
    for (u64 m = blockIdx.x; m < rows; m += gridDim.x) {
        const u32 *d = desc + m * LUT_DESC;
        const bool ok = lut_row_ok(d, wires, lut_count, 1ull << nu);
        const u64 bt = ok ? mod_switch_nu(lut_word(pool, d, n_lwe, n_lwe), L, nu) : 0;
        u64 *row = acc + m * k1N;
        for (u64 p = 2ull * threadIdx.x; p < k1N; p += 512) {        // N >= 2: a pair never straddles a component
            ulonglong2 v = make_ulonglong2(0, 0);
            if (ok && p >= body0) {
                u64 x[2];
#pragma unroll
                for (u32 e = 0; e < 2; e++) {
                    const u64 j = (p - body0 + e) + bt;
                    x[e] = nega_sign(lut_coeff(luts, d[0], t, nu, L, j & (N - 1)), j, L);
                }
                v = make_ulonglong2(x[0], x[1]);
            }
            *reinterpret_cast<ulonglong2 *>(row + p) = v;
        }
        for (u32 j = threadIdx.x; j < n_lwe; j += 256)
            shift[m * n_lwe + j] = ok ? rot_shift(lut_word(pool, d, n_lwe, j), L, nu) : 0u;
    }
}

// TGLWE::sample_extraction (tglwe_sample_extract_kernel's rule) at h = 0 .. F - 1 in one pass: acc [batch][(k+1)][N] ->
// out [F][batch][k N + 1], function-major.  Every mask word a_c[s] is read once and stored F times: it is coefficient
// (h - s) mod N of extraction h, negated where s > h.  The body of extraction h is b[h]: only the first F body words are read.
__global__ __launch_bounds__(256) void tfhe_many_extract_kernel(const u64 *__restrict__ acc, u64 *__restrict__ out, u32 k, u32 L, u32 nu,
                                                                u64 batch) {
    const u64 N = 1ull << L, kN = (u64)k * N, F = 1ull << nu, per = kN + F, orow = kN + 1, total = batch * per;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const u64 b = i / per, r = i - b * per;
        const u64 x = acc[b * (kN + N) + r];                             // r >= kN: body word r - kN < F
        if (r >= kN) {
            out[((r - kN) * batch + b) * orow + kN] = x;
        } else {
            const u64 c = r >> L, s = r & (N - 1);
            for (u64 h = 0; h < F; h++) out[(h * batch + b) * orow + c * N + ((h - s) & (N - 1))] = s <= h ? x : 0ull - x;
        }
    }
}

// ---- packing key switch and the bootstrap with a test vector per row -------------------------------------
// Public functional key switch TLWE -> TGLWE, `count` ciphertexts of a group packed at stride 2^ls, k = 1:
//   out_g[r][c] = [r = k] sum_i b_{g,i} [c = i stride] - sum_i sum_j sum_d sg(i, c) digit_d(a_{g,i,j}) key[j][d][r][(c - i stride) mod N]
// sg = -1 where c < i stride (X^(i stride) wraps), key [n_in][l][(k+1)][N]; ciphertext (g, i) starts at word g gstride + i istride.
// tlwe_private_ks_kernel's wrapping GEMM with a rotated key read: a workgroup owns PK_TG groups and PK_TH columns of one
// component, so the key word a lane fetches for column c - i stride serves all PK_TG groups; the ciphertext words are
// uniform (SGPRs), each field is extracted once per wave, and the sign goes on the key word, which keeps the
// f - 2^(b-1) / sum key form: a term is one v_mad_u64_u32 and one 32-bit multiply of the high half.  PK_TG = 16: the 16
// ciphertext words of a (j, i) step are 32 SGPRs and stay in SGPRs (32 groups spill them into VGPR lanes), and 16
// accumulators leave eight waves per SIMD.  A slot past the last group re-reads the last live row and stores nothing.
constexpr int PK_TG = 16, PK_TH = 64;
// the sums of one lane: acc[t] = sum f kv over (j, i, d) for the tile's group t, ksum = sum kv.  FULL: all PK_TG slots live
template <bool FULL>
__device__ __forceinline__ void packing_ks_sums(const u64 *__restrict__ kc, const u64 *__restrict__ src, u32 n_in, u32 N, u64 kstep, u32 lb, u32 l,
                                                u64 cadd, u64 gstride, u64 istride, u32 count, u32 ls, u32 live, u32 c, u64 (&acc)[PK_TG], u64 &ksum) {
    const u32 sh0 = 64u - lb, mask = (u32)(~0ull >> (64u - lb));
    for (u32 j = 0; j < n_in; j++) {
        const u64 *__restrict__ kr = kc + (u64)j * l * kstep;
        for (u32 i = 0; i < count; i++) {
            u64 w[PK_TG];
            const u64 *__restrict__ p = src + i * istride + j;
#pragma unroll
            for (int t = 0; t < PK_TG; t++) {
                w[t] = *p + cadd;
                p += FULL || (u32)t + 1u < live ? gstride : 0ull;
            }
            const u32 at = i << ls, col = (c - at) & (N - 1u);
            const bool wrap = c < at;
            for (u32 d = 0; d < l; d++) {
                const u64 kw = kr[(u64)d * kstep + col], kv = wrap ? 0ull - kw : kw;
                const u32 sh = sh0 - lb * d;
                ksum += kv;
#pragma unroll
                for (int t = 0; t < PK_TG; t++) acc[t] += (u64)((u32)(w[t] >> sh) & mask) * kv;
            }
        }
    }
}

__global__ __launch_bounds__(PK_TH) void tlwe_packing_ks_kernel(const u64 *__restrict__ key, const u64 *__restrict__ in, u64 *__restrict__ out,
                                                                u32 n_in, u32 L, u32 k1, u32 lb, u32 l, u64 cadd, u64 gstride, u64 istride,
                                                                u32 count, u32 ls, u64 groups, u32 cblocks) {
    const u64 tile = blockIdx.x / cblocks;
    const u32 cb = blockIdx.x - (u32)tile * cblocks, N = 1u << L;
    const u32 r = (cb * PK_TH) >> L, c = ((cb * PK_TH) & (N - 1u)) + threadIdx.x;     // N is a multiple of PK_TH: every lane is live
    const u64 g0 = tile * PK_TG, kstep = (u64)k1 << L;                               // kstep: one (j, d) entry of the key
    const u32 live = (u32)min((u64)PK_TG, groups - g0);
    const u64 *__restrict__ kc = key + ((u64)r << L);
    const u64 *__restrict__ src = in + g0 * gstride;
    u64 acc[PK_TG], ksum = 0;
#pragma unroll
    for (int t = 0; t < PK_TG; t++) acc[t] = 0;
    if (live == PK_TG)
        packing_ks_sums<true>(kc, src, n_in, N, kstep, lb, l, cadd, gstride, istride, count, ls, live, c, acc, ksum);
    else
        packing_ks_sums<false>(kc, src, n_in, N, kstep, lb, l, cadd, gstride, istride, count, ls, live, c, acc, ksum);
    const u64 half = 1ull << (lb - 1u);
    const u32 slot = c >> ls;
    const bool body = r + 1u == k1 && (c & ((1u << ls) - 1u)) == 0 && slot < count;   // coefficient i stride of the body holds b_{g,i}
#pragma unroll
    for (int t = 0; t < PK_TG; t++)
        if ((u32)t < live) out[(((g0 + t) * k1 + r) << L) + c] = (body ? src[t * gstride + slot * istride + n_in] : 0ull) - (acc[t] - half * ksum);
}

// out = X^-half (1 + X + .. + X^(box-1)) in on every component row, box = N >> t, half = box / 2: out[i] is the sum of the
// window in~[i + half - box + 1 .. i + half] of the negacyclic extension (in~[j + N] = -in~[j]).  A workgroup takes a row:
// the row's inclusive prefix sums S (wrapping u64) are formed in LDS, each lane scanning a chunk of N / 256 words and the
// 256 chunk totals scanned in 8 steps, and with E(j) = S[j] (0 <= j < N), S[N-1] - S[j - N] (j >= N), S[N-1] - S[j + N]
// (j < 0; E(-1) = 0) the window is E(i + half) - E(i + half - box): O(N) per row.  t = L copies the row.
__global__ __launch_bounds__(256) void tglwe_box_expand_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, u32 L, u32 t, u64 rows) {
    __shared__ u64 S[4096], part[256];
    const u32 N = 1u << L, chunk = N >> 8, box = N >> t, half = box >> 1;
    for (u64 row = blockIdx.x; row < rows; row += gridDim.x) {
        const u64 *__restrict__ src = in + (row << L);
        for (u32 i = threadIdx.x; i < N; i += 256) S[i] = src[i];
        __syncthreads();
        u64 run = 0;
        for (u32 e = 0; e < chunk; e++) {
            run += S[threadIdx.x * chunk + e];
            S[threadIdx.x * chunk + e] = run;
        }
        part[threadIdx.x] = run;
        __syncthreads();
        for (u32 step = 1; step < 256; step <<= 1) {
            const u64 add = threadIdx.x >= step ? part[threadIdx.x - step] : 0ull;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        const u64 total = part[255];
        auto E = [&](int j) -> u64 {
            const u32 m = (u32)j & (N - 1u), q = m >> (L - 8u);
            const u64 s = S[m] + (q ? part[q - 1u] : 0ull);
            return (j < 0 || j >= (int)N) ? total - s : s;
        };
        for (u32 i = threadIdx.x; i < N; i += 256) out[(row << L) + i] = E((int)(i + half)) - E((int)(i + half) - (int)box);
        __syncthreads();
    }
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

bool br_ext32_on(u64 n, unsigned k, unsigned l) { return fhe_ext32_enabled() && fhe::ext32_shape_supported(n, k, l); }

int check_br(uint64_t n, unsigned k, unsigned l, unsigned n_lwe, const char *who) {
    int rc = check_ring(n, k, who);
    if (rc != FHE_OK) return rc;
    if (l < 1 || l > 64) return fhe_fail(FHE_E_INVALID, "%s: need 1 <= l <= 64 (beta = 2)", who);
    if (n_lwe < 1) return fhe_fail(FHE_E_INVALID, "%s: n_lwe must be at least 1", who);
    if (fhe_tfhe_bsk_prepared_words(n, k, l, n_lwe) == 0)
        return fhe_fail(FHE_E_INVALID, "%s: no prepared bootstrapping key for n=%llu, k=%u, l=%u (fhe_tfhe_bsk_prepared_words is 0)", who,
                        (unsigned long long)n, k, l);
    return FHE_OK;
}

int check_ks(unsigned n_in, unsigned n_out, unsigned beta, unsigned l, const char *who) {
    if (n_in < 1 || n_out < 1) return fhe_fail(FHE_E_INVALID, "%s: need n_in, n_out >= 1", who);
    if (beta != 2) return fhe_fail(FHE_E_INVALID, "%s: only beta = 2 is supported (torus.rs:44)", who);
    if (l < 1 || l > 64) return fhe_fail(FHE_E_INVALID, "%s: need 1 <= l <= 64", who);
    return FHE_OK;
}

// ACC_0 and the shifts of `batch` rows of d_lwe: one table (tstride 0, "tfhe_br_init") or one a row ((k+1) n, "tfhe_br_rows_init")
int br_init(const char *label, uint64_t n, unsigned k, unsigned n_lwe, const void *d_lwe, const void *d_table, u64 tstride, u64 *acc, u32 *shift,
            size_t batch, hipStream_t st) {
    return launch(label, __builtin_ctzll(n), st, fhe::tfhe_br_init_kernel, fhe_ew_grid((u64)batch * ((k + 1) * n + n_lwe)), 256, d_lwe, d_table,
                  tstride, acc, shift, n_lwe, k + 1, __builtin_ctzll(n), batch);
}

// the blind rotation proper, arguments validated: ACC lives in d_out
int blind_rotation(uint64_t n, unsigned k, unsigned l, unsigned n_lwe, const void *d_bsk, const void *d_table, const void *d_lwe, void *d_out,
                   size_t batch, hipStream_t st) {
    const u32 k1 = k + 1, L = (u32)__builtin_ctzll(n);
    const u64 T = (u64)k1 * l, words = fhe_tggsw_prepared_words(n, k, l);
    u64 *acc = (u64 *)d_out;
    void *wsv = nullptr;
    int rc;
    if ((rc = fhe_workspace_get(5, (u64)batch * n_lwe * 4, st, &wsv)) != FHE_OK) return rc;
    u32 *shift = (u32 *)wsv;
    if ((rc = br_init("tfhe_br_init", n, k, n_lwe, d_lwe, d_table, 0, acc, shift, batch, st)) != FHE_OK) return rc;
    if (br_ext32_on(n, k, l)) {
        fhe::Ext32Args a{};
        if ((rc = fhe_ext32_tables(n, &a)) != FHE_OK) return rc;
        u32 parts = 1, tpp = 0;
        fhe::ext32_split(n, batch, (u32)T, &parts, &tpp);
        if ((rc = fhe_workspace_get(1, (u64)batch * parts * 2 * (2 * k1) * n * 4, st, &wsv)) != FHE_OK) return rc;
        a.k = k;
        a.src = acc; a.ct_stride = (u64)k1 * n; a.part32 = (uint32_t *)wsv; a.out = acc; a.batch = batch;
        a.l = l; a.T = (u32)T; a.parts = parts; a.tpp = tpp;
        a.shift_stride = n_lwe;
        for (unsigned j = 0; j < n_lwe; j++) {
            a.key32 = (uint32_t *)const_cast<void *>(d_bsk) + (u64)j * 2 * words;
            a.shift = shift + j;
            hipError_t e = fhe::launch_ext32_mac(a, (int)L, fhe::SRC32_CMUX, st);
            if (e == hipSuccess) e = fhe::launch_ext32_tail_cmux(a, (int)L, st);
            if (e != hipSuccess) return fhe_hip_fail(e, "digit32 CMux kernels");
        }
        return FHE_OK;
    }
    // composed step: D = rot(ACC, e) - ACC, P = BSK_j [x] D, ACC += P
    const u64 cw = (u64)batch * k1 * n;
    if ((rc = fhe_workspace_get(6, 2 * cw * 8, st, &wsv)) != FHE_OK) return rc;
    u64 *D = (u64 *)wsv, *P = D + cw;
    for (unsigned j = 0; j < n_lwe; j++) {
        if ((rc = launch("tfhe_rotdiff", L, st, fhe::tfhe_rotdiff_kernel, fhe_ew_grid(cw), 256, acc, shift + j, n_lwe, D, k1, L, batch)) != FHE_OK)
            return rc;
        if ((rc = fhe_tggsw_external_product_prepared_dev(n, k, l, (const u64 *)d_bsk + (u64)j * words, D, P, batch, st)) != FHE_OK) return rc;
        if ((rc = launch("tfhe_add", L, st, fhe::tfhe_add_kernel, fhe_ew_grid(cw), 256, acc, P, cw)) != FHE_OK) return rc;
    }
    return FHE_OK;
}

int sample_extraction(uint64_t n, unsigned k, unsigned h, const void *d_tglwe, void *d_tlwe, size_t batch, hipStream_t st) {
    const u32 L = (u32)__builtin_ctzll(n);
    return launch("tglwe_sample_extract", L, st, fhe::tglwe_sample_extract_kernel, fhe_ew_grid((u64)batch * (k * n + 1)), 256, d_tglwe, d_tlwe, k, L, h,
                  batch);
}

// the grid of tlwe_ks_kernel for `rows` inputs; 0 when it does not fit one launch
u64 ks_grid(u64 rows, unsigned n_out) {
    const u64 grid = (rows + fhe::KS_TB - 1) / fhe::KS_TB * ((n_out + 1ull + fhe::KS_TH - 1) / fhe::KS_TH);
    return grid > 0x7fffffffull ? 0 : grid;
}
u64 ksk_bytes(u64 n_in, unsigned l, unsigned n_out) { return n_in * l * (n_out + 1ull) * 8; }

// both key switches, arguments validated but for the grid: the tile with the digit policy of `name`
template <class Digit>
int key_switch_launch(const char *name, unsigned n_in, unsigned n_out, unsigned l, const Digit &dg, const void *d_ksk, const void *d_in, void *d_out,
                      size_t batch, hipStream_t st) {
    const u32 cblocks = (n_out + 1 + fhe::KS_TH - 1) / fhe::KS_TH;       // 32 bits like the kernel's column index: 0 from n_out = 2^32 - 64 on,
    const u64 grid = cblocks ? ks_grid(batch, n_out) : 0;                // an empty grid that the launch reports
    if (cblocks && grid == 0) return fhe_fail(FHE_E_INVALID, "fhe_%s_dev: batch too large for one launch", name);
    return launch(name, 0, st, fhe::tlwe_ks_kernel<Digit>, (unsigned)grid, fhe::KS_TH, d_ksk, d_in, d_out, n_in, n_out, l, batch, cblocks, dg);
}

int key_switch(unsigned n_in, unsigned n_out, unsigned l, const void *d_ksk, const void *d_in, void *d_out, size_t batch, hipStream_t st) {
    return key_switch_launch("tlwe_key_switch", n_in, n_out, l, fhe::BitDigit{l}, d_ksk, d_in, d_out, batch, st);
}

// ---- the base-2^b gadget ----
int check_gadget(unsigned log_beta, unsigned l, unsigned max_b, const char *who) {
    if (log_beta < 1 || log_beta > max_b || l < 1 || (u64)log_beta * l > 64)
        return fhe_fail(FHE_E_INVALID, "%s: need 1 <= log_beta <= %u, l >= 1, log_beta l <= 64 (log_beta=%u, l=%u)", who, max_b, log_beta, l);
    return FHE_OK;
}

int check_gext(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const char *who) {
    int rc = check_ring(n, k, who);
    if (rc == FHE_OK) rc = check_gadget(log_beta, l, 64, who);
    if (rc != FHE_OK) return rc;
    if (!fhe::ext32_gadget_supported(n, k, log_beta, l))
        return fhe_fail(FHE_E_INVALID, "%s: no gadget product for n=%llu, k=%u, log_beta=%u, l=%u (needs k = 1, 256 <= n <= 4096, "
                        "(k+1) l n (2^32-1) 2^(log_beta-1) < pA pB / 2)", who, (unsigned long long)n, k, log_beta, l);
    return FHE_OK;
}

int check_gbr(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const char *who) {
    int rc = check_gext(n, k, log_beta, l, who);
    if (rc != FHE_OK) return rc;
    if (n_lwe < 1) return fhe_fail(FHE_E_INVALID, "%s: n_lwe must be at least 1", who);
    return FHE_OK;
}

int check_gks(unsigned n_in, unsigned n_out, unsigned log_beta, unsigned l, const char *who) {
    if (n_in < 1 || n_out < 1) return fhe_fail(FHE_E_INVALID, "%s: need n_in, n_out >= 1", who);
    return check_gadget(log_beta, l, 32, who);
}

u64 gadget_tggsw_words(uint64_t n, unsigned k, unsigned l) { return (u64)2 * (k + 1) * l * (k + 1) * n; }
u64 bsk_bytes(uint64_t n, unsigned k, unsigned l, unsigned n_lwe) { return (u64)n_lwe * gadget_tggsw_words(n, k, l) * 8; }

// `keys` TGGSWs -> the two-prime layout (digit32.hip ntt32_fwd_key_kernel), whatever FHE_EXT32 says
int gadget_prepare(uint64_t n, unsigned k, unsigned l, u64 keys, const void *d_tggsw, void *d_prepared, hipStream_t st) {
    fhe::Ext32Args a{};
    int rc;
    if ((rc = fhe_ext32_tables(n, &a)) != FHE_OK) return rc;
    const u32 k1 = k + 1;
    const u64 grows = (u64)k1 * l * k1;
    a.key64 = (const u64 *)d_tggsw; a.key32 = (uint32_t *)d_prepared; a.rows = 2 * grows; a.key_k1 = k1;
    a.key_stride64 = grows * n; a.key_stride32 = 2 * a.rows * n;
    const hipError_t e = fhe::launch_ext32_key_many(a, (int)__builtin_ctzll(n), keys, st);
    return e == hipSuccess ? FHE_OK : fhe_hip_fail(e, "ntt32_fwd_key_kernel (gadget)");
}

// the mac + tail pair in a gadget mode: src rows of `batch` ciphertexts -> out (EPI32_TORUS) or ACC += (EPI32_CMUX)
int gadget_args(uint64_t n, unsigned k, unsigned log_beta, unsigned l, size_t batch, hipStream_t st, fhe::Ext32Args *a) {
    int rc;
    if ((rc = fhe_ext32_tables(n, a)) != FHE_OK) return rc;
    const u32 k1 = k + 1, T = k1 * l;
    u32 parts = 1, tpp = 0;
    fhe::ext32_gadget_split(n, batch, T, &parts, &tpp);
    void *wsv = nullptr;
    if ((rc = fhe_workspace_get(1, (u64)batch * parts * 2 * (2 * k1) * n * 4, st, &wsv)) != FHE_OK) return rc;
    a->k = k; a->log_beta = log_beta;
    a->ct_stride = (u64)k1 * n; a->part32 = (uint32_t *)wsv; a->batch = batch;
    a->l = l; a->T = T; a->parts = parts; a->tpp = tpp;
    return FHE_OK;
}

// the n_lwe gadget CMux steps of a blind rotation: ACC [batch][(k+1)][n] in place, shift [batch][n_lwe] from an init kernel
int gadget_br_steps(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk, u64 *acc, const u32 *shift,
                    size_t batch, hipStream_t st) {
    const u32 L = (u32)__builtin_ctzll(n);
    const u64 words = gadget_tggsw_words(n, k, l);
    fhe::Ext32Args a{};
    int rc;
    if ((rc = gadget_args(n, k, log_beta, l, batch, st, &a)) != FHE_OK) return rc;
    a.src = acc; a.out = acc; a.shift_stride = n_lwe;
    for (unsigned j = 0; j < n_lwe; j++) {
        a.key32 = (uint32_t *)const_cast<void *>(d_bsk) + (u64)j * 2 * words;
        a.shift = shift + j;
        hipError_t e = fhe::launch_ext32_mac(a, (int)L, fhe::SRC32_GCMUX, st);
        if (e == hipSuccess) e = fhe::launch_ext32_tail_cmux(a, (int)L, st);
        if (e != hipSuccess) return fhe_hip_fail(e, "digit32 gadget CMux kernels");
    }
    return FHE_OK;
}

int gadget_blind_rotation(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk, const void *d_table,
                          const void *d_lwe, void *d_out, size_t batch, hipStream_t st) {
    u64 *acc = (u64 *)d_out;
    void *wsv = nullptr;
    int rc;
    if ((rc = fhe_workspace_get(5, (u64)batch * n_lwe * 4, st, &wsv)) != FHE_OK) return rc;
    u32 *shift = (u32 *)wsv;
    if ((rc = br_init("tfhe_br_init", n, k, n_lwe, d_lwe, d_table, 0, acc, shift, batch, st)) != FHE_OK) return rc;
    return gadget_br_steps(n, k, log_beta, l, n_lwe, d_bsk, acc, shift, batch, st);
}

int gadget_key_switch(unsigned n_in, unsigned n_out, unsigned log_beta, unsigned l, const void *d_ksk, const void *d_in, void *d_out,
                      size_t batch, hipStream_t st) {
    return key_switch_launch("tlwe_gadget_key_switch", n_in, n_out, l, fhe::SignedDigit{log_beta, fhe::gadget_cadd(log_beta, l)}, d_ksk, d_in,
                             d_out, batch, st);
}

// ---- the stages of a gadget bootstrap: checks, workspace, and everything after the init kernel ----
struct BrShape {                                                                     // the blind rotation's part
    uint64_t n;
    unsigned k, log_beta, l, n_lwe;
    u32 k1() const { return k + 1; }
    u32 L() const { return (u32)__builtin_ctzll(n); }
    u64 kn() const { return (u64)k * n; }
    u64 init_items(u64 rows) const { return rows * (k1() * n + n_lwe); }             // what an element-wise init kernel walks
};
struct BootShape : BrShape {                                                         // and the key switch back to n_lwe
    unsigned ks_log_beta, ks_l;
};
u64 bsk_bytes(const BrShape &s) { return bsk_bytes(s.n, s.k, s.l, s.n_lwe); }
u64 ksk_bytes(const BootShape &s) { return ksk_bytes(s.kn(), s.ks_l, s.n_lwe); }
constexpr u64 kEwLimit = 0x7fffffffull * 256;                                        // items of one element-wise launch

int check_boot(const BootShape &s, const char *who) {
    const int rc = check_gbr(s.n, s.k, s.log_beta, s.l, s.n_lwe, who);
    return rc != FHE_OK ? rc : check_gks((unsigned)s.kn(), s.n_lwe, s.ks_log_beta, s.ks_l, who);
}

// the accumulators [acc_rows][(k+1)][n], the extracted rows [ext_rows][k n + 1] and the shifts [acc_rows][n_lwe]
int boot_workspace(const BrShape &s, u64 acc_rows, u64 ext_rows, hipStream_t st, u64 **acc, u64 **ext, u32 **shift) {
    int rc;
    if ((rc = fhe_workspace_get(7, acc_rows * s.k1() * s.n * 8, st, (void **)acc)) != FHE_OK) return rc;
    if ((rc = fhe_workspace_get(8, ext_rows * (s.kn() + 1) * 8, st, (void **)ext)) != FHE_OK) return rc;
    return fhe_workspace_get(5, acc_rows * s.n_lwe * 4, st, (void **)shift);
}

// after the init kernel: the §11 CMux steps over the accumulators, the extraction into ext, the key switch into d_out.
//   EXT_H0     one accumulator a row, extraction at h = 0
//   EXT_MUX    two accumulators a row, out = E[2b] + E[2b + 1] + (0 .. 0, mu)
//   EXT_MANY   extraction at h = 0 .. 2^nu - 1, function-major: 2^nu batch rows go through the key switch
enum Extraction { EXT_H0, EXT_MUX, EXT_MANY };
int finish_boot(const BootShape &s, Extraction how, unsigned nu, const void *d_bsk, const void *d_ksk, u64 *acc, const u32 *shift, u64 *ext,
                void *d_out, size_t batch, hipStream_t st) {
    const u32 L = s.L();
    int rc = gadget_br_steps(s.n, s.k, s.log_beta, s.l, s.n_lwe, d_bsk, acc, shift, (how == EXT_MUX ? 2 : 1) * batch, st);
    if (rc != FHE_OK) return rc;
    u64 ks_rows = batch;
    if (how == EXT_H0) {
        rc = sample_extraction(s.n, s.k, 0, acc, ext, batch, st);
    } else if (how == EXT_MUX) {
        rc = launch("tfhe_mux_extract", L, st, fhe::tfhe_mux_extract_kernel, fhe_ew_grid((u64)batch * (s.kn() + 1)), 256, acc, ext, s.k, L, batch);
    } else {
        ks_rows = (u64)batch << nu;
        rc = launch("tfhe_many_extract", L, st, fhe::tfhe_many_extract_kernel, fhe_ew_grid((u64)batch * (s.kn() + (1ull << nu))), 256, acc, ext, s.k,
                    L, nu, batch);
    }
    if (rc != FHE_OK) return rc;
    return gadget_key_switch((unsigned)s.kn(), s.n_lwe, s.ks_log_beta, s.ks_l, d_ksk, ext, d_out, ks_rows, st);
}

// ---- circuit bootstrapping ----
// the PFKS shape: k = 1, 2^8 <= n <= 2^12, 1 <= b <= 32, l >= 1, b l <= 64
bool pfks_shape(uint64_t n, unsigned k, unsigned log_beta, unsigned l) {
    return k == 1 && n >= 256 && n <= 4096 && (n & (n - 1)) == 0 && log_beta >= 1 && log_beta <= 32 && l >= 1 && (u64)log_beta * l <= 64;
}
u64 pfksk_words(uint64_t n, unsigned k, unsigned l) { return (u64)(k + 1) * ((u64)k * n + 1) * l * (k + 1) * n; }

int check_pfks(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const char *who) {
    int rc = check_ring(n, k, who);
    if (rc != FHE_OK) return rc;
    if (!pfks_shape(n, k, log_beta, l))
        return fhe_fail(FHE_E_INVALID, "%s: no private functional key switch for n=%llu, k=%u, log_beta=%u, l=%u (needs k = 1, "
                        "256 <= n <= 4096, 1 <= log_beta <= 32, l >= 1, log_beta l <= 64)", who, (unsigned long long)n, k, log_beta, l);
    return FHE_OK;
}

// the grid of tlwe_private_ks_kernel for `rows` inputs; 0 when it does not fit one launch
u64 pfks_grid(uint64_t n, unsigned k, u64 rows) {
    const u64 cblocks = ((u64)(k + 1) * n + fhe::PF_TH - 1) / fhe::PF_TH;
    const u64 grid = (rows + fhe::PF_TB - 1) / fhe::PF_TB * cblocks;
    return grid > 0x7fffffffull ? 0 : grid;
}

int private_key_switch(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const void *d_key, const void *d_in, void *d_out, u64 rows,
                       u32 group, hipStream_t st) {
    const u32 cols = (u32)((k + 1) * n), cblocks = (cols + fhe::PF_TH - 1) / fhe::PF_TH;
    return launch("tlwe_private_ks", __builtin_ctzll(n), st, fhe::tlwe_private_ks_kernel, (unsigned)pfks_grid(n, k, rows), fhe::PF_TH, d_key, d_in,
                  d_out, (u32)(k * n), cols, log_beta, l, fhe::gadget_cadd(log_beta, l), rows, group, cblocks);
}

}  // namespace

extern "C" size_t fhe_tfhe_bsk_prepared_words(uint64_t n, unsigned k, unsigned l, unsigned n_lwe) {
    const size_t w = fhe_tggsw_prepared_words(n, k, l);
    if (w == 0 || n_lwe == 0 || w > SIZE_MAX / n_lwe) return 0;
    return w * n_lwe;
}

extern "C" int fhe_tfhe_bsk_prepare_dev(uint64_t n, unsigned k, unsigned l, unsigned n_lwe, const void *d_bsk, void *d_prepared, void *hip_stream) {
    const char *who = "fhe_tfhe_bsk_prepare_dev";
    int rc = check_br(n, k, l, n_lwe, who);
    if (rc != FHE_OK) return rc;
    if (!d_bsk || !d_prepared) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk); REQUIRE_ALIGNED(d_prepared);
    const u64 bsk_bytes = (u64)n_lwe * (k + 1) * l * (k + 1) * n * 8;
    if (overlaps(d_bsk, bsk_bytes, d_prepared, fhe_tfhe_bsk_prepared_words(n, k, l, n_lwe) * 8))
        return fhe_fail(FHE_E_INVALID, "%s: d_prepared overlaps d_bsk", who);
    return fhe_tggsw_prepare_keys(n, k, l, n_lwe, d_bsk, d_prepared, (hipStream_t)hip_stream);
}

extern "C" int fhe_tfhe_blind_rotation_dev(uint64_t n, unsigned k, unsigned l, unsigned n_lwe, const void *d_bsk_prepared, const void *d_table,
                                           const void *d_lwe, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tfhe_blind_rotation_dev";
    int rc = check_br(n, k, l, n_lwe, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_bsk_prepared || !d_table || !d_lwe || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk_prepared); REQUIRE_ALIGNED(d_table); REQUIRE_ALIGNED(d_lwe); REQUIRE_ALIGNED(d_out);
    const u64 out_bytes = (u64)batch * (k + 1) * n * 8;
    if (overlaps_any(d_out, out_bytes, {{d_bsk_prepared, fhe_tfhe_bsk_prepared_words(n, k, l, n_lwe) * 8}, {d_table, (u64)(k + 1) * n * 8},
                                        {d_lwe, (u64)batch * (n_lwe + 1ull) * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    return blind_rotation(n, k, l, n_lwe, d_bsk_prepared, d_table, d_lwe, d_out, batch, (hipStream_t)hip_stream);
}

extern "C" int fhe_tglwe_sample_extraction_dev(uint64_t n, unsigned k, unsigned h, const void *d_tglwe, void *d_tlwe, size_t batch,
                                               void *hip_stream) {
    const char *who = "fhe_tglwe_sample_extraction_dev";
    int rc = check_ring(n, k, who);
    if (rc != FHE_OK) return rc;
    if (h >= n) return fhe_fail(FHE_E_INVALID, "%s: need h < n (h=%u, n=%llu)", who, h, (unsigned long long)n);
    if (batch == 0) return FHE_OK;
    if (!d_tglwe || !d_tlwe) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_tglwe); REQUIRE_ALIGNED(d_tlwe);
    if (overlaps(d_tlwe, (u64)batch * ((u64)k * n + 1) * 8, d_tglwe, (u64)batch * (k + 1) * n * 8))
        return fhe_fail(FHE_E_INVALID, "%s: d_tlwe overlaps d_tglwe", who);
    return sample_extraction(n, k, h, d_tglwe, d_tlwe, batch, (hipStream_t)hip_stream);
}

extern "C" int fhe_tlwe_key_switch_dev(unsigned n_in, unsigned n_out, unsigned beta, unsigned l, const void *d_ksk, const void *d_in, void *d_out,
                                       size_t batch, void *hip_stream) {
    const char *who = "fhe_tlwe_key_switch_dev";
    int rc = check_ks(n_in, n_out, beta, l, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_ksk || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_ksk); REQUIRE_ALIGNED(d_in); REQUIRE_ALIGNED(d_out);
    const u64 out_bytes = (u64)batch * (n_out + 1ull) * 8;
    if (overlaps_any(d_out, out_bytes, {{d_in, (u64)batch * (n_in + 1ull) * 8}, {d_ksk, ksk_bytes(n_in, l, n_out)}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    return key_switch(n_in, n_out, l, d_ksk, d_in, d_out, batch, (hipStream_t)hip_stream);
}

extern "C" int fhe_tfhe_bootstrap_dev(uint64_t n, unsigned k, unsigned l, unsigned n_lwe, const void *d_bsk_prepared, const void *d_table,
                                      unsigned ks_l, const void *d_ksk, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tfhe_bootstrap_dev";
    int rc = check_br(n, k, l, n_lwe, who);
    if (rc != FHE_OK) return rc;
    const u64 kn = (u64)k * n;
    if (kn > 0xffffffffull) return fhe_fail(FHE_E_INVALID, "%s: k n must fit 32 bits", who);
    if ((rc = check_ks((unsigned)kn, n_lwe, 2, ks_l, who)) != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_bsk_prepared || !d_table || !d_ksk || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk_prepared); REQUIRE_ALIGNED(d_table); REQUIRE_ALIGNED(d_ksk); REQUIRE_ALIGNED(d_in); REQUIRE_ALIGNED(d_out);
    const u64 out_bytes = (u64)batch * (n_lwe + 1ull) * 8;
    if (overlaps_any(d_out, out_bytes, {{d_bsk_prepared, fhe_tfhe_bsk_prepared_words(n, k, l, n_lwe) * 8}, {d_table, (u64)(k + 1) * n * 8},
                                        {d_ksk, ksk_bytes(kn, ks_l, n_lwe)}, {d_in, out_bytes}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    hipStream_t st = (hipStream_t)hip_stream;
    void *acc = nullptr, *ext = nullptr;
    if ((rc = fhe_workspace_get(7, (u64)batch * (k + 1) * n * 8, st, &acc)) != FHE_OK) return rc;
    if ((rc = fhe_workspace_get(8, (u64)batch * (kn + 1) * 8, st, &ext)) != FHE_OK) return rc;
    // tlwe.rs:150-161: blind rotation -> sample extraction (h = 0) -> key switch back to dimension n_lwe
    if ((rc = blind_rotation(n, k, l, n_lwe, d_bsk_prepared, d_table, d_in, acc, batch, st)) != FHE_OK) return rc;
    if ((rc = sample_extraction(n, k, 0, acc, ext, batch, st)) != FHE_OK) return rc;
    return key_switch((unsigned)kn, n_lwe, ks_l, d_ksk, ext, d_out, batch, st);
}

// ---- the base-2^b gadget ------------------------------------------------------------------------------
extern "C" int fhe_tn_gadget_decompose_dev(uint64_t n, unsigned log_beta, unsigned l, const void *d_a, void *d_out, size_t rows,
                                           void *hip_stream) {
    const char *who = "fhe_tn_gadget_decompose_dev";
    int rc = check_ring(n, 1, who);
    if (rc == FHE_OK) rc = check_gadget(log_beta, l, 64, who);
    if (rc != FHE_OK) return rc;
    if (rows == 0) return FHE_OK;
    if (!d_a || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_a); REQUIRE_ALIGNED(d_out);
    if ((u64)rows > (~0ull >> 7) / ((u64)l * n)) return fhe_fail(FHE_E_INVALID, "%s: rows too large", who);
    if (overlaps(d_out, (u64)rows * l * n * 8, d_a, (u64)rows * n * 8)) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps d_a", who);
    hipStream_t st = (hipStream_t)hip_stream;
    const u32 L = (u32)__builtin_ctzll(n);
    return launch("tn_gadget_decompose", L, st, fhe::tn_gadget_decompose_kernel, fhe_ew_grid((u64)rows * l * n), 256, d_a, d_out, L, log_beta, l,
                  fhe::gadget_cadd(log_beta, l), rows);
}

extern "C" size_t fhe_tggsw_gadget_prepared_words(uint64_t n, unsigned k, unsigned log_beta, unsigned l) {
    return fhe::ext32_gadget_supported(n, k, log_beta, l) ? (size_t)gadget_tggsw_words(n, k, l) : 0;
}

extern "C" int fhe_tggsw_gadget_prepare_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const void *d_tggsw, void *d_prepared,
                                            void *hip_stream) {
    const char *who = "fhe_tggsw_gadget_prepare_dev";
    int rc = check_gext(n, k, log_beta, l, who);
    if (rc != FHE_OK) return rc;
    if (!d_tggsw || !d_prepared) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_tggsw); REQUIRE_ALIGNED(d_prepared);
    const u64 w = gadget_tggsw_words(n, k, l);
    if (overlaps(d_tggsw, w / 2 * 8, d_prepared, w * 8)) return fhe_fail(FHE_E_INVALID, "%s: d_prepared overlaps d_tggsw", who);
    return gadget_prepare(n, k, l, 1, d_tggsw, d_prepared, (hipStream_t)hip_stream);
}

extern "C" int fhe_tggsw_gadget_external_product_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const void *d_prepared,
                                                     const void *d_tglwe, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tggsw_gadget_external_product_dev";
    int rc = check_gext(n, k, log_beta, l, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_prepared || !d_tglwe || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_prepared); REQUIRE_ALIGNED(d_tglwe); REQUIRE_ALIGNED(d_out);
    const u64 ct_bytes = (u64)batch * (k + 1) * n * 8;
    if (overlaps(d_out, ct_bytes, d_tglwe, ct_bytes) || overlaps(d_out, ct_bytes, d_prepared, gadget_tggsw_words(n, k, l) * 8))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    hipStream_t st = (hipStream_t)hip_stream;
    fhe::Ext32Args a{};
    if ((rc = gadget_args(n, k, log_beta, l, batch, st, &a)) != FHE_OK) return rc;
    a.key32 = (uint32_t *)const_cast<void *>(d_prepared);
    a.src = (const u64 *)d_tglwe; a.out = (u64 *)d_out;
    const int L = (int)__builtin_ctzll(n);
    hipError_t e = fhe::launch_ext32_mac(a, L, fhe::SRC32_GADGET, st);
    if (e == hipSuccess) e = fhe::launch_ext32_tail(a, L, st);
    return e == hipSuccess ? FHE_OK : fhe_hip_fail(e, "digit32 gadget kernels");
}

extern "C" size_t fhe_tfhe_gadget_bsk_prepared_words(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe) {
    const size_t w = fhe_tggsw_gadget_prepared_words(n, k, log_beta, l);
    if (w == 0 || n_lwe == 0 || w > SIZE_MAX / n_lwe) return 0;
    return w * n_lwe;
}

extern "C" int fhe_tfhe_gadget_bsk_prepare_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk,
                                               void *d_prepared, void *hip_stream) {
    const char *who = "fhe_tfhe_gadget_bsk_prepare_dev";
    int rc = check_gbr(n, k, log_beta, l, n_lwe, who);
    if (rc != FHE_OK) return rc;
    if (!d_bsk || !d_prepared) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk); REQUIRE_ALIGNED(d_prepared);
    const u64 w = (u64)n_lwe * gadget_tggsw_words(n, k, l);
    if (overlaps(d_bsk, w / 2 * 8, d_prepared, w * 8)) return fhe_fail(FHE_E_INVALID, "%s: d_prepared overlaps d_bsk", who);
    return gadget_prepare(n, k, l, n_lwe, d_bsk, d_prepared, (hipStream_t)hip_stream);
}

extern "C" int fhe_tfhe_gadget_blind_rotation_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe,
                                                  const void *d_bsk_prepared, const void *d_table, const void *d_lwe, void *d_out,
                                                  size_t batch, void *hip_stream) {
    const char *who = "fhe_tfhe_gadget_blind_rotation_dev";
    int rc = check_gbr(n, k, log_beta, l, n_lwe, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_bsk_prepared || !d_table || !d_lwe || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk_prepared); REQUIRE_ALIGNED(d_table); REQUIRE_ALIGNED(d_lwe); REQUIRE_ALIGNED(d_out);
    const u64 out_bytes = (u64)batch * (k + 1) * n * 8;
    if (overlaps_any(d_out, out_bytes, {{d_bsk_prepared, bsk_bytes(n, k, l, n_lwe)}, {d_table, (u64)(k + 1) * n * 8},
                                        {d_lwe, (u64)batch * (n_lwe + 1ull) * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    return gadget_blind_rotation(n, k, log_beta, l, n_lwe, d_bsk_prepared, d_table, d_lwe, d_out, batch, (hipStream_t)hip_stream);
}

extern "C" int fhe_tlwe_gadget_key_switch_dev(unsigned n_in, unsigned n_out, unsigned log_beta, unsigned l, const void *d_ksk,
                                              const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tlwe_gadget_key_switch_dev";
    int rc = check_gks(n_in, n_out, log_beta, l, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_ksk || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_ksk); REQUIRE_ALIGNED(d_in); REQUIRE_ALIGNED(d_out);
    const u64 out_bytes = (u64)batch * (n_out + 1ull) * 8;
    if (overlaps_any(d_out, out_bytes, {{d_in, (u64)batch * (n_in + 1ull) * 8}, {d_ksk, ksk_bytes(n_in, l, n_out)}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    return gadget_key_switch(n_in, n_out, log_beta, l, d_ksk, d_in, d_out, batch, (hipStream_t)hip_stream);
}

namespace {
// fhe_tfhe_gadget_bootstrap_dev (table_rows = 0: one table) and fhe_tfhe_gadget_bootstrap_rows_dev (table_rows = 1: d_table holds
// [batch][(k+1)][n]): init -> the CMux steps -> extraction at h = 0 -> gadget key switch, 2 n_lwe + 3 launches
int table_bootstrap(const char *who, const char *init_label, const BootShape &s, const void *d_bsk_prepared, const void *d_table, u64 table_rows,
                    const void *d_ksk, const void *d_in, void *d_out, size_t batch, hipStream_t st) {
    int rc = check_boot(s, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_bsk_prepared || !d_table || !d_ksk || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk_prepared);
    if (fhe_misaligned(d_table))                                        // REQUIRE_ALIGNED under the entry point's name for the argument
        return fhe_fail(FHE_E_INVALID, "%s must be 16-byte aligned (got %p)", table_rows ? "d_tables" : "d_table", d_table);
    REQUIRE_ALIGNED(d_ksk); REQUIRE_ALIGNED(d_in); REQUIRE_ALIGNED(d_out);
    const u64 out_bytes = (u64)batch * (s.n_lwe + 1ull) * 8, table_bytes = (u64)s.k1() * s.n * 8;
    if (overlaps_any(d_out, out_bytes, {{d_bsk_prepared, bsk_bytes(s)}, {d_table, table_rows ? (u64)batch * table_bytes : table_bytes},
                                        {d_ksk, ksk_bytes(s)}, {d_in, out_bytes}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    u64 *acc = nullptr, *ext = nullptr;
    u32 *shift = nullptr;
    if ((rc = boot_workspace(s, batch, batch, st, &acc, &ext, &shift)) != FHE_OK) return rc;
    if ((rc = br_init(init_label, s.n, s.k, s.n_lwe, d_in, d_table, table_rows * s.k1() * s.n, acc, shift, batch, st)) != FHE_OK) return rc;
    return finish_boot(s, EXT_H0, 0, d_bsk_prepared, d_ksk, acc, shift, ext, d_out, batch, st);
}
}  // namespace

extern "C" int fhe_tfhe_gadget_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                                             const void *d_table, unsigned ks_log_beta, unsigned ks_l, const void *d_ksk, const void *d_in,
                                             void *d_out, size_t batch, void *hip_stream) {
    return table_bootstrap("fhe_tfhe_gadget_bootstrap_dev", "tfhe_br_init", {n, k, log_beta, l, n_lwe, ks_log_beta, ks_l}, d_bsk_prepared, d_table, 0,
                           d_ksk, d_in, d_out, batch, (hipStream_t)hip_stream);
}

// ---- circuit bootstrapping ------------------------------------------------------------------------------
extern "C" size_t fhe_tfhe_pfksk_words(uint64_t n, unsigned k, unsigned log_beta, unsigned l) {
    return pfks_shape(n, k, log_beta, l) ? (size_t)pfksk_words(n, k, l) : 0;
}

extern "C" int fhe_tlwe_gadget_private_key_switch_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, const void *d_pfksk,
                                                      const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tlwe_gadget_private_key_switch_dev";
    int rc = check_pfks(n, k, log_beta, l, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!d_pfksk || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_pfksk); REQUIRE_ALIGNED(d_in); REQUIRE_ALIGNED(d_out);
    if (pfks_grid(n, k, batch) == 0) return fhe_fail(FHE_E_INVALID, "%s: batch too large for one launch", who);
    const u64 out_bytes = (u64)batch * (k + 1) * (k + 1) * n * 8;
    if (overlaps(d_out, out_bytes, d_in, (u64)batch * ((u64)k * n + 1) * 8) || overlaps(d_out, out_bytes, d_pfksk, pfksk_words(n, k, l) * 8))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    return private_key_switch(n, k, log_beta, l, d_pfksk, d_in, d_out, batch, 1, (hipStream_t)hip_stream);
}

extern "C" int fhe_tggsw_gadget_prepare_many_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, size_t count, const void *d_tggsw,
                                                 void *d_prepared, void *hip_stream) {
    const char *who = "fhe_tggsw_gadget_prepare_many_dev";
    int rc = check_gext(n, k, log_beta, l, who);
    if (rc != FHE_OK) return rc;
    if (count == 0) return FHE_OK;
    if (!d_tggsw || !d_prepared) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_tggsw); REQUIRE_ALIGNED(d_prepared);
    const u64 w = gadget_tggsw_words(n, k, l);
    if ((u64)count > (~0ull >> 4) / w) return fhe_fail(FHE_E_INVALID, "%s: count too large", who);
    if (overlaps(d_tggsw, count * (w / 2) * 8, d_prepared, count * w * 8)) return fhe_fail(FHE_E_INVALID, "%s: d_prepared overlaps d_tggsw", who);
    return gadget_prepare(n, k, l, count, d_tggsw, d_prepared, (hipStream_t)hip_stream);
}

extern "C" int fhe_tggsw_gadget_cmux_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, size_t count, const void *d_prepared,
                                         const void *d_idx, const void *d_c0, const void *d_c1, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tggsw_gadget_cmux_dev";
    int rc = check_gext(n, k, log_beta, l, who);
    if (rc != FHE_OK) return rc;
    if (count < 1 || count > 0xffffffffull) return fhe_fail(FHE_E_INVALID, "%s: need 1 <= count < 2^32 (count=%llu)", who, (unsigned long long)count);
    const u64 w = gadget_tggsw_words(n, k, l);
    if ((u64)count > (~0ull >> 4) / w) return fhe_fail(FHE_E_INVALID, "%s: count too large", who);
    if (batch == 0) return FHE_OK;
    if (!d_prepared || !d_idx || !d_c0 || !d_c1 || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_prepared); REQUIRE_ALIGNED(d_idx); REQUIRE_ALIGNED(d_c0); REQUIRE_ALIGNED(d_c1); REQUIRE_ALIGNED(d_out);
    const u64 ct_bytes = (u64)batch * (k + 1) * n * 8;
    if (overlaps(d_out, ct_bytes, d_c0, ct_bytes) || overlaps(d_out, ct_bytes, d_c1, ct_bytes) || overlaps(d_out, ct_bytes, d_prepared, count * w * 8) ||
        overlaps(d_out, ct_bytes, d_idx, (u64)batch * 4))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    hipStream_t st = (hipStream_t)hip_stream;
    fhe::Ext32Args a{};
    if ((rc = gadget_args(n, k, log_beta, l, batch, st, &a)) != FHE_OK) return rc;
    a.key32 = (uint32_t *)const_cast<void *>(d_prepared); a.key_stride32 = 2 * w; a.sel_count = (uint32_t)count;
    a.sel = (const uint32_t *)d_idx; a.shift_stride = 1;
    a.src = (const u64 *)d_c0; a.src1 = (const u64 *)d_c1; a.out = (u64 *)d_out;
    const int L = (int)__builtin_ctzll(n);
    hipError_t e = fhe::launch_ext32_mac(a, L, fhe::SRC32_GSEL, st);
    if (e == hipSuccess) e = fhe::launch_ext32_tail_sel(a, L, st);
    return e == hipSuccess ? FHE_OK : fhe_hip_fail(e, "digit32 gadget CMux (selector per ciphertext) kernels");
}

extern "C" int fhe_tfhe_circuit_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                                              unsigned cb_log_beta, unsigned cb_l, unsigned pf_log_beta, unsigned pf_l, const void *d_pfksk,
                                              const void *d_lwe, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tfhe_circuit_bootstrap_dev";
    int rc = check_gbr(n, k, log_beta, l, n_lwe, who);
    if (rc == FHE_OK) rc = check_gext(n, k, cb_log_beta, cb_l, who);
    if (rc == FHE_OK) rc = check_pfks(n, k, pf_log_beta, pf_l, who);
    if (rc != FHE_OK) return rc;
    if ((u64)cb_log_beta * cb_l > 63)
        return fhe_fail(FHE_E_INVALID, "%s: need cb_log_beta cb_l <= 63 (alpha = g / 2 of the last level must be a word)", who);
    if (batch == 0) return FHE_OK;
    if (!d_bsk_prepared || !d_pfksk || !d_lwe || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk_prepared); REQUIRE_ALIGNED(d_pfksk); REQUIRE_ALIGNED(d_lwe); REQUIRE_ALIGNED(d_out);
    const u64 rows = (u64)batch * cb_l;
    if ((u64)batch > 0xffffffffull || pfks_grid(n, k, rows) == 0 || rows * (k + 1) * n > kEwLimit)
        return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    const u64 out_bytes = rows * (k + 1) * (k + 1) * n * 8;
    if (overlaps_any(d_out, out_bytes, {{d_bsk_prepared, bsk_bytes(n, k, l, n_lwe)}, {d_pfksk, pfksk_words(n, k, pf_l) * 8},
                                        {d_lwe, (u64)batch * (n_lwe + 1ull) * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps an input", who);
    hipStream_t st = (hipStream_t)hip_stream;
    const BrShape s{n, k, log_beta, l, n_lwe};                           // no LWE key switch: the rows go through the private one
    const u32 L = s.L();
    u64 *acc = nullptr, *tv = nullptr;
    u32 *shift = nullptr;
    if ((rc = boot_workspace(s, rows, rows, st, &acc, &tv, &shift)) != FHE_OK) return rc;
    // the l_cb blind rotations of every input as one blind rotation over batch l_cb rows (row b l_cb + d: level d)
    if ((rc = launch("tfhe_cb_init", L, st, fhe::tfhe_cb_init_kernel, fhe_ew_grid(s.init_items(rows)), 256, d_lwe, acc, shift, n_lwe, s.k1(), L, cb_l,
                     cb_log_beta, rows)) != FHE_OK)
        return rc;
    if ((rc = gadget_br_steps(n, k, log_beta, l, n_lwe, d_bsk_prepared, acc, shift, rows, st)) != FHE_OK) return rc;
    if ((rc = launch("tfhe_cb_extract", L, st, fhe::tfhe_cb_extract_kernel, fhe_ew_grid(rows * (s.kn() + 1)), 256, acc, tv, k, L, cb_l, cb_log_beta,
                     rows)) != FHE_OK)
        return rc;
    // TGGSW row (r, d) = PFKS_r(T_d): the key switch writes [batch][(k+1)][l_cb][(k+1)][n] directly
    return private_key_switch(n, k, pf_log_beta, pf_l, d_pfksk, tv, d_out, rows, cb_l, st);
}

// ---- boolean gates ---------------------------------------------------------------------------------------
static_assert(fhe::GATE_COUNT == FHE_GATE_COUNT && fhe::GATE_AND == FHE_GATE_AND && fhe::GATE_ANDNY == FHE_GATE_ANDNY, "gate codes");

namespace {
// gate init -> the §11 CMux steps over `rows` rows -> extraction (gate: h = 0; MUX: the fused pair sum) -> key switch into d_out
int gate_entry(bool mux, uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk_prepared, unsigned ks_log_beta,
               unsigned ks_l, const void *d_ksk, const void *d_pool, size_t wires, const void *d_desc, void *d_out, size_t batch, void *hip_stream) {
    const char *who = mux ? "fhe_tfhe_gate_mux_dev" : "fhe_tfhe_gate_bootstrap_dev";
    const BootShape s{n, k, log_beta, l, n_lwe, ks_log_beta, ks_l};
    int rc = check_boot(s, who);
    if (rc != FHE_OK) return rc;
    if (wires < 1) return fhe_fail(FHE_E_INVALID, "%s: need wires >= 1", who);
    if (batch == 0) return FHE_OK;
    if (!d_bsk_prepared || !d_ksk || !d_pool || !d_desc || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk_prepared); REQUIRE_ALIGNED(d_ksk); REQUIRE_ALIGNED(d_pool); REQUIRE_ALIGNED(d_desc); REQUIRE_ALIGNED(d_out);
    const u64 rows = (mux ? 2ull : 1ull) * batch;
    if ((u64)batch > 0xffffffffull || s.init_items(rows) > kEwLimit || ks_grid(batch, n_lwe) == 0)
        return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (overlaps_any(d_out, (u64)batch * (n_lwe + 1ull) * 8, {{d_bsk_prepared, bsk_bytes(s)}, {d_ksk, ksk_bytes(s)}, {d_desc, (u64)batch * 3 * 4}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps a key or the descriptors", who);
    hipStream_t st = (hipStream_t)hip_stream;
    u64 *acc = nullptr, *ext = nullptr;
    u32 *shift = nullptr;
    if ((rc = boot_workspace(s, rows, batch, st, &acc, &ext, &shift)) != FHE_OK) return rc;
    if ((rc = launch_named(mux ? "tfhe_mux_init" : "tfhe_gate_init", "tfhe_gate_init_kernel", s.L(), st,
                     mux ? fhe::tfhe_gate_init_kernel<true> : fhe::tfhe_gate_init_kernel<false>, fhe_ew_grid(s.init_items(rows)), 256, d_pool, wires,
                     d_desc, acc, shift, n_lwe, s.k1(), s.L(), rows)) != FHE_OK)
        return rc;
    return finish_boot(s, mux ? EXT_MUX : EXT_H0, 0, d_bsk_prepared, d_ksk, acc, shift, ext, d_out, batch, st);
}
}  // namespace

extern "C" int fhe_tfhe_gate_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                                           unsigned ks_log_beta, unsigned ks_l, const void *d_ksk, const void *d_pool, size_t wires, const void *d_gates,
                                           void *d_out, size_t batch, void *hip_stream) {
    return gate_entry(false, n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, d_pool, wires, d_gates, d_out, batch, hip_stream);
}

extern "C" int fhe_tfhe_gate_mux_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                                     unsigned ks_log_beta, unsigned ks_l, const void *d_ksk, const void *d_pool, size_t wires, const void *d_sel,
                                     void *d_out, size_t batch, void *hip_stream) {
    return gate_entry(true, n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, d_pool, wires, d_sel, d_out, batch, hip_stream);
}

// ---- small integers: a lookup table per row -----------------------------------------------------------------
static_assert(fhe::LUT_DESC == 6, "descriptor row (lut, x, y, sx, sy, o_hi)");

namespace {
// what both calls ask of the pool, the descriptors and d_out, overlaps aside; out_bytes = batch (n_lwe + 1) 8 on success
int check_lut_rows(unsigned n_lwe, const void *d_pool, size_t wires, const void *d_desc, void *d_out, size_t batch, const char *who,
                   u64 *out_bytes) {
    if (wires < 1 || batch < 1) return fhe_fail(FHE_E_INVALID, "%s: need wires >= 1 and batch >= 1", who);
    const u64 row_bytes = (n_lwe + 1ull) * 8;
    if ((u64)batch > 0xffffffffull || (u64)wires > (~0ull >> 1) / row_bytes || (u64)batch * (n_lwe + 1ull) > kEwLimit)
        return fhe_fail(FHE_E_INVALID, "%s: batch or wires too large", who);
    if (!d_pool || !d_desc || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_pool); REQUIRE_ALIGNED(d_desc); REQUIRE_ALIGNED(d_out);
    *out_bytes = (u64)batch * row_bytes;
    return FHE_OK;
}

// fhe_tfhe_lut_bootstrap_dev (many = false, nu = 0: tfhe_lut_init, extraction at h = 0) and fhe_tfhe_lut_many_bootstrap_dev (the row-organised
// init, extraction at h = 0 .. F - 1, F = 2^nu, d_out [F][batch][n_lwe + 1]): init -> the CMux steps -> extraction -> one key switch over the
// F batch extracted rows, 2 n_lwe + 3 launches whatever the mix of tables and whatever nu is
int lut_entry(bool many, const BootShape &s, const void *d_bsk_prepared, const void *d_ksk, unsigned t_bits, unsigned nu, const void *d_luts,
              size_t lut_count, const void *d_pool, size_t wires, const void *d_desc, void *d_out, size_t batch, hipStream_t st) {
    const char *who = many ? "fhe_tfhe_lut_many_bootstrap_dev" : "fhe_tfhe_lut_bootstrap_dev";
    int rc = check_boot(s, who);
    if (rc != FHE_OK) return rc;
    const u32 L = s.L(), n_lwe = s.n_lwe;
    if (t_bits < 1 || t_bits > L) return fhe_fail(FHE_E_INVALID, "%s: need 1 <= t_bits <= log2 n (t_bits=%u, n=%llu)", who, t_bits, (unsigned long long)s.n);
    if (nu > 4 || nu > L - t_bits)
        return fhe_fail(FHE_E_INVALID, "%s: need nu <= min(log2 n - t_bits, 4) (nu=%u, t_bits=%u, n=%llu)", who, nu, t_bits, (unsigned long long)s.n);
    if (lut_count < 1 || (u64)lut_count > 0xffffffffull)
        return fhe_fail(FHE_E_INVALID, "%s: need 1 <= lut_count < 2^32 (lut_count=%llu)", who, (unsigned long long)lut_count);
    u64 row_bytes = 0;                                                  // check_lut_rows: one function's slice, batch rows
    if ((rc = check_lut_rows(n_lwe, d_pool, wires, d_desc, d_out, batch, who, &row_bytes)) != FHE_OK) return rc;
    if (!d_bsk_prepared || !d_ksk || !d_luts) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_bsk_prepared); REQUIRE_ALIGNED(d_ksk); REQUIRE_ALIGNED(d_luts);
    const u64 F = 1ull << nu, frows = F * (u64)batch;                   // the extraction and the key switch see F batch rows
    if (s.init_items(batch) > kEwLimit || frows > 0xffffffffull || frows * (s.kn() + 1) > kEwLimit || ks_grid(frows, n_lwe) == 0)
        return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (overlaps_any(d_out, F * row_bytes, {{d_bsk_prepared, bsk_bytes(s)}, {d_ksk, ksk_bytes(s)}, {d_luts, ((u64)lut_count << t_bits) * 8},
                                            {d_desc, (u64)batch * fhe::LUT_DESC * 4}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps a key, the tables or the descriptors", who);
    u64 *acc = nullptr, *ext = nullptr;
    u32 *shift = nullptr;
    if ((rc = boot_workspace(s, batch, frows, st, &acc, &ext, &shift)) != FHE_OK) return rc;
    rc = many ? launch("tfhe_lut_many_init", L, st, fhe::tfhe_lut_many_init_kernel, (unsigned)std::min<u64>(batch, 256 * 16), 256, d_pool, wires, d_desc,
                       d_luts, lut_count, t_bits, nu, acc, shift, n_lwe, s.k1(), L, batch)
              : launch("tfhe_lut_init", L, st, fhe::tfhe_lut_init_kernel, fhe_ew_grid(s.init_items(batch)), 256, d_pool, wires, d_desc, d_luts, lut_count,
                       t_bits, acc, shift, n_lwe, s.k1(), L, batch);
    if (rc != FHE_OK) return rc;
    return finish_boot(s, many ? EXT_MANY : EXT_H0, nu, d_bsk_prepared, d_ksk, acc, shift, ext, d_out, batch, st);
}
}  // namespace

extern "C" int fhe_tlwe_lincomb_dev(unsigned n_lwe, const void *d_pool, size_t wires, const void *d_desc, void *d_out, size_t batch,
                                    void *hip_stream) {
    const char *who = "fhe_tlwe_lincomb_dev";
    if (n_lwe < 1) return fhe_fail(FHE_E_INVALID, "%s: n_lwe must be at least 1", who);
    u64 out_bytes = 0;
    int rc = check_lut_rows(n_lwe, d_pool, wires, d_desc, d_out, batch, who, &out_bytes);
    if (rc != FHE_OK) return rc;
    if (overlaps(d_out, out_bytes, d_desc, (u64)batch * fhe::LUT_DESC * 4)) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the descriptors", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return launch("tlwe_lincomb", 0, st, fhe::tlwe_lincomb_kernel, fhe_ew_grid((u64)batch * (n_lwe + 1ull)), 256, d_pool, wires, d_desc, d_out, n_lwe,
                  batch);
}

extern "C" int fhe_tfhe_lut_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                                          unsigned ks_log_beta, unsigned ks_l, const void *d_ksk, unsigned t_bits, const void *d_luts,
                                          size_t lut_count, const void *d_pool, size_t wires, const void *d_desc, void *d_out, size_t batch,
                                          void *hip_stream) {
    return lut_entry(false, {n, k, log_beta, l, n_lwe, ks_log_beta, ks_l}, d_bsk_prepared, d_ksk, t_bits, 0, d_luts, lut_count, d_pool, wires, d_desc,
                     d_out, batch, (hipStream_t)hip_stream);
}

// ---- small integers: several tables from one blind rotation ----------------------------------------------------
extern "C" int fhe_tfhe_lut_many_bootstrap_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                                               unsigned ks_log_beta, unsigned ks_l, const void *d_ksk, unsigned t_bits, unsigned nu,
                                               const void *d_luts, size_t lut_count, const void *d_pool, size_t wires, const void *d_desc,
                                               void *d_out, size_t batch, void *hip_stream) {
    return lut_entry(true, {n, k, log_beta, l, n_lwe, ks_log_beta, ks_l}, d_bsk_prepared, d_ksk, t_bits, nu, d_luts, lut_count, d_pool, wires, d_desc,
                     d_out, batch, (hipStream_t)hip_stream);
}

// ---- packing key switch and the bootstrap with a test vector per row ---------------------------------------
namespace {
// the packing shape: §12's PFKS shape (k = 1, 2^8 <= n <= 2^12, 1 <= b <= 32, l >= 1, b l <= 64) and n_in >= 1
bool pks_shape(uint64_t n, unsigned k, unsigned n_in, unsigned log_beta, unsigned l) { return n_in >= 1 && pfks_shape(n, k, log_beta, l); }
u64 pksk_words(uint64_t n, unsigned k, unsigned n_in, unsigned l) { return (u64)n_in * l * (k + 1) * n; }
}  // namespace

extern "C" size_t fhe_tfhe_pksk_words(uint64_t n, unsigned k, unsigned n_in, unsigned log_beta, unsigned l) {
    return pks_shape(n, k, n_in, log_beta, l) ? (size_t)pksk_words(n, k, n_in, l) : 0;
}

extern "C" int fhe_tlwe_gadget_packing_key_switch_dev(uint64_t n, unsigned k, unsigned n_in, unsigned log_beta, unsigned l, const void *d_pksk,
                                                      const void *d_in, size_t in_group_stride, size_t in_item_stride, size_t count,
                                                      unsigned log_stride, void *d_out, size_t groups, void *hip_stream) {
    const char *who = "fhe_tlwe_gadget_packing_key_switch_dev";
    int rc = check_ring(n, k, who);
    if (rc != FHE_OK) return rc;
    if (!pks_shape(n, k, n_in, log_beta, l))
        return fhe_fail(FHE_E_INVALID, "%s: no packing key switch for n=%llu, k=%u, n_in=%u, log_beta=%u, l=%u (needs k = 1, 256 <= n <= 4096, "
                        "n_in >= 1, 1 <= log_beta <= 32, l >= 1, log_beta l <= 64)", who, (unsigned long long)n, k, n_in, log_beta, l);
    const u32 L = (u32)__builtin_ctzll(n), k1 = k + 1;
    if (groups < 1 || count < 1 || log_stride > L || (u64)count > (n >> log_stride))
        return fhe_fail(FHE_E_INVALID, "%s: need groups >= 1, count >= 1, log_stride <= log2 n and count << log_stride <= n (groups=%llu, "
                        "count=%llu, log_stride=%u)", who, (unsigned long long)groups, (unsigned long long)count, log_stride);
    if ((u64)in_group_stride <= n_in || (u64)in_item_stride <= n_in)
        return fhe_fail(FHE_E_INVALID, "%s: both input strides must be at least n_in + 1 words", who);
    if (!d_pksk || !d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_pksk); REQUIRE_ALIGNED(d_in); REQUIRE_ALIGNED(d_out);
    const u32 cblocks = (u32)(k1 * n / fhe::PK_TH);
    const u64 tiles = ((u64)groups - 1) / fhe::PK_TG + 1;                                // every extent in bytes fits 61 bits
    if (tiles * cblocks > 0x7fffffffull || !mul_fits((u64)groups, (u64)k1 * n, kWordLimit) || !mul_fits((u64)groups - 1, in_group_stride, kWordLimit / 2) ||
        !mul_fits((u64)count - 1, in_item_stride, kWordLimit / 2 - n_in - 1))
        return fhe_fail(FHE_E_INVALID, "%s: groups or the input strides are too large for one launch", who);
    const u64 in_words = ((u64)groups - 1) * in_group_stride + ((u64)count - 1) * in_item_stride + n_in + 1;
    const u64 out_bytes = (u64)groups * k1 * n * 8;
    if (overlaps_any(d_out, out_bytes, {{d_pksk, pksk_words(n, k, n_in, l) * 8}, {d_in, in_words * 8}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the key or the input", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return launch("tlwe_packing_ks", L, st, fhe::tlwe_packing_ks_kernel, (unsigned)(tiles * cblocks), fhe::PK_TH, d_pksk, d_in, d_out, n_in, L, k1,
                  log_beta, l, fhe::gadget_cadd(log_beta, l), in_group_stride, in_item_stride, (u32)count, log_stride, groups, cblocks);
}

extern "C" int fhe_tglwe_box_expand_dev(uint64_t n, unsigned k, unsigned t_bits, const void *d_in, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_tglwe_box_expand_dev";
    int rc = check_ring(n, k, who);
    if (rc != FHE_OK) return rc;
    if (k != 1 || n < 256 || n > 4096)
        return fhe_fail(FHE_E_INVALID, "%s: needs k = 1, 256 <= n <= 4096 (n=%llu, k=%u)", who, (unsigned long long)n, k);
    const u32 L = (u32)__builtin_ctzll(n), k1 = k + 1;
    if (t_bits < 1 || t_bits > L) return fhe_fail(FHE_E_INVALID, "%s: need 1 <= t_bits <= log2 n (t_bits=%u, n=%llu)", who, t_bits, (unsigned long long)n);
    if (batch == 0) return FHE_OK;
    if (!d_in || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    REQUIRE_ALIGNED(d_in); REQUIRE_ALIGNED(d_out);
    if (!mul_fits((u64)batch, (u64)k1 * n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    const u64 rows = (u64)batch * k1, bytes = rows * n * 8;
    if (overlaps(d_out, bytes, d_in, bytes)) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps d_in", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return launch("tglwe_box_expand", L, st, fhe::tglwe_box_expand_kernel, (unsigned)std::min<u64>(rows, 256 * 16), 256, d_in, d_out, L, t_bits, rows);
}

extern "C" int fhe_tfhe_gadget_bootstrap_rows_dev(uint64_t n, unsigned k, unsigned log_beta, unsigned l, unsigned n_lwe, const void *d_bsk_prepared,
                                                  const void *d_tables, unsigned ks_log_beta, unsigned ks_l, const void *d_ksk, const void *d_in,
                                                  void *d_out, size_t batch, void *hip_stream) {
    return table_bootstrap("fhe_tfhe_gadget_bootstrap_rows_dev", "tfhe_br_rows_init", {n, k, log_beta, l, n_lwe, ks_log_beta, ks_l}, d_bsk_prepared,
                           d_tables, 1, d_ksk, d_in, d_out, batch, (hipStream_t)hip_stream);
}
