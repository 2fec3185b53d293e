// ckks_client.hip — the client side of CKKS on the device (ckks/src/encoder.rs, ckks/src/lib.rs:46-118): the
// canonical embedding as a double-precision FFT (encode, decode), the secret key, the public key, encryption and decryption.
//
//   embedding  w = exp(i pi / N); slot i of N/2 is the polynomial at w^(2i+1), i < N/2 (the reference's order); slots
//              N-1-i are the conjugates and are never stored
//   decode     z_i = (1/Delta) sum_j p_j w^((2i+1) j), p signed 64-bit words taken to f64 first
//   encode     a_j = (1/N) Re(w^-j sum_i h_i w^(-2ij)) over the Hermitian extension h of Delta z; coefficient j =
//              f64_as_i64(round(a_j)), round half away from zero
//   the fold   with M = N/2 and x_j = (p_j + i p_(j+M)) w^j, F_k = sum_j x_j exp(2 pi i jk / M) is the polynomial at
//              w^(4k+1): slot 2k = F_k / Delta, slot 2k+1 = conj(F_(M-1-k)) / Delta.  Decode is this M-point transform of
//              the folded, twisted coefficients; encode is its inverse (conjugate twiddles, untwist, 1/M) on F built
//              from the slots.  One transform of M = N/2 complex points in 8 N bytes of LDS serves a polynomial.
//   twiddles   d_tw [N] interleaved (cos, sin)(pi k / N), k < N, from fhe_ckks_twiddles: the twist w^j (j < M) and the
//              butterfly factors exp(2 pi i k / (2^s Ns)) = w^(k N / (2^(s-1) Ns)), all below w^N.  No sincos in a kernel.
//   stream     §17's ChaCha20 stream under CKKS_MASK = 0x21, CKKS_ERR = 0x22, CKKS_KEY = 0x23, CKKS_EPH = 0x24
//   secret     ternary from KEY word w: (w AND 1) - ((w >> 1) AND 1) as the residue 0, 1 or q - 1; v the same on EPH words
//   mask       uniform modulo q by §20's 128-bit map (NOT the reference's rounded Uniform(-1, 1), which hides nothing)
//   errors     cdt_error at log_scale 0; encryption row r: ERR rows 2r and 2r + 1, key row r: ERR row 2r
//   pk         (-a s + e, a);  c0 = v pk0 + e0 + (m mod q), c1 = v pk1 + e1, m signed words
//   decrypt    d = c0 + c1 s mod q, centred: d - q where d > floor(q / 2), as signed words
//
// The transform: Stockham autosort, radix-8 rounds (three radix-2 stages in registers, three table twiddles per thread and
// round) and a last round of radix 2^(log2 M mod 3); a thread owns 8 points, a polynomial M/8 threads, small rings share a
// workgroup.  Between rounds the points cross LDS as two planes of doubles (re, im) with the index swizzle `swz`:
// reads are unit-stride over a wave (ds_read_b64: 32-lane groups, 32 double banks: lanes l .. l+31 read a .. a+31, and swz
// is a bijection on each aligned run of 32).  Writes are ds_write_b64: 16-lane groups over 16 double banks (bits 0-3 of
// the index).  Round Ns = 1 writes index 8j + r: a group's lanes vary bits 3-6; round Ns = 8 writes 64 (j / 8) + j mod 8 +
// 8r: lanes vary bits 0-2 and 6; rounds Ns >= 64 write runs of 16.  swz XORs bit 4 into bit 0, bit 5 into bit 1 and bit 6
// into bits 2 and 3: the bank bits of the three patterns are (b3, b4, b5, b6 ^ b3) -> 16 values, (b0, b1, b2, b6) -> 16
// values, and the identity: conflict-free in every round for M >= 128 (smaller rings pack several polynomials into a
// group and may meet 2-way conflicts; they are not the sizes that matter).
//
// N = 2^14 .. 2^16 (fhe_ckks_embed_*): M = N/2 points do not fit a workgroup's LDS; the transform runs as
// two passes of ckks_fft sub-transforms, M = M1 M2, through [batch][M] complex values of workspace slot 11, with the same
// table (the sub-transforms read it with a stride, the factor between the passes is w^(4 j2 k1)), the same load-side work
// in front of pass 1 and the same store-side work behind pass 2.  The kernels and their tile are further down.
#include <cmath>

#include "bfv_client_kernels.hpp"

using fhe::Mod;
using fhe::u32;
using fhe::u64;

namespace fhe {

// CKKS as bfv_client_kernels.hpp's paths take a scheme: its rows of the stream, the signed message without a factor,
// workspace slot 11 (slot 10 is BFV's)
struct Ckks {
    static constexpr u32 MASK = 0x21, ERR = 0x22, KEY = 0x23, EPH = 0x24;
    static constexpr bool SIGNED_MSG = true;
    static constexpr int slot = 11;
    static constexpr const char *route_env = "FHE_CKKS_ENCRYPT_STAGED", *pk_label = "ckks_pk_epilogue", *encrypt_label = "ckks_encrypt_epilogue",
                                *decrypt_label = "ckks_decrypt_epilogue";
};

struct cplx { double re, im; };
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
// a times S i and a times exp(S i pi / 4)
template <int S> __device__ __forceinline__ cplx mul_i(cplx a) { return S > 0 ? cplx{-a.im, a.re} : cplx{a.im, -a.re}; }
template <int S> __device__ __forceinline__ cplx mul_z8(cplx a) {
    constexpr double h = 0.70710678118654752440;
    return S > 0 ? cplx{(a.re - a.im) * h, (a.im + a.re) * h} : cplx{(a.re + a.im) * h, (a.im - a.re) * h};
}
// table entry k (w^k), conjugated for the inverse direction
template <int S> __device__ __forceinline__ cplx tw_at(const double *__restrict__ tw, u32 k) { return {tw[2 * k], S > 0 ? tw[2 * k + 1] : -tw[2 * k + 1]}; }

__host__ __device__ constexpr u32 brev(u32 p, int L) {
    u32 r = 0;
    for (int i = 0; i < L; i++) r |= ((p >> i) & 1u) << (L - 1 - i);
    return r;
}

// The 2^L-point transform with exponent sign S of v[r] w^(r k) in place (w = exp(S 2 pi i / (2^L Ns)), the Stockham input
// twiddle): stage s multiplies by tws[s] = exp(S 2 pi i k / (2^(s+1) Ns)); ONE: k = 0, every twiddle is 1.  Output q sits
// in v[brev(q)].
template <int L, int S, bool ONE>
__device__ __forceinline__ void bfly(cplx *v, const cplx *tws) {
    auto tm = [&](int s, cplx x) { return ONE ? x : cmul(tws[s], x); };
    if constexpr (L == 1) {
        const cplx t = tm(0, v[1]);
        v[1] = csub(v[0], t); v[0] = cadd(v[0], t);
    } else if constexpr (L == 2) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const cplx t = tm(0, v[r + 2]);
            v[r + 2] = csub(v[r], t); v[r] = cadd(v[r], t);
        }
        cplx t = tm(1, v[1]);
        v[1] = csub(v[0], t); v[0] = cadd(v[0], t);
        t = mul_i<S>(tm(1, v[3]));
        v[3] = csub(v[2], t); v[2] = cadd(v[2], t);
    } else if constexpr (L == 3) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const cplx t = tm(0, v[r + 4]);
            v[r + 4] = csub(v[r], t); v[r] = cadd(v[r], t);
        }
#pragma unroll
        for (int q0 = 0; q0 < 2; q0++)
#pragma unroll
            for (int r = 0; r < 2; r++) {
                cplx t = tm(1, v[r + 2 + 4 * q0]);
                if (q0) t = mul_i<S>(t);
                v[r + 2 + 4 * q0] = csub(v[r + 4 * q0], t); v[r + 4 * q0] = cadd(v[r + 4 * q0], t);
            }
#pragma unroll
        for (int q0 = 0; q0 < 2; q0++)
#pragma unroll
            for (int q1 = 0; q1 < 2; q1++) {
                const int o = 2 * q1 + 4 * q0;
                cplx t = tm(2, v[o + 1]);
                if (q0) t = mul_z8<S>(t);
                if (q1) t = mul_i<S>(t);
                v[o + 1] = csub(v[o], t); v[o] = cadd(v[o], t);
            }
    }
}

template <int LM>
struct CkksShape {
    static constexpr int M = 1 << LM, LE = LM < 3 ? LM : 3, E = 1 << LE, TP = M / E;   // points, points and threads of a polynomial
    static constexpr int BT = TP > 256 ? TP : 256, PB = BT / TP;                       // threads and polynomials of a workgroup
    static constexpr int NR8 = LM / 3, LR = LM % 3;                                    // radix-8 rounds, log2 of the last radix
    static constexpr int LDS = LM > 3 ? PB * 2 * M : 1;                                // doubles
};

__device__ __forceinline__ u32 swz(u32 a) { return a ^ (((a >> 4) & 3u) | (((a >> 6) & 1u) * 12u)); }

// One polynomial: X_k = sum_j x_j exp(S 2 pi i jk / M), x_j = in(j), X_k to out(k, .); thread t of the polynomial's TP.
// Every thread of the workgroup calls it (the rounds meet at barriers).  TS: the table is that of a ring 2^TS times as
// large (entry k of this transform's own table is entry k << TS of it); LS: the stride in doubles of the points in sre and
// sim.  Both are constants of the instantiation: at the defaults the indices are what they were before the two-pass kernels.
template <int LM, int S, int TS = 0, int LS = 1, class In, class Out>
__device__ __forceinline__ void ckks_fft(double *sre, double *sim, u32 t, const double *__restrict__ tw, In in, Out out) {
    using Sh = CkksShape<LM>;
    constexpr int E = Sh::E, TP = Sh::TP, NR8 = Sh::NR8, LR = Sh::LR;
    cplx v[E];
#pragma unroll
    for (int e = 0; e < E; e++) v[e] = in(t + e * TP);
    if constexpr (LM <= 3) {
        bfly<LM, S, true>(v, nullptr);
#pragma unroll
        for (int p = 0; p < E; p++) out(brev(p, LM), v[p]);
    } else {
#pragma unroll
        for (int rd = 0; rd < NR8; rd++) {
            const int LNS = 3 * rd;
            const u32 k = t & ((1u << LNS) - 1u);
            if (rd == 0) {
                bfly<3, S, true>(v, nullptr);
            } else {
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 8; r++) v[r] = {sre[swz(t + r * TP) * LS], sim[swz(t + r * TP) * LS]};
                cplx tws[3];
#pragma unroll
                for (int s = 0; s < 3; s++) tws[s] = tw_at<S>(tw, k << (LM + 1 - s - LNS + TS));
                bfly<3, S, false>(v, tws);
            }
            if (rd == NR8 - 1 && LR == 0) {
#pragma unroll
                for (int p = 0; p < 8; p++) out(t + brev(p, 3) * TP, v[p]);
            } else {
                if (rd > 0) __syncthreads();
                const u32 j0 = ((t >> LNS) << (LNS + 3)) + k;
#pragma unroll
                for (int p = 0; p < 8; p++) {
                    const u32 a = swz(j0 + (brev(p, 3) << LNS)) * LS;
                    sre[a] = v[p].re; sim[a] = v[p].im;
                }
            }
        }
        if constexpr (LR > 0) {
            constexpr int R = 1 << LR, LNS = LM - LR;
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 8 / R; u++) {
                const u32 j = t + u * TP;
                cplx x[R], tws[LR];
#pragma unroll
                for (int r = 0; r < R; r++) x[r] = {sre[swz(j + (r << LNS)) * LS], sim[swz(j + (r << LNS)) * LS]};
#pragma unroll
                for (int s = 0; s < LR; s++) tws[s] = tw_at<S>(tw, j << (LR + 1 - s + TS));
                bfly<LR, S, false>(x, tws);
#pragma unroll
                for (int p = 0; p < R; p++) out(j + (brev(p, LR) << LNS), x[p]);
            }
        }
    }
}

// z [batch][N/2] interleaved = decode of p [batch][N] signed words: the i64 -> f64 conversion, the fold and the twist on the
// load, the slot order and the division by Delta on the store
template <int LM>
__global__ __launch_bounds__(CkksShape<LM>::BT) void ckks_decode_kernel(const double *__restrict__ tw, const long long *__restrict__ p, double *__restrict__ z,
                                                                        double delta, u64 batch) {
    using Sh = CkksShape<LM>;
    constexpr u32 M = Sh::M;
    __shared__ double lds[Sh::LDS];
    const u32 pl = threadIdx.x / Sh::TP, t = threadIdx.x % Sh::TP;
    const u64 poly = (u64)blockIdx.x * Sh::PB + pl;
    const bool valid = poly < batch;
    const long long *pp = p + (valid ? poly : 0) * (2 * M);
    double *zz = z + (valid ? poly : 0) * (2 * M);
    auto in = [&](u32 j) -> cplx {
        if (!valid) return {0.0, 0.0};
        const cplx c = {(double)pp[j], (double)pp[j + M]};
        return cmul(c, tw_at<1>(tw, j));
    };
    auto out = [&](u32 k, cplx F) {
        if (!valid) return;
        const bool lo = 2 * k < M;
        const u32 slot = lo ? 2 * k : 2 * M - 1 - 2 * k;
        zz[2 * slot] = F.re / delta;
        zz[2 * slot + 1] = (lo ? F.im : -F.im) / delta;
    };
    ckks_fft<LM, 1>(lds + pl * 2 * M, lds + pl * 2 * M + M, t, tw, in, out);
}

// out [batch][N] signed words = encode of z [batch][N/2] (row r at z + 2 r z_stride doubles; z_stride 0: one vector): Delta
// and the Hermitian extension on the load; the untwist, 1/M, the rounding and the i64 conversion on the store
template <int LM>
__global__ __launch_bounds__(CkksShape<LM>::BT) void ckks_encode_kernel(const double *__restrict__ tw, const double *__restrict__ z, u64 z_stride,
                                                                        long long *__restrict__ o, double delta, u64 batch) {
    using Sh = CkksShape<LM>;
    constexpr u32 M = Sh::M;
    __shared__ double lds[Sh::LDS];
    const u32 pl = threadIdx.x / Sh::TP, t = threadIdx.x % Sh::TP;
    const u64 poly = (u64)blockIdx.x * Sh::PB + pl;
    const bool valid = poly < batch;
    const double *zz = z + (valid ? poly : 0) * z_stride * 2;
    long long *oo = o + (valid ? poly : 0) * (2 * M);
    constexpr double inv_m = 1.0 / (double)M;
    auto in = [&](u32 k) -> cplx {
        if (!valid) return {0.0, 0.0};
        const bool lo = 2 * k < M;
        const u32 slot = lo ? 2 * k : 2 * M - 1 - 2 * k;
        const double re = delta * zz[2 * slot], im = delta * zz[2 * slot + 1];
        return {re, lo ? im : -im};
    };
    auto out = [&](u32 j, cplx X) {
        if (!valid) return;
        const cplx c = cmul(X, tw_at<-1>(tw, j));
        oo[j] = f64_as_i64(round(c.re * inv_m));
        oo[j + M] = f64_as_i64(round(c.im * inv_m));
    };
    ckks_fft<LM, -1>(lds + pl * 2 * M, lds + pl * 2 * M + M, t, tw, in, out);
}

// ---- 2^14 <= N <= 2^16: the same transform in two passes --------------------------------------------------
// M = 2^LB = M1 M2 points, j = j1 M2 + j2, k = k1 + M1 k2:
//   X_k = sum_j2 [ exp(S 2 pi i j2 k1 / M) sum_j1 x_(j1 M2 + j2) exp(S 2 pi i j1 k1 / M1) ] exp(S 2 pi i j2 k2 / M2)
// Pass 1: the M2 transforms of length M1 over j1 (stride M2), the one-pass kernels' load-side work in front, the factor
// exp(S 2 pi i j2 k1 / M) = w^(S 4 j2 k1) behind (4 j2 k1 < 2N; w^(e + N) = -w^e), Y [k1][j2] to the workspace.  Pass 2: the
// M1 transforms of length M2 over the rows k1 of Y, the store-side work behind.  A workgroup takes C = 16 adjacent columns
// j2 (pass 1) or rows k1 (pass 2), so that the strided side of either pass moves runs of 16 words: 128 bytes of signed
// words, 256 of the workspace.
//   pass 1   thread = (t, column c), c the fast index: a wave's loads and stores run along j2.  The points of the 16
//            columns interleave in LDS (point a of column c at 16 a + c, two planes of 16 M1 doubles): a 32-lane read
//            covers 16 columns x 2 points = 32 banks, a 16-lane write 16 columns = 16 banks
//   pass 2   thread = (row c, t), t the fast index: a wave reads runs of TP complex values (>= 256 bytes) of a row; rows
//            sit 2 M2 + 16 doubles apart (two rows of a 32-lane read meet different banks).  The outputs X_(k1 + M1 k2)
//            of a thread run along k2, M1 words apart: they cross LDS once more (row c at c (M2 + 2), so that a read of
//            16 rows x 2 points meets 32 banks) and leave along k1.
template <int LB>
struct EmbedShape {
    static constexpr int L1 = LB == 13 ? 6 : 7, L2 = LB - L1, C = 16;
    static constexpr u32 M = 1u << LB, M1 = 1u << L1, M2 = 1u << L2;
    static constexpr int TP1 = CkksShape<L1>::TP, TP2 = CkksShape<L2>::TP, BT1 = C * TP1, BT2 = C * TP2;
    static constexpr int LDS1 = 2 * C * M1;                                            // doubles
    static constexpr int ROW2 = 2 * M2 + 16, TROW2 = M2 + 2, LDS2 = C * ROW2;          // LDS2 >= 2 C TROW2
    static_assert(M1 % C == 0 && M2 % C == 0 && CkksShape<L1>::E == 8 && CkksShape<L2>::E == 8 && LDS2 >= 2 * C * TROW2, "tile");
};

// the load side of a polynomial: decode's fold and twist of the signed words, encode's Delta and Hermitian order
template <u32 M, bool DEC>
__device__ __forceinline__ cplx embed_load(const double *__restrict__ tw, const void *__restrict__ src, u32 j, double delta) {
    if constexpr (DEC) {
        const long long *pp = (const long long *)src;
        return cmul(cplx{(double)pp[j], (double)pp[j + M]}, tw_at<1>(tw, j));
    } else {
        const double *zz = (const double *)src;
        const bool lo = 2 * j < M;
        const u32 slot = lo ? 2 * j : 2 * M - 1 - 2 * j;
        const double re = delta * zz[2 * slot], im = delta * zz[2 * slot + 1];
        return {re, lo ? im : -im};
    }
}
// the store side: decode's slot order, conjugate and division; encode's untwist, 1/M, rounding and conversion
template <u32 M, bool DEC>
__device__ __forceinline__ void embed_store(const double *__restrict__ tw, void *__restrict__ dst, u32 k, cplx X, double delta) {
    if constexpr (DEC) {
        double *zz = (double *)dst;
        const bool lo = 2 * k < M;
        const u32 slot = lo ? 2 * k : 2 * M - 1 - 2 * k;
        zz[2 * slot] = X.re / delta;
        zz[2 * slot + 1] = (lo ? X.im : -X.im) / delta;
    } else {
        long long *oo = (long long *)dst;
        constexpr double inv_m = 1.0 / (double)M;
        const cplx c = cmul(X, tw_at<-1>(tw, k));
        oo[k] = f64_as_i64(round(c.re * inv_m));
        oo[k + M] = f64_as_i64(round(c.im * inv_m));
    }
}

// src: the chunk's polynomials ([rows][N] signed words, DEC) or slot rows (row r at 2 r src_stride doubles); ws [rows][M]
// complex.  Grid: rows x M2 / C workgroups, all of them whole.
template <int LB, bool DEC>
__global__ __launch_bounds__(EmbedShape<LB>::BT1) void ckks_embed_pass1_kernel(const double *__restrict__ tw, const void *__restrict__ src, u64 src_stride,
                                                                               double2 *__restrict__ ws, double delta) {
    using Sh = EmbedShape<LB>;
    constexpr u32 M = Sh::M, M2 = Sh::M2, N = 2 * M, C = Sh::C;
    constexpr int S = DEC ? 1 : -1;
    __shared__ double lds[Sh::LDS1];
    const u32 c = threadIdx.x % C, t = threadIdx.x / C;
    const u64 row = blockIdx.x / (M2 / C);
    const u32 j2 = (blockIdx.x % (M2 / C)) * C + c;
    const void *sp = DEC ? (const void *)((const long long *)src + row * N) : (const void *)((const double *)src + row * src_stride * 2);
    double2 *wp = ws + row * M;
    auto in = [&](u32 j1) -> cplx { return embed_load<M, DEC>(tw, sp, j1 * M2 + j2, delta); };
    auto out = [&](u32 k1, cplx Y) {
        const u32 e = 4 * j2 * k1;
        const bool neg = e >= N;
        const cplx T = tw_at<S>(tw, neg ? e - N : e);
        const cplx y = cmul(Y, neg ? cplx{-T.re, -T.im} : T);
        wp[k1 * M2 + j2] = make_double2(y.re, y.im);
    };
    ckks_fft<Sh::L1, S, LB - Sh::L1, C>(lds + c, lds + C * Sh::M1 + c, t, tw, in, out);
}

// dst: the chunk's slot rows ([rows][M] complex, DEC) or polynomials ([rows][N] signed words).  Grid: rows x M1 / C.
template <int LB, bool DEC>
__global__ __launch_bounds__(EmbedShape<LB>::BT2) void ckks_embed_pass2_kernel(const double *__restrict__ tw, const double2 *__restrict__ ws,
                                                                               void *__restrict__ dst, double delta) {
    using Sh = EmbedShape<LB>;
    constexpr u32 M = Sh::M, M1 = Sh::M1, M2 = Sh::M2, N = 2 * M, C = Sh::C, TP = Sh::TP2, P = Sh::TROW2;
    constexpr int S = DEC ? 1 : -1;
    __shared__ double lds[Sh::LDS2];
    const u32 c = threadIdx.x / TP, t = threadIdx.x % TP;
    const u64 row = blockIdx.x / (M1 / C);
    const u32 k1_0 = (blockIdx.x % (M1 / C)) * C;
    const double2 *wp = ws + row * M + (u64)(k1_0 + c) * M2;
    void *dp = DEC ? (void *)((double *)dst + row * N) : (void *)((long long *)dst + row * N);
    cplx xs[8];
    u32 ks[8];
    int cnt = 0;
    auto in = [&](u32 j2) -> cplx {
        const double2 v = wp[j2];
        return {v.x, v.y};
    };
    auto out = [&](u32 k2, cplx X) { ks[cnt] = k2; xs[cnt] = X; cnt++; };
    ckks_fft<Sh::L2, S, LB - Sh::L2>(lds + c * Sh::ROW2, lds + c * Sh::ROW2 + M2, t, tw, in, out);
    __syncthreads();
    double *tre = lds, *tim = lds + C * P;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        tre[c * P + ks[i]] = xs[i].re;
        tim[c * P + ks[i]] = xs[i].im;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u32 e = threadIdx.x + i * Sh::BT2, cc = e % C, k2 = e / C;             // e < 8 BT2 = C M2
        embed_store<M, DEC>(tw, dp, k1_0 + cc + M1 * k2, cplx{tre[cc * P + k2], tim[cc * P + k2]}, delta);
    }
}

// out = c0 + P mod q, centred as ring_n.rs:113-127: d - q where d > floor(q / 2), a signed word
__global__ __launch_bounds__(256) void ckks_decrypt_epilogue_kernel(const u64 *__restrict__ c0, const u64 *__restrict__ P, u64 *__restrict__ out, u64 count,
                                                                    Mod m) {
    const u64 stride = (u64)gridDim.x * 256, half = m.q >> 1;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) {
        const u64 d = add63(c0[i], P[i], m);
        out[i] = d > half ? d - m.q : d;
    }
}

}  // namespace fhe

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

constexpr u64 kCkksMaxN = 1ull << 13;           // M = N/2 = 2^12 complex points fill 64 KiB of LDS
constexpr u64 kCkksEmbedMaxN = 1ull << 16;      // the two-pass kernels: M = 2^13 .. 2^15

int check_encoder_n(uint64_t n, u64 max_n, const char *who) {
    if (n < 2 || (n & (n - 1)) != 0 || n > max_n)
        return fhe_fail(FHE_E_INVALID, "%s: n=%llu must be a power of two in [2, 2^%u]", who, (unsigned long long)n, log2_of(max_n));
    return FHE_OK;
}
int check_encoder(uint64_t n, double delta, u64 max_n, const char *who) {
    int rc = check_encoder_n(n, max_n, who);
    if (rc != FHE_OK) return rc;
    if (!(delta > 0.0) || !std::isfinite(delta)) return fhe_fail(FHE_E_INVALID, "%s: the scale must be finite and positive", who);
    return FHE_OK;
}

template <int LM>
int launch_decode(const double *tw, const long long *p, double *z, double delta, u64 batch, hipStream_t st) {
    using Sh = fhe::CkksShape<LM>;
    return launch("ckks_decode", LM + 1, st, fhe::ckks_decode_kernel<LM>, (unsigned)((batch + Sh::PB - 1) / Sh::PB), Sh::BT, tw, p, z, delta, batch);
}
template <int LM>
int launch_encode(const double *tw, const double *z, u64 z_stride, long long *o, double delta, u64 batch, hipStream_t st) {
    using Sh = fhe::CkksShape<LM>;
    return launch("ckks_encode", LM + 1, st, fhe::ckks_encode_kernel<LM>, (unsigned)((batch + Sh::PB - 1) / Sh::PB), Sh::BT, tw, z, z_stride, o, delta, batch);
}
#define CKKS_BY_SIZE(LM, CALL)                                                                                      \
    switch (LM) {                                                                                                   \
        case 0: return CALL(0); case 1: return CALL(1); case 2: return CALL(2); case 3: return CALL(3);             \
        case 4: return CALL(4); case 5: return CALL(5); case 6: return CALL(6); case 7: return CALL(7);             \
        case 8: return CALL(8); case 9: return CALL(9); case 10: return CALL(10); case 11: return CALL(11);         \
        default: return CALL(12);                                                                                   \
    }

// the polynomials of one pass over the workspace: the chunk of the other CKKS calls (2^21 words; 16 MiB of complex values)
u64 embed_chunk(uint64_t n, u64 batch) { return std::min<u64>(batch, std::max<u64>(1, kChunkWords >> log2_of(n))); }

// the two passes over `rows` polynomials of a chunk (rows n / 16 <= 2^17 workgroups a pass)
template <int LB, bool DEC>
int launch_embed(const double *tw, const void *src, u64 src_stride, double2 *ws, void *dst, double delta, u64 rows, hipStream_t st) {
    using Sh = fhe::EmbedShape<LB>;
    int rc = launch(DEC ? "ckks_embed_decode_pass1" : "ckks_embed_encode_pass1", LB + 1, st, fhe::ckks_embed_pass1_kernel<LB, DEC>,
                    (unsigned)(rows * (Sh::M2 / Sh::C)), Sh::BT1, tw, src, src_stride, ws, delta);
    if (rc != FHE_OK) return rc;
    return launch(DEC ? "ckks_embed_decode_pass2" : "ckks_embed_encode_pass2", LB + 1, st, fhe::ckks_embed_pass2_kernel<LB, DEC>,
                  (unsigned)(rows * (Sh::M1 / Sh::C)), Sh::BT2, tw, ws, dst, delta);
}
// 2^14 <= n <= 2^16: chunk by chunk through workspace slot 11 (nothing else of CKKS's is live during an encoder call)
template <bool DEC>
int embed_two_pass(uint64_t n, double delta, const double *tw, const void *src, u64 src_stride, void *dst, u64 batch, hipStream_t st) {
    const u64 chunk = embed_chunk(n, batch);
    void *w = nullptr;
    int rc = fhe_workspace_get(fhe::Ckks::slot, chunk * n * 8, st, &w);
    if (rc != FHE_OK) return rc;
    for (u64 r0 = 0; r0 < batch; r0 += chunk) {
        const u64 rows = std::min<u64>(chunk, batch - r0);
        const void *s = DEC ? (const void *)((const long long *)src + r0 * n) : (const void *)((const double *)src + r0 * src_stride * 2);
        void *d = (void *)((u64 *)dst + r0 * n);                    // n words a row either way: signed words, or n / 2 complex values
        switch (log2_of(n)) {
            case 14: rc = launch_embed<13, DEC>(tw, s, src_stride, (double2 *)w, d, delta, rows, st); break;
            case 15: rc = launch_embed<14, DEC>(tw, s, src_stride, (double2 *)w, d, delta, rows, st); break;
            default: rc = launch_embed<15, DEC>(tw, s, src_stride, (double2 *)w, d, delta, rows, st); break;
        }
        if (rc != FHE_OK) return rc;
    }
    return FHE_OK;
}

// the table of fhe_ckks_twiddles and fhe_ckks_embed_twiddles
int ckks_twiddles(uint64_t n, u64 max_n, double *out, const char *who) {
    int rc = check_encoder_n(n, max_n, who);
    if (rc != FHE_OK) return rc;
    if (!out) return fhe_fail(FHE_E_NULL, "%s: NULL table", who);
    const long double pi = 3.141592653589793238462643383279502884L;
    for (uint64_t k = 0; k < n; k++) {
        // octant symmetry: the argument handed to cosl / sinl never passes pi / 4
        const uint64_t kk = 2 * k <= n ? k : n - k;             // pi kk / n in [0, pi / 2]; cos changes sign past pi / 2
        long double c, s;
        if (4 * kk <= n) {
            const long double a = pi * (long double)kk / (long double)n;
            c = cosl(a); s = sinl(a);
        } else {
            const long double a = pi * (long double)(n - 2 * kk) / (long double)(2 * n);
            c = sinl(a); s = cosl(a);
        }
        out[2 * k] = (double)(2 * k <= n ? c : -c);
        out[2 * k + 1] = (double)s;
    }
    return FHE_OK;
}

// fhe_ckks_encode_dev and fhe_ckks_embed_encode_dev: the checks in the ABI's order, the one-pass kernels up to 2^13
int ckks_encode(const char *who, u64 max_n, uint64_t n, double delta, const void *d_tw, const void *d_z, size_t z_stride, void *d_out, size_t batch,
                void *hip_stream) {
    int rc = check_encoder(n, delta, max_n, who);
    if (rc != FHE_OK) return rc;
    if (z_stride != 0 && z_stride < n / 2) return fhe_fail(FHE_E_INVALID, "%s: z_stride must be 0 (one vector) or at least n / 2", who);
    if (batch == 0) return FHE_OK;
    if (!mul_fits((u64)batch, n, kWordLimit) || !mul_fits((u64)batch - 1, (u64)z_stride, (kWordLimit - n) / 2))
        return fhe_fail(FHE_E_INVALID, "%s: batch or z_stride too large", who);
    if (!d_tw || !d_z || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_tw) || misaligned8(d_z) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    const u64 z_bytes = (((u64)batch - 1) * z_stride + n / 2) * 16;
    if (overlaps_any(d_out, (u64)batch * n * 8, {{d_z, z_bytes}, {d_tw, n * 16}})) return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the slots or the twiddle table", who);
    int dev;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (n > kCkksMaxN) return embed_two_pass<false>(n, delta, (const double *)d_tw, d_z, (u64)z_stride, d_out, (u64)batch, st);
#define CKKS_ENC(LM) launch_encode<LM>((const double *)d_tw, (const double *)d_z, (u64)z_stride, (long long *)d_out, delta, (u64)batch, st)
    CKKS_BY_SIZE(log2_of(n) - 1, CKKS_ENC)
#undef CKKS_ENC
}

int ckks_decode(const char *who, u64 max_n, uint64_t n, double delta, const void *d_tw, const void *d_p, void *d_out, size_t batch, void *hip_stream) {
    int rc = check_encoder(n, delta, max_n, who);
    if (rc != FHE_OK) return rc;
    if (batch == 0) return FHE_OK;
    if (!mul_fits((u64)batch, n, kWordLimit)) return fhe_fail(FHE_E_INVALID, "%s: batch too large", who);
    if (!d_tw || !d_p || !d_out) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_tw) || misaligned8(d_p) || misaligned8(d_out)) return fhe_fail(FHE_E_INVALID, "%s: buffers must be 8-byte aligned", who);
    if (overlaps_any(d_out, (u64)batch * n * 8, {{d_p, (u64)batch * n * 8}, {d_tw, n * 16}}))
        return fhe_fail(FHE_E_INVALID, "%s: d_out overlaps the polynomials or the twiddle table", who);
    int dev;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (n > kCkksMaxN) return embed_two_pass<true>(n, delta, (const double *)d_tw, d_p, 0, d_out, (u64)batch, st);
#define CKKS_DEC(LM) launch_decode<LM>((const double *)d_tw, (const long long *)d_p, (double *)d_out, delta, (u64)batch, st)
    CKKS_BY_SIZE(log2_of(n) - 1, CKKS_DEC)
#undef CKKS_DEC
}

}  // namespace

extern "C" int fhe_ckks_twiddles(uint64_t n, double *out) { return ckks_twiddles(n, kCkksMaxN, out, "fhe_ckks_twiddles"); }
extern "C" int fhe_ckks_embed_twiddles(uint64_t n, double *out) { return ckks_twiddles(n, kCkksEmbedMaxN, out, "fhe_ckks_embed_twiddles"); }

extern "C" int fhe_ckks_encode_dev(uint64_t n, double delta, const void *d_tw, const void *d_z, size_t z_stride, void *d_out, size_t batch, void *hip_stream) {
    return ckks_encode("fhe_ckks_encode_dev", kCkksMaxN, n, delta, d_tw, d_z, z_stride, d_out, batch, hip_stream);
}
extern "C" int fhe_ckks_embed_encode_dev(uint64_t n, double delta, const void *d_tw, const void *d_z, size_t z_stride, void *d_out, size_t batch,
                                         void *hip_stream) {
    return ckks_encode("fhe_ckks_embed_encode_dev", kCkksEmbedMaxN, n, delta, d_tw, d_z, z_stride, d_out, batch, hip_stream);
}

extern "C" int fhe_ckks_decode_dev(uint64_t n, double delta, const void *d_tw, const void *d_p, void *d_out, size_t batch, void *hip_stream) {
    return ckks_decode("fhe_ckks_decode_dev", kCkksMaxN, n, delta, d_tw, d_p, d_out, batch, hip_stream);
}
extern "C" int fhe_ckks_embed_decode_dev(uint64_t n, double delta, const void *d_tw, const void *d_p, void *d_out, size_t batch, void *hip_stream) {
    return ckks_decode("fhe_ckks_embed_decode_dev", kCkksEmbedMaxN, n, delta, d_tw, d_p, d_out, batch, hip_stream);
}

// the workspace of one fhe_ckks_embed_encode_dev / _decode_dev call: the chunk's [M] complex rows; 0 where no workspace is
// taken (n <= 2^13, batch = 0) and for a shape the calls refuse
extern "C" size_t fhe_ckks_embed_workspace_bytes(uint64_t n, size_t batch) {
    if (n < 2 || (n & (n - 1)) != 0 || n > kCkksEmbedMaxN || n <= kCkksMaxN || batch == 0 || !mul_fits((u64)batch, n, kWordLimit)) return 0;
    return (size_t)(embed_chunk(n, (u64)batch) * n * 8);
}

extern "C" int fhe_ckks_secret_key_dev(const fhe_ntt_plan *plan, const uint8_t *seed, uint64_t key_row, void *d_s, void *hip_stream) {
    const char *who = "fhe_ckks_secret_key_dev";
    if (!plan) return fhe_fail(FHE_E_NULL, "%s: plan is NULL", who);
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    if (!d_s) return fhe_fail(FHE_E_NULL, "%s: NULL buffer", who);
    if (misaligned8(d_s)) return fhe_fail(FHE_E_INVALID, "%s: d_s must be 8-byte aligned", who);
    int dev, rc;
    if ((rc = fhe_current_device(&dev)) != FHE_OK) return rc;
    return small_fill(seed_key(seed), fhe::Ckks::KEY, 0, key_row, plan->q, plan->n, (u64 *)d_s, 1, (hipStream_t)hip_stream);
}

extern "C" int fhe_ckks_public_key_dev(const fhe_ntt_plan *plan, const uint8_t *seed, uint64_t row, const void *d_s, const void *d_cdt, unsigned m,
                                       void *d_pk, void *hip_stream) {
    const char *who = "fhe_ckks_public_key_dev";
    if (!plan) return fhe_fail(FHE_E_NULL, "%s: plan is NULL", who);
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    return rlwe_public_key<fhe::Ckks>(who, plan, seed, row, d_s, d_cdt, m, d_pk, (hipStream_t)hip_stream, [&](u64 *S, hipStream_t st) -> int {
        HIP_TRY(hipMemcpyAsync(S, d_s, plan->n * 8, hipMemcpyDeviceToDevice, st));      // the product takes 16-byte aligned rows
        return FHE_OK;
    });
}

extern "C" int fhe_ckks_encrypt_dev(const fhe_ntt_plan *plan, const uint8_t *seed, uint64_t first_row, const void *d_pk_evals, const void *d_msg,
                                    size_t msg_stride, const void *d_cdt, unsigned m, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_encrypt_dev";
    if (!plan) return fhe_fail(FHE_E_NULL, "%s: plan is NULL", who);
    if (!seed) return fhe_fail(FHE_E_NULL, "%s: NULL seed", who);
    return rlwe_encrypt<fhe::Ckks>(who, plan, 0, seed, first_row, d_pk_evals, d_msg, msg_stride, d_cdt, m, d_out, batch, (hipStream_t)hip_stream);
}

extern "C" int fhe_ckks_decrypt_dev(const fhe_ntt_plan *plan, const void *d_s_evals, const void *d_ct, void *d_out, size_t batch, void *hip_stream) {
    const char *who = "fhe_ckks_decrypt_dev";
    if (!plan) return fhe_fail(FHE_E_NULL, "%s: plan is NULL", who);
    hipStream_t st = (hipStream_t)hip_stream;
    return rlwe_decrypt<fhe::Ckks>(who, plan, d_s_evals, d_ct, d_out, batch, st, [&](const char *label, const u64 *c0, const u64 *P, u64 *out, u64 count) {
        return launch(label, (int)plan->log_n, st, fhe::ckks_decrypt_epilogue_kernel, fhe_ew_grid(count), 256, c0, P, out, count, plan->mod);
    });
}
