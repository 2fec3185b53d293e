// capi_internal.hpp — what the sources of the library share behind the public boundary: the plan and its device tables,
// the services of capi.hip (error reporting, device plans, workspace, staging pool, switches), and the host helpers every
// entry point is written with: the argument checks (REQUIRE_ALIGNED, overlaps / overlaps_any, mul_fits, check_ring),
// the timed launch with its check (launch / launch_named), the staging of host buffers around a *_dev call
// (FheHostStage, fhe_host_call), the owner of a table build's device allocations (FheTableUpload; DeviceTables keeps what
// it commits and frees it in release()), the read-once environment switches (fhe_env_switch) and, through
// host_tables.hpp, the host arithmetic behind every table (fhe::host).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fhe_ntt.h"
#include "../../include/fhe_ntt_experimental.h"   // the persistent kernels' switches: exported, outside the boundary
#include "host_tables.hpp"
#include "launch.hpp"
#include "ntt_kernels.hpp"

constexpr int kMaxDevices = 16;

struct DeviceTables {
    fhe::Tw *tw_fwd = nullptr;
    fhe::Tw *tw_inv = nullptr;
    fhe::u64 *digit_lut = nullptr;   // 136 words, n >= 8 (ntt_rounds.hpp: round0_bits)
    fhe::Tw32 *tw32_fwd = nullptr, *tw32_inv = nullptr;   // small moduli (smallq.hip)
    fhe::Tw *tw_fwd_pm = nullptr, *tw_inv_pm = nullptr;   // pseudo-Mersenne moduli: {w, w 2^32 mod q} (zq_device.hpp)
    fhe::Tw *tw_fwd_mg = nullptr, *tw_inv_mg = nullptr;   // q = 1 (mod 2^32) below 2^61: {w 2^32, w 2^64 mod q}
    fhe::Tw *twc_pm = nullptr;   // the one-launch transform's lane-ordered table of the last four stages (ntt_persist.hip), built on first use
    bool ready = false;
    std::vector<void *> owned;   // every allocation behind the pointers above (FheTableUpload::commit)
    void release() {
        for (void *p : owned) (void)hipFree(p);
        *this = DeviceTables();
    }
};

struct fhe_ntt_plan {
    fhe::u64 q = 0, n = 0, psi = 0, n_inv = 0;
    unsigned log_n = 0;
    std::vector<fhe::u64> roots, roots_inv;  // as the reference's CACHE value (ntt.rs:18)
    fhe::Mod mod{};
    fhe::Tw ninv{}, s_ninv{};
    fhe::Tw ninv_pm{}, s_ninv_pm{};   // the same two constants as {w, w 2^32 mod q} when mod.pm_k != 0
    fhe::Tw ninv_mg{}, s_ninv_mg{};   // ... as {w 2^32, w 2^64 mod q} when mod.mg_nqh != 0
    mutable std::mutex dev_lock;
    mutable DeviceTables dev[kMaxDevices];
};

int fhe_fail(int code, const char *fmt, ...);
int fhe_hip_fail(hipError_t e, const char *what);
#define HIP_TRY(expr)                                         \
    do {                                                      \
        hipError_t e_ = (expr);                               \
        if (e_ != hipSuccess) return fhe_hip_fail(e_, #expr); \
    } while (0)

int fhe_current_device(int *dev);
// FHE_NTT_CHECK_CANONICAL / fhe_ntt_set_check_canonical(1): FHE_E_NOT_CANONICAL if any of `count` device words is >= q (synchronises `st`); FHE_OK when the check is off
int fhe_check_canonical_words(uint64_t q, const void *d_x, size_t count, hipStream_t st, const char *who);
int fhe_device_plan(const fhe_ntt_plan *plan, fhe::DevicePlan *dp);
fhe::u64 fhe_batch_tile_for(const fhe_ntt_plan *plan);
// grow-only scratch per (slot, device, stream); slot 0 = fhe_rq_mul_dev / bfv tensor, slot 1 = zring, glue
int fhe_workspace_get(int slot, size_t bytes, hipStream_t st, void **out);
void fhe_workspace_free_all();
void fhe_ext32_free_all();   // zring.hip: tables of the two-small-prime (27-bit) products (digit32.hip)
void fhe_deep_free_all();    // ckks_deep.hip: the extension tables of the deep CKKS chains
namespace fhe { struct Ext32Args; }
int fhe_ext32_tables(uint64_t n, fhe::Ext32Args *a);   // fills the per-prime fields for the current device
// zring.hip: `keys` TGGSWs [key][(k+1)][l][(k+1)][n] -> keys * fhe_tggsw_prepared_words, in one or two launches (unvalidated)
int fhe_tggsw_prepare_keys(uint64_t n, unsigned k, unsigned l, uint64_t keys, const void *d_tggsw, void *d_prepared, hipStream_t st);
// ckks_eval.hip, for bfv_rns.hip: one limb of the eval-domain tensor (three components o_cs words apart, `count`
// words each), and the relinearisation of a chunk's tensor d [limbs][3][cr][n] into rows r0 .. of out [limbs][2][batch][n]
int fhe_rns_tensor_limb(const fhe_ntt_plan *p, const fhe::u64 *a, fhe::u64 a_cs, const fhe::u64 *b, fhe::u64 b_cs, fhe::u64 *out, fhe::u64 o_cs, fhe::u64 count,
                        hipStream_t st);
int fhe_rns_relin_rows(const fhe_ntt_plan *const *plans, unsigned limbs, const fhe_ntt_plan *special, const fhe::u64 *rlk, const fhe::u64 *d, fhe::u64 cr,
                       fhe::u64 *out, fhe::u64 batch, fhe::u64 r0, hipStream_t st);
// ckks_eval.hip, for ckks_deep.hip: one limb of the divide-and-round out = (x - t) inv (+ add) over two components
// of `count` words (g != 0: add's first component gathered at pi_g, for the first component only), and the diagonal term of one
// switching-key row in evals, pk0 += c s^2 or, where galois, c sigma_g(s)
int fhe_rns_divround_limb(const fhe_ntt_plan *p, const fhe::u64 *x, fhe::u64 x_cs, const fhe::u64 *t, fhe::u64 t_cs, const fhe::u64 *add, fhe::u64 add_cs, fhe::u64 *out,
                          fhe::u64 out_cs, fhe::u64 count, fhe::u64 inv, fhe::u32 g, hipStream_t st);
int fhe_rns_keyterm_limb(const fhe_ntt_plan *p, fhe::u64 *pk0, const fhe::u64 *s_evals, fhe::u64 c, fhe::u32 g, bool galois, hipStream_t st);
namespace fhe { struct SmallQArgs; }
// fills the modulus-dependent fields when the plan has a 32-bit form on this device (smallq.hip) and FHE_EXT32 is on
bool fhe_smallq_args(const fhe_ntt_plan *plan, const fhe::DevicePlan &dp, fhe::SmallQArgs *a);
int fhe_smallq_scratch(unsigned log_n, uint64_t rows, hipStream_t st, fhe::SmallQArgs *a);   // a->mid for n > 2^14
bool fhe_mg_enabled();                                 // FHE_MG=0 keeps q = 1 (mod 2^32) on the Shoup forward kernels
bool fhe_pm_enabled();                                 // FHE_PM=0 keeps pseudo-Mersenne moduli on the Shoup kernels
bool fhe_ext32_enabled();                              // FHE_EXT32=0 keeps every product on the 61-bit kernels
bool fhe_digit_mac_fused();                            // FHE_DIGIT_MAC_FUSED=0 (zring.hip): digit transforms written out, then one multiply-accumulate pass
// A switch of the environment: "0" turns one that defaults to on off, "1" turns one that defaults to off on, anything
// else leaves the default.  Read once per process, at first use: `static const bool on = fhe_env_switch("FHE_X", true);`
static inline bool fhe_env_switch(const char *name, bool dflt) {
    const char *e = getenv(name);
    return e ? (dflt ? e[0] != '0' : e[0] == '1') : dflt;
}
// pooled device staging for the host-buffer entry points (capi.hip); release only idle buffers
int fhe_stage_acquire(size_t bytes, void **out, size_t *got, int *dev);
void fhe_stage_release(void *ptr, size_t bytes, int dev);

static inline bool fhe_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
#define REQUIRE_ALIGNED(p)                                                                          \
    do {                                                                                            \
        if ((p) && fhe_misaligned(p))                                                               \
            return fhe_fail(FHE_E_INVALID, #p " must be 16-byte aligned (got %p)", (const void *)(p)); \
    } while (0)

// argument checks shared by the entry points: do two device ranges intersect (an empty or NULL one never does), does a b
// stay within limit, and the extent in words whose size in bytes still fits 61 bits
static inline bool overlaps(const void *a, fhe::u64 abytes, const void *b, fhe::u64 bbytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && abytes && bbytes && x < y + bbytes && y < x + abytes;
}
static inline bool mul_fits(fhe::u64 a, fhe::u64 b, fhe::u64 limit) { return b == 0 || a <= limit / b; }
constexpr fhe::u64 kWordLimit = ~0ull >> 4;

// grid of a grid-stride element-wise kernel: at most 16 blocks of 256 per CU
static inline unsigned fhe_ew_grid(fhe::u64 count) {
    fhe::u64 g = (count + 255) / 256;
    if (g > 256 * 16) g = 256 * 16;
    return (unsigned)(g ? g : 1);
}
// does [d_out, d_out + out_bytes) intersect one of the inputs {pointer, bytes}?
struct Extent { const void *p; fhe::u64 bytes; };
static inline bool overlaps_any(const void *d_out, fhe::u64 out_bytes, std::initializer_list<Extent> inputs) {
    for (const Extent &e : inputs)
        if (overlaps(d_out, out_bytes, e.p, e.bytes)) return true;
    return false;
}

// the ring size every polynomial entry point accepts, and with k the TGLWE dimension as well
static inline int check_ring(uint64_t n, const char *who) {
    if (n < 2 || (n & (n - 1)) != 0 || n > (1ull << 19))
        return fhe_fail(FHE_E_BAD_N, "%s: n=%llu must be a power of two in [2, 2^19]", who, (unsigned long long)n);
    return FHE_OK;
}
static inline int check_ring(uint64_t n, unsigned k, const char *who) {
    int rc = check_ring(n, who);
    if (rc != FHE_OK) return rc;
    if (k < 1 || k > 64) return fhe_fail(FHE_E_INVALID, "%s: need 1 <= k <= 64", who);
    return FHE_OK;
}

// a kernel argument as its parameter type: device pointers arrive as void *, and an integer may widen but not narrow
template <class P, class A>
P kernel_arg(A a) {
    static_assert(!(std::is_integral<P>::value && std::is_integral<A>::value) || sizeof(A) <= sizeof(P), "narrowing kernel argument: cast it at the call");
    return static_cast<P>(a);
}
// one timed launch (tag L for the timer) and its check: the FHE_* code.  A launch error names kernel_name, <label>_kernel if NULL.
template <class... P, class... A>
int launch_named(const char *label, const char *kernel_name, int L, hipStream_t st, void (*kernel)(P...), unsigned grid, unsigned block, A... args) {
    const hipError_t e = fhe::launch_grid(kernel, label, L, dim3(grid), block, 0, st, kernel_arg<P>(args)...);
    if (e == hipSuccess) return FHE_OK;
    char name[64];
    snprintf(name, sizeof name, "%s_kernel", label);
    return fhe_hip_fail(e, kernel_name ? kernel_name : name);
}
template <class K, class... A>
int launch(const char *label, int L, hipStream_t st, K kernel, unsigned grid, unsigned block, A... args) {
    return launch_named(label, nullptr, L, st, kernel, grid, block, args...);
}

// The device allocations of one table build.  alloc / up allocate on the current device (up also uploads `count` host
// elements, blocking); the first hipError_t stays in `err` and turns every later step into a no-op that returns nullptr;
// whatever was allocated is freed again by the destructor unless commit() handed it to the table's own list first.
struct FheTableUpload {
    std::vector<void *> owned;
    hipError_t err = hipSuccess;
    FheTableUpload() = default;
    FheTableUpload(const FheTableUpload &) = delete;
    FheTableUpload &operator=(const FheTableUpload &) = delete;
    ~FheTableUpload() {
        for (void *p : owned) (void)hipFree(p);
    }
    void *alloc(size_t bytes) {
        void *d = nullptr;
        if (err == hipSuccess && (err = hipMalloc(&d, bytes)) == hipSuccess) owned.push_back(d);
        return err == hipSuccess ? d : nullptr;
    }
    template <class T>
    T *up(const T *h, size_t count) {
        void *d = alloc(count * sizeof(T));
        if (d) err = hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice);
        return err == hipSuccess ? static_cast<T *>(d) : nullptr;
    }
    void commit(std::vector<void *> *keep) {
        keep->insert(keep->end(), owned.begin(), owned.end());
        owned.clear();
    }
};

// Staging of HOST buffers around a *_dev entry point: uploads on the calling thread's stream
// (hipStreamPerThread, for which the library workspace is per thread: no lock is needed); the
// destructor drains the stream on error paths before the buffers go back to the pool.
struct FheHostStage {
    struct Buf { void *p; size_t cap; int dev; };
    std::vector<Buf> bufs;
    bool clean = false;   // the stream has been synchronised after the last use of the buffers
    ~FheHostStage() {
        if (!clean) (void)hipStreamSynchronize(hipStreamPerThread);   // error path: drain before reuse
        for (auto &b : bufs) fhe_stage_release(b.p, b.cap, b.dev);
    }
    int up(const void *h, size_t bytes, void **d) {
        *d = nullptr;
        size_t got = 0;
        int dev = 0;
        int rc = fhe_stage_acquire(bytes, d, &got, &dev);
        if (rc != FHE_OK) return rc;
        bufs.push_back(Buf{*d, got, dev});
        if (h && bytes) {
            hipError_t e = hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, hipStreamPerThread);
            if (e != hipSuccess) return fhe_hip_fail(e, "hipMemcpyAsync H2D");
        }
        return FHE_OK;
    }
    // several results: down_async each, then finish() once (one synchronisation per call)
    int down_async(void *h, const void *d, size_t bytes) {
        HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, hipStreamPerThread));
        return FHE_OK;
    }
    int finish() {
        HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
        clean = true;
        return FHE_OK;
    }
    int down(void *h, const void *d, size_t bytes) {
        int rc = down_async(h, d, bytes);
        return rc != FHE_OK ? rc : finish();
    }
};

// A host-buffer entry point after its own argument checks: the device check, the inputs {host pointer, bytes} uploaded in
// order, the output buffer, `call(d)` — the *_dev call on hipStreamPerThread with d[i] input i and d[N] the output — and
// the download.
struct FheHostIn { const void *h; size_t bytes; };
template <size_t N, class F>
int fhe_host_call(const FheHostIn (&in)[N], void *out, size_t out_bytes, F call) {
    int dev, rc = fhe_current_device(&dev);
    if (rc != FHE_OK) return rc;
    FheHostStage hs;
    void *d[N + 1];
    for (size_t i = 0; i < N; i++)
        if ((rc = hs.up(in[i].h, in[i].bytes, &d[i])) != FHE_OK) return rc;
    if ((rc = hs.up(nullptr, out_bytes, &d[N])) != FHE_OK) return rc;
    if ((rc = call(d)) != FHE_OK) return rc;
    return hs.down(out, d[N], out_bytes);
}
