"""ctypes binding of libfhe_ntt.so (include/fhe_ntt.h).

This is plumbing only: every call goes straight to the C ABI, which runs the HIP
kernels.  There is no Python/numpy compute path and no CPU fallback — if the
library is missing, or no GPU is present, calls raise.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FHE_NTT_LIB") or os.path.join(_HERE, "libfhe_ntt.so")  # env: A/B builds
CSRC = os.path.join(_HERE, "csrc")
SOURCES = ["capi.hip", "ntt_kernels.hip", "ntt_kernels_q62.hip", "ntt_persist.hip", "digit_mac.hip", "digit32.hip", "bfv32.hip", "smallq.hip", "generic63.hip", "zring.hip", "glue.hip", "tfhe_boot.hip", "tfhe_client.hip", "bfv_client.hip", "ckks_client.hip", "ckks_eval.hip", "bfv_rns.hip", "ckks_deep.hip"]
HEADERS = ["ntt_kernels.hpp", "ntt_rounds.hpp", "ntt_persist.hpp", "persist_sched.hpp", "digit_mac.hpp", "digit32.hpp", "bfv32.hpp", "smallq.hpp", "ntt32_rounds.hpp", "ntt32_big.hpp", "zq_device.hpp", "capi_internal.hpp", "host_tables.hpp", "host_dispatch.hpp", "launch.hpp", "mac_kernel.hpp", "chacha_stream.hpp", "bfv_client_kernels.hpp", "rns_tables.hpp", "rns_ext_device.hpp", "ntt_kernels.hip",
           os.path.join("..", "..", "include", "fhe_ntt.h"), os.path.join("..", "..", "include", "fhe_ntt_experimental.h")]
OBJ_DIR = os.path.join(_HERE, "build")
# -ffp-contract=off: zring.hip restates the reference's f64 scale-and-round (one IEEE rounding
# per operation); nothing else in the library uses floating point.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
               "-ffp-contract=off"]

FHE_OK = 0
FHE_E_BAD_N = -1
FHE_E_BAD_Q = -2
FHE_E_NO_ROOT = -3
FHE_E_NULL = -4
FHE_E_HIP = -5
FHE_E_NO_DEVICE = -6
FHE_E_PARAM_MISMATCH = -7
FHE_E_NOT_CANONICAL = -8
FHE_E_INVALID = -9
# flags of the N3 batch surfaces (include/fhe_ntt.h)
FHE_A_IS_EVALS, FHE_B_IS_EVALS, FHE_OUT_EVALS = 1, 2, 4

# every symbol include/fhe_ntt.h declares (tests check the .so exports them all)
EXPORTS = [
    "fhe_ntt_plan_get", "fhe_ntt_plan_info", "fhe_ntt_plan_tables",
    "fhe_ntt_forward", "fhe_ntt_inverse", "fhe_rq_mul", "fhe_rq_mul_checked",
    "fhe_rq_pointwise_mul", "fhe_rq_check_canonical",
    "fhe_ntt_forward_dev", "fhe_ntt_inverse_dev", "fhe_rq_mul_dev",
    "fhe_rq_mul_workspace_bytes", "fhe_rq_pointwise_mul_dev", "fhe_fill_synthetic_dev",
    "fhe_ntt_set_batch_tile", "fhe_ntt_kernel_timing_enable", "fhe_ntt_kernel_timing_read",
    "fhe_ntt_kernel_timing_reset",
    "fhe_ntt_device_count", "fhe_last_error", "fhe_ntt_version", "fhe_ntt_shutdown",
    "fhe_ntt_plan_prepare", "fhe_ntt_plan_arithmetic", "fhe_ntt_set_check_canonical", "fhe_shard_range", "fhe_shard_gather_dev", "fhe_ntt_release_stream_workspace", "fhe_ntt_workspace_bytes",
    "fhe_tggsw_prepared_words", "fhe_tggsw_prepare_dev", "fhe_tggsw_external_product_prepared_dev",
    "fhe_glwe_ksk_prepared_words", "fhe_glwe_ksk_prepare_dev", "fhe_glwe_key_switch_prepared_dev",
    "fhe_bfv_rlk_prepared_words", "fhe_bfv_rlk_prepare_dev", "fhe_bfv_relinearize_prepared_dev", "fhe_bfv_mul_prepared_dev",
    # next rows: exact products over Z / mod 2^64 on top of the engine
    "fhe_r_naive_mul", "fhe_r_naive_mul_dev", "fhe_mul_div_round_dev",
    "fhe_bfv_tensor", "fhe_bfv_tensor_dev", "fhe_bfv_relinearize_dev", "fhe_bfv_mul", "fhe_bfv_mul_dev",
    "fhe_tn_mul", "fhe_tn_mul_dev", "fhe_tggsw_external_product", "fhe_tggsw_external_product_dev",
    # rows N3/N4: batch surfaces and element-wise glue
    "fhe_tr_dot_dev", "fhe_tr_mul_r_dev", "fhe_glev_mul_dev", "fhe_glwe_key_switch_dev",
    "fhe_tr_dot", "fhe_tr_mul_r", "fhe_glev_mul", "fhe_glwe_key_switch",
    "fhe_tglwe_mul_tn", "fhe_tglwe_mul_tn_dev", "fhe_tglev_mul", "fhe_tglev_mul_dev",
    "fhe_rq_add_dev", "fhe_rq_sub_dev", "fhe_rq_neg_dev", "fhe_rq_mul_by_u64_dev",
    "fhe_rq_mod_switch_dev", "fhe_rq_mul_div_round_dev", "fhe_rq_decompose_dev",
    "fhe_rq_remodule_dev", "fhe_rq_mul_by_f64_dev", "fhe_rq_div_round_dev",
    # TFHE bootstrapping (tfhe_boot.hip)
    "fhe_tfhe_bsk_prepared_words", "fhe_tfhe_bsk_prepare_dev", "fhe_tfhe_blind_rotation_dev",
    "fhe_tglwe_sample_extraction_dev", "fhe_tlwe_key_switch_dev", "fhe_tfhe_bootstrap_dev",
    # the signed base-2^b gadget (tfhe_boot.hip)
    "fhe_tn_gadget_decompose_dev", "fhe_tggsw_gadget_prepared_words", "fhe_tggsw_gadget_prepare_dev",
    "fhe_tggsw_gadget_external_product_dev", "fhe_tfhe_gadget_bsk_prepared_words", "fhe_tfhe_gadget_bsk_prepare_dev",
    "fhe_tfhe_gadget_blind_rotation_dev", "fhe_tlwe_gadget_key_switch_dev", "fhe_tfhe_gadget_bootstrap_dev",
    # circuit bootstrapping and the CMux with a selector per ciphertext (tfhe_boot.hip)
    "fhe_tfhe_pfksk_words", "fhe_tlwe_gadget_private_key_switch_dev", "fhe_tggsw_gadget_prepare_many_dev",
    "fhe_tggsw_gadget_cmux_dev", "fhe_tfhe_circuit_bootstrap_dev",
    # boolean gates with gate bootstrapping (tfhe_boot.hip)
    "fhe_tfhe_gate_bootstrap_dev", "fhe_tfhe_gate_mux_dev",
    # small integers: a lookup table per row (tfhe_boot.hip)
    "fhe_tlwe_lincomb_dev", "fhe_tfhe_lut_bootstrap_dev",
    # small integers: several tables from one blind rotation (tfhe_boot.hip)
    "fhe_tfhe_lut_many_bootstrap_dev",
    # packing key switch and the bootstrap with a test vector per row (tfhe_boot.hip)
    "fhe_tfhe_pksk_words", "fhe_tlwe_gadget_packing_key_switch_dev", "fhe_tglwe_box_expand_dev", "fhe_tfhe_gadget_bootstrap_rows_dev",
    # key generation, encryption and decryption: the client side (tfhe_client.hip)
    "fhe_tfhe_stream_words_dev", "fhe_tlwe_encrypt_dev", "fhe_tlwe_phase_dev", "fhe_tglwe_encrypt_dev", "fhe_tglwe_phase_dev",
    # BFV key generation, encryption and decryption: the client side (bfv_client.hip)
    "fhe_bfv_secret_key_dev", "fhe_bfv_public_key_dev", "fhe_bfv_relin_key_dev", "fhe_bfv_encrypt_dev", "fhe_bfv_decrypt_dev",
    # CKKS: the FFT encoder, key generation, encryption and decryption (ckks_client.hip)
    "fhe_ckks_twiddles", "fhe_ckks_encode_dev", "fhe_ckks_decode_dev", "fhe_ckks_secret_key_dev", "fhe_ckks_public_key_dev", "fhe_ckks_encrypt_dev",
    "fhe_ckks_decrypt_dev",
    # CKKS on an RNS modulus chain: ct x ct, relinearisation, rescaling (ckks_eval.hip)
    "fhe_ckks_rns_from_i64_dev", "fhe_ckks_rns_relin_key_dev", "fhe_ckks_rns_tensor_dev", "fhe_ckks_rns_relinearize_dev", "fhe_ckks_rns_mul_dev",
    "fhe_ckks_rns_rescale_dev", "fhe_ckks_rns_workspace_bytes",
    # CKKS on the RNS chain: slot rotations and conjugation with Galois keys (ckks_eval.hip)
    "fhe_ckks_galois_evals_dev", "fhe_ckks_rns_galois_key_dev", "fhe_ckks_rns_galois_dev", "fhe_ckks_rns_galois_workspace_bytes",
    # CKKS on the RNS chain: plaintext linear transforms, the double-hoisted diagonal sum (ckks_eval.hip)
    "fhe_ckks_rns_diag_sum_dev", "fhe_ckks_rns_diag_workspace_bytes",
    # CKKS on the RNS chain: fused sums of ciphertexts by public scalars (ckks_eval.hip)
    "fhe_ckks_rns_lincomb_dev",
    # CKKS on the RNS chain: inner products, a sum of ct x ct pairs with one relinearisation (ckks_eval.hip)
    "fhe_ckks_rns_dot_dev",
    # CKKS on the RNS chain: baby-step giant-step linear transforms with hoisted giant steps (ckks_eval.hip)
    "fhe_ckks_rns_bsgs_dev", "fhe_ckks_rns_bsgs_workspace_bytes",
    # CKKS: the encoder up to n = 2^16, a two-pass transform above 2^13 (ckks_client.hip)
    "fhe_ckks_embed_twiddles", "fhe_ckks_embed_encode_dev", "fhe_ckks_embed_decode_dev", "fhe_ckks_embed_workspace_bytes",
    # BFV on an RNS modulus chain: exact basis extension, ct x ct, message scaling, decryption (bfv_rns.hip)
    "fhe_rns_extend_dev", "fhe_bfv_rns_tensor_dev", "fhe_bfv_rns_mul_dev", "fhe_bfv_rns_workspace_bytes", "fhe_bfv_rns_scale_msg_dev", "fhe_bfv_rns_decrypt_dev",
    # BFV on the chain: inner products, one rounding and one relinearisation (bfv_rns.hip)
    "fhe_bfv_rns_dot_dev",
    # CKKS on a deep RNS chain: grouped-digit key switching, up to 32 limbs (ckks_deep.hip)
    "fhe_ckks_deep_relin_key_dev", "fhe_ckks_deep_galois_key_dev", "fhe_ckks_deep_relinearize_dev", "fhe_ckks_deep_mul_dev", "fhe_ckks_deep_galois_dev",
    "fhe_ckks_deep_rescale_dev", "fhe_ckks_deep_workspace_bytes",
    # CKKS on a deep RNS chain: plaintext linear transforms, the double-hoisted diagonal sum (ckks_deep.hip)
    "fhe_ckks_deep_diag_sum_dev", "fhe_ckks_deep_diag_workspace_bytes",
    # CKKS on a deep RNS chain: scalar sums and inner products over a slice of limbs a launch (ckks_deep.hip)
    "fhe_ckks_deep_lincomb_dev", "fhe_ckks_deep_dot_dev",
]
FHE_CKKS_GALOIS_MAX_COUNT = 256              # include/fhe_ntt.h: the most Galois elements of one fhe_ckks_rns_galois_dev call
FHE_CKKS_DIAG_MAX_OUTPUTS = 64               # include/fhe_ntt.h: the most outputs of one fhe_ckks_rns_diag_sum_dev call
FHE_CKKS_LINCOMB_MAX_COUNT, FHE_CKKS_LINCOMB_MAX_OUTPUTS = 64, 16    # include/fhe_ntt.h: the most inputs and outputs of one fhe_ckks_rns_lincomb_dev call
FHE_CKKS_DOT_MAX_COUNT = 64                  # include/fhe_ntt.h: the most pairs of one fhe_ckks_rns_dot_dev call
FHE_BFV_DOT_MAX_COUNT = 64                   # include/fhe_ntt.h: the most pairs of one fhe_bfv_rns_dot_dev call
FHE_CKKS_DEEP_MAX_LIMBS, FHE_CKKS_DEEP_MAX_SPECIALS = 32, 8    # include/fhe_ntt.h: the most chain and special primes of the fhe_ckks_deep_* calls

# FHE_GATE_* (include/fhe_ntt.h): name -> op code of fhe_tfhe_gate_bootstrap_dev
GATES = {"AND": 0, "NAND": 1, "OR": 2, "NOR": 3, "XOR": 4, "XNOR": 5, "ANDNY": 6, "ANDYN": 7, "ORNY": 8, "ORYN": 9}
FHE_GATE_COUNT = 10
FHE_LUT_NONE = 0xFFFFFFFF                    # include/fhe_ntt.h: the index of an operand whose scale is 0, by convention
FHE_STREAM_MASK, FHE_STREAM_ERR, FHE_STREAM_KEY = 1, 2, 3    # include/fhe_ntt.h: the purposes of the random stream
FHE_STREAM_BITS = 1                          # flag of fhe_tfhe_stream_words_dev: every word AND 1
FHE_STREAM_BFV_MASK, FHE_STREAM_BFV_ERR, FHE_STREAM_BFV_KEY, FHE_STREAM_BFV_EPH = 0x11, 0x12, 0x13, 0x14    # the BFV rows of that stream
FHE_STREAM_CKKS_MASK, FHE_STREAM_CKKS_ERR, FHE_STREAM_CKKS_KEY, FHE_STREAM_CKKS_EPH = 0x21, 0x22, 0x23, 0x24    # the CKKS rows


# include/fhe_ntt_experimental.h: the persistent kernels' switches (exported, NOT part of the boundary)
EXPORTS_EXPERIMENTAL = ["fhe_ntt_set_persist", "fhe_ntt_persist_status", "fhe_ntt_persist_profile", "fhe_ntt_set_persist_grid"]


class FheError(RuntimeError):
    """A non-zero return of the C ABI — the situations in which the reference panics."""

    def __init__(self, code, msg):
        super().__init__(f"fhe_ntt error {code}: {msg}")
        self.code = code


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def _deps(src):
    return [os.path.join(CSRC, src)] + [os.path.join(CSRC, h) for h in HEADERS]


def needs_build():
    return _stale(LIB_PATH, [d for s in SOURCES for d in _deps(s)])


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950: one object per source (only stale ones are recompiled),
    linked into fhe-study_amd/libfhe_ntt.so (in-tree, so it travels to the GPU box)."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs, procs = [], []
    for src in SOURCES:
        obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, _deps(src)):
            cmd = [hipcc] + HIPCC_FLAGS + ["-c", "-o", obj, os.path.join(CSRC, src)]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:   # sources compile in parallel (3 processes)
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return LIB_PATH


_u64 = ctypes.c_uint64
_p64 = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_int = ctypes.c_int

_lib = None


def _preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).
    Two HIP runtimes in one process cannot both own the GPU, so if torch is installed its
    copy is loaded first and libfhe_ntt.so binds to it — whichever of the two the process
    imports first.  torch itself is NOT imported here."""
    if "torch" in sys.modules:
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass  # fall back to the loader's default search (RUNPATH /opt/rocm/lib)


def load_library():
    """dlopen the in-tree library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing — run `python -c 'import __graft_entry__ as g; g.build()'`; "
            "there is no fallback path")
    _preload_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    L.fhe_ntt_version.restype = ctypes.c_char_p
    if b"ABLATED" in L.fhe_ntt_version() and os.environ.get("FHE_NTT_ALLOW_ABLATED") != "1":
        # a timing-only build (tools/abl_build.sh: kernels that skip work and return wrong words by design), reached
        # through a stray FHE_NTT_LIB or -D flag: never run tests or benches on it by accident
        raise RuntimeError(f"{LIB_PATH} reports {L.fhe_ntt_version().decode()!r}: a timing-only build with wrong results "
                           "by design; set FHE_NTT_ALLOW_ABLATED=1 to load it on purpose (tools/abl_*.py do)")
    L.fhe_ntt_plan_get.argtypes = [_u64, _u64, ctypes.POINTER(_vp)]
    L.fhe_ntt_plan_info.argtypes = [_vp, _p64, _p64, _p64, _p64]
    L.fhe_ntt_plan_tables.argtypes = [_vp, _p64, _p64]
    L.fhe_ntt_forward.argtypes = [_vp, _vp, _vp, _sz]
    L.fhe_ntt_inverse.argtypes = [_vp, _vp, _vp, _sz]
    L.fhe_rq_mul.argtypes = [_vp, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _sz]
    L.fhe_rq_mul_checked.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _sz]
    L.fhe_rq_pointwise_mul.argtypes = [_vp, _vp, _vp, _vp, _sz]
    L.fhe_rq_check_canonical.argtypes = [_vp, _vp, _sz]
    L.fhe_ntt_forward_dev.argtypes = [_vp, _vp, _vp, _sz, _vp]
    L.fhe_ntt_inverse_dev.argtypes = [_vp, _vp, _vp, _sz, _vp]
    L.fhe_rq_mul_dev.argtypes = [_vp, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _sz, _vp, _vp]
    L.fhe_rq_mul_workspace_bytes.argtypes = [_vp, _sz]
    L.fhe_rq_mul_workspace_bytes.restype = _sz
    L.fhe_rq_pointwise_mul_dev.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp]
    L.fhe_fill_synthetic_dev.argtypes = [_u64, _u64, _u64, _sz, _vp, _vp]
    L.fhe_ntt_set_batch_tile.argtypes = [_sz]
    L.fhe_ntt_set_persist.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
    L.fhe_ntt_persist_status.argtypes = []
    L.fhe_ntt_persist_profile.argtypes = [_vp]
    L.fhe_ntt_set_persist_grid.argtypes = [_int]
    L.fhe_ntt_kernel_timing_enable.argtypes = [_int]
    L.fhe_ntt_kernel_timing_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), _p64, _int]
    L.fhe_ntt_kernel_timing_reset.argtypes = []
    _i64p = ctypes.POINTER(ctypes.c_int64)
    _uint = ctypes.c_uint
    L.fhe_r_naive_mul.argtypes = [_u64, _vp, _vp, _vp, _sz]
    L.fhe_r_naive_mul_dev.argtypes = [_u64, _vp, _vp, _vp, _sz, _uint, _uint, _vp]
    L.fhe_mul_div_round_dev.argtypes = [_u64, _u64, _vp, _u64, _u64, _vp, _sz, _vp]
    L.fhe_bfv_tensor.argtypes = [_u64, _u64, _u64, _vp, _vp, _sz]
    L.fhe_bfv_tensor_dev.argtypes = [_u64, _u64, _u64, _vp, _vp, _sz, _vp]
    L.fhe_bfv_relinearize_dev.argtypes = [_u64, _u64, _u64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_bfv_mul.argtypes = [_u64, _u64, _u64, _u64, _vp, _vp, _vp, _sz]
    L.fhe_bfv_mul_dev.argtypes = [_u64, _u64, _u64, _u64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tn_mul.argtypes = [_u64, _vp, _vp, _vp, _sz]
    L.fhe_tn_mul_dev.argtypes = [_u64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tggsw_external_product.argtypes = [_u64, _uint, _uint, _vp, _vp, _vp, _sz]
    L.fhe_tggsw_external_product_dev.argtypes = [_u64, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_bfv_rlk_prepared_words.argtypes = [_u64, _u64, _u64]
    L.fhe_bfv_rlk_prepared_words.restype = _sz
    L.fhe_bfv_rlk_prepare_dev.argtypes = [_u64, _u64, _u64, _vp, _vp, _vp]
    L.fhe_bfv_relinearize_prepared_dev.argtypes = [_u64, _u64, _u64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_bfv_mul_prepared_dev.argtypes = [_u64, _u64, _u64, _u64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tggsw_prepared_words.argtypes = [_u64, _uint, _uint]
    L.fhe_tggsw_prepared_words.restype = _sz
    L.fhe_tggsw_prepare_dev.argtypes = [_u64, _uint, _uint, _vp, _vp, _vp]
    L.fhe_tggsw_external_product_prepared_dev.argtypes = [_u64, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_bsk_prepared_words.argtypes = [_u64, _uint, _uint, _uint]
    L.fhe_tfhe_bsk_prepared_words.restype = _sz
    L.fhe_tfhe_bsk_prepare_dev.argtypes = [_u64, _uint, _uint, _uint, _vp, _vp, _vp]
    L.fhe_tfhe_blind_rotation_dev.argtypes = [_u64, _uint, _uint, _uint, _vp, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tglwe_sample_extraction_dev.argtypes = [_u64, _uint, _uint, _vp, _vp, _sz, _vp]
    L.fhe_tlwe_key_switch_dev.argtypes = [_uint, _uint, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_bootstrap_dev.argtypes = [_u64, _uint, _uint, _uint, _vp, _vp, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tn_gadget_decompose_dev.argtypes = [_u64, _uint, _uint, _vp, _vp, _sz, _vp]
    L.fhe_tggsw_gadget_prepared_words.argtypes = [_u64, _uint, _uint, _uint]
    L.fhe_tggsw_gadget_prepared_words.restype = _sz
    L.fhe_tggsw_gadget_prepare_dev.argtypes = [_u64, _uint, _uint, _uint, _vp, _vp, _vp]
    L.fhe_tggsw_gadget_external_product_dev.argtypes = [_u64, _uint, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_gadget_bsk_prepared_words.argtypes = [_u64, _uint, _uint, _uint, _uint]
    L.fhe_tfhe_gadget_bsk_prepared_words.restype = _sz
    L.fhe_tfhe_gadget_bsk_prepare_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _vp, _vp]
    L.fhe_tfhe_gadget_blind_rotation_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tlwe_gadget_key_switch_dev.argtypes = [_uint, _uint, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_gadget_bootstrap_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _vp, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_pfksk_words.argtypes = [_u64, _uint, _uint, _uint]
    L.fhe_tfhe_pfksk_words.restype = _sz
    L.fhe_tlwe_gadget_private_key_switch_dev.argtypes = [_u64, _uint, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tggsw_gadget_prepare_many_dev.argtypes = [_u64, _uint, _uint, _uint, _sz, _vp, _vp, _vp]
    L.fhe_tggsw_gadget_cmux_dev.argtypes = [_u64, _uint, _uint, _uint, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_circuit_bootstrap_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _uint, _uint, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_gate_bootstrap_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _uint, _uint, _vp, _vp, _sz, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_gate_mux_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _uint, _uint, _vp, _vp, _sz, _vp, _vp, _sz, _vp]
    L.fhe_tlwe_lincomb_dev.argtypes = [_uint, _vp, _sz, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_lut_bootstrap_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _uint, _uint, _vp, _uint, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_lut_many_bootstrap_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _uint, _uint, _vp, _uint, _uint, _vp, _sz, _vp, _sz, _vp, _vp,
                                                  _sz, _vp]
    L.fhe_tfhe_pksk_words.argtypes = [_u64, _uint, _uint, _uint, _uint]
    L.fhe_tfhe_pksk_words.restype = _sz
    L.fhe_tlwe_gadget_packing_key_switch_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _vp, _sz, _sz, _sz, _uint, _vp, _sz, _vp]
    L.fhe_tglwe_box_expand_dev.argtypes = [_u64, _uint, _uint, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_gadget_bootstrap_rows_dev.argtypes = [_u64, _uint, _uint, _uint, _uint, _vp, _vp, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tfhe_stream_words_dev.argtypes = [ctypes.c_char_p, _uint, _u64, _u64, _uint, _vp, _sz, _vp]
    L.fhe_tlwe_encrypt_dev.argtypes = [_uint, ctypes.c_char_p, _u64, _vp, _vp, _vp, _uint, _uint, _vp, _sz, _vp]
    L.fhe_tlwe_phase_dev.argtypes = [_uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tglwe_encrypt_dev.argtypes = [_u64, _uint, ctypes.c_char_p, _u64, _vp, _vp, _sz, _vp, _uint, _uint, _vp, _sz, _vp]
    L.fhe_tglwe_phase_dev.argtypes = [_u64, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_bfv_secret_key_dev.argtypes = [_u64, ctypes.c_char_p, _u64, _vp, _vp]
    L.fhe_bfv_public_key_dev.argtypes = [_vp, ctypes.c_char_p, _u64, _vp, _vp, _uint, _vp, _vp]
    L.fhe_bfv_relin_key_dev.argtypes = [_u64, _u64, _u64, ctypes.c_char_p, _u64, _vp, _vp, _uint, _vp, _vp]
    L.fhe_bfv_encrypt_dev.argtypes = [_vp, _u64, ctypes.c_char_p, _u64, _vp, _vp, _sz, _vp, _uint, _vp, _sz, _vp]
    L.fhe_bfv_decrypt_dev.argtypes = [_vp, _u64, _vp, _vp, _vp, _sz, _vp]
    _f64 = ctypes.c_double
    L.fhe_ckks_twiddles.argtypes = [_u64, _vp]
    L.fhe_ckks_encode_dev.argtypes = [_u64, _f64, _vp, _vp, _sz, _vp, _sz, _vp]
    L.fhe_ckks_decode_dev.argtypes = [_u64, _f64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_ckks_embed_twiddles.argtypes = [_u64, _vp]
    L.fhe_ckks_embed_encode_dev.argtypes = [_u64, _f64, _vp, _vp, _sz, _vp, _sz, _vp]
    L.fhe_ckks_embed_decode_dev.argtypes = [_u64, _f64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_ckks_embed_workspace_bytes.argtypes = [_u64, _sz]
    L.fhe_ckks_embed_workspace_bytes.restype = _sz
    L.fhe_ckks_secret_key_dev.argtypes = [_vp, ctypes.c_char_p, _u64, _vp, _vp]
    L.fhe_ckks_public_key_dev.argtypes = [_vp, ctypes.c_char_p, _u64, _vp, _vp, _uint, _vp, _vp]
    L.fhe_ckks_encrypt_dev.argtypes = [_vp, ctypes.c_char_p, _u64, _vp, _vp, _sz, _vp, _uint, _vp, _sz, _vp]
    L.fhe_ckks_decrypt_dev.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp]
    _pp = ctypes.POINTER(_vp)
    L.fhe_ckks_rns_from_i64_dev.argtypes = [_pp, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_relin_key_dev.argtypes = [_pp, _uint, _vp, ctypes.c_char_p, _u64, _vp, _vp, _uint, _vp, _vp]
    L.fhe_ckks_rns_tensor_dev.argtypes = [_pp, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_relinearize_dev.argtypes = [_pp, _uint, _vp, _vp, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_mul_dev.argtypes = [_pp, _uint, _vp, _vp, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_rescale_dev.argtypes = [_pp, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_workspace_bytes.argtypes = [_u64, _uint, _sz]
    L.fhe_ckks_rns_workspace_bytes.restype = _sz
    L.fhe_ckks_galois_evals_dev.argtypes = [_vp, _u64, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_galois_key_dev.argtypes = [_pp, _uint, _vp, ctypes.c_char_p, _u64, _u64, _vp, _vp, _uint, _vp, _vp]
    L.fhe_ckks_rns_galois_dev.argtypes = [_pp, _uint, _vp, _pp, ctypes.POINTER(_u64), _uint, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_galois_workspace_bytes.argtypes = [_u64, _uint, _sz, _uint]
    L.fhe_ckks_rns_galois_workspace_bytes.restype = _sz
    L.fhe_ckks_rns_diag_sum_dev.argtypes = [_pp, _uint, _vp, _pp, ctypes.POINTER(_u64), _uint, _uint, _vp, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_diag_workspace_bytes.argtypes = [_u64, _uint, _sz, _uint, _uint]
    L.fhe_ckks_rns_diag_workspace_bytes.restype = _sz
    L.fhe_ckks_rns_bsgs_dev.argtypes = [_pp, _uint, _vp, _pp, ctypes.POINTER(_u64), _uint, _pp, ctypes.POINTER(_u64), _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_ckks_rns_bsgs_workspace_bytes.argtypes = [_u64, _uint, _sz, _uint, _uint]
    L.fhe_ckks_rns_bsgs_workspace_bytes.restype = _sz
    L.fhe_ckks_rns_lincomb_dev.argtypes = [_pp, _uint, _pp, _uint, ctypes.POINTER(_u64), ctypes.POINTER(_u64), _uint, _vp, _sz, _vp]
    L.fhe_ckks_deep_relin_key_dev.argtypes = [_pp, _uint, _pp, _uint, ctypes.c_char_p, _u64, _vp, _vp, _uint, _vp, _vp]
    L.fhe_ckks_deep_galois_key_dev.argtypes = [_pp, _uint, _pp, _uint, ctypes.c_char_p, _u64, _u64, _vp, _vp, _uint, _vp, _vp]
    L.fhe_ckks_deep_relinearize_dev.argtypes = [_pp, _uint, _pp, _uint, _vp, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_deep_mul_dev.argtypes = [_pp, _uint, _pp, _uint, _vp, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_ckks_deep_galois_dev.argtypes = [_pp, _uint, _pp, _uint, _pp, ctypes.POINTER(_u64), _uint, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_deep_rescale_dev.argtypes = [_pp, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_deep_workspace_bytes.argtypes = [_u64, _uint, _uint, _sz]
    L.fhe_ckks_deep_workspace_bytes.restype = _sz
    L.fhe_ckks_deep_diag_sum_dev.argtypes = [_pp, _uint, _pp, _uint, _pp, ctypes.POINTER(_u64), _uint, _uint, _vp, _uint, _vp, _vp, _sz, _vp]
    L.fhe_ckks_deep_diag_workspace_bytes.argtypes = [_u64, _uint, _uint, _sz, _uint, _uint]
    L.fhe_ckks_deep_diag_workspace_bytes.restype = _sz
    L.fhe_ckks_deep_lincomb_dev.argtypes = [_pp, _uint, _pp, _uint, ctypes.POINTER(_u64), ctypes.POINTER(_u64), _uint, _vp, _sz, _vp]
    L.fhe_ckks_deep_dot_dev.argtypes = [_pp, _uint, _pp, _uint, _vp, _uint, _pp, _pp, _uint, ctypes.POINTER(_u64), _vp, _sz, _vp]
    L.fhe_ckks_rns_dot_dev.argtypes = [_pp, _uint, _vp, _vp, _uint, _pp, _pp, _uint, ctypes.POINTER(_u64), _vp, _sz, _vp]
    L.fhe_rns_extend_dev.argtypes = [ctypes.POINTER(_u64), _uint, ctypes.POINTER(_u64), _uint, _int, _vp, _vp, _sz, _vp]
    L.fhe_bfv_rns_tensor_dev.argtypes = [_pp, _uint, _pp, _u64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_bfv_rns_mul_dev.argtypes = [_pp, _uint, _pp, _vp, _u64, _vp, _vp, _vp, _vp, _sz, _vp]
    L.fhe_bfv_rns_dot_dev.argtypes = [_pp, _uint, _pp, _vp, _u64, _vp, _pp, _pp, _uint, ctypes.POINTER(ctypes.c_int64), _vp, _sz, _vp]
    L.fhe_bfv_rns_workspace_bytes.argtypes = [_u64, _uint, _sz]
    L.fhe_bfv_rns_workspace_bytes.restype = _sz
    L.fhe_bfv_rns_scale_msg_dev.argtypes = [_pp, _uint, _u64, _vp, _vp, _sz, _vp]
    L.fhe_bfv_rns_decrypt_dev.argtypes = [_pp, _uint, _u64, _u64, _vp, _vp, _vp, _sz, _vp]
    L.fhe_glwe_ksk_prepared_words.argtypes = [_vp, _uint, _uint, _uint]
    L.fhe_glwe_ksk_prepared_words.restype = _sz
    L.fhe_glwe_ksk_prepare_dev.argtypes = [_vp, _uint, _uint, _uint, _vp, _vp, _vp]
    L.fhe_glwe_key_switch_prepared_dev.argtypes = [_vp, _uint, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tr_dot_dev.argtypes = [_vp, _vp, _vp, _vp, _uint, _sz, _uint, _vp]
    L.fhe_tr_mul_r_dev.argtypes = [_vp, _vp, _vp, _vp, _uint, _sz, _uint, _vp]
    L.fhe_glev_mul_dev.argtypes = [_vp, _uint, _uint, _vp, _vp, _vp, _sz, _uint, _vp]
    L.fhe_glwe_key_switch_dev.argtypes = [_vp, _uint, _uint, _uint, _vp, _vp, _vp, _sz, _uint, _vp]
    L.fhe_tglwe_mul_tn.argtypes = [_u64, _uint, _vp, _vp, _vp, _sz]
    L.fhe_tglwe_mul_tn_dev.argtypes = [_u64, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tglev_mul.argtypes = [_u64, _uint, _uint, _vp, _vp, _vp, _sz]
    L.fhe_tglev_mul_dev.argtypes = [_u64, _uint, _uint, _vp, _vp, _vp, _sz, _vp]
    L.fhe_tr_dot.argtypes = [_vp, _vp, _vp, _vp, _uint, _sz]
    L.fhe_tr_mul_r.argtypes = [_vp, _vp, _vp, _vp, _uint, _sz]
    L.fhe_glev_mul.argtypes = [_vp, _uint, _uint, _vp, _vp, _vp, _sz]
    L.fhe_glwe_key_switch.argtypes = [_vp, _uint, _uint, _uint, _vp, _vp, _vp, _sz]
    L.fhe_rq_add_dev.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp]
    L.fhe_rq_sub_dev.argtypes = [_vp, _vp, _vp, _vp, _sz, _vp]
    L.fhe_rq_neg_dev.argtypes = [_vp, _vp, _vp, _sz, _vp]
    L.fhe_rq_mul_by_u64_dev.argtypes = [_vp, _vp, _u64, _vp, _sz, _vp]
    L.fhe_rq_mod_switch_dev.argtypes = [_u64, _u64, _vp, _vp, _sz, _vp]
    L.fhe_rq_mul_div_round_dev.argtypes = [_u64, _u64, _u64, _vp, _vp, _sz, _vp]
    L.fhe_rq_decompose_dev.argtypes = [_u64, _u64, _uint, _uint, _vp, _vp, _sz, _vp]
    L.fhe_rq_remodule_dev.argtypes = [_u64, _vp, _vp, _sz, _vp]
    L.fhe_rq_mul_by_f64_dev.argtypes = [_u64, ctypes.c_double, _vp, _vp, _sz, _vp]
    L.fhe_rq_div_round_dev.argtypes = [_u64, _u64, _vp, _vp, _sz, _vp]
    L.fhe_ntt_device_count.argtypes = []
    L.fhe_ntt_plan_prepare.argtypes = [_vp]
    L.fhe_ntt_plan_arithmetic.argtypes = [_vp]
    L.fhe_ntt_workspace_bytes.argtypes = []
    L.fhe_ntt_workspace_bytes.restype = _sz
    L.fhe_ntt_release_stream_workspace.argtypes = [_vp]
    L.fhe_ntt_set_check_canonical.argtypes = [_int]
    L.fhe_shard_range.argtypes = [_sz, _uint, _uint, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]
    L.fhe_shard_gather_dev.argtypes = [_sz, _sz, _uint, ctypes.POINTER(_int), ctypes.POINTER(_vp), _int, _vp, _vp]
    L.fhe_last_error.restype = ctypes.c_char_p
    L.fhe_ntt_version.restype = ctypes.c_char_p
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is ctypes.c_int and name not in ("fhe_last_error", "fhe_ntt_version"):
            fn.restype = ctypes.c_int
    _lib = L
    return L


def _check(rc):
    if rc != FHE_OK:
        raise FheError(rc, load_library().fhe_last_error().decode())


def _host(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(_vp)


class Plan:
    """(q,n)-keyed plan — the reference's `roots(q,n)` cache entry, arith/src/ntt.rs:18-38."""

    def __init__(self, q, n):
        L = load_library()
        h = _vp()
        _check(L.fhe_ntt_plan_get(int(q), int(n), ctypes.byref(h)))
        self.handle = h
        self.q, self.n = int(q), int(n)

    ARITH_NAMES = {0: "shoup62", 1: "shoup61", 2: "pseudo-mersenne", 3: "word32", 4: "strict63", 5: "montgomery"}

    def arithmetic(self):
        """fhe_ntt_plan_arithmetic: which exact form of Zq::mul the transform kernels run for this modulus"""
        rc = load_library().fhe_ntt_plan_arithmetic(self.handle)
        if rc < 0:
            _check(rc)
        return rc

    def info(self):
        q, n, psi, ninv = _u64(), _u64(), _u64(), _u64()
        _check(load_library().fhe_ntt_plan_info(self.handle, q, n, psi, ninv))
        return dict(q=q.value, n=n.value, psi=psi.value, n_inv=ninv.value)

    def tables(self):
        r = np.empty(self.n, dtype=np.uint64)
        ri = np.empty(self.n, dtype=np.uint64)
        _check(load_library().fhe_ntt_plan_tables(self.handle, r.ctypes.data_as(_p64),
                                                  ri.ctypes.data_as(_p64)))
        return r, ri

    # -- host buffers ---------------------------------------------------------
    def _batch(self, a):
        if a.size % self.n:
            raise ValueError(f"array of {a.size} values is not a whole number of n={self.n} polynomials")
        return a.size // self.n

    def forward(self, a):
        a, pa = _host(a)
        out = np.empty_like(a)
        _check(load_library().fhe_ntt_forward(self.handle, pa, out.ctypes.data_as(_vp), self._batch(a)))
        return out

    def inverse(self, a):
        a, pa = _host(a)
        out = np.empty_like(a)
        _check(load_library().fhe_ntt_inverse(self.handle, pa, out.ctypes.data_as(_vp), self._batch(a)))
        return out

    def rq_mul(self, a, b, a_is_evals=False, b_is_evals=False, want_evals=True):
        """→ (c, c_evals, a_evals, b_evals); the last three are None unless want_evals."""
        a, pa = _host(a)
        b, pb = _host(b)
        if a.shape != b.shape:
            raise ValueError("operand shapes differ")
        c = np.empty_like(a)
        ce = np.empty_like(a) if want_evals else None
        ae = np.empty_like(a) if want_evals else None
        be = np.empty_like(a) if want_evals else None
        p = lambda x: x.ctypes.data_as(_vp) if x is not None else None
        _check(load_library().fhe_rq_mul(self.handle, pa, int(a_is_evals), pb, int(b_is_evals),
                                         p(c), p(ce), p(ae), p(be), self._batch(a)))
        return c, ce, ae, be

    def pointwise_mul(self, a, b):
        a, pa = _host(a)
        b, pb = _host(b)
        c = np.empty_like(a)
        _check(load_library().fhe_rq_pointwise_mul(self.handle, pa, pb, c.ctypes.data_as(_vp),
                                                   self._batch(a)))
        return c

    def check_canonical(self, a):
        a, pa = _host(a)
        _check(load_library().fhe_rq_check_canonical(self.handle, pa, self._batch(a)))

    # -- device pointers (ints), stream handle (int or None) -----------------------
    def forward_dev(self, d_in, d_out, batch, stream=None):
        _check(load_library().fhe_ntt_forward_dev(self.handle, d_in, d_out, batch, stream))

    def inverse_dev(self, d_in, d_out, batch, stream=None):
        _check(load_library().fhe_ntt_inverse_dev(self.handle, d_in, d_out, batch, stream))

    def rq_mul_dev(self, d_a, d_b, d_c, batch, a_is_evals=False, b_is_evals=False, d_c_evals=None,
                   d_a_evals=None, d_b_evals=None, d_work=None, stream=None):
        _check(load_library().fhe_rq_mul_dev(self.handle, d_a, int(a_is_evals), d_b, int(b_is_evals),
                                             d_c, d_c_evals, d_a_evals, d_b_evals, batch, d_work, stream))

    def pointwise_mul_dev(self, d_a, d_b, d_c, batch, stream=None):
        _check(load_library().fhe_rq_pointwise_mul_dev(self.handle, d_a, d_b, d_c, batch, stream))

    def workspace_bytes(self, batch):
        return int(load_library().fhe_rq_mul_workspace_bytes(self.handle, batch))


def rq_mul_checked(plan_a, plan_b, a, b):
    a, pa = _host(a)
    b, pb = _host(b)
    c = np.empty_like(a)
    _check(load_library().fhe_rq_mul_checked(plan_a.handle, plan_b.handle, pa, pb,
                                             c.ctypes.data_as(_vp), None, a.size // plan_a.n))
    return c


# ---- next rows: exact products over Z / mod 2^64 (host buffers) -----------------------------

def r_naive_mul(n, a, b):
    """arith::ring_n::naive_mul (ring_n.rs:307-320) → (batch, 2n-1) int64"""
    a = np.ascontiguousarray(a, dtype=np.int64)
    b = np.ascontiguousarray(b, dtype=np.int64)
    batch = a.size // n
    out = np.empty(batch * 2 * n, dtype=np.int64)
    _check(load_library().fhe_r_naive_mul(n, a.ctypes.data_as(_vp), b.ctypes.data_as(_vp),
                                          out.ctypes.data_as(_vp), batch))
    return out.reshape(batch, 2 * n)[:, :2 * n - 1]


def bfv_tensor(q, n, t, a0, a1, b0, b1):
    """RLWE::tensor (bfv/src/lib.rs:59-85) → (c0, c1, c2), each (batch, n)"""
    ab = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.uint64).reshape(-1, n) for x in (a0, a1, b0, b1)]))
    batch = ab.shape[1]
    c = np.empty((3, batch, n), dtype=np.uint64)
    _check(load_library().fhe_bfv_tensor(q, n, t, ab.ctypes.data_as(_vp), c.ctypes.data_as(_vp), batch))
    return c[0], c[1], c[2]


def bfv_mul(q, n, t, pq, rlk0, rlk1, a0, a1, b0, b1):
    """RLWE::mul (bfv/src/lib.rs:87-90) → (o0, o1), each (batch, n)"""
    ab = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.uint64).reshape(-1, n) for x in (a0, a1, b0, b1)]))
    rlk = np.ascontiguousarray(np.stack([np.asarray(rlk0, dtype=np.uint64), np.asarray(rlk1, dtype=np.uint64)]))
    batch = ab.shape[1]
    out = np.empty((2, batch, n), dtype=np.uint64)
    _check(load_library().fhe_bfv_mul(q, n, t, pq, rlk.ctypes.data_as(_vp), ab.ctypes.data_as(_vp),
                                      out.ctypes.data_as(_vp), batch))
    return out[0], out[1]


def tn_mul(n, a, b):
    """Tn x Tn (ring_torus.rs:266-298) → (batch, n) uint64"""
    a, pa = _host(a)
    b, pb = _host(b)
    out = np.empty_like(a)
    _check(load_library().fhe_tn_mul(n, pa, pb, out.ctypes.data_as(_vp), a.size // n))
    return out


def tglwe_mul_tn(n, k, tglwe, p):
    """TGLWE x Tn (tfhe/src/tglwe.rs:182-194); tglwe [batch][(k+1)][n], p [batch][n]"""
    c, pc = _host(tglwe)
    t, pt = _host(p)
    out = np.empty_like(c)
    _check(load_library().fhe_tglwe_mul_tn(n, k, pc, pt, out.ctypes.data_as(_vp), t.size // n))
    return out


def tglev_mul(n, k, l, tglev, v):
    """TGLev x Vec<Tn> (tfhe/src/tggsw.rs:139-149); tglev [l][(k+1)][n], v [batch][l][n] -> [batch][(k+1)][n]"""
    g, pg = _host(tglev)
    d, pd = _host(v)
    batch = d.size // (l * n)
    out = np.empty(batch * (k + 1) * n, dtype=np.uint64)
    _check(load_library().fhe_tglev_mul(n, k, l, pg, pd, out.ctypes.data_as(_vp), batch))
    return out.reshape(batch, k + 1, n)


def tggsw_external_product(n, k, l, tggsw, tglwe):
    """TGGSW x TGLWE (tfhe/src/tggsw.rs:45-62); tggsw [(k+1)][l][(k+1)][n], tglwe [batch][(k+1)][n]"""
    g, pg = _host(tggsw)
    t, pt = _host(tglwe)
    batch = t.size // ((k + 1) * n)
    out = np.empty_like(t)
    _check(load_library().fhe_tggsw_external_product(n, k, l, pg, pt, out.ctypes.data_as(_vp), batch))
    return out


def fill_synthetic_dev(q, seed, first_index, count, d_out, stream=None):
    _check(load_library().fhe_fill_synthetic_dev(int(q), int(seed), int(first_index), int(count),
                                                 d_out, stream))


# ---- TFHE bootstrapping (include/fhe_ntt.h; device pointers as ints, words u64) ----------------------------------------
def tfhe_bsk_prepared_words(n, k, l, n_lwe):
    return load_library().fhe_tfhe_bsk_prepared_words(n, k, l, n_lwe)


def tfhe_bsk_prepare_dev(n, k, l, n_lwe, d_bsk, d_prepared, stream=None):
    _check(load_library().fhe_tfhe_bsk_prepare_dev(n, k, l, n_lwe, d_bsk, d_prepared, stream))


def tfhe_blind_rotation_dev(n, k, l, n_lwe, d_bsk_prepared, d_table, d_lwe, d_out, batch, stream=None):
    _check(load_library().fhe_tfhe_blind_rotation_dev(n, k, l, n_lwe, d_bsk_prepared, d_table, d_lwe, d_out, batch, stream))


def tglwe_sample_extraction_dev(n, k, h, d_tglwe, d_tlwe, batch, stream=None):
    _check(load_library().fhe_tglwe_sample_extraction_dev(n, k, h, d_tglwe, d_tlwe, batch, stream))


def tlwe_key_switch_dev(n_in, n_out, beta, l, d_ksk, d_in, d_out, batch, stream=None):
    _check(load_library().fhe_tlwe_key_switch_dev(n_in, n_out, beta, l, d_ksk, d_in, d_out, batch, stream))


def tfhe_bootstrap_dev(n, k, l, n_lwe, d_bsk_prepared, d_table, ks_l, d_ksk, d_in, d_out, batch, stream=None):
    _check(load_library().fhe_tfhe_bootstrap_dev(n, k, l, n_lwe, d_bsk_prepared, d_table, ks_l, d_ksk, d_in, d_out, batch, stream))


# ---- the signed base-2^b gadget (log_beta = b) --------------------------------------------------------
def tn_gadget_decompose_dev(n, log_beta, l, d_a, d_out, rows, stream=None):
    _check(load_library().fhe_tn_gadget_decompose_dev(n, log_beta, l, d_a, d_out, rows, stream))


def tggsw_gadget_prepared_words(n, k, log_beta, l):
    return load_library().fhe_tggsw_gadget_prepared_words(n, k, log_beta, l)


def tggsw_gadget_prepare_dev(n, k, log_beta, l, d_tggsw, d_prepared, stream=None):
    _check(load_library().fhe_tggsw_gadget_prepare_dev(n, k, log_beta, l, d_tggsw, d_prepared, stream))


def tggsw_gadget_external_product_dev(n, k, log_beta, l, d_prepared, d_tglwe, d_out, batch, stream=None):
    _check(load_library().fhe_tggsw_gadget_external_product_dev(n, k, log_beta, l, d_prepared, d_tglwe, d_out, batch, stream))


def tfhe_gadget_bsk_prepared_words(n, k, log_beta, l, n_lwe):
    return load_library().fhe_tfhe_gadget_bsk_prepared_words(n, k, log_beta, l, n_lwe)


def tfhe_gadget_bsk_prepare_dev(n, k, log_beta, l, n_lwe, d_bsk, d_prepared, stream=None):
    _check(load_library().fhe_tfhe_gadget_bsk_prepare_dev(n, k, log_beta, l, n_lwe, d_bsk, d_prepared, stream))


def tfhe_gadget_blind_rotation_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, d_table, d_lwe, d_out, batch, stream=None):
    _check(load_library().fhe_tfhe_gadget_blind_rotation_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, d_table, d_lwe, d_out, batch,
                                                             stream))


def tlwe_gadget_key_switch_dev(n_in, n_out, log_beta, l, d_ksk, d_in, d_out, batch, stream=None):
    _check(load_library().fhe_tlwe_gadget_key_switch_dev(n_in, n_out, log_beta, l, d_ksk, d_in, d_out, batch, stream))


def tfhe_gadget_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, d_table, ks_log_beta, ks_l, d_ksk, d_in, d_out, batch,
                              stream=None):
    _check(load_library().fhe_tfhe_gadget_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, d_table, ks_log_beta, ks_l, d_ksk,
                                                        d_in, d_out, batch, stream))


# ---- circuit bootstrapping ----------------------------------------------------------------------------
def tfhe_pfksk_words(n, k, log_beta, l):
    return load_library().fhe_tfhe_pfksk_words(n, k, log_beta, l)


def tlwe_gadget_private_key_switch_dev(n, k, log_beta, l, d_pfksk, d_in, d_out, batch, stream=None):
    _check(load_library().fhe_tlwe_gadget_private_key_switch_dev(n, k, log_beta, l, d_pfksk, d_in, d_out, batch, stream))


def tggsw_gadget_prepare_many_dev(n, k, log_beta, l, count, d_tggsw, d_prepared, stream=None):
    _check(load_library().fhe_tggsw_gadget_prepare_many_dev(n, k, log_beta, l, count, d_tggsw, d_prepared, stream))


def tggsw_gadget_cmux_dev(n, k, log_beta, l, count, d_prepared, d_idx, d_c0, d_c1, d_out, batch, stream=None):
    _check(load_library().fhe_tggsw_gadget_cmux_dev(n, k, log_beta, l, count, d_prepared, d_idx, d_c0, d_c1, d_out, batch, stream))


def tfhe_circuit_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, cb_log_beta, cb_l, pf_log_beta, pf_l, d_pfksk, d_lwe, d_out,
                               batch, stream=None):
    _check(load_library().fhe_tfhe_circuit_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, cb_log_beta, cb_l, pf_log_beta, pf_l,
                                                         d_pfksk, d_lwe, d_out, batch, stream))


# ---- boolean gates with gate bootstrapping ---------------------------------------------------------------
def tfhe_gate_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, d_pool, wires, d_gates, d_out, batch,
                            stream=None):
    _check(load_library().fhe_tfhe_gate_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, d_pool, wires,
                                                      d_gates, d_out, batch, stream))


def tfhe_gate_mux_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, d_pool, wires, d_sel, d_out, batch, stream=None):
    _check(load_library().fhe_tfhe_gate_mux_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, d_pool, wires, d_sel,
                                                d_out, batch, stream))


# ---- small integers: a lookup table per row ----------------------------------------------------------------
def tlwe_lincomb_dev(n_lwe, d_pool, wires, d_desc, d_out, batch, stream=None):
    _check(load_library().fhe_tlwe_lincomb_dev(n_lwe, d_pool, wires, d_desc, d_out, batch, stream))


def tfhe_lut_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, t_bits, d_luts, lut_count, d_pool, wires,
                           d_desc, d_out, batch, stream=None):
    _check(load_library().fhe_tfhe_lut_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, t_bits, d_luts,
                                                     lut_count, d_pool, wires, d_desc, d_out, batch, stream))


def tfhe_lut_many_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, t_bits, nu, d_luts, lut_count, d_pool,
                                wires, d_desc, d_out, batch, stream=None):
    """d_out [2^nu][batch][n_lwe + 1], function-major"""
    _check(load_library().fhe_tfhe_lut_many_bootstrap_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, ks_log_beta, ks_l, d_ksk, t_bits, nu,
                                                          d_luts, lut_count, d_pool, wires, d_desc, d_out, batch, stream))


# ---- packing key switch and the bootstrap with a test vector per row --------------------------------------
def tfhe_pksk_words(n, k, n_in, log_beta, l):
    return load_library().fhe_tfhe_pksk_words(n, k, n_in, log_beta, l)


def tlwe_gadget_packing_key_switch_dev(n, k, n_in, log_beta, l, d_pksk, d_in, in_group_stride, in_item_stride, count, log_stride, d_out, groups,
                                       stream=None):
    """d_out [groups][(k+1)][n]; ciphertext i of group g starts at word g in_group_stride + i in_item_stride of d_in"""
    _check(load_library().fhe_tlwe_gadget_packing_key_switch_dev(n, k, n_in, log_beta, l, d_pksk, d_in, in_group_stride, in_item_stride, count,
                                                                 log_stride, d_out, groups, stream))


def tglwe_box_expand_dev(n, k, t_bits, d_in, d_out, batch, stream=None):
    _check(load_library().fhe_tglwe_box_expand_dev(n, k, t_bits, d_in, d_out, batch, stream))


def tfhe_gadget_bootstrap_rows_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, d_tables, ks_log_beta, ks_l, d_ksk, d_in, d_out, batch, stream=None):
    """fhe_tfhe_gadget_bootstrap_dev with d_tables [batch][(k+1)][n]: a full TGLWE test vector per row"""
    _check(load_library().fhe_tfhe_gadget_bootstrap_rows_dev(n, k, log_beta, l, n_lwe, d_bsk_prepared, d_tables, ks_log_beta, ks_l, d_ksk, d_in,
                                                             d_out, batch, stream))


# ---- key generation, encryption and decryption (seed: 32 bytes, the ChaCha20 key) ---------------------------
def _seed(seed):
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError(f"the seed is the 32-byte ChaCha20 key ({len(seed)} bytes given)")
    return seed


def tfhe_stream_words_dev(seed, purpose, first_row, row_words, d_out, rows, bits=False, stream=None):
    """d_out [rows][row_words]: the stream words of rows first_row .. under `purpose`; bits: every word AND 1"""
    _check(load_library().fhe_tfhe_stream_words_dev(_seed(seed), purpose, first_row, row_words, FHE_STREAM_BITS if bits else 0, d_out, rows, stream))


def tlwe_encrypt_dev(n, seed, first_row, d_key, d_mu, d_cdt, m, log_scale, d_out, batch, stream=None):
    _check(load_library().fhe_tlwe_encrypt_dev(n, _seed(seed), first_row, d_key, d_mu, d_cdt, m, log_scale, d_out, batch, stream))


def tlwe_phase_dev(n, d_key, d_in, d_out, batch, stream=None):
    _check(load_library().fhe_tlwe_phase_dev(n, d_key, d_in, d_out, batch, stream))


def tglwe_encrypt_dev(n, k, seed, first_row, d_key, d_msg, msg_stride, d_cdt, m, log_scale, d_out, rows, stream=None):
    """d_msg None: M = 0; msg_stride 0: one message polynomial for every row"""
    _check(load_library().fhe_tglwe_encrypt_dev(n, k, _seed(seed), first_row, d_key, d_msg, msg_stride, d_cdt, m, log_scale, d_out, rows, stream))


def tglwe_phase_dev(n, k, d_key, d_in, d_out, rows, stream=None):
    _check(load_library().fhe_tglwe_phase_dev(n, k, d_key, d_in, d_out, rows, stream))


# ---- BFV key generation, encryption and decryption (plan: a Plan, seed: 32 bytes) ---------------------------
def bfv_secret_key_dev(n, seed, key_row, d_s, stream=None):
    """d_s [n]: the 0/1 words of KEY row key_row"""
    _check(load_library().fhe_bfv_secret_key_dev(n, _seed(seed), key_row, d_s, stream))


def bfv_public_key_dev(plan, seed, row, d_s, d_cdt, m, d_pk, stream=None):
    """d_pk [2][n] = (-a s + e, a) mod q"""
    _check(load_library().fhe_bfv_public_key_dev(plan.handle, _seed(seed), row, d_s, d_cdt, m, d_pk, stream))


def bfv_relin_key_dev(q, n, pq, seed, row, d_s, d_cdt, m, d_rlk, stream=None):
    """d_rlk [2][n] = (-(a s + e) + p s^2, a) mod pq, exactly"""
    _check(load_library().fhe_bfv_relin_key_dev(q, n, pq, _seed(seed), row, d_s, d_cdt, m, d_rlk, stream))


def bfv_encrypt_dev(plan, t, seed, first_row, d_pk_evals, d_msg, msg_stride, d_cdt, m, d_out, batch, stream=None):
    """d_out [2][batch][n]; d_msg None: m = 0; msg_stride 0: one message polynomial for every row"""
    _check(load_library().fhe_bfv_encrypt_dev(plan.handle, t, _seed(seed), first_row, d_pk_evals, d_msg, msg_stride, d_cdt, m, d_out, batch, stream))


def bfv_decrypt_dev(plan, t, d_s_evals, d_ct, d_out, batch, stream=None):
    """d_ct [2][batch][n] -> d_out [batch][n], words below t"""
    _check(load_library().fhe_bfv_decrypt_dev(plan.handle, t, d_s_evals, d_ct, d_out, batch, stream))


# ---- CKKS: the encoder and the client side (complex values are interleaved float64 pairs) ---------------------
def ckks_twiddles(n):
    """[n] complex128: exp(i pi k / n), k < n, the table the encoder kernels read (host only, no device)"""
    out = np.empty(n, dtype=np.complex128)
    _check(load_library().fhe_ckks_twiddles(n, out.ctypes.data_as(_vp)))
    return out


def ckks_encode_dev(n, delta, d_tw, d_z, z_stride, d_out, batch, stream=None):
    """d_z [batch][n/2] complex (z_stride in complex values; 0: one vector) -> d_out [batch][n] int64"""
    _check(load_library().fhe_ckks_encode_dev(n, delta, d_tw, d_z, z_stride, d_out, batch, stream))


def ckks_decode_dev(n, delta, d_tw, d_p, d_out, batch, stream=None):
    """d_p [batch][n] int64 -> d_out [batch][n/2] complex"""
    _check(load_library().fhe_ckks_decode_dev(n, delta, d_tw, d_p, d_out, batch, stream))


def ckks_embed_twiddles(n):
    """ckks_twiddles for n <= 2^16: the table of the ckks_embed_* calls"""
    out = np.empty(n, dtype=np.complex128)
    _check(load_library().fhe_ckks_embed_twiddles(n, out.ctypes.data_as(_vp)))
    return out


def ckks_embed_encode_dev(n, delta, d_tw, d_z, z_stride, d_out, batch, stream=None):
    """ckks_encode_dev for n <= 2^16: two passes through the library workspace above 2^13"""
    _check(load_library().fhe_ckks_embed_encode_dev(n, delta, d_tw, d_z, z_stride, d_out, batch, stream))


def ckks_embed_decode_dev(n, delta, d_tw, d_p, d_out, batch, stream=None):
    """ckks_decode_dev for n <= 2^16"""
    _check(load_library().fhe_ckks_embed_decode_dev(n, delta, d_tw, d_p, d_out, batch, stream))


def ckks_embed_workspace_bytes(n, batch):
    """the library workspace of one ckks_embed_* call; 0 for n <= 2^13 and for a refused shape"""
    return int(load_library().fhe_ckks_embed_workspace_bytes(n, batch))


def ckks_secret_key_dev(plan, seed, key_row, d_s, stream=None):
    """d_s [n]: the ternary secret of KEY row key_row as residues 0, 1, q - 1"""
    _check(load_library().fhe_ckks_secret_key_dev(plan.handle, _seed(seed), key_row, d_s, stream))


def ckks_public_key_dev(plan, seed, row, d_s, d_cdt, m, d_pk, stream=None):
    """d_pk [2][n] = (-a s + e, a) mod q"""
    _check(load_library().fhe_ckks_public_key_dev(plan.handle, _seed(seed), row, d_s, d_cdt, m, d_pk, stream))


def ckks_encrypt_dev(plan, seed, first_row, d_pk_evals, d_msg, msg_stride, d_cdt, m, d_out, batch, stream=None):
    """d_out [2][batch][n]; d_msg int64 rows (None: m = 0; msg_stride 0: one message polynomial for every row)"""
    _check(load_library().fhe_ckks_encrypt_dev(plan.handle, _seed(seed), first_row, d_pk_evals, d_msg, msg_stride, d_cdt, m, d_out, batch, stream))


def ckks_decrypt_dev(plan, d_s_evals, d_ct, d_out, batch, stream=None):
    """d_ct [2][batch][n] -> d_out [batch][n] int64, centred"""
    _check(load_library().fhe_ckks_decrypt_dev(plan.handle, d_s_evals, d_ct, d_out, batch, stream))


def _plan_array(plans):
    """a host array of plan handles; a None entry is passed as NULL"""
    return (_vp * max(len(plans), 1))(*[None if p is None else getattr(p, "handle", p) for p in plans])


def _handle(plan):
    return None if plan is None else getattr(plan, "handle", plan)


def ckks_rns_from_i64_dev(plans, d_in, d_out, batch, stream=None, limbs=None):
    """fhe_ckks_rns_from_i64_dev: signed rows [batch][n] -> evals [limbs][batch][n]"""
    _check(load_library().fhe_ckks_rns_from_i64_dev(_plan_array(plans), len(plans) if limbs is None else limbs, d_in, d_out, batch, stream))


def ckks_rns_relin_key_dev(plans, special, seed, first_row, d_s, d_cdt, m, d_rlk, stream=None, limbs=None):
    """fhe_ckks_rns_relin_key_dev: d_rlk [limbs][limbs + 1][2][n] evals from d_s [limbs + 1][n]"""
    _check(load_library().fhe_ckks_rns_relin_key_dev(_plan_array(plans), len(plans) if limbs is None else limbs, _handle(special), _seed(seed), first_row, d_s, d_cdt,
                                                     m, d_rlk, stream))


def ckks_rns_tensor_dev(plans, d_a, d_b, d_out, batch, stream=None, limbs=None):
    """fhe_ckks_rns_tensor_dev: [limbs][2][batch][n] x 2 -> [limbs][3][batch][n]"""
    _check(load_library().fhe_ckks_rns_tensor_dev(_plan_array(plans), len(plans) if limbs is None else limbs, d_a, d_b, d_out, batch, stream))


def ckks_rns_relinearize_dev(plans, special, d_rlk, key_limbs, d_d, d_out, batch, stream=None, limbs=None):
    """fhe_ckks_rns_relinearize_dev: [limbs][3][batch][n] -> [limbs][2][batch][n]"""
    _check(load_library().fhe_ckks_rns_relinearize_dev(_plan_array(plans), len(plans) if limbs is None else limbs, _handle(special), d_rlk, key_limbs, d_d, d_out,
                                                       batch, stream))


def ckks_rns_mul_dev(plans, special, d_rlk, key_limbs, d_a, d_b, d_out, batch, stream=None, limbs=None):
    """fhe_ckks_rns_mul_dev: the tensor and its relinearisation in one call"""
    _check(load_library().fhe_ckks_rns_mul_dev(_plan_array(plans), len(plans) if limbs is None else limbs, _handle(special), d_rlk, key_limbs, d_a, d_b, d_out, batch,
                                               stream))


def ckks_rns_rescale_dev(plans, d_in, d_out, batch, stream=None, limbs=None):
    """fhe_ckks_rns_rescale_dev: [limbs][2][batch][n] -> [limbs - 1][2][batch][n]"""
    _check(load_library().fhe_ckks_rns_rescale_dev(_plan_array(plans), len(plans) if limbs is None else limbs, d_in, d_out, batch, stream))


def ckks_rns_workspace_bytes(n, limbs, batch):
    return int(load_library().fhe_ckks_rns_workspace_bytes(n, limbs, batch))


def ckks_galois_evals_dev(plan, g, d_in, d_out, polys, stream=None):
    """fhe_ckks_galois_evals_dev: rows [polys][n] of evals under sigma_g, out[x] = in[pi_g(x)]"""
    _check(load_library().fhe_ckks_galois_evals_dev(_handle(plan), g, d_in, d_out, polys, stream))


def ckks_rns_galois_key_dev(plans, special, seed, first_row, g, d_s, d_cdt, m, d_gk, stream=None, limbs=None):
    """fhe_ckks_rns_galois_key_dev: d_gk [limbs][limbs + 1][2][n] evals from d_s [limbs + 1][n], the diagonal term on sigma_g(s)"""
    _check(load_library().fhe_ckks_rns_galois_key_dev(_plan_array(plans), len(plans) if limbs is None else limbs, _handle(special), _seed(seed), first_row, g, d_s,
                                                      d_cdt, m, d_gk, stream))


def ckks_rns_galois_dev(plans, special, d_gks, gs, key_limbs, d_in, d_out, batch, stream=None, limbs=None, count=None):
    """fhe_ckks_rns_galois_dev: [limbs][2][batch][n] -> [count][limbs][2][batch][n], one hoisted digit decomposition for all of
    gs; d_gks a list of device key pointers (None is passed as NULL, as is a None list)"""
    keys = None if d_gks is None else (_vp * max(len(d_gks), 1))(*d_gks)
    els = None if gs is None else (_u64 * max(len(gs), 1))(*gs)
    _check(load_library().fhe_ckks_rns_galois_dev(_plan_array(plans), len(plans) if limbs is None else limbs, _handle(special), keys, els,
                                                  len(gs) if count is None else count, key_limbs, d_in, d_out, batch, stream))


def ckks_rns_galois_workspace_bytes(n, limbs, batch, count):
    return int(load_library().fhe_ckks_rns_galois_workspace_bytes(n, limbs, batch, count))


def ckks_rns_diag_sum_dev(plans, special, d_gks, gs, key_limbs, d_pts, outputs, d_in, d_out, batch, stream=None, limbs=None, count=None):
    """fhe_ckks_rns_diag_sum_dev: [limbs][2][batch][n] -> [outputs][limbs][2][batch][n], out_o = sum_r m_{o,r} (.)
    sigma_{gs[r]}(in) with d_pts [outputs][count][limbs + 1][n]; d_gks a list of device key pointers, None (NULL) where gs[r] = 1"""
    keys = None if d_gks is None else (_vp * max(len(d_gks), 1))(*d_gks)
    els = None if gs is None else (_u64 * max(len(gs), 1))(*gs)
    _check(load_library().fhe_ckks_rns_diag_sum_dev(_plan_array(plans), len(plans) if limbs is None else limbs, _handle(special), keys, els,
                                                    len(gs) if count is None else count, key_limbs, d_pts, outputs, d_in, d_out, batch, stream))


def ckks_rns_diag_workspace_bytes(n, limbs, batch, count, outputs):
    return int(load_library().fhe_ckks_rns_diag_workspace_bytes(n, limbs, batch, count, outputs))


def ckks_rns_bsgs_dev(plans, special, d_baby_gks, baby_gs, d_giant_gks, giant_gs, key_limbs, d_pts, d_in, d_out, batch, stream=None, limbs=None, babies=None,
                      giants=None):
    """fhe_ckks_rns_bsgs_dev: [limbs][2][batch][n] -> [limbs][2][batch][n], sum_a sigma_{giant_gs[a]}(sum_b m_{a,b} (.)
    sigma_{baby_gs[b]}(in)) with d_pts [giants][babies][limbs + 1][n] and the giant steps' rotations hoisted; each key list holds
    device pointers, None (NULL) where the element is 1"""
    def arrays(d_gks, gs):
        return (None if d_gks is None else (_vp * max(len(d_gks), 1))(*d_gks)), (None if gs is None else (_u64 * max(len(gs), 1))(*gs))
    bk, bg = arrays(d_baby_gks, baby_gs)
    gk, gg = arrays(d_giant_gks, giant_gs)
    _check(load_library().fhe_ckks_rns_bsgs_dev(_plan_array(plans), len(plans) if limbs is None else limbs, _handle(special), bk, bg,
                                                len(baby_gs) if babies is None else babies, gk, gg, len(giant_gs) if giants is None else giants, key_limbs, d_pts,
                                                d_in, d_out, batch, stream))


def ckks_rns_bsgs_workspace_bytes(n, limbs, batch, babies, giants):
    return int(load_library().fhe_ckks_rns_bsgs_workspace_bytes(n, limbs, batch, babies, giants))


def _plans_or_none(plans):
    return None if plans is None else _plan_array(plans)


def ckks_deep_relin_key_dev(plans, specials, seed, first_row, d_s, d_cdt, m, d_key, stream=None, limbs=None, alpha=None):
    """fhe_ckks_deep_relin_key_dev: d_key [dnum][limbs + alpha][2][n] evals from d_s [limbs + alpha][n]"""
    _check(load_library().fhe_ckks_deep_relin_key_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, _plans_or_none(specials),
                                                      len(specials) if alpha is None else alpha, _seed(seed), first_row, d_s, d_cdt, m, d_key, stream))


def ckks_deep_galois_key_dev(plans, specials, seed, first_row, g, d_s, d_cdt, m, d_key, stream=None, limbs=None, alpha=None):
    """fhe_ckks_deep_galois_key_dev: the same key with the diagonal term on sigma_g(s)"""
    _check(load_library().fhe_ckks_deep_galois_key_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, _plans_or_none(specials),
                                                       len(specials) if alpha is None else alpha, _seed(seed), first_row, g, d_s, d_cdt, m, d_key, stream))


def ckks_deep_relinearize_dev(plans, specials, d_key, key_limbs, d_d, d_out, batch, stream=None, limbs=None, alpha=None):
    """fhe_ckks_deep_relinearize_dev: [limbs][3][batch][n] -> [limbs][2][batch][n]"""
    _check(load_library().fhe_ckks_deep_relinearize_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, _plans_or_none(specials),
                                                        len(specials) if alpha is None else alpha, d_key, key_limbs, d_d, d_out, batch, stream))


def ckks_deep_mul_dev(plans, specials, d_key, key_limbs, d_a, d_b, d_out, batch, stream=None, limbs=None, alpha=None):
    """fhe_ckks_deep_mul_dev: the tensor and its relinearisation in one call"""
    _check(load_library().fhe_ckks_deep_mul_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, _plans_or_none(specials),
                                                len(specials) if alpha is None else alpha, d_key, key_limbs, d_a, d_b, d_out, batch, stream))


def ckks_deep_galois_dev(plans, specials, d_gks, gs, key_limbs, d_in, d_out, batch, stream=None, limbs=None, alpha=None, count=None):
    """fhe_ckks_deep_galois_dev: [limbs][2][batch][n] -> [count][limbs][2][batch][n], one digit decomposition for all of gs;
    d_gks a list of device key pointers (None is passed as NULL, as is a None list)"""
    keys = None if d_gks is None else (_vp * max(len(d_gks), 1))(*d_gks)
    els = None if gs is None else (_u64 * max(len(gs), 1))(*gs)
    _check(load_library().fhe_ckks_deep_galois_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, _plans_or_none(specials),
                                                   len(specials) if alpha is None else alpha, keys, els, len(gs) if count is None else count, key_limbs, d_in, d_out,
                                                   batch, stream))


def ckks_deep_rescale_dev(plans, d_in, d_out, batch, stream=None, limbs=None):
    """fhe_ckks_deep_rescale_dev: [limbs][2][batch][n] -> [limbs - 1][2][batch][n]"""
    _check(load_library().fhe_ckks_deep_rescale_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, d_in, d_out, batch, stream))


def ckks_deep_workspace_bytes(n, limbs, alpha, batch):
    return int(load_library().fhe_ckks_deep_workspace_bytes(n, limbs, alpha, batch))


def ckks_deep_diag_sum_dev(plans, specials, d_gks, gs, key_limbs, d_pts, outputs, d_in, d_out, batch, stream=None, limbs=None, alpha=None, count=None):
    """fhe_ckks_deep_diag_sum_dev: [limbs][2][batch][n] -> [outputs][limbs][2][batch][n], out_o = sum_r m_{o,r} (.)
    sigma_{gs[r]}(in) with d_pts [outputs][count][limbs + alpha][n]; d_gks a list of device key pointers, None (NULL) where gs[r] = 1"""
    keys = None if d_gks is None else (_vp * max(len(d_gks), 1))(*d_gks)
    els = None if gs is None else (_u64 * max(len(gs), 1))(*gs)
    _check(load_library().fhe_ckks_deep_diag_sum_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, _plans_or_none(specials),
                                                     len(specials) if alpha is None else alpha, keys, els, len(gs) if count is None else count, key_limbs, d_pts,
                                                     outputs, d_in, d_out, batch, stream))


def ckks_deep_diag_workspace_bytes(n, limbs, alpha, batch, count, outputs):
    return int(load_library().fhe_ckks_deep_diag_workspace_bytes(n, limbs, alpha, batch, count, outputs))


def ckks_deep_lincomb_dev(plans, d_cts, w, k, outputs, d_out, batch, stream=None, limbs=None, count=None):
    """fhe_ckks_deep_lincomb_dev: ckks_rns_lincomb_dev's arguments on a chain of up to 32 limbs, a slice of 8 limbs
    a launch"""
    cts = None if d_cts is None else (_vp * max(len(d_cts), 1))(*d_cts)
    ws = None if w is None else (_u64 * max(len(w), 1))(*w)
    ks = None if k is None else (_u64 * max(len(k), 1))(*k)
    _check(load_library().fhe_ckks_deep_lincomb_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, cts, len(d_cts) if count is None else count, ws, ks,
                                                    outputs, d_out, batch, stream))


def ckks_deep_dot_dev(plans, specials, d_key, key_limbs, d_as, d_bs, w, d_out, batch, stream=None, limbs=None, alpha=None, count=None):
    """fhe_ckks_deep_dot_dev: relinearize(sum_r w_r tensor(a_r, b_r)) -> [limbs][2][batch][n] with the grouped-digit
    key switch, one whatever the number of pairs; the lists and w as for ckks_rns_dot_dev"""
    a = None if d_as is None else (_vp * max(len(d_as), 1))(*d_as)
    b = None if d_bs is None else (_vp * max(len(d_bs), 1))(*d_bs)
    ws = None if w is None else (_u64 * max(len(w), 1))(*w)
    _check(load_library().fhe_ckks_deep_dot_dev(_plans_or_none(plans), len(plans) if limbs is None else limbs, _plans_or_none(specials),
                                                len(specials) if alpha is None else alpha, d_key, key_limbs, a, b, len(d_as) if count is None else count, ws, d_out,
                                                batch, stream))


def ckks_rns_lincomb_dev(plans, d_cts, w, k, outputs, d_out, batch, stream=None, limbs=None, count=None):
    """fhe_ckks_rns_lincomb_dev: out_o = sum_r w[o][r] ct_r + (k[o], 0) per limb -> [outputs][limbs][2][batch][n];
    d_cts a list of device pointers, w the canonical residues [outputs][count][limbs] and k [outputs][limbs] (None: no constant)
    as flat sequences of integers"""
    cts = None if d_cts is None else (_vp * max(len(d_cts), 1))(*d_cts)
    ws = None if w is None else (_u64 * max(len(w), 1))(*w)
    ks = None if k is None else (_u64 * max(len(k), 1))(*k)
    _check(load_library().fhe_ckks_rns_lincomb_dev(None if plans is None else _plan_array(plans), len(plans) if limbs is None else limbs, cts, len(d_cts) if count is None else count, ws, ks,
                                                   outputs, d_out, batch, stream))


def ckks_rns_dot_dev(plans, special, d_rlk, key_limbs, d_as, d_bs, w, d_out, batch, stream=None, limbs=None, count=None):
    """fhe_ckks_rns_dot_dev: relinearize(sum_r w_r tensor(a_r, b_r)) -> [limbs][2][batch][n], one key switch whatever
    the number of pairs; d_as and d_bs lists of device pointers (None is passed as NULL, as is a None list), w the canonical
    residues [count][limbs] as a flat sequence of integers (None: every weight is 1)"""
    a = None if d_as is None else (_vp * max(len(d_as), 1))(*d_as)
    b = None if d_bs is None else (_vp * max(len(d_bs), 1))(*d_bs)
    ws = None if w is None else (_u64 * max(len(w), 1))(*w)
    _check(load_library().fhe_ckks_rns_dot_dev(None if plans is None else _plan_array(plans), len(plans) if limbs is None else limbs, _handle(special), d_rlk, key_limbs,
                                               a, b, len(d_as) if count is None else count, ws, d_out, batch, stream))


# ---- BFV on an RNS modulus chain (bfv_rns.hip) ---------------------------------------------------------------------
def rns_extend_dev(src_mods, dst_mods, centred, d_in, d_out, count, stream=None, src=None, dst=None):
    """fhe_rns_extend_dev: residues [src][count] modulo src_mods -> [dst][count] modulo dst_mods of the same integer, taken in
    [0, M) or, centred, in (-M/2, M/2]; the moduli are sequences of integers (None is passed as NULL)"""
    sm = None if src_mods is None else (_u64 * max(len(src_mods), 1))(*src_mods)
    dm = None if dst_mods is None else (_u64 * max(len(dst_mods), 1))(*dst_mods)
    _check(load_library().fhe_rns_extend_dev(sm, len(src_mods) if src is None else src, dm, len(dst_mods) if dst is None else dst, int(bool(centred)), d_in, d_out,
                                             count, stream))


def bfv_rns_tensor_dev(plans, aux, t, d_a, d_b, d_out, batch, stream=None, limbs=None):
    """fhe_bfv_rns_tensor_dev: [limbs][2][batch][n] x 2 -> the scaled tensor [limbs][3][batch][n]; aux the limbs + 1 auxiliary plans"""
    _check(load_library().fhe_bfv_rns_tensor_dev(None if plans is None else _plan_array(plans), len(plans) if limbs is None else limbs,
                                                 None if aux is None else _plan_array(aux), t, d_a, d_b, d_out, batch, stream))


def bfv_rns_mul_dev(plans, aux, special, t, d_rlk, d_a, d_b, d_out, batch, stream=None, limbs=None):
    """fhe_bfv_rns_mul_dev: the scaled tensor and its relinearisation against d_rlk [limbs][limbs + 1][2][n] in one call"""
    _check(load_library().fhe_bfv_rns_mul_dev(None if plans is None else _plan_array(plans), len(plans) if limbs is None else limbs,
                                              None if aux is None else _plan_array(aux), _handle(special), t, d_rlk, d_a, d_b, d_out, batch, stream))


def bfv_rns_dot_dev(plans, aux, special, t, d_rlk, d_as, d_bs, w, d_out, batch, stream=None, limbs=None, count=None):
    """fhe_bfv_rns_dot_dev: relinearize(round(t sum_r w_r tensor(a_r, b_r) / Q)) -> [limbs][2][batch][n], one rounding
    and one key switch whatever the number of pairs; d_as and d_bs lists of device pointers (None is passed as NULL, as is a
    None list), w the signed weights [count] as a sequence of integers (None: every weight is 1)"""
    a = None if d_as is None else (_vp * max(len(d_as), 1))(*d_as)
    b = None if d_bs is None else (_vp * max(len(d_bs), 1))(*d_bs)
    ws = None if w is None else (ctypes.c_int64 * max(len(w), 1))(*w)
    _check(load_library().fhe_bfv_rns_dot_dev(None if plans is None else _plan_array(plans), len(plans) if limbs is None else limbs,
                                              None if aux is None else _plan_array(aux), _handle(special), t, d_rlk, a, b, len(d_as) if count is None else count, ws,
                                              d_out, batch, stream))


def bfv_rns_workspace_bytes(n, limbs, batch):
    return int(load_library().fhe_bfv_rns_workspace_bytes(n, limbs, batch))


def bfv_rns_scale_msg_dev(plans, t, d_msg, d_out, batch, stream=None, limbs=None):
    """fhe_bfv_rns_scale_msg_dev: m [batch][n] in [0, t) -> floor(Q / t) m mod q_i, centred signed words [limbs][batch][n]"""
    _check(load_library().fhe_bfv_rns_scale_msg_dev(None if plans is None else _plan_array(plans), len(plans) if limbs is None else limbs, t, d_msg, d_out, batch, stream))


def bfv_rns_decrypt_dev(plans, aux0, t, d_s_evals, d_ct, d_out, batch, stream=None, limbs=None):
    """fhe_bfv_rns_decrypt_dev: [limbs][2][batch][n] evals -> m [batch][n] modulo t; aux0 one auxiliary prime above 2 t + 2"""
    _check(load_library().fhe_bfv_rns_decrypt_dev(None if plans is None else _plan_array(plans), len(plans) if limbs is None else limbs, aux0, t, d_s_evals, d_ct, d_out,
                                                  batch, stream))


def shard_gather_dev(total_rows, row_words, src_devices, d_src_shards, dst_device, d_dst, stream=None):
    """fhe_shard_gather_dev: the shards of a block-partitioned batch (entry r = device pointer to rank r's rows of
    shard_range(total_rows, world, r), or None for an empty shard) copied in rank order onto dst_device — no torch, no RCCL."""
    world = len(src_devices)
    devs = (_int * world)(*[int(d) for d in src_devices])
    ptrs = (_vp * world)(*[(_vp(int(p)) if p else _vp(None)) for p in d_src_shards])
    _check(load_library().fhe_shard_gather_dev(int(total_rows), int(row_words), world, devs, ptrs, int(dst_device), d_dst, stream))


def device_count():
    return int(load_library().fhe_ntt_device_count())


def set_check_canonical(on):
    """FHE_NTT_CHECK_CANONICAL at run time: transforms reject inputs >= q instead of returning garbage."""
    _check(load_library().fhe_ntt_set_check_canonical(int(bool(on))))


def shard_range(total, world, rank):
    """[begin, end) of `total` units owned by `rank` of `world` (fhe_shard_range; host-only)."""
    b, e = _sz(0), _sz(0)
    _check(load_library().fhe_shard_range(int(total), int(world), int(rank), ctypes.byref(b), ctypes.byref(e)))
    return int(b.value), int(e.value)


def set_batch_tile(polys):
    _check(load_library().fhe_ntt_set_batch_tile(int(polys)))


def set_persist(mode, tile_polys=1, lag=1, ringslots=4):
    """The one-launch n = 2^16 forward transform (csrc/ntt_persist.hip): mode 0 off (two-pass kernels), "A" / 1 lagged
    tiles (tile_polys, lag, ringslots; ringslots 0 = through the output buffer), "B" / 2 teams (ringslots)."""
    mode = {"A": 1, "B": 2, "D": 3, "E": 4, "a": 1, "b": 2, "d": 3, "e": 4}.get(mode, mode)
    _check(load_library().fhe_ntt_set_persist(int(mode), int(tile_polys), int(lag), int(ringslots)))


def set_persist_grid(workgroups):
    """Workgroups of a persistent launch (0: as many as the chip holds)."""
    _check(load_library().fhe_ntt_set_persist_grid(int(workgroups)))


def persist_status():
    """Raises FheError if a persistent launch that has finished gave up a bounded wait (call after synchronising)."""
    _check(load_library().fhe_ntt_persist_status())


def kernel_timing_enable(on):
    _check(load_library().fhe_ntt_kernel_timing_enable(int(bool(on))))


def kernel_timing_reset():
    _check(load_library().fhe_ntt_kernel_timing_reset())


def kernel_timing_read(cap=64):
    """→ {kernel_name: (total_ms, launches)}"""
    names = ctypes.create_string_buffer(64 * cap)
    ms = (ctypes.c_double * cap)()
    cnt = (ctypes.c_uint64 * cap)()
    k = load_library().fhe_ntt_kernel_timing_read(names, ms, cnt, cap)
    out = {}
    for i in range(min(k, cap)):
        nm = names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode()
        out[nm] = (float(ms[i]), int(cnt[i]))
    return out


def shutdown():
    global _lib
    if _lib is not None:
        _lib.fhe_ntt_shutdown()
