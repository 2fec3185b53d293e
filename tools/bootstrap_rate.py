#!/usr/bin/env python3
"""tools/bootstrap_rate.py — TFHE bootstrapping rate on one GPU: N = 1024, k = 1, l = 64, n_lwe = 630,
KSK 1024 -> 630 with l = 64, random key words (a rate needs no valid keys).  Per batch: blind rotations / s and full
bootstraps / s; one CMux step against one prepared external product at the same batch, with the per-kernel split
(fhe_ntt_kernel_timing_*); one CMux step of the oracle composition on one host core.  Diagnostic only (the contract
bench is bench.py).  Usage: tools/bootstrap_rate.py [tag] [batch ...]  ->  profiles/<tag>_bootstrap_rate.json"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import fhe_study_amd as pkg
from oracle import load_oracle

from _timing import timeit                           # warm clocks: tools/_timing.py

B, L = pkg.binding, pkg.load_library()
st = torch.cuda.current_stream().cuda_stream
N, K, LV, NL, KS_L = 1024, 1, 64, 630, 64


def rand(shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-(1 << 63), (1 << 63) - 1, shape, dtype=torch.int64, device="cuda", generator=g)


def kernel_split(f, reps=3):
    """{kernel: ms per call of f} over `reps` calls (events around every launch: run after the timed loop)"""
    torch.cuda.synchronize()
    B.kernel_timing_reset()
    B.kernel_timing_enable(1)
    for _ in range(reps): f()
    torch.cuda.synchronize()
    out = {k: {"ms_per_call": v[0] / reps, "launches_per_call": v[1] // reps} for k, v in B.kernel_timing_read().items()}
    B.kernel_timing_enable(0)
    B.kernel_timing_reset()
    return out


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    batches = [int(x) for x in sys.argv[2:]] or [64, 256, 1024, 4096]
    words = L.fhe_tfhe_bsk_prepared_words(N, K, LV, NL)
    tw = L.fhe_tggsw_prepared_words(N, K, LV)
    bsk = rand((NL, K + 1, LV, K + 1, N), 1)
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    t0 = time.perf_counter()
    B._check(L.fhe_tfhe_bsk_prepare_dev(N, K, LV, NL, bsk.data_ptr(), prep.data_ptr(), st))
    torch.cuda.synchronize()
    prep_s = time.perf_counter() - t0
    del bsk
    ksk = rand((K * N, KS_L, NL + 1), 2)
    table = rand((K + 1, N), 3)
    res = {"shape": {"n": N, "k": K, "l": LV, "n_lwe": NL, "ks_l": KS_L, "ks_n_in": K * N, "ks_n_out": NL},
           "bsk_prepare_s_first_call": prep_s, "batches": {}}
    for batch in batches:
        lwe = rand((batch, NL + 1), 4 + batch)
        acc = torch.empty((batch, K + 1, N), dtype=torch.int64, device="cuda")
        out = torch.empty((batch, NL + 1), dtype=torch.int64, device="cuda")
        br = lambda: B._check(L.fhe_tfhe_blind_rotation_dev(N, K, LV, NL, prep.data_ptr(), table.data_ptr(), lwe.data_ptr(), acc.data_ptr(), batch, st))
        boot = lambda: B._check(L.fhe_tfhe_bootstrap_dev(N, K, LV, NL, prep.data_ptr(), table.data_ptr(), KS_L, ksk.data_ptr(), lwe.data_ptr(),
                                                         out.data_ptr(), batch, st))
        x = rand((batch, K + 1, N), 5)
        y = torch.empty_like(x)
        ext = lambda: B._check(L.fhe_tggsw_external_product_prepared_dev(N, K, LV, prep.data_ptr(), x.data_ptr(), y.data_ptr(), batch, st))
        t_br, t_boot = timeit(br, 0.3, 0.5, 2), timeit(boot, 0.3, 0.5, 2)
        t_ext = timeit(ext)
        split_br = kernel_split(br, 2)
        split_ext = kernel_split(ext, 20)
        mac_c = split_br.get("digit_mac32_cmux_10", {}).get("ms_per_call", 0.0) / NL
        tail_c = split_br.get("digit_tail32_cmux_10", {}).get("ms_per_call", 0.0) / NL
        mac_e = split_ext.get("digit_mac32_10", {}).get("ms_per_call", 0.0)
        tail_e = split_ext.get("digit_tail32_10", {}).get("ms_per_call", 0.0)
        r = {"blind_rotation_s": t_br, "blind_rotations_per_s": batch / t_br,
             "bootstrap_s": t_boot, "bootstraps_per_s": batch / t_boot,
             "cmux_step_wall_us": t_br / NL * 1e6, "external_product_wall_us": t_ext * 1e6,
             "cmux_over_external_product_wall": (t_br / NL) / t_ext,
             "cmux_step_kernels_us": {"digit_mac32_cmux": mac_c * 1e3, "digit_tail32_cmux": tail_c * 1e3},
             "external_product_kernels_us": {"digit_mac32": mac_e * 1e3, "digit_tail32": tail_e * 1e3},
             "cmux_over_external_product_kernels": (mac_c + tail_c) / (mac_e + tail_e) if mac_e + tail_e else None,
             "blind_rotation_kernel_split_ms": split_br, "bootstrap_kernel_split_ms": kernel_split(boot, 1)}
        res["batches"][str(batch)] = r
        print(json.dumps({"batch": batch, **{k: v for k, v in r.items() if not k.endswith("split_ms")}}), flush=True)
        del lwe, acc, out, x, y
    # one CMux step of the oracle composition on one host core (a whole CPU bootstrap takes minutes): per step
    O = load_oracle()
    rng = np.random.default_rng(0)
    g = rng.integers(0, 1 << 64, (K + 1, LV, K + 1, N), dtype=np.uint64, endpoint=False)
    a = rng.integers(0, 1 << 64, (1, K + 1, N), dtype=np.uint64, endpoint=False)
    t0 = time.perf_counter()
    j = np.arange(N) + 77
    rot = np.where((j // N) % 2 == 1, np.uint64(0) - a[..., j % N], a[..., j % N])
    a2 = a + O.external_product(N, K, LV, g, rot - a)
    cpu_s = time.perf_counter() - t0
    res["oracle_cmux_step_one_core_s_per_ciphertext"] = cpu_s
    res["oracle_bootstrap_estimate_one_core_s_per_ciphertext"] = cpu_s * NL
    assert a2.shape == (1, K + 1, N)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_bootstrap_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path, "| oracle CMux step on one core: %.3f s per ciphertext" % cpu_s)


if __name__ == "__main__":
    main()
