#!/usr/bin/env python3
"""tools/gadget_bootstrap_rate.py — TFHE bootstrapping rate with the signed base-2^b gadget on one GPU:
N = 1024, k = 1, n_lwe = 630; BSK (b, l) = (8, 3) and (10, 2); KSK 1024 -> 630 with (b, l) = (4, 4); random key words
(a rate needs no valid keys).  Per batch: gadget bootstraps / s and blind rotations / s with the per-kernel split
(fhe_ntt_kernel_timing_*); at batch 4096 the beta = 2, l = 64 bootstrap of DESIGN.md §10 timed in the same process,
alternating with the gadget one.  Diagnostic only (the contract bench is bench.py).
Usage: tools/gadget_bootstrap_rate.py [tag] [batch ...]  ->  profiles/<tag>_gadget_bootstrap_rate.json"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import fhe_study_amd as pkg

from _timing import timeit                           # warm clocks: tools/_timing.py
from bootstrap_rate import kernel_split, rand

B, L = pkg.binding, pkg.load_library()
st = torch.cuda.current_stream().cuda_stream
N, K, NL = 1024, 1, 630
BSK_SHAPES = [(8, 3), (10, 2)]
KS_B, KS_L = 4, 4
B2_L, B2_KS_L = 64, 64


def gadget_key(b, l, seed):
    words = L.fhe_tfhe_gadget_bsk_prepared_words(N, K, b, l, NL)
    assert words > 0
    bsk = rand((NL, K + 1, l, K + 1, N), seed)
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    B._check(L.fhe_tfhe_gadget_bsk_prepare_dev(N, K, b, l, NL, bsk.data_ptr(), prep.data_ptr(), st))
    torch.cuda.synchronize()
    return prep


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    batches = [int(x) for x in sys.argv[2:]] or [64, 256, 1024, 4096]
    ksk = rand((K * N, KS_L, NL + 1), 2)
    table = rand((K + 1, N), 3)
    res = {"shape": {"n": N, "k": K, "n_lwe": NL, "bsk": BSK_SHAPES, "ks": [KS_B, KS_L], "ks_n_in": K * N, "ks_n_out": NL,
                     "ksk_mb": K * N * KS_L * (NL + 1) * 8 / 1e6, "beta2_ksk_mb": K * N * B2_KS_L * (NL + 1) * 8 / 1e6},
           "gadget": {}}
    for b, l in BSK_SHAPES:
        prep = gadget_key(b, l, 10 + b)
        r = {"bsk_prepared_mb": prep.numel() * 8 / 1e6, "batches": {}}
        for batch in batches:
            lwe = rand((batch, NL + 1), 4 + batch)
            acc = torch.empty((batch, K + 1, N), dtype=torch.int64, device="cuda")
            out = torch.empty((batch, NL + 1), dtype=torch.int64, device="cuda")
            br = lambda: B._check(L.fhe_tfhe_gadget_blind_rotation_dev(N, K, b, l, NL, prep.data_ptr(), table.data_ptr(), lwe.data_ptr(),
                                                                       acc.data_ptr(), batch, st))
            boot = lambda: B._check(L.fhe_tfhe_gadget_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), table.data_ptr(), KS_B, KS_L,
                                                                    ksk.data_ptr(), lwe.data_ptr(), out.data_ptr(), batch, st))
            t_br, t_boot = timeit(br, 0.3, 0.5, 3), timeit(boot, 0.3, 0.5, 3)
            x = {"blind_rotation_s": t_br, "blind_rotations_per_s": batch / t_br, "bootstrap_s": t_boot, "bootstraps_per_s": batch / t_boot,
                 "cmux_step_wall_us": t_br / NL * 1e6, "kernel_timing_bootstrap_ms": kernel_split(boot, 2)}
            r["batches"][str(batch)] = x
            print(json.dumps({"bsk": [b, l], "batch": batch, **{k: v for k, v in x.items() if not k.startswith("kernel")}}), flush=True)
            del lwe, acc, out
        res["gadget"][f"b{b}_l{l}"] = r
        del prep
    # beta = 2, l = 64 against (8, 3) at batch 4096, alternating in this process
    batch = 4096
    prep_g = gadget_key(8, 3, 18)
    words = L.fhe_tfhe_bsk_prepared_words(N, K, B2_L, NL)
    bsk = rand((NL, K + 1, B2_L, K + 1, N), 1)
    prep_2 = torch.empty(words, dtype=torch.int64, device="cuda")
    B._check(L.fhe_tfhe_bsk_prepare_dev(N, K, B2_L, NL, bsk.data_ptr(), prep_2.data_ptr(), st))
    del bsk
    ksk_2 = rand((K * N, B2_KS_L, NL + 1), 5)
    lwe = rand((batch, NL + 1), 6)
    out = torch.empty((batch, NL + 1), dtype=torch.int64, device="cuda")
    boot_g = lambda: B._check(L.fhe_tfhe_gadget_bootstrap_dev(N, K, 8, 3, NL, prep_g.data_ptr(), table.data_ptr(), KS_B, KS_L, ksk.data_ptr(),
                                                              lwe.data_ptr(), out.data_ptr(), batch, st))
    boot_2 = lambda: B._check(L.fhe_tfhe_bootstrap_dev(N, K, B2_L, NL, prep_2.data_ptr(), table.data_ptr(), B2_KS_L, ksk_2.data_ptr(),
                                                       lwe.data_ptr(), out.data_ptr(), batch, st))
    tg, t2 = [], []
    for _ in range(3):
        tg.append(timeit(boot_g, 0.2, 0.5, 3))
        t2.append(timeit(boot_2, 0.2, 1.0, 2))
    cmp = {"batch": batch, "gadget_8_3_ks_4_4_s": tg, "beta2_l64_s": t2,
           "gadget_bootstraps_per_s": batch / min(tg), "beta2_bootstraps_per_s": batch / min(t2), "ratio": min(t2) / min(tg),
           "kernel_timing_gadget_ms": kernel_split(boot_g, 2), "kernel_timing_beta2_ms": kernel_split(boot_2, 1)}
    res["same_process_vs_beta2"] = cmp
    print(json.dumps({k: v for k, v in cmp.items() if not k.startswith("kernel")}), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_gadget_bootstrap_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
