#!/usr/bin/env python3
"""tools/bfv_rns_rate.py — the cost of the exact BFV product on an RNS chain on one GPU:
  - fhe_bfv_rns_mul_dev at n = 8192, k = 3 chain primes (59 bits), four auxiliary primes (61 bits), t = 65537, batch 256,
    milliseconds per call after warm-up, beside fhe_ckks_rns_mul_dev at the same n, limbs, primes and batch in the same process;
  - the library's per-kernel timer for fhe_bfv_rns_tensor_dev (the scaled tensor alone), for fhe_bfv_rns_mul_dev and for
    fhe_ckks_rns_mul_dev, summed into transforms, extension kernels (rns_extend, bfv_rns_scale), the tensor kernel and the
    relinearisation's own element-wise kernels; the relinearisation's transforms are the difference of the two BFV calls';
  - before anything is timed: fhe_bfv_rns_mul_dev against fhe_ckks_rns_relinearize_dev of fhe_bfv_rns_tensor_dev, word for word.
Diagnostic only (the contract bench is bench.py).
Usage: tools/bfv_rns_rate.py [tag]  ->  profiles/<tag>_bfv_rns_rate.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import fhe_study_amd as pkg

import _bfv_rns_numpy as R
from _timing import timeit                           # warm clocks: tools/_timing.py

B = pkg.binding
I64 = torch.int64
N, K, BATCH, T = 8192, 3, 256, 65537
EXTENSION = ("rns_extend", "bfv_rns_scale")
RELIN = ("ckks_rns_lift", "ckks_rns_keymac", "ckks_rns_divround")


def kernel_ms(f, reps=5):
    B.kernel_timing_enable(True)
    B.kernel_timing_reset()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    out = {k: (v[0] / reps, v[1] / reps) for k, v in B.kernel_timing_read(256).items()}
    B.kernel_timing_enable(False)
    return out


def split(kernels):
    """the timer's labels summed into the four groups, milliseconds a call"""
    out = {"extension": 0.0, "tensor": 0.0, "relin_elementwise": 0.0, "transforms_and_copies": 0.0}
    for name, (ms, _) in kernels.items():
        group = "extension" if name.startswith(EXTENSION) else "tensor" if name.startswith("ckks_rns_tensor") else \
            "relin_elementwise" if name.startswith(RELIN) else "transforms_and_copies"
        out[group] += ms
    out["total"] = sum(out.values())
    return out


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    mods, aux, P = R.chain(N, K)
    assert R.admitted(mods, aux, T, N)
    plans, ap, sp = [pkg.Plan(q, N) for q in mods], [pkg.Plan(b, N) for b in aux], pkg.Plan(P, N)
    g = torch.Generator(device="cuda").manual_seed(33)
    rlk = torch.stack([torch.stack([torch.randint(0, q, (2, N), dtype=I64, device="cuda", generator=g) for q in list(mods) + [P]]) for _ in range(K)])
    a, b = (torch.stack([torch.randint(0, q, (2, BATCH, N), dtype=I64, device="cuda", generator=g) for q in mods]) for _ in range(2))
    out, want, ck = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    ten = torch.empty((K, 3, BATCH, N), dtype=I64, device="cuda")
    bfv_mul = lambda: B.bfv_rns_mul_dev(plans, ap, sp, T, rlk.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), BATCH)
    bfv_tensor = lambda: B.bfv_rns_tensor_dev(plans, ap, T, a.data_ptr(), b.data_ptr(), ten.data_ptr(), BATCH)
    ckks_mul = lambda: B.ckks_rns_mul_dev(plans, sp, rlk.data_ptr(), K, a.data_ptr(), b.data_ptr(), ck.data_ptr(), BATCH)
    bfv_mul(); bfv_tensor()
    B.ckks_rns_relinearize_dev(plans, sp, rlk.data_ptr(), K, ten.data_ptr(), want.data_ptr(), BATCH)
    torch.cuda.synchronize()
    assert torch.equal(out, want), "fhe_bfv_rns_mul_dev is not the relinearised scaled tensor"
    res = {"shape": {"n": N, "limbs": K, "aux": K + 1, "batch": BATCH, "t": T, "chain_bits": 59, "aux_bits": 61, "chunk_rows": R.chunk_rows(N, K, BATCH)},
           "not_measured": ["k other than 3", "batches other than 256", "n other than 8192", "primes with a 32-bit form", "the fused form of the extension kernels",
                            "hardware counters"]}
    t_b, t_t, t_c = timeit(bfv_mul, 0.3, 0.6, 3), timeit(bfv_tensor, 0.3, 0.6, 3), timeit(ckks_mul, 0.3, 0.6, 3)
    k_b, k_t, k_c = kernel_ms(bfv_mul), kernel_ms(bfv_tensor), kernel_ms(ckks_mul)
    s_b, s_t, s_c = split(k_b), split(k_t), split(k_c)
    res.update({"bfv_mul_ms": t_b * 1e3, "bfv_tensor_ms": t_t * 1e3, "ckks_mul_ms": t_c * 1e3, "bfv_over_ckks": t_b / t_c,
                "bfv_mul_ciphertexts_per_s": BATCH / t_b, "ckks_mul_ciphertexts_per_s": BATCH / t_c,
                "split_bfv_mul": s_b, "split_bfv_tensor": s_t, "split_ckks_mul": s_c,
                "relin_transforms_ms": s_b["transforms_and_copies"] - s_t["transforms_and_copies"],
                "extension_share_of_bfv_mul": s_b["extension"] / s_b["total"],
                "kernels_bfv_mul": {k: list(v) for k, v in sorted(k_b.items())}, "kernels_bfv_tensor": {k: list(v) for k, v in sorted(k_t.items())},
                "kernels_ckks_mul": {k: list(v) for k, v in sorted(k_c.items())}})
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_bfv_rns_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
