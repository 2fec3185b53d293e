#!/usr/bin/env python3
"""tools/ckks_galois_rate.py — the cost of slot rotations on the RNS chain on one GPU, at n = 4096 and 8192,
k = 3 limbs of the (58, 40) test chain, batch 1024:
  - fhe_ckks_rns_galois_dev with one Galois element (count = 1), milliseconds per call and ciphertexts/s;
  - eight rotations from one hoisted call (count = 8) against eight count = 1 calls, in the same process, after their words were
    compared;
  - fhe_ckks_rns_mul_dev at the same shape in the same process;
  - the library's per-kernel timer for the count = 1 and count = 8 calls, with the bytes each kernel's definition moves per call
    and the achieved TB/s (lift: 1 read and a write per target; keymac: k reads and 2 writes, the key rows left out; divround:
    2 reads and 1 write a component and the gathered c0);
  - what was not measured.
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_galois_rate.py [tag]  ->  profiles/<tag>_ckks_galois_rate.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fhe_study_amd as pkg

import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
from _timing import timeit                           # warm clocks: tools/_timing.py
from ckks_eval_rate import kernel_ms, rand_ct, BATCH, K

B = pkg.binding
I64 = torch.int64
ROTS = 8


def moved_bytes(n, k, count):
    """bytes per call that each kernel's definition moves (8-byte words), over all chunks"""
    w = 8 * BATCH * n
    return {"ckks_rns_lift": (k * (1 + k) + count * 2 * (1 + k)) * w, "ckks_rns_keymac": count * (k + 1) * (k + 2) * w, "ckks_rns_divround": count * k * 7 * w}


def kernels_of(f, n, count):
    moved, out = moved_bytes(n, K, count), {}
    for name, (ms, launches) in kernel_ms(f).items():
        out[name] = {"ms_per_call": ms, "launches_per_call": launches}
        for lab, byts in moved.items():
            if name.startswith(lab):
                out[name].update(bytes_per_call=byts, tb_per_s=byts / (ms * 1e-3) / 1e12)
    return out


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"shape": {"batch": BATCH, "limbs": K, "chain": "(58, 40)", "rotations": ROTS}, "not_measured": [
        "chunk sizes other than 2^21 / (n k^2)", "k other than 3", "batches other than 1024", "counts other than 1 and 8",
        "the bare automorphism fhe_ckks_galois_evals_dev", "key generation",
        "hardware counters (the TB/s are bytes by definition over the kernel timer's time; the cache-line behaviour of the gathered reads is argued, not counted)"]}
    tab = pkg.tfhe.cdt_table(3.2)
    d_tab = torch.from_numpy(np.ascontiguousarray(tab).view(np.int64)).cuda()
    seed = bytes(range(32))
    for n in (4096, 8192):
        mods, P = E.chain(n, 58, 40, K - 1)
        plans, sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
        d_s = torch.empty((K + 1, n), dtype=I64, device="cuda")
        for i, p in enumerate(plans + [sp]):
            B.ckks_secret_key_dev(p, seed, 0, d_s[i].data_ptr())
        rlk = torch.empty((K, K + 1, 2, n), dtype=I64, device="cuda")
        B.ckks_rns_relin_key_dev(plans, sp, seed, E.RLK_BASE, d_s.data_ptr(), d_tab.data_ptr(), len(tab), rlk.data_ptr())
        gs = [G.galois_element(n, 1 << t) for t in range(ROTS)]
        gks = []
        for t, g in enumerate(gs):
            gk = torch.empty((K, K + 1, 2, n), dtype=I64, device="cuda")
            B.ckks_rns_galois_key_dev(plans, sp, seed, G.GK_BASE + 64 * t, g, d_s.data_ptr(), d_tab.data_ptr(), len(tab), gk.data_ptr())
            gks.append(gk)
        ptrs = [x.data_ptr() for x in gks]
        a, b = rand_ct(mods, 2, n, 1), rand_ct(mods, 2, n, 2)
        many = torch.empty((ROTS,) + tuple(a.shape), dtype=I64, device="cuda")
        sep = torch.empty_like(many)
        prod = torch.empty_like(a)
        hoisted = lambda: B.ckks_rns_galois_dev(plans, sp, ptrs, gs, K, a.data_ptr(), many.data_ptr(), BATCH)
        one = lambda: B.ckks_rns_galois_dev(plans, sp, ptrs[:1], gs[:1], K, a.data_ptr(), sep[0].data_ptr(), BATCH)

        def separate():
            for r in range(ROTS):
                B.ckks_rns_galois_dev(plans, sp, ptrs[r:r + 1], gs[r:r + 1], K, a.data_ptr(), sep[r].data_ptr(), BATCH)
        mul = lambda: B.ckks_rns_mul_dev(plans, sp, rlk.data_ptr(), K, a.data_ptr(), b.data_ptr(), prod.data_ptr(), BATCH)
        hoisted(); separate()
        torch.cuda.synchronize()
        assert torch.equal(many, sep), "the hoisted call and the separate calls differ"
        t_one, t_h, t_s, t_mul = (timeit(f, 0.3, 0.6, 3) for f in (one, hoisted, separate, mul))
        res[f"n{n}"] = {
            "one_rotation_ms": t_one * 1e3, "one_rotation_ct_per_s": BATCH / t_one,
            "hoisted_8_ms": t_h * 1e3, "separate_8_ms": t_s * 1e3, "separate_over_hoisted": t_s / t_h, "hoisted_rotations_per_s": ROTS * BATCH / t_h,
            "mul_ms": t_mul * 1e3, "one_rotation_over_mul": t_one / t_mul,
            "chunk_rows": E.chunk_rows(n, K, BATCH), "workspace_bytes": B.ckks_rns_galois_workspace_bytes(n, K, BATCH, ROTS),
            "kernels_count_1": kernels_of(one, n, 1), "kernels_count_8": kernels_of(hoisted, n, ROTS), "kernels_mul": {
                name: {"ms_per_call": ms, "launches_per_call": c} for name, (ms, c) in kernel_ms(mul).items()},
        }
        del a, b, many, sep, prod, gks
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_galois_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
