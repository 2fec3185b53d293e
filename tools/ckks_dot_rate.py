#!/usr/bin/env python3
"""tools/ckks_dot_rate.py — the cost of a sum of ct x ct pairs with one relinearisation on one GPU:
  - fhe_ckks_rns_dot_dev at n = 4096 and 8192, k = 3 limbs of the (58, 40) test chain, batch 1024, count in {2, 4, 8, 16}, with and
    without weights, milliseconds per call, against the composed form on the older entry points in the same process: count calls
    of fhe_ckks_rns_mul_dev and one fhe_ckks_rns_lincomb_dev;
  - before anything is timed, the words that should be equal are compared: the call against fhe_ckks_rns_relinearize_dev of the
    weighted sum (fhe_ckks_rns_lincomb_dev) of the pairs' fhe_ckks_rns_tensor_dev, and one unweighted pair against
    fhe_ckks_rns_mul_dev.  The composed form's own words differ by design: it relinearises count times;
  - the bytes each form moves on paper and the bytes per second that makes for the tensorsum kernel (4 count + 3 slabs a limb);
  - the library's per-kernel timer for both.
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_dot_rate.py [tag]  ->  profiles/<tag>_ckks_dot_rate.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fhe_study_amd as pkg

import _ckks_eval_numpy as E
from _timing import timeit                           # warm clocks: tools/_timing.py
from ckks_eval_rate import kernel_ms, moved_bytes, rand_ct, BATCH, K
from ckks_poly_rate import kernels

B = pkg.binding
I64 = torch.int64
COUNTS = (2, 4, 8, 16)


def paper_bytes(n, k, count):
    """bytes each form needs by the kernels' definitions: one relinearisation is mul's kernels without its tensor, and its
    transforms (k inverse and k^2 forward of a slab for the digits, 2 inverse and 2k forward for t_P) move two slabs each"""
    w = 8 * BATCH * n
    mul = moved_bytes(n, k, "mul")
    relin = sum(v for name, v in mul.items() if name != "ckks_rns_tensor") + 2 * (k * k + 3 * k + 2) * w
    tensorsum = (4 * count + 3) * k * w
    return {"tensorsum": tensorsum, "relin": relin, "dot": tensorsum + relin,
            "composed": count * (mul["ckks_rns_tensor"] + relin) + (count + 1) * 2 * k * w}


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"shape": {"batch": BATCH, "limbs": K, "chain": "(58, 40)", "counts": list(COUNTS)}, "not_measured": [
        "a kDotGroup other than 16", "two words a thread in the tensorsum kernel", "k other than 3", "batches other than 1024",
        "counts above 16 (the carried groups)", "a limb of 2^62 or more (the fold of every pair)", "squares and repeated operands (fewer distinct bytes)",
        "hardware counters (bytes are those the algorithm needs, computed from the shapes)"]}
    for n in (4096, 8192):
        mods, P = E.chain(n, 58, 40, K - 1)
        plans, sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
        g = torch.Generator(device="cuda").manual_seed(50 + n)               # a key-shaped array [K][K + 1][2][n] of canonical residues
        rlk = torch.stack([torch.stack([torch.randint(0, q, (2, n), dtype=I64, device="cuda", generator=g) for q in list(mods) + [P]]) for _ in range(K)])
        xs, ys = [rand_ct(mods, 2, n, 100 + r) for r in range(max(COUNTS))], [rand_ct(mods, 2, n, 200 + r) for r in range(max(COUNTS))]
        prods = [torch.empty_like(xs[0]) for _ in range(max(COUNTS))]
        tens = [torch.empty((K, 3, BATCH, n), dtype=I64, device="cuda") for _ in range(max(COUNTS))]
        tsum, fused, comp, want = torch.empty_like(tens[0]), torch.empty_like(xs[0]), torch.empty_like(xs[0]), torch.empty_like(xs[0])
        ct_bytes = xs[0].numel() * 8
        rng = np.random.default_rng(n)
        row = {"ciphertext_bytes": ct_bytes}
        B.ckks_rns_dot_dev(plans, sp, rlk.data_ptr(), K, [xs[0].data_ptr()], [ys[0].data_ptr()], None, fused.data_ptr(), BATCH)
        B.ckks_rns_mul_dev(plans, sp, rlk.data_ptr(), K, xs[0].data_ptr(), ys[0].data_ptr(), want.data_ptr(), BATCH)
        torch.cuda.synchronize()
        assert torch.equal(fused, want), "one unweighted pair is not mul's words"
        for count in COUNTS:
            a, b = [x.data_ptr() for x in xs[:count]], [y.data_ptr() for y in ys[:count]]
            for weighted in (False, True):
                w = [[int(rng.integers(0, q)) if weighted else 1 for q in mods] for _ in range(count)]
                flat = [x for r in w for x in r]
                dot = lambda: B.ckks_rns_dot_dev(plans, sp, rlk.data_ptr(), K, a, b, flat if weighted else None, fused.data_ptr(), BATCH)

                def composed():
                    for r in range(count):
                        B.ckks_rns_mul_dev(plans, sp, rlk.data_ptr(), K, a[r], b[r], prods[r].data_ptr(), BATCH)
                    B.ckks_rns_lincomb_dev(plans, [p.data_ptr() for p in prods[:count]], flat, None, 1, comp.data_ptr(), BATCH)
                # the words that should be equal: relinearize(sum_r w_r tensor(a_r, b_r)), the sum by lincomb on the tensors read as
                # [K][2][3 BATCH / 2][n] (a limb's three components are contiguous, and BATCH is even)
                for r in range(count):
                    B.ckks_rns_tensor_dev(plans, a[r], b[r], tens[r].data_ptr(), BATCH)
                B.ckks_rns_lincomb_dev(plans, [t.data_ptr() for t in tens[:count]], flat, None, 1, tsum.data_ptr(), 3 * BATCH // 2)
                B.ckks_rns_relinearize_dev(plans, sp, rlk.data_ptr(), K, tsum.data_ptr(), want.data_ptr(), BATCH)
                dot(); composed()
                torch.cuda.synchronize()
                assert torch.equal(fused, want), f"the call and the relinearised sum of the tensors differ at count {count}, weighted {weighted}"
                t_d, t_c = timeit(dot, 0.3, 0.6, 3), timeit(composed, 0.3, 0.6, 3)
                k_d, k_c = kernel_ms(dot), kernel_ms(composed)
                paper = paper_bytes(n, K, count)
                ts_ms = sum(ms for name, (ms, _) in k_d.items() if name.startswith("ckks_rns_tensorsum"))
                row[f"count_{count}_{'weighted' if weighted else 'ones'}"] = {
                    "dot_ms": t_d * 1e3, "composed_ms": t_c * 1e3, "composed_over_dot": t_c / t_d, "bytes_dot": paper["dot"], "bytes_composed": paper["composed"],
                    "bytes_ratio": paper["composed"] / paper["dot"], "dot_GBps": paper["dot"] / t_d / 1e9, "composed_GBps": paper["composed"] / t_c / 1e9,
                    "tensorsum_bytes": paper["tensorsum"], "tensorsum_timer_ms": ts_ms, "tensorsum_GBps_by_timer": paper["tensorsum"] / (ts_ms * 1e-3) / 1e9 if ts_ms else None,
                    "kernels_dot": kernels(k_d), "kernels_composed": kernels(k_c)}
        mul = lambda: B.ckks_rns_mul_dev(plans, sp, rlk.data_ptr(), K, xs[0].data_ptr(), ys[0].data_ptr(), want.data_ptr(), BATCH)
        row["one_mul_ms"] = timeit(mul, 0.3, 0.6, 3) * 1e3
        res[f"n{n}"] = row
        del xs, ys, prods, tens, tsum, fused, comp, want
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_dot_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
