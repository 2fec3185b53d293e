#!/usr/bin/env python3
"""tools/ckks_poly_rate.py — the cost of the fused scalar sums and of a Chebyshev evaluation on one GPU:
  - fhe_ckks_rns_lincomb_dev at n = 4096 and 8192, k = 3 limbs of the (58, 40) test chain, batch 1024, count in {3, 7, 15},
    outputs in {1, 2, 4}, milliseconds per call, against the same sums composed from fhe_rq_mul_by_u64_dev and fhe_rq_add_dev in
    the same process, after the words of both were found equal;
  - the slabs each form moves on paper (count + outputs against 3 count outputs - outputs) and the bytes per second that makes;
  - the library's per-kernel timer for both;
  - one degree-15 evaluation of the logistic fit on [-4, 4] end to end (n = 4096, 7 limbs, batch 64) with its kernels.
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_poly_rate.py [tag]  ->  profiles/<tag>_ckks_poly_rate.json"""
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
from ckks_eval_rate import kernel_ms, rand_ct, BATCH, K

B = pkg.binding
I64 = torch.int64
COUNTS, OUTPUTS = (3, 7, 15), (1, 2, 4)


def kernels(d):
    return {name: {"ms_per_call": ms, "launches_per_call": c} for name, (ms, c) in d.items()}


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"shape": {"batch": BATCH, "limbs": K, "chain": "(58, 40)", "counts": list(COUNTS), "outputs": list(OUTPUTS)}, "not_measured": [
        "a kLinOutputs other than 4 or a kLinGroup other than 16", "k other than 3", "batches other than 1024", "constants", "counts above 16 (the carried groups)",
        "hardware counters (bytes are those the algorithm needs, computed from the shapes)"]}
    lib = B.load_library()
    for n in (4096, 8192):
        mods, _ = E.chain(n, 58, 40, K - 1)
        plans = [pkg.Plan(q, n) for q in mods]
        cts = [rand_ct(mods, 2, n, 100 + r) for r in range(max(COUNTS))]
        ptrs = [x.data_ptr() for x in cts]
        fused = torch.empty((max(OUTPUTS),) + tuple(cts[0].shape), dtype=I64, device="cuda")
        acc, tmp = torch.empty_like(fused), torch.empty_like(cts[0])
        slab = cts[0].numel() * 8                                             # bytes of one ciphertext
        rng = np.random.default_rng(n)
        row = {"ciphertext_bytes": slab}
        for count in COUNTS:
            for outputs in OUTPUTS:
                w = [[[int(rng.integers(0, q)) for q in mods] for _ in range(count)] for _ in range(outputs)]
                flat = [x for o in w for r in o for x in r]
                lin = lambda: B.ckks_rns_lincomb_dev(plans, ptrs[:count], flat, None, outputs, fused.data_ptr(), BATCH)

                def composed():
                    for o in range(outputs):
                        for i, p in enumerate(plans):
                            for r in range(count):
                                dst = acc[o, i] if r == 0 else tmp[i]
                                B._check(lib.fhe_rq_mul_by_u64_dev(p.handle, cts[r][i].data_ptr(), w[o][r][i], dst.data_ptr(), 2 * BATCH, None))
                                if r:
                                    B._check(lib.fhe_rq_add_dev(p.handle, acc[o, i].data_ptr(), tmp[i].data_ptr(), acc[o, i].data_ptr(), 2 * BATCH, None))
                lin(); composed()
                torch.cuda.synchronize()
                assert torch.equal(fused[:outputs], acc[:outputs]), f"the fused and the composed words differ at count {count}, outputs {outputs}"
                t_l, t_c = timeit(lin, 0.3, 0.6, 3), timeit(composed, 0.3, 0.6, 3)
                moved_l, moved_c = (count + outputs) * slab, (3 * count - 1) * outputs * slab   # mul: 2 slabs, add: 3, the first product lands in acc
                row[f"count_{count}_outputs_{outputs}"] = {
                    "lincomb_ms": t_l * 1e3, "composed_ms": t_c * 1e3, "composed_over_lincomb": t_c / t_l, "bytes_lincomb": moved_l, "bytes_composed": moved_c,
                    "bytes_ratio": moved_c / moved_l, "lincomb_GBps": moved_l / t_l / 1e9, "composed_GBps": moved_c / t_c / 1e9,
                    "kernels_lincomb": kernels(kernel_ms(lin)), "kernels_composed": kernels(kernel_ms(composed))}
        res[f"n{n}"] = row
        del cts, fused, acc, tmp
        torch.cuda.empty_cache()
    # one degree-15 evaluation end to end
    ck = pkg.ckks
    n, rows = 4096, 64
    mods, P = E.chain(n, 58, 40, 6)
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(bytes(range(32)), param, 2.0 ** 40)
    z = np.random.default_rng(7).uniform(-4, 4, (rows, n // 2)).astype(np.complex128)
    ct = key.encode_and_encrypt(key.public_key(0), z)
    rlk = key.relin_key(0)
    coeffs = ck.chebyshev_fit(lambda x: 1 / (1 + np.exp(-x)), 15, (-4, 4))
    plan = ck.ChebyshevPlan.build(coeffs, (-4, 4))
    run = lambda: ct.eval_chebyshev(plan, rlk)
    out = run()
    err = float(np.abs(key.decrypt_and_decode(out) - np.polynomial.chebyshev.chebval(z.real / 4, coeffs)).max())
    assert err < 2.0 ** -10, f"the decoded slots are off by {err}"
    t = timeit(run, 0.3, 0.6, 3)
    res["degree15"] = {"n": n, "limbs": len(mods), "batch": rows, "levels": plan.levels, "products": plan.products,
                       "lincomb_calls": sum(op[0] == "lincomb" for op in plan.ops), "ms": t * 1e3, "worst_slot_error": err, "kernels": kernels(kernel_ms(run))}
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_poly_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
