#!/usr/bin/env python3
"""tools/ckks_linear_rate.py — the cost of the double-hoisted diagonal sum on one GPU, at n = 4096 and 8192,
k = 3 limbs of the (58, 40) test chain, batch 1024, one output, 8 and 32 rotations:
  - fhe_ckks_rns_diag_sum_dev, milliseconds per call;
  - the composition the entry points of §22 - §23 allow: fhe_ckks_rns_galois_dev with all keys (one digit decomposition, a
    modulus-down per rotation), then pointwise_mul_dev per limb and component, then fhe_rq_add_dev; in the same process, after
    the two results were decrypted at limb 0 and found within the sum of their noise bounds of each other;
  - the library's per-kernel timer for both, and the per-element cost of ckks_rns_diagmac against ckks_rns_keymac_galois;
  - the digit slabs of a chunk against the L2 (4 MiB an XCD);
  - what was not measured.
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_linear_rate.py [tag]  ->  profiles/<tag>_ckks_linear_rate.json"""
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
import _ckks_linear_numpy as LN
from _timing import timeit                           # warm clocks: tools/_timing.py
from ckks_eval_rate import kernel_ms, rand_ct, BATCH, K

B = pkg.binding
I64 = torch.int64
COUNTS = (8, 32)
MMAX = 64                                            # plaintext coefficients in [-MMAX, MMAX]


def phase0(plan, d_s_evals, ct):
    """limb 0 of ct [k][2][batch][n] -> c0 + c1 s, centred int64 [batch][n]"""
    coef = torch.empty_like(ct[0])
    plan.inverse_dev(ct[0].data_ptr(), coef.data_ptr(), 2 * BATCH)
    out = torch.empty((BATCH, ct.shape[-1]), dtype=I64, device="cuda")
    B.ckks_decrypt_dev(plan, d_s_evals.data_ptr(), coef.data_ptr(), out.data_ptr(), BATCH)
    return out


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"shape": {"batch": BATCH, "limbs": K, "chain": "(58, 40)", "outputs": 1, "counts": list(COUNTS)}, "not_measured": [
        "outputs other than 1 (the in-register sharing of the key sums between two outputs)", "a kDiagOutputs other than 2 or a kDiagGroup other than 16",
        "chunk sizes other than 2^21 / (n k^2)", "k other than 3", "batches other than 1024", "counts other than 8 and 32", "LinearTransform end to end",
        "hardware counters (no cache hit rate is claimed: the digit slabs of a chunk are compared with the L2 by size only)"]}
    tab = pkg.tfhe.cdt_table(3.2)
    d_tab = torch.from_numpy(np.ascontiguousarray(tab).view(np.int64)).cuda()
    seed = bytes(range(32))
    for n in (4096, 8192):
        mods, P = E.chain(n, 58, 40, K - 1)
        plans, sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
        d_s = torch.empty((K + 1, n), dtype=I64, device="cuda")
        d_se = torch.empty(n, dtype=I64, device="cuda")
        for i, p in enumerate(plans + [sp]):
            B.ckks_secret_key_dev(p, seed, 0, d_s[i].data_ptr())
        plans[0].forward_dev(d_s[0].data_ptr(), d_se.data_ptr(), 1)
        top = max(COUNTS)
        gs = [G.galois_element(n, t + 1) for t in range(top)]
        gks = []
        for t, g in enumerate(gs):
            gk = torch.empty((K, K + 1, 2, n), dtype=I64, device="cuda")
            B.ckks_rns_galois_key_dev(plans, sp, seed, G.GK_BASE + 64 * t, g, d_s.data_ptr(), d_tab.data_ptr(), len(tab), gk.data_ptr())
            gks.append(gk)
        ptrs = [x.data_ptr() for x in gks]
        m = torch.from_numpy(np.random.default_rng(n).integers(-MMAX, MMAX + 1, (top, n), dtype=np.int64)).cuda()
        pts = torch.empty((top, K + 1, n), dtype=I64, device="cuda")
        for pl, lo in ((plans, 0), ([sp], K)):
            ev = torch.empty((len(pl), top, n), dtype=I64, device="cuda")
            B.ckks_rns_from_i64_dev(pl, m.data_ptr(), ev.data_ptr(), top)
            pts[:, lo:lo + len(pl)] = ev.permute(1, 0, 2)
        a = rand_ct(mods, 2, n, 1)
        fused = torch.empty((1,) + tuple(a.shape), dtype=I64, device="cuda")
        rots = torch.empty((top,) + tuple(a.shape), dtype=I64, device="cuda")
        prod, acc = torch.empty_like(a), torch.empty_like(a)
        lib = B.load_library()
        row = {"chunk_rows": E.chunk_rows(n, K, BATCH), "digit_slab_bytes_per_chunk": K * K * E.chunk_rows(n, K, BATCH) * n * 8, "l2_bytes_per_xcd": 4 << 20}
        for count in COUNTS:
            pt = pts[:count].contiguous()
            diag = lambda: B.ckks_rns_diag_sum_dev(plans, sp, ptrs[:count], gs[:count], K, pt.data_ptr(), 1, a.data_ptr(), fused.data_ptr(), BATCH)

            def composed():
                B.ckks_rns_galois_dev(plans, sp, ptrs[:count], gs[:count], K, a.data_ptr(), rots.data_ptr(), BATCH)
                for r in range(count):
                    dst = acc if r == 0 else prod
                    for i, p in enumerate(plans):
                        for c in range(2):
                            p.pointwise_mul_dev(rots[r, i, c].data_ptr(), ptb[r, i].data_ptr(), dst[i, c].data_ptr(), BATCH)
                    if r:
                        for i, p in enumerate(plans):
                            B._check(lib.fhe_rq_add_dev(p.handle, acc[i].data_ptr(), prod[i].data_ptr(), acc[i].data_ptr(), 2 * BATCH, None))
            ptb = pt[:, :K, None, :].expand(count, K, BATCH, n).contiguous()         # mul_plain's operand: the plaintext per row of the batch
            diag(); composed()
            torch.cuda.synchronize()
            q0 = mods[0]
            diff = torch.remainder(phase0(plans[0], d_se, fused[0]) - phase0(plans[0], d_se, acc), q0)
            diff = torch.where(diff > q0 // 2, diff - q0, diff).abs().max().item()
            norms = [int(x) for x in m[:count].abs().sum(dim=1).tolist()]
            bound = LN.linear_noise(n, K, norms) + sum(norms) * E.relin_noise(n, K)
            assert diff <= bound, f"decrypted results differ by {diff}, the noise bounds allow {bound}"
            t_d, t_c = timeit(diag, 0.3, 0.6, 3), timeit(composed, 0.3, 0.6, 3)
            kd, kc = kernel_ms(diag), kernel_ms(composed)
            mac = sum(ms for name, (ms, _) in kd.items() if name.startswith("ckks_rns_diagmac"))
            kmg = sum(ms for name, (ms, _) in kc.items() if name.startswith("ckks_rns_keymac_galois"))
            row[f"count_{count}"] = {
                "diag_sum_ms": t_d * 1e3, "composed_ms": t_c * 1e3, "composed_over_diag_sum": t_c / t_d, "decrypted_difference": diff, "noise_bound": bound,
                "diag_sum_ms_per_element": t_d * 1e3 / count, "diagmac_ms_per_element": mac / count, "keymac_galois_ms_per_element": kmg / count,
                "diagmac_over_keymac_galois": mac / kmg, "workspace_bytes": B.ckks_rns_diag_workspace_bytes(n, K, BATCH, count, 1),
                "kernels_diag_sum": {name: {"ms_per_call": ms, "launches_per_call": c} for name, (ms, c) in kd.items()},
                "kernels_composed": {name: {"ms_per_call": ms, "launches_per_call": c} for name, (ms, c) in kc.items()}}
            del ptb
        c8, c32 = row["count_8"], row["count_32"]
        row["diag_sum_ms_per_further_element"] = (c32["diag_sum_ms"] - c8["diag_sum_ms"]) / (COUNTS[1] - COUNTS[0])
        row["composed_ms_per_further_element"] = (c32["composed_ms"] - c8["composed_ms"]) / (COUNTS[1] - COUNTS[0])
        res[f"n{n}"] = row
        del a, fused, rots, prod, acc, gks, pts
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_linear_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
