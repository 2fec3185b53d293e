#!/usr/bin/env python3
"""tools/ckks_bsgs_rate.py — the cost of a plaintext linear transform with hoisted giant steps on one GPU, at
n = 4096 and 8192, k = 3 limbs of the (58, 40) test chain, batch 1024, 16 (4 x 4) and 64 (8 x 8) diagonals:
  - RnsCiphertext.linear_transform_hoisted (one fhe_ckks_rns_bsgs_dev call), milliseconds per call;
  - RnsCiphertext.linear_transform (one diag_sum, a rotation and an add per giant step), in the same process, after the two
    results were decrypted at limb 0 and found within the sum of their noise bounds of each other;
  - the cost of a giant step of each, and the library's per-kernel timer for both: ckks_rns_giantmac per giant step with a key
    beside ckks_rns_keymac_galois per rotation;
  - what was not measured.
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_bsgs_rate.py [tag]  ->  profiles/<tag>_ckks_bsgs_rate.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fhe_study_amd as pkg

import _ckks_bsgs_numpy as BN
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
from _timing import timeit                           # warm clocks: tools/_timing.py
from ckks_eval_rate import kernel_ms, rand_ct, BATCH, K
from ckks_linear_rate import phase0

B, ck = pkg.binding, pkg.ckks
I64 = torch.int64
SIDES = (4, 8)                                       # n1 = baby steps = giant steps: 16 and 64 diagonals
MMAX = 64                                            # plaintext coefficients in [-MMAX, MMAX]


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"shape": {"batch": BATCH, "limbs": K, "chain": "(58, 40)", "sides": list(SIDES)}, "not_measured": [
        "k other than 3", "batches other than 1024", "shapes other than 4 x 4 and 8 x 8", "a chunk other than 2^21 / (n k^2) ciphertexts",
        "more than two giant steps a diagmac launch", "hardware counters"]}
    tab = pkg.tfhe.cdt_table(3.2)
    d_tab = torch.from_numpy(np.ascontiguousarray(tab).view(np.int64)).cuda()
    seed = bytes(range(32))
    for n in (4096, 8192):
        mods, P = E.chain(n, 58, 40, K - 1)
        param = ck.RnsParam(n, mods, P)
        plans, sp = param.plans(K - 1), param.special_plan()
        d_s = torch.empty((K + 1, n), dtype=I64, device="cuda")
        d_se = torch.empty(n, dtype=I64, device="cuda")
        for i, p in enumerate(plans + [sp]):
            B.ckks_secret_key_dev(p, seed, 0, d_s[i].data_ptr())
        plans[0].forward_dev(d_s[0].data_ptr(), d_se.data_ptr(), 1)
        ct = ck.RnsCiphertext(param, rand_ct(mods, 2, n, 1), K - 1, 1.0)
        row = {"chunk_rows": E.chunk_rows(n, K, BATCH), "workspace_bytes": B.ckks_rns_bsgs_workspace_bytes(n, K, BATCH, max(SIDES), max(SIDES)),
               "diag_workspace_bytes": B.ckks_rns_diag_workspace_bytes(n, K, BATCH, max(SIDES), max(SIDES))}
        for side in SIDES:
            steps = sorted(set(range(1, side)) | {side * j for j in range(1, side)})
            keys = {}
            for slot, st in enumerate(steps):
                gk = torch.empty((K, K + 1, 2, n), dtype=I64, device="cuda")
                g = ck.galois_element(n, st)
                B.ckks_rns_galois_key_dev(plans, sp, seed, G.GK_BASE + 64 * slot, g, d_s.data_ptr(), d_tab.data_ptr(), len(tab), gk.data_ptr())
                keys[st] = ck.RnsGaloisKey(param, g, gk)
            m = torch.from_numpy(np.random.default_rng(n + side).integers(-MMAX, MMAX + 1, (side * side, n), dtype=np.int64)).cuda()
            pts = torch.empty((side * side, K + 1, n), dtype=I64, device="cuda")
            for pl, lo in ((plans, 0), ([sp], K)):
                ev = torch.empty((len(pl), side * side, n), dtype=I64, device="cuda")
                B.ckks_rns_from_i64_dev(pl, m.data_ptr(), ev.data_ptr(), side * side)
                pts[:, lo:lo + len(pl)] = ev.permute(1, 0, 2)
            baby = giant = list(range(side))
            lt = ck.LinearTransform(param, side, baby, giant, ck.RnsPlaintextSet(param, K - 1, pts.reshape(side, side, K + 1, n), 1.0, [ck.galois_element(n, i) for i in baby]))
            assert lt.required_steps() == steps
            hoisted = lambda: ct.linear_transform_hoisted(lt, keys)
            composed = lambda: ct.linear_transform(lt, keys)
            q0 = mods[0]
            diff = torch.remainder(phase0(plans[0], d_se, hoisted().d) - phase0(plans[0], d_se, composed().d), q0)
            diff = torch.where(diff > q0 // 2, diff - q0, diff).abs().max().item()
            norms = m.abs().sum(dim=1).reshape(side, side).tolist()
            sw1, gsw = [[int(x) for x in r[1:]] for r in norms], [j != 0 for j in giant]
            bound = BN.bsgs_noise(n, K, sw1, gsw) + BN.composed_noise(n, K, sw1, gsw)
            assert diff <= bound, f"decrypted results differ by {diff}, the noise bounds allow {bound}"
            torch.cuda.empty_cache()
            t_h, t_c = timeit(hoisted, 0.3, 0.6, 3), timeit(composed, 0.3, 0.6, 3)
            kh, kc = kernel_ms(hoisted), kernel_ms(composed)
            gm = sum(ms for name, (ms, _) in kh.items() if name.startswith("ckks_rns_giantmac"))
            kmg = sum(ms for name, (ms, _) in kc.items() if name.startswith("ckks_rns_keymac_galois"))
            mh, mc = BN.moddowns([ck.galois_element(n, side * j) for j in giant])
            row[f"side_{side}"] = {
                "diagonals": side * side, "hoisted_ms": t_h * 1e3, "composed_ms": t_c * 1e3, "composed_over_hoisted": t_c / t_h, "decrypted_difference": diff,
                "noise_bound": bound, "hoisted_ms_per_giant": t_h * 1e3 / side, "composed_ms_per_giant": t_c * 1e3 / side,
                "giantmac_ms_per_giant": gm / side, "giantmac_ms_per_giant_with_a_key": gm / (side - 1), "keymac_galois_ms_per_rotation": kmg / (side - 1),
                "component_moddowns_hoisted": mh, "component_moddowns_composed": mc,
                "kernels_hoisted": {name: {"ms_per_call": ms, "launches_per_call": c} for name, (ms, c) in kh.items()},
                "kernels_composed": {name: {"ms_per_call": ms, "launches_per_call": c} for name, (ms, c) in kc.items()}}
            del keys, lt, pts, m
            torch.cuda.empty_cache()
        res[f"n{n}"] = row
        del ct
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_bsgs_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
