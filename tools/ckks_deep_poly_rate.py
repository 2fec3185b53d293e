#!/usr/bin/env python3
"""tools/ckks_deep_poly_rate.py — the cost of the scalar sums and inner products on the deep CKKS chain on one
GPU, milliseconds per call, beside what the entry points before them do on the same words:
  (a) n = 2^15, 24 limbs, batch 4: fhe_ckks_deep_lincomb_dev of 15 ciphertexts into 4 outputs beside fhe_ckks_rns_lincomb_dev over
      three slices of 8 limbs; and per alpha in {1, 3, 4, 8} fhe_ckks_deep_dot_dev of 2, 4 and 16 pairs beside that many
      fhe_ckks_deep_mul_dev and the per-limb fhe_rq_add_dev of their results;
  (b) n = 4096, 3 limbs, alpha = 1, batch 1024: both entry points beside fhe_ckks_rns_lincomb_dev and fhe_ckks_rns_dot_dev.
Keys and ciphertexts are canonical random words: the cost does not depend on the keys being keys.  A measurement keeps the chip
under back-to-back calls for at least 150 ms, then takes the median of seven timed, synchronised calls.  Diagnostic only (the
contract bench is bench.py).
Usage: tools/ckks_deep_poly_rate.py [tag [commit]]  ->  profiles/<tag>_ckks_deep_poly_rate.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import fhe_study_amd as pkg

import _ckks_deep_numpy as D
import _ckks_deep_poly_numpy as DP
from ckks_deep_rate import I64, commit_of, median_ms, words

B = pkg.binding
LIN_COUNT, LIN_OUTPUTS = 15, 4


def lincomb_rows(n, L, batch):
    """the scalar sum of 15 into 4 on L limbs beside §27's entry point on slices of at most 8 plans -> dict"""
    mods, _ = D.case_chain(n, L, 1)
    plans = [pkg.Plan(q, n) for q in mods]
    cts = [words((L, 2, batch, n), 10 + r) for r in range(LIN_COUNT)]
    ptrs = [x.data_ptr() for x in cts]
    out = torch.empty((LIN_OUTPUTS, L, 2, batch, n), dtype=I64, device="cuda")
    outs = [torch.empty((LIN_OUTPUTS, min(8, L - i0), 2, batch, n), dtype=I64, device="cuda") for i0 in range(0, L, 8)]
    w = [3 + i for i in range(LIN_OUTPUTS * LIN_COUNT * L)]
    k = [5 + i for i in range(LIN_OUTPUTS * L)]
    limb_bytes = 2 * batch * n * 8
    ws = [[w[(o * LIN_COUNT + r) * L + i] for o in range(LIN_OUTPUTS) for r in range(LIN_COUNT) for i in range(i0, min(L, i0 + 8))] for i0 in range(0, L, 8)]
    ks = [[k[o * L + i] for o in range(LIN_OUTPUTS) for i in range(i0, min(L, i0 + 8))] for i0 in range(0, L, 8)]

    def sliced():
        for s, i0 in enumerate(range(0, L, 8)):
            B.ckks_rns_lincomb_dev(plans[i0:i0 + 8], [p + i0 * limb_bytes for p in ptrs], ws[s], ks[s], LIN_OUTPUTS, outs[s].data_ptr(), batch)
    row = {"limbs": L, "batch": batch, "count": LIN_COUNT, "outputs": LIN_OUTPUTS, "ciphertext_bytes": L * limb_bytes,
           "launches": {"deep": DP.lincomb_launches(L, LIN_OUTPUTS, LIN_COUNT), "rns_slices": L * -(-LIN_OUTPUTS // 4) * -(-LIN_COUNT // 16)}}
    row["deep_lincomb_ms"] = median_ms(lambda: B.ckks_deep_lincomb_dev(plans, ptrs, w, k, LIN_OUTPUTS, out.data_ptr(), batch))
    row["rns_lincomb_slices_ms"] = median_ms(sliced)
    row["rns_over_deep"] = row["rns_lincomb_slices_ms"] / row["deep_lincomb_ms"]
    # bytes moved: every input once, every output once
    row["deep_lincomb_gbps"] = (LIN_COUNT + LIN_OUTPUTS) * L * limb_bytes / row["deep_lincomb_ms"] / 1e6
    return row


def dot_rows(n, L, alpha, batch, counts, rns):
    """the inner product of `counts` pairs beside that many products and their per-limb sums (rns: and beside §29's entry point)"""
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = [pkg.Plan(q, n) for q in mods], [pkg.Plan(p, n) for p in sps]
    ng, top = D.dnum(L, alpha), max(counts)
    key = words((ng, L + alpha, 2, n), 100)
    held = min(top, 4)                                   # operands cycle over four ciphertexts: the kernels read every pointer as it comes
    xs, ys = [words((L, 2, batch, n), 1 + r) for r in range(held)], [words((L, 2, batch, n), 50 + r) for r in range(held)]
    out, prod = torch.empty((L, 2, batch, n), dtype=I64, device="cuda"), torch.empty((L, 2, batch, n), dtype=I64, device="cuda")
    lib = B.load_library()
    row = {"limbs": L, "alpha": alpha, "dnum": ng, "batch": batch, "chunk_rows": D.chunk_rows(n, L, alpha, batch),
           "workspace_bytes": B.ckks_deep_workspace_bytes(n, L, alpha, batch)}
    for count in counts:
        a, b = [xs[r % held].data_ptr() for r in range(count)], [ys[r % held].data_ptr() for r in range(count)]

        def composed():
            for r in range(count):
                B.ckks_deep_mul_dev(plans, sp, key.data_ptr(), L, a[r], b[r], (prod if r else out).data_ptr(), batch)
                if r:
                    for i, p in enumerate(plans):
                        B._check(lib.fhe_rq_add_dev(p.handle, out[i].data_ptr(), prod[i].data_ptr(), out[i].data_ptr(), 2 * batch, None))
        r_ = {"tensorsum_launches_a_chunk": DP.tensorsum_launches(L, count), "key_switches": {"dot": 1, "composed": count}}
        r_["deep_dot_ms"] = median_ms(lambda: B.ckks_deep_dot_dev(plans, sp, key.data_ptr(), L, a, b, None, out.data_ptr(), batch))
        r_["muls_and_adds_ms"] = median_ms(composed)
        r_["composed_over_dot"] = r_["muls_and_adds_ms"] / r_["deep_dot_ms"]
        if rns:
            r_["rns_dot_ms"] = median_ms(lambda: B.ckks_rns_dot_dev(plans, sp[0], key.data_ptr(), L, a, b, None, out.data_ptr(), batch))
            r_["deep_over_rns"] = r_["deep_dot_ms"] / r_["rns_dot_ms"]
        row[f"count_{count}"] = r_
    return row


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"machine": torch.cuda.get_device_name(0), "commit": commit_of(sys.argv), "torch": torch.__version__, "hip": torch.version.hip,
           "method": "150 ms of back-to-back calls, then the median of 7 timed, synchronised calls; milliseconds per call",
           "not_measured": ["weighted dots", "scalar sums of other counts and outputs", "real keys (random canonical words serve: no branch depends on them)",
                            "batches, n and limbs other than the ones listed", "hardware counters", "a whole Chebyshev plan"]}
    n, L, batch = 1 << 15, 24, 4
    res["a_n32768_l24_lincomb"] = lincomb_rows(n, L, batch)
    print(json.dumps({"a_lincomb": res["a_n32768_l24_lincomb"]}), flush=True)
    torch.cuda.empty_cache()
    for alpha in (1, 3, 4, 8):
        res[f"a_n32768_l24_alpha{alpha}_dot"] = dot_rows(n, L, alpha, batch, (2, 4, 16), False)
        print(json.dumps({f"a_alpha{alpha}": res[f"a_n32768_l24_alpha{alpha}_dot"]}), flush=True)
        torch.cuda.empty_cache()
    n, L, batch = 4096, 3, 1024
    res["b_n4096_l3_lincomb"] = lincomb_rows(n, L, batch)
    torch.cuda.empty_cache()
    res["b_n4096_l3_alpha1_dot"] = dot_rows(n, L, 1, batch, (2, 4, 16), True)
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_deep_poly_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
