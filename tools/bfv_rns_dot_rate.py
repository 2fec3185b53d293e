#!/usr/bin/env python3
"""tools/bfv_rns_dot_rate.py — the cost of the BFV inner product on an RNS chain on one GPU, at §33's shape:
n = 8192, k = 3 chain primes (59 bits), four auxiliary primes (61 bits), t = 65537, batch 256.
  - fhe_bfv_rns_dot_dev over R in {2, 4, 16} pairs, milliseconds per call after warm-up, beside the same sum composed from R
    calls of fhe_bfv_rns_mul_dev and R - 1 additions, in the same process: the composed route is the yardstick;
  - the ratio beside the transform-count prediction (28 R + 50) / (78 R) of k = 3, which counts polynomial transforms alone;
  - the library's per-kernel timer for both routes, summed into transforms (and copies), the per-pair tensor kernels, the
    extension, the scale-and-round, the relinearisation's element-wise kernels and the additions;
  - the noise budget of `dot` over 16 pairs of fresh ciphertexts against the composed sum (batch 1, real keys);
  - before anything is timed: dot of one pair against fhe_bfv_rns_mul_dev, word for word.
Diagnostic only (the contract bench is bench.py); no threshold is set on any figure.
Usage: tools/bfv_rns_dot_rate.py [tag]  ->  profiles/<tag>_bfv_rns_dot_rate.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fhe_study_amd as pkg

import _bfv_rns_numpy as R
from _timing import timeit                           # warm clocks: tools/_timing.py

B = pkg.binding
I64 = torch.int64
N, K, BATCH, T = 8192, 3, 256, 65537
COUNTS = (2, 4, 16)
GROUPS = {"tensorsum": ("bfv_rns_tensorsum", "ckks_rns_tensor"), "extension": ("rns_extend",), "scale": ("bfv_rns_scale",),
          "relin_elementwise": ("ckks_rns_lift", "ckks_rns_keymac", "ckks_rns_divround"), "additions": ("ew_",)}


def kernel_ms(f, reps=3):
    B.kernel_timing_enable(True)
    B.kernel_timing_reset()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    out = {k: (v[0] / reps, v[1] / reps) for k, v in B.kernel_timing_read(256).items()}
    B.kernel_timing_enable(False)
    return out


def split(kernels):
    """the timer's labels summed into groups, milliseconds a call; what no group names is a transform or a copy"""
    out = dict.fromkeys(list(GROUPS) + ["transforms_and_copies"], 0.0)
    launches = 0
    for name, (ms, count) in kernels.items():
        group = next((g for g, prefixes in GROUPS.items() if name.startswith(prefixes)), "transforms_and_copies")
        out[group] += ms
        launches += count
    out["total"] = sum(out.values())
    out["launches"] = launches
    return out


def noise_budgets(count):
    """fresh ciphertexts of random messages under real keys, batch 1: the budget of dot over `count` pairs, of the composed sum
    and of one product"""
    bfv = pkg.bfv
    mods, aux, P = R.chain(N, K)
    param = bfv.RnsParam(N, mods, aux, P, T)
    key = bfv.RnsClientKey.generate(bytes(range(32)), param)
    pk, rlk = key.public_key(0), key.relin_key(0)
    rng = np.random.default_rng(34)
    xs = [key.encrypt(pk, rng.integers(0, T, (1, N))) for _ in range(count)]
    ys = [key.encrypt(pk, rng.integers(0, T, (1, N))) for _ in range(count)]
    fused = bfv.dot(xs, ys, rlk)
    composed = xs[0].mul(ys[0], rlk)
    for x, y in zip(xs[1:], ys[1:]):
        composed = composed + x.mul(y, rlk)
    same = bool(np.array_equal(key.decrypt(fused), key.decrypt(composed)))
    return {"pairs": count, "fresh": key.noise_budget(xs[0]), "one_product": key.noise_budget(xs[0].mul(ys[0], rlk)), "dot": key.noise_budget(fused),
            "composed": key.noise_budget(composed), "decryptions_equal": same}


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    mods, aux, P = R.chain(N, K)
    assert R.admitted(mods, aux, T, N)
    plans, ap, sp = [pkg.Plan(q, N) for q in mods], [pkg.Plan(b, N) for b in aux], pkg.Plan(P, N)
    g = torch.Generator(device="cuda").manual_seed(34)
    rlk = torch.stack([torch.stack([torch.randint(0, q, (2, N), dtype=I64, device="cuda", generator=g) for q in list(mods) + [P]]) for _ in range(K)])
    cts = [torch.stack([torch.randint(0, q, (2, BATCH, N), dtype=I64, device="cuda", generator=g) for q in mods]) for _ in range(2 * max(COUNTS))]
    out, acc, tmp = (torch.empty_like(cts[0]) for _ in range(3))
    L = B.load_library()

    def dot(count):
        B.bfv_rns_dot_dev(plans, ap, sp, T, rlk.data_ptr(), [cts[2 * r].data_ptr() for r in range(count)], [cts[2 * r + 1].data_ptr() for r in range(count)], None,
                          out.data_ptr(), BATCH)

    def composed(count):
        B.bfv_rns_mul_dev(plans, ap, sp, T, rlk.data_ptr(), cts[0].data_ptr(), cts[1].data_ptr(), acc.data_ptr(), BATCH)
        for r in range(1, count):
            B.bfv_rns_mul_dev(plans, ap, sp, T, rlk.data_ptr(), cts[2 * r].data_ptr(), cts[2 * r + 1].data_ptr(), tmp.data_ptr(), BATCH)
            for i, plan in enumerate(plans):
                B._check(L.fhe_rq_add_dev(plan.handle, acc[i].data_ptr(), tmp[i].data_ptr(), acc[i].data_ptr(), 2 * BATCH, None))

    dot(1); composed(1)
    torch.cuda.synchronize()
    assert torch.equal(out, acc), "dot of one pair is not fhe_bfv_rns_mul_dev"
    res = {"shape": {"n": N, "limbs": K, "aux": K + 1, "batch": BATCH, "t": T, "chain_bits": 59, "aux_bits": 61, "chunk_rows": R.chunk_rows(N, K, BATCH)},
           "yardstick": "the same sum from R calls of fhe_bfv_rns_mul_dev and R - 1 of fhe_rq_add_dev per limb, this commit, this process",
           "not_measured": ["k other than 3", "batches other than 256", "n other than 8192", "weighted sums", "squares and repeated operands", "hardware counters"],
           "counts": {}}
    for count in COUNTS:
        t_d, t_c = timeit(lambda: dot(count), 0.3, 0.6, 3), timeit(lambda: composed(count), 0.3, 0.6, 3)
        k_d, k_c = kernel_ms(lambda: dot(count)), kernel_ms(lambda: composed(count))
        res["counts"][str(count)] = {"dot_ms": t_d * 1e3, "composed_ms": t_c * 1e3, "dot_over_composed": t_d / t_c,
                                     "transform_count_prediction": (28 * count + 50) / (78 * count),
                                     "split_dot": split(k_d), "split_composed": split(k_c),
                                     "kernels_dot": {k: list(v) for k, v in sorted(k_d.items())}, "kernels_composed": {k: list(v) for k, v in sorted(k_c.items())}}
        print(count, json.dumps({k: v for k, v in res["counts"][str(count)].items() if not k.startswith("kernels")}), flush=True)
    res["noise_budget_bits"] = noise_budgets(16)
    print(json.dumps(res["noise_budget_bits"]), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_bfv_rns_dot_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
