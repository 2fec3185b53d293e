#!/usr/bin/env python3
"""tools/lut_rate.py — rate of the TFHE lookup-table bootstrap on one GPU: N = 1024, k = 1, n_lwe = 630,
BSK (10, 3), KSK (4, 4), t = 4; random key words (a rate needs no valid keys).  Per batch: rows / s of
fhe_tfhe_lut_bootstrap_dev on a batch that mixes 8 tables and two-operand combinations, and of
fhe_tfhe_gadget_bootstrap_dev with one table on the same batch, alternating three times in one process; the per-kernel
split of both (fhe_ntt_kernel_timing_*), the init kernels side by side; the spread of the single-table runs themselves.
Then the wall time of one LutCircuit.evaluate of the 4-digit base-4 adder over 256 pairs.  Diagnostic only (the contract
bench is bench.py).  Usage: tools/lut_rate.py [tag] [batch ...]  ->  profiles/<tag>_lut_rate.json"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import fhe_study_amd as pkg
from fhe_study_amd import tfhe

from _timing import timeit                           # warm clocks: tools/_timing.py
from bootstrap_rate import kernel_split, rand
from gate_rate import kernel_ms

B, L = pkg.binding, pkg.load_library()
st = torch.cuda.current_stream().cuda_stream
N, K, NL, T = 1024, 1, 630, 4
BSK, KSK = (10, 3), (4, 4)
LUTS = 8
PARTS = {"digit_mac32_gcmux": "blind_rotation", "digit_tail32_cmux": "blind_rotation", "tlwe_gadget_key_switch": "key_switch",
         "tfhe_lut_init": "init", "tfhe_br_init": "init", "tglwe_sample_extract": "extract"}


def split_parts(ks):
    out = {}
    for k, v in ks.items():
        p = PARTS.get(k.rsplit("_", 1)[0], "other")                     # timer names end in _<log2 N> (_0: the key switch)
        out[p] = out.get(p, 0.0) + v["ms_per_call"]
    return out


def adder(c, digits):
    msg, carry_t = tfhe.make_lut(lambda v: v % 4, T), tfhe.make_lut(lambda v: v // 4, T)
    a = [c.input() for _ in range(digits)]
    b = [c.input() for _ in range(digits)]
    carry = None
    for i in range(digits):
        s = c.lin(a[i], 1, b[i], 1)
        c.output(c.lut(msg, s, 1, carry, 0 if carry is None else 1))
        carry = c.lut(carry_t, s, 1, carry, 0 if carry is None else 1)
    c.output(carry)
    return c


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    batches = [int(x) for x in sys.argv[2:]] or [64, 256, 1024, 4096]
    b, l = BSK
    ks_b, ks_l = KSK
    bsk = rand((NL, K + 1, l, K + 1, N), 1)
    ksk = rand((N, ks_l, NL + 1), 2)
    btk = tfhe.BootstrappingKey(N, K, l, NL, bsk, ksk, ks_l=ks_l, log_beta=b, ks_log_beta=ks_b)
    del bsk
    prep = btk.bsk
    luts = rand((LUTS, 1 << T), 3)
    tv = rand((K + 1, N), 5)
    tv[0] = 0
    res = {"shape": {"n": N, "k": K, "n_lwe": NL, "bsk": BSK, "ksk": KSK, "t_bits": T, "luts": LUTS}, "batches": {}}
    rng = np.random.default_rng(9)
    for batch in batches:
        pool = rand((2 * batch, NL + 1), 4 + batch)
        i = np.arange(batch, dtype=np.int64)
        d = np.stack([rng.integers(0, LUTS, batch), i, i + batch, rng.integers(1, 5, batch), rng.integers(-4, 0, batch),
                      rng.integers(0, 32, batch) << (31 - T)], axis=1)
        desc = torch.from_numpy((d & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
        out = torch.empty((batch, NL + 1), dtype=torch.int64, device="cuda")
        lut = lambda: B._check(L.fhe_tfhe_lut_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), T, luts.data_ptr(), LUTS,
                                                            pool.data_ptr(), 2 * batch, desc.data_ptr(), out.data_ptr(), batch, st))
        boot = lambda: B._check(L.fhe_tfhe_gadget_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), tv.data_ptr(), ks_b, ks_l, ksk.data_ptr(),
                                                                pool.data_ptr(), out.data_ptr(), batch, st))
        t_lut, t_boot, k_lut, k_boot = [], [], [], []
        for _ in range(3):                                                 # alternating: clocks and neighbours drift
            t_lut.append(timeit(lut, 0.2, 0.4, 3))
            t_boot.append(timeit(boot, 0.2, 0.4, 3))
            k_lut.append(kernel_split(lut, 3))
            k_boot.append(kernel_split(boot, 3))
        km_lut, km_boot = [kernel_ms(k) for k in k_lut], [kernel_ms(k) for k in k_boot]
        tl, tb = statistics.median(t_lut), statistics.median(t_boot)
        ml, mb = statistics.median(km_lut), statistics.median(km_boot)
        pl, pb = split_parts(k_lut[1]), split_parts(k_boot[1])
        x = {"lut_rows_per_s": batch / tl, "gadget_bootstraps_per_s": batch / tb, "lut_wall_ms": tl * 1e3, "bootstrap_wall_ms": tb * 1e3,
             "lut_wall_ms_runs": [t * 1e3 for t in t_lut], "bootstrap_wall_ms_runs": [t * 1e3 for t in t_boot],
             "lut_kernel_ms_runs": km_lut, "bootstrap_kernel_ms_runs": km_boot, "lut_kernel_ms": ml, "bootstrap_kernel_ms": mb,
             "lut_over_bootstrap_kernel": ml / mb, "lut_over_bootstrap_wall": tl / tb,
             "bootstrap_kernel_spread": (max(km_boot) - min(km_boot)) / mb, "bootstrap_wall_spread": (max(t_boot) - min(t_boot)) / tb,
             "lut_init_ms": pl.get("init"), "br_init_ms": pb.get("init"), "parts_lut_ms": pl, "parts_bootstrap_ms": pb,
             "kernel_timing_lut_ms": k_lut[1], "kernel_timing_bootstrap_ms": k_boot[1]}
        res["batches"][str(batch)] = x
        print(json.dumps({"batch": batch, **{k: v for k, v in x.items() if not k.startswith(("kernel_timing", "parts"))}}), flush=True)
        del pool, desc, out
    # the 4-digit base-4 adder over 256 pairs: 8 inputs of batch 256, 4 bootstrap calls of 512 rows and one lincomb
    circ = adder(tfhe.LutCircuit(), 4)
    plan = circ.plan()
    words = rng.integers(0, 1 << 64, (8, 256, NL + 1), dtype=np.uint64, endpoint=False)
    ins = [tfhe.TLWE(w) for w in words]
    circ.evaluate(btk, ins, T)                                             # warm: workspaces, tables, clocks
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        circ.evaluate(btk, ins, T)
        walls.append(time.perf_counter() - t0)
    res["radix_adder4_256_pairs"] = {"pairs": 256, "levels": plan.depth, "lookups": sum(v["luts"][1] for v in plan.levels),
                                     "bootstrap_calls": len(plan.levels), "lincomb_calls": sum(len(v) for v in plan.lins.values()),
                                     "wall_ms": statistics.median(walls) * 1e3, "wall_ms_runs": [w * 1e3 for w in walls]}
    print(json.dumps({"radix_adder4_256_pairs": res["radix_adder4_256_pairs"]}), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_lut_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
