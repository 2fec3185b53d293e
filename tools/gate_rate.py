#!/usr/bin/env python3
"""tools/gate_rate.py — TFHE boolean gate rate on one GPU: N = 1024, k = 1, n_lwe = 630, BSK (10, 3),
KSK (4, 4); random key words (a rate needs no valid keys).  Per batch: gates / s of fhe_tfhe_gate_bootstrap_dev on a
mixed-op batch and of fhe_tfhe_gadget_bootstrap_dev (the mu test vector) on the same batch, alternating in one process;
MUXes / s of fhe_tfhe_gate_mux_dev; the per-kernel split of all three (fhe_ntt_kernel_timing_*).  Then the wall time of one
Circuit.evaluate of a 4-bit ripple-carry adder over all 256 input pairs (host upload and download included).  Diagnostic
only (the contract bench is bench.py).  Usage: tools/gate_rate.py [tag] [batch ...]  ->  profiles/<tag>_gate_rate.json"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import fhe_study_amd as pkg
from fhe_study_amd import tfhe

from _timing import timeit                           # warm clocks: tools/_timing.py
from bootstrap_rate import kernel_split, rand

B, L = pkg.binding, pkg.load_library()
st = torch.cuda.current_stream().cuda_stream
N, K, NL = 1024, 1, 630
BSK, KSK = (10, 3), (4, 4)
MU = 1 << 61
# kernel -> part of a gate
PARTS = {"digit_mac32_gcmux": "blind_rotation", "digit_tail32_cmux": "blind_rotation", "tlwe_gadget_key_switch": "key_switch",
         "tfhe_gate_init": "init", "tfhe_mux_init": "init", "tfhe_br_init": "init", "tglwe_sample_extract": "extract",
         "tfhe_mux_extract": "extract"}


def split_parts(ks):
    out = {}
    for k, v in ks.items():
        p = PARTS.get(k.rsplit("_", 1)[0], "other")                     # timer names end in _<log2 N> (_0: the key switch)
        out[p] = out.get(p, 0.0) + v["ms_per_call"]
    tot = sum(out.values())
    return {p: {"ms": v, "share": v / tot} for p, v in out.items()}


def kernel_ms(ks):
    return sum(v["ms_per_call"] for v in ks.values())


def adder(c, bits):
    x = [c.input() for _ in range(bits)]
    y = [c.input() for _ in range(bits)]
    carry = c.gate("AND", x[0], y[0])
    c.output(c.gate("XOR", x[0], y[0]))
    for i in range(1, bits):
        t = c.gate("XOR", x[i], y[i])
        c.output(c.gate("XOR", t, carry))
        carry = c.gate("OR", c.gate("AND", x[i], y[i]), c.gate("AND", t, carry))
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
    tv = torch.zeros((K + 1, N), dtype=torch.int64, device="cuda")
    tv[K] = MU
    res = {"shape": {"n": N, "k": K, "n_lwe": NL, "bsk": BSK, "ksk": KSK, "bsk_prepared_mb": prep.numel() * 8 / 1e6,
                     "ksk_mb": ksk.numel() * 8 / 1e6},
           "batches": {}}
    rng = np.random.default_rng(9)
    for batch in batches:
        pool = rand((2 * batch, NL + 1), 4 + batch)
        i = np.arange(batch, dtype=np.uint32)
        gates = torch.from_numpy(np.stack([rng.integers(0, B.FHE_GATE_COUNT, batch).astype(np.uint32), i, i + batch], axis=1).view(np.int32)).cuda()
        sel = torch.from_numpy(np.stack([i, i + batch, (i + 1) % batch], axis=1).view(np.int32)).cuda()
        out = torch.empty((batch, NL + 1), dtype=torch.int64, device="cuda")
        gate = lambda: B._check(L.fhe_tfhe_gate_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), pool.data_ptr(), 2 * batch,
                                                              gates.data_ptr(), out.data_ptr(), batch, st))
        boot = lambda: B._check(L.fhe_tfhe_gadget_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), tv.data_ptr(), ks_b, ks_l, ksk.data_ptr(),
                                                                pool.data_ptr(), out.data_ptr(), batch, st))
        mux = lambda: B._check(L.fhe_tfhe_gate_mux_dev(N, K, b, l, NL, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), pool.data_ptr(), 2 * batch,
                                                       sel.data_ptr(), out.data_ptr(), batch, st))
        t_gate, t_boot = [], []
        for _ in range(3):                                                 # alternating: clocks and neighbours drift
            t_gate.append(timeit(gate, 0.2, 0.4, 3))
            t_boot.append(timeit(boot, 0.2, 0.4, 3))
        t_mux = timeit(mux, 0.2, 0.4, 3)
        k_gate, k_boot, k_mux = kernel_split(gate, 3), kernel_split(boot, 3), kernel_split(mux, 3)
        tg, tb = statistics.median(t_gate), statistics.median(t_boot)
        x = {"gates_per_s": batch / tg, "gadget_bootstraps_per_s": batch / tb, "muxes_per_s": batch / t_mux,
             "gate_wall_ms": tg * 1e3, "bootstrap_wall_ms": tb * 1e3, "mux_wall_ms": t_mux * 1e3,
             "gate_wall_ms_runs": [t * 1e3 for t in t_gate], "bootstrap_wall_ms_runs": [t * 1e3 for t in t_boot],
             "gate_kernel_ms": kernel_ms(k_gate), "bootstrap_kernel_ms": kernel_ms(k_boot), "mux_kernel_ms": kernel_ms(k_mux),
             "gate_over_bootstrap_kernel": kernel_ms(k_gate) / kernel_ms(k_boot), "mux_over_gate_kernel": kernel_ms(k_mux) / kernel_ms(k_gate),
             "parts_gate": split_parts(k_gate), "parts_bootstrap": split_parts(k_boot), "parts_mux": split_parts(k_mux),
             "kernel_timing_gate_ms": k_gate, "kernel_timing_bootstrap_ms": k_boot, "kernel_timing_mux_ms": k_mux}
        res["batches"][str(batch)] = x
        print(json.dumps({"batch": batch, **{k: v for k, v in x.items() if not k.startswith(("kernel_timing", "parts"))}}), flush=True)
        del pool, gates, sel, out
    # one 4-bit adder over all 256 (x, y) pairs: 8 inputs of batch 256, 7 levels
    circ = adder(tfhe.Circuit(), 4)
    plan = circ.plan()
    words = rng.integers(0, 1 << 64, (8, 256, NL + 1), dtype=np.uint64, endpoint=False)
    ins = [tfhe.TLWE(w) for w in words]
    circ.evaluate(btk, ins)                                                # warm: workspaces, tables, clocks
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        circ.evaluate(btk, ins)
        walls.append(time.perf_counter() - t0)
    res["adder4_all_pairs"] = {"pairs": 256, "levels": plan.depth, "gates": sum(v["gates"][1] for v in plan.levels),
                               "gate_calls": sum(1 for v in plan.levels if v["gates"][1]), "wall_ms": statistics.median(walls) * 1e3,
                               "wall_ms_runs": [w * 1e3 for w in walls]}
    print(json.dumps({"adder4_all_pairs": res["adder4_all_pairs"]}), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_gate_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
