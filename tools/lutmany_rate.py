#!/usr/bin/env python3
"""tools/lutmany_rate.py — what sharing a blind rotation buys on one GPU: N = 1024, k = 1, n_lwe = 630,
BSK (10, 3), KSK (4, 4), t = 3; random key words (a rate needs no valid keys).  In one process, alternating three runs each:
  - fhe_tfhe_lut_many_bootstrap_dev with nu = 1 at batch B against fhe_tfhe_lut_bootstrap_dev at batch 2B (the same 2B
    outputs: every input looked up in two tables), wall and kernel time, with the per-kernel split of both;
  - the new init kernel against tfhe_lut_init at the same rows (nu = 0 and nu = 1 at batch B against the old kernel at B);
  - LutCircuit.evaluate of the 4-digit base-4 adder over 256 pairs with share=1 against share=0, wall time.
Beside each ratio, the spread of the baseline's own runs.  Diagnostic only (the contract bench is bench.py).
Usage: tools/lutmany_rate.py [tag] [batch ...]  ->  profiles/<tag>_lutmany_rate.json"""
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
N, K, NL, T, NU = 1024, 1, 630, 3, 1
BSK, KSK = (10, 3), (4, 4)
LUTS = 8
PARTS = {"digit_mac32_gcmux": "blind_rotation", "digit_tail32_cmux": "blind_rotation", "tlwe_gadget_key_switch": "key_switch",
         "tfhe_lut_init": "init", "tfhe_lut_many_init": "init", "tglwe_sample_extract": "extract", "tfhe_many_extract": "extract"}


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


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    batches = [int(x) for x in sys.argv[2:]] or [64, 256, 1024, 2048]
    b, l = BSK
    ks_b, ks_l = KSK
    bsk = rand((NL, K + 1, l, K + 1, N), 1)
    ksk = rand((N, ks_l, NL + 1), 2)
    btk = tfhe.BootstrappingKey(N, K, l, NL, bsk, ksk, ks_l=ks_l, log_beta=b, ks_log_beta=ks_b)
    del bsk
    prep = btk.bsk
    luts = rand((LUTS, 1 << T), 3)
    F = 1 << NU
    res = {"shape": {"n": N, "k": K, "n_lwe": NL, "bsk": BSK, "ksk": KSK, "t_bits": T, "nu": NU, "luts": LUTS}, "batches": {}}
    rng = np.random.default_rng(9)
    for batch in batches:
        pool = rand((2 * batch, NL + 1), 4 + batch)
        i = np.arange(batch, dtype=np.int64)
        d = np.stack([rng.integers(0, LUTS // F, batch) * F, i, i + batch, rng.integers(1, 5, batch), rng.integers(-4, 0, batch),
                      rng.integers(0, 2 << T, batch) << (31 - T)], axis=1)
        d2 = np.concatenate([d + (h, 0, 0, 0, 0, 0) for h in range(F)])        # the unshared call: every row once per table
        dev = lambda x: torch.from_numpy((x & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
        desc, desc2 = dev(d), dev(d2)
        out = torch.empty((F * batch, NL + 1), dtype=torch.int64, device="cuda")
        many = lambda nu=NU: B._check(L.fhe_tfhe_lut_many_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), T, nu,
                                                                        luts.data_ptr(), LUTS, pool.data_ptr(), 2 * batch, desc.data_ptr(),
                                                                        out.data_ptr(), batch, st))
        one = lambda rows=F * batch, dd=desc2: B._check(L.fhe_tfhe_lut_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), T,
                                                                                     luts.data_ptr(), LUTS, pool.data_ptr(), 2 * batch,
                                                                                     dd.data_ptr(), out.data_ptr(), rows, st))
        many()
        torch.cuda.synchronize()
        got = out.clone()
        one()
        torch.cuda.synchronize()
        same_rows = int((got == out).all(dim=1).sum())                          # not equal in general: nu = 1 rounds the mod switch coarser
        t_many, t_one, k_many, k_one, k_many0, k_oneB = [], [], [], [], [], []
        splits = [(k_many, many), (k_one, one), (k_many0, lambda: many(0)),    # the init kernels at the same rows: batch
                  (k_oneB, lambda: one(batch, desc))]
        for r in range(3):                                                     # alternating: clocks and neighbours drift
            t_many.append(timeit(many, 0.2, 0.4, 3))
            t_one.append(timeit(one, 0.2, 0.4, 3))
            for ks, f in splits[r:] + splits[:r]:                              # rotated: the first split after a timed loop pays for
                ks.append(kernel_split(f, 3))                                  # switching the timers on, in its first kernel
        km_many, km_one = [kernel_ms(k) for k in k_many], [kernel_ms(k) for k in k_one]
        tm, to = statistics.median(t_many), statistics.median(t_one)
        mm, mo = statistics.median(km_many), statistics.median(km_one)
        init = lambda ks, name: statistics.median([k[f"{name}_10"]["ms_per_call"] for k in ks])
        x = {"outputs": F * batch, "many_wall_ms": tm * 1e3, "one_wall_ms": to * 1e3, "many_wall_ms_runs": [t * 1e3 for t in t_many],
             "one_wall_ms_runs": [t * 1e3 for t in t_one], "many_kernel_ms": mm, "one_kernel_ms": mo, "many_kernel_ms_runs": km_many,
             "one_kernel_ms_runs": km_one, "many_over_one_wall": tm / to, "many_over_one_kernel": mm / mo,
             "one_wall_spread": spread(t_one), "one_kernel_spread": spread(km_one), "outputs_per_s_many": F * batch / tm,
             "outputs_per_s_one": F * batch / to, "rows_equal_to_the_unshared_call": same_rows,
             "init_ms": {"tfhe_lut_many_init_nu1": init(k_many, "tfhe_lut_many_init"), "tfhe_lut_many_init_nu0": init(k_many0, "tfhe_lut_many_init"),
                         "tfhe_lut_init_same_rows": init(k_oneB, "tfhe_lut_init"), "tfhe_lut_init_2x_rows": init(k_one, "tfhe_lut_init"),
                         "tfhe_lut_many_init_nu1_runs": [k["tfhe_lut_many_init_10"]["ms_per_call"] for k in k_many],
                         "tfhe_lut_many_init_nu0_runs": [k["tfhe_lut_many_init_10"]["ms_per_call"] for k in k_many0],
                         "tfhe_lut_init_same_rows_runs": [k["tfhe_lut_init_10"]["ms_per_call"] for k in k_oneB],
                         "tfhe_lut_init_2x_rows_runs": [k["tfhe_lut_init_10"]["ms_per_call"] for k in k_one]},
             "parts_many_ms": split_parts(k_many[1]), "parts_one_ms": split_parts(k_one[1]),
             "kernel_timing_many_ms": k_many[1], "kernel_timing_one_ms": k_one[1]}
        res["batches"][str(batch)] = x
        print(json.dumps({"batch": batch, **{k: v for k, v in x.items() if not k.startswith(("kernel_timing", "parts"))}}), flush=True)
        del pool, desc, desc2, out, got
    # the 4-digit base-4 adder over 256 pairs: share=1 runs 4 nu = 1 calls of 256 rows, share=0 4 calls of 512 rows
    circ = adder(tfhe.LutCircuit(), 4)
    words = rng.integers(0, 1 << 64, (8, 256, NL + 1), dtype=np.uint64, endpoint=False)
    ins = [tfhe.TLWE(w) for w in words]
    walls = {0: [], 1: []}
    for share in (1, 0):
        circ.evaluate(btk, ins, T, share=share)                                # warm: workspaces, tables, clocks
    for _ in range(3):
        for share in (1, 0):
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                circ.evaluate(btk, ins, T, share=share)
                walls[share].append(time.perf_counter() - t0)
    m1, m0 = statistics.median(walls[1]), statistics.median(walls[0])
    res["radix_adder4_256_pairs"] = {"pairs": 256, "share1_wall_ms": m1 * 1e3, "share0_wall_ms": m0 * 1e3, "share1_over_share0": m1 / m0,
                                     "share0_spread": spread(walls[0]), "share1_wall_ms_runs": [w * 1e3 for w in walls[1]],
                                     "share0_wall_ms_runs": [w * 1e3 for w in walls[0]]}
    print(json.dumps({"radix_adder4_256_pairs": res["radix_adder4_256_pairs"]}), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_lutmany_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
