#!/usr/bin/env python3
"""tools/tree_lookup_rate.py — the cost of a two-digit tree lookup on one GPU: N = 1024, k = 1, n_lwe = 630,
BSK (10, 3), KSK (4, 4), PKSK (8, 4), t = 3, nu = 0; random key words (a rate needs no valid keys).  In one process,
alternating three runs each, per batch B:
  - fhe_tlwe_gadget_packing_key_switch_dev over B groups of 8 against fhe_tlwe_gadget_private_key_switch_dev (PFKSK (8, 4))
    over the same 8 B inputs: kernel time per input, the PFKS's per input and per function scaled by the row ratio
    n_in / (k N + 1) of the two keys;
  - fhe_tfhe_gadget_bootstrap_rows_dev against fhe_tfhe_gadget_bootstrap_dev at batch B (only the init kernel differs);
  - a whole tree lookup on device buffers (lut bootstrap over 8 B rows, packing key switch, box expansion, bootstrap_rows
    over B rows) against fhe_tfhe_lut_bootstrap_dev over 9 B rows, with the share of packing + expansion + rows init.
Beside each ratio, the spread of the baseline's own runs.  Diagnostic only (the contract bench is bench.py).
Usage: tools/tree_lookup_rate.py [tag] [batch ...]  ->  profiles/<tag>_tree_lookup_rate.json"""
import json, os, statistics, sys
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
N, K, NL, T = 1024, 1, 630, 3
BSK, KSK, PKS, PF = (10, 3), (4, 4), (8, 4), (8, 4)
P, LOGN = 1 << T, 10


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def med(ks, name):
    return statistics.median([k[name]["ms_per_call"] for k in ks])


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
    pksk = rand((NL, PKS[1], K + 1, N), 3)
    pfksk = rand((L.fhe_tfhe_pfksk_words(N, K, *PF),), 4)
    luts = rand((P, P), 5)
    row = NL + 1
    res = {"shape": {"n": N, "k": K, "n_lwe": NL, "bsk": BSK, "ksk": KSK, "pksk": PKS, "pfksk": PF, "t_bits": T, "nu": 0,
                     "pksk_mb": pksk.numel() * 8 / 1e6, "pfksk_mb": pfksk.numel() * 8 / 1e6}, "batches": {}}
    for batch in batches:
        x, y = rand((batch, row), 10 + batch), rand((batch, row), 11 + batch)
        g = np.arange(batch, dtype=np.int64)
        dev = lambda d: torch.from_numpy((d & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
        z = np.zeros(P * batch, dtype=np.int64)
        d8 = dev(np.stack([np.tile(np.arange(P), batch), np.repeat(g, P), z + 0xFFFFFFFF, z + 1, z, z], axis=1))
        z9 = np.zeros(9 * batch, dtype=np.int64)
        d9 = dev(np.stack([np.arange(9 * batch) % P, np.arange(9 * batch) % batch, z9 + 0xFFFFFFFF, z9 + 1, z9, z9], axis=1))
        lvl1 = torch.empty((P * batch, row), dtype=torch.int64, device="cuda")
        out9 = torch.empty((9 * batch, row), dtype=torch.int64, device="cuda")
        packed = torch.empty((batch, K + 1, N), dtype=torch.int64, device="cuda")
        tv = torch.empty_like(packed)
        out = torch.empty((batch, row), dtype=torch.int64, device="cuda")
        pf_in = rand((P * batch, N + 1), 12 + batch)
        pf_out = torch.empty((P * batch, K + 1, K + 1, N), dtype=torch.int64, device="cuda")
        lut = lambda desc, rows, dst: B._check(L.fhe_tfhe_lut_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), T, luts.data_ptr(),
                                                                            P, y.data_ptr(), batch, desc.data_ptr(), dst.data_ptr(), rows, st))
        pks = lambda: B._check(L.fhe_tlwe_gadget_packing_key_switch_dev(N, K, NL, PKS[0], PKS[1], pksk.data_ptr(), lvl1.data_ptr(), P * row, row, P,
                                                                        LOGN - T, packed.data_ptr(), batch, st))
        pfks = lambda: B._check(L.fhe_tlwe_gadget_private_key_switch_dev(N, K, PF[0], PF[1], pfksk.data_ptr(), pf_in.data_ptr(), pf_out.data_ptr(),
                                                                         P * batch, st))
        expand = lambda: B._check(L.fhe_tglwe_box_expand_dev(N, K, T, packed.data_ptr(), tv.data_ptr(), batch, st))
        rows_ = lambda: B._check(L.fhe_tfhe_gadget_bootstrap_rows_dev(N, K, b, l, NL, prep.data_ptr(), tv.data_ptr(), ks_b, ks_l, ksk.data_ptr(),
                                                                      x.data_ptr(), out.data_ptr(), batch, st))
        boot = lambda: B._check(L.fhe_tfhe_gadget_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), tv.data_ptr(), ks_b, ks_l, ksk.data_ptr(),
                                                                x.data_ptr(), out.data_ptr(), batch, st))

        def tree():
            lut(d8, P * batch, lvl1); pks(); expand(); rows_()

        nine = lambda: lut(d9, 9 * batch, out9)
        tree()
        torch.cuda.synchronize()
        w = {k: [] for k in ("tree", "nine", "rows", "boot")}
        ks = {k: [] for k in ("tree", "nine", "rows", "boot", "pks", "pfks")}
        fs = {"tree": tree, "nine": nine, "rows": rows_, "boot": boot, "pks": pks, "pfks": pfks}
        order = list(fs)
        for r in range(3):                                                     # alternating: clocks and neighbours drift
            for k in w:
                w[k].append(timeit(fs[k], 0.2, 0.4, 3))
            for k in order[r:] + order[:r]:                                    # rotated: the first split after a timed loop pays for
                ks[k].append(kernel_split(fs[k], 3))                           # switching the timers on, in its first kernel
        m = {k: statistics.median(v) for k, v in w.items()}
        km = {k: [kernel_ms(s) for s in v] for k, v in ks.items()}
        kmed = {k: statistics.median(v) for k, v in km.items()}
        inputs = P * batch
        pks_us = kmed["pks"] * 1e3 / inputs
        pfks_us = kmed["pfks"] * 1e3 / inputs / (K + 1)                         # per input and per function
        scaled = pfks_us * NL / (K * N + 1)                                     # row ratio n_in l_p / ((k N + 1) l_p)
        glue = med(ks["tree"], f"tlwe_packing_ks_{LOGN}") + med(ks["tree"], f"tglwe_box_expand_{LOGN}") + med(ks["tree"], f"tfhe_br_rows_init_{LOGN}")
        res["batches"][str(batch)] = xr = {
            "pks": {"inputs": inputs, "kernel_ms": kmed["pks"], "kernel_ms_runs": km["pks"], "us_per_input": pks_us,
                    "pfks_kernel_ms": kmed["pfks"], "pfks_kernel_ms_runs": km["pfks"], "pfks_us_per_input_per_function": pfks_us,
                    "pfks_scaled_by_rows_us": scaled, "pks_over_scaled_pfks": pks_us / scaled, "pfks_kernel_spread": spread(km["pfks"])},
            "bootstrap_rows": {"rows_wall_ms": m["rows"] * 1e3, "boot_wall_ms": m["boot"] * 1e3, "rows_over_boot_wall": m["rows"] / m["boot"],
                               "rows_kernel_ms": kmed["rows"], "boot_kernel_ms": kmed["boot"], "rows_over_boot_kernel": kmed["rows"] / kmed["boot"],
                               "boot_wall_spread": spread(w["boot"]), "boot_kernel_spread": spread(km["boot"]),
                               "init_ms": {"tfhe_br_rows_init": med(ks["rows"], f"tfhe_br_rows_init_{LOGN}"),
                                           "tfhe_br_init": med(ks["boot"], f"tfhe_br_init_{LOGN}")},
                               "rows_wall_ms_runs": [t * 1e3 for t in w["rows"]], "boot_wall_ms_runs": [t * 1e3 for t in w["boot"]]},
            "tree_lookup": {"tree_wall_ms": m["tree"] * 1e3, "nine_rows_wall_ms": m["nine"] * 1e3, "tree_over_nine_wall": m["tree"] / m["nine"],
                            "tree_kernel_ms": kmed["tree"], "nine_rows_kernel_ms": kmed["nine"], "tree_over_nine_kernel": kmed["tree"] / kmed["nine"],
                            "nine_wall_spread": spread(w["nine"]), "nine_kernel_spread": spread(km["nine"]), "lookups_per_s": batch / m["tree"],
                            "pks_expand_init_ms": glue, "pks_expand_init_share_of_kernel_time": glue / kmed["tree"],
                            "tree_wall_ms_runs": [t * 1e3 for t in w["tree"]], "nine_rows_wall_ms_runs": [t * 1e3 for t in w["nine"]],
                            "kernel_timing_tree_ms": ks["tree"][1]}}
        print(json.dumps({"batch": batch, "pks": xr["pks"], "bootstrap_rows": xr["bootstrap_rows"],
                          "tree_lookup": {k: v for k, v in xr["tree_lookup"].items() if k != "kernel_timing_tree_ms"}}), flush=True)
        del x, y, d8, d9, lvl1, out9, packed, tv, out, pf_in, pf_out
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_tree_lookup_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
