#!/usr/bin/env python3
"""tools/circuit_bootstrap_rate.py — TFHE circuit bootstrapping rate on one GPU: N = 1024, k = 1,
n_lwe = 630, BSK (b, l) = (10, 3), circuit-bootstrap output (6, 2), PFKS (8, 4); random key words (a rate needs no valid
keys).  Per batch: circuit bootstraps / s of fhe_tfhe_circuit_bootstrap_dev followed by fhe_tggsw_gadget_prepare_many_dev
(the TGGSWs ready for a CMux), the per-kernel split into blind rotation, PFKS, preparation and glue
(fhe_ntt_kernel_timing_*), and the kernel time of fhe_tggsw_gadget_cmux_dev (a key per ciphertext) against
fhe_tggsw_gadget_external_product_dev (one shared key) at the same batch.  Diagnostic only (the contract bench is bench.py).
Usage: tools/circuit_bootstrap_rate.py [tag] [batch ...]  ->  profiles/<tag>_circuit_bootstrap_rate.json"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import fhe_study_amd as pkg

from _timing import timeit                           # warm clocks: tools/_timing.py
from bootstrap_rate import kernel_split, rand

B, L = pkg.binding, pkg.load_library()
st = torch.cuda.current_stream().cuda_stream
N, K, NL = 1024, 1, 630
BSK, CB, PF = (10, 3), (6, 2), (8, 4)
# kernel -> part of a circuit bootstrap
PARTS = {"digit_mac32_gcmux": "blind_rotation", "digit_tail32_cmux": "blind_rotation", "tlwe_private_ks": "pfks",
         "ntt32_fwd_key": "preparation", "tfhe_cb_init": "glue", "tfhe_cb_extract": "glue"}


def split_parts(ks):
    out = {}
    for k, v in ks.items():
        p = PARTS.get(k.rsplit("_", 1)[0], "other")                     # timer names end in _<log2 N>
        out[p] = out.get(p, 0.0) + v["ms_per_call"]
    tot = sum(out.values())
    return {p: {"ms": v, "share": v / tot} for p, v in out.items()}


def kernel_ms(ks):
    return sum(v["ms_per_call"] for v in ks.values())


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    batches = [int(x) for x in sys.argv[2:]] or [64, 256, 1024, 4096]
    b, l = BSK
    cb_b, cb_l = CB
    pf_b, pf_l = PF
    words = L.fhe_tfhe_gadget_bsk_prepared_words(N, K, b, l, NL)
    bsk = rand((NL, K + 1, l, K + 1, N), 1)
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    B._check(L.fhe_tfhe_gadget_bsk_prepare_dev(N, K, b, l, NL, bsk.data_ptr(), prep.data_ptr(), st))
    del bsk
    pfksk = rand((L.fhe_tfhe_pfksk_words(N, K, pf_b, pf_l),), 2)
    tw = L.fhe_tggsw_gadget_prepared_words(N, K, cb_b, cb_l)
    torch.cuda.synchronize()
    res = {"shape": {"n": N, "k": K, "n_lwe": NL, "bsk": BSK, "cb": CB, "pfks": PF, "bsk_prepared_mb": words * 8 / 1e6,
                     "pfksk_mb": pfksk.numel() * 8 / 1e6},
           "batches": {}}
    for batch in batches:
        lwe = rand((batch, NL + 1), 4 + batch)
        tg = torch.empty((batch, K + 1, cb_l, K + 1, N), dtype=torch.int64, device="cuda")
        tp = torch.empty(batch * tw, dtype=torch.int64, device="cuda")

        def cbs():
            B._check(L.fhe_tfhe_circuit_bootstrap_dev(N, K, b, l, NL, prep.data_ptr(), cb_b, cb_l, pf_b, pf_l, pfksk.data_ptr(), lwe.data_ptr(),
                                                      tg.data_ptr(), batch, st))
            B._check(L.fhe_tggsw_gadget_prepare_many_dev(N, K, cb_b, cb_l, batch, tg.data_ptr(), tp.data_ptr(), st))

        t = timeit(cbs, 0.3, 0.5, 3)
        ks = kernel_split(cbs, 2)
        # the CMux with the batch's own TGGSWs against the shared-key product of the same batch
        c0, c1 = rand((batch, K + 1, N), 7), rand((batch, K + 1, N), 8)
        out = torch.empty((batch, K + 1, N), dtype=torch.int64, device="cuda")
        idx = torch.randperm(batch, device="cuda").to(torch.int32)
        cmux = lambda: B._check(L.fhe_tggsw_gadget_cmux_dev(N, K, cb_b, cb_l, batch, tp.data_ptr(), idx.data_ptr(), c0.data_ptr(), c1.data_ptr(),
                                                            out.data_ptr(), batch, st))
        ext = lambda: B._check(L.fhe_tggsw_gadget_external_product_dev(N, K, cb_b, cb_l, tp.data_ptr(), c0.data_ptr(), out.data_ptr(), batch, st))
        idx0 = torch.zeros(batch, dtype=torch.int32, device="cuda")        # every selector the same TGGSW (a CMux-tree level)
        cmux0 = lambda: B._check(L.fhe_tggsw_gadget_cmux_dev(N, K, cb_b, cb_l, batch, tp.data_ptr(), idx0.data_ptr(), c0.data_ptr(), c1.data_ptr(),
                                                             out.data_ptr(), batch, st))
        t_cmux, t_ext = timeit(cmux, 0.2, 0.3, 3), timeit(ext, 0.2, 0.3, 3)
        timeit(cmux0, 0.1, 0.1, 3)
        k_cmux, k_ext, k_cmux0 = kernel_split(cmux, 5), kernel_split(ext, 5), kernel_split(cmux0, 5)
        x = {"circuit_bootstrap_s": t, "circuit_bootstraps_per_s": batch / t, "kernel_ms": kernel_ms(ks), "parts": split_parts(ks),
             "cmux_wall_us": t_cmux * 1e6, "shared_product_wall_us": t_ext * 1e6,
             "cmux_kernel_us": kernel_ms(k_cmux) * 1e3, "shared_product_kernel_us": kernel_ms(k_ext) * 1e3,
             "cmux_over_shared_kernel": kernel_ms(k_cmux) / kernel_ms(k_ext), "cmux_one_selector_kernel_us": kernel_ms(k_cmux0) * 1e3,
             "key_bytes_per_ciphertext": tw * 8,
             "kernel_timing_ms": ks, "kernel_timing_cmux_ms": k_cmux, "kernel_timing_shared_product_ms": k_ext,
             "kernel_timing_cmux_one_selector_ms": k_cmux0}
        res["batches"][str(batch)] = x
        print(json.dumps({"batch": batch, **{k: v for k, v in x.items() if not k.startswith("kernel_timing")}}), flush=True)
        del lwe, tg, tp, c0, c1, out, idx, idx0
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_circuit_bootstrap_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
