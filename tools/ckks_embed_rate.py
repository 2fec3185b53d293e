#!/usr/bin/env python3
"""tools/ckks_embed_rate.py — the cost of the two-pass CKKS encoder on one GPU:
fhe_ckks_embed_encode_dev and fhe_ckks_embed_decode_dev at N = 2^14, 2^15 and 2^16 over 2^26 words a call (batch 4096, 2048,
1024: sustained, the chunks of a call back to back), as polynomials/s and bytes/s (32 N bytes per polynomial: 8 N read, 8 N
through the workspace each way, 8 N written), beside fhe_ntt_forward_dev at the same N, batch and the 61-bit modulus in the
same process, with the ratio, and the library's per-kernel timer for the four kernels; and the same three calls at a batch of one
chunk (2^21 words: one launch of each pass), which is what a sustained encoder call repeats 32 times while the NTT covers its
batch in two launches.
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_embed_rate.py [tag]  ->  profiles/<tag>_ckks_embed_rate.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import fhe_study_amd as pkg

from _timing import timeit                           # warm clocks: tools/_timing.py

B = pkg.binding
WORDS = 1 << 26


def kernel_ms(f, reps=10):
    B.kernel_timing_enable(True)
    B.kernel_timing_reset()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    out = {k: v[0] / reps for k, v in B.kernel_timing_read().items()}
    B.kernel_timing_enable(False)
    return out


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"shape": {"words_per_call": WORDS}}
    delta = float(1 << 30)
    for n in (1 << 14, 1 << 15, 1 << 16):
        batch = WORDS // n
        tw = torch.from_numpy(B.ckks_embed_twiddles(n).view(np.float64)).cuda()
        z = torch.randint(-8, 8, (batch, n // 2, 2), dtype=torch.int64, device="cuda").to(torch.float64)
        p = torch.empty((batch, n), dtype=torch.int64, device="cuda")
        back = torch.empty((batch, n // 2, 2), dtype=torch.float64, device="cuda")
        enc = lambda: B.ckks_embed_encode_dev(n, delta, tw.data_ptr(), z.data_ptr(), n // 2, p.data_ptr(), batch)
        dec = lambda: B.ckks_embed_decode_dev(n, delta, tw.data_ptr(), p.data_ptr(), back.data_ptr(), batch)
        enc(); dec(); torch.cuda.synchronize()
        err = float((back - z).abs().max())
        assert err < 1e-5, err                                         # the rounding moves a slot by at most sqrt(N) / Delta
        plan = pkg.Plan(pkg.Q61, n)
        a = torch.randint(0, 1 << 60, (batch, n), dtype=torch.int64, device="cuda")
        b = torch.empty_like(a)
        ntt = lambda: plan.forward_dev(a.data_ptr(), b.data_ptr(), batch)
        te, td, tn = (timeit(f, 0.3, 0.6, 3) for f in (enc, dec, ntt))
        row = lambda t, b=batch: {"ms": t * 1e3, "poly_per_s": b / t, "bytes_per_s": 32 * n * b / t}
        chunk = B.ckks_embed_workspace_bytes(n, batch) // (8 * n)
        enc1 = lambda: B.ckks_embed_encode_dev(n, delta, tw.data_ptr(), z.data_ptr(), n // 2, p.data_ptr(), chunk)
        dec1 = lambda: B.ckks_embed_decode_dev(n, delta, tw.data_ptr(), p.data_ptr(), back.data_ptr(), chunk)
        ntt1 = lambda: plan.forward_dev(a.data_ptr(), b.data_ptr(), chunk)
        te1, td1, tn1 = (timeit(f, 0.3, 0.6, 3) for f in (enc1, dec1, ntt1))
        res[f"n{n}"] = {"batch": batch, "chunk": chunk, "encode": row(te), "decode": row(td),
                        "fhe_ntt_forward_dev_q61": row(tn), "encode_over_ntt_rate": tn / te, "decode_over_ntt_rate": tn / td,
                        "one_chunk": {"encode": row(te1, chunk), "decode": row(td1, chunk), "fhe_ntt_forward_dev_q61": row(tn1, chunk),
                                      "encode_over_ntt_rate": tn1 / te1, "decode_over_ntt_rate": tn1 / td1},
                        "kernels_ms": kernel_ms(lambda: (enc(), dec(), ntt())), "round_trip_max_error": err}
        del z, p, back, a, b
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_embed_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
