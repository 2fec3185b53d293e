#!/usr/bin/env python3
"""tools/ckks_client_rate.py — the cost of CKKS on the device on one GPU:
  - fhe_ckks_encode_dev and fhe_ckks_decode_dev at N = 4096 and 8192, batch 4096, as polynomials/s and bytes/s (16 N bytes
    per polynomial: 8 N read and 8 N written), beside fhe_ntt_forward_dev at the same N, batch and the 61-bit modulus in the
    same process (the same 16 N bytes), with the ratio, and the library's per-kernel timer for the two kernels;
  - fhe_ckks_encrypt_dev and fhe_ckks_decrypt_dev at the three shapes of §20's table, beside fhe_bfv_encrypt_dev and
    fhe_bfv_decrypt_dev (t = 2) measured in the same run;
  - the numpy restatement's time per row (tests/_ckks_numpy.py: encode and decode, the FFT form).
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_client_rate.py [tag]  ->  profiles/<tag>_ckks_client_rate.json"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fhe_study_amd as pkg
from fhe_study_amd import tfhe

import _ckks_numpy as K
from _timing import timeit                           # warm clocks: tools/_timing.py

B = pkg.binding
BATCH, NP_ROWS = 4096, 4
SEED = bytes(range(32))
TAB = tfhe.cdt_table(3.2)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def kernel_ms(f, reps=20):
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
    res = {"shape": {"batch": BATCH, "numpy_rows": NP_ROWS, "sigma": 3.2}}
    delta = float(1 << 30)
    for n in (4096, 8192):
        tw = torch.from_numpy(B.ckks_twiddles(n).view(np.float64)).cuda()
        z_np = K.random_case(n, n, NP_ROWS)
        z = torch.from_numpy(np.resize(z_np, (BATCH, n // 2)).view(np.float64)).cuda()
        p = torch.empty((BATCH, n), dtype=torch.int64, device="cuda")
        back = torch.empty((BATCH, n // 2, 2), dtype=torch.float64, device="cuda")
        enc = lambda: B.ckks_encode_dev(n, delta, tw.data_ptr(), z.data_ptr(), n // 2, p.data_ptr(), BATCH)
        dec = lambda: B.ckks_decode_dev(n, delta, tw.data_ptr(), p.data_ptr(), back.data_ptr(), BATCH)
        enc(); dec(); torch.cuda.synchronize()
        err = float(np.abs(back[:NP_ROWS].cpu().numpy().view(np.complex128).reshape(NP_ROWS, -1) - z_np).max())
        assert err < 1e-6, err                                         # the rounding moves a slot by at most sqrt(N) / Delta
        plan = pkg.Plan(pkg.Q61, n)
        a = torch.randint(0, 1 << 60, (BATCH, n), dtype=torch.int64, device="cuda")
        b = torch.empty_like(a)
        ntt = lambda: plan.forward_dev(a.data_ptr(), b.data_ptr(), BATCH)
        te, td, tn = (timeit(f, 0.3, 0.6, 3) for f in (enc, dec, ntt))
        t0 = time.perf_counter(); K.encode(z_np, delta); t_np_e = (time.perf_counter() - t0) / NP_ROWS
        m_np = p[:NP_ROWS].cpu().numpy()
        t0 = time.perf_counter(); K.decode(m_np, delta); t_np_d = (time.perf_counter() - t0) / NP_ROWS
        row = lambda t: {"ms": t * 1e3, "poly_per_s": BATCH / t, "bytes_per_s": 16 * n * BATCH / t}
        res[f"encoder_n{n}"] = {"encode": row(te), "decode": row(td), "fhe_ntt_forward_dev_q61": row(tn), "encode_over_ntt_rate": tn / te,
                                "decode_over_ntt_rate": tn / td, "kernels_ms": kernel_ms(lambda: (enc(), dec())),
                                "numpy_encode_ms_per_row": t_np_e * 1e3, "numpy_decode_ms_per_row": t_np_d * 1e3, "round_trip_max_error": err}
    d_tab, m = dev(TAB), len(TAB)
    for q, n in ((65537, 4096), (65537, 8192), (pkg.Q61, 4096)):
        plan = pkg.Plan(q, n)
        s, sb = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
        B.ckks_secret_key_dev(plan, SEED, 0, s.data_ptr())
        B.bfv_secret_key_dev(n, SEED, 0, sb.data_ptr())
        pk, pkb = torch.empty((2, n), dtype=torch.int64, device="cuda"), torch.empty((2, n), dtype=torch.int64, device="cuda")
        ev, evb, s_ev, sb_ev = torch.empty_like(pk), torch.empty_like(pk), torch.empty_like(s), torch.empty_like(s)
        B.ckks_public_key_dev(plan, SEED, 1, s.data_ptr(), d_tab.data_ptr(), m, pk.data_ptr())
        B.bfv_public_key_dev(plan, SEED, 1, sb.data_ptr(), d_tab.data_ptr(), m, pkb.data_ptr())
        for src, dst, rows in ((pk, ev, 2), (pkb, evb, 2), (s, s_ev, 1), (sb, sb_ev, 1)):
            plan.forward_dev(src.data_ptr(), dst.data_ptr(), rows)
        msg = torch.randint(-(q // 8), q // 8, (BATCH, n), dtype=torch.int64, device="cuda")
        msgb = torch.randint(0, 2, (BATCH, n), dtype=torch.int64, device="cuda")
        ct = torch.empty((2, BATCH, n), dtype=torch.int64, device="cuda")
        pt = torch.empty((BATCH, n), dtype=torch.int64, device="cuda")
        enc = lambda: B.ckks_encrypt_dev(plan, SEED, 0, ev.data_ptr(), msg.data_ptr(), n, d_tab.data_ptr(), m, ct.data_ptr(), BATCH)
        dec = lambda: B.ckks_decrypt_dev(plan, s_ev.data_ptr(), ct.data_ptr(), pt.data_ptr(), BATCH)
        encb = lambda: B.bfv_encrypt_dev(plan, 2, SEED, 0, evb.data_ptr(), msgb.data_ptr(), n, d_tab.data_ptr(), m, ct.data_ptr(), BATCH)
        decb = lambda: B.bfv_decrypt_dev(plan, 2, sb_ev.data_ptr(), ct.data_ptr(), pt.data_ptr(), BATCH)
        enc(); dec(); torch.cuda.synchronize()
        noise = int((pt - msg).abs().max())
        assert noise < q // 8, noise
        te, td = timeit(enc, 0.3, 0.6, 3), timeit(dec, 0.3, 0.6, 3)
        kern = kernel_ms(enc)
        tbe, tbd = timeit(encb, 0.3, 0.6, 3), timeit(decb, 0.3, 0.6, 3)
        res[f"n{n}" if q == 65537 else f"n{n}_q61"] = {
            "fhe_ckks_encrypt_dev_ms": te * 1e3, "encrypt_ct_per_s": BATCH / te, "fhe_ckks_decrypt_dev_ms": td * 1e3, "decrypt_ct_per_s": BATCH / td,
            "fhe_bfv_encrypt_dev_ms": tbe * 1e3, "fhe_bfv_decrypt_dev_ms": tbd * 1e3, "encrypt_kernels_ms": kern, "worst_noise": noise}
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_client_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
