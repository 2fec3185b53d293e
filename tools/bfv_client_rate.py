#!/usr/bin/env python3
"""tools/bfv_client_rate.py — the cost of the BFV client side on the device on one GPU:
  - key generation at n = 8192, q = 65537, p = q^2: fhe_bfv_public_key_dev and fhe_bfv_relin_key_dev, beside the numpy
    restatement (tests/_bfv_client_numpy.py) with the library's own products as its multiplier (fhe_rq_mul modulo q,
    fhe_tn_mul and one reduction modulo pq; wall time, one run);
  - fhe_bfv_encrypt_dev and fhe_bfv_decrypt_dev at batch 4096 for n = 4096 and 8192 (q = 65537, and n = 4096 at the 61-bit
    headline modulus; t = 2, so that the round trip is exact and asserted: at t = 32 the fresh noise, about 3.2 n^(1/2), is
    a fifth of q / 2t and a few of the 2^24 coefficients fail to decrypt), beside the restatement with the library's
    products as its multiplier (a smaller batch, scaled);
  - both routes of fhe_bfv_encrypt_dev at every shape where both exist: the route the library takes by default and, with
    FHE_BFV_ENCRYPT_STAGED=0 / =1 (read per call), the pointwise route (one forward transform, bfv_pk_pointwise_kernel,
    two inverses) and the staged route (the key rows broadcast over a chunk, fhe_rq_mul_dev twice), each with the library's per-kernel timer, which says what the products cost inside the call;
  - the straightforward composition built here: fhe_rq_mul_dev twice against the key broadcast over the whole batch, u
    given and the epilogue left out (at the 61-bit modulus this is the only staged figure: the library has no staged route
    there).
Diagnostic only (the contract bench is bench.py).
Usage: tools/bfv_client_rate.py [tag]  ->  profiles/<tag>_bfv_client_rate.json"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fhe_study_amd as pkg
from fhe_study_amd import tfhe

import _bfv_client_numpy as BC
from _timing import timeit                           # warm clocks: tools/_timing.py

B = pkg.binding
Q, T, BATCH, NP_BATCH = 65537, 2, 4096, 16
SEED = bytes(range(32))
TAB = tfhe.cdt_table(3.2)


def wall(f):
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def lib_mul(batch, shared, q):
    """the restatement's multiplier on the library's products (host buffers), signed small operands as residues: fhe_rq_mul
    modulo the two primes, else (pq) fhe_tn_mul, whose signed words are the integer product while n q < 2^63, reduced once"""
    batch, shared = np.asarray(batch), np.asarray(shared)
    a = batch.reshape(-1, batch.shape[-1])
    n = a.shape[-1]
    if q not in (Q, pkg.Q61):                                 # pq: composite, no transform modulo it
        words = lambda x: x if x.dtype == np.uint64 else x.astype(np.int64).view(np.uint64)
        c = B.tn_mul(n, words(a), np.broadcast_to(words(shared), a.shape)).reshape(a.shape).view(np.int64)
        c = np.array([int(v) % q for v in c.reshape(-1)], dtype=np.uint64).reshape(a.shape)
    else:
        res = lambda x: x if x.dtype == np.uint64 else np.mod(x.astype(np.int64), q).astype(np.uint64)
        c = pkg.Plan(q, n).rq_mul(res(a), np.broadcast_to(res(shared), a.shape), want_evals=False)[0]
    return c[0] if batch.ndim == 1 else c


def kernel_ms(f, reps=20):
    """per-kernel milliseconds of one call of f (the library's timer serialises launches)"""
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
    d_tab, m = dev(TAB), len(TAB)
    res = {"shape": {"q": Q, "t": T, "batch": BATCH, "numpy_batch": NP_BATCH, "sigma": 3.2}}
    # ---- keys at n = 8192 -----------------------------------------------------------------------------------------------
    n, pq = 8192, Q ** 3
    plan = pkg.Plan(Q, n)
    s = torch.empty(n, dtype=torch.int64, device="cuda")
    B.bfv_secret_key_dev(n, SEED, 0, s.data_ptr())
    s_np = s.cpu().numpy().view(np.uint64)
    out = torch.empty((2, n), dtype=torch.int64, device="cuda")
    res["keys_n8192_ms"] = {
        "fhe_bfv_public_key_dev": timeit(lambda: B.bfv_public_key_dev(plan, SEED, 1, s.data_ptr(), d_tab.data_ptr(), m, out.data_ptr()), 0.2, 0.4, 3) * 1e3,
        "fhe_bfv_relin_key_dev": timeit(lambda: B.bfv_relin_key_dev(Q, n, pq, SEED, 2, s.data_ptr(), d_tab.data_ptr(), m, out.data_ptr()), 0.2, 0.4, 3) * 1e3,
        "numpy_public_key": wall(lambda: BC.public_key(SEED, 1, s_np, Q, TAB, mul=lib_mul)) * 1e3,
        "numpy_relin_key": wall(lambda: BC.relin_key(SEED, 2, s_np, Q, pq, TAB, mul=lib_mul)) * 1e3,
    }
    # ---- encryption and decryption at batch 4096 ------------------------------------------------------------------------------
    for q, n in ((65537, 4096), (65537, 8192), (pkg.Q61, 4096)):
        plan = pkg.Plan(q, n)
        s = torch.empty(n, dtype=torch.int64, device="cuda")
        B.bfv_secret_key_dev(n, SEED, 0, s.data_ptr())
        s_np = s.cpu().numpy().view(np.uint64)
        pk = torch.empty((2, n), dtype=torch.int64, device="cuda")
        pk_ev, s_ev = torch.empty_like(pk), torch.empty_like(s)
        B.bfv_public_key_dev(plan, SEED, 1, s.data_ptr(), d_tab.data_ptr(), m, pk.data_ptr())
        plan.forward_dev(pk.data_ptr(), pk_ev.data_ptr(), 2)
        plan.forward_dev(s.data_ptr(), s_ev.data_ptr(), 1)
        msg = dev(np.random.default_rng(n).integers(0, T, (BATCH, n), dtype=np.uint64))
        ct = torch.empty((2, BATCH, n), dtype=torch.int64, device="cuda")
        pt = torch.empty((BATCH, n), dtype=torch.int64, device="cuda")
        enc = lambda: B.bfv_encrypt_dev(plan, T, SEED, 0, pk_ev.data_ptr(), msg.data_ptr(), n, d_tab.data_ptr(), m, ct.data_ptr(), BATCH)
        dec = lambda: B.bfv_decrypt_dev(plan, T, s_ev.data_ptr(), ct.data_ptr(), pt.data_ptr(), BATCH)
        enc(); dec(); torch.cuda.synchronize()
        assert torch.equal(pt, msg), "decrypt(encrypt(m)) != m"
        # the staged composition: the key rows broadcast over the batch, two full products (u is transformed twice, the key
        # BATCH times); u is taken from a degenerate-key call so that its generation is not charged either
        one = dev(np.stack([np.ones(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]))
        u = torch.empty((2, BATCH, n), dtype=torch.int64, device="cuda")
        B.bfv_encrypt_dev(plan, T, SEED, 0, one.data_ptr(), None, 0, None, 0, u.data_ptr(), BATCH)
        staged0, staged1 = pk[0].expand(BATCH, n).contiguous(), pk[1].expand(BATCH, n).contiguous()
        p0, p1 = torch.empty_like(staged0), torch.empty_like(staged0)

        def staged():
            plan.rq_mul_dev(u[0].data_ptr(), staged0.data_ptr(), p0.data_ptr(), BATCH)
            plan.rq_mul_dev(u[0].data_ptr(), staged1.data_ptr(), p1.data_ptr(), BATCH)

        pk_np = pk.cpu().numpy().view(np.uint64)
        msg_np = msg[:NP_BATCH].cpu().numpy().view(np.uint64)
        ct_np = [None]

        def np_enc():
            ct_np[0] = BC.encrypt(SEED, 0, pk_np[0], pk_np[1], msg_np, NP_BATCH, q, T, TAB, mul=lib_mul)

        t_np_enc = wall(np_enc) * BATCH / NP_BATCH
        assert np.array_equal(ct_np[0][0], ct[0, :NP_BATCH].cpu().numpy().view(np.uint64))
        t_np_dec = wall(lambda: BC.decrypt(s_np, ct_np[0][0], ct_np[0][1], q, T, mul=lib_mul)) * BATCH / NP_BATCH
        d, st = (timeit(f, 0.3, 0.6, 3) for f in (dec, staged))
        routes = {}
        for name, env in (("default", None), ("pointwise", "0"), ("staged", "1")):
            if env is None:
                os.environ.pop("FHE_BFV_ENCRYPT_STAGED", None)
            else:
                os.environ["FHE_BFV_ENCRYPT_STAGED"] = env
            ct.zero_()
            ms = timeit(enc, 0.3, 0.6, 3) * 1e3
            kern = kernel_ms(enc)
            dec(); torch.cuda.synchronize()
            assert torch.equal(pt, msg), name
            prod = sum(v for k, v in kern.items() if not k.startswith(("bfv_ephemeral", "bfv_encrypt_epilogue")))
            routes[name] = {"encrypt_ms": ms, "ct_per_s": BATCH / (ms * 1e-3), "kernels_ms": kern, "products_in_call_ms": prod,
                            "route": "staged" if any(k.startswith("bfv_broadcast") for k in kern) else "pointwise"}
        os.environ.pop("FHE_BFV_ENCRYPT_STAGED", None)
        e = routes["default"]["encrypt_ms"] * 1e-3
        res[f"n{n}" if q == Q else f"n{n}_q61"] = {
            "fhe_bfv_encrypt_dev_ms": e * 1e3, "encrypt_ct_per_s": BATCH / e, "encrypt_routes": routes,
            "fhe_bfv_decrypt_dev_ms": d * 1e3, "decrypt_ct_per_s": BATCH / d,
            "composed_products_only_ms": st * 1e3,
            "numpy_encrypt_ms_scaled": t_np_enc * 1e3, "numpy_decrypt_ms_scaled": t_np_dec * 1e3,
        }
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_bfv_client_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
