#!/usr/bin/env python3
"""tools/ckks_eval_rate.py — the cost of the CKKS evaluator on an RNS chain on one GPU:
  - fhe_ckks_rns_mul_dev and fhe_ckks_rns_rescale_dev at n = 4096 and 8192, k = 3 limbs of the (58, 40) test chain, batch
    1024, milliseconds per call and ciphertexts/s, with the library's per-kernel timer;
  - for each element-wise kernel of ckks_eval.hip the bytes its definition moves per call and the achieved TB/s
    (tensor: 4 reads and 3 writes an element; lift: 1 read and a write per target; keymac: k reads and 2 writes, the key
    rows left out; divround: 3 reads (2 in a rescale) and 1 write);
  - in the same process the same two operations composed only from entry points older than ckks_eval.hip:
    fhe_rq_pointwise_mul_dev, fhe_rq_add_dev, fhe_rq_sub_dev, fhe_rq_mul_by_u64_dev, the transforms, and a lift on the HOST
    (download, numpy, upload).  Its result is compared word for word with the new path's before anything is timed, and its
    time is reported with and without the host lifts;
  - what was not measured.
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_eval_rate.py [tag]  ->  profiles/<tag>_ckks_eval_rate.json"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fhe_study_amd as pkg

import _ckks_eval_numpy as E
from _timing import timeit                           # warm clocks: tools/_timing.py

B = pkg.binding
BATCH, K = 1024, 3
I64 = torch.int64


def rand_ct(mods, comps, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.stack([torch.randint(0, q, (comps, BATCH, n), dtype=I64, device="cuda", generator=g) for q in mods])


def kernel_ms(f, reps=5):
    B.kernel_timing_enable(True)
    B.kernel_timing_reset()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    out = {k: (v[0] / reps, v[1] / reps) for k, v in B.kernel_timing_read(256).items()}
    B.kernel_timing_enable(False)
    return out


def moved_bytes(n, k, op):
    """bytes per call that each kernel's definition moves (8-byte words), over all chunks: the counts do not depend on the chunking"""
    w = 8 * BATCH * n
    if op == "mul":
        lift = sum(1 + k for _ in range(k)) + 2 * (1 + k)                      # k digit lifts to k targets each, t_P (two slabs) to k
        return {"ckks_rns_tensor": 7 * k * w, "ckks_rns_lift": lift * w, "ckks_rns_keymac": (k + 1) * (k + 2) * w, "ckks_rns_divround": k * 2 * 4 * w}
    return {"ckks_rns_lift": 2 * (1 + (k - 1)) * w, "ckks_rns_divround": (k - 1) * 2 * 3 * w}


class Composed:
    """ct x ct with relinearisation, and the rescale, from the older entry points; every buffer allocated once"""

    def __init__(self, mods, P, n, rlk):
        self.mods, self.P, self.n, self.k = mods, P, n, len(mods)
        self.plans = [pkg.Plan(q, n) for q in mods] + [pkg.Plan(P, n)]
        self.L = B.load_library()
        k, e = self.k, lambda *s: torch.empty(s, dtype=I64, device="cuda")
        self.d, self.tmp = e(k, 3, BATCH, n), e(2, BATCH, n)
        self.coef = e(k, BATCH, n)
        self.dig = e(k + 1, k, BATCH, n)                                        # digit j under target i, in evals
        self.t, self.tp, self.e2 = e(k + 1, 2, BATCH, n), e(2, BATCH, n), e(k, 2, BATCH, n)
        # the key rows broadcast over the batch once: fhe_rq_pointwise_mul_dev multiplies row by row
        self.key = rlk[:k][:, list(range(k)) + [rlk.shape[1] - 1]].unsqueeze(3).expand(k, k + 1, 2, BATCH, n).contiguous()
        self.host_s = 0.0

    def pw(self, i, a, b, c, rows=BATCH):
        self.plans[i].pointwise_mul_dev(a.data_ptr(), b.data_ptr(), c.data_ptr(), rows)

    def ew(self, fn, i, a, b, c, rows=BATCH):
        B._check(fn(self.plans[i].handle, a.data_ptr(), b.data_ptr(), c.data_ptr(), rows, None))

    def host_lift(self, src, qj, targets, dsts):
        """the lift of §22 on the host: download, numpy, upload"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = src.cpu().numpy().view(np.uint64)
        for q, dst in zip(targets, dsts):
            dst.copy_(torch.from_numpy(E.lift(x, qj, q).view(np.int64)))
        torch.cuda.synchronize()
        self.host_s += time.perf_counter() - t0

    def divround(self, x, top, top_i, out, add=None):
        """out_i = (x_i - lift(top)) top_q^-1 (+ add_i) per limb i; top [2][BATCH][n] evals under plan top_i"""
        k = out.shape[0]
        top_q = (self.mods + [self.P])[top_i]
        self.plans[top_i].inverse_dev(top.data_ptr(), self.tp.data_ptr(), 2 * BATCH)
        self.host_lift(self.tp, top_q, self.mods[:k], [self.e2[i] for i in range(k)])
        for i in range(k):
            self.plans[i].forward_dev(self.e2[i].data_ptr(), self.e2[i].data_ptr(), 2 * BATCH)
            self.ew(self.L.fhe_rq_sub_dev, i, x[i], self.e2[i], self.tmp, 2 * BATCH)
            dst = out[i] if add is None else self.tmp
            B._check(self.L.fhe_rq_mul_by_u64_dev(self.plans[i].handle, self.tmp.data_ptr(), pow(top_q, -1, self.mods[i]), dst.data_ptr(), 2 * BATCH, None))
            if add is not None:
                self.ew(self.L.fhe_rq_add_dev, i, self.tmp, add[i], out[i], 2 * BATCH)

    def mul(self, a, b, out):
        k, d = self.k, self.d
        for i in range(k):
            self.pw(i, a[i, 0], b[i, 0], d[i, 0])
            self.pw(i, a[i, 0], b[i, 1], d[i, 1])
            self.pw(i, a[i, 1], b[i, 0], self.tmp[0])
            self.ew(self.L.fhe_rq_add_dev, i, d[i, 1], self.tmp[0], d[i, 1])
            self.pw(i, a[i, 1], b[i, 1], d[i, 2])
            self.plans[i].inverse_dev(d[i, 2].data_ptr(), self.coef[i].data_ptr(), BATCH)
        allm = self.mods + [self.P]
        for j in range(k):
            tg = [i for i in range(k + 1) if i != j]
            self.host_lift(self.coef[j], self.mods[j], [allm[i] for i in tg], [self.dig[i, j] for i in tg])
        for i in range(k + 1):
            self.plans[i].forward_dev(self.dig[i].data_ptr(), self.dig[i].data_ptr(), k * BATCH)   # the own slot holds nothing yet:
            if i < k:
                self.dig[i, i].copy_(d[i, 2])                                  # limb i keeps its evals
            for c in range(2):
                self.pw(i, self.dig[i, 0], self.key[0, i, c], self.t[i, c])
                for j in range(1, k):
                    self.pw(i, self.dig[i, j], self.key[j, i, c], self.tmp[0])
                    self.ew(self.L.fhe_rq_add_dev, i, self.t[i, c], self.tmp[0], self.t[i, c])
        self.divround(self.t, self.t[k], k, out, add=d[:, :2])

    def rescale(self, c, out):
        self.divround(c, c[self.k - 1], self.k - 1, out)


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"shape": {"batch": BATCH, "limbs": K, "chain": "(58, 40)"}, "not_measured": [
        "chunk sizes other than 2^21 / (n k^2)", "k other than 3", "batches other than 1024", "hardware counters (the TB/s are bytes by definition over the kernel timer's time)"]}
    tab = pkg.tfhe.cdt_table(3.2)
    d_tab = torch.from_numpy(np.ascontiguousarray(tab).view(np.int64)).cuda()
    seed = bytes(range(32))
    for n in (4096, 8192):
        mods, P = E.chain(n, 58, 40, K - 1)
        plans, sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
        d_s = torch.empty((K + 1, n), dtype=I64, device="cuda")
        for i, p in enumerate(plans + [sp]):
            B.ckks_secret_key_dev(p, seed, 0, d_s[i].data_ptr())
        rlk = torch.empty((K, K + 1, 2, n), dtype=I64, device="cuda")
        B.ckks_rns_relin_key_dev(plans, sp, seed, E.RLK_BASE, d_s.data_ptr(), d_tab.data_ptr(), len(tab), rlk.data_ptr())
        a, b = rand_ct(mods, 2, n, 1), rand_ct(mods, 2, n, 2)
        out, low = torch.empty_like(a), torch.empty((K - 1, 2, BATCH, n), dtype=I64, device="cuda")
        ref, ref_low = torch.empty_like(out), torch.empty_like(low)
        new_mul = lambda: B.ckks_rns_mul_dev(plans, sp, rlk.data_ptr(), K, a.data_ptr(), b.data_ptr(), out.data_ptr(), BATCH)
        new_res = lambda: B.ckks_rns_rescale_dev(plans, out.data_ptr(), low.data_ptr(), BATCH)
        comp = Composed(mods, P, n, rlk)
        new_mul(); new_res(); comp.mul(a, b, ref); comp.rescale(ref, ref_low)
        torch.cuda.synchronize()
        assert torch.equal(out, ref) and torch.equal(low, ref_low), "the composition and the new path differ"
        row = {}
        for op, f_new, f_old in (("mul", new_mul, lambda: comp.mul(a, b, ref)), ("rescale", new_res, lambda: comp.rescale(ref, ref_low))):
            t_new = timeit(f_new, 0.3, 0.6, 3)
            kern = kernel_ms(f_new)
            comp.host_s, reps = 0.0, 2
            f_old(); torch.cuda.synchronize()
            comp.host_s = 0.0
            t0 = time.perf_counter()
            for _ in range(reps):
                f_old()
            torch.cuda.synchronize()
            t_old, t_host = (time.perf_counter() - t0) / reps, comp.host_s / reps
            moved = moved_bytes(n, K, op)
            kernels = {}
            for name, (ms, launches) in kern.items():
                kernels[name] = {"ms_per_call": ms, "launches_per_call": launches}
                for lab, byts in moved.items():
                    if name.startswith(lab):
                        kernels[name].update(bytes_per_call=byts, tb_per_s=byts / (ms * 1e-3) / 1e12)
            own = sum(v["ms_per_call"] for kname, v in kernels.items() if kname.startswith("ckks_rns_"))
            row[op] = {"new_ms": t_new * 1e3, "new_ct_per_s": BATCH / t_new, "composed_ms": t_old * 1e3, "composed_host_lift_ms": t_host * 1e3,
                       "composed_device_part_ms": (t_old - t_host) * 1e3, "composed_over_new": t_old / t_new,
                       "composed_device_part_over_new": (t_old - t_host) / t_new, "kernel_timer_total_ms": sum(v["ms_per_call"] for v in kernels.values()),
                       "kernel_timer_own_kernels_ms": own, "kernels": kernels, "chunk_rows": E.chunk_rows(n, K, BATCH, rescale=(op == "rescale"))}
        res[f"n{n}"] = row
        del comp, a, b, out, low, ref, ref_low
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_eval_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
