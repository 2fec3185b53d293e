#!/usr/bin/env python3
"""tools/ckks_deep_rate.py — the cost of the deep CKKS chain on one GPU, milliseconds per call:
  (a) alpha = 1, 3 limbs, n = 4096, batch 1024: fhe_ckks_deep_mul_dev beside fhe_ckks_rns_mul_dev, and
      fhe_ckks_deep_diag_sum_dev at 8 and 32 rotations beside fhe_ckks_rns_diag_sum_dev, on the same words;
  (b) n = 2^15, 24 limbs, alpha in {1, 3, 4, 8}, a batch of four chunks: ct x ct, one rotation, and the diagonal sum over 8 and 32
      rotations beside the same sum composed from fhe_ckks_deep_galois_dev with all keys (one digit decomposition, a
      modulus-down per rotation), pointwise_mul_dev per limb and component, and fhe_rq_add_dev.
Keys, plaintexts and ciphertexts are canonical random words: the cost does not depend on the keys being keys.  A measurement
keeps the chip under back-to-back calls for at least 150 ms, then takes the median of seven timed, synchronised calls.
Diagnostic only (the contract bench is bench.py).
Usage: tools/ckks_deep_rate.py [tag [commit]]  ->  profiles/<tag>_ckks_deep_rate.json"""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import fhe_study_amd as pkg

import _ckks_deep_numpy as D
import _ckks_eval_numpy as E

B = pkg.binding
I64 = torch.int64
COUNTS = (8, 32)
WORD = 1 << 39                                       # every prime of these chains is above 2^39: words below it are canonical


def median_ms(f, warm_s=0.15, samples=7):
    t0 = time.perf_counter()
    n = 1
    while True:
        for _ in range(n): f()
        torch.cuda.synchronize()
        n *= 2
        if time.perf_counter() - t0 >= warm_s:
            break
    ts = []
    for _ in range(samples):
        t1 = time.perf_counter(); f(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t1) * 1e3)
    return statistics.median(ts)


def words(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, WORD, shape, dtype=I64, device="cuda", generator=g)


def commit_of(argv):
    if len(argv) > 2:
        return argv[2]
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return "unknown"


def deep_rows(n, L, alpha, batch, compose):
    """mul, one rotation and the diagonal sums of one deep chain -> dict"""
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = [pkg.Plan(q, n) for q in mods], [pkg.Plan(p, n) for p in sps]
    ng, top = D.dnum(L, alpha), max(COUNTS)
    keys = [words((ng, L + alpha, 2, n), 100 + t) for t in range(top)]
    ptrs = [x.data_ptr() for x in keys]
    gs = [pow(5, t + 1, 2 * n) for t in range(top)]
    pts = words((top, L + alpha, n), 7)
    a, b = words((L, 2, batch, n), 1), words((L, 2, batch, n), 2)
    out = torch.empty((1, L, 2, batch, n), dtype=I64, device="cuda")
    lib = B.load_library()
    row = {"limbs": L, "alpha": alpha, "dnum": ng, "batch": batch, "chunk_rows_mul": D.chunk_rows(n, L, alpha, batch),
           "workspace_bytes_mul": B.ckks_deep_workspace_bytes(n, L, alpha, batch), "key_bytes": ng * (L + alpha) * 2 * n * 8}
    row["mul_ms"] = median_ms(lambda: B.ckks_deep_mul_dev(plans, sp, ptrs[0], L, a.data_ptr(), b.data_ptr(), out.data_ptr(), batch))
    row["rotate_ms"] = median_ms(lambda: B.ckks_deep_galois_dev(plans, sp, ptrs[:1], gs[:1], L, a.data_ptr(), out.data_ptr(), batch))
    for count in COUNTS:
        pt = pts[:count].contiguous()
        r = {"workspace_bytes": B.ckks_deep_diag_workspace_bytes(n, L, alpha, batch, count, 1)}
        r["diag_sum_ms"] = median_ms(lambda: B.ckks_deep_diag_sum_dev(plans, sp, ptrs[:count], gs[:count], L, pt.data_ptr(), 1, a.data_ptr(), out.data_ptr(), batch))
        if compose:
            rots = torch.empty((count, L, 2, batch, n), dtype=I64, device="cuda")
            prod, acc = torch.empty_like(a), torch.empty_like(a)
            ptb = pt[:, :L, None, :].expand(count, L, batch, n).contiguous()     # mul_plain's operand: the plaintext per row of the batch

            def composed():
                B.ckks_deep_galois_dev(plans, sp, ptrs[:count], gs[:count], L, a.data_ptr(), rots.data_ptr(), batch)
                for t in range(count):
                    dst = acc if t == 0 else prod
                    for i, p in enumerate(plans):
                        for c in range(2):
                            p.pointwise_mul_dev(rots[t, i, c].data_ptr(), ptb[t, i].data_ptr(), dst[i, c].data_ptr(), batch)
                    if t:
                        for i, p in enumerate(plans):
                            B._check(lib.fhe_rq_add_dev(p.handle, acc[i].data_ptr(), prod[i].data_ptr(), acc[i].data_ptr(), 2 * batch, None))
            r["composed_ms"] = median_ms(composed)
            r["composed_over_diag_sum"] = r["composed_ms"] / r["diag_sum_ms"]
            # the rotations alone: what the composition costs whatever the products and sums are made with (they are 3 count limbs
            # small launches here, bound by the host at a batch this small)
            r["rotations_alone_ms"] = median_ms(lambda: B.ckks_deep_galois_dev(plans, sp, ptrs[:count], gs[:count], L, a.data_ptr(), rots.data_ptr(), batch))
            r["rotations_alone_over_diag_sum"] = r["rotations_alone_ms"] / r["diag_sum_ms"]
            r["modulus_downs"] = {"diag_sum": 1, "composed": count}
            del rots, prod, acc, ptb
        row[f"count_{count}"] = r
    return row, (plans, sp, keys, pts, a, b)


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    res = {"machine": torch.cuda.get_device_name(0), "commit": commit_of(sys.argv), "torch": torch.__version__, "hip": torch.version.hip,
           "method": "150 ms of back-to-back calls, then the median of 7 timed, synchronised calls; milliseconds per call",
           "not_measured": ["outputs other than 1", "real keys (random canonical words serve: no branch depends on them)", "batches other than the ones listed",
                            "n other than 4096 and 2^15", "limbs other than 3 and 24", "hardware counters", "the decrypted agreement of the fused and composed sums "
                            "(tests/test_ckks_deep_linear_cpu.py bounds their difference in the restatement)"]}
    # (a) alpha = 1, 3 limbs, n = 4096, batch 1024: the deep entry points beside §22's and §24's on the same words
    n, L, batch = 4096, 3, 1024
    row, (plans, sp, keys, pts, a, b) = deep_rows(n, L, 1, batch, False)
    out = torch.empty((1, L, 2, batch, n), dtype=I64, device="cuda")
    ptrs = [x.data_ptr() for x in keys]
    gs = [pow(5, t + 1, 2 * n) for t in range(max(COUNTS))]
    row["rns_mul_ms"] = median_ms(lambda: B.ckks_rns_mul_dev(plans, sp[0], ptrs[0], L, a.data_ptr(), b.data_ptr(), out.data_ptr(), batch))
    row["deep_over_rns_mul"] = row["mul_ms"] / row["rns_mul_ms"]
    for count in COUNTS:
        pt = pts[:count].contiguous()
        r = row[f"count_{count}"]
        r["rns_diag_sum_ms"] = median_ms(lambda: B.ckks_rns_diag_sum_dev(plans, sp[0], ptrs[:count], gs[:count], L, pt.data_ptr(), 1, a.data_ptr(), out.data_ptr(), batch))
        r["deep_over_rns_diag_sum"] = r["diag_sum_ms"] / r["rns_diag_sum_ms"]
    res["a_n4096_l3_alpha1"] = row
    del plans, sp, keys, pts, a, b, out
    torch.cuda.empty_cache()
    # (b) n = 2^15, 24 limbs: the fused sum beside the composition, per alpha
    n, L = 1 << 15, 24
    for alpha in (1, 3, 4, 8):
        batch = 4 * D.chunk_rows(n, L, alpha, 1 << 20)
        row, keep = deep_rows(n, L, alpha, batch, True)
        res[f"b_n32768_l24_alpha{alpha}"] = row
        print(json.dumps({f"alpha{alpha}": row}), flush=True)
        del keep
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_ckks_deep_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
