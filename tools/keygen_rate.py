#!/usr/bin/env python3
"""tools/keygen_rate.py — the cost of making keys and ciphertexts on the device on one GPU, beside the numpy
generators of the tests on the same box: N = 1024, k = 1, n_lwe = 630, BSK (8, 3), KSK (4, 4), PKSK (8, 4), sigma = 3.2.
  - device: the raw samples of each key (fhe_tglwe_encrypt_dev / fhe_tlwe_encrypt_dev with the torch message builders), and
    the three keys as a user gets them (ClientKey.generate, bootstrapping_key with its BSK preparation, packing_key_switch_key);
  - numpy: tests/_gadget_numpy.tggsw_bits and ksk, tests/_pks_numpy.pksk with the library's fhe_tn_mul as their product, as the
    functional tests call them (wall time, one run each: they take seconds);
  - encryption of a batch of 4096 values: fhe_tlwe_encrypt_dev on device buffers, ClientKey.encrypt_int (host values in,
    host words out), and tests/_tfhe_numpy.lwe_encrypt.
Diagnostic only (the contract bench is bench.py).
Usage: tools/keygen_rate.py [tag]  ->  profiles/<tag>_keygen_rate.json"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fhe_study_amd as pkg
from fhe_study_amd import tfhe

import _gadget_numpy as G
import _lut_numpy as LN
import _pks_numpy as PK
import _tfhe_numpy as R
from _timing import timeit                           # warm clocks: tools/_timing.py

B = pkg.binding
N, NL, BSK, KSK, PKS, SIGMA, T, BATCH = 1024, 630, (8, 3), (4, 4), (8, 4), 3.2, 3, 4096
SEED = bytes(range(32))


def wall(f):
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "local"
    ck = tfhe.ClientKey.generate(SEED, N, NL, noise=(SIGMA, 0))
    first = ck.BSK_BASE
    bsk_rows, ksk_rows, pksk_rows = NL * 2 * BSK[1], N * KSK[1], NL * PKS[1]
    dev = {
        "bsk_samples": lambda: ck._tglwe_rows(first, tfhe.bsk_messages(ck.s_glwe, ck.s_lwe, *BSK), None),
        "ksk_samples": lambda: ck._tlwe_rows(first + bsk_rows, ck.s_lwe, tfhe.ksk_messages(ck.s_glwe, *KSK), None),
        "pksk_samples": lambda: ck._tglwe_rows(ck.PKSK_BASE, tfhe.pksk_messages(ck.s_lwe, N, *PKS), None),
    }

    def keys():
        c = tfhe.ClientKey.generate(SEED, N, NL, noise=(SIGMA, 0))
        return c.bootstrapping_key(BSK, KSK), c.packing_key_switch_key(PKS)

    res = {"shape": {"n": N, "n_lwe": NL, "bsk": BSK, "ksk": KSK, "pksk": PKS, "sigma": SIGMA, "log_scale": 0,
                     "rows": {"bsk": bsk_rows, "ksk": ksk_rows, "pksk": pksk_rows}, "encrypt_batch": BATCH}}
    res["device_ms"] = {k: timeit(f, 0.2, 0.4, 3) * 1e3 for k, f in dev.items()}
    res["device_ms"]["samples_total"] = sum(res["device_ms"].values())
    res["device_ms"]["keys_as_a_user_gets_them"] = timeit(keys, 0.2, 0.4, 3) * 1e3

    rng = np.random.default_rng(1)
    s_glwe, s_lwe = rng.integers(0, 2, N, dtype=np.uint64), rng.integers(0, 2, NL, dtype=np.uint64)
    mul = lambda a, x: B.tn_mul(N, a, np.ascontiguousarray(x))
    res["numpy_ms"] = {
        "bsk": wall(lambda: G.tggsw_bits(rng, mul, N, BSK[0], BSK[1], s_glwe, s_lwe, SIGMA)) * 1e3,
        "ksk": wall(lambda: G.ksk(rng, s_glwe, s_lwe, KSK[0], KSK[1], SIGMA)) * 1e3,
        "pksk": wall(lambda: PK.pksk(rng, mul, N, s_lwe, s_glwe, PKS[0], PKS[1], SIGMA)) * 1e3,
    }
    res["numpy_ms"]["total"] = sum(res["numpy_ms"].values())
    res["keys_numpy_over_device_samples"] = res["numpy_ms"]["total"] / res["device_ms"]["samples_total"]

    values = np.arange(BATCH) % (1 << T)
    mu = torch.from_numpy(tfhe.encode_int(values, T).view(np.int64)).cuda()
    d_cdt, m, log_scale = ck._noise(None)
    out = torch.empty((BATCH, NL + 1), dtype=torch.int64, device="cuda")
    enc = lambda: B.tlwe_encrypt_dev(NL, SEED, 0, ck.s_lwe.data_ptr(), mu.data_ptr(), d_cdt.data_ptr(), m, log_scale, out.data_ptr(), BATCH)
    res["encrypt_ms"] = {
        "fhe_tlwe_encrypt_dev": timeit(enc, 0.2, 0.4, 3) * 1e3,
        "ClientKey.encrypt_int": timeit(lambda: ck.encrypt_int(values, T), 0.2, 0.4, 3) * 1e3,
        "numpy_lwe_encrypt": wall(lambda: R.lwe_encrypt(rng, s_lwe, [LN.encode(v, T) for v in values], SIGMA)) * 1e3,
    }
    res["encrypt_gb_per_s_written"] = BATCH * (NL + 1) * 8 / (res["encrypt_ms"]["fhe_tlwe_encrypt_dev"] * 1e-3) / 1e9
    print(json.dumps(res), flush=True)
    os.makedirs("profiles", exist_ok=True)
    path = os.path.join("profiles", f"{tag}_keygen_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
