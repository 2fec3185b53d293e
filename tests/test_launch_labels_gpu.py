"""One call per launcher family of the transform engines (csrc/ntt_kernels.hip, ntt_kernels_q62.hip, smallq.hip, digit32.hip,
digit_mac.hip, bfv32.hip) at the smallest size the family accepts, with batch 1 and with batch 0, under the kernel timer.

The return code and the exact set of (label, tag, count) rows of fhe_ntt_kernel_timing_read are compared with
tests/golden/launch_labels.json, which was recorded with these same calls on the commit BEFORE the launchers were folded
onto csrc/launch.hpp: a renamed label, a dropped or doubled launch and a zero-batch path that starts
launching all show as a differing row.  Operands are zeros: which kernels run depends on the shapes alone."""
import json
import os

import pytest

from conftest import GOLDEN, Q16, Q61

pytestmark = pytest.mark.gpu

Q62 = 4611686018425815041      # the largest prime = 1 (mod 2^17) below 2^62 (tests/test_rq_rows_cpu.py)
Q63 = 9223372036844421121      # ... below 2^63
FIXTURE = os.path.join(GOLDEN, "launch_labels.json")
BATCHES = (1, 0)


def _buf(words):
    import torch

    return torch.zeros(max(int(words), 2), dtype=torch.int64, device="cuda")


def _plan_cases(pkg, name, q, n):
    """forward, inverse and product of one plan -> [(case name, call(batch) -> return code)]"""
    L = pkg.load_library()
    plan = pkg.Plan(q, n)
    a, b, c = _buf(n), _buf(n), _buf(n)
    work = _buf(plan.workspace_bytes(1) // 8)
    return [
        (f"{name}_forward", lambda batch: L.fhe_ntt_forward_dev(plan.handle, a.data_ptr(), c.data_ptr(), batch, None)),
        (f"{name}_inverse", lambda batch: L.fhe_ntt_inverse_dev(plan.handle, a.data_ptr(), c.data_ptr(), batch, None)),
        (f"{name}_rq_mul", lambda batch: L.fhe_rq_mul_dev(plan.handle, a.data_ptr(), 0, b.data_ptr(), 0, c.data_ptr(), None, None, None, batch,
                                                        work.data_ptr(), None)),
    ]


def cases(pkg):
    L = pkg.load_library()
    out = []
    for name, q, n in (("q61_n16", Q61, 16), ("q61_n16384", Q61, 1 << 14), ("q62_n16", Q62, 16), ("q63_n16", Q63, 16),
                       ("smallq_n256", Q16, 256), ("smallq_n8192", Q16, 1 << 13), ("smallq_n32768", Q16, 1 << 15)):
        out += _plan_cases(pkg, name, q, n)
    n, l = 256, 2
    # TGGSW x TGLWE, k = 1: the key transformed per call (ntt32_fwd_key), digit_mac32, digit_tail32
    tggsw, ct, res = _buf(2 * l * 2 * n), _buf(2 * n), _buf(2 * n)
    out.append(("ext32_external_product", lambda batch: L.fhe_tggsw_external_product_dev(n, 1, l, tggsw.data_ptr(), ct.data_ptr(), res.data_ptr(), batch, None)))
    # GLWE::key_switch, base 2: k = 1 on the two 27-bit primes, k = 2 on the 61-bit digit kernels (digit_mac_zq, digit_tail_ks)
    plan = pkg.Plan(Q61, n)
    for k in (1, 2):
        ksk, glwe, sw = _buf(k * 4 * (k + 1) * n), _buf((k + 1) * n), _buf((k + 1) * n)
        out.append((f"key_switch_k{k}", lambda batch, k=k, ksk=ksk, glwe=glwe, sw=sw: L.fhe_glwe_key_switch_dev(
            plan.handle, k, 2, 4, glwe.data_ptr(), ksk.data_ptr(), sw.data_ptr(), batch, 0, None)))
    # the gadget CMux with a selector per ciphertext: `batch` keys prepared (ntt32_fwd_key through gridDim.z), then the CMux itself
    b = 8
    w = L.fhe_tggsw_gadget_prepared_words(n, 1, b, l)
    raw, prep, idx, c0, c1, mux = _buf(w // 2), _buf(w), _buf(2), _buf(2 * n), _buf(2 * n), _buf(2 * n)
    out.append(("gadget_prepare_many", lambda count: L.fhe_tggsw_gadget_prepare_many_dev(n, 1, b, l, count, raw.data_ptr(), prep.data_ptr(), None)))
    out.append(("gadget_cmux", lambda batch: L.fhe_tggsw_gadget_cmux_dev(n, 1, b, l, 1, prep.data_ptr(), idx.data_ptr(), c0.data_ptr(), c1.data_ptr(),
                                                                        mux.data_ptr(), batch, None)))
    # BFV multiply on the two small primes (bfv32.hip) for both stages: the reference's own parameters at n = 1024
    nb = 1024
    rlk, ab, o = _buf(2 * nb), _buf(4 * nb), _buf(2 * nb)
    out.append(("bfv_mul_n1024", lambda batch: L.fhe_bfv_mul_dev(Q16, nb, 2, Q16 ** 3, rlk.data_ptr(), ab.data_ptr(), o.data_ptr(), batch, None)))
    return out


def collect(pkg):
    """{case: {batch: {"rc": return code, "rows": sorted [label, tag, count]}}} of every case at batch 1 and 0"""
    import torch

    B = pkg.binding
    got = {}
    B.kernel_timing_enable(True)
    try:
        for name, call in cases(pkg):
            got[name] = {}
            for batch in BATCHES:
                torch.cuda.synchronize()
                B.kernel_timing_reset()
                rc = call(batch)
                torch.cuda.synchronize()
                rows = []
                for key, (_, count) in B.kernel_timing_read(256).items():
                    label, tag = key.rsplit("_", 1)
                    rows.append([label, int(tag), count])
                got[name][str(batch)] = {"rc": rc, "rows": sorted(rows)}
    finally:
        B.kernel_timing_reset()
        B.kernel_timing_enable(False)
    return got


@pytest.fixture(scope="module")
def observed(pkg):
    assert pkg.binding.device_count() >= 1, "no HIP device: -m gpu tests need a real MI355X"
    return collect(pkg)


EXPECTED = {}
if os.path.exists(FIXTURE):
    with open(FIXTURE) as _f:
        EXPECTED = json.load(_f)


def test_the_fixture_names_every_case(observed):
    assert EXPECTED and sorted(observed) == sorted(EXPECTED)
    for rows in EXPECTED.values():
        assert sorted(rows) == ["0", "1"]


@pytest.mark.parametrize("name", sorted(EXPECTED))
@pytest.mark.parametrize("batch", BATCHES)
def test_return_code_and_timer_rows_match_the_recording(observed, name, batch):
    want, got = EXPECTED[name][str(batch)], observed[name][str(batch)]
    print(name, batch, got)
    assert got["rc"] == want["rc"]
    assert got["rows"] == want["rows"]
