"""The R_q row surfaces of csrc/glue.hip (rows N3 / N4 of include/fhe_ntt.h) at every launch class of
tests/test_rq_rows_cpu.py, word for word against a plain reference: tests/_rq_rows_numpy.py (Python integers, no NTT) for
n <= 256 and oracle.glue (products through the oracle's NTT) above.  Every check is exact equality of integer words; the
f64 rows are exact too, each step being one IEEE operation on both sides.

Key switch: each (q, n, k, beta, l) of KS_CASES builds a few distinct ciphertexts (one random with the edge words of
Zq::decompose planted, one of q - 1 throughout, the rest random), computes every reference once and tiles the rows into
each batch on the device, so every one of the `batch` output rows is compared (on the device, after the output was
poisoned).  Each batch runs with the key in coefficients, as evals (FHE_A_IS_EVALS) and prepared; the batches of one shape
run descending then ascending on one stream, so workspace slot 1 is reused under a smaller, then a larger `parts`; the
first shape of every n runs on a stream of its own; the kernel timer's names must show the route the restatement predicts.

Distinct rows: 6 while n l <= 8192, 2 beyond.  Measured on an MI355X box: the key-switch sweep takes 0.1 - 0.6 s per n
(1.8 s at n = 256 and 1.2 s at 2^14, nearly all of it the host reference; 12 s for whichever test runs first, which loads
the library and the device), the mac_rows sweep 0.1 s at n <= 16, 1.9 s at 256, 1.3 s at 4096, 2.7 s at 2^13 and 5.1 s at
2^14, the three child processes 6 s; 39 s for the whole module (TIMES below)."""
import hashlib
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _rq_rows_numpy as P
import test_rq_rows_cpu as S
from conftest import Q16, Q61, ROOT
from test_crt_bounds import _has, _ran
from test_gadget_shapes_gpu import _ladder, _tile

pytestmark = pytest.mark.gpu

ROWS_CUT = 8192
POISON = 0x5A5A5A5A5A5A5A5A
PY_REF_MAX_N = 256               # the Python reference up to here, the oracle above
_POOL = ThreadPoolExecutor(8)    # ctypes releases the interpreter lock: oracle references run side by side


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(pkg):
    assert pkg.binding.device_count() >= 1, "no HIP device: -m gpu tests need a real MI355X"


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64).copy()).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _arr(x):
    return np.array(x, dtype=np.uint64)


def _rand(rng, q, shape):
    return rng.integers(0, q, shape, dtype=np.uint64)


def _edges(q, beta, l):
    """the words where Zq::decompose changes branch, kept canonical"""
    w = [0, 1, 2, q - 1, q // 2, (1 << min(l, 63)) - 1, 1 << min(l, 63), (1 << min(l, 63)) + 1, beta ** l - 1, beta ** l, beta ** l + 1]
    return [x for x in w if 0 <= x < q]


# ---- references ----------------------------------------------------------------------------------------------------------------

def ref_key_switch(oracle, q, n, k, beta, l, glwe, ksk):
    if n <= PY_REF_MAX_N:
        return _arr(P.key_switch(q, k, beta, l, glwe, ksk))
    out = np.empty((k + 1, n), dtype=np.uint64)
    oracle.glue("key_switch", q, n, k, beta, l, np.ascontiguousarray(glwe), ksk, out)
    return out


def ref_tr_dot(oracle, q, n, a, b):
    if n <= PY_REF_MAX_N:
        return _arr(P.tr_dot(q, a, b))
    out = np.empty(n, dtype=np.uint64)
    oracle.glue("tr_dot", q, n, len(a), np.ascontiguousarray(a), np.ascontiguousarray(b), out)
    return out


def ref_tr_mul_r(oracle, q, n, a, p):
    if n <= PY_REF_MAX_N:
        return _arr(P.tr_mul_r(q, a, p))
    out = np.empty((len(a), n), dtype=np.uint64)
    oracle.glue("tr_mul_r", q, n, len(a), np.ascontiguousarray(a), np.ascontiguousarray(p), out)
    return out


def ref_glev_mul(oracle, q, n, glev, v):
    if n <= PY_REF_MAX_N:
        return _arr(P.glev_mul(q, glev, v))
    l, k1 = glev.shape[0], glev.shape[1]
    out = np.empty((k1, n), dtype=np.uint64)
    oracle.glue("glev_mul", q, n, k1 - 1, l, np.ascontiguousarray(glev), np.ascontiguousarray(v), out)
    return out


def ref_decompose(oracle, q, n, a, beta, l):
    if n <= PY_REF_MAX_N:
        return _arr(P.rq_decompose(q, a, beta, l))
    out = np.empty((l, n), dtype=np.uint64)
    oracle.glue("rq_decompose", q, n, np.ascontiguousarray(a), beta, l, out)
    return out


def _each(fn, items):
    return [j.result() for j in [_POOL.submit(fn, x) for x in items]]


# ---- key switch ------------------------------------------------------------------------------------------------------------------

def route_names(route, lg):
    """the kernel-timer names (KernelTimer calls of csrc/: name_tag) a route must show, and those it must not"""
    if route == "ks32":
        return ["digit_mac32_%d" % lg, "digit_tail32_ks_%d" % lg], ["mac_rows", "digit_mac_zq", "ks_tail", "decompose"]
    if route == "fused61":
        return ["digit_mac_zq_%d" % lg, "digit_tail_ks_%d" % lg], ["mac_rows", "digit_mac32", "ks_tail", "decompose", "sum_parts"]
    _, dec, tail = route.split("-")
    must = ["mac_rows", "ntt_fwd_zqbits_%d" % lg if dec == "zqbits" else "decompose", "digit_tail_ks_%d" % lg if tail == "tail" else "ks_tail"]
    never = ["digit_mac32", "digit_mac_zq", "decompose" if dec == "zqbits" else "ntt_fwd_zqbits", "ks_tail" if tail == "tail" else "digit_tail_ks"]
    return must, never


class _KsGroup:
    def __init__(self, pkg, oracle, q, n, k, beta, l, st, worst=False):
        import torch

        L, B = pkg.load_library(), pkg.binding
        self.L, self.B, self.q, self.n, self.k, self.beta, self.l = L, B, q, n, k, beta, l
        self.plan = plan = pkg.Plan(q, n)
        d = self.d = 1 if worst else 6 if n * l <= ROWS_CUT else 2
        rng = np.random.default_rng((q % 1000003) * 31 + n * 7 + k * 1009 + beta * 101 + l)
        if worst:
            rows = np.full((1, k + 1, n), q - 1, dtype=np.uint64)
            ksk = np.full((k, l, k + 1, n), q - 1, dtype=np.uint64)
        else:
            rows = _rand(rng, q, (d, k + 1, n))
            e = _edges(q, beta, l)
            flat = rows[0].reshape(-1)
            m = min(len(e), flat.size)
            flat[:m] = e[:m]
            rows[0, k - 1, n - min(n, len(e)):] = e[:min(n, len(e))][::-1]
            rows[1] = q - 1
            ksk = _rand(rng, q, (k, l, k + 1, n))
            ksk[0, 0, 0, : min(n, 2)] = q - 1
        want = np.stack(_each(lambda r: ref_key_switch(oracle, q, n, k, beta, l, r, ksk), list(rows)))
        if worst and beta == 2 and l == 64:
            assert want[0].tolist() == S.ks_worst_closed(q, n, k, l)
        self.rows, self.want = _dev(rows), _dev(want)
        rows_ks = k * l * (k + 1)
        self.ksk = _dev(ksk)
        self.KSK = torch.empty_like(self.ksk)
        plan.forward_dev(self.ksk.data_ptr(), self.KSK.data_ptr(), rows_ks, st)
        words = L.fhe_glwe_ksk_prepared_words(plan.handle, k, beta, l)
        assert words == S.prepared_words(q, n, k, beta, l)
        self.prep = torch.empty(words, dtype=torch.int64, device="cuda")
        self.prep.fill_(POISON)
        src = self.ksk.clone()
        B._check(L.fhe_glwe_ksk_prepare_dev(plan.handle, k, beta, l, src.data_ptr(), self.prep.data_ptr(), st))
        src.zero_()                                                       # the prepared key stands alone

    def call(self, key, ct, out, batch, st):
        L, B, p = self.L, self.B, self.plan.handle
        if key == "coeffs":
            B._check(L.fhe_glwe_key_switch_dev(p, self.k, self.beta, self.l, ct.data_ptr(), self.ksk.data_ptr(), out.data_ptr(), batch, 0, st))
        elif key == "evals":
            B._check(L.fhe_glwe_key_switch_dev(p, self.k, self.beta, self.l, ct.data_ptr(), self.KSK.data_ptr(), out.data_ptr(), batch,
                                               B.FHE_A_IS_EVALS, st))
        else:
            B._check(L.fhe_glwe_key_switch_prepared_dev(p, self.k, self.beta, self.l, ct.data_ptr(), self.prep.data_ptr(), out.data_ptr(), batch, st))

    def shape(self, batch, key):
        return S.ks_shape(self.q, self.n, self.k, self.beta, self.l, batch, key)

    def run(self, batch, st, bad, names_bad=None):
        import torch

        idx = torch.from_numpy(_tile(batch, self.d)).cuda()
        ct, want = self.rows[idx], self.want[idx]
        out = torch.empty_like(ct)
        for key in S.KEYS:
            out.fill_(POISON)
            if names_bad is None:
                self.call(key, ct, out, batch, st)
            else:                                                          # under the kernel timer: the route that ran
                names = _ran(self.B, lambda: self.call(key, ct, out, batch, st))
                s = self.shape(batch, key)
                must, never = route_names(s["route"], self.n.bit_length() - 1)
                word32 = S.arithmetic(self.q, self.n) == S.WORD32
                if word32 and key == "coeffs" and s["route"] != "ks32":
                    must = must + ["sq_forward"]                           # fwd() of glue.hip:152-162 took the 32-bit transform
                if any(not _has(names, m) for m in must) or any(_has(names, x) for x in never):
                    names_bad.append((self.q, self.n, self.k, self.beta, self.l, batch, key, s["route"], sorted(names)))
            eq = (out == want).reshape(batch, -1).all(dim=1)
            if not bool(eq.all()):
                r = torch.nonzero(~eq).reshape(-1)
                bad.append((self.q, self.n, self.k, self.beta, self.l, batch, key, int(r.numel()), int(r[0]), self.shape(batch, key)))


# measured wall seconds per parametrised test on an MI355X box, rounded up (first call included; nearly all of it is the
# host reference).  pytest.mark.timeout is twice that, with a floor of 120 s
TIMES = {"ks": {2: 12, 16: 1, 256: 2, 512: 1, 1024: 1, 2048: 1, 4096: 1, 8192: 1, 16384: 2},
         "mac": {2: 1, 16: 1, 256: 2, 4096: 2, 8192: 3, 16384: 6},
         # the single tests, the slowest case of each: all below a second but the three child processes
         "one": {"grid_stride": 1, "worst": 1, "decompose": 1, "f64": 1, "elementwise": 1, "host": 1, "children": 7}}


def _timeout(kind, n):
    return pytest.mark.timeout(max(120, 2 * TIMES[kind][n]))


@pytest.mark.parametrize("n", [pytest.param(n, marks=_timeout("ks", n)) for n in S.SIZES])
def test_key_switch_sweep(pkg, oracle, n):
    import torch

    groups = {}
    for q, nn, k, beta, l, batch in S.KS_CASES:
        if nn == n:
            groups.setdefault((q, k, beta, l), []).append(batch)
    bad, names_bad = [], []
    t_ref, t0, rows = 0.0, time.time(), 0
    for i, ((q, k, beta, l), batches) in enumerate(groups.items()):
        side = torch.cuda.Stream() if i == 0 else None                    # the first shape on a stream of its own
        st = side.cuda_stream if side else None
        with torch.cuda.stream(side):
            t = time.time()
            g = _KsGroup(pkg, oracle, q, n, k, beta, l, st)
            t_ref += time.time() - t
            order = _ladder(batches)
            rows += sum(order)
            for j, batch in enumerate(order):
                g.run(batch, st, bad, names_bad if j == 0 or j == len(order) - 1 else None)
        torch.cuda.synchronize()
        if side:
            pkg.binding._check(pkg.load_library().fhe_ntt_release_stream_workspace(side.cuda_stream))
        del g
    print("\nkey switch, n = %d: %d shapes, %d cases, %d batch rows through each of 3 key forms, references %.1f s, all %.1f s"
          % (n, len(groups), sum(len(b) for b in groups.values()), rows, t_ref, time.time() - t0))
    for row in names_bad:
        print("ROUTE q=%d n=%d k=%d beta=%d l=%d batch=%d key=%s: predicted %s, ran %s" % row)
    for row in bad:
        print("MISMATCH q=%d n=%d k=%d beta=%d l=%d batch=%d key=%s: %d rows, first %d, %s" % row)
    assert not bad, "%d of the calls gave wrong words; the first: %r" % (len(bad), bad[0])
    assert not names_bad, "%d calls ran another route than the restatement predicts; the first: %r" % (len(names_bad), names_bad[0])


# ---- the mac_rows surfaces: every flag combination ----------------------------------------------------------------------------------

def _mac_rows(rng, q, shape):
    """[d, ...]: row 0 random with edge words, row 1 of q - 1 throughout, the rest random"""
    a = _rand(rng, q, shape)
    flat = a[0].reshape(-1)
    e = [0, 1, q - 1, q // 2, q - 2][: flat.size]
    flat[: len(e)] = e
    if shape[0] > 1:
        a[1] = q - 1
    return a


def _mac_case(pkg, oracle, q, n, entry, T, nc, bad, batch=5, d=3):
    import torch

    L, B = pkg.load_library(), pkg.binding
    plan = pkg.Plan(q, n)
    rng = np.random.default_rng((q % 1000003) + n * 13 + T * 7 + nc)
    t_ref = time.time()
    ntt = lambda x: oracle.ntt(q, n, np.ascontiguousarray(x).reshape(-1, n)).reshape(x.shape)
    if entry == "tr_dot":
        a, b = _mac_rows(rng, q, (d, T, n)), _mac_rows(rng, q, (d, T, n))
        want = np.stack(_each(lambda i: ref_tr_dot(oracle, q, n, a[i], b[i]), range(d)))
    elif entry == "tr_mul_r":
        a, b = _mac_rows(rng, q, (d, nc, n)), _mac_rows(rng, q, (d, n))
        want = np.stack(_each(lambda i: ref_tr_mul_r(oracle, q, n, a[i], b[i]), range(d)))
    else:
        a, b = _mac_rows(rng, q, (1, T, nc, n))[0], _mac_rows(rng, q, (d, T, n))      # the key is shared by the batch
        want = np.stack(_each(lambda i: ref_glev_mul(oracle, q, n, a, b[i]), range(d)))
    idx = torch.from_numpy(_tile(batch, d)).cuda()
    shared = entry == "glev_mul"
    hosts = (ntt(a), ntt(b), ntt(want))                                    # the oracle's transforms are reference work too
    t_ref = time.time() - t_ref
    dw = {0: _dev(want)[idx], 1: _dev(hosts[2])[idx]}
    da = {0: _dev(a) if shared else _dev(a)[idx].contiguous(), 1: _dev(hosts[0]) if shared else _dev(hosts[0])[idx].contiguous()}
    db = {0: _dev(b)[idx].contiguous(), 1: _dev(hosts[1])[idx].contiguous()}
    out = torch.empty_like(dw[0])
    for flags in range(8):
        A, Bv, W = da[flags & 1], db[(flags >> 1) & 1], dw[(flags >> 2) & 1]
        out.fill_(POISON)
        if entry == "tr_dot":
            B._check(L.fhe_tr_dot_dev(plan.handle, A.data_ptr(), Bv.data_ptr(), out.data_ptr(), T, batch, flags, None))
        elif entry == "tr_mul_r":
            B._check(L.fhe_tr_mul_r_dev(plan.handle, A.data_ptr(), Bv.data_ptr(), out.data_ptr(), nc, batch, flags, None))
        else:
            B._check(L.fhe_glev_mul_dev(plan.handle, nc - 1, T, A.data_ptr(), Bv.data_ptr(), out.data_ptr(), batch, flags, None))
        eq = (out == W).reshape(batch, -1).all(dim=1)
        if not bool(eq.all()):
            r = torch.nonzero(~eq).reshape(-1)
            bad.append((entry, q, n, T, nc, flags, batch, int(r.numel()), int(r[0]), S.ARITH_NAMES[S.arithmetic(q, n)]))
    return t_ref


def _report(bad):
    for row in bad:
        print("MISMATCH %s q=%d n=%d T=%d nc=%d flags=%d batch=%d: %d rows, first %d (%s)" % row)
    assert not bad, "%d of the calls gave wrong words; the first: %r" % (len(bad), bad[0])


@pytest.mark.parametrize("n", [pytest.param(n, marks=_timeout("mac", n)) for n in S.MAC_SIZES])
def test_mac_rows_surfaces_with_every_flag_combination(pkg, oracle, n):
    bad, t0, t_ref = [], time.time(), 0.0
    cases = [c for c in S.MAC_CASES if c[1] == n]
    for q, nn, entry, T, nc in cases:
        t_ref += _mac_case(pkg, oracle, q, n, entry, T, nc, bad)
    print("\nmac_rows surfaces, n = %d: %d cases x 8 flag combinations, %d batch rows through each, references %.1f s, all %.1f s"
          % (n, len(cases), 5 * len(cases), t_ref, time.time() - t0))
    _report(bad)


@_timeout("one", "grid_stride")
def test_grid_stride_loops_make_a_second_trip(pkg, oracle):
    """fhe_ew_grid caps a launch at 4096 workgroups (2^20 threads): n = 2^14 with batch 129 gives mac_rows_kernel
    129 * 8192 > 2^20 threads of work in each of the three surfaces, and a key switch of 129 ciphertexts through
    decompose_kernel (batch k n words) and ks_tail_kernel (batch (k+1) n words) the same"""
    import torch

    n, batch, bad = 16384, 129, []
    assert batch * (n // 2) > 1 << 20
    for q in (Q61, S.Q30, S.Q63):
        _mac_case(pkg, oracle, q, n, "tr_dot", 2, 1, bad, batch=batch, d=2)
        _mac_case(pkg, oracle, q, n, "tr_mul_r", 1, 2, bad, batch=batch, d=2)
        _mac_case(pkg, oracle, q, n, "glev_mul", 2, 2, bad, batch=batch, d=2)
    _report(bad)
    kbad, nbad = [], []
    for q, beta, l in ((Q61, 4, 2), (S.Q62, 2, 3)):
        assert S.ks_route(q, n, 1, beta, l, "coeffs") == "generic-decompose-kstail" and batch * n > 1 << 20
        g = _KsGroup(pkg, oracle, q, n, 1, beta, l, None)
        g.run(batch, None, kbad, nbad)
    torch.cuda.synchronize()
    assert not kbad and not nbad, (kbad[:1], nbad[:1])


# ---- worst-case rows with a closed form ----------------------------------------------------------------------------------------------

@_timeout("one", "worst")
@pytest.mark.parametrize("q,n", S.WORST)
def test_worst_case_rows_with_a_closed_form(pkg, oracle, q, n):
    """(i) coefficients: every operand word q - 1, coefficient j of (-(1 + .. + X^(n-1)))^2 is 2 j + 2 - n.  (ii) NTT
    domain, all three flags, every word q - 1: each term is (q - 1)^2 = 1 (mod q), the accumulators see their largest
    terms, and every output word is T mod q; T = 33 passes four folds of 8 (and 16 of 2 at the strict-63 prime)"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    plan = pkg.Plan(q, n)
    batch = 3
    full = lambda *shape: torch.full(shape, q - 1, dtype=torch.int64, device="cuda")
    sq = [2 * j + 2 - n for j in range(n)]
    for T in (3, 5, 33, 40):
        a = full(batch, T, n)
        out = torch.empty((batch, n), dtype=torch.int64, device="cuda")
        out.fill_(POISON)
        B._check(L.fhe_tr_dot_dev(plan.handle, a.data_ptr(), a.data_ptr(), out.data_ptr(), T, batch, 0, None))
        assert _u64(out).tolist() == [[T * s % q for s in sq]] * batch, ("tr_dot coefficients", T)
        out.fill_(POISON)
        B._check(L.fhe_tr_dot_dev(plan.handle, a.data_ptr(), a.data_ptr(), out.data_ptr(), T, batch, 7, None))
        assert torch.equal(out, torch.full_like(out, T % q)), ("tr_dot evals", T)
        for k in (1, 2):
            glev, v = full(T, k + 1, n), full(batch, T, n)
            outg = torch.empty((batch, k + 1, n), dtype=torch.int64, device="cuda")
            outg.fill_(POISON)
            B._check(L.fhe_glev_mul_dev(plan.handle, k, T, glev.data_ptr(), v.data_ptr(), outg.data_ptr(), batch, 0, None))
            assert _u64(outg).tolist() == [[[T * s % q for s in sq]] * (k + 1)] * batch, ("glev_mul coefficients", T, k)
            outg.fill_(POISON)
            B._check(L.fhe_glev_mul_dev(plan.handle, k, T, glev.data_ptr(), v.data_ptr(), outg.data_ptr(), batch, 7, None))
            assert torch.equal(outg, torch.full_like(outg, T % q)), ("glev_mul evals", T, k)
    a, p = full(batch, 3, n), full(batch, n)
    out = torch.empty_like(a)
    out.fill_(POISON)
    B._check(L.fhe_tr_mul_r_dev(plan.handle, a.data_ptr(), p.data_ptr(), out.data_ptr(), 3, batch, 0, None))
    assert _u64(out).tolist() == [[[s % q for s in sq]] * 3] * batch
    out.fill_(POISON)
    B._check(L.fhe_tr_mul_r_dev(plan.handle, a.data_ptr(), p.data_ptr(), out.data_ptr(), 3, batch, 7, None))
    assert torch.equal(out, torch.ones_like(out))
    # key switch, base 2, l = 64: every digit saturates to 1 against a q - 1 key (the sign of test_crt_bounds.py:513-515)
    bad, nbad = [], []
    for k in (1, 2):
        g = _KsGroup(pkg, oracle, q, n, k, 2, 64, None, worst=True)
        for b in (batch, 1):
            g.run(b, None, bad, nbad)
        assert _u64(g.want[0]).tolist() == S.ks_worst_closed(q, n, k, 64)
    assert not bad and not nbad, (bad[:1], nbad[:1])


# ---- decompose ---------------------------------------------------------------------------------------------------------------------

@_timeout("one", "decompose")
@pytest.mark.parametrize("n", [2, 256, 16384])
def test_decompose_both_bases_at_the_branch_edges(pkg, oracle, n):
    import torch

    L, B = pkg.load_library(), pkg.binding
    rng = np.random.default_rng(n)
    for q, beta, l in ((Q16, 2, 1), (Q16, 2, 16), (Q16, 2, 17), (Q16, 4, 6), (Q16, 4, 8), (Q61, 2, 61), (Q61, 2, 64), (Q61, 4, 15), (Q61, 7, 11),
                       (S.Q63, 2, 63), (S.Q63, 2, 64), (S.Q63, 2, 5), (S.Q63, 4, 15), (S.Q63, 3, 20)):
        assert S.decompose_args_ok(q, beta, l)
        d = 3
        a = _rand(rng, q, (d, n))
        e = _edges(q, beta, l)
        for i in range(d):                                                 # the edge words at the front, the middle and the end
            m = min(n, len(e))
            pos = (0, (n - m) // 2, n - m)[i]
            a[i, pos:pos + m] = (e if i != 2 else e[::-1])[:m]
        want = _dev(np.stack(_each(lambda r: ref_decompose(oracle, q, n, r, beta, l), list(a))))
        da = _dev(a)
        for rows in (1, 7, 65 if n == 16384 and l <= 17 else 3):          # 65 * 2^14 > 2^20: the loop's second trip
            idx = torch.from_numpy(_tile(rows, d)).cuda()
            src = da[idx].contiguous()
            out = torch.empty((rows, l, n), dtype=torch.int64, device="cuda")
            out.fill_(POISON)
            B._check(L.fhe_rq_decompose_dev(q, n, beta, l, src.data_ptr(), out.data_ptr(), rows, None))
            assert torch.equal(out, want[idx]), (q, n, beta, l, rows)
    assert 65 * 16384 > 1 << 20


# ---- the f64 rows -------------------------------------------------------------------------------------------------------------------

@_timeout("one", "f64")
@pytest.mark.parametrize("q", S.F64_Q)
def test_f64_rows_at_ties_conversions_and_saturation(pkg, q):
    """against Python floats: for every (num, den), (p, q) and (1, s) the words whose quotient is x.5 as a double, x even
    and odd (test_rq_rows_cpu.float_ties; `round` and `rint` part on the even ones), and their neighbours; words around
    2^53, the largest canonical word, NaN and infinities, e on +-2^63; once per entry point with more than 2^20 words"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    out_of = {}

    def run(words, call, ref, tag):
        a = _arr(sorted(words))
        kind = tag.split("(")[0]                                           # the first call of each kind: count > 2^20
        reps = 1 if kind in out_of else -(-((1 << 20) + 5) // len(a))
        out_of[kind] = True
        da = _dev(np.tile(a, reps))
        out = torch.empty_like(da)
        out.fill_(POISON)
        B._check(call(da.data_ptr(), out.data_ptr(), da.numel()))
        want = _arr([ref(int(v)) for v in a])
        got = _u64(out)
        if not np.array_equal(got, np.tile(want, reps)):
            i = int(np.nonzero(got != np.tile(want, reps))[0][0])
            raise AssertionError("%s: word %d (v = %d): got %d, want %d" % (tag, i, int(np.tile(a, reps)[i]), int(got[i]), int(np.tile(want, reps)[i])))

    for num, den in S.f64_pairs(q):                                        # the sweep is not without its ties
        even, odd = S.float_ties(q, num, den)
        assert S.no_float_tie(q, num, den) or (even and odd and even | odd <= S.tie_words(q, num, den)), (q, num, den)
    t = 65537 if q != Q16 else 17
    for num, den in S.mul_div_pairs(q) + [(t, q)]:
        words = set(S.f64_inputs(q)) | S.tie_words(q, num, den)
        run(words, lambda a, c, cnt: L.fhe_rq_mul_div_round_dev(q, num, den, a, c, cnt, None), lambda v: P.mul_div_round(q, num, den, v),
            "mul_div_round(%d, %d)" % (num, den))
    for p in S.mod_switch_ps(q):
        words = set(S.f64_inputs(q)) | S.tie_words(q, p, q)
        run(words, lambda a, c, cnt: L.fhe_rq_mod_switch_dev(q, p, a, c, cnt, None), lambda v: P.mod_switch(q, p, v), "mod_switch(%d)" % p)
    for s in S.DIV_ROUND_S:
        words = set(S.f64_inputs(q)) | S.tie_words(q, 1, s)
        run(words, lambda a, c, cnt: L.fhe_rq_div_round_dev(q, s, a, c, cnt, None), lambda v: P.div_round(q, s, v), "div_round(%d)" % s)
    for s in S.mul_f64_factors(q):
        run(S.f64_inputs(q), lambda a, c, cnt: L.fhe_rq_mul_by_f64_dev(q, s, a, c, cnt, None), lambda v: P.mul_by_f64(q, s, v), "mul_by_f64(%r)" % s)
    for p in (2, Q16, q, (1 << 63) - 25):
        run(S.f64_inputs(q), lambda a, c, cnt: L.fhe_rq_remodule_dev(p, a, c, cnt, None), lambda v: P.remodule(p, v), "remodule(%d)" % p)
    torch.cuda.synchronize()


@_timeout("one", "elementwise")
@pytest.mark.parametrize("q,n", [(Q16, 256), (S.Q30, 16384), (Q61, 16384), (S.QMG, 1024), (S.Q62, 64), (S.Q63, 16384)])
def test_elementwise_rows_with_a_second_trip(pkg, q, n):
    """add, sub, neg, mul_by_u64 against Python integers, batch n > 2^20 at the large sizes"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    plan = pkg.Plan(q, n)
    batch = 65 if n == 16384 else 5
    rng = np.random.default_rng(n)
    a, b = _rand(rng, q, (batch, n)), _rand(rng, q, (batch, n))
    a[0, :6], b[0, :6] = [0, q - 1, 1, q // 2, 0, q - 1], [0, q - 1, q - 1, q // 2 + 1, q - 1, 0]
    a[-1, -2:], b[-1, -2:] = [q - 1, 0], [q - 1, 1]
    ao, bo = a.astype(object), b.astype(object)
    da, db = _dev(a), _dev(b)
    out = torch.empty_like(da)
    out.fill_(POISON)
    B._check(L.fhe_rq_add_dev(plan.handle, da.data_ptr(), db.data_ptr(), out.data_ptr(), batch, None))
    assert np.array_equal(_u64(out), ((ao + bo) % q).astype(np.uint64))
    out.fill_(POISON)
    B._check(L.fhe_rq_sub_dev(plan.handle, da.data_ptr(), db.data_ptr(), out.data_ptr(), batch, None))
    assert np.array_equal(_u64(out), ((ao - bo) % q).astype(np.uint64))
    out.fill_(POISON)
    B._check(L.fhe_rq_neg_dev(plan.handle, da.data_ptr(), out.data_ptr(), batch, None))
    assert np.array_equal(_u64(out), ((-ao) % q).astype(np.uint64))
    for s in (0, 1, q - 1, q, q + 5, (1 << 64) - 1):
        out.fill_(POISON)
        B._check(L.fhe_rq_mul_by_u64_dev(plan.handle, da.data_ptr(), s, out.data_ptr(), batch, None))
        assert np.array_equal(_u64(out), ((ao * (s % q)) % q).astype(np.uint64)), s


# ---- host-buffer forms -----------------------------------------------------------------------------------------------------------

@_timeout("one", "host")
@pytest.mark.parametrize("q,n", [(Q16, 256), (S.QMG, 64)])
def test_host_buffer_forms(pkg, oracle, q, n):
    """fhe_tr_dot / fhe_tr_mul_r / fhe_glev_mul / fhe_glwe_key_switch on a WORD32 plan and a Montgomery plan, batch 3"""
    import ctypes

    L, chk = pkg.load_library(), pkg.binding._check
    assert S.arithmetic(q, n) == (S.WORD32 if q == Q16 else S.MONTGOMERY)
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    k, beta, l, batch = 2, 2, 9, 3
    plan = pkg.Plan(q, n)
    rng = np.random.default_rng(q % 1000 + n)
    a, b, p = _mac_rows(rng, q, (batch, k, n)), _mac_rows(rng, q, (batch, k, n)), _mac_rows(rng, q, (batch, n))
    c, out = np.full((batch, n), POISON, dtype=np.uint64), np.full((batch, k, n), POISON, dtype=np.uint64)
    chk(L.fhe_tr_dot(plan.handle, vp(a), vp(b), vp(c), k, batch))
    chk(L.fhe_tr_mul_r(plan.handle, vp(a), vp(p), vp(out), k, batch))
    assert c.tolist() == [P.tr_dot(q, a[i], b[i]) for i in range(batch)]
    assert out.tolist() == [P.tr_mul_r(q, a[i], p[i]) for i in range(batch)]
    glev, v = _mac_rows(rng, q, (1, l, k + 1, n))[0], _mac_rows(rng, q, (batch, l, n))
    glwe, ksk = _mac_rows(rng, q, (batch, k + 1, n)), _rand(rng, q, (k, l, k + 1, n))
    got = np.full((batch, k + 1, n), POISON, dtype=np.uint64)
    chk(L.fhe_glev_mul(plan.handle, k, l, vp(glev), vp(v), vp(got), batch))
    assert got.tolist() == [P.glev_mul(q, glev, v[i]) for i in range(batch)]
    got[:] = POISON
    chk(L.fhe_glwe_key_switch(plan.handle, k, beta, l, vp(glwe), vp(ksk), vp(got), batch))
    assert got.tolist() == [P.key_switch(q, k, beta, l, glwe[i], ksk) for i in range(batch)]


# ---- the other routes, in processes of their own -----------------------------------------------------------------------------------

CHILD_SHAPES = [(Q61, 1024, 1, 64), (Q61, 2048, 1, 33), (Q61, 4096, 1, 64), (Q61, 1024, 2, 33), (Q16, 256, 2, 16), (S.QMG, 512, 1, 40),
                (S.Q61S, 256, 1, 64), (S.Q30, 2048, 1, 30)]

_CHILD = r"""
import hashlib, sys
sys.path.insert(0, %r)
import numpy as np, torch
import fhe_study_amd as pkg
L, B = pkg.load_library(), pkg.binding
h = hashlib.sha256()
B.kernel_timing_reset(); B.kernel_timing_enable(True)
for q, n, k, l in %r:
    plan = pkg.Plan(q, n)
    for batch in (1, 130):
        ct = torch.full((batch, k + 1, n), q - 1, dtype=torch.int64, device="cuda")
        ksk = torch.full((k, l, k + 1, n), q - 1, dtype=torch.int64, device="cuda")
        o = torch.empty_like(ct)
        B._check(L.fhe_glwe_key_switch_dev(plan.handle, k, 2, l, ct.data_ptr(), ksk.data_ptr(), o.data_ptr(), batch, 0, None))
        torch.cuda.synchronize()
        h.update(o.cpu().numpy().tobytes())
print("kernels", " ".join(sorted(B.kernel_timing_read())))
print("digest", h.hexdigest())
"""


def _worst_rows_digest():
    """what the child must print: the key switch of q - 1 ciphertexts under a q - 1 key, from Python integers (the
    digits of q - 1: saturated to 1 where q - 1 >= 2^l, its bits otherwise)"""
    h = hashlib.sha256()
    for q, n, k, l in CHILD_SHAPES:
        digits = P.decompose(q, q - 1, 2, l)
        rhs = [k * sum(digits) * (n - 2 - 2 * j) for j in range(n)]        # (q-1)(1+..) x d(1+..) = -d (n - 2 - 2j) ... times -1
        row = [[(0 - r) % q for r in rhs]] * k + [[(q - 1 - r) % q for r in rhs]]
        for batch in (1, 130):
            h.update(np.array([row] * batch, dtype=np.uint64).tobytes())
    return h.hexdigest()


@_timeout("one", "children")
def test_worst_rows_same_words_on_the_other_routes(pkg):
    """fresh processes with the defaults, with FHE_EXT32=0 and with FHE_DIGIT_MAC_FUSED=0: the digest of the closed form in
    all three, and the kernel names prove the route changed"""
    script = _CHILD % (ROOT, CHILD_SHAPES)
    outs = {}
    for name, env in (("default", {}), ("ext32-off", {"FHE_EXT32": "0"}), ("fused-off", {"FHE_DIGIT_MAC_FUSED": "0"})):
        r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=500)
        assert r.returncode == 0, name + r.stdout + r.stderr
        outs[name] = dict(x.split(" ", 1) for x in r.stdout.splitlines() if x.startswith(("digest", "kernels")))
    want = _worst_rows_digest()
    for name in outs:
        assert outs[name]["digest"] == want, name
    k_def, k_ext, k_fus = (outs[x]["kernels"].split() for x in ("default", "ext32-off", "fused-off"))
    for prefix in ("digit_tail32_ks_", "digit_mac32_", "digit_mac_zq_", "digit_tail_ks_", "sq_forward"):
        assert _has(k_def, prefix), (prefix, k_def)
    assert not any(s.startswith(("digit_tail32", "digit_mac32", "ntt32_", "sq")) for s in k_ext), k_ext
    assert _has(k_ext, "digit_mac_zq_") and _has(k_ext, "digit_tail_ks_")
    assert not _has(k_fus, "digit_mac_zq") and _has(k_fus, "mac_rows") and _has(k_fus, "ntt_fwd_zqbits") and _has(k_fus, "digit_tail32_ks_")
