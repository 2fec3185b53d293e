"""The BFV surfaces (fhe_bfv_tensor_dev, fhe_bfv_relinearize*_dev, fhe_bfv_mul*_dev: csrc/zring.hip, csrc/bfv32.hip) at
every launch class of tests/test_bfv_shapes_cpu.py, word for word against a plain reference: tests/_bfv_numpy.py (Python
integers, no NTT) for n <= 64 and the oracle's schoolbook above.  Every check is exact equality of integer words.

Each (q, t, pq) group of an n builds a few distinct input rows (one of q - 1 throughout, one with the words 0, 1, q - 1,
q // 2 planted, the rest random) and a key with one random half and one half of pq - 1 throughout, computes every
reference once and tiles the rows into each batch on the device, so every one of the `batch` output rows is compared (on
the device, after the output was poisoned).  Five entries run at every batch of the group's cover: the tensor, the
relinearisation fed by the REFERENCE's (c0, c1, c2) with the key prepared on the fly, the same against a key prepared once
per group (the raw key zeroed afterwards), fhe_bfv_mul_dev and fhe_bfv_mul_prepared_dev.  The batches of one group run
descending then ascending on one stream, so workspace slots 0 and 1 are reused under a smaller, then a larger request with
the previous call's words in them; the first group of every n runs on a stream of its own; the kernel timer's names must
show the route the restatement predicts and none of the other family's, down to the kind, LA and block size of the
2n-point transforms (rows per workgroup and tile counts do not show in a name: there the comparison of every row stands).

Distinct rows: 6 while n <= 1024, 2 above.  Measured on an MI355X box (references on 8 threads): the sweep takes 0.03 - 0.14 s
per n up to 2048, 0.3 s at 4096, 0.7 s at 8192 (0.5 s of it the host reference) and 1.4 s at 2^14 (1.2 s the reference);
12 s for whichever test runs first, which loads the library and the device; the three child processes 8.9 s together, the
host-buffer forms 0.6 s, every other test below 0.2 s; 25 s for the whole module (TIMES below).

Every route the restatement predicted was the route the kernel timer showed, staging at n = 2 and 4 alone included; no
call of the sweep gave a wrong word."""
import hashlib
import json
import os
import subprocess
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _bfv_numpy as BN
import test_bfv_shapes_cpu as S
from conftest import Q16, Q61, ROOT
from test_crt_bounds import _has, _ran, primes_for_bits, relin_form, tensor_form
from test_gadget_shapes_gpu import POISON, _ladder, _tile

pytestmark = pytest.mark.gpu

PY_REF_MAX_N = 64                # the Python reference up to here, the oracle above
_POOL = ThreadPoolExecutor(8)    # ctypes releases the interpreter lock: oracle references run side by side
CHILD_BATCHES = (1, 8, 9, 17)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(pkg):
    assert pkg.binding.device_count() >= 1, "no HIP device: -m gpu tests need a real MI355X"


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64).copy()).cuda()


def _arr(x):
    return np.array(x, dtype=np.uint64)


# ---- references, computed once per (q, t, pq, n) and shared by every test of the module ------------------------------------------
_TENSOR, _RELIN = {}, {}


def ref_tensor(oracle, q, t, n, ab):
    """-> (3, d, n), one job per distinct row"""
    key = (q, t, n, ab.shape[1])
    if key not in _TENSOR:
        if n <= PY_REF_MAX_N:
            rows = [BN.tensor(q, n, t, *ab[:, i]) for i in range(ab.shape[1])]
            _TENSOR[key] = _arr(rows).transpose(1, 0, 2).copy()
        else:
            jobs = [_POOL.submit(oracle.bfv_tensor, q, n, t, *ab[:, i]) for i in range(ab.shape[1])]
            _TENSOR[key] = np.stack([np.stack([j.result()[w][0] for j in jobs]) for w in range(3)])
    return _TENSOR[key]


def ref_relin(oracle, q, pq, n, rlk, c, ckey):
    """-> (2, d, n): the relinearisation of the reference's tensor, which is also the reference's multiply"""
    key = (q, pq, n, ckey)
    if key not in _RELIN:
        d = c.shape[1]
        if n <= PY_REF_MAX_N:
            rows = [BN.relinearize(q, n, pq, rlk[0], rlk[1], *c[:, i]) for i in range(d)]
            _RELIN[key] = _arr(rows).transpose(1, 0, 2).copy()
        else:
            jobs = [_POOL.submit(oracle.bfv_relinearize, q, n, pq, rlk[0], rlk[1], *c[:, i]) for i in range(d)]
            _RELIN[key] = np.stack([np.stack([j.result()[w][0] for j in jobs]) for w in range(2)])
    return _RELIN[key]


def prefetch(oracle, n, groups):
    """the oracle's references of every (q, t, pq) of `groups` at n at once, a job per distinct row on the pool: all the
    tensors, then all the relinearisations (a group alone keeps two threads busy)"""
    if n <= PY_REF_MAX_N:
        return
    d = S.distinct_rows(n)
    data = {g: S.inputs(g[0], g[2], n, d) for g in groups}
    jobs = {}
    for (q, t, pq), (ab, _) in data.items():
        if (q, t, n, d) not in _TENSOR and (q, t) not in jobs:
            jobs[q, t] = [_POOL.submit(oracle.bfv_tensor, q, n, t, *ab[:, i]) for i in range(d)]
    for (q, t), js in jobs.items():
        _TENSOR[q, t, n, d] = np.stack([np.stack([j.result()[w][0] for j in js]) for w in range(3)])
    jobs = {}
    for (q, t, pq), (_, rlk) in data.items():
        if (q, pq, n, (t, d)) not in _RELIN:
            c = _TENSOR[q, t, n, d]
            jobs[q, t, pq] = [_POOL.submit(oracle.bfv_relinearize, q, n, pq, rlk[0], rlk[1], *c[:, i]) for i in range(d)]
    for (q, t, pq), js in jobs.items():
        _RELIN[q, pq, n, (t, d)] = np.stack([np.stack([j.result()[w][0] for j in js]) for w in range(2)])


class _Group:
    """the data and references of one (q, t, pq, n): everything the batch ladder and the five entries share"""

    def __init__(self, pkg, oracle, q, t, pq, n):
        self.L, self.B = pkg.load_library(), pkg.binding
        self.q, self.t, self.pq, self.n = q, t, pq, n
        d = self.d = S.distinct_rows(n)
        ab, rlk = S.inputs(q, pq, n, d)
        self.h_ab, self.h_rlk = ab, rlk
        self.h_c = ref_tensor(oracle, q, t, n, ab) if oracle is not None else None
        self.h_o = ref_relin(oracle, q, pq, n, rlk, self.h_c, (t, d)) if oracle is not None else None
        self.prep = None

    def upload(self):
        import torch

        self.ab, self.rlk = _dev(self.h_ab), _dev(self.h_rlk)
        self.c = _dev(self.h_c) if self.h_c is not None else None
        self.o = _dev(self.h_o) if self.h_o is not None else None
        self.words = self.L.fhe_bfv_rlk_prepared_words(self.q, self.n, self.pq)
        assert self.words == S.rlk_words(self.q, self.n, self.pq) != 0
        self.prep = torch.empty(self.words, dtype=torch.int64, device="cuda")
        return self

    def prepare(self, st):
        """the key prepared once from a copy of the raw key, which is zeroed afterwards"""
        raw = self.rlk.clone()
        self.prep.fill_(POISON)
        self.B._check(self.L.fhe_bfv_rlk_prepare_dev(self.q, self.n, self.pq, raw.data_ptr(), self.prep.data_ptr(), st))
        raw.zero_()

    def calls(self, batch, st):
        """the five entries at one batch on stream st (the current torch stream) -> the tiling, [(entry, output tensor)]"""
        import torch

        q, t, pq, n, L, B = self.q, self.t, self.pq, self.n, self.L, self.B
        idx = torch.from_numpy(_tile(batch, self.d)).cuda()
        ab = self.ab[:, idx].contiguous()
        outs = []
        c = torch.empty((3, batch, n), dtype=torch.int64, device="cuda").fill_(POISON)
        B._check(L.fhe_bfv_tensor_dev(q, n, t, ab.data_ptr(), c.data_ptr(), batch, st))
        outs.append(("tensor", c))
        cin = self.c[:, idx].contiguous()                                  # the REFERENCE's tensor feeds the relinearisations
        for entry in S.ENTRIES[1:]:
            o = torch.empty((2, batch, n), dtype=torch.int64, device="cuda").fill_(POISON)
            if entry == "relin":
                rc = L.fhe_bfv_relinearize_dev(q, n, pq, self.rlk.data_ptr(), cin.data_ptr(), o.data_ptr(), batch, st)
            elif entry == "prepared":
                rc = L.fhe_bfv_relinearize_prepared_dev(q, n, pq, self.prep.data_ptr(), cin.data_ptr(), o.data_ptr(), batch, st)
            elif entry == "mul":
                rc = L.fhe_bfv_mul_dev(q, n, t, pq, self.rlk.data_ptr(), ab.data_ptr(), o.data_ptr(), batch, st)
            else:
                rc = L.fhe_bfv_mul_prepared_dev(q, n, t, pq, self.prep.data_ptr(), ab.data_ptr(), o.data_ptr(), batch, st)
            B._check(rc)
            outs.append((entry, o))
        return idx, outs

    def run(self, batch, st, bad):
        """the five entries at one batch, each compared with the tiled references; mismatches are appended to bad"""
        idx, outs = self.calls(batch, st)
        for entry, out in outs:
            bad += S.compare_tiled((self.q, self.t, self.pq, self.n, batch, entry), out, self.c if entry == "tensor" else self.o, idx)

    def sweep(self, batches, st, bad):
        self.prepare(st)
        for batch in _ladder(batches):
            self.run(batch, st, bad)


def predicted_names(q, t, pq, n):
    """the kernel-timer names a group's five entries must show, and the prefixes none of them may show"""
    lg2 = n.bit_length()
    (tf, tK), (rf, rK) = tensor_form(q, n), relin_form(q, n, pq)
    must, never = set(), set()
    mdr_k = set()
    if tf == "bfv32":
        must.add("bfv32_tensor_inverse_%d" % lg2)
        never.add("zr_tensor")
    else:
        must.add("zr_tensor_0")
        never.add("bfv32_tensor")
        la = S.inverse_mdr_la(n, tK)
        if la:
            must.add("zr_inv_strided_mdr_%d" % la)
        else:
            mdr_k.add(tK)
    if rf == "bfv32":
        must.add("bfv32_relin_inverse_%d" % lg2)
        never |= {"zr_split_mdr", "zr_mul_bcast"}
    else:
        must.add("zr_mul_bcast_0")
        never.add("bfv32_relin")
        if rf == "split":
            must.add("zr_split_mdr_0")
        else:
            never.add("zr_split_mdr")
            mdr_k.add(rK)
    if tf == "bfv32" and rf == "bfv32":
        never.add("zr_")
    if tf != "bfv32" and rf != "bfv32":
        never.add("bfv32_")
    if tf == "bfv32" or not S.inverse_mdr_la(n, tK):
        never.add("zr_inv_strided_mdr")
    for K in (1, 2, 3):
        (must if K in mdr_k else never).add("zr_crt_mdr_%d" % K)
    if S.staged(n):                                       # (no bfv32 size is staged)
        must.add("zr_reduce_pad_0")
    else:
        never.add("zr_reduce_pad")
    if tf != "bfv32" or rf != "bfv32":                  # the 2n-point transforms of the 61-bit forms: kind, LA and block size of S.transform
        kind, _, la, _ = S.transform(n)
        fused = tf != "bfv32" and S.inverse_mdr_la(n, tK)
        if kind == "tiny":
            must |= {"ntt_tiny_fwd_%d" % lg2, "ntt_tiny_inv_%d" % lg2}
            never |= {"ntt_fwd_reduce", "ntt_fwd_strided", "ntt_inv_contig", "ntt_inv_strided"}
        elif kind == "single":
            must |= {"ntt_fwd_reduce_%d" % lg2, "ntt_inv_contig_final_%d" % lg2}
            never |= {"ntt_tiny", "ntt_fwd_strided", "ntt_inv_strided"}
        else:
            must |= {"ntt_fwd_strided_reduce_%d" % la, "ntt_fwd_contig_final_%d" % (lg2 - la), "ntt_inv_contig_%d" % (lg2 - la)}
            never |= {"ntt_tiny", "ntt_fwd_reduce", "ntt_inv_contig_final"}
            if rf != "bfv32" or not fused:                # (the relinearisation's inverse is never fused)
                must.add("ntt_inv_strided_%d" % la)
    return must, never


def check_route(q, t, pq, n, names):
    must, never = predicted_names(q, t, pq, n)
    for nm in must:
        assert nm in names, (q, t, pq, n, nm, sorted(names))
    for prefix in never:
        assert not _has(names, prefix), (q, t, pq, n, prefix, sorted(names))


def _report(bad):
    for row in bad[:20]:
        print("MISMATCH (q, t, pq, n, batch, entry) = %r: plane %d, %d rows wrong, first %d, last %d" % row)
    assert not bad, "%d planes of the calls gave wrong words; the first: %r" % (len(bad), bad[0])


# measured wall seconds per n on an MI355X box, rounded up (references on 8 threads).  pytest.mark.timeout is twice that, with
# a floor of 120 s: nearly all of it is the schoolbook reference on the host, and a core six times slower than the measured
# one is common
TIMES = {2: 1, 4: 1, 8: 1, 16: 1, 32: 1, 64: 1, 128: 1, 256: 1, 512: 1, 1024: 1, 2048: 1, 4096: 1, 8192: 1, 16384: 2}


def _sweep(pkg, oracle, n):
    import torch

    B = pkg.binding
    bad = []
    t_ref, t0, rows = 0.0, time.time(), 0
    prefetch(oracle, n, [g for g, _ in S.groups_of(n)])
    t_ref += time.time() - t0
    for i, ((q, t, pq), batches) in enumerate(S.groups_of(n)):
        tr = time.time()
        g = _Group(pkg, oracle, q, t, pq, n).upload()
        t_ref += time.time() - tr
        rows += sum(_ladder(batches))
        if i == 0:                                                         # a stream of its own
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                names = _ran(B, lambda: g.sweep(batches, side.cuda_stream, bad))
            torch.cuda.synchronize()
            B._check(pkg.load_library().fhe_ntt_release_stream_workspace(side.cuda_stream))
        else:
            names = _ran(B, lambda: g.sweep(batches, None, bad))
        check_route(q, t, pq, n, names)
        del g
    print("\nn = %d: %d groups, %d batch rows through each of 5 entries, references %.1f s, all %.1f s"
          % (n, len(S.groups_of(n)), rows, t_ref, time.time() - t0))
    _report(bad)


@pytest.mark.parametrize("n", [pytest.param(n, marks=pytest.mark.timeout(max(120, 2 * TIMES[n]))) for n in S.SIZES])
def test_sweep(pkg, oracle, n):
    _sweep(pkg, oracle, n)


HOST_FORMS = [
    # q, t, pq, n, batch: one ragged batch per form
    (Q16, 2, Q16 ** 3, 1024, 9),                    # bfv32 for both stages
    (S.Q20, 5, S.Q20 ** 3, 2048, 9),                # bfv32 tensor, two 61-bit primes behind it
    (Q16, 2, Q16 ** 3, 16, 9),                      # one prime, one pass; split key
    (Q16, 2, Q16 ** 3, 4, 9),                       # staged
    (S.Q30, 3, S.Q30 ** 2, 16, 9),                  # two primes
    (Q61, 16, 2 * Q61, 16, 9),                      # three primes
    (Q16, 2, Q16 ** 3, 16384, 3),                   # the fused last pass
]


@pytest.mark.timeout(240)
def test_host_buffer_forms(pkg, oracle):
    """fhe_bfv_tensor and fhe_bfv_mul (host pointers) at one ragged batch per form, against the same references"""
    forms = set()
    for q, t, pq, n, batch in HOST_FORMS:
        g = _Group(pkg, oracle, q, t, pq, n)
        idx = _tile(batch, g.d)
        ab = np.ascontiguousarray(g.h_ab[:, idx])
        c = np.stack(pkg.binding.bfv_tensor(q, n, t, *ab))
        assert np.array_equal(c, g.h_c[:, idx]), (q, t, n, batch)
        o = np.stack(pkg.binding.bfv_mul(q, n, t, pq, g.h_rlk[0], g.h_rlk[1], *ab))
        assert np.array_equal(o, g.h_o[:, idx]), (q, t, pq, n, batch)
        tf, rf = tensor_form(q, n), relin_form(q, n, pq)
        forms.add((tf[0], tf[1] if tf[0] == "crt" else 0, S.staged(n), bool(S.inverse_mdr_la(n, tf[1])) and tf[0] == "crt", rf[0]))
    if S.EXT32:
        assert len(forms) == len(HOST_FORMS), forms


@pytest.mark.timeout(240)
def test_two_streams_two_threads(pkg, oracle):
    """a bfv32 group and a 61-bit group (two primes) at n = 1024 run their ladders at the same time, each on its own
    stream from its own host thread, with no synchronisation between them: every row of every call is compared"""
    import torch

    n = 1024
    specs = [(Q16, 2, Q16 ** 3), (S.Q30, 3, S.Q30 ** 2)]
    if S.EXT32:
        assert tensor_form(Q16, n)[0] == "bfv32" and relin_form(Q16, n, Q16 ** 3)[0] == "bfv32"
    assert tensor_form(S.Q30, n) == ("crt", 2) and relin_form(S.Q30, n, S.Q30 ** 2) == ("crt", 2)
    jobs = []
    for q, t, pq in specs:
        g = _Group(pkg, oracle, q, t, pq, n).upload()
        jobs.append(dict(g=g, stream=torch.cuda.Stream(), bad=[], err=[]))
    torch.cuda.synchronize()
    batches = (1, 7, 8, 9, 17, 33, 64, 65)

    def worker(j):
        try:
            with torch.cuda.stream(j["stream"]):
                for _ in range(2):
                    j["g"].sweep(batches, j["stream"].cuda_stream, j["bad"])
                j["stream"].synchronize()
        except Exception as e:                                             # reported by the parent thread
            j["err"].append(repr(e))

    threads = [threading.Thread(target=worker, args=(j,)) for j in jobs]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    for j in jobs:
        assert not j["err"], j["err"]
        pkg.binding._check(pkg.load_library().fhe_ntt_release_stream_workspace(j["stream"].cuda_stream))
    _report(jobs[0]["bad"] + jobs[1]["bad"])


# ---- the forms switched off: fresh processes ---------------------------------------------------------------------------------------

def child_groups():
    """the groups of the cover at bfv32's sizes"""
    return [(q, t, pq, n) for n in S.BFV32_SIZES for (q, t, pq), _ in S.groups_of(n)]


def _digest(words):
    return hashlib.sha256(np.ascontiguousarray(words).tobytes()).hexdigest()[:24]


_CHILD = r"""
import json
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import torch
import fhe_study_amd as pkg
import test_bfv_shapes_gpu as G
tensors = np.load(sys.argv[1])
for q, t, pq, n in json.load(open(sys.argv[2])):        # the parent's groups: the cover itself depends on FHE_EXT32
    g = G._Group(pkg, None, q, t, pq, n)
    g.h_c = tensors["%%d_%%d_%%d" %% (q, t, n)]
    g.upload().prepare(None)
    for batch in G.CHILD_BATCHES:
        idx, outs = g.calls(batch, None)
        torch.cuda.synchronize()
        for entry, out in outs:
            print("digest", q, t, pq, n, batch, entry, G._digest(out.cpu().numpy()))
print("done")
""" % (ROOT, os.path.join(ROOT, "tests"))

CHILDREN = [
    ("ext32-off", dict(FHE_EXT32="0")),                                     # the 61-bit forms at bfv32's sizes, the fused pass at 8192
    ("general-forms", dict(FHE_BFV_SMALL_F64="0", FHE_BFV_FAST_DIV="0", FHE_BFV_BELOW_P="0")),
    ("int-round", dict(FHE_BFV_INT_ROUND="1")),
]


@pytest.mark.timeout(900)
def test_forms_switched_off_give_the_same_words(pkg, oracle, tmp_path):
    """three fresh processes, one after another: the groups of bfv32's sizes at batches 1, 8, 9, 17 with (i) FHE_EXT32=0,
    (ii) FHE_BFV_SMALL_F64=0 FHE_BFV_FAST_DIV=0 FHE_BFV_BELOW_P=0, (iii) FHE_BFV_INT_ROUND=1 print a digest per (group, batch,
    entry); each is the digest of the references.  (A child computes no reference: the reference's tensor, which feeds its
    relinearisations as it does in the sweep, reaches it in a file.)"""
    want, tensors = {}, {}
    for n in S.BFV32_SIZES:
        prefetch(oracle, n, [g for g, _ in S.groups_of(n)])
    for q, t, pq, n in child_groups():
        g = _Group(pkg, oracle, q, t, pq, n)
        tensors["%d_%d_%d" % (q, t, n)] = g.h_c
        for batch in CHILD_BATCHES:
            idx = _tile(batch, g.d)
            for entry in S.ENTRIES:
                want["%d %d %d %d %d %s" % (q, t, pq, n, batch, entry)] = _digest((g.h_c if entry == "tensor" else g.h_o)[:, idx])
    path, gpath = str(tmp_path / "tensors.npz"), str(tmp_path / "groups.json")
    np.savez(path, **tensors)
    with open(gpath, "w") as f:
        json.dump(child_groups(), f)
    for name, env in CHILDREN:
        r = subprocess.run([sys.executable, "-c", _CHILD, path, gpath], env=dict(os.environ, **env), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])     # a signal or an error: no further child
        got = dict(l[7:].rsplit(" ", 1) for l in r.stdout.splitlines() if l.startswith("digest "))
        assert r.stdout.rstrip().endswith("done") and set(got) == set(want), (name, len(got), len(want))
        wrong = sorted(k for k in want if got[k] != want[k])
        assert not wrong, (name, len(wrong), wrong[:8])


# ---- related rows ----------------------------------------------------------------------------------------------------------------------

NAIVE_BITS = ((20, 20), (50, 50), (0, 0))           # one, two and three primes at every n of NAIVE_SIZES
NAIVE_SIZES = (2, 16, 256, 4096)


def naive_ladder(n):
    cap = S.EW_CAP // (2 * n)
    return (1, 7, 9, cap - 1, cap, cap + 1)


@pytest.mark.timeout(240)
@pytest.mark.parametrize("n", NAIVE_SIZES)
def test_naive_mul_on_one_two_and_three_primes(pkg, oracle, n):
    """fhe_r_naive_mul_dev with operand bounds that select one, two and three primes, on a short ladder with both sides of
    2^20 / (2n) (zr_crt's second grid-stride trip): the 2n - 1 words of the schoolbook product and a 0 behind them"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    d = S.distinct_rows(n)
    bad = []
    for K, (ab_, bb_) in enumerate(NAIVE_BITS, start=1):
        assert primes_for_bits((ab_ or 64) + (bb_ or 64) + (n - 1).bit_length(), False) == K
        rng = np.random.default_rng([n, K])
        ha = rng.integers(0, 1 << (ab_ or 64), (d, n), dtype=np.uint64, endpoint=False)
        hb = rng.integers(0, 1 << (bb_ or 64), (d, n), dtype=np.uint64, endpoint=False)
        ha[0], hb[0] = (1 << (ab_ or 64)) - 1, (1 << (bb_ or 64)) - 1
        want = np.zeros((d, 2 * n), dtype=np.uint64)
        if n <= PY_REF_MAX_N:
            for i in range(d):
                want[i, :2 * n - 1] = _arr([x % (1 << 64) for x in BN.naive_mul(n, ha[i], hb[i])])
        else:
            jobs = [_POOL.submit(oracle.r_naive_mul, n, ha[i].view(np.int64), hb[i].view(np.int64)) for i in range(d)]
            for i, j in enumerate(jobs):
                want[i, :2 * n - 1] = j.result()[0].view(np.uint64)
        da, db, dw = _dev(ha), _dev(hb), _dev(want)
        for batch in _ladder(naive_ladder(n)):
            idx = torch.from_numpy(_tile(batch, d)).cuda()
            a, b = da[idx].contiguous(), db[idx].contiguous()
            out = torch.empty((1, batch, 2 * n), dtype=torch.int64, device="cuda").fill_(POISON)
            names = _ran(B, lambda: B._check(L.fhe_r_naive_mul_dev(n, a.data_ptr(), b.data_ptr(), out.data_ptr(), batch, ab_, bb_, None)))
            assert "zr_crt_%d" % K in names and ("zr_reduce_pad_0" in names) == S.staged(n), (n, K, sorted(names))
            bad += S.compare_tiled((n, K, batch, "naive_mul"), out, dw[None], idx)
    assert not bad, bad[:8]


I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
MDR_PAIRS = [
    (0, 5),                     # num = 0
    (3, 1), (Q61 - 1, 1),       # den = 1
    (1, 2), (3, 2), (5, 4),     # products exactly halfway between two integers, of both signs
    (1, 1 << 62), (3, (1 << 63) + 1),   # den > num |v| for the small words
    (1 << 40, 1), ((1 << 64) - 1, 3),   # a quotient that saturates `as i64`
    (2, Q16), (16, Q61),
]
MDR_WORDS = [I64_MAX, -I64_MAX, I64_MIN, 0, 1, -1, 2, -2, 3, -3, 5, -5, 6, -6, (1 << 53) + 1, -(1 << 53) - 1, 1 << 40, -(1 << 40),
             (1 << 62) - 1, -(1 << 62), Q61 - 1, 1 - Q61, 7, -7, 9, -9, 10, -10, 11, -11, 13]


@pytest.mark.timeout(120)
def test_mul_div_round_on_planted_words(pkg):
    """fhe_mul_div_round_dev on +-(2^63 - 1), -2^63, ties of both signs, num = 0, den = 1, den > num |v| and quotients
    that saturate `as i64`, against the Python restatement, at two moduli"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    n = 16
    assert len(MDR_WORDS) == 2 * n - 1
    rows = [MDR_WORDS, MDR_WORDS[::-1], [(-1) ** i * (i + 1) for i in range(2 * n - 1)]]
    v = np.array([[x % (1 << 64) for x in r] + [POISON] for r in rows], dtype=np.uint64)    # word 2n - 1 is not read
    dv = _dev(v)
    for q in (Q16, Q61, 2):
        for num, den in MDR_PAIRS:
            out = torch.empty((len(rows), n), dtype=torch.int64, device="cuda").fill_(POISON)
            B._check(L.fhe_mul_div_round_dev(q, n, dv.data_ptr(), num, den, out.data_ptr(), len(rows), None))
            want = _arr([BN.mul_div_round_fold(q, n, r, num, den) for r in rows])
            got = out.cpu().numpy().view(np.uint64)
            assert np.array_equal(got, want), (q, num, den, np.argwhere(got != want)[:4].tolist())
    # the planted quotients are what they are meant to be
    assert BN.mul_div_round(Q61, 1 << 40, 1, 1 << 40) == I64_MAX % Q61 and BN.mul_div_round(Q61, 1 << 40, 1, -(1 << 40)) == I64_MIN % Q61
    assert BN.mul_div_round(Q16, 1, 2, 5) == 3 and BN.mul_div_round(Q16, 1, 2, -5) == Q16 - 3 and BN.mul_div_round(Q16, 1, 1 << 62, 7) == 0
