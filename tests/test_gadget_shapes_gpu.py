"""The gadget kernels of digit32.hip at every launch class (tests/test_gadget_shapes_cpu.py: ring size, step split,
partial step, short last part, T < W, ragged tail, batch either side of every split threshold), word for word against
G.external_product_rows (digit rows against key rows through the C oracle's schoolbook tn_mul).

Each (n, b, l) of the case list builds a few distinct rows, computes every reference once, and tiles the rows into each
batch on the device, so every one of the `batch` output rows is compared (torch.equal on the device, after the output was
poisoned).  The three entry points run at every batch: fhe_tggsw_gadget_external_product_dev (SRC32_GADGET),
fhe_tfhe_gadget_blind_rotation_dev with n_lwe = 1 and 2 (SRC32_GCMUX) and fhe_tggsw_gadget_cmux_dev (SRC32_GSEL).  The
batches of one (n, b, l) run descending then ascending on one stream, so that workspace slot 1 is reused under a smaller,
then a larger `parts` with the previous call's partial sums in it; the first (n, b, l) of every n runs on a stream of its
own, under the kernel timer.

Distinct rows: 6 while n l <= 8192, 2 beyond (the reference costs 16 l tn_mul per row: 31 ms each at n = 4096 on a
slow core).  Measured on an MI355X box (references on 8 threads): 1.3 s at n = 256, 0.6 s at 512, 1.3 s at 1024, 2.3 s at
2048 and 7.8 s at 4096, of which all but 0.1 - 0.3 s is the reference; 16 s for the whole module (TIMES below)."""
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _gadget_numpy as G
import _gates_numpy as GN
import _tfhe_numpy as R
import test_gadget_shapes_cpu as S
from test_bootstrap_gpu import _dev, _edge_lwe, _rand_dev, _u64
from test_crt_bounds import _ran
from test_gadget_cpu import _edge_words

pytestmark = pytest.mark.gpu

ROWS_CUT = 8192                 # n l above this: 2 distinct rows instead of 6
POISON = 0x5A5A5A5A5A5A5A5A
COUNT = 3                       # prepared keys: the product uses key 0, the blind rotation keys 0 and 1, the CMux all three
_POOL = ThreadPoolExecutor(8)   # tn_mul runs outside the interpreter lock


def _mul(oracle, n):
    def mul(x, y):
        step = max(1, -(-len(x) // 32))
        jobs = [_POOL.submit(oracle.tn_mul, n, x[i:i + step], y[i:i + step]) for i in range(0, len(x), step)]
        return np.concatenate([j.result() for j in jobs])
    return mul


def _tile(batch, d):
    """the distinct row of every batch row: stride 5 with a slip of one every 7 rows — coprime to 2 and 6 distinct rows,
    and in no fixed phase with any power-of-two packing of rows into workgroups (2 .. 16 units)"""
    r = np.arange(batch)
    return (r * 5 + r // 7) % d


class _Group:
    """the data and references of one (n, b, l): everything the batch ladder and the three modes share"""

    def __init__(self, pkg, oracle, n, b, l, worst=False):
        import torch

        L, B = pkg.load_library(), pkg.binding
        self.n, self.b, self.l, self.L, self.B = n, b, l, L, B
        d = self.d = 1 if worst else 6 if n * l <= ROWS_CUT else 2
        seed = n * 10007 + b * 101 + l
        rng = np.random.default_rng(seed)
        edges = _edge_words(b, l)
        if worst:                                                         # every key word 2^64 - 1, every digit -2^(b-1)
            dkeys = torch.full((COUNT, 2, l, 2, n), -1, dtype=torch.int64, device="cuda")
            rows = np.full((1, 2, n), edges[5], dtype=np.uint64)
        else:
            dkeys = _rand_dev((COUNT, 2, l, 2, n), seed)
            rows = rng.integers(0, 1 << 64, (d, 2, n), dtype=np.uint64, endpoint=False)
            rows[0, 0, : len(edges)] = edges
            rows[0, 1, n - len(edges):] = edges
            rows[1] = np.uint64(edges[5])                                 # every digit -2^(b-1)
        assert np.all(G.decompose(rows[-1 if worst else 1, 0, :1], b, l) == -(1 << (b - 1)))
        keys = _u64(dkeys)
        self.w = L.fhe_tggsw_gadget_prepared_words(n, 1, b, l)
        assert self.w == 2 * 2 * l * 2 * n
        self.prep = torch.empty(COUNT * self.w, dtype=torch.int64, device="cuda")
        B._check(L.fhe_tggsw_gadget_prepare_many_dev(n, 1, b, l, COUNT, dkeys.data_ptr(), self.prep.data_ptr(), None))
        mul = _mul(oracle, n)
        memo = {}

        def prod(j, x):
            key = (j, x.tobytes())
            if key not in memo:
                memo[key] = G.external_product_rows(mul, keys[j], x, b)
            return memo[key]

        self.rows = _dev(rows)
        want = prod(0, rows)
        if worst:       # coefficient N-1 has no wrapped terms: 2 l N products (-1) (-2^(b-1))
            assert np.all(want[:, :, n - 1] == np.uint64(2 * l * n * (1 << (b - 1))))
        self.want_prod = _dev(want)
        # CMux with a selector per row: c1 - c0 = the rows above; distinct row i goes to key SEL[i]
        c0 = rng.integers(0, 1 << 64, (d, 2, n), dtype=np.uint64, endpoint=False)
        self.sel = np.array([1, 2, 0, 1, 2, 0][:d], dtype=np.int32)
        self.c0, self.c1 = _dev(c0), _dev(c0 + rows)
        self.want_sel = _dev(c0 + np.concatenate([prod(int(self.sel[i]), rows[i:i + 1]) for i in range(d)]))
        self.dsel = torch.from_numpy(self.sel).cuda()
        # blind rotation, n_lwe = 1 and 2: each distinct row its own shifts, 0, N and 2N - 1 among them
        self.want_br = {}
        if not worst:
            lg = n.bit_length() - 1
            e = [0, 1 << 63, 1 << (62 - lg), int(rng.integers(0, 1 << 63)) * 2 + 1, (2 * n - 1) << (63 - lg), (1 << (62 - lg)) - 1]
            lwe = rng.integers(0, 1 << 64, (d, 3), dtype=np.uint64, endpoint=False)
            if d == 6:
                lwe[:, 0], lwe[:, 1] = np.array(e, dtype=np.uint64), np.array(e[3:] + e[:3], dtype=np.uint64)
                lwe[0, 2], lwe[1, 2] = (1 << 64) - 1, 0                    # the body: rounds to 2N = 0; 0
            else:
                lwe[:, 0], lwe[:, 1] = np.array([e[1], e[0]], dtype=np.uint64), np.array([e[2], e[4]], dtype=np.uint64)
            shifts = {int((2 * n - x) % (2 * n)) for x in R.mod_switch(lwe[:, :2], n).reshape(-1)}
            assert {0, n, 2 * n - 1} <= shifts
            table = rng.integers(0, 1 << 64, (2, n), dtype=np.uint64, endpoint=False)
            self.table = _dev(table)
            self.lwe = {1: _dev(lwe[:, [0, 2]]), 2: _dev(lwe)}
            for n_lwe, x in ((1, lwe[:, [0, 2]]), (2, lwe)):              # step 0 of the second is the first's (memo)
                self.want_br[n_lwe] = _dev(R.blind_rotation(prod, n, 1, l, None, table, x))
        torch.cuda.synchronize()

    def run(self, batch, st, bad):
        """the three entry points at one batch on stream st (the current torch stream); mismatches are appended to bad"""
        import torch

        n, b, l, L, B = self.n, self.b, self.l, self.L, self.B
        idx = torch.from_numpy(_tile(batch, self.d)).cuda()
        out = torch.empty((batch, 2, n), dtype=torch.int64, device="cuda")

        def check(mode, want):
            eq = (out == want).reshape(batch, -1).all(dim=1)
            if not bool(eq.all()):
                rows = torch.nonzero(~eq).reshape(-1)
                bad.append((n, b, l, batch, mode, int(rows.numel()), int(rows[0]), S.launch_shape(n, l, batch)))

        ct = self.rows[idx]
        out.fill_(POISON)
        B._check(L.fhe_tggsw_gadget_external_product_dev(n, 1, b, l, self.prep.data_ptr(), ct.data_ptr(), out.data_ptr(), batch, st))
        check("gadget", self.want_prod[idx])
        for n_lwe, want in self.want_br.items():
            lwe = self.lwe[n_lwe][idx]
            out.fill_(POISON)
            B._check(L.fhe_tfhe_gadget_blind_rotation_dev(n, 1, b, l, n_lwe, self.prep.data_ptr(), self.table.data_ptr(), lwe.data_ptr(),
                                                          out.data_ptr(), batch, st))
            check("gcmux n_lwe=%d" % n_lwe, want[idx])
        c0, c1, sel, want = self.c0[idx], self.c1[idx], self.dsel[idx], self.want_sel[idx]
        if batch >= 2:                                                     # one selector out of range: that row is c0
            sel[batch // 2] = COUNT
            want[batch // 2] = c0[batch // 2]
        out.fill_(POISON)
        B._check(L.fhe_tggsw_gadget_cmux_dev(n, 1, b, l, COUNT, self.prep.data_ptr(), sel.data_ptr(), c0.data_ptr(), c1.data_ptr(),
                                             out.data_ptr(), batch, st))
        check("gsel", want)


def _ladder(batches):
    """descending, then ascending again"""
    down = sorted(set(batches), reverse=True)
    return down + down[-2::-1]


# measured wall seconds per n, rounded up (module docstring).  pytest.mark.timeout is twice that, with a floor of 120 s:
# nearly all of it is the schoolbook reference on the host, and a core six times slower than the measured one is common
TIMES = {256: 2, 512: 1, 1024: 2, 2048: 3, 4096: 8}


def _sweep(pkg, oracle, n):
    import torch

    B = pkg.binding
    groups = {}
    for nn, b, l, batch in S.CASES:
        if nn == n:
            groups.setdefault((b, l), []).append(batch)
    bad, names = [], set()
    t_ref, t0, rows = 0.0, time.time(), 0
    for i, ((b, l), batches) in enumerate(groups.items()):
        t = time.time()
        g = _Group(pkg, oracle, n, b, l)
        t_ref += time.time() - t
        rows += sum(_ladder(batches))
        if i == 0:                                                         # a stream of its own, under the kernel timer
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                names = _ran(B, lambda: [g.run(batch, side.cuda_stream, bad) for batch in _ladder(batches)])
            torch.cuda.synchronize()
            B._check(pkg.load_library().fhe_ntt_release_stream_workspace(side.cuda_stream))
        else:
            for batch in _ladder(batches):
                g.run(batch, None, bad)
        del g
    for nn, b, l in S.WORST:
        if nn == n:
            g = _Group(pkg, oracle, n, b, l, worst=True)
            for batch in (3, 1):
                g.run(batch, None, bad)
    print("\nn = %d: %d (b, l), %d batch rows through each of 4 calls, references %.1f s, all %.1f s"
          % (n, len(groups), rows, t_ref, time.time() - t0))
    lg = n.bit_length() - 1
    for fam in ("digit_mac32_gadget", "digit_mac32_gcmux", "digit_mac32_gsel", "digit_tail32", "digit_tail32_cmux", "digit_tail32_sel"):
        assert f"{fam}_{lg}" in names, (fam, lg, sorted(names))
    for row in bad:
        print("MISMATCH n=%d b=%d l=%d batch=%d %s: %d rows, first %d, %s" % row)
    assert not bad, "%d of the calls gave wrong words; the first: %r" % (len(bad), bad[0])


@pytest.mark.parametrize("n", [pytest.param(n, marks=pytest.mark.timeout(max(120, 2 * TIMES[n]))) for n in S.SIZES])
def test_sweep(pkg, oracle, n):
    _sweep(pkg, oracle, n)


@pytest.mark.timeout(600)
def test_gate_bootstraps_of_two_splits_on_two_streams_from_two_threads(pkg):
    """N = 1024, BSK (8, 3): T = 6 is two parts at batch 700 and one part at batch 1100.  Both run at once, each on its own
    stream from its own host thread, several times with no synchronisation between them: the words of the serial calls"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, n_lwe, b, l, ks_b, ks_l, wires = 1024, 16, 8, 3, 4, 4, 23
    assert S.ext32_gadget_split(n, 700, 2 * l)[0] == 2 and S.ext32_gadget_split(n, 1100, 2 * l)[0] == 1
    rng = np.random.default_rng(77)
    bsk = _rand_dev((n_lwe, 2, l, 2, n), 78)
    prep = torch.empty(L.fhe_tfhe_gadget_bsk_prepared_words(n, 1, b, l, n_lwe), dtype=torch.int64, device="cuda")
    B._check(L.fhe_tfhe_gadget_bsk_prepare_dev(n, 1, b, l, n_lwe, bsk.data_ptr(), prep.data_ptr(), None))
    ksk = _rand_dev((n, ks_l, n_lwe + 1), 79)
    pool = _dev(_edge_lwe(rng, wires, n_lwe, n))
    jobs = []
    for batch in (700, 1100):
        desc = np.stack([rng.integers(0, GN.COUNT, batch), rng.integers(0, wires, batch), rng.integers(0, wires, batch)], axis=1)
        dd = torch.from_numpy(desc.astype(np.uint32).view(np.int32)).cuda()
        jobs.append(dict(batch=batch, desc=dd, out=torch.empty((batch, n_lwe + 1), dtype=torch.int64, device="cuda"),
                         stream=torch.cuda.Stream()))

    def call(j, st):
        return L.fhe_tfhe_gate_bootstrap_dev(n, 1, b, l, n_lwe, prep.data_ptr(), ks_b, ks_l, ksk.data_ptr(), pool.data_ptr(), wires,
                                             j["desc"].data_ptr(), j["out"].data_ptr(), j["batch"], st)

    for j in jobs:                                                         # the serial words, on the default stream
        B._check(call(j, None))
        torch.cuda.synchronize()
        j["want"] = _u64(j["out"])
        j["out"].fill_(POISON)
    assert not np.array_equal(jobs[0]["want"][:8], jobs[1]["want"][:8])
    torch.cuda.synchronize()
    codes = []

    def worker(j):
        for _ in range(4):
            codes.append(call(j, j["stream"].cuda_stream))

    threads = [threading.Thread(target=worker, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert codes == [B.FHE_OK] * 8
    for j in jobs:
        assert np.array_equal(_u64(j["out"]), j["want"]), j["batch"]


@pytest.mark.timeout(600)
def test_more_prepared_keys_than_one_launch_takes(pkg, oracle):
    """fhe_tggsw_gadget_prepare_many_dev with 65535 + 3 keys (n = 256, (b, l) = (8, 1)): launch_key32_many_lp's second
    chunk.  Keys 0, 65534, 65535, 65536 and the last are prepared as fhe_tggsw_gadget_prepare_dev prepares them alone, and
    a CMux whose selectors point at exactly those keys gives c0 + the reference product of c1 - c0"""
    import torch

    L, B = pkg.load_library(), pkg.binding
    n, b, l, count = 256, 8, 1, 65535 + 3
    w = L.fhe_tggsw_gadget_prepared_words(n, 1, b, l)
    keys = _rand_dev((count, 2, l, 2, n), 4242)
    prep = torch.empty(count * w, dtype=torch.int64, device="cuda")
    prep.fill_(POISON)
    B._check(L.fhe_tggsw_gadget_prepare_many_dev(n, 1, b, l, count, keys.data_ptr(), prep.data_ptr(), None))
    picks = [0, 65534, 65535, 65536, count - 1]
    one = torch.empty(w, dtype=torch.int64, device="cuda")
    for i in picks:
        B._check(L.fhe_tggsw_gadget_prepare_dev(n, 1, b, l, keys[i].data_ptr(), one.data_ptr(), None))
        assert torch.equal(prep[i * w:(i + 1) * w], one), i
    assert not torch.equal(prep[65535 * w:65536 * w], prep[65534 * w:65535 * w])
    rng = np.random.default_rng(65538)
    batch = 7
    sel = np.array(picks + [count, 65535], dtype=np.uint32)                # one past the end: c0
    c0 = rng.integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    c1 = rng.integers(0, 1 << 64, (batch, 2, n), dtype=np.uint64, endpoint=False)
    c1[0, 0, : len(_edge_words(b, l))] = c0[0, 0, : len(_edge_words(b, l))] + np.array(_edge_words(b, l), dtype=np.uint64)
    out = torch.empty((batch, 2, n), dtype=torch.int64, device="cuda")
    ds, d0, d1 = torch.from_numpy(sel.view(np.int32)).cuda(), _dev(c0), _dev(c1)
    B._check(L.fhe_tggsw_gadget_cmux_dev(n, 1, b, l, count, prep.data_ptr(), ds.data_ptr(), d0.data_ptr(), d1.data_ptr(), out.data_ptr(),
                                         batch, None))
    mul = _mul(oracle, n)
    want = c0.copy()
    for r, s in enumerate(sel):
        if s < count:
            want[r] += G.external_product_rows(mul, _u64(keys[int(s)]), (c1 - c0)[r:r + 1], b)[0]
    assert np.array_equal(_u64(out), want)
