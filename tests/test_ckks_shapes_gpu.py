"""The CKKS evaluator on the device (ckks_eval.hip) at every ring size, depth, alignment and chunk: the
case lists of tests/_ckks_shapes_cases.py, which tests/test_ckks_shapes_cpu.py proves, word for word against the existing
restatements (tests/_ckks_eval_numpy.py and the modules on it).  Every comparison is exact equality of integer words.

    A  test_ladder            every n = 2^1 .. 2^16: from_i64, tensor, relinearise, mul, rescale, the relinearisation one level
                              down, galois_evals, galois_dev (two elements hoisted), diag_sum, bsgs, lincomb, dot, edge residues
                              planted; the keys are the samplers' up to n = 2^13 (and the device's keys are compared with
                              them) and uniform words above; the kernel timer shows the transforms of that log_n and no other
    B  test_depth             n = 256, three orders of the wide chain, k = 1 .. 8, and limbs = 1 .. 7 against a key of 8 limbs:
                              relinearise, Galois, diag sum, bsgs and dot, on a created stream
    C  test_alignment         every entry point with every buffer, the inputs or the outputs one word past a 16-byte boundary:
                              the words, the inputs unchanged, the sentinels either side of every output untouched
       test_staged_from_i64   (4096, 2, 129) into a misaligned output: two chunks, two ckks_rns_lift launches
    D  test_chunk_clamp       (2^16, 6, 2): relinearise and one Galois element in two chunks of one ciphertext
    E  test_workspace_reuse, test_two_streams_interleaved

The rescale's chunk, 2^21 / (n k), clamps only from n = 2^19 on (two 4 MiB rows a limb, a transform of 2^19 points in the
restatement): no test here reaches it, and none pretends to.

Measured on an MI355X box (pytest --durations, restatement included): the ladder 0.03 - 0.18 s a case up to n = 1024, 0.2 - 0.5 s
at 2048 .. 8192, 0.4 s at 2^14, 0.9 s at 2^15, 2.0 s at 2^16; 2.1 s for whichever test runs first, which loads the library and
the device; a depth case 0.01 - 0.12 s (3.1 s for all 31); an alignment case 0.11 s at most (1.6 s for all 108); the staged
from_i64 0.05 s; the clamp case 0.9 s (0.7 s of it the restatement, so no thread pool is used); the two stream tests 0.04 s and
0.15 s; 13.5 s for the whole module.  The sampled keys cost 0.15 s of a case at n = 2^13, k = 3; one key of k = 2 takes the
restatement 0.2 s at 2^14 and 0.8 s at 2^16 on a host core, two of them as much as the rest of that case, which is why
S.KEY_CUT stands at 2^13.

No call of the sweep gave a wrong word, and every transform row the kernel timer showed was the one predicted."""
import numpy as np
import pytest

import _ckks_bsgs_numpy as BN
import _ckks_dot_numpy as DN
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_linear_numpy as LN
import _ckks_numpy as K
import _ckks_poly_numpy as PN
import _ckks_shapes_cases as S
import _client_numpy as C
from test_client_alignment_gpu import Offset

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
SEED = bytes((19 * i + 11) % 256 for i in range(32))


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


@pytest.fixture(scope="module")
def stream():
    import torch

    return torch.cuda.Stream()


class Dev:
    """The entry points over one chain.  Every buffer is an Offset: an input holds its words one word past a 16-byte boundary
    where `mis_in` (on one otherwise), an output likewise under `mis_out`, between sentinel words either way.  take() waits for
    the stream, checks the sentinels of the output, and that every input of the call still holds its words."""

    def __init__(self, pkg, mods, P, n, mis_in=False, mis_out=False, stream=None):
        self.B, self.mods, self.P, self.n = pkg.binding, list(mods), P, n
        self.plans, self.sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
        self.mis_in, self.mis_out, self.stream = mis_in, mis_out, stream
        self.st = None if stream is None else stream.cuda_stream
        self.ins = []

    def inp(self, x):
        x = np.ascontiguousarray(x, dtype=U64)
        o = Offset(x.shape, x, lead=1 if self.mis_in else 2)
        self.ins.append((o, x))
        return o

    def out(self, shape):
        return Offset(tuple(shape), lead=1 if self.mis_out else 2)

    def ready(self):
        """the copies into the buffers ran on the default stream: they end before a call on another stream starts"""
        import torch

        if self.stream is not None:
            torch.cuda.synchronize()

    def take(self, o):
        import torch

        (self.stream or torch.cuda).synchronize()
        got = o.get().copy()
        for d, x in self.ins:
            assert np.array_equal(d.get(), x), "an input was written"
        self.ins = []
        return got

    # -- the entry points: host arrays in, host array out ---------------------------------------------------------------------------
    def from_i64(self, m, k=None):
        k = k or len(self.plans)
        d, o = self.inp(m.view(U64)), self.out((k,) + m.shape)
        self.ready()
        self.B.ckks_rns_from_i64_dev(self.plans[:k], d.ptr, o.ptr, m.shape[0], stream=self.st)
        return self.take(o)

    def secret(self):
        """[k + 1][n] residues of the ternary secret, made on the device"""
        import torch

        d_s = torch.zeros((len(self.plans) + 1, self.n), dtype=torch.int64, device="cuda")
        for i, p in enumerate(self.plans + [self.sp]):
            self.B.ckks_secret_key_dev(p, SEED, 0, d_s[i].data_ptr())
        torch.cuda.synchronize()
        return d_s.cpu().numpy().view(U64)

    def switch_key(self, tab, row, s_res, g=None):
        k = len(self.plans)
        d_s, d_t, o = self.inp(s_res), self.inp(tab), self.out((k, k + 1, 2, self.n))
        self.ready()
        if g is None:
            self.B.ckks_rns_relin_key_dev(self.plans, self.sp, SEED, row, d_s.ptr, d_t.ptr, len(tab), o.ptr, stream=self.st)
        else:
            self.B.ckks_rns_galois_key_dev(self.plans, self.sp, SEED, row, g, d_s.ptr, d_t.ptr, len(tab), o.ptr, stream=self.st)
        return self.take(o)

    def tensor(self, a, b):
        k, _, batch, n = a.shape
        da, db, o = self.inp(a), self.inp(b), self.out((k, 3, batch, n))
        self.ready()
        self.B.ckks_rns_tensor_dev(self.plans[:k], da.ptr, db.ptr, o.ptr, batch, stream=self.st)
        return self.take(o)

    def relinearize(self, rlk, d):
        k, _, batch, n = d.shape
        dk, dd, o = self.inp(rlk), self.inp(d), self.out((k, 2, batch, n))
        self.ready()
        self.B.ckks_rns_relinearize_dev(self.plans[:k], self.sp, dk.ptr, rlk.shape[0], dd.ptr, o.ptr, batch, stream=self.st)
        return self.take(o)

    def mul(self, rlk, a, b):
        k, _, batch, n = a.shape
        dk, da, db, o = self.inp(rlk), self.inp(a), self.inp(b), self.out(a.shape)
        self.ready()
        self.B.ckks_rns_mul_dev(self.plans[:k], self.sp, dk.ptr, rlk.shape[0], da.ptr, db.ptr, o.ptr, batch, stream=self.st)
        return self.take(o)

    def rescale(self, c):
        k, _, batch, n = c.shape
        dc, o = self.inp(c), self.out((k - 1, 2, batch, n))
        self.ready()
        self.B.ckks_rns_rescale_dev(self.plans[:k], dc.ptr, o.ptr, batch, stream=self.st)
        return self.take(o)

    def galois_evals(self, ct, g):
        """a limb's slab of 2 batch rows a call"""
        k, _, batch, n = ct.shape
        dc, o = self.inp(ct), self.out(ct.shape)
        self.ready()
        for i in range(k):
            self.B.ckks_galois_evals_dev(self.plans[i], g, dc.ptr + i * 2 * batch * n * 8, o.ptr + i * 2 * batch * n * 8, 2 * batch, stream=self.st)
        return self.take(o)

    def _keys(self, keys):
        return [None if x is None else self.inp(x) for x in keys]

    def galois(self, gks, gs, ct):
        k, _, batch, n = ct.shape
        dk, dc, o = self._keys(gks), self.inp(ct), self.out((len(gs),) + ct.shape)
        self.ready()
        self.B.ckks_rns_galois_dev(self.plans[:k], self.sp, [x.ptr for x in dk], gs, gks[0].shape[0], dc.ptr, o.ptr, batch, stream=self.st)
        return self.take(o)

    def diag_sum(self, gks, gs, kl, pts, ct):
        k, _, batch, n = ct.shape
        dk, dp, dc, o = self._keys(gks), self.inp(pts), self.inp(ct), self.out((pts.shape[0],) + ct.shape)
        self.ready()
        self.B.ckks_rns_diag_sum_dev(self.plans[:k], self.sp, [x and x.ptr for x in dk], gs, kl, dp.ptr, pts.shape[0], dc.ptr, o.ptr, batch, stream=self.st)
        return self.take(o)

    def bsgs(self, bks, bgs, gks, ggs, kl, pts, ct, wait=True):
        k, _, batch, n = ct.shape
        db, dg, dp, dc, o = self._keys(bks), self._keys(gks), self.inp(pts), self.inp(ct), self.out(ct.shape)
        self.ready()
        self.B.ckks_rns_bsgs_dev(self.plans[:k], self.sp, [x and x.ptr for x in db], bgs, [x and x.ptr for x in dg], ggs, kl, dp.ptr, dc.ptr, o.ptr, batch,
                                 stream=self.st)
        return self.take(o) if wait else o

    def lincomb(self, cts, w, kk):
        k, _, batch, n = cts[0].shape
        dc, o = [self.inp(c) for c in cts], self.out((len(w),) + cts[0].shape)
        self.ready()
        self.B.ckks_rns_lincomb_dev(self.plans[:k], [x.ptr for x in dc], PN.flat(w), PN.flat(kk), len(w), o.ptr, batch, stream=self.st)
        return self.take(o)

    def dot(self, rlk, pairs, w):
        k, _, batch, n = pairs[0][0].shape
        dk, o = self.inp(rlk), self.out(pairs[0][0].shape)
        das, dbs = [self.inp(a) for a, _ in pairs], [self.inp(b) for _, b in pairs]
        self.ready()
        self.B.ckks_rns_dot_dev(self.plans[:k], self.sp, dk.ptr, rlk.shape[0], [x.ptr for x in das], [x.ptr for x in dbs], DN.flat(w), o.ptr, batch, stream=self.st)
        return self.take(o)


def _timed(B, fn):
    """-> (fn's result, {kernel-timer row: launches})"""
    import torch

    torch.cuda.synchronize()
    B.kernel_timing_enable(True)
    B.kernel_timing_reset()
    try:
        res = fn()
        torch.cuda.synchronize()
        got = B.kernel_timing_read(256)
    finally:
        B.kernel_timing_enable(False)
    return res, {name: c for name, (_, c) in got.items()}


def _count(rows, label):
    return sum(c for name, c in rows.items() if name.startswith(label))


class Data:
    """the inputs of one (chain, n, limbs, batch) and, computed on first use, the restatement's words of every entry point"""

    def __init__(self, mods, P, n, k, batch, rng, kl=None, keys=None):
        self.mods, self.P, self.n, self.k, self.batch = list(mods[:k]), P, n, k, batch
        kl = kl or k
        full = list(mods[:kl])
        self.a, self.b = S.planted_ct(self.mods, n, batch, 2, rng), E.case_ct(self.mods, n, batch, 2, rng + 1)
        self.d = S.planted_ct(self.mods, n, batch, 3, rng + 2)
        self.gs = S.galois_pair(n)
        self.diag, self.babies, self.giants = S.reduced(S.DIAG, n), S.reduced(S.BABIES, n), S.reduced(S.GIANTS, n)
        keys = keys or {}
        self.rlk = keys.get("rlk", None)
        if self.rlk is None:
            self.rlk = S.random_key(full, P, n, rng + 3)
        self.gk = {}
        for t, g in enumerate(sorted(set(self.gs + self.diag + self.babies + self.giants))):
            self.gk[g] = keys[g] if g in keys else S.random_key(full, P, n, rng + 10 + t)
        self.kl = kl
        self.diag_pts = LN.random_pts(self.mods, P, n, 1, len(self.diag), rng + 4)
        self.bsgs_pts = LN.random_pts(self.mods, P, n, len(self.giants), len(self.babies), rng + 5)
        self.w_lin, self.k_lin = S.weights(self.mods, (2, 2), rng + 6), S.weights(self.mods, (2,), rng + 7)
        self.w_dot = S.weights(self.mods, (2,), rng + 8)
        self.m = S.signed_rows(n, k, batch)
        self._want = {}

    def keys_of(self, gs):
        return [None if g == 1 else self.gk[g] for g in gs]

    def want(self, what):
        if what not in self._want:
            self._want[what] = getattr(self, "_" + what)()
        return self._want[what]

    def _from_i64(self):
        return E.from_i64(self.mods, self.n, self.m)

    def _tensor(self):
        return E.tensor(self.mods, self.a, self.b)

    def _relinearize(self):
        return E.relinearize(self.mods, self.P, self.rlk, self.d)

    def _mul(self):
        return E.relinearize(self.mods, self.P, self.rlk, self.want("tensor"))

    def _rescale(self):
        return E.rescale(self.mods, self.a)

    def _galois_evals(self):
        return G.galois_evals(self.a, self.gs[0])

    def _galois(self):
        return np.stack([G.apply_galois(self.mods, self.P, self.gk[g], self.a, g) for g in self.gs])

    def _diag_sum(self):
        return LN.diag_sum(self.mods, self.P, self.keys_of(self.diag), self.diag, self.diag_pts, self.a)

    def _bsgs(self):
        return BN.bsgs(self.mods, self.P, self.keys_of(self.babies), self.babies, self.keys_of(self.giants), self.giants, self.bsgs_pts, self.a)

    def _lincomb(self):
        return PN.lincomb(self.mods, [self.a, self.b], self.w_lin, self.k_lin)

    def _dot(self):
        return DN.dot(self.mods, self.P, self.rlk, [(self.a, self.b), (self.b, self.b)], self.w_dot)

    # -- the device's side of the same entries ------------------------------------------------------------------------------------
    def run(self, dev, what):
        if what == "from_i64":
            return dev.from_i64(self.m, self.k)
        if what == "tensor":
            return dev.tensor(self.a, self.b)
        if what == "relinearize":
            return dev.relinearize(self.rlk, self.d)
        if what == "mul":
            return dev.mul(self.rlk, self.a, self.b)
        if what == "rescale":
            return dev.rescale(self.a)
        if what == "galois_evals":
            return dev.galois_evals(self.a, self.gs[0])
        if what == "galois":
            return dev.galois([self.gk[g] for g in self.gs], self.gs, self.a)
        if what == "diag_sum":
            return dev.diag_sum(self.keys_of(self.diag), self.diag, self.kl, self.diag_pts, self.a)
        if what == "bsgs":
            return dev.bsgs(self.keys_of(self.babies), self.babies, self.keys_of(self.giants), self.giants, self.kl, self.bsgs_pts, self.a)
        if what == "lincomb":
            return dev.lincomb([self.a, self.b], self.w_lin, self.k_lin)
        assert what == "dot"
        return dev.dot(self.rlk, [(self.a, self.b), (self.b, self.b)], self.w_dot)

    def check(self, dev, what):
        got = self.run(dev, what)
        want = self.want(what)
        assert got.shape == want.shape and np.array_equal(got, want), (what, self.n, self.k, self.batch, int((got != want).sum()))


SWITCHES = ("relinearize", "galois", "diag_sum", "bsgs", "dot")
EVERY = ("from_i64", "tensor", "relinearize", "mul", "rescale", "galois_evals", "galois", "diag_sum", "bsgs", "lincomb", "dot")


def _sampled_keys(dev, tab, mods, P, n):
    """the relinearisation key and the key of the first element with one, from the samplers; the device's keys are compared with
    them word for word"""
    s = K.secret_key(SEED, 0, n)
    s_res = dev.secret()
    assert np.array_equal(s_res, np.stack([E.residues(s, q) for q in list(mods) + [P]]))
    g = [x for x in S.galois_pair(n) if x != 1][0]
    keys = {"rlk": E.relin_key(SEED, E.RLK_BASE + 64 * 7, s, mods, P, tab), g: G.galois_key(SEED, G.GK_BASE + 64 * 9, s, mods, P, tab, g)}
    assert np.array_equal(dev.switch_key(tab, E.RLK_BASE + 64 * 7, s_res), keys["rlk"])
    assert np.array_equal(dev.switch_key(tab, G.GK_BASE + 64 * 9, s_res, g), keys[g])
    return keys


# ---- A: the ring-size ladder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch", S.LADDER)
def test_ladder(pkg, tab, n, k, batch):
    mods, P = E.chain(n, *S.SPEC, k - 1)
    dev = Dev(pkg, mods, P, n)
    keys = _sampled_keys(dev, tab, mods, P, n) if n <= S.KEY_CUT else None
    data = Data(mods, P, n, k, batch, 7000 + 10 * n + k, keys=keys)
    low = Data(mods, P, n, k - 1, batch, 7000 + 10 * n + k, kl=k, keys={"rlk": data.rlk})

    def run():
        for what in EVERY:
            data.check(dev, what)
        low.check(dev, "relinearize")                                        # the key of the whole chain one level down
    _, rows = _timed(pkg.binding, run)
    L = n.bit_length() - 1
    assert {name for name in rows if name.startswith("ntt_")} == S.transform_names(n), sorted(rows)
    assert all(name.endswith("_%d" % L) for name in rows if name.startswith("ckks_rns_")), sorted(rows)


# ---- B: depth and the place of the wide limb, on a created stream ------------------------------------------------------------------------
@pytest.mark.parametrize("order,k,kl", S.DEPTH + S.DEPTH_LOW)
def test_depth(pkg, stream, order, k, kl):
    mods, P, wide = S.ordered_chain(order)
    n, batch = S.N_DEPTH, S.BATCH_DEPTH
    dev = Dev(pkg, mods[:k], P, n, stream=stream)
    data = Data(mods, P, n, k, batch, 8000 + 100 * S.ORDERS.index(order) + 10 * k + kl, kl=kl)
    assert data.rlk.shape[0] == kl and (wide < k) == any(q >> 62 for q in data.mods)
    for what in SWITCHES:
        data.check(dev, what)


# ---- C: buffers 8-byte but not 16-byte aligned -------------------------------------------------------------------------------------------
_ALIGN = {}


def _align_data(pkg, tab, n, k, batch):
    if (n, k, batch) not in _ALIGN:
        mods, P = E.chain(n, *S.SPEC, k - 1)
        s = K.secret_key(SEED, 0, n)
        data = Data(mods, P, n, k, batch, 9000 + n + k)
        data.s_res = np.stack([E.residues(s, q) for q in list(mods) + [P]])
        data.g = data.gs[0]
        data._relin_key = lambda: E.relin_key(SEED, E.RLK_BASE + 64 * 11, s, mods, P, tab)
        data._galois_key = lambda: G.galois_key(SEED, G.GK_BASE + 64 * 12, s, mods, P, tab, data.g)
        _ALIGN[n, k, batch] = data
    return _ALIGN[n, k, batch]


@pytest.mark.parametrize("what", S.ENTRIES)
@pytest.mark.parametrize("mode", S.ALIGN_MODES)
@pytest.mark.parametrize("n,k,batch", S.ALIGN_SHAPES)
def test_alignment(pkg, tab, n, k, batch, mode, what):
    data = _align_data(pkg, tab, n, k, batch)
    dev = Dev(pkg, data.mods, data.P, n, mis_in=mode != "outputs", mis_out=mode != "inputs")
    if what == "relin_key":
        got = dev.switch_key(tab, E.RLK_BASE + 64 * 11, data.s_res)
    elif what == "galois_key":
        got = dev.switch_key(tab, G.GK_BASE + 64 * 12, data.s_res, data.g)
    else:
        got = data.run(dev, what)
    assert np.array_equal(got, data.want(what)), (what, mode, n, k, batch)


def test_staged_from_i64_over_two_chunks(pkg):
    """a misaligned output takes the staged route: chunks of 128 and 1 rows, each limb of each chunk copied to its rows of the
    output; the aligned call lifts once, into the output itself"""
    n, k, batch = S.STAGED
    mods, P = E.chain(n, *S.SPEC, k - 1)
    m = S.signed_rows(n, k, batch)
    want = E.from_i64(mods, n, m)
    for mis_out, lifts in ((True, 2), (False, 1)):
        dev = Dev(pkg, mods, P, n, mis_in=mis_out, mis_out=mis_out)
        got, rows = _timed(pkg.binding, lambda: dev.from_i64(m))
        assert np.array_equal(got, want), (mis_out, np.nonzero((got != want).any(axis=(0, 2)))[0].tolist())
        assert _count(rows, "ckks_rns_lift") == lifts, (mis_out, sorted(rows.items()))


# ---- D: the chunk clamp --------------------------------------------------------------------------------------------------------------------
def test_chunk_clamp(pkg):
    n, k, batch = S.CLAMP
    mods, P = E.chain(n, *S.SPEC, k - 1)
    dev = Dev(pkg, mods, P, n)
    d = S.planted_ct(mods, n, batch, 3, 61)
    rlk, gk = S.random_key(mods, P, n, 62), S.random_key(mods, P, n, 63)
    got, rows = _timed(pkg.binding, lambda: dev.relinearize(rlk, d))
    assert np.array_equal(got, E.relinearize(mods, P, rlk, d))                # 0.7 s of restatement: no thread pool is needed
    assert (_count(rows, "ckks_rns_keymac"), _count(rows, "ckks_rns_lift"), _count(rows, "ckks_rns_divround")) == (2 * (k + 1), 2 * (k + 1), 2 * k)
    ct, g = d[:, :2].copy(), 5
    got, rows = _timed(pkg.binding, lambda: dev.galois([gk], [g], ct))
    want = G.apply_galois(mods, P, gk, ct, g)
    assert np.array_equal(got[0], want)
    assert (_count(rows, "ckks_rns_keymac_galois"), _count(rows, "ckks_rns_lift"), _count(rows, "ckks_rns_divround_galois")) == (2 * (k + 1), 2 * (k + 1), 2 * k)


# ---- E: streams and the reuse of the workspace ----------------------------------------------------------------------------------------------
def test_workspace_reuse_under_a_smaller_then_a_larger_request(pkg, stream):
    n, k, batches = S.REUSE
    mods, P = E.chain(n, *S.SPEC, k - 1)
    dev = Dev(pkg, mods, P, n, stream=stream)
    rlk = S.random_key(mods, P, n, 71)
    for batch in batches:
        d = S.planted_ct(mods, n, batch, 3, 72 + batch)
        assert np.array_equal(dev.relinearize(rlk, d), E.relinearize(mods, P, rlk, d)), batch


def test_two_streams_interleaved(pkg, stream):
    """relinearise on one stream (slot 12) and bsgs on another (slot 13, and the transforms' own), issued alternately with no
    wait between them; everything is compared at the end"""
    import torch

    B = pkg.binding
    n, k, batch, rounds = S.INTERLEAVE
    mods, P = E.chain(n, *S.SPEC, k - 1)
    one, two = Dev(pkg, mods, P, n, stream=stream), Dev(pkg, mods, P, n, stream=torch.cuda.Stream())
    datas = [Data(mods, P, n, k, batch, 9500 + 20 * r) for r in range(rounds)]
    calls = []
    for data in datas:
        relin = (one.inp(data.rlk), one.inp(data.d), one.out((k, 2, batch, n)))
        bsgs = (two._keys(data.keys_of(data.babies)), two._keys(data.keys_of(data.giants)), two.inp(data.bsgs_pts), two.inp(data.a), two.out(data.a.shape))
        calls.append((data, relin, bsgs))
    torch.cuda.synchronize()                                                 # the copies in; from here on no wait until every call is issued
    for data, (dk, dd, o1), (db, dg, dp, dc, o2) in calls:
        B.ckks_rns_relinearize_dev(one.plans, one.sp, dk.ptr, k, dd.ptr, o1.ptr, batch, stream=one.st)
        B.ckks_rns_bsgs_dev(two.plans, two.sp, [x and x.ptr for x in db], data.babies, [x and x.ptr for x in dg], data.giants, k, dp.ptr, dc.ptr, o2.ptr, batch,
                            stream=two.st)
    torch.cuda.synchronize()
    for r, (data, (_, _, o1), (_, _, _, _, o2)) in enumerate(calls):
        assert np.array_equal(o1.get(), data.want("relinearize")), r
        assert np.array_equal(o2.get(), data.want("bsgs")), r
    for d, x in one.ins + two.ins:
        assert np.array_equal(d.get(), x)
