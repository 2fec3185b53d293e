"""CKKS on the deep RNS chain on the device (ckks_deep.hip) where the tests that came with it do not reach:
the case lists of tests/_ckks_deep_shapes_cases.py, which tests/test_ckks_deep_shapes_cpu.py proves, word for word against the
restatements in Python integers (tests/_ckks_deep_numpy.py, tests/_ckks_deep_linear_numpy.py, tests/_ckks_eval_numpy.py).  Every
comparison is exact equality of 64-bit words; every device buffer sits between sentinel words, and every input is read back.

    A  test_primes_just_below_the_limit, test_mixed_chains, test_centring_decided_at_every_depth, test_modulus_down_at_every_depth
    B  test_ladder
    C  test_diag_sum_counts, test_galois_at_the_count_limit, test_launch_counts_after_two_carries, test_empty_calls_write_nothing
    D  test_key_switch_and_diag_sum_clamped, test_rescale_chunks, test_slot_14_smaller_larger_smaller, test_two_streams_interleaved
    E  test_alignment

Measured on an MI355X box (pytest --durations, restatement included): 182 cases in 28.3 s; 2.5 s the ladder at 2^16 (2.3 s of it the
restatement), 0.9 - 2.0 s the cases of (32, 1, 32) at n = 64 and batch 3 (the restatement's 32 x 33 digit transforms), 1.6 s the first
alignment case at 8192 (it computes that shape's references), 1.2 s the ladder at 2^15, under 1 s every other case.

No call of the sweep gave a wrong word."""
import time

import numpy as np
import pytest

import _ckks_deep_linear_numpy as DL
import _ckks_deep_numpy as D
import _ckks_deep_shapes_cases as S
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_numpy as K
import _ckks_shapes_cases as CS
import _client_numpy as C
from test_bfv_rns_shapes_gpu import OwnStream
from test_bootstrap_gpu import _dev, _u64
from test_ckks_shapes_gpu import _count, _timed
from test_client_alignment_gpu import Offset

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A
SEED = bytes((11 * i + 7) % 256 for i in range(32))


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _sync():
    import torch

    torch.cuda.synchronize()


def _buf(x, mis=False):
    x = np.ascontiguousarray(x, dtype=U64)
    return Offset(x.shape, x, lead=1 if mis else 2)


def _out(shape, mis=False):
    return Offset(tuple(shape), lead=1 if mis else 2)


def _same(got, want, what=""):
    assert got.shape == want.shape and np.array_equal(got, want), (what, np.argwhere(got != want)[:6].tolist())


class Dev:
    """the deep entry points over one chain.  Every buffer is an Offset between sentinels, the inputs one word past a 16-byte
    boundary where mi is set and the outputs where mo is; after the call the sentinels are intact and the inputs unchanged.
    defer: nothing is waited for, and the check is the caller's (-> the output's Offset and the inputs)"""

    def __init__(self, pkg, mods, sps, n, kl=None, stream=None, mi=False, mo=False):
        self.B, self.n, self.kl, self.stream, self.mi, self.mo = pkg.binding, n, kl or len(mods), stream, mi, mo
        self.plans, self.sp = [pkg.Plan(q, n) for q in mods], [pkg.Plan(q, n) for q in sps]

    def _st(self):
        import torch

        if self.stream is None:
            return None
        self.stream.wait_stream(torch.cuda.current_stream())             # the copies into the buffers ran on the default stream
        return self.stream.cuda_stream

    def _take(self, o, ins, defer):
        if defer:
            return o, ins
        _sync()
        for d, x in ins:
            assert np.array_equal(d.get(), x), "an input was written"
        return o.get().copy()

    def _keys(self, keys):
        """one upload per distinct key object"""
        seen = {}
        for x in keys:
            if x is not None and id(x) not in seen:
                seen[id(x)] = (_buf(x, self.mi), x)
        return [None if x is None else seen[id(x)][0].ptr for x in keys], list(seen.values())

    def relinearize(self, key, d, defer=False):
        l, _, batch, n = d.shape
        dk, dd, o = _buf(key, self.mi), _buf(d, self.mi), _out((l, 2, batch, n), self.mo)
        self.B.ckks_deep_relinearize_dev(self.plans[:l], self.sp, dk.ptr, self.kl, dd.ptr, o.ptr, batch, self._st())
        return self._take(o, [(dk, key), (dd, d)], defer)

    def mul(self, key, a, b, defer=False):
        l, batch = a.shape[0], a.shape[2]
        dk, da, db, o = _buf(key, self.mi), _buf(a, self.mi), _buf(b, self.mi), _out(a.shape, self.mo)
        self.B.ckks_deep_mul_dev(self.plans[:l], self.sp, dk.ptr, self.kl, da.ptr, db.ptr, o.ptr, batch, self._st())
        return self._take(o, [(dk, key), (da, a), (db, b)], defer)

    def galois(self, keys, gs, ct, defer=False):
        l, batch = ct.shape[0], ct.shape[2]
        ptrs, held = self._keys(keys)
        dc, o = _buf(ct, self.mi), _out((len(gs),) + ct.shape, self.mo)
        self.B.ckks_deep_galois_dev(self.plans[:l], self.sp, ptrs, list(gs), self.kl, dc.ptr, o.ptr, batch, self._st())
        return self._take(o, held + [(dc, ct)], defer)

    def diag(self, keys, gs, pts, ct, defer=False):
        l, batch = ct.shape[0], ct.shape[2]
        ptrs, held = self._keys(keys)
        dp, dc, o = _buf(pts, self.mi), _buf(ct, self.mi), _out((pts.shape[0],) + ct.shape, self.mo)
        self.B.ckks_deep_diag_sum_dev(self.plans[:l], self.sp, ptrs, list(gs), self.kl, dp.ptr, pts.shape[0], dc.ptr, o.ptr, batch, self._st())
        return self._take(o, held + [(dp, pts), (dc, ct)], defer)

    def rescale(self, ct, defer=False):
        l, _, batch, n = ct.shape
        dc, o = _buf(ct, self.mi), _out((l - 1, 2, batch, n), self.mo)
        self.B.ckks_deep_rescale_dev(self.plans[:l], dc.ptr, o.ptr, batch, self._st())
        return self._take(o, [(dc, ct)], defer)

    def switch_key(self, tab, s_res, row, g=None):
        """the relinearisation key (g None) or the Galois key of g, of the whole chain, from the secret's residues s_res"""
        L, alpha = len(self.plans), len(self.sp)
        ds, dt, o = _buf(s_res, self.mi), _buf(tab, self.mi), _out((D.dnum(L, alpha), L + alpha, 2, self.n), self.mo)
        if g is None:
            self.B.ckks_deep_relin_key_dev(self.plans, self.sp, SEED, row, ds.ptr, dt.ptr, len(tab), o.ptr, self._st())
        else:
            self.B.ckks_deep_galois_key_dev(self.plans, self.sp, SEED, row, g, ds.ptr, dt.ptr, len(tab), o.ptr, self._st())
        return self._take(o, [(ds, s_res), (dt, tab)], False)


def _secret_residues(mods, sps, n):
    s = K.secret_key(SEED, 0, n)
    return s, np.stack([E.residues(s, q) for q in list(mods) + list(sps)])


# ---- A1: every prime just below 2^62, uniform words and the bound-reaching rows ------------------------------------------------------------
@pytest.mark.parametrize("what", ["products", "moves"])
@pytest.mark.parametrize("rows", ["uniform", "bound"])
@pytest.mark.parametrize("L,alpha,l", S.LIMIT_SHAPES)
@pytest.mark.parametrize("batch", S.WIDTH_BATCHES)
@pytest.mark.parametrize("n", S.WIDTH_NS)
def test_primes_just_below_the_limit(pkg, n, batch, L, alpha, l, rows, what):
    """products: mul, relinearize of a given tensor, rescale.  moves: Galois {5, 2n - 1} in one call, diag_sum at 3 and 17 elements
    (the identity among them), two outputs.  bound: the switched component is -1 in batch row 0 and every key and plaintext word
    is m_i - 1, so every digit is m_i - 1 and every term of every sum (m_i - 1)^2 (proved by the CPU module); at (32, 1, 32) that
    is 32 such terms a sum, which wraps 2^128 under a fold schedule looser than the kernels'."""
    mods, sps = S.limit_chain(n, L, alpha)
    lm, rng, top = mods[:l], 100 * n + 10 * L + batch, rows == "bound"
    dev = Dev(pkg, mods, sps, n)
    if what == "products":
        rlk = S.top_key(mods, sps, n) if top else S.uniform_key(mods, sps, n, rng)
        a, b = S.minus_one_pair(lm, n, batch, rng + 1) if top else (E.case_ct(lm, n, batch, 2, rng + 1), E.case_ct(lm, n, batch, 2, rng + 2))
        d = S.minus_one_ct(lm, n, batch, 3, rng + 3, 2) if top else E.case_ct(lm, n, batch, 3, rng + 3)
        _same(dev.mul(rlk, a, b), D.mul(lm, sps, rlk, a, b), "mul")
        _same(dev.relinearize(rlk, d), D.relinearize(lm, sps, rlk, d), "relinearize")
        if l > 1:
            _same(dev.rescale(b), D.rescale(lm, b), "rescale")
        return
    pool = S.pool_keys(lm, sps, n, rng + 4, key_mods=mods, fill=top or None)
    ct = S.minus_one_ct(lm, n, batch, 2, rng + 5, 1) if top else E.case_ct(lm, n, batch, 2, rng + 5)
    Dg = D.digits(lm, sps, ct[:, 1])
    gs = CS.galois_pair(n)
    want = S.galois_many(lm, sps, S.keys_of(pool, gs), gs, ct, Dg)
    got = dev.galois(S.keys_of(pool, gs), gs, ct)
    for r, g in enumerate(gs):
        _same(got[r], want[r], g)
    for count in S.DIAG_COUNTS:
        gs = S.diag_elements(n, count)
        pts = S.top_pts(lm, sps, n, S.DIAG_OUTPUTS, count) if top else DL.random_pts(lm, sps, n, S.DIAG_OUTPUTS, count, rng + count)
        _same(dev.diag(S.keys_of(pool, gs), gs, pts, ct), DL.diag_sum(lm, sps, S.keys_of(pool, gs), gs, pts, ct), count)


# ---- A3: mixed widths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", S.MIXED_ORDERS)
@pytest.mark.parametrize("alpha", S.MIXED_ALPHAS)
@pytest.mark.parametrize("batch", S.WIDTH_BATCHES)
@pytest.mark.parametrize("n", S.WIDTH_NS)
def test_mixed_chains(pkg, n, batch, alpha, order):
    """a 30-bit prime beside 37, 61 and 62-bit ones inside a digit group, small before large and large before small (where the
    Garner digits reduce a 62-bit digit modulo a 30-bit source); the whole chain and one level below a full group"""
    mods, sps = S.mixed_chain(n, alpha, order)
    L, rng = len(mods), 200 * n + 10 * alpha + batch
    dev = Dev(pkg, mods, sps, n)
    rlk, pool = S.uniform_key(mods, sps, n, rng), None
    for l in (L, 2 * alpha - 1):
        lm = mods[:l]
        a, b = CS.planted_ct(lm, n, batch, 2, rng + l), E.case_ct(lm, n, batch, 2, rng + l + 1)
        _same(dev.mul(rlk, a, b), D.mul(lm, sps, rlk, a, b), ("mul", l))
        _same(dev.rescale(a), D.rescale(lm, a), ("rescale", l))
        pool = S.pool_keys(lm, sps, n, rng + 2, key_mods=mods)
        gs = S.diag_elements(n, 3)
        Dg = D.digits(lm, sps, a[:, 1])
        want = S.galois_many(lm, sps, S.keys_of(pool, gs[:1]), gs[:1], a, Dg)
        _same(dev.galois(S.keys_of(pool, gs[:1]), gs[:1], a)[0], want[0], ("galois", l))
        pts = DL.random_pts(lm, sps, n, 2, 3, rng + 3)
        _same(dev.diag(S.keys_of(pool, gs), gs, pts, a), DL.diag_sum(lm, sps, S.keys_of(pool, gs), gs, pts, a), ("diag_sum", l))


@pytest.mark.parametrize("order", S.MIXED_ORDERS)
@pytest.mark.parametrize("alpha", S.MIXED_ALPHAS)
@pytest.mark.parametrize("n", S.WIDTH_NS)
def test_centring_decided_at_every_depth(pkg, n, alpha, order):
    """the switched component's group integers run through S.planted_integers: the edges of §36's test and, for every digit
    position, the integers that differ from floor(Q_j / 2) first at that digit, with the lower digits pointing the other way"""
    mods, sps = S.mixed_chain(n, alpha, order)
    L = len(mods)
    d2, _ = S.planted_rows(mods, alpha, n)
    batch = d2.shape[1]
    d = E.case_ct(mods, n, batch, 3, 300 + n + alpha)
    d[:, 2] = d2
    dev = Dev(pkg, mods, sps, n)
    rlk = S.uniform_key(mods, sps, n, 301 + n)
    _same(dev.relinearize(rlk, d), D.relinearize(mods, sps, rlk, d))
    ct = np.ascontiguousarray(d[:, 1:])
    gs = S.diag_elements(n, 3)
    pool = S.pool_keys(mods, sps, n, 302 + n)
    pts = DL.random_pts(mods, sps, n, 2, 3, 303 + n)
    _same(dev.diag(S.keys_of(pool, gs), gs, pts, ct), DL.diag_sum(mods, sps, S.keys_of(pool, gs), gs, pts, ct))


@pytest.mark.parametrize("alpha", S.DOWN_ALPHAS)
@pytest.mark.parametrize("n", S.WIDTH_NS)
def test_modulus_down_at_every_depth(pkg, n, alpha):
    """the same integers as t modulo P: zero keys with one chosen column steer the key sums of the special primes (proved by the CPU
    module), 2n integers a call; the special primes are just below 2^62"""
    mods, sps, d, keys, ys = S.down_case(n, alpha)
    dev = Dev(pkg, mods, sps, n)
    P = D.product(sps)
    for t, key in enumerate(keys):
        want = D.relinearize(mods, sps, key, d)
        _same(dev.relinearize(key, d), want, t)
        y = [v - P if v > P // 2 else v for v in ys[2 * n * t:2 * n * t + n]]   # the definition, by hand: r = -y / P modulo q_0
        assert [int(v) for v in E.inv(mods[0], n, want[0, 0])[0]] == [(-v * pow(P, -1, mods[0])) % mods[0] for v in y]


# ---- B: the ring ladder --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", S.LADDER)
def test_ladder(pkg, tab, n, batch):
    """(L, alpha, l) = (5, 2, 4): a key of five limbs over four, two digit groups of the key's three, the last group partial at L.
    The kernel timer shows exactly the transform rows of this log n (two passes from 2^14 up) and every deep row tagged with it"""
    L, alpha, l = S.LADDER_SHAPE
    mods, sps = D.case_chain(n, L, alpha)
    lm = mods[:l]
    dev = Dev(pkg, mods, sps, n)
    gs = CS.galois_pair(n)
    t0 = time.time()
    if n <= S.KEY_CUT:                                                       # the samplers' keys, and the device's compared with them
        s, s_res = _secret_residues(mods, sps, n)
        rlk = D.switch_key(SEED, E.RLK_BASE, s, mods, sps, tab)
        gks = [D.switch_key(SEED, G.GK_BASE + 64 * t, s, mods, sps, tab, g) for t, g in enumerate(gs)]
        _same(dev.switch_key(tab, s_res, E.RLK_BASE), rlk, "rlk")
        for t, g in enumerate(gs):
            _same(dev.switch_key(tab, s_res, G.GK_BASE + 64 * t, g), gks[t], g)
    else:
        rlk, gks = S.uniform_key(mods, sps, n, n), [S.uniform_key(mods, sps, n, n + 1 + t) for t in range(2)]
    a, b, d = CS.planted_ct(lm, n, batch, 2, 5 * n), CS.planted_ct(lm, n, batch, 2, 5 * n + 1), CS.planted_ct(lm, n, batch, 3, 5 * n + 2)
    dg = CS.reduced(S.LADDER_DIAG, n)
    dkeys = [None if g == 1 else gks[0] for g in dg]
    pts = DL.random_pts(lm, sps, n, S.LADDER_OUTPUTS, len(dg), 5 * n + 3)
    Dg = D.digits(lm, sps, a[:, 1])
    want = dict(mul=D.mul(lm, sps, rlk, a, b), relin=D.relinearize(lm, sps, rlk, d), gal=S.galois_many(lm, sps, gks, gs, a, Dg), res=D.rescale(lm, a),
                diag=DL.diag_sum(lm, sps, dkeys, dg, pts, a))
    ref_s = time.time() - t0
    got = {}

    def run():
        got.update(mul=dev.mul(rlk, a, b), relin=dev.relinearize(rlk, d), gal=dev.galois(gks, gs, a), res=dev.rescale(a), diag=dev.diag(dkeys, dg, pts, a))
    _, rows = _timed(pkg.binding, run)
    print("ladder n=%d: restatement %.2f s" % (n, ref_s))
    for what in ("mul", "relin", "res", "diag"):
        _same(got[what], want[what], what)
    for r, g in enumerate(gs):
        _same(got["gal"][r], want["gal"][r], g)
    logn = n.bit_length() - 1
    assert {name for name in rows if name.startswith("ntt_")} == CS.transform_names(n), sorted(rows)
    deep = [name for name in rows if name.startswith(("ckks_deep_", "ckks_rns_"))]
    assert all(name.endswith("_%d" % logn) for name in deep), sorted(rows)
    for label in ("ckks_deep_extend", "ckks_deep_keymac", "ckks_deep_keymac_galois", "ckks_deep_diagmac", "ckks_rns_tensor", "ckks_rns_divround"):
        assert _count(rows, label), (label, sorted(rows))


# ---- C: counts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,outputs,ident", S.COUNT_CASES)
@pytest.mark.parametrize("L,alpha,l", S.COUNT_SHAPES)
def test_diag_sum_counts(pkg, L, alpha, l, count, outputs, ident):
    """32 elements (one CARRY launch), 33 (a carry after a carry), 256 (the limit: fifteen); a pool of three keys, repeated; the
    identity first, 16th, 17th, last and filling a whole group; 4 outputs (a second full group of two) and the limit of 64"""
    n, batch = S.COUNT_N, S.COUNT_BATCH
    mods, sps = S.limit_chain(n, L, alpha)
    lm = mods[:l]
    gs = S.diag_elements(n, count, ident)
    pool = S.pool_keys(lm, sps, n, count + outputs, key_mods=mods)
    ct = CS.planted_ct(lm, n, batch, 2, count)
    pts = DL.random_pts(lm, sps, n, outputs, count, count + 1)
    _same(Dev(pkg, mods, sps, n).diag(S.keys_of(pool, gs), gs, pts, ct), DL.diag_sum(lm, sps, S.keys_of(pool, gs), gs, pts, ct))


@pytest.mark.parametrize("L,alpha,l", S.COUNT_SHAPES)
def test_galois_at_the_count_limit(pkg, L, alpha, l):
    """FHE_CKKS_GALOIS_MAX_COUNT elements in one call, each output against D.apply_galois of its element"""
    n, batch = S.COUNT_N, S.COUNT_BATCH
    mods, sps = S.limit_chain(n, L, alpha)
    lm = mods[:l]
    gs = S.diag_elements(n, G.MAX_COUNT, ())
    pool = S.pool_keys(lm, sps, n, 77, key_mods=mods)
    ct = CS.planted_ct(lm, n, batch, 2, 78)
    want = {g: D.apply_galois(lm, sps, pool[g], ct, g) for g in set(gs)}
    got = Dev(pkg, mods, sps, n).galois(S.keys_of(pool, gs), gs, ct)
    assert got.shape[0] == 256
    for r, g in enumerate(gs):
        _same(got[r], want[g], (r, g))


@pytest.mark.parametrize("L,alpha,l", S.COUNT_SHAPES)
def test_launch_counts_after_two_carries(pkg, L, alpha, l):
    n, batch = S.COUNT_N, S.COUNT_BATCH
    count, outputs = S.LAUNCH_CASE
    mods, sps = S.limit_chain(n, L, alpha)
    lm = mods[:l]
    gs = S.diag_elements(n, count, ())
    pool = S.pool_keys(lm, sps, n, 5, key_mods=mods)
    ct, pts = E.case_ct(lm, n, batch, 2, 6), DL.random_pts(lm, sps, n, outputs, count, 7)
    dev = Dev(pkg, mods, sps, n)
    _, rows = _timed(pkg.binding, lambda: dev.diag(S.keys_of(pool, gs), gs, pts, ct))
    labs = {"extend": "ckks_deep_extend", "diagmac": "ckks_deep_diagmac", "keymac": "ckks_deep_keymac", "divround": "ckks_rns_divround"}
    assert {k: _count(rows, v) for k, v in labs.items()} == DL.launch_counts(l, alpha, count, outputs)
    assert _count(rows, "ckks_deep_diagmac") == (l + alpha) * 2 * 3


def test_empty_calls_write_nothing(pkg):
    """count = 0 and batch = 0 return success and leave a poisoned output as it was"""
    B = pkg.binding
    n, (L, alpha, l), batch = S.COUNT_N, S.COUNT_SHAPES[0], S.COUNT_BATCH
    mods, sps = S.limit_chain(n, L, alpha)
    dev = Dev(pkg, mods, sps, n)
    ct, key, pts = _buf(E.case_ct(mods, n, batch, 2, 1)), _buf(S.uniform_key(mods, sps, n, 2)), _buf(DL.random_pts(mods, sps, n, 2, 2, 3))
    o = _out((2, l, 2, batch, n))
    B.ckks_deep_diag_sum_dev(dev.plans, dev.sp, [], [], L, pts.ptr, 2, ct.ptr, o.ptr, batch, count=0)
    B.ckks_deep_diag_sum_dev(dev.plans, dev.sp, [key.ptr, None], [5, 1], L, pts.ptr, 2, ct.ptr, o.ptr, 0)
    B.ckks_deep_galois_dev(dev.plans, dev.sp, [], [], L, ct.ptr, o.ptr, batch, count=0)
    B.ckks_deep_galois_dev(dev.plans, dev.sp, [key.ptr, key.ptr], [5, 15], L, ct.ptr, o.ptr, 0)
    B.ckks_deep_mul_dev(dev.plans, dev.sp, key.ptr, L, ct.ptr, ct.ptr, o.ptr, 0)
    B.ckks_deep_relinearize_dev(dev.plans, dev.sp, key.ptr, L, ct.ptr, o.ptr, 0)
    B.ckks_deep_rescale_dev(dev.plans, ct.ptr, o.ptr, 0)
    _sync()
    assert np.all(o.get() == U64(FILL))


# ---- D: chunks, clamps, workspace ----------------------------------------------------------------------------------------------------------
_CLAMP = {}


def _clamp_data():
    if not _CLAMP:
        n, alpha, l, batch = S.CLAMP
        mods, sps = D.case_chain(n, l, alpha)
        _CLAMP.update(mods=mods, sps=sps, key=S.uniform_key(mods, sps, n, 11), a=CS.planted_ct(mods, n, batch, 2, 12), b=E.case_ct(mods, n, batch, 2, 13))
    return _CLAMP


@pytest.mark.parametrize("what", ["mul", "galois", "diag_sum"])
def test_key_switch_and_diag_sum_clamped(pkg, what):
    """n = 2^14, alpha = 2, 11 limbs, batch 2: 159 and 152 slabs against 128 a chunk, so both quotients are zero and the max(1, 0) of
    slab_chunk is taken: two chunks of one ciphertext, every launch count doubled, the workspaces sized at one row a chunk"""
    n, alpha, l, batch = S.CLAMP
    c = _clamp_data()
    mods, sps, key, a, b = c["mods"], c["sps"], c["key"], c["a"], c["b"]
    B = pkg.binding
    assert B.ckks_deep_workspace_bytes(n, l, alpha, batch) == D.workspace_bytes(n, l, alpha, batch) == 8 * 159 * n
    assert B.ckks_deep_diag_workspace_bytes(n, l, alpha, batch, 3, 2) == DL.workspace_bytes(n, l, alpha, batch, 3, 2) == 8 * 152 * n
    dev = Dev(pkg, mods, sps, n)
    ng, got = D.dnum(l, alpha), {}
    labs = {"extend": "ckks_deep_extend", "diagmac": "ckks_deep_diagmac", "keymac": "ckks_deep_keymac", "tensor": "ckks_rns_tensor", "divround": "ckks_rns_divround"}
    t0 = time.time()
    if what == "mul":
        want = D.mul(mods, sps, key, a, b)
        counts = dict(extend=2 * (ng + 1), diagmac=0, keymac=2 * (l + alpha), tensor=2 * l, divround=2 * l)
        run = lambda: got.update(x=dev.mul(key, a, b))
    elif what == "galois":
        want = D.apply_galois(mods, sps, key, a, 5)
        counts = dict(extend=2 * (ng + 1), diagmac=0, keymac=2 * (l + alpha), tensor=0, divround=2 * l)
        run = lambda: got.update(x=dev.galois([key], [5], a)[0])
    else:
        gs, keys = [1, 5, 5], [None, key, key]
        pts = DL.random_pts(mods, sps, n, 2, 3, 14)
        want = DL.diag_sum(mods, sps, keys, gs, pts, a)
        counts = dict(DL.launch_counts(l, alpha, 3, 2, chunks=2), tensor=0)
        run = lambda: got.update(x=dev.diag(keys, gs, pts, a))
    print("clamp %s: restatement %.2f s" % (what, time.time() - t0))
    _, rows = _timed(B, run)
    _same(got["x"], want, what)
    assert {k: _count(rows, v) for k, v in labs.items()} == counts, sorted(rows)


@pytest.mark.parametrize("n,l,batch", [S.RESCALE_CROSSED, S.RESCALE_CLAMPED])
def test_rescale_chunks(pkg, n, l, batch):
    """(2^14, 16, 5): the rescale's chunk 2^21 / (2 l n) = 4, crossed with a row over, so the top limb's rows are read at a row
    offset.  (2^16, 17, 2): the quotient 32 // 34 is zero, clamped to two chunks of one"""
    mods = E.primes_below(40, n, l)
    chunks = S.chunks_of(batch, S.rescale_chunk(n, l, batch))
    a = CS.planted_ct(mods, n, batch, 2, n + l)
    t0 = time.time()
    want = D.rescale(mods, a)
    print("rescale n=%d l=%d: restatement %.2f s" % (n, l, time.time() - t0))
    dev = Dev(pkg, mods, [], n)
    got = {}
    _, rows = _timed(pkg.binding, lambda: got.update(x=dev.rescale(a)))
    _same(got["x"], want)
    assert _count(rows, "ckks_deep_extend") == len(chunks) and _count(rows, "ckks_rns_divround") == len(chunks) * (l - 1), sorted(rows)
    assert pkg.binding.ckks_deep_workspace_bytes(n, l, 1, batch) >= 8 * 2 * l * n * max(chunks)


def _reuse_data():
    n, (L, alpha, l) = S.REUSE["n"], S.REUSE["shape"]
    mods, sps = D.case_chain(n, L, alpha)
    key = S.uniform_key(mods, sps, n, 21)
    r = CS.planted_ct(mods, n, S.REUSE["rescale_batch"], 2, 22)
    a, b = CS.planted_ct(mods, n, S.REUSE["mul_batch"], 2, 23), E.case_ct(mods, n, S.REUSE["mul_batch"], 2, 24)
    c = CS.planted_ct(mods, n, S.REUSE["diag_batch"], 2, 25)
    gs, keys = [5, 1, 5], [key, None, key]
    pts = DL.random_pts(mods, sps, n, 2, 3, 26)
    return dict(n=n, mods=mods, sps=sps, key=key, r=r, a=a, b=b, c=c, gs=gs, keys=keys, pts=pts, want_r=D.rescale(mods, r), want_m=D.mul(mods, sps, key, a, b),
                want_d=DL.diag_sum(mods, sps, keys, gs, pts, c))


def test_slot_14_smaller_larger_smaller(pkg):
    """one created stream: a rescale (2 l n words of slot 14), a product (deep_slabs 3 n), a diagonal sum (diag_slabs 2 n), the
    rescale again.  The stream is made and destroyed through the HIP runtime and its workspaces released first (§35)"""
    d = _reuse_data()
    n, l, alpha = d["n"], len(d["mods"]), len(d["sps"])
    B = pkg.binding
    sizes = [8 * 2 * l * n, D.workspace_bytes(n, l, alpha, 3), DL.workspace_bytes(n, l, alpha, 2, 3, 2)]
    assert sizes[0] < sizes[2] < sizes[1] and B.ckks_deep_workspace_bytes(n, l, alpha, 3) == sizes[1] and B.ckks_deep_diag_workspace_bytes(n, l, alpha, 2, 3, 2) == sizes[2]
    held = pkg.load_library().fhe_ntt_workspace_bytes()
    st = OwnStream(pkg)
    dev = Dev(pkg, d["mods"], d["sps"], n, stream=st)
    try:
        _same(dev.rescale(d["r"]), d["want_r"], "rescale")
        _same(dev.mul(d["key"], d["a"], d["b"]), d["want_m"], "mul")
        _same(dev.diag(d["keys"], d["gs"], d["pts"], d["c"]), d["want_d"], "diag_sum")
        _same(dev.rescale(d["r"]), d["want_r"], "rescale again")
    finally:
        st.close()
    assert pkg.load_library().fhe_ntt_workspace_bytes() == held


def test_two_streams_interleaved(pkg):
    """a product on one created stream against a diagonal sum on another, issued alternately, nothing waited for in between:
    workspaces are keyed by (device, stream, thread), so slot 14 of one stream is never the other's"""
    d = _reuse_data()
    held = pkg.load_library().fhe_ntt_workspace_bytes()
    one, two = OwnStream(pkg), OwnStream(pkg)
    da, db = Dev(pkg, d["mods"], d["sps"], d["n"], stream=one), Dev(pkg, d["mods"], d["sps"], d["n"], stream=two)
    try:
        calls = []
        for _ in range(3):
            calls.append((da.mul(d["key"], d["a"], d["b"], defer=True), db.diag(d["keys"], d["gs"], d["pts"], d["c"], defer=True)))
        _sync()
        for (om, im), (od, idg) in calls:
            _same(om.get(), d["want_m"], "mul")
            _same(od.get(), d["want_d"], "diag_sum")
            assert all(np.array_equal(x.get(), y) for x, y in im + idg)
    finally:
        _sync()
        one.close()
        two.close()
    assert pkg.load_library().fhe_ntt_workspace_bytes() == held


# ---- E: alignment --------------------------------------------------------------------------------------------------------------------------
_ALIGN = {}


def _align_data(pkg, tab, n, shape, batch):
    """the operands of one shape, the words of every entry point from aligned buffers, and those words held against the
    restatement (the key builders at n = 64 only: at 8192 the sampled reference costs more than the rest of the case)"""
    if n not in _ALIGN:
        L, alpha, l = shape
        mods, sps = D.case_chain(n, L, alpha)
        lm = mods[:l]
        s, s_res = _secret_residues(mods, sps, n)
        g = 5
        rlk, gk = S.uniform_key(mods, sps, n, 31), S.uniform_key(mods, sps, n, 32)
        a, b, d = CS.planted_ct(lm, n, batch, 2, 33), E.case_ct(lm, n, batch, 2, 34), CS.planted_ct(lm, n, batch, 3, 35)
        gs, keys = [g, 1, 2 * n - 1], [gk, None, rlk]
        pts = DL.random_pts(lm, sps, n, 2, 3, 36)
        run = {"relin_key": lambda v: v.switch_key(tab, s_res, E.RLK_BASE + 64 * 5), "galois_key": lambda v: v.switch_key(tab, s_res, G.GK_BASE + 64 * 6, g),
               "relinearize": lambda v: v.relinearize(rlk, d), "mul": lambda v: v.mul(rlk, a, b), "galois": lambda v: v.galois([gk], [g], a),
               "diag_sum": lambda v: v.diag(keys, gs, pts, a), "rescale": lambda v: v.rescale(a)}
        assert set(run) == set(S.ENTRIES)
        aligned = {what: fn(Dev(pkg, mods, sps, n)) for what, fn in run.items()}
        _same(aligned["relinearize"], D.relinearize(lm, sps, rlk, d), "relinearize")
        _same(aligned["mul"], D.mul(lm, sps, rlk, a, b), "mul")
        _same(aligned["galois"][0], D.apply_galois(lm, sps, gk, a, g), "galois")
        _same(aligned["diag_sum"], DL.diag_sum(lm, sps, keys, gs, pts, a), "diag_sum")
        _same(aligned["rescale"], D.rescale(lm, a), "rescale")
        if n == 64:
            _same(aligned["relin_key"], D.switch_key(SEED, E.RLK_BASE + 64 * 5, s, mods, sps, tab), "relin_key")
            _same(aligned["galois_key"], D.switch_key(SEED, G.GK_BASE + 64 * 6, s, mods, sps, tab, g), "galois_key")
        _ALIGN[n] = (mods, sps, run, aligned)
    return _ALIGN[n]


@pytest.mark.parametrize("what", S.ENTRIES)
@pytest.mark.parametrize("mode", S.ALIGN_MODES)
@pytest.mark.parametrize("n,shape,batch", S.ALIGN_SHAPES)
def test_alignment(pkg, tab, n, shape, batch, mode, what):
    """every buffer, the inputs alone or the outputs alone one word past a 16-byte boundary: the words of the aligned run, which
    are the restatement's; the inputs unchanged; a sentinel word intact either side of every buffer.  (64, (9, 3, 7), 3) is one
    chunk; (8192, (12, 4, 12), 2) two chunks of one ciphertext, so the staged copy of inverse_into sees a row offset"""
    mods, sps, run, aligned = _align_data(pkg, tab, n, shape, batch)
    got = run[what](Dev(pkg, mods, sps, n, mi=mode in ("all", "inputs"), mo=mode in ("all", "outputs")))
    _same(got, aligned[what], (what, mode))
