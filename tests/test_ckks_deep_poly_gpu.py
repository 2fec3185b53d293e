"""Scalar sums, inner products and Chebyshev plans on the deep CKKS chain on the device (ckks_deep.hip):
fhe_ckks_deep_lincomb_dev and fhe_ckks_deep_dot_dev word for word against tests/_ckks_deep_poly_numpy.py (tolerance zero), which
tests/test_ckks_deep_poly_cpu.py proved, every output between sentinels; byte for byte against fhe_ckks_rns_lincomb_dev on slices
of at most 8 plans, against fhe_ckks_deep_mul_dev (one pair, no weight) and, at alpha = 1, against fhe_ckks_rns_dot_dev; either
side of every limb-slice edge; bound-reaching rows; mixed 30/61-bit chains; the chunk; a second stream; misaligned buffers; every
rejection with its outputs untouched; the launch counts; and a degree-15 Chebyshev fit of the logistic function and an inner
product of 8 pairs through ckks.eval_chebyshev, ckks.lincomb and ckks.dot on a DeepClientKey."""
import numpy as np
import pytest

import _ckks_deep_numpy as D
import _ckks_deep_poly_numpy as DP
import _ckks_eval_numpy as E
import _ckks_numpy as K
import _client_numpy as C
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A
GUARD = 16


def _refused():
    return pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ")


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


class Guarded:
    """an output of `shape` between two runs of GUARD sentinel words"""

    def __init__(self, shape):
        self.shape, self.words = tuple(shape), int(np.prod(shape))
        self.buf = _empty((self.words + 2 * GUARD,))
        self.view = self.buf[GUARD:GUARD + self.words]

    def ptr(self):
        return self.view.data_ptr()

    def read(self):
        """the words, after checking that the sentinels either side are as they were"""
        assert bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.words:] == FILL).all())
        return _u64(self.view).reshape(self.shape)

    def untouched(self):
        return bool((self.buf == FILL).all())


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _plans(pkg, mods, n):
    return [pkg.Plan(q, n) for q in mods]


def _lincomb(pkg, plans, d_cts, w, k, outputs, batch, n, stream=None):
    out = Guarded((outputs, len(plans), 2, batch, n))
    pkg.binding.ckks_deep_lincomb_dev(plans, [x.data_ptr() for x in d_cts], DP.flat(w), DP.flat(k), outputs, out.ptr(), batch, stream)
    return out.read()


def _dot(pkg, plans, sp, d_key, kl, d_as, d_bs, w, batch, n, stream=None):
    out = Guarded((len(plans), 2, batch, n))
    pkg.binding.ckks_deep_dot_dev(plans, sp, d_key.data_ptr(), kl, [x.data_ptr() for x in d_as], [x.data_ptr() for x in d_bs], DP.flat(w), out.ptr(), batch, stream)
    return out.read()


def _rns_lincomb_slices(pkg, plans, d_cts, w, k, outputs, batch, n):
    """fhe_ckks_rns_lincomb_dev on slices of at most 8 plans of the same buffers -> [outputs][limbs][2][batch][n]"""
    l, limb_bytes = len(plans), 2 * batch * n * 8
    got = np.zeros((outputs, l, 2, batch, n), dtype=U64)
    for i0 in range(0, l, 8):
        i1 = min(l, i0 + 8)
        out = _empty((outputs, i1 - i0, 2, batch, n))
        ws = [[row[i0:i1] for row in o] for o in w]
        ks = None if k is None else [row[i0:i1] for row in k]
        pkg.binding.ckks_rns_lincomb_dev(plans[i0:i1], [x.data_ptr() + i0 * limb_bytes for x in d_cts], DP.flat(ws), DP.flat(ks), outputs, out.data_ptr(), batch)
        got[:, i0:i1] = _u64(out)
    return got


# ---- the scalar sum, word for word ----------------------------------------------------------------------------------------------------------
def _lincomb_case(pkg, mods, n, batch, sweep, rng, cts=None):
    plans = _plans(pkg, mods, n)
    cts = [E.case_ct(mods, n, batch, 2, rng + r) for r in range(5)] if cts is None else cts
    d = [_dev(x) for x in cts]
    for count, outputs, consts in sweep:
        ins = [r % len(cts) for r in range(count)]                             # the same input many times over
        w, k = DP.random_lin_weights(mods, outputs, count, rng + count, consts)
        got = _lincomb(pkg, plans, [d[r] for r in ins], w, k, outputs, batch, n)
        assert np.array_equal(got, DP.lincomb(mods, [cts[r] for r in ins], w, k)), (count, outputs, consts)
        assert np.array_equal(got, _rns_lincomb_slices(pkg, plans, [d[r] for r in ins], w, k, outputs, batch, n)), (count, outputs, consts)
    for x, y in zip(d, cts):
        assert np.array_equal(_u64(x), y)                                     # the inputs are only read


LIN_SWEEP = [(1, 1, True), (8, 4, False), (9, 5, True), (17, 4, True)]


@pytest.mark.parametrize("L,alpha,l", DP.SHAPES)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 8, 64])
def test_lincomb_word_for_word(pkg, n, batch, L, alpha, l):
    mods, _ = D.case_chain(n, L, alpha)
    _lincomb_case(pkg, mods[:l], n, batch, LIN_SWEEP, 1000 * n + 10 * L + l)


@pytest.mark.parametrize("l", DP.SLICE_EDGES + (32,))
def test_lincomb_either_side_of_the_slice_edges(pkg, l):
    """every count and output count of the issue's list at n = 8: the group edge 8 | 9, three launches at 17, the caps 64 and 16"""
    n = 8
    mods = E.primes_below(40, n, l)
    sweep = [(c, 1, c % 2 == 1) for c in DP.LIN_COUNTS] + [(9, o, o % 2 == 0) for o in DP.LIN_OUTPUTS] + [(64, 16, True)]
    _lincomb_case(pkg, mods, n, 1, sweep if l in (9, 32) else [(9, 5, True), (17, 4, False)], 50 + l)


@pytest.mark.parametrize("l", [9, 17])
def test_lincomb_bound_reaching_rows(pkg, l):
    """every word, weight and constant q - 1 for primes just below 2^62, at the full period (8 inputs a launch) and at the caps"""
    n = 8
    mods = E.primes_below(62, n, l)
    assert all((1 << 62) - q < 1 << 13 for q in mods)                       # a term (q - 1)^2 is above 2^124 - 2^76
    plans = _plans(pkg, mods, n)
    ct = DP.top_ct(mods, 2, n)
    d = _dev(ct)
    for count, outputs in ((8, 4), (16, 1), (64, 5)):
        w = [[[q - 1 for q in mods] for _ in range(count)] for _ in range(outputs)]
        k = [[q - 1 for q in mods] for _ in range(outputs)]
        got = _lincomb(pkg, plans, [d] * count, w, k, outputs, 2, n)
        assert np.array_equal(got, DP.lincomb(mods, [ct] * count, w, k))
        for i, q in enumerate(mods):                                         # by hand: count (q - 1)^2 + [c = 0] (q - 1) = count - [c = 0]
            assert (got[:, i, 0] == (count - 1) % q).all() and (got[:, i, 1] == count % q).all()


def test_lincomb_on_a_mixed_chain(pkg):
    """30-bit beside 61-bit primes, in both orders within a slice and across the slice edge"""
    n = 64
    small, big = E.primes_below(30, n, 6), E.primes_below(61, n, 6)
    mods = [x for pair in zip(small[:5], big[:5]) for x in pair] + [big[5], small[5]]
    assert len(mods) == 12
    _lincomb_case(pkg, mods, n, 3, [(9, 5, True), (17, 2, False)], 77)


# ---- the inner product, word for word -------------------------------------------------------------------------------------------------------
def _pairs(items, count):
    """pair r of the cycle over `items`: neighbours, a repeated pointer across pairs, and the last pair a square"""
    m = len(items)
    return [(items[r % m], items[(r + 1) % m]) for r in range(count - 1)] + [(items[(count - 1) % m],) * 2]


def _dot_case(pkg, mods, sps, l, n, batch, sweep, rng, cts=None):
    lm = mods[:l]
    plans, sp = _plans(pkg, lm, n), _plans(pkg, sps, n)
    L, alpha = len(mods), len(sps)
    key = E.case_ct(list(mods) + list(sps), n, D.dnum(L, alpha), 2, rng).transpose(2, 0, 1, 3)   # [dnum][L + alpha][2][n], canonical per column
    key = np.ascontiguousarray(key)
    d_key = _dev(key)
    cts = [E.case_ct(lm, n, batch, 2, rng + 1 + r) for r in range(4)] if cts is None else cts
    d = [_dev(x) for x in cts]
    for count, weighted in sweep:
        w = DP.random_dot_weights(lm, count, rng + 7 * count) if weighted else None
        got = _dot(pkg, plans, sp, d_key, L, [a for a, _ in _pairs(d, count)], [b for _, b in _pairs(d, count)], w, batch, n)
        assert np.array_equal(got, DP.dot(lm, sps, key, _pairs(cts, count), w)), (count, weighted)
    for x, y in zip(d, cts):
        assert np.array_equal(_u64(x), y)
    return plans, sp, d_key, d, cts, key


@pytest.mark.parametrize("L,alpha,l", DP.SHAPES)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 8, 64])
def test_dot_word_for_word(pkg, n, batch, L, alpha, l):
    mods, sps = D.case_chain(n, L, alpha)
    sweep = [(c, wt) for c in DP.DOT_COUNTS for wt in (False, True)] if (n, batch) == (8, 1) else [(5, False), (17, True)]
    _dot_case(pkg, mods, sps, l, n, batch, sweep, 2000 * n + 10 * L + l)


@pytest.mark.parametrize("L,alpha,l", [(32, 8, 32), (32, 1, 32), (17, 3, 8), (17, 3, 9), (17, 3, 16), (17, 3, 17)])
def test_dot_at_thirty_two_limbs_and_the_slice_edges(pkg, L, alpha, l):
    n = 8
    mods, sps = D.case_chain(n, L, alpha)
    _dot_case(pkg, mods, sps, l, n, 1, [(17, True), (4, False)], 300 + L + l)


@pytest.mark.parametrize("alpha,l", [(2, 5), (3, 9)])
def test_dot_bound_reaching_rows(pkg, alpha, l):
    """every word and weight q - 1, the chain primes just below 2^62 and the special primes the few above them, at the full fold
    period (16 pairs a launch: four runs of eight terms in d1) and at the cap"""
    n = 8
    primes = E.primes_below(62, n, l + alpha)
    mods, sps = primes[alpha:], primes[:alpha]
    D.check_chain(n, mods, sps)
    cts = [DP.top_ct(mods, 1, n)] * 4
    _, _, _, _, _, key = _dot_case(pkg, mods, sps, l, n, 1, [(4, False), (16, True), (64, True), (64, False)], 400 + l, cts=cts)
    for count in (4, 16, 64):                                               # by hand: the summed tensor of count squares of -1 is (count, 2 count, count)
        assert np.array_equal(DP.tensor_sum(mods, _pairs(cts, count)), np.stack([np.stack([np.full((1, n), m * count % q, dtype=U64) for m in (1, 2, 1)]) for q in mods]))


@pytest.mark.parametrize("L,alpha,l", [(5, 2, 5), (9, 3, 7), (17, 8, 17)])
def test_one_unweighted_pair_is_byte_for_byte_the_product(pkg, L, alpha, l):
    n, batch = 64, 3
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp, d_key, d, _, _ = _dot_case(pkg, mods, sps, l, n, batch, [], 500 + L)
    old = _empty((l, 2, batch, n))
    pkg.binding.ckks_deep_mul_dev(plans, sp, d_key.data_ptr(), L, d[0].data_ptr(), d[1].data_ptr(), old.data_ptr(), batch)
    assert np.array_equal(_dot(pkg, plans, sp, d_key, L, [d[0]], [d[1]], None, batch, n), _u64(old))


@pytest.mark.parametrize("n,k", [(64, 1), (64, 3), (16, 8)])
def test_alpha_one_is_byte_for_byte_the_rns_entry_point(pkg, n, k):
    """this oracle shares no code with the restatement"""
    batch = 3
    mods, P = E.primes_below(40, n, k), E.primes_below(41, n, 1)[0]
    plans, sp, d_key, d, _, _ = _dot_case(pkg, mods, [P], k, n, batch, [], 600 + n + k)
    for count, weighted in ((1, False), (5, True), (17, False), (64, True)):
        w = DP.random_dot_weights(mods, count, 9 + count) if weighted else None
        xs, ys = [a for a, _ in _pairs(d, count)], [b for _, b in _pairs(d, count)]
        old = _empty((k, 2, batch, n))
        pkg.binding.ckks_rns_dot_dev(plans, sp[0], d_key.data_ptr(), k, [x.data_ptr() for x in xs], [y.data_ptr() for y in ys], DP.flat(w), old.data_ptr(), batch)
        assert np.array_equal(_dot(pkg, plans, sp, d_key, k, xs, ys, w, batch, n), _u64(old)), (count, weighted)


def test_a_batch_one_above_the_chunk(pkg):
    n, l, alpha = 8192, 4, 2
    batch = D.chunk_rows(n, l, alpha, 1 << 20) + 1
    assert batch == 6
    mods, sps = D.case_chain(n, l, alpha)
    _dot_case(pkg, mods, sps, l, n, batch, [(3, True)], 700)


# ---- a second stream, alignment ---------------------------------------------------------------------------------------------------------------
def test_second_stream_and_misaligned_buffers(pkg):
    import torch

    n, batch, (L, alpha, l) = 64, 3, (12, 3, 9)
    mods, sps = D.case_chain(n, L, alpha)
    lm = mods[:l]
    plans, sp, d_key, d, cts, key = _dot_case(pkg, mods, sps, l, n, batch, [], 800)
    count = 5
    w = DP.random_dot_weights(lm, count, 801)
    lw, lk = DP.random_lin_weights(lm, 5, count, 802)
    ins = [r % 4 for r in range(count)]
    want_dot = DP.dot(lm, sps, key, _pairs(cts, count), w)
    want_lin = DP.lincomb(lm, [cts[r] for r in ins], lw, lk)

    def off8(x):
        """a copy of x at an address that is 8 modulo 16"""
        buf = _empty((x.size + 3,))
        view = buf[1:1 + x.size] if buf.data_ptr() % 16 == 0 else buf[2:2 + x.size]
        assert view.data_ptr() % 16 == 8
        view.copy_(_dev(x).reshape(-1))
        return buf, view
    keep = [off8(x) for x in [key] + cts + [np.zeros(want_dot.shape, dtype=U64), np.zeros(want_lin.shape, dtype=U64)]]
    k_, c_, (o_dot, o_lin) = keep[0][1], [v for _, v in keep[1:5]], [v for _, v in keep[5:]]
    B = pkg.binding
    B.ckks_deep_dot_dev(plans, sp, k_.data_ptr(), L, [a.data_ptr() for a, _ in _pairs(c_, count)], [b.data_ptr() for _, b in _pairs(c_, count)], DP.flat(w),
                        o_dot.data_ptr(), batch)
    assert np.array_equal(_u64(o_dot).reshape(want_dot.shape), want_dot)
    B.ckks_deep_lincomb_dev(plans, [c_[r].data_ptr() for r in ins], DP.flat(lw), DP.flat(lk), 5, o_lin.data_ptr(), batch)
    assert np.array_equal(_u64(o_lin).reshape(want_lin.shape), want_lin)
    assert all(np.array_equal(_u64(v).reshape(x.shape), x) for v, x in zip(c_, cts))
    # a stream of the high-priority pool, made and released here: the default pool hands its streams out in turn, and later tests
    # that count the workspace a fresh stream holds (tests/test_round3_gpu.py) depend on which of them they are given
    st = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    B._check(B.load_library().fhe_ntt_release_stream_workspace(st.cuda_stream))
    held = B.load_library().fhe_ntt_workspace_bytes()
    with torch.cuda.stream(st):
        got_lin = _lincomb(pkg, plans, [d[r] for r in ins], lw, lk, 5, batch, n, stream=st.cuda_stream)
        assert B.load_library().fhe_ntt_workspace_bytes() == held                # the scalar sum takes no workspace
        got_dot = _dot(pkg, plans, sp, d_key, L, [a for a, _ in _pairs(d, count)], [b for _, b in _pairs(d, count)], w, batch, n, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(got_lin, want_lin) and np.array_equal(got_dot, want_dot)
    assert D.chunk_rows(n, l, alpha, batch) == batch
    assert B.load_library().fhe_ntt_workspace_bytes() >= held + 8 * D.slabs(l, alpha) * n * batch   # the stream's own workspace: mul's, slot 14
    B._check(B.load_library().fhe_ntt_release_stream_workspace(st.cuda_stream))
    assert B.load_library().fhe_ntt_workspace_bytes() == held
    assert np.array_equal(_dot(pkg, plans, sp, d_key, L, [a for a, _ in _pairs(d, count)], [b for _, b in _pairs(d, count)], w, batch, n), want_dot)


# ---- rejections: nothing is written -------------------------------------------------------------------------------------------------------------
def test_every_rejection_leaves_the_outputs_untouched(pkg):
    import torch

    B = pkg.binding
    n, L, alpha, batch = 8, 9, 3, 2
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    key = _dev(np.zeros((D.dnum(L, alpha), L + alpha, 2, n), dtype=U64))
    a, b = _dev(E.case_ct(mods, n, batch, 2, 5)), _dev(E.case_ct(mods, n, batch, 2, 6))
    out = Guarded((2, L, 2, batch, n))
    other = pkg.Plan(E.primes_below(40, 2 * n, 1)[0], 2 * n)
    wide = pkg.Plan(E.primes_below(63, n, 1)[0], n)
    low = _plans(pkg, E.primes_below(39, n, alpha), n)
    P, K_, A, Bp = out.ptr(), key.data_ptr(), a.data_ptr(), b.data_ptr()
    one = [1] * L
    ct_bytes = L * 2 * batch * n * 8

    def lin(plans=plans, cts=(A, Bp), w=tuple(one * 4), k=tuple(one * 2), outputs=2, o=P, batch=batch, **kw):
        B.ckks_deep_lincomb_dev(plans, None if cts is None else list(cts), None if w is None else list(w), None if k is None else list(k), outputs, o, batch, **kw)

    def dot(plans=plans, sp=sp, key=K_, kl=L, xs=(A, Bp), ys=(Bp, Bp), w=tuple(one * 2), o=P, batch=batch, **kw):
        B.ckks_deep_dot_dev(plans, sp, key, kl, None if xs is None else list(xs), None if ys is None else list(ys), None if w is None else list(w), o, batch, **kw)

    at = lambda i, x=None: tuple(one[:i] + [mods[i] if x is None else x] + one[i + 1:])
    chain = [
        (B.FHE_E_NULL, dict(plans=None, limbs=L)), (B.FHE_E_NULL, dict(plans=plans[:2] + [None] + plans[3:])),
        (B.FHE_E_INVALID, dict(limbs=0)), (B.FHE_E_INVALID, dict(plans=plans * 4, limbs=33)),
        (B.FHE_E_PARAM_MISMATCH, dict(plans=plans[:8] + [other])), (B.FHE_E_INVALID, dict(plans=plans[:8] + plans[:1])), (B.FHE_E_INVALID, dict(plans=plans[:8] + [wide])),
    ]
    lin_calls = chain + [
        (B.FHE_E_INVALID, dict(cts=(), w=())), (B.FHE_E_INVALID, dict(cts=(A,) * 65, w=tuple(one * 130))),
        (B.FHE_E_INVALID, dict(outputs=0)), (B.FHE_E_INVALID, dict(outputs=17, w=tuple(one * 34), k=tuple(one * 17))),
        (B.FHE_E_NULL, dict(cts=None, count=2)), (B.FHE_E_NULL, dict(w=None)),
        (B.FHE_E_INVALID, dict(w=at(0) + tuple(one * 3))), (B.FHE_E_INVALID, dict(w=tuple(one * 3) + at(8))), (B.FHE_E_INVALID, dict(k=tuple(one) + at(8))),
        (B.FHE_E_INVALID, dict(batch=1 << 58)),
        (B.FHE_E_NULL, dict(o=None)), (B.FHE_E_INVALID, dict(o=P + 4)),
        (B.FHE_E_NULL, dict(cts=(A, None))), (B.FHE_E_INVALID, dict(cts=(A, Bp + 4))),
        (B.FHE_E_INVALID, dict(o=A)), (B.FHE_E_INVALID, dict(o=Bp + ct_bytes - 8)), (B.FHE_E_INVALID, dict(o=A - 2 * ct_bytes + 8)),
    ]
    dot_calls = chain + [
        (B.FHE_E_NULL, dict(sp=None, alpha=alpha)), (B.FHE_E_NULL, dict(sp=[sp[0], None, sp[2]])),
        (B.FHE_E_INVALID, dict(alpha=0)), (B.FHE_E_INVALID, dict(sp=sp * 3, alpha=9)),
        (B.FHE_E_PARAM_MISMATCH, dict(sp=sp[:2] + [other])), (B.FHE_E_INVALID, dict(sp=sp[:2] + plans[:1])), (B.FHE_E_INVALID, dict(sp=sp[:2] + [wide])),
        (B.FHE_E_INVALID, dict(sp=low)),
        (B.FHE_E_INVALID, dict(kl=L - 1)), (B.FHE_E_INVALID, dict(kl=33)),
        (B.FHE_E_INVALID, dict(xs=(), ys=(), w=None)), (B.FHE_E_INVALID, dict(xs=(A,) * 65, ys=(Bp,) * 65, w=None)),
        (B.FHE_E_NULL, dict(xs=None, count=2)), (B.FHE_E_NULL, dict(ys=None)),
        (B.FHE_E_INVALID, dict(w=at(0) + tuple(one))), (B.FHE_E_INVALID, dict(w=tuple(one) + at(8))),
        (B.FHE_E_INVALID, dict(batch=1 << 58)),
        (B.FHE_E_NULL, dict(key=None)), (B.FHE_E_NULL, dict(o=None)), (B.FHE_E_INVALID, dict(key=K_ + 4)), (B.FHE_E_INVALID, dict(o=P + 4)),
        (B.FHE_E_INVALID, dict(o=K_)),
        (B.FHE_E_NULL, dict(xs=(A, None))), (B.FHE_E_NULL, dict(ys=(Bp, None))), (B.FHE_E_INVALID, dict(xs=(A, Bp + 4))), (B.FHE_E_INVALID, dict(ys=(Bp + 4, Bp))),
        (B.FHE_E_INVALID, dict(o=A)), (B.FHE_E_INVALID, dict(o=Bp + ct_bytes - 8)), (B.FHE_E_INVALID, dict(o=A - ct_bytes + 8)),
    ]
    for fn, calls in ((lin, lin_calls), (dot, dot_calls)):
        for code, kw in calls:
            with _refused() as e:
                fn(**kw)
            assert e.value.code == code, (fn.__name__, kw, e.value)
    torch.cuda.synchronize()
    assert out.untouched()
    assert not _u64(key).any()
    # batch = 0 is a no-op after the host checks
    B.ckks_deep_lincomb_dev(plans, [None, None], one * 4, None, 2, None, 0)
    B.ckks_deep_dot_dev(plans, sp, None, L, [None], [None], None, None, 0)
    with _refused():
        lin(batch=0, w=at(0) + tuple(one * 3))
    with _refused():
        dot(batch=0, w=at(0) + tuple(one))
    torch.cuda.synchronize()
    assert out.untouched()
    # and the accepted calls write every word
    lin()
    torch.cuda.synchronize()
    assert not bool((out.view == FILL).any())
    out.view.fill_(FILL)
    dot()
    torch.cuda.synchronize()
    assert not bool((out.view[:out.words // 2] == FILL).any()) and bool((out.view[out.words // 2:] == FILL).all())


# ---- the launch counts ----------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(pkg):
    import torch

    B = pkg.binding
    labs = {"lincomb": "ckks_deep_lincomb", "tensorsum": "ckks_deep_tensorsum", "tensor": "ckks_rns_tensor", "extend": "ckks_deep_extend", "keymac": "ckks_deep_keymac",
            "divround": "ckks_rns_divround"}

    def counts(fn):
        torch.cuda.synchronize()
        B.kernel_timing_enable(True)
        B.kernel_timing_reset()
        try:
            fn()
            torch.cuda.synchronize()
            got = B.kernel_timing_read(256)
        finally:
            B.kernel_timing_enable(False)
        return {k: sum(c for name, (_, c) in got.items() if name.rsplit("_", 1)[0] == v) for k, v in labs.items()}

    n, batch = 64, 3
    for L, alpha, l in ((9, 3, 7), (17, 8, 17), (24, 3, 24), (32, 4, 32), (4, 1, 4)):
        mods, sps = D.case_chain(n, L, alpha)
        plans, sp = _plans(pkg, mods, n)[:l], _plans(pkg, sps, n)
        key = _dev(np.random.default_rng(1).integers(0, 1 << 38, (D.dnum(L, alpha), L + alpha, 2, n), dtype=np.uint64))
        a = _dev(E.case_ct(mods[:l], n, batch, 2, 3))
        out = _empty((16, l, 2, batch, n))
        assert D.chunk_rows(n, l, alpha, batch) == batch                     # one chunk
        for count, outputs in ((1, 1), (8, 4), (9, 5), (15, 4), (17, 16), (64, 1)):
            got = counts(lambda: B.ckks_deep_lincomb_dev(plans, [a.data_ptr()] * count, [1] * (outputs * count * l), None, outputs, out.data_ptr(), batch))
            assert got == dict(lincomb=DP.lincomb_launches(l, outputs, count), tensorsum=0, tensor=0, extend=0, keymac=0, divround=0), (l, count, outputs)
            assert got["lincomb"] == -(-l // 8) * -(-outputs // 4) * -(-count // 8)
        for count in (1, 4, 16, 17, 64):
            for w in (None, [1] * (count * l)):
                got = counts(lambda: B.ckks_deep_dot_dev(plans, sp, key.data_ptr(), L, [a.data_ptr()] * count, [a.data_ptr()] * count, w, out.data_ptr(), batch))
                assert got == dict(DP.dot_launch_counts(l, alpha, count), lincomb=0), (l, alpha, count)
                assert got["tensorsum"] == -(-l // 8) * -(-count // 16)
        # the relinearisation's launches are exactly the product's, whose tensor is a launch a limb
        got = counts(lambda: B.ckks_deep_mul_dev(plans, sp, key.data_ptr(), L, a.data_ptr(), a.data_ptr(), out.data_ptr(), batch))
        assert got == dict(DP.dot_launch_counts(l, alpha, 1), tensorsum=0, tensor=l, lincomb=0)


# ---- end to end at n = 64, L = 12, alpha = 3, Delta = 2^40 ------------------------------------------------------------------------------------------
# The end-to-end tests read `key._next_row`, the row ClientKeyBase._on_fresh_rows (rlwe_client.py) hands the next encryption, to
# give the restatement's encryption the same rows: the key has no public accessor for it, and the module's key is shared by both
# tests, so a fixed row would depend on their order.  A change to that bookkeeping shows here first; it is no fault of §39's.
E2E_SEED = bytes((31 * i + 7) % 256 for i in range(32))
E2E_RNG = 3901


@pytest.fixture(scope="module")
def e2e(pkg, tab):
    ck = pkg.ckks
    n, L, alpha, delta = 64, 12, 3, float(1 << 40)
    mods, sps = D.e2e_chain(n, L, alpha)
    param = ck.DeepParam(n, mods, sps)
    key = ck.DeepClientKey.generate(E2E_SEED, param, delta)
    s = K.secret_key(E2E_SEED, 0, n)
    pk_ref = E.public_key(E2E_SEED, E.PK_BASE, s, mods, tab)
    rlk = key.relin_key(0)
    rlk_ref = D.switch_key(E2E_SEED, E.RLK_BASE, s, mods, sps, tab)
    assert np.array_equal(_u64(rlk.d_rlk), rlk_ref)
    return dict(n=n, L=L, alpha=alpha, delta=delta, mods=mods, sps=sps, param=param, key=key, pk=key.public_key(0), s=s, pk_ref=pk_ref, rlk=rlk, rlk_ref=rlk_ref)


def test_logistic_fit_of_degree_15_through_eval_chebyshev(pkg, tab, e2e):
    """a degree-15 Chebyshev fit of the logistic function on [-4, 4]: word-equal to the restated plan wire by wire at its result,
    and decoding within 4 x the restatement's own maximum error against plan.simulate, the rule of §36's and §37's end-to-end
    tests (the figures are in DESIGN.md §39)."""
    ck = pkg.ckks
    n, L, delta, mods, sps, key = e2e["n"], e2e["L"], e2e["delta"], e2e["mods"], e2e["sps"], e2e["key"]
    rows, iv = 2, (-4.0, 4.0)
    x = np.random.default_rng(E2E_RNG).uniform(iv[0], iv[1], (rows, n // 2))
    msg = K.encode(x.astype(np.complex128), delta)
    ct_ref = E.encrypt(E2E_SEED, key._next_row, e2e["pk_ref"], msg, rows, mods, tab)   # the rows the next encryption takes
    ct = key.encrypt(e2e["pk"], msg)
    assert isinstance(ct, ck.DeepCiphertext) and ct.level == L - 1 and np.array_equal(_u64(ct.d), ct_ref)
    coeffs = ck.chebyshev_fit(DP.logistic, 15, iv)
    plan = ck.ChebyshevPlan.build(coeffs, iv)
    assert plan.levels <= L - 1 and plan.products == 7
    res = ck.eval_chebyshev(ct, plan, e2e["rlk"])
    wires = DP.replay(plan, ct_ref, delta, L - 1, mods, sps, e2e["rlk_ref"])
    words, level, scale = wires[plan.result]
    assert isinstance(res, ck.DeepCiphertext) and (res.level, res.scale) == (level, scale) and level == L - 1 - plan.levels
    assert np.array_equal(_u64(res.d), words)
    again = ck.eval_chebyshev(ct, coeffs, e2e["rlk"], interval=iv)          # from coefficients: the same plan, the same words
    assert np.array_equal(_u64(again.d), words)
    want = plan.simulate(x)
    dec_ref = E.decrypt(mods[:1], n, e2e["s"], words[:1])
    low = res.at_level(0)
    assert np.array_equal(key.decrypt(low), dec_ref)
    ref_err = float(np.abs(K.decode(dec_ref, scale) - want).max())
    err = float(np.abs(key.decrypt_and_decode(low) - want).max())
    fit = float(np.abs(want - DP.logistic(x)).max())
    print(f"logistic, degree 15 at n = 64, L = 12, alpha = 3: device error {err:.3e}, restatement error {ref_err:.3e}, fit error {fit:.3e}, levels {plan.levels}")
    assert err <= 4 * ref_err
    with pytest.raises(NotImplementedError):
        ct.eval_chebyshev(plan, e2e["rlk"])
    # lincomb on the deep chain, by its Python surface: 2 x - 1 at the target scale, no level used
    two = ck.lincomb([ct], [2.0], consts=[-1.0])[0]
    ww, kk = DP.lin_weights([[2.0]], [-1.0], delta, [delta], mods)
    assert isinstance(two, ck.DeepCiphertext) and (two.level, two.scale) == (L - 1, delta) and np.array_equal(_u64(two.d), DP.lincomb(mods, [ct_ref], ww, kk)[0])


def test_inner_product_of_eight_pairs_through_dot(pkg, tab, e2e):
    """ckks.dot over 8 fresh pairs, rescaled: word-equal to the restatement and decoding to sum_r x_r y_r under the same rule"""
    ck = pkg.ckks
    n, L, delta, mods, sps, key = e2e["n"], e2e["L"], e2e["delta"], e2e["mods"], e2e["sps"], e2e["key"]
    rows, count = 2, 8
    r = np.random.default_rng(E2E_RNG + 1)
    zs = [r.uniform(-1, 1, (rows, n // 2)) + 1j * r.uniform(-1, 1, (rows, n // 2)) for _ in range(2 * count)]
    msgs = [K.encode(z, delta) for z in zs]
    refs, cts = [], []
    for m in msgs:
        refs.append(E.encrypt(E2E_SEED, key._next_row, e2e["pk_ref"], m, rows, mods, tab))   # the rows the next encryption takes
        cts.append(key.encrypt(e2e["pk"], m))
        assert isinstance(cts[-1], ck.DeepCiphertext) and np.array_equal(_u64(cts[-1].d), refs[-1])
    xs, ys = cts[:count], cts[count:]
    res = ck.dot(xs, ys, e2e["rlk"])
    want_words = DP.dot(mods, sps, e2e["rlk_ref"], list(zip(refs[:count], refs[count:])), None)
    assert isinstance(res, ck.DeepCiphertext) and (res.level, res.scale) == (L - 1, delta * delta) and np.array_equal(_u64(res.d), want_words)
    out, out_ref = res.rescale(), D.rescale(mods, want_words)
    assert out.level == L - 2 and np.array_equal(_u64(out.d), out_ref)
    weighted = ck.dot(xs[:3], ys[:3], e2e["rlk"], coeffs=[1, -2, 3])
    w = DP.dot_weights([1, -2, 3], delta * delta, [delta * delta] * 3, mods)
    assert np.array_equal(_u64(weighted.d), DP.dot(mods, sps, e2e["rlk_ref"], list(zip(refs[:3], refs[count:count + 3])), w))
    want = sum(a * b for a, b in zip(zs[:count], zs[count:]))
    dec_ref = E.decrypt(mods[:1], n, e2e["s"], out_ref[:1])
    low = out.at_level(0)
    assert np.array_equal(key.decrypt(low), dec_ref)
    ref_err = float(np.abs(K.decode(dec_ref, out.scale) - want).max())
    err = float(np.abs(key.decrypt_and_decode(low) - want).max())
    print(f"sum of 8 products at n = 64, L = 12, alpha = 3: device error {err:.3e}, restatement error {ref_err:.3e}")
    assert err <= 4 * ref_err
