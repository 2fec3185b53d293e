"""BFV on the RNS chain on the device (bfv_rns.hip) where the tests that came with it do not reach: the
case lists of tests/_bfv_rns_shapes_cases.py, which tests/test_bfv_rns_shapes_cpu.py proves, word for word against the
restatements (tests/_bfv_rns_numpy.py, tests/_bfv_dot_numpy.py, tests/_ckks_eval_numpy.py).  Every comparison is exact equality
of integer words; outputs sit between sentinel words where alignment or extent is the point.

    A  test_decrypt_word_for_word, test_decrypt_across_its_chunk, test_scale_msg_word_for_word, test_client_rejections
    B  test_extend_mixed_bases, test_extend_second_trip_of_the_grid
    C  test_k3_against_the_definition, test_primes_at_the_limit, test_mixed_chain, test_two_pass_sizes,
       test_workspace_bytes_at_the_clamp, test_alignment, test_client_kernels_misaligned, test_slot_13_grows_between_calls,
       test_two_streams_interleaved

Measured on an MI355X box (pytest --durations, restatement included): 88 cases in 8.3 s; 1.6 s for whichever runs first (it loads
the library and the device), 1.0 - 1.4 s for k = 3 at n = 2048, 0.7 s for the 2^16 products, 0.65 s for the decryption across
its chunk, 0.46 s for the 2^14 products, 0.33 s each for the two workspace tests, 0.2 s and less for every other case.

No call of the sweep gave a wrong word."""
import time

import numpy as np
import pytest

import _bfv_dot_numpy as D
import _bfv_rns_numpy as R
import _bfv_rns_shapes_cases as S
import _ckks_eval_numpy as E
import _ckks_shapes_cases as CS
import _client_numpy as C
from test_bfv_dot_gpu import _case, _timer_rows
from test_bfv_rns_gpu import _device_key, _empty, _operands, _plans
from test_bootstrap_gpu import _dev, _u64
from test_client_alignment_gpu import Offset

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A
T = S.T


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _sync():
    import torch

    torch.cuda.synchronize()


def _ready(stream):
    """the copies into the buffers ran on the default stream: a created stream waits for them on the device, the host does not
    wait; -> the handle the entry points take"""
    import torch

    if stream is None:
        return None
    stream.wait_stream(torch.cuda.current_stream())
    return stream.cuda_stream


def _buf(x, mis=False):
    x = np.ascontiguousarray(x, dtype=U64)
    return Offset(x.shape, x, lead=1 if mis else 2)


def _out(shape, mis=False):
    return Offset(tuple(shape), lead=1 if mis else 2)


# ---- A: the client kernels, directly ---------------------------------------------------------------------------------------------------
def _decrypt(pkg, mods, n, b0, t, s, ct, mis=(False, False, False)):
    batch = ct.shape[2]
    ds, dc, o = _buf(s, mis[0]), _buf(ct, mis[1]), _out((batch, n), mis[2])
    _sync()
    pkg.binding.bfv_rns_decrypt_dev(_plans(pkg, mods, n), b0, t, ds.ptr, dc.ptr, o.ptr, batch)
    _sync()
    assert np.array_equal(ds.get(), s) and np.array_equal(dc.get(), ct), "an input was written"
    return o.get().copy()


@pytest.mark.parametrize("n,k", S.DECRYPT_SHAPES)
def test_decrypt_word_for_word(pkg, n, k):
    """fhe_bfv_rns_decrypt_dev against R.decrypt_phase on phases known by construction, every rounding edge planted, under every
    (t, b_0) of S.decrypt_params: b_0 = 2 t + 3, t = 2, t even, and t = 2^60 - 1 at k = 2"""
    mods = R.chain(n, k)[0]
    Q = R.prod(mods)
    for t, b0 in S.decrypt_params(k):
        batch = S.decrypt_batch(n, len(S.planted_phases(Q, t)))
        rows = S.phase_rows(Q, t, n, batch, 100 * n + k)
        s, ct = S.ct_of_phase(mods, n, rows, 100 * n + k + 1)
        got = _decrypt(pkg, mods, n, b0, t, s, ct)
        want = R.decrypt_phase(mods, t, rows)
        assert np.array_equal(got, want), (t, b0, np.argwhere(got != want)[:8].tolist())


def test_decrypt_across_its_chunk(pkg):
    """(2^16, 3, 11): the decrypt's own chunk is 2^21 / (k n) = 10 rows, so 10 + 1; primes just above 2^30.  The restatement
    (the rows, their evals and R.decrypt_phase) took 0.60 s of the case's 0.65 s on an MI355X box."""
    n, k, batch, t, b0 = S.DECRYPT_CHUNK
    mods = S.small_chain(n, k)[0]
    assert S.chunks_of(batch, R.decrypt_chunk_rows(n, k, batch)) == [10, 1]
    t0 = time.time()
    rows = S.phase_rows(R.prod(mods), t, n, batch, 7)
    s, ct = S.ct_of_phase(mods, n, rows, 8)
    want = R.decrypt_phase(mods, t, rows)
    print("decrypt chunk: restatement %.2f s" % (time.time() - t0))
    got = {}
    rows_seen = _timer_rows(pkg.binding, lambda: got.update(m=_decrypt(pkg, mods, n, b0, t, s, ct)))
    assert np.array_equal(got["m"], want), np.argwhere(got["m"] != want)[:8].tolist()
    assert rows_seen["bfv_rns_decrypt"] == 2 and rows_seen["bfv_rns_phase"] == 2 * k, rows_seen


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [2, 64])
@pytest.mark.parametrize("batch", [1, 3])
def test_scale_msg_word_for_word(pkg, k, n, batch):
    """fhe_bfv_rns_scale_msg_dev on any 64-bit word: floor(Q / t) x mod q_i, centred; t = 2, 65537, Q - 1 and Q (k = 1), 2^64 - 59 (k = 2)"""
    mods = R.chain(n, k)[0]
    for t in S.scale_msg_moduli(k, R.prod(mods)):
        m = S.messages(t, batch, n, 10 * k + batch)
        dm, o = _buf(m), _out((k, batch, n))
        pkg.binding.bfv_rns_scale_msg_dev(_plans(pkg, mods, n), t, dm.ptr, o.ptr, batch)
        _sync()
        assert np.array_equal(o.get(), R.scale_msg(mods, t, m).view(U64)), t
        assert np.array_equal(dm.get(), m)


def test_client_rejections(pkg):
    """every branch of the argument checks of fhe_bfv_rns_decrypt_dev and fhe_bfv_rns_scale_msg_dev, in source order; the
    outputs hold FILL after each"""
    B = pkg.binding
    n, k, batch, t, b0 = 64, 2, 3, 257, 517
    mods = R.chain(n, k)[0]
    Q = R.prod(mods)
    plans = _plans(pkg, mods, n)
    s, ct = S.ct_of_phase(mods, n, S.phase_rows(Q, t, n, batch, 1), 2)
    msg = S.messages(t, batch, n, 3)
    ds, dc, dm = _dev(s), _dev(ct), _dev(msg)
    out, mout = _empty((batch, n)), _empty((k, batch, n))
    Sp, Cp, O, M, MO = ds.data_ptr(), dc.data_ptr(), out.data_ptr(), dm.data_ptr(), mout.data_ptr()

    def untouched():
        assert np.all(_u64(out) == U64(FILL)) and np.all(_u64(mout) == U64(FILL))
        assert np.array_equal(_u64(ds), s) and np.array_equal(_u64(dc), ct) and np.array_equal(_u64(dm), msg)

    def dec(code, p=plans, aux=b0, tt=t, sp=Sp, cp=Cp, o=O, b=batch, **kw):
        with pytest.raises(B.FheError) as e:
            B.bfv_rns_decrypt_dev(p, aux, tt, sp, cp, o, b, **kw)
        assert e.value.code == code, e.value
        untouched()

    def msc(code, p=plans, tt=t, m=M, o=MO, b=batch, **kw):
        with pytest.raises(B.FheError) as e:
            B.bfv_rns_scale_msg_dev(p, tt, m, o, b, **kw)
        assert e.value.code == code, e.value
        untouched()

    wide = pkg.Plan(E.primes_below(63, n, 1)[0], n)
    for both in (dec, msc):
        both(B.FHE_E_NULL, p=None, limbs=k)
        both(B.FHE_E_INVALID, limbs=0)
        both(B.FHE_E_INVALID, p=plans[:1] * 5)
        both(B.FHE_E_NULL, p=[plans[0], None])
        both(B.FHE_E_PARAM_MISMATCH, p=[plans[0], pkg.Plan(mods[1], n // 2)])
        both(B.FHE_E_INVALID, p=[plans[0], wide])                    # a modulus not below 2^62
        both(B.FHE_E_INVALID, p=[plans[0], plans[0]])                # repeated
        both(B.FHE_E_INVALID, tt=1)
        both(B.FHE_E_INVALID, tt=0)
    q0 = mods[0]
    msc(B.FHE_E_INVALID, p=plans[:1], tt=q0 + 1)                     # t = Q + 1 at k = 1: floor(Q / t) = 0
    dec(B.FHE_E_INVALID, aux=2 * t + 4)                              # even
    dec(B.FHE_E_INVALID, aux=2 * t + 2)
    dec(B.FHE_E_INVALID, aux=2 * t + 1)
    dec(B.FHE_E_INVALID, aux=(1 << 62) + 1)
    dec(B.FHE_E_INVALID, aux=S.B0_T60, tt=1 << 60)
    dec(B.FHE_E_INVALID, aux=q0)                                     # not coprime to Q
    for kw in (dict(sp=None), dict(cp=None), dict(o=None)):
        dec(B.FHE_E_NULL, **kw)
    for kw in (dict(m=None), dict(o=None)):
        msc(B.FHE_E_NULL, **kw)
    for kw in (dict(sp=Sp + 4), dict(cp=Cp + 4), dict(o=O + 4)):
        dec(B.FHE_E_INVALID, **kw)
    for kw in (dict(m=M + 4), dict(o=MO + 4)):
        msc(B.FHE_E_INVALID, **kw)
    dec(B.FHE_E_INVALID, o=Sp)                                       # the output over the key: one row over k rows of n words
    dec(B.FHE_E_INVALID, o=Sp + 8 * (k * n - 1), b=1)                # ... over its last word
    dec(B.FHE_E_INVALID, o=Cp + 8 * n)                               # ... inside the ciphertexts
    dec(B.FHE_E_INVALID, sp=O + 8 * (batch * n - 1))                 # the key begins on the output's last word
    msc(B.FHE_E_INVALID, o=M)
    msc(B.FHE_E_INVALID, m=MO + 8 * (k * batch * n - 1), b=batch)    # the messages begin on the output's last word
    B.bfv_rns_decrypt_dev(plans, b0, t, Sp, Cp, O, 0)                # batch = 0: a no-op after the checks
    B.bfv_rns_decrypt_dev(plans, 2 * t + 3, t, None, None, None, 0)
    B.bfv_rns_scale_msg_dev(plans, t, M, MO, 0)
    B.bfv_rns_scale_msg_dev(plans[:1], q0, None, None, 0)            # t = Q is admitted
    _sync()
    untouched()


# ---- B: the extension at its edges -------------------------------------------------------------------------------------------------------
def _extend(pkg, src, dst, centred, res, mis=False):
    count = res.shape[1]
    din, o = _buf(res, mis), _out((len(dst), count), mis)
    pkg.binding.rns_extend_dev(src, dst, centred, din.ptr, o.ptr, count)
    _sync()
    assert np.array_equal(din.get(), res)
    return o.get().copy()


@pytest.mark.parametrize("s", sorted(S.EXT_BASES))
@pytest.mark.parametrize("order", S.EXT_ORDERS)
@pytest.mark.parametrize("centred", [False, True])
def test_extend_mixed_bases(pkg, s, order, centred):
    """sources and targets from 3 to 62 bits in one call, small before large and large before small; 257 integers with the
    planted ones of S.planted_integers first, and the first four again one a call"""
    src, dst = S.ext_base(s, order)
    xs = S.ext_integers(src, S.EXT_COUNT, 100 * s)
    res = np.array([[x % m for x in xs] for m in src], dtype=U64)
    want = S.ext_want(src, dst, xs, centred)
    got = _extend(pkg, src, dst, centred, res, mis=centred)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    for e in range(4):
        assert np.array_equal(_extend(pkg, src, dst, centred, res[:, e:e + 1]), want[:, e:e + 1]), e


@pytest.mark.parametrize("centred", [False, True])
def test_extend_second_trip_of_the_grid(pkg, centred):
    """4096 * 256 + 3 integers, two sources (3 and a 62-bit prime, M < 2^64), two targets: the grid-stride loop's second trip"""
    src, dst, count = S.STRIDE
    M = R.prod(src)
    x = np.random.default_rng(3).integers(0, M, count, dtype=np.uint64)
    x[:4], x[-3:] = np.array([0, M - 1, M // 2, M // 2 + 1], dtype=U64), np.array([M // 2 + 1, M // 2, M - 1], dtype=U64)
    res = np.stack([x % U64(m) for m in src])
    want = np.stack([np.where(x > U64(M // 2), (x % U64(p) + U64(p - M % p)) % U64(p), x % U64(p)) if centred else x % U64(p) for p in dst])
    assert [int(v) for v in want[:, :4].T.reshape(-1)] == [int(v) for v in S.ext_want(src, dst, [0, M - 1, M // 2, M // 2 + 1], centred).T.reshape(-1)]
    got = _extend(pkg, src, dst, centred, res)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()


# ---- C: tensor, mul and dot where they have not been -----------------------------------------------------------------------------------
class Chain:
    """the three products over one chain; every buffer is an Offset between sentinels, misaligned by a word where asked"""

    def __init__(self, pkg, mods, aux, P, n, t, rlk):
        self.B, self.n, self.t, self.k = pkg.binding, n, t, len(mods)
        self.plans, self.ap, self.sp = _plans(pkg, mods, n), _plans(pkg, aux, n), pkg.Plan(P, n)
        self.rlk = np.ascontiguousarray(rlk, dtype=U64)
        self.d_rlk = _dev(self.rlk)

    def _take(self, o, ins, stream):
        if stream is None:
            _sync()
            for d, x in ins:
                assert np.array_equal(d.get(), x), "an input was written"
            return o.get().copy()
        return o, ins

    def tensor(self, a, b, mis="", stream=None):
        batch = a.shape[2]
        da, db, o = _buf(a, "a" in mis), _buf(b, "b" in mis), _out((self.k, 3, batch, self.n), "o" in mis)
        self.B.bfv_rns_tensor_dev(self.plans, self.ap, self.t, da.ptr, db.ptr, o.ptr, batch, _ready(stream))
        return self._take(o, [(da, a), (db, b)], stream)

    def mul(self, a, b, mis="", stream=None):
        batch = a.shape[2]
        da, db, o = _buf(a, "a" in mis), _buf(b, "b" in mis), _out(a.shape, "o" in mis)
        self.B.bfv_rns_mul_dev(self.plans, self.ap, self.sp, self.t, self.d_rlk.data_ptr(), da.ptr, db.ptr, o.ptr, batch, _ready(stream))
        return self._take(o, [(da, a), (db, b)], stream)

    def dot(self, pool, pairs, w, mis="", stream=None):
        """pool [a, b, ...]; "a" in mis misaligns pool[0], "b" the others"""
        batch = pool[0].shape[2]
        dev = [_buf(x, ("a" if i == 0 else "b") in mis) for i, x in enumerate(pool)]
        o = _out(pool[0].shape, "o" in mis)
        self.B.bfv_rns_dot_dev(self.plans, self.ap, self.sp, self.t, self.d_rlk.data_ptr(), [dev[x].ptr for x, _ in pairs], [dev[y].ptr for _, y in pairs], w,
                               o.ptr, batch, _ready(stream))
        return self._take(o, list(zip(dev, pool)), stream)


def _chain_with_device_key(pkg, tab, mods, aux, P, n, t, row):
    return Chain(pkg, mods, aux, P, n, t, _u64(_device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * row)))


def _check_products(ch, mods, P, t, a, b):
    want = R.tensor(mods, t, a, b)
    got = ch.tensor(a, b)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert np.array_equal(ch.mul(a, b), E.relinearize(mods, P, ch.rlk, want))


@pytest.mark.parametrize("n,batch", S.K3)
def test_k3_against_the_definition(pkg, tab, n, batch):
    """k = 3, what the benchmark and both rate tools run: tensor, mul and dot on the bound-reaching rows of _operands"""
    mods, aux, P = R.chain(n, 3)
    ch = _chain_with_device_key(pkg, tab, mods, aux, P, n, T, 20)
    a, b = _operands(mods, n, batch, 3000 * n + batch)
    _check_products(ch, mods, P, T, a, b)
    for count, mode in S.k3_dots(n, batch):
        pool, pairs, w = _case(mods, n, batch, count, mode, 3000 * n + 10 * batch + count)
        assert D.admitted(mods, aux, T, n, D.weight_sum(count, w))
        assert np.array_equal(ch.dot(pool, pairs, w), D.dot(mods, P, T, ch.rlk, [(pool[x], pool[y]) for x, y in pairs], w)), (count, mode)


@pytest.mark.parametrize("k", [1, 4])
def test_primes_at_the_limit(pkg, tab, k):
    """chain, base and special prime all just below 2^62, the documented limit"""
    n, batch = 64, 3
    mods, aux, P = S.limit_chain(n, k)
    assert R.admitted(mods, aux, T, n) and min(mods + aux + [P]) > 1 << 61
    ch = _chain_with_device_key(pkg, tab, mods, aux, P, n, T, 21)
    a, b = _operands(mods, n, batch, 62 + k)
    _check_products(ch, mods, P, T, a, b)
    assert np.array_equal(ch.dot([a, b], [(0, 1), (1, 1)], [3, -2]), D.dot(mods, P, T, ch.rlk, [(a, b), (b, b)], [3, -2]))


def test_mixed_chain(pkg, tab):
    """a 30-bit beside a 61-bit chain prime, a base of 30, 61 and 62 bits: the digits of one size reduced modulo the other"""
    n, batch = 64, 3
    mods, aux, P = S.mixed_chain(n)
    assert R.admitted(mods, aux, T, n)
    ch = _chain_with_device_key(pkg, tab, mods, aux, P, n, T, 22)
    a, b = _operands(mods, n, batch, 30)
    _check_products(ch, mods, P, T, a, b)
    _check_products(Chain(pkg, mods[::-1], aux[::-1], P, n, T, ch.rlk[::-1][:, [1, 0, 2]]), mods[::-1], P, T, a[::-1], b[::-1])


_BIG = {}


def _big(n, k, batch):
    if n not in _BIG:
        t0 = time.time()
        case = S.BigCase(n, k, batch, n + k)
        case.rlk = CS.random_key(case.mods, case.P, n, n + 1)
        case.want = case.tensor()
        case.build_s = time.time() - t0
        _BIG[n] = case
    return _BIG[n]


@pytest.mark.parametrize("n,k,batch,chunks", S.TWO_PASS)
def test_two_pass_sizes(pkg, n, k, batch, chunks):
    """n = 2^14 (chunks of 2 + 1 rows, a ragged tail) and n = 2^16 (the quotient 2^21 / (49 n) is zero: clamped to chunks of
    one): the transforms are the two-pass engines, in place on workspace rows of 2 cr, 3 cr and 4 cr polynomials.  The operands
    are a sparse ciphertext (four coefficients, +-floor(Q / 2) among them) times a dense uniform one, so the product over Z
    costs O(4 n); every eval of both is dense.  The key is uniform canonical words.  Measured on an MI355X box, the
    restatement alone: operands and tensor 0.17 s (2^14) and 0.47 s (2^16), the relinearisation 0.05 s and 0.16 s, the dot at
    2^14 0.20 s; the cases 0.46 s and 0.70 s in all."""
    case = _big(n, k, batch)
    mods, aux, P, t = case.mods, case.aux, case.P, case.t
    assert R.admitted(mods, aux, t, n) and S.chunks_of(batch, R.chunk_rows(n, k, batch)) == chunks
    ch = Chain(pkg, mods, aux, P, n, t, case.rlk)
    got = {}
    rows = _timer_rows(pkg.binding, lambda: got.update(d=ch.tensor(case.a, case.b)))
    assert np.array_equal(got["d"], case.want), np.argwhere(got["d"] != case.want)[:8].tolist()
    assert rows["bfv_rns_scale"] == len(chunks) and rows["rns_extend"] == len(chunks), rows
    t0 = time.time()
    want = E.relinearize(mods, P, case.rlk, case.want)
    relin_s = time.time() - t0
    rows = _timer_rows(pkg.binding, lambda: got.update(m=ch.mul(case.a, case.b)))
    assert np.array_equal(got["m"], want)
    assert rows["bfv_rns_scale"] == len(chunks), rows
    print("two-pass n=%d: restatement operands+tensor %.2f s, relinearisation %.2f s" % (n, case.build_s, relin_s))
    if n == 1 << 14:
        w = S.DOT_WEIGHTS
        assert D.admitted(mods, aux, t, n, sum(map(abs, w)))
        t0 = time.time()
        want = E.relinearize(mods, P, case.rlk, case.tensor(w))
        print("two-pass n=%d: restatement of the dot %.2f s" % (n, time.time() - t0))
        rows = _timer_rows(pkg.binding, lambda: got.update(s=ch.dot([case.a, case.a2, case.b], [(0, 2), (1, 2)], w)))
        assert np.array_equal(got["s"], want)
        assert rows["bfv_rns_scale"] == len(chunks) and rows["bfv_rns_tensorsum"] == 2 * len(chunks), rows


def test_workspace_bytes_at_the_clamp(pkg):
    """at n = 2^16 the workspace is sized from the clamped chunk of one ciphertext, not from the quotient (zero from k = 2 on)"""
    B = pkg.binding
    n = 1 << 16
    for k in (1, 2, 3, 4):
        for batch in (1, 2, 5):
            assert R.chunk_rows(n, k, batch) == 1
            assert B.bfv_rns_workspace_bytes(n, k, batch) == 8 * 7 * (2 * k + 1) * n + B.ckks_rns_galois_workspace_bytes(n, k, 1, 1) > 0
    n, k, batch = 1 << 14, 3, 3                                      # the ragged shape: sized from the full chunk of 2
    assert B.bfv_rns_workspace_bytes(n, k, batch) == 8 * 7 * (2 * k + 1) * n * 2 + B.ckks_rns_galois_workspace_bytes(n, k, 2, 1)


# -- buffers 8-byte but not 16-byte aligned ------------------------------------------------------------------------------------------------
_ALIGN = {}


def _align_data(pkg, tab, n, k, batch):
    if n not in _ALIGN:
        (mods, aux, P), t = S.align_chain(n, k)
        ch = _chain_with_device_key(pkg, tab, mods, aux, P, n, t, 23)
        if n == 64:
            a, b = _operands(mods, n, batch, 64)
        else:
            rng = np.random.default_rng(5)
            a, b = (np.stack([rng.integers(0, q, (2, batch, n)).astype(U64) for q in mods]) for _ in range(2))
        run = {"tensor": lambda mis: ch.tensor(a, b, mis), "mul": lambda mis: ch.mul(a, b, mis),
               "dot": lambda mis: ch.dot([a, b], [(0, 1), (1, 1)], [3, -2], mis)}
        aligned = {what: fn("") for what, fn in run.items()}
        if n == 64:                                                  # the aligned run itself against the definition where that is cheap
            want = R.tensor(mods, t, a, b)
            assert np.array_equal(aligned["tensor"], want) and np.array_equal(aligned["mul"], E.relinearize(mods, P, ch.rlk, want))
            assert np.array_equal(aligned["dot"], D.dot(mods, P, t, ch.rlk, [(a, b), (b, b)], [3, -2]))
        _ALIGN[n] = (ch, a, b, run, aligned)
    return _ALIGN[n]


@pytest.mark.parametrize("what", ["tensor", "mul", "dot"])
@pytest.mark.parametrize("mode", S.ALIGN_MODES)
@pytest.mark.parametrize("n,k,batch", S.ALIGN_SHAPES)
def test_alignment(pkg, tab, n, k, batch, mode, what):
    """a, b, both, or every buffer one word past a 16-byte boundary: the words of the aligned run, the sentinels either side of
    the output intact, the inputs unchanged.  (64, 2, 3) is one chunk (inverse_into takes both components in one call),
    (8192, 4, 5) chunks of 4 + 1 (a call a component).  fhe_bfv_rns_tensor_dev wants its output 16-byte aligned, mul and dot
    do not: an offset output is refused there and nothing is written."""
    ch, a, b, run, aligned = _align_data(pkg, tab, n, k, batch)
    mis = {"a": "a", "b": "b", "ab": "ab", "all": "abo"}[mode]
    if what == "tensor" and mode == "all":
        da, db, o = _buf(a, True), _buf(b, True), _out((k, 3, batch, n), True)
        with pytest.raises(pkg.binding.FheError) as e:
            pkg.binding.bfv_rns_tensor_dev(ch.plans, ch.ap, ch.t, da.ptr, db.ptr, o.ptr, batch)
        _sync()
        assert e.value.code == pkg.binding.FHE_E_INVALID and np.all(o.get() == U64(FILL))
        return
    got = run[what](mis)
    assert np.array_equal(got, aligned[what]), (what, mode, np.argwhere(got != aligned[what])[:8].tolist())


def test_client_kernels_misaligned(pkg):
    """fhe_bfv_rns_decrypt_dev and fhe_bfv_rns_scale_msg_dev with each buffer in turn, and all, one word past a 16-byte boundary"""
    n, k, batch, t, b0 = 64, 2, 3, 257, 517
    mods = R.chain(n, k)[0]
    rows = S.phase_rows(R.prod(mods), t, n, batch, 4)
    s, ct = S.ct_of_phase(mods, n, rows, 5)
    want = R.decrypt_phase(mods, t, rows)
    for mis in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        assert np.array_equal(_decrypt(pkg, mods, n, b0, t, s, ct, mis), want), mis
    m = S.messages(t, batch, n, 6)
    want = R.scale_msg(mods, t, m).view(U64)
    for mis in ((True, False), (False, True), (True, True)):
        dm, o = _buf(m, mis[0]), _out((k, batch, n), mis[1])
        pkg.binding.bfv_rns_scale_msg_dev(_plans(pkg, mods, n), t, dm.ptr, o.ptr, batch)
        _sync()
        assert np.array_equal(o.get(), want) and np.array_equal(dm.get(), m), mis


# -- workspace slot 13 and streams ------------------------------------------------------------------------------------------------------------
def _reuse_data(pkg, tab):
    n, k = S.REUSE["n"], S.REUSE["k"]
    mods, aux, P = R.chain(n, k)
    t, b0 = 257, 517
    rows = S.phase_rows(R.prod(mods), t, n, S.REUSE["decrypt_batch"], 11)
    s, ct = S.ct_of_phase(mods, n, rows, 12)
    ch = _chain_with_device_key(pkg, tab, mods, aux, P, n, T, 24)
    a, b = _operands(mods, n, S.REUSE["mul_batch"], 13)
    a2, b2 = _operands(mods, n, S.REUSE["mul_batch"], 14)
    return dict(mods=mods, P=P, n=n, t=t, b0=b0, s=s, ct=ct, m=R.decrypt_phase(mods, t, rows), ch=ch, a=a, b=b, a2=a2, b2=b2)


def test_slot_13_grows_between_calls(pkg, tab):
    """on the default stream: a decryption (k cb n words of slot 13), a product (7 (2k + 1) cb n), the same decryption, a dot"""
    d = _reuse_data(pkg, tab)
    ch, mods, P = d["ch"], d["mods"], d["P"]
    assert np.array_equal(_decrypt(pkg, mods, d["n"], d["b0"], d["t"], d["s"], d["ct"]), d["m"])
    assert np.array_equal(ch.mul(d["a"], d["b"]), E.relinearize(mods, P, ch.rlk, R.tensor(mods, T, d["a"], d["b"])))
    assert np.array_equal(_decrypt(pkg, mods, d["n"], d["b0"], d["t"], d["s"], d["ct"]), d["m"])
    assert np.array_equal(ch.dot([d["a2"], d["b2"]], [(0, 1), (1, 1)], [3, -2]), D.dot(mods, P, T, ch.rlk, [(d["a2"], d["b2"]), (d["b2"], d["b2"])], [3, -2]))


class OwnStream:
    """A non-blocking stream made through the HIP runtime the process has loaded, outside torch's ring of 32 pooled handles: a
    pooled handle comes back to a later test with whatever workspaces this module left on it, and taking two moves every later
    test two handles on.  Its workspaces go back to the library before it is destroyed, as include/fhe_ntt.h asks."""

    def __init__(self, pkg):
        import ctypes

        import torch

        with open("/proc/self/maps") as f:
            path = next(line.split()[-1] for line in f if "libamdhip64" in line)
        self.hip, self.pkg = ctypes.CDLL(path), pkg
        h = ctypes.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0 and h.value      # hipStreamNonBlocking
        self.handle, self.torch = h.value, torch.cuda.ExternalStream(h.value)
        self.wait_stream, self.cuda_stream = self.torch.wait_stream, h.value

    def close(self):
        import ctypes

        self.torch.synchronize()
        self.pkg.binding._check(self.pkg.load_library().fhe_ntt_release_stream_workspace(ctypes.c_void_p(self.handle)))
        assert self.hip.hipStreamDestroy(ctypes.c_void_p(self.handle)) == 0


def test_two_streams_interleaved(pkg, tab):
    """a product on one created stream and a dot on another, on different operands, both issued before either is waited for.
    The contract (include/fhe_ntt.h): "Entry points that need intermediates use a library-owned workspace keyed by (device,
    stream, calling thread): a thread's calls on a stream are ordered by the stream, and no two threads or streams ever share a
    buffer" - so concurrent use of slot 13 from two streams is the library's to get right, and this is that test."""
    d = _reuse_data(pkg, tab)
    ch, mods, P = d["ch"], d["mods"], d["P"]
    held = pkg.load_library().fhe_ntt_workspace_bytes()
    one, two = OwnStream(pkg), OwnStream(pkg)
    for st in (one, two):                                            # a first call a stream: its workspaces are allocated here
        ch.mul(d["a"], d["b"], stream=st)
    _sync()
    calls = []
    for _ in range(2):
        calls.append((ch.mul(d["a"], d["b"], stream=one), ch.dot([d["a2"], d["b2"]], [(0, 1), (1, 1)], [3, -2], stream=two)))
    _sync()
    want_mul = E.relinearize(mods, P, ch.rlk, R.tensor(mods, T, d["a"], d["b"]))
    want_dot = D.dot(mods, P, T, ch.rlk, [(d["a2"], d["b2"]), (d["b2"], d["b2"])], [3, -2])
    for (om, im), (od, idot) in calls:
        assert np.array_equal(om.get(), want_mul) and np.array_equal(od.get(), want_dot)
        assert all(np.array_equal(x.get(), y) for x, y in im + idot)
    one.close()
    two.close()
    assert pkg.load_library().fhe_ntt_workspace_bytes() == held      # what the two streams took is back
