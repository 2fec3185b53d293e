"""BFV inner products, scalar sums and linear transforms on the RNS chain on the device (bfv_rns.hip):
fhe_bfv_rns_dot_dev word for word against tests/_bfv_dot_numpy.py (tolerance zero: everything is integer), one pair against
fhe_bfv_rns_mul_dev, a batch across a chunk, a second stream, every rejection with its output untouched, the launch counts, and
the Python surface (bfv.dot, square, lincomb, mul_const, diag_sum, linear_transform) end to end at n = 64, t = 257, k = 2."""
import numpy as np
import pytest

import _bfv_dot_numpy as D
import _bfv_rns_numpy as R
import _ckks_eval_numpy as E
import _client_numpy as C
from test_bfv_rns_gpu import SEED, _device_key, _empty, _operands, _plans
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A
T = 65537
MODES = ("null", "ones", "signed")


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _negated(mods, ct):
    """-ct: every eval q - x"""
    return np.stack([(U64(q) - ct[i]) % U64(q) for i, q in enumerate(mods)])


def _case(mods, n, batch, count, mode, seed):
    """-> (pool, pairs, w): `pool` distinct ciphertexts [k][2][batch][n] (with batch = 3 their rows 1 and 2 are the polynomials of
    +-floor(Q / 2) that reach the bound), `pairs` index pairs into it and the weights.  Pair 0 is a square where there is more
    than one pair, and the pointers repeat across pairs once count passes the pool.  Under signed weights the second operand of
    a pair of negative weight is the negated ciphertext, so that every pair pushes the bound rows the same way: |D| reaches
    W n Q^2 / 2 (to the rounding of floor(Q / 2)) with mixed signs too."""
    a, b = _operands(mods, n, batch, seed)
    w = {"null": None, "ones": [1] * count, "signed": D.signed_weights(count, T, seed)}[mode]
    pool = [a, b, _negated(mods, b), _negated(mods, a)]
    pairs = []
    for r in range(count):
        x, y = (0, 0) if (r == 0 and count > 1) else (r % 2, (r + 1) % 2)
        if w is not None and w[r] < 0:
            y = 2 if y == 1 else 3                                   # b -> -b, a -> -a
        pairs.append((x, y))
    return pool, pairs, w


def _run_dot(pkg, mods, aux, P, n, t, d_rlk, pool, pairs, w, stream=None):
    batch = pool[0].shape[2]
    dev = [_dev(x) for x in pool]
    out = _empty(pool[0].shape)
    pkg.binding.bfv_rns_dot_dev(_plans(pkg, mods, n), _plans(pkg, aux, n), pkg.Plan(P, n), t, d_rlk.data_ptr(), [dev[x].data_ptr() for x, _ in pairs],
                                [dev[y].data_ptr() for _, y in pairs], w, out.data_ptr(), batch, stream)
    return out, dev


def _counts_and_modes(n, k, batch):
    """every count of {1, 2, 5, 9} under every weight mode at n = 2 and 8; at n = 64 every count with the mode rotating; at
    n = 2048, where the integer reference is the cost, one count a shape: 5 pairs for one row, 2 for three"""
    if n <= 8:
        return [(c, m) for c in (1, 2, 5, 9) for m in MODES]
    if n == 64:
        return [(c, MODES[(i + k + batch) % 3]) for i, c in enumerate((1, 2, 5, 9))]
    return [(5, MODES[k % 3])] if batch == 1 else [(2, MODES[(k + 1) % 3])]


@pytest.mark.parametrize("n", [2, 8, 64, 2048])
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("batch", [1, 3])
def test_dot_word_for_word(pkg, tab, n, k, batch):
    mods, aux, P = R.chain(n, k)
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 8)
    rlk = _u64(d_rlk)
    for count, mode in _counts_and_modes(n, k, batch):
        pool, pairs, w = _case(mods, n, batch, count, mode, 1000 * n + 100 * k + 10 * batch + count)
        assert D.admitted(mods, aux, T, n, D.weight_sum(count, w))
        out, _ = _run_dot(pkg, mods, aux, P, n, T, d_rlk, pool, pairs, w)
        want = D.dot(mods, P, T, rlk, [(pool[x], pool[y]) for x, y in pairs], w)
        assert np.array_equal(_u64(out), want), (count, mode)


def test_sixty_four_pairs(pkg, tab):
    n, k, batch, count = 8, 2, 1, 64
    mods, aux, P = R.chain(n, k)
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 9)
    pool, pairs, w = _case(mods, n, batch, count, "signed", 64)
    assert D.admitted(mods, aux, T, n, D.weight_sum(count, w))
    out, _ = _run_dot(pkg, mods, aux, P, n, T, d_rlk, pool, pairs, w)
    assert np.array_equal(_u64(out), D.dot(mods, P, T, _u64(d_rlk), [(pool[x], pool[y]) for x, y in pairs], w))


@pytest.mark.parametrize("n,k,batch", [(2, 1, 1), (64, 2, 3), (2048, 4, 3), (8192, 3, 2)])
def test_one_pair_is_mul(pkg, tab, n, k, batch):
    """one pair with w = NULL: the words of fhe_bfv_rns_mul_dev"""
    mods, aux, P = R.chain(n, k)
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 10)
    a, b = _operands(mods, n, batch, 5 * n + k)
    plans, ap, sp = _plans(pkg, mods, n), _plans(pkg, aux, n), pkg.Plan(P, n)
    da, db, want, got = _dev(a), _dev(b), _empty(a.shape), _empty(a.shape)
    pkg.binding.bfv_rns_mul_dev(plans, ap, sp, T, d_rlk.data_ptr(), da.data_ptr(), db.data_ptr(), want.data_ptr(), batch)
    pkg.binding.bfv_rns_dot_dev(plans, ap, sp, T, d_rlk.data_ptr(), [da.data_ptr()], [db.data_ptr()], None, got.data_ptr(), batch)
    assert np.array_equal(_u64(got), _u64(want))
    pkg.binding.bfv_rns_dot_dev(plans, ap, sp, T, d_rlk.data_ptr(), [da.data_ptr()], [db.data_ptr()], [1], got.data_ptr(), batch)
    assert np.array_equal(_u64(got), _u64(want))


def test_batch_across_a_chunk(pkg, tab):
    """n = 8192, k = 4: a chunk is 4 ciphertexts, so a batch of 5 takes two; small primes keep the integers short"""
    n, k, batch, t, count = 8192, 4, 5, 257, 2
    mods, aux, P = R.chain(n, k, bq=21, bb=30, bp=31)
    w = [3, -2]
    assert D.admitted(mods, aux, t, n, 5) and R.chunk_rows(n, k, batch) == 4
    rng = np.random.default_rng(3)
    a, b = (np.stack([rng.integers(0, q, (2, batch, n)).astype(U64) for q in mods]) for _ in range(2))
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 11)
    out, _ = _run_dot(pkg, mods, aux, P, n, t, d_rlk, [a, b], [(0, 1), (1, 1)], w)
    assert np.array_equal(_u64(out), D.dot(mods, P, t, _u64(d_rlk), [(a, b), (b, b)], w))


def test_second_stream(pkg, tab):
    import torch

    n, k, batch, count = 64, 2, 3, 5
    mods, aux, P = R.chain(n, k)
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 12)
    pool, pairs, w = _case(mods, n, batch, count, "signed", 31)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out, _ = _run_dot(pkg, mods, aux, P, n, T, d_rlk, pool, pairs, w, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(_u64(out), D.dot(mods, P, T, _u64(d_rlk), [(pool[x], pool[y]) for x, y in pairs], w))


def test_rejections_leave_the_output_untouched(pkg, tab):
    B = pkg.binding
    n, k, batch = 64, 2, 3
    mods, aux, P = R.chain(n, k)
    plans, ap, sp = _plans(pkg, mods, n), _plans(pkg, aux, n), pkg.Plan(P, n)
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 13)
    a, b = _operands(mods, n, batch, 41)
    da, db, out = _dev(a), _dev(b), _empty(a.shape)
    A, Bp, O, KEY = da.data_ptr(), db.data_ptr(), out.data_ptr(), d_rlk.data_ptr()
    before = (_u64(da).copy(), _u64(db).copy(), _u64(d_rlk).copy())

    def refused(code, *args, **kw):
        with pytest.raises(B.FheError) as e:
            B.bfv_rns_dot_dev(*args, **kw)
        assert e.value.code == code, e.value
        assert np.all(_u64(out) == U64(FILL))
        assert all(np.array_equal(x, y) for x, y in zip(before, (_u64(da), _u64(db), _u64(d_rlk))))

    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A], [Bp], None, O, batch, count=0)
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A] * 65, [Bp] * 65, None, O, batch)
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A, A], [Bp, Bp], [2, 0], O, batch)             # a zero weight
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A, A], [Bp, Bp], [2, 1 << 61], O, batch)       # |w| >= 2^61
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A, A], [Bp, Bp], [2, -(1 << 61)], O, batch)
    refused(B.FHE_E_NULL, plans, ap, sp, T, KEY, None, [Bp], None, O, batch, count=1)               # a NULL array
    refused(B.FHE_E_NULL, plans, ap, sp, T, KEY, [A], None, None, O, batch, count=1)
    refused(B.FHE_E_NULL, plans, ap, sp, T, KEY, [A, None], [Bp, Bp], None, O, batch)               # a NULL entry
    refused(B.FHE_E_NULL, plans, ap, sp, T, KEY, [A, A], [Bp, None], None, O, batch)
    refused(B.FHE_E_NULL, plans, ap, sp, T, None, [A], [Bp], None, O, batch)
    refused(B.FHE_E_NULL, plans, ap, sp, T, KEY, [A], [Bp], None, None, batch)
    refused(B.FHE_E_NULL, plans, None, sp, T, KEY, [A], [Bp], None, O, batch)
    refused(B.FHE_E_NULL, plans, ap, None, T, KEY, [A], [Bp], None, O, batch)
    refused(B.FHE_E_NULL, [plans[0], None], ap, sp, T, KEY, [A], [Bp], None, O, batch)
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A, A], [Bp, Bp], None, A, batch)               # the output is an operand
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A, A], [A, Bp], None, Bp + 8 * n, batch)       # ... inside the last one
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A], [Bp], None, KEY, batch)                    # ... the key
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A + 4], [Bp], None, O, batch)                  # misaligned
    refused(B.FHE_E_INVALID, plans, ap, sp, T, KEY, [A], [Bp], None, O + 4, batch)
    # the rejections of fhe_bfv_rns_mul_dev: a base below the admission, a repeated prime, t < 2, a small special prime
    refused(B.FHE_E_INVALID, plans, _plans(pkg, E.primes_below(40, n, k + 1), n), sp, T, KEY, [A], [Bp], None, O, batch)
    refused(B.FHE_E_INVALID, plans, [ap[0], ap[0], ap[1]], sp, T, KEY, [A], [Bp], None, O, batch)
    refused(B.FHE_E_INVALID, plans, [plans[0]] + ap[1:], sp, T, KEY, [A], [Bp], None, O, batch)
    refused(B.FHE_E_INVALID, plans, ap, sp, 1, KEY, [A], [Bp], None, O, batch)
    refused(B.FHE_E_INVALID, plans, ap, pkg.Plan(E.primes_below(30, n, 1)[0], n), T, KEY, [A], [Bp], None, O, batch)
    refused(B.FHE_E_INVALID, plans[:1] * 5, ap, sp, T, KEY, [A], [Bp], None, O, batch)              # limbs = 5
    # a base that admits `mul` but not this W: the boundary is 7 for this t
    m40, a41, P40 = R.chain(n, k, bq=40, bb=41)
    t_edge = (R.prod(a41) - 2) // (n * R.prod(m40)) // 7
    assert D.max_weight(m40, a41, t_edge, n) == 7
    p40, ap41, sp40 = _plans(pkg, m40, n), _plans(pkg, a41, n), pkg.Plan(P40, n)
    key40 = _device_key(pkg, tab, m40, P40, n, E.RLK_BASE + 64 * 14)
    small = _dev(np.zeros(a.shape, dtype=U64))
    S = small.data_ptr()
    refused(B.FHE_E_INVALID, p40, ap41, sp40, t_edge, key40.data_ptr(), [S] * 8, [S] * 8, None, O, batch)
    refused(B.FHE_E_INVALID, p40, ap41, sp40, t_edge, key40.data_ptr(), [S, S], [S, S], [4, -4], O, batch)
    B.bfv_rns_dot_dev(p40, ap41, sp40, t_edge, key40.data_ptr(), [S, S], [S, S], [3, -4], O, 0)     # batch = 0: a no-op
    B.bfv_rns_dot_dev(plans, ap, sp, T, KEY, [A], [Bp], None, O, 0)
    assert np.all(_u64(out) == U64(FILL))
    B.bfv_rns_dot_dev(p40, ap41, sp40, t_edge, key40.data_ptr(), [S] * 7, [S] * 7, None, O, batch)  # W = 7 is admitted: zeros in, zeros out
    assert not _u64(out).any()


# ---- the launch counts -------------------------------------------------------------------------------------------------------------------
def _timer_rows(B, fn):
    """{label: launches} of one call; the tag (log2 n) is dropped"""
    import torch

    torch.cuda.synchronize()
    B.kernel_timing_enable(True)
    B.kernel_timing_reset()
    try:
        fn()
        torch.cuda.synchronize()
        got = B.kernel_timing_read(256)
    finally:
        B.kernel_timing_enable(False)
    rows = {}
    for name, (_, c) in got.items():
        label = name.rsplit("_", 1)[0]
        rows[label] = rows.get(label, 0) + c
    return rows


@pytest.mark.parametrize("n,k,batch,count", [(64, 2, 3, 5), (64, 1, 1, 1), (8192, 4, 5, 3)])
def test_launch_counts(pkg, tab, n, k, batch, count):
    """bfv_rns_tensorsum once per pair and chunk, whatever k is; the extension once per pair and chunk; bfv_rns_scale once per
    chunk; and no launch of the per-limb tensor kernel.  One chunk of `mul` on the same shape takes 2k + 1 of those."""
    B = pkg.binding
    small = n == 8192
    mods, aux, P = R.chain(n, k, bq=21, bb=30, bp=31) if small else R.chain(n, k)
    t = 257 if small else T
    plans, ap, sp = _plans(pkg, mods, n), _plans(pkg, aux, n), pkg.Plan(P, n)
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 15)
    rng = np.random.default_rng(n + k)
    da = _dev(np.stack([rng.integers(0, q, (2, batch, n)).astype(U64) for q in mods]))
    out = _empty(tuple(da.shape))
    chunks = -(-batch // R.chunk_rows(n, k, batch))
    assert chunks == (2 if small else 1)
    w = None if count == 1 else list(range(1, count + 1))
    rows = _timer_rows(B, lambda: B.bfv_rns_dot_dev(plans, ap, sp, t, d_rlk.data_ptr(), [da.data_ptr()] * count, [da.data_ptr()] * count, w, out.data_ptr(), batch))
    assert rows["bfv_rns_tensorsum"] == count * chunks and rows["rns_extend"] == count * chunks and rows["bfv_rns_scale"] == chunks
    assert "ckks_rns_tensor" not in rows
    one = _timer_rows(B, lambda: B.bfv_rns_mul_dev(plans, ap, sp, t, d_rlk.data_ptr(), da.data_ptr(), da.data_ptr(), out.data_ptr(), batch))
    assert one["ckks_rns_tensor"] == (2 * k + 1) * chunks and one["bfv_rns_scale"] == chunks and "bfv_rns_tensorsum" not in one
    # the key switch is launched as often as in one `mul`, whatever the number of pairs
    relin = {label for label in set(rows) | set(one) if label.startswith("ckks_rns_") and label != "ckks_rns_tensor"}
    assert relin and all(rows.get(label) == one.get(label) for label in relin), (rows, one)


# ---- the Python surface, end to end (n = 64, t = 257, k = 2) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(pkg):
    bfv = pkg.bfv
    n, t, k = 64, 257, 2
    mods, aux, P = R.chain(n, k, bq=50, bb=61, bp=51)
    param = bfv.RnsParam(n, mods, aux, P, t)
    key = bfv.RnsClientKey.generate(SEED, param)
    return dict(bfv=bfv, param=param, key=key, pk=key.public_key(0), rlk=key.relin_key(0), enc=bfv.BatchEncoder(n, t))


def _encrypt_slots(world, slots):
    return world["key"].encrypt(world["pk"], world["enc"].encode(slots))


def _slots_of(world, ct):
    return world["enc"].decode(world["key"].decrypt(ct)).astype(np.int64)


def test_dot_and_square_end_to_end(pkg, world):
    bfv, p, key = world["bfv"], world["param"], world["key"]
    t, N, count = p.t, p.n // 2, 9
    rng = np.random.default_rng(11)
    xs, ys = rng.integers(0, t, (count, 2, 2, N)), rng.integers(0, t, (count, 2, 2, N))        # [pair][batch][2][n/2]
    cx, cy = [_encrypt_slots(world, x) for x in xs], [_encrypt_slots(world, y) for y in ys]
    w = [1, -1, 2, 128, -128, 129 + t, 5, -7, 100]
    got = bfv.dot(cx, cy, world["rlk"], w)
    want = sum(D.centred(wr, t) * xs[r] * ys[r] for r, wr in enumerate(w)) % t
    assert np.array_equal(_slots_of(world, got), want)
    assert key.noise_budget(got) > 0
    plain = bfv.dot(cx, cy, world["rlk"])
    assert np.array_equal(_slots_of(world, plain), (xs * ys).sum(axis=0) % t) and key.noise_budget(plain) > 0
    # one rounding and one relinearisation against nine of each.  Both sums carry the same tensor noise, which dominates; the
    # roundings and key switches are random terms far below it, so the realised budgets can differ by the last bit either way
    # and no further: the budget of `dot` is within one bit of the composed sum's, never lower by more
    composed = cx[0].mul(cy[0], world["rlk"])
    for r in range(1, count):
        composed = composed + cx[r].mul(cy[r], world["rlk"])
    assert np.array_equal(_slots_of(world, composed), (xs * ys).sum(axis=0) % t)
    print("noise budgets: dot", key.noise_budget(plain), "composed", key.noise_budget(composed))
    assert key.noise_budget(plain) >= key.noise_budget(composed) - 1 > 0
    sq = cx[0].square(world["rlk"])
    assert np.array_equal(_u64(sq.d), _u64(cx[0].mul(cx[0], world["rlk"]).d))
    assert np.array_equal(_slots_of(world, sq), xs[0] * xs[0] % t) and key.noise_budget(sq) > 0
    with pytest.raises(ValueError):
        bfv.dot(cx, cy[:-1], world["rlk"])
    with pytest.raises(ValueError):
        bfv.dot(cx[:2], cy[:2], world["rlk"], [1, t])


def test_lincomb_and_mul_const(pkg, world):
    bfv, p, key = world["bfv"], world["param"], world["key"]
    t, N = p.t, p.n // 2
    rng = np.random.default_rng(12)
    xs = rng.integers(0, t, (3, 2, 2, N))
    cts = [_encrypt_slots(world, x) for x in xs]
    weights, consts = [[1, -1, 2], [128, 129, 0], [3, 0, 0]], [0, 5, -77]
    outs = bfv.lincomb(cts, weights, consts)
    assert len(outs) == 3
    for o, ct in enumerate(outs):
        want = (sum(D.centred(wr, t) * xs[r] for r, wr in enumerate(weights[o])) + consts[o]) % t
        assert np.array_equal(_slots_of(world, ct), want), o
        assert key.noise_budget(ct) > 0
    one = bfv.lincomb(cts, [2, 3, -4])
    assert len(one) == 1 and np.array_equal(_slots_of(world, one[0]), (2 * xs[0] + 3 * xs[1] - 4 * xs[2]) % t)
    for c in (0, 1, -1, 77, 128, 129, 3 * t + 2):
        assert np.array_equal(_slots_of(world, cts[0].mul_const(c)), c * xs[0] % t), c
    with pytest.raises(ValueError):
        bfv.lincomb(cts, [1, 2])
    with pytest.raises(ValueError):
        bfv.lincomb(cts, [[1, 2, 3]], [1, 2])


def test_diag_sum(pkg, world):
    p, key = world["param"], world["key"]
    t, N = p.t, p.n // 2
    rng = np.random.default_rng(13)
    x = rng.integers(0, t, (2, 2, N))                                # [batch][2][n/2]
    ct = _encrypt_slots(world, x)
    steps = [0, 1, 5]
    rows = rng.integers(0, t, (2, len(steps), 2, N))                 # two outputs
    pts = key.encode_diagonals(rows, steps)
    assert tuple(pts.d_pts.shape) == (2, 3, len(p.moduli) + 1, p.n) and pts.gs == [1, 5, pow(5, 5, 2 * p.n)]
    gks = [None] + [key.rotation_key(st, 3 + i) for i, st in enumerate(steps[1:])]
    outs = ct.diag_sum(pts, gks)
    assert len(outs) == 2
    for o, got in enumerate(outs):
        want = sum(rows[o, r][None] * np.roll(x, -st, axis=2) for r, st in enumerate(steps)) % t
        assert np.array_equal(_slots_of(world, got), want), o
        assert key.noise_budget(got) > 0
    one = key.encode_diagonals(rows[0], steps)                       # [count][2][n/2]: one output
    assert np.array_equal(_u64(ct.diag_sum(one, gks)[0].d), _u64(outs[0].d))
    with pytest.raises(ValueError):
        ct.diag_sum(pts, gks[:2])
    with pytest.raises(ValueError):
        ct.diag_sum(pts, [None, None, gks[2]])
    with pytest.raises(ValueError):
        key.encode_diagonals(rows[:, :2], steps)


@pytest.fixture(scope="module")
def rotation_keys(world):
    """the keys of every step a transform of n1 in {4, 8} can ask for at N = 32: 1 .. 7, and the multiples of 4"""
    key = world["key"]
    return {st: key.rotation_key(st, 10 + st) for st in sorted(set(range(1, 8)) | set(range(4, 32, 4)))}


@pytest.mark.parametrize("kind", ["dense", "banded", "two_rows"])
@pytest.mark.parametrize("n1", [4, 8])
def test_linear_transform(pkg, world, rotation_keys, kind, n1):
    bfv, p, key = world["bfv"], world["param"], world["key"]
    t, N = p.t, p.n // 2
    rng = np.random.default_rng(14 + n1)
    M = {"dense": lambda: rng.integers(0, t, (N, N)), "banded": lambda: D.banded(rng, N, t, 5),
         "two_rows": lambda: np.stack([rng.integers(0, t, (N, N)), D.banded(rng, N, t, 3)])}[kind]()
    lt = bfv.LinearTransform.from_matrices(p, world["enc"], M, n1)
    assert lt.n1 == n1 and set(lt.required_steps()) <= set(rotation_keys)
    x = rng.integers(0, t, (2, 2, N))
    got = _encrypt_slots(world, x).linear_transform(lt, rotation_keys)
    M2 = np.stack([M, M]) if M.ndim == 2 else M
    assert np.array_equal(_slots_of(world, got), np.stack([D.matvec(M2, x[r], t) for r in range(2)]))
    assert key.noise_budget(got) > 0
    if kind == "banded":
        # the five diagonals 0 .. 4: d = 4 a + b is babies 0 .. 3 under giants 0 and 1, d = 8 a + b babies 0 .. 4 under giant 0
        assert (lt.baby, lt.giant) == (([0, 1, 2, 3], [0, 1]) if n1 == 4 else ([0, 1, 2, 3, 4], [0])) and lt.required_steps() == [1, 2, 3, 4]
        missing = dict(rotation_keys)
        del missing[1]
        with pytest.raises(KeyError):
            _encrypt_slots(world, x).linear_transform(lt, missing)
    with pytest.raises(ValueError):
        bfv.LinearTransform.from_matrices(p, world["enc"], np.zeros((N + 1, N + 1)), n1)
