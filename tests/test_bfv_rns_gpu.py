"""BFV on an RNS modulus chain on the device (bfv_rns.hip): fhe_rns_extend_dev, fhe_bfv_rns_tensor_dev and
fhe_bfv_rns_mul_dev word for word against tests/_bfv_rns_numpy.py (tolerance zero: everything is integer), every rejection with
its output untouched, and the Python surface (bfv.RnsClientKey, bfv.RnsCiphertext, bfv.BatchEncoder) end to end."""
import random

import numpy as np
import pytest

import _bfv_rns_numpy as R
import _ckks_eval_numpy as E
import _ckks_numpy as K
import _client_numpy as C
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A
SEED = bytes((7 * i + 3) % 256 for i in range(32))
T = 65537


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _plans(pkg, mods, n):
    return [pkg.Plan(q, n) for q in mods]


# ---- the exact basis extension ------------------------------------------------------------------------------------------------------
def _ext_inputs(src, count, seed):
    """count integers in [0, M) with the edges first, as residues [len(src)][count]"""
    M = R.prod(src)
    rng = random.Random(seed)
    xs = ([0, M - 1, M // 2, M // 2 + 1] + [rng.randrange(M) for _ in range(count)])[-count:] if count < 4 else \
        [0, M - 1, M // 2, M // 2 + 1] + [rng.randrange(M) for _ in range(count - 4)]
    return xs, np.array([[x % m for x in xs] for m in src], dtype=U64)


@pytest.mark.parametrize("s,t", [(1, 2), (2, 3), (3, 2), (4, 5), (5, 4), (9, 9)])
@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("count", [1, 255, 257, 70001])
def test_extend_word_for_word(pkg, s, t, centred, count):
    ps = E.primes_below(62, 8, s + t) if (s + t) % 2 else E.primes_below(37, 8, s) + E.primes_below(61, 8, t)
    src, dst = ps[:s], ps[s:]
    M = R.prod(src)
    if count == 1:
        cases = [_ext_inputs(src, 4, 11)[0][i:i + 1] for i in range(4)]
    else:
        cases = [_ext_inputs(src, count, 100 * s + t + count)[0]]
    for xs in cases:
        res = np.array([[x % m for x in xs] for m in src], dtype=U64)
        out, din = _empty((t, len(xs))), _dev(res)
        pkg.binding.rns_extend_dev(src, dst, centred, din.data_ptr(), out.data_ptr(), len(xs))
        want = np.array([[(R.centre(x, M) if centred else x) % p for x in xs] for p in dst], dtype=U64)
        assert np.array_equal(_u64(out), want)
    # the restatement itself on a few of them, the CRT written out
    assert np.array_equal(R.extend(src, dst, res[:, :8], centred), want[:, :8])


def test_extend_rejections(pkg):
    B = pkg.binding
    ps = E.primes_below(61, 8, 20)
    src, dst = ps[:3], ps[3:5]
    din, out = _dev(np.zeros((3, 16), dtype=U64)), _empty((2, 16))

    def refused(code, *args, **kw):
        with pytest.raises(B.FheError) as e:
            B.rns_extend_dev(*args, **kw)
        assert e.value.code == code
        assert np.all(_u64(out) == U64(FILL))

    i, o = din.data_ptr(), out.data_ptr()
    refused(B.FHE_E_INVALID, [ps[0], ps[0], ps[1]], dst, False, i, o, 16)           # repeated
    refused(B.FHE_E_INVALID, src, [ps[4], ps[4]], False, i, o, 16)
    refused(B.FHE_E_INVALID, [ps[0], ps[1] + 1, ps[2]], dst, False, i, o, 16)       # even
    refused(B.FHE_E_INVALID, src, [ps[3], 4], False, i, o, 16)
    refused(B.FHE_E_INVALID, [ps[0], (1 << 62) + 1, ps[2]], dst, False, i, o, 16)   # 2^62 and above
    refused(B.FHE_E_INVALID, src, [ps[3], (1 << 62) + 1], False, i, o, 16)
    refused(B.FHE_E_INVALID, ps[:10], dst, False, i, o, 1)                          # more than 9
    refused(B.FHE_E_INVALID, src, ps[5:15], False, i, o, 1)
    refused(B.FHE_E_INVALID, [], dst, False, i, o, 16, src=0)
    refused(B.FHE_E_INVALID, [15, 21, ps[0]], dst, False, i, o, 16)                 # not coprime
    refused(B.FHE_E_NULL, None, dst, False, i, o, 16, src=3)
    refused(B.FHE_E_NULL, src, None, False, i, o, 16, dst=2)
    refused(B.FHE_E_NULL, src, dst, False, None, o, 16)
    refused(B.FHE_E_NULL, src, dst, False, i, None, 16)
    refused(B.FHE_E_INVALID, src, dst, False, i, i + 8 * 16, 16)                    # the output inside the input
    big = _empty((5, 16))
    with pytest.raises(B.FheError) as e:
        B.rns_extend_dev(src, dst, True, big.data_ptr(), big.data_ptr() + 8 * 40, 16)
    assert e.value.code == B.FHE_E_INVALID and np.all(_u64(big) == U64(FILL))
    B.rns_extend_dev(src, dst, True, i, o, 0)                                       # count = 0: a no-op
    assert np.all(_u64(out) == U64(FILL))


# ---- the scaled tensor and the product, word for word ---------------------------------------------------------------------------------
def _operands(mods, n, batch, seed):
    """a, b [k][2][batch][n] evals: row 0 uniform modulo Q; rows 1 and 2 the all-(floor(Q/2)) and all-(floor(Q/2) + 1)
    polynomials, which reach the bound |d| = n Q^2 / 2"""
    Q = R.prod(mods)
    rng = random.Random(seed)
    half, halfp = [Q // 2] * n, [Q // 2 + 1] * n

    def rows(second):
        out = [[rng.randrange(Q) for _ in range(n)] for _ in range(batch)]
        if batch >= 3:
            out[1], out[2] = half, (half if second else halfp)
        return out

    def ct(second):
        return np.stack([R.to_evals(mods, n, rows(second)) for _ in range(2)], axis=1)

    return ct(False), ct(True)


def _device_key(pkg, tab, mods, P, n, row):
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    d_s = _empty((len(mods) + 1, n))
    for i, p in enumerate(plans + [sp]):
        pkg.binding.ckks_secret_key_dev(p, SEED, 0, d_s[i].data_ptr())
    d_rlk, d_tab = _empty((len(mods), len(mods) + 1, 2, n)), _dev(tab)
    pkg.binding.ckks_rns_relin_key_dev(plans, sp, SEED, row, d_s.data_ptr(), d_tab.data_ptr(), len(tab), d_rlk.data_ptr())
    return d_rlk


def _run_tensor(pkg, mods, aux, n, t, a, b, stream=None):
    k, _, batch, _ = a.shape
    out, da, db = _empty((k, 3, batch, n)), _dev(a), _dev(b)
    pkg.binding.bfv_rns_tensor_dev(_plans(pkg, mods, n), _plans(pkg, aux, n), t, da.data_ptr(), db.data_ptr(), out.data_ptr(), batch, stream)
    return out


@pytest.mark.parametrize("n", [2, 8, 64, 2048])
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("batch", [1, 3])
def test_tensor_and_mul_word_for_word(pkg, tab, n, k, batch):
    mods, aux, P = R.chain(n, k)
    assert R.admitted(mods, aux, T, n)
    a, b = _operands(mods, n, batch, 1000 * n + 10 * k + batch)
    want = R.tensor(mods, T, a, b)
    assert np.array_equal(_u64(_run_tensor(pkg, mods, aux, n, T, a, b)), want)
    row = E.RLK_BASE + 64 * 5
    d_rlk = _device_key(pkg, tab, mods, P, n, row)
    out, da, db = _empty(a.shape), _dev(a), _dev(b)
    pkg.binding.bfv_rns_mul_dev(_plans(pkg, mods, n), _plans(pkg, aux, n), pkg.Plan(P, n), T, d_rlk.data_ptr(), da.data_ptr(), db.data_ptr(), out.data_ptr(), batch)
    assert np.array_equal(_u64(out), E.relinearize(mods, P, _u64(d_rlk), want))


def test_batch_across_a_chunk(pkg, tab):
    """n = 8192, k = 4: a chunk is 2^21 / (63 n) = 4 ciphertexts, so a batch of 5 takes two; small primes keep the integers short"""
    n, k, batch, t = 8192, 4, 5, 257
    mods, aux, P = R.chain(n, k, bq=21, bb=30, bp=31)
    assert R.admitted(mods, aux, t, n) and R.chunk_rows(n, k, batch) == 4
    rng = np.random.default_rng(3)
    a, b = (np.stack([rng.integers(0, q, (2, batch, n)).astype(U64) for q in mods]) for _ in range(2))
    want = R.tensor(mods, t, a, b)
    assert np.array_equal(_u64(_run_tensor(pkg, mods, aux, n, t, a, b)), want)
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 6)
    out, da, db = _empty(a.shape), _dev(a), _dev(b)
    pkg.binding.bfv_rns_mul_dev(_plans(pkg, mods, n), _plans(pkg, aux, n), pkg.Plan(P, n), t, d_rlk.data_ptr(), da.data_ptr(), db.data_ptr(), out.data_ptr(), batch)
    assert np.array_equal(_u64(out), E.relinearize(mods, P, _u64(d_rlk), want))


def test_non_default_stream_and_aliasing(pkg, tab):
    import torch

    n, k, batch = 64, 2, 3
    mods, aux, P = R.chain(n, k)
    a, b = _operands(mods, n, batch, 77)
    want = R.tensor(mods, T, a, b)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out = _run_tensor(pkg, mods, aux, n, T, a, b, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(_u64(out), want)
    B = pkg.binding
    plans, ap, sp = _plans(pkg, mods, n), _plans(pkg, aux, n), pkg.Plan(P, n)
    d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 7)
    da, db = _dev(a), _dev(b)
    before = _u64(da).copy()
    for call in (lambda: B.bfv_rns_tensor_dev(plans, ap, T, da.data_ptr(), db.data_ptr(), da.data_ptr(), batch),
                 lambda: B.bfv_rns_mul_dev(plans, ap, sp, T, d_rlk.data_ptr(), da.data_ptr(), db.data_ptr(), da.data_ptr(), batch),
                 lambda: B.bfv_rns_mul_dev(plans, ap, sp, T, d_rlk.data_ptr(), da.data_ptr(), db.data_ptr(), db.data_ptr() + 8 * n, batch),
                 lambda: B.bfv_rns_mul_dev(plans, ap, sp, T, d_rlk.data_ptr(), da.data_ptr(), db.data_ptr(), d_rlk.data_ptr(), batch)):
        with pytest.raises(B.FheError) as e:
            call()
        assert e.value.code == B.FHE_E_INVALID
    assert np.array_equal(_u64(da), before)
    # the admission at one either side of the bound: batch = 0 returns after the checks
    m40, a41, _ = R.chain(n, k, bq=40, bb=41)
    t_edge = (R.prod(a41) - 2) // (n * R.prod(m40))
    B.bfv_rns_tensor_dev(_plans(pkg, m40, n), _plans(pkg, a41, n), t_edge, None, None, None, 0)
    with pytest.raises(B.FheError) as e:
        B.bfv_rns_tensor_dev(_plans(pkg, m40, n), _plans(pkg, a41, n), t_edge + 1, None, None, None, 0)
    assert e.value.code == B.FHE_E_INVALID
    # parameters the calls refuse: a base below the admission, a repeated prime, t < 2
    out = _empty((k, 3, batch, n))
    small_aux = E.primes_below(40, n, k + 1)
    for args in ((plans, _plans(pkg, small_aux, n), T), (plans, [ap[0], ap[0], ap[1]], T), (plans, [plans[0]] + ap[1:], T), (plans, ap, 1)):
        with pytest.raises(B.FheError) as e:
            B.bfv_rns_tensor_dev(args[0], args[1], args[2], da.data_ptr(), db.data_ptr(), out.data_ptr(), batch)
        assert e.value.code == B.FHE_E_INVALID and np.all(_u64(out) == U64(FILL))
    with pytest.raises(B.FheError) as e:
        B.bfv_rns_tensor_dev(plans, None, T, da.data_ptr(), db.data_ptr(), out.data_ptr(), batch)
    assert e.value.code == B.FHE_E_NULL
    B.bfv_rns_tensor_dev(plans, ap, T, da.data_ptr(), db.data_ptr(), out.data_ptr(), 0)
    assert np.all(_u64(out) == U64(FILL))


def test_workspace_bytes(pkg):
    B = pkg.binding
    for n, k, batch in ((64, 2, 3), (8192, 4, 5), (2, 1, 1), (1 << 19, 4, 1)):
        cb = R.chunk_rows(n, k, batch)
        assert B.bfv_rns_workspace_bytes(n, k, batch) == 8 * 7 * (2 * k + 1) * n * cb + B.ckks_rns_galois_workspace_bytes(n, k, cb, 1) > 0
    for n, k, batch in ((0, 1, 1), (1, 1, 1), (48, 2, 1), (1 << 20, 1, 1), (64, 0, 1), (64, 5, 1), (64, 2, 0)):
        assert B.bfv_rns_workspace_bytes(n, k, batch) == 0


# ---- the Python surface, end to end (n = 64, t = 257, k = 2) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(pkg):
    bfv = pkg.bfv

    n, t, k = 64, 257, 2
    mods, aux, P = R.chain(n, k, bq=50, bb=61, bp=51)
    param = bfv.RnsParam(n, mods, aux, P, t)
    key = bfv.RnsClientKey.generate(SEED, param)
    return dict(bfv=bfv, param=param, key=key, pk=key.public_key(0), rlk=key.relin_key(0), enc=bfv.BatchEncoder(n, t), s=K.secret_key(SEED, 0, n))


def _negacyclic_mod(a, b, t):
    return np.array([x % t for x in R.negacyclic([int(v) for v in a], [int(v) for v in b])], dtype=U64)


def test_scale_msg_encrypt_decrypt(pkg, world):
    p, key = world["param"], world["key"]
    rng = np.random.default_rng(1)
    m = rng.integers(0, p.t, (3, p.n))
    m[1], m[2] = 0, p.t - 1
    import torch

    dm = _empty((len(p.moduli), 3, p.n))
    pkg.binding.bfv_rns_scale_msg_dev(p.plans(), p.t, torch.from_numpy(m).cuda().data_ptr(), dm.data_ptr(), 3)
    assert np.array_equal(dm.cpu().numpy(), R.scale_msg(p.moduli, p.t, m))
    ct = key.encrypt(world["pk"], m)
    assert np.array_equal(key.decrypt(ct), m.astype(U64))
    host = _u64(ct.d)
    assert np.array_equal(key.decrypt(ct), R.decrypt(p.moduli, p.n, p.t, world["s"], host))
    v = R.phase(p.moduli, p.n, world["s"], host)
    assert [[int(x) for x in row] for row in key.phase(ct)] == v
    assert key.noise_budget(ct) == R.noise_budget(p.moduli, p.t, v) > 0
    # phases at +-floor(Q / 2) and around: the trivial ciphertexts (v, 0)
    Q = p.Q
    edge = [[Q // 2] * p.n, [-(Q // 2)] * p.n, [(Q // 2 - i) * (-1) ** i for i in range(p.n)]]
    triv = np.stack([R.to_evals(p.moduli, p.n, edge), np.zeros((len(p.moduli), 3, p.n), dtype=U64)], axis=1)
    got = key.decrypt(world["bfv"].RnsCiphertext(p, _dev(triv)))
    assert np.array_equal(got, R.decrypt_phase(p.moduli, p.t, edge))


def test_mul_and_three_squarings(pkg, world):
    p, key = world["param"], world["key"]
    rng = np.random.default_rng(2)
    ma, mb = rng.integers(0, p.t, (2, p.n)), rng.integers(0, p.t, (2, p.n))
    ca, cb = key.encrypt(world["pk"], ma), key.encrypt(world["pk"], mb)
    prod = ca.mul(cb, world["rlk"])
    assert np.array_equal(key.decrypt(prod), np.stack([_negacyclic_mod(ma[r], mb[r], p.t) for r in range(2)]))
    ct, m, budgets = ca, ma.astype(U64), [key.noise_budget(ca)]
    for _ in range(3):
        ct = ct.mul(ct, world["rlk"])
        m = np.stack([_negacyclic_mod(m[r], m[r], p.t) for r in range(2)])
        assert np.array_equal(key.decrypt(ct), m)
        budgets.append(key.noise_budget(ct))
    assert all(b > 0 for b in budgets) and all(x > y for x, y in zip(budgets, budgets[1:])), budgets


def test_add_sub_neg_plain(pkg, world):
    p, key = world["param"], world["key"]
    rng = np.random.default_rng(3)
    ma, mb, mp = (rng.integers(0, p.t, (2, p.n)) for _ in range(3))
    ca, cb = key.encrypt(world["pk"], ma), key.encrypt(world["pk"], mb)
    t = p.t
    assert np.array_equal(key.decrypt(ca + cb), ((ma + mb) % t).astype(U64))
    assert np.array_equal(key.decrypt(ca - cb), ((ma - mb) % t).astype(U64))
    assert np.array_equal(key.decrypt(-ca), ((-ma) % t).astype(U64))
    assert np.array_equal(key.decrypt(ca.add_plain(mp)), ((ma + mp) % t).astype(U64))
    assert np.array_equal(key.decrypt(ca.mul_plain(mp)), np.stack([_negacyclic_mod(ma[r], mp[r], t) for r in range(2)]))


def test_rotations_on_batched_rows(pkg, world):
    p, key, enc = world["param"], world["key"], world["enc"]
    n = p.n
    rng = np.random.default_rng(4)
    slots = rng.integers(0, p.t, (2, 2, n // 2))
    m = enc.encode(slots)
    assert np.array_equal(m, np.stack([R.encode(n, p.t, slots[r]) for r in range(2)]))
    assert np.array_equal(enc.decode(m), slots.astype(U64))
    ct = key.encrypt(world["pk"], m)
    keys = {1: key.rotation_key(1, 0), n // 2 - 1: key.rotation_key(n // 2 - 1, 1)}
    swap = key.row_swap_key(2)
    for step, gk in keys.items():
        assert np.array_equal(enc.decode(key.decrypt(ct.rotate(gk))), np.roll(slots, -step, axis=2).astype(U64))
    assert np.array_equal(enc.decode(key.decrypt(ct.swap_rows(swap))), slots[:, ::-1].astype(U64))
    many = ct.rotate_many([keys[1], keys[n // 2 - 1], swap])
    for got, sep in zip(many, (ct.rotate(keys[1]), ct.rotate(keys[n // 2 - 1]), ct.swap_rows(swap))):
        assert np.array_equal(_u64(got.d), _u64(sep.d))
    with pytest.raises(ValueError):
        ct.rotate(swap)
    with pytest.raises(ValueError):
        ct.swap_rows(keys[1])
    assert key.noise_budget(many[0]) > 0
