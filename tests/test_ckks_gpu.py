"""CKKS on the device (ckks_client.hip): the encoder exactly against the case lists that
tests/test_ckks_cpu.py proved, the decoder within E_dec of the restatement, every scheme entry point word for word against
tests/_ckks_numpy.py (tolerance zero), the additions, the functional tests through ckks.ClientKey on the CPU module's seeds,
and every rejection with its outputs untouched."""
import numpy as np
import pytest

import _bfv_client_numpy as BC
import _ckks_numpy as K
import _client_numpy as C
from conftest import Q16, Q61
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
Q63 = 9223372036844421121
SEED = bytes((7 * i + 3) % 256 for i in range(32))
INVALID = -9
FILL = 0x5A5A5A5A5A5A5A5A
RINGS = [(Q16, 2), (Q16, 16), (Q16, 32), (Q16, 512), (Q16, 4096), (Q61, 16), (Q61, 1024), (Q63, 16)]
ROWS = [(1 << 32) - 1, 1 << 32]


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


def _i64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _cdev(z):
    import torch

    return torch.from_numpy(np.ascontiguousarray(z, dtype=np.complex128).view(np.float64)).cuda()


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


_TW = {}


def _tw(pkg, n):
    if n not in _TW:
        _TW[n] = _cdev(pkg.binding.ckks_twiddles(n))
    return _TW[n]


def _encode(pkg, n, delta, z, batch, stride=None):
    out = _empty((batch, n))
    d_z = _cdev(z)
    pkg.binding.ckks_encode_dev(n, delta, _tw(pkg, n).data_ptr(), d_z.data_ptr(), n // 2 if stride is None else stride, out.data_ptr(), batch)
    return out.cpu().numpy()


def _decode(pkg, n, delta, p, batch):
    import torch

    out = torch.full((batch, n // 2, 2), float("nan"), dtype=torch.float64, device="cuda")
    d_p = _i64(p)
    pkg.binding.ckks_decode_dev(n, delta, _tw(pkg, n).data_ptr(), d_p.data_ptr(), out.data_ptr(), batch)
    return out.cpu().numpy().view(np.complex128).reshape(batch, n // 2)


# ---- encode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 257])
@pytest.mark.parametrize("n,seed,b,ld", K.EXACT_CASES)
def test_encode_returns_the_constructed_polynomial(pkg, n, seed, b, ld, batch):
    delta = float(1 << ld)
    p = K.exact_case(n, seed, b)
    z = K.exact_case_slots(p, delta)
    idx = np.arange(batch) % len(p)
    got = _encode(pkg, n, delta, z[idx], batch)
    assert np.array_equal(got, p[idx])


@pytest.mark.parametrize("n,seed,rows,ld", K.RANDOM_CASES)
def test_encode_of_random_slots_is_the_restatement(pkg, n, seed, rows, ld):
    """and z_stride = 0 equals the replicated rows; an odd stride above n/2"""
    delta = float(1 << ld)
    z = K.random_case(n, seed, rows)
    want = K.encode(z, delta)
    assert np.array_equal(_encode(pkg, n, delta, z, rows), want)
    assert np.array_equal(_encode(pkg, n, delta, z[:1], 5, stride=0), np.repeat(want[:1], 5, axis=0))
    stride = n // 2 + 3
    flat = np.zeros(rows * stride, dtype=np.complex128)
    for r in range(rows):
        flat[r * stride:r * stride + n // 2] = z[r]
    assert np.array_equal(_encode(pkg, n, delta, flat, rows, stride=stride), want)


def test_encode_across_a_workgroup_packing_boundary(pkg):
    """N = 16: a thread per polynomial, 256 polynomials per workgroup; 300 rows cross into a second, partly filled one"""
    n, seed, b, ld = K.EXACT_CASES[3]
    assert n == 16
    p = K.exact_case(n, seed, b)
    z = K.exact_case_slots(p, float(1 << ld))
    idx = (np.arange(300) * 2) % 3
    assert np.array_equal(_encode(pkg, n, float(1 << ld), z[idx], 300), p[idx])


# ---- decode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3, 257])
@pytest.mark.parametrize("n", K.SIZES)
def test_decode_is_within_the_bound_of_the_restatement(pkg, n, batch):
    delta = 1024.0
    p = np.random.default_rng(n).integers(-(1 << 40), 1 << 40, (3, n), dtype=np.int64)
    want, bound = K.decode(p, delta), K.e_dec(p, delta)
    idx = np.arange(batch) % 3
    got = _decode(pkg, n, delta, p[idx], batch)
    err = np.abs(got - want[idx]).max(axis=1)
    print(f"\nN = {n}: worst decode error {err.max():.3e} against E_dec {bound.min():.3e}")
    assert (err <= bound[idx]).all()


def test_decode_edge_polynomials(pkg):
    """coefficients near +-2^52 at N = 4096, the zero polynomial, and the monomials X^0 and X^(N-1)"""
    n, delta = 4096, float(1 << 30)
    rng = np.random.default_rng(52)
    p = np.zeros((5, n), dtype=np.int64)
    p[0] = (1 << 52) - rng.integers(0, 1000, n)
    p[1] = -(1 << 52) + rng.integers(0, 1000, n)
    p[3, 0] = 7
    p[4, n - 1] = -5
    got = _decode(pkg, n, delta, p, 5)
    want, bound = K.decode(p, delta), K.e_dec(p, delta)
    assert (np.abs(got - want).max(axis=1) <= bound).all()
    assert not got[2].any() and np.array_equal(got[3], np.full(n // 2, 7 / delta, dtype=np.complex128))
    for nn in (2, 16):
        q = np.zeros((2, nn), dtype=np.int64)
        q[0, 0], q[1, nn - 1] = 3, 3
        g = _decode(pkg, nn, 2.0, q, 2)
        assert (np.abs(g - K.decode(q, 2.0)).max(axis=1) <= K.e_dec(q, 2.0)).all()


# ---- keys ---------------------------------------------------------------------------------------------------------------------
def _secret(pkg, q, n, row):
    s = _empty((n,))
    pkg.binding.ckks_secret_key_dev(pkg.Plan(q, n), SEED, row, s.data_ptr())
    return s


def _evals(pkg, q, n, x):
    d, out = _dev(x), _empty(np.shape(x))
    pkg.Plan(q, n).forward_dev(d.data_ptr(), out.data_ptr(), int(np.size(x)) // n)
    return out


@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("q,n", RINGS)
def test_secret_and_public_key_word_exact(pkg, tab, q, n, row):
    s = _secret(pkg, q, n, row)
    want_s = K.secret_key(SEED, row, n)
    assert np.array_equal(_u64(s), BC._residues(want_s, q))
    dt, pk = _dev(tab), _empty((2, n))
    pkg.binding.ckks_public_key_dev(pkg.Plan(q, n), SEED, row, s.data_ptr(), dt.data_ptr(), len(tab), pk.data_ptr())
    w0, w1 = K.public_key(SEED, row, want_s, q, tab)
    assert np.array_equal(_u64(pk), np.stack([w0, w1]))
    pkg.binding.ckks_public_key_dev(pkg.Plan(q, n), SEED, row, s.data_ptr(), None, 0, pk.data_ptr())     # m = 0: pk0 + a s = 0
    z0, z1 = K.public_key(SEED, row, want_s, q, tab[:0])
    assert np.array_equal(_u64(pk), np.stack([z0, z1])) and np.array_equal(z1, w1) and (n < 8 or not np.array_equal(z0, w0))


# ---- encryption ---------------------------------------------------------------------------------------------------------------
def _encrypt(pkg, q, n, first_row, d_pk_evals, msg, stride, tab, batch):
    out = _empty((2, batch, n))
    dm, dt = (_i64(msg) if msg is not None else None), (_dev(tab) if len(tab) else None)
    pkg.binding.ckks_encrypt_dev(pkg.Plan(q, n), SEED, first_row, d_pk_evals.data_ptr(), dm.data_ptr() if dm is not None else None, stride,
                                 dt.data_ptr() if dt is not None else None, len(tab), out.data_ptr(), batch)
    return _u64(out)


def _pk(q, n, seed=3):
    return np.random.default_rng(seed + n).integers(0, q, (2, n), dtype=np.uint64)


def _messages(q, n, batch, seed):
    """signed words: small, negative, and of magnitude above q"""
    m = np.random.default_rng(seed).integers(-(1 << 62), 1 << 62, (batch, n), dtype=np.int64)
    m[:, ::2] >>= 40
    m[0, :2] = [-1, np.iinfo(np.int64).min][:min(2, n)]
    return m


@pytest.mark.parametrize("batch", [1, 3, 257])
@pytest.mark.parametrize("q,n", RINGS)
def test_encrypt_word_exact(pkg, tab, q, n, batch):
    """rows (2^32 - 2) .. cross into the high nonce word; a signed message per row; a random public key"""
    first_row = (1 << 32) - 2
    pk = _pk(q, n)
    msg = _messages(q, n, batch, batch)
    got = _encrypt(pkg, q, n, first_row, _evals(pkg, q, n, pk), msg, n, tab, batch)
    c0, c1 = K.encrypt(SEED, first_row, pk[0], pk[1], msg, batch, q, tab)
    assert np.array_equal(got[0], c0) and np.array_equal(got[1], c1)


@pytest.mark.parametrize("q,n", [(Q16, 2), (Q16, 16), (Q61, 1024), (Q63, 16)])
def test_encrypt_message_forms(pkg, tab, q, n):
    """an odd stride, msg_stride 0 (one message), d_msg NULL, and no error table"""
    batch, first_row, stride = 3, 11, n + 3
    pk = _pk(q, n)
    ev = _evals(pkg, q, n, pk)
    flat = _messages(q, 2 * stride + n, 1, n)[0]
    rows = np.stack([flat[r * stride:r * stride + n] for r in range(batch)])
    for msg, st, want_msg, tb in ((flat, stride, rows, tab), (flat, 0, flat[:n], tab), (None, 0, None, tab), (flat, stride, rows, tab[:0])):
        got = _encrypt(pkg, q, n, first_row, ev, msg, st, tb, batch)
        c0, c1 = K.encrypt(SEED, first_row, pk[0], pk[1], want_msg, batch, q, tb)
        assert np.array_equal(got[0], c0) and np.array_equal(got[1], c1), (st, len(tb))


@pytest.mark.parametrize("q,n", [(Q16, 2), (Q16, 512), (Q61, 1024), (Q63, 16)])
def test_degenerate_keys_expose_each_sampler(pkg, tab, q, n):
    """pk = (0, 0): c0 = e0 + m, c1 = e1.  pk = (1, 0) as evals: c0 = v + e0 + m"""
    batch, first_row = 3, (1 << 32) - 1
    msg = _messages(q, n, batch, n)
    e = K.errors(SEED, 2 * first_row, n, 2 * batch, tab).reshape(batch, 2, n)
    e0, e1, mm = BC._residues(e[:, 0], q), BC._residues(e[:, 1], q), K.msg_mod(msg, q)
    got = _encrypt(pkg, q, n, first_row, _dev(np.zeros((2, n), dtype=U64)), msg, n, tab, batch)
    assert np.array_equal(got[0], BC._add(e0, mm, q)) and np.array_equal(got[1], e1)
    one = np.stack([np.ones(n, dtype=U64), np.zeros(n, dtype=U64)])
    got = _encrypt(pkg, q, n, first_row, _dev(one), msg, n, tab, batch)
    v = BC._residues(K.ternary(SEED, K.CKKS_EPH, first_row, n, batch), q)
    assert np.array_equal(got[0], BC._add(BC._add(v, e0, q), mm, q)) and np.array_equal(got[1], e1)
    assert set(np.unique(v)) <= {0, 1, q - 1} and (n < 8 or len(np.unique(v)) == 3)


@pytest.mark.parametrize("q,n,batch", [(Q16, 512, 257), (Q16, 4096, 3), (Q61, 1024, 3), (Q16, 16, 3)])
def test_both_routes_of_encryption_give_the_same_words(pkg, tab, monkeypatch, q, n, batch):
    first_row = (1 << 32) - 2
    pk = _pk(q, n)
    ev = _evals(pkg, q, n, pk)
    msg = _messages(q, n, batch, batch)
    monkeypatch.setenv("FHE_CKKS_ENCRYPT_STAGED", "1")
    staged = _encrypt(pkg, q, n, first_row, ev, msg, n, tab, batch)
    monkeypatch.setenv("FHE_CKKS_ENCRYPT_STAGED", "0")
    pointwise = _encrypt(pkg, q, n, first_row, ev, msg, n, tab, batch)
    assert np.array_equal(staged, pointwise)
    c0, c1 = K.encrypt(SEED, first_row, pk[0], pk[1], msg, batch, q, tab)
    assert np.array_equal(pointwise[0], c0) and np.array_equal(pointwise[1], c1)


@pytest.mark.parametrize("n", [2, 4096])
def test_encrypt_does_not_depend_on_the_chunking(pkg, tab, n):
    """a chunk is 2^21 coefficients: n = 2 takes the pointwise route, n = 4096 (q = 65537) the staged one; two rows more than
    a chunk cross one boundary"""
    q, first_row = Q16, 5
    batch = ((1 << 21) // n) + 2
    pk = _pk(q, n)
    ev = _evals(pkg, q, n, pk)
    got = _encrypt(pkg, q, n, first_row, ev, None, 0, tab, batch)
    for r in (0, batch - 3, batch - 2, batch - 1):
        one = _encrypt(pkg, q, n, first_row + r, ev, None, 0, tab, 1)
        assert np.array_equal(got[:, r], one[:, 0]), r
    c0, c1 = K.encrypt(SEED, first_row + batch - 2, pk[0], pk[1], None, 2, q, tab)
    assert np.array_equal(got[0, batch - 2:], c0) and np.array_equal(got[1, batch - 2:], c1)


# ---- decryption ---------------------------------------------------------------------------------------------------------------
def _decrypt(pkg, q, n, d_se, ct):
    out = _empty(ct.shape[1:])
    d_ct = _dev(ct)
    pkg.binding.ckks_decrypt_dev(pkg.Plan(q, n), d_se.data_ptr(), d_ct.data_ptr(), out.data_ptr(), ct.shape[1])
    return out.cpu().numpy()


@pytest.mark.parametrize("batch", [1, 3, 257])
@pytest.mark.parametrize("q,n", RINGS)
def test_decrypt_word_exact(pkg, q, n, batch):
    """random ciphertext words under a ternary key; with c1 = 0 the residues floor(q/2) and floor(q/2) + 1 straddle the centring"""
    rng = np.random.default_rng(n + batch)
    s = rng.integers(-1, 2, n)
    d_se = _evals(pkg, q, n, BC._residues(s, q))
    ct = rng.integers(0, q, (2, batch, n), dtype=np.uint64)
    assert np.array_equal(_decrypt(pkg, q, n, d_se, ct), K.decrypt(s, ct[0], ct[1], q))
    edge = np.zeros((2, 1, n), dtype=U64)
    edge[0, 0, :2] = [q // 2, q // 2 + 1]
    got = _decrypt(pkg, q, n, d_se, edge)
    assert got[0, 0] == q // 2 and got[0, 1] == q // 2 + 1 - q and not got[0, 2:].any()


# ---- additions and the functional tests through ckks.ClientKey -----------------------------------------------------------------
def _client(pkg, case):
    from fhe_study_amd import ckks

    param = ckks.Param(pkg.RingParam(case["q"], case["n"]))
    return ckks, ckks.ClientKey.generate(case["seed"], param, case["delta"])


def _rounded(z):
    return K.round_away(z.real) + 1j * K.round_away(z.imag)


@pytest.mark.parametrize("q,n", [(Q16, 16), (Q61, 1024)])
def test_add_and_sub_word_exact(pkg, q, n):
    from fhe_study_amd import ckks

    rng = np.random.default_rng(n)
    a, b = rng.integers(0, q, (2, 3, n), dtype=np.uint64), rng.integers(0, q, (2, 3, n), dtype=np.uint64)
    a[0, 0, :2], b[0, 0, :2] = [0, q - 1], [0, q - 1]
    ring = pkg.RingParam(q, n)
    ca, cb = ckks.Ciphertext(ring, a[0], a[1]), ckks.Ciphertext(ring, b[0], b[1])
    for got, want in ((ca + cb, K.add(a, b, q)), (ca - cb, K.sub(a, b, q))):
        assert np.array_equal(got.c0, want[0]) and np.array_equal(got.c1, want[1])


def test_functional_encrypt_decrypt_of_scaled_messages(pkg, tab):
    case = K.FUNCTIONAL["encrypt_32"]
    ckks, ck = _client(pkg, case)
    pk = ck.public_key()
    raw = K.case_raw_message(case)
    ct = ck.encrypt(pk, raw * 512)
    s = K.secret_key(case["seed"], 0, case["n"])
    w = K.public_key(case["seed"], K.PK_BASE, s, case["q"], tab)
    assert np.array_equal(pk.coeffs, np.stack(w))
    c0, c1 = K.encrypt(case["seed"], 0, w[0], w[1], raw * 512, len(raw), case["q"], tab)
    assert np.array_equal(ct.c0, c0) and np.array_equal(ct.c1, c1)
    assert np.array_equal(K.round_away(ck.decrypt(ct) / 512.0), raw)
    with pytest.raises(ValueError):
        ck.public_key()


@pytest.mark.parametrize("name", ["encode_16", "encode_4096_q61"])
def test_functional_encode_encrypt_decrypt_decode(pkg, tab, name):
    case = K.FUNCTIONAL[name]
    ckks, ck = _client(pkg, case)
    pk = ck.public_key()
    z = K.case_slots(case, 0)
    m = ck.encoder.encode(z)
    want_m = K.encode(z, case["delta"])
    assert np.abs(m - want_m).max() <= (0 if name == "encode_16" else 1)           # proved exact only where the CPU module proved the margin
    ct = ck.encode_and_encrypt(pk, z)
    c0, c1 = K.encrypt(case["seed"], 0, pk.coeffs[0], pk.coeffs[1], m, len(m), case["q"], tab)
    assert np.array_equal(ct.c0, c0) and np.array_equal(ct.c1, c1)
    assert np.array_equal(_rounded(ck.decrypt_and_decode(ct)), z)


@pytest.mark.parametrize("name", ["add_16", "sub_16", "add_4096_q61", "sub_4096_q61"])
def test_functional_add_and_sub(pkg, name):
    case = K.FUNCTIONAL[name]
    ckks, ck = _client(pkg, case)
    pk = ck.public_key()
    z0, z1 = K.case_slots(case, 0), K.case_slots(case, 1)
    ca, cb = ck.encode_and_encrypt(pk, z0), ck.encode_and_encrypt(pk, z1)
    got, want = (ck.decrypt_and_decode(ca + cb), z0 + z1) if name.startswith("add") else (ck.decrypt_and_decode(ca - cb), z0 - z1)
    assert np.array_equal(_rounded(got), want)


def test_functional_mul_plain(pkg):
    case = K.FUNCTIONAL["mul_plain_32_q61"]
    ckks, ck = _client(pkg, case)
    pk = ck.public_key()
    z0, z1 = K.case_slots(case, 0), K.case_slots(case, 1)
    m1 = ck.encoder.encode(z1)
    assert np.array_equal(m1, K.encode(z1, case["delta"]))
    ct = ck.encode_and_encrypt(pk, z0)
    prod = ckks.mul_plain(ct, m1)
    p0, p1 = K.mul_plain((ct.c0[0], ct.c1[0]), m1[0], case["q"])
    assert np.array_equal(prod.c0[0], p0) and np.array_equal(prod.c1[0], p1)
    assert np.array_equal(_rounded(ck.decrypt_and_decode(prod, scale=case["delta"] ** 2)), z0 * z1)


# ---- rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(pkg, tab):
    import torch

    L = pkg.load_library()
    q, n, batch = Q16, 16, 2
    plan = pkg.Plan(q, n)
    big = _empty((4 * batch * n,))
    dt, pk, s, msg = _dev(tab), _dev(_pk(q, n)), _dev(np.ones(n, dtype=U64)), _dev(np.zeros((batch, n), dtype=U64))
    bad_order, bad_top = tab.copy(), tab.copy()
    bad_order[3] = bad_order[2]
    bad_top[-1] = 1 << 63
    d_order, d_top = _dev(bad_order), _dev(bad_top)
    m = len(tab)
    tw, z = _tw(pkg, n), _cdev(np.ones((batch, n // 2), dtype=np.complex128))

    def enc(**kw):
        a = dict(first_row=0, pk=pk.data_ptr(), msg=msg.data_ptr(), stride=n, cdt=dt.data_ptr(), m=m, out=big.data_ptr(), batch=batch, plan=plan)
        a.update(kw)
        return L.fhe_ckks_encrypt_dev(a["plan"].handle, SEED, a["first_row"], a["pk"], a["msg"], a["stride"], a["cdt"], a["m"], a["out"], a["batch"], None)

    small = pkg.Plan(17, 8)
    cases = [enc(m=1025), enc(cdt=d_order.data_ptr()), enc(cdt=d_top.data_ptr()), enc(plan=small, m=17), enc(first_row=(1 << 63) - 1), enc(batch=1 << 56),
             enc(out=pk.data_ptr()), enc(out=msg.data_ptr()), enc(out=dt.data_ptr()), enc(stride=n - 1)]
    dec = lambda **kw: L.fhe_ckks_decrypt_dev(plan.handle, s.data_ptr(), kw.get("ct", pk.data_ptr()), kw.get("out", big.data_ptr()), kw.get("batch", 1), None)
    cases += [dec(batch=1 << 56), dec(out=pk.data_ptr()), dec(out=s.data_ptr())]
    pkc = lambda **kw: L.fhe_ckks_public_key_dev(kw.get("plan", plan).handle, SEED, kw.get("row", 0), s.data_ptr(), kw.get("cdt", dt.data_ptr()), kw.get("m", m),
                                                 kw.get("out", big.data_ptr()), None)
    cases += [pkc(m=1025), pkc(cdt=d_order.data_ptr()), pkc(cdt=d_top.data_ptr()), pkc(plan=small, m=17), pkc(row=1 << 63), pkc(out=s.data_ptr())]
    cod = lambda **kw: L.fhe_ckks_encode_dev(kw.get("n", n), kw.get("delta", 64.0), tw.data_ptr(), z.data_ptr(), kw.get("stride", n // 2),
                                             kw.get("out", big.data_ptr()), kw.get("batch", batch), None)
    dcd = lambda **kw: L.fhe_ckks_decode_dev(kw.get("n", n), kw.get("delta", 64.0), tw.data_ptr(), msg.data_ptr(), kw.get("out", big.data_ptr()),
                                             kw.get("batch", batch), None)
    for f in (cod, dcd):
        cases += [f(n=24), f(n=1), f(n=1 << 14), f(delta=0.0), f(delta=-2.0), f(delta=float("inf")), f(delta=float("nan")), f(out=tw.data_ptr()), f(batch=1 << 58)]
    cases += [cod(stride=n // 2 - 1), cod(out=z.data_ptr()), dcd(out=msg.data_ptr())]
    assert cases == [INVALID] * len(cases)
    assert enc(batch=0) == 0 and dec(batch=0) == 0 and cod(batch=0) == 0 and dcd(batch=0) == 0
    torch.cuda.synchronize()
    assert (_u64(big) == U64(FILL)).all()
    assert (_u64(pk) == _pk(q, n)).all() and (_u64(s) == 1).all() and np.array_equal(_u64(dt), tab) and not _u64(msg).any()
    assert np.array_equal(tw.cpu().numpy().view(np.complex128), pkg.binding.ckks_twiddles(n))
    assert enc() == 0 and dec() == 0 and pkc() == 0 and cod() == 0 and dcd() == 0     # and the accepted forms of the same calls run
