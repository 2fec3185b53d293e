"""BFV key generation, encryption and decryption on the device (bfv_client.hip): every entry point word for
word against the restatement of tests/_bfv_client_numpy.py (tolerance zero), decryption against the composition of the existing
R_q entry points, the rejections with their outputs untouched, and the reference's property tests run end to end through
bfv.ClientKey on the seeds, rows and messages that tests/test_bfv_client_cpu.py proved."""
import numpy as np
import pytest

import _bfv_client_numpy as BC
import _client_numpy as C
from conftest import Q16, Q61
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64 = np.uint64
Q63 = 9223372036844421121                                                     # above 2^62, = 1 (mod 2^17): tests/test_glue_rows.py
SEED = bytes((5 * i + 9) % 256 for i in range(32))
INVALID = -9
FILL = 0x5A5A5A5A5A5A5A5A
RINGS = [(Q16, 2), (Q16, 4), (Q16, 8), (Q16, 16), (Q16, 512), (Q16, 4096), (Q61, 16), (Q61, 1024), (Q63, 16)]
ROWS = [(1 << 32) - 1, 1 << 32]


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _secret(pkg, n, row):
    s = _empty((n,))
    pkg.binding.bfv_secret_key_dev(n, SEED, row, s.data_ptr())
    return s


def _evals(pkg, q, n, x):
    """fhe_ntt_forward_dev of the rows of x (numpy [rows][n]) -> device tensor"""
    d, out = _dev(x), _empty(np.shape(x))
    pkg.Plan(q, n).forward_dev(d.data_ptr(), out.data_ptr(), int(np.size(x)) // n)
    return out


# ---- keys ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("q,n", RINGS)
def test_secret_and_public_key_word_exact(pkg, tab, q, n, row):
    s = _secret(pkg, n, row)
    want_s = BC.secret_key(SEED, row, n)
    assert np.array_equal(_u64(s), want_s)
    dt, pk = _dev(tab), _empty((2, n))
    pkg.binding.bfv_public_key_dev(pkg.Plan(q, n), SEED, row, s.data_ptr(), dt.data_ptr(), len(tab), pk.data_ptr())
    w0, w1 = BC.public_key(SEED, row, want_s, q, tab)
    assert np.array_equal(_u64(pk), np.stack([w0, w1]))
    # without errors (m = 0) pk0 + a s = 0: the table is what separates the two
    pkg.binding.bfv_public_key_dev(pkg.Plan(q, n), SEED, row, s.data_ptr(), None, 0, pk.data_ptr())
    z0, z1 = BC.public_key(SEED, row, want_s, q, tab[:0])
    assert np.array_equal(_u64(pk), np.stack([z0, z1])) and np.array_equal(z1, w1) and (n < 8 or not np.array_equal(z0, w0))


@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("n", [16, 8192])
def test_relin_key_word_exact(pkg, tab, n, row):
    """q = 65537, p = q^2: n pq = 2^52 and 2^61; at n = 8192 a coefficient of the integer product a s passes 2^53, where
    the reference's f64 route would round: the exact route is what is compared"""
    q, pq = Q16, Q16 ** 3
    s = _secret(pkg, n, 0)
    dt, out = _dev(tab), _empty((2, n))
    pkg.binding.bfv_relin_key_dev(q, n, pq, SEED, row, s.data_ptr(), dt.data_ptr(), len(tab), out.data_ptr())
    want_s = BC.secret_key(SEED, 0, n)
    k0, k1 = BC.relin_key(SEED, row, want_s, q, pq, tab)
    assert np.array_equal(_u64(out), np.stack([k0, k1]))
    if n == 8192:
        top = sum(int(k1[i]) * int(want_s[n - 1 - i]) for i in range(n))                     # coefficient n - 1 of a s: no wrapped term
        assert top > 1 << 53


# ---- encryption ---------------------------------------------------------------------------------------------------------------
def _encrypt(pkg, q, n, t, first_row, d_pk_evals, msg, stride, tab, batch):
    out = _empty((2, batch, n))
    dm, dt = (_dev(msg) if msg is not None else None), (_dev(tab) if len(tab) else None)
    pkg.binding.bfv_encrypt_dev(pkg.Plan(q, n), t, SEED, first_row, d_pk_evals.data_ptr(), _ptr(dm), stride, _ptr(dt), len(tab), out.data_ptr(), batch)
    return _u64(out)


def _pk(q, n, seed=3):
    rng = np.random.default_rng(seed + n)
    return rng.integers(0, q, (2, n), dtype=np.uint64)


@pytest.mark.parametrize("batch", [1, 3, 257])
@pytest.mark.parametrize("q,n", RINGS)
def test_encrypt_word_exact(pkg, tab, q, n, batch):
    """rows (2^32 - 2) .. cross into the high nonce word; a message per row at stride n; a random public key (the words do not
    ask the key to be one)"""
    t, first_row = 32, (1 << 32) - 2
    pk = _pk(q, n)
    msg = np.random.default_rng(batch).integers(0, t, (batch, n), dtype=np.uint64)
    got = _encrypt(pkg, q, n, t, first_row, _evals(pkg, q, n, pk), msg, n, tab, batch)
    c0, c1, _ = BC.encrypt(SEED, first_row, pk[0], pk[1], msg, batch, q, t, tab)
    assert np.array_equal(got[0], c0) and np.array_equal(got[1], c1)


@pytest.mark.parametrize("q,n", [(Q16, 2), (Q16, 16), (Q61, 1024), (Q63, 16)])
def test_encrypt_message_forms(pkg, tab, q, n):
    """msg_stride 0 (one message), n, an odd stride above n, d_msg NULL; message words at and above t and q (Delta (m mod q));
    no error table (m = 0)"""
    t, batch, first_row = 7, 3, 11
    pk = _pk(q, n)
    ev = _evals(pkg, q, n, pk)
    rng = np.random.default_rng(n)
    stride = n + 3
    flat = rng.integers(0, 1 << 64, 2 * stride + n, dtype=np.uint64, endpoint=False)
    flat[:4] = [q - 1, q, t, q + 1][:min(4, len(flat))]
    rows = np.stack([flat[r * stride:r * stride + n] for r in range(batch)])
    for msg, st, want_msg, tb in ((flat, stride, rows, tab), (flat, 0, flat[:n], tab), (flat[:batch * n], n, flat[:batch * n].reshape(batch, n), tab),
                                  (None, 0, None, tab), (flat, stride, rows, tab[:0])):
        got = _encrypt(pkg, q, n, t, first_row, ev, msg, st, tb, batch)
        c0, c1, _ = BC.encrypt(SEED, first_row, pk[0], pk[1], want_msg, batch, q, t, tb)
        assert np.array_equal(got[0], c0) and np.array_equal(got[1], c1), (st, len(tb))


@pytest.mark.parametrize("q,n", [(Q16, 2), (Q16, 8), (Q16, 512), (Q61, 1024), (Q63, 16)])
def test_degenerate_keys_expose_each_sampler(pkg, tab, q, n):
    """pk = (0, 0): c0 = e1 + Delta m, c1 = e2.  pk = (1, 0) as constants (evals: all ones, all zeros): c0 = u + e1 + Delta m."""
    t, batch, first_row = 32, 3, (1 << 32) - 1
    msg = np.random.default_rng(n).integers(0, t, (batch, n), dtype=np.uint64)
    e = BC.errors(SEED, 2 * first_row, n, 2 * batch, tab).reshape(batch, 2, n)
    e1, e2 = BC._residues(e[:, 0], q), BC._residues(e[:, 1], q)
    dm = BC._delta_m(msg, q, t)
    got = _encrypt(pkg, q, n, t, first_row, _dev(np.zeros((2, n), dtype=U64)), msg, n, tab, batch)
    assert np.array_equal(got[0], BC._add(e1, dm, q)) and np.array_equal(got[1], e2)
    one = np.stack([np.ones(n, dtype=U64), np.zeros(n, dtype=U64)])
    got = _encrypt(pkg, q, n, t, first_row, _dev(one), msg, n, tab, batch)
    u = BC._residues(BC.ephemeral(SEED, first_row, n, batch), q)
    assert np.array_equal(got[0], BC._add(BC._add(u, e1, q), dm, q)) and np.array_equal(got[1], e2)
    assert set(np.unique(u)) <= {0, 1, q - 1} and (n < 8 or len(np.unique(u)) == 3)


@pytest.mark.parametrize("q,n,batch", [(Q16, 512, 257), (Q16, 4096, 3), (Q61, 1024, 3), (Q16, 16, 3)])
def test_both_routes_of_encryption_give_the_same_words(pkg, tab, monkeypatch, q, n, batch):
    """FHE_BFV_ENCRYPT_STAGED, read per call, forces a route: 1 the staged one (the key rows broadcast over a chunk, two
    fhe_rq_mul_dev), 0 the pointwise one (a forward transform, bfv_pk_pointwise_kernel, two inverses).  The default is staged at
    the first three shapes and pointwise at n = 16.  Same words, and the restatement's."""
    t, first_row = 32, (1 << 32) - 2
    pk = _pk(q, n)
    ev = _evals(pkg, q, n, pk)
    msg = np.random.default_rng(batch).integers(0, t, (batch, n), dtype=np.uint64)
    monkeypatch.setenv("FHE_BFV_ENCRYPT_STAGED", "1")
    staged = _encrypt(pkg, q, n, t, first_row, ev, msg, n, tab, batch)
    monkeypatch.setenv("FHE_BFV_ENCRYPT_STAGED", "0")
    pointwise = _encrypt(pkg, q, n, t, first_row, ev, msg, n, tab, batch)
    assert np.array_equal(staged, pointwise)
    c0, c1, _ = BC.encrypt(SEED, first_row, pk[0], pk[1], msg, batch, q, t, tab)
    assert np.array_equal(pointwise[0], c0) and np.array_equal(pointwise[1], c1)


@pytest.mark.parametrize("n", [2, 4096])
def test_encrypt_does_not_depend_on_the_chunking(pkg, tab, n):
    """a chunk is 2^21 coefficients: 2^20 rows at n = 2 (the smallest ring; the pointwise route) and 512 rows at n = 4096 (the
    route of the moduli with a 32-bit form, whose key rows are staged a chunk's worth); a batch of two rows more crosses one
    boundary.  The rows either side of it, the first and the last equal single-row calls, and the rows after the boundary
    equal the restatement."""
    q, t, first_row = Q16, 32, 5
    batch = ((1 << 21) // n) + 2
    pk = _pk(q, n)
    ev = _evals(pkg, q, n, pk)
    got = _encrypt(pkg, q, n, t, first_row, ev, None, 0, tab, batch)
    for r in (0, batch - 3, batch - 2, batch - 1):
        one = _encrypt(pkg, q, n, t, first_row + r, ev, None, 0, tab, 1)
        assert np.array_equal(got[:, r], one[:, 0]), r
    c0, c1, _ = BC.encrypt(SEED, first_row + batch - 2, pk[0], pk[1], None, 2, q, t, tab)
    assert np.array_equal(got[0, batch - 2:], c0) and np.array_equal(got[1, batch - 2:], c1)


# ---- decryption ---------------------------------------------------------------------------------------------------------------
def _decrypt_composed(pkg, q, n, t, ct, s):
    """fhe_rq_mul_dev, fhe_rq_add_dev, fhe_rq_mul_div_round_dev, fhe_rq_remodule_dev"""
    L, plan = pkg.load_library(), pkg.Plan(q, n)
    batch = ct.shape[1]
    c0, c1, sb = _dev(ct[0]), _dev(ct[1]), _dev(np.broadcast_to(s, (batch, n)))
    p, cs, r, out = _empty((batch, n)), _empty((batch, n)), _empty((batch, n)), _empty((batch, n))
    plan.rq_mul_dev(c1.data_ptr(), sb.data_ptr(), p.data_ptr(), batch)
    assert L.fhe_rq_add_dev(plan.handle, c0.data_ptr(), p.data_ptr(), cs.data_ptr(), batch, None) == 0
    assert L.fhe_rq_mul_div_round_dev(q, t, q, cs.data_ptr(), r.data_ptr(), batch * n, None) == 0
    assert L.fhe_rq_remodule_dev(t, r.data_ptr(), out.data_ptr(), batch * n, None) == 0
    return _u64(out)


@pytest.mark.parametrize("q,n", [(Q16, 64), (Q16, 4096), (Q61, 256), (Q63, 16)])
def test_decrypt_is_the_composition_of_the_existing_entry_points(pkg, q, n):
    """random ciphertext words that decrypt to nothing, so every rounding case of the f64 scaling occurs; at q = 65537 also c1 =
    0 with c0 running through every residue"""
    rng = np.random.default_rng(n)
    s = rng.integers(0, 2, n, dtype=np.uint64)
    d_se = _evals(pkg, q, n, s)
    cts = [rng.integers(0, q, (2, 5, n), dtype=np.uint64)]
    if q == Q16 and n == 64:
        every = np.arange(65536, dtype=U64).reshape(-1, n)
        every[0, 0] = 65536
        cts.append(np.stack([every, np.zeros_like(every)]))
    for ct in cts:
        for t in (2, 32, q - 1):
            out = _empty(ct.shape[1:])
            d_ct = _dev(ct)
            pkg.binding.bfv_decrypt_dev(pkg.Plan(q, n), t, d_se.data_ptr(), d_ct.data_ptr(), out.data_ptr(), ct.shape[1])
            got = _u64(out)
            assert np.array_equal(got, _decrypt_composed(pkg, q, n, t, ct, s)), t
            assert int(got.max()) < t
    if n <= 64:
        t = 32
        out = _empty((5, n))
        d_ct = _dev(cts[0])
        pkg.binding.bfv_decrypt_dev(pkg.Plan(q, n), t, d_se.data_ptr(), d_ct.data_ptr(), out.data_ptr(), 5)
        assert np.array_equal(_u64(out), BC.decrypt(s, cts[0][0], cts[0][1], q, t))


# ---- the reference's property tests through bfv.ClientKey ----------------------------------------------------------------------
def _client(pkg, case):
    from fhe_study_amd import bfv

    param = bfv.Param(pkg.RingParam(case["q"], case["n"]), case["t"], case["p"])
    return bfv, param, bfv.ClientKey.generate(case["seed"], param)


@pytest.mark.parametrize("name", ["encrypt_512", "encrypt_4096_q61"])
def test_functional_encrypt_decrypt(pkg, tab, name):
    case = BC.CASES[name]
    bfv, param, ck = _client(pkg, case)
    pk = ck.public_key()
    m = BC.case_messages(case, 0)
    ct = ck.encrypt(pk, pkg.Rq(param.pt(), m))
    assert np.array_equal(ck.decrypt(ct).coeffs, m)
    s = BC.secret_key(case["seed"], 0, case["n"])
    assert np.array_equal(_u64(ck.d_s), s)
    w = BC.public_key(case["seed"], BC.PK_BASE, s, case["q"], tab)
    assert np.array_equal(pk.coeffs, np.stack(w))
    c0, c1, _ = BC.encrypt(case["seed"], 0, w[0], w[1], m, len(m), case["q"], case["t"], tab)
    assert np.array_equal(ct.c0.coeffs, c0) and np.array_equal(ct.c1.coeffs, c1)
    with pytest.raises(ValueError):
        ck.public_key()                                                        # slot 0 is used
    ct2 = ck.encrypt(pk, pkg.Rq(param.pt(), m[:1]))                            # the next call takes the next rows
    d0, _, _ = BC.encrypt(case["seed"], len(m), w[0], w[1], m[:1], 1, case["q"], case["t"], tab)
    assert np.array_equal(ct2.c0.coeffs, d0)


def test_functional_addition(pkg):
    case = BC.CASES["add_128"]
    bfv, param, ck = _client(pkg, case)
    pk = ck.public_key()
    m1, m2 = BC.case_messages(case, 0), BC.case_messages(case, 1)
    c = ck.encrypt(pk, pkg.Rq(param.pt(), m1)) + ck.encrypt(pk, pkg.Rq(param.pt(), m2))
    assert np.array_equal(ck.decrypt(c).coeffs, (m1 + m2) % U64(case["t"]))


@pytest.mark.parametrize("name", ["const_16_t8", "mul_16_t2"])
def test_functional_constants_and_product(pkg, tab, name):
    """add_const, mul_const (t = 8 and 2) and ct x ct (t = 2: the only t at which the reference claims it) with a
    relinearisation key made on the device; RLWE.mul, and the same product through fhe_bfv_mul_prepared_dev"""
    case = BC.CASES[name]
    q, n, t, pq = case["q"], case["n"], case["t"], case["p"] * case["q"]
    bfv, param, ck = _client(pkg, case)
    pk, rlk = ck.public_key(), ck.relin_key()
    s = BC.secret_key(case["seed"], 0, n)
    k0, k1 = BC.relin_key(case["seed"], BC.RLK_BASE, s, q, pq, tab)
    assert np.array_equal(rlk.rlk0, k0) and np.array_equal(rlk.rlk1, k1) and rlk.pq == pq
    m1, m2 = BC.case_messages(case, 0), BC.case_messages(case, 1)
    rows = len(m1)
    c1, c2 = ck.encrypt(pk, pkg.Rq(param.pt(), m1)), ck.encrypt(pk, pkg.Rq(param.pt(), m2))
    want_add = (m1 + m2) % U64(t)
    want_mul = np.stack([BC.negacyclic_schoolbook(m1[r], m2[r], t) for r in range(rows)])
    assert np.array_equal(ck.decrypt(bfv.add_const(c1, pkg.Rq(param.pt(), m2))).coeffs, want_add)
    assert np.array_equal(ck.decrypt(bfv.mul_const(rlk, c1, pkg.Rq(param.pt(), m2))).coeffs, want_mul)
    if t != 2:
        return
    prod = bfv.RLWE.mul(t, rlk, c1, c2)
    assert np.array_equal(ck.decrypt(prod).coeffs, want_mul)
    L = pkg.load_library()
    words = L.fhe_bfv_rlk_prepared_words(q, n, pq)
    d_rlk, prep = _dev(np.stack([rlk.rlk0, rlk.rlk1])), _empty((words,))
    assert L.fhe_bfv_rlk_prepare_dev(q, n, pq, d_rlk.data_ptr(), prep.data_ptr(), None) == 0
    ab, out = _dev(np.stack([c1.c0.coeffs, c1.c1.coeffs, c2.c0.coeffs, c2.c1.coeffs])), _empty((2, rows, n))
    assert L.fhe_bfv_mul_prepared_dev(q, n, t, pq, prep.data_ptr(), ab.data_ptr(), out.data_ptr(), rows, None) == 0
    o = _u64(out)
    assert np.array_equal(o[0], prod.c0.coeffs) and np.array_equal(o[1], prod.c1.coeffs)


# ---- rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(pkg, tab):
    """every FHE_E_INVALID row of the header block, with every output pre-filled and found untouched; the table rows need the
    device (the table is read back); batch = 0 is a no-op"""
    L = pkg.load_library()
    q, n, t, batch = Q16, 16, 32, 2
    plan = pkg.Plan(q, n)
    big = _empty((4 * batch * n,))
    dt, pk, s, msg = _dev(tab), _dev(_pk(q, n)), _dev(np.ones(n, dtype=U64)), _dev(np.zeros((batch, n), dtype=U64))
    bad_order, bad_top = tab.copy(), tab.copy()
    bad_order[3] = bad_order[2]
    bad_top[-1] = 1 << 63
    d_order, d_top = _dev(bad_order), _dev(bad_top)
    m = len(tab)

    def enc(**kw):
        a = dict(t=t, first_row=0, pk=pk.data_ptr(), msg=msg.data_ptr(), stride=n, cdt=dt.data_ptr(), m=m, out=big.data_ptr(), batch=batch, plan=plan)
        a.update(kw)
        return L.fhe_bfv_encrypt_dev(a["plan"].handle, a["t"], SEED, a["first_row"], a["pk"], a["msg"], a["stride"], a["cdt"], a["m"], a["out"], a["batch"], None)

    small = pkg.Plan(17, 8)
    cases = [enc(t=1), enc(t=q), enc(m=1025), enc(cdt=d_order.data_ptr()), enc(cdt=d_top.data_ptr()), enc(plan=small, t=2, m=17),
             enc(first_row=(1 << 63) - 1), enc(batch=1 << 56), enc(out=pk.data_ptr()), enc(out=msg.data_ptr()), enc(out=dt.data_ptr()), enc(stride=n - 1)]
    dec = lambda **kw: L.fhe_bfv_decrypt_dev(plan.handle, kw.get("t", t), s.data_ptr(), kw.get("ct", pk.data_ptr()), kw.get("out", big.data_ptr()),
                                             kw.get("batch", 1), None)
    cases += [dec(t=1), dec(t=q), dec(batch=1 << 56), dec(out=pk.data_ptr()), dec(out=s.data_ptr())]
    pkc = lambda **kw: L.fhe_bfv_public_key_dev(kw.get("plan", plan).handle, SEED, kw.get("row", 0), s.data_ptr(), kw.get("cdt", dt.data_ptr()), kw.get("m", m),
                                                kw.get("out", big.data_ptr()), None)
    cases += [pkc(m=1025), pkc(cdt=d_order.data_ptr()), pkc(cdt=d_top.data_ptr()), pkc(plan=small, m=17), pkc(row=1 << 63), pkc(out=s.data_ptr())]
    rlk = lambda **kw: L.fhe_bfv_relin_key_dev(kw.get("q", q), kw.get("n", n), kw.get("pq", q ** 3), SEED, kw.get("row", 0), s.data_ptr(),
                                               kw.get("cdt", dt.data_ptr()), kw.get("m", m), kw.get("out", big.data_ptr()), None)
    cases += [rlk(pq=q ** 3 + 1), rlk(n=32768), rlk(m=1025), rlk(cdt=d_order.data_ptr()), rlk(cdt=d_top.data_ptr()), rlk(q=3, pq=9, m=9), rlk(row=1 << 63),
              rlk(out=s.data_ptr())]
    assert cases == [INVALID] * len(cases)
    assert enc(batch=0) == 0 and dec(batch=0) == 0
    import torch

    torch.cuda.synchronize()
    assert (_u64(big) == U64(FILL)).all()
    assert (_u64(pk) == _pk(q, n)).all() and (_u64(s) == 1).all() and np.array_equal(_u64(dt), tab) and not _u64(msg).any()
    assert enc() == 0 and dec() == 0 and pkc() == 0 and rlk() == 0              # and the accepted forms of the same calls run
