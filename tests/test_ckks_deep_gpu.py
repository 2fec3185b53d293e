"""CKKS on a deep RNS chain on the device (ckks_deep.hip): the key builders, the relinearisation, ct x ct, the
Galois key switch and the rescale, word for word against tests/_ckks_deep_numpy.py (tolerance zero), which
tests/test_ckks_deep_cpu.py proved; at alpha = 1 byte for byte against the fhe_ckks_rns_* entry points; the centring's edges; the
chunk; a second stream; misaligned buffers; every rejection with its output untouched; the workspace; the launch counts; and a
product chain of 11 ciphertexts through ckks.DeepClientKey."""
import numpy as np
import pytest

import _ckks_deep_numpy as D
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_numpy as K
import _client_numpy as C
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
FILL = 0x5A5A5A5A5A5A5A5A
SEED = bytes((11 * i + 7) % 256 for i in range(32))
SHAPES = [(8, 1, 8), (5, 2, 5), (5, 2, 4), (9, 3, 7), (12, 4, 12), (17, 8, 17), (3, 8, 3)]   # (L, alpha, l)


def _refused():
    return pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ")


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _plans(pkg, mods, n):
    return [pkg.Plan(q, n) for q in mods]


def _secret(pkg, plans, n):
    d_s = _empty((len(plans), n))
    for i, p in enumerate(plans):
        pkg.binding.ckks_secret_key_dev(p, SEED, 0, d_s[i].data_ptr())
    return d_s


def _key(pkg, tab, plans, sps, d_s, n, row, g=None):
    d_key, d_tab = _empty((D.dnum(len(plans), len(sps)), len(plans) + len(sps), 2, n)), _dev(tab)
    if g is None:
        pkg.binding.ckks_deep_relin_key_dev(plans, sps, SEED, row, d_s.data_ptr(), d_tab.data_ptr(), len(tab), d_key.data_ptr())
    else:
        pkg.binding.ckks_deep_galois_key_dev(plans, sps, SEED, row, g, d_s.data_ptr(), d_tab.data_ptr(), len(tab), d_key.data_ptr())
    return d_key


def _galois(pkg, plans, sps, d_gks, gs, kl, d_ct, stream=None):
    k, _, batch, n = d_ct.shape
    out = _empty((len(gs), k, 2, batch, n))
    pkg.binding.ckks_deep_galois_dev(plans, sps, [x.data_ptr() for x in d_gks], gs, kl, d_ct.data_ptr(), out.data_ptr(), batch, stream)
    return _u64(out)


def _mul(pkg, plans, sps, d_key, kl, a, b, stream=None):
    out = _empty(tuple(a.shape))
    pkg.binding.ckks_deep_mul_dev(plans, sps, d_key.data_ptr(), kl, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[2], stream)
    return _u64(out)


# ---- the restated keys, once per (n, L, alpha) ------------------------------------------------------------------------------------------
_KEYS = {}


def _elements(n):
    return [5 % (2 * n), 2 * n - 1, 25 % (2 * n)]                    # a rotation, the conjugation, another rotation


def _ref_keys(n, L, alpha, tab):
    if (n, L, alpha) not in _KEYS:
        mods, sps = D.case_chain(n, L, alpha)
        s = K.secret_key(SEED, 0, n)
        rlk = D.switch_key(SEED, E.RLK_BASE, s, mods, sps, tab)
        gks = [D.switch_key(SEED, G.GK_BASE + 64 * t, s, mods, sps, tab, g) for t, g in enumerate(_elements(n))]
        _KEYS[(n, L, alpha)] = (mods, sps, rlk, gks)
    return _KEYS[(n, L, alpha)]


def _run_case(pkg, tab, n, batch, L, alpha, l):
    B = pkg.binding
    mods, sps, rlk, gks = _ref_keys(n, L, alpha, tab)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    d_s = _secret(pkg, plans + sp, n)
    gs = _elements(n)
    d_rlk = _key(pkg, tab, plans, sp, d_s, n, E.RLK_BASE)
    assert np.array_equal(_u64(d_rlk), rlk)
    d_gks = [_key(pkg, tab, plans, sp, d_s, n, G.GK_BASE + 64 * t, g) for t, g in enumerate(gs)]
    for t in range(3):
        assert np.array_equal(_u64(d_gks[t]), gks[t]), gs[t]
    lm, lp = mods[:l], plans[:l]
    a, b = E.case_ct(lm, n, batch, 2, 1000 * n + 10 * L + l), E.case_ct(lm, n, batch, 2, 2000 * n + 10 * L + l)
    d_a, d_b = _dev(a), _dev(b)
    want = D.mul(lm, sps, rlk, a, b)
    assert np.array_equal(_mul(pkg, lp, sp, d_rlk, L, d_a, d_b), want)
    ten = E.tensor(lm, a, b)
    out, d_ten = _empty(tuple(d_a.shape)), _dev(ten)
    B.ckks_deep_relinearize_dev(lp, sp, d_rlk.data_ptr(), L, d_ten.data_ptr(), out.data_ptr(), batch)
    assert np.array_equal(_u64(out), want)
    refs = [D.apply_galois(lm, sps, gks[t], a, gs[t]) for t in range(3)]
    for t in (0, 1):                                                 # count 1: a rotation and the conjugation
        assert np.array_equal(_galois(pkg, lp, sp, [d_gks[t]], [gs[t]], L, d_a)[0], refs[t]), gs[t]
    many = _galois(pkg, lp, sp, d_gks, gs, L, d_a)                   # count 3
    for t in range(3):
        assert np.array_equal(many[t], refs[t]), gs[t]
    if l > 1:
        out = _empty((l - 1, 2, batch, n))
        B.ckks_deep_rescale_dev(lp, d_a.data_ptr(), out.data_ptr(), batch)
        assert np.array_equal(_u64(out), D.rescale(lm, a))
    assert np.array_equal(_u64(d_a), a) and np.array_equal(_u64(d_b), b)   # the inputs are only read


@pytest.mark.parametrize("L,alpha,l", SHAPES)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 8, 64, 2048])
def test_entry_points_word_for_word(pkg, tab, n, batch, L, alpha, l):
    _run_case(pkg, tab, n, batch, L, alpha, l)


@pytest.mark.parametrize("L,alpha", [(32, 8), (32, 1)])
def test_thirty_two_limbs(pkg, tab, L, alpha):
    """(32, 1, 32) makes 32 digits: four runs of the key sum's folds"""
    _run_case(pkg, tab, 8, 2, L, alpha, 32)


# ---- alpha = 1, L <= 8: byte for byte the §22 / §23 entry points -------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch", [(2, 1, 1), (8, 3, 3), (64, 8, 2), (2048, 4, 3)])
def test_alpha_one_is_byte_for_byte_the_rns_entry_points(pkg, tab, n, k, batch):
    B = pkg.binding
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    d_s, d_tab = _secret(pkg, plans + [sp], n), _dev(tab)
    g = 5 % (2 * n)
    d_rlk, d_gk = _key(pkg, tab, plans, [sp], d_s, n, E.RLK_BASE), _key(pkg, tab, plans, [sp], d_s, n, G.GK_BASE, g)
    o_rlk, o_gk = _empty((k, k + 1, 2, n)), _empty((k, k + 1, 2, n))
    B.ckks_rns_relin_key_dev(plans, sp, SEED, E.RLK_BASE, d_s.data_ptr(), d_tab.data_ptr(), len(tab), o_rlk.data_ptr())
    B.ckks_rns_galois_key_dev(plans, sp, SEED, G.GK_BASE, g, d_s.data_ptr(), d_tab.data_ptr(), len(tab), o_gk.data_ptr())
    assert np.array_equal(_u64(d_rlk), _u64(o_rlk)) and np.array_equal(_u64(d_gk), _u64(o_gk))
    for l in sorted({k, max(1, k - 1)}):
        a, b = _dev(E.case_ct(mods[:l], n, batch, 2, 7 * n + l)), _dev(E.case_ct(mods[:l], n, batch, 2, 9 * n + l))
        old = _empty(tuple(a.shape))
        B.ckks_rns_mul_dev(plans[:l], sp, o_rlk.data_ptr(), k, a.data_ptr(), b.data_ptr(), old.data_ptr(), batch)
        assert np.array_equal(_mul(pkg, plans[:l], [sp], d_rlk, k, a, b), _u64(old))
        ten, new = _empty((l, 3, batch, n)), _empty(tuple(a.shape))
        B.ckks_rns_tensor_dev(plans[:l], a.data_ptr(), b.data_ptr(), ten.data_ptr(), batch)
        B.ckks_rns_relinearize_dev(plans[:l], sp, o_rlk.data_ptr(), k, ten.data_ptr(), old.data_ptr(), batch)
        B.ckks_deep_relinearize_dev(plans[:l], [sp], d_rlk.data_ptr(), k, ten.data_ptr(), new.data_ptr(), batch)
        assert np.array_equal(_u64(new), _u64(old))
        old = _empty((1, l, 2, batch, n))
        B.ckks_rns_galois_dev(plans[:l], sp, [o_gk.data_ptr()], [g], k, a.data_ptr(), old.data_ptr(), batch)
        assert np.array_equal(_galois(pkg, plans[:l], [sp], [d_gk], [g], k, a), _u64(old))
        if l > 1:
            old, new = _empty((l - 1, 2, batch, n)), _empty((l - 1, 2, batch, n))
            B.ckks_rns_rescale_dev(plans[:l], a.data_ptr(), old.data_ptr(), batch)
            B.ckks_deep_rescale_dev(plans[:l], a.data_ptr(), new.data_ptr(), batch)
            assert np.array_equal(_u64(new), _u64(old))


# ---- the centring's edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,alpha", [(5, 2), (7, 3), (3, 8)])
def test_group_integers_at_the_centring_edges(pkg, tab, L, alpha):
    """d2 built so that every group's integer is 0, 1, floor(Q_j / 2), floor(Q_j / 2) + 1 and Q_j - 1 in turn"""
    n = 8
    mods, sps, rlk, _ = _ref_keys(n, L, alpha, tab)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    d_rlk = _dev(rlk)
    d2 = np.zeros((L, 1, n), dtype=U64)
    for grp in D.groups(L, alpha):
        Q = D.product(mods[i] for i in grp)
        xs = [0, 1, Q // 2, Q // 2 + 1, Q - 1, Q // 2 - 1, Q // 3, 2]
        for i in grp:
            d2[i, 0] = E.fwd(mods[i], n, np.array([x % mods[i] for x in xs], dtype=U64))
    d = np.stack([np.zeros_like(d2), np.zeros_like(d2), d2], axis=1)
    out, d_d = _empty((L, 2, 1, n)), _dev(d)
    pkg.binding.ckks_deep_relinearize_dev(plans, sp, d_rlk.data_ptr(), L, d_d.data_ptr(), out.data_ptr(), 1)
    assert np.array_equal(_u64(out), D.relinearize(mods, sps, rlk, d))


@pytest.mark.parametrize("alpha", [1, 2, 3])
def test_key_sums_at_the_edges_of_p(pkg, alpha):
    """zero "keys" with one chosen column: the digit of group 0 is the constant 1 in every limb, so t_{p_m} is key[0][L + m][0]
    itself, steered to make t modulo P floor(P / 2), floor(P / 2) + 1 and their neighbours"""
    n, L = 8, 4
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    P = D.product(sps)
    ys = [P // 2, P // 2 + 1, P // 2 - 1, 0, 1, P - 1, P // 3, 2]
    key = np.zeros((D.dnum(L, alpha), L + alpha, 2, n), dtype=U64)
    for m, p in enumerate(sps):
        key[0, L + m, 0] = E.fwd(p, n, np.array([y % p for y in ys], dtype=U64))
        key[0, L + m, 1] = E.fwd(p, n, np.array([y % p for y in ys[::-1]], dtype=U64))
    one = np.zeros(n, dtype=U64)
    one[0] = 1
    d = np.zeros((L, 3, 1, n), dtype=U64)
    for i in range(min(alpha, L)):
        d[i, 2, 0] = E.fwd(mods[i], n, one)                          # group 0's integer is 1
    out, d_key, d_d = _empty((L, 2, 1, n)), _dev(key), _dev(d)
    pkg.binding.ckks_deep_relinearize_dev(plans, sp, d_key.data_ptr(), L, d_d.data_ptr(), out.data_ptr(), 1)
    want = D.relinearize(mods, sps, key, d)
    assert np.array_equal(_u64(out), want)
    y = [(v - P if v > P // 2 else v) for v in ys]                   # the definition, by hand: r = -y / P modulo q_i
    c0 = E.inv(mods[0], n, want[0, 0])[0]
    assert [int(v) for v in c0] == [(-v * pow(P, -1, mods[0])) % mods[0] for v in y]


# ---- the chunk, a second stream, alignment ------------------------------------------------------------------------------------------------
def test_a_batch_one_above_the_chunk(pkg, tab):
    n, L, alpha = 8192, 12, 4
    batch = D.chunk_rows(n, L, alpha, 1 << 20) + 1
    assert batch == 2
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    key = E.case_ct(list(mods) + list(sps), n, D.dnum(L, alpha), 2, 77).transpose(2, 0, 1, 3).copy()   # any canonical words serve
    a, b = E.case_ct(mods, n, batch, 2, 78), E.case_ct(mods, n, batch, 2, 79)
    d_key, d_a, d_b = _dev(key), _dev(a), _dev(b)
    assert np.array_equal(_mul(pkg, plans, sp, d_key, L, d_a, d_b), D.mul(mods, sps, key, a, b))
    g = 5
    assert np.array_equal(_galois(pkg, plans, sp, [d_key], [g], L, d_a)[0], D.apply_galois(mods, sps, key, a, g))
    out = _empty((L - 1, 2, batch, n))
    pkg.binding.ckks_deep_rescale_dev(plans, d_a.data_ptr(), out.data_ptr(), batch)
    assert np.array_equal(_u64(out), D.rescale(mods, a))


def test_second_stream_and_misaligned_buffers(pkg, tab):
    import torch

    n, batch, (L, alpha, l) = 64, 3, (9, 3, 7)
    mods, sps, rlk, gks = _ref_keys(n, L, alpha, tab)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    lm, lp = mods[:l], plans[:l]
    a, b = E.case_ct(lm, n, batch, 2, 31), E.case_ct(lm, n, batch, 2, 32)
    want = D.mul(lm, sps, rlk, a, b)

    def off8(x):
        """a copy of x at an address that is 8 modulo 16"""
        buf = _empty((x.size + 3,))
        view = buf[1:1 + x.size] if buf.data_ptr() % 16 == 0 else buf[2:2 + x.size]
        assert view.data_ptr() % 16 == 8
        view.copy_(_dev(x).reshape(-1))
        return buf, view
    keep = [off8(x) for x in (rlk, a, b, np.zeros(a.shape, dtype=U64), gks[0])]
    k_, a_, b_, o_, g_ = [v for _, v in keep]
    B = pkg.binding
    B.ckks_deep_mul_dev(lp, sp, k_.data_ptr(), L, a_.data_ptr(), b_.data_ptr(), o_.data_ptr(), batch)
    assert np.array_equal(_u64(o_).reshape(a.shape), want)
    g = _elements(n)[0]
    og, ogv = off8(np.zeros((1,) + a.shape, dtype=U64))
    B.ckks_deep_galois_dev(lp, sp, [g_.data_ptr()], [g], L, a_.data_ptr(), ogv.data_ptr(), batch)
    assert np.array_equal(_u64(ogv).reshape(a.shape), D.apply_galois(lm, sps, gks[0], a, g))
    orr, orv = off8(np.zeros((l - 1,) + a.shape[1:], dtype=U64))
    B.ckks_deep_rescale_dev(lp, a_.data_ptr(), orv.data_ptr(), batch)
    assert np.array_equal(_u64(orv).reshape((l - 1,) + a.shape[1:]), D.rescale(lm, a))
    assert np.array_equal(_u64(a_).reshape(a.shape), a)
    st = torch.cuda.Stream()
    d_rlk, d_a, d_b = _dev(rlk), _dev(a), _dev(b)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        got = _mul(pkg, lp, sp, d_rlk, L, d_a, d_b, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(got, want)
    assert np.array_equal(_mul(pkg, lp, sp, d_rlk, L, d_a, d_b), want)   # and the default stream after it


# ---- rejections: nothing is written ---------------------------------------------------------------------------------------------------------
def test_every_rejection_leaves_the_output_untouched(pkg, tab):
    B = pkg.binding
    n, L, alpha, batch = 8, 5, 2, 2
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    d_s, d_tab = _secret(pkg, plans + sp, n), _dev(tab)
    key = _dev(np.zeros((3, L + alpha, 2, n), dtype=U64))
    a = _dev(E.case_ct(mods, n, batch, 2, 5))
    ten = _dev(E.case_ct(mods, n, batch, 3, 6))
    out = _empty((2, L, 2, batch, n))
    kout = _empty((3, L + alpha, 2, n))
    other = pkg.Plan(E.primes_below(40, 2 * n, 1)[0], 2 * n)
    wide = pkg.Plan(E.primes_below(63, n, 1)[0], n)
    low = _plans(pkg, E.primes_below(39, n, 2), n)
    P, K_ = out.data_ptr(), key.data_ptr()

    def mul(plans=plans, sp=sp, key=K_, kl=L, a=a.data_ptr(), b=a.data_ptr(), o=P, **kw):
        B.ckks_deep_mul_dev(plans, sp, key, kl, a, b, o, batch, **kw)

    def relin(plans=plans, sp=sp, key=K_, kl=L, d=ten.data_ptr(), o=P, **kw):
        B.ckks_deep_relinearize_dev(plans, sp, key, kl, d, o, batch, **kw)

    def gal(plans=plans, sp=sp, keys=(K_,), gs=(5,), kl=L, i=a.data_ptr(), o=P, **kw):
        B.ckks_deep_galois_dev(plans, sp, None if keys is None else list(keys), None if gs is None else list(gs), kl, i, o, batch, **kw)

    def resc(plans=plans, i=a.data_ptr(), o=P, **kw):
        B.ckks_deep_rescale_dev(plans, i, o, batch, **kw)

    def rkey(plans=plans, sp=sp, row=E.RLK_BASE, s=d_s.data_ptr(), t=d_tab.data_ptr(), m=len(tab), o=kout.data_ptr(), **kw):
        B.ckks_deep_relin_key_dev(plans, sp, SEED, row, s, t, m, o, **kw)

    def gkey(g=5, plans=plans, sp=sp, s=d_s.data_ptr(), o=kout.data_ptr(), **kw):
        B.ckks_deep_galois_key_dev(plans, sp, SEED, G.GK_BASE, g, s, d_tab.data_ptr(), len(tab), o, **kw)

    chain_bad = [
        (B.FHE_E_NULL, dict(plans=None, limbs=L)), (B.FHE_E_NULL, dict(plans=plans[:2] + [None] + plans[3:])),
        (B.FHE_E_NULL, dict(sp=None, alpha=alpha)), (B.FHE_E_NULL, dict(sp=[sp[0], None])),
        (B.FHE_E_INVALID, dict(limbs=0)), (B.FHE_E_INVALID, dict(plans=plans * 7, limbs=33)),
        (B.FHE_E_INVALID, dict(alpha=0)), (B.FHE_E_INVALID, dict(sp=sp * 5, alpha=9)),
        (B.FHE_E_PARAM_MISMATCH, dict(plans=plans[:4] + [other])), (B.FHE_E_PARAM_MISMATCH, dict(sp=[sp[0], other])),
        (B.FHE_E_INVALID, dict(plans=plans[:4] + plans[:1])), (B.FHE_E_INVALID, dict(sp=[sp[0], plans[0]])), (B.FHE_E_INVALID, dict(sp=[sp[0], sp[0]])),
        (B.FHE_E_INVALID, dict(sp=[sp[0], wide])), (B.FHE_E_INVALID, dict(plans=plans[:4] + [wide])),
        (B.FHE_E_INVALID, dict(sp=low)),
    ]
    calls = []
    for fn in (mul, relin, gal, rkey, gkey):
        calls += [(code, fn, kw) for code, kw in chain_bad]
    calls += [(code, resc, kw) for code, kw in chain_bad if "sp" not in kw and "alpha" not in kw]
    for fn in (mul, relin, gal):
        calls += [(B.FHE_E_INVALID, fn, dict(kl=L - 1)), (B.FHE_E_INVALID, fn, dict(kl=33)), (B.FHE_E_NULL, fn, dict(o=None)),
                  (B.FHE_E_INVALID, fn, dict(o=P + 4))]
    calls += [(B.FHE_E_NULL, mul, dict(key=None)), (B.FHE_E_NULL, mul, dict(a=None)), (B.FHE_E_NULL, relin, dict(d=None)),
              (B.FHE_E_INVALID, mul, dict(o=a.data_ptr())), (B.FHE_E_INVALID, mul, dict(o=K_)), (B.FHE_E_INVALID, relin, dict(o=ten.data_ptr() + 8 * n)),
              (B.FHE_E_INVALID, relin, dict(o=K_)),
              (B.FHE_E_INVALID, gal, dict(gs=(4,))), (B.FHE_E_INVALID, gal, dict(gs=(2 * n + 1,))), (B.FHE_E_NULL, gal, dict(keys=(None,))),
              (B.FHE_E_NULL, gal, dict(keys=None, count=1)), (B.FHE_E_NULL, gal, dict(gs=None, count=1)), (B.FHE_E_INVALID, gal, dict(gs=(5,) * 257, keys=(K_,) * 257)),
              (B.FHE_E_INVALID, gal, dict(o=a.data_ptr())), (B.FHE_E_INVALID, gal, dict(o=K_)), (B.FHE_E_INVALID, gal, dict(i=a.data_ptr() + 4)),
              (B.FHE_E_INVALID, resc, dict(plans=plans[:1])), (B.FHE_E_INVALID, resc, dict(o=a.data_ptr() + 8 * n)), (B.FHE_E_NULL, resc, dict(i=None)),
              (B.FHE_E_INVALID, gkey, dict(g=6)), (B.FHE_E_INVALID, gkey, dict(g=2 * n + 1)), (B.FHE_E_NULL, rkey, dict(s=None)), (B.FHE_E_NULL, rkey, dict(o=None)),
              (B.FHE_E_INVALID, rkey, dict(o=d_s.data_ptr())), (B.FHE_E_INVALID, rkey, dict(row=(1 << 63) - 2)), (B.FHE_E_INVALID, rkey, dict(m=2000))]
    for code, fn, kw in calls:
        with _refused() as e:
            fn(**kw)
        assert e.value.code == code, (fn.__name__, kw, e.value)
    import torch

    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((kout == FILL).all())
    assert np.array_equal(_u64(key), np.zeros((3, L + alpha, 2, n), dtype=U64))
    # batch = 0 and count = 0 are no-ops
    B.ckks_deep_mul_dev(plans, sp, None, L, None, None, None, 0)
    B.ckks_deep_relinearize_dev(plans, sp, None, L, None, None, 0)
    B.ckks_deep_rescale_dev(plans, None, None, 0)
    B.ckks_deep_galois_dev(plans, sp, None, None, L, None, None, 0, count=3)
    B.ckks_deep_galois_dev(plans, sp, [], [], L, a.data_ptr(), P, batch, count=0)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())


# ---- the workspace and the launch counts ---------------------------------------------------------------------------------------------------
def test_workspace_bytes_and_launch_counts(pkg, tab):
    import torch

    B = pkg.binding
    for n, l, a, b in ((8, 32, 8, 1), (8, 32, 1, 5), (8192, 12, 4, 2), (4096, 8, 1, 1024), (64, 17, 8, 3), (2, 1, 1, 1), (2048, 12, 4, 700)):
        assert B.ckks_deep_workspace_bytes(n, l, a, b) == D.workspace_bytes(n, l, a, b) > 0
    for n, l, a, b in ((8, 33, 1, 1), (8, 0, 1, 1), (8, 4, 9, 1), (8, 4, 0, 1), (8, 4, 1, 0), (12, 4, 1, 1)):
        assert B.ckks_deep_workspace_bytes(n, l, a, b) == 0

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
        labs = {"extend": "ckks_deep_extend", "keymac": "ckks_deep_keymac", "tensor": "ckks_rns_tensor", "divround": "ckks_rns_divround", "lift": "ckks_rns_lift",
                "rns_keymac": "ckks_rns_keymac"}
        return {k: sum(c for name, (_, c) in got.items() if name.startswith(v)) for k, v in labs.items()}

    n, batch = 64, 3
    for L, alpha, l in ((9, 3, 7), (5, 2, 5), (3, 8, 3), (4, 1, 4)):
        mods, sps = D.case_chain(n, L, alpha)
        plans, sp = _plans(pkg, mods, n)[:l], _plans(pkg, sps, n)
        ng = D.dnum(l, alpha)
        keys = [_dev(np.random.default_rng(r).integers(0, 1 << 38, (D.dnum(L, alpha), L + alpha, 2, n), dtype=np.uint64)) for r in range(3)]
        a = _dev(E.case_ct(mods[:l], n, batch, 2, 3))
        out = _empty((3, l, 2, batch, n))
        gs = _elements(n)
        got = counts(lambda: B.ckks_deep_mul_dev(plans, sp, keys[0].data_ptr(), L, a.data_ptr(), a.data_ptr(), out[0].data_ptr(), batch))
        assert got == dict(extend=ng + 1, keymac=l + alpha, tensor=l, divround=l, lift=0, rns_keymac=0), (L, alpha, l)
        for R in (1, 3):                                             # one digit pass for any count of Galois elements
            got = counts(lambda: B.ckks_deep_galois_dev(plans, sp, [x.data_ptr() for x in keys[:R]], gs[:R], L, a.data_ptr(), out.data_ptr(), batch))
            assert got == dict(extend=ng + R, keymac=R * (l + alpha), tensor=0, divround=R * l, lift=0, rns_keymac=0), (L, alpha, l, R)
        got = counts(lambda: B.ckks_deep_rescale_dev(plans, a.data_ptr(), out[0].data_ptr(), batch))
        assert got == dict(extend=1, keymac=0, tensor=0, divround=l - 1, lift=0, rns_keymac=0)


# ---- end to end: a product chain of 11 ciphertexts at n = 64, L = 12, alpha = 3, Delta = 2^40 -------------------------------------------
E2E_SEED = bytes((13 * i + 1) % 256 for i in range(32))
E2E_RNG = 3601


def _e2e_restated(tab):
    """the chain in the restatement -> everything the device run is compared with"""
    n, L, alpha, delta, rows = 64, 12, 3, float(1 << 40), 2
    mods, sps = D.e2e_chain(n, L, alpha)
    s = K.secret_key(E2E_SEED, 0, n)
    pk = E.public_key(E2E_SEED, E.PK_BASE, s, mods, tab)
    rlk = D.switch_key(E2E_SEED, E.RLK_BASE, s, mods, sps, tab)
    r = np.random.default_rng(E2E_RNG)
    zs = [np.exp(2j * np.pi * r.random((rows, n // 2))) * (0.9 + 0.2 * r.random((rows, n // 2))) for _ in range(11)]
    ms = [K.encode(z, delta) for z in zs]
    cts = [E.encrypt(E2E_SEED, t * rows, pk, m, rows, mods, tab) for t, m in enumerate(ms)]
    acc, scale, level = cts[0], delta, L - 1
    for t in range(1, 11):
        lm = mods[:level + 1]
        acc = D.rescale(lm, D.mul(lm, sps, rlk, acc, cts[t][:level + 1]))
        scale = scale * delta / mods[level]
        level -= 1
    assert level == 1                                                # ten products, ten rescales; level 0 is its truncation
    acc = acc[:1]
    dec = E.decrypt(mods, n, s, acc)
    prod = zs[0]
    for z in zs[1:]:
        prod = prod * z
    got = K.decode(dec, scale)
    # level 5: a rotation and the conjugation of the fresh ciphertext cut to six limbs
    lm = mods[:6]
    gs = [G.galois_element(n, 3), G.conjugation_element(n)]
    gks = [D.switch_key(E2E_SEED, G.GK_BASE + 64 * t, s, mods, sps, tab, g) for t, g in enumerate(gs)]
    moved = [D.apply_galois(lm, sps, gks[t], cts[0][:6], gs[t]) for t in range(2)]
    moved_z = [K.decode(E.decrypt(lm, n, s, m), delta) for m in moved]
    want_z = [G.from_rotation_order(np.roll(G.to_rotation_order(zs[0]), -3, axis=-1)), np.conj(zs[0])]
    return dict(n=n, mods=mods, sps=sps, delta=delta, rows=rows, zs=zs, ms=ms, cts=cts, rlk=rlk, gks=gks, gs=gs, acc=acc, scale=scale, dec=dec, prod=prod,
                err=float(np.abs(got - prod).max()), moved=moved, want_z=want_z, moved_err=[float(np.abs(a - b).max()) for a, b in zip(moved_z, want_z)])


def test_product_chain_of_eleven_through_the_client_key(pkg, tab):
    """Word-equal to the restatement at every step; the decoded product within 4 x the restatement's own maximum error on the
    same inputs (E2E_SEED, E2E_RNG; the figure is in DESIGN.md §36); a rotation and the conjugation at level 5 under the same rule."""
    ck = pkg.ckks
    r = _e2e_restated(tab)
    n = r["n"]
    param = ck.DeepParam(n, r["mods"], r["sps"])
    assert (param.max_level, param.dnum) == (11, 4)
    key = ck.DeepClientKey.generate(E2E_SEED, param, r["delta"])
    pk = key.public_key(0)
    rlk = key.relin_key(0)
    assert np.array_equal(_u64(rlk.d_rlk), r["rlk"])
    cts = [key.encrypt(pk, m) for m in r["ms"]]
    for ct, want in zip(cts, r["cts"]):
        assert isinstance(ct, ck.DeepCiphertext) and ct.level == 11 and np.array_equal(_u64(ct.d), want)
    acc = cts[0]
    for t in range(1, 11):
        acc = acc.mul(cts[t], rlk).rescale()
    assert acc.level == 1
    acc = acc.at_level(0)
    assert acc.level == 0 and np.array_equal(_u64(acc.d), r["acc"]) and abs(acc.scale - r["scale"]) <= 1e-9 * r["scale"]
    assert np.array_equal(key.decrypt(acc), r["dec"])
    got = key.decrypt_and_decode(acc)
    err = float(np.abs(got - r["prod"]).max())
    print(f"product of 11: device error {err:.3e}, restatement error {r['err']:.3e}")
    assert err <= 4 * r["err"]
    low = cts[0].at_level(5)
    gks = [key.rotation_key(3, 0), key.conjugation_key(1)]
    for t in range(2):
        assert gks[t].g == r["gs"][t] and np.array_equal(_u64(gks[t].d_gk), r["gks"][t])
    moved = [low.rotate(gks[0]), low.conjugate(gks[1])]
    many = low.rotate_many(gks)
    for t in range(2):
        assert moved[t].level == 5 and np.array_equal(_u64(moved[t].d), r["moved"][t]) and np.array_equal(_u64(many[t].d), r["moved"][t])
        e = float(np.abs(key.decrypt_and_decode(moved[t]) - r["want_z"][t]).max())
        print(f"galois {r['gs'][t]} at level 5: device error {e:.3e}, restatement error {r['moved_err'][t]:.3e}")
        assert e <= 4 * r["moved_err"][t]
    # the rest of the surface, per limb: +, -, unary minus, add_plain, mul_plain against the restatement
    a, b = cts[0], cts[1]
    mods = r["mods"]
    assert np.array_equal(_u64((a + b).d), np.stack([E.padd(q, r["cts"][0][i], r["cts"][1][i]) for i, q in enumerate(mods)]))
    assert np.array_equal(_u64((a - b).d), np.stack([E.psub(q, r["cts"][0][i], r["cts"][1][i]) for i, q in enumerate(mods)]))
    assert np.array_equal(_u64((-a).d), np.stack([E.psub(q, np.zeros_like(r["cts"][0][i]), r["cts"][0][i]) for i, q in enumerate(mods)]))
    assert np.array_equal(_u64(a.add_plain(r["ms"][1]).d), E.add_plain(mods, n, r["cts"][0], r["ms"][1]))
    mp = a.mul_plain(r["ms"][1], r["delta"])
    assert isinstance(mp, ck.DeepCiphertext) and np.array_equal(_u64(mp.d), E.mul_plain(mods, n, r["cts"][0], r["ms"][1]))
    with pytest.raises(NotImplementedError):
        a.add_const(1.0)
    with pytest.raises(ValueError):
        low.rotate(gks[1])
