"""Plaintext linear transforms on the deep CKKS chain on the device (ckks_deep.hip): fhe_ckks_deep_diag_sum_dev word
for word against tests/_ckks_deep_linear_numpy.py (tolerance zero), which tests/test_ckks_deep_linear_cpu.py proved; at alpha = 1
byte for byte against fhe_ckks_rns_diag_sum_dev; the centring's edges; the chunk; a second stream; misaligned buffers; every
rejection with its outputs untouched; the launch counts; and two stacked matrix-vector products through ckks.DeepClientKey."""
import numpy as np
import pytest

import _ckks_deep_linear_numpy as DL
import _ckks_deep_numpy as D
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_linear_numpy as LN
import _ckks_numpy as K
import _client_numpy as C
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
FILL = 0x5A5A5A5A5A5A5A5A
SHAPES = [(5, 2, 5), (5, 2, 4), (9, 3, 7), (17, 8, 17), (3, 8, 3)]            # (L, alpha, l)
OUTPUTS = (1, 2, DL.OUT_CAP + 1)                                             # either side of the register cap


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


def _keys_dev(keys):
    return [None if x is None else _dev(x) for x in keys]


def _diag(pkg, plans, sp, d_keys, gs, kl, d_pts, outputs, d_ct, stream=None):
    k, _, batch, n = d_ct.shape
    out = _empty((outputs, k, 2, batch, n))
    pkg.binding.ckks_deep_diag_sum_dev(plans, sp, None if d_keys is None else [None if x is None else x.data_ptr() for x in d_keys], gs, kl, d_pts.data_ptr(),
                                       outputs, d_ct.data_ptr(), out.data_ptr(), batch, stream)
    return _u64(out)


# ---- the sweep, word for word ---------------------------------------------------------------------------------------------------------
def _run_case(pkg, n, batch, L, alpha, l, lists=None):
    mods, sps = D.case_chain(n, L, alpha)
    lm = mods[:l]
    plans, sp = _plans(pkg, lm, n), _plans(pkg, sps, n)
    ct = E.case_ct(lm, n, batch, 2, 300 * n + 10 * L + l)
    d_ct = _dev(ct)
    top = max(OUTPUTS)
    every = DL.element_lists(n)
    for t, gs in enumerate(every):
        if lists is not None and t not in lists:
            continue
        keys = DL.random_keys(lm, sps, n, gs, 40 * n + t, key_mods=mods)     # the key of the whole chain, at level l - 1
        pts = DL.random_pts(lm, sps, n, top, len(gs), 41 * n + t)
        want = DL.diag_sum(lm, sps, keys, gs, pts, ct)
        d_keys = _keys_dev(keys)
        for outputs in OUTPUTS:                                              # the outputs are independent: the first o of the largest call
            got = _diag(pkg, plans, sp, d_keys, gs, L, _dev(pts[:outputs]), outputs, d_ct)
            assert np.array_equal(got, want[:outputs]), (gs, outputs)
        if all(g == 1 for g in gs):                                          # the identity alone: d_gks itself may be NULL
            assert np.array_equal(_diag(pkg, plans, sp, None, gs, L, _dev(pts), top, d_ct), want)
    assert np.array_equal(_u64(d_ct), ct)                                    # the input is only read


@pytest.mark.parametrize("L,alpha,l", SHAPES)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [2, 8, 64])
def test_diag_sum_word_for_word(pkg, n, batch, L, alpha, l):
    assert [len(x) for x in DL.element_lists(n)] == [1, 1, 3, 3, DL.GROUP, DL.GROUP + 1]
    _run_case(pkg, n, batch, L, alpha, l)


@pytest.mark.parametrize("L,alpha", [(32, 8), (32, 1)])
def test_thirty_two_limbs(pkg, L, alpha):
    """(32, 1, 32) makes 32 digits: every fold of the inner sum; the mixed list of three and the list of 17 (one CARRY launch)"""
    _run_case(pkg, 8, 1, L, alpha, 32, lists=(2, 5))


def test_diag_sum_at_2048(pkg):
    _run_case(pkg, 2048, 2, 5, 2, 4, lists=(2,))


# ---- alpha = 1, l <= 8: byte for byte §24's entry point -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(64, 1), (64, 3), (16, 8)])
def test_alpha_one_is_byte_for_byte_the_rns_entry_point(pkg, n, k):
    """this oracle shares no code with the restatement"""
    B = pkg.binding
    batch = 3
    mods, P = E.primes_below(40, n, k), E.primes_below(41, n, 1)[0]
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    d_ct = _dev(E.case_ct(mods, n, batch, 2, 17 * n + k))
    for t, gs in enumerate(DL.element_lists(n)):
        d_keys = _keys_dev(LN.random_keys(mods, P, n, gs, 70 + t))
        d_pts = _dev(LN.random_pts(mods, P, n, 3, len(gs), 80 + t))
        old = _empty((3, k, 2, batch, n))
        B.ckks_rns_diag_sum_dev(plans, sp, [None if x is None else x.data_ptr() for x in d_keys], gs, k, d_pts.data_ptr(), 3, d_ct.data_ptr(), old.data_ptr(), batch)
        assert np.array_equal(_diag(pkg, plans, [sp], d_keys, gs, k, d_pts, 3, d_ct), _u64(old)), gs


# ---- the centring's edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,alpha", [(5, 2), (7, 3), (3, 8)])
def test_group_integers_at_the_centring_edges(pkg, L, alpha):
    """c1 built as §36's test builds d2: every group's integer is 0, 1, floor(Q_j / 2), floor(Q_j / 2) + 1 and Q_j - 1 in turn"""
    n = 8
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    ct = E.case_ct(mods, n, 1, 2, 90 + L)
    for grp in D.groups(L, alpha):
        Q = D.product(mods[i] for i in grp)
        xs = [0, 1, Q // 2, Q // 2 + 1, Q - 1, Q // 2 - 1, Q // 3, 2]
        for i in grp:
            ct[i, 1, 0] = E.fwd(mods[i], n, np.array([x % mods[i] for x in xs], dtype=U64))
    gs = [5, 1, 2 * n - 1]
    keys = DL.random_keys(mods, sps, n, gs, 91)
    pts = DL.random_pts(mods, sps, n, 2, 3, 92)
    assert np.array_equal(_diag(pkg, plans, sp, _keys_dev(keys), gs, L, _dev(pts), 2, _dev(ct)), DL.diag_sum(mods, sps, keys, gs, pts, ct))


@pytest.mark.parametrize("alpha", [1, 2, 3])
def test_weighted_sums_at_the_edges_of_p(pkg, alpha):
    """zero "keys" with one chosen column, as §36's test: group 0's integer is the constant 1 and the plaintext is the constant 1,
    so U modulo p_m is key[0][L + m] itself, steered to make U modulo P floor(P / 2), floor(P / 2) + 1 and their neighbours"""
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
    ct = np.zeros((L, 2, 1, n), dtype=U64)
    for i in range(min(alpha, L)):
        ct[i, 1, 0] = E.fwd(mods[i], n, one)                                 # group 0's integer is 1; its evals are all ones, whatever pi_g
    pts = np.ones((1, 1, L + alpha, n), dtype=U64)
    g = 5
    want = DL.diag_sum(mods, sps, [key], [g], pts, ct)
    assert np.array_equal(_diag(pkg, plans, sp, [_dev(key)], [g], L, _dev(pts), 1, _dev(ct)), want)
    y = [(v - P if v > P // 2 else v) for v in ys]                           # the definition, by hand: r = -y / P modulo q_i
    c0 = E.inv(mods[0], n, want[0, 0, 0])[0]
    assert [int(v) for v in c0] == [(-v * pow(P, -1, mods[0])) % mods[0] for v in y]


# ---- the chunk, a second stream, alignment ------------------------------------------------------------------------------------------------
def test_a_batch_one_above_the_chunk(pkg):
    n, l, alpha, count, outputs = 8192, 4, 2, 3, 2
    batch = DL.chunk_rows(n, l, alpha, 1 << 20, outputs) + 1
    assert batch == 6
    mods, sps = D.case_chain(n, l, alpha)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    gs = [1, 5, 2 * n - 1]
    ct = E.case_ct(mods, n, batch, 2, 77)
    keys, pts = DL.random_keys(mods, sps, n, gs, 78), DL.random_pts(mods, sps, n, outputs, count, 79)
    assert np.array_equal(_diag(pkg, plans, sp, _keys_dev(keys), gs, l, _dev(pts), outputs, _dev(ct)), DL.diag_sum(mods, sps, keys, gs, pts, ct))


def test_second_stream_and_misaligned_buffers(pkg):
    import torch

    n, batch, (L, alpha, l) = 64, 3, (9, 3, 7)
    mods, sps = D.case_chain(n, L, alpha)
    lm = mods[:l]
    plans, sp = _plans(pkg, lm, n), _plans(pkg, sps, n)
    gs = [5, 1, 2 * n - 1]
    ct = E.case_ct(lm, n, batch, 2, 31)
    keys, pts = DL.random_keys(lm, sps, n, gs, 32, key_mods=mods), DL.random_pts(lm, sps, n, 3, 3, 33)
    want = DL.diag_sum(lm, sps, keys, gs, pts, ct)

    def off8(x):
        """a copy of x at an address that is 8 modulo 16"""
        buf = _empty((x.size + 3,))
        view = buf[1:1 + x.size] if buf.data_ptr() % 16 == 0 else buf[2:2 + x.size]
        assert view.data_ptr() % 16 == 8
        view.copy_(_dev(x).reshape(-1))
        return buf, view
    keep = [off8(x) for x in (keys[0], keys[2], pts, ct, np.zeros(want.shape, dtype=U64))]
    k0, k2, p_, c_, o_ = [v for _, v in keep]
    B = pkg.binding
    B.ckks_deep_diag_sum_dev(plans, sp, [k0.data_ptr(), None, k2.data_ptr()], gs, L, p_.data_ptr(), 3, c_.data_ptr(), o_.data_ptr(), batch)
    assert np.array_equal(_u64(o_).reshape(want.shape), want)
    o_.fill_(FILL)
    B.ckks_deep_diag_sum_dev(plans, sp, None, [1, 1, 1], L, p_.data_ptr(), 3, c_.data_ptr(), o_.data_ptr(), batch)   # the pass without a workspace
    assert np.array_equal(_u64(o_).reshape(want.shape), DL.diag_sum(lm, sps, [None] * 3, [1, 1, 1], pts, ct))
    assert np.array_equal(_u64(c_).reshape(ct.shape), ct)
    # a stream of the high-priority pool: the default pool hands its streams out in turn, and later tests that count the
    # workspace a fresh stream holds (tests/test_round3_gpu.py) depend on which of them they are given
    st = torch.cuda.Stream(priority=-1)
    d_keys, d_pts, d_ct = _keys_dev(keys), _dev(pts), _dev(ct)
    torch.cuda.synchronize()
    B._check(B.load_library().fhe_ntt_release_stream_workspace(st.cuda_stream))
    held = B.load_library().fhe_ntt_workspace_bytes()
    with torch.cuda.stream(st):
        got = _diag(pkg, plans, sp, d_keys, gs, L, d_pts, 3, d_ct, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(got, want)
    assert B.load_library().fhe_ntt_workspace_bytes() >= held + DL.workspace_bytes(n, l, alpha, batch, 3, 3)   # the stream's own workspace
    B._check(B.load_library().fhe_ntt_release_stream_workspace(st.cuda_stream))          # and nothing of it is left behind
    assert B.load_library().fhe_ntt_workspace_bytes() == held
    assert np.array_equal(_diag(pkg, plans, sp, d_keys, gs, L, d_pts, 3, d_ct), want)   # and the default stream after it


# ---- rejections: nothing is written ---------------------------------------------------------------------------------------------------------
def test_every_rejection_leaves_the_output_untouched(pkg):
    import torch

    B = pkg.binding
    n, L, alpha, batch = 8, 5, 2, 2
    mods, sps = D.case_chain(n, L, alpha)
    plans, sp = _plans(pkg, mods, n), _plans(pkg, sps, n)
    key = _dev(np.zeros((3, L + alpha, 2, n), dtype=U64))
    a = _dev(E.case_ct(mods, n, batch, 2, 5))
    pts = _dev(DL.random_pts(mods, sps, n, 2, 2, 6))
    out = _empty((2, L, 2, batch, n))
    other = pkg.Plan(E.primes_below(40, 2 * n, 1)[0], 2 * n)
    wide = pkg.Plan(E.primes_below(63, n, 1)[0], n)
    low = _plans(pkg, E.primes_below(39, n, 2), n)
    P, K_ = out.data_ptr(), key.data_ptr()

    def diag(plans=plans, sp=sp, keys=(K_, None), gs=(5, 1), kl=L, p=pts.data_ptr(), outputs=2, i=a.data_ptr(), o=P, batch=batch, **kw):
        B.ckks_deep_diag_sum_dev(plans, sp, None if keys is None else list(keys), None if gs is None else list(gs), kl, p, outputs, i, o, batch, **kw)

    calls = [
        (B.FHE_E_NULL, dict(plans=None, limbs=L)), (B.FHE_E_NULL, dict(plans=plans[:2] + [None] + plans[3:])),          # check_deep's
        (B.FHE_E_NULL, dict(sp=None, alpha=alpha)), (B.FHE_E_NULL, dict(sp=[sp[0], None])),
        (B.FHE_E_INVALID, dict(limbs=0)), (B.FHE_E_INVALID, dict(plans=plans * 7, limbs=33)),
        (B.FHE_E_INVALID, dict(alpha=0)), (B.FHE_E_INVALID, dict(sp=sp * 5, alpha=9)),
        (B.FHE_E_PARAM_MISMATCH, dict(plans=plans[:4] + [other])), (B.FHE_E_PARAM_MISMATCH, dict(sp=[sp[0], other])),
        (B.FHE_E_INVALID, dict(plans=plans[:4] + plans[:1])), (B.FHE_E_INVALID, dict(sp=[sp[0], plans[0]])), (B.FHE_E_INVALID, dict(sp=[sp[0], sp[0]])),
        (B.FHE_E_INVALID, dict(sp=[sp[0], wide])), (B.FHE_E_INVALID, dict(plans=plans[:4] + [wide])),
        (B.FHE_E_INVALID, dict(sp=low)),
        (B.FHE_E_INVALID, dict(kl=L - 1)), (B.FHE_E_INVALID, dict(kl=33)),                                               # check_key_limbs's
        (B.FHE_E_INVALID, dict(gs=(5,) * 257, keys=(K_,) * 257)), (B.FHE_E_INVALID, dict(outputs=0)), (B.FHE_E_INVALID, dict(outputs=65)),   # §24's
        (B.FHE_E_INVALID, dict(batch=1 << 58)),
        (B.FHE_E_NULL, dict(gs=None, count=2)), (B.FHE_E_NULL, dict(p=None)), (B.FHE_E_NULL, dict(i=None)), (B.FHE_E_NULL, dict(o=None)),
        (B.FHE_E_INVALID, dict(p=pts.data_ptr() + 4)), (B.FHE_E_INVALID, dict(i=a.data_ptr() + 4)), (B.FHE_E_INVALID, dict(o=P + 4)),
        (B.FHE_E_NULL, dict(keys=(None, None))), (B.FHE_E_NULL, dict(keys=None, count=2)), (B.FHE_E_NULL, dict(keys=(K_, None), gs=(1, 5))),
        (B.FHE_E_INVALID, dict(keys=(K_ + 4, None))),
        (B.FHE_E_INVALID, dict(gs=(4, 1))), (B.FHE_E_INVALID, dict(gs=(5, 2 * n + 1))), (B.FHE_E_INVALID, dict(gs=(5, 0))),
        (B.FHE_E_INVALID, dict(o=a.data_ptr())), (B.FHE_E_INVALID, dict(o=a.data_ptr() + 8 * n)), (B.FHE_E_INVALID, dict(o=K_)),
        (B.FHE_E_INVALID, dict(o=pts.data_ptr())),
    ]
    for code, kw in calls:
        with _refused() as e:
            diag(**kw)
        assert e.value.code == code, (kw, e.value)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert np.array_equal(_u64(key), np.zeros((3, L + alpha, 2, n), dtype=U64))
    # batch = 0 and count = 0 are no-ops
    B.ckks_deep_diag_sum_dev(plans, sp, None, None, L, None, 2, None, None, 0, count=2)
    B.ckks_deep_diag_sum_dev(plans, sp, [], [], L, pts.data_ptr(), 2, a.data_ptr(), P, batch, count=0)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # an element 1 beside a NULL key is accepted, and the call then writes
    diag()
    torch.cuda.synchronize()
    assert not bool((out == FILL).any())


# ---- the launch counts ----------------------------------------------------------------------------------------------------------------------
def test_launch_counts(pkg):
    import torch

    B = pkg.binding

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
        labs = {"extend": "ckks_deep_extend", "diagmac": "ckks_deep_diagmac", "keymac": "ckks_deep_keymac", "divround": "ckks_rns_divround"}
        return {k: sum(c for name, (_, c) in got.items() if name.startswith(v)) for k, v in labs.items()}, set(got)

    n, batch = 64, 3
    R = DL.GROUP + 1
    for L, alpha, l in ((9, 3, 7), (5, 2, 5), (3, 8, 3), (4, 1, 4)):
        mods, sps = D.case_chain(n, L, alpha)
        plans, sp = _plans(pkg, mods, n)[:l], _plans(pkg, sps, n)
        keys = [_dev(np.random.default_rng(r).integers(0, 1 << 38, (D.dnum(L, alpha), L + alpha, 2, n), dtype=np.uint64)) for r in range(3)] * 6
        gs = [5, 25, 2 * n - 1] * 6
        a = _dev(E.case_ct(mods[:l], n, batch, 2, 3))
        d_pts = _dev(np.random.default_rng(3).integers(0, 1 << 38, (3, R, l + alpha, n), dtype=np.uint64))
        out = _empty((3, l, 2, batch, n))
        assert DL.chunk_rows(n, l, alpha, batch, 3) == batch                 # one chunk
        for count in (1, 3, DL.GROUP, R):
            for outputs in OUTPUTS:
                pt = d_pts[:outputs, :count].contiguous()
                got, _ = counts(lambda: B.ckks_deep_diag_sum_dev(plans, sp, [x.data_ptr() for x in keys[:count]], gs[:count], L, pt.data_ptr(), outputs, a.data_ptr(),
                                                                 out.data_ptr(), batch))
                assert got == DL.launch_counts(l, alpha, count, outputs), (L, alpha, l, count, outputs)
                assert got == dict(extend=D.dnum(l, alpha) + outputs, diagmac=(l + alpha) * -(-outputs // DL.OUT_CAP) * -(-count // 16), keymac=0, divround=outputs * l)
        pt = d_pts[:3, :R].contiguous()
        got, names = counts(lambda: B.ckks_deep_diag_sum_dev(plans, sp, None, [1] * R, L, pt.data_ptr(), 3, a.data_ptr(), out.data_ptr(), batch))
        assert got == DL.launch_counts(l, alpha, R, 3, switched=False) and got["extend"] == 0
        assert names and all(x.startswith("ckks_deep_diagmac") for x in names)   # the identity alone: no extend, no transform, no modulus-down
        # §36's counts are as they were
        got, _ = counts(lambda: B.ckks_deep_galois_dev(plans, sp, [x.data_ptr() for x in keys[:3]], gs[:3], L, a.data_ptr(), out.data_ptr(), batch))
        assert got == dict(extend=D.dnum(l, alpha) + 3, diagmac=0, keymac=3 * (l + alpha), divround=3 * l)


# ---- end to end: two stacked matrix-vector products at n = 64, L = 12, alpha = 3, Delta = 2^40 ----------------------------------------------
E2E_SEED = bytes((29 * i + 3) % 256 for i in range(32))
E2E_RNG = 3701


def _pt_coeffs(mods, sps, n, d_pts):
    """the centred integer coefficients of a plaintext set, from its limb under p_0, and the check that every limb holds the
    residues of the same polynomial"""
    pts = _u64(d_pts)
    l = len(mods)
    coef = K.centre(E.inv(sps[0], n, pts[..., l, :]), sps[0])
    for i, q in enumerate(list(mods) + list(sps)):
        assert np.array_equal(pts[..., i, :], E.fwd(q, n, E.residues(coef, q)))
    return pts


def test_two_stacked_matrices_through_the_client_key(pkg, tab):
    """ct.linear_transform(A).rescale().linear_transform(B).rescale(): word-equal to the restatement at each step; the result
    decodes to B A w within 4 x the restatement's own maximum error on the same inputs (E2E_SEED, E2E_RNG; the figure is in
    DESIGN.md §37), the rule of §36's end-to-end test."""
    ck = pkg.ckks
    n, L, alpha, delta, rows = 64, 12, 3, float(1 << 40), 2
    N = n // 2
    mods, sps = D.e2e_chain(n, L, alpha)
    param = ck.DeepParam(n, mods, sps)
    key = ck.DeepClientKey.generate(E2E_SEED, param, delta)
    r = np.random.default_rng(E2E_RNG)
    z = np.exp(2j * np.pi * r.random((rows, N))) * (0.9 + 0.2 * r.random((rows, N)))
    A = (r.uniform(-1, 1, (N, N)) + 1j * r.uniform(-1, 1, (N, N))) / 8
    Bm = (r.uniform(-1, 1, (N, N)) + 1j * r.uniform(-1, 1, (N, N))) / 8
    # the restatement's keys and ciphertext
    s = K.secret_key(E2E_SEED, 0, n)
    pk_ref = E.public_key(E2E_SEED, E.PK_BASE, s, mods, tab)
    msg = K.encode(z, delta)
    ct_ref = E.encrypt(E2E_SEED, 0, pk_ref, msg, rows, mods, tab)
    ct = key.encrypt(key.public_key(0), msg)
    assert isinstance(ct, ck.DeepCiphertext) and ct.level == 11 and np.array_equal(_u64(ct.d), ct_ref)
    ltA = ck.LinearTransform.from_matrix(param, key.encoder, A, 11, float(mods[11]))
    ltB = ck.LinearTransform.from_matrix(param, key.encoder, Bm, 10, float(mods[10]))
    assert isinstance(ltA.pts, ck.DeepPlaintextSet) and tuple(ltA.pts.d_pts.shape) == (6, 6, 12 + alpha, n) and tuple(ltB.pts.d_pts.shape) == (6, 6, 11 + alpha, n)
    assert (ltA.n1, ltA.baby, ltA.giant) == DL.bsgs_diagonals(A)[:3] == (6, list(range(6)), list(range(6)))
    steps = ltA.required_steps()
    assert steps == ltB.required_steps() == [1, 2, 3, 4, 5, 6, 12, 18, 24, 30]
    keys = {st: key.rotation_key(st, slot) for slot, st in enumerate(steps)}
    gks = {st: D.switch_key(E2E_SEED, G.GK_BASE + 64 * slot, s, mods, sps, tab, G.galois_element(n, st)) for slot, st in enumerate(steps)}
    for st in steps:
        assert np.array_equal(_u64(keys[st].d_gk), gks[st])
    acc, acc_ref, scale = ct, ct_ref, delta
    for lt, level in ((ltA, 11), (ltB, 10)):
        lm = mods[:level + 1]
        pts = _pt_coeffs(lm, sps, n, lt.pts.d_pts)
        inner_ref, res_ref = DL.linear_transform(lm, sps, lt.n1, lt.baby, lt.giant, pts, gks, acc_ref)
        inner = acc.diag_sum(lt.pts, [keys[i] if i else None for i in lt.baby])
        assert len(inner) == 6
        for o in range(6):
            assert isinstance(inner[o], ck.DeepCiphertext) and (inner[o].level, inner[o].scale) == (level, acc.scale * float(mods[level]))
            assert np.array_equal(_u64(inner[o].d), inner_ref[o]), (level, o)
        res = acc.linear_transform(lt, keys)
        assert isinstance(res, ck.DeepCiphertext) and res.level == level and np.array_equal(_u64(res.d), res_ref)
        acc, acc_ref = res.rescale(), D.rescale(lm, res_ref)
        assert acc.level == level - 1 and np.array_equal(_u64(acc.d), acc_ref) and abs(acc.scale - scale) <= 1e-9 * scale
    two = ct.diag_sum(ck.DeepPlaintextSet(param, 11, ltA.pts.d_pts[:2].contiguous(), ltA.pts.scale, ltA.pts.gs), [keys[i] if i else None for i in ltA.baby])
    assert len(two) == 2 and all(isinstance(x, ck.DeepCiphertext) and (x.level, x.scale) == (11, delta * mods[11]) for x in two)
    want = G.from_rotation_order(G.to_rotation_order(z) @ A.T @ Bm.T)
    low = acc.at_level(0)
    dec_ref = E.decrypt(mods[:1], n, s, acc_ref[:1])
    assert np.array_equal(key.decrypt(low), dec_ref)
    ref_err = float(np.abs(K.decode(dec_ref, scale) - want).max())
    err = float(np.abs(key.decrypt_and_decode(low) - want).max())
    print(f"B A w at n = 64, L = 12, alpha = 3: device error {err:.3e}, restatement error {ref_err:.3e}")
    assert err <= 4 * ref_err
    with pytest.raises(NotImplementedError):
        ct.add_const(1.0)
