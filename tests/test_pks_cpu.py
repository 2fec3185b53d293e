"""The packing key switch, the box expansion and the two-digit tree lookup of DESIGN.md §16 without a device: the numpy
restatement (tests/_pks_numpy.py) with noise-free keys at N = 256, n_in = 8 — the packed phase is the sum of the input
phases at their strides within the rounding bound, wrap signs included; the expansion of a packed table is §14's test
vector for every t; the ideal tree lookup returns table2d[x][y] — and the word counts and argument checks of the new
entry points, which fail before anything touches a GPU."""
import numpy as np
import pytest

import _cb_numpy as CB
import _lut_numpy as LN
import _pks_numpy as PK
import _tfhe_numpy as R

N, N_IN = 256, 8


@pytest.mark.parametrize("b,l", [(8, 4), (1, 3), (3, 7), (16, 4), (32, 2)])
@pytest.mark.parametrize("count,log_stride", [(1, 0), (16, 4), (256, 0), (3, 6), (4, 6)])
def test_noise_free_packing_gives_the_phases_at_their_strides_within_the_rounding_bound(oracle, b, l, count, log_stride):
    """phase(out_g) = sum_i phase(c_{g,i}) X^(i stride) - e with |e| <= n_in 2^(s_p - 1) at the coefficients i stride and 0
    elsewhere, s_p = 64 - b l; e = 0 at s_p = 0.  (16, 4) and (256, 0) fill the ring: every rotation but the first wraps."""
    rng = np.random.default_rng(1600 + 100 * b + 10 * count + log_stride)
    mul = lambda a, x: oracle.tn_mul(N, a, np.ascontiguousarray(x))
    s = rng.integers(0, 2, N, dtype=np.uint64)
    s_in = rng.integers(0, 2, N_IN, dtype=np.uint64)
    key = PK.pksk(rng, mul, N, s_in, s, b, l, 0)
    assert key.shape == (N_IN, l, 2, N)
    groups = 3
    rows = rng.integers(0, 1 << 64, (groups, count, N_IN + 1), dtype=np.uint64, endpoint=False)
    out = PK.packing_key_switch(key, rows, b, l, count, log_stride)
    assert out.shape == (groups, 2, N)
    got = CB.tglwe_phase(mul, out, s)
    want = np.zeros((groups, N), dtype=np.uint64)
    at = np.arange(count) << log_stride
    want[:, at] = CB.tlwe_phase(rows, s_in)
    err = CB.centred(want - got).astype(object)
    sp = 64 - b * l
    bound = N_IN * (1 << (sp - 1)) if sp else 0
    assert np.all(np.abs(err) <= bound)
    off = np.ones(N, dtype=bool)
    off[at] = False
    assert not err[:, off].any()
    if sp:
        assert err.any()                                    # the bound is not vacuous: some word was rounded


def test_packing_restatement_is_the_definition_one_word_at_a_time():
    """the matrix form of the twin against X^(i stride) KS(c_i) built from R.rot and Python-integer digits"""
    import _gadget_numpy as G

    b, l, count, log_stride = 8, 4, 3, 6
    rng = np.random.default_rng(16)
    key = rng.integers(0, 1 << 64, (N_IN, l, 2, N), dtype=np.uint64, endpoint=False)
    rows = rng.integers(0, 1 << 64, (1, count, N_IN + 1), dtype=np.uint64, endpoint=False)
    got = PK.packing_key_switch(key, rows, b, l, count, log_stride)[0]
    want = np.zeros((2, N), dtype=np.uint64)
    for i in range(count):
        ks = np.zeros((2, N), dtype=np.uint64)
        ks[1, 0] = rows[0, i, N_IN]
        for j in range(N_IN):
            _, digits = G.decompose_exact(int(rows[0, i, j]), b, l)
            for d in range(l):
                ks -= np.uint64(digits[d] % (1 << 64)) * key[j, d]
        want += R.rot(ks, 2 * N - (i << log_stride))        # X^(i stride) = X^-(2N - i stride)
    assert np.array_equal(got, want)


def test_function_major_and_contiguous_layouts_agree():
    """ciphertext i of group g at row i groups + g (§15's output) or at row g count + i: the same groups, the same result"""
    b, l, count, log_stride, groups = 8, 4, 4, 6, 5
    rng = np.random.default_rng(17)
    key = rng.integers(0, 1 << 64, (N_IN, l, 2, N), dtype=np.uint64, endpoint=False)
    fm = rng.integers(0, 1 << 64, (count, groups, N_IN + 1), dtype=np.uint64, endpoint=False)
    contiguous = np.ascontiguousarray(fm.transpose(1, 0, 2))
    assert contiguous[2, 3].tobytes() == fm.reshape(-1, N_IN + 1)[3 * groups + 2].tobytes()
    a = PK.packing_key_switch(key, contiguous, b, l, count, log_stride)
    for g in range(groups):
        assert np.array_equal(a[g], PK.packing_key_switch(key, fm[:, g][None], b, l, count, log_stride)[0])


@pytest.mark.parametrize("t", range(1, 9))
def test_box_expansion_of_a_packed_table_is_the_test_vector(t):
    rng = np.random.default_rng(t)
    table = rng.integers(0, 1 << 64, 1 << t, dtype=np.uint64, endpoint=False)
    got = PK.box_expand(PK.pack_plain(table, N, 8 - t), t)
    assert np.array_equal(got, LN.expand(table, N))
    if t == 8:                                              # box = 1: the identity, on any row
        x = rng.integers(0, 1 << 64, (3, 2, N), dtype=np.uint64, endpoint=False)
        assert np.array_equal(PK.box_expand(x, t), x)


def test_box_expansion_is_the_product_with_the_box_polynomial(oracle):
    """X^-half (1 + X + .. + X^(box-1)) in, by the oracle's negacyclic product, on random rows"""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 1 << 64, (4, N), dtype=np.uint64, endpoint=False)
    for t in (1, 4, 7):
        box = N >> t
        p = np.zeros(N, dtype=np.uint64)
        p[:box] = 1
        want = R.rot(oracle.tn_mul(N, x, np.broadcast_to(p, x.shape).copy()), box // 2)
        assert np.array_equal(PK.box_expand(x, t), want)


@pytest.mark.parametrize("t", [2, 3])
def test_ideal_tree_lookup_returns_the_entry_for_every_pair(t):
    P = 1 << t
    rng = np.random.default_rng(40 + t)
    table2d = rng.integers(0, 1 << 64, (P, P), dtype=np.uint64, endpoint=False)
    x, y = np.repeat(np.arange(P), P), np.tile(np.arange(P), P)
    wobble = rng.integers(-(1 << (60 - t)), 1 << (60 - t), (2, P * P)).astype(np.uint64)      # well inside half a box
    xp = np.array([LN.encode(v, t) for v in x], dtype=np.uint64) + wobble[0]
    yp = np.array([LN.encode(v, t) for v in y], dtype=np.uint64) + wobble[1]
    assert np.array_equal(PK.ideal_tree_lookup(table2d, xp, yp, N), table2d[x, y])


def test_word_counts_follow_the_rules(pkg):
    L = pkg.load_library()
    assert L.fhe_tfhe_pksk_words(1024, 1, 630, 8, 4) == 630 * 4 * 2 * 1024          # 41 MB
    assert L.fhe_tfhe_pksk_words(256, 1, 8, 1, 64) == 8 * 64 * 2 * 256
    assert L.fhe_tfhe_pksk_words(4096, 1, 1, 32, 2) == 2 * 2 * 4096
    for shape in [(1024, 2, 630, 8, 4), (1024, 0, 630, 8, 4), (128, 1, 8, 8, 4), (8192, 1, 8, 8, 4), (1000, 1, 8, 8, 4), (1024, 1, 630, 33, 1),
                  (1024, 1, 630, 0, 4), (1024, 1, 630, 13, 5), (1024, 1, 630, 8, 0), (1024, 1, 0, 8, 4)]:
        assert L.fhe_tfhe_pksk_words(*shape) == 0, shape


def test_entry_points_validate_before_touching_the_gpu(pkg):
    L, B = pkg.load_library(), pkg.binding
    d, far = 16, 1 << 40                    # any non-NULL, 16-byte aligned fake device address: validation must fail first
    pk = L.fhe_tlwe_gadget_packing_key_switch_dev

    def call(n=1024, k=1, n_in=630, b=8, l=4, key=far, src=far + (1 << 30), gs=8 * 631, is_=631, count=8, ls=7, out=far + (1 << 32), groups=5):
        return pk(n, k, n_in, b, l, key, src, gs, is_, count, ls, out, groups, None)

    for kw in (dict(groups=0), dict(count=0), dict(count=9), dict(ls=11), dict(count=1, ls=11), dict(gs=630), dict(is_=630), dict(k=2), dict(n=128),
               dict(n=8192), dict(b=33, l=1), dict(b=13, l=5), dict(b=0), dict(l=0), dict(n_in=0), dict(groups=1 << 40),
               dict(gs=1 << 62), dict(is_=1 << 62), dict(out=far + 64), dict(out=far + (1 << 30) + 8 * 631 * 8 * 4),
               dict(out=far + (1 << 30) - 16), dict(out=24)):
        assert call(**kw) == B.FHE_E_INVALID, kw
        assert b"fhe_tlwe_gadget_packing_key_switch_dev" in L.fhe_last_error() or kw == dict(out=24)
    assert call(out=far + 64) == B.FHE_E_INVALID and b"overlap" in L.fhe_last_error()
    assert call(n=1000) == B.FHE_E_BAD_N
    for kw in (dict(key=None), dict(src=None), dict(out=None)):
        assert call(**kw) == B.FHE_E_NULL, kw
    # the function-major layout [count][groups][n_in + 1]: the extent is (groups - 1) gs + (count - 1) is + n_in + 1 words
    extent = (4 * 631 + 7 * 5 * 631 + 631) * 8
    assert call(gs=631, is_=5 * 631, out=far + (1 << 30) + extent - 16) == B.FHE_E_INVALID and b"overlap" in L.fhe_last_error()
    be = L.fhe_tglwe_box_expand_dev
    for args in ((1024, 1, 0, d, far, 1), (1024, 1, 11, d, far, 1), (1024, 2, 3, d, far, 1), (128, 1, 3, d, far, 1), (8192, 1, 3, d, far, 1),
                 (1024, 1, 3, far, far + 2 * 1024 * 8 - 16, 1), (1024, 1, 3, far, far, 1), (1024, 1, 3, far, 24, 1)):
        assert be(*args, None) == B.FHE_E_INVALID, args
    assert be(1000, 1, 3, d, far, 1, None) == B.FHE_E_BAD_N
    assert be(1024, 1, 3, None, far, 1, None) == B.FHE_E_NULL
    assert be(1024, 1, 3, None, None, 0, None) == B.FHE_OK
    br = L.fhe_tfhe_gadget_bootstrap_rows_dev
    ok = [1024, 1, 10, 3, 630, far, far + (1 << 36), 4, 4, far + (1 << 37), far + (1 << 38), far + (1 << 39), 3, None]
    for pos, v in [(1, 2), (0, 128), (0, 8192), (2, 33), (2, 11), (3, 0), (4, 0), (7, 33), (8, 0), (8, 17)]:
        args = list(ok)
        args[pos] = v
        assert br(*args) == B.FHE_E_INVALID, (pos, v)
        assert b"fhe_tfhe_gadget_bootstrap_rows_dev" in L.fhe_last_error()
    for pos in (5, 6, 9, 10, 11):
        args = list(ok)
        args[pos] = None
        assert br(*args) == B.FHE_E_NULL, pos
    for at in (far + 64, far + (1 << 36) + 3 * 2 * 1024 * 8 - 16, far + (1 << 37) + 64, far + (1 << 38) + 16):     # key, the tables' last row, KSK, input
        args = list(ok)
        args[11] = at
        assert br(*args) == B.FHE_E_INVALID and b"overlap" in L.fhe_last_error(), at
    args = list(ok)
    args[12] = 0
    assert br(*args) == B.FHE_OK


def test_header_and_binding_declare_the_new_entry_points(pkg):
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fhe_ntt.h")) as f:
        h = f.read()
    for name in ("fhe_tlwe_gadget_packing_key_switch_dev", "fhe_tglwe_box_expand_dev", "fhe_tfhe_gadget_bootstrap_rows_dev"):
        assert re.search(r"\bint\s+" + name + r"\(", h) and name in pkg.binding.EXPORTS
    assert re.search(r"\bsize_t\s+fhe_tfhe_pksk_words\(", h) and "fhe_tfhe_pksk_words" in pkg.binding.EXPORTS


def test_python_surface_refuses_bad_shapes(pkg):
    from fhe_study_amd import tfhe

    with pytest.raises(ValueError):
        tfhe.PackingKeySwitchKey(np.zeros((8, 4, 2), dtype=np.uint64), 8, 4)
    with pytest.raises(ValueError):
        tfhe.PackingKeySwitchKey(np.zeros((8, 3, 2, 256), dtype=np.uint64), 8, 4)
    with pytest.raises(ValueError):
        tfhe.tree_lookup(type("K", (), {"log_beta": None})(), None, 3, None, None, None)
    key = type("K", (), {"log_beta": 10, "n": 1024, "n_lwe": 630, "k": 1})()
    with pytest.raises(ValueError):
        tfhe.tree_lookup(key, None, 3, None, None, None, nu=1)                    # nu is 0 or t_bits
    with pytest.raises(ValueError):
        tfhe.tree_lookup(key, None, 5, None, None, None, nu=5)                    # t_bits <= min(L - t_bits, 4)
