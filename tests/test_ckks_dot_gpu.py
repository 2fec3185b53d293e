"""The CKKS inner product on the device (ckks_eval.hip): fhe_ckks_rns_dot_dev word for word against
tests/_ckks_dot_numpy.py (tolerance zero) on the case list tests/test_ckks_dot_cpu.py proved; a square, a repeated pointer,
operands at a higher level, q - 1 everywhere at 64 pairs, two chunks, a launch past the grid cap; the operands untouched; every
rejection with the output untouched; the launch counts beside those of one relinearisation; ckks.dot through ckks.RnsClientKey
word for word against the restatement and, beside mul and lincomb composed, within the CPU module's bound."""
import numpy as np
import pytest

import _ckks_dot_numpy as DN
import _ckks_eval_numpy as E
import _ckks_numpy as K
import _client_numpy as C
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0x5A5A5A5A5A5A5A5A


def _refused():
    return pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ")


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


def _plans(pkg, mods, n):
    return [pkg.Plan(q, n) for q in mods]


def _key(mods, P, n, rng):
    """a key-shaped array [k][k + 1][2][n] of canonical residues: the words of a key switch do not ask for more"""
    r = np.random.default_rng(rng)
    return np.stack([np.stack([r.integers(0, q, (2, n), dtype=np.uint64) for q in list(mods) + [P]]) for _ in mods])


def _dot(pkg, plans, sp, d_key, key_limbs, d_as, d_bs, w, batch, n):
    out = _empty((len(plans), 2, batch, n))
    pkg.binding.ckks_rns_dot_dev(plans, sp, d_key.data_ptr(), key_limbs, [x.data_ptr() for x in d_as], [x.data_ptr() for x in d_bs], DN.flat(w), out.data_ptr(), batch)
    return _u64(out)


def _pairs(pool, count):
    """`count` pairs over a pool of six ciphertexts: every ciphertext on both sides, squares among them (r = 0, 6, ..)"""
    return [(pool[r % 6], pool[(5 * r) % 6]) for r in range(count)]


# ---- the sweep, word for word -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch,spec", DN.WORD_CASES)
def test_dot_word_for_word(pkg, n, k, batch, spec):
    mods, P = E.case_chain(n, k, spec)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    key = _key(mods, P, n, 7 * n + k)
    d_key = _dev(key)
    pool = [E.case_ct(mods, n, batch, 2, 900 * n + 7 * k + r) for r in range(6)]
    d_pool = [_dev(x) for x in pool]
    for count, weighted in DN.sweep():
        w = DN.random_weights(mods, count, 31 * count + k) if weighted else None
        got = _dot(pkg, plans, sp, d_key, k, *zip(*_pairs(d_pool, count)), w, batch, n)
        assert np.array_equal(got, DN.dot(mods, P, key, _pairs(pool, count), w)), (count, weighted)
    for x, d in zip(pool, d_pool):                                           # the operands are only read
        assert np.array_equal(_u64(d), x)
    assert np.array_equal(_u64(d_key), key)


def test_a_square_a_repeated_pointer_and_operands_at_a_higher_level(pkg):
    n, batch = 16, 3
    mods, P = E.wide_chain(n)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    key = _key(mods, P, n, 41)                                               # the key of the whole chain serves every level
    d_key = _dev(key)
    full = [E.case_ct(mods, n, batch, 2, 60 + r) for r in range(3)]
    d_full = [_dev(x) for x in full]
    x, y, z = range(3)
    for k in (1, 3, 8):                                                      # operands of 8 limbs read at k: truncation costs nothing
        for order, weighted in (([(x, x)], False),                           # dot([x], [x]) is the square
                                ([(x, x)], True),
                                ([(x, y), (y, x), (x, y)], True),            # a pair twice, and mirrored
                                ([(x, y), (x, z), (x, x), (z, x)], False)):  # one pointer in every pair, on either side
            w = DN.random_weights(mods[:k], len(order), 70 + k) if weighted else None
            got = _dot(pkg, plans[:k], sp, d_key, 8, [d_full[a] for a, _ in order], [d_full[b] for _, b in order], w, batch, n)
            assert np.array_equal(got, DN.dot(mods[:k], P, key, [(full[a], full[b]) for a, b in order], w)), (k, order)
        sq = _dot(pkg, plans[:k], sp, d_key, 8, [d_full[x]], [d_full[x]], None, batch, n)
        out = _empty((k, 2, batch, n))                                       # ... and the square is mul's words
        short = _dev(full[x][:k])
        pkg.binding.ckks_rns_mul_dev(plans[:k], sp, d_key.data_ptr(), 8, short.data_ptr(), short.data_ptr(), out.data_ptr(), batch)
        assert np.array_equal(sq, _u64(out))
    for f, d in zip(full, d_full):
        assert np.array_equal(_u64(d), f)


def test_edge_residues_at_the_most_pairs(pkg):
    """every word and weight at q - 1 for 64 pairs: the fold rules' worst case on both kinds of limb"""
    n, batch = 16, 1
    mods, P = E.wide_chain(n)
    assert mods[0] >= 1 << 62
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    key = _key(mods, P, n, 43)
    edge = np.stack([np.full((2, batch, n), q - 1, dtype=U64) for q in mods])
    d_edge, d_key = _dev(edge), _dev(key)
    for w in ([[q - 1 for q in mods]] * DN.MAX_COUNT, None):
        got = _dot(pkg, plans, sp, d_key, 8, [d_edge] * DN.MAX_COUNT, [d_edge] * DN.MAX_COUNT, w, batch, n)
        assert np.array_equal(got, DN.dot(mods, P, key, [(edge, edge)] * DN.MAX_COUNT, w))


@pytest.mark.parametrize("n,k,batch,spec", [DN.TWO_CHUNKS, DN.PAST_THE_GRID])
def test_two_chunks_and_a_launch_past_the_grid_cap(pkg, n, k, batch, spec):
    mods, P = E.case_chain(n, k, spec)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    key = _key(mods, P, n, 45)
    a, b = E.case_ct(mods, n, batch, 2, 90), E.case_ct(mods, n, batch, 2, 91)
    w = DN.random_weights(mods, 2, 92)
    got = _dot(pkg, plans, sp, _dev(key), k, [_dev(a), _dev(b)], [_dev(b), _dev(b)], w, batch, n)
    assert np.array_equal(got, DN.dot(mods, P, key, [(a, b), (b, b)], w))


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_output_untouched(pkg):
    B = pkg.binding
    n, k, batch = 16, 3, 2
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    key = _key(mods, P, n, 47)
    a, d_key = _dev(E.case_ct(mods, n, batch, 2, 5)), _dev(key)
    out = _empty((k, 2, batch, n))
    A, KEY, O = a.data_ptr(), d_key.data_ptr(), out.data_ptr()
    ct_bytes = k * 2 * batch * n * 8
    one, f = [1] * k, B.ckks_rns_dot_dev
    bad = [
        (B.FHE_E_NULL, (None, sp, KEY, k, [A], [A], None, O, batch), dict(limbs=k)),
        (B.FHE_E_NULL, ([plans[0], None, plans[2]], sp, KEY, k, [A], [A], None, O, batch), {}),
        (B.FHE_E_NULL, (plans, None, KEY, k, [A], [A], None, O, batch), {}),
        (B.FHE_E_NULL, (plans, sp, None, k, [A], [A], None, O, batch), {}),
        (B.FHE_E_NULL, (plans, sp, KEY, k, None, [A], None, O, batch), dict(count=1)),
        (B.FHE_E_NULL, (plans, sp, KEY, k, [A], None, None, O, batch), {}),
        (B.FHE_E_NULL, (plans, sp, KEY, k, [A, None], [A, A], None, O, batch), {}),
        (B.FHE_E_NULL, (plans, sp, KEY, k, [A, A], [A, None], None, O, batch), {}),
        (B.FHE_E_PARAM_MISMATCH, ([plans[0], plans[1], other], sp, KEY, k, [A], [A], None, O, batch), {}),
        (B.FHE_E_PARAM_MISMATCH, (plans, other, KEY, k, [A], [A], None, O, batch), {}),
        (B.FHE_E_INVALID, ([plans[0], plans[1], plans[0]], sp, KEY, k, [A], [A], None, O, batch), {}),
        (B.FHE_E_INVALID, (plans, plans[0], KEY, k, [A], [A], None, O, batch), {}),
        (B.FHE_E_INVALID, (plans, sp, KEY, k - 1, [A], [A], None, O, batch), {}),
        (B.FHE_E_INVALID, (plans, sp, KEY, 9, [A], [A], None, O, batch), {}),
        (B.FHE_E_INVALID, (plans, sp, KEY, k, [], [], None, O, batch), {}),
        (B.FHE_E_INVALID, (plans, sp, KEY, k, [A] * 65, [A] * 65, None, O, batch), {}),
        (B.FHE_E_INVALID, (plans, sp, KEY, k, [A, A], [A, A], one + [1, mods[1], 1], O, batch), {}),
        (B.FHE_E_INVALID, (plans, sp, KEY, k, [A, O + ct_bytes - 8], [A, A], None, O, batch), {}),    # an operand at the output's last word
        (B.FHE_E_INVALID, (plans, sp, KEY, k, [A, A], [O - ct_bytes + 8, A], None, O, batch), {}),    # ... ending in its first
        (B.FHE_E_INVALID, (plans, sp, O + ct_bytes - 8, k, [A], [A], None, O, batch), {}),            # ... and the key
        (B.FHE_E_INVALID, (plans, sp, KEY, k, [A + 4], [A], None, O, batch), {}),
        (B.FHE_E_INVALID, (plans, sp, KEY, k, [A], [A + 4], None, O, batch), {}),
        (B.FHE_E_INVALID, (plans, sp, KEY, k, [A], [A], None, O, 1 << 60), {}),
    ]
    for code, args, kw in bad:
        with _refused() as e:
            f(*args, **kw)
        assert e.value.code == code, args
    with _refused() as e:
        f(plans, sp, KEY, k, [A], [A], None, None, batch)
    assert e.value.code == B.FHE_E_NULL
    f(plans, sp, KEY, k, [A], [A], one, O, 0)                                # batch = 0 writes nothing
    assert (_u64(out) == U64(FILL)).all()
    f(plans, sp, KEY, k, [A], [A], one, O, batch)                            # and the accepted call writes every word: the square
    assert np.array_equal(_u64(out), DN.dot(mods, P, key, [(_u64(a), _u64(a))], [one]))


# ---- the launch counts -------------------------------------------------------------------------------------------------------------------
def _timer_rows(B, fn):
    """{label: launches} of one call, the transforms' labels included; the tag (log2 n) is dropped"""
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


@pytest.mark.parametrize("n,k,batch", [(64, 1, 3), (64, 3, 3), DN.TWO_CHUNKS[:3]])
def test_launch_counts(pkg, n, k, batch):
    B = pkg.binding
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    a, d_key = _dev(E.case_ct(mods, n, batch, 2, 9)), _dev(_key(mods, P, n, 10))
    d3, out = _dev(E.case_ct(mods, n, batch, 3, 11)), _empty((k, 2, batch, n))
    chunks = -(-batch // E.chunk_rows(n, k, batch))
    assert chunks == (2 if n == 4096 else 1)
    relin = _timer_rows(B, lambda: B.ckks_rns_relinearize_dev(plans, sp, d_key.data_ptr(), k, d3.data_ptr(), out.data_ptr(), batch))
    assert relin["ckks_rns_lift"] == (k + 1) * chunks and relin["ckks_rns_keymac"] == (k + 1) * chunks and relin["ckks_rns_divround"] == k * chunks
    assert not any(lab.startswith("ckks_rns_tensor") for lab in relin)
    for count in (1, DN.GROUP, DN.GROUP + 1, 2 * DN.GROUP + 1) if n == 64 else (2,):
        for w in (None, [1] * (count * k)):
            got = _timer_rows(B, lambda: B.ckks_rns_dot_dev(plans, sp, d_key.data_ptr(), k, [a.data_ptr()] * count, [a.data_ptr()] * count, w, out.data_ptr(), batch))
            assert got == dict(relin, ckks_rns_tensorsum=DN.launch_counts(k, count) * chunks), (count, w is None)
            assert "ckks_rns_tensor" not in got
    # one mul shows its tensor kernel where the new call shows none, and is otherwise the same sequence
    got = _timer_rows(B, lambda: B.ckks_rns_mul_dev(plans, sp, d_key.data_ptr(), k, a.data_ptr(), a.data_ptr(), out.data_ptr(), batch))
    assert got == dict(relin, ckks_rns_tensor=k * chunks)


# ---- ckks.dot through the client key ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


@pytest.mark.parametrize("name", list(DN.FUNCTIONAL))
def test_dot_beside_mul_and_lincomb_composed(pkg, tab, name):
    case = DN.FUNCTIONAL[name]
    run = DN.functional_run(case, tab)
    ck = pkg.ckks
    n, count = case["n"], case["count"]
    param = ck.RnsParam(n, run["mods"], run["P"])
    key = ck.RnsClientKey.generate(DN.SEED, param, case["delta"])
    pk, rlk = key.public_key(0), key.relin_key(0)
    # the restatement's encodings are encrypted, in its order, so that every later word is equal
    cts = [tuple(key.encrypt(pk, K.encode(z, case["delta"])) for z in pair) for pair in run["zs"]]
    for (x, y), (rx, ry) in zip(cts, run["cts"]):
        assert np.array_equal(_u64(x.d), rx) and np.array_equal(_u64(y.d), ry)
    xs, ys = [x for x, _ in cts], [y for _, y in cts]
    coeffs, S_arg, S = DN.functional_target(case)
    res = ck.dot(xs, ys, rlk, case["coeffs"], scale=S_arg)
    assert (res.level, res.scale, res.batch) == (2, S, case["rows"])
    assert np.array_equal(_u64(res.d), DN.dot(run["mods"], run["P"], _u64(rlk.d_rlk), run["cts"], run["w"]))   # tolerance zero
    fused = res.rescale()
    assert fused.scale == run["scale"] and np.array_equal(_u64(fused.d), run["res"])
    # the composed form on the same inputs: a mul per pair, one lincomb.  Its words differ by design (count relinearisations)
    comp = ck.lincomb([x.mul(y, rlk) for x, y in zip(xs, ys)], coeffs, scale=S)[0].rescale()
    assert comp.scale == fused.scale and np.array_equal(_u64(comp.d), run["comp"]) and not np.array_equal(_u64(comp.d), _u64(fused.d))
    for label, ct, bound in (("fused", fused, run["raw_bounds"][0]), ("composed", comp, run["raw_bounds"][1])):
        d = key.decrypt(ct)
        err = float(np.abs(K.decode(d, ct.scale) - run["want"]).max())
        bound += float(K.e_dec(d, ct.scale).max())
        print(f"{name}: {label}: worst slot error {err:.3e}, derived bound {bound:.3e}")
        assert err <= bound
    assert np.abs(key.decrypt_and_decode(fused) - key.decrypt_and_decode(comp)).max() <= run["bound"] + run["bound_composed"]


def test_python_surface(pkg):
    ck = pkg.ckks
    n = 16
    mods, P = E.chain(n, 58, 40, 2)
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(DN.SEED, param, 2.0 ** 40)
    pk, rlk = key.public_key(0), key.relin_key(0)
    z = np.random.default_rng(5).uniform(-1, 1, (2, n // 2)).astype(np.complex128)
    x, y = key.encode_and_encrypt(pk, z), key.encode_and_encrypt(pk, 0.5 * z)
    xw, yw, kw = _u64(x.d), _u64(y.d), _u64(rlk.d_rlk)
    sq = ck.dot([x], [x], rlk)                                               # the square, mul's words
    assert (sq.level, sq.scale) == (2, x.scale * x.scale) and np.array_equal(_u64(sq.d), _u64(x.mul(x, rlk).d))
    low = ck.dot([x, y], [y.at_level(1), x], rlk, [2, -1])                   # the level is the lowest operand's; x is read as it is
    assert (low.level, low.scale) == (1, x.scale * y.scale)
    w, _ = DN.weights([2, -1], low.scale, [low.scale] * 2, mods[:2])
    assert np.array_equal(_u64(low.d), DN.dot(mods[:2], P, kw, [(xw, yw), (yw, xw)], w))
    lower = ck.dot([x], [y], rlk, level=0)
    assert lower.level == 0 and np.array_equal(_u64(lower.d), DN.dot(mods[:1], P, kw, [(xw, yw)]))
    # pairs of unequal scales: the weights bring them to the target, here the larger pair scale
    h = x.mul_const(1, scale=8 * x.scale)                                    # x at eight times its scale
    mixed = ck.dot([x, h], [y, x], rlk)
    s = [x.scale * y.scale, h.scale * x.scale]
    assert mixed.level == 2 and mixed.scale == max(s) == 8 * s[0]
    w, big = DN.weights([1, 1], max(s), s, mods)
    assert big == [8, 1]
    assert np.array_equal(_u64(mixed.d), DN.dot(mods, P, kw, [(xw, yw), (_u64(h.d), xw)], w))
    # 1.5 z^2 within 1e-6: a fresh slot is off by at most n (fresh_noise + 1/2) / Delta = 1.4e-8, a product of two by twice that
    # times |z| <= sqrt 2, two pairs by 8e-8; the relinearisation and the rescale are below 1e-9 at these scales
    assert np.abs(key.decrypt_and_decode(mixed.rescale()) - 1.5 * z * z).max() < 1e-6
    with _refused() as e:                                                    # a key of another chain, as in mul
        ck.dot([x], [y], ck.RnsRelinKey(ck.RnsParam(n, mods[:2], P), rlk.d_rlk))
    assert e.value.code == pkg.binding.FHE_E_PARAM_MISMATCH
    with _refused() as e:
        ck.dot([x], [ck.RnsCiphertext(ck.RnsParam(n, mods[:2], P), x.d, 1, 1.0)], rlk)
    assert e.value.code == pkg.binding.FHE_E_PARAM_MISMATCH
    with pytest.raises(ValueError, match="constant polynomial"):
        ck.dot([x], [y], rlk, [1j])
    for bad in (dict(coeffs=[1.0, 2.0]), dict(coeffs=[float("nan")]), dict(level=3), dict(scale=-1.0)):
        with pytest.raises(ValueError):
            ck.dot([x], [y], rlk, **bad)
    with pytest.raises(ValueError):
        ck.dot([], [], rlk)
    with pytest.raises(ValueError):
        ck.dot([x, x], [y], rlk)
