"""The CKKS evaluator on an RNS chain on the device (ckks_eval.hip): every entry point word for word against
tests/_ckks_eval_numpy.py (tolerance zero) on the case lists tests/test_ckks_eval_cpu.py proved, the residues at the edges,
rescaling down to level 0, the Python surface, the functional tests through ckks.RnsClientKey with check 3's bound, every
rejection with its outputs untouched, and the launch counts of §22."""
import numpy as np
import pytest

import _ckks_eval_numpy as E
import _ckks_numpy as K
import _client_numpy as C
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
FILL = 0x5A5A5A5A5A5A5A5A
SEED = bytes((5 * i + 9) % 256 for i in range(32))


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _plans(pkg, mods, n):
    return [pkg.Plan(q, n) for q in mods]


def _tensor(pkg, plans, a, b):
    k, _, batch, n = a.shape
    out, da, db = _empty((k, 3, batch, n)), _dev(a), _dev(b)
    pkg.binding.ckks_rns_tensor_dev(plans, da.data_ptr(), db.data_ptr(), out.data_ptr(), batch)
    return _u64(out)


def _relin(pkg, plans, sp, d_rlk, kl, d):
    k, _, batch, n = d.shape
    out, dd = _empty((k, 2, batch, n)), _dev(d)
    pkg.binding.ckks_rns_relinearize_dev(plans, sp, d_rlk.data_ptr(), kl, dd.data_ptr(), out.data_ptr(), batch)
    return _u64(out)


def _mul(pkg, plans, sp, d_rlk, kl, a, b):
    out, da, db = _empty(a.shape), _dev(a), _dev(b)
    pkg.binding.ckks_rns_mul_dev(plans, sp, d_rlk.data_ptr(), kl, da.data_ptr(), db.data_ptr(), out.data_ptr(), a.shape[2])
    return _u64(out)


def _rescale(pkg, plans, c):
    k, _, batch, n = c.shape
    out, dc = _empty((k - 1, 2, batch, n)), _dev(c)
    pkg.binding.ckks_rns_rescale_dev(plans, dc.data_ptr(), out.data_ptr(), batch)
    return _u64(out)


def _device_key(pkg, tab, mods, P, n, row):
    """the secret per limb and the relinearisation key, both made on the device -> (s signed, d_rlk)"""
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    d_s = _empty((len(mods) + 1, n))
    for i, p in enumerate(plans + [sp]):
        pkg.binding.ckks_secret_key_dev(p, SEED, 0, d_s[i].data_ptr())
    d_rlk, d_tab = _empty((len(mods), len(mods) + 1, 2, n)), _dev(tab)
    pkg.binding.ckks_rns_relin_key_dev(plans, sp, SEED, row, d_s.data_ptr(), d_tab.data_ptr(), len(tab), d_rlk.data_ptr())
    s = K.secret_key(SEED, 0, n)
    for i, q in enumerate(list(mods) + [P]):
        assert np.array_equal(_u64(d_s[i]), E.residues(s, q))
    return s, d_rlk


# ---- every entry point, word for word ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch,spec", E.WORD_CASES)
def test_entry_points_word_for_word(pkg, tab, n, k, batch, spec):
    mods, P = E.case_chain(n, k, spec)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    s, d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 3)
    rlk = E.relin_key(SEED, E.RLK_BASE + 64 * 3, s, mods, P, tab)
    assert np.array_equal(_u64(d_rlk), rlk)
    a, b = E.case_ct(mods, n, batch, 2, 100 * n + k), E.case_ct(mods, n, batch, 2, 100 * n + k + 50)
    d = _tensor(pkg, plans, a, b)
    assert np.array_equal(d, E.tensor(mods, a, b))
    c = _relin(pkg, plans, sp, d_rlk, k, d)
    assert np.array_equal(c, E.relinearize(mods, P, rlk, d))
    assert np.array_equal(_mul(pkg, plans, sp, d_rlk, k, a, b), c)
    if k > 1:
        assert np.array_equal(_rescale(pkg, plans, c), E.rescale(mods, c))
        # the key of the whole chain serves a lower level: digits j < k - 1, columns {0 .. k - 2, P}
        low = _relin(pkg, plans[:-1], sp, d_rlk, k, d[:-1])
        assert np.array_equal(low, E.relinearize(mods[:-1], P, rlk, d[:-1]))
    m = np.random.default_rng(n + k).integers(-(1 << 63), (1 << 63) - 1, (batch, n), dtype=np.int64, endpoint=True)
    m[0, :2] = [-(1 << 63), (1 << 63) - 1]
    out, dm = _empty((k, batch, n)), _dev(m.view(U64))
    pkg.binding.ckks_rns_from_i64_dev(plans, dm.data_ptr(), out.data_ptr(), batch)
    assert np.array_equal(_u64(out), E.from_i64(mods, n, m))


# ---- residues at the edges ----------------------------------------------------------------------------------------------------------
def test_edge_residues_and_the_centring(pkg, tab):
    n, k = 16, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    s, d_rlk = _device_key(pkg, tab, mods, P, n, E.RLK_BASE + 64 * 4)
    rlk = E.relin_key(SEED, E.RLK_BASE + 64 * 4, s, mods, P, tab)
    mono = np.zeros(n, dtype=U64)
    mono[n - 1] = 1
    # rows: all q - 1 (as evals), zero, the monomial X^(n-1), coefficients at floor(q / 2) and floor(q / 2) + 1 alternating
    def rows(q, comps):
        half = np.array([q // 2, q // 2 + 1] * (n // 2), dtype=U64)
        r = np.stack([np.full(n, q - 1, dtype=U64), np.zeros(n, dtype=U64), E.fwd(q, n, mono), E.fwd(q, n, half), E.fwd(q, n, half[::-1].copy())])
        return np.stack([r] * comps)
    a = np.stack([rows(q, 2) for q in mods])
    d = _tensor(pkg, plans, a, a[:, :, ::-1].copy())
    assert np.array_equal(d, E.tensor(mods, a, a[:, :, ::-1]))
    d3 = np.stack([rows(q, 3) for q in mods])                           # d2's coefficients sit exactly at the centring's edge in every limb
    assert np.array_equal(_relin(pkg, plans, sp, d_rlk, k, d3), E.relinearize(mods, P, rlk, d3))
    assert np.array_equal(_relin(pkg, plans, sp, d_rlk, k, d), E.relinearize(mods, P, rlk, d))
    assert np.array_equal(_rescale(pkg, plans, a), E.rescale(mods, a))   # the top limb's coefficients at the edge


def test_rescale_down_to_level_zero_then_refused(pkg):
    n, k = 16, 3
    mods, _ = E.chain(n, 58, 40, k - 1)
    plans = _plans(pkg, mods, n)
    c = E.case_ct(mods, n, 3, 2, 77)
    for lv in (3, 2):
        got = _rescale(pkg, plans[:lv], c)
        assert np.array_equal(got, E.rescale(mods[:lv], c))
        c = got
    out = _empty((1, 2, 3, n))
    with pytest.raises(pkg.FheError) as e:
        dc = _dev(c)
        pkg.binding.ckks_rns_rescale_dev(plans[:1], dc.data_ptr(), out.data_ptr(), 3)
    assert e.value.code == pkg.binding.FHE_E_INVALID and (_u64(out) == U64(FILL)).all()


# ---- the Python surface and the functional tests -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tab):
    return {name: E.functional_run(case, tab) for name, case in E.FUNCTIONAL_GPU.items()}


@pytest.mark.parametrize("name", list(E.FUNCTIONAL_GPU))
def test_product_then_square_through_the_client_key(pkg, runs, name):
    case, r = E.FUNCTIONAL_GPU[name], runs[name]
    ck = pkg.ckks
    param = ck.RnsParam(case["n"], r["mods"], r["P"])
    key = ck.RnsClientKey.generate(case["seed"], param, r["delta"])
    pk, rlk = key.public_key(0), key.relin_key(0)
    assert np.array_equal(_u64(pk.d_evals), r["pk"]) and np.array_equal(_u64(rlk.d_rlk), r["rlk"])
    with pytest.raises(ValueError):
        key.relin_key(0)
    # the restatement's encodings are encrypted, so that every later word is equal: at Delta = 2^40 the encoder's f64 error
    # E_enc passes 1/8, and the device may round a coefficient the other way
    ct1, ct2 = key.encrypt(pk, r["m1"]), key.encrypt(pk, r["m2"])
    assert np.array_equal(_u64(ct1.d), r["ct1"]) and np.array_equal(_u64(ct2.d), r["ct2"])
    prod = ct1.mul(ct2, rlk).rescale()
    sq = prod.mul(prod, rlk).rescale()
    assert (prod.level, sq.level) == (1, 0) and prod.scale == r["s1"] and sq.scale == r["s2"]
    assert np.array_equal(_u64(prod.d), r["prod"]) and np.array_equal(_u64(sq.d), r["sq"])
    assert np.array_equal(key.decrypt(prod), r["d1"]) and np.array_equal(key.decrypt(sq), r["d2"])
    want = r["z1"] * r["z2"]
    for i, (ct, z) in enumerate(((prod, want), (sq, want ** 2))):
        got = key.decrypt_and_decode(ct)
        err, bound = float(np.abs(got - z).max()), r["bounds"][i] + r["edec"][i]
        print(f"{name}: stage {i + 1} worst slot error {err:.3e}, derived bound {bound:.3e}")
        assert err <= bound and err < 0.5
        assert np.array_equal(np.round(got.real), z.real) and np.array_equal(np.round(got.imag), z.imag)
    with pytest.raises(pkg.FheError):
        sq.rescale()
    fresh = key.encode_and_encrypt(pk, r["z1"])                          # the device's own encoder in front of the same path
    assert fresh.level == 2 and np.abs(key.decrypt_and_decode(fresh) - r["z1"]).max() < 1e-6


def test_levels_additions_and_plain_operands(pkg, runs):
    case, r = E.FUNCTIONAL_GPU["n32"], runs["n32"]
    ck = pkg.ckks
    n, mods = case["n"], r["mods"]
    param = ck.RnsParam(n, mods, r["P"])
    a = ck.RnsCiphertext(param, _dev(r["ct1"]), 2, r["delta"])
    b = ck.RnsCiphertext(param, _dev(r["ct2"]), 2, r["delta"])
    low = b.at_level(1)
    assert low.level == 1 and np.array_equal(_u64(low.d), r["ct2"][:2])
    for got, fn in ((a + low, E.padd), (a - low, E.psub), (low + a, E.padd)):
        assert got.level == 1 and got.scale == r["delta"]
        want = np.stack([fn(q, r["ct1"][i], r["ct2"][i]) for i, q in enumerate(mods[:2])])
        assert np.array_equal(_u64(got.d), want)
    with pytest.raises(ValueError):
        a + ck.RnsCiphertext(param, b.d, 2, r["delta"] * (1 + 2.0 ** -19))
    assert (a + ck.RnsCiphertext(param, b.d, 2, r["delta"] * (1 + 2.0 ** -21))).scale == r["delta"]
    with pytest.raises(ValueError):
        a.at_level(3)
    m3 = K.encode(E.functional_slots(case, 3), r["delta"])
    assert np.array_equal(_u64(a.add_plain(m3).d), E.add_plain(mods, n, r["ct1"], m3))
    mp = a.mul_plain(m3, r["delta"])
    assert mp.scale == r["delta"] ** 2 and np.array_equal(_u64(mp.d), E.mul_plain(mods, n, r["ct1"], m3))


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_outputs_untouched(pkg, tab):
    B = pkg.binding
    n, k = 16, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    a = _dev(E.case_ct(mods, n, 2, 2, 5))
    d = _dev(E.case_ct(mods, n, 2, 3, 6))
    rlk, cdt = _dev(E.case_ct(mods, n, 4, 2, 7)), _dev(tab)
    o2, o3, ok = _empty((k, 2, 2, n)), _empty((k, 3, 2, n)), _empty((k, k + 1, 2, n))
    s = _empty((k + 1, n), 0)
    A, D, R, O2, O3, OK, S = (x.data_ptr() for x in (a, d, rlk, o2, o3, ok, s))
    bad = [
        (B.FHE_E_INVALID, B.ckks_rns_tensor_dev, ([plans[0], plans[1], plans[0]], A, A, O3, 2)),
        (B.FHE_E_PARAM_MISMATCH, B.ckks_rns_tensor_dev, ([plans[0], plans[1], other], A, A, O3, 2)),
        (B.FHE_E_NULL, B.ckks_rns_tensor_dev, (plans, A, None, O3, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_tensor_dev, (plans, O3 + 8 * n, A, O3, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_relinearize_dev, (plans, plans[0], R, k, D, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_relinearize_dev, (plans, pkg.Plan(65537, n), R, k, D, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_relinearize_dev, (plans, sp, R, k - 1, D, O2, 2)),
        (B.FHE_E_NULL, B.ckks_rns_relinearize_dev, (plans, None, R, k, D, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_relinearize_dev, (plans, sp, O2, k, D, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_mul_dev, (plans, sp, R, 9, A, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_mul_dev, (plans, sp, R, k, O2, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_rescale_dev, (plans[:1], A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_rescale_dev, (plans, O2, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_from_i64_dev, (plans, O3, O3, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_relin_key_dev, (plans, sp, SEED, (1 << 63) - 2, S, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_INVALID, B.ckks_rns_relin_key_dev, (plans, sp, SEED, 0, S, cdt.data_ptr(), 1025, OK)),
        (B.FHE_E_INVALID, B.ckks_rns_relin_key_dev, (plans, sp, SEED, 0, OK, cdt.data_ptr(), len(tab), OK)),
    ]
    for code, fn, args in bad:
        with pytest.raises(pkg.FheError) as e:
            fn(*args)
        assert e.value.code == code, (fn.__name__, args)
    bad_tab = _dev(np.array([5, 5, 9], dtype=U64))
    with pytest.raises(pkg.FheError):
        B.ckks_rns_relin_key_dev(plans, sp, SEED, 0, S, bad_tab.data_ptr(), 3, OK)
    for out in (o2, o3, ok):
        assert (_u64(out) == U64(FILL)).all()
    B.ckks_rns_mul_dev(plans, sp, R, k, A, A, O2, 0)
    assert (_u64(o2) == U64(FILL)).all()


# ---- the launch counts of §22 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_launch_counts(pkg, tab, k):
    import torch

    B = pkg.binding
    n = 64
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    a = _dev(E.case_ct(mods, n, 3, 2, 9))
    rlk = _dev(np.random.default_rng(10).integers(0, 1 << 39, (k, k + 1, 2, n), dtype=np.uint64))
    out, low = _empty((k, 2, 3, n)), _empty((max(k - 1, 1), 2, 3, n))

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
        return {lab: sum(c for name, (_, c) in got.items() if name.startswith("ckks_rns_" + lab)) for lab in ("tensor", "lift", "keymac", "divround")}

    got = counts(lambda: B.ckks_rns_mul_dev(plans, sp, rlk.data_ptr(), k, a.data_ptr(), a.data_ptr(), out.data_ptr(), 3))
    assert got == dict(tensor=k, lift=k + 1, keymac=k + 1, divround=k)
    if k > 1:
        got = counts(lambda: B.ckks_rns_rescale_dev(plans, a.data_ptr(), low.data_ptr(), 3))
        assert got == dict(tensor=0, lift=1, keymac=0, divround=k - 1)
