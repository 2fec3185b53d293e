"""Slot rotations and conjugation of the CKKS evaluator on the device (ckks_eval.hip): the bare automorphism, the
Galois key, its application at the key's level and one below, and the hoisted call, word for word against
tests/_ckks_galois_numpy.py (tolerance zero) on the case list tests/test_ckks_galois_cpu.py proved; the launch counts; the
Python surface; the functional case through ckks.RnsClientKey with its bound; every rejection with its outputs untouched."""
import numpy as np
import pytest

import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_numpy as K
import _client_numpy as C
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
FILL = 0x5A5A5A5A5A5A5A5A
SEED = G.SEED


def _refused():
    """an FheError, whichever name the package was imported under when it was raised"""
    return pytest.raises(RuntimeError, match="^fhe_ntt error -?[0-9]+: ")


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


def _plans(pkg, mods, n):
    return [pkg.Plan(q, n) for q in mods]


def _secret(pkg, plans_and_special, n):
    d_s = _empty((len(plans_and_special), n))
    for i, p in enumerate(plans_and_special):
        pkg.binding.ckks_secret_key_dev(p, SEED, 0, d_s[i].data_ptr())
    return d_s


def _key(pkg, tab, plans, sp, d_s, d_tab, n, row, g):
    d_gk = _empty((len(plans), len(plans) + 1, 2, n))
    pkg.binding.ckks_rns_galois_key_dev(plans, sp, SEED, row, g, d_s.data_ptr(), d_tab.data_ptr(), len(tab), d_gk.data_ptr())
    return d_gk


def _apply(pkg, plans, sp, d_gks, gs, kl, d_ct):
    k, _, batch, n = d_ct.shape
    out = _empty((len(gs), k, 2, batch, n))
    pkg.binding.ckks_rns_galois_dev(plans, sp, [x.data_ptr() for x in d_gks], gs, kl, d_ct.data_ptr(), out.data_ptr(), batch)
    return _u64(out)


# ---- every entry point, word for word ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch,spec", G.WORD_CASES)
def test_entry_points_word_for_word(pkg, tab, n, k, batch, spec):
    mods, P = E.case_chain(n, k, spec)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    d_s, d_tab = _secret(pkg, plans + [sp], n), _dev(tab)
    s = K.secret_key(SEED, 0, n)
    ct = E.case_ct(mods, n, batch, 2, 300 * n + k)
    d_ct = _dev(ct)
    for t, g in enumerate(G.case_elements(n)):
        # the bare automorphism, a limb's slab of 2 batch rows a call
        d_p = _empty(ct.shape)
        for i, p in enumerate(plans):
            pkg.binding.ckks_galois_evals_dev(p, g, d_ct[i].data_ptr(), d_p[i].data_ptr(), 2 * batch)
        assert np.array_equal(_u64(d_p), G.galois_evals(ct, g)), g
        row = G.GK_BASE + 64 * (5 + t)
        d_gk = _key(pkg, tab, plans, sp, d_s, d_tab, n, row, g)
        gk = G.galois_key(SEED, row, s, mods, P, tab, g)
        assert np.array_equal(_u64(d_gk), gk), g
        assert np.array_equal(_apply(pkg, plans, sp, [d_gk], [g], k, d_ct)[0], G.apply_galois(mods, P, gk, ct, g)), g
        if k > 1:                                                            # the key of the whole chain serves the level below
            low = _apply(pkg, plans[:-1], sp, [d_gk], [g], k, _dev(ct[:-1]))[0]
            assert np.array_equal(low, G.apply_galois(mods[:-1], P, gk, ct[:-1], g)), g


@pytest.mark.parametrize("n,k,batch", [(2, 1, 1), (16, 3, 3), (64, 2, 3), (16, 8, 3)])
def test_hoisted_call_equals_separate_calls(pkg, tab, n, k, batch):
    mods, P = E.case_chain(n, k, "wide" if k == 8 else (58, 40))
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    d_s, d_tab = _secret(pkg, plans + [sp], n), _dev(tab)
    gs = [5 % (2 * n), 25 % (2 * n), 2 * n - 1]
    d_gks = [_key(pkg, tab, plans, sp, d_s, d_tab, n, G.GK_BASE + 64 * (20 + t), g) for t, g in enumerate(gs)]
    ct = E.case_ct(mods, n, batch, 2, 17 * n + k)
    d_ct = _dev(ct)
    many = _apply(pkg, plans, sp, d_gks, gs, k, d_ct)
    s = K.secret_key(SEED, 0, n)
    for t, g in enumerate(gs):
        assert np.array_equal(many[t], _apply(pkg, plans, sp, [d_gks[t]], [g], k, d_ct)[0]), g
        gk = G.galois_key(SEED, G.GK_BASE + 64 * (20 + t), s, mods, P, tab, g)
        assert np.array_equal(many[t], G.apply_galois(mods, P, gk, ct, g)), g
    assert np.array_equal(_u64(d_ct), ct)                                    # the input is only read


def test_edge_residues_and_the_centring(pkg, tab):
    n, k, g = 16, 3, 5
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    d_s, d_tab = _secret(pkg, plans + [sp], n), _dev(tab)
    d_gk = _key(pkg, tab, plans, sp, d_s, d_tab, n, G.GK_BASE + 64 * 30, g)
    gk = G.galois_key(SEED, G.GK_BASE + 64 * 30, K.secret_key(SEED, 0, n), mods, P, tab, g)
    mono = np.zeros(n, dtype=U64)
    mono[n - 1] = 1

    def rows(q):
        half = np.array([q // 2, q // 2 + 1] * (n // 2), dtype=U64)
        r = np.stack([np.full(n, q - 1, dtype=U64), np.zeros(n, dtype=U64), E.fwd(q, n, mono), E.fwd(q, n, half), E.fwd(q, n, half[::-1].copy())])
        return np.stack([r, r])
    ct = np.stack([rows(q) for q in mods])                                   # c1's coefficients sit at the centring's edge in every limb
    assert np.array_equal(_apply(pkg, plans, sp, [d_gk], [g], k, _dev(ct))[0], G.apply_galois(mods, P, gk, ct, g))


# ---- the launch counts of §23 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_launch_counts(pkg, tab, k):
    import torch

    B = pkg.binding
    n = 64
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    a = _dev(E.case_ct(mods, n, 3, 2, 9))
    keys = [_dev(np.random.default_rng(10 + r).integers(0, 1 << 39, (k, k + 1, 2, n), dtype=np.uint64)) for r in range(3)]
    gs = [5, 25, 2 * n - 1]
    out = _empty((3, k, 2, 3, n))

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
        return {lab: sum(c for name, (_, c) in got.items() if name.startswith("ckks_rns_" + lab)) for lab in ("tensor", "lift", "keymac", "divround", "galois")}

    for R in (1, 3):
        got = counts(lambda: B.ckks_rns_galois_dev(plans, sp, [x.data_ptr() for x in keys[:R]], gs[:R], k, a.data_ptr(), out.data_ptr(), 3))
        assert got == dict(tensor=0, lift=k + R, keymac=R * (k + 1), divround=R * k, galois=0), (k, R)
    got = counts(lambda: B.ckks_rns_mul_dev(plans, sp, keys[0].data_ptr(), k, a.data_ptr(), a.data_ptr(), out[0].data_ptr(), 3))
    assert got == dict(tensor=k, lift=k + 1, keymac=k + 1, divround=k, galois=0)       # §22's counts are as they were
    got = counts(lambda: B.ckks_galois_evals_dev(plans[0], 5, a[0].data_ptr(), out[0, 0].data_ptr(), 6))
    assert got == dict(tensor=0, lift=0, keymac=0, divround=0, galois=1)


# ---- the Python surface and the functional case ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tab):
    return {name: G.functional_run(case, tab) for name, case in G.FUNCTIONAL.items()}


@pytest.mark.parametrize("name", list(G.FUNCTIONAL))
def test_slot_sums_through_the_client_key_word_for_word(pkg, runs, name):
    case, r = G.FUNCTIONAL[name], runs[name]
    ck = pkg.ckks
    n = case["n"]
    param = ck.RnsParam(n, r["mods"], r["P"])
    key = ck.RnsClientKey.generate(case["seed"], param, r["delta"])
    pk = key.public_key(0)
    acc = key.encrypt(pk, r["m"])
    assert np.array_equal(_u64(acc.d), r["ct"])
    for t, g in enumerate(r["gs"]):
        last = t == len(r["gs"]) - 1
        gk = key.conjugation_key(t) if last else key.rotation_key(1 << t, t)
        assert gk.g == g and np.array_equal(_u64(gk.d_gk), r["gks"][t])
        acc = acc + (acc.conjugate(gk) if last else acc.rotate(gk))
        assert acc.level == 2 and acc.scale == r["delta"] and np.array_equal(_u64(acc.d), r["accs"][t])
    with pytest.raises(ValueError):
        key.rotation_key(1, 0)                                               # the slot is taken
    assert np.array_equal(key.decrypt(acc), r["d"])
    got = key.decrypt_and_decode(acc)
    err, bound = float(np.abs(got - r["want"]).max()), r["bound"] + r["edec"]
    print(f"{name}: worst slot error {err:.3e}, derived bound {bound:.3e}")
    assert err <= bound and err < 0.5 and np.array_equal(np.round(got.real), r["want"].real)


def test_slot_sums_at_4096(pkg, tab):
    """the first rotation word for word with the restatement, the rest against the expected sums and the bound"""
    case = G.FUNCTIONAL_GPU["n4096"]
    r = G.functional_setup(case, tab)
    ck = pkg.ckks
    n = case["n"]
    assert r["delta"] == 2.0 ** 40
    param = ck.RnsParam(n, r["mods"], r["P"])
    key = ck.RnsClientKey.generate(case["seed"], param, r["delta"])
    acc = key.encrypt(key.public_key(0), r["m"])
    assert np.array_equal(_u64(acc.d), r["ct"])
    for t, g in enumerate(r["gs"]):
        last = t == len(r["gs"]) - 1
        gk = key.conjugation_key(t) if last else key.rotation_key(1 << t, t)
        rot = acc.conjugate(gk) if last else acc.rotate(gk)
        if t == 0:
            want_gk = G.galois_key(case["seed"], G.GK_BASE, r["s"], r["mods"], r["P"], tab, g)
            assert np.array_equal(_u64(gk.d_gk), want_gk)
            assert np.array_equal(_u64(rot.d), G.apply_galois(r["mods"], r["P"], want_gk, r["ct"], g))
            w = ck.to_rotation_order(key.decrypt_and_decode(rot))
            assert np.abs(w - np.roll(G.to_rotation_order(r["z"]), -1, axis=-1)).max() < 1e-3
        acc = acc + rot
    d = key.decrypt(acc)
    got = key.decrypt_and_decode(acc)
    err, bound = float(np.abs(got - r["want"]).max()), r["bound"] + float(K.e_dec(d, r["delta"]).max())
    print(f"n4096: worst slot error {err:.3e}, derived bound {bound:.3e}")
    # the worst-case bound passes 1/2 here, as §22's second stage does: it charges every coefficient its maximum
    assert err <= bound and err < 0.5 and np.array_equal(np.round(got.real), r["want"].real)


def test_python_surface(pkg, runs):
    case, r = G.FUNCTIONAL["n32"], runs["n32"]
    ck = pkg.ckks
    n, mods, P = case["n"], r["mods"], r["P"]
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(case["seed"], param, r["delta"])
    ct = ck.RnsCiphertext(param, _dev(r["ct"]), 2, r["delta"])
    steps = [1, 3, n // 2 - 1]
    rks = [key.rotation_key(st, 10 + i) for i, st in enumerate(steps)]
    cj = key.conjugation_key(20)
    g3 = key.galois_key(3, 21)
    assert [k.g for k in rks] == [G.galois_element(n, st) for st in steps] and cj.g == 2 * n - 1
    for bad in (0, 2, 2 * n):
        with pytest.raises(ValueError):
            key.galois_key(bad, 22)
    with pytest.raises(ValueError):
        key.conjugation_key(20)
    with pytest.raises(ValueError):
        key.galois_key(5, 1 << 16)
    with pytest.raises(ValueError):
        ct.rotate(cj)
    with pytest.raises(ValueError):
        ct.rotate(g3)
    with pytest.raises(ValueError):
        ct.conjugate(rks[0])
    many = ct.rotate_many(rks + [cj, g3])
    assert len(many) == 5 and all(m.level == 2 and m.scale == r["delta"] and m.batch == ct.batch for m in many)
    want_gk = {}
    for gk, slot in zip(rks + [cj, g3], (10, 11, 12, 20, 21)):
        want_gk[gk.g] = G.galois_key(case["seed"], G.GK_BASE + 64 * slot, r["s"], mods, P, C.cdt_table(3.2), gk.g)
        assert np.array_equal(_u64(gk.d_gk), want_gk[gk.g])
    for m, gk in zip(many, rks + [cj, g3]):
        assert np.array_equal(_u64(m.d), G.apply_galois(mods, P, want_gk[gk.g], r["ct"], gk.g))
    assert np.array_equal(_u64(ct.rotate(rks[1]).d), _u64(many[1].d)) and np.array_equal(_u64(ct.conjugate(cj).d), _u64(many[3].d))
    assert np.array_equal(_u64(ct.apply_galois(g3).d), _u64(many[4].d))
    # the slots: a rotation rolls the rotation order, the conjugation conjugates; a key of the chain serves level 1
    w = ck.to_rotation_order(r["z"])
    for m, st in zip(many, steps):
        got = ck.to_rotation_order(key.decrypt_and_decode(m))
        assert np.abs(got - np.roll(w, -st, axis=-1)).max() < 1e-6
    assert np.abs(key.decrypt_and_decode(many[3]) - np.conj(r["z"])).max() < 1e-6
    low = ct.at_level(1).rotate(rks[0])
    assert low.level == 1 and np.array_equal(_u64(low.d), G.apply_galois(mods[:2], P, want_gk[rks[0].g], r["ct"][:2], rks[0].g))
    assert ct.rotate_many([]) == []
    other = ck.RnsParam(n, mods[:2], P)
    with _refused():
        ct.rotate(ck.RnsGaloisKey(other, 5, rks[0].d_gk))


# ---- rejections ------------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_outputs_untouched(pkg, tab):
    B = pkg.binding
    n, k = 16, 3
    mods, P = E.chain(n, 58, 40, k - 1)
    plans, sp = _plans(pkg, mods, n), pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    a = _dev(E.case_ct(mods, n, 2, 2, 5))
    key, cdt = _dev(E.case_ct(mods, n, 4, 2, 7)), _dev(tab)
    o1, o2, ok = _empty((k, 2, 2, n)), _empty((2, k, 2, 2, n)), _empty((k, k + 1, 2, n))
    s = _empty((k + 1, n), 0)
    A, R, O1, O2, OK, S = (x.data_ptr() for x in (a, key, o1, o2, ok, s))
    ct_bytes = k * 2 * 2 * n * 8
    bad = [
        (B.FHE_E_INVALID, B.ckks_galois_evals_dev, (plans[0], 0, A, O1, 4)),
        (B.FHE_E_INVALID, B.ckks_galois_evals_dev, (plans[0], 6, A, O1, 4)),
        (B.FHE_E_INVALID, B.ckks_galois_evals_dev, (plans[0], 2 * n + 1, A, O1, 4)),
        (B.FHE_E_INVALID, B.ckks_galois_evals_dev, (plans[0], 5, O1 + 8 * n, O1, 4)),
        (B.FHE_E_NULL, B.ckks_galois_evals_dev, (plans[0], 5, None, O1, 4)),
        (B.FHE_E_NULL, B.ckks_galois_evals_dev, (None, 5, A, O1, 4)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_key_dev, (plans, sp, SEED, G.GK_BASE, 0, S, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_key_dev, (plans, sp, SEED, G.GK_BASE, 8, S, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_key_dev, (plans, sp, SEED, G.GK_BASE, 2 * n + 3, S, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_key_dev, (plans, sp, SEED, (1 << 63) - 2, 5, S, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_key_dev, (plans, sp, SEED, G.GK_BASE, 5, S, cdt.data_ptr(), 1025, OK)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_key_dev, (plans, sp, SEED, G.GK_BASE, 5, OK, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_key_dev, (plans, plans[0], SEED, G.GK_BASE, 5, S, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_PARAM_MISMATCH, B.ckks_rns_galois_key_dev, ([plans[0], other], sp, SEED, G.GK_BASE, 5, S, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_NULL, B.ckks_rns_galois_key_dev, (plans, sp, SEED, G.GK_BASE, 5, None, cdt.data_ptr(), len(tab), OK)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, sp, [R, R], [5, 4], k, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, sp, [R, R], [0, 5], k, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, sp, [R, R], [5, 2 * n], k, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, sp, [R] * 257, [5] * 257, k, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, sp, [R, R], [5, 25], k - 1, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, sp, [R, R], [5, 25], 9, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, sp, [R, R], [5, 25], k, O2 + ct_bytes, O2, 2)),      # the input inside the second output
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, sp, [R, O2 + 2 * ct_bytes - 8], [5, 25], k, A, O2, 2)),   # the second key at the output's last word
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, plans[0], [R, R], [5, 25], k, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, (plans, pkg.Plan(65537, n), [R, R], [5, 25], k, A, O2, 2)),
        (B.FHE_E_INVALID, B.ckks_rns_galois_dev, ([plans[0], plans[1], plans[0]], sp, [R, R], [5, 25], k, A, O2, 2)),
        (B.FHE_E_PARAM_MISMATCH, B.ckks_rns_galois_dev, ([plans[0], plans[1], other], sp, [R, R], [5, 25], k, A, O2, 2)),
        (B.FHE_E_NULL, B.ckks_rns_galois_dev, (plans, sp, [R, None], [5, 25], k, A, O2, 2)),
        (B.FHE_E_NULL, B.ckks_rns_galois_dev, (plans, sp, [R, R], [5, 25], k, None, O2, 2)),
        (B.FHE_E_NULL, B.ckks_rns_galois_dev, (plans, None, [R, R], [5, 25], k, A, O2, 2)),
    ]
    for code, fn, args in bad:
        with _refused() as e:
            fn(*args)
        assert e.value.code == code, (fn.__name__, args)
    bad_tab = _dev(np.array([5, 5, 9], dtype=U64))
    with _refused():
        B.ckks_rns_galois_key_dev(plans, sp, SEED, G.GK_BASE, 5, S, bad_tab.data_ptr(), 3, OK)
    B.ckks_rns_galois_dev(plans, sp, [R, R], [5, 25], k, A, O2, 0)
    B.ckks_rns_galois_dev(plans, sp, [], [], k, A, O2, 2)
    B.ckks_galois_evals_dev(plans[0], 5, A, O1, 0)
    for out in (o1, o2, ok):
        assert (_u64(out) == U64(FILL)).all()
