"""Small integers with a lookup table per row, without a GPU: the expansion of a table against the
definition at every rotation, the combination and its invalid-row rule, LutCircuit.plan(), and the three netlists of
tests/_lut_numpy.py on noiseless inputs with the bootstrap replaced by its ideal function."""
import numpy as np
import pytest

import _lut_numpy as LN
import _tfhe_numpy as R

T = LN.T_BITS


@pytest.mark.parametrize("n,t", [(256, 1), (256, 2), (256, 4), (256, 8), (1024, 4)])
def test_expand_gives_the_table_at_coefficient_0_for_every_rotation(n, t):
    rng = np.random.default_rng(n + t)
    tab = rng.integers(0, 1 << 64, 1 << t, dtype=np.uint64, endpoint=False)
    L = n.bit_length() - 1
    half = (n >> t) // 2
    v = LN.expand(tab, n)
    assert v.shape == (2, n) and not v[0].any()
    got = np.array([R.rot(v[1], e)[0] for e in range(2 * n)], dtype=np.uint64)
    want = np.empty(2 * n, dtype=np.uint64)
    for e in range(n):
        want[e] = tab[(e + half) >> (L - t)] if e < n - half else LN.w(-int(tab[0]))
    want[n:] = np.uint64(0) - want[:n]
    assert np.array_equal(got, want)
    if t == L:
        assert half == 0 and np.array_equal(v[1], tab)                       # box = 1: no half box
    # a phase within half a box of x Delta gives T[x]; with the padding bit set, -T[x - P]
    for x in range(1 << t):
        for off in ({0} if half == 0 else {-half, 0, half - 1}):
            e = (x * (n >> t) + off) % (2 * n)
            assert got[e] == tab[x] and got[(e + n) % (2 * n)] == LN.w(-int(tab[x]))


def _desc(rows):
    return (np.array(rows, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)


def test_combine_scales_offsets_and_invalid_rows():
    rng = np.random.default_rng(3)
    wires, n_lwe = 5, 7
    pool = rng.integers(0, 1 << 64, (wires, n_lwe + 1), dtype=np.uint64, endpoint=False)
    W = lambda x: np.uint64(x % (1 << 64))
    body = lambda o_hi: np.array([0] * n_lwe + [o_hi << 32], dtype=np.uint64)
    desc = _desc([(0, 1, 2, 3, -4, 0),                                        # a negative scale
                  (0, 0, 4, -1, -1, 0xFFFFFFFF),                              # the largest o_hi
                  (9, 3, LN.NONE, 2, 0, 1 << 19),                             # a zero-scale operand with a wild index is valid
                  (0, 12345, 1, 0, 1, 0),
                  (0, LN.NONE, LN.NONE, 0, 0, 7),                             # no operand at all: a constant
                  (0, wires, 1, 1, 1, 5),                                     # invalid: x out of range with a scale
                  (0, 1, wires, 1, -1, 5),                                    # invalid: y
                  (0, LN.NONE, LN.NONE, 1, 0, 5),                             # invalid: the padding row of the evaluator
                  (0, wires - 1, wires - 1, 1, 1, 0)])
    got = LN.combine(pool, desc)
    want = [W(3) * pool[1] + W(-4) * pool[2], W(-1) * pool[0] + W(-1) * pool[4] + body(0xFFFFFFFF), W(2) * pool[3] + body(1 << 19),
            pool[1], body(7), None, None, None, W(2) * pool[4]]
    for g, x in zip(got, want):
        assert np.array_equal(g, np.zeros(n_lwe + 1, dtype=np.uint64) if x is None else x)
    assert list(LN.valid(desc, wires)) == [x is not None for x in want]
    # the bootstrap's rule adds lut >= lut_count: row 2 names table 9
    assert list(LN.valid(desc, wires, 5)) == [x is not None and i != 2 for i, x in enumerate(want)]
    assert not LN.combine(pool, desc, 5)[2].any() and LN.combine(pool, desc, 10)[2].any()
    # a value times Delta is an o_hi for every t
    for t in range(1, 13):
        assert LN.delta(t) % (1 << 32) == 0 and LN.delta(t) >= 1 << 51


def test_encodings_and_tables_of_the_python_surface_match_the_twin():
    from fhe_study_amd import binding, tfhe

    assert binding.FHE_LUT_NONE == tfhe.LUT_NONE == LN.NONE
    for t in (1, 4, 12):
        assert int(tfhe.encode_int(1, t)) == LN.delta(t) and int(tfhe.encode_int(-1, t)) == (1 << 64) - LN.delta(t)
        f = lambda v: (v * v + 1) % (1 << t)
        assert np.array_equal(tfhe.make_lut(f, t), LN.table(f, t))
    bit = lambda v: (1 << 61) if v else (1 << 64) - (1 << 61)
    assert np.array_equal(tfhe.make_lut(lambda v: v < 4, 4, bit), LN.table(lambda v: v < 4, 4, bit))
    tr = tfhe.trivial_int(np.array([0, 5, 15]), 4, 6)
    assert tr.words.shape == (3, 7) and not tr.words[:, :6].any()
    assert [int(x) for x in tr.words[:, 6]] == [0, 5 << 59, 15 << 59]


def test_header_declares_the_lut_surface():
    import os
    import re

    from fhe_study_amd import binding

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fhe_ntt.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+FHE_LUT_NONE\s+0xFFFFFFFFu", h)
    for name in ("fhe_tlwe_lincomb_dev", "fhe_tfhe_lut_bootstrap_dev"):
        assert re.search(r"\bint\s+" + name + r"\(", h) and name in binding.EXPORTS


def test_entry_points_check_their_arguments(pkg):
    L, B = pkg.load_library(), pkg.binding
    d, o = 16, 1 << 20                         # any non-NULL, 16-byte aligned fake device addresses: validation must fail first
    far = 1 << 40
    f = L.fhe_tfhe_lut_bootstrap_dev
    ok = (1024, 1, 10, 3, 630, d, 4, 4, d, 4, d, 2, d, 8, d, o, 1, None)
    for pos, v in [(0, 1000), (0, 128), (1, 2), (2, 11), (3, 0), (4, 0), (6, 33), (7, 0), (9, 0), (9, 11), (11, 0), (11, 1 << 32), (13, 0), (16, 0),
                   (16, 1 << 33), (13, 1 << 62)]:
        args = list(ok)
        args[pos] = v
        assert f(*args) in (B.FHE_E_INVALID, B.FHE_E_BAD_N), (pos, v)
        assert b"fhe_tfhe_lut_bootstrap_dev" in L.fhe_last_error()
    assert f(8192, 1, 8, 2, 630, d, 4, 4, d, 4, d, 2, d, 8, d, d, 1, None) == B.FHE_E_INVALID          # outside the gadget admission
    for i in (5, 8, 10, 12, 14, 15):
        args = list(ok)
        args[i] = None
        assert f(*args) == B.FHE_E_NULL, i
    args = list(ok)
    args[15] = 24
    assert f(*args) == B.FHE_E_INVALID and b"aligned" in L.fhe_last_error()
    nl, w = 630, L.fhe_tggsw_gadget_prepared_words(1024, 1, 10, 3)
    k_at, ks_at, desc_at, lut_at = far, far + (1 << 36), far + (1 << 37), far + (1 << 38)
    for out in (k_at + nl * w * 8 - 16, ks_at + 64, desc_at + 32, lut_at + 2 * 16 * 8 - 16):
        assert f(1024, 1, 10, 3, nl, k_at, 4, 4, ks_at, 4, lut_at, 2, far + (1 << 39), 8, desc_at, out, 2, None) == B.FHE_E_INVALID
        assert b"overlap" in L.fhe_last_error()
    g = L.fhe_tlwe_lincomb_dev
    for args in ((0, d, 8, d, d, 1, None), (630, d, 0, d, d, 1, None), (630, d, 8, d, d, 0, None), (630, d, 8, d, d, 1 << 33, None),
                 (630, d, 1 << 62, d, o, 1, None), (630, d, 8, d, 24, 1, None), (630, d, 8, desc_at, desc_at + 16, 2, None)):
        assert g(*args) == B.FHE_E_INVALID, args
        assert b"fhe_tlwe_lincomb_dev" in L.fhe_last_error() or b"aligned" in L.fhe_last_error()
    for i in (1, 3, 4):
        args = [630, d, 8, d, d, 1, None]
        args[i] = None
        assert g(*args) == B.FHE_E_NULL, i


def test_python_surface_refuses_bad_arguments():
    from fhe_study_amd import tfhe

    beta2 = type("K", (), {"log_beta": None, "n_lwe": 4})()
    c = tfhe.trivial_int([0, 1], T, 4)
    with pytest.raises(ValueError, match="gadget"):
        tfhe.lut_bootstrap(beta2, T, [tfhe.make_lut(lambda v: v, T)], [(0, 0, tfhe.LUT_NONE, 1, 0, 0)], c)
    with pytest.raises(ValueError, match="gadget"):
        tfhe.LutCircuit().evaluate(beta2, [], T)


def test_plan_of_the_adder_levels_sublevels_and_slices():
    from fhe_study_amd import tfhe

    D = 4
    c = LN.radix_adder(tfhe.LutCircuit(), D)
    p = c.plan()
    assert c.n_inputs == 2 * D and len(c.tables) == 2 and p.depth == D          # MSG and CARRY, each stored once
    kinds = [k for k, _ in c._nodes]
    lins = [w for w, k in enumerate(kinds) if k == "lin"]
    luts = [w for w, k in enumerate(kinds) if k == "lut"]
    assert [p.level[w] for w in lins] == [0] * D and [p.sub[w] for w in lins] == [0] * D
    assert [p.level[w] for w in luts] == [1 + i // 2 for i in range(2 * D)]    # m_i and c_{i+1} share level i + 1
    # slots: inputs, then the level-0 lins, then per level its two lookups: every group one contiguous slice
    assert p.inputs == list(range(2 * D))
    assert len(p.lins[0]) == 1 and p.lins[0][0]["slots"] == (2 * D, D)
    for i, lv in enumerate(p.levels):
        assert lv["level"] == i + 1 and lv["luts"] == (3 * D + 2 * i, 2) and lv["lut_desc"].shape == (2, 6)
        assert [int(x) for x in lv["lut_desc"][:, 0]] == [0, 1]
        s, carry = p.slot[lins[i]], (p.slot[luts[2 * i - 1]] if i else LN.NONE)
        assert [tuple(int(x) for x in r[1:]) for r in lv["lut_desc"]] == [(s, carry, 1, 1 if i else 0, 0)] * 2
        assert not p.lins[i + 1]
    assert p.n_slots == 3 * D + 2 * D and sorted(p.slot) == list(range(p.n_slots))
    assert p.outputs == [p.slot[luts[2 * i]] for i in range(D)] + [p.slot[luts[-1]]]


def test_plan_of_a_lin_chain_runs_in_order():
    from fhe_study_amd import tfhe

    c = tfhe.LutCircuit()
    x, y = c.input(), c.input()
    k = c.const(3)
    a = c.lin(x, 1, y, 1)                       # level 0, sub-level 0
    b = c.lin(a, 2, k, 1)                       # reads a lin of its level: sub-level 1
    d = c.lin(b, 1, a, -1, const=5)             # sub-level 2
    e = c.lin(x, 3)                             # sub-level 0 again
    ident = tfhe.make_lut(lambda v: v, T)
    u = c.lut(ident, d)                         # level 1
    v = c.lut(ident.copy(), e, 1, u, 1)         # level 2; an equal table is not stored twice
    f = c.lin(v, 1, a, 1)                       # level 2, sub-level 0: a is a lin of a lower level
    g = c.lin(f, 1, u, 0)                       # level 2, sub-level 1; the zero-scale operand is no operand
    z = c.lut(tfhe.make_lut(lambda v: 0, T), x, 0)   # no operand at all: level 1
    c.output(g)
    p = c.plan()
    assert len(c.tables) == 2
    assert [p.level[w] for w in (a, b, d, e, u, v, f, g, z)] == [0, 0, 0, 0, 1, 2, 2, 2, 1]
    assert [p.sub[w] for w in (a, b, d, e, f, g)] == [0, 1, 2, 0, 0, 1]
    assert [g_["slots"] for g_ in p.lins[0]] == [(3, 2), (5, 1), (6, 1)] and [p.slot[w] for w in (a, e, b, d)] == [3, 4, 5, 6]
    assert p.consts == [(2, 3)] and not p.lins[1]
    assert p.levels[0]["luts"] == (7, 2) and p.levels[1]["luts"] == (9, 1) and [g_["slots"] for g_ in p.lins[2]] == [(10, 1), (11, 1)]
    assert [int(x) for x in p.lins[0][2]["desc"][0]] == [LN.NONE, p.slot[b], p.slot[a], 1, -1, 5]
    assert [int(x) for x in p.lins[2][1]["desc"][0]] == [LN.NONE, p.slot[f], LN.NONE, 1, 0, 0]
    assert [int(x) for x in p.levels[0]["lut_desc"][1]] == [1, LN.NONE, LN.NONE, 0, 0, 0]
    assert p.outputs == [11] and p.n_slots == 12


def test_wires_used_before_they_are_defined_are_refused():
    from fhe_study_amd import tfhe

    ident = tfhe.make_lut(lambda v: v, T)
    c = tfhe.LutCircuit()
    x = c.input()
    for bad in (lambda: c.lin(1), lambda: c.lin(x, 1, 5, 1), lambda: c.lut(ident, 7), lambda: c.lut(ident, x, 1, -1, 1),
                lambda: c.output(3), lambda: c.lin("x"), lambda: c.lin(x, 1 << 31)):
        with pytest.raises(ValueError):
            bad()
    assert len(c._nodes) == 1
    c._nodes.append(("lin", (2, 1, None, 0, 0)))          # a forward reference smuggled past the builders
    with pytest.raises(ValueError):
        c.plan()


def _digits(v, count):
    return [(v >> (2 * i)) & 3 for i in range(count)]


@pytest.mark.parametrize("n", [256, 1024])
def test_netlists_on_noiseless_inputs_with_the_ideal_bootstrap(n):
    from fhe_study_amd import tfhe

    enc = lambda vals: np.array([LN.encode(v, T) for v in vals], dtype=np.uint64)
    D = 2
    xs, ys = np.repeat(np.arange(16), 16), np.tile(np.arange(16), 16)                   # every pair of 2-digit numbers
    ins = [enc((xs >> (2 * i)) & 3) for i in range(D)] + [enc((ys >> (2 * i)) & 3) for i in range(D)]
    outs = LN.evaluate_ideal(LN.radix_adder(tfhe.LutCircuit(), D), ins, T, n)
    assert np.array_equal(sum(LN.decode(o, T) << (2 * i) for i, o in enumerate(outs)), xs + ys)
    a, b = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    lo, hi = LN.evaluate_ideal(LN.digit_product(tfhe.LutCircuit()), [enc(a), enc(b)], T, n)
    assert np.array_equal(LN.decode(lo, T) + 4 * LN.decode(hi, T), a * b)
    (lt,) = LN.evaluate_ideal(LN.less_than(tfhe.LutCircuit()), [enc(a), enc(b)], T, n)
    assert np.array_equal(LN.decode(lt, T), (a < b).astype(np.int64))
    bit = lambda v: (1 << 61) if v else (1 << 64) - (1 << 61)
    (lt,) = LN.evaluate_ideal(LN.less_than(tfhe.LutCircuit(), bit), [enc(a), enc(b)], T, n)
    assert np.array_equal(lt.view(np.int64) > 0, a < b) and {int(x) for x in lt} == {1 << 61, (1 << 64) - (1 << 61)}
    # the same with half a box of error less one step on every lookup input: still exact
    eps = np.uint64((LN.delta(T) >> 1) - (1 << (63 - n.bit_length() + 1)))
    lo2, hi2 = LN.evaluate_ideal(LN.digit_product(tfhe.LutCircuit()), [enc(a), enc(b) + eps], T, n)
    assert np.array_equal(lo2, lo) and np.array_equal(hi2, hi)
