"""Boolean gates of DESIGN.md §13 without a device: the (alpha, beta, o) table puts every noise-free combination on the
right side of the sign function with a margin of 1/8, the MUX's two rows and finishing sum give the selected bit,
Circuit.plan() levels and slots, the Python helpers that need no bootstrap, and the argument checks of the entry points."""
import os
import re

import numpy as np
import pytest

import _gates_numpy as GN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dist(p, q):
    """torus distance of two words"""
    d = (int(p) - int(q)) % (1 << 64)
    return min(d, (1 << 64) - d)


@pytest.mark.parametrize("name", GN.NAMES)
def test_every_gate_lands_on_the_right_side_with_margin(name):
    alpha, beta, o = GN.TABLE[name]
    for a in (0, 1):
        for b in (0, 1):
            pool = np.zeros((2, 4), dtype=np.uint64)
            pool[0, -1], pool[1, -1] = GN.bit_phase(a), GN.bit_phase(b)
            row = GN.combine(pool, [(GN.NAMES.index(name), 0, 1)])[0]
            phase = row[-1]
            assert int(phase) == (alpha * (GN.MU if a else -GN.MU) + beta * (GN.MU if b else -GN.MU) + o * GN.MU) % (1 << 64)
            assert GN.sign(phase) == GN.bit_phase(GN.TRUTH[name](a, b)), (name, a, b)
            assert _dist(phase, 0) >= GN.MU and _dist(phase, 1 << 63) >= GN.MU, (name, a, b)


def test_mux_rows_and_sum_select_for_all_eight_inputs():
    for s in (0, 1):
        for a in (0, 1):
            for b in (0, 1):
                pool = np.zeros((3, 5), dtype=np.uint64)
                pool[:, -1] = [GN.bit_phase(v) for v in (s, a, b)]
                pool[:, :-1] = np.arange(12, dtype=np.uint64).reshape(3, 4) << np.uint64(40)   # masks combine like the bodies
                rows = GN.mux_rows(pool, [(0, 1, 2)])
                assert np.array_equal(rows[0], GN.combine(pool, [(GN.NAMES.index("AND"), 0, 1)])[0])
                assert np.array_equal(rows[1], GN.combine(pool, [(GN.NAMES.index("ANDNY"), 0, 2)])[0])
                for r in rows:
                    assert _dist(r[-1], 0) >= GN.MU and _dist(r[-1], 1 << 63) >= GN.MU
                # noise-free bootstraps return the sign as a trivial row; the finishing sum is then the selected bit
                ext = np.zeros((2, 5), dtype=np.uint64)
                ext[:, -1] = GN.sign(rows[:, -1])
                assert GN.mux_finish(ext)[0, -1] == GN.bit_phase(a if s else b), (s, a, b)


def test_invalid_rows_combine_to_zero_and_read_nothing():
    rng = np.random.default_rng(3)
    pool = rng.integers(0, 1 << 64, (4, 9), dtype=np.uint64, endpoint=False)
    desc = [(0, 1, 2), (GN.COUNT, 0, 1), (2, 4, 0), (3, 0, 4), (0xFFFFFFFF, 0xFFFFFFFF, 0)]
    out = GN.combine(pool, desc)
    assert np.array_equal(out[0], pool[1] + pool[2] - np.eye(9, dtype=np.uint64)[-1] * np.uint64(GN.MU))
    assert not out[1:].any()


def test_gate_codes_match_the_header():
    from fhe_study_amd import binding

    hdr = open(os.path.join(ROOT, "include", "fhe_ntt.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define FHE_GATE_(\w+) (\d+)", hdr)}
    assert codes.pop("COUNT") == GN.COUNT == binding.FHE_GATE_COUNT
    assert codes == binding.GATES == {n: i for i, n in enumerate(GN.NAMES)}


def test_trivial_bits_and_not_need_no_bootstrap():
    from fhe_study_amd import tfhe

    t = tfhe.trivial_bit([1, 0, 1], 6)
    assert t.words.shape == (3, 7) and not t.words[:, :-1].any()
    assert list(t.words[:, -1]) == [GN.bit_phase(1), GN.bit_phase(0), GN.bit_phase(1)]
    s = np.random.default_rng(1).integers(0, 2, 6, dtype=np.uint64)
    assert list(GN.decode(t.words, s)) == [1, 0, 1]
    c = np.random.default_rng(2).integers(0, 1 << 64, (2, 7), dtype=np.uint64, endpoint=False)
    n = tfhe.gate_not(tfhe.TLWE(c))
    assert np.array_equal(n.words + c, np.zeros_like(c))
    assert list(GN.decode(tfhe.gate_not(t).words, s)) == [0, 1, 0]


def _small_circuit():
    from fhe_study_amd import tfhe

    c = tfhe.Circuit()
    i0, i1, i2 = c.input(), c.input(), c.input()
    one = c.const(1)
    n0 = c.not_(i0)                                   # level 0
    g1 = c.gate("AND", i0, i1)                        # level 1
    g2 = c.gate("xor", n0, one)                       # level 1 (names are case-blind)
    n1 = c.not_(g1)                                   # level 1, no bootstrap
    m1 = c.mux(g1, i2, g2)                            # level 2
    g3 = c.gate(GN.NAMES.index("OR"), n1, m1)         # level 3
    nn = c.not_(c.not_(g3))                           # level 3: resolves to g3 itself
    m2 = c.mux(i0, i1, i2)                            # level 1
    for x in (nn, m2, n0):
        c.output(x)
    return c, dict(i0=i0, i1=i1, i2=i2, one=one, n0=n0, g1=g1, g2=g2, n1=n1, m1=m1, g3=g3, nn=nn, m2=m2)


def test_plan_levels_slots_and_not_chains():
    c, w = _small_circuit()
    p = c.plan()
    lv = {k: p.level[v] for k, v in w.items()}
    assert lv == dict(i0=0, i1=0, i2=0, one=0, n0=0, g1=1, g2=1, n1=1, m1=2, g3=3, nn=3, m2=1)
    assert p.depth == 3 and [x["level"] for x in p.levels] == [1, 2, 3]
    assert p.inputs == [0, 1, 2] and p.consts == [(3, 1)]
    assert sorted(p.slot) == list(range(p.n_slots)) and p.n_slots == len(p.slot)
    # every level's gates, then its MUXes, are contiguous slices right after the previous level's slots
    nxt = 5                                            # 3 inputs, 1 constant, 1 NOT of level 0
    for L in p.levels:
        (g0, gn), (m0, mn) = L["gates"], L["muxes"]
        assert g0 == nxt and m0 == g0 + gn
        gates = sorted(p.slot[v] for k, v in w.items() if k.startswith("g") and p.level[v] == L["level"])
        muxes = sorted(p.slot[v] for k, v in w.items() if k.startswith("m") and p.level[v] == L["level"])
        assert gates == list(range(g0, g0 + gn)) and muxes == list(range(m0, m0 + mn))
        assert L["gate_desc"].shape == (gn, 3) and L["mux_desc"].shape == (mn, 3)
        nxt = m0 + mn + len(p.nots[L["level"]])
    assert nxt == p.n_slots
    s = p.slot
    L1 = p.levels[0]
    assert [tuple(r) for r in L1["gate_desc"]] == [(0, s[w["i0"]], s[w["i1"]]), (4, s[w["n0"]], s[w["one"]])]
    assert [tuple(r) for r in L1["mux_desc"]] == [(s[w["i0"]], s[w["i1"]], s[w["i2"]])]
    assert [tuple(r) for r in p.levels[1]["mux_desc"]] == [(s[w["g1"]], s[w["i2"]], s[w["g2"]])]
    # NOTs carry no level of their own; a chain resolves to its root with the parity of its length
    assert p.nots[0] == [(s[w["n0"]], s[w["i0"]], True)]
    assert p.nots[1] == [(s[w["n1"]], s[w["g1"]], True)]
    assert p.nots[2] == []
    assert p.nots[3] == [(s[w["nn"]] - 1, s[w["g3"]], True), (s[w["nn"]], s[w["g3"]], False)]
    assert p.outputs == [s[w["nn"]], s[w["m2"]], s[w["n0"]]]


def test_plan_of_the_adder_and_the_maximum():
    from fhe_study_amd import tfhe

    p = GN.ripple_adder(tfhe.Circuit(), 4).plan()
    assert len(p.inputs) == 8 and len(p.outputs) == 5
    assert p.depth == 7                                 # XOR, then AND and OR per carry: 1 + 2 per bit after the first
    assert sum(L["gates"][1] for L in p.levels) == 4 * 2 + 3 * 3 and all(L["muxes"][1] == 0 for L in p.levels)
    q = GN.maximum(tfhe.Circuit(), 4).plan()
    assert q.levels[-1]["muxes"][1] == 4 and q.levels[-1]["gates"][1] == 0
    assert sum(len(v) for v in q.nots.values()) == 4


def test_plan_of_the_odd_netlist_keeps_the_pool_invariants():
    """GN.odd_netlist (what test_gates_gpu evaluates at odd batches): slots disjoint, every level's outputs one slice
    right after the slots before it, every descriptor and every NOT reading a slot below the level's first output"""
    from fhe_study_amd import tfhe

    c = GN.odd_netlist(tfhe.Circuit())
    p = c.plan()
    assert sorted(p.slot) == list(range(p.n_slots)) and p.n_slots == len(c._nodes) == 14
    assert p.depth == 4 and p.inputs == [0, 1, 2] and p.consts == [(3, 1)]
    assert p.nots[0] == [(4, 3, True)]                                  # the NOT of the constant
    assert [(L["gates"][1], L["muxes"][1]) for L in p.levels] == [(2, 0), (2, 0), (0, 2), (1, 0)]
    nxt = 5
    for L in p.levels:
        (g0, gn), (m0, mn) = L["gates"], L["muxes"]
        assert g0 == nxt and m0 == g0 + gn
        for desc in (L["gate_desc"][:, 1:], L["mux_desc"]):
            assert desc.size == 0 or int(desc.max()) < g0
        nxt = m0 + mn
        for dst, root, neg in p.nots[L["level"]]:
            assert dst == nxt and root < m0 + mn
            nxt += 1
    assert nxt == p.n_slots
    g1 = p.slot[5]
    assert sum(int((L["gate_desc"][:, 1:] == g1).sum() + (L["mux_desc"] == g1).sum()) for L in p.levels) == 3      # fan-out
    assert tuple(p.levels[0]["gate_desc"][1]) == (GN.NAMES.index("XOR"), 0, 0)                                   # one wire twice
    assert [r[1:] for r in p.nots[2]] == [(p.slot[8], True), (p.slot[8], False)]                                  # NOT of a NOT
    assert p.outputs[1] == 0 and p.outputs[0] == p.outputs[2] and len(p.outputs) == 6


def test_wires_used_before_they_are_defined_are_refused():
    from fhe_study_amd import tfhe

    c = tfhe.Circuit()
    a, b = c.input(), c.input()
    for f in (lambda: c.gate("AND", a, 2), lambda: c.gate("AND", -1, b), lambda: c.not_(5), lambda: c.mux(a, b, 7),
              lambda: c.output(9), lambda: c.gate("AND", a, 1.0)):
        with pytest.raises(ValueError, match="before it is defined"):
            f()
    with pytest.raises(ValueError, match="unknown gate"):
        c.gate("IMPLIES", a, b)
    with pytest.raises(ValueError):
        c.gate(10, a, b)
    # a netlist edited behind the builder's back is refused by plan()
    c._nodes.append(("gate", (0, a, 7)))
    with pytest.raises(ValueError, match="not defined before"):
        c.plan()


def test_gate_entry_points_check_their_arguments(pkg):
    L, B = pkg.load_library(), pkg.binding
    d = 16                                     # any non-NULL, 16-byte aligned fake device address: validation must fail first
    far = 1 << 40
    for f in (L.fhe_tfhe_gate_bootstrap_dev, L.fhe_tfhe_gate_mux_dev):
        ok = (1024, 1, 10, 3, 630, d, 4, 4, d, d, 8, d, d, 1, None)
        bad = [(0, 1000), (1, 2), (2, 11), (3, 0), (4, 0), (6, 33), (7, 0), (2, 0)]
        for pos, v in bad:
            args = list(ok)
            args[pos] = v
            assert f(*args) in (B.FHE_E_INVALID, B.FHE_E_BAD_N), (f, pos, v)
        assert f(8192, 1, 8, 2, 630, d, 4, 4, d, d, 8, d, d, 1, None) == B.FHE_E_INVALID      # outside the gadget admission
        assert f(1024, 1, 10, 3, 630, d, 4, 4, d, d, 0, d, d, 1, None) == B.FHE_E_INVALID
        assert b"wires" in L.fhe_last_error()
        for i in (5, 8, 9, 11, 12):
            args = list(ok)
            args[i] = None
            assert f(*args) == B.FHE_E_NULL, i
        assert f(1024, 1, 10, 3, 630, d, 4, 4, d, d, 8, d, 24, 1, None) == B.FHE_E_INVALID    # misaligned
        nl, w = 630, L.fhe_tggsw_gadget_prepared_words(1024, 1, 10, 3)
        k_at, ks_at, desc_at = far, far + (1 << 36), far + (1 << 37)
        for out in (k_at + nl * w * 8 - 16, ks_at + 64, desc_at + 16):
            assert f(1024, 1, 10, 3, nl, k_at, 4, 4, ks_at, far + (1 << 38), 8, desc_at, out, 2, None) == B.FHE_E_INVALID
            assert b"overlap" in L.fhe_last_error()
        assert f(1024, 1, 10, 3, 630, d, 4, 4, d, d, 8, d, d, 1 << 33, None) == B.FHE_E_INVALID
        assert b"batch" in L.fhe_last_error()
        assert f(1024, 1, 10, 3, 630, None, 4, 4, None, None, 8, None, None, 0, None) == B.FHE_OK


def test_python_gate_surface_refuses_bad_arguments(pkg):
    from fhe_study_amd import tfhe

    beta2 = type("K", (), {"log_beta": None, "n_lwe": 4})()
    c = tfhe.trivial_bit([0, 1], 4)
    with pytest.raises(ValueError, match="gadget"):
        tfhe.gate_bootstrap(beta2, "AND", c, c)
    with pytest.raises(ValueError, match="gadget"):
        tfhe.Circuit().evaluate(beta2, [])
    gk = type("K", (), {"log_beta": 10, "n_lwe": 4})()
    with pytest.raises(ValueError, match="unknown gate"):
        tfhe.gate_bootstrap(gk, "MAYBE", c, c)
    with pytest.raises(ValueError, match="one op per row"):
        tfhe.gate_bootstrap(gk, ["AND"] * 3, c, c)
    with pytest.raises(ValueError, match="same shape"):
        tfhe.mux(gk, c, c, tfhe.trivial_bit([1], 4))
