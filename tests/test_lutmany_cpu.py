"""Several lookup tables from one blind rotation, without a GPU: the interleaved test vector against the
definition at every admissible rotation, the nu-aware mod switch against exact rounding, the rejections of
fhe_tfhe_lut_many_bootstrap_dev that return before the device is touched, and LutCircuit.plan(share) with its plans
executed slot by slot on noiseless inputs with ideal lookups."""
import numpy as np
import pytest

import _lut_numpy as LN
import _lutmany_numpy as LM
import _tfhe_numpy as R


def _shapes():
    """(N, t, nu) for N in {16, 64}: every t, every nu <= min(L - t, 4); nu = L - t and t = L are among them"""
    out = []
    for n in (16, 64):
        L = n.bit_length() - 1
        out += [(n, t, nu) for t in range(1, L + 1) for nu in range(min(L - t, 4) + 1)]
    return out


def test_the_shapes_of_the_twin_identity_include_the_edges():
    s = _shapes()
    assert (16, 4, 0) in s and (64, 6, 0) in s                                  # t = L
    assert (16, 2, 2) in s and (64, 2, 4) in s and (64, 5, 1) in s              # nu = L - t: F = box
    assert (64, 1, 4) in s and (64, 1, 5) not in s                              # nu <= 4


@pytest.mark.parametrize("n,t,nu", _shapes())
def test_expand_many_gives_table_h_at_coefficient_h_for_every_rounded_rotation(n, t, nu):
    rng = np.random.default_rng(1000 * n + 10 * t + nu)
    F, P, box = 1 << nu, 1 << t, n >> t
    tabs = rng.integers(0, 1 << 64, (F, P), dtype=np.uint64, endpoint=False)
    v = LM.expand_many(tabs, n)
    assert v.shape == (2, n) and not v[0].any()
    if nu == 0:
        assert np.array_equal(v, LN.expand(tabs[0], n))
    for e in range(0, 2 * n, F):                                                # every rotation the mod switch can produce
        x = ((e + box // 2) // box) % (2 * P)                                   # the box of e: a phase within half a box of x Delta
        got = R.rot(v[1], e)[:F]
        want = tabs[:, x] if x < P else np.uint64(0) - tabs[:, x - P]
        assert np.array_equal(got, want), (e, x)
    # the ideal lookup is that coefficient, for phases at the centre and at both edges of every box
    L = n.bit_length() - 1
    step = 1 << (63 - L)                                                        # one unit of Z_2N as a torus word
    for x in range(2 * P):
        for off in ({-(box // 2), 0, box // 2 - F} if box // 2 >= F else {0}):                  # F = box: only the centre rounds into it
            ph = np.array([((x * box + off) * step) % (1 << 64)], dtype=np.uint64)
            got = LM.ideal_lookup_many(tabs, ph, n)[:, 0]
            want = tabs[:, x] if x < P else np.uint64(0) - tabs[:, x - P]
            assert np.array_equal(got, want), (x, off)


@pytest.mark.parametrize("n", [16, 256, 1024, 4096])
def test_mod_switch_nu_against_exact_rounding(n):
    L = n.bit_length() - 1
    rng = np.random.default_rng(n)
    for nu in range(0, 5):
        unit = 1 << (63 - L + nu)                                               # one multiple of 2^nu in Z_2N, as a torus word
        ws = [0, 1, (1 << 64) - 1, (1 << 63), (1 << 63) - 1, unit // 2 - 1, unit // 2, unit // 2 + 1, unit, unit + unit // 2 - 1,
              unit + unit // 2, (1 << 64) - unit // 2 - 1, (1 << 64) - unit // 2, (1 << 64) - unit, (7 * unit + unit // 2) % (1 << 64)]
        ws += [int(x) for x in rng.integers(0, 1 << 64, 200, dtype=np.uint64, endpoint=False)]
        got = LM.mod_switch_nu(np.array(ws, dtype=np.uint64), n, nu)
        assert [int(x) for x in got] == [LM.mod_switch_nu_exact(x, n, nu) for x in ws]
        assert not (got & np.uint64((1 << nu) - 1)).any() and (got < 2 * n).all()
        # ties round up; words within half a unit of 2^64 round up to 2N = 0
        assert LM.mod_switch_nu_exact(unit // 2, n, nu) == 1 << nu and LM.mod_switch_nu_exact(unit // 2 - 1, n, nu) == 0
        assert int(LM.mod_switch_nu(np.uint64((1 << 64) - unit // 2), n, nu)) == 0 == int(LM.mod_switch_nu(np.uint64((1 << 64) - 1), n, nu))
        assert int(LM.mod_switch_nu(np.uint64((1 << 64) - unit // 2 - 1), n, nu)) == 2 * n - (1 << nu)
        if nu == 0:
            assert np.array_equal(got, R.mod_switch(np.array(ws, dtype=np.uint64), n))
            assert [int(x) for x in got] == [R.mod_switch_exact(x, n) for x in ws]
        # prerounded words go back to ms_nu through the plain mod switch
        assert np.array_equal(R.mod_switch(LM.prerounded(np.array(ws, dtype=np.uint64), n, nu), n), got)


def test_header_and_binding_declare_the_call():
    import ctypes
    import os
    import re

    from fhe_study_amd import binding, tfhe

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fhe_ntt.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+fhe_tfhe_lut_many_bootstrap_dev\(", h) and "fhe_tfhe_lut_many_bootstrap_dev" in binding.EXPORTS
    m = re.search(r"int\s+fhe_tfhe_lut_many_bootstrap_dev\(([^;]*)\);", h)
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 19 and params[9] == "unsigned t_bits" and params[10] == "unsigned nu"
    L = binding.load_library()
    one, many = L.fhe_tfhe_lut_bootstrap_dev.argtypes, L.fhe_tfhe_lut_many_bootstrap_dev.argtypes
    assert list(many) == list(one[:10]) + [ctypes.c_uint] + list(one[10:])      # `unsigned nu` after t_bits, the rest as §14's
    assert callable(tfhe.lut_many_bootstrap) and callable(binding.tfhe_lut_many_bootstrap_dev)


def test_entry_point_checks_its_arguments(pkg):
    L, B = pkg.load_library(), pkg.binding
    d, o = 16, 1 << 20                         # any non-NULL, 16-byte aligned fake device addresses: validation must fail first
    far = 1 << 40
    f = L.fhe_tfhe_lut_many_bootstrap_dev
    #     n    k  b  l  n_lwe bsk ksb ksl ksk t nu luts cnt pool wires desc out batch stream
    ok = (1024, 1, 10, 3, 630, d, 4, 4, d, 3, 1, d, 2, d, 8, d, o, 1, None)
    bad = [(0, 1000), (0, 128), (1, 2), (2, 11), (3, 0), (4, 0), (6, 33), (7, 0), (9, 0), (9, 11),
           (10, 5), (10, 8),                                                     # nu = 5 (<= L - t here), nu > L - t
           (12, 0), (12, 1 << 32), (14, 0), (17, 0), (17, 1 << 33), (14, 1 << 62)]
    for pos, v in bad:
        args = list(ok)
        args[pos] = v
        assert f(*args) in (B.FHE_E_INVALID, B.FHE_E_BAD_N), (pos, v)
        assert b"fhe_tfhe_lut_many_bootstrap_dev" in L.fhe_last_error()
    for t, nu in ((10, 1), (7, 4), (9, 2), (6, 5), (1, 5)):                     # t_bits = L with nu = 1; nu > L - t; nu = 5
        args = list(ok)
        args[9], args[10] = t, nu
        assert f(*args) == B.FHE_E_INVALID, (t, nu)
        assert b"fhe_tfhe_lut_many_bootstrap_dev" in L.fhe_last_error() and b"nu" in L.fhe_last_error()
    assert f(256, 1, 8, 3, 8, d, 4, 4, d, 8, 1, d, 2, d, 8, d, o, 1, None) == B.FHE_E_INVALID          # t_bits = L = 8, nu = 1
    assert f(8192, 1, 8, 2, 630, d, 4, 4, d, 4, 1, d, 2, d, 8, d, d, 1, None) == B.FHE_E_INVALID       # outside the gadget admission
    for i in (5, 8, 11, 13, 15, 16):
        args = list(ok)
        args[i] = None
        assert f(*args) == B.FHE_E_NULL, i
        assert b"fhe_tfhe_lut_many_bootstrap_dev" in L.fhe_last_error()
    for i in (5, 8, 11, 13, 15, 16):
        args = list(ok)
        args[i] = 24
        assert f(*args) == B.FHE_E_INVALID and b"aligned" in L.fhe_last_error(), i
    # overlaps are taken over all F batch rows of d_out: with nu = 2, batch = 2 the output is 8 rows of 631 words
    nl, w = 630, L.fhe_tggsw_gadget_prepared_words(1024, 1, 10, 3)
    k_at, ks_at, desc_at, lut_at = far, far + (1 << 36), far + (1 << 37), far + (1 << 38)
    row, span = 631 * 8, 8 * 631 * 8

    def call(out, nu):
        return f(1024, 1, 10, 3, nl, k_at, 4, 4, ks_at, 3, nu, lut_at, 4, far + (1 << 39), 8, desc_at, out, 2, None)

    for out in (k_at + nl * w * 8 - 16, ks_at + 64, desc_at + 32, lut_at + 4 * 8 * 8 - 16,
                k_at - span + 16, ks_at - span + 16, desc_at - span + 16, lut_at - span + 16):          # only the last slice reaches in
        assert call(out, 2) == B.FHE_E_INVALID, hex(out)
        assert b"overlap" in L.fhe_last_error() and b"fhe_tfhe_lut_many_bootstrap_dev" in L.fhe_last_error()
    # the same d_out with nu = 1 (4 rows) ends before the buffer: the next check, a launch, would follow.  Not called here.
    assert span - 16 > 4 * row


def test_python_surface_refuses_bad_arguments():
    from fhe_study_amd import tfhe

    beta2 = type("K", (), {"log_beta": None, "n_lwe": 4, "n": 256})()
    c = tfhe.trivial_int([0, 1], 3, 4)
    with pytest.raises(ValueError, match="gadget"):
        tfhe.lut_many_bootstrap(beta2, 3, 1, [tfhe.make_lut(lambda v: v, 3)] * 2, [(0, 0, tfhe.LUT_NONE, 1, 0, 0)], c)
    with pytest.raises(ValueError, match="gadget"):
        tfhe.LutCircuit().evaluate(beta2, [], 3, share=1)
    gadget = type("K", (), {"log_beta": 8, "n_lwe": 4, "n": 256})()
    with pytest.raises(ValueError, match="share"):
        tfhe.LutCircuit().evaluate(gadget, [], 7, share=2)                      # share > L - t_bits = 1
    with pytest.raises(ValueError, match="share"):
        tfhe.LutCircuit().evaluate(gadget, [], 8, share=1)                      # t_bits = L
    for share in (-1, 5):
        with pytest.raises(ValueError, match="share"):
            tfhe.LutCircuit().plan(share=share)


def _same_plan(p, q):
    assert sorted(vars(p)) == sorted(vars(q))
    for name in ("slot", "level", "sub", "n_slots", "inputs", "consts", "outputs", "many_tables"):
        assert getattr(p, name) == getattr(q, name), name
    assert len(p.tables) == len(q.tables) and all(np.array_equal(a, b) for a, b in zip(p.tables, q.tables))
    assert len(p.levels) == len(q.levels)
    for a, b in zip(p.levels, q.levels):
        assert sorted(a) == sorted(b) == ["level", "lut_desc", "luts"]
        assert a["level"] == b["level"] and a["luts"] == b["luts"] and np.array_equal(a["lut_desc"], b["lut_desc"])
    assert sorted(p.lins) == sorted(q.lins)
    for lev in p.lins:
        assert len(p.lins[lev]) == len(q.lins[lev])
        for a, b in zip(p.lins[lev], q.lins[lev]):
            assert sorted(a) == sorted(b) == ["desc", "slots"] and a["slots"] == b["slots"] and np.array_equal(a["desc"], b["desc"])


def test_plan_with_share_0_is_the_plan_of_today():
    from fhe_study_amd import tfhe

    for build in (lambda c: LN.radix_adder(c, 4), LN.digit_product, LN.less_than):
        c = build(tfhe.LutCircuit())
        p0 = c.plan(share=0)
        _same_plan(p0, c.plan())
        assert p0.many_tables == {}
    # and it is §14's: the adder's slots as tests/test_lut_cpu.py states them
    p = LN.radix_adder(tfhe.LutCircuit(), 4).plan(share=0)
    assert [lv["luts"] for lv in p.levels] == [(12 + 2 * i, 2) for i in range(4)] and p.n_slots == 20


def _wire_slots_and_reads(c, p):
    """(the slots of the wires, the slots any descriptor reads)"""
    reads = set()
    groups = [lv["lut_desc"] for lv in p.levels] + [m["desc"] for lv in p.levels for m in lv["many"]] + \
             [g["desc"] for gs in p.lins.values() for g in gs]
    for d in groups:
        for _, x, y, sx, sy, _ in (tuple(int(v) for v in r) for r in d):
            reads |= {s for s, sc in ((x, sx), (y, sy)) if sc}
    return list(p.slot), reads


def _check_plan_structure(c, p):
    slots, reads = _wire_slots_and_reads(c, p)
    assert len(set(slots)) == len(slots) and all(0 <= s < p.n_slots for s in slots)              # all slots are distinct
    assert reads <= set(slots)                                                                   # no descriptor reads a scratch slot
    # blocks do not collide: every slot of the pool is a wire's or a scratch function's, once
    owned = list(slots)
    for lv in p.levels:
        for m in lv["many"]:
            block = set(range(m["block"], m["block"] + (m["chunks"] << m["nu"])))
            owned += sorted(block - set(slots))
    assert sorted(owned) == list(range(p.n_slots))


def _adder_pairs():
    """256 pairs of 4-digit numbers: the 16 edge pairs of {0, 1, 85, 255}^2 and 240 seeded ones (DESIGN.md §14's set)"""
    edge = [(x, y) for x in (0, 1, 85, 255) for y in (0, 1, 85, 255)]
    rnd = np.random.default_rng(2024).integers(0, 256, (240, 2))
    p = np.array(edge + [tuple(r) for r in rnd])
    return p[:, 0], p[:, 1]


def _enc(vals, t):
    return np.array([LN.encode(v, t) for v in vals], dtype=np.uint64)


def test_plan_of_the_t3_adder_with_share_1_and_its_ideal_run():
    from fhe_study_amd import tfhe

    D, t, n = 4, 3, 256
    c = LM.radix_adder(tfhe.LutCircuit(), D, t)
    p = c.plan(share=1)
    assert p.depth == D and set(p.many_tables) == {1}
    assert len(p.many_tables[1]) == 2                                           # (MSG, CARRY), stored once for the four levels
    assert np.array_equal(p.many_tables[1][0], LN.table(lambda v: v % 4, t)) and np.array_equal(p.many_tables[1][1], LN.table(lambda v: v // 4, t))
    luts = [w for w, (k, _) in enumerate(c._nodes) if k == "lut"]
    lins = [w for w, (k, _) in enumerate(c._nodes) if k == "lin"]
    for i, lv in enumerate(p.levels):
        assert lv["luts"][1] == 0 and len(lv["lut_desc"]) == 0                  # no nu = 0 lut
        assert len(lv["many"]) == 1
        m = lv["many"][0]
        assert (m["nu"], m["chunks"], m["block"]) == (1, 1, 3 * D + 2 * i) and m["desc"].shape == (1, 6)
        assert [p.slot[luts[2 * i]], p.slot[luts[2 * i + 1]]] == [m["block"], m["block"] + 1]     # function h at block + h G + g
        carry = p.slot[luts[2 * i - 1]] if i else LN.NONE
        assert [int(x) for x in m["desc"][0]] == [0, p.slot[lins[i]], carry, 1, 1 if i else 0, 0]
    assert p.n_slots == 5 * D
    _check_plan_structure(c, p)
    xs, ys = _adder_pairs()
    ins = [_enc((xs >> (2 * i)) & 3, t) for i in range(D)] + [_enc((ys >> (2 * i)) & 3, t) for i in range(D)]
    got = LM.run_plan_ideal(p, ins, t, n)
    want = LN.evaluate_ideal(c, ins, t, n)
    assert len(got) == D + 1 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(sum(LN.decode(o, t) << (2 * i) for i, o in enumerate(got)), xs + ys)
    # the share = 0 plan of the same netlist, executed the same way, agrees
    got0 = LM.run_plan_ideal(c.plan(share=0), ins, t, n)
    assert all(np.array_equal(g, w) for g, w in zip(got0, want))


def _class_netlist(c, tfhe, t, sizes):
    """two inputs; per size, a class of that many lookups of x + y + const (const distinguishes the classes), each with a table
    of its own; a second level that reads every one of them"""
    x, y = c.input(), c.input()
    outs = []
    for ci, size in enumerate(sizes):
        for j in range(size):
            outs.append(c.lut(tfhe.make_lut(lambda v, a=ci, b=j: (v * (b + 1) + a + b) % 4, t), x, 1, y, 1, const=ci))
    acc = outs[0]
    for w in outs[1:]:
        acc = c.lut(tfhe.make_lut(lambda v: v % 4, t), acc, 1, w, 1)            # a chain: one nu = 0 lookup per level
    for w in outs + [acc]:
        c.output(w)
    return c, outs


@pytest.mark.parametrize("sizes,share,want", [((3,), 2, {2: 1}), ((5,), 2, {2: 1}), ((3, 2, 1), 2, {2: 1, 1: 1}), ((5, 4), 1, {1: 4})])
def test_plan_with_classes_of_3_and_5_wires(sizes, share, want):
    """a class of 3 with share = 2 is one nu = 2 chunk with one padded function; a class of 5 is chunks of 4 + 1, and the
    single wire goes through the nu = 0 call; share = 1 cuts 5 into 2 + 2 + 1 and 4 into 2 + 2"""
    from fhe_study_amd import tfhe

    t, n = 3, 64
    c, outs = _class_netlist(tfhe.LutCircuit(), tfhe, t, sizes)
    p = c.plan(share=share)
    lv = p.levels[0]
    assert {m["nu"]: m["chunks"] for m in lv["many"]} == want
    singles = sum(s % (1 << share) == 1 for s in sizes)
    assert lv["luts"][1] == singles
    assert [m["nu"] for m in lv["many"]] == sorted(want)                        # blocks in the order of nu, after the nu = 0 wires
    nxt = lv["luts"][0] + singles
    for m in lv["many"]:
        assert m["block"] == nxt
        nxt += m["chunks"] << m["nu"]
    _check_plan_structure(c, p)
    if sizes == (3,):
        m = lv["many"][0]
        assert [p.slot[w] for w in outs] == [m["block"], m["block"] + 1, m["block"] + 2]          # G = 1: slots block + h
        tabs = p.many_tables[2]
        assert len(tabs) == 4 and np.array_equal(tabs[3], tabs[0])                              # the padded function repeats the first table
        assert m["block"] + 3 not in p.slot and p.n_slots == len(c._nodes) + 1                  # one scratch slot
    if sizes == (5,):
        m = lv["many"][0]
        assert [p.slot[w] for w in outs[:4]] == [m["block"] + h for h in range(4)] and p.slot[outs[4]] == lv["luts"][0]
        assert int(lv["lut_desc"][0][0]) == c._nodes[outs[4]][1][0]                             # the nu = 0 wire keeps its own table index
    if sizes == (5, 4):
        m = lv["many"][0]                                                                       # G = 4 chunks: function h of chunk g at block + 4 h + g
        chunks = [outs[0:2], outs[2:4], outs[5:7], outs[7:9]]
        for g, ch in enumerate(chunks):
            assert [p.slot[w] for w in ch] == [m["block"] + 4 * h + g for h in range(2)]
        assert [int(r[0]) for r in m["desc"]] == [0, 2, 4, 6] and len(p.many_tables[1]) == 8
    xs, ys = np.repeat(np.arange(3), 3), np.tile(np.arange(3), 3)               # x + y + const <= 2 + 2 + 2 = 6 < 8
    ins = [_enc(xs, t), _enc(ys, t)]
    got = LM.run_plan_ideal(p, ins, t, n)
    want_out = LN.evaluate_ideal(c, ins, t, n)
    assert len(got) == len(want_out) and all(np.array_equal(g, w) for g, w in zip(got, want_out))
    assert all(LN.decode(g, t).max() < 4 for g in got)


def test_identical_chunks_are_stored_once_and_padding_is_per_chunk():
    from fhe_study_amd import tfhe

    t = 3
    c = tfhe.LutCircuit()
    x, y = c.input(), c.input()
    A, B, C = (tfhe.make_lut(f, t) for f in (lambda v: v % 4, lambda v: v // 4, lambda v: (v + 1) % 4))
    for src in (x, y):
        c.output(c.lut(A, src))
        c.output(c.lut(B, src))                                                 # two classes with the same tables (A, B)
    u = [c.lut(tb, x, 1, y, 1) for tb in (B, A, C)]                             # a class of 3: (B, A, C, B) at nu = 2
    p = c.plan(share=2)
    lv = p.levels[0]
    assert {m["nu"]: m["chunks"] for m in lv["many"]} == {1: 2, 2: 1}
    assert [int(r[0]) for r in lv["many"][0]["desc"]] == [0, 0] and len(p.many_tables[1]) == 2
    assert [np.array_equal(a, b) for a, b in zip(p.many_tables[2], (B, A, C, B))] == [True] * 4
    _check_plan_structure(c, p)
    assert len(u) == 3
