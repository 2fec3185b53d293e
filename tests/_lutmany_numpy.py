"""numpy restatement of the many-output small-integer bootstrap of DESIGN.md §15: the mod switch that forces nu low bits
to 0, the test vector that interleaves F = 2^nu tables, the whole of fhe_tfhe_lut_many_bootstrap_dev, the ideal lookup, the
netlists of the tests with t as a parameter, and a plan executed slot by slot with ideal lookups.  Words are u64 and wrap
mod 2^64.  Built on tests/_lut_numpy.py (§14), tests/_gadget_numpy.py (§11) and tests/_tfhe_numpy.py (§10)."""
import numpy as np

import _gadget_numpy as G
import _lut_numpy as LN
import _tfhe_numpy as R

U64 = np.uint64
BASE = LN.BASE


def mod_switch_nu(w, n, nu):
    """ms_nu(w) = ((((w >> (62 - L + nu)) + 1) >> 1) << nu) & (2N - 1): rounding to a multiple of 2^nu in Z_2N"""
    L = int(n).bit_length() - 1
    w = R.u64(w)
    return ((((w >> U64(62 - L + nu)) + U64(1)) >> U64(1)) << U64(nu)) & U64(2 * n - 1)


def mod_switch_nu_exact(w, n, nu):
    """the same with Python integers: w / 2^(63 - L + nu) rounded half up, times 2^nu, mod 2N"""
    L = int(n).bit_length() - 1
    unit = 1 << (63 - L + nu)
    return (((2 * int(w) + unit) // (2 * unit)) << nu) % (2 * n)


def expand_many(tables, n):
    """tables [F][P] -> the test vector [2][n] (mask 0, body v): h = i mod F, q = (i - h + half) >> (L - t),
    v[i] = T_h[q] if q < P, else 0 - T_h[0]"""
    tables = R.u64(tables)
    F, P = tables.shape
    L, t, nu = int(n).bit_length() - 1, P.bit_length() - 1, F.bit_length() - 1
    assert 1 << t == P and 1 << L == n and 1 << nu == F and 1 <= t <= L and nu <= L - t
    half = (n // P) // 2
    i = np.arange(n)
    h = i % F
    q = (i - h + half) >> (L - t)
    v = np.where(q < P, tables[h, np.minimum(q, P - 1)], U64(0) - tables[h, 0]).astype(np.uint64)
    return np.stack([np.zeros(n, dtype=np.uint64), v])


def prerounded(rows, n, nu):
    """words ms_nu(w) << (63 - L), which the plain mod switch (mod_switch_2n) maps back to ms_nu(w)"""
    L = int(n).bit_length() - 1
    return (mod_switch_nu(rows, n, nu) << U64(63 - L)).astype(np.uint64)


def valid_many(desc, wires, lut_count, nu):
    """LN.valid's operand rule, and lut + 2^nu <= lut_count"""
    d = np.asarray(desc, dtype=np.uint32).astype(np.int64).reshape(-1, 6)
    return LN.valid(d, wires) & (d[:, 0] + (1 << nu) <= lut_count)


def combine_many(pool, desc, lut_count, nu):
    """LN.combine with the many-output validity: invalid rows are all zero"""
    rows = LN.combine(pool, desc)
    rows[~valid_many(desc, len(pool), lut_count, nu)] = 0
    return rows


def bootstrap_rows_many(n, b, l, bsk, ks_b, ks_l, ksk, luts, pool, desc, nu):
    """the whole of fhe_tfhe_lut_many_bootstrap_dev in numpy (k = 1) -> [F][rows][n_lwe + 1]: per distinct first table,
    the gadget blind rotation of the pre-rounded combined rows with the interleaved test vector, the extraction at
    h = 0 .. F - 1 and the gadget key switch; invalid rows are all zero in every slice"""
    luts = R.u64(luts)
    F = 1 << nu
    d = np.asarray(desc, dtype=np.uint32).reshape(-1, 6)
    ok = valid_many(d, len(pool), len(luts), nu)
    rows = combine_many(pool, d, len(luts), nu)
    out = np.zeros((F, len(d), R.u64(ksk).shape[2]), dtype=np.uint64)
    for t0 in sorted({int(x) for x in d[ok, 0]}):
        sel = ok & (d[:, 0] == t0)
        acc = G.blind_rotation(n, 1, b, l, bsk, expand_many(luts[t0:t0 + F], n), prerounded(rows[sel], n, nu))
        for h in range(F):
            out[h, sel] = G.key_switch(ksk, R.sample_extraction(acc, h), ks_b, ks_l)
    return out


def ideal_lookup_many(tables, phase, n):
    """what the bootstrap gives for these phases, noise aside -> [F][len(phase)]: coefficients 0 .. F - 1 of
    rot(expand_many(tables), ms_nu(phase))"""
    tables = R.u64(tables)
    F = len(tables)
    v = expand_many(tables, n)[1]
    e = mod_switch_nu(np.atleast_1d(R.u64(phase)), n, F.bit_length() - 1)
    return np.array([R.rot(v, int(x))[:F] for x in e], dtype=np.uint64).T.copy()


# ---- netlists (built with fhe_study_amd.tfhe.LutCircuit), base 4 in a t of the caller's choice ---------------------------
def radix_adder(c, digits, t):
    """_lut_numpy.radix_adder with tables of 2^t entries; the largest lookup input is 3 + 3 + 1 = 7, so t >= 3"""
    assert t >= 3
    msg, carry_t = LN.table(lambda v: v % BASE, t), LN.table(lambda v: v // BASE, t)
    a = [c.input() for _ in range(digits)]
    b = [c.input() for _ in range(digits)]
    carry = None
    for i in range(digits):
        s = c.lin(a[i], 1, b[i], 1)
        c.output(c.lut(msg, s, 1, carry, 1 if carry is not None else 0))
        carry = c.lut(carry_t, s, 1, carry, 1 if carry is not None else 0)
    c.output(carry)
    return c


def digit_product(c, t):
    """_lut_numpy.digit_product with tables of 2^t entries: lo and hi digit of a b from one lookup input 4 a + b < 16, so t >= 4"""
    assert t >= 4
    a, b = c.input(), c.input()
    c.output(c.lut(LN.table(lambda v: (v // BASE) * (v % BASE) % BASE, t), a, BASE, b, 1))
    c.output(c.lut(LN.table(lambda v: (v // BASE) * (v % BASE) // BASE, t), a, BASE, b, 1))
    return c


def run_plan_ideal(plan, inputs, t, n):
    """a LutCircuitPlan executed as LutCircuit.evaluate issues it, on phases (u64 [batch] per input wire) and slot by slot:
    per level the nu = 0 lookups (LN.ideal_lookup), then one many-output call per nu (ideal_lookup_many, function h of chunk g
    into slot block + h G + g, unfilled functions included), then the lin groups -> phases per output.  A slot is read only
    after it was written (KeyError otherwise)."""
    batch = len(inputs[0]) if inputs else 1
    pool = {}
    for s, x in zip(plan.inputs, inputs):
        pool[s] = R.u64(x)
    for s, v in plan.consts:
        pool[s] = np.full(batch, LN.encode(v, t), dtype=np.uint64)

    def combined(row):
        _, x, y, sx, sy, c = (int(v) for v in row)
        s = np.full(batch, LN.encode(c, t), dtype=np.uint64)
        for idx, sc in ((x, sx), (y, sy)):
            if sc:
                s = s + LN.w(sc) * pool[idx]
        return s

    for lev in range(plan.depth + 1):
        if lev:
            lv = plan.levels[lev - 1]
            first, count = lv["luts"]
            for i in range(count):
                pool[first + i] = LN.ideal_lookup(plan.tables[int(lv["lut_desc"][i][0])], combined(lv["lut_desc"][i]), n)
            for m in lv.get("many", []):
                F, tabs = 1 << m["nu"], plan.many_tables[m["nu"]]
                for g in range(m["chunks"]):
                    t0 = int(m["desc"][g][0])
                    out = ideal_lookup_many(np.stack(tabs[t0:t0 + F]), combined(m["desc"][g]), n)
                    for h in range(F):
                        pool[m["block"] + h * m["chunks"] + g] = out[h]
        for grp in plan.lins[lev]:
            first, count = grp["slots"]
            for i in range(count):
                pool[first + i] = combined(grp["desc"][i])
    return [pool[s] for s in plan.outputs]
