"""numpy restatement of the small-integer bootstrap of DESIGN.md §14: the expansion of a lookup table into its test vector,
the combination of pool rows that fhe_tlwe_lincomb_dev writes and fhe_tfhe_lut_bootstrap_dev bootstraps (with the
invalid-row rule), the bootstrap of a mixed batch table by table, the ideal lookup, and the netlists of the tests (base 4
in t = 4).  Words are u64 and wrap mod 2^64.  Built on tests/_tfhe_numpy.py (§10) and tests/_gadget_numpy.py (§11)."""
import numpy as np

import _gadget_numpy as G
import _tfhe_numpy as R

U64 = np.uint64
NONE = 0xFFFFFFFF                          # FHE_LUT_NONE: the index of an operand whose scale is 0, by convention
T_BITS, BASE = 4, 4                        # the netlists below: digits in [0, 4) inside values in [0, 16)


def w(x):
    """a Python integer as a u64 word (mod 2^64)"""
    return U64(int(x) % (1 << 64))


def delta(t):
    return 1 << (63 - t)


def encode(x, t):
    return w(int(x) * delta(t))


def table(f, t, out=None):
    """[2^t] torus words: entry x is out(f(x)), out = value Delta by default"""
    enc = (lambda v: encode(v, t)) if out is None else out
    return np.array([w(enc(f(x))) for x in range(1 << t)], dtype=np.uint64)


def expand(lut, n):
    """table [P] -> its test vector [2][n] (mask 0, body v): v[i] = T[m] for m = (i + half) >> (L - t) < P, else -T[0]"""
    lut = R.u64(lut)
    P, L = len(lut), int(n).bit_length() - 1
    t = P.bit_length() - 1
    assert 1 << t == P and 1 << L == n and 1 <= t <= L
    box = n // P
    half = box // 2
    m = (np.arange(n) + half) >> (L - t)
    v = np.where(m < P, lut[np.minimum(m, P - 1)], w(-int(lut[0]))).astype(np.uint64)
    return np.stack([np.zeros(n, dtype=np.uint64), v])


def valid(desc, wires, lut_count=None):
    """desc [rows][6] (lut, x, y, sx, sy, o_hi) -> bool [rows]: every operand with a non-zero scale has an index < wires
    (and, with lut_count: the bootstrap's rule, lut < lut_count)"""
    d = np.asarray(desc, dtype=np.uint32).astype(np.int64).reshape(-1, 6)
    ok = ((d[:, 3] == 0) | (d[:, 1] < wires)) & ((d[:, 4] == 0) | (d[:, 2] < wires))
    return ok if lut_count is None else ok & (d[:, 0] < lut_count)


def combine(pool, desc, lut_count=None):
    """pool [wires][n_lwe+1], desc [rows][6] u32 (sx, sy as int32) -> [rows][n_lwe+1]: sx pool[x] + sy pool[y] +
    (0 .. 0, o_hi 2^32); an invalid row (see valid) is all zero, and a zero-scale operand is never indexed"""
    pool = R.u64(pool)
    d = np.asarray(desc, dtype=np.uint32).reshape(-1, 6)
    ok = valid(d, pool.shape[0], lut_count)
    out = np.zeros((len(d), pool.shape[1]), dtype=np.uint64)
    for m, (_, x, y, sx, sy, o_hi) in enumerate(d):
        if not ok[m]:
            continue
        for idx, s in ((x, sx), (y, sy)):
            if s:
                out[m] += w(int(s) - ((int(s) >> 31) << 32)) * pool[int(idx)]      # the scale read as int32
        out[m, -1:] += w(int(o_hi) << 32)                # a slice: numpy wraps arrays without a warning
    return out


def bootstrap_rows(n, b, l, bsk, ks_b, ks_l, ksk, luts, pool, desc):
    """the whole of fhe_tfhe_lut_bootstrap_dev in numpy (k = 1): per distinct table, _gadget_numpy.bootstrap of the
    combined rows with the expanded table; invalid rows are all zero"""
    luts = R.u64(luts)
    d = np.asarray(desc, dtype=np.uint32).reshape(-1, 6)
    ok = valid(d, len(pool), len(luts))
    rows = combine(pool, d, len(luts))
    out = np.zeros((len(d), R.u64(ksk).shape[2]), dtype=np.uint64)
    for t in sorted({int(x) for x in d[ok, 0]}):
        sel = ok & (d[:, 0] == t)
        out[sel] = G.bootstrap(n, 1, b, l, bsk, expand(luts[t], n), ks_b, ks_l, ksk, rows[sel])
    return out


def ideal_lookup(lut, phase, n):
    """what the bootstrap gives for these phases, noise aside: coefficient 0 of rot(expand(lut), round(phase 2N / 2^64))"""
    v = expand(lut, n)[1]
    return np.array([R.rot(v, int(e))[0] for e in R.mod_switch(np.atleast_1d(R.u64(phase)), n)], dtype=np.uint64)


def evaluate_ideal(circ, inputs, t, n):
    """a LutCircuit on phases (u64 [batch] per input wire), every bootstrap replaced by ideal_lookup -> phases per output"""
    vals, it = [], iter(inputs)
    tabs = circ.tables
    for kind, args in circ._nodes:
        if kind == "input":
            vals.append(R.u64(next(it)))
            continue
        if kind == "const":
            vals.append(np.full(len(vals[0]) if vals else 1, encode(args[0], t), dtype=np.uint64))
            continue
        x, sx, y, sy, c = args[1:] if kind == "lut" else args
        batch = len(vals[x if x is not None else y]) if (x is not None or y is not None) else 1
        s = np.full(batch, encode(c, t), dtype=np.uint64)
        for v, sc in ((x, sx), (y, sy)):
            if sc:
                s = s + w(sc) * vals[v]
        vals.append(ideal_lookup(tabs[args[0]], s, n) if kind == "lut" else s)
    return [vals[o] for o in circ._outputs]


def decode(phase, t):
    """values of phases: round(phase / Delta) mod 2^(t+1) (the padding bit included)"""
    p = R.u64(phase)
    return (((p >> U64(62 - t)) + U64(1)) >> U64(1)).astype(np.int64) & ((2 << t) - 1)


def phases(lwe, s):
    lwe = R.u64(lwe)
    return lwe[..., -1] - lwe[..., :-1] @ R.u64(s)


def phase_error(lwe, s, want_words):
    """centred phase minus the expected torus words, as Python integers"""
    return (phases(lwe, s) - R.u64(want_words)).view(np.int64).astype(object)


# ---- netlists (built with fhe_study_amd.tfhe.LutCircuit), base 4 in t = 4 ------------------------------------------------
MSG = table(lambda v: v % BASE, T_BITS)
CARRY = table(lambda v: v // BASE, T_BITS)


def radix_adder(c, digits):
    """x + y of two numbers of `digits` base-4 digits (digit 0 the least significant): inputs a_0 .., b_0 .., outputs the
    `digits` digits of the sum and the carry-out.  s_i = a_i + b_i (lin); m_i = MSG[s_i + c_i] and c_{i+1} = CARRY[s_i + c_i]
    are the two lookups of digit i, in one call.  The largest lookup input is 3 + 3 + 1 = 7 < 16."""
    a = [c.input() for _ in range(digits)]
    b = [c.input() for _ in range(digits)]
    carry = None
    for i in range(digits):
        s = c.lin(a[i], 1, b[i], 1)
        c.output(c.lut(MSG, s, 1, carry, 1 if carry is not None else 0))
        carry = c.lut(CARRY, s, 1, carry, 1 if carry is not None else 0)
    c.output(carry)
    return c


def digit_product(c):
    """lo and hi digit of a b from one lookup input 4 a + b"""
    a, b = c.input(), c.input()
    c.output(c.lut(table(lambda v: (v // BASE) * (v % BASE) % BASE, T_BITS), a, BASE, b, 1))
    c.output(c.lut(table(lambda v: (v // BASE) * (v % BASE) // BASE, T_BITS), a, BASE, b, 1))
    return c


def less_than(c, out=None):
    """a < b for single digits: a - b + 4 lies in [1, 7], and is below 4 exactly when a < b; `out` encodes the result bit"""
    a, b = c.input(), c.input()
    c.output(c.lut(table(lambda v: int(v < BASE), T_BITS, out), a, 1, b, -1, const=BASE))
    return c
