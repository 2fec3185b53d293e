"""numpy restatement of the boolean gates of DESIGN.md §13: the (alpha, beta, o) table, the combination of two pool rows
that fhe_tfhe_gate_bootstrap_dev bootstraps, the two rows of a MUX and its finishing sum, the test vector, and bit
encoding / decoding.  Words are u64 and wrap mod 2^64.  Built on tests/_tfhe_numpy.py (§10)."""
import numpy as np

import _tfhe_numpy as R

U64 = np.uint64
MU = 1 << 61                               # bit 1 is phase +MU, bit 0 is -MU
COUNT = 10
# name: (alpha, beta, o / MU), in FHE_GATE_* order
TABLE = {"AND": (1, 1, -1), "NAND": (-1, -1, 1), "OR": (1, 1, 1), "NOR": (-1, -1, -1), "XOR": (2, 2, 2), "XNOR": (-2, -2, -2),
         "ANDNY": (-1, 1, -1), "ANDYN": (1, -1, -1), "ORNY": (-1, 1, 1), "ORYN": (1, -1, 1)}
NAMES = list(TABLE)
TRUTH = {"AND": lambda a, b: a & b, "NAND": lambda a, b: 1 - (a & b), "OR": lambda a, b: a | b, "NOR": lambda a, b: 1 - (a | b),
         "XOR": lambda a, b: a ^ b, "XNOR": lambda a, b: 1 - (a ^ b), "ANDNY": lambda a, b: (1 - a) & b,
         "ANDYN": lambda a, b: a & (1 - b), "ORNY": lambda a, b: (1 - a) | b, "ORYN": lambda a, b: a | (1 - b)}


def w(x):
    """a Python integer as a u64 word (mod 2^64)"""
    return U64(int(x) % (1 << 64))


def bit_phase(bit):
    return w(MU if bit else -MU)


def combine(pool, desc):
    """pool [wires][n_lwe+1], desc [batch][3] (op, x, y) -> [batch][n_lwe+1]: alpha c_x + beta c_y + (0 .. 0, o); an op
    >= COUNT or an index >= wires gives the all-zero row"""
    pool = R.u64(pool)
    wires = pool.shape[0]
    out = np.zeros((len(desc), pool.shape[1]), dtype=np.uint64)
    for m, (op, x, y) in enumerate(np.asarray(desc, dtype=np.int64)):
        if op >= COUNT or x >= wires or y >= wires:
            continue
        a, b, o = TABLE[NAMES[op]]
        out[m] = w(a) * pool[x] + w(b) * pool[y]
        out[m, -1:] += w(o * MU)                      # a slice: numpy wraps arrays without a warning
    return out


def mux_rows(pool, sel):
    """sel [batch][3] (s, a, b) -> the 2 batch rows the MUX blind-rotates: 2b = AND(s, a), 2b + 1 = ANDNY(s, b)"""
    sel = np.asarray(sel, dtype=np.int64)
    desc = np.empty((2 * len(sel), 3), dtype=np.int64)
    desc[0::2] = np.stack([np.full(len(sel), NAMES.index("AND")), sel[:, 0], sel[:, 1]], axis=1)
    desc[1::2] = np.stack([np.full(len(sel), NAMES.index("ANDNY")), sel[:, 0], sel[:, 2]], axis=1)
    return combine(pool, desc)


def mux_finish(ext):
    """extracted rows [2 batch][kN+1] -> [batch][kN+1]: E[2b] + E[2b + 1] + (0 .. 0, MU)"""
    ext = R.u64(ext)
    out = ext[0::2] + ext[1::2]
    out[:, -1] += U64(MU)
    return out


def test_vector(n):
    """(mask 0, body MU in every coefficient), k = 1: [2][n]"""
    v = np.zeros((2, n), dtype=np.uint64)
    v[1] = U64(MU)
    return v


def sign(phase):
    """what the bootstrap with test_vector gives, noise aside: +MU for a phase in [0, 1/2), -MU otherwise"""
    return np.where(R.u64(phase) < U64(1 << 63), U64(MU), U64((1 << 64) - MU))


def decode(lwe, s):
    """bits of TLWEs [..][n+1] under s: 1 where the centred phase is positive"""
    lwe = R.u64(lwe)
    p = lwe[..., -1] - lwe[..., :-1] @ R.u64(s)
    return (p.view(np.int64) > 0).astype(np.int64)


def phase_error(lwe, s, bits):
    """centred phase minus the encoding of `bits`, as Python integers"""
    lwe = R.u64(lwe)
    p = lwe[..., -1] - lwe[..., :-1] @ R.u64(s)
    want = np.array([bit_phase(b) for b in np.asarray(bits).reshape(-1)], dtype=np.uint64).reshape(p.shape)
    return (p - want).view(np.int64).astype(object)


# ---- circuits (built with fhe_study_amd.tfhe.Circuit) -----------------------------------------------------------------
def ripple_adder(c, bits):
    """x + y of two `bits`-bit inputs (bit 0 the least significant): inputs x_0 .. x_{bits-1}, y_0 .., outputs the
    bits + 1 bits of the sum"""
    x = [c.input() for _ in range(bits)]
    y = [c.input() for _ in range(bits)]
    carry = None
    for i in range(bits):
        t = c.gate("XOR", x[i], y[i])
        g = c.gate("AND", x[i], y[i])
        if carry is None:
            c.output(t)
            carry = g
        else:
            c.output(c.gate("XOR", t, carry))
            carry = c.gate("OR", g, c.gate("AND", t, carry))
    c.output(carry)
    return c


def maximum(c, bits):
    """max(x, y) of two `bits`-bit inputs: ge = (x >= y) from the least significant bit up, then a MUX per bit; uses NOT"""
    x = [c.input() for _ in range(bits)]
    y = [c.input() for _ in range(bits)]
    ge = c.gate("OR", x[0], c.not_(y[0]))
    for i in range(1, bits):
        gt = c.gate("AND", x[i], c.not_(y[i]))
        eq = c.gate("XNOR", x[i], y[i])
        ge = c.gate("OR", gt, c.gate("AND", eq, ge))
    for i in range(bits):
        c.output(c.mux(ge, x[i], y[i]))
    return c


def odd_netlist(c):
    """three inputs; fan-out, a gate reading one wire twice, a NOT of a NOT, a NOT of a constant, MUXes whose inputs come
    from different levels, a level with MUXes and no gates, an output that is an input and one wire output twice"""
    x, y, z = c.input(), c.input(), c.input()
    one = c.const(1)
    n_one = c.not_(one)                               # level 0: NOT of a constant
    g1 = c.gate("AND", x, y)                          # level 1, read four times below
    g2 = c.gate("XOR", x, x)                          # level 1: the same wire twice
    g3 = c.gate("OR", g1, n_one)                      # level 2
    g4 = c.gate("NAND", g1, z)                        # level 2
    nn = c.not_(c.not_(g4))                           # level 2: resolves to g4
    m1 = c.mux(g3, x, g2)                             # level 3: inputs of levels 2, 0 and 1
    m2 = c.mux(nn, g1, one)                           # level 3 has MUXes and no gate
    g5 = c.gate("ORNY", m1, m2)                       # level 4
    for w in (g5, x, g5, n_one, nn, m2):
        c.output(w)
    return c
