"""Every failure branch of the TFHE bootstrap and key-switch entry points, without a device: one table of calls per entry
point (each distinct branch, calls that break two rules at once so that the order of the checks is pinned, and the empty
batch), each recorded with its return code and the whole last-error message.  The pointers are made-up addresses: every
call here must be answered before anything touches the GPU."""
import pytest

# the shape every table starts from (tests/test_gadget_cpu.py): N = 1024, k = 1, b = 8, l = 3, n_lwe = 630, key switch b = 4, l = 4
N, K, LB, LL, NL, KSB, KSL = 1024, 1, 8, 3, 630, 4, 4
BSK, TAB, KSK, IN, OUT, POOL, DESC, LUTS = (i << 44 for i in range(1, 9))        # 16-byte aligned and far apart
BSK_BYTES = NL * 2 * (K + 1) * LL * (K + 1) * N * 8
KSK_BYTES = K * N * KSL * (NL + 1) * 8
PFKSK_BYTES = (K + 1) * (K * N + 1) * 2 * (K + 1) * N * 8                          # pf_l = 2

BOOT = dict(n=N, k=K, log_beta=LB, l=LL, n_lwe=NL, bsk=BSK)
KS = dict(ks_log_beta=KSB, ks_l=KSL, ksk=KSK)
ENTRY = {
    "gadget": ("fhe_tfhe_gadget_bootstrap_dev", dict(BOOT, table=TAB, **KS, inp=IN, out=OUT, batch=2, st=None)),
    "rows": ("fhe_tfhe_gadget_bootstrap_rows_dev", dict(BOOT, table=TAB, **KS, inp=IN, out=OUT, batch=2, st=None)),
    "gate": ("fhe_tfhe_gate_bootstrap_dev", dict(BOOT, **KS, pool=POOL, wires=4, desc=DESC, out=OUT, batch=2, st=None)),
    "mux": ("fhe_tfhe_gate_mux_dev", dict(BOOT, **KS, pool=POOL, wires=4, desc=DESC, out=OUT, batch=2, st=None)),
    "lut": ("fhe_tfhe_lut_bootstrap_dev", dict(BOOT, **KS, t=3, luts=LUTS, lut_count=2, pool=POOL, wires=4, desc=DESC, out=OUT, batch=2, st=None)),
    "many": ("fhe_tfhe_lut_many_bootstrap_dev",
             dict(BOOT, **KS, t=3, nu=1, luts=LUTS, lut_count=2, pool=POOL, wires=4, desc=DESC, out=OUT, batch=2, st=None)),
    "cb": ("fhe_tfhe_circuit_bootstrap_dev",
           dict(BOOT, cb_log_beta=4, cb_l=3, pf_log_beta=8, pf_l=2, pfksk=KSK, inp=IN, out=OUT, batch=2, st=None)),
    "ks": ("fhe_tlwe_key_switch_dev", dict(n_in=N, n_out=NL, beta=2, l=64, ksk=KSK, inp=IN, out=OUT, batch=2, st=None)),
    "gks": ("fhe_tlwe_gadget_key_switch_dev", dict(n_in=N, n_out=NL, log_beta=KSB, l=KSL, ksk=KSK, inp=IN, out=OUT, batch=2, st=None)),
}
ROW8 = (NL + 1) * 8                     # bytes of one output row
HUGE_KS = dict(n_in=1, n_out=1, batch=1 << 37, out=16, inp=1 << 60, ksk=1 << 61)      # 2^32 tiles, nothing overlapping

# (entry, what the call breaks, the arguments it changes, return code, last error)
CASES = [
    ("gadget", "n not a power of two", dict(n=1000), -1, "fhe_tfhe_gadget_bootstrap_dev: n=1000 must be a power of two in [2, 2^19]"),
    ("gadget", "no gadget product", dict(log_beta=11), -9,
     "fhe_tfhe_gadget_bootstrap_dev: no gadget product for n=1024, k=1, log_beta=11, l=3 (needs k = 1, 256 <= n <= 4096, "
     "(k+1) l n (2^32-1) 2^(log_beta-1) < pA pB / 2)"),
    ("gadget", "n_lwe = 0", dict(n_lwe=0), -9, "fhe_tfhe_gadget_bootstrap_dev: n_lwe must be at least 1"),
    ("gadget", "empty batch", dict(batch=0, bsk=None, table=None, ksk=None, inp=None, out=None), 0, ""),
    ("gadget", "NULL", dict(ksk=None), -4, "fhe_tfhe_gadget_bootstrap_dev: NULL buffer"),
    ("gadget", "misaligned", dict(table=TAB + 8), -9, "d_table must be 16-byte aligned (got 0x200000000008)"),
    ("gadget", "out in the end of the table", dict(out=TAB + (K + 1) * N * 8 - 16), -9, "fhe_tfhe_gadget_bootstrap_dev: d_out overlaps an input"),
    ("gadget", "out in the end of the KSK", dict(out=KSK + KSK_BYTES - 16), -9, "fhe_tfhe_gadget_bootstrap_dev: d_out overlaps an input"),
    ("gadget", "both gadgets", dict(log_beta=0, ks_l=17), -9,
     "fhe_tfhe_gadget_bootstrap_dev: need 1 <= log_beta <= 64, l >= 1, log_beta l <= 64 (log_beta=0, l=3)"),
    ("gadget", "key-switch gadget and NULL", dict(ks_l=17, out=None), -9,
     "fhe_tfhe_gadget_bootstrap_dev: need 1 <= log_beta <= 32, l >= 1, log_beta l <= 64 (log_beta=4, l=17)"),
    ("gadget", "misaligned and overlapping", dict(inp=OUT + 8), -9, "d_in must be 16-byte aligned (got 0x500000000008)"),

    ("rows", "n_lwe = 0", dict(n_lwe=0), -9, "fhe_tfhe_gadget_bootstrap_rows_dev: n_lwe must be at least 1"),
    ("rows", "empty batch", dict(batch=0, table=None), 0, ""),
    ("rows", "NULL", dict(table=None), -4, "fhe_tfhe_gadget_bootstrap_rows_dev: NULL buffer"),
    ("rows", "misaligned", dict(table=TAB + 8), -9, "d_tables must be 16-byte aligned (got 0x200000000008)"),
    ("rows", "out in the end of the second table", dict(out=TAB + 2 * (K + 1) * N * 8 - 16), -9,
     "fhe_tfhe_gadget_bootstrap_rows_dev: d_out overlaps an input"),
    ("rows", "n_lwe and the key-switch gadget", dict(n_lwe=0, ks_l=0), -9, "fhe_tfhe_gadget_bootstrap_rows_dev: n_lwe must be at least 1"),
    ("rows", "NULL and overlapping", dict(ksk=None, out=IN), -4, "fhe_tfhe_gadget_bootstrap_rows_dev: NULL buffer"),

    ("gate", "k too large", dict(k=65), -9, "fhe_tfhe_gate_bootstrap_dev: need 1 <= k <= 64"),
    ("gate", "wires = 0", dict(wires=0), -9, "fhe_tfhe_gate_bootstrap_dev: need wires >= 1"),
    ("gate", "empty batch", dict(batch=0, pool=None, desc=None), 0, ""),
    ("gate", "batch past 32 bits", dict(batch=1 << 32), -9, "fhe_tfhe_gate_bootstrap_dev: batch too large"),
    ("gate", "batch past one launch", dict(batch=1 << 28), -9, "fhe_tfhe_gate_bootstrap_dev: batch too large"),
    ("gate", "out in the end of the descriptors", dict(out=DESC + 16), -9, "fhe_tfhe_gate_bootstrap_dev: d_out overlaps a key or the descriptors"),
    ("gate", "wires and the empty batch", dict(wires=0, batch=0), -9, "fhe_tfhe_gate_bootstrap_dev: need wires >= 1"),
    ("gate", "misaligned and too large", dict(desc=DESC + 4, batch=1 << 32), -9, "d_desc must be 16-byte aligned (got 0x700000000004)"),

    ("mux", "empty batch", dict(batch=0), 0, ""),
    ("mux", "NULL", dict(desc=None), -4, "fhe_tfhe_gate_mux_dev: NULL buffer"),
    ("mux", "misaligned", dict(ksk=KSK + 8), -9, "d_ksk must be 16-byte aligned (got 0x300000000008)"),
    ("mux", "two rows a gate: half the batch of a gate call", dict(batch=1 << 27), -9, "fhe_tfhe_gate_mux_dev: batch too large"),
    ("mux", "out in the end of the key", dict(out=BSK + BSK_BYTES - 16), -9, "fhe_tfhe_gate_mux_dev: d_out overlaps a key or the descriptors"),
    ("mux", "the key-switch gadget and wires", dict(ks_l=0, wires=0), -9,
     "fhe_tfhe_gate_mux_dev: need 1 <= log_beta <= 32, l >= 1, log_beta l <= 64 (log_beta=4, l=0)"),
    ("mux", "NULL and too large", dict(out=None, batch=1 << 32), -4, "fhe_tfhe_gate_mux_dev: NULL buffer"),
]

CASES += [
    ("lut", "t_bits = 0", dict(t=0), -9, "fhe_tfhe_lut_bootstrap_dev: need 1 <= t_bits <= log2 n (t_bits=0, n=1024)"),
    ("lut", "lut_count = 0", dict(lut_count=0), -9, "fhe_tfhe_lut_bootstrap_dev: need 1 <= lut_count < 2^32 (lut_count=0)"),
    ("lut", "empty batch", dict(batch=0), -9, "fhe_tfhe_lut_bootstrap_dev: need wires >= 1 and batch >= 1"),
    ("lut", "wires past 61 bits of bytes", dict(wires=1 << 60), -9, "fhe_tfhe_lut_bootstrap_dev: batch or wires too large"),
    ("lut", "NULL pool", dict(pool=None), -4, "fhe_tfhe_lut_bootstrap_dev: NULL buffer"),
    ("lut", "NULL tables", dict(luts=None), -4, "fhe_tfhe_lut_bootstrap_dev: NULL buffer"),
    ("lut", "misaligned key-switch key", dict(ksk=KSK + 8), -9, "d_ksk must be 16-byte aligned (got 0x300000000008)"),
    ("lut", "batch past one launch", dict(batch=1 << 28), -9, "fhe_tfhe_lut_bootstrap_dev: batch too large"),
    ("lut", "out in the end of the tables", dict(out=LUTS + 2 * 8 * 8 - 16), -9,
     "fhe_tfhe_lut_bootstrap_dev: d_out overlaps a key, the tables or the descriptors"),
    ("lut", "misaligned pool and NULL key", dict(pool=POOL + 8, ksk=None), -9, "d_pool must be 16-byte aligned (got 0x600000000008)"),
    ("lut", "NULL key and too large", dict(bsk=None, batch=1 << 28), -4, "fhe_tfhe_lut_bootstrap_dev: NULL buffer"),

    ("many", "t_bits past log2 n", dict(t=11), -9, "fhe_tfhe_lut_many_bootstrap_dev: need 1 <= t_bits <= log2 n (t_bits=11, n=1024)"),
    ("many", "nu past 4", dict(nu=5), -9, "fhe_tfhe_lut_many_bootstrap_dev: need nu <= min(log2 n - t_bits, 4) (nu=5, t_bits=3, n=1024)"),
    ("many", "nu past log2 n - t_bits", dict(t=8, nu=3), -9,
     "fhe_tfhe_lut_many_bootstrap_dev: need nu <= min(log2 n - t_bits, 4) (nu=3, t_bits=8, n=1024)"),
    ("many", "NULL key", dict(bsk=None), -4, "fhe_tfhe_lut_many_bootstrap_dev: NULL buffer"),
    ("many", "misaligned tables", dict(luts=LUTS + 8), -9, "d_luts must be 16-byte aligned (got 0x800000000008)"),
    ("many", "F batch rows past 32 bits", dict(nu=4, batch=1 << 28, n_lwe=1), -9, "fhe_tfhe_lut_many_bootstrap_dev: batch too large"),
    ("many", "the second function's slice of out on the descriptors", dict(out=DESC - 2 * ROW8 - 16), -9,
     "fhe_tfhe_lut_many_bootstrap_dev: d_out overlaps a key, the tables or the descriptors"),
    ("many", "nu and lut_count", dict(nu=5, lut_count=0), -9,
     "fhe_tfhe_lut_many_bootstrap_dev: need nu <= min(log2 n - t_bits, 4) (nu=5, t_bits=3, n=1024)"),
    ("many", "lut_count and the empty batch", dict(lut_count=0, batch=0), -9, "fhe_tfhe_lut_many_bootstrap_dev: need 1 <= lut_count < 2^32 (lut_count=0)"),

    ("cb", "private key-switch gadget", dict(pf_log_beta=33, pf_l=1), -9,
     "fhe_tfhe_circuit_bootstrap_dev: no private functional key switch for n=1024, k=1, log_beta=33, l=1 (needs k = 1, "
     "256 <= n <= 4096, 1 <= log_beta <= 32, l >= 1, log_beta l <= 64)"),
    ("cb", "alpha of the last level", dict(cb_log_beta=1, cb_l=64), -9,
     "fhe_tfhe_circuit_bootstrap_dev: need cb_log_beta cb_l <= 63 (alpha = g / 2 of the last level must be a word)"),
    ("cb", "empty batch", dict(batch=0, inp=None), 0, ""),
    ("cb", "NULL", dict(pfksk=None), -4, "fhe_tfhe_circuit_bootstrap_dev: NULL buffer"),
    ("cb", "misaligned", dict(pfksk=KSK + 8), -9, "d_pfksk must be 16-byte aligned (got 0x300000000008)"),
    ("cb", "batch past 32 bits", dict(batch=1 << 32), -9, "fhe_tfhe_circuit_bootstrap_dev: batch too large"),
    ("cb", "out in the end of the private key", dict(out=KSK + PFKSK_BYTES - 16), -9, "fhe_tfhe_circuit_bootstrap_dev: d_out overlaps an input"),
    ("cb", "the end of out (batch l_cb TGGSW rows) in the input", dict(out=IN - 2 * 3 * 2 * 2 * N * 8 + 16), -9,
     "fhe_tfhe_circuit_bootstrap_dev: d_out overlaps an input"),
    ("cb", "both later gadgets", dict(cb_l=0, pf_l=0), -9,
     "fhe_tfhe_circuit_bootstrap_dev: need 1 <= log_beta <= 64, l >= 1, log_beta l <= 64 (log_beta=4, l=0)"),
    ("cb", "alpha and NULL", dict(cb_log_beta=1, cb_l=64, out=None), -9,
     "fhe_tfhe_circuit_bootstrap_dev: need cb_log_beta cb_l <= 63 (alpha = g / 2 of the last level must be a word)"),

    ("ks", "n_in = 0", dict(n_in=0), -9, "fhe_tlwe_key_switch_dev: need n_in, n_out >= 1"),
    ("ks", "l = 65", dict(l=65), -9, "fhe_tlwe_key_switch_dev: need 1 <= l <= 64"),
    ("ks", "empty batch", dict(batch=0, ksk=None, inp=None, out=None), 0, ""),
    ("ks", "NULL", dict(inp=None), -4, "fhe_tlwe_key_switch_dev: NULL buffer"),
    ("ks", "misaligned", dict(out=OUT + 8), -9, "d_out must be 16-byte aligned (got 0x500000000008)"),
    ("ks", "out in the end of the key", dict(out=KSK + N * 64 * ROW8 - 16), -9, "fhe_tlwe_key_switch_dev: d_out overlaps an input"),
    ("ks", "2^32 tiles", HUGE_KS, -9, "fhe_tlwe_key_switch_dev: batch too large for one launch"),
    ("ks", "beta and l", dict(beta=3, l=0), -9, "fhe_tlwe_key_switch_dev: only beta = 2 is supported (torus.rs:44)"),
    ("ks", "overlapping and 2^32 tiles", dict(HUGE_KS, inp=16), -9, "fhe_tlwe_key_switch_dev: d_out overlaps an input"),

    ("gks", "log_beta l = 68", dict(l=17), -9,
     "fhe_tlwe_gadget_key_switch_dev: need 1 <= log_beta <= 32, l >= 1, log_beta l <= 64 (log_beta=4, l=17)"),
    ("gks", "empty batch", dict(batch=0, ksk=None, inp=None, out=None), 0, ""),
    ("gks", "NULL", dict(ksk=None), -4, "fhe_tlwe_gadget_key_switch_dev: NULL buffer"),
    ("gks", "misaligned", dict(ksk=KSK + 4), -9, "d_ksk must be 16-byte aligned (got 0x300000000004)"),
    ("gks", "the end of out in the input", dict(out=IN - 2 * ROW8 + 16), -9, "fhe_tlwe_gadget_key_switch_dev: d_out overlaps an input"),
    ("gks", "2^32 tiles", HUGE_KS, -9, "fhe_tlwe_gadget_key_switch_dev: batch too large for one launch"),
    ("gks", "n_out and the gadget", dict(n_out=0, log_beta=0), -9, "fhe_tlwe_gadget_key_switch_dev: need n_in, n_out >= 1"),
    ("gks", "the gadget and the empty batch", dict(log_beta=33, batch=0), -9,
     "fhe_tlwe_gadget_key_switch_dev: need 1 <= log_beta <= 32, l >= 1, log_beta l <= 64 (log_beta=33, l=4)"),
]

assert len(CASES) <= 80 and len({c[:2] for c in CASES}) == len(CASES)


def run_case(L, entry, change):
    """(return code, last error) of one call; the message of a call that succeeds is not looked at"""
    name, base = ENTRY[entry]
    assert set(change) <= set(base), (entry, change)
    rc = getattr(L, name)(*dict(base, **change).values())
    return rc, (L.fhe_last_error().decode() if rc else "")


@pytest.mark.parametrize("entry", list(ENTRY))
def test_tfhe_entry_point_errors_and_their_order(pkg, entry):
    L = pkg.load_library()
    rows = [c for c in CASES if c[0] == entry]
    got = [(what, *run_case(L, entry, change)) for _, what, change, _, _ in rows]
    assert got == [(what, rc, msg) for _, what, _, rc, msg in rows]
