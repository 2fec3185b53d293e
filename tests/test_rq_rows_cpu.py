"""The launch classes of the R_q row surfaces of csrc/glue.hip (rows N3 / N4 of include/fhe_ntt.h), enumerated without
a device: a Python restatement of the host's rules (which arithmetic a plan runs, which route a key switch takes and how
it is split), the class of a call, the universe of classes an admitted shape can reach on the batch ladder, and the case
lists that tests/test_rq_rows_gpu.py runs.  The restatement only plans the sweep: every comparison of the sweep is against
an independent reference whatever the split really is, and the batch ladder has both sides of every power-of-two
threshold a split can have.  The module also pins the two references against each other: tests/_rq_rows_numpy.py (Python
integers, no NTT) and oracle.glue (products through the oracle's NTT)."""
import functools
import math
import random

import numpy as np
import pytest

import _rq_rows_numpy as P
from conftest import Q16, Q61
from test_parity_gpu import _prime_below

# ---- moduli: one per arithmetic class, at the top of its range ----------------------------------------------------------
SHOUP62, SHOUP61, PMERSENNE, WORD32, STRICT63, MONTGOMERY = 0, 1, 2, 3, 4, 5      # include/fhe_ntt.h:115-120
ARITH_NAMES = {SHOUP62: "shoup62", SHOUP61: "shoup61", PMERSENNE: "pmersenne", WORD32: "word32", STRICT63: "strict63", MONTGOMERY: "montgomery"}
Q12289 = 12289                                          # 3 2^12 + 1: n <= 2048
Q30 = _prime_below(1 << 30, 1 << 17)                    # WORD32 at its top
Q61S = _prime_below((1 << 61) - (1 << 23), 1 << 17)     # 61 bits, 2^61 - q > 2^22: no pseudo-Mersenne form, a plain Shoup-61 prime
QMG = _prime_below(1 << 61, 1 << 32)                    # q = 1 (mod 2^32)
Q62 = _prime_below(1 << 62, 1 << 17)
Q63 = _prime_below(1 << 63, 1 << 17)
MODULI = (Q16, Q12289, Q30, Q61S, Q61, QMG, Q62, Q63)
SIZES = (2, 16, 256, 512, 1024, 2048, 4096, 8192, 16384)
# 1 .. 9 and both sides of every power-of-two threshold 16 .. 2048
LADDER = tuple(sorted(set(range(1, 10)) | {t + d for t in (16, 32, 64, 128, 256, 512, 1024, 2048) for d in (-1, 0, 1)}))
KEYS = ("coeffs", "evals", "prepared")
WS_CAP = 1 << 34                                        # bytes of workspace a sweep case may ask for (the ladder's top at n = 4096, l = 64: 9 GB)


def has_plan(q, n):
    """a negacyclic transform of size n exists modulo the prime q"""
    return (q - 1) % (2 * n) == 0


# ---- the host's rules, restated -------------------------------------------------------------------------------------------

def pm_form(q):
    """capi.hip:135-139: q = 2^k - delta with 56 <= k <= 61 and delta <= 2^(k-39)"""
    k = q.bit_length()
    return 56 <= k <= 61 and (1 << k) - q <= 1 << (k - 39)


def smallq(q, n):
    """smallq.hip:642-644 smallq_supported; capi.hip:996-997 fhe_smallq_args takes the 32-bit transforms exactly there
    (the 32-bit tables exist, capi.hip:284) unless FHE_EXT32=0"""
    return q >= 3 and q % 2 == 1 and q < 1 << 30 and 8 <= n.bit_length() - 1 <= 18


def arithmetic(q, n):
    """capi.hip:391-398 fhe_ntt_plan_arithmetic with FHE_EXT32, FHE_PM, FHE_MG at their defaults"""
    lg = n.bit_length() - 1
    if smallq(q, n):
        return WORD32
    if pm_form(q):
        return PMERSENNE
    if q & 0xFFFFFFFF == 1 and q >> 32 and q < 1 << 61 and not pm_form(q) and lg >= 4:      # capi.hip:154, :395
        return MONTGOMERY
    if q >> 62:
        return STRICT63
    return SHOUP61 if q < 1 << 61 else SHOUP62


def decompose_args_ok(q, beta, l):
    """glue.hip:269-283 check_decompose_args"""
    if beta < 2 or l < 1:
        return False
    if beta == 2:
        return l <= 64
    return beta ** l < 1 << 32 and q // beta ** l > 0


def ks32_usable(q, n, k, beta, l):
    """glue.hip:403-405 ks32_usable with digit32.hip:624-628 ks32_shape_supported"""
    return beta == 2 and q < 1 << 61 and k == 1 and 1 <= l <= 64 and 256 <= n <= 4096 and k * l * n <= 1 << 21


def ext32_units(lg):
    """digit32.hip:636"""
    return (2 if lg == 12 else 4096 >> lg) if 8 <= lg <= 12 else 0


def dm_units(lg, nc):
    """digit_mac.hip:298-303"""
    if lg < 8 or lg > 12 or nc < 2 or nc > 4 or nc * ((1 << lg) // 256) > 16:
        return 0
    return 4096 >> lg


def _split(batch, T, W, slots):
    """the loop of glue.hip:418-420 and digit_mac.hip:309-310, and the tpp of glue.hip:436 / digit_mac.hip:325"""
    parts = 1
    while parts < 8 and batch * parts < slots and T // (parts * 2) >= 2 * W:
        parts *= 2
    return parts, -(-(-(-T // parts)) // W) * W


def ks32_split(n, batch, T):
    """glue.hip:414-436: slots 512, 256 at n = 4096 (not ext32_split's 2048 / 512 / 256)"""
    lg = n.bit_length() - 1
    return _split(batch, T, ext32_units(lg), 256 if lg == 12 else 512)


def digit_mac_split(n, batch, T, nc):
    """digit_mac.hip:305-312 digit_mac_parts (batch * parts < 2048)"""
    return _split(batch, T, dm_units(n.bit_length() - 1, nc), 2048)


def prepared_words(q, n, k, beta, l):
    """glue.hip:535-547 fhe_glwe_ksk_prepared_words"""
    if k == 0 or not decompose_args_ok(q, beta, l):
        return 0
    return (2 if ks32_usable(q, n, k, beta, l) else 1) * k * l * (k + 1) * n


def ks_route(q, n, k, beta, l, key):
    """the route of fhe_glwe_key_switch_dev (glue.hip:444-526) and fhe_glwe_key_switch_prepared_dev (:566-578).
    ks32: two 27-bit primes (:464, :577).  fused61: digit_mac_zq + digit_tail_ks (:467-478; launch_digit_tail_ks cannot
    refuse inside that condition, so the sum_parts fallback of :481-488 is unreachable through this entry point and is
    not a route here).  generic: `zqbits` (launch_ntt_forward_zqbits, ntt_kernels.hip:1102: base 2, 2^4 <= n <= 2^13,
    q < 2^61) or `decompose`, then mac_rows, then the fused tail at 2^8 .. 2^12 with q < 2^61 (:513) or ks_tail."""
    lg = n.bit_length() - 1
    wide = q < 1 << 61
    if key != "evals" and ks32_usable(q, n, k, beta, l):
        return "ks32"
    if beta == 2 and wide and 8 <= lg <= 12 and k + 1 in (2, 3) and dm_units(lg, k + 1):
        return "fused61"
    dec = "zqbits" if beta == 2 and 4 <= lg <= 13 and wide else "decompose"
    return "generic-%s-%s" % (dec, "tail" if wide and 8 <= lg <= 12 else "kstail")


def ks_shape(q, n, k, beta, l, batch, key):
    route = ks_route(q, n, k, beta, l, key)
    lg, T = n.bit_length() - 1, k * l
    if route == "ks32":
        W, (parts, tpp) = ext32_units(lg), ks32_split(n, batch, T)
    elif route == "fused61":
        W, (parts, tpp) = dm_units(lg, k + 1), digit_mac_split(n, batch, T, k + 1)
    else:
        W, parts, tpp = 0, 1, T
    return dict(route=route, W=W, T=T, parts=parts, tpp=tpp, last=T - (parts - 1) * tpp)


def size_bucket(n):
    lg = n.bit_length() - 1
    return 0 if lg < 4 else 1 if lg < 8 else 2 if lg <= 12 else 3 if lg == 13 else 4


def ks_class(q, n, k, beta, l, batch, key):
    """(route, arithmetic, size bucket, k {1, 2, >= 3}, beta > 2, parts, T a whole number of steps, last part
    full / short / empty, T < W, key form); the last four are False / "full" where the route has no split"""
    s = ks_shape(q, n, k, beta, l, batch, key)
    W = s["W"]
    last = "full" if s["last"] == s["tpp"] else "empty" if s["last"] <= 0 else "short"
    return (s["route"], arithmetic(q, n), size_bucket(n), min(k, 3), beta > 2, s["parts"], W == 0 or s["T"] % W == 0, last,
            W != 0 and s["T"] < W, key)


def ks_workspace(q, n, k, l, batch):
    """an upper bound of the bytes a call asks of workspace slot 1 (the generic route, glue.hip:494) plus its operands"""
    T, k1 = k * l, k + 1
    return (2 * batch * T + 3 * batch * k1 + 2 * T * k1) * n * 8


KS_K = (1, 2, 3)
KS_BL = tuple((2, l) for l in (1, 2, 5, 16, 33, 64)) + ((4, 2), (4, 6))


def ks_admitted(q, n, k, beta, l, batch):
    return has_plan(q, n) and decompose_args_ok(q, beta, l) and ks_workspace(q, n, k, l, batch) <= WS_CAP


def ks_classes_of(q, n, k, beta, l, batch):
    return {ks_class(q, n, k, beta, l, batch, key) for key in KEYS}        # every case runs the three key forms


@functools.lru_cache(None)
def ks_universe():
    """class -> the (q, n, k, beta, l, batch) that reach it"""
    out = {}
    for q in MODULI:
        for n in SIZES:
            for k in KS_K:
                for beta, l in KS_BL:
                    for batch in LADDER:
                        if ks_admitted(q, n, k, beta, l, batch):
                            for c in ks_classes_of(q, n, k, beta, l, batch):
                                out.setdefault(c, []).append((q, n, k, beta, l, batch))
    return out


def _ks_cost(n, k, l):
    return n * k * l * (k + 1)                                     # the reference: k l (k+1) products of n words


@functools.lru_cache(None)
def _ks_cover():
    """a greedy cover of the universe: the (q, n, k, beta, l) that reaches the most uncovered classes per unit of
    reference cost, then the ladder batches of it that each add a class -> [((q, n, k, beta, l), [batch ...])]"""
    shapes = {}
    for c, reach in ks_universe().items():
        for q, n, k, beta, l, batch in reach:
            shapes.setdefault((q, n, k, beta, l), {}).setdefault(batch, set()).add(c)
    need, out = set(ks_universe()), []
    while need:
        best = max(shapes, key=lambda s: (len(set().union(*shapes[s].values()) & need) / _ks_cost(s[1], s[2], s[4]), s))
        batches, got = [], set()
        for batch in sorted(shapes[best]):
            new = (shapes[best][batch] & need) - got
            if new:
                got |= new
                batches.append(batch)
        assert got
        need -= got
        out.append((best, batches))
        del shapes[best]
    return out


def _ks_cases():
    """the cover, plus the whole ladder once per split route and ring size at the deepest digit count (l = 64: every
    `parts` the rule has), so that both sides of every threshold run even if a restated threshold were off"""
    out = [(s + (batch,)) for s, batches in _ks_cover() for batch in batches]
    for n in (256, 512, 1024, 2048, 4096):
        out += [(Q61, n, 1, 2, 64, batch) for batch in LADDER]                          # ks32
        if n <= 2048:
            out += [(Q61, n, 2 if n <= 1024 else 1, 2, 64, batch) for batch in LADDER]  # fused61 (k = 1: the evals key form)
    seen, uniq = set(), []
    for c in out:
        if c not in seen and ks_admitted(*c):
            seen.add(c)
            uniq.append(c)
    return uniq


KS_CASES = _ks_cases()

# ---- the mac_rows surfaces --------------------------------------------------------------------------------------------------
MAC_SIZES = (2, 16, 256, 4096, 8192, 16384)
ENTRIES = ("tr_dot", "tr_mul_r", "glev_mul")


def mac_chunk(q, n):
    """zq_device.hpp:525, :541: 128-bit accumulators folded every 8 terms, every 2 at 2^62 <= q (mac_kernel.hpp:68-72)"""
    return 2 if arithmetic(q, n) == STRICT63 else 8


def mac_shapes(q, n):
    """(entry, T, nc) of the sweep at (q, n): tr_dot (T = k, nc = 1), tr_mul_r (T = 1, nc = rows), glev_mul (T = l,
    nc = k + 1) with T below, at and above the fold chunk (not a multiple of it) and nc odd and even"""
    ch = mac_chunk(q, n)
    ts = (ch - 1, ch, ch + 3)
    return [("tr_dot", t, 1) for t in ts] + [("tr_mul_r", 1, r) for r in (2, 3)] + [("glev_mul", t, nc) for t in ts for nc in (2, 3)]


def mac_class(q, n, entry, T, nc, flags):
    ch = mac_chunk(q, n)
    rel = "below" if T < ch else "chunk" if T == ch else "multiple" if T % ch == 0 else "above"
    return (entry, arithmetic(q, n), size_bucket(n), nc % 2 == 1, rel, ch, flags)


@functools.lru_cache(None)
def mac_universe():
    """every class an admitted (q, n) reaches; what no shape reaches is not in it: tr_dot has one output row (nc odd
    only), tr_mul_r has T = 1 (below the chunk only), WORD32 needs n >= 256 and Montgomery n >= 16, 12289 ends at
    n = 2048, and a chunk of 2 belongs to strict-63 alone"""
    out = {}
    for q in MODULI:
        for n in MAC_SIZES:
            if has_plan(q, n):
                for entry, T, nc in mac_shapes(q, n):
                    for flags in range(8):
                        out.setdefault(mac_class(q, n, entry, T, nc, flags), []).append((q, n, entry, T, nc))
    return out


def _mac_cases():
    """(q, n, entry, T, nc), each run with the eight flag combinations: every shape of every (q, n) that has a plan (a
    class names the size bucket, and the transforms differ by n inside a bucket)"""
    return [(q, n, entry, T, nc) for q in MODULI for n in MAC_SIZES if has_plan(q, n) for entry, T, nc in mac_shapes(q, n)]


MAC_CASES = _mac_cases()
# the top modulus of each arithmetic class and the n at which the closed forms of the worst-case rows are asserted
WORST = [(Q30, 1024), (Q61S, 1024), (Q61, 1024), (QMG, 1024), (Q62, 1024), (Q63, 1024), (Q63, 8)]


# ---- tests ---------------------------------------------------------------------------------------------------------------------

def test_each_modulus_is_the_arithmetic_class_intended(pkg):
    want = {Q16: WORD32, Q12289: WORD32, Q30: WORD32, Q61S: SHOUP61, Q61: PMERSENNE, QMG: MONTGOMERY, Q62: SHOUP62, Q63: STRICT63}
    assert (1 << 29) < Q30 < (1 << 30) and (1 << 60) < Q61S < (1 << 61) and (1 << 60) < QMG < (1 << 61) and QMG % (1 << 32) == 1
    assert (1 << 61) < Q62 < (1 << 62) and (1 << 62) < Q63 < (1 << 63) and Q63 == 9223372036844421121
    for q, ar in want.items():
        for n in SIZES:
            if not has_plan(q, n):
                continue
            got = pkg.Plan(q, n).arithmetic()
            assert got == arithmetic(q, n), (q, n, got)
            # below 2^8 a small modulus runs the Shoup-61 kernels, and below 2^4 a Montgomery prime does
            expect = SHOUP61 if (ar == WORD32 and n < 256) or (ar == MONTGOMERY and n < 16) else ar
            assert got == expect, (q, n, ARITH_NAMES[got])
    assert not has_plan(Q12289, 4096) and has_plan(Q12289, 2048)


def test_prepared_words_double_exactly_where_the_two_prime_route_applies(pkg):
    L = pkg.load_library()
    doubled = 0
    for q in MODULI:
        for n in SIZES:
            if not has_plan(q, n):
                continue
            plan = pkg.Plan(q, n)
            for k in KS_K:
                for beta, l in KS_BL + ((2, 65), (4, 16), (3, 1), (2, 0)):
                    got = L.fhe_glwe_ksk_prepared_words(plan.handle, k, beta, l)
                    assert got == prepared_words(q, n, k, beta, l), (q, n, k, beta, l, got)
                    doubled += got == 2 * k * l * (k + 1) * n
    assert doubled >= 100


@pytest.mark.parametrize("n,batch,T,want", [
    # the loop doubles p while batch p < slots, so parts = 8 holds while 4 batch < slots
    (2048, 1, 33, (8, 6)), (2048, 127, 33, (8, 6)), (2048, 128, 33, (4, 10)),   # parts 6 and 7 own no digit below batch 128
    (4096, 1, 64, (8, 8)), (4096, 63, 64, (8, 8)), (4096, 64, 64, (4, 16)), (4096, 127, 64, (4, 16)), (4096, 128, 64, (2, 32)),
    (4096, 255, 64, (2, 32)), (4096, 256, 64, (1, 64)), (1024, 1, 64, (8, 8)), (1024, 127, 64, (8, 8)), (1024, 128, 64, (4, 16)),
    (1024, 256, 64, (2, 32)), (1024, 511, 64, (2, 32)), (1024, 512, 64, (1, 64)),
    (256, 1, 64, (2, 32)), (256, 1, 63, (1, 64)), (512, 1, 5, (1, 8)),
])
def test_the_restated_two_prime_split_at_known_points(n, batch, T, want):
    assert ks32_split(n, batch, T) == want


def test_the_key_switch_case_list_leaves_out_no_class_of_the_universe():
    uni = ks_universe()
    covered = set()
    for c in KS_CASES:
        assert ks_admitted(*c) and c[5] in LADDER
        covered |= ks_classes_of(*c)
    missing = sorted(set(uni) - covered)
    assert not missing, missing[:10]
    assert covered == set(uni)
    print("\nkey switch: %d classes, %d cases in %d shapes" % (len(uni), len(KS_CASES), len({c[:5] for c in KS_CASES})))
    routes = {c[0] for c in uni}
    assert routes == {"ks32", "fused61", "generic-zqbits-tail", "generic-zqbits-kstail", "generic-decompose-tail", "generic-decompose-kstail"}
    assert {c[1] for c in uni} == set(ARITH_NAMES) and {c[2] for c in uni} == {0, 1, 2, 3, 4} and {c[3] for c in uni} == {1, 2, 3}
    assert {c[5] for c in uni if c[0] == "ks32"} == {1, 2, 4, 8} == {c[5] for c in uni if c[0] == "fused61"}
    assert {c[7] for c in uni} == {"full", "short", "empty"} and {c[9] for c in uni} == set(KEYS)
    # the rows of the issue's table
    assert ks_shape(Q61, 2048, 1, 2, 33, 1, "coeffs") == dict(route="ks32", W=2, T=33, parts=8, tpp=6, last=-9)
    assert ks_class(Q61, 2048, 1, 2, 33, 1, "coeffs") in uni                                  # an empty last part
    assert ks_class(Q61, 4096, 1, 2, 64, 257, "coeffs")[:1] + ks_class(Q61, 4096, 1, 2, 64, 257, "coeffs")[5:6] == ("ks32", 1)
    assert ks_shape(Q61, 4096, 1, 2, 64, 257, "coeffs")["parts"] == 1 and (Q61, 4096, 1, 2, 64, 257) in KS_CASES   # parts = 1 at T = 64
    assert any(c[0] == "fused61" and c[1] == WORD32 and c[3] == 2 for c in uni)              # a WORD32 plan with k = 2
    assert any(c[1] == MONTGOMERY for c in uni)
    assert ks_route(Q62, 1024, 1, 2, 16, "coeffs") == "generic-decompose-kstail"             # SHOUP62 at n = 1024: not wide, no fused tail
    assert ks_class(Q62, 1024, 1, 2, 16, 1, "coeffs") in uni
    assert ks_route(Q61, 1024, 2, 4, 6, "coeffs") == "generic-decompose-tail" and ks_class(Q61, 1024, 2, 4, 6, 1, "coeffs") in uni
    assert ks_route(Q61, 16384, 2, 4, 6, "coeffs") == "generic-decompose-kstail" and ks_class(Q61, 16384, 2, 4, 6, 1, "coeffs") in uni
    assert ks_route(Q61, 4096, 1, 2, 16, "evals") == "generic-zqbits-tail"                   # dm_units(12, 2) = 0
    assert ks_route(Q61, 2048, 2, 2, 16, "coeffs") == "generic-zqbits-tail"                  # dm_units(11, 3) = 0
    assert ks_route(Q61, 8192, 1, 2, 16, "coeffs") == "generic-zqbits-kstail"


def test_the_mac_rows_case_list_leaves_out_no_class_of_the_universe():
    uni = mac_universe()
    covered = {mac_class(q, n, entry, T, nc, flags) for q, n, entry, T, nc in MAC_CASES for flags in range(8)}
    assert covered == set(uni)
    print("\nmac_rows surfaces: %d classes, %d cases x 8 flag combinations" % (len(uni), len(MAC_CASES)))
    assert {c[0] for c in uni} == set(ENTRIES) and {c[1] for c in uni} == set(ARITH_NAMES) and {c[2] for c in uni} == {0, 1, 2, 3, 4}
    assert {c[3] for c in uni} == {False, True} and {c[4] for c in uni} == {"below", "chunk", "above"} and {c[5] for c in uni} == {2, 8}
    for ar in ARITH_NAMES:                                             # flags on every arithmetic, WORD32 and Montgomery included
        assert {c[6] for c in uni if c[1] == ar} == set(range(8)), ar
    for q, n in WORST:
        assert has_plan(q, n)
    assert {arithmetic(q, n) for q, n in WORST} == set(ARITH_NAMES)


# ---- the two references agree ------------------------------------------------------------------------------------------------

def _rows(rng, q, shape):
    a = rng.integers(0, q, shape, dtype=np.uint64)
    flat = a.reshape(-1)
    m = min(4, flat.size)
    flat[:m] = [0, 1, q - 1, q // 2][:m]
    return a


def test_the_packed_product_is_the_schoolbook_product():
    rng = np.random.default_rng(11)
    for q in (17, Q16, Q61, Q63):
        for n in (1, 2, 8, 64):
            for a, b in ((_rows(rng, q, n), _rows(rng, q, n)), (np.full(n, q - 1, dtype=np.uint64),) * 2):
                assert P.rq_mul(q, a, b) == P.rq_mul_schoolbook(q, a, b), (q, n)


@pytest.mark.parametrize("q,n,k,beta,l", [(Q16, 8, 3, 2, 16), (Q16, 256, 1, 2, 17), (Q12289, 64, 2, 4, 6), (Q61S, 16, 2, 2, 64), (Q61, 256, 1, 4, 6),
                                          (QMG, 32, 1, 2, 33), (Q62, 64, 2, 2, 5), (Q63, 128, 2, 2, 64), (Q63, 2, 1, 4, 15), (Q30, 256, 2, 2, 30)])
def test_the_python_reference_and_the_oracle_agree(oracle, q, n, k, beta, l):
    rng = np.random.default_rng(n + l)
    a, b = _rows(rng, q, (k, n)), _rows(rng, q, (k, n))
    p = _rows(rng, q, n)
    out = np.empty(n, dtype=np.uint64)
    oracle.glue("tr_dot", q, n, k, a, b, out)
    assert out.tolist() == P.tr_dot(q, a, b)
    outk = np.empty((k, n), dtype=np.uint64)
    oracle.glue("tr_mul_r", q, n, k, a, p, outk)
    assert outk.tolist() == P.tr_mul_r(q, a, p)
    glev, v = _rows(rng, q, (l, k + 1, n)), _rows(rng, q, (l, n))
    outg = np.empty((k + 1, n), dtype=np.uint64)
    oracle.glue("glev_mul", q, n, k, l, glev, v, outg)
    assert outg.tolist() == P.glev_mul(q, glev, v)
    ksk = _rows(rng, q, (k, l, k + 1, n))
    for glwe in (_rows(rng, q, (k + 1, n)), np.full((k + 1, n), q - 1, dtype=np.uint64)):
        glwe.reshape(-1)[4:8] = [min(q - 1, (1 << min(l, 63)) - 1), min(q - 1, 1 << min(l, 63)), min(q - 1, beta ** l - 1), min(q - 1, beta ** l)][: max(0, min(4, glwe.size - 4))]
        oracle.glue("key_switch", q, n, k, beta, l, glwe, ksk, outg)
        assert outg.tolist() == P.key_switch(q, k, beta, l, glwe, ksk)
        dec = np.empty((l, n), dtype=np.uint64)
        oracle.glue("rq_decompose", q, n, glwe[0], beta, l, dec)
        assert dec.tolist() == P.rq_decompose(q, glwe[0], beta, l)


@pytest.mark.parametrize("q,n", WORST + [(Q16, 256)])
def test_closed_forms_of_the_worst_case_rows_on_the_references(oracle, q, n):
    """(i) every operand word q - 1: (-(1 + X + .. + X^(n-1)))^2 in X^n + 1 has coefficient j equal to 2 j + 2 - n.
    (ii) operands whose transforms are q - 1 in every word (what the device is given with all three flags set): the
    transform of the reference's result is T mod q in every word"""
    k, l = 3, 5
    sq = [(2 * j + 2 - n) for j in range(n)]
    full = np.full((l, k + 1, n), q - 1, dtype=np.uint64)
    out = np.empty(n, dtype=np.uint64)
    oracle.glue("tr_dot", q, n, k, full[0, :k], full[0, :k], out)
    assert out.tolist() == [k * s % q for s in sq]
    outk = np.empty((k, n), dtype=np.uint64)
    oracle.glue("tr_mul_r", q, n, k, full[0, :k], full[0, 0], outk)
    assert outk.tolist() == [[s % q for s in sq]] * k
    outg = np.empty((k + 1, n), dtype=np.uint64)
    oracle.glue("glev_mul", q, n, k, l, full, full[:, 0], outg)
    assert outg.tolist() == [[l * s % q for s in sq]] * (k + 1)
    if n <= 256:
        assert P.tr_dot(q, full[0, :k], full[0, :k]) == out.tolist() and P.glev_mul(q, full, full[:, 0]) == outg.tolist()
        assert P.tr_mul_r(q, full[0, :k], full[0, 0]) == outk.tolist()
    # key switch, base 2 with l = 64: every digit saturates to 1 against a q - 1 key (the opposite sign)
    for kk in (1, 2):
        ksk = np.full((kk, 64, kk + 1, n), q - 1, dtype=np.uint64)
        glwe = np.full((kk + 1, n), q - 1, dtype=np.uint64)
        out2 = np.empty((kk + 1, n), dtype=np.uint64)
        oracle.glue("key_switch", q, n, kk, 2, 64, glwe, ksk, out2)
        assert out2.tolist() == ks_worst_closed(q, n, kk, 64)
        if n <= 16:
            assert P.key_switch(q, kk, 2, 64, glwe, ksk) == out2.tolist()
    # (ii): the coefficient row whose transform is q - 1 throughout
    row = oracle.intt(q, n, np.full(n, q - 1, dtype=np.uint64))
    assert oracle.ntt(q, n, row).tolist() == [q - 1] * n
    for T in (5, 33):
        a = np.ascontiguousarray(np.broadcast_to(row, (T, n)))
        oracle.glue("tr_dot", q, n, T, a, a, out)
        assert oracle.ntt(q, n, out).tolist() == [T % q] * n
        g = np.ascontiguousarray(np.broadcast_to(row, (T, 2, n)))
        out2 = np.empty((2, n), dtype=np.uint64)
        oracle.glue("glev_mul", q, n, 1, T, g, a, out2)
        assert oracle.ntt(q, n, out2).tolist() == [[T % q] * n] * 2
        if n <= 16:
            assert P.tr_dot(q, a, a) == out.tolist() and P.glev_mul(q, g, a) == out2.tolist()
    oracle.glue("tr_mul_r", q, n, 2, a[:2], row, out2)
    assert oracle.ntt(q, n, out2).tolist() == [[1] * n] * 2


def ks_worst_closed(q, n, k, l):
    """(c < k ? 0 : q - 1) - k l (n - 2 - 2 j) mod q"""
    rhs = [k * l * (n - 2 - 2 * j) for j in range(n)]
    return [[(0 - r) % q for r in rhs]] * k + [[(q - 1 - r) % q for r in rhs]]


# ---- the f64 rows ----------------------------------------------------------------------------------------------------------------

def f64_inputs(q, extra=()):
    """canonical words where a conversion or a rounding can go wrong: the ends, 2^53 and its neighbours (the first
    integers `as f64` rounds), ties of every call below, and the largest canonical word"""
    w = {0, 1, 2, 3, q // 2, q // 2 + 1, q - 2, q - 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 2, (1 << 53) + 3, (1 << 62) + 1, (1 << 60) + 65}
    w |= set(extra)
    return sorted(x for x in w if 0 <= x < q)


def float_ties(q, num, den, want=12):
    """canonical v whose quotient (float(num) * float(v)) / float(den) IS x.5 as a double, whether or not num v / den is
    a tie in exact integers: v = floor and ceil of (2 m + 1) den / (2 num) for small m, m around every power of two and
    m drawn over the whole range of the quotient -> (those with x even, those with x odd), at most `want` of each.
    `round` and `rint` part on the even ones."""
    rnd = random.Random(num % 1000003 + den % 1000003)
    top = min(num * (q - 1) // den, (1 << 51) - 1)                  # x.5 is no double from 2^52 on
    ms = list(range(40)) + [(1 << j) + i for j in range(5, 51) for i in range(4)] + [rnd.randrange(top + 1) for _ in range(4000)]
    even, odd = set(), set()
    nf, df = float(num), float(den)
    for m in ms:
        if m > top:
            continue
        c = (2 * m + 1) * den // (2 * num)
        for v in (c, c + 1):
            if 0 <= v < q and (nf * float(v)) / df == m + 0.5:
                side = odd if m & 1 else even
                if len(side) < want:
                    side.add(v)
    return even, odd


def tie_words(q, num, den):
    """the words of float_ties and their neighbours on either side"""
    even, odd = float_ties(q, num, den)
    return {v + d for v in even | odd for d in (-1, 0, 1) if 0 <= v + d < q}


def no_float_tie(q, num, den):
    """the argument pairs of this module at which no canonical v gives a quotient of x.5, each for a reason that is
    asserted by test_every_f64_argument_pair_has_ties_of_both_parities finding none:
    den = 1 and float(num) / float(den) a whole number (3 q over q at 2^61 - 2^21 + 1: both convert exactly): whole quotients;
    num / den = 2 / 3 and 1 / 3: 4 v = 3 (2 m + 1) and 2 v = 3 (2 m + 1) miss by at least 1 / 6;
    num = q - 2 over q: v - 2 v / q is half-way only near v = q / 4, where the quotient is past 2^52;
    den >= 2^63 with num = 1: v / den stays below 1 / 2 (v = 2^62 over 2^63 is the one tie, at a 63-bit q: x = 0 only);
    q = 65537: num v / q misses x.5 by at least 1 / (2 q), far more than a double's spacing below num q"""
    if q < 1 << 32 and den == q:
        return True
    if den == 1 or (num, den) in ((2, 3), (1, 3)) or (den == q and num in (q - 2, 3 * q)) or (num == 1 and den >= 1 << 63):
        return True
    return num == 1 and den > 2 * q


F64_Q = (Q16, Q61, Q63)


def mul_div_pairs(q):
    return [(2, q), (16, q), (1, 1 << 20), (2, 3), (q - 1, 1), (1, 2), (3, 2), (1, 6)]


def mod_switch_ps(q):
    return [2, 1 << 10, 1 << 20, q - 2, 3, min(3 * q, (1 << 63) - 1), (1 << 64) - 1]


DIV_ROUND_S = (1, 2, 3, 1000, 12345677, 1 << 63, (1 << 64) - 1)


def mul_f64_factors(q):
    v = q - 1
    return [0.0, 0.5, -0.5, 1.0, 1.0 - 2.0 ** -53, 2.0 ** 10 + 2.0 ** -42, -2.5, 0.333, 1e6, -1e30, 1e30, 2.0 ** 63 / float(v), -(2.0 ** 63) / float(v),
            float("nan"), float("inf"), float("-inf")]


def f64_pairs(q):
    """every (num, den) whose quotient a kernel of the f64 rows rounds: mul_div_round's pairs, (p, q) of mod_switch and
    (1, s) of div_round"""
    t = 65537 if q != Q16 else 17
    return mul_div_pairs(q) + [(t, q)] + [(p, q) for p in mod_switch_ps(q)] + [(1, s) for s in DIV_ROUND_S]


def test_every_f64_argument_pair_has_ties_of_both_parities():
    for q in F64_Q:
        for num, den in f64_pairs(q):
            even, odd = float_ties(q, num, den)
            for v in even | odd:
                x = (float(num) * float(v)) / float(den)
                assert x - math.floor(x) == 0.5 and (math.floor(x) % 2 == 0) == (v in even)
                assert P.rust_round(x) == math.floor(x) + 1
            if no_float_tie(q, num, den):
                assert not odd and (not even or (q, num, den) == (Q63, 1, 1 << 63)), (q, num, den)
            else:
                assert even and odd, (q, num, den)                     # (2, q) has x = 0 and 1 alone
    for q in (Q61, Q63):                                               # what the sweep must not be without
        for num, den in [(p, q) for p in mod_switch_ps(q) if p not in (q - 2, 3 * q)] + [(2, q), (16, q), (65537, q)]:
            assert not no_float_tie(q, num, den) and float_ties(q, num, den)[0], (q, num, den)


def test_f64_reference_against_the_oracle_and_by_hand(oracle):
    assert [P.rust_round(x) for x in (0.5, -0.5, 1.5, 2.5, -2.5, 0.49999999999999994, 4503599627370497.0, 2.0 ** 52 + 0.5)] == \
        [1.0, -1.0, 2.0, 3.0, -3.0, 0.0, 4503599627370497.0, 2.0 ** 52]
    assert (P.as_i64(float("nan")), P.as_i64(1e30), P.as_i64(-1e30), P.as_i64(2.0 ** 63), P.as_i64(-(2.0 ** 63))) == (0, P.I64_MAX, P.I64_MIN, P.I64_MAX, P.I64_MIN)
    assert (P.as_u64(float("nan")), P.as_u64(-1.0), P.as_u64(2.0 ** 64), P.as_u64(2.0 ** 63)) == (0, 0, P.U64 - 1, 1 << 63)
    assert math.isnan(P.rust_round(float("nan"))) and P.rust_round(float("inf")) == float("inf")
    assert P.mul_div_round(Q16, 1, 2, 5) == 3 and P.mul_div_round(Q16, 1, 2, 4) == 2 and P.div_round(Q16, 2, 7) == 4      # ties go up
    assert P.mul_by_f64(Q16, -0.5, 5) == Q16 - 3 and P.mul_by_f64(Q16, float("nan"), 5) == 0
    assert P.mul_by_f64(Q61, float("inf"), 5) == P.I64_MAX % Q61 and P.mul_by_f64(Q61, float("-inf"), 5) == P.I64_MIN % Q61
    for q in F64_Q:
        for num, den in mul_div_pairs(q):
            ties = tie_words(q, num, den)
            a = np.array(f64_inputs(q, ties), dtype=np.uint64)
            out = np.empty_like(a)
            oracle.glue("rq_mul_div_round", q, len(a), a, num, den, out)
            assert out.tolist() == [P.mul_div_round(q, num, den, int(v)) for v in a], (q, num, den)
        for p in mod_switch_ps(q):
            a = np.array(f64_inputs(q, tie_words(q, p, q)), dtype=np.uint64)
            out = np.empty_like(a)
            oracle.glue("rq_mod_switch", q, len(a), a, p, out)
            assert out.tolist() == [P.mod_switch(q, p, int(v)) for v in a], (q, p)
        for s in DIV_ROUND_S:
            a = np.array(f64_inputs(q, tie_words(q, 1, s)), dtype=np.uint64)
            out = np.empty_like(a)
            oracle.glue("rq_div_round", q, len(a), a, s, out)
            assert out.tolist() == [P.div_round(q, s, int(v)) for v in a], (q, s)
        a = np.array(f64_inputs(q), dtype=np.uint64)
        out = np.empty_like(a)
        for s in mul_f64_factors(q):
            oracle.glue("rq_mul_by_f64", q, len(a), a, s, out)
            assert out.tolist() == [P.mul_by_f64(q, s, int(v)) for v in a], (q, s)
        for p in (2, Q16, q, (1 << 63) - 25):
            oracle.glue("rq_remodule", len(a), a, p, out)
            assert out.tolist() == [P.remodule(p, int(v)) for v in a]
    # the factors that land e exactly on +-2^63 do so at the largest canonical word
    for q in (Q61, Q63):
        s = mul_f64_factors(q)[11]
        assert float(q - 1) * s == 2.0 ** 63 and float(q - 1) * -s == -(2.0 ** 63)
