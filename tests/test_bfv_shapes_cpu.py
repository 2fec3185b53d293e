"""The launch classes of the BFV surfaces (fhe_bfv_tensor_dev, fhe_bfv_relinearize*_dev, fhe_bfv_mul*_dev: csrc/zring.hip
and csrc/bfv32.hip), enumerated without a device: what the host code decides from (q, n, t, pq, batch) and is not yet
restated in tests/test_crt_bounds.py (bfv32's groups of eight, the cap of the element-wise grids, the fused last pass,
the staging fallback, rows per workgroup and batch tile of the 2n-point transforms, the relinearisation's epilogue
gates), the class of a call, the universe of classes the modulus menu reaches on the batch ladder, and the case list
(CASES, with the inputs and the comparator) that tests/test_bfv_shapes_gpu.py runs, where the kernel timer's names are
checked against what this module predicts.  The restatement only plans the sweep: every comparison
of the sweep is against an independent reference whatever the split really is.  The module also pins the two references
against each other: tests/_bfv_numpy.py (Python integers, no NTT) and the oracle's schoolbook."""
import functools

import numpy as np
import pytest

import _bfv_numpy as BN
from conftest import Q16, Q61
from test_crt_bounds import (EXT32, bfv32_ok, bfv32_tensor_ok, epilogue_gates, epilogue_ts, primes_for_bits, q_top,
                             relin_form, relin_split_bits, rlk_words, tensor_form)

SIZES = tuple(1 << e for e in range(1, 15))             # every power of two 2 .. 2^14
BFV32_SIZES = (1024, 2048, 4096, 8192)
EW_CAP = 1 << 20                                        # capi_internal.hpp:79-83 fhe_ew_grid: 4096 workgroups of 256 threads
ENTRIES = ("tensor", "relin", "prepared", "mul", "mul_prepared")
Q12289 = 12289
Q20 = 786433                                            # 3 2^18 + 1: the largest bits(q - 1) = 20 the bfv32 tensor takes at 8192
Q30 = (1 << 30) + 3
QPAST = q_top(8192) + 1                                 # one past bfv32's rule at n = 8192: one 61-bit prime, fused last pass


def ladder(n):
    """the batches of the sweep at n: 1 .. 9, both sides of 16 / 32 / 64, and both sides of 2^20 / (2n) (where the
    element-wise kernels over batch 2n words start a second grid-stride trip) wherever that is <= 2049"""
    out = set(range(1, 10)) | {t + d for t in (16, 32, 64) for d in (-1, 0, 1)}
    cap = EW_CAP // (2 * n)
    if cap <= 2049:
        out |= {cap - 1, cap, cap + 1}
    return tuple(sorted(out))


ONE_BATCH = (9,)                                        # the rows of the menu that run at one batch: a ragged group after a full one


def menu(n):
    """(q, t, pq, batches) admitted at n.  The restatement decides the form; the comments say what is intended."""
    rows = [(Q16, 2, Q16 ** 3, None)]                   # the reference's own parameters: split key below 1024, bfv32 for both stages at 1024 .. 8192, fused last pass at 2^14
    if bfv32_tensor_ok(Q16, n):                         # t past the small_f64 gate, and past rdenf's: one batch per bfv32 size
        rows += [(Q16, t, Q16 ** 3, ONE_BATCH) for t in epilogue_ts(Q16, n)[1:]]
    rows += [
        (Q20, 5, Q20 ** 3, None),                       # bfv32 tensor feeding a 61-bit relinearisation
        (Q30, 3, Q30 ** 2, None),                       # tensor and relinearisation on two 61-bit primes
        (QPAST, 2, QPAST ** 2, None),                   # K = 1 with the fused last pass at LA = 6 (n = 8192), at batch > 8
        (Q61, 16, 2 * Q61, None),                       # three primes for both stages, i64 wrap everywhere
        (Q12289, 3, Q12289 * Q12289, None),             # a second reference-sized modulus
        (Q12289, 3, Q12289, None),                      # p = 1: the relinearisation divides by 1
        (Q12289, 3, Q12289 << 20, None),                # p even: the IEEE division
        (Q12289, 3, Q12289 * ((1 << 13) - 1), None),    # either side of the two relinearisation gates
        (Q12289, 3, Q12289 * ((1 << 11) - 1), None),
        (Q12289, 3, Q12289 * 65537 + 1, None),          # pq % q != 0
        (4096, 3, 4096 ** 2, None),                     # q a power of two: the tensor's rdenf is off
        (2, 3, 4, None),                                # q = 2
    ]
    return [r for r in rows if admitted(r[0], n, r[2])]


def admitted(q, n, pq):
    return 2 <= q < 1 << 63 and q <= pq < 1 << 63 and 1 <= tensor_form(q, n)[1] <= 3 and rlk_words(q, n, pq) != 0


# ---- the host's rules, restated -------------------------------------------------------------------------------------------

def group8(rows):
    """bfv32.hip:528, :540-548: the three kernels deal out groups of 8 rows or pairs (16 ((rows + 7) / 8) workgroups,
    24 ((batch + 7) / 8), 16 ((batch + 7) / 8)) and return early on the padding"""
    return "below" if rows < 8 else "one" if rows == 8 else "ragged" if rows % 8 else "full"


def bfv32_grids(batch):
    return 16 * ((4 * batch + 7) // 8), 24 * ((batch + 7) // 8), 16 * ((batch + 7) // 8), 16 * ((batch + 7) // 8)


def ew_capped(count):
    """capi_internal.hpp:79-83: more than 4096 workgroups' worth of words: the kernel's loop takes a second trip"""
    return count > EW_CAP


def contig_w(lp):
    """ntt_rounds.hpp:522-526 ContigCfg: rows per workgroup of a contiguous pass over 2^lp-point blocks"""
    return (256 if lp <= 12 else 512) // ((1 << lp) // 16)


def transform(n):
    """the 2n-point transforms of zring's forms -> (kind, rows per workgroup, LA, batch tile).  ntt_kernels.hip:974-978,
    :1170-1181: below 16 points one thread per row, 256 rows per workgroup; :980, :1183: one pass up to 2^13 points;
    above, ntt_rounds.hpp:768 contig_bits: a contiguous pass over 2^max(L - 8, 8)-point blocks and a strided pass of
    LA = L - that many stages, one row per workgroup column, in tiles of 2^(27 - L) rows (capi.hip:516)"""
    L = n.bit_length()
    if L < 4:
        return "tiny", 256, 0, 0
    if L <= 13:
        return "single", contig_w(L), 0, 0
    LB = max(L - 8, 8)
    return "two-pass", contig_w(LB), L - LB, 1 << (27 - L)


def staged(n):
    """zring.hip:405-416 z_forward_src: launch_ntt_forward_reduce (ntt_kernels.hip:1120) has no kernel below 16 points, so
    the source is reduced and padded by zr_reduce_pad_kernel first"""
    return n.bit_length() < 4


def inverse_mdr_la(n, K):
    """zring.hip:452-479 z_inverse_mdr: one prime, 2n > 2^13, LA in {6, 7, 8} -> LA, else 0"""
    kind, _, la, _ = transform(n)
    return la if K == 1 and kind == "two-pass" and la in (6, 7, 8) else 0


def relin_gates(q, pq):
    """zring.hip:637-639 bfv32_relinearize with :571-574 bfv32_rden -> (small_f64, rdenf), FHE_BFV_SMALL_F64 /
    FHE_BFV_FAST_DIV at their defaults.  (bfv32_rden's p < 2^48 is restated for completeness only: bfv32's own rule keeps
    pq below 2^(82 - 10 - bits(q - 1)), no menu row takes p there, and that side of the gate is not a class of the sweep.)"""
    p = pq // q
    return q < 1 << 30 and p >= 1 << 14, pq % q == 0 and p >= 1 << 12 and p & 1 == 1 and p < 1 << 48


def _fills(W, *rows):
    return tuple(r % W == 0 for r in rows)


def tensor_class(q, n, t, batch):
    form, K = tensor_form(q, n)
    if form == "bfv32":                                 # forward over 4 batch rows, inverse over batch pairs
        return "bfv32", epilogue_gates(q, n, t), group8(batch), group8(4 * batch)
    kind, W, _, tile = transform(n)
    la = inverse_mdr_la(n, K)
    inv = "staged" if staged(n) else "mdr%d" % la if la else kind
    tiles = 1 if not tile else max(-(-4 * batch // tile), 1)
    # zr_tensor over batch 2n words; zr_crt_mdr over 3 batch n where the fused pass does not run
    return "crt", K, inv, _fills(W, 4 * batch, 3 * batch), ew_capped(batch * 2 * n), (not la) and ew_capped(3 * batch * n), tiles


def relin_class(q, n, pq, batch):
    form, K = relin_form(q, n, pq)
    p = pq // q
    pk = "one" if p == 1 else "pow2" if p & (p - 1) == 0 else "odd" if p & 1 else "even"
    if form == "bfv32":
        return "bfv32", relin_gates(q, pq), pk, pq % q != 0, group8(batch)
    _, W, _, tile = transform(n)
    sets = 4 if form == "split" else 2                  # inverse rows per ciphertext and prime (zring.hip:746, :758, :772)
    tiles = 1 if not tile else max(-(-sets * batch // tile), 1)
    # zr_mul_bcast over batch 2n words; zr_split_mdr and zr_crt_mdr over 2 batch n: one threshold
    return form, K, staged(n), pk, pq % q != 0, _fills(W, batch, sets * batch), ew_capped(batch * 2 * n), tiles


def classes_of(q, t, pq, n, batch):
    """a case runs the five entries"""
    tc, rc = tensor_class(q, n, t, batch), relin_class(q, n, pq, batch)
    return {(n, "tensor", tc), (n, "relin", rc), (n, "prepared", rc), (n, "mul", tc, rc), (n, "mul_prepared", tc, rc)}


@functools.lru_cache(None)
def universe():
    """class -> the (q, t, pq, n, batch) that reach it.  What leaves the universe, by rule: a menu row not admitted at n
    (menu), and every batch but ONE_BATCH of the two rows that only move t past an epilogue gate"""
    out = {}
    for n in SIZES:
        for q, t, pq, batches in menu(n):
            for batch in batches or ladder(n):
                for c in classes_of(q, t, pq, n, batch):
                    out.setdefault(c, []).append((q, t, pq, n, batch))
    return out


@functools.lru_cache(None)
def cover():
    """a greedy cover, cheapest reference first: sizes ascending (the schoolbook reference costs n^2), at each the group
    (q, t, pq) that reaches the most uncovered classes, then the ladder batches of it that each add a class
    -> [((q, t, pq, n), [batch ...])]"""
    shapes = {}
    for c, reach in universe().items():
        for q, t, pq, n, batch in reach:
            shapes.setdefault((q, t, pq, n), {}).setdefault(batch, set()).add(c)
    need, out = set(universe()), []
    for n in SIZES:
        mine = {s: v for s, v in shapes.items() if s[3] == n}
        while any(c[0] == n for c in need):
            best = max(mine, key=lambda s: (len(set().union(*mine[s].values()) & need), s))
            batches, got = [], set()
            for batch in sorted(mine[best]):
                new = (mine[best][batch] & need) - got
                if new:
                    got |= new
                    batches.append(batch)
            assert got
            need -= got
            out.append((best, batches))
            del mine[best]
    assert not need
    return out


CASES = [s + (batch,) for s, batches in cover() for batch in batches]


def groups_of(n):
    """[((q, t, pq), [batch ...])] of the cover at n, in cover order"""
    return [(s[:3], batches) for s, batches in cover() if s[3] == n]


def compare_tiled(label, out, want, idx):
    """out: (planes, batch, n) words of a call; want: (planes, D, n) distinct reference rows; idx: the distinct row of
    every batch row -> [] when every word agrees, else [(label, plane, rows wrong, first wrong row, last wrong row)] per
    plane.  Works on host and device tensors alike."""
    import torch

    exp = want[:, idx]
    assert out.shape == exp.shape, (label, tuple(out.shape), tuple(exp.shape))
    if torch.equal(out, exp):
        return []
    bad = []
    for pl in range(out.shape[0]):
        rows = torch.nonzero(~(out[pl] == exp[pl]).all(dim=1)).reshape(-1)
        if rows.numel():
            bad.append((label, pl, int(rows.numel()), int(rows[0]), int(rows[-1])))
    return bad


def inputs(q, pq, n, d):
    """the distinct rows of a group, seeded by (q, n) alone so that groups of one q share their tensor references:
    ab (4, d, n) with row 0 of q - 1 throughout, row 1 with the planted words 0, 1, q - 1, q // 2 at the front of a0 and
    b0 and at the back of a1 and b1, the rest random; rlk (2, n): one random half, one of pq - 1 throughout"""
    rng = np.random.default_rng([q % (1 << 63), n])
    ab = rng.integers(0, q, (4, d, n), dtype=np.uint64)
    ab[:, 0] = q - 1
    plant = [0, 1, q - 1, q // 2][: min(4, n)]
    ab[0, 1, : len(plant)] = plant
    ab[2, 1, : len(plant)] = plant[::-1]
    ab[1, 1, n - len(plant):] = plant
    ab[3, 1, n - len(plant):] = plant[::-1]
    rlk = np.empty((2, n), dtype=np.uint64)
    rlk[0] = np.random.default_rng([pq, n]).integers(0, pq, n, dtype=np.uint64)
    rlk[1] = pq - 1
    return ab, rlk


def distinct_rows(n):
    return 6 if n <= 1024 else 2


# ---- tests ---------------------------------------------------------------------------------------------------------------------

def test_restated_shapes_at_known_points():
    assert [contig_w(lp) for lp in range(4, 14)] == [256, 128, 64, 32, 16, 8, 4, 2, 1, 1]
    assert transform(2)[:2] == ("tiny", 256) and transform(4)[0] == "tiny" and transform(8) == ("single", 256, 0, 0)
    assert transform(4096) == ("single", 1, 0, 0) and transform(8192) == ("two-pass", 16, 6, 8192) and transform(16384) == ("two-pass", 16, 7, 4096)
    assert transform(32768)[2] == 8                                    # LA = 8 starts past the sweep's sizes
    assert staged(2) and staged(4) and not staged(8)
    assert inverse_mdr_la(8192, 1) == 6 and inverse_mdr_la(16384, 1) == 7 and not inverse_mdr_la(8192, 2) and not inverse_mdr_la(4096, 1)
    assert [group8(b) for b in (1, 7, 8, 9, 15, 16, 17, 24)] == ["below"] * 2 + ["one", "ragged", "ragged", "full", "ragged", "full"]
    assert bfv32_grids(9) == (80, 48, 32, 32) and bfv32_grids(8) == (64, 24, 16, 16)
    assert not ew_capped(EW_CAP) and ew_capped(EW_CAP + 1)
    for n in SIZES:
        cap = EW_CAP // (2 * n)
        assert (cap <= 2049) == (n >= 256)
        if n >= 256:
            assert {cap - 1, cap, cap + 1} <= set(ladder(n)) and not ew_capped(cap * 2 * n) and ew_capped((cap + 1) * 2 * n)
        # the largest request of the ladder stays inside one batch tile: the tile loop takes one trip throughout
        tile = transform(n)[3]
        assert not tile or 4 * max(ladder(n)) <= tile
    assert max(ladder(16384)) == 65 and EW_CAP // (2 * 16384) + 1 == 33
    assert relin_gates(Q16, Q16 ** 3) == (True, True) and relin_gates(Q12289, Q12289 ** 2) == (False, True)
    assert relin_gates(Q12289, Q12289) == (False, False) and relin_gates(Q12289, Q12289 << 20) == (True, False)
    assert relin_gates(Q12289, Q12289 * 8191) == (False, True) and relin_gates(Q12289, Q12289 * 2047) == (False, False)
    assert relin_gates(Q12289, Q12289 * 65537 + 1) == (True, False)


def test_menu_rows_take_the_forms_intended():
    for n in SIZES:
        in32 = EXT32 and n in BFV32_SIZES
        assert tensor_form(Q16, n) == (("bfv32", 2) if in32 else ("crt", 1))
        assert relin_form(Q16, n, Q16 ** 3)[0] == ("bfv32" if in32 else "split")
        assert tensor_form(Q20, n)[0] == ("bfv32" if in32 else "crt") and relin_form(Q20, n, Q20 ** 3)[0] in ("split", "crt")
        assert tensor_form(Q30, n) == ("crt", 2) and relin_form(Q30, n, Q30 ** 2) == ("crt", 2)
        assert tensor_form(Q61, n) == ("crt", 3) and relin_form(Q61, n, 2 * Q61) == ("crt", 3)
        assert tensor_form(QPAST, n) == (("bfv32", 2) if EXT32 and n in (1024, 2048) else ("crt", 1))    # 21 bits: past the rule at 4096 too
        assert len(menu(n)) == (15 if n in BFV32_SIZES else 13), (n, len(menu(n)))
    assert not bfv32_tensor_ok(QPAST, 8192) and bfv32_tensor_ok(QPAST - 1, 8192) and inverse_mdr_la(8192, tensor_form(QPAST, 8192)[1]) == 6
    assert bfv32_tensor_ok(Q20, 8192) and not bfv32_ok(Q20, 8192, Q20 ** 3)
    for n in BFV32_SIZES:                                              # the two extra t: small_f64 off, then rdenf off as well
        ts = epilogue_ts(Q16, n)
        assert [epilogue_gates(Q16, n, t) for t in ts] == [(True, True), (False, True), (False, False)]
        assert epilogue_gates(4096, n, 3) == (True, False)


def test_the_case_list_leaves_out_no_class_of_the_universe():
    uni = universe()
    covered = set()
    for q, t, pq, n, batch in CASES:
        assert admitted(q, n, pq) and batch in ladder(n)
        covered |= classes_of(q, t, pq, n, batch)
    missing = sorted(set(uni) - covered, key=repr)
    assert not missing, missing[:10]
    assert covered == set(uni)
    tens = {c[2] for c in uni if c[1] == "tensor"}
    rel = {c[2] for c in uni if c[1] == "relin"}
    print("\nBFV: %d classes (%d tensor, %d relinearisation), %d cases in %d groups"
          % (len(uni), len(tens), len(rel), len(CASES), len(cover())))
    print("tensor forms:", sorted({c[:3] if c[0] == "crt" else c[:2] for c in tens}, key=repr))
    print("relinearisation forms:", sorted({c[:2] for c in rel}, key=repr))
    assert {c[0] for c in uni} == set(SIZES) and {c[1] for c in uni} == set(ENTRIES)
    for n in SIZES:                                                    # every entry at every size
        assert {c[1] for c in uni if c[0] == n} == set(ENTRIES)
    # tensor: each form, each K, each inverse, each gate combination, each batch class
    assert {c[0] for c in tens} == ({"bfv32", "crt"} if EXT32 else {"crt"})
    assert {c[1] for c in tens if c[0] == "crt"} == {1, 2, 3}
    assert {c[2] for c in tens if c[0] == "crt" and c[1] == 1} == {"staged", "single", "mdr6", "mdr7"}
    assert {c[2] for c in tens if c[0] == "crt" and c[1] > 1} == {"staged", "single", "two-pass"}
    for K in (1, 2, 3):
        mine = [c for c in tens if c[0] == "crt" and c[1] == K]
        assert {c[3] for c in mine} >= {(True, True), (False, False), (True, False)}, K     # 4 b fills where 3 b does not
        assert {c[4] for c in mine} == {False, True}, K                                      # either side of the grid cap
    assert {c[5] for c in tens if c[0] == "crt" and not c[2].startswith("mdr")} == {False, True}
    assert {c[6] for c in tens if c[0] == "crt"} == {1}                # one batch tile throughout (asserted on the ladder above)
    # relinearisation: each form and K; crt never runs on one prime (the split's rule is implied by the one-prime rule)
    assert {c[:2] for c in rel if c[0] != "bfv32"} == {("split", 1), ("crt", 2), ("crt", 3)}
    for n in SIZES:
        for q, t, pq, _ in menu(n):
            assert relin_form(q, n, pq) != ("crt", 1)
            if primes_for_bits((q - 1).bit_length() + (pq - 1).bit_length() + (n - 1).bit_length(), False) == 1:
                assert relin_split_bits(q, n, pq) or (EXT32 and bfv32_ok(q, n, pq))
    for form in ("split", "crt"):
        mine = [c for c in rel if c[0] == form]
        assert {c[2] for c in mine} == {False, True}, form                                   # staged or not
        assert {c[5] for c in mine} >= {(True, True), (False, False), (False, True)}, form
        assert {c[6] for c in mine} == {False, True}, form
        assert {c[7] for c in mine} == {1}
    assert {c[3] for c in rel if c[0] == "split"} == {"one", "pow2", "odd"} and {c[4] for c in rel if c[0] == "split"} == {False, True}
    if EXT32:
        b32t = [c for c in tens if c[0] == "bfv32"]
        assert {c[1] for c in b32t} == {(True, True), (False, True), (False, False), (True, False)}
        assert {c[2] for c in b32t} == {"below", "one", "ragged", "full"} and {c[3] for c in b32t} == {"below", "one", "ragged", "full"}
        b32r = [c for c in rel if c[0] == "bfv32"]
        assert {c[1] for c in b32r} == {(True, True), (False, True), (False, False), (True, False)}
        assert {c[2] for c in b32r} == {"one", "pow2", "odd"} and {c[3] for c in b32r} == {False, True}
        assert {c[4] for c in b32r} == {"below", "one", "ragged", "full"}
        for n in BFV32_SIZES:                                          # every batch class of the three kernels at every bfv32 size
            assert {c[2][2] for c in uni if c[0] == n and c[1] == "tensor" and c[2][0] == "bfv32"} == {"below", "one", "ragged", "full"}
            assert {c[2][4] for c in uni if c[0] == n and c[1] == "relin" and c[2][0] == "bfv32"} == {"below", "one", "ragged", "full"}
        # a bfv32 tensor feeding each 61-bit relinearisation form
        assert {c[3][0] for c in uni if c[1] == "mul" and c[2][0] == "bfv32"} == {"bfv32", "split", "crt"}
    # the fused last pass at batch > 8 at both sizes, with the default forms
    assert any(q == QPAST and n == 8192 and batch > 8 for q, t, pq, n, batch in CASES)
    assert any(n == 16384 and batch > 8 and tensor_form(q, n) == ("crt", 1) for q, t, pq, n, batch in CASES)
    assert max(batch for *_, n, batch in CASES if n == 16384) >= 33          # past 2^20 / (2n)
    assert max(batch for *_, batch in CASES) == 2049


def test_prepared_words_of_every_case(pkg):
    L = pkg.load_library()
    seen = set()
    for q, t, pq, n, _ in CASES:
        if (q, n, pq) not in seen:
            seen.add((q, n, pq))
            got = L.fhe_bfv_rlk_prepared_words(q, n, pq)
            assert got == rlk_words(q, n, pq) != 0, (q, n, pq, got)
            form = relin_form(q, n, pq)
            assert got == {"bfv32": 6 * n, "split": 8 * n}.get(form[0], 4 * form[1] * n)
    assert len(seen) == len({(s[0], s[3], s[2]) for s, _ in cover()})


def _menu_everywhere(n):
    rows = [r[:3] for r in menu(n)]
    return rows + [(Q16, t, Q16 ** 3) for t in epilogue_ts(Q16, 1024)[1:] if (Q16, t, Q16 ** 3) not in rows]


@pytest.mark.parametrize("n", [2, 8, 16, 64])
def test_the_python_reference_and_the_oracle_agree(oracle, n):
    """every menu row: the distinct rows of the sweep (one of q - 1 throughout), word for word; relinearize(tensor(.))
    is mul(.) on both sides; the 61-bit row's convolution wraps i64"""
    rows = _menu_everywhere(n)
    assert len(rows) == 15
    for q, t, pq in rows:
        ab, rlk = inputs(q, pq, n, 3)
        assert np.all(ab[:, 0] == q - 1) and np.all(rlk[1] == pq - 1)
        c = oracle.bfv_tensor(q, n, t, *ab)
        o = oracle.bfv_relinearize(q, n, pq, rlk[0], rlk[1], *c)
        m = oracle.bfv_mul(q, n, t, pq, rlk[0], rlk[1], *ab)
        for i in range(3):
            mine = BN.tensor(q, n, t, *ab[:, i])
            assert [list(map(int, x[i])) for x in c] == [list(x) for x in mine], (q, t, n, i)
            rel = BN.relinearize(q, n, pq, rlk[0], rlk[1], *mine)
            assert [list(map(int, x[i])) for x in o] == [list(x) for x in rel], (q, pq, n, i)
            assert BN.mul(q, n, t, pq, rlk[0], rlk[1], *ab[:, i]) == rel
            assert [list(map(int, x[i])) for x in m] == [list(x) for x in rel], (q, pq, n, i)
            a = ab[0, i].astype(np.int64)
            lin = oracle.r_naive_mul(n, a, ab[2, i].astype(np.int64))[0]
            assert lin.tolist() == BN.naive_mul(n, ab[0, i], ab[2, i])
            exact = BN.naive_mul_exact(n, ab[0, i], ab[2, i])
            wraps = any(not -(1 << 63) <= x < 1 << 63 for x in exact)
            # so that the 61-bit case keeps meaning something: its q - 1 row wraps at every n, a small modulus never
            # (2^30 + 3 wraps from n = 8 on)
            assert wraps or not (q == Q61 and i == 0), (q, n, i)
            assert not wraps or q > 1 << 26, (q, n, i)
            assert oracle.mul_div_round(q, n, lin, t, q)[0].tolist() == BN.mul_div_round_fold(q, n, lin.tolist(), t, q)


def test_the_comparator_names_one_flipped_word():
    import torch

    planes, d, n, batch = 3, 6, 8, 23
    from test_gadget_shapes_gpu import _tile

    idx = torch.from_numpy(_tile(batch, d))
    assert set(idx.tolist()) == set(range(d))
    want = torch.arange(planes * d * n, dtype=torch.int64).reshape(planes, d, n)
    out = want[:, idx].clone()
    assert compare_tiled("case", out, want, idx) == []
    out[planes - 1, batch - 1, n - 1] ^= 1
    assert compare_tiled(("q", 9, "mul"), out, want, idx) == [(("q", 9, "mul"), planes - 1, 1, batch - 1, batch - 1)]
    out[0, 2, 0] ^= 1 << 63
    assert compare_tiled("x", out, want, idx) == [("x", 0, 1, 2, 2), ("x", planes - 1, 1, batch - 1, batch - 1)]
