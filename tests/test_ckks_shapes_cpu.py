"""Proofs about the case lists of the CKKS evaluator's shape sweep (tests/_ckks_shapes_cases.py): what
tests/test_ckks_shapes_gpu.py runs covers every ring size, every depth with the wide limb at the bottom, in the middle and at
the top of the chain, the chunk of from_i64's staged route, and the one shape where the chunk clamp acts.  No device."""
import numpy as np
import pytest

import _ckks_bsgs_numpy as BN
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_linear_numpy as LN
import _ckks_shapes_cases as S


# ---- A ---------------------------------------------------------------------------------------------------------------------------
def test_ladder_has_every_ring_size_and_its_own_transform():
    assert {n for n, _, _ in S.LADDER} == {1 << L for L in range(1, 17)}
    for n in {n for n, _, _ in S.LADDER}:
        cases = {(k, b) for nn, k, b in S.LADDER if nn == n}
        assert cases == ({(2, 3), (3, 3)} if n <= 1 << 13 else {(2, 2)})
        mods, P = E.chain(n, *S.SPEC, 2)
        assert len(set(mods + [P])) == 4 and P >= max(mods)
        for q in mods + [P]:
            assert E.is_prime(q) and q % (2 * n) == 1 and 1 << 30 < q < 1 << 62                    # the kinds transform_names speaks of
        assert all(g % 2 == 1 and 0 < g < 2 * n for g in S.galois_pair(n) + S.reduced(S.DIAG + S.BABIES + S.GIANTS, n))
    names = {n: S.transform_names(n) for n, _, _ in S.LADDER}
    assert len({frozenset(v) for v in names.values()}) == 16                                       # a ring size, a set of rows
    assert names[8] == {"ntt_tiny_fwd_3", "ntt_tiny_inv_3"} and names[16] == {"ntt_fwd_contig_final_4", "ntt_inv_contig_final_4"}
    assert names[1 << 13] == {"ntt_fwd_contig_final_13", "ntt_inv_contig_final_13"}
    assert names[1 << 14] == {"ntt_fwd_strided_6", "ntt_fwd_contig_final_8", "ntt_inv_contig_8", "ntt_inv_strided_6"}
    assert names[1 << 16] == {"ntt_fwd_strided_8", "ntt_fwd_contig_final_8", "ntt_inv_contig_8", "ntt_inv_strided_8"}
    assert (S.BABIES, S.GIANTS) == BN.SWEEP and S.KEY_CUT == 1 << 13


def test_planted_rows_sit_at_the_edges():
    n = 16
    mods, _ = E.chain(n, *S.SPEC, 2)
    ct = S.planted_ct(mods, n, 3, 3, 5)
    plain = E.case_ct(mods, n, 3, 3, 5)
    for i, q in enumerate(mods):
        assert (ct[i, :, 0] == q - 1).all()
        for r, first in ((1, q // 2), (2, q // 2 + 1)):
            co = E.inv(q, n, ct[i, 2, r])
            assert co[0] == first and set(co.tolist()) == {q // 2, q // 2 + 1}                    # the centring decides these words
    assert ct.shape == plain.shape and ct.dtype == plain.dtype
    m = S.signed_rows(16, 2, 3)
    assert m[0, 0] == -(1 << 63) and m[0, 1] == (1 << 63) - 1
    key = S.random_key(mods, E.chain(n, *S.SPEC, 2)[1], n, 3)
    assert key.shape == (3, 4, 2, n) and all((key[:, i] < q).all() for i, q in enumerate(mods))
    w = S.weights(mods, (2, 2), 1)
    assert w[0][0] == [q - 1 for q in mods] and all(0 <= x < q for o in w for r in o for x, q in zip(r, mods))


# ---- B ---------------------------------------------------------------------------------------------------------------------------
def test_depth_list_puts_the_wide_limb_everywhere(pkg):
    base, P0 = E.wide_chain(S.N_DEPTH)
    own = {}
    for order in S.ORDERS:
        mods, P, wide = S.ordered_chain(order)
        assert sorted(mods) == sorted(base) and P == P0
        assert len(set(mods + [P])) == 9 and P >= max(mods) and P < 1 << 63 and P >= 1 << 62
        assert [q >> 62 != 0 for q in mods].count(True) == 1 and mods[wide] >> 62
        kinds = [pkg.Plan(q, S.N_DEPTH).arithmetic() for q in mods]
        assert set(kinds) == E.ARITH_KINDS
        assert min(mods) < 1 << 30                                                              # the 32-bit form, at n = 256
        own[order] = wide
    assert own == {"asis": 0, "reversed": 7, "index3": 3}
    ks = {(o, k) for o, k, kl in S.DEPTH if k == kl}
    assert ks == {(o, k) for o in S.ORDERS for k in range(1, 9)} and len(S.DEPTH) == 24
    assert sorted(kl - k for _, k, kl in S.DEPTH_LOW + [("asis", 8, 8)]) == list(range(8))
    # the wide limb as a target of the key sum: own_j in {0, 3, k - 1}; every case has the special-prime column (own_j = k), wide too
    own_js = {(own[o], k) for o, k, _ in S.DEPTH if own[o] < k}
    assert {j for j, _ in own_js} == {0, 3, 7} and (7, 8) in own_js and {k for j, k in own_js if j == 3} == {4, 5, 6, 7, 8}
    assert {k for o, k, _ in S.DEPTH if own[o] >= k} == set(range(1, 8))                         # only P is wide: the reversed order below k = 8


def test_key_sum_folds_once_to_three_times_and_never_overflows():
    q = E.primes_below(63, S.N_DEPTH, 2)[1]
    assert q >> 62
    for held in (0, 1):
        counts = {k: len(S.key_sum_folds(k, held)) for k in range(1, 9)}
        assert min(c for k, c in counts.items() if k >= 3) >= 1 and max(counts.values()) == 3 + held
        # held = 1 folds before every odd digit: four times at k = 8, one more than the three of held = 0
        assert S.key_sum_folds(8, held) == ([2, 4, 6] if held == 0 else [1, 3, 5, 7])
        for k in range(1, 9):
            assert S.key_sum_peak(q, k, held) < 1 << 128
    # across the list, at held = 0 (relinearise, Galois, dot) the wide limb folds 0 .. 3 times, at least once from k = 3
    assert {len(S.key_sum_folds(k, 0)) for _, k, _ in S.DEPTH} == {0, 1, 2, 3}
    assert {len(S.key_sum_folds(k, 1)) for _, k, _ in S.DEPTH} == {0, 1, 2, 3, 4}
    # 128 bits hold four terms below 2^126 (q < 2^63), so the schedule "before even j" at held = 1 (three terms and a carry-over
    # between two folds) gives the same words: the rule of key_sum is one term stricter than the bound needs
    for k in range(1, 9):
        assert S.key_sum_peak(q, k, 1, schedule=lambda j: j % 2 == 0) < 1 << 128
    # ... and a schedule of kMacChunk = 8 terms does not: from five terms on the sum of words q - 1 passes 2^128
    assert S.key_sum_peak(q, 8, 0, schedule=lambda j: j % 8 == 0) >= 1 << 128
    assert min(k for k in range(1, 9) if S.key_sum_peak(q, k, 0, schedule=lambda j: False) >= 1 << 128) == 5


# ---- C ---------------------------------------------------------------------------------------------------------------------------
def test_alignment_shapes_and_the_staged_chunk():
    assert S.ALIGN_SHAPES == [(16, 2, 3), (1024, 3, 3), (1 << 14, 2, 2)] and len(S.ENTRIES) == 12 and len(S.ALIGN_MODES) == 3
    n, k, batch = S.STAGED
    assert E.chunk_rows(n, k, batch) == 128 and batch == 128 + 1
    for n, k, batch in S.ALIGN_SHAPES:
        assert batch <= E.chunk_rows(n, k, batch)
        # one word past a 16-byte boundary, every row of every operand stays there: a row is an even number of words
        assert n % 2 == 0


# ---- D ---------------------------------------------------------------------------------------------------------------------------
def test_clamp_shape_is_the_smallest_and_the_workspaces_follow(pkg):
    B = pkg.binding
    n, k, batch = S.CLAMP
    assert S.chunk_quotient(n, k) == 0 and E.chunk_rows(n, k, batch) == 1
    assert S.chunk_quotient(n, k - 1) >= 1                                                        # 2^16: k = 5 still has a quotient
    for L in range(1, 16):
        for kk in range(1, S.MAX_K + 1):
            assert S.chunk_quotient(1 << L, kk) >= 1, (L, kk)
    assert S.chunk_quotient(1 << 15, 8) == 1 and (1 << 15) * 64 == E.CHUNK_WORDS
    assert E.chunk_rows(n, k, batch, rescale=True) == 2                                            # the rescale's chunk does not clamp here
    assert E.CHUNK_WORDS // ((1 << 18) * 8) == 1 and E.CHUNK_WORDS // ((1 << 19) * 8) == 0          # ... nor below n = 2^19
    slab = n * 8
    assert B.ckks_rns_workspace_bytes(n, k, batch) == S.relin_workspace_bytes(n, k, batch) == (k * k + 8 * k + 2) * slab
    assert B.ckks_rns_galois_workspace_bytes(n, k, batch, 1) == G.workspace_bytes(n, k, batch) == (k * k + 5 * k + 2) * slab
    for outputs in (1, 2, 3):
        assert B.ckks_rns_diag_workspace_bytes(n, k, batch, 2, outputs) == LN.workspace_bytes(n, k, batch, outputs) \
            == (k * k + 3 * k + 2 * (k + 1) * min(outputs, 2)) * slab
    assert B.ckks_rns_bsgs_workspace_bytes(n, k, batch, 2, 2) == BN.workspace_bytes(n, k, batch) == BN.workspace_slabs(k) * slab
    mods, P = E.chain(n, *S.SPEC, k - 1)
    assert len(set(mods + [P])) == k + 1 and P >= max(mods) and all(q % (2 * n) == 1 for q in mods + [P])


# ---- E ---------------------------------------------------------------------------------------------------------------------------
def test_stream_cases_shrink_then_grow_the_workspace():
    n, k, batches = S.REUSE
    sizes = [S.relin_workspace_bytes(n, k, b) for b in batches]
    assert sizes[1] < sizes[0] < sizes[2] and all(b <= E.chunk_rows(n, k, b) for b in batches)
