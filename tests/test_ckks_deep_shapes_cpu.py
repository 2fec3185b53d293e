"""Proofs about the case lists of the deep CKKS chain's sweep (tests/_ckks_deep_shapes_cases.py): every chain is
admitted exactly, the bound-reaching rows reach the bound they claim, the fold schedules of the two sum kernels stay below 2^128
and the looser ones named here do not, every planted integer decides the centring compare at the digit it claims, the kernel's
route equals the definition on all of them, and every case said to cross or clamp a chunk does.  No device."""
import time

import numpy as np
import pytest

import _ckks_deep_linear_numpy as DL
import _ckks_deep_numpy as D
import _ckks_deep_shapes_cases as S
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G

U64 = np.uint64


# ---- A1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.WIDTH_NS)
@pytest.mark.parametrize("L,alpha,l", S.LIMIT_SHAPES)
def test_limit_chains_are_admitted_and_just_below_the_limit(n, L, alpha, l):
    mods, sps = S.limit_chain(n, L, alpha)
    D.check_chain(n, mods, sps)
    assert D.admits(mods, sps) and len(mods) == L and len(sps) == alpha
    assert all((1 << 62) - (1 << 30) < q < 1 << 62 for q in mods + sps)     # 2^62 - 2^30 < q: 17 (q - 1)^2 passes 2^128
    assert 17 * (min(mods + sps) - 1) ** 2 > S.WORD


@pytest.mark.parametrize("L,alpha,l", S.LIMIT_SHAPES)
def test_the_bound_reaching_rows_reach_the_bound(L, alpha, l):
    """a component -1 with keys and plaintexts m_i - 1: every group's centred integer is -1, every lifted digit m_i - 1 in every
    target, every term of every key sum (m_i - 1)^2; the tensor of minus_one_pair has d2 = -1"""
    n, batch = 8, 3
    mods, sps = S.limit_chain(n, L, alpha)
    lm = mods[:l]
    ct = S.minus_one_ct(lm, n, batch, 2, 5, 1)
    for i, q in enumerate(lm):
        assert [int(v) for v in E.inv(q, n, ct[i, 1, 0])] == [q - 1] + [0] * (n - 1)
    for grp in D.groups(l, alpha):
        x = D.centred_int([lm[i] for i in grp], [E.inv(lm[i], n, ct[i, 1, :1]) for i in grp])
        assert x[0, 0] == -1 and not x[0, 1:].any()
    Dg = D.digits(lm, sps, ct[:, 1])
    for i, m in enumerate(lm + sps):
        assert np.all(Dg[i, :, 0] == U64(m - 1)), i
    for g in (1, 5):                                                         # a row of equal words is fixed by every pi_g
        assert np.array_equal(G.galois_evals(ct[:, 1, :1], g), ct[:, 1, :1])
    a, b = S.minus_one_pair(lm, n, batch, 7)
    ten = E.tensor(lm, a, b)
    for i, q in enumerate(lm):
        assert np.all(ten[i, 2, 0] == U64(q - 1))
    key, pts = S.top_key(mods, sps, n), S.top_pts(lm, sps, n, 2, 3)
    assert key.shape == (D.dnum(L, alpha), L + alpha, 2, n) and pts.shape == (2, 3, l + alpha, n)
    for i, m in enumerate(mods + sps):
        assert np.all(key[:, i] == U64(m - 1))
    assert D.dnum(32, 1) == 32                                               # (32, 1, 32): 32 such terms a sum


# ---- A2 -----------------------------------------------------------------------------------------------------------------------------
def test_fold_schedules_replayed():
    """Under the kernels' rule (a fold before digit j > 0 and element r > 0 where the index is a multiple of 8) every accumulator
    stays below 2^128 for every q < 2^62, at every digit count to 32 and every element count to 256.

    Looser schedules, at the primes of S.limit_chain (above 2^62 - 2^30):
      * the key sum of ckks_deep_keymac_kernel folded on j % 16: a run is at most 16 terms and a carry-over, (q - 1) (16 q - 15) <
        2^62 2^66: BELOW 2^128 for every q < 2^62.  reduce128 takes any 128-bit value, so the words are the same: that change
        cannot be detected, up to the 32 digits the unit admits.  The first schedule that passes is a run of 17 terms (j % 17, or
        no fold from 17 digits on).
      * the inner sum of ckks_deep_diagmac_kernel carries the addend's term besides: folded on j % 16 its first run is 17 terms,
        17 (q - 1)^2 > 2^128, and with no fold at all 33 terms at 32 digits.  Both pass.
      * the outer sum folded on r % 16 (no fold at r = 8): 16 terms and the carry-over, below 2^128 as above: not detectable.
        A group that does not start from the canonical word (no fold between launches) cannot be written with this kernel."""
    qmax = (1 << 62) - 1
    for q in (qmax, S.limit_chain(8, 32, 1)[0][0], S.limit_chain(64, 32, 1)[1][0]):
        for k in range(1, 33):
            assert S.keymac_peak(q, k) <= 8 * (q - 1) ** 2 + q - 1 < S.WORD
            assert S.keymac_peak(q, k, fold=lambda j: j % 16 == 0) < S.WORD                      # not detectable
            for count in (1, 8, 9, 16, 17, 32, 33, 256):
                inner, outer = S.diagmac_peaks(q, k, count)
                assert inner <= 9 * (q - 1) ** 2 < S.WORD and outer <= 8 * (q - 1) ** 2 + q - 1 < S.WORD
                assert S.diagmac_peaks(q, k, count, outer=lambda r: r % 16 == 0)[1] < S.WORD     # not detectable
    for n in S.WIDTH_NS:
        mods, sps = S.limit_chain(n, 32, 1)
        for q in mods + sps:
            assert S.keymac_peak(q, 32, fold=lambda j: j % 17 == 0) > S.WORD and S.keymac_peak(q, 17, fold=lambda j: False) > S.WORD
            assert S.keymac_peak(q, 16, fold=lambda j: False) < S.WORD                           # 16 digits never need a fold
            assert S.diagmac_peaks(q, 32, 17, inner=lambda j: j % 16 == 0)[0] > S.WORD
            assert S.diagmac_peaks(q, 32, 17, inner=lambda j: False)[0] > S.WORD
            assert S.diagmac_peaks(q, 15, 17, inner=lambda j: False)[0] < S.WORD                 # addend + 15: only 16 digits and more bite
    # which shapes of the sweep have enough digits for the inner fold to matter: (32, 1, 32) alone
    assert [D.dnum(l, a) for _, a, l in S.LIMIT_SHAPES] == [32, 3, 3, 2]


def test_the_extension_sum_has_a_high_word():
    """at primes just below 2^62 the 128-bit sum of ckks_deep_extend_kernel passes 2^64 (its high word is not zero) and stays below
    2^127; at §36's 40-bit primes it does not reach 2^64 until three sources and more - and then by little"""
    for n in S.WIDTH_NS:
        for L, alpha, l in S.LIMIT_SHAPES:
            mods, sps = S.limit_chain(n, L, alpha)
            for grp in D.groups(l, alpha):
                src = [mods[i] for i in grp]
                _, _, W, _ = D.garner_tables(src, mods[:l] + sps)
                for t in range(l + alpha):
                    peak = S.extend_peak(src, [W[j][t] for j in range(len(src))])
                    assert peak < 1 << 127
            _, _, W, _ = D.garner_tables(sps, mods[:l])
            assert S.extend_peak(sps, [W[j][0] for j in range(alpha)]) >> 64 or alpha == 1


# ---- A3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.WIDTH_NS)
@pytest.mark.parametrize("alpha", S.MIXED_ALPHAS)
@pytest.mark.parametrize("order", S.MIXED_ORDERS)
def test_mixed_chains(n, alpha, order):
    mods, sps = S.mixed_chain(n, alpha, order)
    D.check_chain(n, mods, sps)
    assert D.admits(mods, sps) and len(mods) == 2 * alpha + 1
    bits = [q.bit_length() for q in mods]
    for grp in list(D.groups(len(mods), alpha))[:2]:
        b = [bits[i] for i in grp]
        assert 30 in b and max(b) >= 37                                      # a 30-bit prime beside a wider one
        first_small = b.index(30) < b.index(max(b))
        assert first_small == (order == "up")
    assert {30, 37, 61, 62} <= set(bits) or alpha == 2 and {30, 61, 62} <= set(bits)
    assert all(p.bit_length() == 62 for p in sps)


def _sources():
    for n in S.WIDTH_NS:
        for alpha in S.MIXED_ALPHAS:
            for order in S.MIXED_ORDERS:
                mods, sps = S.mixed_chain(n, alpha, order)
                for grp in D.groups(len(mods), alpha):
                    yield [mods[i] for i in grp], [q for i, q in enumerate(mods) if i not in grp] + sps
        for alpha in S.DOWN_ALPHAS:
            mods, sps = S.limit_chain(n, 4, alpha)
            yield sps, mods


def test_every_planted_integer_decides_the_compare_where_it_claims():
    seen = set()
    for src, dst in _sources():
        M, h = D.product(src), S.half_digits(src)
        assert S.from_digits(src, h) == M // 2
        for i, above, x in S.depth_integers(src):
            a, y = [], x
            for m in src:
                a.append(y % m)
                y //= m
            assert a[i + 1:] == h[i + 1:] and a[i] != h[i] and (a[i] > h[i]) == above == (x > M // 2)
            seen.add((len(src), i))
        if len(src) > 2:                                                     # middle digits, with the low digits pointing the wrong way
            mid = [x for i, above, x in S.depth_integers(src) if 0 < i < len(src) - 1]
            assert any(x > M // 2 and x % src[0] == 0 for x in mid) and any(x < M // 2 and x % src[0] == src[0] - 1 for x in mid)
    assert {(8, i) for i in range(8)} <= seen and {(3, 1), (4, 1), (4, 2)} <= seen


def test_the_kernels_route_is_the_definition_on_every_planted_integer():
    for src, dst in _sources():
        xs = S.planted_integers(src)
        res = [np.array([x % m for x in xs], dtype=U64) for m in src]
        assert np.array_equal(D.extend_garner(src, res, dst), D.extend_crt(src, res, dst)), src


def test_planted_rows_hold_the_planted_integers():
    n, alpha = 8, 4
    mods, sps = S.mixed_chain(n, alpha, "down")
    d2, coef = S.planted_rows(mods, alpha, n)
    assert d2.shape == coef.shape and d2.shape[1] == -(-len(S.planted_integers(mods[:alpha])) // n)
    for grp in D.groups(len(mods), alpha):
        src = [mods[i] for i in grp]
        xs = S.planted_integers(src)
        x = D.centred_int(src, [E.inv(mods[i], n, d2[i]) for i in grp]).reshape(-1)
        M = D.product(src)
        assert [int(v) % M for v in x[:len(xs)]] == xs


@pytest.mark.parametrize("alpha", S.DOWN_ALPHAS)
def test_down_case_steers_t_modulo_p(alpha):
    """t modulo P of the restatement is the planted integer, coefficient by coefficient, component by component"""
    n = 8
    mods, sps, d, keys, ys = S.down_case(n, alpha)
    assert D.admits(mods, sps) and len(keys) * 2 * n == len(ys) >= len(S.planted_integers(sps))
    P = D.product(sps)
    for t, key in enumerate(keys):
        sums = D.key_switch_sums(mods, sps, key, d[:, 2])
        y = D.centred_int(sps, [E.inv(p, n, sums[len(mods) + m]) for m, p in enumerate(sps)])
        assert [int(v) % P for v in y[:, 0].reshape(-1)] == ys[2 * n * t:2 * n * (t + 1)]


# ---- B, C -----------------------------------------------------------------------------------------------------------------------------
def test_ladder_and_count_lists():
    assert sorted([n for n, _ in S.LADDER] + list(S.RAN_BEFORE)) == [1 << L for L in range(1, 17)]
    assert all(b == (3 if n <= 1 << 13 else 2) for n, b in S.LADDER)
    L, alpha, l = S.LADDER_SHAPE
    assert (D.dnum(L, alpha), D.dnum(l, alpha)) == (3, 2) and L % alpha and l < L            # ng = 2 < dnum = 3, the last group partial at L
    for n, _ in S.LADDER:
        D.check_chain(n, *D.case_chain(n, L, alpha))
        assert [g % (2 * n) for g in S.LADDER_DIAG][0] == 1
    for count, outputs, ident in S.COUNT_CASES:
        gs = S.diag_elements(S.COUNT_N, count, ident)
        assert len(gs) == count <= DL.MAX_COUNT and outputs <= DL.MAX_OUTPUTS and [r for r, g in enumerate(gs) if g == 1] == sorted(ident)
        assert all(g % 2 == 1 and g < 2 * S.COUNT_N for g in gs)
    counts = {c for c, _, _ in S.COUNT_CASES}
    assert counts == {32, 33, 256} and {o for _, o, _ in S.COUNT_CASES} >= {4, DL.MAX_OUTPUTS}
    assert set(range(32, 48)) <= set(S.COUNT_CASES[3][2])                    # a whole group of 16 identities
    assert DL.launch_counts(5, 2, 33, 4) == dict(extend=3 + 4, diagmac=7 * 2 * 3, keymac=0, divround=4 * 5)


def test_recurring_keys_are_summed_once_and_give_the_same_words():
    """DL.diag_sum takes the key sums of a (key, element) pair that recurs once; the words are those of separate copies"""
    n, (L, alpha, l) = 8, (5, 2, 5)
    mods, sps = D.case_chain(n, L, alpha)
    gs = S.diag_elements(n, 7, (2,))
    pool = S.pool_keys(mods, sps, n, 3)
    ct, pts = E.case_ct(mods, n, 2, 2, 4), DL.random_pts(mods, sps, n, 2, 7, 5)
    assert np.array_equal(DL.diag_sum(mods, sps, S.keys_of(pool, gs), gs, pts, ct),
                          DL.diag_sum(mods, sps, [None if g == 1 else pool[g].copy() for g in gs], gs, pts, ct))


@pytest.mark.parametrize("n,L,alpha,l", [(8, 5, 2, 4), (16, 3, 8, 3), (8, 9, 3, 7)])
def test_galois_many_is_apply_galois_per_element(n, L, alpha, l):
    """S.galois_many (one set of digits, read at pi_g) against D.apply_galois (the permuted ciphertext, switched): the same words"""
    mods, sps = S.limit_chain(n, L, alpha)
    lm = mods[:l]
    pool = S.pool_keys(lm, sps, n, 9, key_mods=mods)
    gs = S.pool_elements(n) + S.pool_elements(n)[:1]
    ct = S.minus_one_ct(lm, n, 3, 2, 10, 1)
    got = S.galois_many(lm, sps, S.keys_of(pool, gs), gs, ct)
    for r, g in enumerate(gs):
        assert np.array_equal(got[r], D.apply_galois(lm, sps, pool[g], ct, g)), g


# ---- D -----------------------------------------------------------------------------------------------------------------------------
def test_the_clamps_and_the_crossed_chunk():
    n, alpha, l, batch = S.CLAMP
    words = D.CHUNK_WORDS // n
    assert words == 128 and (D.slabs(l, alpha), DL.slabs(l, alpha, 2)) == (159, 152)
    smallest = min(k for k in range(1, 33) if words // D.slabs(k, alpha) == 0 and words // DL.slabs(k, alpha, 2) == 0)
    assert smallest == l
    assert D.chunk_rows(n, l, alpha, batch) == DL.chunk_rows(n, l, alpha, batch, 2) == 1
    assert D.workspace_bytes(n, l, alpha, batch) == 8 * 159 * n and DL.workspace_bytes(n, l, alpha, batch, 3, 2) == 8 * 152 * n
    D.check_chain(n, *D.case_chain(n, l, alpha))
    n, l, batch = S.RESCALE_CROSSED
    assert (D.CHUNK_WORDS // n) // (2 * l) == 4 and S.chunks_of(batch, S.rescale_chunk(n, l, batch)) == [4, 1]
    n, l, batch = S.RESCALE_CLAMPED
    assert (D.CHUNK_WORDS // n) // (2 * l) == 0 and S.chunks_of(batch, S.rescale_chunk(n, l, batch)) == [1, 1]
    assert min(k for k in range(2, 33) if (D.CHUNK_WORDS // n) // (2 * k) == 0) == l
    for n, (L, alpha, l), batch in S.ALIGN_SHAPES:
        assert S.chunks_of(batch, D.chunk_rows(n, l, alpha, batch)) == ([batch] if n == 64 else [1, 1])


def test_reference_cost_of_the_large_cases():
    """the restatement alone of each large case (D3): printed, and held to a generous ceiling so that a change that makes one of
    them slow is seen here and not on the device"""
    out = {}
    n, alpha, l, batch = S.CLAMP
    mods, sps = D.case_chain(n, l, alpha)
    key = S.uniform_key(mods, sps, n, 1)
    a, b = E.case_ct(mods, n, batch, 2, 2), E.case_ct(mods, n, batch, 2, 3)
    t0 = time.time()
    D.mul(mods, sps, key, a, b)
    out["clamp mul"] = time.time() - t0
    t0 = time.time()
    D.apply_galois(mods, sps, key, a, 5)
    out["clamp galois"] = time.time() - t0
    gs = [1, 5, 5]
    pts = DL.random_pts(mods, sps, n, 2, 3, 4)
    t0 = time.time()
    DL.diag_sum(mods, sps, [None, key, key], gs, pts, a)
    out["clamp diag_sum"] = time.time() - t0
    for name, (n, l, batch) in (("rescale crossed", S.RESCALE_CROSSED), ("rescale clamped", S.RESCALE_CLAMPED)):
        mods = E.primes_below(40, n, l)
        a = E.case_ct(mods, n, batch, 2, 5)
        t0 = time.time()
        D.rescale(mods, a)
        out[name] = time.time() - t0
    print("reference alone: " + ", ".join("%s %.2f s" % kv for kv in out.items()))
    assert max(out.values()) < 10
