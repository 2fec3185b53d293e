"""Proofs about the case lists of the sweep of BFV on the RNS chain (tests/_bfv_rns_shapes_cases.py): every planted
phase is a phase, every rounding edge a phase can reach is planted at every (k, t, b_0), the route of the device (Garner's digits,
one auxiliary prime) equals the definition on all of them, the planted integers of the extension differ from floor(M / 2) in the
digit they claim, the sparse-times-dense product is the negacyclic product, and every case said to cross a chunk crosses it.
No device."""
import math
import random

import numpy as np
import pytest

import _bfv_rns_numpy as R
import _bfv_rns_shapes_cases as S
import _ckks_eval_numpy as E


def _decrypt_sets():
    """every (mods, t, b_0) the GPU module decrypts under"""
    out = []
    for n, k in S.DECRYPT_SHAPES:
        mods = R.chain(n, k)[0]
        out += [(mods, t, b0) for t, b0 in S.decrypt_params(k)]
    n, k, _, t, b0 = S.DECRYPT_CHUNK
    return out + [(S.small_chain(n, k)[0], t, b0)]


# ---- A ---------------------------------------------------------------------------------------------------------------------------
def test_planted_phases_are_phases_and_reach_every_edge_a_phase_can():
    seen = set()
    for mods, t, b0 in _decrypt_sets():
        Q, h = R.prod(mods), R.prod(mods) // 2
        assert b0 % 2 == 1 and 2 * t + 2 < b0 < 1 << 62 and t < 1 << 60 and math.gcd(b0, Q) == 1 and Q > 2 * t
        seen.add((t, b0))
        planted = S.planted_phases(Q, t)
        quot = {}
        for c, v in planted:
            assert -Q < 2 * v <= Q, (c, v)                           # in (-Q/2, Q/2]
            m = R.scale_round(v, t, Q)
            assert -(t // 2) - 1 <= m <= t // 2 + 1
            quot.setdefault(c.split(":")[0], set()).add(m)
        # the generator may drop planted values, never a class a phase can reach: every target in [-floor(t/2), floor(t/2)]
        # keeps at least one phase that rounds to it, and the others have none anywhere in the interval
        targets = dict(S.quotient_targets(t))
        assert S.reachable_targets(t) == {"0", "+1", "-1", "+t/2", "-t/2"}
        for name, m in targets.items():
            if name in S.reachable_targets(t):
                assert quot[name] == {m}, (name, t)
            else:
                assert name not in quot and not R.scale_round(-h, t, Q) <= m <= R.scale_round(h, t, Q)
        assert {"zero", "+half", "-half", "+half-1", "-half+1"} <= set(quot)
        assert (R.scale_round(h, t, Q), R.scale_round(-h, t, Q)) == (t // 2, -(t // 2))
        # both sides of every rounding edge: min is the first phase of its quotient, max the last
        for c, v in planted:
            name, _, side = c.partition(":")
            if side == "min" and v > -h:
                assert R.scale_round(v - 1, t, Q) == targets[name] - 1
            if side == "max" and v < h:
                assert R.scale_round(v + 1, t, Q) == targets[name] + 1
        # the kernel's sign branch: negative quotients that are no multiple of t, and none that is (it has no phase)
        ms = {R.scale_round(v, t, Q) for _, v in planted}
        assert any(m < 0 and m % t for m in ms) and not any(m < 0 and m % t == 0 for m in ms)
    assert {(257, 517), (65537, 131077), (2, 7), (1 << 16, (1 << 17) + 3), (S.T60, S.B0_T60)} == seen
    assert E.is_prime(S.B0_T60) and 1 << 61 < S.B0_T60 < 1 << 62


def test_route_decrypt_is_the_definition_on_every_planted_phase():
    rng = random.Random(5)
    for mods, t, b0 in _decrypt_sets():
        Q = R.prod(mods)
        vs = [v for _, v in S.planted_phases(Q, t)] + [rng.randrange(-(Q // 2), Q // 2 + 1) for _ in range(20)]
        assert [R.route_decrypt(mods, b0, t, v) for v in vs] == [int(x) for x in R.decrypt_phase(mods, t, [vs])[0]], (t, b0)


def test_phase_rows_and_the_ciphertext_built_around_them():
    for n, k in [(2, 1), (2, 4), (64, 2)]:
        mods = R.chain(n, k)[0]
        Q = R.prod(mods)
        for t, _ in S.decrypt_params(k):
            planted = [v for _, v in S.planted_phases(Q, t)]
            batch = S.decrypt_batch(n, len(planted))
            rows = S.phase_rows(Q, t, n, batch, 1)
            assert len(rows) == batch and all(len(r) == n for r in rows)
            flat = [v for r in rows for v in r]
            assert flat[:len(planted)] == planted and all(-Q < 2 * v <= Q for v in flat)
            if n >= len(planted):
                assert all(r[:len(planted)] == planted for r in rows)
            s, ct = S.ct_of_phase(mods, n, rows, 2)
            # c0 + c1 (.) s^ per limb, brought back to coefficients and through the CRT, is the rows
            ev = np.stack([E.padd(q, ct[i, 0], E.pmul(q, ct[i, 1], s[i])) for i, q in enumerate(mods)])
            assert R.coeffs_centred(mods, n, ev) == rows
            assert all((ct[i] < q).all() for i, q in enumerate(mods))


def test_messages_and_scale_msg_on_any_word():
    for k in (1, 2, 3, 4):
        mods = R.chain(8, k)[0]
        Q = R.prod(mods)
        ts = S.scale_msg_moduli(k, Q)
        assert ts[:2] == [2, 65537] and all(2 <= t <= Q and t < 1 << 64 for t in ts)
        assert ([Q - 1, Q] == ts[2:] and Q // (Q - 1) == 1) if k == 1 else True
        assert ts[-1] == (1 << 64) - 59 if k == 2 else True
        for t in ts:
            m = S.messages(t, 3, 2, 1)
            assert [int(x) for x in m.reshape(-1)] == [0, t - 1, min(t, 2 ** 64 - 1), min(t + 1, 2 ** 64 - 1), 1 << 63, (1 << 64) - 1]
            assert [int(x) for x in S.messages(t, 1, 2, 1).reshape(-1)] == [0, t - 1]
            got = R.scale_msg(mods, t, m)
            for i, q in enumerate(mods):
                assert [int(x) % q for x in got[i].reshape(-1)] == [(Q // t) * int(x) % q for x in m.reshape(-1)]
                assert all(-(q // 2) <= int(x) <= q // 2 for x in got[i].reshape(-1))
    assert R.prod(R.chain(8, 1)[0]) + 1 < 1 << 64                     # t = Q + 1 fits the word it is refused in


# ---- B ---------------------------------------------------------------------------------------------------------------------------
def test_mixed_bases_and_their_planted_integers():
    for s, (src, dst) in S.EXT_BASES.items():
        assert len(src) == s and len(set(src)) == s and len(set(dst)) == len(dst) <= 9
        assert all(m % 2 == 1 and 3 <= m < 1 << 62 for m in src + dst)
        assert all(math.gcd(a, b) == 1 for i, a in enumerate(src) for b in src[:i])
        bits = {m.bit_length() for m in src}
        assert min(bits) <= 3 and max(bits) == 62 and 3 in dst and {m.bit_length() for m in dst} & {62}
        assert [m.bit_length() for m in src] == sorted(m.bit_length() for m in src) and S.ext_base(s, "down") == (src[::-1], dst[::-1])
    assert min(S.EXT_BASES[2][1]) < min(S.EXT_BASES[2][0]) and min(S.EXT_BASES[3][1]) < min(S.EXT_BASES[3][0])
    assert {len(v[0]) for v in S.EXT_BASES.values()} == {2, 3, 5, 9}
    for s in S.EXT_BASES:
        for order in S.EXT_ORDERS:
            src, dst = S.ext_base(s, order)
            M, h = R.prod(src), R.half_digits(src)
            xs = S.planted_integers(src)
            assert len(xs) == len(set(xs)) <= S.EXT_COUNT and {0, M - 1, M // 2, M // 2 + 1} <= set(xs)
            digits = [R.garner_digits(src, [x % m for m in src]) for x in xs]
            for i in range(s):
                # above and below floor(M / 2) by the digit at i alone, with digit 0 pointing the other way where i > 0
                for step in (1, -1):
                    if 0 <= h[i] + step < src[i]:
                        hit = [d for d in digits if d[i + 1:] == h[i + 1:] and d[i] == h[i] + step]
                        assert len(hit) >= (3 if i else 1)
                        if i:
                            assert any(d[0] == 0 for d in hit) and any(d[0] == src[0] - 1 for d in hit)
                assert any(d[i] and not any(d[:i] + d[i + 1:]) for d in digits)     # a single non-zero digit
            assert any(d == [m - 1 for m in src] for d in digits)
            # an ordering that reads the top digit and digit 0 only gets some planted integer wrong, from three sources on
            if s >= 3:
                def top_and_bottom(d):
                    return d[-1] > h[-1] if d[-1] != h[-1] else d[0] > h[0]
                assert any(top_and_bottom(d) != (x > M // 2) for x, d in zip(xs, digits))


@pytest.mark.parametrize("s", sorted(S.EXT_BASES))
@pytest.mark.parametrize("order", S.EXT_ORDERS)
def test_garner_extend_is_extend_on_the_mixed_bases(s, order):
    src, dst = S.ext_base(s, order)
    xs = S.ext_integers(src, S.EXT_COUNT, 100 * s)
    assert len(xs) == S.EXT_COUNT
    cut = S.planted_integers(src) + xs[-8:]
    res = np.array([[x % m for x in cut] for m in src], dtype=np.uint64)
    for centred in (False, True):
        want = S.ext_want(src, dst, cut, centred)
        assert np.array_equal(R.extend(src, dst, res, centred), want)
        assert [R.garner_extend(src, dst, res[:, e], centred) for e in range(len(cut))] == [[int(v) for v in want[:, e]] for e in range(len(cut))]


def test_stride_case_takes_a_second_trip():
    src, dst, count = S.STRIDE
    assert count > E.GRID_CAP and R.prod(src) < 1 << 64 and len(src) == len(dst) == 2


# ---- C ---------------------------------------------------------------------------------------------------------------------------
def test_chains_are_admitted_and_at_their_limits():
    for n, _ in S.K3:
        mods, aux, P = R.chain(n, 3)
        assert R.admitted(mods, aux, S.T, n) and P >= max(mods)
    for k in (1, 4):
        mods, aux, P = S.limit_chain(64, k)
        ps = mods + aux + [P]
        assert len(mods) == k and len(aux) == k + 1 and len(set(ps)) == 2 * k + 2 and P == max(ps)
        assert all(E.is_prime(p) and p % 128 == 1 and 1 << 61 < p < 1 << 62 for p in ps) and R.admitted(mods, aux, S.T, 64)
    mods, aux, P = S.mixed_chain(64)
    assert [q.bit_length() for q in mods] == [30, 61] and [b.bit_length() for b in aux] == [30, 61, 62]
    assert len(set(mods + aux + [P])) == 6 and P >= max(mods) and R.admitted(mods, aux, S.T, 64)
    for n, k, batch, _ in S.TWO_PASS:
        mods, aux, P = S.small_chain(n, k)
        assert all(1 << 30 < p < 1 << 62 and p % (2 * n) == 1 for p in mods + aux + [P]) and len(set(mods + aux + [P])) == 2 * k + 2
        assert P >= max(mods) and R.prod(aux) > S.T_BIG * n * R.prod(mods) * sum(map(abs, S.DOT_WEIGHTS)) + 1
    for n, k, _ in S.ALIGN_SHAPES:
        (mods, aux, P), t = S.align_chain(n, k)
        assert R.admitted(mods, aux, t, n) and P >= max(mods)


def test_every_chunk_case_crosses_its_chunk():
    n, k, batch, _, _ = S.DECRYPT_CHUNK
    assert (R.CHUNK_WORDS // n) // k == 10 and S.chunks_of(batch, R.decrypt_chunk_rows(n, k, batch)) == [10, 1]
    assert all(R.decrypt_chunk_rows(n, k, S.decrypt_batch(n, 21)) == S.decrypt_batch(n, 21) for n, k in S.DECRYPT_SHAPES)
    (n14, k14, b14, c14), (n16, k16, b16, c16) = S.TWO_PASS
    assert (R.CHUNK_WORDS // n14) // (7 * (2 * k14 + 1)) == 2 and S.chunks_of(b14, R.chunk_rows(n14, k14, b14)) == c14 == [2, 1]
    assert S.chunks_of(b16, R.chunk_rows(n16, k16, b16)) == c16 == [1, 1]
    for k in (1, 2, 3, 4):                                           # at 2^16 the quotient is 32 / 21 = 1 at k = 1 and zero from k = 2 on: the clamp
        assert (R.CHUNK_WORDS // (1 << 16)) // (7 * (2 * k + 1)) == (1 if k == 1 else 0) and R.chunk_rows(1 << 16, k, 2) == 1
    assert S.chunks_of(5, R.chunk_rows(8192, 4, 5)) == [4, 1] and R.chunk_rows(64, 2, 3) == 3      # the alignment shapes
    r = S.REUSE
    small = r["k"] * R.decrypt_chunk_rows(r["n"], r["k"], r["decrypt_batch"]) * r["n"]
    assert small < 7 * (2 * r["k"] + 1) * R.chunk_rows(r["n"], r["k"], r["mul_batch"]) * r["n"]    # the slot grows between the calls


@pytest.mark.parametrize("n", [64, 256])
def test_sparse_times_dense_is_negacyclic(n):
    case = S.BigCase(n, 3, 2, 9)
    Q = R.prod(case.mods)
    for row in range(2):
        for c in range(2):
            sp = case.sp[0][row][c]
            assert sorted(sp) == [0, 1, n // 2, n - 1] and {abs(sp[0]), abs(sp[1]), abs(sp[n - 1])} == {Q // 2}
            assert all(-(Q // 2) <= int(x) <= Q // 2 for x in case.dense[row, c])
            got = S.sparse_negacyclic(sp, case.dense[row, c])
            assert [int(x) for x in got] == R.negacyclic(S.dense_of(sp, n), [int(x) for x in case.dense[row, c]])
    # the operands' evals are those of the coefficients, every one of them dense, and the tensors are the definition's
    assert R.coeffs_centred(case.mods, n, case.a[:, 0]) == [S.dense_of(case.sp[0][row][0], n) for row in range(2)]
    assert R.coeffs_centred(case.mods, n, case.b[:, 1]) == [[int(x) for x in case.dense[row, 1]] for row in range(2)]
    assert all((case.a[i] != 0).mean() > 0.9 for i in range(3))
    assert np.array_equal(case.tensor(), R.tensor(case.mods, case.t, case.a, case.b))
    import _bfv_dot_numpy as D

    assert np.array_equal(case.tensor(S.DOT_WEIGHTS), D.dot_tensor(case.mods, case.t, [(case.a, case.b), (case.a2, case.b)], S.DOT_WEIGHTS))
