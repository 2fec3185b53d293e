"""The CKKS inner product without a device: the accumulators' overflow argument on edge residues in exact integers,
the proofs of the GPU module's case list, every rejection of the C entry point with fake addresses, the Python scale rule, and the
whole pipeline on the restatement within a bound composed from §22's noise terms, which is below the composed form's bound."""
import numpy as np
import pytest

import _ckks_dot_numpy as DN
import _ckks_eval_numpy as E
import _client_numpy as C

U64 = np.uint64


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


# ---- the kernel's overflow argument, in exact integers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("count", DN.OVERFLOW_COUNTS)
def test_overflow_proof_on_edge_residues(count):
    wide, _ = E.wide_chain(16)
    q61, q62 = E.primes_below(61, 16, 1)[0], E.primes_below(62, 16, 1)[0]
    assert wide[0] >= 1 << 62 and (1 << 60) < q61 < (1 << 61) < q62 < (1 << 62)
    assert (DN.fold_period(q61), DN.fold_period(q62), DN.fold_period(wide[0])) == (4, 4, 1)
    for q in (q61, q62, wide[0]):
        words = [(q - 1,) * 4] * count
        for ws in (None, [q - 1] * count):
            w = 1 if ws is None else q - 1
            want = (count * w % q * (q - 1) * (q - 1) % q, 2 * count * w % q * (q - 1) * (q - 1) % q, count * w % q * (q - 1) * (q - 1) % q)
            assert DN.accumulate(q, words, ws) == want, (q, count)
            ct = np.full((1, 2, 1, 4), q - 1, dtype=U64)
            got = DN.tensor_sum([q], [(ct, ct)] * count, None if ws is None else [[q - 1]] * count)
            assert all((got[0, c] == U64(want[c])).all() for c in range(3))
    # the periods are what 128 bits allow for the constants in use: one more pair of d1's terms would not fit at q - 1
    for q in (q62, wide[0]):
        period = DN.fold_period(q)
        most = 15 if q < 1 << 62 else 3                                       # terms below 2^124 / 2^126 beside a carry-over below q
        assert 2 * period <= most and (q - 1) + most * (q - 1) ** 2 < 1 << 128


def test_accumulate_is_the_exact_sum_on_random_words():
    rng = np.random.default_rng(291)
    wide, _ = E.wide_chain(16)
    for q in (E.primes_below(58, 16, 1)[0], wide[0]):
        for count in (1, 5, DN.GROUP + 3, DN.MAX_COUNT):
            words = [tuple(int(x) for x in rng.integers(0, q, 4, dtype=np.uint64)) for _ in range(count)]
            ws = [int(x) for x in rng.integers(0, q, count, dtype=np.uint64)]
            for w in (None, ws):
                wr = [1] * count if w is None else w
                want = (sum(x * a0 * b0 for x, (a0, a1, b0, b1) in zip(wr, words)) % q,
                        sum(x * (a0 * b1 + a1 * b0) for x, (a0, a1, b0, b1) in zip(wr, words)) % q,
                        sum(x * a1 * b1 for x, (a0, a1, b0, b1) in zip(wr, words)) % q)
                assert DN.accumulate(q, words, w) == want


def test_tensor_sum_of_one_pair_is_the_tensor():
    n, k = 16, 3
    mods, _ = E.chain(n, 58, 40, k - 1)
    a, b = E.case_ct(mods, n, 2, 2, 1), E.case_ct(mods, n, 2, 2, 2)
    assert np.array_equal(DN.tensor_sum(mods, [(a, b)]), E.tensor(mods, a, b))
    assert np.array_equal(DN.tensor_sum(mods, [(a, a)]), E.tensor(mods, a, a))
    two = [E.padd(q, E.tensor(mods, a, b)[i], E.tensor(mods, b, b)[i]) for i, q in enumerate(mods)]
    assert np.array_equal(DN.tensor_sum(mods, [(a, b), (b, b)]), np.stack(two))


# ---- the GPU module's case list ------------------------------------------------------------------------------------------------------------
def test_case_list_covers_every_launch_class(pkg):
    B = pkg.binding
    assert B.FHE_CKKS_DOT_MAX_COUNT == DN.MAX_COUNT == 64
    assert {(n, k) for n, k, _, _ in DN.WORD_CASES} >= {(n, k) for n in (4, 16, 64) for k in (1, 2, 3)} | {(16, 8), (256, 8)}
    assert {b for _, _, b, _ in DN.WORD_CASES} == {1, 3}
    assert set(DN.COUNTS) == {1, 2, 3, DN.GROUP, DN.GROUP + 1, 2 * DN.GROUP + 1} and max(DN.COUNTS) <= DN.MAX_COUNT
    cases = DN.sweep()
    assert {c for c, _ in cases} == set(DN.COUNTS)
    # WEIGHTED on and off, for the first group and for a carried one
    assert {(wt, c > DN.GROUP) for c, wt in cases} == {(False, False), (False, True), (True, False), (True, True)}
    # one group, exactly one full group, two groups, three groups
    assert {-(-c // DN.GROUP) for c, _ in cases} == {1, 2, 3} and DN.GROUP in DN.COUNTS
    # both fold regimes, and in each a group that reaches a fold and one that does not
    regimes = set()
    for n, k, _, spec in DN.WORD_CASES:
        mods, _ = E.case_chain(n, k, spec)
        regimes |= {DN.fold_period(q) for q in mods}
        if spec == "wide":
            assert mods[0] >= 1 << 62 and any(q < 1 << 62 for q in mods)
    assert regimes == {DN.CHUNK // 2, DN.CHUNK63 // 2} == {4, 1}
    for period in regimes:
        assert any(min(c, DN.GROUP) > period for c in DN.COUNTS) and any(c <= period for c in DN.COUNTS)
    # one chunk and two chunks; a launch within 2^20 elements and one past it
    for n, k, b, _ in DN.WORD_CASES:
        assert E.chunk_rows(n, k, b) == b and b * n < E.GRID_CAP
    n, k, b, _ = DN.TWO_CHUNKS
    assert (n, k, b) == (4096, 3, 57) and E.chunk_rows(n, k, b) == 56 == b - 1 and 56 * n < E.GRID_CAP
    n, k, b, _ = DN.PAST_THE_GRID
    assert (n, k, b) == (4096, 1, 301) and E.chunk_rows(n, k, b) == b and b * n > E.GRID_CAP
    assert DN.launch_counts(3, 1) == 3 and DN.launch_counts(3, 16) == 3 and DN.launch_counts(3, 17) == 6 and DN.launch_counts(8, 64) == 32


# ---- rejections that need no device -----------------------------------------------------------------------------------------------------------
def test_rejections_without_a_device(pkg):
    B = pkg.binding
    n = 16
    mods, P = E.chain(n, 58, 40, 2)
    plans, sp = [pkg.Plan(q, n) for q in mods], pkg.Plan(P, n)
    other = pkg.Plan(E.chain(32, 58, 40, 0)[0][0], 32)
    low = pkg.Plan(E.primes_below(57, n, 1)[0], n)                                                     # below q_0: no special prime
    a, b, key, out = 0x10000, 0x40000, 0x80000, 0x400000
    ct_bytes, key_bytes = 3 * 2 * n * 8, 3 * 4 * 2 * n * 8
    one = [1, 1, 1]

    def code(*args, **kw):
        with pytest.raises(B.FheError) as e:
            B.ckks_rns_dot_dev(*args, **kw)
        return e.value.code

    assert code(None, sp, key, 3, [a], [b], None, out, 1, limbs=3) == B.FHE_E_NULL
    assert code([plans[0], None, plans[2]], sp, key, 3, [a], [b], None, out, 1) == B.FHE_E_NULL
    assert code(plans, None, key, 3, [a], [b], None, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, None, 3, [a], [b], None, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, key, 3, None, [b], None, out, 1, count=1) == B.FHE_E_NULL
    assert code(plans, sp, key, 3, [a], None, None, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, key, 3, [a, None], [b, b], None, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, key, 3, [a, a], [b, None], None, out, 1) == B.FHE_E_NULL
    assert code(plans, sp, key, 3, [a], [b], None, None, 1) == B.FHE_E_NULL
    assert code([plans[0], other], sp, key, 3, [a], [b], None, out, 1) == B.FHE_E_PARAM_MISMATCH
    assert code(plans, other, key, 3, [a], [b], None, out, 1) == B.FHE_E_PARAM_MISMATCH
    # the chain conditions of the §22 block
    assert code([plans[0], plans[1], plans[0]], sp, key, 3, [a], [b], None, out, 1) == B.FHE_E_INVALID   # repeated moduli
    assert code(plans, plans[1], key, 3, [a], [b], None, out, 1) == B.FHE_E_INVALID                      # ... the special prime among them
    assert code(plans, low, key, 3, [a], [b], None, out, 1) == B.FHE_E_INVALID                           # P < q_0
    assert code([], sp, key, 3, [a], [b], None, out, 1) == B.FHE_E_INVALID                               # limbs = 0, and 9
    assert code(plans * 3, sp, key, 8, [a], [b], None, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, key, 2, [a], [b], None, out, 1) == B.FHE_E_INVALID                            # key_limbs below limbs, and 9
    assert code(plans, sp, key, 9, [a], [b], None, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, key, 3, [], [], None, out, 1) == B.FHE_E_INVALID                              # count = 0, and 65
    assert code(plans, sp, key, 3, [a] * 65, [b] * 65, None, out, 1) == B.FHE_E_INVALID
    for i, q in enumerate(mods):                                                                         # a weight at its modulus
        w = list(one)
        w[i] = q
        assert code(plans, sp, key, 3, [a], [b], w, out, 1) == B.FHE_E_INVALID
        assert code(plans, sp, key, 3, [a, a], [b, b], one + w, out, 1) == B.FHE_E_INVALID               # ... of the second pair
    assert code(plans, sp, key, 3, [out], [b], None, out, 1) == B.FHE_E_INVALID                          # the output overlaps an operand
    assert code(plans, sp, key, 3, [a], [out], None, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, key, 3, [a, out + ct_bytes - 8], [b, b], None, out, 1) == B.FHE_E_INVALID     # ... of the second pair, in its last word
    assert code(plans, sp, key, 3, [a, a], [b, out - ct_bytes + 8], None, out, 1) == B.FHE_E_INVALID     # ... ending in its first
    assert code(plans, sp, out - key_bytes + 8, 3, [a], [b], None, out, 1) == B.FHE_E_INVALID            # ... or the key
    assert code(plans, sp, out + ct_bytes - 8, 3, [a], [b], None, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, key, 3, [a + 4], [b], None, out, 1) == B.FHE_E_INVALID                        # misaligned buffers
    assert code(plans, sp, key, 3, [a], [b + 4], None, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, key + 4, 3, [a], [b], None, out, 1) == B.FHE_E_INVALID
    assert code(plans, sp, key, 3, [a], [b], None, out + 4, 1) == B.FHE_E_INVALID
    assert code(plans, sp, key, 3, [a], [b], None, out, 1 << 60) == B.FHE_E_INVALID                      # the batch-size limit of mul
    with pytest.raises(B.FheError) as e:
        B.ckks_rns_mul_dev(plans, sp, key, 3, a, b, out, 1 << 60)
    assert e.value.code == B.FHE_E_INVALID
    # the accepted layout sits right beside the output on both sides: only the device is missing (or, with one, nothing is reached:
    # batch = 0 is a no-op whatever the buffers)
    B.ckks_rns_dot_dev(plans, sp, None, 3, [None], [None], one, None, 0)
    B.ckks_rns_dot_dev(plans, sp, out, 3, [out], [out + 4], None, out, 0)
    # and fhe_ckks_rns_workspace_bytes already answers for this call: words_per_row = k^2 + 8k + 2 slabs a ciphertext of the chunk
    for nn, k, batch in ((16, 3, 5), (4096, 3, 57), (4096, 1, 301)):
        rows = E.chunk_rows(nn, k, batch)
        assert B.ckks_rns_workspace_bytes(nn, k, batch) == max((k * k + 8 * k + 2) * rows, 2 * k * E.chunk_rows(nn, k, batch, rescale=True)) * nn * 8


# ---- the Python scale rule ----------------------------------------------------------------------------------------------------------------------
def test_scale_rule(pkg):
    ck = pkg.ckks
    mods, _ = E.chain(16, 58, 40, 2)
    d = 2.0 ** 40
    assert ck.dot_weights([d * d, d * d]) == (d * d, None)                                               # every weight 1: w = None
    assert ck.dot_weights([d * d], [1.0]) == (d * d, None)
    assert ck.dot_weights([d * d, d * d], [1, -2]) == (d * d, [1, -2])
    s = [d * d, d * d / mods[2] * d, 3.0 * d]
    for coeffs, S in (([0.3, -0.7, 1.1], d * d * mods[2]), ([1, 2, 3], None), ([1e-3, 5.0, -2.5], 2.0 ** 90)):
        T, w = ck.dot_weights(s, coeffs, S)
        assert T == (max(s) if S is None else S)
        want, big = DN.weights(coeffs, T, s, mods)
        assert w == big == [round(float(c) * T / x) for c, x in zip(coeffs, s)]                           # exactly the rule's integers
        assert want == [[x % q for q in mods] for x in w]
    assert ck.dot_weights(s, None, None)[1] == [round(max(s) / x) for x in s]                            # unequal pair scales: not all 1
    for bad in ([1j, 1, 1], [float("nan"), 1, 1], [float("inf"), 1, 1], [1, 1], [[1, 1, 1]]):
        with pytest.raises(ValueError):
            ck.dot_weights(s, bad)
    for S in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ck.dot_weights(s, [1, 1, 1], S)


def test_python_surface_without_a_device(pkg):
    ck = pkg.ckks
    n = 16
    mods, P = E.chain(n, 58, 40, 2)
    param = ck.RnsParam(n, mods, P)

    class Rows:                                                               # the shape of a device tensor, without one
        shape = (3, 2, 2, n)
    ct = ck.RnsCiphertext(param, Rows(), 2, 2.0 ** 40)
    rlk = ck.RnsRelinKey(param, None)
    for bad in ([1j], [float("nan")], [float("inf")], [1.0, 2.0]):
        with pytest.raises(ValueError):
            ck.dot([ct], [ct], rlk, bad)
    with pytest.raises(ValueError):
        ck.dot([], [], rlk)
    with pytest.raises(ValueError):
        ck.dot([ct, ct], [ct], rlk)
    with pytest.raises(ValueError):
        ck.dot([ct], [ct], rlk, level=3)
    with pytest.raises(ValueError):
        ck.dot([ct], [ct], rlk, scale=0.0)
    shorter = ck.RnsParam(n, mods[:2], P)
    with pytest.raises(pkg.binding.FheError) as e:
        ck.dot([ct], [ck.RnsCiphertext(shorter, Rows(), 1, 1.0)], rlk)
    assert e.value.code == pkg.binding.FHE_E_PARAM_MISMATCH
    with pytest.raises(pkg.binding.FheError) as e:                            # a key of another chain, as in mul
        ck.dot([ct], [ct], ck.RnsRelinKey(shorter, None))
    assert e.value.code == pkg.binding.FHE_E_PARAM_MISMATCH


# ---- the whole pipeline on the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DN.FUNCTIONAL))
def test_pipeline_accuracy_on_the_restatement(tab, name):
    """measured (this test prints them; worst slot error / bound, the fused and the composed form alike to the digits shown): ones
    1.9e-10 / 7.9e-08, integers 3.3e-10 / 2.4e-07, reals 6.9e-07 / 9.6e-05; of the bound the relinearisations are 9.3e-21 fused
    against 1.9e-20, 5.6e-20 and 2.3e-14 composed"""
    case = DN.FUNCTIONAL[name]
    run = DN.functional_run(case, tab)
    print(f"{name}: count {case['count']}: fused error {run['err']:.3e} bound {run['bound']:.3e}; composed error {run['err_composed']:.3e} bound {run['bound_composed']:.3e}; "
          f"of which the relinearisations {run['relin'][0]:.3e} and {run['relin'][1]:.3e}")
    assert (run["w"] is None) == (name == "ones")
    # one relinearisation term against count of them, each times its weight: the rest of the two bounds is the same sum
    assert run["relin"][0] * sum(abs(x) for x in run["big"]) == pytest.approx(run["relin"][1], rel=1e-12) and run["relin"][0] < run["relin"][1]
    assert run["raw_bounds"][0] < run["raw_bounds"][1]
    assert run["err"] <= run["bound"]
    assert run["err_composed"] <= run["bound_composed"]
    assert np.abs(run["want"]).max() > 0.1 and run["bound"] < 0.1 * np.abs(run["want"]).max()   # the test cannot pass on garbage
    assert not np.array_equal(run["res"], run["comp"])
