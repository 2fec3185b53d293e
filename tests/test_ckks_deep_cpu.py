"""CKKS on a deep RNS chain without a device: the kernel's Garner route equals the CRT definition at the
centring's edges; the restated grouped key switch (tests/_ckks_deep_numpy.py) satisfies r0 + r1 s = d s' + eps with eps under
§36's bound, and at alpha = 1 equals §22's and §23's restatements word for word; the admission either side of P = Q_j; the group
and level bookkeeping; DeepParam's rejections; the boundary; the host tables' own program."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _ckks_deep_numpy as D
import _ckks_eval_numpy as E
import _ckks_galois_numpy as G
import _ckks_numpy as K
import _client_numpy as C

U64 = np.uint64
SEED = bytes((5 * i + 9) % 256 for i in range(32))


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


# ---- the extension -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", range(1, 9))
def test_garner_route_is_the_crt(s):
    """group sizes 1 .. 8, 30-bit primes beside primes just below 2^62 in one group, targets of both sizes"""
    n = 64
    small, big, mid = E.primes_below(30, n, 5), E.primes_below(62, n, 5), E.primes_below(45, n, 4)
    src = [(big, small, mid)[i % 3][i // 3] for i in range(s)]
    dst = [small[4], big[4], mid[3], E.primes_below(55, n, 1)[0]] + src[:1]
    Q = D.product(src)
    rng = random.Random(s)
    xs = [0, 1, Q // 2, Q // 2 + 1, Q - 1] + [rng.randrange(Q) for _ in range(60)]
    res = [np.array([x % m for x in xs], dtype=U64) for m in src]
    want = [[(x - Q if x > Q // 2 else x) % p for x in xs] for p in dst]
    assert D.extend_garner(src, res, dst).tolist() == want
    assert D.extend_crt(src, res, dst).tolist() == want


# ---- the key switch and its noise ------------------------------------------------------------------------------------------------------
def _switch_error(mods, specials, s, key, d2, sprime):
    """eps = r0 + r1 s - d2 s' over the integers modulo Q, centred, for (r0, r1) the key switch of d2 [l][batch][n]"""
    n = len(s)
    t = D.key_switch_sums(mods, specials, key, d2)
    r = D.mod_down(mods, specials, t)
    got, Q = E.phase_int(mods, n, s, r)
    d, _ = E.crt_centred(mods, [E.inv(q, n, d2[i]) for i, q in enumerate(mods)])
    want = d
    for row in sprime:                                               # d s' = d times each factor in turn
        want = E.negacyclic_int(want, row)
    eps = (got - want) % Q
    return np.where(eps > Q // 2, eps - Q, eps)


@pytest.mark.parametrize("L,alpha,l", [(8, 1, 8), (5, 2, 5), (5, 2, 4), (9, 3, 7), (3, 8, 3), (12, 4, 12)])
def test_key_switch_noise_is_under_the_bound(tab, L, alpha, l):
    n = 8
    mods, specials = D.case_chain(n, L, alpha)
    s = K.secret_key(SEED, 0, n)
    assert np.abs(s).max() <= 1
    rlk = D.switch_key(SEED, E.RLK_BASE, s, mods, specials, tab)
    d2 = E.case_ct(mods[:l], n, 2, 1, 40 + L)[:, 0]
    P = D.product(specials)
    ratio = max(D.product(mods[i] for i in g) for g in D.groups(l, alpha)) / P
    assert ratio <= 1
    bound = D.switch_noise_bound(n, l, alpha, ratio)
    eps = _switch_error(mods[:l], specials, s, rlk, d2, [s, s])
    print(f"L={L} alpha={alpha} l={l}: |eps| = {int(np.abs(eps).max())}, bound {bound}")
    assert int(np.abs(eps).max()) <= bound
    g = 5
    gk = D.switch_key(SEED, G.GK_BASE, s, mods, specials, tab, g)
    eps = _switch_error(mods[:l], specials, s, gk, d2, [G.galois_int(s, g)])
    assert int(np.abs(eps).max()) <= bound
    assert D.switch_noise_bound(n, l, 1, 1.0) == E.relin_noise(n, l)  # at alpha = 1 and Q_j = P this is §22's bound


# ---- alpha = 1 is §22 / §23 word for word ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,batch", [(4, 1, 1), (16, 3, 3), (8, 8, 2)])
def test_alpha_one_is_the_single_digit_route(tab, n, k, batch):
    mods, P = E.chain(n, 58, 40, k - 1)
    s = K.secret_key(SEED, 0, n)
    rlk = D.switch_key(SEED, E.RLK_BASE + 64, s, mods, [P], tab)
    assert np.array_equal(rlk, E.relin_key(SEED, E.RLK_BASE + 64, s, mods, P, tab))
    g = 2 * n - 1
    gk = D.switch_key(SEED, G.GK_BASE + 64, s, mods, [P], tab, g)
    assert np.array_equal(gk, G.galois_key(SEED, G.GK_BASE + 64, s, mods, P, tab, g))
    a, b = E.case_ct(mods, n, batch, 2, 3 * n + k), E.case_ct(mods, n, batch, 2, 5 * n + k)
    for l in {k, max(1, k - 1)}:
        assert np.array_equal(D.mul(mods[:l], [P], rlk, a[:l], b[:l]), E.mul(mods[:l], P, rlk, a[:l], b[:l]))
        assert np.array_equal(D.apply_galois(mods[:l], [P], gk, a[:l], g), G.apply_galois(mods[:l], P, gk, a[:l], g))
    assert np.array_equal(D.digits(mods, [P], a[:, 1]), G.digits(mods, P, a[:, 1]))


# ---- admission, groups, levels ---------------------------------------------------------------------------------------------------------
def test_admission_either_side_of_equality():
    n = 8
    q = E.primes_below(40, n, 8)                                     # descending
    p = [q[1], q[2], q[3]]
    assert D.admits([q[4], q[5], q[6]], p) and not D.admits([q[0], q[1], q[2]], p)
    # P = Q_j cannot be met by distinct primes, so equality is held on the comparison itself: the same primes on both sides
    assert D.admits([q[3], q[1], q[2]], p)
    # the smallest step either side of it that primes of this size allow
    assert not D.admits([q[0], q[2], q[3]], p) and D.admits([q[4], q[2], q[1]], p)
    # only the last, partial group decides
    big = E.primes_below(61, n, 2)
    assert D.admits(q[4:7] + [q[7]], p) and not D.admits(q[4:7] + big, p[:2] + [q[0]]) and D.admits(q[4:7] + big[:1], p[:2] + [q[0]])
    # alpha = 1: P >= max q_i
    assert D.admits(q[1:4], [q[0]]) and not D.admits(q[0:3], [q[3]])


def test_groups_and_levels():
    assert [list(g) for g in D.groups(5, 2)] == [[0, 1], [2, 3], [4]]
    assert [list(g) for g in D.groups(4, 2)] == [[0, 1], [2, 3]]
    assert [list(g) for g in D.groups(7, 3)] == [[0, 1, 2], [3, 4, 5], [6]]
    assert [list(g) for g in D.groups(3, 8)] == [[0, 1, 2]]
    assert [list(g) for g in D.groups(32, 1)] == [[i] for i in range(32)]
    assert (D.dnum(17, 8), D.dnum(32, 8), D.dnum(32, 1), D.dnum(3, 8), D.dnum(9, 3)) == (3, 4, 32, 1, 3)
    for L, alpha in ((5, 2), (9, 3), (17, 8), (32, 8)):
        for l in range(1, L + 1):                                    # a level's groups are the key's groups cut at l
            assert [list(g) for g in D.groups(l, alpha)] == [[i for i in g if i < l] for g in D.groups(L, alpha) if g[0] < l]
    # the workspace: alpha = 1 is §22's k^2 + 8k + 2 slabs
    for k in range(1, 9):
        assert D.slabs(k, 1) == k * k + 8 * k + 2
    assert D.workspace_bytes(8192, 12, 4, 2) == 8 * D.slabs(12, 4) * 8192 and D.chunk_rows(8192, 12, 4, 2) == 1
    assert D.workspace_bytes(8, 33, 1, 1) == 0 and D.workspace_bytes(8, 4, 9, 1) == 0 and D.workspace_bytes(8, 4, 0, 1) == 0 and D.workspace_bytes(8, 4, 1, 0) == 0


def test_a_key_serves_every_level(tab):
    """alpha > L and a partial last group: the key made for L limbs switches at every l <= L"""
    n = 8
    s = K.secret_key(SEED, 0, n)
    for L, alpha in ((3, 8), (5, 2)):
        mods, specials = D.case_chain(n, L, alpha)
        rlk = D.switch_key(SEED, E.RLK_BASE, s, mods, specials, tab)
        assert rlk.shape == (D.dnum(L, alpha), L + alpha, 2, n)
        for l in range(1, L + 1):
            d2 = E.case_ct(mods[:l], n, 1, 1, l)[:, 0]
            ratio = max(D.product(mods[i] for i in g) for g in D.groups(l, alpha)) / D.product(specials)
            eps = _switch_error(mods[:l], specials, s, rlk, d2, [s, s])
            assert int(np.abs(eps).max()) <= D.switch_noise_bound(n, l, alpha, ratio)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_deep_param_rejections(pkg):
    ck = pkg.ckks
    n = 8
    mods, specials = D.case_chain(n, 5, 2)
    p = ck.DeepParam(n, mods, specials)
    assert (p.max_level, p.dnum, p.moduli, p.specials) == (4, 3, tuple(mods), tuple(specials))
    assert ck.DeepParam(n, E.primes_below(40, n, 32), E.primes_below(41, n, 8)).dnum == 4
    bad = [
        ([], specials), (E.primes_below(40, n, 33), E.primes_below(41, n, 1)),              # limbs outside [1, 32]
        (mods, []), (mods, E.primes_below(41, n, 9)),                                       # alpha outside [1, 8]
        (mods[:2] + mods[:1], specials), (mods, specials[:1] * 2), (mods[:1], mods[:1]),    # a repeated prime
        (E.primes_below(63, n, 1), E.primes_below(64, n, 1)),                               # a prime of 2^62 or more
        (mods[:1], E.primes_below(63, n, 1)),
        (mods, E.primes_below(39, n, 2)),                                                   # a missed admission
        ([mods[0] + 2], specials),                                                    # not 1 modulo 2n
    ]
    for m, sp in bad:
        with pytest.raises(ValueError):
            ck.DeepParam(n, m, sp)
        with pytest.raises(ValueError):
            D.check_chain(n, m, sp)
    D.check_chain(n, mods, specials)
    # RnsParam keeps its own check
    with pytest.raises(ValueError):
        ck.RnsParam(n, E.primes_below(40, n, 9), E.primes_below(41, n, 1)[0])


def test_boundary(pkg):
    from conftest import ROOT

    B = pkg.binding
    names = ["fhe_ckks_deep_relin_key_dev", "fhe_ckks_deep_galois_key_dev", "fhe_ckks_deep_relinearize_dev", "fhe_ckks_deep_mul_dev", "fhe_ckks_deep_galois_dev",
             "fhe_ckks_deep_rescale_dev"]
    h = open(os.path.join(ROOT, "include", "fhe_ntt.h")).read()
    lib = pkg.load_library()
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\(", h) and name in B.EXPORTS and hasattr(lib, name)
    assert re.search(r"\bsize_t\s+fhe_ckks_deep_workspace_bytes\(", h) and "fhe_ckks_deep_workspace_bytes" in B.EXPORTS
    assert re.search(r"#define\s+FHE_CKKS_DEEP_MAX_LIMBS\s+32\b", h) and re.search(r"#define\s+FHE_CKKS_DEEP_MAX_SPECIALS\s+8\b", h)
    assert (B.FHE_CKKS_DEEP_MAX_LIMBS, B.FHE_CKKS_DEEP_MAX_SPECIALS) == (D.MAX_LIMBS, D.MAX_SPECIALS) == (32, 8)
    assert "ckks_deep.hip" in B.SOURCES and "rns_ext_device.hpp" in B.HEADERS
    mk = open(os.path.join(ROOT, "fhe-study_amd", "host", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bckks_deep\b", mk, re.M) and "san_deep:" in mk
    # the size query needs no device
    for n, l, a, b in ((8, 32, 8, 1), (8192, 12, 4, 2), (4096, 8, 1, 1024), (64, 17, 8, 3), (2, 1, 1, 1)):
        assert B.ckks_deep_workspace_bytes(n, l, a, b) == D.workspace_bytes(n, l, a, b) > 0
    for n, l, a, b in ((8, 33, 1, 1), (8, 0, 1, 1), (8, 4, 9, 1), (8, 4, 0, 1), (8, 4, 1, 0), (12, 4, 1, 1), (1, 4, 1, 1)):
        assert B.ckks_deep_workspace_bytes(n, l, a, b) == 0


def test_host_tables_against_their_definitions(pkg):
    """csrc/rns_tables.hpp's deep_groups, deep_admits and deep_ext_tables against their definitions, and the kernel's route against
    the CRT: fhe-study_amd/host/test_deep_tables.cpp, which needs neither the library nor a GPU"""
    from conftest import ROOT

    host = os.path.join(ROOT, "fhe-study_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_deep_tables"])
    r = subprocess.run([os.path.join(host, "test_deep_tables")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all deep table tests passed" in r.stdout
