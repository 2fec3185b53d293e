"""BFV on an RNS modulus chain without a device: the route the kernels take — Garner's digits, the comparison
against the digits of floor(M / 2), steps 3 and 4 of the scaled product, the decryption with one auxiliary prime — equals the
integer definition at the edges of the admission bound; the parameter checks either side of that bound; the batch encoder."""
import os
import random
import subprocess

import numpy as np
import pytest

import _bfv_rns_numpy as R
import _ckks_eval_numpy as E


def _edges(M):
    return [0, 1, M - 1, M // 2, M // 2 + 1, M // 2 - 1, M // 3]


@pytest.mark.parametrize("s,t", [(1, 2), (2, 3), (3, 2), (4, 5), (5, 4), (9, 9)])
@pytest.mark.parametrize("centred", [False, True])
def test_garner_route_is_the_crt(s, t, centred):
    ps = E.primes_below(61, 8, s + t)
    src, dst = ps[:s], ps[s:]
    M = R.prod(src)
    rng = random.Random(17 * s + t)
    for x in _edges(M) + [rng.randrange(M) for _ in range(40)]:
        res = [x % m for m in src]
        want = [(R.centre(x, M) if centred else x) % p for p in dst]
        assert R.garner_extend(src, dst, res, centred) == want
        assert [int(v) for v in R.extend(src, dst, np.array(res, dtype=np.uint64)[:, None], centred)[:, 0]] == want


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("n,t", [(8, 65537), (2048, 65537), (64, 257)])
def test_scale_round_route_is_the_definition(k, n, t):
    mods, aux, _ = R.chain(n, k)
    Q = R.prod(mods)
    assert R.admitted(mods, aux, t, n)
    top = n * Q * Q // 2
    rng = random.Random(1000 * k + n)
    ds = [top, -top, 0, top - 1, 1 - top]
    for mult in (0, 1, -1, 7, -7, top // Q, -(top // Q) + 1):
        ds += [mult * Q + e for e in (0, 1, Q // 2, Q // 2 + 1) if abs(mult * Q + e) <= top]
    ds += [rng.randrange(-top, top + 1) for _ in range(60)]
    for d in ds:
        want = R.scale_round(d, t, Q)
        assert R.route_scale_round(mods, aux, t, d) == [want % q for q in mods], d


@pytest.mark.parametrize("k", [1, 2, 4])
def test_decrypt_route_is_the_definition(k):
    n, t = 64, 257
    mods, aux, _ = R.chain(n, k)
    Q = R.prod(mods)
    rng = random.Random(k)
    small = E.primes_below(11, n, 3)                                 # b_0 just above 2 t + 2 as well
    b_small = min(p for p in small if p > 2 * t + 2)
    for b0 in (aux[0], b_small):
        for v in [Q // 2, -(Q // 2), 0, 1, -1, Q // 2 - 1, 1 - Q // 2] + [rng.randrange(-(Q // 2), Q // 2 + 1) for _ in range(60)]:
            assert R.route_decrypt(mods, b0, t, v) == R.scale_round(v, t, Q) % t, v


def test_negacyclic_packed_equals_schoolbook():
    rng = random.Random(5)
    n, B = 128, 1 << 200
    a, b = [rng.randrange(-B, B + 1) for _ in range(n)], [rng.randrange(-B, B + 1) for _ in range(n)]
    c = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                c[i + j] += x * y
            else:
                c[i + j - n] -= x * y
    assert R.negacyclic(a, b) == c
    assert R.negacyclic([B] * n, [-B] * n)[n - 1] == -n * B * B


def test_tensor_reaches_the_bound():
    """the all-(floor(Q / 2)) and all-(floor(Q / 2) + 1) rows: |d1| touches n Q^2 / 2 up to the rounding of Q / 2"""
    n, k, t = 8, 2, 65537
    mods, aux, _ = R.chain(n, k)
    Q = R.prod(mods)
    half = [Q // 2] * n
    d1 = [2 * x for x in R.negacyclic(half, half)]
    assert max(map(abs, d1)) == 2 * n * (Q // 2) ** 2 <= n * Q * Q // 2
    assert R.route_scale_round(mods, aux, t, d1[n - 1]) == [R.scale_round(d1[n - 1], t, Q) % q for q in mods]


def test_param_checks_either_side_of_the_bound(pkg):
    bfv = pkg.bfv

    n, k = 64, 2
    mods, aux, P = R.chain(n, k, bq=40, bb=41)
    Q, B = R.prod(mods), R.prod(aux)
    t_edge = (B - 2) // (n * Q)                                      # the largest t with B > t n Q + 1
    assert B > t_edge * n * Q + 1 and not B > (t_edge + 1) * n * Q + 1
    assert bfv.RnsParam(n, mods, aux, P, t_edge).t == t_edge
    with pytest.raises(ValueError):
        bfv.RnsParam(n, mods, aux, P, t_edge + 1)
    assert R.admitted(mods, aux, t_edge, n) and not R.admitted(mods, aux, t_edge + 1, n)
    ok = dict(n=n, moduli=mods, aux=aux, special=P, t=257)
    bfv.RnsParam(**ok)
    for bad in (dict(aux=aux[:k]), dict(moduli=mods + [aux[0]]), dict(aux=[mods[0]] + aux[1:]), dict(special=mods[0]), dict(t=1), dict(n=48),
                dict(moduli=[mods[0], mods[1] + 2 * n]), dict(special=E.primes_below(30, n, 1)[0]),
                dict(moduli=E.primes_below(50, n, 5), aux=E.primes_below(61, n, 6))):
        with pytest.raises(ValueError):
            bfv.RnsParam(**dict(ok, **bad))
    with pytest.raises(ValueError):
        bfv.BatchEncoder(n, 259)
    with pytest.raises(ValueError):
        bfv.BatchEncoder(n, 193)                                     # prime, but not 1 modulo 2n


def test_sources_and_exports(pkg):
    assert "bfv_rns.hip" in pkg.binding.SOURCES and "rns_tables.hpp" in pkg.binding.HEADERS
    for name in ("fhe_rns_extend_dev", "fhe_bfv_rns_tensor_dev", "fhe_bfv_rns_mul_dev", "fhe_bfv_rns_workspace_bytes", "fhe_bfv_rns_scale_msg_dev",
                 "fhe_bfv_rns_decrypt_dev"):
        assert name in pkg.binding.EXPORTS


@pytest.mark.parametrize("n,t", [(8, 17), (64, 257)])
def test_encoder_round_trip_and_permutations(pkg, n, t):
    bfv = pkg.bfv

    assert np.array_equal(bfv.slot_index(n), R.slot_index(n))
    assert sorted(R.slot_index(n).reshape(-1).tolist()) == list(range(n))
    rng = np.random.default_rng(n)
    slots = rng.integers(0, t, (2, n // 2))
    m = R.encode(n, t, slots)
    assert np.array_equal(R.decode(n, t, m), slots.astype(np.uint64))
    for step in (1, n // 2 - 1, 3 % (n // 2)):
        rot = R.decode(n, t, R.galois_coeffs(n, t, m, pow(5, step, 2 * n)))
        assert np.array_equal(rot, np.roll(slots, -step, axis=1).astype(np.uint64))
    swapped = R.decode(n, t, R.galois_coeffs(n, t, m, 2 * n - 1))
    assert np.array_equal(swapped, slots[::-1].astype(np.uint64))
    # the slots multiply pointwise: the ring product of two encodings decodes to the product of the slot matrices
    other = rng.integers(0, t, (2, n // 2))
    pm = [x % t for x in R.negacyclic(m.tolist(), R.encode(n, t, other).tolist())]
    assert np.array_equal(R.decode(n, t, np.array(pm, dtype=np.uint64)), (slots * other % t).astype(np.uint64))


def test_host_tables_against_their_definitions(pkg):
    """csrc/rns_tables.hpp (Garner's inverses, the digits of floor(M / 2), the weights, the multi-word integers) against its
    definitions and the route against x mod p: fhe-study_amd/host/test_rns_tables.cpp, which needs neither the library nor a GPU"""
    from conftest import ROOT

    host = os.path.join(ROOT, "fhe-study_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_rns_tables"])
    r = subprocess.run([os.path.join(host, "test_rns_tables")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all rns table tests passed" in r.stdout
