"""The CKKS encoder at N = 2^14 .. 2^16 on the device (the two-pass kernels of ckks_client.hip): encode exactly
against the case lists tests/test_ckks_embed_cpu.py proved, decode within E_dec of the restatement, the one-pass sizes byte
for byte against the entry points they had, the kernels each size runs, every rejection with its outputs untouched, and
the Python surface end to end at N = 2^14 and 2^16."""
import numpy as np
import pytest

import _ckks_embed_cases as EC
import _ckks_eval_numpy as E
import _ckks_numpy as K
from test_bootstrap_gpu import _u64

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
INVALID = -9
FILL = 0x5A5A5A5A5A5A5A5A
SEED = bytes((11 * i + 5) % 256 for i in range(32))
N14 = 1 << 14


def _empty(shape, fill=FILL):
    import torch

    return torch.full(shape, fill, dtype=torch.int64, device="cuda")


def _i64(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.int64, order="C")).cuda()                  # a copy: the shared cases are read-only


def _cdev(z):
    import torch

    return torch.from_numpy(np.array(z, dtype=np.complex128, order="C").view(np.float64)).cuda()


_TW = {}


def _tw(pkg, n):
    if n not in _TW:
        _TW[n] = _cdev(pkg.binding.ckks_embed_twiddles(n))
    return _TW[n]


def _encode(pkg, n, delta, z, batch, stride=None, fn=None):
    out = _empty((batch, n))
    d_z = _cdev(z)
    (fn or pkg.binding.ckks_embed_encode_dev)(n, delta, _tw(pkg, n).data_ptr(), d_z.data_ptr(), n // 2 if stride is None else stride, out.data_ptr(), batch)
    return out.cpu().numpy()


def _decode(pkg, n, delta, p, batch, fn=None):
    import torch

    out = torch.full((batch, n // 2, 2), float("nan"), dtype=torch.float64, device="cuda")
    d_p = _i64(p)
    (fn or pkg.binding.ckks_embed_decode_dev)(n, delta, _tw(pkg, n).data_ptr(), d_p.data_ptr(), out.data_ptr(), batch)
    return out.cpu().numpy().view(np.complex128).reshape(batch, n // 2)


def _chunk(pkg, n):
    """the polynomials of one pass over the workspace, from the rule of fhe_ckks_embed_workspace_bytes"""
    return pkg.binding.ckks_embed_workspace_bytes(n, 1 << 30) // (8 * n)


def _batches(pkg):
    """(n, batch): 1 and 3 at every size; at 2^14 one batch that crosses into a second, partly filled chunk"""
    assert _chunk(pkg, N14) == 128
    return [(n, b) for n in EC.SIZES for b in (1, 3)] + [(N14, _chunk(pkg, N14) + 1)]


# ---- encode -------------------------------------------------------------------------------------------------------------------
def test_encode_returns_the_constructed_polynomial(pkg):
    for n, batch in _batches(pkg):
        p, z = EC.exact_case(n)
        idx = (np.arange(batch) * 2) % 3
        assert np.array_equal(_encode(pkg, n, EC.DELTA, z[idx], batch), p[idx]), (n, batch)


def test_encode_of_random_slots_is_the_restatement(pkg):
    for n, batch in _batches(pkg):
        z, want = EC.random_case(n)
        idx = (np.arange(batch) * 2) % 3
        assert np.array_equal(_encode(pkg, n, EC.DELTA, z[idx], batch), want[idx]), (n, batch)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("n", EC.SIZES)
def test_encode_strides(pkg, n, kind):
    """both kinds of case: z_stride = 0 is the replicated row (across the chunk boundary at 2^14); an odd stride above n/2"""
    if kind == "exact":
        want, z = EC.exact_case(n)
    else:
        z, want = EC.random_case(n)
    rep = _chunk(pkg, n) + 1 if n == N14 else 5
    assert np.array_equal(_encode(pkg, n, EC.DELTA, z[1:2], rep, stride=0), np.repeat(want[1:2], rep, axis=0))
    stride = n // 2 + 3
    flat = np.zeros(3 * stride, dtype=np.complex128)
    for r in range(3):
        flat[r * stride:r * stride + n // 2] = z[r]
    assert np.array_equal(_encode(pkg, n, EC.DELTA, flat, 3, stride=stride), want)


# ---- decode -------------------------------------------------------------------------------------------------------------------
def test_decode_is_within_the_bound_of_the_restatement(pkg):
    for n, batch in _batches(pkg):
        p = np.random.default_rng(n).integers(-(1 << 40), 1 << 40, (3, n), dtype=np.int64)
        want, bound = EC.decode(p, 1024.0), K.e_dec(p, 1024.0)
        idx = (np.arange(batch) * 2) % 3
        err = np.abs(_decode(pkg, n, 1024.0, p[idx], batch) - want[idx]).max(axis=1)
        print(f"\nN = {n}, batch {batch}: worst decode error {err.max():.3e} against E_dec {bound.min():.3e}")
        assert (err <= bound[idx]).all(), (n, batch)


@pytest.mark.parametrize("n", EC.SIZES)
def test_decode_edge_polynomials(pkg, n):
    """the zero polynomial, the constant 7, 3 X^(N/2) (the fold: i at slot 2k, -i at slot 2k + 1) and words +-2^62"""
    delta = float(1 << 30)
    p = np.zeros((5, n), dtype=np.int64)
    p[1, 0] = 7
    p[2, n // 2] = 3
    sign = np.random.default_rng(62).integers(0, 2, (2, n), dtype=np.int64) * 2 - 1
    p[3], p[4] = sign[0] * (1 << 62), (1 << 62) - np.arange(n)
    got = _decode(pkg, n, delta, p, 5)
    assert not got[0].any() and np.array_equal(got[1], np.full(n // 2, 7 / delta, dtype=np.complex128))
    assert np.array_equal(got[2], np.tile([3j / delta, -3j / delta], n // 4))
    assert (np.abs(got - EC.decode(p, delta)).max(axis=1) <= K.e_dec(p, delta)).all()


# ---- the one-pass sizes and the kernels each size runs --------------------------------------------------------------------------
def _timed(pkg, fn):
    import torch

    B = pkg.binding
    torch.cuda.synchronize()
    B.kernel_timing_enable(True)
    B.kernel_timing_reset()
    try:
        fn()
        torch.cuda.synchronize()
        got = B.kernel_timing_read(64)
    finally:
        B.kernel_timing_enable(False)
    return {name: c for name, (_, c) in got.items() if name.startswith("ckks_")}


@pytest.mark.parametrize("n", [2, 512, 8192])
def test_one_pass_sizes_are_the_old_entry_points(pkg, n):
    B = pkg.binding
    assert np.array_equal(B.ckks_embed_twiddles(n).view(U64), B.ckks_twiddles(n).view(U64))
    z = K.random_case(n, 31 + n, 3)
    p = np.random.default_rng(n).integers(-(1 << 40), 1 << 40, (3, n), dtype=np.int64)
    new_e, old_e = _encode(pkg, n, 1024.0, z, 3), _encode(pkg, n, 1024.0, z, 3, fn=B.ckks_encode_dev)
    new_d, old_d = _decode(pkg, n, 1024.0, p, 3), _decode(pkg, n, 1024.0, p, 3, fn=B.ckks_decode_dev)
    assert np.array_equal(new_e.view(U64), old_e.view(U64)) and np.array_equal(new_d.view(U64), old_d.view(U64))
    assert not (new_e == I64(FILL)).all() and not np.isnan(new_d.view(np.float64)).any()
    lg = n.bit_length() - 1
    d_z, d_p, out = _cdev(z), _i64(p), _empty((3, n))
    tw = _tw(pkg, n).data_ptr()
    assert _timed(pkg, lambda: B.ckks_embed_encode_dev(n, 1024.0, tw, d_z.data_ptr(), n // 2, out.data_ptr(), 3)) == {f"ckks_encode_{lg}": 1}
    assert _timed(pkg, lambda: B.ckks_embed_decode_dev(n, 1024.0, tw, d_p.data_ptr(), out.data_ptr(), 3)) == {f"ckks_decode_{lg}": 1}


def test_two_pass_sizes_run_the_two_passes(pkg):
    """a launch of each pass per chunk"""
    B = pkg.binding
    n = N14
    batch = _chunk(pkg, n) + 1
    d_z, d_p, out = _cdev(np.ones((batch, n // 2), dtype=np.complex128)), _i64(np.ones((batch, n), dtype=np.int64)), _empty((batch, n))
    tw = _tw(pkg, n).data_ptr()
    for b, launches in ((3, 1), (batch, 2)):
        got = _timed(pkg, lambda: B.ckks_embed_encode_dev(n, 1024.0, tw, d_z.data_ptr(), n // 2, out.data_ptr(), b))
        assert got == {"ckks_embed_encode_pass1_14": launches, "ckks_embed_encode_pass2_14": launches}
        got = _timed(pkg, lambda: B.ckks_embed_decode_dev(n, 1024.0, tw, d_p.data_ptr(), out.data_ptr(), b))
        assert got == {"ckks_embed_decode_pass1_14": launches, "ckks_embed_decode_pass2_14": launches}


# ---- rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(pkg):
    import torch

    L = pkg.load_library()
    n, batch = N14, 2
    big = _empty((4 * batch * n,))
    tw, z, msg = _tw(pkg, n), _cdev(np.ones((batch, n // 2), dtype=np.complex128)), _i64(np.zeros((batch, n), dtype=np.int64))
    tw_before = tw.clone()
    cod = lambda **kw: L.fhe_ckks_embed_encode_dev(kw.get("n", n), kw.get("delta", 64.0), tw.data_ptr(), z.data_ptr(), kw.get("stride", n // 2),
                                                   kw.get("out", big.data_ptr()), kw.get("batch", batch), None)
    dcd = lambda **kw: L.fhe_ckks_embed_decode_dev(kw.get("n", n), kw.get("delta", 64.0), tw.data_ptr(), msg.data_ptr(), kw.get("out", big.data_ptr()),
                                                   kw.get("batch", batch), None)
    old = [L.fhe_ckks_encode_dev(n, 64.0, tw.data_ptr(), z.data_ptr(), n // 2, big.data_ptr(), batch, None),
           L.fhe_ckks_decode_dev(n, 64.0, tw.data_ptr(), msg.data_ptr(), big.data_ptr(), batch, None)]
    cases = list(old)
    for f in (cod, dcd):
        cases += [f(n=1 << 17), f(n=24), f(n=1), f(delta=0.0), f(delta=-2.0), f(delta=float("inf")), f(delta=float("nan")), f(out=tw.data_ptr()),
                  f(out=tw.data_ptr() + 8 * (2 * n - 1)), f(batch=1 << 58)]
    cases += [cod(stride=n // 2 - 1), cod(out=z.data_ptr()), cod(out=z.data_ptr() - 8), dcd(out=msg.data_ptr()), dcd(out=msg.data_ptr() + 8 * (batch * n - 1))]
    assert cases == [INVALID] * len(cases)
    assert cod(batch=0) == 0 and dcd(batch=0) == 0
    torch.cuda.synchronize()
    assert (_u64(big) == U64(FILL)).all()
    assert torch.equal(tw, tw_before) and not _u64(msg).any() and (z.cpu().numpy().view(np.complex128) == 1).all()
    assert cod() == 0 and dcd() == 0                                     # and the accepted forms of the same calls run
    torch.cuda.synchronize()
    assert not (_u64(big)[:batch * n] == U64(FILL)).any() and (_u64(big)[batch * n:] == U64(FILL)).all()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def _slots(rng, batch, n):
    r = np.random.default_rng(rng)
    return r.integers(0, 8, (batch, n // 2)).astype(np.float64) + 1j * r.integers(0, 8, (batch, n // 2)).astype(np.float64)


def _rounded(z):
    return K.round_away(z.real) + 1j * K.round_away(z.imag)


def test_client_key_round_trip_multiply_and_rotate_at_16384(pkg):
    """RnsClientKey at n = 2^14 (on the parent commit Encoder.__init__ raises: fhe_ckks_twiddles refuses n): two chain primes
    q_0 < 2^50, q_1 < 2^30 and a special prime, Delta = 2^30, slots with integer parts in [0, 8).

    Rounding the decoded slots is exact on paper.  A fresh ciphertext decrypts to m + e with e = v e_pk + e_0 + e_1 s: v and
    s ternary, the e's Gaussian with sigma = 3.2, so a coefficient of e has standard deviation about sigma sqrt(2 (2n/3) + 1)
    ~ sigma sqrt(n), and a slot, a sum of n coefficients by unit-modulus roots divided by Delta, about sqrt(n) sigma sqrt(n) /
    Delta = 2^14 3.2 / 2^30 ~ 5e-5: 1/2 is ten thousand deviations away.  The encoder's own rounding adds at most
    sqrt(n) / (2 Delta) ~ 6e-8.  The product of two such ciphertexts carries z e' + z' e ~ 2 * 11 * 5e-5 per slot before the
    rescale, and relinearisation and rescale add terms of the order n / q_1 ~ 1.5e-5: far below 1/2 again.  A rotation adds the
    key-switch term only.  No tolerance is tuned: the slots are compared after rounding to integers."""
    ck = pkg.ckks
    n, delta = N14, float(1 << 30)
    mods, P = E.chain(n, 50, 30, 1)
    assert len(mods) == 2 and all((q - 1) % (2 * n) == 0 for q in mods + [P])
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(SEED, param, delta)
    pk, rlk, rk = key.public_key(0), key.relin_key(0), key.rotation_key(1, 0)
    z0, z1 = _slots(141, 2, n), _slots(142, 2, n)
    c0, c1 = key.encode_and_encrypt(pk, z0), key.encode_and_encrypt(pk, z1)
    got = key.decrypt_and_decode(c0)
    print(f"\nfresh: worst slot error {np.abs(got - z0).max():.3e}")
    assert np.array_equal(_rounded(got), z0)
    prod = c0.mul(c1, rlk).rescale()
    got = key.decrypt_and_decode(prod)
    print(f"product: worst slot error {np.abs(got - z0 * z1).max():.3e}")
    assert prod.level == 0 and np.array_equal(_rounded(got), z0 * z1)
    rot = ck.to_rotation_order(key.decrypt_and_decode(c0.rotate(rk)))
    want = np.roll(ck.to_rotation_order(z0), -1, axis=-1)
    print(f"rotation: worst slot error {np.abs(rot - want).max():.3e}")
    assert np.array_equal(_rounded(rot), want)


def test_client_key_round_trip_at_65536(pkg):
    """one chain prime, batch 1; the same derivation gives sqrt(n) sigma sqrt(n) / Delta = 2^16 3.2 / 2^30 ~ 2e-4 per slot"""
    ck = pkg.ckks
    n, delta = 1 << 16, float(1 << 30)
    mods, P = E.chain(n, 50, 30, 0)
    key = ck.RnsClientKey.generate(SEED, ck.RnsParam(n, mods, P), delta)
    z = _slots(161, 1, n)
    got = key.decrypt_and_decode(key.encode_and_encrypt(key.public_key(0), z))
    print(f"\nfresh at 2^16: worst slot error {np.abs(got - z).max():.3e}")
    assert np.array_equal(_rounded(got), z)


def test_encoded_diagonals_at_16384(pkg):
    """RnsClientKey.encode_diagonals and RnsCiphertext.diag_sum at n = 2^14: w' = d_0 w + d_1 roll(w, -1) on the rotation order,
    diagonals with integer parts in [0, 4) encoded at Delta = 2^30, then one rescale.  |w'| < 2 * 4.3 * 9.9 < 90; the noise is that
    of the test above times |d| < 4.3 a term, plus a key switch and a rescale: below 1e-2, and the slots round exactly."""
    ck = pkg.ckks
    n, delta = N14, float(1 << 30)
    mods, P = E.chain(n, 50, 30, 1)
    param = ck.RnsParam(n, mods, P)
    key = ck.RnsClientKey.generate(SEED, param, delta)
    pk, rk = key.public_key(0), key.rotation_key(1, 0)
    r = np.random.default_rng(171)
    d = r.integers(0, 4, (2, n // 2)).astype(np.float64) + 1j * r.integers(0, 4, (2, n // 2)).astype(np.float64)
    z = _slots(172, 1, n)
    pts = key.encode_diagonals(d, [0, 1], 1, delta)
    assert pts.outputs == 1 and pts.level == 1 and pts.gs == [1, ck.galois_element(n, 1)]
    out = key.encode_and_encrypt(pk, z).diag_sum(pts, [None, rk])[0].rescale()
    w = ck.to_rotation_order(z)
    want = d[0] * w + d[1] * np.roll(w, -1, axis=-1)
    got = ck.to_rotation_order(key.decrypt_and_decode(out))
    print(f"\ndiagonal sum: worst slot error {np.abs(got - want).max():.3e}")
    assert out.level == 0 and np.array_equal(_rounded(got), want)
