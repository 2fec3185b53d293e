"""The case lists of the two-pass CKKS encoder at N = 2^14, 2^15, 2^16: what tests/test_ckks_embed_cpu.py
proves and tests/test_ckks_embed_gpu.py runs on the device.  The embedding is tests/_ckks_numpy.py's FFT form on a table of
root powers that is built once per N (`root_powers_ld` is a Python loop); the CPU module checks that the two agree bit for
bit.  Nothing here calls the library under test."""
import numpy as np

import _ckks_numpy as K

SIZES = [1 << 14, 1 << 15, 1 << 16]
LOG_DELTA = 10
DELTA = float(1 << LOG_DELTA)
# (N, rng seed): p uniform in (-2^20, 2^20), 3 rows, z = decode(p, Delta); the encoder must give p back
EXACT = {1 << 14: 1400, 1 << 15: 1500, 1 << 16: 1600}
# (N, rng seed): z uniform in the square |re|, |im| < 8, 3 rows; no pre-rounding value within E_enc of a half-integer
RANDOM = {1 << 14: 1414, 1 << 15: 1515, 1 << 16: 1616}

_ROOTS, _CASES = {}, {}


def roots_ld(n):
    """K.root_powers_ld(n, n), once per n"""
    if n not in _ROOTS:
        _ROOTS[n] = K.root_powers_ld(n, n)
    return _ROOTS[n]


def roots(n):
    c, s = roots_ld(n)
    return c.astype(np.float64) + 1j * s.astype(np.float64)


def decode(p, delta):
    """K.decode_fft on the cached table"""
    p = np.atleast_2d(np.asarray(p))
    n = p.shape[-1]
    return (np.fft.ifft(p.astype(np.float64) * roots(n), axis=-1) * n)[:, :n // 2] / delta


def encode_pre(z, delta):
    """K.encode_pre's FFT form on the cached table"""
    z = np.atleast_2d(np.asarray(z, dtype=np.complex128))
    n = 2 * z.shape[-1]
    return (np.fft.fft(K.hermitian(z, delta), axis=-1) * np.conj(roots(n))).real / n


def encode(z, delta):
    return K.round_away(encode_pre(z, delta))


def exact_case(n):
    """-> (p [3][n] int64, z [3][n/2]); computed once, shared, never written to"""
    if ("exact", n) not in _CASES:
        p = np.random.default_rng(EXACT[n]).integers(-(1 << 20) + 1, 1 << 20, (3, n), dtype=np.int64)
        z = decode(p, DELTA)
        p.setflags(write=False)
        z.setflags(write=False)
        _CASES["exact", n] = p, z
    return _CASES["exact", n]


def random_case(n):
    """-> (z [3][n/2], K.encode's words [3][n])"""
    if ("random", n) not in _CASES:
        z = K.random_case(n, RANDOM[n], 3)
        want = encode(z, DELTA)
        z.setflags(write=False)
        want.setflags(write=False)
        _CASES["random", n] = z, want
    return _CASES["random", n]
