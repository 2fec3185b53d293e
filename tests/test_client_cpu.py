"""The client side of DESIGN.md §17 without a device: the numpy ChaCha20 of tests/_client_numpy.py pinned against RFC 8439
and the openssl command-line tool, the stream layout, the properties of the error table in exact rationals, the message
builders (numpy and fhe_study_amd.tfhe's torch expressions, on CPU tensors) against the existing key generators at sigma = 0,
and the CPU check that lookups still decode with key noise 3.2 2^30."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _cb_numpy as CB
import _client_numpy as C
import _gadget_numpy as G
import _lut_numpy as LN
import _pks_numpy as PK
import _tfhe_numpy as R

U64 = np.uint64


# ---- ChaCha20 ---------------------------------------------------------------------------------------------------------------
def test_chacha20_block_is_rfc8439_section_2_3_2():
    key = bytes(range(32))
    out = C.chacha20_blocks(key, [1], [[0x09000000, 0x4A000000, 0]])
    want = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                         "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert out.astype("<u4").tobytes() == want


def test_chacha20_keystream_matches_openssl():
    """`openssl enc -chacha20` takes a 16-byte IV: the 32-bit block counter (little endian), then the 96-bit nonce.  Five blocks
    from counter 0 and from a counter whose low word is about to wrap into nothing the stream layout uses (2^32 - 2: two
    blocks).  Without an openssl binary the test is skipped, visibly: only the RFC vector above then pins the block function."""
    exe = shutil.which("openssl")
    if exe is None:
        pytest.skip("no openssl binary")
    rng = np.random.default_rng(8439)
    for counter, blocks in ((0, 5), (7, 3), ((1 << 32) - 2, 2)):
        key, nonce = rng.bytes(32), rng.bytes(12)
        iv = int(counter).to_bytes(4, "little") + nonce
        got = subprocess.run([exe, "enc", "-chacha20", "-K", key.hex(), "-iv", iv.hex()], input=bytes(64 * blocks), capture_output=True, check=True).stdout
        assert got == C.keystream(key, counter, nonce, 64 * blocks)


def test_stream_layout():
    """word j of block c of a row is u32 word 2j | u32 word 2j + 1 << 32 of ChaCha20(seed, counter c, nonce (purpose, row lo,
    row hi)); rows past 2^32 move into the high nonce word; a shorter row is a prefix of a longer one"""
    seed = bytes(range(100, 132))
    first = (1 << 32) - 1
    w = C.stream_words(seed, C.ERR, first, 17, 3)
    for r in range(3):
        ridx = first + r
        for c in range(3):
            blk = C.chacha20_blocks(seed, [c], [[C.ERR, ridx & 0xFFFFFFFF, ridx >> 32]])[0]
            for j in range(8):
                if 8 * c + j < 17:
                    assert int(w[r, 8 * c + j]) == int(blk[2 * j]) | int(blk[2 * j + 1]) << 32
    assert np.array_equal(C.stream_words(seed, C.ERR, first, 9, 3), w[:, :9])
    assert np.array_equal(C.stream_words(seed, C.ERR, first + 1, 17, 1)[0], w[1])
    assert not np.array_equal(C.stream_words(seed, C.MASK, first, 17, 3), w)
    assert set(C.key_bits(seed, 0, 200)) == {0, 1}


# ---- the error table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [3.2, 1.0, 40.0])
def test_cdt_table_properties(pkg, sigma):
    """strictly increasing, last entry below 2^63, at most ceil(12 sigma) entries; in exact rationals the mean is 0 and the
    variance within 1e-9 of sigma^2, both taken over the signed values that the sampler (C.errors) returns on every interval
    of stream words between two thresholds, for either sign bit.  Why 1e-9 holds with room: for sigma >= 1 the discrete Gaussian's variance differs from
    sigma^2 by O(sigma^4 exp(-2 pi^2 sigma^2)) < 1e-6 at sigma = 1 and < 1e-80 at 3.2 (so sigma = 1 is held to 1e-5), the cut
    at 12 sigma loses mass below exp(-72), and each of the at most 12 sigma thresholds is rounded by at most 2^-64, which
    moves the variance by at most (12 sigma)^3 2^-63 < 1e-12 for sigma = 3.2."""
    from fhe_study_amd import tfhe

    tab = tfhe.cdt_table(sigma)
    assert np.array_equal(tab, C.cdt_table(sigma))
    t = [int(x) for x in tab]
    assert 0 < len(t) <= int(np.ceil(12 * sigma)) and all(a < b for a, b in zip(t, t[1:])) and t[-1] < 1 << 63
    mean, var = C.cdt_moments(tab)
    assert mean == 0
    tol = Fraction(1, 10 ** 9) if sigma >= 3.2 else Fraction(1, 10 ** 5)
    assert abs(var - Fraction(sigma) ** 2) < tol
    if sigma == 3.2:
        print(f"\nsigma = 3.2: {len(t)} thresholds, variance - sigma^2 = {float(var - Fraction(sigma) ** 2):.3e}")


def test_cdt_table_edges(pkg):
    from fhe_study_amd import tfhe

    assert len(tfhe.cdt_table(0)) == 0
    with pytest.raises(ValueError):
        tfhe.cdt_table(-1.0)
    with pytest.raises(ValueError):
        tfhe.cdt_table(100.0)                                                   # 1200 thresholds: more than the kernels take


def test_error_sampler_follows_the_table():
    """the sampler on chosen words: every threshold and its neighbours, both signs, and the shifts 0, 46 and 63"""
    tab = C.cdt_table(3.2)
    r = np.array([0, int(tab[0]) - 1, int(tab[0]), int(tab[0]) + 1, int(tab[5]) - 1, int(tab[5]), int(tab[-1]) - 1, int(tab[-1]), (1 << 63) - 1],
                 dtype=np.uint64)
    mag = [0, 0, 1, 1, 5, 6, len(tab) - 1, len(tab), len(tab)]
    for sign in (0, 1):
        for ls in (0, 46, 63):
            want = [((-m if sign else m) << ls) % (1 << 64) for m in mag]
            assert [int(x) for x in C.errors(tab, (r << U64(1)) | U64(sign), ls)] == want
    assert not C.errors(np.zeros(0, dtype=np.uint64), r, 0).any()
    # and on a stream: the sample variance of 2^16 draws is within 5 % of sigma^2 (a 5 % band is 9 standard errors)
    e = C.errors(tab, C.stream_words(bytes(32), C.ERR, 0, 1 << 16, 1)[0], 0).view(np.int64).astype(np.float64)
    assert abs(e.mean()) < 0.1 and abs(e.var() / 3.2 ** 2 - 1) < 0.05


# ---- message builders against the existing generators at sigma = 0 ----------------------------------------------------------
N, NL = 64, 6                                                                   # the builders know no ring-size limits: small and quick


def _keys():
    rng = np.random.default_rng(17)
    return rng, rng.integers(0, 2, N, dtype=np.uint64), rng.integers(0, 2, NL, dtype=np.uint64)


def _mul(a, x):
    """the generators' mul(a [r][n], x [r][n]); every row of x is the one GLWE key here"""
    assert (x == x[0]).all()
    return G.negacyclic(x[0], a)


def _torch_words(t):
    return t.numpy().view(np.uint64)


@pytest.mark.parametrize("b,l", [(8, 3), (1, 3), (16, 4), (32, 2)])
def test_message_builders_give_the_phases_of_the_existing_generators(pkg, b, l):
    """at sigma = 0 a generated key's phase IS its message: G.tggsw_bits, G.ksk, CB.pfksk and PK.pksk against the numpy builders
    and against fhe_study_amd.tfhe's torch builders (CPU tensors)"""
    from fhe_study_amd import tfhe

    rng, S, s = _keys()
    bsk = G.tggsw_bits(rng, _mul, N, b, l, S, s, 0)
    want = CB.tglwe_phase(_mul, bsk, S)                                        # [n_lwe][2][l][N]
    assert want.any() and np.array_equal(C.bsk_messages(S, s, b, l), want)
    assert np.array_equal(_torch_words(tfhe.bsk_messages(S, s, b, l)), want)
    ksk = G.ksk(rng, S, s, b, l, 0)
    want = CB.tlwe_phase(ksk, s)                                               # [N][l]
    assert np.array_equal(C.ksk_messages(S, b, l), want) and np.array_equal(_torch_words(tfhe.ksk_messages(S, b, l)), want)
    pf = CB.pfksk(rng, _mul, N, S, b, l, 0)
    want = CB.tglwe_phase(_mul, pf, S)                                         # [2][N + 1][l][N]
    assert np.array_equal(C.pfksk_messages(S, b, l), want) and np.array_equal(_torch_words(tfhe.pfksk_messages(S, b, l)), want)
    pk = PK.pksk(rng, _mul, N, s, S, b, l, 0)
    want = CB.tglwe_phase(_mul, pk, S)                                         # [n_lwe][l][N]
    assert np.array_equal(C.pksk_messages(s, N, b, l), want) and np.array_equal(_torch_words(tfhe.pksk_messages(s, N, b, l)), want)


def test_samples_and_phases_of_the_restatement():
    """the restated samples decrypt to mu + e and M + E, and a split batch equals the whole"""
    seed, tab = bytes(range(32)), C.cdt_table(3.2)
    rng, S, s = _keys()
    mu = rng.integers(0, 1 << 64, 5, dtype=np.uint64, endpoint=False)
    c, e = C.lwe_encrypt(seed, 10, s, mu, tab, 46)
    assert e.any() and np.array_equal(C.lwe_phase(c, s), mu + e)
    assert np.array_equal(C.lwe_encrypt(seed, 12, s, mu[2:], tab, 46)[0], c[2:])
    M = rng.integers(0, 1 << 64, (3, N), dtype=np.uint64, endpoint=False)
    t, E = C.tglwe_encrypt(seed, 1 << 40, S, M, 3, tab, 0)
    assert E.any() and np.array_equal(C.tglwe_phase(t, S), M + E)
    assert np.array_equal(C.tglwe_encrypt(seed, 1 << 40, S, None, 3, tab, 0)[0][:, 0], t[:, 0])      # the mask does not depend on M


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_header_binding_and_design_name_the_client_entry_points(pkg):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "fhe_ntt.h")) as f:
        h = f.read()
    for name in ("fhe_tfhe_stream_words_dev", "fhe_tlwe_encrypt_dev", "fhe_tlwe_phase_dev", "fhe_tglwe_encrypt_dev", "fhe_tglwe_phase_dev"):
        assert re.search(r"\bint\s+" + name + r"\(", h) and name in pkg.binding.EXPORTS
    assert "tfhe_client.hip" in pkg.binding.SOURCES
    with open(os.path.join(root, "DESIGN.md")) as f:
        d = f.read()
    assert re.search(r"^## 17\b", d, re.M) or re.search(r"^#+ *§? ?17", d, re.M)


def test_row_ranges_of_the_key_builders_do_not_meet(pkg):
    """every builder's rows at the production shape, slot 0 and slot 2^16 - 1, stay inside its own 2^56 range and slots of
    2^40 rows do not run into each other"""
    from fhe_study_amd import tfhe

    K = tfhe.ClientKey
    n, n_lwe = 4096, 1 << 20                                                    # far beyond any shape the evaluator takes
    need = {"bsk+ksk": n_lwe * 2 * 64 + n * 64, "pfksk": 2 * (n + 1) * 64, "pksk": n_lwe * 64}
    assert max(need.values()) <= K.SLOT_ROWS and (1 << 16) * K.SLOT_ROWS <= 1 << 56
    assert K.ENCRYPT_ROWS <= K.BSK_BASE < K.PFKSK_BASE < K.PKSK_BASE and K.PKSK_BASE + (1 << 56) <= 1 << 64
    assert K.PFKSK_BASE - K.BSK_BASE >= 1 << 56 and K.PKSK_BASE - K.PFKSK_BASE >= 1 << 56


# ---- larger key noise: decoding on the CPU first ------------------------------------------------------------------------------
def test_lookup_decodes_with_key_noise_3p2_times_2_pow_30_at_a_small_shape():
    """The GPU test repeats its lookup with every key error scaled by 2^30.  Here the numpy gadget bootstrap runs x -> x^2 mod
    8 at N = 256, n_lwe = 8, BSK (8, 3), KSK (4, 4) with keys of the restatement at sigma = 3.2, log_scale = 30, on all 8
    values: every output decodes, and with margin: the worst phase error, printed, stays below 2^56, an eighth of the decoding
    bound Delta / 2 = 2^59 (three bits: what one more lookup level of equal error, or a doubling of sigma twice over, would use).
    Expected size: a CMux step adds about (2 l N)^(1/2) 2^7 sigma 2^30 ~ 2^44, n_lwe = 8 steps 2^45.5; the key switch adds
    (N ks_l)^(1/2) 2^3 sigma 2^30 ~ 2^40 and its own rounding, 2^47 N^(1/2) / 3 ~ 2^49.5, which the key noise does not change.
    At the GPU test's shape (N = 1024, n_lwe = 630) the same sums give about 2^50 for the BSK term: nine bits of margin."""
    n, n_lwe, t = 256, 8, 3
    seed, tab = bytes(range(1, 33)), C.cdt_table(3.2)
    S, s = C.key_bits(seed, 1, n), C.key_bits(seed, 0, n_lwe)
    (b, l), (kb, kl) = (8, 3), (4, 4)
    rows, _ = C.tglwe_encrypt(seed, 1 << 56, S, C.bsk_messages(S, s, b, l).reshape(-1, n), n_lwe * 2 * l, tab, 30)
    ksk, _ = C.lwe_encrypt(seed, (1 << 56) + n_lwe * 2 * l, s, C.ksk_messages(S, kb, kl).reshape(-1), tab, 30)
    bsk, ksk = rows.reshape(n_lwe, 2, l, 2, n), ksk.reshape(n, kl, n_lwe + 1)
    x = np.arange(8)
    c, _ = C.lwe_encrypt(seed, 0, s, [LN.encode(v, t) for v in x], tab, 30)
    lut = LN.table(lambda v: v * v % 8, t)
    out = G.bootstrap(n, 1, b, l, bsk, LN.expand(lut, n), kb, kl, ksk, c)
    e = LN.phase_error(out, s, lut[x])
    worst = max(abs(int(v)) for v in e)
    print(f"\nkey noise 3.2 2^30 at N = 256, n_lwe = 8: worst |phase error| log2 {np.log2(max(worst, 1)):.1f} (decoding bound 2^59, asserted below 2^56)")
    assert list(LN.decode(LN.phases(out, s), t)) == [int(v * v % 8) for v in x]
    assert worst < 1 << 56
