"""Key generation, encryption and decryption on the device (tfhe_client.hip): the stream, LWE and TGLWE
encryption and the phases word for word against the numpy restatement (tests/_client_numpy.py; tolerance zero), the
rejections, independence from launch geometry, and the evaluator of §11-§16 run end to end on keys and ciphertexts that
ClientKey made on the device."""
import ctypes

import numpy as np
import pytest

import _client_numpy as C
import _gadget_numpy as G
import _lut_numpy as LN
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

SEED = bytes((7 * i + 3) % 256 for i in range(32))
INVALID = -9


def _empty(shape, fill=None):
    import torch

    t = torch.empty(shape, dtype=torch.int64, device="cuda")
    if fill is not None:
        t.fill_(fill)
    return t


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


# ---- the stream -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_row", [0, (1 << 32) - 1])
@pytest.mark.parametrize("row_words", [1, 7, 8, 9, 17])
def test_stream_words_word_exact(pkg, row_words, first_row):
    B = pkg.binding
    for purpose in (C.MASK, C.ERR, C.KEY):
        out = _empty((3, row_words), 0x5A)
        B.tfhe_stream_words_dev(SEED, purpose, first_row, row_words, out.data_ptr(), 3)
        assert np.array_equal(_u64(out), C.stream_words(SEED, purpose, first_row, row_words, 3))
    bits = _empty((3, row_words), 0x5A)
    B.tfhe_stream_words_dev(SEED, C.KEY, first_row, row_words, bits.data_ptr(), 3, bits=True)
    assert np.array_equal(_u64(bits), C.stream_words(SEED, C.KEY, first_row, row_words, 3) & np.uint64(1))


# ---- LWE ------------------------------------------------------------------------------------------------------------------------
def _lwe_dev(pkg, n, first_row, key, mu, tab, log_scale, batch):
    B = pkg.binding
    out = _empty((batch, n + 1), 0x5A)
    dk, dm, dt = _dev(key), (_dev(mu) if mu is not None else None), (_dev(tab) if len(tab) else None)
    B.tlwe_encrypt_dev(n, SEED, first_row, dk.data_ptr(), dm.data_ptr() if dm is not None else None, dt.data_ptr() if dt is not None else None, len(tab),
                       log_scale, out.data_ptr(), batch)
    ph = _empty((batch,), 0x5A)
    B.tlwe_phase_dev(n, dk.data_ptr(), out.data_ptr(), ph.data_ptr(), batch)
    return _u64(out), _u64(ph)


@pytest.mark.parametrize("batch", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 630])
def test_tlwe_encrypt_and_phase_word_exact(pkg, tab, n, batch):
    """the mask words are the restated stream, b - <a, s> - mu is the restated error word, and the phase entry point returns
    mu + e: with log_scale 0, 46 and 63, without errors (m = 0), without messages, and under a random key, the all-ones key
    and the all-zeros key"""
    rng = np.random.default_rng(n * 100 + batch)
    first_row = (1 << 32) - 2                                                 # the batch of 65 crosses into the high nonce word
    mu = rng.integers(0, 1 << 64, batch, dtype=np.uint64, endpoint=False)
    mask = C.stream_words(SEED, C.MASK, first_row, n, batch)
    u = C.stream_words(SEED, C.ERR, first_row, 1, batch)[:, 0]
    keys = {"random": rng.integers(0, 2, n, dtype=np.uint64), "ones": np.ones(n, dtype=np.uint64), "zeros": np.zeros(n, dtype=np.uint64)}
    for kind, t, log_scale, m_ in (("random", tab, 0, mu), ("random", tab, 46, mu), ("random", tab, 63, mu), ("random", tab[:0], 0, mu),
                                   ("ones", tab, 46, mu), ("zeros", tab, 0, mu), ("random", tab, 0, None)):
        key = keys[kind]
        got, phase = _lwe_dev(pkg, n, first_row, key, m_, t, log_scale, batch)
        e = C.errors(t, u, log_scale)
        msg = mu if m_ is not None else np.zeros(batch, dtype=np.uint64)
        assert np.array_equal(got[:, :n], mask), (kind, log_scale)
        assert np.array_equal(got[:, n] - mask @ key - msg, e), (kind, log_scale)
        assert np.array_equal(phase, msg + e), (kind, log_scale)
        want, _ = C.lwe_encrypt(SEED, first_row, key, msg, t, log_scale)
        assert np.array_equal(got, want)
    assert C.errors(tab, u, 0).any() or batch == 1


def test_tlwe_key_words_count_by_their_low_bit_only(pkg, tab):
    """a key is read as 0/1 words: bit 0"""
    rng = np.random.default_rng(5)
    key = rng.integers(0, 1 << 64, 65, dtype=np.uint64, endpoint=False)
    got, phase = _lwe_dev(pkg, 65, 9, key, None, tab, 0, 3)
    want, e = C.lwe_encrypt(SEED, 9, key & np.uint64(1), np.zeros(3, dtype=np.uint64), tab, 0)
    assert np.array_equal(got, want) and np.array_equal(phase, e)


# ---- TGLWE ----------------------------------------------------------------------------------------------------------------------
def _tglwe_dev(pkg, n, first_row, key, msg, stride, tab, log_scale, rows):
    B = pkg.binding
    out = _empty((rows, 2, n), 0x5A)
    dk, dm, dt = _dev(key), (_dev(msg) if msg is not None else None), (_dev(tab) if len(tab) else None)
    B.tglwe_encrypt_dev(n, 1, SEED, first_row, dk.data_ptr(), dm.data_ptr() if dm is not None else None, stride, dt.data_ptr() if dt is not None else None,
                        len(tab), log_scale, out.data_ptr(), rows)
    ph = _empty((rows, n), 0x5A)
    B.tglwe_phase_dev(n, 1, dk.data_ptr(), out.data_ptr(), ph.data_ptr(), rows)
    return _u64(out), _u64(ph)


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("n", [256, 4096])
def test_tglwe_encrypt_and_phase_word_exact(pkg, tab, n, rows):
    """M per row, M broadcast (msg_stride 0) and M null; the mask is the restated stream and B - A S - M the restated errors,
    A S by the tests' numpy negacyclic product; the phase entry point returns M + E"""
    rng = np.random.default_rng(n + rows)
    first_row = (1 << 56) + 11
    S = rng.integers(0, 2, n, dtype=np.uint64)
    M = rng.integers(0, 1 << 64, (rows, n), dtype=np.uint64, endpoint=False)
    mask = C.stream_words(SEED, C.MASK, first_row, n, rows)
    a_s = G.negacyclic(S, mask)
    u = C.stream_words(SEED, C.ERR, first_row, n, rows)
    for msg, stride, t, log_scale in ((M, n, tab, 0), (M[0], 0, tab, 46), (None, 0, tab, 63), (M, n, tab[:0], 0)):
        got, phase = _tglwe_dev(pkg, n, first_row, S, msg, stride, t, log_scale, rows)
        e = C.errors(t, u, log_scale)
        m = np.zeros((rows, n), dtype=np.uint64) if msg is None else np.broadcast_to(msg, (rows, n))
        assert np.array_equal(got[:, 0], mask)
        assert np.array_equal(got[:, 1] - a_s - m, e)
        assert np.array_equal(phase, m + e)
    assert C.errors(tab, u, 0).any()


def test_tglwe_rows_beyond_one_staging_chunk(pkg, tab):
    """N = 256 stages 2^21 / 256 = 8192 rows at a time: 8195 rows with a message per row; the rows around the chunk edge (and
    the last) against the restatement of those rows alone"""
    n, rows, first_row = 256, 8195, 1 << 40
    rng = np.random.default_rng(8195)
    S = rng.integers(0, 2, n, dtype=np.uint64)
    M = rng.integers(0, 1 << 64, (rows, n), dtype=np.uint64, endpoint=False)
    got, phase = _tglwe_dev(pkg, n, first_row, S, M, n, tab, 0, rows)
    for lo, hi in ((0, 2), (8190, 8195)):
        want, e = C.tglwe_encrypt(SEED, first_row + lo, S, M[lo:hi], hi - lo, tab, 0)
        assert np.array_equal(got[lo:hi], want) and np.array_equal(phase[lo:hi], M[lo:hi] + e)


# ---- independence from launch geometry ------------------------------------------------------------------------------------------
def test_split_calls_give_the_words_of_one_call(pkg, tab):
    """rows [0, 65) in one call against [0, 33) and then [33, 65) with first_row = 33, for LWE (n = 630: rows of 631 words, so
    the second call's output starts 8-byte aligned only) and TGLWE (N = 256)"""
    B = pkg.binding
    rng = np.random.default_rng(65)
    n = 630
    key, mu, dt = _dev(rng.integers(0, 2, n, dtype=np.uint64)), _dev(rng.integers(0, 1 << 64, 65, dtype=np.uint64, endpoint=False)), _dev(tab)
    whole, parts = _empty((65, n + 1), 1), _empty((65, n + 1), 2)
    B.tlwe_encrypt_dev(n, SEED, 0, key.data_ptr(), mu.data_ptr(), dt.data_ptr(), len(tab), 0, whole.data_ptr(), 65)
    B.tlwe_encrypt_dev(n, SEED, 0, key.data_ptr(), mu.data_ptr(), dt.data_ptr(), len(tab), 0, parts.data_ptr(), 33)
    B.tlwe_encrypt_dev(n, SEED, 33, key.data_ptr(), mu.data_ptr() + 33 * 8, dt.data_ptr(), len(tab), 0, parts.data_ptr() + 33 * (n + 1) * 8, 32)
    assert np.array_equal(_u64(whole), _u64(parts))
    N = 256
    S, M = _dev(rng.integers(0, 2, N, dtype=np.uint64)), _dev(rng.integers(0, 1 << 64, (65, N), dtype=np.uint64, endpoint=False))
    whole, parts = _empty((65, 2, N), 1), _empty((65, 2, N), 2)
    B.tglwe_encrypt_dev(N, 1, SEED, 0, S.data_ptr(), M.data_ptr(), N, dt.data_ptr(), len(tab), 0, whole.data_ptr(), 65)
    B.tglwe_encrypt_dev(N, 1, SEED, 0, S.data_ptr(), M.data_ptr(), N, dt.data_ptr(), len(tab), 0, parts.data_ptr(), 33)
    B.tglwe_encrypt_dev(N, 1, SEED, 33, S.data_ptr(), M.data_ptr() + 33 * N * 8, N, dt.data_ptr(), len(tab), 0, parts.data_ptr() + 33 * 2 * N * 8, 32)
    assert np.array_equal(_u64(whole), _u64(parts))


def test_tglwe_buffers_need_8_byte_alignment_only(pkg, tab):
    """every buffer 8 bytes off a 16-byte boundary and an odd msg_stride (N + 1 words): the words of the aligned call"""
    B = pkg.binding
    rng = np.random.default_rng(9)
    N, rows, first_row = 256, 3, 77
    S = rng.integers(0, 2, N, dtype=np.uint64)
    M = rng.integers(0, 1 << 64, (rows, N + 1), dtype=np.uint64, endpoint=False)
    want, e = C.tglwe_encrypt(SEED, first_row, S, M[:, :N], rows, tab, 0)
    pad = np.zeros(1, dtype=np.uint64)
    dk, dm, dt = _dev(np.concatenate([pad, S])), _dev(np.concatenate([pad, M.reshape(-1)])), _dev(np.concatenate([pad, tab]))
    out, ph = _empty((1 + rows * 2 * N,), 0x5A), _empty((1 + rows * N,), 0x5A)
    assert dk.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    B.tglwe_encrypt_dev(N, 1, SEED, first_row, dk.data_ptr() + 8, dm.data_ptr() + 8, N + 1, dt.data_ptr() + 8, len(tab), 0, out.data_ptr() + 8, rows)
    B.tglwe_phase_dev(N, 1, dk.data_ptr() + 8, out.data_ptr() + 8, ph.data_ptr() + 8, rows)
    assert np.array_equal(_u64(out)[1:].reshape(rows, 2, N), want) and np.array_equal(_u64(ph)[1:].reshape(rows, N), M[:, :N] + e)
    assert int(_u64(out)[0]) == 0x5A and int(_u64(ph)[0]) == 0x5A
    L = pkg.load_library()
    assert L.fhe_tglwe_phase_dev(N, 1, dk.data_ptr() + 4, out.data_ptr() + 8, ph.data_ptr() + 8, rows, None) == INVALID


# ---- rejections -------------------------------------------------------------------------------------------------------------------
def test_rejections_return_invalid_and_write_nothing(pkg, tab):
    L = pkg.load_library()
    bad_tab = tab.copy()
    bad_tab[7] = bad_tab[6]                                                   # not strictly increasing
    high_tab = tab.copy()
    high_tab[-1] = np.uint64(1 << 63)                                         # not below 2^63
    long_tab = np.arange(1, 1026, dtype=np.uint64)                            # m = 1025
    dt, dbad, dhigh, dlong = _dev(tab), _dev(bad_tab), _dev(high_tab), _dev(long_tab)
    m = len(tab)
    big = _empty((2 * 2 * 8192 + 8192,), 0x5A)                                  # room for 2 rows at the largest n tried, then a key
    key = big.data_ptr() + 2 * 2 * 8192 * 8
    msg = _dev(np.zeros((2, 8192), dtype=np.uint64))

    def tglwe(n, k, table=dt, m_=m, log_scale=0, out=None, d_key=key):
        return L.fhe_tglwe_encrypt_dev(n, k, SEED, 0, d_key, msg.data_ptr(), n, table.data_ptr(), m_, log_scale, out or big.data_ptr(), 2, None)

    def tlwe(n, table=dt, m_=m, log_scale=0, out=None, d_key=key):
        return L.fhe_tlwe_encrypt_dev(n, SEED, 0, d_key, msg.data_ptr(), table.data_ptr(), m_, log_scale, out or big.data_ptr(), 2, None)

    for n in (384, 1000, 128, 8192):                                          # not a power of two; below and above the scope
        assert tglwe(n, 1) == INVALID and L.fhe_tglwe_phase_dev(n, 1, key, msg.data_ptr(), big.data_ptr(), 1, None) == INVALID
    assert tglwe(1024, 2) == INVALID and tglwe(1024, 0) == INVALID
    assert L.fhe_tglwe_phase_dev(1024, 2, key, msg.data_ptr(), big.data_ptr(), 1, None) == INVALID
    assert tglwe(1024, 1, dlong, 1025) == INVALID and tlwe(630, dlong, 1025) == INVALID
    assert tglwe(1024, 1, dbad) == INVALID and tlwe(630, dbad) == INVALID
    assert tglwe(1024, 1, dhigh) == INVALID and tlwe(630, dhigh) == INVALID
    assert tglwe(1024, 1, log_scale=64) == INVALID and tlwe(630, log_scale=64) == INVALID
    assert tlwe(0) == INVALID and L.fhe_tlwe_phase_dev(0, key, msg.data_ptr(), big.data_ptr(), 1, None) == INVALID
    # an output that overlaps the key (its last row ends inside it), the messages, the table
    assert tglwe(1024, 1, d_key=big.data_ptr() + (2 * 2 * 1024 - 8) * 8) == INVALID
    assert tlwe(630, d_key=big.data_ptr() + 2 * 631 * 8 - 8) == INVALID
    assert tglwe(1024, 1, out=msg.data_ptr()) == INVALID and tlwe(630, out=msg.data_ptr()) == INVALID
    assert tlwe(8, out=dt.data_ptr()) == INVALID
    assert L.fhe_tlwe_phase_dev(630, key, big.data_ptr(), big.data_ptr() + 8 * 630, 2, None) == INVALID
    assert L.fhe_tglwe_phase_dev(1024, 1, key, big.data_ptr(), big.data_ptr() + 1024 * 8, 2, None) == INVALID
    # the stream: purpose, flags, row length, a row range past 2^64
    assert L.fhe_tfhe_stream_words_dev(SEED, 0, 0, 8, 0, big.data_ptr(), 1, None) == INVALID
    assert L.fhe_tfhe_stream_words_dev(SEED, 4, 0, 8, 0, big.data_ptr(), 1, None) == INVALID
    assert L.fhe_tfhe_stream_words_dev(SEED, 1, 0, 8, 2, big.data_ptr(), 1, None) == INVALID
    assert L.fhe_tfhe_stream_words_dev(SEED, 1, 0, 0, 0, big.data_ptr(), 1, None) == INVALID
    assert L.fhe_tfhe_stream_words_dev(SEED, 1, 0, (1 << 35) + 1, 0, big.data_ptr(), 1, None) == INVALID
    assert L.fhe_tfhe_stream_words_dev(SEED, 1, (1 << 64) - 1, 8, 0, big.data_ptr(), 2, None) == INVALID
    assert L.fhe_tlwe_encrypt_dev(8, SEED, (1 << 64) - 1, key, None, None, 0, 0, big.data_ptr(), 2, None) == INVALID
    import torch

    torch.cuda.synchronize()
    assert (_u64(big) == 0x5A).all() and not _u64(msg).any() and np.array_equal(_u64(dt), tab)
    # batch = 0 is a no-op, also with NULL buffers
    assert L.fhe_tlwe_encrypt_dev(8, SEED, 0, None, None, None, 0, 0, None, 0, None) == 0
    assert L.fhe_tglwe_encrypt_dev(1024, 1, SEED, 0, None, None, 0, None, 0, 0, None, 0, None) == 0
    assert L.fhe_tfhe_stream_words_dev(SEED, 1, 0, 8, 0, None, 0, None) == 0


# ---- the evaluator on device-made keys and ciphertexts --------------------------------------------------------------------------
N, NL, BSK, KSK, PKS, CBS, PFS, SIGMA = 1024, 630, (8, 3), (4, 4), (8, 4), (6, 2), (8, 4), 3.2


@pytest.fixture(scope="module")
def client(pkg):
    from fhe_study_amd import tfhe

    ck = tfhe.ClientKey.generate(SEED, N, NL, noise=(SIGMA, 0))
    return ck, ck.bootstrapping_key(BSK, KSK)


def _worst_log2(e):
    return float(np.log2(float(max(max(abs(int(x)) for x in np.asarray(e, dtype=object).reshape(-1)), 1))))


def test_client_key_secrets_are_the_key_stream(pkg, client):
    ck, _ = client
    assert np.array_equal(_u64(ck.s_lwe), C.key_bits(SEED, 0, NL)) and np.array_equal(_u64(ck.s_glwe), C.key_bits(SEED, 1, N))
    with pytest.raises(ValueError):
        ck.bootstrapping_key(BSK, KSK)                                        # slot 0 is taken: the rows would repeat


def _square_lookup(tfhe, ck, btk, noise=None):
    t = 3
    x = np.tile(np.arange(8), 8)
    c = ck.encrypt_int(x, t, noise)
    assert list(ck.decrypt_int(c, t)) == list(x)
    lut = tfhe.make_lut(lambda v: v * v % 8, t)
    out = tfhe.lut_bootstrap(btk, t, [lut], [(0, i, tfhe.LUT_NONE, 1, 0, 0) for i in range(64)], c)
    e = (ck.phase(out) - lut[x]).view(np.int64)
    return x, out, e


def test_lut_bootstrap_on_device_made_keys_and_ciphertexts(pkg, client):
    """encrypt_int of all 8 values at t = 3, batch 64, one lut_bootstrap through x -> x^2 mod 8, decrypt_int equals the table"""
    from fhe_study_amd import tfhe

    ck, btk = client
    x, out, e = _square_lookup(tfhe, ck, btk)
    print(f"\nlut_bootstrap on device-built keys: worst |phase error| log2 {_worst_log2(e):.1f} (margin: 2^59)")
    assert list(ck.decrypt_int(out, 3)) == [int(v * v % 8) for v in x]
    assert max(abs(int(v)) for v in e) < 1 << 59


def test_tree_lookup_with_a_device_made_packing_key(pkg, client):
    """all 64 pairs through x y mod 8"""
    from fhe_study_amd import tfhe

    ck, btk = client
    pk = ck.packing_key_switch_key(PKS)
    t, P = 3, 8
    prod = np.array([[int(tfhe.encode_int(x * y % P, t)) for y in range(P)] for x in range(P)], dtype=np.uint64)
    xv, yv = np.repeat(np.arange(P), P), np.tile(np.arange(P), P)
    out = tfhe.tree_lookup(btk, pk, t, prod, ck.encrypt_int(xv, t), ck.encrypt_int(yv, t))
    e = (ck.phase(out) - prod[xv, yv]).view(np.int64)
    print(f"\ntree_lookup on device-built keys: worst |phase error| log2 {_worst_log2(e):.1f} (margin: 2^59)")
    assert list(ck.decrypt_int(out, t)) == [int(a * b % P) for a, b in zip(xv, yv)]


def test_circuit_bootstrap_and_cmux_with_a_device_made_key(pkg, client):
    """8 bits (phase bit 2^63) through one circuit bootstrap; each selects between two trivial TGLWEs in one cmux"""
    from fhe_study_amd import tfhe

    ck, btk = client
    cbk = ck.circuit_bootstrapping_key(btk, CBS, PFS)
    bits = np.array([0, 1, 1, 0, 1, 0, 0, 1])
    c = ck.encrypt_bit(bits, msb=True)
    assert list(ck.decrypt_bit(c, msb=True)) == list(bits)
    sel = tfhe.PreparedTGGSWs(tfhe.circuit_bootstrap(cbk, c, device=True), CBS[0])
    t = 3
    body = np.zeros((2, 8, N), dtype=np.uint64)
    body[0, :, 0], body[1, :, 0] = tfhe.encode_int(3, t), tfhe.encode_int(5, t)
    zero = np.zeros((8, 1, N), dtype=np.uint64)
    out = tfhe.cmux(sel, np.arange(8), tfhe.TGLWE(zero, body[0]), tfhe.TGLWE(zero, body[1]))
    ph = ck.phase(out)                                                        # [8][N]
    want = np.where(bits.astype(bool), tfhe.encode_int(5, t), tfhe.encode_int(3, t)).astype(np.uint64)
    e0, rest = (ph[:, 0] - want).view(np.int64), ph[:, 1:].view(np.int64)
    print(f"\ncircuit bootstrap + cmux on device-built keys: worst |phase error| log2 {_worst_log2(e0):.1f} at coefficient 0, "
          f"{_worst_log2(rest):.1f} elsewhere (margin: 2^59)")
    assert max(abs(int(v)) for v in e0) < 1 << 59 and int(np.abs(rest).max()) < 1 << 59


def test_lut_bootstrap_with_key_noise_3p2_times_2_pow_30(pkg, client):
    """the same lookup with every error of the keys and of the inputs scaled by 2^30 (a second bootstrapping key of the same
    seed, on its own rows: slot 1); tests/test_client_cpu.py checks the decoding margin at a small shape first"""
    from fhe_study_amd import tfhe

    ck, _ = client
    btk = ck.bootstrapping_key(BSK, KSK, noise=(SIGMA, 30), slot=1)
    x, out, e = _square_lookup(tfhe, ck, btk, noise=(SIGMA, 30))
    print(f"\nlut_bootstrap with key noise 3.2 2^30: worst |phase error| log2 {_worst_log2(e):.1f} (margin: 2^59)")
    assert list(ck.decrypt_int(out, 3)) == [int(v * v % 8) for v in x]
    assert max(abs(int(v)) for v in e) < 1 << 59
