"""Buffers that are 8-byte but not 16-byte aligned through the RLWE client paths (bfv_client_kernels.hpp)
and the evaluator's rescale (ckks_eval.hip, §22).  The client ABI promises 8-byte alignment, the transforms take 16-byte
rows, so a misaligned source is copied to the workspace first: every entry point of BFV and CKKS is handed its device
buffers one word past a 16-byte boundary, and its words are those of the restatements (tests/_bfv_client_numpy.py,
tests/_ckks_numpy.py, tests/_ckks_eval_numpy.py; tolerance zero), never those of an aligned call.  Every output sits
between sentinel words, which stay untouched."""
import numpy as np
import pytest

import _bfv_client_numpy as BC
import _ckks_eval_numpy as E
import _ckks_numpy as K
import _client_numpy as C
from conftest import Q16, Q61
from test_bootstrap_gpu import _dev, _u64

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
SEED = bytes((7 * i + 3) % 256 for i in range(32))
FILL = 0x5A5A5A5A5A5A5A5A
RINGS = [(Q16, 16), (Q61, 1024)]
BATCH, T, ROW = 3, 32, (1 << 32) - 2


@pytest.fixture(scope="module")
def tab():
    return C.cdt_table(3.2)


class Offset:
    """`words` device words that start one word past a 16-byte boundary (lead = 2: on one), FILL or the words of x, with
    `lead` sentinel words before them and one after"""

    def __init__(self, shape, x=None, lead=1):
        import torch

        self.words = int(np.prod(shape))
        self.buf = torch.full((lead + self.words + 1,), FILL, dtype=torch.int64, device="cuda")
        self.view = self.buf[lead:lead + self.words].view(shape)
        if x is not None:
            self.view.copy_(_dev(x).view(shape))
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == (8 if lead == 1 else 0)
        self.lead, self.ptr = lead, self.view.data_ptr()

    def get(self):
        """the window's words, after checking the sentinels either side of it"""
        w = _u64(self.buf)
        assert np.all(w[:self.lead] == U64(FILL)) and w[-1] == U64(FILL), "a sentinel word was written"
        return w[self.lead:-1].reshape(tuple(self.view.shape))


def _secret(scheme, n, q):
    """-> (the secret as the restatement takes it, its residues as the device holds them)"""
    if scheme == "bfv":
        s = BC.secret_key(SEED, 0, n)
        return s, s
    s = K.secret_key(SEED, 0, n)
    return s, E.residues(s, q)


def _evals(pkg, q, n, x):
    d, out = _dev(x), _dev(np.zeros(np.shape(x), dtype=U64))
    pkg.Plan(q, n).forward_dev(d.data_ptr(), out.data_ptr(), int(np.size(x)) // n)
    return _u64(out)


@pytest.mark.parametrize("q,n", RINGS)
@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
def test_public_key_from_and_into_misaligned_buffers(pkg, tab, scheme, q, n):
    s, res = _secret(scheme, n, q)
    d_s, d_pk, dt = Offset((n,), res), Offset((2, n)), _dev(tab)
    if scheme == "bfv":
        pkg.binding.bfv_public_key_dev(pkg.Plan(q, n), SEED, ROW, d_s.ptr, dt.data_ptr(), len(tab), d_pk.ptr)
        want = BC.public_key(SEED, ROW, s, q, tab)
    else:
        pkg.binding.ckks_public_key_dev(pkg.Plan(q, n), SEED, ROW, d_s.ptr, dt.data_ptr(), len(tab), d_pk.ptr)
        want = K.public_key(SEED, ROW, s, q, tab)
    assert np.array_equal(d_pk.get(), np.stack(want))
    assert np.array_equal(d_s.get(), res)


@pytest.mark.parametrize("staged", ["0", "1"])
@pytest.mark.parametrize("q,n", RINGS)
@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
def test_encrypt_with_misaligned_key_messages_and_output(pkg, tab, monkeypatch, scheme, q, n, staged):
    """both routes: the staged one broadcasts the misaligned key rows, the pointwise one reads them in its product"""
    rng = np.random.default_rng(n + int(staged))
    pk = rng.integers(0, q, (2, n), dtype=np.uint64)
    d_ev, d_out, dt = Offset((2, n), _evals(pkg, q, n, pk)), Offset((2, BATCH, n)), _dev(tab)
    monkeypatch.setenv(f"FHE_{scheme.upper()}_ENCRYPT_STAGED", staged)
    if scheme == "bfv":
        msg = rng.integers(0, T, (BATCH, n), dtype=np.uint64)
        d_msg = Offset((BATCH, n), msg)
        pkg.binding.bfv_encrypt_dev(pkg.Plan(q, n), T, SEED, ROW, d_ev.ptr, d_msg.ptr, n, dt.data_ptr(), len(tab), d_out.ptr, BATCH)
        c0, c1, _ = BC.encrypt(SEED, ROW, pk[0], pk[1], msg, BATCH, q, T, tab)
    else:
        msg = rng.integers(-(1 << 40), 1 << 40, (BATCH, n), dtype=np.int64)
        d_msg = Offset((BATCH, n), msg.view(U64))
        pkg.binding.ckks_encrypt_dev(pkg.Plan(q, n), SEED, ROW, d_ev.ptr, d_msg.ptr, n, dt.data_ptr(), len(tab), d_out.ptr, BATCH)
        c0, c1 = K.encrypt(SEED, ROW, pk[0], pk[1], msg, BATCH, q, tab)
    got = d_out.get()
    assert np.array_equal(got[0], c0) and np.array_equal(got[1], c1)


@pytest.mark.parametrize("q,n", RINGS)
@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
def test_decrypt_of_misaligned_ciphertexts(pkg, scheme, q, n):
    """batch 3: c0 and c1 are both an odd number of words past the buffer's start, so both are misaligned; c1 goes through
    the copy to the workspace, c0 is read in place by the epilogue"""
    s, res = _secret(scheme, n, q)
    ct = np.random.default_rng(n).integers(0, q, (2, BATCH, n), dtype=np.uint64)
    d_se, d_ct, d_out = _dev(_evals(pkg, q, n, res)), Offset((2, BATCH, n), ct), Offset((BATCH, n))
    assert (d_ct.ptr + BATCH * n * 8) % 16 == 8
    if scheme == "bfv":
        pkg.binding.bfv_decrypt_dev(pkg.Plan(q, n), T, d_se.data_ptr(), d_ct.ptr, d_out.ptr, BATCH)
        want = BC.decrypt(s, ct[0], ct[1], q, T)
    else:
        pkg.binding.ckks_decrypt_dev(pkg.Plan(q, n), d_se.data_ptr(), d_ct.ptr, d_out.ptr, BATCH)
        want = K.decrypt(s, ct[0], ct[1], q).view(U64)
    assert np.array_equal(d_out.get(), want)
    assert np.array_equal(d_ct.get(), ct)


def test_rescale_of_a_misaligned_ciphertext(pkg):
    """n = 16, two limbs, batch 3: the top limb's two components, read by the inverse transform, start 8 bytes past a
    16-byte boundary and are copied to the workspace"""
    n, k = 16, 2
    mods, _ = E.chain(n, 58, 40, k - 1)
    c = E.case_ct(mods, n, BATCH, 2, 91)
    d_in, d_out = Offset(c.shape, c), Offset((k - 1, 2, BATCH, n), lead=2)
    assert (d_in.ptr + (k - 1) * 2 * BATCH * n * 8) % 16 == 8
    pkg.binding.ckks_rns_rescale_dev([pkg.Plan(q, n) for q in mods], d_in.ptr, d_out.ptr, BATCH)
    assert np.array_equal(d_out.get(), E.rescale(mods, c))
    assert np.array_equal(d_in.get(), c)
