"""Host mirror of the reference's torus products (arith/src/ring_torus.rs, tfhe/src/tggsw.rs)
over the C ABI.

    reference (Rust)                                   here
    Tn * Tn           ring_torus.rs:251-298            Tn.__mul__
    Tn::decompose     ring_torus.rs:67-77              (inside the external product, on the GPU)
    TGLWE(GLWE<Tn>)   tfhe/src/tglwe.rs:33             TGLWE(a [k][n], b [n])
    TGLWE * Tn        tfhe/src/tglwe.rs:182-194        TGLWE.__mul__
    TGLev * Vec<Tn>   tfhe/src/tggsw.rs:139-149        TGLev.__mul__
    TGGSW * TGLWE     tfhe/src/tggsw.rs:45-62          TGGSW.__mul__   (beta = 2, l = 64 as there)
    TGLWE::left_rotate, sample_extraction   tglwe.rs:89-118     TGLWE.left_rotate, TGLWE.sample_extraction
    TLWE::key_switch  tfhe/src/tlwe.rs:101-111         TLWE.key_switch (beta = 2)
    BootstrappingKey  tlwe.rs:163-167                  BootstrappingKey (device-resident: prepared BSK + KSK)
    blind_rotation, bootstrapping   tlwe.rs:121-161    blind_rotation, bootstrapping (the mod switch
                                                       rounds to 2N, and the CMux loop runs over all n_lwe key bits)
    (no counterpart)                                   the signed base-2^b gadget of DESIGN.md §11: gadget_decompose,
                                                       gadget_external_product, BootstrappingKey(log_beta=...),
                                                       TLWE.key_switch(log_beta=...)
"""
import numpy as np

from . import binding


class Tn:
    """element of T_{2^64}[X]/(X^n+1): u64 coefficients, arithmetic wraps (torus.rs:80-153)"""

    def __init__(self, coeffs):
        self.coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)

    @property
    def n(self):
        return self.coeffs.shape[-1]

    def __mul__(self, rhs):
        """naive_poly_mul, ring_torus.rs:266-298"""
        if rhs.n != self.n:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "Tn operands differ in n")
        return Tn(binding.tn_mul(self.n, self.coeffs, rhs.coeffs).reshape(self.coeffs.shape))

    def __eq__(self, other):
        return isinstance(other, Tn) and np.array_equal(self.coeffs, other.coeffs)


class TGLWE:
    """(a_0..a_{k-1}, b): `a` is (k, n), `b` is (n,) — or batches with a leading axis"""

    def __init__(self, a, b):
        self.a = np.ascontiguousarray(a, dtype=np.uint64)
        self.b = np.ascontiguousarray(b, dtype=np.uint64)

    def packed(self):
        return np.concatenate([self.a, self.b[..., None, :]], axis=-2)   # [.., k+1, n]

    def __mul__(self, plaintext):
        """plaintext multiplication, tglwe.rs:182-194: every component times the Tn"""
        x = self.packed()
        k = x.shape[-2] - 1
        out = binding.tglwe_mul_tn(plaintext.n, k, x, plaintext.coeffs).reshape(x.shape)
        return TGLWE(out[..., :k, :], out[..., k, :])

    def left_rotate(self, h):
        """multiply by X^-h, h < 2n (ring_torus.rs:118-132 for h < n; h >= n also negates)"""
        n = self.b.shape[-1]
        j = np.arange(n) + int(h) % (2 * n)
        sign = (j // n) % 2 == 1
        rot = lambda x: np.where(sign, np.uint64(0) - x[..., j % n], x[..., j % n]).astype(np.uint64)
        return TGLWE(rot(self.a), rot(self.b))

    def sample_extraction(self, h):
        """TLWE of dimension k n holding coefficient h of the phase (tglwe.rs:89-115), on the device"""
        torch = _torch()
        x = self.packed()
        k1, n = x.shape[-2], x.shape[-1]
        batch = x.size // (k1 * n)
        d_in = _to_dev(x)
        out = torch.empty((batch, (k1 - 1) * n + 1), dtype=torch.int64, device="cuda")
        binding.tglwe_sample_extraction_dev(n, k1 - 1, h, d_in.data_ptr(), out.data_ptr(), batch)
        return TLWE(_from_dev(out).reshape(x.shape[:-2] + ((k1 - 1) * n + 1,)))


class TGLev:
    """l TGLWEs (tggsw.rs:65): rows [l][(k+1)][n]"""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64)

    def __mul__(self, v):
        """dot product with a Vec<Tn> (usually a decomposition), tggsw.rs:139-149"""
        l, k1, n = self.rows.shape
        if len(v) != l:
            raise binding.FheError(binding.FHE_E_INVALID, "TGLev * Vec<Tn>: lengths differ")   # assert_eq!, :143
        vv = np.stack([t.coeffs for t in v])
        out = binding.tglev_mul(n, k1 - 1, l, self.rows, vv)[0]
        return TGLWE(out[: k1 - 1], out[k1 - 1])


class TGGSW:
    """([k x TGLev], TGLev), each TGLev = l TGLWEs (tggsw.rs:12-14): rows[(k+1)][l][(k+1)][n]"""
    BETA, L = 2, 64   # hard-coded in the reference's external product (tggsw.rs:49-50)

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64)
        k1, l, k1b, _ = self.rows.shape
        if k1 != k1b:
            raise ValueError("rows must be [(k+1)][l][(k+1)][n]")

    def __mul__(self, tglwe):
        """external product, tggsw.rs:45-62"""
        k1, l, _, n = self.rows.shape
        x = tglwe.packed()
        out = binding.tggsw_external_product(n, k1 - 1, l, self.rows, x).reshape(x.shape)
        return TGLWE(out[..., : k1 - 1, :], out[..., k1 - 1, :])


# ---- TFHE bootstrapping (tfhe/src/tlwe.rs) ----------------------------------------------------------------------
def _torch():
    import torch

    return torch


def _to_dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def _from_dev(t):
    return t.cpu().numpy().view(np.uint64)


class TLWE:
    """LWE ciphertexts [a_0 .. a_{m-1}, b]: `words` is (m + 1,) or (batch, m + 1)"""

    def __init__(self, words):
        self.words = np.ascontiguousarray(words, dtype=np.uint64)

    @property
    def dim(self):
        return self.words.shape[-1] - 1

    def key_switch(self, ksk, l, beta=2, *, log_beta=None):
        """tlwe.rs:101-111: ksk [n_in][l][n_out + 1] (numpy or a device tensor) -> TLWE of dimension n_out.
        log_beta = b: the signed base-2^b gadget of DESIGN.md §11 (level d of the KSK holds s_in[i] 2^(64 - b(d+1)))"""
        torch = _torch()
        k = ksk if isinstance(ksk, torch.Tensor) else _to_dev(ksk)
        n_in, n_out = self.dim, k.shape[-1] - 1
        x = self.words.reshape(-1, n_in + 1)
        out = torch.empty((x.shape[0], n_out + 1), dtype=torch.int64, device="cuda")
        dx = _to_dev(x)                  # device buffers are held until the call returns: never a freed temporary's pointer
        if log_beta is None:
            binding.tlwe_key_switch_dev(n_in, n_out, beta, l, k.data_ptr(), dx.data_ptr(), out.data_ptr(), x.shape[0])
        else:
            binding.tlwe_gadget_key_switch_dev(n_in, n_out, log_beta, l, k.data_ptr(), dx.data_ptr(), out.data_ptr(), x.shape[0])
        return TLWE(_from_dev(out).reshape(self.words.shape[:-1] + (n_out + 1,)))


class BootstrappingKey:
    """(Vec<TGGSW>, KSK) of tlwe.rs:163-167 kept on the device: the n_lwe bit-TGGSWs [n_lwe][(k+1)][l][(k+1)][n]
    prepared once (fhe_tfhe_bsk_prepare_dev), and the KSK [k n][ks_l][n_lwe + 1] back to the LWE key.
    log_beta = b: both keys use the signed base-2^b gadget of DESIGN.md §11 (BSK base 2^log_beta with l levels, KSK base
    2^ks_log_beta with ks_l levels); ks_log_beta is then required."""

    def __init__(self, n, k, l, n_lwe, bsk, ksk, ks_l=64, *, log_beta=None, ks_log_beta=None):
        torch = _torch()
        if (log_beta is None) != (ks_log_beta is None):
            raise ValueError("log_beta and ks_log_beta go together: the gadget bootstrap needs both")
        self.n, self.k, self.l, self.n_lwe, self.ks_l = n, k, l, n_lwe, ks_l
        self.log_beta, self.ks_log_beta = log_beta, ks_log_beta
        if log_beta is None:
            words = binding.tfhe_bsk_prepared_words(n, k, l, n_lwe)
        else:
            words = binding.tfhe_gadget_bsk_prepared_words(n, k, log_beta, l, n_lwe)
        if words == 0:
            raise binding.FheError(binding.FHE_E_INVALID, f"no prepared bootstrapping key for n={n}, k={k}, l={l}, log_beta={log_beta}")
        g = bsk if isinstance(bsk, torch.Tensor) else _to_dev(bsk)
        self.bsk = torch.empty(words, dtype=torch.int64, device="cuda")
        if log_beta is None:
            binding.tfhe_bsk_prepare_dev(n, k, l, n_lwe, g.data_ptr(), self.bsk.data_ptr())
        else:
            binding.tfhe_gadget_bsk_prepare_dev(n, k, log_beta, l, n_lwe, g.data_ptr(), self.bsk.data_ptr())
        self.ksk = ksk if isinstance(ksk, torch.Tensor) else _to_dev(ksk)
        torch.cuda.synchronize()


def blind_rotation(c, btk, table):
    """tlwe.rs:121-148 as DESIGN.md §10 defines it: TGLWE that decrypts to X^-phi~ table"""
    torch = _torch()
    x = c.words.reshape(-1, btk.n_lwe + 1)
    out = torch.empty((x.shape[0], btk.k + 1, btk.n), dtype=torch.int64, device="cuda")
    dt, dx = _to_dev(table.packed()), _to_dev(x)
    if btk.log_beta is None:
        binding.tfhe_blind_rotation_dev(btk.n, btk.k, btk.l, btk.n_lwe, btk.bsk.data_ptr(), dt.data_ptr(), dx.data_ptr(), out.data_ptr(),
                                        x.shape[0])
    else:
        binding.tfhe_gadget_blind_rotation_dev(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), dt.data_ptr(),
                                               dx.data_ptr(), out.data_ptr(), x.shape[0])
    o = _from_dev(out)
    return TGLWE(o[:, : btk.k, :], o[:, btk.k, :])


def bootstrapping(btk, table, c):
    """tlwe.rs:150-161: blind rotation, sample extraction at 0, key switch back to dimension n_lwe"""
    torch = _torch()
    x = c.words.reshape(-1, btk.n_lwe + 1)
    out = torch.empty(x.shape, dtype=torch.int64, device="cuda")
    dt, dx = _to_dev(table.packed()), _to_dev(x)
    if btk.log_beta is None:
        binding.tfhe_bootstrap_dev(btk.n, btk.k, btk.l, btk.n_lwe, btk.bsk.data_ptr(), dt.data_ptr(), btk.ks_l, btk.ksk.data_ptr(),
                                   dx.data_ptr(), out.data_ptr(), x.shape[0])
    else:
        binding.tfhe_gadget_bootstrap_dev(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), dt.data_ptr(),
                                          btk.ks_log_beta, btk.ks_l, btk.ksk.data_ptr(), dx.data_ptr(), out.data_ptr(), x.shape[0])
    return TLWE(_from_dev(out).reshape(c.words.shape))


# ---- the signed base-2^b gadget -------------------------------------------------------------------
def gadget_decompose(words, log_beta, l):
    """words [..][n] u64 -> [..][l][n] int64: the signed digits of every word, level 0 the most significant"""
    torch = _torch()
    w = np.ascontiguousarray(words, dtype=np.uint64)
    n = w.shape[-1]
    rows = w.size // n
    dw = _to_dev(w.reshape(rows, n))
    out = torch.empty((rows, l, n), dtype=torch.int64, device="cuda")
    binding.tn_gadget_decompose_dev(n, log_beta, l, dw.data_ptr(), out.data_ptr(), rows)
    return out.cpu().numpy().reshape(w.shape[:-1] + (l, n))


def gadget_external_product(tggsw, tglwe, log_beta):
    """sum_i sum_d digit_d(tglwe_i) tggsw[i][d]: tggsw [(k+1)][l][(k+1)][n] with level d encrypting m 2^(64 - b(d+1))"""
    torch = _torch()
    rows = np.ascontiguousarray(tggsw.rows if isinstance(tggsw, TGGSW) else tggsw, dtype=np.uint64)
    k1, l, _, n = rows.shape
    words = binding.tggsw_gadget_prepared_words(n, k1 - 1, log_beta, l)
    if words == 0:
        raise binding.FheError(binding.FHE_E_INVALID, f"no gadget product for n={n}, k={k1 - 1}, log_beta={log_beta}, l={l}")
    x = tglwe.packed()
    batch = x.size // (k1 * n)
    dg, dx = _to_dev(rows), _to_dev(x.reshape(batch, k1, n))
    prep = torch.empty(words, dtype=torch.int64, device="cuda")
    out = torch.empty((batch, k1, n), dtype=torch.int64, device="cuda")
    binding.tggsw_gadget_prepare_dev(n, k1 - 1, log_beta, l, dg.data_ptr(), prep.data_ptr())
    binding.tggsw_gadget_external_product_dev(n, k1 - 1, log_beta, l, prep.data_ptr(), dx.data_ptr(), out.data_ptr(), batch)
    o = _from_dev(out).reshape(x.shape)
    return TGLWE(o[..., : k1 - 1, :], o[..., k1 - 1, :])
