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
    cmux (tggsw.rs:39-41, a key bit there)             circuit bootstrapping of DESIGN.md §12: private_key_switch,
                                                       CircuitBootstrappingKey, circuit_bootstrap, PreparedTGGSWs,
                                                       cmux (a selector per ciphertext), cmux_tree (vertical packing)
    (no counterpart)                                   boolean gates of DESIGN.md §13 (bits +-2^61): GATES, gate_bootstrap
                                                       (a mixed-op batch in one call), mux, gate_not, trivial_bit, and the
                                                       Circuit netlist (plan levels on the host, evaluate on the device)
    (no counterpart)                                   small integers of DESIGN.md §14 (x in [0, 2^t) is phase x 2^(63-t)):
                                                       encode_int, trivial_int, make_lut, lincomb, lut_bootstrap (a table
                                                       per row in one call), and the LutCircuit netlist
    (no counterpart)                                   several tables from one blind rotation:
                                                       lut_many_bootstrap, LutCircuit.plan / evaluate with share=nu_max
    (no counterpart)                                   two-digit tree lookups: PackingKeySwitchKey,
                                                       packing_key_switch (TLWEs -> one TGLWE), box_expand, bootstrap_rows
                                                       (a test vector per row), tree_lookup (table2d[x][y], t bits each)
    (no counterpart)                                   the client side: cdt_table, ClientKey (generate,
                                                       bootstrapping_key, circuit_bootstrapping_key, packing_key_switch_key,
                                                       encrypt_int / encrypt_bit, decrypt_int / decrypt_bit, phase) and the
                                                       message builders of the keys (bsk_messages, ksk_messages, ..)
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
from .device import from_dev as _from_dev, to_dev as _to_dev, torch as _torch  # noqa: E402  (shared with bfv.py)


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


# ---- circuit bootstrapping and the CMux with a selector per ciphertext -----------------------------------
def _dev_words(x):
    torch = _torch()
    return x if isinstance(x, torch.Tensor) else _to_dev(x)


def private_key_switch(c, pfksk, log_beta, l):
    """TLWE of dimension k n -> TGLWE per function r <= k: out_r = sum_{j <= kn} sum_d digit_d(c_j) pfksk[r][j][d].
    pfksk [(k+1)][k n + 1][l][(k+1)][n] (numpy or a device tensor).  The result's a is [.., (k+1)][k][n], b [.., (k+1)][n]."""
    torch = _torch()
    k1, n = pfksk.shape[0], pfksk.shape[-1]
    kn = c.dim
    size = pfksk.numel() if isinstance(pfksk, torch.Tensor) else np.asarray(pfksk).size
    if pfksk.shape[1] != kn + 1 or binding.tfhe_pfksk_words(n, k1 - 1, log_beta, l) != size:
        raise binding.FheError(binding.FHE_E_INVALID, f"pfksk of shape {tuple(pfksk.shape)} does not match dimension {kn}, log_beta={log_beta}, l={l}")
    x = c.words.reshape(-1, kn + 1)
    dk, dx = _dev_words(pfksk), _to_dev(x)
    out = torch.empty((x.shape[0], k1, k1, n), dtype=torch.int64, device="cuda")
    binding.tlwe_gadget_private_key_switch_dev(n, k1 - 1, log_beta, l, dk.data_ptr(), dx.data_ptr(), out.data_ptr(), x.shape[0])
    o = _from_dev(out).reshape(c.words.shape[:-1] + (k1, k1, n))
    return TGLWE(o[..., : k1 - 1, :], o[..., k1 - 1, :])


class CircuitBootstrappingKey:
    """a gadget BootstrappingKey, and the private functional key switching key [(k+1)][k n + 1][pf_l][(k+1)][n] (function
    r < k: x -> -s_r x, function k: x -> x) kept on the device.  The circuit bootstrap yields gadget TGGSWs with
    (cb_log_beta, cb_l)."""

    def __init__(self, btk, pfksk, cb_log_beta, cb_l, pf_log_beta, pf_l):
        torch = _torch()
        if btk.log_beta is None:
            raise ValueError("circuit bootstrapping needs a gadget BootstrappingKey (log_beta=...)")
        if binding.tggsw_gadget_prepared_words(btk.n, btk.k, cb_log_beta, cb_l) == 0 or cb_log_beta * cb_l > 63:
            raise binding.FheError(binding.FHE_E_INVALID, f"no circuit bootstrap to (cb_log_beta, cb_l) = ({cb_log_beta}, {cb_l})")
        words = binding.tfhe_pfksk_words(btk.n, btk.k, pf_log_beta, pf_l)
        self.pfksk = _dev_words(pfksk)
        if words == 0 or self.pfksk.numel() != words:
            raise binding.FheError(binding.FHE_E_INVALID, f"pfksk has {self.pfksk.numel()} words, (pf_log_beta, pf_l) = ({pf_log_beta}, {pf_l}) "
                                   f"needs {words}")
        self.btk, self.cb_log_beta, self.cb_l, self.pf_log_beta, self.pf_l = btk, cb_log_beta, cb_l, pf_log_beta, pf_l
        torch.cuda.synchronize()


def circuit_bootstrap(cbk, c, *, device=False):
    """TLWE c (dimension n_lwe) of a bit mu, phase mu 2^63 + e -> raw gadget TGGSWs of mu under the GLWE key:
    [.., (k+1)][cb_l][(k+1)][n] (numpy; device=True: the int64 device tensor [batch][..], for PreparedTGGSWs)"""
    torch = _torch()
    b = cbk.btk
    x = c.words.reshape(-1, b.n_lwe + 1)
    k1 = b.k + 1
    out = torch.empty((x.shape[0], k1, cbk.cb_l, k1, b.n), dtype=torch.int64, device="cuda")
    dx = _to_dev(x)
    binding.tfhe_circuit_bootstrap_dev(b.n, b.k, b.log_beta, b.l, b.n_lwe, b.bsk.data_ptr(), cbk.cb_log_beta, cbk.cb_l, cbk.pf_log_beta,
                                       cbk.pf_l, cbk.pfksk.data_ptr(), dx.data_ptr(), out.data_ptr(), x.shape[0])
    if device:
        torch.cuda.synchronize()
        return out
    return _from_dev(out).reshape(c.words.shape[:-1] + (k1, cbk.cb_l, k1, b.n))


class PreparedTGGSWs:
    """`count` gadget TGGSWs rows [count][(k+1)][l][(k+1)][n] (numpy or a device tensor) prepared side by side on the
    device (fhe_tggsw_gadget_prepare_many_dev): the selectors of cmux and cmux_tree"""

    def __init__(self, rows, log_beta):
        torch = _torch()
        shape = tuple(rows.shape)
        if len(shape) != 5 or shape[1] != shape[3]:
            raise ValueError("rows must be [count][(k+1)][l][(k+1)][n]")
        self.count, k1, self.l, _, self.n = shape
        self.k, self.log_beta = k1 - 1, log_beta
        self.words = binding.tggsw_gadget_prepared_words(self.n, self.k, log_beta, self.l)
        if self.words == 0:
            raise binding.FheError(binding.FHE_E_INVALID, f"no gadget product for n={self.n}, k={self.k}, log_beta={log_beta}, l={self.l}")
        g = _dev_words(rows)
        self.prepared = torch.empty(self.count * self.words, dtype=torch.int64, device="cuda")
        binding.tggsw_gadget_prepare_many_dev(self.n, self.k, log_beta, self.l, self.count, g.data_ptr(), self.prepared.data_ptr())
        torch.cuda.synchronize()


def _cmux_dev(sel, d_idx, d_c0, d_c1, batch):
    torch = _torch()
    out = torch.empty((batch, sel.k + 1, sel.n), dtype=torch.int64, device="cuda")
    binding.tggsw_gadget_cmux_dev(sel.n, sel.k, sel.log_beta, sel.l, sel.count, sel.prepared.data_ptr(), d_idx.data_ptr(), d_c0.data_ptr(),
                                  d_c1.data_ptr(), out.data_ptr(), batch)
    return out


def cmux(sel, idx, c0, c1):
    """out_j = c0_j + C[idx_j] [x] (c1_j - c0_j), C = the TGGSWs of `sel` (PreparedTGGSWs), idx [batch] (an idx_j >= count
    gives c0_j); c0, c1 TGLWE batches"""
    torch = _torch()
    x0, x1 = c0.packed(), c1.packed()
    k1, n = sel.k + 1, sel.n
    batch = x0.size // (k1 * n)
    if x1.shape != x0.shape or len(idx) != batch:
        raise ValueError("cmux: c0, c1 and idx must have one entry per ciphertext")
    di = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.uint32).view(np.int32)).cuda()
    d0, d1 = _to_dev(x0.reshape(batch, k1, n)), _to_dev(x1.reshape(batch, k1, n))
    o = _from_dev(_cmux_dev(sel, di, d0, d1, batch)).reshape(x0.shape)
    return TGLWE(o[..., : k1 - 1, :], o[..., k1 - 1, :])


def cmux_tree(sel, bits_idx, table):
    """vertical packing: table [2^m][(k+1)][n] (TGLWEs, shared by the batch), bits_idx [batch][m] indices into `sel` of the
    TGGSWs of bit i of each input x (i = 0 the least significant) -> TGLWE [batch] of table[x].  One CMux launch per
    level: level i halves the candidates with bit i, c0 = entry 2j, c1 = entry 2j + 1."""
    torch = _torch()
    tab = table.packed() if isinstance(table, TGLWE) else np.asarray(table, dtype=np.uint64)
    bits = np.atleast_2d(np.asarray(bits_idx, dtype=np.uint32))
    batch, m = bits.shape
    k1, n = sel.k + 1, sel.n
    if tab.shape != (1 << m, k1, n):
        raise ValueError(f"cmux_tree: table must be [2^{m}][{k1}][{n}]")
    cur = _to_dev(tab).unsqueeze(0).expand(batch, -1, -1, -1)           # [batch][2^m][(k+1)][n]
    db = torch.from_numpy(bits.view(np.int32)).cuda()
    for i in range(m):
        half = cur.shape[1] // 2
        pairs = cur.reshape(batch, half, 2, k1, n)
        c0, c1 = pairs[:, :, 0].contiguous(), pairs[:, :, 1].contiguous()
        di = db[:, i].unsqueeze(1).expand(batch, half).contiguous()
        cur = _cmux_dev(sel, di, c0, c1, batch * half).reshape(batch, half, k1, n)
    o = _from_dev(cur.reshape(batch, k1, n))
    return TGLWE(o[:, : k1 - 1, :], o[:, k1 - 1, :])


# ---- boolean gates with gate bootstrapping -----------------------------------------------------------------
GATES = binding.GATES
MU = 1 << 61                                     # bit 1 is phase +MU, bit 0 is -MU


def _gate_code(op):
    if isinstance(op, str):
        if op.upper() not in GATES:
            raise ValueError(f"unknown gate {op!r}: one of {sorted(GATES)}")
        return GATES[op.upper()]
    return int(op)


def _gate_key(btk):
    if btk.log_beta is None:
        raise ValueError("boolean gates need a gadget BootstrappingKey (log_beta=...)")


def trivial_bit(bit, n_lwe):
    """the noiseless TLWE (0 .. 0, +-MU) of a bit, or of each bit of an array"""
    bits = np.asarray(bit)
    words = np.zeros(bits.shape + (n_lwe + 1,), dtype=np.uint64)
    words[..., n_lwe] = np.where(bits.astype(bool), np.uint64(MU), np.uint64((1 << 64) - MU))
    return TLWE(words)


def gate_not(c):
    """NOT without a bootstrap: every word negated"""
    return TLWE((np.uint64(0) - c.words).astype(np.uint64))


def _gate_call(btk, mux, pool, desc, batch):
    """one fhe_tfhe_gate_bootstrap_dev / fhe_tfhe_gate_mux_dev over the host pool [wires][n_lwe + 1] and descriptors [batch][3]"""
    torch = _torch()
    _gate_key(btk)
    dp = _to_dev(pool)
    dd = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.uint32).view(np.int32)).cuda()
    out = torch.empty((batch, btk.n_lwe + 1), dtype=torch.int64, device="cuda")
    f = binding.tfhe_gate_mux_dev if mux else binding.tfhe_gate_bootstrap_dev
    f(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), btk.ks_log_beta, btk.ks_l, btk.ksk.data_ptr(), dp.data_ptr(), pool.shape[0],
      dd.data_ptr(), out.data_ptr(), batch)
    return _from_dev(out)


def gate_bootstrap(btk, ops, a, b):
    """op(a, b) row by row: `ops` a gate name or code (GATES), or one per row (a mixed batch runs as one call); a, b TLWE
    batches of the same shape under the LWE key of btk (a gadget BootstrappingKey)"""
    x, y = a.words.reshape(-1, btk.n_lwe + 1), b.words.reshape(-1, btk.n_lwe + 1)
    batch = x.shape[0]
    if y.shape != x.shape:
        raise ValueError("gate_bootstrap: a and b must have the same shape")
    if isinstance(ops, str) or np.ndim(ops) == 0:
        codes = np.full(batch, _gate_code(ops), dtype=np.uint32)
    else:
        codes = np.array([_gate_code(o) for o in np.asarray(ops).reshape(-1)], dtype=np.uint32)
        if len(codes) != batch:
            raise ValueError("gate_bootstrap: one op per row")
    i = np.arange(batch, dtype=np.uint32)
    out = _gate_call(btk, False, np.concatenate([x, y]), np.stack([codes, i, i + batch], axis=1), batch)
    return TLWE(out.reshape(a.words.shape))


def mux(btk, s, a, b):
    """s ? a : b row by row (two blind rotations, one key switch); s, a, b TLWE batches of the same shape"""
    rows = [t.words.reshape(-1, btk.n_lwe + 1) for t in (s, a, b)]
    batch = rows[0].shape[0]
    if any(r.shape != rows[0].shape for r in rows):
        raise ValueError("mux: s, a and b must have the same shape")
    i = np.arange(batch, dtype=np.uint32)
    out = _gate_call(btk, True, np.concatenate(rows), np.stack([i, i + batch, i + 2 * batch], axis=1), batch)
    return TLWE(out.reshape(s.words.shape))


class CircuitPlan:
    """Circuit.plan(): pool slots and levels.  Slots: the inputs, the constants and the NOTs of level 0, then per level
    L >= 1 its gates, its MUXes and its NOTs.  levels[L - 1] = {"level", "gates": (first slot, count), "gate_desc" [count][3]
    (op, slot x, slot y), "muxes": (first slot, count), "mux_desc" [count][3] (slot s, slot a, slot b)}; nots[L] = list of
    (slot, root slot, negate): a NOT chain resolved to the bootstrapped (or input, or constant) wire it ends at."""

    def __init__(self, slot, level, n_slots, inputs, consts, levels, nots, outputs):
        self.slot, self.level, self.n_slots = slot, level, n_slots
        self.inputs, self.consts, self.levels, self.nots, self.outputs = inputs, consts, levels, nots, outputs

    @property
    def depth(self):
        return len(self.levels)


class Circuit:
    """A netlist of boolean gates on encrypted bits.  Every builder returns a wire (an int) and takes only wires defined
    before it.  Gates and MUXes are bootstrapped (one level each above their highest input); NOT and constants are not.
    evaluate() runs `batch` independent copies of the circuit with one gate call and at most one MUX call per level."""

    def __init__(self):
        self._nodes = []            # (kind, args): "input" (), "const" (bit,), "gate" (op, x, y), "not" (x,), "mux" (s, x, y)
        self._outputs = []

    def _wires(self, *ws):
        for w in ws:
            if not isinstance(w, (int, np.integer)) or not 0 <= int(w) < len(self._nodes):
                raise ValueError(f"wire {w!r} is used before it is defined ({len(self._nodes)} wires so far)")
        return tuple(int(w) for w in ws)

    def _add(self, kind, *args):
        self._nodes.append((kind, args))
        return len(self._nodes) - 1

    def input(self):
        return self._add("input")

    def const(self, bit):
        return self._add("const", int(bool(bit)))

    def gate(self, op, x, y):
        code = _gate_code(op)
        if not 0 <= code < binding.FHE_GATE_COUNT:
            raise ValueError(f"gate code {code} out of range")
        return self._add("gate", code, *self._wires(x, y))

    def not_(self, x):
        return self._add("not", *self._wires(x))

    def mux(self, s, x, y):
        return self._add("mux", *self._wires(s, x, y))

    def output(self, x):
        self._outputs.append(self._wires(x)[0])
        return x

    @property
    def n_inputs(self):
        return sum(k == "input" for k, _ in self._nodes)

    def plan(self):
        """levels and pool slots (host only)"""
        level = []
        for w, (kind, args) in enumerate(self._nodes):
            ins = args[1:] if kind == "gate" else args if kind in ("not", "mux") else ()
            if any(not 0 <= x < w for x in ins):
                raise ValueError(f"wire {w} reads a wire that is not defined before it")
            if kind in ("input", "const"):
                level.append(0)
            elif kind == "not":
                level.append(level[args[0]])
            else:
                level.append(1 + max(level[x] for x in ins))
        depth = max(level, default=0)
        root = []                                       # (root wire, negate) of every wire
        for w, (kind, args) in enumerate(self._nodes):
            root.append((root[args[0]][0], not root[args[0]][1]) if kind == "not" else (w, False))
        slot = [None] * len(self._nodes)
        nxt = 0

        def place(kinds, lev):
            nonlocal nxt
            first = nxt
            for w, (kind, _) in enumerate(self._nodes):
                if kind in kinds and level[w] == lev:
                    slot[w] = nxt
                    nxt += 1
            return first, nxt - first

        place(("input",), 0)
        place(("const",), 0)
        nots = {}
        place(("not",), 0)
        levels = []
        for lev in range(1, depth + 1):
            g, m = place(("gate",), lev), place(("mux",), lev)
            place(("not",), lev)
            levels.append({"level": lev, "gates": g, "muxes": m,
                           "gate_desc": np.array([(a[0], slot[a[1]], slot[a[2]]) for w, (k, a) in enumerate(self._nodes)
                                                  if k == "gate" and level[w] == lev], dtype=np.uint32).reshape(-1, 3),
                           "mux_desc": np.array([tuple(slot[x] for x in a) for w, (k, a) in enumerate(self._nodes)
                                                 if k == "mux" and level[w] == lev], dtype=np.uint32).reshape(-1, 3)})
        for lev in range(depth + 1):
            nots[lev] = [(slot[w], slot[root[w][0]], root[w][1]) for w, (k, _) in enumerate(self._nodes) if k == "not" and level[w] == lev]
        inputs = [slot[w] for w, (k, _) in enumerate(self._nodes) if k == "input"]
        consts = [(slot[w], a[0]) for w, (k, a) in enumerate(self._nodes) if k == "const"]
        return CircuitPlan(slot, level, nxt, inputs, consts, levels, nots, [slot[w] for w in self._outputs])

    def evaluate(self, btk, inputs):
        """inputs: one TLWE batch [batch][n_lwe + 1] per input wire, in definition order -> one TLWE batch per output.
        The pool is wire-major: slot w holds rows [w S, w S + batch), S = batch rounded up to even so that every slice
        starts 16-byte aligned; each level's gate outputs, then its MUX outputs, are one slice of the pool."""
        torch = _torch()
        _gate_key(btk)
        p = self.plan()
        row = btk.n_lwe + 1
        xs = [np.asarray(t.words if isinstance(t, TLWE) else t, dtype=np.uint64).reshape(-1, row) for t in inputs]
        if len(xs) != len(p.inputs):
            raise ValueError(f"evaluate: {len(p.inputs)} inputs expected, {len(xs)} given")
        batch = xs[0].shape[0] if xs else 1
        if any(x.shape[0] != batch for x in xs):
            raise ValueError("evaluate: every input needs the same batch")
        S = batch + (batch & 1)
        if p.n_slots * S >= 1 << 32:
            raise ValueError("evaluate: the pool needs more than 2^32 rows")
        fixed = len(p.inputs) + len(p.consts)           # the inputs and constants fill slots [0, fixed)
        host = np.zeros((fixed, S, row), dtype=np.uint64)
        for s, x in zip(p.inputs, xs):
            host[s, :batch] = x
        for s, bit in p.consts:
            host[s, :batch] = trivial_bit(np.full(batch, bit), btk.n_lwe).words
        inst, pad = np.arange(S, dtype=np.uint64), np.arange(S) >= batch

        def expand(desc, mux_):
            """[count][3] slot descriptors -> [count S][3] row descriptors (padding rows read nothing), in blocks of 4 rows
            so that every block starts 16-byte aligned"""
            out = np.empty((len(desc), S, 3), dtype=np.uint64)
            for c in range(3):
                v = desc[:, c:c + 1].astype(np.uint64)
                out[:, :, c] = v * np.uint64(S) + inst[None, :] if mux_ or c else v
            out[:, pad, :] = 0xFFFFFFFF
            out = out.reshape(-1, 3)
            return np.concatenate([out, np.zeros((-len(out) % 4, 3), dtype=np.uint64)])

        descs, offs = [], []                            # every level's descriptors, uploaded once
        for lv in p.levels:
            g, m = expand(lv["gate_desc"], False), expand(lv["mux_desc"], True)
            offs.append((sum(len(d) for d in descs), sum(len(d) for d in descs) + len(g)))
            descs += [g, m]
        pool = torch.empty((p.n_slots * S, row), dtype=torch.int64, device="cuda")
        pool[: fixed * S] = _to_dev(host.reshape(-1, row))
        dd = torch.from_numpy(np.concatenate(descs or [np.zeros((0, 3))]).astype(np.uint32).view(np.int32)).cuda()
        nots = []                                       # per level: destination rows, source rows, negate, uploaded once
        for lev in range(p.depth + 1):
            n = np.array(p.nots[lev], dtype=np.int64).reshape(-1, 3)
            rows_of = lambda col: torch.from_numpy((n[:, col:col + 1] * S + np.arange(batch)[None, :]).reshape(-1)).cuda()
            nots.append((rows_of(0), rows_of(1), torch.from_numpy(np.repeat(n[:, 2] != 0, batch)[:, None]).cuda()) if len(n) else None)
        st = torch.cuda.current_stream().cuda_stream

        def run_nots(lev):
            if nots[lev] is not None:
                dst, src, neg = nots[lev]
                v = pool[src]
                pool[dst] = torch.where(neg, -v, v)     # int64 negation wraps: -c mod 2^64

        run_nots(0)
        for lv, off in zip(p.levels, offs):
            for (first, count), mux_, o in ((lv["gates"], False, off[0]), (lv["muxes"], True, off[1])):
                if count:
                    f = binding.tfhe_gate_mux_dev if mux_ else binding.tfhe_gate_bootstrap_dev
                    f(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), btk.ks_log_beta, btk.ks_l, btk.ksk.data_ptr(),
                      pool.data_ptr(), p.n_slots * S, dd.data_ptr() + o * 12, pool.data_ptr() + first * S * row * 8, count * S, st)
            run_nots(lv["level"])
        if not p.outputs:
            return []
        outs = _from_dev(torch.stack([pool[s * S:s * S + batch] for s in p.outputs]))
        return [TLWE(o) for o in outs]


# ---- small integers: a lookup table per row in one bootstrap ---------------------------------------------------
LUT_NONE = binding.FHE_LUT_NONE                  # the index of an operand whose scale is 0, by convention


def _lut_key(btk):
    if btk.log_beta is None:
        raise ValueError("lookup-table bootstraps need a gadget BootstrappingKey (log_beta=...)")


def encode_int(x, t_bits):
    """the torus word x Delta mod 2^64, Delta = 2^(63 - t_bits), of a value or of each value of an array (Python integers,
    so a negative value wraps)"""
    if np.ndim(x) == 0:
        return np.uint64((int(x) << (63 - t_bits)) % (1 << 64))
    return np.array([(int(v) << (63 - t_bits)) % (1 << 64) for v in np.asarray(x).reshape(-1)], dtype=np.uint64).reshape(np.shape(x))


def trivial_int(x, t_bits, n_lwe):
    """the noiseless TLWE (0 .. 0, x Delta) of a value, or of each value of an array"""
    words = np.zeros(np.shape(x) + (n_lwe + 1,), dtype=np.uint64)
    words[..., n_lwe] = encode_int(x, t_bits)
    return TLWE(words)


def make_lut(f, t_bits, out=None):
    """[2^t_bits] torus words: entry x is out(f(x)); `out` maps a value to its torus word (default: value Delta mod 2^64)"""
    enc = (lambda v: encode_int(v, t_bits)) if out is None else out
    return np.array([int(enc(f(x))) % (1 << 64) for x in range(1 << t_bits)], dtype=np.uint64)


def _lut_desc(desc_rows):
    """[rows][6] (lut, x, y, sx, sy, o_hi), scales signed -> u32 words"""
    d = np.asarray(desc_rows, dtype=np.int64).reshape(-1, 6)
    return np.ascontiguousarray((d & 0xFFFFFFFF).astype(np.uint32))


def _desc_dev(desc):
    return _torch().from_numpy(desc.view(np.int32)).cuda()


def _pool_rows(pool):
    w = np.asarray(pool.words if isinstance(pool, TLWE) else pool, dtype=np.uint64)
    return w.reshape(-1, w.shape[-1])


def lincomb(desc_rows, pool):
    """fhe_tlwe_lincomb_dev: row m = sx pool[x] + sy pool[y] + (0 .. 0, o_hi 2^32) of descriptor row m = (lut, x, y, sx, sy,
    o_hi) (the lut word is ignored); pool [wires][n_lwe + 1].  No bootstrap."""
    torch = _torch()
    p, desc = _pool_rows(pool), _lut_desc(desc_rows)
    dp, dd = _to_dev(p), _desc_dev(desc)
    out = torch.empty((len(desc), p.shape[1]), dtype=torch.int64, device="cuda")
    binding.tlwe_lincomb_dev(p.shape[1] - 1, dp.data_ptr(), p.shape[0], dd.data_ptr(), out.data_ptr(), len(desc))
    return TLWE(_from_dev(out))


def lut_bootstrap(btk, t_bits, luts, desc, pool):
    """fhe_tfhe_lut_bootstrap_dev: row m bootstraps its combined input (as lincomb) through table luts[lut] ([lut_count][2^t_bits]
    torus words, see make_lut) -> TLWE [rows][n_lwe + 1] under the LWE key of btk (a gadget BootstrappingKey)"""
    torch = _torch()
    _lut_key(btk)
    p, d = _pool_rows(pool), _lut_desc(desc)
    tabs = np.ascontiguousarray(np.asarray(luts, dtype=np.uint64).reshape(-1, 1 << t_bits))
    dp, dd, dl = _to_dev(p), _desc_dev(d), _to_dev(tabs)
    out = torch.empty((len(d), btk.n_lwe + 1), dtype=torch.int64, device="cuda")
    binding.tfhe_lut_bootstrap_dev(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), btk.ks_log_beta, btk.ks_l, btk.ksk.data_ptr(),
                                   t_bits, dl.data_ptr(), tabs.shape[0], dp.data_ptr(), p.shape[0], dd.data_ptr(), out.data_ptr(), len(d))
    return TLWE(_from_dev(out))


def lut_many_bootstrap(btk, t_bits, nu, luts, desc, pool):
    """fhe_tfhe_lut_many_bootstrap_dev: row m bootstraps its combined input (as lincomb) once and looks it up in the 2^nu
    consecutive tables luts[lut], .., luts[lut + 2^nu - 1] -> TLWE [2^nu][rows][n_lwe + 1], function-major.  Each unit of nu
    costs one bit of mod-switch precision."""
    torch = _torch()
    _lut_key(btk)
    p, d = _pool_rows(pool), _lut_desc(desc)
    tabs = np.ascontiguousarray(np.asarray(luts, dtype=np.uint64).reshape(-1, 1 << t_bits))
    dp, dd, dl = _to_dev(p), _desc_dev(d), _to_dev(tabs)
    out = torch.empty((1 << nu, len(d), btk.n_lwe + 1), dtype=torch.int64, device="cuda")
    binding.tfhe_lut_many_bootstrap_dev(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), btk.ks_log_beta, btk.ks_l,
                                        btk.ksk.data_ptr(), t_bits, nu, dl.data_ptr(), tabs.shape[0], dp.data_ptr(), p.shape[0], dd.data_ptr(),
                                        out.data_ptr(), len(d))
    return TLWE(_from_dev(out))


class LutCircuitPlan:
    """LutCircuit.plan(): pool slots, levels and sub-levels.  Slots: the inputs, the constants and the `lin` wires of level 0
    (sub-level by sub-level), then per level L >= 1 its `lut` wires and its `lin` wires (sub-level by sub-level).
    levels[L - 1] = {"level", "luts": (first slot, count), "lut_desc" [count][6]}; lins[L] = one {"slots": (first slot, count),
    "desc" [count][6]} per sub-level, in order.  A descriptor is (table, slot x, slot y, sx, sy, const): an operand whose scale
    is 0 has slot LUT_NONE, and const is still a value (evaluate turns it into o_hi for its t_bits).
    plan(share >= 1) only: `luts` holds the level's nu = 0 wires, and levels[L - 1]["many"] lists, for each nu that occurs,
    {"nu", "block": first slot, "chunks": G, "desc" [G][6]}: 2^nu G slots after the nu = 0 wires, function h of chunk g at
    block + h G + g (a function a chunk does not fill is scratch: no wire has that slot); a descriptor's table word indexes
    many_tables[nu], the list of [2^t] tables in which every chunk's 2^nu tables are consecutive."""

    def __init__(self, slot, level, sub, n_slots, inputs, consts, levels, lins, outputs, tables, many_tables=None):
        self.slot, self.level, self.sub, self.n_slots = slot, level, sub, n_slots
        self.inputs, self.consts, self.levels, self.lins, self.outputs, self.tables = inputs, consts, levels, lins, outputs, tables
        self.many_tables = many_tables or {}

    @property
    def depth(self):
        return len(self.levels)


class LutCircuit:
    """A netlist of table lookups and linear nodes on encrypted small integers (values in [0, 2^t), see encode_int).  Every
    builder returns a wire (an int) and takes only wires defined before it.  `lut` wires are bootstrapped (one level above
    their highest operand); `lin` wires, inputs and constants are not.  evaluate() runs `batch` independent copies with one
    fhe_tfhe_lut_bootstrap_dev per level and one fhe_tlwe_lincomb_dev per sub-level of `lin` wires."""

    def __init__(self):
        self._nodes = []            # (kind, args): "input" (), "const" (value,), "lin" (x, sx, y, sy, const), "lut" (table, x, sx, y, sy, const)
        self._outputs = []
        self._tables, self._table_index = [], {}

    def _add(self, kind, *args):
        self._nodes.append((kind, args))
        return len(self._nodes) - 1

    def _operands(self, x, sx, y, sy, const):
        """-> (x, sx, y, sy, const) with a zero-scale operand's wire None"""
        sx, sy = int(sx), (0 if y is None else int(sy))
        for s in (sx, sy):
            if not -(1 << 31) <= s < 1 << 31:
                raise ValueError(f"scale {s} does not fit an int32")
        ws = []
        for w, s in ((x, sx), (y, sy)):
            if s == 0:
                ws.append(None)
                continue
            if not isinstance(w, (int, np.integer)) or not 0 <= int(w) < len(self._nodes):
                raise ValueError(f"wire {w!r} is used before it is defined ({len(self._nodes)} wires so far)")
            ws.append(int(w))
        return ws[0], sx, ws[1], sy, int(const)

    def input(self):
        return self._add("input")

    def const(self, value):
        return self._add("const", int(value))

    def lin(self, x, sx=1, y=None, sy=0, const=0):
        """sx x + sy y + const, no bootstrap (the noise of the operands adds up with their scales)"""
        return self._add("lin", *self._operands(x, sx, y, sy, const))

    def lut(self, table, x, sx=1, y=None, sy=0, const=0):
        """table[sx x + sy y + const], bootstrapped; table: [2^t] torus words (make_lut).  Identical tables are stored once."""
        ops = self._operands(x, sx, y, sy, const)
        tab = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1)
        key = tab.tobytes()
        if key not in self._table_index:
            self._table_index[key] = len(self._tables)
            self._tables.append(tab)
        return self._add("lut", self._table_index[key], *ops)

    def output(self, w):
        if not isinstance(w, (int, np.integer)) or not 0 <= int(w) < len(self._nodes):
            raise ValueError(f"wire {w!r} is used before it is defined ({len(self._nodes)} wires so far)")
        self._outputs.append(int(w))
        return w

    @property
    def n_inputs(self):
        return sum(k == "input" for k, _ in self._nodes)

    @property
    def tables(self):
        return list(self._tables)

    def _share_chunks(self, ws, share):
        """the `lut` wires ws of one level -> (the nu = 0 wires, {nu: chunks}): wires with identical operands (x, sx, y, sy,
        const) form a class, in definition order; a class is cut into chunks of at most 2^share wires; a chunk of c > 1
        wires has nu = ceil(log2 c), a chunk of one wire is a nu = 0 wire"""
        classes = {}
        for w in ws:
            classes.setdefault(self._nodes[w][1][1:], []).append(w)
        singles, chunks = [], {}
        for members in classes.values():
            for i in range(0, len(members), 1 << share):
                ch = members[i:i + (1 << share)]
                if len(ch) == 1:
                    singles.append(ch[0])
                else:
                    chunks.setdefault((len(ch) - 1).bit_length(), []).append(ch)
        return sorted(singles), chunks

    def plan(self, share=0):
        """levels, sub-levels and pool slots (host only).  share = nu_max >= 1 lets `lut` wires of one level with identical
        operands share a blind rotation, up to 2^nu_max of them (LutCircuitPlan); share = 0 is the plan of
        one bootstrap per `lut` wire."""
        if not 0 <= int(share) <= 4:
            raise ValueError(f"plan: share must be in 0 .. 4 (share={share})")
        level, sub = [], []
        for w, (kind, args) in enumerate(self._nodes):
            a = args[1:] if kind == "lut" else args
            ins = [v for v in (a[0], a[2]) if v is not None] if kind in ("lin", "lut") else []
            if any(not 0 <= v < w for v in ins):
                raise ValueError(f"wire {w} reads a wire that is not defined before it")
            top = max((level[v] for v in ins), default=0)
            if kind == "lut":
                level.append(1 + top)
                sub.append(-1)
            elif kind == "lin":
                level.append(top)
                sub.append(1 + max((sub[v] for v in ins if level[v] == top and self._nodes[v][0] == "lin"), default=-1))
            else:
                level.append(0)
                sub.append(-1)
        depth = max(level, default=0)
        slot = [None] * len(self._nodes)
        nxt = 0

        def place(kind, lev, sb=-1):
            nonlocal nxt
            first, ws = nxt, []
            for w, (k, _) in enumerate(self._nodes):
                if k == kind and level[w] == lev and sub[w] == sb:
                    slot[w] = nxt
                    nxt += 1
                    ws.append(w)
            return (first, nxt - first), ws

        def descs(ws, tabs=None):
            rows = []
            for i, w in enumerate(ws):
                kind, args = self._nodes[w]
                t, (x, sx, y, sy, c) = (args[0], args[1:]) if kind == "lut" else (LUT_NONE, args)
                rows.append((t if tabs is None else tabs[i], LUT_NONE if x is None else slot[x], LUT_NONE if y is None else slot[y], sx, sy, c))
            return np.array(rows, dtype=np.int64).reshape(-1, 6)

        many_tables, many_index = {}, {}

        def place_shared(lev):
            """the `lut` wires of a level under share >= 1: the nu = 0 wires, then one block of 2^nu G slots per nu"""
            nonlocal nxt
            singles, chunks = self._share_chunks([w for w, (k, _) in enumerate(self._nodes) if k == "lut" and level[w] == lev], share)
            first = nxt
            for w in singles:
                slot[w] = nxt
                nxt += 1
            many = []
            for nu in sorted(chunks):
                G, F, firsts = len(chunks[nu]), 1 << nu, []
                for g, ch in enumerate(chunks[nu]):
                    for h, w in enumerate(ch):
                        slot[w] = nxt + h * G + g
                    ids = [self._nodes[w][1][0] for w in ch]
                    ids = tuple(ids + [ids[0]] * (F - len(ids)))            # a function the chunk does not fill repeats its first table
                    if (nu, ids) not in many_index:
                        tabs = many_tables.setdefault(nu, [])
                        many_index[nu, ids] = len(tabs)
                        tabs.extend(self._tables[i] for i in ids)
                    firsts.append(many_index[nu, ids])
                many.append({"nu": nu, "block": nxt, "chunks": G, "desc": descs([ch[0] for ch in chunks[nu]], firsts)})
                nxt += F * G
            return {"level": lev, "luts": (first, len(singles)), "lut_desc": descs(singles), "many": many}

        place("input", 0)
        place("const", 0)
        levels, lins = [], {}
        for lev in range(depth + 1):
            if lev and share:
                levels.append(place_shared(lev))
            elif lev:
                span, ws = place("lut", lev)
                levels.append({"level": lev, "luts": span, "lut_desc": descs(ws)})
            lins[lev] = []
            for sb in range(1 + max((sub[w] for w in range(len(slot)) if level[w] == lev), default=-1)):
                span, ws = place("lin", lev, sb)
                lins[lev].append({"slots": span, "desc": descs(ws)})
        inputs = [slot[w] for w, (k, _) in enumerate(self._nodes) if k == "input"]
        consts = [(slot[w], a[0]) for w, (k, a) in enumerate(self._nodes) if k == "const"]
        return LutCircuitPlan(slot, level, sub, nxt, inputs, consts, levels, lins, [slot[w] for w in self._outputs], self.tables, many_tables)

    def evaluate(self, btk, inputs, t_bits, share=0):
        """inputs: one TLWE batch [batch][n_lwe + 1] per input wire, in definition order -> one TLWE batch per output.
        The pool is wire-major as Circuit.evaluate's: slot w holds rows [w S, w S + batch), S = batch rounded up to even so
        that every slice (and every block of descriptors, 24 bytes a row) starts 16-byte aligned; the padding copy of a wire
        is an invalid row.  Tables, constants and descriptors are uploaded once; the host waits only for the outputs.
        share = nu_max >= 1 (plan(share)): per level, `lut` wires with identical operands share one blind rotation, up to
        2^nu_max of them, through one fhe_tfhe_lut_many_bootstrap_dev per nu that occurs.  Each unit of nu costs one bit of
        message space at equal failure rate: the mod switch rounds to multiples of 2^nu, so its error doubles with every
        unit, and t_bits has to shrink by as much to keep the margin.  share <= log2 n - t_bits."""
        torch = _torch()
        _lut_key(btk)
        if share > int(btk.n).bit_length() - 1 - t_bits:
            raise ValueError(f"evaluate: share={share} needs share <= log2 n - t_bits = {int(btk.n).bit_length() - 1 - t_bits}")
        p = self.plan(share)
        row = btk.n_lwe + 1
        xs = [np.asarray(t.words if isinstance(t, TLWE) else t, dtype=np.uint64).reshape(-1, row) for t in inputs]
        if len(xs) != len(p.inputs):
            raise ValueError(f"evaluate: {len(p.inputs)} inputs expected, {len(xs)} given")
        batch = xs[0].shape[0] if xs else 1
        if any(x.shape[0] != batch for x in xs):
            raise ValueError("evaluate: every input needs the same batch")
        if any(len(t) != 1 << t_bits for t in p.tables):
            raise ValueError(f"evaluate: every table needs 2^{t_bits} words")
        S = batch + (batch & 1)
        if p.n_slots * S >= 1 << 32:
            raise ValueError("evaluate: the pool needs more than 2^32 rows")
        fixed = len(p.inputs) + len(p.consts)           # the inputs and constants fill slots [0, fixed)
        host = np.zeros((fixed, S, row), dtype=np.uint64)
        for s, x in zip(p.inputs, xs):
            host[s, :batch] = x
        for s, v in p.consts:
            host[s, :batch] = trivial_int(np.full(batch, v), t_bits, btk.n_lwe).words
        inst, pad = np.arange(S, dtype=np.int64), np.arange(S) >= batch

        def expand(desc):
            """[count][6] slot descriptors -> [count S][6] row descriptors; a padding row names wire LUT_NONE with scale 1"""
            out = np.repeat(desc[:, None, :], S, axis=1)
            for c in (1, 2):
                out[:, :, c] = np.where(out[:, :, c] == LUT_NONE, LUT_NONE, out[:, :, c] * S + inst[None, :])
            out[:, :, 5] = [[int(encode_int(v, t_bits)) >> 32] * S for v in desc[:, 5]]
            out[:, pad, :] = (LUT_NONE, LUT_NONE, LUT_NONE, 1, 0, 0)
            return out.reshape(-1, 6)

        calls, descs, off = [], [], 0                   # (nu, or None: lincomb; first slot; rows / S; descriptor row offset), in issue order
        for lev in range(p.depth + 1):
            lv = p.levels[lev - 1] if lev else {}
            groups = ([(0, lv["luts"], lv["lut_desc"])] if lev else []) + \
                     [(m["nu"], (m["block"], m["chunks"]), m["desc"]) for m in lv.get("many", [])] + \
                     [(None, g["slots"], g["desc"]) for g in p.lins[lev]]
            for nu, (first, count), d in groups:
                if count:
                    calls.append((nu, first, count, off))
                    descs.append(expand(d))
                    off += count * S
        pool = torch.empty((p.n_slots * S, row), dtype=torch.int64, device="cuda")
        pool[: fixed * S] = _to_dev(host.reshape(-1, row))
        dd = _desc_dev(_lut_desc(np.concatenate(descs))) if descs else None
        dl = _to_dev(np.stack(p.tables)) if p.tables else None
        dm = {nu: _to_dev(np.stack(tabs)) for nu, tabs in p.many_tables.items()}
        st = torch.cuda.current_stream().cuda_stream
        for nu, first, count, o in calls:
            d_desc, d_out = dd.data_ptr() + o * 24, pool.data_ptr() + first * S * row * 8
            if nu:                                      # [2^nu][count S] rows: function h of chunk g fills slot first + h count + g
                binding.tfhe_lut_many_bootstrap_dev(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), btk.ks_log_beta, btk.ks_l,
                                                    btk.ksk.data_ptr(), t_bits, nu, dm[nu].data_ptr(), len(p.many_tables[nu]), pool.data_ptr(),
                                                    p.n_slots * S, d_desc, d_out, count * S, st)
            elif nu == 0:
                binding.tfhe_lut_bootstrap_dev(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), btk.ks_log_beta, btk.ks_l,
                                               btk.ksk.data_ptr(), t_bits, dl.data_ptr(), len(p.tables), pool.data_ptr(), p.n_slots * S, d_desc,
                                               d_out, count * S, st)
            else:
                binding.tlwe_lincomb_dev(btk.n_lwe, pool.data_ptr(), p.n_slots * S, d_desc, d_out, count * S, st)
        if not p.outputs:
            return []
        outs = _from_dev(torch.stack([pool[s * S:s * S + batch] for s in p.outputs]))
        return [TLWE(o) for o in outs]


# ---- packing key switch, a test vector per row and two-digit tree lookups ----------------------------------------
class PackingKeySwitchKey:
    """the packing key switching key [n_in][l][(k+1)][n] (numpy or a device tensor) kept on the device: entry [j][d] is a
    TGLWE under the GLWE key of the constant polynomial K_in[j] 2^(64 - log_beta (d+1)), K_in the key of the TLWEs that
    are packed (in tree_lookup: the LWE key of the BootstrappingKey, n_in = n_lwe)"""

    def __init__(self, pksk, log_beta, l):
        torch = _torch()
        shape = tuple(pksk.shape)
        if len(shape) != 4 or shape[1] != l:
            raise ValueError("pksk must be [n_in][l][(k+1)][n]")
        self.n_in, self.l, k1, self.n = shape
        self.k, self.log_beta = k1 - 1, log_beta
        words = binding.tfhe_pksk_words(self.n, self.k, self.n_in, log_beta, l)
        self.pksk = _dev_words(pksk)
        if words == 0 or self.pksk.numel() != words:
            raise binding.FheError(binding.FHE_E_INVALID, f"no packing key switch for pksk of shape {shape}, (log_beta, l) = ({log_beta}, {l})")
        torch.cuda.synchronize()


def packing_key_switch(pk, c, log_stride):
    """c: TLWEs [groups][count][n_in + 1] (or [count][n_in + 1]: one group) under the key `pk` switches from -> TGLWE
    [groups] whose phase holds phase(c_{g,i}) at coefficient i 2^log_stride (count 2^log_stride <= n)"""
    torch = _torch()
    w = c.words if c.words.ndim == 3 else c.words[None]
    groups, count, row = w.shape
    if row != pk.n_in + 1:
        raise ValueError(f"packing_key_switch: the TLWEs have dimension {row - 1}, the key switches from {pk.n_in}")
    dx = _to_dev(w)
    out = torch.empty((groups, pk.k + 1, pk.n), dtype=torch.int64, device="cuda")
    binding.tlwe_gadget_packing_key_switch_dev(pk.n, pk.k, pk.n_in, pk.log_beta, pk.l, pk.pksk.data_ptr(), dx.data_ptr(), count * row, row, count,
                                               log_stride, out.data_ptr(), groups)
    o = _from_dev(out)
    o = o if c.words.ndim == 3 else o[0]
    return TGLWE(o[..., : pk.k, :], o[..., pk.k, :])


def box_expand(tglwe, t_bits):
    """every component times X^-half (1 + X + .. + X^(box-1)), box = n >> t_bits, half = box / 2: a packed TGLWE holding m_q
    at coefficient q box becomes the test vector (make_lut's expansion) of the table q -> m_q"""
    torch = _torch()
    x = tglwe.packed()
    k1, n = x.shape[-2], x.shape[-1]
    batch = x.size // (k1 * n)
    dx = _to_dev(x.reshape(batch, k1, n))
    out = torch.empty((batch, k1, n), dtype=torch.int64, device="cuda")
    binding.tglwe_box_expand_dev(n, k1 - 1, t_bits, dx.data_ptr(), out.data_ptr(), batch)
    o = _from_dev(out).reshape(x.shape)
    return TGLWE(o[..., : k1 - 1, :], o[..., k1 - 1, :])


def bootstrap_rows(btk, tables, c):
    """bootstrapping with a test vector per row: tables is a TGLWE batch (full TGLWEs, e.g. encrypted test vectors from
    box_expand), row b of c rotates tables[b]; btk a gadget BootstrappingKey"""
    torch = _torch()
    _lut_key(btk)
    x = c.words.reshape(-1, btk.n_lwe + 1)
    t = tables.packed().reshape(-1, btk.k + 1, btk.n)
    if t.shape[0] != x.shape[0]:
        raise ValueError("bootstrap_rows: one test vector per row")
    out = torch.empty(x.shape, dtype=torch.int64, device="cuda")
    dt, dx = _to_dev(t), _to_dev(x)
    binding.tfhe_gadget_bootstrap_rows_dev(btk.n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), dt.data_ptr(), btk.ks_log_beta,
                                           btk.ks_l, btk.ksk.data_ptr(), dx.data_ptr(), out.data_ptr(), x.shape[0])
    return TLWE(_from_dev(out).reshape(c.words.shape))


def tree_lookup(btk, pksk, t_bits, table2d, x, y, nu=0, *, which=None):
    """table2d[x][y] of two encrypted t_bits-bit digits (the tree-based functional bootstrap): table2d
    [P][P] torus words (P = 2^t_bits, any output encoding, as make_lut's `out`); x, y TLWE batches under the LWE key of btk;
    pksk a PackingKeySwitchKey from that LWE key to the GLWE key.  Level 1 looks y up in the P tables table2d[j]: nu = 0
    is one fhe_tfhe_lut_bootstrap_dev over P batch rows, nu = t_bits one fhe_tfhe_lut_many_bootstrap_dev over batch rows
    (t_bits <= min(log2 n - t_bits, 4); it costs t_bits bits of mod-switch precision).  Then one packing key
    switch (count P, stride box), one box expansion and one bootstrap_rows on x, all on the device: the host waits only
    for the result.  Both digits keep the padding bit of DESIGN.md §14.  A batch may mix functions: table2d [R][P][P] with
    which [batch] naming each row's table (default: table 0)."""
    torch = _torch()
    _lut_key(btk)
    n, row, P = btk.n, btk.n_lwe + 1, 1 << t_bits
    L = int(n).bit_length() - 1
    if nu not in (0, t_bits):
        raise ValueError(f"tree_lookup: nu must be 0 or t_bits (nu={nu}, t_bits={t_bits})")
    if not 1 <= t_bits <= L or (nu and t_bits > min(L - t_bits, 4)):
        raise ValueError(f"tree_lookup: t_bits={t_bits} does not fit n={n}" + (" with nu = t_bits" if nu else ""))
    if (pksk.n, pksk.k, pksk.n_in) != (n, btk.k, btk.n_lwe):
        raise ValueError("tree_lookup: the packing key must switch from the LWE key of btk to its GLWE key")
    tabs = np.ascontiguousarray(np.asarray(table2d, dtype=np.uint64))
    tabs = tabs[None] if tabs.ndim == 2 else tabs
    xs, ys = x.words.reshape(-1, row), y.words.reshape(-1, row)
    batch = xs.shape[0]
    if tabs.shape[1:] != (P, P) or ys.shape != xs.shape:
        raise ValueError(f"tree_lookup: table2d must be [{P}][{P}] (or [R][{P}][{P}]) and x, y batches of the same shape")
    first = np.zeros(batch, dtype=np.int64) if which is None else np.asarray(which, dtype=np.int64).reshape(-1) * P
    if len(first) != batch or first.min() < 0 or first.max() >= len(tabs) * P:
        raise ValueError("tree_lookup: `which` needs one table index below len(table2d) per row")
    dx, dy, dl = _to_dev(xs), _to_dev(ys), _to_dev(tabs)
    lvl1 = torch.empty((P * batch, row), dtype=torch.int64, device="cuda")
    g = np.arange(batch, dtype=np.int64)
    if nu:                                                          # [P][batch] rows, function-major: item j of group g is row j batch + g
        desc = np.stack([first, g, np.full(batch, LUT_NONE), np.ones(batch, dtype=np.int64),
                         np.zeros(batch, dtype=np.int64), np.zeros(batch, dtype=np.int64)], axis=1)
        dd = _desc_dev(_lut_desc(desc))
        binding.tfhe_lut_many_bootstrap_dev(n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), btk.ks_log_beta, btk.ks_l,
                                            btk.ksk.data_ptr(), t_bits, nu, dl.data_ptr(), len(tabs) * P, dy.data_ptr(), batch, dd.data_ptr(),
                                            lvl1.data_ptr(), batch)
        gstride, istride = row, batch * row
    else:                                                           # [batch][P] rows: row g P + j looks y_g up in table2d[j]
        gg, jj = np.repeat(g, P), np.tile(np.arange(P, dtype=np.int64), batch)
        desc = np.stack([jj + np.repeat(first, P), gg, np.full(P * batch, LUT_NONE), np.ones(P * batch, dtype=np.int64), np.zeros(P * batch, dtype=np.int64),
                         np.zeros(P * batch, dtype=np.int64)], axis=1)
        dd = _desc_dev(_lut_desc(desc))
        binding.tfhe_lut_bootstrap_dev(n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), btk.ks_log_beta, btk.ks_l, btk.ksk.data_ptr(),
                                       t_bits, dl.data_ptr(), len(tabs) * P, dy.data_ptr(), batch, dd.data_ptr(), lvl1.data_ptr(), P * batch)
        gstride, istride = P * row, row
    packed = torch.empty((batch, btk.k + 1, n), dtype=torch.int64, device="cuda")
    tv = torch.empty_like(packed)
    out = torch.empty((batch, row), dtype=torch.int64, device="cuda")
    binding.tlwe_gadget_packing_key_switch_dev(n, btk.k, btk.n_lwe, pksk.log_beta, pksk.l, pksk.pksk.data_ptr(), lvl1.data_ptr(), gstride, istride, P,
                                               L - t_bits, packed.data_ptr(), batch)
    binding.tglwe_box_expand_dev(n, btk.k, t_bits, packed.data_ptr(), tv.data_ptr(), batch)
    binding.tfhe_gadget_bootstrap_rows_dev(n, btk.k, btk.log_beta, btk.l, btk.n_lwe, btk.bsk.data_ptr(), tv.data_ptr(), btk.ks_log_beta, btk.ks_l,
                                           btk.ksk.data_ptr(), dx.data_ptr(), out.data_ptr(), batch)
    return TLWE(_from_dev(out).reshape(x.words.shape))


# ---- key generation, encryption and decryption: the client side ------------------------------------------------
def cdt_table(sigma):
    """the error table of fhe_tlwe_encrypt_dev / fhe_tglwe_encrypt_dev for a discrete Gaussian of deviation sigma: strictly
    increasing u64 thresholds below 2^63, entry i = round(2^63 P(magnitude <= i)) for P(0) ~ rho(0), P(j) ~ 2 rho(j), rho(x) =
    exp(-x^2 / 2 sigma^2), j <= ceil(12 sigma).  The tail whose thresholds no longer differ at 2^-63 (or reach 2^63) is cut:
    its mass, below 2^-62, falls on the last magnitude kept.  sigma = 0 gives the empty table (no error).  Computed with
    50-digit decimals, so the rounding of the thresholds is the only error."""
    import decimal
    from fractions import Fraction

    sigma = float(sigma)
    if sigma < 0 or not np.isfinite(sigma):
        raise ValueError(f"cdt_table: sigma={sigma} must be a finite number >= 0")
    if sigma == 0:
        return np.zeros(0, dtype=np.uint64)
    top = int(np.ceil(12 * sigma))
    if top > 1024:
        raise ValueError(f"cdt_table: sigma={sigma} needs more than 1024 thresholds; use a smaller sigma with log_scale")
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        two_s2 = 2 * decimal.Decimal(sigma) ** 2
        rho = [Fraction((-(decimal.Decimal(j) ** 2) / two_s2).exp()) for j in range(top + 1)]
    weights = [rho[0]] + [2 * r for r in rho[1:]]
    total, run, out = sum(weights), Fraction(0), []
    for wgt in weights[:-1]:
        run += wgt
        thr = round(run / total * (1 << 63))
        if thr >= 1 << 63 or (out and thr <= out[-1]):
            break
        out.append(thr)
    return np.array(out, dtype=np.uint64)


def _gadget_i64(log_beta, l):
    """g_d = 2^(64 - b(d+1)) of DESIGN.md §11 as int64 words (2^63 wraps to the most negative value)"""
    if not (1 <= log_beta and 1 <= l and log_beta * l <= 64):
        raise ValueError(f"gadget (log_beta, l) = ({log_beta}, {l}) needs 1 <= log_beta, 1 <= l and log_beta l <= 64")
    g = [1 << (64 - log_beta * (d + 1)) for d in range(l)]
    return [x - (1 << 64) if x >= 1 << 63 else x for x in g]


def _i64(x, like=None):
    """0/1 key words (numpy u64 or a torch tensor) as a torch int64 tensor, on the device of `like` if given"""
    torch = _torch()
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64))
    return t if like is None else t.to(like.device)


# The message builders: what each key encrypts, as int64 torch tensors on the device of the keys they are given (wrapping
# arithmetic; no hot path: a key is built once).  Each returns one message per sample, in the order of the key's layout.
def bsk_messages(s_glwe, s_lwe, log_beta, l):
    """gadget BSK [n_lwe][(k+1)][l][(k+1)][N], k = 1 -> messages [n_lwe][2][l][N]: TGLev 0 of bit i holds -S bit_i g_d, TGLev 1
    the constant polynomial bit_i g_d"""
    torch = _torch()
    S, bits = _i64(s_glwe), _i64(s_lwe, _i64(s_glwe))
    g = torch.tensor(_gadget_i64(log_beta, l), dtype=torch.int64, device=S.device)
    mu = torch.zeros((len(bits), 2, l, len(S)), dtype=torch.int64, device=S.device)
    bg = bits[:, None] * g[None, :]
    mu[:, 0] = -(bg[:, :, None] * S[None, None, :])
    mu[:, 1, :, 0] = bg
    return mu


def ksk_messages(s_in, log_beta, l):
    """gadget KSK [n_in][l][n_out + 1] -> message words [n_in][l]: s_in[i] g_d"""
    torch = _torch()
    s = _i64(s_in)
    return s[:, None] * torch.tensor(_gadget_i64(log_beta, l), dtype=torch.int64, device=s.device)[None, :]


def pfksk_messages(s_glwe, log_beta, l):
    """PFKSK [(k+1)][k N + 1][l][(k+1)][N], k = 1 -> messages [2][N + 1][l][N]: with K~ = (-S_0 .. -S_{N-1}, 1), entry [0][j][d]
    holds -S K~_j g_d and entry [1][j][d] the constant polynomial K~_j g_d"""
    torch = _torch()
    S = _i64(s_glwe)
    g = torch.tensor(_gadget_i64(log_beta, l), dtype=torch.int64, device=S.device)
    kt = torch.cat([-S, torch.ones(1, dtype=torch.int64, device=S.device)])
    sc = kt[:, None] * g[None, :]
    mu = torch.zeros((2, len(S) + 1, l, len(S)), dtype=torch.int64, device=S.device)
    mu[0] = -(sc[:, :, None] * S[None, None, :])
    mu[1, :, :, 0] = sc
    return mu


def pksk_messages(s_in, n, log_beta, l):
    """PKSK [n_in][l][(k+1)][N] -> messages [n_in][l][N]: the constant polynomial K_in[j] g_d"""
    torch = _torch()
    s = _i64(s_in)
    mu = torch.zeros((len(s), l, n), dtype=torch.int64, device=s.device)
    mu[:, :, 0] = ksk_messages(s, log_beta, l)
    return mu


class ClientKey:
    """Both secrets of the §11-§16 evaluator, resident on the device, and everything made from them: evaluation keys,
    ciphertexts, phases.  k = 1.  The 32-byte seed is the whole secret: every key bit, mask word and error
    sample is a word of the ChaCha20 stream it keys, addressed by (purpose, row index).

    Row indices.  Secret keys: KEY row 0 is the LWE key, KEY row 1 the GLWE key.  Samples (MASK and ERR rows, LWE and TGLWE
    alike) are dealt out so that no two samples of one seed share a row:
        [0, 2^56)                       fresh encryptions, in the order of the encrypt_* calls (the key keeps the next row)
        [1 2^56 + slot 2^40, ..)        bootstrapping_key: the n_lwe 2 l TGLWE rows of the BSK, then the N ks_l LWE rows of the KSK
        [2 2^56 + slot 2^40, ..)        circuit_bootstrapping_key: the 2 (N + 1) pf_l TGLWE rows of the PFKSK
        [3 2^56 + slot 2^40, ..)        packing_key_switch_key: the n_lwe l TGLWE rows of the PKSK
    A builder refuses a `slot` (0 <= slot < 2^16) it has already used on this object: a second key of the same kind needs a
    slot of its own.  A ClientKey regenerated from the same seed starts its counters again: do not encrypt fresh data under
    both.  noise = (sigma, log_scale): errors are a discrete Gaussian of deviation sigma (cdt_table) times 2^log_scale."""

    ENCRYPT_ROWS = 1 << 56
    BSK_BASE, PFKSK_BASE, PKSK_BASE = 1 << 56, 2 << 56, 3 << 56
    SLOT_ROWS = 1 << 40

    def __init__(self, seed, n, n_lwe, s_lwe, s_glwe, noise):
        self.seed, self.n, self.k, self.n_lwe, self.noise = bytes(seed), n, 1, n_lwe, noise
        self.s_lwe, self.s_glwe = s_lwe, s_glwe
        self._next_row, self._slots, self._cdt = 0, set(), {}

    @classmethod
    def generate(cls, seed, n, n_lwe, noise=(3.2, 0)):
        """both binary secrets from the KEY stream of `seed` (32 bytes): s_lwe [n_lwe] and s_glwe [n], int64 device tensors"""
        torch = _torch()
        if n_lwe < 1 or n < 256 or n > 4096 or n & (n - 1):
            raise binding.FheError(binding.FHE_E_INVALID, f"ClientKey: needs n_lwe >= 1 and n a power of two in [256, 4096] (n={n}, n_lwe={n_lwe})")
        s_lwe = torch.empty(n_lwe, dtype=torch.int64, device="cuda")
        s_glwe = torch.empty(n, dtype=torch.int64, device="cuda")
        binding.tfhe_stream_words_dev(seed, binding.FHE_STREAM_KEY, 0, n_lwe, s_lwe.data_ptr(), 1, bits=True)
        binding.tfhe_stream_words_dev(seed, binding.FHE_STREAM_KEY, 1, n, s_glwe.data_ptr(), 1, bits=True)
        torch.cuda.synchronize()
        return cls(seed, n, n_lwe, s_lwe, s_glwe, noise)

    # -- plumbing ---------------------------------------------------------------------------------------------------
    def _noise(self, noise):
        """-> (device table or None, m, log_scale)"""
        sigma, log_scale = self.noise if noise is None else noise
        if sigma not in self._cdt:
            tab = cdt_table(sigma)
            self._cdt[sigma] = (_to_dev(tab) if len(tab) else None, len(tab))
        d, m = self._cdt[sigma]
        return d, m, int(log_scale)

    def _take_slot(self, kind, base, slot):
        if not 0 <= int(slot) < 1 << 16:
            raise ValueError(f"{kind}: slot must be in [0, 2^16)")
        if (kind, int(slot)) in self._slots:
            raise ValueError(f"{kind}: slot {slot} of this seed is already used; a second key needs a slot of its own")
        self._slots.add((kind, int(slot)))
        return base + int(slot) * self.SLOT_ROWS

    def _tglwe_rows(self, first_row, messages, noise):
        """messages [rows][N] (an int64 device tensor of any shape [..][N]) -> TGLWE samples [rows][2][N] on rows first_row .."""
        torch = _torch()
        d_cdt, m, log_scale = self._noise(noise)
        msg = messages.reshape(-1, self.n).contiguous()
        out = torch.empty((msg.shape[0], 2, self.n), dtype=torch.int64, device="cuda")
        binding.tglwe_encrypt_dev(self.n, 1, self.seed, first_row, self.s_glwe.data_ptr(), msg.data_ptr(), self.n, d_cdt.data_ptr() if m else None, m,
                                  log_scale, out.data_ptr(), msg.shape[0])
        return out

    def _tlwe_rows(self, first_row, s, mu, noise):
        """message words mu [rows] (int64 device tensor) -> LWE samples [rows][len(s) + 1] under s"""
        torch = _torch()
        d_cdt, m, log_scale = self._noise(noise)
        mu = mu.reshape(-1).contiguous()
        out = torch.empty((mu.shape[0], len(s) + 1), dtype=torch.int64, device="cuda")
        binding.tlwe_encrypt_dev(len(s), self.seed, first_row, s.data_ptr(), mu.data_ptr(), d_cdt.data_ptr() if m else None, m, log_scale,
                                 out.data_ptr(), mu.shape[0])
        return out

    # -- evaluation keys --------------------------------------------------------------------------------------------
    def bootstrapping_key(self, bsk, ksk, noise=None, slot=0):
        """bsk = (log_beta, l), ksk = (ks_log_beta, ks_l) -> the gadget BootstrappingKey: the BSK of the LWE key bits under the
        GLWE key, and the KSK from the extracted GLWE key back to the LWE key"""
        (b, l), (ks_b, ks_l) = bsk, ksk
        if binding.tfhe_gadget_bsk_prepared_words(self.n, 1, b, l, self.n_lwe) == 0:
            raise binding.FheError(binding.FHE_E_INVALID, f"no gadget bootstrapping key for n={self.n}, (log_beta, l) = ({b}, {l})")
        _gadget_i64(ks_b, ks_l)
        first = self._take_slot("bootstrapping_key", self.BSK_BASE, slot)
        rows = self._tglwe_rows(first, bsk_messages(self.s_glwe, self.s_lwe, b, l), noise)
        kk = self._tlwe_rows(first + self.n_lwe * 2 * l, self.s_lwe, ksk_messages(self.s_glwe, ks_b, ks_l), noise)
        return BootstrappingKey(self.n, 1, l, self.n_lwe, rows.reshape(self.n_lwe, 2, l, 2, self.n), kk.reshape(self.n, ks_l, self.n_lwe + 1),
                                ks_l=ks_l, log_beta=b, ks_log_beta=ks_b)

    def circuit_bootstrapping_key(self, btk, cb, pf, noise=None, slot=0):
        """btk: a gadget BootstrappingKey of this key; cb = (cb_log_beta, cb_l), pf = (pf_log_beta, pf_l) -> CircuitBootstrappingKey
        with a PFKSK built here"""
        (cb_b, cb_l), (pf_b, pf_l) = cb, pf
        if (btk.n, btk.k, btk.n_lwe) != (self.n, 1, self.n_lwe):
            raise ValueError("circuit_bootstrapping_key: btk is not a key of this ClientKey's shape")
        if binding.tfhe_pfksk_words(self.n, 1, pf_b, pf_l) == 0:
            raise binding.FheError(binding.FHE_E_INVALID, f"no private key switch for n={self.n}, (pf_log_beta, pf_l) = ({pf_b}, {pf_l})")
        first = self._take_slot("circuit_bootstrapping_key", self.PFKSK_BASE, slot)
        rows = self._tglwe_rows(first, pfksk_messages(self.s_glwe, pf_b, pf_l), noise)
        return CircuitBootstrappingKey(btk, rows.reshape(2, self.n + 1, pf_l, 2, self.n), cb_b, cb_l, pf_b, pf_l)

    def packing_key_switch_key(self, pks, noise=None, slot=0):
        """pks = (log_beta, l) -> the PackingKeySwitchKey from the LWE key to the GLWE key"""
        b, l = pks
        if binding.tfhe_pksk_words(self.n, 1, self.n_lwe, b, l) == 0:
            raise binding.FheError(binding.FHE_E_INVALID, f"no packing key switch for n={self.n}, n_in={self.n_lwe}, (log_beta, l) = ({b}, {l})")
        first = self._take_slot("packing_key_switch_key", self.PKSK_BASE, slot)
        rows = self._tglwe_rows(first, pksk_messages(self.s_lwe, self.n, b, l), noise)
        return PackingKeySwitchKey(rows.reshape(self.n_lwe, l, 2, self.n), b, l)

    # -- ciphertexts ------------------------------------------------------------------------------------------------
    def encrypt_words(self, mu, noise=None):
        """torus words mu (any shape) -> TLWE of the same leading shape under the LWE key, on fresh rows"""
        torch = _torch()
        w = np.ascontiguousarray(mu, dtype=np.uint64)
        if self._next_row + w.size > self.ENCRYPT_ROWS:
            raise ValueError("encrypt: this seed's 2^56 encryption rows are used up")
        out = self._tlwe_rows(self._next_row, self.s_lwe, _to_dev(w.reshape(-1)), noise)
        self._next_row += w.size
        return TLWE(_from_dev(out).reshape(w.shape + (self.n_lwe + 1,)))

    def encrypt_int(self, x, t_bits, noise=None):
        """values in [0, 2^t_bits) in §14's encoding (encode_int): phase x 2^(63 - t_bits) + e, the top bit padding"""
        return self.encrypt_words(encode_int(x, t_bits), noise)

    def encrypt_bit(self, bit, noise=None, *, msb=False):
        """bits in §13's gate encoding, phase +-2^61; msb=True: phase bit 2^63, what circuit_bootstrap takes (§12)"""
        bits = np.asarray(bit).astype(bool)
        words = np.where(bits, np.uint64(1 << 63), np.uint64(0)) if msb else np.where(bits, np.uint64(MU), np.uint64((1 << 64) - MU))
        return self.encrypt_words(words.astype(np.uint64), noise)

    def phase(self, c):
        """b - <a, s> of a TLWE (under the LWE key, or under the extracted GLWE key when its dimension is n != n_lwe), or
        B - A S of a TGLWE: u64 words"""
        torch = _torch()
        if isinstance(c, TGLWE):
            x = c.packed()
            d = _to_dev(x.reshape(-1, 2, self.n))
            out = torch.empty((d.shape[0], self.n), dtype=torch.int64, device="cuda")
            binding.tglwe_phase_dev(self.n, 1, self.s_glwe.data_ptr(), d.data_ptr(), out.data_ptr(), d.shape[0])
            return _from_dev(out).reshape(x.shape[:-2] + (self.n,))
        w = c.words if isinstance(c, TLWE) else np.asarray(c, dtype=np.uint64)
        s = self.s_lwe if w.shape[-1] - 1 == self.n_lwe else self.s_glwe
        if w.shape[-1] - 1 != len(s):
            raise ValueError(f"phase: a TLWE of dimension {w.shape[-1] - 1} is under neither key ({self.n_lwe}, {self.n})")
        d = _to_dev(w.reshape(-1, len(s) + 1))
        out = torch.empty(d.shape[0], dtype=torch.int64, device="cuda")
        binding.tlwe_phase_dev(len(s), s.data_ptr(), d.data_ptr(), out.data_ptr(), d.shape[0])
        return _from_dev(out).reshape(w.shape[:-1])

    def decrypt_int(self, c, t_bits, *, padding=False):
        """round(phase / Delta) mod 2^t_bits, Delta = 2^(63 - t_bits) (padding=True: mod 2^(t_bits + 1), the padding bit kept)"""
        p = self.phase(c)
        v = ((p >> np.uint64(62 - t_bits)) + np.uint64(1)) >> np.uint64(1)
        return v.astype(np.int64) & ((2 << t_bits) - 1 if padding else (1 << t_bits) - 1)

    def decrypt_bit(self, c, *, msb=False):
        """gate encoding: 1 where the centred phase is positive; msb=True: round(phase / 2^63) mod 2"""
        p = self.phase(c)
        if msb:
            return ((((p >> np.uint64(62)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(1)).astype(np.int64)
        return (p.view(np.int64) > 0).astype(np.int64)
