"""Host mirror of the reference's BFV surface (bfv/src/lib.rs) over the C ABI: the product path — `RLWE::tensor`,
`BFV::relinearize_204`, `RLWE::mul` (lib.rs:59-90, 251-271) — and the client side — `new_key`, `encrypt`, `decrypt`,
`add_const`, `mul_const`, `rlk_key` (lib.rs:118-225) — on the device (`Param`, `ClientKey`, `PublicKey`).

    reference (Rust)                         here
    RLWE(Rq, Rq)                lib.rs:47    RLWE(c0, c1)          (coefficients mod q)
    RLK(Rq, Rq)  mod p*q        lib.rs:43    RLK(rlk0, rlk1, pq)
    RLWE::tensor(t, &a, &b)     lib.rs:59    RLWE.tensor(t, a, b) -> (c0, c1, c2)
    RLWE::mul(t, &rlk, &a, &b)  lib.rs:87    RLWE.mul(t, rlk, a, b)
    Param { ring, t, p }        lib.rs:20    Param(ring, t, p)
    BFV::new_key(rng, &param)   lib.rs:120   ClientKey.generate(seed, param), .public_key(slot)
    BFV::rlk_key(rng, ..)       lib.rs:202   ClientKey.relin_key(slot)
    BFV::encrypt / decrypt      lib.rs:142   ClientKey.encrypt(pk, m) / .decrypt(ct)
    BFV::add_const / mul_const  lib.rs:180   add_const(ct, m) / mul_const(rlk, ct, m)
"""
from dataclasses import dataclass

import numpy as np

from . import binding
from .arith import RingParam, Rq, plan_of as _plan
from .device import from_dev as _from_dev, to_dev as _to_dev, torch as _torch
from .rlwe_client import ClientKeyBase, PublicKey  # noqa: F401  (PublicKey: lib.rs:39, exported from here)


@dataclass
class RLK:
    """relinearisation key, coefficients mod p*q (lib.rs:41-43)"""
    rlk0: np.ndarray
    rlk1: np.ndarray
    pq: int


class RLWE:
    """RLWE ciphertext (c0, c1), lib.rs:45-47; `c0`/`c1` are arith.Rq (or batches of them)."""

    def __init__(self, c0, c1):
        if c0.param != c1.param:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "RLWE components differ in RingParam")
        self.c0, self.c1 = c0, c1

    @property
    def param(self):
        return self.c0.param

    def __add__(self, rhs):
        """lib.rs:50-52: (c0 + c0', c1 + c1') with fhe_rq_add_dev"""
        p = self.param
        if rhs.param != p or rhs.c0.coeffs.shape != self.c0.coeffs.shape:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "operands differ in RingParam or shape")
        a, b = _to_dev(np.stack([self.c0.coeffs, self.c1.coeffs])), _to_dev(np.stack([rhs.c0.coeffs, rhs.c1.coeffs]))
        c = _torch().empty_like(a)
        binding._check(binding.load_library().fhe_rq_add_dev(_plan(p).handle, a.data_ptr(), b.data_ptr(), c.data_ptr(), a.numel() // p.n, None))
        out = _from_dev(c)
        return RLWE(Rq(p, out[0]), Rq(p, out[1]))

    @staticmethod
    def tensor(t, a, b):
        """lib.rs:59-85 → (c0, c1, c2) as Rq mod q"""
        p = a.param
        if b.param != p:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "operands differ in RingParam")
        c = binding.bfv_tensor(p.q, p.n, t, a.c0.coeffs, a.c1.coeffs, b.c0.coeffs, b.c1.coeffs)
        shape = a.c0.coeffs.shape
        return tuple(Rq(p, x.reshape(shape)) for x in c)

    @staticmethod
    def mul(t, rlk, a, b):
        """lib.rs:87-90: relinearize_204(rlk, tensor(t, a, b))"""
        p = a.param
        if b.param != p:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "operands differ in RingParam")
        o0, o1 = binding.bfv_mul(p.q, p.n, t, rlk.pq, rlk.rlk0, rlk.rlk1,
                                 a.c0.coeffs, a.c1.coeffs, b.c0.coeffs, b.c1.coeffs)
        shape = a.c0.coeffs.shape
        return RLWE(Rq(p, o0.reshape(shape)), Rq(p, o1.reshape(shape)))


# ---- the client side (lib.rs:118-225) on the device: DESIGN.md §20 ----------------------------------------------------------------
@dataclass(frozen=True)
class Param:
    """lib.rs:20-24: the ciphertext ring, the plaintext modulus t and the relinearisation modulus factor p (0: no rlk)"""
    ring: RingParam
    t: int
    p: int = 0

    def pt(self):
        """the plaintext RingParam, lib.rs:27-32"""
        return RingParam(self.t, self.ring.n)


def _delta_m(ring, t, m, shape):
    """Delta (m mod q) on the device: fhe_rq_remodule_dev then fhe_rq_mul_by_u64_dev, as lib.rs:185-187 -> u64 words of `shape`"""
    L = binding.load_library()
    d = _to_dev(np.broadcast_to(np.ascontiguousarray(m, dtype=np.uint64), shape).copy())
    r, out = _torch().empty_like(d), _torch().empty_like(d)
    binding._check(L.fhe_rq_remodule_dev(ring.q, d.data_ptr(), r.data_ptr(), d.numel(), None))
    binding._check(L.fhe_rq_mul_by_u64_dev(_plan(ring).handle, r.data_ptr(), ring.q // t, out.data_ptr(), d.numel() // ring.n, None))
    return out


def add_const(ct, m):
    """BFV::add_const, lib.rs:180-188: m an Rq mod t (or its coefficients with `t` in m.param.q) -> (c0 + Delta m, c1)"""
    ring, t = ct.param, m.param.q
    d = _delta_m(ring, t, m.coeffs, ct.c0.coeffs.shape)
    c0 = _to_dev(ct.c0.coeffs)
    out = _torch().empty_like(c0)
    binding._check(binding.load_library().fhe_rq_add_dev(_plan(ring).handle, c0.data_ptr(), d.data_ptr(), out.data_ptr(), c0.numel() // ring.n, None))
    return RLWE(Rq(ring, _from_dev(out)), Rq(ring, ct.c1.coeffs.copy()))


def mul_const(rlk, ct, m):
    """BFV::mul_const, lib.rs:189-200: RLWE::mul by the noiseless ciphertext (Delta m, 0)"""
    ring, t = ct.param, m.param.q
    md = RLWE(Rq(ring, _from_dev(_delta_m(ring, t, m.coeffs, ct.c0.coeffs.shape))), Rq(ring, np.zeros_like(ct.c0.coeffs)))
    return RLWE.mul(t, rlk, ct, md)


class ClientKey(ClientKeyBase):
    """The BFV secret, resident on the device with its evals, and what is made from it: public keys, relinearisation keys,
    ciphertexts and plaintexts.  The 32-byte seed is the whole secret: every key bit, mask coefficient,
    ephemeral u and error is a word of the ChaCha20 stream it keys, addressed by (purpose, row).  Row indices never repeat
    within a seed:
        [0, 2^56)          fresh encryptions, in the order of the encrypt calls (the key keeps the next row)
        1 2^56 + slot      public_key(slot)
        2 2^56 + slot      relin_key(slot)
    and a builder refuses a slot (0 <= slot < 2^16) it has used.  The secret is KEY row 0.  A ClientKey regenerated from the
    same seed starts its counters again: do not encrypt fresh data under both.  sigma: the deviation of the discrete Gaussian
    errors (tfhe.cdt_table)."""

    RLK_BASE = 2 << 56

    def __init__(self, seed, param, d_s, d_s_evals, sigma):
        super().__init__(seed, sigma)
        self.param, self.d_s, self.d_s_evals = param, d_s, d_s_evals

    @classmethod
    def generate(cls, seed, param, sigma=3.2):
        torch = _torch()
        n, plan = param.ring.n, _plan(param.ring)
        d_s = torch.empty(n, dtype=torch.int64, device="cuda")
        d_e = torch.empty(n, dtype=torch.int64, device="cuda")
        binding.bfv_secret_key_dev(n, seed, 0, d_s.data_ptr())
        plan.forward_dev(d_s.data_ptr(), d_e.data_ptr(), 1)
        torch.cuda.synchronize()
        return cls(seed, param, d_s, d_e, sigma)

    def public_key(self, slot=0):
        """BFV::new_key's pk = (-a s + e, a), lib.rs:134-137"""
        return self._public_key(binding.bfv_public_key_dev, self.param.ring, slot)

    def relin_key(self, slot=0):
        """BFV::rlk_key, lib.rs:202-225, exactly (n p q < 2^63) -> RLK"""
        torch = _torch()
        ring, pq = self.param.ring, self.param.p * self.param.ring.q
        if self.param.p < 1:
            raise ValueError("relin_key: Param.p is 0")
        row = self._take_slot("relin_key", self.RLK_BASE, slot)
        out = torch.empty((2, ring.n), dtype=torch.int64, device="cuda")
        binding.bfv_relin_key_dev(ring.q, ring.n, pq, self.seed, row, self.d_s.data_ptr(), self._cdt_ptr(), self._m, out.data_ptr())
        w = _from_dev(out)
        return RLK(w[0].copy(), w[1].copy(), pq)

    def encrypt(self, pk, m):
        """BFV::encrypt, lib.rs:142-162: m an Rq mod t (coeffs (n,) or (batch, n)) -> RLWE on fresh rows"""
        torch = _torch()
        ring = self.param.ring
        if m.param != self.param.pt():
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the message is not in the plaintext ring")
        msg = m.coeffs.reshape(-1, ring.n)
        batch = msg.shape[0]
        d_m = _to_dev(msg)
        out = torch.empty((2, batch, ring.n), dtype=torch.int64, device="cuda")
        self._on_fresh_rows(batch, lambda row: binding.bfv_encrypt_dev(_plan(ring), self.param.t, self.seed, row, pk.d_evals.data_ptr(), d_m.data_ptr(), ring.n,
                                                                        self._cdt_ptr(), self._m, out.data_ptr(), batch))
        w = _from_dev(out)
        return RLWE(Rq(ring, w[0].reshape(m.coeffs.shape)), Rq(ring, w[1].reshape(m.coeffs.shape)))

    def decrypt(self, ct):
        """BFV::decrypt, lib.rs:164-178 -> Rq mod t"""
        torch = _torch()
        ring = self.param.ring
        if ct.param != ring:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the ciphertext is not in this key's ring")
        shape = ct.c0.coeffs.shape
        d_ct = _to_dev(np.stack([ct.c0.coeffs.reshape(-1, ring.n), ct.c1.coeffs.reshape(-1, ring.n)]))
        batch = d_ct.shape[1]
        out = torch.empty((batch, ring.n), dtype=torch.int64, device="cuda")
        binding.bfv_decrypt_dev(_plan(ring), self.param.t, self.d_s_evals.data_ptr(), d_ct.data_ptr(), out.data_ptr(), batch)
        return Rq(self.param.pt(), _from_dev(out).reshape(shape))
