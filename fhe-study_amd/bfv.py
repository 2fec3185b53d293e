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


# ---- BFV on an RNS modulus chain: exact ct x ct, batching, slot rotations (bfv_rns.hip) -------------------------------
def _ckks():
    """ckks.py, whose key builders and Galois key switch the chain uses unchanged; imported on first use"""
    from . import ckks
    return ckks


def _is_prime(x):
    """deterministic Miller-Rabin for x < 2^64 (the first twelve primes as bases)"""
    if x < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if x % p == 0:
            return x == p
    d, r = x - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in small:
        y = pow(a, d, x)
        if y in (1, x - 1):
            continue
        for _ in range(r - 1):
            y = y * y % x
            if y == x - 1:
                break
        else:
            return False
    return True


@dataclass(frozen=True)
class RnsParam:
    """n, the chain primes q_0 .. q_{k-1} (1 <= k <= 4, Q their product), the auxiliary base b_0 .. b_k (B its product), the
    special prime P >= max q_i of the switching keys and the plaintext modulus t.  Every prime is distinct, NTT-friendly for n
    (1 modulo 2n) and below 2^62; admission: B > t n Q + 1.  Every ciphertext lives at all k limbs."""
    n: int
    moduli: tuple
    aux: tuple
    special: int
    t: int

    def __post_init__(self):
        for name in ("moduli", "aux"):
            object.__setattr__(self, name, tuple(int(q) for q in getattr(self, name)))
        for name in ("n", "special", "t"):
            object.__setattr__(self, name, int(getattr(self, name)))
        n, k = self.n, len(self.moduli)
        if n < 2 or n & (n - 1) or n > 1 << 19:
            raise ValueError("RnsParam: n must be a power of two in [2, 2^19]")
        if not 1 <= k <= 4:
            raise ValueError("RnsParam: the chain has 1 to 4 primes")
        if len(self.aux) != k + 1:
            raise ValueError(f"RnsParam: the auxiliary base of a chain of {k} primes has {k + 1}")
        every = self.moduli + self.aux + (self.special,)
        if len(set(every)) != len(every):
            raise ValueError("RnsParam: the primes of the chain, the auxiliary base and the special prime must be distinct")
        for p in every:
            if p >= 1 << 62 or p % (2 * n) != 1 or not _is_prime(p):
                raise ValueError(f"RnsParam: {p} is not a prime below 2^62 that is 1 modulo 2n")
        if self.special < max(self.moduli):
            raise ValueError("RnsParam: the special prime must not be below a chain prime")
        if self.t < 2:
            raise ValueError("RnsParam: t must be at least 2")
        if not self.B > self.t * n * self.Q + 1:
            raise ValueError("RnsParam: the auxiliary base must exceed t n Q + 1")

    @property
    def Q(self):
        out = 1
        for q in self.moduli:
            out *= q
        return out

    @property
    def B(self):
        out = 1
        for b in self.aux:
            out *= b
        return out

    @property
    def max_level(self):
        return len(self.moduli) - 1

    @property
    def max_dot_weight(self):
        """the largest W = sum_r |w_r| that `dot` admits: B > t n Q W + 1, so floor((B - 2) / (t n Q)); at least 1"""
        return (self.B - 2) // (self.t * self.n * self.Q)

    def plans(self, level=None):
        """the plans of the chain (`level` is accepted for the CKKS key builders and must name every limb)"""
        if level is not None and level != self.max_level:
            raise ValueError("RnsParam: a BFV ciphertext lives at every limb")
        return [_plan(RingParam(q, self.n)) for q in self.moduli]

    def aux_plans(self):
        return [_plan(RingParam(b, self.n)) for b in self.aux]

    def special_plan(self):
        return _plan(RingParam(self.special, self.n))


class BatchEncoder:
    """t prime, t = 1 (mod 2n): the n slots of a plaintext as a 2 x n/2 matrix.  Slot (r, c) is the value of the polynomial at
    psi^e, e = 5^c mod 2n for r = 0 and 2n - 5^c for r = 1, which the engine's forward transform modulo t leaves at index
    brv((e - 1) / 2): encode and decode are that transform's inverse / forward composed with this index map.  sigma_g with
    g = 5^step rotates both rows left by `step`; g = 2n - 1 swaps the rows."""

    def __init__(self, n, t):
        n, t = int(n), int(t)
        if n < 2 or n & (n - 1):
            raise ValueError("BatchEncoder: n must be a power of two, at least 2")
        if t % (2 * n) != 1 or not _is_prime(t):
            raise ValueError("BatchEncoder: t must be a prime that is 1 modulo 2n")
        self.n, self.t = n, t
        self.index = slot_index(n)

    def _plan(self):
        return _plan(RingParam(self.t, self.n))

    def encode(self, slots):
        """[..][2][n/2] values modulo t -> coefficients [..][n] in [0, t)"""
        s = np.mod(np.asarray(slots, dtype=np.int64), self.t).astype(np.uint64)
        lead = s.shape[:-2]
        ev = np.zeros(lead + (self.n,), dtype=np.uint64)
        ev[..., self.index.reshape(-1)] = s.reshape(lead + (self.n,))
        return self._plan().inverse(ev.reshape(-1, self.n)).reshape(lead + (self.n,))

    def decode(self, m):
        """coefficients [..][n] modulo t -> slots [..][2][n/2]"""
        m = np.ascontiguousarray(m, dtype=np.uint64)
        ev = self._plan().forward(m.reshape(-1, self.n)).reshape(m.shape)
        return ev[..., self.index.reshape(-1)].reshape(m.shape[:-1] + (2, self.n // 2))


def slot_index(n):
    """-> int64 [2][n/2]: the index of slot (r, c) in the engine's order, brv(((+-5^c mod 2n) - 1) / 2) over log2 n bits"""
    L = n.bit_length() - 1
    idx = np.empty((2, max(n // 2, 1)), dtype=np.int64)
    for c in range(max(n // 2, 1)):
        e = pow(5, c, 2 * n)
        for r, ee in enumerate((e, 2 * n - e)):
            idx[r, c] = int(format((ee - 1) // 2, f"0{L}b")[::-1], 2)
    return idx


class RnsCiphertext:
    """A device tensor [k][2][batch][n] of evals over every limb of an RnsParam"""

    def __init__(self, param, d):
        self.param, self.d = param, d

    @property
    def batch(self):
        return self.d.shape[2]

    def _check(self, rhs):
        if rhs.param != self.param or rhs.batch != self.batch:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "operands differ in RnsParam or batch")

    def _rows(self, rhs, fn):
        self._check(rhs)
        out = _torch().empty_like(self.d)
        for i, plan in enumerate(self.param.plans()):
            binding._check(fn(plan.handle, self.d[i].data_ptr(), rhs.d[i].data_ptr(), out[i].data_ptr(), 2 * self.batch, None))
        return RnsCiphertext(self.param, out)

    def __add__(self, rhs):
        return self._rows(rhs, binding.load_library().fhe_rq_add_dev)

    def __sub__(self, rhs):
        return self._rows(rhs, binding.load_library().fhe_rq_sub_dev)

    def __neg__(self):
        out = _torch().empty_like(self.d)
        for i, plan in enumerate(self.param.plans()):
            binding._check(binding.load_library().fhe_rq_neg_dev(plan.handle, self.d[i].data_ptr(), out[i].data_ptr(), 2 * self.batch, None))
        return RnsCiphertext(self.param, out)

    def mul(self, rhs, rlk):
        """ct x ct: the scale-invariant tensor and its relinearisation (fhe_bfv_rns_mul_dev)"""
        self._check(rhs)
        p = self.param
        if rlk.param != p:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the relinearisation key is not of this ciphertext's chain")
        out = _torch().empty_like(self.d)
        binding.bfv_rns_mul_dev(p.plans(), p.aux_plans(), p.special_plan(), p.t, rlk.d_rlk.data_ptr(), self.d.data_ptr(), rhs.d.data_ptr(), out.data_ptr(), self.batch)
        return RnsCiphertext(p, out)

    def _rows_of(self, m):
        return np.array(np.broadcast_to(np.asarray(m, dtype=np.int64), (self.batch, self.param.n)))   # a writable copy

    def add_plain(self, m):
        """c0 + floor(Q / t) m for a plaintext m in [0, t)^n, (n,) or (batch, n)"""
        torch = _torch()
        p, n = self.param, self.param.n
        d_m = torch.from_numpy(np.mod(self._rows_of(m), p.t)).cuda()
        dm = torch.empty((len(p.moduli), self.batch, n), dtype=torch.int64, device="cuda")
        ev = torch.empty_like(dm)
        binding.bfv_rns_scale_msg_dev(p.plans(), p.t, d_m.data_ptr(), dm.data_ptr(), self.batch)
        out = self.d.clone()
        for i, plan in enumerate(p.plans()):
            binding.ckks_rns_from_i64_dev([plan], dm[i].data_ptr(), ev[i].data_ptr(), self.batch)
            binding._check(binding.load_library().fhe_rq_add_dev(plan.handle, self.d[i, 0].data_ptr(), ev[i].data_ptr(), out[i, 0].data_ptr(), self.batch, None))
        return RnsCiphertext(p, out)

    def mul_plain(self, m):
        """both components times the plaintext m in [0, t)^n, lifted centred into every limb (fhe_ckks_rns_from_i64_dev)"""
        torch = _torch()
        p = self.param
        rows = np.mod(self._rows_of(m), p.t)
        rows = np.where(rows > p.t // 2, rows - p.t, rows)
        pt = torch.empty((len(p.moduli), self.batch, p.n), dtype=torch.int64, device="cuda")
        binding.ckks_rns_from_i64_dev(p.plans(), torch.from_numpy(np.ascontiguousarray(rows)).cuda().data_ptr(), pt.data_ptr(), self.batch)
        out = torch.empty_like(self.d)
        for i, plan in enumerate(p.plans()):
            for c in range(2):
                plan.pointwise_mul_dev(self.d[i, c].data_ptr(), pt[i].data_ptr(), out[i, c].data_ptr(), self.batch)
        return RnsCiphertext(p, out)

    def rotate_many(self, gks):
        """sigma_g of this ciphertext for every key of `gks` from one call (fhe_ckks_rns_galois_dev): one digit decomposition"""
        torch = _torch()
        gks, p = list(gks), self.param
        if any(gk.param != p for gk in gks):
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "a Galois key is not of this ciphertext's chain")
        out = torch.empty((len(gks),) + tuple(self.d.shape), dtype=torch.int64, device="cuda")
        binding.ckks_rns_galois_dev(p.plans(), p.special_plan(), [gk.d_gk.data_ptr() for gk in gks], [gk.g for gk in gks], len(p.moduli), self.d.data_ptr(),
                                    out.data_ptr(), self.batch)
        return [RnsCiphertext(p, out[r]) for r in range(len(gks))]

    def rotate(self, gk):
        """both rows of the slot matrix moved left by the key's step; a key that is no rotation key is refused"""
        if not gk.is_rotation:
            raise ValueError(f"rotate: g={gk.g} is no power of 5 modulo 2n")
        return self.rotate_many([gk])[0]

    def swap_rows(self, gk):
        """the two rows of the slot matrix exchanged; a key of another element is refused"""
        if gk.g != 2 * self.param.n - 1:
            raise ValueError(f"swap_rows: g={gk.g} is not 2n - 1")
        return self.rotate_many([gk])[0]

    def square(self, rlk):
        """self x self: dot([self], [self], rlk)"""
        return dot([self], [self], rlk)

    def mul_const(self, c):
        """both components times the integer c, taken centred modulo t: lincomb([self], [c])"""
        return lincomb([self], [int(c)])[0]

    def diag_sum(self, pts, gks):
        """-> [sum_r m_{o,r} (.) sigma_{g_r}(self) for each output o] from one call (fhe_ckks_rns_diag_sum_dev): one digit
        decomposition for all elements and outputs.  pts is what encode_diagonals returns; gks[r] is the key of pts.gs[r], not
        read and possibly None where pts.gs[r] = 1."""
        torch = _torch()
        gks, p = list(gks), self.param
        if pts.param != p or any(gk is not None and gk.param != p for gk in gks):
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the plaintexts or a Galois key are not of this ciphertext's chain")
        if len(gks) != len(pts.gs):
            raise ValueError(f"diag_sum: {len(gks)} keys for {len(pts.gs)} elements")
        for r, (g, gk) in enumerate(zip(pts.gs, gks)):
            if g != 1 and gk is None:
                raise ValueError(f"diag_sum: element {r} (g={g}) has no key")
            if g != 1 and gk.g != g:
                raise ValueError(f"diag_sum: key {r} is of g={gk.g}, the plaintexts' element is {g}")
        out = torch.empty((pts.outputs,) + tuple(self.d.shape), dtype=torch.int64, device="cuda")
        binding.ckks_rns_diag_sum_dev(p.plans(), p.special_plan(), [None if g == 1 else gk.d_gk.data_ptr() for g, gk in zip(pts.gs, gks)], pts.gs, len(p.moduli),
                                      pts.d_pts.data_ptr(), pts.outputs, self.d.data_ptr(), out.data_ptr(), self.batch)
        return [RnsCiphertext(p, out[o]) for o in range(pts.outputs)]

    def linear_transform(self, lt, keys):
        """out[r] = M[r] in[r] mod t on the two slot rows for a LinearTransform, from one call (fhe_ckks_rns_bsgs_dev): the giant
        steps' rotations hoisted, one modulus-down.  keys: step -> Galois key for every step of lt.required_steps(); a missing
        one raises KeyError(step)."""
        missing = [st for st in lt.required_steps() if st not in keys]
        if missing:
            raise KeyError(missing[0])
        torch = _torch()
        pts, p = lt.pts, self.param
        baby = [keys[i] if i else None for i in lt.baby]
        giant = [keys[lt.n1 * j] if j else None for j in lt.giant]
        giant_gs = [_ckks().galois_element(p.n, lt.n1 * j) for j in lt.giant]
        if pts.param != p or any(gk is not None and gk.param != p for gk in baby + giant):
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the plaintexts or a Galois key are not of this ciphertext's chain")
        for g, gk in zip(pts.gs + giant_gs, baby + giant):
            if g != 1 and gk.g != g:
                raise ValueError(f"linear_transform: a key is of g={gk.g}, its step's element is {g}")
        out = torch.empty_like(self.d)
        binding.ckks_rns_bsgs_dev(p.plans(), p.special_plan(), [None if gk is None else gk.d_gk.data_ptr() for gk in baby], pts.gs,
                                  [None if gk is None else gk.d_gk.data_ptr() for gk in giant], giant_gs, len(p.moduli), pts.d_pts.data_ptr(), self.d.data_ptr(),
                                  out.data_ptr(), self.batch)
        return RnsCiphertext(p, out)


# ---- inner products, scalar sums and linear transforms over Z_t --------------------------------------------------------
def centred(x, t):
    """the Python integer x modulo t, in (-t / 2, t / 2]"""
    x = int(x) % t
    return x - t if x > t // 2 else x


def dot_weights(param, count, weights=None):
    """the weights of `dot` -> (w, W): Python integers centred modulo t, W the sum of their absolute values; w is None where
    `weights` is None or every weight is 1 (the kernel then multiplies by nothing).  ValueError for a weight that is zero modulo
    t, and where B <= t n Q W + 1: W is past what the auxiliary base admits (RnsParam.max_dot_weight)."""
    if weights is None:
        w = None
    else:
        w = [centred(x, param.t) for x in weights]
        if len(w) != count:
            raise ValueError("dot: weights must be [len(xs)]")
        if any(x == 0 for x in w):
            raise ValueError("dot: a weight is zero modulo t; leave the pair out")
        if any(abs(x) >> 61 for x in w):
            raise ValueError("dot: a weight is not below 2^61 in absolute value")
    W = count if w is None else sum(abs(x) for x in w)
    if W > param.max_dot_weight:
        raise ValueError(f"dot: the sum of the absolute weights W = {W} is past the auxiliary base: B > t n Q W + 1 admits at most W = {param.max_dot_weight}")
    return (None if w is None or all(x == 1 for x in w) else w), W


def dot(xs, ys, rlk, weights=None):
    """-> sum_r weights[r] xs[r] ys[r] from fhe_bfv_rns_dot_dev: the integer tensors of all pairs are summed before
    the ONE division by Q and relinearised ONCE, so the call rounds once and adds one relinearisation noise term whatever
    len(xs) is.  xs, ys equal-length lists of RnsCiphertext of one RnsParam and batch; dot([x], [x], rlk) is the square.
    weights are Python integers, taken centred modulo t; None: ones."""
    xs, ys = list(xs), list(ys)
    if not xs or len(xs) != len(ys):
        raise ValueError("dot: xs and ys must be non-empty lists of one length")
    param, batch = xs[0].param, xs[0].batch
    if any(ct.param != param or ct.batch != batch for ct in xs + ys):
        raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "dot: operands differ in RnsParam or batch")
    if rlk.param != param:
        raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "dot: the relinearisation key is not of the operands' chain")
    w, _ = dot_weights(param, len(xs), weights)
    out = _torch().empty_like(xs[0].d)
    binding.bfv_rns_dot_dev(param.plans(), param.aux_plans(), param.special_plan(), param.t, rlk.d_rlk.data_ptr(), [ct.d.data_ptr() for ct in xs],
                            [ct.d.data_ptr() for ct in ys], w, out.data_ptr(), batch)
    return RnsCiphertext(param, out)


def lincomb_residues(param, weights, consts=None):
    """what `lincomb` hands fhe_ckks_rns_lincomb_dev -> (w, k): weights [outputs][count] Python integers, centred modulo t, as
    canonical residues [outputs][count][limbs] in a flat list; consts [outputs] (or None -> None) as floor(Q / t) c mod q_i, c
    centred modulo t, [outputs][limbs] in a flat list"""
    delta = param.Q // param.t
    w = [centred(x, param.t) % q for row in weights for x in row for q in param.moduli]
    k = None if consts is None else [delta * centred(c, param.t) % q for c in consts for q in param.moduli]
    return w, k


def lincomb(cts, weights, consts=None):
    """-> [sum_r weights[o][r] cts[r] + consts[o] for each output o] from fhe_ckks_rns_lincomb_dev: every input is read once for
    up to four outputs and nothing is transformed.  weights Python integers [outputs][count] (1-D: one output), taken centred
    modulo t and reduced per limb; consts integers [outputs] or None.  A constant c is added as floor(Q / t) c mod q_i to
    component 0, which is the encoding of the CONSTANT POLYNOMIAL c only: under the batch encoder that is c in every slot, and
    no other plaintext can be added this way (use add_plain).  The noise grows by the sum of the absolute weights."""
    cts = list(cts)
    if not cts:
        raise ValueError("lincomb: no input")
    weights = list(weights)
    if not weights:
        raise ValueError("lincomb: no weight")
    rows = [list(r) for r in weights] if hasattr(weights[0], "__len__") else [weights]
    if any(len(r) != len(cts) for r in rows):
        raise ValueError("lincomb: weights must be [outputs][len(cts)]")
    outputs = len(rows)
    consts = None if consts is None else list(np.asarray(consts, dtype=object).reshape(-1))
    if consts is not None and len(consts) != outputs:
        raise ValueError("lincomb: consts must be [outputs]")
    param, batch = cts[0].param, cts[0].batch
    if any(ct.param != param or ct.batch != batch for ct in cts):
        raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "lincomb: operands differ in RnsParam or batch")
    k = len(param.moduli)
    out = _torch().empty((outputs, k, 2, batch, param.n), dtype=_torch().int64, device="cuda")
    cap = binding.FHE_CKKS_LINCOMB_MAX_OUTPUTS
    for o0 in range(0, outputs, cap):
        o1 = min(outputs, o0 + cap)
        w, kk = lincomb_residues(param, rows[o0:o1], None if consts is None else consts[o0:o1])
        binding.ckks_rns_lincomb_dev(param.plans(), [ct.d.data_ptr() for ct in cts], w, kk, o1 - o0, out[o0].data_ptr(), batch)
    return [RnsCiphertext(param, out[o]) for o in range(outputs)]


def encode_diagonals(param, encoder, rows, steps):
    """rows [outputs][count][2][n/2] (or [count][2][n/2]: one output) slot values modulo t; column r multiplies the ciphertext
    rotated by steps[r].  BatchEncoder.encode, centred modulo t, then fhe_ckks_rns_from_i64_dev over the chain's plans and once
    more over the special prime's plan -> ckks.RnsPlaintextSet with d_pts [outputs][count][k + 1][n], what
    fhe_ckks_rns_diag_sum_dev and fhe_ckks_rns_bsgs_dev take"""
    torch = _torch()
    n, t, k = param.n, param.t, len(param.moduli)
    if encoder.n != n or encoder.t != t:
        raise ValueError("encode_diagonals: the encoder is not of this RnsParam's n and t")
    rows = np.asarray(rows, dtype=np.int64)
    if rows.ndim == 3:
        rows = rows[None]
    steps = [int(st) for st in steps]
    if rows.ndim != 4 or rows.shape[0] < 1 or rows.shape[1:] != (len(steps), 2, max(n // 2, 1)):
        raise ValueError("encode_diagonals: rows must be [outputs][len(steps)][2][n/2]")
    outputs, count = rows.shape[:2]
    coef = encoder.encode(rows.reshape(outputs * count, 2, max(n // 2, 1))).astype(np.int64)
    coef = np.where(coef > t // 2, coef - t, coef)
    d_rows = torch.from_numpy(np.ascontiguousarray(coef)).cuda()
    d_pts = torch.empty((outputs * count, k + 1, n), dtype=torch.int64, device="cuda")
    for plans, lo in ((param.plans(), 0), ([param.special_plan()], k)):
        ev = torch.empty((len(plans), outputs * count, n), dtype=torch.int64, device="cuda")
        binding.ckks_rns_from_i64_dev(plans, d_rows.data_ptr(), ev.data_ptr(), outputs * count)
        d_pts[:, lo:lo + len(plans)] = ev.permute(1, 0, 2)
    ck = _ckks()
    return ck.RnsPlaintextSet(param, k - 1, d_pts.reshape(outputs, count, k + 1, n), 1.0, [ck.galois_element(n, st) for st in steps])


def bsgs_diagonals(M, t, n1=None):
    """The baby-step giant-step form of out[r] = M[r] in[r] mod t on the two slot rows (N = n/2 columns): M integers [2][N][N],
    or [N][N] for both rows.  Diagonal d is diag_d[r][c] = M[r][c][(c + d) mod N]; a diagonal that is zero modulo t in both rows
    is dropped; d = n1 a + b.  -> (n1, baby, giant, rows): the sorted baby steps b and giant steps a that occur, and rows
    int64 [len(giant)][len(baby)][2][N] in [0, t) with rows[a][b] = roll(diag_{n1 giant[a] + baby[b]}, +n1 giant[a]) along the
    columns (zero where that diagonal is dropped), the giant step's plaintext pre-rotated as ckks.bsgs_diagonals does, so that
        M x = sum_a roll(sum_b rows[a][b] * roll(x, -baby[b]), -n1 giant[a])   (mod t, rolls along the columns).
    n1 defaults to the ceiling of the square root of the number of diagonals kept."""
    M = np.asarray(M)
    if M.ndim == 2:
        M = np.stack([M, M])
    if M.ndim != 3 or M.shape[0] != 2 or M.shape[1] != M.shape[2] or M.shape[1] < 1:
        raise ValueError("bsgs_diagonals: M must be [2][N][N] or [N][N]")
    M = np.mod(M.astype(object), int(t)).astype(np.int64)
    N = M.shape[1]
    c = np.arange(N)
    diag = {d: M[:, c, (c + d) % N] for d in range(N)}
    kept = [d for d in range(N) if np.any(diag[d] != 0)] or [0]
    if n1 is None:
        n1 = int(np.ceil(np.sqrt(len(kept))))
    n1 = int(n1)
    if not 1 <= n1 <= N:
        raise ValueError(f"bsgs_diagonals: n1={n1} must be in [1, {N}]")
    baby, giant = sorted({d % n1 for d in kept}), sorted({d // n1 for d in kept})
    rows = np.zeros((len(giant), len(baby), 2, N), dtype=np.int64)
    for d in kept:
        rows[giant.index(d // n1), baby.index(d % n1)] = np.roll(diag[d], n1 * (d // n1), axis=1)
    return n1, baby, giant, rows


class LinearTransform:
    """out[r] = M[r] in[r] mod t on the two slot rows, encoded for RnsCiphertext.linear_transform: one plaintext set whose
    outputs are the giant steps and whose columns the baby steps of bsgs_diagonals"""

    def __init__(self, param, n1, baby, giant, pts):
        self.param, self.n1, self.baby, self.giant, self.pts = param, n1, list(baby), list(giant), pts

    @classmethod
    def from_matrices(cls, param, encoder, M, n1=None):
        N = max(param.n // 2, 1)
        if np.asarray(M).shape not in ((2, N, N), (N, N)):
            raise ValueError(f"LinearTransform: M must be [2][{N}][{N}] or [{N}][{N}]")
        n1, baby, giant, rows = bsgs_diagonals(M, param.t, n1)
        return cls(param, n1, baby, giant, encode_diagonals(param, encoder, rows, baby))

    def required_steps(self):
        """the rotation steps whose keys linear_transform needs: the non-zero baby steps and n1 times the non-zero giant steps"""
        return sorted({i for i in self.baby if i} | {self.n1 * j for j in self.giant if j})


class RnsClientKey(ClientKeyBase):
    """The BFV secret under every prime of an RnsParam, on ClientKeyBase with the row plan of ckks.RnsClientKey:
        [0, 2^56)                    fresh encryptions
        1 2^56 + slot                public_key(slot)
        2 2^56 + 64 slot + j         digit j of relin_key(slot)
        3 2^56 + 64 slot + j         digit j of galois_key(g, slot)
    public_key, relin_key, galois_key and rotation_key go through the key builders of ckks.RnsClientKey, and the keys are the
    same objects (ckks.RnsPublicKey, ckks.RnsRelinKey, ckks.RnsGaloisKey).  row_swap_key is the key of g = 2n - 1."""

    RLK_BASE, GK_BASE = 2 << 56, 3 << 56

    def __init__(self, seed, param, d_s, d_s_evals, sigma):
        super().__init__(seed, sigma)
        self.param, self.d_s, self.d_s_evals = param, d_s, d_s_evals

    @classmethod
    def generate(cls, seed, param, sigma=3.2):
        torch = _torch()
        plans = param.plans() + [param.special_plan()]
        d_s = torch.empty((len(plans), param.n), dtype=torch.int64, device="cuda")
        d_e = torch.empty_like(d_s)
        for i, plan in enumerate(plans):
            binding.ckks_secret_key_dev(plan, seed, 0, d_s[i].data_ptr())
            plan.forward_dev(d_s[i].data_ptr(), d_e[i].data_ptr(), 1)
        torch.cuda.synchronize()
        return cls(seed, param, d_s, d_e, sigma)

    def public_key(self, slot=0):
        return _ckks().RnsClientKey.public_key(self, slot)

    def relin_key(self, slot=0):
        return _ckks().RnsClientKey.relin_key(self, slot)

    def galois_key(self, g, slot):
        return _ckks().RnsClientKey.galois_key(self, g, slot)

    def rotation_key(self, step, slot):
        """the key of g = 5^step mod 2n (ckks.galois_element): both rows of the slot matrix move left by `step`"""
        return self.galois_key(_ckks().galois_element(self.param.n, step), slot)

    def row_swap_key(self, slot):
        return self.galois_key(2 * self.param.n - 1, slot)

    def encode_diagonals(self, rows, steps):
        """the plaintext set of RnsCiphertext.diag_sum: encode_diagonals with the batch encoder of this key's n and t"""
        return encode_diagonals(self.param, BatchEncoder(self.param.n, self.param.t), rows, steps)

    def encrypt(self, pk, m):
        """m in [0, t)^n, (n,) or (batch, n) -> RnsCiphertext: floor(Q / t) m per limb (fhe_bfv_rns_scale_msg_dev), then
        fhe_ckks_encrypt_dev per limb on the same fresh rows"""
        torch = _torch()
        p, n = self.param, self.param.n
        msg = np.mod(np.ascontiguousarray(m, dtype=np.int64).reshape(-1, n), p.t)
        batch = msg.shape[0]
        plans = p.plans()
        d_m = torch.from_numpy(msg).cuda()
        dm = torch.empty((len(plans), batch, n), dtype=torch.int64, device="cuda")
        binding.bfv_rns_scale_msg_dev(plans, p.t, d_m.data_ptr(), dm.data_ptr(), batch)
        out = torch.empty((len(plans), 2, batch, n), dtype=torch.int64, device="cuda")

        def limbs(row):
            for i, plan in enumerate(plans):
                binding.ckks_encrypt_dev(plan, self.seed, row, pk.d_evals[i].data_ptr(), dm[i].data_ptr(), n, self._cdt_ptr(), self._m, out[i].data_ptr(), batch)
                plan.forward_dev(out[i].data_ptr(), out[i].data_ptr(), 2 * batch)

        self._on_fresh_rows(batch, limbs)
        return RnsCiphertext(p, out)

    def _own(self, ct):
        if ct.param != self.param:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the ciphertext is not in this key's chain")

    def decrypt(self, ct):
        """-> m [batch][n] in [0, t): floor((t v + floor(Q / 2)) / Q) mod t of the phase v (fhe_bfv_rns_decrypt_dev)"""
        torch = _torch()
        self._own(ct)
        p = self.param
        out = torch.empty((ct.batch, p.n), dtype=torch.int64, device="cuda")
        binding.bfv_rns_decrypt_dev(p.plans(), p.aux[0], p.t, self.d_s_evals.data_ptr(), ct.d.data_ptr(), out.data_ptr(), ct.batch)
        return out.cpu().numpy().view(np.uint64)

    def phase(self, ct):
        """the phase v = c0 + c1 s centred in Q, as Python integers [batch][n]: per limb on the device, the CRT on the host"""
        torch = _torch()
        self._own(ct)
        p = self.param
        v = torch.empty((len(p.moduli), ct.batch, p.n), dtype=torch.int64, device="cuda")
        w = torch.empty_like(v)
        L = binding.load_library()
        for i, plan in enumerate(p.plans()):
            for r in range(ct.batch):
                plan.pointwise_mul_dev(ct.d[i, 1, r].data_ptr(), self.d_s_evals[i].data_ptr(), v[i, r].data_ptr(), 1)
            binding._check(L.fhe_rq_add_dev(plan.handle, v[i].data_ptr(), ct.d[i, 0].data_ptr(), w[i].data_ptr(), ct.batch, None))
            plan.inverse_dev(w[i].data_ptr(), w[i].data_ptr(), ct.batch)
        res = w.cpu().numpy().view(np.uint64).astype(object)
        Q = p.Q
        x = np.zeros(res.shape[1:], dtype=object)
        for i, q in enumerate(p.moduli):
            x = x + res[i] * ((Q // q) * pow(Q // q, -1, q))
        x = x % Q
        return np.where(x > Q // 2, x - Q, x)

    def noise_budget(self, ct):
        """the bits of log2(Q / (2 |t v - Q m|_inf)) - 1, m the rounded quotient t v / Q: what is left before decryption fails;
        computed on the host in Python integers from the phase"""
        p = self.param
        Q, t = p.Q, p.t
        worst = 0
        for v in self.phase(ct).reshape(-1):
            v = int(v)
            worst = max(worst, abs(t * v - Q * ((t * v + Q // 2) // Q)))
        if worst == 0:
            return Q.bit_length() - 1
        return max((Q // (2 * worst)).bit_length() - 1, 0) - 1
