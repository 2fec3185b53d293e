"""Host mirror of the reference's CKKS surface (ckks/src/encoder.rs, ckks/src/lib.rs) over the C ABI, on the device
(DESIGN.md §21): the canonical embedding as a double-precision FFT, keys, encryption, decryption, and the additions.

    reference (Rust)                          here
    Param { ring, t }             lib.rs:20   Param(ring)                       (t only sizes the reference's test inputs)
    Encoder::new(n, scale)   encoder.rs:30    Encoder(n, delta)                 (holds the device twiddle table)
    Encoder::encode / decode encoder.rs:57    Encoder.encode(z) / .decode(p, scale=None)
    CKKS::new_key(rng)            lib.rs:46   ClientKey.generate(seed, param, delta), .public_key(slot)
    CKKS::encrypt / decrypt       lib.rs:66   ClientKey.encrypt(pk, m) / .decrypt(ct)
    encode_and_encrypt            lib.rs:96   ClientKey.encode_and_encrypt(pk, z)
    decrypt_and_decode            lib.rs:107  ClientKey.decrypt_and_decode(ct, scale=None)
    CKKS::add / sub               lib.rs:113  Ciphertext.__add__ / __sub__     (sub subtracts both components)
    -                                         mul_plain(ct, m): decode with scale = delta^2

Departures, all recorded in §21: the mask a is uniform modulo q (the reference draws it from the secret's distribution),
`sub` subtracts both components (lib.rs:117 adds the second), the errors are §17's discrete Gaussian, and the encoder
is an O(N log N) transform whose roundings are not MKL's.
"""
from dataclasses import dataclass

import numpy as np

from . import binding
from .arith import RingParam, plan_of as _plan
from .device import from_dev as _from_dev, to_dev as _to_dev, torch as _torch
from .rlwe_client import ClientKeyBase, PublicKey  # noqa: F401  (PublicKey: exported from here too)


@dataclass(frozen=True)
class Param:
    """lib.rs:20-23: the ciphertext ring"""
    ring: RingParam


class Encoder:
    """encoder.rs: slot i < n/2 of a polynomial is its value at exp(i pi (2i+1) / n).  Holds fhe_ckks_twiddles(n) on the device.
    n <= 2^13 runs the one-pass entry points as before; 2^14 <= n <= 2^16 the two-pass ones (fhe_ckks_embed_*)."""

    def __init__(self, n, delta):
        self.n, self.delta = int(n), float(delta)
        big = self.n > 1 << 13
        twiddles = binding.ckks_embed_twiddles if big else binding.ckks_twiddles
        self._encode_dev = binding.ckks_embed_encode_dev if big else binding.ckks_encode_dev
        self._decode_dev = binding.ckks_embed_decode_dev if big else binding.ckks_decode_dev
        self.d_tw = _torch().from_numpy(twiddles(self.n).view(np.float64)).cuda()

    def encode_dev(self, d_z, batch, z_stride=None):
        """device complex128 [batch][n/2] -> device int64 [batch][n]"""
        torch = _torch()
        out = torch.empty((batch, self.n), dtype=torch.int64, device="cuda")
        self._encode_dev(self.n, self.delta, self.d_tw.data_ptr(), d_z.data_ptr(), self.n // 2 if z_stride is None else z_stride, out.data_ptr(), batch)
        return out

    def encode(self, z):
        """complex slots (n/2,) or (batch, n/2) -> int64 coefficients of the same leading shape"""
        z = np.ascontiguousarray(z, dtype=np.complex128)
        rows = z.reshape(-1, self.n // 2)
        out = self.encode_dev(_torch().from_numpy(rows.view(np.float64)).cuda(), rows.shape[0])
        return out.cpu().numpy().reshape(z.shape[:-1] + (self.n,))

    def decode_dev(self, d_p, batch, scale=None):
        torch = _torch()
        out = torch.empty((batch, self.n // 2, 2), dtype=torch.float64, device="cuda")
        self._decode_dev(self.n, self.delta if scale is None else float(scale), self.d_tw.data_ptr(), d_p.data_ptr(), out.data_ptr(), batch)
        return out

    def decode(self, p, scale=None):
        """int64 coefficients (n,) or (batch, n) -> complex128 slots; scale: the divisor when it is not delta (delta^2 after mul_plain)"""
        p = np.ascontiguousarray(p, dtype=np.int64)
        rows = p.reshape(-1, self.n)
        out = self.decode_dev(_torch().from_numpy(rows).cuda(), rows.shape[0], scale)
        return out.cpu().numpy().view(np.complex128).reshape(p.shape[:-1] + (self.n // 2,))


class Ciphertext:
    """(c0, c1) mod q, u64 words of shape (n,) or (batch, n)"""

    def __init__(self, ring, c0, c1):
        self.ring, self.c0, self.c1 = ring, c0, c1

    def _rows(self, rhs, fn):
        if rhs.ring != self.ring or rhs.c0.shape != self.c0.shape:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "operands differ in RingParam or shape")
        a, b = _to_dev(np.stack([self.c0, self.c1])), _to_dev(np.stack([rhs.c0, rhs.c1]))
        c = _torch().empty_like(a)
        binding._check(fn(_plan(self.ring).handle, a.data_ptr(), b.data_ptr(), c.data_ptr(), a.numel() // self.ring.n, None))
        out = _from_dev(c)
        return Ciphertext(self.ring, out[0], out[1])

    def __add__(self, rhs):
        """lib.rs:113-115 with fhe_rq_add_dev"""
        return self._rows(rhs, binding.load_library().fhe_rq_add_dev)

    def __sub__(self, rhs):
        """(c0 - c0', c1 - c1') with fhe_rq_sub_dev: both components, unlike lib.rs:117"""
        return self._rows(rhs, binding.load_library().fhe_rq_sub_dev)


def mul_plain(ct, m):
    """both components times the encoded plaintext m (int64 coefficients, (n,) or the ciphertext's shape) through
    fhe_rq_mul_dev: the one multiplication a single modulus carries; decode the result with scale = delta^2"""
    ring = ct.ring
    plan = _plan(ring)
    mm = np.mod(np.broadcast_to(np.asarray(m, dtype=np.int64), ct.c0.shape), np.int64(ring.q)).astype(np.uint64)
    a, b = _to_dev(np.stack([ct.c0, ct.c1])), _to_dev(np.stack([mm, mm]))
    c = _torch().empty_like(a)
    plan.rq_mul_dev(a.data_ptr(), b.data_ptr(), c.data_ptr(), a.numel() // ring.n)
    out = _from_dev(c)
    return Ciphertext(ring, out[0], out[1])


class ClientKey(ClientKeyBase):
    """The CKKS secret, resident on the device with its evals, an Encoder, and what is made from them.  The
    32-byte seed is the whole secret; rows never repeat within a seed, as for bfv.ClientKey:
        [0, 2^56)          fresh encryptions, in the order of the encrypt calls
        1 2^56 + slot      public_key(slot)
    and a builder refuses a slot (0 <= slot < 2^16) it has used.  The secret is KEY row 0."""

    def __init__(self, seed, param, delta, d_s, d_s_evals, sigma):
        super().__init__(seed, sigma)
        self.param, self.d_s, self.d_s_evals = param, d_s, d_s_evals
        self.encoder = Encoder(param.ring.n, delta)

    @classmethod
    def generate(cls, seed, param, delta, sigma=3.2):
        torch = _torch()
        n, plan = param.ring.n, _plan(param.ring)
        d_s = torch.empty(n, dtype=torch.int64, device="cuda")
        d_e = torch.empty(n, dtype=torch.int64, device="cuda")
        binding.ckks_secret_key_dev(plan, seed, 0, d_s.data_ptr())
        plan.forward_dev(d_s.data_ptr(), d_e.data_ptr(), 1)
        torch.cuda.synchronize()
        return cls(seed, param, delta, d_s, d_e, sigma)

    def public_key(self, slot=0):
        """CKKS::new_key's pk = (-a s + e, a), lib.rs:61, with a uniform modulo q"""
        return self._public_key(binding.ckks_public_key_dev, self.param.ring, slot)

    def encrypt(self, pk, m):
        """CKKS::encrypt, lib.rs:66-85: m int64 coefficients (n,) or (batch, n) -> Ciphertext on fresh rows"""
        torch = _torch()
        ring = self.param.ring
        m = np.ascontiguousarray(m, dtype=np.int64)
        msg = m.reshape(-1, ring.n)
        batch = msg.shape[0]
        d_m = torch.from_numpy(msg).cuda()
        out = torch.empty((2, batch, ring.n), dtype=torch.int64, device="cuda")
        self._on_fresh_rows(batch, lambda row: binding.ckks_encrypt_dev(_plan(ring), self.seed, row, pk.d_evals.data_ptr(), d_m.data_ptr(), ring.n, self._cdt_ptr(),
                                                                         self._m, out.data_ptr(), batch))
        w = _from_dev(out)
        return Ciphertext(ring, w[0].reshape(m.shape), w[1].reshape(m.shape))

    def decrypt(self, ct):
        """CKKS::decrypt, lib.rs:87-94 -> int64 coefficients, centred"""
        torch = _torch()
        ring = self.param.ring
        if ct.ring != ring:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the ciphertext is not in this key's ring")
        shape = ct.c0.shape
        d_ct = _to_dev(np.stack([ct.c0.reshape(-1, ring.n), ct.c1.reshape(-1, ring.n)]))
        batch = d_ct.shape[1]
        out = torch.empty((batch, ring.n), dtype=torch.int64, device="cuda")
        binding.ckks_decrypt_dev(_plan(ring), self.d_s_evals.data_ptr(), d_ct.data_ptr(), out.data_ptr(), batch)
        return out.cpu().numpy().reshape(shape)

    def encode_and_encrypt(self, pk, z):
        return self.encrypt(pk, self.encoder.encode(z))

    def decrypt_and_decode(self, ct, scale=None):
        return self.encoder.decode(self.decrypt(ct), scale)


# ---- the RNS modulus chain: ct x ct, relinearisation, rescaling (ckks_eval.hip) ---------------------------------
@dataclass(frozen=True)
class RnsParam:
    """n, the chain primes q_0 .. q_L and the special prime P >= max q_i of the relinearisation key; level l = limbs 0 .. l"""
    n: int
    moduli: tuple
    special: int

    def __post_init__(self):
        object.__setattr__(self, "moduli", tuple(int(q) for q in self.moduli))
        object.__setattr__(self, "special", int(self.special))
        if not 1 <= len(self.moduli) <= 8:
            raise ValueError("RnsParam: the chain has 1 to 8 primes")
        if len(set(self.moduli + (self.special,))) != len(self.moduli) + 1:
            raise ValueError("RnsParam: the primes of the chain and the special prime must be distinct")
        if self.special < max(self.moduli):
            raise ValueError("RnsParam: the special prime must not be below a chain prime")

    @property
    def max_level(self):
        return len(self.moduli) - 1

    def plans(self, level=None):
        """the plans of limbs 0 .. level (default: all)"""
        k = len(self.moduli) if level is None else level + 1
        return [_plan(RingParam(q, self.n)) for q in self.moduli[:k]]

    def special_plan(self):
        return _plan(RingParam(self.special, self.n))

    def special_plans(self):
        return [self.special_plan()]


class RnsRelinKey:
    """rlk [j][i][2][n] evals on the device, j <= L, i in {0 .. L, P}"""

    def __init__(self, param, d_rlk):
        self.param, self.d_rlk = param, d_rlk


class RnsPublicKey:
    """per limb (pk0, pk1) mod q_i as evals [limbs][2][n] on the device"""

    def __init__(self, param, d_evals):
        self.param, self.d_evals = param, d_evals


SCALE_TOLERANCE = 2.0 ** -20


# ---- Galois automorphisms: slot rotations and conjugation ---------------------------------------------------------
def galois_element(n, step):
    """the Galois element of a rotation of the n/2 slots by `step` (in the rotation order): 5^(step mod n/2) mod 2n"""
    return pow(5, int(step) % max(n // 2, 1), 2 * n)


def conjugation_element(n):
    return 2 * n - 1


def rotation_order(n):
    """-> (index, conj): entry t of the rotation order is slot index[t] of the encoder's order, conjugated where conj[t]:
    u_t = 5^t mod 2n is the exponent of the root at which entry t evaluates, slot i sits at exponent 2i + 1, and an
    exponent u >= n is the conjugate of 2n - u"""
    u = np.array([pow(5, t, 2 * n) for t in range(n // 2)], dtype=np.int64)
    conj = u >= n
    return np.where(conj, (2 * n - u - 1) // 2, (u - 1) // 2), conj


def to_rotation_order(z):
    """slots [..][n/2] in the encoder's order -> the order in which rotation by `step` is np.roll(w, -step)"""
    z = np.asarray(z, dtype=np.complex128)
    idx, conj = rotation_order(2 * z.shape[-1])
    return np.where(conj, np.conj(z[..., idx]), z[..., idx])


def from_rotation_order(w):
    w = np.asarray(w, dtype=np.complex128)
    idx, conj = rotation_order(2 * w.shape[-1])
    z = np.empty_like(w)
    z[..., idx] = np.where(conj, np.conj(w), w)
    return z


class RnsGaloisKey:
    """gk_g [j][i][2][n] evals on the device, the shape of a relinearisation key, for the Galois element g"""

    def __init__(self, param, g, d_gk):
        g = int(g)
        if g % 2 == 0 or not 0 < g < 2 * param.n:
            raise ValueError(f"RnsGaloisKey: g={g} must be odd and in [1, 2n)")
        self.param, self.g, self.d_gk = param, g, d_gk

    @property
    def is_conjugation(self):
        return self.g == 2 * self.param.n - 1

    @property
    def is_rotation(self):
        """the powers of 5 modulo 2n are the g = 1 (mod 4)"""
        return self.g % 4 == 1


# ---- plaintext linear transforms: diagonal sums and baby-step giant-step -------------------------------------------
class RnsPlaintextSet:
    """The plaintexts of one diagonal sum, d_pts [outputs][count][level + 2][n] canonical evals on the device (the chain limbs
    0 .. level, then the special prime), their scale, and the Galois element gs[r] that column r multiplies"""

    _limbs_name = "level + 2"

    @staticmethod
    def _special_count(param):
        return 1

    def __init__(self, param, level, d_pts, scale, gs):
        gs = [int(g) for g in gs]
        for g in gs:
            if g % 2 == 0 or not 0 < g < 2 * param.n:
                raise ValueError(f"{type(self).__name__}: g={g} must be odd and in [1, 2n)")
        limbs = level + 1 + self._special_count(param)
        if d_pts is not None and (d_pts.dim() != 4 or d_pts.shape[1] != len(gs) or d_pts.shape[2] != limbs or d_pts.shape[3] != param.n):
            raise ValueError(f"{type(self).__name__}: d_pts is not [outputs][count][{self._limbs_name}][n]")
        self.param, self.level, self.d_pts, self.scale, self.gs = param, int(level), d_pts, float(scale), gs

    @property
    def outputs(self):
        return self.d_pts.shape[0]


class DeepPlaintextSet(RnsPlaintextSet):
    """RnsPlaintextSet on a DeepParam: d_pts [outputs][count][level + 1 + alpha][n], the chain limbs 0 .. level, then the special
    primes p_0 .. p_{alpha-1} in order"""

    _limbs_name = "level + 1 + alpha"

    @staticmethod
    def _special_count(param):
        return len(param.specials)


def encode_diagonals(param, encoder, rows, steps, level, scale):
    """rows complex [outputs][count][n/2] (or [count][n/2]: one output), slots in the rotation order; column r multiplies the
    ciphertext rotated by steps[r].  from_rotation_order and Encoder.encode at `scale`, then fhe_ckks_rns_from_i64_dev over the
    chain limbs 0 .. level and once more over the special prime -> RnsPlaintextSet.  Given a DeepParam: over the chain limbs and
    the special primes in slices of at most 8 plans -> DeepPlaintextSet"""
    torch = _torch()
    n = param.n
    rows = np.asarray(rows, dtype=np.complex128)
    if rows.ndim == 2:
        rows = rows[None]
    steps = [int(st) for st in steps]
    if rows.ndim != 3 or rows.shape[1] != len(steps) or rows.shape[2] != n // 2 or rows.shape[0] < 1:
        raise ValueError("encode_diagonals: rows must be [outputs][len(steps)][n/2]")
    if not 0 <= level <= param.max_level:
        raise ValueError(f"encode_diagonals: level {level} is not in [0, {param.max_level}]")
    outputs, count = rows.shape[:2]
    coef = encoder.encode(from_rotation_order(rows.reshape(outputs * count, n // 2)) * (float(scale) / encoder.delta))
    d_rows = torch.from_numpy(np.ascontiguousarray(coef)).cuda()
    if isinstance(param, DeepParam):
        every = param.plans(level) + param.special_plans()
        slices, kind = [(every[lo:lo + 8], lo) for lo in range(0, len(every), 8)], DeepPlaintextSet
    else:
        slices, kind = [(param.plans(level), 0), ([param.special_plan()], level + 1)], RnsPlaintextSet
    limbs = sum(len(plans) for plans, _ in slices)
    d_pts = torch.empty((outputs * count, limbs, n), dtype=torch.int64, device="cuda")
    for plans, lo in slices:
        ev = torch.empty((len(plans), outputs * count, n), dtype=torch.int64, device="cuda")
        binding.ckks_rns_from_i64_dev(plans, d_rows.data_ptr(), ev.data_ptr(), outputs * count)
        d_pts[:, lo:lo + len(plans)] = ev.permute(1, 0, 2)
    return kind(param, level, d_pts.reshape(outputs, count, limbs, n), scale, [galois_element(n, st) for st in steps])


def bsgs_diagonals(M, n1=None):
    """The baby-step giant-step form of w' = M w for a square complex matrix on the rotation order (N = n/2 slots).  Diagonal t
    is d_t[s] = M[s][(s + t) mod N]; only non-zero diagonals are kept; t = n1 j + i.  -> (n1, baby, giant, rows): the sorted
    baby steps i and giant steps j that occur, and rows [len(giant)][len(baby)][N] with rows[a][b] = roll(d_{n1 giant[a] + baby[b]},
    +n1 giant[a]) (zero where that diagonal is), so that
        M w = sum_a roll(sum_b rows[a][b] * roll(w, -baby[b]), -n1 giant[a]).
    n1 defaults to the ceiling of the square root of the number of diagonals kept."""
    M = np.asarray(M, dtype=np.complex128)
    N = M.shape[0]
    if M.ndim != 2 or M.shape[1] != N or N < 1:
        raise ValueError("bsgs_diagonals: M must be square")
    s = np.arange(N)
    diag = {t: M[s, (s + t) % N] for t in range(N)}
    kept = [t for t in range(N) if np.any(diag[t] != 0)] or [0]
    if n1 is None:
        n1 = int(np.ceil(np.sqrt(len(kept))))
    n1 = int(n1)
    if not 1 <= n1 <= N:
        raise ValueError(f"bsgs_diagonals: n1={n1} must be in [1, {N}]")
    baby, giant = sorted({t % n1 for t in kept}), sorted({t // n1 for t in kept})
    rows = np.zeros((len(giant), len(baby), N), dtype=np.complex128)
    for t in kept:
        rows[giant.index(t // n1), baby.index(t % n1)] = np.roll(diag[t], n1 * (t // n1))
    return n1, baby, giant, rows


class LinearTransform:
    """w' = M w on the rotation order, encoded for RnsCiphertext.linear_transform: one RnsPlaintextSet whose outputs are the
    giant steps and whose columns the baby steps of bsgs_diagonals"""

    def __init__(self, param, n1, baby, giant, pts):
        self.param, self.n1, self.baby, self.giant, self.pts = param, n1, list(baby), list(giant), pts

    @classmethod
    def from_matrix(cls, param, encoder, M, level, scale, n1=None):
        M = np.asarray(M, dtype=np.complex128)
        if M.shape != (param.n // 2, param.n // 2):
            raise ValueError(f"LinearTransform: M must be {param.n // 2} x {param.n // 2}")
        n1, baby, giant, rows = bsgs_diagonals(M, n1)
        return cls(param, n1, baby, giant, encode_diagonals(param, encoder, rows, baby, level, scale))

    @property
    def level(self):
        return self.pts.level

    @property
    def scale(self):
        return self.pts.scale

    def required_steps(self):
        """the rotation steps whose keys linear_transform needs: the non-zero baby steps and n1 times the non-zero giant steps"""
        return sorted({i for i in self.baby if i} | {self.n1 * j for j in self.giant if j})


class RnsCiphertext:
    """A device tensor [level + 1][2][batch][n] of evals with its level and float64 scale"""

    def __init__(self, param, d, level, scale):
        self.param, self.d, self.level, self.scale = param, d, int(level), float(scale)

    @property
    def batch(self):
        return self.d.shape[2]

    def at_level(self, level):
        """dropping top limbs is truncation"""
        if not 0 <= level <= self.level:
            raise ValueError(f"at_level: level {level} is not in [0, {self.level}]")
        return type(self)(self.param, self.d[:level + 1].contiguous(), level, self.scale)

    def _pair(self, rhs):
        if rhs.param != self.param or rhs.batch != self.batch:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "operands differ in RnsParam or batch")
        level = min(self.level, rhs.level)
        return self.at_level(level), rhs.at_level(level), level

    def _rows(self, rhs, fn):
        if abs(rhs.scale - self.scale) > SCALE_TOLERANCE * self.scale:
            raise ValueError(f"the scales {self.scale} and {rhs.scale} differ by more than a relative 2^-20")
        a, b, level = self._pair(rhs)
        out = _torch().empty_like(a.d)
        for i, plan in enumerate(self.param.plans(level)):
            binding._check(fn(plan.handle, a.d[i].data_ptr(), b.d[i].data_ptr(), out[i].data_ptr(), 2 * self.batch, None))
        return type(self)(self.param, out, level, self.scale)

    def __add__(self, rhs):
        return self._rows(rhs, binding.load_library().fhe_rq_add_dev)

    def __sub__(self, rhs):
        return self._rows(rhs, binding.load_library().fhe_rq_sub_dev)

    def mul(self, rhs, rlk):
        """ct x ct and relinearisation (fhe_ckks_rns_mul_dev); the scale multiplies and the result is NOT rescaled"""
        if rlk.param != self.param:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the relinearisation key is not of this ciphertext's chain")
        a, b, level = self._pair(rhs)
        out = _torch().empty_like(a.d)
        binding.ckks_rns_mul_dev(self.param.plans(level), self.param.special_plan(), rlk.d_rlk.data_ptr(), len(self.param.moduli), a.d.data_ptr(), b.d.data_ptr(),
                                 out.data_ptr(), self.batch)
        return RnsCiphertext(self.param, out, level, self.scale * rhs.scale)

    def rescale(self):
        """divide and round by the top prime: level - 1, scale / q_level; refused at level 0"""
        if self.level == 0:
            raise binding.FheError(binding.FHE_E_INVALID, "rescale: a ciphertext at level 0 cannot be rescaled")
        torch = _torch()
        out = torch.empty((self.level, 2, self.batch, self.param.n), dtype=torch.int64, device="cuda")
        binding.ckks_rns_rescale_dev(self.param.plans(self.level), self.d.data_ptr(), out.data_ptr(), self.batch)
        return RnsCiphertext(self.param, out, self.level - 1, self.scale / self.param.moduli[self.level])

    def rotate_many(self, gks):
        """sigma_g of this ciphertext for every key of `gks` from one call (fhe_ckks_rns_galois_dev): the digit decomposition
        of c1 is shared.  Level and scale are unchanged."""
        torch = _torch()
        gks = list(gks)
        if any(gk.param != self.param for gk in gks):
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "a Galois key is not of this ciphertext's chain")
        out = torch.empty((len(gks),) + tuple(self.d.shape), dtype=torch.int64, device="cuda")
        binding.ckks_rns_galois_dev(self.param.plans(self.level), self.param.special_plan(), [gk.d_gk.data_ptr() for gk in gks], [gk.g for gk in gks],
                                    len(self.param.moduli), self.d.data_ptr(), out.data_ptr(), self.batch)
        return [RnsCiphertext(self.param, out[r], self.level, self.scale) for r in range(len(gks))]

    def apply_galois(self, gk):
        """sigma_g with the key's g: (pi_g(c0) + r0, r1), (r0, r1) the key switch of pi_g(c1)"""
        return self.rotate_many([gk])[0]

    def rotate(self, gk):
        """the slots, in the rotation order, moved by the key's step; a key that is no rotation key is refused"""
        if not gk.is_rotation:
            raise ValueError(f"rotate: g={gk.g} is no power of 5 modulo 2n")
        return self.apply_galois(gk)

    def conjugate(self, gk):
        """every slot conjugated; a key of another element is refused"""
        if not gk.is_conjugation:
            raise ValueError(f"conjugate: g={gk.g} is not 2n - 1")
        return self.apply_galois(gk)

    def diag_sum(self, pts, gks):
        """-> [sum_r m_{o,r} (.) sigma_{g_r}(self) for each output o] from one call (fhe_ckks_rns_diag_sum_dev): one digit
        decomposition for all elements and outputs, one division by P an output.  gks[r] is the key of pts.gs[r]; where
        pts.gs[r] = 1 it is not read and may be None.  Level unchanged; the scale multiplies; the caller rescales."""
        torch = _torch()
        key_ptrs = self._diag_keys(pts, gks)
        out = torch.empty((pts.outputs,) + tuple(self.d.shape), dtype=torch.int64, device="cuda")
        binding.ckks_rns_diag_sum_dev(self.param.plans(self.level), self.param.special_plan(), key_ptrs, pts.gs, len(self.param.moduli),
                                      pts.d_pts.data_ptr(), pts.outputs, self.d.data_ptr(), out.data_ptr(), self.batch)
        return [RnsCiphertext(self.param, out[o], self.level, self.scale * pts.scale) for o in range(pts.outputs)]

    def _diag_keys(self, pts, gks):
        """diag_sum's argument checks -> the device pointer of every element's key, None where the element is 1"""
        gks = list(gks)
        if pts.param != self.param or any(gk is not None and gk.param != self.param for gk in gks):
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the plaintexts or a Galois key are not of this ciphertext's chain")
        if pts.level != self.level:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, f"the plaintexts are at level {pts.level}, the ciphertext at {self.level}")
        if len(gks) != len(pts.gs):
            raise ValueError(f"diag_sum: {len(gks)} keys for {len(pts.gs)} elements")
        for r, (g, gk) in enumerate(zip(pts.gs, gks)):
            if g != 1 and gk is None:
                raise ValueError(f"diag_sum: element {r} (g={g}) has no key")
            if g != 1 and gk.g != g:
                raise ValueError(f"diag_sum: key {r} is of g={gk.g}, the plaintexts' element is {g}")
        return [None if g == 1 else gk.d_gk.data_ptr() for g, gk in zip(pts.gs, gks)]

    def linear_transform(self, lt, keys):
        """M w for a LinearTransform: one diag_sum whose outputs are the giant steps' inner sums, then rotate by n1 j and add
        for j > 0.  keys: step -> RnsGaloisKey for every step of lt.required_steps(); a missing one raises KeyError(step)."""
        missing = [st for st in lt.required_steps() if st not in keys]
        if missing:
            raise KeyError(missing[0])
        inner = self.diag_sum(lt.pts, [keys[i] if i else None for i in lt.baby])
        acc = None
        for j, part in zip(lt.giant, inner):
            part = part.rotate(keys[lt.n1 * j]) if j else part
            acc = part if acc is None else acc + part
        return acc

    def linear_transform_hoisted(self, lt, keys):
        """M w for a LinearTransform from one call (fhe_ckks_rns_bsgs_dev): the inner sums stay in the basis Q P,
        a giant step divides only its second component by P before its key switch, and one modulus-down finishes the sum.
        keys as for linear_transform: step -> RnsGaloisKey for every step of lt.required_steps(), a missing one raises
        KeyError(step).  Level unchanged; the scale multiplies; the caller rescales.  The words differ from linear_transform's
        by its roundings; both are within their noise bounds of the product."""
        missing = [st for st in lt.required_steps() if st not in keys]
        if missing:
            raise KeyError(missing[0])
        torch = _torch()
        pts, n = lt.pts, self.param.n
        baby = [keys[i] if i else None for i in lt.baby]
        giant = [keys[lt.n1 * j] if j else None for j in lt.giant]
        giant_gs = [galois_element(n, lt.n1 * j) for j in lt.giant]
        if pts.param != self.param or any(gk is not None and gk.param != self.param for gk in baby + giant):
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the plaintexts or a Galois key are not of this ciphertext's chain")
        if pts.level != self.level:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, f"the plaintexts are at level {pts.level}, the ciphertext at {self.level}")
        for g, gk in zip(pts.gs + giant_gs, baby + giant):
            if g != 1 and gk.g != g:
                raise ValueError(f"linear_transform_hoisted: a key is of g={gk.g}, its step's element is {g}")
        out = torch.empty_like(self.d)
        binding.ckks_rns_bsgs_dev(self.param.plans(self.level), self.param.special_plan(), [None if gk is None else gk.d_gk.data_ptr() for gk in baby], pts.gs,
                                  [None if gk is None else gk.d_gk.data_ptr() for gk in giant], giant_gs, len(self.param.moduli), pts.d_pts.data_ptr(),
                                  self.d.data_ptr(), out.data_ptr(), self.batch)
        return RnsCiphertext(self.param, out, self.level, self.scale * pts.scale)

    def _plain(self, m):
        """signed rows (n,) or (batch, n) -> evals [level + 1][batch][n]"""
        torch = _torch()
        n = self.param.n
        rows = np.array(np.broadcast_to(np.asarray(m, dtype=np.int64), (self.batch, n)))   # a writable copy
        out = torch.empty((self.level + 1, self.batch, n), dtype=torch.int64, device="cuda")
        d_rows = torch.from_numpy(rows).cuda()
        binding.ckks_rns_from_i64_dev(self.param.plans(self.level), d_rows.data_ptr(), out.data_ptr(), self.batch)
        return out

    def add_plain(self, m):
        """c0 + m for an encoded plaintext at this ciphertext's scale"""
        pt, out = self._plain(m), self.d.clone()
        for i, plan in enumerate(self.param.plans(self.level)):
            binding._check(binding.load_library().fhe_rq_add_dev(plan.handle, self.d[i, 0].data_ptr(), pt[i].data_ptr(), out[i, 0].data_ptr(), self.batch, None))
        return type(self)(self.param, out, self.level, self.scale)

    def mul_plain(self, m, scale):
        """both components times an encoded plaintext of scale `scale`; the scale multiplies"""
        pt, out = self._plain(m), _torch().empty_like(self.d)
        for i, plan in enumerate(self.param.plans(self.level)):
            for c in range(2):
                plan.pointwise_mul_dev(self.d[i, c].data_ptr(), pt[i].data_ptr(), out[i, c].data_ptr(), self.batch)
        return type(self)(self.param, out, self.level, self.scale * float(scale))

    # ---- polynomial evaluation ----
    def mul_const(self, c, scale=None):
        """c times this ciphertext for a public real c, as lincomb([self], [c], scale=scale): with scale=None the weight is
        round(c), so pass the target scale (scale * q_level, then rescale()) for a c that is no integer"""
        return lincomb([self], [c], scale=scale)[0]

    def add_const(self, c):
        """this ciphertext plus the public real c in every slot: round(c * scale) added to component 0, level and scale unchanged"""
        return lincomb([self], [1], consts=[c])[0]

    def __neg__(self):
        return lincomb([self], [-1])[0]

    def eval_chebyshev(self, plan_or_coeffs, rlk, interval=(-1, 1)):
        """sum_i coeffs[i] T_i(y) of every slot x, y = (2x - a - b)/(b - a): a ChebyshevPlan, or Chebyshev coefficients from which
        one is built.  Consumes plan.levels levels; the result has this ciphertext's scale (up to float rounding).  A
        ciphertext with fewer levels is refused before anything runs."""
        return eval_chebyshev(self, plan_or_coeffs, rlk, interval)


def _real(x, what):
    if np.iscomplexobj(np.asarray(x)):
        raise ValueError(f"lincomb: {what} must be real: a complex constant is no constant polynomial (i is X^(n/2) in the ring, not a scalar)")
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        raise ValueError(f"lincomb: {what} must be finite")
    return x


def lincomb(cts, coeffs, consts=None, scale=None, level=None):
    """-> [sum_r coeffs[o][r] cts[r] + consts[o] for each output o] from fhe_ckks_rns_lincomb_dev, or from
    fhe_ckks_deep_lincomb_dev where the operands are DeepCiphertexts, which then the outputs are too: every input
    is read once for up to four outputs, nothing is transformed and no level is used.  coeffs real [outputs][count] (1-D: one output), consts
    real [outputs] or None.  The level is the minimum over the inputs (or `level`, not above it: dropping limbs is truncation).
    scale is the target scale S of every output (or one per output, [outputs]): input r takes the integer weight round(coeffs[o][r] S / cts[r].scale), reduced
    per limb, and the constant is round(consts[o] S).  scale=None: S is the largest input scale, so an input at that scale takes
    round(coeff): integers are exact and anything else is the caller's business, who passes S = s q_level and rescales (one
    level) for real coefficients.  lincomb([P, T], [2, -1], scale=P.scale) on an unrescaled product P costs no level."""
    cts = list(cts)
    if not cts:
        raise ValueError("lincomb: no input")
    a = _real(coeffs, "a coefficient")
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] != len(cts) or a.shape[0] < 1:
        raise ValueError("lincomb: coeffs must be [outputs][len(cts)]")
    outputs = a.shape[0]
    k = None if consts is None else _real(consts, "a constant").reshape(-1)
    if k is not None and k.shape[0] != outputs:
        raise ValueError("lincomb: consts must be [outputs]")
    param, batch = cts[0].param, cts[0].batch
    if any(ct.param != param or ct.batch != batch for ct in cts):
        raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "lincomb: operands differ in RnsParam or batch")
    top = min(ct.level for ct in cts)
    level = top if level is None else int(level)
    if not 0 <= level <= top:
        raise ValueError(f"lincomb: level {level} is not in [0, {top}]")
    S = np.broadcast_to(np.asarray(max(ct.scale for ct in cts) if scale is None else scale, dtype=np.float64), (outputs,)).tolist()
    if not all(np.isfinite(x) and x > 0 for x in S):
        raise ValueError("lincomb: the target scale must be positive and finite")
    mods = param.moduli[:level + 1]
    w = [[round(float(a[o, r]) * S[o] / ct.scale) for r, ct in enumerate(cts)] for o in range(outputs)]
    kk = None if k is None else [round(float(c) * S[o]) for o, c in enumerate(k)]
    torch = _torch()
    out = torch.empty((outputs, level + 1, 2, batch, param.n), dtype=torch.int64, device="cuda")
    cap = binding.FHE_CKKS_LINCOMB_MAX_OUTPUTS
    deep = isinstance(param, DeepParam)
    call = binding.ckks_deep_lincomb_dev if deep else binding.ckks_rns_lincomb_dev
    for o0 in range(0, outputs, cap):
        o1 = min(outputs, o0 + cap)
        call(param.plans(level), [ct.d.data_ptr() for ct in cts], [x % q for row in w[o0:o1] for x in row for q in mods],
             None if kk is None else [x % q for x in kk[o0:o1] for q in mods], o1 - o0, out[o0].data_ptr(), batch)
    return [(DeepCiphertext if deep else RnsCiphertext)(param, out[o], level, S[o]) for o in range(outputs)]


def dot_weights(scales, coeffs=None, scale=None):
    """the scale rule of `dot` -> (S, w): pair r of scale scales[r] takes the integer w[r] = round(coeffs[r] S / scales[r]) (the
    float64 product, then the quotient, then Python's round: lincomb's rule), S = `scale`, or the largest pair scale where that
    is None; coeffs real [count], None: ones.  w is None where every weight is 1: the kernel then multiplies by nothing."""
    count = len(scales)
    a = _real(np.ones(count) if coeffs is None else coeffs, "a coefficient")
    if a.ndim != 1 or a.shape[0] != count:
        raise ValueError("dot: coeffs must be [len(xs)]")
    S = float(max(scales) if scale is None else scale)
    if not (np.isfinite(S) and S > 0):
        raise ValueError("dot: the target scale must be positive and finite")
    w = [round(float(a[r]) * S / scales[r]) for r in range(count)]
    return S, None if all(x == 1 for x in w) else w


def dot(xs, ys, rlk, coeffs=None, scale=None, level=None):
    """-> sum_r coeffs[r] xs[r] ys[r] from fhe_ckks_rns_dot_dev, or from fhe_ckks_deep_dot_dev (§39) where the
    operands are DeepCiphertexts, which then the result is too: the tensors of all pairs are summed on the device
    and relinearised ONCE, so the call costs one key switch and one relinearisation noise term whatever len(xs) is.  xs, ys
    equal-length lists of RnsCiphertext of one RnsParam and batch; dot([x], [x], rlk) is the square.  The level is the minimum
    over all operands (or `level`, not above it); an operand at a higher level is read as it is.  Pair r has scale s_r =
    xs[r].scale ys[r].scale and takes the weight of dot_weights, reduced per limb.  The result carries the target scale S and is
    NOT rescaled, like mul."""
    xs, ys = list(xs), list(ys)
    if not xs or len(xs) != len(ys):
        raise ValueError("dot: xs and ys must be non-empty lists of one length")
    param, batch = xs[0].param, xs[0].batch
    if any(ct.param != param or ct.batch != batch for ct in xs + ys):
        raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "dot: operands differ in RnsParam or batch")
    if rlk.param != param:
        raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "dot: the relinearisation key is not of the operands' chain")
    top = min(ct.level for ct in xs + ys)
    level = top if level is None else int(level)
    if not 0 <= level <= top:
        raise ValueError(f"dot: level {level} is not in [0, {top}]")
    S, w = dot_weights([x.scale * y.scale for x, y in zip(xs, ys)], coeffs, scale)
    torch = _torch()
    out = torch.empty((level + 1, 2, batch, param.n), dtype=torch.int64, device="cuda")
    deep = isinstance(param, DeepParam)
    ws = None if w is None else [x % q for x in w for q in param.moduli[:level + 1]]
    if deep:
        binding.ckks_deep_dot_dev(param.plans(level), param.special_plans(), rlk.d_rlk.data_ptr(), len(param.moduli), [ct.d.data_ptr() for ct in xs],
                                  [ct.d.data_ptr() for ct in ys], ws, out.data_ptr(), batch)
    else:
        binding.ckks_rns_dot_dev(param.plans(level), param.special_plan(), rlk.d_rlk.data_ptr(), len(param.moduli), [ct.d.data_ptr() for ct in xs],
                                 [ct.d.data_ptr() for ct in ys], ws, out.data_ptr(), batch)
    return (DeepCiphertext if deep else RnsCiphertext)(param, out, level, S)


def chebyshev_fit(f, degree, interval=(-1, 1)):
    """the Chebyshev coefficients c_0 .. c_degree of the interpolant of f at the degree + 1 Chebyshev nodes of `interval`:
    f(x) ~ sum_i c_i T_i((2x - a - b)/(b - a))"""
    a, b = float(interval[0]), float(interval[1])
    N = int(degree) + 1
    t = np.cos(np.pi * (np.arange(N) + 0.5) / N)
    fx = np.asarray(f((b - a) / 2 * t + (a + b) / 2), dtype=np.float64)
    c = np.array([2.0 / N * np.sum(fx * np.cos(np.pi * i * (np.arange(N) + 0.5) / N)) for i in range(N)])
    c[0] /= 2
    return c


class ChebyshevPlan:
    """sum_i coeffs[i] T_i(y), y = (2x - a - b)/(b - a), as a straight-line program: Paterson-Stockmeyer in the
    Chebyshev basis.  d = deg, m = ceil(log2(d + 1)), n1 = 2^ceil(m/2); babies T_1 .. T_(n1-1), giants T_(n1 2^t) <= d, all from
    T_(a+b) = 2 T_a T_b - T_(a-b); p = q T_g + r (chebdiv) with g the largest giant <= deg p; a leaf is a lincomb over the babies.

    ops, in order, each writing the wires `out`:
        ("lincomb", out [ids], inputs [ids], coeffs [outputs][count], consts [outputs] or None, scales [outputs], drop)
        ("mul", out, a, b)      ("rescale", out, a)
    wire 0 is the input.  A wire has a drop (levels below the input's) and a symbolic scale (p, e): s^p prod_j q_(l-j)^e[j], s and l
    the input's scale and level; scale_value() evaluates it.  A lincomb's `scales` are its outputs' targets as such pairs, `drop`
    its level.  All leaves of one level are the outputs of one lincomb: the babies are read once for them.
    Every sum of two wires is one lincomb whose target is the symbolic scale of the unrescaled product in it, and the targets
    are handed down the tree so that q T_g lands on r's scale: the weights of such a sum are 1 (or 2 and s_a s_b / s_c)."""

    def __init__(self, coeffs, interval, ops, drop, scale, result, levels, products, n1, babies, giants):
        self.coeffs, self.interval, self.ops, self.drop, self.scale, self.result = coeffs, interval, ops, drop, scale, result
        self.levels, self.products, self.n1, self.babies, self.giants = levels, products, n1, babies, giants

    @staticmethod
    def scale_value(sym, s, mods, level):
        """s^p prod_j q_(level-j)^e[j] in float64, the factors taken in this order"""
        p, e = sym
        v = 1.0
        for _ in range(abs(p)):
            v = v * s if p > 0 else v / s
        for j, x in enumerate(e):
            for _ in range(abs(x)):
                v = v * mods[level - j] if x > 0 else v / mods[level - j]
        return v

    @classmethod
    def build(cls, coeffs, interval=(-1, 1)):
        from numpy.polynomial import chebyshev as Ch

        c = np.trim_zeros(_real(coeffs, "a Chebyshev coefficient").reshape(-1), "b")
        lo, hi = float(interval[0]), float(interval[1])
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError("ChebyshevPlan: the interval must be finite with a < b")
        if len(c) < 2:
            raise ValueError("ChebyshevPlan: the degree must be at least 1")
        d = len(c) - 1
        m = int(d).bit_length()                                   # ceil(log2(d + 1))
        n1 = 1 << ((m + 1) // 2)
        if n1 - 1 > binding.FHE_CKKS_LINCOMB_MAX_COUNT:
            raise ValueError(f"ChebyshevPlan: degree {d} needs {n1 - 1} baby steps, more than one lincomb takes")
        ops, drop, scale = [], {0: 0}, {0: (1, ())}

        def new(dr, sc):
            w = len(drop)
            drop[w], scale[w] = dr, sc
            return w

        def smul(x, y):
            n = max(len(x[1]), len(y[1]))
            return (x[0] + y[0], tuple((x[1] + (0,) * n)[j] + (y[1] + (0,) * n)[j] for j in range(n)))

        def sq(j, e=1):                                           # q_(l-j)^e
            return (0, (0,) * j + (e,))

        def sinv(x):
            return (-x[0], tuple(-v for v in x[1]))

        def norm(x):
            e = list(x[1])
            while e and e[-1] == 0:
                e.pop()
            return (x[0], tuple(e))

        def lin(inputs, co, consts, scs, dr):
            scs = [norm(sc) for sc in (scs if isinstance(scs, list) else [scs])]
            outs = [new(dr, sc) for sc in scs]
            ops.append(("lincomb", outs, list(inputs), [list(map(float, row)) for row in co], None if consts is None else list(map(float, consts)), scs, dr))
            return outs

        def mul(a, b):
            w = new(max(drop[a], drop[b]), norm(smul(scale[a], scale[b])))
            ops.append(("mul", w, a, b))
            return w

        def rescale(a):
            w = new(drop[a] + 1, norm(smul(scale[a], sq(drop[a], -1))))
            ops.append(("rescale", w, a))
            return w

        T = {1: 0}
        if (lo, hi) != (-1.0, 1.0):                               # y = (2x - a - b)/(b - a): one lincomb, one rescale
            T[1] = rescale(lin([0], [[2.0 / (hi - lo)]], [-(lo + hi) / (hi - lo)], smul(scale[0], sq(0)), 0)[0])

        def cheb(i):                                              # T_i = 2 T_a T_b - T_(a-b), a = ceil(i/2), b = floor(i/2)
            if i not in T:
                a, b = (i + 1) // 2, i // 2
                P = mul(cheb(a), cheb(b))
                if a == b:
                    T[i] = rescale(lin([P], [[2.0]], [-1.0], scale[P], drop[P])[0])
                else:
                    T[i] = rescale(lin([P, cheb(1)], [[2.0, -1.0]], None, scale[P], drop[P])[0])
            return T[i]

        babies = list(range(1, n1))
        giants = [n1 << t for t in range(m) if (n1 << t) <= d]
        for i in babies + giants:
            cheb(i)

        # the tree: a node is (poly, drop D of its unrescaled value); need(p) is the least D
        def split(p):
            g = max(x for x in giants if x <= len(p) - 1)
            q, r = Ch.chebdiv(p, [0.0] * g + [1.0])
            return g, np.atleast_1d(q), np.atleast_1d(r)

        def need(p):
            if len(p) - 1 < n1:
                return drop[T[max(len(p) - 1, 1)]]
            g, q, r = split(p)
            return max(need(q) + 1, drop[T[g]], need(r))

        leaves = {}                                               # drop -> [(poly, target, holder)]

        def plant(p, D, S):
            """-> a thunk that emits the ops of the unrescaled value of p at drop D with scale S and returns its wire"""
            if len(p) - 1 < n1:
                holder = {}
                leaves.setdefault(D, []).append((p, S, holder))
                return lambda: holder["wire"]
            g, q, r = split(p)
            Sq = smul(smul(S, sinv(scale[T[g]])), sq(D - 1))      # so that rescale(q) T_g has scale S
            tq, tr = plant(q, D - 1, Sq), plant(r, D, S)

            def emit():
                P = mul(rescale(tq()), T[g])
                return lin([P, tr()], [[1.0, 1.0]], None, S, D)[0]
            return emit

        D = need(c)
        top = plant(c, D, smul(scale[0], sq(D)))                  # the result has the input's scale
        cap = binding.FHE_CKKS_LINCOMB_MAX_OUTPUTS
        for dr in sorted(leaves):                                 # all leaves of one level: one multi-output lincomb, each its own target
            ins = [i for i in babies if drop[T[i]] <= dr] or [1]
            for g0 in range(0, len(leaves[dr]), cap):
                group = leaves[dr][g0:g0 + cap]
                co = [[float(p[i]) if i < len(p) else 0.0 for i in ins] for p, _, _ in group]
                for (_, _, holder), w in zip(group, lin([T[i] for i in ins], co, [float(p[0]) for p, _, _ in group], [sc for _, sc, _ in group], dr)):
                    holder["wire"] = w
        result = rescale(top())
        products = sum(1 for op in ops if op[0] == "mul")
        return cls(c, (lo, hi), ops, drop, scale, result, drop[result], products, n1, babies, giants)

    def simulate(self, x):
        """the program on plain floats: every wire is its slot value, lincomb is the real sum (the scales do not enter)"""
        v = {0: np.asarray(x, dtype=np.float64)}
        for op in self.ops:
            if op[0] == "lincomb":
                _, outs, ins, co, consts, _, _ = op
                for o, w in enumerate(outs):
                    v[w] = sum(co[o][r] * v[i] for r, i in enumerate(ins)) + (0.0 if consts is None else consts[o])
            elif op[0] == "mul":
                v[op[1]] = v[op[2]] * v[op[3]]
            else:
                v[op[1]] = v[op[2]]
        return v[self.result]

    def run(self, ct, rlk):
        if ct.level < self.levels:
            raise ValueError(f"eval_chebyshev: the plan needs {self.levels} levels, the ciphertext has {ct.level}")
        mods = ct.param.moduli
        w = {0: ct}
        for op in self.ops:
            if op[0] == "lincomb":
                _, outs, ins, co, consts, sc, dr = op
                res = lincomb([w[i] for i in ins], co, consts, scale=[self.scale_value(x, ct.scale, mods, ct.level) for x in sc], level=ct.level - dr)
                w.update(zip(outs, res))
            elif op[0] == "mul":
                w[op[1]] = w[op[2]].mul(w[op[3]], rlk)
            else:
                w[op[1]] = w[op[2]].rescale()
        return w[self.result]


def eval_chebyshev(ct, plan_or_coeffs, rlk, interval=(-1, 1)):
    """sum_i coeffs[i] T_i(y) of every slot x of `ct`, y = (2x - a - b)/(b - a): a ChebyshevPlan, or Chebyshev coefficients from
    which one is built.  `ct` an RnsCiphertext or a DeepCiphertext; the result is of its class.  Consumes
    plan.levels levels; the result has the ciphertext's scale (up to float rounding).  A ciphertext with fewer levels is refused
    before anything runs."""
    plan = plan_or_coeffs if isinstance(plan_or_coeffs, ChebyshevPlan) else ChebyshevPlan.build(plan_or_coeffs, interval)
    return plan.run(ct, rlk)


class RnsClientKey(ClientKeyBase):
    """The CKKS secret under every prime of an RnsParam: the same ternary row (KEY row 0) as residues and evals per limb, the
    special prime's last.  Rows of a seed, as ClientKey and disjoint from its rows:
        [0, 2^56)                    fresh encryptions
        1 2^56 + slot                public_key(slot)
        2 2^56 + 64 slot + j         digit j of relin_key(slot)
        3 2^56 + 64 slot + j         digit j of galois_key(g, slot)
    A builder refuses a slot (0 <= slot < 2^16) it has used."""

    RLK_BASE, GK_BASE = 2 << 56, 3 << 56

    def __init__(self, seed, param, delta, d_s, d_s_evals, sigma):
        super().__init__(seed, sigma)
        self.param, self.delta, self.d_s, self.d_s_evals = param, float(delta), d_s, d_s_evals
        self.encoder = Encoder(param.n, delta)

    _ciphertext = RnsCiphertext   # what encrypt returns

    def _all_plans(self):
        return self.param.plans() + self.param.special_plans()

    @classmethod
    def generate(cls, seed, param, delta, sigma=3.2):
        torch = _torch()
        plans = param.plans() + param.special_plans()
        d_s = torch.empty((len(plans), param.n), dtype=torch.int64, device="cuda")
        d_e = torch.empty_like(d_s)
        for i, plan in enumerate(plans):
            binding.ckks_secret_key_dev(plan, seed, 0, d_s[i].data_ptr())
            plan.forward_dev(d_s[i].data_ptr(), d_e[i].data_ptr(), 1)
        torch.cuda.synchronize()
        return cls(seed, param, delta, d_s, d_e, sigma)

    def public_key(self, slot=0):
        """fhe_ckks_public_key_dev per limb with one row: the residues of one key (-a s + e, a) modulo Q"""
        torch = _torch()
        row = self._take_slot("public_key", self.PK_BASE, slot)
        plans = self.param.plans()
        pk = torch.empty((len(plans), 2, self.param.n), dtype=torch.int64, device="cuda")
        for i, plan in enumerate(plans):
            binding.ckks_public_key_dev(plan, self.seed, row, self.d_s[i].data_ptr(), self._cdt_ptr(), self._m, pk[i].data_ptr())
            plan.forward_dev(pk[i].data_ptr(), pk[i].data_ptr(), 2)
        return RnsPublicKey(self.param, pk)

    def relin_key(self, slot=0):
        torch = _torch()
        row = self._take_slot("relin_key", self.RLK_BASE, slot, rows=64)
        k = len(self.param.moduli)
        rlk = torch.empty((k, k + 1, 2, self.param.n), dtype=torch.int64, device="cuda")
        binding.ckks_rns_relin_key_dev(self.param.plans(), self.param.special_plan(), self.seed, row, self.d_s.data_ptr(), self._cdt_ptr(),
                                       self._m, rlk.data_ptr())
        return RnsRelinKey(self.param, rlk)

    def galois_key(self, g, slot):
        """the key of sigma_g from rows GK_BASE + 64 slot + j; one slot per key, whatever its g"""
        torch = _torch()
        g = int(g)
        if g % 2 == 0 or not 0 < g < 2 * self.param.n:
            raise ValueError(f"galois_key: g={g} must be odd and in [1, 2n)")
        row = self._take_slot("galois_key", self.GK_BASE, slot, rows=64)
        k = len(self.param.moduli)
        gk = torch.empty((k, k + 1, 2, self.param.n), dtype=torch.int64, device="cuda")
        binding.ckks_rns_galois_key_dev(self.param.plans(), self.param.special_plan(), self.seed, row, g, self.d_s.data_ptr(),
                                        self._cdt_ptr(), self._m, gk.data_ptr())
        return RnsGaloisKey(self.param, g, gk)

    def rotation_key(self, step, slot):
        return self.galois_key(galois_element(self.param.n, step), slot)

    def conjugation_key(self, slot):
        return self.galois_key(conjugation_element(self.param.n), slot)

    def encode_diagonals(self, rows, steps, level, scale):
        """encode_diagonals with this key's encoder"""
        return encode_diagonals(self.param, self.encoder, rows, steps, level, scale)

    def encrypt(self, pk, m, scale=None):
        """m int64 coefficients (n,) or (batch, n) -> RnsCiphertext at the top level: fhe_ckks_encrypt_dev per limb on the same rows"""
        torch = _torch()
        n = self.param.n
        msg = np.ascontiguousarray(m, dtype=np.int64).reshape(-1, n)
        batch = msg.shape[0]
        d_m = torch.from_numpy(msg).cuda()
        plans = self.param.plans()
        out = torch.empty((len(plans), 2, batch, n), dtype=torch.int64, device="cuda")

        def limbs(row):
            for i, plan in enumerate(plans):
                binding.ckks_encrypt_dev(plan, self.seed, row, pk.d_evals[i].data_ptr(), d_m.data_ptr(), n, self._cdt_ptr(), self._m, out[i].data_ptr(), batch)
                plan.forward_dev(out[i].data_ptr(), out[i].data_ptr(), 2 * batch)

        self._on_fresh_rows(batch, limbs)
        return self._ciphertext(self.param, out, self.param.max_level, self.delta if scale is None else scale)

    def decrypt(self, ct):
        """limb 0 only: exact while |m + e| < q_0 / 2 -> int64 coefficients [batch][n]"""
        torch = _torch()
        if ct.param != self.param:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the ciphertext is not in this key's chain")
        plan = self.param.plans(0)[0]
        coef = torch.empty_like(ct.d[0])
        plan.inverse_dev(ct.d[0].data_ptr(), coef.data_ptr(), 2 * ct.batch)
        out = torch.empty((ct.batch, self.param.n), dtype=torch.int64, device="cuda")
        binding.ckks_decrypt_dev(plan, self.d_s_evals[0].data_ptr(), coef.data_ptr(), out.data_ptr(), ct.batch)
        return out.cpu().numpy()

    def encode_and_encrypt(self, pk, z):
        return self.encrypt(pk, self.encoder.encode(z))

    def decrypt_and_decode(self, ct):
        return self.encoder.decode(self.decrypt(ct), ct.scale)


# ---- the deep chain: grouped-digit key switching, up to 32 limbs (ckks_deep.hip) --------------------------------------
@dataclass(frozen=True)
class DeepParam:
    """n, the chain primes q_0 .. q_{L-1} (1 <= L <= 32) and the special primes p_0 .. p_{alpha-1} (1 <= alpha <= 8) of the
    switching keys, P their product: all distinct, 1 modulo 2n, below 2^62.  Digit group j holds limbs [j alpha, (j + 1) alpha);
    P must not be below the product of a group's primes.  Level l = limbs 0 .. l."""
    n: int
    moduli: tuple
    specials: tuple

    def __post_init__(self):
        object.__setattr__(self, "moduli", tuple(int(q) for q in self.moduli))
        object.__setattr__(self, "specials", tuple(int(p) for p in self.specials))
        if not 1 <= len(self.moduli) <= binding.FHE_CKKS_DEEP_MAX_LIMBS:
            raise ValueError("DeepParam: the chain has 1 to 32 primes")
        if not 1 <= len(self.specials) <= binding.FHE_CKKS_DEEP_MAX_SPECIALS:
            raise ValueError("DeepParam: there are 1 to 8 special primes")
        primes = self.moduli + self.specials
        if len(set(primes)) != len(primes):
            raise ValueError("DeepParam: the primes of the chain and the special primes must be distinct")
        if any(p >= 1 << 62 for p in primes):
            raise ValueError("DeepParam: every prime must be below 2^62")
        if any(p % (2 * self.n) != 1 for p in primes):
            raise ValueError("DeepParam: every prime must be 1 modulo 2n")
        P, alpha = 1, len(self.specials)
        for p in self.specials:
            P *= p
        for j in range(0, len(self.moduli), alpha):
            Qj = 1
            for q in self.moduli[j:j + alpha]:
                Qj *= q
            if P < Qj:
                raise ValueError(f"DeepParam: the product of the special primes is below that of digit group {j // alpha}")

    @property
    def max_level(self):
        return len(self.moduli) - 1

    @property
    def dnum(self):
        return -(-len(self.moduli) // len(self.specials))

    def plans(self, level=None):
        """the plans of limbs 0 .. level (default: all)"""
        k = len(self.moduli) if level is None else level + 1
        return [_plan(RingParam(q, self.n)) for q in self.moduli[:k]]

    def special_plans(self):
        return [_plan(RingParam(p, self.n)) for p in self.specials]


class DeepCiphertext(RnsCiphertext):
    """RnsCiphertext on a DeepParam: +, -, at_level, add_plain and mul_plain are the base class's, per limb; the products, the
    rescale, the Galois maps and the diagonal sums go through the fhe_ckks_deep_* entry points; linear_transform is the base
    class's composition over them.  The fused scalar sums, the inner products and the Chebyshev plans are reached through the
    module's lincomb, dot and eval_chebyshev, which dispatch on the operands' param and return DeepCiphertexts;
    the methods mul_const, add_const and eval_chebyshev keep raising NotImplementedError, as the tests of §36 and §37 assert,
    and so does linear_transform_hoisted, which is not carried to the deep chain yet."""

    def mul(self, rhs, rlk):
        """ct x ct and relinearisation (fhe_ckks_deep_mul_dev); the scale multiplies and the result is NOT rescaled"""
        if rlk.param != self.param:
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "the relinearisation key is not of this ciphertext's chain")
        a, b, level = self._pair(rhs)
        out = _torch().empty_like(a.d)
        binding.ckks_deep_mul_dev(self.param.plans(level), self.param.special_plans(), rlk.d_rlk.data_ptr(), len(self.param.moduli), a.d.data_ptr(), b.d.data_ptr(),
                                  out.data_ptr(), self.batch)
        return DeepCiphertext(self.param, out, level, self.scale * rhs.scale)

    def rescale(self):
        if self.level == 0:
            raise binding.FheError(binding.FHE_E_INVALID, "rescale: a ciphertext at level 0 cannot be rescaled")
        torch = _torch()
        out = torch.empty((self.level, 2, self.batch, self.param.n), dtype=torch.int64, device="cuda")
        binding.ckks_deep_rescale_dev(self.param.plans(self.level), self.d.data_ptr(), out.data_ptr(), self.batch)
        return DeepCiphertext(self.param, out, self.level - 1, self.scale / self.param.moduli[self.level])

    def rotate_many(self, gks):
        """sigma_g of this ciphertext for every key of `gks` from one call (fhe_ckks_deep_galois_dev)"""
        torch = _torch()
        gks = list(gks)
        if any(gk.param != self.param for gk in gks):
            raise binding.FheError(binding.FHE_E_PARAM_MISMATCH, "a Galois key is not of this ciphertext's chain")
        out = torch.empty((len(gks),) + tuple(self.d.shape), dtype=torch.int64, device="cuda")
        binding.ckks_deep_galois_dev(self.param.plans(self.level), self.param.special_plans(), [gk.d_gk.data_ptr() for gk in gks], [gk.g for gk in gks],
                                     len(self.param.moduli), self.d.data_ptr(), out.data_ptr(), self.batch)
        return [DeepCiphertext(self.param, out[r], self.level, self.scale) for r in range(len(gks))]

    def _plain(self, m):
        """signed rows -> evals [level + 1][batch][n]: fhe_ckks_rns_from_i64_dev is limb-independent, so in slices of 8 plans"""
        torch = _torch()
        n = self.param.n
        rows = np.array(np.broadcast_to(np.asarray(m, dtype=np.int64), (self.batch, n)))
        out = torch.empty((self.level + 1, self.batch, n), dtype=torch.int64, device="cuda")
        d_rows = torch.from_numpy(rows).cuda()
        plans = self.param.plans(self.level)
        for i in range(0, len(plans), 8):
            binding.ckks_rns_from_i64_dev(plans[i:i + 8], d_rows.data_ptr(), out[i:i + 8].data_ptr(), self.batch)
        return out

    def __neg__(self):
        out = _torch().empty_like(self.d)
        for i, plan in enumerate(self.param.plans(self.level)):
            binding._check(binding.load_library().fhe_rq_neg_dev(plan.handle, self.d[i].data_ptr(), out[i].data_ptr(), 2 * self.batch, None))
        return DeepCiphertext(self.param, out, self.level, self.scale)

    def diag_sum(self, pts, gks):
        """RnsCiphertext.diag_sum from one fhe_ckks_deep_diag_sum_dev call: pts a DeepPlaintextSet"""
        torch = _torch()
        if not isinstance(pts, DeepPlaintextSet):
            raise ValueError("diag_sum: the plaintexts of a deep chain are a DeepPlaintextSet")
        key_ptrs = self._diag_keys(pts, gks)
        out = torch.empty((pts.outputs,) + tuple(self.d.shape), dtype=torch.int64, device="cuda")
        binding.ckks_deep_diag_sum_dev(self.param.plans(self.level), self.param.special_plans(), key_ptrs, pts.gs, len(self.param.moduli), pts.d_pts.data_ptr(),
                                       pts.outputs, self.d.data_ptr(), out.data_ptr(), self.batch)
        return [DeepCiphertext(self.param, out[o], self.level, self.scale * pts.scale) for o in range(pts.outputs)]

    def _not_yet(self, *args, **kwargs):
        raise NotImplementedError("not carried to the deep chain yet (DESIGN.md §36)")

    linear_transform_hoisted = mul_const = add_const = eval_chebyshev = _not_yet


class DeepClientKey(RnsClientKey):
    """RnsClientKey on a DeepParam, on the same row plan: a key slot's 64 rows cover dnum <= 32 digit groups.  The secret's rows
    are the chain's, then the special primes'."""

    _ciphertext = DeepCiphertext

    def _switch_key(self, what, base, slot, build, *element):
        torch = _torch()
        row = self._take_slot(what, base, slot, rows=64)
        L, alpha = len(self.param.moduli), len(self.param.specials)
        key = torch.empty((self.param.dnum, L + alpha, 2, self.param.n), dtype=torch.int64, device="cuda")
        build(self.param.plans(), self.param.special_plans(), self.seed, row, *element, self.d_s.data_ptr(), self._cdt_ptr(), self._m, key.data_ptr())
        return key

    def relin_key(self, slot=0):
        return RnsRelinKey(self.param, self._switch_key("relin_key", self.RLK_BASE, slot, binding.ckks_deep_relin_key_dev))

    def galois_key(self, g, slot):
        g = int(g)
        if g % 2 == 0 or not 0 < g < 2 * self.param.n:
            raise ValueError(f"galois_key: g={g} must be odd and in [1, 2n)")
        return RnsGaloisKey(self.param, g, self._switch_key("galois_key", self.GK_BASE, slot, binding.ckks_deep_galois_key_dev, g))

