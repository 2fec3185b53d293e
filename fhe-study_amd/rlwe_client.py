"""What the RLWE client keys share (bfv.ClientKey, ckks.ClientKey, ckks.RnsClientKey): the seed, the error
table of `sigma` on the device, the bookkeeping of a seed's rows, and the public key both single-modulus schemes return.
Rows never repeat within a seed: fresh encryptions take [0, 2^56) in call order, a builder takes a row at or above its
`*_BASE` (a multiple of 2^56) by its slot, and refuses a slot (0 <= slot < 2^16) it has used."""
from .arith import plan_of as _plan
from .device import from_dev as _from_dev, to_dev as _to_dev, torch as _torch
from .tfhe import cdt_table


class PublicKey:
    """(pk0, pk1) mod q as coefficients (numpy) and, resident on the device, both halves as evals [2][n] (bfv lib.rs:39)"""

    def __init__(self, param, coeffs, d_evals):
        self.param, self.coeffs, self.d_evals = param, coeffs, d_evals


class ClientKeyBase:
    ENCRYPT_ROWS = 1 << 56
    PK_BASE = 1 << 56

    def __init__(self, seed, sigma):
        self.seed = bytes(seed)
        self._next_row, self._slots = 0, set()
        tab = cdt_table(sigma)
        self._cdt, self._m = (_to_dev(tab) if len(tab) else None), len(tab)

    def _cdt_ptr(self):
        return self._cdt.data_ptr() if self._m else None

    def _take_slot(self, kind, base, slot, rows=1):
        """the first row of builder `kind`'s slot, which holds `rows` rows"""
        if not 0 <= int(slot) < 1 << 16:
            raise ValueError(f"{kind}: slot must be in [0, 2^16)")
        if (kind, int(slot)) in self._slots:
            raise ValueError(f"{kind}: slot {slot} of this seed is already used; a second key needs a slot of its own")
        self._slots.add((kind, int(slot)))
        return base + rows * int(slot)

    def _public_key(self, public_key_dev, ring, slot):
        """pk = (-a s + e, a) of row PK_BASE + slot from the scheme's entry point (binding.*_public_key_dev) -> PublicKey"""
        torch = _torch()
        row = self._take_slot("public_key", self.PK_BASE, slot)
        pk = torch.empty((2, ring.n), dtype=torch.int64, device="cuda")
        ev = torch.empty_like(pk)
        public_key_dev(_plan(ring), self.seed, row, self.d_s.data_ptr(), self._cdt_ptr(), self._m, pk.data_ptr())
        _plan(ring).forward_dev(pk.data_ptr(), ev.data_ptr(), 2)
        return PublicKey(self.param, _from_dev(pk), ev)

    def _on_fresh_rows(self, batch, encrypt):
        """encrypt(first_row) on the next `batch` encryption rows, which are spent once it has returned"""
        if self._next_row + batch > self.ENCRYPT_ROWS:
            raise ValueError("encrypt: this seed's 2^56 encryption rows are used up")
        encrypt(self._next_row)
        self._next_row += batch
