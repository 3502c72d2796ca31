"""Pyfhel-2.3.1-shaped compatibility API over the hefl CKKS engine.

The reference drives all HE through Pyfhel 2.3.1 (README.md:7 pins the
version; FLPyfhelin.py:330-344 contextGen/keyGen, :217 encryptFrac, :295
decryptFrac, :337-338/:352-353 to_bytes_/from_bytes_ context/publicKey/
secretKey, :381 PyCtxt.__add__, :385 PyCtxt.__mul__(float), pickled
ciphertexts with a context re-attach at :321).

This module keeps that exact surface — same names, same parameter names
(`m`, not `n`; `p` accepted and ignored by CKKS) — while the engine
underneath is the from-scratch RNS-CKKS of hefl.he.ckks (slot-packing,
HIP kernels on MI355X). Deliberate deltas (SURVEY.md §7 quirks catalog):
`relinKeyGen` works instead of raising NameError (reference
FLPyfhelin.py:363 is dead+buggy), and a pickled PyCtxt round-trips
without a live context (`_pyfhel` re-attach still supported, no longer
required).
"""
from __future__ import annotations

import io
import struct
from typing import Optional

import numpy as np
import torch

from ..config import HEConfig
from .ckks import CKKSContext, Ciphertext, CtxtTensor, KeyPair

_MAGIC = b"HEFL"
_VERSION = 1
# Version 2 appends one byte after the q_bits: the slot packing. A context
# with real packing is still written as version 1, byte for byte what it
# always was, so a stream without the field reads as "real".
_VERSION_PACKING = 2
_PACKINGS = ("real", "complex")


def _pack_header(kind: bytes, cfg: HEConfig) -> bytes:
    ver = _VERSION if cfg.packing == "real" else _VERSION_PACKING
    head = _MAGIC + struct.pack(
        "<H4sIIIH", ver, kind, cfg.m, cfg.scale_bits, cfg.sec,
        len(cfg.q_bits)) + struct.pack(f"<{len(cfg.q_bits)}I", *cfg.q_bits)
    if ver == _VERSION_PACKING:
        head += struct.pack("<B", _PACKINGS.index(cfg.packing))
    return head


def _unpack_header(buf: bytes, expect: bytes):
    if buf[:4] != _MAGIC:
        raise ValueError("not a hefl HE byte stream")
    ver, kind, m, scale_bits, sec, nq = struct.unpack("<H4sIIIH", buf[4:24])
    if ver not in (_VERSION, _VERSION_PACKING):
        raise ValueError(f"unsupported version {ver}")
    if kind != expect:
        raise ValueError(f"expected {expect!r} stream, got {kind!r}")
    q_bits = struct.unpack(f"<{nq}I", buf[24:24 + 4 * nq])
    off = 24 + 4 * nq
    packing = "real"
    if ver == _VERSION_PACKING:
        (code,) = struct.unpack("<B", buf[off:off + 1])
        if code >= len(_PACKINGS):
            raise ValueError(f"unknown packing code {code}")
        packing = _PACKINGS[code]
        off += 1
    cfg = HEConfig(m=m, scale_bits=scale_bits, sec=sec, q_bits=tuple(q_bits),
                   packing=packing)
    return cfg, off


class PyCtxt:
    """A single CKKS ciphertext with Pyfhel-2.3.1 PyCtxt semantics.

    Supports `ct + ct`, `ct + 0` (the reference seeds its accumulator with
    int zeros, FLPyfhelin.py:380-381), and `ct * float` (plaintext-scalar
    multiply, :385). Picklable standalone; `_pyfhel` attribute kept for
    reference-style re-attach (FLPyfhelin.py:321) but a fresh context is
    rebuilt from the embedded params when absent.
    """

    def __init__(self, ct: Ciphertext, pyfhel: "Pyfhel"):
        self._ct = ct
        self._pyfhel = pyfhel

    # ----- arithmetic (the ops the reference exercises) -----
    def _he(self) -> "Pyfhel":
        if self._pyfhel is None:
            raise ValueError("PyCtxt has no attached Pyfhel context")
        return self._pyfhel

    def __add__(self, other):
        if isinstance(other, (int, float)) and other == 0:
            # clone, not self: the reference seeds accumulators with int 0
            # (FLPyfhelin.py:380-381) — returning self would alias the
            # accumulator to the client's ciphertext, so a later in-place
            # mutation of the sum would corrupt the client's upload
            return PyCtxt(self._ct.clone(), self._pyfhel)
        if isinstance(other, PyCtxt):
            he = self._he()
            return PyCtxt(he._ctx.add(self._ct, other._ct), he)
        return NotImplemented

    __radd__ = __add__

    def __mul__(self, other):
        if isinstance(other, (int, float)):
            he = self._he()
            out = he._ctx.mul_scalar(self._ct, float(other))
            if out.level > 1:
                out = he._ctx.rescale(out)
            return PyCtxt(out, he)
        return NotImplemented

    __rmul__ = __mul__

    # ----- slot rotation: ct << k moves slot j+k into slot j (left) -----
    def __lshift__(self, k):
        if isinstance(k, (int, np.integer)):
            return self._he().rotate(self, int(k))
        return NotImplemented

    def __rshift__(self, k):
        if isinstance(k, (int, np.integer)):
            return self._he().rotate(self, -int(k))
        return NotImplemented

    # ----- pickling: standalone, context params embedded -----
    def __getstate__(self):
        he = self._pyfhel
        return {
            "cfg": he._ctx.cfg if he is not None else None,
            "data": self._ct.data.cpu().numpy(),
            "scale": self._ct.scale,
        }

    def __setstate__(self, state):
        self._ct = Ciphertext(torch.from_numpy(state["data"]), state["scale"])
        self._pyfhel = Pyfhel() if state["cfg"] is None else None
        if state["cfg"] is not None:
            he = Pyfhel()
            he.contextGen_cfg(state["cfg"])
            self._pyfhel = he


class Pyfhel:
    """Pyfhel-2.3.1-compatible facade (reference API at FLPyfhelin.py:330-364).

    `contextGen(p=..., m=..., sec=...)` keeps the Pyfhel signature: `m` is
    the ring degree, `p` is accepted for BFV compat and ignored by CKKS,
    `sec` is advisory. Extra kwargs (scale_bits, q_bits, device) configure
    the CKKS engine.
    """

    def __init__(self):
        self._ctx: Optional[CKKSContext] = None
        self._keys: Optional[KeyPair] = None
        self._pk: Optional[torch.Tensor] = None
        self._sk: Optional[torch.Tensor] = None
        self._device = "cpu"

    # ----- context -----
    def contextGen(self, p: int = 65537, m: int = 2048, sec: int = 128,
                   base: int = 2, flagBatching: bool = False,
                   scale_bits: int = 40, q_bits=(60, 40),
                   seed: Optional[int] = None, device: str = "cpu",
                   packing: str = "real"):
        """packing="complex" makes encrypt_tensor put two values in each
        slot; encryptFrac / decryptFrac stay one real scalar either way."""
        cfg = HEConfig(m=m, scale_bits=scale_bits, q_bits=tuple(q_bits),
                       sec=sec, p=p, seed=seed, packing=packing)
        self.contextGen_cfg(cfg, device=device)

    def contextGen_cfg(self, cfg: HEConfig, device: str = "cpu"):
        self._device = device
        self._ctx = CKKSContext(cfg, device=device)

    @property
    def context(self) -> CKKSContext:
        if self._ctx is None:
            raise ValueError("contextGen has not been called")
        return self._ctx

    def __repr__(self):
        if self._ctx is None:
            return "<Pyfhel (no context)>"
        c = self._ctx.cfg
        # mirrors the stored notebook repr shape: contx(p=..., m=..., ...)
        return (f"<Pyfhel CKKS contx(p={c.p}, m={c.m}, base=2, sec={c.sec}, "
                f"scale=2^{c.scale_bits}, qbits={list(c.q_bits)}, batch=True)>")

    # ----- keys -----
    def keyGen(self):
        kp = self.context.keygen()
        self._keys = kp
        self._pk = kp.pk
        self._sk = kp.sk

    def relinKeyGen(self, bitCount: int = 1, size: int = 5):
        """Generate relinearization keys (reference intent at
        FLPyfhelin.py:357-364; its version is dead code with a NameError)."""
        if self._sk is None:
            raise ValueError("keyGen must run before relinKeyGen")
        if self._keys is None:  # keys restored from bytes, not keyGen()
            self._keys = KeyPair(sk=self._sk, pk=self._pk)
        self._keys.relin = self.context.relin_keygen(self._sk)

    def rotateKeyGen(self, bitCount: int = 1, steps=None,
                     conjugate: bool = True):
        """Generate Galois keys for slot rotation (default steps: +-2^k,
        from which any step composes) and, by default, conjugation.
        `bitCount` is accepted for Pyfhel signature parity and ignored:
        the digits are the RNS limbs."""
        if self._sk is None:
            raise ValueError("keyGen must run before rotateKeyGen")
        if self._keys is None:  # keys restored from bytes, not keyGen()
            self._keys = KeyPair(sk=self._sk, pk=self._pk)
        gk = self.context.galois_keygen(self._sk, steps=steps,
                                        conjugate=conjugate)
        if self._keys.galois:   # a later call adds to the keys already held
            gk = {**self._keys.galois, **gk}
        self._keys.galois = gk

    @property
    def _galois(self):
        return None if self._keys is None else self._keys.galois

    def _set_galois(self, gk):
        if self._keys is None:
            self._keys = KeyPair(sk=self._sk, pk=self._pk)
        self._keys.galois = gk

    def rotate(self, ct, k: int):
        """Rotate a PyCtxt or a CtxtTensor left by k slots (k < 0: right)."""
        if isinstance(ct, CtxtTensor):
            return self.context.rotate_tensor(ct, k, self._galois)
        return PyCtxt(self.context.rotate(ct._ct, k, self._galois), self)

    def rotate_many(self, ctxt, steps):
        """[rotate(ctxt, k) for k in steps] from one hoisted digit
        decomposition: a list of PyCtxt (of CtxtTensor for a CtxtTensor), in
        the order given. Every non-zero step needs its exact key —
        rotateKeyGen(steps=steps)."""
        if isinstance(ctxt, CtxtTensor):
            return self.context.rotate_many_tensor(ctxt, steps, self._galois)
        return [PyCtxt(c, self) for c in
                self.context.rotate_many(ctxt._ct, steps, self._galois)]

    def conjugate(self, ct):
        """Complex-conjugate every slot of a PyCtxt or a CtxtTensor."""
        if isinstance(ct, CtxtTensor):
            return self.context.conjugate_tensor(ct, self._galois)
        return PyCtxt(self.context.conjugate(ct._ct, self._galois), self)

    # ----- scalar API (reference-exact shape) -----
    def encryptFrac(self, value: float) -> PyCtxt:
        """One scalar -> one ciphertext (reference FLPyfhelin.py:217).
        Kept for API parity; the batched tensor path is encrypt_tensor."""
        if self._pk is None:
            raise ValueError("no public key")
        pt = self.context.encode(np.array([float(value)]))
        return PyCtxt(self.context.encrypt(pt, self._pk), self)

    def decryptFrac(self, ct: PyCtxt) -> float:
        if self._sk is None:
            raise ValueError("no secret key")
        pt = self.context.decrypt(ct._ct, self._sk)
        return float(self.context.decode(pt, 1)[..., 0])

    # ----- batched tensor API (the hot path) -----
    def encrypt_tensor(self, vec: torch.Tensor) -> CtxtTensor:
        if self._pk is None:
            raise ValueError("no public key")
        return self.context.encrypt_tensor(vec, self._pk)

    def decrypt_tensor(self, ct: CtxtTensor) -> torch.Tensor:
        if self._sk is None:
            raise ValueError("no secret key")
        return self.context.decrypt_tensor(ct, self._sk)

    # ----- serialization (reference FLPyfhelin.py:337-338, 352-353, 257-259) -----
    def to_bytes_context(self) -> bytes:
        return _pack_header(b"CTX\x00", self.context.cfg)

    def from_bytes_context(self, buf: bytes):
        cfg, _ = _unpack_header(buf, b"CTX\x00")
        self.contextGen_cfg(cfg, device=self._device)

    def _key_bytes(self, kind: bytes, t: torch.Tensor) -> bytes:
        head = _pack_header(kind, self.context.cfg)
        body = io.BytesIO()
        np.save(body, t.cpu().numpy(), allow_pickle=False)
        return head + body.getvalue()

    def _key_from_bytes(self, kind: bytes, buf: bytes) -> torch.Tensor:
        cfg, off = _unpack_header(buf, kind)
        if self._ctx is None:
            self.contextGen_cfg(cfg, device=self._device)
        arr = np.load(io.BytesIO(buf[off:]), allow_pickle=False)
        return torch.from_numpy(arr).to(self.context.device)

    def to_bytes_publicKey(self) -> bytes:
        if self._pk is None:
            raise ValueError("no public key")
        return self._key_bytes(b"PK\x00\x00", self._pk)

    def from_bytes_publicKey(self, buf: bytes):
        self._pk = self._key_from_bytes(b"PK\x00\x00", buf)

    def to_bytes_secretKey(self) -> bytes:
        if self._sk is None:
            raise ValueError("no secret key")
        return self._key_bytes(b"SK\x00\x00", self._sk)

    def from_bytes_secretKey(self, buf: bytes):
        self._sk = self._key_from_bytes(b"SK\x00\x00", buf)

    def to_bytes_rotateKey(self) -> bytes:
        """Versioned header (kind GK), key count, then per key its Galois
        element (u64) and the tensor as one .npy record."""
        gk = self._galois
        if not gk:
            raise ValueError("no rotation keys — run rotateKeyGen first")
        body = io.BytesIO()
        body.write(struct.pack("<I", len(gk)))
        for g, t in gk.items():
            body.write(struct.pack("<Q", int(g)))
            np.save(body, t.cpu().numpy(), allow_pickle=False)
        return _pack_header(b"GK\x00\x00", self.context.cfg) + body.getvalue()

    def from_bytes_rotateKey(self, buf: bytes):
        cfg, off = _unpack_header(buf, b"GK\x00\x00")
        if self._ctx is None:
            self.contextGen_cfg(cfg, device=self._device)
        body = io.BytesIO(buf[off:])
        (count,) = struct.unpack("<I", body.read(4))
        gk = {}
        for _ in range(count):
            (g,) = struct.unpack("<Q", body.read(8))
            arr = np.load(body, allow_pickle=False)
            gk[int(g)] = torch.from_numpy(arr).to(self.context.device)
        self._set_galois(gk)

    # Pyfhel pickles whole objects in the reference's export dict
    # (FLPyfhelin.py:233); support that directly. The SECRET key is never
    # pickled: the reference's C-backed pickled Pyfhel carries no usable key
    # material, and a pickled object lands in 'public' artifacts
    # (publickey.pickle, per-client uploads) that the pk-only aggregation
    # server reads — sk must travel only via the explicit
    # to_bytes_secretKey/privatekey.pickle path (hefl/fl/keys.py).
    def __getstate__(self):
        state = {"cfg": None, "pk": None}
        if self._ctx is not None:
            state["cfg"] = self._ctx.cfg
        if self._pk is not None:
            state["pk"] = self._pk.cpu().numpy()
        if self._galois:  # evaluation keys are public, like pk
            state["galois"] = {int(g): t.cpu().numpy()
                               for g, t in self._galois.items()}
        return state

    def __setstate__(self, state):
        self.__init__()
        if state["cfg"] is not None:
            self.contextGen_cfg(state["cfg"])
        if state["pk"] is not None:
            self._pk = torch.from_numpy(state["pk"])
        if state.get("sk") is not None:  # legacy pickles only
            self._sk = torch.from_numpy(state["sk"])
        if state.get("galois"):  # absent from pickles made before rotation
            self._set_galois({int(g): torch.from_numpy(a)
                              for g, a in state["galois"].items()})
