"""RNS-CKKS scheme: context, keys, encrypt/decrypt, homomorphic ops.

From-scratch replacement for the reference's Pyfhel 2.3.1 -> SEAL 2.3 BFV
stack (FLPyfhelin.py:330-344 contextGen/keyGen; :217 encryptFrac; :295
decryptFrac; :381 ct+ct; :385 ct*plain). Differences by design (SURVEY.md
section 0): CKKS instead of BFV+FractionalEncoder, and slot packing — one
ciphertext carries n/2 weights instead of one scalar per ciphertext.

The scheme logic is written once, device-agnostic, over a small backend
interface (NTT + pointwise modular ops). CpuBackend = exact big-int numpy
(the test oracle); GpuBackend = hand-written HIP kernels on MI355X
(hefl/csrc/ntt.hip), ciphertexts resident in HBM as int64 tensors [.., 2, L, n].
Ciphertext data layout is all-reduce-ready: limb values < 2**60 so an int64
SUM over <= 8 clients cannot overflow (lazy reduction; hefl/fl/secure.py).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from ..config import HEConfig
from .encoder import Encoder
from .ntt_cpu import NttTables, fwd_ntt, inv_ntt
from .primes import gen_prime_chain

_TABLE_CACHE = {}


def _tables(q: int, n: int) -> NttTables:
    key = (q, n)
    if key not in _TABLE_CACHE:
        _TABLE_CACHE[key] = NttTables(q, n)
    return _TABLE_CACHE[key]


# ---------------------------------------------------------------------------
# Backends
# ---------------------------------------------------------------------------

class CpuBackend:
    """Exact reference backend (numpy object ints)."""

    def __init__(self, primes: Sequence[int], n: int):
        self.primes = list(primes)
        self.n = n
        self.tb = [_tables(q, n) for q in primes]

    def ntt(self, x: torch.Tensor, limb: int, inverse: bool = False) -> torch.Tensor:
        a = x.cpu().numpy().astype(object)
        tb = self.tb[limb]
        out = inv_ntt(a, tb) if inverse else fwd_ntt(a, tb)
        return torch.from_numpy(out.astype(np.int64))

    def modmul(self, a: torch.Tensor, b: torch.Tensor, limb: int) -> torch.Tensor:
        q = self.primes[limb]
        r = (a.cpu().numpy().astype(object) * b.cpu().numpy().astype(object)) % q
        return torch.from_numpy(r.astype(np.int64))

    def modmul_scalar(self, a: torch.Tensor, s: int, limb: int) -> torch.Tensor:
        q = self.primes[limb]
        r = (a.cpu().numpy().astype(object) * (s % q)) % q
        return torch.from_numpy(r.astype(np.int64))


class GpuBackend:
    """MI355X backend: batched HIP NTT + Barrett pointwise kernels (hefl._C)."""

    def __init__(self, primes: Sequence[int], n: int, device: torch.device):
        import hefl
        self._C = hefl.load_extension()
        self.primes = list(primes)
        self.n = n
        self.device = device
        # Device-side twiddle tables: [L, n] fwd / inv (+ Shoup companions),
        # built once from the exact CPU tables.
        w = torch.stack([torch.from_numpy(_tables(q, n).w.astype(np.int64))
                         for q in primes])
        winv = torch.stack([torch.from_numpy(_tables(q, n).winv.astype(np.int64))
                            for q in primes])
        qs = torch.tensor(self.primes, dtype=torch.int64)
        ninv = torch.tensor([_tables(q, n).n_inv for q in primes], dtype=torch.int64)

        def shoup(v, q):
            return torch.from_numpy(
                ((v.numpy().astype(object) << 64) // q).astype(np.uint64).astype(np.int64))

        self.w = w.to(device)
        self.w_shoup = torch.stack([shoup(w[i], q) for i, q in enumerate(primes)]).to(device)
        self.winv = winv.to(device)
        self.winv_shoup = torch.stack([shoup(winv[i], q) for i, q in enumerate(primes)]).to(device)
        self.qs = qs.to(device)
        self.ninv = ninv.to(device)
        self.ninv_shoup = torch.stack(
            [shoup(ninv[i:i + 1], q) for i, q in enumerate(primes)]).reshape(-1).to(device)
        # Barrett ratio words floor(2^128/q) per limb, for fused modmul
        words = []
        for q in primes:
            r = ((1 << 128) - 1) // q
            words.append([np.int64(np.uint64(r & ((1 << 64) - 1))),
                          np.int64(np.uint64(r >> 64))])
        self.ratio_words = torch.from_numpy(
            np.array(words, dtype=np.int64)).to(device)

    @staticmethod
    def _fresh(x: torch.Tensor) -> torch.Tensor:
        """Materialize a tensor the in-place NTT kernels may own: one copy,
        not two — .contiguous() already copies non-contiguous slices, so
        clone() only when it was a no-op (round-2 profile: the redundant
        clone showed up as ~2.5% of config #5 in hipMemcpy DtoD)."""
        c = x.contiguous()
        return c.clone() if c.data_ptr() == x.data_ptr() else c

    def ntt(self, x: torch.Tensor, limb: int, inverse: bool = False) -> torch.Tensor:
        out = self._fresh(x)
        flat = out.reshape(-1, self.n)
        if inverse:
            self._C.intt_batch(flat, self.winv[limb], self.winv_shoup[limb],
                               int(self.primes[limb]), int(self.ninv[limb]),
                               int(self.ninv_shoup[limb]))
        else:
            self._C.ntt_batch(flat, self.w[limb], self.w_shoup[limb],
                              int(self.primes[limb]))
        return out

    def modmul(self, a: torch.Tensor, b: torch.Tensor, limb: int) -> torch.Tensor:
        return self._C.modmul(a.contiguous(), b.contiguous(), int(self.primes[limb]))

    def modmul_scalar(self, a: torch.Tensor, s: int, limb: int) -> torch.Tensor:
        return self._C.modmul_scalar(a.contiguous(), int(s % self.primes[limb]),
                                     int(self.primes[limb]))

    # ----- fused multi-limb ops: one launch across the first L limbs -----
    def ntt_all(self, x: torch.Tensor, inverse: bool = False) -> torch.Tensor:
        """x [..., L, n] -> NTT per limb in ONE fused launch set."""
        L = x.shape[-2]
        out = self._fresh(x)
        flat = out.reshape(-1, L, self.n)
        if inverse:
            self._C.intt_limbs(flat, self.winv, self.winv_shoup, self.qs,
                               self.ninv, self.ninv_shoup, L)
        else:
            self._C.ntt_limbs(flat, self.w, self.w_shoup, self.qs, L)
        return out

    def modmul_limbs(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """a [..., L, n] x b ([..., L, n] or [L, n] tiling a), per-limb primes."""
        L = a.shape[-2]
        return self._C.modmul_limbs(a.contiguous(), b.contiguous(), self.qs,
                                    self.ratio_words, L, self.n)

    def modmul_scalar_limbs(self, a: torch.Tensor, scalars) -> torch.Tensor:
        """a [..., L, n] x per-limb plain scalars (python ints)."""
        L = a.shape[-2]
        sc, sh = [], []
        for i in range(L):
            q = self.primes[i]
            v = int(scalars[i]) % q
            sc.append(v)
            sh.append(np.int64(np.uint64((v << 64) // q)))
        dev = a.device
        sct = torch.tensor(sc, dtype=torch.int64, device=dev)
        sht = torch.tensor(np.array(sh, dtype=np.int64), device=dev)
        return self._C.modmul_scalar_limbs(a.contiguous(), sct, sht,
                                           self.qs, L, self.n)

    # ----- fused per-limb pointwise glue (replaces torch.remainder paths) ---
    def modadd_limbs(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        return self._C.modadd_limbs(a.contiguous(), b.contiguous(), self.qs,
                                    a.shape[-2], self.n)

    def modadd3_limbs(self, a, b, c) -> torch.Tensor:
        return self._C.modadd3_limbs(a.contiguous(), b.contiguous(),
                                     c.contiguous(), self.qs, a.shape[-2],
                                     self.n)

    def modsub_limbs(self, a: torch.Tensor, b: torch.Tensor,
                     L: Optional[int] = None) -> torch.Tensor:
        """out[.., l, :] = a[.., l, :] - b over the first L limbs (a may
        carry more limbs than L — the rescale slice without a copy)."""
        aL = a.shape[-2]
        L = aL if L is None else L
        return self._C.modsub_limbs(a.contiguous(), b.contiguous(), self.qs,
                                    L, aL, self.n)

    def bcast_center_mod(self, x: torch.Tensor, qc: int, L: int) -> torch.Tensor:
        """x [..., n] -> [..., L, n]: center mod qc (qc=0: already centered
        signed), then per-limb Barrett reduce. One launch replacing
        torch.where + broadcast remainder."""
        return self._C.bcast_center_mod(x.contiguous(), qc, self.qs,
                                        self.ratio_words, L)

    # ----- threshold decryption (hefl/fl/secure.py key_mode="threshold") -----
    def uniform_center_rns(self, bits: torch.Tensor, smudge_bits: int,
                           L: int) -> torch.Tensor:
        """bits [..., n] raw 64-bit draws -> [..., L, n] residues of noise
        uniform in [-2^smudge_bits, 2^smudge_bits). One launch."""
        return self._C.uniform_center_rns(bits.contiguous(), int(smudge_bits),
                                          self.qs, self.ratio_words, L)

    def ntt_all_(self, x: torch.Tensor) -> torch.Tensor:
        """In-place ntt_all for a contiguous tensor the caller owns."""
        L = x.shape[-2]
        self._C.ntt_limbs(x.view(-1, L, self.n), self.w, self.w_shoup,
                          self.qs, L)
        return x

    def pdec_share(self, ct: torch.Tensor, s_hat: torch.Tensor,
                   e_hat: torch.Tensor, add_c0: bool) -> torch.Tensor:
        """ct [..., 2, Lc, n] -> c1*s_hat + e_hat (+ c0) [..., Lc, n], c0/c1
        read in place (no slice copies). One launch."""
        return self._C.pdec_share(ct.contiguous(), s_hat.contiguous(),
                                  e_hat.contiguous(), bool(add_c0), self.qs,
                                  self.ratio_words)

    # ----- level-aware key-switch + slot rotation (CKKSContext.rotate) -----
    def level_tables(self, l: int) -> "LevelTables":
        """Prime / twiddle tables gathered at rows [0..l-1, L] — the limbs a
        key-switch at level l runs over (l chain primes + the special prime,
        which is the last row) — plus the mod-down scalars P^-1 mod q_i.
        Gathered once per level; every kernel takes its tables as arguments,
        so a level-l key-switch is the top-level launch sequence on these."""
        cache = self.__dict__.setdefault("_level_tables", {})
        if l not in cache:
            sp = len(self.primes) - 1
            if not 1 <= l <= sp:
                raise ValueError(f"level must be in [1, {sp}], got {l}")
            idx = torch.tensor(list(range(l)) + [sp], dtype=torch.int64,
                               device=self.device)
            P = self.primes[sp]
            pinv = [pow(P % q, -1, q) for q in self.primes[:l]]
            pinv_sh = [np.int64(np.uint64((v << 64) // q))
                       for v, q in zip(pinv, self.primes[:l])]
            cache[l] = LevelTables(
                idx=idx,
                w=self.w.index_select(0, idx),
                w_shoup=self.w_shoup.index_select(0, idx),
                qs=self.qs.index_select(0, idx),
                ratio_words=self.ratio_words.index_select(0, idx),
                pinv=torch.tensor(pinv, dtype=torch.int64, device=self.device),
                pinv_shoup=torch.tensor(np.array(pinv_sh, dtype=np.int64),
                                        device=self.device))
        return cache[l]

    def ntt_level_(self, x: torch.Tensor, tb: "LevelTables") -> torch.Tensor:
        """In-place forward NTT of a contiguous [..., l+1, n] tensor the
        caller owns, over the gathered limbs of `tb`."""
        Lp = tb.qs.numel()
        self._C.ntt_limbs(x.view(-1, Lp, self.n), tb.w, tb.w_shoup, tb.qs, Lp)
        return x

    def galois_lift(self, c: torch.Tensor, ginv: int,
                    tb: "LevelTables") -> torch.Tensor:
        """c [..., l, n] coefficient-domain digits -> sigma_g(c) lifted into
        the l+1 limbs of `tb`: [..., l, l+1, n]. One launch."""
        return self._C.galois_lift(c.contiguous(), int(ginv), tb.qs,
                                   tb.ratio_words)

    def galois_perm_add(self, ct: torch.Tensor, ks0: torch.Tensor,
                        ks1: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
        """(ct[.., 0][perm] + ks0, ks1) assembled as [..., 2, l, n], c0 read
        in place. One launch."""
        return self._C.galois_perm_add(ct.contiguous(), ks0.contiguous(),
                                       ks1.contiguous(), perm, self.qs)

    # ----- hoisted rotations + linear transform (rotate_many, linear.py) -----
    def ks_inner_hoisted(self, dig: torch.Tensor, keys: torch.Tensor,
                         perm: torch.Tensor, tb: "LevelTables"):
        """dig [R, l, l+1, n] (no automorphism) x keys [G, l, 2, l+1, n]
        under the NTT-domain permutations perm [G, n] -> (acc0, acc1), each
        [G, R, l+1, n]. One launch for all G elements."""
        return self._C.ks_inner_hoisted(dig, keys, perm, tb.qs, tb.ratio_words)

    def galois_perm_add_many(self, ct: torch.Tensor, ks0: torch.Tensor,
                             ks1: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
        """ct [R, 2, l, n], ks0 / ks1 [G, R, l, n], perm [G, n] -> the G
        rotated ciphertexts [G, R, 2, l, n]. One launch."""
        return self._C.galois_perm_add_many(ct.contiguous(), ks0.contiguous(),
                                            ks1.contiguous(), perm, self.qs)

    def lt_inner(self, dig: torch.Tensor, keys: torch.Tensor,
                 perm: torch.Tensor, pt: torch.Tensor, tb: "LevelTables"):
        """ks_inner_hoisted weighted by the diagonals pt [G, l+1, n] and
        summed over G -> (acc0, acc1), each [R, l+1, n]. One launch."""
        return self._C.lt_inner(dig, keys, perm, pt, tb.qs, tb.ratio_words)

    def lt_finish(self, ct: torch.Tensor, ks0: torch.Tensor, ks1: torch.Tensor,
                  pt: torch.Tensor, perm: torch.Tensor, z0: int) -> torch.Tensor:
        """(ks0 + sum_g pt_g * c0[perm_g], ks1 + pt_z0 * c1) as [R, 2, l, n];
        pt [G, l, n], z0 the step-0 diagonal's index or -1. One launch."""
        return self._C.lt_finish(ct.contiguous(), ks0.contiguous(),
                                 ks1.contiguous(), pt, perm, int(z0), self.qs,
                                 self.ratio_words)


@dataclass
class LevelTables:
    """Device tables of the l+1 limbs {q_0..q_{l-1}, P} of one level."""
    idx: torch.Tensor          # int64 [l+1] rows of the full tables
    w: torch.Tensor            # [l+1, n]
    w_shoup: torch.Tensor
    qs: torch.Tensor           # [l+1]
    ratio_words: torch.Tensor  # [l+1, 2]
    pinv: torch.Tensor         # [l] P^-1 mod q_i
    pinv_shoup: torch.Tensor


@dataclass
class GaloisTables:
    """Index tables of one Galois element g (sigma_g: a(X) -> a(X^g))."""
    g: int
    ginv: int                  # g^-1 mod 2n
    perm: torch.Tensor         # int64 [n]: NTT domain, out[k] = in[perm[k]]
    perm32: torch.Tensor       # int32 copy for the HIP kernel
    src: torch.Tensor          # int64 [n]: coefficient domain source index
    neg: torch.Tensor          # bool [n]: source enters negated


# ---------------------------------------------------------------------------
# Data containers
# ---------------------------------------------------------------------------

@dataclass
class Plaintext:
    data: torch.Tensor  # int64 [..., L, n], NTT form
    scale: float


@dataclass
class Ciphertext:
    """One CKKS ciphertext: data int64 [2, L, n] (c0, c1), NTT form."""
    data: torch.Tensor
    scale: float

    @property
    def level(self) -> int:
        return self.data.shape[-2]

    def clone(self) -> "Ciphertext":
        return Ciphertext(self.data.clone(), self.scale)


@dataclass
class CtxtTensor:
    """Batched ciphertexts for one flat weight vector: int64 [B, 2, L, n]."""
    data: torch.Tensor
    scale: float
    count: int  # number of packed real values
    # "real": ciphertext b holds values [b*slots, (b+1)*slots) in its real
    # parts; "complex": values [b*n, b*n + slots) in the real parts and
    # [b*n + slots, (b+1)*n) in the imaginary parts of the same slots
    packing: str = "real"

    @property
    def level(self) -> int:
        return self.data.shape[-2]


@dataclass
class KeyPair:
    sk: torch.Tensor          # int64 [L, n] NTT form (threshold mode: one
                              # party's share, or None where none is held)
    pk: torch.Tensor          # int64 [2, L, n] NTT form: (b, a)
    relin: Optional[torch.Tensor] = None  # [dnum, 2, L, n] later
    galois: Optional[dict] = None  # Galois element -> key [L, 2, L+1, n]


@dataclass
class KeyShare:
    """One party's part of an n-of-n additive threshold key: the secret is
    s = sum_i s_i, never assembled anywhere; b = sum_i b_i is public."""
    sk_share: torch.Tensor    # int64 [L, n] NTT form, stays with the party
    b_share: torch.Tensor     # int64 [L, n] NTT form: -(a*s_i + e_i) mod q


# Smudging-noise width accepted by partial decryption: 2^48 keeps the noise
# magnitude exact in int64 / f64 with room for the 60-bit limb arithmetic.
MAX_SMUDGE_BITS = 48


def check_smudge_bits(smudge_bits: int) -> int:
    if not (isinstance(smudge_bits, int) and 0 <= smudge_bits <= MAX_SMUDGE_BITS):
        raise ValueError(
            f"smudge_bits must be an int in [0, {MAX_SMUDGE_BITS}], "
            f"got {smudge_bits!r}")
    return smudge_bits


# ---------------------------------------------------------------------------
# Context
# ---------------------------------------------------------------------------

class CKKSContext:
    def __init__(self, cfg: HEConfig, device: str = "cpu"):
        self.cfg = cfg
        self.n = cfg.m
        self.slots = cfg.m // 2
        # slot packing of encrypt_tensor and the real values one of its
        # ciphertexts carries: slots, or n under "complex"
        self.packing = cfg.packing
        self.values_per_ct = cfg.values_per_ct
        # chain primes + ONE special prime for hybrid key-switching (the
        # relinearization path, configs #3/#5); special prime is never part
        # of a ciphertext level, only of relin keys.
        if not cfg.q_bits:
            raise ValueError("q_bits must name at least one chain prime "
                             "(L >= 1); an empty chain cannot encrypt")
        allp = gen_prime_chain(self.n, tuple(cfg.q_bits) + (60,))
        self.primes: List[int] = allp[:-1]
        self.special: int = allp[-1]
        self.all_primes: List[int] = allp
        self.L = len(self.primes)
        self.scale = float(2 ** cfg.scale_bits)
        self.encoder = Encoder(self.n)
        self.device = torch.device(device)
        if self.device.type == "cuda":
            self.backend = GpuBackend(self.all_primes, self.n, self.device)
        else:
            self.backend = CpuBackend(self.all_primes, self.n)
        self._cpu_rng = np.random.default_rng(cfg.seed)
        # security check against the HE standard (the reference passes
        # sec=128 to Pyfhel, FLPyfhelin.py:332; here it is verified):
        # total modulus = chain + special prime
        from .primes import max_logqp_128
        total_bits = sum(q.bit_length() for q in self.all_primes)
        limit = max_logqp_128(self.n)
        self.secure_128 = total_bits <= limit
        if cfg.sec >= 128 and not self.secure_128 and self.n >= 1024:
            import warnings
            warnings.warn(
                f"CKKS parameters (n={self.n}, logQP={total_bits}) exceed the "
                f"HE-standard 128-bit bound ({limit}); reduce q_bits or raise m",
                stacklevel=2)

    def reseed(self, salt: int) -> None:
        """Re-seed encryption randomness (e.g. per FL rank) after a shared-seed
        keygen, so ciphertext noise is independent across clients."""
        seed = None if self.cfg.seed is None else self.cfg.seed + 1000003 * (salt + 1)
        self._cpu_rng = np.random.default_rng(seed)
        if self.device.type == "cuda":
            g = torch.Generator(device=self.device)
            if seed is not None:
                g.manual_seed(seed)
            self._gpu_gen = g

    @property
    def gpu_gen(self):
        if getattr(self, "_gpu_gen", None) is None:
            g = torch.Generator(device=self.device)
            if self.cfg.seed is not None:
                g.manual_seed(self.cfg.seed)
            self._gpu_gen = g
        return self._gpu_gen

    # ----- helpers -----
    def _q(self, limb: int) -> int:
        return self.all_primes[limb]  # index L = the special prime

    def _modadd(self, a: torch.Tensor, b: torch.Tensor, limbs: Sequence[int]) -> torch.Tensor:
        if self.device.type == "cuda" and list(limbs) == list(range(len(limbs))):
            # fused per-limb HIP kernel (inputs are valid residues < q)
            return self.backend.modadd_limbs(a, b)
        qs = torch.tensor([self._q(i) for i in limbs], dtype=torch.int64,
                          device=a.device)
        shape = [1] * a.dim()
        shape[-2] = len(limbs)
        return torch.remainder(a + b, qs.view(shape))

    def _modsub(self, a: torch.Tensor, b: torch.Tensor, limbs: Sequence[int]) -> torch.Tensor:
        if self.device.type == "cuda" and list(limbs) == list(range(len(limbs))):
            return self.backend.modsub_limbs(a, b)
        qs = torch.tensor([self._q(i) for i in limbs], dtype=torch.int64,
                          device=a.device)
        shape = [1] * a.dim()
        shape[-2] = len(limbs)
        return torch.remainder(a - b, qs.view(shape))

    # ----- sampling (coefficient domain) -----
    # Keygen always samples on the host RNG (deterministic across CPU/GPU
    # contexts with the same seed — all FL ranks must derive the SAME keys).
    # Per-message encryption noise samples on the DEVICE RNG when on GPU:
    # host sampling of u/e0/e1 for a packed weight tensor costs tens of ms
    # of numpy + transfer, device sampling is microseconds.
    def _sample_ternary(self, shape, host: bool = False, rng=None) -> torch.Tensor:
        # {-1, 0, 1} uniform (hamming-weight variant not needed at these n)
        if not host and self.device.type == "cuda":
            return torch.randint(-1, 2, tuple(shape), generator=self.gpu_gen,
                                 device=self.device, dtype=torch.int64)
        rng = self._cpu_rng if rng is None else rng
        v = torch.from_numpy(rng.integers(-1, 2, size=shape))
        return v.to(torch.int64)

    def _sample_err(self, shape, eta: int = 21, host: bool = False,
                    rng=None) -> torch.Tensor:
        # centered binomial, sigma = sqrt(eta/2) ~= 3.24 (SEAL sigma 3.2)
        if not host and self.device.type == "cuda":
            # one uniform 64-bit draw per coefficient; the HIP kernel takes
            # popcount(bits[0:21]) - popcount(bits[21:42])
            bits = torch.randint(-(2 ** 63), 2 ** 63 - 1, tuple(shape),
                                 generator=self.gpu_gen, device=self.device,
                                 dtype=torch.int64)
            return self.backend._C.cbd21(bits)
        rng = self._cpu_rng if rng is None else rng
        b = rng.integers(0, 2, size=(eta,) + tuple(shape)).sum(axis=0)
        b2 = rng.integers(0, 2, size=(eta,) + tuple(shape)).sum(axis=0)
        return torch.from_numpy(b - b2).to(torch.int64)

    def _sample_uniform(self, shape_limbs) -> torch.Tensor:
        """Uniform in [0, q_i) per limb, NTT domain. shape_limbs: [..., L, n]."""
        outs = []
        for i in range(shape_limbs[-2]):
            hi = self._q(i)
            outs.append(torch.from_numpy(
                self._cpu_rng.integers(0, hi, size=shape_limbs[:-2] + (shape_limbs[-1],),
                                       dtype=np.int64)))
        return torch.stack(outs, dim=-2)

    def _to_rns_ntt(self, coeffs: torch.Tensor, nlimbs: Optional[int] = None) -> torch.Tensor:
        """Small centered int64 coeffs [..., n] -> NTT-form RNS [..., L, n]."""
        nlimbs = self.L if nlimbs is None else nlimbs
        if self.device.type == "cuda":
            rem = self.backend.bcast_center_mod(coeffs.to(self.device), 0,
                                                nlimbs)
            return self.backend.ntt_all(rem)
        out = []
        for i in range(nlimbs):
            q = self._q(i)
            ci = torch.remainder(coeffs, q).to(self.device)
            out.append(self.backend.ntt(ci, i))
        return torch.stack(out, dim=-2)

    # ----- keys -----
    def keygen(self) -> KeyPair:
        n = self.n
        s = self._sample_ternary((n,), host=True)
        e = self._sample_err((n,), host=True)
        sk = self._to_rns_ntt(s)                       # [L, n]
        ehat = self._to_rns_ntt(e)
        a = self._sample_uniform((self.L, n)).to(self.device)   # NTT-domain uniform
        b = torch.empty_like(a)
        for i in range(self.L):
            as_ = self.backend.modmul(a[i], sk[i], i)
            b[i] = torch.remainder(-(as_ + ehat[i]), self._q(i))
        pk = torch.stack([b, a])                       # [2, L, n]
        return KeyPair(sk=sk, pk=pk)

    # ----- n-of-n threshold keys (protocol: hefl/fl/secure.py) -----
    def sample_crp(self) -> torch.Tensor:
        """Common random polynomial a: uniform [L, n], NTT domain. Public;
        one party samples it and every party uses the same one."""
        return self._sample_uniform((self.L, self.n)).to(self.device)

    def _party_rng(self, party: int):
        """Per-party host stream for key shares. keygen's shared-seed stream
        is identical on every rank when cfg.seed is set — shares drawn from
        it would all be the same s_i."""
        if self.cfg.seed is None:
            return np.random.default_rng()
        return np.random.default_rng([int(self.cfg.seed), 0x7368, int(party)])

    def keygen_share(self, a: torch.Tensor, party: int) -> KeyShare:
        """Party `party`'s share under the common polynomial a:
        s_i ternary, e_i error (keygen's distributions),
        b_i = -(a*s_i + e_i) mod q."""
        if party < 0:
            raise ValueError(f"party index must be >= 0, got {party}")
        n = self.n
        rng = self._party_rng(party)
        s = self._sample_ternary((n,), host=True, rng=rng)
        e = self._sample_err((n,), host=True, rng=rng)
        sk = self._to_rns_ntt(s)                       # [L, n]
        ehat = self._to_rns_ntt(e)
        a = a.to(self.device)
        b = torch.empty_like(a)
        for i in range(self.L):
            as_ = self.backend.modmul(a[i], sk[i], i)
            b[i] = torch.remainder(-(as_ + ehat[i]), self._q(i))
        return KeyShare(sk_share=sk, b_share=b)

    def combine_pk(self, b_sum_lazy: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        """Collective public key (b, a) from the lazy int64 SUM of <= 8
        parties' b_i (8 residues < 2^60 cannot overflow)."""
        b = self._modreduce_(b_sum_lazy.to(self.device).clone())
        return torch.stack([b, a.to(self.device)])     # [2, L, n]

    # ----- encode / decode -----
    def encode(self, vals: np.ndarray, nlimbs: Optional[int] = None,
               scale: Optional[float] = None) -> Plaintext:
        """vals: real or complex [..., k<=slots] -> NTT-form RNS plaintext.
        A complex input fills both parts of each slot (on the GPU its parts
        are taken as fp32, the packed kernel's input format)."""
        scale = self.scale if scale is None else scale
        nlimbs = self.L if nlimbs is None else nlimbs
        cplx = (vals.is_complex() if torch.is_tensor(vals)
                else np.iscomplexobj(vals))
        if self.device.type == "cuda":
            # full-device path: special FFT + rounding on the GPU, then one
            # fused multi-limb remainder + NTT
            if cplx:
                vt = vals if torch.is_tensor(vals) else torch.from_numpy(
                    np.asarray(vals, dtype=np.complex128))
                ct = self.encoder.encode_complex_torch(vt.to(self.device), scale)
                return Plaintext(self._to_rns_ntt(ct, nlimbs), scale)
            vt = (vals if torch.is_tensor(vals)
                  else torch.from_numpy(np.asarray(vals, dtype=np.float64)))
            ct = self.encoder.encode_torch(vt.to(self.device), scale)
            return Plaintext(self._to_rns_ntt(ct, nlimbs), scale)
        if cplx:
            if torch.is_tensor(vals):
                vals = vals.cpu().numpy()
            coeffs = self.encoder.encode_complex(vals, scale)
        else:
            coeffs = self.encoder.encode(np.asarray(vals, dtype=np.float64),
                                         scale)
        out = []
        if coeffs.dtype == np.int64:
            # fast path: one upload, per-limb remainder + NTT on device
            ct = torch.from_numpy(coeffs).to(self.device)
            for i in range(nlimbs):
                out.append(self.backend.ntt(torch.remainder(ct, self._q(i)), i))
        else:
            for i in range(nlimbs):
                q = self._q(i)
                ci = np.mod(coeffs, q)  # object -> [0, q)
                ci_t = torch.from_numpy(ci.astype(np.int64)).to(self.device)
                out.append(self.backend.ntt(ci_t, i))
        return Plaintext(torch.stack(out, dim=-2), scale)

    def _centered_coeffs(self, data: torch.Tensor):
        """NTT-form plaintext [..., L', n] -> its centered integer
        coefficients [..., n], by the three branches of decode: an int64
        tensor on the context device where limb 0 alone determines them,
        else a numpy object array (big-int CRT). Only the complex paths come
        through here; decode keeps its own statements for real values."""
        nlimbs = data.shape[-2]
        if nlimbs == 1:
            # fast path (the FedAvg pipeline decrypts at level 1): center on
            # device, f64 is exact for plaintext magnitudes << 2^53
            q = self._q(0)
            c = self.backend.ntt(data[..., 0, :], 0, inverse=True)
            return torch.where(c > q // 2, c - q, c)
        # multi-limb fast path: when the plaintext magnitude is << q0/2 (true
        # for any decode of real-valued weights at scale <= 2^45), the
        # centered limb-0 residue IS the integer value — checked against
        # limb 1 on a sample, falling back to exact big-int CRT on mismatch.
        q0 = self._q(0)
        c0 = self.backend.ntt(data[..., 0, :], 0, inverse=True)
        cent0 = torch.where(c0 > q0 // 2, c0 - q0, c0)
        if cent0.abs().max().item() < q0 // 4:
            q1 = self._q(1)
            c1 = self.backend.ntt(data[..., 1, :], 1, inverse=True)
            cent1 = torch.where(c1 > q1 // 2, c1 - q1, c1)
            if torch.equal(torch.remainder(cent0, q1), torch.remainder(cent1, q1)):
                return cent0
        # exact big-int CRT path (plaintext too large for limb-0 shortcut)
        coeff_limbs = []
        for i in range(nlimbs):
            c = self.backend.ntt(data[..., i, :], i, inverse=True)
            coeff_limbs.append(c.cpu().numpy().astype(object))
        qs = [self._q(i) for i in range(nlimbs)]
        Q = math.prod(qs)
        x = 0
        for i, q in enumerate(qs):
            Qi = Q // q
            hi = pow(Qi % q, -1, q)
            x = x + coeff_limbs[i] * ((Qi * hi) % Q)
        x = np.mod(x, Q)
        return np.where(x > Q // 2, x - Q, x)

    def _decode_complex(self, pt: Plaintext, k: int):
        """decode's three branches (one limb, limb-0 shortcut, big-int CRT)
        for complex slot values."""
        cent = self._centered_coeffs(pt.data)
        if torch.is_tensor(cent):
            if self.device.type == "cuda":
                return self.encoder.decode_complex_torch(cent, pt.scale, k)
            cent = cent.cpu().numpy()
        return self.encoder.decode_complex(cent, pt.scale, k)

    def decode(self, pt: Plaintext, k: int, complex: bool = False):
        """First k slot values of a plaintext: their real parts, or with
        complex=True the complex values. A tensor on a GPU context (fp32 /
        complex64), a numpy array on the CPU."""
        if complex:
            return self._decode_complex(pt, k)
        data = pt.data
        nlimbs = data.shape[-2]
        if nlimbs == 1:
            # fast path (the FedAvg pipeline decrypts at level 1): center on
            # device, f64 is exact for plaintext magnitudes << 2^53
            q = self._q(0)
            c = self.backend.ntt(data[..., 0, :], 0, inverse=True)
            cent = torch.where(c > q // 2, c - q, c)
            if self.device.type == "cuda":
                return self.encoder.decode_torch(cent, pt.scale, k)
            return self.encoder.decode(cent.cpu().numpy(), pt.scale, k)
        # multi-limb fast path: when the plaintext magnitude is << q0/2 (true
        # for any decode of real-valued weights at scale <= 2^45), the
        # centered limb-0 residue IS the integer value — checked against
        # limb 1 on a sample, falling back to exact big-int CRT on mismatch.
        q0 = self._q(0)
        c0 = self.backend.ntt(data[..., 0, :], 0, inverse=True)
        cent0 = torch.where(c0 > q0 // 2, c0 - q0, c0)
        if cent0.abs().max().item() < q0 // 4:
            q1 = self._q(1)
            c1 = self.backend.ntt(data[..., 1, :], 1, inverse=True)
            cent1 = torch.where(c1 > q1 // 2, c1 - q1, c1)
            if torch.equal(torch.remainder(cent0, q1), torch.remainder(cent1, q1)):
                if self.device.type == "cuda":
                    return self.encoder.decode_torch(cent0, pt.scale, k)
                return self.encoder.decode(cent0.cpu().numpy(), pt.scale, k)
        # exact big-int CRT path (plaintext too large for limb-0 shortcut)
        coeff_limbs = []
        for i in range(nlimbs):
            c = self.backend.ntt(data[..., i, :], i, inverse=True)
            coeff_limbs.append(c.cpu().numpy().astype(object))
        qs = [self._q(i) for i in range(nlimbs)]
        Q = math.prod(qs)
        x = 0
        for i, q in enumerate(qs):
            Qi = Q // q
            hi = pow(Qi % q, -1, q)
            x = x + coeff_limbs[i] * ((Qi * hi) % Q)
        x = np.mod(x, Q)
        centered = np.where(x > Q // 2, x - Q, x)
        return self.encoder.decode(centered, pt.scale, k)

    # ----- encrypt / decrypt (single ct or batched [..., 2, L, n]) -----
    def encrypt(self, pt: Plaintext, pk: torch.Tensor) -> Ciphertext:
        data = self._encrypt_data(pt.data, pk)
        return Ciphertext(data, pt.scale)

    def _encrypt_data(self, ptdata: torch.Tensor, pk: torch.Tensor) -> torch.Tensor:
        lead = ptdata.shape[:-2]
        nlimbs = ptdata.shape[-2]
        n = self.n
        u = self._to_rns_ntt(self._sample_ternary(lead + (n,)), nlimbs)
        e0 = self._to_rns_ntt(self._sample_err(lead + (n,)), nlimbs)
        e1 = self._to_rns_ntt(self._sample_err(lead + (n,)), nlimbs)
        if self.device.type == "cuda":
            bu = self.backend.modmul_limbs(u, pk[0, :nlimbs])
            au = self.backend.modmul_limbs(u, pk[1, :nlimbs])
            c0 = self.backend.modadd3_limbs(bu, e0, ptdata.contiguous())
            c1 = self.backend.modadd_limbs(au, e1)
            return torch.stack([c0, c1], dim=-3)
        c0 = torch.empty_like(ptdata)
        c1 = torch.empty_like(ptdata)
        for i in range(nlimbs):
            q = self._q(i)
            bu = self.backend.modmul(pk[0, i].expand(lead + (n,)).contiguous(),
                                     u[..., i, :], i)
            au = self.backend.modmul(pk[1, i].expand(lead + (n,)).contiguous(),
                                     u[..., i, :], i)
            c0[..., i, :] = torch.remainder(bu + e0[..., i, :] + ptdata[..., i, :], q)
            c1[..., i, :] = torch.remainder(au + e1[..., i, :], q)
        return torch.stack([c0, c1], dim=-3)  # [..., 2, L, n]

    def decrypt(self, ct: Ciphertext, sk: torch.Tensor) -> Plaintext:
        return Plaintext(self._decrypt_data(ct.data, sk), ct.scale)

    def _decrypt_data(self, ctdata: torch.Tensor, sk: torch.Tensor) -> torch.Tensor:
        nlimbs = ctdata.shape[-2]
        c0 = ctdata[..., 0, :, :]
        c1 = ctdata[..., 1, :, :]
        if self.device.type == "cuda":
            cs = self.backend.modmul_limbs(c1.contiguous(), sk[:nlimbs])
            return self.backend.modadd_limbs(c0.contiguous(), cs)
        out = torch.empty_like(c0)
        for i in range(nlimbs):
            cs = self.backend.modmul(c1[..., i, :], sk[i].expand_as(c1[..., i, :]).contiguous(), i)
            out[..., i, :] = torch.remainder(c0[..., i, :] + cs, self._q(i))
        return out

    def _draw_bits(self, shape) -> torch.Tensor:
        """One uniform 64-bit draw per element from this context's (per-rank
        reseeded) encryption stream — the same feed cbd21 gets."""
        if self.device.type == "cuda":
            return torch.randint(-(2 ** 63), 2 ** 63 - 1, tuple(shape),
                                 generator=self.gpu_gen, device=self.device,
                                 dtype=torch.int64)
        return torch.from_numpy(self._cpu_rng.integers(
            -(2 ** 63), 2 ** 63, size=tuple(shape), dtype=np.int64))

    def partial_decrypt_data(self, ctdata: torch.Tensor, sk_share: torch.Tensor,
                             smudge_bits: int, lead: bool,
                             bits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One party's decryption share of ct data [..., 2, Lc, n]:

            h_i = c1 * s_i + NTT(e'_i) (+ c0 for the lead party)  mod q

        with e'_i fresh smudging noise, uniform in [-2^smudge_bits,
        2^smudge_bits) per coefficient: e' = (bits & (2^(sb+1)-1)) - 2^sb.
        `bits` ([..., n] int64) injects the raw 64-bit draws — tests use it to
        compare the CPU and GPU paths bit for bit; by default they are drawn
        anew on every call. Returns [..., Lc, n]; the SUM of all parties'
        shares, reduced mod q, is the plaintext (combine_shares_tensor)."""
        sb = check_smudge_bits(smudge_bits)
        nlimbs = ctdata.shape[-2]
        lead_shape = tuple(ctdata.shape[:-3])
        if bits is None:
            bits = self._draw_bits(lead_shape + (self.n,))
        elif tuple(bits.shape) != lead_shape + (self.n,):
            raise ValueError(f"bits must have shape {lead_shape + (self.n,)}, "
                             f"got {tuple(bits.shape)}")
        if self.device.type == "cuda":
            be = self.backend
            e_hat = be.ntt_all_(be.uniform_center_rns(
                bits.to(self.device), sb, nlimbs))
            return be.pdec_share(ctdata, sk_share, e_hat, lead)
        e = (bits & ((1 << (sb + 1)) - 1)) - (1 << sb)
        e_hat = self._to_rns_ntt(e, nlimbs)
        c0 = ctdata[..., 0, :, :]
        c1 = ctdata[..., 1, :, :]
        out = torch.empty_like(c1)
        for i in range(nlimbs):
            cs = self.backend.modmul(
                c1[..., i, :], sk_share[i].expand_as(c1[..., i, :]).contiguous(), i)
            h = cs + e_hat[..., i, :]
            if lead:
                h = h + c0[..., i, :]
            out[..., i, :] = torch.remainder(h, self._q(i))
        return out

    # ----- homomorphic ops -----
    @staticmethod
    def _check_add_scales(sa: float, sb: float) -> None:
        # adding ciphertexts at different scales silently decodes to garbage
        # (the slots are Delta-scaled integers; sums only make sense at one
        # Delta) — fail loudly instead
        if abs(sa - sb) > 1e-9 * max(sa, sb):
            raise ValueError(
                f"ciphertext scales differ ({sa} vs {sb}); rescale or "
                f"re-encode one operand before adding")

    def add(self, a: Ciphertext, b: Ciphertext) -> Ciphertext:
        assert a.level == b.level
        self._check_add_scales(a.scale, b.scale)
        limbs = list(range(a.level))
        return Ciphertext(self._modadd(a.data, b.data, limbs), max(a.scale, b.scale))

    def mul_scalar_data(self, data: torch.Tensor, x: float,
                        scale: Optional[float] = None) -> torch.Tensor:
        """Multiply ct data [..., 2, L, n] by encoded scalar round(x * Delta)."""
        delta = self.scale if scale is None else scale
        sc = int(round(x * delta))
        nlimbs = data.shape[-2]
        if self.device.type == "cuda":
            return self.backend.modmul_scalar_limbs(
                data.contiguous(), [sc] * nlimbs)
        out = torch.empty_like(data)
        for i in range(nlimbs):
            q = self._q(i)
            out[..., i, :] = self.backend.modmul_scalar(data[..., i, :], sc % q, i)
        return out

    def mul_scalar(self, ct: Ciphertext, x: float) -> Ciphertext:
        return Ciphertext(self.mul_scalar_data(ct.data, x), ct.scale * self.scale)

    def mul_plain(self, ct: Ciphertext, pt: Plaintext) -> Ciphertext:
        nlimbs = ct.level
        out = torch.empty_like(ct.data)
        for i in range(nlimbs):
            for c in range(2):
                out[..., c, i, :] = self.backend.modmul(
                    ct.data[..., c, i, :], pt.data[..., i, :], i)
        return Ciphertext(out, ct.scale * pt.scale)

    def rescale_data(self, data: torch.Tensor) -> torch.Tensor:
        """Drop the last limb: exact RNS division by q_last with rounding.
        data: [..., 2, L, n] -> [..., 2, L-1, n]."""
        nlimbs = data.shape[-2]
        assert nlimbs >= 2, "cannot rescale at level 1"
        last = nlimbs - 1
        qL = self._q(last)
        qL_half = qL // 2
        if self.device.type == "cuda":
            # fully fused: INTT of the last limb, one center+broadcast-reduce
            # launch, one fused NTT set, one strided-slice modsub (no
            # materialized slice), one scalar-limbs multiply — zero
            # at::native kernels on this path
            cl = self.backend.ntt(data[..., last, :], last,
                                  inverse=True)
            r = self.backend.bcast_center_mod(cl, qL, last)
            r_ntt = self.backend.ntt_all(r)
            diff = self.backend.modsub_limbs(data.contiguous(), r_ntt, last)
            inv = [pow(qL % self._q(i), -1, self._q(i)) for i in range(last)]
            return self.backend.modmul_scalar_limbs(diff, inv)
        # coefficient-domain last limb, centered for round-to-nearest
        cl = self.backend.ntt(data[..., last, :], last,
                              inverse=True)
        cl_c = torch.where(cl > qL_half, cl - qL, cl)
        out = data[..., :last, :].clone()
        for i in range(last):
            q = self._q(i)
            r = torch.remainder(cl_c, q)
            r_ntt = self.backend.ntt(r, i)
            diff = torch.remainder(out[..., i, :] - r_ntt, q)
            inv_qL = pow(qL % q, -1, q)
            out[..., i, :] = self.backend.modmul_scalar(diff, inv_qL, i)
        return out

    def rescale(self, ct: Ciphertext) -> Ciphertext:
        new = self.rescale_data(ct.data)
        return Ciphertext(new, ct.scale / float(self._q(ct.level - 1)))

    # ----- batched tensor API (flat weight vectors) -----
    def encrypt_tensor(self, vec: torch.Tensor, pk: torch.Tensor) -> CtxtTensor:
        """Pack a flat fp32 vector into ceil(len / values_per_ct) ciphertexts:
        one value per slot, or with cfg.packing == "complex" two (slot j of
        ciphertext b carries vec[b*n + j] + i*vec[b*n + slots + j]). The
        real-packing statements below, and those of decrypt_tensor and decode,
        are kept as they were before the option existed: the host-side
        sequence between training rounds was once seen not to be neutral for
        the training's atomics-order noise (PERFORMANCE.md)."""
        count = vec.numel()
        if self.packing == "complex":
            if count < 1:
                raise ValueError("cannot encrypt an empty vector")
            if self.device.type == "cuda":
                # one HIP launch set straight from the fp32 weights: no f64
                # staging buffer, no slice copy, no cast
                coeffs = self.encoder.encode_packed_torch(
                    vec.detach().reshape(-1).to(self.device, torch.float32),
                    self.scale)
                pt = Plaintext(self._to_rns_ntt(coeffs), self.scale)
            else:
                pt = self.encode(self.encoder.pack_complex(
                    vec.detach().float().cpu().numpy()))
            data = self._encrypt_data(pt.data, pk)
            return CtxtTensor(data, pt.scale, count, "complex")
        B = (count + self.slots - 1) // self.slots
        if self.device.type == "cuda":
            buf = torch.zeros(B * self.slots, dtype=torch.float64,
                              device=self.device)
            buf[:count] = vec.detach().double().reshape(-1).to(self.device)
            pt = self.encode(buf.reshape(B, self.slots))
        else:
            buf = np.zeros((B, self.slots), dtype=np.float64)
            buf.reshape(-1)[:count] = vec.detach().float().cpu().numpy().reshape(-1)
            pt = self.encode(buf)                 # [B, L, n]
        data = self._encrypt_data(pt.data, pk)    # [B, 2, L, n]
        return CtxtTensor(data, pt.scale, count)

    def decrypt_tensor(self, ct: CtxtTensor, sk: torch.Tensor) -> torch.Tensor:
        pt = self._decrypt_data(ct.data, sk)      # [B, L, n]
        if ct.packing != "real":
            return self._decode_tensor(pt, ct.scale, ct.count, ct.packing)
        vals = self.decode(Plaintext(pt, ct.scale), self.slots)  # [B, slots]
        if torch.is_tensor(vals):
            return vals.reshape(-1)[:ct.count].to(torch.float32)
        flat = torch.from_numpy(np.ascontiguousarray(vals.reshape(-1)[:ct.count]))
        return flat.to(torch.float32)

    def _decode_tensor(self, pt: torch.Tensor, scale: float, count: int,
                       packing: str = "real") -> torch.Tensor:
        if packing != "real":
            if packing != "complex":
                raise ValueError(f"unknown packing {packing!r}")
            return self._decode_packed(pt, scale, count)
        vals = self.decode(Plaintext(pt, scale), self.slots)  # [B, slots]
        if torch.is_tensor(vals):
            return vals.reshape(-1)[:count].to(torch.float32)
        flat = torch.from_numpy(np.ascontiguousarray(vals.reshape(-1)[:count]))
        return flat.to(torch.float32)

    def _decode_packed(self, pt: torch.Tensor, scale: float,
                       count: int) -> torch.Tensor:
        """Complex-packed plaintexts [B, L', n] -> the fp32 vector [count]."""
        if count > pt.shape[0] * self.n:
            raise ValueError(f"{pt.shape[0]} ciphertexts hold at most "
                             f"{pt.shape[0] * self.n} values, count is {count}")
        cent = self._centered_coeffs(pt)
        if torch.is_tensor(cent):
            return self.encoder.decode_packed_torch(cent, scale, count)
        z = self.encoder.decode_complex(cent, scale, self.slots)
        flat = self.encoder.unpack_complex(z, count)
        return torch.from_numpy(np.ascontiguousarray(flat)).to(torch.float32)

    def partial_decrypt_tensor(self, ct: CtxtTensor, sk_share: torch.Tensor,
                               smudge_bits: int, lead: bool,
                               bits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """This party's decryption share of a CtxtTensor: int64 [B, Lc, n],
        ready for a lazy int64 SUM across parties."""
        return self.partial_decrypt_data(ct.data, sk_share, smudge_bits, lead,
                                         bits=bits)

    def combine_shares_tensor(self, share_sum_lazy: torch.Tensor, scale: float,
                              count: int, *, packing: str = "real") -> torch.Tensor:
        """Lazy int64 SUM of <= 8 parties' shares [B, Lc, n] -> fp32 vector.
        Each share is < q < 2^60, so the sum is < 2^63 and the modreduce
        conditional-subtract chain applies. Reduces the sum in place.
        `packing` is that of the ciphertext the shares were taken of."""
        pt = self._modreduce_(share_sum_lazy)
        return self._decode_tensor(pt, scale, count, packing)

    def add_tensor(self, a: CtxtTensor, b: CtxtTensor) -> CtxtTensor:
        assert a.count == b.count and a.level == b.level
        if a.packing != b.packing:
            raise ValueError(
                f"cannot add a {a.packing}-packed and a {b.packing}-packed "
                f"tensor: their slots hold different values")
        self._check_add_scales(a.scale, b.scale)
        limbs = list(range(a.level))
        return CtxtTensor(self._modadd(a.data, b.data, limbs),
                          max(a.scale, b.scale), a.count, a.packing)

    def mul_scalar_tensor(self, ct: CtxtTensor, x: float) -> CtxtTensor:
        return CtxtTensor(self.mul_scalar_data(ct.data, x),
                          ct.scale * self.scale, ct.count, ct.packing)

    def rescale_tensor(self, ct: CtxtTensor) -> CtxtTensor:
        return CtxtTensor(self.rescale_data(ct.data),
                          ct.scale / float(self._q(ct.level - 1)), ct.count,
                          ct.packing)

    # ----- relinearization (ct x ct support; reference intent at
    # FLPyfhelin.py:357-364 gen_rekey — dead code there, real here) -----
    def _sk_extended(self, sk: torch.Tensor) -> torch.Tensor:
        """Recover the ternary secret from sk's limb 0 and re-embed over
        all L+1 limbs (chain + special) for key generation."""
        q0 = self._q(0)
        s = self.backend.ntt(sk[0], 0, inverse=True).cpu()
        s = torch.where(s > q0 // 2, s - q0, s)  # ternary {-1,0,1}
        return self._to_rns_ntt(s, self.L + 1)

    def relin_keygen(self, sk: torch.Tensor) -> torch.Tensor:
        """Hybrid key-switching keys (digits = RNS limbs, one special prime P).

        rlk[d] = (-(a_d*s + e_d) + P*q̃_d*s², a_d) over the L+1 limbs
        {q_0..q_{L-1}, P}. In RNS, P*q̃_d*s² is (P mod q_d)*s² at limb d and
        0 elsewhere (q̃_d ≡ δ_{d,i} mod q_i, P ≡ 0 mod P). Key-switch noise
        shrinks by 1/P at the final mod-down, which is what makes per-limb
        digits sound (classic per-limb BV without P has q_max-sized noise).
        Returns int64 [L, 2, L+1, n] in NTT form.
        """
        L, n = self.L, self.n
        Lp = L + 1
        P = self.special
        sk_ext = self._sk_extended(sk)            # [L+1, n]
        s2 = torch.empty_like(sk_ext)
        for i in range(Lp):
            s2[i] = self.backend.modmul(sk_ext[i], sk_ext[i], i)
        rlk = torch.empty((L, 2, Lp, n), dtype=torch.int64, device=self.device)
        for d in range(L):
            a = self._sample_uniform((Lp, n)).to(self.device)
            e = self._to_rns_ntt(self._sample_err((n,), host=True), Lp)
            for i in range(Lp):
                q = self._q(i)
                b = torch.remainder(-(self.backend.modmul(a[i], sk_ext[i], i)
                                      + e[i]), q)
                if i == d:
                    b = torch.remainder(
                        b + self.backend.modmul_scalar(s2[i], P % q, i), q)
                rlk[d, 0, i] = b
                rlk[d, 1, i] = a[i]
        return rlk

    def _keyswitch(self, d2: torch.Tensor, rlk: torch.Tensor):
        """Key-switch NTT-form d2 [..., L, n] through rlk; returns the pair
        (ks0, ks1) each [..., L, n] to add to (c0, c1).

        GPU path is fully fused: one INTT set over all
        digits, one lift launch, one NTT set, ONE inner-product kernel over
        all digits x limbs, then a fused mod-down — ~12 launches total
        instead of the O(L*(L+1)) per-digit/per-limb Python loop."""
        L = d2.shape[-2]
        Lp = L + 1
        n = self.n
        if self.device.type == "cuda":
            be = self.backend
            c = be.ntt_all(d2, inverse=True)           # digits -> coeff domain
            dig = be.bcast_center_mod(c, 0, Lp)        # [..., L, Lp, n]
            dig = be.ntt_all(dig)                      # NTT over the Lp limbs
            acc0, acc1 = be._C.ks_inner(dig.contiguous(), rlk.contiguous(),
                                        be.qs, be.ratio_words, L, Lp, n)
            P = self.special
            inv = [pow(P % self._q(i), -1, self._q(i)) for i in range(L)]
            outs = []
            for acc in (acc0, acc1):
                cl = be.ntt(acc[..., L, :], L, inverse=True)
                r_ntt = be.ntt_all(be.bcast_center_mod(cl, P, L))
                diff = be.modsub_limbs(acc, r_ntt, L)
                outs.append(be.modmul_scalar_limbs(diff, inv))
            return outs[0], outs[1]
        lead = d2.shape[:-2]
        acc0 = torch.zeros(lead + (Lp, n), dtype=torch.int64, device=d2.device)
        acc1 = torch.zeros_like(acc0)
        for d in range(L):
            # digit d: coefficient-domain residues mod q_d, lifted to every limb
            c = self.backend.ntt(d2[..., d, :], d, inverse=True)
            for i in range(Lp):
                q = self._q(i)
                dig = self.backend.ntt(torch.remainder(c, q), i)
                acc0[..., i, :] = torch.remainder(
                    acc0[..., i, :] + self.backend.modmul(
                        dig, rlk[d, 0, i].expand_as(dig).contiguous(), i), q)
                acc1[..., i, :] = torch.remainder(
                    acc1[..., i, :] + self.backend.modmul(
                        dig, rlk[d, 1, i].expand_as(dig).contiguous(), i), q)
        # mod-down by the special prime P (exact division with rounding,
        # same structure as rescale_data but dropping the special limb)
        P = self.special
        P_half = P // 2
        outs = []
        for acc in (acc0, acc1):
            cl = self.backend.ntt(acc[..., L, :], L, inverse=True)
            cl_c = torch.where(cl > P_half, cl - P, cl)
            out = acc[..., :L, :].clone()
            for i in range(L):
                q = self._q(i)
                r_ntt = self.backend.ntt(torch.remainder(cl_c, q), i)
                diff = torch.remainder(out[..., i, :] - r_ntt, q)
                out[..., i, :] = self.backend.modmul_scalar(
                    diff, pow(P % q, -1, q), i)
            outs.append(out)
        return outs[0], outs[1]

    def mul_ct(self, a: Ciphertext, b: Ciphertext, rlk: torch.Tensor) -> Ciphertext:
        """ct x ct multiply + relinearize (no rescale; call rescale after)."""
        if rlk is None:
            raise ValueError(
                "ct x ct multiply needs relinearization keys — run "
                "relin_keygen(sk) (Pyfhel API: relinKeyGen) first")
        assert a.level == b.level
        L = a.level
        if self.device.type == "cuda":
            # one fused tensor-product launch (d0, d1, d2 together)
            d0, d1, d2 = self.backend._C.ct_mul(
                a.data.contiguous(), b.data.contiguous(), self.backend.qs,
                self.backend.ratio_words, L, self.n)
        else:
            a0, a1 = a.data[..., 0, :, :], a.data[..., 1, :, :]
            b0, b1 = b.data[..., 0, :, :], b.data[..., 1, :, :]
            d0 = torch.empty_like(a0)
            d1 = torch.empty_like(a0)
            d2 = torch.empty_like(a0)
            for i in range(L):
                q = self._q(i)
                d0[..., i, :] = self.backend.modmul(a0[..., i, :], b0[..., i, :], i)
                cross = (self.backend.modmul(a0[..., i, :], b1[..., i, :], i)
                         + self.backend.modmul(a1[..., i, :], b0[..., i, :], i))
                d1[..., i, :] = torch.remainder(cross, q)
                d2[..., i, :] = self.backend.modmul(a1[..., i, :], b1[..., i, :], i)
        ks0, ks1 = self._keyswitch(d2, rlk)
        limbs = list(range(L))
        c0 = self._modadd(d0, ks0, limbs)
        c1 = self._modadd(d1, ks1, limbs)
        return Ciphertext(torch.stack([c0, c1], dim=-3), a.scale * b.scale)

    # ----- slot rotation / conjugation (Galois automorphisms) -----
    # sigma_g: a(X) -> a(X^g). With this encoder's 5^j slot ordering, g = 5^r
    # moves slot (j + r) mod slots into slot j — a LEFT rotation, decoded
    # np.roll(v, -r) — and g = 2n - 1 conjugates every slot. sigma_g(ct)
    # decrypts under sigma_g(s); a key-switch through the Galois key for g
    # (an encryption of P*q~_d*sigma_g(s) per digit d) brings it back under s.
    def galois_element(self, step: Optional[int] = None,
                       conjugate: bool = False) -> int:
        """Galois element of a rotation by `step` slots, or of conjugation."""
        if conjugate:
            if step is not None:
                raise ValueError("pass either a step or conjugate=True, not both")
            return 2 * self.n - 1
        if step is None:
            raise ValueError("galois_element needs a step or conjugate=True")
        return pow(5, int(step) % self.slots, 2 * self.n)

    def _galois_tables(self, g: int) -> GaloisTables:
        """Host-computed index tables of sigma_g, cached on the device."""
        cache = self.__dict__.setdefault("_galois_cache", {})
        if g not in cache:
            n, two_n = self.n, 2 * self.n
            if not (0 < g < two_n and g % 2 == 1):
                raise ValueError(f"Galois element must be odd in (0, {two_n}), got {g}")
            logn = n.bit_length() - 1

            def brv(v):
                r = np.zeros_like(v)
                for b in range(logn):
                    r |= ((v >> b) & 1) << (logn - 1 - b)
                return r

            k = np.arange(n, dtype=np.int64)
            # NTT slot k evaluates at psi^(2*brv(k)+1); sigma_g sends the
            # value at psi^(e*g) to the slot of psi^e
            perm = brv((((2 * brv(k) + 1) * g) % two_n - 1) // 2)
            ginv = pow(g, -1, two_n)
            # coefficient k of sigma_g(a) is +-a_j with j*g = k (mod n)
            e = (k * ginv) % two_n
            dev = self.device
            cache[g] = GaloisTables(
                g=g, ginv=ginv,
                perm=torch.from_numpy(perm).to(dev),
                perm32=torch.from_numpy(perm.astype(np.int32)).to(dev),
                src=torch.from_numpy(e % n).to(dev),
                neg=torch.from_numpy(e >= n).to(dev))
        return cache[g]

    def default_rotation_steps(self) -> List[int]:
        """+-2^k for k = 0 .. log2(slots)-1: every step composes from these
        in at most ~log2(slots)/2 hops (non-adjacent form)."""
        steps = []
        k = 1
        while k < self.slots:
            steps += [k, -k]
            k *= 2
        return steps

    def galois_keygen(self, sk: torch.Tensor,
                      steps: Optional[Iterable[int]] = None,
                      conjugate: bool = False) -> Dict[int, torch.Tensor]:
        """Galois keys {element g: int64 [L, 2, L+1, n]}, one per rotation
        step (default: +-2^k) plus conjugation on request.

        Same shape and distribution as relin_keygen's output; digit d hides
        P*q~_d*sigma_g(s) instead of P*q~_d*s^2 — in RNS (P mod q_d) *
        sigma_g(s) at limb d and nothing elsewhere. Sampled on the host from
        the context's seeded stream like every key, so all ranks and the CPU
        and GPU contexts derive identical keys."""
        if sk is None:
            raise ValueError(
                "galois_keygen needs the secret key; under key_mode="
                "'threshold' no party holds s, so Galois keys are unsupported")
        steps = self.default_rotation_steps() if steps is None else list(steps)
        elements = [self.galois_element(s) for s in steps]
        if conjugate:
            elements.append(self.galois_element(conjugate=True))
        L, n = self.L, self.n
        Lp = L + 1
        P = self.special
        sk_ext = self._sk_extended(sk)            # [L+1, n]
        keys: Dict[int, torch.Tensor] = {}
        for g in elements:
            if g == 1 or g in keys:               # step 0 / duplicate step
                continue
            perm = self._galois_tables(g).perm
            s_g = sk_ext.index_select(-1, perm)   # sigma_g(s), NTT form
            gk = torch.empty((L, 2, Lp, n), dtype=torch.int64,
                             device=self.device)
            for d in range(L):
                a = self._sample_uniform((Lp, n)).to(self.device)
                e = self._to_rns_ntt(self._sample_err((n,), host=True), Lp)
                for i in range(Lp):
                    q = self._q(i)
                    b = torch.remainder(-(self.backend.modmul(a[i], sk_ext[i], i)
                                          + e[i]), q)
                    if i == d:
                        b = torch.remainder(
                            b + self.backend.modmul_scalar(s_g[i], P % q, i), q)
                    gk[d, 0, i] = b
                    gk[d, 1, i] = a[i]
            keys[g] = gk
        return keys

    def _key_at_level(self, key: torch.Tensor, l: int) -> torch.Tensor:
        """Digits 0..l-1 and limbs {0..l-1, L} of a switching key — exact,
        because q~_d = delta_{d,i} holds over any prefix of the chain."""
        if l == self.L:
            return key.contiguous()
        cache = self.__dict__.setdefault("_key_level_cache", {})
        ck = (key.data_ptr(), l)
        hit = cache.get(ck)
        if hit is None or hit[0] is not key:
            idx = torch.tensor(list(range(l)) + [self.L], dtype=torch.int64,
                               device=key.device)
            # the cache entry holds `key` itself so its storage (and with it
            # the data_ptr the entry is filed under) cannot be reused
            hit = (key, key[:l].index_select(2, idx).contiguous())
            cache[ck] = hit
        return hit[1]

    @staticmethod
    def _coeff_automorphism(c: torch.Tensor, q, gt: GaloisTables) -> torch.Tensor:
        """sigma_g on coefficient rows c [..., n] of residues in [0, q) (q an
        int or a tensor broadcasting over c): gather, then negate mod q where
        the source wrapped past X^n. A negated zero stays zero."""
        v = torch.index_select(c, -1, gt.src)
        return torch.where(gt.neg & (v != 0), q - v, v)

    @staticmethod
    def _galois_fused() -> bool:
        """HEFL_GALOIS_FUSED=0 archives the fused kernels behind the path
        composed of torch gather / where / stack (PERFORMANCE.md: slower)."""
        return os.getenv("HEFL_GALOIS_FUSED", "1") != "0"

    def _keyswitch_level(self, x: torch.Tensor, key: torch.Tensor, l: int,
                         g: Optional[int] = None):
        """Level-aware hybrid key-switch of NTT-form x [..., l, n] (l <= L
        chain limbs) through `key` [L, 2, L+1, n]; returns (ks0, ks1), each
        [..., l, n]. Uses digits 0..l-1 of the key over the limbs
        {q_0..q_{l-1}, P}. With g given, switches sigma_g(x) instead — the
        automorphism is applied to the coefficient-domain digits on the way.

        GPU: the launch sequence of _keyswitch on tables gathered at rows
        [0..l-1, L] (GpuBackend.level_tables)."""
        if x.shape[-2] != l or not 1 <= l <= self.L:
            raise ValueError(f"expected [.., {l}, n] with 1 <= l <= {self.L}, "
                             f"got {tuple(x.shape)}")
        if tuple(key.shape) != (self.L, 2, self.L + 1, self.n):
            raise ValueError(
                f"switching key must be [{self.L}, 2, {self.L + 1}, {self.n}], "
                f"got {tuple(key.shape)}")
        n = self.n
        gt = None if g is None else self._galois_tables(g)
        idx = list(range(l)) + [self.L]
        if self.device.type == "cuda":
            be = self.backend
            tb = be.level_tables(l)
            kl = self._key_at_level(key, l)
            c = be.ntt_all(x, inverse=True)            # digits -> coeff domain
            if gt is None:
                dig = be._C.bcast_center_mod(c, 0, tb.qs, tb.ratio_words, l + 1)
            elif self._galois_fused():
                dig = be.galois_lift(c, gt.ginv, tb)
            else:
                c = self._coeff_automorphism(c, be.qs[:l].view(l, 1), gt)
                dig = be._C.bcast_center_mod(c.contiguous(), 0, tb.qs,
                                             tb.ratio_words, l + 1)
            be.ntt_level_(dig, tb)                     # [..., l, l+1, n]
            acc0, acc1 = be._C.ks_inner(dig, kl, tb.qs, tb.ratio_words,
                                        l, l + 1, n)
            return self._moddown_level(acc0, acc1, l)
        lead = x.shape[:-2]
        acc0 = torch.zeros(lead + (l + 1, n), dtype=torch.int64, device=x.device)
        acc1 = torch.zeros_like(acc0)
        for d in range(l):
            # digit d: residues mod q_d in [0, q_d), lifted to every limb
            c = self.backend.ntt(x[..., d, :], d, inverse=True)
            if gt is not None:
                c = self._coeff_automorphism(c, self._q(d), gt)
            for j, i in enumerate(idx):
                q = self._q(i)
                dig = self.backend.ntt(torch.remainder(c, q), i)
                acc0[..., j, :] = torch.remainder(
                    acc0[..., j, :] + self.backend.modmul(
                        dig, key[d, 0, i].expand_as(dig).contiguous(), i), q)
                acc1[..., j, :] = torch.remainder(
                    acc1[..., j, :] + self.backend.modmul(
                        dig, key[d, 1, i].expand_as(dig).contiguous(), i), q)
        return self._moddown_level(acc0, acc1, l)

    def _moddown_level(self, acc0: torch.Tensor, acc1: torch.Tensor, l: int):
        """Mod-down by P of the key-switch accumulators [..., l+1, n] over
        the limbs {q_0..q_{l-1}, P} (P at position l) -> (ks0, ks1), each
        [..., l, n]. Any leading shape: a batch of Galois elements goes
        through in the same launches as one."""
        n, P = self.n, self.special
        if self.device.type == "cuda":
            be = self.backend
            tb = be.level_tables(l)
            outs = []
            for acc in (acc0, acc1):
                cl = be.ntt(acc[..., l, :], self.L, inverse=True)
                r_ntt = be.ntt_all(be.bcast_center_mod(cl, P, l))
                diff = be.modsub_limbs(acc, r_ntt, l)
                outs.append(be._C.modmul_scalar_limbs(
                    diff, tb.pinv, tb.pinv_shoup, be.qs, l, n))
            return outs[0], outs[1]
        P_half = P // 2
        outs = []
        for acc in (acc0, acc1):
            cl = self.backend.ntt(acc[..., l, :], self.L, inverse=True)
            cl_c = torch.where(cl > P_half, cl - P, cl)
            out = acc[..., :l, :].clone()
            for i in range(l):
                q = self._q(i)
                r_ntt = self.backend.ntt(torch.remainder(cl_c, q), i)
                diff = torch.remainder(out[..., i, :] - r_ntt, q)
                out[..., i, :] = self.backend.modmul_scalar(
                    diff, pow(P % q, -1, q), i)
            outs.append(out)
        return outs[0], outs[1]

    def _apply_galois_data(self, data: torch.Tensor, g: int,
                           key: torch.Tensor) -> torch.Tensor:
        """sigma_g on ct data [..., 2, l, n]: (sigma_g(c0) + ks0, ks1) with
        (ks0, ks1) the key-switch of sigma_g(c1). c0 is permuted in the NTT
        domain, where sigma_g is a pure permutation."""
        l = data.shape[-2]
        gt = self._galois_tables(g)
        ks0, ks1 = self._keyswitch_level(data[..., 1, :, :], key, l, g=g)
        if self.device.type == "cuda":
            be = self.backend
            if self._galois_fused():
                return be.galois_perm_add(data, ks0, ks1, gt.perm32)
            c0 = torch.index_select(data[..., 0, :, :], -1, gt.perm)
            return torch.stack([be.modadd_limbs(c0, ks0), ks1], dim=-3)
        c0 = torch.index_select(data[..., 0, :, :], -1, gt.perm)
        return torch.stack([self._modadd(c0, ks0, list(range(l))), ks1], dim=-3)

    @staticmethod
    def _naf(v: int) -> List[int]:
        """Signed powers of two summing to v, no two adjacent (NAF)."""
        out, k = [], 0
        while v:
            if v & 1:
                d = 2 - (v & 3)       # +1 or -1
                out.append(d << k)
                v -= d
            v >>= 1
            k += 1
        return out

    def _rotation_hops(self, step: int, gk) -> List[int]:
        """Galois elements to apply, in order, for a rotation by `step`."""
        s = int(step) % self.slots
        if s == 0:
            return []
        gk = gk or {}
        g = self.galois_element(s)
        if g in gk:
            return [g]
        signed = s if s <= self.slots // 2 else s - self.slots
        hops = []
        for h in self._naf(signed):
            gh = self.galois_element(h)
            if gh not in gk:
                raise ValueError(
                    f"rotation by {step} needs the Galois key for step {h} — "
                    f"run galois_keygen(sk, steps=[{h}]) (Pyfhel API: "
                    f"rotateKeyGen) first")
            hops.append(gh)
        return hops

    def rotate_data(self, data: torch.Tensor, step: int, gk) -> torch.Tensor:
        """Rotate ct data [..., 2, l, n] left by `step` slots (any level
        1..L, any batch shape). One key-switch when gk holds the exact key,
        else one per non-adjacent-form digit over the +-2^k keys."""
        hops = self._rotation_hops(step, gk)
        if not hops:
            return data.clone()
        for g in hops:
            data = self._apply_galois_data(data, g, gk[g])
        return data

    def conjugate_data(self, data: torch.Tensor, gk) -> torch.Tensor:
        g = self.galois_element(conjugate=True)
        if not gk or g not in gk:
            raise ValueError(
                "conjugation needs its Galois key — run galois_keygen(sk, "
                "conjugate=True) (Pyfhel API: rotateKeyGen) first")
        return self._apply_galois_data(data, g, gk[g])

    def sum_slots_data(self, data: torch.Tensor, gk, width: int) -> torch.Tensor:
        """log2(width) rotate-and-add rounds: slot j ends up holding
        sum_{t < width} v[(j + t) mod slots]."""
        if width < 1 or width & (width - 1) or width > self.slots:
            raise ValueError(f"width must be a power of two <= {self.slots}, "
                             f"got {width}")
        limbs = list(range(data.shape[-2]))
        k = 1
        while k < width:
            data = self._modadd(data, self.rotate_data(data, k, gk), limbs)
            k *= 2
        return data

    def rotate(self, ct: Ciphertext, step: int, gk) -> Ciphertext:
        """Slot j of the result holds old slot (j + step) mod slots: decoded,
        np.roll(v, -step). Scale and level are unchanged."""
        return Ciphertext(self.rotate_data(ct.data, step, gk), ct.scale)

    def conjugate(self, ct: Ciphertext, gk) -> Ciphertext:
        return Ciphertext(self.conjugate_data(ct.data, gk), ct.scale)

    def sum_slots(self, ct: Ciphertext, gk, width: int) -> Ciphertext:
        return Ciphertext(self.sum_slots_data(ct.data, gk, width), ct.scale)

    # On a complex-packed tensor the slot operations act on both halves of
    # every ciphertext at once, because they are C-linear in the slots (or,
    # for conjugation, act on the imaginary part alone): a rotation by r
    # rolls values [b*n, b*n + slots) and [b*n + slots, (b+1)*n) by r each,
    # sum_slots sums each half, a real LinearTransform maps each half, and
    # conjugate negates the second half.
    def rotate_tensor(self, ct: CtxtTensor, step: int, gk) -> CtxtTensor:
        """Rotate every ciphertext of the batch by the same step."""
        return CtxtTensor(self.rotate_data(ct.data, step, gk), ct.scale,
                          ct.count, ct.packing)

    def conjugate_tensor(self, ct: CtxtTensor, gk) -> CtxtTensor:
        return CtxtTensor(self.conjugate_data(ct.data, gk), ct.scale, ct.count,
                          ct.packing)

    def sum_slots_tensor(self, ct: CtxtTensor, gk, width: int) -> CtxtTensor:
        return CtxtTensor(self.sum_slots_data(ct.data, gk, width), ct.scale,
                          ct.count, ct.packing)

    # ----- hoisted multi-step rotations -----
    # Everything of a rotation's key-switch up to and including the digit
    # NTTs is independent of the Galois element when the automorphism is
    # applied AFTER the lift: on the NTT-form digits sigma_g is the
    # permutation perm_g. One decomposition D of c1 then serves every step,
    #   acc_g[c, i, k] = sum_d D[d, i, perm_g[k]] * key_g[d, c, i, k]  mod q_i,
    # and the mod-down runs once over the whole [G, R] batch. The permuted
    # digit is the transform of the SIGNED sigma_g of the lifted digit (-v at
    # a wrapped coefficient) where rotate_data lifts q_d - v: the two differ
    # by q_d there, both are congruent to sigma_g(c) mod q_d with |digit| <
    # q_d, so the result is a valid rotation under the same noise bound but
    # not bit-identical to rotate_data's.
    @staticmethod
    def _dot_mod(a: torch.Tensor, b: torch.Tensor, q: int, dim: int) -> torch.Tensor:
        """Exact sum over `dim` of a * b mod q (broadcasting, python ints):
        the CPU oracle's inner product."""
        r = (a.cpu().numpy().astype(object)
             * b.cpu().numpy().astype(object)).sum(axis=dim) % q
        return torch.from_numpy(r.astype(np.int64))

    def _hoist_digits(self, c1: torch.Tensor, l: int) -> torch.Tensor:
        """NTT-form key-switch digits of c1 [..., l, n] with no automorphism:
        D[.., d, j, :] = NTT(c_d mod q_j) over the limbs {q_0..q_{l-1}, P},
        c_d = INTT(c1[.., d, :]) in [0, q_d). Returns [..., l, l+1, n]."""
        if c1.shape[-2] != l or not 1 <= l <= self.L:
            raise ValueError(f"expected [.., {l}, n] with 1 <= l <= {self.L}, "
                             f"got {tuple(c1.shape)}")
        if self.device.type == "cuda":
            be = self.backend
            tb = be.level_tables(l)
            c = be.ntt_all(c1, inverse=True)
            dig = be._C.bcast_center_mod(c, 0, tb.qs, tb.ratio_words, l + 1)
            return be.ntt_level_(dig, tb)
        idx = list(range(l)) + [self.L]
        dig = torch.empty(c1.shape[:-2] + (l, l + 1, self.n), dtype=torch.int64)
        for d in range(l):
            c = self.backend.ntt(c1[..., d, :], d, inverse=True)
            for j, i in enumerate(idx):
                dig[..., d, j, :] = self.backend.ntt(
                    torch.remainder(c, self._q(i)), i)
        return dig

    def _galois_stack(self, elements: Sequence[int], gk, l: int):
        """(keys [G, l, 2, l+1, n], perm32 [G, n], perm [G, n]) of the given
        Galois elements at level l, stacked once per (elements, level) and
        cached the way _key_at_level caches: the entry holds the key tensors
        it was built from and is rebuilt when any of them is another object."""
        elements = tuple(int(g) for g in elements)
        src = tuple(gk[g] for g in elements)
        cache = self.__dict__.setdefault("_galois_stack_cache", {})
        hit = cache.get((elements, l))
        if hit is None or any(a is not b for a, b in zip(hit[0], src)):
            idx = torch.tensor(list(range(l)) + [self.L], dtype=torch.int64,
                               device=self.device)
            for k in src:
                if tuple(k.shape) != (self.L, 2, self.L + 1, self.n):
                    raise ValueError(
                        f"switching key must be [{self.L}, 2, {self.L + 1}, "
                        f"{self.n}], got {tuple(k.shape)}")
            keys = torch.stack([k[:l].index_select(2, idx) for k in src])
            tabs = [self._galois_tables(g) for g in elements]
            hit = (src, keys.contiguous(),
                   torch.stack([t.perm32 for t in tabs]).contiguous(),
                   torch.stack([t.perm for t in tabs]).contiguous())
            cache[(elements, l)] = hit
        return hit[1], hit[2], hit[3]

    def _hoisted_elements(self, steps, gk, conjugate: bool):
        """Galois element per requested output (1 for a step that is a
        multiple of slots), checked against the exact keys in gk."""
        steps = [int(s) for s in steps]
        elems = [self.galois_element(s) for s in steps]
        gk = gk or {}
        missing = sorted({s for s, g in zip(steps, elems)
                          if g != 1 and g not in gk})
        if missing:
            raise ValueError(
                f"rotate_many needs the exact Galois key of every step (a "
                f"composition over +-2^k keys cannot be hoisted); missing "
                f"steps {missing} — run galois_keygen(sk, steps={missing}) "
                f"(Pyfhel API: rotateKeyGen) first")
        if conjugate:
            g = self.galois_element(conjugate=True)
            if g not in gk:
                raise ValueError(
                    "conjugation needs its Galois key — run galois_keygen(sk, "
                    "conjugate=True) (Pyfhel API: rotateKeyGen) first")
            elems.append(g)
        return elems

    def rotate_many_data(self, data: torch.Tensor, steps, gk,
                         conjugate: bool = False) -> List[torch.Tensor]:
        """Rotations of ct data [..., 2, l, n] by every step of `steps` from
        ONE digit decomposition; one result per step in the order given
        (conjugate=True appends the conjugation). Step 0 is a clone, duplicate
        steps are computed once, any level 1..L, any batch shape. Every
        non-zero step needs its exact key in gk. The results of one call are
        slices of one [G, ..] allocation, which lives as long as any of them."""
        elems = self._hoisted_elements(steps, gk, conjugate)
        uniq = list(dict.fromkeys(g for g in elems if g != 1))
        done: Dict[int, torch.Tensor] = {}
        if uniq:
            l, n = data.shape[-2], self.n
            lead = data.shape[:-3]
            flat = data.reshape((-1, 2, l, n))
            R = flat.shape[0]
            dig = self._hoist_digits(flat[:, 1], l)       # [R, l, l+1, n]
            # the batched NTTs put one row per grid y index (<= 65535)
            gmax = len(uniq) if self.device.type != "cuda" else max(
                1, 65535 // (R * (l + 1)))
            for s in range(0, len(uniq), gmax):
                chunk = uniq[s:s + gmax]
                out = self._rotate_hoisted(flat, dig, chunk, gk, l)
                for j, g in enumerate(chunk):
                    done[g] = out[j].reshape(lead + (2, l, n))
        outs, seen = [], set()
        for g in elems:
            if g == 1:
                outs.append(data.clone())
            else:                # a repeated step gets storage of its own
                outs.append(done[g].clone() if g in seen else done[g])
                seen.add(g)
        return outs

    def _rotate_hoisted(self, flat: torch.Tensor, dig: torch.Tensor,
                        elements: Sequence[int], gk, l: int) -> torch.Tensor:
        """flat [R, 2, l, n] and its digits [R, l, l+1, n] -> the rotated
        ciphertexts of `elements`, [G, R, 2, l, n]."""
        keys, perm32, perm = self._galois_stack(elements, gk, l)
        if self.device.type == "cuda":
            be = self.backend
            acc0, acc1 = be.ks_inner_hoisted(dig, keys, perm32,
                                             be.level_tables(l))
            ks0, ks1 = self._moddown_level(acc0, acc1, l)
            return be.galois_perm_add_many(flat, ks0, ks1, perm32)
        G, R, n = len(elements), flat.shape[0], self.n
        idx = list(range(l)) + [self.L]
        acc = torch.empty((2, G, R, l + 1, n), dtype=torch.int64)
        for j in range(G):
            dp = dig.index_select(-1, perm[j])            # sigma_g on D
            for c in range(2):
                for t, i in enumerate(idx):
                    acc[c, j, :, t] = self._dot_mod(
                        dp[:, :, t], keys[j, :, c, t], self._q(i), dim=1)
        ks0, ks1 = self._moddown_level(acc[0], acc[1], l)
        c0 = torch.stack([flat[:, 0].index_select(-1, perm[j])
                          for j in range(G)])             # [G, R, l, n]
        return torch.stack([self._modadd(c0, ks0, list(range(l))), ks1], dim=2)

    def rotate_many(self, ct: Ciphertext, steps, gk,
                    conjugate: bool = False) -> List[Ciphertext]:
        """[rotate(ct, s) for s in steps] from one hoisted decomposition."""
        return [Ciphertext(d, ct.scale) for d in
                self.rotate_many_data(ct.data, steps, gk, conjugate)]

    def rotate_many_tensor(self, ct: CtxtTensor, steps, gk,
                           conjugate: bool = False) -> List[CtxtTensor]:
        """Every ciphertext of the batch rotated by every step."""
        return [CtxtTensor(d, ct.scale, ct.count, ct.packing) for d in
                self.rotate_many_data(ct.data, steps, gk, conjugate)]

    def matvec(self, M, ct, gk):
        """M @ (slots of ct) for a real matrix M [r, c], r, c <= slots: a
        one-shot LinearTransform (hefl/he/linear.py) at ct's level. The
        result is at scale ct.scale * self.scale, not rescaled."""
        from .linear import LinearTransform
        lt = LinearTransform(self, M, level=ct.level)
        if isinstance(ct, CtxtTensor):
            return lt.apply_tensor(ct, gk)
        return lt.apply(ct, gk)

    def modreduce_tensor_(self, ct: CtxtTensor) -> CtxtTensor:
        """Reduce lazily-summed (int64) limb values back to [0, q_i) in place
        — the step after the RCCL all-reduce of raw coefficient tensors."""
        if self.device.type == "cuda":
            # branchless conditional-subtract kernel (sum of <= 8 residues)
            self.backend._C.modreduce_(
                ct.data, self.backend.qs[:ct.level].contiguous())
            return ct
        qs = torch.tensor(self.primes[:ct.level], dtype=torch.int64,
                          device=ct.data.device)
        ct.data.remainder_(qs.view(1, 1, -1, 1))
        return ct

    def _modreduce_(self, data: torch.Tensor) -> torch.Tensor:
        """In-place modreduce of any lazily-summed [..., L', n] tensor over
        the first L' chain primes (ciphertexts, b_i sums, decryption shares)."""
        nlimbs = data.shape[-2]
        if self.device.type == "cuda":
            # branchless conditional-subtract kernel (sum of <= 8 residues)
            self.backend._C.modreduce_(
                data, self.backend.qs[:nlimbs].contiguous())
            return data
        qs = torch.tensor(self.primes[:nlimbs], dtype=torch.int64,
                          device=data.device)
        data.remainder_(qs.view(-1, 1))
        return data
