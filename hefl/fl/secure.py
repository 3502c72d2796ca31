"""Encrypted FedAvg: CKKS ciphertexts summed by an RCCL all-reduce over xGMI.

This collapses the reference's whole aggregation stack — pickle export
(FLPyfhelin.py:230-240), import (:303-328) and the per-scalar Python
add/mult loop (:366-390, timed at 231 s for 2 clients) — into:

  1. encrypt the client's flat fp32 weight vector into slot-packed CKKS
     ciphertexts resident in HBM (one [B, 2, L, n] int64 tensor), in SLABS
     (n/2 weights per ciphertext, or n with he.packing="complex": every
     step below is C-linear in the slots, so both parts of a slot average),
  2. per slab, ONE async all-reduce(SUM) on the raw RNS coefficients,
     issued as soon as that slab is encrypted — the collective for slab i
     rides the 7 xGMI links while slab i+1 is still encrypting on the
     compute stream. Limb primes are < 2**60 (hefl/he/primes.py), so an
     int64 SUM over <= 8 clients is overflow-free lazy reduction — no
     per-hop modular arithmetic, RCCL's stock int64 sum rings do the work,
  3. one modreduce kernel back to [0, q_i), one ct x plain(1/n) multiply,
     one rescale — run for EVERY n including n=1, so a 1-GPU round is
     structurally identical to the 8-GPU round minus the collective,
  4. decrypt. The aggregation itself used no key at all, preserving the
     reference's pk-only-server model (FLPyfhelin.py:370); who can decrypt
     depends on the key mode below.

Key agreement, key_mode="shared" (default): the reference shares ONE keypair
via pickle files (cell 1 + FLPyfhelin.py:346-355). Here rank 0's keys are
broadcast over the process group at init — correctness no longer depends on
every rank seeding keygen identically (with he.seed=None each rank's keygen
draws OS entropy; summing ciphertexts under different keys would decrypt to
noise with no error).

Key separation: in shared mode EVERY rank holds sk, so any client can decrypt
any other client's ciphertext, including the partial sums it sees during the
ring all-reduce. That is the reference's trust model (one privatekey.pickle
read by everybody), not a privacy property. key_mode="threshold" removes it.

Key agreement, key_mode="threshold": n-of-n additive threshold CKKS, semi-
honest parties, k <= 8 parties so the lazy int64 sums below cannot overflow.
All arithmetic is per RNS limb, NTT domain, mod q:

  common polynomial   a uniform [L, n], public; rank 0 samples it and
                      broadcasts it (single-process simulation: sampled once)
  party i key share   s_i ternary, e_i error (keygen's distributions), drawn
                      from a per-party stream (seed + party index, or OS
                      entropy) — the shared-seed keygen stream is identical
                      on every rank and would give every party the same s_i;
                      b_i = -(a*s_i + e_i);  party i keeps only s_i
  collective pk       b = sum_i b_i  (int64 SUM all-reduce + modreduce; eight
                      residues < 2^60 cannot overflow),  pk = (b, a).
                      The secret s = sum_i s_i exists nowhere. Encryption and
                      aggregation run unchanged under pk.
  decryption share    on the aggregated ct = (c0, c1) at Lc limbs:
                      h_i = c1*s_i + NTT(e'_i) (+ c0 for the lead party,
                      rank 0), e'_i fresh smudging noise uniform in
                      [-2^smudge_bits, 2^smudge_bits) per coefficient, drawn
                      anew for every decryption from the party's own
                      reseeded RNG
  combine             pt = modreduce(sum_i h_i)  (int64 SUM all-reduce: each
                      h_i < q < 2^60, eight of them < 2^63), then decode.

After aggregation every rank holds the same averaged ciphertext, so that one
extra all-reduce of shares yields the plaintext mean on every rank. A single
share decodes to noise: no rank can decrypt alone, neither another client's
upload nor a partial sum.

smudge_bits trades statistical hiding of the decryption noise (which depends
on the ciphertext's noise, hence on s) against precision: worst-case slot
error added k*n*2^smudge_bits/scale, typically 2^smudge_bits*sqrt(k*n/3)/scale
(~3e-5 at n=8192, scale 2^40, k=8, the default 16). Valid range 0..48. It is
a tunable, NOT a proof of simulation security. Collective relinearisation-key
generation is out of scope, so threshold mode excludes the encrypted
denominator (ct x ct); t-of-n thresholds and malicious parties are too.

The timing labels mirror the reference's prints (FLPyfhelin.py:224,267,389)
for log familiarity.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Dict, Optional

import torch
import torch.distributed as dist

from ..he.ckks import CKKSContext, CtxtTensor, KeyPair, check_smudge_bits

# Per-slab payload for the bucketed all-reduce. xGMI is 7 point-to-point
# links x ~153 GB/s per GPU; ~64 MiB slabs are big enough to amortize ring
# setup yet small enough that several are in flight while later slabs
# encrypt (collectives row).
DEFAULT_BUCKET_BYTES = 64 << 20


@dataclass
class AggStats:
    seconds: Dict[str, float] = field(default_factory=dict)


class SecureAggregator:
    """Per-rank helper owning the CKKS context + keys for encrypted FedAvg.

    key_mode="shared": rank 0 generates the keypair (and relin keys /
    encrypted denominator if configured) and broadcasts it; every other rank
    adopts it. key_mode="threshold": the ranks run the collective keygen of
    the module docstring and `keys.sk` holds only this rank's share. Either
    way encryption randomness is then re-seeded per rank so client
    ciphertexts are independent.
    """

    def __init__(self, ctx: CKKSContext, rank: int = 0, verbose: bool = False,
                 denom_mode: str = "plain", n_clients: Optional[int] = None,
                 bucket_bytes: int = DEFAULT_BUCKET_BYTES,
                 key_mode: str = "shared", smudge_bits: int = 16):
        """denom_mode:
        - "plain":     divide the summed ciphertext by plaintext 1/n
                       (ct x plain mult + rescale — what the reference
                       actually exercises, FLPyfhelin.py:385);
        - "encrypted": multiply by an ENCRYPTED 1/n (ct x ct + relinearize +
                       rescale — the reference's commented-out intent,
                       c_denom at FLPyfhelin.py:371; BASELINE.json config #3).
                       Requires n_clients at construction.
        key_mode: "shared" | "threshold" (module docstring); smudge_bits is
        the threshold-decryption noise width, 0..48.
        """
        assert denom_mode in ("plain", "encrypted")
        if key_mode not in ("shared", "threshold"):
            raise ValueError(
                f"key_mode must be 'shared' or 'threshold', got {key_mode!r}")
        check_smudge_bits(smudge_bits)
        if key_mode == "threshold" and denom_mode == "encrypted":
            raise ValueError(
                "key_mode='threshold' cannot use denom_mode='encrypted': "
                "collective relinearisation-key generation is not implemented")
        self.ctx = ctx
        self.rank = rank
        self.key_mode = key_mode
        self.smudge_bits = smudge_bits
        self.denom_mode = denom_mode
        self.bucket_bytes = bucket_bytes
        self.enc_denom = None
        # threshold mode never runs the full keygen: no sk to begin with
        self.keys: Optional[KeyPair] = (
            ctx.keygen() if key_mode == "shared" else None)
        if denom_mode == "encrypted":
            if ctx.L < 3:
                raise ValueError(
                    "encrypted denominator needs a >=3-limb chain "
                    "(ct x ct consumes one rescale level)")
            if n_clients is None:
                raise ValueError("denom_mode='encrypted' needs n_clients")
            self.keys.relin = ctx.relin_keygen(self.keys.sk)
            import numpy as np
            pt = ctx.encode(np.full(ctx.slots, 1.0 / n_clients))
            self.enc_denom = ctx.encrypt(pt, self.keys.pk)
        self._sync_keys()
        ctx.reseed(rank)
        self.verbose = verbose
        self.stats = AggStats()

    def _sync_keys(self) -> None:
        """Shared mode: broadcast rank 0's key material so all ranks share
        ONE keypair (the reference's single publickey.pickle /
        privatekey.pickle model). Threshold mode: the collective keygen —
        no secret material is ever sent."""
        if self.key_mode == "threshold":
            self.keys = self._threshold_keygen()
            return
        if not (dist.is_initialized() and dist.get_world_size() > 1):
            return
        dist.broadcast(self.keys.sk, src=0)
        dist.broadcast(self.keys.pk, src=0)
        if self.keys.relin is not None:
            dist.broadcast(self.keys.relin, src=0)
        if self.enc_denom is not None:
            dist.broadcast(self.enc_denom.data, src=0)

    def _threshold_keygen(self) -> KeyPair:
        """Collective keygen: broadcast a, all-reduce the b_i. Only public
        values cross the wire; the returned sk is this rank's share alone.
        World size 1 runs the same sequence without the collectives."""
        ctx = self.ctx
        world = dist.get_world_size() if dist.is_initialized() else 1
        assert world <= 8, "lazy int64 reduction is proven for <= 8 summands"
        a = ctx.sample_crp()
        if world > 1:
            dist.broadcast(a, src=0)
        share = ctx.keygen_share(a, self.rank)
        b_sum = share.b_share.clone()
        if world > 1:
            dist.all_reduce(b_sum, op=dist.ReduceOp.SUM)
        return KeyPair(sk=share.sk_share, pk=ctx.combine_pk(b_sum, a))

    def _t(self, label: str, t0: float):
        dt = time.perf_counter() - t0
        self.stats.seconds[label] = self.stats.seconds.get(label, 0.0) + dt
        if self.verbose:
            print(f"Time to {label}:", dt)

    def _slab_cts(self, polys: Optional[int] = None) -> int:
        """Ciphertexts per all-reduce bucket (>=1). `polys` = limb rows per
        item: 2*L for a fresh ciphertext (default), Lc for a decryption
        share."""
        polys = 2 * self.ctx.L if polys is None else polys
        per_ct = polys * self.ctx.n * 8  # int64 bytes
        return max(1, self.bucket_bytes // per_ct)

    def encrypt(self, vec: torch.Tensor) -> CtxtTensor:
        t0 = time.perf_counter()
        ct = self.ctx.encrypt_tensor(vec, self.keys.pk)
        self._t("encrypt weights", t0)
        return ct

    def _divide(self, ct: CtxtTensor, n: int) -> CtxtTensor:
        """ct x (1/n) + rescale — ALWAYS executed (n=1 included) so the
        per-round op sequence does not depend on world size."""
        if self.denom_mode == "encrypted":
            from ..he.ckks import Ciphertext
            prod = self.ctx.mul_ct(Ciphertext(ct.data, ct.scale),
                                   self.enc_denom, self.keys.relin)
            # the encrypted 1/n is a real constant in every slot, so the
            # product keeps whatever packing ct has
            out = CtxtTensor(prod.data, prod.scale, ct.count, ct.packing)
            return self.ctx.rescale_tensor(out)
        return self.ctx.rescale_tensor(
            self.ctx.mul_scalar_tensor(ct, 1.0 / n))

    def aggregate(self, ct: CtxtTensor, n_clients: Optional[int] = None) -> CtxtTensor:
        """Sum ciphertexts across ranks (bucketed lazy int64 all-reduce) and
        divide by n."""
        t0 = time.perf_counter()
        world = dist.get_world_size() if dist.is_initialized() else 1
        n = n_clients if n_clients is not None else world
        assert n <= 8, "lazy int64 reduction is proven for <= 8 summands"
        if world > 1:
            slab = self._slab_cts()
            works = [dist.all_reduce(ct.data[i:i + slab], op=dist.ReduceOp.SUM,
                                     async_op=True)
                     for i in range(0, ct.data.shape[0], slab)]
            for w in works:
                w.wait()
        self.ctx.modreduce_tensor_(ct)
        out = self._divide(ct, n)
        self._t("aggregate", t0)
        return out

    def fedavg_ct(self, vec: torch.Tensor,
                  n_clients: Optional[int] = None) -> CtxtTensor:
        """Encrypt + all-reduce with slab pipelining: the all-reduce for
        slab i overlaps the encryption of slab i+1 (encrypt runs on the
        compute stream, the collective on RCCL's own streams)."""
        t0 = time.perf_counter()
        world = dist.get_world_size() if dist.is_initialized() else 1
        n = n_clients if n_clients is not None else world
        assert n <= 8, "lazy int64 reduction is proven for <= 8 summands"
        ctx = self.ctx
        per_ct = ctx.values_per_ct     # slots, or n under complex packing
        count = vec.numel()
        B = (count + per_ct - 1) // per_ct
        slab = self._slab_cts()
        if world <= 1 or B <= slab:
            ct = self.encrypt(vec)
            return self.aggregate(ct, n_clients=n)
        data = torch.empty((B, 2, ctx.L, ctx.n), dtype=torch.int64,
                           device=ctx.device)
        works = []
        scale, packing = None, "real"
        for b0 in range(0, B, slab):
            b1 = min(B, b0 + slab)
            sub = vec[b0 * per_ct: min(count, b1 * per_ct)]
            ct_slab = ctx.encrypt_tensor(sub, self.keys.pk)
            data[b0:b1].copy_(ct_slab.data)
            scale, packing = ct_slab.scale, ct_slab.packing
            works.append(dist.all_reduce(data[b0:b1], op=dist.ReduceOp.SUM,
                                         async_op=True))
        self._t("encrypt weights", t0)
        t1 = time.perf_counter()
        for w in works:
            w.wait()
        ct = CtxtTensor(data, scale, count, packing)
        self.ctx.modreduce_tensor_(ct)
        out = self._divide(ct, n)
        self._t("aggregate", t1)
        return out

    def decrypt(self, ct: CtxtTensor) -> torch.Tensor:
        t0 = time.perf_counter()
        if self.key_mode == "threshold":
            vec = self._threshold_decrypt(ct)
        else:
            vec = self.ctx.decrypt_tensor(ct, self.keys.sk)
        self._t("decrypt", t0)
        return vec

    def _threshold_decrypt(self, ct: CtxtTensor) -> torch.Tensor:
        """This rank's share of the (identical on every rank) aggregated
        ciphertext, a bucketed lazy int64 all-reduce of the shares, combine.
        A ResNet-size share tensor is hundreds of MB, hence the buckets."""
        world = dist.get_world_size() if dist.is_initialized() else 1
        assert world <= 8, "lazy int64 reduction is proven for <= 8 summands"
        share = self.ctx.partial_decrypt_tensor(
            ct, self.keys.sk, self.smudge_bits,
            lead=self.rank == 0 or world == 1)
        if world > 1:
            slab = self._slab_cts(ct.level)
            works = [dist.all_reduce(share[i:i + slab], op=dist.ReduceOp.SUM,
                                     async_op=True)
                     for i in range(0, share.shape[0], slab)]
            for w in works:
                w.wait()
        return self.ctx.combine_shares_tensor(share, ct.scale, ct.count,
                                              packing=ct.packing)

    def fedavg(self, vec: torch.Tensor, n_clients: Optional[int] = None) -> torch.Tensor:
        """Full encrypted FedAvg of a flat fp32 weight vector."""
        return self.decrypt(self.fedavg_ct(vec, n_clients)).to(vec.device)
