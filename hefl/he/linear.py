"""Encrypted matrix-vector product: a real matrix applied to the slots of a
CKKS ciphertext by the diagonal method, on hoisted rotations.

With diag_k[j] = M[j, (j + k) mod slots] and rot_k the left rotation by k
slots,  M @ v = sum_k diag_k * rot_k(v).  All rotations share one digit
decomposition D of c1 (CKKSContext._hoist_digits), and the plaintext factor is
applied BEFORE the mod-down, over the limbs {q_0..q_{l-1}, P}:

    acc[c, i, k] = sum_{b, step != 0} pt_b[i, k] *
                   (sum_d D[d, i, perm_b[k]] * key_b[d, c, i, k])
    (ks0, ks1)   = moddown_P(acc)                          one mod-down
    out0[i, k]   = ks0[i, k] + sum_b pt_b[i, k] * c0[i, perm_b[k]]
    out1[i, k]   = ks1[i, k] + pt_0[i, k] * c1[i, k]       step-0 diagonal

so a transform of G diagonals costs one decomposition, one inner kernel
(lt_inner), one mod-down and one finishing kernel (lt_finish), whatever G is.
The result stays at the input level with scale ct.scale * pt_scale; like
mul_ct and mul_plain it is not rescaled.

Out of scope: baby-step/giant-step splitting (needs ~2*sqrt(r + c) keys where
this needs one per non-zero diagonal), complex matrices, Galois keys under
key_mode="threshold", checkpointing a transform.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .ckks import CKKSContext, Ciphertext, CtxtTensor


class LinearTransform:
    """A real matrix M [r, c] (r, c <= slots), zero-padded to slots x slots,
    encoded once for ciphertexts at `level` and held on the context's device.

    steps: the rotation steps whose exact Galois keys apply() needs —
    pass them to galois_keygen(sk, steps=lt.steps)."""

    def __init__(self, ctx: CKKSContext, M, level: Optional[int] = None,
                 scale: Optional[float] = None):
        M = np.asarray(M)
        if np.iscomplexobj(M):
            raise ValueError("complex matrices are not supported")
        M = M.astype(np.float64)
        slots = ctx.slots
        if M.ndim != 2 or not (1 <= M.shape[0] <= slots
                               and 1 <= M.shape[1] <= slots):
            raise ValueError(f"matrix must be [r, c] with 1 <= r, c <= {slots}, "
                             f"got {M.shape}")
        r, c = M.shape
        j = np.arange(r)
        diags = {}
        for k in sorted({k % slots for k in range(-(r - 1), c)}):
            col = (j + k) % slots              # only these can be non-zero
            ok = col < c
            d = np.zeros(slots, dtype=np.float64)
            d[j[ok]] = M[j[ok], col[ok]]
            diags[k] = d
        self.shape = (r, c)
        self._setup(ctx, diags, level, scale)

    @classmethod
    def from_diagonals(cls, ctx: CKKSContext, diagonals, level: Optional[int] = None,
                       scale: Optional[float] = None) -> "LinearTransform":
        """The transform given by its generalised diagonals {step k: real
        vector [<= slots]} directly, without the slots x slots matrix."""
        self = cls.__new__(cls)
        diags = {}
        for k, d in diagonals.items():
            d = np.asarray(d)
            if np.iscomplexobj(d):
                raise ValueError("complex matrices are not supported")
            if d.ndim != 1 or d.shape[0] > ctx.slots:
                raise ValueError(f"a diagonal holds at most {ctx.slots} values")
            full = np.zeros(ctx.slots, dtype=np.float64)
            full[:d.shape[0]] = d
            diags[int(k) % ctx.slots] = full
        self.shape = (ctx.slots, ctx.slots)
        self._setup(ctx, dict(sorted(diags.items())), level, scale)
        return self

    def _setup(self, ctx, diags, level, scale):
        level = ctx.L if level is None else int(level)
        if not 1 <= level <= ctx.L:
            raise ValueError(f"level must be in [1, {ctx.L}], got {level}")
        self.ctx = ctx
        self.level = level
        self.scale = ctx.scale if scale is None else float(scale)
        self.diag_steps: List[int] = [k for k, d in diags.items() if d.any()]
        if not self.diag_steps:
            raise ValueError("the matrix is zero: nothing to apply")
        self.steps: List[int] = [k for k in self.diag_steps if k != 0]
        self.z0 = self.diag_steps.index(0) if 0 in self.diag_steps else -1

        # Diagonals are encoded on the host (the CPU and the device context
        # hold bit-identical plaintexts) over {q_0..q_{l-1}, P}.
        coeffs = ctx.encoder.encode(
            np.stack([diags[k] for k in self.diag_steps]), self.scale)
        rows = []
        for i in list(range(level)) + [ctx.L]:
            ci = np.mod(coeffs, ctx._q(i)).astype(np.int64)
            rows.append(ctx.backend.ntt(
                torch.from_numpy(ci).to(ctx.device), i))
        pt_ext = torch.stack(rows, dim=-2)                 # [G', l+1, n]
        self.pt = pt_ext[:, :level].contiguous()           # lt_finish operand
        keyed = [b for b, k in enumerate(self.diag_steps) if k != 0]
        self.pt_keyed = pt_ext[keyed].contiguous()         # lt_inner operand
        self.elements = [ctx.galois_element(k) for k in self.steps]
        tabs = [ctx._galois_tables(ctx.galois_element(k))
                if k else None for k in self.diag_steps]
        ident = torch.arange(ctx.n, dtype=torch.int64, device=ctx.device)
        self.perm = torch.stack([ident if t is None else t.perm
                                 for t in tabs]).contiguous()
        self.perm32 = self.perm.to(torch.int32).contiguous()

    def apply_data(self, data: torch.Tensor, gk) -> torch.Tensor:
        """ct data [..., 2, l, n] -> transformed ct data, same shape."""
        ctx, l, n = self.ctx, self.level, self.ctx.n
        if data.shape[-2] != l:
            raise ValueError(
                f"this LinearTransform was encoded for level {l} but the "
                f"ciphertext is at level {data.shape[-2]}; build it with "
                f"level={data.shape[-2]} or bring the ciphertext to level {l}")
        gk = gk or {}
        missing = [k for k, g in zip(self.steps, self.elements) if g not in gk]
        if missing:
            raise ValueError(
                f"the transform needs the exact Galois key of every non-zero "
                f"diagonal; missing steps {missing} — run galois_keygen(sk, "
                f"steps={missing}) (Pyfhel API: rotateKeyGen) first")
        lead = data.shape[:-3]
        flat = data.reshape((-1, 2, l, n))
        R = flat.shape[0]
        on_gpu = ctx.device.type == "cuda"
        if self.elements:
            dig = ctx._hoist_digits(flat[:, 1], l)         # [R, l, l+1, n]
            keys, perm32, perm = ctx._galois_stack(self.elements, gk, l)
            if on_gpu:
                acc0, acc1 = ctx.backend.lt_inner(
                    dig, keys, perm32, self.pt_keyed,
                    ctx.backend.level_tables(l))
            else:
                acc0, acc1 = self._inner_cpu(dig, keys, perm)
            ks0, ks1 = ctx._moddown_level(acc0, acc1, l)
        else:                                              # step 0 only
            ks0 = torch.zeros((R, l, n), dtype=torch.int64, device=ctx.device)
            ks1 = torch.zeros_like(ks0)
        if on_gpu:
            out = ctx.backend.lt_finish(flat, ks0, ks1, self.pt, self.perm32,
                                        self.z0)
        else:
            out = self._finish_cpu(flat, ks0, ks1)
        return out.reshape(lead + (2, l, n))

    # ----- exact CPU path: the same integer algebra, the device's oracle -----
    def _inner_cpu(self, dig, keys, perm):
        ctx, l = self.ctx, self.level
        R, n = dig.shape[0], ctx.n
        idx = list(range(l)) + [ctx.L]
        acc = torch.zeros((2, R, l + 1, n), dtype=torch.int64)
        for b in range(len(self.elements)):
            dp = dig.index_select(-1, perm[b])
            for c in range(2):
                for t, i in enumerate(idx):
                    q = ctx._q(i)
                    inner = ctx._dot_mod(dp[:, :, t], keys[b, :, c, t], q, dim=1)
                    term = ctx.backend.modmul(
                        inner, self.pt_keyed[b, t].expand_as(inner).contiguous(), i)
                    acc[c, :, t] = torch.remainder(acc[c, :, t] + term, q)
        return acc[0], acc[1]

    def _finish_cpu(self, flat, ks0, ks1):
        ctx, l = self.ctx, self.level
        out0, out1 = ks0.clone(), ks1.clone()
        for i in range(l):
            q = ctx._q(i)
            for b in range(len(self.diag_steps)):
                p = self.pt[b, i]
                c0 = flat[:, 0, i].index_select(-1, self.perm[b])
                out0[:, i] = torch.remainder(out0[:, i] + ctx.backend.modmul(
                    c0, p.expand_as(c0).contiguous(), i), q)
                if b == self.z0:
                    c1 = flat[:, 1, i]
                    out1[:, i] = torch.remainder(
                        out1[:, i] + ctx.backend.modmul(
                            c1.contiguous(), p.expand_as(c1).contiguous(), i), q)
        return torch.stack([out0, out1], dim=1)

    def apply(self, ct: Ciphertext, gk) -> Ciphertext:
        """Encryption of M @ v at scale ct.scale * self.scale, level
        unchanged; the caller rescales (at level 1 it cannot be)."""
        return Ciphertext(self.apply_data(ct.data, gk), ct.scale * self.scale)

    def apply_tensor(self, ct: CtxtTensor, gk) -> CtxtTensor:
        """Every ciphertext (vector) of the batch through the one matrix; on
        a complex-packed tensor, both halves of every ciphertext."""
        return CtxtTensor(self.apply_data(ct.data, gk), ct.scale * self.scale,
                          ct.count, ct.packing)
