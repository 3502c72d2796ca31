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

Baby-step/giant-step (bsgs="auto" or a baby-step count n1; opt-in, bsgs=None
is the method above bit for bit): one key per non-zero diagonal becomes about
2*sqrt(diagonals) keys. A step k = g + j with j = k mod n1 (baby) and g = k - j
(giant), and with roll(d, g)[t] = d[(t - g) mod slots]

    M @ v = sum_g rot_g( sum_j roll(diag_{g+j}, g) * rot_j(v) )

    babies    rot_j(ct), j != 0: ONE decomposition of c1, rotate_many's
              launches; baby 0 is ct itself, read in place
    u[g]      = sum_j pt[g+j] * baby_j  over both components  (bsgs_mac; pt
              stored pre-rotated, CSR by giant, over the l chain limbs only)
    acc[c]    = sum_{g != 0} sum_d D_g[d, i, perm_g[k]] * key_g[d, c, i, k]
              with D_g the digits of u[g]'s c1      (bsgs_giant_inner)
    (ks0,ks1) = moddown_P(acc)              one mod-down for ALL giants
    out0      = ks0 + sum_g u[g].c0[perm_g]           (bsgs_finish)
    out1      = ks1 + u[0].c1

The keys are those of the non-zero baby and giant steps (.steps). It costs a
second key-switch round, so it wins once the diagonal method's key traffic
outweighs that (PERFORMANCE.md), and it is the only form whose keys fit for a
dense slots x slots matrix (126 keys instead of 4095 at n = 2^13).

Out of scope: double hoisting (babies kept over QP), complex matrices,
device-side encoding of the diagonals, Galois keys under
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
    pass them to galois_keygen(sk, steps=lt.steps).

    bsgs: None (the diagonal method: one key per non-zero diagonal), "auto"
    (baby-step/giant-step with the power-of-two n1 in [1, slots] that needs
    the fewest keys for this matrix, ties to the smaller) or n1 itself,
    1 <= n1 <= slots. n1, baby_steps and giant_steps are None without it."""

    def __init__(self, ctx: CKKSContext, M, level: Optional[int] = None,
                 scale: Optional[float] = None, bsgs=None):
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
        self._setup(ctx, diags, level, scale, bsgs)

    @classmethod
    def from_diagonals(cls, ctx: CKKSContext, diagonals, level: Optional[int] = None,
                       scale: Optional[float] = None,
                       bsgs=None) -> "LinearTransform":
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
        self._setup(ctx, dict(sorted(diags.items())), level, scale, bsgs)
        return self

    def _setup(self, ctx, diags, level, scale, bsgs=None):
        level = ctx.L if level is None else int(level)
        if not 1 <= level <= ctx.L:
            raise ValueError(f"level must be in [1, {ctx.L}], got {level}")
        self.ctx = ctx
        self.level = level
        self.scale = ctx.scale if scale is None else float(scale)
        self.diag_steps: List[int] = [k for k, d in diags.items() if d.any()]
        if not self.diag_steps:
            raise ValueError("the matrix is zero: nothing to apply")
        self.n1 = self.baby_steps = self.giant_steps = None
        if bsgs is not None:
            self._setup_bsgs(diags, bsgs)
            return
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

    # ----- baby-step/giant-step form ---------------------------------------
    @staticmethod
    def _bsgs_split(steps, n1):
        """(sorted baby steps, sorted giant steps) of the diagonal steps."""
        return (sorted({k % n1 for k in steps}),
                sorted({k - k % n1 for k in steps}))

    def _setup_bsgs(self, diags, bsgs):
        ctx, l, n, slots = self.ctx, self.level, self.ctx.n, self.ctx.slots
        if isinstance(bsgs, str) and bsgs == "auto":
            best = None
            n1 = 1
            while n1 <= slots:             # fewest keys; ties: the smaller n1
                J, I = self._bsgs_split(self.diag_steps, n1)
                cost = len(J) - (0 in J) + len(I) - (0 in I)
                if best is None or cost < best[0]:
                    best = (cost, n1)
                n1 *= 2
            n1 = best[1]
        elif (isinstance(bsgs, (int, np.integer)) and not isinstance(bsgs, bool)
              and 1 <= bsgs <= slots):
            n1 = int(bsgs)
        else:
            raise ValueError(f'bsgs must be None, "auto" or a baby-step count '
                             f"in [1, {slots}], got {bsgs!r}")
        self.n1 = n1
        self.baby_steps, self.giant_steps = self._bsgs_split(self.diag_steps, n1)
        self.steps = [s for s in self.baby_steps + self.giant_steps if s]
        self.elements = [ctx.galois_element(s) for s in self.steps]
        nbk = len(self.baby_steps) - (0 in self.baby_steps)
        self.baby_elements = self.elements[:nbk]
        self.giant_elements = self.elements[nbk:]
        self.has0 = self.baby_steps[0] == 0       # baby 0: the input itself
        self.z0 = 0 if self.giant_steps[0] == 0 else -1

        # CSR over giants: diagonal k = g + j is stored pre-rotated,
        # roll(diag_k, +g), over the l chain limbs only (the plaintext factor
        # is applied after the babies' mod-down, so P is not needed).
        order = sorted(self.diag_steps, key=lambda k: (k - k % n1, k % n1))
        giant_of = [k - k % n1 for k in order]
        goff = np.searchsorted(giant_of, self.giant_steps + [slots]).astype(np.int32)
        bidx = np.array([self.baby_steps.index(k % n1) for k in order],
                        dtype=np.int32)
        self.goff_host, self.bidx_host = goff.tolist(), bidx.tolist()
        self.goff = torch.from_numpy(goff).to(ctx.device)
        self.bidx = torch.from_numpy(bidx).to(ctx.device)
        self.pt = torch.empty((len(order), l, n), dtype=torch.int64,
                              device=ctx.device)
        step = 256                                 # bounds the host buffers
        for s in range(0, len(order), step):
            coeffs = ctx.encoder.encode(
                np.stack([np.roll(diags[k], k - k % n1)
                          for k in order[s:s + step]]), self.scale)
            for i in range(l):
                ci = np.mod(coeffs, ctx._q(i)).astype(np.int64)
                self.pt[s:s + step, i] = ctx.backend.ntt(
                    torch.from_numpy(ci).to(ctx.device), i)
        ident = torch.arange(n, dtype=torch.int64, device=ctx.device)
        self.perm = torch.stack(
            [ctx._galois_tables(ctx.galois_element(g)).perm if g else ident
             for g in self.giant_steps]).contiguous()
        self.perm32 = self.perm.to(torch.int32).contiguous()

    def _apply_bsgs(self, flat: torch.Tensor, gk) -> torch.Tensor:
        """flat [R, 2, l, n] -> [R, 2, l, n]: hoisted baby rotations, the
        multiply-accumulate per giant, ONE key-switch round and mod-down for
        all giants, the finishing adds."""
        ctx, l, n = self.ctx, self.level, self.ctx.n
        be = ctx.backend
        on_gpu = ctx.device.type == "cuda"
        flat = flat.contiguous()
        R = flat.shape[0]
        # the batched NTTs put one row per grid y index (<= 65535)
        gmax = max(1, 65535 // (R * (l + 1))) if on_gpu else len(self.elements)
        if self.baby_elements:
            dig = ctx._hoist_digits(flat[:, 1], l)         # [R, l, l+1, n]
            parts = [ctx._rotate_hoisted(flat, dig,
                                         self.baby_elements[s:s + gmax], gk, l)
                     for s in range(0, len(self.baby_elements), gmax)]
            rot = parts[0] if len(parts) == 1 else torch.cat(parts)
            del dig, parts
        else:
            rot = flat.new_empty((0, R, 2, l, n))
        if on_gpu:
            u = be.bsgs_mac(flat, rot, self.pt, self.goff, self.bidx, self.has0)
        else:
            u = self._mac_cpu(flat, rot)                   # [Ng, R, 2, l, n]
        del rot
        if not self.giant_elements:                        # giant 0 only
            return u[0]
        keys, perm32, perm = ctx._galois_stack(self.giant_elements, gk, l)
        x = u[self.z0 + 1:, :, 1]                          # [Ng', R, l, n]
        acc = None
        for s in range(0, x.shape[0], gmax):
            xs = x[s:s + gmax]
            dig = ctx._hoist_digits(xs.reshape(-1, l, n), l).reshape(
                (xs.shape[0], R, l, l + 1, n))
            if on_gpu:
                a = be.bsgs_giant_inner(dig, keys[s:s + gmax],
                                        perm32[s:s + gmax], be.level_tables(l))
            else:
                a = self._giant_inner_cpu(dig, keys[s:s + gmax],
                                          perm[s:s + gmax])
            del dig
            # chunks add up BEFORE the mod-down, over {q_0..q_{l-1}, P}
            acc = a if acc is None else [
                ctx._modadd(p, c, list(range(l)) + [ctx.L])
                for p, c in zip(acc, a)]
        ks0, ks1 = ctx._moddown(acc[0], acc[1], l)         # one mod-down
        if on_gpu:
            return be.bsgs_finish(u, ks0, ks1, self.perm32, self.z0)
        return self._finish_bsgs_cpu(u, ks0, ks1)

    # exact CPU mirrors of bsgs_mac / bsgs_giant_inner / bsgs_finish
    def _mac_cpu(self, flat, rot):
        ctx, l = self.ctx, self.level
        babies = ([flat] if self.has0 else []) + list(rot)
        u = torch.zeros((len(self.giant_steps),) + tuple(flat.shape),
                        dtype=torch.int64)
        for g in range(len(self.giant_steps)):
            lo, hi = self.goff_host[g], self.goff_host[g + 1]
            b = torch.stack([babies[j] for j in self.bidx_host[lo:hi]])
            for i in range(l):
                u[g, :, :, i] = ctx._dot_mod(
                    b[:, :, :, i], self.pt[lo:hi, i][:, None, None],
                    ctx._q(i), dim=0)
        return u

    def _giant_inner_cpu(self, dig, keys, perm):
        ctx, l = self.ctx, self.level
        R, n = dig.shape[1], ctx.n
        acc = torch.zeros((2, R, l + 1, n), dtype=torch.int64)
        for g in range(dig.shape[0]):
            dp = dig[g].index_select(-1, perm[g])
            for c in range(2):
                for t, i in enumerate(list(range(l)) + [ctx.L]):
                    q = ctx._q(i)
                    acc[c, :, t] = torch.remainder(acc[c, :, t] + ctx._dot_mod(
                        dp[:, :, t], keys[g, :, c, t], q, dim=1), q)
        return [acc[0], acc[1]]

    def _finish_bsgs_cpu(self, u, ks0, ks1):
        ctx, limbs = self.ctx, list(range(self.level))
        out0, out1 = ks0, ks1
        for g in range(u.shape[0]):
            out0 = ctx._modadd(
                out0, u[g, :, 0].index_select(-1, self.perm[g]), limbs)
        if self.z0 >= 0:
            out1 = ctx._modadd(out1, u[self.z0, :, 1], limbs)
        return torch.stack([out0, out1], dim=1)

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
            what = ("non-zero diagonal" if self.n1 is None
                    else "non-zero baby and giant step")
            raise ValueError(
                f"the transform needs the exact Galois key of every {what}"
                f"; missing steps {missing} — run galois_keygen(sk, "
                f"steps={missing}) (Pyfhel API: rotateKeyGen) first")
        lead = data.shape[:-3]
        flat = data.reshape((-1, 2, l, n))
        if self.n1 is not None:
            return self._apply_bsgs(flat, gk).reshape(lead + (2, l, n))
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
            ks0, ks1 = ctx._moddown(acc0, acc1, l)
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
