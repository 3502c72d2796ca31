"""Baby-step/giant-step LinearTransform (bsgs=...) on the exact CPU backend,
the oracle of the device path.

Accuracy rule of test_hoist_cpu.py: after one rescale the slot error against
float64 M @ v is below 1e-4 max|Mv| and at most 4x the error of the path
composed of rotate, mul_plain and add on the same inputs (two independent
noise samples of the same structure; a wrong roll direction, permutation or
key gives an error of order max|Mv|). The errors are printed.
"""
import functools

import numpy as np
import pytest
import torch

from hefl.config import HEConfig
from hefl.he import CKKSContext, CtxtTensor, LinearTransform
from hefl.he.ckks import Ciphertext

# (n, chain, scale_bits) — the fixtures' parameters of test_hoist_cpu.py
PARAMS = {"n64": (64, (50, 30, 30), 30), "n256": (256, (60, 40, 40), 40)}

# name: (ring, matrix shape or "dense", n1, below_top, complex-packed rows R)
CASES = {
    "dense-n1=4": ("n64", "dense", 4, False, 0),
    "5x7-n1=8-wraps": ("n64", (5, 7), 8, False, 0),
    "ragged-n1=3": ("n64", (5, 7), 3, False, 0),
    "no-babies-n1=1": ("n64", (5, 7), 1, False, 0),
    "no-giants-n1=slots": ("n64", (5, 7), 32, False, 0),
    "below-top": ("n64", (5, 7), 4, True, 0),
    "complex-packed-R=2": ("n64", (5, 7), 4, False, 2),
    "n256-8x16-n1=4": ("n256", (8, 16), 4, False, 0),
}


@functools.lru_cache(maxsize=None)
def _ring(name):
    n, chain, sb = PARAMS[name]
    ctx = CKKSContext(HEConfig(m=n, scale_bits=sb, q_bits=chain, seed=11))
    return ctx, ctx.keygen()


def _rows(ctx, kp, data, scale):
    """Complex slot values [R, slots] of ct data [R, 2, l, n]."""
    return np.stack([ctx.decode(ctx.decrypt(Ciphertext(d, scale), kp.sk),
                                ctx.slots, complex=True) for d in data])


@pytest.mark.parametrize("case", sorted(CASES))
def test_bsgs_slot_accuracy(case):
    ring, shape, n1, below_top, packed = CASES[case]
    ctx, kp = _ring(ring)
    slots = ctx.slots
    r, c = (slots, slots) if shape == "dense" else shape
    rng = np.random.default_rng(17)
    M = rng.uniform(-1, 1, (r, c))
    R = packed or 1
    z = np.zeros((R, slots), dtype=np.complex128)
    z[:, :c] = rng.uniform(-1, 1, (R, c))
    if packed:
        z[:, :c] += 1j * rng.uniform(-1, 1, (R, c))
    pt = ctx.encode(z if packed else z.real)
    ct = CtxtTensor(ctx._encrypt_data(pt.data, kp.pk), pt.scale,
                    R * (ctx.n if packed else slots),
                    "complex" if packed else "real")
    if below_top:
        ct = ctx.rescale_tensor(ctx.mul_scalar_tensor(ct, 1.0))
    lt = LinearTransform(ctx, M, level=ct.level, bsgs=n1)
    diag = LinearTransform(ctx, M, level=ct.level)
    assert lt.n1 == n1 and lt.diag_steps == diag.diag_steps
    gk = ctx.galois_keygen(kp.sk, steps=sorted(set(lt.steps + diag.steps)))
    out = lt.apply_tensor(ct, gk)
    assert out.level == ct.level and out.scale == ct.scale * lt.scale
    assert out.packing == ct.packing and out.count == ct.count
    assert out.data.shape == ct.data.shape
    new = ctx.rescale_tensor(out)

    full = np.zeros((slots, slots))
    full[:r, :c] = M
    j = np.arange(slots)
    ref = []
    for row in ct.data:                       # rotate, mul_plain, add
        acc = None
        for k in diag.diag_steps:
            d = ctx.encode(full[j, (j + k) % slots], nlimbs=ct.level,
                           scale=lt.scale)
            term = ctx.mul_plain(ctx.rotate(Ciphertext(row, ct.scale), k, gk), d)
            acc = term if acc is None else ctx.add(acc, term)
        ref.append(ctx.rescale(acc).data)
    want = z @ full.T
    peak = np.abs(want).max()
    err_new = np.abs(_rows(ctx, kp, new.data, new.scale) - want).max()
    err_ref = np.abs(_rows(ctx, kp, torch.stack(ref), new.scale) - want).max()
    print(f"{case}: {len(lt.steps)} keys (babies {lt.baby_steps}, giants "
          f"{lt.giant_steps}), err_bsgs {err_new:.3e}, err_composed "
          f"{err_ref:.3e}, max|Mv| {peak:.3f}")
    assert err_ref < 1e-4 * peak and err_new < 1e-4 * peak
    assert err_new <= 4 * err_ref


def test_bsgs_steps_and_interface():
    ctx, kp = _ring("n64")
    slots = ctx.slots
    M = np.random.default_rng(3).uniform(-1, 1, (slots, slots))
    auto = LinearTransform(ctx, M, bsgs="auto")
    assert len(LinearTransform(ctx, M).steps) == 31
    assert auto.n1 == 4 and len(auto.steps) == 10      # 3 babies + 7 giants
    small = np.random.default_rng(4).uniform(-1, 1, (5, 7))
    for n1 in (1, 3, 8, slots):
        lt = LinearTransform(ctx, small, bsgs=n1)
        ks = lt.diag_steps
        assert lt.baby_steps == sorted({k % n1 for k in ks})
        assert lt.giant_steps == sorted({k - k % n1 for k in ks})
        assert lt.steps == sorted((set(lt.baby_steps) | set(lt.giant_steps))
                                  - {0})
    assert LinearTransform(ctx, small, bsgs=8).giant_steps == [0, 24]
    for bad in (0, slots + 1, "sqrt", 2.0, True):
        with pytest.raises(ValueError, match="bsgs"):
            LinearTransform(ctx, small, bsgs=bad)

    lt = LinearTransform(ctx, small, bsgs=8)
    v = np.random.default_rng(5).uniform(-1, 1, 7)
    ct = ctx.encrypt(ctx.encode(v), kp.pk)
    gk = ctx.galois_keygen(kp.sk, steps=[s for s in lt.steps if s != 24])
    with pytest.raises(ValueError, match=r"missing steps \[24\].*"
                                         r"galois_keygen\(sk, steps=\[24\]\)"):
        lt.apply(ct, gk)
    with pytest.raises(ValueError, match="level"):
        LinearTransform(ctx, small, level=ctx.L - 1, bsgs=8).apply(ct, gk)
    # bsgs=None is the diagonal method, bit for bit; matvec passes bsgs on
    gk = ctx.galois_keygen(kp.sk, steps=sorted(
        set(lt.steps + LinearTransform(ctx, small).steps)))
    plain = LinearTransform(ctx, small).apply(ct, gk)
    assert torch.equal(LinearTransform(ctx, small, bsgs=None).apply(ct, gk).data,
                       plain.data)
    assert torch.equal(ctx.matvec(small, ct, gk).data, plain.data)
    assert torch.equal(ctx.matvec(small, ct, gk, bsgs=8).data,
                       lt.apply(ct, gk).data)
    by_diag = LinearTransform.from_diagonals(
        ctx, {0: np.full(slots, 0.5), 9: np.full(slots, -0.25)}, bsgs=8)
    assert by_diag.baby_steps == [0, 1] and by_diag.giant_steps == [0, 8]
