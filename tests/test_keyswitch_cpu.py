"""CPU tests of the one level-aware key-switch: keys and top-level results
pinned to the integers of the commit before relinearization and rotations
shared it, ct x ct below the top level, argument checks, batched operands."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hefl.config import HEConfig
from hefl.he.ckks import CKKSContext, Ciphertext

GOLDEN = os.path.join(os.path.dirname(__file__), "golden",
                      "keyswitch_parent_m64.npz")


def test_keys_and_top_level_results_match_parent_commit():
    """Bit-identity with commit 2c263f4 (the parent of the change that
    folded the two key-switch routines and the two key generators into one).
    The golden file holds what that commit computed on the CPU from ONE
    context, HEConfig(m=64, scale_bits=26, q_bits=(55, 26, 26), seed=0), in
    this call order, so the seeded host stream lines up:

        keygen; relin_keygen; galois_keygen(steps=[1, -1], conjugate=True);
        v1, v2 from default_rng(5) as in test_mul_ct_relin_rescale;
        encrypt(v1); encrypt(v2); mul_ct(ct1, ct2); rotate(ct1, 1);
        rotate_many(ct1, [1, -1], conjugate=True)
    """
    gold = np.load(GOLDEN)
    ctx = CKKSContext(HEConfig(m=64, scale_bits=26, q_bits=(55, 26, 26), seed=0))
    kp = ctx.keygen()
    rlk = ctx.relin_keygen(kp.sk)
    gk = ctx.galois_keygen(kp.sk, steps=[1, -1], conjugate=True)
    rng = np.random.default_rng(5)
    v1, v2 = rng.normal(size=32) * 0.5, rng.normal(size=32) * 0.5
    ct1 = ctx.encrypt(ctx.encode(v1), kp.pk)
    ct2 = ctx.encrypt(ctx.encode(v2), kp.pk)

    def same(name, t):
        assert torch.equal(t, torch.from_numpy(gold[name])), name

    same("rlk", rlk)
    assert sorted(f"gk_{g}" for g in gk) == sorted(
        k for k in gold.files if k.startswith("gk_"))
    for g, key in gk.items():
        same(f"gk_{g}", key)
    same("mul_ct", ctx.mul_ct(ct1, ct2, rlk).data)
    same("rotate_1", ctx.rotate(ct1, 1, gk).data)
    many = ctx.rotate_many(ct1, [1, -1], gk, conjugate=True)
    assert len(many) == 3
    for i, r in enumerate(many):
        same(f"rotate_many_{i}", r.data)


@pytest.fixture(scope="module")
def deep():
    """L = 4 chain with two top-level ciphertexts and their level-3 forms:
    each a top-level ct x ct by an encrypted all-ones vector, rescaled."""
    ctx = CKKSContext(HEConfig(m=64, scale_bits=26, q_bits=(55, 26, 26, 26),
                               seed=0))
    kp = ctx.keygen()
    rlk = ctx.relin_keygen(kp.sk)
    rng = np.random.default_rng(5)
    v1, v2 = rng.normal(size=32) * 0.5, rng.normal(size=32) * 0.5
    ct1 = ctx.encrypt(ctx.encode(v1), kp.pk)
    ct2 = ctx.encrypt(ctx.encode(v2), kp.pk)
    ones = ctx.encrypt(ctx.encode(np.ones(32)), kp.pk)
    l1 = ctx.rescale(ctx.mul_ct(ct1, ones, rlk))
    l2 = ctx.rescale(ctx.mul_ct(ct2, ones, rlk))
    assert l1.level == l2.level == 3
    return SimpleNamespace(ctx=ctx, kp=kp, rlk=rlk, v1=v1, v2=v2,
                           ct1=ct1, ct2=ct2, l1=l1, l2=l2)


def _assert_residues(ctx, ct):
    for i in range(ct.level):
        limb = ct.data[..., i, :]
        assert limb.min().item() >= 0 and limb.max().item() < ctx.primes[i], i


def test_mul_ct_below_top_level(deep):
    """mul_ct at levels 3, 2 and 1 of an L = 4 chain.

    Decoded: level 3 against v1*v2 and level 2 against the square of what
    its operand decodes to, each after one rescale and within 1e-3, the
    bound test_mul_ct_relin_rescale sets for one multiply + rescale at this
    scale. At both the product (scale ~2^52) sits far below the remaining
    modulus (~2^107 and ~2^81). Not decoded: level 1, where the product at
    scale ~2^52 has only the 55-bit q_0 left — no limb to rescale into and
    three bits for value and noise together; there mul_ct must run and
    return valid residues."""
    ctx, sk, rlk = deep.ctx, deep.kp.sk, deep.rlk

    def dec(ct):
        return ctx.decode(ctx.decrypt(ct, sk), 32)

    p3 = ctx.mul_ct(deep.l1, deep.l2, rlk)
    assert p3.level == 3
    _assert_residues(ctx, p3)
    x2 = ctx.rescale(p3)
    err3 = np.abs(dec(x2) - deep.v1 * deep.v2).max()
    print(f"level 3: max error {err3:.3g}")
    assert err3 < 1e-3

    p2 = ctx.mul_ct(x2, x2, rlk)
    assert p2.level == 2
    _assert_residues(ctx, p2)
    x1 = ctx.rescale(p2)
    err2 = np.abs(dec(x1) - dec(x2) ** 2).max()
    print(f"level 2: max error {err2:.3g}")
    assert err2 < 1e-3

    p1 = ctx.mul_ct(x1, x1, rlk)
    assert p1.level == 1 and p1.data.shape == (2, 1, ctx.n)
    _assert_residues(ctx, p1)


def test_mul_ct_argument_checks(deep):
    ctx = deep.ctx
    with pytest.raises(ValueError, match="same level"):
        ctx.mul_ct(deep.ct1, deep.l2, deep.rlk)
    with pytest.raises(ValueError, match="relinearization"):
        ctx.mul_ct(deep.ct1, deep.ct2, None)


@pytest.mark.parametrize("below_top", [False, True])
def test_mul_ct_batched_equals_single_calls(deep, below_top):
    """a [3, 2, l, n] x b [2, l, n] (the form scripts/bench_he.py and
    fl/secure.py use) is the three single products stacked, at l = L and
    l = L - 1."""
    ctx, rlk = deep.ctx, deep.rlk
    if below_top:
        a, b = deep.l1, deep.l2
    else:
        a, b = deep.ct1, deep.ct2
    rows = [a.data, b.data, ctx.add(a, a).data]
    batch = Ciphertext(torch.stack(rows), a.scale)
    assert batch.data.shape == (3, 2, a.level, ctx.n)
    got = ctx.mul_ct(batch, b, rlk)
    want = torch.stack([ctx.mul_ct(Ciphertext(r, a.scale), b, rlk).data
                        for r in rows])
    assert got.data.shape == want.shape
    assert torch.equal(got.data, want)
