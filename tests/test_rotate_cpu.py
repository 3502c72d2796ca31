"""CKKS slot rotation / conjugation on the exact CPU backend.

Correctness is an integer statement: decrypt input and output to exact
centred big-int coefficients (CRT over the level's limbs) and bound
    max |coeffs(rot(ct)) - sigma_g(coeffs(ct))|
by the worst case of one hybrid key-switch at level l,

    l * n * 21 * q_max / P  +  (n + 1) / 2  +  1

(l digits < q_max times an eta=21 CBD error |e| <= 21 over n terms, divided
by P at the mod-down; the mod-down rounding adds 1/2 on ks0 and 1/2 times a
ternary s of at most n terms on ks1; +1 for the two floors). A decoded slot
sees at most n times a coefficient error (the special FFT sums n terms of
modulus 1), so slot tolerances are that bound * n / scale per hop, on top of
the encode/encrypt error measured on the unrotated ciphertext.

Observed: deviations 4-6 against bounds 36-37 at n=64, 62-101 against
10882-16258 at n=256.
"""
import functools
import math
import pickle

import numpy as np
import pytest
import torch

from hefl.config import HEConfig
from hefl.he import CKKSContext, CtxtTensor, Pyfhel
from hefl.he.ntt_cpu import NttTables, fwd_ntt

# (n, chain, scale_bits)
PARAMS = {"n64": (64, (50, 30, 30), 30), "n256": (256, (60, 40, 40), 40)}


@functools.lru_cache(maxsize=None)
def _setup(name):
    """Context, keys (default +-2^k steps, the issue's extra steps and
    conjugation) and one ciphertext per level, shared by every test."""
    n, chain, sb = PARAMS[name]
    ctx = CKKSContext(HEConfig(m=n, scale_bits=sb, q_bits=chain, seed=11))
    kp = ctx.keygen()
    gk_pow2 = ctx.galois_keygen(kp.sk)
    gk = dict(gk_pow2)
    gk.update(ctx.galois_keygen(kp.sk, steps=[3], conjugate=True))
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, ctx.slots)
    top = ctx.encrypt(ctx.encode(v), kp.pk)
    cts = {ctx.L: top}
    ct = top
    while ct.level > 1:
        ct = ctx.rescale(ctx.mul_scalar(ct, 1.0))
        cts[ct.level] = ct
    return ctx, kp, gk, gk_pow2, v, cts


def _hop_bound(ctx, l):
    """Worst-case coefficient error of one key-switch at level l."""
    q_max = max(ctx.primes[:l])
    return l * ctx.n * 21 * q_max / ctx.special + (ctx.n + 1) / 2 + 1


def _slot_tol(ctx, l, scale, hops=1):
    return hops * _hop_bound(ctx, l) * ctx.n / scale


def _coeffs(ctx, ct, sk):
    """Exact centred big-int coefficients of the decryption of ct."""
    pt = ctx.decrypt(ct, sk).data
    l = pt.shape[-2]
    qs = ctx.primes[:l]
    Q = math.prod(qs)
    x = 0
    for i, q in enumerate(qs):
        c = ctx.backend.ntt(pt[i], i, inverse=True).numpy().astype(object)
        Qi = Q // q
        x = x + c * ((Qi * pow(Qi % q, -1, q)) % Q)
    x = np.mod(x, Q)
    return np.where(x > Q // 2, x - Q, x)


def _sigma(c, g):
    """a(X) -> a(X^g) on a coefficient vector, straight from the definition:
    coefficient j moves to j*g mod 2n, negated past X^n."""
    n = len(c)
    out = np.zeros_like(c)
    for j in range(n):
        e = (j * g) % (2 * n)
        if e < n:
            out[e] = c[j]
        else:
            out[e - n] = -c[j]
    return out


def _decode(ctx, ct, sk):
    return ctx.decode(ctx.decrypt(ct, sk), ctx.slots)


# ----- the NTT-domain permutation ------------------------------------------

@pytest.mark.parametrize("n", [16, 64])
def test_perm_matches_coefficient_automorphism(n):
    ctx = CKKSContext(HEConfig(m=n, scale_bits=30, q_bits=(40, 30), seed=1))
    q = ctx.primes[0]
    tb = NttTables(q, n)
    a = np.array([int(x) for x in
                  np.random.default_rng(n).integers(0, q, n)], dtype=object)
    a_hat = fwd_ntt(a, tb)
    for g in (5, pow(5, -1, 2 * n), 25, 2 * n - 1):
        perm = ctx._galois_tables(g).perm.numpy()
        assert sorted(perm.tolist()) == list(range(n))
        want = fwd_ntt(np.mod(_sigma(a, g), q), tb)
        assert np.array_equal(a_hat[perm], want), g


def test_galois_element():
    ctx = _setup("n64")[0]
    assert ctx.galois_element(1) == 5
    assert ctx.galois_element(-1) == pow(5, -1, 128)
    assert ctx.galois_element(ctx.slots) == 1
    assert ctx.galois_element(conjugate=True) == 127
    with pytest.raises(ValueError):
        ctx.galois_element()


def test_galois_key_shape_and_determinism():
    ctx, kp, gk, gk_pow2, _, _ = _setup("n64")
    slots = ctx.slots
    want = {ctx.galois_element(s * 2 ** k)
            for k in range(slots.bit_length() - 1) for s in (1, -1)}
    assert set(gk_pow2) == want
    for t in gk.values():
        assert t.shape == (ctx.L, 2, ctx.L + 1, ctx.n) and t.dtype == torch.int64
    n, chain, sb = PARAMS["n64"]
    again = CKKSContext(HEConfig(m=n, scale_bits=sb, q_bits=chain, seed=11))
    kp2 = again.keygen()
    gk2 = again.galois_keygen(kp2.sk)
    assert all(torch.equal(gk2[g], gk_pow2[g]) for g in gk_pow2)


# ----- rotation as an exact integer statement --------------------------------

@pytest.mark.parametrize("below_top", [False, True])
@pytest.mark.parametrize("op", ["1", "-1", "3", "half", "conj"])
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_rotation_exact_coefficients_and_slots(name, op, below_top):
    ctx, kp, gk, _, v, cts = _setup(name)
    l = ctx.L - 1 if below_top else ctx.L
    ct = cts[l]
    if op == "conj":
        g, want_slots = ctx.galois_element(conjugate=True), v
        out = ctx.conjugate(ct, gk)
    else:
        r = ctx.slots // 2 if op == "half" else int(op)
        g, want_slots = ctx.galois_element(r), np.roll(v, -r)
        out = ctx.rotate(ct, r, gk)
    assert g in gk                       # one hop: the exact key is present
    assert out.level == l and out.scale == ct.scale
    dev = int(np.abs(_coeffs(ctx, out, kp.sk)
                     - _sigma(_coeffs(ctx, ct, kp.sk), g)).max())
    bound = _hop_bound(ctx, l)
    print(f"{name} l={l} {op}: coefficient deviation {dev}, bound {bound:.1f}")
    # dev <= l*n*21*q_max/P + (n+1)/2 + 1, in integers
    q_max, P, n = max(ctx.primes[:l]), ctx.special, ctx.n
    assert 2 * P * dev <= 2 * l * n * 21 * q_max + (n + 1) * P + 2 * P
    enc_err = np.abs(_decode(ctx, ct, kp.sk) - v).max()
    err = np.abs(_decode(ctx, out, kp.sk) - want_slots).max()
    tol = _slot_tol(ctx, l, ct.scale) + enc_err
    print(f"  slot error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("step", ["3", "-5", "slots-1"])
def test_naf_composition_over_power_of_two_keys(step):
    ctx, kp, _, gk_pow2, v, cts = _setup("n64")
    r = ctx.slots - 1 if step == "slots-1" else int(step)
    hops = len(ctx._rotation_hops(r, gk_pow2))
    assert hops == {"3": 2, "-5": 2, "slots-1": 1}[step]
    ct = cts[ctx.L]
    out = ctx.rotate(ct, r, gk_pow2)
    enc_err = np.abs(_decode(ctx, ct, kp.sk) - v).max()
    err = np.abs(_decode(ctx, out, kp.sk) - np.roll(v, -r)).max()
    assert err <= _slot_tol(ctx, ctx.L, ct.scale, hops) + enc_err


def test_step_zero_needs_no_key():
    ctx, kp, _, _, _, cts = _setup("n64")
    ct = cts[ctx.L]
    for step in (0, ctx.slots, -ctx.slots):
        out = ctx.rotate(ct, step, None)
        assert torch.equal(out.data, ct.data)
        assert out.data.data_ptr() != ct.data.data_ptr()


def test_missing_key_raises():
    ctx, kp, gk, gk_pow2, _, cts = _setup("n64")
    ct = cts[ctx.L]
    only1 = {ctx.galois_element(1): gk[ctx.galois_element(1)]}
    with pytest.raises(ValueError, match=r"step 2\b"):
        ctx.rotate(ct, 2, only1)
    with pytest.raises(ValueError, match="step -1"):
        ctx.rotate(ct, 3, only1)         # 3 = 4 - 1
    with pytest.raises(ValueError, match="galois_keygen"):
        ctx.rotate(ct, 1, None)
    with pytest.raises(ValueError, match="conjugat"):
        ctx.conjugate(ct, gk_pow2)
    with pytest.raises(ValueError, match="threshold"):
        ctx.galois_keygen(None)


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_level_one(name):
    ctx, kp, gk, _, v, cts = _setup(name)
    ct = cts[1]
    assert ct.level == 1
    out = ctx.rotate(ct, 1, gk)
    dev = int(np.abs(_coeffs(ctx, out, kp.sk)
                     - _sigma(_coeffs(ctx, ct, kp.sk), 5)).max())
    assert dev <= _hop_bound(ctx, 1)
    enc_err = np.abs(_decode(ctx, ct, kp.sk) - v).max()
    err = np.abs(_decode(ctx, out, kp.sk) - np.roll(v, -1)).max()
    assert err <= _slot_tol(ctx, 1, ct.scale) + enc_err


# ----- sum_slots -------------------------------------------------------------
# Each rotate-and-add round doubles the error already present and adds one
# hop's: after log2(w) rounds at most w * err_0 + (w - 1) * hop.

def _windowed(v, w):
    return sum(np.roll(v, -t) for t in range(w))


@pytest.mark.parametrize("width", ["full", "4"])
def test_sum_slots(width):
    ctx, kp, _, gk_pow2, _, _ = _setup("n64")
    w = ctx.slots if width == "full" else int(width)
    v = np.arange(ctx.slots, dtype=np.float64) / 8 - 1.5
    ct = ctx.encrypt(ctx.encode(v), kp.pk)
    out = ctx.sum_slots(ct, gk_pow2, w)
    assert out.level == ct.level and out.scale == ct.scale
    enc_err = np.abs(_decode(ctx, ct, kp.sk) - v).max()
    tol = w * enc_err + (w - 1) * _slot_tol(ctx, ctx.L, ct.scale)
    got = _decode(ctx, out, kp.sk)
    assert np.abs(got - _windowed(v, w)).max() <= tol
    if width == "full":
        assert np.abs(got - v.sum()).max() <= tol
    with pytest.raises(ValueError):
        ctx.sum_slots(ct, gk_pow2, 3)
    with pytest.raises(ValueError):
        ctx.sum_slots(ct, gk_pow2, 2 * ctx.slots)


def test_sum_of_squares_below_top_level():
    """mul_ct at the top level, rescale, then sum_slots at level L-1."""
    ctx, kp, _, gk_pow2, v, cts = _setup("n256")
    rlk = ctx.relin_keygen(kp.sk)
    ct = cts[ctx.L]
    sq = ctx.rescale(ctx.mul_ct(ct, ct, rlk))
    assert sq.level == ctx.L - 1
    out = ctx.sum_slots(sq, gk_pow2, ctx.slots)
    assert out.level == ctx.L - 1
    w = ctx.slots
    sq_err = np.abs(_decode(ctx, sq, kp.sk) - v * v).max()
    tol = w * sq_err + (w - 1) * _slot_tol(ctx, sq.level, sq.scale)
    got = _decode(ctx, out, kp.sk)
    print(f"sum x^2: error {np.abs(got - (v * v).sum()).max():.3e}, tol {tol:.3e}")
    assert np.abs(got - (v * v).sum()).max() <= tol


# ----- batched --------------------------------------------------------------

@pytest.mark.parametrize("below_top", [False, True])
def test_rotate_tensor_matches_per_row(below_top):
    ctx, kp, gk, gk_pow2, _, _ = _setup("n64")
    vec = torch.from_numpy(np.random.default_rng(2).uniform(
        -1, 1, 3 * ctx.slots - 5)).float()
    ct = ctx.encrypt_tensor(vec, kp.pk)
    if below_top:
        ct = ctx.rescale_tensor(ctx.mul_scalar_tensor(ct, 1.0))
    assert ct.data.shape == (3, 2, ct.level, ctx.n)
    for step, keys in ((1, gk), (3, gk_pow2)):
        out = ctx.rotate_tensor(ct, step, keys)
        assert out.count == ct.count and out.scale == ct.scale
        for b in range(3):
            row = ctx.rotate_data(ct.data[b], step, keys)
            assert torch.equal(out.data[b], row)
    out = ctx.conjugate_tensor(ct, gk)
    assert torch.equal(out.data[1], ctx.conjugate_data(ct.data[1], gk))
    s = ctx.sum_slots_tensor(ct, gk_pow2, 4)
    assert torch.equal(s.data[2], ctx.sum_slots_data(ct.data[2], gk_pow2, 4))


# ----- Pyfhel facade -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _facade():
    he = Pyfhel()
    he.contextGen(m=64, scale_bits=30, q_bits=(50, 30, 30), seed=4)
    he.keyGen()
    he.rotateKeyGen()
    return he


def test_facade_rotate_key_gen():
    he = _facade()
    ctx = he.context
    gk = he._keys.galois
    assert ctx.galois_element(conjugate=True) in gk
    assert all(ctx.galois_element(s) in gk
               for s in ctx.default_rotation_steps())
    fresh = Pyfhel()
    fresh.contextGen(m=64, scale_bits=30, q_bits=(50, 30, 30), seed=4)
    with pytest.raises(ValueError):
        fresh.rotateKeyGen()


def test_facade_shift_operators():
    he = _facade()
    ctx = he.context
    ct = he.encryptFrac(0.75)
    base = he.decryptFrac(ct)
    hop = _slot_tol(ctx, ct._ct.level, ct._ct.scale)
    enc_err = abs(base - 0.75)
    away = ct >> 1                       # slot 0 -> slot 1
    assert abs(he.decryptFrac(away)) <= hop + enc_err
    slots = ctx.decode(ctx.decrypt(away._ct, he._sk), ctx.slots)
    assert abs(slots[1] - 0.75) <= hop + enc_err
    back = away << 1
    assert abs(he.decryptFrac(back) - 0.75) <= 2 * hop + enc_err
    assert abs(he.decryptFrac(he.rotate(ct, 0)) - base) == 0
    conj = he.conjugate(ct)
    assert abs(he.decryptFrac(conj) - 0.75) <= hop + enc_err
    t = he.encrypt_tensor(torch.arange(40, dtype=torch.float32) / 40)
    rt = he.rotate(t, 2)
    assert isinstance(rt, CtxtTensor) and rt.count == t.count
    assert torch.equal(rt.data, ctx.rotate_data(t.data, 2, he._keys.galois))


def test_facade_rotate_key_bytes_round_trip():
    he = _facade()
    buf = he.to_bytes_rotateKey()
    other = Pyfhel()
    other.from_bytes_rotateKey(buf)      # builds the context from the header
    assert other.context.cfg.q_bits == he.context.cfg.q_bits
    gk, gk2 = he._keys.galois, other._keys.galois
    assert list(gk2) == list(gk)
    assert all(torch.equal(gk[g], gk2[g]) for g in gk)
    with pytest.raises(ValueError):
        other.from_bytes_rotateKey(he.to_bytes_publicKey())
    with pytest.raises(ValueError):
        Pyfhel().to_bytes_rotateKey()


def test_facade_pickle_carries_rotate_keys():
    he = _facade()
    clone = pickle.loads(pickle.dumps(he))
    assert clone._sk is None             # the secret key is never pickled
    gk, gk2 = he._keys.galois, clone._keys.galois
    assert set(gk2) == set(gk) and all(torch.equal(gk[g], gk2[g]) for g in gk)
    ct = he.encryptFrac(-0.5)
    moved = clone.rotate(ct, -1)         # evaluation needs no secret key
    assert torch.equal(moved._ct.data, (ct >> 1)._ct.data)
    # a state written before rotation keys existed
    old = Pyfhel()
    old.__setstate__({"cfg": he.context.cfg, "pk": he._pk.numpy()})
    assert old._galois is None and torch.equal(old._pk, he._pk)
    bare = Pyfhel()
    bare.contextGen(m=64, scale_bits=30, q_bits=(50, 30, 30), seed=4)
    bare.keyGen()
    assert "galois" not in bare.__getstate__()
    assert pickle.loads(pickle.dumps(bare))._galois is None
