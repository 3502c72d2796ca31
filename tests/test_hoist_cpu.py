"""Hoisted multi-step rotations and the encrypted linear transform on the
exact CPU backend (the oracle the device path is compared to).

Hoisting applies the automorphism AFTER the digit lift, as the NTT-domain
permutation perm_g of the shared digits D. The permuted digit is the transform
of the signed sigma_g of the lifted digit (-v at a wrapped coefficient) where
rotate() lifts q_d - v; test_digit_identity pins exactly that. Both digits are
congruent to sigma_g(c) mod q_d and have |digit| < q_d <= q_max, and the
one-hop bound of test_rotate_cpu.py,

    l * n * 21 * q_max / P  +  (n + 1) / 2  +  1,

uses nothing else about the digits (l digits below q_max times an eta = 21
error over n terms, divided by P; the mod-down rounding adds 1/2 on ks0 and
1/2 times a ternary s of at most n terms on ks1; +1 for the two floors). So it
holds for rotate_many unchanged, although the low bits differ from rotate()'s.

Linear transform: with E = coeffs(out) - sum_b ptcoef_b (*) sigma_b(coeffs(ct))
mod Q, centred ((*) the negacyclic product),

    max|E| <= sum_{b, step != 0} |pt_b|_inf * l * n^2 * 21 * q_max / P
              + (n + 1) / 2 + 1.

Per digit |digit (*) e| <= n * q_max * 21, l digits, a further negacyclic
product with pt_b multiplies by at most n * |pt_b|_inf, all of it divided by
P, and the ONE mod-down adds the same rounding term as a single hop. The
step-0 diagonal and the c0 terms are exact. |pt_b|_inf is taken from the
encoder's coefficients of each diagonal.

Observed (printed by the tests): rotate_many coefficient deviations 3-5
against bounds 36-37 at n = 64 and 63-117 against 10882-16258 at n = 256,
decoded slots within 7e-8 (n = 64) / 7e-9 (n = 256) of rotate()'s against
tolerances of 4e-6 / 5e-6 to 8e-6; linear transform max|E| 3.3e7 against
9.8e10 (n = 64, top level, 10 keyed diagonals), 3.4e7 against 6.5e10 (n = 64,
one below), 9.4e13 against 1.5e18 (n = 256, top, 22 keyed diagonals) and
5.4e13 against 1.0e18 (n = 256, one below); slot errors of the transform
3.4e-7 against the composed path's 3.3e-7 at n = 64 (max|Mv| 0.92) and 1.7e-9
against 4.4e-9 at n = 256 (max|Mv| 2.71).
"""
import functools
import math

import numpy as np
import pytest
import torch

from hefl.config import HEConfig
from hefl.he import CKKSContext, CtxtTensor, LinearTransform, Pyfhel, PyCtxt
from hefl.he.ntt_cpu import NttTables, fwd_ntt

# (n, chain, scale_bits) — the fixtures' parameters of test_rotate_cpu.py
PARAMS = {"n64": (64, (50, 30, 30), 30), "n256": (256, (60, 40, 40), 40)}
MAT_SHAPE = {"n64": (4, 8), "n256": (8, 16)}


def _steps(ctx):
    return [1, -1, 3, ctx.slots // 2]


@functools.lru_cache(maxsize=None)
def _setup(name):
    """Context, exact-step keys (+ conjugation) and one ciphertext per level."""
    n, chain, sb = PARAMS[name]
    ctx = CKKSContext(HEConfig(m=n, scale_bits=sb, q_bits=chain, seed=11))
    kp = ctx.keygen()
    gk = ctx.galois_keygen(kp.sk, steps=_steps(ctx), conjugate=True)
    v = np.random.default_rng(5).uniform(-1, 1, ctx.slots)
    top = ctx.encrypt(ctx.encode(v), kp.pk)
    cts = {ctx.L: top}
    ct = top
    while ct.level > 1:
        ct = ctx.rescale(ctx.mul_scalar(ct, 1.0))
        cts[ct.level] = ct
    return ctx, kp, gk, v, cts


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
    """a(X) -> a(X^g) on a coefficient vector, from the definition."""
    n = len(c)
    out = np.zeros_like(c)
    for j in range(n):
        e = (j * g) % (2 * n)
        if e < n:
            out[e] = c[j]
        else:
            out[e - n] = -c[j]
    return out


def _negacyclic(a, b):
    """a (*) b mod X^n + 1 on big-int object vectors."""
    n = len(a)
    out = np.zeros(n, dtype=object)
    for j in range(n):
        if a[j] == 0:
            continue
        out[j:] += a[j] * b[:n - j]
        out[:j] -= a[j] * b[n - j:]
    return out


def _decode(ctx, ct, sk):
    return ctx.decode(ctx.decrypt(ct, sk), ctx.slots)


# ----- 1. the one subtle point: which digit the permutation transforms -------

@pytest.mark.parametrize("name", sorted(PARAMS))
def test_digit_identity(name):
    ctx, kp, gk, v, cts = _setup(name)
    l, n = ctx.L, ctx.n
    c1 = cts[l].data[1]
    dig = ctx._hoist_digits(c1, l)
    assert dig.shape == (l, l + 1, n) and dig.dtype == torch.int64
    idx = list(range(l)) + [ctx.L]
    for g in (5, pow(5, -1, 2 * n), 2 * n - 1):
        gt = ctx._galois_tables(g)
        got = dig.index_select(-1, gt.perm).numpy()
        differs = 0
        for d in range(l):
            qd = ctx.primes[d]
            c = ctx.backend.ntt(c1[d], d, inverse=True)      # in [0, q_d)
            signed = _sigma(c.numpy().astype(object), g)     # -v where wrapped
            old = ctx._coeff_automorphism(c, qd, gt).numpy().astype(object)
            for j, i in enumerate(idx):
                q = ctx._q(i)
                tb = NttTables(q, n)
                want = fwd_ntt(np.mod(signed, q), tb).astype(np.int64)
                assert np.array_equal(got[d, j], want), (g, d, i)
                lifted = fwd_ntt(np.mod(old, q), tb).astype(np.int64)
                if i == d:        # q_d - v == -v mod q_d: same residues
                    assert np.array_equal(got[d, j], lifted)
                else:
                    differs += int(not np.array_equal(got[d, j], lifted))
        # rotate()'s digit (q_d - v lifted) is another representative
        assert differs == l * l, (g, differs)


# ----- 2. rotate_many as an exact integer statement ---------------------------

@pytest.mark.parametrize("below_top", [False, True])
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_rotate_many_coefficient_bound(name, below_top):
    ctx, kp, gk, v, cts = _setup(name)
    l = ctx.L - 1 if below_top else ctx.L
    ct = cts[l]
    steps = _steps(ctx)
    outs = ctx.rotate_many(ct, steps, gk, conjugate=True)
    assert len(outs) == len(steps) + 1
    base = _coeffs(ctx, ct, kp.sk)
    q_max, P, n = max(ctx.primes[:l]), ctx.special, ctx.n
    bound = _hop_bound(ctx, l)
    labels = [str(s) for s in steps] + ["conj"]
    for label, out in zip(labels, outs):
        if label == "conj":
            g = ctx.galois_element(conjugate=True)
            ref = ctx.conjugate(ct, gk)
        else:
            g = ctx.galois_element(int(label))
            ref = ctx.rotate(ct, int(label), gk)
        assert out.level == l and out.scale == ct.scale
        dev = int(np.abs(_coeffs(ctx, out, kp.sk) - _sigma(base, g)).max())
        print(f"{name} l={l} {label}: coefficient deviation {dev}, "
              f"bound {bound:.1f}")
        # dev <= l*n*21*q_max/P + (n+1)/2 + 1, in integers
        assert 2 * P * dev <= 2 * l * n * 21 * q_max + (n + 1) * P + 2 * P
        # a valid rotation with other low bits than rotate()'s
        assert not torch.equal(out.data, ref.data)
        diff = np.abs(_decode(ctx, out, kp.sk) - _decode(ctx, ref, kp.sk)).max()
        tol = 2 * _slot_tol(ctx, l, ct.scale)
        print(f"  slots vs rotate(): {diff:.3e}, tolerance {tol:.3e}")
        assert diff <= tol


# ----- 3. rotate_many interface -----------------------------------------------

@pytest.mark.parametrize("below_top", [False, True])
def test_rotate_many_tensor_matches_per_row(below_top):
    ctx, kp, gk, _, _ = _setup("n64")
    vec = torch.from_numpy(np.random.default_rng(2).uniform(
        -1, 1, 3 * ctx.slots - 5)).float()
    ct = ctx.encrypt_tensor(vec, kp.pk)
    if below_top:
        ct = ctx.rescale_tensor(ctx.mul_scalar_tensor(ct, 1.0))
    assert ct.data.shape == (3, 2, ct.level, ctx.n)
    steps = [3, 0, -1, 3, ctx.slots]            # order, duplicate, zeros
    outs = ctx.rotate_many_tensor(ct, steps, gk, conjugate=True)
    assert len(outs) == len(steps) + 1
    for out in outs:
        assert isinstance(out, CtxtTensor)
        assert out.count == ct.count and out.scale == ct.scale
        assert out.data.shape == ct.data.shape
    for b in range(3):
        rows = ctx.rotate_many_data(ct.data[b], steps, gk, conjugate=True)
        for out, row in zip(outs, rows):
            assert torch.equal(out.data[b], row)
    # step 0 (and a multiple of slots): a clone, not the input itself
    for j in (1, 4):
        assert torch.equal(outs[j].data, ct.data)
        assert outs[j].data.data_ptr() != ct.data.data_ptr()
    # duplicates: same bits, separate storage
    assert torch.equal(outs[0].data, outs[3].data)
    assert outs[0].data.data_ptr() != outs[3].data.data_ptr()
    # order: each entry is its own step's rotation
    single = ctx.rotate_many_tensor(ct, [-1], gk)[0]
    assert torch.equal(outs[2].data, single.data)
    assert not torch.equal(outs[0].data, single.data)
    conj = ctx.rotate_many_tensor(ct, [], gk, conjugate=True)
    assert len(conj) == 1 and torch.equal(conj[0].data, outs[-1].data)


def test_rotate_many_missing_key_raises():
    ctx, kp, gk, _, cts = _setup("n64")
    ct = cts[ctx.L]
    with pytest.raises(ValueError, match=r"missing steps \[2\].*"
                                         r"galois_keygen\(sk, steps=\[2\]\)"):
        ctx.rotate_many(ct, [1, 2], gk)
    # 2 = 1 + 1 would compose for rotate(); a hoisted step needs its own key
    only1 = {ctx.galois_element(1): gk[ctx.galois_element(1)]}
    with pytest.raises(ValueError, match=r"\[-1, 3\]"):
        ctx.rotate_many(ct, [3, 1, -1], only1)
    with pytest.raises(ValueError, match="galois_keygen"):
        ctx.rotate_many(ct, [1], None)
    with pytest.raises(ValueError, match="conjugat"):
        ctx.rotate_many(ct, [1], only1, conjugate=True)
    assert len(ctx.rotate_many(ct, [0], None)) == 1     # step 0 needs no key


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_rotate_many_level_one(name):
    ctx, kp, gk, v, cts = _setup(name)
    ct = cts[1]
    assert ct.level == 1
    outs = ctx.rotate_many(ct, [1, -1], gk)
    base = _coeffs(ctx, ct, kp.sk)
    enc_err = np.abs(_decode(ctx, ct, kp.sk) - v).max()
    for r, out in zip((1, -1), outs):
        assert out.level == 1
        dev = int(np.abs(_coeffs(ctx, out, kp.sk)
                         - _sigma(base, ctx.galois_element(r))).max())
        assert dev <= _hop_bound(ctx, 1)
        err = np.abs(_decode(ctx, out, kp.sk) - np.roll(v, -r)).max()
        assert err <= _slot_tol(ctx, 1, ct.scale) + enc_err


# ----- 4. / 5. the linear transform -------------------------------------------

@functools.lru_cache(maxsize=None)
def _lt_case(name, below_top):
    """Matrix, vector, transform, its keys and the input ciphertext."""
    ctx, kp, _, _, _ = _setup(name)
    r, c = MAT_SHAPE[name]
    rng = np.random.default_rng(17)
    M = rng.uniform(-1, 1, (r, c))
    v = rng.uniform(-1, 1, c)
    ct = ctx.encrypt(ctx.encode(v), kp.pk)
    if below_top:
        ct = ctx.rescale(ctx.mul_scalar(ct, 1.0))
    lt = LinearTransform(ctx, M, level=ct.level)
    gk = ctx.galois_keygen(kp.sk, steps=lt.steps)
    return ctx, kp, M, v, ct, lt, gk


@pytest.mark.parametrize("below_top", [False, True])
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_linear_transform_coefficient_bound(name, below_top):
    ctx, kp, M, v, ct, lt, gk = _lt_case(name, below_top)
    l, n = ct.level, ctx.n
    out = lt.apply(ct, gk)
    assert out.level == l and out.scale == ct.scale * lt.scale
    full = np.zeros((ctx.slots, ctx.slots))
    full[:M.shape[0], :M.shape[1]] = M
    j = np.arange(ctx.slots)
    base = _coeffs(ctx, ct, kp.sk)
    Q = math.prod(ctx.primes[:l])
    want = np.zeros(n, dtype=object)
    norm_sum = 0
    for k in lt.diag_steps:
        ptc = ctx.encoder.encode(full[j, (j + k) % ctx.slots],
                                 lt.scale).astype(object)
        want = want + _negacyclic(ptc, _sigma(base, ctx.galois_element(k)))
        if k != 0:
            norm_sum += int(np.abs(ptc).max())
    E = np.mod(_coeffs(ctx, out, kp.sk) - want, Q)
    E = np.where(E > Q // 2, E - Q, E)
    dev = int(np.abs(E).max())
    q_max, P = max(ctx.primes[:l]), ctx.special
    bound = norm_sum * l * n * n * 21 * q_max / P + (n + 1) / 2 + 1
    print(f"{name} l={l}: max|E| {dev:.3e}, bound {bound:.3e} "
          f"({len(lt.steps)} keyed diagonals)")
    # dev <= norm_sum*l*n^2*21*q_max/P + (n+1)/2 + 1, in integers
    assert 2 * P * dev <= (2 * norm_sum * l * n * n * 21 * q_max
                           + (n + 1) * P + 2 * P)


def _composed(ctx, ct, lt, M, gk):
    """The same product from the existing ops: rotate with exact keys,
    mul_plain, add (rescaled by the caller)."""
    full = np.zeros((ctx.slots, ctx.slots))
    full[:M.shape[0], :M.shape[1]] = M
    j = np.arange(ctx.slots)
    acc = None
    for k in lt.diag_steps:
        pt = ctx.encode(full[j, (j + k) % ctx.slots], nlimbs=ct.level,
                        scale=lt.scale)
        term = ctx.mul_plain(ctx.rotate(ct, k, gk), pt)
        acc = term if acc is None else ctx.add(acc, term)
    return acc


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_linear_transform_slot_accuracy(name):
    ctx, kp, M, v, ct, lt, gk = _lt_case(name, False)
    want = np.zeros(ctx.slots)
    want[:M.shape[0]] = M @ v
    peak = np.abs(want).max()
    new = ctx.rescale(lt.apply(ct, gk))
    ref = ctx.rescale(_composed(ctx, ct, lt, M, gk))
    assert new.level == ref.level == ct.level - 1
    assert abs(new.scale - ref.scale) <= 1e-9 * ref.scale
    err_new = np.abs(_decode(ctx, new, kp.sk) - want).max()
    err_ref = np.abs(_decode(ctx, ref, kp.sk) - want).max()
    print(f"{name}: err_new {err_new:.3e}, err_ref {err_ref:.3e}, "
          f"max|Mv| {peak:.3f}")
    assert err_ref < 1e-4 * peak and err_new < 1e-4 * peak
    assert err_new <= 4 * err_ref


# ----- 6. structure -----------------------------------------------------------

def test_linear_transform_steps_are_the_nonzero_diagonals():
    ctx = _setup("n64")[0]
    slots = ctx.slots
    M = np.zeros((slots, slots))
    j = np.arange(slots)
    for k in (0, 2, slots - 3):
        M[j, (j + k) % slots] = 0.5
    lt = LinearTransform(ctx, M)
    assert lt.steps == [2, slots - 3] and lt.diag_steps == [0, 2, slots - 3]
    r, c = MAT_SHAPE["n64"]
    dense = LinearTransform(ctx, np.ones((r, c)))
    assert sorted(dense.steps) == sorted(
        k % slots for k in range(-(r - 1), c) if k != 0)
    with pytest.raises(ValueError):
        LinearTransform(ctx, np.zeros((2, 2)))
    with pytest.raises(ValueError):
        LinearTransform(ctx, np.ones((slots + 1, 2)))
    with pytest.raises(ValueError):
        LinearTransform(ctx, np.ones((2, 2)) * 1j)


def test_from_diagonals_equals_the_matrix_form():
    ctx, kp, M, _, ct, lt, gk = _lt_case("n64", False)
    full = np.zeros((ctx.slots, ctx.slots))
    full[:M.shape[0], :M.shape[1]] = M
    j = np.arange(ctx.slots)
    by_diag = LinearTransform.from_diagonals(
        ctx, {k - ctx.slots: full[j, (j + k) % ctx.slots]
              for k in lt.diag_steps})
    assert by_diag.diag_steps == lt.diag_steps and by_diag.steps == lt.steps
    assert torch.equal(by_diag.pt, lt.pt)
    assert torch.equal(by_diag.apply(ct, gk).data, lt.apply(ct, gk).data)


def test_identity_needs_no_key():
    ctx, kp, _, _, cts = _setup("n64")
    ct = cts[ctx.L]
    lt = LinearTransform(ctx, np.eye(ctx.slots))
    assert lt.steps == []
    out = lt.apply(ct, None)
    want = ctx.mul_plain(ct, ctx.encode(np.ones(ctx.slots)))
    assert torch.equal(out.data, want.data) and out.scale == want.scale


def test_step_zero_and_one_other_diagonal():
    ctx, kp, _, v, cts = _setup("n64")
    ct = cts[ctx.L]
    slots = ctx.slots
    j = np.arange(slots)
    M = np.zeros((slots, slots))
    M[j, j] = 0.5
    M[j, (j + 3) % slots] = -0.25
    lt = LinearTransform(ctx, M)
    assert lt.steps == [3]
    gk = ctx.galois_keygen(kp.sk, steps=lt.steps)
    got = _decode(ctx, ctx.rescale(lt.apply(ct, gk)), kp.sk)
    ref = _decode(ctx, ctx.rescale(_composed(ctx, ct, lt, M, gk)), kp.sk)
    want = M @ v
    err_new, err_ref = np.abs(got - want).max(), np.abs(ref - want).max()
    assert err_ref < 1e-4 * np.abs(want).max() and err_new <= 4 * err_ref
    with pytest.raises(ValueError, match=r"missing steps \[3\]"):
        lt.apply(ct, None)


def test_apply_tensor_matches_per_row_and_matvec():
    ctx, kp, M, _, _, lt, gk = _lt_case("n64", False)
    vec = torch.from_numpy(np.random.default_rng(8).uniform(
        -1, 1, 3 * ctx.slots)).float()
    ct = ctx.encrypt_tensor(vec, kp.pk)
    out = lt.apply_tensor(ct, gk)
    assert isinstance(out, CtxtTensor) and out.count == ct.count
    assert out.scale == ct.scale * lt.scale
    for b in range(3):
        assert torch.equal(out.data[b], lt.apply_data(ct.data[b], gk))
    assert torch.equal(ctx.matvec(M, ct, gk).data, out.data)


def test_level_mismatch_and_one_below_top():
    ctx, kp, M, v, ct, lt, gk = _lt_case("n64", True)
    assert ct.level == ctx.L - 1 and lt.level == ctx.L - 1
    top = _setup("n64")[4][ctx.L]
    with pytest.raises(ValueError, match="level"):
        lt.apply(top, gk)
    with pytest.raises(ValueError, match="level"):
        LinearTransform(ctx, M, level=ctx.L + 1)
    want = np.zeros(ctx.slots)
    want[:M.shape[0]] = M @ v
    out = ctx.matvec(M, ct, gk)                  # one-shot, at ct's level
    assert torch.equal(out.data, lt.apply(ct, gk).data)
    got = _decode(ctx, ctx.rescale(out), kp.sk)
    ref = _decode(ctx, ctx.rescale(_composed(ctx, ct, lt, M, gk)), kp.sk)
    err_new, err_ref = np.abs(got - want).max(), np.abs(ref - want).max()
    print(f"one below top: err_new {err_new:.3e}, err_ref {err_ref:.3e}")
    assert err_ref < 1e-4 * np.abs(want).max() and err_new <= 4 * err_ref


def test_level_one_applies_but_cannot_rescale():
    ctx, kp, _, _, cts = _setup("n64")
    ct = cts[1]
    lt = LinearTransform(ctx, np.eye(ctx.slots) * 0.5, level=1)
    out = lt.apply(ct, None)
    assert out.level == 1
    with pytest.raises(AssertionError):
        ctx.rescale(out)


def test_facade_rotate_many_round_trip():
    he = Pyfhel()
    he.contextGen(m=64, scale_bits=30, q_bits=(50, 30, 30), seed=4)
    he.keyGen()
    he.rotateKeyGen(steps=[1, -2])
    ctx = he.context
    ct = he.encryptFrac(0.75)
    outs = he.rotate_many(ct, [1, 0, -2])
    assert len(outs) == 3 and all(isinstance(o, PyCtxt) for o in outs)
    hop = _slot_tol(ctx, ct._ct.level, ct._ct.scale)
    enc_err = abs(he.decryptFrac(ct) - 0.75)
    for k, o in zip((1, 0, -2), outs):
        a = ctx.decode(ctx.decrypt(o._ct, he._sk), ctx.slots)
        b = ctx.decode(ctx.decrypt(he.rotate(ct, k)._ct, he._sk), ctx.slots)
        assert np.abs(a - b).max() <= 2 * hop
        assert abs(a[(-k) % ctx.slots] - 0.75) <= hop + enc_err   # slot 0 moved
    t = he.encrypt_tensor(torch.arange(40, dtype=torch.float32) / 40)
    rt = he.rotate_many(t, [1, -2])
    assert all(isinstance(o, CtxtTensor) and o.count == t.count for o in rt)
    want = ctx.rotate_many_data(t.data, [1, -2], he._keys.galois)
    assert all(torch.equal(o.data, w) for o, w in zip(rt, want))
    with pytest.raises(ValueError, match=r"steps=\[3\]"):
        he.rotate_many(ct, [3])
