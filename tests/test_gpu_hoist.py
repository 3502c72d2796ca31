"""Hoisted rotations and the encrypted linear transform on the MI355X: the
ks_inner_hoisted, galois_perm_add_many, lt_inner and lt_finish HIP kernels
bit-exact against numpy big-int references on planted residues, and
rotate_many_tensor / LinearTransform.apply_tensor bit-exact against the CPU
oracle (same seeded context, keys and ciphertext).

Every path is exact modular arithmetic on canonical residues, so all
comparisons are torch.equal / array_equal. The n = 2^13 case decodes and uses
the accuracy rule of test_hoist_cpu.py: the transform's slot error is at most
4x that of the path composed of rotate, mul_plain, add and rescale (two
independent noise samples of comparable distribution; a wrong permutation,
key or diagonal gives an error of order max|Mv|), both below 1e-4 max|Mv|.
"""
import functools

import numpy as np
import pytest
import torch

from hefl.config import HEConfig

pytestmark = pytest.mark.gpu

CHAINS = {"60-40-40": (60, 40, 40), "50-30-20": (50, 30, 20)}
# (R, n, l)
KERNEL_SHAPES = [(1, 16, 1), (3, 64, 3), (2, 1024, 2)]
GS = [1, 3]


@functools.lru_cache(maxsize=None)
def _ctx(n, q_bits, device, seed=21):
    from hefl.he import CKKSContext
    return CKKSContext(HEConfig(m=n, scale_bits=min(q_bits[1:] or (30,)),
                                q_bits=q_bits, seed=seed), device=device)


def _planted(lead, primes, n, seed):
    """Residues [*lead, len(primes), n] per limb prime: first quarter of each
    row 0, second quarter q - 1, the rest uniform in [0, q)."""
    rng = np.random.default_rng(seed)
    rows = []
    for q in primes:
        r = rng.integers(0, q, size=tuple(lead) + (n,), dtype=np.int64)
        r[..., :n // 4] = 0
        r[..., n // 4:n // 2] = q - 1
        rows.append(r)
    return torch.from_numpy(np.stack(rows, axis=-2))


def _elements(n, G):
    return [5, pow(5, -1, 2 * n), 2 * n - 1][:G]


def _perms(ctx, elements):
    """(int32 device [G, n], numpy [G, n]); element 1 is the identity."""
    rows = [np.arange(ctx.n) if g == 1 else
            ctx._galois_tables(g).perm.cpu().numpy() for g in elements]
    p = np.stack(rows)
    return torch.from_numpy(p.astype(np.int32)).cuda(), p


def _unaligned(t):
    """A device copy of t whose storage starts 8 bytes off a 16-byte line."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:]
    v = buf.view(t.shape).copy_(t.cuda())
    assert v.data_ptr() % 16 == 8
    return v


def _strided(t):
    """A device copy of t with t's shape and a stride of 2 along the rows."""
    buf = torch.empty(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype,
                      device="cuda")
    v = buf[..., ::2].copy_(t.cuda())
    assert not v.is_contiguous()
    return v


def _col(primes):
    return np.array(list(primes), dtype=object).reshape(-1, 1)


def _obj(t):
    return t.numpy().astype(object)


# ----- numpy big-int references ------------------------------------------------

def _ref_inner(dig, keys, perm, targets):
    """[2, G, R, Lp, n]: sum_d dig[r, d, i, perm[g, k]] * keys[g, d, c, i, k]."""
    d, k, qs = _obj(dig), _obj(keys), _col(targets)
    out = []
    for c in range(2):
        out.append(np.stack([
            (d[..., perm[g]] * k[g][:, c][None]).sum(axis=1) % qs
            for g in range(len(perm))]))
    return np.stack(out)


def _ref_perm_add_many(ct, ks0, ks1, perm, primes):
    l = ct.shape[-2]
    qs = _col(primes[:l])
    c0 = _obj(ct[:, 0])
    out0 = np.stack([(c0[..., perm[g]] + _obj(ks0[g])) % qs
                     for g in range(len(perm))]).astype(np.int64)
    return np.stack([out0, ks1.numpy()], axis=2)


def _ref_lt_inner(dig, keys, perm, pt, targets):
    qs = _col(targets)
    inner = _ref_inner(dig, keys, perm, targets)        # [2, G, R, Lp, n]
    p = _obj(pt)[None, :, None]                         # [1, G, 1, Lp, n]
    return ((inner * p) % qs).sum(axis=1) % qs          # [2, R, Lp, n]


def _ref_lt_finish(ct, ks0, ks1, pt, perm, z0, primes):
    l = ct.shape[-2]
    qs = _col(primes[:l])
    c0, c1, p = _obj(ct[:, 0]), _obj(ct[:, 1]), _obj(pt)
    out0, out1 = _obj(ks0), _obj(ks1)
    for g in range(len(perm)):
        out0 = (out0 + c0[..., perm[g]] * p[g][None]) % qs
    if z0 >= 0:
        out1 = (out1 + c1 * p[z0][None]) % qs
    return np.stack([out0, out1], axis=1).astype(np.int64)


def _inner_inputs(ctx, R, n, l, G, seed):
    targets = ctx.primes[:l] + [ctx.special]
    dig = _planted((R, l), targets, n, seed=seed)
    keys = torch.roll(_planted((G, l, 2), targets, n, seed=seed + 1),
                      n // 8, -1)       # (q-1)*(q-1), 0*x, mixed pairs
    pt = torch.roll(_planted((G,), targets, n, seed=seed + 2), n // 3, -1)
    return targets, dig, keys, pt


# ----- ks_inner_hoisted --------------------------------------------------------

@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_ks_inner_hoisted_bit_exact(R, n, l, chain, G):
    ctx = _ctx(n, CHAINS[chain], "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    targets, dig, keys, _ = _inner_inputs(ctx, R, n, l, G, seed=R * n + l + G)
    assert tb.qs.cpu().tolist() == targets
    perm32, perm = _perms(ctx, _elements(n, G))
    acc0, acc1 = be.ks_inner_hoisted(dig.cuda(), keys.cuda(), perm32, tb)
    assert acc0.shape == acc1.shape == (G, R, l + 1, n)
    assert acc0.dtype == torch.int64
    want = _ref_inner(dig, keys, perm, targets).astype(np.int64)
    assert np.array_equal(acc0.cpu().numpy(), want[0])
    assert np.array_equal(acc1.cpu().numpy(), want[1])


def test_ks_inner_hoisted_scalar_path():
    """Keys off a 16-byte boundary take the non-vector kernel; the digits are
    only gathered, so an unaligned digit tensor keeps the vector kernel."""
    n, l, R, G = 64, 2, 3, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    targets, dig, keys, _ = _inner_inputs(ctx, R, n, l, G, seed=9)
    perm32, perm = _perms(ctx, _elements(n, G))
    want = _ref_inner(dig, keys, perm, targets).astype(np.int64)
    for d, k in ((dig.cuda(), _unaligned(keys)), (_unaligned(dig), keys.cuda())):
        acc0, acc1 = be.ks_inner_hoisted(d, k, perm32, tb)
        assert np.array_equal(acc0.cpu().numpy(), want[0])
        assert np.array_equal(acc1.cpu().numpy(), want[1])


def test_ks_inner_hoisted_rejects_bad_arguments():
    n, l, R, G = 64, 2, 2, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    _, dig, keys, _ = _inner_inputs(ctx, R, n, l, G, seed=1)
    dig, keys = dig.cuda(), keys.cuda()
    perm32, _ = _perms(ctx, _elements(n, G))
    f = be._C.ks_inner_hoisted
    f(dig, keys, perm32, tb.qs, tb.ratio_words)                  # accepted
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32.long(), tb.qs, tb.ratio_words)       # dtype
    with pytest.raises(RuntimeError):
        f(dig, keys[:, :1].contiguous(), perm32, tb.qs, tb.ratio_words)  # shape
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32[:2], tb.qs, tb.ratio_words)          # G mismatch
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32[:, :32].contiguous(), tb.qs, tb.ratio_words)
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32, tb.qs[:2], tb.ratio_words)          # prime table
    with pytest.raises(RuntimeError):
        f(dig.cpu(), keys, perm32, tb.qs, tb.ratio_words)        # device
    with pytest.raises(RuntimeError):
        f(_strided(dig), keys, perm32, tb.qs, tb.ratio_words)    # strides


# ----- galois_perm_add_many ----------------------------------------------------

def _perm_add_inputs(ctx, R, n, l, G, seed):
    ct = _planted((R, 2), ctx.primes[:l], n, seed=seed)
    ks0 = torch.roll(_planted((G, R), ctx.primes[:l], n, seed=seed + 1),
                     n // 8, -1)        # (q-1) + (q-1), 0 + 0, mixed pairs
    ks1 = _planted((G, R), ctx.primes[:l], n, seed=seed + 2)
    return ct, ks0, ks1


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_galois_perm_add_many_bit_exact(R, n, l, chain, G):
    ctx = _ctx(n, CHAINS[chain], "cuda")
    be = ctx.backend
    ct, ks0, ks1 = _perm_add_inputs(ctx, R, n, l, G, seed=R + n + l + G)
    perm32, perm = _perms(ctx, _elements(n, G))
    out = be.galois_perm_add_many(ct.cuda(), ks0.cuda(), ks1.cuda(), perm32)
    assert out.shape == (G, R, 2, l, n) and out.dtype == torch.int64
    want = _ref_perm_add_many(ct, ks0, ks1, perm, ctx.primes)
    assert np.array_equal(out.cpu().numpy(), want)
    # one element: the single-rotation kernel's result
    one = be.galois_perm_add(ct.cuda(), ks0[0].cuda(), ks1[0].cuda(),
                             perm32[0].contiguous())
    assert torch.equal(out[0], one)


def test_galois_perm_add_many_scalar_path():
    n, l, R, G = 64, 3, 3, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    ct, ks0, ks1 = _perm_add_inputs(ctx, R, n, l, G, seed=4)
    perm32, perm = _perms(ctx, _elements(n, G))
    out = be._C.galois_perm_add_many(_unaligned(ct), _unaligned(ks0),
                                     ks1.cuda(), perm32, be.qs)
    want = _ref_perm_add_many(ct, ks0, ks1, perm, ctx.primes)
    assert np.array_equal(out.cpu().numpy(), want)


def test_galois_perm_add_many_rejects_bad_arguments():
    n, l, R, G = 64, 2, 2, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    ct, ks0, ks1 = (t.cuda() for t in _perm_add_inputs(ctx, R, n, l, G, 1))
    perm32, _ = _perms(ctx, _elements(n, G))
    f = be._C.galois_perm_add_many
    f(ct, ks0, ks1, perm32, be.qs)                               # accepted
    with pytest.raises(RuntimeError):
        f(ct, ks0[:2].contiguous(), ks1, perm32, be.qs)          # shape
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, perm32.long(), be.qs)                    # dtype
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, perm32[:, :32].contiguous(), be.qs)      # short perm
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1.cpu(), perm32, be.qs)                     # device
    with pytest.raises(RuntimeError):
        f(ct, _strided(ks0), ks1, perm32, be.qs)                 # strides
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, perm32, be.qs[:1])                       # prime table


# ----- lt_inner ----------------------------------------------------------------

@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_lt_inner_bit_exact(R, n, l, chain, G):
    ctx = _ctx(n, CHAINS[chain], "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    targets, dig, keys, pt = _inner_inputs(ctx, R, n, l, G,
                                           seed=2 * R * n + l + G)
    perm32, perm = _perms(ctx, _elements(n, G))
    acc0, acc1 = be.lt_inner(dig.cuda(), keys.cuda(), perm32, pt.cuda(), tb)
    assert acc0.shape == acc1.shape == (R, l + 1, n)
    want = _ref_lt_inner(dig, keys, perm, pt, targets).astype(np.int64)
    assert np.array_equal(acc0.cpu().numpy(), want[0])
    assert np.array_equal(acc1.cpu().numpy(), want[1])


def test_lt_inner_scalar_path():
    n, l, R, G = 64, 2, 3, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    targets, dig, keys, pt = _inner_inputs(ctx, R, n, l, G, seed=19)
    perm32, perm = _perms(ctx, _elements(n, G))
    want = _ref_lt_inner(dig, keys, perm, pt, targets).astype(np.int64)
    acc0, acc1 = be.lt_inner(dig.cuda(), keys.cuda(), perm32, _unaligned(pt), tb)
    assert np.array_equal(acc0.cpu().numpy(), want[0])
    assert np.array_equal(acc1.cpu().numpy(), want[1])


def test_lt_inner_rejects_bad_arguments():
    n, l, R, G = 64, 2, 2, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    _, dig, keys, pt = (t if isinstance(t, list) else t.cuda()
                        for t in _inner_inputs(ctx, R, n, l, G, seed=1))
    perm32, _ = _perms(ctx, _elements(n, G))
    f = be._C.lt_inner
    f(dig, keys, perm32, pt, tb.qs, tb.ratio_words)              # accepted
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32, pt[:2].contiguous(), tb.qs, tb.ratio_words)
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32, pt[:, :l].contiguous(), tb.qs, tb.ratio_words)
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32, pt.to(torch.int32), tb.qs, tb.ratio_words)
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32, pt.cpu(), tb.qs, tb.ratio_words)    # device
    with pytest.raises(RuntimeError):
        f(dig, keys, perm32, _strided(pt), tb.qs, tb.ratio_words)
    with pytest.raises(RuntimeError):
        f(dig, keys[:2].contiguous(), perm32, pt, tb.qs, tb.ratio_words)


# ----- lt_finish ---------------------------------------------------------------

def _finish_inputs(ctx, R, n, l, G, seed):
    ct = _planted((R, 2), ctx.primes[:l], n, seed=seed)
    ks0 = torch.roll(_planted((R,), ctx.primes[:l], n, seed=seed + 1),
                     n // 8, -1)
    ks1 = torch.roll(_planted((R,), ctx.primes[:l], n, seed=seed + 2),
                     n // 3, -1)
    pt = torch.roll(_planted((G,), ctx.primes[:l], n, seed=seed + 3),
                    n // 5, -1)
    return ct, ks0, ks1, pt


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_lt_finish_bit_exact(R, n, l, chain, G):
    ctx = _ctx(n, CHAINS[chain], "cuda")
    be = ctx.backend
    ct, ks0, ks1, pt = _finish_inputs(ctx, R, n, l, G, seed=3 * R * n + l + G)
    # with and without a step-0 diagonal (element 1, at the last index)
    for z0 in (-1, G - 1):
        elements = _elements(n, G)
        if z0 >= 0:
            elements[z0] = 1
        perm32, perm = _perms(ctx, elements)
        out = be.lt_finish(ct.cuda(), ks0.cuda(), ks1.cuda(), pt.cuda(),
                           perm32, z0)
        assert out.shape == ct.shape and out.dtype == torch.int64
        want = _ref_lt_finish(ct, ks0, ks1, pt, perm, z0, ctx.primes)
        assert np.array_equal(out.cpu().numpy(), want), z0


def test_lt_finish_scalar_path():
    n, l, R, G = 64, 3, 3, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    ct, ks0, ks1, pt = _finish_inputs(ctx, R, n, l, G, seed=6)
    perm32, perm = _perms(ctx, [5, 1, 2 * n - 1])
    out = be._C.lt_finish(_unaligned(ct), _unaligned(ks0), ks1.cuda(),
                          pt.cuda(), perm32, 1, be.qs, be.ratio_words)
    want = _ref_lt_finish(ct, ks0, ks1, pt, perm, 1, ctx.primes)
    assert np.array_equal(out.cpu().numpy(), want)


def test_lt_finish_rejects_bad_arguments():
    n, l, R, G = 64, 2, 2, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    ct, ks0, ks1, pt = (t.cuda() for t in _finish_inputs(ctx, R, n, l, G, 1))
    perm32, _ = _perms(ctx, _elements(n, G))
    qs, rw = be.qs, be.ratio_words
    f = be._C.lt_finish
    f(ct, ks0, ks1, pt, perm32, -1, qs, rw)                      # accepted
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, pt, perm32, G, qs, rw)                   # z0 range
    with pytest.raises(RuntimeError):
        f(ct, ks0[:1].contiguous(), ks1, pt, perm32, -1, qs, rw)  # shape
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, pt[:2].contiguous(), perm32, -1, qs, rw)  # G mismatch
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, pt, perm32.long(), -1, qs, rw)           # dtype
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, pt.cpu(), perm32, -1, qs, rw)            # device
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, _strided(pt), perm32, -1, qs, rw)        # strides
    with pytest.raises(RuntimeError):
        f(ct, ks0, ks1, pt, perm32, -1, qs[:1], rw)              # prime table


# ----- whole operations, device == CPU oracle ------------------------------------

OP_RINGS = {64: (50, 30, 30), 1024: (60, 40)}
MAT = (3, 5)        # diagonals -2 .. 4: six keyed ones and step 0


@functools.lru_cache(maxsize=None)
def _op_ring(n):
    """Contexts, keys and the matrix of one ring, made on the CPU context."""
    chain = OP_RINGS[n]
    cpu = _ctx(n, chain, "cpu", seed=31)
    gpu = _ctx(n, chain, "cuda", seed=31)
    assert cpu.primes == gpu.primes
    kp = cpu.keygen()
    M = np.random.default_rng(n).uniform(-1, 1, MAT)
    diag_steps = [k % cpu.slots for k in range(-(MAT[0] - 1), MAT[1]) if k]
    gk = cpu.galois_keygen(
        kp.sk, steps=[1, -1, cpu.slots // 2] + diag_steps, conjugate=True)
    gk_dev = {g: t.cuda() for g, t in gk.items()}
    return cpu, gpu, kp, gk, gk_dev, M


@functools.lru_cache(maxsize=None)
def _op_case(B, n, below_top):
    from hefl.he import CtxtTensor
    cpu, gpu, kp, gk, gk_dev, M = _op_ring(n)
    vec = torch.from_numpy(np.random.default_rng(B * n).uniform(
        -1, 1, B * cpu.slots)).float()
    ct = cpu.encrypt_tensor(vec, kp.pk)
    if below_top:
        ct = cpu.rescale_tensor(cpu.mul_scalar_tensor(ct, 1.0))
    level = cpu.L - 1 if below_top else cpu.L
    assert ct.data.shape == (B, 2, level, n)
    return ct, CtxtTensor(ct.data.cuda(), ct.scale, ct.count)


@pytest.mark.parametrize("below_top", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", sorted(OP_RINGS))
def test_rotate_many_gpu_matches_cpu_oracle(n, B, below_top):
    cpu, gpu, kp, gk, gk_dev, _ = _op_ring(n)
    ct, ct_dev = _op_case(B, n, below_top)
    steps = [1, 0, cpu.slots // 2, -1, 1]
    want = cpu.rotate_many_tensor(ct, steps, gk, conjugate=True)
    got = gpu.rotate_many_tensor(ct_dev, steps, gk_dev, conjugate=True)
    assert len(got) == len(want) == len(steps) + 1
    for g, w in zip(got, want):
        assert g.data.shape == ct.data.shape
        assert g.scale == ct.scale and g.count == ct.count
        assert torch.equal(g.data.cpu(), w.data)


@pytest.mark.parametrize("below_top", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", sorted(OP_RINGS))
def test_linear_transform_gpu_matches_cpu_oracle(n, B, below_top):
    from hefl.he import LinearTransform
    cpu, gpu, kp, gk, gk_dev, M = _op_ring(n)
    ct, ct_dev = _op_case(B, n, below_top)
    lt_c = LinearTransform(cpu, M, level=ct.level)
    lt_g = LinearTransform(gpu, M, level=ct.level)
    assert lt_g.steps == lt_c.steps and 0 in lt_g.diag_steps
    assert torch.equal(lt_g.pt.cpu(), lt_c.pt)
    assert torch.equal(lt_g.pt_keyed.cpu(), lt_c.pt_keyed)
    want = lt_c.apply_tensor(ct, gk)
    got = lt_g.apply_tensor(ct_dev, gk_dev)
    assert got.data.shape == ct.data.shape
    assert got.scale == want.scale and got.count == want.count
    assert torch.equal(got.data.cpu(), want.data)


# ----- n = 2^13, the config #2 chain: decoded accuracy on the device -------------

def test_linear_transform_n8192_accuracy():
    from hefl.he import CtxtTensor, LinearTransform
    from hefl.he.ckks import Ciphertext, Plaintext
    n, chain, B = 1 << 13, (60, 40), 2
    ctx = _ctx(n, chain, "cuda", seed=5)
    host = _ctx(n, chain, "cpu", seed=5)       # exact f64 decode
    kp = ctx.keygen()
    rng = np.random.default_rng(13)
    M = rng.uniform(-1, 1, (2, 3))             # G = 4 diagonals: -1, 0, 1, 2
    lt = LinearTransform(ctx, M)
    assert len(lt.diag_steps) == 4 and len(lt.steps) == 3
    gk = ctx.galois_keygen(kp.sk, steps=lt.steps)
    v = rng.uniform(-1, 1, (B, 3))
    buf = torch.zeros(B, ctx.slots, dtype=torch.float64)
    buf[:, :3] = torch.from_numpy(v)
    pt = ctx.encode(buf)
    ct = CtxtTensor(ctx._encrypt_data(pt.data, kp.pk), pt.scale, B * ctx.slots)
    want = np.zeros((B, ctx.slots))
    want[:, :2] = v @ M.T
    peak = np.abs(want).max()

    def decoded(data, scale):
        p = ctx._decrypt_data(data, kp.sk).cpu()
        return host.decode(Plaintext(p, scale), host.slots)

    new = ctx.rescale_tensor(lt.apply_tensor(ct, gk))
    full = np.zeros((ctx.slots, ctx.slots))
    full[:2, :3] = M
    j = np.arange(ctx.slots)
    acc = None
    for k in lt.diag_steps:                    # rotate, mul_plain, add
        d = ctx.encode(torch.from_numpy(full[j, (j + k) % ctx.slots]),
                       scale=lt.scale)
        term = ctx.mul_plain(Ciphertext(ctx.rotate_data(ct.data, k, gk),
                                        ct.scale), d)
        acc = term if acc is None else ctx.add(acc, term)
    ref = ctx.rescale(acc)
    assert new.level == ref.level == 1
    err_new = np.abs(decoded(new.data, new.scale) - want).max()
    err_ref = np.abs(decoded(ref.data, ref.scale) - want).max()
    print(f"n=2^13: err_new {err_new:.3e}, err_ref {err_ref:.3e}, "
          f"max|Mv| {peak:.3f}")
    assert err_ref < 1e-4 * peak and err_new < 1e-4 * peak
    assert err_new <= 4 * err_ref
