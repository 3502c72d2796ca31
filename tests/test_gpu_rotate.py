"""Slot rotation on the MI355X: the galois_lift and galois_perm_add HIP
kernels bit-exact against numpy big-int references on planted residues, the
whole rotation bit-exact against the CPU oracle (same key, same ciphertext),
and n = 2^15 end to end on the device.

Every path is exact modular arithmetic on canonical residues, so device and
CPU results are compared with torch.equal. The n = 2^15 case decodes and uses
the derived per-hop bound of test_rotate_cpu.py.
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


def _elements(n):
    return [5, pow(5, -1, 2 * n), 2 * n - 1]


def _ref_lift(c, g, digit_primes, target_primes):
    """sigma_g on each digit's residues in [0, q_d) (negated zero stays 0),
    then reduced into every target prime: [R, l, Lp, n], big-int."""
    R, l, n = c.shape
    a = c.numpy().astype(object)
    out = np.empty((R, l, len(target_primes), n), dtype=object)
    for d, qd in enumerate(digit_primes):
        rot = np.zeros((R, n), dtype=object)
        for j in range(n):
            e = (j * g) % (2 * n)
            if e < n:
                rot[:, e] = a[:, d, j]
            else:
                rot[:, e - n] = (qd - a[:, d, j]) % qd
        for i, q in enumerate(target_primes):
            out[:, d, i, :] = rot % q
    return out.astype(np.int64)


def _unaligned(t):
    """A device copy of t whose storage starts 8 bytes off a 16-byte line."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:]
    v = buf.view(t.shape).copy_(t.cuda())
    assert v.data_ptr() % 16 == 8
    return v


# ----- galois_lift -----------------------------------------------------------

@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_galois_lift_bit_exact(R, n, l, chain):
    ctx = _ctx(n, CHAINS[chain], "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    targets = ctx.primes[:l] + [ctx.special]
    assert tb.qs.cpu().tolist() == targets
    c = _planted((R,), ctx.primes[:l], n, seed=R * n + l)
    for g in _elements(n):
        out = be.galois_lift(c.cuda(), pow(g, -1, 2 * n), tb)
        assert out.shape == (R, l, l + 1, n) and out.dtype == torch.int64
        want = _ref_lift(c, g, ctx.primes[:l], targets)
        assert np.array_equal(out.cpu().numpy(), want), g


def test_galois_lift_unaligned_source():
    """The source is only gathered (8-byte reads), so a view off the 16-byte
    grid takes the same vector-store kernel and must give the same result."""
    n, l = 64, 2
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    c = _planted((3,), ctx.primes[:l], n, seed=9)
    out = be._C.galois_lift(_unaligned(c), pow(5, -1, 2 * n), tb.qs,
                            tb.ratio_words)
    want = _ref_lift(c, 5, ctx.primes[:l], ctx.primes[:l] + [ctx.special])
    assert np.array_equal(out.cpu().numpy(), want)


def test_galois_lift_rejects_bad_arguments():
    ctx = _ctx(64, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    tb = be.level_tables(2)
    c = _planted((1,), ctx.primes[:2], 64, seed=1).cuda()
    with pytest.raises(RuntimeError):
        be._C.galois_lift(c, 4, tb.qs, tb.ratio_words)        # even
    with pytest.raises(RuntimeError):
        be._C.galois_lift(c, 129, tb.qs, tb.ratio_words)      # >= 2n
    with pytest.raises(RuntimeError):
        be._C.galois_lift(c, 5, tb.qs[:1], tb.ratio_words[:1])  # Lp < D


# ----- galois_perm_add -------------------------------------------------------

def _ref_perm_add(ct, ks0, ks1, perm, primes):
    l = ct.shape[-2]
    qs = np.array(primes[:l], dtype=object).reshape(l, 1)
    c0 = ct[:, 0].numpy().astype(object)[..., perm]
    out0 = (c0 + ks0.numpy().astype(object)) % qs
    return np.stack([out0.astype(np.int64), ks1.numpy()], axis=1)


@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_galois_perm_add_bit_exact(R, n, l, chain):
    ctx = _ctx(n, CHAINS[chain], "cuda")
    be = ctx.backend
    ct = _planted((R, 2), ctx.primes[:l], n, seed=R + n + l)
    ks0 = _planted((R,), ctx.primes[:l], n, seed=3 * n)
    ks0 = torch.roll(ks0, n // 8, -1)    # (q-1) + (q-1), 0 + 0, mixed pairs
    ks1 = _planted((R,), ctx.primes[:l], n, seed=5 * n)
    for g in _elements(n):
        gt = ctx._galois_tables(g)
        out = be.galois_perm_add(ct.cuda(), ks0.cuda(), ks1.cuda(), gt.perm32)
        assert out.shape == ct.shape and out.dtype == torch.int64
        want = _ref_perm_add(ct, ks0, ks1, gt.perm.cpu().numpy(), ctx.primes)
        assert np.array_equal(out.cpu().numpy(), want), g


def test_galois_perm_add_scalar_path():
    """ks0 off a 16-byte boundary takes the non-vector kernel."""
    n, l = 64, 3
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    ct = _planted((3, 2), ctx.primes[:l], n, seed=4)
    ks0 = _planted((3,), ctx.primes[:l], n, seed=5)
    ks1 = _planted((3,), ctx.primes[:l], n, seed=6)
    gt = ctx._galois_tables(2 * n - 1)
    out = be._C.galois_perm_add(_unaligned(ct), _unaligned(ks0), ks1.cuda(),
                                gt.perm32, be.qs)
    want = _ref_perm_add(ct, ks0, ks1, gt.perm.cpu().numpy(), ctx.primes)
    assert np.array_equal(out.cpu().numpy(), want)


def test_galois_perm_add_rejects_bad_arguments():
    n = 64
    ctx = _ctx(n, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    ct = _planted((2, 2), ctx.primes[:2], n, seed=1).cuda()
    ks = _planted((2,), ctx.primes[:2], n, seed=2).cuda()
    perm = ctx._galois_tables(5).perm32
    with pytest.raises(RuntimeError):
        be._C.galois_perm_add(ct, ks[:1], ks, perm, be.qs)     # shape
    with pytest.raises(RuntimeError):
        be._C.galois_perm_add(ct, ks, ks, perm[:32], be.qs)    # short perm
    with pytest.raises(RuntimeError):
        be._C.galois_perm_add(ct, ks, ks, perm.long(), be.qs)  # dtype


# ----- whole rotation, device == CPU oracle ------------------------------------

# (B, n, chain, level)
OP_SHAPES = [(1, 64, (50, 30, 30), 3), (3, 64, (50, 30, 30), 2),
             (2, 64, (50, 30, 30), 1), (2, 1024, (60, 40), 2),
             (1, 8192, (60, 40, 40), 2)]


@functools.lru_cache(maxsize=None)
def _op_case(B, n, chain, level):
    """Key and ciphertext made on a CPU context, plus their device copies."""
    cpu = _ctx(n, chain, "cpu", seed=31)
    gpu = _ctx(n, chain, "cuda", seed=31)
    assert cpu.primes == gpu.primes
    kp = cpu.keygen()
    gk = cpu.galois_keygen(kp.sk, steps=[1, -1, cpu.slots // 2],
                           conjugate=True)
    vec = torch.from_numpy(np.random.default_rng(B * n).uniform(
        -1, 1, B * cpu.slots)).float()
    ct = cpu.encrypt_tensor(vec, kp.pk)
    while ct.level > level:
        ct = cpu.rescale_tensor(cpu.mul_scalar_tensor(ct, 1.0))
    assert ct.data.shape == (B, 2, level, n)
    from hefl.he import CtxtTensor
    gk_dev = {g: t.cuda() for g, t in gk.items()}
    ct_dev = CtxtTensor(ct.data.cuda(), ct.scale, ct.count)
    return cpu, gpu, gk, gk_dev, ct, ct_dev, kp


@pytest.mark.parametrize("op", ["1", "-1", "half", "conj"])
@pytest.mark.parametrize("B,n,chain,level", OP_SHAPES)
def test_rotate_gpu_matches_cpu_oracle(B, n, chain, level, op):
    cpu, gpu, gk, gk_dev, ct, ct_dev, _ = _op_case(B, n, chain, level)
    if op == "conj":
        want = cpu.conjugate_tensor(ct, gk)
        got = gpu.conjugate_tensor(ct_dev, gk_dev)
    else:
        r = cpu.slots // 2 if op == "half" else int(op)
        want = cpu.rotate_tensor(ct, r, gk)
        got = gpu.rotate_tensor(ct_dev, r, gk_dev)
    assert got.data.shape == (B, 2, level, n)
    assert got.scale == ct.scale and got.count == ct.count
    assert torch.equal(got.data.cpu(), want.data)


def test_composed_path_matches_fused(monkeypatch):
    """HEFL_GALOIS_FUSED=0 (torch gather / where / stack around the same
    key-switch) computes the same bits as the fused kernels."""
    cpu, gpu, gk, gk_dev, ct, ct_dev, _ = _op_case(3, 64, (50, 30, 30), 2)
    fused = gpu.rotate_tensor(ct_dev, 1, gk_dev)
    monkeypatch.setenv("HEFL_GALOIS_FUSED", "0")
    composed = gpu.rotate_tensor(ct_dev, 1, gk_dev)
    assert torch.equal(fused.data, composed.data)


def test_galois_keygen_same_on_device():
    """Keys are host-sampled: a device context derives the CPU context's."""
    n, chain = 64, (50, 30, 30)
    cpu = _ctx(n, chain, "cpu", seed=77)
    gpu = _ctx(n, chain, "cuda", seed=77)
    gk_c = cpu.galois_keygen(cpu.keygen().sk, steps=[1, -2], conjugate=True)
    gk_g = gpu.galois_keygen(gpu.keygen().sk, steps=[1, -2], conjugate=True)
    assert list(gk_c) == list(gk_g)
    assert all(torch.equal(gk_g[g].cpu(), gk_c[g]) for g in gk_c)


def test_sum_slots_tensor_gpu_matches_cpu():
    cpu, gpu, _, _, ct, ct_dev, kp = _op_case(2, 1024, (60, 40), 2)
    gk = cpu.galois_keygen(kp.sk)        # the +-2^k keys
    gk_dev = {g: t.cuda() for g, t in gk.items()}
    want = cpu.sum_slots_tensor(ct, gk, cpu.slots)
    got = gpu.sum_slots_tensor(ct_dev, gk_dev, gpu.slots)
    assert torch.equal(got.data.cpu(), want.data)


# ----- n = 2^15: global-stage NTT, device only ---------------------------------

def test_rotate_n32768_on_device():
    n, chain = 1 << 15, (60, 40)
    ctx = _ctx(n, chain, "cuda", seed=5)
    kp = ctx.keygen()
    gk = ctx.galois_keygen(kp.sk, steps=[1], conjugate=True)
    v = torch.from_numpy(np.random.default_rng(15).uniform(
        -1, 1, ctx.slots)).float()
    ct = ctx.encrypt_tensor(v, kp.pk)
    l = ct.level
    base = ctx.decrypt_tensor(ct, kp.sk).cpu().numpy().astype(np.float64)
    vv = v.numpy().astype(np.float64)
    enc_err = np.abs(base - vv).max()
    # one hop's worst case (test_rotate_cpu.py) seen through the special FFT,
    # plus the f32 rounding of the decoded output
    q_max = max(ctx.primes[:l])
    hop = l * n * 21 * q_max / ctx.special + (n + 1) / 2 + 1
    tol = hop * n / ct.scale + enc_err + 2.0 ** -23
    rot = ctx.decrypt_tensor(ctx.rotate_tensor(ct, 1, gk), kp.sk).cpu().numpy()
    conj = ctx.decrypt_tensor(ctx.conjugate_tensor(ct, gk), kp.sk).cpu().numpy()
    err_r = np.abs(rot - np.roll(vv, -1)).max()
    err_c = np.abs(conj - vv).max()
    print(f"n=2^15: rotate err {err_r:.3e}, conj err {err_c:.3e}, tol {tol:.3e}")
    assert err_r <= tol and err_c <= tol
