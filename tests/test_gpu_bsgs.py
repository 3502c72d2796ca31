"""Baby-step/giant-step linear transform on the MI355X: the bsgs_mac,
bsgs_giant_inner and bsgs_finish HIP kernels bit-exact against numpy big-int
references on planted residues (0, q - 1 and uniform ones in every row), and
LinearTransform(..., bsgs=...).apply_tensor bit-exact against the CPU oracle
(same seeded context, keys and ciphertext).

Everything is exact modular arithmetic on canonical residues, so comparisons
are array_equal / torch.equal. The n = 1024 case also decodes, under the rule
of test_bsgs_cpu.py: slot error below 1e-4 max|Mv| and at most 4x that of the
path composed of rotate, mul_plain and add.
"""
import functools

import numpy as np
import pytest
import torch

from hefl.config import HEConfig

pytestmark = pytest.mark.gpu

CHAIN = (50, 30, 20)
KERNEL_SHAPES = [(1, 16, 1), (3, 64, 3), (2, 1024, 2)]      # (R, n, l)


@functools.lru_cache(maxsize=None)
def _ctx(n, q_bits, device, seed=21):
    from hefl.he import CKKSContext
    return CKKSContext(HEConfig(m=n, scale_bits=min(q_bits[1:]),
                                q_bits=q_bits, seed=seed), device=device)


def _planted(lead, primes, n, seed):
    """Residues [*lead, len(primes), n]: first quarter of each row 0, second
    quarter q - 1, the rest uniform in [0, q)."""
    rng = np.random.default_rng(seed)
    rows = []
    for q in primes:
        r = rng.integers(0, q, size=tuple(lead) + (n,), dtype=np.int64)
        r[..., :n // 4] = 0
        r[..., n // 4:n // 2] = q - 1
        rows.append(r)
    return torch.from_numpy(np.stack(rows, axis=-2))


def _unaligned(t):
    """A device copy of t whose storage starts 8 bytes off a 16-byte line."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:]
    v = buf.view(t.shape).copy_(t.cuda())
    assert v.data_ptr() % 16 == 8
    return v


def _col(primes):
    return np.array(list(primes), dtype=object).reshape(-1, 1)


def _obj(t):
    return t.numpy().astype(object)


def _perms(ctx, elements):
    """(int32 device [G, n], numpy [G, n]); element 1 is the identity."""
    p = np.stack([np.arange(ctx.n) if g == 1 else
                  ctx._galois_tables(g).perm.cpu().numpy() for g in elements])
    return torch.from_numpy(p.astype(np.int32)).cuda(), p


# ----- bsgs_mac ------------------------------------------------------------------

def _mac_layouts(C):
    """name: (Nb, has0, baby indices per giant, operand stored unaligned)."""
    F, tile = C.BSGS_FLUSH_TERMS, C.BSGS_BABY_TILE
    return {
        # (q-1)*(q-1) F + 2 times in one sum; an empty giant
        "flush": (3, True, [[t % 3 for t in range(F + 2)], [1], []], None),
        # one baby past the LDS tile; giants with terms in the 2nd tile only
        "tile+1": (tile + 1, True, [list(range(tile + 1)), [tile], [0, tile],
                                    [5], [tile - 1, tile]], None),
        "no-baby-0": (2, False, [[0, 1], [1]], None),
        "baby-0-only": (1, True, [[0], [0], [0]], None),
        # more giants than one pass of the waves
        "many-giants": (2, True, [[g % 2] for g in range(133)], None),
        "unaligned-pt": (2, False, [[0, 1], [1]], "pt"),
        "unaligned-ct": (3, True, [[0, 2], [1]], "ct"),
    }


@pytest.mark.parametrize("layout", ["flush", "tile+1", "no-baby-0",
                                    "baby-0-only", "many-giants",
                                    "unaligned-pt", "unaligned-ct"])
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_bsgs_mac_bit_exact(R, n, l, layout):
    ctx = _ctx(n, CHAIN, "cuda")
    be = ctx.backend
    Nb, has0, groups, off = _mac_layouts(be._C)[layout]
    primes = ctx.primes[:l]
    seed = R * n + l + Nb
    babies = _planted((Nb, R, 2), primes, n, seed=seed)
    bidx = [b for g in groups for b in g]
    goff = np.cumsum([0] + [len(g) for g in groups])
    # unrolled pt keeps 0 and q - 1 facing 0 and q - 1: (q-1)^2 in every term
    pt = _planted((len(bidx),), primes, n, seed=seed + 1)
    ct = babies[0] if has0 else _planted((R, 2), primes, n, seed=seed + 2)
    rot = babies[1:] if has0 else babies
    place = {name: (_unaligned if off == name else torch.Tensor.cuda)
             for name in ("ct", "pt")}
    u = be.bsgs_mac(place["ct"](ct), rot.cuda(), place["pt"](pt),
                    torch.tensor(goff, dtype=torch.int32).cuda(),
                    torch.tensor(bidx, dtype=torch.int32).cuda(), has0)
    assert u.shape == (len(groups), R, 2, l, n) and u.dtype == torch.int64
    b_o, p_o, qs = _obj(babies), _obj(pt), _col(primes)
    want = np.zeros(u.shape, dtype=object)
    for g in range(len(groups)):
        for t in range(goff[g], goff[g + 1]):
            want[g] += b_o[bidx[t]] * p_o[t][None, None]
    assert np.array_equal(u.cpu().numpy(), (want % qs).astype(np.int64))


# ----- bsgs_giant_inner / bsgs_finish --------------------------------------------

def _ref_giant_inner(dig, keys, perm, targets):
    """[2, R, Lp, n]: sum_g sum_d dig[g, r, d, i, perm[g, k]] * keys[g, d, c, i, k]."""
    d, k, qs = _obj(dig), _obj(keys), _col(targets)
    return np.stack([sum((d[g][..., perm[g]] * k[g][:, c][None]).sum(axis=1)
                         for g in range(len(perm))) % qs for c in range(2)])


# G = 44 with l = 3 digits is 132 > BSGS_FLUSH_TERMS products in one sum
@pytest.mark.parametrize("G", [1, 3, 44])
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_bsgs_giant_inner_bit_exact(R, n, l, G):
    ctx = _ctx(n, CHAIN, "cuda")
    be = ctx.backend
    tb = be.level_tables(l)
    targets = ctx.primes[:l] + [ctx.special]
    assert tb.qs.cpu().tolist() == targets
    dig = _planted((G, R, l), targets, n, seed=R * n + l + G)
    keys = torch.roll(_planted((G, l, 2), targets, n, seed=R * n + l + G + 1),
                      n // 8, -1)
    if G == 44:                      # the largest sum there is: all (q-1)^2
        dig[:] = torch.tensor(targets).view(-1, 1) - 1
        keys[:] = torch.tensor(targets).view(-1, 1) - 1
    perm32, perm = _perms(ctx, [pow(5, j + 1, 2 * n) for j in range(G)])
    want = _ref_giant_inner(dig, keys, perm, targets).astype(np.int64)
    for d in (dig.cuda(), _unaligned(dig)):          # dig is only gathered
        acc0, acc1 = be.bsgs_giant_inner(d, keys.cuda(), perm32, tb)
        assert acc0.shape == acc1.shape == (R, l + 1, n)
        assert np.array_equal(acc0.cpu().numpy(), want[0])
        assert np.array_equal(acc1.cpu().numpy(), want[1])
    acc0, acc1 = be.bsgs_giant_inner(dig.cuda(), _unaligned(keys), perm32, tb)
    assert np.array_equal(acc0.cpu().numpy(), want[0])      # V = 1 kernel
    assert np.array_equal(acc1.cpu().numpy(), want[1])


@pytest.mark.parametrize("z0", [-1, 0])
@pytest.mark.parametrize("Ng", [1, 3])
@pytest.mark.parametrize("R,n,l", KERNEL_SHAPES)
def test_bsgs_finish_bit_exact(R, n, l, Ng, z0):
    ctx = _ctx(n, CHAIN, "cuda")
    be = ctx.backend
    primes = ctx.primes[:l]
    seed = 3 * R * n + l + Ng
    u = _planted((Ng, R, 2), primes, n, seed=seed)
    ks0 = torch.roll(_planted((R,), primes, n, seed=seed + 1), n // 8, -1)
    ks1 = torch.roll(_planted((R,), primes, n, seed=seed + 2), n // 8, -1)
    elements = [5, pow(5, -1, 2 * n), 2 * n - 1][:Ng]
    if z0 == 0:
        elements[0] = 1                              # giant 0: the identity
    perm32, perm = _perms(ctx, elements)
    qs = _col(primes)
    out0 = _obj(ks0)
    for g in range(Ng):
        out0 = (out0 + _obj(u[g, :, 0])[..., perm[g]]) % qs
    out1 = (_obj(ks1) + (_obj(u[z0, :, 1]) if z0 >= 0 else 0)) % qs
    want = np.stack([out0, out1], axis=1).astype(np.int64)
    for args in ((u.cuda(), ks0.cuda(), ks1.cuda()),
                 (_unaligned(u), ks0.cuda(), ks1.cuda()),
                 (u.cuda(), ks0.cuda(), _unaligned(ks1))):
        out = be.bsgs_finish(*args, perm32, z0)
        assert out.shape == (R, 2, l, n) and out.dtype == torch.int64
        assert np.array_equal(out.cpu().numpy(), want)


def test_bsgs_kernels_reject_bad_arguments():
    n, l, R = 64, 2, 2
    ctx = _ctx(n, CHAIN, "cuda")
    be = ctx.backend
    C, tb = be._C, be.level_tables(l)
    ct = _planted((R, 2), ctx.primes[:l], n, seed=1).cuda()
    rot = ct[None].clone()
    pt = _planted((2,), ctx.primes[:l], n, seed=2).cuda()
    goff = torch.tensor([0, 2], dtype=torch.int32).cuda()
    bidx = torch.tensor([0, 1], dtype=torch.int32).cuda()
    qs, rw = be.qs, be.ratio_words
    C.bsgs_mac(ct, rot, pt, goff, bidx, True, qs, rw)             # accepted
    for bad in ((ct, rot[:, :1], pt, goff, bidx, True, qs, rw),   # rot shape
                (ct, rot[:0], pt, goff, bidx, False, qs, rw),     # no babies
                (ct, rot, pt[:, :1], goff, bidx, True, qs, rw),   # pt limbs
                (ct, rot, pt, goff.long(), bidx, True, qs, rw),   # dtype
                (ct, rot, pt, goff, bidx[:1], True, qs, rw),      # bidx length
                (ct, rot, pt.cpu(), goff, bidx, True, qs, rw),    # device
                (ct, rot, pt, goff, bidx, True, qs[:1], rw)):     # prime table
        with pytest.raises(RuntimeError):
            C.bsgs_mac(*bad)
    targets = ctx.primes[:l] + [ctx.special]
    dig = _planted((3, R, l), targets, n, seed=3).cuda()
    keys = _planted((3, l, 2), targets, n, seed=4).cuda()
    perm32, _ = _perms(ctx, [5, 25, 125])
    C.bsgs_giant_inner(dig, keys, perm32, tb.qs, tb.ratio_words)  # accepted
    for bad in ((dig[0], keys, perm32), (dig[:2], keys, perm32),
                (dig, keys, perm32[:2]), (dig, keys, perm32.long())):
        with pytest.raises(RuntimeError):
            C.bsgs_giant_inner(*bad, tb.qs, tb.ratio_words)
    u = torch.stack([ct, ct])
    ks = ct[:, 0].contiguous()
    C.bsgs_finish(u, ks, ks, perm32[:2], 1, qs)                   # accepted
    for bad in ((u, ks, ks, perm32[:2], 2, qs), (u, ks[:1], ks, perm32[:2], 0, qs),
                (u, ks, ks, perm32, 0, qs), (u, ks, ks, perm32[:2], 0, qs[:1])):
        with pytest.raises(RuntimeError):
            C.bsgs_finish(*bad)


# ----- the whole transform: device == CPU oracle ---------------------------------

OP_CHAINS = {64: (50, 30, 30), 1024: (60, 40, 40)}
# name: (n, matrix, n1, below_top, R)
OP_CASES = {"n64-dense-n1=4": (64, "dense", 4, False, 3),
            "n64-5x7-n1=3": (64, (5, 7), 3, False, 1),
            "n1024-banded-below-top": (1024, "band", 4, True, 2)}


@pytest.mark.parametrize("case", sorted(OP_CASES))
def test_bsgs_transform_gpu_matches_cpu_oracle(case):
    from hefl.he import CtxtTensor, LinearTransform
    from hefl.he.ckks import Ciphertext, Plaintext
    n, kind, n1, below_top, R = OP_CASES[case]
    cpu = _ctx(n, OP_CHAINS[n], "cpu", seed=31)
    gpu = _ctx(n, OP_CHAINS[n], "cuda", seed=31)
    assert cpu.primes == gpu.primes
    slots = cpu.slots
    rng = np.random.default_rng(n + n1)
    j = np.arange(slots)
    if kind == "band":                               # steps -4 .. 4
        M = np.zeros((slots, slots))
        for k in range(-4, 5):
            M[j, (j + k) % slots] = rng.uniform(-1, 1, slots)
    else:
        M = rng.uniform(-1, 1, (slots, slots) if kind == "dense" else kind)
    kp = cpu.keygen()
    v = np.zeros((R, slots))
    v[:, :M.shape[1]] = rng.uniform(-1, 1, (R, M.shape[1]))
    pt = cpu.encode(v)
    ct = CtxtTensor(cpu._encrypt_data(pt.data, kp.pk), pt.scale, R * slots)
    if below_top:
        ct = cpu.rescale_tensor(cpu.mul_scalar_tensor(ct, 1.0))
    lt_c = LinearTransform(cpu, M, level=ct.level, bsgs=n1)
    lt_g = LinearTransform(gpu, M, level=ct.level, bsgs=n1)
    assert lt_g.steps == lt_c.steps and torch.equal(lt_g.pt.cpu(), lt_c.pt)
    decode = kind == "band"
    gk = cpu.galois_keygen(kp.sk, steps=sorted(
        set(lt_c.steps) | ({k for k in lt_c.diag_steps if k} if decode
                           else set())))
    gk_dev = {g: t.cuda() for g, t in gk.items()}
    ct_dev = CtxtTensor(ct.data.cuda(), ct.scale, ct.count)
    want = lt_c.apply_tensor(ct, gk)
    got = lt_g.apply_tensor(ct_dev, gk_dev)
    assert got.scale == want.scale and got.count == want.count
    assert torch.equal(got.data.cpu(), want.data)
    if not decode:
        return
    acc = None
    for k in lt_g.diag_steps:                        # rotate, mul_plain, add
        d = gpu.encode(torch.from_numpy(M[j, (j + k) % slots]),
                       nlimbs=ct.level, scale=lt_g.scale)
        term = gpu.mul_plain(Ciphertext(gpu.rotate_data(ct_dev.data, k, gk_dev),
                                        ct.scale), d)
        acc = term if acc is None else gpu.add(acc, term)
    truth = v @ M.T
    peak = np.abs(truth).max()
    sk = kp.sk.cuda()
    errs = []
    for res in (gpu.rescale_tensor(got), gpu.rescale(acc)):
        p = Plaintext(gpu._decrypt_data(res.data, sk).cpu(), res.scale)
        errs.append(np.abs(cpu.decode(p, slots) - truth).max())  # exact f64
    print(f"{case}: err_bsgs {errs[0]:.3e}, err_composed {errs[1]:.3e}, "
          f"max|Mv| {peak:.3f}")
    assert errs[1] < 1e-4 * peak and errs[0] < 1e-4 * peak
    assert errs[0] <= 4 * errs[1]
