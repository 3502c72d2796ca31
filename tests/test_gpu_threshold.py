"""Threshold decryption on the MI355X: the uniform_center_rns and pdec_share
HIP kernels bit-exact against big-int / CPU-oracle references, the combine
boundary, and the whole n-of-n protocol end to end on the device.

End-to-end bound (see test_threshold_cpu.py): 1e-3 for the CKKS pipeline
itself plus the worst case k * n * 2^smudge_bits / scale the smudging noise
of k parties can add to one slot.
"""
import functools

import numpy as np
import pytest
import torch

from hefl.config import HEConfig

pytestmark = pytest.mark.gpu

CHAINS = {"60-40-40": (60, 40, 40), "50-30-20": (50, 30, 20)}
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
# (R, n, nlimbs)
SHAPES = [(3, 64, 1), (3, 64, 3), (5, 1024, 2)]


@functools.lru_cache(maxsize=None)
def _ctx(n, q_bits, device, seed=21):
    from hefl.he import CKKSContext
    return CKKSContext(HEConfig(m=n, scale_bits=min(q_bits[1:] or (30,)),
                                q_bits=q_bits, seed=seed), device=device)


def _bits(R, n, seed):
    """Random 64-bit draws with the extreme values planted: whole rows when
    there are enough rows, else quarter-rows of row 0."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(INT64_MIN, INT64_MAX, (R, n), generator=g,
                         dtype=torch.int64)
    special = [0, -1, INT64_MIN, INT64_MAX]
    if R > len(special):
        for r, v in enumerate(special):
            bits[r] = v
    else:
        for i, v in enumerate(special):
            bits[0, i * (n // 4):(i + 1) * (n // 4)] = v
    return bits


def _ref_uniform_center_rns(bits, sb, primes):
    v = (bits.numpy().astype(object) & ((1 << (sb + 1)) - 1)) - (1 << sb)
    assert (v >= -(1 << sb)).all() and (v < (1 << sb)).all()
    return np.stack([(v % q) for q in primes], axis=-2).astype(np.int64)


def _residues(shape_lead, primes, n, seed):
    """Uniform residues [*lead, len(primes), n], limb l in [0, q_l)."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack(
        [rng.integers(0, q, size=tuple(shape_lead) + (n,), dtype=np.int64)
         for q in primes], axis=-2))


# ----- uniform_center_rns --------------------------------------------------

@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("sb", [0, 20, 48])
@pytest.mark.parametrize("R,n,nlimbs", SHAPES)
def test_uniform_center_rns_bit_exact(R, n, nlimbs, sb, chain):
    ctx = _ctx(n, CHAINS[chain], "cuda")
    bits = _bits(R, n, seed=R * n + sb)
    out = ctx.backend.uniform_center_rns(bits.cuda(), sb, nlimbs)
    assert out.shape == (R, nlimbs, n) and out.dtype == torch.int64
    want = _ref_uniform_center_rns(bits, sb, ctx.primes[:nlimbs])
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("case", ["odd_n", "unaligned"])
def test_uniform_center_rns_scalar_path(case):
    """Odd n, or storage off a 16-byte boundary, takes the non-vector kernel."""
    ctx = _ctx(64, CHAINS["50-30-20"], "cuda")
    be = ctx.backend
    if case == "odd_n":
        bits = _bits(5, 63, seed=1)
        dev = bits.cuda()
    else:
        bits = _bits(5, 64, seed=2)
        dev = torch.empty(5 * 64 + 1, dtype=torch.int64, device="cuda")[1:]
        dev = dev.view(5, 64).copy_(bits.cuda())
        assert dev.data_ptr() % 16 == 8
    out = be._C.uniform_center_rns(dev, 48, be.qs, be.ratio_words, 3)
    want = _ref_uniform_center_rns(bits, 48, ctx.primes[:3])
    assert np.array_equal(out.cpu().numpy(), want)


# ----- pdec_share ----------------------------------------------------------

@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("lead", [False, True])
@pytest.mark.parametrize("B,n,Lc", SHAPES)
def test_partial_decrypt_gpu_matches_cpu_oracle(B, n, Lc, lead, chain):
    """Same ct, same s_hat, same injected bits: the device path (noise
    kernel + NTT + pdec_share) equals the CPU path bit for bit."""
    cpu = _ctx(n, CHAINS[chain], "cpu")
    gpu = _ctx(n, CHAINS[chain], "cuda")
    assert cpu.primes == gpu.primes
    ct = _residues((B, 2), cpu.primes[:Lc], n, seed=B + n)
    s_hat = _residues((), cpu.primes, n, seed=99)        # [L >= Lc, n]
    bits = _bits(B, n, seed=7 * B + Lc)
    for sb in (0, 20, 48):
        want = cpu.partial_decrypt_data(ct, s_hat, sb, lead, bits=bits)
        got = gpu.partial_decrypt_data(ct.cuda(), s_hat.cuda(), sb, lead,
                                       bits=bits.cuda())
        assert got.shape == (B, Lc, n)
        assert torch.equal(got.cpu(), want), (sb,)


def _ref_pdec(ct, s_hat, e_hat, lead, primes):
    c0 = ct[..., 0, :, :].numpy().astype(object)
    c1 = ct[..., 1, :, :].numpy().astype(object)
    L = c1.shape[-2]
    qs = np.array(primes[:L], dtype=object).reshape(L, 1)
    h = c1 * s_hat[:L].numpy().astype(object) + e_hat.numpy().astype(object)
    if lead:
        h = h + c0
    return (h % qs).astype(np.int64)


@pytest.mark.parametrize("lead", [False, True])
@pytest.mark.parametrize("s_val", ["q-1", "1"])
def test_pdec_share_maximal_residues(lead, s_val):
    """Every input q_l - 1. With s = q-1 the product is 1; with s = 1 it is
    q-1 and the three-term sum 3q-3 needs both conditional subtracts."""
    for chain in CHAINS.values():
        ctx = _ctx(64, chain, "cuda")
        L = ctx.L
        qs = torch.tensor(ctx.primes, dtype=torch.int64).view(L, 1)
        top = (qs - 1).expand(L, 64)
        ct = top.expand(3, 2, L, 64).contiguous()
        s_hat = top.contiguous() if s_val == "q-1" else torch.ones(
            L, 64, dtype=torch.int64)
        e_hat = top.expand(3, L, 64).contiguous()
        got = ctx.backend.pdec_share(ct.cuda(), s_hat.cuda(), e_hat.cuda(),
                                     lead).cpu()
        want = _ref_pdec(ct, s_hat, e_hat, lead, ctx.primes)
        assert np.array_equal(got.numpy(), want)
        if lead and s_val == "1":
            assert torch.equal(got, (qs - 3).expand(3, L, 64))


@pytest.mark.parametrize("n", [64, 63])
@pytest.mark.parametrize("lead", [False, True])
def test_pdec_share_distinct_planes(lead, n):
    """c0 and c1 planes hold unrelated random data, s_hat carries more limbs
    than the ciphertext: a swapped or mis-strided plane cannot pass. n = 63
    takes the non-vector kernel."""
    ctx = _ctx(64, CHAINS["60-40-40"], "cuda")
    be = ctx.backend
    Lc = 2
    ct = _residues((4, 2), ctx.primes[:Lc], n, seed=5)
    assert not torch.equal(ct[:, 0], ct[:, 1])
    s_hat = _residues((), ctx.primes, n, seed=6)
    e_hat = _residues((4,), ctx.primes[:Lc], n, seed=8)
    got = be._C.pdec_share(ct.cuda(), s_hat.cuda(), e_hat.cuda(), lead,
                           be.qs, be.ratio_words).cpu()
    assert np.array_equal(got.numpy(),
                          _ref_pdec(ct, s_hat, e_hat, lead, ctx.primes))


def test_pdec_share_rejects_bad_shapes():
    ctx = _ctx(64, CHAINS["60-40-40"], "cuda")
    be = ctx.backend
    ct = _residues((2, 2), ctx.primes[:2], 64, seed=1).cuda()
    s_hat = _residues((), ctx.primes, 64, seed=2).cuda()
    e_hat = _residues((2,), ctx.primes[:2], 64, seed=3).cuda()
    with pytest.raises(RuntimeError):      # s_hat with fewer limbs than ct
        be.pdec_share(ct, s_hat[:1], e_hat, True)
    with pytest.raises(RuntimeError):      # e_hat batch mismatch
        be.pdec_share(ct, s_hat, e_hat[:1], True)
    with pytest.raises(RuntimeError):      # not a (c0, c1) pair
        be.pdec_share(ct[:, :1], s_hat, e_hat, True)
    with pytest.raises(RuntimeError):      # more limbs than the prime table
        be._C.uniform_center_rns(ct[:, 0, 0].contiguous(), 4, be.qs,
                                 be.ratio_words, 9)
    with pytest.raises(RuntimeError):      # smudge_bits past the int64 budget
        be._C.uniform_center_rns(ct[:, 0, 0].contiguous(), 49, be.qs,
                                 be.ratio_words, 2)


# ----- combine boundary ----------------------------------------------------

def test_combine_eight_maximal_shares():
    ctx = _ctx(64, (60, 40, 20), "cuda")
    L, n = ctx.L, ctx.n
    qs = torch.tensor(ctx.primes, dtype=torch.int64, device="cuda").view(L, 1)
    assert [q.bit_length() for q in ctx.primes] == [60, 40, 20]
    share = (qs - 1).expand(L, n).contiguous()
    lazy = torch.stack([share] * 8).sum(0)
    want = (qs - 8).expand(L, n)
    pk = ctx.combine_pk(lazy, share)
    assert torch.equal(pk[0], want) and torch.equal(pk[1], share)
    batch = lazy.expand(3, L, n).contiguous()
    ctx.backend._C.modreduce_(batch, ctx.backend.qs[:L].contiguous())
    assert torch.equal(batch, want.expand(3, L, n))


# ----- end to end on the device --------------------------------------------

def _bound(k, n, sb, scale):
    return 1e-3 + k * n * (2.0 ** sb) / scale


@pytest.mark.parametrize("k,m,q_bits,sb,count", [
    (3, 256, (60, 40), 16, 300),
    (8, 8192, (60, 40), 16, 9000),             # config2's ring, 3 cts, Lc=1
    (2, 32768, (60, 40, 40, 40), 16, 20000),   # Lc=3, global-stage NTT
])
def test_threshold_fedavg_on_device(k, m, q_bits, sb, count):
    from hefl.he.ckks import CtxtTensor
    ctx = _ctx(m, q_bits, "cuda")
    g = torch.Generator().manual_seed(k)
    vecs = [torch.randn(count, generator=g).cuda() for _ in range(k)]
    a = ctx.sample_crp()
    shares = [ctx.keygen_share(a, i) for i in range(k)]
    pk = ctx.combine_pk(torch.stack([s.b_share for s in shares]).sum(0), a)
    agg = None
    for i, v in enumerate(vecs):
        ctx.reseed(i)
        ct = ctx.encrypt_tensor(v, pk)
        agg = ct if agg is None else CtxtTensor(agg.data + ct.data, agg.scale,
                                                agg.count)
    ctx.modreduce_tensor_(agg)
    avg = ctx.rescale_tensor(ctx.mul_scalar_tensor(agg, 1.0 / k))
    assert avg.level == len(q_bits) - 1
    acc = None
    for i, s in enumerate(shares):
        h = ctx.partial_decrypt_tensor(avg, s.sk_share, sb, lead=(i == 0))
        assert h.is_cuda and h.shape == (avg.data.shape[0], avg.level, m)
        acc = h if acc is None else acc + h
    out = ctx.combine_shares_tensor(acc, avg.scale, avg.count)
    mean = torch.stack(vecs).mean(0)
    err = (out - mean).abs().max().item()
    print(f"k={k} m={m} Lc={avg.level} sb={sb}: max err {err:.3e}")
    assert err < _bound(k, m, sb, avg.scale)
    if avg.level == 1:
        # one share alone decodes to noise
        alone = ctx.decrypt_tensor(avg, shares[0].sk_share)
        assert (alone - mean).abs().max().item() > 1.0


def test_threshold_aggregator_single_rank_on_device():
    from hefl.fl.secure import SecureAggregator
    from hefl.he import CKKSContext
    ctx = CKKSContext(HEConfig(m=1024, scale_bits=40, q_bits=(60, 40), seed=4),
                      device="cuda")
    agg = SecureAggregator(ctx, 0, key_mode="threshold", smudge_bits=16)
    vec = torch.randn(1500, generator=torch.Generator().manual_seed(1)).cuda()
    out = agg.fedavg(vec)
    assert out.is_cuda
    assert (out - vec).abs().max().item() < _bound(1, 1024, 16, 2.0 ** 40)


def test_sequential_fl_threshold_on_device():
    from hefl.config import preset
    from hefl.fl.sequential import SequentialFL
    from hefl.fl.weights import flat_params
    cfg = preset("config2")
    cfg.fl.n_clients = 2
    cfg.fl.samples_per_client = 64
    cfg.he.m = 256
    cfg.fl.key_mode = "threshold"
    fl = SequentialFL(cfg, device="cuda")
    assert fl.keys.sk is None and len(fl.key_shares) == 2
    fl.run_round(epochs=1)
    mean = torch.stack([c.get_weights() for c in fl.clients]).mean(0)
    err = (flat_params(fl.global_model) - mean).abs().max().item()
    print(f"SequentialFL threshold: max err {err:.3e}")
    assert err < _bound(2, 256, cfg.fl.smudge_bits, 2.0 ** 40)
