"""Complex packing on the MI355X: the fft_encode_packed / fft_decode_packed
HIP kernels against the CPU oracle (Encoder.encode_complex / decode_complex),
their masking at `count`, argument rejection, and the engine, threshold and
aggregator paths on the device.

Tolerances are those of the real-packing tests of the same operations:
test_gpu_he.py::test_hip_fft_encode_decode_matches_oracle (coefficients within
1, > 99 % exact, decode within 1e-5 of the oracle and 1e-4 of the input),
1e-3 for the lazy-sum mean, test_gpu_threshold.py's smudging bound.
"""
import functools
import math

import numpy as np
import pytest
import torch

from hefl.config import HEConfig

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** 40
RINGS = [256, 16384, 32768]   # one small block, the full LDS block, the split
PAST = 1e30                   # what lies behind the end of the input


def _counts(m):
    s = m // 2
    return {"full": 3 * m, "one_past_row": m + 1, "im_partly": m + s + 3,
            "re_partly": s - 5}


CASES = [(m, name) for m in RINGS for name in _counts(256)]


@functools.lru_cache(maxsize=None)
def _enc(m):
    from hefl.he.encoder import Encoder
    return Encoder(m)


@functools.lru_cache(maxsize=None)
def _case(m, name):
    """Input, oracle coefficients and oracle decode of one (ring, count),
    computed once and shared; nothing here is written to afterwards."""
    enc = _enc(m)
    count = _counts(m)[name]
    rng = np.random.default_rng(m + count)
    vals = rng.standard_normal(count).astype(np.float32)
    ref = np.ascontiguousarray(
        enc.encode_complex(enc.pack_complex(vals), SCALE))
    assert ref.dtype == np.int64 and ref.shape == (math.ceil(count / m), m)
    ref_back = enc.unpack_complex(
        enc.decode_complex(ref, SCALE, enc.slots), count)
    return count, vals, ref, ref_back


def _C():
    import hefl
    return hefl.load_extension()


# ----- 1. encode ---------------------------------------------------------------

@pytest.mark.parametrize("m,name", CASES)
def test_encode_packed_matches_oracle(m, name):
    enc = _enc(m)
    count, vals, ref, _ = _case(m, name)
    tw_enc, _ = enc._hip_tables("cuda")
    big = torch.full((count + 2 * m + 13,), PAST, dtype=torch.float32,
                     device="cuda")
    big[:count] = torch.from_numpy(vals).cuda()
    got = _C().fft_encode_packed(big[:count], count, tw_enc, SCALE, enc.slots)
    assert got.dtype == torch.int64 and tuple(got.shape) == ref.shape
    diff = (got.cpu() - torch.from_numpy(ref)).abs()
    print(f"m={m} count={count}: max coefficient diff {int(diff.max())}, "
          f"exact {(diff == 0).float().mean().item():.5f}")
    # identical butterfly order; FMA contraction may flip an int rounding. A
    # read past `count` would bring 1e30 * 2^40 into every coefficient.
    assert (diff <= 1).all(), diff.max()
    assert (diff == 0).float().mean() > 0.99


# ----- 2. decode ---------------------------------------------------------------

@pytest.mark.parametrize("m,name", CASES)
def test_decode_packed_matches_oracle(m, name):
    enc = _enc(m)
    count, vals, ref, ref_back = _case(m, name)
    _, tw_dec = enc._hip_tables("cuda")
    coeffs = torch.from_numpy(ref).cuda()
    back = _C().fft_decode_packed(coeffs, tw_dec, SCALE, count)
    assert back.dtype == torch.float32 and tuple(back.shape) == (count,)
    got = back.cpu().numpy().astype(np.float64)
    print(f"m={m} count={count}: vs oracle {np.abs(got - ref_back).max():.3e}, "
          f"vs input {np.abs(got - vals).max():.3e}")
    assert np.abs(got - ref_back).max() < 1e-5
    assert np.abs(got - vals).max() < 1e-4


@pytest.mark.parametrize("m,name", CASES)
def test_decode_packed_into_out_writes_nothing_else(m, name):
    enc = _enc(m)
    count, vals, ref, ref_back = _case(m, name)
    _, tw_dec = enc._hip_tables("cuda")
    buf = torch.full((7 + count + 2 * m + 9,), -77.0, dtype=torch.float32,
                     device="cuda")
    out = buf[7:7 + count]
    assert out.data_ptr() % 16 != 0
    ret = _C().fft_decode_packed(torch.from_numpy(ref).cuda(), tw_dec, SCALE,
                                 count, out=out)
    assert ret.data_ptr() == out.data_ptr() and ret.shape == out.shape
    host = buf.cpu()
    assert (host[:7] == -77.0).all() and (host[7 + count:] == -77.0).all()
    got = host[7:7 + count].numpy().astype(np.float64)
    assert np.abs(got - ref_back).max() < 1e-5
    assert np.abs(got - vals).max() < 1e-4


# ----- 3. argument rejection ------------------------------------------------------

def test_packed_kernels_reject_bad_arguments():
    C = _C()
    m = 256
    enc = _enc(m)
    s = enc.slots
    tw_enc, tw_dec = enc._hip_tables("cuda")
    vec = torch.randn(3 * m, device="cuda")
    good = C.fft_encode_packed(vec, vec.numel(), tw_enc, SCALE, s)
    assert good.shape == (3, m)
    bad_encode = [
        (vec.cpu(), vec.numel()),                 # not on the device
        (vec.double(), vec.numel()),              # wrong dtype
        (vec[::2], vec.numel() // 2),             # not contiguous
        (vec, 0),                                 # count < 1
        (vec, vec.numel() + 1),                   # count past the vector
    ]
    for v, count in bad_encode:
        with pytest.raises(RuntimeError):
            C.fft_encode_packed(v, count, tw_enc, SCALE, s)
    with pytest.raises(RuntimeError):
        C.fft_encode_packed(vec, vec.numel(), tw_enc.cpu(), SCALE, s)
    with pytest.raises(RuntimeError):
        C.fft_encode_packed(vec, vec.numel(), tw_enc, SCALE, s + 1)
    with pytest.raises(RuntimeError):              # tables of another ring
        C.fft_encode_packed(vec, vec.numel(), tw_enc, SCALE, 2 * s)
    bad_decode = [
        (good.cpu(), 3 * m),
        (good.to(torch.int32), 3 * m),
        (good.t(), 3 * m),
        (good, 0),
        (good, 3 * m + 1),                        # beyond B * 2 * slots
    ]
    for c, count in bad_decode:
        with pytest.raises(RuntimeError):
            C.fft_decode_packed(c, tw_dec, SCALE, count)
    sentinel = torch.full((6 * m,), -77.0, device="cuda")
    bad_out = [sentinel[:3 * m + 1],              # one too long
               sentinel[:3 * m - 1],              # one too short
               sentinel[:3 * m].double(),         # wrong dtype
               sentinel[::2],                     # right length, strided
               sentinel[:3 * m].cpu()]            # not on the device
    for out in bad_out:
        with pytest.raises(RuntimeError):
            C.fft_decode_packed(good, tw_dec, SCALE, 3 * m, out=out)
    assert (sentinel == -77.0).all()              # nothing was launched
    with pytest.raises(RuntimeError):              # more than 65535 rows
        C.fft_encode_packed(torch.zeros(65536 * 16, device="cuda"),
                            65536 * 16, _enc(16)._hip_tables("cuda")[0],
                            SCALE, 8)


# ----- 4. the engine on the device -----------------------------------------------

@functools.lru_cache(maxsize=None)
def _ctx(m, q_bits, device="cuda", packing="complex"):
    from hefl.he import CKKSContext
    return CKKSContext(HEConfig(m=m, scale_bits=40, q_bits=q_bits, seed=21,
                                packing=packing), device=device)


def _lazy_mean(ctx, pk, vecs):
    from hefl.he.ckks import CtxtTensor
    agg = None
    for i, v in enumerate(vecs):
        ctx.reseed(i)
        ct = ctx.encrypt_tensor(v, pk)
        agg = ct if agg is None else CtxtTensor(
            agg.data + ct.data, agg.scale, agg.count, agg.packing)
    ctx.modreduce_tensor_(agg)
    return ctx.rescale_tensor(ctx.mul_scalar_tensor(agg, 1.0 / len(vecs)))


@pytest.mark.parametrize("m,q_bits,count,k", [
    (8192, (60, 40), 222722, 8),                 # config #2: 28 instead of 55
    (256, (60, 40), 1000, 8),
    (32768, (60, 40, 40, 40), 2 * 32768 + 17, 2),   # level 4 -> 3
])
def test_engine_lazy_sum_mean_on_device(m, q_bits, count, k):
    ctx = _ctx(m, q_bits)
    kp = ctx.keygen()
    g = torch.Generator().manual_seed(count)
    vec = torch.randn(count, generator=g).cuda()
    vecs = [vec * (i + 1) for i in range(k)]
    avg = _lazy_mean(ctx, kp.pk, vecs)
    B = math.ceil(count / m)
    assert avg.packing == "complex" and avg.data.shape[0] == B
    assert avg.level == len(q_bits) - 1
    if m == 8192:
        assert B == 28
    out = ctx.decrypt_tensor(avg, kp.sk)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == (count,)
    err = (out - torch.stack(vecs).mean(0)).abs().max().item()
    print(f"m={m} B={B} k={k}: max err {err:.3e}")
    assert err < 1e-3


# ----- 5. the device context against the CPU context ------------------------------

def test_context_encode_decode_complex_matches_cpu():
    m, q_bits = 256, (60, 40)
    gpu, cpu = _ctx(m, q_bits), _ctx(m, q_bits, "cpu")
    assert gpu.primes == cpu.primes
    rng = np.random.default_rng(9)
    # fp32-representable parts: the device kernel takes fp32 pairs
    z = (rng.standard_normal((3, gpu.slots)).astype(np.float32)
         + 1j * rng.standard_normal((3, gpu.slots)).astype(np.float32)
         ).astype(np.complex128)
    pg, pc = gpu.encode(z), cpu.encode(z)
    assert pg.data.is_cuda and pg.data.shape == pc.data.shape == (3, 2, m)
    for i, q in enumerate(gpu.primes):
        a = gpu.backend.ntt(pg.data[..., i, :], i, inverse=True).cpu()
        b = cpu.backend.ntt(pc.data[..., i, :], i, inverse=True)
        d = torch.remainder(a - b, q)
        d = torch.minimum(d, q - d)                 # lifted to (-q/2, q/2]
        assert d.max().item() <= 1, (i, d.max())
    # one device plaintext, decoded on both sides (limb-0 shortcut, then the
    # single-limb branch)
    from hefl.he.ckks import Plaintext
    for data in (pg.data, pg.data[..., :1, :].contiguous()):
        on_gpu = gpu.decode(Plaintext(data, pg.scale), gpu.slots, complex=True)
        on_cpu = cpu.decode(Plaintext(data.cpu(), pg.scale), cpu.slots,
                            complex=True)
        assert on_gpu.is_cuda and on_gpu.is_complex()
        diff = np.abs(on_gpu.cpu().numpy() - on_cpu).max()
        print(f"decode, {data.shape[-2]} limb(s): gpu vs cpu {diff:.3e}")
        assert diff < 1e-5
        assert np.abs(on_cpu - z).max() < 1e-4


# ----- 6. threshold decryption on the device ---------------------------------------

def test_threshold_decrypt_complex_on_device():
    k, m, sb = 2, 8192, 16
    ctx = _ctx(m, (60, 40))
    g = torch.Generator().manual_seed(k)
    vecs = [torch.randn(m + 5, generator=g).cuda() for _ in range(k)]
    a = ctx.sample_crp()
    shares = [ctx.keygen_share(a, i) for i in range(k)]
    pk = ctx.combine_pk(torch.stack([s.b_share for s in shares]).sum(0), a)
    avg = _lazy_mean(ctx, pk, vecs)
    assert avg.data.shape[0] == 2
    acc = None
    for i, s in enumerate(shares):
        h = ctx.partial_decrypt_tensor(avg, s.sk_share, sb, lead=(i == 0))
        acc = h if acc is None else acc + h
    out = ctx.combine_shares_tensor(acc, avg.scale, avg.count,
                                    packing=avg.packing)
    err = (out - torch.stack(vecs).mean(0)).abs().max().item()
    print(f"threshold k={k} m={m}: max err {err:.3e}")
    assert err < 1e-3 + k * m * (2.0 ** sb) / avg.scale   # test_gpu_threshold


# ----- 7. world-size-1 aggregator and runner ----------------------------------------

@pytest.mark.parametrize("key_mode,denom_mode,q_bits", [
    ("shared", "plain", (60, 40)),
    ("threshold", "plain", (60, 40)),
    ("shared", "encrypted", (60, 40, 40)),
])
def test_aggregator_single_rank_complex(key_mode, denom_mode, q_bits):
    from hefl.fl.secure import SecureAggregator
    from hefl.he import CKKSContext
    m = 1024
    ctx = CKKSContext(HEConfig(m=m, scale_bits=40, q_bits=q_bits, seed=4,
                               packing="complex"), device="cuda")
    agg = SecureAggregator(ctx, 0, key_mode=key_mode, denom_mode=denom_mode,
                           n_clients=1, smudge_bits=16)
    vec = torch.randn(2 * m + 452,
                      generator=torch.Generator().manual_seed(1)).cuda()
    ct = agg.fedavg_ct(vec)
    assert ct.packing == "complex" and ct.data.shape[0] == 3
    out = agg.decrypt(ct)
    assert out.is_cuda and out.shape == vec.shape
    err = (out - vec).abs().max().item()
    print(f"{key_mode}/{denom_mode}: max err {err:.3e}")
    bound = 1e-3
    if key_mode == "threshold":
        bound += m * (2.0 ** 16) / ct.scale
    assert err < bound
    assert (agg.fedavg(vec) - vec).abs().max().item() < bound


def test_sequential_round_complex_on_device():
    """The existing GPU e2e test's preset and accuracy assertion, one round,
    complex packing."""
    from hefl.config import preset
    from hefl.fl.sequential import SequentialFL
    from hefl.fl.weights import flat_params
    torch.manual_seed(0)
    cfg = preset("config2")
    cfg.fl.n_clients = 2
    cfg.fl.samples_per_client = 96
    cfg.fl.test_samples = 96
    cfg.model.n_classes = 2
    cfg.he.seed = 17
    cfg.he.packing = "complex"
    fl = SequentialFL(cfg, device="cuda:0")
    rep = fl.run_round(epochs=2)
    assert fl.ctx.device.type == "cuda" and fl.ctx.values_per_ct == 8192
    assert all(math.isfinite(s["loss"]) for s in rep.client_stats)
    mean = torch.stack([c.get_weights() for c in fl.clients]).mean(0)
    err = (flat_params(fl.global_model) - mean).abs().max().item()
    print(f"SequentialFL complex: max err {err:.3e}, metrics {rep.metrics}")
    assert err < 1e-3
    assert rep.metrics["accuracy"] > 0.8, rep.metrics
