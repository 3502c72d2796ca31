"""n-of-n threshold CKKS decryption (key_mode="threshold") on the CPU oracle
backend: protocol correctness, privacy shape, the gloo multi-process path,
error paths and the CLI flags.

Error bound used throughout: the shared-key pipeline's 1e-3 (as in
test_fl_encrypted.py) plus the worst case the smudging noise can add to a
slot, k * n * 2^smudge_bits / scale (k parties, n coefficients each below
2^smudge_bits in magnitude, |slot| <= sum |coeff| / scale).
"""
import json
import multiprocessing as mp
import os
import subprocess
import sys

import pytest
import torch

from hefl.config import HEConfig
from hefl.he import CKKSContext, KeyShare
from hefl.he.ckks import CtxtTensor


def smudge_bound(k, n, sb, scale):
    return 1e-3 + k * n * (2.0 ** sb) / scale


def _vecs(k, count, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(count, generator=g) for _ in range(k)]


def _keygen(ctx, k):
    a = ctx.sample_crp()
    shares = [ctx.keygen_share(a, i) for i in range(k)]
    b_sum = torch.stack([s.b_share for s in shares]).sum(0)
    return shares, ctx.combine_pk(b_sum, a)


def _aggregate(ctx, pk, vecs):
    """encrypt each party's vector under the collective pk, lazy sum,
    modreduce, x 1/k, rescale — exactly the shared-mode pipeline."""
    agg = None
    for i, v in enumerate(vecs):
        ctx.reseed(i)
        ct = ctx.encrypt_tensor(v, pk)
        agg = ct if agg is None else CtxtTensor(agg.data + ct.data, agg.scale,
                                                agg.count)
    ctx.modreduce_tensor_(agg)
    return ctx.rescale_tensor(ctx.mul_scalar_tensor(agg, 1.0 / len(vecs)))


def _threshold_decrypt(ctx, avg, shares, sb):
    hs = [ctx.partial_decrypt_tensor(avg, s.sk_share, sb, lead=(i == 0))
          for i, s in enumerate(shares)]
    out = ctx.combine_shares_tensor(torch.stack(hs).sum(0), avg.scale,
                                    avg.count)
    return out, hs


@pytest.mark.parametrize("m,q_bits,scale_bits,k,sb", [
    (128, (50, 30), 30, 3, 0),
    (128, (50, 30), 30, 3, 10),
    (128, (50, 30), 30, 8, 12),
    (256, (60, 40, 40), 40, 2, 20),   # Lc = 2 after the rescale
])
def test_protocol_matches_plain_mean(m, q_bits, scale_bits, k, sb):
    ctx = CKKSContext(HEConfig(m=m, scale_bits=scale_bits, q_bits=q_bits,
                               seed=11))
    vecs = _vecs(k, 150)
    shares, pk = _keygen(ctx, k)
    assert all(isinstance(s, KeyShare) for s in shares)
    assert pk.shape == (2, ctx.L, ctx.n)
    avg = _aggregate(ctx, pk, vecs)
    assert avg.level == len(q_bits) - 1
    out, hs = _threshold_decrypt(ctx, avg, shares, sb)
    assert hs[0].shape == (avg.data.shape[0], avg.level, ctx.n)
    assert out.dtype == torch.float32 and out.shape == (150,)
    err = (out - torch.stack(vecs).mean(0)).abs().max().item()
    print(f"m={m} k={k} sb={sb}: max err {err:.3e}")
    assert err < 1e-3
    assert err < smudge_bound(k, m, sb, avg.scale)


def test_single_share_cannot_decrypt():
    ctx = CKKSContext(HEConfig(m=128, scale_bits=30, q_bits=(50, 30), seed=11))
    vecs = _vecs(3, 150)
    shares, pk = _keygen(ctx, 3)
    avg = _aggregate(ctx, pk, vecs)
    mean = torch.stack(vecs).mean(0)
    for s in shares:
        alone = ctx.decrypt_tensor(avg, s.sk_share)   # c0 + c1 * s_i
        assert (alone - mean).abs().max().item() > 1.0


def test_shares_differ_across_parties_with_fixed_seed():
    cfg = HEConfig(m=128, scale_bits=30, q_bits=(50, 30), seed=5)
    # one context per party, as on separate ranks: same he.seed everywhere
    ctxs = [CKKSContext(cfg) for _ in range(3)]
    a = ctxs[0].sample_crp()
    shares = [c.keygen_share(a, i) for i, c in enumerate(ctxs)]
    for i in range(3):
        for j in range(i + 1, 3):
            assert not torch.equal(shares[i].sk_share, shares[j].sk_share)
            assert not torch.equal(shares[i].b_share, shares[j].b_share)
    # and the per-party stream is reproducible from (seed, party)
    again = CKKSContext(cfg).keygen_share(a, 1)
    assert torch.equal(again.sk_share, shares[1].sk_share)
    # the share really is ternary: it must decode back to {-1, 0, 1}
    q0 = ctxs[0].primes[0]
    s = ctxs[0].backend.ntt(shares[1].sk_share[0], 0, inverse=True)
    s = torch.where(s > q0 // 2, s - q0, s)
    assert s.abs().max().item() <= 1 and s.abs().sum().item() > 0


def test_smudging_noise_is_fresh_per_decryption():
    sb, k, m = 10, 3, 128
    ctx = CKKSContext(HEConfig(m=m, scale_bits=30, q_bits=(50, 30), seed=11))
    vecs = _vecs(k, 150)
    shares, pk = _keygen(ctx, k)
    avg = _aggregate(ctx, pk, vecs)
    out1, hs1 = _threshold_decrypt(ctx, avg, shares, sb)
    out2, hs2 = _threshold_decrypt(ctx, avg, shares, sb)
    for h1, h2 in zip(hs1, hs2):
        assert not torch.equal(h1, h2)
    mean = torch.stack(vecs).mean(0)
    bound = smudge_bound(k, m, sb, avg.scale)
    assert (out1 - mean).abs().max().item() < bound
    assert (out2 - mean).abs().max().item() < bound
    assert (out1 - out2).abs().max().item() < 2 * bound


def test_injected_bits_make_the_share_deterministic():
    ctx = CKKSContext(HEConfig(m=128, scale_bits=30, q_bits=(50, 30), seed=11))
    shares, pk = _keygen(ctx, 2)
    avg = _aggregate(ctx, pk, _vecs(2, 100))
    g = torch.Generator().manual_seed(3)
    bits = torch.randint(-(2 ** 63), 2 ** 63 - 1, (avg.data.shape[0], ctx.n),
                         generator=g, dtype=torch.int64)
    h1 = ctx.partial_decrypt_data(avg.data, shares[1].sk_share, 10, False,
                                  bits=bits)
    h2 = ctx.partial_decrypt_data(avg.data, shares[1].sk_share, 10, False,
                                  bits=bits)
    assert torch.equal(h1, h2)
    # sb = 0 keeps one bit: e' = (bits & 1) - 1, so bits = 1 everywhere is
    # e' = 0 and the non-lead share is the bare c1 * s_i
    bare = ctx.partial_decrypt_data(avg.data, shares[1].sk_share, 0, False,
                                    bits=torch.ones_like(bits))
    want = torch.stack([ctx.backend.modmul(
        avg.data[:, 1, i], shares[1].sk_share[i].expand_as(avg.data[:, 1, i])
        .contiguous(), i) for i in range(avg.level)], dim=-2)
    assert torch.equal(bare, want)
    with pytest.raises(ValueError):
        ctx.partial_decrypt_data(avg.data, shares[1].sk_share, 10, False,
                                 bits=bits[:, :-1])


def test_combine_pk_reduces_eight_maximal_residues():
    ctx = CKKSContext(HEConfig(m=64, scale_bits=20, q_bits=(60, 40, 20),
                               seed=1))
    qs = torch.tensor(ctx.primes, dtype=torch.int64).view(-1, 1)
    one = (qs - 1).expand(ctx.L, ctx.n).contiguous()
    lazy = one * 8
    a = ctx.sample_crp()
    pk = ctx.combine_pk(lazy, a)
    assert torch.equal(pk[0], (qs - 8).expand(ctx.L, ctx.n))
    assert torch.equal(pk[1], a)
    assert torch.equal(lazy, one * 8)      # the caller's sum is not clobbered


# ----- error paths ---------------------------------------------------------

def _ctx3():
    return CKKSContext(HEConfig(m=128, scale_bits=30, q_bits=(50, 30, 30),
                                seed=5))


def test_threshold_rejects_encrypted_denominator():
    from hefl.fl.secure import SecureAggregator
    with pytest.raises(ValueError):
        SecureAggregator(_ctx3(), 0, denom_mode="encrypted", n_clients=2,
                         key_mode="threshold")


@pytest.mark.parametrize("sb", [-1, 49, 64])
def test_smudge_bits_out_of_range(sb):
    from hefl.fl.secure import SecureAggregator
    with pytest.raises(ValueError):
        SecureAggregator(_ctx3(), 0, key_mode="threshold", smudge_bits=sb)
    ctx = _ctx3()
    shares, pk = _keygen(ctx, 1)
    ct = ctx.encrypt_tensor(torch.zeros(10), pk)
    with pytest.raises(ValueError):
        ctx.partial_decrypt_tensor(ct, shares[0].sk_share, sb, True)


def test_unknown_key_mode_rejected():
    from hefl.config import preset
    from hefl.fl.secure import SecureAggregator
    from hefl.fl.sequential import SequentialFL
    with pytest.raises(ValueError):
        SecureAggregator(_ctx3(), 0, key_mode="split")
    cfg = preset("config2")
    cfg.fl.key_mode = "split"
    cfg.he.m = 256
    with pytest.raises(ValueError):
        SequentialFL(cfg, device="cpu")


def test_world_one_aggregator_holds_only_a_share_and_decrypts():
    from hefl.fl.secure import SecureAggregator
    agg = SecureAggregator(CKKSContext(HEConfig(
        m=128, scale_bits=30, q_bits=(50, 30), seed=5)), 0,
        key_mode="threshold", smudge_bits=10)
    vec = _vecs(1, 300)[0]
    out = agg.fedavg(vec)
    assert (out - vec).abs().max().item() < 1e-3
    assert "decrypt" in agg.stats.seconds


def test_sequential_fl_threshold_round_is_the_client_mean():
    from hefl.config import preset
    from hefl.fl.sequential import SequentialFL
    from hefl.fl.weights import flat_params
    cfg = preset("config2")
    cfg.fl.n_clients = 2
    cfg.fl.samples_per_client = 64
    cfg.he.m = 256
    cfg.he.seed = 3
    cfg.fl.key_mode = "threshold"
    fl = SequentialFL(cfg, device="cpu")
    assert fl.keys.sk is None and len(fl.key_shares) == 2
    fl.run_round(epochs=1)
    mean = torch.stack([c.get_weights() for c in fl.clients]).mean(0)
    err = (flat_params(fl.global_model) - mean).abs().max().item()
    assert err < smudge_bound(2, 256, cfg.fl.smudge_bits, 2.0 ** 40)


# ----- gloo multi-process --------------------------------------------------

def _env(rank, world, port):
    os.environ.update({
        "RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world),
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
    })


def _worker_direct(rank, world, port, q):
    _env(rank, world, port)
    import torch.distributed as dist
    from hefl.fl.secure import SecureAggregator
    from hefl.parallel.dist import init_distributed

    init_distributed(backend="gloo")
    expect = torch.stack([
        torch.randn(300, generator=torch.Generator().manual_seed(42 + r))
        for r in range(world)]).mean(0)
    vec = torch.randn(300, generator=torch.Generator().manual_seed(42 + rank))
    res = {}
    # default buckets; then (world 2 only) one ciphertext / one share per
    # all-reduce to exercise the bucketed share reduction
    for name, kw in [("default", {})] + (
            [("bucket1", {"bucket_bytes": 1})] if world == 2 else []):
        cfg = HEConfig(m=128, scale_bits=30, q_bits=(50, 30), seed=5)
        agg = SecureAggregator(CKKSContext(cfg), rank, key_mode="threshold",
                               smudge_bits=10, **kw)
        out = agg.fedavg(vec)
        sks = [torch.zeros_like(agg.keys.sk) for _ in range(world)]
        pks = [torch.zeros_like(agg.keys.pk) for _ in range(world)]
        dist.all_gather(sks, agg.keys.sk)
        dist.all_gather(pks, agg.keys.pk)
        res[name] = {
            "err": (out - expect).abs().max().item(),
            "sk_distinct": all(not torch.equal(sks[i], sks[j])
                               for i in range(world)
                               for j in range(i + 1, world)),
            "pk_same": all(torch.equal(pks[0], p) for p in pks[1:]),
        }
    q.put((rank, res))
    dist.destroy_process_group()


def _worker_round(rank, world, port, q):
    _env(rank, world, port)
    import torch.distributed as dist
    from hefl.config import preset
    from hefl.fl.round import FLRunner
    from hefl.parallel.dist import init_distributed

    init_distributed(backend="gloo")
    cfg = preset("config2")
    cfg.he.m = 256
    cfg.he.seed = 99
    cfg.fl.n_clients = world
    cfg.fl.samples_per_client = 64
    cfg.fl.key_mode = "threshold"
    runner = FLRunner(cfg, device="cpu", rank=rank)
    assert runner.agg.key_mode == "threshold"
    runner.run_round(epochs=1)
    local = runner.client.get_weights().clone()
    gathered = [torch.zeros_like(local) for _ in range(world)]
    dist.all_gather(gathered, local)
    same = torch.allclose(gathered[0], gathered[1], atol=1e-6)
    finite = bool(torch.isfinite(local).all()) and local.abs().max().item() < 1e3
    q.put((rank, bool(same), finite))
    dist.destroy_process_group()


def _run(target, world, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    return results


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_gloo_threshold_fedavg(world):
    from conftest import free_port
    results = _run(_worker_direct, world, free_port())
    assert len(results) == world
    for rank, res in results:
        assert set(res) == ({"default", "bucket1"} if world == 2
                            else {"default"})
        for name, r in res.items():
            assert r["err"] < 1e-3, (rank, name, r)
            assert r["sk_distinct"], (rank, name)
            assert r["pk_same"], (rank, name)


@pytest.mark.timeout(300)
def test_gloo_threshold_fl_round():
    from conftest import free_port
    results = _run(_worker_round, 2, free_port())
    assert all(same and finite for _, same, finite in results), results


# ----- CLI -----------------------------------------------------------------

def test_cli_threshold_key_mode():
    out = subprocess.run(
        [sys.executable, "-m", "hefl", "--preset", "config2", "--clients",
         "2", "--rounds", "1", "--epochs", "1", "--device", "cpu",
         "--key-mode", "threshold", "--smudge-bits", "12", "--json"],
        capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["clients"] == 2 and d["encrypted"] is True
    assert 0.0 <= d["metrics"]["accuracy"] <= 1.0
    bad = subprocess.run(
        [sys.executable, "-m", "hefl", "--key-mode", "split"],
        capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--key-mode" in bad.stderr
