"""Complex packing (HEConfig.packing="complex") on the exact CPU backend: slot
j of ciphertext b carries w[b*n + j] + i*w[b*n + slots + j], so a ciphertext
holds n weights instead of n/2.

Tolerances are the project's own for the same operations at the same rings:
1e-4 for an encrypt/decrypt round trip (test_he_cpu.py, m=64, (50, 30), scale
2^30), 1e-3 for the eight-way lazy-sum mean and for ct x ct at (55, 26, 26),
test_threshold_cpu.py's 1e-3 and smudging bound, test_rotate_cpu.py's
key-switch slot tolerance and test_hoist_cpu.py's 1e-4 * peak for the linear
transform.
"""
import json
import math
import multiprocessing as mp
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from hefl.config import HEConfig, preset
from hefl.he import CKKSContext, Pyfhel
from hefl.he.ckks import Ciphertext, CtxtTensor
from hefl.he.encoder import Encoder
from hefl.he.linear import LinearTransform

SMALL = HEConfig(m=64, scale_bits=30, q_bits=(50, 30), seed=1,
                 packing="complex")


@pytest.fixture(scope="module")
def ctx():
    return CKKSContext(SMALL)


@pytest.fixture(scope="module")
def keys(ctx):
    return ctx.keygen()


# ----- 1. / 2. the oracle -----------------------------------------------------

def test_oracle_restricts_to_the_real_encoder():
    enc = Encoder(64)
    rng = np.random.default_rng(0)
    for k in (enc.slots, 5):
        v = rng.normal(size=(3, k))
        c_real = enc.encode(v, 2.0 ** 30)
        c_cplx = enc.encode_complex(v + 0j, 2.0 ** 30)
        assert c_cplx.dtype == c_real.dtype == np.int64
        assert np.array_equal(c_cplx, c_real)
        back = enc.decode_complex(c_real, 2.0 ** 30, k)
        assert np.array_equal(back.real, enc.decode(c_real, 2.0 ** 30, k))
    # the overflow guard: past 2^52 both switch to exact Python ints
    big = enc.encode_complex(np.array([1.0 + 2.0j]), 2.0 ** 60)
    assert big.dtype == object and isinstance(big.reshape(-1)[0], int)
    assert enc.encode(np.array([1.0]), 2.0 ** 60).dtype == object
    with pytest.raises(ValueError, match="too many"):
        enc.encode_complex(np.zeros(enc.slots + 1, dtype=complex), 2.0 ** 30)


def test_oracle_against_direct_evaluation_at_the_roots():
    """Independent of the special FFT: the encoded polynomial, evaluated at
    zeta^(5^j) by direct summation, is the complex input up to the rounding
    of n coefficients by at most 1/2 each, n / (2 * scale) per part."""
    n, scale = 64, 2.0 ** 30
    enc = Encoder(n)
    rng = np.random.default_rng(1)
    z = rng.normal(size=enc.slots) + 1j * rng.normal(size=enc.slots)
    coeffs = enc.encode_complex(z, scale).astype(np.float64)
    zeta = np.exp(2j * np.pi / (2 * n))
    roots = np.array([zeta ** pow(5, j, 2 * n) for j in range(enc.slots)])
    powers = roots[:, None] ** np.arange(n)[None, :]          # [slots, n]
    got = (powers * coeffs[None, :]).sum(axis=1) / scale
    bound = n / (2 * scale) + 1e-12                           # + float slack
    print(f"max part error {max(np.abs((got - z).real).max(), np.abs((got - z).imag).max()):.3e}, "
          f"bound {bound:.3e}")
    assert np.abs((got - z).real).max() <= bound
    assert np.abs((got - z).imag).max() <= bound
    # and the oracle's own decode agrees with the direct evaluation
    assert np.abs(enc.decode_complex(coeffs, scale, enc.slots) - got).max() < 1e-9


def test_torch_counterparts_match_the_oracle():
    enc = Encoder(64)
    rng = np.random.default_rng(2)
    z = rng.normal(size=(2, enc.slots)) + 1j * rng.normal(size=(2, enc.slots))
    c_np = enc.encode_complex(z, 2.0 ** 30)
    c_t = enc.encode_complex_torch(torch.from_numpy(z), 2.0 ** 30)
    assert c_t.dtype == torch.int64
    assert np.abs(c_t.numpy() - c_np).max() <= 1
    d_t = enc.decode_complex_torch(torch.from_numpy(c_np), 2.0 ** 30, 7)
    assert np.abs(d_t.numpy() - enc.decode_complex(c_np, 2.0 ** 30, 7)).max() < 1e-9
    # packed: the CPU composes the oracle
    vec = torch.randn(64 + 32 + 3)
    cp = enc.encode_packed_torch(vec, 2.0 ** 30)
    assert cp.shape == (2, 64)
    assert np.array_equal(cp.numpy(), enc.encode_complex(
        enc.pack_complex(vec.numpy()), 2.0 ** 30))
    back = enc.decode_packed_torch(cp, 2.0 ** 30, vec.numel())
    assert back.dtype == torch.float32 and back.shape == vec.shape
    assert (back - vec).abs().max().item() < 1e-5
    out = torch.full((vec.numel(),), 9.0)
    assert enc.decode_packed_torch(cp, 2.0 ** 30, vec.numel(), out=out) is out
    assert torch.equal(out, back)


# ----- 3. encrypt_tensor / decrypt_tensor -------------------------------------

def _counts(c):
    s, n = c.slots, c.n
    return [1, s - 1, s, s + 1, n, n + 1, n + s + 3, 3 * n]


def test_tensor_roundtrip_counts(ctx, keys):
    assert ctx.values_per_ct == ctx.n
    g = torch.Generator().manual_seed(3)
    for count in _counts(ctx):
        vec = torch.randn(count, generator=g)
        ct = ctx.encrypt_tensor(vec, keys.pk)
        assert ct.packing == "complex" and ct.count == count
        assert ct.data.shape[0] == math.ceil(count / ctx.n)
        back = ctx.decrypt_tensor(ct, keys.sk)
        assert back.dtype == torch.float32 and back.shape == (count,)
        err = (back - vec).abs().max().item()
        print(f"count {count}: B {ct.data.shape[0]}, max err {err:.3e}")
        assert err < 1e-4        # test_he_cpu.py::test_tensor_pack_roundtrip


def test_context_encode_decode_complex(ctx, keys):
    rng = np.random.default_rng(4)
    z = rng.normal(size=ctx.slots) + 1j * rng.normal(size=ctx.slots)
    ct = ctx.encrypt(ctx.encode(z), keys.pk)
    pt = ctx.decrypt(ct, keys.sk)                       # limb-0 shortcut
    out = ctx.decode(pt, ctx.slots, complex=True)
    assert np.iscomplexobj(out) and np.abs(out - z).max() < 1e-4
    assert np.array_equal(ctx.decode(pt, ctx.slots), out.real)
    low = ctx.decrypt(ctx.rescale(ctx.mul_scalar(ct, 1.0)), keys.sk)
    assert low.data.shape[-2] == 1                      # one limb
    assert np.abs(ctx.decode(low, 5, complex=True) - z[:5]).max() < 1e-4
    # big-int CRT: a plaintext at scale 2^60 is far past the shortcut
    pt_big = ctx.encode(z, scale=2.0 ** 60)
    out_big = ctx.decode(pt_big, ctx.slots, complex=True)
    assert np.abs(out_big - z).max() < 1e-9
    # a real input takes the real path, bit for bit
    v = rng.normal(size=ctx.slots)
    assert torch.equal(ctx.encode(v).data, ctx.encode(v + 0j).data)


# ----- 4. the FedAvg pipeline -------------------------------------------------

def _lazy_sum(c, pk, vecs):
    agg = None
    for i, v in enumerate(vecs):
        c.reseed(i)
        ct = c.encrypt_tensor(v, pk)
        agg = ct if agg is None else CtxtTensor(
            agg.data + ct.data, agg.scale, agg.count, agg.packing)
    return c.modreduce_tensor_(agg)


def test_lazy_sum_fedavg_complex(ctx, keys):
    vec = torch.randn(100, generator=torch.Generator().manual_seed(5))
    vecs = [vec * (i + 1) for i in range(8)]
    agg = _lazy_sum(ctx, keys.pk, vecs)
    avg = ctx.rescale_tensor(ctx.mul_scalar_tensor(agg, 1.0 / 8))
    assert avg.packing == "complex" and avg.data.shape[0] == 2
    out = ctx.decrypt_tensor(avg, keys.sk)
    assert (out - torch.stack(vecs).mean(0)).abs().max().item() < 1e-3


def test_encrypted_denominator_complex():
    """ct x enc(1/8) + relinearise + rescale at the (55, 26, 26) chain of
    test_mul_ct_relin_rescale: 1/n is a real constant in every slot, so both
    parts of a slot are divided."""
    from hefl.fl.secure import SecureAggregator
    cfg = HEConfig(m=64, scale_bits=26, q_bits=(55, 26, 26), seed=0,
                   packing="complex")
    agg = SecureAggregator(CKKSContext(cfg), denom_mode="encrypted",
                           n_clients=8)
    c = agg.ctx
    g = torch.Generator().manual_seed(6)
    vecs = [torch.randn(c.n + 9, generator=g) * 0.5 for _ in range(8)]
    summed = _lazy_sum(c, agg.keys.pk, vecs)
    avg = agg._divide(summed, 8)
    assert avg.packing == "complex" and avg.level == 2
    out = agg.decrypt(avg)
    assert (out - torch.stack(vecs).mean(0)).abs().max().item() < 1e-3


# ----- 5. threshold mode ------------------------------------------------------

@pytest.mark.parametrize("k,sb", [(2, 10), (8, 12)])
def test_threshold_decrypt_complex(k, sb):
    m = 128
    c = CKKSContext(HEConfig(m=m, scale_bits=30, q_bits=(50, 30), seed=11,
                             packing="complex"))
    g = torch.Generator().manual_seed(7)
    vecs = [torch.randn(m + 22, generator=g) for _ in range(k)]
    a = c.sample_crp()
    shares = [c.keygen_share(a, i) for i in range(k)]
    pk = c.combine_pk(torch.stack([s.b_share for s in shares]).sum(0), a)
    agg = _lazy_sum(c, pk, vecs)
    avg = c.rescale_tensor(c.mul_scalar_tensor(agg, 1.0 / k))
    hs = [c.partial_decrypt_tensor(avg, s.sk_share, sb, lead=(i == 0))
          for i, s in enumerate(shares)]
    out = c.combine_shares_tensor(torch.stack(hs).sum(0), avg.scale,
                                  avg.count, packing="complex")
    assert out.shape == (m + 22,)
    err = (out - torch.stack(vecs).mean(0)).abs().max().item()
    print(f"k={k} sb={sb}: max err {err:.3e}")
    assert err < 1e-3
    assert err < 1e-3 + k * m * (2.0 ** sb) / avg.scale   # smudge_bound
    # read as real packing the same shares give the first halves only
    hs = [c.partial_decrypt_tensor(avg, s.sk_share, sb, lead=(i == 0))
          for i, s in enumerate(shares)]
    real = c.combine_shares_tensor(torch.stack(hs).sum(0), avg.scale, 10)
    assert (real - torch.stack(vecs).mean(0)[:10]).abs().max().item() < 1e-3


# ----- 6. slot operations -----------------------------------------------------

def _hop_bound(c, l):
    """test_rotate_cpu.py: worst-case coefficient error of one key-switch."""
    q_max = max(c.primes[:l])
    return l * c.n * 21 * q_max / c.special + (c.n + 1) / 2 + 1


def _slot_tol(c, l, scale, hops=1):
    return hops * _hop_bound(c, l) * c.n / scale


@pytest.fixture(scope="module")
def rot_case():
    c = CKKSContext(HEConfig(m=64, scale_bits=30, q_bits=(50, 30, 30),
                             seed=11, packing="complex"))
    kp = c.keygen()
    gk = c.galois_keygen(kp.sk, steps=[1, -3], conjugate=True)
    v = np.random.default_rng(5).uniform(-1, 1, 2 * c.n)
    ct = c.encrypt_tensor(torch.from_numpy(v).float(), kp.pk)
    v = v.astype(np.float32).astype(np.float64)
    enc_err = np.abs(c.decrypt_tensor(ct, kp.sk).double().numpy() - v).max()
    return c, kp, gk, v, ct, enc_err


def _halves(c, v):
    return v.reshape(-1, 2, c.slots)            # [B, half, slots]


@pytest.mark.parametrize("step", [1, -3])
def test_rotate_rolls_both_halves(rot_case, step):
    c, kp, gk, v, ct, enc_err = rot_case
    out = c.rotate_tensor(ct, step, gk)
    assert out.packing == "complex" and out.count == ct.count
    got = c.decrypt_tensor(out, kp.sk).double().numpy()
    want = np.roll(_halves(c, v), -step, axis=-1).reshape(-1)
    err = np.abs(got - want).max()
    tol = _slot_tol(c, ct.level, ct.scale) + enc_err
    print(f"step {step}: error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    many = c.rotate_many_tensor(ct, [step], gk)[0]
    assert many.packing == "complex"
    got = c.decrypt_tensor(many, kp.sk).double().numpy()
    assert np.abs(got - want).max() <= tol       # hoisted: the same bound


def test_conjugate_negates_second_halves(rot_case):
    c, kp, gk, v, ct, enc_err = rot_case
    out = c.conjugate_tensor(ct, gk)
    assert out.packing == "complex"
    want = _halves(c, v).copy()
    want[:, 1] *= -1
    got = c.decrypt_tensor(out, kp.sk).double().numpy()
    assert np.abs(got - want.reshape(-1)).max() <= \
        _slot_tol(c, ct.level, ct.scale) + enc_err


def test_sum_slots_sums_each_half(rot_case):
    c, kp, gk, v, ct, enc_err = rot_case
    w = 2
    out = c.sum_slots_tensor(ct, gk, w)
    assert out.packing == "complex"
    h = _halves(c, v)
    want = (h + np.roll(h, -1, axis=-1)).reshape(-1)
    got = c.decrypt_tensor(out, kp.sk).double().numpy()
    # test_rotate_cpu.py: w * enc_err + (w - 1) hops
    assert np.abs(got - want).max() <= \
        w * enc_err + (w - 1) * _slot_tol(c, ct.level, ct.scale)


def test_linear_transform_maps_both_halves(rot_case):
    c, kp, _, v, ct, _ = rot_case
    M = np.random.default_rng(17).uniform(-1, 1, (4, 8))   # MAT_SHAPE n64
    lt = LinearTransform(c, M, level=ct.level)
    gk = c.galois_keygen(kp.sk, steps=lt.steps)
    out = c.rescale_tensor(lt.apply_tensor(ct, gk))
    assert out.packing == "complex"
    h = _halves(c, v)
    want = np.zeros_like(h)
    want[:, :, :4] = h[:, :, :8] @ M.T
    got = c.decrypt_tensor(out, kp.sk).double().numpy()
    peak = np.abs(want).max()
    err = np.abs(got - want.reshape(-1)).max()
    print(f"linear transform: error {err:.3e}, peak {peak:.3f}")
    assert err < 1e-4 * peak
    assert c.matvec(M, ct, gk).packing == "complex"


# ----- 7. serialisation and error paths ---------------------------------------

def test_error_paths(ctx, keys):
    with pytest.raises(ValueError, match="packing"):
        HEConfig(packing="x")
    real_ctx = CKKSContext(HEConfig(m=64, scale_bits=30, q_bits=(50, 30),
                                    seed=1))
    vec = torch.randn(10)
    a = ctx.encrypt_tensor(vec, keys.pk)
    b = real_ctx.encrypt_tensor(vec, keys.pk)
    assert a.data.shape == b.data.shape
    with pytest.raises(ValueError, match="packed"):
        ctx.add_tensor(a, b)
    assert ctx.add_tensor(a, a).packing == "complex"
    with pytest.raises(ValueError, match="empty"):
        ctx.encrypt_tensor(torch.zeros(0), keys.pk)
    with pytest.raises(ValueError, match="at most"):
        ctx._decode_tensor(a.data[:, 0], a.scale, ctx.n + 1, "complex")
    with pytest.raises(ValueError, match="unknown packing"):
        ctx._decode_tensor(a.data[:, 0], a.scale, 1, "x")


def test_export_import_keeps_the_packing(tmp_path):
    from hefl.fl.export import (decrypt_into_model, encrypt_model_weights,
                                export_weights, import_encrypted_weights)
    from hefl.models import CNN2

    he = Pyfhel()
    he.contextGen(m=256, q_bits=(50, 30), scale_bits=30, seed=2,
                  packing="complex")
    he.keyGen()
    model = CNN2((28, 28, 1), 2, seed=5)
    weights = encrypt_model_weights(he, model)
    for p, d in zip(model.parameters(), weights.values()):
        assert d["packing"] == "complex"
        assert d["data"].shape[0] == math.ceil(p.numel() / 256)
    path = str(tmp_path / "client_1.pickle")
    export_weights(path, weights, he)
    he2, val = import_encrypted_weights(path)
    assert he2.context.cfg.packing == "complex"
    assert all(ct.packing == "complex" for ct in val.values())
    he2._sk = he._sk
    m2 = CNN2((28, 28, 1), 2, seed=77)
    decrypt_into_model(he2, val, m2)
    for a, b in zip(model.parameters(), m2.parameters()):
        assert (a - b).abs().max() < 1e-3
    # the dict form, as decrypt_into_model also takes it
    m3 = CNN2((28, 28, 1), 2, seed=78)
    decrypt_into_model(he2, weights, m3)
    for a, b in zip(model.parameters(), m3.parameters()):
        assert (a - b).abs().max() < 1e-3


def test_export_dict_without_packing_reads_as_real(tmp_path):
    from hefl.fl.export import (encrypt_model_weights, export_weights,
                                import_encrypted_weights)
    from hefl.models import CNN2

    he = Pyfhel()
    he.contextGen(m=256, q_bits=(50, 30), scale_bits=30, seed=2)
    he.keyGen()
    weights = encrypt_model_weights(he, CNN2((28, 28, 1), 2, seed=5))
    for d in weights.values():
        assert d.pop("packing") == "real"
    path = str(tmp_path / "old.pickle")
    export_weights(path, weights, he)
    he2, val = import_encrypted_weights(path)
    assert he2.context.cfg.packing == "real"
    assert all(ct.packing == "real" for ct in val.values())


def test_facade_bytes_and_pickle_keep_the_packing():
    he = Pyfhel()
    he.contextGen(m=64, q_bits=(50, 30), scale_bits=30, seed=1,
                  packing="complex")
    he.keyGen()
    he2 = pickle.loads(pickle.dumps(he))
    assert he2.context.cfg.packing == "complex"
    assert he2.context.values_per_ct == 64
    for blob, load in ((he.to_bytes_context(), "from_bytes_context"),
                       (he.to_bytes_publicKey(), "from_bytes_publicKey"),
                       (he.to_bytes_secretKey(), "from_bytes_secretKey")):
        fresh = Pyfhel()
        getattr(fresh, load)(blob)
        assert fresh.context.cfg.packing == "complex"
    # a real-packing stream is what it was before the field existed
    # (version 1, nothing after the q_bits) and reads as real
    real = Pyfhel()
    real.contextGen(m=64, q_bits=(50, 30), scale_bits=30, seed=1)
    blob = real.to_bytes_context()
    assert blob[4:6] == b"\x01\x00" and len(blob) == 24 + 8
    assert len(he.to_bytes_context()) == len(blob) + 1
    fresh = Pyfhel()
    fresh.from_bytes_context(blob)
    assert fresh.context.cfg.packing == "real"
    # a pickled HEConfig from before the field has no such attribute
    old = HEConfig.__new__(HEConfig)
    state = dict(vars(HEConfig(m=64, q_bits=(50, 30), scale_bits=30)))
    del state["packing"]
    old.__dict__.update(state)
    assert pickle.loads(pickle.dumps(old)).packing == "real"
    # the scalar API stays one real value per ciphertext
    assert abs(he.decryptFrac(he.encryptFrac(1.25)) - 1.25) < 1e-4
    # a checkpoint carries the context bytes
    ct = he.encrypt_tensor(torch.arange(70.0) / 70)
    assert ct.packing == "complex" and ct.data.shape[0] == 2
    assert (he.decrypt_tensor(ct) - torch.arange(70.0) / 70).abs().max() < 1e-4


def test_checkpoint_keeps_the_packing(tmp_path):
    from hefl.fl.checkpoint import load_round_state, save_round_state
    from hefl.models import CNN2
    from hefl.ops.adam import FusedAdam

    he = Pyfhel()
    he.contextGen(m=64, q_bits=(50, 30), scale_bits=30, seed=1,
                  packing="complex")
    he.keyGen()
    m = CNN2((28, 28, 1), 2, seed=3)
    opt = FusedAdam(m.parameters(), lr=2e-3)
    save_round_state(str(tmp_path / "round.pt"), m, opt, round_idx=1, he=he)
    he2 = Pyfhel()
    load_round_state(str(tmp_path / "round.pt"), CNN2((28, 28, 1), 2, seed=4),
                     FusedAdam(m.parameters(), lr=1e-9), he=he2)
    assert he2.context.cfg.packing == "complex"


# ----- 8. runners and CLI -----------------------------------------------------

def _tiny_cfg(key_mode):
    cfg = preset("config2")
    cfg.fl.n_clients = 2
    cfg.fl.samples_per_client = 64
    cfg.fl.test_samples = 96
    cfg.fl.key_mode = key_mode
    cfg.he.m = 256
    cfg.he.seed = 7
    cfg.he.packing = "complex"
    cfg.model.n_classes = 2
    return cfg


@pytest.mark.parametrize("key_mode", ["shared", "threshold"])
def test_sequential_round_complex(key_mode):
    from hefl.fl.sequential import SequentialFL
    from hefl.fl.weights import flat_params
    torch.manual_seed(0)
    fl = SequentialFL(_tiny_cfg(key_mode), device="cpu")
    assert fl.ctx.values_per_ct == 256
    rep = fl.run_round(epochs=1)
    mean = torch.stack([c.get_weights() for c in fl.clients]).mean(0)
    got = flat_params(fl.global_model)
    assert got.shape == mean.shape
    assert (got - mean).abs().max().item() < 1e-3
    assert set(rep.metrics) == {"accuracy", "precision", "recall", "f1"}


def _worker(rank, world, port, q):
    os.environ.update({
        "RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world),
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
    })
    import torch.distributed as dist
    from hefl.fl.aggregate import plaintext_fedavg
    from hefl.fl.round import FLRunner
    from hefl.parallel.dist import init_distributed

    init_distributed(backend="gloo")
    cfg = _tiny_cfg("shared")
    cfg.he.seed = 99
    runner = FLRunner(cfg, device="cpu", rank=rank)
    runner.client.local_train(1)
    vec = runner.client.get_weights()
    expect = plaintext_fedavg(vec.clone())
    # buckets of 100 ciphertexts: several slabs, the pipelined path
    runner.agg.bucket_bytes = 100 * 2 * runner.agg.ctx.L * 256 * 8
    ct = runner.agg.fedavg_ct(vec, n_clients=world)
    B = ct.data.shape[0]
    out = runner.agg.decrypt(ct)
    err = (out - expect).abs().max().item()
    # and the runner's own round goes through
    res = runner.run_round(epochs=1)
    q.put((rank, err, B, vec.numel(), ct.packing, float(res.round_seconds)))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_process_runner_complex():
    from conftest import free_port
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = free_port()
    procs = [mpc.Process(target=_worker, args=(r, 2, port, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    for rank, err, B, count, packing, _ in results:
        assert packing == "complex" and B == math.ceil(count / 256)
        assert B > 100                        # more than one slab
        assert err < 1e-3, (rank, err)


def test_cli_accepts_he_packing():
    out = subprocess.run(
        [sys.executable, "-m", "hefl", "--preset", "config1", "--rounds", "1",
         "--epochs", "1", "--clients", "2", "--device", "cpu", "--json",
         "--he-packing", "complex"],
        capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["clients"] == 2 and d["he_packing"] == "complex"
    bad = subprocess.run(
        [sys.executable, "-m", "hefl", "--he-packing", "polar"],
        capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--he-packing" in bad.stderr


# ----- 9. defaults ------------------------------------------------------------

def test_defaults_stay_real():
    assert HEConfig().packing == "real"
    assert HEConfig().values_per_ct == HEConfig().slots
    c = CKKSContext(HEConfig(m=64, scale_bits=30, q_bits=(50, 30), seed=1))
    kp = c.keygen()
    assert c.values_per_ct == c.slots
    for count in (1, c.slots, c.slots + 1, 5 * c.slots + 7):
        ct = c.encrypt_tensor(torch.randn(count), kp.pk)
        assert ct.packing == "real"
        assert ct.data.shape[0] == math.ceil(count / c.slots)
    assert CtxtTensor(ct.data, ct.scale, ct.count).packing == "real"
    assert isinstance(c.encrypt(c.encode(np.ones(3)), kp.pk), Ciphertext)
