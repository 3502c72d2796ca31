"""`image_batch` HIP kernel vs its CPU mirror, on i.i.d. uint8 noise: on
noise a one-pixel misplacement is an O(1) error, not something a tolerance
absorbs. Plus the capturable form, the epoch-graph wiring and the wrapper's
refusals."""
import os

import numpy as np
import pytest
import torch

import hefl
from hefl.config import preset
from hefl.data.files import (ImageFolderDataset, augment_params,
                             image_batch_reference)
from hefl.data.imageio import write_png

pytestmark = pytest.mark.gpu

INV255 = float(np.float32(1.0) / np.float32(255.0))
# one bf16 ulp in the top binade of [0, 1]: both sides sample the same
# continuous bilinear surface and differ by a few fp32 ulps (contraction,
# ordering), so one bf16 rounding step is the only admissible difference
TOL = 2.0 ** -8
FULL = (0.2, 0.2, True)


def C():
    return hefl.load_extension()


def rand_store(n, h, w, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8)


def mixed_idx(N, n=5):
    """n indices into [0, N): out of order, with a repeat."""
    idx = [(2 * k + 1) % N for k in range(n)]
    idx[-1] = idx[0]
    return torch.tensor(idx, dtype=torch.int64)


def run(store, idx, seed, H, W, aff=(0.0, 0.0, False)):
    out = C().image_batch(store.cuda(), idx.cuda(), seed, H, W, zoom=aff[0],
                          shear=aff[1], flip=int(aff[2]))
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16
    assert out.shape == (idx.numel(), H, W, store.shape[3])
    return out.cpu()


@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 7, 3), (8, 8, 1)])
@pytest.mark.parametrize("N", [3, 4, 5, 6, 7])
def test_fast_path_is_bit_exact(shape, N):
    # 4x4x4: 64 B/image (vector path); 5x7x3: 105 B (scalar fallback)
    h, w, c = shape
    store = rand_store(N, h, w, c, seed=N)
    idx = mixed_idx(N)
    want = (store[idx].float() * INV255).to(torch.bfloat16)
    assert torch.equal(run(store, idx, 0, h, w), want)


@pytest.mark.parametrize("shape", [(4, 4, 4), (5, 7, 3), (8, 8, 1)])
def test_fast_path_every_byte_value(shape):
    h, w, c = shape
    n = -(-256 // (h * w * c)) + 1
    store = (torch.arange(n * h * w * c) % 256).to(torch.uint8).view(n, h, w, c)
    assert store.unique().numel() == 256
    idx = torch.arange(n - 1, -1, -1)
    want = (store[idx].float() * INV255).to(torch.bfloat16)
    assert torch.equal(run(store, idx, 0, h, w), want)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("src,dst", [((13, 9), (8, 8)), ((4, 4), (11, 7)),
                                     ((6, 6), (1, 5)), ((6, 6), (5, 1))])
def test_resize_only(src, dst, c):
    store = rand_store(6, src[0], src[1], c, seed=7)
    idx = mixed_idx(6)
    ref = image_batch_reference(store, idx, 0, dst[0], dst[1])
    err = (run(store, idx, 0, dst[0], dst[1]).float() - ref).abs().max()
    print(f"resize {src}->{dst} C={c}: max |gpu-ref| = {float(err):.3e}")
    assert float(err) <= TOL


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("src,dst", [((12, 10), (12, 10)), ((13, 9), (8, 8))])
def test_full_augmentation(src, dst, c):
    n, seed = 6, 21
    zoom, shear, sf = augment_params(seed, n, *FULL)
    assert (sf < 0).any() and (sf > 0).any()  # a flipped and an unflipped one
    store = rand_store(7, src[0], src[1], c, seed=8)
    idx = torch.tensor([6, 2, 2, 0, 5, 1])
    ref = image_batch_reference(store, idx, seed, dst[0], dst[1], *FULL)
    err = (run(store, idx, seed, dst[0], dst[1], FULL).float() - ref).abs().max()
    print(f"augment {src}->{dst} C={c}: max |gpu-ref| = {float(err):.3e}")
    assert float(err) <= TOL


def test_more_than_one_block_and_grid_stride():
    # 40 x 33 x 31 pixels = 160 blocks of 256; odd sizes, C = 3
    store = rand_store(9, 35, 37, 3, seed=3)
    idx = torch.randint(0, 9, (40,), generator=torch.Generator().manual_seed(1))
    ref = image_batch_reference(store, idx, 77, 33, 31, *FULL)
    err = (run(store, idx, 77, 33, 31, FULL).float() - ref).abs().max()
    assert float(err) <= TOL


def test_source_offsets_past_2_31_bytes():
    # image 2049 of a [2050, 1024, 1024, 1] store starts 2049 * 2^20 bytes in:
    # a 32-bit source offset would wrap. Vector, scalar and general paths.
    g = torch.Generator(device="cuda").manual_seed(5)
    store = torch.randint(0, 256, (2050, 1024, 1024, 1), generator=g,
                          dtype=torch.uint8, device="cuda")
    idx = torch.tensor([2049, 0, 2048], device="cuda")
    out = C().image_batch(store, idx, 0, 1024, 1024)
    assert torch.equal(out, (store[idx].float() * INV255).to(torch.bfloat16))
    # the same memory as 1023x1025 images (1,048,575 B each: scalar fallback)
    odd = store.view(-1)[:2050 * 1023 * 1025].view(2050, 1023, 1025, 1)
    out = C().image_batch(odd, idx, 0, 1023, 1025)
    assert torch.equal(out, (odd[idx].float() * INV255).to(torch.bfloat16))
    small = store[idx].cpu()
    ref = image_batch_reference(small, torch.arange(3), 9, 24, 20, *FULL)
    got = C().image_batch(store, idx, 9, 24, 20, zoom=0.2, shear=0.2, flip=1)
    torch.cuda.synchronize()
    assert float((got.float().cpu() - ref).abs().max()) <= TOL


def test_seed_buffer_form_matches_the_scalar_seed():
    store = rand_store(5, 9, 11, 3, seed=4).cuda()
    idx = mixed_idx(5).cuda()
    seed_buf = torch.tensor([123456789], dtype=torch.int64, device="cuda")
    a = C().image_batch_g(store, idx, seed_buf, 17, 8, 8, zoom=0.2, shear=0.2,
                          flip=1)
    b = C().image_batch(store, idx, 123456789 + 17, 8, 8, zoom=0.2, shear=0.2,
                        flip=1)
    other = C().image_batch(store, idx, 123456789 + 18, 8, 8, zoom=0.2,
                            shear=0.2, flip=1)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, other)


@pytest.fixture(scope="module")
def noise_folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("noise")
    rng = np.random.default_rng(9)
    for cls in ("a", "b"):
        os.makedirs(root / cls)
        for i in range(4):
            write_png(str(root / cls / f"{i}.png"),
                      rng.integers(0, 256, (10, 9, 3), dtype=np.uint8))
    return str(root)


def test_dataset_batch_runs_the_kernel(noise_folder):
    ds = ImageFolderDataset(noise_folder, (8, 8, 3), device="cuda",
                            dtype=torch.bfloat16, seed=2)
    assert ds.store.is_cuda and ds.store.shape == (8, 10, 9, 3)
    idx = torch.tensor([5, 0, 7, 5])
    x, y = ds.batch(idx, affine=FULL)
    assert x.dtype == torch.bfloat16 and x.is_cuda
    ref = image_batch_reference(ds.store, idx, ds.seed * 0x10001 + 1, 8, 8,
                                *FULL)
    assert float((x.float().cpu() - ref).abs().max()) <= TOL
    assert torch.equal(y.cpu(), ds.labels.cpu()[idx])
    with pytest.raises(IndexError):
        ds.batch(torch.tensor([8]))


def test_graph_batch_capture_and_replay(noise_folder):
    ds = ImageFolderDataset(noise_folder, (8, 8, 3), device="cuda",
                            dtype=torch.bfloat16, seed=2)
    order = torch.arange(8, device="cuda")
    seed_buf = torch.zeros(1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ds.graph_batch(order, seed_buf, FULL)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        X, Y = ds.graph_batch(order, seed_buf, FULL)
    for perm, seed in (([3, 1, 7, 0, 2, 6, 5, 4], 1001),
                       ([4, 4, 0, 6, 1, 3, 2, 7], 52)):
        order.copy_(torch.tensor(perm))
        seed_buf.fill_(seed)
        g.replay()
        eager = C().image_batch(ds.store, order, seed, 8, 8, zoom=0.2,
                                shear=0.2, flip=1)
        torch.cuda.synchronize()
        assert torch.equal(X, eager)
        assert torch.equal(Y, ds.labels[order])
        ref = image_batch_reference(ds.store, order, seed, 8, 8, *FULL)
        assert float((X.float().cpu() - ref).abs().max()) <= TOL


def test_wrapper_refusals():
    store = rand_store(3, 4, 4, 3).cuda()
    idx = torch.tensor([0, 1], device="cuda")
    bad = {
        "fp32 store": (store.float(), idx),
        "C = 2": (rand_store(3, 4, 4, 2).cuda(), idx),
        "non-contiguous store": (rand_store(3, 4, 8, 3).cuda()[:, :, ::2], idx),
        "CPU store": (store.cpu(), idx),
        "CPU idx": (store, idx.cpu()),
        "int32 idx": (store, idx.int()),
    }
    for name, (s, i) in bad.items():
        with pytest.raises(RuntimeError):
            C().image_batch(s, i, 0, 4, 4)
            pytest.fail(f"{name} was launched")
    # 2 x 32768 x 32768 x 3 output elements >= 2^32: refused before any
    # allocation (the index decode is 32-bit)
    with pytest.raises(RuntimeError):
        C().image_batch(store, idx, 0, 32768, 32768)
    torch.cuda.synchronize()


def make_separable(root, n, seed):
    rng = np.random.default_rng(seed)
    for k, name in enumerate(("dark", "bright")):
        os.makedirs(os.path.join(root, name))
        for i in range(n // 2):
            a = rng.integers(0, 80, (28, 28, 1)) + 150 * k
            write_png(os.path.join(root, name, f"{i:03d}.png"),
                      a.astype(np.uint8))


def test_local_client_trains_a_folder_through_the_epoch_graph(tmp_path):
    from hefl.fl.client import LocalClient
    make_separable(str(tmp_path / "train"), 64, 1)
    make_separable(str(tmp_path / "test"), 40, 2)
    cfg = preset("config1")
    cfg.model.n_classes = 2
    cfg.fl.n_clients = 1
    cfg.fl.val_samples_per_client = 0   # all 64 images train (2 steps of 32)
    cfg.fl.augment = "full"
    cfg.fl.data_dir = str(tmp_path / "train")
    cfg.fl.test_dir = str(tmp_path / "test")
    c = LocalClient(cfg, 0, device="cuda")
    assert c.loader.indices.numel() == 64 and c.loader.batch_size == 32
    s1 = c.local_train(epochs=3)
    assert c._ep_ent["in_graph_data"] is True
    assert s1.steps == 6 and s1.samples == 192
    s2 = c.local_train(epochs=3)
    print(f"loss {s1.train_loss:.4f} -> {s2.train_loss:.4f}")
    assert s2.train_loss < s1.train_loss
    test_ds = ImageFolderDataset(cfg.fl.test_dir, cfg.model.in_shape,
                                 device="cuda", dtype=torch.bfloat16,
                                 seed=cfg.fl.seed)
    y, p = c.evaluate(test_ds, torch.arange(test_ds.n_samples))
    acc = float((y == p).float().mean())
    print(f"held-out accuracy {acc:.3f}")
    assert acc >= 0.9
