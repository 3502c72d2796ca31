"""Real-image folders on the CPU path: the `image_batch` mirror,
ImageFolderDataset, the LocalClient / SequentialFL wiring and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hefl.config import preset
from hefl.data import imageio
from hefl.data.files import (ImageFolderDataset, augment_params,
                             image_batch_reference)
from hefl.data.imageio import write_png, write_ppm
from hefl.data.shard import prep_df

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV255 = float(np.float32(1.0) / np.float32(255.0))


def rand_store(n, h, w, c, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8)


# ----------------------------------------------------- image_batch_reference

def test_reference_plain_is_exact_gather():
    store = rand_store(5, 6, 7, 3)
    idx = torch.tensor([4, 0, 4, 2])
    out = image_batch_reference(store, idx, 9, 6, 7)
    assert out.dtype == torch.float32 and out.shape == (4, 6, 7, 3)
    # the normative rescale is the fp32 product u * (1/255), which is what
    # the kernel computes; it is within one fp32 ulp of the quotient u / 255
    assert torch.equal(out, store[idx].float() * INV255)
    assert torch.allclose(out, store[idx].float() / 255.0, rtol=2e-7, atol=0)


def test_reference_flip_only_is_exact_mirror():
    n, seed = 8, 3
    _, _, sf = augment_params(seed, n, 0.0, 0.0, True)
    assert (sf < 0).any() and (sf > 0).any()  # both branches for this seed
    store = rand_store(n, 5, 6, 1, seed=1)
    out = image_batch_reference(store, torch.arange(n), seed, 5, 6,
                                0.0, 0.0, True)
    plain = store.float() * INV255
    for j in range(n):
        want = plain[j].flip(1) if sf[j] < 0 else plain[j]
        assert torch.equal(out[j], want), j


def test_reference_keys_on_position_not_stored_index():
    store = rand_store(4, 8, 8, 1, seed=2)
    same = torch.stack([store[1]] * 4)          # one image in every slot
    a = image_batch_reference(same, torch.tensor([0, 1, 2, 3]), 5, 8, 8,
                              0.2, 0.2, True)
    b = image_batch_reference(same, torch.tensor([3, 2, 1, 0]), 5, 8, 8,
                              0.2, 0.2, True)
    assert torch.equal(a, b)                    # stored index is irrelevant
    assert not torch.equal(a[0], a[1])          # the position is not
    c = image_batch_reference(same, torch.tensor([0, 1, 2, 3]), 6, 8, 8,
                              0.2, 0.2, True)
    assert not torch.equal(a, c)                # another seed, other params


def test_reference_stays_inside_the_source():
    # constant-255 images: any tap outside the source (a zero or garbage
    # read) or any weight pair not summing to 1 would leave [0, 1]
    store = torch.full((6, 9, 13, 3), 255, dtype=torch.uint8)
    out = image_batch_reference(store, torch.arange(6), 11, 8, 8,
                                0.2, 0.2, True)
    assert float(out.min()) >= 1.0 - 1e-6 and float(out.max()) <= 1.0 + 1e-6
    noise = image_batch_reference(rand_store(6, 9, 13, 3), torch.arange(6),
                                  11, 8, 8, 0.2, 0.2, True)
    assert float(noise.min()) >= 0.0 and float(noise.max()) <= 1.0


def test_reference_rejects_bad_index():
    with pytest.raises(IndexError):
        image_batch_reference(rand_store(3, 4, 4, 1), torch.tensor([3]), 0,
                              4, 4)


# ------------------------------------------------------- ImageFolderDataset

def make_mixed_tree(root, size=(6, 5)):
    """2 classes x 4 files, one per format; `a/2.pgm` is the lone gray file
    among RGB. Returns {path: uint8 HWC source array}."""
    rng = np.random.default_rng(5)
    h, w = size
    src = {}
    for cls in ("a", "b"):
        os.makedirs(os.path.join(root, cls))
        for i, ext in enumerate(("png", "ppm", "pgm" if cls == "a" else "bmp",
                                 "npy")):
            p = os.path.join(root, cls, f"{i}.{ext}")
            a = rng.integers(0, 256, (h, w, 1 if ext == "pgm" else 3),
                             dtype=np.uint8)
            if ext == "png":
                write_png(p, a)
            elif ext in ("ppm", "pgm"):
                write_ppm(p, a)
            elif ext == "npy":
                np.save(p, a)
            else:
                write_bmp24(p, a)
            src[p] = a
    return src


def write_bmp24(path, px):
    import struct
    h, w, _ = px.shape
    pad = (-3 * w) % 4
    body = b"".join(r.tobytes() + b"\0" * pad for r in px[::-1, :, ::-1])
    info = struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, len(body), 2835,
                       2835, 0, 0)
    with open(path, "wb") as f:
        f.write(b"BM" + struct.pack("<IHHI", 54 + len(body), 0, 0, 54) + info
                + body)


def luma(a):
    v = a.astype(np.uint32)
    return ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128)
            >> 8).astype(np.uint8)[..., None]


def test_folder_labels_and_channel_conversion(tmp_path):
    src = make_mixed_tree(str(tmp_path))
    for c in (3, 1):
        ds = ImageFolderDataset(str(tmp_path), (6, 5, c), seed=3)
        assert ds.class_to_idx == {"a": 0, "b": 1}
        assert ds.n_classes == 2 and ds.n_samples == 8 and ds.seed == 3
        assert ds.store.dtype == torch.uint8 and ds.store.shape == (8, 6, 5, c)
        assert ds.labels.dtype == torch.int64
        assert (ds.H, ds.W, ds.C) == (6, 5, c)
        for k, p in enumerate(ds.paths):
            cls = os.path.basename(os.path.dirname(p))
            assert int(ds.labels[k]) == ds.class_to_idx[cls]
            a = src[p]
            if a.shape[2] == 1 and c == 3:
                want = np.repeat(a, 3, axis=2)      # gray -> RGB
            elif a.shape[2] == 3 and c == 1:
                want = luma(a)                      # RGB -> gray
            else:
                want = a
            assert np.array_equal(ds.store[k].numpy(), want), p
        x, y = ds.batch(torch.tensor([7, 0, 3]))
        assert x.dtype == torch.float32 and x.shape == (3, 6, 5, c)
        assert torch.equal(x, ds.store[[7, 0, 3]].float() * INV255)
        assert torch.equal(y, ds.labels[[7, 0, 3]])


def test_folder_listing_is_shuffled_across_classes(tmp_path):
    make_mixed_tree(str(tmp_path))
    seed = 2  # (seed 3 happens to sort these 8 files by class: a shuffle of
    #           8 can; the assertion below is what pins a mixing seed)
    ds = ImageFolderDataset(str(tmp_path), (6, 5, 3), seed=seed)
    assert ds.paths == list(prep_df(str(tmp_path), shuffle=True,
                                    seed=seed)["Path"])
    # both halves (= the two clients' contiguous shards) hold both classes
    for half in (ds.labels[:4], ds.labels[4:]):
        assert set(half.tolist()) == {0, 1}


def test_folder_rows_decode_only_their_files(tmp_path, monkeypatch):
    make_mixed_tree(str(tmp_path))
    seen = []
    real = imageio.read_image

    def counting(path):
        seen.append(path)
        return real(path)

    monkeypatch.setattr(imageio, "read_image", counting)
    full = list(prep_df(str(tmp_path), shuffle=True, seed=3)["Path"])
    rows = torch.tensor([5, 1, 6])
    ds = ImageFolderDataset(str(tmp_path), (6, 5, 3), seed=3, rows=rows)
    assert seen == [full[5], full[1], full[6]] == ds.paths
    assert ds.n_samples == 3 and ds.n_classes == 2 and ds.n_listed == 8
    with pytest.raises(IndexError):
        ImageFolderDataset(str(tmp_path), (6, 5, 3), seed=3,
                           rows=torch.tensor([8]))


def test_folder_same_size_sources_keep_their_size(tmp_path):
    make_mixed_tree(str(tmp_path))
    ds = ImageFolderDataset(str(tmp_path), (4, 4, 3), seed=3)
    assert ds.store.shape == (8, 6, 5, 3)       # resized when sampled
    x, _ = ds.batch(torch.arange(8))
    assert x.shape == (8, 4, 4, 3)
    assert torch.equal(x, image_batch_reference(ds.store, torch.arange(8), 0,
                                                4, 4))


def test_folder_mixed_sizes_are_resized_at_load(tmp_path):
    make_mixed_tree(str(tmp_path))
    big = np.random.default_rng(1).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    extra = str(tmp_path / "b" / "big.png")
    write_png(extra, big)
    ds = ImageFolderDataset(str(tmp_path), (4, 4, 3), seed=3)
    assert ds.store.shape == (9, 4, 4, 3)
    k = ds.paths.index(extra)
    ref = image_batch_reference(torch.from_numpy(big)[None],
                                torch.tensor([0]), 0, 4, 4)[0]
    assert torch.equal(ds.store[k],
                       torch.floor(255.0 * ref + 0.5).to(torch.uint8))


def test_folder_bad_index_raises_before_any_work(tmp_path):
    make_mixed_tree(str(tmp_path))
    ds = ImageFolderDataset(str(tmp_path), (6, 5, 3), seed=3)
    for bad in ([8], [-1], [0, 9]):
        with pytest.raises(IndexError):
            ds.batch(torch.tensor(bad))


def test_folder_augmented_batches_advance_per_call(tmp_path):
    make_mixed_tree(str(tmp_path))
    ds1 = ImageFolderDataset(str(tmp_path), (6, 5, 3), seed=3)
    ds2 = ImageFolderDataset(str(tmp_path), (6, 5, 3), seed=3)
    idx = torch.arange(8)
    a1, _ = ds1.batch(idx, affine=(0.2, 0.2, True))
    a2, _ = ds2.batch(idx, affine=(0.2, 0.2, True))
    a3, _ = ds1.batch(idx, affine=(0.2, 0.2, True))
    assert torch.equal(a1, a2) and not torch.equal(a1, a3)


# ------------------------------------------- LocalClient / SequentialFL / CLI

def make_separable(root, n, seed):
    """n 28x28x1 PNGs, half `dark` (0..79) and half `bright` (150..229):
    no class overlap, and h-flip cannot turn one into the other."""
    rng = np.random.default_rng(seed)
    for k, name in enumerate(("dark", "bright")):
        os.makedirs(os.path.join(root, name))
        for i in range(n // 2):
            a = rng.integers(0, 80, (28, 28, 1)) + 150 * k
            write_png(os.path.join(root, name, f"{i:03d}.png"),
                      a.astype(np.uint8))


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    root = tmp_path_factory.mktemp("xray")
    make_separable(str(root / "train"), 80, 1)
    make_separable(str(root / "test"), 40, 2)
    return str(root / "train"), str(root / "test")


def folder_cfg(folders, encrypted=False):
    cfg = preset("config1")
    cfg.model.n_classes = 2
    cfg.fl.n_clients = 2
    cfg.fl.encrypted = encrypted
    cfg.fl.augment = "hflip"
    cfg.he.m = 256
    cfg.he.seed = 7
    cfg.fl.data_dir, cfg.fl.test_dir = folders
    return cfg


def test_config_defaults_keep_synthetic_data():
    cfg = preset("config2")
    assert cfg.fl.data_dir is None and cfg.fl.test_dir is None


def test_local_client_shards_and_val_split(folders):
    from hefl.fl.client import LocalClient
    cfg = folder_cfg(folders)
    listing = list(prep_df(folders[0], shuffle=True, seed=cfg.fl.seed)["Path"])
    held = []
    for cid in range(2):
        c = LocalClient(cfg, cid, device="cpu")
        assert isinstance(c.dataset, ImageFolderDataset)
        assert c.dataset.paths == listing[cid * 40:(cid + 1) * 40]
        # 720 : 80 configured -> the trailing 10% of the 40-file shard
        assert torch.equal(c.loader.indices, torch.arange(36))
        assert torch.equal(c.val_loader.indices, torch.arange(36, 40))
        assert set(c.dataset.labels.tolist()) == {0, 1}
        held += c.dataset.paths
    assert len(set(held)) == 80  # disjoint shards cover the folder
    cfg.fl.samples_per_client, cfg.fl.val_samples_per_client = 3, 1
    c = LocalClient(cfg, 0, device="cpu")
    assert c.loader.indices.numel() == 30 and c.val_loader.indices.numel() == 10


def test_class_count_mismatch_names_both_numbers(folders):
    from hefl.fl.client import LocalClient
    cfg = folder_cfg(folders)
    cfg.model.n_classes = 10
    with pytest.raises(ValueError) as e:
        LocalClient(cfg, 0, device="cpu")
    assert "2" in str(e.value) and "10" in str(e.value)


def test_sequential_without_test_dir_refuses(folders):
    from hefl.fl.sequential import SequentialFL
    cfg = folder_cfg(folders)
    cfg.fl.test_dir = None
    with pytest.raises(ValueError, match="test_dir"):
        SequentialFL(cfg, device="cpu")


def test_sequential_learns_the_folder_plain_and_encrypted(folders):
    """2 clients x 40 images (36 train / 4 val each), 40 held-out images.
    Observed on the fp32 CPU path: test accuracy is 0.5-0.6 after 5 local
    epochs for two of three seeds tried and 1.0 after 8 epochs for all
    three (fl.seed 1234, 1, 2), so the round runs 8 epochs; >= 0.9 leaves
    room for seed-to-seed variation on a task with no class overlap."""
    from hefl.fl.sequential import SequentialFL
    acc = {}
    for enc in (False, True):
        fl = SequentialFL(folder_cfg(folders, encrypted=enc), device="cpu")
        assert fl.test_ds.n_samples == 40
        rep = fl.run_round(epochs=8)
        acc[enc] = rep.metrics["accuracy"]
    assert acc[False] >= 0.9, acc
    assert acc[True] == acc[False], acc


def run_cli(*extra):
    return subprocess.run(
        [sys.executable, "-m", "hefl", "--preset", "config1", "--rounds", "1",
         "--epochs", "2", "--device", "cpu", "--json", *extra],
        cwd=REPO, capture_output=True, text=True, timeout=600)


def test_cli_runs_on_a_folder(folders):
    out = run_cli("--data-dir", folders[0], "--test-dir", folders[1])
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert {"accuracy", "precision", "recall", "f1"} <= set(d["metrics"])
    assert d["clients"] == 2 and d["rounds"] == 1


def test_cli_requires_test_dir(folders):
    out = run_cli("--data-dir", folders[0])
    assert out.returncode != 0
    assert "--test-dir" in out.stderr
