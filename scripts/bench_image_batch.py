"""image_batch microbench + folder-vs-synthetic LocalClient throughput.

Kernel part, at the reference shape (720 x 256x256x3) and the config #2
shape (720 x 28x28x1): `image_batch` on the fast path (gather + convert),
`image_batch` with full augmentation, and the composed torch path it
replaces (fp32 cache index_select + device grid_sample + bf16 cast, with
the sampling grid prebuilt on the device — which favours torch). Each is
warmed up, then timed REPS times over ITERS back-to-back launches;
median / min / max of the per-launch time and GB/s against the traffic
model (1 B read + 2 B written per element; 4 B read for the fp32 cache).

End-to-end part (`--e2e PRESET`, default both shapes' presets): one
LocalClient epoch through the whole-epoch graph, samples/s with a generated
image folder next to the synthetic dataset on the same preset.

    python scripts/bench_image_batch.py [--skip-e2e] [--e2e reference config2]
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import statistics
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

import hefl
from hefl.config import preset
from hefl.data.imageio import write_png
from hefl.fl.client import LocalClient

C = hefl.load_extension()
REPS, ITERS = 7, 20


def bench(fn, iters=ITERS, reps=REPS):
    """[us per call] x reps, after a warm-up."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000 / iters)
    return out


def show(name, ts, nbytes):
    med = statistics.median(ts)
    print(f"  {name:28s} {med:9.1f} us (min {min(ts):.1f}, max {max(ts):.1f})"
          f"  {nbytes / med / 1e3:7.0f} GB/s")


def kernel_part():
    for tag, n, H, W, Cc in (("reference 720x256x256x3", 720, 256, 256, 3),
                             ("config2   720x28x28x1", 720, 28, 28, 1)):
        print(tag)
        N = n + 80
        store = torch.randint(0, 256, (N, H, W, Cc), dtype=torch.uint8,
                              device="cuda")
        idx = torch.randperm(N, device="cuda")[:n].contiguous()
        elems = n * H * W * Cc
        show("image_batch fast path",
             bench(lambda: C.image_batch(store, idx, 1, H, W)), elems * 3)
        show("image_batch full augment",
             bench(lambda: C.image_batch(store, idx, 1, H, W, zoom=0.2,
                                         shear=0.2, flip=1)), elems * 3)
        cache = store.float().div_(255.0)  # the fp32 cache it replaces
        theta = torch.eye(2, 3, device="cuda").repeat(n, 1, 1)
        theta[:, 0, 0] += 0.1
        theta[:, 0, 1] += 0.1
        grid = F.affine_grid(theta, (n, Cc, H, W), align_corners=True)

        def composed():
            x = cache.index_select(0, idx)
            x = F.grid_sample(x.permute(0, 3, 1, 2), grid, mode="bilinear",
                              padding_mode="border", align_corners=True)
            return x.permute(0, 2, 3, 1).to(torch.bfloat16)

        show("torch select+grid_sample+cast", bench(composed, iters=5),
             elems * 6)
        show("torch select+cast (no aug)",
             bench(lambda: cache.index_select(0, idx).to(torch.bfloat16),
                   iters=5), elems * 6)
        del cache, grid, theta, store
        torch.cuda.empty_cache()


def make_folder(root, n, shape, n_classes, seed):
    rng = np.random.default_rng(seed)
    for k in range(n_classes):
        os.makedirs(os.path.join(root, f"c{k}"))
    for i in range(n):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        write_png(os.path.join(root, f"c{i % n_classes}", f"{i:05d}.png"), a)


def client_rate(cfg, epochs=3, reps=5):
    c = LocalClient(cfg, 0, device="cuda")
    c.local_train(epochs=1)  # builds + warms the epoch graph
    rates = []
    for _ in range(reps):
        s = c.local_train(epochs=epochs)
        rates.append(s.samples / s.seconds)
    return rates, c._ep_ent["in_graph_data"]


def e2e_part(names):
    for name in names:
        cfg = preset(name)
        cfg.fl.n_clients = 1
        r_syn, _ = client_rate(cfg)
        with tempfile.TemporaryDirectory() as d:
            per = cfg.fl.samples_per_client + cfg.fl.val_samples_per_client
            make_folder(d, per, cfg.model.in_shape, cfg.model.n_classes, 0)
            cfg.fl.data_dir = d
            r_dir, in_graph = client_rate(cfg)
        assert in_graph
        for tag, r in (("synthetic", r_syn), ("folder", r_dir)):
            print(f"{name:10s} {tag:10s} {statistics.median(r):9.0f} samples/s"
                  f" (min {min(r):.0f}, max {max(r):.0f}; {len(r)} runs of 3"
                  " epochs)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--e2e", nargs="*", default=["config2", "reference"])
    a = ap.parse_args()
    kernel_part()
    if not a.skip_e2e:
        e2e_part(a.e2e)
