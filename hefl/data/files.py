"""File-backed datasets over the reference's `folder/<class>/*` layout.

The reference trains on image folders through Keras ImageDataGenerator
(`flow_from_dataframe` over prep_df's (Path, Label) frame,
FLPyfhelin.py:38-55,57-114). The north-star benchmarks use synthetic data
(no network for datasets), but a migrating user with real data gets the
same folder/<class> layout here. `ImageFolderDataset` decodes PNG / PGM /
PPM / BMP / .npy files with the standard library (hefl/data/imageio.py;
other formats through Pillow when it is installed), keeps them as a uint8
store on the device and stages batches with the `image_batch` HIP kernel,
so real images run through the same whole-epoch graph as the synthetic
benchmark. `FileImageDataset` is the older fp32 `.npy`-only cache. Both
present the same `batch(indices, affine=...)` surface as
SyntheticMedicalImages, so ClientLoader / get_train_data / get_test_data
work unchanged.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import imageio
from .shard import prep_df
from .synthetic import affine_sample


class FileImageDataset:
    """Images from `folder/<class>/*.npy` (HWC float or uint8 arrays).

    uint8 arrays are rescaled by 1/255 like the reference's
    ImageDataGenerator(rescale=1./255) (FLPyfhelin.py:59); float arrays are
    taken as-is. The whole set is materialized once (`cache=True`, default)
    — medical-image folders at the reference's scale (~1200 images of
    256x256x3) are ~300 MB, trivial beside 288 GB of HBM.
    """

    def __init__(self, folder: str, device: str = "cpu",
                 dtype: torch.dtype = torch.float32, cache: bool = True,
                 seed: int = 0):
        self.df = prep_df(folder, shuffle=False)
        if len(self.df) == 0:
            raise ValueError(f"no files under {folder}/<class>/")
        self.classes = sorted(self.df["Label"].unique())
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.n_classes = len(self.classes)
        self.n_samples = len(self.df)
        self.device = torch.device(device)
        self.dtype = dtype
        self.seed = int(seed)
        self.labels = torch.tensor(
            [self.class_to_idx[l] for l in self.df["Label"]],
            dtype=torch.int64, device=self.device)
        self._paths = list(self.df["Path"])
        self._cache: Optional[torch.Tensor] = None
        if cache:
            imgs = [self._load(p) for p in self._paths]
            shapes = {tuple(i.shape) for i in imgs}
            if len(shapes) != 1:
                raise ValueError(f"mixed image shapes in {folder}: {shapes}")
            self._cache = torch.stack(imgs).to(self.device)
        h, w, c = (self._cache.shape[1:] if self._cache is not None
                   else self._load(self._paths[0]).shape)
        self.H, self.W, self.C = int(h), int(w), int(c)

    @staticmethod
    def _load(path: str) -> torch.Tensor:
        a = np.load(path, allow_pickle=False)
        if a.ndim == 2:
            a = a[..., None]
        if a.dtype == np.uint8:
            a = a.astype(np.float32) / 255.0  # reference rescale=1/255
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))

    def batch(self, indices: torch.Tensor,
              affine=None) -> Tuple[torch.Tensor, torch.Tensor]:
        idx = indices.to(self.device)
        y = self.labels[idx]
        if self._cache is not None:
            x = self._cache.index_select(0, idx)
        else:
            x = torch.stack([self._load(self._paths[int(i)])
                             for i in indices]).to(self.device)
        if affine is not None and (affine[0] or affine[1] or affine[2]):
            zr, sr, fl = affine
            self._aug_ctr = getattr(self, "_aug_ctr", 0) + 1
            g = torch.Generator(device="cpu").manual_seed(
                self.seed * 31 + self._aug_ctr)
            x = affine_sample(x, zr, sr, fl, g)
        return x.to(self.dtype), y


# ---------------------------------------------------------------------------
# uint8 image store + one-pass resize/augment staging (`image_batch`)
# ---------------------------------------------------------------------------

_M64 = (1 << 64) - 1
_U32_TO_UNIT = np.float32(2.3283064e-10)  # 2**-32, as the kernels spell it


def _splitmix64(z: int) -> int:
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def augment_params(seed: int, n: int, zr: float, sr: float, fl):
    """Per-sample (zoom, shear, sf) float32 arrays for output positions
    0..n-1 — the hash chain of synth_batch_kernel<true> / image_batch_kernel
    (cnn.hip), so both device generators and this mirror augment alike."""
    f32 = np.float32
    zoom = np.empty(n, dtype=f32)
    shear = np.empty(n, dtype=f32)
    sf = np.empty(n, dtype=f32)
    for j in range(n):
        pz = _splitmix64((int(seed) & _M64) ^ ((0xA5A5A5A5 + j) & _M64))
        uz = f32(pz & 0xFFFFFFFF) * _U32_TO_UNIT
        us = f32(pz >> 32) * _U32_TO_UNIT
        uf = f32(_splitmix64(pz) & 0xFFFFFFFF) * _U32_TO_UNIT
        zoom[j] = f32(1) + f32(zr) * (f32(2) * uz - f32(1))
        shear[j] = f32(sr) * (f32(2) * us - f32(1))
        sf[j] = f32(-1) if (fl and uf < f32(0.5)) else f32(1)
    return zoom, shear, sf


def image_batch_reference(store: torch.Tensor, idx: torch.Tensor, seed: int,
                          H: int, W: int, zr: float = 0.0, sr: float = 0.0,
                          fl=False) -> torch.Tensor:
    """CPU mirror of the `image_batch` kernel: float32 [n, H, W, C].

    Gathers `store[idx]` (uint8 [N,Hs,Ws,C]), and for output sample j (its
    POSITION in idx) and pixel (h, w) of the HxW target grid samples the
    source bilinearly, border-clamped, at the inverse-mapped point

        ty = cy + (h - cy) / zoom
        tx = cx + (w - cx) * sf / zoom + shear * (h - cy)
        sy = ty * (Hs-1)/(H-1),  sx = tx * (Ws-1)/(W-1)    (ratio 0 if H|W=1)

    then rescales by 1/255 — resize and augmentation in ONE sampling pass.
    The oracle for the kernel and the CPU path of ImageFolderDataset."""
    store = torch.as_tensor(store).cpu()
    idx = torch.as_tensor(idx).cpu().to(torch.int64).reshape(-1)
    if store.dtype != torch.uint8 or store.dim() != 4:
        raise ValueError("store must be uint8 [N, Hs, Ws, C]")
    N, Hs, Ws, C = store.shape
    n = idx.numel()
    if n and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise IndexError(f"sample index outside [0, {N})")
    H, W = int(H), int(W)
    src = store.index_select(0, idx).to(torch.float32)
    zoom, shear, sf = (torch.from_numpy(a).view(n, 1, 1)
                       for a in augment_params(seed, n, zr, sr, fl))
    f32 = np.float32
    cy, cx = float(f32(0.5) * f32(H - 1)), float(f32(0.5) * f32(W - 1))
    ry = float(f32(Hs - 1) / f32(H - 1)) if H > 1 else 0.0
    rx = float(f32(Ws - 1) / f32(W - 1)) if W > 1 else 0.0
    dy = (torch.arange(H, dtype=torch.float32) - cy).view(1, H, 1)
    dx = (torch.arange(W, dtype=torch.float32) - cx).view(1, 1, W)
    ty = cy + dy / zoom                          # [n, H, 1]
    tx = cx + dx * sf / zoom + shear * dy        # [n, H, W]
    sy = (ty * ry).clamp(0.0, float(Hs - 1))
    sx = (tx * rx).clamp(0.0, float(Ws - 1))
    y0, x0 = sy.floor().long(), sx.floor().long()
    y1, x1 = (y0 + 1).clamp(max=Hs - 1), (x0 + 1).clamp(max=Ws - 1)
    fy, fx = (sy - y0).unsqueeze(-1), (sx - x0).unsqueeze(-1)
    b = torch.arange(n).view(n, 1, 1)
    t00, t01 = src[b, y0, x0], src[b, y0, x1]    # [n, H, W, C]
    t10, t11 = src[b, y1, x0], src[b, y1, x1]
    t = ((t00 * (1 - fx) + t01 * fx) * (1 - fy)
         + (t10 * (1 - fx) + t11 * fx) * fy)
    return t * float(f32(1.0) / f32(255.0))


def _to_channels(a: np.ndarray, c: int, path: str) -> np.ndarray:
    """uint8 [H,W,1|3] -> [H,W,c]: gray -> RGB by replication, RGB -> gray
    by the integer luma (77R + 150G + 29B + 128) >> 8."""
    if a.shape[2] == c:
        return a
    if a.shape[2] == 1 and c == 3:
        return np.repeat(a, 3, axis=2)
    if a.shape[2] == 3 and c == 1:
        v = a.astype(np.uint32)
        g = (77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8
        return g.astype(np.uint8)[..., None]
    raise ValueError(f"{path}: cannot convert {a.shape[2]} channels to {c}")


class ImageFolderDataset:
    """Images from `folder/<class>/*` as a device-resident uint8 store.

    The listing is `prep_df(folder, shuffle=True, seed=seed)` — shuffled,
    because shard_indices cuts CONTIGUOUS shards and the unshuffled listing
    is sorted by class. `rows` (indices into that listing) restricts
    decoding to those files: a federated client decodes and holds only its
    own shard. Sample indices passed to `batch` are positions in the loaded
    set, 0..n_samples-1.

    Sources that all share one size are stored at that size and resized to
    `in_shape` by the sampling kernel, in the same pass as the augmentation;
    mixed sizes are resized to `in_shape` at load. uint8 keeps the store at
    the bytes of the source pixels (the reference's 800 x 256x256x3 shard:
    157 MB instead of 629 MB fp32).
    """

    def __init__(self, folder: str, in_shape: Tuple[int, int, int],
                 device: str = "cpu", dtype: torch.dtype = torch.float32,
                 seed: int = 0, rows: Optional[torch.Tensor] = None):
        self.H, self.W, self.C = (int(v) for v in in_shape)
        if self.C not in (1, 3):
            raise ValueError(f"in_shape channels must be 1 or 3, got {self.C}")
        self.device = torch.device(device)
        self.dtype = dtype
        self.seed = int(seed)
        df = prep_df(folder, shuffle=True, seed=self.seed)
        if len(df) == 0:
            raise ValueError(f"no files under {folder}/<class>/")
        self.classes = sorted(df["Label"].unique())
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.n_classes = len(self.classes)
        self.n_listed = len(df)
        paths, labels = list(df["Path"]), list(df["Label"])
        if rows is not None:
            rows = [int(r) for r in torch.as_tensor(rows).reshape(-1)]
            if rows and (min(rows) < 0 or max(rows) >= len(paths)):
                raise IndexError(f"rows outside the {len(paths)}-file listing "
                                 f"of {folder}")
            paths = [paths[r] for r in rows]
            labels = [labels[r] for r in rows]
        if not paths:
            raise ValueError(f"no files selected from {folder}")
        self.paths = paths
        imgs = [_to_channels(imageio.read_image(p), self.C, p) for p in paths]
        if len({im.shape for im in imgs}) != 1:
            # mixed source sizes: one common size is needed for the store
            imgs = [self._resize(im) for im in imgs]
        self.store = torch.from_numpy(np.stack(imgs)).to(self.device)
        self.labels = torch.tensor([self.class_to_idx[l] for l in labels],
                                   dtype=torch.int64, device=self.device)
        self.n_samples = len(paths)
        self._ctr = 0

    def _resize(self, im: np.ndarray) -> np.ndarray:
        x = image_batch_reference(torch.from_numpy(im)[None],
                                  torch.zeros(1, dtype=torch.int64), 0,
                                  self.H, self.W)
        return torch.floor(255.0 * x[0] + 0.5).to(torch.uint8).numpy()

    def _on_kernel(self) -> bool:
        return self.device.type == "cuda" and self.dtype == torch.bfloat16

    def batch(self, indices: torch.Tensor,
              affine=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(x[NHWC], y[N]) for the given sample indices; `affine` =
        (zoom_range, shear_range, hflip) as in SyntheticMedicalImages."""
        if indices.numel() and (int(indices.min()) < 0
                                or int(indices.max()) >= self.n_samples):
            raise IndexError(
                f"sample index outside [0, {self.n_samples})")
        idx = indices.to(self.device, torch.int64).contiguous()
        y = self.labels[idx]
        zr, sr, fl = affine if affine else (0.0, 0.0, False)
        self._ctr += 1
        seed = self.seed * 0x10001 + self._ctr  # per-call counter seed
        if self._on_kernel():
            import hefl
            x = hefl.load_extension().image_batch(
                self.store, idx, seed, self.H, self.W, zoom=zr, shear=sr,
                flip=int(bool(fl)))
            return x, y
        x = image_batch_reference(self.store, idx, seed, self.H, self.W,
                                  zr, sr, fl)
        return x.to(self.device, self.dtype), y

    def graph_batch(self, order_buf: torch.Tensor, seed_buf: torch.Tensor,
                    affine=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Capturable staging of one epoch: (X, Y) for the sample order in
        `order_buf` (device int64), augmentation seeded from `seed_buf`
        (device int64[1]); the host rewrites both before each replay."""
        import hefl
        zr, sr, fl = affine if affine else (0.0, 0.0, False)
        Y = self.labels.index_select(0, order_buf)
        X = hefl.load_extension().image_batch_g(
            self.store, order_buf, seed_buf, 0, self.H, self.W, zoom=zr,
            shear=sr, flip=int(bool(fl)))
        return X, Y
