"""Dependency-free image decoding for the folder dataset.

The reference reads its image folders through Keras/Pillow
(`flow_from_dataframe`, FLPyfhelin.py:57-114). hefl must run where neither
ships, so the lossless formats medical-image folders are usually converted
to are decoded here with the standard library alone: PNG (stdlib `zlib`),
binary PGM/PPM, uncompressed BMP and `.npy`. Anything else (JPEG, ...) goes
through Pillow when it is importable and is refused otherwise.

`read_image` dispatches on the file's magic bytes, never on its extension,
and returns uint8 `[H, W, C]` with C in {1, 3}. Every decode failure is a
`ValueError` naming the file.
"""
from __future__ import annotations

import io
import struct
import zlib

import numpy as np

SUPPORTED = ("PNG (8-bit, non-interlaced)", "binary PGM/PPM (P5/P6)",
             "BMP (uncompressed 24-bit / 8-bit palette)", ".npy")

_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
_NPY_MAGIC = b"\x93NUMPY"
# PNG colour type -> samples per pixel
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def read_image(path: str) -> np.ndarray:
    """Decode `path` to a uint8 [H, W, C] array, C in {1, 3}."""
    path = str(path)
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError as e:
        raise ValueError(f"{path}: cannot read file: {e}") from e
    try:
        if data.startswith(_PNG_MAGIC):
            return _read_png(data, path)
        if data[:2] in (b"P5", b"P6"):
            return _read_pnm(data, path)
        if data[:2] == b"BM":
            return _read_bmp(data, path)
        if data.startswith(_NPY_MAGIC):
            return _read_npy(data, path)
    except ValueError:
        raise
    except (IndexError, struct.error, zlib.error, KeyError, TypeError) as e:
        raise ValueError(f"{path}: corrupt image file ({e})") from e
    return _read_pillow(data, path)


def _hwc(a: np.ndarray) -> np.ndarray:
    if a.ndim == 2:
        a = a[..., None]
    # a fresh, writable array: several decoders hand in read-only views of
    # the file's bytes
    return np.array(a, dtype=np.uint8, order="C")


# ----------------------------------------------------------------- PNG ----

def _png_chunks(data: bytes, path: str):
    pos = len(_PNG_MAGIC)
    while True:
        if pos + 8 > len(data):
            raise ValueError(f"{path}: truncated PNG (no IEND chunk)")
        length, ctype = struct.unpack(">I4s", data[pos:pos + 8])
        end = pos + 8 + length + 4
        if end > len(data):
            raise ValueError(
                f"{path}: truncated PNG ({ctype.decode('latin-1')} chunk "
                "runs past the end of the file)")
        body = data[pos + 8:pos + 8 + length]
        crc, = struct.unpack(">I", data[end - 4:end])
        if zlib.crc32(ctype + body) & 0xFFFFFFFF != crc:
            raise ValueError(
                f"{path}: bad CRC in PNG {ctype.decode('latin-1')} chunk")
        yield ctype, body
        if ctype == b"IEND":
            return
        pos = end


def _paeth_row(cur: np.ndarray, prev: np.ndarray, bpp: int) -> None:
    """In-place Paeth unfilter of one row (serial along the row)."""
    row = cur.tolist()
    up = prev.tolist()
    for i in range(len(row)):
        a = row[i - bpp] if i >= bpp else 0
        b = up[i]
        c = up[i - bpp] if i >= bpp else 0
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
        row[i] = (row[i] + pred) & 0xFF
    cur[:] = row


def _unfilter(raw: np.ndarray, h: int, stride: int, bpp: int,
              path: str) -> np.ndarray:
    """`raw` is uint8 [h, 1 + stride] (filter byte + filtered scanline)."""
    if not raw[:, 0].any():  # every row unfiltered (what write_png emits)
        return raw[:, 1:]
    out = np.zeros((h, stride), dtype=np.uint8)
    zero = np.zeros(stride, dtype=np.uint8)
    for y in range(h):
        ft = int(raw[y, 0])
        cur = raw[y, 1:].copy()
        prev = out[y - 1] if y else zero
        if ft == 0:
            pass
        elif ft == 2:  # Up: whole-row add
            cur += prev
        elif ft == 1:
            # Sub: recon[i] = filt[i] + recon[i-bpp] is a running sum (mod
            # 256) along each of the bpp interleaved byte lanes
            n = (stride + bpp - 1) // bpp
            lanes = np.zeros(n * bpp, dtype=np.uint8)
            lanes[:stride] = cur
            cur = np.cumsum(lanes.reshape(n, bpp), axis=0,
                            dtype=np.uint8).reshape(-1)[:stride]
        elif ft == 3:  # Average: serial along the row, bpp bytes at a time
            p16 = prev.astype(np.uint16)
            c16 = cur.astype(np.uint16)
            for i in range(0, stride, bpp):
                j = min(i + bpp, stride)
                left = c16[i - bpp:i][:j - i] if i else 0
                c16[i:j] = (c16[i:j] + ((left + p16[i:j]) >> 1)) & 0xFF
            cur = c16.astype(np.uint8)
        elif ft == 4:
            _paeth_row(cur, prev, bpp)
        else:
            raise ValueError(f"{path}: unknown PNG filter type {ft} "
                             f"on row {y}")
        out[y] = cur
    return out


def _read_png(data: bytes, path: str) -> np.ndarray:
    ihdr = None
    palette = None
    idat = []
    for ctype, body in _png_chunks(data, path):
        if ctype == b"IHDR":
            if len(body) != 13:
                raise ValueError(f"{path}: malformed PNG IHDR chunk")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif ctype == b"PLTE":
            if len(body) % 3:
                raise ValueError(f"{path}: malformed PNG PLTE chunk")
            palette = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3)
        elif ctype == b"IDAT":
            idat.append(body)
    if ihdr is None:
        raise ValueError(f"{path}: PNG without an IHDR chunk")
    w, h, depth, ctype, comp, flt, interlace = ihdr
    if interlace != 0:
        raise ValueError(f"{path}: interlaced PNG is not supported")
    if depth != 8:
        raise ValueError(f"{path}: PNG bit depth {depth} is not supported "
                         "(8-bit only)")
    if ctype not in _PNG_CHANNELS or comp != 0 or flt != 0:
        raise ValueError(f"{path}: unsupported PNG colour type {ctype} / "
                         f"compression {comp} / filter method {flt}")
    if w == 0 or h == 0 or not idat:
        raise ValueError(f"{path}: PNG without image data")
    ch = _PNG_CHANNELS[ctype]
    stride = w * ch
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError(f"{path}: corrupt PNG image data ({e})") from e
    if len(raw) < h * (stride + 1):
        raise ValueError(f"{path}: truncated PNG image data ({len(raw)} of "
                         f"{h * (stride + 1)} bytes)")
    raw = np.frombuffer(raw, dtype=np.uint8,
                        count=h * (stride + 1)).reshape(h, stride + 1)
    px = _unfilter(raw, h, stride, ch, path).reshape(h, w, ch)
    if ctype == 3:
        if palette is None:
            raise ValueError(f"{path}: palette PNG without a PLTE chunk")
        if int(px.max()) >= len(palette):
            raise ValueError(f"{path}: PNG palette index out of range")
        return _hwc(palette[px[..., 0]])
    if ctype in (4, 6):  # drop alpha
        px = px[..., :ch - 1]
    return _hwc(px)


def _png_chunk(ctype: bytes, body: bytes) -> bytes:
    return (struct.pack(">I", len(body)) + ctype + body
            + struct.pack(">I", zlib.crc32(ctype + body) & 0xFFFFFFFF))


def _as_u8_hwc(arr, what: str) -> np.ndarray:
    a = np.asarray(arr)
    if a.ndim == 2:
        a = a[..., None]
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"{what} needs a uint8 [H, W] or [H, W, 1|3] array, "
                         f"got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def write_png(path: str, arr) -> None:
    """Write uint8 [H, W, 1|3] as an 8-bit PNG (filter 0, one IDAT)."""
    a = _as_u8_hwc(arr, "write_png")
    h, w, c = a.shape
    rows = np.zeros((h, 1 + w * c), dtype=np.uint8)
    rows[:, 1:] = a.reshape(h, w * c)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 0 if c == 1 else 2, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _png_chunk(b"IHDR", ihdr)
                + _png_chunk(b"IDAT", zlib.compress(rows.tobytes()))
                + _png_chunk(b"IEND", b""))


# ------------------------------------------------------------- PGM/PPM ----

def _read_pnm(data: bytes, path: str) -> np.ndarray:
    ch = 1 if data[:2] == b"P5" else 3
    pos = 2
    vals = []
    while len(vals) < 3:
        # skip whitespace and '#' comments between header tokens
        while True:
            if pos >= len(data):
                raise ValueError(f"{path}: truncated PNM header")
            b = data[pos:pos + 1]
            if b == b"#":
                while pos < len(data) and data[pos:pos + 1] not in b"\r\n":
                    pos += 1
            elif b.isspace():
                pos += 1
            else:
                break
        start = pos
        while pos < len(data) and data[pos:pos + 1].isdigit():
            pos += 1
        if pos == start:
            raise ValueError(f"{path}: malformed PNM header")
        vals.append(int(data[start:pos]))
    w, h, maxval = vals
    if not (0 < maxval <= 255):
        raise ValueError(f"{path}: PNM maxval {maxval} is not supported "
                         "(<= 255 only)")
    pos += 1  # the single whitespace byte that ends the header
    need = w * h * ch
    if w <= 0 or h <= 0 or len(data) - pos < need:
        raise ValueError(f"{path}: truncated PNM pixel data")
    a = np.frombuffer(data, dtype=np.uint8, count=need, offset=pos)
    return _hwc(a.reshape(h, w, ch))


def write_ppm(path: str, arr) -> None:
    """Write uint8 [H, W, 3] as binary PPM (P6), [H, W, 1] as PGM (P5)."""
    a = _as_u8_hwc(arr, "write_ppm")
    h, w, c = a.shape
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P5" if c == 1 else b"P6", w, h))
        f.write(a.tobytes())


# ----------------------------------------------------------------- BMP ----

def _read_bmp(data: bytes, path: str) -> np.ndarray:
    if len(data) < 54:
        raise ValueError(f"{path}: truncated BMP header")
    off, = struct.unpack("<I", data[10:14])
    hdr, w, h, planes, bpp, comp = struct.unpack("<IiiHHI", data[14:34])
    ncol, = struct.unpack("<I", data[46:50])
    if hdr < 40 or comp != 0 or bpp not in (8, 24):
        raise ValueError(f"{path}: unsupported BMP (header {hdr}, {bpp} bpp, "
                         f"compression {comp}); uncompressed 24-bit and 8-bit "
                         "palettised only")
    top_down = h < 0
    h = abs(h)
    if w <= 0 or h == 0:
        raise ValueError(f"{path}: bad BMP dimensions {w}x{h}")
    row = (w * bpp // 8 + 3) & ~3  # rows are padded to 4 bytes
    if off + row * h > len(data):
        raise ValueError(f"{path}: truncated BMP pixel data")
    px = np.frombuffer(data, dtype=np.uint8, count=row * h,
                       offset=off).reshape(h, row)
    if not top_down:
        px = px[::-1]
    if bpp == 24:
        return _hwc(px[:, :w * 3].reshape(h, w, 3)[..., ::-1])  # BGR -> RGB
    ncol = ncol or 256
    if 14 + hdr + 4 * ncol > len(data):
        raise ValueError(f"{path}: truncated BMP palette")
    pal = np.frombuffer(data, dtype=np.uint8, count=4 * ncol,
                        offset=14 + hdr).reshape(ncol, 4)[:, 2::-1]
    ind = px[:, :w]
    if int(ind.max()) >= ncol:
        raise ValueError(f"{path}: BMP palette index out of range")
    return _hwc(pal[ind])


# ----------------------------------------------------------------- npy ----

def _read_npy(data: bytes, path: str) -> np.ndarray:
    try:
        a = np.load(io.BytesIO(data), allow_pickle=False)
    except Exception as e:  # np.load raises several unrelated types
        raise ValueError(f"{path}: corrupt .npy file ({e})") from e
    if a.ndim == 2:
        a = a[..., None]
    if a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"{path}: .npy image must be [H, W] or "
                         f"[H, W, 1|3], got shape {a.shape}")
    if a.dtype == np.uint8:
        return _hwc(a)
    if a.dtype.kind == "f":
        if a.size and (float(a.min()) < 0.0 or float(a.max()) > 1.0):
            raise ValueError(f"{path}: float .npy image outside [0, 1]")
        return _hwc(np.floor(255.0 * a.astype(np.float64) + 0.5))
    raise ValueError(f"{path}: .npy image dtype {a.dtype} is not supported "
                     "(uint8 or float in [0, 1])")


# -------------------------------------------------------------- Pillow ----

def _read_pillow(data: bytes, path: str) -> np.ndarray:
    try:
        from PIL import Image
    except ImportError:
        raise ValueError(
            f"{path}: unrecognised image format; supported without Pillow: "
            + ", ".join(SUPPORTED)) from None
    try:
        with Image.open(io.BytesIO(data)) as im:
            im = im.convert("L" if im.mode in ("1", "L", "I;16", "I") else "RGB")
            return _hwc(np.asarray(im))
    except Exception as e:
        raise ValueError(
            f"{path}: Pillow could not decode the file ({e}); supported "
            "without Pillow: " + ", ".join(SUPPORTED)) from e
