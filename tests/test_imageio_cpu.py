"""hefl.data.imageio: the stdlib-only decoders against files built by hand.

Every PNG/BMP here is assembled in the test from struct/zlib, so each
scanline filter, chunk layout and row order is covered without Pillow; the
Pillow cross-check at the end is an extra that runs where Pillow exists.
"""
import struct
import zlib

import numpy as np
import pytest

from hefl.data.imageio import read_image, write_png, write_ppm

RNG = np.random.default_rng(20240611)
RGB = RNG.integers(0, 256, (4, 5, 3), dtype=np.uint8)  # 5 wide x 4 high


def _chunk(ctype, body):
    return (struct.pack(">I", len(body)) + ctype + body
            + struct.pack(">I", zlib.crc32(ctype + body) & 0xFFFFFFFF))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def _filter_row(ft, cur, prev, bpp):
    """PNG-filter one scanline (lists of ints) — the encoder side, written
    from the PNG specification's definitions."""
    out = []
    for i, x in enumerate(cur):
        a = cur[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        pred = (0, a, b, (a + b) // 2, _paeth(a, b, c))[ft]
        out.append((x - pred) & 0xFF)
    return out


def _png_bytes(px, colour_type, filters, n_idat=1, depth=8, interlace=0,
               palette=None):
    """px: uint8 [H, W, samples]; filters: one filter type per row."""
    h, w, ch = px.shape
    raw = bytearray()
    prev = [0] * (w * ch)
    for y in range(h):
        cur = px[y].reshape(-1).tolist()
        raw.append(filters[y])
        raw.extend(_filter_row(filters[y], cur, prev, ch))
        prev = cur
    z = zlib.compress(bytes(raw))
    cuts = [len(z) * k // n_idat for k in range(n_idat + 1)]
    out = b"\x89PNG\r\n\x1a\n" + _chunk(
        b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, 0, 0,
                             interlace))
    if palette is not None:
        out += _chunk(b"PLTE", palette.tobytes())
    for k in range(n_idat):
        out += _chunk(b"IDAT", z[cuts[k]:cuts[k + 1]])
    return out + _chunk(b"IEND", b"")


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4])
def test_png_each_filter_on_every_row(tmp_path, ft):
    p = _write(tmp_path, f"f{ft}.png", _png_bytes(RGB, 2, [ft] * 4))
    got = read_image(p)
    assert got.dtype == np.uint8 and got.shape == (4, 5, 3)
    assert np.array_equal(got, RGB)


def test_png_mixed_filters(tmp_path):
    p = _write(tmp_path, "mixed.png", _png_bytes(RGB, 2, [4, 1, 3, 2]))
    assert np.array_equal(read_image(p), RGB)


def test_png_idat_split_in_three(tmp_path):
    p = _write(tmp_path, "split.png",
               _png_bytes(RGB, 2, [1, 4, 0, 3], n_idat=3))
    assert np.array_equal(read_image(p), RGB)


def test_png_gray_palette_and_alpha_variants(tmp_path):
    gray = RNG.integers(0, 256, (4, 5, 1), dtype=np.uint8)
    got = read_image(_write(tmp_path, "g.png",
                            _png_bytes(gray, 0, [3, 4, 1, 2])))
    assert got.shape == (4, 5, 1) and np.array_equal(got, gray)

    pal = RNG.integers(0, 256, (7, 3), dtype=np.uint8)
    ind = RNG.integers(0, 7, (4, 5, 1), dtype=np.uint8)
    got = read_image(_write(tmp_path, "p.png",
                            _png_bytes(ind, 3, [0, 1, 2, 4], palette=pal)))
    assert got.shape == (4, 5, 3) and np.array_equal(got, pal[ind[..., 0]])

    ga = RNG.integers(0, 256, (4, 5, 2), dtype=np.uint8)
    got = read_image(_write(tmp_path, "ga.png",
                            _png_bytes(ga, 4, [4, 3, 1, 2])))
    assert got.shape == (4, 5, 1) and np.array_equal(got, ga[..., :1])

    rgba = RNG.integers(0, 256, (4, 5, 4), dtype=np.uint8)
    got = read_image(_write(tmp_path, "rgba.png",
                            _png_bytes(rgba, 6, [2, 4, 3, 1])))
    assert got.shape == (4, 5, 3) and np.array_equal(got, rgba[..., :3])


def test_dispatch_is_by_magic_not_extension(tmp_path):
    p = _write(tmp_path, "really_a_png.bmp", _png_bytes(RGB, 2, [0] * 4))
    assert np.array_equal(read_image(p), RGB)


@pytest.mark.parametrize("shape", [(7, 3, 3), (6, 5, 1)])
def test_write_png_round_trip(tmp_path, shape):
    a = RNG.integers(0, 256, shape, dtype=np.uint8)
    p = str(tmp_path / "rt.png")
    write_png(p, a)
    assert np.array_equal(read_image(p), a)


def test_write_ppm_round_trip_and_header_comment(tmp_path):
    a3 = RNG.integers(0, 256, (7, 3, 3), dtype=np.uint8)
    a1 = RNG.integers(0, 256, (6, 5, 1), dtype=np.uint8)
    p3, p1 = str(tmp_path / "a.ppm"), str(tmp_path / "a.pgm")
    write_ppm(p3, a3)
    write_ppm(p1, a1)
    assert open(p3, "rb").read(2) == b"P6" and open(p1, "rb").read(2) == b"P5"
    assert np.array_equal(read_image(p3), a3)
    assert np.array_equal(read_image(p1), a1)
    pc = _write(tmp_path, "c.pgm",
                b"P5\n# made by hand\n5 6\n# another\n255\n" + a1.tobytes())
    assert np.array_equal(read_image(pc), a1)


def _bmp24(px, top_down):
    h, w, _ = px.shape
    pad = (-3 * w) % 4
    rows = px[..., ::-1]  # RGB -> BGR
    if not top_down:
        rows = rows[::-1]
    body = b"".join(r.tobytes() + b"\0" * pad for r in rows)
    info = struct.pack("<IiiHHIIiiII", 40, w, -h if top_down else h, 1, 24, 0,
                       len(body), 2835, 2835, 0, 0)
    return (b"BM" + struct.pack("<IHHI", 54 + len(body), 0, 0, 54) + info
            + body)


def test_bmp_24bit_both_row_orders(tmp_path):
    px = RNG.integers(0, 256, (3, 5, 3), dtype=np.uint8)  # 15 B rows + 1 pad
    assert (-3 * 5) % 4 == 1
    up = read_image(_write(tmp_path, "up.bmp", _bmp24(px, False)))
    down = read_image(_write(tmp_path, "down.bmp", _bmp24(px, True)))
    assert up.shape == (3, 5, 3)
    assert np.array_equal(up, px) and np.array_equal(down, px)


def test_bmp_8bit_palette(tmp_path):
    h, w, ncol = 3, 5, 6
    pal = RNG.integers(0, 256, (ncol, 3), dtype=np.uint8)
    ind = RNG.integers(0, ncol, (h, w), dtype=np.uint8)
    pad = (-w) % 4
    body = b"".join(r.tobytes() + b"\0" * pad for r in ind[::-1])
    table = b"".join(bytes([c[2], c[1], c[0], 0]) for c in pal.tolist())
    off = 54 + len(table)
    info = struct.pack("<IiiHHIIiiII", 40, w, h, 1, 8, 0, len(body), 2835,
                       2835, ncol, 0)
    data = (b"BM" + struct.pack("<IHHI", off + len(body), 0, 0, off) + info
            + table + body)
    got = read_image(_write(tmp_path, "pal.bmp", data))
    assert got.shape == (h, w, 3) and np.array_equal(got, pal[ind])


def test_npy_uint8_and_float(tmp_path):
    a = RNG.integers(0, 256, (4, 6, 3), dtype=np.uint8)
    np.save(tmp_path / "u.npy", a)
    assert np.array_equal(read_image(str(tmp_path / "u.npy")), a)
    g = RNG.integers(0, 256, (4, 6), dtype=np.uint8)
    np.save(tmp_path / "g.npy", g)
    assert np.array_equal(read_image(str(tmp_path / "g.npy")), g[..., None])
    f = RNG.random((4, 6, 1)).astype(np.float32)
    f[0, 0, 0], f[0, 1, 0] = 0.0, 1.0
    np.save(tmp_path / "f.npy", f)
    got = read_image(str(tmp_path / "f.npy"))
    want = np.floor(255.0 * f.astype(np.float64) + 0.5).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert got[0, 0, 0] == 0 and got[0, 1, 0] == 255


def test_errors_name_the_file(tmp_path):
    good = _png_bytes(RGB, 2, [0, 1, 2, 3])
    cases = {
        "interlaced.png": _png_bytes(RGB, 2, [0] * 4, interlace=1),
        "deep.png": _png_bytes(RGB, 2, [0] * 4, depth=16),
        # flip one byte of the IDAT chunk's CRC (12 B IEND chunk follows it)
        "crc.png": good[:-13] + bytes([good[-13] ^ 0xFF]) + good[-12:],
        # cut inside the IDAT body: 8 magic + 25 IHDR + 8 IDAT head + 5
        "cut.png": good[:8 + 25 + 8 + 5],
        "what.xyz": b"\x00\x01 not an image at all",
    }
    want = {"interlaced.png": "interlace", "deep.png": "16"}
    for name, data in cases.items():
        p = _write(tmp_path, name, data)
        with pytest.raises(ValueError) as e:
            read_image(p)
        assert p in str(e.value), name
        assert want.get(name, "") in str(e.value), name


def test_corrupt_zlib_stream_is_a_value_error(tmp_path):
    body = b"\x78\x9c" + b"\xff" * 20  # zlib header, garbage deflate data
    data = (b"\x89PNG\r\n\x1a\n"
            + _chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 4, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", body) + _chunk(b"IEND", b""))
    p = _write(tmp_path, "zl.png", data)
    with pytest.raises(ValueError) as e:
        read_image(p)
    assert p in str(e.value)


def test_unknown_format_without_pillow_lists_the_formats(tmp_path, monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "PIL", None)  # `import PIL` now fails
    p = _write(tmp_path, "photo.jpg", b"\xff\xd8\xff\xe0" + b"\0" * 32)
    with pytest.raises(ValueError) as e:
        read_image(p)
    assert p in str(e.value)
    for fmt in ("PNG", "PGM/PPM", "BMP", ".npy"):
        assert fmt in str(e.value)
    # and the stdlib decoders never needed it
    png = _write(tmp_path, "ok.png", _png_bytes(RGB, 2, [4, 3, 2, 1]))
    assert np.array_equal(read_image(png), RGB)


def test_pillow_cross_check(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a = RNG.integers(0, 256, (17, 33, 3), dtype=np.uint8)
    # smooth half so the optimiser picks adaptive (non-zero) filters
    a[:, :16] = (np.arange(17)[:, None, None] * 9
                 + np.arange(16)[None, :, None] * 5).astype(np.uint8)
    for mode, arr in (("RGB", a), ("L", a[..., 0])):
        p = str(tmp_path / f"pil_{mode}.png")
        Image.fromarray(arr, mode).save(p, optimize=True)
        want = arr if arr.ndim == 3 else arr[..., None]
        assert np.array_equal(read_image(p), want)
        pb = str(tmp_path / f"pil_{mode}.bmp")
        Image.fromarray(arr, mode).save(pb)
        got = read_image(pb)
        if mode == "L":  # Pillow writes gray BMPs as 8-bit palettised
            assert np.array_equal(got, np.repeat(want, 3, axis=2))
        else:
            assert np.array_equal(got, want)
