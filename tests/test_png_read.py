"""CPU tests of ws_png_read_rgba8 (include/websplat.h): round trips through the writer, hand-made files of every filter type and
colour type against the oracle's reader, damaged files refused without a crash, unsupported flavours named as such."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ws_oracle_io as oio  # noqa: E402

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}


def _chunk(typ, data, crc=None):
    crc = zlib.crc32(typ + data) if crc is None else crc
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", crc & 0xFFFFFFFF)


def _filter_rows(px, filters):
    """px: H x W x C uint8; filters: one type per row (cycled) -> the filtered scanlines (ISO/IEC 15948 section 9)"""
    h, w, c = px.shape
    rows = px.reshape(h, w * c).astype(np.int32)
    out = bytearray()
    for y in range(h):
        f = filters[y % len(filters)]
        cur, prev = rows[y], rows[y - 1] if y else np.zeros(w * c, np.int32)
        a = np.concatenate([np.zeros(c, np.int32), cur[:-c]])
        cc = np.concatenate([np.zeros(c, np.int32), prev[:-c]])
        if f == 0:
            pr = np.zeros_like(cur)
        elif f == 1:
            pr = a
        elif f == 2:
            pr = prev
        elif f == 3:
            pr = (a + prev) // 2
        else:
            pa, pb, pc = np.abs(prev - cc), np.abs(a - cc), np.abs(a + prev - 2 * cc)
            pr = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, cc))
        out.append(f)
        out += ((cur - pr) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def _png(px, ctype, filters=(0,), depth=8, interlace=0, idat_parts=1, extra=(), level=6):
    h, w = px.shape[:2]
    raw = zlib.compress(_filter_rows(px, filters), level)
    step = max(1, (len(raw) + idat_parts - 1) // idat_parts)
    body = b"".join(_chunk(b"IDAT", raw[i:i + step]) for i in range(0, len(raw), step))
    return SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)) + b"".join(extra) + body + _chunk(b"IEND", b"")


def _expand(px, ctype):
    h, w = px.shape[:2]
    out = np.full((h, w, 4), 255, np.uint8)
    if ctype in (0, 4):
        out[..., :3] = px[..., :1]
        if ctype == 4:
            out[..., 3] = px[..., 1]
    else:
        out[..., :px.shape[2]] = px
    return out


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _pixels(w, h, c, seed=0):
    rng = np.random.default_rng(seed)
    smooth = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[..., None] + np.arange(c) * 40) & 255   # gradients: every predictor matters
    return np.where(rng.random((h, w, c)) < 0.2, rng.integers(0, 256, (h, w, c)), smooth).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (64, 3), (33, 17)])
def test_round_trip_through_the_writer(ws, tmp_path, shape):
    w, h = shape
    img = _pixels(w, h, 4, seed=w)
    p = str(tmp_path / "rt.png")
    ws.write_png(p, img)
    got = ws.read_png(p)
    assert got.dtype == np.uint8 and got.shape == (h, w, 4) and np.array_equal(got, img)
    assert np.array_equal(oio.png_read_rgba8(p), img)


@pytest.mark.parametrize("filters", [(0,), (1,), (2,), (3,), (4,), (4, 3, 2, 1, 0), (1, 4)])
def test_rgba_filter_types_against_the_oracle(ws, tmp_path, filters):
    img = _pixels(23, 11, 4, seed=sum(filters))
    p = _write(tmp_path, "f.png", _png(img, 6, filters, idat_parts=3))
    want = oio.png_read_rgba8(p)
    assert np.array_equal(want, img)              # (the hand-made file says what it was meant to)
    assert np.array_equal(ws.read_png(p), want)


@pytest.mark.parametrize("ctype", [0, 4, 2])
@pytest.mark.parametrize("filters", [(0,), (1,), (2,), (3,), (4,), (2, 4, 1, 3)])
def test_grey_greyalpha_rgb(ws, tmp_path, ctype, filters):
    """The oracle reads RGBA only: the same pixels, expanded, written as an RGBA file are its answer."""
    px = _pixels(19, 13, CHANNELS[ctype], seed=ctype)
    text = _chunk(b"tEXt", b"Comment\0hand-made")  # an ancillary chunk is skipped (its CRC still checked)
    p = _write(tmp_path, "c.png", _png(px, ctype, filters, extra=(text,)))
    q = _write(tmp_path, "c_rgba.png", _png(_expand(px, ctype), 6, filters))
    assert np.array_equal(ws.read_png(p), oio.png_read_rgba8(q))


def _refused(ws, path, codes):
    from websplat import _lib as L
    with pytest.raises(ws.WebSplatError) as e:
        ws.read_png(path)
    assert e.value.code in [getattr(L, c) for c in codes], (e.value.code, str(e.value))
    return str(e.value)


def test_damaged_files_are_refused(ws, tmp_path):
    img = _pixels(31, 9, 4, seed=3)
    good = _png(img, 6, (4, 1), level=0)
    assert np.array_equal(ws.read_png(_write(tmp_path, "good.png", good)), img)
    for cut in (0, 4, 8, 20, 33, 40, len(good) // 2, len(good) - 13, len(good) - 12, len(good) - 1):
        _refused(ws, _write(tmp_path, "cut.png", good[:cut]), ["WS_ERR_IO"])
    rng = np.random.default_rng(1)
    for pos in sorted(set([0, 9, 17, 30, len(good) - 2] + list(rng.integers(8, len(good), 40)))):
        bad = bytearray(good)
        bad[pos] ^= 1 << int(rng.integers(0, 8))
        _refused(ws, _write(tmp_path, "flip.png", bytes(bad)), ["WS_ERR_IO", "WS_ERR_UNSUPPORTED"])
    # a bad CRC alone
    ihdr = struct.pack(">IIBBBBB", 31, 9, 8, 6, 0, 0, 0)
    idat = zlib.compress(_filter_rows(img, (0,)))
    msg = _refused(ws, _write(tmp_path, "crc.png", SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat, crc=0x12345678) + _chunk(b"IEND", b"")),
                   ["WS_ERR_IO"])
    assert "CRC" in msg
    # valid CRCs, damaged contents: a filter type that does not exist, too few and too many scanlines
    rows = bytearray(_filter_rows(img, (0,)))
    rows[0] = 5
    for payload in (bytes(rows), _filter_rows(img[:-1], (0,)), _filter_rows(np.concatenate([img, img[:1]]), (0,))):
        data = SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(payload)) + _chunk(b"IEND", b"")
        _refused(ws, _write(tmp_path, "rows.png", data), ["WS_ERR_IO"])
    # absurd sizes in a header with a valid CRC: refused before anything is allocated
    for w, h in ((0x7FFFFFFF, 0x7FFFFFFF), (0xFFFFFFFF, 1), (0, 5), (1 << 20, 1 << 20), (30000, 30000)):
        data = SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"")
        _refused(ws, _write(tmp_path, "huge.png", data), ["WS_ERR_IO"])
    _refused(ws, str(tmp_path / "missing.png"), ["WS_ERR_IO"])
    _refused(ws, _write(tmp_path, "not.png", b"P6 1 1 255 abc"), ["WS_ERR_IO"])


def test_unsupported_flavours(ws, tmp_path):
    img = _pixels(8, 8, 4, seed=5)
    plte = _chunk(b"PLTE", bytes(range(48)))
    files = {"16-bit": _png(np.repeat(img, 2, axis=2), 6, depth=16),
             "palette": _png(img[..., :1] & 15, 3, extra=(plte,)),
             "interlaced": _png(img, 6, interlace=1),
             "grey 4-bit": _png(img[:, :4, :1], 0, depth=4)}
    for name, data in files.items():
        assert "ws_png_read_rgba8" in _refused(ws, _write(tmp_path, "u.png", data), ["WS_ERR_UNSUPPORTED"]), name
