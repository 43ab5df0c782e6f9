"""TIFF Predictor = 2 (horizontal differencing, TIFF 6.0 section 14) restated in numpy: the
yardstick of tests/test_tiff_predictor.py and tests/test_gpu_tiff_predictor.py.

A tile is h rows of w samples of bpp bytes, big-endian.  Sample 0 of every row stays; sample
i > 0 becomes (s[i] - s[i-1]) mod 2^(8 bpp), subtracted on the sample value and stored
big-endian.  Tiled TIFF: every row of every T x T sub-tile restarts, and the zero padding of an
edge sub-tile is differenced like data (the first pad sample is 0 - last valid, the rest 0).
Nothing here reads the library under test."""
import zlib

import numpy as np

BPP = [1, 1, 2, 2, 4, 4, 4, 8]
UDT = {1: ">u1", 2: ">u2", 4: ">u4"}
TAG_PREDICTOR = 317


def _samples(tile_be, w, h, bpp):
    """The tile's samples as unsigned integers of their width (two's complement bit patterns)."""
    a = np.frombuffer(bytes(tile_be), UDT[bpp])
    assert a.size == w * h, (a.size, w, h)
    return a.reshape(h, w).astype("=u%d" % bpp)


def forward(tile_be, w, h, bpp):
    """Big-endian tile bytes -> the differenced stream bytes."""
    s = _samples(tile_be, w, h, bpp)
    d = s.copy()
    d[:, 1:] = s[:, 1:] - s[:, :-1]  # unsigned arithmetic wraps mod 2^(8 bpp)
    return d.astype(UDT[bpp]).tobytes()


def inverse(stream, w, h, bpp):
    """The differenced stream bytes -> big-endian tile bytes (what a decoder accumulates)."""
    d = _samples(stream, w, h, bpp)
    return np.cumsum(d, axis=1, dtype=d.dtype).astype(UDT[bpp]).tobytes()


def pad_subtile(tile_be, w, h, bpp, t, tx, ty):
    """Sub-tile (tx, ty) of a w x h tile as t x t big-endian samples, zero-padded."""
    a = np.frombuffer(bytes(tile_be), UDT[bpp]).reshape(h, w)
    pad = np.zeros((t, t), UDT[bpp])
    part = a[ty * t:(ty + 1) * t, tx * t:(tx + 1) * t]
    pad[:part.shape[0], :part.shape[1]] = part
    return pad.tobytes()


def forward_subtiles(tile_be, w, h, bpp, t):
    """The differenced t x t streams of every sub-tile, row-major over the region."""
    ntx, nty = -(-w // t), -(-h // t)
    return [forward(pad_subtile(tile_be, w, h, bpp, t, tx, ty), t, t, bpp)
            for ty in range(nty) for tx in range(ntx)]


# ------------------------------------------------------------------------- reading a TIFF

def ifd(body):
    """{tag: (type, count, value-or-offset)} and the tag order of a big-endian classic TIFF."""
    assert body[:4] == b"MM\x00\x2a"
    at = int.from_bytes(body[4:8], "big")
    n = int.from_bytes(body[at:at + 2], "big")
    tags, order = {}, []
    for k in range(n):
        e = body[at + 2 + 12 * k: at + 14 + 12 * k]
        tag, typ, cnt = (int.from_bytes(e[0:2], "big"), int.from_bytes(e[2:4], "big"),
                         int.from_bytes(e[4:8], "big"))
        val = int.from_bytes(e[8:10], "big") if typ == 3 and cnt == 1 else int.from_bytes(e[8:12], "big")
        tags[tag] = (typ, cnt, val)
        order.append(tag)
    assert int.from_bytes(body[at + 2 + 12 * n: at + 6 + 12 * n], "big") == 0  # no next IFD
    return tags, order, at + 6 + 12 * n


def _array(body, entry):
    typ, cnt, val = entry
    if cnt == 1:
        return [val]
    assert typ == 4
    return [int.from_bytes(body[val + 4 * k: val + 4 * k + 4], "big") for k in range(cnt)]


def pieces(body):
    """The inflated strips (tags 273 / 279) or sub-tiles (324 / 325) of a deflated TIFF, in
    order, and its tags.  The Predictor is not undone."""
    tags, order, _ = ifd(body)
    assert tags[259][2] == 8
    o, c = (324, 325) if 324 in tags else (273, 279)
    offs, cnts = _array(body, tags[o]), _array(body, tags[c])
    return [zlib.decompress(body[a:a + n]) for a, n in zip(offs, cnts)], tags, order


# ------------------------------------------------------------------------------ test data

def smooth_scene(w, h, seed):
    """Poisson counts of a smooth lambda field (50..430): uint16, the kind of plane a microscope
    writes -- spatially correlated, with shot noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.arange(h, dtype=np.float64)[:, None], np.arange(w, dtype=np.float64)[None, :]
    lam = 240.0 + 110.0 * np.sin(xx / 83.0 + 0.3) * np.cos(yy / 61.0) + 80.0 * np.sin((xx + 2 * yy) / 190.0)
    return rng.poisson(np.clip(lam, 50.0, 430.0)).astype(np.uint16)
