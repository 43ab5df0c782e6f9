"""TIFF Predictor = 3 (the floating-point predictor, Adobe TIFF Technical Note 3) restated in
numpy, a segment builder on tests/_tiff_src.py's writer, and Zstandard segments (Compression =
50000) through the system libzstd (tests/_zarr.py).  Independent of the library under test; pinned
by tests/test_tiff_fp_host.py against the tifffile- and libtiff-written fixtures of
tests/golden/tiff_fp/ and against libtiff (through PIL).

The rule.  A segment row of wc samples of bpp bytes is stored as bpp byte planes of wc bytes
each, plane 0 the most significant bytes in II and MM files alike, and the row's bpp * wc bytes
are differenced byte by byte, each minus the one before it, straight across the plane
boundaries."""
import json
import os
import zlib

import numpy as np

import _tiff_src as T
import _zarr

ZSTD = 50000
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "tiff_fp")


def predict3(a):
    """Forward Predictor = 3 of a (rows, width) float32 / float64 array: the segment rows' bytes
    as they are handed to the codec, a (rows, width * bpp) uint8 array (the same for either byte
    order of `a`)."""
    a = np.ascontiguousarray(a)
    rows, wc = a.shape
    bpp = a.dtype.itemsize
    be = a.astype(a.dtype.newbyteorder(">")).view(np.uint8).reshape(rows, wc, bpp)  # MSB first
    t = np.ascontiguousarray(be.transpose(0, 2, 1)).reshape(rows, bpp * wc)          # byte planes
    d = t.copy()
    d[:, 1:] = t[:, 1:] - t[:, :-1]
    return d


def unpredict3(rows_bytes, dtype):
    """Inverse: (rows, width * bpp) decoded bytes -> the (rows, width) samples as `dtype` (its byte
    order is the file's).  cumsum mod 256, the planes back into samples, reversed for II."""
    dtype = np.dtype(dtype)
    d = np.ascontiguousarray(rows_bytes, dtype=np.uint8)
    rows, rb = d.shape
    bpp = dtype.itemsize
    wc = rb // bpp
    t = np.cumsum(d, axis=1, dtype=np.uint8)
    be = np.ascontiguousarray(t.reshape(rows, bpp, wc).transpose(0, 2, 1))  # (rows, wc, bpp) MSB first
    return be.view(dtype.newbyteorder(">")).reshape(rows, wc).astype(dtype)  # (a byte swap: bit patterns kept)


def compress(seg, compression, checksum=False):
    """_tiff_src.compress plus Compression 50000: one zstd frame (libzstd writes the content
    size; `checksum` adds the XXH64 content checksum)."""
    if compression == ZSTD:
        return _zarr.zstd_frame(bytes(seg), checksum=checksum)
    return T.compress(seg, compression)


def segments_of(a, tile=None, rows_per_strip=None, predictor=1, pad=None):
    """_tiff_src.segments_of with Predictor = 3, and edge tiles padded with the bytes of `pad` (a
    numpy Generator: random padding, which writers difference too; None: zeros)."""
    a = np.ascontiguousarray(a)
    if predictor != 3:
        return T.segments_of(a, tile, rows_per_strip, predictor)
    h, w = a.shape
    segs = []
    if tile:
        tw, th = tile
        for y in range(0, h, th):
            for x in range(0, w, tw):
                if pad is None:
                    t = np.zeros((th, tw), a.dtype)
                else:
                    t = pad.integers(0, 256, th * tw * a.dtype.itemsize, dtype=np.uint8).view(a.dtype).reshape(th, tw)
                    t = t.copy()
                piece = a[y:y + th, x:x + tw]
                t[:piece.shape[0], :piece.shape[1]] = piece
                segs.append(predict3(t).tobytes())
    else:
        rps = rows_per_strip or h
        for y in range(0, h, rps):
            segs.append(predict3(a[y:y + rps]).tobytes())
    return segs


def page_of(a, compression=1, predictor=1, tile=None, rows_per_strip=None, pad=None, **kw):
    """A page dict for _tiff_src.write_tiff from a (rows, width) array in the file's byte order,
    with Predictor 3 and Compression 50000 as well."""
    a = np.ascontiguousarray(a)
    segs = [compress(s, compression) for s in segments_of(a, tile, rows_per_strip, predictor, pad)]
    return dict(width=a.shape[1], length=a.shape[0], bits=a.dtype.itemsize * 8,
                sampleformat={"u": 1, "i": 2, "f": 3}[a.dtype.kind], compression=compression, predictor=predictor,
                tile=tile, rows_per_strip=rows_per_strip or a.shape[0], segments=segs,
                description=kw.get("description"), subifds=list(kw.get("subifds", ())), extra=list(kw.get("extra", ())))


# ------------------------------------------------------------------------- the fixtures
def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)["files"]


def expected(ref):
    """The big-endian plane a manifest reference names ({"npy": ..., "derive": ...})."""
    a = np.load(os.path.join(GOLD, ref["npy"]))
    if ref.get("derive") == "f8_div3":  # the float64 scene: the float32 one / 3 (make_tiff_fp_golden.py)
        a = (a.astype(np.float64) / 3).astype(">f8")
    return a


def zstd_decode(frame, dlen):
    import ctypes
    L = _zarr._libzstd()
    L.ZSTD_decompress.restype = ctypes.c_size_t
    L.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    out = ctypes.create_string_buffer(max(dlen, 1))
    n = L.ZSTD_decompress(out, dlen, bytes(frame), len(frame))
    assert not L.ZSTD_isError(n) and n == dlen, (n, dlen)
    return out.raw[:dlen]


def decode_ifd(path, ifd, sample=0):
    """The plane that is group `sample` of an IFD (a pbx.tiff_ifds dict), decoded on the CPU with
    zlib / libzstd / the Python LZW decoder and the numpy inverse predictors: a (length, width)
    array in the file's byte order."""
    bpp = ifd["bits"] // 8
    dt = np.dtype(ifd["byteorder"] + {1: "u", 2: "i", 3: "f"}[ifd["sampleformat"]] + str(bpp))
    data = open(path, "rb").read()
    gx = -(-ifd["width"] // ifd["seg_w"]) if ifd["tiled"] else 1
    gy = -(-ifd["length"] // ifd["seg_h"])
    out = np.zeros((gy * ifd["seg_h"], gx * ifd["seg_w"]), dt)
    base = sample * gx * gy
    for i in range(gx * gy):
        o, cnt = ifd["offsets"][base + i], ifd["counts"][base + i]
        x0, y0 = (i % gx) * ifd["seg_w"], (i // gx) * ifd["seg_h"]
        rows = ifd["seg_h"] if ifd["tiled"] else min(ifd["seg_h"], ifd["length"] - y0)
        dlen = ifd["seg_w"] * rows * bpp
        raw = data[o:o + cnt]
        c = ifd["compression"]
        dec = (raw if c == 1 else T.lzw_decode(raw, dlen) if c == 5 else zstd_decode(raw, dlen) if c == ZSTD
               else zlib.decompress(raw))
        assert len(dec) == dlen
        if ifd["predictor"] == 3:
            seg = unpredict3(np.frombuffer(dec, np.uint8).reshape(rows, ifd["seg_w"] * bpp), dt)
        else:
            seg = np.frombuffer(dec, dt).reshape(rows, ifd["seg_w"])
            if ifd["predictor"] == 2:
                u = seg.astype(dt.newbyteorder("=")).view("u%d" % bpp)
                seg = np.cumsum(u, axis=1, dtype=u.dtype).view(dt.newbyteorder("=")).astype(dt)
        out[y0:y0 + rows, x0:x0 + ifd["seg_w"]] = seg
    return out[:ifd["length"], :ifd["width"]]
