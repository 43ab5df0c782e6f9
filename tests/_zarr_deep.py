"""Zarr v2 arrays whose chunks hold several planes, cut and written by the tests themselves
(test infrastructure only): the expected planes are numpy slices of the 5-D array the chunks
were cut from."""
import itertools
import json

import numpy as np

import _zarr


def noise_array(shape, dtype, seed=0):
    """A (t, c, z, y, x) array, every plane different: a blocky 12-bit background with 9-bit
    noise on one sample in five (compressible with and without shuffle, for every dtype)."""
    t, c, z, h, w = shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    k = np.arange(t * c * z).reshape(t, c, z, 1, 1)
    a = 256 + ((x >> 3) + (y >> 3) + k) % 16 * 48 + 37 * k
    a = a + rng.integers(0, 512, size=shape) * (rng.random(shape) < 0.2)
    a = a.astype(np.float64)
    if np.dtype(dtype).kind == "f":
        a = a * 0.25 - 300.0
    elif np.dtype(dtype).itemsize == 1:
        a = a / 16
    return a.astype(dtype)


def cut_chunks(arr, chunks):
    """{chunk index tuple: full-size chunk array (edges zero-padded on every axis)}."""
    grid = [-(-n // c) for n, c in zip(arr.shape, chunks)]
    out = {}
    for idx in itertools.product(*[range(g) for g in grid]):
        sel = tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, chunks))
        blk = arr[sel]
        full = np.zeros(chunks, dtype=arr.dtype)
        full[tuple(slice(0, n) for n in blk.shape)] = blk
        out[idx] = full
    return out


def encoder(compressor, **kw):
    """bytes -> chunk file for the .zarray compressor id, as _zarr.encode_chunks picks them."""
    def enc(raw, itemsize):
        if compressor == "blosc" and "cname" in kw:
            return _zarr.cblosc_encode(raw, itemsize, **kw)
        if compressor == "blosc":
            return _zarr.blosc_encode(raw, itemsize, **kw)
        if compressor == "zlib":
            return _zarr.zlib_encode(raw, kw.get("level", 1))
        return raw
    return enc


def layer_files(cut, lead, grid_yx, enc, missing=()):
    """The chunk files of one layer (leading chunk indices `lead`), C order over (j, i)."""
    gy, gx = grid_yx
    out = []
    for j in range(gy):
        for i in range(gx):
            idx = tuple(lead) + (j, i)
            out.append(None if idx in missing else enc(cut[idx].tobytes(), cut[idx].dtype.itemsize))
    return out


def slice_of(lead_index, lead_chunks):
    """(leading chunk indices, slice inside the chunk) of a plane's leading (t, c, z) index."""
    s = 0
    for v, e in zip(lead_index, lead_chunks):
        s = s * e + v % e
    return tuple(v // e for v, e in zip(lead_index, lead_chunks)), s


def write_array(root, arr, chunks, compressor, enc, sep="/", missing=(), fill_value=0):
    """An array directory: .zarray and one file per chunk (not those in `missing`)."""
    root.mkdir(parents=True, exist_ok=True)
    meta = {"zarr_format": 2, "shape": list(arr.shape), "chunks": list(chunks), "dtype": arr.dtype.str,
            "order": "C", "fill_value": fill_value, "filters": None, "dimension_separator": sep,
            "compressor": None if compressor is None else {"id": compressor}}
    (root / ".zarray").write_text(json.dumps(meta))
    cut = cut_chunks(arr, chunks)
    for idx, blk in cut.items():
        if idx in missing:
            continue
        path = root / sep.join(str(v) for v in idx)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(enc(blk.tobytes(), blk.dtype.itemsize))
    return cut
