"""Zarr v3 (NGFF 0.5) arrays written by hand for the tests (test infrastructure only; no zarr
library): zarr.json, chunk keys, the gzip / zstd / blosc / crc32c codecs over _zarr's encoders,
and sharding_indexed shard files with the index at either end and the inner chunks in any order.
Formats: the Zarr v3 core specification and its codec documents, RFC 1952, RFC 8878."""
import itertools
import json
import os
import struct
import zlib

import numpy as np

import _zarr

DATA_TYPES = {"i1": "int8", "u1": "uint8", "i2": "int16", "u2": "uint16", "i4": "int32", "u4": "uint32",
              "f4": "float32", "f8": "float64"}
_TABLE = []


def crc32c(data: bytes) -> int:
    """CRC-32C (Castagnoli), bit by bit into a table, then bytewise."""
    if not _TABLE:
        for n in range(256):
            c = n
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            _TABLE.append(c)
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def with_crc32c(data: bytes) -> bytes:
    return data + struct.pack("<I", crc32c(data))


def gzip_member(raw: bytes, level: int = 6, fname: bytes = None, extra: bytes = None, comment: bytes = None,
                fhcrc: bool = False, flg_extra_bits: int = 0, crc: int = None, isize: int = None) -> bytes:
    """One RFC 1952 member around a raw deflate stream of `raw` (level 0: stored blocks)."""
    flg = (2 if fhcrc else 0) | (4 if extra is not None else 0) | (8 if fname is not None else 0) | \
        (16 if comment is not None else 0) | flg_extra_bits
    head = bytes([0x1f, 0x8b, 8, flg]) + struct.pack("<IBB", 0, 0, 255)
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        head += fname + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(raw) + co.flush()
    return head + body + struct.pack("<II", zlib.crc32(raw) if crc is None else crc,
                                     len(raw) & 0xFFFFFFFF if isize is None else isize)


def zstd_frame_nosize(data: bytes, level: int = 3):
    """A zstd frame whose header carries no content size (ZSTD_c_contentSizeFlag = 200 off), or
    None when libzstd's advanced API does not produce one here."""
    import ctypes
    L = _zarr._libzstd()
    cc = L.ZSTD_createCCtx()
    try:
        L.ZSTD_CCtx_setParameter(cc, 100, level)
        if L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cc, 200, 0)):
            return None
        cap = L.ZSTD_compressBound(len(data))
        out = ctypes.create_string_buffer(cap)
        n = L.ZSTD_compress2(cc, out, cap, data, len(data))
        assert not L.ZSTD_isError(n)
        f = out.raw[:n]
    finally:
        L.ZSTD_freeCCtx(cc)
    fhd = f[4]
    return f if (fhd >> 6) == 0 and not (fhd >> 5) & 1 else None  # no FCS field at all


def codec_entry(codec):
    """The zarr.json entry of a bytes-to-bytes codec name."""
    if codec == "blosc":
        return {"name": "blosc", "configuration": {"cname": "lz4", "clevel": 5, "shuffle": "shuffle",
                                                   "typesize": 2, "blocksize": 0}}
    if codec == "gzip":
        return {"name": "gzip", "configuration": {"level": 5}}
    if codec == "zstd":
        return {"name": "zstd", "configuration": {"level": 3, "checksum": False}}
    raise ValueError(codec)


def encode(raw: bytes, itemsize: int, name, crc: bool = False, **kw) -> bytes:
    """A chunk's bytes through the codec `name` (None, "blosc", "gzip", "zstd"; kw: the
    encoder's options) and, with crc, the crc32c codec."""
    if name == "zstd":
        out = _zarr.zstd_frame(raw, kw.get("level", 3), kw.get("checksum", False))
    elif name == "gzip":
        out = gzip_member(raw, **kw)
    elif name == "blosc":
        out = _zarr.blosc_encode(raw, itemsize, **kw)
    else:
        out = raw
    return with_crc32c(out) if crc else out


def chunk_key(idx, encoding="default", sep=None) -> str:
    if encoding == "default":
        return (sep or "/").join(["c"] + [str(v) for v in idx])
    return (sep or ".").join(str(v) for v in idx)


def cut(arr: np.ndarray, idx, shape) -> np.ndarray:
    """Chunk idx of arr as a full chunk of `shape` (edges zero-padded)."""
    out = np.zeros(shape, dtype=arr.dtype)
    sl = tuple(slice(i * n, (i + 1) * n) for i, n in zip(idx, shape))
    part = arr[sl]
    out[tuple(slice(0, n) for n in part.shape)] = part
    return out


def grid(shape, chunk):
    return itertools.product(*[range(-(-s // c)) for s, c in zip(shape, chunk)])


def shard_file(inner, index_location="end", index_crc=True, order=None) -> bytes:
    """A shard from its inner chunks (C order over the shard's inner grid; None = missing):
    the chunks laid out in `order` (a permutation of the present ones' positions; default C
    order), the index of (offset, nbytes) uint64 LE pairs at the end or the start."""
    n = len(inner)
    size = 16 * n + (4 if index_crc else 0)
    present = [k for k in range(n) if inner[k] is not None]
    order = present if order is None else [k for k in order if inner[k] is not None]
    assert sorted(order) == present
    pos = size if index_location == "start" else 0
    entries = [(2 ** 64 - 1, 2 ** 64 - 1)] * n
    body = b""
    for k in order:
        entries[k] = (pos, len(inner[k]))
        body += inner[k]
        pos += len(inner[k])
    index = b"".join(struct.pack("<QQ", *e) for e in entries)
    if index_crc:
        index = with_crc32c(index)
    return index + body if index_location == "start" else body + index


def write_array(adir, arr: np.ndarray, chunk, codec=None, crc=False, shard=None, index_location="end",
                index_crc=True, permute=None, missing=(), missing_shards=(), encoding="default", sep=None,
                fill_value=0, endian="big", enc_kw=None, extra_meta=None):
    """Write arr (big-endian values in, stored in `endian` order) as a Zarr v3 array directory.
    chunk: the chunk shape, or with shard=(shard shape) the inner chunk shape.  missing: inner /
    plain chunk indices left out; missing_shards: shard indices whose file is not written;
    permute: a function(list of inner positions) -> the order they get in the file."""
    os.makedirs(adir, exist_ok=True)
    dt = arr.dtype.newbyteorder("<" if endian == "little" else ">")
    stored = arr.astype(dt)
    item = dt.itemsize
    inner = [{"name": "bytes", "configuration": {"endian": endian}}]
    if item == 1 and endian is None:
        inner = [{"name": "bytes"}]
    if codec:
        inner.append(codec_entry(codec))
    if crc:
        inner.append({"name": "crc32c"})
    if shard:
        codecs = [{"name": "sharding_indexed", "configuration": {
            "chunk_shape": list(chunk), "codecs": inner, "index_location": index_location,
            "index_codecs": [{"name": "bytes", "configuration": {"endian": "little"}}] +
                            ([{"name": "crc32c"}] if index_crc else [])}}]
    else:
        codecs = inner
    key_cfg = {"name": encoding}
    if sep is not None:
        key_cfg["configuration"] = {"separator": sep}
    meta = {"zarr_format": 3, "node_type": "array", "shape": list(arr.shape),
            "data_type": DATA_TYPES[dt.str[1:]],
            "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": list(shard or chunk)}},
            "chunk_key_encoding": key_cfg, "fill_value": fill_value, "codecs": codecs, "attributes": {}}
    meta.update(extra_meta or {})
    with open(os.path.join(adir, "zarr.json"), "w") as f:
        json.dump(meta, f)
    enc_kw = enc_kw or {}

    def put(idx, data):
        path = os.path.join(adir, chunk_key(idx, encoding, sep))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)

    if not shard:
        for idx in grid(arr.shape, chunk):
            if idx not in missing:
                put(idx, encode(cut(stored, idx, chunk).tobytes(), item, codec, crc, **enc_kw))
        return
    per = [s // c for s, c in zip(shard, chunk)]
    for sidx in grid(arr.shape, shard):
        if sidx in missing_shards:
            continue
        parts = []
        for sub in itertools.product(*[range(p) for p in per]):
            idx = tuple(s * p + k for s, p, k in zip(sidx, per, sub))
            outside = any(i * c >= n for i, c, n in zip(idx, chunk, arr.shape))
            parts.append(None if idx in missing or outside else
                         encode(cut(stored, idx, chunk).tobytes(), item, codec, crc, **enc_kw))
        order = permute(list(range(len(parts)))) if permute else None
        put(sidx, shard_file(parts, index_location, index_crc, order))


def write_group(gdir, ome: dict):
    os.makedirs(gdir, exist_ok=True)
    with open(os.path.join(gdir, "zarr.json"), "w") as f:
        json.dump({"zarr_format": 3, "node_type": "group", "attributes": {"ome": ome}}, f)
