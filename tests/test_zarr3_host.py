"""Zarr v3 (NGFF 0.5) arrays, host side (no GPU): zarr3_array_meta, chunk keys, fill values,
shard indexes, which files a band spec opens, and the host planner (pbx_test_zarr_plan) for the
zstd / gzip codecs and the crc32c flag.

Arrays are written by tests/_zarr3.py; the expected chunk bytes are what that writer's encoders
give for the numpy array the test started from."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

import _zarr
import _zarr3 as Z3
import pbx


def test_crc32c_check_value():
    assert pbx.crc32c(b"123456789") == 0xE3069283
    assert Z3.crc32c(b"123456789") == 0xE3069283
    assert pbx.crc32c(b"") == 0
    assert pbx.crc32c(b"6789", pbx.crc32c(b"12345")) == 0xE3069283  # continues from a running value


def test_names_are_exported():
    assert (pbx.ZARR_ZSTD, pbx.ZARR_GZIP, pbx.ZARR_F_CRC32C) == (3, 4, 1)
    assert pbx.ZARR_CODECS["zstd"] == 3 and pbx.ZARR_CODECS["gzip"] == 4
    assert ctypes_sizeof_chunks() == 40 and pbx.lib().pbx_abi_version() == 9


def ctypes_sizeof_chunks():
    import ctypes
    assert pbx.PbxZarrChunks.flags.offset == 12
    return ctypes.sizeof(pbx.PbxZarrChunks)


# ------------------------------------------------------------------------------ metadata
def base_meta(**change):
    m = {"zarr_format": 3, "node_type": "array", "shape": [3, 70, 100], "data_type": "uint16",
         "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": [1, 32, 64]}},
         "chunk_key_encoding": {"name": "default"}, "fill_value": 0,
         "codecs": [{"name": "bytes", "configuration": {"endian": "little"}}], "attributes": {}}
    m.update(change)
    return m


def meta_of(tmp_path, doc):
    d = tmp_path / ("m%d" % len(list(tmp_path.iterdir())))
    d.mkdir()
    (d / "zarr.json").write_text(json.dumps(doc))
    return pbx.zarr3_array_meta(str(d))


BYTES_LE = {"name": "bytes", "configuration": {"endian": "little"}}
BYTES_BE = {"name": "bytes", "configuration": {"endian": "big"}}


def sharding(inner=None, chunk=(1, 16, 32), **cfg):
    c = {"chunk_shape": list(chunk), "codecs": inner or [BYTES_LE, {"name": "zstd"}],
         "index_codecs": [BYTES_LE, {"name": "crc32c"}]}
    c.update(cfg)
    return [{"name": "sharding_indexed", "configuration": c}]


def test_meta_accepts_the_supported_forms(tmp_path):
    m = meta_of(tmp_path, base_meta())
    assert m["shape"] == [3, 70, 100] and m["chunks"] == [1, 32, 64] and m["dtype"] == "<u2"
    assert m["compressor"] is None and not m["crc32c"] and m["shard"] is None
    assert m["key_encoding"] == ("c", "/") and m["zarr_format"] == 3
    for name in ("blosc", "gzip", "zstd"):
        for crc in (False, True):
            codecs = [BYTES_BE, {"name": name, "configuration": {}}] + ([{"name": "crc32c"}] if crc else [])
            m = meta_of(tmp_path, base_meta(codecs=codecs))
            assert m["compressor"] == {"id": name} and m["crc32c"] is crc and m["dtype"] == ">u2"
    m = meta_of(tmp_path, base_meta(codecs=[BYTES_LE, {"name": "crc32c"}]))
    assert m["compressor"] is None and m["crc32c"]
    for v3, v2 in Z3.DATA_TYPES.items():
        m = meta_of(tmp_path, base_meta(data_type=v2))
        assert m["dtype"][1:] == v3
    # 1-byte types need no endian
    assert meta_of(tmp_path, base_meta(data_type="uint8", codecs=[{"name": "bytes"}]))["dtype"] == "|u1"
    # shards: the inner chunk shape becomes the chunk grid
    m = meta_of(tmp_path, base_meta(codecs=sharding()))
    assert m["chunks"] == [1, 16, 32] and m["compressor"] == {"id": "zstd"}
    assert m["shard"] == dict(shape=[1, 32, 64], index_location="end", index_crc32c=True)
    m = meta_of(tmp_path, base_meta(codecs=sharding([BYTES_BE, {"name": "gzip"}, {"name": "crc32c"}],
                                                    index_location="start", index_codecs=[BYTES_LE])))
    assert m["shard"] == dict(shape=[1, 32, 64], index_location="start", index_crc32c=False)
    assert m["crc32c"] and m["dtype"] == ">u2" and m["compressor"] == {"id": "gzip"}


REFUSED = {
    "zarr_format 2": base_meta(zarr_format=2),
    "a group": base_meta(node_type="group"),
    "complex64": base_meta(data_type="complex64"),
    "bool": base_meta(data_type="bool"),
    "int64": base_meta(data_type="int64"),
    "rectilinear grid": base_meta(chunk_grid={"name": "rectilinear", "configuration": {"chunk_shape": [1, 32, 64]}}),
    "unknown key encoding": base_meta(chunk_key_encoding={"name": "fancy"}),
    "storage transformer": base_meta(storage_transformers=[{"name": "x"}]),
    "fill_value string": base_meta(fill_value="nope"),
    "fill_value NaN for an integer": base_meta(fill_value="NaN"),
    "fill_value too wide": base_meta(fill_value="0x12345"),
    "fill_value out of range": base_meta(fill_value=70000),
    "fill_value list": base_meta(fill_value=[1, 2]),
    "no codecs": base_meta(codecs=[]),
    "no bytes codec": base_meta(codecs=[{"name": "zstd"}]),
    "no endian for 2 bytes": base_meta(codecs=[{"name": "bytes"}]),
    "transpose": base_meta(codecs=[{"name": "transpose", "configuration": {"order": [0, 2, 1]}}, BYTES_LE]),
    "transpose after bytes": base_meta(codecs=[BYTES_LE, {"name": "transpose"}]),
    "two compressors": base_meta(codecs=[BYTES_LE, {"name": "gzip"}, {"name": "zstd"}]),
    "crc32c not last": base_meta(codecs=[BYTES_LE, {"name": "crc32c"}, {"name": "zstd"}]),
    "unknown codec": base_meta(codecs=[BYTES_LE, {"name": "lzma"}]),
    "sharding beside another codec": base_meta(codecs=sharding() + [{"name": "crc32c"}]),
    "nested sharding": base_meta(codecs=sharding(sharding(chunk=(1, 8, 8)))),
    "inner shape does not divide": base_meta(codecs=sharding(chunk=(1, 10, 32))),
    "inner shape rank": base_meta(codecs=sharding(chunk=(16, 32))),
    "index_location": base_meta(codecs=sharding(index_location="middle")),
    "big-endian index": base_meta(codecs=sharding(index_codecs=[BYTES_BE])),
    "compressed index": base_meta(codecs=sharding(index_codecs=[BYTES_LE, {"name": "zstd"}])),
    "chunk rank": base_meta(chunk_grid={"name": "regular", "configuration": {"chunk_shape": [32, 64]}}),
    "chunk extent 0": base_meta(chunk_grid={"name": "regular", "configuration": {"chunk_shape": [1, 0, 64]}}),
    "rank 1": base_meta(shape=[100], chunk_grid={"name": "regular", "configuration": {"chunk_shape": [10]}}),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_meta_refuses(tmp_path, what):
    with pytest.raises(pbx.PbxError) as ei:
        meta_of(tmp_path, REFUSED[what])
    assert ei.value.status == 400


def test_v2_zarray_saying_format_3_stays_400(tmp_path):
    """The v2 reader is not the way in: a .zarray wins over a zarr.json beside it."""
    d = tmp_path / "a"
    d.mkdir()
    (d / ".zarray").write_text(json.dumps({"zarr_format": 3, "shape": [8, 8], "chunks": [8, 8],
                                           "dtype": "<u2", "order": "C", "compressor": None}))
    (d / "zarr.json").write_text(json.dumps(base_meta()))
    with pytest.raises(pbx.PbxError) as ei:
        pbx.zarr_array_meta(str(d))
    assert ei.value.status == 400
    with pytest.raises(pbx.PbxError) as ei:
        pbx.zarr_plane_spec(str(d), 1, 0, 0, 0)
    assert ei.value.status == 400


@pytest.mark.parametrize("fv,dtype,bits", [
    (9, "uint16", 9), (-2, "int16", 0xFFFE), (1.5, "float32", 0x3FC00000), ("NaN", "float32", 0x7FC00000),
    ("Infinity", "float32", 0x7F800000), ("-Infinity", "float64", 0xFFF0000000000000),
    ("0x7fc00001", "float32", 0x7FC00001), ("0x00ff", "uint16", 0xFF), (0, "uint8", 0), (3.0, "uint8", 3)])
def test_fill_values(tmp_path, fv, dtype, bits):
    codecs = [{"name": "bytes"}] if dtype.endswith("int8") else [BYTES_LE]
    m = meta_of(tmp_path, base_meta(fill_value=fv, data_type=dtype, codecs=codecs))
    assert m["fill_bits"] == bits
    # ... and it reaches the spec (no chunk file exists: every chunk is fill)
    d = tmp_path / "spec"
    d.mkdir()
    (d / "zarr.json").write_text(json.dumps(base_meta(fill_value=fv, data_type=dtype, codecs=codecs)))
    sp = pbx.zarr_plane_spec(str(d), 1, 2, 0, 0)
    assert sp["fill_bits"] == bits and sp["chunks"] == [None] * 6 and "crc32c" not in sp


# ------------------------------------------------------------------------------ chunk keys
@pytest.fixture
def opened(monkeypatch):
    """The files pbx reads (present or not), in order."""
    paths = []
    real = pbx._read_chunk_file

    def spy(path):
        paths.append(path)
        return real(path)
    monkeypatch.setattr(pbx, "_read_chunk_file", spy)
    return paths


@pytest.mark.parametrize("encoding,sep,names", [
    ("default", None, ["c/1/0/0", "c/1/0/1", "c/1/1/0", "c/1/1/1"]),
    ("default", ".", ["c.1.0.0", "c.1.0.1", "c.1.1.0", "c.1.1.1"]),
    ("v2", None, ["1.0.0", "1.0.1", "1.1.0", "1.1.1"]),
    ("v2", "/", ["1/0/0", "1/0/1", "1/1/0", "1/1/1"])])
def test_key_encodings(tmp_path, opened, encoding, sep, names):
    arr = np.arange(2 * 40 * 100, dtype=">u2").reshape(2, 40, 100)
    adir = str(tmp_path / "a")
    Z3.write_array(adir, arr, (1, 32, 64), "gzip", crc=True, encoding=encoding, sep=sep, endian="little",
                   missing={(1, 1, 0)})
    sp = pbx.zarr_plane_spec(adir, 4, 1, 0, 0)  # 3-D: the leading axis is z
    assert [os.path.relpath(p, adir) for p in opened] == names
    assert (sp["size_x"], sp["size_y"], sp["chunk_x"], sp["chunk_y"]) == (100, 40, 64, 32)
    assert sp["codec"] == "gzip" and sp["crc32c"] is True and not sp["big_endian"] and sp["pixel_type"] == pbx.UINT16
    stored = arr.astype("<u2")
    for k, idx in enumerate([(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]):
        if idx == (1, 1, 0):
            assert sp["chunks"][k] is None
            continue
        data = sp["chunks"][k]
        assert Z3.crc32c(data[:-4]) == struct.unpack("<I", data[-4:])[0]
        import gzip
        assert gzip.decompress(data[:-4]) == Z3.cut(stored, idx, (1, 32, 64)).tobytes()


# ------------------------------------------------------------------------------ shards
SH_SHAPE, SH_SHARD, SH_INNER = (2, 150, 200), (1, 64, 128), (1, 32, 32)


def sharded(tmp_path, name, **kw):
    arr = _zarr.noise_plane(SH_SHAPE[0] * SH_SHAPE[1], SH_SHAPE[2], ">u2", seed=3).reshape(SH_SHAPE)
    adir = str(tmp_path / name)
    Z3.write_array(adir, arr, SH_INNER, "zstd", shard=SH_SHARD, **kw)
    return arr, adir


def check_plane(arr, z, sp, rows=None):
    gx = -(-SH_SHAPE[2] // 32)
    j0 = 0 if rows is None else rows[0] // 32
    for k, data in enumerate(sp["chunks"]):
        j, i = j0 + k // gx, k % gx
        if data is None:
            continue
        want = Z3.cut(arr, (z, j, i), SH_INNER).tobytes()
        body = data[:-4] if sp.get("crc32c") else data
        assert Z3.encode(want, 2, "zstd") == body, (z, j, i)


@pytest.mark.parametrize("loc", ["end", "start"])
@pytest.mark.parametrize("index_crc", [True, False])
def test_shard_index_end_and_start(tmp_path, loc, index_crc):
    missing = {(1, 0, 1), (1, 3, 5)}
    arr, adir = sharded(tmp_path, "s", index_location=loc, index_crc=index_crc, missing=missing,
                        permute=lambda ks: ks[::-1], crc=True)
    sp = pbx.zarr_plane_spec(adir, 1, 1, 0, 0)
    assert (sp["chunk_x"], sp["chunk_y"], sp["codec"], sp["crc32c"]) == (32, 32, "zstd", True)
    gx = 7
    assert len(sp["chunks"]) == 5 * gx
    assert [k for k, d in enumerate(sp["chunks"]) if d is None] == [0 * gx + 1, 3 * gx + 5]
    check_plane(arr, 1, sp)


def test_missing_shard_file_and_chunks_past_the_array(tmp_path):
    arr, adir = sharded(tmp_path, "s", missing_shards={(0, 1, 0)})
    sp = pbx.zarr_plane_spec(adir, 1, 0, 0, 0)
    gx = 7
    none = sorted(k for k, d in enumerate(sp["chunks"]) if d is None)
    # shard (0, 1, 0) holds inner rows 2..3, inner columns 0..3
    assert none == sorted(j * gx + i for j in (2, 3) for i in range(4))
    check_plane(arr, 0, sp)


def corrupt(adir, key, fn):
    path = os.path.join(adir, key)
    data = bytearray(open(path, "rb").read())
    data = fn(data)
    open(path, "wb").write(bytes(data))


@pytest.mark.parametrize("loc", ["end", "start"])
def test_bad_shard_indexes_are_400(tmp_path, loc):
    n, size = 2 * 4, 16 * 8 + 4
    arr, adir = sharded(tmp_path, "crc", index_location=loc)

    def flip(d):
        d[(0 if loc == "start" else len(d) - size) + 3] ^= 1
        return d
    corrupt(adir, "c/0/0/0", flip)
    with pytest.raises(pbx.PbxError) as ei:
        pbx.zarr_plane_spec(adir, 1, 0, 0, 0)
    assert ei.value.status == 400 and "checksum" in str(ei.value)
    pbx.zarr_band_spec(adir, 1, 0, 0, 70, 30)  # rows of other shards do not open it

    # a range past the file / inside the index, with a valid index checksum
    for off, nb in ((10 ** 6, 8), (None, 10 ** 6), ("index", 8)):
        arr, adir = sharded(tmp_path, "r%s%s" % (off, nb), index_location=loc)

        def move(d):
            lo = 0 if loc == "start" else len(d) - size
            o = lo + 4 if off == "index" else (struct.unpack_from("<Q", d, lo)[0] if off is None else off)
            struct.pack_into("<QQ", d, lo, o, nb)
            struct.pack_into("<I", d, lo + size - 4, Z3.crc32c(bytes(d[lo:lo + size - 4])))
            return d
        corrupt(adir, "c/0/0/0", move)
        with pytest.raises(pbx.PbxError) as ei:
            pbx.zarr_plane_spec(adir, 1, 0, 0, 0)
        assert ei.value.status == 400 and "outside" in str(ei.value)
    # a file shorter than its index
    arr, adir = sharded(tmp_path, "short", index_location=loc)
    corrupt(adir, "c/0/0/0", lambda d: d[:size - 1])
    with pytest.raises(pbx.PbxError) as ei:
        pbx.zarr_plane_spec(adir, 1, 0, 0, 0)
    assert ei.value.status == 400


def test_band_spec_opens_only_the_covering_shards_once(tmp_path, opened):
    arr, adir = sharded(tmp_path, "s")
    rel = lambda: [os.path.relpath(p, adir) for p in opened]
    sp = pbx.zarr_band_spec(adir, 1, 0, 0, 70, 50)  # rows 70..119: inner rows 2..3 = shard row 1
    assert rel() == ["c/1/1/0", "c/1/1/1"]
    assert len(sp["chunks"]) == 2 * 7 and (sp["y0"], sp["rows"]) == (70, 50)
    check_plane(arr, 1, sp, rows=(70, 50))
    del opened[:]
    sp = pbx.zarr_band_spec(adir, 0, 0, 0, 60, 10)  # rows 60..69 straddle shard rows 0 and 1
    assert rel() == ["c/0/0/0", "c/0/0/1", "c/0/1/0", "c/0/1/1"]
    check_plane(arr, 0, sp, rows=(60, 10))
    del opened[:]
    sp = pbx.zarr_band_spec(adir, 0, 0, 0, 0, 0)  # geometry only
    assert rel() == [] and sp["chunks"] == []
    # NgffSource goes the same way (an NGFF 0.5 group around the array)
    root = tmp_path / "img"
    Z3.write_group(str(root), {"version": "0.5", "multiscales": [{
        "axes": [{"name": a} for a in "zyx"], "datasets": [{"path": "0"}]}]})
    os.rename(adir, str(root / "0"))
    src = pbx.NgffSource({3: str(root)})
    px = src.get_pixels(3)
    assert (px.size_z, px.size_c, px.size_t, px.size_x, px.size_y, px.levels) == (2, 1, 1, 200, 150, 1)
    assert px.pixel_type == pbx.UINT16 and src.level_size(px, 0) == (200, 150)
    del opened[:]
    bs = src.band_chunks(px, 1, 0, 0, 0, 128, 22)
    assert [os.path.relpath(p, str(root / "0")) for p in opened] == ["c/1/2/0", "c/1/2/1"]
    check_plane(arr, 1, bs, rows=(128, 22))


def test_ngff_05_group_attributes(tmp_path):
    root = tmp_path / "plate"
    Z3.write_group(str(root), {"version": "0.5", "bioformats2raw.layout": 3})
    ms = {"version": "0.5", "multiscales": [{"axes": [{"name": a} for a in "cyx"],
                                             "datasets": [{"path": "0"}, {"path": "1"}]}]}
    Z3.write_group(str(root / "0"), ms)
    got, where = pbx.ngff_multiscales(str(root))
    assert where == str(root / "0") and [d["path"] for d in got["datasets"]] == ["0", "1"]
    bad = tmp_path / "bad"
    Z3.write_group(str(bad), {"version": "0.5"})
    with pytest.raises(pbx.PbxError) as ei:
        pbx.ngff_multiscales(str(bad))
    assert ei.value.status == 400
    (tmp_path / "arr").mkdir()
    (tmp_path / "arr" / "zarr.json").write_text(json.dumps(base_meta()))
    with pytest.raises(pbx.PbxError) as ei:
        pbx.ngff_multiscales(str(tmp_path / "arr"))
    assert ei.value.status == 400


def test_v2_zarray_with_zstd_and_gzip_compressors(tmp_path):
    for comp in ("zstd", "gzip"):
        d = tmp_path / comp
        d.mkdir()
        (d / ".zarray").write_text(json.dumps({
            "zarr_format": 2, "shape": [40, 40], "chunks": [32, 32], "dtype": "<u2", "order": "C",
            "fill_value": 0, "filters": None, "compressor": {"id": comp, "level": 1}}))
        sp = pbx.zarr_plane_spec(str(d), 1, 0, 0, 0)
        assert sp["codec"] == comp and sp["codec"] in pbx.ZARR_CODECS and "crc32c" not in sp


# ------------------------------------------------------------------------------ the planner
CY, CX, BPP = 24, 40, 2
CB = CY * CX * BPP


def plan(chunks, codec, flags=0, gx=2, gy=2):
    import ctypes
    data, offsets = pbx.pack_chunks(chunks)
    zc = pbx.PbxZarrChunks()
    zc.chunk_x, zc.chunk_y, zc.codec, zc.flags = CX, CY, codec, flags
    zc.data, zc.offsets = data.ctypes.data, offsets.ctypes.data
    out = (ctypes.c_uint64 * 4)()
    sl = (ctypes.c_int32 * 1)(0)
    st = pbx.lib().pbx_test_zarr_plan(ctypes.byref(zc), CX * gx, CY * gy, BPP, 1, sl, 1, 0, 0, out)
    return st, list(out)


def raws(n=4):
    rng = np.random.default_rng(7)
    return [rng.integers(0, 300, CY * CX).astype("<u2").tobytes() for _ in range(n)]


def test_plan_zstd_and_gzip_one_stream_per_present_chunk():
    r = raws()
    for codec, enc in ((pbx.ZARR_ZSTD, lambda b: _zarr.zstd_frame(b, 3)), (pbx.ZARR_GZIP, Z3.gzip_member)):
        chunks = [enc(r[0]), None, enc(r[2]), enc(r[3])]
        assert plan(chunks, codec) == (0, [3, 3 * CB, 0, 3 * ((CB + 255) & ~255)])
        crc = [Z3.with_crc32c(c) if c else None for c in chunks]
        assert plan(crc, codec, pbx.ZARR_F_CRC32C)[:1] == (0,)
        assert plan(crc, codec, pbx.ZARR_F_CRC32C)[1][0] == 3
        # without the flag the 4 checksum bytes trail the frame / move the trailer
        assert plan(crc, codec)[0] == 400
    # zstd with a content checksum, and gzip with every optional header field
    assert plan([_zarr.zstd_frame(b, 3, checksum=True) for b in r], pbx.ZARR_ZSTD)[0] == 0
    full = [Z3.gzip_member(b, 6, fname=b"chunk", extra=b"ab\x02\x00xy", comment=b"hi", fhcrc=True) for b in r]
    assert plan(full, pbx.ZARR_GZIP) == (0, [4, 4 * CB, 0, 4 * ((CB + 255) & ~255)])
    # raw chunks under the flag plan no stream
    assert plan([Z3.with_crc32c(b) for b in r], pbx.ZARR_RAW, pbx.ZARR_F_CRC32C) == (0, [0, 0, 0, 0])


def plan_one(chunk, codec, flags=0):
    st, _ = plan([chunk], codec, flags, gx=1, gy=1)
    err = pbx.lib().pbx_last_error().decode()
    return st, err


def test_plan_refusals():
    r = raws(1)[0]
    z = _zarr.zstd_frame(r, 3)
    g = Z3.gzip_member(r)
    assert plan_one(z, pbx.ZARR_ZSTD)[0] == 0 and plan_one(g, pbx.ZARR_GZIP)[0] == 0
    # zstd: content size != chunk bytes; trailing bytes; truncated; not a frame; skippable; dictionary id
    st, err = plan_one(_zarr.zstd_frame(r + b"ab", 3), pbx.ZARR_ZSTD)
    assert st == 400 and "content size" in err
    assert plan_one(z + b"\0", pbx.ZARR_ZSTD)[0] == 400
    assert plan_one(z + z, pbx.ZARR_ZSTD)[0] == 400
    assert plan_one(z[:-1], pbx.ZARR_ZSTD)[0] == 400
    assert plan_one(g, pbx.ZARR_ZSTD)[0] == 400
    st, err = plan_one(struct.pack("<II", 0x184D2A53, 4) + b"abcd", pbx.ZARR_ZSTD)
    assert st == 400 and "skippable" in err
    with_did = bytearray(z)
    with_did[4] |= 1
    st, err = plan_one(bytes(with_did), pbx.ZARR_ZSTD)
    assert st == 400 and "dictionary" in err
    # gzip: ISIZE != chunk bytes; reserved FLG bit; wrong magic / method; truncated header
    st, err = plan_one(Z3.gzip_member(r, isize=CB + 1), pbx.ZARR_GZIP)
    assert st == 400 and "ISIZE" in err
    st, err = plan_one(Z3.gzip_member(r + b"ab"), pbx.ZARR_GZIP)
    assert st == 400 and "ISIZE" in err
    for bit in (0x20, 0x40, 0x80):
        st, err = plan_one(Z3.gzip_member(r, flg_extra_bits=bit), pbx.ZARR_GZIP)
        assert st == 400 and "FLG" in err
    assert plan_one(zlib.compress(r), pbx.ZARR_GZIP)[0] == 400
    assert plan_one(g[:2] + b"\x07" + g[3:], pbx.ZARR_GZIP)[0] == 400
    assert plan_one(g[:12], pbx.ZARR_GZIP)[0] == 400
    assert plan_one(Z3.gzip_member(r, extra=b"x" * 40)[:30] + g[-8:], pbx.ZARR_GZIP)[0] == 400
    # the crc flag: a chunk shorter than 4 bytes
    for n in (1, 2, 3):
        st, err = plan_one(b"\1" * n, pbx.ZARR_RAW, pbx.ZARR_F_CRC32C)
        assert st == 400 and "crc32c" in err
    assert plan_one(Z3.with_crc32c(r), pbx.ZARR_RAW, pbx.ZARR_F_CRC32C)[0] == 0
    assert plan_one(Z3.with_crc32c(r)[:-1], pbx.ZARR_RAW, pbx.ZARR_F_CRC32C)[0] == 400  # raw bytes < chunk
    # codec 5, codec -1, unknown flag bits
    assert plan_one(r, 5)[0] == 400 and plan_one(r, -1)[0] == 400
    for flags in (2, 3, 4, 0x100, -2):
        st, err = plan_one(Z3.with_crc32c(r), pbx.ZARR_RAW, flags)
        assert st == 400 and "flags" in err


def test_python_layer_refuses_unknown_codec_names():
    with pytest.raises(pbx.PbxError) as ei:
        pbx.PixelsService.register_zarr_plane(None, 1, 0, 0, 0, pbx.UINT16, 8, 8, 8, 8, "lz4", [b""])
    assert ei.value.status == 400
