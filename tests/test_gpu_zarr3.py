"""Zarr v3 (NGFF 0.5) on the GPU: the checksum kernel (k_zarr_crc) through raw chunks under the
crc32c flag, whole-chunk gzip and zstd, the flag with zstd and blosc, sharded arrays (index at
either end, permuted and missing inner chunks, a missing shard, deep inner chunks), the on-demand
path through NgffSource, an NGFF 0.5 multiscale group, and the two new v2 compressor ids.

The expected plane is always the numpy array the chunks were written from (tests/_zarr3.py),
read back with plane_read_be or as raw tiles; every comparison is byte-exact."""
import itertools
import json
import os
import struct

import numpy as np
import pytest

import _zarr
import _zarr3 as Z3
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(1700000)  # disjoint from the other test files (shared service)


def register(service, plane, cy, cx, codec, chunks, **kw):
    """Register the chunks of a 2-D plane under a fresh image id; returns (image id, plane id)."""
    iid = next(_ids)
    dt = plane.dtype
    pid = service.register_zarr_plane(iid, 0, 0, 0, pbx._ZARR_DTYPES[dt.str[1:]], plane.shape[1], plane.shape[0],
                                      cx, cy, codec, chunks, big_endian=dt.str[0] != "<", **kw)
    return iid, pid


def be(plane):
    return np.ascontiguousarray(plane).astype(plane.dtype.newbyteorder(">")).tobytes()


def check_ok(service, plane, cy, cx, codec, chunks, **kw):
    iid, pid = register(service, plane, cy, cx, codec, chunks, **kw)
    try:
        assert service.read_plane_be(pid, plane.nbytes) == be(plane)
    finally:
        service.release_plane(pid)


def check_400(service, plane, cy, cx, codec, chunks, word=None, **kw):
    with pytest.raises(pbx.PbxError) as ei:
        register(service, plane, cy, cx, codec, chunks, **kw)
    assert ei.value.status == 400
    if word:
        assert word in str(ei.value), str(ei.value)


def encoded(plane, cy, cx, enc):
    return [enc(c.tobytes()) for c in _zarr.chunk_grid(plane, cy, cx)]


# ------------------------------------------------------------------- k_zarr_crc alone
LENGTHS = [1, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097, 65536 + 5]
BIG = (1 << 20) + 3
SPLIT = [(1 << 17) - 1, 1 << 17]  # the last range a wave takes and the first a workgroup takes
_crc_cases = {}


def crc_case(dtype):
    """A one-row plane of 1 x 1 chunks (raw chunks may be longer than the chunk: the rest of the
    file is ignored by the placement but covered by its checksum).  Chunk k's file is a payload
    of one of LENGTHS and its crc32c; filler chunks between them move the next start, so that
    every length begins at every offset mod 16.  The two lengths either side of the kernel's
    wave / workgroup split and one chunk of BIG bytes follow.  A 2-byte sample does not fit a
    1-byte chunk: that dtype takes length 2 in its place.  Made once per dtype and never
    changed."""
    if dtype not in _crc_cases:
        item = np.dtype(dtype).itemsize
        rng = np.random.default_rng(11 + item)
        lengths = [max(n, item) for n in LENGTHS]
        files, pos, starts = [], 0, {}

        def add(n):
            nonlocal pos
            payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            files.append(Z3.with_crc32c(payload))
            pos += n + 4

        for n in lengths:
            for r in range(16):
                if pos % 16 != r:  # a filler whose file moves the next start to residue r
                    need = (r - pos - 4) % 16
                    add(need if need >= item else need + 16)
                assert pos % 16 == r
                starts.setdefault(n, set()).add(pos % 16)
                add(n)
        for n in SPLIT:
            add(n)
        add(BIG)
        assert all(v == set(range(16)) for v in starts.values())
        plane = np.array([[int.from_bytes(f[:item], "little") for f in files]], dtype="<" + dtype[-2:])
        _crc_cases[dtype] = (plane, files)
    return _crc_cases[dtype]


@pytest.mark.parametrize("dtype", ["u1", "<u2"])
def test_crc_kernel_every_length_at_every_alignment(service, dtype):
    plane, files = crc_case(dtype)
    check_ok(service, plane, 1, 1, None, files, crc32c=True)


def flipped(files, k, byte, bit=0):
    out = list(files)
    b = bytearray(out[k])
    b[byte] ^= 1 << bit
    out[k] = bytes(b)
    return out


@pytest.mark.parametrize("dtype", ["u1", "<u2"])
def test_crc_kernel_flipped_bits_are_400_then_a_clean_register_succeeds(service, dtype):
    plane, files = crc_case(dtype)
    iid = next(_ids)
    pt = pbx._ZARR_DTYPES[dtype[-2:]]
    n = len(files)
    by_len = {}
    for k, f in enumerate(files):
        by_len.setdefault(len(f) - 4, k)
    # one-wave ranges and workgroup ranges; first, middle and last payload byte; each checksum byte
    cases = []
    for length in (max(1, np.dtype(dtype).itemsize), 17, 257, 4097, 65536 + 5, SPLIT[0], SPLIT[1], BIG):
        k = by_len[length]
        cases += [(k, 0, 0), (k, length // 2, 7), (k, length - 1, 3), (k, length, 0), (k, length + 3, 7)]
    for k, byte, bit in cases:
        with pytest.raises(pbx.PbxError) as ei:
            service.register_zarr_plane(iid, 0, 0, 0, pt, n, 1, 1, 1, None, flipped(files, k, byte, bit),
                                        big_endian=False, crc32c=True)
        assert ei.value.status == 400 and "checksum" in str(ei.value), (k, byte, bit)
        assert service.lookup_plane(iid, 0, 0, 0) is None  # nothing registered
    pid = service.register_zarr_plane(iid, 0, 0, 0, pt, n, 1, 1, 1, None, files, big_endian=False, crc32c=True)
    try:
        assert service.read_plane_be(pid, plane.nbytes) == be(plane)
    finally:
        service.release_plane(pid)


def test_crc_flag_on_a_band_leaves_the_band_as_it_was(service):
    """A mismatch fails the band's load like a decoder error; the same rows then load clean."""
    plane = _zarr.noise_plane(64, 96, "<u2", seed=5)
    files = [Z3.with_crc32c(c.tobytes()) for c in _zarr.chunk_grid(plane, 32, 48)]
    iid = next(_ids)
    pid = service.create_sparse_plane(iid, 0, 0, 0, pbx.UINT16, 96, 64, 32, big_endian=False)
    try:
        with pytest.raises(pbx.PbxError) as ei:
            service.band_write_zarr(pid, 32, 32, 48, 32, None, flipped(files[2:], 1, 100), crc32c=True)
        assert ei.value.status == 400
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_ABSENT]
        service.band_write_zarr(pid, 32, 32, 48, 32, None, files[2:], crc32c=True)
        service.band_write_zarr(pid, 0, 32, 48, 32, None, files[:2], crc32c=True)
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 0, 96, 64))
        assert st == pbx.OK and body == be(plane)
    finally:
        service.release_plane(pid)


# ------------------------------------------------------------------------------- gzip
@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("chunk,shape", [((64, 96), (150, 200)), ((300, 300), (300, 500))], ids=["96x64", "300x300"])
def test_gzip_chunks(service, chunk, shape, level):
    plane = _zarr.noise_plane(shape[0], shape[1], ">u2", seed=level)
    check_ok(service, plane, chunk[0], chunk[1], "gzip",
             encoded(plane, chunk[0], chunk[1], lambda b: Z3.gzip_member(b, level)))


def test_gzip_header_fields_and_stored_blocks(service):
    plane = _zarr.noise_plane(300, 500, "<u2", seed=3)
    check_ok(service, plane, 300, 300, "gzip", encoded(plane, 300, 300, lambda b: Z3.gzip_member(
        b, 6, fname=b"0.0", extra=b"zz\x03\x00abc", fhcrc=True)))
    check_ok(service, plane, 300, 300, "gzip", encoded(plane, 300, 300, lambda b: Z3.gzip_member(
        b, 6, fname=b"name", comment=b"comment")))
    check_ok(service, plane, 300, 300, "gzip", encoded(plane, 300, 300, lambda b: Z3.gzip_member(b, 0)))  # stored


def test_gzip_refusals(service):
    plane = _zarr.noise_plane(64, 192, ">u2", seed=8)
    good = encoded(plane, 64, 96, Z3.gzip_member)
    raw1 = _zarr.chunk_grid(plane, 64, 96)[1].tobytes()
    check_ok(service, plane, 64, 96, "gzip", good)
    bad_crc = Z3.gzip_member(raw1, crc=(struct.unpack("<I", good[1][-8:-4])[0] ^ 0x100))
    check_400(service, plane, 64, 96, "gzip", [good[0], bad_crc], "checksum")
    # one flipped bit of the decoded data: a literal byte of a stored member
    stored = bytearray(Z3.gzip_member(raw1, 0))
    stored[10 + 5 + 1000] ^= 4
    check_400(service, plane, 64, 96, "gzip", [good[0], bytes(stored)], "checksum")
    check_400(service, plane, 64, 96, "gzip", [good[0], Z3.gzip_member(raw1, isize=len(raw1) - 2)], "ISIZE")
    # a second member: its ISIZE is right, its deflate data does not end 8 bytes before the end
    check_400(service, plane, 64, 96, "gzip", [good[0], good[1] + good[1]], "gzip")
    # 3 trailing bytes: whatever the last 8 bytes then say, the chunk is refused
    check_400(service, plane, 64, 96, "gzip", [good[0], good[1] + b"\0\0\0"])
    moved = good[1] + good[1][-8:]  # ... also when they repeat a valid trailer
    check_400(service, plane, 64, 96, "gzip", [good[0], moved], "gzip")
    check_400(service, plane, 64, 96, "gzip", [good[0], good[1][:-9] + good[1][-8:]])  # a byte of data lost


# ------------------------------------------------------------------------------- zstd
def test_zstd_chunks_of_several_blocks(service):
    plane = _zarr.noise_plane(300, 500, ">u2", seed=21)
    chunks = encoded(plane, 300, 300, lambda b: _zarr.zstd_frame(b, 3))
    assert len(chunks[0]) > 3 and 300 * 300 * 2 > 128 * 1024  # more than one block per frame
    check_ok(service, plane, 300, 300, "zstd", chunks)


def test_zstd_matches_beyond_128k_rle_and_raw_blocks(service):
    half = _zarr.noise_plane(256, 300, "<u2", seed=4)
    plane = np.concatenate([half, half])  # 512 x 300: the second 150 KiB repeat the first
    frame = _zarr.zstd_frame(plane.tobytes(), 3)
    assert len(frame) < 0.6 * len(_zarr.zstd_frame(half.tobytes(), 3)) * 2  # the repeat was found
    check_ok(service, plane, 512, 300, "zstd", [frame])
    const = np.full((300, 300), 0x1234, "<u2")
    check_ok(service, const, 300, 300, "zstd", [_zarr.zstd_frame(const.tobytes(), 3)])
    noise = np.random.default_rng(2).integers(0, 65536, (300, 300)).astype("<u2")
    f = _zarr.zstd_frame(noise.tobytes(), 3)
    assert len(f) >= noise.nbytes  # raw blocks
    check_ok(service, noise, 300, 300, "zstd", [f])


def test_zstd_content_checksum_and_sizes(service):
    plane = _zarr.noise_plane(96, 200, ">u2", seed=6)
    chunks = encoded(plane, 96, 100, lambda b: _zarr.zstd_frame(b, 3, checksum=True))
    check_ok(service, plane, 96, 100, "zstd", chunks)
    check_400(service, plane, 96, 100, "zstd", flipped(chunks, 1, len(chunks[1]) - 2, 5), "zstd")
    raw = _zarr.chunk_grid(plane, 96, 100)
    # a frame for another size: refused by the host when the header says so ...
    wrong = _zarr.zstd_frame(raw[1].tobytes()[:-2], 3)
    check_400(service, plane, 96, 100, "zstd", [chunks[0], wrong], "content size")
    nosize = [Z3.zstd_frame_nosize(c.tobytes()) for c in raw]
    if None in nosize:
        pytest.skip("this libzstd writes a content size whatever ZSTD_c_contentSizeFlag says")
    check_ok(service, plane, 96, 100, "zstd", nosize)
    # ... and by the decoder's length check when it does not
    check_400(service, plane, 96, 100, "zstd", [nosize[0], Z3.zstd_frame_nosize(raw[1].tobytes()[:-2])], "zstd")
    check_400(service, plane, 96, 100, "zstd", [chunks[0], chunks[1] + b"\0"])  # bytes after the frame


def test_crc_flag_with_zstd_and_blosc(service):
    plane = _zarr.noise_plane(150, 200, ">u2", seed=9)
    for codec, enc in (("zstd", lambda b: _zarr.zstd_frame(b, 3)), ("blosc", lambda b: _zarr.blosc_encode(b, 2)),
                       ("gzip", Z3.gzip_member), ("zlib", _zarr.zlib_encode)):
        chunks = encoded(plane, 64, 96, lambda b: Z3.with_crc32c(enc(b)))
        check_ok(service, plane, 64, 96, codec, chunks, crc32c=True)
        check_400(service, plane, 64, 96, codec, flipped(chunks, 4, len(chunks[4]) - 1), "checksum", crc32c=True)
        check_400(service, plane, 64, 96, codec, flipped(chunks, 4, 20), crc32c=True)


# ----------------------------------------------------------------------------- shards
H, W = 600, 500
SHARD, INNER = (256, 256), (64, 64)
MISSING = {(0, 1), (3, 3), (4, 7), (9, 0)}  # inner chunks (64 x 64) left out
MISSING_SHARD = (1, 1)                      # rows 256..511, columns 256..499
ENC_KW = {"zstd": {}, "gzip": {"level": 5}, "blosc": {"codec": "lz4", "clevel": 5, "shuffle": True}}


def with_fill(arr, fill=9):
    """arr with the missing inner chunks and the missing shard set to the fill value."""
    out = arr.copy()
    for j, i in MISSING:
        out[..., j * 64:(j + 1) * 64, i * 64:(i + 1) * 64] = fill
    sj, si = MISSING_SHARD
    out[..., sj * 256:(sj + 1) * 256, si * 256:(si + 1) * 256] = fill
    return out


def shuffled(ks):
    return list(np.random.default_rng(len(ks)).permutation(ks))


_arr2d = None


def plane2d():
    global _arr2d
    if _arr2d is None:
        _arr2d = _zarr.noise_plane(H, W, ">u2", seed=17)
    return _arr2d


@pytest.mark.parametrize("loc", ["end", "start"])
@pytest.mark.parametrize("codec", ["zstd", "gzip", "blosc"])
def test_sharded_array(service, tmp_path, codec, loc):
    arr = plane2d()
    adir = str(tmp_path / "a")
    Z3.write_array(adir, arr, INNER, codec, crc=(loc == "start"), shard=SHARD, index_location=loc,
                   permute=shuffled, missing=MISSING, missing_shards={MISSING_SHARD}, fill_value=9,
                   endian="little" if codec == "gzip" else "big", enc_kw=ENC_KW[codec])
    iid = next(_ids)
    pid = service.register_zarr_array(adir, iid, 0, 0, 0)
    try:
        assert service.read_plane_be(pid, arr.nbytes) == be(with_fill(arr))
    finally:
        service.release_plane(pid)


def test_sharded_array_with_a_corrupt_inner_chunk_is_400(service, tmp_path):
    arr = plane2d()
    adir = str(tmp_path / "a")
    Z3.write_array(adir, arr, INNER, "zstd", crc=True, shard=SHARD)
    path = os.path.join(adir, "c", "1", "0")
    data = bytearray(open(path, "rb").read())
    data[1000] ^= 1
    open(path, "wb").write(bytes(data))
    iid = next(_ids)
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_array(adir, iid, 0, 0, 0)
    assert ei.value.status == 400 and "checksum" in str(ei.value)
    assert service.lookup_plane(iid, 0, 0, 0) is None


def test_shard_with_deep_inner_chunks(service, tmp_path):
    arr = np.stack([_zarr.noise_plane(H, W, ">u2", seed=s) for s in (1, 2, 3)]).reshape(1, 1, 3, H, W)
    adir = str(tmp_path / "a")
    Z3.write_array(adir, arr, (1, 1, 2, 64, 64), "zstd", shard=(1, 1, 2, 256, 256), permute=shuffled,
                   missing={(0, 0) + (1,) + m for m in MISSING}, fill_value=9)
    iid = next(_ids)
    ids = service.register_zarr_array_planes(adir, iid)
    try:
        assert sorted(ids) == [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
        for z in range(3):
            want = arr[0, 0, z]
            if z >= 2:  # the second deep chunk along z holds the missing ones
                want = want.copy()
                for j, i in MISSING:
                    want[j * 64:(j + 1) * 64, i * 64:(i + 1) * 64] = 9
            assert service.read_plane_be(ids[(z, 0, 0)], want.nbytes) == be(want), z
    finally:
        for pid in ids.values():
            service.release_plane(pid)


# ------------------------------------------------------------------- on demand, NGFF 0.5
def write_image(root, levels, codec="zstd", **kw):
    """An NGFF 0.5 image: a v3 group with "ome" multiscales over one sharded array per level."""
    Z3.write_group(root, {"version": "0.5", "multiscales": [{
        "axes": [{"name": "y", "type": "space"}, {"name": "x", "type": "space"}],
        "datasets": [{"path": "s%d" % k} for k in range(len(levels))]}]})
    for k, a in enumerate(levels):
        Z3.write_array(os.path.join(root, "s%d" % k), a, INNER, codec, shard=SHARD, enc_kw=ENC_KW[codec], **kw)


def test_ngff_source_serves_a_sharded_array_on_demand(oracle, tmp_path, monkeypatch):
    arr = plane2d()
    root = str(tmp_path / "img")
    write_image(root, [arr], "zstd", crc=True, permute=shuffled, missing=MISSING, fill_value=9)
    want = arr.copy()
    for j, i in MISSING:
        want[j * 64:(j + 1) * 64, i * 64:(i + 1) * 64] = 9
    opened = []
    real = pbx._read_chunk_file
    monkeypatch.setattr(pbx, "_read_chunk_file", lambda p: (opened.append(os.path.relpath(p, root)), real(p))[1])
    iid = next(_ids)
    src = pbx.NgffSource({iid: root})
    with pbx.PixelsService(sparse_band_rows=128) as svc:
        # rows 200..299 lie in bands 1 and 2 (rows 128..383) = shard rows 0 and 1; columns 200..319
        # cross the shard boundary at 256
        tc = pbx.TileCtx(iid, 0, 0, 0, 200, 200, 120, 100)
        assert pbx.TileRequestHandler(svc, tc, src).get_tile() == want[200:300, 200:320].tobytes()
        # band 1 (rows 128..255) needs shard row 0, band 2 (rows 256..383) shard row 1: each file once per band
        assert sorted(opened) == sorted(["s0/c/0/0", "s0/c/0/1", "s0/c/1/0", "s0/c/1/1"])
        tc = pbx.TileCtx(iid, 0, 0, 0, 0, 500, W, 100, format="tif")  # bands 3 and 4: shard rows 1 and 2
        r, px, _ = oracle.tiff_decode(pbx.TileRequestHandler(svc, tc, src).get_tile(), W * 100 * 2)
        assert r == 0 and px == want[500:600].tobytes()
        assert sorted(opened[4:]) == sorted(["s0/c/1/0", "s0/c/1/1", "s0/c/2/0", "s0/c/2/1"])
        tc = pbx.TileCtx(iid, 0, 0, 0, 250, 250, 12, 12)  # all four shards' corner, bands resident
        assert pbx.TileRequestHandler(svc, tc, src).get_tile() == want[250:262, 250:262].tobytes()
        assert len(opened) == 8


def test_register_ngff_05_image_with_two_levels(service, tmp_path):
    full = plane2d()
    half = _zarr.noise_plane(300, 250, ">u2", seed=23)
    root = str(tmp_path / "img")
    write_image(root, [full, half], "gzip", index_location="start")
    iid = next(_ids)
    ids = service.register_ngff_image(root, iid)
    try:
        assert sorted(ids) == [0, 1] and all(list(v) == [(0, 0, 0)] for v in ids.values())
        # OMERO numbering: resolution 1 = full, 0 = the smaller level
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 230, 240, 60, 40, resolution=1))
        assert st == pbx.OK and body == full[240:280, 230:290].tobytes()
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 100, 250, 150, 50, resolution=0))
        assert st == pbx.OK and body == half[250:300, 100:250].tobytes()
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 0, 16, 16))  # no resolution: full
        assert st == pbx.OK and body == full[:16, :16].tobytes()
    finally:
        for v in ids.values():
            for pid in v.values():
                service.release_plane(pid)


def test_v2_zarray_with_the_zstd_compressor(service, tmp_path):
    plane = _zarr.noise_plane(150, 200, "<u2", seed=31)
    d = tmp_path / "a"
    d.mkdir()
    (d / ".zarray").write_text(json.dumps({
        "zarr_format": 2, "shape": [150, 200], "chunks": [64, 96], "dtype": "<u2", "order": "C",
        "fill_value": 0, "filters": None, "compressor": {"id": "zstd", "level": 3}}))
    for k, c in enumerate(_zarr.chunk_grid(plane, 64, 96)):
        (d / ("%d.%d" % divmod(k, 3))).write_bytes(_zarr.zstd_frame(c.tobytes(), 3))
    iid = next(_ids)
    pid = service.register_zarr_array(str(d), iid, 0, 0, 0)
    try:
        assert service.read_plane_be(pid, plane.nbytes) == be(plane)
    finally:
        service.release_plane(pid)
