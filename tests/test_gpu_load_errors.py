"""What a source load says when a decoder or a checksum refuses a stream, where the other GPU
test files leave it open: the stream's index and kind in a call whose layers use several kinds
(the index counts the launch's streams kind by kind in the order of enum ZS_*, not plane by
plane), a checksum mismatch in such a call, the second of two JPEG and of two JPEG 2000 segment
streams, and the band-write entry points on a plane that is not sparse or not there.  Planes are
48 x 40 at most, chunks and segments 16 x 16; every refusal is a 400 (or 404) with the whole
message the library wrote."""
import itertools
import struct
import zlib

import numpy as np
import pytest

import _tiff_j2k as J2
import _tiff_jpeg as JP
import _zarr
import _zarr3 as Z3
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(9_700_000)  # disjoint from the other test files (shared service)

# pbx_decode_types.h, enum ZS_*: the order the streams of one launch are numbered in
KIND_ORDER = ["lz4", "zlib", "stored", "blosclz", "zstd", "gzip", "lzw"]
W, H, C = 48, 40, 16


def _plane(seed):
    """Compressible bytes (every chunk becomes Huffman blocks, not stored ones)."""
    y, x = np.mgrid[0:H, 0:W]
    return ((x * 3 + y * 5 + seed) % 64 + np.random.default_rng(seed).integers(0, 4, (H, W))).astype(np.uint8)


ENCODERS = {"zlib": lambda b: zlib.compress(b, 6), "zstd": lambda b: _zarr.zstd_frame(b, 3), "gzip": Z3.gzip_member}
_mixed = {}


def mixed():
    """codec -> (plane, its 3 x 3 chunks); made once and never changed."""
    if not _mixed:
        for seed, codec in enumerate(ENCODERS):
            a = _plane(seed)
            _mixed[codec] = (a, [ENCODERS[codec](c.tobytes()) for c in _zarr.chunk_grid(a, C, C)])
    return _mixed


def mixed_specs(images, chunks_of):
    """One register_zarr_planes call of three planes, gzip first: the call's order of planes is
    not the order of kinds."""
    return [dict(image_id=images[codec], z=0, c=0, t=0, pixel_type=pbx.UINT8, size_x=W, size_y=H, chunk_x=C, chunk_y=C,
                 codec=codec, chunks=chunks_of[codec], big_endian=False) for codec in ("gzip", "zlib", "zstd")]


def stream_index(kind, k, counts):
    """The launch-wide number of stream k of `kind`: the streams of the kinds before it first."""
    return sum(counts.get(n, 0) for n in KIND_ORDER[:KIND_ORDER.index(kind)]) + k


def damaged(stream, at):
    b = bytearray(stream)
    b[at] ^= 0x55
    return bytes(b)


def inflates(body):
    """zlib inflates the raw deflate data to one chunk and ends where the data ends."""
    try:
        d = zlib.decompressobj(-15)
        out = d.decompress(body)
        return d.eof and len(out) == C * C and not d.unused_data
    except zlib.error:
        return False


def test_mixed_kinds_register_and_decode(service):
    images = {codec: next(_ids) for codec in ENCODERS}
    ids = service.register_zarr_planes(mixed_specs(images, {c: v[1] for c, v in mixed().items()}))
    try:
        for pid, codec in zip(ids, ("gzip", "zlib", "zstd")):
            assert service.read_plane_be(pid, W * H) == mixed()[codec][0].tobytes(), codec
    finally:
        for pid in ids:
            service.release_plane(pid)


def test_corrupt_stream_is_named_by_kind_and_launch_wide_index(service):
    """One byte in the middle of the deflate data of the gzip layer's second chunk: the byte nearest
    the middle after whose change zlib itself cannot inflate the data to the chunk's 256 bytes, so
    that it is the decoder that refuses and not the trailer's CRC."""
    chunks = {c: list(v[1]) for c, v in mixed().items()}
    good = chunks["gzip"][1]
    assert good[3] == 0  # no optional header field: the deflate data is bytes 10 .. len - 8
    mid = 10 + (len(good) - 18) // 2
    bad = next(b for b in (damaged(good, mid + d) for d in (0, 1, -1, 2, -2, 3, -3, 4, -4)) if not inflates(b[10:-8]))
    chunks["gzip"][1] = bytes(bad)
    images = {codec: next(_ids) for codec in ENCODERS}
    s = stream_index("gzip", 1, {c: len(v) for c, v in chunks.items()})
    assert s == 9 + 9 + 1
    before = service.residency_stats()["resident_bytes"]
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_planes(mixed_specs(images, chunks))
    assert ei.value.status == 400
    msg = str(ei.value)
    assert "corrupt chunk stream %d (gzip, decoder code " % s in msg, msg
    assert all(service.lookup_plane(i, 0, 0, 0) is None for i in images.values())
    assert service.residency_stats()["resident_bytes"] == before


def test_checksum_mismatch_in_a_mixed_call(service):
    """Every stream intact; one bit of the CRC-32 in the trailer of the gzip layer's fifth chunk."""
    a, good = mixed()["gzip"]
    raw = _zarr.chunk_grid(a, C, C)[4].tobytes()
    given = struct.unpack("<I", good[4][-8:-4])[0] ^ 0x00010000
    chunks = {c: list(v[1]) for c, v in mixed().items()}
    chunks["gzip"][4] = Z3.gzip_member(raw, crc=given)
    images = {codec: next(_ids) for codec in ENCODERS}
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_planes(mixed_specs(images, chunks))
    assert ei.value.status == 400
    assert "chunk checksum mismatch: the gzip CRC-32 of %d bytes is not 0x%08x" % (C * C, given) in str(ei.value), str(ei.value)
    assert all(service.lookup_plane(i, 0, 0, 0) is None for i in images.values())


def tiff_spec(image, w, h, pixel_type, packed, **kw):
    return dict(image_id=image, z=0, c=0, t=0, pixel_type=pixel_type, size_x=w, size_y=h, big_endian=False, seg_w=C, seg_h=C,
                tiled=True, predictor=1, samples_per_pixel=1, sample=0, segments=packed, **kw)


def test_second_jpeg_segment_cut_short(service):
    """Two 16 x 16 baseline tiles; the second one's entropy-coded data ends half way."""
    pg = JP.kind_page("gray", JP.noise(2 * C, C, 41), tile=(C, C), quality=85, tables="segment")
    segs = list(pg["segments"])
    assert len(segs) == 2
    d = JP.header(segs[1])["data"]
    segs[1] = segs[1][:d + (len(segs[1]) - d) // 2]
    image = next(_ids)
    spec = tiff_spec(image, 2 * C, C, pbx.UINT8, pbx.pack_chunks(segs), compression=pbx.TIFF_JPEG,
                     jpeg=dict(tables=None, ycbcr=False))
    with pytest.raises(pbx.PbxError) as ei:
        service.register_tiff_planes([spec])
    assert ei.value.status == 400
    assert "corrupt segment stream 1 (jpeg, decoder code 1: entropy data ends before the last MCU)" in str(ei.value), \
        str(ei.value)
    assert service.lookup_plane(image, 0, 0, 0) is None


def test_second_j2k_segment_damaged(service):
    """Two 16 x 16 tiles; the second one's first packet header rewritten as test_gpu_tiff_j2k.py's
    "zero bit-planes above Mb" does: non-empty, included, then 46 zeros of the zero-bit-plane tag
    tree, more missing bit-planes than any band has (J2E_PLANES = 3)."""
    pg = J2.page_of(np.random.default_rng(43).integers(0, 65536, (C, 2 * C), dtype=np.uint16), tile=(C, C),
                    num_resolutions=3)
    segs = list(pg["segments"])
    assert len(segs) == 2
    hd = J2.parse(segs[1])
    bad = bytearray(segs[1])
    bad[hd["data"]] = 0xC0
    bad[hd["data"] + 1:hd["data"] + 6] = bytes(5)
    segs[1] = bytes(bad)
    image = next(_ids)
    spec = tiff_spec(image, 2 * C, C, pbx.UINT16, pbx.pack_chunks(segs), compression=pbx.TIFF_J2K, j2k=True)
    with pytest.raises(pbx.PbxError) as ei:
        service.register_tiff_planes([spec])
    assert ei.value.status == 400
    assert "corrupt segment stream 1 (j2k, decoder code 3)" in str(ei.value), str(ei.value)
    assert service.lookup_plane(image, 0, 0, 0) is None


def test_band_write_on_a_plane_that_is_not_sparse_or_not_there(service):
    image, other = next(_ids), next(_ids)
    pid = service.register_plane(image, 0, 0, 0, pbx.UINT8, W, H, generator="noise", seed=5)
    oid = service.register_plane(other, 0, 0, 0, pbx.UINT8, W, H, generator="noise", seed=6)
    try:
        st, tile = service.get_tile(pbx.TileCtx(other, 0, 0, 0, 0, 0, W, H))
        assert st == pbx.OK
        seg = pbx.pack_chunks([bytes(C * C)] * 3)
        with pytest.raises(pbx.PbxError) as ei:
            service.band_write_tiff(pid, 0, C, C, C, True, 1, 1, seg)
        assert ei.value.status == 400 and "plane %d is not a sparse plane" % pid in str(ei.value), str(ei.value)
        assert service.get_tile(pbx.TileCtx(other, 0, 0, 0, 0, 0, W, H)) == (pbx.OK, tile)
        missing = 1 << 62
        with pytest.raises(pbx.PbxError) as ei:
            service.band_write_tiff(missing, 0, C, C, C, True, 1, 1, seg)
        assert ei.value.status == 404 and "no plane %d" % missing in str(ei.value), str(ei.value)
        assert service.get_tile(pbx.TileCtx(other, 0, 0, 0, 0, 0, W, H)) == (pbx.OK, tile)
        assert service.get_tile(pbx.TileCtx(image, 0, 0, 0, 0, 0, W, H))[0] == pbx.OK  # and its pin went back
        service.release_plane(pid)
        pid = None
        assert service.lookup_plane(image, 0, 0, 0) is None
    finally:
        for p in (pid, oid):
            if p is not None:
                service.release_plane(p)
