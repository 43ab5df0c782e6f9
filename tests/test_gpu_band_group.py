"""Band writes that span planes (pbx_band_write_tiff_group, pbx_band_write_zarr_group) and
PixelsService(fill_siblings=True): one upload and decode fills the bands of every plane that
shares the segments or chunks.

Every expected value is the bytes of a registration of the same segments or chunks, or the numpy
array they were built from (both pinned against PIL / libtiff by the host tests); every comparison
is byte for byte.  Shapes are the smallest that cut segments: the chunky cases are the one-sample
band test's 21 x 65 image (tests/test_gpu_tiff_rgb.py), a one-band sparse plane per sample with
sentinel rows 0 .. 6 and 14 .. 20 around two pieces, [7, 10) and [10, 14), that begin and end inside
a segment."""
import ctypes
import itertools
import json
import os
import threading

import numpy as np
import pytest

import _tiff_j2k as J2
import _tiff_j2k_chroma as C
import _tiff_jpeg as J
import _tiff_packed as K
import _tiff_rgb as R
import _values as V
import _zarr_deep as ZD
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(13_700_000)  # disjoint from the other test files (shared service)
HERE = os.path.dirname(os.path.abspath(__file__))
OK, ABSENT, LOADING, READY = pbx.OK, pbx.BS_ABSENT, pbx.BS_LOADING, pbx.BS_READY
H, W = 21, 65
LOW, HIGH = b"\xA5", b"\x5A"


# ------------------------------------------------------------------------------ helpers
def be_bytes(a):
    return np.ascontiguousarray(a).astype(a.dtype.newbyteorder(">")).tobytes()


def rows_of(svc, image, y0, rows, w, c=0):
    st, body = svc.get_tile(pbx.TileCtx(image, 0, c, 0, 0, y0, w, rows))
    assert st == pbx.OK, st
    return body


def full_range(pt, w, h, S, bo, seed):
    """(h, w, S) samples of uniform random bits, in the file's byte order (as tests/test_gpu_tiff_rgb.py)."""
    a = V.random_bits(pt, w * S, h, seed).reshape(h, w, S)
    return a.astype(a.dtype.newbyteorder(bo)) if a.dtype.itemsize > 1 else a


def chunky(a, pt, bo, tile, rps, comp, predictor):
    """(the segments of a chunky layer as a list, the keywords every call on them shares)."""
    h, w, S = a.shape
    segs = [R.compress(x, comp) for x in R.chunky_segments(a, tile, rps, predictor)]
    return segs, dict(pixel_type=pt, size_x=w, size_y=h, big_endian=bo == ">", seg_w=tile[0] if tile else w,
                      seg_h=tile[1] if tile else rps, tiled=tile is not None, compression=comp, predictor=predictor)


def specs_from(segs, base, image, S, **extra):
    """register_tiff_planes specs of all S samples, sharing one segments object."""
    packed = pbx.pack_chunks(segs)
    return [dict(base, image_id=image, z=0, c=s, t=0, segments=packed, samples_per_pixel=S, sample=s, **extra)
            for s in range(S)]


def piece(segs, base, y0, rows):
    """The segment rows that cover rows [y0, y0 + rows), as a list."""
    gx = -(-base["size_x"] // base["seg_w"]) if base["tiled"] else 1
    return segs[(y0 // base["seg_h"]) * gx:-(-(y0 + rows) // base["seg_h"]) * gx]


def group_write(svc, ids, primary, segs, base, y0, rows, **kw):
    return svc.band_write_tiff_group(ids, primary, y0, rows, base["seg_w"], base["seg_h"], base["tiled"],
                                     base["compression"], base["predictor"], piece(segs, base, y0, rows), **kw)


def sparse_planes(svc, image, S, base, band_rows=None):
    return [svc.create_sparse_plane(image, 0, c, 0, base["pixel_type"], base["size_x"], base["size_y"],
                                    band_rows or base["size_y"], big_endian=base["big_endian"]) for c in range(S)]


def row_bytes(base):
    return base["size_x"] * pbx.BYTES_PER_PIXEL[base["pixel_type"]]


def sentinels(svc, pid, base, lo, hi):
    """Rows [0, lo) and [hi, size_y) of a one-band plane from band_write."""
    row, h = row_bytes(base), base["size_y"]
    svc.band_write(pid, 0, lo, LOW * (lo * row))
    svc.band_write(pid, hi, h - hi, HIGH * ((h - hi) * row))


def check_window(svc, image, c, base, lo, hi, want):
    """Plane c: the sentinel rows as they were, rows [lo, hi) those of `want` (the whole plane's bytes)."""
    row, h = row_bytes(base), base["size_y"]
    got = rows_of(svc, image, 0, h, base["size_x"], c=c)
    assert got[:lo * row] == LOW * (lo * row) and got[hi * row:] == HIGH * ((h - hi) * row), c
    assert got[lo * row:hi * row] == want[lo * row:hi * row], c


def registered(svc, specs):
    """The planes' bytes as a registration of the same segments stores them."""
    ids = svc.register_tiff_planes(specs)
    try:
        return [svc.read_plane_be(pid, sp["size_x"] * sp["size_y"] * pbx.BYTES_PER_PIXEL[sp["pixel_type"]])
                for pid, sp in zip(ids, specs)]
    finally:
        for pid in ids:
            svc.release_plane(pid)


def release(svc, pids):
    for pid in pids:
        svc.release_plane(pid)


# ------------------------------------------------------------------------------ 1. chunky samples
@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("comp", [pbx.TIFF_NONE, pbx.TIFF_LZW, pbx.TIFF_DEFLATE], ids=["stored", "lzw", "deflate"])
@pytest.mark.parametrize("tile", [None, (16, 16)], ids=["strips", "tiles"])
@pytest.mark.parametrize("kind,pt", [("u1", pbx.UINT8), ("u2", pbx.UINT16)], ids=["u8", "u16"])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_chunky_samples(service, S, kind, pt, tile, comp, predictor):
    """Every primary, with all samples wanted and with one id 0 (that sample's plane, all sentinel
    from band_write, stays as it was and its status is -1)."""
    a = full_range(pt, W, H, S, ">", 60 + 10 * S + predictor)
    segs, base = chunky(a, pt, ">", tile, 4, comp, predictor)
    want = registered(service, specs_from(segs, base, next(_ids), S))
    assert want == [be_bytes(a[:, :, s]) for s in range(S)]
    row = row_bytes(base)
    for primary in range(S):
        for skip in (None, (primary + 1) % S):
            image = next(_ids)
            pids = sparse_planes(service, image, S, base)
            try:
                for c in range(S):
                    if c == skip:
                        service.band_write(pids[c], 0, H, bytes([0x30 + c]) * (H * row))
                    else:
                        sentinels(service, pids[c], base, 7, 14)
                ids = [0 if c == skip else pids[c] for c in range(S)]
                for y0, rows in ((7, 3), (10, 4)):
                    st, ms = group_write(service, ids, primary, segs, base, y0, rows)
                    assert st == [-1 if c == skip else OK for c in range(S)] and len(ms) == 2
                for c in range(S):
                    assert service.band_info(pids[c])[1] == [READY]
                    if c == skip:
                        assert rows_of(service, image, 0, H, W, c=c) == bytes([0x30 + c]) * (H * row)
                    else:
                        check_window(service, image, c, base, 7, 14, want[c])
            finally:
                release(service, pids)


# ------------------------------------------------------------------------------ 2. JPEG
@pytest.mark.parametrize("kind", ["420", "444"])
def test_jpeg(service, kind):
    """16 x 16 tiles, two tile rows, 37 columns; the window [5, 27) begins and ends inside a tile row."""
    w, h = 37, 30
    pg = J.kind_page(kind, J.noise(w, h, 29), tile=(16, 16), quality=85)
    tabs = next((bytes(t[2]) for t in pg["extra"] if t[0] == 347), None)
    jpeg = dict(tables=tabs, ycbcr=pg["photometric"] == 6)
    base = dict(pixel_type=pbx.UINT8, size_x=w, size_y=h, big_endian=False, seg_w=16, seg_h=16, tiled=True,
                compression=pbx.TIFF_JPEG, predictor=1)
    segs = list(pg["segments"])
    want = registered(service, specs_from(segs, base, next(_ids), 3, jpeg=jpeg))
    model = J.decode_page(pg)
    assert want == [model[:, :, c].tobytes() for c in range(3)]
    for primary in range(3):
        image = next(_ids)
        pids = sparse_planes(service, image, 3, base)
        try:
            for pid in pids:
                sentinels(service, pid, base, 5, 27)
            st, _ = group_write(service, pids, primary, segs, base, 5, 22, jpeg=jpeg)
            assert st == [OK] * 3
            for c in range(3):
                assert service.band_info(pids[c])[1] == [READY]
                check_window(service, image, c, base, 5, 27, want[c])
        finally:
            release(service, pids)


# ------------------------------------------------------------------------------ 3. JPEG 2000
def test_j2k_lossless_rgb_with_the_colour_transform(service):
    w, h = 70, 50
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    pg = J2.page_of(a, tile=(32, 32), mct=1, num_resolutions=3)
    base = dict(pixel_type=pbx.UINT8, size_x=w, size_y=h, big_endian=False, seg_w=32, seg_h=32, tiled=True,
                compression=pbx.TIFF_J2K, predictor=1)
    segs = list(pg["segments"])
    want = registered(service, specs_from(segs, base, next(_ids), 3, j2k=True))
    assert want == [a[:, :, c].tobytes() for c in range(3)]
    for primary in (0, 2):
        image = next(_ids)
        pids = sparse_planes(service, image, 3, base)
        try:
            for pid in pids:
                sentinels(service, pid, base, 9, 41)
            st, _ = group_write(service, pids, primary, segs, base, 9, 32, j2k=True)
            assert st == [OK] * 3
            for c in range(3):
                assert service.band_info(pids[c])[1] == [READY]
                check_window(service, image, c, base, 9, 41, want[c])
        finally:
            release(service, pids)


@pytest.mark.parametrize("ycc", [False, True], ids=["as stored", "to RGB"])
def test_j2k_subsampled_chroma(service, ycc):
    """A 4:2:0 page through k_tiff_j2k_place_chroma, with and without the YCbCr conversion."""
    w, h = 70, 50
    flags = pbx.TIFF_F_J2K_SUBSAMPLED | (pbx.TIFF_F_J2K_YCBCR if ycc else 0)
    pg = C.page_of(C.ycc_smooth(w, h, 33), 2, 2, tile=(32, 32), num_resolutions=3)
    base = dict(pixel_type=pbx.UINT8, size_x=w, size_y=h, big_endian=False, seg_w=32, seg_h=32, tiled=True,
                compression=pbx.TIFF_J2K, predictor=1)
    segs = list(pg["segments"])
    want = registered(service, specs_from(segs, base, next(_ids), 3, j2k=True, flags=flags))
    planes = C.page_planes(pg, ycc)
    assert want == [np.ascontiguousarray(planes[:, :, c]).tobytes() for c in range(3)]
    image = next(_ids)
    pids = sparse_planes(service, image, 3, base)
    try:
        for pid in pids:
            sentinels(service, pid, base, 9, 41)
        st, _ = group_write(service, pids, 1, segs, base, 9, 32, j2k=True, flags=flags)
        assert st == [OK] * 3
        for c in range(3):
            assert service.band_info(pids[c])[1] == [READY]
            check_window(service, image, c, base, 9, 41, want[c])
    finally:
        release(service, pids)


# ------------------------------------------------------------------------------ 4. packed
def test_packed_4_bit_samples_in_strips(service):
    S, bits, w, h, rps = 3, 4, 41, 17, 7
    a = K.noise(np.random.default_rng(35), h, w, bits, S)
    segs = [K.compress(x, 1) for x in K.segments_of(a, bits, None, rps, 1, 1, "<")]
    base = dict(pixel_type=pbx.UINT8, size_x=w, size_y=h, big_endian=False, seg_w=w, seg_h=rps, tiled=False,
                compression=1, predictor=1)
    packed = dict(bits=bits, fill_order=1)
    want = registered(service, specs_from(segs, base, next(_ids), S, packed=packed))
    assert want == [K.expected_be(a[:, :, c], bits) for c in range(S)]
    for primary in range(S):
        image = next(_ids)
        pids = sparse_planes(service, image, S, base)
        try:
            for pid in pids:
                sentinels(service, pid, base, 5, 12)
            for y0, rows in ((5, 4), (9, 3)):
                st, _ = group_write(service, pids, primary, segs, base, y0, rows, packed=packed)
                assert st == [OK] * S
            for c in range(S):
                assert service.band_info(pids[c])[1] == [READY]
                check_window(service, image, c, base, 5, 12, want[c])
        finally:
            release(service, pids)


# ------------------------------------------------------------------------------ 5. Zarr
ZH, ZW, ZCH = 70, 100, (1, 3, 1, 40, 72)
ZCODECS = {"blosc-lz4": ("blosc", {"codec": "lz4", "shuffle": True, "blocksize": 4096}), "raw": (None, {})}


@pytest.fixture(scope="module")
def channels():
    """A (1, 3, 1, 70, 100) uint16 array in chunks that hold its three channels, and its chunk
    files (2 x 2 of them) per codec."""
    arr = ZD.noise_array((1, 3, 1, ZH, ZW), ">u2", seed=37)
    cut = ZD.cut_chunks(arr, ZCH)
    return arr, {name: ZD.layer_files(cut, (0, 0, 0), (2, 2), ZD.encoder(comp, **kw)) for name, (comp, kw) in ZCODECS.items()}


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)], ids=["in order", "permuted"])
@pytest.mark.parametrize("codec", list(ZCODECS))
def test_zarr_channels_of_one_chunk(service, channels, codec, order):
    """Bands of 64 rows: band 0 needs chunk rows 0 and 1 (rows 40 .. 69, which straddle its end),
    band 1 (rows 64 .. 69) chunk row 1 alone.  Member i is channel order[i] = slice order[i]."""
    arr, files = channels
    comp, files = ZCODECS[codec][0], files[codec]
    image = next(_ids)
    descs = [dict(image_id=image, z=0, c=c, t=0, pixel_type=pbx.UINT16, size_x=ZW, size_y=ZH, big_endian=True) for c in range(3)]
    layer = dict(chunk_x=72, chunk_y=40, codec=comp, chunk_planes=3, fill_bits=0, chunks=files)
    whole = service.register_zarr_planes_deep(descs, [(0, c) for c in range(3)], [layer])
    try:
        want = [service.read_plane_be(pid, ZH * ZW * 2) for pid in whole]
    finally:
        release(service, whole)
    assert want == [arr[0, c, 0].tobytes() for c in range(3)]
    image = next(_ids)
    pids = [service.create_sparse_plane(image, 0, c, 0, pbx.UINT16, ZW, ZH, 64) for c in range(3)]
    try:
        ids = [pids[c] for c in order]
        st, ms = service.band_write_zarr_group(ids, list(order), 1, 0, 64, 72, 40, comp, files, chunk_planes=3)
        assert st == [OK] * 3 and len(ms) == 2
        assert all(service.band_info(pid)[1] == [READY, ABSENT] for pid in pids)
        st, _ = service.band_write_zarr_group(ids, list(order), 2, 64, 6, 72, 40, comp, files[2:], chunk_planes=3)
        assert st == [OK] * 3
        for c in range(3):
            assert service.band_info(pids[c])[1] == [READY, READY]
            assert rows_of(service, image, 0, ZH, ZW, c=c) == want[c], c
    finally:
        release(service, pids)


def test_zarr_sibling_kept_out_is_not_decoded_into(service, channels):
    """A resident sibling is dropped (409): the launch is planned again for those that joined."""
    arr, files = channels
    files = files["blosc-lz4"]
    image = next(_ids)
    pids = [service.create_sparse_plane(image, 0, c, 0, pbx.UINT16, ZW, ZH, 64) for c in range(3)]
    try:
        service.band_write(pids[1], 0, 64, b"\x11" * (64 * ZW * 2))
        st, _ = service.band_write_zarr_group(pids, [0, 1, 2], 0, 0, 64, 72, 40, "blosc", files, chunk_planes=3)
        assert st == [OK, pbx.E_EXISTS, OK]
        assert rows_of(service, image, 0, 64, ZW, c=1) == b"\x11" * (64 * ZW * 2)
        for c in (0, 2):
            assert rows_of(service, image, 0, 64, ZW, c=c) == arr[0, c, 0][:64].tobytes()
    finally:
        release(service, pids)


# ------------------------------------------------------------------------------ 6 .. 8: states
@pytest.fixture(scope="module")
def rgb16():
    """The chunky 21 x 65 uint16 RGB layer (LZW strips of 4 rows, Predictor 2) the state tests share."""
    a = full_range(pbx.UINT16, W, H, 3, ">", 71)
    segs, base = chunky(a, pbx.UINT16, ">", None, 4, pbx.TIFF_LZW, 2)
    return a, segs, base, [be_bytes(a[:, :, c]) for c in range(3)]


def test_a_resident_sibling_is_kept_out(service, rgb16):
    a, segs, base, want = rgb16
    image, row = next(_ids), row_bytes(base)
    pids = sparse_planes(service, image, 3, base)
    try:
        service.band_write(pids[1], 0, H, b"\x31" * (H * row))
        for c in (0, 2):
            sentinels(service, pids[c], base, 7, 14)
        for y0, rows in ((7, 3), (10, 4)):
            st, _ = group_write(service, pids, 0, segs, base, y0, rows)
            assert st == [OK, pbx.E_EXISTS, OK]
        assert [service.band_info(pid)[1] for pid in pids] == [[READY]] * 3
        assert rows_of(service, image, 0, H, W, c=1) == b"\x31" * (H * row)
        for c in (0, 2):
            check_window(service, image, c, base, 7, 14, want[c])
    finally:
        release(service, pids)


def test_a_sibling_with_a_piece_from_a_single_call_joins_and_completes(service, rgb16):
    a, segs, base, want = rgb16
    image = next(_ids)
    pids = sparse_planes(service, image, 3, base)
    try:
        for pid in pids:
            sentinels(service, pid, base, 7, 14)
        service.band_write_tiff(pids[2], 7, 3, base["seg_w"], base["seg_h"], False, base["compression"], 2,
                                piece(segs, base, 7, 3), samples_per_pixel=3, sample=2)
        assert [service.band_info(pid)[1] for pid in pids] == [[LOADING]] * 3
        st, _ = group_write(service, [pids[0], pids[1], 0], 1, segs, base, 7, 3)
        assert st == [OK, OK, -1]
        st, _ = group_write(service, pids, 0, segs, base, 10, 4)
        assert st == [OK] * 3
        assert [service.band_info(pid)[1] for pid in pids] == [[READY]] * 3
        for c in range(3):
            check_window(service, image, c, base, 7, 14, want[c])
    finally:
        release(service, pids)


def test_a_resident_primary_ends_the_call(service, rgb16):
    a, segs, base, want = rgb16
    image, row = next(_ids), row_bytes(base)
    pids = sparse_planes(service, image, 3, base)
    try:
        service.band_write(pids[1], 0, H, b"\x31" * (H * row))
        with pytest.raises(pbx.PbxError, match="band 0 is resident") as e:
            group_write(service, pids, 1, segs, base, 0, H)
        assert e.value.status == pbx.E_EXISTS and e.value.statuses == [-1, pbx.E_EXISTS, -1]
        assert [service.band_info(pid)[1] for pid in pids] == [[ABSENT], [READY], [ABSENT]]
        assert rows_of(service, image, 0, H, W, c=1) == b"\x31" * (H * row)
    finally:
        release(service, pids)


def test_injected_upload_failure_fails_every_joined_band(service, rgb16):
    a, segs, base, want = rgb16
    image = next(_ids)
    pids = sparse_planes(service, image, 3, base)
    try:
        before = service.residency_stats()["resident_bytes"]
        service.test_fail_band_write(1)
        with pytest.raises(pbx.PbxError, match="injected upload failure") as e:
            group_write(service, pids, 2, segs, base, 0, H)
        assert e.value.status == pbx.E_INTERNAL and e.value.statuses == [pbx.E_INTERNAL] * 3
        assert [service.band_info(pid)[1] for pid in pids] == [[ABSENT]] * 3
        assert service.residency_stats()["resident_bytes"] == before
        st, _ = group_write(service, pids, 2, segs, base, 0, H)
        assert st == [OK] * 3
        assert [rows_of(service, image, 0, H, W, c=c) for c in range(3)] == want
    finally:
        service.test_fail_band_write(0)
        release(service, pids)


def test_corrupt_stream_fails_every_joined_band(service, rgb16):
    """The decoder's own error code for a stream it rejects (the handled path of the existing
    corrupt-stream tests): a code far above the next free one right after the Clear."""
    a, segs, base, want = rgb16
    bad = list(segs)
    bad[2] = b"\x80\x7f\xff" + bad[2][3:]
    image = next(_ids)
    pids = sparse_planes(service, image, 3, base)
    try:
        before = service.residency_stats()["resident_bytes"]
        with pytest.raises(pbx.PbxError, match=r"corrupt chunk stream 2 \(lzw, decoder code") as e:
            group_write(service, pids, 0, bad, base, 0, H)
        assert e.value.status == 400 and e.value.statuses == [400] * 3
        assert [service.band_info(pid)[1] for pid in pids] == [[ABSENT]] * 3
        assert service.residency_stats()["resident_bytes"] == before
        assert all(service.get_tile(pbx.TileCtx(image, 0, c, 0, 0, 0, W, H))[0] == pbx.E_NOT_RESIDENT for c in range(3))
        st, _ = group_write(service, pids, 0, segs, base, 0, H)
        assert st == [OK] * 3
        assert [rows_of(service, image, 0, H, W, c=c) for c in range(3)] == want
    finally:
        release(service, pids)


@pytest.mark.parametrize("primary,statuses", [(1, [OK, OK, pbx.E_NO_SPACE]), (2, [OK, pbx.E_NO_SPACE, OK])])
def test_budget_of_two_bands(rgb16, primary, statuses):
    """A private service whose residency budget is exactly two bands, nothing else resident: the
    primary's band is allocated first, then the siblings' in order; bands that are loading are not
    evictable, so the third allocation answers 507, whichever member it is."""
    a, segs, base, want = rgb16
    band_bytes = (row_bytes(base) + 255) // 256 * 256 * H + 256
    with pbx.PixelsService() as svc:
        svc.set_residency_budget(2 * band_bytes)
        image = next(_ids)
        pids = sparse_planes(svc, image, 3, base)
        assert svc.residency_stats()["resident_bytes"] == 0
        st, _ = group_write(svc, pids, primary, segs, base, 0, H)
        assert st == statuses
        assert b"residency budget" not in pbx.lib().pbx_last_error()  # a dropped sibling is no error of the call's
        assert [svc.band_info(pid)[1] for pid in pids] == [[READY if s == OK else ABSENT] for s in st]
        assert svc.residency_stats()["resident_bytes"] == 2 * band_bytes
        for c in range(3):
            status, body = svc.get_tile(pbx.TileCtx(image, 0, c, 0, 3, 2, 40, 11))
            if st[c] == OK:
                assert status == OK and body == be_bytes(a[2:13, 3:43, c])
            else:
                assert status == pbx.E_NOT_RESIDENT


# ------------------------------------------------------------------------------ 9. refusals
def test_refusals(service, rgb16, channels):
    a, segs, base, want = rgb16
    L = pbx.lib()
    image = next(_ids)
    pids = sparse_planes(service, image, 3, base)
    whole = service.register_plane(next(_ids), 0, 0, 0, pbx.UINT16, W, H, data=np.zeros((H, W), ">u2"))
    odd = [service.create_sparse_plane(next(_ids), 0, 0, 0, pbx.UINT16, W + 1, H, H),              # another size
           service.create_sparse_plane(next(_ids), 0, 0, 0, pbx.INT16, W, H, H),                   # another type
           service.create_sparse_plane(next(_ids), 0, 0, 0, pbx.UINT16, W, H, H, big_endian=False),  # another byte order
           service.create_sparse_plane(next(_ids), 0, 0, 0, pbx.UINT16, W, H, 7)]                  # other bands
    dbl = [service.create_sparse_plane(next(_ids), 0, c, 0, pbx.DOUBLE, W, H, H) for c in range(2)]
    s = pbx.PbxTiffSegments()
    kept = pbx._fill_tiff_segments(s, dict(base, segments=segs))
    arr, files = channels
    z = pbx.PbxZarrChunks()
    kept += pbx._fill_zarr_chunks(z, dict(chunk_x=72, chunk_y=40, codec=None, chunks=files["raw"]))
    zp = [service.create_sparse_plane(next(_ids), 0, c, 0, pbx.UINT16, ZW, ZH, 64) for c in range(3)]

    def u64(v):
        return (ctypes.c_uint64 * len(v))(*v)

    def i32(v):
        return (ctypes.c_int32 * len(v))(*v)

    def tiff(ids, primary, msg, status=400, n=None, y0=0, rows=H, segments=s, packed=None, j2k=0):
        st = i32([7] * 4)
        rc = L.pbx_band_write_tiff_group(service.handle, u64(ids) if ids is not None else None, len(ids) if n is None else n,
                                         primary, y0, rows, ctypes.byref(segments) if segments is not None else None, None,
                                         j2k, ctypes.byref(packed) if packed is not None else None, st, None)
        assert rc == status and msg in L.pbx_last_error().decode(), (rc, L.pbx_last_error())

    def zarr(ids, slices, primary, msg, status=400, n=None, y0=0, rows=64, chunks=z, depth=3):
        rc = L.pbx_band_write_zarr_group(service.handle, u64(ids) if ids is not None else None,
                                         i32(slices) if slices is not None else None, len(ids) if n is None else n, primary,
                                         y0, rows, ctypes.byref(chunks) if chunks is not None else None, depth, None, None)
        assert rc == status and msg in L.pbx_last_error().decode(), (rc, L.pbx_last_error())

    try:
        assert L.pbx_band_write_tiff_group(None, u64(pids), 3, 0, 0, H, ctypes.byref(s), None, 0, None, None, None) == 400
        assert L.pbx_last_error() == b"null argument"
        tiff(None, 0, "null argument", n=3)
        tiff(pids, 0, "null argument", segments=None)
        zarr(None, [0, 1, 2], 0, "null argument", n=3)
        zarr(zp, None, 0, "null argument")
        zarr(zp, [0, 1, 2], 0, "null argument", chunks=None)
        for call, ps in ((tiff, pids), (lambda ids, *a, **k: zarr(ids, list(range(len(ids))), *a, **k), zp)):
            call(ps, 0, "group of 0 planes outside 1 .. 4", n=0)
            call(ps + [0], 0, "group of 5 planes outside 1 .. 4", n=5)
            call(ps, 3, "primary 3 outside the group of 3")
            call(ps, -1, "primary -1 outside the group of 3")
            call([ps[0], 0, ps[2]], 1, "primary 1 names plane id 0")
            call([ps[0], ps[1], ps[0]], 1, "plane %d is members 0 and 2 of the group" % ps[0])
            call([ps[0], 1 << 40, ps[2]], 0, "no plane %d" % (1 << 40), status=404)
            call([ps[0], whole, ps[2]], 0, "plane %d is not a sparse plane" % whole)
        for other in odd:
            tiff([pids[0], other, pids[2]], 0, "differ in size, pixel type, byte order or band rows")
        zarr([zp[0], pids[1], zp[2]], [0, 1, 2], 0, "differ in size, pixel type, byte order or band rows")
        tiff(pids, 0, "rows 0+22 outside the plane (21 rows)", rows=22)
        tiff(pids, 0, "rows -1+5 outside the plane", y0=-1, rows=5)
        zarr(zp, [0, 1, 2], 0, "rows 60+8 cross the end of band 0 (rows 0..64)", y0=60, rows=8)
        # the codecs' own refusals (flat: the same segments declared without a predictor)
        flat = pbx.PbxTiffSegments()
        keep2 = pbx._fill_tiff_segments(flat, dict(base, predictor=1, segments=segs))
        tiff(dbl + [0], 0, "predictor 2 on floating-point samples")
        tiff(dbl + [0], 0, "samples_per_pixel 3 on 64-bit samples", segments=flat)
        tiff(pids, 0, "bad compression 5 (the JPEG 2000 calls take 34712)", j2k=1)
        k = pbx.PbxTiffPacked()
        pbx._fill_tiff_packed(k, dict(bits=12), 2, 0)
        tiff(pids, 0, "group of 3 planes on segments of 2 samples per pixel", packed=k)
        pbx._fill_tiff_packed(k, dict(bits=0), 3, 0)
        tiff(pids, 0, "bad bits 0 (1 .. 16)", packed=k, segments=flat)
        thin = pbx.PbxTiffSegments()
        keep2 += pbx._fill_tiff_segments(thin, dict(base, seg_w=0, segments=segs))
        tiff(pids, 0, "bad segment shape 0 x 4", segments=thin)
        zarr(zp, [0, 1, 3], 0, "slice 3 outside chunks of 3 planes")
        zarr(zp, [0, -1, 2], 0, "slice -1 outside chunks of 3 planes")
        zarr(zp, [0, 1, 1], 0, "slice 1 is members 1 and 2 of the group")
        zarr(zp, [0, 1, 2], 0, "chunk_planes 0 < 1", depth=0)
        bad = pbx.PbxZarrChunks()
        keep2 += pbx._fill_zarr_chunks(bad, dict(chunk_x=0, chunk_y=40, codec=None, chunks=files["raw"]))
        zarr(zp, [0, 1, 2], 0, "bad chunk shape", chunks=bad)
        # nothing was joined
        assert [service.band_info(pid)[1] for pid in pids] == [[ABSENT]] * 3
        assert [service.band_info(pid)[1] for pid in zp] == [[ABSENT, ABSENT]] * 3
        del kept, keep2
    finally:
        release(service, pids + odd + dbl + zp + [whole])


def test_a_group_of_one_is_the_single_call(service, rgb16):
    a, segs, base, want = rgb16
    grey_segs, grey = chunky(a[:, :, :1], pbx.UINT16, ">", None, 4, pbx.TIFF_LZW, 2)
    image = next(_ids)
    (pid,) = sparse_planes(service, image, 1, grey)
    try:
        sentinels(service, pid, grey, 7, 14)
        for y0, rows in ((7, 3), (10, 4)):
            st, _ = group_write(service, [pid], 0, grey_segs, grey, y0, rows)
            assert st == [OK]
        check_window(service, image, 0, grey, 7, 14, want[0])
        with pytest.raises(pbx.PbxError, match="band 0 is resident") as e:
            group_write(service, [pid], 0, grey_segs, grey, 7, 3)
        assert e.value.status == pbx.E_EXISTS
    finally:
        service.release_plane(pid)


# ------------------------------------------------------------------------------ 10. the handler
class Counting:
    """A source that counts the band reads (rows > 0) of the source it wraps."""

    def __init__(self, src):
        self.src, self.reads, self.lock = src, [], threading.Lock()

    def __getattr__(self, name):
        return getattr(self.src, name)

    def _count(self, name, pixels, z, c, t, level, y0, rows):
        spec = getattr(self.src, name)(pixels, z, c, t, level, y0, rows)
        if rows > 0 and spec is not None:  # (None: the source has no access of that kind)
            with self.lock:
                self.reads.append((c, y0, rows))
        return spec

    def band_segments(self, *a):
        return self._count("band_segments", *a)

    def band_chunks(self, *a):
        return self._count("band_chunks", *a)


def tile(svc, src, image, c, x, y, w, h):
    return pbx.TileRequestHandler(svc, pbx.TileCtx(image, 0, c, 0, x, y, w, h), src).get_tile()


def rgb_pyramid():
    gold = os.path.join(HERE, "golden", "tiff_rgb")
    with open(os.path.join(gold, "manifest.json")) as f:
        entry = next(e for e in json.load(f)["files"] if e["file"].startswith("pyramid"))
    planes = []
    for c in range(3):
        npy, s = entry["planes"]["0"]["0,%d,0" % c]
        a = np.load(os.path.join(gold, npy))
        planes.append(np.ascontiguousarray(a[s[0], :, :, s[1]] if isinstance(s, list) else a[:, :, s]))
    return os.path.join(gold, entry["file"]), planes, (5, 30, 140, 20)


def jpeg_pyramid():
    entry = next(e for e in J.manifest() if e["file"].startswith("pyramid"))
    return os.path.join(J.GOLD, entry["file"]), [J.expected(entry, 0, "0,%d,0" % c) for c in range(3)], (5, 30, 90, 20)


@pytest.mark.parametrize("fixture", [rgb_pyramid, jpeg_pyramid], ids=["rgb", "jpeg"])
def test_handler_fills_the_siblings_of_a_tiff(fixture):
    """Rows 30 .. 49 lie in bands 1, 2 and 3 of 16 rows."""
    path, planes, (x, y, w, h) = fixture()
    want = [p[y:y + h, x:x + w].tobytes() for p in planes]
    image, nbands = next(_ids), 3
    with pbx.PixelsService(sparse_band_rows=16, fill_siblings=True) as svc:
        src = Counting(pbx.TiffSource({image: path}))
        assert [tile(svc, src, image, c, x, y, w, h) for c in range(3)] == want
        assert sorted(src.reads) == [(0, 16 * k, 16) for k in (1, 2, 3)]  # once per covered band, all by c = 0
        for c in range(3):
            assert svc.band_info(svc.lookup_plane(image, 0, c, 0)[0])[1][1:4] == [READY] * 3
    with pbx.PixelsService(sparse_band_rows=16, fill_siblings=True) as svc:  # three channels at once
        src = Counting(pbx.TiffSource({image: path}))
        got = [None] * 3

        def ask(c):
            got[c] = tile(svc, src, image, c, x, y, w, h)
        threads = [threading.Thread(target=ask, args=(c,)) for c in range(3)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert got == want
        assert nbands <= len(src.reads) <= 3 * nbands
    with pbx.PixelsService(sparse_band_rows=16) as svc:  # the default: nothing changed
        src = Counting(pbx.TiffSource({image: path}))
        assert tile(svc, src, image, 0, x, y, w, h) == want[0]
        assert svc.lookup_plane(image, 0, 1, 0) is None and svc.lookup_plane(image, 0, 2, 0) is None
        assert len(src.reads) == nbands
        assert [tile(svc, src, image, c, x, y, w, h) for c in (1, 2)] == want[1:]
        assert sorted(src.reads) == sorted((c, 16 * k, 16) for c in range(3) for k in (1, 2, 3))
        # load_bands' keyword overrides the service's setting
        pixels = src.get_pixels(image)
        svc.load_bands(src, pixels, 0, 0, 0, 0, 0, 16, siblings=True)
        assert [svc.band_info(svc.lookup_plane(image, 0, c, 0)[0])[1][0] for c in range(3)] == [READY] * 3
        assert src.reads[-1] == (0, 0, 16) and len(src.reads) == 3 * nbands + 1


def test_handler_fills_the_siblings_of_an_ngff_array(tmp_path):
    """Chunks that hold the three channels; rows 50 .. 61 lie in band 3 (chunk row 1)."""
    arr = ZD.noise_array((1, 3, 1, ZH, ZW), ">u2", seed=39)
    comp, kw = ZCODECS["blosc-lz4"]
    ZD.write_array(tmp_path / "img" / "0", arr, ZCH, comp, ZD.encoder(comp, **kw), "/")
    (tmp_path / "img" / ".zattrs").write_text(json.dumps({"multiscales": [{
        "version": "0.4", "axes": [{"name": n} for n in "tczyx"], "datasets": [{"path": "0"}]}]}))
    image = next(_ids)
    want = [arr[0, c, 0][50:62, 10:90].tobytes() for c in range(3)]
    with pbx.PixelsService(sparse_band_rows=16, fill_siblings=True) as svc:
        src = Counting(pbx.NgffSource({image: str(tmp_path / "img")}))
        assert tile(svc, src, image, 1, 10, 50, 80, 12) == want[1]
        assert [tile(svc, src, image, c, 10, 50, 80, 12) for c in (0, 2)] == [want[0], want[2]]
        assert src.reads == [(1, 48, 16)]
        for c in range(3):
            assert svc.band_info(svc.lookup_plane(image, 0, c, 0)[0])[1] == [ABSENT] * 3 + [READY, ABSENT]
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = Counting(pbx.NgffSource({image: str(tmp_path / "img")}))
        assert tile(svc, src, image, 0, 10, 50, 80, 12) == want[0]
        assert svc.lookup_plane(image, 0, 1, 0) is None and src.reads == [(0, 48, 16)]
        assert [tile(svc, src, image, c, 10, 50, 80, 12) for c in (1, 2)] == want[1:]
        assert sorted(src.reads) == [(c, 48, 16) for c in range(3)]


@pytest.mark.parametrize("how", ["released", "whole plane", "other bands"])
def test_a_sibling_that_went_away_does_not_fail_the_primary(how):
    """Siblings are best effort: one that is released, replaced by a whole plane or by a plane of
    other bands between the lookup and the group call leaves the request to the single call."""
    path, planes, (x, y, w, h) = rgb_pyramid()
    image = next(_ids)
    with pbx.PixelsService(sparse_band_rows=16, fill_siblings=True) as svc:
        src = Counting(pbx.TiffSource({image: path}))
        real = svc._sibling_group

        def spoiled(source, pixels, z, c, t, level, sx, sy, *a):
            group = real(source, pixels, z, c, t, level, sx, sy, *a)
            svc.release_plane(group["ids"][1])
            if how == "whole plane":
                group["ids"][1] = svc.register_plane(image, 0, 1, 0, pixels.pixel_type, sx, sy,
                                                     data=np.zeros((sy, sx), planes[1].dtype))
            elif how == "other bands":
                group["ids"][1] = svc.create_sparse_plane(image, 0, 1, 0, pixels.pixel_type, sx, sy, 8, big_endian=False)
            return group
        svc._sibling_group = spoiled
        assert tile(svc, src, image, 0, x, y, w, h) == planes[0][y:y + h, x:x + w].tobytes()
        # the first band's segments are read for the refused group call and again for the single one
        assert src.reads == [(0, 16, 16), (0, 16, 16), (0, 32, 16), (0, 48, 16)]
        assert svc.band_info(svc.lookup_plane(image, 0, 0, 0)[0])[1][1:4] == [READY] * 3
        c2 = svc.lookup_plane(image, 0, 2, 0)  # the other sibling was created and stays unfilled
        assert c2 is not None and svc.band_info(c2[0])[1][1:4] == [ABSENT] * 3
