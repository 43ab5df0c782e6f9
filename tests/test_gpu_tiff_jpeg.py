"""JPEG-compressed TIFF segments (Compression 7) on the GPU: k_tiff_jpeg_decode and
k_tiff_jpeg_place against tests/_tiff_jpeg.py's numpy model, which tests/test_tiff_jpeg_host.py
holds equal to PIL (libjpeg-turbo) byte for byte.  Every comparison is exact."""
import itertools
import os

import numpy as np
import pytest

import _tiff_jpeg as J
import pbx
from _tiff_jpeg import (GOLD, KINDS, bad_streams, checker, expected, generated_streams, kind_page as page, noise, ramp,
                        stream_page)

pytestmark = pytest.mark.gpu

FILES = J.manifest()
IDS = [f["file"] for f in FILES]
_ids = itertools.count(8_300_000)  # disjoint from the other test files (shared service)


def rows_of(svc, image, y0, rows, w, z=0, c=0, t=0, resolution=None):
    st, body = svc.get_tile(pbx.TileCtx(image, z, c, t, 0, y0, w, rows, resolution=resolution))
    assert st == pbx.OK, st
    return body


def specs_of(page, image, samples=None):
    """register_tiff_planes specs straight from a page_of() page: one per sample."""
    h, w, s, tile = page["length"], page["width"], page["spp"], page["tile"]
    tabs = next((bytes(t[2]) for t in page["extra"] if t[0] == 347), None)
    base = dict(image_id=image, z=0, t=0, pixel_type=pbx.UINT8, size_x=w, size_y=h, big_endian=False,
                seg_w=tile[0] if tile else w, seg_h=tile[1] if tile else min(page["rows_per_strip"], h),
                tiled=tile is not None, compression=pbx.TIFF_JPEG, predictor=1,
                jpeg=dict(tables=tabs, ycbcr=page["photometric"] == 6))
    segs = page["segments"]
    if page["planar"] == 2 and s > 1:
        n = len(segs) // s
        return [dict(base, c=c, samples_per_pixel=1, sample=0, segments=pbx.pack_chunks(segs[c * n:(c + 1) * n]))
                for c in (samples or range(s))]
    packed = pbx.pack_chunks(segs)
    return [dict(base, c=c, samples_per_pixel=s, sample=c, segments=packed) for c in (samples or range(s))]


def check_pages(svc, pages, what=""):
    """Every page a layer of ONE registration; every plane equal to the model's."""
    specs, wants = [], []
    for page in pages:
        sp = specs_of(page, next(_ids))
        want = J.decode_page(page)
        specs += sp
        wants += [want[:, :, c] if want.ndim == 3 else want for c in range(len(sp))]
    ids = svc.register_tiff_planes(specs)
    try:
        for k, (pid, want) in enumerate(zip(ids, wants)):
            got = np.frombuffer(svc.read_plane_be(pid, want.size), np.uint8).reshape(want.shape)
            assert np.array_equal(got, want), (what, k, specs[k]["size_x"], specs[k]["size_y"], specs[k]["c"],
                                               np.argwhere(got != want)[:4].tolist())
    finally:
        for pid in ids:
            svc.release_plane(pid)


# ------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_registered_whole(service, entry):
    image = next(_ids)
    ids = service.register_tiff_image(os.path.join(GOLD, entry["file"]), image)
    try:
        assert sorted(ids) == sorted(int(k) for k in entry["planes"])
        for level, planes in ids.items():
            assert sorted("%d,%d,%d" % p for p in planes) == sorted(entry["planes"][str(level)])
            for (z, c, t), pid in planes.items():
                want = expected(entry, level, "%d,%d,%d" % (z, c, t))
                assert service.read_plane_be(pid, want.nbytes) == want.tobytes(), (entry["file"], level, z, c, t)
    finally:
        for planes in ids.values():
            for pid in planes.values():
                service.release_plane(pid)


@pytest.mark.parametrize("B", [16, 40, 100], ids=["16", "40", "whole"])
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_band_by_band(service, entry, B):
    path = os.path.join(GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    S = lay["samples"]
    for (z, c0, t), ifd in zip(lay["planes"], lay["ifds"]):
        for level, d in enumerate([ifd] + ifd["subifds"]):
            for s in range(S):
                want = expected(entry, level, "%d,%d,%d" % (z, c0 + s, t))
                h, w = want.shape
                rows = h if B == 100 else B
                image = next(_ids)
                pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, w, h, rows, big_endian=False)
                try:
                    for r0 in range(0, h, rows):
                        n = min(rows, h - r0)
                        sp = pbx.tiff_band_spec(path, d, r0, n, sample=s)
                        service.band_write_tiff(pid, r0, n, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"],
                                                sp["predictor"], sp["segments"], jpeg=sp["jpeg"],
                                                samples_per_pixel=sp["samples_per_pixel"], sample=sp["sample"])
                        assert rows_of(service, image, r0, n, w) == want[r0:r0 + n].tobytes(), (entry["file"], s, r0)
                    assert set(service.band_info(pid)[1]) == {pbx.BS_READY}
                finally:
                    service.release_plane(pid)


# ------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("rps", [8, 16])
@pytest.mark.parametrize("kind", list(KINDS))
def test_strip_images(service, kind, rps):
    """Partial MCUs on both edges, chroma planes one sample wide or high, strips whose last one is
    short: every width x height as a layer of one registration."""
    pages = [page(kind, noise(w, h, 100 * w + h), rows_per_strip=rps, quality=85)
             for w in (1, 7, 8, 9, 15, 16, 17, 33) for h in (1, 8, 9, 17)]
    check_pages(service, pages, kind)


@pytest.mark.parametrize("tile", [16, 64])
@pytest.mark.parametrize("shape", [(40, 30), (100, 70)], ids=["40x30", "100x70"])
def test_clipped_tiles(service, tile, shape):
    w, h = shape
    a = noise(w, h, tile + w) // 2 + ramp(w, h) // 2
    check_pages(service, [page(k, a, tile=(tile, tile), quality=80) for k in KINDS], "tiles %d" % tile)


@pytest.mark.parametrize("kind", ["420", "444"])
def test_one_tile_of_256(service, kind):
    """More blocks than one batch, many MCU rows, a refilled input window."""
    check_pages(service, [page(kind, noise(256, 256, 7), tile=(256, 256), quality=75)], kind)


@pytest.mark.parametrize("quality", [30, 75, 95, 100])
def test_qualities(service, quality):
    pages, stuffed = [], 0
    for a in (noise(40, 24, quality), ramp(40, 24), checker(40, 24)):
        for kind in ("gray", "444", "420"):
            pages.append(page(kind, a, rows_per_strip=16, quality=quality, tables="segment"))
            stuffed += sum(b"\xff\x00" in s[J.header(s)["data"]:] for s in pages[-1]["segments"])
    assert stuffed, "no stream holds a stuffed FF"
    check_pages(service, pages, "quality %d" % quality)


def test_generated_streams(service):
    check_pages(service, [stream_page(w, h, s) for _, w, h, s in generated_streams()], "generated")


@pytest.mark.parametrize("kind", ["gray", "444", "420"])
def test_restart_intervals(service, kind):
    a = noise(50, 40, 11)
    pages = [page(kind, a, rows_per_strip=24, quality=80, restart_blocks=1),
             page(kind, a, rows_per_strip=24, quality=80, restart_blocks=3),
             page(kind, a, tile=(32, 32), quality=80, restart_rows=1)]
    assert all(J.header(p["segments"][0])["restart"] for p in pages)
    check_pages(service, pages, kind)


def test_tables_in_the_tag_in_the_segment_and_both(service):
    a = noise(40, 30, 13) // 2 + ramp(40, 30) // 2
    pages = [page(k, a, tile=(16, 16), quality=q, tables=t)
             for k, q in (("420", 90), ("gray", 50), ("rgb", 70)) for t in ("tag", "segment", "both")]
    check_pages(service, pages, "tables")


def test_one_sample_of_three(service):
    a = noise(40, 30, 17)
    pg = page("422", a, tile=(16, 16), quality=85)
    want = J.decode_page(pg)
    image = next(_ids)
    (pid,) = service.register_tiff_planes(specs_of(pg, image, samples=[1]))
    try:
        assert service.read_plane_be(pid, 40 * 30) == want[:, :, 1].tobytes()
        assert service.lookup_plane(image, 0, 0, 0) is None and service.lookup_plane(image, 0, 2, 0) is None
    finally:
        service.release_plane(pid)


@pytest.mark.parametrize("tile", [None, (16, 16)], ids=["strips", "tiles"])
@pytest.mark.parametrize("kind", ["420", "444", "rgb"])
def test_one_sample_band_write(service, kind, tile):
    """Rows 7 .. 13 of a 21-row plane from two pieces cut inside a segment; sentinel rows around
    them and sentinel sibling planes stay as they were."""
    S, h, w = 3, 21, 65
    pg = page(kind, noise(w, h, 23), tile=tile, rows_per_strip=8, quality=85)
    want = J.decode_page(pg)
    sp0 = specs_of(pg, 0)[0]
    data, offsets = sp0["segments"]
    gx, seg_h = (-(-w // 16) if tile else 1), sp0["seg_h"]
    for target in range(S):
        image = next(_ids)
        pids = [service.create_sparse_plane(image, 0, c, 0, pbx.UINT8, w, h, h, big_endian=False) for c in range(S)]
        try:
            for c in range(S):
                if c != target:
                    service.band_write(pids[c], 0, h, bytes([0x30 + c]) * (h * w))
            service.band_write(pids[target], 0, 7, b"\xA5" * (7 * w))
            service.band_write(pids[target], 14, 7, b"\x5A" * (7 * w))
            for y0, rows in ((7, 3), (10, 4)):
                k0, k1 = (y0 // seg_h) * gx, -(-(y0 + rows) // seg_h) * gx
                piece = (data[int(offsets[k0]):int(offsets[k1])].copy(), offsets[k0:k1 + 1] - offsets[k0])
                service.band_write_tiff(pids[target], y0, rows, sp0["seg_w"], seg_h, tile is not None, 7, 1, piece,
                                        samples_per_pixel=S, sample=target, jpeg=sp0["jpeg"])
            assert service.band_info(pids[target])[1] == [pbx.BS_READY]
            got = rows_of(service, image, 0, h, w, c=target)
            assert got[:7 * w] == b"\xA5" * (7 * w) and got[14 * w:] == b"\x5A" * (7 * w)
            assert got[7 * w:14 * w] == want[7:14, :, target].tobytes()
            for c in range(S):
                if c != target:
                    assert rows_of(service, image, 0, h, w, c=c) == bytes([0x30 + c]) * (h * w)
        finally:
            for pid in pids:
                service.release_plane(pid)


# ------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("case", bad_streams(), ids=lambda c: c[0])
def test_device_refusals(service, case):
    name, w, h, stream, code = case
    pg = stream_page(w, h, stream)
    with pytest.raises(J.JpegError) as me:
        J.decode_page(pg)
    assert me.value.code == code
    image = next(_ids)
    specs = specs_of(pg, image)
    with pytest.raises(pbx.PbxError, match=r"corrupt segment stream 0 \(jpeg, decoder code %d" % code) as e:
        service.register_tiff_planes(specs)
    assert e.value.status == 400
    assert all(service.lookup_plane(image, 0, c, 0) is None for c in range(pg["spp"]))
    # a band write: 400, and the band is as it was
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, w, h, h, big_endian=False)
    try:
        with pytest.raises(pbx.PbxError, match="corrupt segment stream") as e:
            service.band_write_tiff(pid, 0, h, w, h, False, 7, 1, specs[0]["segments"], jpeg=specs[0]["jpeg"],
                                    samples_per_pixel=pg["spp"], sample=0)
        assert e.value.status == 400
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT]
    finally:
        service.release_plane(pid)


def test_injected_upload_failure(service):
    pg = page("420", noise(40, 30, 37), tile=(16, 16), quality=85)
    want = J.decode_page(pg)
    image = next(_ids)
    sp = specs_of(pg, image)[0]
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, 40, 30, 30, big_endian=False)
    try:
        service.test_fail_band_write(1)
        with pytest.raises(pbx.PbxError):
            service.band_write_tiff(pid, 0, 30, 16, 16, True, 7, 1, sp["segments"], jpeg=sp["jpeg"], samples_per_pixel=3,
                                    sample=0)
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT]
        service.band_write_tiff(pid, 0, 30, 16, 16, True, 7, 1, sp["segments"], jpeg=sp["jpeg"], samples_per_pixel=3,
                                sample=0)
        assert rows_of(service, image, 0, 30, 40) == want[:, :, 0].tobytes()
    finally:
        service.release_plane(pid)


def test_flipped_bits(service):
    """A bit flipped in the entropy data may still decode: the write succeeds or is a 400, and
    the rows and planes around it keep their bytes either way."""
    w, h = 48, 48
    pg = page("420", noise(w, h, 41), rows_per_strip=16, quality=85, restart_blocks=2)
    sp0 = specs_of(pg, 0)[0]
    data, offsets = sp0["segments"]
    seg = bytes(data[int(offsets[1]):int(offsets[2])])  # the strip of rows 16 .. 31
    d = J.header(seg)["data"]
    rng = np.random.default_rng(43)
    for _ in range(10):
        at = int(rng.integers(d, len(seg) - 2))
        bad = bytearray(seg)
        bad[at] ^= 1 << int(rng.integers(8))
        image = next(_ids)
        pids = [service.create_sparse_plane(image, 0, c, 0, pbx.UINT8, w, h, 16, big_endian=False) for c in range(2)]
        try:
            service.band_write(pids[0], 0, 16, b"\xA5" * (16 * w))
            service.band_write(pids[0], 32, 16, b"\x5A" * (16 * w))
            for k in range(3):
                service.band_write(pids[1], 16 * k, 16, b"\x33" * (16 * w))
            try:
                service.band_write_tiff(pids[0], 16, 16, w, 16, False, 7, 1, [bytes(bad)], jpeg=sp0["jpeg"],
                                        samples_per_pixel=3, sample=0)
                assert service.band_info(pids[0])[1] == [pbx.BS_READY] * 3
            except pbx.PbxError as e:
                assert e.status == 400, e
                assert service.band_info(pids[0])[1] == [pbx.BS_READY, pbx.BS_ABSENT, pbx.BS_READY]
            assert rows_of(service, image, 0, 16, w) == b"\xA5" * (16 * w)
            assert rows_of(service, image, 32, 16, w) == b"\x5A" * (16 * w)
            assert rows_of(service, image, 0, h, w, c=1) == b"\x33" * (h * w)
        finally:
            for pid in pids:
                service.release_plane(pid)


# --------------------------------------------------------------------- behind the handler
def test_tiff_source_serves_a_ycbcr_pyramid(oracle):
    entry = next(e for e in FILES if e["file"].startswith("pyramid"))
    path = os.path.join(GOLD, entry["file"])
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({71: path})
        for c in range(3):
            want = expected(entry, 0, "0,%d,0" % c)
            body = pbx.TileRequestHandler(svc, pbx.TileCtx(71, 0, c, 0, 5, 30, 90, 20), src).get_tile()
            assert body == want[30:50, 5:95].tobytes(), c
            tif = pbx.TileRequestHandler(svc, pbx.TileCtx(71, 0, c, 0, 8, 33, 40, 10, format="tif"), src).get_tile()
            r, px, _ = oracle.tiff_decode(tif, 40 * 10)
            assert r == 0 and px == want[33:43, 8:48].tobytes(), c
            # rows 30 .. 49 lie in bands 1, 2 and 3 of 16 rows: only those were read
            pid = svc.lookup_plane(71, 0, c, 0)[0]
            states = svc.band_info(pid)[1]
            assert [s == pbx.BS_READY for s in states] == [False, True, True, True, False], states
        # stored level 1 is resolution 1 of 3 (resolution 0 is the smallest)
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(71, 0, 2, 0, 3, 10, 40, 20, resolution=1), src).get_tile()
        assert body == expected(entry, 1, "0,2,0")[10:30, 3:43].tobytes()


def test_a_file_that_mixes_jpeg_and_deflate_levels(service, tmp_path):
    """register_tiff_image on a JPEG page with a deflate SubIFD: two registrations behind one call,
    and when the JPEG one is refused nothing of the other stays registered."""
    import _tiff_rgb as R
    a = noise(40, 30, 51) // 2 + ramp(40, 30) // 2
    low = np.ascontiguousarray(a[::2, ::2])
    sub = R.page_of(low, compression=pbx.TIFF_DEFLATE, tile=(16, 16))
    pg = J.page_of(a, tile=(16, 16), subsampling=2, quality=85, subifds=[sub])
    path = str(tmp_path / "mixed.tif")
    J.write_tiff(path, [pg])
    image = next(_ids)
    ids = service.register_tiff_image(path, image)
    try:
        want = J.decode_page(pg)
        for c in range(3):
            assert service.read_plane_be(ids[0][(0, c, 0)], 40 * 30) == want[:, :, c].tobytes()
            assert service.read_plane_be(ids[1][(0, c, 0)], 20 * 15) == low[:, :, c].tobytes()
    finally:
        for planes in ids.values():
            for pid in planes.values():
                service.release_plane(pid)
    segs = list(pg["segments"])
    segs[1] = segs[1][:J.header(segs[1])["data"] + 3]  # entropy data cut short: the device refuses it
    J.write_tiff(path, [dict(pg, segments=segs)])
    image = next(_ids)
    with pytest.raises(pbx.PbxError, match="corrupt segment stream"):
        service.register_tiff_image(path, image)
    assert all(service.lookup_plane(image, 0, c, 0, level) is None for c in range(3) for level in (0, 1))
