"""TIFF strips and tile rows decoded on demand into the bands of a sparse plane
(pbx_band_write_tiff): the decoders of pbx_planes_register_tiff on the covering segment rows
only, k_zarr_place for Predictor 1 (stored segments read where they were uploaded) and
k_tiff_unpred_place for Predictor 2.

Expected bytes: the fixtures' .npy (tests/golden/tiff), or the numpy array the segments were made
from by tests/_tiff_src.py.  Every comparison is byte for byte; sparse planes are read back
through full-width raw tiles (big-endian samples, as every raw tile)."""
import itertools
import json
import os

import numpy as np
import pytest

import _tiff_src as T
import pbx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "tiff")
with open(os.path.join(GOLD, "manifest.json")) as _f:
    FILES = json.load(_f)["files"]
_ids = itertools.count(7_600_000)  # disjoint from the other test files (shared service)


def expected(entry, level="0", key="0,0,0"):
    npy = entry["planes"][level][key]
    if npy is None:  # the PIL-written ramp
        w, h = entry["width"], entry["length"]
        return ((np.arange(w)[None, :] % 100 + np.arange(h)[:, None] // 4) & 0xFF).astype(np.uint8)
    return np.load(os.path.join(GOLD, npy))


def be_bytes(a):
    return np.ascontiguousarray(a).astype(a.dtype.newbyteorder(">")).tobytes()


def rows_of(svc, image, y0, rows, w, z=0, c=0, t=0):
    """Rows [y0, y0 + rows) of a plane, full width, as a raw tile."""
    st, body = svc.get_tile(pbx.TileCtx(image, z, c, t, 0, y0, w, rows))
    assert st == pbx.OK, st
    return body


def covering(segs, gx, seg_h, y0, rows):
    """The segment rows of a whole-plane segment list that cover rows [y0, y0 + rows)."""
    return segs[(y0 // seg_h) * gx:-(-(y0 + rows) // seg_h) * gx]


def write_piece(svc, pid, sp, y0, rows, **kw):
    """One band_write_tiff from a plane's spec (dict: size_x, seg_w, seg_h, tiled, compression,
    predictor, segs = every segment of the plane)."""
    gx = -(-sp["size_x"] // sp["seg_w"]) if sp["tiled"] else 1
    return svc.band_write_tiff(pid, y0, rows, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"],
                               sp["predictor"], covering(sp["segs"], gx, sp["seg_h"], y0, rows), **kw)


# -------------------------------------------------------------- parity with the fixtures
def fixture_planes(entry):
    """(IFD, expected array) of every plane of every level of a fixture file."""
    path = os.path.join(GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    for (z, c, t), ifd in zip(lay["planes"], lay["ifds"]):
        for level, d in enumerate([ifd] + ifd["subifds"]):
            yield d, expected(entry, str(level), "%d,%d,%d" % (z, c, t))


@pytest.mark.parametrize("B", [16, 40, 100], ids=["16", "40", "whole"])
@pytest.mark.parametrize("entry", FILES, ids=[f["file"] for f in FILES])
def test_fixture_band_by_band(service, entry, B):
    """16 puts several bands in one segment row, 40 straddles segment rows, the last is one
    band of the plane's height."""
    path = os.path.join(GOLD, entry["file"])
    for ifd, want in fixture_planes(entry):
        h, w = want.shape
        rows = h if B == 100 else B
        head = pbx.tiff_band_spec(path, ifd, 0, 0)
        assert head["segments"] is None
        image = next(_ids)
        pid = service.create_sparse_plane(image, 0, 0, 0, head["pixel_type"], w, h, rows,
                                          big_endian=head["big_endian"])
        try:
            for r0 in range(0, h, rows):
                n = min(rows, h - r0)
                sp = pbx.tiff_band_spec(path, ifd, r0, n)
                service.band_write_tiff(pid, r0, n, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"],
                                        sp["predictor"], sp["segments"])
                assert rows_of(service, image, r0, n, w) == want[r0:r0 + n].tobytes(), (entry["file"], r0)
            assert set(service.band_info(pid)[1]) == {pbx.BS_READY}
        finally:
            service.release_plane(pid)


# ------------------------------------------------- the fused kernel where it can go wrong
INT_TYPES = [("i1", pbx.INT8), ("u1", pbx.UINT8), ("i2", pbx.INT16), ("u2", pbx.UINT16), ("i4", pbx.INT32),
             ("u4", pbx.UINT32)]
COMPS = [pbx.TIFF_NONE, pbx.TIFF_LZW, pbx.TIFF_DEFLATE]
BAND = 7


def random_plane(rng, dt, h, w):
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, (h, w), dtype=np.int64, endpoint=True).astype(dt)


def plane_spec(a, tile, rps, comp, predictor):
    segs = [T.compress(s, comp) for s in T.segments_of(a, tile, rps, predictor=predictor)]
    return dict(size_x=a.shape[1], size_y=a.shape[0], seg_w=tile[0] if tile else a.shape[1],
                seg_h=tile[1] if tile else rps, tiled=tile is not None, compression=comp, predictor=predictor,
                segs=segs)


@pytest.mark.parametrize("bo", ["<", ">"], ids=["II", "MM"])
@pytest.mark.parametrize("kind,pt", INT_TYPES, ids=[k for k, _ in INT_TYPES])
def test_unpredict_and_place(service, kind, pt, bo):
    """Full-range random samples (every sum wraps) differenced in the file's byte order, written
    in bands of 7 rows, the first band in two pieces at a row that is no segment boundary.
    Width 4097 is more than one 1024-byte step of a row (the carry); 63 and 65 end in a partial
    group and, tiled, in padding that is never stored."""
    dt = np.dtype(bo + kind) if kind[1] != "1" else np.dtype(kind)
    n = 2 * [k for k, _ in INT_TYPES].index(kind) + (bo == ">")  # the seed, and where the codecs' cycle starts
    rng = np.random.default_rng(n)
    used = set()
    for w in (1, 63, 64, 65, 4097):
        layouts = [(None, 5, 2)]
        if w in (63, 65):
            layouts += [((16, 16), 37, None), ((64, 64), 70, None)]
        for tile, h, rps in layouts:
            a = random_plane(rng, dt, h, w)
            comp = COMPS[n % 3]
            n += 1
            used.add(comp)
            sp = plane_spec(a, tile, rps, comp, 2)
            want = be_bytes(a)
            row = w * dt.itemsize
            image = next(_ids)
            pid = service.create_sparse_plane(image, 0, 0, 0, pt, w, h, BAND, big_endian=bo == ">")
            try:
                for r0 in range(0, h, BAND):
                    r1 = min(r0 + BAND, h)
                    cuts = [r0, r0 + 3, r1] if r0 == 0 else [r0, r1]  # 3: inside a strip of 2, a tile of 16
                    for lo, hi in zip(cuts[:-1], cuts[1:]):
                        write_piece(service, pid, sp, lo, hi - lo)
                    assert rows_of(service, image, r0, r1 - r0, w) == want[r0 * row:r1 * row], (w, tile, comp, r0)
            finally:
                service.release_plane(pid)
    assert used == set(COMPS)


# -------------------------------------------------- rows outside the window are not written
@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("comp", COMPS, ids=["stored", "lzw", "deflate"])
@pytest.mark.parametrize("tile", [None, (64, 64)], ids=["strips", "tiles"])
def test_rows_outside_the_piece_survive(service, tile, comp, predictor):
    """Rows 0..9 and 50..69 of a one-band plane are sentinel bytes from band_write; the piece
    [10, 50) from band_write_tiff begins and ends inside a segment (strips of 16, tiles of 64)
    and must leave them alone."""
    h, w = 70, 65
    a = random_plane(np.random.default_rng(11 + predictor), np.dtype("<u2"), h, w)
    sp = plane_spec(a, tile, 16, comp, predictor)
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT16, w, h, h, big_endian=False)
    try:
        service.band_write(pid, 0, 10, b"\xA5" * (10 * w * 2))
        service.band_write(pid, 50, 20, b"\x5A" * (20 * w * 2))
        assert service.band_info(pid)[1] == [pbx.BS_LOADING]
        write_piece(service, pid, sp, 10, 40)
        assert service.band_info(pid)[1] == [pbx.BS_READY]
        got = rows_of(service, image, 0, h, w)
        assert got[:10 * w * 2] == b"\xA5" * (10 * w * 2)
        assert got[50 * w * 2:] == b"\x5A" * (20 * w * 2)
        assert got[10 * w * 2:50 * w * 2] == be_bytes(a[10:50])
    finally:
        service.release_plane(pid)


# ------------------------------------------------------------------------ stored segments
def test_stored_segments_and_timing(service):
    """Stored fixtures (Predictor 1) and a stored Predictor-2 plane; timing=True is a list of two
    device times, the first about 0 for stored segments (no decoder is launched)."""
    for entry in (e for e in FILES if e["compression"] == "none"):
        path = os.path.join(GOLD, entry["file"])
        ifd = pbx.tiff_ifds(path)[0]
        want = expected(entry)
        h, w = want.shape
        head = pbx.tiff_band_spec(path, ifd, 0, 0)
        image = next(_ids)
        pid = service.create_sparse_plane(image, 0, 0, 0, head["pixel_type"], w, h, 24, big_endian=head["big_endian"])
        try:
            for r0 in range(0, h, 24):
                n = min(24, h - r0)
                sp = pbx.tiff_band_spec(path, ifd, r0, n)
                ms = service.band_write_tiff(pid, r0, n, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"],
                                             sp["predictor"], sp["segments"], timing=True)
                assert isinstance(ms, list) and len(ms) == 2 and ms[0] >= 0 and ms[1] >= 0
            assert rows_of(service, image, 0, h, w) == want.tobytes()
        finally:
            service.release_plane(pid)
    a = random_plane(np.random.default_rng(5), np.dtype(">u4"), 45, 150)
    for tile in (None, (32, 16)):
        sp = plane_spec(a, tile, 8, pbx.TIFF_NONE, 2)
        image = next(_ids)
        pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT32, 150, 45, 20, big_endian=True)
        try:
            for r0 in range(0, 45, 20):
                ms = write_piece(service, pid, sp, r0, min(20, 45 - r0), timing=True)
                assert isinstance(ms, list) and len(ms) == 2 and ms[0] >= 0 and ms[1] >= 0
            assert rows_of(service, image, 0, 45, 150) == a.tobytes()
        finally:
            service.release_plane(pid)
    # a compressed piece times both stages
    sp = plane_spec(a, (32, 16), None, pbx.TIFF_LZW, 2)
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT32, 150, 45, 45, big_endian=True)
    try:
        ms = write_piece(service, pid, sp, 0, 45, timing=True)
        assert isinstance(ms, list) and ms[0] > 0 and ms[1] > 0
        assert rows_of(service, image, 0, 45, 150) == a.tobytes()
    finally:
        service.release_plane(pid)


# ------------------------------------------------------------------ float and double planes
@pytest.mark.parametrize("dtype,pt", [("<f4", pbx.FLOAT), (">f4", pbx.FLOAT), ("<f8", pbx.DOUBLE), (">f8", pbx.DOUBLE)])
def test_float_and_double_planes(service, dtype, pt):
    rng = np.random.default_rng(3)
    a = (rng.standard_normal((45, 70)) * 1000).astype(dtype)
    for tile, comp in ((None, pbx.TIFF_LZW), ((32, 32), pbx.TIFF_DEFLATE), ((16, 16), pbx.TIFF_NONE)):
        sp = plane_spec(a, tile, 8, comp, 1)
        image = next(_ids)
        pid = service.create_sparse_plane(image, 0, 0, 0, pt, 70, 45, 20, big_endian=dtype[0] == ">")
        try:
            for r0 in range(0, 45, 20):
                write_piece(service, pid, sp, r0, min(20, 45 - r0))
            assert rows_of(service, image, 0, 45, 70) == be_bytes(a)
            # Predictor 2 is not defined for IEEE samples: refused, the resident band untouched
            with pytest.raises(pbx.PbxError, match="predictor 2 on floating-point") as ei:
                service.band_write_tiff(pid, 0, 20, sp["seg_w"], sp["seg_h"], sp["tiled"], comp, 2,
                                        covering(sp["segs"], 1 if tile is None else -(-70 // tile[0]), sp["seg_h"], 0, 20))
            assert ei.value.status == 400
        finally:
            service.release_plane(pid)


# ------------------------------------------------------------------------------- failures
def smooth_plane(h, w, seed):
    return (np.random.default_rng(seed).poisson(6, (h, w)) & 0xFF).astype(np.uint8)


@pytest.mark.parametrize("case", ["truncated lzw", "wrong adler32"])
def test_corrupt_stream_fails_the_band_load(service, case):
    """400 naming the stream; the band reads absent again and its HBM is returned -- for a band
    written in one piece and for one that already held rows -- and a good retry loads it."""
    a = smooth_plane(64, 100, 8)
    comp = pbx.TIFF_LZW if case == "truncated lzw" else pbx.TIFF_DEFLATE
    good = plane_spec(a, None, 8, comp, 1)
    bad = dict(good, segs=list(good["segs"]))
    s = bad["segs"][5]
    bad["segs"][5] = s[:len(s) // 2] if comp == pbx.TIFF_LZW else s[:-1] + bytes([s[-1] ^ 0x55])
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, 100, 64, 32)
    try:
        base = service.residency_stats()["resident_bytes"]
        for first in (None, (32, 5)):
            if first is not None:
                write_piece(service, pid, good, *first)
                assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_LOADING]
                assert service.residency_stats()["resident_bytes"] > base
            with pytest.raises(pbx.PbxError, match=r"corrupt chunk stream \d+ \((lzw|zlib)") as ei:
                write_piece(service, pid, bad, 37, 27)
            assert ei.value.status == 400
            assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_ABSENT]
            assert service.residency_stats()["resident_bytes"] == base
            assert service.get_tile(pbx.TileCtx(image, 0, 0, 0, 0, 32, 16, 16))[0] == pbx.E_NOT_RESIDENT
        write_piece(service, pid, good, 32, 32)
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_READY]
        assert rows_of(service, image, 32, 32, 100) == a[32:].tobytes()
    finally:
        service.release_plane(pid)


def test_injected_upload_failure(service):
    a = smooth_plane(64, 100, 9)
    sp = plane_spec(a, (32, 32), None, pbx.TIFF_LZW, 2)
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, 100, 64, 32)
    try:
        base = service.residency_stats()["resident_bytes"]
        write_piece(service, pid, sp, 0, 10)
        service.test_fail_band_write(1)
        with pytest.raises(pbx.PbxError, match="injected upload failure") as ei:
            write_piece(service, pid, sp, 10, 22)
        assert ei.value.status == pbx.E_INTERNAL
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_ABSENT]
        assert service.residency_stats()["resident_bytes"] == base
        write_piece(service, pid, sp, 0, 32)
        assert service.band_info(pid)[1] == [pbx.BS_READY, pbx.BS_ABSENT]
        assert rows_of(service, image, 0, 32, 100) == a[:32].tobytes()
    finally:
        service.test_fail_band_write(0)
        service.release_plane(pid)


def test_bad_arguments_leave_a_half_loaded_band_alone(service):
    a = smooth_plane(64, 100, 10)
    sp = plane_spec(a, None, 8, pbx.TIFF_DEFLATE, 1)
    image, wimage = next(_ids), next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, 100, 64, 32)
    whole = service.register_plane(wimage, 0, 0, 0, pbx.UINT8, 100, 64, generator="noise", seed=1)
    try:
        write_piece(service, pid, sp, 32, 12)
        used = service.residency_stats()["resident_bytes"]

        def refused(plane, y0, rows, match, **change):
            with pytest.raises(pbx.PbxError, match=match) as ei:
                write_piece(service, plane, dict(sp, **change), y0, rows)
            assert ei.value.status == 400, ei.value
            assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_LOADING]
            assert service.residency_stats()["resident_bytes"] == used

        refused(pid, 44, 20, "bad compression 7", compression=7)
        refused(pid, 44, 20, "bad predictor 3", predictor=3)
        refused(pid, 44, 20, "strip width 99", seg_w=99)
        refused(pid, 20, 20, "cross the end of band 0")
        refused(pid, 44, 21, "outside the plane")
        refused(pid, 44, 0, "outside the plane")
        refused(whole, 32, 32, "not a sparse plane")
        with pytest.raises(pbx.PbxError) as ei:
            write_piece(service, pid + 12345, sp, 32, 32)
        assert ei.value.status == pbx.E_NOTFOUND
        # host rows and TIFF pieces mix within one load
        service.band_write(pid, 44, 4, a[44:48].tobytes())
        write_piece(service, pid, sp, 48, 16)
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_READY]
        assert rows_of(service, image, 32, 32, 100) == a[32:].tobytes()
        with pytest.raises(pbx.PbxError) as ei:
            write_piece(service, pid, sp, 40, 8)
        assert ei.value.status == pbx.E_EXISTS
    finally:
        service.release_plane(pid)
        service.release_plane(whole)


# ------------------------------------------------------------------- behind the handler
@pytest.fixture
def band_reads(monkeypatch):
    """(ifd width, y0, rows) of every tiff_band_spec call that reads segments."""
    seen, real = [], pbx.tiff_band_spec

    def spy(path, ifd, y0, rows):
        if rows:
            seen.append((ifd["width"], y0, rows))
        return real(path, ifd, y0, rows)
    monkeypatch.setattr(pbx, "tiff_band_spec", spy)
    return seen


def test_tiff_source_on_a_sparse_service(band_reads):
    entry = next(e for e in FILES if e["file"].startswith("pyramid"))
    path = os.path.join(GOLD, entry["file"])
    full, lv2 = expected(entry, "0"), expected(entry, "2")
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({41: path})
        assert svc.residency_stats()["bands"] == 0
        # rows 20..79 of level 0: bands 1..4
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(41, 0, 0, 0, 10, 20, 100, 60), src).get_tile()
        assert body == full[20:80, 10:110].tobytes()
        assert svc.residency_stats()["bands"] == 4 and svc.residency_stats()["planes"] == 0
        assert band_reads == [(150, 16 * k, 16) for k in (1, 2, 3, 4)]
        pid = svc.lookup_plane(41, 0, 0, 0)[0]
        R, A = pbx.BS_READY, pbx.BS_ABSENT
        assert svc.band_info(pid) == (16, [A, R, R, R, R, A, A])
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(41, 0, 0, 0, 0, 33, 150, 40), src).get_tile()
        assert body == full[33:73].tobytes()
        assert svc.residency_stats()["bands"] == 4 and len(band_reads) == 4  # nothing more was loaded
        # stored level 2 (38 x 25) is OMERO resolution 0
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(41, 0, 0, 0, 3, 2, 30, 20, resolution=0), src).get_tile()
        assert body == lv2[2:22, 3:33].tobytes()
        assert band_reads[4:] == [(38, 0, 16), (38, 16, 9)] and svc.residency_stats()["bands"] == 6
        status, payload, _ = pbx.handle_get_tile(svc, pbx.TileCtx(41, 0, 0, 0, 0, 90, 8, 8).to_json(), src)
        assert status == 200 and payload == full[90:98, :8].tobytes()
        assert pbx.TileRequestHandler(svc, pbx.TileCtx(42, 0, 0, 0, 0, 0, 16, 16), src).get_tile() is None


def test_evicted_band_is_decoded_again(band_reads):
    entry = next(e for e in FILES if e["file"].startswith("pyramid"))
    path = os.path.join(GOLD, entry["file"])
    full = expected(entry, "0")
    band_bytes = 512 * 16 + 256  # 150 uint16 samples pitch to 512 bytes
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({43: path})
        svc.set_residency_budget(2 * band_bytes + 100)
        for n, k in enumerate([0, 1, 2, 0]):
            body = pbx.TileRequestHandler(svc, pbx.TileCtx(43, 0, 0, 0, 5, 16 * k + 2, 140, 12), src).get_tile()
            assert body == full[16 * k + 2:16 * k + 14, 5:145].tobytes()
            assert band_reads[-1] == (150, 16 * k, 16) and len(band_reads) == n + 1
            s = svc.residency_stats()
            assert s["resident_bytes"] <= s["budget"] and s["bands"] == min(n + 1, 2)
        assert svc.residency_stats()["band_evictions"] == 2


def test_ome_plane_loads_its_own_band_only(band_reads):
    entry = next(e for e in FILES if "ome" in e)
    path = os.path.join(GOLD, entry["file"])
    want = expected(entry, "0", "1,2,1")
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({44: path})
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(44, 1, 2, 1, 4, 20, 60, 10), src).get_tile()
        assert body == want[20:30, 4:64].tobytes()
        assert band_reads == [(70, 16, 16)] and svc.residency_stats()["bands"] == 1
        assert svc.lookup_plane(44, 0, 0, 0) is None and svc.lookup_plane(44, 1, 2, 1) is not None
        assert pbx.TileRequestHandler(svc, pbx.TileCtx(44, 2, 0, 0, 0, 0, 8, 8), src).get_tile() is None
