"""Float TIFF stored with the floating-point predictor (Predictor = 3: k_tiff_fpunpred_place) and
Zstandard TIFF (Compression = 50000: k_zarr_zstd behind the TIFF planner) on the GPU, at
registration (pbx_planes_register_tiff) and band by band (pbx_band_write_tiff).

Expected bytes: the fixtures' .npy (tests/golden/tiff_fp, written by tifffile and libtiff), or the
numpy array a segment was encoded from by tests/_tiff_fp.py (whose rule tests/test_tiff_fp_host.py
pins against those files and against libtiff).  Everything is compared byte for byte: the kernel
sweep runs on uniform random bit patterns (NaN payloads, +-0, infinities, denormals).

The kernel walks 64 / bpp samples a lane a step: a wave step is 1024 float32 or 512 float64
samples, so the widths below end one under, at and one over one and two steps of either."""
import itertools
import os

import numpy as np
import pytest

import _oracle as O
import _tiff_fp as F
import _tiff_rgb as R
import pbx

pytestmark = pytest.mark.gpu

FILES = F.manifest()
IDS = [f["file"] for f in FILES]
_ids = itertools.count(7_900_000)  # disjoint from the other test files (shared service)
COMPS = [pbx.TIFF_NONE, pbx.TIFF_DEFLATE, pbx.TIFF_LZW, pbx.TIFF_ZSTD]
FP_TYPES = [("<f4", pbx.FLOAT), (">f4", pbx.FLOAT), ("<f8", pbx.DOUBLE), (">f8", pbx.DOUBLE)]
WIDTHS = [1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]
BAND = 7


def be_bytes(a):
    return np.ascontiguousarray(a).astype(a.dtype.newbyteorder(">")).tobytes()


def random_bits(rng, dt, h, w):
    dt = np.dtype(dt)
    return rng.integers(0, 256, h * w * dt.itemsize, dtype=np.uint8).view(dt).reshape(h, w)


def rows_of(svc, image, y0, rows, w, z=0, c=0, t=0):
    st, body = svc.get_tile(pbx.TileCtx(image, z, c, t, 0, y0, w, rows))
    assert st == pbx.OK, st
    return body


def plane_spec(a, tile, rps, comp, predictor, pad=None, checksum=False):
    """A plane's geometry and every one of its segments (tests/_tiff_fp.py)."""
    segs = [F.compress(s, comp, checksum) if comp == F.ZSTD else F.compress(s, comp)
            for s in F.segments_of(a, tile, rps, predictor, pad)]
    return dict(size_x=a.shape[1], size_y=a.shape[0], seg_w=tile[0] if tile else a.shape[1],
                seg_h=tile[1] if tile else rps, tiled=tile is not None, compression=comp, predictor=predictor,
                segs=segs)


def reg_spec(sp, pt, bo, image):
    return dict(image_id=image, z=0, c=0, t=0, pixel_type=pt, size_x=sp["size_x"], size_y=sp["size_y"],
                seg_w=sp["seg_w"], seg_h=sp["seg_h"], tiled=sp["tiled"], compression=sp["compression"],
                predictor=sp["predictor"], big_endian=bo == ">", segments=sp["segs"])


def write_piece(svc, pid, sp, y0, rows, **kw):
    gx = -(-sp["size_x"] // sp["seg_w"]) if sp["tiled"] else 1
    segs = sp["segs"][(y0 // sp["seg_h"]) * gx:-(-(y0 + rows) // sp["seg_h"]) * gx]
    return svc.band_write_tiff(pid, y0, rows, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"],
                               sp["predictor"], segs, **kw)


# ------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_whole(service, entry):
    """register_tiff_image: every plane of every level (SubIFDs, planar samples) in one call."""
    image = next(_ids)
    ids = service.register_tiff_image(os.path.join(F.GOLD, entry["file"]), image)
    try:
        assert sorted(ids) == sorted(int(k) for k in entry["planes"])
        for level, planes in ids.items():
            assert sorted("%d,%d,%d" % p for p in planes) == sorted(entry["planes"][str(level)])
            for (z, c, t), pid in planes.items():
                want = F.expected(entry["planes"][str(level)]["%d,%d,%d" % (z, c, t)])
                assert service.read_plane_be(pid, want.nbytes) == want.tobytes(), (entry["file"], level, c)
    finally:
        for planes in ids.values():
            for pid in planes.values():
                service.release_plane(pid)


@pytest.mark.parametrize("B", [16, 40, 0], ids=["16", "40", "whole"])
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_band_by_band(service, entry, B):
    """16 puts several bands in one segment row, 40 straddles segment rows, the last is one band
    of the plane's height.  (pbx_plane_read_be does not read sparse planes: the rows come back as
    one raw tile of the plane's size, which is the same big-endian bytes.)"""
    path = os.path.join(F.GOLD, entry["file"])
    main = pbx.tiff_ifds(path)[0]
    for level, ifd in enumerate([main] + main["subifds"]):
        for key, ref in sorted(entry["planes"][str(level)].items()):
            sample = int(key.split(",")[1])
            want = F.expected(ref)
            h, w = want.shape
            rows = B or h
            head = pbx.tiff_band_spec(path, ifd, 0, 0, sample=sample)
            assert head["segments"] is None
            image = next(_ids)
            pid = service.create_sparse_plane(image, 0, 0, 0, head["pixel_type"], w, h, rows,
                                              big_endian=head["big_endian"])
            try:
                for r0 in range(0, h, rows):
                    n = min(rows, h - r0)
                    sp = pbx.tiff_band_spec(path, ifd, r0, n, sample=sample)
                    service.band_write_tiff(pid, r0, n, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"],
                                            sp["predictor"], sp["segments"],
                                            samples_per_pixel=sp["samples_per_pixel"], sample=sp["sample"])
                assert set(service.band_info(pid)[1]) == {pbx.BS_READY}
                assert rows_of(service, image, 0, h, w) == want.tobytes(), (entry["file"], level, sample)
            finally:
                service.release_plane(pid)


# ------------------------------------------------------------ the kernel on full-range bytes
def sweep_layouts(w):
    """Strips of 2 rows at every width; 16 x 16 and 64 x 64 tiles where the plane's width and
    height are no tile multiples (the edge tiles' padding is random, not zero: a carry taken over
    the visible width only gives wrong bytes in the planes after the first)."""
    layouts = [(None, 5, 2)]
    if w in (17, 63, 65, 257):
        layouts += [((16, 16), 37, None), ((64, 64), 70, None)]
    return layouts


@pytest.mark.parametrize("dt,pt", FP_TYPES, ids=[d for d, _ in FP_TYPES])
def test_fpunpred_place_at_registration(service, dt, pt):
    n = [d for d, _ in FP_TYPES].index(dt)  # the seed, and where the codecs' cycle starts
    rng = np.random.default_rng(100 + n)
    specs, wants = [], []
    for w in WIDTHS:
        for tile, h, rps in sweep_layouts(w):
            a = random_bits(rng, dt, h, w)
            sp = plane_spec(a, tile, rps, COMPS[n % 4], 3, pad=rng)
            n += 1
            specs.append(reg_spec(sp, pt, dt[0], next(_ids)))
            wants.append(be_bytes(a))
    assert {s["compression"] for s in specs} == set(COMPS)
    ids = service.register_tiff_planes(specs)
    try:
        for pid, want, sp in zip(ids, wants, specs):
            assert service.read_plane_be(pid, len(want)) == want, (sp["size_x"], sp["seg_w"], sp["compression"])
    finally:
        for pid in ids:
            service.release_plane(pid)


@pytest.mark.parametrize("dt,pt", FP_TYPES, ids=[d for d, _ in FP_TYPES])
def test_fpunpred_place_in_bands(service, dt, pt):
    """Bands of 7 rows, the first written in two pieces at a row that is no segment boundary."""
    n = [d for d, _ in FP_TYPES].index(dt) + 1
    rng = np.random.default_rng(200 + n)
    used = set()
    for w in WIDTHS:
        for tile, h, rps in sweep_layouts(w):
            a = random_bits(rng, dt, h, w)
            comp = COMPS[n % 4]
            n += 1
            used.add(comp)
            sp = plane_spec(a, tile, rps, comp, 3, pad=rng)
            want = be_bytes(a)
            image = next(_ids)
            pid = service.create_sparse_plane(image, 0, 0, 0, pt, w, h, BAND, big_endian=dt[0] == ">")
            try:
                for r0 in range(0, h, BAND):
                    r1 = min(r0 + BAND, h)
                    cuts = [r0, r0 + 3, r1] if r0 == 0 else [r0, r1]  # 3: inside a strip of 2, a tile of 16
                    for lo, hi in zip(cuts[:-1], cuts[1:]):
                        write_piece(service, pid, sp, lo, hi - lo)
                assert rows_of(service, image, 0, h, w) == want, (w, tile, comp)
            finally:
                service.release_plane(pid)
    assert used == set(COMPS)


@pytest.mark.parametrize("comp", COMPS, ids=["stored", "deflate", "lzw", "zstd"])
@pytest.mark.parametrize("tile", [None, (64, 64)], ids=["strips", "tiles"])
def test_rows_outside_the_piece_survive(service, tile, comp):
    """Rows 0..9 and 50..69 of a one-band plane are sentinel bytes from band_write; the piece
    [10, 50) begins and ends inside a segment (strips of 16, tiles of 64), keeps only part of
    those segments' rows, and must leave the sentinels alone."""
    h, w = 70, 65
    for dt, pt in (("<f4", pbx.FLOAT), (">f8", pbx.DOUBLE)):
        a = random_bits(np.random.default_rng(31), dt, h, w)
        row = w * a.dtype.itemsize
        sp = plane_spec(a, tile, 16, comp, 3, pad=np.random.default_rng(32))
        image = next(_ids)
        pid = service.create_sparse_plane(image, 0, 0, 0, pt, w, h, h, big_endian=dt[0] == ">")
        try:
            service.band_write(pid, 0, 10, b"\xA5" * (10 * row))
            service.band_write(pid, 50, 20, b"\x5A" * (20 * row))
            assert service.band_info(pid)[1] == [pbx.BS_LOADING]
            ms = write_piece(service, pid, sp, 10, 40, timing=True)
            assert len(ms) == 2 and ms[1] > 0
            assert service.band_info(pid)[1] == [pbx.BS_READY]
            got = rows_of(service, image, 0, h, w)
            assert got[:10 * row] == b"\xA5" * (10 * row)
            assert got[50 * row:] == b"\x5A" * (20 * row)
            assert got[10 * row:50 * row] == be_bytes(a[10:50])
        finally:
            service.release_plane(pid)


def test_many_predictor3_layers_in_one_call(service):
    """One registration with Predictor 3 planes of both sample sizes and byte orders next to
    Predictor 1 and 2 planes: every layer has its own destination entry."""
    rng = np.random.default_rng(7)
    specs, wants = [], []
    for k, (dt, pt, pred) in enumerate([("<f4", pbx.FLOAT, 3), (">f8", pbx.DOUBLE, 3), ("<u2", pbx.UINT16, 2),
                                        (">f4", pbx.FLOAT, 3), ("<f8", pbx.DOUBLE, 1), ("<f8", pbx.DOUBLE, 3)]):
        a = random_bits(rng, dt, 40 + k, 70 + 3 * k)
        sp = plane_spec(a, (32, 32) if k % 2 else None, 16, COMPS[k % 4], pred, pad=rng)
        specs.append(reg_spec(sp, pt, dt[0], next(_ids)))
        wants.append(be_bytes(a))
    ids, ms = service.register_tiff_planes(specs, timing=True)
    try:
        assert ms[1] > 0
        for pid, want in zip(ids, wants):
            assert service.read_plane_be(pid, len(want)) == want
    finally:
        for pid in ids:
            service.release_plane(pid)


# --------------------------------------------------------- zstd behind Predictor 1 and 2
INT_TYPES = [("u1", pbx.UINT8), ("<i2", pbx.INT16), (">u2", pbx.UINT16), ("<u4", pbx.UINT32), (">i4", pbx.INT32)]


@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("dt,pt", INT_TYPES, ids=[d for d, _ in INT_TYPES])
def test_zstd_segments_of_integer_planes(service, dt, pt, predictor):
    rng = np.random.default_rng(50 + predictor)
    bo = ">" if dt[0] == ">" else "<"
    for w, tile, h, rps in ((65, None, 21, 8), (150, (64, 64), 100, None), (1025, None, 5, 2)):
        # smooth samples (sequences, repeated offsets, compressed literals) with noise in the low bits
        base = (np.arange(w)[None, :] // 3 + np.arange(h)[:, None] * 5 + rng.integers(0, 4, (h, w)))
        a = base.astype(np.dtype(dt).newbyteorder("=")).astype(dt)
        sp = plane_spec(a, tile, rps, F.ZSTD, predictor, checksum=True)
        want = be_bytes(a)
        pid, = service.register_tiff_planes([reg_spec(sp, pt, bo, next(_ids))])
        try:
            assert service.read_plane_be(pid, len(want)) == want, (w, "registration")
        finally:
            service.release_plane(pid)
        image = next(_ids)
        pid = service.create_sparse_plane(image, 0, 0, 0, pt, w, h, BAND, big_endian=bo == ">")
        try:
            for r0 in range(0, h, BAND):
                write_piece(service, pid, sp, r0, min(BAND, h - r0))
            assert rows_of(service, image, 0, h, w) == want, (w, "bands")
        finally:
            service.release_plane(pid)


@pytest.mark.parametrize("predictor", [1, 2])
def test_zstd_chunky_rgb(service, predictor):
    """k_tiff_split_place behind ZS_ZSTD: RGB uint8, registration and one sample band by band."""
    rng = np.random.default_rng(60 + predictor)
    h, w, S = 45, 70, 3
    a = ((np.arange(w)[None, :, None] + np.arange(h)[:, None, None] * 2 + np.arange(S)[None, None, :] * 40 +
          rng.integers(0, 3, (h, w, S))) & 0xFF).astype(np.uint8)
    for tile, rps in ((None, 8), ((32, 32), None)):
        segs = [F.compress(x, F.ZSTD) for x in R.chunky_segments(a, tile, rps, predictor)]
        image = next(_ids)
        geo = dict(seg_w=tile[0] if tile else w, seg_h=tile[1] if tile else rps, tiled=tile is not None)
        specs = [dict(image_id=image, z=0, c=s, t=0, pixel_type=pbx.UINT8, size_x=w, size_y=h, compression=F.ZSTD,
                      predictor=predictor, segments=pbx.pack_chunks(segs), samples_per_pixel=S, sample=s, **geo)
                 for s in range(S)]
        ids = service.register_tiff_planes(specs)
        try:
            for s, pid in enumerate(ids):
                assert service.read_plane_be(pid, h * w) == a[:, :, s].tobytes(), (tile, s)
        finally:
            for pid in ids:
                service.release_plane(pid)
        image = next(_ids)
        pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, w, h, 20)
        try:
            gx = -(-w // geo["seg_w"]) if tile else 1
            for r0 in range(0, h, 20):
                n = min(20, h - r0)
                piece = segs[(r0 // geo["seg_h"]) * gx:-(-(r0 + n) // geo["seg_h"]) * gx]
                service.band_write_tiff(pid, r0, n, geo["seg_w"], geo["seg_h"], geo["tiled"], F.ZSTD, predictor, piece,
                                        samples_per_pixel=S, sample=1)
            assert rows_of(service, image, 0, h, w) == a[:, :, 1].tobytes()
        finally:
            service.release_plane(pid)


# ------------------------------------------------------------------------------- failures
def smooth_f4(h, w, seed):
    return (np.random.default_rng(seed).poisson(6, (h, w)) * 0.25).astype("<f4")


def damaged(segs, k, case):
    segs = list(segs)
    s = segs[k]
    if case == "flipped checksum bit":   # the frame's last four bytes: its XXH64 content checksum
        segs[k] = s[:-1] + bytes([s[-1] ^ 0x10])
    elif case == "flipped data bit":     # inside the last block's data, past every header
        segs[k] = s[:-8] + bytes([s[-8] ^ 0x04]) + s[-7:]
    else:
        segs[k] = s[:len(s) // 2]
    return segs


CASES = ["flipped checksum bit", "flipped data bit", "truncated"]


@pytest.mark.parametrize("case", CASES)
def test_corrupt_zstd_segment_registers_nothing(service, case):
    a = smooth_f4(32, 100, 8)
    good = plane_spec(a, None, 8, F.ZSTD, 3, checksum=True)
    bad = dict(good, segs=damaged(good["segs"], 2, case))
    before = service.residency_stats()
    g, b = next(_ids), next(_ids)
    match = "segment 2: truncated zstd frame" if case == "truncated" else r"corrupt chunk stream \d+ \(zstd"
    with pytest.raises(pbx.PbxError, match=match) as e:
        service.register_tiff_planes([reg_spec(good, pbx.FLOAT, "<", g), reg_spec(bad, pbx.FLOAT, "<", b)])
    assert e.value.status == 400
    after = service.residency_stats()
    assert (after["planes"], after["resident_bytes"]) == (before["planes"], before["resident_bytes"])
    assert service.lookup_plane(g, 0, 0, 0) is None and service.lookup_plane(b, 0, 0, 0) is None
    ids = service.register_tiff_planes([reg_spec(good, pbx.FLOAT, "<", g), reg_spec(good, pbx.FLOAT, "<", b)])
    try:
        assert all(service.read_plane_be(p, a.nbytes) == be_bytes(a) for p in ids)
    finally:
        for p in ids:
            service.release_plane(p)


@pytest.mark.parametrize("case", CASES)
def test_corrupt_zstd_segment_fails_the_band_load(service, case):
    """The band state is as it was for a refusal on the host (a truncated frame); a stream the
    device rejects fails the band's load like a failed upload: absent again, its HBM returned."""
    a = smooth_f4(64, 100, 9)
    good = plane_spec(a, None, 8, F.ZSTD, 3, checksum=True)
    bad = dict(good, segs=damaged(good["segs"], 5, case))
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.FLOAT, 100, 64, 32, big_endian=False)
    try:
        base = service.residency_stats()["resident_bytes"]
        write_piece(service, pid, good, 32, 5)
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_LOADING]
        held = service.residency_stats()["resident_bytes"]
        assert held > base
        if case == "truncated":
            with pytest.raises(pbx.PbxError, match="segment 1: truncated zstd frame") as ei:
                write_piece(service, pid, bad, 37, 27)
            assert ei.value.status == 400
            assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_LOADING]
            assert service.residency_stats()["resident_bytes"] == held
            write_piece(service, pid, good, 37, 27)
        else:
            with pytest.raises(pbx.PbxError, match=r"corrupt chunk stream \d+ \(zstd") as ei:
                write_piece(service, pid, bad, 37, 27)
            assert ei.value.status == 400
            assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_ABSENT]
            assert service.residency_stats()["resident_bytes"] == base
            assert service.get_tile(pbx.TileCtx(image, 0, 0, 0, 0, 32, 16, 16))[0] == pbx.E_NOT_RESIDENT
            write_piece(service, pid, good, 32, 32)
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_READY]
        assert rows_of(service, image, 32, 32, 100) == be_bytes(a[32:])
    finally:
        service.release_plane(pid)


def test_injected_upload_failure(service):
    a = smooth_f4(64, 100, 10)
    sp = plane_spec(a, (32, 32), None, F.ZSTD, 3)
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.FLOAT, 100, 64, 32, big_endian=False)
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
        assert rows_of(service, image, 0, 32, 100) == be_bytes(a[:32])
    finally:
        service.test_fail_band_write(0)
        service.release_plane(pid)


def test_refusals_of_the_real_calls(service):
    """Predictor 3 on an integer plane: 400 at registration and in a band write, the band untouched."""
    a = np.arange(40 * 16, dtype="<u4").reshape(16, 40)
    sp = dict(plane_spec(a.view("<f4"), None, 8, pbx.TIFF_NONE, 3))
    with pytest.raises(pbx.PbxError, match=r"bad predictor 3 \(the floating-point predictor\) on a plane of integer") as e:
        service.register_tiff_planes([reg_spec(sp, pbx.UINT32, "<", next(_ids))])
    assert e.value.status == 400
    pid = service.create_sparse_plane(next(_ids), 0, 0, 0, pbx.INT32, 40, 16, 16, big_endian=False)
    try:
        with pytest.raises(pbx.PbxError, match="bad predictor 3") as e:
            write_piece(service, pid, sp, 0, 16)
        assert e.value.status == 400 and service.band_info(pid)[1] == [pbx.BS_ABSENT]
    finally:
        service.release_plane(pid)


# ------------------------------------------------------------------- behind the handler
def test_tiff_source_on_a_sparse_service():
    """A float32 zstd + Predictor 3 file behind TileRequestHandler: raw and TIFF tiles are the
    oracle's for the .npy plane, and only the bands the rows cover are loaded."""
    entry = next(e for e in FILES if e["file"] == "float_tiles_zstd_p3_II.tif")
    path = os.path.join(F.GOLD, entry["file"])
    want = F.expected(entry["planes"]["0"]["0,0,0"])
    h, w = want.shape
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({51: path})
        assert svc.residency_stats()["bands"] == 0
        for fmt, ofmt in ((None, O.FMT_RAW), ("tif", O.FMT_TIF)):
            x, y, tw, th = 10, 20, 100, 60
            body = pbx.TileRequestHandler(svc, pbx.TileCtx(51, 0, 0, 0, x, y, tw, th, format=fmt), src).get_tile()
            st, ref, _, _ = O.get_tile(want, True, O.FLOAT, w, h, x, y, tw, th, ofmt)
            assert st == 0 and body == ref, fmt
            assert svc.residency_stats()["bands"] == 4 and svc.residency_stats()["planes"] == 0
        pid = svc.lookup_plane(51, 0, 0, 0)[0]
        R_, A = pbx.BS_READY, pbx.BS_ABSENT
        assert svc.band_info(pid) == (16, [A, R_, R_, R_, R_, A, A])
        status, payload, _ = pbx.handle_get_tile(svc, pbx.TileCtx(51, 0, 0, 0, 0, 90, 8, 8).to_json(), src)
        assert status == 200 and payload == want[90:98, :8].tobytes()
