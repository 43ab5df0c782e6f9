"""Lossless JPEG 2000 TIFF segments (Compression 33003 / 33004 / 33005 / 34712) on the GPU:
k_tiff_j2k_packets, k_tiff_j2k_blocks, k_tiff_j2k_idwt and k_tiff_j2k_place against the pixels the
streams were encoded from, which is what PIL (OpenJPEG) decodes from them too and what
tests/test_tiff_j2k_host.py holds tests/_tiff_j2k.py's model to.  Every comparison is exact: the
reversible path has no tolerance anywhere."""
import itertools
import os

import numpy as np
import pytest

import _tiff_j2k as J
import pbx
from _tiff_j2k import GOLD, be_bytes, expected

pytestmark = pytest.mark.gpu

FILES = J.manifest()
IDS = [f["file"] for f in FILES]
_ids = itertools.count(8_500_000)  # disjoint from the other test files (shared service)
PROGRESSIONS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]


def noise(w, h, seed, dtype=np.uint8, samples=1):
    rng = np.random.default_rng(seed)
    shape = (h, w) if samples == 1 else (h, w, samples)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, shape, dtype=dtype)


def smooth(w, h, seed, dtype=np.uint16):
    """Poisson-like counts on a smooth background: few significant bit-planes, long runs."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    lam = 40 + 30 * np.sin(x / 9.0 + seed) * np.cos(y / 11.0)
    return rng.poisson(lam).astype(dtype)


def ptype(a):
    return pbx.UINT8 if a.dtype == np.uint8 else pbx.UINT16


def rows_of(svc, image, y0, rows, w, z=0, c=0, t=0, resolution=None):
    st, body = svc.get_tile(pbx.TileCtx(image, z, c, t, 0, y0, w, rows, resolution=resolution))
    assert st == pbx.OK, st
    return body


def specs_of(page, image, samples=None, big_endian=False):
    """register_tiff_planes specs straight from a page_of() page: one per sample."""
    h, w, s, tile = page["length"], page["width"], page["spp"], page["tile"]
    base = dict(image_id=image, z=0, t=0, pixel_type=ptype(page["array"]), size_x=w, size_y=h, big_endian=big_endian,
                seg_w=tile[0] if tile else w, seg_h=tile[1] if tile else min(page["rows_per_strip"], h),
                tiled=tile is not None, compression=pbx.TIFF_J2K, predictor=1, j2k=True)
    segs = page["segments"]
    if page["planar"] == 2 and s > 1:
        n = len(segs) // s
        return [dict(base, c=c, samples_per_pixel=1, sample=0, segments=pbx.pack_chunks(segs[c * n:(c + 1) * n]))
                for c in (samples or range(s))]
    packed = pbx.pack_chunks(segs)
    return [dict(base, c=c, samples_per_pixel=s, sample=c, segments=packed) for c in (samples or range(s))]


def check_pages(svc, pages, what="", big_endian=False):
    """Every page a layer of ONE registration; every plane equal to the array it was encoded from."""
    specs, wants = [], []
    for page in pages:
        sp = specs_of(page, next(_ids), big_endian=big_endian)
        a = page["array"]
        specs += sp
        wants += [a[:, :, c] if a.ndim == 3 else a for c in range(len(sp))]
    ids = svc.register_tiff_planes(specs)
    try:
        for k, (pid, want) in enumerate(zip(ids, wants)):
            got = np.frombuffer(svc.read_plane_be(pid, want.nbytes), want.dtype.newbyteorder(">")).reshape(want.shape)
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
                assert service.read_plane_be(pid, want.nbytes) == be_bytes(want), (entry["file"], level, z, c, t)
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
                pid = service.create_sparse_plane(image, 0, 0, 0, ptype(want), w, h, rows, big_endian=d["byteorder"] == ">")
                try:
                    for r0 in range(0, h, rows):
                        n = min(rows, h - r0)
                        sp = pbx.tiff_band_spec(path, d, r0, n, sample=s)
                        assert sp["j2k"] and sp["compression"] == pbx.TIFF_J2K
                        service.band_write_tiff(pid, r0, n, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"],
                                                sp["predictor"], sp["segments"], j2k=True,
                                                samples_per_pixel=sp["samples_per_pixel"], sample=sp["sample"])
                        assert rows_of(service, image, r0, n, w) == be_bytes(want[r0:r0 + n]), (entry["file"], s, r0)
                    assert set(service.band_info(pid)[1]) == {pbx.BS_READY}
                finally:
                    service.release_plane(pid)


# ------------------------------------------------------------------------------ geometry
KINDS = {"u8": dict(dtype=np.uint8), "u16": dict(dtype=np.uint16), "rgb": dict(samples=3, mct=0),
         "rct": dict(samples=3, mct=1)}


def kind_array(kind, w, h, seed):
    k = KINDS[kind]
    return noise(w, h, seed, k.get("dtype", np.uint8), k.get("samples", 1))


@pytest.mark.parametrize("rps", [8, 16])
@pytest.mark.parametrize("kind", list(KINDS))
def test_strip_sweep(service, kind, rps):
    """Widths 1 .. 34 x heights 1 .. 18: sub-bands of no samples, resolutions of one row or column,
    short last strips, code blocks alternating between 4 x 4 and 64 x 64.  One registration per
    width."""
    mct = KINDS[kind].get("mct", 0)
    for w in range(1, 35):
        pages = []
        for h in range(1, 19):
            cb = (4, 4) if (w + h) & 1 else (64, 64)
            pages.append(J.page_of(kind_array(kind, w, h, 100 * w + h), rows_per_strip=rps, codeblock_size=cb, mct=mct,
                                   num_resolutions=6, progression=PROGRESSIONS[(w + h) % 5]))
        check_pages(service, pages, "%s w=%d" % (kind, w))


@pytest.mark.parametrize("tile", [16, 64])
@pytest.mark.parametrize("shape", [(40, 30), (100, 70)], ids=["40x30", "100x70"])
def test_clipped_tiles(service, tile, shape):
    w, h = shape
    check_pages(service, [J.page_of(kind_array(k, w, h, tile + w), tile=(tile, tile), mct=KINDS[k].get("mct", 0),
                                    num_resolutions=4) for k in KINDS], "tiles %d" % tile)


@pytest.mark.parametrize("cb", [64, 32])
def test_one_tile_of_256(service, cb):
    """Five levels, 16 (or 64) code blocks in the largest sub-bands, tag trees of three (four) levels."""
    pages = [J.page_of(smooth(256, 256, 7), tile=(256, 256), codeblock_size=(cb, cb), num_resolutions=6),
             J.page_of(noise(256, 256, 8, samples=3), tile=(256, 256), codeblock_size=(cb, cb), num_resolutions=6, mct=1)]
    check_pages(service, pages, "256 / %d" % cb)


@pytest.mark.parametrize("cb", [(1024, 4), (4, 1024)], ids=["1024x4", "4x1024"])
def test_long_code_blocks(service, cb):
    w, h = (2048, 16) if cb[0] == 1024 else (16, 2048)
    check_pages(service, [J.page_of(noise(w, h, 9, np.uint16), tile=(w, h), codeblock_size=cb, num_resolutions=2)], str(cb))


def test_extreme_tiles(service):
    """All zero, all 32768 (after the level shift every coefficient is zero: every code block is
    left out of its packet), all 65535, and a 0 / 65535 checkerboard, which has the most
    bit-planes the path can meet."""
    y, x = np.mgrid[0:48, 0:48]
    arrays = [np.zeros((48, 48), np.uint16), np.full((48, 48), 32768, np.uint16), np.full((48, 48), 65535, np.uint16),
              (((x + y) & 1) * 65535).astype(np.uint16), np.zeros((48, 48), np.uint8), np.full((48, 48, 3), 255, np.uint8)]
    check_pages(service, [J.page_of(a, tile=(48, 48), num_resolutions=4) for a in arrays] +
                [J.page_of(arrays[3], tile=(48, 48), num_resolutions=1)], "extremes")


@pytest.mark.parametrize("prog", PROGRESSIONS)
def test_progressions(service, prog):
    pages = [J.page_of(noise(40, 30, 11, samples=3), tile=(32, 32), mct=m, progression=prog, num_resolutions=3) for m in (0, 1)]
    pages.append(J.page_of(noise(40, 30, 12, np.uint16), rows_per_strip=16, progression=prog, num_resolutions=4,
                           precinct_size=(64, 64), codeblock_size=(16, 16)))
    assert J.parse(pages[-1]["segments"][0])["scod"] & 1
    check_pages(service, pages, prog)


def test_layers_with_different_cods_and_byte_orders(service):
    a8, a16 = noise(40, 30, 13), noise(40, 30, 14, np.uint16)
    pages = [J.page_of(a8, tile=(16, 16), num_resolutions=1), J.page_of(a16, rows_per_strip=8, num_resolutions=3),
             J.page_of(a16, tile=(32, 32), codeblock_size=(8, 32), num_resolutions=5, progression="CPRL"),
             J.page_of(noise(40, 30, 15, samples=3), tile=(16, 16), mct=1, codeblock_size=(4, 4), num_resolutions=2)]
    check_pages(service, pages, "little-endian planes")
    check_pages(service, pages, "big-endian planes", big_endian=True)


def test_one_sample_of_three(service):
    a = noise(40, 30, 17, samples=3)
    pg = J.page_of(a, tile=(16, 16), mct=1, num_resolutions=3)
    image = next(_ids)
    (pid,) = service.register_tiff_planes(specs_of(pg, image, samples=[1]))
    try:
        assert service.read_plane_be(pid, 40 * 30) == a[:, :, 1].tobytes()
        assert service.lookup_plane(image, 0, 0, 0) is None and service.lookup_plane(image, 0, 2, 0) is None
    finally:
        service.release_plane(pid)


@pytest.mark.parametrize("tile", [None, (16, 16)], ids=["strips", "tiles"])
@pytest.mark.parametrize("kind", ["rct", "rgb"])
def test_one_sample_band_write(service, kind, tile):
    """Rows 7 .. 13 of a 21-row plane from two pieces cut inside a segment; sentinel rows around
    them and sentinel sibling planes stay as they were."""
    S, h, w = 3, 21, 65
    a = kind_array(kind, w, h, 23)
    pg = J.page_of(a, tile=tile, rows_per_strip=8, mct=KINDS[kind]["mct"], num_resolutions=3)
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
                service.band_write_tiff(pids[target], y0, rows, sp0["seg_w"], seg_h, tile is not None, pbx.TIFF_J2K, 1,
                                        piece, samples_per_pixel=S, sample=target, j2k=True)
            assert service.band_info(pids[target])[1] == [pbx.BS_READY]
            got = rows_of(service, image, 0, h, w, c=target)
            assert got[:7 * w] == b"\xA5" * (7 * w) and got[14 * w:] == b"\x5A" * (7 * w)
            assert got[7 * w:14 * w] == a[7:14, :, target].tobytes()
            for c in range(S):
                if c != target:
                    assert rows_of(service, image, 0, h, w, c=c) == bytes([0x30 + c]) * (h * w)
        finally:
            for pid in pids:
                service.release_plane(pid)


# ------------------------------------------------------------------------------ refusals
def bad_streams():
    """(name, w, h, stream, decoder code): streams only the device can refuse."""
    w, h = 40, 24
    good = J.encode(noise(w, h, 31, np.uint16), num_resolutions=3, codeblock_size=(16, 16))
    hd = J.parse(good)
    found = J.packets(good, hd, J.geometry(hd)[0])
    first = min(v[0] for comp in found for band in comp for v in band.values())  # the first code-block byte
    last = max(v[0] + v[1] for comp in found for band in comp for v in band.values())
    assert last == hd["end"]
    out = [("cut inside a packet header", w, h, good[:hd["data"] + 1], 1),
           ("cut inside code-block data", w, h, good[:last - 5], 1)]
    # the first packet (resolution 0: one block) begins: 1 non-empty, 1 included, then the
    # zero-bit-plane tag tree's zeros up to a 1, then the passes codeword
    zeros = bytearray(good)
    zeros[hd["data"]] = 0xC0
    zeros[hd["data"] + 1:hd["data"] + 6] = bytes(5)  # 46 zeros: more missing bit-planes than the band has
    out.append(("zero bit-planes above Mb", w, h, bytes(zeros), 3))
    z0 = found[0][0][(0, 0)][3]
    passes = bytearray(good)
    assert hd["data"] + 3 < first
    # non-empty, included, z0 zeros and a one, then 1111 11111 1111111: 164 passes
    bits = "11" + "0" * z0 + "1" + "1" * 16
    patch, i = bytearray(), 0
    while i < len(bits):  # B.10.1: the byte after an FF holds 7 bits
        n = 7 if patch and patch[-1] == 0xFF else 8
        patch.append(int(bits[i:i + n].ljust(n, "0"), 2))
        i += n
    passes[hd["data"]:hd["data"] + len(patch)] = patch
    out.append(("more passes than bit-planes", w, h, bytes(passes), 3))
    return out


@pytest.mark.parametrize("case", bad_streams(), ids=lambda c: c[0])
def test_device_refusals(service, case):
    name, w, h, stream, code = case
    image = next(_ids)
    spec = dict(image_id=image, z=0, c=0, t=0, pixel_type=pbx.UINT16, size_x=w, size_y=h, big_endian=False, seg_w=w, seg_h=h,
                tiled=False, compression=pbx.TIFF_J2K, predictor=1, j2k=True, segments=pbx.pack_chunks([stream]))
    with pytest.raises(pbx.PbxError, match=r"corrupt segment stream 0 \(j2k, decoder code %d\)" % code) as e:
        service.register_tiff_planes([spec])
    assert e.value.status == 400
    assert service.lookup_plane(image, 0, 0, 0) is None
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT16, w, h, h, big_endian=False)
    try:
        with pytest.raises(pbx.PbxError, match="corrupt segment stream") as e:
            service.band_write_tiff(pid, 0, h, w, h, False, pbx.TIFF_J2K, 1, spec["segments"], j2k=True)
        assert e.value.status == 400
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT]
    finally:
        service.release_plane(pid)


def test_injected_upload_failure(service):
    a = noise(40, 30, 37, samples=3)
    sp = specs_of(J.page_of(a, tile=(16, 16), mct=1, num_resolutions=3), next(_ids))[0]
    image = sp["image_id"]
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, 40, 30, 30, big_endian=False)
    try:
        service.test_fail_band_write(1)
        with pytest.raises(pbx.PbxError):
            service.band_write_tiff(pid, 0, 30, 16, 16, True, pbx.TIFF_J2K, 1, sp["segments"], j2k=True, samples_per_pixel=3,
                                    sample=0)
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT]
        service.band_write_tiff(pid, 0, 30, 16, 16, True, pbx.TIFF_J2K, 1, sp["segments"], j2k=True, samples_per_pixel=3,
                                sample=0)
        assert rows_of(service, image, 0, 30, 40) == a[:, :, 0].tobytes()
    finally:
        service.release_plane(pid)


def test_flipped_bits(service):
    """Garbage code-block bytes cannot be an error in JPEG 2000; a flipped bit in a packet header
    can.  The write succeeds or is a 400, and the rows and planes around it keep their bytes
    either way."""
    w, h = 48, 48
    pg = J.page_of(noise(w, h, 41), rows_per_strip=16, num_resolutions=3, codeblock_size=(16, 16))
    seg = pg["segments"][1]  # the strip of rows 16 .. 31
    d = J.parse(seg)["data"]
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
                service.band_write_tiff(pids[0], 16, 16, w, 16, False, pbx.TIFF_J2K, 1, [bytes(bad)], j2k=True)
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
def test_tiff_source_serves_a_pyramid(oracle):
    entry = next(e for e in FILES if e["file"].startswith("pyramid"))
    path = os.path.join(GOLD, entry["file"])
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({71: path})
        want = expected(entry, 0, "0,0,0")
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(71, 0, 0, 0, 5, 30, 90, 20), src).get_tile()
        assert body == be_bytes(want[30:50, 5:95])
        png = pbx.TileRequestHandler(svc, pbx.TileCtx(71, 0, 0, 0, 8, 33, 40, 10, format="png"), src).get_tile()
        r, px, _ = oracle.png_decode(png)
        assert r == 0 and px == be_bytes(want[33:43, 8:48])
        # rows 30 .. 49 lie in bands 1, 2 and 3 of 16 rows: only those were read
        states = svc.band_info(svc.lookup_plane(71, 0, 0, 0)[0])[1]
        assert [s == pbx.BS_READY for s in states] == [False, True, True, True, False], states
        # stored level 1 is resolution 1 of 3 (resolution 0 is the smallest)
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(71, 0, 0, 0, 3, 10, 40, 20, resolution=1), src).get_tile()
        assert body == be_bytes(expected(entry, 1, "0,0,0")[10:30, 3:43])


def test_a_file_that_mixes_j2k_and_deflate_levels(service, tmp_path):
    """register_tiff_image on a JPEG 2000 page with a deflate SubIFD: two registrations behind one
    call, and when the JPEG 2000 one is refused nothing of the other stays registered."""
    import _tiff_rgb as R
    a = noise(40, 30, 51, samples=3)
    low = np.ascontiguousarray(a[::2, ::2])
    sub = R.page_of(low, compression=pbx.TIFF_DEFLATE, tile=(16, 16))
    pg = J.page_of(a, 33005, tile=(16, 16), mct=1, num_resolutions=3)
    path = str(tmp_path / "mixed.tif")
    J.write_tiff(path, [dict(pg, subifds=[sub])])  # (the other writer's page has the keys ours reads)
    image = next(_ids)
    ids = service.register_tiff_image(path, image)
    try:
        for c in range(3):
            assert service.read_plane_be(ids[0][(0, c, 0)], 40 * 30) == a[:, :, c].tobytes()
            assert service.read_plane_be(ids[1][(0, c, 0)], 20 * 15) == low[:, :, c].tobytes()
    finally:
        for planes in ids.values():
            for pid in planes.values():
                service.release_plane(pid)
    segs = list(pg["segments"])
    segs[1] = segs[1][:J.parse(segs[1])["data"] + 1]  # cut inside the first packet header: the device refuses it
    J.write_tiff(path, [dict(pg, segments=segs, subifds=[sub])])
    image = next(_ids)
    with pytest.raises(pbx.PbxError, match="corrupt segment stream"):
        service.register_tiff_image(path, image)
    assert all(service.lookup_plane(image, 0, c, 0, level) is None for c in range(3) for level in (0, 1))
