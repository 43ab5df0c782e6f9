"""Lossy JPEG 2000 TIFF segments (9/7 wavelet, scalar quantisation, ICT) on the GPU:
k_tiff_j2k_blocks' midpoint magnitudes and dequantising store, k_tiff_j2k_idwt97 and
k_tiff_j2k_place's float branch.

Two yardsticks.  The CPU hook (pbx_test_tiff_j2k_decode) calls the very functions the kernels call
(tiff_j2k_dev.h), in their order, so generated streams are held to its bytes, exactly.  The hook
in turn is held to tests/_tiff_j2k97.py's float64 model by tests/test_tiff_j2k97_host.py, and the
fixtures of tests/golden/tiff_j2k97/ carry that model's rounded values and in-window masks, so
the kernels are held to the model there too, with no model run on this machine."""
import itertools
import os

import numpy as np
import pytest

import _tiff_j2k as J
import _tiff_j2k97 as M
import pbx
from test_gpu_tiff_j2k import KINDS, PROGRESSIONS, kind_array, noise, ptype, rows_of, smooth, specs_of

pytestmark = pytest.mark.gpu

FILES = M.manifest()
IDS = [f["file"] for f in FILES]
_ids = itertools.count(8_700_000)  # disjoint from the other test files (shared service)
DB = (30, 42)  # two quality targets: streams that stop at different passes per code block


def hook(page):
    rc, msg, want = M.hook_page(page)
    assert rc == 0, msg
    return want


def check_pages(svc, pages, what="", big_endian=False):
    """Every page a layer of ONE registration; every plane byte for byte the CPU hook's (pages of
    reversible streams: the array they were encoded from, which is what the hook gives too)."""
    specs, wants = [], []
    for page in pages:
        sp = specs_of(page, next(_ids), big_endian=big_endian)
        a = page["array"] if page.get("exact") else hook(page)
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
    ids = service.register_tiff_image(os.path.join(M.GOLD, entry["file"]), image)
    try:
        assert sorted(ids) == sorted(int(k) for k in entry["planes"])
        for level, planes in ids.items():
            assert sorted("%d,%d,%d" % p for p in planes) == sorted(entry["planes"][str(level)])
            for (z, c, t), pid in planes.items():
                want, mask = M.expected(entry, level, "%d,%d,%d" % (z, c, t))
                got = np.frombuffer(service.read_plane_be(pid, want.nbytes), want.dtype.newbyteorder(">")).reshape(want.shape)
                M.check_close(got, want, mask, (entry["file"], level, c))
                if entry.get("mixed") and level == 1:  # the reversible level: no window at all
                    assert not mask.any() and np.array_equal(got, want)
    finally:
        for planes in ids.values():
            for pid in planes.values():
                service.release_plane(pid)


@pytest.mark.parametrize("B", [16, 40, 100], ids=["16", "40", "whole"])
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_band_by_band(service, entry, B):
    path = os.path.join(M.GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    S = lay["samples"]
    for (z, c0, t), ifd in zip(lay["planes"], lay["ifds"]):
        for level, d in enumerate([ifd] + ifd["subifds"]):
            for s in range(S):
                want, mask = M.expected(entry, level, "%d,%d,%d" % (z, c0 + s, t))
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
                        got = np.frombuffer(rows_of(service, image, r0, n, w), want.dtype.newbyteorder(">")).reshape(n, w)
                        M.check_close(got, want[r0:r0 + n], mask[r0:r0 + n], (entry["file"], s, r0))
                    assert set(service.band_info(pid)[1]) == {pbx.BS_READY}
                finally:
                    service.release_plane(pid)


# ------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("rps", [8, 16])
@pytest.mark.parametrize("kind", list(KINDS))
def test_strip_sweep(service, kind, rps):
    """Widths 1 .. 34 x heights 1 .. 18, 0 .. 5 levels: signals of one and two samples, odd
    lengths, sub-bands of no samples (where the symmetric extension goes wrong), short last strips,
    code blocks alternating between 4 x 4 and 64 x 64.  One registration per width."""
    mct = KINDS[kind].get("mct", 0)
    for w in range(1, 35):
        pages = []
        for h in range(1, 19):
            cb = (4, 4) if (w + h) & 1 else (64, 64)
            pages.append(M.page_of(kind_array(kind, w, h, 100 * w + h), rows_per_strip=rps, codeblock_size=cb, mct=mct,
                                   num_resolutions=1 + (5 * w + h) % 6, progression=PROGRESSIONS[(w + h) % 5]))
        check_pages(service, pages, "%s w=%d" % (kind, w))


@pytest.mark.parametrize("tile", [16, 64])
@pytest.mark.parametrize("shape", [(40, 30), (100, 70)], ids=["40x30", "100x70"])
def test_clipped_tiles(service, tile, shape):
    w, h = shape
    check_pages(service, [M.page_of(kind_array(k, w, h, tile + w), tile=(tile, tile), mct=KINDS[k].get("mct", 0),
                                    num_resolutions=4) for k in KINDS], "tiles %d" % tile)


def test_one_tile_of_256(service):
    """Five levels, 64 x 64 blocks: equal to the hook, and within 1 + D of PIL.  D is the largest
    |PIL - rint(model)|; the model's pure-Python tier 1 does not run at this size, so D is the
    bound tests/test_tiff_j2k97_host.py holds every stream's to: 3 at 16 bits (OpenJPEG's own
    high-band constant), 1 at 8 bits."""
    pages = [M.page_of(smooth(256, 256, 7), tile=(256, 256), codeblock_size=(64, 64), num_resolutions=6),
             M.page_of(noise(256, 256, 8, samples=3), tile=(256, 256), codeblock_size=(64, 64), num_resolutions=6, mct=1)]
    check_pages(service, pages, "256")
    for page, D in zip(pages, (3, 1)):
        pil = J.pil_decode(page["segments"][0]).astype(np.int64)
        assert np.abs(hook(page).astype(np.int64) - pil).max() <= 1 + D


@pytest.mark.parametrize("db", DB)
def test_truncated_streams(service, db):
    """quality_mode="dB": fewer passes than bit-planes, the lowest coded bit-plane differing from
    coefficient to coefficient: the midpoint is tier 1's to find."""
    o = dict(quality_mode="dB", quality_layers=[db])
    rgb = np.stack([smooth(100, 70, 4 + c, np.uint8) for c in range(3)], axis=-1)
    pages = [M.page_of(smooth(100, 70, 3), tile=(64, 64), num_resolutions=4, **o),
             M.page_of(smooth(40, 30, 5, np.uint8), rows_per_strip=16, num_resolutions=3, **o),
             M.page_of(rgb, tile=(32, 32), mct=1, num_resolutions=4, codeblock_size=(16, 16), **o)]
    hd = M.parse(pages[0]["segments"][0])
    found = J.packets(pages[0]["segments"][0], hd, J.geometry(hd)[0])
    full = [3 * (J.geometry(hd)[0][b]["mb"] - v[3]) - 2 for b, band in enumerate(found[0]) for v in band.values()]
    got = [v[2] for band in found[0] for v in band.values()]
    assert any(g < f for g, f in zip(got, full)), "the stream is not truncated"
    check_pages(service, pages, "dB %d" % db)


@pytest.mark.parametrize("prog", PROGRESSIONS)
def test_progressions(service, prog):
    pages = [M.page_of(noise(40, 30, 11, samples=3), tile=(32, 32), mct=m, progression=prog, num_resolutions=3) for m in (0, 1)]
    pages.append(M.page_of(noise(40, 30, 12, np.uint16), rows_per_strip=16, progression=prog, num_resolutions=4,
                           codeblock_size=(16, 16)))
    check_pages(service, pages, prog)


def test_byte_orders_and_style_1(service):
    a8, a16 = noise(40, 30, 13), noise(40, 30, 14, np.uint16)
    style1 = lambda a, **kw: M.to_style1(M.encode(a, **kw))
    pages = [M.page_of(a8, tile=(16, 16), num_resolutions=1), M.page_of(a16, rows_per_strip=8, num_resolutions=3),
             M.page_of(a16, tile=(32, 32), codeblock_size=(8, 32), num_resolutions=5, progression="CPRL"),
             M.page_of(smooth(40, 30, 16), tile=(32, 32), num_resolutions=4, encoder=style1),
             M.page_of(noise(40, 30, 15, samples=3), tile=(16, 16), mct=1, codeblock_size=(4, 4), num_resolutions=2)]
    assert M.parse(pages[3]["segments"][0])["qstyle"] == 1
    check_pages(service, pages, "little-endian planes")
    check_pages(service, pages, "big-endian planes", big_endian=True)


def test_reversible_and_irreversible_layers_in_one_registration(service):
    """5/3 and 9/7 layers side by side: int32 and float planes in one scratch buffer, both wavelet
    kernels in one launch.  The reversible layers stay exact against their originals."""
    a16, rgb = noise(40, 30, 21, np.uint16), noise(40, 30, 22, samples=3)
    pages = [dict(J.page_of(a16, tile=(16, 16), num_resolutions=3), exact=True),
             M.page_of(a16, tile=(16, 16), num_resolutions=3),
             dict(J.page_of(rgb, rows_per_strip=16, mct=1, num_resolutions=4), exact=True),
             M.page_of(rgb, rows_per_strip=16, mct=1, num_resolutions=4),
             dict(J.page_of(a16, rows_per_strip=8, num_resolutions=2), exact=True)]
    check_pages(service, pages, "mixed")


def test_one_sample_of_three(service):
    a = noise(40, 30, 17, samples=3)
    pg = M.page_of(a, tile=(16, 16), mct=1, num_resolutions=3)
    image = next(_ids)
    (pid,) = service.register_tiff_planes(specs_of(pg, image, samples=[1]))
    try:
        assert service.read_plane_be(pid, 40 * 30) == hook(pg)[:, :, 1].tobytes()
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
    pg = M.page_of(a, tile=tile, rows_per_strip=8, mct=KINDS[kind]["mct"], num_resolutions=3)
    want = hook(pg)
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
            assert got[7 * w:14 * w] == want[7:14, :, target].tobytes()
            for c in range(S):
                if c != target:
                    assert rows_of(service, image, 0, h, w, c=c) == bytes([0x30 + c]) * (h * w)
        finally:
            for pid in pids:
                service.release_plane(pid)


# ------------------------------------------------------------------------------ refusals
def bad_streams():
    """(name, w, h, stream, decoder code): 9/7 streams only the device can refuse."""
    w, h = 40, 24
    good = M.encode(noise(w, h, 31, np.uint16), num_resolutions=3, codeblock_size=(16, 16))
    hd = M.parse(good)
    found = J.packets(good, hd, J.geometry(hd)[0])
    first = min(v[0] for comp in found for band in comp for v in band.values())  # the first code-block byte
    out = [("cut inside a packet header", w, h, good[:hd["data"] + 1], 1)]
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


def test_flipped_bits(service):
    """Garbage code-block bytes decode to garbage coefficients, floats of any size included: the
    write succeeds or is a 400, and the rows and planes around it keep their bytes either way."""
    w, h = 48, 48
    pg = M.page_of(noise(w, h, 41), rows_per_strip=16, num_resolutions=3, codeblock_size=(16, 16))
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
def test_tiff_source_serves_a_png_tile(oracle):
    entry = next(e for e in FILES if e["file"].startswith("gray16_tiles32"))
    path = os.path.join(M.GOLD, entry["file"])
    want, mask = M.expected(entry, 0, "0,0,0")
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({73: path})
        png = pbx.TileRequestHandler(svc, pbx.TileCtx(73, 0, 0, 0, 8, 20, 40, 10, format="png"), src).get_tile()
        r, px, _ = oracle.png_decode(png)
        assert r == 0
        got = np.frombuffer(px, np.dtype(">u2")).reshape(10, 40)
        M.check_close(got, want[20:30, 8:48], mask[20:30, 8:48], "png")
        # rows 20 .. 29 lie in band 1 of 16 rows alone
        states = svc.band_info(svc.lookup_plane(73, 0, 0, 0)[0])[1]
        assert [s == pbx.BS_READY for s in states] == [False, True, False, False], states
