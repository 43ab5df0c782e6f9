"""JPEG 2000 TIFF segments with subsampled chroma and YCbCr components on the GPU
(PBX_TIFF_F_J2K_SUBSAMPLED, PBX_TIFF_F_J2K_YCBCR): tier 2, tier 1 and the inverse wavelets on every
component's own size, and k_tiff_j2k_place_chroma replicating, converting and placing.

The yardstick is the CPU hook (pbx_test_tiff_j2k_decode), which places with the functions the kernel
runs (tiff_j2k_dev.h) and is held to the encoder's inputs, to the float64 model and to
tests/_tiff_jpeg.py's ycc_to_rgb by tests/test_tiff_j2k_chroma_host.py; reversible streams are held
to the inputs here too."""
import itertools
import os

import numpy as np
import pytest

import _tiff_j2k as J
import _tiff_j2k97 as J97
import _tiff_j2k_chroma as C
import _tiff_j2k_packets as K
import pbx
from _tiff_jpeg import ycc_to_rgb
from test_gpu_tiff_j2k import rows_of, specs_of

pytestmark = pytest.mark.gpu

FILES = C.manifest()
_ids = itertools.count(9_100_000)  # disjoint from the other test files (shared service)
SUB, YCC, PK = pbx.TIFF_F_J2K_SUBSAMPLED, pbx.TIFF_F_J2K_YCBCR, pbx.TIFF_F_J2K_PACKETS
SMALL = dict(precinct_size=(16, 16), codeblock_size=(8, 8))


def hook(pg, flags):
    rc, msg, want = K.hook_page(pg, flags)
    assert rc == 0, msg
    return want


def read(svc, pid, shape):
    return np.frombuffer(svc.read_plane_be(pid, shape[0] * shape[1]), np.uint8).reshape(shape)


def check_pages(svc, pages, what="", big_endian=False, samples=None):
    """Every page a layer of ONE registration, once per value of its "flags" list; every plane byte
    for byte the CPU hook's, and for a reversible page the expectation from its inputs."""
    specs, wants = [], []
    for pg in pages:
        for flags in pg["flags"]:
            sp = [dict(s, flags=flags) if flags else s for s in specs_of(pg, next(_ids), samples=samples, big_endian=big_endian)]
            a = hook(pg, flags)
            if "factors" in pg and not pg.get("lossy"):
                assert np.array_equal(a, C.page_planes(pg, bool(flags & YCC))), what
            specs += sp
            wants += [a[:, :, s["sample"]] if a.ndim == 3 else a for s in sp]
    ids = svc.register_tiff_planes(specs)
    try:
        for k, (pid, want) in enumerate(zip(ids, wants)):
            got = np.frombuffer(svc.read_plane_be(pid, want.nbytes), want.dtype.newbyteorder(">")).reshape(want.shape)
            assert np.array_equal(got, want), (what, k, specs[k]["size_x"], specs[k]["size_y"], specs[k]["c"], specs[k].get("flags"),
                                               np.argwhere(got != want)[:4].tolist())
    finally:
        for pid in ids:
            svc.release_plane(pid)


def check_bands(svc, pg, B, flags, sample, what=""):
    """One sample of the page band by band (B rows a band) through pbx_band_write_tiff_j2k."""
    want = hook(pg, flags)[:, :, sample]
    h, w = want.shape
    sp0 = specs_of(pg, 0)[0]
    data, offsets = sp0["segments"]
    gx, seg_h = (-(-w // sp0["seg_w"]) if sp0["tiled"] else 1), sp0["seg_h"]
    rows = min(B, h)
    image = next(_ids)
    pid = svc.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, w, h, rows, big_endian=False)
    try:
        for r0 in range(0, h, rows):
            n = min(rows, h - r0)
            k0, k1 = (r0 // seg_h) * gx, -(-(r0 + n) // seg_h) * gx
            piece = (data[int(offsets[k0]):int(offsets[k1])].copy(), offsets[k0:k1 + 1] - offsets[k0])
            svc.band_write_tiff(pid, r0, n, sp0["seg_w"], seg_h, sp0["tiled"], pbx.TIFF_J2K, 1, piece, samples_per_pixel=3,
                                sample=sample, j2k=True, flags=flags)
            got = np.frombuffer(rows_of(svc, image, r0, n, w), np.uint8).reshape(n, w)
            assert np.array_equal(got, want[r0:r0 + n]), (what, B, r0, sample)
        assert set(svc.band_info(pid)[1]) == {pbx.BS_READY}
    finally:
        svc.release_plane(pid)


# ------------------------------------------------------------------------------ files
def stored(entry):
    """The components as stored without the conversion, and of a lossy file the in-window mask."""
    want = np.load(os.path.join(C.GOLD, entry["file"].replace(".tif", ".npy")))
    if not entry["lossy"]:
        return want, None
    mask = np.unpackbits(np.load(os.path.join(C.GOLD, entry["file"].replace(".tif", "_mask.npy"))))[:want.size]
    return want, mask.reshape(want.shape).astype(bool)


def file_hook(entry, flags):
    path = os.path.join(C.GOLD, entry["file"])
    sp = pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0, j2k_packets=True, j2k_chroma=True)
    rc, msg, out = K.cpu_decode(sp["segments"], entry["width"], entry["length"], sp["seg_w"], sp["seg_h"], sp["tiled"], np.uint8, 3,
                                flags=flags)
    assert rc == 0, msg
    return np.moveaxis(out, 0, 2)


@pytest.mark.parametrize("entry", FILES, ids=[f["file"] for f in FILES])
def test_fixture_registered_whole(service, entry):
    """register_tiff_image takes subsampled files by default and Photometric 6 as YCbCr; Aperio's
    33003 under Photometric 2 with aperio_ycbcr.  Without the keyword: the refusal it always was --
    which is what this file's registration answers on a tree without the feature."""
    path = os.path.join(C.GOLD, entry["file"])
    comps, mask = stored(entry)
    ycc = file_hook(entry, PK | SUB)
    rgb = file_hook(entry, PK | SUB | YCC)
    if entry["lossy"]:
        J97.check_close(ycc, comps, mask, entry["file"])
    else:
        assert np.array_equal(ycc, comps)
    assert np.array_equal(rgb, ycc_to_rgb(ycc[:, :, 0], ycc[:, :, 1], ycc[:, :, 2]))
    for kw, want in ((dict(aperio_ycbcr=True), rgb), ({}, rgb if entry["photometric"] == 6 else ycc)):
        ids = service.register_tiff_image(path, next(_ids), **kw)
        try:
            assert sorted(ids[0]) == [(0, 0, 0), (0, 1, 0), (0, 2, 0)]
            for (z, c, t), pid in ids[0].items():
                assert np.array_equal(read(service, pid, want.shape[:2]), want[:, :, c]), (entry["file"], c, kw)
        finally:
            for pid in ids[0].values():
                service.release_plane(pid)
    xs, ys = entry["factors"]
    image = next(_ids)
    with pytest.raises(pbx.PbxError, match=r"segment 0: subsampled components \(component 1: %d x %d\)|PhotometricInterpretation 6 with "
                       r"SamplesPerPixel 3" % (xs, ys)) as e:
        service.register_tiff_image(path, image, j2k_chroma=False)
    assert e.value.status == 400 and service.lookup_plane(image, 0, 0, 0) is None


@pytest.mark.parametrize("entry", FILES, ids=[f["file"] for f in FILES])
def test_fixture_band_by_band_through_tiff_source(entry):
    """TiffSource on a sparse service: bands of 16, 40 and the whole, every channel, raw tiles."""
    path = os.path.join(C.GOLD, entry["file"])
    want = file_hook(entry, PK | SUB | YCC)
    h, w = want.shape[:2]
    for B in (16, 40, h):
        with pbx.PixelsService(sparse_band_rows=B) as svc:
            src = pbx.TiffSource({75: path}, aperio_ycbcr=True)
            for c in range(3):
                for r0 in range(0, h, B):
                    n = min(B, h - r0)
                    body = pbx.TileRequestHandler(svc, pbx.TileCtx(75, 0, c, 0, 0, r0, w, n), src).get_tile()
                    assert np.array_equal(np.frombuffer(body, np.uint8).reshape(n, w), want[r0:r0 + n, :, c]), (B, c, r0)


def test_tiff_source_serves_a_png_tile(oracle):
    """The R plane of Aperio's 4:2:2 file as a PNG tile, from the one band its rows lie in."""
    entry = next(e for e in FILES if e.get("aperio"))
    path = os.path.join(C.GOLD, entry["file"])
    comps, _ = stored(entry)
    want = ycc_to_rgb(comps[:, :, 0], comps[:, :, 1], comps[:, :, 2])[:, :, 0]
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({76: path}, aperio_ycbcr=True)
        png = pbx.TileRequestHandler(svc, pbx.TileCtx(76, 0, 0, 0, 8, 36, 40, 10, format="png"), src).get_tile()
        r, px, _ = oracle.png_decode(png)
        assert r == 0
        assert np.array_equal(np.frombuffer(px, np.uint8).reshape(10, 40), want[36:46, 8:48])
        states = svc.band_info(svc.lookup_plane(76, 0, 0, 0)[0])[1]
        assert [s == pbx.BS_READY for s in states] == [False, False, True, False, False], states


# ------------------------------------------------------------------------------ generated
def test_strip_sweep(service):
    """Widths 1 .. 20 x heights 1 .. 12 in strips of 8 rows, the factor pairs, levels, progressions
    and block sizes rotating, 5/3 and every fifth 9/7, with and without the conversion; five widths
    a registration.  Components of one sample, one row, one column; odd sizes round up."""
    for w0 in range(1, 21, 5):
        pages = []
        for w in range(w0, w0 + 5):
            for h in range(1, 13):
                xs, ys = C.FACTORS[(w + h) % 3]  # (strips of 8 rows start on even rows)
                a = C.ycc_smooth(w, h, 100 * w + h) if (w + h) % 4 else C.ycc_noise(w, h, 100 * w + h)
                lossy = (w + 2 * h) % 5 == 0
                pg = C.page_of(a, xs, ys, rows_per_strip=8, irreversible=lossy, num_resolutions=1 + (w + 2 * h) % 4,
                               progression=K.PROGRESSIONS[(w + h) % 5], codeblock_size=(4, 4) if w % 2 else (32, 32))
                pages.append(dict(pg, lossy=lossy, flags=[SUB | YCC if (w + h) % 2 else SUB]))
        check_pages(service, pages, "w %d .. %d" % (w0, w0 + 4))


def test_tiles_clipped_by_the_image(service):
    """64 x 64 tiles at 2 x 2 on a 100 x 70 image: the right column's and the bottom row's tiles are
    clipped by the plane, in luma and in chroma; whole, and band by band."""
    pg = dict(C.page_of(C.ycc_smooth(100, 70, 7), 2, 2, tile=(64, 64), num_resolutions=4), flags=[SUB, SUB | YCC])
    check_pages(service, [pg], "64 x 64 tiles")
    for B in (16, 40):
        check_bands(service, pg, B, SUB | YCC, 1, "64 x 64 tiles")


@pytest.mark.parametrize("prog", ["RPCL", "PCRL", "CPRL"])
def test_precincts_layers_and_markers(service, prog):
    """Flags 1 | 4 | 8 on 40 x 24 and 37 x 23: 16 x 16 precincts over 8 x 8 blocks in the three
    position-first progressions, plain, with three layers, and with SOP + EPH."""
    import test_tiff_j2k_chroma_host as T
    pages = []
    for k, (w, h) in enumerate(((40, 24), (37, 23))):
        xs, ys = C.FACTORS[(k + K.PROGRESSIONS.index(prog)) % 3]
        for extra in ({}, dict(layers=(3, T.three)), dict(sop=True, eph=True)):
            pg = C.page_of(C.ycc_smooth(w, h, 11 + w), xs, ys, num_resolutions=3, progression=prog, **dict(SMALL, **extra))
            pages.append(dict(pg, flags=[PK | SUB | YCC]))
    assert K.parse(pages[1]["segments"][0])["layers"] == 3 and K.parse(pages[2]["segments"][0])["scod"] == 7
    check_pages(service, pages, prog)
    check_bands(service, pages[1], 16, PK | SUB | YCC, 2, prog)


def test_mixed_layers_in_one_registration(service):
    """A 1 x 1 RGB layer (k_tiff_j2k_place's), a 4:2:2 5/3 layer and a 4:2:0 9/7 layer
    (k_tiff_j2k_place_chroma's, int32 and float planes) in one registration, and a 1 x 1 YCbCr one."""
    a = C.ycc_smooth(40, 24, 21)
    pages = [dict(J.page_of(a, tile=(16, 16), num_resolutions=3, mct=1), flags=[0]),
             dict(C.page_of(a, 2, 1, tile=(16, 16), num_resolutions=3), flags=[SUB | YCC]),
             dict(C.page_of(a, 2, 2, rows_per_strip=16, irreversible=True, num_resolutions=3), lossy=True, flags=[SUB | YCC, SUB]),
             dict(J.page_of(a, rows_per_strip=8, num_resolutions=2, mct=0), flags=[YCC]),
             dict(J.page_of(K.noise(40, 24, 22), rows_per_strip=8, num_resolutions=2), flags=[0])]
    check_pages(service, pages, "mixed")


def test_irreversible_conversion_is_that_of_the_unconverted_output(service):
    """9/7 with flag 8: exactly ycc_to_rgb of the same stream's flag-4 planes, from the device."""
    pg = C.page_of(C.ycc_smooth(40, 24, 31), 2, 2, tile=(32, 32), irreversible=True, num_resolutions=3)
    out = {}
    for flags in (SUB, SUB | YCC):
        ids = service.register_tiff_planes([dict(s, flags=flags) for s in specs_of(pg, next(_ids))])
        try:
            out[flags] = np.stack([read(service, pid, (24, 40)) for pid in ids], axis=-1)
        finally:
            for pid in ids:
                service.release_plane(pid)
    y = out[SUB]
    assert np.array_equal(out[SUB | YCC], ycc_to_rgb(y[:, :, 0], y[:, :, 1], y[:, :, 2]))
    m = C.page_model(pg)
    for c in range(3):
        assert J97.close(y[:, :, c], m[:, :, c], J97.WINDOW8, 8)[0], c


def test_one_sample_of_three_and_all_three(service):
    pg = dict(C.page_of(C.ycc_smooth(40, 24, 41), 2, 2, tile=(16, 16), num_resolutions=3), flags=[SUB | YCC])
    for samples in ([0], [1], [2], [0, 1, 2]):
        check_pages(service, [pg], "samples %s" % samples, samples=samples)


def test_one_sample_between_sentinels(service):
    """Rows 9 .. 22 of one sample by pbx_band_write_tiff_j2k, cut inside the 32 x 32 tiles: the rows
    around them and the sibling planes stay as they were."""
    S, h, w = 3, 32, 48
    pg = C.page_of(C.ycc_smooth(w, h, 51), 2, 2, tile=(32, 32), num_resolutions=3)
    want = hook(pg, SUB | YCC)
    sp0 = specs_of(pg, 0)[0]
    for target in range(S):
        image = next(_ids)
        pids = [service.create_sparse_plane(image, 0, c, 0, pbx.UINT8, w, h, h, big_endian=False) for c in range(S)]
        try:
            for c in range(S):
                if c != target:
                    service.band_write(pids[c], 0, h, bytes([0x30 + c]) * (h * w))
            service.band_write(pids[target], 0, 9, b"\xA5" * (9 * w))
            service.band_write(pids[target], 23, 9, b"\x5A" * (9 * w))
            service.band_write_tiff(pids[target], 9, 14, 32, 32, True, pbx.TIFF_J2K, 1, sp0["segments"], samples_per_pixel=S,
                                    sample=target, j2k=True, flags=SUB | YCC)
            assert service.band_info(pids[target])[1] == [pbx.BS_READY]
            got = rows_of(service, image, 0, h, w, c=target)
            assert got[:9 * w] == b"\xA5" * (9 * w) and got[23 * w:] == b"\x5A" * (9 * w)
            assert got[9 * w:23 * w] == want[9:23, :, target].tobytes()
            for c in range(S):
                if c != target:
                    assert rows_of(service, image, 0, h, w, c=c) == bytes([0x30 + c]) * (h * w)
        finally:
            for pid in pids:
                service.release_plane(pid)


def test_plane_descriptors_of_both_byte_orders(service):
    """The planes are uint8: a big-endian descriptor stores the same bytes."""
    pg = dict(C.page_of(C.ycc_smooth(37, 23, 61), 2, 1, rows_per_strip=8, num_resolutions=3), flags=[SUB | YCC])
    check_pages(service, [pg], "little-endian")
    check_pages(service, [pg], "big-endian", big_endian=True)


# ------------------------------------------------------------------------------ refusals
def test_a_chroma_component_cut_short(service):
    """The stream ends inside the last component's data: device code 1, nothing registered, the band
    as it was."""
    a = C.ycc_smooth(40, 24, 71)
    s, _ = C.encode(a[:, :, 0], C.sub(a[:, :, 1], 2, 2), C.sub(a[:, :, 2], 2, 2), 2, 2, num_resolutions=3, progression="CPRL")
    image = next(_ids)
    spec = dict(image_id=image, z=0, c=0, t=0, pixel_type=pbx.UINT8, size_x=40, size_y=24, big_endian=False, seg_w=40, seg_h=24,
                tiled=False, compression=pbx.TIFF_J2K, predictor=1, j2k=True, flags=SUB | YCC, samples_per_pixel=3, sample=0,
                segments=pbx.pack_chunks([s[:-30]]))
    rc, msg, _ = K.cpu_decode([s[:-30]], 40, 24, 40, 24, False, np.uint8, 3, flags=SUB | YCC)
    assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code 1)" in msg
    with pytest.raises(pbx.PbxError, match=r"corrupt segment stream 0 \(j2k, decoder code 1\)") as e:
        service.register_tiff_planes([spec])
    assert e.value.status == 400 and service.lookup_plane(image, 0, 0, 0) is None
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, 40, 24, 24, big_endian=False)
    try:
        with pytest.raises(pbx.PbxError, match=r"corrupt segment stream 0 \(j2k, decoder code 1\)"):
            service.band_write_tiff(pid, 0, 24, 40, 24, False, pbx.TIFF_J2K, 1, spec["segments"], samples_per_pixel=3, sample=0,
                                    j2k=True, flags=SUB | YCC)
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT]
    finally:
        service.release_plane(pid)


def test_without_the_flags_nothing_changes(service):
    a = C.ycc_smooth(40, 24, 81)
    s, _ = C.encode(a[:, :, 0], C.sub(a[:, :, 1], 2, 1), C.sub(a[:, :, 2], 2, 1), 2, 1, num_resolutions=3)
    image = next(_ids)
    spec = dict(image_id=image, z=0, c=0, t=0, pixel_type=pbx.UINT8, size_x=40, size_y=24, big_endian=False, seg_w=40, seg_h=24,
                tiled=False, compression=pbx.TIFF_J2K, predictor=1, j2k=True, samples_per_pixel=3, sample=0,
                segments=pbx.pack_chunks([s]))
    for flags in (0, PK, YCC):
        with pytest.raises(pbx.PbxError, match=r"segment 0: subsampled components \(component 1: 2 x 1\)") as e:
            service.register_tiff_planes([dict(spec, flags=flags)])
        assert e.value.status == 400
    with pytest.raises(pbx.PbxError, match="bad flags 0x2"):
        service.register_tiff_planes([dict(spec, flags=2)])
    with pytest.raises(pbx.PbxError, match="bad flags 0x6"):
        service.register_tiff_planes([dict(spec, flags=6)])
    with pytest.raises(pbx.PbxError, match="bad flags 0x4"):  # the flags are the JPEG 2000 calls' alone
        service.register_tiff_planes([dict(spec, j2k=False, compression=8, flags=4)])
    assert service.lookup_plane(image, 0, 0, 0) is None
