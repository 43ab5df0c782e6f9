"""RGB and other multi-sample TIFF / OME-TIFF planes on the GPU: chunky segments split into one
plane per sample by k_tiff_split_place (pbx_planes_register_tiff_samples,
pbx_band_write_tiff_sample), planar ones through the single-sample calls.

Expected bytes: the fixtures' .npy (tests/golden/tiff_rgb), or the numpy array the segments were
made from by tests/_tiff_rgb.py (pinned against libtiff by tests/test_tiff_rgb_host.py).  Every
comparison is byte for byte; sparse planes are read back through full-width raw tiles."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

import _tiff_rgb as R
import _tiff_src as T
import _values as V
import pbx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "tiff_rgb")
with open(os.path.join(GOLD, "manifest.json")) as _f:
    FILES = json.load(_f)["files"]
IDS = [f["file"] for f in FILES]
_ids = itertools.count(7_900_000)  # disjoint from the other test files (shared service)
_NPY = {}


def expected(entry, level, key):
    """The (rows, width) big-endian plane the manifest names: sample s of an image's .npy."""
    npy, s = entry["planes"][str(level)][key]
    if npy not in _NPY:
        _NPY[npy] = np.load(os.path.join(GOLD, npy))
    a = _NPY[npy]
    return np.ascontiguousarray(a[s[0], :, :, s[1]] if isinstance(s, list) else a[:, :, s])


def be_bytes(a):
    return np.ascontiguousarray(a).astype(a.dtype.newbyteorder(">")).tobytes()


def rows_of(svc, image, y0, rows, w, z=0, c=0, t=0, resolution=None):
    st, body = svc.get_tile(pbx.TileCtx(image, z, c, t, 0, y0, w, rows, resolution=resolution))
    assert st == pbx.OK, st
    return body


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
        # one raw tile of the last channel, across a segment boundary
        level = len(ids) - 1
        z, c, t = sorted(ids[level])[-1]
        want = expected(entry, level, "%d,%d,%d" % (z, c, t))
        h, w = want.shape
        x, y, tw, th = w // 3, h // 4, w // 2, h // 2
        st, body = service.get_tile(pbx.TileCtx(image, z, c, t, x, y, tw, th, resolution=0 if len(ids) > 1 else None))
        assert st == pbx.OK and body == want[y:y + th, x:x + tw].tobytes()
    finally:
        for planes in ids.values():
            for pid in planes.values():
                service.release_plane(pid)


@pytest.mark.parametrize("B", [16, 40, 100], ids=["16", "40", "whole"])
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_band_by_band(service, entry, B):
    """Every channel of every level as a sparse plane of its own, loaded band by band: 16 puts
    several bands in one segment row, 40 straddles segment rows, the last is one band."""
    path = os.path.join(GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    S = lay["samples"]
    for (z, c0, t), ifd in zip(lay["planes"], lay["ifds"]):
        for level, d in enumerate([ifd] + ifd["subifds"]):
            for s in range(S):
                want = expected(entry, level, "%d,%d,%d" % (z, c0 + s, t))
                h, w = want.shape
                rows = h if B == 100 else B
                head = pbx.tiff_band_spec(path, d, 0, 0, sample=s)
                image = next(_ids)
                pid = service.create_sparse_plane(image, 0, 0, 0, head["pixel_type"], w, h, rows,
                                                  big_endian=head["big_endian"])
                try:
                    for r0 in range(0, h, rows):
                        n = min(rows, h - r0)
                        sp = pbx.tiff_band_spec(path, d, r0, n, sample=s)
                        service.band_write_tiff(pid, r0, n, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"],
                                                sp["predictor"], sp["segments"],
                                                samples_per_pixel=sp["samples_per_pixel"], sample=sp["sample"])
                        assert rows_of(service, image, r0, n, w) == want[r0:r0 + n].tobytes(), (entry["file"], s, r0)
                    assert set(service.band_info(pid)[1]) == {pbx.BS_READY}
                finally:
                    service.release_plane(pid)


# ---------------------------------------------------------------------- the kernel sweep
TYPES = [("i1", pbx.INT8), ("u1", pbx.UINT8), ("i2", pbx.INT16), ("u2", pbx.UINT16), ("i4", pbx.INT32),
         ("u4", pbx.UINT32), ("f4", pbx.FLOAT)]


def full_range(pt, w, h, S, bo, seed):
    """(h, w, S) samples of uniform random bits (every predictor sum wraps; floats of every
    class), in the file's byte order."""
    a = V.random_bits(pt, w * S, h, seed).reshape(h, w, S)
    return a.astype(a.dtype.newbyteorder(bo)) if a.dtype.itemsize > 1 else a


def layer_specs(a, pt, bo, image, tile, rps, comp, predictor, samples=None):
    """The specs of the samples of one chunky layer (all by default), sharing one segments object."""
    h, w, S = a.shape
    segs = pbx.pack_chunks([R.compress(x, comp) for x in R.chunky_segments(a, tile, rps, predictor)])
    return [dict(image_id=image, z=0, c=s, t=0, pixel_type=pt, size_x=w, size_y=h, big_endian=bo == ">",
                 seg_w=tile[0] if tile else w, seg_h=tile[1] if tile else rps, tiled=tile is not None,
                 compression=comp, predictor=predictor, segments=segs, samples_per_pixel=S, sample=s)
            for s in (range(S) if samples is None else samples)]


def register_and_compare(service, layers):
    """layers: [(array, specs)].  One call registers every plane of every layer."""
    specs = [sp for _, sps in layers for sp in sps]
    ids = service.register_tiff_planes(specs)
    try:
        k = 0
        for a, sps in layers:
            for sp in sps:
                want = be_bytes(a[:, :, sp["sample"]])
                assert service.read_plane_be(ids[k], len(want)) == want, \
                    (a.shape, sp["sample"], sp["seg_w"], sp["seg_h"], sp["compression"], sp["predictor"])
                k += 1
    finally:
        for pid in ids:
            service.release_plane(pid)


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("bo", ["<", ">"], ids=["II", "MM"])
@pytest.mark.parametrize("kind,pt", TYPES, ids=[k for k, _ in TYPES])
def test_split_place_sweep(service, kind, pt, bo, S):
    """Stored segments, so every byte is the kernel's.  A wave step is 1024 / bpp pixels: widths
    at both sides of one and of two steps (the carries), and 1, 5, 17 (a partial first group,
    one lane, two lanes) as strips of 2 rows on 5 rows (a short last strip); 16 x 16 and
    64 x 64 tiles on 65 x 33 and 150 x 100 (padded edges that are never stored).  All layers of
    a layout go through ONE registration: one launch, one destination entry per layer."""
    bpp = int(kind[1])
    step = 1024 // bpp
    preds = (1,) if kind == "f4" else (1, 2)
    seed = itertools.count(100 * S + 10 * [k for k, _ in TYPES].index(kind) + (bo == ">"))
    strips, tiles = [], []
    for predictor in preds:
        for w in (1, 5, 17, step - 1, step, step + 1, 2 * step + 1):
            a = full_range(pt, w, 5, S, bo, next(seed))
            strips.append((a, layer_specs(a, pt, bo, next(_ids), None, 2, pbx.TIFF_NONE, predictor)))
        for tile, (w, h) in (((16, 16), (65, 33)), ((64, 64), (150, 100))):
            a = full_range(pt, w, h, S, bo, next(seed))
            tiles.append((a, layer_specs(a, pt, bo, next(_ids), tile, None, pbx.TIFF_NONE, predictor)))
    register_and_compare(service, strips)
    register_and_compare(service, tiles)


@pytest.mark.parametrize("comp", [pbx.TIFF_LZW, pbx.TIFF_DEFLATE], ids=["lzw", "deflate"])
def test_split_place_from_decoded_segments(service, comp):
    """A few shapes of the sweep again, compressed: the kernel reads the decoders' scratch."""
    layers = []
    for n, (kind, pt, bo, S, tile, (w, h)) in enumerate([
            ("u1", pbx.UINT8, "<", 3, None, (1025, 5)), ("u2", pbx.UINT16, ">", 4, (16, 16), (65, 33)),
            ("i4", pbx.INT32, "<", 2, (64, 64), (150, 100)), ("u2", pbx.UINT16, "<", 3, None, (513, 5))]):
        a = full_range(pt, w, h, S, bo, 900 + n)
        layers.append((a, layer_specs(a, pt, bo, next(_ids), tile, 2, comp, 2)))
    register_and_compare(service, layers)


def test_some_samples_of_a_layer_and_mixed_single_sample_planes(service):
    """A registration that names only samples 2 and 0 of an RGB layer (in that order), next to
    an ordinary single-sample plane: the old and the new planner in one launch."""
    a = full_range(pbx.UINT16, 70, 20, 3, "<", 5)
    g = full_range(pbx.UINT8, 33, 9, 1, "<", 6)
    grey = layer_specs(g, pbx.UINT8, "<", next(_ids), None, 4, pbx.TIFF_LZW, 2)
    grey[0].update(samples_per_pixel=1)
    grey[0]["segments"] = pbx.pack_chunks([R.compress(x, pbx.TIFF_LZW) for x in
                                           T.segments_of(g[:, :, 0], None, 4, 2)])
    register_and_compare(service, [(a, layer_specs(a, pbx.UINT16, "<", next(_ids), (16, 16), None,
                                                   pbx.TIFF_DEFLATE, 2, samples=(2, 0))), (g, grey)])


# ------------------------------------------------------------------------ band writes
BAND = 7


@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("comp", [pbx.TIFF_NONE, pbx.TIFF_LZW, pbx.TIFF_DEFLATE], ids=["stored", "lzw", "deflate"])
@pytest.mark.parametrize("tile", [None, (16, 16)], ids=["strips", "tiles"])
def test_one_sample_band_write(service, tile, comp, predictor):
    """A one-band plane per sample, 21 rows: rows 0..6 and 14..20 are sentinel bytes from
    band_write, and rows 7..13 come from two band_write_tiff pieces, [7, 10) and [10, 14), that
    begin and end inside a segment (strips of 4 rows, tiles of 16).  The sentinel rows and the
    sibling planes (all sentinel) must stay as they were, and the rows written must be those of
    a registration of the same segments."""
    S, h, w = 3, 21, 65
    a = full_range(pbx.UINT16, w, h, S, ">", 40 + predictor)
    specs = layer_specs(a, pbx.UINT16, ">", next(_ids), tile, 4, comp, predictor)
    (data, offsets), gx, seg_h = specs[0]["segments"], (-(-w // 16) if tile else 1), specs[0]["seg_h"]
    row = w * 2
    reg = service.register_tiff_planes(specs)
    try:
        for target in range(S):
            image = next(_ids)
            pids = [service.create_sparse_plane(image, 0, c, 0, pbx.UINT16, w, h, h, big_endian=True)
                    for c in range(S)]
            try:
                for c in range(S):
                    if c != target:
                        service.band_write(pids[c], 0, h, bytes([0x30 + c]) * (h * row))
                service.band_write(pids[target], 0, 7, b"\xA5" * (7 * row))
                service.band_write(pids[target], 14, 7, b"\x5A" * (7 * row))
                for y0, rows in ((7, 3), (10, 4)):
                    k0, k1 = (y0 // seg_h) * gx, -(-(y0 + rows) // seg_h) * gx
                    piece = (data[int(offsets[k0]):int(offsets[k1])].copy(), offsets[k0:k1 + 1] - offsets[k0])
                    service.band_write_tiff(pids[target], y0, rows, specs[0]["seg_w"], seg_h, tile is not None,
                                            comp, predictor, piece, samples_per_pixel=S, sample=target)
                assert service.band_info(pids[target])[1] == [pbx.BS_READY]
                got = rows_of(service, image, 0, h, w, c=target)
                assert got[:7 * row] == b"\xA5" * (7 * row) and got[14 * row:] == b"\x5A" * (7 * row)
                assert got[7 * row:14 * row] == be_bytes(a[7:14, :, target])
                assert got[7 * row:14 * row] == service.read_plane_be(reg[target], h * row)[7 * row:14 * row]
                for c in range(S):
                    if c != target:
                        assert rows_of(service, image, 0, h, w, c=c) == bytes([0x30 + c]) * (h * row)
            finally:
                for pid in pids:
                    service.release_plane(pid)
    finally:
        for pid in reg:
            service.release_plane(pid)


# --------------------------------------------------------------------- behind the handler
def test_tiff_source_serves_every_channel_of_an_rgb_pyramid():
    entry = next(e for e in FILES if e["file"].startswith("pyramid"))
    path = os.path.join(GOLD, entry["file"])
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({61: path})
        for c in range(3):
            body = pbx.TileRequestHandler(svc, pbx.TileCtx(61, 0, c, 0, 5, 30, 140, 20), src).get_tile()
            assert body == expected(entry, 0, "0,%d,0" % c)[30:50, 5:145].tobytes(), c
        # stored level 1 is resolution 1 of 3 (resolution 0 is the smallest)
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(61, 0, 2, 0, 3, 10, 60, 25, resolution=1), src).get_tile()
        assert body == expected(entry, 1, "0,2,0")[10:35, 3:63].tobytes()


def test_tiff_source_serves_the_second_z_of_an_rgb_ome_tiff():
    entry = next(e for e in FILES if "ome" in e)
    path = os.path.join(GOLD, entry["file"])
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({62: path})
        for c in (1, 2):
            body = pbx.TileRequestHandler(svc, pbx.TileCtx(62, 1, c, 0, 4, 20, 60, 10), src).get_tile()
            assert body == expected(entry, 0, "1,%d,0" % c)[20:30, 4:64].tobytes()
    with pbx.PixelsService() as svc:  # whole planes: only the requested channel is registered
        src = pbx.TiffSource({62: path})
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(62, 1, 2, 0, 4, 20, 60, 10), src).get_tile()
        assert body == expected(entry, 0, "1,2,0")[20:30, 4:64].tobytes()
        assert svc.lookup_plane(62, 1, 2, 0) is not None and svc.lookup_plane(62, 1, 0, 0) is None


# --------------------------------------------------------------------------------- errors
def test_refused_arguments(service):
    a = full_range(pbx.UINT8, 40, 10, 3, "<", 1)

    def specs(**kw):
        sps = layer_specs(a, pbx.UINT8, "<", next(_ids), None, 4, pbx.TIFF_NONE, 1)
        for sp in sps:
            sp.update(kw)
        return sps

    def refused(sps, msg):
        with pytest.raises(pbx.PbxError, match=msg) as e:
            service.register_tiff_planes(sps)
        assert e.value.status == 400

    refused(specs(samples_per_pixel=5), "samples_per_pixel 5 outside 1 .. 4")
    sps = specs()
    sps[2]["sample"] = 3
    refused(sps, "sample 3 outside segments of 3 samples per pixel")
    sps = specs()
    sps[2]["sample"] = 1
    refused(sps, "both name sample 1 of layer 0")
    sps = specs()
    sps[1]["size_y"] = 9
    refused(sps, "planes of layer 0 disagree on size, type or byte order")
    sps = specs()
    sps[1]["big_endian"] = True
    sps[1]["pixel_type"] = sps[0]["pixel_type"] = sps[2]["pixel_type"] = pbx.UINT16
    refused(sps, "disagree on size, type or byte order")
    refused(specs(pixel_type=pbx.DOUBLE), "samples_per_pixel 3 on 64-bit samples")
    refused(specs(samples_per_pixel=2)[:2], "uncompressed segment 0: 480 bytes, not 320")
    # a layer no plane names: the C call alone (the Python layer builds layers from planes)
    sp = specs()[0]
    d = (pbx.PbxPlaneDesc * 2)()
    image = next(_ids)
    for c in range(2):
        d[c].image_id, d[c].c, d[c].pixel_type, d[c].size_x, d[c].size_y = image, c, pbx.UINT8, 40, 10
    rf = (pbx.PbxZarrSlice * 2)()
    rf[1].slice = 1
    sg = (pbx.PbxTiffSegments * 2)()
    for s in sg:
        s.seg_w, s.seg_h, s.compression, s.predictor = 40, 4, 1, 1
        s.data, s.offsets = sp["segments"][0].ctypes.data, sp["segments"][1].ctypes.data
    spp = (ctypes.c_int32 * 2)(3, 3)
    ids = (ctypes.c_uint64 * 2)()
    assert pbx.lib().pbx_planes_register_tiff_samples(service.handle, 2, d, rf, 2, sg, spp, ids, None) == 400
    assert b"layer 1: no plane names it" in pbx.lib().pbx_last_error()
    # band writes
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, 40, 10, 10, big_endian=False)
    try:
        for kw, msg in ((dict(samples_per_pixel=5, sample=0), "samples_per_pixel 5 outside"),
                        (dict(samples_per_pixel=3, sample=3), "sample 3 outside"),
                        (dict(samples_per_pixel=1, sample=1), "sample 1 outside"),
                        (dict(samples_per_pixel=4, sample=0), "uncompressed segment 0")):
            with pytest.raises(pbx.PbxError, match=msg) as e:
                service.band_write_tiff(pid, 0, 10, 40, 4, False, 1, 1, sp["segments"], **kw)
            assert e.value.status == 400
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT]
        service.band_write_tiff(pid, 0, 10, 40, 4, False, 1, 1, sp["segments"], samples_per_pixel=3, sample=1)
        assert rows_of(service, image, 0, 10, 40) == a[:, :, 1].tobytes()
    finally:
        service.release_plane(pid)


def test_corrupt_stream_registers_none_of_the_layers_planes(service):
    a = full_range(pbx.UINT8, 150, 40, 3, "<", 2)
    image = next(_ids)
    good = layer_specs(a, pbx.UINT8, "<", image, None, 8, pbx.TIFF_LZW, 2)
    segs = [R.compress(x, pbx.TIFF_LZW) for x in R.chunky_segments(a, None, 8, 2)]
    # a code far above the next free one, right after the Clear: 0x80 0x7F 0xF0 = Clear, 4095 >> 3 ...
    segs[2] = b"\x80\x7f\xff" + segs[2][3:]
    bad_segs = pbx.pack_chunks(segs)
    bad = [dict(sp, segments=bad_segs) for sp in good]
    with pytest.raises(pbx.PbxError, match="corrupt chunk stream") as e:
        service.register_tiff_planes(bad)
    assert e.value.status == 400
    assert all(service.lookup_plane(image, 0, c, 0) is None for c in range(3))
    ids = service.register_tiff_planes(good)  # the keys are free, and the good layer loads
    try:
        for c, pid in enumerate(ids):
            assert service.read_plane_be(pid, 150 * 40) == a[:, :, c].tobytes()
    finally:
        for pid in ids:
            service.release_plane(pid)
