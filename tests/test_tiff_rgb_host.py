"""RGB and other multi-sample TIFF / OME-TIFF files, host side (no GPU): the helper of the tests
(tests/_tiff_rgb.py) pinned against libtiff, the container reader, the layout and the specs on
every fixture (each spec's segments are decoded with numpy / zlib / the helper's LZW decoder and
compared with the fixture's .npy, so the plane <-> (IFD, sample) mapping is checked without a
device), the host planner (pbx_test_tiff_plan_samples) and every refusal of the Python layer and
of the planner.

Fixtures: tests/golden/tiff_rgb/ (make_tiff_rgb_golden.py: tifffile, libtiff's tiffcp, PIL)."""
import ctypes
import itertools
import json
import os
import re
import zlib

import numpy as np
import pytest

import _tiff_rgb as R
import _tiff_src as T
import pbx

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "tiff_rgb")
with open(os.path.join(GOLD, "manifest.json")) as _f:
    FILES = json.load(_f)["files"]
IDS = [f["file"] for f in FILES]
_NPY = {}


def expected(entry, level, key):
    """The (rows, width) big-endian plane the manifest names: sample s of an image's .npy."""
    npy, s = entry["planes"][str(level)][key]
    if npy not in _NPY:
        _NPY[npy] = np.load(os.path.join(GOLD, npy))
    a = _NPY[npy]
    return a[s[0], :, :, s[1]] if isinstance(s, list) else a[:, :, s]


def test_exports():
    L = pbx.lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "pbx.h")).read()
    for name in ("pbx_planes_register_tiff_samples", "pbx_band_write_tiff_sample", "pbx_test_tiff_plan_samples"):
        assert name in pbx.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert ctypes.sizeof(pbx.PbxTiffSegments) == 40 and L.pbx_abi_version() == 9


# --------------------------------------------------------------------------- the helper
def colour(rows, width, s, dtype=np.uint8, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.poisson(6, (rows, width, s)) * 37 + np.arange(s) * 5).astype(dtype)


@pytest.mark.parametrize("s", [3, 4])
def test_helper_files_decode_under_libtiff(tmp_path, s):
    Image = pytest.importorskip("PIL.Image")
    a = colour(100, 150, s, seed=s)
    for n, (geo, comp, pred, planar) in enumerate(itertools.product(
            (dict(rows_per_strip=32), dict(tile=(64, 64))), (1, 5, 8), (1, 2), (1, 2))):
        if s == 4 and planar == 2:
            continue  # (PIL has no reader for planar RGBA)
        if comp == 1 and pred == 2:
            continue  # (libtiff's predictor is part of its LZW and deflate codecs: stored data is not summed)
        p = str(tmp_path / ("h%d.tif" % n))
        R.write_tiff(p, [R.page_of(a, comp, pred, planar=planar, extrasamples=[2] if s == 4 else None, **geo)])
        got = np.array(Image.open(p))
        assert got.shape == a.shape and (got == a).all(), (geo, comp, pred, planar)


def test_helper_predictor_is_per_component():
    a = colour(3, 5, 3, np.uint16, 1)
    d = R.predict2s(a)
    assert (d[:, 0] == a[:, 0]).all()
    assert (np.cumsum(d.astype(np.uint32), axis=1).astype(np.uint16) == a).all()
    for s in range(3):  # = the single-sample predictor of every component
        assert (d[:, :, s] == T.predict2(a[:, :, s])).all()
    be = R.predict2s(a.astype(">u2"))
    assert be.dtype == np.dtype(">u2") and (be == d).all()


# ------------------------------------------------------------- container, layout, specs
def decode_spec(sp):
    """The (size_y, size_x) plane a spec describes, from its segments, without the library."""
    data, offsets = sp["segments"]
    bo = ">" if sp["big_endian"] else "<"
    dt = np.dtype({pbx.UINT8: "u1", pbx.INT8: "i1", pbx.UINT16: "u2", pbx.INT16: "i2", pbx.UINT32: "u4",
                   pbx.INT32: "i4", pbx.FLOAT: "f4"}[sp["pixel_type"]]).newbyteorder(bo)
    S, w, h = sp["samples_per_pixel"], sp["size_x"], sp["size_y"]
    gx = -(-w // sp["seg_w"]) if sp["tiled"] else 1
    out = np.zeros((h, w), dt)
    for k in range(len(offsets) - 1):
        raw = bytes(data[int(offsets[k]):int(offsets[k + 1])])
        y0, x0 = (k // gx) * sp["seg_h"], (k % gx) * sp["seg_w"]
        rows = sp["seg_h"] if sp["tiled"] else min(sp["seg_h"], h - y0)
        n = rows * sp["seg_w"] * S * dt.itemsize
        if sp["compression"] == pbx.TIFF_DEFLATE:
            raw = zlib.decompress(raw)
        elif sp["compression"] == pbx.TIFF_LZW:
            raw = T.lzw_decode(raw, n)
        assert len(raw) == n
        seg = np.frombuffer(raw, dt).reshape(rows, sp["seg_w"], S)
        if sp["predictor"] == 2:
            u = seg.astype(dt.newbyteorder("=")).view("u%d" % dt.itemsize)
            seg = np.cumsum(u, axis=1, dtype=u.dtype).view(dt.newbyteorder("=")).astype(dt)
        piece = seg[:, :, sp["sample"]][:h - y0, :w - x0]
        out[y0:y0 + piece.shape[0], x0:x0 + piece.shape[1]] = piece
    return out


@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_layout_and_specs(entry):
    path = os.path.join(GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    S = entry["samples"]
    ome = entry.get("ome", dict(size_z=1, size_c=S, size_t=1))
    assert (lay["size_z"], lay["size_c"], lay["size_t"], lay["samples"]) == \
        (ome["size_z"], ome["size_c"], ome["size_t"], S)
    assert lay["levels"] == len(entry["planes"])
    assert all(c % S == 0 for _, c, _ in lay["planes"]) and len(lay["planes"]) == len(lay["ifds"])
    for ifd in lay["ifds"]:
        assert ifd["spp"] == ifd["bits_count"] == S and ifd["sampleformat_count"] in (1, S)
        assert ifd["planar"] == entry["planar"] and ifd["photometric"] == 2
        assert ifd["extrasamples"] == ([2] if S == 4 else [])
    src = pbx.TiffSource({5: path})
    px = src.get_pixels(5)
    assert (px.size_z, px.size_c, px.size_t, px.levels) == (ome["size_z"], ome["size_c"], ome["size_t"], lay["levels"])
    seen = set()
    for level in range(lay["levels"]):
        for key in entry["planes"][str(level)]:
            z, c, t = (int(v) for v in key.split(","))
            want = expected(entry, level, key)
            sp = src.plane_segments(px, z, c, t, level)
            assert (sp["z"], sp["c"], sp["t"], sp["level"]) == (z, c, t, level)
            if entry["planar"] == 2:
                assert (sp["samples_per_pixel"], sp["sample"]) == (1, 0)
            else:
                assert (sp["samples_per_pixel"], sp["sample"]) == (S, c % S)
            got = decode_spec(sp)
            assert got.astype(got.dtype.newbyteorder(">")).tobytes() == want.tobytes(), (level, key)
            seen.add((level, z, c, t))
    assert len(seen) == lay["levels"] * ome["size_z"] * ome["size_c"] * ome["size_t"]


@pytest.mark.parametrize("entry", [f for f in FILES if "pil" not in f["file"]],
                         ids=[f for f in IDS if "pil" not in f])
def test_band_spec_reads_only_the_covering_segments_of_its_sample(entry):
    path = os.path.join(GOLD, entry["file"])
    ifd = pbx.tiff_ifds(path)[0]
    S, sample = entry["samples"], entry["samples"] - 1
    gx = -(-ifd["width"] // ifd["seg_w"]) if ifd["tiled"] else 1
    gy = -(-ifd["length"] // ifd["seg_h"])
    y0 = ifd["seg_h"] - 3  # from the first segment row into the second, or (strips) the third
    rows = min(ifd["seg_h"] + 5, ifd["length"] - y0)
    sp = pbx.tiff_band_spec(path, ifd, y0, rows, sample=sample)
    base = sample * gx * gy if entry["planar"] == 2 else 0
    ks = range(base, base + -(-(y0 + rows) // ifd["seg_h"]) * gx)
    data, offsets = sp["segments"]
    assert list(np.diff(offsets.astype(np.int64))) == [ifd["counts"][k] for k in ks]
    blob = open(path, "rb").read()
    assert bytes(data[:int(offsets[-1])]) == b"".join(blob[ifd["offsets"][k]:ifd["offsets"][k] + ifd["counts"][k]]
                                                      for k in ks)
    assert (sp["samples_per_pixel"], sp["sample"]) == ((1, 0) if entry["planar"] == 2 else (S, sample))
    assert (sp["y0"], sp["rows"]) == (y0, rows)
    empty = pbx.tiff_band_spec(path, ifd, 0, 0, sample=sample)
    assert empty["segments"] is None and empty["samples_per_pixel"] == sp["samples_per_pixel"]
    with pytest.raises(pbx.PbxError, match="sample %d outside SamplesPerPixel %d" % (S, S)):
        pbx.tiff_band_spec(path, ifd, 0, 1, sample=S)


def test_register_tiff_image_shares_one_segments_object_per_chunky_ifd(monkeypatch):
    got = []
    svc = pbx.PixelsService.__new__(pbx.PixelsService)
    monkeypatch.setattr(pbx.PixelsService, "register_tiff_planes", lambda self, specs: got.append(specs) or
                        list(range(len(specs))))
    monkeypatch.setattr(pbx.PixelsService, "__del__", lambda self: None)
    ids = svc.register_tiff_image(os.path.join(GOLD, "pyramid_rgb8_deflate.tif"), 9)
    specs = got[0]
    assert sorted(ids) == [0, 1, 2] and all(sorted(v) == [(0, 0, 0), (0, 1, 0), (0, 2, 0)] for v in ids.values())
    assert len(specs) == 9 and len({id(s["segments"]) for s in specs}) == 3
    assert [(s["level"], s["c"], s["sample"]) for s in specs] == [(l, c, c) for l in range(3) for c in range(3)]
    got.clear()
    svc.register_tiff_image(os.path.join(GOLD, "rgb8_planar_tiles_deflate_p2_II.tif"), 9)
    assert [(s["c"], s["sample"], s["samples_per_pixel"]) for s in got[0]] == [(0, 0, 1), (1, 0, 1), (2, 0, 1)]
    assert len({id(s["segments"]) for s in got[0]}) == 3


# ------------------------------------------------------------------------- the planner
def plan(segs, size_x, size_y, bpp, spp, seg_w, seg_h, tiled, compression, predictor=1, y0=0, rows=0, flags=0):
    data, offsets = pbx.pack_chunks(segs)
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor, s.flags = seg_w, seg_h, tiled, compression, predictor, flags
    s.data, s.offsets = data.ctypes.data, offsets.ctypes.data
    out = (ctypes.c_uint64 * 4)()
    rc = pbx.lib().pbx_test_tiff_plan_samples(ctypes.byref(s), size_x, size_y, bpp, spp, y0, rows, out)
    return rc, list(out), pbx.lib().pbx_last_error().decode()


def r256(n):
    return (n + 255) & ~255


@pytest.mark.parametrize("spp", [1, 2, 3, 4])
@pytest.mark.parametrize("bpp", [1, 2, 4])
def test_planner_counts_strips_and_tiles(spp, bpp):
    # strips of 32 rows on 150 x 100: 32, 32, 32, 4 rows; compressed, so one stream a strip
    rc, out, err = plan([b"\x80\0\1\2"] * 4, 150, 100, bpp, spp, 150, 32, 0, 5, 2)
    assert rc == 0, err
    one = 150 * 100 * bpp
    assert out[:2] == [4, spp * one]
    assert out[2] == 3 * r256(150 * 32 * bpp * spp) + r256(150 * 4 * bpp * spp)
    assert out[3] == (4 if spp > 1 else 1)
    # tiles of 64 x 64: 3 x 2 full tiles, deflate, predictor 1
    rc, out, err = plan([b"\x78\x9c\0\0"] * 6, 150, 100, bpp, spp, 64, 64, 1, 8, 1)
    assert rc == 0, err
    assert out == [6, 6 * 64 * 64 * bpp * spp, 6 * r256(64 * 64 * bpp * spp), 6 if spp > 1 else 0]
    # a band: rows 40 .. 69 lie in tile rows 0 and 1, rows 70 .. 99 in tile row 1 alone
    rc, out, err = plan([b"\x78\x9c\0\0"] * 3, 150, 100, bpp, spp, 64, 64, 1, 8, 2, y0=70, rows=30)
    assert rc == 0, err
    assert out == [3, 3 * 64 * 64 * bpp * spp, 3 * r256(64 * 64 * bpp * spp), 3 if spp > 1 else 1]


@pytest.mark.parametrize("spp", [2, 3, 4])
def test_planner_reads_stored_multi_sample_segments_in_place(spp):
    segs = [bytes(150 * r * 2 * spp) for r in (32, 32, 32, 4)]
    for pred in (1, 2):
        rc, out, err = plan(segs, 150, 100, 2, spp, 150, 32, 0, 1, pred)
        assert rc == 0, err
        assert out == [0, 150 * 100 * 2 * spp, 0, 4]  # no stream, no scratch, every segment split
        rc, out, err = plan(segs[1:3], 150, 100, 2, spp, 150, 32, 0, 1, pred, y0=33, rows=40)
        assert rc == 0 and out == [0, 150 * 64 * 2 * spp, 0, 2], err
    # a single-sample registration still copies stored segments into scratch
    rc, out, _ = plan([bytes(150 * r * 2) for r in (32, 32, 32, 4)], 150, 100, 2, 1, 150, 32, 0, 1)
    assert rc == 0 and out[0] == 4 and out[2] > 0


def test_planner_spp1_is_the_old_planner():
    segs = [b"\x80\0\1\2"] * 4
    a = dict(size_x=150, size_y=100, bpp=2)
    for pred in (1, 2):
        rc, out, _ = plan(segs, spp=1, seg_w=150, seg_h=32, tiled=0, compression=5, predictor=pred, **a)
        data, offsets = pbx.pack_chunks(segs)
        s = pbx.PbxTiffSegments()
        s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor = 150, 32, 0, 5, pred
        s.data, s.offsets = data.ctypes.data, offsets.ctypes.data
        old = (ctypes.c_uint64 * 4)()
        assert pbx.lib().pbx_test_tiff_plan(ctypes.byref(s), 150, 100, 2, old) == 0
        assert rc == 0 and out == list(old)


PLAN_REFUSALS = [
    ("spp 0", dict(spp=0), "samples_per_pixel 0 outside 1 .. 4"),
    ("spp 5", dict(spp=5), "samples_per_pixel 5 outside 1 .. 4"),
    ("double", dict(bpp=8, compression=5, segs=[b"\x80\0\1\2"] * 4), "samples_per_pixel 3 on 64-bit samples"),
    ("stored length", dict(segs=[bytes(150 * 32 * 2)] * 4), "uncompressed segment 0: 9600 bytes, not 28800"),
    ("short last strip", dict(segs=[bytes(28800)] * 4), "uncompressed segment 3: 28800 bytes, not 3600"),
    ("empty", dict(compression=5, segs=[b"\x80\0", b"", b"\x80\0", b"\x80\0"]), "segment 1 is empty"),
    ("strip width", dict(seg_w=100), "strip width 100 != plane width 150"),
    ("tile shape", dict(tiled=1, seg_w=60, seg_h=64), "multiples of 16"),
    ("compression", dict(compression=7), "bad compression 7"),
    ("predictor", dict(predictor=3), "bad predictor 3"),
    ("flags", dict(flags=1), "bad flags 0x1"),
    ("old-style LZW", dict(compression=5, segs=[b"\0\1\2\3"] * 4), "old-style"),
    ("too large", dict(size_x=1 << 20, seg_w=1 << 20, seg_h=400, size_y=400, bpp=4, compression=5,
                       segs=[b"\x80\0\1\2"]), "segment 0 too large"),
    ("rows outside", dict(y0=90, rows=20), "outside the plane"),
]


@pytest.mark.parametrize("name,change,msg", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_planner_refusals(name, change, msg):
    a = dict(segs=[bytes(150 * r * 2 * 3) for r in (32, 32, 32, 4)], size_x=150, size_y=100, bpp=2, spp=3,
             seg_w=150, seg_h=32, tiled=0, compression=1)
    a.update(change)
    rc, _, err = plan(**a)
    assert rc == 400 and msg in err, (rc, err)


def test_planner_too_large_counts_the_samples():
    # 1.5 GiB a strip for one sample, past 2^31 - 1 with two
    a = dict(segs=[b"\x80\0\1\2"], size_x=1 << 19, size_y=768, bpp=4, seg_w=1 << 19, seg_h=768, tiled=0, compression=5)
    assert plan(spp=1, **a)[0] == 0
    rc, _, err = plan(spp=2, **a)
    assert rc == 400 and "too large" in err


# ------------------------------------------------------------------ the Python layer
def rgb_page(**kw):
    return R.page_of(colour(30, 40, 3), 8, 2, rows_per_strip=16, **kw)


def write(tmp_path, page, name="r.tif", **kw):
    p = str(tmp_path / name)
    R.write_tiff(p, [page], **kw)
    return p


def test_helper_written_file_layout(tmp_path):
    for bo, big in (("<", False), (">", False), ("<", True)):
        a = colour(30, 40, 4).astype(bo + "u1")
        p = write(tmp_path, R.page_of(a, 5, 2, tile=(16, 16), extrasamples=[1]), byteorder=bo, bigtiff=big)
        lay = pbx.tiff_image_layout(p)
        ifd = lay["ifds"][0]
        assert (lay["size_c"], lay["samples"], ifd["bits_count"], ifd["extrasamples"]) == (4, 4, 4, [1])
        for c in range(4):
            sp = pbx.tiff_plane_spec(p, ifd, 1, 0, c, 0, sample=c)
            assert (decode_spec(sp) == a[:, :, c]).all()


PY_REFUSALS = [
    ("spp 5", lambda pg: pg.update(spp=5, extra=[(258, 3, [8] * 5)]), "SamplesPerPixel 5 (1 to 4 are supported)"),
    ("bits count", lambda pg: pg.update(extra=[(258, 3, [8, 8])]), "SamplesPerPixel 3 with 2 BitsPerSample value(s)"),
    ("bits differ", lambda pg: pg.update(extra=[(258, 3, [8, 8, 16])]), "samples differ in bits"),
    ("ycbcr", lambda pg: pg.update(photometric=6), "PhotometricInterpretation 6 with SamplesPerPixel 3"),
    ("cmyk", lambda pg: pg.update(photometric=5), "PhotometricInterpretation 5 with SamplesPerPixel 3"),
    ("palette", lambda pg: pg.update(photometric=3), "PhotometricInterpretation 3 with SamplesPerPixel 3"),
    ("planar 3", lambda pg: pg.update(planar=3), "PlanarConfiguration 3"),
    ("64-bit", lambda pg: pg.update(bits=64, sampleformat=3, predictor=1), "SamplesPerPixel 3 with 64-bit samples"),
    ("planar count", lambda pg: pg.update(planar=2), "2 segments for 3 planar samples on a grid of 1 x 2"),
]


@pytest.mark.parametrize("name,change,msg", PY_REFUSALS, ids=[r[0] for r in PY_REFUSALS])
def test_python_refusals(tmp_path, name, change, msg):
    page = rgb_page()
    change(page)
    p = write(tmp_path, page)
    with pytest.raises(pbx.PbxError, match=re.escape(msg)) as e:
        pbx.tiff_plane_spec(p, pbx.tiff_ifds(p)[0], 1, 0, 0, 0)
    assert e.value.status == 400
    if name != "planar count":  # (the layout reads no segment table)
        with pytest.raises(pbx.PbxError, match=re.escape(msg)) as e:
            pbx.tiff_image_layout(p)
        assert e.value.status == 400


def test_single_value_bitspersample_is_the_count_rule(tmp_path):
    # what tests/test_tiff_src_host.py::test_python_refusals[spp] writes: spp = 3, one BitsPerSample value
    a = np.zeros((30, 40), np.uint8)
    p = str(tmp_path / "s.tif")
    T.write_tiff(p, [dict(T.page_of(a, rows_per_strip=16), spp=3)])
    with pytest.raises(pbx.PbxError, match=re.escape("SamplesPerPixel 3 with 1 BitsPerSample value(s)")):
        pbx.tiff_image_layout(p)


def test_pages_must_agree_on_samples(tmp_path):
    p = str(tmp_path / "m.tif")
    R.write_tiff(p, [rgb_page(), R.page_of(colour(30, 40, 4), 8, 2, rows_per_strip=16)])
    with pytest.raises(pbx.PbxError, match="IFD 1 has SamplesPerPixel 4, the first has 3"):
        pbx.tiff_image_layout(p)
    R.write_tiff(p, [rgb_page(), rgb_page()])
    lay = pbx.tiff_image_layout(p)  # plain TIFF: page k is t = k, the samples are the channels
    assert (lay["size_z"], lay["size_c"], lay["size_t"], lay["planes"]) == (1, 3, 2, [(0, 0, 0), (0, 0, 1)])


OME = '<?xml version="1.0"?><OME xmlns="http://www.openmicroscopy.org/Schemas/OME/2016-06">%s</OME>'
IMG = ('<Image ID="Image:0"><Pixels ID="Pixels:0" DimensionOrder="%s" Type="uint8" SizeX="40" SizeY="30" '
       'SizeZ="2" SizeC="%d" SizeT="1">%s</Pixels></Image>')
CH = '<Channel ID="Channel:0:%d" SamplesPerPixel="%d"/>'


def ome_file(tmp_path, xml, pages):
    p = str(tmp_path / "o.ome.tif")
    R.write_tiff(p, [rgb_page(description=xml)] + [rgb_page() for _ in range(pages - 1)])
    return p


def test_ome_channel_groups(tmp_path):
    # SizeC = 6 as two RGB channels: 4 IFDs over (Z = 2) x (2 groups); XYCZT: the group runs fastest
    xml = OME % (IMG % ("XYCZT", 6, CH % (0, 3) + CH % (1, 3) +
                        '<TiffData IFD="0"/><TiffData IFD="1" FirstC="3"/><TiffData IFD="2" FirstZ="1"/>'))
    p = ome_file(tmp_path, xml, 4)
    lay = pbx.tiff_image_layout(p)
    assert (lay["size_z"], lay["size_c"], lay["samples"]) == (2, 6, 3)
    assert lay["planes"] == [(0, 0, 0), (0, 3, 0), (1, 0, 0), (1, 3, 0)]
    src = pbx.TiffSource({3: p})
    px = src.get_pixels(3)
    assert px.size_c == 6
    for c in range(6):
        ifd, sample = src._ifd(px, 1, c, 0, 0)
        assert ifd is src._open(3)["ifds"][2 + c // 3] and sample == c % 3
    lay = pbx.tiff_image_layout(ome_file(tmp_path, OME % (IMG % ("XYZCT", 6, CH % (0, 3) + CH % (1, 3))), 4))
    assert lay["planes"] == [(0, 0, 0), (1, 0, 0), (0, 3, 0), (1, 3, 0)]


OME_REFUSALS = [
    ("channel samples", IMG % ("XYCZT", 3, CH % (0, 1) + CH % (1, 1) + CH % (2, 1)),
     "Channel with SamplesPerPixel 1, the first IFD has 3"),
    ("absent counts as 1", IMG % ("XYCZT", 3, '<Channel ID="Channel:0:0"/>'),
     "Channel with SamplesPerPixel 1, the first IFD has 3"),
    ("size_c", IMG % ("XYCZT", 4, CH % (0, 3)), "SizeC 4 is no multiple of the IFDs' SamplesPerPixel 3"),
    ("first_c", IMG % ("XYCZT", 6, CH % (0, 3) + CH % (1, 3) + '<TiffData IFD="1" FirstC="1"/>'),
     "TiffData puts plane z=0 c=1 t=0 in IFD 1"),
    ("too few IFDs", IMG % ("XYCZT", 9, CH % (0, 3)), "names 6 planes, the file has 4 IFDs"),
]


@pytest.mark.parametrize("name,img,msg", OME_REFUSALS, ids=[r[0] for r in OME_REFUSALS])
def test_ome_refusals(tmp_path, name, img, msg):
    with pytest.raises(pbx.PbxError, match=re.escape(msg)) as e:
        pbx.tiff_image_layout(ome_file(tmp_path, OME % img, 4))
    assert e.value.status == 400
