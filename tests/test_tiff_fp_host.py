"""Float TIFF with the floating-point predictor (Predictor = 3) and Zstandard TIFF (Compression =
50000), host side (no GPU): the numpy restatement of the predictor (tests/_tiff_fp.py) pinned
against the tifffile- and libtiff-written fixtures of tests/golden/tiff_fp/ and against libtiff
(through PIL), the host planner's counts for the new kinds, and every new refusal of the C-ABI
and of the Python layer with its message."""
import builtins
import ctypes
import os
import re

import numpy as np
import pytest

import _tiff_fp as F
import _tiff_src as T
import _zarr
import pbx

FILES = F.manifest()
IDS = [f["file"] for f in FILES]


def fixture_planes(entry):
    """(IFD, sample group, expected big-endian array) of every plane of every level."""
    path = os.path.join(F.GOLD, entry["file"])
    main = pbx.tiff_ifds(path)[0]
    for level, ifd in enumerate([main] + main["subifds"]):
        for key, ref in sorted(entry["planes"][str(level)].items()):
            yield ifd, int(key.split(",")[1]), F.expected(ref)


# ------------------------------------------------------------------- exports and the rule
def test_exports_and_values():
    header = open(os.path.join(os.path.dirname(F.HERE), "include", "pbx.h")).read()
    assert pbx.TIFF_ZSTD == 50000 == F.ZSTD
    assert re.search(r"PBX_TIFF_DEFLATE = 8, PBX_TIFF_ZSTD = 50000 }", header)
    assert pbx.lib().pbx_abi_version() == 9 and ctypes.sizeof(pbx.PbxTiffSegments) == 40


def test_rule_on_a_worked_row():
    # two big-endian float32 samples 0x01020304, 0x11121314: planes 01 11 | 02 12 | 03 13 | 04 14
    a = np.array([[0x01020304, 0x11121314]], ">u4").view(">f4")
    d = F.predict3(a)
    assert d.tolist() == [[0x01, 0x10, 0xF1, 0x10, 0xF1, 0x10, 0xF1, 0x10]]
    assert (F.predict3(a.astype("<f4")) == d).all()  # the encoded bytes do not depend on the byte order
    assert F.unpredict3(d, ">f4").tobytes() == a.tobytes()
    assert F.unpredict3(d, "<f4").tobytes() == a.astype("<f4").tobytes()


@pytest.mark.parametrize("dt", ["<f4", ">f4", "<f8", ">f8"])
def test_forward_and_inverse_on_random_bits(dt):
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 256, 7 * 33 * np.dtype(dt).itemsize, dtype=np.uint8)
    a = raw.view(dt).reshape(7, 33)
    assert F.unpredict3(F.predict3(a), dt).tobytes() == a.tobytes()


# ------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_decodes_on_the_cpu(entry):
    """zlib / libzstd / the Python LZW decoder and the numpy inverse give the .npy plane."""
    path = os.path.join(F.GOLD, entry["file"])
    ifd0 = pbx.tiff_ifds(path)[0]
    assert ifd0["predictor"] == entry["predictor"] and ifd0["byteorder"] == entry["byteorder"]
    assert ifd0["compression"] == {"deflate": 8, "zstd": 50000, "lzw": 5}[entry["compression"]]
    assert ifd0["bigtiff"] == entry["bigtiff"] and ifd0["tiled"] == (entry["layout"] == "tiles")
    n = 0
    for ifd, sample, want in fixture_planes(entry):
        got = F.decode_ifd(path, ifd, sample)
        assert got.astype(got.dtype.newbyteorder(">")).tobytes() == want.tobytes(), (entry["file"], sample)
        n += 1
    assert n == sum(len(v) for v in entry["planes"].values())


def test_fixtures_cover_every_pair_of_layout_codec_and_byte_order():
    have = {(e["layout"], e["compression"], e["predictor"], e["byteorder"]) for e in FILES}
    for layout in ("strips", "tiles"):
        for comp in ("deflate", "zstd", "lzw"):
            assert any(h[:3] == (layout, comp, 3) for h in have)
    for comp in ("deflate", "zstd", "lzw"):
        for bo in "<>":
            assert any((h[1], h[2], h[3]) == (comp, 3, bo) for h in have)
    for pred in (1, 2):
        assert {e["writer"] for e in FILES if e["compression"] == "zstd" and e["predictor"] == pred} == \
            {"tifffile", "tiffcp"}
    assert any(e["bigtiff"] for e in FILES) and any(len(e["planes"]) == 3 for e in FILES)
    assert any(e.get("samples") == 2 for e in FILES)
    sizes = [os.path.getsize(os.path.join(F.GOLD, f)) for f in os.listdir(F.GOLD)]
    assert max(sizes) <= 64 * 1024 and sum(sizes) < 1 << 20


def test_both_zstd_frame_shapes_are_in_the_fixtures():
    shapes = set()
    for e in FILES:
        if e["compression"] != "zstd":
            continue
        path = os.path.join(F.GOLD, e["file"])
        ifd = pbx.tiff_ifds(path)[0]
        with open(path, "rb") as f:
            f.seek(ifd["offsets"][0])
            head = f.read(6)
        assert head[:4] == b"\x28\xb5\x2f\xfd"
        shapes.add((e["writer"], (head[4] >> 5) & 1, head[4] >> 6))  # Single_Segment, Frame_Content_Size flag
    assert ("tifffile", 1, 1) in shapes  # a single-segment frame with a 2-byte content size
    assert ("tiffcp", 0, 0) in shapes    # a window descriptor, no content size


# (PIL has no image mode for float64 samples or for two float samples: it does not open those)
PIL_FILES = [e for e in FILES if e["byteorder"] == "<" and not e.get("samples") and not e["file"].startswith("double")]


@pytest.mark.parametrize("entry", PIL_FILES, ids=[e["file"] for e in PIL_FILES])
def test_pil_decodes_every_II_fixture(entry):
    """libtiff (through PIL) agrees on every II file it has a mode for.  (It gives wrong values
    for MM Predictor 3 files, which are pinned by tifffile and by the rule above.)"""
    Image = pytest.importorskip("PIL.Image")
    want = F.expected(entry["planes"]["0"]["0,0,0"])
    got = np.array(Image.open(os.path.join(F.GOLD, entry["file"])))
    assert got.astype(want.dtype).tobytes() == want.tobytes()


# --------------------------------------------------------------------------- the planner
def plan(segs, size_x, size_y, bpp, seg_w, seg_h, tiled, compression, predictor=1, spp=1, y0=0, rows=0):
    data, offs = pbx.pack_chunks(segs)
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor, s.flags = seg_w, seg_h, tiled, compression, predictor, 0
    s.data, s.offsets = data.ctypes.data, offs.ctypes.data
    out = (ctypes.c_uint64 * 4)()
    L = pbx.lib()
    if spp == 1 and rows == 0:
        rc = L.pbx_test_tiff_plan(ctypes.byref(s), size_x, size_y, bpp, out)
    elif spp == 1:
        rc = L.pbx_test_tiff_band_plan(ctypes.byref(s), size_x, size_y, bpp, y0, rows, out)
    else:
        rc = L.pbx_test_tiff_plan_samples(ctypes.byref(s), size_x, size_y, bpp, spp, y0, rows, out)
    return rc, list(out), L.pbx_last_error().decode()


def r256(n):
    return (n + 255) & ~255


def frames(dlens):
    return [_zarr.zstd_frame(bytes(n)) for n in dlens]


@pytest.mark.parametrize("bpp", [4, 8])
def test_plan_predictor3_counts(bpp):
    # 150 x 100 in strips of 32 rows: 3 full strips and one of 4 rows
    dl = [150 * r * bpp for r in (32, 32, 32, 4)]
    for comp, segs in ((8, [b"x\x9c\3\0"] * 4), (5, [b"\x80\0\1"] * 4), (50000, frames(dl))):
        rc, out, err = plan(segs, 150, 100, bpp, 150, 32, 0, comp, 3)
        assert rc == 0, err
        assert out == [4, sum(dl), sum(r256(n) for n in dl), 4]  # a stream and a TPlace per segment
        # rows [40, 70): strips 1 and 2
        rc, out, err = plan(segs[1:3], 150, 100, bpp, 150, 32, 0, comp, 3, y0=40, rows=30)
        assert rc == 0 and out == [2, dl[1] + dl[2], r256(dl[1]) + r256(dl[2]), 2], err
    # 64 x 64 tiles: 3 x 2, every one full; pbx_test_tiff_plan_samples with one sample agrees
    t = 64 * 64 * bpp
    rc, out, err = plan(frames([t] * 6), 150, 100, bpp, 64, 64, 1, 50000, 3)
    assert rc == 0 and out == [6, 6 * t, 6 * t, 6], err
    data, offs = pbx.pack_chunks(frames([t] * 3))
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor = 64, 64, 1, 50000, 3
    s.data, s.offsets = data.ctypes.data, offs.ctypes.data
    out = (ctypes.c_uint64 * 4)()
    assert pbx.lib().pbx_test_tiff_plan_samples(ctypes.byref(s), 150, 100, bpp, 1, 70, 30, out) == 0
    assert list(out) == [3, 3 * t, 3 * t, 3]


@pytest.mark.parametrize("bpp", [4, 8])
def test_plan_stored_predictor3_needs_no_stream_and_no_scratch(bpp):
    segs = [bytes(150 * r * bpp) for r in (32, 32, 32, 4)]
    rc, out, err = plan(segs, 150, 100, bpp, 150, 32, 0, 1, 3)
    assert rc == 0 and out == [0, 150 * 100 * bpp, 0, 4], err  # registration too: read where it was uploaded
    rc, out, err = plan(segs[2:], 150, 100, bpp, 150, 32, 0, 1, 3, y0=90, rows=10)
    assert rc == 0 and out == [0, 150 * 36 * bpp, 0, 2], err
    # Predictor 1 still copies stored segments into scratch at registration
    rc, out, _ = plan(segs, 150, 100, bpp, 150, 32, 0, 1, 1)
    assert rc == 0 and out[0] == 4 and out[2] > 0 and out[3] == 0


@pytest.mark.parametrize("pred,bpp,spp", [(1, 1, 1), (2, 2, 1), (2, 4, 1), (1, 8, 1), (1, 1, 3), (2, 2, 4)])
def test_plan_zstd_behind_the_other_predictors(pred, bpp, spp):
    dl = [150 * r * bpp * spp for r in (32, 32, 32, 4)]
    rc, out, err = plan(frames(dl), 150, 100, bpp, 150, 32, 0, 50000, pred, spp)
    assert rc == 0, err
    assert out == [4, sum(dl), sum(r256(n) for n in dl), 4 if spp > 1 else pred - 1]
    rc, out, err = plan(frames(dl[1:3]), 150, 100, bpp, 150, 32, 0, 50000, pred, spp, y0=33, rows=40)
    assert rc == 0 and out == [2, dl[1] + dl[2], r256(dl[1]) + r256(dl[2]), 2 if spp > 1 else pred - 1], err


def test_plan_old_inputs_are_unchanged():
    """The figures of tests/test_tiff_src_host.py, restated: nothing of today's planning moved."""
    segs = [b"\0" * (150 * 32 * 2)] * 3 + [b"\0" * (150 * 4 * 2)]
    assert plan(segs, 150, 100, 2, 150, 32, 0, 1)[1] == [4, 30000, 3 * 9728 + 1280, 0]
    assert plan([b"\x80\0\1"] * 4, 150, 100, 2, 150, 32, 0, 5, 2)[1] == [4, 30000, 3 * 9728 + 1280, 1]
    assert plan([b"\0" * 9600] * 2, 150, 100, 2, 150, 32, 0, 1, 2, y0=40, rows=30)[1] == [0, 19200, 0, 1]


def frame_with(fhd_or=0, fcs=None, tail=b""):
    f = bytearray(_zarr.zstd_frame(bytes(150 * 32 * 4)))
    assert f[4] >> 6 == 1 and (f[4] >> 5) & 1  # libzstd: single segment, a 2-byte content size
    f[4] |= fhd_or
    if fcs is not None:
        f[5:7] = int(fcs - 256).to_bytes(2, "little")
    return bytes(f) + tail


PLAN_REFUSALS = [
    ("p3 on bytes", dict(bpp=1, predictor=3), "bad predictor 3 (the floating-point predictor) on 1-byte samples"),
    ("p3 on shorts", dict(bpp=2, predictor=3), "bad predictor 3 (the floating-point predictor) on 2-byte samples"),
    ("p3 on rgb", dict(bpp=4, predictor=3, spp=3), "bad predictor 3 (the floating-point predictor) on chunky "
                                                   "segments of 3 samples per pixel"),
    ("predictor 4", dict(predictor=4), "bad predictor 4"),
    ("compression 50001", dict(compression=50001), "bad compression 50001 (1 none, 5 LZW, 8 deflate, 50000 zstd)"),
    ("not a frame", dict(compression=50000, segs=[b"x\x9c\3\0\0\0\0\0"] * 4), "segment 0: not a zstd frame"),
    ("short frame", dict(compression=50000, segs=[b"\x28\xb5\x2f\xfd"] * 4), "segment 0: short zstd frame"),
    ("content size", dict(compression=50000, bpp=4, segs=[frame_with()] * 4),
     "segment 3: zstd content size 19200 != segment bytes 2400"),
    ("content size field", dict(compression=50000, bpp=4, segs=[frame_with(fcs=19201)] * 4),
     "segment 0: zstd content size 19201 != segment bytes 19200"),
    ("bytes after", dict(compression=50000, bpp=4, segs=[frame_with(tail=b"\0\0")] * 4),
     "segment 0: 2 bytes after the zstd frame"),
    ("dictionary id", dict(compression=50000, bpp=4, segs=[frame_with(fhd_or=1)] * 4),
     "segment 0: zstd frame with a dictionary id"),
    ("skippable", dict(compression=50000, segs=[b"\x50\x2a\x4d\x18\4\0\0\0abcd"] * 4), "segment 0: skippable zstd frame"),
]


@pytest.mark.parametrize("name,change,msg", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_planner_refusals(name, change, msg):
    a = dict(segs=[b"\x80\0\1\2"] * 4, size_x=150, size_y=100, bpp=2, seg_w=150, seg_h=32, tiled=0, compression=5)
    a.update(change)
    for band in ({}, dict(y0=0, rows=100)):
        rc, _, err = plan(**a, **band)
        assert rc == 400 and msg in err, (rc, err)


# -------------------------------------------------------------------- the Python layer
def fp_file(tmp_path, name="f.tif", **change):
    a = (np.arange(40 * 30).reshape(30, 40) / 7).astype("<f4")
    page = F.page_of(a, 8, 3, rows_per_strip=8)
    page.update(change)
    p = str(tmp_path / name)
    T.write_tiff(p, [page])
    return p, a


def test_python_accepts_predictor3_and_zstd(tmp_path):
    p, a = fp_file(tmp_path)
    ifd = pbx.tiff_ifds(p)[0]
    sp = pbx.tiff_plane_spec(p, ifd, 1, 0, 0, 0)
    assert (sp["pixel_type"], sp["predictor"], sp["compression"], sp["samples_per_pixel"]) == (pbx.FLOAT, 3, 8, 1)
    assert pbx.tiff_image_layout(p)["pixel_type"] == pbx.FLOAT
    assert F.decode_ifd(p, ifd).tobytes() == a.tobytes()
    p = str(tmp_path / "z.tif")
    T.write_tiff(p, [F.page_of(a.astype(">f8"), F.ZSTD, 3, tile=(16, 16))], byteorder=">")
    ifd = pbx.tiff_ifds(p)[0]
    sp = pbx.tiff_band_spec(p, ifd, 16, 10)
    assert (sp["pixel_type"], sp["predictor"], sp["compression"], sp["big_endian"]) == (pbx.DOUBLE, 3, 50000, True)
    assert len(sp["segments"][1]) == 3 + 1  # rows 16 .. 25: tile row 1 of 40 / 16 -> 3 tiles


def test_python_accepts_planar_predictor3():
    entry = next(e for e in FILES if e.get("samples") == 2)
    path = os.path.join(F.GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    assert (lay["samples"], lay["size_c"], lay["pixel_type"]) == (2, 2, pbx.FLOAT)
    for sample in (0, 1):
        sp = pbx.tiff_plane_spec(path, lay["ifds"][0], 1, 0, sample, 0, sample=sample)
        assert (sp["samples_per_pixel"], sp["sample"], sp["predictor"], sp["compression"]) == (1, 0, 3, 50000)


PY_REFUSALS = [
    ("p3 on uint8", dict(bits=8, sampleformat=1), "Predictor 3 (the floating-point predictor) on integer samples"),
    ("p3 on int32", dict(bits=32, sampleformat=2), "Predictor 3 (the floating-point predictor) on integer samples"),
    ("half", dict(bits=16, sampleformat=3), "SampleFormat 3 with 16 bits"),
    ("predictor 4", dict(predictor=4), "Predictor 4 (1, 2, or 3 on floating-point samples)"),
    ("lzma", dict(compression=34925), "Compression 34925 (1 none, 5 LZW, 8 / 32946 deflate, 50000 zstd)"),
    ("jpeg", dict(compression=7), "Compression 7 (1 none"),
    ("packbits", dict(compression=32773), "Compression 32773 (1 none"),
]


@pytest.mark.parametrize("name,change,msg", PY_REFUSALS, ids=[r[0] for r in PY_REFUSALS])
def test_python_refusals(tmp_path, name, change, msg):
    p, _ = fp_file(tmp_path, **change)
    for call in (lambda: pbx.tiff_image_layout(p), lambda: pbx.tiff_plane_spec(p, pbx.tiff_ifds(p)[0], 1, 0, 0, 0),
                 lambda: pbx.tiff_band_spec(p, pbx.tiff_ifds(p)[0], 0, 0)):
        with pytest.raises(pbx.PbxError, match=re.escape(msg)) as e:
            call()
        assert e.value.status == 400


def test_python_refuses_predictor3_on_chunky_samples(tmp_path):
    """RGB float with Predictor 3 is out of scope: the IFD of a float file, restated as chunky with
    three samples (tests/_tiff_src.py writes one BitsPerSample value)."""
    p, _ = fp_file(tmp_path)
    ifd = dict(pbx.tiff_ifds(p)[0], spp=3, bits_count=3, photometric=2, planar=1)
    for call in (lambda: pbx.tiff_plane_spec(p, ifd, 1, 0, 0, 0), lambda: pbx.tiff_band_spec(p, ifd, 0, 0)):
        with pytest.raises(pbx.PbxError, match=re.escape("Predictor 3 (the floating-point predictor) on chunky "
                                                         "segments of 3 samples per pixel")) as e:
            call()
        assert e.value.status == 400
    with pytest.raises(pbx.PbxError, match="segments for 3 planar samples"):  # planar: past the predictor check
        pbx.tiff_plane_spec(p, dict(ifd, planar=2), 1, 0, 0, 0)


# ----------------------------------------------------------------------- tiff_band_spec
def test_band_spec_reads_only_the_covering_segment_rows_of_a_zstd_file(monkeypatch):
    entry = next(e for e in FILES if e["file"] == "float_tiles_zstd_p3_II.tif")
    path = os.path.join(F.GOLD, entry["file"])
    ifd = pbx.tiff_ifds(path)[0]
    gx = -(-ifd["width"] // ifd["seg_w"])
    reads = []
    real_open = builtins.open

    class Spy:
        def __init__(self, f):
            self.f = f

        def __enter__(self):
            return self

        def __exit__(self, *a):
            self.f.close()

        def seek(self, o):
            self.at = o
            return self.f.seek(o)

        def readinto(self, b):
            reads.append((self.at, len(b)))
            return self.f.readinto(b)

    def spy_open(p, mode="r", *a, **kw):
        f = real_open(p, mode, *a, **kw)
        return Spy(f) if os.path.abspath(str(p)) == os.path.abspath(path) else f

    monkeypatch.setattr(builtins, "open", spy_open)
    sp = pbx.tiff_band_spec(path, ifd, 70, 20)  # tile row 1 alone
    assert reads == list(zip(ifd["offsets"][gx:2 * gx], ifd["counts"][gx:2 * gx]))
    assert len(sp["segments"][1]) == gx + 1 and sp["compression"] == pbx.TIFF_ZSTD and sp["predictor"] == 3
    del reads[:]
    assert pbx.tiff_band_spec(path, ifd, 0, 0)["segments"] is None and reads == []
