"""Planes from TIFF / OME-TIFF files, host side (no GPU): the exports, the helper of the tests
(tests/_tiff_src.py) pinned against libtiff and the fixtures, the IFD reader on good and damaged
files, the host planner (pbx_test_tiff_plan) and every refusal of the C-ABI and the Python layer.

Fixtures: tests/golden/tiff/ (make_tiff_golden.py: tifffile, libtiff's tiffcp, PIL)."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest

import _tiff_src as T
import pbx

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "tiff")
with open(os.path.join(GOLD, "manifest.json")) as _f:
    FILES = json.load(_f)["files"]
IDS = [f["file"] for f in FILES]


def expected(entry, level="0", key="0,0,0"):
    """The plane's big-endian bytes."""
    npy = entry["planes"][level][key]
    if npy is None:  # the PIL-written ramp
        w, h = entry["width"], entry["length"]
        return ((np.arange(w)[None, :] % 100 + np.arange(h)[:, None] // 4) & 0xFF).astype(np.uint8).tobytes()
    return np.load(os.path.join(GOLD, npy)).tobytes()


# ------------------------------------------------------------------- exports and sizes
def test_exports_and_sizes():
    L = pbx.lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "pbx.h")).read()
    for name in ("pbx_planes_register_tiff", "pbx_test_tiff_plan"):
        assert name in pbx.EXPORTS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert "typedef struct pbx_tiff_segments" in header
    assert (pbx.TIFF_NONE, pbx.TIFF_LZW, pbx.TIFF_DEFLATE) == (1, 5, 8)
    assert re.search(r"PBX_TIFF_NONE = 1, PBX_TIFF_LZW = 5, PBX_TIFF_DEFLATE = 8", header)
    # the C value: the static_assert next to the planner
    rt = open(os.path.join(os.path.dirname(HERE), "omero-ms-pixel-buffer_amd", "csrc", "source_plan.cpp")).read()
    c_size = int(re.search(r"static_assert\(sizeof\(pbx_tiff_segments\) == (\d+)", rt).group(1))
    assert ctypes.sizeof(pbx.PbxTiffSegments) == c_size == 40
    assert pbx.PbxTiffSegments.data.offset == 24 and pbx.PbxTiffSegments.offsets.offset == 32
    assert L.pbx_abi_version() == 9
    sizes = (ctypes.c_uint64 * 16)()
    assert L.pbx_abi_sizes(sizes, 16) == 8


# --------------------------------------------------------------------------- the helper
def test_helper_encoder_decodes_under_libtiff(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, (100, 150), dtype=np.uint8)  # crosses every width change and a Clear
    smooth = (rng.poisson(6, (100, 150)) & 0xFF).astype(np.uint8)
    const = np.full((100, 150), 9, np.uint8)
    u16 = rng.integers(0, 65536, (100, 150)).astype("<u2")
    cases = [("noise", noise, dict(rows_per_strip=100), {}), ("smooth", smooth, dict(rows_per_strip=32), {}),
             ("const", const, dict(rows_per_strip=100), {}), ("tiles", smooth, dict(tile=(64, 64)), {}),
             ("pred", u16, dict(tile=(64, 64), predictor=2), {}),
             ("clears", smooth, dict(rows_per_strip=100), dict(clear_every=65)),
             ("clear_at", smooth, dict(rows_per_strip=100), dict(clear_at=(1, 2, 700)))]
    for name, a, geo, knobs in cases:
        p = str(tmp_path / (name + ".tif"))
        T.write_tiff(p, [T.page_of(a, 5, **geo, **knobs)])
        got = np.array(Image.open(p))
        assert got.dtype == a.dtype and (got == a).all(), name


def lzw_fixture_segments():
    for e in FILES:
        if e["compression"] != "lzw":
            continue
        path = os.path.join(GOLD, e["file"])
        for k, ifd in enumerate(pbx.tiff_ifds(path)):
            yield e, path, k, ifd


def test_helper_decoder_on_every_lzw_fixture():
    n = 0
    for e, path, k, ifd in lzw_fixture_segments():
        lay = pbx.tiff_image_layout(path)
        z, c, t = lay["planes"][k]
        bpp = ifd["bits"] // 8
        dt = np.dtype(ifd["byteorder"] + {1: "u", 2: "i", 3: "f"}[ifd["sampleformat"]] + str(bpp))
        want = np.frombuffer(expected(e, "0", "%d,%d,%d" % (z, c, t)), dt.newbyteorder(">")).reshape(
            ifd["length"], ifd["width"])
        data = open(path, "rb").read()
        gx = -(-ifd["width"] // ifd["seg_w"]) if ifd["tiled"] else 1
        for i, (o, cnt) in enumerate(zip(ifd["offsets"], ifd["counts"])):
            x0, y0 = (i % gx) * ifd["seg_w"], (i // gx) * ifd["seg_h"]
            rows = ifd["seg_h"] if ifd["tiled"] else min(ifd["seg_h"], ifd["length"] - y0)
            seg = np.frombuffer(T.lzw_decode(data[o:o + cnt], ifd["seg_w"] * rows * bpp), dt).reshape(rows, ifd["seg_w"])
            if ifd["predictor"] == 2:
                u = seg.astype(dt.newbyteorder("=")).view("u%d" % bpp)
                seg = np.cumsum(u, axis=1, dtype=u.dtype).view(dt.newbyteorder("="))
            piece = want[y0:y0 + rows, x0:x0 + ifd["seg_w"]]
            assert (seg[:piece.shape[0], :piece.shape[1]] == piece).all(), (e["file"], k, i)
            n += 1
    assert n > 100


def test_width_rule():
    rng = np.random.default_rng(0)
    codes, widths = [], []
    s = T.lzw_encode(rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), codes_out=codes)
    T.lzw_decode(s, widths=widths)
    clears = [i for i, (c, _) in enumerate(codes) if c == 256]
    assert clears[:2] == [0, 3837]  # the leading Clear, then a run of 3,836 codes and its Clear
    run = widths[1:3838]             # codes j = 0 .. 3836 of the run (j = 3836: the Clear)
    assert len(run) == 3837
    assert run == [9 + (j >= 254) + (j >= 766) + (j >= 1790) for j in range(3837)]
    assert [w for _, w in codes] == widths[:len(codes)]


def test_raw_code_packer_and_the_full_table():
    """lzw_pack writes the encoder's own codes to the encoder's own bytes (two runs, all four
    widths); the decoder takes the RUN_MAX codes that fill the table and refuses a further one."""
    data = np.random.default_rng(1).integers(0, 256, 5000, dtype=np.uint8).tobytes()
    codes = []
    s = T.lzw_encode(data, codes_out=codes)
    assert T.lzw_pack([c for c, _ in codes[1:]]) == s
    assert T.lzw_pack([c for c, _ in codes], leading_clear=False) == s
    lit = list(data[:T.RUN_MAX + 1])
    assert T.lzw_decode(T.lzw_pack(lit[:T.RUN_MAX] + [T.EOI])) == data[:T.RUN_MAX]
    assert T.lzw_decode(T.lzw_pack(lit[:T.RUN_MAX] + [T.CLEAR] + lit[:3] + [T.EOI])) == data[:T.RUN_MAX] + data[:3]
    with pytest.raises(ValueError, match="no Clear"):
        T.lzw_decode(T.lzw_pack(lit + [T.EOI]))


def test_predict2_wraps():
    a = np.array([[0, 65535, 1, 0]], ">u2")
    d = T.predict2(a)
    assert d.dtype == a.dtype and d.tolist() == [[0, 65535, 2, 65535]]


# ---------------------------------------------------------------------------- tiff_ifds
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_tiff_ifds_on_fixture(entry):
    path = os.path.join(GOLD, entry["file"])
    ifds = pbx.tiff_ifds(path)
    d = ifds[0]
    assert (d["width"], d["length"]) == (entry["width"], entry["length"])
    assert d["tiled"] == (entry["layout"] == "tiles")
    assert d["compression"] in {"none": (1,), "lzw": (5,), "deflate": (8, 32946)}[entry["compression"]]
    assert d["predictor"] == entry["predictor"] and d["byteorder"] == entry["byteorder"]
    assert d["bigtiff"] == entry["bigtiff"] and d["spp"] == 1
    gx = -(-d["width"] // d["seg_w"]) if d["tiled"] else 1
    assert len(d["offsets"]) == len(d["counts"]) == gx * -(-d["length"] // d["seg_h"])
    if d["tiled"]:
        assert d["seg_w"] % 16 == 0 and d["seg_h"] % 16 == 0
    else:
        assert d["seg_w"] == d["width"] and d["length"] % d["seg_h"] != 0  # a short last strip
    lay = pbx.tiff_image_layout(path)
    assert lay["levels"] == len(entry["planes"]) == 1 + len(d["subifds"])
    assert sorted("%d,%d,%d" % p for p in lay["planes"]) == sorted(entry["planes"]["0"])
    spec = pbx.tiff_plane_spec(path, d, 1, 0, 0, 0)
    assert spec["compression"] in (1, 5, 8) and int(spec["segments"][1][-1]) == sum(d["counts"])
    assert spec["big_endian"] == (entry["byteorder"] == ">")


def test_ome_axes():
    entry = next(e for e in FILES if "ome" in e)
    lay = pbx.tiff_image_layout(os.path.join(GOLD, entry["file"]))
    assert (lay["size_z"], lay["size_c"], lay["size_t"]) == (2, 3, 2) and len(lay["ifds"]) == 12
    # DimensionOrder XYCTZ: c runs fastest over the IFDs, then t, then z
    assert lay["planes"] == [(z, c, t) for z in range(2) for t in range(2) for c in range(3)]
    assert "DimensionOrder=\"XYCTZ\"" in lay["ifds"][0]["description"]


def test_subifds_are_levels():
    entry = next(e for e in FILES if e["file"].startswith("pyramid"))
    d = pbx.tiff_ifds(os.path.join(GOLD, entry["file"]))
    assert len(d) == 1 and [(s["width"], s["length"]) for s in d[0]["subifds"]] == [(75, 50), (38, 25)]


def small_tiff(tmp_path, name="a.tif", **kw):
    a = (np.arange(40 * 30).reshape(30, 40) % 251).astype(np.uint8)
    p = str(tmp_path / name)
    page = T.page_of(a, kw.pop("compression", 1), rows_per_strip=kw.pop("rows_per_strip", 8), **kw)
    return p, page, a


def test_damaged_files(tmp_path):
    p, page, _ = small_tiff(tmp_path)
    good = T.write_tiff(p, [page, page])
    assert len(pbx.tiff_ifds(p)) == 2
    first = struct.unpack("<I", good[4:8])[0]

    def written(b, name):
        q = str(tmp_path / name)
        open(q, "wb").write(b)
        return q
    # the first IFD's offset past the end of the file
    with pytest.raises(pbx.PbxError, match="past the end of the file") as e:
        pbx.tiff_ifds(written(good[:4] + struct.pack("<I", len(good) + 10) + good[8:], "eof.tif"))
    assert e.value.status == 400
    # a strip offset past the end of the file
    n = struct.unpack("<H", good[first:first + 2])[0]
    bad = bytearray(good)
    for k in range(n):
        at = first + 2 + 12 * k
        if struct.unpack("<H", bad[at:at + 2])[0] == 273:
            off = struct.unpack("<I", bad[at + 8:at + 12])[0]  # 4 strips: out of line
            struct.pack_into("<I", bad, off, len(good))
    with pytest.raises(pbx.PbxError, match="segment at offset .* past the end of the file") as e:
        pbx.tiff_ifds(written(bytes(bad), "seg.tif"))
    assert e.value.status == 400
    # the second IFD's next pointer leads back to the first
    loop = bytearray(good)
    nxt1 = first + 2 + 12 * n
    second = struct.unpack("<I", loop[nxt1:nxt1 + 4])[0]
    n2 = struct.unpack("<H", loop[second:second + 2])[0]
    struct.pack_into("<I", loop, second + 2 + 12 * n2, first)
    with pytest.raises(pbx.PbxError, match="IFD loop") as e:
        pbx.tiff_ifds(written(bytes(loop), "loop.tif"))
    assert e.value.status == 400
    # a file cut inside its last IFD
    with pytest.raises(pbx.PbxError, match="past the end of the file") as e:
        pbx.tiff_ifds(written(good[:len(good) - 7], "cut.tif"))
    assert e.value.status == 400
    with pytest.raises(pbx.PbxError, match="not a TIFF") as e:
        pbx.tiff_ifds(written(b"PK\3\4" + good[4:], "zip.tif"))
    assert e.value.status == 400


# ------------------------------------------------------------------------- the planner
def plan(segs, size_x, size_y, bpp, seg_w, seg_h, tiled, compression, predictor=1, flags=0, offsets=None,
         null=None):
    data, offs = pbx.pack_chunks(segs)
    if offsets is not None:
        offs = np.array(offsets, np.uint64)
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor, s.flags = seg_w, seg_h, tiled, compression, predictor, flags
    s.data = None if null == "data" else data.ctypes.data
    s.offsets = None if null == "offsets" else offs.ctypes.data
    out = (ctypes.c_uint64 * 4)()
    rc = pbx.lib().pbx_test_tiff_plan(None if null == "segs" else ctypes.byref(s), size_x, size_y, bpp,
                                      None if null == "out" else out)
    return rc, list(out), pbx.lib().pbx_last_error().decode()


def test_plan_counts_short_last_strip():
    # 150 x 100 uint16 in strips of 32 rows: 3 full strips and one of 4 rows
    segs = [b"\0" * (150 * 32 * 2)] * 3 + [b"\0" * (150 * 4 * 2)]
    rc, out, _ = plan(segs, 150, 100, 2, 150, 32, 0, 1)
    assert rc == 0 and out[0] == 4 and out[1] == 150 * 100 * 2 and out[3] == 0
    assert out[2] == 3 * 9728 + 1280  # every segment's bytes rounded up to 256
    rc, out, _ = plan([b"\x80\0\1"] * 4, 150, 100, 2, 150, 32, 0, 5, predictor=2)
    assert rc == 0 and out[:2] == [4, 150 * 100 * 2] and out[3] == 1


def test_plan_counts_padded_edge_tiles():
    # 150 x 100 uint8 in 64 x 64 tiles: 3 x 2 tiles, every one full
    rc, out, _ = plan([b"x\x9c\3\0"] * 6, 150, 100, 1, 64, 64, 1, 8)
    assert rc == 0 and out == [6, 6 * 64 * 64, 6 * 64 * 64, 0]
    rc, out, _ = plan([b"\0" * 4096] * 6, 150, 100, 1, 64, 64, 1, 1, predictor=2)
    assert rc == 0 and out == [6, 6 * 4096, 6 * 4096, 1]


REFUSALS = [
    ("null segs", dict(null="segs"), "null argument"),
    ("null data", dict(null="data"), "null argument"),
    ("null offsets", dict(null="offsets"), "null argument"),
    ("null out", dict(null="out"), "null argument"),
    ("offsets decrease", dict(offsets=[0, 8, 4, 12, 16]), "bad offsets"),
    ("empty segment", dict(offsets=[0, 8, 8, 12, 16]), "segment 1 is empty"),
    ("seg_w 0", dict(seg_w=0), "bad segment shape"),
    ("seg_h 0", dict(seg_h=0), "bad segment shape"),
    ("tile width 24", dict(tiled=1, seg_w=24, seg_h=32), "multiples of 16"),
    ("tile length 40", dict(tiled=1, seg_w=32, seg_h=40), "multiples of 16"),
    ("strip width", dict(seg_w=149), "strip width 149 != plane width 150"),
    ("compression 7", dict(compression=7), "bad compression 7"),
    ("compression 32946", dict(compression=32946), "bad compression 32946"),
    ("predictor 3", dict(predictor=3), "bad predictor 3"),
    ("predictor 0", dict(predictor=0), "bad predictor 0"),
    ("predictor 2 on double", dict(predictor=2, bpp=8), "predictor 2 on floating-point"),
    ("flags", dict(flags=1), "bad flags"),
    ("uncompressed length", dict(compression=1), "uncompressed segment 0: 4 bytes, not 9600"),
    ("old-style LZW", dict(segs=[b"\0\1\2\3"] * 4), "old-style"),
]


@pytest.mark.parametrize("name,change,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_planner_refusals(name, change, msg):
    a = dict(segs=[b"\x80\0\1\2"] * 4, size_x=150, size_y=100, bpp=2, seg_w=150, seg_h=32, tiled=0,
             compression=5)
    a.update(change)
    rc, _, err = plan(**a)
    assert rc == 400 and msg in err, (rc, err)


def test_old_style_lzw_is_libtiffs_test():
    # first byte 0 and bit 0 of the second byte: refused; either alone is a TIFF 6.0 stream
    ok = dict(size_x=150, size_y=100, bpp=2, seg_w=150, seg_h=32, tiled=0, compression=5)
    assert plan([b"\0\2\0\0"] * 4, **ok)[0] == 0
    assert plan([b"\1\1\0\0"] * 4, **ok)[0] == 0
    assert plan([b"\0\3\0\0"] * 4, **ok)[0] == 400


# -------------------------------------------------------------------- the Python layer
def write_with(tmp_path, name, extra=(), **change):
    p, page, _ = small_tiff(tmp_path, name)
    page.update(change)
    page["extra"] = list(extra)
    T.write_tiff(p, [page])
    return p


PY_REFUSALS = [
    ("spp", dict(spp=3), (), "SamplesPerPixel 3"),
    ("bits", dict(bits=12), (), "BitsPerSample 12"),
    ("sampleformat", dict(sampleformat=6), (), "SampleFormat 6"),
    ("int64", dict(bits=64, sampleformat=1), (), "SampleFormat 1 with 64 bits"),
    ("compression", dict(compression=7), (), "Compression 7"),
    ("packbits", dict(compression=32773), (), "Compression 32773"),
    ("predictor3", dict(predictor=3), (), "Predictor 3"),
    ("predictor2 float", dict(predictor=2, bits=32, sampleformat=3), (), "Predictor 2 on floating-point"),
    ("fillorder", {}, [(266, 3, [2])], "FillOrder 2"),
    ("orientation", {}, [(274, 3, [3])], "Orientation 3"),
]


@pytest.mark.parametrize("name,change,extra,msg", PY_REFUSALS, ids=[r[0] for r in PY_REFUSALS])
def test_python_refusals(tmp_path, name, change, extra, msg):
    p = write_with(tmp_path, "r.tif", extra, **change)
    with pytest.raises(pbx.PbxError, match=re.escape(msg)) as e:
        pbx.tiff_image_layout(p)
    assert e.value.status == 400
    with pytest.raises(pbx.PbxError, match=re.escape(msg)) as e:
        pbx.tiff_plane_spec(p, pbx.tiff_ifds(p)[0], 1, 0, 0, 0)
    assert e.value.status == 400


OME = ('<?xml version="1.0"?><OME xmlns="http://www.openmicroscopy.org/Schemas/OME/2016-06">%s</OME>')
IMG = ('<Image ID="Image:%d"><Pixels ID="Pixels:%d" DimensionOrder="XYZCT" Type="uint8" SizeX="40" SizeY="30" '
       'SizeZ="2" SizeC="1" SizeT="1">%s</Pixels></Image>')


def ome_file(tmp_path, xml, pages=2):
    p, page, _ = small_tiff(tmp_path, "o.ome.tif")
    first = dict(page, description=xml)
    T.write_tiff(p, [first] + [page] * (pages - 1))
    return p


def test_ome_refusals_and_restated_order(tmp_path):
    ok = OME % (IMG % (0, 0, '<TiffData IFD="0" FirstZ="0" PlaneCount="1"/><TiffData IFD="1" FirstZ="1"/>'))
    lay = pbx.tiff_image_layout(ome_file(tmp_path, ok))
    assert lay["planes"] == [(0, 0, 0), (1, 0, 0)] and lay["size_z"] == 2
    same = OME % (IMG % (0, 0, '<TiffData><UUID FileName="o.ome.tif">urn:uuid:0</UUID></TiffData>'))
    assert pbx.tiff_image_layout(ome_file(tmp_path, same))["size_z"] == 2
    for xml, msg in (
            (OME % (IMG % (0, 0, '<TiffData><UUID FileName="other.ome.tif">urn:uuid:0</UUID></TiffData>')),
             "names another file"),
            (OME % ((IMG % (0, 0, "")) + (IMG % (1, 1, ""))), "2 Image elements"),
            (OME % (IMG % (0, 0, '<TiffData IFD="0" FirstZ="1"/>')), "not in DimensionOrder"),
            (OME % (IMG % (0, 0, "")).replace("XYZCT", "XYZTT"), "DimensionOrder"),
            (OME % (IMG % (0, 0, "")).replace('Type="uint8"', 'Type="uint16"'), "disagree with the first IFD")):
        with pytest.raises(pbx.PbxError, match=msg) as e:
            pbx.tiff_image_layout(ome_file(tmp_path, xml))
        assert e.value.status == 400
    with pytest.raises(pbx.PbxError, match="names 2 planes, the file has 1 IFDs") as e:
        pbx.tiff_image_layout(ome_file(tmp_path, OME % (IMG % (0, 0, "")), pages=1))
    assert e.value.status == 400


def test_plain_pages_are_timepoints(tmp_path):
    p, page, _ = small_tiff(tmp_path, "pages.tif")
    T.write_tiff(p, [page] * 3, byteorder=">", bigtiff=True)
    lay = pbx.tiff_image_layout(p)
    assert lay["planes"] == [(0, 0, 0), (0, 0, 1), (0, 0, 2)] and (lay["size_z"], lay["size_c"], lay["size_t"]) == (1, 1, 3)
    src = pbx.TiffSource({5: p})
    px = src.get_pixels(5)
    assert (px.size_x, px.size_y, px.size_t, px.levels, px.pixel_type) == (40, 30, 3, 1, pbx.UINT8)
    assert src.get_pixels(6) is None
    sp = src.plane_segments(px, 0, 0, 2, 0)
    assert (sp["t"], sp["seg_h"], sp["tiled"], sp["big_endian"]) == (2, 8, False, True)
