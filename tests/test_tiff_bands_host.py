"""TIFF strips and tile rows on demand, the host side (no GPU): the pbx_band_write_tiff and
pbx_test_tiff_band_plan exports, the band planner's counts and refusals, tiff_band_spec on every
fixture of tests/golden/tiff and TiffSource.band_segments."""
import builtins
import ctypes
import json
import os
import re

import numpy as np
import pytest

import pbx
from test_tiff_src_host import REFUSALS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "tiff")
with open(os.path.join(GOLD, "manifest.json")) as _f:
    FILES = json.load(_f)["files"]
IDS = [f["file"] for f in FILES]


# ------------------------------------------------------------------------------ exports
def test_exports_and_signatures():
    L = pbx.lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "pbx.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in ("pbx_band_write_tiff", "pbx_test_tiff_band_plan"):
        assert name in pbx.EXPORTS and hasattr(L, name)
    assert ("int pbx_band_write_tiff(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows, "
            "const pbx_tiff_segments* segs, double* kernel_ms);") in flat
    assert ("int pbx_test_tiff_band_plan(const pbx_tiff_segments* segs, int32_t size_x, int32_t size_y, "
            "int32_t bpp, int32_t y0, int32_t rows, uint64_t out[4]);") in flat
    assert len(L.pbx_band_write_tiff.argtypes) == 6 and len(L.pbx_test_tiff_band_plan.argtypes) == 7
    # nothing of the ABI moved
    assert L.pbx_abi_version() == 9
    sizes = (ctypes.c_uint64 * 16)()
    assert L.pbx_abi_sizes(sizes, 16) == 8
    assert ctypes.sizeof(pbx.PbxTiffSegments) == 40
    # null arguments are refused before anything is touched
    s = pbx.PbxTiffSegments()
    assert L.pbx_band_write_tiff(None, 1, 0, 1, ctypes.byref(s), None) == pbx.E_BADARG
    assert L.pbx_band_write_tiff(None, 1, 0, 1, None, None) == pbx.E_BADARG


# -------------------------------------------------------------------------- the planner
def band_plan(segs, size_x, size_y, bpp, y0, rows, seg_w, seg_h, tiled, compression, predictor=1, flags=0,
              offsets=None, null=None):
    data, offs = pbx.pack_chunks(segs)
    if offsets is not None:
        offs = np.array(offsets, np.uint64)
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor, s.flags = seg_w, seg_h, tiled, compression, predictor, flags
    s.data = None if null == "data" else data.ctypes.data
    s.offsets = None if null == "offsets" else offs.ctypes.data
    out = (ctypes.c_uint64 * 4)()
    rc = pbx.lib().pbx_test_tiff_band_plan(None if null == "segs" else ctypes.byref(s), size_x, size_y, bpp,
                                           y0, rows, None if null == "out" else out)
    return rc, list(out), pbx.lib().pbx_last_error().decode()


STRIPS = dict(size_x=150, size_y=100, bpp=2, seg_w=150, seg_h=32, tiled=0)


def test_plan_covers_only_the_segment_rows_of_the_piece():
    # 150 x 100 uint16 in strips of 32 rows; rows [40, 70) lie in strips 1 and 2
    rc, out, _ = band_plan([b"\x80\0\1"] * 2, y0=40, rows=30, compression=5, **STRIPS)
    assert rc == 0 and out == [2, 19200, 2 * 9728, 0]
    # rows [90, 100): strip 2 and the short last strip of 4 rows
    rc, out, _ = band_plan([b"\x80\0\1"] * 2, y0=90, rows=10, compression=5, **STRIPS)
    assert rc == 0 and out == [2, 9600 + 1200, 9728 + 1280, 0]
    rc, out, _ = band_plan([b"\x80\0\1"] * 2, y0=90, rows=10, compression=5, predictor=2, **STRIPS)
    assert rc == 0 and out == [2, 9600 + 1200, 9728 + 1280, 1]
    # one band inside one strip
    rc, out, _ = band_plan([b"\x80\0\1"], y0=33, rows=7, compression=5, **STRIPS)
    assert rc == 0 and out == [1, 9600, 9728, 0]


@pytest.mark.parametrize("predictor", [1, 2])
def test_plan_stored_strips_need_no_decoder_and_no_scratch(predictor):
    rc, out, _ = band_plan([b"\0" * 9600] * 2, y0=40, rows=30, compression=1, predictor=predictor, **STRIPS)
    assert rc == 0 and out == [0, 19200, 0, predictor - 1]
    rc, out, _ = band_plan([b"\0" * 9600, b"\0" * 1200], y0=90, rows=10, compression=1, predictor=predictor,
                           **STRIPS)
    assert rc == 0 and out == [0, 9600 + 1200, 0, predictor - 1]


def test_plan_tile_rows_are_full_width_and_full_height():
    # 150 x 100 uint8 in 64 x 64 tiles: rows [60, 70) straddle both tile rows, 3 tiles each
    rc, out, _ = band_plan([b"x\x9c\3\0"] * 6, 150, 100, 1, 60, 10, 64, 64, 1, 8)
    assert rc == 0 and out == [6, 6 * 4096, 6 * 4096, 0]
    rc, out, _ = band_plan([b"x\x9c\3\0"] * 3, 150, 100, 1, 64, 36, 64, 64, 1, 8, predictor=2)
    assert rc == 0 and out == [3, 3 * 4096, 3 * 4096, 1]


@pytest.mark.parametrize("name,change,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_planner_refusals_on_a_two_strip_piece(name, change, msg):
    """Every refusal of pbx_test_tiff_plan, on the two strips that cover rows [40, 70)."""
    a = dict(segs=[b"\x80\0\1\2"] * 2, y0=40, rows=30, compression=5, **STRIPS)
    change = dict(change)
    if "offsets" in change:
        change["offsets"] = change["offsets"][:3]  # two segments: three offsets
    if "segs" in change:
        change["segs"] = change["segs"][:2]
    a.update(change)
    rc, _, err = band_plan(**a)
    assert rc == 400 and msg in err, (rc, err)


@pytest.mark.parametrize("y0,rows", [(0, 0), (40, 0), (-1, 10), (95, 6), (100, 1), (0, 101)])
def test_planner_refuses_rows_outside_the_plane(y0, rows):
    rc, _, err = band_plan([b"\x80\0\1"] * 4, y0=y0, rows=rows, compression=5, **STRIPS)
    assert rc == 400 and "outside the plane" in err, (rc, err)


# ----------------------------------------------------------------------- tiff_band_spec
def pieces(length):
    return [(0, length), (0, 1), (length - 1, 1), (0, 16), (16, 16), (40, 30), (31, 2), (90, length - 90),
            (64, 36), (33, 7)]


@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_band_spec_is_a_slice_of_the_plane_spec(entry):
    path = os.path.join(GOLD, entry["file"])
    n = 0
    for main in pbx.tiff_ifds(path)[:2]:
        for ifd in [main] + main["subifds"]:
            whole = pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0)
            wdata, woffs = whole["segments"]
            gx = -(-ifd["width"] // ifd["seg_w"]) if ifd["tiled"] else 1
            for y0, rows in pieces(ifd["length"]):
                if y0 < 0 or rows < 1 or y0 + rows > ifd["length"]:
                    continue
                sp = pbx.tiff_band_spec(path, ifd, y0, rows)
                for key in ("pixel_type", "size_x", "size_y", "big_endian", "seg_w", "seg_h", "tiled",
                            "compression", "predictor"):
                    assert sp[key] == whole[key], key
                assert (sp["y0"], sp["rows"]) == (y0, rows)
                k0, k1 = (y0 // ifd["seg_h"]) * gx, -(-(y0 + rows) // ifd["seg_h"]) * gx
                data, offs = sp["segments"]
                assert len(offs) == k1 - k0 + 1 and int(offs[0]) == 0
                assert int(offs[-1]) == sum(ifd["counts"][k0:k1])
                assert (offs == woffs[k0:k1 + 1] - woffs[k0]).all()
                assert data[:int(offs[-1])].tobytes() == wdata[int(woffs[k0]):int(woffs[k1])].tobytes()
                n += 1
    assert n >= 5


def test_band_spec_reads_only_the_covering_byte_ranges(monkeypatch):
    entry = next(e for e in FILES if e["file"] == "uint16_tiles_deflate_p2_MM.tif")
    path = os.path.join(GOLD, entry["file"])
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
    sr = 1 if ifd["length"] > ifd["seg_h"] else 0
    sp = pbx.tiff_band_spec(path, ifd, sr * ifd["seg_h"], 1)
    assert reads == list(zip(ifd["offsets"][sr * gx:(sr + 1) * gx], ifd["counts"][sr * gx:(sr + 1) * gx]))
    assert len(sp["segments"][1]) == gx + 1
    # rows == 0: the geometry and byte order alone, no segment is opened
    del reads[:]
    sp = pbx.tiff_band_spec(path, ifd, 0, 0)
    assert reads == [] and sp["segments"] is None
    assert sp["big_endian"] and sp["predictor"] == 2 and sp["tiled"] and sp["pixel_type"] == pbx.UINT16


def test_band_spec_refusals(tmp_path):
    import _tiff_src as T
    from test_tiff_src_host import PY_REFUSALS, write_with
    entry = FILES[0]
    path = os.path.join(GOLD, entry["file"])
    ifd = pbx.tiff_ifds(path)[0]
    for y0, rows in ((-1, 1), (0, -1), (ifd["length"], 1), (0, ifd["length"] + 1)):
        with pytest.raises(pbx.PbxError, match="outside the image") as e:
            pbx.tiff_band_spec(path, ifd, y0, rows)
        assert e.value.status == 400
    for name, change, extra, msg in PY_REFUSALS:  # the same 400s as tiff_plane_spec, rows == 0 included
        p = write_with(tmp_path, "r_%s.tif" % name.replace(" ", "_"), extra, **change)
        for rows in (0, 4):
            with pytest.raises(pbx.PbxError, match=re.escape(msg)) as e:
                pbx.tiff_band_spec(p, pbx.tiff_ifds(p)[0], 0, rows)
            assert e.value.status == 400
    # a segment count that does not match the grid
    a = (np.arange(40 * 30).reshape(30, 40) % 251).astype(np.uint8)
    p = str(tmp_path / "grid.tif")
    T.write_tiff(p, [T.page_of(a, 1, rows_per_strip=8)])
    short = dict(pbx.tiff_ifds(p)[0])
    short["offsets"], short["counts"] = short["offsets"][:-1], short["counts"][:-1]
    with pytest.raises(pbx.PbxError, match="3 segments for a grid of 1 x 4") as e:
        pbx.tiff_band_spec(p, short, 0, 8)
    assert e.value.status == 400


# ------------------------------------------------------------------------- the sources
def test_pixel_source_default_has_no_segment_access():
    assert pbx.PixelSource().band_segments(None, 0, 0, 0, 0, 0, 16) is None
    assert "tiff_band_spec" in pbx.PixelSource.band_segments.__doc__


def test_tiff_source_band_segments_on_a_stored_level():
    entry = next(e for e in FILES if e["file"].startswith("pyramid"))
    path = os.path.join(GOLD, entry["file"])
    src = pbx.TiffSource({9: path})
    px = src.get_pixels(9)
    assert px.levels == 3 and src.level_size(px, 2) == (38, 25)
    sub = pbx.tiff_ifds(path)[0]["subifds"][1]
    sp = src.band_segments(px, 0, 0, 0, 2, 16, 9)
    want = pbx.tiff_band_spec(path, sub, 16, 9)
    assert (sp["size_x"], sp["size_y"], sp["y0"], sp["rows"]) == (38, 25, 16, 9)
    assert sp["segments"][0].tobytes() == want["segments"][0].tobytes()
    assert (sp["segments"][1] == want["segments"][1]).all()
    assert sp["big_endian"] == (entry["byteorder"] == ">")
    assert src.band_segments(px, 0, 0, 0, 2, 0, 0)["segments"] is None
    with pytest.raises(pbx.PbxError, match="band_segments") as e:
        src.read_rows(px, 0, 0, 0, 0, 0, 16)
    assert e.value.status == 400
    assert "band_write_tiff" in pbx.TiffSource.__doc__ and "not implemented" not in pbx.TiffSource.__doc__
