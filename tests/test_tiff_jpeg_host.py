"""JPEG-compressed TIFF segments (Compression 7) without a GPU: tests/_tiff_jpeg.py's numpy model
against PIL (libjpeg-turbo + libtiff) byte for byte, the Python layer's layout, specs and refusals,
and the C-ABI's header parser and planner through pbx_test_tiff_jpeg_plan."""
import ctypes
import os

import numpy as np
import pytest

import _tiff_jpeg as J
import pbx

GOLD = J.GOLD
FILES = J.manifest()
IDS = [f["file"] for f in FILES]


def pages_of_file(path, ifd):
    """The model's planes (h, w, S) of one IFD of a file, from the bytes tiff_plane_spec reads."""
    S = ifd["spp"]
    out = np.zeros((ifd["length"], ifd["width"], S), np.uint8)
    for s in range(S if ifd["planar"] == 2 and S > 1 else 1):
        sp = pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, sample=s)
        data, offs = sp["segments"]
        gx = -(-sp["size_x"] // sp["seg_w"]) if sp["tiled"] else 1
        for k in range(len(offs) - 1):
            d = J.decode(bytes(data[int(offs[k]):int(offs[k + 1])]), sp["jpeg"]["tables"], ycbcr=sp["jpeg"]["ycbcr"])
            d = d.reshape(d.shape[0], d.shape[1], -1)
            x, y = (k % gx) * sp["seg_w"], (k // gx) * sp["seg_h"]
            d = d[:ifd["length"] - y, :ifd["width"] - x]
            if sp["samples_per_pixel"] == 1 and S > 1:
                out[y:y + d.shape[0], x:x + d.shape[1], s] = d[:, :, 0]
            else:
                out[y:y + d.shape[0], x:x + d.shape[1]] = d
    return out


# ------------------------------------------------------------------------------ model == PIL
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_model_equals_pil_on_fixtures(entry):
    path = os.path.join(GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    assert lay["samples"] == entry["samples"] and lay["levels"] == len(entry["planes"])
    for (z, c0, t), ifd in zip(lay["planes"], lay["ifds"]):
        for level, d in enumerate([ifd] + ifd["subifds"]):
            got = pages_of_file(path, d)
            for s in range(lay["samples"]):
                want = J.expected(entry, level, "%d,%d,%d" % (z, c0 + s, t))
                assert np.array_equal(got[:, :, s], want), (entry["file"], level, z, c0 + s, t)


def test_model_equals_pil_on_generated_streams():
    """...and asserts the [-512, 511] condition on every one of them (idct_islow)."""
    for name, w, h, s in J.generated_streams():
        assert np.array_equal(J.decode(s), J.pil_decode(s)), name
    hdr = J.header(J.generated_streams()[2][3])
    assert hdr["width"] == 32  # dc11
    with pytest.raises(AssertionError, match="leaves"):
        J.idct_islow(np.array([[4000] + [0] * 63], np.int64) * 8)


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_model_equals_pil_on_small_images(sub):
    """Every width 1 .. 18 and 33 against heights 1 .. 4, 8, 9, 17: partial MCUs, chroma planes of
    one or two samples (libjpeg replicates those), replicated edge rows."""
    rng = np.random.default_rng(sub)
    for w in list(range(1, 19)) + [33]:
        for h in (1, 2, 3, 4, 8, 9, 17):
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            for q in (30, 95):
                s = J.pil_jpeg(a, quality=q, subsampling=sub)
                assert np.array_equal(J.decode(s), J.pil_decode(s)), (w, h, q)


def test_model_equals_pil_on_gray_rgb_restarts_and_qualities():
    a = J.noise(50, 40, 3)
    for q in (30, 75, 95, 100):
        for img in (a, J.ramp(50, 40), J.checker(50, 40)):
            for kw in (dict(subsampling=2), dict(subsampling=0, restart_blocks=3), dict(keep_rgb=True),
                       dict(subsampling=1, restart_rows=1)):
                s = J.pil_jpeg(img, quality=q, **kw)
                assert np.array_equal(J.decode(s, ycbcr=not kw.get("keep_rgb")), J.pil_decode(s)), (q, kw)
            s = J.pil_jpeg(np.ascontiguousarray(img[:, :, 0]), quality=q, restart_blocks=1)
            assert np.array_equal(J.decode(s), J.pil_decode(s))


def test_model_equals_pil_through_the_container(tmp_path):
    """Hand-built TIFFs open in PIL to the pixels the model gives for their segments."""
    from PIL import Image
    a = J.noise(70, 50, 5) // 2 + J.ramp(70, 50) // 2
    for k, kw in enumerate((dict(tile=(32, 32), subsampling=2), dict(rows_per_strip=16, subsampling=1, tables="segment"),
                            dict(tile=(16, 16), subsampling=0, tables="both"), dict(rows_per_strip=8, photometric=2),
                            dict(tile=(16, 16), subsampling=2, restart_blocks=1))):
        pg = J.page_of(a, quality=80, **kw)
        p = str(tmp_path / ("t%d.tif" % k))
        J.write_tiff(p, [pg])
        assert np.array_equal(J.decode_page(pg), np.asarray(Image.open(p))), kw


# ------------------------------------------------------------------------------ layout and specs
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_layout_and_specs(entry):
    path = os.path.join(GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    ifd = lay["ifds"][0]
    assert (ifd["width"], ifd["length"], ifd["compression"], ifd["tiled"]) == (entry["width"], entry["length"], 7,
                                                                               entry["tiled"])
    assert lay["pixel_type"] == pbx.UINT8 and ifd["byteorder"] == entry["byteorder"] and ifd["bigtiff"] == entry["bigtiff"]
    if "ome" in entry:
        assert (lay["size_z"], lay["size_c"], lay["size_t"]) == (2, 3, 1)
    sp = pbx.tiff_plane_spec(path, ifd, 9, 0, 0, 0)
    assert sp["compression"] == pbx.TIFF_JPEG and sp["predictor"] == 1 and sp["pixel_type"] == pbx.UINT8
    if entry.get("pil"):
        assert ifd["photometric"] == 2 and sp["jpeg"]["ycbcr"] is False and sp["jpeg"]["tables"][:2] == b"\xff\xd8"
        return
    assert sp["jpeg"]["ycbcr"] is entry["ycbcr"]
    assert (sp["jpeg"]["tables"] is None) == (entry.get("tables") == "segment")
    assert sp["samples_per_pixel"] == (1 if entry.get("planar") == 2 else entry["samples"])
    if entry["ycbcr"]:
        assert ifd["photometric"] == 6 and ifd["ycbcr_subsampling"] == entry["sampling"]
    # a band reads exactly the byte ranges of the segment rows that cover it
    seg_h, h = ifd["seg_h"], ifd["length"]
    gx = -(-ifd["width"] // ifd["seg_w"]) if ifd["tiled"] else 1
    y0, rows = seg_h + 3, min(seg_h, h - seg_h - 3)
    band = pbx.tiff_band_spec(path, ifd, y0, rows)
    k0, k1 = (y0 // seg_h) * gx, -(-(y0 + rows) // seg_h) * gx
    with open(path, "rb") as f:
        raw = f.read()
    want = b"".join(raw[o:o + n] for o, n in zip(ifd["offsets"][k0:k1], ifd["counts"][k0:k1]))
    assert bytes(band["segments"][0][:int(band["segments"][1][-1])]) == want and band["jpeg"] == sp["jpeg"]
    assert pbx.tiff_band_spec(path, ifd, 0, 0)["segments"] is None


# ------------------------------------------------------------------------------ the planner
def plan(page, y0=0, rows=0, spp=None, tables="page", ycbcr=None, segs=None, **seg_kw):
    """pbx_test_tiff_jpeg_plan on a page_of() page: (status, message, out[6])."""
    segs = page["segments"] if segs is None else segs
    data, offs = pbx.pack_chunks(segs)
    if len(data) == 0 or not any(len(s) for s in segs):
        data = np.zeros(1, np.uint8)
    tile = page["tile"]
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h = (tile if tile else (page["width"], min(page["rows_per_strip"], page["length"])))
    s.tiled, s.compression, s.predictor, s.flags = 1 if tile else 0, 7, 1, 0
    for k, v in seg_kw.items():
        setattr(s, k, v)
    # the segments in a buffer of exactly their bytes
    buf = (ctypes.c_uint8 * max(1, int(offs[-1]))).from_buffer_copy(bytes(data[:max(1, int(offs[-1]))]))
    s.data, s.offsets = ctypes.addressof(buf), offs.ctypes.data
    if tables == "page":
        tables = next((bytes(t[2]) for t in page["extra"] if t[0] == 347), None)
    j = pbx.PbxTiffJpeg()
    keep = pbx._fill_tiff_jpeg(j, dict(tables=tables, ycbcr=page["photometric"] == 6 if ycbcr is None else ycbcr))
    out = (ctypes.c_uint64 * 6)()
    rc = pbx.lib().pbx_test_tiff_jpeg_plan(ctypes.byref(s), ctypes.byref(j), page["width"], page["length"],
                                           page["spp"] if spp is None else spp, y0, rows, out)
    del keep
    return rc, pbx.lib().pbx_last_error().decode(), list(out)


def test_planner_counts_and_table_sets():
    a = J.noise(100, 70, 1)
    pg = J.page_of(a, tile=(32, 32), subsampling=2, quality=75)
    rc, msg, out = plan(pg)
    assert rc == 0, msg
    # 4 x 3 tiles; 3 components of 32 x 32 samples each; Y 32 x 32 + 2 x (16 x 16) in scratch per
    # tile (each plane a multiple of 256 bytes already); one table set for all of them; h2v2
    assert out[:5] == [12, 12 * 3 * 32 * 32, 12 * (1024 + 2 * 256), 1, 3]
    assert out[5] == sum(len(s) - J.header(s)["data"] for s in pg["segments"])
    rc, msg, out = plan(pg, y0=40, rows=20, segs=pg["segments"][4:8])  # tile row 1 only
    assert rc == 0 and out[0] == 4, msg
    # every tile with tables of its own quality: as many sets as there are distinct tables
    segs = [J.pil_jpeg(np.ascontiguousarray(p), quality=50 + 10 * (k % 3), subsampling=2)
            for k, p in enumerate(J._pieces(a, (32, 32), None))]
    rc, msg, out = plan(dict(pg, segments=segs), tables=None)
    assert rc == 0 and out[3] == 3, (msg, out)
    # strips: 4:2:2 rows of MCUs 16 x 8, the last strip short; gray; RGB kept as it is
    pg = J.page_of(a, rows_per_strip=16, subsampling=1, quality=75)
    rc, msg, out = plan(pg)
    assert rc == 0 and out[0] == 5 and out[4] == 2, msg
    # Y pitch 7 MCUs x 16 = 112, chroma 56 -> 64; the last strip's 6 rows are one MCU row of 8, its Y
    # plane of 896 bytes rounded up to 1024
    assert out[2] == 4 * (112 * 16 + 2 * 64 * 16) + (1024 + 2 * 64 * 8)
    rc, msg, out = plan(J.page_of(a[:, :, 0].copy(), rows_per_strip=16))
    assert rc == 0 and out[4] == 0 and out[1] == 100 * 70, msg
    rc, msg, out = plan(J.page_of(a, rows_per_strip=16, photometric=2))
    assert rc == 0 and out[4] == 0 and out[1] == 3 * 100 * 70, msg
    rc, msg, out = plan(J.page_of(a, tile=(16, 16), subsampling=0, tables="both"))
    assert rc == 0 and out[4] == 1 and out[3] == 1, msg


def _set(stream, code, payload_edit):
    """The stream with the payload of its first marker segment `code` edited in place."""
    b = bytearray(stream)
    for c, o, n in J.segments(stream):
        if c == code:
            payload_edit(b, o, n)
            return bytes(b)
    raise AssertionError("no marker %02x" % code)


def _sof(stream, new_code):
    b = bytearray(stream)
    for c, o, n in J.segments(stream):
        if c == 0xC0:
            b[o - 3] = new_code
    return bytes(b)


def c_refusals():
    a = J.noise(16, 16, 2)
    good = J.pil_jpeg(a, quality=80, subsampling=2)
    gray = J.pil_jpeg(a[:, :, 0].copy(), quality=80)

    def poke(at, v):
        def f(b, o, n):
            b[o + at] = v
        return f
    hdr_end = J.header(good)["data"]
    dht = [(c, o, n) for c, o, n in J.segments(good) if c == 0xC4][0]
    no_dht = good[:dht[1] - 4] + good[dht[1] + dht[2]:]
    sos = [(c, o, n) for c, o, n in J.segments(good) if c == 0xDA][0]
    two_scans = good[:sos[1] - 4] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + good[hdr_end:]
    return [
        ("SOF1", _sof(good, 0xC1), "SOF1 (extended sequential) is not supported"),
        ("SOF2", _sof(good, 0xC2), "SOF2 (progressive) is not supported"),
        ("SOF3", _sof(good, 0xC3), "SOF3 (lossless) is not supported"),
        ("arithmetic", _sof(good, 0xC9), "SOF9 (arithmetic coding) is not supported"),
        ("precision", _set(good, 0xC0, poke(0, 12)), "sample precision 12"),
        ("4 components", _set(good, 0xC0, poke(5, 4)), "4 components"),
        ("sampling 4x1", _set(good, 0xC0, poke(7, 0x41)), "sampling factors 4x1, 1x1, 1x1"),
        ("chroma 2x1", _set(good, 0xC0, poke(10, 0x21)), "sampling factors 2x2, 2x1, 1x1"),
        ("SOF size", _set(good, 0xC0, poke(2, 17)), "SOF size 16 x 17 != segment size 16 x 16"),
        ("two scans", two_scans, "more than one scan"),
        ("no Huffman table", no_dht, "missing Huffman table"),
        ("oversubscribed", _set(good, 0xC4, poke(1, 3)), "over-subscribed Huffman table"),
        ("no quantiser", _set(good, 0xC0, poke(8, 3)), "missing quantiser 3"),
        ("16-bit quantiser", _set(good, 0xDB, poke(0, 0x10)), "16-bit quantiser"),
        ("no SOI", b"\x00" + good[1:], "segment 0 does not start with SOI"),
        ("gray in three samples", gray, "a stream of 1 components in segments of 3 samples per pixel"),
    ]


@pytest.mark.parametrize("case", c_refusals(), ids=lambda c: c[0])
def test_c_abi_refusals(case):
    name, stream, msg = case
    pg = J.stream_page(16, 16, stream, photometric=6, spp=3)
    rc, err, _ = plan(pg)
    assert rc == 400 and msg in err, err


def test_c_abi_refusals_of_the_arguments():
    a = J.noise(16, 16, 2)
    good = J.pil_jpeg(a, quality=80, subsampling=2)
    pg = J.stream_page(16, 16, good)
    for kw, msg in ((dict(compression=8), "bad compression 8 (the JPEG calls take 7)"),
                    (dict(predictor=2), "bad predictor 2 on JPEG segments"), (dict(flags=1), "bad flags 0x1")):
        rc, err, _ = plan(pg, **kw)
        assert rc == 400 and msg in err, err
    rc, err, _ = plan(pg, ycbcr=False)
    assert rc == 400 and "subsampling 2x2 without PhotometricInterpretation 6" in err, err
    rc, err, _ = plan(pg, spp=4)
    assert rc == 400 and "JPEG segments of 4 samples per pixel" in err, err
    rc, err, _ = plan(J.stream_page(16, 16, J.pil_jpeg(a[:, :, 0].copy())), spp=1, ycbcr=True)
    assert rc == 400 and "YCbCr (PhotometricInterpretation 6) with 1 samples per pixel" in err, err
    rc, err, _ = plan(pg, tables=b"\xff\xd9")
    assert rc == 400 and "JPEGTables does not start with SOI" in err, err
    # the other TIFF calls keep refusing compression 7
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.compression, s.predictor = 16, 16, 7, 1
    data, offs = pbx.pack_chunks([good])
    s.data, s.offsets = data.ctypes.data, offs.ctypes.data
    out = (ctypes.c_uint64 * 4)()
    assert pbx.lib().pbx_test_tiff_plan(ctypes.byref(s), 16, 16, 1, out) == 400
    assert b"bad compression 7 (1 none, 5 LZW, 8 deflate, 50000 zstd)" in pbx.lib().pbx_last_error()


def test_every_prefix_of_a_header_is_refused():
    """A segment or a tables stream cut anywhere before its end of header: 400, and (the buffer is
    exactly the prefix's bytes) nothing past it is read."""
    a = J.noise(16, 16, 4)
    good = J.pil_jpeg(a, quality=80, subsampling=2, restart_blocks=1)
    end = J.header(good)["data"]
    pg = J.stream_page(16, 16, good)
    assert plan(pg)[0] == 0
    for cut in range(end):
        rc, err, _ = plan(pg, segs=[good[:cut]])
        assert rc == 400, (cut, err)
    tabs, rest = J.split_tables(good)
    assert plan(pg, segs=[rest], tables=tabs)[0] == 0
    for cut in range(len(tabs)):
        rc, err, _ = plan(pg, segs=[rest], tables=tabs[:cut] or None)
        if cut == 0:
            assert rc == 400 and "missing" in err, err  # no tables at all
        else:
            assert rc == 400 and "JPEGTables" in err, (cut, err)


# ------------------------------------------------------------------------------ Python refusals
def py_refusals():
    out = [(n, s, m) for n, s, m in c_refusals() if n not in ("no Huffman table", "oversubscribed", "no quantiser",
                                                              "gray in three samples")]
    return out


@pytest.mark.parametrize("case", py_refusals(), ids=lambda c: c[0])
def test_python_refusals_from_the_first_segment(tmp_path, case):
    name, stream, msg = case
    pg = J.stream_page(16, 16, stream, photometric=6, spp=3)
    p = str(tmp_path / "bad.tif")
    J.write_tiff(p, [pg])
    for call in (lambda: pbx.tiff_image_layout(p), lambda: pbx.tiff_plane_spec(p, pbx.tiff_ifds(p)[0], 1, 0, 0, 0)):
        with pytest.raises(pbx.PbxError, match="Compression 7") as e:
            call()
        assert e.value.status == 400 and msg in str(e.value), str(e.value)


def test_python_refusals_from_the_ifd(tmp_path):
    a = J.noise(16, 16, 6)
    good = J.page_of(a, rows_per_strip=16, subsampling=0, quality=80)

    def refused(page, msg, **kw):
        p = str(tmp_path / "r.tif")
        J.write_tiff(p, [page], **kw)
        with pytest.raises(pbx.PbxError, match=msg) as e:
            pbx.tiff_image_layout(p)
        assert e.value.status == 400

    gray = J.page_of(a[:, :, 0].copy(), rows_per_strip=16)
    refused(dict(gray, compression=6), r"Compression 6 \(1 none, 5 LZW, 8 / 32946 deflate, 50000 zstd\)")  # old-style JPEG
    refused(dict(good, predictor=2), "Predictor 2 with Compression 7")
    refused(dict(good, compression=8), "PhotometricInterpretation 6 with SamplesPerPixel 3")
    refused(dict(good, bits=16), "Compression 7 .1 none")
    planar = J.page_of(a, rows_per_strip=16, planar=2, photometric=2)
    refused(dict(planar, photometric=6), "PhotometricInterpretation 6 .YCbCr. with PlanarConfiguration 2")
    sub = J.page_of(a, rows_per_strip=16, subsampling=2)
    refused(dict(sub, photometric=2), "subsampling 2x2 without PhotometricInterpretation 6")
    cmyk = dict(good, spp=4, photometric=5, extrasamples=[])
    refused(cmyk, "PhotometricInterpretation 5 with SamplesPerPixel 4")
    refused(dict(good, spp=4, photometric=2, extrasamples=[0]), "Compression 7 with SamplesPerPixel 4")
    tabs_bad = dict(good, extra=[t if t[0] != 347 else (347, 1, [0, 1, 2]) for t in good["extra"]])
    refused(tabs_bad, "Compression 7: JPEGTables does not start with SOI")


def test_exports_and_abi():
    assert ctypes.sizeof(pbx.PbxTiffJpeg) == 24 and ctypes.sizeof(pbx.PbxTiffSegments) == 40
    for name in ("pbx_planes_register_tiff_jpeg", "pbx_band_write_tiff_jpeg", "pbx_test_tiff_jpeg_plan"):
        assert name in pbx.EXPORTS and hasattr(pbx.lib(), name)
    assert pbx.TIFF_JPEG == 7
