"""Lossless JPEG 2000 TIFF segments (Compression 33003 / 33004 / 33005 / 34712) without a GPU:
tests/_tiff_j2k.py's model against PIL (OpenJPEG) and against the encoder's input, bit for bit; the
Python layer's layout, specs and refusals; the C-ABI's header parser and planner through
pbx_test_tiff_j2k_plan; and the device's own serial code (packet headers, MQ and bit-plane decoder)
run on the CPU through pbx_test_tiff_j2k_decode."""
import ctypes
import os
import struct

import numpy as np
import pytest

import _tiff_j2k as J
import pbx

GOLD = J.GOLD
FILES = J.manifest()
IDS = [f["file"] for f in FILES]
PROGRESSIONS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]


def noise(w, h, seed, dtype=np.uint8, samples=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, (h, w) if samples == 1 else (h, w, samples), dtype=dtype)


def segments_struct(segs, seg_w, seg_h, tiled, compression=pbx.TIFF_J2K, predictor=1):
    data, offs = segs if isinstance(segs, tuple) else pbx.pack_chunks(segs)
    if len(data) == 0:
        data = np.zeros(1, np.uint8)
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor, s.flags = seg_w, seg_h, 1 if tiled else 0, compression, predictor, 0
    s.data, s.offsets = data.ctypes.data, offs.ctypes.data
    return s, (data, offs)


def plan(segs, w, h, seg_w, seg_h, tiled, pixel_type, spp, y0=0, rows=0, **kw):
    """pbx_test_tiff_j2k_plan: (status, message, [streams, code blocks, packets, scratch bytes])."""
    s, keep = segments_struct(segs, seg_w, seg_h, tiled, **kw)
    out = (ctypes.c_uint64 * 4)()
    rc = pbx.lib().pbx_test_tiff_j2k_plan(ctypes.byref(s), w, h, pixel_type, spp, y0, rows, out)
    return rc, pbx.lib().pbx_last_error().decode() if rc else "", list(out)


def cpu_decode(segs, w, h, seg_w, seg_h, tiled, dtype, spp):
    """pbx_test_tiff_j2k_decode: (status, message, (spp, h, w) array)."""
    s, keep = segments_struct(segs, seg_w, seg_h, tiled)
    out = np.zeros((spp, h, w), dtype)
    rc = pbx.lib().pbx_test_tiff_j2k_decode(ctypes.byref(s), w, h, pbx.UINT8 if dtype == np.uint8 else pbx.UINT16, spp,
                                            out.ctypes.data, out.nbytes)
    return rc, pbx.lib().pbx_last_error().decode() if rc else "", out


def one(stream, a):
    """One stream as the single strip of a plane of a's shape."""
    h, w = a.shape[:2]
    return [stream], w, h, w, h, False


def planes(a):
    return a[None] if a.ndim == 2 else np.moveaxis(a, 2, 0)


def check(a, **kw):
    """model == PIL == the array == the device's serial code on the CPU, and the planner's counts."""
    s = J.encode(a, **kw)
    assert np.array_equal(J.pil_decode(s), a), kw
    assert np.array_equal(J.decode(s), a), (a.shape, kw)
    spp = 1 if a.ndim == 2 else 3
    rc, msg, got = cpu_decode(*one(s, a), a.dtype.type, spp)
    assert rc == 0 and np.array_equal(got, planes(a)), (a.shape, kw, msg)
    rc, msg, out = plan(*one(s, a), pbx.UINT8 if a.dtype == np.uint8 else pbx.UINT16, spp)
    assert rc == 0 and out == [1] + list(J.counts(s)), (out, J.counts(s), msg)
    return s


# ------------------------------------------------------------------------------ model == PIL
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_model_equals_pil_on_fixtures(entry):
    path = os.path.join(GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    assert lay["samples"] == entry["samples"] and lay["levels"] == len(entry["planes"])
    for (z, c0, t), ifd in zip(lay["planes"], lay["ifds"]):
        for level, d in enumerate([ifd] + ifd["subifds"]):
            S = d["spp"]
            for s in range(S if d["planar"] == 2 and S > 1 else 1):
                sp = pbx.tiff_plane_spec(path, d, 1, 0, 0, 0, sample=s)
                data, offs = sp["segments"]
                gx = -(-sp["size_x"] // sp["seg_w"]) if sp["tiled"] else 1
                dt = np.uint8 if sp["pixel_type"] == pbx.UINT8 else np.uint16
                got = np.zeros((sp["samples_per_pixel"], d["length"], d["width"]), dt)
                for k in range(len(offs) - 1):
                    seg = bytes(data[int(offs[k]):int(offs[k + 1])])
                    m = J.decode(seg)
                    assert np.array_equal(m, J.pil_decode(seg))
                    x, y = (k % gx) * sp["seg_w"], (k // gx) * sp["seg_h"]
                    m = planes(m)[:, :d["length"] - y, :d["width"] - x]
                    got[:, y:y + m.shape[1], x:x + m.shape[2]] = m
                rc, msg, cpu = cpu_decode((data, offs), d["width"], d["length"], sp["seg_w"], sp["seg_h"], sp["tiled"], dt,
                                          sp["samples_per_pixel"])
                assert rc == 0 and np.array_equal(cpu, got), msg
                for q in range(sp["samples_per_pixel"]):
                    want = J.expected(entry, level, "%d,%d,%d" % (z, c0 + s + q, t))
                    assert np.array_equal(got[q], want), (entry["file"], level, z, c0 + s + q, t)


@pytest.mark.parametrize("kind", ["u8", "u16", "rgb", "rct"])
def test_small_images(kind):
    """Widths 1 .. 18 x heights 1 .. 17: empty sub-bands, resolutions of one row or column.  Code
    blocks, levels and progressions rotate over the sizes."""
    blocks = [(4, 4), (32, 32), (64, 64), (1024, 4)]
    n = 0
    for w in range(1, 19):
        for h in range(1, 18):
            n += 1
            if kind in ("u8", "u16"):
                a = noise(w, h, n, np.uint8 if kind == "u8" else np.uint16)
                kw = {}
            else:
                a = noise(w, h, n, samples=3)
                kw = dict(mct=1 if kind == "rct" else 0)
            check(a, codeblock_size=blocks[n % 4], num_resolutions=1 + n % 6, progression=PROGRESSIONS[n % 5], **kw)


def test_levels_blocks_progressions_and_precincts():
    a16, rgb = noise(50, 40, 3, np.uint16), noise(50, 40, 4, samples=3)
    for levels in range(6):
        for cb in ((4, 4), (32, 32), (64, 64), (1024, 4)):
            check(a16, num_resolutions=levels + 1, codeblock_size=cb)
    for prog in PROGRESSIONS:
        for mct in (0, 1):
            check(rgb, progression=prog, mct=mct, num_resolutions=4, codeblock_size=(16, 16))
        s = check(a16, progression=prog, num_resolutions=4, precinct_size=(64, 64), codeblock_size=(16, 16))
        assert J.parse(s)["scod"] & 1 and J.parse(s)["prog"] == PROGRESSIONS.index(prog)


def test_extreme_images():
    y, x = np.mgrid[0:48, 0:48]
    check(np.zeros((48, 48), np.uint16), num_resolutions=4)
    # the level shift makes 32768 the image whose coefficients are all zero: no block is included
    mid = check(np.full((48, 48), 32768, np.uint16), num_resolutions=4)
    hd = J.parse(mid)
    assert not any(band for comp in J.packets(mid, hd, J.geometry(hd)[0]) for band in comp), "a block is included"
    check(np.full((48, 48), 65535, np.uint16), num_resolutions=4)
    check((((x + y) & 1) * 65535).astype(np.uint16), num_resolutions=4)
    check((((x + y) & 1) * 65535).astype(np.uint16), num_resolutions=1)
    check(np.full((48, 48, 3), 255, np.uint8), num_resolutions=3, mct=1)


def test_one_tile_of_256():
    rng = np.random.default_rng(5)
    a = rng.poisson(60, (256, 256)).astype(np.uint16)
    s = J.encode(a, num_resolutions=6, codeblock_size=(64, 64))
    rc, msg, got = cpu_decode(*one(s, a), np.uint16, 1)
    assert rc == 0 and np.array_equal(got[0], a), msg


# ------------------------------------------------------------------------------ layout and specs
@pytest.mark.parametrize("entry", FILES, ids=IDS)
def test_fixture_layout_and_specs(entry):
    path = os.path.join(GOLD, entry["file"])
    lay = pbx.tiff_image_layout(path)
    ifd = lay["ifds"][0]
    assert (ifd["width"], ifd["length"], ifd["compression"], ifd["tiled"]) == (entry["width"], entry["length"],
                                                                               entry["compression"], entry["tiled"])
    assert entry["compression"] in J.J2K_COMPRESSIONS
    assert lay["pixel_type"] == (pbx.UINT8 if entry["bits"] == 8 else pbx.UINT16)
    assert ifd["byteorder"] == entry["byteorder"] and ifd["bigtiff"] == entry["bigtiff"]
    if entry["file"].endswith(".ome.tif"):
        assert (lay["size_z"], lay["size_c"], lay["size_t"]) == (2, 1, 1)
    sp = pbx.tiff_plane_spec(path, ifd, 9, 0, 0, 0)
    assert sp["compression"] == pbx.TIFF_J2K and sp["j2k"] is True and sp["predictor"] == 1 and "jpeg" not in sp
    assert sp["samples_per_pixel"] == (1 if entry.get("planar") == 2 else entry["samples"])
    assert sp["big_endian"] == (entry["byteorder"] == ">")
    # a band reads exactly the byte ranges of the segment rows that cover it
    seg_h, h = ifd["seg_h"], ifd["length"]
    gx = -(-ifd["width"] // ifd["seg_w"]) if ifd["tiled"] else 1
    y0, rows = seg_h + 3, min(seg_h, h - seg_h - 3)
    band = pbx.tiff_band_spec(path, ifd, y0, rows)
    k0, k1 = (y0 // seg_h) * gx, -(-(y0 + rows) // seg_h) * gx
    with open(path, "rb") as f:
        raw = f.read()
    want = b"".join(raw[o:o + n] for o, n in zip(ifd["offsets"][k0:k1], ifd["counts"][k0:k1]))
    assert bytes(band["segments"][0][:int(band["segments"][1][-1])]) == want and band["j2k"] is True
    assert pbx.tiff_band_spec(path, ifd, 0, 0)["segments"] is None
    # the planner on the band's segment rows and on the whole plane
    spp = sp["samples_per_pixel"]
    rc, msg, out = plan(band["segments"], ifd["width"], h, ifd["seg_w"], seg_h, ifd["tiled"], sp["pixel_type"], spp, y0, rows)
    assert rc == 0 and out[0] == k1 - k0, msg
    data, offs = sp["segments"]
    segs = [bytes(data[int(offs[k]):int(offs[k + 1])]) for k in range(len(offs) - 1)]
    rc, msg, out = plan(sp["segments"], ifd["width"], h, ifd["seg_w"], seg_h, ifd["tiled"], sp["pixel_type"], spp)
    assert rc == 0 and out == [len(segs)] + [sum(v) for v in zip(*[J.counts(s) for s in segs])], msg


def test_header_reader():
    s = J.encode(noise(40, 30, 6, samples=3), mct=1, num_resolutions=4, progression="RPCL", codeblock_size=(32, 16))
    h = pbx.j2k_header(s, "x")
    assert (h["width"], h["height"], h["components"]) == (40, 30, [(8, 0, 1, 1)] * 3)
    assert (h["mct"], h["levels"], h["progression"], h["xcb"], h["ycb"], h["layers"]) == (1, 3, 2, 5, 4, 1)
    assert (h["transformation"], h["qstyle"], len(h["exponents"]), h["style"], h["scod"]) == (1, 0, 10, 0, 0)
    assert h["markers"][:3] == [0x51, 0x52, 0x5C] and h["markers"][-1] == 0x90 and s[h["data"] - 2:h["data"]] == b"\xff\x93"


# ------------------------------------------------------------------------------ refusals
W0, H0 = 40, 24
GOOD = J.encode(noise(W0, H0, 7, np.uint16), num_resolutions=3)
RGB = J.encode(noise(W0, H0, 8, samples=3), num_resolutions=3, mct=1)


def insert_before(data, code, segment):
    q = J.find_marker(data, code)
    return data[:q] + segment + data[q:]


def second_tile_part(data):
    """Psot set to end where EOC stood, and an SOT there."""
    q = J.find_marker(data, 0x90)
    end = len(data) - 2
    assert data[end:] == b"\xff\xd9"
    return data[:q + 6] + struct.pack(">I", end - q) + data[q + 10:end] + b"\xff\x90\x00\x0a" + bytes(8) + b"\xff\x93\xff\xd9"


def siz_field(data, at, value):
    q = J.find_marker(data, 0x51) + 4 + at
    return data[:q] + struct.pack(">I", value) + data[q + 4:]


REFUSALS = [
    ("irreversible", J.patch(GOOD, 0x52, 9, 0), "irreversible wavelet"),
    ("quantised", J.patch(GOOD, 0x5C, 0, 0x42), "quantisation style 2"),
    ("derived", J.patch(GOOD, 0x5C, 0, 0x41), "quantisation style 1"),
    ("layers", J.patch(GOOD, 0x52, 3, 2), "2 quality layers"),
    ("bypass", J.patch(GOOD, 0x52, 8, 0x01), "code-block style 0x01"),
    ("termall", J.patch(GOOD, 0x52, 8, 0x04), "code-block style 0x04"),
    ("segmentation", J.patch(GOOD, 0x52, 8, 0x20), "code-block style 0x20"),
    ("sop", J.patch(GOOD, 0x52, 0, 0x02), "SOP or EPH markers"),
    ("eph", J.patch(GOOD, 0x52, 0, 0x04), "SOP or EPH markers"),
    ("signed", J.patch(GOOD, 0x51, 36, 0x8F), "signed components"),
    ("precision 12", J.patch(GOOD, 0x51, 36, 11), "precision 12 (8 or 16)"),
    ("rgb16", J.patch(J.patch(J.patch(RGB, 0x51, 36, 15), 0x51, 39, 15), 0x51, 42, 15), "three components at precision 16"),
    ("subsampled", J.patch(RGB, 0x51, 40, 2), "subsampled components"),
    ("xosiz", siz_field(GOOD, 10, 1), "non-zero image or tile offsets"),
    ("tiles", siz_field(GOOD, 18, 16), "more than one tile"),
    ("coc", insert_before(GOOD, 0x5C, b"\xff\x53\x00\x09" + bytes(7)), "COC markers are not supported"),
    ("poc", insert_before(GOOD, 0x5C, b"\xff\x5f\x00\x09" + bytes(7)), "POC markers are not supported"),
    ("rgn", insert_before(GOOD, 0x90, b"\xff\x5e\x00\x05" + bytes(3)), "RGN markers are not supported"),
    ("second SOT", second_tile_part(GOOD), "more than one tile-part"),
    ("tile-part 1", J.patch(GOOD, 0x90, 6, 1), "more than one tile-part"),
    ("jp2", b"\x00\x00\x00\x0cjP  \r\n\x87\n" + GOOD, "jp2 box, not a codestream"),
    ("no SOC", b"\xff\xd8" + GOOD[2:], "does not start with SOC"),
    ("levels", J.patch(GOOD, 0x52, 5, 3), "QCD of 7 sub-bands for 3 decomposition levels"),
    ("block size", J.patch(GOOD, 0x52, 6, 9), "bad code-block size"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0])
def test_refusals_of_both_layers(case, tmp_path):
    name, stream, text = case
    spp = 3 if stream[2:].startswith(RGB[2:8]) and name in ("rgb16", "subsampled") else 1
    pt = pbx.UINT8 if spp == 3 else pbx.UINT16
    rc, msg, _ = plan([stream], W0, H0, W0, H0, False, pt, spp)
    assert rc == 400 and text in msg and "segment 0" in msg, msg
    rc, msg, _ = cpu_decode([stream], W0, H0, W0, H0, False, np.uint8 if spp == 3 else np.uint16, spp)
    assert rc == 400 and text in msg
    pg = dict(width=W0, length=H0, bits=8 if spp == 3 else 16, spp=spp, compression=33003, photometric=2 if spp == 3 else 1,
              planar=1, tile=None, rows_per_strip=H0, segments=[stream], subifds=[], description=None)
    path = str(tmp_path / "r.tif")
    J.write_tiff(path, [pg])
    with pytest.raises(pbx.PbxError, match="Compression 33003: segment 0") as e:
        pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0)
    assert e.value.status == 400 and text in str(e.value), str(e.value)
    with pytest.raises(pbx.PbxError) as e:
        pbx.tiff_band_spec(path, pbx.tiff_ifds(path)[0], 0, 0)
    assert text in str(e.value)


def test_refusals_that_need_the_segment_or_the_plane(tmp_path):
    a = noise(W0, H0, 9, np.uint16)
    s = J.encode(a, num_resolutions=3)
    assert "SIZ size 40 x 24 != segment size 40 x 16" in plan([s, s], W0, 32, W0, 16, False, pbx.UINT16, 1)[1]
    assert "SIZ size 40 x 24 != segment size 48 x 32" in plan([s], 48, 32, 48, 32, True, pbx.UINT16, 1)[1]
    assert "precision 16 on a plane of 8-bit samples" in plan([s], W0, H0, W0, H0, False, pbx.UINT8, 1)[1]
    assert "a stream of 1 components in segments of 3 samples per pixel" in plan([s], W0, H0, W0, H0, False, pbx.UINT16, 3)[1]
    assert "bad predictor 2 on JPEG 2000 segments" in plan([s], W0, H0, W0, H0, False, pbx.UINT16, 1, predictor=2)[1]
    assert "bad compression 8 (the JPEG 2000 calls take 34712)" in plan([s], W0, H0, W0, H0, False, pbx.UINT16, 1,
                                                                        compression=8)[1]
    assert "neither uint8 nor uint16" in plan([s], W0, H0, W0, H0, False, pbx.INT16, 1)[1]
    assert "2 samples per pixel" in plan([s], W0, H0, W0, H0, False, pbx.UINT16, 2)[1]
    assert "segment 0 is empty" in plan([b""], W0, H0, W0, H0, False, pbx.UINT16, 1)[1]
    # more than one precinct in a resolution: 16 x 16 precincts on 40 x 24 (PIL declares them only above the block size)
    many = J.encode(a, num_resolutions=3, precinct_size=(16, 16), codeblock_size=(8, 8))
    assert "more than one precinct in resolution" in plan([many], W0, H0, W0, H0, False, pbx.UINT16, 1)[1]
    # the IFD's own refusals
    pg = J.page_of(a, 34712, num_resolutions=3)
    path = str(tmp_path / "p.tif")
    for patch, text in ((dict(photometric=6), "PhotometricInterpretation 6 with Compression 34712"),
                        (dict(bits=32), "neither uint8 nor uint16"),
                        (dict(bits=8), "precision 16 on a plane of 8-bit samples"),
                        (dict(segments=[many]), "more than one precinct in resolution")):
        J.write_tiff(path, [dict(pg, **patch)])
        with pytest.raises(pbx.PbxError) as e:
            pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0)
        assert e.value.status == 400 and text in str(e.value), str(e.value)
    ifd = dict(pbx.tiff_ifds(path)[0], predictor=2)
    with pytest.raises(pbx.PbxError, match="Predictor 2 with Compression 34712"):
        pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0)


def test_every_prefix_of_a_header_is_a_400(tmp_path):
    for good in (GOOD, J.encode(noise(W0, H0, 10, samples=3), mct=1, num_resolutions=4, precinct_size=(64, 64))):
        end = J.parse(good)["data"]
        for cut in range(end):
            rc, msg, _ = plan([good[:cut]] if cut else [b"\x00"], W0, H0, W0, H0, False, pbx.UINT16, 1)
            assert rc == 400, (cut, msg)
            with pytest.raises(pbx.PbxError) as e:
                pbx.j2k_header(good[:cut], "segment 0")
            assert e.value.status == 400
    # the whole header with nothing after it: the device's to say (no packet can be read)
    rc, msg, _ = plan([GOOD[:J.parse(GOOD)["data"]]], W0, H0, W0, H0, False, pbx.UINT16, 1)
    assert rc == 0
    rc, msg, _ = cpu_decode([GOOD[:J.parse(GOOD)["data"]]], W0, H0, W0, H0, False, np.uint16, 1)
    assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code 1)" in msg


def test_device_codes_on_the_cpu():
    """The serial code's refusals, through the CPU hook: the cases of tests/test_gpu_tiff_j2k.py."""
    hd = J.parse(GOOD)
    found = J.packets(GOOD, hd, J.geometry(hd)[0])
    last = max(v[0] + v[1] for comp in found for band in comp for v in band.values())
    for stream, code in ((GOOD[:hd["data"] + 1], 1), (GOOD[:last - 5], 1)):
        rc, msg, _ = cpu_decode([stream], W0, H0, W0, H0, False, np.uint16, 1)
        assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code %d)" % code in msg, msg
    zeros = bytearray(GOOD)
    zeros[hd["data"]] = 0xC0
    zeros[hd["data"] + 1:hd["data"] + 6] = bytes(5)
    rc, msg, _ = cpu_decode([bytes(zeros)], W0, H0, W0, H0, False, np.uint16, 1)
    assert rc == 400 and "decoder code 3" in msg, msg
    with pytest.raises(ValueError, match="zero bit-planes above Mb"):
        J.decode(bytes(zeros))
    # flipped bits anywhere after the header: decoded (to garbage) or refused, never anything else
    rng = np.random.default_rng(11)
    for _ in range(200):
        bad = bytearray(GOOD)
        bad[int(rng.integers(hd["data"], len(GOOD)))] ^= 1 << int(rng.integers(8))
        rc, msg, _ = cpu_decode([bytes(bad)], W0, H0, W0, H0, False, np.uint16, 1)
        assert rc == 0 or (rc == 400 and "corrupt segment stream 0 (j2k, decoder code" in msg), msg


def test_older_calls_keep_their_texts(tmp_path):
    """The four new Compression values in the calls that do not take them, and an unsupported
    value in the Python layer: byte for byte what they answered before."""
    for comp in J.J2K_COMPRESSIONS:
        s, keep = segments_struct([GOOD], W0, H0, False, compression=comp)
        out4 = (ctypes.c_uint64 * 4)()
        assert pbx.lib().pbx_test_tiff_plan(ctypes.byref(s), W0, H0, 2, out4) == 400
        assert pbx.lib().pbx_last_error().decode() == "bad compression %d (1 none, 5 LZW, 8 deflate, 50000 zstd)" % comp
        assert pbx.lib().pbx_test_tiff_plan_samples(ctypes.byref(s), W0, H0, 1, 3, 0, 0, out4) == 400
        assert pbx.lib().pbx_last_error().decode() == "bad compression %d (1 none, 5 LZW, 8 deflate, 50000 zstd)" % comp
        j = pbx.PbxTiffJpeg()
        out6 = (ctypes.c_uint64 * 6)()
        assert pbx.lib().pbx_test_tiff_jpeg_plan(ctypes.byref(s), ctypes.byref(j), W0, H0, 1, 0, 0, out6) == 400
        assert pbx.lib().pbx_last_error().decode() == "bad compression %d (the JPEG calls take 7)" % comp
    pg = J.page_of(noise(W0, H0, 12), 34713, num_resolutions=3)
    path = str(tmp_path / "c.tif")
    J.write_tiff(path, [pg])
    with pytest.raises(pbx.PbxError) as e:
        pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0)
    assert str(e.value).endswith("Compression 34713 (1 none, 5 LZW, 8 / 32946 deflate, 50000 zstd)")
