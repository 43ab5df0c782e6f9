"""Bit-packed TIFF samples, PackBits and FillOrder 2 without a GPU: the restatement of
tests/_tiff_packed.py against itself, np.packbits and PIL; the host planner (tiff_packed_plan,
through pbx_test_tiff_packed_plan): padded row bytes, short segments, band rows, every refusal with
its text; the Python layer with the `packed` keyword on and off.

PIL is the only TIFF library here and opens 1-bit files of either fill order and 8-bit PackBits
files; for every other width (2, 4, 7, 10, 12, 14, 15 bits) the restatement stands alone: its
packer (shift-and-or, one bit at a time) and its unpacker (one big integer per row) are written
the opposite way round and must agree.  The sanitizer run of the planner is `make san`
(scripts/tiff_packed_san.cpp)."""
import ctypes
import re

import numpy as np
import pytest

import _tiff_packed as K
import _tiff_src as T
import pbx

RNG = np.random.default_rng(1273)
ALL_BITS = [1, 2, 4, 7, 8, 10, 12, 14, 15, 16]


# ------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("bits,fill", [(b, f) for b in ALL_BITS for f in (1, 2) if (b, f) != (16, 2)])
def test_packer_and_unpacker_agree(bits, fill):
    for w in (1, 7, 16, 41, 70):  # (FillOrder 2 on 16-bit samples is refused: not a case)
        a = K.noise(RNG, 5, w, bits)
        packed = K.pack_rows(a, bits, fill)
        assert packed.shape == (5, K.row_bytes(w, bits))
        assert (K.unpack_rows(packed.tobytes(), 5, w, bits, fill) == a).all()


def test_packer_against_numpy_packbits_and_plain_bytes():
    a = K.noise(RNG, 9, 70, 1)
    for fill in (1, 2):
        assert (K.pack_rows(a, 1, fill) == K.pack_rows_1bit(a, fill)).all()
    assert K.pack_rows(a, 1)[0, 0] == 0x80 | (K.pack_rows(a, 1)[0, 0] & 0x3f)  # sample 0 (1) is the MSB, sample 1 (0) next
    b = K.noise(RNG, 3, 41, 8)
    assert K.pack_rows(b, 8).tobytes() == b.astype(np.uint8).tobytes()
    c = K.noise(RNG, 3, 41, 16)
    assert K.pack_rows(c, 16, byteorder=">").tobytes() == c.astype(">u2").tobytes()
    assert K.pack_rows(c, 16, byteorder="<").tobytes() == c.astype("<u2").tobytes()
    # 12 bits, two samples: AB CD EF -> 0xABC, 0xDEF
    assert K.pack_rows(np.array([[0xABC, 0xDEF]]), 12).tobytes() == bytes([0xAB, 0xCD, 0xEF])
    # 4 bits, FillOrder 2: the byte 0x1E read bit-reversed
    assert K.pack_rows(np.array([[1, 0xE]]), 4, 2).tobytes() == bytes([0x78])


def test_packbits_restatement():
    for data in (b"", b"a", b"ab" * 100, b"\0" * 1000, bytes(RNG.integers(0, 4, 3000, dtype=np.uint8)),
                 bytes(RNG.integers(0, 256, 700, dtype=np.uint8)), b"x" * 128 + b"y" * 129 + b"zz"):
        enc = K.packbits_encode(data)
        assert K.packbits_decode(enc, len(data)) == data
        assert K.packbits_decode(enc + b"\x05trailing", len(data)) == data
    # TIFF 6.0 section 9's own example
    raw = bytes([0xAA, 0xAA, 0xAA, 0x80, 0x00, 0x2A, 0xAA, 0xAA, 0xAA, 0xAA, 0x80, 0x00, 0x2A, 0x22] + [0xAA] * 10)
    spec = bytes([0xFE, 0xAA, 0x02, 0x80, 0x00, 0x2A, 0xFD, 0xAA, 0x03, 0x80, 0x00, 0x2A, 0x22, 0xF7, 0xAA])
    assert K.packbits_decode(spec, len(raw)) == raw
    with pytest.raises(ValueError):
        K.packbits_decode(spec[:-1], len(raw))
    with pytest.raises(ValueError):
        K.packbits_decode(spec, len(raw) - 1)


def test_pil_agrees_where_it_can_open_the_file(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a = K.noise(RNG, 45, 70, 1)
    for fill in (1, 2):
        for comp in (1, K.PACKBITS):
            for bo in ("<", ">"):
                p = str(tmp_path / ("m%d_%d%s.tif" % (fill, comp, "l" if bo == "<" else "b")))
                K.write_tiff(p, [K.page_of(a, 1, comp, rows_per_strip=7, fill_order=fill, byteorder=bo)], bo)
                with Image.open(p) as im:
                    got = np.array(im.convert("L"))
                assert (got == a * 255).all(), (fill, comp, bo)  # PIL shows 0 / 255, the restatement 0 / 1
    b = K.noise(RNG, 45, 70, 8)
    p = str(tmp_path / "g8.tif")
    K.write_tiff(p, [K.page_of(b, 8, K.PACKBITS, rows_per_strip=7)], ">")
    with Image.open(p) as im:
        assert (np.array(im) == b).all()


# ------------------------------------------------------------------------------ the planner
def plan(segs, bits, size_x, size_y, seg_w, seg_h, tiled=0, compression=1, fill_order=1, spp=1, sample=0,
         pixel_type=None, predictor=1, flags=0, y0=0, rows=0):
    data, offsets = segs if isinstance(segs, tuple) else pbx.pack_chunks(segs)
    s = pbx.PbxTiffSegments(seg_w, seg_h, tiled, compression, predictor, flags, data.ctypes.data, offsets.ctypes.data)
    k = pbx.PbxTiffPacked(bits, fill_order, spp, sample)
    out = (ctypes.c_uint64 * 6)()
    if pixel_type is None:
        pixel_type = pbx.UINT16 if bits > 8 else pbx.UINT8
    rc = pbx.lib().pbx_test_tiff_packed_plan(ctypes.byref(s), ctypes.byref(k), size_x, size_y, pixel_type, y0, rows,
                                             out)
    return rc, list(out), pbx.lib().pbx_last_error().decode()


@pytest.mark.parametrize("bits,w,rb", [(12, 41, 62), (1, 70, 9), (10, 16, 20), (4, 41, 21), (7, 333, 292),
                                       (14, 70, 123), (2, 41, 11), (15, 41, 77), (8, 41, 41), (16, 41, 82)])
def test_padded_row_bytes(bits, w, rb):
    assert K.row_bytes(w, bits) == rb
    rc, out, err = plan([b"\0" * (rb * 5)], bits, w, 5, w, 5)
    assert (rc, out) == (0, [0, 5 * rb, 0, 1, rb, 5]), err
    # three chunky samples share the row's padding: ceil(w * 3 * bits / 8)
    rb3 = (w * 3 * bits + 7) // 8
    rc, out, err = plan([b"\0" * (rb3 * 5)], bits, w, 5, w, 5, spp=3, sample=2)
    assert (rc, out[4]) == (0, rb3), err
    # one byte more or less is not the segment
    for n in (rb * 5 - 1, rb * 5 + 1):
        rc, _, err = plan([b"\0" * n], bits, w, 5, w, 5)
        assert rc == 400 and "uncompressed segment 0: %d bytes, not %d" % (n, rb * 5) in err


def test_short_last_strip_edge_tiles_and_band_rows():
    rb = K.row_bytes(70, 12)  # 105
    strips = [b"\1" * (rb * r) for r in (7, 7, 7, 7, 7, 7, 3)]
    rc, out, err = plan(strips, 12, 70, 45, 70, 7)
    assert (rc, out) == (0, [0, 45 * rb, 0, 7, rb, 45]), err
    # rows 40 .. 44 (y0 no multiple of 7): strips 5 and 6, 7 + 3 rows
    rc, out, err = plan(strips[5:], 12, 70, 45, 70, 7, y0=40, rows=5)
    assert (rc, out) == (0, [0, 10 * rb, 0, 2, rb, 10]), err
    # handing over the full last strip where 3 rows are left is refused
    rc, _, err = plan([strips[0], strips[0]], 12, 70, 45, 70, 7, y0=40, rows=5)
    assert rc == 400 and "uncompressed segment 1" in err
    # compressed strips: one stream each, scratch of rows * padded bytes rounded up to 256
    rc, out, err = plan([b"\x81\0"] * 7, 12, 70, 45, 70, 7, compression=K.PACKBITS)
    assert (rc, out) == (0, [7, 45 * rb, 6 * 768 + 512, 7, rb, 45]), err
    # 32 x 16 tiles on 70 x 45: 3 x 3 full tiles of 48 bytes a row
    tiles = [b"\2" * (48 * 16)] * 9
    rc, out, err = plan(tiles, 12, 70, 45, 32, 16, tiled=1)
    assert (rc, out) == (0, [0, 9 * 768, 0, 9, 48, 144]), err
    rc, out, err = plan(tiles[:6], 12, 70, 45, 32, 16, tiled=1, y0=17, rows=17)  # tile rows 1 and 2
    assert (rc, out) == (0, [0, 6 * 768, 0, 6, 48, 96]), err
    rc, out, err = plan(tiles[:3], 12, 70, 45, 32, 16, tiled=1, y0=33, rows=12)  # the last tile row alone
    assert (rc, out[3]) == (0, 3), err
    # 1-bit 16 x 16 tiles: 2 bytes a row, no padding
    rc, out, err = plan([b"\0" * 32] * 15, 1, 70, 45, 16, 16, tiled=1)
    assert (rc, out) == (0, [0, 15 * 32, 0, 15, 2, 240]), err


C_REFUSALS = [
    ("bits 0", dict(bits=0), "bad bits 0 (1 .. 16)"),
    ("bits 17", dict(bits=17), "bad bits 17 (1 .. 16)"),
    ("12 bits on uint8", dict(pixel_type=pbx.UINT8), "12-bit samples on a plane of pixel type 1"),
    ("12 bits on float", dict(pixel_type=pbx.FLOAT), "12-bit samples on a plane of pixel type 6"),
    ("12 bits on uint32", dict(pixel_type=pbx.UINT32), "12-bit samples on a plane of pixel type 5"),
    ("4 bits on uint16", dict(bits=4, pixel_type=pbx.UINT16), "4-bit samples on a plane of pixel type 3"),
    ("8 bits on uint16", dict(bits=8, pixel_type=pbx.UINT16), "8-bit samples on a plane of pixel type 3"),
    ("fill_order 0", dict(fill_order=0), "bad fill_order 0 (1 or 2)"),
    ("fill_order 3", dict(fill_order=3), "bad fill_order 3 (1 or 2)"),
    ("fill_order 2 on 16 bits", dict(bits=16, fill_order=2), "fill_order 2 on 16-bit samples"),
    ("predictor 2", dict(predictor=2), "bad predictor 2 (bit-packed samples take 1 only"),
    ("predictor 3", dict(predictor=3), "bad predictor 3 (bit-packed samples take 1 only"),
    ("flags", dict(flags=1), "bad flags 0x1"),
    ("spp 0", dict(spp=0), "samples_per_pixel 0 outside 1 .. 4"),
    ("spp 5", dict(spp=5), "samples_per_pixel 5 outside 1 .. 4"),
    ("sample 3 of 3", dict(spp=3, sample=3), "sample 3 outside segments of 3 samples per pixel"),
    # what tiff_segments_check refuses
    ("compression 2", dict(compression=2), "bad compression 2 (1 none, 5 LZW, 8 deflate, 50000 zstd, 32773 PackBits)"),
    ("compression 7", dict(compression=7), "bad compression 7"),
    ("seg_w 0", dict(seg_w=0), "bad segment shape 0 x 4"),
    ("tile 24 x 16", dict(tiled=1, seg_w=24, seg_h=16), "TileWidth and TileLength must be multiples of 16"),
    ("strip width", dict(seg_w=40), "strip width 40 != plane width 41"),
    ("rows outside", dict(y0=3, rows=2), "rows 3+2 outside the plane (4 rows)"),
]


@pytest.mark.parametrize("name,change,msg", C_REFUSALS, ids=[r[0] for r in C_REFUSALS])
def test_planner_refusals(name, change, msg):
    kw = dict(bits=12, size_x=41, size_y=4, seg_w=41, seg_h=4)
    assert plan([b"\0" * 248], **kw)[0] == 0
    kw.update(change)
    rc, _, err = plan([b"\0" * 248], **kw)
    assert rc == 400 and msg in err, err


def test_planner_refuses_bad_segments():
    kw = dict(bits=12, size_x=41, size_y=4, seg_w=41, seg_h=4)
    rc, _, err = plan([b""], compression=K.PACKBITS, **kw)
    assert rc == 400 and "segment 0 is empty" in err
    rc, _, err = plan([b"\0\1\0"], compression=5, **kw)
    assert rc == 400 and "old-style" in err
    rc, _, err = plan([b"\x78\x9c\3\0\0\0\0\1"], compression=K.ZSTD, **kw)
    assert rc == 400 and "zstd" in err


def test_the_old_calls_keep_refusing():
    """pbx_planes_register_tiff, its _samples form and pbx_band_write_tiff (their planner hooks):
    compression 32773 and non-zero flags are answered as they always were."""
    data, offsets = pbx.pack_chunks([b"\x81\0"])
    out = (ctypes.c_uint64 * 4)()
    L = pbx.lib()
    for flags, comp, msg in ((0, K.PACKBITS, "bad compression 32773 (1 none, 5 LZW, 8 deflate, 50000 zstd)"),
                             (1, 1, "bad flags 0x1")):
        s = pbx.PbxTiffSegments(41, 4, 0, comp, 1, flags, data.ctypes.data, offsets.ctypes.data)
        for rc in (L.pbx_test_tiff_plan(ctypes.byref(s), 41, 4, 1, out),
                   L.pbx_test_tiff_plan_samples(ctypes.byref(s), 41, 4, 1, 3, 0, 0, out),
                   L.pbx_test_tiff_band_plan(ctypes.byref(s), 41, 4, 1, 0, 4, out)):
            assert rc == 400 and L.pbx_last_error().decode().endswith(msg)
    assert L.pbx_abi_version() == 9 and ctypes.sizeof(pbx.PbxTiffSegments) == 40 and ctypes.sizeof(pbx.PbxTiffPacked) == 16


# ------------------------------------------------------------------------- the Python layer
def packed_file(tmp_path, name, bits, comp=1, fill=1, bo=">", tile=None, rps=7, s=None, planar=1, **page_kw):
    a = K.noise(RNG, 45, 70, bits, s)
    p = str(tmp_path / name)
    K.write_tiff(p, [K.page_of(a, bits, comp, tile=tile, rows_per_strip=rps, planar=planar, fill_order=fill,
                               byteorder=bo, **page_kw)], bo)
    return p, a


PY_CASES = [
    ("1 bit", dict(bits=1), pbx.UINT8, "BitsPerSample 1 (8, 16, 32 or 64)"),
    ("4 bits", dict(bits=4), pbx.UINT8, "BitsPerSample 4 (8, 16, 32 or 64)"),
    ("12 bits", dict(bits=12, bo="<"), pbx.UINT16, "BitsPerSample 12 (8, 16, 32 or 64)"),
    ("14 bits tiled", dict(bits=14, tile=(32, 16)), pbx.UINT16, "BitsPerSample 14 (8, 16, 32 or 64)"),
    ("packbits 8", dict(bits=8, comp=K.PACKBITS), pbx.UINT8,
     "Compression 32773 (1 none, 5 LZW, 8 / 32946 deflate, 50000 zstd)"),
    ("packbits 1", dict(bits=1, comp=K.PACKBITS), pbx.UINT8, "BitsPerSample 1 (8, 16, 32 or 64)"),
    ("fillorder 2 on 8", dict(bits=8, fill=2), pbx.UINT8, "FillOrder 2 (only 1 is supported)"),
    ("fillorder 2 on 12", dict(bits=12, fill=2), pbx.UINT16, "BitsPerSample 12 (8, 16, 32 or 64)"),
]


@pytest.mark.parametrize("name,kw,pt,old", PY_CASES, ids=[c[0] for c in PY_CASES])
def test_python_specs_with_the_keyword_and_old_refusals_without(tmp_path, name, kw, pt, old):
    p, a = packed_file(tmp_path, "f.tif", **kw)
    ifd = pbx.tiff_ifds(p)[0]
    for call in (lambda: pbx.tiff_image_layout(p), lambda: pbx.tiff_plane_spec(p, ifd, 1, 0, 0, 0),
                 lambda: pbx.tiff_band_spec(p, ifd, 0, 0)):
        with pytest.raises(pbx.PbxError, match=re.escape(old)) as e:
            call()
        assert e.value.status == 400
    assert pbx.tiff_image_layout(p, packed=True)["pixel_type"] == pt
    sp = pbx.tiff_plane_spec(p, ifd, 1, 0, 0, 0, packed=True)
    assert sp["packed"] == dict(bits=kw["bits"], fill_order=kw.get("fill", 1))
    assert sp["pixel_type"] == pt and sp["compression"] == kw.get("comp", 1) and sp["predictor"] == 1
    assert sp["big_endian"] == (kw.get("bo", ">") == ">") and sp["samples_per_pixel"] == 1
    data, offsets = sp["segments"]
    # the planner takes what the spec hands over, and the file's segments are the restatement's
    tile = kw.get("tile")
    rc, out, err = plan((data, offsets), kw["bits"], 70, 45, sp["seg_w"], sp["seg_h"], 1 if tile else 0,
                        sp["compression"], sp["packed"]["fill_order"])
    assert rc == 0 and out[3] == (9 if tile else 7), err
    bsp = pbx.tiff_band_spec(p, ifd, 40, 5, packed=True)
    assert bsp["packed"] == sp["packed"] and len(bsp["segments"][1]) == (3 if tile else 2) + 1
    if kw.get("comp", 1) == 1 and not tile:
        rows = K.unpack_rows(bytes(data[:int(offsets[1])]), 7, 70, kw["bits"], kw.get("fill", 1), kw.get("bo", ">"))
        assert (rows == a[:7]).all()


def test_python_specs_of_ordinary_files_do_not_change(tmp_path):
    a = np.arange(45 * 70, dtype="<u2").reshape(45, 70)
    p = str(tmp_path / "plain.tif")
    T.write_tiff(p, [T.page_of(a, 5, rows_per_strip=7)])
    ifd = pbx.tiff_ifds(p)[0]
    plain, on = pbx.tiff_plane_spec(p, ifd, 1, 0, 0, 0), pbx.tiff_plane_spec(p, ifd, 1, 0, 0, 0, packed=True)
    assert "packed" not in on and sorted(plain) == sorted(on)
    assert pbx.tiff_image_layout(p, packed=True)["pixel_type"] == pbx.UINT16
    assert pbx.TiffSource({1: p})._j2k_kw(ifd) == {}


def test_python_chunky_and_planar_specs(tmp_path):
    p, a = packed_file(tmp_path, "rgb4.tif", 4, s=3)
    ifd = pbx.tiff_ifds(p)[0]
    sp = pbx.tiff_plane_spec(p, ifd, 1, 0, 1, 0, sample=1, packed=True)
    assert (sp["samples_per_pixel"], sp["sample"], sp["pixel_type"]) == (3, 1, pbx.UINT8)
    assert int(sp["segments"][1][1]) == 7 * K.row_bytes(70 * 3, 4)
    lay = pbx.tiff_image_layout(p, packed=True)
    assert (lay["samples"], lay["size_c"]) == (3, 3)
    p, a = packed_file(tmp_path, "planar12.tif", 12, s=3, planar=2, bo="<")
    ifd = pbx.tiff_ifds(p)[0]
    sp = pbx.tiff_plane_spec(p, ifd, 1, 0, 2, 0, sample=2, packed=True)
    assert (sp["samples_per_pixel"], sp["sample"], sp["pixel_type"]) == (1, 0, pbx.UINT16)
    rows = K.unpack_rows(bytes(sp["segments"][0][:int(sp["segments"][1][1])]), 7, 70, 12)
    assert (rows == a[:7, :, 2]).all()
    assert pbx.TiffSource({1: p})._j2k_kw(ifd) == {"packed": True}
    assert pbx.TiffSource({1: p}, packed=False)._j2k_kw(ifd) == {}


PY_STILL_REFUSED = [
    ("palette", dict(bits=4, photometric=3), "PhotometricInterpretation 3 (palette colour) is not supported"),
    ("palette packbits 8", dict(bits=8, comp=K.PACKBITS, photometric=3), "PhotometricInterpretation 3 (palette colour)"),
    ("white is zero", dict(bits=1, photometric=0), "PhotometricInterpretation 0 (WhiteIsZero) on 1-bit packed samples"),
    ("predictor 2 on 12 bits", dict(bits=12, predictor=2),"Predictor 2 with BitsPerSample 12"),
    ("predictor 2 on packbits", dict(bits=8, comp=K.PACKBITS, predictor=2), "Predictor 2 with Compression 32773"),
    ("signed 4 bits", dict(bits=4, sampleformat=2), "SampleFormat 2 with BitsPerSample 4"),
    ("unequal bits", dict(bits=4, s=3, extra=[(258, 3, [4, 4, 2])]), "samples differ in bits"),
    ("fill order 2 on 16", dict(bits=16, fill=2), "FillOrder 2 with 16-bit samples"),
    ("fill order 3", dict(bits=4, extra=[(266, 3, [3])]), "FillOrder 3"),
    ("ccitt", dict(bits=1, extra=[(259, 3, [4])]), "Compression 4"),
    ("orientation", dict(bits=4, extra=[(274, 3, [3])]), "Orientation 3"),
]


@pytest.mark.parametrize("name,kw,msg", PY_STILL_REFUSED, ids=[c[0] for c in PY_STILL_REFUSED])
def test_python_refusals_with_the_keyword_on(tmp_path, name, kw, msg):
    p, _ = packed_file(tmp_path, "r.tif", **kw)
    for call in (lambda: pbx.tiff_image_layout(p, packed=True),
                 lambda: pbx.tiff_plane_spec(p, pbx.tiff_ifds(p)[0], 1, 0, 0, 0, packed=True),
                 lambda: pbx.TiffSource({1: p}).get_pixels(1)):
        with pytest.raises(pbx.PbxError, match=re.escape(msg)) as e:
            call()
        assert e.value.status == 400
