"""Bit-packed TIFF samples (k_tiff_unpack_place), PackBits (k_tiff_packbits) and FillOrder 2 on the
GPU, at registration (pbx_planes_register_tiff_packed) and band by band
(pbx_band_write_tiff_packed).

Expected bytes: the numpy array a segment was packed from by tests/_tiff_packed.py, as uint8
(1 .. 8 bits) or big-endian uint16 (9 .. 16), unscaled: what Bio-Formats hands the reference.  That
restatement stands alone for every width but 1 and 8 bits, where tests/test_tiff_packed_host.py
holds it against PIL; everything is compared byte for byte on values over the whole range.

Sizes: a lane of k_tiff_unpack_place owns 16 output bytes and a wave step 1024, so width 41 ends a
row mid-byte and leaves most lanes idle, 70 is a row shorter than a wave's step with a partial
last lane, and 333 (uint16: 666 bytes) and 1100 (uint8) take more than one wave step; strips of 7
rows on 17 give a short last strip, and a workgroup walks 16 rows, so 17-row tiles' planes (45
rows, 16-row tiles) and 20-row strips cross it."""
import itertools

import numpy as np
import pytest

import _tiff_packed as K
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(12_300_000)  # disjoint from the other test files (shared service)
ALL_BITS = [1, 2, 4, 7, 8, 10, 12, 14, 15, 16]
RNG = np.random.default_rng(32773)


def pt_of(bits):
    return pbx.UINT8 if bits <= 8 else pbx.UINT16


def layer(a, bits, comp=1, tile=None, rps=None, fill=1, bo=">", image=None, segs=None):
    """Register specs (one per sample, sharing one segments object) of a (rows, width[, S]) array."""
    a3 = a if a.ndim == 3 else a[:, :, None]
    h, w, s = a3.shape
    if segs is None:
        segs = [K.compress(x, comp) for x in K.segments_of(a3, bits, tile, rps, 1, fill, bo)]
    image = next(_ids) if image is None else image
    base = dict(image_id=image, z=0, t=0, pixel_type=pt_of(bits), size_x=w, size_y=h,
                seg_w=tile[0] if tile else w, seg_h=tile[1] if tile else (rps or h), tiled=tile is not None,
                compression=comp, predictor=1, big_endian=bo == ">", segments=segs,
                packed=dict(bits=bits, fill_order=fill), samples_per_pixel=s)
    return [dict(base, c=c, sample=c) for c in range(s)]


def check(service, specs, wants):
    ids = service.register_tiff_planes(specs)
    try:
        for pid, sp, want in zip(ids, specs, wants):
            got = service.read_plane_be(pid, len(want))
            assert got == want, (sp["packed"], sp["size_x"], sp["seg_w"], sp["seg_h"], sp["compression"], sp["sample"])
    finally:
        for pid in ids:
            service.release_plane(pid)


def rows_of(svc, image, y0, rows, w, c=0):
    st, body = svc.get_tile(pbx.TileCtx(image, 0, c, 0, 0, y0, w, rows))
    assert st == pbx.OK, st
    return body


# ----------------------------------------------------------------- widths, byte orders, layouts
@pytest.mark.parametrize("bo", ["<", ">"], ids=["II", "MM"])
def test_strips_of_every_width(service, bo):
    """Widths 41, 70, 333 and 1100, strips of 7 rows on 17 (a short last strip), every sample width,
    all planes of a byte order in one registration."""
    specs, wants = [], []
    for bits in ALL_BITS:
        for w in (41, 70, 333, 1100):
            a = K.noise(RNG, 17, w, bits)
            specs += layer(a, bits, rps=7, bo=bo)
            wants.append(K.expected_be(a, bits))
    check(service, specs, wants)


@pytest.mark.parametrize("bo", ["<", ">"], ids=["II", "MM"])
def test_tiles_whose_padding_never_reaches_the_plane(service, bo):
    """16 x 16 and 32 x 16 tiles on 70 x 45: padding columns and rows are all ones, the planes are
    read back whole, and (pitched rows, 256 bytes) a byte stored past the width would show in no
    read: the last rows' neighbours are checked through a second plane registered right after."""
    specs, wants = [], []
    for bits in ALL_BITS:
        for tile in ((16, 16), (32, 16)):
            a = K.noise(RNG, 45, 70, bits)
            a[:, -1] = 0  # the column next to the padding
            a[-1, :] = 0
            specs += layer(a, bits, tile=tile, bo=bo)
            wants.append(K.expected_be(a, bits))
    check(service, specs, wants)


def test_fill_order_2(service):
    specs, wants = [], []
    for bits in (1, 4, 12, 8):
        for tile, rps, w in ((None, 7, 41), (None, 7, 333), ((16, 16), None, 70)):
            a = K.noise(RNG, 17, w, bits)
            specs += layer(a, bits, tile=tile, rps=rps, fill=2, bo="<")
            wants.append(K.expected_be(a, bits))
    check(service, specs, wants)


def test_chunky_samples_into_separate_planes(service):
    """S = 3 at 4 bits and S = 2 at 12 bits (the issue's pair), and S = 4 at 1, 7 and 14 bits, where
    a lane's span is the longest; strips and tiles; one layer each, decoded once."""
    specs, wants = [], []
    for bits, s in ((4, 3), (12, 2), (1, 4), (7, 4), (14, 4), (10, 3), (8, 3), (16, 2)):
        for tile, rps, w, bo in ((None, 7, 41, "<"), (None, 5, 333, ">"), ((32, 16), None, 70, "<")):
            a = K.noise(RNG, 17 if tile is None else 45, w, bits, s)
            specs += layer(a, bits, tile=tile, rps=rps, bo=bo)
            wants += [K.expected_be(a[:, :, c], bits) for c in range(s)]
    check(service, specs, wants)


def test_one_sample_of_a_chunky_layer(service):
    """Not every sample need be named: the others' destinations are null."""
    a = K.noise(RNG, 17, 70, 12, 3)
    specs = layer(a, 12, rps=7)
    check(service, specs[1:2], [K.expected_be(a[:, :, 1], 12)])


def test_planar_file_and_chunky_file(service, tmp_path):
    """register_tiff_image (packed on by default): a planar S = 3 file of 12-bit samples gives three
    single-sample layers, a chunky 4-bit one a single layer."""
    for bits, planar, bo in ((12, 2, "<"), (4, 1, ">")):
        a = K.noise(RNG, 45, 70, bits, 3)
        p = str(tmp_path / ("s3_%d.tif" % bits))
        K.write_tiff(p, [K.page_of(a, bits, 5, tile=(32, 16), planar=planar, byteorder=bo)], bo)
        image = next(_ids)
        ids = service.register_tiff_image(p, image)
        try:
            assert sorted(ids[0]) == [(0, c, 0) for c in range(3)]
            for c in range(3):
                want = K.expected_be(a[:, :, c], bits)
                assert service.read_plane_be(ids[0][(0, c, 0)], len(want)) == want, (bits, c)
        finally:
            for pid in ids[0].values():
                service.release_plane(pid)


# -------------------------------------------------------------------------------- compressions
def _have_zstd():
    try:
        import _zarr
        _zarr._libzstd()
        return True
    except OSError:
        return False


@pytest.mark.parametrize("comp", [1, 5, 8, K.PACKBITS,
                                  pytest.param(K.ZSTD, marks=pytest.mark.skipif(not _have_zstd(),
                                                                                reason="no system libzstd"))],
                         ids=["stored", "lzw", "deflate", "packbits", "zstd"])
def test_compressions(service, comp):
    """1 and 12 bits behind every decoder, whose decoded length is rows x padded row bytes; smooth
    data too, so that LZW, deflate and PackBits find runs."""
    specs, wants = [], []
    for bits in (1, 12):
        for tile, rps, w in ((None, 7, 70), ((16, 16), None, 70), (None, 20, 333)):
            a = K.noise(RNG, 45, w, bits)
            a[10:30, 5:60] = a[10, 5]
            specs += layer(a, bits, comp, tile=tile, rps=rps)
            wants.append(K.expected_be(a, bits))
    check(service, specs, wants)


# ---------------------------------------------------------------------- hand-built PackBits
def lit(data):
    assert 1 <= len(data) <= 128
    return bytes([len(data) - 1]) + bytes(data)


def rep(n, b):
    assert 2 <= n <= 128
    return bytes([257 - n, b])


ROW = 150  # bytes of a row: 8 bits x 150 px; 4 rows = 600 bytes


def hand_streams():
    body = bytes(RNG.integers(0, 256, 600, dtype=np.uint8))
    streams = {}
    # a 128-byte literal, a 128-byte replicate, a 2-byte replicate, a no-op between runs, runs that
    # cross the rows' boundaries at 150, 300 and 450
    d = body[:128] + bytes([7]) * 128 + bytes([9]) * 2 + body[258:300] + bytes([1]) * 100 + body[400:600]
    s = (lit(d[:128]) + rep(128, 7) + b"\x80" + rep(2, 9) + b"\x80\x80" + lit(d[258:300]) + rep(100, 1) +
         lit(d[400:528]) + lit(d[528:600]))
    streams["runs of every kind"] = (s, d)
    streams["trailing bytes after the last row"] = (s + b"\x05trail\x80" + rep(128, 3), d)
    d2 = bytes([5]) * 600
    streams["replicates only"] = (rep(128, 5) * 4 + rep(88, 5), d2)
    streams["one-byte literals"] = (b"".join(lit(body[k:k + 1]) for k in range(600)), body)
    return streams


def packbits_spec(stream, image, bits=8, h=4, w=ROW):
    return dict(image_id=image, z=0, c=0, t=0, pixel_type=pt_of(bits), size_x=w, size_y=h, seg_w=w, seg_h=h,
                tiled=False, compression=K.PACKBITS, predictor=1, big_endian=True, segments=[stream],
                packed=dict(bits=bits, fill_order=1), samples_per_pixel=1, sample=0)


def test_hand_built_packbits_streams(service):
    streams = hand_streams()
    for name, (s, d) in streams.items():
        assert K.packbits_decode(s, 600) == d, name
    specs = [packbits_spec(s, next(_ids)) for s, _ in streams.values()]
    check(service, specs, [d for _, d in streams.values()])
    # the same bytes as rows of 12-bit samples: 4 rows of 100 samples
    s, d = streams["runs of every kind"]
    want = K.unpack_rows(d, 4, 100, 12).astype(">u2").tobytes()
    check(service, [packbits_spec(s, next(_ids), bits=12, w=100)], [want])


@pytest.mark.parametrize("case", ["truncated in a literal", "truncated before a header", "truncated in a replicate",
                                  "a literal overshooting", "a replicate overshooting"])
def test_bad_packbits_streams_register_nothing(service, case):
    s, d = hand_streams()["runs of every kind"]
    code = 1
    if case == "truncated in a literal":
        bad = s[:-10]
    elif case == "truncated before a header":
        bad = s[:-(1 + 72)]  # the last literal is gone altogether
    elif case == "truncated in a replicate":
        bad = rep(128, 5) * 4 + bytes([257 - 88])
    elif case == "a literal overshooting":
        bad, code = s[:-(1 + 72)] + lit(d[528:600] + b"x"), 3
    else:
        bad, code = rep(128, 5) * 4 + rep(89, 5), 3
    image, good_image = next(_ids), next(_ids)
    # all or none: the good plane of the same call is not registered either
    specs = [packbits_spec(s, good_image), packbits_spec(bad, image)]
    with pytest.raises(pbx.PbxError, match=r"corrupt chunk stream 1 \(packbits, decoder code %d\)" % code) as ei:
        service.register_tiff_planes(specs)
    assert ei.value.status == 400
    assert service.lookup_plane(image, 0, 0, 0) is None and service.lookup_plane(good_image, 0, 0, 0) is None


def test_refused_on_the_host_and_through_the_old_calls(service):
    a = K.noise(RNG, 17, 70, 12)
    sp = layer(a, 12, rps=7)[0]
    for change, msg in ((dict(packed=dict(bits=17)), "bad bits 17"), (dict(pixel_type=pbx.UINT8), "12-bit samples on a plane"),
                        (dict(packed=dict(bits=12, fill_order=3)), "bad fill_order 3"), (dict(predictor=2), "bad predictor 2"),
                        (dict(flags=1), "bad flags 0x1"), (dict(samples_per_pixel=5), "samples_per_pixel 5"),
                        (dict(compression=7), "bad compression 7")):
        with pytest.raises(pbx.PbxError, match=msg) as ei:
            service.register_tiff_planes([dict(sp, **change)])
        assert ei.value.status == 400
    assert service.lookup_plane(sp["image_id"], 0, 0, 0) is None
    # without `packed` the spec goes through pbx_planes_register_tiff, which knows no PackBits
    old = dict(packbits_spec(b"\x81\0", next(_ids)))
    del old["packed"]
    with pytest.raises(pbx.PbxError, match=r"bad compression 32773 \(1 none, 5 LZW, 8 deflate, 50000 zstd\)"):
        service.register_tiff_planes([old])
    with pytest.raises(pbx.PbxError, match=r"bad compression 32773 \(1 none, 5 LZW, 8 deflate, 50000 zstd\)"):
        service.register_tiff_planes([dict(old, samples_per_pixel=3, pixel_type=pbx.UINT8)])


# -------------------------------------------------------------------------------------- bands
def band_piece(svc, pid, sp, y0, rows, **kw):
    gx = -(-sp["size_x"] // sp["seg_w"]) if sp["tiled"] else 1
    segs = sp["segments"][(y0 // sp["seg_h"]) * gx:-(-(y0 + rows) // sp["seg_h"]) * gx]
    return svc.band_write_tiff_packed(pid, y0, rows, sp["seg_w"], sp["seg_h"], sp["tiled"], sp["compression"], segs,
                                      sp["packed"]["bits"], sp["packed"]["fill_order"], sp["samples_per_pixel"],
                                      sp["sample"], **kw)


@pytest.mark.parametrize("bits,comp,tile", [(12, 1, None), (12, K.PACKBITS, (32, 16)), (1, K.PACKBITS, None),
                                            (4, 5, (16, 16)), (10, 8, None)],
                         ids=["12 stored strips", "12 packbits tiles", "1 packbits strips", "4 lzw tiles",
                              "10 deflate strips"])
def test_bands_in_pieces(service, bits, comp, tile):
    """A sparse plane of 45 rows in bands of 20, written in pieces at rows that straddle strips of 7
    rows and tile rows of 16, some by this call and some by plain pbx_band_write."""
    a = K.noise(RNG, 45, 70, bits)
    sp = layer(a, bits, comp, tile=tile, rps=7)[0]
    want = K.expected_be(a, bits)
    rowb = len(want) // 45
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pt_of(bits), 70, 45, 20, big_endian=True)
    try:
        band_piece(service, pid, sp, 0, 9)                              # strips 0 .. 1, tile row 0
        service.band_write(pid, 9, 2, want[9 * rowb:11 * rowb])         # host rows in the same band
        ms = band_piece(service, pid, sp, 11, 9, timing=True)           # strips 1 .. 2, tile rows 0 .. 1
        assert len(ms) == 2 and ms[1] > 0
        assert service.band_info(pid)[1] == [pbx.BS_READY, pbx.BS_ABSENT, pbx.BS_ABSENT]
        band_piece(service, pid, sp, 20, 20)
        band_piece(service, pid, sp, 40, 5)                             # the short last strip, the last tile row
        assert set(service.band_info(pid)[1]) == {pbx.BS_READY}
        assert rows_of(service, image, 0, 45, 70) == want
        with pytest.raises(pbx.PbxError) as ei:
            band_piece(service, pid, sp, 0, 20)
        assert ei.value.status == pbx.E_EXISTS
    finally:
        service.release_plane(pid)


def test_one_sample_of_chunky_segments_band_by_band(service):
    a = K.noise(RNG, 45, 70, 4, 3)
    specs = layer(a, 4, 1, tile=(32, 16), bo="<")
    for c in (0, 2):
        image = next(_ids)
        pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, 70, 45, 16)
        try:
            for r0 in range(0, 45, 16):
                band_piece(service, pid, specs[c], r0, min(16, 45 - r0))
            assert rows_of(service, image, 0, 45, 70) == K.expected_be(a[:, :, c], 4)
        finally:
            service.release_plane(pid)


def test_a_bad_stream_fails_the_band_load(service):
    a = K.noise(RNG, 45, 70, 12)
    sp = layer(a, 12, K.PACKBITS, rps=7)[0]
    bad = dict(sp, segments=list(sp["segments"]))
    bad["segments"][1] = bad["segments"][1][:-4]
    image = next(_ids)
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT16, 70, 45, 20, big_endian=True)
    try:
        with pytest.raises(pbx.PbxError, match=r"corrupt chunk stream 1 \(packbits, decoder code 1\)") as ei:
            band_piece(service, pid, bad, 0, 20)
        assert ei.value.status == 400
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT] * 3
        with pytest.raises(pbx.PbxError, match="bad bits 0") as ei:
            band_piece(service, pid, dict(sp, packed=dict(bits=0, fill_order=1)), 0, 20)
        assert ei.value.status == 400
        band_piece(service, pid, sp, 0, 20)
        assert rows_of(service, image, 0, 20, 70) == K.expected_be(a[:20], 12)
    finally:
        service.release_plane(pid)


def test_tiles_served_from_a_loaded_plane(service):
    """A PNG tile and a raw tile from the loaded plane equal the same tiles from a plane registered
    from the unpacked array."""
    a = K.noise(RNG, 45, 70, 12)
    sp = layer(a, 12, K.PACKBITS, tile=(32, 16), bo="<")[0]
    other = next(_ids)
    pid = service.register_tiff_planes([sp])[0]
    ref = service.register_plane(other, 0, 0, 0, pbx.UINT16, 70, 45, data=a.astype("<u2"))
    try:
        for fmt in ("png", None):
            kw = dict(format=fmt) if fmt else {}
            got = service.get_tile(pbx.TileCtx(sp["image_id"], 0, 0, 0, 3, 5, 60, 37, **kw))
            want = service.get_tile(pbx.TileCtx(other, 0, 0, 0, 3, 5, 60, 37, **kw))
            assert got[0] == pbx.OK and got == want, fmt
        assert got[1] == a[5:42, 3:63].astype(">u2").tobytes()
    finally:
        service.release_plane(pid)
        service.release_plane(ref)


# --------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("bits,comp,tile,sparse", [(12, 8, (32, 16), 0), (12, 1, (32, 16), 16),
                                                   (1, K.PACKBITS, None, 0), (1, K.PACKBITS, None, 16)],
                         ids=["12-bit tiles whole", "12-bit tiles in bands", "1-bit packbits whole",
                              "1-bit packbits in bands"])
def test_tiff_source(tmp_path, bits, comp, tile, sparse):
    a = K.noise(RNG, 45, 70, bits)
    a[20:30, 10:50] = 1
    bo = "<" if bits == 12 else ">"
    p = str(tmp_path / "e2e.tif")
    K.write_tiff(p, [K.page_of(a, bits, comp, tile=tile, rows_per_strip=7, byteorder=bo)], bo)
    image = next(_ids)
    with pbx.PixelsService(**({"sparse_band_rows": sparse} if sparse else {})) as svc:
        src = pbx.TiffSource({image: p})
        assert src.get_pixels(image).pixel_type == pt_of(bits)
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(image, 0, 0, 0, 3, 18, 60, 20), src).get_tile()
        assert body == K.expected_be(a[18:38, 3:63], bits)
        if sparse:
            assert svc.residency_stats()["bands"] == 2 and svc.residency_stats()["planes"] == 0
        # with the keyword off the file is refused as it always was
        with pytest.raises(pbx.PbxError, match="BitsPerSample %d" % bits):
            pbx.TiffSource({image: p}, packed=False).get_pixels(image)
