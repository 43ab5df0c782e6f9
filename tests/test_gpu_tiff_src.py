"""Planes loaded from TIFF / OME-TIFF segments on the GPU (pbx_planes_register_tiff): k_tiff_lzw,
k_tiff_unpred, and the deflate / stored segments through the Zarr decoders.

Expected bytes: the fixtures' .npy (tests/golden/tiff), or the numpy array a stream was encoded
from by tests/_tiff_src.py (whose encoder tests/test_tiff_src_host.py pins against libtiff).
Everything is compared byte for byte."""
import itertools
import json
import os

import numpy as np
import pytest

import _tiff_src as T
import pbx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "tiff")
with open(os.path.join(GOLD, "manifest.json")) as _f:
    FILES = json.load(_f)["files"]
_ids = itertools.count(7_300_000)


def expected(entry, level="0", key="0,0,0"):
    npy = entry["planes"][level][key]
    if npy is None:  # the PIL-written ramp
        w, h = entry["width"], entry["length"]
        return ((np.arange(w)[None, :] % 100 + np.arange(h)[:, None] // 4) & 0xFF).astype(np.uint8)
    return np.load(os.path.join(GOLD, npy))


def raw_tile(svc, image_id, z, c, t, x, y, w, h, resolution=None):
    st, body = svc.get_tile(pbx.TileCtx(image_id, z, c, t, x, y, w, h, resolution=resolution))
    assert st == 0, st
    return body


# ------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("entry", FILES, ids=[f["file"] for f in FILES])
def test_fixture(service, entry):
    image = next(_ids)
    ids = service.register_tiff_image(os.path.join(GOLD, entry["file"]), image)
    try:
        assert sorted(ids) == sorted(int(k) for k in entry["planes"])
        levels = len(ids)
        for level, planes in ids.items():
            assert sorted("%d,%d,%d" % p for p in planes) == sorted(entry["planes"][str(level)])
            for (z, c, t), pid in planes.items():
                want = expected(entry, str(level), "%d,%d,%d" % (z, c, t))
                got = service.read_plane_be(pid, want.nbytes)
                assert got == want.tobytes(), (entry["file"], level, z, c, t)
        # one raw tile request, across a segment boundary where the image has one
        level = levels - 1
        (z, c, t) = sorted(ids[level])[-1]
        want = expected(entry, str(level), "%d,%d,%d" % (z, c, t))
        h, w = want.shape
        x, y, tw, th = w // 3, h // 4, w // 2, h // 2
        body = raw_tile(service, image, z, c, t, x, y, tw, th, resolution=0 if levels > 1 else None)
        assert body == want[y:y + th, x:x + tw].tobytes()
    finally:
        for planes in ids.values():
            for pid in planes.values():
                service.release_plane(pid)


# ---------------------------------------------------------------------- LZW edge streams
def u8_plane(image, w, h, streams, seg_h=None, **kw):
    return dict(image_id=image, z=0, c=0, t=0, pixel_type=pbx.UINT8, size_x=w, size_y=h, seg_w=w,
                seg_h=seg_h or h, tiled=False, compression=pbx.TIFF_LZW, predictor=1, segments=streams, **kw)


def check_u8(service, a, streams, seg_h=None):
    """Register the (h, w) uint8 array from its strips' streams and compare."""
    pid, = service.register_tiff_planes([u8_plane(next(_ids), a.shape[1], a.shape[0], streams, seg_h)])
    try:
        assert service.read_plane_be(pid, a.size) == a.tobytes()
    finally:
        service.release_plane(pid)


def smooth(n, seed=1):
    return (np.random.default_rng(seed).poisson(6, n) & 0xFF).astype(np.uint8)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 70000])
def test_lzw_constant_bytes(service, n):
    # KwKwK on every code and ever longer self-overlapping matches
    w = 700 if n == 70000 else n
    a = np.full((n // w, w), 0xA7, np.uint8)
    check_u8(service, a, [T.lzw_encode(a.tobytes())])


def test_lzw_width_changes_and_the_clear_at_3836(service):
    a = np.random.default_rng(2).integers(0, 256, (60, 100), dtype=np.uint8)  # incompressible: 6000 codes
    codes = []
    s = T.lzw_encode(a.tobytes(), codes_out=codes)
    assert [i for i, (c, _) in enumerate(codes) if c == 256][:2] == [0, 3837]
    assert {w for _, w in codes} == {9, 10, 11, 12}
    check_u8(service, a, [s])


@pytest.mark.parametrize("every", [1, 63, 64, 65])
def test_lzw_clear_at_every_phase_of_a_round(service, every):
    a = smooth(5000).reshape(50, 100)
    codes = []
    s = T.lzw_encode(a.tobytes(), clear_every=every, codes_out=codes)
    assert sum(c == 256 for c, _ in codes) >= 5000 // (every * 4)
    check_u8(service, a, [s])


def test_lzw_clears_at_arbitrary_positions(service):
    a = smooth(5000, 4).reshape(50, 100)
    check_u8(service, a, [T.lzw_encode(a.tobytes(), clear_at=(1, 2, 3, 64, 65, 127, 129, 1000, 1001))])


def test_lzw_without_eoi_and_without_leading_clear(service):
    a = smooth(3000, 5).reshape(30, 100)
    with_eoi = T.lzw_encode(a.tobytes())
    no_eoi = T.lzw_encode(a.tobytes(), eoi=False)
    assert len(no_eoi) <= len(with_eoi) and no_eoi != with_eoi
    check_u8(service, a, [no_eoi])
    check_u8(service, a, [T.lzw_encode(a.tobytes(), leading_clear=False)])
    check_u8(service, a, [T.lzw_encode(a.tobytes(), leading_clear=False, eoi=False)])


def test_lzw_match_sources_beyond_the_ring(service):
    # a period-300 ramp of 64 KiB: strings named late in a run lie far more than 4 KiB back
    a = ((np.arange(65536) % 300) & 0xFF).astype(np.uint8).reshape(256, 256)
    check_u8(service, a, [T.lzw_encode(a.tobytes())])


def test_lzw_256_one_row_strips(service):
    a = smooth(256 * 100, 6).reshape(256, 100)
    check_u8(service, a, [T.lzw_encode(r.tobytes()) for r in a], seg_h=1)


def test_lzw_plane_one_pixel_wide(service):
    a = smooth(77, 7).reshape(77, 1)
    check_u8(service, a, [T.lzw_encode(a[y:y + 16].tobytes()) for y in range(0, 77, 16)], seg_h=16)


# -------------------------------------------------------------------------- un-predictor
INT_TYPES = [("i1", pbx.INT8), ("u1", pbx.UINT8), ("i2", pbx.INT16), ("u2", pbx.UINT16), ("i4", pbx.INT32),
             ("u4", pbx.UINT32)]
COMPS = [pbx.TIFF_NONE, pbx.TIFF_LZW, pbx.TIFF_DEFLATE]


@pytest.mark.parametrize("bo", ["<", ">"], ids=["II", "MM"])
@pytest.mark.parametrize("kind,pt", INT_TYPES, ids=[k for k, _ in INT_TYPES])
def test_unpredictor(service, kind, pt, bo):
    """Full-range random samples (every sum wraps), differenced by the helper in the file's byte
    order; the plane must hold the original samples."""
    dt = np.dtype(bo + kind) if kind[1] != "1" else np.dtype(kind)
    info = np.iinfo(dt)
    n = 2 * [k for k, _ in INT_TYPES].index(kind) + (bo == ">")  # the seed, and where the codecs' cycle starts
    rng = np.random.default_rng(n)
    specs, wants = [], []
    for w in (1, 63, 64, 65, 4097):
        layouts = [("strips", None, 5, 2)]
        if w in (63, 65):
            layouts += [("tiles", (16, 16), 37, None), ("tiles", (64, 64), 70, None)]
        for layout, tile, h, rps in layouts:
            a = rng.integers(info.min, info.max, (h, w), dtype=np.int64, endpoint=True).astype(dt)
            comp = COMPS[n % 3]
            n += 1
            segs = [T.compress(s, comp) for s in T.segments_of(a, tile, rps, predictor=2)]
            specs.append(dict(image_id=next(_ids), z=0, c=0, t=0, pixel_type=pt, size_x=w, size_y=h,
                              seg_w=tile[0] if tile else w, seg_h=tile[1] if tile else rps, tiled=tile is not None,
                              compression=comp, predictor=2, big_endian=bo == ">", segments=segs))
            wants.append(a.astype(dt.newbyteorder(">")).tobytes())
    assert {s["compression"] for s in specs} == set(COMPS)
    ids = service.register_tiff_planes(specs)
    try:
        for pid, want, sp in zip(ids, wants, specs):
            assert service.read_plane_be(pid, len(want)) == want, (sp["size_x"], sp["seg_w"], sp["compression"])
    finally:
        for pid in ids:
            service.release_plane(pid)


# ------------------------------------------------- round trip of the project's own writer
@pytest.mark.parametrize("deflate", [True, False], ids=["deflate", "stored"])
def test_reads_its_own_tiff_output(tmp_path, deflate):
    with pbx.PixelsService(tiff_deflate=deflate, tiff_tile=64,
                           tiff_predictor=pbx.TIFF_PREDICTOR_HORIZONTAL) as svc:
        svc.register_plane(1, 0, 0, 0, pbx.UINT16, 700, 500, generator="noise", seed=3)
        svc.register_plane(2, 0, 0, 0, pbx.INT8, 300, 200, generator="fake", seed=1)
        for image, (x, y, w, h) in ((1, (37, 61, 200, 130)), (2, (5, 9, 64, 64))):
            st, tif = svc.get_tile(pbx.TileCtx(image, 0, 0, 0, x, y, w, h, format="tif"))
            assert st == 0
            path = str(tmp_path / ("own%d.tif" % image))
            with open(path, "wb") as f:
                f.write(tif)
            d = pbx.tiff_ifds(path)[0]
            if deflate:
                assert d["tiled"] and d["predictor"] == 2 and d["compression"] in (8, 32946)
            back = next(_ids)
            ids = svc.register_tiff_image(path, back)
            assert list(ids) == [0] and list(ids[0]) == [(0, 0, 0)]
            assert raw_tile(svc, back, 0, 0, 0, 0, 0, w, h) == raw_tile(svc, image, 0, 0, 0, x, y, w, h)


# ------------------------------------------------------------------ many planes, one call
def test_many_planes_in_one_call(service):
    ome = next(e for e in FILES if "ome" in e)
    other = next(e for e in FILES if e["file"] == "uint16_tiles_deflate_p2_MM.tif")
    specs, wants = [], []
    for entry in (ome, other):
        path = os.path.join(GOLD, entry["file"])
        lay = pbx.tiff_image_layout(path)
        image = next(_ids)
        for (z, c, t), ifd in zip(lay["planes"], lay["ifds"]):
            specs.append(pbx.tiff_plane_spec(path, ifd, image, z, c, t))
            wants.append(expected(entry, "0", "%d,%d,%d" % (z, c, t)).tobytes())
    assert len(specs) == 13
    ids, ms = service.register_tiff_planes(specs, timing=True)
    try:
        assert len(set(ids)) == 13 and ms[0] > 0 and ms[1] > 0
        for pid, want in zip(ids, wants):
            assert service.read_plane_be(pid, len(want)) == want
    finally:
        for pid in ids:
            service.release_plane(pid)


# ------------------------------------------------------------------------ corrupt streams
def bad_code_stream():
    b = T._Bits()
    for v in (256, 65, 66, 300):  # entry 300 does not exist yet: the next free code is 260
        b.put(v, 9)
    b.put(257, 9)
    return b.done()


@pytest.mark.parametrize("case", ["code above the next free code", "truncated mid-code", "one byte short",
                                  "wrong adler32"])
def test_corrupt_streams_register_nothing(service, case):
    a = smooth(4 * 8 * 100, 8).reshape(32, 100)
    strips = [a[y:y + 8].tobytes() for y in range(0, 32, 8)]
    comp = pbx.TIFF_DEFLATE if case == "wrong adler32" else pbx.TIFF_LZW
    segs = [T.compress(s, comp) for s in strips]
    if case == "code above the next free code":
        segs[2] = bad_code_stream()
    elif case == "truncated mid-code":
        segs[2] = segs[2][:len(segs[2]) // 2]
    elif case == "one byte short":
        segs[2] = T.lzw_encode(strips[2][:-1])
    else:
        segs[2] = segs[2][:-1] + bytes([segs[2][-1] ^ 0x55])
    keep_image = next(_ids)
    keep = service.register_plane(keep_image, 0, 0, 0, pbx.UINT8, 64, 64, generator="noise", seed=1)
    before = service.residency_stats()
    image = next(_ids)
    good = u8_plane(next(_ids), 100, 32, [T.lzw_encode(s) for s in strips], seg_h=8)
    bad = dict(u8_plane(image, 100, 32, segs, seg_h=8), compression=comp)
    try:
        with pytest.raises(pbx.PbxError, match="corrupt chunk stream") as e:
            service.register_tiff_planes([good, bad])
        assert e.value.status == 400
        after = service.residency_stats()
        assert (after["planes"], after["resident_bytes"]) == (before["planes"], before["resident_bytes"])
        assert service.lookup_plane(image, 0, 0, 0) is None
        assert service.lookup_plane(good["image_id"], 0, 0, 0) is None
        st, body = service.get_tile(pbx.TileCtx(keep_image, 0, 0, 0, 0, 0, 16, 16))
        assert st == 0 and len(body) == 256
        # and the same planes load once the stream is whole
        bad["segments"] = [T.lzw_encode(s) for s in strips]
        bad["compression"] = pbx.TIFF_LZW
        ids = service.register_tiff_planes([good, bad])
        assert all(service.read_plane_be(p, a.size) == a.tobytes() for p in ids)
        for p in ids:
            service.release_plane(p)
    finally:
        service.release_plane(keep)


# k_tiff_lzw's refusal codes (kernels_tiff_src.hip): 1 fewer bytes than dlen, 2 a code beyond the
# next free one, 3 a string past dlen, 4 no Clear before the table is full.  Raw code values
# after a Clear; the plane is one strip of `n` bytes.
def _lzw_refusals():
    lit = [int(v) for v in smooth(4000, 9)]
    return {
        "EOI before dlen": (T.lzw_pack([65, 66, 67, T.EOI]), 300, 1),
        # code 2 of a round names entry 10, which code 11 of the same round would define
        "code above the next free one, in the round that would define it":
            (T.lzw_pack(lit[:2] + [T.FIRST + 10] + lit[3:100] + [T.EOI]), 300, 2),
        # code 70, in the second round of 64, names entry 100
        "code above the next free one, in a later round":
            (T.lzw_pack(lit[:70] + [T.FIRST + 100] + lit[71:200] + [T.EOI]), 300, 2),
        # entry 258 = "AB": the fifth code's two bytes end one past the five of the strip
        "string past dlen mid-round": (T.lzw_pack([65, 66, 67, 68, T.FIRST, T.EOI]), 5, 3),
        "3838 codes without a Clear and then no Clear": (T.lzw_pack(lit[:T.RUN_MAX + 2] + [T.EOI]), 4000, 4),
    }


@pytest.mark.parametrize("case", list(_lzw_refusals()))
def test_lzw_refusal_names_its_decoder_code(service, case):
    stream, n, code = _lzw_refusals()[case]
    # the table-based decoder refuses the same streams: an error, or fewer bytes than the strip;
    # code 3 is the exception: it decodes the whole string and merely cuts it at `expect`
    try:
        short = len(T.lzw_decode(stream, n)) < n
    except ValueError:
        short = True
    assert short == (code != 3)
    if code == 3:
        assert len(T.lzw_decode(stream)) > n
    image = next(_ids)
    with pytest.raises(pbx.PbxError) as e:
        service.register_tiff_planes([u8_plane(image, n, 1, [stream])])
    assert e.value.status == 400 and "(lzw, decoder code %d)" % code in str(e.value), str(e.value)
    assert service.lookup_plane(image, 0, 0, 0) is None
    a = smooth(n, 10).reshape(1, n)
    check_u8(service, a, [T.lzw_encode(a.tobytes())])


# ------------------------------------------------------- TiffSource behind the handler
def test_tiff_source_behind_the_handler():
    entry = next(e for e in FILES if e["file"].startswith("pyramid"))
    path = os.path.join(GOLD, entry["file"])
    full = expected(entry, "0")
    lv2 = expected(entry, "2")
    with pbx.PixelsService() as svc:
        src = pbx.TiffSource({41: path})
        cold = svc.residency_stats()["planes"]
        # format=jpg on a cold image: the reference answers null before it opens anything
        assert pbx.TileRequestHandler(svc, pbx.TileCtx(41, 0, 0, 0, 0, 0, 16, 16, format="jpg"), src).get_tile() is None
        assert svc.residency_stats()["planes"] == cold
        assert pbx.TileRequestHandler(svc, pbx.TileCtx(42, 0, 0, 0, 0, 0, 16, 16), src).get_tile() is None
        assert svc.residency_stats()["planes"] == cold
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(41, 0, 0, 0, 10, 20, 100, 60), src).get_tile()
        assert body == full[20:80, 10:110].tobytes()
        assert svc.residency_stats()["planes"] == cold + 1  # one load: the requested plane, whole
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(41, 0, 0, 0, 0, 0, 30, 20), src).get_tile()
        assert body == full[:20, :30].tobytes() and svc.residency_stats()["planes"] == cold + 1
        # stored level 2 is OMERO resolution 0
        body = pbx.TileRequestHandler(svc, pbx.TileCtx(41, 0, 0, 0, 3, 2, 30, 20, resolution=0), src).get_tile()
        assert body == lv2[2:22, 3:33].tobytes()
        status, payload, headers = pbx.handle_get_tile(svc, pbx.TileCtx(41, 0, 0, 0, 0, 0, 8, 8).to_json(), src)
        assert status == 200 and payload == full[:8, :8].tobytes()
        status, _, _ = pbx.handle_get_tile(svc, pbx.TileCtx(43, 0, 0, 0, 0, 0, 8, 8).to_json(), src)
        assert status == 404
