"""JPEG 2000 TIFF segments with quality layers, precincts and SOP / EPH markers
(PBX_TIFF_F_J2K_PACKETS; DESIGN.md section 10b "Layers, precincts and packet markers") without a
GPU: tests/_tiff_j2k_packets.py's model against PIL (OpenJPEG) and the encoder's input; the planner
through pbx_test_tiff_j2k_plan; the device's own packet walker and gather arithmetic run on the CPU
through pbx_test_tiff_j2k_decode; and the Python layer's keyword."""
import functools

import numpy as np
import pytest

import _tiff_j2k as J
import _tiff_j2k97 as J97
import _tiff_j2k_packets as K
import pbx

PROGRESSIONS = K.PROGRESSIONS
RATES = {1: [0], 2: [12, 0], 3: [8, 3, 0], 8: [60, 40, 25, 15, 10, 6, 3, 0]}
# (precinct_size, codeblock_size, the code-block size the COD is rewritten to say).  PIL's encoder
# declares precincts only from twice the block size up, and halves them from resolution to
# resolution, so (16, 16) over 8 x 8 has precincts smaller than the block at its low resolutions
# (B.7: the block is clipped) and the third and fourth case come out without precincts: they stay
# for what the encoder then writes.  The last case is the fourth as it was meant: the second's
# stream with its COD saying 16 x 16 blocks, which the 16 x 16 precincts (8 x 8 in a band) clip
# back to the 8 x 8 the encoder wrote, at every resolution; PIL reads the rewritten bytes alike.
# (Not with 0 levels, where the one resolution's precinct is 16 x 16 in its band.)
PRECINCTS = [(None, (8, 8), None), ((16, 16), (8, 8), None), ((32, 32), (32, 32), None), ((8, 8), (16, 16), None),
             ((16, 16), (8, 8), (16, 16))]


def pt_of(a):
    return pbx.UINT8 if a.dtype == np.uint8 else pbx.UINT16


def encode(a, layers, precinct, cb, says=None, **kw):
    kw = dict(kw, codeblock_size=cb, quality_mode="rates", quality_layers=RATES[layers])
    if precinct:
        kw["precinct_size"] = precinct
    s = J.encode(a, **kw)
    if says and K.parse(s)["levels"]:  # (with no levels resolution 0 keeps the whole 16 x 16: nothing clips)
        s = J.patch(J.patch(s, 0x52, 6, says[0].bit_length() - 3), 0x52, 7, says[1].bit_length() - 3)
    return s


def check(a, s):
    """the CPU hook == the model == PIL == the array, and the planner's counts are the model's."""
    spp = 1 if a.ndim == 2 else 3
    assert np.array_equal(J.pil_decode(s), a)
    assert np.array_equal(K.decode(s), a), a.shape
    rc, msg, got = K.cpu_decode(*K.one(s, a), a.dtype.type, spp)
    assert rc == 0 and np.array_equal(got, K.planes(a)), (a.shape, msg)
    rc, msg, out = K.plan(*K.one(s, a), pt_of(a), spp)
    assert rc == 0 and out == [1] + list(K.counts(s)), (out, K.counts(s), msg)


def image(kind, w, h, seed):
    if kind == "u8":
        return K.noise(w, h, seed), {}
    if kind == "u16":
        return K.smooth(w, h, seed, np.uint16), {}
    return K.smooth(w, h, seed, np.uint8, samples=3), dict(mct=1 if kind == "rct" else 0)


# ------------------------------------------------------------------------------ reversible
@pytest.mark.parametrize("layers", [1, 2, 3, 8])
def test_layers_precincts_levels_progressions(layers):
    """Every combination of precincts, levels and progression; the pixel kind and the size rotate."""
    n = 0
    for precinct, cb, says in PRECINCTS:
        for levels in range(5):
            for prog in PROGRESSIONS:
                n += 1
                kind = ("u8", "u16", "rgb", "rct")[n % 4]
                a, kw = image(kind, 33 + n % 3, 19 + n % 5, n)
                s = encode(a, layers, precinct, cb, says, num_resolutions=levels + 1, progression=prog, **kw)
                h = K.parse(s)
                assert h["layers"] == layers and h["prog"] == PROGRESSIONS.index(prog)
                assert bool(h["scod"] & 1) == bool(precinct and precinct[0] >= 2 * cb[0])
                if h["scod"] & 1:
                    assert h["pp"][-1] == (precinct[0].bit_length() - 1,) * 2
                if says and levels:
                    assert 1 << h["xcb"] == says[0] and all(b["cbw"] <= 8 for b in K.geometry(h)[0])
                check(a, s)


def test_small_images():
    """Widths 1 .. 18 x heights 1 .. 17: empty sub-bands, resolutions of one row or column,
    precincts of one sample.  Kinds, layers, precincts, levels and progressions rotate."""
    n = 0
    for w in range(1, 19):
        for h in range(1, 18):
            n += 1
            kind = ("u8", "u16", "rgb", "rct")[n % 4]
            a, kw = image(kind, w, h, n)
            precinct, cb, says = PRECINCTS[(n // 4) % 5]
            s = encode(a, (1, 2, 3, 8)[(n // 3) % 4], precinct, cb, says, num_resolutions=1 + n % 5, progression=PROGRESSIONS[n % 5], **kw)
            check(a, s)


def test_blocks_clipped_to_precincts():
    """B.7 at every resolution but the top one, and a 64 x 64 block grid that precincts cut."""
    a = K.smooth(50, 40, 3, np.uint16)
    s = encode(a, 3, (32, 32), (16, 16), num_resolutions=4)
    bands = K.geometry(K.parse(s))[0]
    assert K.parse(s)["pp"] == [(2, 2), (3, 3), (4, 4), (5, 5)] and sorted({b["cbw"] for b in bands}) == [4, 8, 16]
    check(a, s)
    s = encode(a, 2, (16, 16), (8, 8), num_resolutions=5)  # resolution 0: precincts of 1 x 1 (PPx = PPy = 0)
    assert K.parse(s)["pp"][0] == (0, 0) and K.geometry(K.parse(s))[0][0]["cbw"] == 1
    check(a, s)


# The fixture of the six conditions: 65 x 33 uint16, K.smooth seed 1, rates 8 / 3 / lossless,
# 16 x 16 precincts over 8 x 8 blocks, 4 resolutions.  (Seeds 1 and 3 satisfy all six, seed 2 misses
# the Lblock growth; 40 x 24 images have no empty precinct: 65 = 4 * 16 + 1 gives the HL and HH bands
# of the top resolution a precinct column that misses them.)
FIX_W, FIX_H, FIX_SEED = 65, 33, 1


@functools.lru_cache(maxsize=None)
def fixture(prog="RPCL"):
    a = K.smooth(FIX_W, FIX_H, FIX_SEED, np.uint16)
    return a, encode(a, 3, (16, 16), (8, 8), num_resolutions=4, progression=prog)


@pytest.mark.parametrize("prog", PROGRESSIONS)
def test_the_fixture_exercises_the_walker(prog):
    a, s = fixture(prog)
    f = K.facts(s)
    assert f["several"], "no block has contributions in two layers"
    assert f["late"], "no block is first included after layer 0"
    assert f["skipped"], "no included block is skipped in a later layer"
    assert f["lblock_grows"], "no block's Lblock grows after its first inclusion"
    assert f["partial_precinct"], "no resolution has a partial last precinct column and row"
    assert f["empty_precinct"], "no band has an empty precinct"
    check(a, s)


# ------------------------------------------------------------------------------ irreversible
@pytest.mark.parametrize("kind", ["u8", "u16", "rct"])
@pytest.mark.parametrize("precinct", [None, (16, 16)])
def test_irreversible_layers(kind, precinct):
    a, kw = image(kind, 40, 24, 21)
    kw = dict(kw, num_resolutions=4, codeblock_size=(8, 8), quality_mode="dB", quality_layers=[30, 40, 50])
    if precinct:
        kw["precinct_size"] = precinct
    s = J97.encode(a, **kw)
    h = K.parse(s)
    assert h["transform"] == 0 and h["layers"] == 3 and bool(h["scod"] & 1) == bool(precinct)
    assert K.facts(s)["several"]
    spp, prec = (1 if a.ndim == 2 else 3), 8 * a.dtype.itemsize
    rc, msg, got = K.cpu_decode(*K.one(s, a), a.dtype.type, spp)
    assert rc == 0, msg
    got = got[0] if spp == 1 else np.moveaxis(got, 0, 2)
    # the float32 model follows the library's order of operations: bit for bit
    assert np.array_equal(J97.rint(K.decode_real(s, np.float32), prec), got)
    ok, _, outside = J97.close(got, K.decode_real(s), J97.window(prec), prec)
    assert ok, outside
    d = int(np.abs(J.pil_decode(s).astype(np.int64) - got.astype(np.int64)).max())
    assert d <= (1 if prec == 8 else 3), d
    rc, msg, out = K.plan(*K.one(s, a), pt_of(a), spp)
    assert rc == 0 and out == [1] + list(K.counts(s)), (out, K.counts(s), msg)


# ------------------------------------------------------------------------------ SOP / EPH
@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("sop,eph", [(True, False), (False, True), (True, True)])
def test_sop_and_eph(layers, sop, eph):
    a = K.smooth(40, 24, 5, np.uint16)
    for prog in ("LRCP", "RPCL", "CPRL"):
        s = encode(a, layers, (16, 16), (8, 8), num_resolutions=4, progression=prog)
        t = K.insert_sop_eph(s, sop, eph)
        assert len(t) > len(s) and K.parse(t)["scod"] & 6 == (2 if sop else 0) | (4 if eph else 0)
        check(a, t)  # (PIL on the rewritten bytes is the judge)


def test_sop_bit_without_markers_and_missing_eph():
    a, s = fixture()
    check(a, K.set_scod(s, 2))  # the SOP bit allows the marker, no packet has to carry one
    some = K.insert_sop_eph(s, True, False, skip_sop_of=range(1, 200, 2))
    check(a, some)
    n = len(K.walk(s)[3])
    for k in (0, n // 2, n - 1):
        bad = K.insert_sop_eph(s, False, True, skip_eph_of=k)
        rc, msg, _ = K.cpu_decode(*K.one(bad, a), np.uint16, 1)
        assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code 2)" in msg, (k, msg)
        with pytest.raises(ValueError, match="malformed packet header"):
            K.decode(bad)


# ------------------------------------------------------------------------------ refusals
def test_layer_bounds():
    a, s = fixture()
    q = J.find_marker(s, 0x52) + 4 + 2
    for n, text in ((65, "65 quality layers (1 .. 64)"), (0, "0 quality layers (1 .. 64)"), (300, "300 quality layers (1 .. 64)")):
        bad = s[:q] + bytes([n >> 8, n & 255]) + s[q + 2:]
        for rc, msg, _ in (K.plan(*K.one(bad, a), pbx.UINT16, 1), K.cpu_decode(*K.one(bad, a), np.uint16, 1)):
            assert rc == 400 and text in msg and "segment 0" in msg, msg
    # 64 are taken: the stream's own three, then 61 layers of packets that are not there
    many = s[:q] + bytes([0, 64]) + s[q + 2:]
    assert K.plan(*K.one(many, a), pbx.UINT16, 1)[0] == 0


def test_every_prefix_of_two_headers_is_a_400():
    a, s = fixture()
    rgb = K.smooth(40, 24, 10, np.uint8, samples=3)
    t = K.insert_sop_eph(encode(rgb, 2, (32, 32), (16, 16), num_resolutions=4, mct=1, progression="PCRL"), True, True)
    for good, im in ((s, a), (t, rgb)):
        end = K.parse(good)["data"]
        for cut in range(end):
            rc, msg, _ = K.plan([good[:cut]] if cut else [b"\x00"], *K.one(good, im)[1:], pt_of(im), 1 if im.ndim == 2 else 3)
            assert rc == 400, (cut, msg)
        rc, msg, _ = K.plan([good[:end]], *K.one(good, im)[1:], pt_of(im), 1 if im.ndim == 2 else 3)
        assert rc == 0, msg
        rc, msg, _ = K.cpu_decode([good[:end]], *K.one(good, im)[1:], im.dtype.type, 1 if im.ndim == 2 else 3)
        assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code 1)" in msg


def test_remaining_refusals_keep_their_texts():
    """Every refusal the existing file pins that the flag does not lift, with the flag set; and
    the three it lifts, with the flag clear."""
    import test_tiff_j2k_host as T
    lifted = {"layers", "sop", "eph"}
    for name, stream, text in T.REFUSALS:
        spp = 3 if stream[2:].startswith(T.RGB[2:8]) and name in ("rgb16", "subsampled") else 1
        pt, dt = (pbx.UINT8, np.uint8) if spp == 3 else (pbx.UINT16, np.uint16)
        for flags in (0, K.FLAG):
            rc, msg, _ = K.plan([stream], T.W0, T.H0, T.W0, T.H0, False, pt, spp, flags=flags)
            rc2, msg2, _ = K.cpu_decode([stream], T.W0, T.H0, T.W0, T.H0, False, dt, spp, flags=flags)
            if flags and name in lifted:
                assert rc == 0, msg  # (the header passes; what the packets then hold is the device's to say)
                assert rc2 == 0 or "decoder code" in msg2, msg2
            else:
                assert rc == 400 and text in msg and "segment 0" in msg, (name, msg)
                assert rc2 == 400 and text in msg2, (name, msg2)
    a = K.noise(T.W0, T.H0, 9, np.uint16)
    many = J.encode(a, num_resolutions=3, precinct_size=(16, 16), codeblock_size=(8, 8))
    assert "more than one precinct in resolution 0" in K.plan(*K.one(many, a), pbx.UINT16, 1, flags=0)[1]
    assert K.plan(*K.one(many, a), pbx.UINT16, 1)[0] == 0
    assert "2 quality layers (1)" in K.plan(*K.one(J.patch(T.GOOD, 0x52, 3, 2), a), pbx.UINT16, 1, flags=0)[1]
    assert "SOP or EPH markers (Scod 0x02)" in K.plan(*K.one(J.patch(T.GOOD, 0x52, 0, 2), a), pbx.UINT16, 1, flags=0)[1]
    # the flag belongs to the JPEG 2000 calls; any other bit is refused there too
    import ctypes
    s, keep = K.segments_struct([T.GOOD], T.W0, T.H0, False, flags=K.FLAG)
    out = (ctypes.c_uint64 * 4)()
    assert pbx.lib().pbx_test_tiff_plan(ctypes.byref(s), T.W0, T.H0, 2, out) == 400
    for flags in (2, 3, 0x100, -1):
        rc, msg, _ = K.plan([T.GOOD], T.W0, T.H0, T.W0, T.H0, False, pbx.UINT16, 1, flags=flags)
        assert rc == 400 and msg == "bad flags 0x%x" % (flags & 0xFFFFFFFF), msg


# ------------------------------------------------------------------------------ device codes
def test_device_codes_on_the_cpu():
    a, s = K.device_case()
    hdr_cut, data_cut = K.layer2_cuts(s)
    for cut in (hdr_cut, data_cut):
        rc, msg, _ = K.cpu_decode(*K.one(s[:cut], a), np.uint16, 1)
        assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code 1)" in msg, (cut, msg)
    bad = K.passes_overflow_in_the_sum(s)
    rc, msg, _ = K.cpu_decode(*K.one(bad, a), np.uint16, 1)
    assert rc == 400 and "decoder code 3" in msg, msg
    with pytest.raises(ValueError, match="more passes than the bit-planes allow"):
        K.decode(bad)


def test_flipped_bits_are_decoded_or_refused():
    a, s = K.flip_case()
    codes = {}
    for bad in K.flipped(s, 200, 11):
        rc, msg, _ = K.cpu_decode(*K.one(bad, a), np.uint16, 1)
        assert rc == 0 or (rc == 400 and "corrupt segment stream 0 (j2k, decoder code" in msg), msg
        codes[msg[-2:-1] if rc else "0"] = codes.get(msg[-2:-1] if rc else "0", 0) + 1
    assert codes.get("0") and len(codes) >= 3, codes  # decoded, and refused for more than one reason


# ------------------------------------------------------------------------------ the Python layer
def test_python_keyword(tmp_path):
    a, s = fixture()
    pg = dict(J.page_of(a, 33003, num_resolutions=3), segments=[s])
    path = str(tmp_path / "layered.tif")
    J.write_tiff(path, [pg])
    ifd = pbx.tiff_ifds(path)[0]
    with pytest.raises(pbx.PbxError, match="3 quality layers \\(1\\)") as e:
        pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0)
    assert e.value.status == 400
    with pytest.raises(pbx.PbxError, match="3 quality layers \\(1\\)"):
        pbx.tiff_band_spec(path, ifd, 0, 8)
    with pytest.raises(pbx.PbxError, match="3 quality layers \\(1\\)"):
        pbx.tiff_image_layout(path)
    sp = pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_packets=True)
    assert sp["flags"] == pbx.TIFF_F_J2K_PACKETS == 1 and sp["j2k"] is True
    bd = pbx.tiff_band_spec(path, ifd, 0, 8, j2k_packets=True)
    assert bd["flags"] == 1 and bytes(bd["segments"][0]) == s
    assert pbx.tiff_image_layout(path, j2k_packets=True)["pixel_type"] == pbx.UINT16
    # one layer, several precincts; SOP / EPH
    one_layer = encode(a, 1, (16, 16), (8, 8), num_resolutions=4)
    for stream, text in ((one_layer, "more than one precinct in resolution 0"),
                         (K.insert_sop_eph(one_layer, True, True), "SOP or EPH markers")):
        J.write_tiff(path, [dict(pg, segments=[stream])])
        ifd = pbx.tiff_ifds(path)[0]
        with pytest.raises(pbx.PbxError, match=text):
            pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0)
        assert pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_packets=True)["flags"] == 1
    # what stays refused with the keyword, in the same words
    q = J.find_marker(s, 0x52) + 4 + 2
    for stream, text in ((s[:q] + bytes([0, 65]) + s[q + 2:], "65 quality layers \\(1 .. 64\\)"),
                         (J.patch(s, 0x52, 8, 1), "code-block style 0x01")):
        J.write_tiff(path, [dict(pg, segments=[stream])])
        with pytest.raises(pbx.PbxError, match=text):
            pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0, j2k_packets=True)
    # a file that is not JPEG 2000 carries no flags, keyword or not
    from PIL import Image
    plain = str(tmp_path / "plain.tif")
    Image.fromarray(a).save(plain)
    assert "flags" not in pbx.tiff_plane_spec(plain, pbx.tiff_ifds(plain)[0], 1, 0, 0, 0, j2k_packets=True)


def test_the_serving_path_accepts_by_default(tmp_path):
    """TiffSource hands over flagged specs by default (register_tiff_image's default is covered on
    the GPU: it registers)."""
    a, s = fixture()
    path = str(tmp_path / "layered.tif")
    J.write_tiff(path, [dict(J.page_of(a, 33003, num_resolutions=3), segments=[s])])
    src = pbx.TiffSource({7: path})
    px = src.get_pixels(7)
    assert (px.size_x, px.size_y) == (FIX_W, FIX_H)
    assert src.plane_segments(px, 0, 0, 0, 0)["flags"] == 1
    assert src.band_segments(px, 0, 0, 0, 0, 0, 8)["flags"] == 1
    with pytest.raises(pbx.PbxError, match="3 quality layers \\(1\\)"):
        pbx.TiffSource({7: path}, j2k_packets=False).get_pixels(7)
    import inspect
    assert inspect.signature(pbx.PixelsService.register_tiff_image).parameters["j2k_packets"].default is True
    assert inspect.signature(pbx.tiff_plane_spec).parameters["j2k_packets"].default is False
    assert inspect.signature(pbx.tiff_band_spec).parameters["j2k_packets"].default is False


# ------------------------------------------------------------------------------ re-cut streams
def test_recut_streams():
    """K.relayer's streams (the GPU tests' gather cases): contributions of 0, 1, 63, 64, 65 and 129
    bytes, PIL reading the re-cut bytes to the same pixels."""
    for size, res in ((64, 1), (128, 2)):
        a = K.noise(size, size, size)
        for prog in PROGRESSIONS:
            t = K.relayer(J.encode(a, num_resolutions=res, codeblock_size=(64, 64), progression=prog), 8, K.wave_edges)
            L = K.facts(t)["lengths"]
            assert 0 in L and 1 in L and any(60 <= n <= 68 for n in L) and any(n > 128 for n in L), L
            assert K.facts(t)["lblock_grows"]
            check(a, t)
    a = K.smooth(65, 33, 1)
    t = K.relayer(J.encode(a, num_resolutions=4, codeblock_size=(8, 8), precinct_size=(16, 16), progression="PCRL"), 3, K.thirds)
    f = K.facts(t)
    assert f["several"] and f["late"] and f["skipped"] and 0 in f["lengths"]
    check(a, t)
    check(a, K.insert_sop_eph(t, True, True))
