"""JPEG 2000 TIFF segments with subsampled chroma (PBX_TIFF_F_J2K_SUBSAMPLED) and YCbCr components
outside the codestream (PBX_TIFF_F_J2K_YCBCR) on the CPU: the planner (per-component sizes, the
position loops with sampling factors) and the CPU decode hook, which places with the functions
k_tiff_j2k_place_chroma runs (tiff_j2k_dev.h), and the Python layer's keywords.

The streams are merged from three single-component PIL streams (tests/_tiff_j2k_chroma.py), so the
right answer of a reversible stream is the three inputs, the chroma replicated, and with the
YCbCr flag tests/_tiff_jpeg.py's ycc_to_rgb of them; an irreversible stream's components are held
to the float64 model of their own single-component streams by J97.close."""
import inspect
import os

import numpy as np
import pytest

import _tiff_j2k as J
import _tiff_j2k97 as J97
import _tiff_j2k_chroma as C
import _tiff_j2k_packets as K
import pbx
from _tiff_jpeg import ycc_to_rgb

SUB, YCC, PK = pbx.TIFF_F_J2K_SUBSAMPLED, pbx.TIFF_F_J2K_YCBCR, pbx.TIFF_F_J2K_PACKETS
SMALL = dict(precinct_size=(16, 16), codeblock_size=(8, 8))


def test_the_flags_values():
    assert (PK, SUB, YCC) == (1, 4, 8) == (C.F_PACKETS, C.F_SUB, C.F_YCC)


def comps(w, h, xs, ys, seed, kind="smooth"):
    a = C.ycc_smooth(w, h, seed) if kind == "smooth" else C.ycc_noise(w, h, seed)
    return a[:, :, 0], C.sub(a[:, :, 1], xs, ys), C.sub(a[:, :, 2], xs, ys)


def decode(stream, w, h, flags):
    rc, msg, out = K.cpu_decode([stream], w, h, w, h, False, np.uint8, 3, flags=flags)
    assert rc == 0, msg
    return np.moveaxis(out, 0, 2)


def check(y, cb, cr, xs, ys, merged, singles, flags, what):
    """The hook's planes with and without the YCbCr flag, and the planner's counts."""
    h, w = y.shape
    got = decode(merged, w, h, flags)
    rgb = decode(merged, w, h, flags | YCC)
    if K.parse(merged)["transform"] == 1:
        assert np.array_equal(got, C.planes(y, cb, cr, xs, ys, False)), what
        assert np.array_equal(rgb, C.planes(y, cb, cr, xs, ys, True)), what
    else:
        m = C.model(singles, xs, ys)
        for c in range(3):
            ok, inside, bad = J97.close(got[:, :, c], m[:, :, c], J97.WINDOW8, 8)
            assert ok, (what, c, inside, bad)
        assert np.array_equal(rgb, ycc_to_rgb(got[:, :, 0], got[:, :, 1], got[:, :, 2])), what
    for f in (flags, flags | YCC):
        rc, msg, out = K.plan([merged], w, h, w, h, False, pbx.UINT8, 3, flags=f)
        assert rc == 0 and (out[0], out[1], out[2], out[3]) == (1,) + C.counts(singles), (what, msg, out, C.counts(singles))


# ------------------------------------------------------------------------------ the sweep
WIDTHS, HEIGHTS = (1, 2, 3, 16, 17, 33, 40), (1, 2, 3, 16, 23)


@pytest.mark.parametrize("xs,ys", C.FACTORS, ids=["2x1", "1x2", "2x2"])
def test_shape_sweep(xs, ys):
    """Every width x height x factor pair, one precinct per resolution (flags 4 and 4 | 8): 0 .. 3
    levels as the sizes allow, 4 x 4 and 32 x 32 blocks, the five progressions rotating; 5/3 on all
    shapes, 9/7 on every fourth."""
    n = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            n += 1
            kw = dict(num_resolutions=1 + (w + 2 * h + xs) % 4, codeblock_size=(4, 4) if n % 2 else (32, 32),
                      progression=K.PROGRESSIONS[n % 5])
            y, cb, cr = comps(w, h, xs, ys, 1000 * xs + 100 * w + h, "noise" if n % 3 == 0 else "smooth")
            for irr in ([False, True] if n % 4 == 0 else [False]):
                merged, singles = C.encode(y, cb, cr, xs, ys, irr, **kw)
                hd = K.parse(merged)
                assert hd["levels"] == C.num_resolutions(w, h, xs, ys, kw["num_resolutions"]) - 1
                check(y, cb, cr, xs, ys, merged, singles, SUB, (w, h, xs, ys, irr, kw))
                # such a stream needs no packet list, and takes one
                assert np.array_equal(decode(merged, w, h, SUB | PK), decode(merged, w, h, SUB))


def test_the_sweep_reaches_every_level_count_and_odd_chroma_sizes():
    levels = {C.num_resolutions(w, h, xs, ys, 1 + (w + 2 * h + xs) % 4) - 1 for w in WIDTHS for h in HEIGHTS for xs, ys in C.FACTORS}
    assert levels == {0, 1, 2, 3}
    assert J.cdiv(17, 2) == 9 and J.cdiv(33, 2) == 17 and J.cdiv(23, 2) == 12 and J.cdiv(3, 2) == 2 and J.cdiv(1, 2) == 1


# ------------------------------------------------------------------------------ packets
@pytest.mark.parametrize("prog", ["RPCL", "PCRL", "CPRL", "LRCP", "RLCP"])
@pytest.mark.parametrize("w,h", [(40, 24), (37, 23)])
def test_precincts_with_subsampling(w, h, prog):
    """Flags 1 | 4 | 8: 16 x 16 precincts over 8 x 8 blocks, where the position loops of B.12.1.3 -
    5 must step with XRsiz 2^(PPx + NL - r): a chroma precinct lies twice as far along the
    reference grid as the luma precinct of the same index."""
    for xs, ys in C.FACTORS:
        y, cb, cr = comps(w, h, xs, ys, 7 * w + xs + 2 * ys)
        merged, singles = C.encode(y, cb, cr, xs, ys, num_resolutions=3, progression=prog, **SMALL)
        hd = K.parse(merged)
        assert hd["scod"] & 1 and hd["pp"][-1] == (4, 4) and hd["prog"] == K.PROGRESSIONS.index(prog)
        _, geo, _, pk = K.walk(singles[1])
        assert max(p["px"] for p in pk) >= 1 or max(p["py"] for p in pk) >= 1  # the chroma has several precincts too
        check(y, cb, cr, xs, ys, merged, singles, PK | SUB, (w, h, xs, ys, prog))


def test_the_order_differs_from_the_unsampled_one():
    """The fixture is not vacuous: with the chroma's factors ignored the position loops would give
    another order of packets."""
    y, cb, cr = comps(40, 24, 2, 2, 3)
    merged, singles = C.encode(y, cb, cr, 2, 2, num_resolutions=3, progression="PCRL", **SMALL)
    precs = [K.walk(s)[1][3] for s in singles]
    h = K.parse(singles[0])
    assert C.packet_order(h, precs, [(1, 1), (2, 2), (2, 2)]) != C.packet_order(h, precs, [(1, 1)] * 3)


def halves(key, passes, n):
    """K.relayer split over 2 layers: the first pass and a third of the bytes, then the rest."""
    return [(1, n // 3), (passes - 1, n - n // 3)] if passes > 1 else [(0, 0), (passes, n)]


def three(key, passes, n):
    """... over 3 layers: a pass and a quarter of the bytes in each of the first two, then the rest
    (a block of fewer than three passes: all in the first)."""
    return [(1, n // 4), (1, n // 4), (passes - 2, n - 2 * (n // 4))] if passes >= 3 else [(passes, n), (0, 0), (0, 0)]


@pytest.mark.parametrize("layers,split", [(2, halves), (3, three)], ids=["2", "3"])
def test_layers_through_relayer(layers, split):
    for (xs, ys), prog in zip(C.FACTORS, ("RPCL", "PCRL", "CPRL")):
        y, cb, cr = comps(40, 24, xs, ys, 31 + xs)
        merged, singles = C.encode(y, cb, cr, xs, ys, layers=(layers, split), num_resolutions=3, progression=prog, **SMALL)
        assert K.parse(merged)["layers"] == layers
        check(y, cb, cr, xs, ys, merged, singles, PK | SUB, (xs, ys, prog, layers))
    if layers == 3:  # Pillow reads the re-cut, merged stream to the same pixels (even sizes)
        want = C.planes(y, cb, cr, xs, ys, True).astype(np.int64)
        assert np.abs(J.pil_decode(merged).astype(np.int64) - want).max() <= 1


def test_sop_and_eph():
    for (xs, ys), prog in zip(C.FACTORS, ("CPRL", "RPCL", "LRCP")):
        y, cb, cr = comps(37, 23, xs, ys, 41 + xs)
        merged, singles = C.encode(y, cb, cr, xs, ys, sop=True, eph=True, num_resolutions=3, progression=prog, **SMALL)
        assert K.parse(merged)["scod"] == 7
        check(y, cb, cr, xs, ys, merged, singles, PK | SUB, (xs, ys, prog))
        rc, msg, _ = K.plan([merged], 37, 23, 37, 23, False, pbx.UINT8, 3, flags=SUB)
        assert rc == 400 and "SOP or EPH markers (Scod 0x07)" in msg


def test_irreversible_precincts_and_layers():
    y, cb, cr = comps(40, 24, 2, 2, 51)
    merged, singles = C.encode(y, cb, cr, 2, 2, True, num_resolutions=3, progression="RPCL", quality_mode="dB",
                               quality_layers=[32, 44], **SMALL)
    hd = K.parse(merged)
    assert hd["transform"] == 0 and hd["layers"] == 2
    check(y, cb, cr, 2, 2, merged, singles, PK | SUB, "9/7 layers")


def test_ycbcr_without_subsampling():
    """Flag 8 alone: a 1 x 1 stream of three stored components, 5/3 and 9/7; and with MCT 1 the
    refusal."""
    a = C.ycc_smooth(40, 24, 61)
    for enc in (J.encode, J97.encode):
        s = enc(a, mct=0, num_resolutions=3)
        plain, rgb = decode(s, 40, 24, 0), decode(s, 40, 24, YCC)
        assert np.array_equal(rgb, ycc_to_rgb(plain[:, :, 0], plain[:, :, 1], plain[:, :, 2]))
        assert not np.array_equal(rgb, plain)
        if enc is J.encode:
            assert np.array_equal(plain, a)
    s = J.encode(a, mct=1, num_resolutions=3)
    for hook in (K.plan, K.cpu_decode):
        rc, msg, _ = hook([s], 40, 24, 40, 24, False, pbx.UINT8 if hook is K.plan else np.uint8, 3, flags=YCC)
        assert rc == 400 and "segment 0: YCbCr conversion (PBX_TIFF_F_J2K_YCBCR) on a stream with the multiple-component transform" in msg
    g = J.encode(a[:, :, 0], num_resolutions=3)
    rc, msg, _ = K.plan([g], 40, 24, 40, 24, False, pbx.UINT8, 1, flags=YCC)
    assert rc == 400 and "YCbCr conversion (PBX_TIFF_F_J2K_YCBCR) on JPEG 2000 segments of 1 sample(s) per pixel of 8 bits (3 of 8)" in msg
    g16 = J.encode(K.smooth(40, 24, 1, np.uint16), num_resolutions=3)
    rc, msg, _ = K.plan([g16], 40, 24, 40, 24, False, pbx.UINT16, 1, flags=YCC)
    assert rc == 400 and "YCbCr conversion" in msg and "of 16 bits" in msg


def test_tiles_and_strips_through_the_hook():
    """Pages of several segments: tiles clipped by the image, a last strip of odd height."""
    for (xs, ys), lay in zip(C.FACTORS, (dict(tile=(32, 32)), dict(rows_per_strip=8), dict(tile=(16, 16)))):
        pg = C.page_of(C.ycc_smooth(50, 37, 71 + xs), xs, ys, num_resolutions=3, **lay)
        for ycc in (False, True):
            rc, msg, got = C.hook_page(pg, SUB | (YCC if ycc else 0))
            assert rc == 0, msg
            assert np.array_equal(got, C.page_planes(pg, ycc)), (xs, ys, ycc)


# ------------------------------------------------------------------------------ band specs
def test_band_plans_cover_the_same_segment_rows():
    pg = C.page_of(C.ycc_smooth(40, 40, 81), 2, 2, rows_per_strip=8, num_resolutions=3)
    per = [C.counts(ss) for ss in pg["singles"]]
    for y0, rows in ((0, 8), (3, 2), (7, 2), (8, 32), (39, 1)):
        k0, k1 = y0 // 8, -(-(y0 + rows) // 8)
        rc, msg, out = K.plan(pg["segments"][k0:k1], 40, 40, 40, 8, False, pbx.UINT8, 3, y0=y0, rows=rows, flags=SUB)
        assert rc == 0, msg
        assert out == [k1 - k0] + [sum(p[i] for p in per[k0:k1]) for i in range(3)]


# ------------------------------------------------------------------------------ refusals
def good_stream(xs=2, ys=1):
    y, cb, cr = comps(40, 24, xs, ys, 91)
    return C.encode(y, cb, cr, xs, ys, num_resolutions=3)[0]


def refusal_cases():
    s = good_stream()
    one = J.encode(comps(40, 24, 2, 1, 91)[0], num_resolutions=3)
    return [
        ("other factors", J.patch(J.patch(s, 0x51, 40, 4), 0x51, 43, 4), 3,
         "sampling factors 4 x 1 on component 1 (2 x 1, 1 x 2 or 2 x 2)"),
        ("factor 3", J.patch(J.patch(s, 0x51, 41, 3), 0x51, 44, 3), 3,
         "sampling factors 2 x 3 on component 1 (2 x 1, 1 x 2 or 2 x 2)"),
        ("factor 0", J.patch(J.patch(s, 0x51, 40, 0), 0x51, 43, 0), 3,
         "sampling factors 0 x 1 on component 1 (2 x 1, 1 x 2 or 2 x 2)"),
        ("first component", J.patch(s, 0x51, 37, 2), 3, "subsampled first component (2 x 1)"),
        ("chroma differ", J.patch(s, 0x51, 44, 2), 3, "chroma components of different sampling factors (2 x 1 and 2 x 2)"),
        ("second only", J.patch(s, 0x51, 43, 1), 3, "chroma components of different sampling factors (2 x 1 and 1 x 1)"),
        ("third only", J.patch(s, 0x51, 40, 1), 3, "chroma components of different sampling factors (1 x 1 and 2 x 1)"),
        ("mct", J.patch(s, 0x52, 4, 1), 3, "subsampled components (2 x 1) with the multiple-component transform"),
        ("one component", J.patch(one, 0x51, 37, 2), 1, "subsampling on a stream of one component (2 x 1)"),
    ]


@pytest.mark.parametrize("case", refusal_cases(), ids=lambda c: c[0])
def test_new_refusals_of_both_layers(case, tmp_path):
    name, stream, spp, text = case
    for flags in (SUB, SUB | PK, SUB | YCC) if spp == 3 else (SUB, SUB | PK):
        rc, msg, _ = K.plan([stream], 40, 24, 40, 24, False, pbx.UINT8, spp, flags=flags)
        assert rc == 400 and msg == "segment 0: " + text, msg
        rc, msg, _ = K.cpu_decode([stream], 40, 24, 40, 24, False, np.uint8, spp, flags=flags)
        assert rc == 400 and msg == "segment 0: " + text, msg
    # without the flag: the text it always was, whatever the factors
    rc, msg, _ = K.plan([stream], 40, 24, 40, 24, False, pbx.UINT8, spp, flags=0)
    assert rc == 400 and ("subsampled components (component" in msg or name == "mct") and text not in msg, msg
    pg = dict(width=40, length=24, bits=8, spp=spp, compression=33003, photometric=2 if spp == 3 else 1, planar=1, tile=None,
              rows_per_strip=24, segments=[stream], subifds=[], description=None)
    path = str(tmp_path / "r.tif")
    J.write_tiff(path, [pg])
    ifd = pbx.tiff_ifds(path)[0]
    if spp == 3:
        with pytest.raises(pbx.PbxError) as e:
            pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_chroma=True)
        assert e.value.status == 400 and str(e.value).endswith("Compression 33003: segment 0: " + text), str(e.value)
        with pytest.raises(pbx.PbxError) as e:
            pbx.tiff_band_spec(path, ifd, 0, 0, j2k_chroma=True)
        assert text in str(e.value)
        with pytest.raises(pbx.PbxError) as e:
            pbx.tiff_image_layout(path, j2k_chroma=True)
        assert text in str(e.value)
    else:  # the keyword means nothing on a one-sample IFD: the old text
        with pytest.raises(pbx.PbxError, match=r"subsampled components \(component 0: 2 x 1\)"):
            pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_chroma=True)


def test_every_prefix_of_a_merged_header_is_a_400():
    s = good_stream(2, 2)
    end = K.parse(s)["data"]
    for cut in range(end):
        rc, msg, _ = K.plan([s[:cut]] if cut else [b"\x00"], 40, 24, 40, 24, False, pbx.UINT8, 3, flags=SUB | YCC)
        assert rc == 400, (cut, msg)
    assert K.plan([s[:end]], 40, 24, 40, 24, False, pbx.UINT8, 3, flags=SUB | YCC)[0] == 0
    rc, msg, _ = K.cpu_decode([s[:end]], 40, 24, 40, 24, False, np.uint8, 3, flags=SUB | YCC)
    assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code 1)" in msg
    # one chroma component's data cut short
    rc, msg, _ = K.cpu_decode([s[:-40]], 40, 24, 40, 24, False, np.uint8, 3, flags=SUB)
    assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code 1)" in msg


def test_the_old_texts_without_the_flags():
    for xs, ys in C.FACTORS:
        s = good_stream(xs, ys)
        for flags in (0, PK):
            for hook, pt in ((K.plan, pbx.UINT8), (K.cpu_decode, np.uint8)):
                rc, msg, _ = hook([s], 40, 24, 40, 24, False, pt, 3, flags=flags)
                assert rc == 400 and msg == "segment 0: subsampled components (component 1: %d x %d)" % (xs, ys), msg
        rc, msg, _ = K.plan([s], 40, 24, 40, 24, False, pbx.UINT8, 3, flags=YCC)  # the YCbCr flag does not lift it
        assert rc == 400 and msg == "segment 0: subsampled components (component 1: %d x %d)" % (xs, ys), msg
    for flags in (2, 3, 6, 10, 0x10, 0x100, -1):
        rc, msg, _ = K.plan([s], 40, 24, 40, 24, False, pbx.UINT8, 3, flags=flags)
        assert rc == 400 and msg == "bad flags 0x%x" % (flags & 0xFFFFFFFF), msg
    # the flags are the JPEG 2000 calls' alone
    import ctypes
    for flags in (SUB, YCC):
        st, keep = K.segments_struct([s], 40, 24, False, flags=flags)
        out = (ctypes.c_uint64 * 4)()
        assert pbx.lib().pbx_test_tiff_plan(ctypes.byref(st), 40, 24, 1, out) == 400


# ------------------------------------------------------------------------------ the Python layer
FUNCS = [pbx.tiff_plane_spec, pbx.tiff_band_spec, pbx.tiff_image_layout, pbx.PixelsService.register_tiff_image, pbx.TiffSource.__init__]


def test_defaults_of_the_five_signatures():
    for f, want in zip(FUNCS, (False, False, False, True, True)):
        p = inspect.signature(f).parameters
        assert p["j2k_chroma"].default is want, f
        assert p["aperio_ycbcr"].default is False, f


def write_page(tmp_path, name, **kw):
    path = str(tmp_path / name)
    pg = C.page_of(C.ycc_smooth(40, 24, 5), **kw)
    J.write_tiff(path, [pg])
    return path, pg, pbx.tiff_ifds(path)[0]


def test_python_keywords(tmp_path):
    path, pg, ifd = write_page(tmp_path, "a.tif", xs=2, ys=1, compression=33003, photometric=2, num_resolutions=3)
    # without the keyword: the text it always was, from all three
    for call in (lambda **kw: pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, **kw), lambda **kw: pbx.tiff_band_spec(path, ifd, 0, 8, **kw),
                 lambda **kw: pbx.tiff_image_layout(path, **kw)):
        for kw in ({}, dict(j2k_packets=True), dict(aperio_ycbcr=True)):
            with pytest.raises(pbx.PbxError, match=r"segment 0: subsampled components \(component 1: 2 x 1\)") as e:
                call(**kw)
            assert e.value.status == 400
    sp = pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_chroma=True)
    assert sp["flags"] == SUB and sp["j2k"] is True and sp["samples_per_pixel"] == 3
    assert pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_chroma=True, j2k_packets=True)["flags"] == SUB | PK
    assert pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_chroma=True, aperio_ycbcr=True)["flags"] == SUB | YCC
    bd = pbx.tiff_band_spec(path, ifd, 0, 8, sample=2, j2k_chroma=True, aperio_ycbcr=True, j2k_packets=True)
    assert bd["flags"] == SUB | YCC | PK and bytes(bd["segments"][0]) == pg["segments"][0] and bd["sample"] == 2
    assert pbx.tiff_image_layout(path, j2k_chroma=True)["size_c"] == 3
    # Aperio's rule is Compression 33003's alone
    for comp in (33004, 33005, 34712):
        p2, _, ifd2 = write_page(tmp_path, "c%d.tif" % comp, xs=2, ys=1, compression=comp, photometric=2, num_resolutions=3)
        assert pbx.tiff_plane_spec(p2, ifd2, 1, 0, 0, 0, j2k_chroma=True, aperio_ycbcr=True)["flags"] == SUB
    # PhotometricInterpretation 6
    path, pg, ifd = write_page(tmp_path, "b.tif", xs=2, ys=2, compression=34712, photometric=6, num_resolutions=3)
    for kw in ({}, dict(j2k_packets=True), dict(aperio_ycbcr=True)):
        with pytest.raises(pbx.PbxError, match="PhotometricInterpretation 6 with SamplesPerPixel 3"):
            pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, **kw)
    assert pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_chroma=True)["flags"] == SUB | YCC
    # ... on 1 x 1 components: the YCbCr flag alone; and no flag at all where nothing needs one
    a = C.ycc_smooth(40, 24, 5)
    path = str(tmp_path / "d.tif")
    J.write_tiff(path, [J.page_of(a, 34712, photometric=6, num_resolutions=3)])
    assert pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0, j2k_chroma=True)["flags"] == YCC
    J.write_tiff(path, [J.page_of(a, 33003, num_resolutions=3)])
    ifd = pbx.tiff_ifds(path)[0]
    assert "flags" not in pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_chroma=True)
    assert "flags" not in pbx.tiff_band_spec(path, ifd, 0, 8, j2k_chroma=True)
    assert pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, aperio_ycbcr=True)["flags"] == YCC
    J.write_tiff(path, [J.page_of(a, 33003, num_resolutions=3, mct=1)])
    with pytest.raises(pbx.PbxError, match=r"segment 0: YCbCr conversion \(PBX_TIFF_F_J2K_YCBCR\) on a stream with the multiple"):
        pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0, aperio_ycbcr=True)
    assert "flags" not in pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0, j2k_chroma=True)
    # Photometric 6 on a one-sample IFD, and on a planar one, stays refused in every case
    g = np.ascontiguousarray(a[:, :, 0])
    J.write_tiff(path, [J.page_of(g, 33003, photometric=6, num_resolutions=3)])
    for kw in ({}, dict(j2k_chroma=True), dict(j2k_chroma=True, aperio_ycbcr=True)):
        with pytest.raises(pbx.PbxError, match="PhotometricInterpretation 6 with Compression 33003"):
            pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0, **kw)
    J.write_tiff(path, [J.page_of(a, 33003, planar=True, photometric=6, num_resolutions=3)])
    with pytest.raises(pbx.PbxError, match="PhotometricInterpretation 6 with SamplesPerPixel 3"):
        pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0, j2k_chroma=True, aperio_ycbcr=True)
    # a file that is not JPEG 2000 carries no flags, keywords or not
    from PIL import Image
    plain = str(tmp_path / "plain.tif")
    Image.fromarray(a).save(plain)
    assert "flags" not in pbx.tiff_plane_spec(plain, pbx.tiff_ifds(plain)[0], 1, 0, 0, 0, j2k_chroma=True, aperio_ycbcr=True)


def test_band_specs_read_the_same_byte_ranges(tmp_path, monkeypatch):
    """The keywords change which flags a spec carries, never what is read: segment 0 for the header
    check, then exactly the covering segment rows."""
    path, pg, ifd = write_page(tmp_path, "s.tif", xs=2, ys=2, compression=33003, photometric=2, rows_per_strip=8, num_resolutions=3)
    plain = str(tmp_path / "p.tif")
    J.write_tiff(plain, [J.page_of(C.ycc_smooth(40, 24, 5), 33003, rows_per_strip=8, num_resolutions=3)])
    import builtins
    real = builtins.open

    def ranges(p, d, **kw):
        seen = []

        class Spy:
            def __init__(self, f):
                self.f, self.at = f, 0

            def seek(self, o):
                self.at = o
                return self.f.seek(o)

            def read(self, n=-1):
                seen.append((self.at, n))
                return self.f.read(n)

            def readinto(self, b):
                seen.append((self.at, len(b)))
                return self.f.readinto(b)

            def __enter__(self):
                return self

            def __exit__(self, *a):
                self.f.close()
        monkeypatch.setattr(builtins, "open", lambda *a, **k: Spy(real(*a, **k)))
        try:
            pbx.tiff_band_spec(p, d, 9, 3, **kw)
        finally:
            monkeypatch.setattr(builtins, "open", real)
        return seen
    want = [(ifd["offsets"][0], ifd["counts"][0]), (ifd["offsets"][1], ifd["counts"][1])]
    assert ranges(path, ifd, j2k_chroma=True) == want == ranges(path, ifd, j2k_chroma=True, aperio_ycbcr=True, j2k_packets=True)
    d = pbx.tiff_ifds(plain)[0]
    assert ranges(plain, d) == ranges(plain, d, j2k_chroma=True, aperio_ycbcr=True) == [(d["offsets"][0], d["counts"][0]),
                                                                                         (d["offsets"][1], d["counts"][1])]


def test_the_serving_path_accepts_by_default(tmp_path):
    path, pg, ifd = write_page(tmp_path, "t.tif", xs=2, ys=1, compression=33003, photometric=2, tile=(32, 32), num_resolutions=3)
    src = pbx.TiffSource({7: path})
    px = src.get_pixels(7)
    assert (px.size_x, px.size_y, px.size_c) == (40, 24, 3)
    assert src.plane_segments(px, 0, 1, 0, 0)["flags"] == SUB | PK
    assert src.band_segments(px, 0, 2, 0, 0, 0, 8)["flags"] == SUB | PK
    ap = pbx.TiffSource({7: path}, aperio_ycbcr=True)
    assert ap.plane_segments(ap.get_pixels(7), 0, 0, 0, 0)["flags"] == SUB | PK | YCC
    with pytest.raises(pbx.PbxError, match=r"subsampled components \(component 1: 2 x 1\)"):
        pbx.TiffSource({7: path}, j2k_chroma=False).get_pixels(7)


# ------------------------------------------------------------------------------ the fixtures
FILES = C.manifest()


@pytest.mark.parametrize("entry", FILES, ids=[f["file"] for f in FILES])
def test_fixture_on_the_cpu(entry):
    """The committed files through tiff_plane_spec and the hook: the stored components, the share
    the manifest records, Pillow at even sizes."""
    import hashlib
    path = os.path.join(C.GOLD, entry["file"])
    ifd = pbx.tiff_ifds(path)[0]
    xs, ys = entry["factors"]
    want = np.load(os.path.join(C.GOLD, entry["file"].replace(".tif", ".npy")))
    for c in range(3):
        assert hashlib.sha256(J.be_bytes(np.ascontiguousarray(want[:, :, c]))).hexdigest() == entry["planes"]["0"]["0,%d,0" % c][2]
    with pytest.raises(pbx.PbxError, match=r"subsampled components \(component 1: %d x %d\)|PhotometricInterpretation 6" % (xs, ys)):
        pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_packets=True)
    sp = pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0, j2k_packets=True, j2k_chroma=True, aperio_ycbcr=bool(entry.get("aperio")))
    assert sp["flags"] == PK | SUB | YCC
    geo = (entry["width"], entry["length"], sp["seg_w"], sp["seg_h"], sp["tiled"], np.uint8, 3)
    rc, msg, got = K.cpu_decode(sp["segments"], *geo, flags=PK | SUB)
    assert rc == 0, msg
    got = np.moveaxis(got, 0, 2)
    rc, msg, rgb = K.cpu_decode(sp["segments"], *geo, flags=PK | SUB | YCC)
    assert rc == 0, msg
    assert np.array_equal(np.moveaxis(rgb, 0, 2), ycc_to_rgb(got[:, :, 0], got[:, :, 1], got[:, :, 2]))
    if entry["lossy"]:
        mask = np.unpackbits(np.load(os.path.join(C.GOLD, entry["file"].replace(".tif", "_mask.npy"))))[:want.size]
        mask = mask.reshape(want.shape).astype(bool)
        assert round(float(mask.mean()), 4) == entry["inside"] <= 0.0361
        J97.check_close(got, want, mask, entry["file"])
    else:
        assert entry["inside"] == 0 and np.array_equal(got, want)
    # Pillow, a second opinion on the fixtures of even sizes (never the device's yardstick): the
    # generator's largest |Pillow's RGB - ycc_to_rgb of the stored planes|
    assert entry["pil"] == (None if entry["file"].startswith("ycc422_strips8_w37") else 1)


def test_pillow_agrees_with_the_expectation_at_even_sizes():
    """Pillow (OpenJPEG) replicates too: its RGB of a merged stream is within 1 of ycc_to_rgb of the
    replicated inputs on 5/3 streams (its colour conversion rounds differently), as measured."""
    worst = 0
    for w, h, xs, ys in ((40, 24, 2, 2), (64, 64, 2, 2), (40, 23, 2, 1), (38, 22, 2, 2), (40, 24, 1, 2)):
        y, cb, cr = comps(w, h, xs, ys, w + h)
        merged, _ = C.encode(y, cb, cr, xs, ys, num_resolutions=3)
        pil = J.pil_decode(merged)
        assert pil.shape == (h, w, 3)
        worst = max(worst, int(np.abs(pil.astype(np.int64) - C.planes(y, cb, cr, xs, ys, True).astype(np.int64)).max()))
    assert worst == 1
