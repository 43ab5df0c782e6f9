"""Lossy JPEG 2000 TIFF segments (9/7 wavelet, scalar quantisation, ICT) without a GPU:
tests/_tiff_j2k97.py's float64 model against PIL (OpenJPEG); the device's own arithmetic
(tiff_j2k_dev.h) run on the CPU through pbx_test_tiff_j2k_decode against the model; the header
reader, the planner and every refusal of both layers.

close(got, model, window): got == rint(model) wherever the model's value lies farther than
`window` from a half-integer, within 1 of it elsewhere, and the share of pixels inside the window
at most 2 * window + 0.05.  8 bits: window 1/64, which PIL meets too.  16 bits: OpenJPEG scales
the high band by 1.625732422 where 2 / K is 1.625786, 2 grey levels at 65535, so PIL is held to
|PIL - rint(model)| <= 3 and the library, which computes T.800's constants in float32, to
M.WINDOW16 (see M.MEASURED16)."""
import functools
import os

import numpy as np
import pytest

import _tiff_j2k as J
import _tiff_j2k97 as M
import pbx
from test_tiff_j2k_host import PROGRESSIONS, cpu_decode, noise, one, plan

W0, H0 = 24, 17


def smooth(w, h, seed, dtype=np.uint8, samples=1):
    """Structure a quantiser keeps, over the whole range of the type, plus noise."""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    y, x = np.mgrid[0:h, 0:w]
    out = [np.clip((0.5 + 0.4 * np.sin(x / (3.0 + s) + seed) * np.cos(y / (4.0 + s)) + rng.normal(0, 0.06, (h, w))) * top, 0, top)
           for s in range(samples)]
    a = np.stack(out, axis=-1) if samples > 1 else out[0]
    return a.astype(dtype)


def cases():
    """(id, array, encoder options): every axis the issue names, rotated against the others."""
    out = []
    kinds = [("u8", dict(dtype=np.uint8), {}), ("u16", dict(dtype=np.uint16), {}),
             ("rgb", dict(samples=3), dict(mct=0)), ("ict", dict(samples=3), dict(mct=1))]
    n = 0
    for name, akw, ekw in kinds:
        for levels in range(6):
            cb = (4, 4) if levels % 3 == 0 else (32, 32) if levels % 3 == 1 else (64, 64)
            q = {} if levels % 3 == 0 else dict(quality_mode="dB", quality_layers=[32 if levels % 3 == 1 else 44])
            a = smooth(W0 + levels, H0 + (n % 3), 10 + n, **akw) if n & 1 else noise(W0 + levels, H0 + (n % 3), 10 + n, **akw)
            out.append(("%s-L%d-cb%d%s" % (name, levels, cb[0], "-dB%d" % q["quality_layers"][0] if q else ""), a,
                        dict(ekw, num_resolutions=levels + 1, codeblock_size=cb, progression=PROGRESSIONS[n % 5], **q)))
            n += 1
    for name, akw, ekw in kinds:
        for w, h in ((1, 1), (1, 9), (9, 1), (2, 3)):
            out.append(("%s-%dx%d" % (name, w, h), noise(w, h, 50 + w + h, **akw), dict(ekw, num_resolutions=6)))
    # one image of more than 256 pixels per kind carries the share cap on its own
    for name, akw, ekw in kinds:
        out.append(("%s-40x30" % name, smooth(40, 30, 70, **akw), dict(ekw, num_resolutions=4, codeblock_size=(16, 16))))
    return out


CASES = cases()


@functools.lru_cache(maxsize=None)
def decoded(i, style1=False):
    """stream, model (float64), model (float32), PIL, hook: computed once per case."""
    _, a, kw = CASES[i]
    s = M.encode(a, **kw)
    if style1:
        s = M.to_style1(s)
    spp = 1 if a.ndim == 2 else 3
    rc, msg, got = cpu_decode(*one(s, a), a.dtype.type, spp)
    assert rc == 0, msg
    got = got[0] if spp == 1 else np.moveaxis(got, 0, 2)
    return s, M.decode97(s), M.decode97(s, np.float32), J.pil_decode(s), got


def exact_halves(s):
    """A single resolution without a colour transform: step 1, every value an exact half."""
    h = M.parse(s)
    return h["levels"] == 0 and not h["mct"] and all(st == 1.0 for _, st in M.steps(h))


def held(got, model, prec, win, D=None):
    """close(), or for PIL at 16 bits the bound of 3; returns the share inside the window."""
    if D is not None:
        d = int(np.abs(got.astype(np.int64) - M.rint(model, prec).astype(np.int64)).max())
        assert d <= D, d
        return float(M.in_window(model, win).mean())
    ok, inside, outside = M.close(got, model, win, prec)
    assert ok, (outside, inside)
    return inside


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_model_pil_and_hook(i):
    name, a, kw = CASES[i]
    s, m, m32, pil, got = decoded(i)
    prec = 8 * a.dtype.itemsize
    win = M.window(prec)
    assert M.parse(s)["transform"] == 0 and M.parse(s)["qstyle"] == 2
    # PIL against the model
    inside = held(pil, m, prec, M.WINDOW8, None if prec == 8 else 3)
    # the device's arithmetic against the model, with the window of its precision
    held(got, m, prec, win)
    if exact_halves(s):  # no arithmetic to differ in: round half to even, exactly
        assert np.array_equal(got, M.rint(m, prec)) and np.array_equal(pil, M.rint(m, prec))
    elif a.shape[0] * a.shape[1] >= 256:
        assert inside <= 2 * M.WINDOW8 + 0.05 and M.in_window(m, win).mean() <= 2 * win + 0.05
    # the float32 model is the hook's value before rounding: its rounding is the hook's output
    assert np.array_equal(M.rint(m32, prec), got)
    if prec == 16:
        assert np.abs(m32.astype(np.float64) - m).max() <= M.MEASURED16, np.abs(m32.astype(np.float64) - m).max()
    spp = 1 if a.ndim == 2 else 3
    rc, msg, out = plan(*one(s, a), pbx.UINT8 if prec == 8 else pbx.UINT16, spp)
    assert rc == 0 and out == [1] + list(J.counts(s)), (out, J.counts(s), msg)


def test_window_of_16_bits_and_share_over_the_sweep():
    """M.WINDOW16 is twice the largest |float32 - float64| over these inputs, rounded up to a
    power of two, and at most 1/4; over all small images the share inside the windows is capped."""
    worst, inside, total = 0.0, 0, 0
    for i, (name, a, kw) in enumerate(CASES):
        s, m, m32, pil, got = decoded(i)
        prec = 8 * a.dtype.itemsize
        if prec == 16:
            worst = max(worst, float(np.abs(m32.astype(np.float64) - m).max()))
        if not exact_halves(s):
            inside += int(M.in_window(m, M.window(prec)).sum())
            total += m.size
    for entry in M.manifest():  # the 16-bit fixtures are inputs of these tests too
        if entry["bits"] == 16:
            path = os.path.join(M.GOLD, entry["file"])
            data, offs = pbx.tiff_plane_spec(path, pbx.tiff_image_layout(path)["ifds"][0], 1, 0, 0, 0)["segments"]
            for k in range(len(offs) - 1):
                seg = bytes(data[int(offs[k]):int(offs[k + 1])])
                worst = max(worst, float(np.abs(M.decode97(seg, np.float32).astype(np.float64) - M.decode97(seg)).max()))
    print("largest |float32 - float64| at 16 bits: %.5f" % worst)
    assert worst <= M.MEASURED16 and 2 * M.MEASURED16 <= M.WINDOW16 <= 0.25
    assert M.WINDOW16 / 2 < 2 * M.MEASURED16, "the window is the next power of two, not a wider one"
    assert inside / total <= 2 * M.WINDOW16 + 0.05


@pytest.mark.parametrize("i", [k for k, c in enumerate(CASES) if "-L" in c[0] and "-L0" not in c[0]][::2],
                         ids=lambda i: CASES[i][0])
def test_style_1(i):
    """The QCD rewritten as style 1 (every step derived from the LL entry): OpenJPEG decodes
    those too, so the same three-way check."""
    name, a, kw = CASES[i]
    s, m, m32, pil, got = decoded(i, True)
    prec = 8 * a.dtype.itemsize
    assert pbx.j2k_header(s, "s")["qstyle"] == 1 and len(pbx.j2k_header(s, "s")["qcd"]) == 2
    held(pil, m, prec, M.WINDOW8, None if prec == 8 else 3)
    held(got, m, prec, M.window(prec))
    assert np.array_equal(M.rint(m32, prec), got)


@pytest.mark.parametrize("kind", ["u8", "u16", "rgb", "ict"])
def test_small_sweep(kind):
    """Widths 1 .. 10 x heights 1 .. 9, levels and blocks rotating: lengths of 1 and 2, odd
    lengths, empty sub-bands."""
    akw = dict(u8=dict(), u16=dict(dtype=np.uint16), rgb=dict(samples=3), ict=dict(samples=3))[kind]
    prec = 16 if kind == "u16" else 8
    inside = total = 0
    for w in range(1, 11):
        for h in range(1, 10):
            a = noise(w, h, 100 * w + h, **akw)
            s = M.encode(a, mct=1 if kind == "ict" else 0, num_resolutions=1 + (w + 2 * h) % 6,
                         codeblock_size=(4, 4) if (w + h) & 1 else (32, 32), progression=PROGRESSIONS[(w + h) % 5])
            m, pil = M.decode97(s), J.pil_decode(s)
            rc, msg, got = cpu_decode(*one(s, a), a.dtype.type, 1 if a.ndim == 2 else 3)
            assert rc == 0, msg
            got = got[0] if a.ndim == 2 else np.moveaxis(got, 0, 2)
            held(pil, m, prec, M.WINDOW8, None if prec == 8 else 3)
            held(got, m, prec, M.window(prec))
            if exact_halves(s):
                assert np.array_equal(got, M.rint(m, prec))
            else:
                inside += int(M.in_window(m, M.window(prec)).sum())
                total += m.size
    assert inside / total <= 2 * M.window(prec) + 0.05


# ------------------------------------------------------------------------------ the header
GOOD = M.encode(smooth(40, 24, 3, np.uint16), num_resolutions=4, codeblock_size=(16, 16))
RGB = M.encode(smooth(40, 24, 4, samples=3), num_resolutions=3, mct=1)
REV = J.encode(noise(40, 24, 5, np.uint16), num_resolutions=4)


def test_header_reader_fields():
    h = pbx.j2k_header(GOOD, "s")
    hd = M.parse(GOOD)
    assert h["transformation"] == 0 and h["qstyle"] == 2 and h["levels"] == 3 and h["guard"] == hd["guard"]
    assert h["exponents"] == hd["eps"] and h["mantissas"] == hd["mu"] and len(h["qcd"]) == 2 * 10
    assert pbx.j2k_steps(h) == M.steps(hd)
    h1 = pbx.j2k_header(M.to_style1(GOOD), "s")
    assert h1["qstyle"] == 1 and h1["exponents"] == hd["eps"][:1] and h1["mantissas"] == hd["mu"][:1]
    st = pbx.j2k_steps(h1)
    assert [e for e, _ in st] == [hd["eps"][0] - (0 if b == 0 else (b + 2) // 3 - 1) for b in range(10)]
    hr = pbx.j2k_header(REV, "s")
    assert hr["transformation"] == 1 and hr["qstyle"] == 0 and hr["mantissas"] == [] and len(hr["exponents"]) == 10


def qcd_of(stream, style, entries, guard=2):
    """`stream` with its QCD replaced: Sqcd and the entries' bytes."""
    import struct
    q = J.find_marker(stream, 0x5C)
    L = struct.unpack(">H", stream[q + 2:q + 4])[0]
    return stream[:q + 2] + struct.pack(">HB", 3 + len(entries), guard << 5 | style) + bytes(entries) + stream[q + 2 + L:]


def refusals():
    ent = GOOD[J.find_marker(GOOD, 0x5C) + 5:][:20]
    many = bytes([30 << 3, 0]) + ent[2:]  # exponent 30 with 2 guard bits: 31 bit-planes on the LL band
    return [("9/7 unquantised", J.patch(GOOD, 0x5C, 0, 0x40), "irreversible wavelet (9/7) with quantisation style 0"),
            ("5/3 expounded", J.patch(REV, 0x5C, 0, 0x42), "quantisation style 2 (scalar quantisation) with the reversible wavelet"),
            ("5/3 derived", J.patch(REV, 0x5C, 0, 0x41), "quantisation style 1 (scalar quantisation) with the reversible wavelet"),
            ("style 3", J.patch(GOOD, 0x5C, 0, 0x43), "bad quantisation style 3"),
            ("style 2 one band short", qcd_of(GOOD, 2, ent[:18]), "QCD of 9 sub-bands for 3 decomposition levels"),
            ("style 2 one band long", qcd_of(GOOD, 2, ent + ent[:2]), "QCD of 11 sub-bands for 3 decomposition levels"),
            ("style 2 odd length", qcd_of(GOOD, 2, ent[:19]), "QCD of 19 bytes in 16-bit entries"),
            ("style 1 two entries", qcd_of(GOOD, 1, ent[:4]), "QCD of 4 bytes for the one entry of style 1"),
            ("style 1 no entry", qcd_of(GOOD, 1, b""), "QCD of 0 bytes for the one entry of style 1"),
            ("style 1 negative exponent", qcd_of(GOOD, 1, bytes([1 << 3, 0])), "quantisation style 1 derives exponent -1 for sub-band 7"),
            ("31 bit-planes", qcd_of(GOOD, 2, many), "31 magnitude bit-planes on a 9/7 sub-band (at most 30)"),
            ("transformation 2", J.patch(GOOD, 0x52, 9, 2), "bad wavelet transformation 2")]


@pytest.mark.parametrize("case", refusals(), ids=lambda c: c[0])
def test_refusals_of_both_layers(case, tmp_path):
    name, stream, text = case
    rc, msg, _ = plan([stream], 40, 24, 40, 24, False, pbx.UINT16, 1)
    assert rc == 400 and text in msg and "segment 0" in msg, msg
    rc, msg, _ = cpu_decode([stream], 40, 24, 40, 24, False, np.uint16, 1)
    assert rc == 400 and text in msg
    pg = dict(width=40, length=24, bits=16, spp=1, compression=33005, photometric=1, planar=1, tile=None, rows_per_strip=24,
              segments=[stream], subifds=[], description=None)
    path = str(tmp_path / "r.tif")
    J.write_tiff(path, [pg])
    with pytest.raises(pbx.PbxError, match="Compression 33005: segment 0") as e:
        pbx.tiff_plane_spec(path, pbx.tiff_ifds(path)[0], 1, 0, 0, 0)
    assert e.value.status == 400 and text in str(e.value), str(e.value)
    with pytest.raises(pbx.PbxError) as e:
        pbx.tiff_band_spec(path, pbx.tiff_ifds(path)[0], 0, 0)
    assert text in str(e.value)


def test_30_bit_planes_are_accepted():
    ent = GOOD[J.find_marker(GOOD, 0x5C) + 5:][:20]
    rc, msg, _ = plan([qcd_of(GOOD, 2, bytes([29 << 3, 0]) + ent[2:])], 40, 24, 40, 24, False, pbx.UINT16, 1)
    assert rc == 0, msg


def test_every_prefix_of_a_header_is_a_400():
    for good, pt, spp in ((GOOD, pbx.UINT16, 1), (M.to_style1(GOOD), pbx.UINT16, 1), (RGB, pbx.UINT8, 3)):
        end = J.parse(good)["data"]
        for cut in range(end):
            rc, msg, _ = plan([good[:cut]] if cut else [b"\x00"], 40, 24, 40, 24, False, pt, spp)
            assert rc == 400, (cut, msg)
            with pytest.raises(pbx.PbxError) as e:
                pbx.j2k_header(good[:cut], "segment 0")
            assert e.value.status == 400
        rc, msg, _ = cpu_decode([good[:end]], 40, 24, 40, 24, False, np.uint16 if spp == 1 else np.uint8, spp)
        assert rc == 400 and "corrupt segment stream 0 (j2k, decoder code 1)" in msg


def test_flipped_bits_end_in_a_400_or_an_image():
    """200 flipped bits after the header, through the hook: garbage magnitudes of up to 30
    bit-planes through float arithmetic still land inside the sample range (the output type holds
    nothing else) and no run reads or writes outside its blocks (the sanitizer program's part)."""
    rng = np.random.default_rng(7)
    for good, dt, spp in ((GOOD, np.uint16, 1), (RGB, np.uint8, 3)):
        d = J.parse(good)["data"]
        seen = set()
        for _ in range(100):
            bad = bytearray(good)
            bad[int(rng.integers(d, len(good) - 2))] ^= 1 << int(rng.integers(8))
            rc, msg, got = cpu_decode([bytes(bad)], 40, 24, 40, 24, False, dt, spp)
            assert rc in (0, 400), (rc, msg)
            seen.add(rc)
        assert 0 in seen


def test_huge_steps_saturate():
    """The largest steps a QCD can name (exponent 0: 2^16 .. 2^18 times 1.9995) stay far below
    float32's range at 30 bit-planes (2^31 * 2^18), so no infinity arises from an accepted header;
    the values leave the sample range by orders of magnitude and are clamped to its ends.  (What
    the rounding does with NaN and infinities is scripts/tiff_j2k97_san.cpp's to show.)"""
    huge = qcd_of(GOOD, 2, bytes([0x07, 0xFF]) * 10, guard=7)
    rc, msg, got = cpu_decode([huge], 40, 24, 40, 24, False, np.uint16, 1)
    assert rc in (0, 400), msg
    if rc == 0:
        assert np.isin(got, (0, 65535)).mean() > 0.9


def test_reversible_fixtures_still_decode_to_their_originals():
    for entry in J.manifest():
        path = os.path.join(J.GOLD, entry["file"])
        lay = pbx.tiff_image_layout(path)
        (z, c0, t), d = lay["planes"][0], lay["ifds"][0]
        sp = pbx.tiff_plane_spec(path, d, 1, 0, 0, 0, sample=0)
        dt = np.uint8 if sp["pixel_type"] == pbx.UINT8 else np.uint16
        rc, msg, cpu = cpu_decode(sp["segments"], d["width"], d["length"], sp["seg_w"], sp["seg_h"], sp["tiled"], dt,
                                  sp["samples_per_pixel"])
        assert rc == 0, msg
        for q in range(sp["samples_per_pixel"]):
            assert np.array_equal(cpu[q], J.expected(entry, 0, "%d,%d,%d" % (z, c0 + q, t))), entry["file"]


def test_fixtures_match_their_manifest():
    """The stored rint(model) and masks are what the model gives today, and the hook meets them."""
    for entry in M.manifest():
        path = os.path.join(M.GOLD, entry["file"])
        lay = pbx.tiff_image_layout(path)
        (z, c0, t), ifd = lay["planes"][0], lay["ifds"][0]
        for level, d in enumerate([ifd] + ifd["subifds"]):
            S = d["spp"]
            for s in range(S if d["planar"] == 2 and S > 1 else 1):
                sp = pbx.tiff_plane_spec(path, d, 1, 0, 0, 0, sample=s)
                dt = np.uint8 if sp["pixel_type"] == pbx.UINT8 else np.uint16
                rc, msg, cpu = cpu_decode(sp["segments"], d["width"], d["length"], sp["seg_w"], sp["seg_h"], sp["tiled"], dt,
                                          sp["samples_per_pixel"])
                assert rc == 0, msg
                for q in range(sp["samples_per_pixel"]):
                    want, mask = M.expected(entry, level, "%d,%d,%d" % (z, c0 + s + q, t))
                    M.check_close(cpu[q], want, mask, (entry["file"], level, s + q))
        if entry["file"].startswith("gray8_strips16"):  # one file through the model again
            data, offs = pbx.tiff_plane_spec(path, ifd, 1, 0, 0, 0)["segments"]
            m = np.concatenate([M.decode97(bytes(data[int(offs[k]):int(offs[k + 1])])) for k in range(len(offs) - 1)])
            want, mask = M.expected(entry, 0, "0,0,0")
            assert np.array_equal(M.rint(m, 8), want) and np.array_equal(M.in_window(m, M.WINDOW8), mask)
