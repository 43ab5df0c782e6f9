"""The hand-built JPEG scans (tests/_tiff_jpeg_frames.py, tests/_tiff_jpeg_cases.py) without a GPU:
every well-formed one decodes under the model (_tiff_jpeg.decode) to exactly PIL's pixels
(libjpeg-turbo: the judge, as everywhere in the JPEG tests) and under the schedule model (a second
decoder, restated from the kernel's text) to the model's coefficients; the planner accepts every
one; the censuses of the schedule model cover the checklist line by line; the model's range
assertion is lifted for padding blocks only; every malformed stream ends in its decoder code under
both models.  test_gpu_tiff_jpeg_frames.py then gives the same streams to k_tiff_jpeg_decode and
k_tiff_jpeg_place."""
import itertools
import os
import re
from collections import Counter

import numpy as np
import pytest

import _tiff_jpeg as J
import _tiff_jpeg_cases as C
import _tiff_jpeg_frames as F
from test_tiff_jpeg_host import plan

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omero-ms-pixel-buffer_amd", "csrc")
GROUPS = list(C.cases())


def exempt_of(case):
    return F.padding_blocks(case[3]) if case[0] in C.EXEMPT else None


def model(case):
    return J.decode(case[3], ycbcr=case[4] != "rgb", exempt=exempt_of(case))


def pil(stream):
    """PIL's pixels.  LOAD_TRUNCATED_IMAGES: of a complete scan without EOI libjpeg decodes every
    MCU, and only PIL's file layer would refuse the file for its missing end."""
    from PIL import ImageFile
    old = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = True
    try:
        return J.pil_decode(stream)
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = old


def test_kernel_constants_are_the_sources():
    text = open(os.path.join(CSRC, "kernels_tiff_jpeg.hip")).read()
    for name, value in F.KERNEL_CONSTANTS.items():
        assert re.findall(r"constexpr uint32_t %s = (\d+);" % name, text) == [str(value)], name
    # what the model restates, where the kernel spells it
    for snippet in ("static_assert(J_LOW * 8 >= 27 + 63 * 26 + 64", "for (uint32_t k = 0; k < rem; k += 256)",
                    "while (!pend && cend <= J_CAP - 64)", "} else if (rawp + 64 >= csize) {",
                    "const bool marker = have && prev == 0xFF && b != 0 && b != 0xFF;",
                    "const bool keep = have && !marker && !(b == 0 && prev == 0xFF) && (b != 0xFF || next == 0);",
                    "if (!s.pend && s.cend * 8 < s.cp * 8 - s.nb + J_LOW * 8) jrefill(s, raw, csize, lane);",
                    "if (!s.pend) jrefill(s, raw, csize, lane);", "const uint32_t per = 64 / bpm;", "l = 10;",
                    "if (s.pend != 0xD0 + (rstn & 7) || (posb + 7) >> 3 != s.cend) { bad = 5; break; }",
                    "J_Q + c * 128", "J_H + 2 * c * (uint32_t)sizeof(JHuff)", "off < vis; off += 1024"):
        assert snippet in text, snippet
    assert F.FAT == 27 + 63 * 26 == 1665 and F.J_LOW * 8 >= F.FAT + 64 and F.J_PAD * 8 >= F.FAT + 64


# ------------------------------------------------------------------------------ well-formed
@pytest.mark.parametrize("group", GROUPS)
def test_model_equals_pil_and_the_schedule_model_equals_the_model(group):
    for case in C.cases()[group]:
        name, w, h, stream, kind = case
        got = model(case)
        assert got.shape[:2] == (h, w), name
        assert np.array_equal(got, pil(stream)), name
        bad, census, coefs = F.schedule(stream)
        assert bad == 0, (name, bad)
        want = J.decode_coefficients(stream)[1]
        assert all(np.array_equal(a, b) for a, b in zip(F.dequantised(stream, coefs), want)), name
        assert len(F.entropy(stream)) <= 8192, name


@pytest.mark.parametrize("group", GROUPS)
def test_the_planner_accepts_every_case_and_plans_what_the_header_says(group):
    """What pbx_test_tiff_jpeg_plan shows of the JStream it planned: one stream, its decoded
    samples, the scratch of its MCU grid, one table set, the placement mode, the entropy bytes."""
    modes = {"gray": 0, "rgb": 0, "444": 1, "422": 2, "420": 3}
    for name, w, h, stream, kind in C.cases()[group]:
        H = J.header(stream)
        nc = len(H["comps"])
        assert (H["width"], H["height"], nc) == (w, h, 1 if kind == "gray" else 3), name
        hs, vs = (H["comps"][0][1], H["comps"][0][2]) if nc == 3 else (1, 1)
        assert (hs, vs) == {"422": (2, 1), "420": (2, 2)}.get(kind, (1, 1)), name
        mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
        pitch0, pitchc = (mcux * hs * 8 + 15) & ~15, (mcux * 8 + 15) & ~15
        size0 = (pitch0 * mcuy * vs * 8 + 255) & ~255
        sizec = (pitchc * mcuy * 8 + 255) & ~255 if nc == 3 else 0
        for pg in pages_of(stream, w, h, kind, both=group == "tables"):
            rc, msg, out = plan(pg)
            assert rc == 0, (name, msg)
            assert out == [1, w * h * nc, size0 + 2 * sizec, 1, modes[kind], len(F.entropy(stream))], (name, out)


def pages_of(stream, w, h, kind, both=False):
    """The one-strip page around a case; for the table cases also the one with the tables in tag
    347 and the segment abbreviated."""
    pg = J.stream_page(w, h, stream, photometric=2 if kind == "rgb" else None)
    if not both:
        return [pg]
    tabs, rest = J.split_tables(stream)
    return [pg, dict(pg, segments=[rest], extra=[(347, 1, list(tabs))])]


def test_tables_in_the_tag_decode_as_in_the_segment():
    for case in C.cases()["tables"]:
        name, w, h, stream, kind = case
        tabs, rest = J.split_tables(stream)
        assert b"\xff\xdb" not in rest[:J.header(rest)["data"]] and b"\xff\xc4" not in rest[:J.header(rest)["data"]]
        assert np.array_equal(J.decode(rest, tabs, ycbcr=kind != "rgb"), model(case)), name


# ------------------------------------------------------------------------------ censuses
def censuses():
    return {c[0]: F.schedule(c[3])[1] for c in C.all_cases()}


def test_the_censuses_cover_the_whole_checklist():
    seen = Counter()
    for cs in censuses().values():
        seen.update(cs)
    missing = [k for k in C.CHECKLIST if not seen[k]]
    assert not missing, missing
    assert len(set(C.CHECKLIST)) == len(C.CHECKLIST)
    # and what the cases file calls unreachable, no well-formed case reaches
    assert all(not seen[k] for k in C.UNREACHABLE), {k: seen[k] for k in C.UNREACHABLE}
    assert not any(k.startswith("move:iterations:") and k != "move:iterations:1" for k in seen)


def test_named_cases_reach_what_their_names_say():
    cs = censuses()
    for p in C.LANES:
        # p empty bytes, 6 of content, the prefix, the code; 65 fill bytes move it on by 65
        assert cs["marker_lane_p%02d_fill0" % p]["marker:lane:%d" % ((p + 7) % 64)] == 2
        assert cs["marker_lane_p%02d_fill65" % p]["marker:lane:%d" % ((p + 7 + 65) % 64)] == 2
        assert cs["stuff_lane_ac_p%02d" % p]["stuff:lane:%d" % ((p + 1) % 64)] == 1
        assert cs["stuff_lane_dc_p%02d" % p]["stuff:lane:%d" % ((p + 2) % 64)] == 1
    assert cs["stuff_lane_ac_p62"]["stuff-split"] == 1 and cs["stuff_lane_dc_p61"]["stuff-split"] == 1
    assert cs["marker_lane_p57_fill0"]["prefix-split"] == 2       # both intervals: FF at lane 63, the code at lane 0
    assert cs["marker_lane_p57_fill65"]["fill-round"] == 2        # FF from lane 63 on: a whole round of fill bytes
    assert cs["marker_lane_p00_fill65"]["fill-run-crosses-round"] >= 1
    assert cs["end_exactly_on_a_round_no_eoi"]["eos:exact-round"] == 1
    assert cs["end_last_byte_ff_no_eoi"]["eos:last-byte-FF"] == 1 and cs["end_no_eoi"]["eos:no-EOI"] == 1
    assert cs["end_junk_after_eoi"]["eos:junk-after-EOI"] == 1 and cs["all_eob"]["stream:all-eob"] == 1
    assert cs["fill_byte_before_a_stuffed_pair"]["FF FF 00"] == 1
    fat = [n for n in cs if n.startswith("fat_1665")]
    assert len(fat) == 4 and all(cs[n]["fat:1665"] == 24 and cs[n]["block-bits:max"] == 1665 for n in fat)
    assert cs["fat_1665_in_padding_behind_longer_visible_blocks"]["refill:in-front-of-a-fat-block"] >= 2
    assert cs["fat_1665_in_padding_12_mcus"]["refill:just-after-a-fat-block"] >= 2
    assert cs["fat_1665_in_padding_interval_1_fill_70"]["refill:restart"] == 11
    bits, _ = C.fattest_visible()
    assert cs["fat_visible_%d_bits" % bits]["block-bits:max"] == bits and 1400 < bits < F.FAT
    sym = cs["symbols_every_length_size_and_pattern"]
    assert all(sym["code:ac:len:%d:%s" % (l, "lut" if l < 10 else "walk")] for l in range(1, 17))
    chains = [n for n in cs if cs[n]["refill:moved"] >= 3]
    assert any(n.startswith("refill_") for n in chains)


# ------------------------------------------------------------------------------ would a wrong decoder pass?
CAUGHT_BY = {
    # lane 0 without the byte before it: the marker code whose FF ended the last round is kept as data, the zero after
    # an FF at lane 63 too
    "no-prev": ("marker_lane_p57_fill0", "marker_lane_p56_fill1", "stuff_lane_ac_p62", "stuff_lane_dc_p61"),
    # lane 63 without the byte after it: a data FF there is dropped as if it were a prefix
    "no-next": ("stuff_lane_ac_p62", "stuff_lane_dc_p61"),
    # the moved remainder begins inside a byte: every refill case has moved refills with skip != 0
    "no-skip": ("refill_gray_seed1", "refill_444_seed1", "refill_422_seed1", "refill_420_seed1",
                "fat_1665_in_padding_12_mcus"),
    # component 2 with component 1's tables
    "c-offset": ("tables_444_tq302_td213_ta302", "tables_rgb_tq302_td213_ta302", "tables_420_tq302_td213_ta302",
                 "symbols_every_length_size_and_pattern"),
}


@pytest.mark.parametrize("mutation", F.MUTATIONS)
def test_a_decoder_wrong_in_one_place_fails_named_cases(mutation):
    """The schedule model with one line of the kernel restated wrongly: each named case then ends in
    an error or in other coefficients, so the device, held to the model byte for byte on the same
    case, could not pass with that line wrong."""
    by_name = {c[0]: c for c in C.all_cases()}
    for name in CAUGHT_BY[mutation]:
        stream = by_name[name][3]
        good = F.schedule(stream)
        bad = F.schedule(stream, mutate=mutation)
        assert good[0] == 0 and (bad[0] != 0 or bad[2] != good[2]), name
    if mutation == "no-skip":
        assert all(any(F.schedule(by_name[n][3])[1]["skip:%d" % k] for k in range(1, 8)) for n in CAUGHT_BY[mutation])


def test_the_wide_pages_hold_pixels_past_the_first_placement_step():
    """k_tiff_jpeg_place without its `off += 1024` step would leave columns 1024 .. unwritten
    (zero in a fresh plane): every wide page's expected planes are non-zero there, in every row."""
    for name, pg in C.wide_pages():
        want = J.decode_page(pg).reshape(pg["length"], pg["width"], -1)
        assert want[:, 1024:].any(axis=1).all(), name
        if pg["width"] > 2048:
            assert want[:, 2048:].any(axis=1).all(), name


# ------------------------------------------------------------------------------ exemptions
def test_exemptions_are_padding_blocks_only():
    """The range assertion is lifted for blocks no sample of which lies inside width x height, in
    the named cases only; every other case passed the assertion whole (above), and the exempt
    cases need the exemption (their fat blocks do leave the range)."""
    names = {c[0] for c in C.all_cases()}
    assert C.EXEMPT <= names and all(n.startswith("fat_1665_in_padding") for n in C.EXEMPT)
    for case in C.all_cases():
        name, w, h, stream, kind = case
        if name not in C.EXEMPT:
            continue
        H = J.header(stream)
        hs, vs = H["comps"][0][1], H["comps"][0][2]
        masks = exempt_of(case)
        assert sum(int(m.sum()) for m in masks) == 24
        for c, m in enumerate(masks):
            cw, ch = (w, h) if c == 0 else (-(-w // hs), -(-h // vs))
            inside = np.zeros((m.shape[0] * 8, m.shape[1] * 8), bool)
            inside[:ch, :cw] = True
            blocks = inside.reshape(m.shape[0], 8, m.shape[1], 8).any(axis=(1, 3))  # holds a visible sample
            assert np.array_equal(m, ~blocks), (name, c)
        with pytest.raises(AssertionError, match="leaves"):
            J.decode(stream)


# ------------------------------------------------------------------------------ tables
def test_exchanging_any_two_quantisers_changes_visible_pixels():
    """...so a decoder that took component c's quantiser (or Huffman tables: then the stream does
    not decode at all) from another component's slot cannot pass the table cases."""
    for kind, w, h in C.TABLE_KINDS:
        base = J.decode(C.table_stream(kind, w, h), ycbcr=kind != "rgb")
        for a, b in itertools.combinations(range(3), 2):
            tq = list(C.TABLE_IDS[0])
            tq[a], tq[b] = tq[b], tq[a]
            try:
                other = J.decode(C.table_stream(kind, w, h, tuple(tq)), ycbcr=kind != "rgb")
            except AssertionError:
                continue  # out of range under the wrong quantiser: different, then
            assert (other != base).mean() > 0.25, (kind, a, b)
    q, huff = C.three_table_sets()
    assert len({tuple(v) for v in map(tuple, q.values())}) == 3
    assert len({(tuple(b), tuple(v)) for b, v in huff.values()}) == 6


# ------------------------------------------------------------------------------ wide rows
def test_wide_rows_change_chroma_across_the_step_boundary():
    for name, pg in C.wide_pages():
        w = pg["width"]
        if pg["spp"] == 1 or pg["photometric"] != 6 or pg["tile"]:
            continue
        tabs = next(bytes(t[2]) for t in pg["extra"] if t[0] == 347)
        H, planes = J.component_planes(pg["segments"][0], tabs)
        hs, vs = H["comps"][0][1], H["comps"][0][2]
        for c in (1, 2):
            up = J.upsample(planes[c], hs, vs, w, pg["length"])
            for at in range(1024, w, 1024):
                assert len(set(up[0, at - 2:at + 2].tolist())) > 1, (name, c, at)
    assert (C.WIDE + 1) // 2 == 523 and C.WIDE == 1024 + 16 + 5


def test_model_equals_pil_on_the_wide_pages(tmp_path):
    from PIL import Image
    for k, (name, pg) in enumerate(C.wide_pages()):
        if not pg["tile"] and pg["length"] != 3:
            continue
        p = str(tmp_path / ("w%d.tif" % k))
        J.write_tiff(p, [pg])
        assert np.array_equal(J.decode_page(pg), np.asarray(Image.open(p))), name


# ------------------------------------------------------------------------------ malformed
@pytest.mark.parametrize("name", list(C.malformed()))
def test_malformed_stream_ends_in_its_code_under_both_models(name):
    w, h, stream, kind, code, why = C.malformed()[name]
    with pytest.raises(J.JpegError) as e:
        J.decode(stream, exempt=F.padding_blocks(stream))
    assert e.value.code == code, (e.value.code, why)
    assert F.schedule(stream)[0] == code
    rc, msg, out = plan(J.stream_page(w, h, stream))
    assert rc == 0, msg  # the planner reads no entropy-coded byte: the refusal is the device's


def test_malformed_cases_name_every_code_and_the_unreachable_refill():
    assert {v[4] for v in C.malformed().values()} == {1, 2, 3, 4, 5}
    cs = F.schedule(C.malformed()["junk_of_j_cap_bytes_after_an_interval"][2])[1]
    assert cs["refill:restart:no-marker-seen"] == 1 and cs["move:iterations:4"] == 1
    cs = F.schedule(C.malformed()["junk_after_an_interval_marker_already_seen"][2])[1]
    assert cs["refill:restart:no-marker-seen"] == 0 and cs["refill-end:marker"] == 1
    for k in ("dc", "ac"):
        assert F.schedule(C.malformed()["%s_pattern_in_no_table_from_the_walk" % k][2])[1]["code:%s:walk-past-16" % k] == 1
