"""The hand-built deflate streams (tests/_deflate_frames.py, tests/_deflate_cases.py) on the CPU:
every well-formed one decodes under zlib (Python's module and the oracle's pbxo_zlib_inflate) to
exactly the writer's bytes, the reference inflater agrees, the censuses cover the whole checklist,
and zlib's verdict on each malformed stream is pinned.  The reference is zlib, never the kernel;
test_gpu_deflate_frames.py then gives the same streams to k_zarr_inflate2 and k_zarr_inflate."""
import gzip
import os
import re
import zlib

import pytest

import _deflate_cases as C
import _deflate_frames as F

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omero-ms-pixel-buffer_amd", "csrc")


def zlib_verdict(stream, dlen):
    """The decoded bytes, or zlib's message; "length" for a stream that decodes to another size
    than the chunk's, "incomplete or truncated" for one that ends early."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream)
    except zlib.error as e:
        return str(e)
    if not d.eof:
        return "incomplete or truncated"
    return out if len(out) == dlen else "length"


def test_kernel_constants_are_the_sources():
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("kernels_zarr.hip", "zarr_dev.h"))
    for name, value in C.KERNEL_CONSTANTS.items():
        found = re.findall(r"constexpr uint32_t %s = (\d+);" % name, text)
        assert found == [str(value)], (name, found)


@pytest.mark.parametrize("name", C.small_cases())
def test_well_formed_stream_decodes_under_zlib_and_the_oracle(oracle, name):
    b = C.cases()[name]
    assert zlib.decompress(b.frame) == b.content
    assert oracle.zlib_inflate(b.frame, len(b.content)) == (0, b.content)
    got, census = F.inflate(b.frame[2:-4])
    assert got == b.content and census == b.census


@pytest.mark.parametrize("dist", F.RING_DISTS)
def test_ring_boundary_streams_decode_under_zlib(oracle, dist):
    for phase in range(64):
        b = C.cases()["ring_dist_%d_phase_%02d" % (dist, phase)]
        assert len(b.content) == C.RING_LEN
        assert zlib.decompress(b.frame) == b.content, phase
        assert oracle.zlib_inflate(b.frame, C.RING_LEN) == (0, b.content), phase


def test_censuses_cover_the_whole_checklist():
    """A condition, not a measurement: every path of the checklist is taken by some case."""
    seen = set().union(*(b.census for b in C.cases().values()))
    missing = [item for item in C.CHECKLIST if item not in seen]
    assert not missing, missing
    assert len(set(C.CHECKLIST)) == len(C.CHECKLIST)


def test_the_7_bit_block_is_serial_in_its_first_round_only():
    """No 7-bit window of the block's data, at any offset, is the all-ones prefix of the two 8-bit
    codes, so a chain off the token grid never meets the true one; the model of the producer's
    schedule then gives 63 pass-B iterations in the first round (S = 128, whole FIFO free: 1171
    tokens fit) and segments of 168 = 24 tokens from then on, where every lane starts on a token."""
    b = C.cases()["uniform_7_bit_tokens_serial_pass_b_in_the_first_round"]
    assert "block:uniform_token_width:7" in b.census
    start = 8 * 2 + F.header_bits(F.dyn([7] * 127 + [0] * 128 + [8, 8], [0], [], items=C.ITEMS7))
    bits = int.from_bytes(b.frame, "little") >> start
    for k in range(7 * C.NTOK_SYNC - 7):
        assert (bits >> k) & 127 != 127, k
    rounds = F.producer_schedule(b.frame[2:-4])
    assert (rounds[0]["S"], rounds[0]["depth"], rounds[0]["tokens"]) == (128, 63, 1171)
    assert all(r["S"] == 7 * C.ZP_SEGTOK and r["depth"] == 0 for r in rounds[1:])


def test_the_periodic_block_keeps_pass_b_serial_in_every_round():
    """The model of zp_huff_block's schedule (F.producer_schedule: segment lengths from `sbits`,
    pass A from every segment start, pass B until no entry changes) on the 88-bit-period block:
    every one of its macro-rounds but the last (where the block ends) has S = ZP_SMAX, lane 1 off
    the token grid and 63 iterations of pass B, the serial hand-over across all 64 lanes; there
    are four such rounds.  The stream has fewer tokens than the FIFO, so no round is cut."""
    b = C.cases()[C.SERIAL]
    assert "block:two_token_period_of_88_bits" in b.census
    rounds = [r for r in F.producer_schedule(b.frame[2:-4]) if r["block"] == 1]
    assert sum(r["tokens"] for r in F.producer_schedule(b.frame[2:-4])) < C.ZP_TOKQ
    full = rounds[:-1]
    assert len(full) == 4
    for r in full:
        assert r["S"] == C.ZP_SMAX and r["depth"] == 63 and 1 not in r["on_grid"], r
        assert r["on_grid"][0] == 0 and all(i % 11 == 0 for i in r["on_grid"])


def test_zlib_decodes_the_three_incomplete_sets_it_accepts():
    cs = C.cases()
    for name, item in (("single_distance_code_of_1_bit", "incomplete:single_dist_code"),
                       ("hlit_257_hdist_1_hclen_5_no_distance_code", "incomplete:no_dist_code"),
                       ("literal_code_that_is_only_a_1_bit_end_of_block", "incomplete:eob_only_lit_code")):
        assert item in cs[name].census
        assert zlib.decompress(cs[name].frame) == cs[name].content


# Nothing here: zlib refuses every stream the kernels are meant to refuse.  (A case zlib turned
# out to decode would be named here and asserted to decode, not dropped.)
ZLIB_LENIENT = set()


@pytest.mark.parametrize("name", list(C.malformed()))
def test_zlib_verdict_on_malformed_stream(oracle, name):
    stream, dlen, code, guard = C.malformed()[name]
    assert guard[:3] in ("P: ", "C: ")
    got = zlib_verdict(stream, dlen)
    assert name not in ZLIB_LENIENT
    assert isinstance(got, str), "zlib decoded %d bytes" % len(got)
    assert any(m in got for m in C.ZLIB_MESSAGES[code]), got
    r, out = oracle.zlib_inflate(stream, dlen)
    assert r != 0 or len(out) != dlen


def test_the_four_newly_refused_sets_have_zlibs_messages():
    m = C.malformed()
    for name, msg in (("code_length_code_incomplete", "invalid code lengths set"),
                      ("literal_code_incomplete", "invalid literal/lengths set"),
                      ("distance_code_incomplete", "invalid distances set"),
                      ("literal_code_without_end_of_block", "invalid code -- missing end-of-block")):
        assert msg in zlib_verdict(m[name][0], m[name][1]), name


@pytest.mark.parametrize("name", list(C.truncated()))
def test_zlib_refuses_a_stream_cut_inside_a_huffman_block(name):
    stream, dlen = C.truncated()[name]
    assert isinstance(zlib_verdict(stream, dlen), str)


def test_gzip_and_blosc_cases(oracle):
    members, trailing = C.gzip_cases()
    for b in members:
        assert gzip.decompress(b.frame) == b.content
    d = zlib.decompressobj(31)
    assert d.decompress(trailing) == members[0].content and d.eof and len(d.unused_data) == 8
    import ctypes
    chunk, raw = C.blosc_case()
    out = ctypes.create_string_buffer(len(raw))
    rc = oracle.lib().pbxo_zarr_decode_chunk(1, chunk, ctypes.c_size_t(len(chunk)), out, ctypes.c_size_t(len(raw)))
    assert rc == 0 and out.raw == raw
