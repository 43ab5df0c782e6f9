"""Hand-built deflate streams for k_zarr_inflate2 and k_zarr_inflate (csrc/kernels_zarr.hip): every
case is the smallest stream that reaches the path it is named after.  CHECKLIST is what the union
of the censuses (tests/_deflate_frames.py: inflate) must contain; malformed() gives the refusals
with the decoder code each must set, from reading the kernels."""
import struct
import zlib

import numpy as np

import _deflate_frames as F
from _deflate_frames import M, build, dyn, fixed, staircase, stored

# The kernels' constants the cases are built around (test_deflate_frames_host.py reads the
# definitions and compares): kernels_zarr.hip "inflate, two-wave pipeline" and zarr_dev.h.
ZPLUT = 10        # the producer's first-level tables (zp_decode_at; longer codes: canon_lane)
ZLUT = 9          # k_zarr_inflate's first-level tables (decode_fast; longer codes: decode_sym)
ZP_SMAX = 256     # longest segment of a macro-round, bits
ZP_SEGTOK = 24    # tokens per segment aimed at
ZP_TOKQ = 2048    # FIFO tokens per stream
ZP_BATCH = 32     # the consumer waits for this many tokens (or the end)
ZP_RINGB = 16384  # the consumer's output ring: sources farther than ZP_RINGB - 64 come from HBM
ZP_WINB = 3072    # the producer's input window
ZR_INF = 32768    # k_zarr_inflate's ring: the whole window
KERNEL_CONSTANTS = dict(ZPLUT=ZPLUT, ZLUT=ZLUT, ZP_SMAX=ZP_SMAX, ZP_SEGTOK=ZP_SEGTOK, ZP_TOKQ=ZP_TOKQ,
                        ZP_BATCH=ZP_BATCH, ZP_RINGB=ZP_RINGB, ZP_WINB=ZP_WINB, ZR_INF=ZR_INF)
assert F.RING_DISTS == (ZP_RINGB - 65, ZP_RINGB - 64, ZP_RINGB - 63, ZP_RINGB - 1, ZP_RINGB, ZP_RINGB + 1,
                        ZR_INF - 1, ZR_INF)

PERIOD = 251                    # a prime: a source wrong by 1 or by 64 reads another byte
PREFIX = PERIOD + 127 * 258     # 33017 >= 32768 + 63 bytes of history


def rnd(n, seed, top=256):
    return np.random.RandomState(seed).randint(0, top, n).astype(np.uint8).tobytes()


def prefix_tokens(seed):
    """PREFIX bytes: PERIOD noise literals repeated by matches."""
    return list(rnd(PERIOD, seed)) + [M(258, PERIOD)] * 127


def used_dyn(tokens, **kw):
    """A dynamic block whose codes are complete and about flat over the symbols its tokens use."""
    ls = {256} | {t if isinstance(t, int) else t[0] for t in tokens}
    ds = {t[2] for t in tokens if not isinstance(t, int)}
    if len(ls) < 2:
        ls.add(0 if 0 not in ls else 1)
    while len(ds) < 2:
        ds.add(min(set(range(30)) - ds))
    return dyn(F.complete_lengths(ls, max(257, max(ls) + 1)), F.complete_lengths(ds, max(ds) + 1), tokens, **kw)


# 15 literals with codes of 1..15 bits (and the end of block at 15); the same for length and
# distance symbols
LITS15 = list(range(65, 80))
LL_LITS = staircase(LITS15 + [256], 257)
LL_LENS = staircase(list(range(257, 272)) + [256], 272)
DL_STAIR = staircase(list(range(16)), 16)
# the widest token: 'a' in 1 bit, length symbol 284 (5 extra bits) and the end of block in 15;
# distance symbols 29 and 28 (13 extra bits) in 15
LL_WIDE = staircase([97] + list(range(1, 14)) + [284, 256], 285)
LL_WIDE44 = staircase([97] + list(range(1, 14)) + [265, 256], 266)  # 265: 1 extra bit, base 11
DL_WIDE = staircase(list(range(14)) + [29, 28], 30)


def _framing():
    out = {}
    lit = lambda n, s: list(rnd(n, s))  # noqa: E731
    S, Fx, D = (lambda k: stored(rnd(5 + k, 10 + k))), (lambda k: fixed(lit(4, 20 + k))), \
        (lambda k: used_dyn(lit(6, 30 + k) + [M(4, 3)]))
    order = [S, S, Fx, Fx, D, D, S, D, Fx, S]  # every ordered pair of block types
    out["every_ordered_pair_of_block_types"] = build([f(k) for k, f in enumerate(order)])
    out["final_fixed_block"] = build([S(0), D(1), Fx(2)])
    out["final_dynamic_block"] = build([S(0), Fx(1), D(2)])
    # a fixed block after a byte boundary ends at bit phase (3 + 9k + 7) & 7 with k 9-bit literals
    for nxt, f in (("stored", S), ("fixed", Fx), ("dynamic", D)):
        blocks = []
        for k in range(8):
            blocks += [stored(b"\x5a"), fixed([200 + k] * k), f(k)]
        out["fixed_block_ends_at_every_bit_phase_then_%s" % nxt] = build(blocks + [stored(b"end")])
    for k in range(8):
        out["fixed_block_ends_at_bit_phase_%d_then_trailer" % ((k + 2) & 7)] = \
            build([stored(b"\xa5" * 9), fixed([201] * k + lit(8 - k, 40 + k))])
    blocks = []
    for k in range(40):
        t = lit(1 + k % 3, 50 + k)
        blocks.append(fixed(t) if k & 1 else used_dyn(t))
    out["forty_blocks_of_1_to_3_tokens"] = build(blocks)
    out["empty_fixed_and_dynamic_blocks"] = build([fixed([]), used_dyn([]), fixed([66]), used_dyn([]), fixed([])])
    out["stored_len_0_1_2_3_and_65535"] = build([stored(b""), stored(b"a"), stored(b"bc"), stored(b"def"),
                                                 stored(rnd(65535, 60)), stored(b"")])
    return out


# HLIT 286, HDIST 30, HCLEN 19; 16 x 3 / 6, 17 x 3 / 10, 18 x 11 / 138; a 16 that runs from the last
# literal/length lengths into the distance lengths; code-length codes of 7 bits (17 and 18)
HDR_LL = [8] * 10 + [0] * 162 + [6] * 9 + [7] * 105
HDR_DL = [7] * 4 + [4] * 5 + [5] * 21
HDR_ITEMS = [8, (16, 6), (16, 3), (17, 3), (17, 10), (18, 11), (18, 138)] + [6] * 9 + [7] * 102 + [(16, 5)] + \
    [7, 7, 4, (16, 4), 5, (16, 6), (16, 6), (16, 5), 5, 5, 5]
HDR_CL = [0] * 19
for _s, _n in ((7, 2), (5, 2), (0, 3), (8, 3), (4, 3), (6, 4), (16, 5), (15, 6), (17, 7), (18, 7)):
    HDR_CL[_s] = _n


def _headers():
    out = {}
    toks = [0, 5, 9, 172, 180, 181, 255, M(3, 1), M(258, 2), M(20, 9), M(10, 7)]
    out["hlit_286_hdist_30_hclen_19_and_every_repeat_form"] = build(
        [dyn(HDR_LL, HDR_DL, toks, items=HDR_ITEMS, cl=HDR_CL)])
    # HLIT 257, HDIST 1, HCLEN 5: the code-length code names only 0 and 8 (HCLEN 4 names no
    # non-zero length at all, so no valid block has it: malformed()["hclen_4"]); no distance code
    ll = [0] + [8] * 256
    out["hlit_257_hdist_1_hclen_5_no_distance_code"] = build([dyn(ll, [0], [1 + b % 255 for b in rnd(300, 70)])])
    # the incomplete sets zlib accepts
    out["single_distance_code_of_1_bit"] = build([used_dyn([1, 2, 3, 4]), dyn(
        F.complete_lengths({1, 2, 256, 257, 260}, 261), [1], [1, 2, 1, (257, 0, 0, 0), 2, (260, 0, 0, 0)])])
    out["literal_code_that_is_only_a_1_bit_end_of_block"] = build(
        [fixed([7, 8, 9]), dyn([0] * 256 + [1], [0], []), fixed([10])])
    return out


def _code_lengths():
    out = {}
    lits = [LITS15[b % 15] for b in rnd(200, 80)] + LITS15
    lens = []
    for k in range(15):
        lens += [(257 + k, 0, k, 0), (257 + k, 0, 15 - (k & 1), 0)]
    out["codes_of_every_length_1_to_15_in_both_alphabets"] = build(
        [dyn(LL_LITS, [0], lits), dyn(LL_LENS, DL_STAIR, lens * 3)])
    # complete codes whose short codes go unused: every token (and the end of block) is searched
    ll = [0] * 257
    for k in range(10):
        ll[k] = k + 1
    for s, n in ((100, 11), (101, 12), (102, 13), (103, 14), (256, 15)):
        ll[s] = n
    ll += [0] * 7 + [15]  # length symbol 264 (10)
    dl = [k + 1 for k in range(10)] + [11, 12, 13, 14, 15, 15]
    toks = []
    for k, b in enumerate(rnd(120, 81)):
        toks.append(100 + b % 4 if k % 3 else (264, 0, 10 + b % 6, (b >> 3) & 15))
    out["every_token_beyond_the_first_level_tables"] = build([stored(rnd(700, 82)), dyn(ll, dl, toks)])
    return out


def _widest():
    toks = []
    for phase in range(8):
        for le, de in ((31, 8191), (0, 0)):
            toks += [("phase", phase, 97), (284, le, 29, de), 97, 97, 97]
    return {"widest_token_48_bits_at_every_bit_phase": build([fixed(prefix_tokens(90)), dyn(LL_WIDE, DL_WIDE, toks)])}


def _tables():
    toks = []
    for ls in range(257, 286):
        toks += [(ls, 0, 0, 0), (ls, (1 << F.LEXT[ls - 257]) - 1, 0, 0)]
    for ds in range(30):
        toks += [(257, 0, ds, 0), (257, 0, ds, (1 << F.DEXT[ds]) - 1)]
    return {"every_length_and_distance_symbol_with_min_and_max_extra":
            build([fixed(prefix_tokens(91)), fixed(toks + [(284, 31, 3, 0), (285, 0, 3, 0)])])}


NTOK_SYNC = 3 * ZP_TOKQ
ITEMS7 = [7] + [(16, 6)] * 21 + [(18, 128), 8, 8, 0]
SERIAL = "periodic_44_bit_tokens_serial_pass_b_in_every_round"
SERIAL_PATTERN = [(265, 1, 29, 4435), (265, 1, 29, 7219)]


def _sync():
    out = {}
    # 255 literals at 8 bits, literal 255 and the end of block at 9.  Literals < 128 have a 0 at
    # the head of their code, so no 8-bit window is all ones and every chain decodes 8-bit tokens.
    # (Segments are multiples of 8 bits from the block's start, so here every lane starts ON a
    # token: the chains agree at once.  The block that keeps them apart is the 7-bit one below.)
    ll8 = [8] * 255 + [9, 9]
    blocks = []
    for phase in range(1, 8):
        d = dyn(ll8, [0], list(rnd(NTOK_SYNC, 100 + phase, 128)))
        blocks += [fixed([("phase", (phase - F.header_bits(d) - 7) & 7, 200)]), d]
    out["uniform_8_bit_tokens_from_every_bit_phase"] = build(blocks)
    # 127 codes of 7 bits, literal 255 and the end of block at 8.  Even literals < 64 have a 0 at
    # both ends of their code: no 7-bit window at any offset is all ones, so every chain decodes
    # 7-bit tokens for ever and one that is off the token grid never meets the true one.  That
    # holds for the FIRST macro-round only (S = 128: pass B hands the true chain on lane by lane,
    # 63 iterations; a lane that started on the grid loses its chain to the false one entering
    # it).  From the second round on S = 7 * ZP_SEGTOK = 168, a multiple of 7, and every lane
    # starts on a token (as for any uniform width of 3..10 bits): see the periodic block below.
    ll7 = [7] * 127 + [0] * 128 + [8, 8]
    out["uniform_7_bit_tokens_serial_pass_b_in_the_first_round"] = build(
        [dyn(ll7, [0], [2 * b for b in rnd(NTOK_SYNC, 108, 32)], items=ITEMS7)])
    # Two match tokens of 44 bits, repeated: the bit stream has a period of 88 bits, so the chain
    # from any bit is one of 88 orbits, and with these extra bits (found by search over the
    # model F.producer_schedule) none of the 86 false ones ever reaches a true token start.
    # At 44 bits a token S stays at ZP_SMAX = 256, and 256 * i is a multiple of 44 only for i =
    # 11 k: in EVERY macro-round lane 1 starts off the grid and pass B runs serially over all 64
    # lanes (63 iterations).  Fewer than ZP_TOKQ tokens in the whole stream, so the FIFO never
    # fills and the rounds are the model's whatever the consumer's pace.
    out[SERIAL] = build([fixed(prefix_tokens(93)), dyn(LL_WIDE44, DL_WIDE, SERIAL_PATTERN * 750)])
    out["one_bit_literals_more_than_the_fifo_per_round"] = build(
        [dyn(staircase([97, 98, 256], 257), [0], [97] * (4 * ZP_TOKQ))])
    toks = []
    for k in range(3):
        toks += [97] * ZP_TOKQ + [(265, b & 1, 29, 8191 - 7 * b) for b in rnd(256, 110 + k)]
    out["bits_per_token_swing_between_1_and_44"] = build([fixed(prefix_tokens(92)), dyn(LL_WIDE44, DL_WIDE, toks)])
    return out


def _matches():
    out = {}
    toks = list(rnd(64, 120))
    for d in range(1, 65):
        toks += [M(n, d) for n in F.MATCH_LENS]
    out["distances_1_to_64_with_lengths_3_63_64_65_258"] = build([fixed(toks)])
    toks = list(rnd(8, 121)) + [M(8, 8), M(10, 10)]
    plen = 10
    for b in rnd(300, 122):
        n, d = 3 + (b & 3), 1 + (b >> 2) % plen
        toks.append(M(n, d))
        plen = n
    out["chains_of_sources_inside_the_match_before"] = build([fixed(toks)])
    out["sixty_four_matches_of_258_in_one_batch"] = build([stored(rnd(300, 123)), fixed([M(258, 300)] * 64 + [1, 2, 3])])
    return out


RING_LEN = PREFIX + 2 + 63 + 258


def ring_frame(dist, phase):
    """A match of 258 at `dist` that starts `phase` bytes into the first step of its batch: the
    stored run before the block ends the batch before, and the block's tokens (<= 64) are
    published together.  Every frame decodes to RING_LEN bytes."""
    seed = 1000 * phase + dist
    return build([fixed(prefix_tokens(seed)), stored(rnd(2, seed + 1)),
                  fixed(list(rnd(phase, seed + 2)) + [M(258, dist)] + list(rnd(63 - phase, seed + 3)))])


def _ring():
    out = {}
    for dist in F.RING_DISTS:
        for phase in range(64):
            out["ring_dist_%d_phase_%02d" % (dist, phase)] = ring_frame(dist, phase)
    return out


def _fifo():
    out = {}
    for pos in (62, 63):
        out["stored_token_at_position_%d_of_a_batch" % pos] = build(
            [stored(rnd(300, 130)), fixed([M(258, 300)] * 64 + list(rnd(pos, 131))), stored(rnd(100, 132)),
             fixed(list(rnd(40, 133)))])
    out["stored_run_across_the_fifo_wrap_and_over_two_fifos_of_tokens"] = build(
        [fixed(list(rnd(ZP_TOKQ - 1, 134))), stored(rnd(70, 135)), fixed(list(rnd(ZP_TOKQ + 200, 136)))])
    for r in range(1, ZP_BATCH):
        out["tail_of_%02d_tokens_after_two_batches" % r] = build(
            [fixed(list(rnd(63 + r, 140 + r)) + [M(65 - r, 50)])])
    return out


_cases = None


def cases():
    """name -> Built(frame, content, census) of every well-formed case (zlib framing)."""
    global _cases
    if _cases is None:
        _cases = {}
        for part in (_framing, _headers, _code_lengths, _widest, _tables, _sync, _matches, _ring, _fifo):
            for k, v in part().items():
                assert k not in _cases
                _cases[k] = v
    return _cases


def small_cases():
    return [n for n in cases() if not n.startswith("ring_dist_")]


CHECKLIST = (
    ["block:%s:%s" % (t, f) for t in ("stored", "fixed", "dynamic") for f in ("final", "nonfinal")] +
    ["pair:%s>%s" % (a, b) for a in ("stored", "fixed", "dynamic") for b in ("stored", "fixed", "dynamic")] +
    ["huff_end_phase:%d>%s" % (p, n) for p in range(8) for n in ("stored", "fixed", "dynamic", "trailer")] +
    ["stored_pad_after_huffman:%d" % p for p in range(8)] +
    ["blocks_of_1_to_3_tokens:16", "empty_block:fixed", "empty_block:dynamic"] +
    ["stored_len:%d" % n for n in (0, 1, 2, 3, 65535)] +
    # HCLEN 4 names only 16, 17, 18 and 0, so no block with it has an end-of-block code: the
    # smallest well-formed HCLEN is 5, and HCLEN 4 is malformed()["hclen_4"]
    ["hlit:257", "hlit:286", "hdist:1", "hdist:30", "hclen:5", "hclen:19",
     "rep16:3", "rep16:6", "rep17:3", "rep17:10", "rep18:11", "rep18:138", "rep16_crosses_lit_dist", "clcode_len:7",
     "incomplete:single_dist_code", "incomplete:no_dist_code", "incomplete:eob_only_lit_code"] +
    ["%s_code_len:%d" % (a, n) for a in ("lit", "len", "dist") for n in range(1, 16)] +
    ["block:every_code_longer_than_the_tables"] +
    ["widest_token:phase:%d:extra:%s" % (p, e) for p in range(8) for e in ("ones", "zeros")] +
    ["lsym:%d:%s" % (s, t) for s in range(257, 286) for t in ("min", "max")] +
    ["dsym:%d:%s" % (s, t) for s in range(30) for t in ("min", "max")] +
    ["block:uniform_token_width:8:phase:%d" % p for p in range(1, 8)] +
    ["block:uniform_token_width:7", "block:two_token_period_of_88_bits"] +
    ["block:1bit_literals_beyond_the_fifo", "block:bits_per_token_swing_3_to_40"] +
    ["match:d%d:l%d" % (d, n) for d in range(1, 65) for n in F.MATCH_LENS] +
    ["match:sources_in_the_match_before:depth_4", "match:64_in_a_row_of_258", "match:dist_eq_len"] +
    ["ring:%d:phase:%d" % (d, p) for d in F.RING_DISTS for p in range(64)] +
    ["fifo:stored_token_at_index_62_mod_64", "fifo:stored_token_at_index_63_mod_64",
     "fifo:stored_pair_straddles_wrap", "fifo:more_than_2_tokq_tokens"] +
    ["fifo:tokens_mod_32:%d" % r for r in range(1, ZP_BATCH)])


# ------------------------------------------------------------------------------- malformed
# name -> (stream, decoded length registered, decoder code, guard).  The guard is where the code
# is set; how BOTH waves of k_zarr_inflate2 end for it:
#   producer-side (P): zp_producer leaves its block loop with `bad` set and puts the end token
#     0xC0000000 | bad (TokOut::room(1) returns at once or when the consumer frees a slot: the
#     consumer takes every token before the end token); the consumer reads it as `code` and ends.
#   consumer-side (C): zp_consumer sets `code`, `done`, stores ZPC_ABORT and leaves.  The producer
#     goes on decoding (its bit reader feeds zeros past the input, zp_huff_block refuses `q >
#     ilen` with 26, every macro-round advances by >= 1 token) until the stream's last block or
#     an error, and TokOut::room returns false on ZPC_ABORT whenever the FIFO is full.
# k_zarr_inflate is one wave: every guard is a `break` out of its block loop.  It checks no
# Adler-32 (28 / 29 are the known difference of that A/B path, not run there) and is never given
# a gzip member (31).
# A stream cut INSIDE a Huffman block decodes the bytes that follow it in the upload buffer, so
# its code depends on them: truncated() cases assert only the refusal.
_malformed = None


def _raw(blocks):
    return build(blocks, wrap="raw", check=False, census=False).frame


def _z(body, content=None, adler=None, header=None):
    a = zlib.adler32(content) if adler is None else adler
    return (F.zlib_header() if header is None else header) + body + struct.pack(">I", a)


def malformed():
    global _malformed
    if _malformed is not None:
        return _malformed
    m = {}
    ok = build([fixed(list(b"hello, world"))], wrap="raw")
    n = len(ok.content)

    def hdr(name, **kw):
        m[name] = (_z(ok.frame, ok.content, header=F.zlib_header(**kw)), n, 10, "P: the RFC 1950 header test")
    hdr("header_cm_7", cm=7)
    hdr("header_cinfo_8", cinfo=8)
    hdr("header_fdict", fdict=1)
    hdr("header_bad_fcheck", fcheck=3)
    m["stored_nlen_mismatch"] = (_z(_raw([stored(b"abcd", nlen=0x1234)]), b"abcd"), 4, 11, "P: len ^ 0xffff != nlen")
    m["stored_run_outruns_the_input"] = (_z(_raw([stored(b"abcd", len_=4000)]), b"abcd"), 4000, 12,
                                         "P: q + len > ilen")
    m["stored_run_outruns_the_output"] = (_z(_raw([stored(b"abcdefgh")]), b"abcdefgh"), 6, 12,
                                          "C: len > olen - op at the stored-run token")
    w = F.BitWriter()
    w.put(1, 1), w.put(3, 2), w.align()
    m["block_type_3"] = (_z(bytes(w.out), b""), 4, 13, "P: type == 3")
    lits = [1, 2, 3]
    for name, hl, hd in (("hlit_287", 287, 2), ("hlit_288", 288, 2), ("hdist_31", 257, 31), ("hdist_32", 257, 32)):
        b = dyn([8] * 256 + [8] + [0] * (hl - 257), [1, 1] + [0] * (hd - 2), lits)
        m[name] = (_z(_raw([b]), bytes(lits)), 3, 14, "P: hlit > 286 || hdist > 30")
    good_ll, good_dl = [0] + [8] * 256, [1, 1]
    cl_over = [0] * 19
    cl_over[0] = cl_over[8] = cl_over[1] = 1
    m["code_length_code_over_subscribed"] = (_z(_raw([dyn(good_ll, good_dl, lits, cl=cl_over)]), bytes(lits)), 3, 15,
                                             "P: build_table(ct) over-subscribed")
    m["literal_code_over_subscribed"] = (_z(_raw([dyn([7] + [8] * 256, good_dl, lits)]), bytes(lits)), 3, 19,
                                         "P: build_table(lt) over-subscribed")
    m["distance_code_over_subscribed"] = (_z(_raw([dyn(good_ll, [1, 1, 1], lits)]), bytes(lits)), 3, 20,
                                          "P: build_table(dt) over-subscribed")
    cl = F.complete_lengths({0, 8, 16, 1}, 19)
    m["repeat_16_first"] = (_z(_raw([dyn(good_ll, good_dl, lits, items=[(16, 3)] + [8] * 254 + [1, 1], cl=cl)]),
                               bytes(lits)), 3, 17, "P: sym == 16 with k == 0")
    m["repeat_overruns_the_length_count"] = (
        _z(_raw([dyn(good_ll, good_dl, lits, items=[0] + [8] * 256 + [1, (16, 3)], cl=cl)]), bytes(lits)), 3, 18,
        "P: k + rep > hlit + hdist")
    eob_only = dyn([0] * 256 + [1], [0], [], eob=False)
    w = F.BitWriter()
    F.write_deflate(w, [eob_only], bytearray())
    w.put(1, 1)  # the unassigned 1-bit code
    w.align()
    m["unassigned_literal_code_of_the_1_bit_set"] = (_z(bytes(w.out), b""), 4, 21,
                                                     "P: zp_decode_at e == 0xFFFF after canon_lane (ZK_BAD 21)")
    for s in (286, 287):
        m["length_symbol_%d_in_a_fixed_block" % s] = (_z(_raw([fixed([65, 66, s, 67])]), b"ABC"), 3, 23,
                                                      "P: zp_decode_at ls >= 29 (ZK_BAD 23)")
    for d in (30, 31):
        m["distance_symbol_%d_in_a_fixed_block" % d] = (_z(_raw([fixed([65, 66, (257, 0, d, 0), 67])]), b"ABC"), 6, 24,
                                                        "P: zp_decode_at de == 0xFFFF (ZK_BAD 24)")
    m["match_in_a_block_without_a_distance_code"] = (
        _z(_raw([dyn(F.complete_lengths({65, 256, 257}, 258), [0], [65, 65, (257, 0, None, 0)], eob=False)]), b"AA"),
        5, 24, "P: zp_decode_at de == 0xFFFF: every distance entry is unassigned (ZK_BAD 24)")
    m["distance_past_the_start_at_output_0"] = (_z(_raw([fixed([M(3, 1), 65])]), b""), 4, 25,
                                                "C: dist > op0 + start")
    m["distance_past_the_start_in_mid_batch"] = (_z(_raw([fixed(list(b"0123456789") + [M(3, 11), 65])]), b""), 14, 25,
                                                 "C: dist > op0 + start")
    over = build([fixed(list(b"0123456789") + [M(20, 5)])], wrap="raw")
    m["match_overruns_the_output"] = (_z(over.frame, over.content), 25, 25,
                                      "C: T > olen - op0 in a batch with a match")
    m["literal_overruns_the_output"] = (_z(_raw([fixed(list(b"0123456789"))]), b"0123456789"), 9, 22,
                                        "C: T > olen - op0 in a batch of literals")
    m["stream_ends_short_of_the_chunk"] = (_z(_raw([fixed(list(b"0123456789"))]), b"0123456789"), 11, 27,
                                           "C: o.op != o.olen after the end token")
    m["trailer_cut"] = (_z(_raw([fixed(list(b"0123456789"))]), b"0123456789")[:-2], 10, 28, "P: q + 4 > ilen")
    for k in (1, 255, 256, 257, 70000):
        data = (rnd(PERIOD, 150 + k) * (k // PERIOD + 1))[:k]
        toks = list(data[:PERIOD])
        while len(toks) < PERIOD + (k - PERIOD) // 258 and k > PERIOD:
            toks.append(M(258, PERIOD))
        rest = k - min(k, PERIOD) - 258 * (len(toks) - PERIOD) if k > PERIOD else 0
        if rest >= 3:
            toks.append(M(rest, PERIOD))
        elif rest:
            toks += list(data[k - rest:])
        b = build([fixed(toks)], wrap="raw")
        assert b.content == data
        m["wrong_adler32_of_%d_bytes" % k] = (_z(b.frame, adler=zlib.adler32(data) ^ 0x00010000), k, 29,
                                              "C: o.adler32() != the trailer")
    # the sets zlib's inflate_table refuses and build_table used to take
    cl_inc = [0] * 19
    cl_inc[0], cl_inc[8], cl_inc[1] = 1, 2, 3
    m["code_length_code_incomplete"] = (_z(_raw([dyn(good_ll, good_dl, lits, cl=cl_inc)]), bytes(lits)), 3, 15,
                                        "P: build_table(ct, strict): left > 0")
    m["literal_code_incomplete"] = (_z(_raw([dyn([0] * 2 + [8] * 255, good_dl, [2, 3, 4])]), bytes([2, 3, 4])), 3, 19,
                                    "P: build_table(lt): left > 0 with a code longer than 1 bit")
    m["distance_code_incomplete"] = (_z(_raw([dyn(good_ll, [2, 2, 2], lits)]), bytes(lits)), 3, 20,
                                     "P: build_table(dt): left > 0 with a code longer than 1 bit")
    m["literal_code_without_end_of_block"] = (
        _z(_raw([dyn([8] * 256 + [0], good_dl, lits, eob=False)]), bytes(lits)), 3, 19, "P: lens[256] == 0")
    m["hclen_4"] = (_z(_raw([dyn([0] * 257, [0], [], items=[(18, 138), (18, 120)], cl=[1, 0, 0] + [0] * 15 + [1],
                                 hclen=4, eob=False)]), b""), 3, 19, "P: lens[256] == 0")
    _malformed = m
    return m


# zlib's message for each decoder code (the host test pins the class of every case)
ZLIB_MESSAGES = {
    10: ("incorrect header check", "invalid window size", "unknown compression method",
         "Error 2 while"),  # (Z_NEED_DICT)
    11: ("invalid stored block lengths",), 12: ("incomplete or truncated", "length"), 13: ("invalid block type",),
    14: ("too many length or distance symbols",), 15: ("invalid code lengths set",),
    17: ("invalid bit length repeat",), 18: ("invalid bit length repeat",),
    19: ("invalid literal/lengths set", "invalid code -- missing end-of-block"), 20: ("invalid distances set",),
    21: ("invalid literal/length code",), 23: ("invalid literal/length code",), 24: ("invalid distance code",),
    25: ("invalid distance too far back", "length"), 22: ("length",), 27: ("length",),
    28: ("incomplete or truncated",), 29: ("incorrect data check",)}
ONE_WAVE_SKIPS = (28, 29)  # k_zarr_inflate checks no trailer


def truncated():
    """name -> (stream, decoded length): cut inside a Huffman block; the refusal's code is not fixed."""
    b = cases()["distances_1_to_64_with_lengths_3_63_64_65_258"]
    c = cases()["uniform_7_bit_tokens_serial_pass_b_in_the_first_round"]
    return {"fixed_block_cut_in_the_middle": (b.frame[:len(b.frame) // 2], len(b.content)),
            "dynamic_block_cut_in_the_middle": (c.frame[:len(c.frame) // 2], len(c.content))}


def gzip_cases():
    """Two gzip members (the v3 route) and the code-31 refusal: bytes after the trailer that end in
    a second copy of it, so that the host's ISIZE test passes and the device's does not."""
    blocks = [fixed(prefix_tokens(160)[:PERIOD + 3]), stored(b"gz"),
              dyn(LL_LITS, [0], [LITS15[b % 15] for b in rnd(99, 161)])]
    a = build(blocks, wrap="gzip")
    b = build([used_dyn(list(rnd(60, 162)) + [M(258, 17)] * 4 + [M(34, 60)])], wrap="gzip")
    assert len(a.content) == len(b.content)
    return [a, b], a.frame + a.frame[-8:]


def blosc_case():
    """A c-blosc 1 chunk (one block, byte shuffle, typesize 2, codec zlib) whose two splits are
    hand-built zlib streams; (chunk, the bytes it decodes to)."""
    cs = cases()
    builts = [cs["ring_dist_16321_phase_05"], cs["ring_dist_32768_phase_63"]]
    ts, neb = len(builts), len(builts[0].content)
    assert all(len(b.content) == neb and 0 < len(b.frame) < neb for b in builts)
    body = b"".join(len(b.frame).to_bytes(4, "little") + b.frame for b in builts)
    chunk = bytes([2, 1, 0x1 | (3 << 5), ts]) + (ts * neb).to_bytes(4, "little") * 2 + \
        (20 + len(body)).to_bytes(4, "little") + (20).to_bytes(4, "little") + body
    raw = np.stack([np.frombuffer(b.content, np.uint8) for b in builts], axis=1).tobytes()
    return chunk, raw
