"""The hand-built zstd frames of test_zstd_frames_host.py (checked against libzstd and against
the coverage checklist) and test_gpu_zstd_frames.py (decoded by k_zarr_zstd).  Each case is named
for the path it is for; all of them are deterministic and built once per process."""
import numpy as np

import _zstd_frames as F
from _zstd_frames import Comp, O, build


def rnd(n, seed, top=256):
    return np.random.default_rng(seed).integers(0, top, n, dtype=np.uint8).tobytes()


def norm_of(nsym, log, lt1=(), zero=()):
    """A count vector over nsym symbols: -1 for `lt1`, 0 for `zero`, the rest shared out."""
    norm = [0] * nsym
    for s in lt1:
        norm[s] = -1
    free = [s for s in range(nsym) if s not in lt1 and s not in zero]
    left = (1 << log) - len(lt1)
    for s in free:
        norm[s] = left // len(free)
    norm[free[0]] += left - left // len(free) * len(free)
    return norm


def small_seqs(n, seed, have):
    """n small pseudo-random sequences valid after `have` output bytes; returns them and the
    literals they use plus a tail."""
    rng = np.random.default_rng(seed)
    seqs, nlit = [], 0
    for _ in range(n):
        ll, ml = int(rng.integers(0, 6)), int(rng.integers(3, 21))
        off = int(rng.integers(1, min(have + ll, 200) + 1))
        seqs.append((ll, O(off), ml))
        have += ll + ml
        nlit += ll
    return seqs, rnd(nlit + 5, seed + 1)


# ------------------------------------------------------------------------- well-formed
def _headers():
    body = [("raw", rnd(40, 1)), Comp(rnd(9, 2), [(4, O(17), 6), (3, 1, 4)])]
    big = [("raw", rnd(300, 3)), Comp(rnd(9, 4), [(4, O(290), 6), (3, 1, 4)])]
    return {
        "hdr_fcs1_single_segment": build(body, fcs=1),
        "hdr_fcs2_plus256_single_segment": build(big, fcs=2, checksum=True),
        "hdr_fcs2_minimum_256": build([("raw", rnd(256, 5))], fcs=2),
        "hdr_fcs2_window_descriptor": build(big, fcs=2, single=False),
        "hdr_fcs4_checksum": build(big, fcs=4, checksum=True),
        "hdr_fcs8": build(big, fcs=8),
        "hdr_no_content_size_window_descriptor": build(big, fcs=0, checksum=True),
    }


def _blocks_and_repeats():
    pre = ("raw", rnd(64, 10))
    allrep = Comp(rnd(40, 11), [
        (5, O(10), 4),   # new offset
        (3, 1, 5),       # case 0: rep1
        (2, 2, 4),       # case 1: rep2
        (1, 3, 4),       # case 2: rep3
        (2, O(33), 3),
        (0, 1, 4),       # ll == 0: value 1 is rep2
        (0, 2, 4),       # ll == 0: value 2 is rep3
        (2, O(21), 3),
        (0, 3, 5),       # ll == 0: value 3 is rep1 - 1
        (4, 1, 6)])
    across = [
        pre, Comp(rnd(12, 12), [(3, O(20), 5), (2, O(31), 4), (1, O(7), 3)]),
        Comp(rnd(6, 13), [(2, 2, 6), (1, 1, 4)]),            # history from the compressed block before
        ("rle", 0xA5, 37),
        Comp(rnd(6, 14), [(0, 1, 5), (2, 3, 4)]),            # ... across an RLE block (ll == 0 first)
        ("raw", rnd(21, 15)),
        Comp(rnd(8, 16), [(3, 3, 7), (0, 3, 4)]),            # ... across a raw block
        ("raw", b""), ("rle", 7, 1)]
    return {
        "rep_all_four_cases_and_ll0_shift": build([pre, allrep]),
        "rep_history_across_compressed_rle_and_raw_blocks": build(across),
    }


def _nseq_forms():
    out = {}
    s, lits = small_seqs(127, 20, 64)
    out["nseq_1byte_127"] = build([("raw", rnd(64, 21)), Comp(lits, s)])
    s, lits = small_seqs(128, 22, 64)
    out["nseq_2byte_128"] = build([("raw", rnd(64, 23)), Comp(lits, s)])
    s, lits = small_seqs(5, 24, 64)
    out["nseq_2byte_form_for_5"] = build([("raw", rnd(64, 25)), Comp(lits, s, nseq_bytes=2)])
    # the 2-byte form's last count and the 3-byte form: cycles of eight sequences through every
    # repeat-offset case, 1 KiB of noise in front
    for name, n in (("nseq_2byte_0x7EFF", 0x7EFF), ("nseq_3byte_32600", 32600)):
        rng = np.random.default_rng(n)
        seqs = []
        while len(seqs) < n:
            a, b = (int(x) for x in rng.integers(16, 900, 2))
            seqs += [(1, O(a), 3), (1, O(b), 3), (1, 1, 3), (0, 1, 3), (1, 2, 3), (1, 3, 3), (0, 2, 3), (0, 3, 3)]
        seqs = seqs[:n]
        out[name] = build([("raw", rnd(1024, n + 1)), Comp(rnd(sum(x[0] for x in seqs) + 3, n + 2), seqs)])
    return out


def _wide_sequences():
    """T = the bits one sequence reads: offset code + both lengths' extra bits + the three state
    updates.  Predefined tables: LL code 34 and ML codes 51 / 52 are "less than 1" symbols (6 bits
    each), offset codes 9, 10 and 16 have count 1 (5 bits): 17 bits of updates."""
    out = {}
    for name, pre, ll, off, ml, T in (
            ("T56_read64_limit", 4096, 32768 + 1234, 509 + 77, 32771 + 4321, 56),
            ("T57_first_split_read", 4096, 32768 + 30000, 1021 + 1000, 32771 + 29000, 57),
            ("T64_split_read", 70000, 32768 + 777, 65533 + 3000, 65539 + 20000, 64)):
        seqs = [(ll, O(off), ml), (3, O(40), 9), (2, 2, 5)]
        b = build([("raw", rnd(pre, T)), Comp(rnd(ll + 9, T + 1), seqs)])
        assert "max_T:%d" % T in b.census, (name, [c for c in b.census if c.startswith("max_T")])
        out[name] = b
    # accuracy logs 9 / 8 / 9 with "less than 1" symbols for the wide codes: 16 + 16 + 15 extra bits
    # and 9 + 9 + 8 bits of updates
    ll_n = norm_of(36, 9, lt1=(34, 35))
    of_n = norm_of(17, 8, lt1=(16,), zero=(10, 11, 12, 13, 14, 15))
    ml_n = norm_of(53, 9, lt1=(50, 51, 52))
    seqs = [(32768 + 5, O(65533 + 11), 65539 + 13), (3, O(40), 9), (2, 2, 5), (1, O(5), 40)]
    b = build([("raw", rnd(70000, 73)), Comp(rnd(32768 + 5 + 9, 74), seqs,
                                             modes=(("fse", ll_n, 9), ("fse", of_n, 8), ("fse", ml_n, 9)))])
    assert "max_T:73" in b.census
    out["T73_fse_tables_at_accuracy_logs_9_8_9"] = b
    return out


def _table_modes():
    pre = ("raw", rnd(64, 30))
    same = [(2, O(5), 7), (2, O(6), 7), (2, O(7), 7)]  # one code per table: LL 2, OF 3, ML 4
    ll_n = norm_of(20, 6, lt1=(16, 19), zero=(17, 18))
    of_n = norm_of(11, 5, lt1=(10,), zero=(1, 2, 3, 4, 5, 6, 7, 8))  # zero run of 8: flags 3, 3, 2
    ml_n = norm_of(40, 7, lt1=(39,), zero=tuple(range(28, 35)))
    fse = (("fse", ll_n, 6), ("fse", of_n, 5), ("fse", ml_n, 7))
    mixed = [(3, O(600), 30), (16, O(1100), 42), (0, 1, 3), (17, 1, 60), (1, O(700), 4)]
    three = ("repeat", "repeat", "repeat")
    s1, l1 = small_seqs(20, 31, 64)
    s2, l2 = small_seqs(20, 32, 400)
    seq = [pre,
           Comp(l1, s1),                                        # predefined
           Comp(l2, s2, modes=three),                            # repeat of predefined
           Comp(rnd(8, 33), same, modes=("rle", "rle", "rle")),
           Comp(rnd(7, 34), same, modes=three),                   # repeat of RLE
           ("raw", rnd(1200, 35)),
           Comp(rnd(40, 36), mixed, modes=fse),
           Comp(rnd(11, 37), [], lit="raw"),                      # nseq == 0: literals only
           Comp(rnd(40, 38), mixed, modes=three)]                 # repeat of FSE, across the block above
    combos = {}
    for name, modes in (("predef_rle_fse", ("predef", "rle", fse[2])), ("fse_predef_rle", (fse[0], "predef", "rle")),
                        ("rle_fse_predef", ("rle", fse[1], "predef"))):
        s = [(2, O(5), 7), (2, O(6), 7)] if "rle" == modes[0] else [(16, O(5), 7), (3, O(6), 7)]
        if modes[1] == fse[1]:
            s = [(s[0][0], O(600), 7), (s[1][0], 1, 7)]
        if modes[2] == fse[2]:
            s = [(s[0][0], s[0][1], 42), (s[1][0], s[1][1], 3)]
        combos["modes_" + name] = build([("raw", rnd(700, 39)), Comp(rnd(40, 40), s, modes=modes)])
    combos["modes_predefined_rle_fse_and_repeat_of_each"] = build(seq)
    return combos


def _literals():
    out = {}
    tail = [(3, O(9), 5), (2, 1, 4)]
    pre = ("raw", rnd(32, 50))
    for mode, byte in (("raw", None), ("rle", 0x5A)):
        for sf, n in ((0, 31), (2, 17), (1, 4095), (3, 4096), (3, 20)):
            lits = rnd(n, 51 + n) if byte is None else bytes([byte]) * n
            out["lit_%s_size_format_%d_%dB" % (mode, sf, n)] = build([pre, Comp(lits, tail, lit=mode, lit_sf=sf)])
    w16 = [1] * 16                      # 15 listed weights (odd), table log 4
    w5 = [2, 2, 1, 1, 2]                # 4 listed weights (even), table log 3
    w11 = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]  # table log 11
    out["huf_1stream_direct_odd_weights"] = build([pre, Comp(rnd(200, 60, 16), tail, lit="huf", weights=w16)])
    out["huf_1stream_direct_even_weights"] = build([pre, Comp(rnd(100, 61, 5), tail, lit="huf", weights=w5)])
    out["huf_4stream_10bit_sizes"] = build([pre, Comp(rnd(1001, 62, 16), tail, lit="huf", weights=w16, lit_sf=1)])
    out["huf_4stream_14bit_sizes"] = build([pre, Comp(rnd(6001, 63, 16), tail, lit="huf", weights=w16, lit_sf=2)])
    out["huf_4stream_18bit_sizes"] = build([pre, Comp(rnd(17003, 64, 16), tail, lit="huf", weights=w16, lit_sf=3)])
    out["huf_4stream_shortest_6_literals"] = build([pre, Comp(rnd(6, 65, 16), [(3, O(9), 5)], lit="huf",
                                                              weights=w16, lit_sf=1)])
    skew = np.random.default_rng(66).choice(12, 3000, p=[2 ** -(k + 1) for k in range(11)] + [2 ** -11])
    out["huf_table_log_11"] = build([pre, Comp(bytes(skew.astype(np.uint8)), tail, lit="huf", weights=w11, lit_sf=2)])
    # FSE-compressed weights: 42 listed weights leave the two-state loop after a state-1 update,
    # 43 after a state-2 update
    wa = [1] * 32 + [2] * 8 + [3] * 2 + [4]
    wb = [1] * 32 + [2] * 8 + [3] * 2 + [0] + [4]
    la = np.random.default_rng(67).choice(43, 900).astype(np.uint8).tobytes()
    lb = np.random.default_rng(68).choice([s for s in range(44) if s != 42], 900).astype(np.uint8).tobytes()
    out["huf_fse_weights_exit_after_state1"] = build([pre, Comp(la, tail, lit="huf", weights=wa,
                                                                tree=("fse", [0, 44, 12, 8], 6))])
    out["huf_fse_weights_exit_after_state2"] = build([pre, Comp(lb, tail, lit="huf", weights=wb, lit_sf=1,
                                                                tree=("fse", [-1, 21, 6, 4], 5))])
    out["huf_treeless_across_blocks_and_raw_and_rle_literals"] = build([
        pre,
        Comp(rnd(300, 70, 16), tail, lit="huf", weights=w16),
        Comp(rnd(150, 71, 16), tail, lit="treeless"),
        Comp(rnd(50, 72), tail, lit="raw"),
        Comp(rnd(1000, 73, 16), tail, lit="treeless", lit_sf=1),
        ("rle", 3, 10),
        Comp(b"\x09" * 40, tail, lit="rle"),
        Comp(rnd(99, 74, 16), [], lit="treeless")])
    return out


RING_PRE, RING_LITS = 4200, 80


def ring_frame(off, phase):
    """One match of offset `off` that starts `phase` bytes into the batch's first 64-byte step and
    runs through five steps, then a repeat of it; every frame decodes to the same length."""
    lits = rnd(RING_LITS, 1000 * phase + off)
    return build([("raw", rnd(RING_PRE, off * 64 + phase)), Comp(lits, [(phase, O(off), 300), (7, 1, 70)])])


def _ring():
    out = {}
    for off in F.RING_OFFSETS:
        for phase in range(64):
            out["ring_offset_%d_phase_%02d" % (off, phase)] = ring_frame(off, phase)
    per = []
    for k, p in enumerate((1, 2, 3, 7, 63, 64)):
        per += [(3 + k, O(p), 200 + 37 * k)]
    out["periods_1_2_3_7_63_64_through_several_steps"] = build([("raw", rnd(64, 80)), Comp(rnd(40, 81), per)])
    for n in (64, 65):
        s, lits = small_seqs(n, 82 + n, 64)
        out["batch_of_%d_sequences" % n] = build([("raw", rnd(64, 83)), Comp(lits, s)])
    runs = [(250, O(20), 5), (10, O(30), 4), (300, 1, 6), (700, O(100), 9), (0, O(3), 30), (511, 2, 3), (1, O(900), 64)]
    out["literal_runs_across_256B_windows"] = build([("raw", rnd(64, 84)), Comp(rnd(2400, 85), runs)])
    return out


def blosc_chunk_of_splits(builts):
    """A c-blosc 1.x chunk (the framing _zarr.blosc_encode writes: one block, byte shuffle,
    typesize = the number of splits, codec zstd) whose splits are the given frames.  Returns the
    chunk and the bytes it decodes to (the splits' contents, interleaved)."""
    ts, neb = len(builts), len(builts[0].content)
    assert neb >= 128 and all(len(b.content) == neb and 0 < len(b.frame) < neb for b in builts)
    nbytes = ts * neb
    body = b"".join(len(b.frame).to_bytes(4, "little") + b.frame for b in builts)
    chunk = bytes([2, 1, 0x1 | (4 << 5), ts]) + nbytes.to_bytes(4, "little") * 2 + \
        (20 + len(body)).to_bytes(4, "little") + (20).to_bytes(4, "little") + body
    raw = np.stack([np.frombuffer(b.content, np.uint8) for b in builts], axis=1).tobytes()
    return chunk, raw


def blosc_case():
    cs = cases()
    return blosc_chunk_of_splits([cs["ring_offset_4097_phase_05"], cs["ring_offset_4032_phase_63"]])


_cases = None


def cases():
    """name -> Built(frame, content, census) of every well-formed case."""
    global _cases
    if _cases is None:
        _cases = {}
        for part in (_headers, _blocks_and_repeats, _nseq_forms, _wide_sequences, _table_modes, _literals, _ring):
            for k, v in part().items():
                assert k not in _cases
                _cases[k] = v
    return _cases


# --------------------------------------------------------------------------- malformed
# name -> (frame, content size the frame is registered for, the decoder code k_zarr_zstd sets).
# The guard that stops each one, from reading kernels_zstd.hip / zarr_dev.h:
#   33  the sequence loop's `if (!exec_batch())`: exec_batch's `lp + TL > nlit` (literal lengths
#       past the block's literals) or seq_batch's `T > o.olen - op0` (more output than the
#       content size) or its ballot of `boff == 0 || boff > op0 + st0 + bll` (offset 0, offset
#       beyond the output so far); nothing is copied before those tests
#   36  after the blocks: `o.op != o.olen` (fewer bytes than the content size)
#   34  `br.pos != 0` after the last sequence (bits left over)
#   24  `nseq == 0` with `q != bend`
#   26  `modes & 3`
#   27 / 28 / 29  seq_table() < 0 for LL / OF / ML: a repeat with have == false, an RLE symbol
#       `s > max_sym`, read_ncount's `log > max_log` or its final `remaining != 1`
#   16  treeless literals with have_huf == false
#   15  read_huf_tree() == 0: `rest & (rest - 1)` (weights not completable), a weight > 12
#   17  huf_stream()'s `br.pos == 0` (one stream)
#   19  the jump table's `d2 > lend`
#   10  `bsize > ZSTD_LITBUF` for a compressed block
#   37  the content checksum
_malformed = None
OFFSET0 = "offset_0_from_rep1_minus_1"


def malformed():
    global _malformed
    if _malformed is not None:
        return _malformed
    pre = ("raw", rnd(8, 90))
    good = [(2, O(4), 10)]

    def bad(blocks, size, code, **kw):
        b = build(blocks, check=False, declared=size, **kw)
        return b.frame, size, code

    m = {}
    # RFC 8878 3.1.1.5: an offset of 0 is corrupt.  libzstd decodes it as offset 1; the kernel refuses.
    m[OFFSET0] = bad([pre, Comp(b"", [(0, 3, 4)])], 12, 33)
    m["offset_beyond_the_output_so_far"] = bad([pre, Comp(rnd(4, 91), [(2, O(50), 4)])], 16, 33)
    m["literal_lengths_past_the_literals"] = bad([pre, Comp(rnd(5, 92), [(4, O(2), 3), (4, 1, 3)])], 22, 33)
    m["more_bytes_than_the_content_size"] = bad([pre, Comp(rnd(2, 93), good)], 16, 33)
    m["fewer_bytes_than_the_content_size"] = bad([pre, Comp(rnd(2, 93), good)], 24, 36)
    m["bits_left_over_in_the_sequence_stream"] = bad([pre, Comp(rnd(2, 93), good, extra_zero_bits=3)], 20, 34)
    m["nseq_0_with_trailing_bytes"] = bad([pre, Comp(rnd(12, 94), [], tail=b"\0")], 20, 24)
    m["reserved_mode_bits"] = bad([pre, Comp(rnd(2, 93), good, modes_low_bits=1)], 20, 26)
    for k, kind in enumerate(F.KINDS):
        modes = tuple("repeat" if j == k else "predef" for j in range(3))
        m["repeat_mode_without_a_table_%s" % kind] = bad([pre, Comp(rnd(2, 93), good, modes=modes)], 20, 27 + k)
        modes = tuple("rle" if j == k else "predef" for j in range(3))
        m["rle_symbol_above_the_alphabet_%s_%d" % (kind, F.MAX_SYM[kind] + 1)] = bad(
            [pre, Comp(rnd(2, 93), good, modes=modes, rle_symbols={kind: F.MAX_SYM[kind] + 1})], 20, 27 + k)
    m["treeless_literals_without_a_tree"] = bad([pre, Comp(rnd(30, 95, 16), good, lit="treeless")], 48, 16)
    fse_ll = (("fse", None, None), "predef", "predef")
    m["ncount_accuracy_log_10_for_literal_lengths"] = bad(
        [pre, Comp(rnd(2, 93), good, modes=fse_ll, ncount_raw={"LL": F.write_ncount(norm_of(36, 10), 10)})], 20, 27)
    # (a count cannot exceed what is left of the table: the field's range ends there.  What a
    # description can do is run on past the alphabet: 41 counts for the 36 literal-length codes)
    m["ncount_counts_run_past_the_alphabet"] = bad(
        [pre, Comp(rnd(2, 93), good, modes=fse_ll, ncount_raw={"LL": F.write_ncount([1] * 40 + [24], 6)})], 20, 27)
    m["huffman_weights_not_completable_to_a_power_of_two"] = bad(
        [pre, Comp(rnd(30, 96, 3), good, lit="huf", listed_weights=[3, 1])], 48, 15)
    m["huffman_weight_13"] = bad([pre, Comp(rnd(30, 96, 3), good, lit="huf", listed_weights=[1, 13, 1])], 48, 15)
    m["huffman_stream_not_ending_at_bit_0"] = bad(
        [pre, Comp(rnd(30, 97, 16), good, lit="huf", weights=[1] * 16, huf_extra_zero_bits=2)], 48, 17)
    m["jump_table_past_the_literal_section"] = bad(
        [pre, Comp(rnd(40, 98, 16), good, lit="huf", weights=[1] * 16, lit_sf=1, jump_add=1000)], 58, 19)
    m["compressed_block_larger_than_128KiB"] = bad([pre, Comp(rnd(2, 93), good, pad_to=128 * 1024 + 1)], 20, 10)
    m["wrong_checksum"] = bad([pre, Comp(rnd(2, 93), good)], 20, 37, checksum=True, bad_checksum=True)
    _malformed = m
    return m


# --------------------------------------------------------------------------- checklist
# Every item must appear in the union of the censuses of cases(); none may be waived.
CHECKLIST = (
    # 1. the sequence loop's split reads (T > 56) and the last single read
    ["T:56", "T:57", "T:>57", "max_T:64", "max_T:73"]
    # 2. Number_of_Sequences forms
    + ["nseq:1B", "nseq:2B", "nseq:3B", "nseq:0"]
    # 3. repeat offsets
    + ["rep:case0", "rep:case1", "rep:case2", "rep:case1:ll0", "rep:case2:ll0", "rep:case3:ll0",
       "rep:first_sequence_after_compressed_block", "rep:first_sequence_after_rle_block",
       "rep:first_sequence_after_raw_block"]
    # 4. symbol-compression modes
    + ["%s:%s" % (k, m) for k in F.KINDS for m in ("predef", "rle", "fse", "repeat:predef", "repeat:rle",
                                                   "repeat:fse", "repeat:across_nseq0")]
    + ["fse:less_than_one", "fse:zero_run_3_3_r", "fse:max_log:LL", "fse:max_log:OF", "fse:max_log:ML"]
    # 5. literal sections
    + ["lit:%s:%dB" % (m, n) for m in ("raw", "rle") for n in (1, 2, 3)]
    + ["lit:huf:sf0:1stream", "lit:huf:sf1:4stream", "lit:huf:sf2:4stream", "lit:huf:sf3:4stream",
       "lit:treeless:sf0:1stream", "lit:treeless:sf1:4stream",
       "tree:direct:odd", "tree:direct:even", "tree:fse:exit_after_state1", "tree:fse:exit_after_state2",
       "huf:table_log_11", "treeless:after:huf", "treeless:after:huf+raw", "treeless:after:huf+raw+rle"]
    # 6. seq_batch boundaries for RING = 4096
    + ["ring:%d:phase%d" % (o, p) for o in F.RING_OFFSETS for p in range(64)]
    + ["period:%d:several_steps" % p for p in (1, 2, 3, 7, 63, 64)]
    + ["batch:64_sequences", "batch:65_sequences", "literal_run_crosses_256B_window"]
    # 7. frame headers
    + ["fcs:0B", "fcs:1B", "fcs:2B", "fcs:4B", "fcs:8B", "single_segment", "window_descriptor",
       "checksum:on", "checksum:off"]
    # (blocks)
    + ["block:raw", "block:rle", "block:compressed"]
)
