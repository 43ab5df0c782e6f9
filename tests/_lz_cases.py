"""Hand-built LZ4 and BloscLZ streams for k_zarr_lz4 and k_zarr_blosclz (csrc/kernels_zarr.hip,
csrc/zarr_dev.h): every case is a small stream that reaches the path it is named after, which the
census of the schedule model (tests/_lz_frames.py) confirms.  LZ4_CHECKLIST / BLZ_CHECKLIST are
what the union of the censuses must contain; lz4_malformed() / blz_malformed() give the refusals
with the decoder code each must set, from reading the kernels.

Every stream must be strictly shorter than its content (the blosc frame reads csize == blocksize
as stored and refuses csize > blocksize), so every case carries one long "fill" match that also
brings its content to one of a few lengths: cases of equal length share a frame and a launch.

Lines of the checklist that cannot be built, and why:
  * LZ4 "a stream that is one literal-only sequence": its token and extension bytes make it longer
    than its content, which the frame rule refuses before any kernel runs.
  * LZ4 "remainders up to 259 in the batch": a match joins the batch only up to JOIN_MAX = 256
    bytes, so the largest remainder r - s_ll in seq_batch is 255; 255 is covered.
  * BloscLZ code 1 (empty stream): the planner refuses a split of size 0 before the kernel.
  * BloscLZ code 6 (OutRing::match refuses): the guard of code 5 tests the same two conditions
    first and a BloscLZ distance is never 0, so no stream reaches it.
  * BloscLZ "ending on a match": a match in the short near form whose distance byte is the
    stream's last byte stops at the guard of code 3 (as c-blosc's `ip + 1 >= ip_limit` does); only
    a match with extension bytes or in the far form is parsed to its end and then not copied
    (code 8).  Both are among the refusals."""
from collections import namedtuple

import numpy as np

import _lz_frames as F
from _lz_frames import BFill, Fill, L, M, S

KERNEL_CONSTANTS = dict(ZWIN=F.ZWIN, ZR_LZ4=F.ZR_LZ4)

A = 6144                  # most cases
A_LENGTHS = (A - 1, A, A + 1)   # content ending one byte before, on, and one byte after a 256-byte flush boundary
B = 74 * 1024             # the far cases: BloscLZ distances reach 8192 + 65535
assert A % 256 == 0 and B % 256 == 0

Case = namedtuple("Case", "stream content census counts")


def noise(n, seed):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


TAIL = 16  # final literals that keep liblz4's end rules (last 5 bytes literal, last match 12 from the end)


def lz4_case(seqs, length=A):
    stream, content = F.lz4_build(seqs, length)
    code, census, counts = F.lz4_schedule(stream, length)
    assert code == 0, code
    return Case(stream, content, census, counts)


def blz_case(ops, length=A):
    stream, content = F.blz_build(ops, length)
    code, census, counts = F.blosclz_schedule(stream, length)
    assert code == 0, code
    return Case(stream, content, census, counts)


HEAD = S(noise(64, 1), 17, 8)   # 64 literals of history (a serial sequence: first of its round)


def _x0_head(x0, extra=0):
    """A first sequence (per-sequence path: the window stays at 0) after which, and after `extra`
    more stream bytes, ip = x0."""
    n0 = x0 - extra - 9  # token, 4 extension bytes, n0 literals, offset, 2 match-extension bytes
    assert 15 + 3 * 255 <= n0 < 15 + 4 * 255
    return S(noise(n0, 2), 97, 300)


SHORT3 = [S(noise(1, 70 + k), 6, 4) for k in range(3)]  # 12 stream bytes: a pending batch


# ------------------------------------------------------------------------------------- LZ4
def _lz4_small():
    out = {}
    fill = Fill(noise(3, 3), 61)
    end = S(noise(TAIL, 4))
    out["literal_lengths_0_1_14_15_16_269_270_525"] = lz4_case(
        [HEAD] + [S(noise(n, 10 + k), 29, 5) for k, n in enumerate((0, 1, 14, 15, 16, 269, 270, 525))] + [fill, end])
    out["literals_and_matches_at_the_join_limit_256_and_257"] = lz4_case(
        [S(noise(256, 20), 31, 8), S(noise(257, 21), 31, 8), S(noise(3, 22), 31, 256), S(noise(3, 23), 31, 257),
         fill, end])
    out["literal_run_across_window_reloads"] = lz4_case([HEAD, S(noise(2500, 24), 100, 8), fill, end])
    # 950 literals from ls = 5 stay inside the first window; ip = 959 afterwards does not
    out["window_reloaded_after_a_per_sequence_copy"] = lz4_case(
        [S(noise(950, 25), 40, 300)] + SHORT3 + [fill, end])
    out["match_lengths_4_18_19_273_274"] = lz4_case(
        [HEAD] + [S(noise(2, 30 + k), 23, m) for k, m in enumerate((4, 18, 19, 273, 274))] + [fill, end])
    out["match_above_1024_near"] = lz4_case([HEAD, S(noise(1, 35), 40, 1500), fill, end])
    out["matches_above_1024_far"] = lz4_case(
        [Fill(noise(251, 36), 251), S(noise(2, 37), 5000, 2500), S(noise(1, 38), 65535, 1500), end], B)
    # source [p - 4097, p - 3073) with p = 2 (mod 256): the run that holds its last byte was flushed 11
    # flush stores before the load (12 for p = 0, 1): the tightest the vmcnt(8) wait is ever asked
    out["far_match_of_1024_at_4097_eleven_stores_after_its_source"] = lz4_case(
        [Fill(noise(251, 39), 251), S(b"", 4097, 1024), S(noise(238 + TAIL, 40))])
    # rounds
    out["rounds_of_22_sequences_and_a_batch_cut_at_64"] = lz4_case(
        [HEAD] + [S(b"", 7, 4)] * 200 + [fill, end])
    out["rounds_of_4_sequences"] = lz4_case([HEAD] + [S(noise(14, 100 + k), 19, 4) for k in range(100)] + [fill, end])
    out["batch_reaches_64_from_a_serial_join"] = lz4_case(
        [Fill(noise(64, 41), 17)] + [S(b"", 7, 4)] * 63 + [S(noise(15, 42), 9, 5)] + [S(b"", 11, 6)] * 5 + [end])
    out["serial_sequence_is_the_last_candidate"] = lz4_case(
        [Fill(noise(64, 43), 17)] + [S(b"", 7, 4)] * 21 + [S(noise(20, 44), 9, 5), end])
    # the window end inside each field of a serial header (the window starts at 0, ip <= 940)
    t = lambda ml: S(noise(100, 45), 50, ml)  # noqa: E731  (token, 1 extension byte, 100 literals, offset ...)
    for name, x0, ml in (("offset_low_byte", 922, 8), ("offset_high_byte", 921, 8), ("match_extension", 920, 40)):
        out["window_ends_before_the_%s_with_a_pending_batch" % name] = lz4_case(
            [_x0_head(x0, 12)] + SHORT3 + [t(ml), fill, end])
    out["window_ends_inside_the_literal_extension_with_a_pending_batch"] = lz4_case(
        [_x0_head(940, 12)] + SHORT3 + [S(noise(15 + 255 * 90 + 7, 46), 50, 8), Fill(b"", 61), end], B)
    out["serial_sequence_kept_from_the_batch_by_the_window_end_only"] = lz4_case(
        [_x0_head(910, 12)] + SHORT3 + [t(8), fill, end])
    # periods
    for g in range(4):
        offs = range(16 * g + 1, 16 * g + 17)
        out["batch_periods_%d_to_%d_of_256" % (offs[0], offs[-1])] = lz4_case(
            [Fill(noise(80, 50 + g), 70)] + [S(noise(3, 200 + d), d, 256) for d in offs] + [end])
        out["per_sequence_periods_%d_to_%d_of_300" % (offs[0], offs[-1])] = lz4_case(
            [Fill(noise(80, 60 + g), 70)] + [S(noise(3, 300 + d), d, 300) for d in offs] + [end])
    out["matches_chained_through_one_step"] = lz4_case(
        [HEAD] + [S(b"", 4, 4)] * 40 + [S(b"", 3, 18), S(noise(1, 47), 5, 17), S(b"", 2, 9)] + [fill, end])
    # ends
    out["final_sequence_of_5_literals"] = lz4_case([HEAD, fill, S(noise(5, 48))])
    out["final_sequence_of_100_literals"] = lz4_case([HEAD, fill, S(noise(100, 49))])
    out["final_sequence_of_0_literals"] = lz4_case([HEAD, fill, S(b"")])
    out["final_sequence_of_1_literal"] = lz4_case([HEAD, fill, S(noise(1, 51))])
    for n in (A - 1, A + 1):
        out["content_of_%d_bytes" % n] = lz4_case([HEAD] + [S(noise(2, 52), 9, 5)] * 30 + [fill, end], n)
    return out


# liblz4's decoder applies the encoder-side end rules; the oracle (and the kernel) do not.
LZ4_ORACLE_ONLY = {
    "final_sequence_of_0_literals": "the last 5 bytes are not literals",
    "final_sequence_of_1_literal": "the last 5 bytes are not literals",
}

PREFIXES = range(84)


def _lz4_prefixes():
    """0..83 more literals in the first sequence before a fixed body of 4-byte sequences (16 to a
    round, 64 stream bytes): the loop top's reload then meets every ip - base from 941 to 1004."""
    out = {}
    for k in PREFIXES:
        out["top_reload_prefix_%02d" % k] = lz4_case(
            [S(noise(20 + k, 400), 20, 4)] + [S(noise(1, 401 + (j & 7)), 6, 4) for j in range(520)] +
            [Fill(noise(3, 3), 61), S(noise(TAIL, 4))])
    return out


def lz4_phase_name(off, path, phase):
    return "ring_%s_off_%d_phase_%02d" % (path, off, phase)


def lz4_phase_length(off):
    return B if off > A - 600 else A


def _lz4_phases(off, path):
    """The match starts at 224 + phase (mod 256), after `phase` literals of its own sequence:
    "batch": a match of 8 that is the first sequence of a batch (phase = its start in the batch's
    64-byte steps); "outring": a match of 300 through OutRing::match, whose steps start at op: its
    phase is op & 63 = (32 + phase) & 63."""
    out, n = {}, lz4_phase_length(off)
    ml, t0 = (8, 217) if path == "batch" else (300, 181)
    for p in range(64):
        c = lz4_case([Fill(noise(251, 500 + p), 251), S(noise(p, 600 + p), off, ml), S(noise(t0 + 63 - p, 700 + p))], n)
        assert "%s:off:%d:phase:%d" % (path, off, p if path == "batch" else (224 + p) & 63) in c.census
        assert "%s:off:%d:flushphase:%d" % (path, off, (224 + p) & 255) in c.census
        out[lz4_phase_name(off, path, p)] = c
    return out


_cache = {}


def _memo(key, fn, *args):
    if key not in _cache:
        _cache[key] = fn(*args)
    return _cache[key]


def lz4_cases():
    """name -> Case: the named cases and the prefix sweep (not the ring phases)."""
    return _memo("lz4", lambda: dict(_lz4_small(), **_lz4_prefixes()))


def lz4_small_names():
    return [n for n in lz4_cases() if not n.startswith("top_reload_prefix_")]


def lz4_phases(off, path):
    return _memo(("lz4p", off, path), _lz4_phases, off, path)


LZ4_PATHS = ("batch", "outring")

LZ4_CHECKLIST = (
    ["ll:%d/ext%d" % v for v in ((0, 0), (1, 0), (14, 0), (15, 1), (16, 1), (269, 1), (270, 2), (525, 3))] +
    ["join:ll:256", "perseq:only_because:ll:257", "reload:literals_mid_run"] +
    ["ml:%d/ext%d" % v for v in ((4, 0), (18, 0), (19, 1), (273, 1), (274, 2))] +
    ["join:ml:256", "perseq:only_because:ml:257", "outring:len>1024:near", "outring:len>1024:far",
     "outring:far:chunks>1"] +
    ["round:full:22", "round:full:4", "batch_full:fast", "walk_stop:cap_cuts_the_walk", "batch_full:join",
     "serial_at:first", "serial_at:middle", "serial_at:last", "walk_stop:long_successor"] +
    ["batch_exec:full:of:64", "reload:top", "reload:after_perseq"] +
    ["top_reload:%d:pending" % v for v in range(941, 1005)] +
    ["sbyte_reload:%s:pending" % f for f in ("llext", "off_lo", "off_hi", "mlext")] +
    ["perseq:only_because:window"] +
    ["batch:off:%d:len:256" % d for d in range(1, 65)] +
    ["batch:period:%d:rm:%d" % (d, r) for d in range(1, 64) for r in (0, 63, 64, 65, 127, 128, 255)] +
    ["outring:period:%d:len>64" % d for d in range(1, 64)] + ["outring:off:64:src:ring"] +
    ["batch:same_step:overlapping", "batch:jump_iterations:4"] +
    ["end:final_ll:0", "end:final_ll:1", "end:final_ll:>=5", "end:final_ll:>64"] +
    ["end:olen_mod_256:%d" % v for v in (255, 0, 1)] +
    ["hbm:min_vm_ops_since_source_flush:11"])

LZ4_PHASE_CHECKLIST = (
    ["%s:off:%d:phase:%d" % (path, off, p) for path in LZ4_PATHS for off in F.LZ4_RING_OFFS for p in range(64)] +
    ["batch:off:%d:src:%s" % (off, "hbm" if off > F.BATCH_SPLIT else "ring") for off in F.LZ4_RING_OFFS] +
    ["outring:off:%d:src:%s" % (off, "hbm" if off > F.MATCH_SPLIT else "ring") for off in F.LZ4_RING_OFFS] +
    ["batch:off:%d:flushphase:%d" % (off, f) for off in (4032, 4033) for f in (254, 255, 0, 1)] +
    ["outring:off:%d:flushphase:%d" % (off, f) for off in (4096, 4097) for f in (254, 255, 0, 1)])

# batch executions by cause (counts): every cause occurs
LZ4_CAUSES = ("full", "reload_top", "reload_sbyte", "before_copy")


# --------------------------------------------------------------------------------- BloscLZ
def lits(data):
    """Literal runs of at most 32 bytes."""
    return [L(data[k:k + 32]) for k in range(0, len(data), 32)]


def _blz_prefix(target, first=()):
    """Ops whose stream is exactly `target` bytes, all read through win.byte (no literal run after
    the first): 33 bytes (then `first`), then matches of 2 bytes and, for the parity, one of 3."""
    ops = [L(noise(32, 800))] + list(first)
    n = len(_bcat(ops))
    if (target - n) & 1:
        ops.append(M(9, 9))
        n += 3
    k = 0
    while n < target:
        ops.append(M(4, 9 + k % 20))
        n += 2
        k += 1
    assert n == target
    return ops


def _blz_small():
    out = {}
    head, fill, end = L(noise(32, 801)), BFill(29), L(noise(4, 802))
    out["literal_runs_of_1_31_32_and_33"] = blz_case(
        [head, M(5, 7), L(noise(1, 803)), M(5, 7), L(noise(31, 804)), M(5, 7), L(noise(32, 805)), L(noise(1, 806)),
         fill, end])
    for lv in range(8):
        out["first_control_byte_level_%d" % lv] = blz_case([L(noise(7 + lv, 810 + lv), level=lv), BFill(5), end])
    out["match_lengths_3_8_9_263_264"] = blz_case(
        [head] + [x for k, m in enumerate((3, 8, 9, 263, 264)) for x in (M(m, 5 + k), L(noise(2, 820 + k)))] +
        [fill, end])
    out["match_above_1024_near"] = blz_case([head, M(1500, 27), fill, end])
    out["match_above_1024_far"] = blz_case([head, BFill(29), M(1500, 4200), end])
    out["distances_1_2_63_64_65_256_and_the_ring_split"] = blz_case(
        [head, L(noise(32, 830)), L(noise(32, 831)), BFill(95)] +
        [x for k, d in enumerate((1, 2, 63, 64, 65, 256, 4095, 4096, 4097)) for x in (M(7, d), L(noise(2, 840 + k)))] +
        [end])
    out["distances_8191_8192_8193_and_73727"] = blz_case(
        [head, L(noise(32, 832)), L(noise(32, 833)), BFill(95)] +
        [x for k, d in enumerate((8191, 8192, 8193, 8192 + 65535)) for x in (M(70, d), L(noise(2, 850 + k)))] +
        [end], B)
    out["periods_1_to_64_of_70"] = blz_case(
        [head, L(noise(32, 834)), L(noise(32, 835)), BFill(95)] +
        [x for d in range(1, 65) for x in (L(noise(3, 860 + d)), M(70, d))] + [end])
    # the window's first reload, at stream byte 1024 (or at a literal run that starts past 960), in every field
    out["window_reload_at_a_control_byte"] = blz_case(_blz_prefix(1024) + [M(4, 9), fill, end])
    out["window_reload_at_a_length_extension_byte"] = blz_case(_blz_prefix(1023) + [M(9, 9), fill, end])
    out["window_reload_at_a_distance_byte"] = blz_case(_blz_prefix(1023) + [M(4, 9), fill, end])
    out["window_reload_at_a_literal_run"] = blz_case(_blz_prefix(961) + [L(noise(32, 870)), fill, end])
    far = [M(9000, 29)]  # the history of a far match, from 38 stream bytes
    out["window_reload_at_the_far_field_high_byte"] = blz_case(_blz_prefix(1022, far) + [M(4, 9000), fill, end], B)
    out["window_reload_at_the_far_field_low_byte"] = blz_case(_blz_prefix(1021, far) + [M(4, 9000), fill, end], B)
    return out


def blz_phase_name(dist, phase):
    return "ring_dist_%d_phase_%02d" % (dist, phase)


def _blz_phases(dist):
    out = {}
    for p in range(64):
        c = blz_case([L(noise(32, 900 + p)), BFill(29)] + lits(noise(p, 1000 + p)) + [M(70, dist)] +
                     lits(noise(155 + 63 - p, 1100 + p)))
        assert "match:off:%d:phase:%d" % (dist, (224 + p) & 63) in c.census
        out[blz_phase_name(dist, p)] = c
    return out


def blz_cases():
    return _memo("blz", _blz_small)


def blz_phases(dist):
    return _memo(("blzp", dist), _blz_phases, dist)


BLZ_CHECKLIST = (
    ["lit:1", "lit:31", "lit:32", "lit:32>lit:1"] + ["level:%d" % v for v in range(8)] +
    ["match:len:%d/ext%d" % v for v in ((3, 0), (8, 0), (9, 1), (263, 1), (264, 2))] +
    ["match:len>1024:near", "match:len>1024:far", "match:far:chunks>1"] +
    ["dist:%d:form:13" % d for d in (1, 2, 63, 64, 65, 256, 4095, 4096, 4097, 8191)] +
    ["dist:%d:form:16" % d for d in (8192, 8193, 8192 + 65535)] +
    ["match:off:4096:src:ring", "match:off:4097:src:hbm"] +
    ["match:period:%d:len>64" % d for d in range(1, 64)] + ["match:off:64:src:ring"] +
    ["reload:%s" % f for f in ("ctrl", "lenext", "dist", "far_hi", "far_lo", "literals")] +
    ["end:literals"])

BLZ_PHASE_CHECKLIST = ["match:off:%d:phase:%d" % (d, p) for d in F.BLZ_RING_DISTS for p in range(64)]


# ------------------------------------------------------------------------------- malformed
def _cat(seqs):
    return b"".join(F.lz4_seq_bytes(s) for s in seqs)


def lz4_malformed():
    """name -> (stream, block length, decoder code, guard, path).  Every read of these streams is
    bounded by ilen (the serial parse) or lies in the window (the candidates, whose `ok` test keeps
    what lies past ilen out of the batch): no code depends on the bytes after the stream."""
    out = {}
    good = [HEAD, S(noise(3, 3), 61, A - 64 - 8 - 3 - TAIL)]  # A - TAIL bytes; then TAIL final literals
    pre = [HEAD, S(noise(2, 5), 9, 300)]  # a per-sequence match: the batch is empty after it
    short = [S(noise(2, 6), 9, 5)] * 3    # three fast-path sequences: a pending batch
    end = S(noise(TAIL, 4))
    out["input_ends_after_a_match"] = (
        _cat([HEAD, S(noise(3, 3), 61, A - 64 - 8 - 3)]), A, 1, "loop top: ip >= ilen",
        "the match is pending in the batch")
    out["literal_extension_cut"] = (
        _cat(good) + b"\xf0\xff", A, 2, "serial: ip + k >= ilen in the literal extension", "serial")
    out["literals_past_the_input"] = (
        _cat(good) + b"\xa0" + noise(5, 7), A, 3, "serial: lln > ilen - ls",
        "serial (no candidate passes q + 3 + ll <= ilen)")
    out["literals_past_the_output"] = (
        _cat(good + [S(noise(TAIL + 1, 8))]), A, 3, "serial: lln > olen - op", "serial, empty batch")
    # the batch holds 3 x 7 bytes that op does not count yet: 300 literals fit olen - op, not what is left after it
    out["literals_past_the_output_behind_a_pending_batch"] = (
        _cat([HEAD, S(noise(3, 3), 61, A - 64 - 8 - 3 - 310)] + short + [S(noise(300, 9))]), A, 3,
        "per-sequence: lln > olen - op once the batch is out", "per-sequence, after a batch of 3")
    out["literals_past_the_output_behind_a_pending_batch_then_a_match"] = (
        _cat([HEAD, S(noise(3, 3), 61, A - 64 - 8 - 3 - 310)] + short + [S(noise(300, 9), 9, 2000), end]), A, 3,
        "per-sequence: lln > olen - op once the batch is out", "per-sequence, after a batch of 3")
    out["offset_cut"] = (
        _cat(good) + b"\x20" + noise(2, 10) + b"\x09", A, 4, "serial: fewer than 2 bytes after the literals", "serial")
    out["match_extension_cut"] = (_cat(good) + b"\x1f" + noise(1, 11) + b"\x09\x00\xff", A, 5,
                                  "serial: ip + k >= ilen in the match extension", "serial")
    out["offset_0_in_the_batch"] = (_cat(pre + [S(noise(2, 12), 0, 6), end]), A, 6, "seq_batch: boff == 0", "fast path")
    out["offset_0_per_sequence"] = (
        _cat(pre + [S(noise(2, 12), 0, 300), end]), A, 6, "OutRing::match: off == 0", "per-sequence")
    # 64 + 8 + 2 + 300 + 3 * 7 + 2 = 397 bytes before the bad match
    out["offset_one_beyond_the_start_mid_batch"] = (
        _cat(pre + short + [S(noise(2, 13), 398, 6)] + short + [end]), A, 6,
        "seq_batch: boff > op0 + st0 + bll", "fast path, the 4th of 7 sequences")
    out["offset_one_beyond_the_start_per_sequence"] = (
        _cat(pre + [S(noise(2, 13), 377, 300), end]), A, 6, "OutRing::match: off > op", "per-sequence")
    out["match_past_the_output_in_the_batch"] = (
        _cat(good[:1] + [S(noise(3, 3), 61, A - 64 - 8 - 3 - 10), S(noise(2, 14), 9, 9), S(noise(5, 15))]), A, 6,
        "seq_batch: T > olen - op0", "fast path (the final literals fit what op counts)")
    out["match_past_the_output_per_sequence"] = (
        _cat(good[:1] + [S(noise(3, 3), 61, A - 64 - 8 - 3 - 302), S(noise(2, 14), 9, 301), end]), A, 6,
        "OutRing::match: len > olen - op", "per-sequence")
    out["output_short"] = (
        _cat([HEAD, S(noise(3, 3), 61, A - 64 - 8 - 3 - TAIL - 1), end]), A, 7, "end: op != olen", "any")
    return out


# what the model must report beside the code: the path the case file claims
LZ4_MALFORMED_PATHS = {
    "offset_0_in_the_batch": ("fast", 1), "offset_one_beyond_the_start_mid_batch": ("fast", 7),
    "match_past_the_output_in_the_batch": ("fast", 1),
    "offset_0_per_sequence": ("perseq", 2), "offset_one_beyond_the_start_per_sequence": ("perseq", 2),
    "match_past_the_output_per_sequence": ("perseq", 2),
    "literals_past_the_output_behind_a_pending_batch": ("fast", 3),
    "literals_past_the_output_behind_a_pending_batch_then_a_match": ("fast", 3),
}


def _bcat(ops):
    return b"".join(F.blz_op_bytes(o, k == 0) for k, o in enumerate(ops))


def blz_malformed():
    """name -> (stream, block length, decoder code, guard)."""
    out = {}
    head = [L(noise(32, 801)), M(A - 32 - 40, 29)]  # A - 40 bytes
    out["length_extension_cut"] = (_bcat(head) + b"\xe0\xff\x05", A, 2, "ip + 1 >= ilen in the length extension")
    out["distance_byte_is_the_last_byte"] = (
        _bcat(head) + b"\x40\x05", A, 3, "ip + 1 >= ilen before the distance byte")
    out["far_distance_cut"] = (_bcat(head) + b"\x5f\xff\x00", A, 4, "ip + 1 >= ilen before the far field")
    out["match_past_the_output"] = (_bcat(head + [M(41, 5)] + lits(noise(4, 1))), A, 5, "len > olen - op")
    out["distance_one_beyond_the_start"] = (
        _bcat([L(noise(32, 801)), M(5, 33)] + lits(noise(4, 1))), A, 5, "dist > op")
    out["far_distance_beyond_the_start"] = (
        _bcat(head + [M(5, 8192)] + lits(noise(4, 1))), A, 5, "dist > op (far form)")
    out["literal_run_past_the_output"] = (_bcat(head + lits(noise(41, 2))), A, 7, "nl > olen - op")
    out["literal_run_past_the_input"] = (_bcat(head) + b"\x09" + noise(5, 3), A, 7, "ip + nl > ilen")
    out["output_short"] = (_bcat(head + lits(noise(39, 4))), A, 8, "end: op != olen")
    out["ends_on_a_match_with_extension_bytes"] = (
        _bcat(head[:1] + [M(A - 32 - 40, 29), L(noise(1, 5)), M(39, 7)]), A, 8,
        "the match is parsed, not copied: op != olen")
    out["ends_on_a_far_match"] = (
        _bcat([L(noise(32, 801)), M(B - 32 - 40, 29), L(noise(1, 5)), M(39, 9000, ext=[30])]), B, 8,
        "the match is parsed, not copied: op != olen")
    return out
