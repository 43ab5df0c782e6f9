"""The hand-built JPEG scans (tests/_tiff_jpeg_frames.py's writer) the JPEG kernels are tested on,
and the checklists their censuses must cover.  Every case is (name, w, h, stream, kind), kind one
of _tiff_jpeg.KINDS; cases() groups them as the GPU test registers them.  All streams are built at
first use, seeded.  test_tiff_jpeg_frames_host.py holds every one equal to PIL and the censuses to
the checklists; test_gpu_tiff_jpeg_frames.py gives the same streams to the device."""
import functools

import numpy as np

import _tiff_jpeg as J
import _tiff_jpeg_frames as F
from _tiff_jpeg_frames import EOB, ZRL

ONES = {i: np.ones(64, np.int64) for i in range(4)}
FLAT = {(0, 0): F.FLAT_DC, (1, 0): F.FLAT_AC}
EMPTY = [(0, 0), EOB]  # under the flat 4-bit codes exactly one byte, 00
LANES = range(64)
FILLS = (0, 1, 65)

# cases whose padding blocks are exempt from the model's [-512, 511] assertion (the blocks are
# F.padding_blocks(stream), nothing else: the host test asserts it)
EXEMPT = frozenset(["fat_1665_in_padding_12_mcus", "fat_1665_in_padding_interval_1_fill_70",
                    "fat_1665_in_padding_interval_5", "fat_1665_in_padding_behind_longer_visible_blocks"])


# ------------------------------------------------------------------------------ lane sweeps
def _gray(w, h, mcus, restart=0, **kw):
    return F.write_stream(w, h, mcus, q=ONES, huff=FLAT, tq=(0,), td=(0,), ta=(0,), restart=restart, **kw)


def marker_sweep(p, fill):
    """Two restart intervals of p one-byte empty blocks and two content blocks (6 bytes): the RSTn
    code, and then the EOI's, stands p + 7 + fill bytes after its round began."""
    content = [[[F.value_bits(37), (0,) + F.value_bits(-9), (0,) + F.value_bits(2), EOB]],
               [[F.value_bits(-60), (1,) + F.value_bits(1), EOB]]]
    s = _gray(8 * (p + 2), 16, ([[EMPTY]] * p + content) * 2, restart=p + 2)
    assert len(F.entropy(s)) == 2 * (p + 6 + 2) and b"\xff\x00" not in F.entropy(s)
    return ("marker_lane_p%02d_fill%d" % (p, fill), 8 * (p + 2), 16, F.fill_before_markers(s, fill), "gray")


def stuff_sweep(p, dc):
    """p one-byte empty blocks, then a data FF made of the 8 value bits of a size-8 coefficient
    (255 at k = 1) or of a size-8 DC difference (+255 after -15), at raw byte p + 1 or p + 2."""
    if dc:
        content = [[[(4, 0), EOB]], [[(8, 255), EOB]]]
    else:
        content = [[[(0, 0), (0, 8, 255), EOB]]]
    content.append([[F.value_bits(9), EOB]])  # a block behind the pair: a zero kept by mistake moves its bits
    n = p + len(content)
    s = _gray(8 * n, 8, [[EMPTY]] * p + content)
    assert F.entropy(s)[p + 1 + dc:p + 3 + dc] == b"\xff\x00"
    return ("stuff_lane_%s_p%02d" % ("dc" if dc else "ac", p), 8 * n, 8, s, "gray")


def fill_before_stuffed(stream):
    """A fill byte in front of the first stuffed pair: FF FF 00."""
    d = J.header(stream)["data"]
    at = stream.index(b"\xff\x00", d)
    return stream[:at] + b"\xff" + stream[at:]


# ------------------------------------------------------------------------------ content streams
def _planes(kind, w, h, seed, amp=4):
    """Low-amplitude noise on a ramp (in range under every quantiser used here), per component at
    its own MCU-padded resolution."""
    hs, vs = {"gray": (1, 1), "444": (1, 1), "rgb": (1, 1), "422": (2, 1), "420": (2, 2)}[kind]
    nc = 1 if kind == "gray" else 3
    pw, ph = -(-w // (8 * hs)) * 8 * hs, -(-h // (8 * vs)) * 8 * vs
    rng = np.random.default_rng(seed)
    out = []
    for c in range(nc):
        cw, ch = (pw, ph) if c == 0 else (pw // hs, ph // vs)
        a = rng.integers(0, 256, (ch, cw)) // amp + 96 + (np.arange(cw) * 40 // cw)[None, :] * (c + 1) // 2
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out, (hs, vs)


def content_stream(kind, w, h, seed, restart=0, q=None, huff=None, ids=((0, 1, 1),) * 3, amp=4, **kw):
    T = J.std_tables()
    q = q if q is not None else T["q"]
    planes, samp = _planes(kind, w, h, seed, amp)
    tq, td, ta = ids
    blocks = [J.quantised_blocks(p, q[tq[c]]) for c, p in enumerate(planes)]
    return F.write_stream(w, h, F.mcus_of(blocks, samp, restart), nc=len(planes), sampling=samp, q=q, huff=huff, tq=tq,
                          td=td, ta=ta, restart=restart, **kw)


BPM = {"gray": 1, "444": 3, "422": 4, "420": 6}
# kind -> (w, h) of nmcu == per + 1, == per, < per
BATCH_SHAPES = {"gray": ((101, 40), (64, 61), (16, 8)), "444": ((85, 16), (56, 21), (24, 8)),
                "422": ((270, 8), (64, 30), (32, 8)), "420": ((170, 16), (77, 32), (32, 16))}


def batch_cases():
    out = []
    for k, kind in enumerate(BATCH_SHAPES):
        (w1, h1), (w2, h2), (w3, h3) = BATCH_SHAPES[kind]
        out.append(("batch_%s_per_plus_1_interval_1" % kind, w1, h1, content_stream(kind, w1, h1, 10 + k, restart=1), kind))
        out.append(("batch_%s_per_interval_3" % kind, w2, h2, content_stream(kind, w2, h2, 20 + k, restart=3), kind))
        out.append(("batch_%s_per_interval_longer_than_the_stream" % kind, w2, h2,
                    content_stream(kind, w2, h2, 30 + k, restart=64 // BPM[kind] + 5), kind))
        out.append(("batch_%s_fewer_than_per" % kind, w3, h3, content_stream(kind, w3, h3, 40 + k), kind))
    return out


# ------------------------------------------------------------------------------ tables
def _variant(code):
    """The same code lengths with the symbols in reverse order: another code over the same set."""
    bits, vals = code
    return list(bits), list(vals)[::-1]


def three_table_sets():
    """Three quantisers far apart and six different Huffman codes, under ids in no default order:
    component c uses quantiser TQ[c], DC table TD[c] and AC table TA[c]."""
    T = J.std_tables()
    q = {3: np.full(64, 2, np.int64), 0: np.full(64, 9, np.int64), 2: np.full(64, 23, np.int64)}
    huff = {(0, 2): T["h"][(0, 0)], (1, 3): T["h"][(1, 0)], (0, 1): T["h"][(0, 1)], (1, 0): T["h"][(1, 1)],
            (0, 3): _variant(T["h"][(0, 0)]), (1, 2): _variant(T["h"][(1, 0)])}
    return q, huff


TABLE_IDS = ((3, 0, 2), (2, 1, 3), (3, 0, 2))  # tq, td, ta
TABLE_KINDS = (("444", 24, 16), ("rgb", 24, 16), ("420", 40, 24))


def table_stream(kind, w, h, tq=TABLE_IDS[0]):
    """The three-table stream of `kind`; with another tq the same entropy bytes and DQT segments
    under exchanged quantiser ids (the host test: every exchange changes visible pixels)."""
    q, huff = three_table_sets()
    planes, samp = _planes(kind, w, h, 77, amp=2)
    blocks = [J.quantised_blocks(p, q[TABLE_IDS[0][c]]) for c, p in enumerate(planes)]
    # (component ids R, G, B: how libjpeg, the judge, knows that a stream without markers holds RGB)
    return F.write_stream(w, h, F.mcus_of(blocks, samp), nc=3, sampling=samp, q=q, huff=huff, tq=tq, td=TABLE_IDS[1],
                          ta=TABLE_IDS[2], comp_ids=(82, 71, 66) if kind == "rgb" else (1, 2, 3))


def table_cases():
    return [("tables_%s_tq302_td213_ta302" % kind, w, h, table_stream(kind, w, h), kind) for kind, w, h in TABLE_KINDS]


# ------------------------------------------------------------------------------ symbols
AC16 = [0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0xF0, 0x11, 0x21, 0xE1, 0x12]
PATTERNS = ("zeros", "ones", "0111", "1000")


def _pattern_bits(size, name):
    return {"zeros": 0, "ones": (1 << size) - 1, "0111": (1 << (size - 1)) - 1, "1000": 1 << (size - 1)}[name]


def symbol_stream():
    """4:4:4, quantisers of ones.  Component 0: a DC code with one symbol at each length 1 .. 12 and
    an AC code with one at each length 1 .. 16; component 1: DC lengths 5 .. 16.  Components 0 and 1
    take every DC size with its four extreme patterns (zeros, ones: net 0; 0111, 1000: net 0, so
    the predictor stays in [-2047, 0] and every sample in range); component 0 then every AC size
    1 .. 10 with the four patterns at k = 1 (at most 1023 x 0.174 = 178 in a sample), three ZRL
    and a coefficient at 63, a ZRL that lands on 63, and every other symbol of the code."""
    huff = {(0, 0): F.ladder_code(range(12), range(1, 13)), (1, 0): F.ladder_code(AC16, range(1, 17)),
            (0, 1): F.ladder_code(range(12), range(5, 17)), (1, 1): F.flat_code([0x00, 0x01]),
            (0, 2): F.FLAT_DC, (1, 2): F.FLAT_AC}
    dcs = [[(0, 0), EOB]] + [[(s, _pattern_bits(s, p)), EOB] for s in range(1, 12) for p in PATTERNS]
    c0 = list(dcs)
    c0 += [[(0, 0), (0, s, _pattern_bits(s, p)), EOB] for s in range(1, 11) for p in PATTERNS]
    c0 += [[(0, 0), ZRL, ZRL, ZRL, (14, 1, 1)],            # k = 49, then run 14: coefficient 63, no EOB
           [(0, 0), (14, 1, 0), ZRL, ZRL, ZRL],            # k = 15, 16 .. 48, ZRL from 48 lands on 63
           [(0, 0), (1, 1, 1), (2, 1, 0), (1, 2, 2), EOB]]
    n = len(c0)
    c1 = dcs + [[(0, 0), EOB]] * (n - len(dcs))
    c2 = [[F.value_bits(3 if i % 2 == 0 else -3), EOB] for i in range(n)]
    assert n == 88
    return ("symbols_every_length_size_and_pattern", 88, 64,
            F.write_stream(88, 64, [[a, b, c] for a, b, c in zip(c0, c1, c2)], nc=3, q=ONES, huff=huff, tq=(0, 0, 0),
                           td=(0, 1, 2), ta=(0, 1, 2)), "444")


# ------------------------------------------------------------------------------ fat blocks
FAT_DC = F.ladder_code([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16])
FAT_AC = F.ladder_code([0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A], list(range(1, 11)) + [16])
FAT_HUFF = {(0, 0): FAT_DC, (1, 0): FAT_AC, (0, 1): F.FLAT_DC, (1, 1): F.FLAT_AC}


def fat_mcus(nmcu, restart, seed=3, big=False):
    """4:2:0 MCUs for an image 8 pixels wide: luma blocks 1 and 3 lie wholly outside it and are the
    1,665-bit block (DC +-1200 so every luma DC difference is size 11, behind its 16-bit code, and
    63 coefficients of size 10 behind theirs); blocks 0 and 2 and the chroma blocks are small."""
    rng = np.random.default_rng(seed)
    blocks = [np.zeros((2 * nmcu, 2, 64), np.int64), np.zeros((nmcu, 1, 64), np.int64), np.zeros((nmcu, 1, 64), np.int64)]
    blocks[0][:, 0, 0] = rng.integers(-40, 40, 2 * nmcu)
    blocks[0][:, 0, 1:4] = rng.integers(1, 4, (2 * nmcu, 3)) * rng.choice([-1, 1], (2 * nmcu, 3))  # (no runs in FAT_AC)
    if big:  # visible blocks of some 90 bytes: a refill falls due inside one, in front of a fat block
        blocks[0][:, 0, 1:] = rng.integers(16, 32, (2 * nmcu, 63)) * rng.choice([-1, 1], (2 * nmcu, 63))
        for r, n in enumerate(rng.integers(8, 64, 2 * nmcu)):  # of different lengths, so the phase moves
            blocks[0][r, 0, n:] = 0
    blocks[0][:, 1, 0] = np.where(np.arange(2 * nmcu) % 2 == 0, 1200, -1200)
    blocks[0][:, 1, 1:] = rng.integers(512, 1024, (2 * nmcu, 63)) * rng.choice([-1, 1], (2 * nmcu, 63))
    for c in (1, 2):
        blocks[c][:, 0, 0] = rng.integers(-30, 30, nmcu)
        blocks[c][:, 0, 1] = rng.integers(-2, 3, nmcu)
    return F.mcus_of(blocks, (2, 2), restart)


def fat_stream(nmcu=12, restart=0, fill=0, big=False, seed=3):
    s = F.write_stream(8, 16 * nmcu, fat_mcus(nmcu, restart, seed, big), nc=3, sampling=(2, 2), q=ONES, huff=FAT_HUFF,
                       tq=(0, 0, 0), td=(0, 1, 1), ta=(0, 1, 1), restart=restart)
    return F.fill_before_markers(s, fill) if fill else s


def fat_cases():
    out = [("fat_1665_in_padding_12_mcus", 8, 192, fat_stream(), "420"),
           ("fat_1665_in_padding_interval_1_fill_70", 8, 192, fat_stream(restart=1, fill=70), "420"),
           ("fat_1665_in_padding_interval_5", 8, 192, fat_stream(restart=5), "420"),
           # (seed 18 of 3 .. 19: its refills fall due in front of blocks 1 and 3, the fat ones, by the census)
           ("fat_1665_in_padding_behind_longer_visible_blocks", 8, 192, fat_stream(big=True, seed=18), "420")]
    assert {c[0] for c in out} == EXEMPT
    return out


FLAT16 = {(0, 0): F.flat_code(range(12), 16), (1, 0): F.flat_code(list(range(0x0B)) + [0xF0], 16)}


@functools.lru_cache(None)
def fattest_visible():
    """The fattest block the model's range assertion admits, by a seeded search.  Every code is 16
    bits long (FLAT16), so a block of 64 non-zero coefficients takes 64 x 16 bits and its sizes on
    top; all of them at size 10 cannot stay in range (Parseval: the samples' energy is the
    coefficients').  Each coefficient takes the least magnitude of its size, 2^(size - 1), under a
    quantiser of ones; one size is raised or one sign turned at a time, and the move is kept when
    the block stays in [-512, 511] and either gains bits or lowers its peak.
    -> (bits, 64 zigzag coefficients)."""
    rng = np.random.default_rng(2024)

    def excess(sizes, signs):
        nat = np.zeros((1, 64), np.int64)
        nat[0, J.NAT] = [sg << (s - 1) for s, sg in zip(sizes, signs)]
        b = nat.reshape(1, 8, 8)
        cols = J._idct1([b[..., r, :] for r in range(8)])
        ws = np.stack([(x + (1 << 10)) >> 11 for x in cols], axis=-2)
        rows = J._idct1([ws[..., :, c] for c in range(8)])
        out = np.stack([(x + (1 << 17)) >> 18 for x in rows], axis=-1)
        return max(int(out.max()) - 511, -512 - int(out.min()))  # <= 0: in range

    sizes = [1] + [7] * 63
    signs = [int(x) for x in rng.choice([-1, 1], 64)]
    cur = excess(sizes, signs)
    assert cur <= 0
    for _ in range(3000):
        k = int(rng.integers(64))
        s2, g2 = list(sizes), list(signs)
        if rng.integers(3) == 0:
            g2[k] = -g2[k]
        elif s2[k] < (11 if k == 0 else 10):
            s2[k] += 1
        else:
            continue
        e = excess(s2, g2)
        if e <= 0 and (s2 != sizes or e < cur):
            sizes, signs, cur = s2, g2, e
    return 64 * 16 + sum(sizes), np.array([sg << (s - 1) for s, sg in zip(sizes, signs)], np.int64)


def fat_visible_case():
    bits, z = fattest_visible()
    blocks = [np.zeros((2, 3, 64), np.int64)]
    blocks[0][:, :, 0] = [[5, 0, 14], [0, 7, 0]]
    blocks[0][0, 1] = z
    blocks[0][1, 2] = -z
    mcus = F.mcus_of(blocks)
    # the DC differences of the fat blocks are the searched ones: the predictor in front of them is 0
    s = F.write_stream(24, 16, mcus, q=ONES, huff=FLAT16, tq=(0,), td=(0,), ta=(0,), restart=1)
    return ("fat_visible_%d_bits" % bits, 24, 16, s, "gray")


# ------------------------------------------------------------------------------ ends, refills
def end_cases():
    body = [[EMPTY]] * 122 + [[[F.value_bits(13), EOB]], [[F.value_bits(-13), EOB]]] * 2  # 122 + 6 bytes, 126 blocks
    s = _gray(112, 72, body)
    assert len(F.entropy(s)) == 130
    ac = stuff_sweep(5, 0)[3]
    out = [("end_exactly_on_a_round_no_eoi", 112, 72, F.drop_eoi(s), "gray"),
           ("end_last_byte_ff_no_eoi", 112, 72, F.append_bytes(F.drop_eoi(s), b"\xff"), "gray"),
           ("end_no_eoi", 56, 8, F.drop_eoi(stuff_sweep(5, 0)[3]), "gray"),
           ("end_junk_after_eoi", 56, 8, F.append_bytes(ac, b"\x12\xff\xd0\x00\xff\xff\x34" * 20), "gray"),
           ("fill_byte_before_a_stuffed_pair", 56, 8, fill_before_stuffed(ac), "gray"),
           ("all_eob", 24, 16, _gray(24, 16, [[EMPTY]] * 6), "gray")]
    return out


def refill_cases():
    """Streams of several KB of clean bytes: refills ended by the cap, moved remainders with every
    skip, a refill in front of every block index of the MCU, chains of moved refills."""
    out = []
    for kind, w, h in (("gray", 96, 80), ("444", 64, 48), ("422", 96, 48), ("420", 96, 64)):
        for seed in (1, 2):
            out.append(("refill_%s_seed%d" % (kind, seed), w, h, content_stream(kind, w, h, 50 + seed, amp=1,
                                                                               q=ONES_STD), kind))
    return out


ONES_STD = {0: np.full(64, 6, np.int64), 1: np.full(64, 6, np.int64)}


# ------------------------------------------------------------------------------ wide rows
WIDE = 1045  # k_tiff_jpeg_place's step of 1024 pixels, one whole group of 16 and a partial group of 5


@functools.lru_cache(None)
def wide_pages():
    """[(name, page)] for the placement kernel's step loop: strips 1045 and 2080 pixels wide and 1,
    2 and 3 rows high in every kind (cw = 523, ch = 1 and 2, the far chroma row clamped at both
    ends), and a layer of 1040 x 16 tiles in a 1045 x 20 image whose second tile is clipped to 5
    columns.  PIL's encoder at quality 85 on noise over a ramp: chroma changes across column 1024."""
    out = []
    for w in (WIDE, 2080):
        for h in (1, 2, 3):
            a = J.noise(w, h, 7 * w + h) // 2 + J.ramp(w, h) // 2
            out += [("wide_%s_%dx%d" % (kind, w, h), J.kind_page(kind, a, quality=85)) for kind in J.KINDS]
    a = J.noise(WIDE, 20, 99) // 2 + J.ramp(WIDE, 20) // 2
    out += [("wide_tiles_%s" % kind, J.kind_page(kind, a, tile=(1040, 16), quality=85)) for kind in J.KINDS]
    return out


# ------------------------------------------------------------------------------ all of them
@functools.lru_cache(None)
def cases():
    """group -> [(name, w, h, stream, kind)]: one registration a group on the device."""
    g = {}
    g["markers"] = [marker_sweep(p, f) for f in FILLS for p in LANES]
    g["stuffing"] = [stuff_sweep(p, dc) for dc in (0, 1) for p in LANES] + end_cases()
    g["refills"] = refill_cases()
    g["fat"] = fat_cases() + [fat_visible_case()]
    g["tables"] = table_cases()
    g["symbols"] = [symbol_stream()]
    g["batches"] = batch_cases()
    names = [c[0] for v in g.values() for c in v]
    assert len(set(names)) == len(names)
    return g


def all_cases():
    return [c for v in cases().values() for c in v]


# ------------------------------------------------------------------------------ checklists
def _bpm_keys(fmt, bpms=(1, 3, 4, 6)):
    return [fmt % b for b in bpms]


CHECKLIST = (
    ["marker:lane:%d" % l for l in LANES] + ["stuff:lane:%d" % l for l in LANES]
    + ["prefix-split", "fill-round", "fill-run-crosses-round", "stuff-split", "FF FF 00"]
    + ["eos:exact-round", "eos:last-byte-FF", "eos:no-EOI", "eos:junk-after-EOI"]
    + ["refill-end:cap", "refill-end:marker", "refill-end:eos", "refill:first", "refill:block", "refill:restart"]
    + ["skip:%d" % k for k in range(8)] + ["move:iterations:1", "refill:moved-chain-of-3"]
    + ["refill-at-block:bpm6:%d" % b for b in range(6)] + ["refill-at-block:bpm4:%d" % b for b in range(4)]
    + ["refill-at-block:bpm3:%d" % b for b in range(3)] + ["refill-at-block:bpm1:0"]
    + ["fat:%d" % F.FAT, "refill:in-front-of-a-fat-block", "refill:just-after-a-fat-block"]
    + ["tables:tq:3,0,2", "tables:td/ta:2/3,1/0,3/2"]
    + ["code:%s:len:%d:%s" % (c, l, "lut" if l < 10 else "walk") for c in ("dc", "ac") for l in range(1, 17)]
    + ["receive:dc:size:0"] + ["receive:dc:size:%d:%s" % (s, p) for s in range(1, 12) for p in PATTERNS]
    + ["receive:ac:size:%d:%s" % (s, p) for s in range(1, 11) for p in PATTERNS]
    + ["zrl:x3-then-63", "zrl:lands-on-63", "coef63:no-eob", "stream:all-eob"]
    + _bpm_keys("batch:bpm%d:nmcu<per") + _bpm_keys("batch:bpm%d:nmcu==per") + _bpm_keys("batch:bpm%d:nmcu==1+per")
    + _bpm_keys("batch:bpm%d:last-of-one-mcu") + _bpm_keys("restart:bpm%d:inside-batch")
    + _bpm_keys("restart:bpm%d:on-batch-boundary") + _bpm_keys("restart:bpm%d:interval-1")
    + _bpm_keys("rstn-wrap:bpm%d") + _bpm_keys("restart:bpm%d:interval-longer-than-the-stream"))

# What no well-formed stream reaches, and why (kernels_tiff_jpeg.hip):
UNREACHABLE = {
    "move:iterations:2": "jrefill's move loop steps k by 256 and runs while k < rem.  A block-start refill happens only "
                         "when cend * 8 < posb + J_LOW * 8, i.e. with rem <= 256 bytes unread, so k = 256 is never "
                         "entered there; the first refill and the one after a restart have byte0 == 0 and move nothing.  "
                         "Only the !pend refill at a restart can have more unread, and that one is unreachable too.",
    "refill:restart:no-marker-seen": "At a block's start either pend is set or at least J_LOW = 256 clean bytes of the "
                                     "interval lie ahead, none of them behind a marker (a refill never passes one); a block "
                                     "takes at most 1,665 bits = 209 bytes, so with pend clear at least 47 bytes of the "
                                     "same interval follow the block and the interval is not over.  Where an interval ends "
                                     "within 7 bits of its last block, pend is set.  (Junk of J_CAP bytes in front of a "
                                     "marker does reach it: malformed(), code 5.)",
}


# ------------------------------------------------------------------------------ malformed
def _cut_in_fat(n):
    """fat_stream() cut n bytes into its first 1,665-bit block (block 1 of MCU 0)."""
    s = fat_stream()
    mcu = fat_mcus(12, 0)[0]
    head = F.write_stream(8, 192, [[mcu[0]] + [[("raw", 0, 0)]] * 5], nc=3, sampling=(2, 2), q=ONES, huff=FAT_HUFF,
                          tq=(0, 0, 0), td=(0, 1, 1), ta=(0, 1, 1))
    at = len(F.entropy(head)) - 2 - 1  # whole bytes of block 0 (its last, partial byte is the fat block's first)
    assert F.entropy(s)[:at] == F.entropy(head)[:at]
    return s[:J.header(s)["data"] + at + n]


@functools.lru_cache(None)
def malformed():
    """name -> (w, h, stream, kind, code, why).  Where two defects could apply the one the decoder
    meets first in the stream decides; inside a block the order is the kernel's: a code in no
    table (2), a run past 63 (3), a size out of range (4), and only at the block's end bits taken
    from past the data (1); a restart marker is judged (5) only when an interval's MCUs are done."""
    out = {}
    # gray, flat codes, 6 MCUs in intervals of 2; blocks of 12 bits, so an interval is 3 bytes
    blk = [F.value_bits(9), EOB]
    six = [[blk]] * 6
    out["junk_after_an_interval_marker_already_seen"] = (
        48, 8, _gray(48, 8, six, restart=2, junk=lambda n: b"\x00" * 5 if n == 0 else b""), "gray", 5,
        "5 clean bytes between interval 0's end and RST0: the first refill has recorded RST0 (pend), but the "
        "decoder does not stand at cend")
    out["junk_of_j_cap_bytes_after_an_interval"] = (
        48, 8, _gray(48, 8, six, restart=2, junk=lambda n: b"\x00" * (F.J_CAP + 40) if n == 0 else b""), "gray", 5,
        "the first refill ends at the cap with no marker seen: the restart takes the !pend refill, which moves more "
        "than 256 unread bytes and again ends at the cap; pend is still clear, so the marker is missing")
    two = [(0, 0), (0,) + F.value_bits(9), EOB]  # 16 bits: no padding bits
    out["marker_one_mcu_early_after_a_whole_byte"] = (
        48, 8, _gray(48, 8, [[two]] * 6, restart=1, dri=2), "gray", 1,
        "RST0 after MCU 0 of an interval of 2: MCU 1 takes its bits from the zeros behind the marker (an empty block "
        "under the flat codes), and that is judged at the block's end (1), before any marker is (5)")
    out["marker_one_mcu_early_after_padding_bits"] = (
        48, 8, _gray(48, 8, six, restart=1, dri=2), "gray", 2,
        "the same with MCUs of 12 bits: MCU 1 begins with interval 0's four padding bits, 1111, which the flat DC code "
        "of twelve symbols does not assign (2), met before the block's end (1)")
    out["ninth_marker_rst1_instead_of_rst0"] = (
        80, 8, _gray(80, 8, [[blk]] * 10, restart=1, marker=lambda n: 0xD1 if n == 8 else 0xD0 + (n & 7)), "gray", 5,
        "RSTn wraps after RST7: the ninth is RST0")
    out["rstn_without_dri"] = (
        48, 8, _gray(48, 8, six, restart=2, dri=0), "gray", 1,
        "no restart interval declared: the refill stops at the marker for good and MCU 2 reads past it")
    eoi_early = _gray(48, 8, six[:4])
    out["eoi_before_the_last_mcu"] = (48, 8, eoi_early, "gray", 1, "4 of 6 MCUs, then EOI")
    for n in (1, 100, 207):
        out["fat_block_cut_at_%d_bytes" % n] = (
            8, 192, _cut_in_fat(n), "420", 1,
            "the zeros after the data decode (FAT_AC's 1-bit code is EOB) and the block ends: 1 at its end")
    # a 16-bit pattern past maxcode[16]: FAT_DC / FAT_AC's 16-bit code is 1111111111111110
    out["dc_pattern_in_no_table_from_the_walk"] = (
        16, 8, _gray16(16, 8, [[[("raw", 16, 0xFFFF)]], [blk]]), "gray", 2, "sixteen ones: the walk passes length 16")
    out["ac_pattern_in_no_table_from_the_walk"] = (
        16, 8, _gray16(16, 8, [[[(0, 0), ("raw", 16, 0xFFFF)]], [blk]]), "gray", 2, "sixteen ones in the AC walk")
    out["zrl_from_k_49"] = (
        16, 8, _gray(16, 8, [[[(0, 0), ZRL, ZRL, ZRL, ZRL]], [blk]]), "gray", 3, "k = 49 + 15 passes 63")
    big = {(0, 0): FLAT16[(0, 0)], (1, 0): F.flat_code(list(range(0x0C)), 16)}
    out["ac_size_11_behind_a_16_bit_code"] = (
        16, 8, F.write_stream(16, 8, [[[(0, 0), (0, 11, 1030), EOB]], [blk]], q=ONES, huff=big, tq=(0,), td=(0,), ta=(0,)),
        "gray", 4, "symbol 0x0B from the walk")
    return out


def _gray16(w, h, mcus):
    return F.write_stream(w, h, mcus, q=ONES, huff=FAT_HUFF, tq=(0,), td=(0,), ta=(0,))
