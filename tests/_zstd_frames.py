"""A deterministic Zstandard (RFC 8878) frame writer for the decoder tests: pure Python, no use
of libzstd's encoder.  A frame is built from an explicit description (header options, a list
of raw / RLE / compressed blocks; per compressed block the literal bytes and their mode, the
(literal_length, offset_value, match_length) sequences and the mode of each of the three
tables), so a test chooses the format path instead of hoping an encoder takes it.

build() returns the frame, the bytes it must decode to (a small sequence executor with the RFC's
repeat-offset rules) and a census of what was emitted, which test_zstd_frames_host.py checks
against a written-out checklist.

FSE: the decoding table is built as the RFC describes and the encoder is its inverse (walking
the symbols last to first, picking the entry of the symbol whose [base, base + 2^nb) holds the
following state), so the two cannot disagree and the bits each sequence reads (T) are known.
"""
from collections import namedtuple

LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256,
           512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1,
          -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
assert len(LL_BASE) == len(LL_BITS) == len(LL_DEF) == 36 and len(ML_BASE) == len(ML_BITS) == len(ML_DEF) == 53
assert len(OF_DEF) == 29
KINDS = ("LL", "OF", "ML")
DEFS = {"LL": (LL_DEF, 6), "OF": (OF_DEF, 5), "ML": (ML_DEF, 6)}
MAX_LOG = {"LL": 9, "OF": 8, "ML": 9}
MAX_SYM = {"LL": 35, "OF": 31, "ML": 52}
RING_OFFSETS = (4031, 4032, 4033, 4095, 4096, 4097)

Tab = namedtuple("Tab", "entries log origin")  # entries: (symbol, nbBits, baseline) per state


def O(offset):
    """The offset_value of a new (non-repeat) offset."""
    return offset + 3


def code_of(value, base, bits):
    c = max(k for k in range(len(base)) if base[k] <= value)
    assert value < base[c] + (1 << bits[c]), value
    return c, value - base[c], bits[c]


# --------------------------------------------------------------------------- bit packing
def pack_forward(fields):
    """(value, nbits) fields, LSB first, zero-padded to a byte."""
    out, acc, n = bytearray(), 0, 0
    for v, nb in fields:
        assert 0 <= v < (1 << nb) or (nb == 0 and v == 0), (v, nb)
        acc |= v << n
        n += nb
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8
    if n:
        out.append(acc)
    return bytes(out)


def pack_backward(fields, extra_zero_bits=0):
    """A backward bitstream that a decoder reads as `fields` in the order given: the last field
    is written first, then the end mark.  extra_zero_bits: bits nobody reads, below the first
    field (malformed streams)."""
    out, acc, n = bytearray(), 0, extra_zero_bits
    while n >= 8:
        out.append(0)
        n -= 8
    for v, nb in reversed(fields):
        assert 0 <= v < (1 << nb) or (nb == 0 and v == 0), (v, nb)
        acc |= v << n
        n += nb
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8
    out.append(acc | (1 << n))
    return bytes(out)


# ---------------------------------------------------------------------------------- FSE
def fse_table(norm, log, origin="fse"):
    size = 1 << log
    assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
    sym = [None] * size
    high = size - 1
    nxt = {}
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
            nxt[s] = 1
        else:
            nxt[s] = c
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0 and None not in sym
    entries = []
    for u in range(size):
        s = sym[u]
        ns = nxt[s]
        nxt[s] += 1
        nb = log - (ns.bit_length() - 1)
        entries.append((s, nb, (ns << nb) - size))
    return Tab(entries, log, origin)


def rle_table(symbol):
    return Tab([(symbol, 0, 0)], 0, "rle")


def fse_states(tab, syms):
    """One state per symbol: tab.entries[st[i]] carries syms[i] and its range holds st[i + 1].
    The last state is the symbol's first (the one with the most update bits)."""
    by = {}
    for u, (s, nb, base) in enumerate(tab.entries):
        by.setdefault(s, []).append((u, nb, base))
    for s in set(syms):
        assert s in by, "symbol %d has no state in the table" % s
    st = [0] * len(syms)
    st[-1] = by[syms[-1]][0][0]
    for i in range(len(syms) - 2, -1, -1):
        for u, nb, base in by[syms[i]]:
            if base <= st[i + 1] < base + (1 << nb):
                st[i] = u
                break
        else:
            raise AssertionError("no state")
    return st


def write_ncount(norm, log):
    """FSE_NCount (RFC 8878 4.1.1) of a count vector (-1: "less than 1"; the last count is not 0)."""
    assert norm[-1] != 0 and sum(abs(c) for c in norm) == 1 << log
    f = [(log - 5, 4)]
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    sym, prev0 = 0, False
    while remaining > 1:
        if prev0:
            run = 0
            while norm[sym] == 0:
                sym += 1
                run += 1
            while run >= 3:
                f.append((3, 2))
                run -= 3
            f.append((run, 2))
        count = norm[sym]
        sym += 1
        maxv = 2 * threshold - 1 - remaining
        remaining -= abs(count)
        v = count + 1
        if v >= threshold:
            v += maxv
        f.append((v, nb - 1) if v < maxv else (v, nb))
        prev0 = count == 0
        while remaining < threshold and nb > 1:
            nb -= 1
            threshold >>= 1
    assert sym == len(norm)
    return pack_forward(f)


def ncount_features(norm, log, kind):
    out = set()
    if -1 in norm:
        out.add("fse:less_than_one")
    run = best = 0
    for c in norm:
        run = run + 1 if c == 0 else 0
        best = max(best, run)
    if best >= 6:
        out.add("fse:zero_run_3_3_r")
    if kind in MAX_LOG and log == MAX_LOG[kind]:
        out.add("fse:max_log:" + kind)
    return out


# ------------------------------------------------------------------------------ Huffman
def huf_codes(weights):
    """weights[s] for every symbol 0..max (the last one non-zero) -> table log, {s: (code, nbits)}
    in the RFC's order: weight 1 first, symbols ascending within a weight."""
    total = sum(1 << (w - 1) for w in weights if w)
    hlog = total.bit_length() - 1
    assert total == 1 << hlog and weights[-1], "weights do not fill a power of two"
    codes, idx = {}, 0
    for w in range(1, hlog + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (idx >> (w - 1), hlog + 1 - w)
                idx += 1 << (w - 1)
    assert idx == total
    return hlog, codes


def huf_stream(codes, data, extra_zero_bits=0):
    return pack_backward([codes[b] for b in data], extra_zero_bits)


def tree_direct(listed):
    """Tree description as 4-bit weights (the last symbol's weight is implied, not listed)."""
    n = len(listed)
    assert 1 <= n <= 128
    nib = list(listed) + [0] * (n & 1)
    return bytes([127 + n]) + bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2))


def tree_fse(listed, norm, log):
    """Tree description as FSE-compressed weights: two interleaved states over one table."""
    n = len(listed)
    assert n >= 2
    tab = fse_table(norm, log)
    chains = [listed[0::2], listed[1::2]]
    sts = [fse_states(tab, c) for c in chains]
    fields = [(sts[0][0], log), (sts[1][0], log)]
    for i in range(n - 2):  # the update after weight i gives the state of weight i + 2
        _, nb, base = tab.entries[sts[i & 1][i >> 1]]
        fields.append((sts[i & 1][(i >> 1) + 1] - base, nb))
    # the update after weight n - 2 must over-read (that ends the loop): its state has bits
    assert tab.entries[sts[(n - 2) & 1][(n - 2) >> 1]][1] > 0
    body = write_ncount(norm, log) + pack_backward(fields)
    assert len(body) < 128
    return bytes([len(body)]) + body


# -------------------------------------------------------------------------------- XXH64
_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                           0x27D4EB2F165667C5)


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, v):
    return _rotl((acc + v * _P2) & _M, 31) * _P1 & _M


def xxh64(data, seed=0):
    n, i = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = _round(v[k], int.from_bytes(data[i + 8 * k:i + 8 * k + 8], "little"))
            i += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for k in range(4):
            h = ((h ^ _round(0, v[k])) * _P1 + _P4) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[i:i + 8], "little")), 27) * _P1 + _P4) & _M
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        i += 4
    while i < n:
        h = _rotl(h ^ (data[i] * _P5 & _M), 11) * _P1 & _M
        i += 1
    h ^= h >> 33
    h = h * _P2 & _M
    h ^= h >> 29
    h = h * _P3 & _M
    h ^= h >> 32
    return h


# --------------------------------------------------------------------- block descriptions
class Comp:
    """A compressed block.

    literals: the block's literal bytes.  lit: "raw" | "rle" | "huf" | "treeless"; lit_sf: the
    Size_Format (None: the smallest that fits; Huffman: 0 = one stream, 1..3 = four streams).
    weights: for "huf", the weight of every symbol 0..max (None: a flat tree over the symbols);
    tree: "direct" | ("fse", norm, log).  seqs: (literal_length, offset_value, match_length).
    modes: for LL, OF, ML each "predef" | "rle" | ("fse", norm, log) | "repeat".
    nseq_bytes: force the 2- or 3-byte Number_of_Sequences form.
    The remaining arguments write malformed blocks (see _zstd_cases.MALFORMED)."""

    def __init__(self, literals=b"", seqs=(), lit="raw", lit_sf=None, weights=None, tree="direct",
                 modes=("predef", "predef", "predef"), nseq_bytes=None, modes_low_bits=0, tail=b"",
                 extra_zero_bits=0, listed_weights=None, huf_extra_zero_bits=0, jump_add=0, pad_to=0,
                 rle_symbols=None, ncount_raw=None):
        self.literals, self.seqs, self.lit, self.lit_sf = bytes(literals), list(seqs), lit, lit_sf
        self.weights, self.tree, self.modes, self.nseq_bytes = weights, tree, modes, nseq_bytes
        self.modes_low_bits, self.tail, self.extra_zero_bits = modes_low_bits, tail, extra_zero_bits
        self.listed_weights, self.huf_extra_zero_bits, self.jump_add = listed_weights, huf_extra_zero_bits, jump_add
        self.pad_to, self.rle_symbols, self.ncount_raw = pad_to, rle_symbols or {}, ncount_raw or {}


Built = namedtuple("Built", "frame content census")


class _Writer:
    def __init__(self, check):
        self.check = check
        self.out = bytearray()
        self.reps = [1, 4, 8]
        self.tabs = {k: None for k in KINDS}
        self.huf = None  # (hlog, codes)
        self.census = set()
        self.max_T = 0
        self.prev_block = None         # type of the block before this one
        self.comp_blocks = 0
        self.lit_since_tree = None     # literal modes of the blocks since the last tree
        self.nseq0_since = {k: False for k in KINDS}

    # ---- literals
    def literals_section(self, b):
        c, lits, n = self.census, b.literals, len(b.literals)
        if b.lit in ("raw", "rle"):
            sf = b.lit_sf if b.lit_sf is not None else (0 if n < 32 else 1 if n < 4096 else 3)
            t = 0 if b.lit == "raw" else 1
            if sf in (0, 2):
                assert n < 32
                hdr = bytes([(n << 3) | (sf << 2) | t])
            elif sf == 1:
                assert n < 4096
                hdr = ((n << 4) | (1 << 2) | t).to_bytes(2, "little")
            else:
                assert n < (1 << 20)
                hdr = ((n << 4) | (3 << 2) | t).to_bytes(3, "little")
            c.add("lit:%s:%dB" % (b.lit, len(hdr)))
            if self.lit_since_tree is not None:
                self.lit_since_tree.add(b.lit)
            if b.lit == "rle":
                assert not self.check or (n and lits == lits[:1] * n)
                return hdr + lits[:1]
            return hdr + lits
        body = b""
        if b.lit == "huf":
            weights = b.weights
            if weights is None:  # a flat tree over the symbols 0..max (max + 1 a power of two)
                weights = [1] * (max(lits) + 1)
            listed = list(weights[:-1]) if b.listed_weights is None else list(b.listed_weights)
            if b.listed_weights is None:
                self.huf = huf_codes(list(weights))
                if self.huf[0] == 11:
                    c.add("huf:table_log_11")
            if b.tree == "direct":
                body = tree_direct(listed)
                c.add("tree:direct:%s" % ("odd" if len(listed) & 1 else "even"))
            else:
                _, norm, log = b.tree
                body = tree_fse(listed, norm, log)
                # an even number of listed weights leaves the loop after a state-1 update
                c.add("tree:fse:exit_after_state%d" % (1 if len(listed) % 2 == 0 else 2))
                c.update(ncount_features(norm, log, "W"))
            self.lit_since_tree = set()
        else:
            if self.check:
                assert self.huf is not None
            if self.lit_since_tree is not None:
                c.add("treeless:after:" + "+".join(sorted(self.lit_since_tree | {"huf"})))
        if self.huf is None:  # malformed (no tree, or one that cannot be built): any codes will do
            assert not self.check
            self.huf = huf_codes([1] * 256)
        hlog, codes = self.huf
        sf = b.lit_sf if b.lit_sf is not None else (0 if n < 1024 else 2)
        if sf == 0:
            body += huf_stream(codes, lits, b.huf_extra_zero_bits)
            streams = 1
        else:
            per = (n + 3) // 4
            parts = [huf_stream(codes, lits[k * per:(k + 1) * per], b.huf_extra_zero_bits if k == 0 else 0)
                     for k in range(4)]
            jt = [len(p) for p in parts[:3]]
            jt[2] += b.jump_add
            body += b"".join(x.to_bytes(2, "little") for x in jt) + b"".join(parts)
            streams = 4
        nbits, hs = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[sf]
        assert n < (1 << nbits) and len(body) < (1 << nbits), (n, len(body), nbits)
        t = 2 if b.lit == "huf" else 3
        c.add("lit:%s:sf%d:%dstream" % (b.lit, sf, streams))
        return (t | (sf << 2) | (n << 4) | (len(body) << (4 + nbits))).to_bytes(hs, "little") + body

    # ---- sequences
    def table_for(self, kind, mode, syms, b):
        c = self.census
        if mode == "predef":
            norm, log = DEFS[kind]
            self.tabs[kind] = fse_table(norm, log, "predef")
            c.add("%s:predef" % kind)
            return 0, b""
        if mode == "rle":
            s = b.rle_symbols.get(kind, syms[0])
            assert not self.check or set(syms) == {s}
            self.tabs[kind] = rle_table(syms[0])
            c.add("%s:rle" % kind)
            return 1, bytes([s])
        if mode == "repeat":
            if self.tabs[kind] is None:  # malformed: nothing to repeat; encode with the predefined one
                assert not self.check
                norm, log = DEFS[kind]
                self.tabs[kind] = fse_table(norm, log, "none")
            c.add("%s:repeat:%s" % (kind, self.tabs[kind].origin))
            if self.nseq0_since[kind]:
                c.add("%s:repeat:across_nseq0" % kind)
            return 3, b""
        if kind in b.ncount_raw:  # a malformed description: the bitstream after it does not matter
            self.tabs[kind] = fse_table(*DEFS[kind])
            return 2, b.ncount_raw[kind]
        _, norm, log = mode
        assert log <= MAX_LOG[kind] and len(norm) <= MAX_SYM[kind] + 1
        self.tabs[kind] = fse_table(norm, log)
        c.add("%s:fse" % kind)
        c.update(ncount_features(norm, log, kind))
        return 2, write_ncount(norm, log)

    def sequences_section(self, b, block_start):
        c, n = self.census, len(b.seqs)
        if b.nseq_bytes == 3 or (b.nseq_bytes is None and n >= 0x7F00):
            hdr = bytes([255]) + (n - 0x7F00).to_bytes(2, "little")
        elif b.nseq_bytes == 2 or (b.nseq_bytes is None and n >= 128):
            assert n < 0x7F00
            hdr = bytes([128 + (n >> 8), n & 255])
        else:
            assert n < 128
            hdr = bytes([n])
        c.add("nseq:%dB" % len(hdr))
        if n == 0:
            c.add("nseq:0")
            for k in KINDS:
                if self.tabs[k] is not None:
                    self.nseq0_since[k] = True
            return hdr + b.tail
        codes = {"LL": [], "OF": [], "ML": []}
        for ll, ofv, ml in b.seqs:
            codes["LL"].append(code_of(ll, LL_BASE, LL_BITS))
            codes["ML"].append(code_of(ml, ML_BASE, ML_BITS))
            oc = ofv.bit_length() - 1
            codes["OF"].append((oc, ofv - (1 << oc), oc))
        mbyte, desc = b.modes_low_bits, b""
        for k, kind in enumerate(KINDS):
            m, d = self.table_for(kind, b.modes[k], [x[0] for x in codes[kind]], b)
            mbyte |= m << (6 - 2 * k)
            desc += d
            self.nseq0_since[kind] = False
        tabs = [self.tabs[k] for k in KINDS]
        sts = [fse_states(tabs[k], [x[0] for x in codes[kind]]) for k, kind in enumerate(KINDS)]
        fields = [(sts[0][0], tabs[0].log), (sts[1][0], tabs[1].log), (sts[2][0], tabs[2].log)]
        for i in range(n):
            T = 0
            for kind in ("OF", "ML", "LL"):
                _, extra, nb = codes[kind][i]
                fields.append((extra, nb))
                T += nb
            if i + 1 < n:
                for k in (0, 2, 1):  # literal lengths, match lengths, offsets
                    _, nb, base = tabs[k].entries[sts[k][i]]
                    fields.append((sts[k][i + 1] - base, nb))
                    T += nb
            self.max_T = max(self.max_T, T)
            if T in (56, 57):
                c.add("T:%d" % T)
            if T > 57:
                c.add("T:>57")
        return hdr + bytes([mbyte]) + desc + pack_backward(fields, b.extra_zero_bits) + b.tail

    # ---- the expected bytes
    def execute(self, b):
        out, lits, reps, c, lp = self.out, b.literals, self.reps, self.census, 0
        n = len(b.seqs)
        if n in (64, 65):
            c.add("batch:%d_sequences" % n)
        batch_op0 = len(out)
        for i, (ll, ofv, ml) in enumerate(b.seqs):
            if i % 64 == 0:
                batch_op0 = len(out)
            if ll and lp // 256 != (lp + ll - 1) // 256:
                c.add("literal_run_crosses_256B_window")
            out += lits[lp:lp + ll]
            lp += ll
            if ofv > 3:
                off = ofv - 3
                reps[:] = [off, reps[0], reps[1]]
            else:
                idx = ofv - 1 + (1 if ll == 0 else 0)
                c.add("rep:case%d%s" % (idx, ":ll0" if ll == 0 else ""))
                if i == 0 and self.comp_blocks > 1:
                    c.add("rep:first_sequence_after_%s_block" % self.prev_block)
                if idx == 0:
                    off = reps[0]
                elif idx == 1:
                    off = reps[1]
                    reps[:] = [off, reps[0], reps[2]]
                elif idx == 2:
                    off = reps[2]
                    reps[:] = [off, reps[0], reps[1]]
                else:
                    off = reps[0] - 1
                    reps[:] = [off, reps[0], reps[1]]
            if self.check:
                assert 0 < off <= len(out), (i, off, len(out))
            elif not 0 < off <= len(out):
                return  # (malformed: the content is not defined)
            if off in RING_OFFSETS:
                c.add("ring:%d:phase%d" % (off, (len(out) - batch_op0) % 64))
            if off <= 64 and ml >= 192:
                c.add("period:%d:several_steps" % off)
            if off >= ml:
                out += out[len(out) - off:len(out) - off + ml]
            else:
                seg = bytes(out[len(out) - off:])
                out += (seg * (ml // off + 1))[:ml]
        assert not self.check or lp <= len(lits)
        out += lits[lp:]


def build(blocks, fcs="auto", single=None, checksum=False, check=True, declared=None, bad_checksum=False):
    """blocks: ("raw", bytes) | ("rle", byte value, count) | Comp.  fcs: the Frame_Content_Size
    field's bytes (0, 1, 2, 4, 8; "auto": the smallest).  single: Single_Segment (None: whenever the
    field allows).  check=False writes malformed frames (no assertion on the sequences); `declared`
    is then the content size the header states."""
    w = _Writer(check)
    body = bytearray()
    for k, b in enumerate(blocks):
        last = 1 if k == len(blocks) - 1 else 0
        if not isinstance(b, Comp) and b[0] == "raw":
            data = bytes(b[1])
            body += (last | (len(data) << 3)).to_bytes(3, "little") + data
            w.out += data
            w.census.add("block:raw")
            w.prev_block = "raw"
        elif not isinstance(b, Comp) and b[0] == "rle":
            body += (last | 2 | (b[2] << 3)).to_bytes(3, "little") + bytes([b[1]])
            w.out += bytes([b[1]]) * b[2]
            w.census.add("block:rle")
            w.prev_block = "rle"
        else:
            w.comp_blocks += 1
            start = len(w.out)
            payload = w.literals_section(b) + w.sequences_section(b, start)
            payload += bytes(max(0, b.pad_to - len(payload)))
            assert len(payload) < (1 << 21)
            assert not check or len(payload) <= 128 * 1024
            body += (last | 4 | (len(payload) << 3)).to_bytes(3, "little") + payload
            w.execute(b)
            assert not check or len(w.out) - start <= 128 * 1024
            w.census.add("block:compressed")
            w.prev_block = "compressed"
    content = bytes(w.out)
    n = len(content) if declared is None else declared
    if fcs == "auto":
        fcs = 1 if n < 256 and single is not False else 2 if 256 <= n < 65536 + 256 else 4
    if single is None:
        single = fcs != 0
    assert not (fcs == 1 and not single) and not (fcs == 0 and single)
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    hdr = bytes([0x28, 0xB5, 0x2F, 0xFD, (flag << 6) | (int(single) << 5) | (int(checksum) << 2)])
    if not single:
        exp = max(0, (max(n, 1) - 1).bit_length() - 10)
        hdr += bytes([exp << 3])  # Window_Size = 2^(10 + exp) >= the content
    if fcs:
        hdr += (n - 256 if fcs == 2 else n).to_bytes(fcs, "little")
    frame = hdr + bytes(body)
    if checksum:
        frame += ((xxh64(content) ^ (1 if bad_checksum else 0)) & 0xFFFFFFFF).to_bytes(4, "little")
    c = w.census
    c.add("fcs:%dB" % fcs)
    c.add("single_segment" if single else "window_descriptor")
    c.add("checksum:on" if checksum else "checksum:off")
    c.add("max_T:%d" % w.max_T)
    return Built(frame, content, frozenset(c))
