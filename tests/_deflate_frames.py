"""A bit-exact RFC 1951 deflate writer and a counting reference inflater (pure Python; no zlib
encoder).  A stream is described block by block: stored blocks with chosen LEN / NLEN, fixed
blocks, dynamic blocks with chosen code lengths for all three alphabets, a chosen HCLEN and a chosen
spelling of the lengths (plain, or 16 / 17 / 18 repeats with chosen counts); tokens are literals,
or (length symbol, extra, distance symbol, extra), so non-canonical spellings (284 + 31) and the
unassigned symbols (286, 287, distance 30, 31) can be written.  The writer executes its tokens
and so knows the bytes; inflate() decodes exactly what the writer can write and returns the bytes
with a census of the paths taken.  tests/test_deflate_frames_host.py checks both against zlib."""
import struct
import zlib
from collections import namedtuple

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
         258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32

RING_DISTS = (16319, 16320, 16321, 16383, 16384, 16385, 32767, 32768)
MATCH_LENS = (3, 63, 64, 65, 258)

Built = namedtuple("Built", "frame content census")
Stored = namedtuple("Stored", "data len nlen final")
Fixed = namedtuple("Fixed", "tokens eob final")
Dyn = namedtuple("Dyn", "ll dl tokens items cl hclen eob final hlit hdist")


def stored(data, len_=None, nlen=None, final=None):
    return Stored(bytes(data), len_, nlen, final)


def fixed(tokens, eob=True, final=None):
    return Fixed(list(tokens), eob, final)


def dyn(ll, dl, tokens, items=None, cl=None, hclen=None, eob=True, final=None, hlit=None, hdist=None):
    """ll / dl: the literal/length and distance code lengths (HLIT / HDIST = their counts unless
    given); items: the lengths as code-length symbols, ints 0..15 or (16 | 17 | 18, repeat); cl: the
    19 lengths of the code-length code (default: a complete code over the symbols used)."""
    return Dyn(list(ll), list(dl), list(tokens), items, cl, hclen, eob, final, hlit, hdist)


def M(length, dist):
    """The canonical (length symbol, extra, distance symbol, extra) of a match."""
    ls = 28 if length == 258 else max(i for i in range(28) if LBASE[i] <= length)
    ds = max(i for i in range(30) if DBASE[i] <= dist)
    return (257 + ls, length - LBASE[ls], ds, dist - DBASE[ds])


def canon(lengths):
    """symbol -> (code, length), the canonical assignment (also of an incomplete set)."""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def complete_lengths(symbols, n):
    """n lengths, a complete code over `symbols` (>= 2 of them) with lengths as equal as can be."""
    symbols = sorted(set(symbols))
    assert len(symbols) >= 2
    k = (len(symbols) - 1).bit_length()
    short = (1 << k) - len(symbols)
    out = [0] * n
    for i, s in enumerate(symbols):
        out[s] = k - 1 if i < short else k
    return out


def staircase(symbols, n):
    """n lengths: symbols[0] gets 1 bit, symbols[1] 2 ... the last two the same (complete)."""
    assert 2 <= len(symbols) <= 16
    out = [0] * n
    for i, s in enumerate(symbols):
        out[s] = min(i + 1, len(symbols) - 1)
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):  # a Huffman code goes out most significant bit first
        code, k = c  # (an over-subscribed set's codes run past k bits: cut, the header is refused anyway)
        self.put(int(format(code & ((1 << k) - 1), "0%db" % k)[::-1], 2), k)

    def pos(self):
        return 8 * len(self.out) + self.n

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def _copy(out, dist, length):
    assert 1 <= dist <= len(out), "distance %d at %d" % (dist, len(out))
    if dist >= length:
        out += out[len(out) - dist:len(out) - dist + length]
    else:
        seg = bytes(out[len(out) - dist:])
        out += (seg * (length // dist + 1))[:length]


def _tokens(w, out, tokens, lc, dc, check):
    for t in tokens:
        if not isinstance(t, int) and t[0] == "phase":  # ("phase", P, filler symbol): fill up to bit phase P
            while w.pos() & 7 != t[1]:
                w.code(lc[t[2]])
                out.append(t[2])
            continue
        if isinstance(t, int):
            w.code(lc[t])
            if t < 256:
                out.append(t)
            continue
        ls, le, ds, de = t
        w.code(lc[ls])
        if ls - 257 < 29:
            w.put(le, LEXT[ls - 257])
        if ds is None:
            continue
        w.code(dc[ds])
        if ds < 30:
            w.put(de, DEXT[ds])
        if check:
            _copy(out, DBASE[ds] + de, LBASE[ls - 257] + le)


def default_items(lens):
    return list(lens)


def header_bits(b):
    """The bits of a dynamic block's header (BFINAL and BTYPE included)."""
    w = BitWriter()
    write_deflate(w, [b._replace(tokens=[], eob=False)], bytearray())
    return w.pos()


def write_deflate(w, blocks, out, check=True):
    """The blocks' bits (the last one final unless a block says otherwise); appends what they decode
    to to `out`.  check=False: matches are not executed (malformed streams)."""
    for i, b in enumerate(blocks):
        final = (i == len(blocks) - 1) if b.final is None else b.final
        w.put(int(final), 1)
        if isinstance(b, Stored):
            w.put(0, 2)
            w.align()
            n = len(b.data) if b.len is None else b.len
            w.put(n, 16)
            w.put(n ^ 0xFFFF if b.nlen is None else b.nlen, 16)
            w.out += b.data
            out += b.data
        elif isinstance(b, Fixed):
            w.put(1, 2)
            _tokens(w, out, b.tokens + ([256] if b.eob else []), canon(FIXED_LL), canon(FIXED_D), check)
        else:
            w.put(2, 2)
            hlit = len(b.ll) if b.hlit is None else b.hlit
            hdist = len(b.dl) if b.hdist is None else b.hdist
            items = default_items(b.ll + b.dl) if b.items is None else b.items
            used = {it if isinstance(it, int) else it[0] for it in items}
            cl = b.cl
            if cl is None:
                cl = complete_lengths(used | ({0, 8} if len(used) < 2 else set()), 19)
            hclen = b.hclen
            if hclen is None:
                hclen = max([4] + [k + 1 for k in range(19) if cl[CLORD[k]]])
            w.put(hlit - 257, 5)
            w.put(hdist - 1, 5)
            w.put(hclen - 4, 4)
            for k in range(hclen):
                w.put(cl[CLORD[k]], 3)
            cc = canon(cl)
            for it in items:
                if isinstance(it, int):
                    w.code(cc[it])
                else:
                    sym, rep = it
                    w.code(cc[sym])
                    w.put(rep - (11 if sym == 18 else 3), {16: 2, 17: 3, 18: 7}[sym])
            _tokens(w, out, b.tokens + ([256] if b.eob else []), canon(b.ll), canon(b.dl), check)


def zlib_header(cm=8, cinfo=7, fdict=0, flevel=0, fcheck=None):
    cmf = cinfo << 4 | cm
    flg = flevel << 6 | fdict << 5
    if fcheck is None:
        fcheck = (31 - (cmf * 256 + flg) % 31) % 31
    return bytes([cmf, flg | fcheck])


def build(blocks, wrap="zlib", check=True, census=True):
    """Built(frame, content, census).  wrap: "zlib" (RFC 1950), "raw", or "gzip" (a whole RFC 1952
    member: 10 header bytes, the body, CRC-32 and ISIZE)."""
    w, out = BitWriter(), bytearray()
    write_deflate(w, blocks, out, check)
    w.align()
    body, content = bytes(w.out), bytes(out)
    if wrap == "zlib":
        frame = zlib_header() + body + struct.pack(">I", zlib.adler32(content))
    elif wrap == "gzip":
        frame = b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + body + struct.pack("<II", zlib.crc32(content), len(content))
    else:
        frame = body
    cen = frozenset()
    if census:
        got, cen = inflate(body)
        assert got == content, "the reference inflater disagrees with the writer"
    return Built(frame, content, cen)


# ------------------------------------------------------------------- the reference inflater
class Malformed(Exception):
    pass


class _Bits:
    def __init__(self, data):
        self.d, self.p = data + b"\0" * 8, 0
        self.end = 8 * len(data)

    def peek(self, k):
        q = self.p >> 3
        return (int.from_bytes(self.d[q:q + 8], "little") >> (self.p & 7)) & ((1 << k) - 1)

    def get(self, k):
        v = self.peek(k)
        self.p += k
        if self.p > self.end:
            raise Malformed("input ends")
        return v


def _decoder(lengths):
    """(reversed code bits, length) -> symbol, and the set's state."""
    tab = {}
    for s, (code, k) in canon(lengths).items():
        tab[(int(format(code, "0%db" % k)[::-1], 2), k)] = s
    left = 1
    for k in range(1, 16):
        left = 2 * left - sum(1 for n in lengths if n == k)
        if left < 0:
            raise Malformed("over-subscribed")
    return tab, left, max(lengths) if lengths else 0


def _sym(br, tab):
    for k in range(1, 16):
        s = tab.get((br.peek(k), k))
        if s is not None:
            br.get(k)
            return s, k
    raise Malformed("unassigned code")


def inflate(body, zp_tokq=2048, zplut=10, blocks=None):
    """(bytes, census) of a raw deflate body the writer wrote.  The census names block framing,
    header forms, code lengths, base/extra entries, match geometry and the FIFO token positions
    (a literal or a match is one token of k_zarr_inflate2's FIFO, a non-empty stored block two).
    The fifo:stored_token_at_index_* and ring:*:phase:* items are a MODEL of the consumer's batches
    (tokens, or bytes, since the last stored run, modulo 64): a stored run does end a batch, but
    where the next ones end depends on what the producer has published when the consumer reads
    `tail`.  The cases make the modelled batch likely (the tokens of a small block are published
    in one store; 64 matches of 258 keep the consumer busy while the stored pair arrives), not
    certain; the bytes are checked whichever batches the run takes.
    blocks (a list): receives (first data bit, literal/length lengths, distance lengths, token starts)
    of every Huffman block."""
    br, out, cen = _Bits(body), bytearray(), set()
    prev, ntok, tiny, huff_end = None, 0, 0, None
    since = 0  # tokens since the last stored run: the consumer's batches start anew after one
    after_stored = False
    while True:
        final = br.get(1)
        typ = br.get(2)
        kind = ("stored", "fixed", "dynamic", None)[typ]
        if kind is None:
            raise Malformed("block type 3")
        cen.add("block:%s:%s" % (kind, "final" if final else "nonfinal"))
        if prev:
            cen.add("pair:%s>%s" % (prev, kind))
        if huff_end is not None:
            cen.add("huff_end_phase:%d>%s" % (huff_end, kind))
        huff_end = None
        if kind == "stored":
            pad = -br.p & 7
            if prev in ("fixed", "dynamic"):
                cen.add("stored_pad_after_huffman:%d" % pad)
            br.get(pad)
            n, nn = br.get(16), br.get(16)
            if n ^ 0xFFFF != nn:
                raise Malformed("NLEN")
            if n in (0, 1, 2, 3, 65535):
                cen.add("stored_len:%d" % n)
            q = br.p >> 3
            if q + n > len(body):
                raise Malformed("stored run past the input")
            out += body[q:q + n]
            br.p += 8 * n
            if n:
                if ntok % zp_tokq == zp_tokq - 1:
                    cen.add("fifo:stored_pair_straddles_wrap")
                if since % 64 in (62, 63):
                    cen.add("fifo:stored_token_at_index_%d_mod_64" % (since % 64))
                ntok += 2
                since = 0
            after_stored = True
        else:
            if kind == "fixed":
                ll, dl = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                if hlit > 286 or hdist > 30:
                    raise Malformed("too many symbols")
                for k, v in (("hlit", hlit), ("hdist", hdist), ("hclen", hclen)):
                    cen.add("%s:%d" % (k, v))
                cl = [0] * 19
                for k in range(hclen):
                    cl[CLORD[k]] = br.get(3)
                ctab, left, _ = _decoder(cl)
                if left:
                    raise Malformed("incomplete code-length code")
                lens = []
                while len(lens) < hlit + hdist:
                    s, k = _sym(br, ctab)
                    cen.add("clcode_len:%d" % k)
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16 and not lens:
                        raise Malformed("repeat first")
                    rep = br.get({16: 2, 17: 3, 18: 7}[s]) + (11 if s == 18 else 3)
                    cen.add("rep%d:%d" % (s, rep))
                    if len(lens) + rep > hlit + hdist:
                        raise Malformed("repeat overruns")
                    if s == 16 and len(lens) < hlit < len(lens) + rep:
                        cen.add("rep16_crosses_lit_dist")
                    lens += [lens[-1] if s == 16 else 0] * rep
                ll, dl = lens[:hlit], lens[hlit:]
                if not ll[256]:
                    raise Malformed("no end-of-block code")
            ltab, lleft, lmax = _decoder(ll)
            dtab, dleft, dmax = _decoder(dl)
            if (lleft and lmax > 1) or (dleft and dmax > 1):
                raise Malformed("incomplete set")
            if kind == "dynamic":
                if lleft:
                    cen.add("incomplete:eob_only_lit_code")
                if dleft:
                    cen.add("incomplete:single_dist_code" if dmax else "incomplete:no_dist_code")
            start, n0, o0 = br.p, ntok, len(out)
            starts = set()
            if blocks is not None:
                blocks.append((start, list(ll), list(dl), starts))
            if kind == "dynamic":
                cen.add("dynamic_data_phase:%d" % (start & 7))
            widths, all_long, run258, chain, plen = [], True, 0, 0, 0
            while True:
                p0 = br.p
                starts.add(p0)
                s, k = _sym(br, ltab)
                all_long = all_long and k > zplut
                if s == 256:
                    break
                if s < 256:
                    cen.add("lit_code_len:%d" % k)
                    out.append(s)
                    run258 = chain = plen = 0
                else:
                    if s > 285:
                        raise Malformed("length symbol")
                    cen.add("len_code_len:%d" % k)
                    e = LEXT[s - 257]
                    x = br.get(e)
                    length = LBASE[s - 257] + x
                    if length > 258:
                        raise Malformed("length")
                    for tag, hit in (("min", x == 0), ("max", x == (1 << e) - 1)):
                        if hit:
                            cen.add("lsym:%d:%s" % (s, tag))
                    ds, dk = _sym(br, dtab)
                    if ds > 29:
                        raise Malformed("distance symbol")
                    all_long = all_long and dk > zplut
                    cen.add("dist_code_len:%d" % dk)
                    de = DEXT[ds]
                    dx = br.get(de)
                    for tag, hit in (("min", dx == 0), ("max", dx == (1 << de) - 1)):
                        if hit:
                            cen.add("dsym:%d:%s" % (ds, tag))
                    dist = DBASE[ds] + dx
                    if dist > len(out):
                        raise Malformed("distance too far")
                    if k == 15 and e == 5 and dk == 15 and de == 13 and x in (0, 31) and dx in (0, 8191) and \
                            (x == 0) == (dx == 0):
                        cen.add("widest_token:phase:%d:extra:%s" % (p0 & 7, "ones" if x else "zeros"))
                    if dist <= 64 and length in MATCH_LENS:
                        cen.add("match:d%d:l%d" % (dist, length))
                    if dist == length:
                        cen.add("match:dist_eq_len")
                    if length == 258 and dist in RING_DISTS and after_stored and ntok - n0 < 64:
                        cen.add("ring:%d:phase:%d" % (dist, (len(out) - o0) & 63))
                    run258 = run258 + 1 if length == 258 else 0
                    chain = chain + 1 if 0 < plen and dist <= plen else 0  # the source lies in the match before
                    plen = length
                    if chain >= 4:
                        cen.add("match:sources_in_the_match_before:depth_4")
                    if run258 == 64:
                        cen.add("match:64_in_a_row_of_258")
                    _copy(out, dist, length)
                ntok += 1
                since += 1
                widths.append(br.p - p0)
            nb = ntok - n0
            huff_end = br.p & 7
            if nb == 0:
                cen.add("empty_block:%s" % kind)
            if 1 <= nb <= 3:
                tiny += 1
            if nb >= 64 and all_long:
                cen.add("block:every_code_longer_than_the_tables")
            if nb >= 3 * zp_tokq and len(set(widths)) == 1:
                cen.add("block:uniform_token_width:%d" % widths[0])
                cen.add("block:uniform_token_width:%d:phase:%d" % (widths[0], start & 7))
            if nb >= 3 * zp_tokq and max(widths) == 1:
                cen.add("block:1bit_literals_beyond_the_fifo")
            if nb >= 1024 and all(widths[i] == 44 and widths[i] == widths[i % 2] for i in range(nb)) and \
                    body[(start >> 3) + 1:(start >> 3) + 12] == body[(start >> 3) + 12:(start >> 3) + 23]:
                cen.add("block:two_token_period_of_88_bits")
            means = [sum(widths[i:i + 256]) / 256.0 for i in range(0, len(widths) - 255, 256)]
            if means and min(means) < 3 and max(means) > 40:
                cen.add("block:bits_per_token_swing_3_to_40")
            after_stored = False
        prev = kind
        if final:
            break
    if huff_end is not None:
        cen.add("huff_end_phase:%d>trailer" % huff_end)
    if tiny >= 16:
        cen.add("blocks_of_1_to_3_tokens:16")
    if ntok > 2 * zp_tokq:
        cen.add("fifo:more_than_2_tokq_tokens")
    if ntok >= 64:
        cen.add("fifo:tokens_mod_32:%d" % (ntok % 32))
    if (br.p + 7) >> 3 != len(body):
        raise Malformed("bytes after the last block")
    return bytes(out), frozenset(cen)


# ------------------------------------------- a model of k_zarr_inflate2's producer schedule
def _decode_at(br, pos, ltab, dtab):
    """zp_decode_at: (kind, bits) of the whole token at bit `pos`; kind "tok", "eob" or "bad"."""
    br.p = pos
    try:
        s, _ = _sym(br, ltab)
        if s == 256:
            return "eob", br.p - pos
        if s > 256:
            if s > 285:
                return "bad", 0
            br.p += LEXT[s - 257]
            d, _ = _sym(br, dtab)
            if d > 29:
                return "bad", 0
            br.p += DEXT[d]
    except Malformed:
        return "bad", 0
    return "tok", br.p - pos


def producer_schedule(body, sbits=128, seg_tok=24, smax=256):
    """zp_huff_block's macro-rounds over the Huffman blocks of a raw deflate body, as the code
    runs them while the FIFO never fills (a stream of fewer than ZP_TOKQ tokens): per round a dict
    of the block's index, the segment length S, the lanes whose segment starts on a true token
    start (`on_grid`), and `depth`, the iterations of pass B's outer loop (each hands the true
    chain on by one lane from every lane that already has it)."""
    blocks, rounds = [], []
    inflate(body, blocks=blocks)
    for bi, (B, ll, dl, starts) in enumerate(blocks):
        ltab, dtab = _decoder(ll)[0], _decoder(dl)[0]
        br = _Bits(body)
        br.end = 1 << 60
        while True:
            S = sbits
            b0 = [B + i * S for i in range(64)]
            xs, fl, vis = [0] * 64, ["tok"] * 64, [None] * 64

            def walk(i, p, old):  # lane i's chain from p; stops where it meets `old`
                seen = set()
                while True:
                    if old is not None and p - b0[i] in old:
                        return None
                    kind, adv = _decode_at(br, p, ltab, dtab)
                    seen.add(p - b0[i])
                    p += adv
                    if kind != "tok" or p >= b0[i] + S:
                        return p, kind, seen
            for i in range(64):
                xs[i], fl[i], vis[i] = walk(i, b0[i], None)
            chk, depth = list(b0), 0
            while True:
                ent = [B] + xs[:-1]
                todo = [i for i in range(1, 64) if fl[i - 1] == "tok" and ent[i] != chk[i]]
                if not todo:
                    break
                depth += 1
                for i in todo:
                    r = walk(i, ent[i], vis[i])
                    if r is not None:
                        xs[i], fl[i], vis[i] = r
                    else:  # met: the starts below the meeting point are the new chain's (not needed here)
                        pass
                    chk[i] = ent[i]
                # (a met chain keeps its exit; its record would be spliced, which changes no later meeting
                # at or above the meeting point -- and a later entry is never below an earlier one)
            ends = [i for i in range(64) if fl[i] != "tok"]
            last = ends[0] if ends else 63
            ent = [B] + xs[:-1]
            total = 0
            for i in range(last + 1):
                p = ent[i]
                while True:
                    kind, adv = _decode_at(br, p, ltab, dtab)
                    if kind != "tok":
                        break
                    total += 1
                    p += adv
                    if p >= b0[i] + S:
                        break
            nB = xs[last]
            rounds.append(dict(block=bi, S=S, depth=depth, tokens=total,
                               on_grid=[i for i in range(64) if b0[i] in starts]))
            if total:
                bpt = ((nB - B) * seg_tok + total - 1) // total
                sbits = 64 if bpt < 64 else smax if bpt > smax else (bpt + 7) & ~7
            if ends:
                break
            B = nB
    return rounds
