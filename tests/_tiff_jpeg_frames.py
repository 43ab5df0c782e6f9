"""Hand-built baseline JPEG scans for k_tiff_jpeg_decode, and a model of what its wave does with
them.

The writer states a scan symbol by symbol: per-component table ids (quantiser, DC and AC ids 0 .. 3,
all three components different if wanted), arbitrary (bits, vals) codes, blocks as explicit symbol
lists -- (DC size, value bits), then (run, size, value bits) .., ZRL or EOB -- so a case chooses
every bit, and named raw edits of the finished entropy bytes (fill bytes in front of a marker, no
EOI, bytes appended).

schedule() restates, from the text of kernels_tiff_jpeg.hip, the decoder's wave on a stream: the
refill rounds of 64 raw bytes (what each lane keeps or drops, the first marker lane, why a refill
ended), every refill call (byte0, skip, rem, rounds), the batches of whole MCUs, where restarts fall
in them, and every symbol (table, class, code length, LUT or walk) and receive (size, bit pattern).
It decodes from its own clean-byte buffer, so it is a second decoder: its error code is the code
the device must give, and its coefficients are held equal to _tiff_jpeg.decode_coefficients' by
tests/test_tiff_jpeg_frames_host.py.  The census is a Counter of string keys, as _lz_frames.py's."""
import struct
from collections import Counter

import numpy as np

import _tiff_jpeg as J

# kernels_tiff_jpeg.hip's constants (pinned against its text by the host test)
J_CAP, J_PAD, J_LOW, J_BLK = 1024, 320, 256, 132
KERNEL_CONSTANTS = dict(J_CAP=J_CAP, J_PAD=J_PAD, J_LOW=J_LOW, J_BLK=J_BLK)
J_CLEANSZ = J_CAP + 64 + J_PAD
FAT = 27 + 63 * 26  # the most bits a block can take: DC 16 + 11, 63 x (16 + 10)

EOB, ZRL = (0, 0, 0), (15, 0, 0)


# ------------------------------------------------------------------------------ codes
def flat_code(symbols, length=4):
    """Every symbol the same length.  (libjpeg refuses a code that uses the all-ones word: at most
    2^length - 1 symbols.)"""
    symbols = list(symbols)
    assert len(symbols) < 1 << length
    bits = [0] * 16
    bits[length - 1] = len(symbols)
    return bits, symbols


def ladder_code(symbols, lengths):
    """One symbol at each of `lengths` (ascending; symbols[i] gets lengths[i])."""
    symbols, lengths = list(symbols), list(lengths)
    assert len(symbols) == len(lengths) and lengths == sorted(lengths)
    bits = [0] * 16
    for l in lengths:
        bits[l - 1] += 1
    assert sum(b << (16 - l) for l, b in enumerate(bits, 1)) < 65536
    return bits, symbols


FLAT_DC = flat_code(range(12))
FLAT_AC = flat_code([0x00, 0x01, 0x02, 0x04, 0x08, 0x0A, 0xF0, 0x11, 0xE1, 0xF1])


# ------------------------------------------------------------------------------ symbols
def value_bits(v, size=None):
    """(size, bits) of a coefficient or DC difference."""
    s = J._category(v) if size is None else size
    return s, (v if v > 0 else v + (1 << s) - 1) if s else 0


def block_symbols(coefs, pred=0, keep_eob=True):
    """The symbol list of a block of 64 zigzag coefficients after DC predictor `pred`."""
    out = [value_bits(int(coefs[0]) - pred)]
    run = 0
    for k in range(1, 64):
        x = int(coefs[k])
        if x == 0:
            run += 1
            continue
        while run > 15:
            out.append(ZRL)
            run -= 16
        out.append((run,) + value_bits(x))
        run = 0
    if run and keep_eob:
        out.append(EOB)
    return out


def mcus_of(blocks, sampling=(1, 1), restart=0, keep_eob=True):
    """MCUs (lists of symbol lists, scan order) from per-component coefficient arrays (block rows,
    block cols, 64) over the MCU-padded grid; predictors reset every `restart` MCUs."""
    nc = len(blocks)
    hs, vs = sampling if nc == 3 else (1, 1)
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    mcuy, mcux = blocks[0].shape[0] // vs, blocks[0].shape[1] // hs
    out, pred = [], [0] * nc
    for m in range(mcux * mcuy):
        if restart and m % restart == 0:
            pred = [0] * nc
        mx, my = m % mcux, m // mcux
        mcu = []
        for c in range(nc):
            h, v = samp[c]
            for b in range(h * v):
                blk = blocks[c][my * v + b // h, mx * h + b % h]
                mcu.append(block_symbols(blk, pred[c], keep_eob))
                pred[c] = int(blk[0])
        out.append(mcu)
    return out


# ------------------------------------------------------------------------------ the writer
def write_stream(width, height, mcus, nc=1, sampling=(1, 1), q=None, huff=None, tq=(0, 1, 1), td=(0, 1, 1),
                 ta=(0, 1, 1), restart=0, dri=None, tables_in_stream=True, comp_ids=(1, 2, 3), marker=None, junk=None):
    """A baseline stream.  mcus: per MCU its blocks in scan order, each a symbol list: (DC size,
    bits), then (run, size, bits) ..; a ("raw", nbits, value) item writes bits as they are.  q =
    {id: 64 zigzag values}; huff = {(class, id): (bits, vals)}; tq / td / ta name the tables of
    each component.  A marker RSTn stands after every `restart` MCUs (dri: the interval the DRI
    segment declares, if another; marker(n) -> code of the n-th marker, if another; junk(n) ->
    clean bytes written between interval n and its marker)."""
    T = J.std_tables()
    q = q if q is not None else T["q"]
    huff = huff if huff is not None else T["h"]
    hs, vs = sampling if nc == 3 else (1, 1)
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    out = bytearray(b"\xff\xd8")
    if tables_in_stream:
        for i in sorted(q):
            out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(int(x) for x in q[i])
        for (tc, th), (bits, vals) in sorted(huff.items()):
            out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc << 4 | th) + bytes(bits) + bytes(vals)
    out += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * nc, 8, height, width, nc)
    for c in range(nc):
        out += bytes([comp_ids[c], samp[c][0] << 4 | samp[c][1], tq[c]])
    dri = restart if dri is None else dri
    if dri:
        out += b"\xff\xdd" + struct.pack(">HH", 4, dri)
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * nc, nc)
    for c in range(nc):
        out += bytes([comp_ids[c], td[c] << 4 | ta[c]])
    out += bytes([0, 63, 0])
    enc = {k: J._enc_table(*v) for k, v in huff.items()}
    comp_of = [c for c in range(nc) for _ in range(samp[c][0] * samp[c][1])]
    wr, n = J._Writer(), 0
    for m, mcu in enumerate(mcus):
        if restart and m and m % restart == 0:
            out += wr.flush() + (junk(n) if junk else b"") + bytes([0xFF, marker(n) if marker else 0xD0 + (n & 7)])
            n += 1
        assert len(mcu) == len(comp_of), "an MCU of %d blocks" % len(mcu)
        for c, syms in zip(comp_of, mcu):
            dc, ac = enc[(0, td[c])], enc[(1, ta[c])]
            for i, item in enumerate(syms):
                if item[0] == "raw":
                    wr.put(item[2], item[1])
                elif i == 0:
                    wr.put(dc[item[0]][1], dc[item[0]][0])
                    wr.put(item[1], item[0])
                else:
                    rs = item[0] << 4 | item[1]
                    wr.put(ac[rs][1], ac[rs][0])
                    wr.put(item[2], item[1])
    return bytes(out) + wr.flush() + b"\xff\xd9"


# raw edits of a finished stream's entropy bytes
def _markers(stream):
    """Offsets of the FF of every marker in the entropy-coded data (RSTn, EOI)."""
    out, i = [], J.header(stream)["data"]
    while i + 1 < len(stream):
        if stream[i] == 0xFF and stream[i + 1] not in (0x00, 0xFF):
            out.append(i)
            i += 2
        else:
            i += 1
    return out


def fill_before_markers(stream, n, which=None):
    """n fill bytes (FF) in front of every marker of the entropy data (which: a set of marker
    indices, if not all).  Legal per T.81 B.1.1.2."""
    b = bytearray(stream)
    for k, at in reversed(list(enumerate(_markers(stream)))):
        if which is None or k in which:
            b[at:at] = b"\xff" * n
    return bytes(b)


def drop_eoi(stream):
    assert stream[-2:] == b"\xff\xd9"
    return stream[:-2]


def append_bytes(stream, tail):
    return stream + bytes(tail)


def entropy(stream):
    return stream[J.header(stream)["data"]:]


# ------------------------------------------------------------------------------ padding blocks
def padding_blocks(stream):
    """Per component a bool array (block rows, block cols): the blocks that lie entirely outside
    width x height (at the component's own resolution), so no sample of theirs is ever placed."""
    H = J.header(stream)
    nc = len(H["comps"])
    hs, vs = (H["comps"][0][1], H["comps"][0][2]) if nc == 3 else (1, 1)
    w, h = H["width"], H["height"]
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    out = []
    for c in range(nc):
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        cw, chh = (w, h) if c == 0 else (-(-w // hs), -(-h // vs))
        m = np.zeros((mcuy * cv, mcux * ch), bool)
        m[-(-chh // 8):, :] = True
        m[:, -(-cw // 8):] = True
        out.append(m)
    return out


# ------------------------------------------------------------------------------ the schedule model
class _Huff:
    """JHuff as jpeg_build_huff makes it."""

    def __init__(self, bits, vals):
        self.lut, self.maxcode, self.valoff = [0] * 512, [-1] * 18, [0] * 18
        self.val = list(vals) + [0] * (256 - len(vals))
        code = p = 0
        for l in range(1, 17):
            self.valoff[l] = p - code
            for _ in range(bits[l - 1]):
                if l <= 9:
                    for k in range(1 << (9 - l)):
                        self.lut[(code << (9 - l)) + k] = l << 8 | vals[p]
                p += 1
                code += 1
            if bits[l - 1]:
                self.maxcode[l] = code - 1
            code <<= 1


def _patterns(size, bits):
    """The named extreme patterns `bits` of `size` bits is."""
    out = []
    if bits == 0:
        out.append("zeros")
    if bits == (1 << size) - 1:
        out.append("ones")
    if bits == (1 << (size - 1)) - 1:
        out.append("0111")
    if bits == 1 << (size - 1):
        out.append("1000")
    return out


class _Wave:
    """The decoder's stream state (JBits) over its LDS clean-byte buffer."""

    def __init__(self, raw, census, mutate=None):
        self.raw, self.csize, self.cs, self.mutate = raw, len(raw), census, mutate
        self.buf = bytearray(J_CLEANSZ)
        self.pos = self.cend = self.rawp = self.pend = 0  # pos: bits consumed (cp * 8 - nb)

    def refill(self, why):
        raw, csize, cs = self.raw, self.csize, self.cs
        byte0 = min(self.pos >> 3, self.cend)
        skip = self.pos - byte0 * 8
        rem = self.cend - byte0
        cs["refill:" + why] += 1
        if byte0:
            iters = len(range(0, rem, 256))
            cs["move:iterations:%d" % iters] += 1
            cs["refill:moved"] += 1
            if skip < 8:
                cs["skip:%d" % skip] += 1
            self.buf[0:rem] = self.buf[byte0:byte0 + rem]
        cend, rawp, pend, rounds, end = rem, self.rawp, self.pend, 0, "none"
        while not pend and cend <= J_CAP - 64:
            rounds += 1
            kept, fm = [], 64
            for lane in range(64):
                i = rawp + lane
                if i >= csize:
                    break
                b = raw[i]
                prev = raw[i - 1] if i > 0 else 0
                nxt = raw[i + 1] if i + 1 < csize else 1
                if self.mutate == "no-prev" and lane == 0:
                    prev = 0
                if self.mutate == "no-next" and lane == 63:
                    nxt = 1
                if prev == 0xFF and b != 0 and b != 0xFF:
                    fm = lane
                    break
                if b == 0 and prev == 0xFF:
                    continue  # stuffing
                if b == 0xFF and nxt != 0:
                    continue  # fill byte or marker prefix
                kept.append(b)
                if b == 0xFF:
                    cs["stuff:lane:%d" % lane] += 1
                    if lane == 63:
                        cs["stuff-split"] += 1
                    if prev == 0xFF:
                        cs["FF FF 00"] += 1
            have = min(64, csize - rawp)
            if fm < 64:
                cs["marker:lane:%d" % fm] += 1
                if fm == 0:
                    cs["prefix-split"] += 1
            elif have == 64 and raw[rawp + 63] == 0xFF and rawp + 64 < csize and raw[rawp + 64] != 0:
                cs["fill-run-crosses-round"] += 1
            if fm == 64 and not kept and have:
                cs["fill-round"] += 1
            self.buf[cend:cend + len(kept)] = bytes(kept)
            cend += len(kept)
            if fm < 64:
                pend = raw[rawp + fm]
                rawp += fm + 1
                end = "marker"
                if pend == 0xD9 and rawp < csize:
                    cs["eos:junk-after-EOI"] += 1
            elif rawp + 64 >= csize:
                if rawp + 64 == csize:
                    cs["eos:exact-round"] += 1
                if csize and raw[csize - 1] == 0xFF:
                    cs["eos:last-byte-FF"] += 1
                pend, rawp, end = 0x100, csize, "eos"
            else:
                rawp += 64
                end = "cap"
        cs["refill-end:" + end] += 1
        cs["rounds:%d" % rounds] += 1
        self.buf[cend:cend + J_PAD] = bytes(J_PAD)
        self.cend, self.rawp, self.pend, self.pos = cend, rawp, pend, 0 if self.mutate == "no-skip" else skip
        return byte0

    def peek(self, n):
        """The next n bits (zeros past the buffer's last dword, as jfill reads)."""
        v = 0
        for k in range(n):
            p = self.pos + k
            byte = self.buf[p >> 3] if (p >> 3) < J_CLEANSZ else 0
            v = v << 1 | (byte >> (7 - (p & 7)) & 1)
        return v

    def sym(self, h, key):
        e = h.lut[self.peek(9)]
        if e:
            l, s = e >> 8, e & 255
            self.cs["%s:len:%d:lut" % (key, l)] += 1
        else:
            l = 10
            while l <= 16 and self.peek(l) > h.maxcode[l]:
                l += 1
            if l > 16:
                self.cs["%s:walk-past-16" % key] += 1
                return 256
            s = h.val[(self.peek(l) + h.valoff[l]) & 255]
            self.cs["%s:len:%d:walk" % (key, l)] += 1
        self.pos += l
        return s

    def receive(self, n, key):
        v = self.peek(n)
        self.pos += n
        for p in _patterns(n, v):
            self.cs["%s:size:%d:%s" % (key, n, p)] += 1
        self.cs["%s:size:%d" % (key, n)] += 1
        return v - (1 << n) + 1 if v < 1 << (n - 1) else v


MUTATIONS = ("no-prev", "no-next", "no-skip", "c-offset")


def schedule(stream, tables=None, mutate=None):
    """(error code, census, [per block in scan order its 64 zigzag coefficients as decoded]) of
    k_tiff_jpeg_decode on the stream's entropy data.  mutate: one of MUTATIONS, a decoder that is
    wrong in one place -- a round's lane 0 does not see the byte before it, lane 63 not the byte
    after it, the moved remainder's bit offset is dropped, component 2 takes component 1's Huffman
    tables -- for the host test's proof that named cases would catch it."""
    T = J.new_tables()
    if tables is not None:
        J.read_tables(tables, T)
    J.read_tables(stream, T)
    H = J.header(stream)
    comps = H["comps"]
    ncomp = len(comps)
    hs, vs = (comps[0][1], comps[0][2]) if ncomp == 3 else (1, 1)
    mcux, mcuy = -(-H["width"] // (8 * hs)), -(-H["height"] // (8 * vs))
    nmcu, ri = mcux * mcuy, H["restart"]
    nluma = hs * vs
    bpm = nluma + 2 if ncomp == 3 else 1
    per = 64 // bpm
    huffs = [(_Huff(*T["h"][(0, td)]), _Huff(*T["h"][(1, ta)])) for td, ta in H["scan"]]
    cs = Counter()
    cs["per:%d" % per] += 1
    cs["tables:tq:" + ",".join(str(c[3]) for c in comps)] += 1
    cs["tables:td/ta:" + ",".join("%d/%d" % s for s in H["scan"])] += 1
    for rel, word in ((nmcu < per, "<"), (nmcu == per, "=="), (nmcu == per + 1, "==1+")):
        if rel:
            cs["batch:bpm%d:nmcu%sper" % (bpm, word)] += 1
    if nmcu % per == 1 and nmcu > per:
        cs["batch:bpm%d:last-of-one-mcu" % bpm] += 1
    if ri >= nmcu:
        cs["restart:bpm%d:interval-longer-than-the-stream" % bpm] += 1
    if mutate == "c-offset":
        huffs = [huffs[min(c, 1)] for c in range(ncomp)]
    s = _Wave(entropy(stream), cs, mutate)
    s.refill("first")
    pred, todo, rstn, bad, coefs = [0, 0, 0], ri, 0, 0, []
    fat_before = False
    all_eob = True
    m0 = 0
    while m0 < nmcu and not bad:
        m1 = min(m0 + per, nmcu)
        for m in range(m0, m1):
            if ri and todo == 0:
                if not s.pend:
                    s.refill("restart:no-marker-seen")
                if s.pend != 0xD0 + (rstn & 7) or (s.pos + 7) >> 3 != s.cend:
                    bad = 5
                    break
                cs["restart:bpm%d:%s" % (bpm, "on-batch-boundary" if m == m0 else "inside-batch")] += 1
                if ri == 1:
                    cs["restart:bpm%d:interval-1" % bpm] += 1
                rstn += 1
                if rstn > 8:
                    cs["rstn-wrap"] += 1
                    cs["rstn-wrap:bpm%d" % bpm] += 1
                todo, pred = ri, [0, 0, 0]
                s.pend = s.cend = s.pos = 0
                s.refill("restart")
                fat_before = False
            todo -= 1
            for b in range(bpm):
                c = 0 if b < nluma else b - nluma + 1
                refilled = False
                if not s.pend and s.cend * 8 < s.pos + J_LOW * 8:
                    s.refill("block")
                    refilled = True
                    cs["refill-at-block:bpm%d:%d" % (bpm, b)] += 1
                    if fat_before:
                        cs["refill:just-after-a-fat-block"] += 1
                start = s.pos
                blk = [0] * 64
                dct, act = huffs[c]
                sd = s.sym(dct, "code:dc")
                if sd > 11:
                    bad = 2 if sd == 256 else 4
                    break
                if sd:
                    pred[c] += s.receive(sd, "receive:dc")
                else:
                    cs["receive:dc:size:0"] += 1
                blk[0] = ((pred[c] + 0x8000) & 0xFFFF) - 0x8000
                k, zrls = 1, 0
                while k < 64:
                    rs = s.sym(act, "code:ac")
                    if rs == 256:
                        bad = 2
                        break
                    r, sz = rs >> 4, rs & 15
                    if not sz:
                        if r != 15:
                            break
                        if k + 15 == 63:
                            cs["zrl:lands-on-63"] += 1
                        k += 15
                        zrls += 1
                        if k > 63:
                            bad = 3
                            break
                        k += 1
                        continue
                    all_eob = False
                    k += r
                    if k > 63:
                        bad = 3
                        break
                    if sz > 10:
                        bad = 4
                        break
                    blk[k] = s.receive(sz, "receive:ac")
                    if k == 63:
                        cs["coef63:no-eob"] += 1
                        if zrls == 3 and not any(blk[1:63]):
                            cs["zrl:x3-then-63"] += 1
                    k += 1
                if bad:
                    break
                if blk[0] or sd:
                    all_eob = False
                if s.pos > s.cend * 8:
                    bad = 1
                    break
                nbits = s.pos - start
                cs["block-bits:max"] = max(cs["block-bits:max"], nbits)
                fat_before = nbits >= FAT - 64
                if nbits == FAT:
                    cs["fat:%d" % FAT] += 1
                    if refilled:
                        cs["refill:in-front-of-a-fat-block"] += 1
                coefs.append(blk)
            if bad:
                break
        m0 += per
    if not bad:
        if all_eob:
            cs["stream:all-eob"] += 1
        if s.pend == 0x100 or (not s.pend and s.rawp >= s.csize):
            cs["eos:no-EOI"] += 1
        elif not s.pend:
            cs["eos:end-not-seen"] += 1
        if cs["refill:moved"] >= 3:
            cs["refill:moved-chain-of-3"] += 1
    return bad, cs, coefs


def dequantised(stream, coefs, tables=None):
    """schedule()'s coefficients in decode_coefficients' form."""
    T = J.new_tables()
    if tables is not None:
        J.read_tables(tables, T)
    J.read_tables(stream, T)
    H = J.header(stream)
    comps = H["comps"]
    nc = len(comps)
    hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    mcux, mcuy = -(-H["width"] // (8 * hs)), -(-H["height"] // (8 * vs))
    out = [np.zeros((mcuy * v, mcux * h, 64), np.int64) for h, v in samp]
    it = iter(coefs)
    for m in range(mcux * mcuy):
        mx, my = m % mcux, m // mcux
        for c in range(nc):
            h, v = samp[c]
            qn = np.zeros(64, np.int64)
            qn[J.NAT] = T["q"][comps[c][3]]
            for b in range(h * v):
                blk = np.zeros(64, np.int64)
                blk[J.NAT] = next(it)
                out[c][my * v + b // h, mx * h + b % h] = blk * qn
    return out
