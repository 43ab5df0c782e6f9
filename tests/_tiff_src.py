"""Pure-Python / numpy restatement of what the TIFF loading tests need (TIFF 6.0): the section 13
LZW encoder (with knobs the edge-case tests turn) and decoder, the forward horizontal predictor
(section 14) and a minimal TIFF / BigTIFF writer for strips and tiles.  Independent of the
library under test; pinned by tests/test_tiff_src_host.py against libtiff (through PIL) and
against the tifffile-written fixtures of tests/golden/tiff/."""
import struct

import numpy as np

CLEAR, EOI, FIRST = 256, 257, 258
CLEAR_AFTER = 3836  # libtiff sends Clear as the 3,837th code of a run: the table holds 4,094 codes


def code_width(j):
    """Bits of code j of a run (j = 0: the code after a Clear), with the "early change"."""
    return 9 + (j >= 254) + (j >= 766) + (j >= 1790)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, w):
        self.acc = (self.acc << w) | v
        self.n += w
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 0xFF)
            self.n = 0
        return bytes(self.out)


def lzw_encode(data, clear_every=None, clear_at=(), eoi=True, leading_clear=True, codes_out=None):
    """TIFF LZW stream of `data`.  clear_every = N: a Clear after every N data codes;
    clear_at: a Clear after the data codes with these ordinals (1-based, counted over the whole
    stream); eoi / leading_clear = False leave those codes out.  codes_out (a list) receives
    every (code, width)."""
    data = bytes(data)
    bits, j, table, nxt = _Bits(), 0, {}, FIRST
    clear_at = set(clear_at)

    def emit(v):
        nonlocal j
        w = code_width(j)
        bits.put(v, w)
        if codes_out is not None:
            codes_out.append((v, w))
        j += 1

    def clear():
        nonlocal j, table, nxt
        emit(CLEAR)
        j, table, nxt = 0, {}, FIRST

    if leading_clear:
        clear()
    i, n, ndata, since = 0, len(data), 0, 0
    while i < n:
        code, k = data[i], i + 1
        while k < n and (code, data[k]) in table:
            code = table[(code, data[k])]
            k += 1
        emit(code)
        ndata += 1
        since += 1
        if k < n:
            table[(code, data[k])] = nxt
        nxt += 1  # (the decoder defines an entry for every code but the first of a run)
        i = k
        forced = (clear_every and since >= clear_every) or ndata in clear_at
        if i < n and (j == CLEAR_AFTER or forced):
            clear()
            since = 0
    if eoi:
        emit(EOI)
    return bits.done()


def lzw_pack(codes, leading_clear=True):
    """The stream of the raw code values `codes`, written as they are (after a Clear, unless
    leading_clear is False), each at the width of its place in its run (the early change); a
    Clear among them starts a new run.  No EOI is added."""
    bits, j = _Bits(), 0
    for v in ([CLEAR] if leading_clear else []) + list(codes):
        bits.put(v, code_width(j))
        j = 0 if v == CLEAR else j + 1
    return bits.done()


RUN_MAX = 3838  # codes of a run: the last one defines entry 4095


def lzw_decode(stream, expect=None, widths=None):
    """Table-based decoder (the textbook form, not the library's).  Stops at EOI, at the end of
    the input or once `expect` bytes are out.  widths (a list) receives every code's width.
    Raises ValueError for a code beyond the next free one, and for a code other than Clear or EOI
    after the RUN_MAX codes that fill the table."""
    stream = bytes(stream)
    out, table, nxt, nbits, old, run = bytearray(), {}, FIRST, 9, None, 0
    pos, total = 0, len(stream) * 8
    while pos + nbits <= total and (expect is None or len(out) < expect):
        q, r = pos >> 3, pos & 7
        v = int.from_bytes(stream[q:q + 4].ljust(4, b"\0"), "big")
        code = (v >> (32 - r - nbits)) & ((1 << nbits) - 1)
        pos += nbits
        if widths is not None:
            widths.append(nbits)
        if code == CLEAR:
            table, nxt, nbits, old, run = {}, FIRST, 9, None, 0
            continue
        if code == EOI:
            break
        if run >= RUN_MAX:
            raise ValueError("LZW: no Clear after the %d codes that fill the table" % RUN_MAX)
        run += 1
        if old is None:
            if code > 255:
                raise ValueError("LZW: code %d right after a Clear" % code)
            s = bytes([code])
        else:
            prev = table[old] if old >= FIRST else bytes([old])
            if code < 256:
                s = bytes([code])
            elif code < nxt:
                s = table[code]
            elif code == nxt:
                s = prev + prev[:1]
            else:
                raise ValueError("LZW: code %d above the next free code %d" % (code, nxt))
            table[nxt] = prev + s[:1]
            nxt += 1
            if nxt == (1 << nbits) - 1 and nbits < 12:  # early change
                nbits += 1
        out += s
        old = code
    return bytes(out if expect is None else out[:expect])


def predict2(a):
    """Forward Predictor = 2 of a (rows, width) integer array: every sample minus its left
    neighbour, modulo 2^bits.  Returns an array of the same dtype (byte order kept)."""
    a = np.ascontiguousarray(a)
    native = a.astype(a.dtype.newbyteorder("="))
    u = native.view(np.dtype("u%d" % native.dtype.itemsize))
    d = u.copy()
    d[:, 1:] = u[:, 1:] - u[:, :-1]
    return d.view(native.dtype).astype(a.dtype)


def segments_of(a, tile=None, rows_per_strip=None, predictor=1):
    """The uncompressed segment bytes of a (rows, width) array in its own byte order: tiles
    (tile = (tw, th), edge tiles zero-padded) or strips of rows_per_strip rows."""
    a = np.ascontiguousarray(a)
    h, w = a.shape
    segs = []
    if tile:
        tw, th = tile
        for y in range(0, h, th):
            for x in range(0, w, tw):
                t = np.zeros((th, tw), a.dtype)
                piece = a[y:y + th, x:x + tw]
                t[:piece.shape[0], :piece.shape[1]] = piece
                segs.append((predict2(t) if predictor == 2 else t).tobytes())
    else:
        rps = rows_per_strip or h
        for y in range(0, h, rps):
            s = a[y:y + rps]
            segs.append((predict2(s) if predictor == 2 else s).tobytes())
    return segs


def compress(seg, compression, **lzw_knobs):
    import zlib
    if compression == 1:
        return bytes(seg)
    if compression == 5:
        return lzw_encode(seg, **lzw_knobs)
    if compression in (8, 32946):
        return zlib.compress(bytes(seg), 6)
    raise ValueError(compression)


_SF = {"u": 1, "i": 2, "f": 3}


def page_of(a, compression=1, predictor=1, tile=None, rows_per_strip=None, description=None,
            subifds=(), extra=(), **lzw_knobs):
    """A page dict for write_tiff from a (rows, width) array (its dtype's byte order must be the
    file's)."""
    a = np.ascontiguousarray(a)
    segs = [compress(s, compression, **lzw_knobs) for s in segments_of(a, tile, rows_per_strip, predictor)]
    return dict(width=a.shape[1], length=a.shape[0], bits=a.dtype.itemsize * 8,
                sampleformat=_SF[a.dtype.kind], compression=compression, predictor=predictor,
                tile=tile, rows_per_strip=rows_per_strip or a.shape[0], segments=segs,
                description=description, subifds=list(subifds), extra=list(extra))


def write_tiff(path, pages, byteorder="<", bigtiff=False):
    """Classic TIFF or BigTIFF with one IFD per page (chained) and their SubIFDs (tag 330).
    extra: (tag, type, values) entries added as they are (type 3 SHORT, 4 LONG).  Returns the
    file's bytes (path = None: writes nothing)."""
    bo = byteorder
    buf = bytearray((b"II" if bo == "<" else b"MM"))
    buf += struct.pack(bo + "HHHQ", 43, 8, 0, 0) if bigtiff else struct.pack(bo + "HI", 42, 0)
    first_ptr = 8 if bigtiff else 4
    OFFT, OFFC = (16, "Q") if bigtiff else (4, "I")
    inline = 8 if bigtiff else 4
    fmts = {1: "B", 2: "c", 3: "H", 4: "I", 16: "Q", 13: "I", 18: "Q"}

    def align():
        if len(buf) & 1:
            buf.append(0)

    def put_ifd(page):
        subs = [put_ifd(sp)[0] for sp in page.get("subifds", ())]
        offs = []
        for s in page["segments"]:
            align()
            offs.append(len(buf))
            buf.extend(s)
        counts = [len(s) for s in page["segments"]]
        tags = [(256, 4, [page["width"]]), (257, 4, [page["length"]]), (258, 3, [page["bits"]]),
                (259, 3, [page["compression"]]), (262, 3, [1]), (277, 3, [page.get("spp", 1)]),
                (339, 3, [page["sampleformat"]])]
        if page.get("description") is not None:
            d = page["description"].encode() + b"\0"
            tags.append((270, 2, d))
        if page.get("predictor", 1) != 1:
            tags.append((317, 3, [page["predictor"]]))
        if page.get("tile"):
            tags += [(322, 4, [page["tile"][0]]), (323, 4, [page["tile"][1]]),
                     (324, OFFT, offs), (325, OFFT, counts)]
        else:
            tags += [(278, 4, [page["rows_per_strip"]]), (273, OFFT, offs), (279, OFFT, counts)]
        if subs:
            tags.append((330, 18 if bigtiff else 13, subs))
        tags += [tuple(t) for t in page.get("extra", ())]
        tags.sort(key=lambda t: t[0])
        entries = []
        for tag, typ, vals in tags:
            raw = bytes(vals) if typ == 2 else struct.pack(bo + fmts[typ] * len(vals), *vals)
            n = len(vals)
            if len(raw) <= inline:
                field = raw.ljust(inline, b"\0")
            else:
                align()
                field = struct.pack(bo + OFFC, len(buf))
                buf.extend(raw)
            entries.append(struct.pack(bo + ("HHQ" if bigtiff else "HHI"), tag, typ, n) + field)
        align()
        at = len(buf)
        buf.extend(struct.pack(bo + ("Q" if bigtiff else "H"), len(entries)))
        for e in entries:
            buf.extend(e)
        nxt = len(buf)
        buf.extend(struct.pack(bo + OFFC, 0))
        return at, nxt

    ptr = first_ptr
    for page in pages:
        at, nxt = put_ifd(page)
        struct.pack_into(bo + OFFC, buf, ptr, at)
        ptr = nxt
    if path is not None:
        with open(path, "wb") as f:
            f.write(buf)
    return bytes(buf)
