"""Test-side model of JPEG-compressed TIFF segments (Compression 7): a numpy restatement of the
decoder the GPU runs (markers, Huffman, the "islow" integer IDCT, fancy upsampling, YCbCr -> RGB,
all as the libjpeg 6b lineage does them), a small baseline encoder for streams PIL's never writes,
and a TIFF container writer around JPEG segments.  The model is checked against PIL (libjpeg-turbo)
byte for byte in tests/test_tiff_jpeg_host.py; the GPU is checked against the model."""
import io
import json
import os
import struct

import numpy as np

import _tiff_rgb as R

# NAT[k]: the natural (row-major) position of zigzag index k
NAT = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
       21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
       61, 54, 47, 55, 62, 63]


class JpegError(ValueError):
    """A stream the decoder refuses: code = the kernel's err[] code (0 for a header refusal)."""

    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


# ------------------------------------------------------------------------------ markers
def segments(data):
    """[(code, payload offset, payload length)] of the marker segments up to and including SOS (or
    EOI for a tables-only stream), fill bytes skipped."""
    assert data[:2] == b"\xff\xd8", "no SOI"
    out, q = [], 2
    while True:
        assert data[q] == 0xFF
        while data[q] == 0xFF:
            q += 1
        code = data[q]
        q += 1
        if code == 0xD9:
            out.append((code, q, 0))
            return out
        L = data[q] << 8 | data[q + 1]
        out.append((code, q + 2, L - 2))
        q += L
        if code == 0xDA:
            return out


def new_tables():
    return dict(q={}, h={})


def read_tables(data, T):
    """The DQT / DHT segments of a stream into T: q[tq] = 64 values in zigzag order, h[(tc, th)] =
    (bits[1..16], vals)."""
    for code, o, n in segments(data):
        p = data[o:o + n]
        if code == 0xDB:
            k = 0
            while k < n:
                assert p[k] >> 4 == 0
                T["q"][p[k] & 15] = np.frombuffer(p[k + 1:k + 65], np.uint8).astype(np.int64)
                k += 65
        elif code == 0xC4:
            k = 0
            while k < n:
                bits = list(p[k + 1:k + 17])
                T["h"][(p[k] >> 4, p[k] & 15)] = (bits, list(p[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
    return T


def header(data):
    """SOF0 / DRI / SOS of a stream: width, height, comps = [(id, h, v, tq)], scan = [(td, ta)],
    restart, data = offset of the entropy-coded bytes."""
    H = dict(restart=0)
    for code, o, n in segments(data):
        p = data[o:o + n]
        if code == 0xC0:
            assert p[0] == 8
            H.update(height=p[1] << 8 | p[2], width=p[3] << 8 | p[4],
                     comps=[(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(p[5])])
        elif code == 0xDD:
            H["restart"] = p[0] << 8 | p[1]
        elif code == 0xDA:
            assert p[0] == len(H["comps"])
            H["scan"] = [(p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(p[0])]
            H["data"] = o + n
    return H


def clean_intervals(ent):
    """The entropy-coded bytes as the decoder sees them: [(clean bytes, marker code that ended
    them or None at the end of the data)]: stuffing zeros and fill bytes removed."""
    out, cur, i, n = [], bytearray(), 0, len(ent)
    while i < n:
        b = ent[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        j = i
        while j < n and ent[j] == 0xFF:
            j += 1
        if j >= n:
            break
        if ent[j] == 0:
            cur.append(0xFF)
            i = j + 1
            continue
        out.append((bytes(cur), ent[j]))
        cur = bytearray()
        i = j + 1
        if not 0xD0 <= ent[j] <= 0xD7:
            return out
    out.append((bytes(cur), None))
    return out


# ------------------------------------------------------------------------------ entropy decoding
def code_table(bits, vals):
    """{(length, code): symbol} of a canonical code."""
    out, code, p = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[(l, code)] = vals[p]
            p += 1
            code += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self, data):
        self.s = "".join("{:08b}".format(b) for b in data)
        self.pos = 0

    def sym(self, table):
        for l in range(1, 17):
            v = table.get((l, int(self.s[self.pos:self.pos + l].ljust(l, "0"), 2)))
            if v is not None:
                self.pos += l
                return v
        raise JpegError("a code that is in no table", 2)

    def receive(self, n):
        v = int(self.s[self.pos:self.pos + n].ljust(n, "0"), 2)
        self.pos += n
        return v if v >= 1 << (n - 1) else v - (1 << n) + 1


def decode_coefficients(data, tables=None):
    """(header, [per component: int64 array (block rows, block cols, 64) of dequantised
    coefficients, natural order, over the MCU-padded grid])."""
    T = new_tables()
    if tables is not None:
        read_tables(tables, T)
    read_tables(data, T)
    H = header(data)
    comps = H["comps"]
    nc = len(comps)
    hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    mcux = -(-H["width"] // (8 * hs))
    mcuy = -(-H["height"] // (8 * vs))
    out = [np.zeros((mcuy * v, mcux * h, 64), np.int64) for h, v in samp]
    dct = [code_table(*T["h"][(0, td)]) for td, _ in H["scan"]]
    act = [code_table(*T["h"][(1, ta)]) for _, ta in H["scan"]]
    qn = []
    for c in comps:
        q = np.zeros(64, np.int64)
        q[NAT] = T["q"][c[3]]
        qn.append(q)
    ivals = clean_intervals(data[H["data"]:])
    ri = H["restart"]
    nmcu = mcux * mcuy
    m, k_iv = 0, 0
    while m < nmcu:
        if k_iv >= len(ivals):
            raise JpegError("entropy data ends before the last MCU", 1)
        clean, marker = ivals[k_iv]
        br = _Bits(clean)
        pred = [0] * nc
        last = min(nmcu, m + ri) if ri else nmcu
        while m < last:
            mx, my = m % mcux, m // mcux
            for c in range(nc):
                h, v = samp[c]
                for b in range(h * v):
                    blk = np.zeros(64, np.int64)
                    s = br.sym(dct[c])
                    if s > 11:
                        raise JpegError("DC size %d" % s, 4)
                    if s:
                        pred[c] += br.receive(s)
                    blk[0] = ((pred[c] + 0x8000) & 0xFFFF) - 0x8000  # stored as int16, as libjpeg's JCOEF
                    k = 1
                    while k < 64:
                        rs = br.sym(act[c])
                        r, sz = rs >> 4, rs & 15
                        if sz == 0:
                            if r != 15:
                                break
                            k += 16
                            if k > 64:
                                raise JpegError("a run that passes coefficient 63", 3)
                            continue
                        k += r
                        if k > 63:
                            raise JpegError("a run that passes coefficient 63", 3)
                        if sz > 10:
                            raise JpegError("AC size %d" % sz, 4)
                        blk[NAT[k]] = br.receive(sz)
                        k += 1
                    if br.pos > 8 * len(clean):
                        raise JpegError("entropy data ends before the last MCU", 1)
                    out[c][my * v + b // h, mx * h + b % h] = blk * qn[c]
            m += 1
        if m < nmcu:  # a restart marker stands here, the next in sequence
            if marker != 0xD0 + (k_iv & 7) or (br.pos + 7) // 8 != len(clean):
                raise JpegError("restart marker missing, out of sequence or misplaced", 5)
        k_iv += 1
    return H, out


# ------------------------------------------------------------------------------ IDCT
def _idct1(i):
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (i[0] + i[4]) << 13
    tmp1 = (i[0] - i[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
            tmp10 - tmp3]


def idct_islow(coefs, exempt=None):
    """jidctint.c on an int64 array (..., 64) of dequantised coefficients: uint8 samples (..., 8,
    8).  Asserts the condition under which libjpeg's builds agree: every sample lies in [-512, 511]
    before the level shift and the clamp.  exempt: None, or a bool array coefs.shape[:-1] of blocks
    the assertion leaves out (blocks no sample of which is ever placed: _tiff_jpeg_frames.py)."""
    b = coefs.reshape(coefs.shape[:-1] + (8, 8))
    cols = _idct1([b[..., r, :] for r in range(8)])
    ws = np.stack([(x + (1 << 10)) >> 11 for x in cols], axis=-2)
    rows = _idct1([ws[..., :, c] for c in range(8)])
    out = np.stack([(x + (1 << 17)) >> 18 for x in rows], axis=-1)
    held = out if exempt is None else out[~np.asarray(exempt, bool)]
    assert held.size == 0 or (held.min() >= -512 and held.max() <= 511), \
        "IDCT output %d .. %d leaves [-512, 511]" % (held.min(), held.max())
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def component_planes(data, tables=None, exempt=None):
    """(header, [uint8 plane per component at its own resolution, padded to whole MCUs]).  exempt:
    None, or per component a bool array (block rows, block cols) for idct_islow."""
    H, coefs = decode_coefficients(data, tables)
    planes = []
    for k, c in enumerate(coefs):
        px = idct_islow(c, None if exempt is None else exempt[k])  # (by, bx, 8, 8)
        planes.append(px.transpose(0, 2, 1, 3).reshape(c.shape[0] * 8, c.shape[1] * 8))
    return H, planes


# ------------------------------------------------------------------------------ upsampling, colour
def upsample(c, hs, vs, w, h):
    """jdsample.c: chroma plane c (MCU-padded) to w x h.  Edges are the component's own
    downsampled size; a plane at most two samples wide is replicated (libjpeg's fancy upsamplers
    need downsampled_width > 2)."""
    if hs == 1 and vs == 1:
        return c[:h, :w].astype(np.int64)
    cw, ch = -(-w // 2), (-(-h // 2) if vs == 2 else h)
    c = c[:ch, :cw].astype(np.int64)
    if cw <= 2:
        return np.repeat(np.repeat(c, vs, axis=0), 2, axis=1)[:h, :w]
    if vs == 1:
        prev = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
        nxt = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        even, odd = (3 * c + prev + 1) >> 2, (3 * c + nxt + 2) >> 2
        even[:, 0], odd[:, -1] = c[:, 0], c[:, -1]
    else:
        up = np.concatenate([c[:1], c[:-1]], axis=0)
        dn = np.concatenate([c[1:], c[-1:]], axis=0)
        s = np.empty((2 * ch, cw), np.int64)
        s[0::2], s[1::2] = 3 * c + up, 3 * c + dn
        prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        nxt = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        even, odd = (3 * s + prev + 8) >> 4, (3 * s + nxt + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
    out = np.empty((even.shape[0], 2 * cw), np.int64)
    out[:, 0::2], out[:, 1::2] = even, odd
    return out[:h, :w]


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c's 16-bit fixed-point tables."""
    y, u, v = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * v + 32768) >> 16)
    g = y + ((-22554 * u - 46802 * v + 32768) >> 16)
    b = y + ((116130 * u + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data, tables=None, ycbcr=True, exempt=None):
    """A segment as the GPU stores it: (h, w) for one component, else (h, w, 3): converted to RGB
    with `ycbcr` (PhotometricInterpretation 6), else the components as they are."""
    H, planes = component_planes(data, tables, exempt)
    w, h = H["width"], H["height"]
    if len(planes) == 1:
        return planes[0][:h, :w]
    hs, vs = H["comps"][0][1], H["comps"][0][2]
    y = planes[0][:h, :w]
    if not ycbcr:
        assert (hs, vs) == (1, 1)
        return np.stack([p[:h, :w] for p in planes], axis=-1)
    return ycc_to_rgb(y, upsample(planes[1], hs, vs, w, h), upsample(planes[2], hs, vs, w, h))


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


# ------------------------------------------------------------------------------ PIL-made streams
def pil_jpeg(a, quality=75, subsampling=0, keep_rgb=False, restart_blocks=0, restart_rows=0):
    """A baseline JPEG stream from PIL's encoder (standard Huffman tables): a (h, w) array as a
    one-component stream, a (h, w, 3) one as YCbCr with `subsampling` (0 4:4:4, 1 4:2:2, 2 4:2:0),
    or with keep_rgb as three unconverted 1x1 components."""
    from PIL import Image
    kw = dict(quality=quality)
    if a.ndim == 3:
        kw.update(subsampling=0 if keep_rgb else subsampling, keep_rgb=keep_rgb)
    if restart_blocks:
        kw["restart_marker_blocks"] = restart_blocks
    if restart_rows:
        kw["restart_marker_rows"] = restart_rows
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def split_tables(data):
    """(tables-only stream for tag 347, abbreviated stream without DQT / DHT) of a whole stream."""
    tabs, rest, last = bytearray(b"\xff\xd8"), bytearray(b"\xff\xd8"), 0
    for code, o, n in segments(data):
        raw = bytes([0xFF, code]) + data[o - 2:o + n]
        (tabs if code in (0xDB, 0xC4) else rest).extend(raw)
        last = o + n
    return bytes(tabs) + b"\xff\xd9", bytes(rest) + data[last:]


def _pieces(a, tile, rows_per_strip):
    h, w = a.shape[:2]
    if tile:
        tw, th = tile
        pad = [(0, -h % th), (0, -w % tw)] + [(0, 0)] * (a.ndim - 2)
        p = np.pad(a, pad, mode="edge")
        return [p[y:y + th, x:x + tw] for y in range(0, h, th) for x in range(0, w, tw)]
    rps = rows_per_strip or h
    return [a[y:y + rps] for y in range(0, h, rps)]


def page_of(a, tile=None, rows_per_strip=None, photometric=None, tables="tag", planar=1, encode=None,
            description=None, subifds=(), extra=(), **jpeg_kw):
    """A page dict for write_tiff from a (h, w) or (h, w, 3) uint8 array, every strip or tile a
    JPEG stream of its own (pil_jpeg(**jpeg_kw), or encode(piece) -> stream).  photometric: 6
    (YCbCr, the default for three samples), 2 (RGB kept as it is) or 1.  tables: "tag" (tag 347
    holds them, the segments are abbreviated), "segment" (no tag 347), "both" (tag 347 holds
    OTHER tables -- those of a quality-10 stream -- and every segment its own, which override)."""
    a = np.ascontiguousarray(a)
    s = 1 if a.ndim == 2 else a.shape[2]
    if photometric is None:
        photometric = 6 if s == 3 else 1
    if encode is None:
        def encode(x):
            return pil_jpeg(np.ascontiguousarray(x), keep_rgb=(photometric == 2 and x.ndim == 3), **jpeg_kw)
    if planar == 2:
        streams = [encode(p) for c in range(s) for p in _pieces(a[:, :, c], tile, rows_per_strip)]
    else:
        streams = [encode(p) for p in _pieces(a, tile, rows_per_strip)]
    extra = list(extra)
    if tables == "tag":
        tabs = split_tables(streams[0])[0]
        assert all(split_tables(x)[0] == tabs for x in streams)
        streams = [split_tables(x)[1] for x in streams]
        extra.append((347, 1, list(tabs)))
    elif tables == "both":
        other = pil_jpeg(np.zeros((8, 8) + a.shape[2:], np.uint8), quality=10,
                         **({"keep_rgb": photometric == 2} if s == 3 else {}))
        extra.append((347, 1, list(split_tables(other)[0])))
    if photometric == 6:
        sub = header(streams[0])["comps"][0]
        extra.append((530, 3, [sub[1], sub[2]]))
    h, w = a.shape[:2]
    return dict(width=w, length=h, bits=8, sampleformat=1, spp=s, compression=7, predictor=1, tile=tile,
                rows_per_strip=rows_per_strip or h, segments=streams, planar=planar, photometric=photometric,
                extrasamples=[], description=description, subifds=[R._finish(p) for p in subifds], extra=extra)


def write_tiff(path, pages, byteorder="<", bigtiff=False):
    return R.write_tiff(path, pages, byteorder, bigtiff)


def decode_page(page, jpeg_tables=None):
    """The model's planes of a page_of() page: (h, w) or (h, w, S)."""
    h, w, s = page["length"], page["width"], page["spp"]
    tabs = jpeg_tables
    for t in page["extra"]:
        if t[0] == 347:
            tabs = bytes(t[2])
    out = np.zeros((h, w, s), np.uint8)
    tile, rps = page["tile"], page["rows_per_strip"]
    grid = [(x, y) for y in range(0, h, tile[1]) for x in range(0, w, tile[0])] if tile else \
        [(0, y) for y in range(0, h, rps)]
    groups = s if page["planar"] == 2 and s > 1 else 1
    for g in range(groups):
        for (x, y), seg in zip(grid, page["segments"][g * len(grid):(g + 1) * len(grid)]):
            d = decode(seg, tabs, ycbcr=page["photometric"] == 6)
            d = d.reshape(d.shape[0], d.shape[1], -1)[:h - y, :w - x]
            if groups > 1:
                out[y:y + d.shape[0], x:x + d.shape[1], g] = d[:, :, 0]
            else:
                out[y:y + d.shape[0], x:x + d.shape[1]] = d
    return out[:, :, 0] if s == 1 else out


# ------------------------------------------------------------------------------ test-only encoder
def std_tables():
    """The standard (T.81 Annex K) tables as PIL's encoder writes them at quality 75."""
    return read_tables(pil_jpeg(np.zeros((8, 8, 3), np.uint8)), new_tables())


def long_code_table(symbols):
    """A canonical code over `symbols` whose first 14 have lengths 2 .. 15 and the rest 16 bits:
    codes up to 16 bits long, and (the code is incomplete) codes that are in no table."""
    symbols = list(symbols)
    bits = [0] * 16
    for l in range(2, 16):
        if l - 2 < len(symbols):
            bits[l - 1] = 1
    bits[15] = max(0, len(symbols) - 14)
    return bits, symbols


def _fdct(block):
    k = np.arange(8)
    C = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), 0.5)
    return C @ block @ C.T


def quantised_blocks(plane, q_zigzag):
    """(block rows, block cols, 64) int coefficients in zigzag order of a uint8 plane whose sides
    are multiples of 8: float FDCT of the level-shifted samples, divided and rounded."""
    h, w = plane.shape
    q = np.zeros(64)
    q[NAT] = q_zigzag
    out = np.zeros((h // 8, w // 8, 64), np.int64)
    for by in range(h // 8):
        for bx in range(w // 8):
            d = _fdct(plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].astype(np.float64) - 128).reshape(64)
            out[by, bx] = np.rint(d / q).astype(np.int64)[NAT]
    return out


class _Writer:
    def __init__(self):
        self.bits = []

    def put(self, code, n):
        self.bits.append("{:0{n}b}".format(code, n=n) if n else "")

    def flush(self):
        s = "".join(self.bits)
        s += "1" * (-len(s) % 8)
        self.bits = []
        out = bytearray()
        for i in range(0, len(s), 8):
            b = int(s[i:i + 8], 2)
            out.append(b)
            if b == 0xFF:
                out.append(0)
        return bytes(out)


def _enc_table(bits, vals):
    return {v: (l, c) for (l, c), v in code_table(bits, vals).items()}


def _category(v):
    return 0 if v == 0 else int(abs(int(v))).bit_length()


def encode_stream(width, height, blocks, sampling=(1, 1), q=None, huff=None, restart=0, tables_in_stream=True,
                  comp_ids=(1, 2, 3), keep_eob=True):
    """A baseline stream from quantised coefficients: blocks = per component an int array (block
    rows, block cols, 64) in zigzag order over the MCU-padded grid.  q = {tq: 64 zigzag values},
    component c using table min(c, 1); huff = {(tc, th): (bits, vals)}, component c using tables
    min(c, 1).  An End-of-Block code is written only where coefficient 63 is zero."""
    T = std_tables()
    q = q if q is not None else T["q"]
    huff = huff if huff is not None else T["h"]
    nc = len(blocks)
    hs, vs = sampling if nc == 3 else (1, 1)
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    out = bytearray(b"\xff\xd8")
    if tables_in_stream:
        for tq in sorted(q):
            out += b"\xff\xdb" + struct.pack(">HB", 67, tq) + bytes(int(x) for x in q[tq])
        for (tc, th), (bits, vals) in sorted(huff.items()):
            out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc << 4 | th) + bytes(bits) + bytes(vals)
    out += b"\xff\xc0" + struct.pack(">HBHHB", 8 + 3 * nc, 8, height, width, nc)
    for c in range(nc):
        out += bytes([comp_ids[c], samp[c][0] << 4 | samp[c][1], min(c, 1)])
    if restart:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart)
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * nc, nc)
    for c in range(nc):
        out += bytes([comp_ids[c], min(c, 1) << 4 | min(c, 1)])
    out += bytes([0, 63, 0])
    enc = {k: _enc_table(*v) for k, v in huff.items()}
    mcuy, mcux = blocks[0].shape[0] // vs, blocks[0].shape[1] // hs
    wr, pred, n = _Writer(), [0] * nc, 0
    for m in range(mcux * mcuy):
        if restart and m and m % restart == 0:
            out += wr.flush() + bytes([0xFF, 0xD0 + (n & 7)])
            n += 1
            pred = [0] * nc
        mx, my = m % mcux, m // mcux
        for c in range(nc):
            h, v = samp[c]
            dc, ac = enc[(0, min(c, 1))], enc[(1, min(c, 1))]
            for b in range(h * v):
                blk = blocks[c][my * v + b // h, mx * h + b % h]
                d = int(blk[0]) - pred[c]
                pred[c] = int(blk[0])
                s = _category(d)
                wr.put(dc[s][1], dc[s][0])
                if s:
                    wr.put(d if d > 0 else d + (1 << s) - 1, s)
                run = 0
                for k in range(1, 64):
                    x = int(blk[k])
                    if x == 0:
                        run += 1
                        continue
                    while run > 15:
                        wr.put(ac[0xF0][1], ac[0xF0][0])
                        run -= 16
                    s = _category(x)
                    wr.put(ac[run << 4 | s][1], ac[run << 4 | s][0])
                    wr.put(x if x > 0 else x + (1 << s) - 1, s)
                    run = 0
                if run and keep_eob:
                    wr.put(ac[0][1], ac[0][0])
    return bytes(out) + wr.flush() + b"\xff\xd9"


def encode_planes(planes, width, height, sampling=(1, 1), q=None, **kw):
    """encode_stream from uint8 component planes already at their own resolution, padded to whole
    MCUs."""
    T = std_tables()
    q = q if q is not None else T["q"]
    blocks = [quantised_blocks(p, q[min(c, 1)]) for c, p in enumerate(planes)]
    return encode_stream(width, height, blocks, sampling, q=q, **kw)


# ------------------------------------------------------------------------------ shared by the tests
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_jpeg")
_NPY = {}


def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)["files"]


def expected(entry, level, key):
    """The (rows, width) plane the manifest names (PIL's decode of the fixture)."""
    npy, idx = entry["planes"][str(level)][key]
    if npy not in _NPY:
        _NPY[npy] = np.load(os.path.join(GOLD, npy))
    a = _NPY[npy]
    if len(idx) == 2:
        return np.ascontiguousarray(a[idx[0], :, :, idx[1]])
    if len(idx) == 1:
        return np.ascontiguousarray(a[:, :, idx[0]] if a.ndim == 3 else a[idx[0]])
    return a


def noise(w, h, seed, s=3):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, s), dtype=np.uint8)
    return a if s > 1 else a[:, :, 0].copy()


def ramp(w, h, s=3):
    a = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[..., None] + np.array([0, 70, 140])[:s]) % 256
    return np.ascontiguousarray(a.astype(np.uint8) if s > 1 else a[:, :, 0].astype(np.uint8))


def checker(w, h, s=3):
    a = (((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255)[..., None] * np.ones(s, int)).astype(np.uint8)
    return np.ascontiguousarray(a if s > 1 else a[:, :, 0])


KINDS = {"gray": dict(s=1), "444": dict(subsampling=0), "422": dict(subsampling=1), "420": dict(subsampling=2),
         "rgb": dict(photometric=2)}


def kind_page(kind, a, **kw):
    """page_of() for one of KINDS from a (h, w, 3) array (gray: its first sample)."""
    o = dict(KINDS[kind])
    o.pop("s", None)
    o.update(kw)
    return page_of(a if kind != "gray" or a.ndim == 2 else np.ascontiguousarray(a[:, :, 0]), **o)


def stream_page(w, h, stream, photometric=None, spp=None):
    """A one-strip page around one stream (spp: for streams whose header the model cannot read)."""
    nc = spp or len(header(stream)["comps"])
    return dict(width=w, length=h, bits=8, sampleformat=1, spp=nc, compression=7, predictor=1, tile=None, rows_per_strip=h,
                segments=[stream], planar=1, photometric=photometric or (6 if nc == 3 else 1), extrasamples=[],
                description=None, subifds=[], extra=[])


def generated_streams():
    """Streams PIL's encoder never writes (this module's encoder), as (name, w, h, stream)."""
    T = std_tables()
    out = []
    w, h = 24, 16
    smooth = ramp(w, h, 1)
    for name, qv in (("q1", 1), ("q64", 64)):
        q = {0: np.full(64, qv, np.int64), 1: np.full(64, qv, np.int64)}
        out.append((name, w, h, encode_planes([smooth], w, h, q=q)))
    # DC differences of size 11: blocks alternating black and white under a quantiser of ones
    bw = np.zeros((16, 32), np.uint8)
    bw[:, 8:16] = bw[:, 24:32] = 255
    out.append(("dc11", 32, 16, encode_planes([bw], 32, 16, q={0: np.ones(64, np.int64), 1: np.ones(64, np.int64)})))
    # coefficient 63 non-zero (no End-of-Block), runs over 16 zeros (ZRL), three components 4:2:0
    rng = np.random.default_rng(5)
    blocks = []
    for shape in ((2, 4), (1, 2), (1, 2)):
        b = np.zeros(shape + (64,), np.int64)
        b[..., 0] = rng.integers(-20, 20, shape)
        b[..., 63] = rng.integers(1, 3, shape)
        b[..., 20] = rng.integers(-2, 3, shape)
        b[0, 0, 40] = -1
        blocks.append(b)
    out.append(("coef63_zrl_420", 32, 16, encode_stream(32, 16, blocks, sampling=(2, 2))))
    # codes of 16 bits: incomplete canonical codes whose rarest symbols are 16 bits long
    huff = {(0, 0): long_code_table([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11][::-1]),
            (1, 0): long_code_table(sorted(T["h"][(1, 0)][1], reverse=True))}
    huff[(0, 1)], huff[(1, 1)] = huff[(0, 0)], huff[(1, 0)]
    out.append(("codes16", w, h, encode_planes([noise(w, h, 3, 1) // 4 + 96], w, h, huff=huff)))
    # forced FF 00, with a restart interval: the first noise plane whose stream holds stuffed bytes
    for seed in range(64):
        s = encode_planes([noise(w, h, seed, 1)], w, h, restart=2)
        if s[header(s)["data"]:].count(b"\xff\x00") >= 2:
            break
    assert s[header(s)["data"]:].count(b"\xff\x00") >= 2
    out.append(("ff00_restart2", w, h, s))
    return out


def rename_symbol(stream, tc, th, old, new):
    """The stream with symbol `old` of its Huffman table (tc, th) declared as `new`."""
    b = bytearray(stream)
    for code, o, n in segments(stream):
        k = o
        while code == 0xC4 and k < o + n:
            cnt = sum(b[k + 1:k + 17])
            if (b[k] >> 4, b[k] & 15) == (tc, th):
                at = bytes(b[k + 17:k + 17 + cnt]).index(bytes([old]))
                b[k + 17 + at] = new
                return bytes(b)
            k += 17 + cnt
    raise AssertionError("no table %d/%d" % (tc, th))


def bad_streams():
    """(name, w, h, stream, decoder code): streams the device must refuse, one code each of 1 .. 5."""
    T = std_tables()
    a = noise(24, 16, 31)
    good = pil_jpeg(a, quality=85, subsampling=2)
    d = header(good)["data"]
    out = [("cut at %d" % cut, 24, 16, good[:d + cut], 1) for cut in (0, 1, 7, (len(good) - d) // 2, len(good) - d - 3)]
    out.append(("unassigned code", 24, 16, good[:d] + b"\xff\x00" * 16 + b"\xff\xd9", 2))
    # DC difference 0, then four ZRL codes: the fourth passes coefficient 63
    enc, dc = _enc_table(*T["h"][(1, 0)]), _enc_table(*T["h"][(0, 0)])
    wr = _Writer()
    wr.put(dc[0][1], dc[0][0])
    for _ in range(4):
        wr.put(enc[0xF0][1], enc[0xF0][0])
    gray = pil_jpeg(a[:, :, 0].copy(), quality=85)
    out.append(("run past 63", 24, 16, gray[:header(gray)["data"]] + wr.flush() + b"\x00" * 8 + b"\xff\xd9", 3))
    # a DC table whose symbols run to 12, an AC table that holds 0x0B (run 0, size 11): the noise
    # stream meets size-4 DC differences and (0, 1) coefficients at once
    gray = pil_jpeg(noise(24, 16, 33, 1), quality=85)
    out.append(("DC size 12", 24, 16, rename_symbol(gray, 0, 0, 4, 12), 4))
    out.append(("AC size 11", 24, 16, rename_symbol(gray, 1, 0, 0x01, 0x0B), 4))
    rst = pil_jpeg(a, quality=85, subsampling=0, restart_blocks=1)
    assert b"\xff\xd1" in rst
    out.append(("wrong RSTn", 24, 16, rst.replace(b"\xff\xd1", b"\xff\xd2", 1), 5))
    out.append(("missing RSTn", 24, 16, rst.replace(b"\xff\xd1", b"", 1), 5))
    return out
