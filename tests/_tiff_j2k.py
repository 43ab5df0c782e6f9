"""Test helper: a pure-Python / numpy model of the lossless JPEG 2000 decoder behind the TIFF source
path (Compression 33003 / 33004 / 33005 / 34712; DESIGN.md section 10b "JPEG 2000 segments"), and
a writer of the TIFF pages around PIL's codestreams.

The model follows ITU-T T.800: the main header (SIZ, COD, QCD), the packet headers (B.10: tag
trees, the number-of-passes codeword, Lblock), the MQ decoder (Annex C), the three coding passes
(Annex D), the inverse 5/3 lifting (F.3) and the inverse reversible colour transform (G.2).  It is
slow and meant for images of a few hundred pixels.  The reversible path has a right answer that no
library's arithmetic enters: the encoder's input, bit for bit."""
import hashlib
import io
import json
import os
import struct

import numpy as np

J2K_COMPRESSIONS = (33003, 33004, 33005, 34712)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_j2k")


def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)["files"]


def expected(entry, level, key):
    """The (h, w) array of plane `key` ("z,c,t") of stored level `level`: the pixels the file was
    encoded from, checked against the manifest's hash of their big-endian bytes."""
    npy, index, digest = entry["planes"][str(level)][key]
    a = np.load(os.path.join(GOLD, npy))
    index = list(index)  # [page] if the file has several, then [sample] if its pixels have several
    c = index.pop() if entry["samples"] > 1 else None
    if index:
        a = a[index[0]]
    a = np.ascontiguousarray(a if c is None else a[:, :, c])
    assert hashlib.sha256(a.astype(a.dtype.newbyteorder(">")).tobytes()).hexdigest() == digest, (entry["file"], key)
    return a


def be_bytes(a):
    """What read_plane_be and a raw tile hold: big-endian samples."""
    return a.astype(a.dtype.newbyteorder(">")).tobytes()


# T.800 table C.2: Qe, NMPS, NLPS, SWITCH
MQ = [(0x5601, 1, 1, 1), (0x3401, 2, 6, 0), (0x1801, 3, 9, 0), (0x0AC1, 4, 12, 0), (0x0521, 5, 29, 0),
      (0x0221, 38, 33, 0), (0x5601, 7, 6, 1), (0x5401, 8, 14, 0), (0x4801, 9, 14, 0), (0x3801, 10, 14, 0),
      (0x3001, 11, 17, 0), (0x2401, 12, 18, 0), (0x1C01, 13, 20, 0), (0x1601, 29, 21, 0), (0x5601, 15, 14, 1),
      (0x5401, 16, 14, 0), (0x5101, 17, 15, 0), (0x4801, 18, 16, 0), (0x3801, 19, 17, 0), (0x3401, 20, 18, 0),
      (0x3001, 21, 19, 0), (0x2801, 22, 19, 0), (0x2401, 23, 20, 0), (0x2201, 24, 21, 0), (0x1C01, 25, 22, 0),
      (0x1801, 26, 23, 0), (0x1601, 27, 24, 0), (0x1401, 28, 25, 0), (0x1201, 29, 26, 0), (0x1101, 30, 27, 0),
      (0x0AC1, 31, 28, 0), (0x09C1, 32, 29, 0), (0x08A1, 33, 30, 0), (0x0521, 34, 31, 0), (0x0441, 35, 32, 0),
      (0x02A1, 36, 33, 0), (0x0221, 37, 34, 0), (0x0141, 38, 35, 0), (0x0111, 39, 36, 0), (0x0085, 40, 37, 0),
      (0x0049, 41, 38, 0), (0x0025, 42, 39, 0), (0x0015, 43, 40, 0), (0x0009, 44, 41, 0), (0x0005, 45, 42, 0),
      (0x0001, 45, 43, 0), (0x5601, 46, 46, 0)]


def cdiv(a, b):
    return -(-a // b)


def max_resolutions(w, h):
    """The most resolutions (levels + 1) PIL's encoder takes for a w x h tile."""
    return int(np.floor(np.log2(min(w, h)))) + 1


def encode(arr, **kw):
    """A raw reversible codestream of a uint8 / uint16 gray or uint8 RGB array, by PIL (OpenJPEG).
    num_resolutions above what the size allows is lowered to that."""
    from PIL import Image
    h, w = arr.shape[:2]
    kw = dict(kw)
    kw["num_resolutions"] = min(kw.get("num_resolutions", 6), max_resolutions(w, h))
    kw.setdefault("mct", 0)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG2000", no_jp2=True, irreversible=False, **kw)
    return buf.getvalue()


def pil_decode(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


# ------------------------------------------------------------------------------- main header
def parse(data):
    """The main and tile-part header of a valid one-tile codestream: a dict, `data` / `end` being
    the span of the packets."""
    assert data[:2] == b"\xff\x4f", "no SOC"
    q, out = 2, {}
    while True:
        code = data[q + 1]
        assert data[q] == 0xFF
        if code == 0x93:  # SOD
            out["data"] = q + 2
            break
        L = struct.unpack(">H", data[q + 2:q + 4])[0]
        p = data[q + 4:q + 2 + L]
        if code == 0x51:
            xs, ys, xo, yo, xt, yt, xto, yto, nc = struct.unpack(">8IH", p[2:36])
            out.update(w=xs, h=ys, ncomp=nc, prec=(p[36] & 127) + 1, signed=p[36] >> 7)
        elif code == 0x52:
            out.update(scod=p[0], prog=p[1], layers=struct.unpack(">H", p[2:4])[0], mct=p[4], levels=p[5],
                       xcb=p[6] + 2, ycb=p[7] + 2, style=p[8], transform=p[9],
                       pp=[(b & 15, b >> 4) for b in p[10:]] if p[0] & 1 else [(15, 15)] * (p[5] + 1))
        elif code == 0x5C:
            out.update(guard=p[0] >> 5, qstyle=p[0] & 31, exps=[b >> 3 for b in p[1:]])
        elif code == 0x90:
            psot = struct.unpack(">I", p[2:6])[0]
            out["end"] = min(q + psot, len(data)) if psot else (len(data) - 2 if data[-2:] == b"\xff\xd9" else len(data))
        q += 2 + L
    return out


def geometry(h):
    """Per component the sub-bands in QCD order (LL, then HL, LH, HH of resolutions 1 ..): dicts of
    r, orient (0 LL, 1 HL, 2 LH, 3 HH), the rectangle x0, y0, w, h in the component's plane (every
    resolution's low-pass band top left), the block size cbw x cbh, the grid nbx x nby, mb."""
    W, H, NL = h["w"], h["h"], h["levels"]
    rw = [cdiv(W, 1 << (NL - r)) for r in range(NL + 1)]
    rh = [cdiv(H, 1 << (NL - r)) for r in range(NL + 1)]
    bands = []
    for r in range(NL + 1):
        ppx, ppy = h["pp"][r]
        assert cdiv(rw[r], 1 << ppx) == 1 and cdiv(rh[r], 1 << ppy) == 1, "more than one precinct"
        cbw = 1 << min(h["xcb"], ppx - (1 if r else 0))
        cbh = 1 << min(h["ycb"], ppy - (1 if r else 0))
        if r == 0:
            rects = [(0, 0, 0, rw[0], rh[0])]
        else:
            lw, lh = rw[r - 1], rh[r - 1]
            rects = [(1, lw, 0, rw[r] - lw, lh), (2, 0, lh, lw, rh[r] - lh), (3, lw, lh, rw[r] - lw, rh[r] - lh)]
        for o, x0, y0, bw, bh in rects:
            empty = bw == 0 or bh == 0
            bands.append(dict(r=r, orient=o, x0=x0, y0=y0, w=bw, h=bh, cbw=cbw, cbh=cbh,
                              nbx=0 if empty else cdiv(bw, cbw), nby=0 if empty else cdiv(bh, cbh),
                              mb=h["guard"] + h["exps"][len(bands)] - 1))
    return bands, rw, rh


def counts(data):
    """(code blocks, packets, coefficient bytes: two int32 planes per component, each rounded up
    to 256 bytes) of one codestream: what the planner reports."""
    h = parse(data)
    bands, _, _ = geometry(h)
    plane = (h["w"] * h["h"] * 4 + 255) & ~255
    return h["ncomp"] * sum(b["nbx"] * b["nby"] for b in bands), h["ncomp"] * (h["levels"] + 1), 2 * plane * h["ncomp"]


# ------------------------------------------------------------------------------ packet headers
class Bits:
    """B.10.1: after an FF byte the next byte gives 7 bits."""

    def __init__(self, data, pos, end):
        self.d, self.pos, self.end, self.buf, self.ct = data, pos, end, 0, 0

    def bit(self):
        if self.ct == 0:
            if self.pos >= self.end:
                raise ValueError("packet header runs past the stream's end")
            self.ct = 7 if self.buf == 0xFF else 8
            self.buf = self.d[self.pos]
            self.pos += 1
        self.ct -= 1
        return (self.buf >> self.ct) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v

    def align(self):
        if self.buf == 0xFF:  # (the byte just read: a stuffed byte follows)
            self.pos += 1
        self.ct = 0
        self.buf = 0
        return self.pos


class TagTree:
    def __init__(self, w, h):
        self.dims = []
        while True:
            self.dims.append((w, h))
            if w <= 1 and h <= 1:
                break
            w, h = cdiv(w, 2), cdiv(h, 2)
        self.val = [[None] * (a * b) for a, b in self.dims]
        self.low = [[0] * (a * b) for a, b in self.dims]

    def decode(self, bits, x, y, threshold):
        low = 0
        for l in range(len(self.dims) - 1, -1, -1):
            i = (y >> l) * self.dims[l][0] + (x >> l)
            if low > self.low[l][i]:
                self.low[l][i] = low
            else:
                low = self.low[l][i]
            while low < threshold and (self.val[l][i] is None or low < self.val[l][i]):
                if bits.bit():
                    self.val[l][i] = low
                else:
                    low += 1
            self.low[l][i] = low
        v = self.val[0][(y * self.dims[0][0]) + x]
        return v is not None and v < threshold


def packets(data, h, bands):
    """Tier 2: per component and band a dict (bx, by) -> (offset, length, passes, zero bit-planes)
    of the included code blocks."""
    NL, nc, nb = h["levels"], h["ncomp"], 3 * h["levels"] + 1
    order = [(r, c) for r in range(NL + 1) for c in range(nc)] if h["prog"] < 3 else \
            [(r, c) for c in range(nc) for r in range(NL + 1)]
    found = [[{} for _ in range(nb)] for _ in range(nc)]
    pos = h["data"]
    for r, c in order:
        bits = Bits(data, pos, h["end"])
        if not bits.bit():
            pos = bits.align()
            continue
        mine = [0] if r == 0 else [3 * r - 2, 3 * r - 1, 3 * r]
        todo = []
        for b in mine:
            B = bands[b]
            if B["nbx"] * B["nby"] == 0:
                continue
            incl, zbp = TagTree(B["nbx"], B["nby"]), TagTree(B["nbx"], B["nby"])
            for by in range(B["nby"]):
                for bx in range(B["nbx"]):
                    if not incl.decode(bits, bx, by, 1):
                        continue
                    z = 1
                    while not zbp.decode(bits, bx, by, z):
                        z += 1
                        if z - 1 > B["mb"]:
                            raise ValueError("zero bit-planes above Mb")
                    z -= 1
                    if not bits.bit():
                        n = 1
                    elif not bits.bit():
                        n = 2
                    else:
                        n = bits.bits(2)
                        if n < 3:
                            n += 3
                        else:
                            n = bits.bits(5)
                            n = n + 6 if n < 31 else bits.bits(7) + 37
                    if n > 3 * (B["mb"] - z) - 2:
                        raise ValueError("more passes than the bit-planes allow")
                    lblock = 3
                    while bits.bit():
                        lblock += 1
                    ln = bits.bits(lblock + n.bit_length() - 1)
                    todo.append((b, bx, by, ln, n, z))
        pos = bits.align()
        for b, bx, by, ln, n, z in todo:
            if pos + ln > h["end"]:
                raise ValueError("packet data runs past the stream's end")
            found[c][b][(bx, by)] = (pos, ln, n, z)
            pos += ln
    return found


# ---------------------------------------------------------------------------------- code blocks
class MQDecoder:
    def __init__(self, data):
        self.d, self.bp = data, 0
        self.I, self.mps = [0] * 19, [0] * 19
        self.I[0], self.I[17], self.I[18] = 4, 3, 46
        self.c = self.byte(0) << 16
        self.bytein()
        self.c <<= 7
        self.ct -= 7
        self.a = 0x8000

    def byte(self, i):
        return self.d[i] if i < len(self.d) else 0xFF  # termination: 1-bits past the last byte

    def bytein(self):
        if self.byte(self.bp) == 0xFF:
            if self.byte(self.bp + 1) > 0x8F:
                self.c += 0xFF00
                self.ct = 8
            else:
                self.bp += 1
                self.c += self.byte(self.bp) << 9
                self.ct = 7
        else:
            self.bp += 1
            self.c += self.byte(self.bp) << 8
            self.ct = 8

    def decode(self, cx):
        qe, nmps, nlps, sw = MQ[self.I[cx]]
        self.a -= qe
        if (self.c >> 16) < qe:
            if self.a < qe:
                d, self.I[cx] = self.mps[cx], nmps
            else:
                d, self.I[cx] = 1 - self.mps[cx], nlps
                self.mps[cx] ^= sw
            self.a = qe
        else:
            self.c -= qe << 16
            if self.a & 0x8000:
                return self.mps[cx]
            if self.a < qe:
                d, self.I[cx] = 1 - self.mps[cx], nlps
                self.mps[cx] ^= sw
            else:
                d, self.I[cx] = self.mps[cx], nmps
        while True:
            if self.ct == 0:
                self.bytein()
            self.a = (self.a << 1) & 0xFFFF
            self.c = (self.c << 1) & 0xFFFFFFFF
            self.ct -= 1
            if self.a & 0x8000:
                return d


def zc_context(orient, hh, vv, dd):
    if orient == 1:
        hh, vv = vv, hh
    if orient == 3:
        hv = hh + vv
        if dd >= 3:
            return 8
        if dd == 2:
            return 7 if hv >= 1 else 6
        if dd == 1:
            return 5 if hv >= 2 else 4 if hv == 1 else 3
        return 2 if hv >= 2 else hv
    if hh == 2:
        return 8
    if hh == 1:
        return 7 if vv >= 1 else 6 if dd >= 1 else 5
    if vv == 2:
        return 4
    if vv == 1:
        return 3
    return 2 if dd >= 2 else dd


SC = {(1, 1): (13, 0), (1, 0): (12, 0), (1, -1): (11, 0), (0, 1): (10, 0), (0, 0): (9, 0), (0, -1): (10, 1),
      (-1, 1): (11, 1), (-1, 0): (12, 1), (-1, -1): (13, 1)}


def decode_block(code, w, h, orient, planes, passes):
    """Tier 1: the w x h coefficients of one code block whose `passes` coding passes start at
    bit-plane planes - 1."""
    mag = np.zeros((h, w), np.int64)
    sig = np.zeros((h + 2, w + 2), np.int8)   # bordered
    sgn = np.zeros((h + 2, w + 2), np.int8)   # +1 / -1 where significant
    vis = np.zeros((h, w), np.int8)
    ref = np.zeros((h, w), np.int8)
    if passes == 0:
        return mag
    mq = MQDecoder(code)

    def nbr(y, x):
        Y, X = y + 1, x + 1
        return (int(sig[Y, X - 1] + sig[Y, X + 1]), int(sig[Y - 1, X] + sig[Y + 1, X]),
                int(sig[Y - 1, X - 1] + sig[Y - 1, X + 1] + sig[Y + 1, X - 1] + sig[Y + 1, X + 1]))

    def sign(y, x, p):
        Y, X = y + 1, x + 1
        hc = max(-1, min(1, int(sgn[Y, X - 1]) + int(sgn[Y, X + 1])))
        vc = max(-1, min(1, int(sgn[Y - 1, X]) + int(sgn[Y + 1, X])))
        cx, xr = SC[(hc, vc)]
        s = mq.decode(cx) ^ xr
        sig[Y, X] = 1
        sgn[Y, X] = -1 if s else 1
        mag[y, x] |= 1 << p

    p, kind = planes - 1, 2
    for _ in range(passes):
        for y0 in range(0, h, 4):
            for x in range(w):
                ys = range(y0, min(y0 + 4, h))
                if kind == 0:
                    for y in ys:
                        if sig[y + 1, x + 1]:
                            continue
                        cx = zc_context(orient, *nbr(y, x))
                        if cx == 0:
                            continue
                        if mq.decode(cx):
                            sign(y, x, p)
                        vis[y, x] = 1
                elif kind == 1:
                    for y in ys:
                        if not sig[y + 1, x + 1] or vis[y, x]:
                            continue
                        cx = 16 if ref[y, x] else 15 if sum(nbr(y, x)) else 14
                        mag[y, x] |= mq.decode(cx) << p
                        ref[y, x] = 1
                else:
                    first = y0
                    if len(ys) == 4 and all(not sig[y + 1, x + 1] and not vis[y, x] and sum(nbr(y, x)) == 0 for y in ys):
                        if not mq.decode(17):
                            continue
                        first = y0 + (mq.decode(18) << 1 | mq.decode(18))
                        sign(first, x, p)
                        first += 1
                    for y in range(first, ys[-1] + 1):
                        if sig[y + 1, x + 1] or vis[y, x]:
                            continue
                        if mq.decode(zc_context(orient, *nbr(y, x))):
                            sign(y, x, p)
        if kind == 2:
            vis[:] = 0
            p -= 1
        kind = (kind + 1) % 3
    return mag * sgn[1:-1, 1:-1]


# ------------------------------------------------------------------------------------- wavelet
def sr_1d(low, high):
    """Inverse 5/3 lifting along the last axis: `low` the even samples, `high` the odd ones."""
    nl, nh = low.shape[-1], high.shape[-1]
    n = nl + nh
    x = np.zeros(low.shape[:-1] + (n,), np.int64)
    x[..., 0::2], x[..., 1::2] = low, high
    if n == 1:
        return x
    ext = lambda i: -i if i < 0 else 2 * (n - 1) - i if i >= n else i  # whole-sample symmetric
    for i in range(0, n, 2):
        x[..., i] -= (x[..., ext(i - 1)] + x[..., ext(i + 1)] + 2) >> 2
    for i in range(1, n, 2):
        x[..., i] += (x[..., ext(i - 1)] + x[..., ext(i + 1)]) >> 1
    return x


def idwt(plane, rw, rh):
    """plane: every resolution's low-pass band top left (geometry's rectangles); in place."""
    for r in range(1, len(rw)):
        lw, lh, cw, ch = rw[r - 1], rh[r - 1], rw[r], rh[r]
        a = plane[:ch, :cw].copy()
        rows = sr_1d(a[:, :lw], a[:, lw:])                       # HOR_SR
        plane[:ch, :cw] = sr_1d(rows[:lh].T, rows[lh:].T).T      # VER_SR
    return plane


def decode(data):
    """The whole decoder: a (h, w) or (h, w, 3) uint8 / uint16 array."""
    h = parse(data)
    assert h["transform"] == 1 and h["qstyle"] == 0 and h["layers"] == 1 and h["style"] == 0
    bands, rw, rh = geometry(h)
    found = packets(data, h, bands)
    comps = []
    for c in range(h["ncomp"]):
        plane = np.zeros((h["h"], h["w"]), np.int64)
        for b, B in enumerate(bands):
            for (bx, by), (off, ln, n, z) in found[c][b].items():
                x0, y0 = bx * B["cbw"], by * B["cbh"]
                w, hh = min(B["cbw"], B["w"] - x0), min(B["cbh"], B["h"] - y0)
                plane[B["y0"] + y0:B["y0"] + y0 + hh, B["x0"] + x0:B["x0"] + x0 + w] = \
                    decode_block(data[off:off + ln], w, hh, B["orient"], B["mb"] - z, n)
        comps.append(idwt(plane, rw, rh))
    if h["ncomp"] == 3 and h["mct"]:
        y, u, v = comps
        g = y - ((u + v) >> 2)
        comps = [v + g, g, u + g]
    P = h["prec"]
    out = [np.clip(c + (1 << (P - 1)), 0, (1 << P) - 1).astype(np.uint8 if P <= 8 else np.uint16) for c in comps]
    return out[0] if len(out) == 1 else np.stack(out, axis=-1)


# ------------------------------------------------------------------------------ header patches
def find_marker(data, code):
    """Offset of main-header marker FF `code` (walking the marker segments)."""
    q = 2
    while True:
        if data[q + 1] == code:
            return q
        assert data[q + 1] != 0x93, "marker FF %02X not found" % code
        q += 2 + struct.unpack(">H", data[q + 2:q + 4])[0]


def patch(data, code, at, value):
    """`data` with byte `at` of marker FF `code`'s payload (0: the first byte after its length)
    replaced."""
    q = find_marker(data, code) + 4 + at
    return data[:q] + bytes([value]) + data[q + 1:]


# ----------------------------------------------------------------------------- TIFF container
def page_of(arr, compression=33003, tile=None, rows_per_strip=None, planar=False, photometric=None, **kw):
    """A TIFF page (dict for write_tiff) of `arr` ((h, w) or (h, w, 3)) in JPEG 2000 strips or
    tiles: every segment one raw codestream of exactly its size, edge tiles padded by edge
    replication."""
    h, w = arr.shape[:2]
    spp = 1 if arr.ndim == 2 else arr.shape[2]
    subifds, description = kw.pop("subifds", []), kw.pop("description", None)
    segs = []
    srcs = [arr[..., s] for s in range(spp)] if planar and spp > 1 else [arr]
    for src in srcs:
        if tile:
            tw, th = tile
            pad = [(0, -h % th), (0, -w % tw)] + [(0, 0)] * (src.ndim - 2)
            full = np.pad(src, pad, mode="edge")
            for y in range(0, h, th):
                for x in range(0, w, tw):
                    segs.append(encode(np.ascontiguousarray(full[y:y + th, x:x + tw]), **kw))
        else:
            rps = rows_per_strip or h
            for y in range(0, h, rps):
                segs.append(encode(np.ascontiguousarray(src[y:y + rps]), **kw))
    return dict(width=w, length=h, bits=8 * arr.dtype.itemsize, spp=spp, compression=compression,
                photometric=photometric if photometric is not None else (2 if spp == 3 else 1),
                planar=2 if planar and spp > 1 else 1, tile=tile, rows_per_strip=rows_per_strip or h,
                segments=segs, subifds=subifds, description=description, array=arr)


def write_tiff(path, pages, byteorder="<", bigtiff=False):
    """Writes the pages (page_of's dicts; `subifds` = further pages under tag 330)."""
    bo = byteorder
    out = bytearray()
    if bigtiff:
        out += (b"II" if bo == "<" else b"MM") + struct.pack(bo + "HHHQ", 43, 8, 0, 0)
    else:
        out += (b"II" if bo == "<" else b"MM") + struct.pack(bo + "HI", 42, 0)
    off_fmt, off_type, inline = ("Q", 16, 8) if bigtiff else ("I", 4, 4)

    def put(b):
        if len(out) & 1:
            out.append(0)
        at = len(out)
        out.extend(b)
        return at

    def write_ifd(pg):
        """Appends the page's data and its IFD; returns (IFD offset, offset of its next-IFD field)."""
        subs = [write_ifd(s)[0] for s in pg["subifds"]]
        offs = [put(s) for s in pg["segments"]]
        cnts = [len(s) for s in pg["segments"]]
        spp = pg["spp"]
        tags = [(256, 4, [pg["width"]]), (257, 4, [pg["length"]]), (258, 3, [pg["bits"]] * spp),
                (259, 3, [pg["compression"]]), (262, 3, [pg["photometric"]]), (277, 3, [spp]),
                (284, 3, [pg["planar"]])]
        if pg.get("description"):
            tags.append((270, 2, pg["description"].encode() + b"\0"))
        if pg["tile"]:
            tags += [(322, 4, [pg["tile"][0]]), (323, 4, [pg["tile"][1]]), (324, off_type, offs), (325, 4, cnts)]
        else:
            tags += [(278, 4, [pg["rows_per_strip"]]), (273, off_type, offs), (279, 4, cnts)]
        if subs:
            tags.append((330, off_type, subs))
        tags.sort()
        entries = []
        for tag, typ, vals in tags:
            if typ == 2:
                raw, count = bytes(vals), len(vals)
            else:
                fmt = {3: "H", 4: "I", 16: "Q"}[typ]
                raw, count = struct.pack(bo + fmt * len(vals), *vals), len(vals)
            if len(raw) <= inline:
                field = raw.ljust(inline, b"\0")
            else:
                field = struct.pack(bo + off_fmt, put(raw))
            entries.append(struct.pack(bo + "HH" + off_fmt, tag, typ, count) + field)
        at = put(b"")
        out.extend(struct.pack(bo + ("Q" if bigtiff else "H"), len(entries)))
        for e in entries:
            out.extend(e)
        nxt = len(out)
        out.extend(struct.pack(bo + off_fmt, 0))
        return at, nxt

    prev = 8 if bigtiff else 4
    for pg in pages:
        at, nxt = write_ifd(pg)
        struct.pack_into(bo + off_fmt, out, prev, at)
        prev = nxt
    with open(path, "wb") as f:
        f.write(out)
