"""Test helper: the packet structure of JPEG 2000 (T.800 B.6 - B.12) on top of tests/_tiff_j2k.py
and tests/_tiff_j2k97.py, whose models take one layer and one precinct per resolution: precinct
geometry, the five progression orders written as the standard's own loops, tier 2 over several
quality layers (inclusion against layer + 1, Lblock and passes kept from layer to layer, a block's
bytes concatenated over its packets), and SOP / EPH markers.  Tier 1, the wavelets and the colour
transforms are those modules'.  Slow; for images of a few hundred pixels.

walk() also keeps what the tests assert about their fixtures (which blocks contribute in which
layers, how Lblock grows, which precincts are empty) and where every packet's header and data lie,
from which insert_sop_eph() rewrites a stream with the markers PIL cannot switch on."""
import struct

import numpy as np

import _tiff_j2k as J
import _tiff_j2k97 as J97

encode_plain = _encode = J.encode  # (J97.page_of swaps J.encode for its caller's encoder while it runs)
PROGRESSIONS = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"]
FLAG = 1  # pbx.TIFF_F_J2K_PACKETS


def parse(data):
    h = J97.parse(data)
    if h["qstyle"] == 0:
        h["exps"] = J.parse(data)["exps"]
    return h


def geometry(h):
    """J.geometry without its one-precinct rule, plus per resolution the precinct grid: bands (QCD
    order, each with its precinct's size in code blocks pbx x pby), rw, rh, precs[r] = (ppx, ppy,
    npx, npy)."""
    W, H, NL = h["w"], h["h"], h["levels"]
    rw = [J.cdiv(W, 1 << (NL - r)) for r in range(NL + 1)]
    rh = [J.cdiv(H, 1 << (NL - r)) for r in range(NL + 1)]
    bands, precs = [], []
    for r in range(NL + 1):
        ppx, ppy = h["pp"][r]
        assert r == 0 or (ppx and ppy), "precinct exponent 0 above resolution 0"
        precs.append((ppx, ppy, J.cdiv(rw[r], 1 << ppx), J.cdiv(rh[r], 1 << ppy)))
        pbw, pbh = 1 << (ppx - (1 if r else 0)), 1 << (ppy - (1 if r else 0))  # the precinct in a band
        cbw, cbh = min(1 << h["xcb"], pbw), min(1 << h["ycb"], pbh)           # B.7: clipped to it
        if r == 0:
            rects = [(0, 0, 0, rw[0], rh[0])]
        else:
            lw, lh = rw[r - 1], rh[r - 1]
            rects = [(1, lw, 0, rw[r] - lw, lh), (2, 0, lh, lw, rh[r] - lh), (3, lw, lh, rw[r] - lw, rh[r] - lh)]
        for o, x0, y0, bw, bh in rects:
            empty = bw == 0 or bh == 0
            bands.append(dict(r=r, orient=o, x0=x0, y0=y0, w=bw, h=bh, cbw=cbw, cbh=cbh,
                              nbx=0 if empty else J.cdiv(bw, cbw), nby=0 if empty else J.cdiv(bh, cbh),
                              pbx=pbw // cbw, pby=pbh // cbh, mb=h["guard"] + h["exps"][len(bands)] - 1))
    return bands, rw, rh, precs


def window(B, px, py):
    """Precinct (px, py)'s code blocks of band B: (first bx, first by, count x, count y)."""
    x0, y0 = px * B["pbx"], py * B["pby"]
    if x0 >= B["nbx"] or y0 >= B["nby"]:
        return x0, y0, 0, 0
    return x0, y0, min(B["pbx"], B["nbx"] - x0), min(B["pby"], B["nby"] - y0)


def packet_order(h, precs):
    """(layer, resolution, component, px, py) of every packet in stream order: B.12.1.1 - 5 as the
    standard writes them, the position loops walking the reference grid (no offsets, no
    subsampling, one tile)."""
    NL, nc, L = h["levels"], h["ncomp"], h["layers"]
    W, H = h["w"], h["h"]
    out = []
    raster = lambda r: [(px, py) for py in range(precs[r][3]) for px in range(precs[r][2])]
    if h["prog"] == 0:
        return [(l, r, c, px, py) for l in range(L) for r in range(NL + 1) for c in range(nc) for px, py in raster(r)]
    if h["prog"] == 1:
        return [(l, r, c, px, py) for r in range(NL + 1) for l in range(L) for c in range(nc) for px, py in raster(r)]
    sx = min(1 << (precs[r][0] + NL - r) for r in range(NL + 1))
    sy = min(1 << (precs[r][1] + NL - r) for r in range(NL + 1))

    def here(r, x, y):
        ex, ey = precs[r][0] + NL - r, precs[r][1] + NL - r
        if x % (1 << ex) or y % (1 << ey):
            return None
        return x >> ex, y >> ey
    if h["prog"] == 2:
        for r in range(NL + 1):
            for y in range(0, H, sy):
                for x in range(0, W, sx):
                    for c in range(nc):
                        p = here(r, x, y)
                        if p:
                            out += [(l, r, c) + p for l in range(L)]
    elif h["prog"] == 3:
        for y in range(0, H, sy):
            for x in range(0, W, sx):
                for c in range(nc):
                    for r in range(NL + 1):
                        p = here(r, x, y)
                        if p:
                            out += [(l, r, c) + p for l in range(L)]
    else:
        for c in range(nc):
            for y in range(0, H, sy):
                for x in range(0, W, sx):
                    for r in range(NL + 1):
                        p = here(r, x, y)
                        if p:
                            out += [(l, r, c) + p for l in range(L)]
    return out


class Block:
    def __init__(self):
        self.lblock, self.passes, self.zbp = 3, 0, None
        self.parts = []      # (layer, offset, length, passes) of every packet it is included in
        self.lblocks = []    # Lblock after each of them
        self.skipped = []    # layers after its first in which it is not included

    @property
    def length(self):
        return sum(p[2] for p in self.parts)


def walk(data, h=None):
    """Tier 2: (header, geometry, blocks, packets).  blocks[(c, b, bx, by)] is a Block for every
    included code block; packets holds per packet dict(l, r, c, px, py, start, header_end,
    data_end, empty): `start` before an SOP marker, header_end after the stuffed byte and an EPH
    marker.  ValueError with the device's words for what the device refuses."""
    h = h or parse(data)
    geo = geometry(h)
    bands, _, _, precs = geo
    nb = 3 * h["levels"] + 1
    blocks, trees, pk = {}, {}, []
    pos, end = h["data"], h["end"]
    for l, r, c, px, py in packet_order(h, precs):
        rec = dict(l=l, r=r, c=c, px=px, py=py, start=pos, sop=False)
        if h["scod"] & 2 and data[pos:pos + 2] == b"\xff\x91" and end - pos >= 6:
            pos += 6
            rec["sop"] = True
        rec["header"] = pos
        bits = J.Bits(data, pos, end)
        todo = []
        nonempty = bits.bit()
        for b in ([0] if r == 0 else [3 * r - 2, 3 * r - 1, 3 * r]) if nonempty else []:
            B = bands[b]
            x0, y0, nx, ny = window(B, px, py)
            if nx * ny == 0:
                continue
            key = (c, b, px, py)
            if key not in trees:
                trees[key] = (J.TagTree(nx, ny), J.TagTree(nx, ny))
            incl, zbp = trees[key]
            for by in range(ny):
                for bx in range(nx):
                    k = (c, b, x0 + bx, y0 + by)
                    blk = blocks.get(k)
                    if blk is None:
                        if not incl.decode(bits, bx, by, l + 1):
                            continue
                        blk = blocks[k] = Block()
                        z = 1
                        while not zbp.decode(bits, bx, by, z):
                            z += 1
                            if z - 1 > B["mb"]:
                                raise ValueError("zero bit-planes above Mb")
                        blk.zbp = z - 1
                    elif not bits.bit():
                        blk.skipped.append(l)
                        continue
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
                    blk.passes += n
                    if blk.passes > 3 * (B["mb"] - blk.zbp) - 2:
                        raise ValueError("more passes than the bit-planes allow")
                    while bits.bit():
                        blk.lblock += 1
                    nbits = blk.lblock + n.bit_length() - 1
                    if nbits > 32:
                        raise ValueError("malformed packet header")
                    todo.append((blk, bits.bits(nbits), n))
                    blk.lblocks.append(blk.lblock)
        pos = bits.align()
        if h["scod"] & 4:
            if pos + 2 > end or data[pos:pos + 2] != b"\xff\x92":
                raise ValueError("malformed packet header")
            pos += 2
        rec["header_end"] = pos
        for blk, ln, n in todo:
            if pos + ln > end:
                raise ValueError("packet data runs past the stream's end")
            blk.parts.append((l, pos, ln, n))
            pos += ln
        rec.update(data_end=pos, empty=not nonempty)
        pk.append(rec)
    return h, geo, blocks, pk


def code_bytes(data, blk):
    return b"".join(data[o:o + n] for _, o, n, _ in blk.parts)


def decode(data):
    """The whole decoder, reversible (J's arithmetic, exact) or irreversible (J97's float64 model,
    rounded half to even): a (h, w) or (h, w, 3) uint8 / uint16 array."""
    m = decode_real(data)
    h = parse(data)
    return m if h["transform"] == 1 else J97.rint(m, h["prec"])


def decode_real(data, dtype=np.float64):
    """A reversible stream's pixels, or an irreversible one's real values before rounding (dtype
    float32: the library's order of operations, J97.decode97's)."""
    h, (bands, rw, rh, _), blocks, _ = walk(data)
    assert h["style"] == 0
    irrev = h["transform"] == 0
    st = J97.steps(h) if irrev else None
    dt = dtype
    comps = [np.zeros((h["h"], h["w"]), dt if irrev else np.int64) for _ in range(h["ncomp"])]
    for (c, b, bx, by), blk in blocks.items():
        B = bands[b]
        x0, y0 = bx * B["cbw"], by * B["cbh"]
        w, hh = min(B["cbw"], B["w"] - x0), min(B["cbh"], B["h"] - y0)
        at = (slice(B["y0"] + y0, B["y0"] + y0 + hh), slice(B["x0"] + x0, B["x0"] + x0 + w))
        code = code_bytes(data, blk)
        if irrev:
            mag, sgn, low = J97.decode_block(code, w, hh, B["orient"], B["mb"] - blk.zbp, blk.passes)
            m2 = np.where(low >= 0, 2 * mag + (1 << np.maximum(low, 0)), 0)
            v = m2.astype(dt) * dt(0.5 * st[b][1])
            comps[c][at] = np.where(sgn < 0, -v, v)
        else:
            comps[c][at] = J.decode_block(code, w, hh, B["orient"], B["mb"] - blk.zbp, blk.passes)
    P = h["prec"]
    if irrev:
        comps = [J97.idwt97(p, rw, rh, dt) for p in comps]
        if h["ncomp"] == 3 and h["mct"]:
            y, cb, cr = comps
            comps = [y + dt(1.402) * cr, (y - dt(0.34413) * cb) - dt(0.71414) * cr, y + dt(1.772) * cb]
        out = [c + dt(1 << (P - 1)) for c in comps]
    else:
        comps = [J.idwt(p, rw, rh) for p in comps]
        if h["ncomp"] == 3 and h["mct"]:
            y, u, v = comps
            g = y - ((u + v) >> 2)
            comps = [v + g, g, u + g]
        out = [np.clip(c + (1 << (P - 1)), 0, (1 << P) - 1).astype(np.uint8 if P <= 8 else np.uint16) for c in comps]
    return out[0] if len(out) == 1 else np.stack(out, axis=-1)


def counts(data):
    """(code blocks, packets, scratch bytes) of one codestream as the planner reports them: two
    dword planes per component, each rounded up to 256 bytes, and for a stream of several layers
    a gather area of the packets' length, rounded up likewise."""
    h = parse(data)
    bands, _, _, precs = geometry(h)
    plane = (h["w"] * h["h"] * 4 + 255) & ~255
    gather = ((h["end"] - h["data"] + 255) & ~255) if h["layers"] > 1 else 0
    return (h["ncomp"] * sum(b["nbx"] * b["nby"] for b in bands),
            h["ncomp"] * h["layers"] * sum(p[2] * p[3] for p in precs), 2 * plane * h["ncomp"] + gather)


def facts(data):
    """What a fixture exercises of the walker, as a dict of booleans / lists."""
    h, (bands, rw, rh, precs), blocks, pk = walk(data)
    v = list(blocks.values())
    partial = False
    for r, (ppx, ppy, npx, npy) in enumerate(precs):
        partial |= npx > 1 and npy > 1 and rw[r] % (1 << ppx) != 0 and rh[r] % (1 << ppy) != 0
    empty = any(window(bands[b], px, py)[2:] == (0, 0) and bands[b]["nbx"] * bands[b]["nby"] > 0
                for b in range(len(bands)) for px in range(precs[bands[b]["r"]][2]) for py in range(precs[bands[b]["r"]][3]))
    return dict(several=any(sum(1 for p in b.parts if p[2]) >= 2 for b in v),
                late=any(b.parts[0][0] > 0 for b in v),
                skipped=any(b.skipped for b in v),
                lblock_grows=any(b.lblocks[-1] > b.lblocks[0] for b in v),
                partial_precinct=partial, empty_precinct=empty,
                lengths=sorted(p[2] for b in v if len(b.parts) > 1 for p in b.parts))


# ------------------------------------------------------------------------------ SOP / EPH
def set_scod(data, bits):
    q = J.find_marker(data, 0x52) + 4
    return data[:q] + bytes([data[q] | bits]) + data[q + 1:]


def insert_sop_eph(stream, sop, eph, skip_eph_of=None, skip_sop_of=()):
    """`stream` (no markers in it) with FF91 0004 Nsop before every packet and / or FF92 after every
    packet header, the Scod bits set and the added bytes counted into Psot.  skip_eph_of: the
    index of a packet that gets no EPH (a broken stream); skip_sop_of: packets that get no SOP
    (legal: the marker is optional per packet)."""
    h, _, _, pk = walk(stream)
    assert not h["scod"] & 6
    out = bytearray(stream[:h["data"]])
    for i, p in enumerate(pk):
        if sop and i not in skip_sop_of:
            out += b"\xff\x91\x00\x04" + struct.pack(">H", i & 0xFFFF)
        out += stream[p["start"]:p["header_end"]]
        if eph and i != skip_eph_of:
            out += b"\xff\x92"
        out += stream[p["header_end"]:p["data_end"]]
    added = len(out) - pk[-1]["data_end"] if pk else 0
    out += stream[pk[-1]["data_end"] if pk else h["data"]:]
    out = set_scod(bytes(out), (2 if sop else 0) | (4 if eph else 0))
    q = J.find_marker(out, 0x90)
    psot = struct.unpack(">I", out[q + 6:q + 10])[0]
    if psot:
        out = out[:q + 6] + struct.pack(">I", psot + added) + out[q + 10:]
    return out


# ------------------------------------------------------------------------------ the C-ABI hooks
def segments_struct(segs, seg_w, seg_h, tiled, flags=FLAG):
    import pbx
    data, offs = segs if isinstance(segs, tuple) else pbx.pack_chunks(segs)
    if len(data) == 0:
        data = np.zeros(1, np.uint8)
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor, s.flags = seg_w, seg_h, 1 if tiled else 0, pbx.TIFF_J2K, 1, flags
    s.data, s.offsets = data.ctypes.data, offs.ctypes.data
    return s, (data, offs)


def plan(segs, w, h, seg_w, seg_h, tiled, pixel_type, spp, y0=0, rows=0, flags=FLAG):
    """pbx_test_tiff_j2k_plan: (status, message, [streams, code blocks, packets, scratch bytes])."""
    import ctypes
    import pbx
    s, keep = segments_struct(segs, seg_w, seg_h, tiled, flags)
    out = (ctypes.c_uint64 * 4)()
    rc = pbx.lib().pbx_test_tiff_j2k_plan(ctypes.byref(s), w, h, pixel_type, spp, y0, rows, out)
    return rc, pbx.lib().pbx_last_error().decode() if rc else "", list(out)


def cpu_decode(segs, w, h, seg_w, seg_h, tiled, dtype, spp, flags=FLAG):
    """pbx_test_tiff_j2k_decode: (status, message, (spp, h, w) array)."""
    import ctypes
    import pbx
    s, keep = segments_struct(segs, seg_w, seg_h, tiled, flags)
    out = np.zeros((spp, h, w), dtype)
    rc = pbx.lib().pbx_test_tiff_j2k_decode(ctypes.byref(s), w, h, pbx.UINT8 if dtype == np.uint8 else pbx.UINT16, spp,
                                            out.ctypes.data, out.nbytes)
    return rc, pbx.lib().pbx_last_error().decode() if rc else "", out


def one(stream, a):
    h, w = a.shape[:2]
    return [stream], w, h, w, h, False


def planes(a):
    return a[None] if a.ndim == 2 else np.moveaxis(a, 2, 0)


def hook_page(page, flags=FLAG):
    """J97.hook_page with the flag: the CPU hook's planes of a page_of() page, (status, message,
    (h, w) or (h, w, spp) array).  The kernels are held to these bytes."""
    h, w, spp, tile = page["length"], page["width"], page["spp"], page["tile"]
    dt = page["array"].dtype.type
    rc, msg, out = cpu_decode(page["segments"], w, h, tile[0] if tile else w, tile[1] if tile else min(page["rows_per_strip"], h),
                              bool(tile), dt, spp, flags)
    if rc:
        return rc, msg, None
    return 0, "", out[0] if spp == 1 else np.moveaxis(out, 0, 2)


def noise(w, h, seed, dtype=np.uint8, samples=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, (h, w) if samples == 1 else (h, w, samples), dtype=dtype)


def smooth(w, h, seed, dtype=np.uint16, samples=1):
    """A gradient with texture and noise: blocks of very different sizes, so that a rate allocator
    spreads them over the layers."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    top = float(np.iinfo(dtype).max)
    out = []
    for s in range(samples):
        v = 0.5 + 0.3 * np.sin((x + 3 * s) / 5.0) * np.cos(y / 7.0) + 0.15 * (x / max(w - 1, 1)) + 0.04 * rng.standard_normal((h, w))
        out.append(np.clip(v, 0, 1) * top)
    a = np.stack(out, axis=-1).astype(dtype)
    return a[:, :, 0] if samples == 1 else a


# ------------------------------------------------------------------------------ a tier-2 writer
# PIL's rate allocator decides which passes go into which layer; a test that needs a block's bytes
# cut at given lengths (one byte, a wave's width, none at all) writes the packets itself.  A code
# block of style 0 is one codeword segment: wherever its bytes and passes are cut into layers, a
# decoder that gathers them reads the same segment, so PIL decodes a re-cut stream to the same
# pixels and stays the judge.
class BitsOut:
    """B.10.1 from the writer's side: the byte after an FF takes 7 bits."""

    def __init__(self):
        self.out, self.buf, self.ct = bytearray(), 0, 8

    def put(self, b):
        if self.ct == 0:
            self.out.append(self.buf)
            self.ct = 7 if self.buf == 0xFF else 8
            self.buf = 0
        self.ct -= 1
        self.buf |= (b & 1) << self.ct

    def bits(self, v, n):
        for k in range(n - 1, -1, -1):
            self.put(v >> k)

    def finish(self):
        self.out.append(self.buf)
        if self.buf == 0xFF:
            self.out.append(0)
        return bytes(self.out)


class TagOut:
    """B.10.2 from the writer's side: leaf values in raster order, a node the least of its children."""

    def __init__(self, w, h, leaves):
        self.dims = []
        while True:
            self.dims.append((w, h))
            if w <= 1 and h <= 1:
                break
            w, h = cdiv2(w), cdiv2(h)
        self.val = [list(leaves)]
        for l in range(1, len(self.dims)):
            pw, ph = self.dims[l - 1]
            w, h = self.dims[l]
            self.val.append([min(self.val[l - 1][yy * pw + xx] for yy in range(2 * y, min(2 * y + 2, ph))
                                 for xx in range(2 * x, min(2 * x + 2, pw))) for y in range(h) for x in range(w)])
        self.low = [[0] * len(v) for v in self.val]
        self.known = [[False] * len(v) for v in self.val]

    def encode(self, bits, x, y, threshold):
        low = 0
        for l in range(len(self.dims) - 1, -1, -1):
            i = (y >> l) * self.dims[l][0] + (x >> l)
            low = max(low, self.low[l][i])
            while low < threshold:
                if low >= self.val[l][i]:
                    if not self.known[l][i]:
                        bits.put(1)
                        self.known[l][i] = True
                    break
                bits.put(0)
                low += 1
            self.low[l][i] = low


def cdiv2(a):
    return (a + 1) // 2


def put_passes(bits, n):
    if n == 1:
        bits.put(0)
    elif n == 2:
        bits.bits(0b10, 2)
    elif n <= 5:
        bits.bits(0b11, 2)
        bits.bits(n - 3, 2)
    elif n <= 36:
        bits.bits(0b1111, 4)
        bits.bits(n - 6, 5)
    else:
        bits.bits(0b111111111, 9)
        bits.bits(n - 37, 7)


def relayer(stream, layers, split):
    """`stream` with its packets written anew for `layers` quality layers: split(key, passes, nbytes)
    -> per layer (passes, bytes) of block key = (c, b, bx, by), passes 0 where the layer leaves the
    block out; the sums are the block's.  Progression, precincts and everything else stay."""
    h, (bands, _, _, precs), blocks, _ = walk(stream)
    assert not h["scod"] & 6
    cut = {}
    for key, blk in blocks.items():
        parts = split(key, blk.passes, blk.length)
        assert len(parts) == layers and sum(p for p, _ in parts) == blk.passes and sum(n for _, n in parts) == blk.length
        assert all(p > 0 or n == 0 for p, n in parts)
        cut[key] = parts
    code = {key: code_bytes(stream, blk) for key, blk in blocks.items()}
    done = {key: 0 for key in blocks}       # bytes written so far
    lblock = {key: 3 for key in blocks}
    trees = {}
    out = bytearray()
    for l, r, c, px, py in packet_order(dict(h, layers=layers), precs):
        bits, body = BitsOut(), bytearray()
        mine = []
        for b in [0] if r == 0 else [3 * r - 2, 3 * r - 1, 3 * r]:
            x0, y0, nx, ny = window(bands[b], px, py)
            keys = [(c, b, x0 + bx, y0 + by) for by in range(ny) for bx in range(nx)]
            if nx * ny:
                mine.append((b, nx, ny, keys))
        if not any(key in cut and cut[key][l][0] for _, _, _, keys in mine):
            bits.put(0)
            out += bits.finish()
            continue
        bits.put(1)
        for b, nx, ny, keys in mine:
            tk = (c, b, px, py)
            if tk not in trees:
                first = [next((i for i, (p, _) in enumerate(cut[k]) if p), layers) if k in cut else layers for k in keys]
                trees[tk] = (TagOut(nx, ny, first), TagOut(nx, ny, [blocks[k].zbp if k in cut else 99 for k in keys]), first)
            incl, zbp, first = trees[tk]
            for i, k in enumerate(keys):
                bx, by = i % nx, i // nx
                if first[i] >= l:  # not included before this layer
                    incl.encode(bits, bx, by, l + 1)
                    if first[i] != l:
                        continue
                    zbp.encode(bits, bx, by, 10 ** 6)
                else:
                    bits.put(1 if cut[k][l][0] else 0)
                    if not cut[k][l][0]:
                        continue
                n, ln = cut[k][l]
                put_passes(bits, n)
                while lblock[k] + n.bit_length() - 1 < max(ln.bit_length(), 1):
                    bits.put(1)
                    lblock[k] += 1
                bits.put(0)
                bits.bits(ln, lblock[k] + n.bit_length() - 1)
                body += code[k][done[k]:done[k] + ln]
                done[k] += ln
        out += bits.finish() + body
    q = find_cod(stream) + 2
    res = stream[:q] + struct.pack(">H", layers) + stream[q + 2:h["data"]] + bytes(out) + stream[h["end"]:]
    q = J.find_marker(res, 0x90)
    psot = struct.unpack(">I", res[q + 6:q + 10])[0]
    if psot:
        res = res[:q + 6] + struct.pack(">I", psot + len(out) - (h["end"] - h["data"])) + res[q + 10:]
    return res


def find_cod(stream):
    return J.find_marker(stream, 0x52) + 4


# ------------------------------------------------------------------------------ shared cases
def wave_edges(key, passes, n):
    """relayer split over 8 layers: a pass without bytes, then 1, 63, 64 and 65 bytes, a layer that
    leaves the block out, 129 bytes, the rest."""
    parts, left_p, left_n = [], passes, n
    for w in (0, 1, 63, 64, 65, None, 129):
        if w is None or left_p <= 1 or left_n < w:
            parts.append((0, 0))
            continue
        parts.append((1, w))
        left_p, left_n = left_p - 1, left_n - w
    return parts + [(left_p, left_n)]


def thirds(key, passes, n):
    """relayer split over 3 layers, by the block's place: one layer alone (fewer than 3 passes), the first
    and the last with the middle one leaving it out, the last two, or all three with 0 and 1 byte
    first."""
    k = (key[2] + key[3]) % 3
    if passes < 3:
        return [(0, 0)] * k + [(passes, n)] + [(0, 0)] * (2 - k)
    if k == 1:
        return [(1, n // 5), (0, 0), (passes - 1, n - n // 5)]
    if k == 2:
        return [(0, 0), (1, n // 5), (passes - 1, n - n // 5)]
    return [(1, 0), (1, min(n, 1)), (passes - 2, n - min(n, 1))]


def encode_layers(a, rates=(8, 3, 0), precinct=(16, 16), cb=(8, 8), **kw):
    """A reversible stream of len(rates) layers by PIL, precincts declared (precinct >= 2 cb)."""
    return _encode(a, quality_mode="rates", quality_layers=list(rates), precinct_size=precinct, codeblock_size=cb, **kw)


def device_case():
    """The 40 x 24 uint16 stream of the device-code tests (CPU hook and GPU): LRCP, 3 layers."""
    a = smooth(40, 24, 5, np.uint16)
    return a, encode_layers(a, num_resolutions=4, progression="LRCP")


def flip_case():
    a = smooth(40, 24, 5, np.uint16)
    return a, insert_sop_eph(encode_layers(a, num_resolutions=4, progression="RPCL"), True, True)


def layer2_cuts(s):
    """(a cut inside a layer-2 packet header, a cut inside the last contribution of a block whose
    bytes are gathered) of an LRCP stream."""
    h, _, blocks, pk = walk(s)
    p = next(p for p in pk if p["l"] == 2 and not p["empty"] and p["header_end"] - p["header"] >= 2)
    multi = [b for b in blocks.values() if sum(1 for q in b.parts if q[2]) >= 2]
    last = max((b.parts[-1] for b in multi), key=lambda q: q[1])
    return p["header"] + 1, last[1] + last[2] - 1


def passes_overflow_in_the_sum(s):
    """`s` with the exponent of one sub-band lowered in the QCD, by as much as leaves every single
    packet's passes within the new bound and only a sum across layers above it."""
    h, (bands, _, _, _), blocks, _ = walk(s)
    q = J.find_marker(s, 0x5C) + 5
    for (c, b, bx, by), blk in sorted(blocks.items()):
        if len(blk.parts) < 2:
            continue
        # the new Mb: the first layers' passes fit, all of them do not
        for mb in range(bands[b]["mb"] - 1, blk.zbp, -1):
            allowed = 3 * (mb - blk.zbp) - 2
            firsts = blk.parts[0][3]
            mine = [v for k, v in blocks.items() if k[1] == b]
            if firsts <= allowed < blk.passes and all(v.zbp < mb and v.parts[0][3] <= 3 * (mb - v.zbp) - 2 for v in mine):
                exp = mb + 1 - h["guard"]
                return s[:q + b] + bytes([exp << 3]) + s[q + b + 1:]
    raise AssertionError("no block of this stream can overflow in the sum alone")


def flipped(s, n, seed):
    """n copies of s with one bit flipped after the header, seeded."""
    rng = np.random.default_rng(seed)
    start = parse(s)["data"]
    out = []
    for _ in range(n):
        bad = bytearray(s)
        bad[int(rng.integers(start, len(s)))] ^= 1 << int(rng.integers(8))
        out.append(bytes(bad))
    return out


