"""Test helper: JPEG 2000 codestreams with subsampled chroma, and YCbCr components outside the
codestream (DESIGN.md section 10b "Subsampled and YCbCr components"), on top of
tests/_tiff_j2k_packets.py.

PIL's OpenJPEG encoder cannot subsample, so a subsampled stream is assembled at tier 2 from three
single-component PIL streams: Y at W x H, Cb and Cr at ceil(W / xs) x ceil(H / ys), all with the same
COD and QCD.  The merged stream is the Y stream's main header with SIZ rewritten (Csiz 3, XRsiz and
YRsiz of components 1 and 2) and Psot zeroed, then the three streams' packets interleaved in the
merged stream's own order (T.800 B.12 with sampling factors), then EOC.

The expected planes need no decoder of merged streams: component c of the merged stream is the
single-component stream it came from, so plane 0 is Y's pixels and planes 1, 2 are Cb's and Cr's,
replicated (plane sample (x, y) = component sample (x / xs, y / ys)), and with the YCbCr flag
tests/_tiff_jpeg.py's ycc_to_rgb of those three."""
import json
import os
import struct

import numpy as np

import _tiff_j2k as J
import _tiff_j2k97 as J97
import _tiff_j2k_packets as P
from _tiff_jpeg import ycc_to_rgb

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_j2k_chroma")
F_PACKETS, F_SUB, F_YCC = 1, 4, 8  # pbx.TIFF_F_J2K_PACKETS, _SUBSAMPLED, _YCBCR
FACTORS = [(2, 1), (1, 2), (2, 2)]


def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)["files"]


def sub(a, xs, ys):
    """What an encoder that subsamples by dropping keeps of a full-size component."""
    return np.ascontiguousarray(a[::ys, ::xs])


def up(c, xs, ys, w, h):
    """Replication: plane sample (x, y) is component sample (x // xs, y // ys)."""
    return np.repeat(np.repeat(c, ys, axis=0), xs, axis=1)[:h, :w]


def planes(y, cb, cr, xs, ys, ycbcr):
    """The (h, w, 3) array the library stores for components y (h, w), cb and cr (subsampled)."""
    h, w = y.shape
    u, v = up(cb, xs, ys, w, h), up(cr, xs, ys, w, h)
    return ycc_to_rgb(y, u, v) if ycbcr else np.stack([y, u, v], axis=-1)


def num_resolutions(w, h, xs, ys, want=6):
    """The same count for the three streams, or their packets cannot be interleaved."""
    return min(want, J.max_resolutions(w, h), J.max_resolutions(J.cdiv(w, xs), J.cdiv(h, ys)))


# ------------------------------------------------------------------------------ packet order
def packet_order(h, precs, factors):
    """P.packet_order with sampling factors: (layer, resolution, component, px, py) of every packet
    of a stream whose component c has the precinct grids precs[c] and the factors factors[c].  The
    position loops of B.12.1.3 - 5 walk the reference grid and take a precinct where x is a
    multiple of XRsiz 2^(PPx + NL - r) and y of YRsiz 2^(PPy + NL - r) (no offsets, one tile)."""
    NL, nc, L = h["levels"], len(factors), h["layers"]
    W, H = h["w"], h["h"]
    out = []
    raster = lambda c, r: [(px, py) for py in range(precs[c][r][3]) for px in range(precs[c][r][2])]
    if h["prog"] == 0:
        return [(l, r, c, px, py) for l in range(L) for r in range(NL + 1) for c in range(nc) for px, py in raster(c, r)]
    if h["prog"] == 1:
        return [(l, r, c, px, py) for r in range(NL + 1) for l in range(L) for c in range(nc) for px, py in raster(c, r)]
    sx = min(factors[c][0] << (precs[c][r][0] + NL - r) for c in range(nc) for r in range(NL + 1))
    sy = min(factors[c][1] << (precs[c][r][1] + NL - r) for c in range(nc) for r in range(NL + 1))

    def here(c, r, x, y):
        dx, dy = factors[c][0] << (precs[c][r][0] + NL - r), factors[c][1] << (precs[c][r][1] + NL - r)
        if x % dx or y % dy:
            return None
        p = x // dx, y // dy  # (inside the grid whenever the factors are the component's: merge() counts)
        return p if p[0] < precs[c][r][2] and p[1] < precs[c][r][3] else None
    if h["prog"] == 2:
        loops = ((r, y, x, c) for r in range(NL + 1) for y in range(0, H, sy) for x in range(0, W, sx) for c in range(nc))
    elif h["prog"] == 3:
        loops = ((r, y, x, c) for y in range(0, H, sy) for x in range(0, W, sx) for c in range(nc) for r in range(NL + 1))
    else:
        loops = ((r, y, x, c) for c in range(nc) for y in range(0, H, sy) for x in range(0, W, sx) for r in range(NL + 1))
    for r, y, x, c in loops:
        p = here(c, r, x, y)
        if p:
            out += [(l, r, c) + p for l in range(L)]
    return out


# ------------------------------------------------------------------------------ the merge
def siz(w, h, comps):
    """A SIZ marker segment of one tile without offsets; comps = (Ssiz, XRsiz, YRsiz) each."""
    body = struct.pack(">H8IH", 0, w, h, 0, 0, w, h, 0, 0, len(comps)) + b"".join(bytes(c) for c in comps)
    return b"\xff\x51" + struct.pack(">H", len(body) + 2) + body


def marker_bytes(s, code):
    q = J.find_marker(s, code)
    return s[q:q + 2 + struct.unpack(">H", s[q + 2:q + 4])[0]]


def merge(streams, xs, ys):
    """One codestream of three components, the second and third subsampled xs x ys, from three
    single-component streams of the same COD and QCD (layers, precincts, SOP / EPH included)."""
    hs = [P.parse(s) for s in streams]
    assert len(streams) == 3 and all(h["ncomp"] == 1 and h["prec"] == 8 for h in hs)
    w, h = hs[0]["w"], hs[0]["h"]
    assert all((q["w"], q["h"]) == (J.cdiv(w, xs), J.cdiv(h, ys)) for q in hs[1:])
    assert all(marker_bytes(s, 0x52) == marker_bytes(streams[0], 0x52) for s in streams), "the CODs differ"
    assert all(marker_bytes(s, 0x5C) == marker_bytes(streams[0], 0x5C) for s in streams), "the QCDs differ"
    pk, precs = [], []
    for s in streams:
        _, geo, _, packets = P.walk(s)
        precs.append(geo[3])
        pk.append({(p["l"], p["r"], p["px"], p["py"]): s[p["start"]:p["data_end"]] for p in packets})
    order = packet_order(hs[0], precs, [(1, 1), (xs, ys), (xs, ys)])
    assert len(order) == sum(len(d) for d in pk)
    body = b"".join(pk[c][(l, r, px, py)] for l, r, c, px, py in order)
    s = streams[0]
    q = J.find_marker(s, 0x51)
    L = struct.unpack(">H", s[q + 2:q + 4])[0]
    head = s[:q] + siz(w, h, [(7, 1, 1), (7, xs, ys), (7, xs, ys)]) + s[q + 2 + L:hs[0]["data"]]
    q = J.find_marker(head, 0x90)
    head = head[:q + 6] + struct.pack(">I", 0) + head[q + 10:]
    return head + body + b"\xff\xd9"


def encode(y, cb, cr, xs, ys, irreversible=False, layers=None, sop=False, eph=False, **kw):
    """(merged stream, the three single-component streams) of components y (h, w) and cb, cr
    (subsampled already).  layers: (count, P.relayer split) cuts every component's packets anew;
    sop / eph: P.insert_sop_eph on every component."""
    h, w = y.shape
    kw = dict(kw)
    kw["num_resolutions"] = num_resolutions(w, h, xs, ys, kw.get("num_resolutions", 6))
    enc = J97.encode if irreversible else J.encode
    ss = [enc(np.ascontiguousarray(a), **kw) for a in (y, cb, cr)]
    if layers:
        ss = [P.relayer(s, layers[0], layers[1]) for s in ss]
    if sop or eph:
        ss = [P.insert_sop_eph(s, sop, eph) for s in ss]
    if not irreversible:  # PIL stays the judge of what the rewriting left
        assert all(np.array_equal(J.pil_decode(s), a) for s, a in zip(ss, (y, cb, cr)))
    return merge(ss, xs, ys), ss


def counts(singles):
    """(code blocks, packets, scratch bytes) of a merged stream as the planner reports them: every
    component's own grids, two dword planes of the component's own size each rounded up to 256
    bytes, and with several layers a gather area of the merged packets' length."""
    blocks = packets = scratch = length = 0
    for s in singles:
        h = P.parse(s)
        b, p, _ = P.counts(s)
        blocks, packets = blocks + b, packets + p
        scratch += 2 * ((h["w"] * h["h"] * 4 + 255) & ~255)
        length += h["end"] - h["data"]
    if P.parse(singles[0])["layers"] > 1:
        scratch += (length + 255) & ~255
    return blocks, packets, scratch


def model(singles, xs, ys):
    """The reals before rounding of the three components of a merged irreversible stream, each its
    own single-component stream's float64 model, replicated: (h, w, 3)."""
    ms = [P.decode_real(s) for s in singles]
    h, w = ms[0].shape
    return np.stack([ms[0], up(ms[1], xs, ys, w, h), up(ms[2], xs, ys, w, h)], axis=-1)


# ------------------------------------------------------------------------------ TIFF pages
def page_of(ycc, xs, ys, compression=33003, tile=None, rows_per_strip=None, photometric=2, irreversible=False, **kw):
    """A J.write_tiff page of the full-size (h, w, 3) components `ycc` in merged strips or tiles:
    the chroma of every segment is sub() of its part of the (edge-padded) full-size chroma, which
    is the whole image's sub() because segments start on even rows and columns.  The page keeps
    `singles` (per segment the three streams) beside `segments`."""
    h, w = ycc.shape[:2]
    segs, singles = [], []
    if tile:
        tw, th = tile
        full = np.pad(ycc, [(0, -h % th), (0, -w % tw), (0, 0)], mode="edge")
        cuts = [full[y:y + th, x:x + tw] for y in range(0, h, th) for x in range(0, w, tw)]
    else:
        rps = rows_per_strip or h
        assert rps % ys == 0 or rps >= h
        cuts = [ycc[y:y + rps] for y in range(0, h, rps)]
    for a in cuts:
        m, ss = encode(a[:, :, 0], sub(a[:, :, 1], xs, ys), sub(a[:, :, 2], xs, ys), xs, ys, irreversible, **kw)
        segs.append(m)
        singles.append(ss)
    return dict(width=w, length=h, bits=8, spp=3, compression=compression, photometric=photometric, planar=1, tile=tile,
                rows_per_strip=rows_per_strip or h, segments=segs, singles=singles, subifds=[], description=None,
                array=ycc, factors=(xs, ys))


def page_planes(page, ycbcr):
    """The (h, w, 3) array the library stores for a reversible page_of() page."""
    a = page["array"]
    xs, ys = page["factors"]
    return planes(a[:, :, 0], sub(a[:, :, 1], xs, ys), sub(a[:, :, 2], xs, ys), xs, ys, ycbcr)


def page_model(page):
    """J97.assemble of an irreversible page: the (h, w, 3) reals of its components, replicated."""
    xs, ys = page["factors"]
    lookup = dict(zip(page["segments"], page["singles"]))
    return J97.assemble(page, lambda seg: model(lookup[seg], xs, ys))


def hook_page(page, flags):
    return P.hook_page(page, flags)


def ycc_noise(w, h, seed):
    return P.noise(w, h, seed, np.uint8, 3)


def ycc_smooth(w, h, seed):
    """Y a textured gradient, Cb and Cr smooth and away from 128, so that the conversion shows."""
    a = P.smooth(w, h, seed, np.uint8, 3)
    a[:, :, 1] = 64 + a[:, :, 1] // 4
    a[:, :, 2] = 224 - a[:, :, 2] // 3
    return a
