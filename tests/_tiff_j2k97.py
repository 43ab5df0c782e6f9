"""Test helper: a numpy model of the irreversible JPEG 2000 decoder (9/7 wavelet, scalar
quantisation, ICT) behind the TIFF source path (DESIGN.md section 10b "JPEG 2000 segments"), on
top of tests/_tiff_j2k.py's parser, geometry, packet headers and MQ decoder.

The lossy path has no input to be equal to, and OpenJPEG's own arithmetic is not T.800's at 16
bits (its decoder scales the high band by the literal 1.625732422 where 2 / K is 1.625786), so
the right answer is T.800's arithmetic in float64: decode97(data) gives the real values before
rounding.  The same model in float32 (dtype=np.float32) follows the library's order of
operations step for step and shows what single precision costs."""
import io
import json
import os
import struct

import numpy as np

import _tiff_j2k as J

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_j2k97")
K = 1.230174105
LIFT = (0.443506852, 0.882911075, -0.052980118, -1.586134342)  # delta, gamma, beta, alpha: the inverse's order


def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)["files"]


def encode(arr, **kw):
    """A raw irreversible codestream of a uint8 / uint16 gray or uint8 RGB array, by PIL (OpenJPEG):
    all passes, or with quality_mode="dB", quality_layers=[target] a truncated one."""
    from PIL import Image
    h, w = arr.shape[:2]
    kw = dict(kw)
    kw["num_resolutions"] = min(kw.get("num_resolutions", 6), J.max_resolutions(w, h))
    kw.setdefault("mct", 0)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG2000", no_jp2=True, irreversible=True, **kw)
    return buf.getvalue()


def page_of(arr, compression=33005, encoder=encode, **kw):
    """J.page_of with the segments encoded by `encoder` (this module's irreversible one)."""
    old = J.encode
    J.encode = encoder
    try:
        return J.page_of(arr, compression, **kw)
    finally:
        J.encode = old


def parse(data):
    """J.parse, plus the QCD's 16-bit entries: eps, mu per entry (one for style 1)."""
    h = J.parse(data)
    q = J.find_marker(data, 0x5C)
    L = struct.unpack(">H", data[q + 2:q + 4])[0]
    p = data[q + 5:q + 2 + L]
    if h["qstyle"] in (1, 2):
        ent = struct.unpack(">%dH" % (len(p) // 2), p)
        h["eps"], h["mu"] = [e >> 11 for e in ent], [e & 2047 for e in ent]
        h["exps"] = [e for e, _ in steps(h)]  # (what J.geometry takes Mb from)
    return h


def steps(h):
    """(eps_b, step_b) per sub-band in QCD order: T.800 E.1.1, style 1 by equation E-5."""
    NL, out = h["levels"], []
    for b in range(3 * NL + 1):
        if h["qstyle"] == 2:
            eps, mu = h["eps"][b], h["mu"][b]
        else:
            nb = NL if b == 0 else NL - ((b + 2) // 3 - 1)
            eps, mu = h["eps"][0] - (NL - nb), h["mu"][0]
        gain = 0 if b == 0 else 2 if (b - 1) % 3 == 2 else 1
        out.append((eps, 2.0 ** (h["prec"] + gain - eps) * (1 + mu / 2048.0)))
    return out


def to_style1(data):
    """The stream with its style-2 QCD rewritten as style 1: the LL entry alone, every other band's
    step derived from it.  (The code blocks were quantised with other steps: the image changes,
    the decoder's duty does not.)"""
    q = J.find_marker(data, 0x5C)
    L = struct.unpack(">H", data[q + 2:q + 4])[0]
    assert data[q + 4] & 31 == 2
    return data[:q + 2] + struct.pack(">HB", 5, (data[q + 4] & 0xE0) | 1) + data[q + 5:q + 7] + data[q + 2 + L:]


def decode_block(code, w, h, orient, planes, passes):
    """Tier 1 that remembers, per coefficient, the lowest bit-plane it was coded in: (magnitude,
    sign, low), low = -1 where the coefficient never became significant."""
    mag = np.zeros((h, w), np.int64)
    low = np.full((h, w), -1, np.int64)
    sig = np.zeros((h + 2, w + 2), np.int8)
    sgn = np.zeros((h + 2, w + 2), np.int8)
    vis = np.zeros((h, w), np.int8)
    ref = np.zeros((h, w), np.int8)
    if passes == 0:
        return mag, sgn[1:-1, 1:-1], low
    mq = J.MQDecoder(code)

    def nbr(y, x):
        Y, X = y + 1, x + 1
        return (int(sig[Y, X - 1] + sig[Y, X + 1]), int(sig[Y - 1, X] + sig[Y + 1, X]),
                int(sig[Y - 1, X - 1] + sig[Y - 1, X + 1] + sig[Y + 1, X - 1] + sig[Y + 1, X + 1]))

    def sign(y, x, p):
        Y, X = y + 1, x + 1
        hc = max(-1, min(1, int(sgn[Y, X - 1]) + int(sgn[Y, X + 1])))
        vc = max(-1, min(1, int(sgn[Y - 1, X]) + int(sgn[Y + 1, X])))
        cx, xr = J.SC[(hc, vc)]
        s = mq.decode(cx) ^ xr
        sig[Y, X] = 1
        sgn[Y, X] = -1 if s else 1
        mag[y, x] |= 1 << p
        low[y, x] = p

    p, kind = planes - 1, 2
    for _ in range(passes):
        for y0 in range(0, h, 4):
            for x in range(w):
                ys = range(y0, min(y0 + 4, h))
                if kind == 0:
                    for y in ys:
                        if sig[y + 1, x + 1]:
                            continue
                        cx = J.zc_context(orient, *nbr(y, x))
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
                        low[y, x] = p
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
                        if mq.decode(J.zc_context(orient, *nbr(y, x))):
                            sign(y, x, p)
        if kind == 2:
            vis[:] = 0
            p -= 1
        kind = (kind + 1) % 3
    return mag, sgn[1:-1, 1:-1], low


def sr97_1d(low, high, dt):
    """Inverse 9/7 lifting along the last axis (F.3.8), every operation rounded to dt: scale, then
    four steps x[i] -= c * (x[i - 1] + x[i + 1]) on alternating parities."""
    nl, nh = low.shape[-1], high.shape[-1]
    n = nl + nh
    x = np.zeros(low.shape[:-1] + (n,), dt)
    x[..., 0::2], x[..., 1::2] = low, high
    if n == 1:
        return x
    x[..., 0::2] = x[..., 0::2] * dt(K)
    x[..., 1::2] = x[..., 1::2] * (dt(np.float32(1.0 / K)) if dt is np.float32 else dt(1.0 / K))
    idx = np.arange(n)
    ext = lambda i: np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))  # whole-sample symmetric
    for k, c in enumerate(LIFT):
        i = idx[k & 1::2]
        s = x[..., ext(i - 1)] + x[..., ext(i + 1)]
        x[..., i] = x[..., i] - dt(c) * s
    return x


def idwt97(plane, rw, rh, dt):
    for r in range(1, len(rw)):
        lw, lh, cw, ch = rw[r - 1], rh[r - 1], rw[r], rh[r]
        a = plane[:ch, :cw].copy()
        rows = sr97_1d(a[:, :lw], a[:, lw:], dt)
        plane[:ch, :cw] = sr97_1d(rows[:lh].T, rows[lh:].T, dt).T
    return plane


def decode97(data, dtype=np.float64):
    """The values before rounding, level shift included: a float (h, w) or (h, w, 3) array."""
    dt = dtype
    h = parse(data)
    assert h["transform"] == 0 and h["qstyle"] in (1, 2) and h["layers"] == 1 and h["style"] == 0
    st = steps(h)
    bands, rw, rh = J.geometry(h)
    found = J.packets(data, h, bands)
    comps = []
    for c in range(h["ncomp"]):
        plane = np.zeros((h["h"], h["w"]), dt)
        for b, B in enumerate(bands):
            for (bx, by), (off, ln, n, z) in found[c][b].items():
                x0, y0 = bx * B["cbw"], by * B["cbh"]
                w, hh = min(B["cbw"], B["w"] - x0), min(B["cbh"], B["h"] - y0)
                mag, sgn, low = decode_block(data[off:off + ln], w, hh, B["orient"], B["mb"] - z, n)
                # twice the midpoint, an integer, times half the step: the library's order
                m2 = np.where(low >= 0, 2 * mag + (1 << np.maximum(low, 0)), 0)
                v = m2.astype(dt) * dt(0.5 * st[b][1])
                plane[B["y0"] + y0:B["y0"] + y0 + hh, B["x0"] + x0:B["x0"] + x0 + w] = np.where(sgn < 0, -v, v)
        comps.append(idwt97(plane, rw, rh, dt))
    if h["ncomp"] == 3 and h["mct"]:
        y, cb, cr = comps
        comps = [y + dt(1.402) * cr, (y - dt(0.34413) * cb) - dt(0.71414) * cr, y + dt(1.772) * cb]
    out = [c + dt(1 << (h["prec"] - 1)) for c in comps]
    return out[0] if len(out) == 1 else np.stack(out, axis=-1)


def rint(model, prec):
    """Round half to even and clamp: the decoder's output for these real values."""
    return np.clip(np.rint(model), 0, (1 << prec) - 1).astype(np.uint8 if prec <= 8 else np.uint16)


def in_window(model, window):
    """True where the real value lies within `window` of a half-integer: either neighbour is a fair
    answer of a decoder that computes in finite precision."""
    return np.abs(np.abs(model - np.floor(model)) - 0.5) <= window


def close(got, model, window, prec):
    """The acceptance criterion: (ok, share of pixels inside the window, mismatches outside it).
    got == rint(model) outside the window, within 1 of it inside."""
    want = rint(model, prec).astype(np.int64)
    d = np.abs(got.astype(np.int64) - want)
    inside = in_window(model, window)
    # a clamped value is not a rounding case
    ok = bool(np.all(d[~inside] == 0) and np.all(d <= 1))
    return ok, float(inside.mean()), int(np.count_nonzero(d[~inside]))


# --------------------------------------------------------------------------------- fixtures
# Windows of close(): how far from a half-integer a float32 decoder's value may lie and still
# round the other way.  8 bits: float32 has an ulp of 2^-14 at these magnitudes, over some 50
# operations.  16 bits: twice the largest |float32 model - float64 model| met over the CPU test
# inputs, generated streams and 16-bit fixtures (MEASURED16; tests/test_tiff_j2k97_host.py asserts
# that it is not exceeded and that the float32 model rounds to the library's bytes), rounded up to
# a power of two.
WINDOW8 = 1.0 / 64
MEASURED16 = 0.0567  # (0.05663, on pyramid_mixed_gray16.tif's five-level tiles)
WINDOW16 = 1.0 / 8


def window(prec):
    return WINDOW8 if prec <= 8 else WINDOW16


def decode_any(seg, dtype=np.float64):
    """decode97 of an irreversible stream, J.decode (exact) of a reversible one, as reals."""
    return decode97(seg, dtype) if J.parse(seg)["transform"] == 0 else J.decode(seg).astype(dtype)


def assemble(page, dec=decode_any):
    """The (h, w) or (h, w, spp) plane of a page_of() page from dec(segment) of its segments."""
    h, w, spp, tile = page["length"], page["width"], page["spp"], page["tile"]
    planar = page["planar"] == 2 and spp > 1
    tw, th = tile if tile else (w, min(page["rows_per_strip"], h))
    gx, gy = J.cdiv(w, tw), J.cdiv(h, th)
    out = None
    for k, seg in enumerate(page["segments"]):
        s, i = divmod(k, gx * gy) if planar else (0, k)
        x, y = (i % gx) * tw, (i // gx) * th
        m = np.asarray(dec(seg))
        m = m.reshape(m.shape[0], m.shape[1], -1)[:h - y, :w - x]
        if out is None:
            out = np.zeros((h, w, spp), m.dtype)
        if planar:
            out[y:y + m.shape[0], x:x + m.shape[1], s] = m[:, :, 0]
        else:
            out[y:y + m.shape[0], x:x + m.shape[1], :] = m
    return out[:, :, 0] if spp == 1 else out


def expected(entry, level, key):
    """(rint(model), in-window mask) of plane `key` ("z,c,t") of stored level `level`, as the
    generator stored them; the values checked against the manifest's hash."""
    import hashlib
    npy, index, digest = entry["planes"][str(level)][key]
    a, m = np.load(os.path.join(GOLD, npy)), np.load(os.path.join(GOLD, npy.replace(".npy", "_mask.npy")))
    m = np.unpackbits(m)[:a.size].reshape(a.shape).astype(bool)
    if index:
        a, m = a[:, :, index[0]], m[:, :, index[0]]
    a = np.ascontiguousarray(a)
    assert hashlib.sha256(J.be_bytes(a)).hexdigest() == digest, (entry["file"], key)
    return a, m


def check_close(got, want, mask, what=""):
    """close() against a stored rint(model) and mask."""
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert np.all(d[~mask] == 0) and np.all(d <= 1), (what, np.argwhere((d > 1) | ((d > 0) & ~mask))[:4].tolist())


def hook_page(page):
    """The CPU hook's (pbx_test_tiff_j2k_decode) planes of a page_of() page: (status, message,
    (h, w) or (h, w, spp) array).  The kernels are held to these bytes."""
    import ctypes
    import pbx
    h, w, spp, tile = page["length"], page["width"], page["spp"], page["tile"]
    dt = page["array"].dtype.type
    planar = page["planar"] == 2 and spp > 1
    segs, n = page["segments"], len(page["segments"]) // (spp if planar else 1)
    outs = []
    for c in range(spp if planar else 1):
        data, offs = pbx.pack_chunks(segs[c * n:(c + 1) * n] if planar else segs)
        s = pbx.PbxTiffSegments()
        s.seg_w, s.seg_h = (tile[0], tile[1]) if tile else (w, min(page["rows_per_strip"], h))
        s.tiled, s.compression, s.predictor, s.flags = 1 if tile else 0, pbx.TIFF_J2K, 1, 0
        s.data, s.offsets = data.ctypes.data, offs.ctypes.data
        k = 1 if planar else spp
        out = np.zeros((k, h, w), dt)
        rc = pbx.lib().pbx_test_tiff_j2k_decode(ctypes.byref(s), w, h, pbx.UINT8 if dt == np.uint8 else pbx.UINT16, k,
                                                out.ctypes.data, out.nbytes)
        if rc:
            return rc, pbx.lib().pbx_last_error().decode(), None
        outs += list(out)
    return 0, "", outs[0] if spp == 1 else np.stack(outs, axis=-1)
