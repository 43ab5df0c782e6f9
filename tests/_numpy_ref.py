"""Independent numpy restatement of the synthetic plane generators.

Written separately from oracle/pbx_oracle.c and csrc/pbx_common.h so that the three agree
only if each follows the definitions: G_FAKE = Bio-Formats FakeReader.openBytes
(pixel = typeMin + x, 10-pixel boxes {series, planeNo, z, c, t} on rows y < 10);
G_NOISE = splitmix64 counter-hash noise, 257..1486.
"""
import numpy as np

DTYPES_BE = [">i1", ">u1", ">i2", ">u2", ">i4", ">u4", ">f4", ">f8"]
TYPE_MIN = [-128, 0, -32768, 0, -(1 << 31), 0, 0, 0]


def _splitmix(k):
    with np.errstate(over="ignore"):
        z = k + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _cast(pt, v):
    v = np.asarray(v, dtype=np.int64)
    if pt <= 5:
        bits = [8, 8, 16, 16, 32, 32][pt]
        u = (v & ((1 << bits) - 1)).astype(np.uint64)
        return u.astype(DTYPES_BE[pt].replace(">i", ">u"), copy=False).view(DTYPES_BE[pt]) \
            if pt in (0, 2, 4) else u.astype(DTYPES_BE[pt])
    return v.astype(DTYPES_BE[pt])


def region(kind, pt, x0, y0, w, h, seed=0, plane_no=0, z=0, c=0, t=0):
    """Big-endian bytes of a w x h region of the plane."""
    y, x = np.mgrid[y0:y0 + h, x0:x0 + w].astype(np.int64)
    if kind == 1:  # G_FAKE
        v = TYPE_MIN[pt] + x
        box = x // 10
        special = (y < 10) & (box <= 4)
        vals = np.choose(np.clip(box, 0, 4), [0, plane_no, z, c, t])
        v = np.where(special, vals, v)
    else:
        xu, yu = x.astype(np.uint64), y.astype(np.uint64)
        k = (np.uint64(seed) << np.uint64(48)) ^ (np.uint64(plane_no) << np.uint64(40)) ^ \
            (yu << np.uint64(20)) ^ xu
        r = _splitmix(k)
        v = (256 + ((x >> 5) + (y >> 5)) % 16 * 48 + (r & np.uint64(0xFF)).astype(np.int64)
             + ((r >> np.uint64(8)) & np.uint64(0xFF)).astype(np.int64))
    return np.ascontiguousarray(_cast(pt, v)).tobytes()


def downsample(a):
    """One level of the resolution pyramid (include/pbx.h pbx_plane_build_pyramid), restated
    independently of csrc/kernels_io.hip: the 2x2 box mean, the last column / row repeated
    for odd sizes; integers (exact sum + 2) >> 2 (floor for signed), floats
    ((a + b) + (c + d)) * 0.25 in the array's precision.  `a`: 2-D array (any byte order)."""
    if a.shape[1] % 2:
        a = np.concatenate([a, a[:, -1:]], axis=1)
    if a.shape[0] % 2:
        a = np.concatenate([a, a[-1:, :]], axis=0)
    p, q, r, s = a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]
    if a.dtype.kind == "f":
        return ((p + q) + (r + s)) * a.dtype.type(0.25)
    tot = p.astype(np.int64) + q.astype(np.int64) + r.astype(np.int64) + s.astype(np.int64)
    return ((tot + 2) >> 2).astype(a.dtype)


# ------------------------------------------------------------------ the PNG scanline stream
# Restated from the PNG specification (ISO/IEC 15948 clause 9: filter types 0..4 and the
# minimum-sum-of-absolute-differences heuristic of 12.8), not from oracle/pbx_oracle.c.

PNG_BPP = {0: 1, 1: 1, 2: 2, 3: 2}  # int8, uint8, int16, uint16: bytes per (grey) pixel


def png_rows(tile_be, pt, w, h, filt=0, paeth=None):
    """The filtered scanlines of a w x h tile of big-endian samples, with what led to them.

    tile_be: bytes / uint8 array of the tile (h rows of w big-endian samples).  Signed types
    get the most significant byte of every sample flipped (x ^ 0x80: PNG samples are
    unsigned).  filt 0..4: that filter on every row.  filt 5 (include/pbx.h, DESIGN.md §9
    item 5): first the tile mode -- on the middle row h // 2 (zeros above the tile), the best
    of Sub/Up/Avg/Paeth by the sum of |byte - prediction| (the lowest on ties) against None by
    the sum over the two byte planes ((i mod bpp) & 1) of the squared counts of the byte
    values, None winning ties -- and if None does not win, per row the filter 0..4 with the
    smallest sum of |byte - prediction|, the lowest on ties.

    paeth: None, or a function (left, up, ul) -> prediction that replaces the specification's
    Paeth predictor (tests/test_values.py: does a wrong predictor change these tiles' rows?).

    Returns dict(stream=uint8 (h, 1 + rb), sums=int64 (h, 5), choice=int (h,),
    tile_none=bool, q=(q0, q1))."""
    bpp = PNG_BPP[pt]
    rb = w * bpp
    a = np.frombuffer(bytes(tile_be), np.uint8).reshape(h, rb).astype(np.int32)
    if pt in (0, 2):
        a[:, 0::bpp] ^= 0x80
    left = np.zeros_like(a)
    left[:, bpp:] = a[:, :rb - bpp]
    up = np.zeros_like(a)
    up[1:] = a[:-1]
    ul = np.zeros_like(a)
    ul[1:, bpp:] = a[:-1, :rb - bpp]
    p = left + up - ul
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
    pae = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    if paeth is not None:
        pae = paeth(left, up, ul)
    pred = [np.zeros_like(a), left, up, (left + up) >> 1, pae]
    filtered = [(a - q) & 0xFF for q in pred]
    sums = np.stack([abs(a - q).sum(axis=1, dtype=np.int64) for q in pred], axis=1)
    tile_none, q0, q1 = False, 0, 0
    if filt == 5:
        r = h // 2
        fb = 1 + int(np.argmin(sums[r, 1:]))  # argmin: the first of equal minima

        def collisions(row):
            tot = 0
            for pl in (0, 1):
                sel = row[((np.arange(rb) % bpp) & 1) == pl]
                c = np.bincount(sel, minlength=256).astype(np.int64)
                tot += int((c * c).sum())
            return tot

        q0, q1 = collisions(a[r]), collisions(filtered[fb][r])
        tile_none = rb > 0 and h > 0 and q0 >= q1
        choice = np.zeros(h, np.int64) if tile_none else np.argmin(sums, axis=1)
    else:
        choice = np.full(h, filt, np.int64)
    stream = np.empty((h, 1 + rb), np.uint8)
    stream[:, 0] = choice
    allf = np.stack(filtered)  # (5, h, rb)
    stream[:, 1:] = allf[choice, np.arange(h)]
    return dict(stream=stream, sums=sums, choice=choice, tile_none=bool(tile_none), q=(q0, q1))


def png_stream(tile_be, pt, w, h, filt=0):
    """The bytes a PNG's IDAT inflates to (see png_rows)."""
    return png_rows(tile_be, pt, w, h, filt)["stream"].tobytes()
