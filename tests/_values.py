"""Value planes for the I/O kernels (csrc/kernels_io.hip): full-range sample values.

The synthetic generators give small positive numbers (G_NOISE: 257..1486) or a ramp (G_FAKE),
so most of the kernels' input domain never reaches them.  The planes here do: uniform random
bits, the extreme values of every pixel type in every 2x2 arrangement, every (left, up,
up-left) byte triple of the Paeth predictor, and rows whose filter sums tie.  numpy only;
tests/test_values.py checks on the CPU that the planes hold what they claim, on exactly the
regions tests/test_gpu_values.py requests.

Planes are 2-D arrays of big-endian samples (dtype _numpy_ref.DTYPES_BE[pt]); `.tobytes()`
is the big-endian byte plane.
"""
import functools

import numpy as np

import _numpy_ref as R

INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT, DOUBLE = range(8)
BPP = [1, 1, 2, 2, 4, 4, 4, 8]
PNG_TYPES = [INT8, UINT8, INT16, UINT16]


def le(plane):
    """The same samples in little-endian byte order (a host plane of the other order)."""
    return plane.astype(plane.dtype.newbyteorder("<"))


def from_bytes(buf, pt, sx, sy):
    return np.frombuffer(bytes(buf), R.DTYPES_BE[pt]).reshape(sy, sx)


# ------------------------------------------------------------------------- random bits

def random_bits(pt, sx, sy, seed):
    """Every bit of every sample uniform: negative values, all byte positions busy, floats of
    every class (denormals, infinities, NaNs with payloads)."""
    raw = np.random.default_rng([seed, pt, sx, sy]).bytes(sx * sy * BPP[pt])
    return from_bytes(raw, pt, sx, sy)


# ---------------------------------------------------------------------------- extremes

def extreme_values(pt):
    """The short per-type value list, as a big-endian array."""
    dt = R.DTYPES_BE[pt]
    if pt in (INT8, INT16, INT32):
        bits = 8 * BPP[pt]
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        return np.array([lo, hi, -1, 0, 1, lo + 1, hi - 1], dtype=np.int64).astype(dt)
    if pt in (UINT8, UINT16, UINT32):
        bits = 8 * BPP[pt]
        hi = (1 << bits) - 1
        return np.array([0, 1, hi - 1, hi, 1 << (bits - 1), (1 << (bits - 1)) - 1],
                        dtype=np.uint64).astype(dt)
    # floats by bit pattern: zero, smallest / largest denormal, smallest normal, 1, max
    # finite, infinity -- each with both signs -- and one quiet NaN
    if pt == FLOAT:
        pos = [0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000]
        sign, nan, ut = 0x80000000, 0x7FC00000, ">u4"
    else:
        pos = [0x0000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x0010000000000000,
               0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000]
        sign, nan, ut = 0x8000000000000000, 0x7FF8000000000000, ">u8"
    pats = [p for q in pos for p in (q, q | sign)] + [nan]
    return np.array(pats, dtype=np.uint64).astype(ut).view(dt)


# positions in extreme_values() of the float list
_F = dict(pz=0, nz=1, pd=2, nd=3, pD=4, nD=5, pn=6, nn=7, p1=8, n1=9, pmax=10, nmax=11, pinf=12,
          ninf=13, nan=14)


def required_cells(pt):
    """2x2 cells (indices into extreme_values, row-major a b / c d) a plane starts with, so that
    the smallest planes hold them too."""
    if pt <= UINT32:
        lo, hi = (0, 1) if pt in (INT8, INT16, INT32) else (0, 3)
        return [(lo, lo, lo, lo), (hi, hi, hi, hi)]
    f = _F
    return [(f["pmax"],) * 4, (f["pmax"], f["nmax"], f["pmax"], f["nmax"]), (f["nz"],) * 4,
            (f["pinf"], f["ninf"], f["p1"], f["p1"]),
            # denormal cells whose sum * 0.25 is a round-to-even tie: 3 D + d = 4 k + 2 units,
            # d + d + d - d = 2 units, D + D + d + d = 2^(m+1) units exactly (no tie)
            (f["pD"], f["pD"], f["pD"], f["pd"]), (f["pd"], f["pd"], f["pd"], f["nd"]),
            (f["nD"], f["nD"], f["nD"], f["nd"]), (f["pD"], f["pD"], f["pd"], f["pd"])]


@functools.lru_cache(maxsize=None)
def extreme_cells(pt):
    """(ncell, 4) indices: the required cells, then every combination of the value list, in an
    order that mixes the values early (k -> k * P mod n^4, P prime to n)."""
    n = len(extreme_values(pt))
    k = (np.arange(n ** 4, dtype=np.int64) * 1000003) % (n ** 4)
    combos = np.stack([k // n ** 3 % n, k // n ** 2 % n, k // n % n, k % n], axis=1)
    return np.concatenate([np.array(required_cells(pt), dtype=np.int64), combos])


def extremes_full_shape(pt):
    """The smallest even (sx, sy), about square, whose plane holds every cell."""
    ncell = len(extreme_cells(pt))
    ncx = int(np.ceil(np.sqrt(ncell)))
    ncy = -(-ncell // ncx)
    return 2 * ncx, 2 * ncy


def extremes(pt, sx, sy, start=0):
    """A plane tiled from 2x2 cells: cell (cx, cy) is extreme_cells[start + cy * ncx + cx]."""
    vals, cells = extreme_values(pt), extreme_cells(pt)
    ncx, ncy = (sx + 1) // 2, (sy + 1) // 2
    ids = (start + np.arange(ncx * ncy, dtype=np.int64)) % len(cells)
    c = cells[ids].reshape(ncy, ncx, 2, 2)           # [cy, cx, dy, dx]
    full = vals[c].transpose(0, 2, 1, 3).reshape(2 * ncy, 2 * ncx)
    return np.ascontiguousarray(full[:sy, :sx])


# ------------------------------------------------------------------------ Paeth triples

@functools.lru_cache(maxsize=None)
def de_bruijn():
    """B(256, 2): 65,536 bytes, cyclic, every ordered pair of bytes exactly once (the Lyndon
    words of length 1 and 2 over 0..255 in order: a, then a b for every b > a)."""
    seq = []
    for a in range(256):
        seq.append(a)
        for b in range(a + 1, 256):
            seq += [a, b]
    return np.array(seq, dtype=np.uint8)


PAETH_OVERLAP = 8  # symbols two neighbouring windows share (1 would do for one shift; with
#                    four shifts a pair at a window's edge must stay inside some window)


def paeth_windows(bpp, W):
    """Windows (rows) per constant: enough to walk the whole sequence, and even."""
    step = W // bpp - PAETH_OVERLAP
    n = -(-65536 // step)
    return n + (n & 1)


def paeth_tile_rows(bpp, W):
    return 2 * paeth_windows(bpp, W) + 2


def paeth_triples(bpp, W, a_lo, a_hi, shift=0):
    """uint8 (rows, W): for every constant a in [a_lo, a_hi), paeth_tile_rows rows that
    alternate a window of the de Bruijn sequence D and a row of bytes a.  On a constant row,
    at byte i >= bpp, (left, up, up-left) = (a, D[j], D[j - 1]).  bpp 2: every symbol fills
    both bytes of a sample.  `shift` moves every window start (a pair lands in another byte
    lane).  Cut tiles at even rows with even heights: a constant row must not start a tile.

    After the first half of a constant's windows come two equal rows of a byte ramp: they are
    the middle of the constant's tile (row h // 2 is the second), where Up leaves zeros, so the
    adaptive option's tile mode keeps filtering and its per-row sums see every row.  (Without
    them the middle row is a sequence row under a constant row, Up's residuals are a
    relabelling of the bytes, q0 == q1, and every tile goes to None.)"""
    D = de_bruijn()
    nsym = W // bpp
    nwin = paeth_windows(bpp, W)
    start = shift + np.arange(nwin, dtype=np.int64) * (nsym - PAETH_OVERLAP)
    seq = D[(start[:, None] + np.arange(nsym)[None, :]) % 65536]
    seq = np.repeat(seq, bpp, axis=1)                  # (nwin, W)
    n = a_hi - a_lo
    alt = np.empty((n, nwin, 2, W), np.uint8)
    alt[:, :, 0, :] = seq[None]
    alt[:, :, 1, :] = np.arange(a_lo, a_hi, dtype=np.uint8)[:, None, None]
    alt = alt.reshape(n, 2 * nwin, W)
    ramp = np.broadcast_to((np.arange(W) & 0xFF).astype(np.uint8), (n, 2, W))
    out = np.concatenate([alt[:, :nwin], ramp, alt[:, nwin:]], axis=1)
    return out.reshape(n * (2 * nwin + 2), W)


# The exhaustive device runs of tests/test_gpu_values.py (routing: see its docstring).  W: row
# bytes of a tile; x0: the tile's first byte in the plane (the plane has x0 pad bytes in front);
# per: constants per parametrised slice (about 4 MiB of plane, 8 MiB for the 16-bit planes of
# 1 KiB rows, which need twice the windows); shifts: (0,) = all triples in aggregate, four
# shifts = all triples in every byte lane.
PAETH_RUNS = {
    "f3_g1_u8": dict(pt=UINT8, W=1024, x0=0, per=32, shifts=(0, 1, 2, 3)),
    "f3_g2_u8": dict(pt=UINT8, W=2048, x0=0, per=32, shifts=(0,)),
    "f3_g1_u16": dict(pt=UINT16, W=1024, x0=0, per=32, shifts=(0,)),
    "f3_g1_i16": dict(pt=INT16, W=1024, x0=0, per=32, shifts=(0,)),
    "f3_g2_u16": dict(pt=UINT16, W=2048, x0=0, per=32, shifts=(0,)),
    "f2_u8": dict(pt=UINT8, W=1020, x0=0, per=32, shifts=(0, 1, 2, 3)),
    "f2_u16": dict(pt=UINT16, W=1020, x0=0, per=32, shifts=(0,)),
    "kf_u8": dict(pt=UINT8, W=1023, x0=1, per=32, shifts=(0,)),
}


def paeth_slices(run):
    per = PAETH_RUNS[run]["per"]
    return [(a, a + per) for a in range(0, 256, per)]


def paeth_cases():
    """(run, shift, a_lo, a_hi) of every parametrised device case."""
    return [(run, sh, lo, hi) for run, r in PAETH_RUNS.items() for sh in r["shifts"]
            for lo, hi in paeth_slices(run)]


def paeth_case(run, shift, a_lo, a_hi):
    """(plane, tiles): the big-endian plane of one case and its tiles (x, y, w, h) in samples,
    one tile per constant."""
    r = PAETH_RUNS[run]
    bpp = BPP[r["pt"]]
    body = paeth_triples(bpp, r["W"], a_lo, a_hi, shift)
    pitch = -(-(r["x0"] + r["W"]) // bpp) * bpp
    raw = np.zeros((body.shape[0], pitch), np.uint8)
    raw[:, r["x0"]:r["x0"] + r["W"]] = body
    plane = from_bytes(raw.tobytes(), r["pt"], pitch // bpp, body.shape[0])
    h = paeth_tile_rows(bpp, r["W"])
    tiles = [(r["x0"] // bpp, k * h, r["W"] // bpp, h) for k in range(a_hi - a_lo)]
    return plane, tiles


def cut(plane, x, y, w, h):
    """Big-endian bytes of a tile of a plane."""
    return np.ascontiguousarray(plane[y:y + h, x:x + w]).tobytes()


# --------------------------------------------------------------------------------- ties

# three two-valued alphabets (sums tie); and five neighbouring values, where Paeth's own tie
# pb == pc < pa (up against up-left: up - ul == -2 (left - ul)) occurs and its sum is close
# to the others', so that the order of Paeth's comparisons decides rows and tile modes
TIE_ALPHABETS = [(0, 255), (0, 1), (127, 128), (0, 1, 2, 3, 4)]
# row bytes of the tie tiles by the kernel that takes them (both sample sizes)
TIE_RB = {"f3": (16, 32, 48, 64), "f2": (20, 36), "kf": (18, 34)}
TIE_HEIGHTS = (1, 2, 3, 4, 6, 9, 13, 17)
TIE_PER_RB = 24          # tiles per (plane, row length)
TIE_WIDE_RB = 4000       # k_filter's plane-reading path (>= 3,840 B)
TIE_UNSTAGED_RB = 16400  # a row k_adaptive_mode cannot stage: the whole batch reads the plane
TIE_SPARSE_TILES, TIE_SPARSE_H = 16, 5
DET_H = 20


def _two_valued(rng, alphabet, rows, rb):
    return np.array(alphabet, np.uint8)[rng.integers(0, len(alphabet), (rows, rb))]


def tie_planes(unstaged=False):
    """Planes whose rows tie, each with its tiles: a list of dict(name, pt, plane, tiles, group)
    with tiles (x, y, w, h) in samples and group the kernel path that takes them ("f3", "f2",
    "kf" = k_filter from LDS, "kfw" = k_filter from the plane).

    Random planes over the TIE_ALPHABETS, rows of 16..64 bytes cut into tiles of 1..17 rows
    (and some of 4,000 bytes); and per sample size three deterministic blocks -- all zero (every
    sum 0; the tile mode's q0 == q1), every row equal to the row above but not constant (the
    first row: None ties Up, Sub ties Paeth), one constant non-zero byte -- cut at every path's
    widths.  unstaged=True adds a 16,400-byte tile and 2 KiB k_filter3 tiles: in such a batch
    k_adaptive_mode reads every tile from the plane and k_filter3 runs its two-chunk form."""
    out = []
    for pt in (UINT8, UINT16):
        bpp = BPP[pt]
        for ai, alphabet in enumerate(TIE_ALPHABETS):
            rng = np.random.default_rng([91, pt, ai])
            per_rb = TIE_PER_RB * (1 if len(alphabet) == 2 else 4)  # (few rows hang on Paeth's order)
            rows_per_rb = sum(TIE_HEIGHTS) * (per_rb // len(TIE_HEIGHTS))
            for group, rbs in TIE_RB.items():
                raw = _two_valued(rng, alphabet, rows_per_rb * len(rbs), 64)
                tiles, y = [], 0
                for rb in rbs:
                    for k in range(per_rb):
                        h = TIE_HEIGHTS[k % len(TIE_HEIGHTS)]
                        tiles.append((0, y, rb // bpp, h))
                        y += h
                out.append(dict(name="%s_%d_%d" % (group, pt, ai), pt=pt, group=group, tiles=tiles,
                                plane=from_bytes(raw.tobytes(), pt, 64 // bpp, raw.shape[0])))
            # 4,000-byte rows: dense two-valued rows do not tie, sparse ones do -- all the first
            # value but for eight columns that take the second with probability 0.4, so every
            # sum is a small number
            raw = _two_valued(rng, alphabet, 7, TIE_WIDE_RB)
            nsparse = TIE_SPARSE_TILES * (1 if len(alphabet) == 2 else 4)
            sparse = np.full((nsparse * TIE_SPARSE_H, TIE_WIDE_RB), alphabet[0], np.uint8)
            if len(alphabet) == 2:
                cols = rng.choice(np.arange(8, TIE_WIDE_RB), 8, replace=False)
                hit = rng.random((sparse.shape[0], 8)) < 0.4
                sparse[:, cols] = np.where(hit, alphabet[1], alphabet[0]).astype(np.uint8)
            else:  # one run of 24 busy bytes in every row
                sparse[:, 64:88] = _two_valued(rng, alphabet, sparse.shape[0], 24)
            raw = np.concatenate([raw, sparse])
            tiles = [(0, 0, TIE_WIDE_RB // bpp, 1), (0, 1, TIE_WIDE_RB // bpp, 6)]
            tiles += [(0, 7 + k * TIE_SPARSE_H, TIE_WIDE_RB // bpp, TIE_SPARSE_H)
                      for k in range(nsparse)]
            out.append(dict(name="kfw_%d_%d" % (pt, ai), pt=pt, group="kfw", tiles=tiles,
                            plane=from_bytes(raw.tobytes(), pt, TIE_WIDE_RB // bpp, raw.shape[0])))
        # deterministic blocks
        rng = np.random.default_rng([92, pt])
        wide = TIE_UNSTAGED_RB if unstaged else TIE_WIDE_RB
        raw = np.zeros((3 * DET_H, wide), np.uint8)
        raw[DET_H:2 * DET_H] = rng.integers(0, 256, (1, wide), dtype=np.uint8)
        raw[2 * DET_H:] = 7
        det = from_bytes(raw.tobytes(), pt, wide // bpp, 3 * DET_H)
        widths = [("f3", 16), ("f3", 64), ("f3", 1024), ("f2", 20), ("f2", 2044), ("kf", 18),
                  ("kf", 2052), ("kfw", TIE_WIDE_RB)]
        if unstaged:
            widths += [("f3", 2048), ("kfw", TIE_UNSTAGED_RB)]
        for group in ("f3", "f2", "kf", "kfw"):
            tiles = [(0, blk * DET_H, rb // bpp, DET_H) for g, rb in widths if g == group
                     for blk in range(3)]
            out.append(dict(name="det_%s_%d" % (group, pt), pt=pt, group=group, tiles=tiles, plane=det))
    return out


# ------------------------------------------------------------------------------ pyramid

def pyramid_shapes(pt):
    """(sx, sy) of the pyramid cases of a pixel type: the degenerate planes, and around the
    vector groups of k_downsample (N = 8 / sizeof(T) outputs from one 16-byte load per row):
    the last group whole, one sample short, one sample over."""
    n = 8 // BPP[pt]
    shapes = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3)]
    for w in (2 * n - 1, 2 * n, 2 * n + 1, 4 * n - 1, 4 * n + 1):
        shapes += [(w, h) for h in (1, 2, 3)]
    return list(dict.fromkeys(shapes))


def levels_to_1x1(sx, sy):
    n = 0
    while sx > 1 or sy > 1:
        sx, sy, n = (sx + 1) // 2, (sy + 1) // 2, n + 1
    return n


def nan_cells_listed(plane):
    """Where one pyramid level of an `extremes` float plane must be NaN, from the classes of the
    cell's values alone (no arithmetic): a NaN in the cell; a pair (a, b) or (c, d) of opposite
    infinities; or the two pair sums infinite with opposite signs, a pair sum being infinite
    when it holds an infinity or max + max of one sign."""
    a = plane
    if a.shape[1] % 2:
        a = np.concatenate([a, a[:, -1:]], axis=1)
    if a.shape[0] % 2:
        a = np.concatenate([a, a[-1:, :]], axis=0)
    a = a.astype(a.dtype.newbyteorder("="))
    big = np.finfo(a.dtype).max

    def pair(p, q):
        nan = np.isnan(p) | np.isnan(q) | (np.isinf(p) & np.isinf(q) & (np.signbit(p) != np.signbit(q)))
        pos = ~nan & ((p == np.inf) | (q == np.inf) | ((p == big) & (q == big)))
        neg = ~nan & ((p == -np.inf) | (q == -np.inf) | ((p == -big) & (q == -big)))
        return nan, pos, neg

    n1, p1, m1 = pair(a[0::2, 0::2], a[0::2, 1::2])
    n2, p2, m2 = pair(a[1::2, 0::2], a[1::2, 1::2])
    return n1 | n2 | (p1 & m2) | (m1 & p2)
