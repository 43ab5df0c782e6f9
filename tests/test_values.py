"""CPU checks of the value planes (tests/_values.py) and of the references the GPU tests of
tests/test_gpu_values.py compare against.

Coverage conditions are asserted on exactly the planes and tiles the GPU tests request, so
that those cannot pass vacuously; the oracle's PNG stream is pinned to the numpy restatement
written from the PNG specification; the pyramid restatement is pinned to exact integer
arithmetic.
"""
import numpy as np
import pytest

import _numpy_ref as R
import _values as V

INT_TYPES = [V.INT8, V.UINT8, V.INT16, V.UINT16, V.INT32, V.UINT32]


def _png_bytes(tile_be, pt, w, h):
    """(h, rb) bytes as the filters see them (signed types flipped)."""
    a = np.frombuffer(tile_be, np.uint8).reshape(h, w * V.BPP[pt]).copy()
    if pt in (V.INT8, V.INT16):
        a[:, 0::V.BPP[pt]] ^= 0x80
    return a


def _triple_codes(a, bpp):
    """left << 16 | up << 8 | up-left of every byte with a left neighbour, rows 1.. of a tile
    (row 0's neighbours above are the zeros outside the tile), and the byte's column."""
    left = a[1:, :-bpp].astype(np.uint32)
    up = a[:-1, bpp:].astype(np.uint32)
    ul = a[:-1, :-bpp].astype(np.uint32)
    return (left << 16) | (up << 8) | ul


# ------------------------------------------------------------------------ Paeth triples

def test_de_bruijn_holds_every_pair_once():
    D = V.de_bruijn()
    assert D.shape == (65536,)
    pairs = D.astype(np.uint32) << 8 | np.roll(D, -1)
    assert np.array_equal(np.sort(pairs), np.arange(65536))


@pytest.mark.parametrize("W", [1024, 2048])
def test_paeth_plane_size_and_distinct_triples(W):
    """32 constants of uint8 rows: about 4 MiB, and on the constant rows exactly 32 x 65,536
    distinct (left, up, up-left) triples, every one with left = the row's constant."""
    plane = V.paeth_triples(1, W, 64, 96)
    assert 4.0 <= plane.nbytes / 2 ** 20 <= 4.5
    h = V.paeth_tile_rows(1, W)
    seen = []
    for k in range(32):
        t = plane[k * h:(k + 1) * h]
        const = np.flatnonzero((t == t[:, :1]).all(axis=1))
        assert len(const) == V.paeth_windows(1, W) and const.min() >= 1
        codes = (t[const, :-1].astype(np.uint32) << 16) | (t[const - 1, 1:].astype(np.uint32) << 8) | t[const - 1, :-1]
        u = np.unique(codes)
        assert (u >> 16 == 64 + k).all()
        seen.append(len(u))
    assert seen == [65536] * 32


@pytest.mark.parametrize("run", list(V.PAETH_RUNS))
def test_paeth_runs_cover_every_triple(run):
    """The union over a run's parametrised slices, cut into the tiles the GPU test requests and
    seen as the filters see them (int16: high bytes flipped), holds all 2^24 (left, up,
    up-left) triples -- for the four-shift runs in every byte lane (i mod 4) of a row, for
    16-bit samples in both byte planes.

    Measured: every run 16,777,216 of 16,777,216; f3_g1_u8 and f2_u8 16,777,216 in each of the
    four lanes; with shift 0 alone their lanes hold 4,227,109..4,243,751 each."""
    r = V.PAETH_RUNS[run]
    pt, bpp = r["pt"], V.BPP[r["pt"]]
    per_lane = len(r["shifts"]) == 4
    groups = 4 if per_lane else bpp
    seen = np.zeros((groups, 1 << 24), bool)
    for rn, shift, lo, hi in V.paeth_cases():
        if rn != run:
            continue
        plane, tiles = V.paeth_case(run, shift, lo, hi)
        assert len(tiles) == hi - lo
        for (x, y, w, h) in tiles:
            assert y % 2 == 0 and h % 2 == 0 and w * bpp == r["W"] and x * bpp == r["x0"]
            a = _png_bytes(V.cut(plane, x, y, w, h), pt, w, h)
            # a tile starts on a sequence row: its second row is the first constant row
            assert (a[1].reshape(-1, bpp) == a[1, :bpp]).all() and not (a[0] == a[0, 0]).all()
            codes = _triple_codes(a, bpp)
            for g in range(groups):
                seen[g, codes[:, (g - bpp) % groups::groups].ravel()] = True
        assert y + h == plane.shape[0]
    counts = seen.sum(axis=1)
    assert (counts == 1 << 24).all(), counts
    assert seen.any(axis=0).all()


# --------------------------------------------------------------------------------- ties

def _tie_stats(planes):
    st = {}
    for p in planes:
        for (x, y, w, h) in p["tiles"]:
            d = R.png_rows(V.cut(p["plane"], x, y, w, h), p["pt"], w, h, 5)
            e = st.setdefault(p["group"], dict(tiles=0, none=0, q_eq=0, rows=0, shared=0,
                                               win=np.zeros(5, int), rows16=0, shared16=0))
            s = d["sums"]
            shared = (s == s.min(axis=1, keepdims=True)).sum(axis=1) >= 2
            e["tiles"] += 1
            e["none"] += d["tile_none"]
            e["q_eq"] += d["q"][0] == d["q"][1]
            if w * V.BPP[p["pt"]] == 16:
                e["rows16"] += h
                e["shared16"] += int(shared.sum())
            if not d["tile_none"]:
                e["rows"] += h
                e["shared"] += int(shared.sum())
                e["win"] += np.bincount(s.argmin(axis=1)[shared], minlength=5)
    return st


@pytest.mark.parametrize("unstaged", [False, True])
def test_tie_tiles_tie(unstaged):
    """On every path that implements the adaptive choice -- k_filter3 (f3), k_filter2 (f2),
    k_filter from LDS (kf) and from the plane (kfw) -- the tie tiles hold, among the tiles the
    tile mode does not send to None, rows whose minimum sum is shared by two or more filters
    with the lowest of them None, Sub and Up; a tile with q0 == q1; tiles in the None mode and
    tiles not in it.  16-byte rows tie often.

    Measured (staged set; rows of tiles not in the None mode / of those with a shared
    minimum / lowest winner None, Sub, Up, Avg, Paeth):
      f3  1,362 tiles, 1,275 None mode, 58 q0 == q1: 719 / 244 / 15 66 154 9 0
      f2    684 tiles,   613 None mode, 29 q0 == q1: 554 / 196 / 26 72 98 0 0
      kf    684 tiles,   616 None mode, 35 q0 == q1: 465 / 158 / 17 43 96 2 0
      kfw   246 tiles,   146 None mode, 33 q0 == q1: 530 / 172 / 51 51 65 5 0
    16-byte rows (all tiles): 813 of 2,430 rows share their minimum (33 %)."""
    st = _tie_stats(V.tie_planes(unstaged))
    assert set(st) == {"f3", "f2", "kf", "kfw"}
    for g, e in st.items():
        assert e["win"][0] >= 1 and e["win"][1] >= 1 and e["win"][2] >= 1, (g, e)
        assert e["q_eq"] >= 1 and 1 <= e["none"] < e["tiles"], (g, e)
    assert 0.20 <= st["f3"]["shared16"] / st["f3"]["rows16"] <= 0.50, st["f3"]
    print({g: {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in e.items()} for g, e in st.items()})


def _paeth_variant(strict):
    """Paeth's predictor with `pa <= pc` or `pb <= pc` turned into `<`.  (`pa < pb` is the same
    function: pa == pb with left != up means up-left lies midway, pc == 0, and up-left wins
    either way.)"""
    def pred(l, u, ul):
        p = l + u - ul
        pa, pb, pc = abs(p - l), abs(p - u), abs(p - ul)
        ab = pa <= pb
        ac = pa < pc if strict == "ac" else pa <= pc
        bc = pb < pc if strict == "bc" else pb <= pc
        return np.where(ab & ac, l, np.where(bc, u, ul))
    return pred


@pytest.mark.parametrize("strict", ["ac", "bc"])
def test_tie_tiles_hang_on_paeth_order(strict):
    """The order of Paeth's comparisons decides rows of the tie tiles on every path, and tile
    modes: with `pa <= pc` or `pb <= pc` of the predictor turned into `<`, the adaptive choice
    differs on at least one row of each group, and at least one tile changes its mode.  (k_filter and
    k_adaptive_mode take their sums from a predictor of their own, filt_pred, which the
    fixed-filter runs over all triples never execute.)

    Measured, rows whose choice differs in f3 / f2 / kf / kfw, tiles whose mode differs:
      pa < pc: 7 / 8 / 5 / 7, 3;  pb < pc: 8 / 11 / 2 / 6, 5."""
    rows, modes = {}, 0
    for p in V.tie_planes():
        for (x, y, w, h) in p["tiles"]:
            t = V.cut(p["plane"], x, y, w, h)
            a = R.png_rows(t, p["pt"], w, h, 5)
            b = R.png_rows(t, p["pt"], w, h, 5, paeth=_paeth_variant(strict))
            modes += a["tile_none"] != b["tile_none"]
            if not a["tile_none"] and not b["tile_none"]:
                rows[p["group"]] = rows.get(p["group"], 0) + int((a["choice"] != b["choice"]).sum())
    print(strict, rows, modes)
    assert all(rows[g] >= 1 for g in ("f3", "f2", "kf", "kfw")) and modes >= 1


def test_tie_deterministic_tiles():
    """All zero: every sum 0, q0 == q1, None mode.  Rows equal to the row above: not None mode,
    row 0 ties None with Up and Sub with Paeth, later rows take Up.  One constant byte: Up
    leaves zeros on the middle row, q0 == q1, None mode."""
    det = [p for p in V.tie_planes() if p["name"].startswith("det_")]
    assert len(det) == 8
    for p in det:
        for (x, y, w, h) in p["tiles"]:
            d = R.png_rows(V.cut(p["plane"], x, y, w, h), p["pt"], w, h, 5)
            blk = y // V.DET_H
            if blk == 0:
                assert not d["sums"].any() and d["tile_none"] and d["q"][0] == d["q"][1]
            elif blk == 1:
                s = d["sums"]
                assert not d["tile_none"]
                assert s[0, 0] == s[0, 2] and s[0, 1] == s[0, 4] and (d["choice"][1:] == 2).all()
            else:
                assert d["tile_none"] and d["q"][0] == d["q"][1] and d["sums"][1:, 2].max() == 0


# --------------------------------------------------------------- oracle against numpy

def _check_streams(oracle, tile_be, pt, w, h, filters=range(6)):
    tb = np.frombuffer(tile_be, np.uint8)
    for f in filters:
        assert oracle.png_filter_stream(tb, pt, w, h, f).tobytes() == R.png_stream(tile_be, pt, w, h, f), \
            (pt, w, h, f)
    assert oracle.adaptive_tile_none(tb, pt, w, h) == R.png_rows(tile_be, pt, w, h, 5)["tile_none"]


@pytest.mark.parametrize("pt", V.PNG_TYPES)
def test_oracle_png_stream_equals_numpy(oracle, pt):
    """oracle.png_filter_stream (the GPU tests' second reference) equals the restatement from
    the PNG specification for filters 0..5 on random bits and extremes."""
    for (w, h) in [(1, 1), (2, 1), (1, 5), (16, 13), (67, 23), (301, 48)]:
        for plane in (V.random_bits(pt, w, h, 3), V.extremes(pt, w, h)):
            _check_streams(oracle, plane.tobytes(), pt, w, h)


def test_oracle_png_stream_equals_numpy_on_ties(oracle):
    for p in V.tie_planes(True):
        for (x, y, w, h) in p["tiles"]:
            _check_streams(oracle, V.cut(p["plane"], x, y, w, h), p["pt"], w, h, (5,))
    for p in V.tie_planes()[:3]:
        for (x, y, w, h) in p["tiles"][::7]:
            _check_streams(oracle, V.cut(p["plane"], x, y, w, h), p["pt"], w, h)


@pytest.mark.parametrize("run", ["f3_g1_u8", "f3_g1_i16"])
def test_oracle_png_stream_equals_numpy_on_paeth_slice(oracle, run):
    lo, hi = V.paeth_slices(run)[5]
    plane, tiles = V.paeth_case(run, 0, lo, hi)
    pt = V.PAETH_RUNS[run]["pt"]
    for k, (x, y, w, h) in enumerate(tiles):
        _check_streams(oracle, V.cut(plane, x, y, w, h), pt, w, h, range(6) if k == 0 else (4, 5))
        # the adaptive option must reach the per-row choice on these tiles
        assert not R.png_rows(V.cut(plane, x, y, w, h), pt, w, h, 5)["tile_none"]


@pytest.mark.parametrize("run", list(V.PAETH_RUNS))
def test_paeth_tiles_keep_the_adaptive_choice(oracle, run):
    """No tile of any slice goes to the tile mode None (there the Paeth sums would go unused)."""
    pt = V.PAETH_RUNS[run]["pt"]
    for rn, shift, lo, hi in V.paeth_cases():
        if rn == run and shift == 0:
            plane, tiles = V.paeth_case(run, shift, lo, hi)
            for (x, y, w, h) in tiles:
                assert not oracle.adaptive_tile_none(np.frombuffer(V.cut(plane, x, y, w, h), np.uint8), pt, w, h)


# -------------------------------------------------------------------------- the pyramid

def _cells(plane):
    sy, sx = plane.shape
    return plane.reshape(sy // 2, 2, sx // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)


def _exact_downsample(a):
    """floor((sum + 2) / 4) of every 2x2 box in Python integers; edges repeated."""
    o = a.astype(object)
    if o.shape[1] % 2:
        o = np.concatenate([o, o[:, -1:]], axis=1)
    if o.shape[0] % 2:
        o = np.concatenate([o, o[-1:, :]], axis=0)
    s = o[0::2, 0::2] + o[0::2, 1::2] + o[1::2, 0::2] + o[1::2, 1::2]
    return s, np.vectorize(lambda v: (v + 2) // 4, otypes=[object])(s)


@pytest.mark.parametrize("pt", INT_TYPES)
def test_extremes_integer_cells_and_exact_pyramid(pt):
    """The full `extremes` plane holds every combination of the value list in a 2x2 cell, the
    all-min and all-max cells, and every residue mod 4 of the cell sum with a negative and
    with a positive sum (signed types; unsigned: with sums below and above 2^32 for uint32);
    _numpy_ref.downsample equals exact integer arithmetic on it, level after level, and on
    the small shapes and random bits."""
    sx, sy = V.extremes_full_shape(pt)
    plane = V.extremes(pt, sx, sy)
    vals = V.extreme_values(pt).astype(object)
    n = len(vals)
    cells = _cells(plane).astype(object)
    assert len({tuple(c) for c in cells.tolist()}) == n ** 4
    s, _ = _exact_downsample(plane)
    sums = np.array(s.ravel().tolist(), dtype=object)
    assert 4 * min(vals) in sums and 4 * max(vals) in sums
    for res in range(4):
        if pt in (V.INT8, V.INT16, V.INT32):
            assert any(v % 4 == res and v < 0 for v in sums) and any(v % 4 == res and v > 0 for v in sums)
        else:
            assert any(v % 4 == res for v in sums)
    if pt in (V.INT32, V.UINT32):  # sums a 32-bit accumulator cannot hold
        assert any(not -(1 << 31) <= v + 2 < (1 << 32) for v in sums)
    planes = [plane, V.random_bits(pt, 67, 23, 1)]
    planes += [V.extremes(pt, w, h, start=k) for k, (w, h) in enumerate(V.pyramid_shapes(pt))]
    for a in planes:
        while a.shape != (1, 1):
            _, want = _exact_downsample(a)
            a = R.downsample(a)
            assert a.astype(object).tolist() == want.tolist()


@pytest.mark.parametrize("pt", [V.FLOAT, V.DOUBLE])
def test_extremes_float_cells(pt):
    """The full plane holds all 15^4 cells and the required ones; cells of four denormals whose
    exact sum is 4 k + 2 units of the smallest denormal (sum * 0.25 is a round-to-even tie); the
    small shapes start with the required cells.  The reference's NaNs at level 1 are exactly the
    listed NaN cells.

    Measured (float and double alike): 50,625 distinct cells, 128 four-denormal tie cells,
    14,401 listed NaN cells."""
    sx, sy = V.extremes_full_shape(pt)
    plane = V.extremes(pt, sx, sy)
    ut = ">u%d" % V.BPP[pt]
    vals = V.extreme_values(pt).view(ut)
    bits = _cells(plane.view(ut))
    idx = np.searchsorted(np.sort(vals), bits)
    idx = np.argsort(vals)[idx]                       # value-list positions of every cell
    assert np.array_equal(vals[idx], bits)
    have = {tuple(c) for c in idx.tolist()}
    assert len(vals) == 15 and len(have) == 15 ** 4
    for c in V.required_cells(pt):
        assert tuple(c) in have
    # denormal ties, in units of the smallest denormal (exact integers)
    D = int(vals[V._F["pD"]])
    unit = {V._F["pd"]: 1, V._F["nd"]: -1, V._F["pD"]: D, V._F["nD"]: -D}
    ties = [c for c in have if all(v in unit for v in c) and sum(unit[v] for v in c) % 4 == 2]
    assert len(ties) >= 4
    print("four-denormal tie cells:", len(ties))
    with np.errstate(all="ignore"):
        ref = R.downsample(plane)
    assert np.array_equal(np.isnan(ref), V.nan_cells_listed(plane))
    # the documented results of the required cells: overflow, cancellation, -0, inf - inf, ties
    small = V.extremes(pt, 16, 2)
    with np.errstate(all="ignore"):
        got = R.downsample(small)[0].astype(small.dtype.newbyteorder("="))
    ev = V.extreme_values(pt).astype(got.dtype)
    d, Dn = ev[V._F["pd"]], ev[V._F["pD"]]
    assert got[0] == np.inf and got[1] == 0 and not np.signbit(got[1])
    assert got[2] == 0 and np.signbit(got[2]) and np.isnan(got[3])
    # (3 D + d) / 4 = 3 * 2^(m-2) - 1/2 units: the even neighbour is 3 * 2^(m-2)
    assert got[4] == (3 * ((D + 1) // 4)) * d and got[5] == 0 and got[6] == -got[4]
    assert got[7] == (D + 1) // 2 * d and Dn == D * d


@pytest.mark.parametrize("pt", [V.FLOAT, V.DOUBLE])
def test_random_bits_nan_share(pt):
    """Level 1 of uniform random bits is NaN where a cell holds a NaN (float: an all-ones
    exponent with a non-zero mantissa, 1 sample in 256, so about 1.6 % of the cells; double: 1 in
    2,048, about 0.2 %) or opposite infinities: well under the 5 % the GPU test may exclude.

    Measured on 301 x 97 (7,399 outputs): float 1.51 %, double 0.19 %; over the small shapes
    float 1 of 70 outputs, double 0 of 36."""
    a = V.random_bits(pt, 301, 97, 11)
    with np.errstate(all="ignore"):
        share = np.isnan(R.downsample(a)).mean()
    print("NaN share", share)
    assert share <= 0.05
    assert (0.010 <= share <= 0.025) if pt == V.FLOAT else (0.0005 <= share <= 0.005)
    n = tot = 0
    for k, (w, h) in enumerate(V.pyramid_shapes(pt)):
        with np.errstate(all="ignore"):
            lvl = R.downsample(V.random_bits(pt, w, h, 20 + k))
        n, tot = n + int(np.isnan(lvl).sum()), tot + lvl.size
    print("small shapes:", n, "of", tot)
    assert n <= 0.05 * tot
