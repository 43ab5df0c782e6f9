"""Zarr chunk rows decoded on demand into the bands of a sparse plane (pbx_band_write_zarr).

Expected bytes are the numpy plane the chunks were encoded from, and the responses of the same
chunks registered whole (pbx_plane_register_zarr) under another image id; both comparisons
are byte-exact.
"""
import itertools
import json
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _zarr
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(1200000)  # disjoint from the other test files (shared service)
PT = {"i1": 0, "u1": 1, "i2": 2, "u2": 3, "i4": 4, "u4": 5, "f4": 6, "f8": 7}
H, W = 300, 500

CODECS = {
    "raw": (None, {}),
    "zlib": ("zlib", {"level": 1}),
    "blosc-lz4": ("blosc", {"codec": "lz4", "clevel": 5, "shuffle": True}),
    "blosc-bitshuffle": ("blosc", {"cname": "lz4", "clevel": 5, "shuffle": 2}),  # c-blosc writes it
    "blosc-zstd": ("blosc", {"cname": "zstd", "clevel": 5, "shuffle": 1}),
}


def be_bytes(a):
    """A region as the tiles carry it: packed big-endian samples."""
    return np.ascontiguousarray(a).astype(a.dtype.newbyteorder(">")).tobytes()


def make_plane(dtype, seed):
    plane = _zarr.noise_plane(H, W, dtype, seed=seed)
    if np.dtype(dtype).kind == "f":
        plane = (plane.astype(np.float64) * 0.25 - 300.0).astype(dtype)
    return plane


def covering(chunks, gx, cy, y0, rows):
    """The chunk rows of a whole-plane chunk list that cover rows [y0, y0 + rows)."""
    return chunks[(y0 // cy) * gx:-(-(y0 + rows) // cy) * gx]


def load_band(svc, pid, k, B, sy, chunks, gx, cx, cy, comp, fill_bits=0):
    r0, r1 = k * B, min((k + 1) * B, sy)
    svc.band_write_zarr(pid, r0, r1 - r0, cx, cy, comp, covering(chunks, gx, cy, r0, r1 - r0), fill_bits)


def tile_requests(iid, B, dtype):
    """Full-width raw tiles per band, tiles straddling every band boundary (odd x), and a PNG
    (8- and 16-bit types) and a TIFF tile over the first boundary."""
    bounds = list(range(B, H, B))
    reqs = [pbx.TileCtx(iid, 0, 0, 0, 0, lo, W, min(lo + B, H) - lo) for lo in range(0, H, B)]
    reqs += [pbx.TileCtx(iid, 0, 0, 0, 3, b - 7, 333, 15) for b in bounds]
    reqs += [pbx.TileCtx(iid, 0, 0, 0, W - 101, b - 1, 101, 2) for b in bounds]
    y = bounds[0] - 20 if bounds else 130
    if np.dtype(dtype).itemsize <= 2:
        reqs.append(pbx.TileCtx(iid, 0, 0, 0, 16, y, 256, 48, format="png"))
    reqs.append(pbx.TileCtx(iid, 0, 0, 0, 5, y, 200, 41, format="tif"))
    return reqs


def check_pixels(oracle, plane, tc, body):
    ref = be_bytes(plane[tc.y:tc.y + tc.h, tc.x:tc.x + tc.w])
    if tc.format is None:
        assert body == ref, (tc.x, tc.y, tc.w, tc.h)
    elif tc.format == "png":
        r, px, _ = oracle.png_decode(body)
        assert r == 0 and px == ref, (tc.x, tc.y, tc.w, tc.h)
    else:
        r, px, _ = oracle.tiff_decode(body, len(ref))
        assert r == 0 and px == ref, (tc.x, tc.y, tc.w, tc.h)


_whole = {}


def whole_reference(service, chunk, dtype, codec):
    """The plane, its chunks and the whole-plane registration of them: made once per
    (chunk shape, dtype, codec) and shared by the band_rows cases; the registered plane stays
    for the session (300 x 500 samples)."""
    key = (chunk, dtype, codec)
    if key not in _whole:
        comp, kw = CODECS[codec]
        cy, cx = chunk
        plane = make_plane(dtype, seed=cy + len(dtype) + len(codec))
        chunks = _zarr.encode_chunks(plane, cy, cx, comp, **kw)
        dt = np.dtype(dtype)
        iid = next(_ids)
        service.register_zarr_plane(iid, 0, 0, 0, PT[dt.str[1:]], W, H, cx, cy, comp, chunks,
                                    big_endian=dt.str[0] != "<")
        _whole[key] = (plane, chunks, iid, {})
    return _whole[key]


@pytest.mark.parametrize("B", [64, 100, 300])
@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("dtype", ["u1", ">u2", "<i4", ">f8"])
@pytest.mark.parametrize("chunk", [(64, 128), (48, 100)], ids=["64x128", "48x100"])
def test_parity_with_whole_plane_registration(service, oracle, chunk, dtype, codec, B):
    if "cname" in CODECS[codec][1] and _zarr.cblosc() is None:
        pytest.skip("c-blosc 1.21 library not in this image")
    comp = CODECS[codec][0]
    cy, cx = chunk
    gx = -(-W // cx)
    dt = np.dtype(dtype)
    plane, chunks, whole_iid, answers = whole_reference(service, chunk, dtype, codec)
    iid = next(_ids)
    pid = service.create_sparse_plane(iid, 0, 0, 0, PT[dt.str[1:]], W, H, B, big_endian=dt.str[0] != "<")
    try:
        nb = -(-H // B)
        order = list(np.random.default_rng(B + cy).permutation(nb))
        for n, k in enumerate(order):
            assert service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, int(k) * B, 8, 1))[0] == pbx.E_NOT_RESIDENT
            load_band(service, pid, int(k), B, H, chunks, gx, cx, cy, comp)
            states = service.band_info(pid)[1]
            assert sorted(j for j, s in enumerate(states) if s == pbx.BS_READY) == sorted(int(j) for j in order[:n + 1])
        reqs = tile_requests(iid, B, dtype)
        got = service.get_tiles(reqs)
        if B not in answers:
            answers[B] = service.get_tiles(tile_requests(whole_iid, B, dtype))
        for tc, (st, body), (wst, wbody) in zip(reqs, got, answers[B]):
            assert st == pbx.OK and wst == pbx.OK
            assert body == wbody, (tc.format, tc.x, tc.y, tc.w, tc.h)
            check_pixels(oracle, plane, tc, body)
    finally:
        service.release_plane(pid)


@pytest.mark.parametrize("dtype,codec", [(">u2", "blosc-lz4"), ("u1", "zlib"), (">f8", "raw"),
                                         ("<i4", "blosc-bitshuffle")])
def test_rows_outside_the_window_are_not_written(service, dtype, codec):
    """Bands of 100 rows over chunk rows of 64, each written in three pieces at rows that are no
    chunk boundaries, the middle one 5 rows inside one 16-row block, and every piece encoded
    from a different plane: each served row comes from the piece whose window held it, in
    whatever order the pieces arrive."""
    if "cname" in CODECS[codec][1] and _zarr.cblosc() is None:
        pytest.skip("c-blosc 1.21 library not in this image")
    comp, kw = CODECS[codec]
    cy, cx, B = 64, 128, 100
    gx = -(-W // cx)
    dt = np.dtype(dtype)
    planes = [make_plane(dtype, seed=70 + n) for n in range(3)]
    chunks = [_zarr.encode_chunks(p, cy, cx, comp, **kw) for p in planes]
    iid = next(_ids)
    pid = service.create_sparse_plane(iid, 0, 0, 0, PT[dt.str[1:]], W, H, B, big_endian=dt.str[0] != "<")
    try:
        # band 1: rows 100..200 (chunk row 2 starts at 128: rows 137..141 lie in its first
        # 16-row block); band 2: rows 200..300 (chunk row 3 starts at 192: 233..237 in its third)
        for band, pieces, order in [(1, [(100, 37), (137, 5), (142, 58)], (0, 1, 2)),
                                    (2, [(200, 33), (233, 5), (238, 62)], (2, 1, 0))]:
            for n, j in enumerate(order):
                y0, rows = pieces[j]
                assert service.band_info(pid)[1][band] == (pbx.BS_LOADING if n else pbx.BS_ABSENT)
                service.band_write_zarr(pid, y0, rows, cx, cy, comp, covering(chunks[j], gx, cy, y0, rows))
            assert service.band_info(pid)[1][band] == pbx.BS_READY
            want = np.concatenate([planes[j][y0:y0 + rows] for j, (y0, rows) in enumerate(pieces)])
            st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, band * B, W, B))
            assert st == pbx.OK
            got = np.frombuffer(body, dt.newbyteorder(">")).reshape(B, W)
            bad = np.nonzero((got.view(np.uint8) != want.astype(got.dtype).view(np.uint8)).any(axis=1))[0]
            assert bad.size == 0, "rows %s of band %d hold another piece's bytes" % (bad[:8] + band * B, band)
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_READY, pbx.BS_READY]
    finally:
        service.release_plane(pid)


@pytest.mark.parametrize("dtype", ["<u2", ">u2", "u1", ">f8", "<f8"])
def test_missing_chunks_take_the_fill_value(service, dtype):
    """Absent chunks (None and b"") of a band read as fill_value in the plane's byte order, in
    the 16-byte group body (aligned chunks), the sample body (100-column chunks, 8-byte
    samples) and rows cut by the band window."""
    dt = np.dtype(dtype)
    cy, cx, B = 48, 100, 100
    gx = -(-W // cx)
    plane = make_plane(dtype, seed=9)
    chunks = _zarr.encode_chunks(plane, cy, cx, "zlib")
    fill_val = np.array([0x1234 % (1 << (8 * min(dt.itemsize, 2))) if dt.kind != "f" else -7.25],
                        dtype=dt.newbyteorder("="))
    fill_bits = int(fill_val.view("u%d" % dt.itemsize)[0])
    want = plane.copy()
    for k, blank in ((2, None), (gx + 4, b""), (2 * gx, None), (6 * gx + 4, None)):
        chunks[k] = blank
        j, i = divmod(k, gx)
        want[j * cy:(j + 1) * cy, i * cx:(i + 1) * cx] = fill_val[0]
    iid, wid = next(_ids), next(_ids)
    pid = service.create_sparse_plane(iid, 0, 0, 0, PT[dt.str[1:]], W, H, B, big_endian=dt.str[0] != "<")
    whole = service.register_zarr_plane(wid, 0, 0, 0, PT[dt.str[1:]], W, H, cx, cy, "zlib", chunks,
                                        big_endian=dt.str[0] != "<", fill_bits=fill_bits)
    try:
        for k in (2, 0, 1):
            load_band(service, pid, k, B, H, chunks, gx, cx, cy, "zlib", fill_bits)
        for k in range(3):
            st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, k * B, W, B))
            wst, wbody = service.get_tile(pbx.TileCtx(wid, 0, 0, 0, 0, k * B, W, B))
            assert st == pbx.OK and wst == pbx.OK
            assert body == wbody == be_bytes(want[k * B:(k + 1) * B])
    finally:
        service.release_plane(pid)
        service.release_plane(whole)


def _damaged(codec, damage, chunk):
    c = bytearray(chunk)
    if damage == "truncate":
        return bytes(c[:len(c) // 2])
    if codec == "blosc":  # as test_gpu_corrupt_chunk_is_400: LZ4 sequences inside the first split
        for k in range(40, min(len(c), 400), 7):
            c[k] ^= 0xA5
    else:                 # as test_gpu_corrupt_zlib_is_400
        for k in range(20, 200, 5):
            c[k] ^= 0x3C
    return bytes(c)


@pytest.mark.parametrize("damage", ["truncate", "flip"])
@pytest.mark.parametrize("codec", ["zlib", "blosc"])
def test_corrupt_chunk_fails_the_band_load(service, codec, damage):
    """A damaged chunk answers 400; the band reads absent, its HBM is returned, and a clean
    reload serves exact tiles -- for a band written in one piece and for one that already held
    rows of an earlier piece."""
    h = w = 256
    plane = _zarr.noise_plane(h, w, ">u2", seed=1)
    kw = {"level": 6} if codec == "zlib" else {}
    good = _zarr.encode_chunks(plane, 128, 128, codec, **kw)
    bad = list(good)
    bad[2] = _damaged(codec, damage, good[2])
    iid = next(_ids)
    pid = service.create_sparse_plane(iid, 0, 0, 0, pbx.UINT16, w, h, 128)
    try:
        base = service.residency_stats()["resident_bytes"]
        for first in (None, (128, 16)):
            if first is not None:  # rows 128..143 are in: the load is under way
                service.band_write_zarr(pid, first[0], first[1], 128, 128, codec, good[2:4])
                assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_LOADING]
                assert service.residency_stats()["resident_bytes"] > base
            with pytest.raises(pbx.PbxError) as ei:
                service.band_write_zarr(pid, 128, 128, 128, 128, codec, bad[2:4])
            assert ei.value.status == 400
            if first is None or not (codec == "blosc" and damage == "truncate"):
                # (a truncated blosc frame is refused by the host plan: the load it did not
                # join goes on, see test_bad_arguments_leave_a_half_loaded_band_alone)
                assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_ABSENT]
                assert service.residency_stats()["resident_bytes"] == base
            else:
                service.band_abort(pid, 128)
            assert service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 128, 64, 64))[0] == pbx.E_NOT_RESIDENT
        service.band_write_zarr(pid, 128, 128, 128, 128, codec, good[2:4])
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_READY]
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 128, w, 128))
        assert st == pbx.OK and body == plane[128:].tobytes()
    finally:
        service.release_plane(pid)


def test_bad_arguments_leave_a_half_loaded_band_alone(service):
    """Input the host can refuse (offsets, blosc headers, codec, chunk shape, rows that leave the
    band, a plane that is not sparse) is 400 and does not join the load: the band stays loading
    with the rows it has, and the remaining rows complete it.  A resident band is 409.  The
    band-write failure hook counts these writes too."""
    h = w = 256
    plane = _zarr.noise_plane(h, w, ">u2", seed=6)
    good = _zarr.encode_chunks(plane, 128, 128, "blosc")
    iid, wid = next(_ids), next(_ids)
    pid = service.create_sparse_plane(iid, 0, 0, 0, pbx.UINT16, w, h, 128)
    whole = service.register_zarr_plane(wid, 0, 0, 0, pbx.UINT16, w, h, 128, 128, "blosc", good)
    try:
        service.band_write_zarr(pid, 128, 40, 128, 128, "blosc", good[2:4])
        used = service.residency_stats()["resident_bytes"]

        def refused(*a, **kw):
            with pytest.raises(pbx.PbxError) as ei:
                service.band_write_zarr(*a, **kw)
            assert ei.value.status == 400, ei.value
            assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_LOADING]
            assert service.residency_stats()["resident_bytes"] == used

        data, offsets = pbx.pack_chunks(good[2:4])
        backwards = offsets.copy()
        backwards[0], backwards[1] = 5, 3                   # chunk 0 would have a negative length
        refused(pid, 168, 88, 128, 128, "blosc", (data, backwards))
        beyond = offsets.copy()
        beyond[1] = offsets[2] + 100                        # past the end of the data
        refused(pid, 168, 88, 128, 128, "blosc", (data, beyond))
        hdr = bytearray(good[3])
        hdr[16:20] = (len(hdr) + 100).to_bytes(4, "little")  # block start outside the frame
        refused(pid, 168, 88, 128, 128, "blosc", [good[2], bytes(hdr)])
        hdr = bytearray(good[2])
        hdr[0] = 3                                          # a blosc2-era format version
        refused(pid, 168, 88, 128, 128, "blosc", [bytes(hdr), good[3]])
        refused(pid, 168, 88, 128, 128, "blosc", [good[2][:10], good[3]])
        refused(pid, 168, 88, 128, 0, "blosc", good[2:4])   # chunk shape
        refused(pid, 100, 60, 128, 128, "blosc", good[0:4])   # rows cross the end of band 0
        refused(pid, 250, 10, 128, 128, "blosc", good[2:4])   # ... and of the plane
        refused(pid, 168, 0, 128, 128, "blosc", good[2:4])
        refused(whole, 128, 128, 128, 128, "blosc", good[2:4])  # not a sparse plane
        with pytest.raises(pbx.PbxError) as ei:
            service.band_write_zarr(pid + 12345, 128, 128, 128, 128, "blosc", good[2:4])
        assert ei.value.status == pbx.E_NOTFOUND
        # raw rows and Zarr pieces mix within one load
        service.band_write(pid, 168, 8, plane[168:176].tobytes())
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_LOADING]
        service.band_write_zarr(pid, 176, 80, 128, 128, "blosc", good[2:4])
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_READY]
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 128, w, 128))
        assert st == pbx.OK and body == plane[128:].tobytes()
        for y0, rows in ((128, 128), (200, 8)):
            with pytest.raises(pbx.PbxError) as ei:
                service.band_write_zarr(pid, y0, rows, 128, 128, "blosc", good[2:4])
            assert ei.value.status == pbx.E_EXISTS
        # the injected upload failure counts Zarr writes: the load fails, the band is given back
        base = service.residency_stats()["resident_bytes"]
        service.band_write_zarr(pid, 0, 64, 128, 128, "blosc", good[0:2])
        service.test_fail_band_write(1)
        with pytest.raises(pbx.PbxError) as ei:
            service.band_write_zarr(pid, 64, 64, 128, 128, "blosc", good[0:2])
        assert ei.value.status == pbx.E_INTERNAL
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_READY]
        assert service.residency_stats()["resident_bytes"] == base
        service.band_write_zarr(pid, 0, 128, 128, 128, "blosc", good[0:2])
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 0, w, h))
        assert st == pbx.OK and body == plane.tobytes()
    finally:
        service.test_fail_band_write(0)
        service.release_plane(pid)
        service.release_plane(whole)


# ------------------------------------------------------------ on demand through the handler
SY, SX, CH, BAND = 2048, 1024, 256, 512


def _write_level(root, plane, sep):
    root.mkdir(parents=True)
    h, w = plane.shape
    meta = {"zarr_format": 2, "shape": [1, 1, 1, h, w], "chunks": [1, 1, 1, CH, CH], "dtype": ">u2",
            "order": "C", "fill_value": 0, "filters": None, "dimension_separator": sep,
            "compressor": {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}}
    (root / ".zarray").write_text(json.dumps(meta))
    gx = -(-w // CH)
    for k, ch in enumerate(_zarr.encode_chunks(plane, CH, CH, "blosc")):
        j, i = divmod(k, gx)
        path = root / sep.join(str(v) for v in (0, 0, 0, j, i))
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_bytes(ch)


@pytest.fixture(scope="module")
def slides(tmp_path_factory):
    """One two-level NGFF image per dimension separator: {sep: (directory, [level planes])}."""
    out = {}
    for sep, name in (("/", "slash"), (".", "dot")):
        root = tmp_path_factory.mktemp("ngff_" + name) / "img"
        root.mkdir()
        levels = [_zarr.noise_plane(SY, SX, ">u2", seed=21), _zarr.noise_plane(SY // 2, SX // 2, ">u2", seed=22)]
        for k, p in enumerate(levels):
            _write_level(root / str(k), p, sep)
        (root / ".zattrs").write_text(json.dumps({"multiscales": [{
            "version": "0.4", "axes": [{"name": a} for a in "tczyx"],
            "datasets": [{"path": "0"}, {"path": "1"}]}]}))
        out[sep] = (str(root), levels)
    return out


@pytest.fixture
def opened(monkeypatch):
    """The chunk files pbx reads, as (level directory name, chunk row, chunk column)."""
    seen, lock, real = [], threading.Lock(), pbx._read_chunk_file

    def spy(path):
        adir, name = path.split(os.sep + "img" + os.sep)[1].split(os.sep, 1)
        idx = [int(v) for v in name.replace(os.sep, ".").split(".")]
        with lock:
            seen.append((adir, idx[-2], idx[-1]))
        return real(path)
    monkeypatch.setattr(pbx, "_read_chunk_file", spy)
    return seen


def band_files(level, k, gx=SX // CH, per_band=BAND // CH):
    return sorted((str(level), j, i) for j in range(k * per_band, (k + 1) * per_band) for i in range(gx))


def serve(oracle, svc, src, plane, tc):
    body = pbx.TileRequestHandler(svc, tc, src).get_tile()
    assert body is not None
    check_pixels(oracle, plane, tc, body)
    return body


@pytest.mark.parametrize("sep", ["/", "."], ids=["slash", "dot"])
def test_cold_tile_reads_its_band_only(oracle, slides, opened, sep):
    root, (full, _) = slides[sep]
    iid = next(_ids)
    src = pbx.NgffSource({iid: root})
    with pbx.PixelsService(sparse_band_rows=BAND) as svc:
        serve(oracle, svc, src, full, pbx.TileCtx(iid, 0, 0, 0, 300, 1100, 256, 256))  # band 2
        assert sorted(opened) == band_files(0, 2) and len(opened) == 2 * 4
        s = svc.residency_stats()
        assert s["bands"] == 1 and s["planes"] == 0 and s["resident_bytes"] == BAND * SX * 2 + 256
        serve(oracle, svc, src, full, pbx.TileCtx(iid, 0, 0, 0, 300, 1100, 256, 256, format="png"))
        assert len(opened) == 8
        # rows 1500..1599 straddle bands 2 and 3: only band 3 is read
        serve(oracle, svc, src, full, pbx.TileCtx(iid, 0, 0, 0, 7, 1500, 333, 100))
        serve(oracle, svc, src, full, pbx.TileCtx(iid, 0, 0, 0, 512, 1500, 256, 100, format="png"))
        assert sorted(opened[8:]) == band_files(0, 3)
        pid = svc.lookup_plane(iid, 0, 0, 0)[0]
        assert svc.band_info(pid)[1] == [pbx.BS_ABSENT, pbx.BS_ABSENT, pbx.BS_READY, pbx.BS_READY]
        assert pbx.TileRequestHandler(svc, pbx.TileCtx(iid + 1, 0, 0, 0, 0, 0, 8, 8), src).get_tile() is None


def test_concurrent_requests_read_a_band_once(oracle, slides, opened):
    root, (full, _) = slides["/"]
    iid = next(_ids)
    src = pbx.NgffSource({iid: root})
    ctxs = [pbx.TileCtx(iid, 0, 0, 0, 96 * n, 520 + 30 * n, 256, 256, format=[None, "png"][n % 2])
            for n in range(8)]  # all inside band 1
    with pbx.PixelsService(sparse_band_rows=BAND) as svc:
        barrier = threading.Barrier(8)

        def worker(tc):
            barrier.wait()
            return pbx.TileRequestHandler(svc, tc, src).get_tile()

        with ThreadPoolExecutor(8) as ex:
            bodies = list(ex.map(worker, ctxs))
        for tc, body in zip(ctxs, bodies):
            check_pixels(oracle, full, tc, body)
        assert sorted(opened) == band_files(0, 1)
        assert svc.residency_stats()["bands"] == 1


def test_evicted_band_is_decoded_again(oracle, slides, opened):
    root, (full, _) = slides["."]
    iid = next(_ids)
    src = pbx.NgffSource({iid: root})
    with pbx.PixelsService(sparse_band_rows=BAND) as svc:
        svc.set_residency_budget(2 * (BAND * SX * 2 + 256) + 1000)
        for n, k in enumerate([0, 1, 2, 0]):
            serve(oracle, svc, src, full, pbx.TileCtx(iid, 0, 0, 0, 128, k * BAND + 100, 512, 300, format="png"))
            assert sorted(opened[8 * n:]) == band_files(0, k)
            s = svc.residency_stats()
            assert s["resident_bytes"] <= s["budget"] and s["bands"] == min(n + 1, 2)
        assert svc.residency_stats()["band_evictions"] == 2
        pid = svc.lookup_plane(iid, 0, 0, 0)[0]
        assert svc.band_info(pid)[1] == [pbx.BS_READY, pbx.BS_ABSENT, pbx.BS_READY, pbx.BS_ABSENT]


def test_lower_level_in_omero_numbering(oracle, slides, opened):
    """resolution 0 is the smallest stored level (dataset 1), resolution 1 and an absent
    resolution the full one."""
    root, (full, half) = slides["."]
    iid = next(_ids)
    src = pbx.NgffSource({iid: root})
    with pbx.PixelsService(sparse_band_rows=BAND) as svc:
        tc = pbx.TileCtx(iid, 0, 0, 0, 100, 600, 300, 200, resolution=0)  # band 1 of 1024 x 512
        body = pbx.TileRequestHandler(svc, tc, src).get_tile()
        assert body == half[600:800, 100:400].tobytes()
        assert sorted(opened) == band_files(1, 1, gx=2)
        tc = pbx.TileCtx(iid, 0, 0, 0, 100, 600, 300, 200, resolution=1)
        body = pbx.TileRequestHandler(svc, tc, src).get_tile()
        assert body == full[600:800, 100:400].tobytes()
        assert sorted(opened[4:]) == band_files(0, 1)


def test_ngff_source_needs_sparse_bands(slides):
    root, _ = slides["/"]
    iid = next(_ids)
    with pbx.PixelsService() as svc:
        with pytest.raises(pbx.PbxError) as ei:
            pbx.TileRequestHandler(svc, pbx.TileCtx(iid, 0, 0, 0, 0, 0, 64, 64), pbx.NgffSource({iid: root})).get_tile()
        assert ei.value.status == pbx.E_BADARG and "sparse_band_rows" in str(ei.value)
