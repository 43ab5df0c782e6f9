"""Zarr chunks that hold more than one plane (pbx_planes_register_zarr_deep,
pbx_band_write_zarr_deep), on the GPU.

Every expected plane is a numpy slice of the 5-D array the chunks were cut from (with the fill
value where a chunk file is absent); comparisons are byte-exact.  Planes are 100 x 70 at most.
"""
import itertools
import json
import os
import threading

import numpy as np
import pytest

import _zarr
import _zarr_deep as ZD
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(1500000)  # disjoint from the other test files (shared service)
PT = {"i1": 0, "u1": 1, "i2": 2, "u2": 3, "i4": 4, "u4": 5, "f4": 6, "f8": 7}
SHAPE = (1, 2, 5, 70, 100)
H, W = SHAPE[-2:]

# explicit blosc block sizes: 4,096 and 1,024 bytes divide no slice of 40 x 72 or 40 x 36
# samples times 1, 2, 4 or 8 bytes evenly for every dtype, so blocks straddle slices, and the
# chunk ends in a leftover block
CODECS = {
    "raw": (None, {}),
    "zlib": ("zlib", {"level": 1}),
    "lz4-shuffle-4096": ("blosc", {"codec": "lz4", "shuffle": True, "blocksize": 4096}),
    "lz4-shuffle-1024": ("blosc", {"codec": "lz4", "shuffle": True, "blocksize": 1024}),
    "lz4-noshuffle": ("blosc", {"codec": "lz4", "shuffle": False, "blocksize": 4096}),
    "lz4-nosplit": ("blosc", {"codec": "lz4", "shuffle": True, "blocksize": 4096, "split": False}),
    "zstd": ("blosc", {"codec": "zstd", "shuffle": True, "blocksize": 4096}),
    "blosc-zlib": ("blosc", {"codec": "zlib", "shuffle": True, "blocksize": 1024}),
    "blosclz": ("blosc", {"cname": "blosclz", "clevel": 5, "shuffle": 1, "blocksize": 4096}),  # c-blosc
    "bitshuffle-4096": ("blosc", {"cname": "lz4", "clevel": 5, "shuffle": 2, "blocksize": 4096}),
    "bitshuffle-1024": ("blosc", {"cname": "lz4", "clevel": 5, "shuffle": 2, "blocksize": 1024}),
}
GRIDS = {"2x3x40x72": (1, 2, 3, 40, 72), "1x3x40x36": (1, 1, 3, 40, 36)}
NOISE = (0, 0, 0, 0, 0)    # this chunk (no edge on any axis) holds random bytes: blosc writes it memcpyed
ABSENT = (0, 0, 0, 1, 0)   # this chunk file is absent: its samples read as fill_value


def need(codec):
    if "cname" in CODECS[codec][1] and _zarr.cblosc() is None:
        pytest.skip("c-blosc 1.21 library not in this image")


def be_bytes(a):
    return np.ascontiguousarray(a).astype(a.dtype.newbyteorder(">")).tobytes()


def fill_of(dt):
    """(fill_value as a sample, its bit pattern)"""
    v = np.array([-7.25 if dt.kind == "f" else 0x1234 % (1 << (8 * min(dt.itemsize, 2)))], dtype=dt.newbyteorder("="))
    return v[0], int(v.view("u%d" % dt.itemsize)[0])


_made = {}


def volume(dtype, grid):
    """(array with one chunk of random bytes, its chunks, the array as served: fill where the
    absent chunk is), made once per (dtype, chunk shape)."""
    key = (dtype, grid)
    if key not in _made:
        dt = np.dtype(dtype)
        chunks = GRIDS[grid]
        arr = ZD.noise_array(SHAPE, dtype, seed=len(_made) + 1)
        sel = tuple(slice(i * c, min((i + 1) * c, n)) for i, c, n in zip(NOISE, chunks, SHAPE))
        rnd = np.random.default_rng(5).integers(0, 256, arr[sel].size * dt.itemsize, dtype=np.uint8)
        if dt.kind == "f":  # keep the random floats finite: clear the top exponent bit
            rnd.reshape(-1, dt.itemsize)[:, -1 if dt.str[0] == "<" else 0] &= 0xBF
        arr[sel] = rnd.view(dt).reshape(arr[sel].shape)
        served = arr.copy()
        sel = tuple(slice(i * c, (i + 1) * c) for i, c in zip(ABSENT, chunks))
        served[sel] = fill_of(dt)[0]
        _made[key] = (arr, ZD.cut_chunks(arr, chunks), served)
    return _made[key]


def layers_of(cut, chunks, codec, dt, leads=None):
    """([layer dicts], {leading chunk indices: layer index}) for register_zarr_planes_deep."""
    comp, kw = CODECS[codec]
    enc = ZD.encoder(comp, **kw)
    grid = [-(-n // c) for n, c in zip(SHAPE, chunks)]
    depth = chunks[0] * chunks[1] * chunks[2]
    layers, index = [], {}
    for lead in itertools.product(*[range(g) for g in grid[:3]]):
        if leads is not None and lead not in leads:
            continue
        index[lead] = len(layers)
        layers.append(dict(chunk_x=chunks[4], chunk_y=chunks[3], codec=comp, chunk_planes=depth,
                           fill_bits=fill_of(dt)[1],
                           chunks=ZD.layer_files(cut, lead, grid[3:], enc, missing={ABSENT})))
    return layers, index


def plane_desc(iid, z, c, t, dt, level=0):
    return dict(image_id=iid, z=z, c=c, t=t, pixel_type=PT[dt.str[1:]], size_x=W, size_y=H,
                big_endian=dt.str[0] != "<", level=level)


def read_plane(service, pid, dt):
    return service.read_plane_be(pid, H * W * dt.itemsize)


@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("dtype", ["u1", "<u2", ">u2", "<f4", ">f8"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_registration_parity(service, grid, dtype, codec):
    """All 10 planes of the array in one deep call; then 2 non-adjacent slices of one layer alone
    (blocks of the other slices are not decoded)."""
    need(codec)
    dt = np.dtype(dtype)
    chunks = GRIDS[grid]
    arr, cut, served = volume(dtype, grid)
    layers, index = layers_of(cut, chunks, codec, dt)
    if CODECS[codec][1].get("codec") == "lz4":  # (c-blosc and zstd store such blocks split by split)
        assert layers[index[NOISE[:3]]]["chunks"][0][2] & 0x2, "the noise chunk should be a memcpyed frame"
        assert not layers[0]["chunks"][1][2] & 0x2
    iid = next(_ids)
    zct = [(z, c, 0) for c in range(SHAPE[1]) for z in range(SHAPE[2])]
    refs = []
    for z, c, t in zct:
        lead, slc = ZD.slice_of((t, c, z), chunks[:3])
        refs.append((index[lead], slc))
    ids = service.register_zarr_planes_deep([plane_desc(iid, z, c, t, dt) for z, c, t in zct], refs, layers)
    try:
        for (z, c, t), pid in zip(zct, ids):
            assert read_plane(service, pid, dt) == be_bytes(served[t, c, z]), (z, c, t)
    finally:
        for pid in ids:
            service.release_plane(pid)
    # two slices of the first layer that are not neighbours: slices 0 and 2 (depth 3), 1 and 4 (depth 6)
    lead = (0, 0, 0)
    depth = layers[0]["chunk_planes"]
    picks = [(0, 0, 0), (2, 0, 0)] if depth == 3 else [(1, 0, 0), (1, 1, 0)]
    sl = [ZD.slice_of((t, c, z), chunks[:3]) for z, c, t in picks]
    assert all(l == lead for l, _ in sl) and abs(sl[0][1] - sl[1][1]) >= 2
    ids = service.register_zarr_planes_deep([plane_desc(iid, z, c, t, dt) for z, c, t in picks],
                                            [(0, s) for _, s in sl], [layers[index[lead]]])
    try:
        for (z, c, t), pid in zip(picks, ids):
            assert read_plane(service, pid, dt) == be_bytes(served[t, c, z]), (z, c, t)
    finally:
        for pid in ids:
            service.release_plane(pid)


def test_tiles_equal_those_of_host_bytes(service):
    """raw, PNG and TIFF tiles of a deep-registered >u2 plane and of the same plane from host bytes."""
    dt = np.dtype(">u2")
    chunks = GRIDS["2x3x40x72"]
    arr, cut, served = volume(">u2", "2x3x40x72")
    layers, index = layers_of(cut, chunks, "lz4-shuffle-1024", dt, leads={(0, 0, 0)})
    z, c = 1, 1
    lead, slc = ZD.slice_of((0, c, z), chunks[:3])
    iid, hid = next(_ids), next(_ids)
    pid = service.register_zarr_planes_deep([plane_desc(iid, z, c, 0, dt)], [(0, slc)], layers)[0]
    host = service.register_plane(hid, z, c, 0, pbx.UINT16, W, H, data=served[0, c, z])
    try:
        def reqs(i):
            return [pbx.TileCtx(i, z, c, 0, 0, 0, W, H), pbx.TileCtx(i, z, c, 0, 3, 35, 91, 11),
                    pbx.TileCtx(i, z, c, 0, 8, 30, 64, 40, format="png"),
                    pbx.TileCtx(i, z, c, 0, 71, 39, 29, 31, format="png"),
                    pbx.TileCtx(i, z, c, 0, 5, 1, 90, 69, format="tif")]
        got, want = service.get_tiles(reqs(iid)), service.get_tiles(reqs(hid))
        for tc, (st, body), (wst, wbody) in zip(reqs(iid), got, want):
            assert st == pbx.OK and wst == pbx.OK and body == wbody, (tc.format, tc.x, tc.y)
        assert got[0][1] == served[0, c, z].tobytes()
    finally:
        service.release_plane(pid)
        service.release_plane(host)


# ------------------------------------------------------------------------------- NGFF images
def write_image(root, levels, sep="/"):
    """levels: [(array, chunk shape, codec name)] -> an NGFF image directory."""
    for k, (arr, chunks, codec) in enumerate(levels):
        comp, kw = CODECS[codec]
        ZD.write_array(root / str(k), arr, chunks, comp, ZD.encoder(comp, **kw), sep)
    (root / ".zattrs").write_text(json.dumps({"multiscales": [{
        "version": "0.4", "axes": [{"name": a} for a in "tczyx"],
        "datasets": [{"path": str(k)} for k in range(len(levels))]}]}))


@pytest.mark.parametrize("low", [(1, 2, 3, 24, 40), (1, 1, 1, 24, 40)], ids=["deep-deep", "deep-flat"])
def test_ngff_image_both_levels(service, tmp_path, low, monkeypatch):
    """register_ngff_image on deep chunks (and on a deep level 0 over a one-plane-per-chunk
    level 1): every (z, c, t) at both resolutions in OMERO numbering, each chunk file read once."""
    full = ZD.noise_array((1, 2, 5, 70, 100), ">u2", seed=31)
    half = ZD.noise_array((1, 2, 5, 35, 50), ">u2", seed=32)
    write_image(tmp_path / "img", [(full, (1, 2, 3, 40, 72), "lz4-shuffle-4096"), (half, low, "zlib")], ".")
    seen = []
    real = pbx._read_chunk_file
    monkeypatch.setattr(pbx, "_read_chunk_file", lambda path: seen.append(path) or real(path))
    iid = next(_ids)
    ids = service.register_ngff_image(str(tmp_path / "img"), iid)
    try:
        assert sorted(ids) == [0, 1] and all(len(v) == 10 for v in ids.values())
        assert len(seen) == len(set(seen))
        assert len(seen) == 2 * 4 + (2 * 4 if low[2] == 3 else 10 * 4)
        for c in range(2):
            for z in range(5):
                st, body = service.get_tile(pbx.TileCtx(iid, z, c, 0, 0, 0, 100, 70, resolution=1))
                assert st == pbx.OK and body == full[0, c, z].tobytes(), (z, c)
                st, body = service.get_tile(pbx.TileCtx(iid, z, c, 0, 0, 0, 100, 70))
                assert st == pbx.OK and body == full[0, c, z].tobytes(), (z, c)
                st, body = service.get_tile(pbx.TileCtx(iid, z, c, 0, 3, 2, 45, 33, resolution=0))
                assert st == pbx.OK and body == half[0, c, z][2:35, 3:48].tobytes(), (z, c)
    finally:
        for level in ids.values():
            for pid in level.values():
                service.release_plane(pid)


def test_array_planes_and_one_plane(service, tmp_path):
    """register_zarr_array_planes (a subset) and register_zarr_array (one plane) on deep chunks."""
    arr = ZD.noise_array((1, 2, 5, 70, 100), "<u2", seed=33)
    comp, kw = CODECS["lz4-shuffle-1024"]
    ZD.write_array(tmp_path / "a", arr, (1, 2, 3, 40, 72), comp, ZD.encoder(comp, **kw), "/")
    iid = next(_ids)
    got = service.register_zarr_array_planes(str(tmp_path / "a"), iid, planes=[(0, 0, 0), (4, 1, 0), (2, 1, 0)])
    one = service.register_zarr_array(str(tmp_path / "a"), iid, 3, 0, 0)
    try:
        for (z, c, t), pid in list(got.items()) + [((3, 0, 0), one)]:
            assert service.read_plane_be(pid, H * W * 2) == be_bytes(arr[t, c, z]), (z, c, t)
    finally:
        for pid in list(got.values()) + [one]:
            service.release_plane(pid)


# ------------------------------------------------------------------------------------- bands
BCH = (1, 1, 4, 40, 72)


@pytest.fixture(scope="module")
def band_volume():
    arr = ZD.noise_array((1, 1, 4, 70, 100), ">u2", seed=41)
    cut = ZD.cut_chunks(arr, BCH)
    files = {}
    for codec in ("lz4-shuffle-4096", "zlib", "bitshuffle-1024"):
        if "cname" in CODECS[codec][1] and _zarr.cblosc() is None:
            continue
        comp, kw = CODECS[codec]
        files[codec] = ZD.layer_files(cut, (0, 0, 0), (2, 2), ZD.encoder(comp, **kw))
    return arr, files


def write_rows(service, pid, files, codec, slc, y0, rows):
    lo, hi = y0 // 40, -(-(y0 + rows) // 40)
    service.band_write_zarr(pid, y0, rows, 72, 40, CODECS[codec][0], files[codec][lo * 2:hi * 2],
                            chunk_planes=4, slice=slc)


@pytest.mark.parametrize("codec", ["lz4-shuffle-4096", "zlib", "bitshuffle-1024"])
@pytest.mark.parametrize("slc", [0, 3])
def test_bands_from_deep_chunks(service, band_volume, codec, slc):
    """band_rows 16 under chunk rows of 40: whole bands, pieces at rows that are no chunk
    boundaries (one piece crossing rows 39|40 of two chunk rows), a piece from pbx_band_write in
    the same band, and a tile over two bands."""
    need(codec)
    arr, files = band_volume
    plane = arr[0, 0, slc]
    iid = next(_ids)
    pid = service.create_sparse_plane(iid, 0, 0, 0, pbx.UINT16, W, H, 16)
    try:
        write_rows(service, pid, files, codec, slc, 0, 16)        # band 0, whole
        write_rows(service, pid, files, codec, slc, 64, 6)        # band 4 (rows 64..69), whole
        assert service.band_info(pid)[1] == [pbx.BS_READY] + [pbx.BS_ABSENT] * 3 + [pbx.BS_READY]
        # band 2 = rows 32..47 over chunk rows 0 and 1, in three pieces, the middle one raw rows
        write_rows(service, pid, files, codec, slc, 43, 5)
        assert service.band_info(pid)[1][2] == pbx.BS_LOADING
        service.band_write(pid, 35, 3, plane[35:38].tobytes())
        write_rows(service, pid, files, codec, slc, 38, 5)        # rows 38..42: both chunk rows
        write_rows(service, pid, files, codec, slc, 32, 3)
        assert service.band_info(pid)[1][2] == pbx.BS_READY
        write_rows(service, pid, files, codec, slc, 21, 11)       # band 1 in two pieces
        write_rows(service, pid, files, codec, slc, 16, 5)
        assert service.band_info(pid)[1] == [pbx.BS_READY] * 3 + [pbx.BS_ABSENT, pbx.BS_READY]
        for y, h in ((0, 16), (64, 6), (32, 16), (16, 16), (9, 30)):  # the last: bands 0, 1 and 2
            st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, y, W, h))
            assert st == pbx.OK and body == plane[y:y + h].tobytes(), (y, h)
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 65, 12, 35, 9, format="png"))
        assert st == pbx.OK
        assert service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 48, 8, 8))[0] == pbx.E_NOT_RESIDENT
        with pytest.raises(pbx.PbxError) as ei:
            write_rows(service, pid, files, codec, slc, 0, 16)
        assert ei.value.status == pbx.E_EXISTS
    finally:
        service.release_plane(pid)


def test_cold_tile_through_the_handler(oracle, tmp_path, monkeypatch):
    """A TileRequestHandler over NgffSource on a sparse_band_rows service: a cold tile of z=2
    from a depth-4 array reads the covering chunk files only."""
    arr = ZD.noise_array((1, 1, 4, 70, 100), ">u2", seed=43)
    write_image(tmp_path / "img", [(arr, BCH, "lz4-shuffle-1024")], "/")
    seen, lock, real = [], threading.Lock(), pbx._read_chunk_file

    def spy(path):
        with lock:
            seen.append(os.path.relpath(path, str(tmp_path / "img")))
        return real(path)
    monkeypatch.setattr(pbx, "_read_chunk_file", spy)
    iid = next(_ids)
    src = pbx.NgffSource({iid: str(tmp_path / "img")})
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        tc = pbx.TileCtx(iid, 2, 0, 0, 10, 50, 80, 12)  # rows 50..61: bands 3 (48..63), chunk row 1
        body = pbx.TileRequestHandler(svc, tc, src).get_tile()
        assert body == arr[0, 0, 2][50:62, 10:90].tobytes()
        assert sorted(seen) == [os.path.join("0", "0", "0", "0", "1", str(i)) for i in range(2)]
        tc = pbx.TileCtx(iid, 2, 0, 0, 0, 30, 100, 20, format="tif")  # bands 1 and 2 (rows 16..47)
        body = pbx.TileRequestHandler(svc, tc, src).get_tile()
        r, px, _ = oracle.tiff_decode(body, 100 * 20 * 2)
        assert r == 0 and px == arr[0, 0, 2][30:50].tobytes()
        # band 1 lies in chunk row 0, band 2 (rows 32..47) in chunk rows 0 and 1
        assert sorted(seen[2:]) == sorted([os.path.join("0", "0", "0", "0", "0", str(i)) for i in range(2)] * 2 +
                                          [os.path.join("0", "0", "0", "0", "1", str(i)) for i in range(2)])
        pid = svc.lookup_plane(iid, 2, 0, 0)[0]
        assert svc.band_info(pid)[1] == [pbx.BS_ABSENT] + [pbx.BS_READY] * 3 + [pbx.BS_ABSENT]


# ------------------------------------------------------------------------------------ errors
def corrupt_needed_block(frame, nbytes, bs, lo):
    """Flip bytes inside the compressed streams of the blosc block that holds decoded byte `lo`."""
    b = lo // bs
    nblocks = -(-nbytes // bs)
    start = int.from_bytes(frame[16 + 4 * b:20 + 4 * b], "little")
    end = int.from_bytes(frame[20 + 4 * b:24 + 4 * b], "little") if b + 1 < nblocks else len(frame)
    c = bytearray(frame)
    for k in range(start + 4, min(end, start + 300), 7):  # after the first split's size word
        c[k] ^= 0xA5
    return bytes(c)


def test_corrupt_needed_block_registers_nothing(service):
    dt = np.dtype(">u2")
    chunks = GRIDS["2x3x40x72"]
    arr, cut, served = volume(">u2", "2x3x40x72")
    layers, _ = layers_of(cut, chunks, "lz4-shuffle-4096", dt, leads={(0, 0, 0)})
    good = layers[0]
    nbytes = 6 * 40 * 72 * 2
    picks = [(1, 0, 0), (1, 1, 0)]  # slices 1 and 4
    bad = dict(good, chunks=list(good["chunks"]))
    bad["chunks"][1] = corrupt_needed_block(good["chunks"][1], nbytes, 4096, 4 * 40 * 72 * 2 + 5000)
    iid = next(_ids)
    descs = [plane_desc(iid, z, c, t, dt) for z, c, t in picks]
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_planes_deep(descs, [(0, 1), (0, 4)], [bad])
    assert ei.value.status == 400
    assert service.lookup_plane(iid, 1, 0, 0) is None and service.lookup_plane(iid, 1, 1, 0) is None
    ids = service.register_zarr_planes_deep(descs, [(0, 1), (0, 4)], [good])  # the keys are free
    try:
        for (z, c, t), pid in zip(picks, ids):
            assert read_plane(service, pid, dt) == be_bytes(served[t, c, z])
    finally:
        for pid in ids:
            service.release_plane(pid)


def test_bad_slices_and_layers_are_400(service):
    dt = np.dtype(">u2")
    chunks = GRIDS["2x3x40x72"]
    arr, cut, served = volume(">u2", "2x3x40x72")
    layers, _ = layers_of(cut, chunks, "zlib", dt)
    iid = next(_ids)
    d0, d1 = plane_desc(iid, 0, 0, 0, dt), plane_desc(iid, 1, 0, 0, dt)

    def refused(descs, refs, ls):
        with pytest.raises(pbx.PbxError) as ei:
            service.register_zarr_planes_deep(descs, refs, ls)
        assert ei.value.status == 400, ei.value
        assert service.lookup_plane(iid, 0, 0, 0) is None

    refused([d0], [(0, 6)], layers[:1])                                   # slice >= chunk_planes
    refused([d0], [(0, 0)], [dict(layers[0], chunk_planes=0)])
    refused([d0, d1], [(0, 0), (0, 1)], layers)                           # layer 1: no plane
    refused([d0], [(1, 0)], layers[:1])                                   # no such layer
    refused([d0, dict(d1, size_y=H - 1)], [(0, 0), (0, 1)], layers[:1])   # sizes differ in a layer
    refused([d0, dict(d1, big_endian=False)], [(0, 0), (0, 1)], layers[:1])
    refused([d0, dict(d1, image_id=iid + 1, pixel_type=pbx.INT16)], [(0, 0), (0, 1)], layers[:1])
    refused([d0, d0], [(0, 0), (0, 1)], layers[:1])                       # the same key twice
    ids = service.register_zarr_planes_deep([d0, d1], [(0, 0), (0, 1)], layers[:1])
    for pid in ids:
        service.release_plane(pid)


def test_corrupt_needed_block_fails_the_band_load(service, band_volume):
    """As pbx_band_write_zarr: 400, the band reads absent again and its HBM is returned; the
    same damage in a block the rows do not need is never decoded."""
    arr, files = band_volume
    good = files["lz4-shuffle-4096"]
    nbytes, slc = 4 * 40 * 72 * 2, 3
    plane = arr[0, 0, slc]
    lo = (slc * 40 + 16) * 72 * 2  # row 16 of the slice: band 1
    bad = list(good)
    bad[0] = corrupt_needed_block(good[0], nbytes, 4096, lo + 1000)
    iid = next(_ids)
    pid = service.create_sparse_plane(iid, 0, 0, 0, pbx.UINT16, W, H, 16)
    try:
        base = service.residency_stats()["resident_bytes"]
        with pytest.raises(pbx.PbxError) as ei:
            service.band_write_zarr(pid, 16, 16, 72, 40, "blosc", bad[0:2], chunk_planes=4, slice=slc)
        assert ei.value.status == 400
        assert service.band_info(pid)[1][1] == pbx.BS_ABSENT
        assert service.residency_stats()["resident_bytes"] == base
        # slice 0's rows lie in other blocks: the damaged one is skipped
        service.band_write_zarr(pid, 16, 16, 72, 40, "blosc", bad[0:2], chunk_planes=4, slice=0)
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 16, W, 16))
        assert st == pbx.OK and body == arr[0, 0, 0][16:32].tobytes()
        for args in ((4, 4), (4, -1), (0, 0)):
            with pytest.raises(pbx.PbxError) as ei:
                service.band_write_zarr(pid, 0, 16, 72, 40, "blosc", good[0:2], chunk_planes=args[0], slice=args[1])
            assert ei.value.status == 400
        assert service.band_info(pid)[1][0] == pbx.BS_ABSENT
        service.band_write_zarr(pid, 0, 16, 72, 40, "blosc", good[0:2], chunk_planes=4, slice=slc)
        st, body = service.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 0, W, 16))
        assert st == pbx.OK and body == plane[0:16].tobytes()
    finally:
        service.release_plane(pid)
