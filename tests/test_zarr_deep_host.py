"""Zarr chunks that hold more than one plane, host side: the Python mirror's chunk files and
slices on an array directory, and the host planner (pbx_test_zarr_plan) with its block skip.
No GPU: nothing here makes a device call.

Expected planes are numpy slices of the 5-D array the chunks were cut from; expected stream
counts are derived here from the rule in include/pbx.h (a blosc block gets streams iff its
byte range meets the wanted slices' row ranges), not taken from the planner."""
import ctypes
import json
import zlib

import numpy as np
import pytest

import _zarr
import _zarr_deep as ZD
import pbx

SHAPE, CHUNKS = (2, 4, 5, 70, 100), (1, 2, 3, 40, 72)
MISSING = {(1, 1, 0, 1, 1)}  # t=1, c in 2..3, z in 0..2, chunk row 1, chunk column 1


@pytest.fixture(scope="module")
def arrays(tmp_path_factory):
    """The array written once per dimension separator as an NGFF image with one dataset."""
    arr = ZD.noise_array(SHAPE, ">u2", seed=4)
    enc = ZD.encoder("zlib")
    out = {}
    for sep, name in (("/", "slash"), (".", "dot")):
        root = tmp_path_factory.mktemp("deep_" + name) / "img"
        cut = ZD.write_array(root / "0", arr, CHUNKS, "zlib", enc, sep, MISSING, fill_value=7)
        (root / ".zattrs").write_text(json.dumps({"multiscales": [{
            "version": "0.4", "axes": [{"name": a} for a in "tczyx"], "datasets": [{"path": "0"}]}]}))
        out[sep] = (root, cut)
    return arr, enc, out


def expected_files(cut, enc, lead, rows):
    files = []
    for j in rows:
        for i in range(2):
            idx = lead + (j, i)
            files.append(None if idx in MISSING else enc(cut[idx].tobytes(), 2))
    return files


def check_slices(arr, t, c, z, sp, rows):
    """Slice sp["slice"] of every decompressed chunk is the numpy plane's part of that chunk."""
    assert sp["chunk_planes"] == 6 and (sp["chunk_y"], sp["chunk_x"]) == (40, 72)
    assert (sp["size_y"], sp["size_x"]) == (70, 100) and sp["codec"] == "zlib" and sp["big_endian"]
    assert sp["pixel_type"] == pbx.UINT16 and sp["fill_bits"] == 7
    for k, data in enumerate(sp["chunks"]):
        j, i = rows[k // 2], k % 2
        if data is None:
            continue
        dec = np.frombuffer(zlib.decompress(data), ">u2").reshape(6, 40, 72)
        want = arr[t, c, z, j * 40:(j + 1) * 40, i * 72:(i + 1) * 72]
        assert np.array_equal(dec[sp["slice"]][:want.shape[0], :want.shape[1]], want), (t, c, z, j, i)


@pytest.mark.parametrize("sep", ["/", "."], ids=["slash", "dot"])
def test_specs_name_the_chunk_files_and_the_slice(arrays, sep):
    arr, enc, dirs = arrays
    root, cut = dirs[sep]
    adir = str(root / "0")
    src = pbx.NgffSource({5: str(root)})
    px = src.get_pixels(5)
    assert (px.size_z, px.size_c, px.size_t, px.size_x, px.size_y) == (5, 4, 2, 100, 70)
    absent = 0
    for t in range(2):
        for c in range(4):
            for z in range(5):
                lead, slc = (t, c // 2, z // 3), (c % 2) * 3 + z % 3
                assert ZD.slice_of((t, c, z), CHUNKS[:3]) == (lead, slc)
                sp = pbx.zarr_plane_spec(adir, 5, z, c, t)
                assert sp["slice"] == slc and sp["chunks"] == expected_files(cut, enc, lead, (0, 1))
                assert (sp["image_id"], sp["z"], sp["c"], sp["t"], sp["level"]) == (5, z, c, t, 0)
                check_slices(arr, t, c, z, sp, (0, 1))
                absent += sp["chunks"].count(None)
                # rows 45..69 lie in chunk row 1 only; rows 30..49 in both
                for y0, rows, crows in ((45, 25, (1,)), (30, 20, (0, 1)), (0, 40, (0,))):
                    for bs in (pbx.zarr_band_spec(adir, z, c, t, y0, rows),
                               src.band_chunks(px, z, c, t, 0, y0, rows)):
                        assert bs["slice"] == slc and bs["chunks"] == expected_files(cut, enc, lead, crows)
                        check_slices(arr, t, c, z, bs, crows)
    assert absent == 6  # the absent file, once for each of the 6 planes it holds


def test_rows_zero_opens_no_file(arrays, monkeypatch):
    arr, enc, dirs = arrays
    root, _ = dirs["/"]
    seen = []
    real = pbx._read_chunk_file
    monkeypatch.setattr(pbx, "_read_chunk_file", lambda path: seen.append(path) or real(path))
    src = pbx.NgffSource({5: str(root)})
    sp = src.band_chunks(src.get_pixels(5), 4, 3, 1, 0, 0, 0)
    assert seen == [] and sp["chunks"] == [] and sp["chunk_planes"] == 6 and sp["slice"] == 1 * 3 + 4 % 3
    sp = pbx.zarr_band_spec(str(root / "0"), 4, 3, 1, 0, 0)
    assert seen == [] and sp["chunk_planes"] == 6
    pbx.zarr_band_spec(str(root / "0"), 4, 3, 1, 0, 40)
    assert len(seen) == 2


def test_planes_of_a_layer_share_one_read(arrays, monkeypatch):
    """With the registration's cache, the 6 planes of a layer hold the same chunk list."""
    arr, enc, dirs = arrays
    root, _ = dirs["."]
    seen = []
    real = pbx._read_chunk_file
    monkeypatch.setattr(pbx, "_read_chunk_file", lambda path: seen.append(path) or real(path))
    cache = {}
    specs = [pbx.zarr_plane_spec(str(root / "0"), 5, z, c, 0, cache=cache) for c in range(4) for z in range(5)]
    assert len(seen) == len(set(seen)) == 2 * 2 * 4  # (c, z) chunk grid 2 x 2, 4 files per layer
    assert len({sp["layer"] for sp in specs}) == 4
    for a in specs:
        for b in specs:
            assert (a["chunks"] is b["chunks"]) == (a["layer"] == b["layer"])


def test_one_plane_per_chunk_spec_is_unchanged(tmp_path):
    arr = ZD.noise_array((1, 2, 3, 50, 60), "<u2", seed=1)
    enc = ZD.encoder("zlib")
    cut = ZD.write_array(tmp_path / "a", arr, (1, 1, 1, 32, 32), "zlib", enc, ".")
    sp = pbx.zarr_plane_spec(str(tmp_path / "a"), 9, 2, 1, 0, level=3)
    files = [enc(cut[(0, 1, 2, j, i)].tobytes(), 2) for j in range(2) for i in range(2)]
    assert sp == dict(pixel_type=pbx.UINT16, size_x=60, size_y=50, chunk_x=32, chunk_y=32, codec="zlib",
                      chunks=files, big_endian=False, fill_bits=0, image_id=9, z=2, c=1, t=0, level=3)
    bs = pbx.zarr_band_spec(str(tmp_path / "a"), 2, 1, 0, 32, 10)
    assert bs == dict(pixel_type=pbx.UINT16, size_x=60, size_y=50, chunk_x=32, chunk_y=32, codec="zlib",
                      chunks=files[2:], big_endian=False, fill_bits=0, y0=32, rows=10)


def test_other_array_forms_stay_400(tmp_path):
    arr = ZD.noise_array((1, 1, 2, 8, 8), "<u2")
    for change in ({"order": "F"}, {"zarr_format": 3}, {"dtype": "<c8"}, {"filters": [{"id": "delta"}]},
                   {"chunks": [2, 8, 8]}, {"chunks": [1, 1, 0, 8, 8]}):
        d = tmp_path / ("a%d" % len(list(tmp_path.iterdir())))
        ZD.write_array(d, arr, (1, 1, 2, 8, 8), None, ZD.encoder(None))
        meta = json.loads((d / ".zarray").read_text())
        meta.update(change)
        (d / ".zarray").write_text(json.dumps(meta))
        with pytest.raises(pbx.PbxError) as ei:
            pbx.zarr_array_meta(str(d))
        assert ei.value.status == 400, change


# ------------------------------------------------------------------------- the host planner
D, CY, CX, BPP, BS = 8, 40, 72, 2, 4096
NBYTES = D * CY * CX * BPP


def plan(chunks, codec, depth, slices, y0=0, rows=0, cx=CX, cy=CY, sx=CX, sy=CY, bpp=BPP):
    """pbx_test_zarr_plan -> (status, [streams, sum of dlen, blocks skipped, scratch bytes])."""
    if chunks is None:
        data, offsets = None, np.zeros(2, np.uint64)
    else:
        data, offsets = pbx.pack_chunks(chunks)
    zc = pbx.PbxZarrChunks()
    zc.chunk_x, zc.chunk_y, zc.codec = cx, cy, pbx.ZARR_CODECS[codec]
    zc.data, zc.offsets = (data.ctypes.data if data is not None else None), offsets.ctypes.data
    sl = (ctypes.c_int32 * len(slices))(*slices)
    out = (ctypes.c_uint64 * 4)()
    rc = pbx.lib().pbx_test_zarr_plan(ctypes.byref(zc), sx, sy, bpp, depth, sl, len(slices), y0, rows, out)
    return rc, list(out)


def by_the_rule(nbytes, bs, ts, ranges):
    """(streams, sum of dlen, blocks skipped) of a split blosc frame by the rule of pbx.h: block
    b = bytes [b * bs, min((b + 1) * bs, nbytes)) gets streams iff it meets one of `ranges`;
    then every split does (c-blosc splits a block into `ts` streams when it holds >= 128
    elements and is not the leftover block)."""
    streams = dlen = skipped = 0
    nblocks = -(-nbytes // bs)
    for b in range(nblocks):
        b0, b1 = b * bs, min((b + 1) * bs, nbytes)
        leftover = b == nblocks - 1 and nbytes % bs != 0
        if any(b0 < hi and lo < b1 for lo, hi in ranges):
            streams += ts if (b1 - b0) // ts >= 128 and not leftover else 1
            dlen += b1 - b0
        else:
            skipped += 1
    return streams, dlen, skipped


def rows_of(slices, ra=0, rb=CY):
    return [((s * CY + ra) * CX * BPP, (s * CY + rb) * CX * BPP) for s in slices]


@pytest.fixture(scope="module")
def deep_chunk():
    vol = ZD.noise_array((1, 1, D, CY, CX), "<u2", seed=2)[0, 0]
    frame = _zarr.blosc_encode(vol.tobytes(), 2, blocksize=BS)
    assert len(vol.tobytes()) == NBYTES == 46080 and not frame[2] & 0x2  # compressed, not memcpyed
    assert -(-NBYTES // BS) == 12 and NBYTES % BS == 1024
    return vol, frame


@pytest.mark.parametrize("slices,y0,rows", [([3], 0, 0), ([1, 6], 0, 0), (list(range(D)), 0, 0), ([5], 8, 16)],
                         ids=["one", "two-apart", "all", "band-rows-8-23-of-5"])
def test_planner_decodes_only_the_blocks_of_the_wanted_rows(deep_chunk, slices, y0, rows):
    _, frame = deep_chunk
    ranges = rows_of(slices, y0, y0 + rows) if rows else rows_of(slices)
    streams, dlen, skipped = by_the_rule(NBYTES, BS, 2, ranges)
    # slices of 5,760 bytes straddle the 4,096-byte blocks
    assert any(lo % BS and hi % BS for lo, hi in ranges)
    rc, out = plan([frame], "blosc", D, slices, y0, rows)
    assert rc == 0, pbx.lib().pbx_last_error()
    assert out[:3] == [streams, dlen, skipped]
    assert out[3] >= NBYTES  # scratch stays sized for the whole chunk
    if len(slices) == D:
        assert skipped == 0 and dlen == NBYTES
    else:
        assert 0 < skipped < 12


def test_band_window_skips_more_than_its_slice(deep_chunk):
    _, frame = deep_chunk
    whole, part = plan([frame], "blosc", D, [5])[1], plan([frame], "blosc", D, [5], 8, 16)[1]
    assert part[2] > whole[2] and part[3] == whole[3]


def test_zlib_and_raw_layers_are_taken_whole(deep_chunk):
    vol, _ = deep_chunk
    rc, out = plan([zlib.compress(vol.tobytes(), 1)], "zlib", D, [2])
    assert rc == 0 and out[:3] == [1, NBYTES, 0] and out[3] >= NBYTES
    rc, out = plan([vol.tobytes()], None, D, [2], 8, 16)
    assert rc == 0 and out == [0, 0, 0, 0]
    noise = np.random.default_rng(0).integers(0, 256, NBYTES, dtype=np.uint8).tobytes()
    frame = _zarr.blosc_encode(noise, 2, blocksize=BS)
    assert frame[2] & 0x2  # memcpyed
    rc, out = plan([frame], "blosc", D, [2])
    assert rc == 0 and out == [0, 0, 0, 0]
    rc, out = plan([None], "blosc", D, [2])  # a missing chunk
    assert rc == 0 and out == [0, 0, 0, 0]


def test_planner_400s(deep_chunk):
    _, frame = deep_chunk
    for depth, slices in ((D, [D]), (D, [0, -1]), (0, [0]), (-3, [0])):
        assert plan([frame], "blosc", depth, slices)[0] == 400, (depth, slices)
    assert plan([frame], "blosc", 4, [0])[0] == 400      # blosc nbytes != chunk bytes
    assert plan([frame], "blosc", 16, [0])[0] == 400
    assert plan([frame], "blosc", D, [0], 30, 11)[0] == 400  # rows outside the plane
    # 2^31 bytes: one plane of 32768 x 32768 uint16, and 2 planes of 16384 x 32768
    assert plan(None, None, 1, [0], cx=32768, cy=32768, sx=32768, sy=32768)[0] == 400
    assert plan(None, None, 2, [1], cx=32768, cy=16384, sx=32768, sy=16384)[0] == 400
    assert plan(None, None, 65536, [0], cx=32768, cy=32768, sx=32768, sy=32768)[0] == 400
    assert plan(None, None, 1, [0], cx=32768, cy=16384, sx=32768, sy=16384)[0] == 0  # 2^30: fine


def test_depth_one_plans_every_block():
    """chunk_planes == 1 is the planner of one plane per chunk: every block of every chunk,
    whatever the rows (a 100 x 70 plane of 40 x 72 chunks, 1,024-byte blocks + leftover)."""
    plane = _zarr.noise_plane(70, 100, "<u2", seed=3)
    chunks = _zarr.encode_chunks(plane, CY, CX, "blosc", blocksize=1024)
    per_chunk = by_the_rule(CY * CX * BPP, 1024, 2, [(0, CY * CX * BPP)])
    assert per_chunk[2] == 0
    rc, out = plan(chunks, "blosc", 1, [0], sx=100, sy=70)
    assert rc == 0 and out[:3] == [4 * per_chunk[0], 4 * per_chunk[1], 0]
    rc, out = plan(chunks[2:], "blosc", 1, [0], 45, 10, sx=100, sy=70)  # chunk row 1, whole
    assert rc == 0 and out[:3] == [2 * per_chunk[0], 2 * per_chunk[1], 0]


def test_exports():
    for name in ("pbx_planes_register_zarr_deep", "pbx_band_write_zarr_deep", "pbx_test_zarr_plan"):
        assert name in pbx.EXPORTS and hasattr(pbx.lib(), name)
    assert ctypes.sizeof(pbx.PbxZarrSlice) == 8
    assert pbx.lib().pbx_abi_version() == 9
