"""Zarr chunk rows on demand, the host side (no GPU): the pbx_band_write_zarr export,
zarr_band_spec's choice of chunk files and NgffSource's metadata.
"""
import json
import os

import numpy as np
import pytest

import _zarr
import pbx
from test_host import header_functions


def test_export_is_declared_and_present():
    assert "pbx_band_write_zarr" in pbx.EXPORTS
    assert header_functions() == sorted(pbx.EXPORTS)
    assert hasattr(pbx.lib(), "pbx_band_write_zarr")


def test_null_context_is_400():
    zc = pbx.PbxZarrChunks()
    assert pbx.lib().pbx_band_write_zarr(None, 1, 0, 1, zc, None) == pbx.E_BADARG
    assert pbx.lib().pbx_band_write_zarr(None, 1, 0, 1, None, None) == pbx.E_BADARG


def _write_array(root, shape, chunks, dtype, sep, compressor="zlib", fill=0, skip=()):
    """A Zarr v2 array directory of noise planes; returns {lead index tuple: plane}."""
    root.mkdir(parents=True, exist_ok=True)
    meta = {"zarr_format": 2, "shape": list(shape), "chunks": list(chunks), "dtype": dtype,
            "order": "C", "fill_value": fill, "filters": None, "dimension_separator": sep,
            "compressor": None if compressor is None else {"id": compressor}}
    (root / ".zarray").write_text(json.dumps(meta))
    planes = {}
    gx = -(-shape[-1] // chunks[-1])
    for lead in np.ndindex(*shape[:-2]):
        p = _zarr.noise_plane(shape[-2], shape[-1], dtype, seed=sum(lead) + 5)
        planes[lead] = p
        for k, ch in enumerate(_zarr.encode_chunks(p, chunks[-2], chunks[-1], compressor)):
            j, i = divmod(k, gx)
            if (lead, j, i) in skip:
                continue
            path = root / sep.join(str(v) for v in list(lead) + [j, i])
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_bytes(ch)
    return planes


@pytest.fixture
def opened(monkeypatch):
    """The chunk file paths pbx reads (present or not), in order."""
    paths = []
    real = pbx._read_chunk_file

    def spy(path):
        paths.append(path)
        return real(path)
    monkeypatch.setattr(pbx, "_read_chunk_file", spy)
    return paths


@pytest.mark.parametrize("ndim,sep", [(5, "/"), (5, "."), (3, "."), (3, "/"), (2, "."), (2, "/")])
def test_band_spec_reads_the_covering_chunk_rows_only(tmp_path, opened, ndim, sep):
    """200 rows in chunk rows of 32 (7 chunk rows, the last 8 rows tall), 3 chunk columns: the
    first, a middle and the last band of 64 and of 50 rows (not on chunk boundaries), and a
    5-row piece inside one chunk row."""
    import zlib
    sy, sx, cy, cx = 200, 90, 32, 40
    shape = [2, 3, 2, sy, sx][5 - ndim:]
    lead = tuple([1, 2, 1][3 - (ndim - 2):]) if ndim > 2 else ()
    adir = tmp_path / "a"
    planes = _write_array(adir, shape, [1] * (ndim - 2) + [cy, cx], ">u2", sep, fill=11,
                          skip={(lead, 3, 1)})
    z, c, t = (lead[-1] if ndim >= 3 else 0), (lead[-2] if ndim >= 4 else 0), (lead[-3] if ndim >= 5 else 0)
    grid = _zarr.chunk_grid(planes[lead], cy, cx)
    for y0, rows, want_rows in [(0, 64, [0, 1]), (64, 64, [2, 3]), (192, 8, [6]),
                                (0, 50, [0, 1]), (50, 50, [1, 2, 3]), (150, 50, [4, 5, 6]),
                                (100, 5, [3]), (95, 2, [2, 3]), (0, 200, list(range(7)))]:
        del opened[:]
        sp = pbx.zarr_band_spec(str(adir), z, c, t, y0, rows)
        want_paths = [os.path.join(str(adir), sep.join(str(v) for v in list(lead) + [j, i]))
                      for j in want_rows for i in range(3)]
        assert opened == want_paths, (y0, rows)
        assert (sp["y0"], sp["rows"], sp["size_x"], sp["size_y"]) == (y0, rows, sx, sy)
        assert (sp["chunk_x"], sp["chunk_y"], sp["codec"]) == (cx, cy, "zlib")
        assert sp["pixel_type"] == pbx.UINT16 and sp["big_endian"] is True and sp["fill_bits"] == 11
        assert len(sp["chunks"]) == 3 * len(want_rows)
        for n, (j, i) in enumerate((j, i) for j in want_rows for i in range(3)):
            if (j, i) == (3, 1):
                assert sp["chunks"][n] is None  # the absent file
            else:
                assert zlib.decompress(sp["chunks"][n]) == grid[j * 3 + i].tobytes()
    # the same files as the whole-plane spec, which keeps its contents
    whole = pbx.zarr_plane_spec(str(adir), 5, z, c, t)
    assert whole["chunks"] == pbx.zarr_band_spec(str(adir), z, c, t, 0, sy)["chunks"]
    assert (whole["image_id"], whole["level"], whole["size_y"]) == (5, 0, sy)
    # no rows: no file
    del opened[:]
    sp = pbx.zarr_band_spec(str(adir), z, c, t, 0, 0)
    assert opened == [] and sp["chunks"] == [] and sp["big_endian"] is True
    with pytest.raises(pbx.PbxError) as ei:  # a plane outside the array
        pbx.zarr_band_spec(str(adir), 99 if ndim >= 3 else 0, c, t + (ndim < 3), 0, 64)
    assert ei.value.status == 404 and opened == []
    with pytest.raises(pbx.PbxError) as ei:  # rows outside it
        pbx.zarr_band_spec(str(adir), z, c, t, 150, 64)
    assert ei.value.status == 400 and opened == []


def _write_image(root, sizes, lead, chunk, dtype, seps):
    """A multiscale image: dataset k is an array of size sizes[k] with separator seps[k]."""
    root.mkdir(parents=True, exist_ok=True)
    arrays = []
    for k, (h, w) in enumerate(sizes):
        arrays.append(_write_array(root / str(k), list(lead) + [h, w], [1] * len(lead) + list(chunk),
                                   dtype, seps[k]))
    axes = ["t", "c", "z", "y", "x"][3 - len(lead):]
    (root / ".zattrs").write_text(json.dumps({"multiscales": [{
        "version": "0.4", "axes": [{"name": a} for a in axes],
        "datasets": [{"path": str(k)} for k in range(len(sizes))]}]}))
    return arrays


def test_ngff_source_metadata(tmp_path, opened):
    _write_image(tmp_path / "img", [(70, 90), (35, 45)], (2, 3), (32, 40), "<i4", "/.")
    src = pbx.NgffSource({41: str(tmp_path / "img")})
    assert src.get_pixels(42) is None
    px = src.get_pixels(41)
    assert (px.image_id, px.pixel_type, px.size_x, px.size_y) == (41, pbx.INT32, 90, 70)
    assert (px.size_z, px.size_c, px.size_t, px.levels) == (3, 2, 1, 2)
    assert src.level_size(px, 0) == (90, 70) and src.level_size(px, 1) == (45, 35)
    assert opened == []  # metadata only
    sp = src.band_chunks(px, 2, 1, 0, 1, 32, 3)  # level 1 ("." separator), its last chunk row
    assert opened == [os.path.join(str(tmp_path / "img" / "1"), "1.2.1.%d" % i) for i in range(2)]
    assert sp["big_endian"] is False and (sp["size_x"], sp["size_y"]) == (45, 35)
    assert src.band_chunks(px, 0, 0, 0, 0, 0, 0)["chunks"] == []
    with pytest.raises(pbx.PbxError) as ei:
        src.read_rows(px, 0, 0, 0, 0, 0, 8)
    assert ei.value.status == pbx.E_BADARG and "sparse_band_rows" in str(ei.value)
