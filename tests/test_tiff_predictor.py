"""TIFF Predictor = 2 on the CPU: the numpy restatement (tests/_tiff_pred.py) pinned against an
independent decoder (PIL with libtiff), the shared header writers of csrc/pbx_common.h through
the emulator library, the Python option's validation, and what the differencing buys in bytes
through the emulated deflate."""
import ctypes
import zlib

import numpy as np
import pytest

import _emu
import _tiff_pred as TP
import pbx

GEN_FAKE = 1


def _emu_lib():
    L = _emu.lib()
    u8p, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.pbxemu_tiff_header.restype = u32
    L.pbxemu_tiff_header.argtypes = [u8p] + [u32] * 7
    L.pbxemu_tiff_tiled_header.restype = ctypes.c_uint64
    L.pbxemu_tiff_tiled_header.argtypes = [u8p] + [u32] * 10 + [ctypes.POINTER(u32)]
    L.pbxemu_tiff_pred_run_rows.restype = u32
    return L


def strip_header(w, h, bpp, sf, comp, nbytes, predictor):
    buf = ctypes.create_string_buffer(b"\xAA" * 256, 256)
    off = _emu_lib().pbxemu_tiff_header(buf, w, h, bpp, sf, comp, nbytes, predictor)
    assert buf.raw[off:] == b"\xAA" * (256 - off)  # nothing written past the header
    return buf.raw[:off]


def tiled_header(w, h, t, bpp, sf, comp, n, off0, cnt0, predictor):
    buf = ctypes.create_string_buffer(b"\xAA" * 256, 256)
    arrays = ctypes.c_uint32()
    data = _emu_lib().pbxemu_tiff_tiled_header(buf, w, h, t, bpp, sf, comp, n, off0, cnt0, predictor,
                                               ctypes.byref(arrays))
    assert buf.raw[arrays.value:] == b"\xAA" * (256 - arrays.value)
    return buf.raw[:arrays.value], arrays.value, data


# ------------------------------------------------------------------------- restatement

@pytest.mark.parametrize("bpp", [1, 2, 4])
def test_restatement_roundtrip_and_padding(bpp):
    rng = np.random.default_rng(bpp)
    w, h, t = 37, 9, 16
    tile = rng.bytes(w * h * bpp)
    s = TP.forward(tile, w, h, bpp)
    assert len(s) == len(tile) and TP.inverse(s, w, h, bpp) == tile
    a = np.frombuffer(tile, TP.UDT[bpp]).reshape(h, w).astype(np.int64)
    d = np.frombuffer(s, TP.UDT[bpp]).reshape(h, w).astype(np.int64)
    assert (d[:, 0] == a[:, 0]).all()
    assert (d[:, 1:] == (a[:, 1:] - a[:, :-1]) % (1 << (8 * bpp))).all()
    subs = TP.forward_subtiles(tile, w, h, bpp, t)
    assert len(subs) == 3 and all(len(x) == t * t * bpp for x in subs)
    last = np.frombuffer(subs[2], TP.UDT[bpp]).reshape(t, t).astype(np.int64)
    # the padding is differenced like data: 0 - last valid sample, then zeros; pad rows all zero
    assert (last[:h, 5] == (-a[:, 36]) % (1 << (8 * bpp))).all() and not last[:h, 6:].any() and not last[h:].any()
    for k, x in enumerate(subs):
        assert TP.inverse(x, t, t, bpp) == TP.pad_subtile(tile, w, h, bpp, t, k, 0)


@pytest.mark.parametrize("pt,mode", [(pbx.UINT8, "L"), (pbx.UINT16, "I;16B")])
def test_pil_decodes_header_plus_deflated_restatement(pt, mode):
    """An independent decoder undoes the restated stream: libtiff through PIL."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check("libtiff"):
        pytest.skip("PIL without libtiff")
    import io
    bpp = TP.BPP[pt]
    w, h = 67, 21
    tile = np.random.default_rng(pt).bytes(w * h * bpp)  # full-range values: low bytes borrow
    z = zlib.compress(TP.forward(tile, w, h, bpp), 6)
    body = strip_header(w, h, bpp, 1, 8, len(z), 2) + z
    im = Image.open(io.BytesIO(body))
    assert im.mode == mode and im.size == (w, h)
    got = np.asarray(im)
    want = np.frombuffer(tile, TP.UDT[bpp]).reshape(h, w)
    assert (got.astype(np.int64) == want.astype(np.int64)).all()


# -------------------------------------------------------------------------- header writers

@pytest.mark.parametrize("pt", range(6))
def test_strip_header_with_and_without_the_predictor(oracle, pt):
    bpp = TP.BPP[pt]
    sf = 2 if pt in (pbx.INT8, pbx.INT16, pbx.INT32) else 1
    w, h = 40, 12
    tile = np.frombuffer(np.random.default_rng(pt).bytes(w * h * bpp), np.uint8)
    st, ref = oracle.tiff_encode(tile, pt, w, h)
    assert st == 0
    assert strip_header(w, h, bpp, sf, 1, w * h * bpp, 1) == ref[:160]  # off: today's bytes
    hdr = strip_header(w, h, bpp, sf, 8, 777, 2)
    assert len(hdr) == 160
    tags, order, end = TP.ifd(hdr)
    assert order == sorted(order) and len(set(order)) == len(order) == 12 and end == 158
    assert tags[TP.TAG_PREDICTOR] == (3, 1, 2) and order.index(317) == order.index(284) + 1 == order.index(339) - 1
    assert tags[273][2] == 160 and tags[279][2] == 777 and tags[259][2] == 8
    off_tags, off_order, off_end = TP.ifd(strip_header(w, h, bpp, sf, 8, 777, 1))
    assert off_end == 146 and 317 not in off_tags
    assert {k: v for k, v in tags.items() if k != 317} == off_tags  # every other entry unchanged


@pytest.mark.parametrize("n", [1, 6])
def test_tiled_header_with_and_without_the_predictor(oracle, n):
    t, bpp = 16, 2
    w, h = (16, 16) if n == 1 else (40, 20)
    tile = np.random.default_rng(n).bytes(w * h * bpp)
    ref = oracle.tiff_tiled_write(tile, w, h, bpp, 1, t, 1)
    hdr, arrays, data = tiled_header(w, h, t, bpp, 1, 1, n, 160, t * t * bpp, 1)
    assert arrays == 160 and hdr == ref[:160]  # off: today's bytes
    assert data == (160 if n == 1 else (160 + 8 * n + 15) // 16 * 16)
    hdr, arrays, data = tiled_header(w, h, t, bpp, 1, 8, n, 176, 99, 2)
    tags, order, end = TP.ifd(hdr)
    assert order == sorted(order) and len(set(order)) == len(order) == 13 and end == 170
    assert tags[TP.TAG_PREDICTOR] == (3, 1, 2) and order.index(317) == order.index(284) + 1 == order.index(322) - 1
    assert arrays == 176 and data == (176 if n == 1 else (176 + 8 * n + 15) // 16 * 16) and data % 16 == 0
    if n == 1:
        assert tags[324] == (4, 1, 176) and tags[325] == (4, 1, 99)
    else:
        assert tags[324] == (4, n, 176) and tags[325] == (4, n, 176 + 4 * n)
    off = TP.ifd(tiled_header(w, h, t, bpp, 1, 8, n, 160, 99, 1)[0])[0]
    same = {k: v for k, v in tags.items() if k not in (317, 324, 325)}
    assert same == {k: v for k, v in off.items() if k not in (324, 325)}


def test_fast_kernel_run_length_is_exported():
    assert _emu_lib().pbxemu_tiff_pred_run_rows() >= 2


# --------------------------------------------------------------------------------- option

def test_python_option_validation_and_symbols():
    assert (pbx.TIFF_PREDICTOR_NONE, pbx.TIFF_PREDICTOR_HORIZONTAL) == (1, 2)
    for bad in (0, 3, -1, 317):
        with pytest.raises(pbx.PbxError) as e:
            pbx.make_config(tiff_predictor=bad)
        assert e.value.status == pbx.E_BADARG == 400
        with pytest.raises(pbx.PbxError) as e:
            pbx.PixelsService(tiff_predictor=bad)
        assert e.value.status == pbx.E_BADARG
    for ok in (None, 1, 2):
        assert ctypes.sizeof(pbx.make_config(tiff_predictor=ok)) == ctypes.sizeof(pbx.PbxConfig)
    L = pbx.lib()
    for name in ("pbx_set_tiff_predictor", "pbx_get_tiff_predictor", "pbx_batch_pred_tiles"):
        assert name in pbx.EXPORTS and hasattr(L, name)
    assert L.pbx_set_tiff_predictor(None, 2) == pbx.E_BADARG  # null context
    assert hasattr(pbx.PixelsService, "set_tiff_predictor") and isinstance(pbx.PixelsService.tiff_predictor, property)


def test_environment_value_is_validated_at_init(monkeypatch):
    """$PBX_TIFF_PREDICTOR outside {1, 2}: pbx_init answers 400, before it looks for a device."""
    for bad in ("0", "3", "22", "x", ""):
        monkeypatch.setenv("PBX_TIFF_PREDICTOR", bad)
        with pytest.raises(pbx.PbxError) as e:
            pbx.PixelsService()
        assert e.value.status == pbx.E_BADARG and "PBX_TIFF_PREDICTOR" in str(e.value), bad


# ---------------------------------------------------------------------------------- bytes

def bytes_tiles(oracle):
    """The two 512 x 512 uint16 tiles of the byte comparisons (also uploaded by the GPU test):
    G_FAKE's ramp and the seeded smooth scene."""
    fake = oracle.gen_region(GEN_FAKE, pbx.UINT16, 512, 512, 512, 512).tobytes()
    scene = TP.smooth_scene(512, 512, 7).astype(">u2").tobytes()
    return {"fake": fake, "scene": scene}


@pytest.mark.parametrize("kind", ["fake", "scene"])
def test_predictor_stream_deflates_smaller(oracle, kind):
    """The pipeline's own deflate (emulated) on one 512 x 512 uint16 tile: the differenced stream
    is smaller than the plain one (zlib level 6: 0.51 on a ramp, about 0.9 on the scene)."""
    tile = bytes_tiles(oracle)[kind]
    plain, _ = _emu.deflate(tile, 1024)
    s = TP.forward(tile, 512, 512, 2)
    pred, _ = _emu.deflate(s, 1024)
    assert zlib.decompress(pred) == s and TP.inverse(s, 512, 512, 2) == tile
    print(kind, "plain", len(plain), "predictor", len(pred), "ratio %.3f" % (len(pred) / len(plain)),
          "zlib-6", len(zlib.compress(tile, 6)), len(zlib.compress(s, 6)))
    assert len(pred) < len(plain)
