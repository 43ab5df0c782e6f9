"""The deflate strategies on the CPU emulator (csrc/emu.cpp pbxemu_deflate_strategy /
pbxemu_lz77_strategy: what the GPU matches byte for byte): DEFAULT is today's deflate,
HUFFMAN_ONLY holds no match, AUTO decides per 16 KiB segment from a sample of its bytes
(csrc/deflate_seg.h ph_sample).  Ten seeded 512 x 512 tile kinds (DESIGN.md §2's table)."""
import functools
import zlib

import numpy as np
import pytest

import _emu
import _emu_strategy as ES

KINDS = [name for name, _ in ES.tile_kinds(8, 64)]
NOISY = {"noise16", "noise8", "poisson250_16", "poisson30_8"}            # AUTO: every segment Huffman-only
STRUCTURED = {"ramp16", "noise_half_zero16", "noise_7of8_zero16"}        # AUTO: every segment parsed


@functools.lru_cache(maxsize=None)
def _tiles():
    return {name: (a, ES.png_stream(a), 1 + a.shape[1] * a.dtype.itemsize) for name, a in ES.tile_kinds()}


@functools.lru_cache(maxsize=None)
def _deflated(name, strategy):
    _, stream, rowlen = _tiles()[name]
    return ES.deflate(stream, rowlen, strategy)


@functools.lru_cache(maxsize=None)
def _lz(name, strategy):
    _, stream, rowlen = _tiles()[name]
    return ES.lz77(stream, rowlen, strategy)


@pytest.mark.parametrize("name", KINDS)
def test_every_strategy_inflates_to_the_stream(name):
    stream = _tiles()[name][1]
    for st in ES.STRATEGIES:
        assert zlib.decompress(_deflated(name, st)) == stream, (name, st)


@pytest.mark.parametrize("name", KINDS)
def test_default_strategy_is_todays_deflate(name):
    _, stream, rowlen = _tiles()[name]
    z, _ = _emu.deflate(stream, rowlen)
    assert _deflated(name, ES.DEFAULT) == z
    h0, m0 = _emu.lz77(stream, rowlen)
    h, m, modes = _lz(name, ES.DEFAULT)
    assert (h == h0).all() and (m == m0).all() and not modes.any()


@pytest.mark.parametrize("name", KINDS)
def test_huffman_only_has_no_match(name):
    h, m, modes = _lz(name, ES.HUFFMAN_ONLY)
    assert not m.any(), name          # no per-wave match count, no record
    assert not h[:, 257:].any(), name  # no length symbol, no distance count
    assert (h[:, 256] == 1).all() and (modes == 1).all()
    _, stream, _ = _tiles()[name]
    assert int(h[:, :256].sum()) == len(stream)  # every byte a literal


@pytest.mark.parametrize("name", KINDS)
def test_huffman_only_bytes_against_zlib(name):
    """zlib's Z_HUFFMAN_ONLY splits blocks where the statistics change; here the segments of a
    tile share one code: at most 3 % more bytes."""
    stream = _tiles()[name][1]
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    ref = len(c.compress(stream) + c.flush())
    got = len(_deflated(name, ES.HUFFMAN_ONLY))
    print(name, "huffman-only", got, "zlib Z_HUFFMAN_ONLY", ref, "ratio %.4f" % (got / ref))
    assert got <= ref * 1.03, (name, got, ref)


@pytest.mark.parametrize("name", KINDS)
def test_auto_never_loses_to_default(name):
    d, a = len(_deflated(name, ES.DEFAULT)), len(_deflated(name, ES.AUTO))
    print(name, "default", d, "auto", a, "ratio %.5f" % (a / d))
    assert a <= d * 1.001, (name, a, d)


@pytest.mark.parametrize("name", KINDS)
def test_auto_modes(name):
    modes = _lz(name, ES.AUTO)[2]
    if name in NOISY:
        assert (modes == 1).all(), (name, modes)
    if name in STRUCTURED:
        assert (modes == 0).all(), (name, modes)
    # AUTO's segments are DEFAULT's where parsed and HUFFMAN_ONLY's where not
    h, m, _ = _lz(name, ES.AUTO)
    for st, sel in ((ES.DEFAULT, modes == 0), (ES.HUFFMAN_ONLY, modes == 1)):
        hs, ms, _ = _lz(name, st)
        assert (h[sel] == hs[sel]).all() and (m[sel] == ms[sel]).all(), (name, st)


@pytest.mark.parametrize("name", KINDS)
def test_rule_restated_in_numpy(name):
    _, stream, rowlen = _tiles()[name]
    want = [mode for _, _, mode in ES.rule_numpy(stream, rowlen)]
    assert _lz(name, ES.AUTO)[2].tolist() == want, name


def test_rule_restated_on_short_and_odd_streams():
    """Streams around the sample's edges: empty, shorter than 6 bytes (no sample: parsed), a
    last segment ending in a partial chunk, rows longer than the window, runs and noise."""
    rng = np.random.default_rng(9)
    for n, rowlen in ((0, 3), (1, 2), (5, 3), (6, 3), (37, 5), (16384 + 6, 129), (16384 * 2 + 45, 1025),
                      (40000, 5201), (33000, 257)):
        for kind in ("noise", "runs"):
            s = rng.integers(0, 256, n).astype(np.uint8)
            if kind == "runs":
                s = (np.arange(n) // 40 % 7).astype(np.uint8)
            stream = s.tobytes()
            want = [mode for _, _, mode in ES.rule_numpy(stream, rowlen)]
            _, _, modes = ES.lz77(stream, rowlen, ES.AUTO)
            assert modes.tolist() == want, (n, rowlen, kind)
            for st in ES.STRATEGIES:
                assert zlib.decompress(ES.deflate(stream, rowlen, st)) == stream, (n, rowlen, kind, st)


def test_threshold_pair():
    """One full segment (512 sampled chunks): 10 hits are under 20 per mille (Huffman-only),
    11 are not (parsed)."""
    for want, a, stream in ES.threshold_pair():
        assert len(stream) == 16384 and stream == ES.png_stream(a)
        (hits, sampled, mode), = ES.rule_numpy(stream, 128)
        assert (hits, sampled) == (want, 512)
        assert mode == (1 if want == 10 else 0)
        _, m, modes = ES.lz77(stream, 128, ES.AUTO)
        assert modes.tolist() == [mode]
        assert zlib.decompress(ES.deflate(stream, 128, ES.AUTO)) == stream


def test_strategy_out_of_range():
    L = ES.lib()
    assert L.pbxemu_deflate_strategy(b"abc", 3, 4, 3, None, 0, None, None) == -3
    assert L.pbxemu_lz77_strategy(b"abc", 3, 4, -1, None, None, None) == -3


def test_bad_strategy_is_400_before_any_device_query(monkeypatch):
    """$PBX_DEFLATE_STRATEGY outside 0 / 1 / 2 and a bad ``deflate_strategy=`` keyword are
    refused like a bad png_filter: checked before the device is looked for, so this runs
    without a GPU."""
    import pbx
    for bad in ("3", "-1", "auto", "", "02"):
        monkeypatch.setenv("PBX_DEFLATE_STRATEGY", bad)
        with pytest.raises(pbx.PbxError) as e:
            pbx.PixelsService()
        assert e.value.status == pbx.E_BADARG and "PBX_DEFLATE_STRATEGY" in str(e.value), bad
    monkeypatch.delenv("PBX_DEFLATE_STRATEGY")
    for bad in (3, -1):
        with pytest.raises(pbx.PbxError) as e:
            pbx.PixelsService(deflate_strategy=bad)
        assert e.value.status == pbx.E_BADARG
    assert (pbx.DEFLATE_DEFAULT, pbx.DEFLATE_HUFFMAN_ONLY, pbx.DEFLATE_AUTO) == ES.STRATEGIES
