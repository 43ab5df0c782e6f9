"""ctypes binding of the emulator's deflate-strategy entry points (lib/libpbx_emu.so:
pbxemu_deflate_strategy, pbxemu_lz77_strategy) and the ten seeded tile kinds the strategy
tests and scripts/deflate_strategy_table.py share."""
import ctypes

import numpy as np

import _emu

DEFAULT, HUFFMAN_ONLY, AUTO = 0, 1, 2
STRATEGIES = (DEFAULT, HUFFMAN_ONLY, AUTO)

_bound = False


def lib():
    global _bound
    L = _emu.lib()
    if not _bound:
        L.pbxemu_deflate_strategy.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_emu.SegOut)]
        L.pbxemu_lz77_strategy.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _bound = True
    return L


def deflate(data: bytes, rowlen: int, strategy: int) -> bytes:
    """The zlib stream the GPU pipeline produces for one tile stream under `strategy`."""
    data = bytes(data)
    L = lib()
    n = L.pbxemu_nblocks(len(data))
    segs = (_emu.SegOut * n)()
    out = ctypes.create_string_buffer(len(data) + 1024 + 16 * n)
    ol = ctypes.c_uint64()
    r = L.pbxemu_deflate_strategy(data, len(data), rowlen, strategy, out, len(out), ctypes.byref(ol), segs)
    assert r == 0, r
    return out.raw[: ol.value]


def lz77(data: bytes, rowlen: int, strategy: int):
    """(hist[nseg, 320], mrec[nseg, MREC_WORDS], modes[nseg]) as k_lz77 writes them under
    `strategy`; modes: 0 = parsed, 1 = Huffman-only."""
    data = bytes(data)
    L = lib()
    n = L.pbxemu_nsegs(len(data))
    hw, mw = L.pbxemu_hist_words(), L.pbxemu_mrec_words()
    h = np.zeros(n * hw, np.uint32)
    m = np.zeros(n * mw, np.uint32)
    modes = np.zeros(n, np.uint8)
    r = L.pbxemu_lz77_strategy(data, len(data), rowlen, strategy, h.ctypes.data, m.ctypes.data, modes.ctypes.data)
    assert r == 0, r
    return h.reshape(n, hw), m.reshape(n, mw), modes


def png_stream(a) -> bytes:
    """Filter-None PNG scanlines of a 2-D pixel array: a zero byte, then the row big-endian."""
    be = np.ascontiguousarray(a.astype(a.dtype.newbyteorder(">")))
    rows = be.view(np.uint8).reshape(a.shape[0], -1)
    return np.concatenate([np.zeros((a.shape[0], 1), np.uint8), rows], axis=1).tobytes()


def tile_kinds(h: int = 512, w: int = 512, seed: int = 5):
    """[(name, pixels)]: the ten tile kinds of DESIGN.md §2's strategy table, h x w, seeded."""
    rng = np.random.default_rng(seed)
    u16, u8 = np.uint16, np.uint8
    noise = rng.integers(0, 4096, (h, w)).astype(u16)  # G_NOISE-like: 12 significant bits
    pois250 = rng.poisson(250.0, (h, w)).astype(u16)
    ramp = np.tile(np.arange(w, dtype=u16), (h, 1))  # FakeReader's ramp: the pixel is its column,
    ramp[:10, :50] = 0                               # and the index boxes of its first ten rows
    half = rng.integers(0, 4096, (h, w)).astype(u16)
    half[:, w // 2:] = 0
    eighth = rng.integers(0, 4096, (h, w)).astype(u16)
    eighth[:, w // 8:] = 0
    blob = rng.poisson(250.0, (h, w)).astype(u16)
    blob[h // 4:h // 4 + 60, w // 4:w // 4 + 200] = 65535  # a saturated area
    pois3 = rng.poisson(3.0, (h, w)).astype(u16)
    noise8 = rng.integers(0, 256, (h, w)).astype(u8)
    pois3_8 = rng.poisson(3.0, (h, w)).astype(u8)
    pois30_8 = rng.poisson(30.0, (h, w)).astype(u8)
    return [("noise16", noise), ("poisson250_16", pois250), ("ramp16", ramp), ("noise_half_zero16", half),
            ("noise_7of8_zero16", eighth), ("poisson_blob16", blob), ("poisson3_16", pois3),
            ("noise8", noise8), ("poisson3_8", pois3_8), ("poisson30_8", pois30_8)]


def match_minlen(d: int) -> int:
    return 3 if d <= 256 else 4 if d <= 4096 else 6


def rule_numpy(stream: bytes, rowlen: int):
    """AUTO's per-segment rule restated in numpy, independently of csrc/deflate_seg.h: per
    segment (hits, sampled, mode).  Segments: an equal split of at most 16 KiB rounded up to 16
    bytes; window: one row rounded up to 16 bytes, at most 4 KiB and the bytes before the
    segment.  Sampled: every 32nd position p with p + 6 <= the segment's length; hit: at
    distance 1, 2 or one row (rows longer than 2 bytes), not before the window, the first
    match_minlen bytes repeat; Huffman-only iff hits * 1000 < sampled * 20 and sampled > 0."""
    s = np.frombuffer(bytes(stream), np.uint8)
    n = len(s)
    seg, win = 16384, 4096
    n0 = max(1, -(-n // seg))
    ln = min(seg, (-(-n // n0) + 15) & ~15) if n else 16
    nseg = max(1, -(-n // ln))
    out = []
    for k in range(nseg):
        s0 = k * ln
        sl = min(ln, n - s0)
        wl = min(s0, min(win, (max(rowlen, 2) + 15) & ~15))
        pos = np.arange(0, max(sl - 5, 0), 32)
        hit = np.zeros(len(pos), bool)
        for d in (1, 2) + ((rowlen,) if rowlen > 2 else ()):
            eq = d <= wl + pos
            for j in range(match_minlen(d)):
                eq = eq & (s[s0 + pos + j] == s[np.maximum(s0 + pos + j - d, 0)])
            hit |= eq
        h, m = int(hit.sum()), len(pos)
        out.append((h, m, int(m > 0 and h * 1000 < m * 20)))
    return out


def threshold_pair(seed: int = 77):
    """[(hits, pixels uint8 (128, 127), stream)] for hits = 10 and 11: uint8 noise whose PNG
    stream is one full 16 KiB segment (128 rows of 128 bytes: 512 sampled chunks) with exactly
    that many chunk starts repeating the byte before them three times -- one below and one at
    AUTO's 20 per mille threshold (10 / 512 = 19.5, 11 / 512 = 21.5)."""
    out = []
    for want in (10, 11):
        rng = np.random.default_rng(seed)
        s = rng.integers(0, 256, 128 * 128).astype(np.uint8)
        s[::128] = 0
        planted = [32 * t for t in range(1, 64) if t % 4][:want]  # chunk starts that are no filter byte
        for p in planted:
            s[p:p + 3] = s[p - 1]
        for _ in range(8):  # chance hits of the noise (and of the planted bytes' row-down chunks): break them
            stray = [32 * t for t in range(512) if _chunk_hit(s, 32 * t, 128) and 32 * t not in planted]
            if not stray:
                break
            for p in stray:
                s[p + 1] = (int(s[p + 1]) + 1) % 256
        a = s.reshape(128, 128)[:, 1:].copy()
        out.append((want, a, s.tobytes()))
    return out


def _chunk_hit(s, p, rowlen):
    return any(d <= p and all(s[p + j] == s[p + j - d] for j in range(match_minlen(d))) for d in (1, 2, rowlen))
