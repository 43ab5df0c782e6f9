"""Bit-packed TIFF samples and PackBits, restated in numpy for the tests of the pbx_*_tiff_packed
calls (tests/test_tiff_packed_host.py, tests/test_gpu_tiff_packed.py).

A segment row of n samples of `bits` bits is a bit stream, most significant bit first whatever the
file's byte order, padded to a whole byte; FillOrder 2 reverses the bits of every byte of it.
Samples of 8 bits are bytes and samples of 16 bits two bytes in the FILE's byte order (libtiff's
rule), which for a big-endian file is the same bit stream again.  Bio-Formats, through which the
reference opens such files, unpacks 1 .. 8 bits into uint8 and 9 .. 16 into uint16 without
scaling: `expected_be` is the plane pbx_plane_read_be must return.

No TIFF library on this machine writes or reads 2-, 4-, 10-, 12- or 14-bit samples (PIL reads 1-bit
files of either fill order and 8-bit PackBits ones, which tests/test_tiff_packed_host.py holds
against this file): elsewhere this restatement stands alone, packer and unpacker checked against
each other and against np.packbits."""
import numpy as np

import _tiff_src as T

PACKBITS = 32773
ZSTD = 50000
_REV = np.array([int("{:08b}".format(b)[::-1], 2) for b in range(256)], dtype=np.uint8)


def row_bytes(n, bits):
    return (n * bits + 7) // 8


def pack_rows(a, bits, fill_order=1, byteorder=">"):
    """(rows, n) unsigned values below 2^bits -> (rows, row_bytes(n, bits)) uint8: shift-and-or,
    one output bit at a time.  bits == 16 in a little-endian file: the samples' own bytes."""
    a = np.ascontiguousarray(a).astype(np.uint32)
    rows, n = a.shape
    assert (a >> bits).max(initial=0) == 0
    if bits == 16 and byteorder == "<":
        out = a.astype("<u2").view(np.uint8).reshape(rows, 2 * n)
    else:
        out = np.zeros((rows, row_bytes(n, bits)), dtype=np.uint8)
        pos = np.arange(n, dtype=np.int64) * bits
        for k in range(bits):  # bit k of a sample, counted from its most significant one
            bit = ((a >> (bits - 1 - k)) & 1).astype(np.uint8)
            p = pos + k
            np.bitwise_or.at(out, (slice(None), p >> 3), bit << (7 - (p & 7)).astype(np.uint8))
    return _REV[out] if fill_order == 2 else out


def pack_rows_1bit(a, fill_order=1):
    """The same for bits == 1 by np.packbits (its 'big' bit order is MSB first)."""
    out = np.packbits(np.ascontiguousarray(a).astype(np.uint8), axis=1, bitorder="big")
    return _REV[out] if fill_order == 2 else out


def unpack_rows(buf, rows, n, bits, fill_order=1, byteorder=">"):
    """The inverse, written the other way round (a big integer per row): (rows, n) uint16."""
    b = np.frombuffer(bytes(buf), dtype=np.uint8).reshape(rows, -1)
    if fill_order == 2:
        b = _REV[b]
    if bits == 16 and byteorder == "<":
        return b.copy().view("<u2").astype(np.uint16).reshape(rows, n)
    out = np.zeros((rows, n), dtype=np.uint16)
    nb = b.shape[1] * 8
    for r in range(rows):
        v = int.from_bytes(b[r].tobytes(), "big")
        for i in range(n):
            out[r, i] = (v >> (nb - (i + 1) * bits)) & ((1 << bits) - 1)
    return out


def packbits_encode(data, literal_only=False):
    """TIFF 6.0 section 9: replicate runs of 3 or more equal bytes (up to 128), the rest as
    literals of up to 128 bytes."""
    data = bytes(data)
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i
        while j + 1 < n and data[j + 1] == data[i] and j + 1 - i < 128:
            j += 1
        run = j - i + 1
        if run >= 3 and not literal_only:
            out += bytes([257 - run, data[i]])
            i += run
            continue
        k = i
        while k < n and k - i < 128:
            if not literal_only and k + 2 < n and data[k] == data[k + 1] == data[k + 2]:
                break
            k += 1
        out += bytes([k - i - 1]) + data[i:k]
        i = k
    return bytes(out)


def packbits_decode(stream, expect):
    """The textbook decoder: stops once `expect` bytes are out; ValueError for a stream that ends
    before that or a run that passes it."""
    out, i = bytearray(), 0
    while len(out) < expect:
        if i >= len(stream):
            raise ValueError("stream ends after %d of %d bytes" % (len(out), expect))
        h = stream[i]
        i += 1
        if h == 128:
            continue
        if h < 128:
            piece = stream[i:i + h + 1]
            if len(piece) != h + 1:
                raise ValueError("literal cut short")
            i += h + 1
        else:
            if i >= len(stream):
                raise ValueError("replicate run cut short")
            piece = bytes([stream[i]]) * (257 - h)
            i += 1
        if len(out) + len(piece) > expect:
            raise ValueError("run past the segment's end")
        out += piece
    return bytes(out)


def compress(seg, compression):
    if compression == PACKBITS:
        return packbits_encode(seg)
    if compression == ZSTD:
        import _zarr
        return _zarr.zstd_frame(bytes(seg))
    return T.compress(seg, compression)


def segments_of(a, bits, tile=None, rows_per_strip=None, planar=1, fill_order=1, byteorder=">"):
    """The uncompressed segments of a (rows, width, S) array of values below 2^bits: tiles (edge
    tiles padded with `pad` samples that must never reach a plane: all ones) or strips; chunky
    (sample i of a row is component i % S of pixel i // S) or planar (S groups of segments)."""
    a = np.ascontiguousarray(a)
    h, w, s = a.shape
    groups = [a[:, :, k:k + 1] for k in range(s)] if planar == 2 else [a]
    segs = []
    for g in groups:
        if tile:
            tw, th = tile
            for y in range(0, h, th):
                for x in range(0, w, tw):
                    t = np.full((th, tw, g.shape[2]), (1 << bits) - 1, dtype=a.dtype)
                    piece = g[y:y + th, x:x + tw]
                    t[:piece.shape[0], :piece.shape[1]] = piece
                    segs.append(pack_rows(t.reshape(th, -1), bits, fill_order, byteorder).tobytes())
        else:
            rps = rows_per_strip or h
            for y in range(0, h, rps):
                piece = g[y:y + rps]
                segs.append(pack_rows(piece.reshape(piece.shape[0], -1), bits, fill_order, byteorder).tobytes())
    return segs


def page_of(a, bits, compression=1, tile=None, rows_per_strip=None, planar=1, fill_order=1, byteorder=">",
            photometric=None, sampleformat=1, predictor=1, extra=()):
    """A page for write_tiff from a (rows, width) or (rows, width, S) array of values below 2^bits."""
    a = np.ascontiguousarray(a)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, s = a.shape
    segs = [compress(x, compression) for x in segments_of(a, bits, tile, rows_per_strip, planar, fill_order, byteorder)]
    if photometric is None:
        photometric = 2 if s >= 3 else 1
    tags = [(258, 3, [bits] * s), (339, 3, [sampleformat] * s), (262, 3, [photometric]), (284, 3, [planar])]
    if fill_order != 1:
        tags.append((266, 3, [fill_order]))
    nex = s - (3 if photometric == 2 else 1)
    if nex > 0:
        tags.append((338, 3, [0] * nex))
    own = {t[0] for t in extra}
    return dict(width=w, length=h, bits=bits, sampleformat=sampleformat, spp=s, compression=compression,
                predictor=predictor, tile=tile, rows_per_strip=rows_per_strip or h, segments=segs,
                extra=list(extra) + [t for t in tags if t[0] not in own], _finished=True)


def write_tiff(path, pages, byteorder=">", bigtiff=False):
    """tests/_tiff_src.write_tiff, with each page's own BitsPerSample / SampleFormat / Photometric
    entries in place of that writer's (tests/_tiff_rgb.py drops the first of every pair)."""
    import _tiff_rgb as R
    return R._write(path, pages, byteorder, bigtiff)


def expected_be(a, bits):
    """The plane pbx_plane_read_be returns for a (rows, width) array: uint8, or big-endian uint16."""
    return np.ascontiguousarray(a).astype(np.uint8 if bits <= 8 else ">u2").tobytes()


def noise(rng, h, w, bits, s=None):
    """Uniform values over the whole range of `bits` bits, the extremes included."""
    shape = (h, w) if s is None else (h, w, s)
    a = rng.integers(0, 1 << bits, shape, dtype=np.uint32).astype(np.uint16)
    a.reshape(-1)[:2] = [(1 << bits) - 1, 0]
    return a
