"""What the Zarr v3 forms cost on the device: kernel_ms[0] (decode + checksum
kernels) and kernel_ms[1] (placement) of one plane registered from each stored form.

  python scripts/zarr3_probe.py forms [side]
      A side^2 (default 16384) uint16 G_NOISE plane and a ramp, each stored as
        v2 zlib 512^2 chunks (the existing path: the baseline), v3 gzip 512^2 chunks (the same
        deflate level), v3 zstd-3 512^2 whole chunks, v3 2048^2 shards of 128^2 zstd-3 inner
        chunks (to the C-ABI: a 128^2 chunk grid), blosc-zstd5 512^2 chunks (the existing
        frame-per-split form), raw 512^2 chunks with and without the crc32c flag (the difference
        is k_zarr_crc alone).
      Prints GB/s of decoded bytes for each.
  python scripts/zarr3_probe.py crc [side]
      k_zarr_crc alone at five range lengths (4, 32, 64, 128 and 512 KiB raw chunks of a side^2
      plane, default 8192): raw chunks with the crc32c flag minus plain raw chunks.  Run it with
      PBX_ZARR_CRC_SPLIT=1 (a workgroup per range) and =2147483647 (a wave per range) to place
      the split.
"""
import os
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("PBX_PKG") or os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
import _zarr  # noqa: E402
import _zarr3 as Z3  # noqa: E402
import pbx  # noqa: E402

REPS, LEVEL = 3, 5


def crc32c_many(rows: np.ndarray) -> np.ndarray:
    """CRC-32C of every row of a 2-D uint8 array, all rows at once: the rows are cut into pieces
    that run through the byte table side by side, and the pieces' registers are folded with the
    linear map "append one piece of zeros" (the table update is linear over GF(2) in register
    and data)."""
    Z3.crc32c(b"")
    tab = np.array(Z3._TABLE, dtype=np.uint32)
    n, length = rows.shape
    piece = 1
    while piece * 2 <= 4096 and length % (piece * 2) == 0:
        piece *= 2
    k = length // piece
    cols = np.ascontiguousarray(rows.reshape(n * k, piece).T)  # cols[j] = byte j of every piece
    reg = np.zeros(n * k, dtype=np.uint32)
    reg[::k] = 0xFFFFFFFF  # a row's first piece carries the initial value
    for j in range(piece):
        reg = tab[(reg ^ cols[j]) & 0xFF] ^ (reg >> 8)
    basis = (np.uint32(1) << np.arange(32, dtype=np.uint32))
    for _ in range(piece):  # the images of the 32 register bits under `piece` zero bytes
        basis = tab[basis & 0xFF] ^ (basis >> 8)
    reg = reg.reshape(n, k)
    acc = reg[:, 0].copy()
    for i in range(1, k):
        nxt = reg[:, i].copy()
        for b in range(32):
            nxt ^= np.where((acc >> np.uint32(b)) & 1, basis[b], np.uint32(0)).astype(np.uint32)
        acc = nxt
    return acc ^ np.uint32(0xFFFFFFFF)


def pool_map(fn, items):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(fn, items))


def raw_chunks(plane, cy, cx):
    return [c.tobytes() for c in _zarr.chunk_grid(plane, cy, cx)]


def with_crcs(raws):
    a = np.frombuffer(b"".join(raws), np.uint8).reshape(len(raws), -1)
    crcs = crc32c_many(a)
    return [r + int(c).to_bytes(4, "little") for r, c in zip(raws, crcs)]


def time_form(svc, name, plane, cy, cx, codec, chunks, crc32c=False, base_ms=None):
    side_y, side_x = plane.shape
    packed = pbx.pack_chunks(chunks)
    dec, plc = [], []
    for r in range(REPS + 1):
        pid, (md, mp) = svc.register_zarr_plane(77, 0, 0, 0, pbx.UINT16, side_x, side_y, cx, cy, codec, packed,
                                                big_endian=False, timing=True, crc32c=crc32c)
        if r:
            dec.append(md), plc.append(mp)
        if r == REPS:
            got = np.frombuffer(svc.read_plane_be(pid, plane.nbytes), ">u2").reshape(plane.shape)
            assert np.array_equal(got, plane), name
        svc.release_plane(pid)
    md, mp = min(dec), min(plc)
    extra = "" if base_ms is None else "  (+%.3f ms over plain raw)" % (md - base_ms)
    print("%-34s %7.1f MB in %6d chunks: decode+checks %8.3f ms = %7.1f GB/s decoded, place %.3f ms%s   [%s]"
          % (name, len(packed[0]) / 1e6, len(chunks), md, plane.nbytes / md / 1e6, mp, extra,
             " ".join("%.3f" % v for v in dec)), flush=True)
    return md


def planes(svc, side):
    pid = svc.register_plane(76, 0, 0, 0, pbx.UINT16, side, side, generator="noise", plane_no=0)
    noise = np.frombuffer(svc.read_plane_be(pid, side * side * 2), ">u2").reshape(side, side).astype("<u2")
    svc.release_plane(pid)
    y, x = np.mgrid[0:side, 0:side]
    ramp = ((x + y) & 0xFFFF).astype("<u2")
    return (("noise", noise), ("ramp", ramp))


def forms(side):
    with pbx.PixelsService(device=0) as svc:
        for label, plane in planes(svc, side):
            print("--- %s %d^2 uint16" % (label, side), flush=True)
            raws = raw_chunks(plane, 512, 512)
            time_form(svc, "v2 zlib-%d 512^2" % LEVEL, plane, 512, 512, "zlib",
                      pool_map(lambda b: zlib.compress(b, LEVEL), raws))
            time_form(svc, "v3 gzip-%d 512^2" % LEVEL, plane, 512, 512, "gzip",
                      pool_map(lambda b: Z3.gzip_member(b, LEVEL), raws))
            time_form(svc, "v3 zstd-3 512^2 whole chunks", plane, 512, 512, "zstd",
                      pool_map(lambda b: _zarr.zstd_frame(b, 3), raws))
            time_form(svc, "v3 shards: 128^2 zstd-3 inner", plane, 128, 128, "zstd",
                      pool_map(lambda b: _zarr.zstd_frame(b, 3), raw_chunks(plane, 128, 128)))
            time_form(svc, "blosc-zstd5 512^2", plane, 512, 512, "blosc",
                      pool_map(lambda b: _zarr.blosc_encode(b, 2, clevel=5, codec="zstd"), raws))
            base = time_form(svc, "raw 512^2", plane, 512, 512, None, raws)
            time_form(svc, "raw 512^2 + crc32c", plane, 512, 512, None, with_crcs(raws), crc32c=True, base_ms=base)


def crc(side):
    print("PBX_ZARR_CRC_SPLIT=%s" % os.environ.get("PBX_ZARR_CRC_SPLIT", "(default)"), flush=True)
    with pbx.PixelsService(device=0) as svc:
        plane = planes(svc, side)[0][1]
        for cy, cx in ((32, 64), (128, 128), (128, 256), (256, 256), (512, 512)):
            raws = raw_chunks(plane, cy, cx)
            base = time_form(svc, "raw %dx%d" % (cx, cy), plane, cy, cx, None, raws)
            time_form(svc, "raw %dx%d + crc32c" % (cx, cy), plane, cy, cx, None, with_crcs(raws), crc32c=True,
                      base_ms=base)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else ""
    if which == "forms":
        forms(int(sys.argv[2]) if len(sys.argv) > 2 else 16384)
    elif which == "crc":
        crc(int(sys.argv[2]) if len(sys.argv) > 2 else 8192)
    else:
        sys.exit(__doc__)
