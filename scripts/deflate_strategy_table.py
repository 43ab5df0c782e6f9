"""Bytes per tile of the three deflate strategies (pbx_set_deflate_strategy) on ten seeded
512 x 512 tile kinds, from the CPU emulator (lib/libpbx_emu.so: the bytes the GPU writes),
next to zlib level 6 and zlib Z_HUFFMAN_ONLY on the same filter-None PNG scanlines, and AUTO's
Huffman-only segment count.  CPU only; prints the markdown table of DESIGN.md §2."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _emu_strategy as ES  # noqa: E402


def main():
    print("| tile kind | default | Huffman-only | auto (20 per mille) | auto: Huffman-only segments | zlib-6 | zlib Z_HUFFMAN_ONLY |")
    print("|---|---|---|---|---|---|---|")
    for name, a in ES.tile_kinds():
        stream = ES.png_stream(a)
        rowlen = 1 + a.shape[1] * a.dtype.itemsize
        n = [len(ES.deflate(stream, rowlen, st)) for st in ES.STRATEGIES]
        modes = ES.lz77(stream, rowlen, ES.AUTO)[2]
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        zh = len(c.compress(stream) + c.flush())
        print("| %s | %s | %s | %s | %d / %d | %s | %s |" % (
            name, *("{:,}".format(v) for v in n), int(modes.sum()), len(modes),
            "{:,}".format(len(zlib.compress(stream, 6))), "{:,}".format(zh)))


if __name__ == "__main__":
    main()
