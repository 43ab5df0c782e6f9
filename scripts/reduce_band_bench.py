"""k_reduce_band against the chain of k_downsample launches, on the same rows.

For uint8, uint16 and float and k = 1 .. 4, on a band-shaped generated base (32768 columns x 4096
rows, a dense plane), alternating in one process for three rounds:

  chain   pbx_plane_build_pyramid(levels=k): k launches of k_downsample, each level written to HBM
          and read back by the next (its kernel_ms is printed)
  reduced pbx_band_write_reduced of the whole level k into a sparse plane of one band: k = 1 one
          launch of k_reduce_band1; k >= 2 one launch of k_reduce_band, the base read once, level k
          alone written -- except one-byte samples at k = 2, which go level by level through scratch
          (k_reduce_band1, then k_downsample)

Device times of both come from a kernel trace of this process:

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/reduce_band_bench.py
  python scripts/reduce_band_bench.py --table OUT

The table gives, per type and k, the three chain and three reduced times (microseconds, each the
sum of its kernels), the reduction's base bytes per second and (bytes read + bytes
written) / time as a fraction of the 8 TB/s HBM peak, the figure k_downsample's 0.72-0.77 is.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))

SX, SY, ROUNDS = 32768, 4096, 3
TYPES = [("uint8", 1, 1), ("uint16", 3, 2), ("float", 6, 4)]  # name, pixel type, bytes per sample
PEAK = 8.0e12


def sizes(k):
    w, h = [SX], [SY]
    for _ in range(k):
        w.append((w[-1] + 1) // 2)
        h.append((h[-1] + 1) // 2)
    return w, h


def run():
    import pbx
    with pbx.PixelsService() as svc:
        for n, (name, pt, bpp) in enumerate(TYPES):
            iid = 9100 + n
            svc.declare_image(pbx.Pixels(iid, pt, SX, SY, levels=5))
            base = svc.register_plane(iid, 0, 0, 0, pt, SX, SY, generator="noise", seed=n)
            for rnd in range(ROUNDS):
                for k in (1, 2, 3, 4):
                    ids, ms = svc.build_pyramid(base, k, timing=True)
                    for q in ids:
                        svc.release_plane(q)
                    w, h = sizes(k)
                    dst = svc.create_sparse_plane(iid, 0, 0, 0, pt, w[k], h[k], h[k], k, big_endian=False)
                    svc.band_write_reduced(dst, 0, h[k], base, k)
                    svc.release_plane(dst)
                    print("%s k=%d round %d: chain kernel_ms %.4f" % (name, k, rnd + 1, ms), flush=True)


def reduced_kernels(bpp, k):
    """The kernels one pbx_band_write_reduced launches (launch_reduce_band, kernels_io.hip)."""
    if k == 1:
        return ["k_reduce_band1"]
    if k == 2 and bpp == 1:
        return ["k_reduce_band1", "k_downsample"]  # level by level through scratch
    return ["k_reduce_band<"]


def table(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ev = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
          for r in rows if "k_reduce_band" in r["Kernel_Name"] or "k_downsample" in r["Kernel_Name"]]
    pos = 0

    def take(names):
        nonlocal pos
        us = 0.0
        for want in names:
            name, t = ev[pos]
            assert want in name + "<" and (want != "k_reduce_band<" or "k_reduce_band1" not in name), (pos, want, name)
            us, pos = us + t, pos + 1
        return us

    print("type    k  reduced by                   chain us (3 rounds)          reduced us (3 rounds)        base TB/s  (read+written)/peak  chain (read+written)/peak")
    res = {}
    for name, pt, bpp in TYPES:
        for rnd in range(ROUNDS):
            for k in (1, 2, 3, 4):
                c = take(["k_downsample"] * k)
                f = take(reduced_kernels(bpp, k))
                res.setdefault((name, k), ([], []))[0].append(c)
                res[(name, k)][1].append(f)
    assert pos == len(ev), (pos, len(ev))
    for name, pt, bpp in TYPES:
        for k in (1, 2, 3, 4):
            c, f = res[(name, k)]
            w, h = sizes(k)
            lv = [w[j] * h[j] * bpp for j in range(k + 1)]
            chain_bytes = sum(lv[j] + lv[j + 1] for j in range(k))
            kern = reduced_kernels(bpp, k)
            fused_bytes = chain_bytes if len(kern) > 1 else lv[0] + lv[k]
            fm, cm = sorted(f)[1], sorted(c)[1]
            print("%-7s %d  %-28s %-28s %-28s %6.2f     %.3f                %.3f" % (
                name, k, "+".join(x.rstrip("<") for x in kern), " ".join("%8.1f" % x for x in c),
                " ".join("%8.1f" % x for x in f), lv[0] / (fm * 1e-6) / 1e12, fused_bytes / (fm * 1e-6) / PEAK,
                chain_bytes / (cm * 1e-6) / PEAK))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        run()
