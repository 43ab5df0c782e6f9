"""The TIFF predictor pass (pbx_set_tiff_predictor: k_tiff_pred3 / k_tiff_pred) and what it does
to the deflate chain: 4096 x 512^2 uint16 deflate-TIFF tiles a batch on G_NOISE, G_FAKE, the
Poisson plane of scripts/poisson_probe.py and a smooth scene (Poisson counts of a smooth lambda
field), serial kernel stream (set_kernel_streams(1, 0): per-kernel HIP-event times without
overlap).  Predictor off / on x strategy DEFAULT / AUTO in one process, the settings alternated,
three rounds: the staging pass (ms_filter: the predictor kernel; nothing with the predictor off,
where k_lz77 reads the plane) and its share of HBM peak over 2 x tile bytes, k_lz77, k_encode,
the chain, bytes per tile.  Yardsticks in the same run: k_filter3 Sub (PNG) on the same tiles
for the fast kernel, k_rows (PNG filter None at x + 3) beside the general kernel on the same
unaligned tiles.  Prints one line per measurement; needs the GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
import pbx  # noqa: E402

side = 32768
REPS = int(os.environ.get("PBX_PROBE_REPS", "3"))
ROUNDS = int(os.environ.get("PBX_PROBE_ROUNDS", "3"))
PLANES = os.environ.get("PBX_PROBE_PLANES", "G_NOISE,G_FAKE,poisson,scene").split(",")
HBM_PEAK = 8.0e12  # bytes / s (MI355X)
TILE_BYTES = 4096 * 512 * 512 * 2


def poisson_plane(lam64):
    """uint16 Poisson counts of a lambda field given on a 64-sample grid (drawn on the GPU)."""
    gen = torch.Generator(device="cuda").manual_seed(1234)
    lam_t = torch.from_numpy(lam64.astype(np.float32)).cuda().repeat_interleave(64, 0).repeat_interleave(64, 1)
    out = torch.poisson(lam_t, generator=gen).to(torch.int16).cpu().numpy().view(np.uint16)
    del lam_t
    torch.cuda.empty_cache()
    return out


yy, xx = np.mgrid[0:side:64, 0:side:64]
host = {}
if "poisson" in PLANES:
    host["poisson"] = poisson_plane(200.0 + 100.0 * (0.5 + 0.25 * np.sin(xx / 900.0) + 0.25 * np.cos(yy / 1300.0)))
if "scene" in PLANES:  # tests/_tiff_pred.py smooth_scene's field, lambda 50..430
    host["scene"] = poisson_plane(np.clip(240.0 + 110.0 * np.sin(xx / 83.0 + 0.3) * np.cos(yy / 61.0) +
                                          80.0 * np.sin((xx + 2 * yy) / 190.0), 50.0, 430.0))


def tiles(iid, fmt, dx=0):
    cols = 63 if dx else 64  # (x + dx + 512 stays inside the plane; a few tiles then repeat)
    return pbx.make_reqs([pbx.TileCtx(iid, 0, 0, 0, (i % cols) * 512 + dx, (i // 64) * 512, 512, 512, format=fmt)
                          for i in range(4096)])


def run(svc, reqs):
    rows = []
    for k in range(REPS + 1):
        b = pbx.Batch(svc, reqs=reqs)
        routing = b.pred_tiles()
        b.launch()
        b.sync()
        st = b.stats()
        if k:  # (the first launch warms the pools)
            rows.append((st.ms_filter, st.ms_lz77, st.ms_encode, st.ms_deflate, st.ms_total))
        b.close()
    return np.mean(rows, 0), np.min(rows, 0), np.max(rows, 0), st.deflate_out_bytes / 4096, routing


def line(plane, what, r):
    m, lo, hi, bpt, routing = r
    share = 2 * TILE_BYTES / (m[0] * 1e-3) / HBM_PEAK if m[0] > 0.05 else 0.0
    print(f"{plane:8s} {what:34s} pass {m[0]:.3f} [{lo[0]:.3f}-{hi[0]:.3f}] ms ({share:.3f} of HBM peak)  "
          f"lz77 {m[1]:.3f} [{lo[1]:.3f}-{hi[1]:.3f}] encode {m[2]:.3f} chain {m[3]:.3f} [{lo[3]:.3f}-{hi[3]:.3f}] "
          f"total {m[4]:.3f} ms  {bpt:.0f} B/tile  fast/general tiles {routing[0]}/{routing[1]}", flush=True)


pnames = {pbx.TIFF_PREDICTOR_NONE: "off", pbx.TIFF_PREDICTOR_HORIZONTAL: "on"}
snames = {pbx.DEFLATE_DEFAULT: "default", pbx.DEFLATE_AUTO: "auto"}
with pbx.PixelsService(device=0, tiff_deflate=True) as svc, \
        pbx.PixelsService(device=0, png_filter=pbx.FILTER_SUB) as sub, pbx.PixelsService(device=0) as none:
    for s in (svc, sub, none):
        s.set_kernel_streams(1, 0)
    for iid, plane in enumerate(("G_NOISE", "G_FAKE", "poisson", "scene"), 1):
        if plane not in PLANES:
            continue
        for s in (svc, sub, none):
            if plane in host:
                s.register_plane(iid, 0, 0, 0, pbx.UINT16, side, side, data=host[plane], big_endian=False)
            else:
                s.register_plane(iid, 0, 0, 0, pbx.UINT16, side, side, generator="noise" if plane == "G_NOISE" else "fake")
        tif, png, tif_u, png_u = tiles(iid, "tif"), tiles(iid, "png"), tiles(iid, "tif", 3), tiles(iid, "png", 3)
        for rnd in range(ROUNDS):
            for strat in (pbx.DEFLATE_DEFAULT, pbx.DEFLATE_AUTO):
                for pred in (pbx.TIFF_PREDICTOR_NONE, pbx.TIFF_PREDICTOR_HORIZONTAL):
                    svc.set_deflate_strategy(strat)
                    svc.set_tiff_predictor(pred)
                    line(plane, f"round {rnd} predictor {pnames[pred]:3s} {snames[strat]}", run(svc, tif))
            line(plane, f"round {rnd} k_filter3 Sub (PNG)", run(sub, png))
            svc.set_deflate_strategy(pbx.DEFLATE_DEFAULT)
            svc.set_tiff_predictor(pbx.TIFF_PREDICTOR_HORIZONTAL)
            line(plane, f"round {rnd} predictor on, x + 3 (general)", run(svc, tif_u))
            line(plane, f"round {rnd} k_rows, x + 3 (PNG None)", run(none, png_u))
        for s in (svc, sub, none):
            s.release_image(iid)
