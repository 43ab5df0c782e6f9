"""The deflate chain under each strategy (pbx_set_deflate_strategy) on G_NOISE, G_FAKE and the
Poisson-like plane of scripts/poisson_probe.py: 4096 x 512^2 uint16 PNG tiles a batch, filter
None, serial kernel stream (set_kernel_streams(1, 0): per-kernel HIP-event times without
overlap) -- ms_lz77 / ms_huff / ms_encode / ms_deflate, bytes per tile, and how many segments
AUTO coded Huffman-only.  Prints one line per plane and strategy; needs the GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
import pbx  # noqa: E402

side = 32768
REPS = int(os.environ.get("PBX_PROBE_REPS", "5"))
PLANES = os.environ.get("PBX_PROBE_PLANES", "G_NOISE,G_FAKE,poisson").split(",")  # (one plane under rocprofv3)
yy, xx = np.mgrid[0:side:64, 0:side:64]
lam = 200.0 + 100.0 * (0.5 + 0.25 * np.sin(xx / 900.0) + 0.25 * np.cos(yy / 1300.0))
gen = torch.Generator(device="cuda").manual_seed(1234)
lam_t = torch.from_numpy(lam.astype(np.float32)).cuda().repeat_interleave(64, 0).repeat_interleave(64, 1)
pois = torch.poisson(lam_t, generator=gen).to(torch.int16).cpu().numpy().view(np.uint16)
del lam_t
torch.cuda.empty_cache()
names = {pbx.DEFLATE_DEFAULT: "default", pbx.DEFLATE_HUFFMAN_ONLY: "huffman-only", pbx.DEFLATE_AUTO: "auto"}
with pbx.PixelsService(device=0) as svc:
    svc.set_kernel_streams(1, 0)
    svc.register_plane(1, 0, 0, 0, pbx.UINT16, side, side, generator="noise")
    svc.register_plane(2, 0, 0, 0, pbx.UINT16, side, side, generator="fake")
    svc.register_plane(3, 0, 0, 0, pbx.UINT16, side, side, data=pois, big_endian=False)
    for iid, plane in ((1, "G_NOISE"), (2, "G_FAKE"), (3, "poisson")):
        if plane not in PLANES:
            continue
        reqs = pbx.make_reqs([pbx.TileCtx(iid, 0, 0, 0, (i % 64) * 512, (i // 64) * 512, 512, 512, format="png")
                              for i in range(4096)])
        for rnd in range(2):  # every strategy twice, alternating: the spread of a repeat
            for strat in (pbx.DEFLATE_DEFAULT, pbx.DEFLATE_HUFFMAN_ONLY, pbx.DEFLATE_AUTO):
                svc.set_deflate_strategy(strat)
                rows = []
                for k in range(REPS + 1):
                    b = pbx.Batch(svc, reqs=reqs)
                    b.launch()
                    b.sync()
                    st = b.stats()
                    if k:  # (the first launch warms the pools)
                        rows.append((st.ms_lz77, st.ms_huff, st.ms_encode, st.ms_deflate, st.ms_total))
                    ho = int(b.lz_modes().sum())
                    b.close()
                m, lo, hi = np.mean(rows, 0), np.min(rows, 0), np.max(rows, 0)
                print(f"{plane:8s} {names[strat]:13s} run {rnd} lz77 {m[0]:.3f} [{lo[0]:.3f}-{hi[0]:.3f}] huff {m[1]:.3f} "
                      f"encode {m[2]:.3f} [{lo[2]:.3f}-{hi[2]:.3f}] deflate {m[3]:.3f} [{lo[3]:.3f}-{hi[3]:.3f}] "
                      f"total {m[4]:.3f} ms  {st.deflate_out_bytes / 4096:.0f} B/tile  huffman-only segments "
                      f"{ho} / {st.segments}", flush=True)
