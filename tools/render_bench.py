"""Views per second of the asset renderer (include/gpn.h section RD, gapartnet_amd/dataset/render_assets.py) on fixture asset
45780 (2080 vertices, 5384 triangles), 16 views of 800 x 800:
  (a) the setup, raster and annotate entry points, each between its own pair of device events (tables already on the device)
  (b) the whole render_views call on the GPU (host tables, uploads, kernels, ONE device-to-host copy)
  (c) the package's vectorised numpy path on the same views, one view per process over 16 processes
  (d) the CLI on files (render_dataset: parse, render, write on host threads)
Medians of --reps runs; (b) and (c) alternate.  There is no earlier renderer in this repository: (c) is the baseline.

    python tools/render_bench.py [--views 16] [--size 800] [--reps 7] [--out profiles/render_bench.txt]
"""
import argparse
import multiprocessing as mp
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gapartnet_amd.dataset import render_assets as RA  # noqa: E402
from tests import render_ref  # noqa: E402

ASSET = None  # the unpacked fixture (set in main before the workers are forked)
_ASSET = None


def _numpy_view(job):
    global _ASSET
    if _ASSET is None:
        _ASSET = RA.load_asset(ASSET)
    req, size = job
    return RA.render_views([_ASSET], [req], size, size, device="cpu")[0].depth.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.txt"))
    a = ap.parse_args()
    global ASSET
    ASSET = render_ref.fixture_asset()
    pool = mp.get_context("fork").Pool(a.procs)  # (before the GPU is opened: the workers never touch it)
    import torch
    from gapartnet_amd import hip_ops
    assert torch.cuda.is_available(), "render_bench measures the GPU path: no GPU, no number"
    dev = torch.device("cuda:0")
    V, S = a.views, a.size
    asset = RA.load_asset(ASSET)
    rng = np.random.RandomState(0)
    reqs = [RA.RenderRequest(0, RA.sample_qpos(asset, rng), RA.sample_camera(RA.DEFAULT_CAMERA_RANGE, rng)) for _ in range(V)]
    g = RA.geometry_tables([asset])
    t, _ = RA.view_tables([asset], reqs, S, S)
    Nt = len(g["tris"])
    lines = [f"# tools/render_bench.py: asset 45780 ({len(g['verts'])} vertices, {Nt} triangles), {V} views of {S} x {S}, "
             f"medians of {a.reps}, {torch.cuda.get_device_name(dev)}"]

    def log(s):
        print(s, flush=True)
        lines.append(s)

    med = lambda xs: float(np.median(xs))
    gd = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in g.items()}
    td = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in t.items() if isinstance(x, np.ndarray)}
    layout, total = hip_ops.render_layout(V, S, S, t["link_cat"].shape[1])
    buf = torch.empty((total,), dtype=torch.uint8, device=dev)
    hip_ops.render_batch(gd, td, S, S, t["Nt_max"], RA.BACKGROUND_RGB, buf=buf)  # warm-up: code objects, workspace
    torch.cuda.synchronize()
    RA.render_views([asset], reqs[:2], S, S, device=dev)
    pool.map(_numpy_view, [(r, 64) for r in reqs])  # every worker has parsed the asset

    # (a) the three entry points
    ms = []
    for _ in range(a.reps):
        ev = []
        hip_ops.render_batch(gd, td, S, S, t["Nt_max"], RA.BACKGROUND_RGB, timings=ev, buf=buf)
        torch.cuda.synchronize()
        ms.append([x.elapsed_time(y) for x, y in ev])
    setup, raster, annotate = (med([m[i] for m in ms]) for i in range(3))
    kern = setup + raster + annotate
    log(f"(a) kernels, batch of {V}: setup {setup:.3f} ms, raster {raster:.3f} ms, annotate {annotate:.3f} ms, sum {kern:.3f} ms = "
        f"{V / kern * 1e3:.0f} views/s; raster share {raster / kern * 100:.0f} %")
    tiles = ((S + 15) // 16) ** 2
    f = hip_ops.render_fields(buf.cpu(), layout)
    drawn = int(V * Nt - int(f["counters"].sum()))
    log(f"    triangle scan: {tiles} tiles x {Nt} boxes x 8 B = {tiles * Nt * 8 / 1e6:.1f} MB of (cached) box reads per view, plus one "
        f"64-B record per (tile, overlapping triangle); {drawn / V:.0f} of {Nt} triangles drawn per view, "
        f"{float((f['depth'] > 0).float().mean()) * 100:.0f} % of the pixels covered")

    # (b) / (c) alternating
    tb, tc = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        RA.render_views([asset], reqs, S, S, device=dev)
        tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        pool.map(_numpy_view, [(r, S) for r in reqs], chunksize=1)
        tc.append(time.perf_counter() - t0)
    log(f"(b) render_views on the GPU (tables, uploads, kernels, one copy back), {V} views: {med(tb) * 1e3:.1f} ms = "
        f"{V / med(tb):.1f} views/s  (min {min(tb) * 1e3:.1f}, max {max(tb) * 1e3:.1f} ms)")
    log(f"(c) numpy path, {V} views over {a.procs} processes: {med(tc) * 1e3:.0f} ms = {V / med(tc):.2f} views/s  "
        f"(min {min(tc) * 1e3:.0f}, max {max(tc) * 1e3:.0f} ms)")
    log(f"(b) / (c) = {med(tc) / med(tb):.1f}x;  kernels alone / (c) = {med(tc) * 1e3 / kern:.0f}x")

    # (d) the CLI on files
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data"))
        os.symlink(ASSET, os.path.join(tmp, "data", "45780"))
        with open(os.path.join(tmp, "ids.txt"), "w") as fd:
            fd.write("StorageFurniture 45780\n")
        td_, st = [], None
        for i in range(a.reps):
            t0 = time.perf_counter()
            st = RA.render_dataset("partnet", os.path.join(tmp, "data"), os.path.join(tmp, "ids.txt"), [45780], V,
                                   os.path.join(tmp, f"out{i}"), None, S, S, 16, 0, dev, workers=16, echo=False)
            td_.append(time.perf_counter() - t0)
        log(f"(d) CLI on files, {V} views, --batch 16, 16 writer threads: {med(td_):.2f} s = {V / med(td_):.1f} views/s "
            f"(render_views {st['render_s']:.2f} s of the last run; the rest is parsing and png / npz compression)")
    pool.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
