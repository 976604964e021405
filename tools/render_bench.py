"""Views per second of the asset renderer (include/gpn.h section RD, gapartnet_amd/dataset/render_assets.py) on fixture asset
45780 (2080 vertices, 5384 triangles), 16 views of 800 x 800:
  (a) the setup, raster and annotate entry points, each between its own pair of device events (tables already on the device)
  (b) the whole render_views call on the GPU (host tables, uploads, kernels, ONE device-to-host copy)
  (c) the package's vectorised numpy path on the same views, one view per process over 16 processes
  (d) the CLI on files (render_dataset: parse, render, write on host threads)
Medians of --reps runs; (b) and (c) alternate.  There is no earlier renderer in this repository: (c) is the baseline.

--shading textured measures section RS instead (the result is appended to --out under its own heading): the same views of the
same asset with generated 1024 x 1024 textures written where its materials' map_Kd lines point,
  (e) the shade entry point between its own device events next to setup / raster / annotate, a flat and a textured batch taking
      turns
  (f) the whole render_views(shading="textured") call on the GPU against (g) the numpy path of the same contract, taking turns

    python tools/render_bench.py [--views 16] [--size 800] [--reps 7] [--out profiles/render_bench.txt] [--shading textured]
"""
import argparse
import multiprocessing as mp
import os
import shutil
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
TEXTURED = "# --shading textured"
TEX_SIZE = 1024


def _numpy_view_textured(job):
    global _ASSET
    if _ASSET is None:
        _ASSET = RA.load_asset(ASSET, textures=True)
    req, size = job
    return int(RA.render_views([_ASSET], [req], size, size, device="cpu", shading="textured")[0].rgb.sum())


def textured_copy(src, tmp):
    """a copy of the asset with a generated TEX_SIZE^2 image (a colour ramp under noise) at every file its map_Kd lines name"""
    from PIL import Image
    dst = os.path.join(tmp, "asset")
    shutil.copytree(src, dst)
    files = set()
    for name in sorted(os.listdir(os.path.join(dst, "textured_objs"))):
        if name.endswith(".mtl"):
            files |= {m["map_Kd"] for m in RA.read_mtl_textured(os.path.join(dst, "textured_objs", name)).values() if m["map_Kd"]}
    rng = np.random.default_rng(0)
    ys, xs = np.mgrid[0:TEX_SIZE, 0:TEX_SIZE]
    for i, f in enumerate(sorted(files)):
        img = np.stack([xs // 4, ys // 4, (xs + ys) // 8], -1) + rng.integers(0, 64, (TEX_SIZE, TEX_SIZE, 3)) + 16 * i
        os.makedirs(os.path.dirname(f), exist_ok=True)
        Image.fromarray((img % 256).astype(np.uint8)).save(f)
    return dst, len(files)


def textured_leg(a, pool_of, tmp):
    """(e), (f), (g) -> lines"""
    global ASSET
    ASSET, n_files = textured_copy(ASSET, tmp)
    pool = pool_of()  # (before the GPU is opened: the workers never touch it)
    import torch
    from gapartnet_amd import hip_ops
    assert torch.cuda.is_available(), "render_bench measures the GPU path: no GPU, no number"
    dev = torch.device("cuda:0")
    V, S = a.views, a.size
    asset = RA.load_asset(ASSET, textures=True)
    rng = np.random.RandomState(0)
    reqs = [RA.RenderRequest(0, RA.sample_qpos(asset, rng), RA.sample_camera(RA.DEFAULT_CAMERA_RANGE, rng)) for _ in range(V)]
    g = RA.geometry_tables([asset])
    t, _ = RA.view_tables([asset], reqs, S, S)
    lines = [TEXTURED, f"# asset 45780 with {len(asset.textures)} generated textures of {TEX_SIZE} x {TEX_SIZE} ({n_files} files named by its "
             f"map_Kd lines, {int((asset.tri_tex >= 0).sum())} of {len(asset.tris)} triangles textured), {t['lights'].shape[1]} lights, {V} views "
             f"of {S} x {S}, medians of {a.reps}, {torch.cuda.get_device_name(dev)}"]

    def log(s):
        print(s, flush=True)
        lines.append(s)

    med = lambda xs: float(np.median(xs))
    gd = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in g.items()}
    td = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in t.items() if isinstance(x, np.ndarray)}
    layout, total = hip_ops.render_layout(V, S, S, t["link_cat"].shape[1])
    buf = torch.empty((total,), dtype=torch.uint8, device=dev)
    for mode in RA.SHADINGS:  # warm-up: code objects, workspace
        hip_ops.render_batch(gd, td, S, S, t["Nt_max"], RA.BACKGROUND_RGB, buf=buf, shading=mode)
    torch.cuda.synchronize()
    RA.render_views([asset], reqs[:2], S, S, device=dev, shading="textured")
    pool.map(_numpy_view_textured, [(r, 64) for r in reqs])  # every worker has parsed the asset and decoded its textures
    ms = {m: [] for m in RA.SHADINGS}
    for _ in range(a.reps):
        for mode in RA.SHADINGS:
            ev = []
            hip_ops.render_batch(gd, td, S, S, t["Nt_max"], RA.BACKGROUND_RGB, timings=ev, buf=buf, shading=mode, check_tables=False)
            torch.cuda.synchronize()
            ms[mode].append([x.elapsed_time(y) for x, y in ev])
    flat = [med([m[i] for m in ms["flat"]]) for i in range(3)]
    lit = [med([m[i] for m in ms["textured"]]) for i in range(4)]
    log(f"(e) kernels, batch of {V}, textured: setup {lit[0]:.3f} ms, raster {lit[1]:.3f} ms, annotate {lit[2]:.3f} ms, shade {lit[3]:.3f} ms, "
        f"sum {sum(lit):.3f} ms = {V / sum(lit) * 1e3:.0f} views/s; flat in the same turns: {flat[0]:.3f} + {flat[1]:.3f} + {flat[2]:.3f} = "
        f"{sum(flat):.3f} ms")
    f = hip_ops.render_fields(buf.cpu(), layout)
    covered = float((f["tri"] >= 0).float().mean())
    px_n = V * S * S
    log(f"    shade: {px_n * covered / lit[3] / 1e6:.1f} M shaded pixels/ms; it reads 8 B (tri, depth) and writes 3 B per pixel = "
        f"{px_n * 11 / lit[3] / 1e6:.1f} GB/s of image traffic, plus per drawn pixel the triangle's rows and four texels "
        f"({covered * 100:.0f} % of the pixels drawn)")
    tb, tc = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        RA.render_views([asset], reqs, S, S, device=dev, shading="textured")
        tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        pool.map(_numpy_view_textured, [(r, S) for r in reqs], chunksize=1)
        tc.append(time.perf_counter() - t0)
    log(f"(f) render_views(shading='textured') on the GPU (tables, uploads incl. {g['tex_data'].nbytes / 1e6:.1f} MB of texels, kernels, one "
        f"copy back), {V} views: {med(tb) * 1e3:.1f} ms = {V / med(tb):.1f} views/s  (min {min(tb) * 1e3:.1f}, max {max(tb) * 1e3:.1f} ms)")
    log(f"(g) numpy path of the same contract, {V} views over {a.procs} processes: {med(tc) * 1e3:.0f} ms = {V / med(tc):.2f} views/s  "
        f"(min {min(tc) * 1e3:.0f}, max {max(tc) * 1e3:.0f} ms)")
    log(f"(f) / (g) = {med(tc) / med(tb):.1f}x;  kernels alone / (g) = {med(tc) * 1e3 / sum(lit):.0f}x")
    pool.close()
    return lines


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
    ap.add_argument("--shading", default="flat", choices=RA.SHADINGS)
    a = ap.parse_args()
    global ASSET
    ASSET = render_ref.fixture_asset()
    if a.shading == "textured":
        with tempfile.TemporaryDirectory() as tmp:
            lines = textured_leg(a, lambda: mp.get_context("fork").Pool(a.procs), tmp)
        old = []
        if os.path.exists(a.out):
            with open(a.out) as fh:
                old = fh.read().split("\n")
            old = old[:old.index(TEXTURED)] if TEXTURED in old else old
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join([x for x in old if x] + lines) + "\n")
        return
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
