"""Views per second of the rendered-views converter on 800 x 800 synthetic views (~2.5 x 10^5 valid pixels) at 20 000 samples:
  (a) the three launches of include/gpn.h section VP for a batch of views (hip_ops.view_convert, inputs already on the device)
  (b) a loop over the per-view gpn_pn2_furthest_point_sampling_ws plus torch glue (back-projection, gather, normalisation)
  (c) the CLI on files (python -m gapartnet_amd.dataset.convert_rendered), split into read / GPU / write time

    python tools/convert_bench.py [--views 64] [--num_points 20000] [--out profiles/convert_bench.txt]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gapartnet_amd import hip_ops  # noqa: E402
from gapartnet_amd.dataset import convert_rendered as CR  # noqa: E402
from tests import render_views as RV  # noqa: E402


def torch_glue_view(depth, rgb, sem, ins, npcs, K, m):
    """(b): one view: back-projection and compaction in torch, FPS through the existing per-view entry point, the rest in torch"""
    valid = (sem != -2) & (ins != -2)
    ys, xs = torch.nonzero(valid, as_tuple=True)
    z = depth[ys, xs].double()
    pts = torch.stack([((xs.double() - K[0, 2]) * z) / K[0, 0], ((ys.double() - K[1, 2]) * z) / K[1, 1], z], 1)
    idx = hip_ops.pn2_furthest_point_sampling(pts.float()[None], m)[0].long()
    s = pts[idx]
    center = (s.max(0).values + s.min(0).values) / 2
    r = ((s - center) ** 2).sum(1).max().sqrt()
    return ((s - center) / r).float(), (rgb[ys, xs][idx].double() / 255.0).float(), sem[ys, xs][idx] + 1, ins[ys, xs][idx], \
        npcs[ys, xs][idx], torch.stack([ys, xs], 1)[idx].int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--num_points", type=int, default=20000)
    ap.add_argument("--loop_views", type=int, default=8, help="views timed for (b) (it is per view)")
    ap.add_argument("--cli_views", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = a.num_points
    views = [RV.full_size_view(s) for s in range(a.views)]
    keys = ("depth", "rgb", "sem", "ins", "npcs", "K")
    d = {k: torch.from_numpy(np.stack([v[k] for v in views])).to(dev) for k in keys}
    n_valid = [int(((v["sem"] != -2) & (v["ins"] != -2)).sum()) for v in views]
    lines = [f"# tools/convert_bench.py: {a.views} synthetic 800x800 views, {np.mean(n_valid):.0f} valid pixels each, "
             f"{m} samples, {torch.cuda.get_device_name(dev)}"]

    def log(s):
        print(s, flush=True)
        lines.append(s)

    # (a) the three launches, one batch
    hip_ops.view_convert(*(d[k][:2] for k in keys), m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    buf, layout = hip_ops.view_convert(*(d[k] for k in keys), m)
    torch.cuda.synchronize()
    ta = time.perf_counter() - t0
    status = hip_ops.view_fields(buf.cpu(), layout)["status"]
    assert int((status != 0).sum()) == 0
    log(f"(a) three launches, batch of {a.views}: {ta * 1e3:.1f} ms = {a.views / ta:.2f} views/s")

    # (b) per-view loop over the existing FPS entry point + torch glue
    torch_glue_view(*(d[k][0] for k in keys[:5]), d["K"][0], m)
    torch.cuda.synchronize()
    nb = min(a.loop_views, a.views)
    t0 = time.perf_counter()
    for i in range(nb):
        out = torch_glue_view(*(d[k][i] for k in keys[:5]), d["K"][i], m)
        [t.cpu() for t in out]
    tb = time.perf_counter() - t0
    log(f"(b) per-view loop (gpn_pn2_furthest_point_sampling_ws + torch glue), {nb} views: {tb / nb * 1e3:.1f} ms/view = "
        f"{nb / tb:.2f} views/s")
    log(f"(a) / (b) = {(a.views / ta) / (nb / tb):.2f}x")

    # (c) the CLI on files
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "rendered")
        nc = min(a.cli_views, a.views)
        for i in range(nc):
            RV.write_view(data, f"StorageFurniture_{i:05d}_00_000", views[i])
        for batch in (16, 32):
            t0 = time.perf_counter()
            st = CR.convert_directory(data, os.path.join(tmp, f"out{batch}"), num_points=m, batch=batch, workers=16,
                                      log_path=os.path.join(tmp, "log.txt"), echo=False)
            tc = time.perf_counter() - t0
            log(f"(c) CLI, {nc} views, --batch {batch} --workers 16: {tc:.2f} s = {nc / tc:.2f} views/s; read {st['read_s']:.2f} s "
                f"(summed over reader threads), GPU {st['gpu_s']:.2f} s (convert_views incl. copies), write {st['write_s']:.2f} s "
                f"(summed over 2 writer threads), wall {st['wall_s']:.2f} s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
