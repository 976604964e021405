"""Parts of one object from several posed views, stage by stage (gapartnet_amd/misc/multiview.py; csrc/multiview.hip; include/gpn.h
section MV) -> profiles/multiview_bench.txt.

    python tools/multiview_bench.py [--out profiles/multiview_bench.txt] [--reps 5] [--views 8] [--height 720] [--width 1280]

Workload: --views views of --width x --height of one object - a 4 x 4 grid of 16 box-shaped parts in front of a body, ray-cast
from cameras on an arc around it (the renderer's camera_frame), every view numbering the parts in its own order - with about 60 %
valid depth (the workload of tools/frame_bench.py) and 16 parts a view, so GT = 128: the largest table the LDS form of the pair
table takes.  Device-event times in ms, medians of --reps runs, warmed up, the legs taking turns inside every repetition:
  new       every entry point of section MV on its own, gpn_views_overlap in both forms of its pair table (LDS and global, switched by
            gpn_views_overlap_lds_parts), and the whole of fuse_parts without and with the box fit
  baseline  what a user of the parent commit can do on the same GPU: the world transform and the keys by torch ops, torch.unique
            over the same keys, the pair table as a dense occupancy product, one host read, the greedy loop on the host
Both paths' tables and partitions are asserted equal.
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s (MI355X)


def make_views(V, H, W, seed=0, valid=0.6, grid=4):
    """depth f32 [V,H,W] (0 = hole), inst i32 [V,H,W], npcs f32 [V,H,W,3], classes [V][<= grid^2] i64, K, R, t"""
    from gapartnet_amd.dataset.render_assets import camera_frame
    rng = np.random.RandomState(seed)
    boxes = [((-.30, -.50, -.50), (.30, .50, .50))]  # the body: no part
    step = 1.0 / grid
    for r in range(grid):
        for c in range(grid):
            y0, z0 = -.5 + c * step + 0.02, -.5 + r * step + 0.02
            boxes.append(((-.30 - 0.03 - 0.01 * ((r + c) % 3), y0, z0), (-.30, y0 + step - 0.04, z0 + step - 0.04)))
    cls = rng.randint(1, 10, size=len(boxes))
    out = {k: [] for k in ("depth", "inst", "npcs", "classes", "K", "R", "t")}
    for v in range(V):
        a, e = math.radians(180.0 + (v - (V - 1) / 2.0) * 12.0), math.radians(15.0)
        K, R, t = camera_frame(1.9 * np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)]), H, W)
        u, w = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        d = np.stack([(u - K[0, 2]) / K[0, 0], (w - K[1, 2]) / K[1, 1], np.ones_like(u)], -1) @ R.T
        best, which = np.full((H, W), np.inf), np.full((H, W), -1, np.int64)
        with np.errstate(all="ignore"):
            for i, (lo, hi) in enumerate(boxes):
                t0, t1 = (np.asarray(lo) - t) / d, (np.asarray(hi) - t) / d
                near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
                hit = (near <= far) & (near > 0) & (near < best)
                best[hit], which[hit] = near[hit], i
        depth = np.where(which >= 0, best, 2.5).astype(np.float32)
        depth[rng.rand(H, W) >= valid] = 0
        point = t + d * depth.astype(np.float64)[..., None]
        npcs = np.zeros((H, W, 3), np.float32)
        seen = [int(b) for b in np.unique(which[which >= 1])]
        order = [seen[i] for i in rng.permutation(len(seen))]
        local = np.full(len(boxes) + 1, -1, np.int64)
        for j, b in enumerate(order):
            local[b] = j
            lo, hi = np.asarray(boxes[b][0]), np.asarray(boxes[b][1])
            npcs[which == b] = np.clip((point[which == b] - lo) / (hi - lo), 0, 1).astype(np.float32)
        for k, x in (("depth", depth), ("inst", local[which].astype(np.int32)), ("npcs", npcs), ("classes", cls[order].astype(np.int64)),
                     ("K", K), ("R", R), ("t", t)):
            out[k].append(x)
    return {k: (np.stack(x) if k != "classes" else x) for k, x in out.items()}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def fmt(ts):
    return f"{statistics.median(ts):10.3f} [{min(ts):10.3f} .. {max(ts):10.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiview_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--cell", type=float, default=0.01)
    args = ap.parse_args()
    from gapartnet_amd import hip_ops
    from gapartnet_amd.misc import multiview as MV
    dev = torch.device("cuda:0")
    V, H, W, cell = args.views, args.height, args.width, args.cell
    min_inter, min_overlap = 4, 0.25
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    d = make_views(V, H, W)
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    depth, inst, npcs = t(d["depth"]), t(d["inst"]), t(d["npcs"])
    classes = d["classes"]
    n = [len(c) for c in classes]
    GT = sum(n)
    rgb = torch.zeros((V, H, W, 3), dtype=torch.uint8, device=dev)
    Kd, Rd, td = t(d["K"]), t(d["R"]), t(d["t"])
    cls_all = t(np.concatenate(classes).astype(np.int32))
    rows, valid, _ = hip_ops.frame_backproject(depth, rgb, Kd)
    wrows, part_of, area, lo = hip_ops.views_world(rows, valid, inst, n, Rd, td, GT)
    vol, inter, dropped = hip_ops.views_overlap(wrows, part_of, lo, cell, GT)
    m = hip_ops.views_merge(inter, vol, cls_all, n, min_inter, min_overlap)
    fused_inst = hip_ops.views_relabel(part_of, m["fused_of"])
    F = int(m["n_fused"][0])
    fo, ar = m["fused_of"].cpu().numpy(), area.cpu().numpy()
    n_points = np.bincount(fo[fo >= 0], weights=ar[fo >= 0], minlength=F).astype(np.int64)
    seg = torch.from_numpy(np.concatenate([[0], np.cumsum(n_points)])[:-1].astype(np.int64)).to(dev)
    M = int(n_points.sum())
    lds_default = hip_ops.views_overlap_lds_parts()
    say(f"parts of one object from posed views: {V} views of {W} x {H}, {100 * float((depth > 0).double().mean()):.0f} % valid depth, "
        f"{n} parts a view (GT = {GT}), cell {cell}, {M} member pixels, {int(vol.sum())} distinct (voxel, part), {F} fused parts, "
        f"{int(m['n_links'][0])} unions, {int(dropped.sum())} pixels dropped")
    say(f"median [min .. max] of {args.reps} in ms (device events), warmed up, the legs taking turns; device: {torch.cuda.get_device_name(0)}")

    def overlap_with(parts):
        hip_ops.views_overlap_lds_parts(parts)
        try:
            return hip_ops.views_overlap(wrows, part_of, lo, cell, GT)
        finally:
            hip_ops.views_overlap_lds_parts(lds_default)

    # ---- the baseline: torch ops and the host ----
    def torch_keys():
        xyz = rows.reshape(V, H * W, 6)[:, :, :3].double()
        nn = torch.tensor(n, device=dev)[:, None]
        base = torch.tensor(np.concatenate([[0], np.cumsum(n)])[:-1], device=dev)[:, None]
        q = inst.reshape(V, -1).long()
        member = (valid.reshape(V, -1) != 0) & (q >= 0) & (q < nn)
        g = torch.where(member, base + q, -1)
        x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
        w = torch.stack([((x * Rd[:, k, 0, None] + y * Rd[:, k, 1, None]) + z * Rd[:, k, 2, None]) + td[:, k, None] for k in range(3)], -1).float()
        low = torch.where(member[..., None], w, float("inf")).reshape(-1, 3).amin(0).double()
        idx = torch.floor((w.double() - low) / cell)
        ok = member & ((idx >= 0) & (idx < 1024)).all(-1)
        i = torch.where(ok[..., None], idx, 0).long()
        return torch.where(ok, ((i[..., 0] << 20 | i[..., 1] << 10 | i[..., 2]) << 9) | g, -1), g

    def torch_tables():
        keys, g = torch_keys()
        u = torch.unique(keys)
        u = u[u >= 0]
        vox = torch.unique(u >> 9, return_inverse=True)[1]
        occ = torch.zeros((int(vox.max()) + 1, GT), dtype=torch.float32, device=dev)  # (a host read: the table's height)
        occ[vox, u & 511] = 1
        tab = (occ.T @ occ).round().int()
        return tab.diagonal().clone(), tab - torch.diag(tab.diagonal()), g

    def baseline_all():
        v_, i_, g = torch_tables()
        host = MV._merge_numpy(i_.cpu().numpy(), v_.cpu().numpy(), cls_all.cpu().numpy(), n, min_inter, min_overlap)
        fo_ = torch.from_numpy(np.concatenate([host["fused_of"], [-1]])).to(dev)
        return host, fo_[torch.where(g >= 0, g, GT)]

    bv, bi, _ = torch_tables()
    assert torch.equal(bv, vol) and torch.equal(bi, inter), "both paths count the same tables"
    for parts in (0, lds_default):
        v2, i2, _ = overlap_with(parts)
        assert torch.equal(v2, vol) and torch.equal(i2, inter), "both forms of the pair table agree"
    host, b_inst = baseline_all()
    assert np.array_equal(host["fused_of"], fo) and torch.equal(b_inst.reshape(V, H, W).int(), fused_inst), "both paths fuse the same parts"

    fuse = lambda with_npcs: MV.fuse_parts(depth, d["K"], inst, classes, d["R"], d["t"], npcs=npcs if with_npcs else None, cell=cell,  # noqa: E731
                                           min_inter=min_inter, min_overlap=min_overlap)
    legs = {
        "new: back-projection (gpn_frame_backproject)": lambda: hip_ops.frame_backproject(depth, rgb, Kd),
        "new: gpn_views_world": lambda: hip_ops.views_world(rows, valid, inst, n, Rd, td, GT),
        f"new: gpn_views_overlap, pair table in LDS (GT <= {lds_default})": lambda: overlap_with(lds_default),
        "new: gpn_views_overlap, pair table in global memory": lambda: overlap_with(0),
        "new: gpn_views_merge": lambda: hip_ops.views_merge(inter, vol, cls_all, n, min_inter, min_overlap),
        "new: gpn_views_relabel": lambda: hip_ops.views_relabel(part_of, m["fused_of"]),
        "new: gpn_views_gather (xyz, npcs, src)": lambda: hip_ops.views_gather(wrows, npcs, fused_inst, seg, M),
        "new: fuse_parts without npcs (association only)": lambda: fuse(False),
        "new: fuse_parts with npcs (association + gather + box fit)": lambda: fuse(True),
        "baseline: keys by torch ops": torch_keys,
        "baseline: keys + torch.unique + occupancy product": torch_tables,
        "baseline: ... + host read + greedy loop on the host + relabel": baseline_all,
    }
    times = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    for _ in range(args.reps):
        for k, fn in legs.items():
            times[k].append(event_ms(fn)[0])
    for k, ts in times.items():
        say(f"  {k:66s}{fmt(ts)}")
    med = lambda k: statistics.median(times[k])  # noqa: E731
    px = float(V * H * W)
    keys = list(legs)
    # least bytes, counted from the source.  world: 12 (xyz of the row) + 4 (inst) + 1 (valid) in, 12 + 4 out a pixel.  overlap: the
    # key pass reads 16 and writes 8 a pixel; a 40-bit radix sort in 8-bit digits is five passes of 8 in + 8 out plus one histogram
    # read of 8 (rocPRIM's own choice of digit width is not ours to count: REASONED, not measured); unique reads 8 a pixel.
    # gather: two passes over the 4-byte map, 24 in and 56 out a kept row.
    say(f"  world:   {px * 33 / (med(keys[1]) * 1e-3) / 1e12:6.2f} TB/s of its least bytes (33 a pixel) against {HBM_PEAK / 1e12:.1f} TB/s")
    say(f"  overlap: {px * 120 / (med(keys[2]) * 1e-3) / 1e12:6.2f} TB/s of its least bytes (120 a pixel: keys 24, sort 88 - reasoned from a 40-bit "
        f"sort in 8-bit digits -, unique 8)")
    say(f"  gather:  {(px * 8 + M * 80.0) / (med(keys[6]) * 1e-3) / 1e12:6.2f} TB/s of its least bytes (two passes of 4 a pixel, 24 in and 56 out a kept row)")
    say(f"  pair table, LDS against global: {med(keys[3]) / med(keys[2]):.3f} x (global / LDS time of the whole entry point)")
    say(f"  association, new against baseline: {med(keys[11]) / med(keys[7]):.1f} x (fuse_parts without npcs includes the back-projection; "
        f"the baseline starts from the rows)")
    say("  measured: every time above.  reasoned: the byte counts (from the source; the sort's pass count is rocPRIM's).")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
