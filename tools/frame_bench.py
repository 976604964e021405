"""Part inference on RGB-D frames, stage by stage (gapartnet_amd/inference.py; csrc/frameprep.hip) -> profiles/frame_bench.txt.

    python tools/frame_bench.py [--out profiles/frame_bench.txt] [--reps 7] [--frames 8] [--height 720] [--width 1280]

Workload: --frames frames of --width x --height with about 60 % valid depth (the synthetic scenes' points splatted in front of a
wall, the rest holes), num_points = 20000, presample 4 (cap = 80000 rows a frame).  Device-event times, medians of --reps runs, the
two legs taking turns inside every repetition:
  new       gpn_frame_backproject, gpn_frame_select (select + compaction; the compaction alone is the cap = 0 call), gpn_view_fps over
            at most cap rows a frame, gpn_cloud_finish
  baseline  what the parent commit offers: numpy back-projection on the host to an [H*W, 6] cloud with NaNs (wall clock, reported on
            its own line), the upload, then prepare_clouds - FPS over every valid row
then nearest, the network and the overlay on the new leg's result, the three new kernel stages' own kernel times (torch.profiler) with their least bytes against the HBM peak,
and FPS at cap rows against FPS at all valid rows.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s (MI355X)


def make_frames(V, H, W, seed=0, valid=0.6):
    """depth f32 [V,H,W] (metres, 0 = hole), rgb u8, K [V,3,3]: a synthetic scene's points splatted over a wall; holes at random"""
    from gapartnet_amd.dataset import synthetic
    depth = np.zeros((V, H, W), np.float32)
    rgb = np.zeros((V, H, W, 3), np.uint8)
    K = np.zeros((V, 3, 3))
    for v in range(V):
        rng = np.random.RandomState(seed + v)
        xyz, col = (np.asarray(a, np.float64) for a in synthetic.make_scene_arrays(seed + v, 20000)[:2])
        xyz = xyz * 0.4 + [0.0, 0.0, 1.5]
        f = 0.9 * W
        K[v] = [[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]]
        d = np.full((H, W), 2.5, np.float32) + rng.rand(H, W).astype(np.float32) * 0.01
        c = np.full((H, W, 3), 128, np.uint8)
        u = np.rint(xyz[:, 0] * f / xyz[:, 2] + K[v, 0, 2]).astype(np.int64)
        w = np.rint(xyz[:, 1] * f / xyz[:, 2] + K[v, 1, 2]).astype(np.int64)
        r = max(int(f * 0.004), 1)   # a point covers a (2 r + 1)^2 patch
        for j in np.argsort(-xyz[:, 2]):
            y0, y1, x0, x1 = max(w[j] - r, 0), min(w[j] + r + 1, H), max(u[j] - r, 0), min(u[j] + r + 1, W)
            if y0 < y1 and x0 < x1:
                d[y0:y1, x0:x1] = xyz[j, 2]
                c[y0:y1, x0:x1] = np.clip(col[j] * 255, 0, 255)
        d[rng.rand(H, W) >= valid] = 0
        depth[v], rgb[v] = d, c
    return depth, rgb, K


def numpy_backproject(depth, rgb, K):
    """the parent commit's user: [V, H*W, 6] f32 clouds with NaN xyz on the holes"""
    V, H, W = depth.shape
    z = depth.astype(np.float64)
    u, v = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
    x = (u - K[:, 0, 2, None, None]) * z / K[:, 0, 0, None, None]
    y = (v - K[:, 1, 2, None, None]) * z / K[:, 1, 1, None, None]
    xyz = np.stack([x, y, z], -1).astype(np.float32)
    xyz[depth == 0] = np.nan
    return np.concatenate([xyz, (rgb / 255.0).astype(np.float32)], -1).reshape(V, H * W, 6)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--num_points", type=int, default=20000)
    ap.add_argument("--presample", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_bench needs a GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    from gapartnet_amd import hip_ops, inference
    from gapartnet_amd.smoke import make_model
    from gapartnet_amd.structure.point_cloud import PointCloud
    V, H, W, m = args.frames, args.height, args.width, args.num_points
    cap, HW = args.presample * m, args.height * args.width
    depth, rgb, K = make_frames(V, H, W)
    n_valid = (depth > 0).reshape(V, -1).sum(1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    fh = open(args.out, "w")

    def say(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    say(f"part inference on RGB-D frames: {V} frames of {W} x {H}, {100 * n_valid.sum() / (V * HW):.1f} % valid depth "
        f"({n_valid.min()} .. {n_valid.max()} pixels a frame), num_points = {m}, cap = {cap}")
    say(f"median [min .. max] of {args.reps} in ms (device events unless said), warmed up, the two legs taking turns")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say()
    d_dev, c_dev, k_dev = torch.from_numpy(depth).to(dev), torch.from_numpy(rgb).to(dev), torch.from_numpy(K).to(dev)
    seeds = list(range(V))
    off = [v * HW for v in range(V + 1)]

    off_dev = torch.tensor(off, dtype=torch.int64, device=dev)

    def new_stages():
        """the four stages of hip_ops.frame_prepare, one after the other with an event pair around each"""
        t = {}
        t["backproject"], (rows, valid, vc) = event_ms(lambda: hip_ops.frame_backproject(d_dev, c_dev, k_dev))
        t["select+compact"], (packed, pix, counts, status) = event_ms(lambda: hip_ops.frame_select(rows, valid, vc, seeds, cap))
        t["fps"], idx = event_ms(lambda: hip_ops.view_fps(packed, counts, status, m))
        t["finish"], _ = event_ms(lambda: hip_ops.cloud_finish(rows, 6, off_dev, pix, HW, counts, idx, status, m))
        return t

    def new_leg():
        return hip_ops.frame_prepare(d_dev, c_dev, k_dev, m, cap, seeds)

    def base_leg():
        t0 = time.perf_counter()
        clouds = numpy_backproject(depth, rgb, K)
        t1 = time.perf_counter()
        ms_up, dev_clouds = event_ms(lambda: torch.from_numpy(clouds).to(dev))
        ms_prep, prep = event_ms(lambda: inference.prepare_clouds(list(dev_clouds), m))
        return (t1 - t0) * 1e3, ms_up, ms_prep, prep

    new_leg(), new_stages(), base_leg()   # warm-up
    stages = {k: [] for k in ("backproject", "select+compact", "fps", "finish", "frame_prepare (whole call, one host read)")}
    base = {k: [] for k in ("numpy back-projection (host, wall clock)", "upload", "prepare_clouds (pack, FPS over all valid rows, finish)")}
    for _ in range(args.reps):
        for name, ms in new_stages().items():
            stages[name].append(ms)
        stages["frame_prepare (whole call, one host read)"].append(event_ms(new_leg)[0])
        h, up, pr, _ = base_leg()
        for k, x in zip(base, (h, up, pr)):
            base[k].append(x)
    say("== new front: frames -> the network's input ==")
    for k, ts in stages.items():
        say(f"  {k:<58} {fmt(ts)}")
    say("== baseline (the parent commit): numpy back-projection + prepare_clouds ==")
    for k, ts in base.items():
        say(f"  {k:<58} {fmt(ts)}")
    new_med = statistics.median(stages["frame_prepare (whole call, one host read)"])
    base_dev = statistics.median(base["upload"]) + statistics.median(base["prepare_clouds (pack, FPS over all valid rows, finish)"])
    base_all = base_dev + statistics.median(base["numpy back-projection (host, wall clock)"])
    say(f"  baseline / new: {base_dev / new_med:.2f} x on the device (upload + prepare_clouds), {base_all / new_med:.2f} x with the host's "
        f"back-projection")
    say()

    # the compaction alone (cap = 0: count, scan, ordered stores; no select passes) and the select passes by difference
    rows, valid, vc = hip_ops.frame_backproject(d_dev, c_dev, k_dev)
    hip_ops.frame_select(rows, valid, vc, seeds, 0), hip_ops.frame_select(rows, valid, vc, seeds, cap)
    both, alone = [], []
    for _ in range(args.reps):
        both.append(event_ms(lambda: hip_ops.frame_select(rows, valid, vc, seeds, cap))[0])
        alone.append(event_ms(lambda: hip_ops.frame_select(rows, valid, vc, seeds, 0))[0])
    say("== select and compaction ==")
    say(f"  {'gpn_frame_select, cap = ' + str(cap) + ' (4 histogram passes + compaction)':<58} {fmt(both)}")
    say(f"  {'gpn_frame_select, cap = 0 (compaction of all valid rows)':<58} {fmt(alone)}")
    say()

    # the three new kernel stages by themselves: kernel times from the profiler (no launch gaps), least bytes (every needed
    # byte once) against the HBM peak.  select = the 4 histogram passes + the count pass; compaction = the scan + the stores
    M = V * HW
    kept = int(np.minimum(n_valid, cap).sum())
    groups = {"back-projection": (("fr_backproject_kernel",), M * (4 + 3) + M * (24 + 1)),   # depth + rgb read; rows + validity written
              "select": (("fr_hist_kernel", "fr_count_kernel"), M * 5),                     # the validity bytes, once a pass
              "compaction": (("fr_scan_kernel", "fr_compact_kernel"), M + kept * 12 + kept * 20)}  # validity + kept xyz read; packed + index written
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(args.reps):
            r2, v2, c2 = hip_ops.frame_backproject(d_dev, c_dev, k_dev)
            hip_ops.frame_select(r2, v2, c2, seeds, cap)
        torch.cuda.synchronize()
    us = {k: 0.0 for k in groups}
    for e in prof.key_averages():
        total = getattr(e, "device_time_total", None)
        total = e.cuda_time_total if total is None else total
        for k, (names, _) in groups.items():
            if any(n in e.key for n in names):
                us[k] += total / args.reps
    say(f"== the new kernels alone (torch.profiler kernel times, mean of {args.reps} calls), least bytes, share of the "
        f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak ==")
    for k, (_, nbytes) in groups.items():
        if us[k] <= 0:
            raise SystemExit(f"the profiler returned no kernel of the {k} stage")
        say(f"  {k:<18} {us[k]:10.1f} us  {nbytes / 1e6:9.2f} MB  {nbytes / (us[k] * 1e-6) / 1e9:8.1f} GB/s  "
            f"{100 * nbytes / (us[k] * 1e-6) / HBM_PEAK:6.2f} % of peak")
    say()
    del r2, v2, c2

    # FPS at cap rows against FPS at all valid rows (gpn_view_fps on the two packed layouts)
    p_cap, _, c_cap, s_cap = hip_ops.frame_select(rows, valid, vc, seeds, cap)
    p_all, _, c_all, s_all = hip_ops.frame_select(rows, valid, vc, seeds, 0)
    hip_ops.view_fps(p_cap, c_cap, s_cap.clone(), m), hip_ops.view_fps(p_all, c_all, s_all.clone(), m)
    f_cap, f_all, f_one = [], [], []
    for _ in range(args.reps):
        f_cap.append(event_ms(lambda: hip_ops.view_fps(p_cap, c_cap, s_cap.clone(), m))[0])
        f_all.append(event_ms(lambda: hip_ops.view_fps(p_all, c_all, s_all.clone(), m))[0])
        f_one.append(event_ms(lambda: hip_ops.view_fps(p_cap, c_cap, s_cap.clone(), m, max_groups=1))[0])
    say("== gpn_view_fps ==")
    say(f"  {'over cap = ' + str(cap) + ' rows a frame':<58} {fmt(f_cap)}")
    say(f"  {'over all valid rows (' + str(int(n_valid.mean())) + ' a frame)':<58} {fmt(f_all)}")
    say(f"  {'over cap rows, max_groups = 1 (one workgroup a frame, no waits)':<58} {fmt(f_one)}")
    say(f"  all / cap: {statistics.median(f_all) / statistics.median(f_cap):.2f} x; per sample at cap rows: "
        f"{statistics.median(f_cap) * 1e3 / m:.1f} us")
    say()
    del p_cap, p_all, rows, valid

    # behind the preparation: nearest, network, overlay
    prep = inference.prepare_frames(d_dev, c_dev, K, m, args.presample, seeds)
    t = prep.table
    counts = prep.counts.tolist()
    net_off = np.concatenate([[0], np.cumsum(counts)]).tolist()
    model = make_model((0, 0)).to(dev).eval()
    pcs = [PointCloud(pc_id=str(s), points=prep.points[net_off[s]:net_off[s + 1]].contiguous(), obj_cat=0) for s in range(V)]
    boxes = [torch.tensor(np.random.RandomState(v).rand(6, 8, 3) * [0.8, 0.6, 0.5] + [-0.4, -0.3, 1.2], device=dev) for v in range(V)]
    legs = {"nearest (every pixel -> its sample)": lambda: hip_ops.cloud_nearest(prep.source, off, t["sample_rows"], t["counts"], t["status"]),
            "network": lambda: model(pcs),
            "overlay (6 boxes a frame)": lambda: inference.draw_overlays(c_dev, boxes, torch.from_numpy(K))}
    say("== behind the preparation ==")
    with torch.no_grad():
        for k, fn in legs.items():
            fn()
            say(f"  {k:<58} {fmt([event_ms(fn)[0] for _ in range(args.reps)])}")
    fh.close()


if __name__ == "__main__":
    main()
