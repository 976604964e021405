"""The two samplers of the inference path side by side (include/gpn.h sections VP / GS) -> profiles/sampler_bench.txt.

    python tools/sampler_bench.py [--out profiles/sampler_bench.txt] [--reps 7] [--frames 8] [--height 720] [--width 1280]

Workload: tools/frame_bench.py's - --frames frames of --width x --height with about 60 % valid depth, num_points = 20000 - at
presample 4 (cap = 80000 rows a frame) and at presample 0 (every valid pixel).  Device-event times, medians of --reps runs, the two
samplers taking turns inside every repetition:
  the stage alone   gpn_cloud_grid_sample against gpn_view_fps (the parent's path, the baseline) on the same packed rows
  frame_prepare     the whole preparation with each sampler (one host read)
  predict_frames    a whole call with each sampler, synthetic weights
and per frame, for both samplers: the coverage radius (the largest distance from a valid pixel's point to its nearest sample),
the mean of that distance, the grid's level L* and cell count C_L*, and the share of valid pixels whose semantic label agrees
between the two samplers.  The weights are synthetic (gapartnet_amd.smoke.make_model): that share says how far two sample sets
move an untrained network's labels, nothing about a trained checkpoint.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from frame_bench import HBM_PEAK, event_ms, fmt, make_frames  # noqa: E402


def cells_at(xyz, level):
    """the occupied level-`level` cells of a cloud [n, 3] f32 by section GS's quantisation (level >= 0)"""
    lo, hi = xyz.min(0), xyz.max(0)
    e = np.float32((hi - lo).max())
    if not (e > 0 and np.isfinite(e)):
        return 1
    x = (xyz - lo) * np.float32(1024.0 / np.float64(e))
    q = np.where(x < np.float32(1023.0), x, np.float32(1023.0)).astype(np.int64) >> (10 - level)
    return int(np.unique((q[:, 0] << 20) | (q[:, 1] << 10) | q[:, 2]).shape[0])


def grid_stage_bytes(rows_total, live, m_total, key_bits):
    """the least bytes the grid stage moves, from the source (csrc/gridsample.hip), every needed byte once per pass: bounds read the
    live xyzw; keys read them again and write a u64 key + u32 row for every slot; the sort's histogram reads the keys and each of
    its ceil(key_bits / 8) scatter passes reads and writes a (key, row) pair; levels and mark read the sorted keys (mark the rows
    too) and write two bytes; the four select passes, the tie count and the pick read the candidate byte (and a key per
    candidate, not counted); count and emit read the flag byte; emit writes the indices"""
    passes = -(-key_bits // 8)
    return (live * 16 * 2 + rows_total * 12 + rows_total * 8 + passes * rows_total * 24 + live * (8 + 12 + 2) + live * 6 * 1 + live * 2 * 1
            + m_total * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--num_points", type=int, default=20000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench needs a GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    from gapartnet_amd import hip_ops, inference
    from gapartnet_amd.smoke import make_model
    V, H, W, m = args.frames, args.height, args.width, args.num_points
    HW = H * W
    depth, rgb, K = make_frames(V, H, W)
    n_valid = (depth > 0).reshape(V, -1).sum(1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    fh = open(args.out, "w")

    def say(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    say(f"samplers of the inference path: {V} frames of {W} x {H}, {100 * n_valid.sum() / (V * HW):.1f} % valid depth "
        f"({n_valid.min()} .. {n_valid.max()} pixels a frame), num_points = {m}")
    say(f"median [min .. max] of {args.reps} in ms (device events), warmed up, the two samplers taking turns")
    say(f"device: {torch.cuda.get_device_name(0)}")
    d_dev, c_dev, k_dev = torch.from_numpy(depth).to(dev), torch.from_numpy(rgb).to(dev), torch.from_numpy(K).to(dev)
    seeds = list(range(V))
    off = [v * HW for v in range(V + 1)]
    model = make_model((0, 0)).to(dev).eval()
    Kt = torch.from_numpy(K)
    for pre in (4, 0):
        cap = pre * m
        say()
        say(f"======== presample {pre}: " + (f"cap = {cap} rows a frame" if cap else "no cut, every valid pixel") + " ========")
        rows, valid, vc = hip_ops.frame_backproject(d_dev, c_dev, k_dev)
        packed, pix, counts, status = hip_ops.frame_select(rows, valid, vc, seeds, cap)
        live = int(np.minimum(n_valid, cap).sum()) if cap else int(n_valid.sum())
        nb = int(packed.shape[1])
        stage = {"fps": lambda: hip_ops.view_fps(packed, counts, status.clone(), m),
                 "grid": lambda: hip_ops.cloud_grid_sample(packed, counts, status.clone(), seeds, m)}
        whole = {s: (lambda s=s: hip_ops.frame_prepare(d_dev, c_dev, k_dev, m, cap, seeds, sampler=s)) for s in ("fps", "grid")}
        pred = {s: inference.PartPredictor(model, num_points=m, sampler=s) for s in ("fps", "grid")}
        call = {s: (lambda s=s: pred[s].predict_frames(d_dev, c_dev, Kt, presample=pre, seed=seeds)) for s in ("fps", "grid")}
        times = {}
        for name, legs in (("the stage alone", stage), ("frame_prepare (whole call, one host read)", whole), ("predict_frames (whole call)", call)):
            for fn in legs.values():
                fn()   # warm-up
            ts = {s: [] for s in legs}
            for _ in range(args.reps):
                for s, fn in legs.items():
                    ts[s].append(event_ms(fn)[0])
            times[name] = ts
            say(f"== {name} ==")
            label = {"fps": "gpn_view_fps (baseline)", "grid": "gpn_cloud_grid_sample"}
            for s in legs:
                say(f"  {label[s]:<34} {fmt(ts[s])}")
            say(f"  fps / grid: {statistics.median(ts['fps']) / statistics.median(ts['grid']):.1f} x")
        t_grid = statistics.median(times["the stage alone"]["grid"]) * 1e-3
        key_bits = 31 + max((V - 1).bit_length(), 1)
        nbytes = grid_stage_bytes(V * nb, live, V * m, key_bits)
        say(f"== the grid stage's least bytes (from the source, not from counters): {nbytes / 1e6:.1f} MB over {V * nb} slots, "
            f"{live} live rows -> {nbytes / t_grid / 1e9:.1f} GB/s, {100 * nbytes / t_grid / HBM_PEAK:.2f} % of the "
            f"{HBM_PEAK / 1e12:.0f} TB/s HBM peak ==")
        say(f"  at the peak these bytes take {nbytes / HBM_PEAK * 1e6:.1f} us of the {t_grid * 1e6:.0f} us measured; the stage is a chain of "
            f"12 launches plus the sort's, each waiting for the one before, and the sort's scatter passes write 12-byte pairs to 256 "
            f"places at once: launch and dependency latency bound the small case, the sort the large one (reasoning from the "
            f"source; no counter run was made)")
        # quality: distance of every valid pixel's point to its nearest sample, per frame
        say("== quality per frame: coverage radius / mean distance to the nearest sample (metres), grid level and cells ==")
        got = {s: whole[s]() for s in ("fps", "grid")}
        d = {}
        for s in ("fps", "grid"):
            _, d2 = hip_ops.cloud_nearest(rows, off, got[s]["sample_rows"], got[s]["counts_dev"], got[s]["status_dev"], want_d2=True)
            d[s] = torch.sqrt(d2.reshape(V, HW).double())
        ok = torch.from_numpy(depth > 0).reshape(V, HW).to(dev)
        packed_host = packed.cpu().numpy()
        counts_host = counts.cpu().numpy()
        sem = {s: torch.stack([p.sem.reshape(-1) for p in call[s]()]) for s in ("fps", "grid")}
        ratios = []
        for v in range(V):
            cov = {s: float(d[s][v][ok[v]].max()) for s in d}
            mean = {s: float(d[s][v][ok[v]].mean()) for s in d}
            L = int(got["grid"]["level"][v])
            cells = cells_at(packed_host[v, :counts_host[v], :3], L) if L >= 0 else 0
            agree = float((sem["fps"][v][ok[v]] == sem["grid"][v][ok[v]]).double().mean())
            ratios.append((cov["grid"] / cov["fps"], mean["grid"] / mean["fps"]))
            say(f"  frame {v}: coverage fps {cov['fps']:.5f} grid {cov['grid']:.5f} ({ratios[-1][0]:.2f} x)   mean fps {mean['fps']:.5f} "
                f"grid {mean['grid']:.5f} ({ratios[-1][1]:.3f} x)   L* {L}  C_L* {cells}   sem agreement {100 * agree:.1f} % "
                f"(synthetic weights)")
        say(f"  grid / fps over the frames: coverage {min(r[0] for r in ratios):.2f} .. {max(r[0] for r in ratios):.2f} x, mean distance "
            f"{min(r[1] for r in ratios):.3f} .. {max(r[1] for r in ratios):.3f} x")
        del rows, valid, packed, pix, got, d
    fh.close()


if __name__ == "__main__":
    main()
