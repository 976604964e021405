"""Label-free inference, stage by stage (gapartnet_amd/inference.py; csrc/cloudprep.hip) -> profiles/inference_bench.txt.

    python tools/inference_bench.py [--out profiles/inference_bench.txt] [--reps 5] [--sizes 20000 200000 1000000] [--batches 1 8]
    python tools/inference_bench.py --kernels-only      (the new kernels alone, twice per shape: the run to put under
                                                         rocprofv3 --kernel-trace --stats --output-format csv)
    python tools/inference_bench.py --trace DIR         (append to --out each new kernel's time in that run's *kernel_trace.csv
                                                         - the second of its two dispatches per shape - and its share of the HBM peak)

Per (points per cloud, S): device-event times of prepare / network / post-processing + boxes / nearest, each shape warmed up, the
median of --reps.  The parent commit has no inference path, so each new kernel is compared with the best the parent offers, in the
same process with the legs alternating:
  cloud_nearest  against gpn_pn2_knn with k = 1, cloud by cloud
  cloud_prepare  against a loop over the clouds of gpn_pn2_furthest_point_sampling_ws plus the torch glue around it (valid-row
                 compaction, gather, float64 ball normalisation)
and the least bytes each new kernel has to move are printed next to its time (share of the HBM peak: kernel times from the
profiler run).  Clouds: the synthetic scenes' surfaces scaled into a camera frame, 0.5 % of the rows NaN.
"""
import argparse
import csv
import glob
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s (MI355X)


def make_clouds(S, n, device, seed=0):
    from gapartnet_amd.dataset import synthetic
    out = []
    for s in range(S):
        rng = np.random.RandomState(seed + s)
        # a 20 000-point synthetic scene, repeated with 2 mm of noise up to n points: the same surfaces, more densely scanned
        xyz, rgb = (np.asarray(a, np.float32) for a in synthetic.make_scene_arrays(seed + s, min(n, 20000))[:2])
        rep = (n + xyz.shape[0] - 1) // xyz.shape[0]
        xyz = (np.tile(xyz, (rep, 1))[:n] + rng.normal(scale=2e-3, size=(n, 3))).astype(np.float32)
        rgb = np.tile(rgb, (rep, 1))[:n]
        cloud = np.concatenate([xyz * 0.4 + [0.1, -0.2, 1.5], rgb], 1).astype(np.float32)
        cloud[rng.choice(n, max(n // 200, 1), replace=False), rng.randint(0, 3)] = np.nan
        out.append(torch.from_numpy(cloud).to(device))
    return out


def timed(fn, reps):
    """median device-event milliseconds of fn() over reps runs (the caller warmed the shape up)"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def alternating(legs, reps):
    """{name: (median, min, max)} with the legs taking turns inside every repetition"""
    ts = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def prepare_baseline(clouds, m):
    """the parent's way: cloud by cloud, gpn_pn2_furthest_point_sampling_ws + torch glue -> (points, rows, scale) per cloud"""
    from gapartnet_amd import hip_ops
    out = []
    for c in clouds:
        rows = torch.nonzero(torch.isfinite(c[:, :3]).all(1)).squeeze(1)
        if rows.shape[0] > m:
            idx = hip_ops.pn2_furthest_point_sampling(c[rows, :3][None].contiguous(), m)[0].long()
            rows = rows[idx]
        p = c[rows, :3].double()
        ctr = (p.amax(0) + p.amin(0)) / 2
        d = p - ctr
        r = torch.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).amax())
        pts = c[rows].clone()
        pts[:, :3] = (d / r).float()
        out.append((pts, rows, torch.cat([r[None], ctr])))
    return out


def nearest_baseline(clouds, sample_rows):
    from gapartnet_amd import hip_ops
    return [hip_ops.pn2_knn(c[None, :, :3].contiguous(), c[r, :3][None].contiguous(), 1)[1] for c, r in zip(clouds, sample_rows)]


KERNELS = ("cp_pack_kernel", "cp_finish_kernel", "cn_build_kernel", "cn_query_kernel")


def least_bytes(S, n, C, ms):
    """the least bytes each new kernel has to move (every needed byte once) for S clouds of n rows, C columns, ms samples in all"""
    M = S * n
    return {"cp_pack_kernel": M * 12 + M * 20,                        # xyz read; packed float4 + row index written
            "cp_finish_kernel": ms * (8 + C * 4) + ms * (C * 4 + 4),  # FPS index + row index + the sampled row read; out + rows written
            "cn_build_kernel": ms * (4 + 12) + ms * 16,               # sample rows + their xyz read; sorted float4 written
            "cn_query_kernel": M * 12 + M * 4 + ms * 16}              # queries read, nn written, every sorted sample once


def trace_summary(trace_dir, shapes, m, C, out):
    """per shape and new kernel: microseconds of its second dispatch in the profiler's kernel trace, least bytes, share of the peak"""
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {trace_dir}")
    runs = {k: [] for k in KERNELS}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                for k in KERNELS:
                    if row["Kernel_Name"].startswith(k) or ("::" + k) in row["Kernel_Name"] or (" " + k) in row["Kernel_Name"]:
                        runs[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    lines = ["", f"kernel times of the new kernels (rocprofv3 --kernel-trace, a run of its own; the second of two dispatches per shape), "
                 f"least bytes, share of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak"]
    for k in KERNELS:
        runs[k].sort()
        if len(runs[k]) != 2 * len(shapes):
            raise SystemExit(f"{k}: {len(runs[k])} dispatches in the trace, {2 * len(shapes)} expected")
    for i, (n, S) in enumerate(shapes):
        ms = S * min(n - max(n // 200, 1), m)
        need = least_bytes(S, n, C, ms)
        lines.append(f"== {n} points x S = {S} ==")
        for k in KERNELS:
            a, b = runs[k][2 * i + 1]
            us = (b - a) / 1e3
            lines.append(f"  {k:<18} {us:10.1f} us  {need[k] / 1e6:9.2f} MB  {need[k] / (us * 1e-6) / 1e9:8.1f} GB/s  "
                         f"{100 * need[k] / (us * 1e-6) / HBM_PEAK:6.2f} % of peak")
    with open(out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inference_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 200000, 1000000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--num_points", type=int, default=20000)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--trace", default=None, help="directory of a profiler run of --kernels-only with the same --sizes / --batches")
    args = ap.parse_args()
    if args.trace:
        return trace_summary(args.trace, [(n, S) for n in args.sizes for S in args.batches], args.num_points, 6, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("inference_bench needs a GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    from gapartnet_amd import hip_ops, inference
    from gapartnet_amd.smoke import make_model
    from gapartnet_amd.structure.point_cloud import PointCloud
    m = args.num_points
    model = make_model((0, 0)).to(dev).eval()
    predictor = inference.PartPredictor(model, num_points=m)
    lines = [f"label-free inference, num_points = {m}, median [min .. max] of {args.reps} in ms (device events), every shape warmed up",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    if not args.kernels_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def say(s=""):
        print(s, flush=True)
        with open(args.out, "a") as fh:  # (line by line: a run that is cut short keeps what it measured)
            fh.write(s + "\n")

    for n in args.sizes:
        for S in args.batches:
            clouds = make_clouds(S, n, dev)
            src = torch.cat(clouds)
            off = [i * n for i in range(S + 1)]
            if args.kernels_only:
                for _ in range(2):
                    got = hip_ops.cloud_prepare(src, off, m)
                    hip_ops.cloud_nearest(src, off, got["sample_rows"], got["counts_dev"], got["status_dev"])
                torch.cuda.synchronize()
                print(f"{n} x {S}: done", flush=True)
                del clouds, src, got
                continue
            prep = inference.prepare_clouds(clouds, m)   # (warm-up of the shape, and the tables the later stages read)
            t = prep.table
            counts = prep.counts.tolist()
            net_off = np.concatenate([[0], np.cumsum(counts)]).tolist()
            pcs = [PointCloud(pc_id=str(s), points=prep.points[net_off[s]:net_off[s + 1]].contiguous(), obj_cat=0) for s in range(S)]
            state = {}

            def network():
                state["fwd"] = model(pcs)

            def post():
                props = state["fwd"][2]
                if props is not None:
                    kept = model._post_process_kept_points(props)
                    state["pred"] = inference._scene_predictions(kept, net_off, None, predictor.max_iters)

            np.random.seed(0)
            network(), post()   # warm-up
            stage = {"prepare": timed(lambda: inference.prepare_clouds(clouds, m), args.reps), "network": timed(network, args.reps),
                     "post+boxes": timed(post, args.reps),
                     "nearest": timed(lambda: hip_ops.cloud_nearest(src, off, t["sample_rows"], t["counts"], t["status"]), args.reps)}
            say(f"== {n} points x S = {S} ==")
            for k, (med, lo, hi) in stage.items():
                say(f"  {k:<12} {med:9.3f} [{lo:9.3f} .. {hi:9.3f}]")
            say(f"  total        {sum(v[0] for v in stage.values()):9.3f}")
            # the new kernels against the parent's best, legs alternating
            rows = [prep.sample_rows[net_off[s]:net_off[s + 1]] for s in range(S)]
            prepare_baseline(clouds, m), nearest_baseline(clouds, rows)   # warm-up
            ab = alternating({"cloud_prepare": lambda: hip_ops.cloud_prepare(src, off, m),
                              "fps loop + torch": lambda: prepare_baseline(clouds, m)}, args.reps)
            ab.update(alternating({"cloud_nearest": lambda: hip_ops.cloud_nearest(src, off, t["sample_rows"], t["counts"], t["status"]),
                                   "pn2_knn k=1": lambda: nearest_baseline(clouds, rows)}, args.reps))
            for k, (med, lo, hi) in ab.items():
                say(f"  A/B {k:<18} {med:9.3f} [{lo:9.3f} .. {hi:9.3f}]")
            say()
            del clouds, src, prep, pcs, state
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
