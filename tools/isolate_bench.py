"""Object isolation on raw RGB-D frames, stage by stage (gapartnet_amd/hip_ops.py frame_isolate; csrc/isolate.hip; include/gpn.h
section OB) -> profiles/isolate_bench.txt.

    python tools/isolate_bench.py [--out profiles/isolate_bench.txt] [--reps 7] [--frames 8] [--sizes 480x640 720x1280]

Workload: --frames synthetic frames a size (a sphere on a tilted table in front of a wall, 2.5 mm noise, 5 % holes, flying pixels:
tests/isolate_scenes.py), 256 hypotheses, 2 plane rounds.  Device-event times in ms, medians of --reps runs, warmed up:
  every stage of section OB by itself, and the whole of frame_isolate (all rounds, no host read)
  the score stage three ways, taking turns: the LDS-broadcast kernel (variant 0), the ballot kernel (variant 1), and plain torch
      (rows @ hyp.T in float64, compare, sum - frame by frame, its [H*W, n_hyp] product does not fit otherwise)
  the score kernel against its two ceilings: float64 operations a second and LDS broadcast reads a second
  the numpy / scipy formulation (inference.isolate_objects on CPU tensors) on ONE frame, wall clock - what the parent commit's user
      would run, there being no such path on the device
  predict_frames with and without isolate (random-init model, 20000 points), the legs taking turns
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

FP64_PEAK = 78.6e12 / 2  # float64 vector operations a second: the data sheet's 78.6 T counts an FMA as two, and the library is built
                         # with -ffp-contract=off (the contract's bits are numpy's), so every multiply and add issues on its own
CUS, LDS_CLK = 256, 2.4e9


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isolate_bench.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sizes", nargs="+", default=["480x640", "720x1280"])
    ap.add_argument("--no_predict", action="store_true")
    args = ap.parse_args()
    from gapartnet_amd import hip_ops, inference
    from tests import isolate_scenes as S
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"object isolation on raw RGB-D frames: {args.frames} frames a size, 256 hypotheses, 2 plane rounds, tol 5 mm")
    say(f"median [min .. max] of {args.reps} in ms (device events unless said), warmed up; device: {torch.cuda.get_device_name(0)}")
    V, NH, TOL = args.frames, 256, 0.005
    for size in args.sizes:
        H, W = (int(x) for x in size.split("x"))
        scenes = [S.make_scene(H, W, 100 + v, wall=True, radius=0.13) for v in range(V)]
        depth = torch.from_numpy(np.stack([s["depth"] for s in scenes])).to(dev)
        rgb = torch.from_numpy(np.stack([s["rgb"] for s in scenes])).to(dev)
        K = torch.from_numpy(np.stack([s["K"] for s in scenes]))
        seeds = list(range(V))
        rows, valid, vc = hip_ops.frame_backproject(depth, rgb, K.to(dev))
        _, pix, _, _ = hip_ops.frame_select(rows, valid, vc, seeds, 0)
        seeds_t = hip_ops._seed_tensor(seeds, V, dev)
        cand0 = hip_ops.frame_candidates(rows, valid)
        hyp, hyp_pix = hip_ops.frame_plane_hypotheses(rows, cand0, pix, vc, seeds_t, NH, 0)
        counts = hip_ops.frame_plane_score(rows, cand0, hyp, TOL)
        win = hip_ops.frame_plane_winner(counts)
        planes, inl, n_planes = hip_ops.frame_plane_refit(rows, cand0, hyp, hyp_pix, win, TOL, 0.1, 0, 1)
        cand1 = hip_ops.frame_plane_cut(rows, cand0.clone(), planes, TOL, 0)
        labels, sizes, n_comp = hip_ops.frame_components(rows, cand1)
        n_cand = int(cand0.sum())
        say()
        say(f"== {W} x {H}: {n_cand // V} candidates a frame, {int(cand1.sum()) // V} after the first cut, "
            f"{int(n_comp.sum()) // V} components of 6+ pixels a frame ==")

        def torch_score():
            out = []
            for v in range(V):
                xyz = rows[v * H * W:(v + 1) * H * W, :3].double()
                d = xyz @ hyp[v, :, :3].T + hyp[v, :, 3]
                out.append(((d.abs() <= TOL) & (cand0[v].reshape(-1, 1) != 0)).sum(0))
            return torch.stack(out)

        assert torch.equal(hip_ops.frame_plane_score(rows, cand0, hyp, TOL, 1), counts)
        agree = float((torch_score() == counts).double().mean())  # (the matmul's order of operations is its own: a few counts may differ)
        stages = {
            "candidates": lambda: hip_ops.frame_candidates(rows, valid),
            "select, cap = 0 (pix)": lambda: hip_ops.frame_select(rows, valid, vc, seeds, 0),
            "hypotheses": lambda: hip_ops.frame_plane_hypotheses(rows, cand0, pix, vc, seeds_t, NH, 0),
            "score (LDS broadcast, variant 0)": lambda: hip_ops.frame_plane_score(rows, cand0, hyp, TOL, 0),
            "score (ballot, variant 1)": lambda: hip_ops.frame_plane_score(rows, cand0, hyp, TOL, 1),
            "score (plain torch: rows @ hyp.T, compare, sum)": torch_score,
            "winner": lambda: hip_ops.frame_plane_winner(counts),
            "refit (sums, solve, count, accept)": lambda: hip_ops.frame_plane_refit(rows, cand0, hyp, hyp_pix, win, TOL, 0.1, 0, 1),
            "cut": lambda: hip_ops.frame_plane_cut(rows, cand1, planes, TOL, 0),
            "components (tiles, borders, flatten, count)": lambda: hip_ops.frame_components(rows, cand1),
            "select": lambda: hip_ops.frame_component_select(labels, sizes, n_planes, "largest", 6),
            "frame_isolate (everything, 2 rounds)": lambda: hip_ops.frame_isolate(rows, valid, vc, seeds, max_planes=2, n_hyp=NH, tol=TOL),
        }
        times = {k: [] for k in stages}
        for fn in stages.values():
            fn()
        for _ in range(args.reps):
            for k, fn in stages.items():
                times[k].append(event_ms(fn)[0])
        for k, ts in times.items():
            say(f"  {k:62s}{fmt(ts)}")
        say(f"  plain torch counts equal to the kernel's: {100 * agree:.2f} % of the hypotheses")
        evals = float(n_cand) * NH
        for k in ("score (LDS broadcast, variant 0)", "score (ballot, variant 1)"):
            t = statistics.median(times[k]) * 1e-3
            # per evaluation: 3 multiplies + 3 adds + |.| + compare in float64; variant 0 also reads 3 float64 from LDS (a broadcast
            # serves a wave of 64 hypotheses with one read of 8 bytes: 128 bytes a clock and CU)
            say(f"  {k}: {evals / t / 1e9:8.1f} G plane evaluations / s = {6 * evals / t / 1e12:6.2f} T float64 op / s "
                f"({100 * 6 * evals / t / FP64_PEAK:5.1f} % of {FP64_PEAK / 1e12:.1f} T)")
        t0 = statistics.median(times["score (LDS broadcast, variant 0)"]) * 1e-3
        lds_reads = 3 * evals / 64  # wave-wide broadcast reads of one float64
        say(f"  variant 0 LDS: {lds_reads / t0 / 1e9:8.1f} G broadcast reads / s of {CUS * LDS_CLK / 1e9:.0f} G issue slots "
            f"({100 * lds_reads / t0 / (CUS * LDS_CLK):5.1f} %)")
        t = time.perf_counter()
        inference.isolate_objects(torch.from_numpy(scenes[0]["depth"]), scenes[0]["K"], seed=0,
                                  config=inference.IsolateConfig(max_planes=2, n_hyp=NH, tol=TOL))
        cpu = (time.perf_counter() - t) * 1e3
        dev_ms = statistics.median(times["frame_isolate (everything, 2 rounds)"])
        say(f"  numpy / scipy formulation, ONE frame, host wall clock: {cpu:10.1f} ms  ({cpu * V / dev_ms:.0f} x the device's time a frame)")
        if args.no_predict:
            continue
        from gapartnet_amd.smoke import make_model
        predictor = inference.PartPredictor(make_model((0, 0)).to(dev).eval(), num_points=20000)
        cfg = inference.IsolateConfig(max_planes=2, n_hyp=NH, tol=TOL)
        legs = {"predict_frames": lambda: predictor.predict_frames(depth, rgb, K, seed=seeds),
                "predict_frames(isolate=...)": lambda: predictor.predict_frames(depth, rgb, K, seed=seeds, isolate=cfg)}
        pt = {k: [] for k in legs}
        for fn in legs.values():
            fn()
        for _ in range(args.reps):
            for k, fn in legs.items():
                pt[k].append(event_ms(fn)[0])
        for k, ts in pt.items():
            say(f"  {k:62s}{fmt(ts)}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
