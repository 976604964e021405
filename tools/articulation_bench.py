"""Articulation from two frames, stage by stage (gapartnet_amd/misc/articulation.py; csrc/articulate.hip; include/gpn.h section AR)
-> profiles/articulation_bench.txt.

    python tools/articulation_bench.py [--out profiles/articulation_bench.txt] [--reps 5] [--frames 8] [--height 720] [--width 1280]

Workload: --frames frame pairs of --width x --height with about 60 % valid depth (the workload of tools/frame_bench.py), 16 parts a
frame: a 4 x 4 grid of rectangles over a wall, each at its own depth; frame B has the grid shifted by a few pixels, every part
moved a little towards the camera and the numbering permuted.  500 samples a side.  Device-event times in ms, medians of --reps
runs, warmed up, the legs taking turns inside every repetition:
  new       gpn_parts_overlap, gpn_parts_match, gpn_parts_gather (one side), and the whole of articulation_from_maps
            (back-projection of both frames, overlap, match, the one host read, both gathers, ONE joint pass over all pairs)
  baseline  what a user of the parent commit can do on the same GPU: the contingency table by torch ops (a bincount over
            i * PB + j a frame pair), the greedy matching on the host, then one joints_from_frames per matched part - which
            back-projects both frames and sorts every pixel of both frames once per part
The two paths' matches are asserted equal.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s (MI355X)


def make_pairs(V, H, W, seed=0, valid=0.6, grid=4):
    """depth_a, depth_b f32 [V,H,W] (0 = hole), inst_a, inst_b i32 [V,H,W], classes [V][grid^2] i64, K [3,3]"""
    rng = np.random.RandomState(seed)
    P = grid * grid
    f = 0.9 * W
    K = np.array([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]])
    out = {k: [] for k in ("depth_a", "depth_b", "inst_a", "inst_b", "cls_a", "cls_b")}
    ch, cw = H // grid, W // grid
    for v in range(V):
        cls = rng.randint(1, 10, size=P).astype(np.int64)
        z = 1.0 + rng.rand(P) * 0.8
        perm = rng.permutation(P)
        for side, shift, dz, number in (("a", 0, 0.0, np.arange(P)), ("b", 6, -0.03, perm)):
            d = np.full((H, W), 2.5, np.float32) + rng.rand(H, W).astype(np.float32) * 0.01
            inst = np.full((H, W), -1, np.int32)
            for p in range(P):
                r, c = divmod(p, grid)
                y0, x0 = r * ch + ch // 8 + shift, c * cw + cw // 8 + shift
                d[y0:y0 + 3 * ch // 4, x0:x0 + 3 * cw // 4] = z[p] + dz
                inst[y0:y0 + 3 * ch // 4, x0:x0 + 3 * cw // 4] = number[p]
            d[rng.rand(H, W) >= valid] = 0
            out["depth_" + side].append(d)
            out["inst_" + side].append(inst)
            c_side = np.zeros(P, np.int64)
            c_side[number] = cls
            out["cls_" + side].append(c_side)
    return {k: (np.stack(x) if k[:3] != "cls" else x) for k, x in out.items()}, K


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "articulation_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    args = ap.parse_args()
    from gapartnet_amd import hip_ops
    from gapartnet_amd.misc import articulation as AR
    from gapartnet_amd.misc import joint_fitting as JF
    dev = torch.device("cuda:0")
    V, H, W = args.frames, args.height, args.width
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    d, K = make_pairs(V, H, W)
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    da, db, ia, ib = t(d["depth_a"]), t(d["depth_b"]), t(d["inst_a"]), t(d["inst_b"])
    cls_a, cls_b = d["cls_a"], d["cls_b"]
    P = len(cls_a[0])
    n = [P] * V
    rgb = torch.zeros((V, H, W, 3), dtype=torch.uint8, device=dev)
    Kd = torch.from_numpy(np.stack([K] * V)).to(dev)
    rows_a, valid_a, _ = hip_ops.frame_backproject(da, rgb, Kd)
    rows_b, valid_b, _ = hip_ops.frame_backproject(db, rgb, Kd)
    ca, cb = AR._class_table([torch.from_numpy(c) for c in cls_a], P, dev), AR._class_table([torch.from_numpy(c) for c in cls_b], P, dev)
    inter, area_a, area_b = hip_ops.parts_overlap(ia, valid_a, n, ib, valid_b, n, P, P)
    m = hip_ops.parts_match(inter, area_a, area_b, n, n, ca, cb, 0.1)
    match_ab, areas = m["match_ab"].cpu().numpy(), area_a.cpu().numpy()
    seg = np.full((V, P), -1, np.int64)
    live = match_ab >= 0
    seg[live] = np.concatenate([[0], np.cumsum(areas[live])])[:-1]
    seg_t, n_total = torch.from_numpy(seg).to(dev), int(areas[live].sum())
    G = int(live.sum())
    say(f"articulation from two frames: {V} frame pairs of {W} x {H}, {100 * float((da > 0).double().mean()):.0f} % valid depth, {P} parts a "
        f"frame, {G} matched pairs, {n_total} member pixels a side, 500 samples a side")
    say(f"median [min .. max] of {args.reps} in ms (device events), warmed up, the legs taking turns; device: {torch.cuda.get_device_name(0)}")

    def torch_table():
        out = []
        for v in range(V):
            ka = torch.where((valid_a[v] != 0) & (ia[v] >= 0) & (ia[v] < P), ia[v], -1).reshape(-1).long()
            kb = torch.where((valid_b[v] != 0) & (ib[v] >= 0) & (ib[v] < P), ib[v], -1).reshape(-1).long()
            both = (ka >= 0) & (kb >= 0)
            out.append(torch.stack([torch.bincount(ka[ka >= 0], minlength=P), torch.bincount(kb[kb >= 0], minlength=P)]))
            out.append(torch.bincount((ka * P + kb)[both], minlength=P * P).reshape(P, P))
        return out

    def baseline_match():
        got = torch_table()
        tab = [x.cpu().numpy() for x in got]   # (the host read of the tables)
        inter_h = np.stack(tab[1::2]).astype(np.int32)
        area = np.stack(tab[0::2]).astype(np.int32)
        return AR._match_numpy(inter_h, area[:, 0], area[:, 1], n, n, ca_h, cb_h, 0.1)[0]

    ca_h, cb_h = ca.cpu().numpy(), cb.cpu().numpy()
    assert np.array_equal(baseline_match(), match_ab), "the two paths match the same parts"

    def baseline_all():
        mab = baseline_match()
        out = []
        for v in range(V):
            for i in np.flatnonzero(mab[v] >= 0):
                out.append(JF.joints_from_frames(da[v], db[v], K, (ia[v] == int(i)), (ib[v] == int(mab[v, i]))))
        return out

    new_all = lambda: AR.articulation_from_maps(da, db, K, ia, ib, cls_a, cls_b)  # noqa: E731
    legs = {
        "new: gpn_parts_overlap": lambda: hip_ops.parts_overlap(ia, valid_a, n, ib, valid_b, n, P, P),
        "new: gpn_parts_match": lambda: hip_ops.parts_match(inter, area_a, area_b, n, n, ca, cb, 0.1),
        "new: gpn_parts_gather (one side)": lambda: hip_ops.parts_gather(rows_a, ia, valid_a, n, seg_t, n_total),
        "new: back-projection of both frames": lambda: (hip_ops.frame_backproject(da, rgb, Kd), hip_ops.frame_backproject(db, rgb, Kd)),
        "new: articulation_from_maps (everything)": new_all,
        "baseline: contingency tables by torch ops": torch_table,
        "baseline: tables + host read + matching on the host": baseline_match,
        "baseline: ... + one joints_from_frames per matched part": baseline_all,
    }
    times = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    for _ in range(args.reps):
        for k, fn in legs.items():
            times[k].append(event_ms(fn)[0])
    for k, ts in times.items():
        say(f"  {k:62s}{fmt(ts)}")
    art = new_all()
    pc = hip_ops.parts_gather(rows_a, ia, valid_a, n, seg_t, n_total)
    sizes1, sizes2 = art.n_points_a.tolist(), art.n_points_b.tolist()
    seg_b = np.full((V, P), -1, np.int64)   # (the B side's segments in the order of the pairs, as articulation_from_maps lays them out)
    seg_b[np.nonzero(live)[0], match_ab[live]] = np.concatenate([[0], np.cumsum(sizes2)])[:-1]
    pc2 = hip_ops.parts_gather(rows_b, ib, valid_b, n, torch.from_numpy(seg_b).to(dev), sum(sizes2))
    assert pc.shape[0] == sum(sizes1) and np.array_equal(art.part_b, match_ab[live])
    ts = [event_ms(lambda: JF.estimate_joints_packed(pc, pc2, sizes1, sizes2))[0] for _ in range(args.reps + 1)][1:]
    say(f"  {'the joint pass alone (estimate_joints_packed, ' + str(G) + ' pairs)':62s}{fmt(ts)}")
    med = lambda k: statistics.median(times[k])  # noqa: E731
    px = float(V * H * W)
    # least bytes: overlap reads two i32 maps and two u8 maps once; gather reads one of each twice (the count pass and the store
    # pass, 5 bytes a pixel each), 12 bytes of every kept row, and writes 24
    say(f"  overlap: {px * 10 / (med('new: gpn_parts_overlap') * 1e-3) / 1e12:6.2f} TB/s of its least bytes (10 a pixel) against {HBM_PEAK / 1e12:.1f} TB/s")
    say(f"  gather:  {(px * 10 + n_total * 36.0) / (med('new: gpn_parts_gather (one side)') * 1e-3) / 1e12:6.2f} TB/s of its least bytes "
        f"(two passes of 5 a pixel, 12 in and 24 out a kept row)")
    say(f"  whole call, new against baseline: {med('baseline: ... + one joints_from_frames per matched part') / med('new: articulation_from_maps (everything)'):.1f} x")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
