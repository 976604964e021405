"""Grounding (csrc/ground.hip, include/gpn.h section GR): mask resize, mask pool, the k-nearest-neighbour vote and a whole
``PartGrounder.label_masks``, the vote against a torch formulation on the same GPU -> profiles/grounding_bench.txt.

    python tools/grounding_bench.py [--out profiles/grounding_bench.txt] [--reps 9] [--inner 20] [--no_sklearn]

Workload: K = 64 masks of 800 x 800, one 50 x 50 x 1024 feature map, a bank of 65 536 x 1024 float32 rows (268 MB) with 10
classes, k = 5.  The parent commit has no such path, so the baseline is what its user could have written in torch: ``cdist`` +
``topk`` + a one-hot vote for the classifier, a broadcast product + ``amax`` for the pool.  The resize has no torch counterpart
(Pillow's integer resample is not ``interpolate``), so it is timed alone.  scikit-learn's brute-force classifier on the CPU is
reported once, for scale.
Method: device events around ``--inner`` back-to-back calls (one call is too short for the clock), a warm-up of every leg, then
``--reps`` rounds in which the legs take turns; median [min .. max] per call.  The bank sweep's bandwidth is the bank's bytes over
the kNN call (its three launches), against the 8.0 TB/s HBM peak; the bank is about the size of the 256 MB last-level cache, so
back-to-back sweeps may find part of it there - the figure is a rate of bank bytes consumed, not a pure HBM measurement.
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

K, H, W, HF, WF, C, M, NK, CLASSES = 64, 800, 800, 50, 50, 1024, 65536, 5, 10
HBM_PEAK = 8.0e12


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def take_turns(legs, reps, inner):
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn, inner))
    return times


def line(name, ms):
    return f"  {name:<52s}{statistics.median(ms):9.4f} [{min(ms):9.4f} .. {max(ms):9.4f}]"


def workload(dev):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((K, H, W), dtype=bool)
    for k in range(K):
        cy, cx, ry, rx = rng.uniform(100, 700), rng.uniform(100, 700), rng.uniform(20, 250), rng.uniform(20, 250)
        masks[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    g = torch.Generator().manual_seed(0)
    centres = torch.randn(CLASSES, C, generator=g)
    labels = torch.randint(0, CLASSES, (M,), generator=g)
    bank = centres[labels] + 0.7 * torch.randn(M, C, generator=g)
    fea = torch.randn(HF, WF, C, generator=g)
    return torch.from_numpy(masks).to(dev), fea.to(dev), bank.to(dev), labels.to(dev)


def torch_knn(q, bank, labels):
    d = torch.cdist(q, bank)
    dist, idx = torch.topk(d, NK, dim=1, largest=False)
    votes = torch.nn.functional.one_hot(labels[idx], CLASSES).sum(1)
    return idx, dist, votes, votes.argmax(1)


def torch_pool(fea, levels):
    w = (128 - levels.clamp(max=128).float()) / 128
    return torch.stack([(fea * w[k][..., None]).amax((0, 1)) for k in range(levels.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grounding_bench.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no_sklearn", action="store_true")
    args = ap.parse_args()
    from gapartnet_amd.misc import grounding
    dev = torch.device("cuda:0")
    masks, fea, bank, labels = workload(dev)
    grounder = grounding.PartGrounder(bank, labels, k=NK, n_classes=CLASSES)
    levels = grounding.resize_masks(masks, (HF, WF))
    feats = grounding.pool_levels(fea, levels)
    out = [f"grounding: {K} masks of {H} x {W}, a {HF} x {WF} x {C} feature map, a bank of {M} x {C} f32 ({M * C * 4 / 1e6:.0f} MB), k = {NK}",
           f"ms per call: median [min .. max] of {args.reps} rounds of {args.inner} back-to-back calls by device events, after a warm-up of "
           "every leg; the legs take turns", f"device: {torch.cuda.get_device_name(0)}", ""]

    t = take_turns({"resize": lambda: grounding.resize_masks(masks, (HF, WF))}, args.reps, args.inner)
    ms = statistics.median(t["resize"])
    out += ["== gpn_ground_mask_resize: two launches ==", line("kernel", t["resize"]),
            f"  mask bytes read {K * H * W / 1e6:.0f} MB -> {K * H * W / ms / 1e9:.2f} TB/s ({K * H * W / ms / 1e9 / (HBM_PEAK / 1e12) * 100:.0f} % of the HBM peak); "
            "no torch counterpart", ""]

    t = take_turns({"kernel": lambda: grounding.pool_levels(fea, levels), "torch": lambda: torch_pool(fea, levels)}, args.reps, args.inner)
    diff = float((grounding.pool_levels(fea, levels) - torch_pool(fea, levels)).abs().max())
    out += ["== gpn_ground_mask_pool: one launch ==", line("kernel", t["kernel"]), line("torch formulation, same GPU (product + amax a mask)", t["torch"]),
            f"  torch / kernel: {statistics.median(t['torch']) / statistics.median(t['kernel']):.2f} x; max |kernel - torch| {diff:.1e}", ""]

    t = take_turns({"kernel": lambda: grounder.kneighbors(feats), "torch": lambda: torch_knn(feats, bank, labels)}, args.reps, args.inner)
    a, b = grounder.kneighbors(feats), torch_knn(feats, bank, labels)
    same = int((a["index"].long().sort(1).values == b[0].sort(1).values).all(1).sum())
    ms = statistics.median(t["kernel"])
    bw = M * C * 4 / (ms * 1e-3)
    ratio = statistics.median(t["torch"]) / ms
    out += [f"== gpn_ground_knn: {K} queries, three launches (query norms, sweep, merge + vote) ==", line("kernel", t["kernel"]),
            line("torch formulation, same GPU (cdist + topk + one-hot vote)", t["torch"]),
            f"  torch / kernel: {ratio:.2f} x ({'the kernel is faster' if ratio > 1 else 'the kernel is SLOWER than the torch formulation'}); "
            f"neighbour sets equal for {same} of {K} queries, labels equal for {int((a['label'].long() == b[3]).sum())}",
            f"  bank bytes consumed: {bw / 1e12:.2f} TB/s = {bw / HBM_PEAK * 100:.0f} % of the 8.0 TB/s HBM peak; "
            f"{2.0 * K * M * C / (ms * 1e-3) / 1e12:.1f} TFLOP/s of exact-fp32 MFMA work", ""]

    t = take_turns({"label_masks": lambda: grounder.label_masks(fea, masks)}, args.reps, args.inner)
    out += ["== PartGrounder.label_masks: resize + pool + kNN, six launches, no host read ==", line("kernels", t["label_masks"]), ""]

    if not args.no_sklearn:
        try:
            from sklearn.neighbors import KNeighborsClassifier
            X, y, q = bank.cpu().numpy(), labels.cpu().numpy(), feats.cpu().numpy()
            t0 = time.perf_counter()
            clf = KNeighborsClassifier(n_neighbors=NK, algorithm="brute").fit(X, y)
            t1 = time.perf_counter()
            pred = clf.predict(q)
            t2 = time.perf_counter()
            out += ["== for scale: scikit-learn KNeighborsClassifier(brute) on the CPU, one run ==",
                    f"  fit {1e3 * (t1 - t0):.1f} ms, predict {1e3 * (t2 - t1):.1f} ms; labels equal to the kernel's for "
                    f"{int((pred == a['label'].cpu().numpy()).sum())} of {K} queries", ""]
        except ImportError:
            out += ["== scikit-learn is not installed: the CPU figure was not measured ==", ""]
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
