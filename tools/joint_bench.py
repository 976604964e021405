"""Joint estimation: the CPD rigid registration of a batch of pairs, three ways (csrc/joint.hip; gapartnet_amd/misc/joint_fitting.py)
-> profiles/joint_bench.txt.

    python tools/joint_bench.py [--out profiles/joint_bench.txt] [--reps 5]

Workload: hinge pairs (a slab turned 25 degrees about an edge, 1 mm noise), K rows sampled independently from each observation and
normalised as gpn_joint_sample does; default settings (max_iterations 100, tolerance 1e-3).  Sizes: K = 500 for B = 1, 16, 128 and
K = 2048 for B = 16.  Three paths over the same inputs:
  kernel   gpn_cpd_rigid: one launch, one workgroup a pair, the whole EM loop on the device (device events)
  torch    the torch formulation of the same contract on the same GPU - dense [B, K, K] responsibilities, a host read of "has
           every pair stopped" per iteration: what the parent commit's user could write, the parent having no path (device
           events).  It is the plain, untuned statement of the contract: the ratios are against a simple baseline
  numpy    the float64 oracle of tests/joint_ref.py on the CPU, pair after pair (wall clock; timed on at most 2 pairs, 1 at K = 2048)
Medians of --reps runs after a warm-up run of every shape, kernel and torch taking turns.  The iteration counts are reported next to
the times because the work differs by input, and the kernel's rate as exponentials per second (iterations x M x N per pair: the
kernel evaluates every responsibility once per iteration).  Then the accuracy table of tests/test_gpu_joint.py: the oracle's own
spread under a row permutation and the kernel's error, per pair and iteration count.
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

SIZES = ((500, 1), (500, 16), (500, 128), (2048, 16))


def make_pairs(B, K, seed=100):
    from tests import joint_ref as JR
    X, Y = np.zeros((B, K, 3)), np.zeros((B, K, 3))
    for b in range(B):
        pc1, pc2, _ = JR.hinge_pair(seed + b, 25.0, 2 * K, 2 * K)
        rng = np.random.RandomState(seed + b)
        X[b], Y[b], _ = JR.joint_sample_ref(pc1, pc2, rng.choice(2 * K, K, replace=False), rng.choice(2 * K, K, replace=False))
    return X, Y


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("joint_bench needs a GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    from gapartnet_amd.misc import joint_fitting as JF
    from tests import joint_ref as JR
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    fh = open(args.out, "w")

    def say(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    say("joint estimation: CPD rigid registration of B pairs of K x K points, max_iterations 100, tolerance 1e-3")
    say(f"median [min .. max] of {args.reps} in ms, warmed up; kernel and torch by device events, taking turns; numpy by wall clock")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say("the torch formulation is the plain statement of the contract (it builds the [B, K, K, 3] differences twice an iteration); it is")
    say("not tuned - an expanded |x|^2 + |y|^2 - 2 x.y form would be cheaper - so the ratios are against a simple baseline")
    say()
    ratios = {}
    for K, B in SIZES:
        X, Y = make_pairs(B, K)
        Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
        n = torch.full((B,), K, dtype=torch.int32, device=dev)

        def kernel():
            return JF.cpd_rigid_batched(Xd, Yd, n, n)

        def formulation():
            return JF.cpd_rigid_batched(Xd, Yd, n, n, formulation="torch")
        got, ref = kernel(), formulation()   # warm-up
        torch.cuda.synchronize()
        tk, tt = [], []
        for _ in range(args.reps):
            tk.append(event_ms(kernel)[0])
            tt.append(event_ms(formulation)[0])
        pairs = min(B, 1 if K > 1000 else 2)
        t0 = time.perf_counter()
        oracle = [JR.cpd_rigid_ref(X[b], Y[b]) for b in range(pairs)]
        t_np = (time.perf_counter() - t0) * 1e3 / pairs
        its = got["iterations"].cpu().numpy()
        its_t = ref["iterations"].cpu().numpy()
        dR = float((got["R"] - ref["R"]).abs().max())
        mk, mt = statistics.median(tk), statistics.median(tt)
        exps = float(its.sum()) * K * K
        say(f"== K = {K}, B = {B} ==")
        say(f"  iterations: kernel {its.min()} .. {its.max()} (mean {its.mean():.1f}); torch {its_t.min()} .. {its_t.max()}; "
            f"numpy {[o['iterations'] for o in oracle]} (first {pairs}); kernel and torch counts equal: {bool((its == its_t).all())}; "
            f"max |R kernel - R torch| {dR:.1e}")
        say(f"  {'kernel (gpn_cpd_rigid, one launch)':<48} {fmt(tk)}   {B / mk * 1e3:10.1f} pairs/s   {exps / mk / 1e6:8.2f} G exp/s")
        say(f"  {'torch formulation, same GPU':<48} {fmt(tt)}   {B / mt * 1e3:10.1f} pairs/s")
        say(f"  {'numpy oracle, CPU (per pair, wall clock)':<48} {t_np:10.3f}                            {1e3 / t_np:10.1f} pairs/s")
        say(f"  torch / kernel: {mt / mk:.2f} x; numpy / kernel (per pair): {t_np / (mk / B):.1f} x")
        say()
        ratios[(K, B)] = mt / mk
        del Xd, Yd, got, ref
    if ratios[(500, 16)] < 1.0:
        say("NOTE: at B = 16, K = 500 the kernel path is SLOWER than the torch formulation on the same GPU.")
        say()

    # the accuracy table of tests/test_gpu_joint.py (the shared batch and the oracle's spread: tests/joint_ref.py)
    Xb, Yb, nx, ny = JR.cpd_batch()
    Xd, Yd = torch.from_numpy(Xb).to(dev), torch.from_numpy(Yb).to(dev)
    say("== accuracy (tests/test_gpu_joint.py): the oracle's spread under a row permutation, the kernel's error, tolerance 0 ==")
    for iterations in (1, 5, 30):
        got = JF.cpd_rigid_batched(Xd, Yd, torch.from_numpy(nx), torch.from_numpy(ny), tolerance=0.0, max_iterations=iterations)
        got = {k: v.cpu().numpy() for k, v in got.items()}
        for b, o in JR.cpd_oracle().items():
            spread = o["spread"][iterations - 1]
            err = JR.state_gap((got["s"][b], got["R"][b], got["t"][b], got["sigma2"][b]), o["history"][iterations - 1])
            say(f"  iterations {iterations:2d} pair {str(JR.CPD_SHAPES[b][0]):<12} spread {spread:.2e}  kernel error {err:.2e}  ratio {err / spread:5.1f}"
                f"  (allowed 64)")
    fh.close()


if __name__ == "__main__":
    main()
