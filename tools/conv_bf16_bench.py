"""The bf16 inference conv against the fp32 conv at the bench's level shapes (8 x 20k-point scenes, voxel 0.01; every subm / down /
inverse conv of levels 0-6, the list tools/conv_tiles_bench.py builds).

Per shape three launches, timed ALTERNATING in one process through the C ABI (device events around back-to-back launches, warm-up
per shape, packed weights and prebuilt rulebooks outside the timed region):
  fp32     gpn_spconv_fwd_ordered - the public form, no epilogue
  bf16     gpn_spconv_fwd_bf16 without epilogue, bf16 store (the like-for-like pair)
  bf16+ep  gpn_spconv_fwd_bf16 with BatchNorm + residual + ReLU + bf16 store (what the network executor launches)
Each is timed `--rounds` times in turn; the median is reported and, next to the fp32 figure, the spread (min .. max) of its repeated
runs - a bf16 / fp32 difference inside that spread is no difference.  Algorithmic bytes = rows (cin + cout) element size
(+ the residual's rows cout 2 for bf16+ep) + the neighbour table (K n_dst 4) + the weights (K cin cout element size): what the conv
has to move at least once, not what the gather re-reads.

    python tools/conv_bf16_bench.py [--levels 7] [--iters 40] [--warm 5] [--rounds 5]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from gapartnet_amd import _C, hip_ops as H
from gapartnet_amd.smoke import make_batch
from gapartnet_amd.structure.point_cloud import PointCloud

dev = torch.device("cuda:0")
L = _C.lib()


def timeit(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def fp32_call(x, packed, rb, cin, cout, out):
    ws_ptr, ws_size, stream = H._fast_ws(dev)
    rc = L.gpn_spconv_fwd_ordered(H.ptr(x), H.ptr(packed), H.ptr(rb.nbr), H.ptr(rb.nbr_p), H.ptr(rb.perm), H.i32(rb.K),
                                  H.i64(rb.n_dst), H.i32(cin), H.i32(cout), H.ptr(out), ctypes.c_void_p(ws_ptr),
                                  ctypes.c_size_t(ws_size), ctypes.c_void_p(stream))
    assert rc == 0, L.gpn_last_error()


def bf16_call(x, packed, rb, cin, cout, ep, out):
    rc = L.gpn_spconv_fwd_bf16(H.ptr(x), H.ptr(packed), H.ptr(rb.nbr), H.ptr(rb.nbr_p), H.ptr(rb.perm), H.i32(rb.K), H.i64(rb.n_dst),
                               H.i32(cin), H.i32(cout), ctypes.byref(ep) if ep is not None else None, H.ptr(out), H._stream())
    assert rc == 0, L.gpn_last_error()


def level_shapes(n_levels):
    """[(level, kind, rulebook, cin, cout)] as tools/conv_tiles_bench.py builds them"""
    torch.manual_seed(0)
    pcs = [pc.to(dev) for pc in make_batch(8, 20000)]
    batch = PointCloud.collate(pcs, voxel_size=(0.01, 0.01, 0.01))
    idx, shape = batch.voxel_tensor.indices, list(batch.voxel_tensor.spatial_shape)
    out = []
    for lvl in range(n_levels):
        rb = H.rulebook_subm3(idx, shape)
        c = 16 * (lvl + 1)
        out += [(lvl, "subm", rb, c, c), (lvl, "subm", rb, 2 * c, c)]
        if lvl + 1 < n_levels:
            idx, shape, rbd, rbu = H.rulebook_down(idx, shape, 8)
            out += [(lvl, "down", rbd, c, c + 16), (lvl, "inv", rbu, c + 16, c)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="alternating timing rounds per shape (median reported)")
    args = ap.parse_args()
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"# {torch.cuda.get_device_name(0)}; {args.rounds} alternating rounds x {args.iters} launches per shape and form, "
          f"{args.warm} warm-up launches; us = median, [min .. max] = the spread of the fp32 rounds")
    print(f"{'level rows':>13s} {'conv':>15s} | {'fp32 us':>8s} {'[spread]':>15s} {'MB':>7s} {'GB/s':>6s} | {'bf16 us':>8s} {'MB':>7s} "
          f"{'GB/s':>6s} {'x fp32':>6s} | {'bf16+ep us':>10s} {'MB':>7s} {'GB/s':>6s} {'x fp32':>6s}")
    slower = []
    for lvl, kind, rb, cin, cout in level_shapes(args.levels):
        K, n_src, n_dst = rb.K, rb.n_src, rb.n_dst
        x32 = torch.randn(n_src, cin, device=dev)
        w = torch.randn(K, cin, cout, device=dev) / (K * cin) ** 0.5
        p32, p16 = H.pack_weights(w, 0), H.conv_pack_bf16(w)
        x16 = H.rows_to_bf16(x32)
        res = H.rows_to_bf16(torch.randn(n_dst, cout, device=dev))
        o32 = torch.empty(n_dst, cout, device=dev)
        o16 = torch.empty(n_dst, cout, device=dev, dtype=torch.bfloat16)
        bn = [torch.randn(cout, device=dev) * 0.3, torch.rand(cout, device=dev) + 0.5, torch.rand(cout, device=dev) + 0.5,
              torch.randn(cout, device=dev) * 0.2]
        ep = H._EpilogueBf16(bn[0].data_ptr(), bn[1].data_ptr(), bn[2].data_ptr(), bn[3].data_ptr(), res.data_ptr(), 1e-4, 1, 0)
        forms = [lambda: fp32_call(x32, p32, rb, cin, cout, o32), lambda: bf16_call(x16, p16, rb, cin, cout, None, o16),
                 lambda: bf16_call(x16, p16, rb, cin, cout, ep, o16)]
        for f in forms:  # warm-up of every form of this shape before the first timed round
            timeit(f, args.warm, args.warm)
        t = [[], [], []]
        for _ in range(args.rounds):
            for i, f in enumerate(forms):
                t[i].append(timeit(f, args.iters, args.warm))
        table = K * n_dst * 4
        rows = n_src * cin + n_dst * cout
        mb = [(rows * 4 + table + K * cin * cout * 4) / 1e6, (rows * 2 + table + K * cin * cout * 2) / 1e6,
              (rows * 2 + n_dst * cout * 2 + table + K * cin * cout * 2) / 1e6]
        us = [med(v) for v in t]
        gbs = [mb[i] * 1e6 / (us[i] * 1e-6) / 1e9 for i in range(3)]
        print(f"L{lvl} {n_dst:10d} {kind:>5s} {cin:3d}->{cout:<3d} K{K:<2d} | {us[0]:8.1f} [{min(t[0]):6.1f}..{max(t[0]):6.1f}] {mb[0]:7.2f} "
              f"{gbs[0]:6.0f} | {us[1]:8.1f} {mb[1]:7.2f} {gbs[1]:6.0f} {us[1] / us[0]:6.2f} | {us[2]:10.1f} {mb[2]:7.2f} {gbs[2]:6.0f} "
              f"{us[2] / us[0]:6.2f}")
        if us[1] > max(t[0]):
            slower.append(f"L{lvl} {kind} {cin}->{cout}: bf16 {us[1]:.1f} us vs fp32 {us[0]:.1f} us (fp32 rounds up to {max(t[0]):.1f})")
    print("# shapes whose bf16 conv (no epilogue) is slower than every fp32 round: " + ("; ".join(slower) if slower else "none"))


if __name__ == "__main__":
    main()
