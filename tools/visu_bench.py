"""Scenes per second of the test-time rendering (gapartnet_amd/misc/visu.py) for a batch of 8 synthetic scenes of 20 000 points with
all twelve options, against the numpy restatement of the same contracts (tests/visu_ref.py) on the same box:
  (a) the four launches alone (render_panels: winner, paint, pred boxes, GT boxes; inputs and boxes already on the device)
  (b) device -> host copy of the canvas plus PNG encoding on the host threads
  (c) end to end on files (visualize_scenes: reading the scene files, the GT fits, rendering, copying, captions, PNG files)
  (r) the numpy restatement of (a), per scene
Warm-up first, then alternating legs (a), (r), (a), (r) ...; medians.  The parent commit has no such path: (r) is the baseline.

    python tools/visu_bench.py [--scenes 8] [--points 20000] [--reps 7] [--out profiles/visu_bench.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gapartnet_amd.dataset import synthetic  # noqa: E402
from gapartnet_amd.misc import visu  # noqa: E402
from tests import visu_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref_scenes", type=int, default=2, help="scenes the restatement renders per leg (it is per scene)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visu_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, n = a.scenes, a.points
    rng = np.random.default_rng(0)
    palette = visu.default_palette()
    scenes = []
    for s in range(S):
        xyz, rgb, sem, ins, npcs, _ = synthetic.make_scene_arrays(9000 + s, n)
        scenes.append(dict(xyz=xyz.astype(np.float32), rgb=rgb.astype(np.float32), sem_gt=sem.astype(np.int32), ins_gt=ins.astype(np.int32),
                           npcs_gt=npcs.astype(np.float32), sem_pred=rng.integers(0, 10, n).astype(np.int32),
                           ins_pred=rng.integers(0, 30, n).astype(np.int32), npcs_pred=rng.uniform(0, 1, (n, 3)).astype(np.float32),
                           trans=np.asarray([0.5, 0.0, 0.0, 1.8])))
    off = np.arange(S + 1) * n
    cat = lambda k: torch.as_tensor(np.concatenate([sc[k] for sc in scenes])).to(dev)
    d = {k: cat(k) for k in ("xyz", "rgb", "sem_gt", "ins_gt", "npcs_gt", "sem_pred", "ins_pred", "npcs_pred")}
    trans = torch.as_tensor(np.stack([sc["trans"] for sc in scenes])).to(dev)
    np.random.seed(0)
    bbox, bscene = visu.gt_boxes(d["xyz"], d["ins_gt"], d["npcs_gt"], off)
    for s, sc in enumerate(scenes):
        sc["bbox_gt"] = sc["bbox_pred"] = bbox[bscene == s].cpu().numpy()
    lines = [f"# tools/visu_bench.py: {S} synthetic scenes x {n} points, 12 options, {visu.HEIGHT}x{visu.WIDTH} tiles, "
             f"{int(bbox.shape[0])} boxes, {torch.cuda.get_device_name(dev)}"]

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def launches():
        return visu.render_panels(d["xyz"], d["rgb"], off, trans, sem_pred=d["sem_pred"], ins_pred=d["ins_pred"],
                                  npcs_pred=d["npcs_pred"], bbox_pred=bbox, bbox_pred_scene=bscene, sem_gt=d["sem_gt"],
                                  ins_gt=d["ins_gt"], npcs_gt=d["npcs_gt"], bbox_gt=bbox, bbox_gt_scene=bscene, palette=palette)

    def restatement():
        for sc in scenes[:a.ref_scenes]:
            R.assemble(R.render_tiles(sc, palette, visu.HEIGHT, visu.WIDTH, options=visu.OPTIONS[1:]), visu.HEIGHT, visu.WIDTH, visu.EDGE)

    def timed(fn, sync):
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for _ in range(2):   # warm-up
        canvas = launches()
    torch.cuda.synchronize()
    restatement()
    ta, tr = [], []
    for _ in range(a.reps):
        ta.append(timed(launches, True)[0])
        tr.append(timed(restatement, False)[0] / a.ref_scenes)
    ma, mr = statistics.median(ta), statistics.median(tr)
    log(f"(a) four launches, batch of {S}: median {ma * 1e3:.2f} ms (min {min(ta) * 1e3:.2f}, max {max(ta) * 1e3:.2f}) = {S / ma:.1f} scenes/s")
    log(f"(r) numpy restatement: median {mr * 1e3:.1f} ms/scene (min {min(tr) * 1e3:.1f}, max {max(tr) * 1e3:.1f}) = {1 / mr:.2f} scenes/s")
    log(f"(a) / (r) = {(S / ma) * mr:.0f}x")

    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as pool:
        def copy_and_encode():
            host = canvas.cpu().numpy()
            jobs = [pool.submit(visu._write_panel, host[s], os.path.join(tmp, f"b{s}.png"), visu.OPTIONS[1:], False, None,
                                visu.HEIGHT, visu.WIDTH, visu.EDGE) for s in range(S)]
            [j.result() for j in jobs]
        copy_and_encode()
        tb = [timed(copy_and_encode, False)[0] for _ in range(a.reps)]
        mb = statistics.median(tb)
        log(f"(b) device -> host + captions + PNG (8 threads), batch of {S}: median {mb * 1e3:.0f} ms = {S / mb:.1f} scenes/s")
        # (c) files in, files out
        root = os.path.join(tmp, "data")
        os.makedirs(os.path.join(root, "val", "pth"))
        os.makedirs(os.path.join(root, "val", "meta"))
        names = [f"StorageFurniture_{s:05d}_00_000" for s in range(S)]
        for name, sc in zip(names, scenes):
            torch.save((sc["xyz"], sc["rgb"], sc["sem_gt"], sc["ins_gt"], sc["npcs_gt"]), os.path.join(root, "val", "pth", name + ".pth"))
            np.savetxt(os.path.join(root, "val", "meta", name + ".txt"), sc["trans"])

        def end_to_end():
            visu.visualize_scenes(os.path.join(tmp, "out"), root, "", list(visu.OPTIONS), names, "val", dev,
                                  [sc["sem_pred"] for sc in scenes], [sc["ins_pred"] for sc in scenes],
                                  [sc["npcs_pred"] for sc in scenes], [sc["bbox_pred"] for sc in scenes], batch=S, pool=pool)
        end_to_end()
        tc = [timed(end_to_end, False)[0] for _ in range(max(a.reps // 2, 3))]
        mc = statistics.median(tc)
        log(f"(c) end to end on files, batch of {S}: median {mc * 1e3:.0f} ms = {S / mc:.2f} scenes/s")
        log(f"(c) / (r) = {(S / mc) * mr:.1f}x  (the restatement draws tiles only: no files, no fits, no PNG)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
