"""Rendered RGB-D views -> GAPartNet training scenes on the GPU.

The reference's dataset/process_tools/convert_rendered_into_input.py turns the renderer's output (rgb/*.png,
depth/*.npz['depth_map'], segmentation/*.npz['semantic_segmentation', 'instance_segmentation'], npcs/*.npz['npcs_map'],
metafile/*.json) into the training set: per view pth/<name>.pth (the 6-tuple of numpy arrays the loaders read), meta/<name>.txt
(scale_param) and gt/<name>.txt (evaluation labels).  Here the per-view work - back-projection, furthest point sampling,
ball normalisation, relabelling - runs for a batch of views at a time in the three launches of include/gpn.h section VP, and the
files are the reference's: the same arrays bit for bit after torch.load, the same bytes in the text files.

    python -m gapartnet_amd.dataset.convert_rendered --data_path <renders> --save_path <out> [--dataset partnet|akb48]
        [--num_points 20000] [--batch 16] [--workers 8] [--log ./log_sample.txt]

Differences from the reference ("Behavioural differences"): a view whose labels disagree ((sem == -1) !=
(ins == -1) at a valid pixel, where the reference asserts after writing nothing and stops the run) or whose sampled instance ids
reach the library's table bound gets a status, a log line and no files, and the run goes on; the log goes to --log.
"""
import argparse
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

PARTNET_OBJECT_CATEGORIES = [
    'Box', 'Camera', 'CoffeeMachine', 'Dishwasher', 'KitchenPot', 'Microwave', 'Oven', 'Phone', 'Refrigerator',
    'Remote', 'Safe', 'StorageFurniture', 'Table', 'Toaster', 'TrashCan', 'WashingMachine', 'Keyboard', 'Laptop', 'Door', 'Printer',
    'Suitcase', 'Bucket', 'Toilet'
]
AKB48_OBJECT_CATEGORIES = ['Box', 'TrashCan', 'Bucket', 'Drawer']
MAX_INSTANCE_NUM = 1000
LOG_PATH = './log_sample.txt'
MAX_WORKERS = 16
STAGING_BYTES = 1 << 30  # pinned host staging of one batch's inputs

# per-view status (include/gpn.h GPN_VIEW_*)
VIEW_OK, VIEW_TOO_FEW, VIEW_LABEL_MISMATCH, VIEW_INSTANCE_BOUND = 0, 1, 2, 3


@dataclass
class ViewResult:
    status: int
    arrays: Optional[tuple] = None  # (xyz f32 [m,3], rgb f32 [m,3], sem i32 [m], ins i32 [m], npcs f32 [m,3], idx i32 [m,2])
    scale_param: Optional[np.ndarray] = None  # f64 [4] = (radius, cx, cy, cz)
    gt: Optional[np.ndarray] = None  # i32 [m]


def _tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def _labels_i32(a, what):
    t = _tensor(a)
    if t.dtype == torch.int32:
        return t
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError(f"{what} must be an integer map, got {t.dtype}")
    if t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
        raise ValueError(f"{what} holds values outside int32")
    return t.to(torch.int32)


def convert_views(rgb, depth, sem, ins, npcs, K, num_points, device=None, max_groups=0) -> List[ViewResult]:
    """One batch of V views of one size H x W -> a ViewResult per view.

    rgb [V,H,W,3] uint8, depth [V,H,W] float32 or float64 (used as given: float64 depth is supported, never cast), sem / ins
    [V,H,W] integer maps (-2 background, -1 "others"), npcs [V,H,W,3], K [V,3,3] float64.  numpy arrays or torch tensors (host,
    pinned or already on the device).  The same call serves the frames of a live depth camera.  A batch costs one host read."""
    from .. import hip_ops
    depth = _tensor(depth)
    if depth.dim() != 3:
        raise ValueError(f"depth must be [V,H,W], got {tuple(depth.shape)}")
    if depth.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"depth must be float32 or float64, got {depth.dtype}")
    V, H, W = depth.shape
    rgb = _tensor(rgb)
    if rgb.dtype != torch.uint8 or tuple(rgb.shape) != (V, H, W, 3):
        raise ValueError(f"rgb must be uint8 [V,H,W,3], got {rgb.dtype} {tuple(rgb.shape)}")
    sem, ins = _labels_i32(sem, "sem"), _labels_i32(ins, "ins")
    npcs = _tensor(npcs)
    if npcs.dtype != torch.float32:  # the reference casts the gathered rows to float32: the same values
        npcs = npcs.to(torch.float32)
    K = _tensor(np.asarray(K, dtype=np.float64)) if not isinstance(K, torch.Tensor) else K.to(torch.float64)
    K = K.reshape(V, 3, 3)
    if tuple(sem.shape) != (V, H, W) or tuple(ins.shape) != (V, H, W) or tuple(npcs.shape) != (V, H, W, 3):
        raise ValueError("sem / ins must be [V,H,W] and npcs [V,H,W,3]")
    if V == 0:
        return []
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def up(t):
        return t.to(device, non_blocking=True)

    buf, layout = hip_ops.view_convert(up(depth), up(rgb), up(sem), up(ins), up(npcs), up(K), int(num_points), max_groups)
    f = {k: v.numpy() for k, v in hip_ops.view_fields(buf.cpu(), layout).items()}  # the batch's one host read
    out = []
    for v in range(V):
        st = int(f["status"][v])
        if st != VIEW_OK:
            out.append(ViewResult(st))
            continue
        arrays = (f["xyz"][v], f["rgb"][v], f["sem"][v], f["ins"][v], f["npcs"][v], f["pix"][v])
        out.append(ViewResult(st, arrays, f["scale"][v], f["gt"][v]))
    return out


# ---------------------------------------------------------------------------------------------------- files
def read_view(data_path, name):
    """one view in the renderer's layout (the reference's utils/read_utils.py; bbox/*.pkl is not needed)"""
    from PIL import Image
    rgb = np.array(Image.open(os.path.join(data_path, 'rgb', f'{name}.png')))
    depth = np.load(os.path.join(data_path, 'depth', f'{name}.npz'))['depth_map']
    seg = np.load(os.path.join(data_path, 'segmentation', f'{name}.npz'))
    npcs = np.load(os.path.join(data_path, 'npcs', f'{name}.npz'))['npcs_map']
    with open(os.path.join(data_path, 'metafile', f'{name}.json')) as fh:
        meta = json.load(fh)
    K = np.array(meta['camera_intrinsic'], dtype=np.float64).reshape(3, 3)
    return dict(rgb=rgb, depth=depth, sem=seg['semantic_segmentation'], ins=seg['instance_segmentation'], npcs=npcs, K=K)


def write_view(save_path, name, res: ViewResult):
    """the reference's three files of a converted view (:156-173)"""
    torch.save(tuple(res.arrays), os.path.join(save_path, 'pth', name + '.pth'))
    np.savetxt(os.path.join(save_path, 'meta', name + '.txt'), res.scale_param, delimiter=',')
    np.savetxt(os.path.join(save_path, 'gt', name + '.txt'), res.gt, fmt='%d')


def category_lists(names, categories):
    """names grouped by the first category they start with, in category order (:203-209); other names are skipped"""
    groups = {c: [] for c in categories}
    for fn in names:
        for c in categories:
            if fn.startswith(c):
                groups[c].append(fn)
                break
    return groups


def scan(data_path, dataset):
    if dataset == 'partnet':
        categories = PARTNET_OBJECT_CATEGORIES
    elif dataset == 'akb48':
        categories = AKB48_OBJECT_CATEGORIES
    else:
        raise ValueError(f'Unknown dataset {dataset}')
    names = sorted([x.split('.')[0] for x in os.listdir(os.path.join(data_path, 'rgb'))])
    return category_lists(names, categories)


def result_line(status, fn, category):
    if status == VIEW_OK:
        return f'Finish: {fn}'
    if status == VIEW_TOO_FEW:
        return f'Error in {fn} {category}, num of points less than NUM_POINTS!'
    if status == VIEW_LABEL_MISMATCH:
        return f'Error in {fn} {category}, semantic and instance labels do not match!'
    return f'Error in {fn} {category}, instance id beyond the converter\'s table!'


def _stack_pinned(views, key):
    t = torch.from_numpy(np.stack([v[key] for v in views]))
    return t.pin_memory() if torch.cuda.is_available() else t


def _convert_batch(views, num_points, device, stats):
    """views of one chunk -> results in order; views of different H x W (or depth dtype) go in different batches, each batch's
    pinned staging within STAGING_BYTES"""
    res = [None] * len(views)
    groups = {}
    for i, v in enumerate(views):
        groups.setdefault((v['depth'].shape, v['depth'].dtype.str), []).append(i)
    for ids in groups.values():
        per_view = sum(views[ids[0]][k].nbytes for k in ('rgb', 'depth', 'sem', 'ins', 'npcs'))
        step = max(1, STAGING_BYTES // max(per_view, 1))
        for s in range(0, len(ids), step):
            sub = ids[s:s + step]
            vs = [views[i] for i in sub]
            t0 = time.perf_counter()
            out = convert_views(_stack_pinned(vs, 'rgb'), _stack_pinned(vs, 'depth'), _stack_pinned(vs, 'sem'),
                                _stack_pinned(vs, 'ins'), _stack_pinned(vs, 'npcs'), np.stack([v['K'] for v in vs]), num_points,
                                device=device)
            stats['gpu_s'] += time.perf_counter() - t0
            for i, r in zip(sub, out):
                res[i] = r
    return res


def convert_directory(data_path, save_path, dataset='partnet', num_points=20000, batch=16, workers=8, log_path=LOG_PATH,
                      device=None, echo=True):
    """the reference's driver (:178-236) over a directory of renders; returns timing statistics (seconds): read_s / write_s =
    summed over the reader / writer threads, gpu_s = the batches' convert_views calls, wall_s = the whole run"""
    t_start = time.perf_counter()
    groups = scan(data_path, dataset)
    if not os.path.exists(save_path):
        os.mkdir(save_path)
    jobs = [(cat, fn) for cat, fns in groups.items() for fn in fns]
    if jobs:
        for sub in ('pth', 'meta', 'gt'):
            os.makedirs(os.path.join(save_path, sub), exist_ok=True)
    stats = dict(views=len(jobs), written=0, read_s=0.0, gpu_s=0.0, write_s=0.0, statuses={})
    batch = max(1, int(batch))
    workers = max(1, min(int(workers), MAX_WORKERS))
    chunks = [jobs[i:i + batch] for i in range(0, len(jobs), batch)]

    def timed_read(fn):
        t0 = time.perf_counter()
        v = read_view(data_path, fn)
        return v, time.perf_counter() - t0

    def timed_write(fn, r):
        t0 = time.perf_counter()
        write_view(save_path, fn, r)
        return time.perf_counter() - t0

    with open(log_path, 'w') as log, ThreadPoolExecutor(workers) as readers, ThreadPoolExecutor(2) as writers:
        def log_writer(s):
            log.write(s + '\n')
            if echo:
                print(s)

        def results():  # (fn, ViewResult) in job order; the next chunk is read while this one is on the GPU
            pending = [readers.submit(timed_read, fn) for _, fn in chunks[0]] if chunks else []
            for ci, chunk in enumerate(chunks):
                views = []
                for fut in pending:
                    v, dt = fut.result()
                    views.append(v)
                    stats['read_s'] += dt
                pending = [readers.submit(timed_read, fn) for _, fn in chunks[ci + 1]] if ci + 1 < len(chunks) else []
                for (cat, fn), r in zip(chunk, _convert_batch(views, num_points, device, stats)):
                    if r.status == VIEW_OK:
                        writes.append(writers.submit(timed_write, fn, r))
                    yield fn, r

        writes = []
        it = results()
        for category, fn_list in groups.items():
            log_writer(f'Start: {category}')
            log_writer(f'{category} : {len(fn_list)}')
            for idx, fn in enumerate(fn_list):
                log_writer(f'Sampling {idx}/{len(fn_list)} {fn}')
                got, r = next(it)
                assert got == fn
                stats['statuses'][fn] = r.status
                log_writer(result_line(r.status, fn, category))
            log_writer(f'Finish: {category}')
        for w in writes:
            stats['write_s'] += w.result()
        stats['written'] = len(writes)
    stats['wall_s'] = time.perf_counter() - t_start
    return stats


def main(argv=None):
    parser = argparse.ArgumentParser(description="rendered RGB-D views -> GAPartNet training scenes (pth / meta / gt), on the GPU")
    parser.add_argument('--dataset', type=str, default='partnet', help='Specify the dataset to render')
    parser.add_argument('--data_path', type=str, default='./rendered_data', help='Specify the path to the rendered data')
    parser.add_argument('--save_path', type=str, default='./sampled_data', help='Specify the path to save the sampled data')
    parser.add_argument('--num_points', type=int, default=20000, help='Specify the number of points to sample')
    parser.add_argument('--visualize', type=bool, default=False, help='not supported (needs open3d)')
    parser.add_argument('--batch', type=int, default=16, help='views per GPU batch')
    parser.add_argument('--workers', type=int, default=8, help=f'reader threads (at most {MAX_WORKERS})')
    parser.add_argument('--log', type=str, default=LOG_PATH, help='log file (the reference writes ./log_sample.txt)')
    args = parser.parse_args(argv)
    if args.visualize:
        parser.error('--visualize needs open3d, which this converter does not use; run without it')
    stats = convert_directory(args.data_path, args.save_path, args.dataset, args.num_points, args.batch, args.workers, args.log)
    print('All finished!')
    return stats


if __name__ == '__main__':
    main()
