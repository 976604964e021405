"""Label-free inference on raw point clouds: from a cloud to parts and part boxes (reference: the deployment entry points
gapartnet/tools/visu.py:79-143 ``_inference_perception_model`` / ``inference_real`` and structure/utils.py:118-192; its CPU front
end tools/visu_utils.py:141-173 ``OBJfile2points`` / ``FindMaxDis`` / ``WorldSpaceToBallSpace``).

``prepare_clouds``   ragged raw clouds of any size, sensor NaNs included -> the network's input: valid rows, FPS down to
                     ``num_points``, ball normalisation over the sampled points (csrc/cloudprep.hip; include/gpn.h section CP);
                     ``sampler="grid"`` (here, in ``prepare_frames``, ``PartPredictor`` and ``--sampler``): the opt-in octree-cell
                     sampler instead of FPS (csrc/gridsample.hip; section GS; ``grid_sample_rows`` is its contract in numpy)
``PartPredictor``    ``model(pcs)`` -> score filter + NMS -> per-point maps and one box per part (the kernels of the test epoch's
                     rendering) -> every row of the caller's cloud through its nearest sampled point (gpn_cloud_nearest)
``PartPredictor.predict_with_masks``  parts the CALLER found (point masks with a part class each, on the raw rows): NPCS, a score
                     and a 9-DoF box per mask (``GAPartNet.forward_with_masks``; csrc/proposals.hip section MP)
``read_obj_points``  the reference's OBJ reader
``python -m gapartnet_amd.inference --ckpt X --input a.npy b.obj ... --out DIR [--num_points N] [--sampler grid] [--inference_dtype bf16]
        [--panels] [--no_flip] [--masks a.npz b.npz ...]``   (``--masks``: parallel to ``--input``, each file ``masks`` [K, N] and
        ``labels`` [K]; the output gains the ``mask_*`` arrays and the panels draw the masks' boxes)
``prepare_frames`` / ``PartPredictor.predict_frames`` / ``predict_frames_with_masks``  the same from RGB-D frames: depth, image and
                     intrinsics in (the reference's ObjIns.get_pc / get_downsampled_pc), per-pixel parts, camera-frame boxes and the
                     image with the boxes drawn out (csrc/frameprep.hip; include/gpn.h section FR)
``python -m gapartnet_amd.inference --ckpt X --depth d.npy|d.png --rgb i.png --intrinsics K.txt|K.npy [--depth_scale 1000
        --keep_mask m.png --flip --presample 4 --seed 0 --sampler grid --masks a.npz] --out DIR``   writes DIR/<name>.npz and DIR/<name>_overlay.png
        ``--isolate [--isolate_planes N --plane_tol T --isolate_select largest|center|all --z_max Z]``: raw frames - the object is
        cut out first (``isolate_objects``; csrc/isolate.hip, include/gpn.h section OB); the ``.npz`` gains ``keep``, ``planes``, ``isolate_status``
        (``--masks``: ``masks`` [K, H, W] and ``labels`` [K] per frame); frames of different sizes go in separate batches
        ``--bank bank.npy --features f0.npy ...`` next to ``--masks``: class-agnostic masks (a segmenter's) - the ``.npz`` may omit
        ``labels``; each mask's class is a 5-nearest-neighbour vote of its pooled image feature against the bank
        (misc/grounding.py; csrc/ground.hip, include/gpn.h section GR) and the output gains ``mask_label_votes``

CUDA tensors run on the HIP library; CPU tensors take the same graph in torch ops (FPS as a plain loop) - for tests and tiny
inputs, never chosen for a CUDA tensor.
"""
import argparse
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import torch

from .hip_ops import CLOUD_DEGENERATE, CLOUD_EMPTY, CLOUD_OK  # (include/gpn.h section CP; importing loads no library)
from .misc.pose_fitting_batched import estimate_pose_from_npcs_batched
from .structure.point_cloud import PointCloud

STATUS_NAMES = {CLOUD_OK: "ok", CLOUD_EMPTY: "empty", CLOUD_DEGENERATE: "degenerate"}


@dataclass
class PreparedClouds:
    points: torch.Tensor        # [sum m_s, C] f32: ball-normalised xyz + the caller's other columns, the OK clouds' samples in order
    counts: torch.Tensor        # [S] i64 (host): m_s = min(valid rows, num_points) of an OK cloud, 0 otherwise
    sample_rows: torch.Tensor   # [sum m_s] i64: the row of every sample inside its caller's cloud
    scale: torch.Tensor         # [S, 4] f64 (host): (r, cx, cy, cz) - caller's frame = normalised * r + c
    status: torch.Tensor        # [S] i64 (host): CLOUD_OK / CLOUD_EMPTY / CLOUD_DEGENERATE
    offsets: List[int]          # [S+1]: the clouds' rows in ``source``
    source: torch.Tensor        # [M, C] f32: the caller's clouds, concatenated
    table: Optional[dict] = None  # device tables gpn_cloud_nearest reads (CUDA only)
    level: Optional[torch.Tensor] = None  # [S] i64 (host), sampler "grid" only: the octree level used, -1 where a cloud was not sampled
    isolation: Optional["ObjectIsolation"] = None  # ``prepare_frames(isolate=...)`` only


# ---------------------------------------------------------------------------------------------------- torch formulation (CPU)
def _fps_loop(xyz: np.ndarray, m: int) -> np.ndarray:
    """pointnet2's furthest point sampling on one cloud as a plain loop (float32, start 0): per "thread" t of a block of
    B = largest power of two <= n (at most 1024) the first maximum over k = t, t + B, ..., then the block's tree reduction in which the
    lower thread wins a tie - the order csrc/viewprep.hip's fps_better states in closed form"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    n = xyz.shape[0]
    B = min(1 << (int(n).bit_length() - 1), 1024)
    rows = (n + B - 1) // B
    t = np.full(n, 1e10, dtype=np.float32)
    out = np.zeros(m, dtype=np.int64)
    pad = np.full(rows * B, -1.0, dtype=np.float32)
    old = 0
    for j in range(1, m):
        d = xyz - xyz[old]
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        t = np.minimum(t, dd)
        pad[:n] = t
        grid = pad.reshape(rows, B)
        first = grid.argmax(0)  # (first maximum: the lowest k of the thread)
        val, idx = grid[first, np.arange(B)], first * B + np.arange(B)
        s = B // 2
        while s >= 1:
            v1, v2, i1, i2 = val[:s], val[s:2 * s], idx[:s], idx[s:2 * s]
            idx = np.where(v2 > v1, i2, i1)
            val = np.maximum(v1, v2)
            s //= 2
        old = int(idx[0])
        out[j] = old
    return out


def _prepare_cloud_torch(cloud: torch.Tensor, m: int, sampler: str = "fps", seed: int = 0):
    """one cloud -> (status, normalised [m_s, C] f32, sample_rows [m_s] i64, scale [4] f64, the grid sampler's level or -1)"""
    C = cloud.shape[1]
    none = (torch.zeros((0, C), dtype=torch.float32), torch.zeros(0, dtype=torch.int64), torch.zeros(4, dtype=torch.float64))
    rows = torch.nonzero(torch.isfinite(cloud[:, :3]).all(1)).squeeze(1)
    n = int(rows.shape[0])
    level = -1
    if n == 0:
        return (CLOUD_EMPTY,) + none + (level,)
    if n > m and sampler == "grid":
        picked, level = grid_sample_rows(cloud[rows, :3].numpy(), m, seed)
        rows = rows[torch.from_numpy(picked)]
    elif n > m:
        rows = rows[torch.from_numpy(_fps_loop(cloud[rows, :3].numpy(), m))]
    p = cloud[rows, :3].double()
    c = (p.max(0)[0] + p.min(0)[0]) / 2
    d = p - c
    r = torch.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
    scale = torch.cat([r[None], c])
    if not bool(r > 0):
        return CLOUD_DEGENERATE, none[0], none[1], scale, level
    out = cloud[rows].clone()
    out[:, :3] = (d / r).float()
    return CLOUD_OK, out, rows, scale, level


def _nearest_torch(queries: torch.Tensor, samples: torch.Tensor, chunk: int = 4096) -> torch.Tensor:
    """[n] i64: per query the nearest sample, fp32 (dx*dx + dy*dy) + dz*dz, lowest index on ties; -1 for a non-finite query"""
    n, ms = queries.shape[0], samples.shape[0]
    nn = torch.full((n,), -1, dtype=torch.int64, device=queries.device)
    if ms == 0:
        return nn
    ar = torch.arange(ms, device=queries.device)
    for a in range(0, n, chunk):
        q = queries[a:a + chunk]
        dx, dy, dz = (q[:, None, k] - samples[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        best = torch.where(d == d.amin(1, keepdim=True), ar[None, :], ms).amin(1)
        nn[a:a + chunk] = torch.where(torch.isfinite(q).all(1), best, -1)
    return nn


# ---------------------------------------------------------------------------------------------------- front end
def _check_clouds(clouds: Sequence[torch.Tensor]):
    clouds = [torch.as_tensor(c) for c in clouds]
    if not clouds:
        raise ValueError("no clouds given")
    C, dev = clouds[0].shape[-1], clouds[0].device
    for c in clouds:
        if c.dim() != 2 or c.shape[1] != C or C < 3 or c.dtype != torch.float32 or c.device != dev:
            raise ValueError("clouds must be float32 tensors [N_i, C] with one C >= 3 on one device")
    return clouds


def _prepared_from_tables(got, m: int, offsets: List[int], source: torch.Tensor) -> PreparedClouds:
    """the device tables of ``cloud_prepare`` / ``frame_prepare`` ([S, m] slots per cloud) as a ``PreparedClouds`` over ``source``"""
    status = got["status"]
    counts = torch.where(status == CLOUD_OK, got["counts"], torch.zeros_like(got["counts"]))
    # (the live slots of the [S, m] tables, listed on the host from the counts it already holds: no second host read)
    live = torch.arange(m)[None, :] < counts[:, None]
    take = torch.nonzero(live.reshape(-1)).squeeze(1).to(source.device, non_blocking=True)
    points = got["out"].reshape(counts.shape[0] * m, -1).index_select(0, take)
    sample_rows = got["sample_rows"].reshape(-1).index_select(0, take).long()
    table = dict(sample_rows=got["sample_rows"], counts=got["counts_dev"], status=got["status_dev"])
    return PreparedClouds(points, counts, sample_rows, got["scale"], status, offsets, source, table, got.get("level"))


def _prepared_from_parts(parts, offsets: List[int], source: torch.Tensor, sampler: str) -> PreparedClouds:
    """the per-cloud results of ``_prepare_cloud_torch`` as a ``PreparedClouds`` over ``source``"""
    level = torch.tensor([p[4] for p in parts], dtype=torch.int64) if sampler == "grid" else None
    return PreparedClouds(torch.cat([p[1] for p in parts]), torch.tensor([p[1].shape[0] for p in parts], dtype=torch.int64),
                          torch.cat([p[2] for p in parts]), torch.stack([p[3] for p in parts]),
                          torch.tensor([p[0] for p in parts], dtype=torch.int64), offsets, source, None, level)


SAMPLERS = ("fps", "grid")


def _check_sampler(sampler: str) -> str:
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    return sampler


def prepare_clouds(clouds: Sequence[torch.Tensor], num_points: int = 20000, max_groups: int = 0, sampler: str = "fps",
                   seed=0) -> PreparedClouds:
    """``clouds``: [N_i, C] float32 tensors, xyz first, any N_i (0 included); rows with a non-finite coordinate are skipped.  A cloud
    with more than ``num_points`` valid rows is sampled by FPS, a smaller one keeps every valid row; centre and radius of the ball
    normalisation are those of the SAMPLED points, as in the converter the training data came from.  ``sampler`` "grid" (opt-in):
    the octree-cell sampler of include/gpn.h section GS instead of FPS - a sort and a few passes instead of ``num_points``
    sequential steps, a coarser cover (the checkpoints were trained on FPS samples); ``seed``: one uint32 per cloud, or an int s for
    s, s + 1, ...; the result's ``level`` is the octree level of every cloud."""
    clouds = _check_clouds(clouds)
    _check_sampler(sampler)
    m = int(num_points)
    if m < 1:
        raise ValueError("num_points must be positive")
    seeds = _frame_seeds(seed, len(clouds))
    offsets = [0]
    for c in clouds:
        offsets.append(offsets[-1] + int(c.shape[0]))
    source = torch.cat(clouds, 0)
    if source.is_cuda:
        from . import backend
        hip = backend.raw()
        if hip.name != "hip":
            raise RuntimeError("prepare_clouds on GPU tensors needs the HIP library as the operator backend")
        return _prepared_from_tables(hip.cloud_prepare(source, offsets, m, max_groups, sampler=sampler, seeds=seeds), m, offsets, source)
    return _prepared_from_parts([_prepare_cloud_torch(c, m, sampler, seeds[i]) for i, c in enumerate(clouds)], offsets, source, sampler)


def nearest_samples(prep: PreparedClouds) -> torch.Tensor:
    """[M] i64: for every row of the caller's clouds the position (inside its cloud's samples) of the nearest sampled point, in the
    caller's coordinates; -1 for invalid rows and for clouds that are not OK"""
    if prep.source.is_cuda:
        from . import backend
        t = prep.table
        return backend.raw().cloud_nearest(prep.source, prep.offsets, t["sample_rows"], t["counts"], t["status"]).long()
    out, first = [], 0
    for s, ms in enumerate(prep.counts.tolist()):
        cloud = prep.source[prep.offsets[s]:prep.offsets[s + 1], :3]
        out.append(_nearest_torch(cloud, cloud[prep.sample_rows[first:first + ms]]))
        first += ms
    return torch.cat(out)


# ---------------------------------------------------------------------------------------------------- RGB-D frames
def frame_hash(seed: int, pixel: np.ndarray, hash_bits: int = 32) -> np.ndarray:
    """the presample's hash (include/gpn.h section FR), uint32: mix(mix(pixel + seed * 0x9E3779B9) ^ seed) >> (32 - hash_bits)"""
    def mix(x):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846ca68b)
        return x ^ (x >> np.uint32(16))

    seed = np.uint32(int(seed) & 0xffffffff)
    with np.errstate(over="ignore"):
        h = mix(mix(np.asarray(pixel).astype(np.uint32) + seed * np.uint32(0x9E3779B9)) ^ seed)
    return h >> np.uint32(32 - int(hash_bits))


def select_pixels(valid_pixels: np.ndarray, seed: int, cap: int, hash_bits: int = 32) -> np.ndarray:
    """the seeded presample on the host: of the valid pixels (linear indices) the ``cap`` with the smallest key
    (hash << 32) | pixel, ascending; all of them when there are at most ``cap`` or ``cap`` is 0"""
    pix = np.sort(np.asarray(valid_pixels, dtype=np.int64))
    if cap <= 0 or pix.shape[0] <= cap:
        return pix
    key = (frame_hash(seed, pix, hash_bits).astype(np.uint64) << np.uint64(32)) | pix.astype(np.uint64)
    return np.sort(pix[np.argsort(key, kind="stable")[:cap]])


def grid_sample_rows(xyz: np.ndarray, m: int, seed: int = 0, hash_bits: int = 32):
    """the octree-cell sampler on the host (include/gpn.h section GS): of the n rows of ``xyz`` [n, 3] f32 (all finite) -> (the m
    chosen rows ascending i64, the octree level L*); n <= m: (every row, -1)"""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)[:, :3])
    n, m = xyz.shape[0], int(m)
    if n <= m:
        return np.arange(n, dtype=np.int64), -1
    q = np.zeros((n, 3), dtype=np.uint32)
    with np.errstate(all="ignore"):
        lo, hi = xyz.min(0), xyz.max(0)
        e = np.float32((hi - lo).max())
        if e > 0 and np.isfinite(e):
            x = (xyz - lo) * np.float32(1024.0 / np.float64(e))
            q = np.where(x < np.float32(1023.0), x, np.float32(1023.0)).astype(np.uint32)  # (a NaN, 0 * inf, takes 1023)
    code = np.zeros(n, dtype=np.uint32)
    for i in range(10):
        for a in range(3):
            code |= ((q[:, a] >> np.uint32(i)) & np.uint32(1)) << np.uint32(3 * i + a)
    order = np.argsort(code, kind="stable")  # by (code, row): the order of the keys code << 32 | row
    sc = code[order].astype(np.int64)
    # the first level at which a sorted row opens a new cell: cells of level L differ when a bit >= 30 - 3 L of the codes differs
    d = sc[1:] ^ sc[:-1]
    top = np.floor(np.log2(np.maximum(d, 1))).astype(np.int64)
    first = np.concatenate([[0], np.where(d == 0, 11, 10 - top // 3)])
    cells = np.cumsum(np.bincount(first, minlength=12))[:11]  # C_0 .. C_10
    L = int(np.nonzero(cells <= m)[0].max())
    r = m - int(cells[L])
    chosen = [order[first <= L]]  # stage A: a cell's first row in key order
    if r > 0:
        if L < 10:  # the level-(L+1) cells without a stage-A point, by (hash(cell), cell); each gives its first row
            pos = np.nonzero(first == L + 1)[0]
            item = sc[pos] >> (30 - 3 * (L + 1))
        else:       # the rows stage A left, by (hash(row), row)
            pos = np.nonzero(first == 11)[0]
            item = order[pos].astype(np.int64)
        key = (frame_hash(seed, item, hash_bits).astype(np.uint64) << np.uint64(32)) | item.astype(np.uint64)
        chosen.append(order[pos[np.argsort(key, kind="stable")[:r]]])
    return np.sort(np.concatenate(chosen)).astype(np.int64), L


def _frame_seeds(seed, V: int) -> List[int]:
    """one uint32 per frame: a sequence as given, an int s as s, s + 1, ... (mod 2^32)"""
    if isinstance(seed, (int, np.integer)):
        return [(int(seed) + v) & 0xffffffff for v in range(V)]
    seeds = [int(s) & 0xffffffff for s in (seed.tolist() if hasattr(seed, "tolist") else seed)]
    if len(seeds) != V:
        raise ValueError(f"{V} frames need {V} seeds, got {len(seeds)}")
    return seeds


def _backproject_numpy(depth, rgb, K, keep, depth_scale, flip):
    """section FR's back-projection on host arrays -> (rows [V*H*W, 6] f32, valid [V, H*W] bool)"""
    V, H, W = depth.shape
    with np.errstate(all="ignore"):
        z = depth.astype(np.float64) / np.float64(depth_scale)
        valid = np.isfinite(z) & (z > 0)
        if keep is not None:
            valid &= np.asarray(keep).reshape(V, H, W) != 0
        u = np.arange(W, dtype=np.float64)[None, None, :]
        v = np.arange(H, dtype=np.float64)[None, :, None]
        Kd = np.asarray(K, dtype=np.float64).reshape(V, 3, 3)
        x = ((u - Kd[:, 0, 2, None, None]) * z) / Kd[:, 0, 0, None, None]
        y = ((v - Kd[:, 1, 2, None, None]) * z) / Kd[:, 1, 1, None, None]
        xyz = np.stack([x, y, z], -1).astype(np.float32)
    valid &= np.isfinite(xyz).all(-1)
    if flip:
        xyz[..., 1:] = -xyz[..., 1:]
    xyz[~valid] = np.nan
    col = (np.asarray(rgb).reshape(V, H, W, 3).astype(np.float64) / 255.0).astype(np.float32)
    return np.concatenate([xyz, col], -1).reshape(V * H * W, 6), valid.reshape(V, H * W)


def _check_frames(depth, rgb, K, keep):
    """``rgb`` None: frames without colours (``backproject_frames`` takes them as black)"""
    depth, rgb = torch.as_tensor(depth), None if rgb is None else torch.as_tensor(rgb)
    if depth.dim() == 2:
        depth, rgb = depth[None], None if rgb is None else rgb[None]
    if depth.dim() != 3 or depth.dtype not in (torch.float32, torch.float64, torch.uint16, torch.int16):
        raise ValueError("depth must be [V, H, W] (or [H, W]) float32, float64 or uint16")
    V, H, W = (int(v) for v in depth.shape)
    if rgb is not None and (tuple(rgb.shape) != (V, H, W, 3) or rgb.dtype != torch.uint8):
        raise ValueError(f"rgb must be uint8 [{V}, {H}, {W}, 3]")
    K = torch.as_tensor(K).detach().cpu().double()  # (host data: the overlay's camera is read from it)
    if K.numel() == 9:
        K = K.reshape(1, 3, 3).expand(V, 3, 3)
    K = K.reshape(V, 3, 3).contiguous()
    if keep is not None:
        keep = torch.as_tensor(keep)
        keep = keep[None] if keep.dim() == 2 else keep
        if tuple(keep.shape) != (V, H, W):
            raise ValueError(f"keep must be [{V}, {H}, {W}]")
    return depth, rgb, K, keep


def backproject_frames(depth, rgb, K, keep, depth_scale, flip):
    """section FR's back-projection of frames that passed ``_check_frames``, on whichever device they live on; ``rgb`` None: black.
    -> (rows [V*H*W, 6] f32, valid [V,H,W] u8, counts [V] = the valid pixels of every frame) on the frames' device.  No host read."""
    V, H, W = (int(v) for v in depth.shape)
    dev = depth.device
    if rgb is None:
        rgb = torch.zeros((V, H, W, 3), dtype=torch.uint8, device=dev)
    if depth.is_cuda:
        from . import backend
        hip = backend.raw()
        if hip.name != "hip":
            raise RuntimeError("backproject_frames on GPU tensors needs the HIP library as the operator backend")
        return hip.frame_backproject(depth, rgb, K.to(dev, non_blocking=True), keep, depth_scale, flip)
    d = depth.numpy()
    rows, valid = _backproject_numpy(d.view(np.uint16) if d.dtype == np.int16 else d, rgb.numpy(), K.numpy(),
                                     None if keep is None else keep.numpy(), depth_scale, flip)
    valid = torch.from_numpy(valid.reshape(V, H, W).astype(np.uint8))
    return torch.from_numpy(rows), valid, valid.sum((1, 2))


# ---------------------------------------------------------------------------------------------------- object isolation
ISOLATE_OK, ISOLATE_NO_PLANE, ISOLATE_EMPTY = 0, 1, 2  # (include/gpn.h section OB)
ISOLATE_STATUS_NAMES = {ISOLATE_OK: "ok", ISOLATE_NO_PLANE: "no plane", ISOLATE_EMPTY: "empty"}
ISOLATE_SELECT = ("largest", "center", "all")
_ISOLATE_MAX_PLANES, _ISOLATE_MAX_HYP, _ISOLATE_TRIES = 4, 1024, 8


@dataclass
class IsolateConfig:
    """the parameters of include/gpn.h section OB; lengths in the units of the rows (depth / depth_scale)"""
    max_planes: int = 1                 # RANSAC rounds: 1 (the table) .. 4
    n_hyp: int = 256                    # plane hypotheses per round, 1 .. 1024
    tol: float = 0.005                  # a pixel within tol of a plane is on it
    min_plane_fraction: float = 0.1     # a plane is accepted when it holds this share of the round's candidates
    z_min: float = 0.0                  # candidates: z_min <= |z| <= z_max
    z_max: float = float("inf")
    jump_abs: float = 0.01              # neighbours are linked when |za - zb| <= jump_abs + jump_rel * min(za, zb)
    jump_rel: float = 0.01
    select: str = "largest"             # "largest" | "center" | "all"
    min_pixels: int = 6                 # components below this count for nothing
    anchor: Optional[Sequence] = None   # "center": [V,2] or [2] pixels (column, line); default rint(K02), rint(K12)

    def __post_init__(self):
        if not 1 <= int(self.max_planes) <= _ISOLATE_MAX_PLANES:
            raise ValueError(f"max_planes must be 1 .. {_ISOLATE_MAX_PLANES}, got {self.max_planes}")
        if not 1 <= int(self.n_hyp) <= _ISOLATE_MAX_HYP:
            raise ValueError(f"n_hyp must be 1 .. {_ISOLATE_MAX_HYP}, got {self.n_hyp}")
        for name in ("tol", "jump_abs", "jump_rel"):
            if not (0.0 <= float(getattr(self, name)) < float("inf")):
                raise ValueError(f"{name} must be finite and non-negative, got {getattr(self, name)}")
        if not 0.0 <= float(self.min_plane_fraction) <= 1.0:
            raise ValueError(f"min_plane_fraction must be in [0, 1], got {self.min_plane_fraction}")
        if not (0.0 <= float(self.z_min) <= float(self.z_max)):
            raise ValueError(f"0 <= z_min <= z_max is required, got {self.z_min}, {self.z_max}")
        if self.select not in ISOLATE_SELECT:
            raise ValueError(f"select must be one of {ISOLATE_SELECT}, got {self.select!r}")
        if int(self.min_pixels) < 1:
            raise ValueError(f"min_pixels must be positive, got {self.min_pixels}")
        if self.anchor is not None and np.asarray(self.anchor).size % 2:
            raise ValueError("anchor must be [V, 2] or [2] pixels (column, line)")


@dataclass
class ObjectIsolation:
    """``isolate_objects``: everything on the input's device"""
    keep: torch.Tensor            # [V,H,W] u8: the object's pixels
    labels: torch.Tensor          # [V,H,W] i32: the smallest pixel index of the pixel's component, -1 off the candidates
    sizes: torch.Tensor           # [V,H*W] i32: a component's pixels, at its root pixel
    planes: torch.Tensor          # [V,max_planes,4] f64: (nx, ny, nz, d), d > 0; NaN for a round that accepted none
    plane_inliers: torch.Tensor   # [V,max_planes] i32
    n_planes: torch.Tensor        # [V] i32
    chosen: torch.Tensor          # [V] i32: the chosen component's root, -1 when none
    status: torch.Tensor          # [V] i32: ISOLATE_OK / ISOLATE_NO_PLANE / ISOLATE_EMPTY


def _plane_dist(pl, x, y, z):
    return ((pl[..., 0:1] * x + pl[..., 1:2] * y) + pl[..., 2:3] * z) + pl[..., 3:4]


def _isolate_frame_numpy(xyz, valid, H, W, seed, cfg: IsolateConfig, anchor):
    """section OB on one frame's rows (xyz [HW,3] f32, valid [HW] bool) in numpy / scipy, float64 in the contract's order"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    HW, nh, tol = H * W, int(cfg.n_hyp), float(cfg.tol)
    P = xyz.astype(np.float64)
    with np.errstate(invalid="ignore"):
        absz = np.abs(P[:, 2])
        cand = valid & (absz >= cfg.z_min) & (absz <= cfg.z_max)
    pix = np.nonzero(valid)[0]
    planes = np.full((cfg.max_planes, 4), np.nan)
    inliers = np.zeros(cfg.max_planes, dtype=np.int32)
    for r in range(int(cfg.max_planes)):
        # stage 1: the triples, with the redraw of pixels that are no candidates any more
        hyp = np.full((nh, 4), np.nan)
        p0_pix = np.full(nh, -1, dtype=np.int64)
        if pix.shape[0] >= 3:
            counter = 3 * nh * r + np.arange(3 * nh, dtype=np.int64)
            rank = np.full(3 * nh, -1, dtype=np.int64)
            for t in range(_ISOLATE_TRIES):
                todo = rank < 0
                if not todo.any():
                    break
                got = frame_hash(seed, counter[todo] + t * 3 * nh * _ISOLATE_MAX_PLANES).astype(np.int64) % pix.shape[0]
                rank[todo] = np.where(cand[pix[got]], got, -1)
            rk = rank.reshape(nh, 3)
            ok = (rk >= 0).all(1) & (rk[:, 0] != rk[:, 1]) & (rk[:, 0] != rk[:, 2]) & (rk[:, 1] != rk[:, 2])
            tri = P[pix[np.maximum(rk, 0)]]  # [nh, 3 points, 3]
            e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
            m = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            sq = lambda a: (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]  # noqa: E731
            with np.errstate(all="ignore"):
                mm = sq(m)
                ok &= mm > 1e-12 * (sq(e1) * sq(e2))
                n = m / np.sqrt(mm)[:, None]
                d = -((n[:, 0] * tri[:, 0, 0] + n[:, 1] * tri[:, 0, 1]) + n[:, 2] * tri[:, 0, 2])
            neg = d < 0
            n, d = np.where(neg[:, None], -n, n), np.where(neg, -d, d)
            ok &= d > 0
            hyp[ok] = np.concatenate([n, d[:, None]], 1)[ok]
            p0_pix[ok] = pix[rk[ok, 0]]
        # stage 2 and the winner
        C = P[cand]
        counts = np.zeros(nh, dtype=np.int64)
        with np.errstate(invalid="ignore"):
            for k0 in range(0, nh, 64):
                h = hyp[k0:k0 + 64]
                counts[k0:k0 + 64] = (np.abs(_plane_dist(h, C[None, :, 0], C[None, :, 1], C[None, :, 2])) <= tol).sum(1)
        win = int(np.argmax(counts)) if counts.max(initial=0) > 0 else -1  # (argmax: the lowest k of the largest count)
        # stage 3: refit and accept
        plane, n_in = None, 0
        if win >= 0:
            with np.errstate(invalid="ignore"):
                inl = cand & (np.abs(_plane_dist(hyp[win], P[:, 0], P[:, 1], P[:, 2])) <= tol)
            cnt = int(inl.sum())
            if cnt >= 3:
                p0 = P[p0_pix[win]]
                q = P[inl] - p0
                s = q.sum(0)
                mean = p0 + s / np.float64(cnt)
                nrm = np.linalg.eigh(q.T @ q - np.outer(s, s) / np.float64(cnt))[1][:, 0]
                nrm = nrm / np.sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2])
                d = -((nrm[0] * mean[0] + nrm[1] * mean[1]) + nrm[2] * mean[2])
                if d < 0:
                    nrm, d = -nrm, -d
                if d > 0:
                    fit = np.array([nrm[0], nrm[1], nrm[2], d])
                    with np.errstate(invalid="ignore"):
                        n_in = int((cand & (np.abs(_plane_dist(fit, P[:, 0], P[:, 1], P[:, 2])) <= tol)).sum())
                    if n_in >= 3 and float(n_in) >= float(cfg.min_plane_fraction) * float(cand.sum()):
                        plane = fit
        if plane is not None:  # stage 4
            planes[r], inliers[r] = plane, n_in
            with np.errstate(invalid="ignore"):
                cand = cand & (_plane_dist(plane, P[:, 0], P[:, 1], P[:, 2]) > tol)
    n_planes = int((planes[:, 3] > 0).sum())
    # stage 5
    with np.errstate(invalid="ignore"):
        z, c2 = absz.reshape(H, W), cand.reshape(H, W)
        lr = c2[:, :-1] & c2[:, 1:] & (np.abs(z[:, :-1] - z[:, 1:]) <= cfg.jump_abs + cfg.jump_rel * np.minimum(z[:, :-1], z[:, 1:]))
        ud = c2[:-1] & c2[1:] & (np.abs(z[:-1] - z[1:]) <= cfg.jump_abs + cfg.jump_rel * np.minimum(z[:-1], z[1:]))
    idx = np.arange(HW).reshape(H, W)
    a, b = np.concatenate([idx[:, :-1][lr], idx[:-1][ud]]), np.concatenate([idx[:, 1:][lr], idx[1:][ud]])
    _, comp = connected_components(csr_matrix((np.ones(a.shape[0], dtype=np.int8), (a, b)), shape=(HW, HW)), directed=False)
    order = np.argsort(comp, kind="stable")                      # a component's pixels ascending: its first is the label
    first = np.r_[True, comp[order][1:] != comp[order][:-1]]
    root_of_comp = np.zeros(comp.max() + 1, dtype=np.int64)
    root_of_comp[comp[order][first]] = order[first]
    labels = np.where(cand, root_of_comp[comp], -1).astype(np.int32)
    sizes = np.bincount(labels[cand], minlength=HW).astype(np.int32)
    # stage 6
    big = sizes >= int(cfg.min_pixels)
    chosen = -1
    if big.any():
        if cfg.select == "center":
            ax, ay = (min(max(int(v), -16384), 32767) for v in anchor)
            p = np.nonzero(cand & big[np.maximum(labels, 0)])[0]
            key = (((p % W - ax) ** 2 + (p // W - ay) ** 2).astype(np.uint64) << np.uint64(32)) | p.astype(np.uint64)
            chosen = int(labels[p[np.argmin(key)]])
        else:
            roots = np.nonzero(big)[0]
            key = (sizes[roots].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - roots.astype(np.uint64))
            chosen = int(roots[np.argmax(key)])
    if chosen < 0:
        keep, status = np.zeros(HW, dtype=np.uint8), ISOLATE_EMPTY
    else:
        keep = ((cand & big[np.maximum(labels, 0)]) if cfg.select == "all" else labels == chosen).astype(np.uint8)
        status = ISOLATE_OK if n_planes > 0 else ISOLATE_NO_PLANE
    return keep, labels, sizes, planes, inliers, n_planes, chosen, status


def _isolate_anchor(cfg: IsolateConfig, K: torch.Tensor, V: int) -> np.ndarray:
    """[V,2] i32 (column, line): the caller's anchor, or the principal point rounded half to even"""
    if cfg.anchor is None:
        Kn = K.numpy()
        a = np.stack([np.rint(Kn[:, 0, 2]), np.rint(Kn[:, 1, 2])], 1)
    else:
        a = np.rint(np.asarray(torch.as_tensor(cfg.anchor).cpu() if torch.is_tensor(cfg.anchor) else cfg.anchor, dtype=np.float64))
        a = np.broadcast_to(a.reshape(-1, 2), (V, 2)) if a.size == 2 else a.reshape(-1, 2)
        if a.shape[0] != V:
            raise ValueError(f"{V} frames need {V} anchors, got {a.shape[0]}")
    return np.clip(a, -16384, 32767).astype(np.int32)


def _isolate_checked(depth, K, keep, seeds, depth_scale, flip, cfg: IsolateConfig) -> ObjectIsolation:
    V, H, W = (int(v) for v in depth.shape)
    anchor = _isolate_anchor(cfg, K, V)
    if depth.is_cuda:
        from . import backend
        hip = backend.raw()
        if hip.name != "hip":
            raise RuntimeError("isolate_objects on GPU tensors needs the HIP library as the operator backend")
        dev = depth.device
        rows, valid, valid_counts = backproject_frames(depth, None, K, keep, depth_scale, flip)  # (the rows' colours are not read here)
        got = hip.frame_isolate(rows, valid, valid_counts, seeds, cfg.max_planes, cfg.n_hyp, cfg.tol, cfg.min_plane_fraction, cfg.z_min,
                                cfg.z_max, cfg.jump_abs, cfg.jump_rel, cfg.select, cfg.min_pixels,
                                torch.from_numpy(anchor).to(dev, non_blocking=True) if cfg.select == "center" else None)
        return ObjectIsolation(*(got[f] for f in ("keep", "labels", "sizes", "planes", "plane_inliers", "n_planes", "chosen", "status")))
    rows, valid, _ = backproject_frames(depth, None, K, keep, depth_scale, flip)
    rows, valid = rows.numpy(), valid.numpy().reshape(V, H * W) != 0
    per = [_isolate_frame_numpy(rows[v * H * W:(v + 1) * H * W, :3], valid[v], H, W, seeds[v], cfg, anchor[v]) for v in range(V)]
    col = lambda i, dt: torch.from_numpy(np.stack([np.asarray(p[i]) for p in per]).astype(dt)) if V else torch.zeros((0,), dtype=torch.int32)  # noqa: E731
    return ObjectIsolation(keep=col(0, np.uint8).reshape(V, H, W), labels=col(1, np.int32).reshape(V, H, W), sizes=col(2, np.int32).reshape(V, H * W),
                           planes=col(3, np.float64).reshape(V, cfg.max_planes, 4), plane_inliers=col(4, np.int32).reshape(V, cfg.max_planes),
                           n_planes=col(5, np.int32).reshape(V), chosen=col(6, np.int32).reshape(V), status=col(7, np.int32).reshape(V))


def isolate_objects(depth, K, depth_scale: float = 1.0, flip: bool = False, keep=None, seed=0,
                    config: Optional[IsolateConfig] = None) -> ObjectIsolation:
    """The object of every raw RGB-D frame without a segmenter (include/gpn.h section OB; csrc/isolate.hip): the dominant planes by
    seeded RANSAC (the table, a wall), what lies on or behind them dropped, the connected components of the rest under a
    depth-continuity rule, and the object's component chosen (``IsolateConfig.select``).  ``depth`` [V,H,W] (or [H,W]), ``K``, ``keep``,
    ``depth_scale``, ``flip``, ``seed`` as in ``prepare_frames``.  The result's ``keep`` is what ``prepare_frames(keep=)`` takes; no
    host read is made.  CPU tensors take the same contract in numpy / scipy."""
    cfg = IsolateConfig() if config is None else config
    depth, _, K, keep = _check_frames(depth, None, K, keep)
    return _isolate_checked(depth, K, keep, _frame_seeds(seed, int(depth.shape[0])), depth_scale, flip, cfg)


def prepare_frames(depth, rgb, K, num_points: int = 20000, presample: int = 4, seed=0, keep=None, depth_scale: float = 1.0,
                   flip: bool = False, hash_bits: int = 32, max_groups: int = 0, sampler: str = "fps",
                   isolate: Optional[IsolateConfig] = None) -> PreparedClouds:
    """V RGB-D frames of one size -> the network's input (include/gpn.h section FR; the reference's ObjIns.get_pc /
    get_downsampled_pc, structure/gapartnet.py:541-627).  ``depth`` [V,H,W] f32 / f64 / u16 (divided by ``depth_scale``), ``rgb``
    [V,H,W,3] u8, ``K`` [V,3,3] or [3,3] (host data), ``keep`` [V,H,W] or None.  Every pixel becomes a row [x y z r g b] (NaN xyz
    where there is no depth); a frame with more than ``presample * num_points`` valid pixels is cut to that many by the seeded
    hash rule (``seed``: one uint32 per frame, or an int s for s, s + 1, ...; ``presample`` 0: no cut), then FPS and the ball
    normalisation of ``prepare_clouds``.  The result's ``source`` is the [V*H*W, 6] rows, its ``sample_rows`` are pixel indices.
    ``sampler`` "grid": ``prepare_clouds``' octree-cell sampler behind the (unchanged) presample, with the frames' seeds.
    ``isolate``: an ``IsolateConfig`` - the frames are back-projected and the object isolated first (``isolate_objects`` with the same
    ``keep`` and seeds); its mask is the ``keep`` of everything behind, and the result's ``isolation`` holds the
    ``ObjectIsolation``.  None: nothing changes."""
    depth, rgb, K, keep = _check_frames(depth, rgb, K, keep)
    return _prepare_checked_frames(depth, rgb, K, keep, num_points, presample, seed, depth_scale, flip, hash_bits, max_groups, sampler,
                                   isolate)


def _prepare_checked_frames(depth, rgb, K, keep, num_points, presample, seed, depth_scale, flip, hash_bits=32, max_groups=0,
                            sampler="fps", isolate=None):
    """``prepare_frames`` behind its argument check (``_check_frames``), which the predictor's frame entries run themselves"""
    _check_sampler(sampler)
    if isolate is not None:
        # (the isolation's candidates are valid pixels of a back-projection under the caller's keep: its mask lies inside it)
        iso = _isolate_checked(depth, K, keep, _frame_seeds(seed, int(depth.shape[0])), depth_scale, flip, isolate)
        prep = _prepare_checked_frames(depth, rgb, K, iso.keep, num_points, presample, seed, depth_scale, flip, hash_bits, max_groups,
                                       sampler)
        prep.isolation = iso
        return prep
    V, H, W = (int(v) for v in depth.shape)
    m, cap = int(num_points), int(presample) * int(num_points)
    if m < 1 or cap < 0:
        raise ValueError("num_points must be positive and presample non-negative")
    seeds = _frame_seeds(seed, V)
    offsets = [v * H * W for v in range(V + 1)]
    if depth.is_cuda:
        from . import backend
        hip = backend.raw()
        if hip.name != "hip":
            raise RuntimeError("prepare_frames on GPU tensors needs the HIP library as the operator backend")
        got = hip.frame_prepare(depth, rgb, K.to(depth.device, non_blocking=True), m, cap, seeds, keep=keep, depth_scale=depth_scale, flip=flip,
                                hash_bits=hash_bits, max_groups=max_groups, sampler=sampler)
        return _prepared_from_tables(got, m, offsets, got["rows"])
    rows, valid, _ = backproject_frames(depth, rgb, K, keep, depth_scale, flip)
    valid = valid.numpy().reshape(V, H * W)
    parts = []
    for v in range(V):
        frame = rows[offsets[v]:offsets[v + 1]].numpy().copy()
        drop = np.ones(H * W, dtype=bool)
        drop[select_pixels(np.nonzero(valid[v])[0], seeds[v], cap, hash_bits)] = False
        frame[drop, :3] = np.nan
        parts.append(_prepare_cloud_torch(torch.from_numpy(frame), m, sampler, seeds[v]))
    return _prepared_from_parts(parts, offsets, rows, sampler)


# the box edges of draw_bbox (structure/utils.py:73-89; include/gpn.h section VS): (corner a, corner b, colour as written, thickness)
_BOX_DRAWS = [(a, b, (255, 0, 255), 2) for a, b in ((0, 1), (0, 2), (0, 3), (1, 4), (1, 5), (2, 6), (6, 3), (4, 7), (5, 7), (3, 5),
                                                    (2, 4), (6, 7))] + \
             [(0, 1, (255, 0, 0), 3), (0, 3, (0, 0, 255), 3), (0, 2, (0, 255, 0), 3)]


def _draw_line_numpy(img, a, b, colour, t):
    """the line rule of include/gpn.h section VS on a host image (what gpn_boxes_draw does on the device)"""
    H, W = img.shape[:2]
    pts = np.array([a[0], a[1], b[0], b[1]], dtype=np.float64)
    if not np.isfinite(pts).all() or not all(-4 * W <= x < 5 * W for x in pts[0::2]) or not all(-4 * H <= y < 5 * H for y in pts[1::2]):
        return
    x, y, x1, y1 = (int(p) for p in pts)
    dx, dy = abs(x1 - x), -abs(y1 - y)
    sx, sy = (1 if x < x1 else -1), (1 if y < y1 else -1)
    err = dx + dy
    while True:
        tx, ty = x - t // 2, y - t // 2
        img[max(ty, 0):max(min(ty + t, H), 0), max(tx, 0):max(min(tx + t, W), 0)] = colour
        if x == x1 and y == y1:
            return
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy


def project_corners(bbox: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """[Q,8,2] f64 (u, v) of box corners [Q,8,3] in the camera frame: rint(x fx / z + cx), rint(y fy / z + cy), half to even
    (structure/utils.py:70-71; the projection rule of section VS); possibly non-finite"""
    K = K.to(bbox.device, non_blocking=True)
    b = bbox.double()
    u = torch.round(b[..., 0] * K[0, 0] / b[..., 2] + K[0, 2])
    v = torch.round(b[..., 1] * K[1, 1] / b[..., 2] + K[1, 2])
    return torch.stack([u, v], -1)


def draw_overlays(rgb: torch.Tensor, boxes: Sequence[torch.Tensor], K: torch.Tensor) -> torch.Tensor:
    """``rgb`` [V,H,W,3] u8 with every frame's boxes (``boxes[v]`` [Q_v,8,3] f64, camera frame) drawn into it by draw_bbox's
    rule: gpn_boxes_draw with one tile at the origin, edge 0, trans (1, 0, 0, 0) - one launch per distinct K; host loops for CPU"""
    V, H, W, _ = rgb.shape
    canvas = rgb.clone().contiguous()
    if not rgb.is_cuda:
        img = canvas.numpy()
        for v in range(V):
            for corners in project_corners(boxes[v], K[v]).numpy():
                for a, b, colour, t in _BOX_DRAWS:
                    _draw_line_numpy(img[v], corners[a], corners[b], colour, t)
        return canvas
    from . import backend
    hip = backend.raw()
    groups = {}
    for v in range(V):
        groups.setdefault(tuple(K[v].reshape(-1).tolist()), []).append(v)
    for cam, frames in groups.items():
        # (a group that is not a run of frames draws into a copy of its frames)
        run = frames == list(range(frames[0], frames[-1] + 1))
        which = None if run else torch.tensor(frames).to(rgb.device, non_blocking=True)
        sub = canvas[frames[0]:frames[-1] + 1] if run else canvas.index_select(0, which)
        bb = torch.cat([boxes[v].double().reshape(-1, 8, 3) for v in frames])
        scene = torch.cat([torch.full((boxes[v].shape[0],), k, dtype=torch.int32) for k, v in enumerate(frames)]).to(rgb.device, non_blocking=True)
        trans = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * len(frames), dtype=torch.float64).to(rgb.device, non_blocking=True)
        if bb.shape[0]:
            hip.boxes_draw(bb.contiguous(), scene, trans, H, W, cam[0], cam[4], cam[2], cam[5], [(0, 0)], sub, 0)
        if not run:
            canvas.index_copy_(0, which, sub)
    return canvas


@dataclass
class FramePrediction:
    """one frame of ``PartPredictor.predict_frames`` (``masks``: the per-mask fields of ``predict_frames_with_masks``, else None)"""
    status: int                     # CLOUD_OK / CLOUD_EMPTY / CLOUD_DEGENERATE
    scale: torch.Tensor             # [4] f64: (r, cx, cy, cz) of the ball normalisation
    sem: torch.Tensor               # [H,W] i64: part class of every pixel (0 = no part), -1 where there is no depth
    instance: torch.Tensor          # [H,W] i64: position (in proposal_scores) of the pixel's part, -1 where none
    npcs: torch.Tensor              # [H,W,3] f32
    proposal_scores: torch.Tensor   # [P] f32
    proposal_classes: torch.Tensor  # [P] i64
    bbox: torch.Tensor              # [Q,8,3] f64 in the CAMERA frame (un-flipped when the rows were flipped); with masks: one per
                                    # mask, NaN where the mask has no valid box
    box_proposal: torch.Tensor      # [Q] i64
    corners_px: torch.Tensor        # [Q,8,2] f64: the corners' pixels (u, v)
    overlay: torch.Tensor           # [H,W,3] u8: the frame's RGB with every box drawn (draw_bbox, structure/utils.py:55-90)
    sample_rows: torch.Tensor       # [m] i64: the sampled pixels (linear indices)
    masks: Optional["MaskPrediction"] = None
    keep: Optional[torch.Tensor] = None            # with ``isolate``: [H,W] u8, the object's pixels (include/gpn.h section OB)
    planes: Optional[torch.Tensor] = None          # with ``isolate``: [max_planes,4] f64 (nx, ny, nz, d), NaN where none was accepted
    isolate_status: Optional[int] = None           # with ``isolate``: ISOLATE_OK / ISOLATE_NO_PLANE / ISOLATE_EMPTY

    def to_numpy(self) -> dict:
        out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in self.__dict__.items()
               if k != "masks" and not (k in ("keep", "planes", "isolate_status") and v is None)}
        if self.masks is not None:
            out.update({"mask_" + f: v for f, v in self.masks.to_numpy().items() if f in MASK_FIELDS or f == "label_votes"})
        return out


# ---------------------------------------------------------------------------------------------------- predictions
@dataclass
class PartPrediction:
    status: int                     # CLOUD_OK / CLOUD_EMPTY / CLOUD_DEGENERATE; everything below is empty / -1 unless OK
    scale: torch.Tensor             # [4] f64: (r, cx, cy, cz)
    sem: torch.Tensor               # [N] i64: part class of every row (0 = no part), -1 on invalid rows
    instance: torch.Tensor          # [N] i64: position (in proposal_scores) of the kept proposal the row belongs to, -1 where none
    npcs: torch.Tensor              # [N, 3] f32 (zero where no proposal)
    proposal_scores: torch.Tensor   # [P] f32
    proposal_classes: torch.Tensor  # [P] i64
    bbox: torch.Tensor              # [Q, 8, 3] f64 in the caller's frame
    box_proposal: torch.Tensor      # [Q] i64: the proposal of every box
    # the network's own view of the cloud (what the panels show)
    sample_rows: torch.Tensor       # [m] i64
    sampled_points: torch.Tensor    # [m, C] f32, normalised frame
    sampled_sem: torch.Tensor       # [m] i64
    sampled_instance: torch.Tensor  # [m] i64
    sampled_npcs: torch.Tensor      # [m, 3] f32
    bbox_normalised: torch.Tensor   # [Q, 8, 3] f64

    def to_numpy(self) -> dict:
        return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in self.__dict__.items()}


@dataclass
class MaskPrediction:
    """one cloud of ``PartPredictor.predict_with_masks``: per mask of the caller, in the caller's order (K of them)"""
    status: int                     # CLOUD_OK / CLOUD_EMPTY / CLOUD_DEGENERATE; a cloud that is not OK has every mask dropped
    cloud_scale: torch.Tensor       # [4] f64: (r, cx, cy, cz) of the ball normalisation
    sem: torch.Tensor               # [N] i64: the network's own part class of every row, -1 on invalid rows (as ``predict``)
    kept: torch.Tensor              # [K] bool: the mask had at least ``min_points`` SAMPLED members
    n_points: torch.Tensor          # [K] i64: sampled members of a kept mask, 0 for a dropped one
    label: torch.Tensor             # [K] i64: the caller's part class
    score: torch.Tensor             # [K] f32: sigmoid of the score head at the mask's class; NaN where dropped
    valid: torch.Tensor             # [K] bool: a box was fitted (kept, at least 5 points, the fit found a pose)
    scale: torch.Tensor             # [K] f64: the similarity NPCS - 0.5 -> the caller's frame (these four); NaN where not valid
    rotation: torch.Tensor          # [K, 3, 3] f64
    translation: torch.Tensor       # [K, 3] f64
    transform: torch.Tensor         # [K, 4, 4] f64
    bbox: torch.Tensor              # [K, 8, 3] f64 in the caller's frame; NaN where not valid
    bbox_normalised: torch.Tensor   # [K, 8, 3] f64 in the network's (ball) frame
    member_offsets: torch.Tensor    # [K + 1] i64: CSR over the masks of ...
    member_rows: torch.Tensor       # [M] i64: ... the sampled member rows (rows of the caller's cloud, ascending sample order)
    member_npcs: torch.Tensor       # [M, 3] f32: the NPCS of every member under ITS mask's class
    sample_rows: torch.Tensor       # [m] i64
    sampled_points: torch.Tensor    # [m, C] f32, normalised frame
    sampled_sem: torch.Tensor       # [m] i64
    label_votes: Optional[torch.Tensor] = None  # [K, n_classes] i32: the neighbours' votes behind ``label`` where a PartGrounder
                                                # chose it (``predict_frames_with_masks`` with ``labels[v] = None``), else None

    def to_numpy(self) -> dict:
        return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in self.__dict__.items()
                if v is not None}


def scene_maps_torch(valid_indices, sorted_indices, proposal_offsets, npcs_valid_mask, npcs_preds, n_rows):
    """gpn_scene_maps in torch ops (include/gpn.h section VS): a row written by several proposal points keeps the highest"""
    dev = sorted_indices.device
    M = sorted_indices.shape[0]
    rows = valid_indices[sorted_indices]
    po = proposal_offsets.long()
    ar = torch.arange(M, device=dev)
    pid = torch.searchsorted(po[1:].contiguous(), ar, right=True)
    winner = torch.full((n_rows,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, rows, ar, "amax")
    hit = winner >= 0
    w = winner.clamp(min=0)
    ins_map = torch.where(hit, pid[w] + 1, 0).to(torch.int32) if M else torch.zeros(n_rows, dtype=torch.int32, device=dev)
    npcs_map = torch.zeros((n_rows, 3), dtype=torch.float32, device=dev)
    if M:
        mask = npcs_valid_mask.bool()
        slot = (mask.long().cumsum(0) - 1).clamp(min=0)
        inside = hit & mask[w]
        npcs_map = torch.where(inside[:, None], npcs_preds[slot[w]] if npcs_preds.shape[0] else npcs_map, npcs_map)
    return ins_map, npcs_map, npcs_map[rows] - 0.5


def _scene_predictions(kept, scene_offsets, picks, max_iters):
    """misc.visu.scene_predictions on the GPU; the same steps in torch ops for CPU tensors"""
    from .misc import visu
    if kept.sorted_indices.is_cuda:
        return visu.scene_predictions(kept, scene_offsets, picks=picks, max_iters=max_iters)
    off = torch.as_tensor(scene_offsets, dtype=torch.int64)
    po = kept.proposal_offsets.long()
    ins_map, npcs_map, fit_npcs = scene_maps_torch(kept.valid_indices, kept.sorted_indices, po, kept.npcs_valid_mask,
                                                   kept.npcs_preds, int(off[-1]))
    P = po.shape[0] - 1
    empty = torch.zeros(0, dtype=torch.int64)
    if P <= 0:
        return visu.ScenePredictions(ins_map, npcs_map, torch.zeros((0, 8, 3), dtype=torch.float64), empty, empty, off)
    fit = estimate_pose_from_npcs_batched(kept.pt_xyz, fit_npcs, po, picks=picks, max_iters=max_iters)
    keep = ((po[1:] - po[:-1]) >= 10) & fit["valid"]
    box_proposal = torch.nonzero(keep).squeeze(1)
    box_scene = kept.batch_indices.index_select(0, po[:-1]).long().index_select(0, box_proposal)
    return visu.ScenePredictions(ins_map, npcs_map, fit["bbox"].index_select(0, box_proposal), box_scene, box_proposal, off)


Picks = Union[None, torch.Tensor, Callable[[List[int]], torch.Tensor]]
# what the command line writes per mask (``mask_<field>`` in the cloud's .npz)
MASK_FIELDS = ("kept", "n_points", "label", "score", "valid", "scale", "rotation", "translation", "transform", "bbox", "bbox_normalised",
               "member_offsets", "member_rows", "member_npcs")


def _rows_through_nearest(prep: PreparedClouds, net_off: List[int], *per_sample: torch.Tensor) -> List[torch.Tensor]:
    """every row of the caller's clouds through its nearest sampled point: for each tensor over the network's rows (``net_off``: the
    clouds' first rows there) the tensor over the caller's rows; -1 (integers) or 0 (floats) on rows that have no sample"""
    dev = prep.source.device
    nn = nearest_samples(prep)
    first = torch.repeat_interleave(torch.tensor(net_off[:-1], dtype=torch.int64).to(dev),
                                    torch.tensor([b - a for a, b in zip(prep.offsets[:-1], prep.offsets[1:])]).to(dev),
                                    output_size=prep.offsets[-1])
    hit = nn >= 0
    g = (first + nn).clamp(min=0, max=max(net_off[-1] - 1, 0))
    return [torch.where(hit.reshape(-1, *[1] * (v.dim() - 1)), v[g], 0.0 if v.is_floating_point() else -1) for v in per_sample]


class PartPredictor:
    """``predict(clouds)``: raw clouds in, per cloud the parts of EVERY row and one 9-DoF box per part in the caller's frame.
    ``picks``: the RANSAC draws of the box fits - None (drawn from numpy's global generator), a tensor [kept proposals,
    max_iters, 5], or a callable taking the kept proposals' sizes (in batch order) and returning that tensor."""

    def __init__(self, model, num_points: int = 20000, max_iters: int = 100, sampler: str = "fps"):
        self.model, self.num_points, self.max_iters = model.eval(), int(num_points), int(max_iters)
        self.sampler = _check_sampler(sampler)  # "grid": the opt-in octree-cell sampler (clouds take the seeds 0, 1, ...)

    def with_sampler(self, sampler: Optional[str]) -> "PartPredictor":
        """this predictor, or one of the same model and settings with another ``sampler`` (None: keep this one's)"""
        if sampler is None or sampler == self.sampler:
            return self
        return type(self)(self.model, num_points=self.num_points, max_iters=self.max_iters, sampler=sampler)

    def _empty(self, n: int, C: int, status: int, scale, dev) -> PartPrediction:
        i64, f32 = torch.int64, torch.float32
        z = lambda *shape, dtype=i64: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
        return PartPrediction(status=status, scale=scale, sem=torch.full((n,), -1, dtype=i64, device=dev),
                              instance=torch.full((n,), -1, dtype=i64, device=dev), npcs=z(n, 3, dtype=f32),
                              proposal_scores=z(0, dtype=f32), proposal_classes=z(0), bbox=z(0, 8, 3, dtype=torch.float64),
                              box_proposal=z(0), sample_rows=z(0), sampled_points=z(0, C, dtype=f32), sampled_sem=z(0),
                              sampled_instance=z(0), sampled_npcs=z(0, 3, dtype=f32), bbox_normalised=z(0, 8, 3, dtype=torch.float64))

    @torch.no_grad()
    def predict(self, clouds: Sequence[torch.Tensor], picks: Picks = None) -> List[PartPrediction]:
        return self._predict_prepared(prepare_clouds(clouds, self.num_points, sampler=self.sampler), picks)

    def _predict_prepared(self, prep: PreparedClouds, picks: Picks = None) -> List[PartPrediction]:
        """everything behind the preparation, shared by ``predict`` (raw clouds) and ``predict_frames`` (RGB-D frames)"""
        model = self.model
        C = prep.source.shape[1]
        if C < model.in_channels:
            raise ValueError(f"the model reads {model.in_channels} columns per point, the clouds have {C}")
        dev = prep.source.device
        S = len(prep.offsets) - 1
        counts = prep.counts.tolist()
        net_off = [0]
        for c in counts:
            net_off.append(net_off[-1] + c)
        ok = [s for s in range(S) if counts[s] > 0]
        out = [self._empty(prep.offsets[s + 1] - prep.offsets[s], C, int(prep.status[s]), prep.scale[s], dev) for s in range(S)]
        if not ok:
            return out
        pcs = [PointCloud(pc_id=str(s), points=prep.points[net_off[s]:net_off[s + 1], :model.in_channels].contiguous(), obj_cat=0)
               for s in ok]
        _, sem_seg, proposals = model(pcs)
        n_net = net_off[-1]
        sem = sem_seg.sem_preds.long()
        ins = torch.full((n_net,), -1, dtype=torch.int64, device=dev)
        npcs = torch.zeros((n_net, 3), dtype=torch.float32, device=dev)
        kept = pred = None
        if proposals is not None:
            kept = model._post_process_kept_points(proposals)
            sizes = kept.proposal_offsets[1:] - kept.proposal_offsets[:-1]
            if callable(picks):
                picks = picks(sizes.tolist())
            # (scene k of the network's batch is the k-th OK cloud; the clouds that are not OK own no rows)
            pred = _scene_predictions(kept, [net_off[s] for s in ok] + [n_net], picks, self.max_iters)
            ins, npcs = pred.ins_map.long() - 1, pred.npcs_map
        sem_all, ins_all, npcs_all = _rows_through_nearest(prep, net_off, sem, ins, npcs)
        if kept is not None:
            P = kept.score_preds.shape[0]
            prop_scene = kept.batch_indices.index_select(0, kept.proposal_offsets[:-1].long()).long()  # [P], in the OK clouds' numbering
            # position of every proposal among its own scene's proposals
            local = torch.zeros(P, dtype=torch.int64, device=dev)
            for k in range(len(ok)):
                mine = prop_scene == k
                local = torch.where(mine, mine.long().cumsum(0) - 1, local)
            local_pad = torch.cat([local, local.new_full((1,), -1)])
            # (the scene of every proposal and of every box in ONE copy to the host: the clouds' slices are listed there)
            scene_host = torch.cat([prop_scene, pred.box_scene.long()]).cpu()
            prop_scene_host, box_scene_host = scene_host[:P], scene_host[P:]
        for k, s in enumerate(ok):
            a, b = prep.offsets[s], prep.offsets[s + 1]
            na, nb = net_off[s], net_off[s + 1]
            o = out[s]
            o.sem, o.npcs = sem_all[a:b], npcs_all[a:b]
            o.sample_rows, o.sampled_points = prep.sample_rows[na:nb], prep.points[na:nb]
            o.sampled_sem, o.sampled_npcs = sem[na:nb], npcs[na:nb]
            o.instance, o.sampled_instance = ins_all[a:b], ins[na:nb]
            if kept is None:
                continue
            o.instance, o.sampled_instance = local_pad[ins_all[a:b]], local_pad[ins[na:nb]]
            mine = torch.nonzero(prop_scene_host == k).squeeze(1).to(dev, non_blocking=True)
            o.proposal_scores = kept.score_preds.index_select(0, mine)
            o.proposal_classes = kept.pt_sem_classes.index_select(0, mine).long()
            boxes = torch.nonzero(box_scene_host == k).squeeze(1).to(dev, non_blocking=True)
            o.bbox_normalised = pred.bbox.index_select(0, boxes)
            sc = prep.scale[s].to(dev)
            o.bbox = o.bbox_normalised * sc[0] + sc[1:]
            o.box_proposal = local[pred.box_proposal.index_select(0, boxes)]
        return out

    @torch.no_grad()
    def predict_with_masks(self, clouds: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], labels: Sequence[torch.Tensor],
                           picks: Picks = None, min_points: int = 6) -> List[MaskPrediction]:
        """``masks[s]`` [K_s, N_s] bool / u8 on the RAW rows of cloud s (a row with a non-finite coordinate is never sampled, so it is
        never a member), ``labels[s]`` [K_s] part classes.  A mask with fewer than ``min_points`` SAMPLED members is dropped (the
        reference's ``sum > 5``, structure/gapartnet.py:635).  Every kept mask is fitted with its OWN NPCS (a point shared by two
        masks carries two predictions); a box needs at least 5 points and a valid fit (the reference's ``<= 4: continue``)."""
        return self._predict_masks_prepared(prepare_clouds(clouds, self.num_points, sampler=self.sampler), masks, labels, picks,
                                            min_points)

    def _predict_masks_prepared(self, prep: PreparedClouds, masks, labels, picks: Picks = None, min_points: int = 6) -> List[MaskPrediction]:
        """everything behind the preparation, shared by ``predict_with_masks`` and ``predict_frames_with_masks``"""
        model = self.model
        C = prep.source.shape[1]
        if C < model.in_channels:
            raise ValueError(f"the model reads {model.in_channels} columns per point, the clouds have {C}")
        dev = prep.source.device
        S = len(prep.offsets) - 1
        if len(masks) != S or len(labels) != S:
            raise ValueError(f"{S} clouds need {S} mask tensors and {S} label tensors")
        masks = [torch.as_tensor(m).to(dev) for m in masks]
        labels = [torch.as_tensor(v).to(dev).long().reshape(-1) for v in labels]
        for s in range(S):
            n = prep.offsets[s + 1] - prep.offsets[s]
            if masks[s].dim() != 2 or masks[s].shape[0] != labels[s].shape[0] or (masks[s].shape[0] and masks[s].shape[1] != n):
                raise ValueError(f"cloud {s}: masks must be [K, {n}] with one label per mask, got {tuple(masks[s].shape)} and "
                                 f"{labels[s].shape[0]} labels")
        counts = prep.counts.tolist()
        net_off = [0]
        for c in counts:
            net_off.append(net_off[-1] + c)
        ok = [s for s in range(S) if counts[s] > 0]
        f64, i64, nan = torch.float64, torch.int64, float("nan")

        def dropped(s, K):
            z = lambda *shape, dtype=f64, fill=nan: torch.full(shape, fill, dtype=dtype, device=dev)  # noqa: E731
            n = prep.offsets[s + 1] - prep.offsets[s]
            return MaskPrediction(
                status=int(prep.status[s]), cloud_scale=prep.scale[s], sem=z(n, dtype=i64, fill=-1), kept=z(K, dtype=torch.bool, fill=False),
                n_points=z(K, dtype=i64, fill=0), label=labels[s], score=z(K, dtype=torch.float32), valid=z(K, dtype=torch.bool, fill=False),
                scale=z(K), rotation=z(K, 3, 3), translation=z(K, 3), transform=z(K, 4, 4), bbox=z(K, 8, 3), bbox_normalised=z(K, 8, 3),
                member_offsets=z(K + 1, dtype=i64, fill=0), member_rows=z(0, dtype=i64, fill=0), member_npcs=z(0, 3, dtype=torch.float32),
                sample_rows=z(0, dtype=i64, fill=0), sampled_points=z(0, C, dtype=torch.float32), sampled_sem=z(0, dtype=i64, fill=0))

        out = [dropped(s, int(masks[s].shape[0])) for s in range(S)]
        if not ok:
            return out
        pcs = [PointCloud(pc_id=str(s), points=prep.points[net_off[s]:net_off[s + 1], :model.in_channels].contiguous(), obj_cat=0)
               for s in ok]
        _, sem_seg, props, _ = model.forward_with_masks(pcs, [masks[s] for s in ok], [labels[s] for s in ok], min_points=min_points,
                                                        sample_rows=prep.sample_rows)
        sem = sem_seg.sem_preds.long()
        sem_all, = _rows_through_nearest(prep, net_off, sem)
        # per mask of the batch (the OK clouds' masks, concatenated): scattered from the kept ones
        gstart = [0]
        for s in ok:
            gstart.append(gstart[-1] + int(masks[s].shape[0]))
        Kt = gstart[-1]
        full = lambda *shape, dtype=f64, fill=nan: torch.full((Kt,) + shape, fill, dtype=dtype, device=dev)  # noqa: E731
        kept, n_points, score, valid = full(dtype=torch.bool, fill=False), full(dtype=i64, fill=0), full(dtype=torch.float32), \
            full(dtype=torch.bool, fill=False)
        pose = dict(scale=full(), rotation=full(3, 3), translation=full(3), transform=full(4, 4), bbox=full(8, 3))
        sizes_host = [0] * Kt
        if props is not None:
            pm = props.proposal_mask
            po = props.proposal_offsets.long()
            sizes = po[1:] - po[:-1]
            n_points[pm] = sizes
            sizes_host = n_points.tolist()  # the call's one read behind the model's: member CSR of every cloud, the fits' draws
            kept_sizes = [n for n in sizes_host if n > 0]
            if callable(picks):
                picks = picks(kept_sizes)
            elif picks is None:
                from .misc.pose_fitting_batched import draw_picks
                picks = draw_picks(kept_sizes, self.max_iters)
            fit = estimate_pose_from_npcs_batched(props.pt_xyz, props.npcs_preds - 0.5, po, picks=picks, max_iters=self.max_iters)
            box = (sizes >= 5) & fit["valid"]
            kept[pm], score[pm], valid[pm] = True, props.score_preds, box
            for f in pose:
                shape = (-1,) + (1,) * (fit[f].dim() - 1)
                pose[f][pm] = torch.where(box.reshape(shape), fit[f], torch.full_like(fit[f], nan))
            member_rows = prep.sample_rows.index_select(0, props.point_indices)
        cum = np.concatenate([[0], np.cumsum(sizes_host)]).astype(np.int64)
        cum_dev = torch.from_numpy(cum).to(dev)
        for k, s in enumerate(ok):
            a, b = prep.offsets[s], prep.offsets[s + 1]
            na, nb = net_off[s], net_off[s + 1]
            g0, g1 = gstart[k], gstart[k + 1]
            o = out[s]
            o.sem = sem_all[a:b]
            o.sample_rows, o.sampled_points, o.sampled_sem = prep.sample_rows[na:nb], prep.points[na:nb], sem[na:nb]
            o.kept, o.n_points, o.score, o.valid = kept[g0:g1], n_points[g0:g1], score[g0:g1], valid[g0:g1]
            sc = prep.scale[s].to(dev)
            r, c = sc[0], sc[1:]
            # caller's frame = normalised * r + c: the similarity's linear part and translation scale by r, the centre is added
            o.scale, o.rotation = pose["scale"][g0:g1] * r, pose["rotation"][g0:g1]
            o.translation = pose["translation"][g0:g1] * r + c
            T = pose["transform"][g0:g1].clone()
            T[:, :3, :3] = T[:, :3, :3] * r
            T[:, :3, 3] = o.translation
            o.transform = T
            o.bbox_normalised = pose["bbox"][g0:g1]
            o.bbox = o.bbox_normalised * r + c
            o.member_offsets = cum_dev[g0:g1 + 1] - int(cum[g0])
            if props is not None:
                o.member_rows = member_rows[int(cum[g0]):int(cum[g1])]
                o.member_npcs = props.npcs_preds[int(cum[g0]):int(cum[g1])]
        return out

    # ------------------------------------------------------------------------------------------------ RGB-D frames
    def _frame_predictions(self, preds, rgb, K, flip) -> List["FramePrediction"]:
        V, H, W, _ = rgb.shape
        unflip = torch.tensor([1.0, -1.0, -1.0] if flip else [1.0, 1.0, 1.0], dtype=torch.float64).to(rgb.device, non_blocking=True)
        boxes = [p.bbox * unflip for p in preds]
        overlay = draw_overlays(rgb, boxes, K)
        return [FramePrediction(status=p.status, scale=p.scale, sem=p.sem.reshape(H, W), instance=p.instance.reshape(H, W),
                                npcs=p.npcs.reshape(H, W, 3), proposal_scores=p.proposal_scores, proposal_classes=p.proposal_classes,
                                bbox=boxes[v], box_proposal=p.box_proposal, corners_px=project_corners(boxes[v], K[v]),
                                overlay=overlay[v], sample_rows=p.sample_rows) for v, p in enumerate(preds)]

    @staticmethod
    def _ground_labels(ask, labels, votes, masks, size, V, features, grounder):
        """the frames ``ask`` of ``predict_frames_with_masks`` carry no labels: one ``PartGrounder.label_masks`` call over all their
        masks (``mask_view`` = the frame's place among the asked ones) -> (labels, votes) with those frames filled in"""
        from ._C import GpnError
        if features is None or grounder is None:
            raise GpnError(f"frames {ask} have no labels: pass features= (one feature map per frame) and grounder= (a PartGrounder)")
        if len(features) != V:
            raise GpnError(f"{V} frames need {V} feature maps, got {len(features)}")
        dev = grounder.device
        maps = [torch.as_tensor(features[v]).to(dev) for v in ask]
        if any(m.dim() != 3 or m.shape != maps[0].shape for m in maps):
            raise GpnError(f"feature maps must be [Hf, Wf, C] of one size, got {[tuple(m.shape) for m in maps]}")
        counts = [int(torch.as_tensor(masks[v]).shape[0]) for v in ask]
        with_masks = [torch.as_tensor(masks[v]).to(dev) for v, n in zip(ask, counts) if n]
        stacked = torch.cat(with_masks) if with_masks else torch.zeros((0,) + tuple(size), dtype=torch.bool, device=dev)
        view = torch.tensor([j for j, n in enumerate(counts) for _ in range(n)], dtype=torch.int32)
        got = grounder.label_masks(torch.stack(maps), stacked, view)
        labels, votes = list(labels), list(votes)
        start = 0
        for v, n in zip(ask, counts):
            labels[v], votes[v] = got["label"][start:start + n], got["votes"][start:start + n]
            start += n
        return labels, votes

    @torch.no_grad()
    def predict_frames(self, depth, rgb, K, picks: Picks = None, presample: int = 4, seed=0, keep=None, depth_scale: float = 1.0,
                       flip: bool = False, isolate: Optional[IsolateConfig] = None) -> List["FramePrediction"]:
        """RGB-D frames in (``prepare_frames``), per frame the parts of EVERY pixel as [H,W] maps, one 9-DoF box per part in the
        camera frame, the boxes' corner pixels and the RGB image with the boxes drawn.  ``flip``: the rows (and so the network's
        input) have y and z negated, as the reference's ``get_pc`` mode 2; boxes are turned back before they are returned and drawn.
        Host reads: 6, those of ``predict`` and no more (7 when ``picks`` is a callable) - ONE for the preparation (counts, status,
        scale), the model's own (voxelisation, proposal stage), post-processing, box selection, ONE for the scenes of the proposals
        and boxes; ``K`` is host data.  ``isolate``: the object is cut out of the raw frame first (``isolate_objects``); the
        predictions gain ``keep``, ``planes`` and ``isolate_status``, for ONE more host read (the statuses)."""
        depth, rgb, K, keep = _check_frames(depth, rgb, K, keep)
        prep = _prepare_checked_frames(depth, rgb, K, keep, self.num_points, presample, seed, depth_scale, flip, sampler=self.sampler,
                                       isolate=isolate)
        return self._with_isolation(self._frame_predictions(self._predict_prepared(prep, picks), rgb, K, flip), prep)

    @staticmethod
    def _with_isolation(frames: List["FramePrediction"], prep: PreparedClouds) -> List["FramePrediction"]:
        iso = prep.isolation
        if iso is not None:
            status = iso.status.cpu().tolist()  # (the one host read isolation adds)
            for v, f in enumerate(frames):
                f.keep, f.planes, f.isolate_status = iso.keep[v], iso.planes[v], int(status[v])
        return frames

    @torch.no_grad()
    def predict_frames_with_masks(self, depth, rgb, K, masks: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], picks: Picks = None,
                                  min_points: int = 6, presample: int = 4, seed=0, keep=None, depth_scale: float = 1.0,
                                  flip: bool = False, features=None, grounder=None,
                                  isolate: Optional[IsolateConfig] = None) -> List["FramePrediction"]:
        """``predict_with_masks`` on frames: ``masks[v]`` [K_v, H, W] bool / u8 pixel masks (SAM's, or given ones;
        the reference's pixel_mask_to_point_mask), ``labels[v]`` [K_v] part classes.  Flattened, a pixel mask is a mask over the
        frame's rows.  -> ``FramePrediction`` per frame, its fields PER MASK in the caller's order where ``predict_frames`` has them
        per part: ``sem`` is the network's own class map; ``masks`` holds the per-mask fields of ``MaskPrediction`` (boxes in the
        rows' frame); ``bbox`` [K,8,3] / ``corners_px`` [K,8,2] are the masks' boxes in the camera frame, NaN for a mask without a
        valid box (``masks.valid``); ``overlay`` shows the valid ones (the line rule skips a non-finite corner);
        ``proposal_scores`` / ``proposal_classes`` are the masks' scores (NaN where dropped) and the caller's labels;
        ``box_proposal`` = arange(K).  Masks may overlap, so there is no per-pixel part: ``instance`` is -1 and ``npcs`` zero
        everywhere (the members' NPCS are in ``masks.member_npcs``).  Host reads: 4, those of ``predict_with_masks`` - ONE for the
        preparation, the model's two (voxelisation, mask stage), ONE for the masks' sizes; nothing behind them has a
        data-dependent size.

        Class-agnostic masks: ``labels[v] = None`` (or ``labels=None`` for every frame) with ``features`` - one image feature map
        [Hf,Wf,C] per frame, all of one size - and ``grounder``, a ``misc.grounding.PartGrounder``: the masks of those frames are
        labelled first (``PartGrounder.label_masks``, one call for all of them, no host read), ``masks.label`` /
        ``proposal_classes`` are the chosen classes and ``masks.label_votes`` [K,n_classes] the neighbours' votes.  A call that
        passes every label never touches ``features`` or ``grounder``.  (Masks on cloud rows, ``predict_with_masks``, have no pixel
        grid to pool a feature map over: label those with ``PartGrounder.label_masks`` / ``.predict`` on your own features.)"""
        depth, rgb, K, keep = _check_frames(depth, rgb, K, keep)
        V, H, W = (int(v) for v in depth.shape)
        flat = []
        for v, mk in enumerate(masks):
            mk = torch.as_tensor(mk)
            if mk.dim() != 3 or (mk.shape[0] and tuple(mk.shape[1:]) != (H, W)):
                raise ValueError(f"frame {v}: masks must be [K, {H}, {W}], got {tuple(mk.shape)}")
            flat.append(mk.reshape(mk.shape[0], H * W))
        labels = [None] * len(flat) if labels is None else list(labels)
        votes = [None] * len(labels)
        ask = [v for v, lab in enumerate(labels) if lab is None]
        if ask:
            labels, votes = self._ground_labels(ask, labels, votes, masks, (H, W), V, features, grounder)
        prep = _prepare_checked_frames(depth, rgb, K, keep, self.num_points, presample, seed, depth_scale, flip, sampler=self.sampler,
                                       isolate=isolate)
        mp = self._predict_masks_prepared(prep, flat, labels, picks, min_points)
        for p, vt in zip(mp, votes):
            p.label_votes = vt
        dev = rgb.device
        unflip = torch.tensor([1.0, -1.0, -1.0] if flip else [1.0, 1.0, 1.0], dtype=torch.float64).to(dev, non_blocking=True)
        boxes = [p.bbox * unflip for p in mp]   # (NaN where not valid: drawn by nobody)
        overlay = draw_overlays(rgb, boxes, K)
        return self._with_isolation(
            [FramePrediction(status=p.status, scale=p.cloud_scale, sem=p.sem.reshape(H, W),
                             instance=torch.full((H, W), -1, dtype=torch.int64, device=dev),
                             npcs=torch.zeros((H, W, 3), dtype=torch.float32, device=dev), proposal_scores=p.score,
                             proposal_classes=p.label, bbox=boxes[v], box_proposal=torch.arange(boxes[v].shape[0], device=dev),
                             corners_px=project_corners(boxes[v], K[v]), overlay=overlay[v], sample_rows=p.sample_rows, masks=p)
             for v, p in enumerate(mp)], prep)


# ---------------------------------------------------------------------------------------------------- files and the command line
def read_obj_points(path: str) -> np.ndarray:
    """the reference's OBJfile2points (tools/visu_utils.py:141-155): every line ``v x y z r g b`` up to the first ``vt`` line
    -> float64 [n, 6]"""
    points = []
    with open(path) as fh:
        for line in fh:
            strs = line.split(" ")
            if strs[0] == "v":
                points.append(tuple(float(v) for v in strs[1:7]))
            if strs[0] == "vt":
                break
    return np.array(points)


def load_model(ckpt: str, device, inference_dtype: Optional[str] = None):
    """a checkpoint as gapartnet_amd.trainer writes it ({"state_dict", "hyper_parameters"}) -> GAPartNet in eval mode"""
    from .network.model import GAPartNet
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    args = dict(ck["hyper_parameters"])
    args["ckpt"] = ""
    args["inference_dtype"] = torch.bfloat16 if inference_dtype == "bf16" else None
    model = GAPartNet(**args)
    model.load_state_dict(ck["state_dict"])
    return model.to(device).eval()


def _read_cloud(path: str, flip: bool) -> np.ndarray:
    if path.endswith(".obj"):
        pts = read_obj_points(path)
        if flip:  # tools/visu.py:150-151
            pts[:, 2] = -pts[:, 2]
            pts[:, 1] = -pts[:, 1]
        return pts.astype(np.float32)
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32)
    raise ValueError(f"{path}: inputs are .npy arrays [N, C >= 3] or .obj files with `v x y z r g b` lines")


def _write_panels(preds: Sequence[PartPrediction], names: Sequence[str], out_dir: str, mask_preds=None):
    """the prediction tiles of the test epoch's panel (misc/visu.render_panels) over the sampled points of every OK cloud; with
    ``mask_preds`` (predict_with_masks) the box tiles draw the caller's masks' boxes instead of the clustered parts'"""
    from .misc import visu
    if mask_preds is not None:
        import copy
        shown = []
        for p, mp in zip(preds, mask_preds):
            p = copy.copy(p)
            if p.status == CLOUD_OK:
                p.bbox_normalised, p.bbox = mp.bbox_normalised[mp.valid], mp.bbox[mp.valid]
            shown.append(p)
        preds = shown
    rows = [(n, p) for n, p in zip(names, preds) if p.status == CLOUD_OK]
    if not rows:
        return []
    dev = rows[0][1].sampled_points.device
    off = np.concatenate([[0], np.cumsum([p.sampled_points.shape[0] for _, p in rows])]).astype(np.int64)
    xyz = torch.cat([p.sampled_points[:, :3] for _, p in rows]).contiguous()
    rgb = torch.cat([p.sampled_points[:, 3:6] if p.sampled_points.shape[1] >= 6 else torch.full_like(p.sampled_points[:, :3], 0.6)
                     for _, p in rows]).contiguous()
    options = ("pc", "sem_pred", "ins_pred", "npcs_pred", "bbox_pred", "bbox_pred_pure")
    canvas = visu.render_panels(
        xyz, rgb, off, torch.stack([p.scale for _, p in rows]).to(dev),
        sem_pred=torch.cat([p.sampled_sem for _, p in rows]).int(), ins_pred=torch.cat([p.sampled_instance + 1 for _, p in rows]).int(),
        npcs_pred=torch.cat([p.sampled_npcs for _, p in rows]).contiguous(),
        bbox_pred=torch.cat([p.bbox_normalised for _, p in rows]),
        bbox_pred_scene=torch.cat([torch.full((p.bbox.shape[0],), k, dtype=torch.int32, device=dev) for k, (_, p) in enumerate(rows)]),
        options=options).cpu().numpy()
    from PIL import Image
    paths = []
    for k, (name, _) in enumerate(rows):
        paths.append(os.path.join(out_dir, name + ".png"))
        Image.fromarray(canvas[k]).save(paths[-1], compress_level=1)
    return paths


def _read_image(path: str) -> np.ndarray:
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image
    return np.asarray(Image.open(path))


def _read_depth(path: str) -> np.ndarray:
    """[H, W] float32 / float64 / uint16 (a 16-bit PNG stays uint16: --depth_scale turns it into metres on the device)"""
    d = _read_image(path)
    if d.ndim != 2:
        raise ValueError(f"{path}: a depth map is [H, W], got {d.shape}")
    if d.dtype in (np.float32, np.float64, np.uint16):
        return d
    if d.dtype.kind in "iu" and d.min() >= 0 and d.max() < 65536:  # (PIL opens 16-bit PNGs as int32 "I")
        return d.astype(np.uint16)
    return d.astype(np.float32)


def _main_frames(ap, args, model, device) -> int:
    n = len(args.depth)
    if args.rgb is None or len(args.rgb) != n or args.intrinsics is None or len(args.intrinsics) not in (1, n):
        ap.error(f"--depth takes one --rgb per frame ({n}) and --intrinsics once or per frame")
    if args.keep_mask is not None and len(args.keep_mask) != n:
        ap.error(f"--keep_mask takes one file per frame ({n}), got {len(args.keep_mask)}")
    if args.masks is not None and len(args.masks) != n:
        ap.error(f"--masks takes one file per frame ({n}), got {len(args.masks)}")
    if args.panels:
        ap.error("--panels belongs to --input; frames write <name>_overlay.png")
    depth = [_read_depth(p) for p in args.depth]
    rgb = [np.ascontiguousarray(_read_image(p)[..., :3]).astype(np.uint8) for p in args.rgb]
    Ks = [(np.load(p) if p.endswith(".npy") else np.loadtxt(p)).astype(np.float64).reshape(3, 3) for p in args.intrinsics]
    Ks = Ks * n if len(Ks) == 1 else Ks
    keep = None if args.keep_mask is None else [(_read_image(p).reshape(d.shape[0], d.shape[1], -1) != 0).any(-1).astype(np.uint8)
                                                for p, d in zip(args.keep_mask, depth)]
    given = None
    if args.masks is not None:
        given = []
        for path, d in zip(args.masks, depth):
            z = np.load(path)
            m = np.asarray(z["masks"]) != 0
            if "labels" not in z.files and args.bank is not None:  # class-agnostic masks: the bank labels them
                if m.shape[1:] != d.shape:
                    ap.error(f"{path}: `masks` must be [K, {d.shape[0]}, {d.shape[1]}], got {m.shape}")
                given.append((m, None))
                continue
            lab = np.asarray(z["labels"]).astype(np.int64).reshape(-1)
            if m.shape != (lab.shape[0],) + d.shape:
                ap.error(f"{path}: `masks` must be [K, {d.shape[0]}, {d.shape[1]}] with `labels` [K], got {m.shape} and {lab.shape}")
            given.append((m, lab))
    grounder, fmaps = None, None
    if args.bank is not None and any(lab is None for _, lab in given):
        from .misc.grounding import PartGrounder, load_feature_bank
        grounder = PartGrounder(*load_feature_bank(args.bank), device=device)
        fmaps = [np.load(p).astype(np.float32) for p in args.features]
        if any(f.ndim != 3 or f.shape != fmaps[0].shape for f in fmaps):
            ap.error(f"--features: maps must be [Hf, Wf, C] of one size, got {[f.shape for f in fmaps]}")
    for d, c, p in zip(depth, rgb, args.rgb):
        if c.shape != d.shape + (3,):
            ap.error(f"{p}: the image must be [{d.shape[0]}, {d.shape[1]}, 3], got {c.shape}")
    names = [os.path.splitext(os.path.basename(p))[0] for p in args.depth]
    os.makedirs(args.out, exist_ok=True)
    predictor = PartPredictor(model, num_points=args.num_points, sampler=args.sampler)
    isolate = None
    if args.isolate:
        try:
            isolate = IsolateConfig(max_planes=args.isolate_planes, tol=args.plane_tol, select=args.isolate_select, z_max=args.z_max)
        except ValueError as e:
            ap.error(str(e))
    preds: List[Optional[FramePrediction]] = [None] * n
    # (one batch per frame size and depth type)
    for key in sorted({(d.shape, d.dtype.str) for d in depth}):
        ids = [i for i, d in enumerate(depth) if (d.shape, d.dtype.str) == key]
        stack = lambda arrs: torch.from_numpy(np.stack([arrs[i] for i in ids])).to(device)  # noqa: E731
        kw = dict(presample=args.presample, seed=[(args.seed + i) & 0xffffffff for i in ids], keep=None if keep is None else stack(keep),
                  depth_scale=args.depth_scale, flip=args.flip, isolate=isolate)
        K = torch.from_numpy(np.stack([Ks[i] for i in ids]))
        if given is None:
            got = predictor.predict_frames(stack(depth), stack(rgb), K, **kw)
        else:
            if grounder is not None:
                kw.update(features=[torch.from_numpy(fmaps[i]).to(device) for i in ids], grounder=grounder)
            got = predictor.predict_frames_with_masks(stack(depth), stack(rgb), K, [torch.from_numpy(given[i][0]).to(device) for i in ids],
                                                      [None if given[i][1] is None else torch.from_numpy(given[i][1]).to(device) for i in ids],
                                                      **kw)
        for i, p in zip(ids, got):
            preds[i] = p
    from PIL import Image
    for name, p in zip(names, preds):
        arrays = p.to_numpy()
        np.savez(os.path.join(args.out, name + ".npz"), **arrays)
        Image.fromarray(arrays["overlay"]).save(os.path.join(args.out, name + "_overlay.png"), compress_level=1)
        line = f"{name}: {STATUS_NAMES.get(p.status, p.status)}, {p.sem.shape[0]} x {p.sem.shape[1]} pixels"
        if p.isolate_status is not None:
            line += f", isolation {ISOLATE_STATUS_NAMES.get(p.isolate_status, p.isolate_status)} ({int(arrays['keep'].sum())} pixels kept)"
        if p.masks is not None:
            line += f"; {p.masks.kept.shape[0]} masks, {int(p.masks.kept.sum())} kept, {int(p.masks.valid.sum())} boxes"
        else:
            line += f", {p.proposal_scores.shape[0]} parts, {p.bbox.shape[0]} boxes"
        print(line)
    return 0


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gapartnet_amd.inference", description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--input", nargs="+", default=None, help="raw clouds: .npy [N, C >= 3] or .obj")
    ap.add_argument("--depth", nargs="+", default=None, help="RGB-D frames instead of --input: depth maps, .npy or (16-bit) .png")
    ap.add_argument("--rgb", nargs="+", default=None, help="one image per depth map")
    ap.add_argument("--intrinsics", nargs="+", default=None, help="K [3,3] as .txt or .npy: one for all frames or one per frame")
    ap.add_argument("--depth_scale", type=float, default=1.0, help="depth units per metre (1000 for millimetre PNGs)")
    ap.add_argument("--keep_mask", nargs="+", default=None, help="one image per frame: non-zero pixels are kept")
    ap.add_argument("--flip", action="store_true", help="frames: negate y and z of the rows (the reference's get_pc mode 2)")
    ap.add_argument("--isolate", action="store_true",
                    help="frames: cut the object out of the raw frame first (planes by RANSAC, connected components); the .npz gains "
                         "keep, planes and isolate_status")
    ap.add_argument("--isolate_planes", type=int, default=1, help="--isolate: plane rounds, 1 (the table) .. 4")
    ap.add_argument("--plane_tol", type=float, default=0.005, help="--isolate: a pixel within this of a plane is on it (depth units)")
    ap.add_argument("--isolate_select", choices=ISOLATE_SELECT, default="largest", help="--isolate: which component is the object")
    ap.add_argument("--z_max", type=float, default=float("inf"), help="--isolate: ignore pixels deeper than this")
    ap.add_argument("--presample", type=int, default=4, help="frames: keep at most presample * num_points pixels before FPS (0: all)")
    ap.add_argument("--seed", type=int, default=0, help="frames: seed of the presample (frame i of the command line takes seed + i)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--num_points", type=int, default=20000)
    ap.add_argument("--sampler", choices=SAMPLERS, default="fps",
                    help="how a cloud or frame is cut to num_points: fps (what the checkpoints were trained on) or grid, the "
                         "octree-cell sampler - far faster on large inputs, a coarser cover")
    ap.add_argument("--inference_dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--panels", action="store_true")
    ap.add_argument("--no_flip", action="store_true", help="keep the y and z signs of .obj inputs")
    ap.add_argument("--masks", nargs="+", default=None,
                    help="one .npz per input, in order: `masks` [K, N] on the input's rows and `labels` [K] part classes")
    ap.add_argument("--bank", default=None,
                    help="frames with --masks: a bank of labelled part features (misc.grounding.load_feature_bank); the masks' "
                         "`labels` may then be missing and are chosen by a 5-nearest-neighbour vote")
    ap.add_argument("--features", nargs="+", default=None, help="with --bank: one image feature map [Hf, Wf, C] (.npy) per frame")
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    if (args.bank is None) != (args.features is None):
        ap.error("--bank and --features are given together")
    if args.bank is not None:
        if args.depth is None or args.masks is None:
            ap.error("--bank / --features label pixel masks: they go with --depth ... --masks")
        if len(args.features) != len(args.depth):
            ap.error(f"--features takes one feature map per frame ({len(args.depth)}), got {len(args.features)}")
    if args.panels and device.type != "cuda":
        ap.error("--panels renders on the GPU (misc/visu.render_panels): it cannot be combined with --device cpu")
    if (args.input is None) == (args.depth is None):
        ap.error("give either --input (raw clouds) or --depth / --rgb / --intrinsics (RGB-D frames)")
    model = load_model(args.ckpt, device, args.inference_dtype)
    if args.depth is not None:
        return _main_frames(ap, args, model, device)
    clouds = [torch.from_numpy(_read_cloud(p, not args.no_flip)).to(device) for p in args.input]
    given = None
    if args.masks is not None:
        if len(args.masks) != len(args.input):
            ap.error(f"--masks takes one file per input ({len(args.input)}), got {len(args.masks)}")
        given = []
        for path, cloud in zip(args.masks, clouds):
            z = np.load(path)
            m, lab = np.asarray(z["masks"]) != 0, np.asarray(z["labels"]).astype(np.int64).reshape(-1)
            if m.ndim != 2 or m.shape != (lab.shape[0], cloud.shape[0]):
                ap.error(f"{path}: `masks` must be [K, {cloud.shape[0]}] with `labels` [K], got {m.shape} and {lab.shape}")
            given.append((torch.from_numpy(m).to(device), torch.from_numpy(lab).to(device)))
    names = [os.path.splitext(os.path.basename(p))[0] for p in args.input]
    os.makedirs(args.out, exist_ok=True)
    # (one batch per column count: a batch shares its C)
    preds: List[Optional[PartPrediction]] = [None] * len(clouds)
    predictor = PartPredictor(model, num_points=args.num_points, sampler=args.sampler)
    for C in sorted({int(c.shape[1]) for c in clouds}):
        ids = [i for i, c in enumerate(clouds) if c.shape[1] == C]
        for i, p in zip(ids, predictor.predict([clouds[i] for i in ids])):
            preds[i] = p
    mask_preds: Optional[List[Optional[MaskPrediction]]] = None
    if given is not None:
        mask_preds = [None] * len(clouds)
        for C in sorted({int(c.shape[1]) for c in clouds}):
            ids = [i for i, c in enumerate(clouds) if c.shape[1] == C]
            got = predictor.predict_with_masks([clouds[i] for i in ids], [given[i][0] for i in ids], [given[i][1] for i in ids])
            for i, p in zip(ids, got):
                mask_preds[i] = p
    for k, (name, p) in enumerate(zip(names, preds)):
        arrays = p.to_numpy()
        line = (f"{name}: {STATUS_NAMES.get(p.status, p.status)}, {p.sem.shape[0]} rows, {p.proposal_scores.shape[0]} parts, "
                f"{p.bbox.shape[0]} boxes")
        if mask_preds is not None:
            mp = mask_preds[k]
            arrays.update({"mask_" + f: v for f, v in mp.to_numpy().items() if f in MASK_FIELDS})
            line += f"; {mp.kept.shape[0]} masks, {int(mp.kept.sum())} kept, {int(mp.valid.sum())} boxes"
        np.savez(os.path.join(args.out, name + ".npz"), **arrays)
        print(line)
    if args.panels:
        _write_panels(preds, names, args.out, mask_preds)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
