"""Raw (no autograd) HIP operators: torch CUDA tensors in/out, every computation inside libgpn_hip.so.

PyTorch is used here only for device memory (caching allocator) and the current HIP stream.  Every function
raises if given non-CUDA tensors — there is no CPU path in the product (the CPU oracle lives in ``oracle/``
and is test infrastructure).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _C
from ._C import check, f32, host_f32x3, host_i32x3, i32, i64, ptr, szt

TILE_ROWS = 32
PACK_TRANSPOSE = 1
PACK_REVERSE = 2
name = "hip"


def _stream():
    # raw current-stream handle (the C call behind torch.cuda.current_stream(), ~20x cheaper than building the wrapper)
    return _C.ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _dev(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _C.GpnError("gapartnet_amd HIP operators need CUDA(HIP) tensors; got a CPU tensor "
                              "(there is no CPU fallback in the product path)")
        dev = t.device
    return dev


def _c(t, dtype):
    if t is None:
        return None
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


_WS_CACHE = {}


def _ws(nbytes, device):
    """scratch workspace for one kernel call.  One grow-only buffer per (device, stream) is reused by every call:
    kernels on a stream run in order, so a later call can only overwrite scratch an earlier one is done with."""
    nbytes = max(int(nbytes), 256)
    key = (device.index, torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device()))
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty((max(nbytes * 2, 64 << 20),), dtype=torch.uint8, device=device)
        _WS_CACHE[key] = buf
    return buf


def n_tiles(n):
    return (int(n) + TILE_ROWS - 1) // TILE_ROWS


@dataclass
class Rulebook:
    """K pair lists ordered by (tap, dst) + per-32-row tile offsets (see include/gpn.h)."""
    pair_src: torch.Tensor
    pair_dst: torch.Tensor
    tile_off: torch.Tensor
    K: int
    n_src: int
    n_dst: int
    num_pairs: torch.Tensor  # 0-dim int64 on device (no host sync)
    nbr: Optional[torch.Tensor] = None  # tap-major neighbour table [K*n_dst + 1] i32 (-1 = none) the fused conv gathers from
    # optional tile order of the large levels (gpn_rulebook_tile_order): the table with its columns sorted by neighbour
    # mask inside 16384-row blocks, and the destination row of every tile position
    nbr_p: Optional[torch.Tensor] = None
    perm: Optional[torch.Tensor] = None
    # device-counted rulebooks (section DEV): n_src / n_dst above are the buffers' bounds, these the live counts' counters
    live_src: Optional["DevCount"] = None
    live_dst: Optional["DevCount"] = None

    def pairs_host(self) -> int:
        return int(self.num_pairs.item())


class ArenaRulebook:
    """A Rulebook whose tables are slices of ONE arena (gpn_backbone_prepare).  The network executor only needs addresses
    (``ptrs`` = nbr, nbr_p, perm, pair_src, pair_dst, tile_off; 0 = absent) - 28 rulebooks x 7 tables per batch were ~150 tensor
    views made and ~250 addresses read back per step for that; the views are made when something asks for them (the module-by-
    module path, the tests), through the same attribute names."""
    __slots__ = ("_owner", "_spec", "_made", "K", "n_src", "n_dst", "live_src", "live_dst", "ptrs")
    _FIELDS = ("nbr", "nbr_p", "perm", "pair_src", "pair_dst", "tile_off", "num_pairs")

    def __init__(self, owner, spec, K, n_src, n_dst):
        self._owner, self._spec, self._made = owner, spec, {}
        self.K, self.n_src, self.n_dst = K, n_src, n_dst
        self.live_src = self.live_dst = None
        base = owner.arena_ptr
        self.ptrs = tuple(base + spec[f][0] if spec.get(f) is not None else 0 for f in self._FIELDS[:6])

    def __getattr__(self, name):  # (only reached for names that are not slots: the table fields)
        if name not in ArenaRulebook._FIELDS:
            raise AttributeError(name)
        made = self._made
        if name not in made:
            ent = self._spec.get(name)
            t = None
            if ent is not None:
                off, count, dtype, shape = ent
                t = self._owner._view(off, count, dtype)
                t = t[0] if shape == () else (t.view(*shape) if shape is not None else t)
            made[name] = t
        return made[name]

    def pairs_host(self) -> int:
        return int(self.num_pairs.item())


class DevCount:
    """A row count that is still on the device (include/gpn.h section DEV): ``t`` = int64 [1] device tensor (usually a view
    into the counts array of the launch that produced it), ``plan`` = the host's estimate of its value (0 = none; it sizes
    grids and picks kernel variants, results never depend on it).  Tensors that go with it are allocated for a BOUND."""
    __slots__ = ("t", "plan")

    def __init__(self, t: torch.Tensor, plan: int = 0):
        assert t.dtype == torch.int64 and t.numel() == 1 and t.is_cuda
        self.t, self.plan = t, max(int(plan), 0)

    @property
    def ptr(self):
        return _C.ctypes.c_void_p(self.t.data_ptr())

    def args(self):
        """(device pointer, plan) as ctypes arguments"""
        return _C.ctypes.c_void_p(self.t.data_ptr()), _C.ctypes.c_int64(self.plan)


# ---------------------------------------------------------------------------------------------------- V
def voxelize(points, feats, seg_offsets, seg_range_min, seg_range_max, voxel_size, grid_dims, want_csr=False,
             want_stats=False):
    """Kernel V. Returns (voxel_feats [V,C], voxel_coords [V,3] i32, voxel_seg [V] i32, pc_voxel_id [M] i32
    [, point_order [M] i32, voxel_point_start [V+1] i32] [, stats]).  One host sync (number of voxels); with
    ``want_stats`` the same read also brings stats = {"max_coord": [3 ints], "dropped": points outside the grid}."""
    dev = _dev(points, feats, seg_offsets)
    points, feats = _c(points, torch.float32), _c(feats, torch.float32)
    seg_offsets = _c(seg_offsets, torch.int64)
    M, C, S = points.shape[0], feats.shape[1], seg_offsets.shape[0] - 1
    rmin = _c(seg_range_min.reshape(-1, 3).expand(S, 3), torch.float32)
    rmax = _c(seg_range_max.reshape(-1, 3).expand(S, 3), torch.float32)
    vf = torch.empty((M, C), dtype=torch.float32, device=dev)
    vc = torch.empty((M, 3), dtype=torch.int32, device=dev)
    vseg = torch.empty((M,), dtype=torch.int32, device=dev)
    pid = torch.empty((M,), dtype=torch.int32, device=dev)
    nv = torch.empty((1,), dtype=torch.int64, device=dev)  # (always written by the library)
    order = torch.empty((M,), dtype=torch.int32, device=dev) if want_csr else None
    vstart = torch.empty((M + 1,), dtype=torch.int32, device=dev) if want_csr else None
    L = _C.lib()
    ws = _ws(L.gpn_voxelize_ws_bytes(i64(M), i32(C)), dev)
    check(L.gpn_voxelize_ex(ptr(points), ptr(feats), ptr(seg_offsets), ptr(rmin), ptr(rmax), i64(M), i32(C),
                            i64(S), host_f32x3(voxel_size), host_i32x3(grid_dims), ptr(vf), ptr(vc), ptr(vseg),
                            ptr(pid), ptr(nv), ptr(order), ptr(vstart), ptr(ws), szt(ws.numel()), _stream()),
          "gpn_voxelize")
    stats = None
    if want_stats:
        live = torch.arange(M, device=dev)[:, None] < nv
        head = torch.cat([nv, torch.where(live, vc, torch.zeros_like(vc)).amax(0).to(torch.int64) if M > 0 else
                          torch.zeros((3,), dtype=torch.int64, device=dev), (pid < 0).sum()[None]]).tolist()
        V, stats = head[0], {"max_coord": head[1:4], "dropped": head[4]}
    else:
        V = int(nv.item())
    out = (vf[:V], vc[:V], vseg[:V], pid)
    if want_csr:
        out = out + (order, vstart[:V + 1])
    if want_stats:
        out = out + (stats,)
    return out


_PINNED_STATS = []  # pinned int64 buffers of finished voxelize_scenes_begin / _finish pairs, for reuse


def voxelize_scenes_begin(points, feats, seg_offsets, voxel_size, n_levels=0, sorted_form=False):
    """first half of ``voxelize_scenes``: every launch of gpn_voxelize_scenes plus an asynchronous copy of its statistics to
    pinned memory - NO host read.  ``voxelize_scenes_finish(handle)`` is the second half; issued a step later (the device
    prefetcher does: dataset/prefetch.py) it finds the statistics there and does not wait."""
    dev = _dev(points, feats, seg_offsets)
    points, feats = _c(points, torch.float32), _c(feats, torch.float32)
    seg_offsets = _c(seg_offsets, torch.int64)
    M, C, S = points.shape[0], feats.shape[1], seg_offsets.shape[0] - 1
    vf = torch.empty((M, C), dtype=torch.float32, device=dev)
    idx4 = torch.empty((max(M, 1), 4), dtype=torch.int32, device=dev)
    pid = torch.empty((M,), dtype=torch.int32, device=dev)
    order = torch.empty((M,), dtype=torch.int32, device=dev)
    vstart = torch.empty((M + 1,), dtype=torch.int32, device=dev)
    stats = torch.empty((8 + n_levels,), dtype=torch.int64, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_voxelize_scenes_ws_bytes(i64(M), i32(C), i64(S), i32(n_levels)), dev)
    # (sorted_form: the stable-sort implementation the sort-free one replaced in round 5 - kept as the fallback for grids that do
    # not fit the occupancy bitmap, and what the tests compare the sort-free form with)
    fn = L.gpn_voxelize_scenes_sorted if sorted_form else L.gpn_voxelize_scenes
    check(fn(ptr(points), ptr(feats), ptr(seg_offsets), i64(M), i32(C), i64(S), host_f32x3(voxel_size),
             i32(n_levels), ptr(vf), ptr(idx4), ptr(pid), ptr(order), ptr(vstart), ptr(stats), ptr(ws),
             szt(ws.numel()), _stream()), "gpn_voxelize_scenes")
    host = None
    for i, buf in enumerate(_PINNED_STATS):
        if buf.numel() == stats.numel():
            host = _PINNED_STATS.pop(i)
            break
    if host is None:
        host = torch.empty((stats.numel(),), dtype=torch.int64).pin_memory()
    host.copy_(stats, non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    return dict(vf=vf, idx4=idx4, pid=pid, order=order, vstart=vstart, stats=stats, host=host, done=done, n_levels=n_levels)


def voxelize_scenes_finish(handle):
    """second half: the one host read of batch preparation (of pinned memory, after the copy's event) and the slicing"""
    handle["done"].synchronize()
    st = handle["host"].tolist()
    if len(_PINNED_STATS) < 8:
        _PINNED_STATS.append(handle["host"])
    if st[5] != 0:
        return None
    V, n_levels = st[0], handle["n_levels"]
    return (handle["vf"][:V], handle["idx4"][:V], handle["pid"], handle["order"], handle["vstart"][:V + 1], st[1:4], st[4],
            st[8:8 + n_levels])


def voxelize_scenes(points, feats, seg_offsets, voxel_size, n_levels=0, sorted_form=False):
    """Scene-batch voxelisation with the reference's per-scene ranges and NO host read before or between the launches
    (gpn_voxelize_scenes).  -> (voxel_feats [V,C], indices [V,4] i32 = (scene,x,y,z), pc_voxel_id [M] i32, point_order [M],
    voxel_point_start [V+1], max_coord [3 ints], dropped, level_counts [n_levels ints]) after ONE host read, or None when
    a cell index did not fit the packed keys (>= 1024 cells along an axis: the caller takes voxelize() instead)."""
    got = voxelize_scenes_finish(voxelize_scenes_begin(points, feats, seg_offsets, voxel_size, n_levels, sorted_form))
    if got is None and not sorted_form:  # (stats[5] = 2: the batch's grid does not fit the sort-free form's bitmap)
        got = voxelize_scenes_finish(voxelize_scenes_begin(points, feats, seg_offsets, voxel_size, n_levels, True))
    return got


# ---------------------------------------------------------------------------------------------------- BP
class PreparedBackbone:
    """what gpn_backbone_prepare left in its arena: ``run()`` is the blocking native call (meant for a worker thread: ctypes
    releases the interpreter lock for its whole duration), ``wrap()`` turns the descriptor into tensors / Rulebooks (views of the
    arena)"""
    KHEAD, KRB = 16, 10
    KLEVEL = 8 + 4 * KRB

    def __init__(self, xyz, feats, seg_offsets, voxel_size, n_levels, ident_levels, stream):
        dev = _dev(xyz, feats, seg_offsets)
        self.xyz, self.feats, self.seg_offsets = _c(xyz, torch.float32), _c(feats, torch.float32), _c(seg_offsets, torch.int64)
        self.voxel_size, self.n_levels, self.ident_levels = [float(v) for v in voxel_size], int(n_levels), int(ident_levels)
        self.M, self.C, self.S = int(self.xyz.shape[0]), int(self.feats.shape[1]), int(self.seg_offsets.shape[0]) - 1
        L = _C.lib()
        L.gpn_backbone_prepare_arena_bytes.restype = _C.ctypes.c_size_t
        need = int(L.gpn_backbone_prepare_arena_bytes(i64(self.M), i32(self.C), i64(self.S), i32(self.n_levels)))
        self.arena = torch.empty((need,), dtype=torch.uint8, device=dev)  # (on the caller's current stream)
        self.desc = np.full((int(L.gpn_backbone_prepare_desc_words(i32(self.n_levels))),), -1, np.int64)
        self.pinned = torch.empty((8 + self.n_levels,), dtype=torch.int64).pin_memory()
        self.stream_handle = int(stream.cuda_stream)
        self.device_index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.rc, self.error = None, None
        self._typed = {}
        self.arena_ptr = self.arena.data_ptr()

    def run(self):
        L = _C.lib()
        rc = L.gpn_backbone_prepare(ptr(self.xyz), ptr(self.feats), ptr(self.seg_offsets), i64(self.M), i32(self.C), i64(self.S),
                                    host_f32x3(self.voxel_size), i32(self.n_levels), _C.ctypes.c_uint32(self.ident_levels),
                                    i64(TILE_ORDER_MIN_ROWS), i32(TILE_ORDER_BLOCK), i32(self.device_index), ptr(self.arena),
                                    szt(self.arena.numel()), _C.ctypes.c_void_p(self.desc.ctypes.data),
                                    _C.ctypes.c_void_p(self.pinned.data_ptr()), _C.ctypes.c_void_p(self.stream_handle))
        self.rc = int(rc)
        if rc:
            self.error = L.gpn_last_error().decode("utf-8", "replace")
        return self

    def fallback(self) -> bool:
        return self.rc != 0 or int(self.desc[5]) != 0

    _ITEM = {torch.int32: 4, torch.float32: 4, torch.int64: 8}

    def _view(self, off, count, dtype):
        """``count`` elements of ``dtype`` at byte offset ``off`` of the arena (one slicing op on a typed view of the whole arena:
        ~150 of these per batch)"""
        if off < 0:
            return None
        base = self._typed.get(dtype)
        if base is None:
            size = self._ITEM[dtype]
            base = self._typed[dtype] = self.arena[:self.arena.numel() // size * size].view(dtype)
        first = off // self._ITEM[dtype]  # (the library aligns every table to 256 bytes)
        return base[first:first + count]

    def _rulebook(self, words):
        o_nbr, o_src, o_dst, o_toff, o_np, o_nbrp, o_perm, n_src, n_dst, K = (int(v) for v in words)
        if o_nbr < 0:
            return None
        # pair-list capacities as gpn_backbone_prepare carved them: 27 n (SubM), the fine row count (stride-2 maps), n (identity)
        cap = 27 * n_dst if K == 27 else (n_dst if K == 1 else max(n_src, n_dst))
        i32 = torch.int32
        spec = dict(pair_src=(o_src, cap, i32, None), pair_dst=(o_dst, cap, i32, None),
                    tile_off=(o_toff, K * (n_tiles(n_dst) + 1), i32, (K, -1)), num_pairs=(o_np, 1, torch.int64, ()),
                    nbr=(o_nbr, K * n_dst + 1, i32, None))
        if o_perm >= 0:
            spec["perm"] = (o_perm, (n_dst + 15) // 16 * 16 + 16, i32, None)
            spec["nbr_p"] = (o_nbrp, K * n_dst + 1, i32, None)
        return ArenaRulebook(self, spec, K, n_src, n_dst)

    def wrap(self):
        """-> dict(features, indices, spatial_shape, pc_voxel_id, csr, level_counts, levels = [dict(indices, shape, subm,
        down_fwd, down_bwd, ident)])"""
        d = self.desc
        V = int(d[0])
        M, C = self.M, self.C
        out = dict(features=self._view(int(d[8]), M * C, torch.float32).view(M, C)[:V],
                   indices=self._view(int(d[9]), M * 4, torch.int32).view(M, 4)[:V], spatial_shape=[int(v) for v in d[1:4]],
                   pc_voxel_id=self._view(int(d[10]), M, torch.int32),
                   csr=(self._view(int(d[11]), M, torch.int32), self._view(int(d[12]), M + 1, torch.int32)[:V + 1]),
                   dropped=int(d[4]), levels=[])
        for l in range(self.n_levels):
            w = d[self.KHEAD + l * self.KLEVEL: self.KHEAD + (l + 1) * self.KLEVEL]
            rows = int(w[0])
            idx = out["indices"] if l == 0 else self._view(int(w[4]), rows * 4, torch.int32).view(rows, 4)
            rbs = [self._rulebook(w[8 + k * self.KRB: 8 + (k + 1) * self.KRB]) for k in range(4)]
            out["levels"].append(dict(indices=idx, shape=[int(v) for v in w[1:4]], subm=rbs[0], down_fwd=rbs[1], down_bwd=rbs[2],
                                      ident=rbs[3]))
        out["level_counts"] = [int(lv["indices"].shape[0]) for lv in out["levels"][1:]]
        return out


# ---------------------------------------------------------------------------------------------------- K
def rulebook_subm3(indices, spatial_shape, rows: Optional[DevCount] = None) -> Rulebook:
    """``rows``: the live row count of ``indices`` is a device counter (indices.shape[0] = its bound): every buffer is sized for
    the bound, the tables are laid out for the live count, no tile order"""
    dev = _dev(indices)
    indices = _c(indices, torch.int32)
    N = indices.shape[0]
    cap = max(27 * N, 1)
    src = torch.empty((cap,), dtype=torch.int32, device=dev)
    dst = torch.empty((cap,), dtype=torch.int32, device=dev)
    toff = torch.empty((27, n_tiles(N) + 1), dtype=torch.int32, device=dev)
    npairs = torch.empty((1,), dtype=torch.int64, device=dev)  # (always written by the library)
    L = _C.lib()
    ws = _ws(L.gpn_rulebook_subm3_ws_bytes(i64(N)), dev)
    nbr = torch.empty((27 * N + 1,), dtype=torch.int32, device=dev)
    if rows is not None:
        check(L.gpn_rulebook_subm3_dev(ptr(indices), i64(N), *rows.args(), host_i32x3(spatial_shape), ptr(nbr), ptr(src), ptr(dst),
                                       ptr(toff), ptr(npairs), ptr(ws), szt(ws.numel()), _stream()), "gpn_rulebook_subm3_dev")
        return Rulebook(src, dst, toff, 27, N, N, npairs[0], nbr, live_src=rows, live_dst=rows)
    check(L.gpn_rulebook_subm3(ptr(indices), i64(N), host_i32x3(spatial_shape), ptr(nbr), ptr(src), ptr(dst), ptr(toff),
                               ptr(npairs), ptr(ws), szt(ws.numel()), _stream()), "gpn_rulebook_subm3")
    return _with_tile_order(Rulebook(src, dst, toff, 27, N, N, npairs[0], nbr))


import os as _os
# Rows re-ordered by neighbour mask (gpn_rulebook_tile_order) for the masked-tile conv kernel (csrc/spconv_tiles.hip): a
# tile executes a tap as soon as ANY of its rows has that neighbour.  In voxel order a level-0 tile of the bench scenes runs
# 4.3x the MFMA row-slots of its useful pairs, sorted by mask inside 16384-row blocks 2.1x (levels 1 / 2: 2.2x / 2.0x ->
# 1.4x; stride-2 convs 4.4x -> 1.3x, inverse convs 4.3x -> 1.0x; tools/conv_tiles_bench.py).  The order costs a block-local sort (one workgroup per 16384 rows)
# and a permuted table per rulebook; levels below TILE_ORDER_MIN_ROWS rows keep voxel order (below 4096 tiles a level runs on
# the masked tap-split kernel, which reads either order).
# (round 4: also level 2 of the bench - 25k rows, direct / split kernel through `perm`: 8.17 / 8.23 / 8.14 -> 8.10 / 8.10 / 8.09 ms
# per step in three interleaved same-box runs, profiles/r04_findings.md; 4096 gave nothing more)
TILE_ORDER_MIN_ROWS = 16384  # (module attributes: tests and tools set them to order small inputs)
TILE_ORDER_BLOCK = 16384


def _with_tile_order(rb: "Rulebook") -> "Rulebook":
    if rb.nbr is not None and rb.n_dst >= TILE_ORDER_MIN_ROWS:
        rb.perm, rb.nbr_p = tile_order(rb.nbr, rb.K, rb.n_dst)
    return rb


def tile_order(nbr, K, n):
    """-> (perm [ceil(n/16)*16 + 16] i32, nbr_p [K*n + 1] i32): rows of every 16384-row block sorted by neighbour mask"""
    dev = nbr.device
    L = _C.lib()
    perm = torch.empty(((n + 15) // 16 * 16 + 16,), dtype=torch.int32, device=dev)
    nbr_p = torch.empty((K * n + 1,), dtype=torch.int32, device=dev)
    ws = _ws(L.gpn_rulebook_tile_order_ws_bytes(i64(n)), dev)
    check(L.gpn_rulebook_tile_order(ptr(nbr), i32(K), i64(n), i32(TILE_ORDER_BLOCK), ptr(perm), ptr(nbr_p), ptr(ws),
                                    szt(ws.numel()), _stream()), "gpn_rulebook_tile_order")
    return perm, nbr_p




def rulebook_identity(n, device, rows_dev: Optional[DevCount] = None) -> Rulebook:
    """the K = 1 rulebook over ``n`` rows (SubMConv3d(k=1), linear layers on the conv kernels) in one launch; ``rows_dev``: n is
    a bound, the live count a device counter"""
    rows = torch.empty((max(n, 1),), dtype=torch.int32, device=device)[:n]
    tile_off = torch.empty((1, n_tiles(n) + 1), dtype=torch.int32, device=device)
    nbr = torch.empty((n + 1,), dtype=torch.int32, device=device)
    npairs = torch.empty((1,), dtype=torch.int64, device=device)
    if rows_dev is not None:
        check(_C.lib().gpn_rulebook_identity_dev(i64(n), *rows_dev.args(), ptr(rows), ptr(tile_off), ptr(nbr), ptr(npairs), _stream()),
              "gpn_rulebook_identity_dev")
        return Rulebook(rows, rows, tile_off, 1, n, n, npairs[0], nbr, live_src=rows_dev, live_dst=rows_dev)
    check(_C.lib().gpn_rulebook_identity(i64(n), ptr(rows if n > 0 else nbr), ptr(tile_off), ptr(nbr), ptr(npairs), _stream()),
          "gpn_rulebook_identity")
    return Rulebook(rows, rows, tile_off, 1, n, n, npairs[0], nbr)


def rulebook_level_counts(indices, spatial_shape, batch_size, n_levels):
    """-> device tensor [n_levels] i64: rows of each of the next ``n_levels`` stride-2 levels below ``indices`` (what the
    successive rulebook_down calls would report), so that a caller can fetch them all with ONE host read."""
    dev = _dev(indices)
    indices = _c(indices, torch.int32)
    N = indices.shape[0]
    counts = torch.empty((n_levels,), dtype=torch.int64, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_rulebook_level_counts_ws_bytes(i64(N), i32(n_levels)), dev)
    check(L.gpn_rulebook_level_counts(ptr(indices), i64(N), ptr(None), i64(batch_size), host_i32x3(spatial_shape), i32(n_levels),
                                      ptr(counts), ptr(ws), szt(ws.numel()), _stream()), "gpn_rulebook_level_counts")
    return counts


def rulebook_down(indices, spatial_shape, batch_size, n_out=None):
    """Returns (out_indices [No,4] i32, out_shape, rb_fwd (dst=coarse), rb_bwd (dst=fine)).  One host sync, none when the
    caller already knows the coarse row count ``n_out`` (rulebook_level_counts / the proposal stage's counts)."""
    dev = _dev(indices)
    indices = _c(indices, torch.int32)
    N = indices.shape[0]
    out_idx = torch.empty((max(N, 1), 4), dtype=torch.int32, device=dev)
    f2c = torch.empty((max(N, 1),), dtype=torch.int32, device=dev)
    tap = torch.empty((max(N, 1),), dtype=torch.int32, device=dev)
    nout = torch.empty((1,), dtype=torch.int64, device=dev)  # (always written by the library)
    L = _C.lib()
    ws = _ws(L.gpn_rulebook_down_ws_bytes(i64(N)), dev)
    check(L.gpn_rulebook_down(ptr(indices), i64(N), i64(batch_size), host_i32x3(spatial_shape), ptr(out_idx),
                              ptr(f2c), ptr(tap), ptr(nout), ptr(ws), szt(ws.numel()), _stream()),
          "gpn_rulebook_down")
    No = int(nout.item()) if n_out is None else int(n_out)
    cap = max(N, 1)
    fs = torch.empty((cap,), dtype=torch.int32, device=dev)
    fd = torch.empty((cap,), dtype=torch.int32, device=dev)
    bs = torch.empty((cap,), dtype=torch.int32, device=dev)
    bd = torch.empty((cap,), dtype=torch.int32, device=dev)
    ft = torch.empty((8, n_tiles(No) + 1), dtype=torch.int32, device=dev)
    bt = torch.empty((8, n_tiles(N) + 1), dtype=torch.int32, device=dev)
    npairs = torch.empty((1,), dtype=torch.int64, device=dev)  # (always written by the library)
    ws = _ws(L.gpn_rulebook_down_lists_ws_bytes(i64(N), i64(No)), dev)
    fn = torch.empty((8 * No + 1,), dtype=torch.int32, device=dev)
    bn = torch.empty((8 * N + 1,), dtype=torch.int32, device=dev)
    check(L.gpn_rulebook_down_lists(ptr(f2c), ptr(tap), i64(N), i64(No), ptr(fn), ptr(fs), ptr(fd), ptr(ft), ptr(bn),
                                    ptr(bs), ptr(bd), ptr(bt), ptr(npairs), ptr(ws), szt(ws.numel()), _stream()),
          "gpn_rulebook_down_lists")
    out_shape = [int(s) // 2 for s in spatial_shape]
    rb_fwd = Rulebook(fs, fd, ft, 8, N, No, npairs[0], fn)  # (dst = coarse: 1-8 children per row, the order buys nothing: 10.7 -> 10 us)
    rb_bwd = _with_tile_order(Rulebook(bs, bd, bt, 8, No, N, npairs[0], bn))  # dst = fine: one tap per row, 4.3x -> 1.0x slots
    return out_idx[:No], out_shape, rb_fwd, rb_bwd


def rulebook_down_dev(indices, spatial_shape, batch_size, rows: DevCount, batch: Optional[DevCount], out_plan: int = 0):
    """rulebook_down with the fine row count (and optionally the number of batch entries - the proposals of a step) on the
    device: no host read.  ``indices.shape[0]`` / ``batch_size`` are bounds.  -> (out_indices [bound,4], out_shape, rb_fwd,
    rb_bwd, coarse rows as a DevCount with plan ``out_plan``)"""
    dev = _dev(indices)
    indices = _c(indices, torch.int32)
    N = indices.shape[0]
    out_idx = torch.empty((N, 4), dtype=torch.int32, device=dev)
    f2c = torch.empty((N,), dtype=torch.int32, device=dev)
    tap = torch.empty((N,), dtype=torch.int32, device=dev)
    nout = torch.empty((1,), dtype=torch.int64, device=dev)
    L = _C.lib()
    shape = host_i32x3(spatial_shape)
    ws = _ws(L.gpn_rulebook_down_dev_ws_bytes(i64(N), i64(batch_size), shape), dev)
    b_ptr, b_plan = batch.args() if batch is not None else (_C.ctypes.c_void_p(0), _C.ctypes.c_int64(0))
    check(L.gpn_rulebook_down_dev(ptr(indices), i64(N), *rows.args(), i64(batch_size), b_ptr, b_plan, shape, ptr(out_idx), ptr(f2c),
                                  ptr(tap), ptr(nout), ptr(ws), szt(ws.numel()), _stream()), "gpn_rulebook_down_dev")
    out_rows = DevCount(nout, out_plan)
    No = N  # bound of the coarse level
    fs = torch.empty((N,), dtype=torch.int32, device=dev)
    fd = torch.empty((N,), dtype=torch.int32, device=dev)
    bs = torch.empty((N,), dtype=torch.int32, device=dev)
    bd = torch.empty((N,), dtype=torch.int32, device=dev)
    ft = torch.empty((8, n_tiles(No) + 1), dtype=torch.int32, device=dev)
    bt = torch.empty((8, n_tiles(N) + 1), dtype=torch.int32, device=dev)
    npairs = torch.empty((1,), dtype=torch.int64, device=dev)
    ws = _ws(L.gpn_rulebook_down_lists_ws_bytes(i64(N), i64(No)), dev)
    fn = torch.empty((8 * No + 1,), dtype=torch.int32, device=dev)
    bn = torch.empty((8 * N + 1,), dtype=torch.int32, device=dev)
    check(L.gpn_rulebook_down_lists_dev(ptr(f2c), ptr(tap), i64(N), *rows.args(), i64(No), *out_rows.args(), ptr(fn), ptr(fs), ptr(fd),
                                        ptr(ft), ptr(bn), ptr(bs), ptr(bd), ptr(bt), ptr(npairs), ptr(ws), szt(ws.numel()), _stream()),
          "gpn_rulebook_down_lists_dev")
    out_shape = [int(s) // 2 for s in spatial_shape]
    rb_fwd = Rulebook(fs, fd, ft, 8, N, No, npairs[0], fn, live_src=rows, live_dst=out_rows)
    rb_bwd = Rulebook(bs, bd, bt, 8, No, N, npairs[0], bn, live_src=out_rows, live_dst=rows)
    return out_idx, out_shape, rb_fwd, rb_bwd, out_rows


# ---------------------------------------------------------------------------------------------------- C
LAYOUT_OKI = 4
WGRAD_MAX_COUT = 128  # widest dout gpn_spconv_wgrad contracts in one call


def _wdims(W, layout):
    """(K, cin, cout) of a weight given as canonical [K, Cin, Cout] ("kio") or parameter layout [Cout, K, Cin] ("oki")"""
    if layout == "oki":
        return W.shape[1], W.shape[2], W.shape[0]
    return W.shape[0], W.shape[1], W.shape[2]


def pack_weights(W, flags, layout="kio"):
    dev = _dev(W)
    W = _c(W, torch.float32)
    K, cin, cout = _wdims(W, layout)
    packed = torch.empty((K * cin * cout,), dtype=torch.float32, device=dev)
    if layout == "oki":
        flags |= LAYOUT_OKI
    check(_C.lib().gpn_spconv_pack_weights(ptr(W), i32(K), i32(cin), i32(cout), i32(flags), ptr(packed), _stream()),
          "gpn_spconv_pack_weights")
    return packed


def _conv_packed(features, packed, rb: Rulebook, cin, cout):
    dev = _dev(features)
    features = _c(features, torch.float32)
    assert features.shape[0] == rb.n_src and features.shape[1] == cin, (features.shape, rb.n_src, cin)
    out = torch.empty((rb.n_dst, cout), dtype=torch.float32, device=dev)
    L = _C.lib()
    ws_bytes = L.gpn_spconv_fwd_ws_bytes(i32(rb.K), i64(rb.n_dst), i32(cin), i32(cout))
    ws = _ws(ws_bytes, dev) if ws_bytes else None
    check(L.gpn_spconv_fwd(ptr(features), ptr(packed), ptr(rb.nbr), i32(rb.K), i64(rb.n_dst), i32(cin), i32(cout),
                           ptr(out), ptr(ws), szt(ws.numel() if ws is not None else 0), _stream()), "gpn_spconv_fwd")
    return out


_FAST_WS = {}


def _fast_ws(device, need=0):
    """(pointer, bytes) of the shared per-(device, stream) scratch buffer, grown on demand (see _ws)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    stream = torch._C._cuda_getCurrentRawStream(idx)
    key = (idx, stream)
    ent = _FAST_WS.get(key)
    if ent is None or ent[1] < need:
        size = max(int(need) * 2, 256 << 20)
        buf = torch.empty((size,), dtype=torch.uint8, device=device)
        ent = (buf.data_ptr(), size, buf)
        _FAST_WS[key] = ent
    return ent[0], ent[1], stream


def _raise(what):
    raise _C.GpnError(f"{what} failed: {_C.lib().gpn_last_error().decode('utf-8', 'replace')}")


def _conv_w(features, W, layout, flags, rb: Rulebook, cin_op, cout_op):
    """pack + fused conv in one library call; features must be contiguous fp32 on the GPU (autograd wrappers ensure it)"""
    if not features.is_cuda:
        _dev(features)
    K, cin_w, cout_w = _wdims(W, layout)
    assert features.shape[0] == rb.n_src and features.shape[1] == cin_op, (features.shape, rb.n_src, cin_op)
    L = _C.lib()
    out = torch.empty((rb.n_dst, cout_op), dtype=torch.float32, device=features.device)
    if layout == "oki":
        flags |= LAYOUT_OKI
    ws_ptr, ws_size, stream = _fast_ws(features.device)
    rc = L.gpn_spconv_fwd_w(features.data_ptr(), W.data_ptr(), K, cin_w, cout_w, flags, rb.nbr.data_ptr(), rb.n_dst,
                            out.data_ptr(), ws_ptr, ws_size, stream)
    if rc == 2:  # workspace too small: grow once and retry
        ws_ptr, ws_size, stream = _fast_ws(features.device, L.gpn_spconv_fwd_w_ws_bytes(K, rb.n_dst, cin_op, cout_op))
        rc = L.gpn_spconv_fwd_w(features.data_ptr(), W.data_ptr(), K, cin_w, cout_w, flags, rb.nbr.data_ptr(), rb.n_dst,
                                out.data_ptr(), ws_ptr, ws_size, stream)
    if rc:
        _raise("gpn_spconv_fwd_w")
    return out


def conv_fwd_ordered(features, W, rb: Rulebook, flags=0):
    """conv over ``rb`` through gpn_spconv_fwd_ordered: uses the rulebook's tile order (nbr_p / perm) when it has one.
    ``W`` canonical [K, Cin, Cout]; ``flags`` = PACK_TRANSPOSE | PACK_REVERSE turns the call into the dgrad of a SubM conv
    (features = dout).  What the network executor does per layer; the per-layer autograd path (conv_fwd) passes the plain
    table only."""
    dev = _dev(features)
    features = _c(features, torch.float32)
    K, cin_w, cout_w = W.shape
    cin, cout = (cout_w, cin_w) if flags & PACK_TRANSPOSE else (cin_w, cout_w)
    assert features.shape == (rb.n_src, cin), (features.shape, rb.n_src, cin)
    packed = pack_weights(W, flags)
    out = torch.empty((rb.n_dst, cout), dtype=torch.float32, device=dev)
    L = _C.lib()
    ws_bytes = L.gpn_spconv_fwd_ws_bytes(i32(K), i64(rb.n_dst), i32(cin), i32(cout))
    ws = _ws(ws_bytes, dev) if ws_bytes else None
    check(L.gpn_spconv_fwd_ordered(ptr(features), ptr(packed), ptr(rb.nbr), ptr(rb.nbr_p), ptr(rb.perm), i32(K), i64(rb.n_dst),
                                   i32(cin), i32(cout), ptr(out), ptr(ws), szt(ws.numel() if ws is not None else 0), _stream()),
          "gpn_spconv_fwd_ordered")
    return out


def conv_fwd(features, W, rb: Rulebook, layout="kio"):
    """out[dst] = sum_k in[src] @ W[k];  channel counts multiples of 16."""
    K, cin, cout = _wdims(W, layout)
    return _conv_w(features, W, layout, 0, rb, cin, cout)


def conv_dgrad(dout, W, rb: Rulebook, rb_t: Rulebook, reverse_taps: bool, layout="kio"):
    """din[src] = sum_k dout[dst] @ W[k]^T, computed as a forward conv over the transposed rulebook rb_t."""
    K, cin, cout = _wdims(W, layout)
    return _conv_w(dout, W, layout, PACK_TRANSPOSE | (PACK_REVERSE if reverse_taps else 0), rb_t, cout, cin)


def conv_wgrad(features, dout, rb: Rulebook, layout="kio"):
    """weight gradient in the same layout as the weight was given ("kio": [K,Cin,Cout]; "oki": [Cout,K,Cin])"""
    if not (features.is_cuda and dout.is_cuda):
        _dev(features, dout)
    cin, cout = features.shape[1], dout.shape[1]
    shape = (cout, rb.K, cin) if layout == "oki" else (rb.K, cin, cout)
    if cout > WGRAD_MAX_COUT:
        # the contraction takes at most 128 output columns (gpn_spconv_wgrad, include/gpn.h): balanced pieces of <= 128 columns
        # of dout, each piece's gradient copied into its columns ("kio") / rows ("oki") of dW
        nt = cout // 16
        n = -(-nt // (WGRAD_MAX_COUT // 16))
        dW = torch.empty(shape, dtype=torch.float32, device=features.device)
        c0 = 0
        for i in range(n):
            c1 = c0 + 16 * (nt // n + (1 if i < nt % n else 0))
            piece = conv_wgrad(features, dout[:, c0:c1].contiguous(), rb, layout)
            if layout == "oki":
                dW[c0:c1].copy_(piece)
            else:
                dW[:, :, c0:c1].copy_(piece)
            c0 = c1
        return dW
    dW = torch.empty(shape, dtype=torch.float32, device=features.device)
    L = _C.lib()
    ws_ptr, ws_size, stream = _fast_ws(features.device, 0)
    args = (features.data_ptr(), dout.data_ptr(), rb.pair_src.data_ptr(), rb.pair_dst.data_ptr(), rb.tile_off.data_ptr(),
            rb.K, rb.n_dst, cin, cout, LAYOUT_OKI if layout == "oki" else 0, dW.data_ptr())
    rc = L.gpn_spconv_wgrad(*args, ws_ptr, ws_size, stream)
    if rc == 2:
        ws_ptr, ws_size, stream = _fast_ws(features.device, L.gpn_spconv_wgrad_ws_bytes(i32(rb.K), i32(cin), i32(cout), i64(rb.n_dst)))
        rc = L.gpn_spconv_wgrad(*args, ws_ptr, ws_size, stream)
    if rc:
        _raise("gpn_spconv_wgrad")
    return dW


# ---------------------------------------------------------------------------------------------------- P
def point_losses_fwd(logits, labels, offsets, gt_offsets, instance_labels, ignore_index, metrics=False):
    """-> (losses [4] f32 = focal, dice, offset distance, offset direction; stats = opaque device block for the backward);
    ``metrics``: also (preds [M] i64 = argmax of the logits, accu [2] f32 = point accuracy over all points / over the points
    on a part) from the same pass (gpn_point_losses_fwd_metrics)"""
    dev = _dev(logits, offsets)
    logits, offsets, gt_offsets = _c(logits, torch.float32), _c(offsets, torch.float32), _c(gt_offsets, torch.float32)
    labels, instance_labels = _c(labels, torch.int64), _c(instance_labels, torch.int32)
    M, C = logits.shape
    losses = torch.empty((4,), dtype=torch.float32, device=dev)
    stats = torch.empty((4,), dtype=torch.float64, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_point_losses_ws_bytes(i64(M)), dev)
    if metrics:
        preds = torch.empty((M,), dtype=torch.int64, device=dev)
        accu = torch.empty((2,), dtype=torch.float32, device=dev)
        check(L.gpn_point_losses_fwd_metrics(ptr(logits), ptr(labels), ptr(offsets), ptr(gt_offsets), ptr(instance_labels), i64(M),
                                             i32(C), i64(ignore_index), ptr(losses), ptr(preds), ptr(accu), ptr(stats), ptr(ws),
                                             szt(ws.numel()), _stream()), "gpn_point_losses_fwd_metrics")
        return losses, stats, preds, accu
    check(L.gpn_point_losses_fwd(ptr(logits), ptr(labels), ptr(offsets), ptr(gt_offsets), ptr(instance_labels), i64(M),
                                 i32(C), i64(ignore_index), ptr(losses), ptr(stats), ptr(ws), szt(ws.numel()), _stream()),
          "gpn_point_losses_fwd")
    return losses, stats


def point_losses_bwd(logits, labels, offsets, gt_offsets, instance_labels, ignore_index, stats, grad_losses):
    dev = _dev(logits, offsets)
    M, C = logits.shape
    d_logits = torch.empty((M, C), dtype=torch.float32, device=dev)
    d_offsets = torch.empty((M, 3), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_point_losses_bwd(ptr(logits), ptr(labels), ptr(offsets), ptr(gt_offsets), ptr(instance_labels),
                                        i64(M), i32(C), i64(ignore_index), ptr(stats), ptr(_c(grad_losses, torch.float32)),
                                        ptr(d_logits), ptr(d_offsets), _stream()), "gpn_point_losses_bwd")
    return d_logits, d_offsets


# ---------------------------------------------------------------------------------------------------- BN
def _p(t):
    return None if t is None else t.data_ptr()


def bn_fwd(x, res, weight, bias, running_mean, running_var, training, momentum, eps, relu):
    """fused BatchNorm1d(+residual)(+ReLU) forward -> (y, mean, invstd); running stats updated in place when training.
    x / res must be contiguous fp32 (the autograd wrapper ensures it)."""
    if not x.is_cuda:
        _dev(x)
    N, C = x.shape
    y = torch.empty_like(x)
    L = _C.lib()
    if training:
        stats = torch.empty((2, C), dtype=torch.float32, device=x.device)
        mean, invstd = stats[0], stats[1]
        ws_ptr, ws_size, stream = _fast_ws(x.device, 0)
        rc = L.gpn_bn_fwd_train(x.data_ptr(), _p(res), weight.data_ptr(), bias.data_ptr(), N, C, eps, momentum,
                                1 if relu else 0, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _p(running_mean),
                                _p(running_var), ws_ptr, ws_size, stream)
        if rc:
            _raise("gpn_bn_fwd_train")
    else:
        mean = running_mean
        invstd = 1.0 / torch.sqrt(running_var + eps)
        rc = L.gpn_bn_fwd_eval(x.data_ptr(), _p(res), weight.data_ptr(), bias.data_ptr(), mean.data_ptr(),
                               invstd.data_ptr(), N, C, 1 if relu else 0, y.data_ptr(),
                               torch._C._cuda_getCurrentRawStream(x.device.index))
        if rc:
            _raise("gpn_bn_fwd_eval")
    return y, mean, invstd


def bn_bwd(x, y, dy, weight, mean, invstd, relu, training, has_res):
    """-> (dx, dres or None, dweight, dbias)"""
    if not x.is_cuda:
        _dev(x)
    N, C = x.shape
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if has_res else None
    dwb = torch.empty((2, C), dtype=torch.float32, device=x.device)
    dw, db = dwb[0], dwb[1]
    ws_ptr, ws_size, stream = _fast_ws(x.device, 0)
    rc = _C.lib().gpn_bn_bwd(x.data_ptr(), y.data_ptr(), dy.data_ptr(), weight.data_ptr(), mean.data_ptr(),
                             invstd.data_ptr(), N, C, 1 if relu else 0, 1 if training else 0, dx.data_ptr(), _p(dres),
                             dw.data_ptr(), db.data_ptr(), ws_ptr, ws_size, stream)
    if rc:
        _raise("gpn_bn_bwd")
    return dx, dres, dw, db


# ---------------------------------------------------------------------------------------------------- G
def gather_rows(table, idx, rows: Optional[DevCount] = None):
    dev = _dev(table, idx)
    table, idx = _c(table, torch.float32), _c(idx, torch.int32)
    out = torch.empty((idx.shape[0], table.shape[1]), dtype=torch.float32, device=dev)
    if rows is not None:  # the live length of idx is a device counter (rows of `out` past it stay unwritten)
        check(_C.lib().gpn_gather_rows_dev(ptr(table), ptr(idx), i64(idx.shape[0]), *rows.args(), i32(table.shape[1]), ptr(out),
                                           _stream()), "gpn_gather_rows_dev")
        return out
    check(_C.lib().gpn_gather_rows(ptr(table), ptr(idx), i64(idx.shape[0]), i32(table.shape[1]), ptr(out), _stream()),
          "gpn_gather_rows")
    return out


def rows_csr(idx, n_rows):
    """CSR of positions grouped by row id (stable): (order [n] i32 with idx<0 entries last, starts [n_rows+1] i32)."""
    idx = idx.to(torch.int64)
    key = torch.where(idx >= 0, idx, torch.full_like(idx, n_rows))
    _, order = torch.sort(key, stable=True)
    counts = torch.bincount(key, minlength=n_rows + 1)[:n_rows]
    starts = torch.zeros((n_rows + 1,), dtype=torch.int32, device=idx.device)
    starts[1:] = counts.cumsum(0).to(torch.int32)
    return order.to(torch.int32), starts


def scatter_rows(dout, idx, n_rows, csr=None, rows: Optional[DevCount] = None):
    """transpose of gather_rows: dtable[r] = ordered sum of dout[i] over idx[i] == r.  ``rows``: the live number of table rows
    is a device counter (n_rows = its bound; needs ``csr``)."""
    dev = _dev(dout, idx)
    dout = _c(dout, torch.float32)
    order, starts = csr if csr is not None else rows_csr(idx, n_rows)
    out = torch.empty((n_rows, dout.shape[1]), dtype=torch.float32, device=dev)
    if rows is not None:
        assert csr is not None, "a device-counted scatter needs the caller's CSR"
        check(_C.lib().gpn_scatter_rows_csr_dev(ptr(dout), ptr(_c(order, torch.int32)), ptr(_c(starts, torch.int32)), i64(n_rows),
                                                *rows.args(), i32(dout.shape[1]), ptr(out), _stream()), "gpn_scatter_rows_csr_dev")
        return out
    check(_C.lib().gpn_scatter_rows_csr(ptr(dout), ptr(_c(order, torch.int32)), ptr(_c(starts, torch.int32)),
                                        i64(n_rows), i32(dout.shape[1]), ptr(out), _stream()),
          "gpn_scatter_rows_csr")
    return out


# ---------------------------------------------------------------------------------------------------- B/L
def ball_query(points, query, batch_indices, batch_offsets, radius, num_samples, point_labels=None,
               query_labels=None):
    dev = _dev(points, query)
    points, query = _c(points, torch.float32), _c(query, torch.float32)
    bi, bo = _c(batch_indices, torch.int32), _c(batch_offsets, torch.int32)
    pl, ql = _c(point_labels, torch.int32), _c(query_labels, torch.int32)
    Q, K = query.shape[0], int(num_samples)
    idx = torch.empty((Q, K), dtype=torch.int32, device=dev)
    cnt = torch.zeros((Q,), dtype=torch.int32, device=dev)
    L = _C.lib()
    Np = points.shape[0]
    if Np >= 2048 and radius > 0:  # grid-accelerated form (identical results); tiny inputs: the plain scan is one launch
        ws = _ws(L.gpn_ball_query_grid_ws_bytes(i64(Np)), dev)
        check(L.gpn_ball_query_grid(ptr(points), ptr(query), ptr(bi), ptr(bo), ptr(pl), ptr(ql), i64(Np), i64(Q),
                                    i64(bo.shape[0] - 1), f32(radius), i32(K), ptr(idx), ptr(cnt), ptr(ws),
                                    szt(ws.numel()), _stream()), "gpn_ball_query_grid")
        return idx, cnt
    check(L.gpn_ball_query(ptr(points), ptr(query), ptr(bi), ptr(bo), ptr(pl), ptr(ql), i64(Np),
                           i64(Q), i64(bo.shape[0] - 1), f32(radius), i32(K), ptr(idx), ptr(cnt), _stream()),
          "gpn_ball_query")
    return idx, cnt


def ccl(begin_end, edges, compacted=False):
    dev = _dev(begin_end, edges)
    be, edges = _c(begin_end, torch.int32), _c(edges, torch.int32)
    Q = be.shape[0] // 2
    labels = torch.empty((Q,), dtype=torch.int32, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_ccl_ws_bytes(i64(Q)), dev)
    check(L.gpn_ccl(ptr(be), ptr(edges), i64(Q), i64(edges.shape[0]), i32(1 if compacted else 0), ptr(labels),
                    ptr(ws), szt(ws.numel()), _stream()), "gpn_ccl")
    return labels


# ---------------------------------------------------------------------------------------------------- R/I/N
_MODES = {"sum": 0, "min": 1, "max": 2}


def segmented_reduce(values, begin, end, mode):
    dev = _dev(values, begin, end)
    values, begin, end = _c(values, torch.float32), _c(begin, torch.int32), _c(end, torch.int32)
    P, C = begin.shape[0], values.shape[1]
    out = torch.empty((P, C), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_segmented_reduce(ptr(values), ptr(begin), ptr(end), i64(P), i32(C), i32(_MODES[mode]), ptr(out),
                                        _stream()), "gpn_segmented_reduce")
    return out


def segmented_maxpool_fwd(values, begin, end, rows: Optional[DevCount] = None):
    dev = _dev(values, begin, end)
    values, begin, end = _c(values, torch.float32), _c(begin, torch.int32), _c(end, torch.int32)
    P, C = begin.shape[0], values.shape[1]
    pooled = torch.empty((P, C), dtype=torch.float32, device=dev)
    arg = torch.empty((P, C), dtype=torch.int32, device=dev)
    if rows is not None:  # the number of segments is a device counter (P = its bound)
        check(_C.lib().gpn_segmented_maxpool_fwd_dev(ptr(values), ptr(begin), ptr(end), i64(P), *rows.args(), i32(C), ptr(pooled),
                                                     ptr(arg), _stream()), "gpn_segmented_maxpool_fwd_dev")
        return pooled, arg
    check(_C.lib().gpn_segmented_maxpool_fwd(ptr(values), ptr(begin), ptr(end), i64(P), i32(C), ptr(pooled), ptr(arg),
                                             _stream()), "gpn_segmented_maxpool_fwd")
    return pooled, arg


def segmented_maxpool_bwd(dpooled, argmax, M, rows: Optional[DevCount] = None, m_rows: Optional[DevCount] = None):
    dev = _dev(dpooled, argmax)
    dpooled, argmax = _c(dpooled, torch.float32), _c(argmax, torch.int32)
    P, C = dpooled.shape
    dv = torch.empty((M, C), dtype=torch.float32, device=dev)
    if rows is not None:
        check(_C.lib().gpn_segmented_maxpool_bwd_dev(ptr(dpooled), ptr(argmax), i64(P), *rows.args(), i32(C), i64(M), *m_rows.args(),
                                                     ptr(dv), _stream()), "gpn_segmented_maxpool_bwd_dev")
        return dv
    check(_C.lib().gpn_segmented_maxpool_bwd(ptr(dpooled), ptr(argmax), i64(P), i32(C), i64(M), ptr(dv), _stream()),
          "gpn_segmented_maxpool_bwd")
    return dv


def instance_iou(proposal_offsets, instance_labels, batch_indices, num_points_per_instance, rows: Optional[DevCount] = None):
    dev = _dev(proposal_offsets, instance_labels, batch_indices, num_points_per_instance)
    po, il = _c(proposal_offsets, torch.int32), _c(instance_labels, torch.int32)
    bi, npi = _c(batch_indices, torch.int32), _c(num_points_per_instance, torch.int32)
    P, (B, I) = po.shape[0] - 1, npi.shape
    if rows is not None:  # the proposal count is a device counter (P = its bound; rows past it stay unwritten)
        out = torch.empty((P, I), dtype=torch.float32, device=dev)
        check(_C.lib().gpn_instance_iou_dev(ptr(po), ptr(il), ptr(bi), ptr(npi), i64(P), *rows.args(), i64(B), i32(I), ptr(out),
                                            _stream()), "gpn_instance_iou_dev")
        return out
    out = torch.zeros((P, I), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_instance_iou(ptr(po), ptr(il), ptr(bi), ptr(npi), i64(P), i64(B), i32(I), ptr(out), _stream()),
          "gpn_instance_iou")
    return out


def nms(ious, scores, threshold):
    dev = _dev(ious, scores)
    ious, scores = _c(ious, torch.float32), _c(scores, torch.float32)
    P = scores.shape[0]
    order = torch.sort(scores, descending=True, stable=True)[1].to(torch.int32)
    keep = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
    nk = torch.zeros((1,), dtype=torch.int32, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_nms_ws_bytes(i64(P)), dev)
    check(L.gpn_nms(ptr(ious), ptr(order), i64(P), f32(threshold), ptr(keep), ptr(nk), ptr(ws), szt(ws.numel()),
                    _stream()), "gpn_nms")
    return keep[: int(nk.item())].to(torch.int64)


# ---------------------------------------------------------------------------------------------------- F
def pn2_ball_query(radius, nsample, xyz, new_xyz):
    dev = _dev(xyz, new_xyz)
    xyz, new_xyz = _c(xyz, torch.float32), _c(new_xyz, torch.float32)
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.zeros((b, m, nsample), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_pn2_ball_query(i32(b), i32(n), i32(m), f32(radius), i32(nsample), ptr(new_xyz), ptr(xyz),
                                      ptr(idx), _stream()), "gpn_pn2_ball_query")
    return idx


def pn2_group_points(points, idx):
    dev = _dev(points, idx)
    points, idx = _c(points, torch.float32), _c(idx, torch.int32)
    b, c, n = points.shape
    _, npts, ns = idx.shape
    out = torch.empty((b, c, npts, ns), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_pn2_group_points(i32(b), i32(c), i32(n), i32(npts), i32(ns), ptr(points), ptr(idx), ptr(out),
                                        _stream()), "gpn_pn2_group_points")
    return out


def pn2_group_points_grad(grad_out, idx, n):
    dev = _dev(grad_out, idx)
    grad_out, idx = _c(grad_out, torch.float32), _c(idx, torch.int32)
    b, c, npts, ns = grad_out.shape
    gp = torch.zeros((b, c, n), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_pn2_group_points_grad(i32(b), i32(c), i32(n), i32(npts), i32(ns), ptr(grad_out), ptr(idx),
                                             ptr(gp), _stream()), "gpn_pn2_group_points_grad")
    return gp


def pn2_gather_points(points, idx):
    dev = _dev(points, idx)
    points, idx = _c(points, torch.float32), _c(idx, torch.int32)
    b, c, n = points.shape
    m = idx.shape[1]
    out = torch.empty((b, c, m), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_pn2_gather_points(i32(b), i32(c), i32(n), i32(m), ptr(points), ptr(idx), ptr(out), _stream()),
          "gpn_pn2_gather_points")
    return out


def pn2_gather_points_grad(grad_out, idx, n):
    dev = _dev(grad_out, idx)
    grad_out, idx = _c(grad_out, torch.float32), _c(idx, torch.int32)
    b, c, m = grad_out.shape
    gp = torch.zeros((b, c, n), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_pn2_gather_points_grad(i32(b), i32(c), i32(n), i32(m), ptr(grad_out), ptr(idx), ptr(gp),
                                              _stream()), "gpn_pn2_gather_points_grad")
    return gp


def pn2_furthest_point_sampling(xyz, npoint):
    dev = _dev(xyz)
    xyz = _c(xyz, torch.float32)
    b, n, _ = xyz.shape
    temp = torch.full((b, n), 1e10, dtype=torch.float32, device=dev)
    idx = torch.zeros((b, npoint), dtype=torch.int32, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_pn2_furthest_point_sampling_ws_bytes(i32(b), i32(n)), dev)  # non-empty only for clouds of >= 65536 points
    check(L.gpn_pn2_furthest_point_sampling_ws(i32(b), i32(n), i32(npoint), ptr(xyz), ptr(temp), ptr(idx), ptr(ws),
                                               szt(ws.numel()), _stream()), "gpn_pn2_furthest_point_sampling_ws")
    return idx


def pn2_three_nn(unknown, known):
    dev = _dev(unknown, known)
    unknown, known = _c(unknown, torch.float32), _c(known, torch.float32)
    b, n, _ = unknown.shape
    m = known.shape[1]
    d2 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((b, n, 3), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_pn2_three_nn(i32(b), i32(n), i32(m), ptr(unknown), ptr(known), ptr(d2), ptr(idx), _stream()),
          "gpn_pn2_three_nn")
    return d2, idx


def pn2_knn(unknown, known, k):
    dev = _dev(unknown, known)
    unknown, known = _c(unknown, torch.float32), _c(known, torch.float32)
    b, n, _ = unknown.shape
    m = known.shape[1]
    d2 = torch.empty((b, n, k), dtype=torch.float32, device=dev)
    idx = torch.empty((b, n, k), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_pn2_knn(i32(b), i32(n), i32(m), i32(k), ptr(unknown), ptr(known), ptr(d2), ptr(idx), _stream()),
          "gpn_pn2_knn")
    return d2, idx


def pn2_three_interpolate(points, idx, weight):
    dev = _dev(points, idx, weight)
    points, idx, weight = _c(points, torch.float32), _c(idx, torch.int32), _c(weight, torch.float32)
    b, c, m = points.shape
    n = idx.shape[1]
    out = torch.empty((b, c, n), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_pn2_three_interpolate(i32(b), i32(c), i32(m), i32(n), ptr(points), ptr(idx), ptr(weight),
                                             ptr(out), _stream()), "gpn_pn2_three_interpolate")
    return out


def pn2_three_interpolate_grad(grad_out, idx, weight, m):
    dev = _dev(grad_out, idx, weight)
    grad_out, idx, weight = _c(grad_out, torch.float32), _c(idx, torch.int32), _c(weight, torch.float32)
    b, c, n = grad_out.shape
    gp = torch.zeros((b, c, m), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_pn2_three_interpolate_grad(i32(b), i32(c), i32(n), i32(m), ptr(grad_out), ptr(idx),
                                                  ptr(weight), ptr(gp), _stream()), "gpn_pn2_three_interpolate_grad")
    return gp


# ---------------------------------------------------------------------------------------------------- PR
def proposals_build(points_xyz, offset_preds, sem_preds, instance_labels, batch_indices, batch_size, radius, K1, K2,
                    min_points, fullscale, max_scale, jitter, read_counts: bool = True):
    """Section PR of include/gpn.h: the whole proposal stage (model.py:228-346 of the reference) in one library call and ONE
    host read.  ``points_xyz`` = [N,3] view of the [N,6] point matrix (row stride passed through).  -> dict of tensors
    sliced to their actual sizes, or None when no proposal survives."""
    dev = _dev(points_xyz, offset_preds, sem_preds, batch_indices)
    N = int(points_xyz.shape[0])
    assert points_xyz.dtype == torch.float32 and points_xyz.stride(1) == 1 and sem_preds.dtype == torch.int64
    stride = int(points_xyz.stride(0))
    offset_preds = _c(offset_preds.detach(), torch.float32)
    sem_preds = sem_preds.contiguous()
    batch_indices = _c(batch_indices, torch.int32)
    inst = _c(instance_labels, torch.int32) if instance_labels is not None else None
    jit = torch.cat([jitter[0].reshape(3), jitter[1].reshape(3)]).to(device=dev, dtype=torch.float32).contiguous()
    L = _C.lib()
    L.gpn_proposals_max_proposals.restype = _C.ctypes.c_int64
    P_ub = int(L.gpn_proposals_max_proposals(i64(N), i32(min_points)))
    T2 = 2 * N

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)
    counts = new((8,), torch.int64)
    valid_mask = new((N,), torch.bool)
    valid_indices = new((N,), torch.int64)
    sorted_indices, point_indices, proposal_indices = new((T2,), torch.int64), new((T2,), torch.int64), new((T2,), torch.int64)
    batch_p, sem_p, inst_p = new((T2,), torch.int32), new((T2,), torch.int32), new((T2,), torch.int32)
    xyz_p = new((T2, 3), torch.float32)
    sizes, offsets = new((P_ub + 1,), torch.int64), new((P_ub + 1,), torch.int32)
    member_slot = new((T2,), torch.int32)
    coords4 = new((T2, 4), torch.int32)
    pid, order, vstart = new((T2,), torch.int32), new((T2,), torch.int32), new((T2 + 1,), torch.int32)
    ws = _ws(L.gpn_proposals_build_ws_bytes(i64(N), i64(batch_size), i32(K1), i32(K2), i32(min_points)), dev)
    check(L.gpn_proposals_build(ptr(points_xyz), i32(stride), ptr(offset_preds), ptr(sem_preds), ptr(inst), ptr(batch_indices),
                                i64(N), i64(batch_size), f32(radius), i32(K1), i32(K2), i32(min_points), f32(fullscale),
                                f32(max_scale), ptr(jit), ptr(counts), ptr(valid_mask), ptr(valid_indices), ptr(sorted_indices),
                                ptr(point_indices), ptr(proposal_indices), ptr(batch_p), ptr(xyz_p), ptr(sem_p), ptr(inst_p),
                                ptr(sizes), ptr(offsets), ptr(member_slot), ptr(coords4), ptr(pid), ptr(order), ptr(vstart),
                                ptr(ws), szt(ws.numel()), _stream()), "gpn_proposals_build")
    if not read_counts:
        # no host read: every output at its bound, the counts stay on the device (DevCount views of `counts`; section DEV of
        # include/gpn.h).  P_ub + 1 offsets, T2 = 2 N per-point rows, T2 voxel rows.
        return dict(counts=counts, Q_dev=counts[0:1], M_dev=counts[1:2], P_dev=counts[2:3], V_dev=counts[3:4],
                    coarse_dev=counts[6:7], P=P_ub, M=T2, V=T2, valid_mask=valid_mask, valid_indices=valid_indices,
                    sorted_indices=sorted_indices, point_indices=point_indices, proposal_indices=proposal_indices,
                    batch_indices=batch_p, pt_xyz=xyz_p, sem_preds=sem_p, instance_labels=inst_p if instance_labels is not None else None,
                    sizes=sizes[:P_ub], proposal_offsets=offsets, member_slot=member_slot, voxel_coords=coords4, pc_voxel_id=pid,
                    point_order=order, voxel_point_start=vstart)
    Q, M, P, V, dropped, _, coarse = counts.tolist()[:7]  # the stage's single device -> host read
    if M == 0:
        return None
    return dict(counts_host=(Q, M, P, V, dropped, coarse), Q=Q, M=M, P=P, V=V, dropped=dropped, coarse=coarse, valid_mask=valid_mask, valid_indices=valid_indices[:Q],
                sorted_indices=sorted_indices[:M], point_indices=point_indices[:M], proposal_indices=proposal_indices[:M],
                batch_indices=batch_p[:M], pt_xyz=xyz_p[:M], sem_preds=sem_p[:M],
                instance_labels=inst_p[:M] if instance_labels is not None else None, sizes=sizes[:P],
                proposal_offsets=offsets[:P + 1], member_slot=member_slot, voxel_coords=coords4[:V], pc_voxel_id=pid[:M],
                point_order=order[:M], voxel_point_start=vstart[:V + 1])


# ---------------------------------------------------------------------------------------------------- MP
def mask_tables(scene_counts, masks_per_scene, device):
    """the small tables sections MP's two calls share, from HOST lists (no device read): points per scene of the network batch
    and masks per scene -> dict(mask_scene [K] i32, scene_offsets [S+1] i64, K, S, N, W = words per mask, cap = sum over the
    masks of their scene's points: the bound of the member total)"""
    counts = [int(c) for c in scene_counts]
    per = [int(k) for k in masks_per_scene]
    if len(counts) != len(per) or any(c < 0 for c in counts) or any(k < 0 for k in per):
        raise ValueError("scene_counts and masks_per_scene are per scene and non-negative")
    scene_of = np.repeat(np.arange(len(per), dtype=np.int32), per)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dict(mask_scene=torch.from_numpy(scene_of).to(device), scene_offsets=torch.from_numpy(off).to(device), K=int(sum(per)),
                S=len(counts), N=int(off[-1]), W=(max(counts + [0]) + 63) // 64, cap=int(sum(c * k for c, k in zip(counts, per))))


def mask_pack(masks, mask_base, tables, sample_rows=None):
    """gpn_mask_pack: ``masks`` flat u8 / bool (non-zero = member), mask k = the bytes from ``mask_base[k]`` over the rows of its
    caller's cloud; ``sample_rows`` [N] i64 = row of every network point inside its cloud (None: the masks are on the network's
    points).  -> bits [K, W] int64 (the u64 words' bit patterns)."""
    dev = _dev(masks, sample_rows)
    K, W = tables["K"], tables["W"]
    bits = torch.empty((K, W), dtype=torch.int64, device=dev)
    if K == 0 or W == 0:
        return bits
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    assert masks.dtype == torch.uint8 and masks.dim() == 1 and masks.is_contiguous()
    base = torch.as_tensor(mask_base, dtype=torch.int64).to(dev).contiguous()
    assert base.shape == (K,)
    rows = _c(sample_rows, torch.int64)
    assert rows is None or rows.shape == (tables["N"],)
    check(_C.lib().gpn_mask_pack(ptr(masks), ptr(base), ptr(tables["mask_scene"]), ptr(tables["scene_offsets"]), ptr(rows), i64(K), i64(W),
                                 ptr(bits), _stream()), "gpn_mask_pack")
    return bits


def proposals_from_masks(bits, tables, mask_label, points_xyz, n_classes, min_points, fullscale, max_scale, jitter, M_cap=None,
                         _new=None):
    """Section MP of include/gpn.h: bit sets of caller-supplied masks -> the proposal stage's tables, the re-voxelisation included, in
    one library call and ONE host read (the counts).  Same dict as ``proposals_build`` without ``member_slot`` (a point may sit in
    any number of masks) and with ``proposal_mask`` [P] i64 = position of every proposal in the caller's mask list; None when no mask
    is kept.  Raises on a mask whose label lies outside [1, n_classes) and when the members exceed ``M_cap`` (default: the bound)."""
    dev = _dev(bits, points_xyz, mask_label)
    K, S, W, N = tables["K"], tables["S"], tables["W"], tables["N"]
    assert points_xyz.dtype == torch.float32 and points_xyz.stride(1) == 1 and int(points_xyz.shape[0]) == N
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (K, W) and bits.is_contiguous()
    cap = int(tables["cap"] if M_cap is None else M_cap)
    if K == 0 or cap == 0 or N == 0:
        return None
    label = _c(mask_label, torch.int64)
    assert label.shape == (K,)
    jit = torch.cat([jitter[0].reshape(3), jitter[1].reshape(3)]).to(device=dev, dtype=torch.float32).contiguous()
    new = _new or (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev))
    counts = torch.empty((8,), dtype=torch.int64, device=dev)
    valid_mask, valid_indices = new((N,), torch.bool), new((N,), torch.int64)
    sorted_indices, point_indices, proposal_indices = new((cap,), torch.int64), new((cap,), torch.int64), new((cap,), torch.int64)
    batch_p, sem_p, xyz_p = new((cap,), torch.int32), new((cap,), torch.int32), new((cap, 3), torch.float32)
    sizes, offsets, prop_mask = new((K + 1,), torch.int64), new((K + 1,), torch.int32), new((K + 1,), torch.int64)
    coords4 = new((cap, 4), torch.int32)
    pid, order, vstart = new((cap,), torch.int32), new((cap,), torch.int32), new((cap + 1,), torch.int32)
    L = _C.lib()
    ws = _ws(L.gpn_proposals_from_masks_ws_bytes(i64(K), i64(S), i64(W), i64(cap)), dev)
    check(L.gpn_proposals_from_masks(ptr(bits), i64(W), ptr(tables["mask_scene"]), ptr(label), ptr(tables["scene_offsets"]),
                                     ptr(points_xyz), i32(points_xyz.stride(0)), i64(K), i64(S), i64(N), i32(min_points), i32(n_classes),
                                     f32(fullscale), f32(max_scale), ptr(jit), i64(cap), ptr(counts), ptr(valid_mask), ptr(valid_indices),
                                     ptr(sorted_indices), ptr(point_indices), ptr(proposal_indices), ptr(batch_p), ptr(xyz_p), ptr(sem_p),
                                     ptr(sizes), ptr(offsets), ptr(prop_mask), ptr(coords4), ptr(pid), ptr(order), ptr(vstart), ptr(ws),
                                     szt(ws.numel()), _stream()), "gpn_proposals_from_masks")
    Q, M, P, V, dropped, bad, coarse, overflow = counts.tolist()  # the stage's single device -> host read
    if bad:
        raise _C.GpnError(f"proposals_from_masks: {bad} mask(s) carry a label outside [1, {n_classes})")
    if overflow:
        raise _C.GpnError(f"proposals_from_masks: the masks have {overflow} members, the tables hold {cap}")
    if M == 0:
        return None
    return dict(counts_host=(Q, M, P, V, dropped, coarse), Q=Q, M=M, P=P, V=V, dropped=dropped, coarse=coarse, valid_mask=valid_mask,
                valid_indices=valid_indices[:Q], sorted_indices=sorted_indices[:M], point_indices=point_indices[:M],
                proposal_indices=proposal_indices[:M], batch_indices=batch_p[:M], pt_xyz=xyz_p[:M], sem_preds=sem_p[:M],
                instance_labels=None, sizes=sizes[:P], proposal_offsets=offsets[:P + 1], proposal_mask=prop_mask[:P],
                voxel_coords=coords4[:V], pc_voxel_id=pid[:M], point_order=order[:M], voxel_point_start=vstart[:V + 1])


def proposals_postprocess(score_preds, sizes, proposal_offsets, point_indices, proposal_indices, member_slot, score_threshold,
                          min_points, iou_threshold, rows: Optional[DevCount] = None, defer: bool = False):
    """Section PP of include/gpn.h: score filter + NMS + compaction tables of a validation step's proposals in one call and ONE
    host read.  -> (kept_ids [P''] i32 ascending, new_offsets [P''+1] i32, src_row [M''] i64), or None when a kernel table
    overflowed (the caller falls back to the torch formulation)."""
    dev = _dev(score_preds, sizes)
    P = int(score_preds.shape[0])
    M = int(point_indices.shape[0])
    N = int(member_slot.shape[0]) // 2
    L = _C.lib()
    kept_ids = torch.empty((max(P, 1),), dtype=torch.int32, device=dev)
    new_offsets = torch.empty((P + 1,), dtype=torch.int32, device=dev)
    src_row = torch.empty((max(M, 1),), dtype=torch.int64, device=dev)
    counts = torch.empty((3,), dtype=torch.int64, device=dev)
    ws = _ws(L.gpn_proposals_postprocess_ws_bytes(i64(P)), dev)
    p_dev, p_plan = (rows.ptr, i64(rows.plan)) if rows is not None else (ptr(None), i64(0))
    check(L.gpn_proposals_postprocess(ptr(_c(score_preds, torch.float32)), ptr(_c(sizes, torch.int64)), ptr(_c(proposal_offsets, torch.int32)),
                                      ptr(_c(point_indices, torch.int64)), ptr(_c(proposal_indices, torch.int64)),
                                      ptr(_c(member_slot, torch.int32)), i64(N), i64(P), p_dev, p_plan, f32(score_threshold),
                                      i64(min_points), f32(iou_threshold), ptr(kept_ids), ptr(new_offsets), ptr(src_row), ptr(counts),
                                      ptr(ws), szt(ws.numel()), _stream()), "gpn_proposals_postprocess")
    if defer:  # the read is the caller's, later (PostprocessHandle.result): nothing waits for this step's kernels now
        host = _PINNED_COUNTS.pop() if _PINNED_COUNTS else torch.empty((3,), dtype=torch.int64).pin_memory()
        host.copy_(counts, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return PostprocessHandle(kept_ids, new_offsets, src_row, host, ev)
    n_kept, n_points, overflow = counts.tolist()  # the step's one read of its post-processing
    if overflow:
        return None
    return kept_ids[:n_kept], new_offsets[:n_kept + 1], src_row[:n_points]


def scene_prepare(points, sem_labels, instance_labels, seg_offsets, mats=None, shifts=None):
    """Section SP of include/gpn.h: label compaction, augmentation and the per-instance statistics of a batch of RAW scenes in three
    launches and ONE host read (the instances per scene).  points [N, 3 + C] f32, sem_labels [N] int16 / int32 / int64,
    instance_labels [N] i32, seg_offsets [B + 1] i64 (device), mats [B, 3, 3] / shifts [B, C] f64 on the device or None.
    -> dict(points, batch_indices, instance_labels, instance_regions, num_points_per_instance, instance_sem_labels [B, max K],
    num_instances = [K per scene]) or None when a scene has more distinct ids than the kernel tables hold."""
    dev = _dev(points, instance_labels)
    points, instance_labels = _c(points, torch.float32), _c(instance_labels, torch.int32)
    sem_labels = sem_labels.contiguous()
    sem_bytes = sem_labels.element_size()
    assert sem_labels.dtype in (torch.int16, torch.int32, torch.int64), sem_labels.dtype
    N, W = points.shape
    B = int(seg_offsets.shape[0]) - 1
    L = _C.lib()
    cap = L.gpn_scene_prepare_max_instances()
    out_points = torch.empty_like(points)
    batch_indices = torch.empty((N,), dtype=torch.int32, device=dev)
    ins_out = torch.empty((N,), dtype=torch.int32, device=dev)
    regions = torch.empty((N, 9), dtype=torch.float32, device=dev)
    npi = torch.empty((B, cap), dtype=torch.int32, device=dev)
    isl = torch.empty((B, cap), dtype=torch.int32, device=dev)
    overflow = torch.empty((1,), dtype=torch.int32, device=dev)
    k_host = _PINNED_K.pop() if _PINNED_K and _PINNED_K[-1].numel() >= B else torch.empty((max(B, 64),), dtype=torch.int64).pin_memory()
    ws = _ws(L.gpn_scene_prepare_ws_bytes(i32(B)), dev)
    check(L.gpn_scene_prepare(ptr(points), ptr(sem_labels), i32(sem_bytes), ptr(instance_labels), ptr(_c(seg_offsets, torch.int64)),
                              i64(N), i32(W - 3), i32(B), ptr(_c(mats, torch.float64)), ptr(_c(shifts, torch.float64)),
                              ptr(out_points), ptr(batch_indices), ptr(ins_out), ptr(regions), ptr(npi), ptr(isl), ptr(k_host),
                              ptr(overflow), ptr(ws), szt(ws.numel()), _stream()), "gpn_scene_prepare")
    ev = torch.cuda.Event(blocking=True)
    ev.record()
    ev.synchronize()  # the preparation's one host read: K per scene, written into pinned memory by the first kernel
    k = k_host[:B].tolist()
    _PINNED_K.append(k_host)
    if min(k) < 0:
        return None
    width = max(k)
    return dict(points=out_points, batch_indices=batch_indices, instance_labels=ins_out, instance_regions=regions,
                num_points_per_instance=npi[:, :width].contiguous(), instance_sem_labels=isl[:, :width].contiguous(),
                num_instances=k)


_PINNED_K = []
_PINNED_COUNTS = []


class PostprocessHandle:
    """outputs of a gpn_proposals_postprocess call whose counts have not been read yet; ``result()`` waits for them (no wait if
    the call's kernels have run) -> (kept_ids, new_offsets, src_row) sliced to size, or None after a table overflow"""

    def __init__(self, kept_ids, new_offsets, src_row, host, event):
        self.kept_ids, self.new_offsets, self.src_row, self.host, self.event = kept_ids, new_offsets, src_row, host, event

    def result(self):
        self.event.synchronize()
        n_kept, n_points, overflow = self.host.tolist()
        _PINNED_COUNTS.append(self.host)
        if overflow:
            return None
        return self.kept_ids[:n_kept], self.new_offsets[:n_kept + 1], self.src_row[:n_points]


def proposals_targets(sem_labels, gt_npcs, point_indices, rows: DevCount):
    """sem_labels [N] i64 / gt_npcs [N,3] f32 (either may be None) at the proposal points -> ([M] i64 or None, [M,3] f32 or
    None), M = point_indices.shape[0] = the bound; rows past the device count stay unwritten"""
    dev = _dev(point_indices)
    M = point_indices.shape[0]
    sem_out = torch.empty((M,), dtype=torch.int64, device=dev) if sem_labels is not None else None
    npcs_out = torch.empty((M, 3), dtype=torch.float32, device=dev) if gt_npcs is not None else None
    check(_C.lib().gpn_proposals_targets_dev(ptr(_c(sem_labels, torch.int64)), ptr(_c(gt_npcs, torch.float32)), ptr(point_indices),
                                             i64(M), *rows.args(), ptr(sem_out), ptr(npcs_out), _stream()), "gpn_proposals_targets_dev")
    return sem_out, npcs_out


def proposals_voxel_mean(feats, point_indices, point_order, voxel_point_start, V, rows: Optional[DevCount] = None):
    dev = _dev(feats)
    feats = _c(feats, torch.float32)
    out = torch.empty((V, feats.shape[1]), dtype=torch.float32, device=dev)
    if rows is not None:
        check(_C.lib().gpn_proposals_voxel_mean_dev(ptr(feats), ptr(point_indices), ptr(point_order), ptr(voxel_point_start), i64(V),
                                                    *rows.args(), i32(feats.shape[1]), ptr(out), _stream()), "gpn_proposals_voxel_mean_dev")
        return out
    check(_C.lib().gpn_proposals_voxel_mean(ptr(feats), ptr(point_indices), ptr(point_order), ptr(voxel_point_start), i64(V),
                                            i32(feats.shape[1]), ptr(out), _stream()), "gpn_proposals_voxel_mean")
    return out


def proposals_voxel_mean_bwd(dout, member_slot, pc_voxel_id, voxel_point_start, N):
    dev = _dev(dout)
    dout = _c(dout, torch.float32)
    dfeats = torch.empty((N, dout.shape[1]), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_proposals_voxel_mean_bwd(ptr(dout), ptr(member_slot), ptr(pc_voxel_id), ptr(voxel_point_start), i64(N),
                                                i32(dout.shape[1]), ptr(dfeats), _stream()), "gpn_proposals_voxel_mean_bwd")
    return dfeats


# ---------------------------------------------------------------------------------------------------- NPCS loss
def _npcs_args(sym):
    i32a = lambda v: (_C.ctypes.c_int32 * len(v))(*v)  # noqa: E731
    return i32a(sym["first"]), i32a(sym["count"]), i32a(sym["group"]), i32(len(sym["first"]))


def npcs_loss_fwd(logits, gt_npcs, sem_preds, sem_labels, proposal_offsets, sym, rows: Optional[DevCount] = None):
    """-> (loss [1] f32, scratch for the backward).  ``sym`` = dict(sym_of_class i64 [classes], mats f32 [n,3,3] (device),
    first / count / group: python lists per symmetry type)."""
    dev = _dev(logits, gt_npcs)
    logits, gt_npcs = _c(logits, torch.float32), _c(gt_npcs, torch.float32)
    sem_preds, sem_labels = _c(sem_preds, torch.int32), _c(sem_labels, torch.int64)
    proposal_offsets = _c(proposal_offsets, torch.int32)
    P = proposal_offsets.shape[0] - 1
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    scratch = torch.empty((9 * P + 4,), dtype=torch.float32, device=dev)
    first, count, group, n = _npcs_args(sym)
    if rows is not None:  # the proposal count is a device counter (P = its bound)
        check(_C.lib().gpn_npcs_loss_fwd_dev(ptr(logits), i32(logits.shape[1]), ptr(gt_npcs), ptr(sem_preds), ptr(sem_labels),
                                             ptr(proposal_offsets), i64(P), *rows.args(), ptr(sym["sym_of_class"]), ptr(sym["mats"]),
                                             first, count, group, n, ptr(loss), ptr(scratch), _stream()), "gpn_npcs_loss_fwd_dev")
        return loss, scratch
    check(_C.lib().gpn_npcs_loss_fwd(ptr(logits), i32(logits.shape[1]), ptr(gt_npcs), ptr(sem_preds), ptr(sem_labels),
                                     ptr(proposal_offsets), i64(P), ptr(sym["sym_of_class"]), ptr(sym["mats"]), first, count,
                                     group, n, ptr(loss), ptr(scratch), _stream()), "gpn_npcs_loss_fwd")
    return loss, scratch


def npcs_loss_bwd(logits, gt_npcs, sem_preds, sem_labels, proposal_indices, P, sym, scratch, grad_loss,
                  m_rows: Optional[DevCount] = None):
    dev = _dev(logits)
    d_logits = torch.empty_like(logits)
    first, count, group, n = _npcs_args(sym)
    if m_rows is not None:  # the point count is a device counter (rows of d_logits past it stay unwritten)
        check(_C.lib().gpn_npcs_loss_bwd_dev(ptr(logits), i32(logits.shape[1]), ptr(gt_npcs), ptr(sem_preds), ptr(sem_labels),
                                             ptr(_c(proposal_indices, torch.int64)), i64(logits.shape[0]), *m_rows.args(), i64(P),
                                             ptr(sym["sym_of_class"]), ptr(sym["mats"]), first, count, group, n, ptr(scratch),
                                             ptr(_c(grad_loss.reshape(1), torch.float32)), ptr(d_logits), _stream()), "gpn_npcs_loss_bwd_dev")
        return d_logits
    check(_C.lib().gpn_npcs_loss_bwd(ptr(logits), i32(logits.shape[1]), ptr(gt_npcs), ptr(sem_preds), ptr(sem_labels),
                                     ptr(_c(proposal_indices, torch.int64)), i64(logits.shape[0]), i64(P), ptr(sym["sym_of_class"]),
                                     ptr(sym["mats"]), first, count, group, n, ptr(scratch),
                                     ptr(_c(grad_loss.reshape(1), torch.float32)), ptr(d_logits), _stream()), "gpn_npcs_loss_bwd")
    return d_logits


# ---------------------------------------------------------------------------------------------------- H (dense heads)
def linear_supported(cin: int, cout: int) -> bool:
    return bool(_C.lib().gpn_linear_supported(i32(cin), i32(cout)))


def linear_fwd(x, weight, bias, rows: Optional[DevCount] = None):
    """y = x @ weight.T + bias in one launch (csrc/linear.hip); weight [cout, cin] as torch.nn.Linear holds it"""
    dev = _dev(x, weight)
    x, weight = _c(x, torch.float32), _c(weight, torch.float32)
    N, cin = x.shape
    cout = weight.shape[0]
    y = torch.empty((N, cout), dtype=torch.float32, device=dev)
    if rows is not None:  # the row count is a device counter (N = its bound)
        check(_C.lib().gpn_linear_fwd_dev(ptr(x), ptr(weight), ptr(_c(bias, torch.float32) if bias is not None else None), i64(N),
                                          *rows.args(), i32(cin), i32(cout), ptr(y), _stream()), "gpn_linear_fwd_dev")
        return y
    check(_C.lib().gpn_linear_fwd(ptr(x), ptr(weight), ptr(_c(bias, torch.float32) if bias is not None else None), i64(N),
                                  i32(cin), i32(cout), ptr(y), _stream()), "gpn_linear_fwd")
    return y


def linear_bwd(x, weight, dy, need_dx: bool, need_dw: bool, need_db: bool, rows: Optional[DevCount] = None):
    """-> (dx or None, dW or None, db or None): three launches at most (dx; partial dW / db per 512 rows; their ordered sum)"""
    dev = _dev(x, dy)
    x, weight, dy = _c(x, torch.float32), _c(weight, torch.float32), _c(dy, torch.float32)
    N, cin = x.shape
    cout = weight.shape[0]
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(weight) if need_dw else None
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if need_db else None
    L = _C.lib()
    ws = _ws(L.gpn_linear_bwd_ws_bytes(i64(N), i32(cin), i32(cout)), dev) if (need_dw or need_db) else None
    if rows is not None:
        check(L.gpn_linear_bwd_dev(ptr(x), ptr(weight), ptr(dy), i64(N), *rows.args(), i32(cin), i32(cout), ptr(dx), ptr(dw), ptr(db),
                                   ptr(ws), szt(ws.numel() if ws is not None else 0), _stream()), "gpn_linear_bwd_dev")
        return dx, dw, db
    check(L.gpn_linear_bwd(ptr(x), ptr(weight), ptr(dy), i64(N), i32(cin), i32(cout), ptr(dx), ptr(dw), ptr(db), ptr(ws),
                           szt(ws.numel() if ws is not None else 0), _stream()), "gpn_linear_bwd")
    return dx, dw, db


def score_loss(logits, cls_source, proposal_offsets, ious, fg_thresh, bg_thresh, rows: Optional[DevCount] = None):
    """-> (loss [1] f32, score_preds [P] f32, d_logits [P, C1] f32) in one launch (gpn_score_loss)"""
    dev = _dev(logits, ious)
    logits, ious = _c(logits, torch.float32), _c(ious, torch.float32)
    po = _c(proposal_offsets, torch.int32)
    cls_source = cls_source.contiguous()
    assert cls_source.dtype in (torch.int64, torch.int32)
    P, C1 = logits.shape
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    preds = torch.empty((P,), dtype=torch.float32, device=dev)
    d_logits = torch.empty_like(logits)
    is64 = cls_source.dtype == torch.int64
    if rows is not None:  # the proposal count is a device counter (P = its bound; rows past it stay unwritten and unread)
        check(_C.lib().gpn_score_loss_dev(ptr(logits), i32(C1), ptr(cls_source if is64 else None), ptr(None if is64 else cls_source),
                                          ptr(po), ptr(ious), i32(ious.shape[1]), i64(P), rows.ptr, f32(fg_thresh), f32(bg_thresh),
                                          ptr(loss), ptr(preds), ptr(d_logits), _stream()), "gpn_score_loss_dev")
        return loss, preds, d_logits
    check(_C.lib().gpn_score_loss(ptr(logits), i32(C1), ptr(cls_source if is64 else None), ptr(None if is64 else cls_source),
                                  ptr(po), ptr(ious), i32(ious.shape[1]), i64(P), f32(fg_thresh), f32(bg_thresh), ptr(loss),
                                  ptr(preds), ptr(d_logits), _stream()), "gpn_score_loss")
    return loss, preds, d_logits


# ---------------------------------------------------------------------------------------------------- VP (rendered views)
VIEW_OK, VIEW_TOO_FEW, VIEW_LABEL_MISMATCH, VIEW_INSTANCE_BOUND = 0, 1, 2, 3


def view_max_instance_ids() -> int:
    return int(_C.lib().gpn_view_max_instance_ids())


def view_backproject(depth, sem, ins, K, status=None):
    """depth [V,H,W] f32 / f64, sem / ins [V,H,W] i32, K [V,3,3] f64 -> (pixel [V,H*W] i32 = the valid pixels' linear indices in
    row-major order, points [V,H*W,4] f32 = the float32 cast of their float64 back-projection in .xyz, counts [V] i32,
    status [V] i32), all left on the device"""
    dev = _dev(depth, sem, ins, K)
    if depth.dtype not in (torch.float32, torch.float64):
        raise _C.GpnError(f"view depth must be float32 or float64, got {depth.dtype}")
    depth = depth.contiguous()
    sem, ins, K = _c(sem, torch.int32), _c(ins, torch.int32), _c(K, torch.float64)
    V, H, W = depth.shape
    pixel = torch.empty((V, H * W), dtype=torch.int32, device=dev)
    points = torch.empty((V, H * W, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((V,), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty((V,), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_view_backproject(ptr(depth), i32(depth.element_size()), ptr(sem), ptr(ins), ptr(K), i32(V), i32(H), i32(W),
                                        ptr(pixel), ptr(points), ptr(counts), ptr(status), _stream()), "gpn_view_backproject")
    return pixel, points, counts, status


def view_fps(points, counts, status, m, max_groups=0):
    """ragged FPS of all V views in one launch: for each view with status VIEW_OK the m samples gpn_pn2_furthest_point_sampling
    takes from points[v, :counts[v], :3] alone (counts[v] == m: arange; < m: status VIEW_TOO_FEW).  points [V, n_bound, 4] f32
    (.w is overwritten).  max_groups > 0 caps the workgroups per view (1: the form without inter-workgroup waits)."""
    dev = _dev(points, counts, status)
    V, nb, _ = points.shape
    idx = torch.zeros((V, int(m)), dtype=torch.int32, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_view_fps_ws_bytes(i32(V)), dev)
    check(L.gpn_view_fps(ptr(points), i64(nb), ptr(counts), ptr(status), i32(V), i32(m), i32(max_groups), ptr(idx), ptr(ws),
                         szt(ws.numel()), _stream()), "gpn_view_fps")
    return idx


def view_fps_ragged(xyz, counts, m, max_groups=0):
    """view_fps over clouds given as xyz [V, n_max, 3] f32 with counts [V] live rows -> (idx [V, m] i32, status [V] i32)"""
    dev = _dev(xyz, counts)
    V, nb, _ = xyz.shape
    points = torch.zeros((V, nb, 4), dtype=torch.float32, device=dev)
    points[..., :3] = xyz
    status = torch.zeros((V,), dtype=torch.int32, device=dev)
    idx = view_fps(points, _c(counts, torch.int32), status, m, max_groups)
    return idx, status


_VIEW_FIELDS = (("xyz", torch.float32, 3), ("rgb", torch.float32, 3), ("sem", torch.int32, 0), ("ins", torch.int32, 0),
                ("npcs", torch.float32, 3), ("pix", torch.int32, 2), ("gt", torch.int32, 0))


def view_layout(V, m):
    """(name, dtype, shape, byte offset) of every result of view_convert inside its one buffer, and the buffer's size"""
    fields = [("scale", torch.float64, (V, 4)), ("status", torch.int32, (V,))]
    fields += [(name, dt, (V, m, c) if c else (V, m)) for name, dt, c in _VIEW_FIELDS]
    layout, total = [], 0
    for name, dt, shape in fields:
        layout.append((name, dt, shape, total))
        total += (int(np.prod(shape)) * (8 if dt == torch.float64 else 4) + 255) // 256 * 256
    return layout, total


def view_fields(buf, layout):
    """views of a view_convert buffer (on the device or a host copy of it) by name"""
    out = {}
    for name, dt, shape, off in layout:
        nbytes = int(np.prod(shape)) * (8 if dt == torch.float64 else 4)
        out[name] = buf[off:off + nbytes].view(dt).view(shape)
    return out


def view_convert(depth, rgb, sem, ins, npcs, K, m, max_groups=0):
    """rendered views -> training scenes for V views of one size (the three launches of include/gpn.h section VP, no host read
    in between).  depth [V,H,W] f32 / f64, rgb [V,H,W,3] u8, sem / ins [V,H,W] i32, npcs [V,H,W,3] f32, K [V,3,3] f64.
    -> (buffer, layout): every result in ONE device buffer, so that a batch costs one host read (view_fields names them:
    scale [V,4] f64, status [V] i32, xyz / rgb / npcs [V,m,3] f32, sem / ins / gt [V,m] i32, pix [V,m,2] i32)."""
    dev = _dev(depth, rgb, sem, ins, npcs, K)
    if depth.dtype not in (torch.float32, torch.float64):
        raise _C.GpnError(f"view depth must be float32 or float64, got {depth.dtype}")
    V, H, W = depth.shape
    m = int(m)
    depth = depth.contiguous()
    rgb, npcs = _c(rgb, torch.uint8), _c(npcs, torch.float32)
    sem, ins, K = _c(sem, torch.int32), _c(ins, torch.int32), _c(K, torch.float64)
    if tuple(rgb.shape) != (V, H, W, 3) or tuple(npcs.shape) != (V, H, W, 3) or tuple(sem.shape) != (V, H, W) \
            or tuple(ins.shape) != (V, H, W) or K.numel() != V * 9:
        raise _C.GpnError("view_convert: rgb / npcs must be [V,H,W,3], sem / ins [V,H,W], K [V,3,3]")
    layout, total = view_layout(V, m)
    buf = torch.empty((total,), dtype=torch.uint8, device=dev)
    f = view_fields(buf, layout)
    pixel, points, counts, _ = view_backproject(depth, sem, ins, K, status=f["status"])
    idx = view_fps(points, counts, f["status"], m, max_groups)
    check(_C.lib().gpn_view_finish(ptr(depth), i32(depth.element_size()), ptr(rgb), ptr(sem), ptr(ins), ptr(npcs), ptr(K), i32(V),
                                   i32(H), i32(W), ptr(pixel), ptr(idx), i32(m), ptr(f["status"]), ptr(f["xyz"]), ptr(f["rgb"]),
                                   ptr(f["sem"]), ptr(f["ins"]), ptr(f["npcs"]), ptr(f["pix"]), ptr(f["gt"]), ptr(f["scale"]),
                                   _stream()), "gpn_view_finish")
    return buf, layout


# ---------------------------------------------------------------------------------------------------- RD (asset rendering)
RENDER_COUNTERS = 5
_RENDER_DT = {torch.float32: 4, torch.int32: 4, torch.uint8: 1}


def render_layout(V, H, W, L):
    """(name, dtype, shape, byte offset) of every result of render_batch inside its one buffer, and the buffer's size"""
    fields = [("counters", torch.int32, (V, RENDER_COUNTERS)), ("link_area", torch.int32, (V, L)), ("link_inst", torch.int32, (V, L)),
              ("depth", torch.float32, (V, H, W)), ("tri", torch.int32, (V, H, W)), ("sem", torch.int32, (V, H, W)),
              ("ins", torch.int32, (V, H, W)), ("npcs", torch.float32, (V, H, W, 3)), ("rgb", torch.uint8, (V, H, W, 3))]
    layout, total = [], 0
    for name, dt, shape in fields:
        layout.append((name, dt, shape, total))
        total += (int(np.prod(shape)) * _RENDER_DT[dt] + 255) // 256 * 256
    return layout, total


def render_fields(buf, layout):
    """views of a render_batch buffer (on the device or a host copy of it) by name"""
    out = {}
    for name, dt, shape, off in layout:
        nbytes = int(np.prod(shape)) * _RENDER_DT[dt]
        out[name] = buf[off:off + nbytes].view(dt).view(shape)
    return out


def render_max_links() -> int:
    return int(_C.lib().gpn_render_max_links())


RENDER_SHADINGS = ("flat", "textured")


def render_max_lights() -> int:
    return int(_C.lib().gpn_render_max_lights())


def render_shade(geom, views, depth, tri, rgb, H, W, Nt_max, background=(0, 0, 0), check_tables=True):
    """textured, lit RGB for rendered views (include/gpn.h section RS): overwrites rgb [V,H,W,3] u8 from depth [V,H,W] f32 and
    tri [V,H,W] i32 of render_batch.  geom as for render_batch plus, when the asset set has textures, tri_uv [Nt,3,2] f32, tri_tex
    [Nt] i32, tex_table [T,4] i32 and tex_data [texels,4] u8; views plus lights [V,NL,8] f64.  check_tables: the
    contents of tri_tex and tex_table are checked on the device first (one small host read BEFORE the launch); a caller that built
    the tables on the host and checked them there passes False."""
    verts, tris = _c(geom["verts"], torch.float32), _c(geom["tris"], torch.int32)
    tri_visual, tri_color, assets = _c(geom["tri_visual"], torch.int32), _c(geom["tri_color"], torch.float32), _c(geom["assets"], torch.int32)
    view_asset, cam, vis_mat = _c(views["view_asset"], torch.int32), _c(views["cam"], torch.float64), _c(views["vis_mat"], torch.float64)
    if "lights" not in views:
        raise _C.GpnError("render_shade: views has no lights [V,NL,8] table")
    lights = _c(views["lights"], torch.float64)
    depth, tri = _c(depth, torch.float32), _c(tri, torch.int32)
    if rgb.dtype != torch.uint8 or not rgb.is_contiguous():
        raise _C.GpnError("render_shade: rgb must be a contiguous uint8 tensor")
    tensors = [verts, tris, tri_visual, tri_color, assets, view_asset, cam, vis_mat, lights, depth, tri, rgb]
    V, H, W, Nt_max = int(view_asset.shape[0]), int(H), int(W), int(Nt_max)
    Nv, Nt, A = int(verts.shape[0]), int(tris.shape[0]), int(assets.shape[0])
    if tuple(verts.shape) != (Nv, 3) or tuple(tris.shape) != (Nt, 3) or tri_visual.numel() != Nt or tuple(tri_color.shape) != (Nt, 3) \
            or tuple(assets.shape) != (A, 4):
        raise _C.GpnError("render_shade: verts [Nv,3], tris [Nt,3], tri_visual [Nt], tri_color [Nt,3], assets [A,4]")
    if cam.numel() != V * 20 or vis_mat.dim() != 3 or vis_mat.shape[0] != V or vis_mat.shape[2] != 12 or lights.dim() != 3 \
            or lights.shape[0] != V or lights.shape[2] != 8:
        raise _C.GpnError("render_shade: cam [V,20], vis_mat [V,M,12], lights [V,NL,8]")
    if depth.numel() != V * H * W or tri.numel() != V * H * W or rgb.numel() != V * H * W * 3:
        raise _C.GpnError("render_shade: depth / tri [V,H,W], rgb [V,H,W,3]")
    M, NL = int(vis_mat.shape[1]), int(lights.shape[1])
    tri_uv = tri_tex = tex_table = tex_data = None
    T = texels = 0
    if geom.get("tex_table") is not None and int(geom["tex_table"].shape[0]) > 0:
        tri_uv, tri_tex = _c(geom["tri_uv"], torch.float32), _c(geom["tri_tex"], torch.int32)
        tex_table, tex_data = _c(geom["tex_table"], torch.int32), geom["tex_data"]
        T = int(tex_table.shape[0])
        texels = tex_data.numel() // 4
        if tri_uv.numel() != Nt * 6 or tri_tex.numel() != Nt or tuple(tex_table.shape) != (T, 4) or tex_data.dtype != torch.uint8 \
                or tex_data.numel() % 4 or not tex_data.is_contiguous():
            raise _C.GpnError("render_shade: tri_uv [Nt,3,2], tri_tex [Nt], tex_table [T,4], tex_data [texels,4]")
        tensors += [tri_uv, tri_tex, tex_table, tex_data]
    _dev(*tensors)
    if T and check_tables and Nt:
        tt = tex_table.to(torch.int64)
        bad = torch.stack([((tri_tex < -1) | (tri_tex >= T)).any(),
                           ((tt[:, 0] < 0) | (tt[:, 1] < 1) | (tt[:, 2] < 1) | (tt[:, 0] + tt[:, 1] * tt[:, 2] > texels)).any()]).tolist()
        if bad[0]:
            raise _C.GpnError(f"render_shade: bad argument: tri_tex outside [-1, {T})")
        if bad[1]:
            raise _C.GpnError(f"render_shade: bad argument: a tex_table row spans texels outside tex_data ({texels} texels)")
    check(_C.lib().gpn_render_shade(ptr(verts), i32(Nv), ptr(tris), ptr(tri_visual), ptr(tri_color), i32(Nt), ptr(assets), i32(A),
                                    ptr(view_asset), ptr(cam), ptr(vis_mat), i32(M), ptr(tri_uv), ptr(tri_tex), ptr(tex_table), i32(T),
                                    ptr(tex_data), i64(texels), ptr(lights), i32(NL), ptr(depth), ptr(tri), i32(V), i32(H), i32(W),
                                    i32(Nt_max), i32(background[0]), i32(background[1]), i32(background[2]), ptr(rgb), _stream()),
          "gpn_render_shade")
    return rgb


def render_batch(geom, views, H, W, Nt_max, background=(0, 0, 0), timings=None, buf=None, shading="flat", check_tables=True):
    """V views of articulated assets -> depth, winning triangle, labels, NPCS and RGB (include/gpn.h section RD: setup, raster,
    annotate; no host read in between).  geom: verts [Nv,3] f32, tris [Nt,3] i32, tri_visual / tri_link [Nt] i32, tri_color [Nt,3]
    f32, assets [A,4] i32.  views: view_asset [V] i32, cam [V,20] f64, vis_mat [V,M,12] f64, link_cat / link_rank [V,L] i32,
    link_frame [V,L,13] f64.  -> (buffer, layout): every result in ONE device buffer (render_fields names them).  timings: a list
    that receives (start, end) torch events around each of the entry points.  buf: a uint8 device buffer of the layout's
    size to write into (default: a new one).  shading "textured": render_shade runs as a fourth launch and overwrites the rgb
    field of the same buffer (section RS; geom and views then also carry its tables)."""
    if shading not in RENDER_SHADINGS:
        raise _C.GpnError(f"render_batch: shading must be one of {RENDER_SHADINGS}, got {shading!r}")
    verts, tris = _c(geom["verts"], torch.float32), _c(geom["tris"], torch.int32)
    tri_visual, tri_link = _c(geom["tri_visual"], torch.int32), _c(geom["tri_link"], torch.int32)
    tri_color, assets = _c(geom["tri_color"], torch.float32), _c(geom["assets"], torch.int32)
    view_asset, cam, vis_mat = _c(views["view_asset"], torch.int32), _c(views["cam"], torch.float64), _c(views["vis_mat"], torch.float64)
    link_cat, link_rank = _c(views["link_cat"], torch.int32), _c(views["link_rank"], torch.int32)
    link_frame = _c(views["link_frame"], torch.float64)
    dev = _dev(verts, tris, tri_visual, tri_link, tri_color, assets, view_asset, cam, vis_mat, link_cat, link_rank, link_frame)
    V, H, W, Nt_max = int(view_asset.shape[0]), int(H), int(W), int(Nt_max)
    Nv, Nt, A = int(verts.shape[0]), int(tris.shape[0]), int(assets.shape[0])
    if tuple(verts.shape) != (Nv, 3) or tuple(tris.shape) != (Nt, 3) or tri_visual.numel() != Nt or tri_link.numel() != Nt \
            or tuple(tri_color.shape) != (Nt, 3) or tuple(assets.shape) != (A, 4):
        raise _C.GpnError("render_batch: verts [Nv,3], tris [Nt,3], tri_visual / tri_link [Nt], tri_color [Nt,3], assets [A,4]")
    if cam.numel() != V * 20 or vis_mat.dim() != 3 or vis_mat.shape[0] != V or vis_mat.shape[2] != 12 or link_cat.dim() != 2 \
            or link_cat.shape[0] != V or link_rank.shape != link_cat.shape or link_frame.numel() != link_cat.numel() * 13:
        raise _C.GpnError("render_batch: cam [V,20], vis_mat [V,M,12], link_cat / link_rank [V,L], link_frame [V,L,13]")
    M, L = int(vis_mat.shape[1]), int(link_cat.shape[1])
    layout, total = render_layout(V, H, W, L)
    if buf is None:
        buf = torch.empty((total,), dtype=torch.uint8, device=dev)
    elif buf.dtype != torch.uint8 or buf.numel() != total or not buf.is_contiguous() or buf.device != dev:
        raise _C.GpnError(f"render_batch: buf must be a contiguous uint8 tensor of {total} bytes on {dev}")
    f = render_fields(buf, layout)
    lib = _C.lib()
    nbytes = lib.gpn_render_ws_bytes(i32(V), i32(Nt_max))
    ws = _ws(nbytes, dev)
    wsp, wsb = (ptr(ws), szt(ws.numel())) if nbytes else (ptr(None), szt(0))

    def timed(call, what):
        if timings is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
        check(call(), what)
        if timings is not None:
            b.record()
            timings.append((a, b))

    timed(lambda: lib.gpn_render_setup(ptr(verts), i32(Nv), ptr(tris), ptr(tri_visual), i32(Nt), ptr(assets), i32(A), ptr(view_asset),
                                       ptr(cam), ptr(vis_mat), i32(M), i32(V), i32(H), i32(W), i32(Nt_max), wsp, wsb,
                                       ptr(f["counters"]), _stream()), "gpn_render_setup")
    timed(lambda: lib.gpn_render_raster(ptr(assets), i32(A), ptr(view_asset), i32(Nt), i32(V), i32(H), i32(W), i32(Nt_max), wsp, wsb,
                                        ptr(f["depth"]), ptr(f["tri"]), _stream()), "gpn_render_raster")
    timed(lambda: lib.gpn_render_annotate(ptr(f["depth"]), ptr(f["tri"]), ptr(tri_link), ptr(tri_color), i32(Nt), ptr(assets), i32(A),
                                          ptr(view_asset), ptr(cam), ptr(link_cat), ptr(link_rank), ptr(link_frame), i32(L), i32(V),
                                          i32(H), i32(W), i32(Nt_max), wsp, wsb, i32(background[0]), i32(background[1]),
                                          i32(background[2]), ptr(f["link_area"]), ptr(f["link_inst"]), ptr(f["sem"]), ptr(f["ins"]),
                                          ptr(f["npcs"]), ptr(f["rgb"]), _stream()), "gpn_render_annotate")
    if shading == "textured":
        a = b = None
        if timings is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
        render_shade(geom, views, f["depth"], f["tri"], f["rgb"], H, W, Nt_max, background, check_tables=check_tables)
        if timings is not None:
            b.record()
            timings.append((a, b))
    return buf, layout


# ---------------------------------------------------------------------------------------------------- CP (raw clouds)
CLOUD_OK, CLOUD_FEW, CLOUD_EMPTY, CLOUD_DEGENERATE = 0, 1, 2, 3


def _cloud_args(points, offsets):
    """points [M, C] f32 whose rows may be a column slice of a wider array (unit stride inside a row), offsets [S+1] known on
    the host -> (points, row pitch in floats, host offsets list, device offsets i64)"""
    dev = _dev(points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3:
        raise _C.GpnError(f"clouds must be float32 [M, C >= 3], got {points.dtype} {tuple(points.shape)}")
    if points.shape[0] > 0 and (points.stride(1) != 1 or points.stride(0) < points.shape[1]):
        points = points.contiguous()
    pitch = int(points.stride(0)) if points.shape[0] > 1 else int(points.shape[1])
    host = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    if len(host) < 1 or host[0] != 0 or host[-1] != points.shape[0] or any(b < a for a, b in zip(host[:-1], host[1:])):
        raise _C.GpnError("cloud offsets must rise from 0 to the number of rows")
    return points, pitch, host, torch.tensor(host, dtype=torch.int64).to(dev, non_blocking=True)


def cloud_prepare(points, offsets, m, max_groups=0, sampler="fps", seeds=None, hash_bits=32):
    """S ragged raw clouds -> the network's input (include/gpn.h section CP): gpn_cloud_pack, gpn_view_fps (or, ``sampler`` "grid",
    gpn_cloud_grid_sample with one uint32 of ``seeds`` per cloud; the result gains ``level`` [S] i64 on the host), gpn_cloud_finish, no
    host read between them and ONE at the end (counts, status, scale).  points [M, C >= 3] f32 (xyz first; rows with a
    non-finite coordinate are skipped), offsets [S+1] on the host.
    -> dict: out [S, m, C] f32 (ball-normalised xyz + the other columns; rows past counts[s] zero), sample_rows [S, m] i32 (-1 past
    counts[s]), offsets (device i64), and on the host counts [S] i64 = min(valid rows, m), status [S] i64, scale [S, 4] f64."""
    points, pitch, host, off_dev = _cloud_args(points, offsets)
    dev = points.device
    S, M, C, m = len(host) - 1, int(points.shape[0]), int(points.shape[1]), int(m)
    nb = max(max((b - a for a, b in zip(host[:-1], host[1:])), default=1), 1)
    packed = torch.empty((S, nb, 4), dtype=torch.float32, device=dev)
    rows = torch.empty((S, nb), dtype=torch.int32, device=dev)
    counts, status = torch.empty((S,), dtype=torch.int32, device=dev), torch.empty((S,), dtype=torch.int32, device=dev)
    if S > 0:
        check(_C.lib().gpn_cloud_pack(ptr(points), i64(M), i32(pitch), ptr(off_dev), i32(S), i64(nb), ptr(packed), ptr(rows),
                                      ptr(counts), ptr(status), _stream()), "gpn_cloud_pack")
    return _sample_and_finish(points, pitch, off_dev, S, packed, rows, nb, counts, status, m, max_groups, sampler, seeds, hash_bits)


def cloud_finish(points, pitch, off_dev, rows, n_bound, counts, idx, status, m):
    """gpn_cloud_finish: points [M, C] f32 of row pitch ``pitch``, off_dev [S+1] i64, rows [S, n_bound] i32 (the valid rows of
    every cloud), counts / status [S] i32, idx [S, m] i32 (gpn_view_fps) -> (out [S, m, C] f32, sample_rows [S, m] i32,
    scale [S, 4] f64) on the device; status is updated in place"""
    dev = points.device
    S, C = int(counts.shape[0]), int(points.shape[1])
    out = torch.empty((S, m, C), dtype=torch.float32, device=dev)
    sample_rows = torch.empty((S, m), dtype=torch.int32, device=dev)
    scale = torch.empty((S, 4), dtype=torch.float64, device=dev)
    if S > 0:
        check(_C.lib().gpn_cloud_finish(ptr(points), i64(points.shape[0]), i32(pitch), i32(C), ptr(off_dev), i32(S), i64(n_bound),
                                        ptr(rows), ptr(counts), ptr(idx), i32(m), ptr(status), ptr(out), ptr(sample_rows), ptr(scale),
                                        _stream()), "gpn_cloud_finish")
    return out, sample_rows, scale


SAMPLERS = ("fps", "grid")


def _seed_tensor(seeds, S, dev):
    """[S] uint32 values as the int32 tensor the library reads"""
    t = torch.as_tensor(np.asarray(seeds, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(-1)).to(dev, non_blocking=True)
    if t.shape[0] != S:
        raise _C.GpnError(f"{S} clouds need {S} seeds, got {t.shape[0]}")
    return t


def cloud_grid_sample(packed, counts, status, seeds, m, hash_bits=32):
    """the octree-cell sampler (include/gpn.h section GS) in the slot of view_fps: packed [S, n_bound, 4] f32 (not written), counts /
    status [S] i32 as gpn_cloud_pack / gpn_frame_select write them (status: n < m becomes CLOUD_FEW), seeds [S] uint32 values
    -> (idx [S, m] i32 ascending packed rows, level [S] i32 = the octree level used, -1 where nothing was sampled)"""
    dev = _dev(packed, counts, status)
    S, nb, _ = packed.shape
    idx = torch.zeros((S, int(m)), dtype=torch.int32, device=dev)
    level = torch.full((S,), -1, dtype=torch.int32, device=dev)
    if S == 0:
        return idx, level
    seeds = _seed_tensor(seeds, S, dev)
    L = _C.lib()
    ws = _ws(L.gpn_cloud_grid_sample_ws_bytes(i32(S), i64(nb)), dev)
    check(L.gpn_cloud_grid_sample(ptr(packed), i64(nb), ptr(counts), ptr(status), ptr(seeds), i32(S), i32(m), i32(hash_bits), ptr(idx),
                                  ptr(level), ptr(ws), szt(ws.numel()), _stream()), "gpn_cloud_grid_sample")
    return idx, level


def _sample_and_finish(points, pitch, off_dev, S, packed, rows, n_bound, counts, status, m, max_groups, sampler="fps", seeds=None,
                       hash_bits=32):
    """what follows the packing, for raw clouds (cloud_prepare) and frames (frame_prepare) alike: gpn_view_fps (``sampler`` "fps")
    or gpn_cloud_grid_sample ("grid", one uint32 of ``seeds`` per cloud) over ``packed``, gpn_cloud_finish over ``rows``
    [S, n_bound], then counts, status, scale and the grid sampler's level in ONE copy to the host"""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    dev = points.device
    # counts, status and scale share one buffer: one copy to the host
    tail = torch.zeros((S, 6), dtype=torch.float64, device=dev)
    ints = tail[:, 4:].view(torch.int32)  # [S, 4] i32: column 0 counts, column 1 status, column 2 the grid sampler's level
    level = None
    if S == 0:
        idx = None
    elif sampler == "grid":
        idx, level = cloud_grid_sample(packed, counts, status, [0] * S if seeds is None else seeds, m, hash_bits)
    else:
        idx = view_fps(packed, counts, status, m, max_groups)
    out, sample_rows, scale = cloud_finish(points, pitch, off_dev, rows, n_bound, counts, idx, status, m)
    if S > 0:
        tail[:, :4] = scale
        ints[:, 0] = counts
        ints[:, 1] = status
        if level is not None:
            ints[:, 2] = level
    host_tail = tail.cpu()
    host_ints = host_tail[:, 4:].view(torch.int32)
    got = dict(out=out, sample_rows=sample_rows, offsets=off_dev, counts_dev=counts, status_dev=status,
               counts=host_ints[:, 0].long().clamp(max=m), status=host_ints[:, 1].long(), scale=host_tail[:, :4].clone())
    if sampler == "grid":
        got["level"] = host_ints[:, 2].long()
    return got


def cloud_nearest(points, offsets, sample_rows, counts, status, want_d2=False):
    """for every row of the caller's clouds the nearest sample of its own cloud, exact (include/gpn.h section CP): points [M, C] f32,
    offsets [S+1] (host), sample_rows [S, m] i32, counts / status [S] i32 on the device (the valid-row counts and statuses of
    cloud_prepare) -> nn [M] i32 = the sample's position in its cloud, -1 for invalid rows and clouds that are not OK
    (, d2 [M] f32)"""
    points, pitch, host, off_dev = _cloud_args(points, offsets)
    dev = _dev(points, sample_rows, counts, status)
    S, M = len(host) - 1, int(points.shape[0])
    sample_rows, counts, status = _c(sample_rows, torch.int32), _c(counts, torch.int32), _c(status, torch.int32)
    if sample_rows.dim() != 2 or sample_rows.shape[0] != S or counts.shape[0] != S or status.shape[0] != S:
        raise _C.GpnError("cloud_nearest: sample_rows must be [S, m], counts and status [S]")
    m = int(sample_rows.shape[1])
    nn = torch.empty((M,), dtype=torch.int32, device=dev)
    d2 = torch.empty((M,), dtype=torch.float32, device=dev) if want_d2 else None
    if S > 0 and M > 0:
        L = _C.lib()
        ws = _ws(L.gpn_cloud_nearest_ws_bytes(i32(S), i32(m)), dev)
        check(L.gpn_cloud_nearest(ptr(points), i64(M), i32(pitch), ptr(off_dev), i32(S), ptr(sample_rows), ptr(counts), ptr(status),
                                  i32(m), ptr(nn), ptr(d2), ptr(ws), szt(ws.numel()), _stream()), "gpn_cloud_nearest")
    else:
        nn.fill_(-1)
    return (nn, d2) if want_d2 else nn


# ---------------------------------------------------------------------------------------------------- FR (RGB-D frames)
_FRAME_DEPTH = {torch.float32: 0, torch.float64: 1, torch.uint16: 2, torch.int16: 2}


def frame_backproject(depth, rgb, K, keep=None, depth_scale=1.0, flip=False):
    """depth [V,H,W] f32 / f64 / u16 (int16 storage is read as u16), rgb [V,H,W,3] u8, K [V,3,3] f64, keep [V,H,W] u8 / bool or None
    -> (rows [V*H*W, 6] f32 with NaN xyz on invalid pixels, valid [V,H,W] u8, valid_counts [V] i32), all on the device
    (include/gpn.h section FR)"""
    dev = _dev(depth, rgb, K)
    if depth.dtype not in _FRAME_DEPTH or depth.dim() != 3:
        raise _C.GpnError(f"frame depth must be [V,H,W] float32, float64 or uint16, got {depth.dtype} {tuple(depth.shape)}")
    V, H, W = (int(v) for v in depth.shape)
    depth = depth.contiguous()
    rgb, K = _c(rgb, torch.uint8), _c(K, torch.float64)
    if tuple(rgb.shape) != (V, H, W, 3) or K.numel() != V * 9:
        raise _C.GpnError("frame_backproject: rgb must be [V,H,W,3] and K [V,3,3]")
    if keep is not None:
        _dev(keep)
        keep = _c(keep.to(torch.uint8) if keep.dtype == torch.bool else keep, torch.uint8)
        if tuple(keep.shape) != (V, H, W):
            raise _C.GpnError("frame_backproject: keep must be [V,H,W]")
    rows = torch.empty((V * H * W, 6), dtype=torch.float32, device=dev)
    valid = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    valid_counts = torch.empty((V,), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_frame_backproject(ptr(depth), i32(_FRAME_DEPTH[depth.dtype]), _C.ctypes.c_double(float(depth_scale)), ptr(rgb),
                                         ptr(keep), ptr(K), i32(V), i32(H), i32(W), i32(1 if flip else 0), ptr(rows), ptr(valid),
                                         ptr(valid_counts), _stream()), "gpn_frame_backproject")
    return rows, valid, valid_counts


def frame_select(rows, valid, valid_counts, seeds, cap, hash_bits=32):
    """the seeded presample and the ordered compaction of section FR: rows [V*H*W, 6] f32, valid [V,H,W] u8, valid_counts [V] i32,
    seeds [V] (uint32 values) -> (packed [V, n_bound, 4] f32, pix [V, H*W] i32 = the kept pixels ascending, counts [V] i32,
    status [V] i32); n_bound = cap, or H*W for cap == 0 (no presample)"""
    dev = _dev(rows, valid, valid_counts)
    V, H, W = (int(v) for v in valid.shape)
    cap = int(cap)
    nb = cap if cap > 0 else H * W
    seeds = torch.as_tensor(np.asarray(seeds, dtype=np.int64).astype(np.uint32).view(np.int32).reshape(-1)).to(dev, non_blocking=True)
    if seeds.shape[0] != V or rows.shape[0] != V * H * W:
        raise _C.GpnError("frame_select: one seed per frame and one row per pixel")
    packed = torch.empty((V, nb, 4), dtype=torch.float32, device=dev)
    pix = torch.empty((V, H * W), dtype=torch.int32, device=dev)
    counts = torch.empty((V,), dtype=torch.int32, device=dev)
    status = torch.empty((V,), dtype=torch.int32, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_frame_select_ws_bytes(i32(V), i32(H), i32(W)), dev)
    check(L.gpn_frame_select(ptr(rows), ptr(valid), ptr(valid_counts), ptr(seeds), i32(V), i32(H), i32(W), i32(cap), i32(hash_bits),
                             i64(nb), ptr(packed), ptr(pix), ptr(counts), ptr(status), ptr(ws), szt(ws.numel()), _stream()),
          "gpn_frame_select")
    return packed, pix, counts, status


def frame_prepare(depth, rgb, K, m, cap, seeds, keep=None, depth_scale=1.0, flip=False, hash_bits=32, max_groups=0, sampler="fps"):
    """V RGB-D frames of one size -> the network's input (include/gpn.h sections FR and CP): gpn_frame_backproject,
    gpn_frame_select, gpn_view_fps (``sampler`` "grid": gpn_cloud_grid_sample with the presample's seeds) over at most ``cap`` rows a
    frame, gpn_cloud_finish; no host read between them and ONE at the
    end (counts, status, scale).  -> what cloud_prepare returns (a frame is the cloud of its H*W pixel rows; sample_rows are pixel
    indices), plus ``rows`` [V*H*W, 6] f32 and ``valid_counts`` [V] i32 on the device."""
    V, H, W = (int(v) for v in depth.shape)
    rows, valid, valid_counts = frame_backproject(depth, rgb, K, keep, depth_scale, flip)
    packed, pix, counts, status = frame_select(rows, valid, valid_counts, seeds, cap, hash_bits)
    off_dev = torch.tensor([v * H * W for v in range(V + 1)], dtype=torch.int64).to(rows.device, non_blocking=True)
    # (pix has the pitch H*W: gpn_cloud_finish bounds the row indices it reads by its n_bound)
    # (``hash_bits`` is the presample's: the grid sampler hashes with all 32 bits, as cloud_prepare does)
    got = _sample_and_finish(rows, 6, off_dev, V, packed, pix, H * W, counts, status, int(m), max_groups, sampler, seeds)
    got.update(rows=rows, valid_counts=valid_counts)
    return got


# ---------------------------------------------------------------------------------------------------- OB (object isolation)
ISOLATE_OK, ISOLATE_NO_PLANE, ISOLATE_EMPTY = 0, 1, 2
ISOLATE_SELECT = {"largest": 0, "center": 1, "all": 2}
ISOLATE_MAX_PLANES, ISOLATE_MAX_HYP, ISOLATE_TRIES = 4, 1024, 8
_dbl = _C.ctypes.c_double


def _frame_dims(t):
    if t.dim() != 3:
        raise _C.GpnError(f"a per-pixel frame tensor must be [V,H,W], got {tuple(t.shape)}")
    return (int(v) for v in t.shape)


def frame_candidates(rows, valid, z_min=0.0, z_max=float("inf")):
    """cand [V,H,W] u8 = valid && z_min <= |z| <= z_max (include/gpn.h section OB)"""
    dev = _dev(rows, valid)
    V, H, W = _frame_dims(valid)
    cand = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    check(_C.lib().gpn_frame_candidates(ptr(rows), ptr(valid), i32(V), i32(H), i32(W), _dbl(float(z_min)), _dbl(float(z_max)), ptr(cand),
                                        _stream()), "gpn_frame_candidates")
    return cand


def frame_plane_hypotheses(rows, cand, pix, valid_counts, seeds, n_hyp=256, round=0):
    """stage 1: -> (hyp [V, n_hyp, 4] f64, NaN where degenerate; hyp_pix [V, n_hyp] i32 = the pixel of p0 or -1); ``seeds``: [V]
    uint32 values or the int32 tensor of them"""
    dev = _dev(rows, cand, pix, valid_counts)
    V, H, W = _frame_dims(cand)
    seeds = seeds if torch.is_tensor(seeds) else _seed_tensor(seeds, V, dev)
    n_hyp = int(n_hyp)
    hyp = torch.empty((V, max(n_hyp, 0), 4), dtype=torch.float64, device=dev)
    hyp_pix = torch.empty((V, max(n_hyp, 0)), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_frame_plane_hypotheses(ptr(rows), ptr(cand), ptr(pix), ptr(valid_counts), ptr(seeds), i32(V), i32(H), i32(W),
                                              i32(n_hyp), i32(round), ptr(hyp), ptr(hyp_pix), _stream()), "gpn_frame_plane_hypotheses")
    return hyp, hyp_pix


def frame_plane_score(rows, cand, hyp, tol, variant=0):
    """stage 2: counts [V, n_hyp] i32 = the candidates within ``tol`` of every hypothesis"""
    dev = _dev(rows, cand, hyp)
    V, H, W = _frame_dims(cand)
    n_hyp = int(hyp.shape[1])
    counts = torch.empty((V, n_hyp), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_frame_plane_score(ptr(rows), ptr(cand), ptr(hyp), i32(V), i32(H), i32(W), i32(n_hyp), _dbl(float(tol)),
                                         i32(variant), ptr(counts), _stream()), "gpn_frame_plane_score")
    return counts


def frame_plane_winner(counts):
    """winner [V] i32: the hypothesis of the largest count, ties to the lowest; -1 when every count is 0"""
    dev = _dev(counts)
    V, n_hyp = (int(v) for v in counts.shape)
    winner = torch.empty((V,), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_frame_plane_winner(ptr(counts), i32(V), i32(n_hyp), ptr(winner), _stream()), "gpn_frame_plane_winner")
    return winner


def frame_plane_refit(rows, cand, hyp, hyp_pix, winner, tol, min_plane_fraction=0.1, round=0, max_planes=1, planes=None,
                      plane_inliers=None, n_planes=None):
    """stage 3: refit the winner on its inliers and accept it or not -> (planes [V, max_planes, 4] f64, plane_inliers
    [V, max_planes] i32, n_planes [V] i32); entry ``round`` is written (pass the three tensors of round 0 to the later rounds)"""
    dev = _dev(rows, cand, hyp, hyp_pix, winner)
    V, H, W = _frame_dims(cand)
    max_planes = int(max_planes)
    if planes is None:
        planes = torch.full((V, max(max_planes, 1), 4), float("nan"), dtype=torch.float64, device=dev)
        plane_inliers = torch.zeros((V, max(max_planes, 1)), dtype=torch.int32, device=dev)
        n_planes = torch.zeros((V,), dtype=torch.int32, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_frame_plane_refit_ws_bytes(i32(V), i32(H), i32(W)), dev)
    check(L.gpn_frame_plane_refit(ptr(rows), ptr(cand), ptr(hyp), ptr(hyp_pix), ptr(winner), i32(V), i32(H), i32(W), i32(hyp.shape[1]),
                                  _dbl(float(tol)), _dbl(float(min_plane_fraction)), i32(round), i32(max_planes), ptr(planes),
                                  ptr(plane_inliers), ptr(n_planes), ptr(ws), szt(ws.numel()), _stream()), "gpn_frame_plane_refit")
    return planes, plane_inliers, n_planes


def frame_plane_cut(rows, cand, planes, tol, round=0):
    """stage 4, IN PLACE on ``cand``: under an accepted plane of ``round`` only what lies more than ``tol`` on the camera's side stays"""
    _dev(rows, cand, planes)
    V, H, W = _frame_dims(cand)
    check(_C.lib().gpn_frame_plane_cut(ptr(rows), ptr(planes), i32(V), i32(H), i32(W), i32(planes.shape[1]), i32(round), _dbl(float(tol)),
                                       ptr(cand), _stream()), "gpn_frame_plane_cut")
    return cand


def frame_components(rows, cand, jump_abs=0.01, jump_rel=0.01, min_pixels=6):
    """stage 5: 4-connected components with the depth-continuity rule -> (labels [V,H,W] i32 = the component's smallest pixel, -1
    off the candidates; sizes [V, H*W] i32 at the roots; n_components [V] i32 of at least ``min_pixels`` pixels)"""
    dev = _dev(rows, cand)
    V, H, W = _frame_dims(cand)
    labels = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    sizes = torch.empty((V, H * W), dtype=torch.int32, device=dev)
    n_comp = torch.empty((V,), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_frame_components(ptr(rows), ptr(cand), i32(V), i32(H), i32(W), _dbl(float(jump_abs)), _dbl(float(jump_rel)),
                                        i32(min_pixels), ptr(labels), ptr(sizes), ptr(n_comp), _stream()), "gpn_frame_components")
    return labels, sizes, n_comp


def frame_component_select(labels, sizes, n_planes, select="largest", min_pixels=6, anchor=None):
    """stage 6: -> (keep [V,H,W] u8, chosen [V] i32 = the root or -1, status [V] i32 = ISOLATE_OK / _NO_PLANE / _EMPTY); ``anchor``
    [V,2] i32 (column, line) for select "center\""""
    dev = _dev(labels, sizes, n_planes, anchor)
    V, H, W = _frame_dims(labels)
    if select not in ISOLATE_SELECT:
        raise ValueError(f"select must be one of {tuple(ISOLATE_SELECT)}, got {select!r}")
    anchor = _c(anchor, torch.int32)
    if anchor is not None and anchor.numel() != V * 2:
        raise _C.GpnError("frame_component_select: anchor must be [V,2]")
    keep = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    chosen = torch.empty((V,), dtype=torch.int32, device=dev)
    status = torch.empty((V,), dtype=torch.int32, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_frame_component_select_ws_bytes(i32(V)), dev)
    check(L.gpn_frame_component_select(ptr(labels), ptr(sizes), ptr(n_planes), ptr(anchor), i32(V), i32(H), i32(W),
                                       i32(ISOLATE_SELECT[select]), i32(min_pixels), ptr(keep), ptr(chosen), ptr(status), ptr(ws),
                                       szt(ws.numel()), _stream()), "gpn_frame_component_select")
    return keep, chosen, status


def frame_isolate(rows, valid, valid_counts, seeds, max_planes=1, n_hyp=256, tol=0.005, min_plane_fraction=0.1, z_min=0.0,
                  z_max=float("inf"), jump_abs=0.01, jump_rel=0.01, select="largest", min_pixels=6, anchor=None):
    """the whole of section OB on what frame_backproject returned: candidates, ``max_planes`` rounds of hypotheses / score / winner /
    refit / cut, components, select.  No host read.  -> dict(keep, labels, sizes, planes, plane_inliers, n_planes, n_components,
    chosen, status), all on the device"""
    dev = _dev(rows, valid, valid_counts)
    V, H, W = _frame_dims(valid)
    seeds_t = _seed_tensor(seeds, V, dev)
    # (cap == 0: pix = the valid pixels ascending; the packed rows are not needed here)
    _, pix, _, _ = frame_select(rows, valid, valid_counts, np.asarray(seeds, dtype=np.int64), 0)
    cand = frame_candidates(rows, valid, z_min, z_max)
    planes = inl = n_planes = None
    for r in range(int(max_planes)):
        hyp, hyp_pix = frame_plane_hypotheses(rows, cand, pix, valid_counts, seeds_t, n_hyp, r)
        winner = frame_plane_winner(frame_plane_score(rows, cand, hyp, tol))
        planes, inl, n_planes = frame_plane_refit(rows, cand, hyp, hyp_pix, winner, tol, min_plane_fraction, r, max_planes, planes, inl,
                                                  n_planes)
        frame_plane_cut(rows, cand, planes, tol, r)
    if planes is None:
        raise ValueError("max_planes must be at least 1")
    labels, sizes, n_comp = frame_components(rows, cand, jump_abs, jump_rel, min_pixels)
    keep, chosen, status = frame_component_select(labels, sizes, n_planes, select, min_pixels, anchor)
    return dict(keep=keep, labels=labels, sizes=sizes, planes=planes, plane_inliers=inl, n_planes=n_planes, n_components=n_comp,
                chosen=chosen, status=status, cand=cand)


# ---------------------------------------------------------------------------------------------------- JE (joint estimation)
JOINT_TYPES = {"revolute": 0, "prismatic": 1}


def joint_sample(pc1, pc2, off1, off2, picks1, picks2, k1, k2):
    """pc1 [n1,3], pc2 [n2,3] f64 (pair b = rows off[b]:off[b+1], off [B+1] i64), picks [B,K] i64 (rows inside the segment), k [B]
    i32 live picks -> (X [B,K,3], Y [B,K,3], norm [B,4] = (S, Mx, My, Mz)), include/gpn.h section JE"""
    dev = _dev(pc1, pc2, off1, off2, picks1, picks2, k1, k2)
    f64 = torch.float64
    pc1, pc2 = _c(pc1, f64), _c(pc2, f64)
    off1, off2, picks1, picks2 = (_c(t, torch.int64) for t in (off1, off2, picks1, picks2))
    k1, k2 = _c(k1, torch.int32), _c(k2, torch.int32)
    B, K = (int(v) for v in picks1.shape)
    if tuple(picks2.shape) != (B, K) or off1.numel() != B + 1 or off2.numel() != B + 1 or k1.numel() != B or k2.numel() != B:
        raise _C.GpnError("joint_sample: picks [B,K] twice, offsets [B+1] twice, k [B] twice")
    X = torch.empty((B, K, 3), dtype=f64, device=dev)
    Y = torch.empty((B, K, 3), dtype=f64, device=dev)
    norm = torch.empty((B, 4), dtype=f64, device=dev)
    check(_C.lib().gpn_joint_sample(ptr(pc1), ptr(pc2), ptr(off1), ptr(off2), ptr(picks1), ptr(picks2), ptr(k1), ptr(k2), i64(B),
                                    i32(K), ptr(X), ptr(Y), ptr(norm), _stream()), "gpn_joint_sample")
    return X, Y, norm


def cpd_rigid(X, Y, nx, ny, max_iterations=100, tolerance=1e-3, w=0.0, scale=True, want_trace=False):
    """CPD rigid registration of Y [B,K,3] (ny[b] rows) onto X [B,K,3] (nx[b] rows), the whole EM loop of every pair in one launch
    (section JE) -> dict: s [B], R [B,3,3], t [B,3] (TY = s Y R + t), sigma2, q, diff [B], iterations [B] i32, and sigma2_trace
    [B,max_iterations] when asked for"""
    dev = _dev(X, Y, nx, ny)
    f64 = torch.float64
    X, Y, nx, ny = _c(X, f64), _c(Y, f64), _c(nx, torch.int32), _c(ny, torch.int32)
    if X.dim() != 3 or X.shape[2] != 3 or Y.shape != X.shape or nx.numel() != X.shape[0] or ny.numel() != X.shape[0]:
        raise _C.GpnError("cpd_rigid: X and Y [B,K,3], nx and ny [B]")
    B, K = int(X.shape[0]), int(X.shape[1])
    out = {"s": torch.empty(B, dtype=f64, device=dev), "R": torch.empty(B, 3, 3, dtype=f64, device=dev),
           "t": torch.empty(B, 3, dtype=f64, device=dev), "sigma2": torch.empty(B, dtype=f64, device=dev),
           "q": torch.empty(B, dtype=f64, device=dev), "diff": torch.empty(B, dtype=f64, device=dev),
           "iterations": torch.empty(B, dtype=torch.int32, device=dev)}
    if want_trace:
        out["sigma2_trace"] = torch.empty(B, int(max_iterations), dtype=f64, device=dev)
    dbl = _C.ctypes.c_double
    check(_C.lib().gpn_cpd_rigid(ptr(X), ptr(Y), ptr(nx), ptr(ny), i64(B), i32(K), i32(int(max_iterations)), dbl(float(tolerance)),
                                 dbl(float(w)), i32(1 if scale else 0), ptr(out["s"]), ptr(out["R"]), ptr(out["t"]),
                                 ptr(out["sigma2"]), ptr(out["q"]), ptr(out["diff"]), ptr(out["iterations"]),
                                 ptr(out.get("sigma2_trace")), _stream()), "gpn_cpd_rigid")
    return out


def joint_from_rigid(rotation, translation, norm, joint_type="revolute"):
    """rotation [G,3,3], translation [G,3], norm [G,4] f64 -> (axis [G,3], pivot [G,3], angle [G]), section JE"""
    dev = _dev(rotation, translation, norm)
    f64 = torch.float64
    rotation, translation, norm = _c(rotation, f64), _c(translation, f64), _c(norm, f64)
    G = int(translation.shape[0])
    if rotation.numel() != G * 9 or translation.numel() != G * 3 or norm.numel() != G * 4:
        raise _C.GpnError("joint_from_rigid: rotation [G,3,3], translation [G,3], norm [G,4]")
    if joint_type not in JOINT_TYPES:
        raise _C.GpnError(f"joint_from_rigid: joint_type is 'revolute' or 'prismatic', got {joint_type!r}")
    axis = torch.empty((G, 3), dtype=f64, device=dev)
    pivot = torch.empty((G, 3), dtype=f64, device=dev)
    angle = torch.empty((G,), dtype=f64, device=dev)
    check(_C.lib().gpn_joint_from_rigid(ptr(rotation), ptr(translation), ptr(norm), i64(G), i32(JOINT_TYPES[joint_type]), ptr(axis),
                                        ptr(pivot), ptr(angle), _stream()), "gpn_joint_from_rigid")
    return axis, pivot, angle


# ---------------------------------------------------------------------------------------------------- AR (articulation)
PARTS_MAX = 64


def _part_maps(inst, valid, what, top=PARTS_MAX):
    """inst [V,H,W] i32 / i64 (FramePrediction.instance is i64) and valid [V,H,W] u8 / bool -> contiguous i32 / u8; ``top``: the
    table's widest (a wider integer type is clamped to -1 .. top before the cast)"""
    V, H, W = _frame_dims(inst)
    if inst.dtype != torch.int32:
        if inst.dtype not in (torch.int64, torch.int16, torch.int8, torch.uint8):
            raise _C.GpnError(f"{what}: an instance map is an integer tensor, got {inst.dtype}")
        # (every value outside 0 .. top - 1 belongs to no part; a plain cast of an int64 would wrap, and so would -1 in an unsigned clamp)
        inst = inst.to(torch.int64).clamp(-1, top).to(torch.int32)
    if tuple(valid.shape) != (V, H, W):
        raise _C.GpnError(f"{what}: valid must be [V,H,W] like the instance map")
    return inst.contiguous(), _c(valid, torch.uint8), V, H, W


def _part_counts(n, V, dev, what):
    """[V] part counts (a tensor on the device, or host ints) -> i32 tensor on the device"""
    if torch.is_tensor(n):
        n = _c(n.to(dev, non_blocking=True), torch.int32)
    else:
        n = torch.tensor([int(x) for x in n], dtype=torch.int32).to(dev, non_blocking=True)
    if n.numel() != V:
        raise _C.GpnError(f"{what}: one part count per frame")
    return n


def _part_width(P, what):
    P = int(P)
    if not 0 <= P <= PARTS_MAX:
        raise _C.GpnError(f"{what}: a table width is 0 .. {PARTS_MAX}, got {P}")
    return P


def _part_classes(cls, V, P, dev, what):
    """ragged class lists (a sequence of V tensors / lists) or a [V,P] tensor -> [V,P] i32 on the device, -1 beyond a list's end"""
    if cls is None:
        return None
    if torch.is_tensor(cls):
        if tuple(cls.shape) != (V, P):
            raise _C.GpnError(f"{what}: a class table is [V,P]")
        return _c(cls.to(dev, non_blocking=True), torch.int32)
    if len(cls) != V:
        raise _C.GpnError(f"{what}: one class list per frame")
    table = torch.full((V, P), -1, dtype=torch.int32, device=dev)
    for v, c in enumerate(cls):  # (a list that lives on the device is padded there: no host read)
        c = torch.as_tensor(c).reshape(-1)
        if c.shape[0] > P:
            raise _C.GpnError(f"{what}: frame {v} has {c.shape[0]} classes, the table is {P} wide")
        if c.shape[0]:
            table[v, :c.shape[0]] = c.to(dev, non_blocking=True).to(torch.int32)
    return table


def parts_overlap(inst_a, valid_a, n_a, inst_b, valid_b, n_b, PA, PB):
    """the contingency table of two instance maps (include/gpn.h section AR): inst [V,H,W] i32 / i64, valid [V,H,W] u8 / bool,
    n [V] part counts, PA / PB the table widths -> (inter [V,PA,PB], area_a [V,PA], area_b [V,PB]) i32 on the device"""
    dev = _dev(inst_a, valid_a, inst_b, valid_b)
    inst_a, valid_a, V, H, W = _part_maps(inst_a, valid_a, "parts_overlap")
    inst_b, valid_b, Vb, Hb, Wb = _part_maps(inst_b, valid_b, "parts_overlap")
    if (Vb, Hb, Wb) != (V, H, W):
        raise _C.GpnError("parts_overlap: both frames of a pair have one size")
    PA, PB = _part_width(PA, "parts_overlap"), _part_width(PB, "parts_overlap")
    n_a, n_b = _part_counts(n_a, V, dev, "parts_overlap"), _part_counts(n_b, V, dev, "parts_overlap")
    inter = torch.empty((V, PA, PB), dtype=torch.int32, device=dev)
    area_a = torch.empty((V, PA), dtype=torch.int32, device=dev)
    area_b = torch.empty((V, PB), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_parts_overlap(ptr(inst_a), ptr(valid_a), ptr(n_a), ptr(inst_b), ptr(valid_b), ptr(n_b), i32(V), i32(H), i32(W),
                                     i32(PA), i32(PB), ptr(inter), ptr(area_a), ptr(area_b), _stream()), "gpn_parts_overlap")
    return inter, area_a, area_b


def parts_match(inter, area_a, area_b, n_a, n_b, cls_a=None, cls_b=None, min_iou=0.1):
    """greedy one-to-one matching by exact mask IoU (section AR): the tables of parts_overlap, n [V] part counts, cls = ragged class
    lists or [V,P] tables (None: all classes equal) -> dict(match_ab [V,PA], match_ba [V,PB], n_matched [V], inter [V,PA],
    union [V,PA]) i32 on the device"""
    dev = _dev(inter, area_a, area_b)
    if inter.dim() != 3:
        raise _C.GpnError("parts_match: inter is [V,PA,PB]")
    V, PA, PB = (int(v) for v in inter.shape)
    _part_width(PA, "parts_match"), _part_width(PB, "parts_match")
    inter, area_a, area_b = (_c(t, torch.int32) for t in (inter, area_a, area_b))
    if tuple(area_a.shape) != (V, PA) or tuple(area_b.shape) != (V, PB):
        raise _C.GpnError("parts_match: area_a [V,PA] and area_b [V,PB]")
    n_a, n_b = _part_counts(n_a, V, dev, "parts_match"), _part_counts(n_b, V, dev, "parts_match")
    cls_a, cls_b = _part_classes(cls_a, V, PA, dev, "parts_match"), _part_classes(cls_b, V, PB, dev, "parts_match")
    out = dict(match_ab=torch.empty((V, PA), dtype=torch.int32, device=dev), match_ba=torch.empty((V, PB), dtype=torch.int32, device=dev),
               n_matched=torch.empty((V,), dtype=torch.int32, device=dev), inter=torch.empty((V, PA), dtype=torch.int32, device=dev),
               union=torch.empty((V, PA), dtype=torch.int32, device=dev))
    check(_C.lib().gpn_parts_match(ptr(inter), ptr(area_a), ptr(area_b), ptr(n_a), ptr(n_b), ptr(cls_a), ptr(cls_b), _dbl(float(min_iou)),
                                   i32(V), i32(PA), i32(PB), ptr(out["match_ab"]), ptr(out["match_ba"]), ptr(out["n_matched"]),
                                   ptr(out["inter"]), ptr(out["union"]), _stream()), "gpn_parts_match")
    return out


def parts_gather(rows, inst, valid, n_parts, seg_start, n_total, out=None):
    """the matched parts' pixels as ragged clouds (section AR): rows [V*H*W,6] f32 of frame_backproject, inst / valid [V,H,W],
    n_parts [V], seg_start [V,P] i64 (negative: drop the part) -> pc [n_total,3] f64; rows no segment covers are not written
    (``out``: write into this tensor)"""
    dev = _dev(rows, inst, valid)
    inst, valid, V, H, W = _part_maps(inst, valid, "parts_gather")
    rows = _c(rows, torch.float32)
    if rows.numel() != V * H * W * 6 or seg_start.dim() != 2 or seg_start.shape[0] != V:
        raise _C.GpnError("parts_gather: one row per pixel and seg_start [V,P]")
    P = _part_width(seg_start.shape[1], "parts_gather")
    seg_start = _c(seg_start.to(dev, non_blocking=True), torch.int64)
    n_parts = _part_counts(n_parts, V, dev, "parts_gather")
    n_total = int(n_total)
    pc = torch.empty((n_total, 3), dtype=torch.float64, device=dev) if out is None else out
    if pc.dtype != torch.float64 or tuple(pc.shape) != (n_total, 3) or not pc.is_contiguous() or pc.device != dev:
        raise _C.GpnError("parts_gather: out must be a contiguous [n_total,3] float64 tensor on the frames' device")
    L = _C.lib()
    ws = _ws(L.gpn_parts_gather_ws_bytes(i32(V), i32(H), i32(W), i32(P)), dev)
    check(L.gpn_parts_gather(ptr(rows), ptr(inst), ptr(valid), ptr(n_parts), ptr(seg_start), i32(V), i32(H), i32(W), i32(P), i64(n_total),
                             ptr(pc), ptr(ws), szt(ws.numel()), _stream()), "gpn_parts_gather")
    return pc


# ---------------------------------------------------------------------------------------------------- MV (posed views)
VIEWS_MAX = 64
FUSE_PARTS_MAX = 512


def _view_dims(t, what):
    V, H, W = _frame_dims(t)
    if V > VIEWS_MAX:
        raise _C.GpnError(f"{what}: at most {VIEWS_MAX} views, got {V}")
    return V, H, W


def _fuse_width(GT, what):
    GT = int(GT)
    if not 0 <= GT <= FUSE_PARTS_MAX:
        raise _C.GpnError(f"{what}: at most {FUSE_PARTS_MAX} parts over all views, got {GT}")
    return GT


def views_world(rows, valid, inst, n_parts, R, t, GT):
    """member pixels -> the world frame (include/gpn.h section MV): rows [V*H*W,6] f32 and valid [V,H,W] u8 of frame_backproject
    (flip = 0), inst [V,H,W] i32 / i64, n_parts [V], R [V,3,3], t [V,3] f64 (a camera point is (world - t) @ R), GT = the table
    width -> (wrows [V*H*W,3] f32, part_of [V,H,W] i32, area [GT] i32, lo [3] f64) on the device"""
    dev = _dev(rows, valid, inst, R, t)
    _view_dims(inst, "views_world")
    GT = _fuse_width(GT, "views_world")
    inst, valid, V, H, W = _part_maps(inst, valid, "views_world", FUSE_PARTS_MAX)
    rows, R, t = _c(rows, torch.float32), _c(R, torch.float64), _c(t, torch.float64)
    if rows.numel() != V * H * W * 6 or R.numel() != V * 9 or t.numel() != V * 3:
        raise _C.GpnError("views_world: one row per pixel, R [V,3,3] and t [V,3]")
    n_parts = _part_counts(n_parts, V, dev, "views_world")
    wrows = torch.empty((V * H * W, 3), dtype=torch.float32, device=dev)
    part_of = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    area = torch.empty((GT,), dtype=torch.int32, device=dev)
    lo = torch.empty((3,), dtype=torch.float64, device=dev)
    check(_C.lib().gpn_views_world(ptr(rows), ptr(valid), ptr(inst), ptr(n_parts), ptr(R), ptr(t), i32(V), i32(H), i32(W), i32(GT),
                                   ptr(wrows), ptr(part_of), ptr(area), ptr(lo), _stream()), "gpn_views_world")
    return wrows, part_of, area, lo


def views_overlap(wrows, part_of, lo, cell, GT, want_keys=False):
    """the occupancy tables on the 1024-cell grid (section MV): -> (vol [GT], inter [GT,GT], dropped [V]) i32 on the device, and the
    pixels' keys [V,H,W] as int64 bit patterns with ``want_keys``"""
    dev = _dev(wrows, part_of, lo)
    V, H, W = _view_dims(part_of, "views_overlap")
    GT = _fuse_width(GT, "views_overlap")
    wrows, part_of, lo = _c(wrows, torch.float32), _c(part_of, torch.int32), _c(lo, torch.float64)
    if wrows.numel() != V * H * W * 3 or lo.numel() != 3:
        raise _C.GpnError("views_overlap: one world row per pixel and lo [3]")
    vol = torch.empty((GT,), dtype=torch.int32, device=dev)
    inter = torch.empty((GT, GT), dtype=torch.int32, device=dev)
    dropped = torch.empty((V,), dtype=torch.int32, device=dev)
    keys = torch.empty((V, H, W), dtype=torch.int64, device=dev) if want_keys else None
    L = _C.lib()
    ws = _ws(L.gpn_views_overlap_ws_bytes(i32(V), i32(H), i32(W)), dev)
    check(L.gpn_views_overlap(ptr(wrows), ptr(part_of), ptr(lo), _dbl(float(cell)), i32(V), i32(H), i32(W), i32(GT), ptr(vol), ptr(inter),
                              ptr(dropped), ptr(keys), ptr(ws), szt(ws.numel()), _stream()), "gpn_views_overlap")
    return (vol, inter, dropped, keys) if want_keys else (vol, inter, dropped)


def views_overlap_lds_parts(parts=-1):
    """the largest GT whose pair table gpn_views_overlap sums in LDS (negative: query)"""
    return int(_C.lib().gpn_views_overlap_lds_parts(i32(parts)))


def views_merge(inter, vol, cls, n_parts, min_inter=4, min_overlap=0.25):
    """the greedy single-linkage merge of section MV: inter [GT,GT], vol [GT], cls [GT] or None, n_parts [V] -> dict(fused_of [GT],
    n_fused [1], fused_views [GT] (uint64 bit patterns in int64), fused_class [GT], fused_vol [GT], fused_parts [GT,V], links [GT,3],
    n_links [1]) on the device"""
    dev = _dev(inter, vol)
    GT = _fuse_width(vol.numel(), "views_merge")
    inter, vol = _c(inter, torch.int32), _c(vol, torch.int32)
    if inter.numel() != GT * GT:
        raise _C.GpnError("views_merge: inter is [GT,GT]")
    V = len(n_parts)
    if V > VIEWS_MAX:
        raise _C.GpnError(f"views_merge: at most {VIEWS_MAX} views, got {V}")
    n_parts = _part_counts(n_parts, V, dev, "views_merge")
    if cls is not None:
        cls = _c(cls.to(dev, non_blocking=True), torch.int32)
        if cls.numel() != GT:
            raise _C.GpnError("views_merge: cls is [GT]")
    i32t = torch.int32
    out = dict(fused_of=torch.empty((GT,), dtype=i32t, device=dev), n_fused=torch.empty((1,), dtype=i32t, device=dev),
               fused_views=torch.empty((GT,), dtype=torch.int64, device=dev), fused_class=torch.empty((GT,), dtype=i32t, device=dev),
               fused_vol=torch.empty((GT,), dtype=i32t, device=dev), fused_parts=torch.empty((GT, V), dtype=i32t, device=dev),
               links=torch.empty((GT, 3), dtype=i32t, device=dev), n_links=torch.empty((1,), dtype=i32t, device=dev))
    check(_C.lib().gpn_views_merge(ptr(inter), ptr(vol), ptr(cls), ptr(n_parts), i32(V), i32(GT), i32(min_inter), _dbl(float(min_overlap)),
                                   ptr(out["fused_of"]), ptr(out["n_fused"]), ptr(out["fused_views"]), ptr(out["fused_class"]),
                                   ptr(out["fused_vol"]), ptr(out["fused_parts"]), ptr(out["links"]), ptr(out["n_links"]), _stream()),
          "gpn_views_merge")
    return out


def views_relabel(part_of, fused_of):
    """fused_inst [V,H,W] i32 = fused_of[part_of], or -1 (section MV)"""
    dev = _dev(part_of, fused_of)
    V, H, W = _view_dims(part_of, "views_relabel")
    part_of, fused_of = _c(part_of, torch.int32), _c(fused_of, torch.int32)
    GT = _fuse_width(fused_of.numel(), "views_relabel")
    fused_inst = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_views_relabel(ptr(part_of), ptr(fused_of), i32(V), i32(H), i32(W), i32(GT), ptr(fused_inst), _stream()),
          "gpn_views_relabel")
    return fused_inst


def views_gather(wrows, npcs, fused_inst, seg_start, n_total):
    """the fused parts' clouds (section MV): wrows [V*H*W,3] f32, npcs [V,H,W,3] f32 or None, fused_inst [V,H,W] i32, seg_start [F] i64
    (negative: drop the part) -> (xyz [M,3] f64, npcs_out [M,3] f64 or None, src [M] i64); rows no segment covers are not written"""
    dev = _dev(wrows, fused_inst)
    V, H, W = _view_dims(fused_inst, "views_gather")
    wrows, fused_inst = _c(wrows, torch.float32), _c(fused_inst, torch.int32)
    seg_start = _c(seg_start.to(dev, non_blocking=True), torch.int64).reshape(-1)
    F = _fuse_width(seg_start.numel(), "views_gather")
    M = int(n_total)
    if wrows.numel() != V * H * W * 3:
        raise _C.GpnError("views_gather: one world row per pixel")
    if npcs is not None:
        _dev(npcs)
        npcs = _c(npcs, torch.float32)
        if npcs.numel() != V * H * W * 3:
            raise _C.GpnError("views_gather: npcs is [V,H,W,3]")
    xyz = torch.empty((M, 3), dtype=torch.float64, device=dev)
    npcs_out = torch.empty((M, 3), dtype=torch.float64, device=dev) if npcs is not None else None
    src = torch.empty((M,), dtype=torch.int64, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_views_gather_ws_bytes(i32(V), i32(H), i32(W), i32(F)), dev)
    check(L.gpn_views_gather(ptr(wrows), ptr(npcs), ptr(fused_inst), ptr(seg_start), i32(V), i32(H), i32(W), i32(F), i64(M), ptr(xyz),
                             ptr(npcs_out), ptr(src), ptr(ws), szt(ws.numel()), _stream()), "gpn_views_gather")
    return xyz, npcs_out, src


# ---------------------------------------------------------------------------------------------------- PE (pose evaluation)
def pose_gt_fit(xyz, npcs, slot, scene_offsets, W):
    """xyz, npcs [N,3] f32, slot [N] i32 (scene * W + instance id, negative = none), scene_offsets [S+1] i64 -> dict per slot
    [S*W]: count i64, valid u8, scale, rotation [.,3,3], translation [.,3], half [.,3], bbox [.,8,3] f64 (section PE)"""
    dev = _dev(xyz, npcs, slot, scene_offsets)
    f64 = torch.float64
    xyz, npcs, slot, scene_offsets = _c(xyz, torch.float32), _c(npcs, torch.float32), _c(slot, torch.int32), _c(scene_offsets, torch.int64)
    N, S, W = int(slot.numel()), int(scene_offsets.numel()) - 1, int(W)
    if xyz.numel() != N * 3 or npcs.numel() != N * 3 or S < 0 or W < 0:
        raise _C.GpnError("pose_gt_fit: xyz and npcs [N,3], slot [N], scene_offsets [S+1], W >= 0")
    G = S * W
    out = {"count": torch.empty(G, dtype=torch.int64, device=dev), "valid": torch.empty(G, dtype=torch.uint8, device=dev),
           "scale": torch.empty(G, dtype=f64, device=dev), "rotation": torch.empty(G, 3, 3, dtype=f64, device=dev),
           "translation": torch.empty(G, 3, dtype=f64, device=dev), "half": torch.empty(G, 3, dtype=f64, device=dev),
           "bbox": torch.empty(G, 8, 3, dtype=f64, device=dev)}
    check(_C.lib().gpn_pose_gt_fit(ptr(xyz), ptr(npcs), ptr(slot), ptr(scene_offsets), i64(N), i32(S), i32(W), ptr(out["count"]),
                                   ptr(out["valid"]), ptr(out["scale"]), ptr(out["rotation"]), ptr(out["translation"]),
                                   ptr(out["half"]), ptr(out["bbox"]), _stream()), "gpn_pose_gt_fit")
    return out


def box_iou_3d(a, b):
    """exact IoU of P pairs of oriented boxes a, b [P,8,3] f64 (corner order of gpn_pose_fit's bbox) -> [P] f64; NaN for a
    non-finite corner or a zero extent (section PE, with the tie rule of the clipping)"""
    dev = _dev(a, b)
    a, b = _c(a, torch.float64), _c(b, torch.float64)
    if a.dim() != 3 or tuple(a.shape[1:]) != (8, 3) or a.shape != b.shape:
        raise _C.GpnError("box_iou_3d: a and b [P,8,3]")
    P = int(a.shape[0])
    iou = torch.empty(P, dtype=torch.float64, device=dev)
    check(_C.lib().gpn_box_iou_3d(ptr(a), ptr(b), i64(P), ptr(iou), _stream()), "gpn_box_iou_3d")
    return iou


def pose_pair_errors(pred, gt, sym_type, sym_table, sym_start, sym_count):
    """pred, gt = (scale [P], rotation [P,3,3], translation [P,3], half [P,3]) f64, sym_type [P] i32, sym_table [K,3,3] f64 with
    sym_start, sym_count [T] i32 -> dict: re_deg, te, se, iou [P] f64, k_re, k_iou [P] i32 (section PE)"""
    f64, i32t = torch.float64, torch.int32
    dev = _dev(*pred, *gt, sym_type, sym_table, sym_start, sym_count)
    pred, gt = [_c(t, f64) for t in pred], [_c(t, f64) for t in gt]
    sym_type, sym_table, sym_start, sym_count = _c(sym_type, i32t), _c(sym_table, f64), _c(sym_start, i32t), _c(sym_count, i32t)
    P, K, T = int(sym_type.numel()), int(sym_table.shape[0]), int(sym_start.numel())
    for side in (pred, gt):
        if [int(t.numel()) for t in side] != [P, P * 9, P * 3, P * 3]:
            raise _C.GpnError("pose_pair_errors: scale [P], rotation [P,3,3], translation [P,3], half [P,3] on both sides")
    if sym_table.numel() != K * 9 or sym_count.numel() != T:
        raise _C.GpnError("pose_pair_errors: sym_table [K,3,3], sym_start and sym_count [T]")
    out = {k: torch.empty(P, dtype=f64, device=dev) for k in ("re_deg", "te", "se", "iou")}
    out["k_re"], out["k_iou"] = torch.empty(P, dtype=i32t, device=dev), torch.empty(P, dtype=i32t, device=dev)
    check(_C.lib().gpn_pose_pair_errors(*(ptr(t) for t in pred), *(ptr(t) for t in gt), ptr(sym_type), i64(P), ptr(sym_table), i32(K),
                                        ptr(sym_start), ptr(sym_count), i32(T), ptr(out["re_deg"]), ptr(out["k_re"]), ptr(out["te"]),
                                        ptr(out["se"]), ptr(out["iou"]), ptr(out["k_iou"]), _stream()), "gpn_pose_pair_errors")
    return out


# ---------------------------------------------------------------------------------------------------- VS (test-time rendering)
VISU_RGB, VISU_LABEL, VISU_LABEL_MOD20, VISU_LABEL_MOD19P1, VISU_BLANK = 0, 1, 2, 3, 4
VISU_MAX_LAYERS = 16


class _VisuLayer(_C.ctypes.Structure):
    _fields_ = [("kind", _C.ctypes.c_int32), ("row", _C.ctypes.c_int32), ("col", _C.ctypes.c_int32),
                ("offset", _C.ctypes.c_float), ("src", _C.ctypes.c_void_p)]


def scene_maps(valid_indices, sorted_indices, proposal_offsets, npcs_valid_mask, npcs_preds, n_rows):
    """one batch's kept proposals -> (ins_map [N] i32, npcs_map [N,3] f32, fit_npcs [M,3] f32) (include/gpn.h section VS);
    any of the proposal tensors may be empty"""
    dev = _dev(valid_indices, sorted_indices, proposal_offsets, npcs_valid_mask, npcs_preds)
    vi, si, po = _c(valid_indices, torch.int64), _c(sorted_indices, torch.int64), _c(proposal_offsets, torch.int64)
    mask, preds = _c(npcs_valid_mask, torch.uint8), _c(npcs_preds, torch.float32)
    N, M, P = int(n_rows), int(si.shape[0]), max(int(po.shape[0]) - 1, 0)
    if mask.shape[0] != M or preds.dim() != 2 or preds.shape[1] != 3:
        raise _C.GpnError("scene_maps: npcs_valid_mask must be [M] and npcs_preds [Mv,3]")
    ins_map = torch.empty((N,), dtype=torch.int32, device=dev)
    npcs_map = torch.empty((N, 3), dtype=torch.float32, device=dev)
    fit_npcs = torch.empty((M, 3), dtype=torch.float32, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_scene_maps_ws_bytes(i64(N), i64(M)), dev)
    check(L.gpn_scene_maps(ptr(vi), i64(vi.shape[0]), ptr(si), ptr(po), i64(P), ptr(mask), i64(M), ptr(preds),
                           i64(preds.shape[0]), i64(N), ptr(ins_map), ptr(npcs_map), ptr(fit_npcs), ptr(ws), szt(ws.numel()),
                           _stream()), "gpn_scene_maps")
    return ins_map, npcs_map, fit_npcs


def _cam(fx, fy, u0, v0):
    d = _C.ctypes.c_double
    return d(float(fx)), d(float(fy)), d(float(u0)), d(float(v0))


def points_winner(xyz, scene_offsets, trans, H, W, fx, fy, u0, v0):
    """xyz [n,3] f32 (normalised frame, scenes as the CSR scene_offsets [S+1]), trans [S,4] f64 = (r, cx, cy, cz)
    -> winner [S,H,W] i32: the highest point index of the scene covering each pixel, -1 where none"""
    dev = _dev(xyz, scene_offsets, trans)
    xyz, off, trans = _c(xyz, torch.float32), _c(scene_offsets, torch.int64), _c(trans, torch.float64)
    S = int(off.shape[0]) - 1
    if S < 0 or trans.numel() != S * 4 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise _C.GpnError("points_winner: xyz must be [n,3], scene_offsets [S+1] and trans [S,4]")
    winner = torch.empty((S, int(H), int(W)), dtype=torch.int32, device=dev)
    check(_C.lib().gpn_points_winner(ptr(xyz), ptr(off), i64(xyz.shape[0]), ptr(trans), i32(S), i32(H), i32(W),
                                     *_cam(fx, fy, u0, v0), ptr(winner), _stream()), "gpn_points_winner")
    return winner


def points_paint(winner, scene_offsets, layers, palette, canvas, edge):
    """paints every layer of every scene into canvas [S,CH,CW,3] u8 in one launch.  layers: (kind, source, tile row, tile col[,
    offset]) with source a per-point tensor over all scenes' rows ([n,3] f32 for VISU_RGB, [n] i32 for the label kinds, None for
    VISU_BLANK); palette [K,3] u8"""
    dev = _dev(winner, scene_offsets, palette, canvas)
    S, H, W = winner.shape
    off = _c(scene_offsets, torch.int64)
    if canvas.dtype != torch.uint8 or not canvas.is_contiguous() or canvas.dim() != 4 or canvas.shape[0] != S or canvas.shape[3] != 3:
        raise _C.GpnError("points_paint: canvas must be a contiguous [S,CH,CW,3] uint8 tensor")
    if winner.dtype != torch.int32 or not winner.is_contiguous():
        raise _C.GpnError("points_paint: winner must be a contiguous int32 tensor")
    if len(layers) > VISU_MAX_LAYERS:
        raise _C.GpnError(f"points_paint: at most {VISU_MAX_LAYERS} layers per call")
    arr = (_VisuLayer * max(len(layers), 1))()
    keep = []
    for k, layer in enumerate(layers):
        kind, src, row, col = layer[:4]
        offset = float(layer[4]) if len(layer) > 4 else 0.0
        if kind != VISU_BLANK:
            _dev(src)
            src = _c(src, torch.float32 if kind == VISU_RGB else torch.int32)
            if (src.dim() != 2 or src.shape[1] != 3) if kind == VISU_RGB else src.dim() != 1:
                raise _C.GpnError("points_paint: a VISU_RGB source must be [n,3], a label source [n]")
            keep.append(src)
        arr[k] = _VisuLayer(int(kind), int(row), int(col), offset, src.data_ptr() if kind != VISU_BLANK else None)
    palette = _c(palette, torch.uint8)
    check(_C.lib().gpn_points_paint(ptr(winner), ptr(off), i32(S), i32(H), i32(W), arr, i32(len(layers)), ptr(palette),
                                    i32(palette.shape[0]), i32(edge), i32(canvas.shape[1]), i32(canvas.shape[2]), ptr(canvas),
                                    _stream()), "gpn_points_paint")
    return canvas


def boxes_draw(bbox, box_scene, trans, H, W, fx, fy, u0, v0, tiles, canvas, edge):
    """draws every box (bbox [Q,8,3] f64, normalised frame; box_scene [Q]) into the listed tiles [(row, col), ...] of its scene's
    panel in canvas [S,CH,CW,3] u8, box by box in the reference's draw order (include/gpn.h section VS: the line rule)"""
    dev = _dev(bbox, box_scene, trans, canvas)
    bbox, box_scene, trans = _c(bbox, torch.float64), _c(box_scene, torch.int32), _c(trans, torch.float64)
    Q, S = int(bbox.shape[0]), int(canvas.shape[0])
    if canvas.dtype != torch.uint8 or not canvas.is_contiguous() or canvas.dim() != 4 or canvas.shape[3] != 3:
        raise _C.GpnError("boxes_draw: canvas must be a contiguous [S,CH,CW,3] uint8 tensor")
    if tuple(bbox.shape[1:]) != (8, 3) or box_scene.shape[0] != Q or trans.numel() != S * 4:
        raise _C.GpnError("boxes_draw: bbox must be [Q,8,3], box_scene [Q] and trans [S,4]")
    flat = [int(v) for rc in tiles for v in rc]
    tiles_host = (_C.ctypes.c_int32 * max(len(flat), 1))(*flat)
    L = _C.lib()
    ws = _ws(L.gpn_boxes_draw_ws_bytes(i32(S), i32(H), i32(W)), dev)
    check(L.gpn_boxes_draw(ptr(bbox), ptr(box_scene), i64(Q), ptr(trans), i32(S), i32(H), i32(W), *_cam(fx, fy, u0, v0),
                           tiles_host, i32(len(tiles)), i32(edge), i32(canvas.shape[1]), i32(canvas.shape[2]), ptr(canvas),
                           ptr(ws), szt(ws.numel()), _stream()), "gpn_boxes_draw")
    return canvas


# ---------------------------------------------------------------------------------------------------- C16
# The opt-in bf16 INFERENCE ops (include/gpn.h section C16, csrc/spconv_bf16.hip): torch.bfloat16 tensors in and out, fp32
# accumulation, one round-to-nearest-even per stored activation.  No autograd: an input that requires grad is an error.
class _EpilogueBf16(_C.ctypes.Structure):
    _fields_ = [("mean", _C.ctypes.c_void_p), ("var", _C.ctypes.c_void_p), ("weight", _C.ctypes.c_void_p),
                ("bias", _C.ctypes.c_void_p), ("res", _C.ctypes.c_void_p), ("eps", _C.ctypes.c_float),
                ("relu", _C.ctypes.c_int32), ("out_f32", _C.ctypes.c_int32)]


def _inference_only(*tensors):
    for t in tensors:
        if t is not None and t.requires_grad:
            raise _C.GpnError("the bf16 ops are inference-only (no autograd): an input requires grad")


def _as_bf16(t, what):
    if t.dtype != torch.bfloat16:
        raise _C.GpnError(f"{what} must be a torch.bfloat16 tensor, got {t.dtype}")
    return t.contiguous()


def conv_pack_bf16(W, layout="kio"):
    """fp32 weight, canonical [K, Cin, Cout] ("kio") or parameter layout [Cout, K, Cin] ("oki"), -> the bf16 kernel's packed
    weight (flat bfloat16 tensor of K * Cin * Cout elements, each rounded to nearest even)"""
    dev = _dev(W)
    _inference_only(W)
    W = _c(W, torch.float32)
    K, cin, cout = _wdims(W, layout)
    packed = torch.empty((K * cin * cout,), dtype=torch.bfloat16, device=dev)
    check(_C.lib().gpn_spconv_pack_weights_bf16(ptr(W), i32(K), i32(cin), i32(cout), i32(LAYOUT_OKI if layout == "oki" else 0),
                                                ptr(packed), _stream()), "gpn_spconv_pack_weights_bf16")
    return packed


def conv_fwd_bf16(features, packed, rb: Rulebook, cin, cout, bn=None, res=None, relu=False, out_f32=False, out=None):
    """conv over ``rb`` (its tile order when it has one) on bf16 ``features`` [n_src, cin] and a ``conv_pack_bf16`` weight, with
    the fused epilogue: ``bn`` = (running_mean, running_var, weight, bias, eps) fp32 or None, ``res`` a bf16 [n_dst, cout]
    residual or None, ``relu``.  -> [n_dst, cout] bfloat16, or float32 (unrounded) with ``out_f32``.  ``out``: write there."""
    dev = _dev(features, packed)
    _inference_only(features, packed, res, *(bn[:4] if bn is not None else ()))
    features = _as_bf16(features, "features")
    packed = _as_bf16(packed, "packed weight")
    assert features.shape == (rb.n_src, cin), (features.shape, rb.n_src, cin)
    assert packed.numel() == rb.K * cin * cout, (packed.numel(), rb.K, cin, cout)
    ep = _EpilogueBf16(0, 0, 0, 0, 0, 0.0, 1 if relu else 0, 1 if out_f32 else 0)
    keep = []
    if bn is not None:
        mean, var, weight, bias, eps = bn
        keep = [_c(t, torch.float32) for t in (mean, var, weight, bias)]
        assert all(t.numel() == cout for t in keep)
        ep.mean, ep.var, ep.weight, ep.bias = (t.data_ptr() for t in keep)
        ep.eps = float(eps)
    if res is not None:
        res = _as_bf16(res, "residual")
        assert res.shape == (rb.n_dst, cout), (res.shape, rb.n_dst, cout)
        ep.res = res.data_ptr()
    if out is None:
        out = torch.empty((rb.n_dst, cout), dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    check(_C.lib().gpn_spconv_fwd_bf16(ptr(features), ptr(packed), ptr(rb.nbr), ptr(rb.nbr_p), ptr(rb.perm), i32(rb.K),
                                       i64(rb.n_dst), i32(cin), i32(cout), _C.ctypes.byref(ep), ptr(out), _stream()),
          "gpn_spconv_fwd_bf16")
    return out


def rows_to_bf16(x):
    """fp32 [n, C] -> bfloat16, round to nearest even"""
    dev = _dev(x)
    _inference_only(x)
    x = _c(x, torch.float32)
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=dev)
    check(_C.lib().gpn_rows_to_bf16(ptr(x), i64(x.shape[0]), i32(x.numel() // max(x.shape[0], 1)), ptr(y), _stream()),
          "gpn_rows_to_bf16")
    return y


def bn_act_bf16(x, weight, bias, running_mean, running_var, eps, relu, res=None):
    """eval-mode BatchNorm [+ bf16 residual] [+ ReLU] on a float32 or bfloat16 [N, C] tensor -> bfloat16 (the bf16 conv's
    epilogue arithmetic on a tensor no conv produced)"""
    dev = _dev(x)
    _inference_only(x, weight, bias, res)
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise _C.GpnError(f"bn_act_bf16 takes float32 or bfloat16 rows, got {x.dtype}")
    x = x.contiguous()
    N, C = x.shape
    pars = [_c(t, torch.float32) for t in (weight, bias, running_mean, running_var)]
    assert all(t.numel() == C for t in pars)
    if res is not None:
        res = _as_bf16(res, "residual")
        assert res.shape == x.shape
    y = torch.empty((N, C), dtype=torch.bfloat16, device=dev)
    check(_C.lib().gpn_bn_act_bf16(ptr(x), i32(1 if x.dtype == torch.float32 else 0), ptr(res), ptr(pars[0]), ptr(pars[1]),
                                   ptr(pars[2]), ptr(pars[3]), f32(eps), i64(N), i32(C), i32(1 if relu else 0), ptr(y), _stream()),
          "gpn_bn_act_bf16")
    return y


# ---------------------------------------------------------------------------------------------------- PM (PointNet dense layers)
def pointmlp_supported(cin: int, cout: int) -> bool:
    return bool(_C.lib().gpn_pointmlp_supported(i32(cin), i32(cout)))


def _host_offsets(offsets_host):
    if offsets_host is None:
        return None
    return (_C.ctypes.c_int64 * len(offsets_host))(*[int(v) for v in offsets_host])


def _pointmlp_x(x, view, N, cin, offsets_host):
    """-> (strided, sb, sc, sn) of gpn_pointmlp_*'s X~; a strided ``view`` = (sb, sc, sn) over the flat array ``x`` is checked
    against the array's size here (the kernels trust it), which takes the host copy of the offsets"""
    if view is None:
        assert x.dim() == 2 and x.shape == (N, cin), (tuple(x.shape), N, cin)
        return 0, 0, 0, 0
    sb, sc, sn = (int(v) for v in view)
    if offsets_host is None or min(sb, sc, sn) < 0:
        raise _C.GpnError("a strided point-MLP input needs the host copy of the segment offsets and non-negative strides")
    longest = max(offsets_host[s + 1] - offsets_host[s] for s in range(len(offsets_host) - 1))
    if (len(offsets_host) - 2) * sb + (cin - 1) * sc + (longest - 1) * sn >= x.numel():
        raise _C.GpnError("the strided point-MLP view reaches past its array")
    return 1, sb, sc, sn


def pointmlp_fwd(x, weight, bias=None, G=None, scale=None, shift=None, relu=False, offsets=None, offsets_host=None, view=None,
                 want_y=True, want_max=False):
    """epi(x~ W_s^T + bias + G[s]) of csrc/pointmlp.hip -> (Y [N, cout] or None, M [S, cout] or None).  ``weight`` [cout, cin] or
    [S, cout, cin]; ``offsets`` [S + 1] int64 on the device (None: one segment); ``view`` = (sb, sc, sn): x is a flat array
    read as (segment, channel, point)."""
    dev = _dev(x, weight)
    x, weight = _c(x, torch.float32), _c(weight, torch.float32)
    per_segment = weight.dim() == 3
    cout, cin = weight.shape[-2:]
    S = 1 if offsets is None else offsets.shape[0] - 1
    assert not per_segment or weight.shape[0] == S
    if offsets is not None:
        assert offsets.dtype == torch.int64 and offsets.is_cuda
        offsets = offsets.contiguous()
    N = x.shape[0] if view is None else int(offsets_host[-1])
    strided, sb, sc, sn = _pointmlp_x(x, view, N, cin, offsets_host)
    bias, G, scale, shift = (_c(t, torch.float32) for t in (bias, G, scale, shift))
    assert G is None or G.shape == (S, cout)
    y = torch.empty((N, cout), dtype=torch.float32, device=dev) if want_y else None
    m = torch.empty((S, cout), dtype=torch.float32, device=dev) if want_max else None
    check(_C.lib().gpn_pointmlp_fwd(ptr(x), i32(strided), i64(sb), i64(sc), i64(sn), ptr(weight), i32(per_segment), ptr(bias), ptr(G),
                                    ptr(scale), ptr(shift), i32(bool(relu)), ptr(offsets), _host_offsets(offsets_host), i64(S), i64(N),
                                    i32(cin), i32(cout), ptr(y), ptr(m), _stream()), "gpn_pointmlp_fwd")
    return y, m


def pointmlp_wgrad(x, dy, cin, offsets=None, offsets_host=None, view=None, per_segment=False, need_dw=True, need_db=False):
    """-> (dW [cout, cin] or [S, cout, cin] = dy^T x~, db [cout] = column sums of dy), either None when not needed"""
    dev = _dev(x, dy)
    x, dy = _c(x, torch.float32), _c(dy, torch.float32)
    N, cout = dy.shape
    S = 1 if offsets is None else offsets.shape[0] - 1
    strided, sb, sc, sn = _pointmlp_x(x, view, N, cin, offsets_host)
    dw = torch.empty(((S, cout, cin) if per_segment else (cout, cin)), dtype=torch.float32, device=dev) if need_dw else None
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if need_db else None
    if not (need_dw or need_db):
        return None, None
    L = _C.lib()
    ws = _ws(L.gpn_pointmlp_wgrad_ws_bytes(i64(N), i64(S), i32(cin), i32(cout)), dev)
    check(L.gpn_pointmlp_wgrad(ptr(x), i32(strided), i64(sb), i64(sc), i64(sn), ptr(dy), ptr(offsets), _host_offsets(offsets_host),
                               i64(S), i64(N), i32(cin), i32(cout), i32(bool(per_segment)), ptr(dw), ptr(db), ptr(ws), szt(ws.numel()),
                               _stream()), "gpn_pointmlp_wgrad")
    return dw, db


# ---------------------------------------------------------------------------------------------------- GR (grounding)
GROUND_MAX_K = 32
GROUND_MAX_CLASSES = 64
GROUND_MAX_SIDE = 4096
_GROUND_TABLES = {}


def ground_mask_resize(masks, size, tables):
    """binary masks [K,H,W] u8 / bool (non-zero = member) -> levels [K,Hf,Wf] u8 in 0..128 (0 = inside): Pillow's 8-bit bicubic
    resize of 128 (1 - m), byte for byte (include/gpn.h section GR).  ``size`` = (Hf, Wf); ``tables`` = (xbounds [Wf,2], xcoef
    [Wf,ksx], ybounds [Hf,2], ycoef [Hf,ksy]) int32 numpy arrays, Pillow's coefficient tables (misc/grounding.py:
    resample_tables).  They are uploaded once per (shape, device)."""
    dev = _dev(masks)
    if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool):
        raise _C.GpnError("ground_mask_resize: masks [K,H,W] of dtype uint8 or bool (float-valued masks are not supported)")
    masks = masks.contiguous()
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    K, H, W = (int(v) for v in masks.shape)
    Hf, Wf = int(size[0]), int(size[1])
    xb, xc, yb, yc = (np.ascontiguousarray(t, dtype=np.int32) for t in tables)
    if xb.shape != (Wf, 2) or yb.shape != (Hf, 2) or xc.ndim != 2 or yc.ndim != 2 or xc.shape[0] != Wf or yc.shape[0] != Hf:
        raise _C.GpnError("ground_mask_resize: tables are (xbounds [Wf,2], xcoef [Wf,ksx], ybounds [Hf,2], ycoef [Hf,ksy])")
    # (keyed by the caller's array objects, which the entry keeps alive: resample_tables hands out one tuple per shape)
    key = (dev.index,) + tuple(id(t) for t in tables)
    hit = _GROUND_TABLES.get(key)
    if hit is None:
        if len(_GROUND_TABLES) >= 64:  # (a caller that builds new tables every call must not grow the cache without bound)
            _GROUND_TABLES.clear()
        flat = np.concatenate([xb.reshape(-1), xc.reshape(-1), yb.reshape(-1), yc.reshape(-1)])
        hit = _GROUND_TABLES[key] = (torch.from_numpy(flat).to(dev), tuple(tables))
    tables_dev = hit[0]
    levels = torch.empty((K, Hf, Wf), dtype=torch.uint8, device=dev)
    L = _C.lib()
    ws = _ws(L.gpn_ground_mask_resize_ws_bytes(i32(K), i32(H), i32(Wf)), dev)
    hp = lambda a: _C.ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    check(L.gpn_ground_mask_resize(ptr(masks), i32(K), i32(H), i32(W), i32(Hf), i32(Wf), hp(xb), hp(xc), i32(xc.shape[1]), hp(yb),
                                   hp(yc), i32(yc.shape[1]), ptr(tables_dev), ptr(levels), ptr(ws), szt(ws.numel()), _stream()),
          "gpn_ground_mask_resize")
    return levels


def ground_mask_pool(feature_maps, levels, mask_view):
    """feature_maps [V,Hf,Wf,C] f32, levels [K,Hf,Wf] u8 (0..128, 0 = inside), mask_view [K] (the map of each mask) -> feat [K,C]
    f32 = max over the pixels of fea * ((128 - level) / 128), section GR"""
    dev = _dev(feature_maps, levels, mask_view)
    fea = _c(feature_maps, torch.float32)
    levels, mask_view = _c(levels, torch.uint8), _c(mask_view, torch.int32)
    if fea.dim() != 4 or levels.dim() != 3 or tuple(levels.shape[1:]) != tuple(fea.shape[1:3]) or mask_view.numel() != levels.shape[0]:
        raise _C.GpnError("ground_mask_pool: feature_maps [V,Hf,Wf,C], levels [K,Hf,Wf] of the maps' size, mask_view [K]")
    V, Hf, Wf, C = (int(v) for v in fea.shape)
    K = int(levels.shape[0])
    feat = torch.empty((K, C), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_ground_mask_pool(ptr(fea), ptr(levels), ptr(mask_view), i32(V), i32(Hf), i32(Wf), i32(C), i32(K), ptr(feat),
                                        _stream()), "gpn_ground_mask_pool")
    return feat


def ground_bank_norms(bank):
    """bank [M,D] f32 -> squared row norms [M] f32 (section GR; once per bank)"""
    dev = _dev(bank)
    bank = _c(bank, torch.float32)
    if bank.dim() != 2:
        raise _C.GpnError("ground_bank_norms: bank [M,D]")
    norms = torch.empty((bank.shape[0],), dtype=torch.float32, device=dev)
    check(_C.lib().gpn_ground_bank_norms(ptr(bank), i64(bank.shape[0]), i32(bank.shape[1]), ptr(norms), _stream()),
          "gpn_ground_bank_norms")
    return norms


def ground_knn(queries, bank, bank_norms, bank_labels, k, n_classes):
    """queries [Q,D], bank [M,D] f32 (contiguous), bank_norms [M] f32 (ground_bank_norms), bank_labels [M] i32 in [0, n_classes)
    -> (nn_index [Q,k] i32 ascending by (d2, row), nn_d2 [Q,k] f32, votes [Q,n_classes] i32, label [Q] i32), section GR.  The
    labels are on the device and are not read here: a bank is checked once where it is built (misc/grounding.PartGrounder)."""
    dev = _dev(queries, bank, bank_norms, bank_labels)
    queries = _c(queries, torch.float32)
    if (bank.dtype != torch.float32 or bank_norms.dtype != torch.float32 or bank_labels.dtype != torch.int32
            or not (bank.is_contiguous() and bank_norms.is_contiguous() and bank_labels.is_contiguous())):
        raise _C.GpnError("ground_knn: the bank is contiguous f32 [M,D] with f32 norms [M] and i32 labels [M]")
    if queries.dim() != 2 or bank.dim() != 2 or queries.shape[1] != bank.shape[1] or bank_norms.numel() != bank.shape[0] \
            or bank_labels.numel() != bank.shape[0]:
        raise _C.GpnError("ground_knn: queries [Q,D], bank [M,D], bank_norms [M], bank_labels [M]")
    Q, D, M, k, n_classes = int(queries.shape[0]), int(queries.shape[1]), int(bank.shape[0]), int(k), int(n_classes)
    L = _C.lib()
    # (bad k / M / D / n_classes: the library refuses them before any launch; outputs are sized only for sane values)
    ks, cs = min(max(k, 0), GROUND_MAX_K), min(max(n_classes, 0), GROUND_MAX_CLASSES)
    nn_index = torch.empty((Q, ks), dtype=torch.int32, device=dev)
    nn_d2 = torch.empty((Q, ks), dtype=torch.float32, device=dev)
    votes = torch.empty((Q, cs), dtype=torch.int32, device=dev)
    label = torch.empty((Q,), dtype=torch.int32, device=dev)
    ws = _ws(L.gpn_ground_knn_ws_bytes(i64(Q), i64(M), i32(k)), dev)
    check(L.gpn_ground_knn(ptr(queries), i64(Q), ptr(bank), ptr(bank_norms), ptr(bank_labels), i64(M), i32(D), i32(k), i32(n_classes),
                           ptr(nn_index), ptr(nn_d2), ptr(votes), ptr(label), ptr(ws), szt(ws.numel()), _stream()), "gpn_ground_knn")
    return nn_index, nn_d2, votes, label
