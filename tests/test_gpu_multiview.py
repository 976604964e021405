"""csrc/multiview.hip (include/gpn.h section MV) on the GPU against the restatement in tests/multiview_ref.py, entry point by entry
point.  Everything is integer work, an exact cast or float64 arithmetic in a fixed order, so every comparison is exact: world rows,
``lo`` and the voxel keys bit for bit.  Shapes: one wave and its border (1 x 63 / 64 / 65), exactly one chunk of 1024 pixels and one
pixel more (32 x 32, 25 x 41), 257 chunks a view with V = 2 - the seam of a 256-wide scan tile (512 x 514); V = 1, 2, 3, 64 (bit 63 of
the view mask); GT = 0, 1, 128 / 129 (the LDS and the global pair table), 511, 512; part counts with zeros in the middle.  Every
output sits in a buffer with sentinels behind it."""
import ctypes

import numpy as np
import pytest
import torch

from tests import multiview_ref as REF

pytestmark = pytest.mark.gpu
SENT, PAD = 0xA5, 256
FILL = -7.0
INT32_MIN = -2 ** 31


class Guarded:
    """a device buffer of ``shape`` filled with sentinel bytes, with PAD more of them behind it"""

    def __init__(self, shape, dtype, cuda):
        self.n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.n + PAD,), SENT, dtype=torch.uint8, device=cuda)
        self.t = self.raw[:self.n].view(dtype).view(shape)

    def check(self, what):
        assert bool((self.raw[self.n:] == SENT).all()), f"{what}: written past its end"


def _lib():
    from gapartnet_amd import _C
    from gapartnet_amd.hip_ops import _stream
    return _C, _C.lib(), _stream


def _finish(bufs):
    torch.cuda.synchronize()
    for name, b in bufs.items():
        b.check(name)
    return {k: b.t.cpu().numpy() for k, b in bufs.items()}


def _up(cuda, x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(cuda)


def run_world(cuda, rows, valid, inst, n_parts, R, t, GT):
    _C, L, _stream = _lib()
    V, H, W = inst.shape
    # (the inputs are held in locals until the call has run)
    r, va, i, n, Rd, td = (_up(cuda, rows, np.float32), _up(cuda, valid, np.uint8), _up(cuda, inst, np.int32), _up(cuda, n_parts, np.int32),
                           _up(cuda, R, np.float64), _up(cuda, t, np.float64))
    bufs = dict(wrows=Guarded((V * H * W, 3), torch.float32, cuda), part_of=Guarded((V, H, W), torch.int32, cuda),
                area=Guarded((GT,), torch.int32, cuda), lo=Guarded((3,), torch.float64, cuda))
    p = lambda name: _C.ptr(bufs[name].t)  # noqa: E731
    _C.check(L.gpn_views_world(_C.ptr(r), _C.ptr(va), _C.ptr(i), _C.ptr(n), _C.ptr(Rd), _C.ptr(td), _C.i32(V), _C.i32(H), _C.i32(W),
                               _C.i32(GT), p("wrows"), p("part_of"), p("area"), p("lo"), _stream()), "gpn_views_world")
    return _finish(bufs)


def run_overlap(cuda, wrows, part_of, lo, cell, GT):
    _C, L, _stream = _lib()
    V, H, W = part_of.shape
    w, po, l = _up(cuda, wrows, np.float32), _up(cuda, part_of, np.int32), _up(cuda, lo, np.float64)
    L.gpn_views_overlap_ws_bytes.restype = ctypes.c_size_t
    nbytes = int(L.gpn_views_overlap_ws_bytes(_C.i32(V), _C.i32(H), _C.i32(W)))
    bufs = dict(vol=Guarded((GT,), torch.int32, cuda), inter=Guarded((GT, GT), torch.int32, cuda), dropped=Guarded((V,), torch.int32, cuda),
                keys=Guarded((V, H, W), torch.int64, cuda), ws=Guarded((max(nbytes, 1),), torch.uint8, cuda))
    p = lambda name: _C.ptr(bufs[name].t)  # noqa: E731
    _C.check(L.gpn_views_overlap(_C.ptr(w), _C.ptr(po), _C.ptr(l), ctypes.c_double(cell), _C.i32(V), _C.i32(H), _C.i32(W), _C.i32(GT),
                                 p("vol"), p("inter"), p("dropped"), p("keys"), p("ws"), _C.szt(nbytes), _stream()), "gpn_views_overlap")
    out = _finish(bufs)
    out.pop("ws")
    out["keys"] = out["keys"].view(np.uint64)
    return out


MERGE_OUT = dict(fused_of=(1, torch.int32), n_fused=(0, torch.int32), fused_views=(1, torch.int64), fused_class=(1, torch.int32),
                 fused_vol=(1, torch.int32), fused_parts=(2, torch.int32), links=(3, torch.int32), n_links=(0, torch.int32))


def run_merge(cuda, inter, vol, cls, n_parts, min_inter, min_overlap):
    _C, L, _stream = _lib()
    GT, V = int(vol.shape[0]), len(n_parts)
    shape = {0: (1,), 1: (GT,), 2: (GT, V), 3: (GT, 3)}
    it, vo, n = _up(cuda, inter, np.int32), _up(cuda, vol, np.int32), _up(cuda, n_parts, np.int32)
    c = None if cls is None else _up(cuda, cls, np.int32)
    bufs = {k: Guarded(shape[kind], dt, cuda) for k, (kind, dt) in MERGE_OUT.items()}
    p = lambda name: _C.ptr(bufs[name].t)  # noqa: E731
    _C.check(L.gpn_views_merge(_C.ptr(it), _C.ptr(vo), _C.ptr(c), _C.ptr(n), _C.i32(V), _C.i32(GT), _C.i32(min_inter),
                               ctypes.c_double(min_overlap), p("fused_of"), p("n_fused"), p("fused_views"), p("fused_class"), p("fused_vol"),
                               p("fused_parts"), p("links"), p("n_links"), _stream()), "gpn_views_merge")
    out = _finish(bufs)
    out["fused_views"] = out["fused_views"].view(np.uint64)
    return out


def run_relabel(cuda, part_of, fused_of):
    _C, L, _stream = _lib()
    V, H, W = part_of.shape
    po, fo = _up(cuda, part_of, np.int32), _up(cuda, fused_of, np.int32)
    bufs = dict(fused_inst=Guarded((V, H, W), torch.int32, cuda))
    _C.check(L.gpn_views_relabel(_C.ptr(po), _C.ptr(fo), _C.i32(V), _C.i32(H), _C.i32(W), _C.i32(fused_of.shape[0]), _C.ptr(bufs["fused_inst"].t),
                                 _stream()), "gpn_views_relabel")
    return _finish(bufs)["fused_inst"]


def run_gather(cuda, wrows, npcs, fused_inst, seg_start, n_total):
    _C, L, _stream = _lib()
    V, H, W = fused_inst.shape
    F = len(seg_start)
    w, fi, sg = _up(cuda, wrows, np.float32), _up(cuda, fused_inst, np.int32), _up(cuda, seg_start, np.int64)
    nd = None if npcs is None else _up(cuda, npcs, np.float32)
    L.gpn_views_gather_ws_bytes.restype = ctypes.c_size_t
    nbytes = int(L.gpn_views_gather_ws_bytes(_C.i32(V), _C.i32(H), _C.i32(W), _C.i32(F)))
    bufs = dict(xyz=Guarded((n_total, 3), torch.float64, cuda), npcs=Guarded((n_total, 3), torch.float64, cuda),
                src=Guarded((n_total,), torch.int64, cuda), ws=Guarded((max(nbytes, 1),), torch.uint8, cuda))
    bufs["xyz"].t.fill_(FILL)
    bufs["npcs"].t.fill_(FILL)
    bufs["src"].t.fill_(int(FILL))
    _C.check(L.gpn_views_gather(_C.ptr(w), _C.ptr(nd), _C.ptr(fi), _C.ptr(sg), _C.i32(V), _C.i32(H), _C.i32(W), _C.i32(F), _C.i64(n_total),
                                _C.ptr(bufs["xyz"].t), _C.ptr(bufs["npcs"].t) if npcs is not None else _C.ptr(None), _C.ptr(bufs["src"].t),
                                _C.ptr(bufs["ws"].t), _C.szt(nbytes), _stream()), "gpn_views_gather")
    out = _finish(bufs)
    return out["xyz"], out["npcs"], out["src"]


# ---- random views ------------------------------------------------------------------------------------------------------------------------
def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def random_views(V, H, W, n_parts, seed, blobs=True):
    """camera rows in [-1, 1]^3 f32, 85 % valid, instance maps with every kind of non-member value; the maps are piecewise constant
    (``blobs``: runs of equal values, as real masks) or pixel noise"""
    rng = np.random.RandomState(seed)
    rows = np.zeros((V * H * W, 6), np.float32)
    rows[:, :3] = rng.uniform(-1, 1, (V * H * W, 3)).astype(np.float32)
    valid = (rng.uniform(size=(V, H, W)) < 0.85).astype(np.uint8)
    rows[valid.reshape(-1) == 0, :3] = np.nan
    inst = np.zeros((V, H, W), np.int32)
    for v in range(V):
        n = n_parts[v]
        pick = rng.randint(-1, n + 1, size=H * W)  # -1 and n: no part
        if blobs:
            pick = np.repeat(pick[::7], 7)[:H * W]
        pick = pick.astype(np.int64)
        pick[rng.uniform(size=H * W) < 0.02] = INT32_MIN
        inst[v] = pick.reshape(H, W).astype(np.int32)
    R = np.stack([_rotation(rng) for _ in range(V)]) if V else np.zeros((0, 3, 3))
    t = rng.uniform(-0.2, 0.2, (V, 3))
    return rows, valid, inst, R, t


CASES = {
    # name: (V, H, W, n_parts, cell)
    "wave-1": (1, 1, 63, [3], 0.5), "wave": (1, 1, 64, [3], 0.5), "wave+1": (2, 1, 65, [3, 2], 0.5),
    "chunk": (2, 32, 32, [4, 5], 0.3), "chunk+1": (3, 25, 41, [5, 0, 7], 0.3),
    "scan-seam": (2, 512, 514, [20, 20], 0.12),
    "gt0": (2, 4, 9, [0, 0], 0.5), "gt1": (1, 8, 8, [1], 0.5),
    "lds-128": (3, 16, 48, [43, 43, 42], 0.5), "global-129": (3, 16, 48, [43, 43, 43], 0.5),
    "v64-gt511": (64, 3, 21, [8] * 31 + [7] + [8] * 32, 0.6), "v64-gt512": (64, 3, 21, [8] * 64, 0.6),
    "zeros-in-the-middle": (5, 6, 11, [2, 0, 0, 3, 0], 0.5),
    "dropped": (2, 20, 30, [3, 3], 0.002),  # the clouds span about 1900 cells an axis: many pixels lie beyond the grid
}


@pytest.fixture(scope="module")
def pipeline_refs():
    return {}


def _reference(name, cache):
    if name not in cache:
        V, H, W, n_parts, cell = CASES[name]
        rows, valid, inst, R, t = random_views(V, H, W, n_parts, seed=len(name) * 7 + V, blobs=name != "chunk")
        rng = np.random.RandomState(5)
        GT = sum(n_parts)
        cls = rng.randint(1, 3, size=GT).astype(np.int32)
        npcs = rng.uniform(0, 1, (V, H, W, 3)).astype(np.float32)
        ref = REF.fuse(rows, valid, inst, n_parts, cls, R, t, cell, 1, 0.05, npcs=npcs, fast=V * H * W > 20000)
        cache[name] = dict(rows=rows, valid=valid, inst=inst, R=R, t=t, cls=cls, npcs=npcs, n_parts=n_parts, cell=cell, GT=GT, ref=ref)
    return cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_entry_point_equals_the_reference(cuda, name, pipeline_refs):
    """each entry point is fed the REFERENCE's output of the step before it, so one wrong step does not hide behind another"""
    c = _reference(name, pipeline_refs)
    ref, GT = c["ref"], c["GT"]
    member = ref["part_of"].reshape(-1) >= 0
    w = run_world(cuda, c["rows"], c["valid"], c["inst"], c["n_parts"], c["R"], c["t"], GT)
    np.testing.assert_array_equal(w["part_of"], ref["part_of"])
    np.testing.assert_array_equal(w["wrows"].view(np.uint32)[member], ref["wrows"].view(np.uint32)[member])
    assert np.isnan(w["wrows"][~member]).all()
    np.testing.assert_array_equal(w["area"], ref["area"])
    np.testing.assert_array_equal(w["lo"].view(np.uint64), ref["lo"].view(np.uint64))
    o = run_overlap(cuda, ref["wrows"], ref["part_of"], ref["lo"], c["cell"], GT)
    np.testing.assert_array_equal(o["keys"], ref["keys"])
    np.testing.assert_array_equal(o["dropped"], ref["dropped"])
    np.testing.assert_array_equal(o["vol"], ref["vol"])
    np.testing.assert_array_equal(o["inter"], ref["inter"])
    m = run_merge(cuda, ref["inter"], ref["vol"], c["cls"], c["n_parts"], 1, 0.05)
    for k in MERGE_OUT:
        np.testing.assert_array_equal(m[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(run_relabel(cuda, ref["part_of"], ref["fused_of"]), ref["fused_inst"])
    # gather: two rows of padding in front, three behind, the second fused part dropped
    F = int(ref["n_fused"][0])
    if F == 0:
        return
    seg, at = [], 2
    for f in range(F):
        if f == 1:
            seg.append(-1)
            continue
        seg.append(at)
        at += int(ref["n_points"][f])
    n_total = at + 3
    want = REF.gather(ref["wrows"], c["npcs"], ref["fused_inst"], seg, n_total, FILL)
    got = run_gather(cuda, ref["wrows"], c["npcs"], ref["fused_inst"], np.array(seg, np.int64), n_total)
    for g, x in zip(got, want):
        np.testing.assert_array_equal(g, x)
    assert (got[2][:2] == int(FILL)).all() and (got[2][-3:] == int(FILL)).all()


def test_the_cases_merge_and_refuse(pipeline_refs):
    """the reference's own results are not trivial: unions happen, and parts of one view that share voxels stay apart"""
    pass_through = _reference("chunk", pipeline_refs)["ref"]
    assert int(pass_through["n_links"][0]) > 0 and int(pass_through["n_fused"][0]) > 1
    r = _reference("v64-gt512", pipeline_refs)["ref"]
    assert int(r["n_links"][0]) > 50 and (r["fused_views"] >> np.uint64(63)).any()
    r = _reference("chunk+1", pipeline_refs)
    same_view = r["ref"]["inter"][:5, :5]
    assert same_view.sum() > 0  # two parts of one view in one voxel
    assert (r["ref"]["fused_parts"][:int(r["ref"]["n_fused"][0])] >= 0).sum(1).max() <= 3


# ---- voxel cases on hand-made world rows ---------------------------------------------------------------------------------------------------
def _overlap_both(cuda, wrows, part_of, lo, cell, GT):
    got = run_overlap(cuda, wrows, part_of, lo, cell, GT)
    keys, dropped = REF.keys(wrows, part_of, lo, cell, GT)
    vol, inter = REF.tables(keys, GT)
    np.testing.assert_array_equal(got["keys"], keys)
    np.testing.assert_array_equal(got["dropped"], dropped)
    np.testing.assert_array_equal(got["vol"], vol)
    np.testing.assert_array_equal(got["inter"], inter)
    return got


def test_all_pixels_in_one_voxel(cuda):
    rng = np.random.RandomState(0)
    V, H, W, GT = 2, 30, 37, 6
    wrows = rng.uniform(0.0, 0.999, (V * H * W, 3)).astype(np.float32)
    part_of = np.concatenate([rng.randint(-1, 3, (1, H, W)), rng.randint(3, 6, (1, H, W))]).astype(np.int32)
    got = _overlap_both(cuda, wrows, part_of, np.zeros(3), 1.0, GT)
    assert got["vol"].tolist() == [1] * 6 and got["inter"].sum() == 30


def test_one_voxel_seen_by_all_64_views_and_the_merge_of_it(cuda):
    """a run of 64 distinct parts in one voxel; every view holds one part, so all 64 fuse into one part whose view mask is all ones"""
    V, H, W = 64, 2, 3
    wrows = np.full((V * H * W, 3), 0.25, np.float32)
    part_of = np.repeat(np.arange(V, dtype=np.int32), H * W).reshape(V, H, W)
    got = _overlap_both(cuda, wrows, part_of, np.zeros(3), 1.0, V)
    assert (got["inter"] == 1 - np.eye(V, dtype=np.int32)).all()
    m = run_merge(cuda, got["inter"], got["vol"], None, [1] * V, 1, 0.5)
    want = REF.merge(got["inter"], got["vol"], None, [1] * V, 1, 0.5)
    for k in MERGE_OUT:
        np.testing.assert_array_equal(m[k], want[k], err_msg=k)
    assert int(m["n_fused"][0]) == 1 and m["fused_views"][0] == np.uint64(2 ** 64 - 1) and int(m["n_links"][0]) == 63
    # three views of it: the members of the one fused part come in (view, pixel) order
    fused_inst = np.zeros((3, H, W), np.int32)
    fused_inst[1, 0, 1] = -1
    xyz, _, src = run_gather(cuda, wrows[:3 * H * W], None, fused_inst, np.array([0], np.int64), 3 * H * W - 1)
    assert src.tolist() == [i for i in range(3 * H * W) if i != H * W + 1] and (xyz == 0.25).all()


def test_two_parts_of_one_view_in_one_voxel_stay_apart(cuda):
    wrows = np.full((2 * 4, 3), 0.5, np.float32)
    part_of = np.array([[[0, 0, 1, 1]], [[2, 2, 2, -1]]], np.int32)
    got = _overlap_both(cuda, wrows, part_of, np.zeros(3), 1.0, 3)
    m = run_merge(cuda, got["inter"], got["vol"], None, [2, 1], 1, 0.0)
    assert m["fused_of"].tolist() == [0, 1, 0] and m["links"][0].tolist() == [0, 2, 1] and int(m["n_links"][0]) == 1


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_grid_borders_on_each_axis(cuda, axis):
    """exactly at lo: index 0; index 1023 is kept (the top key bits of its axis), index 1024 is dropped and counted"""
    lo = np.array([-3.0, 5.0, 0.5])
    cell = 0.5
    at = lambda i: (lo[axis] + i * cell)  # noqa: E731 (exact in f32)
    coords = [at(0), at(1023), at(1023.5), at(1024), at(2000), np.nextafter(np.float32(at(1024)), np.float32(0))]
    wrows = np.tile(lo.astype(np.float32), (2 * len(coords), 1))
    wrows[:len(coords), axis] = coords
    wrows[len(coords):, axis] = coords
    part_of = np.array([[[0] * len(coords)], [[1] * len(coords)]], np.int32)
    got = _overlap_both(cuda, wrows, part_of, lo, cell, 2)
    assert got["dropped"].tolist() == [2, 2]
    shift = np.uint64(9 + 10 * (2 - axis))
    assert [int(k >> shift) for k in got["keys"][0, 0, [0, 1, 2, 5]]] == [0, 1023, 1023, 1023]
    assert (got["keys"][0, 0, [3, 4]] == REF.DEAD).all() and got["vol"].tolist() == [2, 2] and got["inter"][0, 1] == 2


def test_both_pair_table_forms_give_the_same_tables(cuda, pipeline_refs):
    """the LDS table and the global one: gpn_views_overlap_lds_parts moves the switch and is put back"""
    _C, L, _ = _lib()
    c = _reference("chunk", pipeline_refs)
    ref = c["ref"]
    before = L.gpn_views_overlap_lds_parts(_C.i32(-1))
    assert before == 128 and L.gpn_views_overlap_lds_parts(_C.i32(4096)) == 128
    try:
        assert L.gpn_views_overlap_lds_parts(_C.i32(0)) == 0
        o = run_overlap(cuda, ref["wrows"], ref["part_of"], ref["lo"], c["cell"], c["GT"])
    finally:
        L.gpn_views_overlap_lds_parts(_C.i32(before))
    np.testing.assert_array_equal(o["inter"], ref["inter"])
    np.testing.assert_array_equal(o["vol"], ref["vol"])


# ---- merge on random tables at the table widths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("GT,V", [(1, 1), (37, 3), (511, 64), (512, 64), (512, 1)])
def test_merge_on_random_tables(cuda, GT, V):
    rng = np.random.RandomState(GT + V)
    cut = np.sort(rng.randint(0, GT + 1, V - 1)) if V > 1 else np.zeros(0, np.int64)
    n_parts = np.diff(np.concatenate([[0], cut, [GT]])).tolist()
    vol = rng.randint(0, 40, GT).astype(np.int32)
    vol[rng.uniform(size=GT) < 0.1] = 0
    up = np.triu((rng.uniform(size=(GT, GT)) < min(1.0, 6.0 / GT)) * rng.randint(1, 12, (GT, GT)), 1)
    inter = np.minimum(up + up.T, np.minimum(vol[:, None], vol[None, :])).astype(np.int32)
    cls = rng.randint(0, 2, GT).astype(np.int32)
    got = run_merge(cuda, inter, vol, cls, n_parts, 2, 0.25)
    want = REF.merge(inter, vol, cls, n_parts, 2, 0.25)
    for k in MERGE_OUT:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    if GT > 1 and V > 1:
        assert int(want["n_links"][0]) > 0


def test_merge_when_only_the_index_breaks_the_ties(cuda):
    """every pair of the table has the same inter and every part the same volume: one ratio for all candidates, so each round's
    arg-max is decided by the tie rule alone (the smaller (g, h)), in the lanes, across the 16 waves - 130 rows put candidates
    in every wave - and against the empty candidate of a thread without one"""
    GT, V = 130, 64
    n_parts = [3, 3] + [2] * 62
    assert sum(n_parts) == GT
    vol = np.full(GT, 6, np.int32)
    inter = np.full((GT, GT), 3, np.int32)
    np.fill_diagonal(inter, 0)
    got = run_merge(cuda, inter, vol, None, n_parts, 1, 0.25)
    want = REF.merge(inter, vol, None, n_parts, 1, 0.25)
    for k in MERGE_OUT:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    links = want["links"][:int(want["n_links"][0])]
    assert len(links) > 60 and (links[:, 2] == 3).all() and (links[0, :2] == (0, 3)).all()


# ---- gather at more than 256 fused parts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_npcs", [False, True])
@pytest.mark.parametrize("V,H,W,F", [(2, 1, 1030, 300), (3, 5, 411, 512)])
def test_gather_of_more_than_256_fused_parts_over_several_chunks(cuda, V, H, W, F, with_npcs):
    """gpn_views_gather on a synthetic map (no merge behind it): more fused parts than the workgroup has threads, so the slot table
    is walked in more than one step, and pixel noise, so a wave ballots over many distinct 9-bit keys; more than one chunk a view.
    Keys run over -1 .. F (F itself is no part) with INT32_MIN among them, every part occurs; segments in a shuffled order, every
    fifth part dropped, padding rows in front and behind"""
    rng = np.random.RandomState(F)
    N = V * H * W
    assert F > 256 and H * W > 1024
    fused = rng.randint(-1, F + 1, N).astype(np.int64)
    at = rng.permutation(N)
    fused[at[:F]] = np.arange(F)
    fused[at[F:F + N // 50]] = INT32_MIN
    fused = fused.astype(np.int32).reshape(V, H, W)
    count = np.bincount(fused[(fused >= 0) & (fused < F)], minlength=F)
    assert (count > 0).all() and (fused == F).any() and (fused == -1).any()
    wrows = rng.standard_normal((N, 3)).astype(np.float32)
    npcs = rng.uniform(size=(V, H, W, 3)).astype(np.float32) if with_npcs else None
    seg, row = np.full(F, -1, np.int64), 2
    for f in rng.permutation(F):
        if f % 5 == 4:
            continue
        seg[f] = row
        row += int(count[f])
    n_total = row + 3
    want = REF.gather(wrows, npcs, fused, seg.tolist(), n_total, FILL)
    got = run_gather(cuda, wrows, npcs, fused, seg, n_total)
    for g, x in zip(got, want):
        np.testing.assert_array_equal(g, x)
    assert (got[2][:2] == int(FILL)).all() and (got[2][-3:] == int(FILL)).all() and (got[2][2:-3] >= 0).all()


# ---- argument errors and empty calls -------------------------------------------------------------------------------------------------------
def test_argument_errors_and_empty_calls(cuda):
    _C, L, _stream = _lib()
    z = ctypes.c_void_p(0)
    one = torch.zeros(64, dtype=torch.float64, device=cuda)
    p = _C.ptr(one)
    i = _C.i32
    # more than 512 parts, more than 64 views, a cell that is not positive: argument errors
    assert L.gpn_views_world(p, p, p, p, p, p, i(1), i(2), i(2), i(513), p, p, p, p, _stream()) == 1
    assert L.gpn_views_world(p, p, p, p, p, p, i(65), i(2), i(2), i(4), p, p, p, p, _stream()) == 1
    assert L.gpn_views_overlap(p, p, p, ctypes.c_double(0.0), i(1), i(2), i(2), i(4), p, p, p, z, p, _C.szt(1 << 20), _stream()) == 1
    assert L.gpn_views_overlap(p, p, p, ctypes.c_double(float("nan")), i(1), i(2), i(2), i(4), p, p, p, z, p, _C.szt(1 << 20), _stream()) == 1
    assert L.gpn_views_merge(p, p, z, p, i(1), i(513), i(1), ctypes.c_double(0.1), p, p, p, p, p, p, p, p, _stream()) == 1
    assert L.gpn_views_gather(p, z, p, p, i(1), i(2), i(2), i(513), _C.i64(4), p, z, p, p, _C.szt(64), _stream()) == 1
    # V == 0: nothing is launched on the maps; the tables are written empty
    lo = Guarded((3,), torch.float64, cuda)
    area = Guarded((4,), torch.int32, cuda)
    _C.check(L.gpn_views_world(z, z, z, z, z, z, i(0), i(2), i(2), i(4), z, z, _C.ptr(area.t), _C.ptr(lo.t), _stream()), "gpn_views_world")
    torch.cuda.synchronize()
    assert lo.t.tolist() == [0.0] * 3 and area.t.tolist() == [0] * 4
    lo.check("lo")
    area.check("area")
    m = run_merge(cuda, np.zeros((0, 0), np.int32), np.zeros(0, np.int32), None, [0, 0], 4, 0.25)
    assert int(m["n_fused"][0]) == 0 and int(m["n_links"][0]) == 0
