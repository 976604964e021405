"""csrc/articulate.hip (include/gpn.h section AR) on the GPU against the restatement in plain loops (tests/articulation_ref.py).
Everything is integer or an exact cast, so every comparison is exact.  Shapes: one wave and its border (1 x 63 / 64 / 65), exactly
one chunk of 1024 pixels and one pixel more (32 x 32, 25 x 41), 257 chunks - the seam of a 256-wide scan tile (512 x 514) - and the
table paddings 0 / 1 / 63 / 64.  Every output sits in a buffer with sentinels behind it."""
import ctypes

import numpy as np
import pytest
import torch

from gapartnet_amd.misc import articulation as AR
from gapartnet_amd.misc import joint_fitting as JF
from tests import articulation_ref as REF
from tests import articulation_scenes as SC

pytestmark = pytest.mark.gpu
SENT, PAD = 0xA5, 256
PC_SENT = -7.25
MIN_IOU = 0.05


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


def run_overlap_match(cuda, d, PA, PB, cls_a=None, cls_b=None, min_iou=MIN_IOU):
    """gpn_parts_overlap + gpn_parts_match into guarded buffers -> host arrays"""
    _C, L, _stream = _lib()
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(cuda)  # noqa: E731
    V, H, W = d["inst_a"].shape
    ia, ib, va, vb = t(d["inst_a"], np.int32), t(d["inst_b"], np.int32), t(d["valid_a"], np.uint8), t(d["valid_b"], np.uint8)
    na, nb = t(d["n_a"], np.int32), t(d["n_b"], np.int32)
    i32 = torch.int32
    bufs = dict(inter=Guarded((V, PA, PB), i32, cuda), area_a=Guarded((V, PA), i32, cuda), area_b=Guarded((V, PB), i32, cuda),
                match_ab=Guarded((V, PA), i32, cuda), match_ba=Guarded((V, PB), i32, cuda), n_matched=Guarded((V,), i32, cuda),
                m_inter=Guarded((V, PA), i32, cuda), m_union=Guarded((V, PA), i32, cuda))
    p = lambda name: _C.ptr(bufs[name].t)  # noqa: E731
    _C.check(L.gpn_parts_overlap(_C.ptr(ia), _C.ptr(va), _C.ptr(na), _C.ptr(ib), _C.ptr(vb), _C.ptr(nb), _C.i32(V), _C.i32(H), _C.i32(W),
                                 _C.i32(PA), _C.i32(PB), p("inter"), p("area_a"), p("area_b"), _stream()), "gpn_parts_overlap")
    ca = None if cls_a is None else t(cls_a, np.int32)
    cb = None if cls_b is None else t(cls_b, np.int32)
    _C.check(L.gpn_parts_match(p("inter"), p("area_a"), p("area_b"), _C.ptr(na), _C.ptr(nb), _C.ptr(ca), _C.ptr(cb), ctypes.c_double(min_iou),
                               _C.i32(V), _C.i32(PA), _C.i32(PB), p("match_ab"), p("match_ba"), p("n_matched"), p("m_inter"), p("m_union"),
                               _stream()), "gpn_parts_match")
    torch.cuda.synchronize()
    for name, b in bufs.items():
        b.check(name)
    return {k: b.t.cpu().numpy() for k, b in bufs.items()}


def run_gather(cuda, rows, inst, valid, n, seg_start, n_total):
    """gpn_parts_gather into a guarded buffer pre-filled with PC_SENT -> [n_total,3] f64 on the host"""
    _C, L, _stream = _lib()
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(cuda)  # noqa: E731
    V, H, W = inst.shape
    P = seg_start.shape[1]
    pc = Guarded((n_total, 3), torch.float64, cuda)
    pc.t.fill_(PC_SENT)
    nbytes = int(L.gpn_parts_gather_ws_bytes(_C.i32(V), _C.i32(H), _C.i32(W), _C.i32(P)))
    ws = Guarded((nbytes,), torch.uint8, cuda)
    # (the inputs are held in locals until the call has run: a temporary's memory would be handed to the next upload)
    r, i, va, nn, sg = t(rows, np.float32), t(inst, np.int32), t(valid, np.uint8), t(n, np.int32), t(seg_start, np.int64)
    _C.check(L.gpn_parts_gather(_C.ptr(r), _C.ptr(i), _C.ptr(va), _C.ptr(nn), _C.ptr(sg), _C.i32(V), _C.i32(H), _C.i32(W), _C.i32(P),
                                _C.i64(n_total), _C.ptr(pc.t), _C.ptr(ws.t), _C.szt(nbytes), _stream()), "gpn_parts_gather")
    torch.cuda.synchronize()
    pc.check("pc")
    ws.check("ws")
    return pc.t.cpu().numpy()


def _padded(lists, P):
    out = np.full((len(lists), P), -1, np.int32)
    for v, c in enumerate(lists):
        out[v, :len(c)] = c
    return out


def _special(kind):
    if kind == "one pair":       # every pixel of a 64 x 64 frame is pair (0, 0): maximal contention on one bin
        z = np.zeros((1, 64, 64), np.int32)
        return dict(inst_a=z, inst_b=z.copy(), valid_a=np.ones_like(z, np.uint8), valid_b=np.ones_like(z, np.uint8), n_a=[1], n_b=[1])
    r, c = np.meshgrid(np.arange(64, dtype=np.int32), np.arange(64, dtype=np.int32), indexing="ij")  # pixel (r, c) is pair (r, c)
    return dict(inst_a=r[None].copy(), inst_b=c[None].copy(), valid_a=np.ones((1, 64, 64), np.uint8), valid_b=np.ones((1, 64, 64), np.uint8),
                n_a=[64], n_b=[64])


CASES = {
    "1x1": lambda: SC.random_pair(1, 1, 1, 1, [2], [2], valid_rate=1.0),
    "1x63": lambda: SC.random_pair(2, 1, 1, 63, [5], [7], junk=True),
    "1x64": lambda: SC.random_pair(3, 1, 1, 64, [5], [7], junk=True),
    "1x65": lambda: SC.random_pair(4, 1, 1, 65, [5], [7], junk=True),
    "32x32": lambda: SC.random_pair(5, 1, 32, 32, [5], [7], junk=True),
    "25x41": lambda: SC.random_pair(6, 1, 25, 41, [5], [7], junk=True),
    "512x514": lambda: SC.random_pair(7, 1, 512, 514, [5], [7], junk=True),
    "parts 0 and 1": lambda: SC.random_pair(8, 1, 25, 41, [0], [1]),
    "parts 1 and 0": lambda: SC.random_pair(9, 1, 25, 41, [1], [0]),
    "parts 63 and 64": lambda: SC.random_pair(10, 1, 25, 41, [63], [64], junk=True),
    "parts 64 and 64": lambda: SC.random_pair(11, 1, 33, 33, [64], [64], junk=True),
    "ragged batch": lambda: SC.random_pair(12, 3, 25, 41, [0, 63, 64], [1, 64, 3], junk=True),
    "one pair": lambda: _special("one pair"),
    "every bin 1": lambda: _special("every bin 1"),
}
_cache = {}


def _case(name):
    """the case's maps, its class tables, and the restatement's tables per frame pair - computed once"""
    if name not in _cache:
        d = CASES[name]()
        V, H, W = d["inst_a"].shape
        if name == "512x514":    # part 0 of frame A has a pixel in every one of the 257 chunks
            flat_i, flat_v = d["inst_a"].reshape(V, -1), d["valid_a"].reshape(V, -1)
            flat_i[0, ::1024], flat_v[0, ::1024] = 0, 1
            assert len(range(0, H * W, 1024)) == 257
        PA, PB = max(d["n_a"]), max(d["n_b"])
        cls_a, cls_b = _padded(SC.class_lists(21, d["n_a"], 2), PA), _padded(SC.class_lists(22, d["n_b"], 2), PB)
        ref = []
        for v in range(V):
            inter, area_a, area_b = REF.overlap(d["inst_a"][v], d["valid_a"][v], d["n_a"][v], d["inst_b"][v], d["valid_b"][v], d["n_b"][v])
            taken = REF.match(inter, area_a, area_b, cls_a[v], cls_b[v], MIN_IOU)
            ref.append((REF.tables(d["inst_a"][v], d["valid_a"][v], d["n_a"][v], d["inst_b"][v], d["valid_b"][v], d["n_b"][v], PA, PB),
                        REF.match_tables(taken, PA, PB)))
        _cache[name] = (d, PA, PB, cls_a, cls_b, ref)
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_overlap_and_match_equal_the_restatement(cuda, name):
    d, PA, PB, cls_a, cls_b, ref = _case(name)
    got = run_overlap_match(cuda, d, PA, PB, cls_a, cls_b)
    for v, ((inter, area_a, area_b), (ab, ba, n, mi, mu)) in enumerate(ref):
        assert np.array_equal(got["inter"][v], inter) and np.array_equal(got["area_a"][v], area_a) and np.array_equal(got["area_b"][v], area_b), v
        assert np.array_equal(got["match_ab"][v], ab) and np.array_equal(got["match_ba"][v], ba) and got["n_matched"][v] == n, v
        assert np.array_equal(got["m_inter"][v], mi) and np.array_equal(got["m_union"][v], mu), v
    again = run_overlap_match(cuda, d, PA, PB, cls_a, cls_b)
    assert all(np.array_equal(got[k], again[k]) for k in got), "reruns are bit-equal"
    if name == "one pair":
        assert got["inter"][0, 0, 0] == 4096 and got["area_a"][0, 0] == 4096 and got["area_b"][0, 0] == 4096
    if name == "every bin 1":
        assert (got["inter"] == 1).all() and (got["area_a"] == 64).all() and (got["area_b"] == 64).all()
    if name == "512x514":
        assert got["n_matched"][0] > 0
    if name == "ragged batch":   # a frame pair alone = in the batch
        for v in range(3):
            one = {k: (x[v:v + 1] if isinstance(x, np.ndarray) else x[v:v + 1]) for k, x in d.items()}
            alone = run_overlap_match(cuda, one, PA, PB, cls_a[v:v + 1], cls_b[v:v + 1])
            assert all(np.array_equal(alone[k][0], got[k][v]) for k in got), v


def test_null_classes_mean_all_classes_equal(cuda):
    d, PA, PB, _, _, _ = _case("25x41")
    got = run_overlap_match(cuda, d, PA, PB)
    ones = run_overlap_match(cuda, d, PA, PB, np.ones((1, PA), np.int32), np.ones((1, PB), np.int32))
    assert all(np.array_equal(got[k], ones[k]) for k in got) and got["n_matched"][0] > 0
    inter, area_a, area_b = REF.overlap(d["inst_a"][0], d["valid_a"][0], d["n_a"][0], d["inst_b"][0], d["valid_b"][0], d["n_b"][0])
    ab = REF.match_tables(REF.match(inter, area_a, area_b, None, None, MIN_IOU), PA, PB)[0]
    assert np.array_equal(got["match_ab"][0], ab)


def test_match_when_only_the_index_breaks_the_ties(cuda):
    """gpn_parts_match on a 64 x 64 table whose pairs all have the same inter and whose parts all have the same area: one IoU for
    all 4096 candidates, so each round's arg-max is decided by the tie rule alone (the smaller (i, j)), in the lanes and across waves"""
    _C, L, _stream = _lib()
    P = 64
    inter, area = np.full((P, P), 5, np.int32), np.full(P, 10, np.int32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(cuda)  # noqa: E731
    it, aa, ab, n = t(inter[None]), t(area[None]), t(area[None]), t([P])
    bufs = {k: Guarded(shape, torch.int32, cuda) for k, shape in dict(match_ab=(1, P), match_ba=(1, P), n_matched=(1,), m_inter=(1, P),
                                                                     m_union=(1, P)).items()}
    p = lambda name: _C.ptr(bufs[name].t)  # noqa: E731
    _C.check(L.gpn_parts_match(_C.ptr(it), _C.ptr(aa), _C.ptr(ab), _C.ptr(n), _C.ptr(n), _C.ptr(None), _C.ptr(None), ctypes.c_double(MIN_IOU),
                               _C.i32(1), _C.i32(P), _C.i32(P), p("match_ab"), p("match_ba"), p("n_matched"), p("m_inter"), p("m_union"),
                               _stream()), "gpn_parts_match")
    torch.cuda.synchronize()
    for name, b in bufs.items():
        b.check(name)
    got = {k: b.t.cpu().numpy() for k, b in bufs.items()}
    areas = {i: 10 for i in range(P)}
    taken = REF.match({(i, j): 5 for i in range(P) for j in range(P)}, areas, areas, None, None, MIN_IOU)
    ab_, ba_, n_, mi, mu = REF.match_tables(taken, P, P)
    assert n_ == P and np.array_equal(ab_, np.arange(P)), "the restatement matches (i, i), in that order"
    assert np.array_equal(got["match_ab"][0], ab_) and np.array_equal(got["match_ba"][0], ba_) and got["n_matched"][0] == n_
    assert np.array_equal(got["m_inter"][0], mi) and np.array_equal(got["m_union"][0], mu)


@pytest.mark.parametrize("name", ["1x1", "1x64", "1x65", "32x32", "25x41", "512x514", "parts 63 and 64", "parts 64 and 64", "ragged batch",
                                  "every bin 1"])
def test_gather_equals_the_restatement(cuda, name):
    """segments in an order that is not the part order, some parts dropped (seg_start = -1), parts of 0 and 1 pixels among them, a gap
    before the first segment and one behind the last: every row of pc outside the segments keeps its sentinel"""
    d, _, _, _, _, _ = _case(name)
    inst, valid, n = d["inst_a"], d["valid_a"], d["n_a"]
    V, H, W = inst.shape
    P = max(max(n), 1)
    rng = np.random.RandomState(3)
    rows = rng.randn(V * H * W, 6).astype(np.float32)
    parts = {v: REF.gather_all(rows[v * H * W:(v + 1) * H * W, :3], inst[v], valid[v], n[v]) for v in range(V)}
    order = [(v, p) for v in range(V) for p in range(n[v])]
    rng.shuffle(order)
    dropped = set(order[::4][1:])   # (every fourth part, but never the first of the order)
    seg = np.full((V, P), -1, np.int64)
    want, at = [np.full((2, 3), PC_SENT)], 2
    for v, p in order:
        if (v, p) in dropped:
            continue
        seg[v, p] = at
        want.append(parts[v][p])
        at += len(parts[v][p])
    want = np.concatenate(want + [np.full((3, 3), PC_SENT)])
    got = run_gather(cuda, rows, inst, valid, n, seg, len(want))
    assert np.array_equal(got, want)
    assert np.array_equal(run_gather(cuda, rows, inst, valid, n, seg, len(want)), got), "reruns are bit-equal"
    sizes = [len(parts[v][p]) for v, p in order]
    if name in ("25x41", "512x514"):
        assert max(sizes) > 64
    if name == "parts 63 and 64":
        assert 0 in sizes or 1 in sizes, "a part of 0 or 1 pixels"
    if name == "512x514":
        px = np.flatnonzero((inst[0].reshape(-1) == 0) & (valid[0].reshape(-1) != 0))
        assert len(np.unique(px // 1024)) == 257 and seg[0, 0] >= 0, "a kept part with pixels in all 257 chunks"
    if name == "ragged batch":   # a frame alone = in the batch
        for v in range(V):
            if n[v] == 0:
                continue
            alone = run_gather(cuda, rows[v * H * W:(v + 1) * H * W], inst[v:v + 1], valid[v:v + 1], n[v:v + 1], seg[v:v + 1], len(want))
            mine = np.full_like(want, PC_SENT)
            for p in range(n[v]):
                if seg[v, p] >= 0:
                    mine[seg[v, p]:seg[v, p] + len(parts[v][p])] = parts[v][p]
            assert np.array_equal(alone, mine), v


def test_argument_errors_and_empty_calls(cuda):
    _C, L, _stream = _lib()
    z = torch.zeros(64, dtype=torch.int32, device=cuda)
    p, i32 = _C.ptr(z), _C.i32
    nul = _C.ptr(None)
    assert L.gpn_parts_overlap(p, p, p, p, p, p, i32(1), i32(2), i32(2), i32(65), i32(1), p, p, p, _stream()) == 1
    assert b"bad argument" in L.gpn_last_error()
    assert L.gpn_parts_overlap(p, p, p, p, p, p, i32(65536), i32(2), i32(2), i32(1), i32(1), p, p, p, _stream()) == 1
    assert L.gpn_parts_overlap(p, p, p, p, p, p, i32(1), i32(16385), i32(2), i32(1), i32(1), p, p, p, _stream()) == 1
    assert L.gpn_parts_overlap(nul, p, p, p, p, p, i32(1), i32(2), i32(2), i32(1), i32(1), p, p, p, _stream()) == 1
    assert L.gpn_parts_match(p, p, p, p, p, nul, nul, ctypes.c_double(0.1), i32(1), i32(1), i32(65), p, p, p, p, p, _stream()) == 1
    assert L.gpn_parts_match(nul, p, p, p, p, nul, nul, ctypes.c_double(0.1), i32(1), i32(1), i32(1), p, p, p, p, p, _stream()) == 1
    assert L.gpn_parts_gather(p, p, p, p, p, i32(1), i32(2), i32(2), i32(65), _C.i64(4), p, nul, _C.szt(0), _stream()) == 1
    assert L.gpn_parts_gather(p, p, p, p, p, i32(1), i32(2), i32(2), i32(2), _C.i64(4), nul, nul, _C.szt(0), _stream()) == 1
    assert L.gpn_parts_gather(p, p, p, p, p, i32(1), i32(64), i32(64), i32(2), _C.i64(4), p, nul, _C.szt(0), _stream()) == 2, "no workspace"
    # counts of 0 launch nothing and need no pointers
    assert L.gpn_parts_overlap(nul, nul, nul, nul, nul, nul, i32(0), i32(2), i32(2), i32(4), i32(4), nul, nul, nul, _stream()) == 0
    assert L.gpn_parts_match(nul, nul, nul, nul, nul, nul, nul, ctypes.c_double(0.1), i32(0), i32(4), i32(4), nul, nul, nul, nul, nul, _stream()) == 0
    assert L.gpn_parts_gather(nul, nul, nul, nul, nul, i32(0), i32(2), i32(2), i32(4), _C.i64(0), nul, nul, _C.szt(0), _stream()) == 0
    assert int(L.gpn_parts_gather_ws_bytes(i32(0), i32(2), i32(2), i32(4))) == 0
    torch.cuda.synchronize()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
def test_match_parts_on_the_gpu_equals_the_cpu_path(cuda):
    """int64 maps as FramePrediction has them, with values a plain cast to int32 would wrap into a part"""
    d = SC.random_pair(31, 3, 25, 41, [0, 6, 64], [2, 5, 64], junk=True)
    cls_a, cls_b = SC.class_lists(5, d["n_a"], 2), SC.class_lists(6, d["n_b"], 2)
    ia, ib = d["inst_a"].astype(np.int64), d["inst_b"].astype(np.int64)
    ia[1, 0, :7], ib[1, 0, :7] = 2 ** 32, 2 ** 32 + 1
    t = torch.from_numpy
    for va, vb in ((None, None), (t(d["valid_a"]), t(d["valid_b"]))):
        want = AR.match_parts(t(ia), t(ib), cls_a, cls_b, va, vb, MIN_IOU)
        got = AR.match_parts(t(ia).to(cuda), t(ib).to(cuda), [t(c).to(cuda) for c in cls_a], cls_b, None if va is None else va.to(cuda),
                             None if vb is None else vb.to(cuda), MIN_IOU)
        for f in ("pairs", "inter", "union", "iou", "unmatched_a", "unmatched_b", "area_a", "area_b"):
            for v in range(3):
                assert np.array_equal(getattr(got, f)[v], getattr(want, f)[v]), (f, v)
        assert sum(len(p) for p in got.pairs) > 0


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int8, torch.int16])
def test_narrow_integer_maps_match_as_on_the_cpu(cuda, dtype):
    """an unsigned map has no -1: 255 (and 200) belong to no part, as every value at or above the part count"""
    d = SC.random_pair(41, 2, 25, 41, [4, 6], [5, 3])
    cls_a, cls_b = SC.class_lists(7, d["n_a"], 2), SC.class_lists(8, d["n_b"], 2)
    ia, ib = (torch.from_numpy(np.where(d[k] < 0, 200 if dtype == torch.uint8 else -1, d[k])).to(dtype) for k in ("inst_a", "inst_b"))
    va, vb = torch.from_numpy(d["valid_a"]), torch.from_numpy(d["valid_b"])
    want = AR.match_parts(torch.from_numpy(d["inst_a"]), torch.from_numpy(d["inst_b"]), cls_a, cls_b, va, vb, MIN_IOU)
    for dev in ("cpu", cuda):
        got = AR.match_parts(ia.to(dev), ib.to(dev), cls_a, cls_b, va.to(dev), vb.to(dev), MIN_IOU)
        for f in ("pairs", "inter", "union", "area_a", "area_b"):
            for v in range(2):
                assert np.array_equal(getattr(got, f)[v], getattr(want, f)[v]), (dev, f, v)
    assert sum(len(p) for p in want.pairs) > 0 and sum(int(a.sum()) for a in want.area_a) > 0


@pytest.fixture(scope="module")
def scene():
    return SC.cabinet_scene()


def _scene_args(s, dev):
    t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    sizes1 = [int((s["inst_a"] == i).sum()) for i in range(3)]
    sizes2 = [int((s["inst_b"] == s["partner"][i]).sum()) for i in range(3)]
    picks, ransac = SC.whole_picks(sizes1, sizes2, 256)
    args = (t(s["depth_a"]), t(s["depth_b"]), s["K"], t(s["inst_a"]), t(s["inst_b"]), s["classes_a"], s["classes_b"])
    return args, dict(sample_number=256, picks=picks, ransac_picks=ransac)


def _sync_count(fn):
    """the synchronising torch calls fn() makes, as torch's sync debug mode reports them"""
    import warnings
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in caught)


def _cut_clouds(scene, cuda, args):
    """the three pairs' clouds by boolean indexing of the back-projected rows: ([A's parts 0, 1, 2], [B's parts 2, 0, 1])"""
    from gapartnet_amd import hip_ops
    K = torch.from_numpy(scene["K"])[None].to(cuda)
    clouds = []
    for depth, inst, parts in ((args[0], args[3], [0, 1, 2]), (args[1], args[4], [2, 0, 1])):
        rows, valid, _ = hip_ops.frame_backproject(depth[None], torch.zeros((1, 48, 64, 3), dtype=torch.uint8, device=cuda), K)
        xyz = rows[:, :3]
        clouds.append([xyz[((inst == p) & (valid[0] != 0)).reshape(-1)].double() for p in parts])
    return clouds


def test_articulation_from_maps_equals_one_joint_pass_on_the_cut_out_clouds(cuda, scene):
    args, kw = _scene_args(scene, cuda)
    art = AR.articulation_from_maps(*args, **kw)
    assert art.part_a.tolist() == [0, 1, 2] and art.part_b.tolist() == [2, 0, 1] and art.joint_type == ["revolute", "prismatic", "fixed"]
    # the same pairs' clouds by boolean indexing, one estimate_joints call with the same picks
    clouds = _cut_clouds(scene, cuda, args)
    est = JF.estimate_joints(clouds[0], clouds[1], sample_number=256, picks=kw["picks"], ransac_picks=kw["ransac_picks"])
    eq = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))  # noqa: E731
    assert torch.equal(art.iterations, est.iterations) and torch.equal(art.norm, est.norm)
    for mine, ref in ((art.cpd, est.cpd), (art.ransac, est.ransac)):
        for f in ("scale", "rotation", "translation"):
            assert eq(getattr(mine, f), getattr(ref, f)), f
        p_axis, p_pivot, p_angle = JF.joint_from_rigid(ref.rotation[1:2], ref.translation[1:2], est.norm[1:2], "prismatic")
        assert eq(mine.axis[0], ref.axis[0]) and eq(mine.pivot[0], ref.pivot[0]) and eq(mine.angle[0], ref.angle[0])
        assert eq(mine.axis[1], p_axis[0]) and eq(mine.pivot[1], p_pivot[0]) and eq(mine.angle[1], p_angle[0])
        assert bool(torch.isnan(mine.axis[2]).all()) and bool(torch.isnan(mine.pivot[2]).all()) and bool(torch.isnan(mine.angle[2]))
    assert bool(torch.isfinite(art.cpd.axis[:2]).all()) and abs(np.rad2deg(float(art.cpd.angle[0])) - 24.0) <= 1.0
    # the CPU path: the same integer fields
    cpu_args, cpu_kw = _scene_args(scene, "cpu")
    cpu = AR.articulation_from_maps(*cpu_args, **cpu_kw)
    for f in ("frame", "part_a", "part_b", "part_class", "n_points_a", "n_points_b", "iou2d"):
        assert np.array_equal(getattr(art, f), getattr(cpu, f)), f
    assert art.joint_type == cpu.joint_type and torch.equal(art.iterations.cpu(), cpu.iterations)
    for f in ("pairs", "inter", "union", "area_a", "area_b", "unmatched_a", "unmatched_b"):
        assert np.array_equal(getattr(art.matches, f)[0], getattr(cpu.matches, f)[0]), f
    again = AR.articulation_from_maps(*args, **kw)
    assert eq(again.cpd.axis, art.cpd.axis) and eq(again.ransac.pivot, art.ransac.pivot), "reruns are bit-equal"


def test_articulation_from_maps_reads_the_host_once_in_front_of_the_joint_pass(cuda, scene):
    """the joint pass by itself (``estimate_joints_packed`` on the same clouds) makes its own synchronising calls; the whole call adds
    exactly one: the read of the match and area tables"""
    args, kw = _scene_args(scene, cuda)
    art = AR.articulation_from_maps(*args, **kw)   # (warm-up: first calls build caches)
    sizes1, sizes2 = art.n_points_a.tolist(), art.n_points_b.tolist()
    pc1, pc2 = (torch.cat(c) for c in _cut_clouds(scene, cuda, args))
    assert pc1.shape[0] == sum(sizes1) and pc2.shape[0] == sum(sizes2)
    joint = lambda: JF.estimate_joints_packed(pc1, pc2, sizes1, sizes2, 256, kw["picks"], kw["ransac_picks"])  # noqa: E731
    joint()
    n_joint, n_all = _sync_count(joint), _sync_count(lambda: AR.articulation_from_maps(*args, **kw))
    print(f"synchronising calls: the joint pass {n_joint}, articulation_from_maps {n_all}")
    assert n_all == n_joint + 1
    n_match = _sync_count(lambda: AR.match_parts(args[3], args[4], scene["classes_a"], scene["classes_b"]))
    assert n_match == 1
