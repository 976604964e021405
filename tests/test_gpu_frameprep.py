"""csrc/frameprep.hip (include/gpn.h section FR) on the GPU against the numpy restatement (tests/frame_ref.py): every output
exactly - integers equal, floats bit-equal - with sentinel bytes behind every output buffer and in every slot the contract leaves
unwritten.  m = 32 samples and cap = 128 unless said otherwise."""
import ctypes

import numpy as np
import pytest
import torch

from tests import frame_ref as F

pytestmark = pytest.mark.gpu
M, CAP = 32, 128
PAD, SENT = 256, 0xA5
SIZES = [(1, 1), (1, 65), (3, 64), (16, 16), (37, 53), (256, 257)]   # the last spans 65 compaction chunks of 1024 pixels
KINDS = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint16): 2}


class Guarded:
    """a device buffer of ``shape`` filled with sentinel bytes, with PAD more of them behind it"""

    def __init__(self, shape, dtype, cuda):
        self.n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.n + PAD,), SENT, dtype=torch.uint8, device=cuda)
        self.t = self.raw[:self.n].view(dtype).view(shape)

    def check(self, what):
        assert bool((self.raw[self.n:] == SENT).all()), f"{what}: written past its end"

    def untouched(self, index):
        """the bytes of self.t[index] are still sentinels"""
        part = self.t[index].contiguous().view(torch.uint8)
        return bool((part == SENT).all())


def run_kernels(cuda, depth, rgb, K, seeds, cap, keep=None, depth_scale=1.0, flip=False, hash_bits=32):
    """gpn_frame_backproject + gpn_frame_select into guarded buffers -> host arrays"""
    from gapartnet_amd import _C
    from gapartnet_amd.hip_ops import _stream
    L = _C.lib()
    V, H, W = depth.shape
    HW = H * W
    nb = cap if cap > 0 else HW
    d = torch.from_numpy(depth).to(cuda)
    c = torch.from_numpy(rgb).to(cuda)
    k = torch.from_numpy(np.ascontiguousarray(K, dtype=np.float64)).to(cuda)
    kp = None if keep is None else torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8)).to(cuda)
    sd = torch.from_numpy(np.asarray(seeds, dtype=np.int64).astype(np.uint32).view(np.int32)).to(cuda)
    rows, valid, vcount = Guarded((V * HW, 6), torch.float32, cuda), Guarded((V, HW), torch.uint8, cuda), Guarded((V,), torch.int32, cuda)
    packed, pix = Guarded((V, nb, 4), torch.float32, cuda), Guarded((V, HW), torch.int32, cuda)
    counts, status = Guarded((V,), torch.int32, cuda), Guarded((V,), torch.int32, cuda)
    _C.check(L.gpn_frame_backproject(_C.ptr(d), _C.i32(KINDS[depth.dtype]), ctypes.c_double(depth_scale), _C.ptr(c), _C.ptr(kp), _C.ptr(k),
                                     _C.i32(V), _C.i32(H), _C.i32(W), _C.i32(int(flip)), _C.ptr(rows.t), _C.ptr(valid.t), _C.ptr(vcount.t),
                                     _stream()), "gpn_frame_backproject")
    nbytes = int(L.gpn_frame_select_ws_bytes(_C.i32(V), _C.i32(H), _C.i32(W)))
    ws = Guarded((nbytes,), torch.uint8, cuda)
    _C.check(L.gpn_frame_select(_C.ptr(rows.t), _C.ptr(valid.t), _C.ptr(vcount.t), _C.ptr(sd), _C.i32(V), _C.i32(H), _C.i32(W), _C.i32(cap),
                                _C.i32(hash_bits), _C.i64(nb), _C.ptr(packed.t), _C.ptr(pix.t), _C.ptr(counts.t), _C.ptr(status.t),
                                _C.ptr(ws.t), _C.szt(nbytes), _stream()), "gpn_frame_select")
    torch.cuda.synchronize()
    bufs = dict(rows=rows, valid=valid, valid_counts=vcount, packed=packed, pix=pix, counts=counts, status=status, ws=ws)
    for name, b in bufs.items():
        b.check(name)
    return bufs


def check_against_restatement(bufs, depth, rgb, K, seeds, cap, keep=None, depth_scale=1.0, flip=False, hash_bits=32):
    V, H, W = depth.shape
    HW = H * W
    rows = bufs["rows"].t.cpu().numpy()
    valid = bufs["valid"].t.cpu().numpy()
    packed, pix = bufs["packed"].t.cpu().numpy(), bufs["pix"].t.cpu().numpy()
    counts, status, vcount = (bufs[k].t.cpu().numpy() for k in ("counts", "status", "valid_counts"))
    for v in range(V):
        w_rows, w_valid = F.backproject_np(depth[v], rgb[v], K[v], None if keep is None else keep[v], depth_scale, flip)
        g_rows, hole = rows[v * HW:(v + 1) * HW], np.isnan(w_rows)
        assert np.array_equal(np.isnan(g_rows), hole), v
        assert np.array_equal(g_rows.view(np.uint32)[~hole], w_rows.view(np.uint32)[~hole]), v
        assert np.array_equal(valid[v] != 0, w_valid) and set(np.unique(valid[v])) <= {0, 1} and vcount[v] == w_valid.sum(), v
        kept = F.select_np(w_valid, seeds[v], cap, hash_bits)
        n = kept.shape[0]
        assert n == (min(int(w_valid.sum()), cap) if cap > 0 else int(w_valid.sum()))
        assert counts[v] == n and status[v] == (F.OK if n else F.EMPTY), (v, counts[v], n)
        assert np.array_equal(pix[v, :n], kept), v
        assert np.array_equal(packed[v, :n, :3].view(np.uint32), w_rows[kept, :3].view(np.uint32)), v
        assert (packed[v, :n, 3] == np.float32(1e10)).all(), v
        # nothing is written past the count
        assert bufs["packed"].untouched((v, slice(n, None))) and bufs["pix"].untouched((v, slice(n, None))), v


def frames_with_valid_counts(H, W, wanted, seed):
    """one frame per feasible entry of ``wanted`` ('all' or a count <= H*W) with exactly that many valid pixels at random places;
    an empty frame is put second (in the middle of the batch); a different camera and seed per frame"""
    HW = H * W
    ns = [HW if n == "all" else n for n in wanted if n == "all" or n <= HW]
    ns = [n for i, n in enumerate(ns) if n not in ns[:i]]
    if 0 in ns and len(ns) > 2:
        ns.remove(0)
        ns.insert(1, 0)
    V = len(ns)
    depth, rgb, K = F.synthetic_frames(V, H, W, seed=seed, hole=0.0)
    rng = np.random.RandomState(seed + 1)
    for v, n in enumerate(ns):
        off = rng.permutation(HW)[n:]
        depth[v].reshape(-1)[off] = 0
    seeds = [(0x9e3779b1 * (v + 1) + seed) & 0xffffffff for v in range(V)]
    return depth, rgb, K, seeds, ns


@pytest.mark.parametrize("hash_bits", [32, 1])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_sizes_and_valid_counts(cuda, size, hash_bits):
    H, W = size
    depth, rgb, K, seeds, ns = frames_with_valid_counts(H, W, [0, 1, M - 1, M, CAP - 1, CAP, CAP + 1, "all"], seed=H * 1000 + W)
    assert (depth > 0).reshape(len(ns), -1).sum(1).tolist() == ns
    bufs = run_kernels(cuda, depth, rgb, K, seeds, CAP, hash_bits=hash_bits)
    check_against_restatement(bufs, depth, rgb, K, seeds, CAP, hash_bits=hash_bits)


def _batch3(kind, bad=False):
    """V = 3 frames of 37 x 53 with a different K per frame and the empty frame in the middle"""
    depth, rgb, K = F.synthetic_frames(3, 37, 53, seed=17)
    depth[1] = 0
    scale = 1.0
    if bad:
        rng = np.random.RandomState(3)
        flat = depth.reshape(-1)
        where = rng.choice(flat.shape[0], 400, replace=False)
        flat[where] = rng.choice(np.asarray([np.nan, np.inf, -np.inf, -1.5, 0.0, -0.0, 3.0e38, 1e-30], np.float32), size=400)
        depth[1] = rng.choice(np.asarray([np.nan, np.inf, -np.inf, -1.5, 0.0, -0.0], np.float32), size=depth[1].shape)   # still empty
    if kind == "f64":
        depth = depth.astype(np.float64)
        if bad:
            depth[0, 1, :3] = [1e300, 1e39, -1e300]   # finite float64 that overflow float32: no point
    elif kind == "u16":
        depth, scale = np.rint(depth * 1000).astype(np.uint16), 1000.0
        depth[0, 0, :4] = [0, 1, 65535, 32768]
    return depth, rgb, K, scale


@pytest.mark.parametrize("kind,bad,use_keep,flip,hash_bits,seeds", [
    ("f32", False, False, False, 32, [0, 1, 0xffffffff]),
    ("f64", False, True, True, 4, [0xffffffff, 5, 0]),
    ("u16", False, True, False, 1, [7, 0, 0xffffffff]),
    ("f32", True, False, True, 32, [0, 0xffffffff, 9]),
    ("f64", True, True, False, 4, [11, 12, 13]),
])
def test_depth_types_bad_depth_options_ties_and_seeds(cuda, kind, bad, use_keep, flip, hash_bits, seeds):
    depth, rgb, K, scale = _batch3(kind, bad)
    keep = None
    if use_keep:
        keep = (np.random.RandomState(5).rand(*depth.shape) < 0.8).astype(np.uint8) * 200
    bufs = run_kernels(cuda, depth, rgb, K, seeds, CAP, keep=keep, depth_scale=scale, flip=flip, hash_bits=hash_bits)
    check_against_restatement(bufs, depth, rgb, K, seeds, CAP, keep=keep, depth_scale=scale, flip=flip, hash_bits=hash_bits)
    got = [int(v) for v in bufs["counts"].t.cpu()]
    assert got[0] == CAP and got[1] == 0 and got[2] == CAP, "frames 0 and 2 are cut by the presample, frame 1 is empty"
    # two reruns are bit-equal
    for _ in range(2):
        again = run_kernels(cuda, depth, rgb, K, seeds, CAP, keep=keep, depth_scale=scale, flip=flip, hash_bits=hash_bits)
        for name in ("rows", "valid", "valid_counts", "packed", "pix", "counts", "status"):
            assert torch.equal(bufs[name].raw, again[name].raw), name


@pytest.mark.parametrize("size", [(37, 53), (256, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_presample_off_equals_cloud_pack_bit_for_bit(cuda, size):
    from gapartnet_amd import _C
    from gapartnet_amd.hip_ops import _stream
    H, W = size
    HW = H * W
    depth, rgb, K = F.synthetic_frames(3, H, W, seed=23)
    depth[1] = 0
    bufs = run_kernels(cuda, depth, rgb, K, [1, 2, 3], 0)
    check_against_restatement(bufs, depth, rgb, K, [1, 2, 3], 0)
    V = 3
    off = torch.tensor([v * HW for v in range(V + 1)], dtype=torch.int64, device=cuda)
    packed, rows = Guarded((V, HW, 4), torch.float32, cuda), Guarded((V, HW), torch.int32, cuda)
    counts, status = Guarded((V,), torch.int32, cuda), Guarded((V,), torch.int32, cuda)
    _C.check(_C.lib().gpn_cloud_pack(_C.ptr(bufs["rows"].t), _C.i64(V * HW), _C.i32(6), _C.ptr(off), _C.i32(V), _C.i64(HW), _C.ptr(packed.t),
                                     _C.ptr(rows.t), _C.ptr(counts.t), _C.ptr(status.t), _stream()), "gpn_cloud_pack")
    torch.cuda.synchronize()
    # (unwritten slots hold the same sentinels on both sides: the whole buffers are compared)
    assert torch.equal(packed.raw, bufs["packed"].raw) and torch.equal(rows.raw, bufs["pix"].raw)
    assert torch.equal(counts.raw, bufs["counts"].raw) and torch.equal(status.raw, bufs["status"].raw)


@pytest.mark.parametrize("size,cap", [((37, 53), CAP), ((256, 257), CAP), ((256, 257), 0), ((64, 80), 2048)],
                         ids=lambda s: str(s).replace(" ", ""))
def test_frame_prepare_equals_cloud_prepare_on_the_masked_rows(cuda, size, cap):
    """the chain: back-projection, presample, gpn_view_fps over the packed rows, gpn_cloud_finish"""
    from gapartnet_amd import hip_ops
    H, W = size
    HW = H * W
    depth, rgb, K = F.synthetic_frames(3, H, W, seed=31)
    depth[1] = 0
    depth[2].reshape(-1)[np.random.RandomState(1).permutation(HW)[M - 5:]] = 0     # fewer valid pixels than m: all kept
    seeds = [4, 5, 0xffffffff]
    keep = (np.random.RandomState(6).rand(3, H, W) < 0.9)
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    got = hip_ops.frame_prepare(t(depth), t(rgb), t(K), M, cap, seeds, keep=t(keep), flip=True)
    masked = []
    for v in range(3):
        rows, valid = F.backproject_np(depth[v], rgb[v], K[v], keep[v], 1.0, True)
        assert np.array_equal(got["rows"][v * HW:(v + 1) * HW].cpu().numpy(), rows, equal_nan=True)
        masked.append(F.masked_rows(rows, F.select_np(valid, seeds[v], cap)))
    assert int(got["valid_counts"][1]) == 0 and 0 < int(got["valid_counts"][2]) <= M - 5
    want = hip_ops.cloud_prepare(t(np.concatenate(masked)), [v * HW for v in range(4)], M)
    assert want["status"].tolist() == [F.OK, F.EMPTY, F.OK]
    for f in ("status", "counts", "scale"):
        assert torch.equal(got[f], want[f]), f
    assert torch.equal(got["sample_rows"], want["sample_rows"])
    assert torch.equal(got["out"].view(torch.int32), want["out"].view(torch.int32))
    assert torch.equal(got["counts_dev"], want["counts_dev"]) and torch.equal(got["status_dev"], want["status_dev"])
    # ... and through the Python front: PreparedClouds field by field, the nearest sample of every pixel
    from gapartnet_amd import inference
    pre = cap // M
    a = inference.prepare_frames(t(depth), t(rgb), torch.from_numpy(K), num_points=M, presample=pre, seed=seeds, keep=t(keep), flip=True)
    b = inference.prepare_clouds([t(x) for x in masked], num_points=M)
    for f in ("points", "sample_rows"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    for f in ("counts", "status", "scale"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert list(a.offsets) == list(b.offsets)
    nn = inference.nearest_samples(a)
    finite = torch.isfinite(a.source[:, :3]).all(1)
    ok = torch.repeat_interleave(a.status == F.OK, HW).to(cuda)
    assert torch.equal(nn >= 0, finite & ok)


def test_argument_errors(cuda):
    from gapartnet_amd import _C, hip_ops
    depth, rgb, K = F.synthetic_frames(1, 4, 4)
    t = lambda x: torch.from_numpy(x).to(cuda)  # noqa: E731
    with pytest.raises(_C.GpnError):
        hip_ops.frame_backproject(t(depth).int(), t(rgb), t(K))
    with pytest.raises(_C.GpnError):
        hip_ops.frame_backproject(t(depth), t(rgb), t(K), depth_scale=0.0)
    rows, valid, vc = hip_ops.frame_backproject(t(depth), t(rgb), t(K))
    with pytest.raises(_C.GpnError):
        hip_ops.frame_select(rows, valid, vc, [0], 8, hash_bits=33)
