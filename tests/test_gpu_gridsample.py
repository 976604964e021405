"""csrc/gridsample.hip (include/gpn.h section GS) on the GPU against the independent restatement (tests/grid_ref.py): idx and level
exactly, with sentinel bytes behind every output and in every slot the contract leaves unwritten."""
import ctypes

import numpy as np
import pytest
import torch

from tests import grid_ref as G
from tests import inference_ref as R

pytestmark = pytest.mark.gpu
PAD, SENT = 256, 0xA5
SENT32 = int(np.frombuffer(bytes([SENT] * 4), np.int32)[0])
OK, FEW, EMPTY = 0, 1, 2


class Guarded:
    """a device buffer of ``shape`` filled with sentinel bytes, with PAD more of them behind it"""

    def __init__(self, shape, dtype, cuda):
        self.n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.n + PAD,), SENT, dtype=torch.uint8, device=cuda)
        self.t = self.raw[:self.n].view(dtype).view(shape)

    def check(self, what):
        assert bool((self.raw[self.n:] == SENT).all()), f"{what}: written past its end"


def pack(clouds, statuses=None, n_bound=None):
    """clouds [n_s, 3] f32 -> (packed [S, nb, 4] with .w = 1e10 and NaN rows past the count, counts, status)"""
    nb = n_bound or max(max(len(c) for c in clouds), 1)
    packed = np.full((len(clouds), nb, 4), np.nan, np.float32)
    for s, c in enumerate(clouds):
        packed[s, :len(c), :3] = c
        packed[s, :len(c), 3] = 1e10
    counts = np.array([len(c) for c in clouds], np.int32)
    status = np.array(statuses if statuses is not None else [OK if len(c) else EMPTY for c in clouds], np.int32)
    return packed, counts, status


def run_kernel(cuda, packed, counts, status, seeds, m, hash_bits=32):
    """gpn_cloud_grid_sample into guarded buffers -> (idx [S, m], level [S], status [S]) on the host; packed must come back unchanged"""
    from gapartnet_amd import _C
    from gapartnet_amd.hip_ops import _stream
    L = _C.lib()
    S, nb, _ = packed.shape
    p = torch.from_numpy(packed).to(cuda)
    before = p.clone()
    c, st = torch.from_numpy(counts).to(cuda), torch.from_numpy(status.copy()).to(cuda)
    sd = torch.from_numpy(np.asarray(seeds, dtype=np.int64).astype(np.uint32).view(np.int32)).to(cuda)
    idx, level = Guarded((S, m), torch.int32, cuda), Guarded((S,), torch.int32, cuda)
    nbytes = int(L.gpn_cloud_grid_sample_ws_bytes(_C.i32(S), _C.i64(nb)))
    ws = Guarded((nbytes,), torch.uint8, cuda)
    _C.check(L.gpn_cloud_grid_sample(_C.ptr(p), _C.i64(nb), _C.ptr(c), _C.ptr(st), _C.ptr(sd), _C.i32(S), _C.i32(m), _C.i32(hash_bits),
                                     _C.ptr(idx.t), _C.ptr(level.t), _C.ptr(ws.t), _C.szt(nbytes), _stream()), "gpn_cloud_grid_sample")
    torch.cuda.synchronize()
    for g, what in ((idx, "idx"), (level, "level"), (ws, "workspace")):
        g.check(what)
    assert torch.equal(p.view(torch.int32), before.view(torch.int32)), "packed was written"
    return idx.t.cpu().numpy(), level.t.cpu().numpy(), st.cpu().numpy()


def check_against_ref(got, clouds, status_in, seeds, m, hash_bits=32):
    idx, level, status = got
    for s, c in enumerate(clouds):
        n = len(c)
        if status_in[s] != OK:
            assert status[s] == status_in[s] and level[s] == -1 and (idx[s] == SENT32).all(), s
        elif n < m:
            assert status[s] == FEW and level[s] == -1 and (idx[s] == SENT32).all(), s
        elif n == m:
            assert status[s] == OK and level[s] == -1 and np.array_equal(idx[s], np.arange(m)), s
        else:
            want, want_level = G.grid_sample(c, m, seeds[s], hash_bits)
            assert status[s] == OK and level[s] == want_level, (s, n, level[s], want_level)
            assert np.array_equal(idx[s], want), (s, n, np.nonzero(idx[s] != np.asarray(want))[0][:8])


def _ragged(rng, m):
    sizes = [0, max(m - 1, 0), m, m + 1, 2, 63, 64, 65, 1025, 300]
    clouds = [rng.randn(n, 3).astype(np.float32) for n in sizes]
    clouds.append(rng.randn(40 + m, 3).astype(np.float32))      # an OK-sized cloud whose status says DEGENERATE: skipped
    packed, counts, status = pack(clouds)
    status[-1] = 3
    return clouds, packed, counts, status


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65])
def test_ragged_batch_equals_the_restatement(cuda, m):
    rng = np.random.RandomState(100 + m)
    clouds, packed, counts, status = _ragged(rng, m)
    seeds = [(7 * s + m) & 0xffffffff for s in range(len(clouds))]
    seeds[3] = 0xffffffff
    got = run_kernel(cuda, packed, counts, status, seeds, m)
    check_against_ref(got, clouds, status, seeds, m)
    # reruns are bit-equal, and every cloud alone gives what it gives in the batch
    again = run_kernel(cuda, packed, counts, status, seeds, m)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)
    for s in (3, 7, 8, 9):
        if len(clouds[s]) <= m:
            continue
        p1, c1, s1 = pack([clouds[s]])
        alone = run_kernel(cuda, p1, c1, s1, [seeds[s]], m)
        assert np.array_equal(alone[0][0], got[0][s]) and alone[1][0] == got[1][s], s


@pytest.mark.parametrize("seed,hash_bits", [(0, 32), (0xffffffff, 4), (5, 1)])
def test_degenerate_families_and_every_level(cuda, seed, hash_bits):
    rng = np.random.RandomState(3)
    fam = G.families(rng)
    groups = {}
    for name, (xyz, m) in fam.items():
        groups.setdefault(m, []).append(xyz)
    for L in range(11):
        groups.setdefault(12 if L else 7, []).append(G.level_cloud(rng, L))
    for n in (90, 200):   # hash ties at every rank
        groups.setdefault(n // 2, []).append(rng.randn(n, 3).astype(np.float32))
    levels = set()
    for m, clouds in sorted(groups.items()):
        packed, counts, status = pack(clouds)
        seeds = [seed] * len(clouds)
        got = run_kernel(cuda, packed, counts, status, seeds, m, hash_bits)
        check_against_ref(got, clouds, status, seeds, m, hash_bits)
        levels |= set(got[1].tolist())
    assert levels >= set(range(11))


def test_a_cloud_that_spans_many_chunks(cuda):
    rng = np.random.RandomState(8)
    big = (rng.randn(70000, 3) * [1.0, 0.6, 0.2]).astype(np.float32)
    packed, counts, status = pack([big])                       # an S = 1 call
    got = run_kernel(cuda, packed, counts, status, [12345], 20000)
    check_against_ref(got, [big], status, [12345], 20000)
    assert got[1][0] >= 4


def test_argument_errors_return_before_any_launch(cuda):
    from gapartnet_amd import _C
    L = _C.lib()
    p = torch.zeros((1, 8, 4), device=cuda)
    i, z = torch.zeros(8, dtype=torch.int32, device=cuda), ctypes.c_size_t
    nbytes = int(L.gpn_cloud_grid_sample_ws_bytes(_C.i32(1), _C.i64(8)))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)

    def call(m=2, hash_bits=32, ws_bytes=nbytes):
        return L.gpn_cloud_grid_sample(_C.ptr(p), _C.i64(8), _C.ptr(i), _C.ptr(i), _C.ptr(i), _C.i32(1), _C.i32(m), _C.i32(hash_bits),
                                       _C.ptr(i), _C.ptr(i), _C.ptr(ws), z(ws_bytes), None)
    assert call(m=0) == 1 and call(hash_bits=0) == 1 and call(hash_bits=33) == 1 and call(ws_bytes=nbytes - 1) == 1
    assert b"bad argument" in L.gpn_last_error()
    torch.cuda.synchronize()
    assert not bool(i.any()), "a refused call wrote"


def test_cloud_prepare_with_the_grid_sampler_equals_the_cpu_path(cuda):
    from gapartnet_amd import hip_ops, inference
    rng = np.random.RandomState(11)
    m = 256
    clean, holes = rng.randn(1000, 6).astype(np.float32), rng.randn(1000, 6).astype(np.float32)
    holes[rng.choice(1000, 120, replace=False), rng.randint(0, 3, size=120)] = np.nan
    exact, few = rng.randn(m, 6).astype(np.float32), rng.randn(100, 6).astype(np.float32)
    same = np.tile(rng.randn(1, 6).astype(np.float32), (300, 1))
    clouds = [clean, holes, exact, few, np.zeros((0, 6), np.float32), same, rng.randn(5000, 6).astype(np.float32)]
    seeds = [3, 4, 5, 6, 7, 0xffffffff, 9]
    offsets = [0] + np.cumsum([c.shape[0] for c in clouds]).tolist()
    got = hip_ops.cloud_prepare(torch.from_numpy(np.concatenate(clouds)).to(cuda), offsets, m, sampler="grid", seeds=seeds)
    want = inference.prepare_clouds([torch.from_numpy(c) for c in clouds], m, sampler="grid", seed=seeds)
    assert got["status"].tolist() == want.status.tolist() == [R.OK, R.OK, R.OK, R.OK, R.EMPTY, R.DEGENERATE, R.OK]
    assert got["level"].tolist() == want.level.tolist()
    out, rows = got["out"].cpu().numpy(), got["sample_rows"].cpu().numpy()
    first = 0
    for s in range(len(clouds)):
        ms = int(want.counts[s])
        if want.status[s] != R.EMPTY:
            assert np.array_equal(got["scale"][s].numpy(), want.scale[s].numpy()), s
        if ms == 0:
            continue
        assert int(got["counts"][s]) == ms
        assert np.array_equal(rows[s, :ms], want.sample_rows[first:first + ms].numpy()) and (rows[s, ms:] == -1).all(), s
        assert np.array_equal(out[s, :ms].view(np.uint32), want.points[first:first + ms].numpy().view(np.uint32)), s
        assert not out[s, ms:].any(), s
        first += ms
    with pytest.raises(ValueError):
        hip_ops.cloud_prepare(torch.from_numpy(clean).to(cuda), [0, 1000], m, sampler="octree")
