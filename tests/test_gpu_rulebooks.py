"""GPU: the rulebook builders (csrc/rulebook.hip) against the CPU oracle, bit-exactly, at the seams of their kernels.

1. the host-counted builders on every case of tests/rulebook_cases.py - pair lists, tile offsets, the neighbour table the fused
   conv kernels read and its sentinel, the coarse rows, fine_to_coarse, tap, the level counts;
2. the sort form of gpn_rulebook_down (taken when the occupancy bitmap does not fit the workspace handed in) against the oracle
   and against the bitmap form;
3. the device-counted builders (hip_ops.DevCount: buffers for a bound, live count on the device, `plan` only sizes grids) in the
   live layout, for every plan, with second rounds of the grid-stride loops and with stale bits in the bitmap workspace.

There are no tolerances: every quantity is an integer.  Nothing in any input is out of range except the batch entries
>= batch_size of the cases that say so, which the builders must drop."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import rulebook_cases as C
from tests import rulebook_ref as R

pytestmark = pytest.mark.gpu

WRAPPER_WS = 64 << 20  # what hip_ops._ws hands out at least


@pytest.fixture(scope="module")
def H():
    from gapartnet_amd import hip_ops
    return hip_ops


def host(t):
    return t.detach().cpu().numpy()


def dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)  # (a copy: the cases' arrays are read-only)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from gapartnet_amd import _C
    return _C.lib()


def _built(rb, live):
    """a hip_ops.Rulebook read in the layout of `live` destination rows"""
    return R.built_rulebook(host(rb.pair_src), host(rb.pair_dst), host(rb.tile_off), host(rb.nbr), int(rb.num_pairs.item()), rb.K, live)


def _align(n):
    return (n + 255) // 256 * 256


def _form(shape, batch_size, ws_bytes):
    """which form gpn_rulebook_down takes: the bitmap form iff bitmap, word prefixes and block sums fit the workspace"""
    words, blocks = C.bitmap_words(shape, batch_size), C.bitmap_blocks(shape, batch_size)
    return "bitmap" if _align(8 * words) + _align(4 * words) + _align(4 * blocks) <= ws_bytes and words <= (1 << 28) else "sort"


def _down_raw(H, cuda, idx, shape, batch_size, ws_bytes):
    """gpn_rulebook_down itself, with a workspace of exactly ws_bytes; outputs pre-filled so that an unwritten entry shows"""
    L, N = _lib(), idx.shape[0]
    out_idx = torch.full((N, 4), -7, dtype=torch.int32, device=cuda)
    f2c = torch.full((N,), -7, dtype=torch.int32, device=cuda)
    tap = torch.full((N,), -7, dtype=torch.int32, device=cuda)
    nout = torch.full((1,), -7, dtype=torch.int64, device=cuda)
    ws = torch.empty((int(ws_bytes),), dtype=torch.uint8, device=cuda)
    rc = L.gpn_rulebook_down(H.ptr(idx), H.i64(N), H.i64(batch_size), H.host_i32x3(shape), H.ptr(out_idx), H.ptr(f2c), H.ptr(tap),
                             H.ptr(nout), H.ptr(ws), H.szt(ws.numel()), _stream())
    assert rc == 0, L.gpn_last_error()
    No = int(nout.item())
    return dict(out_indices=host(out_idx)[:max(No, 0)], rest=host(out_idx)[max(No, 0):], fine_to_coarse=host(f2c), tap=host(tap), num_out=No)


@functools.lru_cache(maxsize=None)
def _subm_ref(name):
    idx, shape, _ = C.SUBM_CASES[name]()
    return R.subm3(idx, shape)


@functools.lru_cache(maxsize=None)
def _down_ref(name):
    return R.down(*C.DOWN_CASES[name]())


# ------------------------------------------------------------------------------------------------ 1. host-counted
@pytest.mark.parametrize("name", list(C.SUBM_CASES))
def test_subm3_cases_equal_the_oracle(H, cuda, name):
    idx, shape, _ = C.SUBM_CASES[name]()
    n = idx.shape[0]
    rb = H.rulebook_subm3(dev(idx, cuda), shape)
    assert (rb.K, rb.n_src, rb.n_dst) == (27, n, n) and tuple(rb.tile_off.shape) == (27, R.n_tiles(n) + 1)
    R.assert_rulebook_equal(_built(rb, n), _subm_ref(name))


@pytest.mark.parametrize("name", list(C.DOWN_CASES))
def test_down_cases_equal_the_oracle(H, cuda, name):
    idx, shape, batch = C.DOWN_CASES[name]()
    n, want, t = idx.shape[0], _down_ref(name), dev(idx, cuda)
    assert _form(shape, batch, WRAPPER_WS) == "bitmap"
    out_idx, out_shape, rb_f, rb_b = H.rulebook_down(t, shape, batch)
    raw = _down_raw(H, cuda, t, shape, batch, WRAPPER_WS)  # (the wrapper keeps fine_to_coarse and tap to itself)
    assert raw["num_out"] == out_idx.shape[0] and np.array_equal(raw["out_indices"], host(out_idx))
    assert (rb_f.K, rb_f.n_src, rb_f.n_dst, rb_b.K, rb_b.n_src, rb_b.n_dst) == (8, n, want["num_out"], 8, want["num_out"], n)
    got = dict(out_indices=host(out_idx), out_shape=out_shape, num_out=out_idx.shape[0], fine_to_coarse=raw["fine_to_coarse"],
               tap=raw["tap"], fwd=_built(rb_f, want["num_out"]), bwd=_built(rb_b, n))
    R.assert_rulebook_equal(got, want)
    assert H.rulebook_level_counts(t, shape, batch, 3).tolist() == R.level_counts(idx, shape, batch, 3)


# ------------------------------------------------------------------------------------------------ 2. the sort form
@pytest.mark.parametrize("variant", ["random", "odd", "dropped", "all_dropped"])
@pytest.mark.parametrize("n", [1, 257, 3000])
def test_sort_form_equals_bitmap_form_equals_oracle(H, cuda, variant, n):
    """gpn_rulebook_down with a workspace of exactly gpn_rulebook_down_ws_bytes(N) bytes on a grid whose bitmap alone is larger:
    down_keys / radix sort / down_flags / inclusive scan / down_emit answer.  The same call with the wrapper's 64 MB answers from
    the bitmap.  Both must equal the oracle."""
    idx, shape, batch = C.sort_form_input(variant, n)
    t, want = dev(idx, cuda), R.down(idx, shape, batch)
    ws_bytes = int(_lib().gpn_rulebook_down_ws_bytes(H.i64(n)))
    assert 8 * C.bitmap_words(shape, batch) > ws_bytes and _form(shape, batch, ws_bytes) == "sort", "the bitmap must not fit"
    assert _form(shape, batch, WRAPPER_WS) == "bitmap"
    by_sort = _down_raw(H, cuda, t, shape, batch, ws_bytes)
    by_bitmap = _down_raw(H, cuda, t, shape, batch, WRAPPER_WS)
    out_idx = H.rulebook_down(t, shape, batch)[0]
    for got in (by_sort, by_bitmap):
        assert got["num_out"] == want["num_out"]
        assert np.array_equal(got["out_indices"], want["out_indices"])
        assert np.array_equal(got["fine_to_coarse"], want["fine_to_coarse"]) and np.array_equal(got["tap"], want["tap"])
        assert (got["rest"] == -7).all(), "nothing written behind the coarse rows"
    assert np.array_equal(host(out_idx), want["out_indices"])
    if variant == "all_dropped":
        assert want["num_out"] == 0 and (by_sort["fine_to_coarse"] == -1).all()


# ------------------------------------------------------------------------------------------------ 3. device-counted
BOUND = 300
LIVES = [0, 1, 31, 32, 33, 257, BOUND - 1, BOUND]
DEV_SHAPE, DEV_BATCH = [8, 6, 10], 2  # 960 cells, 300 of them occupied: the rows past the live count touch live voxels


def _count(H, cuda, live, plan):
    return H.DevCount(torch.tensor([live], dtype=torch.int64, device=cuda), plan)


def _plans(live, bound):
    return sorted({0, 1, live, bound})


@functools.lru_cache(maxsize=None)
def _dev_input():
    rng = np.random.default_rng(300)
    lin = rng.choice(960, size=BOUND, replace=False)
    idx = np.stack([lin // 480, lin // 60 % 8, lin // 10 % 6, lin % 10], 1).astype(np.int32)
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def _dev_ref(kind, live):
    idx = _dev_input()[:live]
    return R.subm3(idx, DEV_SHAPE) if kind == "subm" else R.down(idx, DEV_SHAPE, DEV_BATCH)


def _check_down_dev(H, res, want, live):
    out_idx, out_shape, rb_f, rb_b, out_rows = res
    num_out = int(out_rows.t.item())
    assert num_out == want["num_out"]
    got = dict(out_indices=host(out_idx)[:num_out], out_shape=out_shape, num_out=num_out, fwd=_built(rb_f, num_out), bwd=_built(rb_b, live))
    R.assert_rulebook_equal(got, want)


@pytest.mark.parametrize("live", LIVES)
def test_device_counted_subm3(H, cuda, live):
    t, want = dev(_dev_input(), cuda), _dev_ref("subm", live)
    for plan in _plans(live, BOUND):
        rb = H.rulebook_subm3(t, DEV_SHAPE, rows=_count(H, cuda, live, plan))
        assert (rb.n_dst, rb.nbr.numel(), tuple(rb.tile_off.shape)) == (BOUND, 27 * BOUND + 1, (27, R.n_tiles(BOUND) + 1)), "bound-sized"
        try:
            R.assert_rulebook_equal(_built(rb, live), want)
        except AssertionError as e:
            raise AssertionError(f"plan {plan}: {e}") from None


@pytest.mark.parametrize("live", LIVES)
def test_device_counted_down(H, cuda, live):
    t, want = dev(_dev_input(), cuda), _dev_ref("down", live)
    for plan in _plans(live, BOUND):
        res = H.rulebook_down_dev(t, DEV_SHAPE, DEV_BATCH, _count(H, cuda, live, plan), None, out_plan=plan)
        try:
            _check_down_dev(H, res, want, live)
        except AssertionError as e:
            raise AssertionError(f"plan {plan}: {e}") from None


@pytest.mark.parametrize("live", LIVES)
def test_device_counted_identity(H, cuda, live):
    rows = np.arange(live, dtype=np.int32)
    toff = np.minimum(np.arange(R.n_tiles(live) + 1) * 32, live).astype(np.int32)[None]
    want = R.rulebook(rows, rows, toff, 1, live)
    for plan in _plans(live, BOUND):
        rb = H.rulebook_identity(BOUND, cuda, rows_dev=_count(H, cuda, live, plan))
        assert (rb.K, rb.n_src, rb.n_dst) == (1, BOUND, BOUND)
        R.assert_rulebook_equal(_built(rb, live), want)


@pytest.mark.parametrize("live", LIVES)
def test_device_counted_level_counts(H, cuda, live):
    """gpn_rulebook_level_counts with n_dev: the rows past the live count are not counted"""
    L, t = _lib(), dev(_dev_input(), cuda)
    counts = torch.full((3,), -7, dtype=torch.int64, device=cuda)
    ws = torch.empty((int(L.gpn_rulebook_level_counts_ws_bytes(H.i64(BOUND), H.i32(3))),), dtype=torch.uint8, device=cuda)
    n_dev = torch.tensor([live], dtype=torch.int64, device=cuda)
    rc = L.gpn_rulebook_level_counts(H.ptr(t), H.i64(BOUND), H.ptr(n_dev), H.i64(DEV_BATCH), H.host_i32x3(DEV_SHAPE), H.i32(3),
                                     H.ptr(counts), H.ptr(ws), H.szt(ws.numel()), _stream())
    assert rc == 0, L.gpn_last_error()
    assert counts.tolist() == R.level_counts(_dev_input()[:live], DEV_SHAPE, DEV_BATCH, 3)


def test_live_zero_equals_the_host_counted_empty_rulebook(H, cuda):
    """a device counter of 0 gives what N = 0 gives: every tap's end marker 0, no pairs, the sentinel in nbr[0]"""
    t = dev(_dev_input(), cuda)
    empty = H.rulebook_subm3(t[:0], DEV_SHAPE)
    assert tuple(empty.tile_off.shape) == (27, 1) and not empty.tile_off.any() and int(empty.num_pairs.item()) == 0
    assert int(empty.nbr[0]) == -1
    for plan in (0, 1, BOUND):
        rb = H.rulebook_subm3(t, DEV_SHAPE, rows=_count(H, cuda, 0, plan))
        nbr, sentinel, toff = R.live_layout(host(rb.nbr), host(rb.tile_off), 27, 0)
        assert np.array_equal(toff, host(empty.tile_off)) and int(rb.num_pairs.item()) == 0 and sentinel == -1 and nbr.size == 0
        out_idx, out_shape, rb_f, rb_b, out_rows = H.rulebook_down_dev(t, DEV_SHAPE, DEV_BATCH, _count(H, cuda, 0, plan), None)
        assert int(out_rows.t.item()) == 0
        for r in (rb_f, rb_b):
            nbr, sentinel, toff = R.live_layout(host(r.nbr), host(r.tile_off), 8, 0)
            assert toff.shape == (8, 1) and not toff.any() and int(r.num_pairs.item()) == 0 and sentinel == -1


@pytest.mark.parametrize("which", ["surface", "large"])
def test_device_counted_builders_take_second_rounds(H, cuda, which):
    """plan = 1: the grids are the 1024-workgroup floor.  12 000 live rows of 16 000 outrun it in the SubM lookup (27 entries per
    row) and in the list kernels; 280 000 of 300 000 in the hash insert and in the mark and rank loops of the stride-2 level"""
    (idx, shape, batch), live = (C.subm_surface(16000), 12000) if which == "surface" else (C.SUBM_CASES["large_300000"](), 280000)
    bound = idx.shape[0]
    assert live < bound and (27 * live > 1024 * 256 and C.workgroup_sums(27, live) > 1024 if which == "surface" else live > 1024 * 256)
    t = dev(idx, cuda)
    rb = H.rulebook_subm3(t, shape, rows=_count(H, cuda, live, 1))
    R.assert_rulebook_equal(_built(rb, live), R.subm3(idx[:live], shape))
    res = H.rulebook_down_dev(t, shape, batch, _count(H, cuda, live, 1), None, out_plan=1)
    _check_down_dev(H, res, R.down(idx[:live], shape, batch), live)


def test_device_counted_batch_ignores_stale_bitmap_words(H, cuda):
    """batch entries on the device, bound 16 x fine [256, 256, 256] (512 scan blocks): 12 live entries with batch_plan = 1 - 384
    scan blocks on the 256-workgroup floor, and a second round of the bitmap clear - then, on the same stream and in the same
    workspace, 3 live entries: the words of entries 3 .. 11 still hold the first call's bits and must not count"""
    shape, bound_batch, bound, live = [256, 256, 256], 16, 8000, 6000
    words_per_entry = 128 ** 3 // 64
    assert (12 * words_per_entry) // C.SCAN_BLOCK_WORDS == 384 > 256 and 12 * words_per_entry > 1024 * 256

    def rows(seed, entries):
        rng = np.random.default_rng(seed)
        lin = rng.choice(entries * 256 ** 3, size=bound, replace=False)
        return np.stack([lin // 256 ** 3, lin // 65536 % 256, lin // 256 % 256, lin % 256], 1).astype(np.int32)
    first, second = rows(1, 12), rows(2, 3)
    res = H.rulebook_down_dev(dev(first, cuda), shape, bound_batch, _count(H, cuda, live, 1), _count(H, cuda, 12, 1))
    ws_before = H._ws(256, cuda).data_ptr()
    want = R.down(first[:live], shape, bound_batch)
    assert (want["out_indices"][:, 0] >= 3).sum() > 3000, "the first call leaves bits behind entry 2"
    _check_down_dev(H, res, want, live)
    res = H.rulebook_down_dev(dev(second, cuda), shape, bound_batch, _count(H, cuda, live, 1), _count(H, cuda, 3, 1))
    assert H._ws(256, cuda).data_ptr() == ws_before, "the same workspace: the stale words are really there"
    _check_down_dev(H, res, R.down(second[:live], shape, bound_batch), live)
