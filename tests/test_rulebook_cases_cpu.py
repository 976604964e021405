"""CPU: the inputs and the reference of tests/test_gpu_rulebooks.py.  Every case of tests/rulebook_cases.py has the property
it is named for (recomputed here), the reference of tests/rulebook_ref.py equals a brute-force dictionary lookup, and
assert_rulebook_equal rejects every single-entry mutation of a correct rulebook."""
import copy

import numpy as np
import pytest

from tests import rulebook_cases as C
from tests import rulebook_ref as R


def _sums(K, n):
    return -(-(K * -(-n // 32)) // 8)


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", list(C.SUBM_CASES) + ["down:" + k for k in C.DOWN_CASES])
def test_rows_are_unique_and_in_range(name):
    idx, shape, batch = (C.DOWN_CASES[name[5:]] if name.startswith("down:") else C.SUBM_CASES[name])()
    assert idx.dtype == np.int32 and idx.ndim == 2 and idx.shape[1] == 4 and idx.shape[0] >= 1
    assert np.unique(idx, axis=0).shape[0] == idx.shape[0]
    assert (idx >= 0).all() and (idx[:, 1:] < np.asarray(shape)).all()
    if name not in ("down:batch_dropped", "down:all_dropped"):
        assert (idx[:, 0] < batch).all()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257])
def test_subm_row_counts_sit_on_the_tile_and_workgroup_seams(n):
    idx, shape, batch = C.SUBM_CASES[f"rows_{n}"]()
    assert idx.shape[0] == n
    tiles = -(-n // 32)
    assert tiles == {1: 1, 31: 1, 32: 1, 33: 2, 255: 8, 256: 8, 257: 9}[n]
    # a workgroup's eight tiles straddle two taps unless the tile count is a multiple of 8
    assert (27 * tiles % 8 != 0) == (n not in (255, 256))
    assert C.workgroup_sums(27, n) == _sums(27, n)


def test_subm_scan_cases_cross_from_one_sum_per_thread_to_two():
    a, b = C.SUBM_CASES["scan_9696"]()[0].shape[0], C.SUBM_CASES["scan_9697"]()[0].shape[0]
    assert (a, b) == (9696, 9697)
    assert (_sums(27, a), _sums(27, b)) == (1023, 1026) and _sums(27, a) <= C.SCAN_THREADS < _sums(27, b)


def test_full_grid_has_all_27_taps_on_interior_rows():
    idx, shape, batch = C.SUBM_CASES["full_grid"]()
    assert idx.shape[0] == 2 * 6 * 5 * 7 and not np.array_equal(idx, np.unique(idx, axis=0)), "full and shuffled"
    nbr = R.subm3(idx, shape)["nbr"]
    interior = ((idx[:, 1:] >= 1) & (idx[:, 1:] <= np.asarray(shape) - 2)).all(1)
    assert interior.sum() == 2 * 4 * 3 * 5
    assert ((nbr >= 0).sum(0)[interior] == 27).all() and ((nbr >= 0).sum(0)[~interior] < 27).all()
    assert (idx[nbr[:, interior].reshape(-1), 0] == np.tile(idx[interior, 0], 27)).all(), "no neighbour in the other entry"


@pytest.mark.parametrize("name,taps", [("line_1_1_40", [12, 13, 14]), ("line_1_9_1", [10, 13, 16]), ("line_7_1_1", [4, 13, 22])])
def test_extent_one_grids_have_three_taps(name, taps):
    idx, shape, batch = C.SUBM_CASES[name]()
    assert sorted(shape)[:2] == [1, 1] and idx.shape[0] == batch * max(shape)
    nbr = R.subm3(idx, shape)["nbr"]
    assert np.flatnonzero((nbr >= 0).any(1)).tolist() == taps


def test_isolated_voxels_have_only_the_centre_tap():
    idx, shape, batch = C.SUBM_CASES["isolated"]()
    rb = R.subm3(idx, shape)
    assert (idx[:, 1:] % 2 == 0).all() and rb["num_pairs"] == idx.shape[0]
    assert np.flatnonzero((rb["nbr"] >= 0).any(1)).tolist() == [13]


def test_large_subm_cases_take_second_rounds_when_device_counted():
    """the device-counted grids are max(1.5 plan, 1024) workgroups of 256 threads (csrc/gpn_common.h, dev_grid): with plan = 1,
    12 000 live rows outrun the lookup and list grids, 280 000 the per-row grids"""
    n, shape, batch = C.SUBM_CASES["surface_12000"]()[0].shape[0], *C.SUBM_CASES["surface_12000"]()[1:]
    assert n == 12000 and batch == 3
    assert 27 * n > 1024 * 256 and _sums(27, n) > 1024
    big = C.SUBM_CASES["large_300000"]()
    assert big[0].shape[0] == 300000 and big[1] == [128, 128, 128] and big[2] == 4
    assert 280000 > 1024 * 256


def test_odd_extents_have_rows_in_the_dropped_planes():
    idx, shape, batch = C.DOWN_CASES["odd_extents"]()
    assert shape == [5, 7, 9]
    dropped = (idx[:, 1] == 4) | (idx[:, 2] == 6) | (idx[:, 3] == 8)
    d = R.down(idx, shape, batch)
    assert 0 < dropped.sum() < idx.shape[0] and np.array_equal(d["fine_to_coarse"] < 0, dropped)
    assert d["num_out"] == 2 * 2 * 3 * 4
    keys = C.coarse_keys(d["out_indices"] * np.array([1, 2, 2, 2]), shape)
    assert (np.diff(keys) > 0).all(), "coarse rows ascend in (b, x, y, z)"


def _bitmap(idx, shape, batch):
    keys = np.unique(C.coarse_keys(idx, shape))
    words = np.zeros(C.bitmap_words(shape, batch), np.int64)
    np.add.at(words, keys >> 6, 1)
    return keys, words


def test_dense_down_cases_fill_every_bitmap_word():
    idx, shape, batch = C.DOWN_CASES["one_child_per_cell"]()
    keys, words = _bitmap(idx, shape, batch)
    assert idx.shape[0] == keys.shape[0] == 16384 and words.shape[0] == 256 and (words == 64).all()
    idx8, shape8, batch8 = C.DOWN_CASES["eight_children_in_a_quarter"]()
    keys8, words8 = _bitmap(idx8, shape8, batch8)
    assert shape8 == shape and (words8 == 64).all()
    per_cell = np.bincount(np.searchsorted(keys8, C.coarse_keys(idx8, shape8)), minlength=16384)
    assert (per_cell == 8).sum() == 4096 and (per_cell == 1).sum() == 12288


def test_seam_keys_are_the_chosen_coarse_cells():
    idx, shape, batch = C.DOWN_CASES["seam_keys"]()
    keys, _ = _bitmap(idx, shape, batch)
    assert keys.tolist() == [0, 63, 64, 255, 256, 16383, 16384, 65535, 65536, 131071]
    assert C.bitmap_words(shape, batch) * 64 == 131072 and keys[-1] == 131071, "the last cell of the grid"
    word = keys >> 6
    assert word[1] != word[2], "63 | 64: two words"
    assert word[3] // 4 != word[4] // 4, "255 | 256: two thread quads"
    assert word[5] // 256 != word[6] // 256 and word[5] // 1024 == word[6] // 1024, "16383 | 16384: two waves of one block"
    assert word[7] // 1024 != word[8] // 1024, "65535 | 65536: two scan blocks"
    assert idx.shape[0] == 8 * 2 + 8


@pytest.mark.parametrize("n,sums", [(32768, 1024), (32769, 1025)])
def test_down_row_counts_sit_on_the_scan_seam(n, sums):
    idx, shape, batch = C.DOWN_CASES[f"rows_{n}"]()
    keys, _ = _bitmap(idx, shape, batch)
    assert idx.shape[0] == n and keys.shape[0] == n, "fine rows and coarse rows"
    assert _sums(8, n) == sums and C.workgroup_sums(8, n) == sums


def test_many_blocks_case_outruns_the_totals_workgroup():
    idx, shape, batch = C.DOWN_CASES["many_blocks"]()
    keys, words = _bitmap(idx, shape, batch)
    n_words, n_blocks = C.bitmap_words(shape, batch), C.bitmap_blocks(shape, batch)
    assert (batch, n_words, n_blocks) == (9, 1125000, 1099) and n_blocks > 1024
    ws = 8 * n_words + 4 * n_words + 4 * n_blocks
    assert 13.4e6 < ws < 13.6e6 and ws < (64 << 20), "still the bitmap form in the wrapper's 64 MB workspace"
    blocks = np.unique(keys >> 16)
    assert set(C.BLOCKS_HIT) <= set(blocks.tolist()) and blocks.max() == n_blocks - 1
    assert 2000 < idx.shape[0] < 20000 and {0, 8} <= set(np.unique(idx[:, 0]).tolist())


def test_batch_dropping_cases_drop_what_they_say():
    idx, shape, batch = C.DOWN_CASES["batch_dropped"]()
    share = (idx[:, 0] >= batch).mean()
    assert 0.4 < share < 0.6 and R.down(idx, shape, batch)["num_out"] > 0
    idx, shape, batch = C.DOWN_CASES["all_dropped"]()
    d = R.down(idx, shape, batch)
    assert (idx[:, 0] >= batch).all() and d["num_out"] == 0 and (d["fine_to_coarse"] == -1).all()
    assert d["fwd"]["num_pairs"] == 0 and (d["bwd"]["nbr"] == -1).all() and (d["bwd"]["tile_off"] == 0).all()


@pytest.mark.parametrize("variant", ["random", "odd", "dropped", "all_dropped"])
@pytest.mark.parametrize("n", [1, 257, 3000])
def test_sort_form_inputs(variant, n):
    idx, shape, batch = C.sort_form_input(variant, n)
    assert idx.shape == (n, 4) and np.unique(idx, axis=0).shape[0] == n and (idx[:, 1:] < np.asarray(shape)).all() and (idx >= 0).all()
    assert 8 * C.bitmap_words(shape, batch) > 7.9e6, "8 MB of bitmap: far more than the workspace of 3000 rows"
    kept = R.kept_rows(idx, batch)
    if variant == "all_dropped":
        assert not kept.any()
    elif variant == "dropped" and n > 1:
        assert 0.2 < 1 - kept.mean() < 0.45
    else:
        assert variant == "dropped" or kept.all()
    if variant == "odd":
        assert (idx[:, 1] == 510).sum() >= (n + 3) // 4


# ------------------------------------------------------------------------------------------------ the reference
SMALL_SUBM = ["rows_1", "rows_33", "full_grid", "line_1_1_40", "line_1_9_1", "line_7_1_1"]
SMALL_DOWN = ["odd_extents", "batch_dropped", "all_dropped", "seam_keys"]


@pytest.mark.parametrize("name", SMALL_SUBM)
def test_subm_reference_equals_the_dictionary_lookup(name):
    idx, shape, batch = C.SUBM_CASES[name]()
    R.assert_rulebook_equal(R.subm3(idx, shape), R.brute_subm3(idx, shape))


@pytest.mark.parametrize("name", SMALL_DOWN)
def test_down_reference_equals_the_dictionary_lookup(name):
    idx, shape, batch = C.DOWN_CASES[name]()
    R.assert_rulebook_equal(R.down(idx, shape, batch), R.brute_down(idx, shape, batch))


def test_down_reference_on_the_full_grid_and_its_level_counts():
    idx, shape, batch = C.SUBM_CASES["full_grid"]()
    want = R.brute_down(idx, shape, batch)
    R.assert_rulebook_equal(R.down(idx, shape, batch), want)
    assert R.level_counts(idx, shape, batch, 3) == [want["num_out"], 2 * 1 * 1 * 1, 0]
    idx, shape, batch = C.DOWN_CASES["batch_dropped"]()
    lvl1 = R.brute_down(idx, shape, batch)
    lvl2 = R.brute_down(lvl1["out_indices"], lvl1["out_shape"], batch)
    assert R.level_counts(idx, shape, batch, 2) == [lvl1["num_out"], lvl2["num_out"]]


def test_live_layout_reads_the_front_of_bound_sized_buffers():
    idx, shape, batch = C.SUBM_CASES["rows_257"]()
    live, bound = 33, 257
    want = R.subm3(idx[:live], shape)
    nbr = np.full((27 * bound + 1,), 12345, np.int32)
    nbr[:27 * live] = want["nbr"].reshape(-1)
    nbr[27 * live] = -1
    toff = np.full((27, -(-bound // 32) + 1), 777, np.int32)
    toff.reshape(-1)[:27 * 3] = want["tile_off"].reshape(-1)
    src = np.concatenate([want["pair_src"], np.full(50, 99, np.int32)])
    dst = np.concatenate([want["pair_dst"], np.full(50, 99, np.int32)])
    R.assert_rulebook_equal(R.built_rulebook(src, dst, toff, nbr, want["num_pairs"], 27, live), want)
    with pytest.raises(AssertionError):  # the layout of the bound is another table
        R.assert_rulebook_equal(R.built_rulebook(src, dst, toff, nbr, want["num_pairs"], 27, bound), want)


# ------------------------------------------------------------------------------------------------ the comparison is sharp
def _subm_ok():
    idx, shape, batch = C.SUBM_CASES["rows_257"]()
    return R.subm3(idx, shape)


def _down_ok():
    idx, shape, batch = C.DOWN_CASES["odd_extents"]()
    return R.down(idx, shape, batch)


def _swap_two_pairs(rb):
    toff = rb["tile_off"]
    k, t = next((k, t) for k in range(27) for t in range(toff.shape[1] - 1) if toff[k, t + 1] - toff[k, t] >= 2)
    p = int(toff[k, t])
    for f in ("pair_src", "pair_dst"):
        rb[f] = rb[f].copy()
        rb[f][[p, p + 1]] = rb[f][[p + 1, p]]


def _tile_off_by_one(rb):
    rb["tile_off"] = rb["tile_off"].copy()
    rb["tile_off"][5, 3] += 1


def _nbr_to_next_tap(rb):
    nbr = rb["nbr"] = rb["nbr"].copy()
    k, o = next((k, o) for k in range(26) for o in range(nbr.shape[1]) if nbr[k, o] >= 0 and nbr[k + 1, o] < 0)
    nbr[k + 1, o], nbr[k, o] = nbr[k, o], -1


def _sentinel_zero(rb):
    rb["sentinel"] = 0


def _f2c_off_by_one(d):
    d["fine_to_coarse"] = d["fine_to_coarse"].copy()
    d["fine_to_coarse"][int(np.flatnonzero(d["fine_to_coarse"] >= 0)[7])] += 1


def _swap_coarse_rows(d):
    d["out_indices"] = d["out_indices"].copy()
    d["out_indices"][[3, 4]] = d["out_indices"][[4, 3]]


def _num_out_too_large(d):
    d["num_out"] += 1


@pytest.mark.parametrize("mutate,make", [(_swap_two_pairs, _subm_ok), (_tile_off_by_one, _subm_ok), (_nbr_to_next_tap, _subm_ok),
                                         (_sentinel_zero, _subm_ok), (_f2c_off_by_one, _down_ok), (_swap_coarse_rows, _down_ok),
                                         (_num_out_too_large, _down_ok)], ids=lambda f: f.__name__.strip("_"))
def test_every_single_mutation_is_rejected(mutate, make):
    want = make()
    got = copy.deepcopy(want)
    R.assert_rulebook_equal(got, want)
    mutate(got)
    with pytest.raises(AssertionError):
        R.assert_rulebook_equal(got, want)
    if "fwd" in want:  # ... and the same mutations inside a down level's two rulebooks
        for side in ("fwd", "bwd"):
            for m in (_tile_off_by_one_small, _sentinel_zero):
                got = copy.deepcopy(want)
                m(got[side])
                with pytest.raises(AssertionError):
                    R.assert_rulebook_equal(got, want)


def _tile_off_by_one_small(rb):
    rb["tile_off"] = rb["tile_off"].copy()
    rb["tile_off"][2, 0] += 1
