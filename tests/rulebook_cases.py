"""Named inputs for the rulebook builders (csrc/rulebook.hip), each chosen for one seam of the kernels and named for it.  numpy
only.  A case is a function -> (indices [N, 4] int32 (b, x, y, z), spatial_shape, batch_size); all coordinates are unique and in
range unless the case says otherwise.  tests/test_rulebook_cases_cpu.py checks that every case has the property it is named
for; tests/test_gpu_rulebooks.py runs them.

The seams: pair lists come from a ballot per 32-row tile (TILE), eight tiles per workgroup (WG_TILES), and one 1024-thread
workgroup that scans the workgroup sums (SCAN_THREADS: more than one sum per thread beyond 1024 sums).  The stride-2 levels rank
coarse cells by an occupancy bitmap: 64-bit words, 4 words per thread, 64 threads per wave, 1024 words per scan block
(SCAN_BLOCK_WORDS), one 1024-thread workgroup over the block totals."""
import functools

import numpy as np

TILE = 32
WG_TILES = 8
SCAN_THREADS = 1024
SCAN_BLOCK_WORDS = 1024


def workgroup_sums(K, n_rows):
    """sums the list builder's scan workgroup adds up for a [K, n_rows] table"""
    tiles = (n_rows + TILE - 1) // TILE
    return (K * tiles + WG_TILES - 1) // WG_TILES


def bitmap_words(shape, batch_size):
    cells = batch_size * (shape[0] // 2) * (shape[1] // 2) * (shape[2] // 2)
    return (cells + 63) // 64


def bitmap_blocks(shape, batch_size):
    return (bitmap_words(shape, batch_size) + SCAN_BLOCK_WORDS - 1) // SCAN_BLOCK_WORDS


def coarse_keys(indices, shape):
    """linear key of every row's coarse cell (rows assumed kept)"""
    o = [s // 2 for s in shape]
    c = np.asarray(indices, np.int64)
    return ((c[:, 0] * o[0] + (c[:, 1] >> 1)) * o[1] + (c[:, 2] >> 1)) * o[2] + (c[:, 3] >> 1)


def _frozen(a):
    a = np.ascontiguousarray(a, np.int32)
    a.setflags(write=False)
    return a


def _decode(lin, batch, shape):
    lin = np.asarray(lin, np.int64).copy()
    z = lin % shape[2]; lin //= shape[2]
    y = lin % shape[1]; lin //= shape[1]
    x = lin % shape[0]; b = lin // shape[0]
    assert (b < batch).all()
    return np.stack([b, x, y, z], 1)


def _random_unique(seed, batch, shape, n):
    rng = np.random.default_rng(seed)
    total = batch * shape[0] * shape[1] * shape[2]
    assert n <= total
    return _decode(rng.choice(total, size=n, replace=False), batch, shape)


def _sheet(seed, batch, shape, n):
    """n voxels of a wavy sheet per batch entry (a depth scan's occupancy: many neighbours), as thick as n needs; shuffled"""
    rng = np.random.default_rng(seed)
    per_layer = batch * shape[0] * shape[1]
    thick = (n + per_layer - 1) // per_layer + 1
    assert thick < shape[2] // 2
    b, x, y = np.meshgrid(np.arange(batch), np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    z0 = ((0.5 + 0.25 * np.sin(4.0 * x / shape[0] + b) * np.cos(3.0 * y / shape[1])) * (shape[2] - 1 - thick)).astype(np.int64)
    rows = np.concatenate([np.stack([b, x, y, z0 + t], -1).reshape(-1, 4) for t in range(thick)], 0)
    return rows[rng.permutation(rows.shape[0])[:n]]


# ------------------------------------------------------------------------------------------------ SubM
def _subm_rows(n):
    # (2 x [9, 8, 10] = 1440 cells: 257 rows fill 18 % of them, so most taps of most tiles are non-empty)
    return lambda: (_frozen(_random_unique(100 + n, 2, [9, 8, 10], n)), [9, 8, 10], 2)


def _subm_scan(n):
    return lambda: (_frozen(_random_unique(200 + n, 2, [24, 24, 24], n)), [24, 24, 24], 2)


def subm_full_grid():
    """2 x [6, 5, 7] fully occupied, shuffled: every interior row has all 27 taps; nothing wraps across a face or an entry"""
    rows = _decode(np.arange(2 * 6 * 5 * 7), 2, [6, 5, 7])
    return _frozen(rows[np.random.default_rng(1).permutation(rows.shape[0])]), [6, 5, 7], 2


def _subm_line(shape, batch):
    def case():
        rows = _decode(np.arange(batch * shape[0] * shape[1] * shape[2]), batch, shape)
        return _frozen(rows[np.random.default_rng(sum(shape)).permutation(rows.shape[0])]), list(shape), batch
    return case


def subm_isolated():
    """300 voxels on even coordinates only: 26 taps are empty, every end marker comes from the 'end of the previous tap' rule"""
    rows = _random_unique(7, 2, [8, 8, 8], 300) * np.array([1, 2, 2, 2])
    return _frozen(rows), [16, 16, 16], 2


def subm_surface(n=12000):
    return _frozen(_sheet(11, 3, [64, 64, 64], n)), [64, 64, 64], 3


def subm_large(n=300000):
    return _frozen(_sheet(12, 4, [128, 128, 128], n)), [128, 128, 128], 4


SUBM_CASES = {f"rows_{n}": _subm_rows(n) for n in (1, 31, 32, 33, 255, 256, 257)}
SUBM_CASES.update({f"scan_{n}": _subm_scan(n) for n in (9696, 9697)})
SUBM_CASES.update(full_grid=subm_full_grid, line_1_1_40=_subm_line((1, 1, 40), 1), line_1_9_1=_subm_line((1, 9, 1), 2),
                  line_7_1_1=_subm_line((7, 1, 1), 2), isolated=subm_isolated, surface_12000=subm_surface, large_300000=subm_large)


# ------------------------------------------------------------------------------------------------ down
def _children(seed, keys, batch, shape, how):
    """fine rows for the coarse cells `keys` (linear keys of the coarse grid): how = 'one' random child, 'all' eight"""
    rng = np.random.default_rng(seed)
    o = [s // 2 for s in shape]
    c = _decode(keys, batch, o)
    if how == "one":
        bits = rng.integers(0, 2, (c.shape[0], 3))
        return np.concatenate([c[:, :1], c[:, 1:] * 2 + bits], 1)
    kids = np.stack(np.meshgrid([0, 1], [0, 1], [0, 1], indexing="ij"), -1).reshape(8, 3)
    return np.concatenate([np.concatenate([c[:, :1], c[:, 1:] * 2 + k], 1) for k in kids], 0)


def _shuffled(seed, rows):
    return rows[np.random.default_rng(seed).permutation(rows.shape[0])]


def down_odd_extents():
    """2 x [5, 7, 9] fully occupied: the planes x = 4, y = 6, z = 8 have no coarse cell"""
    rows = _decode(np.arange(2 * 5 * 7 * 9), 2, [5, 7, 9])
    return _frozen(_shuffled(2, rows)), [5, 7, 9], 2


DENSE_SHAPE = [32, 32, 64]  # coarse 16 x 16 x 32 x 2 entries = 16384 cells = 256 bitmap words


def down_one_child_per_cell():
    """every coarse cell of 2 x [32, 32, 64] has one child: every bitmap word is all ones (the largest prefixes)"""
    return _frozen(_shuffled(3, _children(3, np.arange(16384), 2, DENSE_SHAPE, "one"))), list(DENSE_SHAPE), 2


def down_eight_children_in_a_quarter():
    """the same coarse grid: all eight children in a quarter of the cells, one child in the others"""
    rng = np.random.default_rng(4)
    perm = rng.permutation(16384)
    rows = np.concatenate([_children(4, perm[:4096], 2, DENSE_SHAPE, "all"), _children(5, perm[4096:], 2, DENSE_SHAPE, "one")], 0)
    return _frozen(_shuffled(4, rows)), list(DENSE_SHAPE), 2


SEAM_SHAPE = [64, 64, 128]  # coarse 32 x 32 x 64 x 2 entries = 131072 cells
SEAM_KEYS = [0, 63, 64, 255, 256, 64 * 255 + 63, 64 * 256, 65535, 65536, 131071]


def down_seam_keys():
    """coarse cells at the bitmap's seams: word (63 | 64), thread quad (255 | 256), wave (64*255+63 | 64*256), scan block
    (65535 | 65536) and the last cell of the grid; two of them with all eight children"""
    keys = np.asarray(SEAM_KEYS)
    rows = np.concatenate([_children(6, keys[[1, 6]], 2, SEAM_SHAPE, "all"), _children(6, np.delete(keys, [1, 6]), 2, SEAM_SHAPE, "one")])
    return _frozen(_shuffled(6, rows)), list(SEAM_SHAPE), 2


def _down_rows(n):
    # one child per coarse cell of [64, 64, 80] (40960 cells): n fine rows AND n coarse rows
    def case():
        keys = np.random.default_rng(n).choice(40960, size=n, replace=False)
        return _frozen(_children(n, keys, 1, [64, 64, 80], "one")), [64, 64, 80], 1
    return case


BLOCKS_SHAPE = [400, 400, 400]  # coarse 200^3 x 9 entries = 72 M cells = 1 125 000 words = 1099 scan blocks (13.5 MB of workspace)
BLOCKS_HIT = [0, 1023, 1024, 1098]


def down_many_blocks():
    """9 x [400, 400, 400]: rows in the first and last batch entry and in the bitmap blocks 0, 1023, 1024 and 1098 of 1099 - the
    totals kernel takes more than one block per thread"""
    rng = np.random.default_rng(8)
    per_block, cells = 64 * SCAN_BLOCK_WORDS, 9 * 200 ** 3
    keys = [b * per_block + rng.choice(min(per_block, cells - b * per_block), size=700, replace=False) for b in BLOCKS_HIT]
    keys.append(rng.choice(200 ** 3, size=500, replace=False))                  # anywhere in entry 0
    keys.append(8 * 200 ** 3 + rng.choice(200 ** 3, size=500, replace=False))  # anywhere in entry 8
    keys = np.unique(np.concatenate(keys))
    rows = np.concatenate([_children(8, keys[::3], 9, BLOCKS_SHAPE, "all"), _children(9, np.delete(keys, np.s_[::3]), 9, BLOCKS_SHAPE, "one")])
    return _frozen(_shuffled(8, rows)), list(BLOCKS_SHAPE), 9


def down_batch_dropped():
    """entries 0 .. 3 present, batch_size = 2: the rows of entries 2 and 3 are dropped (fine_to_coarse == -1)"""
    return _frozen(_random_unique(10, 4, [12, 10, 14], 900)), [12, 10, 14], 2


def down_all_dropped():
    """every row sits in entry 2 or 3 with batch_size = 2: num_out == 0"""
    rows = _random_unique(11, 2, [12, 10, 14], 300) + np.array([2, 0, 0, 0])
    return _frozen(rows), [12, 10, 14], 2


DOWN_CASES = dict(odd_extents=down_odd_extents, one_child_per_cell=down_one_child_per_cell,
                  eight_children_in_a_quarter=down_eight_children_in_a_quarter, seam_keys=down_seam_keys,
                  rows_32768=_down_rows(32768), rows_32769=_down_rows(32769), many_blocks=down_many_blocks,
                  batch_dropped=down_batch_dropped, all_dropped=down_all_dropped)

# (a case is built once per process and shared read-only: the arrays are frozen)
SUBM_CASES = {k: functools.lru_cache(maxsize=None)(f) for k, f in SUBM_CASES.items()}
DOWN_CASES = {k: functools.lru_cache(maxsize=None)(f) for k, f in DOWN_CASES.items()}


# ---- inputs of the sort form of gpn_rulebook_down: grids whose bitmap alone outgrows the workspace of N rows ----------------------
def sort_form_input(variant, n):
    """(indices, shape, batch_size): fine [512, 512, 512] x 4 (8 MB of bitmap); 'odd' [511, 513, 512] with rows in the dropped
    plane; 'dropped' a third of the rows in entries >= batch_size; 'all_dropped' all of them"""
    shape = [511, 513, 512] if variant == "odd" else [512, 512, 512]
    entries = {"random": 4, "odd": 4, "dropped": 6, "all_dropped": 2}[variant]
    rows = _random_unique(1000 + n, entries, shape, n)
    if variant == "odd":
        rows[: (n + 3) // 4, 1] = 510  # the dropped plane (the seeds are fixed: the rows stay unique)
        assert np.unique(rows, axis=0).shape[0] == n
    if variant == "all_dropped":
        rows = rows + np.array([4, 0, 0, 0])
    return _frozen(rows), shape, 4
