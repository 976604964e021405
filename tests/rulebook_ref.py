"""Reference for the rulebook builders (csrc/rulebook.hip): the CPU oracle (oracle.rulebook_subm3 / rulebook_down, pinned to
torch's dense conv3d by tests/test_oracle_pins.py) plus the few things the oracle does not state - the tap-major neighbour
table the fused conv kernels read, the "live layout" of a device-counted rulebook inside buffers sized for a bound, and the
rows the GPU builders drop for their batch entry.  numpy only; every quantity is an integer and every comparison is exact.

A rulebook is a dict: K, n_dst, num_pairs, pair_src [P], pair_dst [P], tile_off [K, n_tiles + 1], nbr [K, n_dst], sentinel.
A down level is a dict: out_indices [No, 4], out_shape, fine_to_coarse [N], tap [N], num_out, fwd, bwd (rulebooks)."""
import numpy as np

import oracle as O

TILE_ROWS = 32


def n_tiles(n):
    return (int(n) + TILE_ROWS - 1) // TILE_ROWS


def nbr_table(pair_src, pair_dst, tile_off, K, n_dst):
    """the tap-major table [K, n_dst] (-1 = no neighbour) the pair lists and their offsets describe"""
    table = np.full((K, n_dst), -1, np.int32)
    for k in range(K):
        p0, p1 = int(tile_off[k, 0]), int(tile_off[k, -1])
        table[k, pair_dst[p0:p1]] = pair_src[p0:p1]
    return table


def rulebook(pair_src, pair_dst, tile_off, K, n_dst):
    """a reference rulebook from the oracle's (pair_src, pair_dst, tile_off)"""
    tile_off = np.asarray(tile_off, np.int32).reshape(K, n_tiles(n_dst) + 1)
    return dict(K=K, n_dst=int(n_dst), num_pairs=int(pair_src.shape[0]), pair_src=np.asarray(pair_src, np.int32),
                pair_dst=np.asarray(pair_dst, np.int32), tile_off=tile_off,
                nbr=nbr_table(pair_src, pair_dst, tile_off, K, n_dst), sentinel=-1)


def live_layout(nbr_flat, tile_off_flat, K, live):
    """(nbr [K, live], sentinel, tile_off [K, n_tiles(live) + 1]) of a rulebook laid out for `live` rows at the front of flat
    buffers that may be sized for a larger bound"""
    nbr_flat, tile_off_flat = np.asarray(nbr_flat).reshape(-1), np.asarray(tile_off_flat).reshape(-1)
    nt = n_tiles(live)
    return nbr_flat[:K * live].reshape(K, live), int(nbr_flat[K * live]), tile_off_flat[:K * (nt + 1)].reshape(K, nt + 1)


def built_rulebook(pair_src, pair_dst, tile_off_flat, nbr_flat, num_pairs, K, live):
    """a rulebook a builder wrote (host arrays), read in the layout of `live` destination rows"""
    nbr, sentinel, tile_off = live_layout(nbr_flat, tile_off_flat, K, live)
    P = int(num_pairs)
    return dict(K=K, n_dst=int(live), num_pairs=P, pair_src=np.asarray(pair_src).reshape(-1)[:max(P, 0)],
                pair_dst=np.asarray(pair_dst).reshape(-1)[:max(P, 0)], tile_off=tile_off, nbr=nbr, sentinel=sentinel)


def subm3(indices, shape):
    indices = np.ascontiguousarray(indices, np.int32).reshape(-1, 4)
    src, dst, toff = O.rulebook_subm3(indices, shape)
    return rulebook(src, dst, toff, 27, indices.shape[0])


def kept_rows(indices, batch_size):
    """rows the stride-2 builders keep before the extent test: batch entry inside [0, batch_size), no negative coordinate"""
    indices = np.asarray(indices).reshape(-1, 4)
    return (indices[:, 0] >= 0) & (indices[:, 0] < batch_size) & (indices[:, 1:] >= 0).all(1)


def down(indices, shape, batch_size):
    """oracle.rulebook_down with the GPU builders' batch_size rule: the oracle runs on the kept rows and its row numbers are
    mapped back; a dropped row has fine_to_coarse == -1 and still gets its tap"""
    indices = np.ascontiguousarray(indices, np.int32).reshape(-1, 4)
    N = indices.shape[0]
    keep = kept_rows(indices, batch_size)
    d = O.rulebook_down(indices[keep], shape)
    No = d["out_indices"].shape[0]
    tap = ((indices[:, 1] & 1) * 4 + (indices[:, 2] & 1) * 2 + (indices[:, 3] & 1)).astype(np.int32)
    if keep.all():
        f2c, (fs, fd, ft), (bs, bd, bt) = d["fine_to_coarse"], d["fwd"], d["bwd"]
        assert np.array_equal(tap, d["tap"])
    else:
        rows = np.flatnonzero(keep).astype(np.int32)  # kept row -> row (increasing: (tap, dst) order survives)
        assert np.array_equal(tap[keep], d["tap"])
        f2c = np.full((N,), -1, np.int32)
        f2c[keep] = d["fine_to_coarse"]
        fs, fd, ft = rows[d["fwd"][0]], d["fwd"][1], d["fwd"][2]  # (src = fine row, dst = coarse row: tiles unchanged)
        bs, bd = d["bwd"][0], rows[d["bwd"][1]]                   # (dst = fine row: the tiles are those of all N rows)
        old = d["bwd"][2]
        bt = np.zeros((8, n_tiles(N) + 1), np.int32)
        starts = np.arange(n_tiles(N) + 1, dtype=np.int64) * TILE_ROWS
        for k in range(8):
            p0, p1 = int(old[k, 0]), int(old[k, -1])
            bt[k] = p0 + np.searchsorted(bd[p0:p1], starts, side="left")
    return dict(out_indices=d["out_indices"], out_shape=list(d["out_shape"]), fine_to_coarse=np.asarray(f2c, np.int32), tap=tap,
                num_out=int(No), fwd=rulebook(fs, fd, ft, 8, No), bwd=rulebook(bs, bd, bt, 8, N))


def level_counts(indices, shape, batch_size, n_levels):
    """row counts of the next n_levels stride-2 levels: the chain of down levels"""
    counts, cur, cur_shape = [], np.asarray(indices, np.int32).reshape(-1, 4), list(shape)
    cur = cur[kept_rows(cur, batch_size)]
    for _ in range(n_levels):
        d = O.rulebook_down(cur, cur_shape)
        counts.append(int(d["out_indices"].shape[0]))
        cur, cur_shape = d["out_indices"], d["out_shape"]
    return counts


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise AssertionError(f"{name}: shape {got.shape} != {want.shape}")
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        raise AssertionError(f"{name}: {bad.size} of {got.size} entries differ, first at flat index {int(bad[0])}: "
                             f"{got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}")


def _assert_rb(got, want, name):
    for f in ("K", "n_dst", "num_pairs", "sentinel"):
        if int(got[f]) != int(want[f]):
            raise AssertionError(f"{name}{f}: {got[f]} != {want[f]}")
    P = int(want["num_pairs"])
    _same(name + "pair_src", got["pair_src"][:P], want["pair_src"][:P])
    _same(name + "pair_dst", got["pair_dst"][:P], want["pair_dst"][:P])
    _same(name + "tile_off", got["tile_off"], want["tile_off"])
    _same(name + "nbr", got["nbr"], want["nbr"])


def assert_rulebook_equal(got, want):
    """bit-exact: num_pairs, the first P pairs, tile_off, the neighbour table and its sentinel; for a down level also out_indices,
    out_shape, fine_to_coarse, tap, num_out and both directions' rulebooks"""
    if "fwd" not in want:
        return _assert_rb(got, want, "")
    if int(got["num_out"]) != int(want["num_out"]):
        raise AssertionError(f"num_out: {got['num_out']} != {want['num_out']}")
    if list(got["out_shape"]) != list(want["out_shape"]):
        raise AssertionError(f"out_shape: {got['out_shape']} != {want['out_shape']}")
    No = int(want["num_out"])
    _same("out_indices", np.asarray(got["out_indices"]).reshape(-1, 4)[:No], want["out_indices"])
    if got.get("fine_to_coarse") is None:
        # a wrapper that keeps the two arrays to itself: the table of the fine rows states them (nbr[tap[i], i] = fine_to_coarse[i],
        # the only entry of column i), so read them from there - the taps of dropped rows are then not covered
        nbr = np.asarray(got["bwd"]["nbr"])
        f2c = nbr.max(0) if nbr.shape[1] else np.zeros((0,), np.int32)
        got = dict(got, fine_to_coarse=f2c, tap=np.where(f2c >= 0, nbr.argmax(0) if nbr.shape[1] else 0, want["tap"]))
    _same("fine_to_coarse", got["fine_to_coarse"], want["fine_to_coarse"])
    _same("tap", got["tap"], want["tap"])
    _assert_rb(got["fwd"], want["fwd"], "fwd.")
    _assert_rb(got["bwd"], want["bwd"], "bwd.")


# ---- brute force: a dictionary from (b, x, y, z) to the row, a loop over taps ------------------------------------------------
def _lists(table):
    K, n = table.shape
    src, dst, toff = [], [], np.zeros((K, n_tiles(n) + 1), np.int32)
    for k in range(K):
        for o in range(n):
            if o % TILE_ROWS == 0:
                toff[k, o // TILE_ROWS] = len(src)
            if table[k, o] >= 0:
                src.append(int(table[k, o]))
                dst.append(o)
        toff[k, n_tiles(n)] = len(src)
    return dict(K=K, n_dst=n, num_pairs=len(src), pair_src=np.asarray(src, np.int32), pair_dst=np.asarray(dst, np.int32), tile_off=toff,
                nbr=table.copy(), sentinel=-1)


def brute_subm3(indices, shape):
    rows = {tuple(int(v) for v in c): i for i, c in enumerate(indices)}
    table = np.full((27, len(indices)), -1, np.int32)
    for o, (b, x, y, z) in enumerate(indices):
        for k in range(27):
            q = (int(x) + k // 9 - 1, int(y) + (k // 3) % 3 - 1, int(z) + k % 3 - 1)
            if all(0 <= q[a] < shape[a] for a in range(3)):
                table[k, o] = rows.get((int(b),) + q, -1)
    return _lists(table)


def brute_down(indices, shape, batch_size):
    oshape = [int(s) // 2 for s in shape]
    N = len(indices)
    cell = []
    for b, x, y, z in indices:
        q = (int(b), int(x) >> 1, int(y) >> 1, int(z) >> 1)
        ok = 0 <= b < batch_size and min(x, y, z) >= 0 and all(q[a + 1] < oshape[a] for a in range(3))
        cell.append(q if ok else None)
    coarse = sorted({q for q in cell if q is not None})  # lexicographic (b, x, y, z) = ascending linear key
    row_of = {q: i for i, q in enumerate(coarse)}
    f2c = np.asarray([row_of[q] if q is not None else -1 for q in cell], np.int32).reshape(N)
    tap = np.asarray([(int(x) & 1) * 4 + (int(y) & 1) * 2 + (int(z) & 1) for _, x, y, z in indices], np.int32).reshape(N)
    tf, tb = np.full((8, len(coarse)), -1, np.int32), np.full((8, N), -1, np.int32)
    for i in range(N):
        if f2c[i] >= 0:
            tf[tap[i], f2c[i]] = i
            tb[tap[i], i] = f2c[i]
    return dict(out_indices=np.asarray(coarse, np.int32).reshape(-1, 4), out_shape=oshape, fine_to_coarse=f2c, tap=tap,
                num_out=len(coarse), fwd=_lists(tf), bwd=_lists(tb))
