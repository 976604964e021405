"""Pins the CPU oracle at the edge inputs of tests/op_edge_cases.py against the independent numpy statements kept there
(stable argsort, fancy indexing, the FPS tie-break in closed form, scipy connected components, the plain NMS loop, per-segment
loops, the one-hot product).  tests/test_gpu_op_edges.py compares the HIP kernels with the oracle on the very same inputs; the
oracle functions of the PointNet++ family are line-by-line twins of the kernels, so without these pins a misreading shared by
both would pass.  No GPU."""
import numpy as np
import pytest

import oracle as O
from tests import op_edge_cases as E


@pytest.mark.parametrize("n,m,k", E.KNN_SHAPES)
def test_knn_and_three_nn_vs_stable_argsort(n, m, k):
    unknown, known, dist, idx, dist3, idx3 = E.knn_case(n, m, k)
    d, i = O.pn2_knn(unknown, known, k)
    assert np.array_equal(i, idx) and np.array_equal(d, dist)
    d, i = O.pn2_three_nn(unknown, known)
    assert np.array_equal(i, idx3) and np.array_equal(d, dist3)
    if m < 3:
        assert np.isinf(dist3[..., m:]).all() and not idx3[..., m:].any()
    if m > 1:
        live = min(k, m)
        assert (dist[..., 1:live] == dist[..., :live - 1]).any(), "the lattice must produce exact ties"


@pytest.mark.parametrize("n,m,nsample", E.PN2_BALL_SHAPES)
def test_pn2_ball_query_vs_numpy(n, m, nsample):
    xyz, new_xyz, idx = E.pn2_ball_case(n, m, nsample)
    assert np.array_equal(O.pn2_ball_query(E.PN2_BALL_RADIUS, nsample, xyz, new_xyz), idx)
    if m > 3:
        assert not idx[:, 3::4].any(), "the far queries have no hit: rows stay zero"


def test_pn2_ball_query_cases_cover_truncation_and_padding():
    _, _, idx = E.pn2_ball_case(700, 300, 16)
    assert (np.diff(idx[:, 0::4], axis=-1) > 0).all(-1).any(), "a row with nsample distinct ascending hits (truncated)"
    _, _, idx = E.pn2_ball_case(257, 256, 64)
    rows = idx[:, 0::4].reshape(-1, 64)
    assert (rows[:, -1] == rows[:, 0]).all(), "nsample above the hits: every row ends in padding with its first hit"


@pytest.mark.parametrize("n", E.FPS_SIZES)
def test_fps_vs_closed_form(n):
    xyz, want, m = E.fps_case(n)
    assert np.array_equal(O.pn2_furthest_point_sampling(xyz, m), want)
    if m > n:
        assert len(set(want[0].tolist())) < m


@pytest.mark.parametrize("name", E.CCL_CASES)
def test_ccl_vs_scipy(name):
    be, edges, labels, compact = E.ccl_case(name)
    assert np.array_equal(O.ccl(be, edges, compacted=False), labels)
    assert np.array_equal(O.ccl(be, edges, compacted=True), compact)
    n_comp = {"permuted_path": 1, "star_hub_last": 1, "two_paths_bridge_junk": 101, "no_edges": 1025}[name]
    assert compact.max() + 1 == n_comp


@pytest.mark.parametrize("kind", E.NMS_KINDS)
@pytest.mark.parametrize("P", E.NMS_SIZES)
def test_nms_vs_python_loop(P, kind):
    ious, scores, keep = E.nms_case(P, kind)
    assert np.array_equal(O.nms(ious, scores, E.NMS_THR), keep)


@pytest.mark.parametrize("C", E.SEG_CHANNELS)
def test_segmented_ops_vs_per_segment_loop(C):
    vals, begin, end, red, pooled, arg = E.segment_case(C)
    for mode in ("sum", "min", "max"):
        assert np.array_equal(O.segmented_reduce(vals, begin, end, mode), red[mode]), mode
    p, a = O.segmented_maxpool(vals, begin, end)
    assert np.array_equal(p, pooled) and np.array_equal(a, arg)
    assert (arg[[0, 4, 7]] == -1).all() and np.isneginf(pooled[6]).all() and (arg[6] == begin[6]).all()
    assert (arg[3] == begin[3]).all(), "ties: the first occurrence wins"


@pytest.mark.parametrize("I", E.IOU_INSTANCES)
def test_instance_iou_vs_onehot(I):
    offs, il, bi, npi, want = E.iou_case(I)
    assert np.array_equal(O.instance_iou(offs, il, bi, npi), want)
    assert (il == -1).any() and (il >= I).any() and not want[7].any()


def test_group_gather_interpolate_vs_fancy_indexing():
    g = E.gather_case()
    assert np.array_equal(O.pn2_group_points(g["feats"], g["gidx"]), g["grouped"])
    assert np.array_equal(O.pn2_gather_points(g["feats"], g["sidx"]), g["gathered"])
    assert np.array_equal(O.pn2_three_interpolate(g["known"], g["idx3"], g["w"]), g["interp"])


@pytest.mark.parametrize("kind", E.GRAD_KINDS)
@pytest.mark.parametrize("op", ["group_points", "gather_points", "three_interpolate"])
def test_gradient_oracles_within_the_summation_bound(op, kind):
    """the oracle's ordered float32 sums obey the bound the GPU test applies to the kernels' atomic sums"""
    args, ref, bound = E.grad_case(op, kind)
    got = getattr(O, "pn2_" + op + "_grad")(*args)
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
