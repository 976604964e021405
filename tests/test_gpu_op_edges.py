"""GPU parity at the edges: the grouping (csrc/cluster.hip) and PointNet++ (csrc/pointnet2.hip) kernels against the CPU
oracle on the inputs of tests/op_edge_cases.py, where tests/test_oracle_pins_edges.py pins the oracle to independent numpy
statements.  Everything with a fixed order is compared with np.array_equal (indices, distances including the inf slots, pooled
values and arg-max, ordered sums, IoU, keep lists, labels); the three atomic gradient kernels are compared with a float64 sum
under a derived bound.  Every index handed to a gather / group kernel is in range and no input holds a NaN."""
import os

import numpy as np
import pytest
import torch

import oracle as O
from tests import op_edge_cases as E

pytestmark = pytest.mark.gpu


def dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)  # (a copy: the shared cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def H():
    from gapartnet_amd import hip_ops
    return hip_ops


if os.environ.get("GPN_TEST_LOGIC_ON_CPU"):
    # self-check of the test logic in a GPU-less container: oracle vs oracle on CPU tensors (proves nothing about
    # the kernels; never set on the GPU box)
    @pytest.fixture(scope="module")
    def H():  # noqa: F811
        from oracle import torch_ops
        return torch_ops

    @pytest.fixture(scope="module")
    def cuda():  # noqa: F811
        return torch.device("cpu")


# ------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("n,m,k", E.KNN_SHAPES)
def test_knn_and_three_nn_with_ties_and_short_clouds(H, cuda, n, m, k):
    """exact distance ties (lattice points), m < 3, m < k (index 0 / inf in the unused slots), k = 200, n and m across the
    256-point tile edge of three_nn"""
    unknown, known = E.knn_case(n, m, k)[:2]
    d, i = H.pn2_knn(dev(unknown, cuda), dev(known, cuda), k)
    rd, ri = O.pn2_knn(unknown, known, k)
    assert np.array_equal(host(i), ri) and np.array_equal(host(d), rd)
    d, i = H.pn2_three_nn(dev(unknown, cuda), dev(known, cuda))
    rd, ri = O.pn2_three_nn(unknown, known)
    assert np.array_equal(host(i), ri) and np.array_equal(host(d), rd)


@pytest.mark.parametrize("n,m,nsample", E.PN2_BALL_SHAPES)
def test_pn2_ball_query_without_hits_and_past_the_hits(H, cuda, n, m, nsample):
    """queries without a hit (row stays zero), nsample above the hits (padding with the first hit), truncation, n at 255 /
    256 / 257 (the candidate tile), m at 256 / 257 (the query block)"""
    xyz, new_xyz, _ = E.pn2_ball_case(n, m, nsample)
    got = host(H.pn2_ball_query(E.PN2_BALL_RADIUS, nsample, dev(xyz, cuda), dev(new_xyz, cuda)))
    assert np.array_equal(got, O.pn2_ball_query(E.PN2_BALL_RADIUS, nsample, xyz, new_xyz))


@pytest.mark.parametrize("n", E.FPS_SIZES)
def test_fps_across_the_reference_block_sizes(H, cuda, n):
    """n from 1 to 3000: every reference block size 1 .. 1024, n one off a power of two, fewer points than a wave, more
    samples than points (repeated picks); an integer lattice, so almost every step is decided by the tie-break"""
    xyz, _, m = E.fps_case(n)
    assert np.array_equal(host(H.pn2_furthest_point_sampling(dev(xyz, cuda), m)), O.pn2_furthest_point_sampling(xyz, m))


def test_group_gather_interpolate_forward(H, cuda):
    g = E.gather_case()
    assert np.array_equal(host(H.pn2_group_points(dev(g["feats"], cuda), dev(g["gidx"], cuda))),
                          O.pn2_group_points(g["feats"], g["gidx"]))
    assert np.array_equal(host(H.pn2_gather_points(dev(g["feats"], cuda), dev(g["sidx"], cuda))),
                          O.pn2_gather_points(g["feats"], g["sidx"]))
    assert np.array_equal(host(H.pn2_three_interpolate(dev(g["known"], cuda), dev(g["idx3"], cuda), dev(g["w"], cuda))),
                          O.pn2_three_interpolate(g["known"], g["idx3"], g["w"]))


@pytest.mark.parametrize("kind", E.GRAD_KINDS)
@pytest.mark.parametrize("op", ["group_points", "gather_points", "three_interpolate"])
def test_atomic_gradient_kernels_within_the_summation_bound(H, cuda, op, kind):
    """group_points_grad / gather_points_grad / three_interpolate_grad add with atomics in no fixed order: elementwise
    against a float64 sum of the same float32 addends, bound (k + 1) 2^-24 sum|addend| (tests/op_edge_cases.grad_case);
    `contended`: 2048 addends on one element; `sparse`: most elements receive nothing and must be exactly zero"""
    args, ref, bound = E.grad_case(op, kind)
    targs = [dev(a, cuda) if isinstance(a, np.ndarray) else a for a in args]
    got = host(getattr(H, "pn2_" + op + "_grad")(*targs)).astype(np.float64)
    err = np.abs(got - ref)
    print(op, kind, "max err", err.max(), "max err / bound", (err[bound > 0] / bound[bound > 0]).max())
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ B / L
@pytest.mark.parametrize("case", ["labels", "truncated", "shuffled_batches"])
def test_plain_ball_query(H, cuda, case):
    """fewer than 2048 points: gpn_ball_query itself (not the grid form) with the label filter, with truncation at K and with
    queries in shuffled batch order; 1500 points in 3 segments, the middle one empty"""
    rng = np.random.default_rng({"labels": 1, "truncated": 2, "shuffled_batches": 3}[case])
    offs = np.array([0, 700, 700, 1500], np.int32)
    Np = 1500
    assert Np < 2048
    batch = np.repeat(np.arange(3, dtype=np.int32), np.diff(offs))
    K, r = 16, 0.05
    if case == "truncated":
        centres = rng.uniform(-0.5, 0.5, (5, 3))
        pts = (centres[rng.integers(0, 5, Np)] + rng.normal(scale=0.004, size=(Np, 3))).astype(np.float32)
        K = 4
    else:
        pts = rng.uniform(-0.2, 0.2, (Np, 3)).astype(np.float32)
    lab = rng.integers(1, 4, Np).astype(np.int32) if case == "labels" else None
    q, qb, ql = pts, batch, lab
    if case == "shuffled_batches":
        q = np.concatenate([pts[::2] + np.float32(0.01), rng.uniform(-0.2, 0.2, (300, 3)).astype(np.float32)])
        qb = rng.integers(0, 3, q.shape[0]).astype(np.int32)  # includes queries into the empty segment
    ref_idx, ref_cnt = O.ball_query(pts, q, qb, offs, r, K, lab, ql)
    idx, cnt = H.ball_query(dev(pts, cuda), dev(q, cuda), dev(qb, cuda), dev(offs, cuda), r, K,
                            None if lab is None else dev(lab, cuda), None if ql is None else dev(ql, cuda))
    assert np.array_equal(host(cnt), ref_cnt) and np.array_equal(host(idx), ref_idx)
    if case == "truncated":
        assert (ref_cnt == K).mean() >= 0.5, "most queries must truncate at K"
    if case == "shuffled_batches":
        assert (ref_cnt[qb == 1] == 0).all() and (qb == 1).any() and ref_cnt.max() > 1


@pytest.mark.parametrize("name", E.CCL_CASES)
def test_ccl_on_one_sided_graphs(H, cuda, name):
    """edges listed on one side only (a permuted path: chains of hooks), a 2499-edge row at the highest vertex, ignored
    entries (-1, >= Q), isolated vertices, no edge at all; plain and compacted labels"""
    be, edges, _, _ = E.ccl_case(name)
    for compacted in (False, True):
        got = host(H.ccl(dev(be, cuda), dev(edges, cuda), compacted))
        assert np.array_equal(got, O.ccl(be, edges, compacted)), compacted


# ------------------------------------------------------------------------------------------------ R / I / N
@pytest.mark.parametrize("kind", E.NMS_KINDS)
@pytest.mark.parametrize("P", E.NMS_SIZES)
def test_nms_across_the_mask_word_edges(H, cuda, P, kind):
    """P = 1, 63 / 64 / 65 and 129 (one, two and three 64-bit mask words), asymmetric matrices (row = the kept proposal),
    entries equal to the threshold, suppression chains, everything / nothing overlapping"""
    ious, scores, _ = E.nms_case(P, kind)
    got = host(H.nms(dev(ious, cuda), dev(scores, cuda), E.NMS_THR))
    assert np.array_equal(got, O.nms(ious, scores, E.NMS_THR))


@pytest.mark.parametrize("C", E.SEG_CHANNELS)
def test_segmented_ops_channel_counts_and_empty_segments(H, cuda, C):
    """C = 3, 48, 100 take the serial max-pool kernel (256 % C != 0), C = 1 and 256 the two ends of the workgroup form;
    empty segments first / middle / last, one row, 700 rows, ties, a segment of -inf; the backward on that arg-max"""
    vals, begin, end = E.segment_case(C)[:3]
    tv, tb, te = dev(vals, cuda), dev(begin, cuda), dev(end, cuda)
    for mode in ("sum", "min", "max"):
        assert np.array_equal(host(H.segmented_reduce(tv, tb, te, mode)), O.segmented_reduce(vals, begin, end, mode)), mode
    p, a = H.segmented_maxpool_fwd(tv, tb, te)
    rp, ra = O.segmented_maxpool(vals, begin, end)
    assert np.array_equal(host(p), rp) and np.array_equal(host(a), ra)
    g = np.random.default_rng(C).normal(size=rp.shape).astype(np.float32)
    M = vals.shape[0]
    dv = host(H.segmented_maxpool_bwd(dev(g, cuda), a, M))
    assert np.array_equal(dv, O.segmented_maxpool_bwd(g, ra, M))
    selected = np.zeros((M, C), bool)
    live = ra >= 0
    selected[ra[live], np.broadcast_to(np.arange(C), ra.shape)[live]] = True
    assert not dv[~selected].any() and selected.sum() == 5 * C, "zero wherever nothing was selected; 5 non-empty segments"


@pytest.mark.parametrize("I", E.IOU_INSTANCES)
def test_instance_iou_instance_counts(H, cuda, I):
    """I = 1, 129 (one past the 128-thread stride) and 300; an empty proposal, labels -1 and >= I, a proposal of 200 points"""
    offs, il, bi, npi, _ = E.iou_case(I)
    got = host(H.instance_iou(dev(offs, cuda), dev(il, cuda), dev(bi, cuda), dev(npi, cuda)))
    assert np.array_equal(got, O.instance_iou(offs, il, bi, npi))
