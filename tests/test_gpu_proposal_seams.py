"""GPU: the proposal stage (csrc/proposals.hip) and its post-processing (csrc/postprocess.hip) against the plain reference of
tests/proposal_ref.py on the cases of tests/proposal_cases.py - inputs that sit on the seams of the kernels.

1. hip_ops.proposals_build: every table and count equal, no tolerance (the voxel cells included: the reference transcribes the
   frame one fp32 operation per line), host-counted and with the counts left on the device;
2. hip_ops.proposals_postprocess: host-counted and device-counted, status bytes in LDS and in the workspace: the result equals
   the reference or is None (a neighbour table overflowed - a designed return value), never a wrong table;
3. the per-voxel mean of gathered features and its gradient against float64, with derived bounds.

No input here is out of range."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import proposal_cases as C
from tests import proposal_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from gapartnet_amd import hip_ops
    return hip_ops


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(cuda)  # (a copy: the cases' arrays are read-only)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return R.build(*C.build_args(C.BUILD_CASES[name]()), div="mul")


@functools.lru_cache(maxsize=None)
def _post_ref(name):
    c = C.POST_CASES[name]()
    return R.postprocess(c["score"], c["sizes"], c["proposal_offsets"], c["point_indices"], c["proposal_indices"], c["score_thr"],
                         c["min_points"], c["iou_thr"], live=c["live"])


def _build(H, cuda, c, read_counts=True):
    pts = c["points"]
    if pts.flags.c_contiguous:
        points = dev(pts, cuda)
    else:  # the [N, 3] view of an [N, 6] matrix: the row stride goes through to the kernel
        wide = torch.full((pts.shape[0], 6), 7.5, dtype=torch.float32, device=cuda)
        wide[:, :3] = dev(pts, cuda)
        points = wide[:, :3]
        assert points.stride(0) == 6
    return H.proposals_build(points, dev(c["offset_preds"], cuda), dev(c["sem_preds"], cuda), dev(c["instance_labels"], cuda),
                             dev(c["batch_indices"], cuda), c["batch_size"], c["radius"], c["K1"], c["K2"], c["min_points"],
                             float(c["fullscale"]), float(c["max_scale"]), tuple(torch.from_numpy(j.copy()) for j in c["jitter"]),
                             read_counts=read_counts)


# ------------------------------------------------------------------------------------------------ 1. proposals_build
@pytest.mark.parametrize("name", list(C.BUILD_CASES))
def test_build_equals_the_reference(H, cuda, name):
    want = _ref(name)
    built = _build(H, cuda, C.BUILD_CASES[name]())
    if built is None or want is None:
        R.assert_tables_equal(built, want)
        return
    got = {k: built[k] for k in R.BUILD_COUNTS}
    got.update({k: host(built[k]) for k in R.BUILD_TABLES})
    R.assert_tables_equal(got, want)


@pytest.mark.parametrize("name", list(C.BUILD_CASES))
def test_build_with_the_counts_on_the_device(H, cuda, name):
    c, want = C.BUILD_CASES[name](), _ref(name)
    built = _build(H, cuda, c, read_counts=False)
    N = c["points"].shape[0]
    counts = built["counts"].tolist()
    got = dict(Q=counts[0], M=counts[1], P=counts[2], V=counts[3], dropped=counts[4], coarse=counts[6])
    for key, view in (("Q", "Q_dev"), ("M", "M_dev"), ("P", "P_dev"), ("V", "V_dev"), ("coarse", "coarse_dev")):
        assert int(built[view].item()) == got[key], view
    if want is None:
        assert (got["M"], got["P"], got["V"], got["dropped"]) == (0, 0, 0, 0)
        M = P = 0
    else:
        R.assert_tables_equal(got, {k: want[k] for k in R.BUILD_COUNTS})
        M, P, V, Q = want["M"], want["P"], want["V"], want["Q"]
        live = dict(valid_mask=N, valid_indices=Q, sorted_indices=M, point_indices=M, proposal_indices=M, batch_indices=M, pt_xyz=M,
                    sem_preds=M, instance_labels=M, sizes=P, proposal_offsets=P + 1, member_slot=2 * N, voxel_coords=V, pc_voxel_id=M,
                    point_order=M, voxel_point_start=V + 1)
        tables = {k: None if built[k] is None else host(built[k])[:n] for k, n in live.items()}
        R.assert_tables_equal(tables, {k: want[k] for k in live})
    # the rows behind the live ones: closing offsets, dropped rows in their own order
    assert built["proposal_offsets"].shape[0] == built["P"] + 1 and built["M"] == 2 * N
    assert (host(built["proposal_offsets"])[P:] == M).all()
    assert (host(built["pc_voxel_id"])[M:] == -1).all()
    assert np.array_equal(host(built["point_order"])[M:], np.arange(M, 2 * N))


# ------------------------------------------------------------------------------------------------ 2. proposals_postprocess
def _lds_proposals(n):
    from gapartnet_amd import _C
    f = _C.lib().gpn_proposals_postprocess_lds_proposals
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int64]
    return f(n)


@pytest.mark.parametrize("form", ["lds", "workspace"])
@pytest.mark.parametrize("counted", ["host", "device"])
@pytest.mark.parametrize("name", list(C.POST_CASES))
def test_postprocess_equals_the_reference_or_reports_an_overflow(H, cuda, name, counted, form):
    c, want = C.POST_CASES[name](), _post_ref(name)
    rows = None
    if counted == "device":
        live = c["live"] if c["live"] is not None else len(c["score"])
        rows = H.DevCount(torch.tensor([live], dtype=torch.int64, device=cuda), plan=live)
    before = _lds_proposals(0) if form == "workspace" else None  # (0: every step keeps its status bytes in the workspace)
    try:
        out = H.proposals_postprocess(dev(c["score"], cuda), dev(c["sizes"], cuda), dev(c["proposal_offsets"], cuda),
                                      dev(c["point_indices"], cuda), dev(c["proposal_indices"], cuda), dev(c["member_slot"], cuda),
                                      c["score_thr"], c["min_points"], c["iou_thr"], rows=rows)
        torch.cuda.synchronize()
    finally:
        if before is not None:
            _lds_proposals(before)
    if c["expect"] == "none":
        assert out is None, "a table overflowed: the call must say so"
        return
    if c["expect"] == "equal":
        assert out is not None, "every table of this case fits"
    if out is not None:
        R.assert_tables_equal(dict(zip(R.POST_TABLES, (host(t) for t in out))), want)


# ------------------------------------------------------------------------------------------------ 3. voxel means
U = 2.0 ** -24  # unit roundoff of float32


@pytest.mark.parametrize("C_feat", [16, 3])
@pytest.mark.parametrize("name", ["sizes_63_64_65_128_129_257_513", "fullscale_7", "collapsed_blob"])
def test_voxel_mean_and_its_gradient_against_float64(H, cuda, name, C_feat):
    c, ref = C.BUILD_CASES[name](), _ref(name)
    N, V = c["points"].shape[0], ref["V"]
    rng = np.random.default_rng(V + C_feat)
    feats = rng.standard_normal((N, C_feat)).astype(np.float32)
    t = {k: dev(ref[k], cuda) for k in ("point_indices", "point_order", "voxel_point_start", "member_slot", "pc_voxel_id")}
    want, mag = R.voxel_mean64(feats, ref["point_indices"], ref["point_order"], ref["voxel_point_start"])
    n_v = np.diff(ref["voxel_point_start"]).astype(np.float64)[:, None]
    assert n_v.max() > 1
    # an ordered fp32 sum of n terms is off by at most (n - 1) u sum|x| = (n - 1) u n mean|x| (first order); dividing by n leaves
    # (n - 1) u mean|x|, and the division rounds once more: u |mean| <= u mean|x|.  Together n u mean|x|.
    bound = n_v * U * mag
    got = host(H.proposals_voxel_mean(dev(feats, cuda), t["point_indices"], t["point_order"], t["voxel_point_start"], V))
    err = np.abs(got.astype(np.float64) - want)
    print(f"voxel mean: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), f"voxel {int(np.argwhere(err > bound)[0][0])}"
    # device-counted: the output is sized for a bound, the live count is on the device
    V_b = V + 37
    rows = H.DevCount(torch.tensor([V], dtype=torch.int64, device=cuda), plan=V)
    got_dev = host(H.proposals_voxel_mean(dev(feats, cuda), t["point_indices"], t["point_order"], t["voxel_point_start"], V_b, rows=rows))
    assert got_dev.shape == (V_b, C_feat) and np.array_equal(got_dev[:V], got)
    # backward: d feats[i] = sum over the point's (at most two) memberships of d out[voxel] / n_voxel.  Each quotient rounds
    # once (u |term|) and the one addition rounds once (u |sum| <= u sum|terms|): 2 u sum|terms|; the bound leaves a factor 2.
    dout = rng.standard_normal((V, C_feat)).astype(np.float32)
    want_g, mag_g = R.voxel_mean_bwd64(dout, ref["member_slot"], ref["pc_voxel_id"], ref["voxel_point_start"], N)
    got_g = host(H.proposals_voxel_mean_bwd(dev(dout, cuda), t["member_slot"], t["pc_voxel_id"], t["voxel_point_start"], N))
    err_g, bound_g = np.abs(got_g.astype(np.float64) - want_g), 4 * U * mag_g
    assert ((ref["member_slot"][:N] >= 0) & (ref["member_slot"][N:] >= 0)).any(), "points with two memberships"
    assert (err_g <= bound_g).all(), f"point {int(np.argwhere(err_g > bound_g)[0][0])}"
    assert (got_g[~ref["valid_mask"]] == 0).all()
