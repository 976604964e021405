"""The joint-estimation kernels (csrc/joint.hip, include/gpn.h section JE) on the device against the numpy float64 oracle
(tests/joint_ref.py), the CPU forms and the golden fixture of the reference (tests/golden/joint_axis.npz).

The tolerance rule of the CPD tests is not a fixed number: the oracle itself is run a second time with the rows of X and of Y
randomly permuted - the same mathematics in another summation order - and the largest difference between the two runs over s, R,
t and sigma2 (relative) after k iterations is the oracle's own spread at k.  The device result may differ from the oracle by 64 x
that spread: the device ``exp`` and numpy's may differ by an ulp in every term, which a permutation does not exercise.  Inputs are
chosen so that 64 x spread <= 1e-9 and sigma2 >= 1e-8 at every iteration (both asserted), so that the oracle's
|diff_k - tolerance| >= 1e-5 at every iteration of the default run (asserted): the stopping iteration is then not a matter of
round-off; and so that the permutation's spread is a fair sample at every iteration (asserted; tests/joint_ref.py, CPD_SHAPES).
"""
import os

import numpy as np
import pytest
import torch

from gapartnet_amd.misc import joint_fitting as JF
from tests import joint_ref as JR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "joint_axis.npz")

SHAPES, LIVE = JR.CPD_SHAPES, JR.CPD_LIVE   # the shared batch: inputs, oracle runs and the oracle's spread live in tests/joint_ref.py
MAX_ITERATIONS = 100   # the default: four pairs stop by the rule before it ((500, 500) among them), (1100, 900) runs into it
TOL = 1e-3             # the default tolerance
FACTOR = 64.0
_batch, _oracle, _gap = JR.cpd_batch, JR.cpd_oracle, JR.state_gap


def _run(cuda, X, Y, nx, ny, **kw):
    got = JF.cpd_rigid_batched(torch.from_numpy(X).to(cuda), torch.from_numpy(Y).to(cuda), torch.from_numpy(nx), torch.from_numpy(ny), **kw)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _state(got, b):
    return got["s"][b], got["R"][b], got["t"][b], got["sigma2"][b]


def test_the_inputs_meet_the_conditions_of_the_tolerance_rule():
    """over the oracle's whole default run of every pair: 64 x spread <= 1e-9, sigma2 >= 1e-8, and no diff within 1e-5 of the
    tolerance; the permutation's spread is a fair sample at every iteration (never below 1/16 of its running maximum: the reasoning
    is with CPD_SHAPES in tests/joint_ref.py); the (500, 500) pair stops by the rule, and one pair runs into max_iterations"""
    stops = {}
    for b, o in _oracle().items():
        print(f"pair {SHAPES[b][0]}: stop {o['stop']}, spread {min(o['spread']):.1e} .. {max(o['spread']):.1e}, sigma2 >= "
              f"{min(h[3] for h in o['history']):.1e}, |diff - tolerance| >= {min(abs(d - TOL) for d in o['diffs'][:o['stop']]):.1e}")
        assert all(FACTOR * s <= 1e-9 for s in o["spread"]), (b, max(o["spread"]))
        assert all(h[3] >= 1e-8 for h in o["history"]), b
        assert all(abs(d - TOL) >= 1e-5 for d in o["diffs"][:o["stop"]]), b
        spread = np.array(o["spread"])
        assert (spread * JR.CPD_FAIR >= np.maximum.accumulate(spread)).all(), (b, (np.maximum.accumulate(spread) / spread).max())
        stops[SHAPES[b][0]] = o["stop"]
    assert stops[(500, 500)] < MAX_ITERATIONS and max(stops.values()) == MAX_ITERATIONS, stops


@pytest.mark.parametrize("iterations", [1, 5, 30])
def test_cpd_rigid_matches_the_oracle_at_a_fixed_iteration_count(cuda, iterations):
    """tolerance 0: every pair runs exactly ``iterations`` iterations.  s, R, t (absolute) and sigma2 (relative) against the oracle
    within 64 x the oracle's own spread under a row permutation; the (500, 500) pair also as a batch of one.
    Observed on the MI355X (the table in profiles/joint_bench.txt): after 1 iteration the spread is 2.5e-16 .. 6.7e-16 and the
    kernel's error 3.9e-16 .. 1.0e-15 (at most 1.9 x the spread); after 5, 1.5e-15 .. 1.3e-14 and 8.9e-16 .. 8.1e-15 (at most
    4.4 x); after 30, 2.9e-15 .. 2.3e-13 and 5.6e-16 .. 3.0e-14 (at most 4.1 x); 64 x is allowed."""
    X, Y, nx, ny = _batch()
    got = _run(cuda, X, Y, nx, ny, tolerance=0.0, max_iterations=iterations)
    one = _run(cuda, X[3:4, :500], Y[3:4, :500], nx[3:4], ny[3:4], tolerance=0.0, max_iterations=iterations)
    failures = []
    for b, o in _oracle().items():
        want, spread = o["history"][iterations - 1], o["spread"][iterations - 1]
        err = _gap(_state(got, b), want)
        print(f"iterations {iterations} pair {SHAPES[b][0]}: spread {spread:.2e} kernel error {err:.2e} ratio {err / spread:.1f}")
        assert got["iterations"][b] == iterations
        if not err <= FACTOR * spread:
            failures.append((SHAPES[b][0], err, spread))
    err = _gap(_state(one, 0), _oracle()[3]["history"][iterations - 1])
    assert err <= FACTOR * _oracle()[3]["spread"][iterations - 1], err
    assert not failures, failures


def test_cpd_rigid_at_the_default_tolerance_stops_where_the_oracle_stops(cuda):
    """default tolerance and max_iterations: iterations equal the oracle's, the results agree within the rule, and every entry k
    of sigma2_trace is the oracle's sigma2 after iteration k + 1 within the rule at that iteration count - 64 x the spread of
    (s, R, t, sigma2) there - and NaN after the last.  Observed on the MI355X: 34, 36, 36, 59, 100
    iterations; final states: spread 1.5e-14 .. 3.2e-13, kernel error 4.3e-14 .. 2.1e-13 (at most 3.2 x the spread); the worst
    trace entry of each pair: 23.1 x (entry 7: spread 6.7e-16, error 1.5e-14), 17.9 x, 6.0 x, 11.0 x, 3.5 x the spread there."""
    X, Y, nx, ny = _batch()
    got = _run(cuda, X, Y, nx, ny, want_trace=True)
    assert got["sigma2_trace"].shape == (len(SHAPES), MAX_ITERATIONS)
    failures = []
    for b, o in _oracle().items():
        stop = o["stop"]
        assert got["iterations"][b] == stop, (b, got["iterations"][b], stop)
        err, spread = _gap(_state(got, b), o["history"][stop - 1]), o["spread"][stop - 1]
        print(f"default tolerance pair {SHAPES[b][0]}: {stop} iterations, spread {spread:.2e} kernel error {err:.2e} ratio {err / spread:.1f}")
        assert err <= FACTOR * spread, (b, err, spread)
        trace, want = got["sigma2_trace"][b], np.array([h[3] for h in o["history"][:stop]])
        ratio = np.abs(trace[:stop] - want) / want / np.array(o["spread"][:stop])
        k = int(np.argmax(ratio))
        print(f"   sigma2_trace: worst entry {k}: spread {o['spread'][k]:.2e} kernel error {ratio[k] * o['spread'][k]:.2e} ratio {ratio[k]:.1f}")
        failures += [(SHAPES[b][0], int(j), float(ratio[j])) for j in np.nonzero(~(ratio <= FACTOR))[0]]
        assert np.isnan(trace[stop:]).all()
    assert not failures, failures


def test_degenerate_pairs_are_nan_and_leave_the_others_untouched(cuda):
    """(0, 50): nothing to register - NaN and 0 iterations; (1, 1): YPY = 0, so s = 0 / 0 and everything after it is NaN, after
    one iteration, as in the oracle.  Every other pair of the batch is bit-equal to the same pair run alone."""
    X, Y, nx, ny = _batch()
    got = _run(cuda, X, Y, nx, ny, tolerance=0.0, max_iterations=5, want_trace=True)
    for name in ("s", "R", "t", "sigma2", "q", "diff", "sigma2_trace"):
        assert np.isnan(got[name][5]).all(), name
    assert got["iterations"][5] == 0
    want = JR.cpd_rigid_ref(X[6, :1], Y[6, :1], tolerance=0.0, max_iterations=5)
    assert got["iterations"][6] == want["iterations"] == 1
    for name in ("s", "t", "sigma2", "q", "diff"):
        assert np.isnan(got[name][6]).all() and np.isnan(want[name]).all(), name
    for b in LIVE:
        k = max(nx[b], ny[b])
        alone = _run(cuda, X[b:b + 1, :k].copy(), Y[b:b + 1, :k].copy(), nx[b:b + 1], ny[b:b + 1], tolerance=0.0, max_iterations=5,
                     want_trace=True)
        for name, v in alone.items():
            assert np.array_equal(v[0], got[name][b], equal_nan=True), (b, name)


def test_two_runs_are_bit_equal(cuda):
    X, Y, nx, ny = _batch()
    a = _run(cuda, X, Y, nx, ny, max_iterations=12, want_trace=True)
    b = _run(cuda, X, Y, nx, ny, max_iterations=12, want_trace=True)
    for name in a:
        assert np.array_equal(a[name], b[name], equal_nan=True), name


@pytest.mark.parametrize("n", [1, 63, 4097])
def test_joint_sample_within_derived_bounds(cuda, n):
    """n rows in every segment, k < K picks.  With eps = 2^-53 and a = the largest |coordinate|: a mean of n numbers summed in any
    order is within n eps a of the exact mean, so the kernel's M and the oracle's differ by eM <= 2 n eps a.  p - M then differs
    by eM + 2 a eps (its own rounding, |p - M| <= 2 a), the extent S = max - min by eS <= 2 (eM + 2 a eps) + 2 a eps, and
    (p - M) / S, whose size is at most 2 a / S, by (eM + 2 a eps) / S + (2 a / S)(eS / S) + 2 a eps / S, to first order.
    n = 1: M is the point, S = 0 and the division gives the same inf / NaN bit for bit."""
    rng = np.random.RandomState(n)
    K, ks = 48, ((min(n, 40), min(n, 31)), (min(n, 17), min(n, 40)))
    pcs1 = [rng.randn(n, 3) * 0.3 + [0.2, -0.1, 1.4], rng.randn(n, 3) * 2.0 + [5.0, 1.0, -3.0]]
    pcs2 = [rng.randn(n, 3) * 0.3 + [0.25, -0.1, 1.4], rng.randn(n, 3) * 2.0 + [5.0, 1.5, -3.0]]
    picks1, picks2 = np.zeros((2, K), np.int64), np.zeros((2, K), np.int64)
    for b, (k1, k2) in enumerate(ks):
        picks1[b, :k1], picks2[b, :k2] = rng.choice(n, k1, replace=False), rng.choice(n, k2, replace=False)
    from gapartnet_amd import hip_ops
    off = torch.tensor([0, n, 2 * n], dtype=torch.int64).to(cuda)
    X, Y, norm = hip_ops.joint_sample(torch.from_numpy(np.concatenate(pcs1)).to(cuda), torch.from_numpy(np.concatenate(pcs2)).to(cuda), off,
                                      off, torch.from_numpy(picks1).to(cuda), torch.from_numpy(picks2).to(cuda),
                                      torch.tensor([k[0] for k in ks], dtype=torch.int32).to(cuda),
                                      torch.tensor([k[1] for k in ks], dtype=torch.int32).to(cuda))
    X, Y, norm = X.cpu().numpy(), Y.cpu().numpy(), norm.cpu().numpy()
    eps = 2.0 ** -53
    for b, (k1, k2) in enumerate(ks):
        with np.errstate(all="ignore"):
            x, y, nrm = JR.joint_sample_ref(pcs1[b], pcs2[b], picks1[b, :k1], picks2[b, :k2])
        assert not X[b, k1:].any() and not Y[b, k2:].any(), "rows beyond k are zero"
        if n == 1:
            assert nrm[0] == 0 and np.array_equal(norm[b], nrm)
            assert np.array_equal(X[b, :k1], x, equal_nan=True) and np.array_equal(Y[b, :k2], y, equal_nan=True)
            continue
        a = max(np.abs(pcs1[b]).max(), np.abs(pcs2[b]).max())
        S = nrm[0]
        eM = 2 * n * eps * a
        eS = 2 * (eM + 2 * a * eps) + 2 * a * eps
        eX = (eM + 2 * a * eps) / S + (2 * a / S) * (eS / S) + 2 * a * eps / S
        assert np.abs(norm[b, 1:] - nrm[1:]).max() <= eM and abs(norm[b, 0] - S) <= eS
        assert np.abs(X[b, :k1] - x).max() <= eX and np.abs(Y[b, :k2] - y).max() <= eX


@pytest.mark.parametrize("joint_type", ["revolute", "prismatic"])
def test_joint_from_rigid_matches_the_cpu_form(cuda, joint_type):
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(3)
    G = 70
    rot = Rotation.from_rotvec(rng.randn(G, 3)).as_matrix()
    rot[0] = np.eye(3)                                         # angle 0: a NaN axis, as in the reference
    rot[1] = Rotation.from_rotvec([0, np.deg2rad(179.0), 0]).as_matrix()
    trans, norm = rng.randn(G, 3) * 0.2, np.concatenate([rng.rand(G, 1) + 0.2, rng.randn(G, 3)], 1)
    want = JF.joint_from_rigid(torch.from_numpy(rot), torch.from_numpy(trans), torch.from_numpy(norm), joint_type)
    got = JF.joint_from_rigid(torch.from_numpy(rot).to(cuda), torch.from_numpy(trans).to(cuda), torch.from_numpy(norm).to(cuda), joint_type)
    for g, w_ in zip(got, want):
        assert torch.allclose(g.cpu(), w_, rtol=0, atol=1e-12, equal_nan=True)
    if joint_type == "revolute":
        assert bool(torch.isnan(got[0][0]).all()) and float(got[2][0]) == 0.0
        assert not bool(torch.isnan(got[0][1:]).any())


def test_estimate_joints_on_the_gpu_matches_the_cpu_path_on_the_golden_pairs(cuda):
    import random
    g = np.load(GOLD)
    names = [str(n) for n in g["names"]]
    pc1s, pc2s = [torch.from_numpy(g[f"{n}/pc1"]) for n in names], [torch.from_numpy(g[f"{n}/pc2"]) for n in names]
    K = 64
    random.seed(5)
    picks = JF.draw_joint_picks([p.shape[0] for p in pc1s], [p.shape[0] for p in pc2s], K)
    rp = torch.from_numpy(np.stack([g[f"{n}/ransac_picks"] % K for n in names]))
    want = JF.estimate_joints(pc1s, pc2s, picks=picks, ransac_picks=rp)
    got = JF.estimate_joints([p.to(cuda) for p in pc1s], [p.to(cuda) for p in pc2s], picks=picks, ransac_picks=rp)
    assert torch.equal(got.iterations.cpu(), want.iterations)
    assert torch.allclose(got.norm.cpu(), want.norm, rtol=0, atol=1e-12)
    for leg in ("cpd", "ransac"):
        a, b = getattr(got, leg), getattr(want, leg)
        for field, tol in (("axis", 1e-9), ("angle", 1e-9), ("rotation", 1e-9), ("translation", 1e-9), ("pivot", 1e-8)):
            assert torch.allclose(getattr(a, field).cpu(), getattr(b, field), rtol=0, atol=tol, equal_nan=True), (leg, field)
    assert not bool(torch.isnan(got.cpd.axis).any())


def _slab_frames(angle_deg, H=24, W=32):
    """two depth frames [H,W] f32 of a 0.5 x 0.36 rectangle 1.2 in front of the camera, before and after it turned about its left
    edge (a vertical axis), with the rectangle's mask in each, the camera, and the truth (axis, a point on it, the angle)"""
    K = np.array([[38.0, 0.0, 15.5], [0.0, 38.0, 11.5], [0.0, 0.0, 1.0]])
    hinge, axis = np.array([-0.25, 0.0, 1.2]), np.array([0.0, 1.0, 0.0])
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    frames = []
    for a in (np.deg2rad(8.0), np.deg2rad(8.0 + angle_deg)):
        along = np.array([np.cos(a), 0.0, np.sin(a)])          # the rectangle's width direction, turning about the hinge
        normal = np.cross(along, axis)
        z = (hinge @ normal) / (rays @ normal)
        pts = rays * z[..., None]
        s, t = (pts - hinge) @ along, (pts - hinge) @ axis
        mask = (z > 0) & (s >= 0) & (s <= 0.5) & (np.abs(t) <= 0.18)
        frames.append((np.where(mask, z, 0.0).astype(np.float32), mask))
    return frames, K, (axis, hinge, np.deg2rad(angle_deg))


def test_joints_from_frames_recovers_a_turned_slab(cuda):
    """two 24 x 32 depth frames of a rectangle turned by 24 degrees: the angle within 1 degree and the axis within 2 degrees of the
    truth - loose functional bounds, which the numpy oracle meets on the same back-projected pixels (asserted too)"""
    from gapartnet_amd import inference
    (fa, fb), K, (axis, hinge, angle) = _slab_frames(24.0)
    got = JF.joints_from_frames(torch.from_numpy(fa[0]).to(cuda), torch.from_numpy(fb[0]).to(cuda), K, torch.from_numpy(fa[1]).to(cuda),
                                torch.from_numpy(fb[1]).to(cuda))
    clouds = []
    for depth, mask in (fa, fb):
        rows, valid = inference._backproject_numpy(depth[None], np.zeros((1,) + depth.shape + (3,), np.uint8), K[None], mask[None], 1.0, False)
        clouds.append(rows[valid[0], :3].astype(np.float64))
    x, y, nrm = JR.joint_sample_ref(clouds[0], clouds[1], np.arange(len(clouds[0])), np.arange(len(clouds[1])))
    ref = JR.cpd_rigid_ref(x, y)
    ref_axis, _, ref_angle = JR.joint_from_rigid_ref(ref["R"], ref["t"], nrm)

    def off_axis(a):
        return np.rad2deg(np.arccos(min(1.0, abs(float(np.dot(a, axis))))))
    for name, ax, an in (("oracle", ref_axis, ref_angle), ("device", got.cpd.axis[0].cpu().numpy(), float(got.cpd.angle[0]))):
        print(f"{name}: angle {np.rad2deg(an):.3f} deg (truth {np.rad2deg(angle):.1f}), axis off by {off_axis(ax):.3f} deg")
        assert abs(np.rad2deg(an) - np.rad2deg(angle)) <= 1.0, name
        assert off_axis(ax) <= 2.0, name
    assert int(got.iterations[0]) == ref["iterations"]
