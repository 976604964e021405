"""Object isolation on the GPU (include/gpn.h section OB; csrc/isolate.hip): every stage at its seam, fed the inputs of the numpy /
scipy restatement (tests/isolate_ref.py) on the seeded scenes of tests/isolate_scenes.py.  Every comparison is exact except the
refit, the only stage whose float result depends on a summation order."""
import numpy as np
import pytest
import torch

from tests import isolate_ref as R
from tests import isolate_scenes as S

pytestmark = pytest.mark.gpu
CFG = S.CFG
TOL = CFG["tol"]
# refit: |kernel - float64 numpy| per component of (n, d).  E_ref = |float64 numpy - longdouble numpy| is the rounding noise of the
# problem itself (about 1e-16 here: the scatter's entries are ~1e2, its gap ~5e1, so eps * |C| / gap ~ 2e-16 rad, and forming C
# about p0 adds eps * |Q| / gap of the same size).  The kernel's summation tree and Jacobi SVD differ from numpy's pairwise sum and
# LAPACK by a few such roundings; 1e-10 is five orders above that estimate and seven below tol.
REFIT_ABS = 1e-10


def _upload(scenes, cuda, seeds=None):
    """a batch of same-size scenes -> (rows, valid, valid_counts, pix, seeds) on the device and per frame (xyz, valid) on the host"""
    from gapartnet_amd import hip_ops
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)  # noqa: E731
    seeds = [s["seed"] for s in scenes] if seeds is None else seeds
    rows, valid, vc = hip_ops.frame_backproject(t(np.stack([s["depth"] for s in scenes])), t(np.stack([s["rgb"] for s in scenes])),
                                                t(np.stack([s["K"] for s in scenes])))
    _, pix, _, _ = hip_ops.frame_select(rows, valid, vc, seeds, 0)
    host = [R.backproject(s["depth"], s["K"]) for s in scenes]
    H, W = scenes[0]["depth"].shape
    got = rows.cpu().numpy().reshape(len(scenes), H * W, 6)
    for v, (xyz, ok) in enumerate(host):
        assert np.array_equal(got[v, :, :3], xyz, equal_nan=True) and np.array_equal(valid[v].cpu().numpy().reshape(-1) != 0, ok)
    return rows, valid, vc, pix, seeds, host


def _names(names):
    return [S.scene(n) for n in names]


BATCHES = [["s48x64", "clean", "tile"], ["s61x97", "wall"], ["tile-1"], ["tile+1"], ["1x1"], ["1xW"], ["Hx1"]]


@pytest.mark.parametrize("names", BATCHES, ids=lambda n: "+".join(n))
def test_hypotheses_score_winner(cuda, names):
    from gapartnet_amd import hip_ops
    scenes = _names(names)
    rows, valid, vc, pix, seeds, host = _upload(scenes, cuda)
    H, W = scenes[0]["depth"].shape
    cand = hip_ops.frame_candidates(rows, valid)
    for n_hyp in (256, 1, 255, 1024):
        hyp, hyp_pix = hip_ops.frame_plane_hypotheses(rows, cand, pix, vc, seeds, n_hyp, 0)
        counts = hip_ops.frame_plane_score(rows, cand, hyp, TOL)
        counts1 = hip_ops.frame_plane_score(rows, cand, hyp, TOL, variant=1)
        win = hip_ops.frame_plane_winner(counts)
        for v, (xyz, ok) in enumerate(host):
            c = R.candidates(xyz, ok)
            assert np.array_equal(cand[v].cpu().numpy().reshape(-1) != 0, c)
            h, hp = R.hypotheses(xyz, c, ok, seeds[v], n_hyp, 0)
            assert np.array_equal(hyp[v].cpu().numpy(), h, equal_nan=True), (names[v], n_hyp)
            assert np.array_equal(hyp_pix[v].cpu().numpy(), hp)
            want = R.score(xyz, c, h, TOL)
            assert np.array_equal(counts[v].cpu().numpy(), want) and np.array_equal(counts1[v].cpu().numpy(), want), (names[v], n_hyp)
            assert int(win[v]) == R.winner(want)


def test_hypotheses_degenerate_and_redrawn(cuda):
    """a frame of 3 valid pixels (most triples repeat a rank), the collinear pixels of a 1 x W frame (every triple degenerate), and
    round 1 after a cut: pixels that are no candidates are redrawn, a hypothesis whose tries all miss is degenerate"""
    from gapartnet_amd import hip_ops
    three = S.all_invalid()
    three["depth"][2, 3], three["depth"][10, 20], three["depth"][15, 7] = 1.0, 1.2, 0.9
    rows, valid, vc, pix, seeds, host = _upload([three], cuda)
    hyp, hyp_pix = hip_ops.frame_plane_hypotheses(rows, hip_ops.frame_candidates(rows, valid), pix, vc, seeds, 256, 0)
    h, hp = R.hypotheses(host[0][0], R.candidates(*host[0]), host[0][1], seeds[0], 256, 0)
    assert np.array_equal(hyp[0].cpu().numpy(), h, equal_nan=True) and np.array_equal(hyp_pix[0].cpu().numpy(), hp)
    assert np.isnan(h[:, 0]).any() and np.isfinite(h[:, 0]).any(), "repeated ranks and proper triples both occur"
    # collinear points: the pixels of one image line at one depth lie on a line in space
    flat = S.all_invalid(1, 70)
    flat["depth"][:] = 1.0
    rows, valid, vc, pix, seeds, host = _upload([flat], cuda)
    hyp, _ = hip_ops.frame_plane_hypotheses(rows, hip_ops.frame_candidates(rows, valid), pix, vc, seeds, 256, 0)
    assert bool(torch.isnan(hyp).all()) and np.isnan(R.hypotheses(host[0][0], host[0][1], host[0][1], seeds[0], 256, 0)[0]).all()
    # round 1: the table is cut, what is left is a twentieth of the valid pixels - 8 tries miss now and then
    sc = S.scene("s61x97")
    rows, valid, vc, pix, seeds, host = _upload([sc], cuda)
    xyz, ok = host[0]
    c1 = R.cut(xyz, R.candidates(xyz, ok), sc["table"], TOL)
    cand = torch.from_numpy(c1.astype(np.uint8).reshape(1, 61, 97)).to(cuda)
    hyp, hyp_pix = hip_ops.frame_plane_hypotheses(rows, cand, pix, vc, seeds, 256, 1)
    h, hp = R.hypotheses(xyz, c1, ok, seeds[0], 256, 1)
    assert np.array_equal(hyp[0].cpu().numpy(), h, equal_nan=True) and np.array_equal(hyp_pix[0].cpu().numpy(), hp)
    assert np.isnan(h[:, 0]).any() and np.isfinite(h[:, 0]).any()
    assert np.array_equal(hip_ops.frame_plane_score(rows, cand, hyp, TOL)[0].cpu().numpy(), R.score(xyz, c1, h, TOL))


def test_winner_ties_go_to_the_lower_k(cuda):
    from gapartnet_amd import hip_ops
    counts = np.zeros((4, 300), dtype=np.int32)
    counts[0, [7, 250, 299]] = 41            # a three-way tie
    counts[1, 299], counts[1, 0] = 5, 4      # the last one wins outright
    counts[2, :] = 9                         # all equal
    got = hip_ops.frame_plane_winner(torch.from_numpy(counts).to(cuda)).cpu().tolist()
    assert got == [7, 299, 0, -1] == [R.winner(c) for c in counts]


@pytest.mark.parametrize("names", BATCHES[:4], ids=lambda n: "+".join(n))
def test_refit(cuda, names, capsys):
    from gapartnet_amd import hip_ops
    scenes = _names(names)
    rows, valid, vc, pix, seeds, host = _upload(scenes, cuda)
    cand = hip_ops.frame_candidates(rows, valid)
    hyp, hyp_pix = hip_ops.frame_plane_hypotheses(rows, cand, pix, vc, seeds, 256, 0)
    win = hip_ops.frame_plane_winner(hip_ops.frame_plane_score(rows, cand, hyp, TOL))
    runs = [hip_ops.frame_plane_refit(rows, cand, hyp, hyp_pix, win, TOL, 0.1, 0, 1) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.cpu(), b.cpu()), "two runs are bit-equal"
    planes, inl, n_planes = (x.cpu().numpy() for x in runs[0])
    for v, (xyz, ok) in enumerate(host):
        c = R.candidates(xyz, ok)
        h, hp = hyp[v].cpu().numpy(), hyp_pix[v].cpu().numpy()
        want, want_inl, _ = R.refit(xyz, c, h, hp, int(win[v]), TOL, 0.1)
        exact = R.refit(xyz, c, h, hp, int(win[v]), TOL, 0.1, dtype=np.longdouble)[2]
        e_ref = float(np.abs(want.astype(np.longdouble) - exact).max())
        err = float(np.abs(planes[v, 0] - want).max())
        with capsys.disabled():
            print(f"\nrefit {names[v]}: E_ref {e_ref:.3e}  kernel error {err:.3e}  bound {4 * e_ref + REFIT_ABS:.3e}")
        assert np.isfinite(want).all() and n_planes[v] == 1
        assert err <= 4 * e_ref + REFIT_ABS, (names[v], err, e_ref)
        assert inl[v, 0] == want_inl


def _after_planes(cuda, scenes, max_planes):
    """stages 1 - 4 on the device -> (rows, cand after the cuts, planes, plane_inliers, n_planes, host)"""
    from gapartnet_amd import hip_ops
    rows, valid, vc, pix, seeds, host = _upload(scenes, cuda)
    cand = hip_ops.frame_candidates(rows, valid)
    planes = inl = n_planes = None
    for r in range(max_planes):
        hyp, hyp_pix = hip_ops.frame_plane_hypotheses(rows, cand, pix, vc, seeds, 256, r)
        win = hip_ops.frame_plane_winner(hip_ops.frame_plane_score(rows, cand, hyp, TOL))
        planes, inl, n_planes = hip_ops.frame_plane_refit(rows, cand, hyp, hyp_pix, win, TOL, 0.1, r, max_planes, planes, inl, n_planes)
        hip_ops.frame_plane_cut(rows, cand, planes, TOL, r)
    return rows, cand, planes, inl, n_planes, seeds, host


@pytest.mark.parametrize("names,max_planes", [(b, 1) for b in BATCHES] + [(["s61x97", "wall"], 2)], ids=lambda n: "+".join(n) if isinstance(n, list) else str(n))
def test_cut_components_select_with_the_kernels_planes(cuda, names, max_planes):
    from gapartnet_amd import hip_ops
    scenes = _names(names)
    H, W = scenes[0]["depth"].shape
    rows, cand, planes, inl, n_planes, seeds, host = _after_planes(cuda, scenes, max_planes)
    labels, sizes, n_comp = hip_ops.frame_components(rows, cand, CFG["jump_abs"], CFG["jump_rel"], CFG["min_pixels"])
    cfg = dict(CFG, max_planes=max_planes)
    for rule in ("largest", "center", "all"):
        anchor = np.array([[W // 2, H // 2]] * len(scenes), dtype=np.int32)
        keep, chosen, status = hip_ops.frame_component_select(labels, sizes, n_planes, rule, CFG["min_pixels"], torch.from_numpy(anchor).to(cuda))
        for v, (xyz, ok) in enumerate(host):
            want = R.isolate_frame(xyz, ok, H, W, seeds[v], select_rule=rule, anchor=anchor[v], planes_in=planes[v].cpu().numpy(), **cfg)
            assert np.array_equal(cand[v].cpu().numpy().reshape(-1) != 0, want["cand"]), names[v]
            assert np.array_equal(inl[v].cpu().numpy(), want["plane_inliers"]) and int(n_planes[v]) == want["n_planes"]
            assert np.array_equal(labels[v].cpu().numpy(), want["labels"]) and np.array_equal(sizes[v].cpu().numpy(), want["sizes"])
            assert int(n_comp[v]) == want["n_components"]
            assert np.array_equal(keep[v].cpu().numpy(), want["keep"]), (names[v], rule)
            assert (int(chosen[v]), int(status[v])) == (want["chosen"], want["status"]), (names[v], rule)
    if max_planes == 2:
        assert n_planes.cpu().tolist()[1] == 2, "the wall scene accepts two planes"


# ---- components on adversarial masks -------------------------------------------------------------------------------------------------
AH, AW = 50, 70  # 4 x 5 tiles of 16, none of the sizes a multiple


def _spiral(H, W):
    """a one-pixel-wide spiral path with one-pixel gaps between its arms: one component that crosses every tile many times"""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        steps = 0
        while 0 <= y + dy < H and 0 <= x + dx < W and not m[y + dy, x + dx] and \
                not (0 <= y + 2 * dy < H and 0 <= x + 2 * dx < W and m[y + 2 * dy, x + 2 * dx]):
            y, x, steps = y + dy, x + dx, steps + 1
            m[y, x] = True
        if steps == 0:
            return m
        dy, dx = dx, -dy


def _adversarial():
    """[(name, cand [AH,AW] bool, z [AH,AW] f32)]"""
    one = np.ones((AH, AW), np.float32)
    yy, xx = np.mgrid[:AH, :AW]
    out = [("spiral", _spiral(AH, AW), one)]
    serp = np.zeros((AH, AW), bool)
    serp[::2] = True
    for i, y in enumerate(range(1, AH, 2)):
        serp[y, AW - 1 if i % 2 == 0 else 0] = True
    out.append(("serpentine", serp, one))
    out.append(("checkerboard", (yy + xx) % 2 == 0, one))
    out.append(("full", np.ones((AH, AW), bool), one))
    blobs = np.zeros((AH, AW), bool)
    blobs[10:16, 10:16] = True   # ends at the tile border 15 | 16
    blobs[12:14, 16:22] = True   # touches it only across the border: one component
    blobs[26:32, 26:32] = True   # ends at the tile corner (31, 31)
    blobs[32:38, 32:38] = True   # touches it only diagonally: two components
    out.append(("blobs", blobs, one))
    i = yy // 2  # the position along the serpentine's path: row 2i runs left to right for even i, its connector follows it
    along = np.where(yy % 2 == 0, i * (AW + 1) + np.where(i % 2 == 0, xx, AW - 1 - xx), i * (AW + 1) + AW)
    stairs = (1.0 + 0.009 * along).astype(np.float32)  # 9 mm a step: every neighbour on the path is linked
    out.append(("staircase", serp, stairs))
    ramp = (1.0 + 0.001 * xx + 0.0 * yy).astype(np.float32)
    ramp[:, 33:] += np.float32(0.0215)  # one jump just over 0.01 + 0.01 * z ~ 0.0203: two components
    out.append(("ramp", np.ones((AH, AW), bool), ramp))
    return out


def _component_inputs(frames, cuda):
    rows = np.zeros((len(frames), AH * AW, 6), np.float32)
    cand = np.zeros((len(frames), AH, AW), np.uint8)
    for v, (_, c, z) in enumerate(frames):
        rows[v, :, 2] = z.reshape(-1)
        cand[v] = c
    return torch.from_numpy(rows.reshape(-1, 6)).to(cuda), torch.from_numpy(cand).to(cuda)


def test_components_on_adversarial_masks(cuda):
    from gapartnet_amd import hip_ops
    frames = _adversarial()
    frames = frames + [frames[0], frames[4], frames[0]]  # batch independence: the same frame at several positions
    rows, cand = _component_inputs(frames, cuda)
    labels, sizes, n_comp = hip_ops.frame_components(rows, cand, 0.01, 0.01, 6)
    labels, sizes, n_comp = labels.cpu().numpy(), sizes.cpu().numpy(), n_comp.cpu().numpy()
    seen = {}
    for v, (name, c, z) in enumerate(frames):
        want_l, want_s, want_n = R.components(z.reshape(-1), c.reshape(-1), AH, AW, 0.01, 0.01, 6)
        assert np.array_equal(labels[v].reshape(-1), want_l), name
        assert np.array_equal(sizes[v], want_s) and n_comp[v] == want_n, name
        seen.setdefault(name, []).append(int(np.count_nonzero(want_s)))
    assert seen["full"] == [1] and seen["checkerboard"] == [AH * AW // 2] and seen["spiral"] == [1, 1, 1]
    assert seen["serpentine"] == [1] and seen["staircase"] == [1] and seen["ramp"] == [2] and seen["blobs"][0] == 3
    for v in (len(frames) - 3, len(frames) - 1):
        assert np.array_equal(labels[v], labels[0])
    assert np.array_equal(labels[len(frames) - 2], labels[4])


def test_staircase_ends_differ_by_metres():
    z = _adversarial()[5][2]
    assert float(z.max() - z.min()) > 10.0


def test_select_rules(cuda):
    from gapartnet_amd import hip_ops
    c = np.zeros((AH, AW), bool)
    c[2:6, 2:7] = True      # 20 pixels, root (2, 2)
    c[20:24, 40:45] = True  # 20 pixels, root (20, 40): a tie in size - the smaller root wins
    c[40:42, 60:62] = True  # 4 pixels: below min_pixels
    crumbs = np.zeros((AH, AW), bool)
    crumbs[::3, ::3] = True
    frames = [("two", c, np.ones((AH, AW), np.float32)), ("crumbs", crumbs, np.ones((AH, AW), np.float32))]
    rows, cand = _component_inputs(frames, cuda)
    labels, sizes, _ = hip_ops.frame_components(rows, cand, 0.01, 0.01, 6)
    n_planes = torch.tensor([1, 0], dtype=torch.int32, device=cuda)
    ref = [R.components(z.reshape(-1), m.reshape(-1), AH, AW, 0.01, 0.01, 6) for _, m, z in frames]
    cases = [("largest", None), ("all", None), ("center", (42, 21)), ("center", (61, 41)), ("center", (30, 12)), ("center", (-5000, -7)),
             ("center", (10 ** 6, 10 ** 6)), ("center", (0, 0))]
    for rule, anchor in cases:
        a = None if anchor is None else torch.tensor([anchor, anchor], dtype=torch.int64).clamp(-2 ** 31, 2 ** 31 - 1).int().to(cuda)
        keep, chosen, status = hip_ops.frame_component_select(labels, sizes, n_planes, rule, 6, a)
        for v in range(2):
            wk, wc, ws = R.select(ref[v][0], ref[v][1], int(n_planes[v]), AH, AW, rule, 6, anchor)
            assert np.array_equal(keep[v].cpu().numpy().reshape(-1), wk), (rule, anchor, v)
            assert (int(chosen[v]), int(status[v])) == (wc, ws), (rule, anchor, v)
    keep, chosen, status = hip_ops.frame_component_select(labels, sizes, n_planes, "largest", 6)
    assert chosen.cpu().tolist() == [2 * AW + 2, -1] and status.cpu().tolist() == [R.OK, R.EMPTY] and not bool(keep[1].any())
    keep, chosen, status = hip_ops.frame_component_select(labels, sizes, n_planes, "center", 6, torch.tensor([[61, 41]] * 2, dtype=torch.int32, device=cuda))
    assert int(chosen[0]) == 20 * AW + 40, "the anchor sits on a component below min_pixels: the nearest qualifying one is taken"
    keep, chosen, status = hip_ops.frame_component_select(labels, sizes, n_planes, "largest", 1)
    assert status.cpu().tolist() == [R.OK, R.NO_PLANE]


@pytest.mark.parametrize("names,max_planes", [(b, 1) for b in BATCHES] + [(["s61x97", "wall"], 2)], ids=lambda n: "+".join(n) if isinstance(n, list) else str(n))
def test_frame_isolate_end_to_end(cuda, names, max_planes):
    """the chained call equals the reference pipeline (its own float64 refit, not the kernel's): the scenes keep every pixel 1e-9
    clear of tol (tests/test_isolate_cpu.py), and the two refits differ by 1e-15"""
    from gapartnet_amd import hip_ops
    scenes = _names(names)
    H, W = scenes[0]["depth"].shape
    rows, valid, vc, pix, seeds, host = _upload(scenes, cuda)
    cfg = dict(CFG, max_planes=max_planes)
    got = hip_ops.frame_isolate(rows, valid, vc, seeds, **cfg)
    again = hip_ops.frame_isolate(rows, valid, vc, seeds, **cfg)
    for f in ("keep", "labels", "sizes", "planes", "plane_inliers", "n_planes", "chosen", "status"):
        assert torch.equal(torch.nan_to_num(got[f].double(), nan=-7.0), torch.nan_to_num(again[f].double(), nan=-7.0)), f
    for v, (xyz, ok) in enumerate(host):
        want = R.isolate_frame(xyz, ok, H, W, seeds[v], **cfg)
        assert np.array_equal(got["keep"][v].cpu().numpy(), want["keep"]), names[v]
        assert np.array_equal(got["labels"][v].cpu().numpy(), want["labels"]) and np.array_equal(got["plane_inliers"][v].cpu().numpy(), want["plane_inliers"])
        assert (int(got["chosen"][v]), int(got["status"][v]), int(got["n_planes"][v])) == (want["chosen"], want["status"], want["n_planes"])
        assert np.allclose(got["planes"][v].cpu().numpy(), want["planes"], rtol=0, atol=REFIT_ABS * 10, equal_nan=True)


def test_frame_isolate_on_frames_with_nothing_in_them(cuda):
    from gapartnet_amd import hip_ops
    cfg = dict(CFG, min_plane_fraction=0.5)  # (a cap of the lone sphere within tol of a plane holds a tenth of its pixels)
    for sc, status in ((S.all_invalid(), R.EMPTY), (S.two_valid(), R.EMPTY), (S.no_plane(), R.NO_PLANE)):
        H, W = sc["depth"].shape
        rows, valid, vc, pix, seeds, host = _upload([sc], cuda)
        got = hip_ops.frame_isolate(rows, valid, vc, seeds, **cfg)
        want = R.isolate_frame(host[0][0], host[0][1], H, W, seeds[0], **cfg)
        assert np.array_equal(got["keep"][0].cpu().numpy(), want["keep"]) and int(got["status"][0]) == want["status"] == status
        assert int(got["n_planes"][0]) == want["n_planes"] == 0 and bool(torch.isnan(got["planes"][0]).all())


def test_batch_of_three_with_distinct_seeds(cuda):
    """one frame three times with three seeds: every frame as if alone with its seed"""
    from gapartnet_amd import hip_ops
    sc = S.scene("s61x97")
    seeds = [2, 77, 0xfffffffe]
    rows, valid, vc, pix, _, host = _upload([sc] * 3, cuda, seeds)
    got = hip_ops.frame_isolate(rows, valid, vc, seeds, **CFG)
    for v in range(3):
        r1, v1, c1, _, _, _ = _upload([sc], cuda, [seeds[v]])
        alone = hip_ops.frame_isolate(r1, v1, c1, [seeds[v]], **CFG)
        for f in ("keep", "labels", "planes", "plane_inliers", "chosen", "status"):
            assert torch.equal(got[f][v], alone[f][0]), (v, f)
    assert not torch.equal(got["planes"][0], got["planes"][1]), "another seed draws other triples"


def test_argument_errors(cuda):
    """argument errors return an error code without a launch"""
    from gapartnet_amd import _C, hip_ops
    sc = S.scene("tile-1")
    rows, valid, vc, pix, seeds, _ = _upload([sc], cuda)
    cand = hip_ops.frame_candidates(rows, valid)
    hyp, hyp_pix = hip_ops.frame_plane_hypotheses(rows, cand, pix, vc, seeds, 16, 0)
    counts = hip_ops.frame_plane_score(rows, cand, hyp, TOL)
    win = hip_ops.frame_plane_winner(counts)
    planes, inl, n_planes = hip_ops.frame_plane_refit(rows, cand, hyp, hyp_pix, win, TOL)
    labels, sizes, _ = hip_ops.frame_components(rows, cand)
    bad = [lambda: hip_ops.frame_candidates(rows, valid, z_min=-1.0),
           lambda: hip_ops.frame_candidates(rows, valid, z_min=2.0, z_max=1.0),
           lambda: hip_ops.frame_plane_hypotheses(rows, cand, pix, vc, seeds, 0, 0),
           lambda: hip_ops.frame_plane_hypotheses(rows, cand, pix, vc, seeds, 1025, 0),
           lambda: hip_ops.frame_plane_hypotheses(rows, cand, pix, vc, seeds, 16, 4),
           lambda: hip_ops.frame_plane_score(rows, cand, hyp, -1.0),
           lambda: hip_ops.frame_plane_score(rows, cand, hyp, float("nan")),
           lambda: hip_ops.frame_plane_score(rows, cand, hyp, TOL, variant=2),
           lambda: hip_ops.frame_plane_refit(rows, cand, hyp, hyp_pix, win, TOL, min_plane_fraction=1.5),
           lambda: hip_ops.frame_plane_refit(rows, cand, hyp, hyp_pix, win, TOL, round=1, max_planes=1),
           lambda: hip_ops.frame_plane_refit(rows, cand, hyp, hyp_pix, win, TOL, max_planes=5),
           lambda: hip_ops.frame_plane_cut(rows, cand, planes, TOL, round=1),
           lambda: hip_ops.frame_components(rows, cand, jump_abs=-0.1),
           lambda: hip_ops.frame_components(rows, cand, min_pixels=0),
           lambda: hip_ops.frame_component_select(labels, sizes, n_planes, "center", 6, None),
           lambda: hip_ops.frame_component_select(labels, sizes, n_planes, "largest", 0)]
    before = cand.clone()
    for fn in bad:
        with pytest.raises(_C.GpnError):
            fn()
    with pytest.raises(ValueError):
        hip_ops.frame_component_select(labels, sizes, n_planes, "nearest")
    assert torch.equal(cand, before)
    L = _C.lib()
    assert L.gpn_frame_plane_refit_ws_bytes(0, 4, 4) == 0 and L.gpn_frame_component_select_ws_bytes(0) == 0
