"""Test-time rendering without a GPU: the numpy restatement (tests/visu_ref.py) against what the reference's visualize_gapartnet
produced (tests/golden/visu_panels.npz: tile arrays, the canvas, the recorded cv2.line calls and RANSAC draws), the line rule on
hand-made segments, the argument checks and exports of the new entry points, and the untouched visualize=False path."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import visu_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = ("gpn_scene_maps_ws_bytes", "gpn_scene_maps", "gpn_points_winner", "gpn_points_paint", "gpn_boxes_draw_ws_bytes",
           "gpn_boxes_draw")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "visu_panels.npz"))


fixture_scene, fixture_geometry = R.golden_scene, R.golden_geometry


@pytest.fixture(scope="module")
def restated(gold):
    """the restatement's tiles of both fixture scenes, computed once"""
    H, W, _ = fixture_geometry(gold)
    return [R.render_tiles(fixture_scene(gold, s), gold["COLOR20"], H, W) for s in range(2)]


def line_mask(scene, which, H, W):
    white = np.full((H, W, 3), 255, np.uint8)
    return (R.draw_boxes(white.copy(), scene[which], scene["trans"]) != white).any(-1)


def test_fixture_constants_are_the_defaults(gold):
    from gapartnet_amd.misc import visu
    assert fixture_geometry(gold) == (visu.HEIGHT, visu.WIDTH, visu.EDGE)
    K = gold["K"]
    assert (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) == (visu.FX, visu.FY, visu.U0, visu.V0) == R.CAM
    assert list(gold["options"]) == list(visu.OPTIONS) and visu.TILE_POS == R.TILE_POS
    pal = visu.default_palette()
    assert pal.shape == (21, 3) and pal.dtype == np.uint8 and tuple(pal[0]) == (230, 230, 230)
    assert len({tuple(c) for c in pal}) == 21, "21 distinct colours"
    assert not np.array_equal(pal, gold["COLOR20"]), "a table of our own"


def test_fixture_scenes_hold_every_edge_case(gold):
    """the cases the contract names are present in the scenes, so the bit-equality below exercises them"""
    H, W, _ = fixture_geometry(gold)
    sc = fixture_scene(gold, 0)
    with np.errstate(all="ignore"):
        c = sc["xyz"].astype(np.float64) * sc["trans"][0] + sc["trans"][1:4]
        fu = c[:, 0] * R.FX / c[:, 2] + R.U0
        fv = c[:, 1] * R.FY / c[:, 2] + R.V0
    u, v = R.project(sc["xyz"], sc["trans"])
    assert ((fu == 410.5) & (u == 410)).any() and ((fu == 411.5) & (u == 412)).any(), "half to even, both ways"
    assert ((fv == 250.5) & (v == 250)).any() and ((fv == 251.5) & (v == 252)).any()
    assert ((fu < 0) & (fu > -0.01) & (u == 0) & np.signbit(u)).any(), "-0.0015 rounds to -0"
    assert ((fv < 0) & (fv > -0.01) & (v == 0) & np.signbit(v)).any()
    assert (u == W - 2).any() and (u == W - 1).any() and (v == H - 2).any() and (v == H - 1).any()
    assert (c[:, 2] == 0).any() and (c[:, 2] < 0).any() and np.isnan(u).any() and np.isinf(u).any()
    pix = np.stack([u, v], 1)[np.isfinite(u) & np.isfinite(v)]
    assert np.unique(pix, axis=0).shape[0] < pix.shape[0], "two points on one pixel"
    assert (sc["ins_gt"] == -100).any() and (sc["ins_gt"] >= 20).any() and (sc["ins_pred"] >= 20).any() and (sc["sem_gt"] == 20).any()
    for k, off in (("rgb", 0.0), ("npcs_pred", 0.0), ("npcs_gt", 0.5)):
        f = (sc[k] + np.float32(off)) * np.float32(255.0)
        assert f.min() >= 0 and f.max() <= 255.99 and (f != np.trunc(f)).any(), k
    # the winner of the pixel two points share is the higher index, and a -0 column is painted
    win = R.points_winner(sc["xyz"], sc["trans"], H, W)
    both = np.nonzero((u == 100) & (v == 100))[0]
    assert both.shape[0] == 2 and win[100, 100] == both.max()
    assert (win[:, 0] >= 0).any() and (win[0, :] >= 0).any() and (win[:, W - 1] >= 0).any() and (win[H - 1, :] >= 0).any()


@pytest.mark.parametrize("s", [0, 1])
def test_restatement_equals_the_reference_tiles(gold, restated, s):
    """bit-equal to every tile the reference wrote; on the four box tiles outside the restatement's line pixels (the reference's
    recorded tiles carry no lines: cv2.line is recorded, not drawn)"""
    H, W, _ = fixture_geometry(gold)
    scene, tiles = fixture_scene(gold, s), restated[s]
    assert set(tiles) == set(R.TILE_POS)
    for name, img in tiles.items():
        want = gold[f"s{s}_tile_{name}"]
        if name.startswith("bbox"):
            mask = line_mask(scene, "bbox_pred" if "pred" in name else "bbox_gt", H, W)
            assert mask.any() and not mask.all()
            assert np.array_equal(img[~mask], want[~mask]), name
        else:
            assert np.array_equal(img, want), name


@pytest.mark.parametrize("s", [0, 1])
def test_restatement_equals_the_reference_canvas(gold, restated, s):
    H, W, EDGE = fixture_geometry(gold)
    want = gold[f"s{s}_canvas"]
    assert want.shape[:2] == R.canvas_shape(H, W, EDGE)
    scene = fixture_scene(gold, s)
    got = R.assemble(restated[s], H, W, EDGE)
    mask = np.zeros(want.shape[:2], bool)
    for name in ("bbox_pred", "bbox_pred_pure", "bbox_gt", "bbox_gt_pure"):
        y0, x0 = R.tile_origin(name, H, W, EDGE)
        mask[y0:y0 + H, x0:x0 + W] = line_mask(scene, "bbox_pred" if "pred" in name else "bbox_gt", H, W)
    assert np.array_equal(got[~mask], want[~mask])
    # the captions sit at the anchors the reference computes, one per option
    anchors = {str(t): tuple(a) for t, a in zip(gold[f"s{s}_texts"], gold[f"s{s}_text_anchor"])}
    for name in R.TILE_POS:
        y0, x0 = R.tile_origin(name, H, W, EDGE)
        assert anchors[name] == (x0 + int(0.5 * (W - 3 * EDGE)), y0 + H + int(0.5 * EDGE))


@pytest.mark.parametrize("s", [0, 1])
def test_projected_corners_equal_the_recorded_line_calls(gold, s):
    """corner projection, which boxes are drawn, edge order, colours and thickness: the recorded cv2.line calls, exactly"""
    scene = fixture_scene(gold, s)
    options = list(gold["options"])
    lines = gold[f"s{s}_lines"]
    valid, boxes = gold[f"s{s}_fit_valid"], gold[f"s{s}_fit_bbox"]
    half = valid.shape[0] // 2
    assert list(gold[f"s{s}_fit_sizes"][:half]) == [180, 150], "instances with more than 5 points, in ascending id"
    per_tile = {"bbox_pred": scene["bbox_pred"], "bbox_pred_pure": scene["bbox_pred"], "bbox_gt": boxes[:half][valid[:half]],
                "bbox_gt_pure": boxes[half:][valid[half:]]}
    seen = 0
    for name, bb in per_tile.items():
        rec = lines[lines[:, 0] == options.index(name)]
        corners = R.box_corners(bb, scene["trans"])
        assert np.isfinite(corners).all()
        want = [(int(c[a][0]), int(c[a][1]), int(c[b][0]), int(c[b][1])) + colour + (t,) for c in corners
                for a, b, colour, t in R.BOX_DRAWS]
        assert [tuple(int(v) for v in r[1:]) for r in rec] == want, name
        seen += rec.shape[0]
    assert seen == lines.shape[0] > 0


def _drawn(a, b, t, H=12, W=16):
    img = np.zeros((H, W, 3), np.uint8)
    R.draw_line(img, a, b, (1, 2, 3), t)
    ys, xs = np.nonzero(img.any(-1))
    return sorted(zip(xs.tolist(), ys.tolist()))


def test_line_rule_on_hand_made_segments():
    assert _drawn((2, 3), (6, 3), 1) == [(x, 3) for x in range(2, 7)]                                   # horizontal
    assert _drawn((4, 1), (4, 5), 1) == [(4, y) for y in range(1, 6)]                                   # vertical
    assert _drawn((1, 1), (3, 7), 1) == [(1, 1), (1, 2), (2, 3), (2, 4), (2, 5), (3, 6), (3, 7)]         # steep
    assert _drawn((0, 0), (5, 2), 1) == sorted([(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)])
    assert _drawn((3, 7), (1, 1), 1) == sorted([(3, 7), (3, 6), (2, 5), (2, 4), (2, 3), (1, 2), (1, 1)])  # reversed: its own walk
    assert _drawn((5, 5), (5, 5), 2) == [(4, 4), (4, 5), (5, 4), (5, 5)]                                 # t = 2: top-left (x-1, y-1)
    assert _drawn((5, 5), (5, 5), 3) == sorted((x, y) for x in (4, 5, 6) for y in (4, 5, 6))             # t = 3: centred
    assert _drawn((13, 4), (20, 4), 1) == [(13, 4), (14, 4), (15, 4)]                                    # crossing the border
    assert _drawn((-3, -3), (2, 2), 2) == sorted({(x, y) for k in range(0, 3) for x in (k - 1, k) for y in (k - 1, k)
                                                   if x >= 0 and y >= 0})
    assert _drawn((0, 0), (5 * 16, 3), 1) == [] and _drawn((0, -4 * 12 - 1), (3, 3), 1) == []            # outside the bound: skipped
    assert _drawn((0, 0), (5 * 16 - 1, 0), 1) == [(x, 0) for x in range(16)]                             # just inside: walked
    assert _drawn((np.nan, 0), (3, 3), 1) == [] and _drawn((0, 0), (np.inf, 3), 1) == []                 # non-finite: skipped


def test_scene_maps_restatement_last_writer_wins():
    # rows 0..5; valid rows 1,2,3,5; proposals {1,2} and {2,3}: row 2 is shared, the second proposal wins both maps
    vi, si, po = [1, 2, 3, 5], [0, 1, 1, 2], [0, 2, 4]
    preds = np.arange(9, dtype=np.float32).reshape(3, 3) / 10
    ins, npcs, fit = R.scene_maps(vi, si, po, [True, True, True, False], preds, 6)
    assert ins.tolist() == [0, 1, 2, 2, 0, 0]
    assert np.array_equal(npcs[2], preds[2]) and np.array_equal(npcs[1], preds[0]) and not npcs[3].any()
    assert np.array_equal(fit[1], preds[2] - np.float32(0.5)) and np.array_equal(fit[3], np.full(3, -0.5, np.float32))


# ---------------------------------------------------------------------------------------------------- library boundary
@pytest.fixture(scope="module")
def lib():
    from gapartnet_amd import _C
    if not os.path.exists(_C.SO_PATH):
        _C.build()
    return _C.lib()


def test_library_exports_and_registers_the_new_symbols(lib):
    names = {lib.gpn_entry_point_name(i).decode() for i in range(lib.gpn_num_entry_points())}
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in names, s
    assert lib.gpn_scene_maps_ws_bytes(ctypes.c_int64(1000), ctypes.c_int64(500)) >= 2 * 4000 + 2000
    assert lib.gpn_boxes_draw_ws_bytes(ctypes.c_int(2), ctypes.c_int(48), ctypes.c_int(64)) >= 2 * 48 * 64 * 4
    assert lib.gpn_boxes_draw_ws_bytes(ctypes.c_int(0), ctypes.c_int(48), ctypes.c_int(64)) == 0


def test_argument_errors_do_not_touch_the_device(lib):
    from gapartnet_amd.hip_ops import _VisuLayer
    i, l, d, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    st = ctypes.c_size_t
    cam = (d(100.0), d(100.0), d(32.0), d(24.0))
    p = vp(16)   # a non-null pointer that is never dereferenced: every call below fails its checks first
    assert lib.gpn_scene_maps(None, l(4), None, None, l(1), None, l(4), None, l(2), l(8), None, None, None, None, st(0), None) == 1
    assert b"bad argument" in lib.gpn_last_error()
    assert lib.gpn_scene_maps(p, l(4), p, p, l(1), p, l(4), p, l(5), l(8), p, p, p, p, st(1 << 20), None) == 1      # Mv > M
    assert lib.gpn_scene_maps(p, l(4), p, p, l(1), p, l(4), p, l(2), l(-1), p, p, p, p, st(1 << 20), None) == 1     # N < 0
    assert lib.gpn_scene_maps(p, l(4), p, p, l(1), p, l(4), p, l(2), l(8), p, p, p, p, st(16), None) != 0           # workspace
    assert lib.gpn_scene_maps(None, l(0), None, None, l(0), None, l(0), None, l(0), l(0), None, None, None, None, st(0), None) == 0
    assert lib.gpn_points_winner(None, None, l(10), None, i(1), i(48), i(64), *cam, None, None) == 1
    assert lib.gpn_points_winner(p, p, l(10), p, i(1), i(1), i(64), *cam, p, None) == 1                            # H < 2
    assert lib.gpn_points_winner(p, p, l(-1), p, i(1), i(48), i(64), *cam, p, None) == 1
    assert lib.gpn_points_winner(None, None, l(0), None, i(0), i(48), i(64), *cam, None, None) == 0                # no scene
    layer = (_VisuLayer * 1)(_VisuLayer(0, 0, 0, 0.0, 16))
    ok = (i(1), i(48), i(64), layer, i(1), p, i(21), i(4), i(3 * 52 + 4), i(4 * 68 + 4), p, None)
    assert lib.gpn_points_paint(None, p, *ok) == 1                                                                  # no winner
    bad = (_VisuLayer * 1)(_VisuLayer(9, 0, 0, 0.0, 16))
    assert lib.gpn_points_paint(p, p, i(1), i(48), i(64), bad, i(1), p, i(21), i(4), i(160), i(276), p, None) == 1  # kind
    far = (_VisuLayer * 1)(_VisuLayer(0, 3, 0, 0.0, 16))
    assert lib.gpn_points_paint(p, p, i(1), i(48), i(64), far, i(1), p, i(21), i(4), i(160), i(276), p, None) == 1  # tile outside
    mod = (_VisuLayer * 1)(_VisuLayer(2, 0, 0, 0.0, 16))
    assert lib.gpn_points_paint(p, p, i(1), i(48), i(64), mod, i(1), p, i(19), i(4), i(160), i(276), p, None) == 1  # palette < 20
    assert lib.gpn_points_paint(p, p, i(1), i(48), i(64), layer, i(17), p, i(21), i(4), i(160), i(276), p, None) == 1
    tiles = (ctypes.c_int32 * 2)(2, 2)
    assert lib.gpn_boxes_draw(None, None, l(3), None, i(1), i(48), i(64), *cam, tiles, i(1), i(4), i(160), i(276), None, None, st(0),
                              None) == 1
    assert lib.gpn_boxes_draw(p, p, l(-1), p, i(1), i(48), i(64), *cam, tiles, i(1), i(4), i(160), i(276), p, p, st(1 << 20), None) == 1
    out = (ctypes.c_int32 * 2)(3, 0)
    assert lib.gpn_boxes_draw(p, p, l(3), p, i(1), i(48), i(64), *cam, out, i(1), i(4), i(160), i(276), p, p, st(1 << 20), None) == 1
    assert lib.gpn_boxes_draw(p, p, l(3), p, i(1), i(48), i(64), *cam, tiles, i(1), i(4), i(160), i(276), p, p, st(16), None) != 0
    assert lib.gpn_boxes_draw(None, None, l(0), None, i(1), i(48), i(64), *cam, tiles, i(1), i(4), i(160), i(276), None, None, st(0),
                              None) == 0                                                                            # no box


def test_wrappers_refuse_cpu_tensors():
    from gapartnet_amd import _C, hip_ops
    with pytest.raises(_C.GpnError):
        hip_ops.points_winner(torch.zeros(4, 3), torch.tensor([0, 4]), torch.zeros(1, 4, dtype=torch.float64), 48, 64, 1., 1., 0., 0.)
    with pytest.raises(_C.GpnError):
        hip_ops.scene_maps(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.tensor([0, 2]),
                           torch.ones(2, dtype=torch.bool), torch.zeros(2, 3), 4)


def test_test_epoch_end_without_visualize_logs_what_validation_logs():
    """visualize=False: on_test_epoch_end is the metrics pass alone, as before"""
    from gapartnet_amd.smoke import make_model
    from gapartnet_amd.structure.segmentation import Segmentation
    model = make_model((0, 0)).eval()
    assert model.visualize_cfg.get("visualize", False) is False
    g = torch.Generator().manual_seed(0)

    def outputs():
        out = []
        for _ in range(3):
            pred, lab = torch.randint(0, 10, (2 * 50,), generator=g), torch.randint(0, 10, (2 * 50,), generator=g)
            out.append([(["a", "b"], Segmentation(batch_size=2, sem_preds=pred, sem_labels=lab, all_accu=torch.tensor(0.5),
                                                  pixel_accu=0.25), None)])
        return out
    recs = []
    for end in ("on_validation_epoch_end", "on_test_epoch_end"):
        g.manual_seed(0)
        rec = {}
        model._log_sink = lambda name, value, bs, sync, rec=rec: rec.__setitem__(name, float(value))
        model.validation_step_outputs = outputs()
        getattr(model, end)()
        recs.append(rec)
        assert model._visualize_outputs == [] and model.validation_step_outputs == []
    assert recs[0] == recs[1] and "monitor_metrics/mean_mAP" in recs[0] and "val/miou" in recs[0]
