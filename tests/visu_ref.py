"""numpy restatement of the four contracts of include/gpn.h section VS (scene maps, points -> pixels, tile colours, boxes), the
oracle of tests/test_visu_cpu.py and tests/test_gpu_visu.py.  It is checked itself against tests/golden/visu_panels.npz, what the
reference's visualize_gapartnet produced (tests/golden/make_golden_visu.py).  Every "last writer wins" of the reference's loops is
a maximum over the writer's position here too, so nothing depends on an evaluation order."""
import numpy as np

FX = FY = 1268.637939453125   # the dataset's render settings (misc/visu_util.py:14)
U0 = V0 = 400.0
CAM = (FX, FY, U0, V0)
# (row, col) of every option in the 3 x 4 panel (misc/visu.py:55-260)
TILE_POS = {"raw": (0, 0), "sem_gt": (0, 1), "ins_gt": (0, 2), "npcs_gt": (0, 3),
            "pc": (1, 0), "sem_pred": (1, 1), "ins_pred": (1, 2), "npcs_pred": (1, 3),
            "bbox_gt_pure": (2, 0), "bbox_gt": (2, 1), "bbox_pred": (2, 2), "bbox_pred_pure": (2, 3)}
# draw_bbox (misc/visu_util.py:56-70): (corner a, corner b, colour in the written file, thickness)
BOX_DRAWS = [(a, b, (255, 0, 255), 2) for a, b in ((0, 1), (0, 2), (0, 3), (1, 4), (1, 5), (2, 6), (6, 3), (4, 7), (5, 7), (3, 5),
                                                    (2, 4), (6, 7))] + \
            [(0, 1, (255, 0, 0), 3), (0, 3, (0, 0, 255), 3), (0, 2, (0, 255, 0), 3)]


# ---------------------------------------------------------------------------------------------------- scene maps
def scene_maps(valid_indices, sorted_indices, proposal_offsets, npcs_valid_mask, npcs_preds, n_rows):
    """model.py:954-971 on host arrays -> (ins_map [N] i32, npcs_map [N,3] f32, fit_npcs [M,3] f32).  The reference's loops and
    index assignments run in ascending m (numpy: the last value assigned to a repeated index stays)."""
    vi, si, po = (np.asarray(a, dtype=np.int64) for a in (valid_indices, sorted_indices, proposal_offsets))
    mask = np.asarray(npcs_valid_mask, dtype=bool)
    rows = vi[si] if si.size else np.zeros(0, np.int64)
    ins_map = np.zeros(n_rows, np.int32)
    for p in range(max(po.shape[0] - 1, 0)):
        ins_map[rows[po[p]:po[p + 1]]] = p + 1
    npcs_map = np.zeros((n_rows, 3), np.float32)
    for m, j in zip(np.nonzero(mask)[0], range(int(mask.sum()))):
        npcs_map[rows[m]] = npcs_preds[j]
    fit = npcs_map[rows] - np.float32(0.5) if si.size else np.zeros((0, 3), np.float32)
    return ins_map, npcs_map, fit.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- projection
def project(points, trans, cam=CAM):
    """points [...,3] in the normalised frame, trans (r, cx, cy, cz) -> (u, v) float64, rounded half to even, possibly non-finite"""
    fx, fy, u0, v0 = cam
    trans = np.asarray(trans, dtype=np.float64)
    c = np.asarray(points).astype(np.float64) * trans[0] + trans[1:4]
    with np.errstate(all="ignore"):
        u = np.around(c[..., 0] * fx / c[..., 2] + u0)
        v = np.around(c[..., 1] * fy / c[..., 2] + v0)
    return u, v


def points_winner(xyz, trans, H, W, cam=CAM):
    """[H,W] i32: the highest point index covering each pixel (2 x 2 splats), -1 where none"""
    u, v = project(np.asarray(xyz, dtype=np.float32), trans, cam)
    with np.errstate(all="ignore"):
        keep = np.isfinite(u) & np.isfinite(v) & ~(v + 1 >= H) & ~(v < 0) & ~(u + 1 >= W) & ~(u < 0)
    idx = np.nonzero(keep)[0].astype(np.int32)
    iu, iv = u[keep].astype(np.int64), v[keep].astype(np.int64)
    winner = np.full((H, W), -1, np.int32)
    for dy, dx in ((0, 0), (1, 0), (1, 1), (0, 1)):
        np.maximum.at(winner, (iv + dy, iu + dx), idx)
    return winner


# ---------------------------------------------------------------------------------------------------- colours
def to_u8(f):
    """the C cast float32 -> uint8 where it is defined; clamped to [0, 255] outside, NaN -> 0"""
    f = np.asarray(f, dtype=np.float32)
    with np.errstate(all="ignore"):
        g = np.where(f > 0, np.minimum(f, np.float32(255.0)), np.float32(0.0))   # (NaN > 0 is False)
    return np.trunc(g).astype(np.uint8)


def colours_rgb(src, offset=0.0):
    return to_u8((np.asarray(src, dtype=np.float32) + np.float32(offset)) * np.float32(255.0))


def colours_label(labels, palette, rule="label"):
    labels = np.asarray(labels).astype(np.int64)
    palette = np.asarray(palette, dtype=np.uint8)
    if rule == "label":
        return palette[np.mod(labels, palette.shape[0])]
    if rule == "mod20":
        return palette[np.mod(labels, 20)]
    out = palette[np.mod(labels, 19) + 1].copy()
    out[labels == -100] = 230
    return out


def paint(winner, colours):
    out = np.full(winner.shape + (3,), 255, np.uint8)
    m = winner >= 0
    out[m] = colours[winner[m]]
    return out


# ---------------------------------------------------------------------------------------------------- lines
def draw_line(img, a, b, colour, t):
    """the line rule of include/gpn.h: integer Bresenham from a to b inclusive, t x t stamps with top-left (x - t//2, y - t//2),
    pixels outside the tile dropped; skipped if an endpoint is non-finite or outside [-4W, 5W) x [-4H, 5H)"""
    H, W = img.shape[:2]
    pts = np.array([a[0], a[1], b[0], b[1]], dtype=np.float64)
    if not np.isfinite(pts).all():
        return
    if not all(-4 * W <= x < 5 * W for x in pts[0::2]) or not all(-4 * H <= y < 5 * H for y in pts[1::2]):
        return
    x, y, x1, y1 = (int(p) for p in pts)
    dx, dy = abs(x1 - x), -abs(y1 - y)
    sx, sy = (1 if x < x1 else -1), (1 if y < y1 else -1)
    err = dx + dy
    while True:
        tx, ty = x - t // 2, y - t // 2
        img[max(ty, 0):max(min(ty + t, H), 0), max(tx, 0):max(min(tx + t, W), 0)] = colour
        if x == x1 and y == y1:
            return
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy


def box_corners(bboxes, trans, cam=CAM):
    """[Q,8,2] float64 (u, v) of the corners of bboxes [Q,8,3] (normalised frame)"""
    u, v = project(np.asarray(bboxes, dtype=np.float64).reshape(-1, 8, 3), trans, cam)
    return np.stack([u, v], axis=-1)


def draw_boxes(img, bboxes, trans, cam=CAM):
    """box by box, draw by draw, each over the last"""
    for corners in box_corners(bboxes, trans, cam):
        for a, b, colour, t in BOX_DRAWS:
            draw_line(img, corners[a], corners[b], colour, t)
    return img


# ---------------------------------------------------------------------------------------------------- panel
def canvas_shape(H, W, edge):
    return 3 * (H + edge) + edge, 4 * (W + edge) + edge


def tile_origin(name, H, W, edge):
    r, c = TILE_POS[name]
    return edge + r * (H + edge), edge + c * (W + edge)


def render_tiles(scene, palette, H, W, cam=CAM, options=tuple(TILE_POS)):
    """scene: dict with xyz [n,3] f32, rgb [n,3] f32, trans [4], and - as far as the options need them - sem_gt, ins_gt, npcs_gt,
    sem_pred, ins_pred, npcs_pred, bbox_pred [Q,8,3], bbox_gt [G,8,3], raw [H,W,3] u8 -> {option: [H,W,3] u8}"""
    winner = points_winner(scene["xyz"], scene["trans"], H, W, cam)
    pc = paint(winner, colours_rgb(scene["rgb"]))
    white = np.full((H, W, 3), 255, np.uint8)
    tiles = {}
    for name in options:
        if name == "raw":
            if scene.get("raw") is not None:
                tiles[name] = scene["raw"]
        elif name == "pc":
            tiles[name] = pc
        elif name == "sem_pred":
            tiles[name] = paint(winner, colours_label(scene["sem_pred"], palette))
        elif name == "ins_pred":
            tiles[name] = paint(winner, colours_label(scene["ins_pred"], palette, "mod20"))
        elif name == "npcs_pred":
            tiles[name] = paint(winner, colours_rgb(scene["npcs_pred"]))
        elif name == "sem_gt":
            tiles[name] = paint(winner, colours_label(scene["sem_gt"], palette))
        elif name == "ins_gt":
            tiles[name] = paint(winner, colours_label(scene["ins_gt"], palette, "mod19p1"))
        elif name == "npcs_gt":
            tiles[name] = paint(winner, colours_rgb(scene["npcs_gt"], 0.5))
        elif name in ("bbox_pred", "bbox_gt"):
            tiles[name] = draw_boxes(pc.copy(), scene[name], scene["trans"], cam)
        else:
            tiles[name] = draw_boxes(white.copy(), scene[name[:-5]], scene["trans"], cam)
    return tiles


def assemble(tiles, H, W, edge):
    ch, cw = canvas_shape(H, W, edge)
    canvas = np.full((ch, cw, 3), 255, np.uint8)
    for name, img in tiles.items():
        y0, x0 = tile_origin(name, H, W, edge)
        canvas[y0:y0 + H, x0:x0 + W] = img
    return canvas


# ---------------------------------------------------------------------------------------------------- the fixture
def golden_scene(gold, s):
    """scene s of tests/golden/visu_panels.npz as ``render_tiles`` takes it"""
    keys = ("xyz", "rgb", "sem_gt", "ins_gt", "npcs_gt", "sem_pred", "ins_pred", "npcs_pred", "bbox_pred", "trans", "raw")
    scene = {k: gold[f"s{s}_{k}"] for k in keys}
    # the GT tiles' boxes as the reference fitted them for its bbox_gt tile (the first half of the recorded fits)
    valid, boxes = gold[f"s{s}_fit_valid"], gold[f"s{s}_fit_bbox"]
    half = valid.shape[0] // 2
    scene["bbox_gt"] = boxes[:half][valid[:half]]
    return scene


def golden_geometry(gold):
    return int(gold["HEIGHT"]), int(gold["WIDTH"]), int(gold["EDGE"])
