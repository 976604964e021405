"""Test-time part predictions and the 3 x 4 panel of images per sampled scene, on the GPU (reference: network/model.py:930-999,
misc/visu.py, misc/visu_util.py; the kernels: csrc/visu.hip, include/gpn.h section VS).

``scene_predictions``   a batch's kept proposals -> per-point instance / NPCS maps and one 9-DoF box per proposal
``render_panels``       all twelve tiles of all sampled scenes into one uint8 canvas on the device: four launches
``visualize_gapartnet`` the reference's entry point: reads a scene's files, renders, writes the PNG files
``visualize_scenes``    the same for a batch of scenes; PNG encoding runs on host threads

The reference draws the panel scene by scene in Python (map2image: a loop over 20 000 points per tile) and needs OpenCV.  Two stated
deviations: colour sources outside [0, 256) are clamped and NaN gives 0 where the reference's cast is undefined,
and box edges follow the line rule of include/gpn.h instead of cv2.line.  Captions use PIL's default font.
"""
import colorsys
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .pose_fitting_batched import estimate_pose_from_npcs_batched

HEIGHT, WIDTH, EDGE = 800, 800, 40             # the dataset's render settings
FX = FY = 1268.637939453125
U0 = V0 = 400.0
OPTIONS = ("raw", "pc", "sem_pred", "ins_pred", "npcs_pred", "bbox_pred", "bbox_pred_pure", "sem_gt", "ins_gt", "npcs_gt", "bbox_gt",
           "bbox_gt_pure")
# (row, col) of every option in the panel
TILE_POS = {"raw": (0, 0), "sem_gt": (0, 1), "ins_gt": (0, 2), "npcs_gt": (0, 3),
            "pc": (1, 0), "sem_pred": (1, 1), "ins_pred": (1, 2), "npcs_pred": (1, 3),
            "bbox_gt_pure": (2, 0), "bbox_gt": (2, 1), "bbox_pred": (2, 2), "bbox_pred_pure": (2, 3)}
_FILE_OF = {"bbox_pred_pure": "bbox_pure"}     # the reference's name of that tile's file
_SPLIT_DIRS = ("val", "test_intra", "test_inter")


def default_palette() -> np.ndarray:
    """[21,3] uint8: index 0 is the light grey of "no part"; 20 distinct colours on a golden-ratio walk around the hue circle"""
    rows = [(230, 230, 230)]
    for i in range(20):
        r, g, b = colorsys.hsv_to_rgb((0.11 + i * 0.6180339887) % 1.0, 0.55 + 0.15 * (i % 3), 0.95 - 0.2 * (i % 2))
        rows.append((int(r * 255), int(g * 255), int(b * 255)))
    return np.asarray(rows, dtype=np.uint8)


def canvas_shape(H: int = HEIGHT, W: int = WIDTH, edge: int = EDGE):
    return 3 * (H + edge) + edge, 4 * (W + edge) + edge


@dataclass
class ScenePredictions:
    ins_map: torch.Tensor       # [N] i32: 0, or proposal + 1
    npcs_map: torch.Tensor      # [N,3] f32
    bbox: torch.Tensor          # [Q,8,3] f64, normalised frame
    box_scene: torch.Tensor     # [Q] i64
    box_proposal: torch.Tensor  # [Q] i64
    scene_offsets: torch.Tensor  # [S+1] i64 (host)


def _raw():
    from .. import backend
    raw = backend.raw()
    if raw.name != "hip":
        raise RuntimeError("test-time rendering needs the HIP library as the operator backend")
    return raw


def _offsets(scene_offsets) -> torch.Tensor:
    return torch.as_tensor(scene_offsets, dtype=torch.int64).cpu()


@torch.no_grad()
def scene_predictions(proposals, scene_offsets, picks: Optional[torch.Tensor] = None, max_iters: int = 100) -> ScenePredictions:
    """``proposals``: the Instances ``test_step`` keeps of one batch (valid_mask or valid_indices, sorted_indices,
    proposal_offsets, npcs_valid_mask, npcs_preds, pt_xyz, batch_indices); ``scene_offsets`` [S+1]: the scenes' rows in the batch.
    One call of gpn_scene_maps, then every proposal's box in one gpn_pose_fit.  A proposal with fewer than 10 points gets no box
    (model.py:973), nor does one the fit marks invalid.  ``picks`` [P,H,5]: the RANSAC draws (drawn if None)."""
    hip = _raw()
    off = _offsets(scene_offsets)
    n_rows = int(off[-1])
    dev = proposals.sorted_indices.device
    valid_indices = proposals.valid_indices
    if valid_indices is None:
        valid_indices = torch.nonzero(proposals.valid_mask).squeeze(1)
    po = proposals.proposal_offsets.to(dev).long()
    npcs_preds = proposals.npcs_preds
    if npcs_preds is None:
        npcs_preds = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    mask = proposals.npcs_valid_mask
    if mask is None:
        mask = torch.zeros(proposals.sorted_indices.shape[0], dtype=torch.bool, device=dev)
    ins_map, npcs_map, fit_npcs = hip.scene_maps(valid_indices, proposals.sorted_indices, po, mask, npcs_preds, n_rows)
    P = po.shape[0] - 1
    if P <= 0:
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        return ScenePredictions(ins_map, npcs_map, torch.zeros((0, 8, 3), dtype=torch.float64, device=dev), empty, empty, off)
    fit = estimate_pose_from_npcs_batched(proposals.pt_xyz, fit_npcs, po, picks=picks, max_iters=max_iters)
    keep = ((po[1:] - po[:-1]) >= 10) & fit["valid"]
    box_proposal = torch.nonzero(keep).squeeze(1)
    box_scene = proposals.batch_indices.index_select(0, po[:-1]).long().index_select(0, box_proposal)
    return ScenePredictions(ins_map, npcs_map, fit["bbox"].index_select(0, box_proposal), box_scene, box_proposal, off)


@torch.no_grad()
def gt_boxes(xyz, ins_gt, npcs_gt, scene_offsets, picks: Optional[torch.Tensor] = None, max_iters: int = 100):
    """the boxes of the GT tiles (misc/visu.py:204-217): every instance 0 .. max of every scene with more than 5 points, fitted
    from its GT NPCS, all scenes in one gpn_pose_fit.  -> (bbox [G,8,3] f64, box_scene [G] i64), scene by scene in ascending
    instance id.  ``picks`` [number of fitted instances, H, 5]."""
    dev = xyz.device
    off = _offsets(scene_offsets)
    S = off.shape[0] - 1
    sizes = (off[1:] - off[:-1]).to(dev)
    scene = torch.repeat_interleave(torch.arange(S, device=dev), sizes, output_size=int(off[-1]))
    ins = ins_gt.to(dev).long()
    rows = torch.nonzero(ins >= 0).squeeze(1)
    none = (torch.zeros((0, 8, 3), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev))
    if rows.numel() == 0:
        return none
    stride = int(ins.max()) + 1
    key = scene[rows] * stride + ins[rows]
    key, order = torch.sort(key, stable=True)       # the instance's points keep their order
    rows = rows[order]
    uniq, counts = torch.unique_consecutive(key, return_counts=True)
    fitted = counts > 5
    if not bool(fitted.any()):
        return none
    take = torch.repeat_interleave(fitted, counts)
    rows = rows[take]
    po = torch.zeros(int(fitted.sum()) + 1, dtype=torch.int64, device=dev)
    po[1:] = counts[fitted].cumsum(0)
    fit = estimate_pose_from_npcs_batched(xyz[rows].contiguous(), npcs_gt.to(dev)[rows].contiguous(), po, picks=picks,
                                          max_iters=max_iters)
    ok = fit["valid"]
    return fit["bbox"][ok], torch.div(uniq[fitted], stride, rounding_mode="floor")[ok]


@torch.no_grad()
def render_panels(xyz, rgb, scene_offsets, trans, *, sem_pred=None, ins_pred=None, npcs_pred=None, bbox_pred=None,
                  bbox_pred_scene=None, sem_gt=None, ins_gt=None, npcs_gt=None, bbox_gt=None, bbox_gt_scene=None,
                  raw: Optional[Sequence] = None, options: Sequence[str] = OPTIONS, H: int = HEIGHT, W: int = WIDTH,
                  EDGE: int = EDGE, fx: float = FX, fy: float = FY, u0: float = U0, v0: float = V0, palette=None,
                  gt_picks=None) -> torch.Tensor:
    """-> uint8 [S, 3 (H + EDGE) + EDGE, 4 (W + EDGE) + EDGE, 3] on the device: the reference's panel of every scene, without
    captions.  Per-point tensors cover all scenes' rows (scene s = rows scene_offsets[s]:scene_offsets[s+1]): xyz [n,3] f32 in the
    normalised frame, rgb [n,3] in [0, 1], sem_* / ins_* [n] labels, npcs_pred [n,3] in [0, 1], npcs_gt [n,3] in [-0.5, 0.5];
    trans [S,4] f64 = (r, cx, cy, cz) of the meta files; boxes [Q,8,3] f64 with their scene [Q]; raw: per scene an [H,W,3] uint8
    image or None.  GT boxes are fitted here (``gt_boxes``) unless given.  An option whose inputs are missing is an error."""
    hip = _raw()
    dev = xyz.device
    off = _offsets(scene_offsets)
    S = off.shape[0] - 1
    unknown = [o for o in options if o not in TILE_POS]
    if unknown:
        raise ValueError(f"unknown visualisation options {unknown}")
    ch, cw = canvas_shape(H, W, EDGE)
    canvas = torch.full((S, ch, cw, 3), 255, dtype=torch.uint8, device=dev)
    if S == 0:
        return canvas
    off_dev = off.to(dev)
    cam = (fx, fy, u0, v0)
    palette = torch.as_tensor(default_palette() if palette is None else np.asarray(palette, dtype=np.uint8)).to(dev)

    n_total = int(off[-1])
    if xyz.shape[0] != n_total or rgb.shape[0] != n_total or trans.numel() != S * 4:
        raise ValueError("render_panels: xyz / rgb must have scene_offsets[-1] rows and trans must be [S,4]")

    def need(name, value, per_point=True):
        if value is None:
            raise ValueError(f"render_panels: option {name!r} needs an input that was not given")
        if per_point and value.shape[0] != n_total:
            raise ValueError(f"render_panels: the input of option {name!r} has {value.shape[0]} rows, the scenes {n_total}")
        return value

    sources = {"pc": lambda: (hip.VISU_RGB, rgb, 0.0), "npcs_pred": lambda: (hip.VISU_RGB, need("npcs_pred", npcs_pred), 0.0),
               "npcs_gt": lambda: (hip.VISU_RGB, need("npcs_gt", npcs_gt), 0.5),
               "sem_pred": lambda: (hip.VISU_LABEL, need("sem_pred", sem_pred), 0.0),
               "sem_gt": lambda: (hip.VISU_LABEL, need("sem_gt", sem_gt), 0.0),
               "ins_pred": lambda: (hip.VISU_LABEL_MOD20, need("ins_pred", ins_pred), 0.0),
               "ins_gt": lambda: (hip.VISU_LABEL_MOD19P1, need("ins_gt", ins_gt), 0.0),
               "bbox_pred": lambda: (hip.VISU_RGB, rgb, 0.0), "bbox_gt": lambda: (hip.VISU_RGB, rgb, 0.0),
               "bbox_pred_pure": lambda: (hip.VISU_BLANK, None, 0.0), "bbox_gt_pure": lambda: (hip.VISU_BLANK, None, 0.0)}
    layers = []
    for name in options:
        if name != "raw":
            kind, src, offset = sources[name]()
            layers.append((kind, src, TILE_POS[name][0], TILE_POS[name][1], offset))
    winner = hip.points_winner(xyz, off_dev, trans, H, W, *cam)
    hip.points_paint(winner, off_dev, layers, palette, canvas, EDGE)
    if "raw" in options and raw is not None:
        y0, x0 = EDGE, EDGE
        for s, img in enumerate(raw):
            if img is not None:
                canvas[s, y0:y0 + H, x0:x0 + W] = torch.as_tensor(img, dtype=torch.uint8).to(dev)
    tiles = [TILE_POS[o] for o in ("bbox_pred", "bbox_pred_pure") if o in options]
    if tiles:
        hip.boxes_draw(need("bbox_pred", bbox_pred, False), need("bbox_pred", bbox_pred_scene, False), trans, H, W, *cam, tiles, canvas, EDGE)
    tiles = [TILE_POS[o] for o in ("bbox_gt", "bbox_gt_pure") if o in options]
    if tiles:
        if bbox_gt is None:
            bbox_gt, bbox_gt_scene = gt_boxes(xyz, need("bbox_gt", ins_gt), need("bbox_gt", npcs_gt), off, picks=gt_picks)
        hip.boxes_draw(bbox_gt, bbox_gt_scene, trans, H, W, *cam, tiles, canvas, EDGE)
    return canvas


# ---------------------------------------------------------------------------------------------------- files
def load_scene(data_root: str, split: str, name: str):
    """{root}/{split}/pth/{name}.pth (a 5- or 6-tuple: xyz, rgb, sem, ins, npcs[, ...]) and meta/{name}.txt (r, cx, cy, cz)"""
    data = torch.load(f"{data_root}/{split}/pth/{name}.pth", weights_only=False)
    pc, rgb, sem, ins, npcs = (np.asarray(a) for a in data[:5])
    trans = np.loadtxt(f"{data_root}/{split}/meta/{name}.txt").astype(np.float64).reshape(-1)[:4]
    return dict(xyz=pc.astype(np.float32), rgb=rgb.astype(np.float32), sem_gt=sem.astype(np.int32), ins_gt=ins.astype(np.int32),
                npcs_gt=npcs.astype(np.float32), trans=trans)


def _read_raw(raw_root: str, name: str, H: int, W: int):
    path = f"{raw_root}/{name}.png"
    if not raw_root or not os.path.exists(path):
        return None
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGB"))
    if img.shape[:2] != (H, W):
        raise ValueError(f"{path}: raw image is {img.shape[:2]}, the panel's tiles are {(H, W)}")
    return img


def _write_panel(canvas: np.ndarray, path: str, options, have_raw: bool, detail_dir: Optional[str], H: int, W: int, edge: int):
    """host side of one scene: the per-tile files, the captions (PIL's default font at the reference's anchor), the panel"""
    from PIL import Image, ImageDraw, ImageFont
    if detail_dir is not None:
        os.makedirs(detail_dir, exist_ok=True)
        for name in options:
            if name == "raw" and not have_raw:
                continue
            y0, x0 = edge + TILE_POS[name][0] * (H + edge), edge + TILE_POS[name][1] * (W + edge)
            Image.fromarray(np.ascontiguousarray(canvas[y0:y0 + H, x0:x0 + W])).save(
                os.path.join(detail_dir, _FILE_OF.get(name, name) + ".png"), compress_level=1)
    img = Image.fromarray(canvas)
    draw = ImageDraw.Draw(img)
    try:
        font = ImageFont.load_default(size=max(edge // 2, 8))
    except TypeError:   # (a Pillow whose default font has one size)
        font = ImageFont.load_default()
    for name in options:
        if name == "raw" and not have_raw:
            continue
        y0, x0 = edge + TILE_POS[name][0] * (H + edge), edge + TILE_POS[name][1] * (W + edge)
        at = (x0 + int(0.5 * (W - 3 * edge)), y0 + H + int(0.5 * edge))
        try:
            draw.text(at, name, fill=(0, 0, 0), font=font, anchor="ls")
        except ValueError:   # (a bitmap font has no anchors: its top-left corner a line above the anchor)
            draw.text((at[0], at[1] - 11), name, fill=(0, 0, 0), font=font)
    img.save(path, compress_level=1)


@torch.no_grad()
def visualize_scenes(SAVE_ROOT: str, GAPARTNET_DATA_ROOT: str, RAW_IMG_ROOT: str, save_option: Sequence[str], names: Sequence[str],
                     split: str, device, sem_preds: Sequence, ins_preds: Sequence, npcs_preds: Sequence, bboxes: Sequence,
                     save_detail: bool = False, batch: int = 8, pool: Optional[ThreadPoolExecutor] = None, H: int = HEIGHT,
                     W: int = WIDTH, edge: int = EDGE, palette=None, **camera) -> List[str]:
    """renders and writes the panels of ``names``; per scene the predictions as ``visualize_gapartnet`` takes them (tensors on the
    device or arrays; bboxes[i]: [Q_i,8,3]).  Scenes go through the GPU in batches of ``batch``; a batch's PNG files are encoded
    on host threads while the next batch renders.  -> the panel files' paths"""
    options = [o for o in OPTIONS if o in save_option]
    os.makedirs(f"{SAVE_ROOT}/{split}", exist_ok=True)
    own_pool = pool is None
    pool = pool or ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
    jobs, paths = [], []

    def dev_cat(items, dtype, trailing):
        items = [torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=device, dtype=dtype) for a in items]
        return torch.cat([a.reshape((-1,) + trailing) for a in items]) if items else torch.zeros((0,) + trailing, dtype=dtype,
                                                                                                  device=device)
    try:
        for b0 in range(0, len(names), batch):
            ids = range(b0, min(b0 + batch, len(names)))
            scenes = [load_scene(GAPARTNET_DATA_ROOT, split, names[i]) for i in ids]
            for i, sc in zip(ids, scenes):
                for what, given in (("sem_preds", sem_preds), ("ins_preds", ins_preds), ("npcs_preds", npcs_preds)):
                    if given is not None and given[i] is not None and len(given[i]) != sc["xyz"].shape[0]:
                        raise ValueError(f"{names[i]}: {what} has {len(given[i])} rows, the scene file {sc['xyz'].shape[0]}")
            off = np.concatenate([[0], np.cumsum([sc["xyz"].shape[0] for sc in scenes])]).astype(np.int64)
            raws = [_read_raw(RAW_IMG_ROOT, names[i], H, W) for i in ids] if "raw" in options else None
            boxes = [torch.as_tensor(np.asarray(bboxes[i], dtype=np.float64)).reshape(-1, 8, 3) if bboxes is not None and
                     bboxes[i] is not None and len(bboxes[i]) else torch.zeros((0, 8, 3), dtype=torch.float64) for i in ids]
            pick = (lambda given, dtype, trailing: None if given is None else dev_cat([given[i] for i in ids], dtype, trailing))
            canvas = render_panels(
                dev_cat([sc["xyz"] for sc in scenes], torch.float32, (3,)), dev_cat([sc["rgb"] for sc in scenes], torch.float32, (3,)),
                off, torch.as_tensor(np.stack([sc["trans"] for sc in scenes])).to(device),
                sem_pred=pick(sem_preds, torch.int32, ()), ins_pred=pick(ins_preds, torch.int32, ()),
                npcs_pred=pick(npcs_preds, torch.float32, (3,)), bbox_pred=torch.cat(boxes).to(device),
                bbox_pred_scene=torch.cat([torch.full((b.shape[0],), k, dtype=torch.int32) for k, b in enumerate(boxes)]).to(device),
                sem_gt=dev_cat([sc["sem_gt"] for sc in scenes], torch.int32, ()),
                ins_gt=dev_cat([sc["ins_gt"] for sc in scenes], torch.int32, ()),
                npcs_gt=dev_cat([sc["npcs_gt"] for sc in scenes], torch.float32, (3,)), raw=raws, options=options, H=H, W=W,
                EDGE=edge, palette=palette, **camera)
            host = canvas.cpu().numpy()   # (waits for this batch; the threads below run while the next one is prepared and rendered)
            for k, i in enumerate(ids):
                path = f"{SAVE_ROOT}/{split}/{names[i]}.png"
                paths.append(path)
                jobs.append(pool.submit(_write_panel, host[k], path, options, raws is not None and raws[k] is not None,
                                        f"{SAVE_ROOT}/{split}/{names[i]}" if save_detail else None, H, W, edge))
        for j in jobs:
            j.result()
    finally:
        if own_pool:
            pool.shutdown(wait=True)
    return paths


def visualize_gapartnet(SAVE_ROOT, GAPARTNET_DATA_ROOT, RAW_IMG_ROOT, save_option: List = [], name: str = "pc", split: str = "",
                        bboxes=None, sem_preds=None, ins_preds=None, npcs_preds=None, have_proposal=True, save_detail=False,
                        device=None):
    """the reference's entry point (misc/visu.py:35-261) for one scene: reads ``{root}/{split}/pth/{name}.pth`` and
    ``meta/{name}.txt``, writes ``{SAVE_ROOT}/{split}/{name}.png`` (and the tiles under ``{SAVE_ROOT}/{split}/{name}/`` with
    ``save_detail``).  ``device``: the GPU to render on (default: the current one)."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return visualize_scenes(SAVE_ROOT, GAPARTNET_DATA_ROOT, RAW_IMG_ROOT, save_option, [name], split, device,
                            None if sem_preds is None else [sem_preds], None if ins_preds is None else [ins_preds],
                            None if npcs_preds is None else [npcs_preds], [bboxes], save_detail=save_detail)[0]
