"""Class labels for class-agnostic 2D masks (include/gpn.h section GR): mask pooling and a k-nearest-neighbour part classifier.

Restates the part of the reference's ``structure/`` pipeline that turns "pixel masks + an image feature map" into "the part class
of every mask":
  ``mask_change_reso`` (structure/utils.py:491-497)            -> ``resize_masks``
  ``mask_fea_process`` / ``sam_mask_fea_process`` (gapartnet.py:145-158) -> ``mask_features``
  ``load_data_single_file`` (utils.py:499-520)                 -> ``load_feature_bank``
  ``KNN_classifier`` + ``load_models`` (utils.py:522-528, gapartnet.py:777-782) -> ``PartGrounder``
  ``get_GAPart_grounding_result`` / ``get_sam_grounding_result`` (gapartnet.py:180-204) -> ``PartGrounder.predict`` / ``.label_masks``
The feature extractor (DINOv2) and the segmenter (SAM) are the caller's: feature maps and the bank come in as arrays.

For a 0/1 mask the reference's detour through a colour map collapses: the map only ever yields its two end entries, whose first
channel is 128 outside the mask and 0 inside, so the low-resolution weight is ``1 - clip(L, 0, 128) / 128`` with L = Pillow's default
(bicubic) resize of the 8-bit image ``128 (1 - m)``.  ``resize_masks`` returns the clipped bytes L ("levels", 0 = inside) and is
byte-equal to Pillow: the resample is integer arithmetic (coefficients with 22 fraction bits, a horizontal pass to a uint8
intermediate, then a vertical pass, each ``clip8((2^21 + sum c p) >> 22)``), restated here.

The classifier is ``KNeighborsClassifier(n_neighbors=k)`` with two rules made explicit: equal distances put the lower bank row
first (sklearn leaves that open), equal votes give the smallest class id (as sklearn does).

On GPU tensors every step is a launch of csrc/ground.hip and nothing is read back; on CPU tensors the numpy formulation below runs
the same contracts (distances in float64 there), as every module of this package does.
"""
import functools
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..hip_ops import GROUND_MAX_CLASSES as MAX_CLASSES  # (the limits of include/gpn.h section GR; importing loads no library)
from ..hip_ops import GROUND_MAX_K as MAX_K
from ..hip_ops import GROUND_MAX_SIDE as MAX_SIDE
from .info import PART_ID2NAME

PRECISION_BITS = 22  # fraction bits of Pillow's 8-bit resample coefficients


def _err(msg: str):
    from .._C import GpnError
    return GpnError(msg)


# ---- Pillow's bicubic coefficient tables -------------------------------------------------------------------------------------------
def _bicubic(x: float) -> float:
    x = abs(x)
    if x < 1.0:
        return (1.5 * x - 2.5) * x * x + 1
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5
    return 0.0


def _axis_table(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """one axis: (bounds [n_out,2] int32 = (first input index, count), coef [n_out,ksize] int32).  Window, weights (a = -0.5,
    support 2 max(1, in/out)), their normalisation in double and the rounding trunc(+-0.5 + w 2^22) are Pillow's."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for i in range(n_out):
        center = (i + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n_in) - first
        w = [_bicubic((j + first - center + 0.5) / filterscale) for j in range(count)]
        total = 0.0
        for v in w:
            total += v
        bounds[i] = (first, count)
        for j, v in enumerate(w):
            if total != 0.0:
                v = v / total
            coef[i, j] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
    return bounds, coef


@functools.lru_cache(maxsize=64)
def resample_tables(H: int, W: int, Hf: int, Wf: int):
    """-> (xbounds [Wf,2], xcoef [Wf,ksx], ybounds [Hf,2], ycoef [Hf,ksy]) for the resize (H, W) -> (Hf, Wf); one tuple per shape"""
    xb, xc = _axis_table(W, Wf)
    yb, yc = _axis_table(H, Hf)
    for a in (xb, xc, yb, yc):
        a.setflags(write=False)
    return xb, xc, yb, yc


def _resample_pass(img: np.ndarray, bounds: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """the integer pass along the last axis of a uint8 array"""
    out = np.empty(img.shape[:-1] + (bounds.shape[0],), dtype=np.uint8)
    wide = img.astype(np.int32)
    for i in range(bounds.shape[0]):
        first, count = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (wide[..., first:first + count] * coef[i, :count]).sum(axis=-1, dtype=np.int32) + (1 << (PRECISION_BITS - 1))
        out[..., i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_masks(masks, size: Tuple[int, int]):
    """binary masks [K,H,W] (bool or uint8, non-zero = member) -> levels [K,Hf,Wf] uint8 in 0..128, 0 = fully inside; ``size`` =
    (Hf, Wf).  Byte-equal to ``np.array(Image.fromarray(128 * (1 - m)).resize((Wf, Hf))).clip(0, 128)``.  The reference's weight is
    ``(128 - level) / 128``.  Float-valued masks are refused."""
    masks = torch.as_tensor(masks)
    if masks.dim() != 3 or masks.dtype not in (torch.bool, torch.uint8):
        raise _err("resize_masks: masks [K,H,W] of dtype bool or uint8 (float-valued masks are not supported)")
    Hf, Wf = int(size[0]), int(size[1])
    H, W = int(masks.shape[1]), int(masks.shape[2])
    if not (1 <= Hf <= MAX_SIDE and 1 <= Wf <= MAX_SIDE and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise _err(f"resize_masks: sides must lie in 1..{MAX_SIDE}, got {(H, W)} -> {(Hf, Wf)}")
    tables = resample_tables(H, W, Hf, Wf)
    if masks.is_cuda:
        from .. import hip_ops
        return hip_ops.ground_mask_resize(masks, (Hf, Wf), tables)
    xb, xc, yb, yc = tables
    img = np.where(masks.numpy() != 0, 0, 128).astype(np.uint8)
    mid = _resample_pass(img, xb, xc)
    out = np.swapaxes(_resample_pass(np.swapaxes(mid, 1, 2), yb, yc), 1, 2)
    return torch.from_numpy(np.minimum(out, 128).astype(np.uint8))


def _views(mask_view, K: int, V: int, device) -> torch.Tensor:
    if mask_view is None:
        if V != 1:
            raise _err(f"mask_view is needed with {V} feature maps")
        return torch.zeros(K, dtype=torch.int32, device=device)
    mv = torch.as_tensor(mask_view).reshape(-1)
    if mv.numel() != K:
        raise _err(f"mask_view: one entry per mask ({K}), got {mv.numel()}")
    if not mv.is_cuda and K and (int(mv.min()) < 0 or int(mv.max()) >= V):
        raise _err(f"mask_view: entries must lie in 0..{V - 1}")
    return mv.to(device=device, dtype=torch.int32)


def pool_levels(feature_maps, levels, mask_view=None):
    """feature_maps [V,Hf,Wf,C] (or [Hf,Wf,C]) f32, levels [K,Hf,Wf] uint8 -> [K,C] f32: the max over the pixels of
    ``fea * ((128 - min(level, 128)) / 128)`` - one fp32 product per element, the weight being exact.  ``mask_view`` [K]: the map
    of each mask (on the device it is clamped into 0..V-1 instead of being read back)."""
    fea = torch.as_tensor(feature_maps)
    if fea.dim() == 3:
        fea = fea[None]
    levels = torch.as_tensor(levels)
    if fea.dim() != 4 or levels.dim() != 3 or levels.dtype != torch.uint8 or tuple(levels.shape[1:]) != tuple(fea.shape[1:3]):
        raise _err("pool_levels: feature_maps [V,Hf,Wf,C] and uint8 levels [K,Hf,Wf] of the maps' size")
    K, V = int(levels.shape[0]), int(fea.shape[0])
    mv = _views(mask_view, K, V, fea.device)
    if fea.is_cuda:
        from .. import hip_ops
        return hip_ops.ground_mask_pool(fea, levels.to(fea.device), mv)
    f = fea.to(torch.float32).numpy()
    w = ((128 - np.minimum(levels.numpy().astype(np.int32), 128)).astype(np.float32) / np.float32(128.0))
    out = np.empty((K, f.shape[-1]), dtype=np.float32)
    for k in range(K):
        out[k] = (f[int(mv[k])] * w[k][..., None]).max(axis=(0, 1))
    return torch.from_numpy(out)


def mask_features(feature_maps, masks, mask_view=None):
    """feature_maps [V,Hf,Wf,C] (or [Hf,Wf,C]), binary masks [K,H,W] -> [K,C] f32: ``resize_masks`` to the maps' size, then
    ``pool_levels`` (the reference's fea_max / sam_fea_max).  Masks follow the maps' device."""
    fea = torch.as_tensor(feature_maps)
    masks = torch.as_tensor(masks).to(fea.device)
    size = tuple(int(v) for v in fea.shape[-3:-1])
    return pool_levels(fea, resize_masks(masks, size), mask_view)


# ---- the bank ------------------------------------------------------------------------------------------------------------------------
def load_feature_bank(path: str, split: Optional[str] = "train") -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (feats f32 [M,D], labels i64 [M]).  Reads the reference's bank file - ``np.save`` of a dict with ``feas``, ``cat_ids``,
    ``splits`` (and more), loaded as ``np.load(path, allow_pickle=True).item()`` does - keeping the rows whose split equals
    ``split`` (None: all rows) with the ids cast to int one by one as ``load_data_single_file`` does; or a plain ``.npz`` with
    ``feas`` and ``cat_ids`` (and optionally ``splits``).  A pickled file runs code when loaded: read only banks you trust."""
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            data = {k: z[k] for k in z.files}
    else:
        data = np.load(path, allow_pickle=True)
        data = data.item() if isinstance(data, np.ndarray) and data.dtype == object and data.shape == () else data
    if not isinstance(data, dict) or "feas" not in data or "cat_ids" not in data:
        raise ValueError(f"{path}: a feature bank is a dict with `feas` and `cat_ids` (and `splits`)")
    feas = np.asarray(data["feas"])
    ids = np.array([int(v) for v in np.asarray(data["cat_ids"]).reshape(-1)], dtype=np.int64)
    if feas.ndim != 2 or feas.shape[0] != ids.shape[0]:
        raise ValueError(f"{path}: `feas` must be [M,D] with `cat_ids` [M], got {feas.shape} and {ids.shape}")
    if split is not None and "splits" in data:
        keep = np.asarray(data["splits"]).reshape(-1) == split
        if keep.shape[0] != ids.shape[0]:
            raise ValueError(f"{path}: `splits` must have one entry per row")
        feas, ids = feas[keep], ids[keep]
    return torch.from_numpy(np.ascontiguousarray(feas, dtype=np.float32)), torch.from_numpy(ids)


def _knn_numpy(q: np.ndarray, bank: np.ndarray, labels: np.ndarray, k: int, n_classes: int):
    q64, b64 = q.astype(np.float64), bank.astype(np.float64)
    Q, M = q64.shape[0], b64.shape[0]
    idx = np.zeros((Q, k), dtype=np.int32)
    d2 = np.zeros((Q, k), dtype=np.float32)
    votes = np.zeros((Q, n_classes), dtype=np.int32)
    rows = np.arange(M)
    for i in range(Q):
        d = ((b64 - q64[i]) ** 2).sum(axis=1)
        order = np.lexsort((rows, d))[:k]  # by distance, then by row
        idx[i], d2[i] = order, d[order]
        votes[i] = np.bincount(labels[order], minlength=n_classes)
    return idx, d2, votes, votes.argmax(axis=1).astype(np.int32)  # argmax: the first (smallest) class among equal votes


class PartGrounder:
    """The k-nearest-neighbour part classifier over a bank of labelled part features (the reference's
    ``KNeighborsClassifier(n_neighbors=5)`` fitted on the train rows of its bank).  Holds the bank, its squared norms and its labels
    on the bank's device once; the labels are checked here (``GpnError`` for one outside ``[0, n_classes)``, for ``M < k`` and for
    k, n_classes out of range), so that no call has to read them back."""

    def __init__(self, bank_feats, bank_labels, k: int = 5, n_classes: int = len(PART_ID2NAME), device=None):
        feats = torch.as_tensor(bank_feats)
        labels = torch.as_tensor(bank_labels).reshape(-1)
        if device is not None:
            feats = feats.to(device)
        k, n_classes = int(k), int(n_classes)
        if feats.dim() != 2 or feats.shape[1] < 1 or labels.numel() != feats.shape[0]:
            raise _err(f"PartGrounder: bank_feats [M,D] with bank_labels [M], got {tuple(feats.shape)} and {tuple(labels.shape)}")
        if not (1 <= k <= MAX_K) or not (1 <= n_classes <= MAX_CLASSES):
            raise _err(f"PartGrounder: k in 1..{MAX_K} and n_classes in 1..{MAX_CLASSES}, got k = {k}, n_classes = {n_classes}")
        if feats.shape[0] < k:
            raise _err(f"PartGrounder: the bank has {feats.shape[0]} rows, fewer than k = {k}")
        if labels.dtype.is_floating_point or int(labels.min()) < 0 or int(labels.max()) >= n_classes:
            raise _err(f"PartGrounder: bank labels must be integers in [0, {n_classes})")
        self.k, self.n_classes = k, n_classes
        self.feats = feats.to(torch.float32).contiguous()
        self.labels = labels.to(device=self.feats.device, dtype=torch.int32).contiguous()
        self.norms = None
        if self.feats.is_cuda:
            from .. import hip_ops
            self.norms = hip_ops.ground_bank_norms(self.feats)

    @property
    def device(self):
        return self.feats.device

    def kneighbors(self, feats) -> Dict[str, torch.Tensor]:
        """feats [Q,D] -> dict: ``index`` [Q,k] i32 (bank rows, ascending by (distance, row)), ``d2`` [Q,k] f32 squared
        distances, ``votes`` [Q,n_classes] i32, ``label`` [Q] i32"""
        q = torch.as_tensor(feats)
        if q.dim() != 2 or q.shape[1] != self.feats.shape[1]:
            raise _err(f"PartGrounder: features must be [Q,{self.feats.shape[1]}], got {tuple(q.shape)}")
        if q.device != self.feats.device:
            raise _err(f"PartGrounder: features on {q.device}, the bank on {self.feats.device}")
        if self.feats.is_cuda:
            from .. import hip_ops
            got = hip_ops.ground_knn(q, self.feats, self.norms, self.labels, self.k, self.n_classes)
        else:
            got = tuple(torch.from_numpy(a) for a in _knn_numpy(q.to(torch.float32).numpy(), self.feats.numpy(), self.labels.numpy(),
                                                                 self.k, self.n_classes))
        return dict(zip(("index", "d2", "votes", "label"), got))

    def predict(self, feats) -> torch.Tensor:
        """feats [Q,D] -> part class [Q] i64 (the reference's ``classifier.predict``)"""
        return self.kneighbors(feats)["label"].long()

    def label_masks(self, feature_maps, masks, mask_view=None) -> Dict[str, torch.Tensor]:
        """feature_maps [V,Hf,Wf,C] (or [Hf,Wf,C]) on the bank's device, binary masks [K,H,W], ``mask_view`` [K] -> dict: ``label``
        [K] i64, ``votes`` [K,n_classes] i32, ``index`` / ``d2`` [K,k], ``features`` [K,C] f32 (the pooled vectors)"""
        fea = torch.as_tensor(feature_maps)
        if fea.device != self.feats.device:
            raise _err(f"PartGrounder: feature maps on {fea.device}, the bank on {self.feats.device}")
        pooled = mask_features(fea, masks, mask_view)
        out = self.kneighbors(pooled)
        out["label"] = out["label"].long()
        out["features"] = pooled
        return out
