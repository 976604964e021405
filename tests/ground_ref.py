"""Oracle of the grounding path (include/gpn.h section GR), numpy only: Pillow's 8-bit bicubic resample restated as the integer
arithmetic it is, the float64 mask pool, and an exact float64 k-nearest-neighbour vote with the tie rules of the contract (equal
distances: the lower bank row first; equal votes: the smallest class id).  Written from Pillow's documented algorithm
(src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the horizontal then the vertical 8bpc pass), independently
of gapartnet_amd/misc/grounding.py; tests/test_grounding_cpu.py holds it against Pillow itself and against the golden file."""
import math

import numpy as np

PRECISION_BITS = 22


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def pillow_coeffs(n_in: int, n_out: int):
    """-> (bounds [n_out, 2] int32 = (first input index, count), coef [n_out, ksize] int32 with 22 fraction bits)"""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, coef


def _pass(img: np.ndarray, bounds, coef) -> np.ndarray:
    """one pass along the LAST axis of a uint8 array"""
    out = np.empty(img.shape[:-1] + (bounds.shape[0],), np.uint8)
    src = img.astype(np.int64)
    for xx in range(bounds.shape[0]):
        lo, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., lo:lo + n] * coef[xx, :n].astype(np.int64)).sum(-1)
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resample_u8(img: np.ndarray, size) -> np.ndarray:
    """Pillow's Image.resize(size = (Hf, Wf) here, as rows x columns) with the bicubic filter on [..., H, W] uint8"""
    Hf, Wf = size
    H, W = img.shape[-2:]
    mid = _pass(img, *pillow_coeffs(W, Wf))
    return np.swapaxes(_pass(np.swapaxes(mid, -1, -2), *pillow_coeffs(H, Hf)), -1, -2)


def mask_levels(masks: np.ndarray, size) -> np.ndarray:
    """binary masks [K, H, W] -> levels [K, Hf, Wf] uint8 in 0..128 (0 = inside)"""
    img = np.where(np.asarray(masks) != 0, 0, 128).astype(np.uint8)
    return np.minimum(resample_u8(img, size), 128).astype(np.uint8)


def mask_pool(fea: np.ndarray, levels: np.ndarray, mask_view=None) -> np.ndarray:
    """fea [V, Hf, Wf, C], levels [K, Hf, Wf] -> [K, C] float64"""
    fea = np.asarray(fea, np.float64)
    K = levels.shape[0]
    view = np.zeros(K, np.int64) if mask_view is None else np.asarray(mask_view, np.int64)
    w = (128.0 - np.minimum(levels.astype(np.float64), 128.0)) / 128.0
    return np.stack([(fea[view[k]] * w[k][..., None]).max(axis=(0, 1)) for k in range(K)]) if K else np.zeros((0, fea.shape[-1]))


def knn(queries: np.ndarray, bank: np.ndarray, labels: np.ndarray, k: int, n_classes: int):
    """-> (index [Q, k], d2 [Q, k] float64, votes [Q, n_classes], label [Q], all_d2 [Q, M]); d2 = the sum of squared differences
    in float64"""
    q = np.asarray(queries, np.float64)
    b = np.asarray(bank, np.float64)
    Q, M = q.shape[0], b.shape[0]
    d2 = np.empty((Q, M))
    for i in range(Q):
        d2[i] = ((b - q[i]) ** 2).sum(1)
    idx = np.stack([np.lexsort((np.arange(M), d2[i]))[:k] for i in range(Q)]) if Q else np.zeros((0, k), np.int64)
    nd = np.take_along_axis(d2, idx, 1)
    votes = np.zeros((Q, n_classes), np.int64)
    lab = np.asarray(labels, np.int64)[idx]
    for i in range(Q):
        votes[i] = np.bincount(lab[i], minlength=n_classes)
    return idx, nd, votes, votes.argmax(1), d2
