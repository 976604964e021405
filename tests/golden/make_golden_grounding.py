"""Records tests/golden/grounding.npz from the two libraries the reference's grounding path calls: Pillow's ``Image.resize`` (what
``mask_change_reso`` runs on every mask) and scikit-learn's ``KNeighborsClassifier(n_neighbors=5)`` (what ``KNN_classifier``
fits and ``get_GAPart_grounding_result`` asks for predictions).  Needs Pillow and scikit-learn; the tests that read the file need
neither.

    python tests/golden/make_golden_grounding.py

Masks: the image handed to Pillow is the one the reference builds for a 0/1 mask - an RGB image whose first channel is 128
outside the mask and 0 inside (the two end entries of its colour map; the other two channels ride along and do not meet the first)
- resized with Pillow's default filter, first channel, clipped to 0..128.  Stored bit-packed.
kNN: a clustered bank of 600 x 48 float32 rows with 10 classes and 40 queries; ``predict`` and ``kneighbors``.
"""
import os

import numpy as np


def blob_masks(rng, K, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((K, H, W), dtype=bool)
    for k in range(K):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = rng.uniform(1.5, H / 2), rng.uniform(1.5, W / 2)
            if rng.random() < 0.5:
                masks[k] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            else:
                masks[k] |= (abs(yy - cy) <= ry / 2) & (abs(xx - cx) <= rx / 2)
        masks[k] ^= rng.random((H, W)) < 0.02  # speckle: single pixels exercise the negative lobes
    return masks


def pillow_levels(mask, Hf, Wf):
    from PIL import Image
    rgb = np.zeros(mask.shape + (3,), dtype=np.uint8)
    rgb[..., 0] = np.where(mask, 0, 128)
    rgb[..., 2] = np.where(mask, 128, 0)
    img = Image.fromarray(rgb, "RGB").resize((Wf, Hf))
    return np.array(img)[:, :, 0].clip(0, 128).astype(np.uint8)


def main():
    import PIL
    import sklearn
    from sklearn.neighbors import KNeighborsClassifier
    rng = np.random.default_rng(20240611)
    out = {"pillow_version": np.array(PIL.__version__), "sklearn_version": np.array(sklearn.__version__)}
    for name, (K, H, W, Hf, Wf) in {"a": (3, 96, 128, 50, 50), "b": (2, 50, 50, 50, 50), "c": (2, 37, 53, 16, 12)}.items():
        masks = blob_masks(rng, K, H, W)
        out[f"masks_{name}_bits"] = np.packbits(masks.reshape(K, -1), axis=1)
        out[f"masks_{name}_shape"] = np.array([K, H, W, Hf, Wf], dtype=np.int64)
        out[f"levels_{name}"] = np.stack([pillow_levels(m, Hf, Wf) for m in masks])
    M, D, Q, C = 600, 48, 40, 10
    centres = rng.normal(size=(C, D)).astype(np.float32) * 1.5
    labels = rng.integers(0, C, size=M)
    bank = (centres[labels] + rng.normal(size=(M, D)) * 0.7).astype(np.float32)
    qlab = rng.integers(0, C, size=Q)
    queries = (centres[qlab] + rng.normal(size=(Q, D)) * 0.9).astype(np.float32)
    clf = KNeighborsClassifier(n_neighbors=5).fit(bank, labels)
    dist, idx = clf.kneighbors(queries)
    out.update(knn_bank=bank, knn_labels=labels.astype(np.int64), knn_queries=queries, knn_pred=clf.predict(queries).astype(np.int64),
               knn_index=idx.astype(np.int64), knn_dist=dist.astype(np.float64))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "grounding.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
