"""TEST INFRASTRUCTURE - numpy float64 restatement of the pose-evaluation contract (include/gpn.h section PE), one item at a time
in plain loops: the instance fit by numpy.linalg.svd, the rotation angle, the face clipping with its tie rule.  The kernels
(csrc/poseeval.hip) and the torch formulation (gapartnet_amd/misc/pose_metrics.py) are compared with it; it is itself compared
with scipy's half-space intersection (tests/test_pose_eval_cpu.py).  Only tests import this module."""
import numpy as np

SIGNS = np.array([[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, -1], [1, -1, 1], [-1, 1, 1], [1, 1, 1]], dtype=np.float64)
FACES = [(0, 2, 6, 3), (1, 4, 7, 5), (0, 1, 5, 3), (2, 4, 7, 6), (0, 1, 4, 2), (3, 5, 7, 6)]  # face 2 * axis + side


def box_corners(scale, frame, t, half):
    """corners of the box with half extents half * scale along the rows of `frame` about t"""
    return (SIGNS * np.asarray(half) * scale) @ np.asarray(frame) + np.asarray(t)


def fit_instance(xyz, npcs):
    """xyz ~ npcs @ (s R) + t over all points (float32 values, float64 arithmetic) -> dict or None where there is no pose"""
    src, dst = np.asarray(npcs, np.float32).astype(np.float64), np.asarray(xyz, np.float32).astype(np.float64)
    n = src.shape[0]
    if n < 3:
        return None
    mu_s, mu_d = src.mean(0), dst.mean(0)
    cs, cd = src - mu_s, dst - mu_d
    cov, css = cd.T @ cs / n, cs.T @ cs / n
    if not (np.isfinite(cov).all() and np.isfinite(css).all()):
        return None
    sv = np.linalg.svd(css, compute_uv=False)
    if not (sv[0] > 0 and sv[1] >= 1e-9 * sv[0]):
        return None
    U, S, Vh = np.linalg.svd(cov)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2], U[:, 2] = -S[2], -U[:, 2]
    scale = S.sum() / np.trace(css)
    R = (U @ Vh).T
    t = mu_d - mu_s @ (scale * R)
    half = np.abs(src).max(0)
    return {"count": n, "scale": scale, "rotation": R, "translation": t, "half": half, "bbox": box_corners(scale, R, t, half)}


def fit_slots(xyz, npcs, slot, scene_offsets, W):
    """every slot scene * W + id of every scene, from the rows of its own scene -> list of (count, dict or None)"""
    out = []
    for s in range(len(scene_offsets) - 1):
        lo, hi = int(scene_offsets[s]), int(scene_offsets[s + 1])
        for w in range(W):
            rows = lo + np.nonzero(np.asarray(slot[lo:hi]) == s * W + w)[0]
            out.append((len(rows), fit_instance(xyz[rows], npcs[rows])))
    return out


def _frame(corners):
    c = corners.sum(0) / 8.0
    e = (corners[1:4] - corners[0]) / 2.0
    h = np.sqrt((e * e).sum(1))
    with np.errstate(all="ignore"):
        return c, e / h[:, None], h


def _dist(p, c, n, h):
    q = p - c
    return (q[0] * n[0] + q[1] * n[1]) + q[2] * n[2] - h


SNAP = 2.0 ** -26  # a vertex within SNAP x the largest half extent of the two boxes of a plane is ON it


def _clip_face(verts, normal, c, u, h, ties_may_be_inside, snap):
    poly = [np.array(v, dtype=np.float64) for v in verts]
    for pl in range(6):
        pn = u[pl // 2] * (1.0 if pl % 2 else -1.0)
        tie_in = ties_may_be_inside and float(normal @ pn) > 0.0
        inside = lambda d: d < 0.0 or (d == 0.0 and tie_in)
        new = []
        for i, p in enumerate(poly):
            q = poly[(i + 1) % len(poly)]
            dp, dq = _dist(p, c, pn, h[pl // 2]), _dist(q, c, pn, h[pl // 2])
            dp, dq = (0.0 if abs(dp) <= snap else dp), (0.0 if abs(dq) <= snap else dq)
            if inside(dp):
                new.append(p)
            if inside(dp) != inside(dq):
                new.append(p + dp / (dp - dq) * (q - p))
        poly = new
        if not poly:
            break
    return poly


def _cone(poly, normal, apex):
    if len(poly) < 3:
        return 0.0
    s = np.zeros(3)
    for i in range(1, len(poly) - 1):
        s += np.cross(poly[i] - poly[0], poly[i + 1] - poly[0])
    return 0.5 * abs(float(s @ normal)) * float((poly[0] - apex) @ normal) / 3.0


def box_intersection(a, b):
    """(intersection volume, volume of a, volume of b) of two boxes given as [8,3] corners; NaN without a volume"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ca, ua, ha = _frame(a)
    cb, ub, hb = _frame(b)
    va, vb = 8.0 * ha.prod(), 8.0 * hb.prod()
    if not (np.isfinite(a).all() and np.isfinite(b).all() and va > 0 and vb > 0):
        return float("nan"), va, vb
    inter, snap = 0.0, SNAP * max(ha.max(), hb.max())
    for f in range(6):
        n = ua[f // 2] * (1.0 if f % 2 else -1.0)
        inter += _cone(_clip_face(a[list(FACES[f])], n, cb, ub, hb, True, snap), n, ca)
    for f in range(6):
        n = ub[f // 2] * (1.0 if f % 2 else -1.0)
        inter += _cone(_clip_face(b[list(FACES[f])], n, ca, ua, ha, False, snap), n, ca)
    return inter, va, vb


def box_iou(a, b):
    inter, va, vb = box_intersection(a, b)
    return inter / (va + vb - inter)


def angle_deg(Rp, F):
    M = np.asarray(Rp) @ np.asarray(F).T
    v = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2.0
    return float(np.degrees(np.arctan2(np.sqrt(v @ v), (np.trace(M) - 1.0) / 2.0)))


def pair_errors(pred, gt, candidates):
    """pred, gt: (scale, rotation, translation, half); candidates [n,3,3] -> dict with every candidate's angle and IoU as well"""
    sp, Rp, tp, hp = pred
    sg, Rg, tg, hg = gt
    box_p = box_corners(sp, Rp, tp, hp)
    res, ious = [], []
    for Sk in candidates:
        F = np.asarray(Sk) @ np.asarray(Rg)
        res.append(angle_deg(Rp, F))
        ious.append(box_iou(box_p, box_corners(sg, F, tg, hg)))
    k_re, k_iou = 0, 0
    for k in range(1, len(res)):
        if res[k] < res[k_re]:
            k_re = k
        if ious[k] > ious[k_iou]:
            k_iou = k
    return {"re_deg": res[k_re], "k_re": k_re, "te": float(np.linalg.norm(np.asarray(tp) - np.asarray(tg))), "se": abs(sp - sg),
            "iou": ious[k_iou], "k_iou": k_iou, "all_re": np.array(res), "all_iou": np.array(ious)}


def scipy_intersection_volume(a, b):
    """volume of the intersection of two boxes by scipy's half-space intersection and convex hull; 0 when they do not overlap"""
    from scipy.spatial import ConvexHull, HalfspaceIntersection
    from scipy.optimize import linprog
    rows = []
    for corners in (a, b):
        c, u, h = _frame(np.asarray(corners, np.float64))
        for i in range(3):
            rows.append(np.concatenate([u[i], [-(u[i] @ c) - h[i]]]))
            rows.append(np.concatenate([-u[i], [(u[i] @ c) - h[i]]]))
    hs = np.array(rows)
    # the deepest interior point (Chebyshev centre): maximise r subject to n.x + r <= -offset
    res = linprog(np.array([0, 0, 0, -1.0]), A_ub=np.hstack([hs[:, :3], np.ones((12, 1))]), b_ub=-hs[:, 3], bounds=[(None, None)] * 4)
    if res.status != 0 or res.x[3] <= 1e-12:
        return 0.0
    return float(ConvexHull(HalfspaceIntersection(hs, res.x[:3]).intersections).volume)
