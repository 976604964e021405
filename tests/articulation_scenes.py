"""Seeded instance maps and one rendered two-frame scene for the articulation tests (include/gpn.h section AR)."""
import numpy as np

INT32_MIN = -2 ** 31
DOOR, DRAWER, HANDLE = 4, 5, 1   # hinge_door, slider_drawer, line_fixed_handle (misc/info.TARGET_PARTS)


def blocky_map(rng, H, W, n, block=5):
    """[H,W] i32: piecewise constant over blocks of ``block`` pixels, values -1 .. n-1 (what an instance map looks like), with a
    tenth of the pixels redrawn one by one"""
    if n == 0:
        return np.full((H, W), -1, np.int32)
    coarse = rng.randint(-1, n, size=((H + block - 1) // block, (W + block - 1) // block))
    m = np.repeat(np.repeat(coarse, block, 0), block, 1)[:H, :W].astype(np.int32)
    noise = rng.rand(H, W) < 0.1
    m[noise] = rng.randint(-1, n, size=int(noise.sum()))
    return m


def random_pair(seed, V, H, W, n_a, n_b, junk=False, valid_rate=0.8):
    """-> dict(inst_a, inst_b [V,H,W] i32, valid_a, valid_b [V,H,W] u8, n_a, n_b lists).  ``junk``: a twentieth of the pixels carry
    values that belong to no part - n_parts itself, INT32_MIN, large positives"""
    rng = np.random.RandomState(seed)
    out = {"n_a": list(n_a), "n_b": list(n_b)}
    for side, ns in (("a", n_a), ("b", n_b)):
        inst = np.stack([blocky_map(rng, H, W, ns[v]) for v in range(V)]) if V else np.zeros((0, H, W), np.int32)
        if junk:
            for v in range(V):
                bad = rng.rand(H, W) < 0.05
                inst[v][bad] = rng.choice([ns[v], ns[v] + 1, INT32_MIN, 2 ** 31 - 1, -2], size=int(bad.sum()))
        out["inst_" + side] = inst.astype(np.int32)
        out["valid_" + side] = (rng.rand(V, H, W) < valid_rate).astype(np.uint8)
    return out


def class_lists(seed, ns, n_classes=3):
    rng = np.random.RandomState(seed)
    return [rng.randint(1, 1 + n_classes, size=n).astype(np.int64) for n in ns]


def whole_picks(sizes1, sizes2, K):
    """the ``picks`` of ``estimate_joints`` that take the first min(n, K) rows of every cloud in order (torch tensors), and seeded
    RANSAC draws [B, 32, 5] over the rows both sides have"""
    import torch
    B = len(sizes1)
    picks, k = np.zeros((2, B, K), np.int64), np.zeros((2, B), np.int32)
    for side, sizes in enumerate((sizes1, sizes2)):
        for b, n in enumerate(sizes):
            k[side, b] = min(int(n), K)
            picks[side, b, :k[side, b]] = np.arange(k[side, b])
    rng = np.random.RandomState(7)
    ransac = np.stack([rng.randint(max(int(min(k[0, b], k[1, b])), 2), size=(32, 5)) for b in range(B)]).astype(np.int64)
    return tuple(torch.from_numpy(x) for x in (picks[0], picks[1], k[0], k[1])), torch.from_numpy(ransac)


# ---- the rendered scene --------------------------------------------------------------------------------------------------------
def _rays(H, W, K):
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)


def _rect(rays, origin, along, up, s_range, t_range):
    """a rectangle in the plane through ``origin`` spanned by ``along`` and ``up`` -> (z [H,W], hit [H,W])"""
    normal = np.cross(along, up)
    with np.errstate(all="ignore"):
        z = (origin @ normal) / (rays @ normal)
    pts = rays * z[..., None]
    s, t = (pts - origin) @ along, (pts - origin) @ up
    return z, (z > 0) & (s >= s_range[0]) & (s <= s_range[1]) & (t >= t_range[0]) & (t <= t_range[1])


def cabinet_scene(H=48, W=64, door_deg=24.0, drawer_move=0.08):
    """two frames of one static camera: a body plane at z = 1.6; a door slab (0.5 x 0.36, hinge at (-0.25, 0, 1.2) along y, at 8
    degrees, then turned by ``door_deg``: the slab of the joint tests, restated); a drawer front (0.6 x 0.15 at z = 1.3) moved
    ``drawer_move`` towards the camera; a fixed handle on the body (z = 1.5).  The nearest surface wins a pixel.
    -> dict: depth_a, depth_b [H,W] f32; inst_a, inst_b [H,W] i32 (-1 = body); classes_a, classes_b; K [3,3]; partner = {i: j};
    door = (axis, hinge, angle in radians); parts in frame A: 0 door, 1 drawer, 2 handle; frame B numbers them 2, 0, 1."""
    K = np.array([[38.0, 0.0, (W - 1) / 2.0], [0.0, 38.0, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    rays = _rays(H, W, K)
    hinge, axis = np.array([-0.25, 0.0, 1.2]), np.array([0.0, 1.0, 0.0])
    ex, ey = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    perm = {0: 2, 1: 0, 2: 1}
    out = {"K": K, "partner": perm, "door": (axis, hinge, np.deg2rad(door_deg)), "drawer_move": drawer_move}
    for side, a, dz in (("a", np.deg2rad(8.0), 0.0), ("b", np.deg2rad(8.0 + door_deg), -drawer_move)):
        surfaces = [(-1,) + _rect(rays, np.array([0.0, 0.0, 1.6]), ex, ey, (-10, 10), (-10, 10)),
                    (0,) + _rect(rays, hinge, np.array([np.cos(a), 0.0, np.sin(a)]), axis, (0.0, 0.5), (-0.18, 0.18)),
                    (1,) + _rect(rays, np.array([0.0, 0.0, 1.3 + dz]), ex, ey, (-0.3, 0.3), (0.3, 0.45)),
                    (2,) + _rect(rays, np.array([0.0, 0.0, 1.5]), ex, ey, (0.45, 0.6), (-0.3, 0.0))]
        depth, inst = np.full((H, W), np.inf), np.full((H, W), -1, np.int32)
        for part, z, hit in surfaces:
            win = hit & (z < depth)
            depth[win], inst[win] = z[win], part
        if side == "b":
            inst = np.where(inst >= 0, np.vectorize(lambda p: perm.get(p, -1))(inst), -1).astype(np.int32)
        out["depth_" + side], out["inst_" + side] = depth.astype(np.float32), inst
    out["classes_a"] = np.array([DOOR, DRAWER, HANDLE], np.int64)
    out["classes_b"] = np.array([DRAWER, HANDLE, DOOR], np.int64)   # (frame B's part j is frame A's part i with perm[i] == j)
    return out
