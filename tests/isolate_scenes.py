"""Seeded synthetic RGB-D frames for the object-isolation tests (include/gpn.h section OB): a tilted table, optionally a wall behind
it, a sphere standing on the table; millimetre noise, holes (zero, NaN, negative depth) and a band of flying pixels along the
sphere's silhouette.  Every scene comes with its generating planes and its object mask.  Units are metres."""
import numpy as np

TILE = 16  # the tile of gpn_frame_components
# sigma of the depth noise: half of CFG's tol, so the inlier counts of good hypotheses differ and the round has ONE winner
NOISE = 0.0025

# what the tests run the pipeline with.  At 64 pixels across, one pixel step on the sphere's flank is centimetres of depth, so the
# absolute jump is wider than the default that suits a VGA frame; the flying pixels are placed well beyond it.
CFG = dict(max_planes=1, n_hyp=256, tol=0.005, min_plane_fraction=0.1, jump_abs=0.04, jump_rel=0.01, min_pixels=6)


def camera(H, W):
    f = 1.6 * max(W, 8)
    return np.array([[f, 0.0, (W - 1) / 2.0 + 0.25], [0.0, f, (H - 1) / 2.0 - 0.25], [0.0, 0.0, 1.0]])


def table_plane(tilt_deg=40.0):
    t = np.deg2rad(tilt_deg)
    n = np.array([0.0, -np.cos(t), -np.sin(t)])
    return np.concatenate([n, [-(n @ np.array([0.0, 0.1, 1.0]))]])  # through (0, 0.1, 1), the camera on the positive side


def make_scene(H, W, seed=0, wall=False, noise=NOISE, holes=0.05, flying=True, radius=0.1, tilt_deg=40.0, sphere=True):
    """-> dict(depth [H,W] f32, rgb [H,W,3] u8, K [3,3], table [4], wall [4] or None, object [H,W] bool, height [H,W] = the true
    height of the seen surface above the table, on_table [H,W] bool = pixels that show the table)"""
    rng = np.random.default_rng(seed)
    K = camera(H, W)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], -1)
    table = table_plane(tilt_deg)
    with np.errstate(divide="ignore", invalid="ignore"):
        zt = -table[3] / (ray @ table[:3])
    zt = np.where(zt > 0, zt, np.inf)
    depth, kind = zt.copy(), np.zeros((H, W), dtype=np.int8)  # kind: 0 table, 1 wall, 2 object
    wall_plane = None
    if wall:
        t = np.deg2rad(tilt_deg)  # at a right angle to the table, so the band of wall pixels within tol of the table is thin
        wall_plane = np.array([0.0, np.sin(t), -np.cos(t), np.cos(t) * 1.3])
        with np.errstate(divide="ignore", invalid="ignore"):
            zw = -wall_plane[3] / (ray @ wall_plane[:3])
        zw = np.where(zw > 0, zw, np.inf)
        kind[zw < depth] = 1
        depth = np.minimum(depth, zw)
    obj = np.zeros((H, W), dtype=bool)
    if sphere:
        foot = np.array([0.0, 0.0, -table[3] / table[2]])  # where the optical axis meets the table
        c = foot + table[:3] * radius
        b = ray @ c
        a = (ray * ray).sum(-1)
        disc = b * b - a * (c @ c - radius * radius)
        zs = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
        obj = zs < depth
        depth = np.where(obj, zs, depth)
        kind[obj] = 2
    clean = depth.copy()
    with np.errstate(invalid="ignore"):
        height = (ray * depth[..., None]) @ table[:3] + table[3]
    if flying and sphere and H > 2 and W > 2:
        pad = np.pad(obj, 1, constant_values=False)
        rim = obj & ~(pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:])
        back = np.where(np.isfinite(depth), depth, 2.0)
        mix = rng.uniform(0.35, 0.65, size=(H, W))
        fly = rim & (rng.random((H, W)) < 0.6) & (back - clean > 0.3)
        depth = np.where(fly, clean + mix * (back - clean), depth)
        obj = obj & ~fly
    if noise > 0:
        depth = depth + rng.normal(0.0, noise, size=(H, W))
    depth = np.where(np.isfinite(depth), depth, 0.0).astype(np.float32)
    if holes > 0:
        h = rng.random((H, W))
        depth[h < holes / 3] = 0.0
        depth[(h >= holes / 3) & (h < 2 * holes / 3)] = np.nan
        depth[(h >= 2 * holes / 3) & (h < holes)] = -1.0
        obj = obj & ~(h < holes)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    return dict(depth=depth, rgb=rgb, K=K, table=table, wall=wall_plane, object=obj, height=height, on_table=(kind == 0), seed=seed,
                H=H, W=W)


# (name, H, W, seed, keywords): the frames every exact comparison runs over.  The seeds are chosen so that the conditions of
# tests/test_isolate_cpu.py hold (one winner per round, nothing within 1e-9 of a threshold).
SCENES = [
    ("s48x64", 48, 64, 1, {}),
    ("s61x97", 61, 97, 2, {}),
    ("tile-1", TILE * 3 - 1, TILE * 4 - 1, 3, {}),
    ("tile", TILE * 3, TILE * 4, 4, {}),
    ("tile+1", TILE * 3 + 1, TILE * 4 + 1, 9, {}),
    ("wall", 61, 97, 6, dict(wall=True)),
    ("clean", 48, 64, 7, dict(noise=0.0, holes=0.0, flying=False)),
]
THIN = [("1x1", 1, 1, 11, {}), ("1xW", 1, 70, 12, {}), ("Hx1", 70, 1, 13, {})]


def scene(name):
    for n, H, W, seed, kw in SCENES + THIN:
        if n == name:
            return make_scene(H, W, seed, **kw)
    raise KeyError(name)


def all_invalid(H=20, W=33):
    s = make_scene(H, W, 21)
    s["depth"] = np.zeros((H, W), dtype=np.float32)
    s["object"][:] = False
    return s


def two_valid(H=20, W=33):
    s = all_invalid(H, W)
    s["depth"][3, 4] = 1.0
    s["depth"][3, 5] = 1.001
    return s


def no_plane(H=48, W=64, seed=31):
    """a frame without a plane: the sphere alone (the table and everything else is a hole)"""
    s = make_scene(H, W, seed, noise=0.0, holes=0.0, flying=False)
    s["depth"] = np.where(s["object"], s["depth"], 0.0).astype(np.float32)
    return s
