"""numpy restatement of include/gpn.h section FR (RGB-D frames -> rows, the seeded presample, the packed layout) and of the frame
overlay, the oracle of tests/test_frames_cpu.py and tests/test_gpu_frameprep.py.  It is checked itself against
tests/golden/frames_backproject.npz, what the reference's get_point_cloud and draw_bbox produced
(tests/golden/make_golden_frames.py).  The overlay is the line rule of tests/visu_ref.py with the frame's own camera."""
import numpy as np

from tests import visu_ref as VR

OK, FEW, EMPTY, DEGENERATE = 0, 1, 2, 3
M32 = 0xffffffff


def backproject(depth, rgb, K, keep=None, depth_scale=1.0, flip=False):
    """one frame: depth [H,W], rgb [H,W,3] u8, K [3,3] -> (rows [H*W, 6] f32, valid [H*W] bool), pixel by pixel in python floats
    (IEEE float64, the order of the header)"""
    H, W = depth.shape
    K = np.asarray(K, dtype=np.float64)
    rows = np.empty((H * W, 6), np.float32)
    valid = np.zeros(H * W, bool)
    with np.errstate(all="ignore"):
        for v in range(H):
            for u in range(W):
                p = v * W + u
                z = np.float64(depth[v, u]) / np.float64(depth_scale)
                ok = bool(np.isfinite(z)) and z > 0 and (keep is None or keep[v, u] != 0)
                xyz = np.full(3, np.nan, np.float32)
                if ok:
                    x = ((np.float64(u) - K[0, 2]) * z) / K[0, 0]
                    y = ((np.float64(v) - K[1, 2]) * z) / K[1, 1]
                    xyz = np.asarray([x, y, z], np.float64).astype(np.float32)
                    ok = bool(np.isfinite(xyz).all())
                    if flip:
                        xyz[1:] = -xyz[1:]
                    if not ok:
                        xyz[:] = np.nan
                rows[p, :3] = xyz
                rows[p, 3:] = (rgb[v, u].astype(np.float64) / 255.0).astype(np.float32)
                valid[p] = ok
    return rows, valid


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def hash_pixel(seed, pixel, hash_bits=32):
    """python integers: mix(mix(pixel + seed * 0x9E3779B9) ^ seed) >> (32 - hash_bits)"""
    seed &= M32
    return mix(mix((pixel + seed * 0x9E3779B9) & M32) ^ seed) >> (32 - hash_bits)


def keys(seed, pixels, hash_bits=32):
    return np.asarray([(hash_pixel(int(seed), int(p), hash_bits) << 32) | int(p) for p in pixels], dtype=np.uint64)


def select(valid, seed, cap, hash_bits=32):
    """the kept pixels, ascending: the cap smallest keys among the valid pixels (np.argpartition), all of them when there are at
    most cap or cap == 0"""
    pix = np.nonzero(valid)[0].astype(np.int64)
    if cap <= 0 or pix.shape[0] <= cap:
        return pix
    k = keys(seed, pix, hash_bits)
    return np.sort(pix[np.argpartition(k, cap - 1)[:cap]])


def pack(rows, kept, n_bound):
    """the layout gpn_cloud_pack writes for one frame: packed [n_bound, 4] (NaN past the count), pix, count, status"""
    packed = np.full((n_bound, 4), np.nan, np.float32)
    packed[:kept.shape[0], :3] = rows[kept, :3]
    packed[:kept.shape[0], 3] = np.float32(1e10)
    return packed, kept.astype(np.int32), kept.shape[0], (OK if kept.shape[0] else EMPTY)


def masked_rows(rows, kept):
    """the frame's rows with the xyz of every pixel that was not kept set to NaN: the cloud whose ``prepare_clouds`` equals the
    frame's ``prepare_frames``"""
    out = rows.copy()
    drop = np.ones(rows.shape[0], bool)
    drop[kept] = False
    out[drop, :3] = np.nan
    return out


def corners_px(bbox, K):
    """[Q,8,2] f64: structure/utils.py:70-71 (= the projection of section VS with trans (1, 0, 0, 0))"""
    K = np.asarray(K, dtype=np.float64)
    return VR.box_corners(bbox, (1.0, 0.0, 0.0, 0.0), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def overlay(rgb, bbox, K):
    """[H,W,3] u8: the image with every box drawn, box by box and draw by draw"""
    K = np.asarray(K, dtype=np.float64)
    return VR.draw_boxes(np.array(rgb, dtype=np.uint8, copy=True), np.asarray(bbox, np.float64).reshape(-1, 8, 3), (1.0, 0.0, 0.0, 0.0),
                         (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def synthetic_frames(V, H, W, seed=0, hole=0.4):
    """depth f32 [V,H,W] in metres with a fraction of zero holes, rgb u8, K [V,3,3] with a different non-square camera per frame"""
    rng = np.random.RandomState(seed)
    depth = (0.5 + rng.rand(V, H, W) * 2).astype(np.float32)
    depth[rng.rand(V, H, W) < hole] = 0
    rgb = rng.randint(0, 256, size=(V, H, W, 3)).astype(np.uint8)
    K = np.zeros((V, 3, 3))
    for v in range(V):
        K[v] = [[W * (1.1 + 0.1 * v), 0, W / 2 - 0.5 + 0.25 * v], [0, W * (1.3 + 0.05 * v), H / 2 - 0.25 * v], [0, 0, 1]]
    return depth, rgb, K


def frames_from_clouds(clouds, H, W):
    """raw camera-frame clouds [n, 6] (xyz + rgb in [0, 1]) seen by a pinhole camera that holds each of them: per cloud a z-buffered
    depth map f32 [H,W] (0 where no point lands), the image u8 and K - frames whose back-projection has the clouds' structure"""
    depth = np.zeros((len(clouds), H, W), np.float32)
    rgb = np.zeros((len(clouds), H, W, 3), np.uint8)
    K = np.zeros((len(clouds), 3, 3))
    for s, c in enumerate(clouds):
        c = np.asarray(c, dtype=np.float64)
        ext = np.abs(c[:, :2] / c[:, 2:3]).max(0)            # the tangents the camera has to cover
        fx, fy = (W / 2 - 1) / ext[0], (H / 2 - 1) / ext[1]
        K[s] = [[fx, 0, W / 2 - 0.5], [0, fy, H / 2 - 0.5], [0, 0, 1]]
        u = np.rint(c[:, 0] * fx / c[:, 2] + K[s, 0, 2]).astype(np.int64)
        v = np.rint(c[:, 1] * fy / c[:, 2] + K[s, 1, 2]).astype(np.int64)
        for j in np.argsort(-c[:, 2]):                        # far to near: the nearest point of a pixel stays
            depth[s, v[j], u[j]] = c[j, 2]
            rgb[s, v[j], u[j]] = np.clip(np.rint(c[j, 3:6] * 255), 0, 255)
    return depth, rgb, K


# ---------------------------------------------------------------------------------------------------- array forms (large frames)
def backproject_np(depth, rgb, K, keep=None, depth_scale=1.0, flip=False):
    """``backproject`` on whole arrays (tests/test_frames_cpu.py holds it against the pixel loop)"""
    H, W = depth.shape
    K = np.asarray(K, dtype=np.float64)
    with np.errstate(all="ignore"):
        z = depth.astype(np.float64) / np.float64(depth_scale)
        valid = np.isfinite(z) & (z > 0)
        if keep is not None:
            valid &= keep != 0
        u, v = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
        xyz = np.stack([((u - K[0, 2]) * z) / K[0, 0], ((v - K[1, 2]) * z) / K[1, 1], z], -1).astype(np.float32)
    valid &= np.isfinite(xyz).all(-1)
    if flip:
        xyz[..., 1:] = -xyz[..., 1:]
    xyz[~valid] = np.nan
    col = (rgb.astype(np.float64) / 255.0).astype(np.float32)
    return np.concatenate([xyz, col], -1).reshape(H * W, 6), valid.reshape(-1)


def hash_np(seed, pixels, hash_bits=32):
    """``hash_pixel`` on an array, in uint64 arithmetic masked to 32 bits (no wrap-around is relied on)"""
    m = np.uint64(M32)

    def mix_np(x):
        x = x ^ (x >> np.uint64(16))
        x = (x * np.uint64(0x7feb352d)) & m
        x = x ^ (x >> np.uint64(15))
        x = (x * np.uint64(0x846ca68b)) & m
        return x ^ (x >> np.uint64(16))

    seed = np.uint64(int(seed) & M32)
    x = (np.asarray(pixels).astype(np.uint64) + ((seed * np.uint64(0x9E3779B9)) & m)) & m
    return mix_np(mix_np(x) ^ seed) >> np.uint64(32 - hash_bits)


def select_np(valid, seed, cap, hash_bits=32):
    """``select`` with the array hash"""
    pix = np.nonzero(valid)[0].astype(np.int64)
    if cap <= 0 or pix.shape[0] <= cap:
        return pix
    k = (hash_np(seed, pix, hash_bits) << np.uint64(32)) | pix.astype(np.uint64)
    return np.sort(pix[np.argpartition(k, cap - 1)[:cap]])
