"""An independent restatement of the octree-cell sampler's contract (include/gpn.h section GS): a plain loop over the points, a dict
of cells per level, Python ints for the hash, no sort of the cloud and no code shared with the package."""
import math

import numpy as np

M32 = 0xffffffff


def mix(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def hq(v, seed, hash_bits):
    return mix(mix((v + seed * 0x9E3779B9) & M32) ^ seed) >> (32 - hash_bits)


def codes(xyz):
    """the 30-bit Morton code of every row of xyz [n, 3] float32, as Python ints"""
    f32 = np.float32
    n = len(xyz)
    lo = [min(xyz[j][a] for j in range(n)) for a in range(3)]
    hi = [max(xyz[j][a] for j in range(n)) for a in range(3)]
    with np.errstate(all="ignore"):
        e = max(f32(hi[a]) - f32(lo[a]) for a in range(3))
        out = []
        flat = not (e > 0 and math.isfinite(float(e)))
        s = f32(0) if flat else f32(1024.0 / float(e))
        for j in range(n):
            code = 0
            for a in range(3):
                q = 0
                if not flat:
                    x = (f32(xyz[j][a]) - f32(lo[a])) * s
                    q = int(x) if x < f32(1023.0) else 1023
                for i in range(10):
                    code |= ((q >> i) & 1) << (3 * i + a)
            out.append(code)
    return out


def grid_sample(xyz, m, seed=0, hash_bits=32):
    """-> (the m chosen rows ascending as a list, L*); n <= m: (every row, -1)"""
    xyz = np.asarray(xyz, dtype=np.float32)
    n, seed = len(xyz), int(seed) & M32
    if n <= m:
        return list(range(n)), -1
    code = codes(xyz)
    # per level: cell -> the smallest key (code << 32 | row) among its points
    best = [dict() for _ in range(11)]
    for j in range(n):
        key = (code[j] << 32) | j
        for L in range(11):
            cell = code[j] >> (30 - 3 * L)
            if cell not in best[L] or key < best[L][cell]:
                best[L][cell] = key
    L = max(l for l in range(11) if len(best[l]) <= m)
    chosen = {key & M32 for key in best[L].values()}
    r = m - len(chosen)
    if r > 0:
        if L < 10:
            taken = {code[j] >> (30 - 3 * (L + 1)) for j in chosen}
            cand = sorted((hq(cell, seed, hash_bits) << 32) | cell for cell in best[L + 1] if cell not in taken)
            assert len(cand) > r
            chosen |= {best[L + 1][k & M32] & M32 for k in cand[:r]}
        else:
            cand = sorted((hq(j, seed, hash_bits) << 32) | j for j in range(n) if j not in chosen)
            chosen |= {k & M32 for k in cand[:r]}
    assert len(chosen) == m
    return sorted(chosen), L


# ---------------------------------------------------------------------------------------------------- the cases both test files share
def level_cloud(rng, L, cells=6, per_cell=8):
    """a cloud in [0, 1]^3 (both corners present) whose points fill `cells` cells of level L, `per_cell` points each: with
    cells + 2 <= m < C_{L+1} the sampler stops at L* = L"""
    side = 1 << L
    pick = rng.randint(0, side, size=(cells, 3))
    pts = (np.repeat(pick, per_cell, 0) + rng.rand(cells * per_cell, 3)) / side
    return np.concatenate([[[0, 0, 0], [1, 1, 1]], pts]).astype(np.float32)


def families(rng):
    """the degenerate families: name -> (xyz, m)"""
    dup = np.repeat(rng.randn(12, 3).astype(np.float32), 5, 0)[rng.permutation(60)]
    lattice = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 256  # borders at 256 k
    line = np.outer(rng.rand(90), [1.0, -2.0, 0.5]).astype(np.float32)
    plane = rng.randn(120, 3).astype(np.float32)
    plane[:, 1] = 0.25
    far = rng.randn(80, 3).astype(np.float32)
    far[17] = [4e4, -3e4, 1e4]
    huge = rng.randn(40, 3).astype(np.float32)
    huge[3, 0], huge[9, 0] = 3e38, -3e38                       # the extent overflows fp32
    tiny = np.zeros((30, 3), np.float32)
    tiny[::2, 2] = 1e-44                                       # 1024 / e overflows fp32: 0 * inf on the rows at the minimum
    return {"duplicates_L10": (dup, 20), "duplicates_fill": (dup, 47), "all_equal": (np.tile(rng.randn(1, 3).astype(np.float32), (25, 1)), 9),
            "lattice": (lattice, 40), "line": (line, 33), "plane": (plane, 50), "outlier": (far, 30), "overflow": (huge, 11),
            "tiny_extent": (tiny, 7)}
