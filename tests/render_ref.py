"""A plain restatement of include/gpn.h section RD, one triangle and one pixel at a time, written independently of the package's
vectorised numpy path (gapartnet_amd/dataset/render_assets.render_tables_numpy) and of the kernels (csrc/render.hip).

Python ints are exact integers (the int64 edge functions cannot overflow here) and Python floats are IEEE float64 evaluated one
operation at a time, so every expression below has the operation order the header writes down, without contraction.
``round`` on a float is round-half-to-even, as ``rint``.  Inputs are the geometry and view tables of section RD as numpy arrays
(``geometry_tables`` / ``view_tables`` build them from assets; the GPU tests also build them by hand).
"""
import atexit
import math
import os
import shutil
import tempfile
import zipfile

import numpy as np

NEAR = 0.1
GUARD = 16384 * 256
N_COUNTERS = 5
IDX, NEAR_C, GUARD_C, ZERO, OFF = range(5)


_UNPACKED = {}


def fixture_asset(name="45780"):
    """the mesh fixture tests/golden/assets/<name>.zip (the asset's URDF, annotation, OBJ and MTL files as shipped, in one archive
    so that 108 mesh files are not 13 000 lines of history) unpacked into a temporary directory, once per process -> its path"""
    if name not in _UNPACKED:
        tmp, owner = tempfile.mkdtemp(prefix="gpn_asset_"), os.getpid()
        with zipfile.ZipFile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assets", name + ".zip")) as z:
            z.extractall(tmp)
        atexit.register(lambda: os.getpid() == owner and shutil.rmtree(tmp, ignore_errors=True))
        _UNPACKED[name] = os.path.join(tmp, name)
    return _UNPACKED[name]


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def owns(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return dy < 0 or (dy == 0 and dx > 0)


def span(g, t, v):
    A, Nt = len(g['assets']), len(g['tris'])
    a = int(t['view_asset'][v])
    if not 0 <= a < A:
        return 0, 0, 0, 0
    first, count, nvis, nlinks = (int(x) for x in g['assets'][a])
    if first < 0 or count < 0 or first > Nt or count > Nt - first:
        count = 0
    return first, min(count, int(t['Nt_max'])), nvis, nlinks


def setup_triangle(g, t, v, k, first, nvis):
    """-> (counter index, None) for a dropped triangle, (None, record) otherwise"""
    H, W = int(t['H']), int(t['W'])
    M, Nv = t['vis_mat'].shape[1], len(g['verts'])
    tri = [int(i) for i in g['tris'][first + k]]
    vis = int(g['tri_visual'][first + k])
    if vis < 0 or vis >= M or vis >= nvis or any(i < 0 or i >= Nv for i in tri):
        return IDX, None
    cam = [float(c) for c in t['cam'][v]]
    fx, fy, cx, cy = cam[:4]
    m = [float(c) for c in t['vis_mat'][v, vis]]
    P = []
    for i in tri:
        x, y, z = (float(c) for c in g['verts'][i])  # float32 -> float64, exact
        P.append([((m[r * 4] * x + m[r * 4 + 1] * y) + m[r * 4 + 2] * z) + m[r * 4 + 3] for r in range(3)])
    if not all(p[2] >= NEAR for p in P):
        return NEAR_C, None
    X, Y = [], []
    for p in P:
        u = (fx * p[0]) / p[2] + cx
        w = (fy * p[1]) / p[2] + cy
        su, sv = u * 256.0, w * 256.0
        if not (math.isfinite(su) and math.isfinite(sv) and abs(round(su)) <= GUARD and abs(round(sv)) <= GUARD):
            return GUARD_C, None
        X.append(int(round(su)))
        Y.append(int(round(sv)))
    area2 = edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
    if area2 == 0:
        return ZERO, None
    o = [0, 1, 2] if area2 > 0 else [0, 2, 1]
    e1 = [P[1][c] - P[0][c] for c in range(3)]
    e2 = [P[2][c] - P[0][c] for c in range(3)]
    nx = e1[1] * e2[2] - e1[2] * e2[1]
    ny = e1[2] * e2[0] - e1[0] * e2[2]
    nz = e1[0] * e2[1] - e1[1] * e2[0]
    nn = math.sqrt((nx * nx + ny * ny) + nz * nz)
    d = (nx * cam[16] + ny * cam[17]) + nz * cam[18]
    shade = 0.5 + 0.5 * (abs(d) / nn) if nn > 0.0 else 0.5
    x0, x1 = max(-((-min(X)) // 256), 0), min(max(X) // 256, W - 1)
    y0, y1 = max(-((-min(Y)) // 256), 0), min(max(Y) // 256, H - 1)
    if x0 > x1 or y0 > y1:
        return OFF, None
    return None, dict(x=[X[i] for i in o], y=[Y[i] for i in o], iz=[1.0 / P[i][2] for i in o], shade=shade, box=(x0, y0, x1, y1))


def render(g, t):
    """-> dict(depth, tri, sem, ins, npcs, rgb, link_area, link_inst, counters) for all views"""
    V, H, W = len(t['view_asset']), int(t['H']), int(t['W'])
    L = t['link_cat'].shape[1]
    bg = t.get('background', (0, 0, 0))
    out = dict(depth=np.zeros((V, H, W), np.float32), tri=np.full((V, H, W), -1, np.int32), sem=np.zeros((V, H, W), np.int32),
               ins=np.zeros((V, H, W), np.int32), npcs=np.zeros((V, H, W, 3), np.float32), rgb=np.zeros((V, H, W, 3), np.uint8),
               link_area=np.zeros((V, L), np.int32), link_inst=np.full((V, L), -1, np.int32),
               counters=np.zeros((V, N_COUNTERS), np.int32))
    for v in range(V):
        first, count, nvis, nlinks = span(g, t, v)
        best = [[0.0] * W for _ in range(H)]
        win = [[-1] * W for _ in range(H)]
        shade = {}
        for k in range(count):
            why, r = setup_triangle(g, t, v, k, first, nvis)
            if r is None:
                out['counters'][v, why] += 1
                continue
            shade[k] = r['shade']
            x, y, iz = r['x'], r['y'], r['iz']
            own = [owns(x[1], y[1], x[2], y[2]), owns(x[2], y[2], x[0], y[0]), owns(x[0], y[0], x[1], y[1])]
            x0, y0, x1, y1 = r['box']
            for py in range(y0, y1 + 1):
                for px in range(x0, x1 + 1):
                    sx, sy = px * 256, py * 256
                    e = [edge(x[1], y[1], x[2], y[2], sx, sy), edge(x[2], y[2], x[0], y[0], sx, sy),
                         edge(x[0], y[0], x[1], y[1], sx, sy)]
                    if any(ei < 0 or (ei == 0 and not oi) for ei, oi in zip(e, own)):
                        continue
                    a2 = float((e[0] + e[1]) + e[2])
                    l0, l1, l2 = float(e[0]) / a2, float(e[1]) / a2, float(e[2]) / a2
                    invz = (l0 * iz[0] + l1 * iz[1]) + l2 * iz[2]
                    if invz > best[py][px]:  # ascending k: a tie stays with the lower triangle
                        best[py][px] = invz
                        win[py][px] = k
        cam = [float(c) for c in t['cam'][v]]
        fx, fy, cx, cy = cam[:4]
        R, tt = cam[4:13], cam[13:16]
        cat, rank = t['link_cat'][v], t['link_rank'][v]
        links = min(nlinks, L)

        def link_of(k):
            if k < 0:
                return -1
            l = int(g['tri_link'][first + k])
            return l if 0 <= l < links else -1

        for py in range(H):
            for px in range(W):
                l = link_of(win[py][px])
                if l >= 0:
                    out['link_area'][v, l] += 1
        cnt = 0
        for r in range(L):
            for l in range(L):
                if int(rank[l]) == r and int(cat[l]) >= 0 and out['link_area'][v, l] > 0:
                    out['link_inst'][v, l] = cnt
                    cnt += 1
        for py in range(H):
            for px in range(W):
                k = win[py][px]
                depth = np.float32(1.0 / best[py][px]) if k >= 0 else np.float32(0.0)
                out['depth'][v, py, px] = depth
                out['tri'][v, py, px] = first + k if k >= 0 else -1
                l = link_of(k)
                s = i = -1
                if l >= 0 and int(cat[l]) >= 0 and int(out['link_inst'][v, l]) >= 0:
                    s, i = int(cat[l]), int(out['link_inst'][v, l])
                if abs(float(depth)) < float(np.float32(1e-6)):
                    s = i = -2
                out['sem'][v, py, px], out['ins'][v, py, px] = s, i
                if i >= 0:
                    z = float(depth)
                    pc = [((float(px) - cx) * z) / fx, ((float(py) - cy) * z) / fy, z]
                    f = [float(c) for c in t['link_frame'][v, l]]
                    gq = [((((pc[0] * R[r * 3] + pc[1] * R[r * 3 + 1]) + pc[2] * R[r * 3 + 2]) + tt[r]) - f[r]) / f[3] for r in range(3)]
                    for r in range(3):
                        out['npcs'][v, py, px, r] = np.float32((gq[0] * f[4 + r * 3] + gq[1] * f[5 + r * 3]) + gq[2] * f[6 + r * 3])
                if k >= 0:
                    for r in range(3):
                        val = round((float(g['tri_color'][first + k, r]) * shade[k]) * 255.0)
                        out['rgb'][v, py, px, r] = min(max(val, 0), 255)
                else:
                    out['rgb'][v, py, px] = bg
    return out


# ---- small hand-made scenes for the kernel tests ---------------------------------------------------------------------------
def identity_views(V, H, W, links=1, M=1, f=None, view_asset=None, Nt_max=0, background=(7, 8, 9)):
    """view tables whose camera and visuals are the identity: vertices are camera-space points.  fx = fy = f, cx = cy = 0."""
    f = float(f if f is not None else 1.0)
    cam = np.zeros((V, 20))
    cam[:, 0] = cam[:, 1] = f
    cam[:, 4:13] = np.eye(3).reshape(-1)
    cam[:, 16:19] = np.array([0.0, 1.0, -1.0]) / math.sqrt(2.0)
    vis = np.zeros((V, M, 12))
    vis[:, :, [0, 5, 10]] = 1.0
    frame = np.zeros((V, links, 13))
    frame[:, :, 3] = 1.0
    frame[:, :, 4:] = np.eye(3).reshape(-1)
    return dict(view_asset=np.zeros(V, np.int32) if view_asset is None else np.asarray(view_asset, np.int32), cam=cam, vis_mat=vis,
                link_cat=np.zeros((V, links), np.int32), link_rank=np.tile(np.arange(links, dtype=np.int32), (V, 1)),
                link_frame=frame, Nt_max=int(Nt_max), H=int(H), W=int(W), background=tuple(background))


def soup(tris_xyz, links=None, colors=None):
    """geometry tables of one asset from a list of triangles given as three camera-space points each"""
    tris_xyz = np.asarray(tris_xyz, np.float32).reshape(-1, 3, 3)
    n = len(tris_xyz)
    links = np.zeros(n, np.int32) if links is None else np.asarray(links, np.int32)
    colors = np.full((n, 3), 0.8, np.float32) if colors is None else np.asarray(colors, np.float32)
    return dict(verts=tris_xyz.reshape(-1, 3).copy(), tris=np.arange(3 * n, dtype=np.int32).reshape(n, 3),
                tri_visual=np.zeros(n, np.int32), tri_link=links, tri_color=colors,
                assets=np.array([[0, n, 1, int(links.max()) + 1 if n else 1]], np.int32))


def merge(geoms):
    """several one-asset geometry tables -> one asset set"""
    v0 = t0 = 0
    parts = {k: [] for k in ('verts', 'tris', 'tri_visual', 'tri_link', 'tri_color', 'assets')}
    for g in geoms:
        parts['verts'].append(g['verts'])
        parts['tris'].append(g['tris'] + v0)
        for k in ('tri_visual', 'tri_link', 'tri_color'):
            parts[k].append(g[k])
        a = g['assets'].copy()
        a[:, 0] += t0
        parts['assets'].append(a)
        v0 += len(g['verts'])
        t0 += len(g['tris'])
    return {k: np.concatenate(p) for k, p in parts.items()}
