"""A plain restatement of include/gpn.h section RS (textured, lit RGB), one pixel at a time, written from the contract and not from
the package's vectorised path (render_assets.shade_tables_numpy) or the kernel (csrc/render.hip, rs_shade_kernel).

Python floats are IEEE float64 evaluated one operation at a time and Python ints are exact, so every expression has the operation
order the header writes down.  ``round`` is round-half-to-even, as ``rint``.  The winning triangle and the depth of a pixel are
inputs (tests/render_ref.render produces them; on the GPU the raster kernel does).
"""
import math

import numpy as np

from tests import render_ref as RR

AMBIENT, DIRECTIONAL, POINT = 0, 1, 2


def light_table(V, rows):
    """rows of (kind, (x, y, z), (r, g, b)) in the camera frame -> lights [V,NL,8], the same rows for every view"""
    t = np.zeros((V, len(rows), 8))
    for i, (kind, xyz, rgb) in enumerate(rows):
        t[:, i, 0], t[:, i, 1:4], t[:, i, 4:7] = kind, xyz, rgb
    return t


def add_textures(g, images, tri_tex, tri_uv):
    """geometry tables plus the section-RS tables: images [h,w,3] u8 each, tri_tex [Nt], tri_uv [Nt,3,2]"""
    g = dict(g)
    rows, first = [], 0
    for img in images:
        rows.append([first, img.shape[1], img.shape[0], 0])
        first += img.shape[0] * img.shape[1]
    data = np.full((first, 4), 255, np.uint8)
    if images:
        data[:, :3] = np.concatenate([np.asarray(i, np.uint8).reshape(-1, 3) for i in images])
    g.update(tri_uv=np.asarray(tri_uv, np.float32).reshape(-1, 3, 2), tri_tex=np.asarray(tri_tex, np.int32).reshape(-1),
             tex_table=np.asarray(rows, np.int32).reshape(-1, 4), tex_data=data)
    return g


def camera_corners(g, t, v, tri, nvis):
    """P[3] in camera space (parsed order) and the snapped screen corners, as the setup step of section RD computes them"""
    M, Nv = t['vis_mat'].shape[1], len(g['verts'])
    idx = [int(i) for i in g['tris'][tri]]
    vis = int(g['tri_visual'][tri])
    if vis < 0 or vis >= M or vis >= nvis or any(i < 0 or i >= Nv for i in idx):
        return None
    cam = [float(c) for c in t['cam'][v]]
    fx, fy, cx, cy = cam[:4]
    m = [float(c) for c in t['vis_mat'][v, vis]]
    P, X, Y = [], [], []
    for i in idx:
        x, y, z = (float(c) for c in g['verts'][i])
        P.append([((m[r * 4] * x + m[r * 4 + 1] * y) + m[r * 4 + 2] * z) + m[r * 4 + 3] for r in range(3)])
    if not all(p[2] >= RR.NEAR for p in P):
        return None
    for p in P:
        su, sv = ((fx * p[0]) / p[2] + cx) * 256.0, ((fy * p[1]) / p[2] + cy) * 256.0
        if not (math.isfinite(su) and math.isfinite(sv) and abs(round(su)) <= RR.GUARD and abs(round(sv)) <= RR.GUARD):
            return None
        X.append(int(round(su)))
        Y.append(int(round(sv)))
    return P, X, Y


def sample(image_rows, w, h, u, v):
    """bilinear, wrapping sample of one texture; image_rows(k, i) -> (r, g, b) of row k, column i.  -> three floats in 0 ... 255"""
    uu = u - math.floor(u)
    f = 1.0 - v
    vv = f - math.floor(f)
    X, Y = uu * float(w) - 0.5, vv * float(h) - 0.5
    i, k = math.floor(X), math.floor(Y)
    fx, fy = X - i, Y - k
    a00, a01 = image_rows(k % h, i % w), image_rows(k % h, (i + 1) % w)
    a10, a11 = image_rows((k + 1) % h, i % w), image_rows((k + 1) % h, (i + 1) % w)
    return [(float(a00[c]) * (1.0 - fx) + float(a01[c]) * fx) * (1.0 - fy) + (float(a10[c]) * (1.0 - fx) + float(a11[c]) * fx) * fy
            for c in range(3)]


def barycentrics(P, X, Y, px, py, affine=False):
    """perspective-correct weights of the parsed corners at pixel (px, py); affine: the screen-space weights instead (what a
    renderer without the correction would use - the perspective test shows the two apart)"""
    area2 = RR.edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
    if area2 == 0:
        return None
    o = [0, 1, 2] if area2 > 0 else [0, 2, 1]
    x, y = [X[i] for i in o], [Y[i] for i in o]
    sx, sy = px * 256, py * 256
    e = [RR.edge(x[1], y[1], x[2], y[2], sx, sy), RR.edge(x[2], y[2], x[0], y[0], sx, sy), RR.edge(x[0], y[0], x[1], y[1], sx, sy)]
    a2 = float((e[0] + e[1]) + e[2])
    lam = [float(e[j]) / a2 for j in range(3)]
    if affine:
        w = lam
    else:
        w = [lam[j] * (1.0 / P[o[j]][2]) for j in range(3)]
        s = (w[0] + w[1]) + w[2]
        w = [w[j] / s for j in range(3)]
    b = [0.0, 0.0, 0.0]
    for j in range(3):
        b[o[j]] = w[j]
    return b


def shade_pixel(g, t, v, tri, depth, px, py, nvis, affine=False):
    """-> [r, g, b] ints, or None for the background colour"""
    corners = camera_corners(g, t, v, tri, nvis)
    if corners is None:
        return None
    P, X, Y = corners
    b = barycentrics(P, X, Y, px, py, affine)
    if b is None:
        return None
    alb = [float(g['tri_color'][tri, c]) * 255.0 for c in range(3)]
    T = len(g['tex_table']) if g.get('tex_table') is not None else 0
    if T:
        tx = int(g['tri_tex'][tri])
        uv = [[float(g['tri_uv'][tri, j, c]) for c in range(2)] for j in range(3)]
        if 0 <= tx < T and all(math.isfinite(q) for row in uv for q in row):
            first, w, h = (int(q) for q in g['tex_table'][tx][:3])
            if first >= 0 and w >= 1 and h >= 1 and first + w * h <= len(g['tex_data']):
                u = (b[0] * uv[0][0] + b[1] * uv[1][0]) + b[2] * uv[2][0]
                vv = (b[0] * uv[0][1] + b[1] * uv[1][1]) + b[2] * uv[2][1]
                alb = sample(lambda k, i: g['tex_data'][first + k * w + i], w, h, u, vv)
    e1 = [P[1][c] - P[0][c] for c in range(3)]
    e2 = [P[2][c] - P[0][c] for c in range(3)]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    nn = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    lit = nn > 0.0
    if lit:
        n = [c / nn for c in n]
        if (n[0] * P[0][0] + n[1] * P[0][1]) + n[2] * P[0][2] > 0.0:
            n = [-c for c in n]
    cam = [float(c) for c in t['cam'][v]]
    z = float(depth)
    p = [((float(px) - cam[2]) * z) / cam[0], ((float(py) - cam[3]) * z) / cam[1], z]
    I = [0.0, 0.0, 0.0]
    for row in t['lights'][v]:
        kind, L, col = float(row[0]), [float(c) for c in row[1:4]], [float(c) for c in row[4:7]]
        if kind == 0.0:
            I = [I[c] + col[c] for c in range(3)]
        elif kind == 1.0 and lit:
            nd = (n[0] * L[0] + n[1] * L[1]) + n[2] * L[2]
            m = nd if nd > 0.0 else 0.0
            I = [I[c] + col[c] * m for c in range(3)]
        elif kind == 2.0 and lit:
            D = [L[c] - p[c] for c in range(3)]
            r2 = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
            r = math.sqrt(r2)
            if r > 0.0:
                nd = ((n[0] * D[0] + n[1] * D[1]) + n[2] * D[2]) / r
                m = nd if nd > 0.0 else 0.0
                I = [I[c] + (col[c] * m) / r2 for c in range(3)]
    out = []
    for c in range(3):
        val = alb[c] * I[c]
        val = round(val) if math.isfinite(val) else (255 if val > 0 else 0)
        out.append(min(max(int(val), 0), 255))
    return out


def shade(g, t, tri, depth, affine=False):
    """tri [V,H,W] i32 and depth [V,H,W] f32 of section RD -> rgb [V,H,W,3] u8 of section RS"""
    V, H, W = len(t['view_asset']), int(t['H']), int(t['W'])
    bg = t.get('background', (0, 0, 0))
    rgb = np.zeros((V, H, W, 3), np.uint8)
    for v in range(V):
        first, count, nvis, _ = RR.span(g, t, v)
        for py in range(H):
            for px in range(W):
                k = int(tri[v, py, px])
                col = None
                if first <= k < first + count:
                    col = shade_pixel(g, t, v, k, depth[v, py, px], px, py, nvis, affine)
                rgb[v, py, px] = bg if col is None else col
    return rgb


def render(g, t):
    """sections RD and RS: tests/render_ref.render with its rgb replaced"""
    out = RR.render(g, t)
    out['rgb'] = shade(g, t, out['tri'], out['depth'])
    return out
