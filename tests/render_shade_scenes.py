"""Hand-made scenes for the section-RS tests (CPU and GPU): identity cameras with fx = fy = 16 and cx = cy = 0, so a camera point
(u z / 16, v z / 16, z) lands exactly on pixel position (u, v); small textures with distinct texels; a generated two-link asset with
textures written by PIL."""
import json
import os

import numpy as np

from tests import render_ref as RR
from tests import render_shade_ref as RS

F = 16.0
AMBIENT_ONE = [(RS.AMBIENT, (0, 0, 0), (1, 1, 1))]


def px(pts, z=1.0):
    """pixel positions (u, v) [and a depth each] -> camera-space points"""
    out = []
    for p in pts:
        d = float(p[2]) if len(p) > 2 else float(z)
        out.append([p[0] * d / F, p[1] * d / F, d])
    return out


def texture(w, h, seed=0):
    """[h,w,3] u8 with distinct texels, none 0 or 255"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    return rng.permutation(np.arange(3 * w * h) % 199 + 20).reshape(h, w, 3).astype(np.uint8)


def quad(x0, y0, x1, y1, z=2.0, uv=((0, 1), (1, 1), (1, 0), (0, 0))):
    """two triangles over pixel positions [x0, x1] x [y0, y1]; uv of the corners top-left, top-right, bottom-right, bottom-left
    (default: the whole texture, upright) -> (triangles [2,3,3], uv [2,3,2])"""
    c = px([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], z)
    uv = [list(map(float, q)) for q in uv]
    return [[c[0], c[1], c[2]], [c[0], c[2], c[3]]], [[uv[0], uv[1], uv[2]], [uv[0], uv[2], uv[3]]]


def scene(tris, uvs, tex_ids, images, lights, H, W, colors=None, V=1, links=None, background=(7, 8, 9)):
    """one asset seen by V identical identity views -> (g, t)"""
    g = RR.soup(np.asarray(tris, np.float64).reshape(-1, 3, 3), links=links, colors=colors)
    n = len(g["tris"])
    if images is not None:
        g = RS.add_textures(g, images, tex_ids, uvs)
    t = RR.identity_views(V, H, W, links=int(g["assets"][0, 3]), f=F, Nt_max=n, background=background)
    t["lights"] = RS.light_table(V, lights)
    return g, t


def merge(geoms):
    """several one-asset textured geometry tables -> one asset set (textures rebased)"""
    g = RR.merge(geoms)
    uv, tex, rows, data, n_tex, texels = [], [], [], [], 0, 0
    for q in geoms:
        n = len(q["tris"])
        has = q.get("tex_table") is not None and len(q["tex_table"])
        uv.append(q["tri_uv"] if has else np.full((n, 3, 2), np.nan, np.float32))
        tex.append(np.where(q["tri_tex"] >= 0, q["tri_tex"] + n_tex, -1).astype(np.int32) if has else np.full(n, -1, np.int32))
        if has:
            r = q["tex_table"].copy()
            r[:, 0] += texels
            rows.append(r)
            data.append(q["tex_data"])
            n_tex += len(r)
            texels += len(q["tex_data"])
    g.update(tri_uv=np.concatenate(uv), tri_tex=np.concatenate(tex),
             tex_table=np.concatenate(rows) if rows else np.zeros((0, 4), np.int32),
             tex_data=np.concatenate(data) if data else np.zeros((0, 4), np.uint8))
    return g


# ---- a generated asset: a textured body and a textured revolute door, written as files ---------------------------------------
def _textured_box(path, lo, hi, mtl, material):
    """a box of six quads, every face mapped onto the whole texture"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    c = [[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)]
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    with open(path, "w") as fd:
        fd.write(f"mtllib {mtl}\nusemtl {material}\n")
        for v in c:
            fd.write("v %.6f %.6f %.6f\n" % tuple(v))
        fd.write("vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n")
        for f in faces:
            fd.write("f " + " ".join(f"{i + 1}/{k + 1}" for k, i in enumerate(f)) + "\n")


def write_textured_asset(root):
    """body (33 x 17 texture) + door on a revolute joint (a 4 x 4 texture in a sub-directory named with a space), both GAParts of
    a known class so that a rendered view converts into a training scene -> the asset's directory"""
    from PIL import Image
    root = str(root)
    os.makedirs(os.path.join(root, "objs", "my images"), exist_ok=True)
    Image.fromarray(texture(33, 17, 1)).save(os.path.join(root, "objs", "body.png"))
    Image.fromarray(texture(4, 4, 2)).save(os.path.join(root, "objs", "my images", "door 1.png"))
    with open(os.path.join(root, "objs", "paint.mtl"), "w") as fd:
        fd.write("newmtl body\nKd 0.9 0.5 0.1\nmap_Kd body.png\nnewmtl door\nKd 0.2 0.4 0.6\nmap_Kd -s 1 1 1 my images\\door 1.png\n")
    parts = {"link_body": ((-0.4, -0.5, -0.5), (0.4, 0.5, 0.3), "slider_drawer", "body"),
             "link_door": ((-0.47, -0.5, -0.5), (-0.4, 0.2, 0.3), "hinge_door", "door")}
    for name, (lo, hi, _, mat) in parts.items():
        _textured_box(os.path.join(root, "objs", f"{name}.obj"), lo, hi, "paint.mtl", mat)
    link = lambda n: f'<link name="{n}"><visual name="{n}-0"><origin xyz="0 0 0"/><geometry><mesh filename="objs/{n}.obj"/></geometry></visual></link>'
    urdf = ('<?xml version="1.0"?><robot name="boxes"><link name="base"/>' + link("link_body") + link("link_door")
            + '<joint name="joint_base" type="fixed"><origin xyz="0 0 0" rpy="0 0 0"/><child link="link_body"/><parent link="base"/></joint>'
            + '<joint name="joint_door" type="revolute"><origin xyz="-0.4 -0.5 0" rpy="0 0 0"/><axis xyz="0 0 1"/>'
              '<limit lower="0" upper="0.6"/><child link="link_door"/><parent link="link_body"/></joint></robot>')
    # the door's mesh is written in the body frame: shift it back by the joint origin through the visual origin
    urdf = urdf.replace('<visual name="link_door-0"><origin xyz="0 0 0"/>', '<visual name="link_door-0"><origin xyz="0.4 0.5 0"/>')
    with open(os.path.join(root, "mobility_annotation_gapartnet.urdf"), "w") as fd:
        fd.write(urdf)

    def corners(lo, hi):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        return [[x0, y1, z1], [x1, y1, z1], [x1, y0, z1], [x0, y0, z1], [x0, y1, z0], [x1, y1, z0], [x1, y0, z0], [x0, y0, z0]]

    anno = [dict(link_name=n, is_gapart=True, category=cat, bbox=corners(lo, hi)) for n, (lo, hi, cat, _) in parts.items()]
    with open(os.path.join(root, "link_annotation_gapartnet.json"), "w") as fd:
        json.dump(anno, fd)
    return root
