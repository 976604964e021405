"""The section-RS kernel (csrc/render.hip: rs_shade_kernel behind gpn_render_shade) against the per-pixel restatement
tests/render_shade_ref.py, byte for byte, on the smallest scenes that can break it, on fixture asset 45780, and on a generated
textured asset taken through render -> convert -> one training step.  The restatement shades the winning triangle and the depth
the raster kernel produced (tests/test_gpu_render.py holds those to their own restatement), so ties on shared edges are the
raster's."""
import os

import numpy as np
import pytest
import torch

from tests import render_ref as RR
from tests import render_shade_ref as RS
from tests import render_shade_scenes as SC
from tests.render_shade_scenes import px, quad, scene, texture

pytestmark = pytest.mark.gpu
OTHERS = ("depth", "tri", "sem", "ins", "npcs", "link_area", "link_inst", "counters")
FILL = 0xA5


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _up(d, cuda):
    return {k: torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for k, a in d.items() if isinstance(a, np.ndarray)}


def render_hip(g, t, cuda, shading="textured"):
    """the kernels on the tables, into a buffer prefilled with a sentinel: the padding behind every output must keep it"""
    from gapartnet_amd import hip_ops
    V, L = len(t["view_asset"]), t["link_cat"].shape[1]
    layout, total = hip_ops.render_layout(V, t["H"], t["W"], L)
    buf = torch.full((total,), FILL, dtype=torch.uint8, device=cuda)
    out, _ = hip_ops.render_batch(_up(g, cuda), _up(t, cuda), t["H"], t["W"], t["Nt_max"], t.get("background", (0, 0, 0)), buf=buf,
                                  shading=shading)
    assert out is buf
    host = buf.cpu()
    used = torch.zeros(total, dtype=torch.bool)
    for name, dt, shape, off in layout:
        used[off:off + int(np.prod(shape)) * hip_ops._RENDER_DT[dt]] = True
    assert bool((host[~used] == FILL).all()), "a kernel wrote behind an output"
    return {k: a.numpy() for k, a in hip_ops.render_fields(host, layout).items()}


def check(g, t, cuda):
    """textured call: rgb equals the restatement byte for byte; every other field is bit-equal to a flat call's"""
    got, flat = render_hip(g, t, cuda), render_hip(g, t, cuda, "flat")
    for k in OTHERS:
        assert np.array_equal(_bits(got[k]), _bits(flat[k])), k
    want = RS.shade(g, t, got["tri"], got["depth"])
    assert got["rgb"].dtype == np.uint8 and got["rgb"].shape == want.shape
    assert np.array_equal(got["rgb"], want), np.argwhere(got["rgb"] != want)[:5]
    return got


TEXTURES = [texture(1, 1), texture(2, 2), texture(3, 2), texture(257, 5)]


def mixed_scene(rng, H, W, lights, V=1):
    """random small triangles over the image with every kind of texture state: one of the four textures or none, uv in and far out
    of [0, 1], some corners without vt; plus a square split along a diagonal through pixel centres (shared edge) and a triangle
    with its mirror image"""
    n = 40
    c = rng.uniform([-2, -2], [W + 2, H + 2], (n, 1, 2))
    uv_px = c + rng.uniform(-6, 6, (n, 3, 2))
    z = rng.uniform(1.0, 3.0, (n, 3, 1))
    tris = list(np.concatenate([uv_px * z / SC.F, z], -1))
    uvs = list(rng.uniform(-3, 4, (n, 3, 2)))
    tex = list(rng.integers(-1, len(TEXTURES), n))
    for k in range(0, n, 7):
        uvs[k][k % 3] = [np.nan, 0.25]
    uvs[1] = uvs[1] * 1e4
    a, b = px([(2, 2), (10, 2), (10, 10)], 2.5), px([(2, 2), (10, 10), (2, 10)], 2.5)
    m = px([(12, 3), (15, 13), (3, 12)], 2.2)
    tris += [a, b, m, [m[0], m[2], m[1]]]
    uvs += [[(0, 1), (1, 1), (1, 0)], [(0, 1), (1, 0), (0, 0)], [(0.1, 0.9), (0.9, 0.8), (0.2, 0.1)], [(0.1, 0.9), (0.2, 0.1), (0.9, 0.8)]]
    tex += [2, 3, 2, 2]
    return scene(tris, uvs, tex, TEXTURES, lights, H, W, colors=rng.uniform(0, 1, (len(tris), 3)), V=V, links=rng.integers(0, 3, len(tris)))


def some_lights(rng, n):
    kinds = [RS.AMBIENT] + [RS.DIRECTIONAL + i % 2 for i in range(n - 1)]
    rows = []
    for k in kinds[:n]:
        xyz = rng.uniform(-2, 2, 3)
        if k == RS.DIRECTIONAL:
            xyz = xyz / np.linalg.norm(xyz)
        rows.append((k, xyz, rng.uniform(0, 0.7, 3)))
    return rows


@pytest.mark.parametrize("H,W,NL", [(1, 1, 1), (17, 15, 0), (17, 15, 16), (48, 64, 5)])
def test_mixed_textures_image_sizes_and_light_counts(cuda, H, W, NL):
    rng = np.random.default_rng(H * 100 + W + NL)
    g, t = mixed_scene(rng, H, W, some_lights(rng, NL))
    if H == 1:  # one pixel: make sure it is drawn, by a textured triangle
        g, t = scene([px([(-3, -3), (9, -3), (-3, 9)], 2.0)], [[(0.1, 0.2), (2.3, 0.4), (0.5, 3.6)]], [3], TEXTURES, some_lights(rng, NL), 1, 1)
    got = check(g, t, cuda)
    hit = got["tri"][0] >= 0
    assert hit.any()
    if NL == 0:
        assert (got["rgb"][0][hit] == 0).all() and (got["rgb"][0][~hit] == (7, 8, 9)).all()
    if H > 1:
        assert len(np.unique(got["tri"][0])) > 12 and (~hit).any()
    if H == 48:
        drawn = np.unique(got["tri"][0][hit])
        tex, nan = g["tri_tex"][drawn], np.isnan(g["tri_uv"][drawn]).any(axis=(1, 2))
        assert set(tex.tolist()) == {-1, 0, 1, 2, 3} and nan.any() and (~nan).any()  # every texture state is on screen
        square = got["tri"][0][2:10, 2:10]
        assert set(np.unique(square)) >= {40, 41}  # both halves of the shared-edge square won pixels


def test_no_textures_at_all(cuda):
    """T = 0: geometry tables without the texture tables, Kd under the lights"""
    rng = np.random.default_rng(1)
    tris, _ = quad(1, 1, 14, 12, z=2.0)
    g, t = scene(tris, None, None, None, some_lights(rng, 4), 15, 17, colors=rng.uniform(0, 1, (2, 3)))
    assert "tex_table" not in g
    check(g, t, cuda)
    g0 = RS.add_textures(g, [], [-1, -1], np.full((2, 3, 2), np.nan))  # empty tables are T = 0 as well
    assert np.array_equal(render_hip(g0, t, cuda)["rgb"], render_hip(g, t, cuda)["rgb"])


def test_point_light_on_the_surface_and_behind_it(cuda):
    tris, uvs = quad(2, 2, 11, 11, z=2.0)
    lights = [(RS.AMBIENT, (0, 0, 0), (0.5, 0.5, 0.5)), (RS.POINT, (1, 1, 2), (1, 1, 1)), (RS.POINT, (1, 1, 4), (1, 1, 1))]
    got = check(*scene(tris, uvs, [0, 0], [texture(2, 2)], lights, 12, 12), cuda)
    assert np.isfinite(got["depth"]).all() and got["tri"][0, 8, 8] >= 0  # (8, 8) is the pixel at the light: r = 0 there
    only_ambient = check(*scene(tris, uvs, [0, 0], [texture(2, 2)], lights[:1], 12, 12), cuda)
    assert np.array_equal(got["rgb"][0, 8, 8], only_ambient["rgb"][0, 8, 8])


def test_mixed_assets_with_their_own_textures_and_a_view_without_an_asset(cuda):
    rng = np.random.default_rng(2)
    a, ta = mixed_scene(rng, 15, 17, [])
    tris, uvs = quad(-1, -1, 30, 30, z=1.5, uv=((-1, 2), (2, 2), (2, -1), (-1, -1)))
    b, _ = scene(tris, uvs, [1, 0], [texture(5, 3, 9), texture(2, 7, 9)], [], 15, 17)
    c, _ = scene(quad(3, 3, 9, 9)[0], None, None, None, [], 15, 17)  # an asset without textures between textured ones
    g = SC.merge([a, c, b])
    assert g["tex_table"].shape == (6, 4) and g["tri_tex"].max() == 5
    t = RR.identity_views(4, 15, 17, links=3, f=SC.F, view_asset=[2, -1, 0, 1], Nt_max=len(a["tris"]))
    t["lights"] = RS.light_table(4, some_lights(rng, 3))
    t["lights"][1:, :, 4:7] *= 0.5  # the rows are per view
    got = check(g, t, cuda)
    assert (got["tri"][1] == -1).all() and (got["rgb"][1] == (7, 8, 9)).all() and (got["tri"][0] >= len(a["tris"]) + 2).all()
    again = render_hip(g, t, cuda)
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k  # reruns are bit-equal


def test_shade_alone_writes_rgb_and_nothing_else(cuda):
    """render_shade on its own tensors: the bytes in front of and behind rgb keep a sentinel, depth and tri are only read"""
    from gapartnet_amd import hip_ops
    rng = np.random.default_rng(3)
    g, t = mixed_scene(rng, 15, 17, some_lights(rng, 6), V=2)
    base = render_hip(g, t, cuda, "flat")
    n = 2 * 15 * 17 * 3
    slab = torch.full((n + 512,), FILL, dtype=torch.uint8, device=cuda)
    depth, tri = torch.from_numpy(base["depth"]).to(cuda), torch.from_numpy(base["tri"]).to(cuda)
    hip_ops.render_shade(_up(g, cuda), _up(t, cuda), depth, tri, slab[256:256 + n], 15, 17, t["Nt_max"], t["background"])
    host = slab.cpu().numpy()
    assert (host[:256] == FILL).all() and (host[256 + n:] == FILL).all()
    assert np.array_equal(host[256:256 + n].reshape(2, 15, 17, 3), RS.shade(g, t, base["tri"], base["depth"]))
    assert np.array_equal(_bits(depth.cpu().numpy()), _bits(base["depth"])) and np.array_equal(tri.cpu().numpy(), base["tri"])


def test_wrong_arguments_are_refused(cuda):
    from gapartnet_amd import _C, hip_ops
    rng = np.random.default_rng(4)
    g, t = mixed_scene(rng, 15, 17, some_lights(rng, 2))
    gd, td = _up(g, cuda), _up(t, cuda)
    run = lambda gd_, td_, **kw: hip_ops.render_batch(gd_, td_, 15, 17, t["Nt_max"], t["background"], shading="textured", **kw)
    run(gd, td)
    with pytest.raises(_C.GpnError, match="shading"):
        hip_ops.render_batch(gd, td, 15, 17, t["Nt_max"], shading="phong")
    with pytest.raises(_C.GpnError, match="NL"):
        run(gd, dict(td, lights=torch.zeros(1, 17, 8, dtype=torch.float64, device=cuda)))
    with pytest.raises(_C.GpnError, match="lights"):
        run(gd, {k: a for k, a in td.items() if k != "lights"})
    with pytest.raises(_C.GpnError, match="lights"):
        run(gd, dict(td, lights=torch.zeros(1, 2, 7, dtype=torch.float64, device=cuda)))
    with pytest.raises(_C.GpnError, match="tri_tex outside"):
        run(dict(gd, tri_tex=gd["tri_tex"] + 1), td)
    with pytest.raises(_C.GpnError, match="tri_tex outside"):
        run(dict(gd, tri_tex=gd["tri_tex"] - 1), td)
    with pytest.raises(_C.GpnError, match="outside tex_data"):
        run(dict(gd, tex_data=gd["tex_data"][:-1].contiguous()), td)
    with pytest.raises(_C.GpnError, match="tri_uv"):
        run(dict(gd, tri_uv=gd["tri_uv"][:-1].contiguous()), td)
    with pytest.raises(_C.GpnError):
        run(dict(gd, tex_data=gd["tex_data"].cpu()), td)
    # with the host-side check switched off the kernel's own bounds checks hold: such a triangle is shaded with its Kd
    bad = dict(gd, tri_tex=torch.full_like(gd["tri_tex"], 99))
    buf, layout = run(bad, td, check_tables=False)
    kd = RS.shade(dict(g, tri_tex=np.full_like(g["tri_tex"], -1)), t, *(hip_ops.render_fields(buf.cpu(), layout)[k].numpy() for k in ("tri", "depth")))
    assert np.array_equal(hip_ops.render_fields(buf.cpu(), layout)["rgb"].numpy(), kd)


def test_fixture_asset_under_the_reference_rig(cuda):
    from gapartnet_amd.dataset import render_assets as RA
    asset = RA.load_asset(RR.fixture_asset(), textures=True)
    rng = np.random.RandomState(7)
    reqs = [RA.RenderRequest(0, RA.sample_qpos(asset, rng), RA.sample_camera(RA.DEFAULT_CAMERA_RANGE, rng)) for _ in range(2)]
    g = RA.geometry_tables([asset])
    t, _ = RA.view_tables([asset], reqs, 96, 96)
    t["background"] = RA.BACKGROUND_RGB
    got = check(g, t, cuda)
    assert (got["depth"] > 0).sum() > 4000 and t["lights"].shape == (2, 5, 8)
    views = RA.render_views([asset], reqs, 96, 96, device=cuda, shading="textured")  # the public call gives the same images
    flat = RA.render_views([asset], reqs, 96, 96, device=cuda)
    for v, view in enumerate(views):
        assert np.array_equal(view.rgb, got["rgb"][v]) and not np.array_equal(view.rgb, flat[v].rgb)
        assert np.array_equal(_bits(view.depth), _bits(flat[v].depth)) and np.array_equal(view.ins, flat[v].ins)
        assert np.array_equal(_bits(view.npcs), _bits(flat[v].npcs)) and view.counters == flat[v].counters


def test_textured_render_convert_train_end_to_end(cuda, tmp_path):
    from gapartnet_amd.dataset import convert_rendered as CR
    from gapartnet_amd.dataset import render_assets as RA
    asset = RA.load_asset(SC.write_textured_asset(tmp_path / "asset"), textures=True)
    assert len(asset.textures) == 2 and asset.missing_textures == 0
    rng = np.random.RandomState(11)
    reqs = [RA.RenderRequest(0, RA.sample_qpos(asset, rng), RA.sample_camera(RA.DEFAULT_CAMERA_RANGE, rng)) for _ in range(2)]
    g = RA.geometry_tables([asset])
    t, _ = RA.view_tables([asset], reqs, 64, 64)
    t["background"] = RA.BACKGROUND_RGB
    got = check(g, t, cuda)
    assert np.array_equal(got["rgb"], RA.render_tables_numpy(g, t, "textured")["rgb"])  # the CPU path of the same contract
    data, save = str(tmp_path / "rendered"), str(tmp_path / "sampled")
    views = RA.render_views([asset], reqs, 64, 64, device=cuda, shading="textured")
    for i, view in enumerate(views):
        assert np.array_equal(view.rgb, got["rgb"][i]) and len(np.unique(view.rgb.reshape(-1, 3), axis=0)) > 50
        RA.write_view(data, f"Box_7_0_{i}", view, dict(model_id=7, category="Box", camera_idx=0, render_idx=i))
    stats = CR.convert_directory(data, save, dataset="partnet", num_points=512, batch=2, workers=2, log_path=str(tmp_path / "log.txt"),
                                 device=cuda, echo=False)
    assert stats["views"] == 2 and stats["written"] == 2, stats
    from gapartnet_amd.dataset.gapartnet import GAPartNetDataset
    from gapartnet_amd.smoke import make_model
    ds = GAPartNetDataset(os.path.join(save, "pth"), max_points=512, voxel_size=(0.01, 0.01, 0.01))
    scenes = [ds[i] for i in range(len(ds))]
    assert len(scenes) == 2 and all(bool((s.instance_labels >= 0).any()) for s in scenes)
    model = make_model((0, 0), seed=0).to(cuda)
    model.train()
    loss = model.training_step([s.to(cuda) for s in scenes], 0)
    loss.backward()
    assert torch.isfinite(loss).item()
