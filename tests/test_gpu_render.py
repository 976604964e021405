"""The section-RD kernels (csrc/render.hip: setup, raster, annotate) against the per-pixel restatement tests/render_ref.py:
depth and NPCS bit-equal, tri / sem / ins / link_area / link_inst / counters equal, RGB within one level - on the smallest scenes
that can break them, on fixture asset 45780, and end to end into a training step."""
import os

import numpy as np
import pytest
import torch

from tests import render_ref as RR

pytestmark = pytest.mark.gpu
EXACT = ("depth", "tri", "sem", "ins", "link_area", "link_inst", "npcs", "counters")
F = 16.0  # focal length of the hand-made scenes: a camera point (u / 16, v / 16, 1) lands exactly on pixel position (u, v)
FILL = 0xA5


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def render_hip(g, t, cuda):
    """the kernels on the tables, into a buffer prefilled with a sentinel: the padding behind every output must keep it"""
    from gapartnet_amd import hip_ops
    gd = {k: torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for k, a in g.items()}
    td = {k: torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for k, a in t.items() if isinstance(a, np.ndarray)}
    V, L = len(t["view_asset"]), t["link_cat"].shape[1]
    layout, total = hip_ops.render_layout(V, t["H"], t["W"], L)
    buf = torch.full((total,), FILL, dtype=torch.uint8, device=cuda)
    out, _ = hip_ops.render_batch(gd, td, t["H"], t["W"], t["Nt_max"], t.get("background", (0, 0, 0)), buf=buf)
    assert out is buf
    host = buf.cpu()
    used = torch.zeros(total, dtype=torch.bool)
    for name, dt, shape, off in layout:
        used[off:off + int(np.prod(shape)) * hip_ops._RENDER_DT[dt]] = True
    assert bool((host[~used] == FILL).all()), "a kernel wrote behind an output"
    return {k: a.numpy() for k, a in hip_ops.render_fields(host, layout).items()}


def check(g, t, cuda):
    got, want = render_hip(g, t, cuda), RR.render(g, t)
    for k in EXACT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, np.argwhere(_bits(got[k]) != _bits(want[k]))[:5])
    assert np.abs(got["rgb"].astype(np.int32) - want["rgb"].astype(np.int32)).max(initial=0) <= 1
    return got


def px(pts, z=1.0):
    """pixel positions (u, v) [and a depth each] -> camera-space points"""
    out = []
    for p in pts:
        d = float(p[2]) if len(p) > 2 else float(z)
        out.append([p[0] * d / F, p[1] * d / F, d])
    return out


def small_soup(rng, n, H, W):
    """n triangles of a few pixels' extent at random places and depths, some hanging over the image border"""
    c = rng.uniform([-2, -2], [W + 2, H + 2], (n, 1, 2))
    uv = c + rng.uniform(-3.5, 3.5, (n, 3, 2))
    z = rng.uniform(1.0, 3.0, (n, 3, 1))
    tri = np.concatenate([uv * z / F, z], -1)
    return RR.soup(tri, links=rng.integers(0, 3, n) if n else None, colors=rng.uniform(0, 1, (n, 3)))


@pytest.mark.parametrize("H,W", [(1, 1), (16, 16), (17, 33), (48, 64)])
def test_image_sizes_and_chunk_boundaries(cuda, H, W):
    """one batch of five views over five assets with 0, 1, 255, 256 and 257 triangles (the scan's chunk is 256)"""
    rng = np.random.default_rng(H * 100 + W)
    counts = (0, 1, 255, 256, 257)
    geoms = [small_soup(rng, n, H, W) for n in counts]
    geoms[1] = RR.soup([px([(-1, -1), (3 * W + 40, -1), (-1, 3 * H + 40)], 2.0)])  # the single triangle covers the image
    g = RR.merge(geoms)
    t = RR.identity_views(len(counts), H, W, links=3, f=F, view_asset=range(len(counts)), Nt_max=257)
    t["link_cat"][:] = [4, -1, 2]
    t["link_frame"][:, :, :3] = rng.uniform(-0.2, 0.2, (len(counts), 3, 3))
    t["link_frame"][:, :, 3] = rng.uniform(0.8, 1.6, (len(counts), 3))
    got = check(g, t, cuda)
    assert (got["tri"][0] == -1).all() and (got["depth"][0] == 0).all() and (got["sem"][0] == -2).all()
    assert (got["tri"][1] == 0).all() and (got["depth"][1] == 2.0).all()  # fronto-parallel: exactly constant depth
    assert (got["rgb"][0] == np.array(t["background"], np.uint8)).all()
    if H > 1:
        assert len(np.unique(got["tri"][4])) > 20


def test_no_triangles_at_all(cuda):
    g = RR.soup(np.zeros((0, 3, 3)))
    t = RR.identity_views(2, 17, 33, f=F)
    got = check(g, t, cuda)
    assert (got["tri"] == -1).all() and (got["ins"] == -2).all() and (got["counters"] == 0).all() and (got["link_inst"] == -1).all()


def test_shared_edges_vertices_and_slivers(cuda):
    """the diagonal of the square runs through pixel centres and its corners sit on them: each centre belongs to one triangle"""
    a = px([(2, 2), (10, 2), (10, 10)])
    b = px([(2, 2), (10, 10), (2, 10)])
    sliver = px([(2.3, 2.6), (7.5, 3.42), (7.5, 3.38)])  # its pixel box holds centres, the triangle none
    g = RR.merge([RR.soup([a, b]), RR.soup([a]), RR.soup([b[::-1]]), RR.soup([sliver])])  # (b wound the other way: no culling)
    t = RR.identity_views(4, 16, 16, f=F, view_asset=[0, 1, 2, 3], Nt_max=2)
    got = check(g, t, cuda)
    both, only_a, only_b = (got["tri"][v] >= 0 for v in range(3))
    square = np.zeros((16, 16), bool)
    square[2:10, 2:10] = True  # top and left edges in, bottom and right edges out
    assert np.array_equal(both, square)
    assert not (only_a & only_b).any() and np.array_equal(only_a | only_b, square)
    assert only_a[2, 2] != only_b[2, 2] and not both[10, 10] and not both[2, 10] and not both[10, 2]
    assert (got["tri"][3] == -1).all() and (got["counters"] == 0).all()


def test_depth_order_and_ties(cuda):
    H, W = 48, 64
    cover = px([(-1, -1), (200, -1), (-1, 200)], 3.0)
    twin = px([(4, 4), (40, 6), (10, 30)], 2.0)
    left = px([(20, 2, 1.0), (20, 46, 1.0), (60, 24, 2.5)])   # two triangles that cut through each other
    right = px([(60, 2, 1.0), (60, 46, 1.0), (20, 24, 2.5)])
    g = RR.merge([RR.soup([cover, twin, twin]), RR.soup([twin, cover, twin]), RR.soup([left, right])])
    t = RR.identity_views(3, H, W, f=F, view_asset=[0, 1, 2], Nt_max=3)
    got = check(g, t, cuda)
    assert (got["tri"][0] >= 0).all()  # one triangle covers every tile
    assert set(np.unique(got["tri"][0])) == {0, 1}  # never the second copy
    assert set(np.unique(got["tri"][1])) == {3, 4} and (got["tri"][1] == 3).sum() == (got["tri"][0] == 1).sum()
    cut = got["tri"][2]
    assert (cut == 6).any() and (cut == 7).any() and (cut[:, :30] != 7).all() and (cut[:, 51:] != 6).all()


def test_dropped_triangles_are_counted_and_not_drawn(cuda):
    good = px([(2, 2), (12, 3), (5, 13)], 2.0)
    tris = [good,
            px([(1, 1), (5, 5), (9, 9)]),                          # zero area
            px([(40, 3), (50, 3), (45, 12)]),                      # off the image
            px([(2, 2, -2.0), (12, 3, -2.0), (5, 13, -2.0)]),      # behind the camera
            px([(2, 2, 1.0), (12, 3, 0.05), (5, 13, 1.0)]),        # crosses near
            px([(2, 2), (17000, 3), (5, 13)]),                     # beyond the +-16384 px guard
            good]
    g = RR.soup(tris)
    g["tri_visual"][6] = 3  # a visual outside the table
    t = RR.identity_views(1, 16, 16, f=F, Nt_max=len(tris))
    got = check(g, t, cuda)
    assert got["counters"][0].tolist() == [1, 2, 1, 1, 1]  # index, near, guard, zero area, off screen
    assert set(np.unique(got["tri"][0])) == {-1, 0}


def test_mixed_assets_hidden_links_and_views_without_targets(cuda):
    """V = 3 over two assets of different triangle and link counts.  Asset 0: four target links; the link ranked second is fully
    hidden, so the later ids close up.  Asset 1: two links, neither a target."""
    H, W = 17, 33
    front = px([(-1, -1), (100, -1), (-1, 100)], 1.0)
    quad = lambda x0, z: [px([(x0, 2), (x0 + 6, 2), (x0 + 6, 12)], z), px([(x0, 2), (x0 + 6, 12), (x0, 12)], z)]
    a0 = RR.soup(quad(1, 2.0) + quad(9, 2.0) + quad(17, 2.0) + quad(25, 2.0) + quad(9, 1.5), links=[0, 0, 1, 1, 2, 2, 3, 3, 4, 4])
    a1 = RR.soup([front] + quad(3, 0.5), links=[0, 1, 1])
    g = RR.merge([a0, a1])
    t = RR.identity_views(3, H, W, links=5, f=F, view_asset=[0, 1, 0], Nt_max=10)
    t["link_cat"][:] = [3, 0, 5, 1, -1]      # link 4 is "others" and hides link 1
    t["link_rank"][:] = [2, 1, 0, 3, -1]
    t["link_cat"][1] = -1
    t["link_frame"][:, :, 3] = 2.0
    got = check(g, t, cuda)
    assert got["link_inst"][0].tolist() == [1, -1, 0, 2, -1] and got["link_area"][0, 1] == 0 and got["link_area"][0, 4] > 0
    assert np.array_equal(got["link_inst"][2], got["link_inst"][0])
    assert set(np.unique(got["ins"][0])) == {-2, -1, 0, 1, 2} and set(np.unique(got["sem"][0])) == {-2, -1, 3, 5, 1}
    assert (got["link_inst"][1] == -1).all() and set(np.unique(got["ins"][1])) == {-1} and (got["npcs"][1] == 0).all()
    assert got["link_area"][1].tolist()[:2] == [H * W - got["link_area"][1, 1], got["link_area"][1, 1]]
    again = render_hip(g, t, cuda)
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k  # reruns are bit-equal


def test_sloped_plane_depth_stays_within_the_snapping_bound(cuda):
    """vertices off the 1/256 grid on a plane whose depth grows with u only.  Snapping moves a vertex by at most 1/512 px on an
    axis, so the drawn surface at a pixel is the true plane seen at most 1/256 px away; with the factor 2 of slack the depth
    differs from the float64 ray-plane intersection by at most |dz/du| * (1/256) * 2, each pixel against its own slope."""
    H, W = 48, 64
    rng = np.random.default_rng(3)
    z_of_u = lambda u: 1.5 + 0.02 * u  # depth along the plane at image position u: dz/du = 0.02 per pixel at the vertices
    uv = [(1.3 + rng.uniform(0, 1 / 256), 2.7), (61.77, 3.21), (30.123, 45.9)]
    g = RR.soup([px([(u, v, z_of_u(u)) for u, v in uv])])
    t = RR.identity_views(1, H, W, f=F)
    t["Nt_max"] = 1
    got = check(g, t, cuda)
    P = g["verts"].astype(np.float64)  # the plane n . p = d through the float32 vertices
    n = np.cross(P[1] - P[0], P[2] - P[0])
    d = n @ P[0]
    ys, xs = np.nonzero(got["tri"][0] == 0)
    assert len(ys) > 800
    along = np.stack([xs / F, ys / F, np.ones(len(xs))], -1) @ n  # n . ray of the pixel; z = d / along
    z_true = d / along
    dz_du = np.abs(d * (n[0] / F) / (along * along))
    z_got = got["depth"][0][ys, xs].astype(np.float64)
    bound = dz_du * (1 / 256) * 2
    print("sloped plane: max |dz| %.3e, smallest bound %.3e, dz/du %.4f .. %.4f" % (np.abs(z_got - z_true).max(), bound.min(),
                                                                                   dz_du.min(), dz_du.max()))
    assert (np.abs(z_got - z_true) <= bound).all()


@pytest.fixture(scope="module")
def asset():
    from gapartnet_amd.dataset import render_assets as RA
    return RA.load_asset(RR.fixture_asset())


def test_fixture_asset_equals_the_restatement(cuda, asset):
    from gapartnet_amd.dataset import render_assets as RA
    rng = np.random.RandomState(7)
    reqs = [RA.RenderRequest(0, RA.sample_qpos(asset, rng), RA.sample_camera(RA.DEFAULT_CAMERA_RANGE, rng)) for _ in range(2)]
    assert reqs[0].joint_qpos != reqs[1].joint_qpos
    g = RA.geometry_tables([asset])
    t, _ = RA.view_tables([asset], reqs, 96, 96)
    t["background"] = RA.BACKGROUND_RGB
    got = check(g, t, cuda)
    assert (got["link_inst"][:, [1, 2]] >= 0).all() and (got["depth"] > 0).sum() > 4000 and (got["counters"][:, :3] == 0).all()
    views = RA.render_views([asset], reqs, 96, 96, device=cuda)  # the public call gives the same images
    for v, view in enumerate(views):
        assert np.array_equal(_bits(view.depth), _bits(got["depth"][v])) and np.array_equal(view.ins, got["ins"][v])
        assert np.array_equal(_bits(view.npcs), _bits(got["npcs"][v])) and np.array_equal(view.rgb, got["rgb"][v])
        assert list(view.bbox_pose_dict) == [n for n in asset.targets if got["link_inst"][v][asset.links.index(n)] >= 0]


def test_render_convert_train_end_to_end(cuda, asset, tmp_path):
    from gapartnet_amd.dataset import convert_rendered as CR
    from gapartnet_amd.dataset import render_assets as RA
    rng = np.random.RandomState(11)
    reqs = [RA.RenderRequest(0, RA.sample_qpos(asset, rng), RA.sample_camera(RA.DEFAULT_CAMERA_RANGE, rng)) for _ in range(4)]
    data, save = str(tmp_path / "rendered"), str(tmp_path / "sampled")
    for i, view in enumerate(RA.render_views([asset], reqs, 200, 200, device=cuda)):
        RA.write_view(data, f"StorageFurniture_45780_0_{i}", view, dict(model_id=45780, category="StorageFurniture", camera_idx=0,
                                                                        render_idx=i))
    stats = CR.convert_directory(data, save, dataset="partnet", num_points=2048, batch=4, workers=4,
                                 log_path=str(tmp_path / "log.txt"), device=cuda, echo=False)
    assert stats["views"] == 4 and stats["written"] == 4, stats
    from gapartnet_amd.dataset.gapartnet import GAPartNetDataset
    from gapartnet_amd.smoke import make_model
    ds = GAPartNetDataset(os.path.join(save, "pth"), max_points=2048, voxel_size=(0.01, 0.01, 0.01))
    scenes = [ds[i] for i in range(len(ds))]
    assert len(scenes) == 4 and all(bool((s.instance_labels >= 0).any()) for s in scenes)
    model = make_model((0, 0), seed=0).to(cuda)
    model.train()
    loss = model.training_step([s.to(cuda) for s in scenes[:2]], 0)
    loss.backward()
    assert torch.isfinite(loss).item()


def test_wrong_arguments_are_refused(cuda):
    from gapartnet_amd import _C, hip_ops
    g = RR.soup([px([(2, 2), (12, 3), (5, 13)])])
    gd = {k: torch.from_numpy(a).to(cuda) for k, a in g.items()}

    def views(**kw):
        t = RR.identity_views(1, 16, 16, f=F, **kw)
        return {k: torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for k, a in t.items() if isinstance(a, np.ndarray)}

    with pytest.raises(_C.GpnError, match="bad argument"):
        hip_ops.render_batch(gd, views(), 0, 16, 1)
    with pytest.raises(_C.GpnError, match="Nt_max <= Nt"):
        hip_ops.render_batch(gd, views(), 16, 16, 2)
    with pytest.raises(_C.GpnError, match="kMaxLinks"):
        hip_ops.render_batch(gd, views(links=hip_ops.render_max_links() + 1), 16, 16, 1)
    with pytest.raises(_C.GpnError, match="bg_r"):
        hip_ops.render_batch(gd, views(), 16, 16, 1, background=(256, 0, 0))
    with pytest.raises(_C.GpnError):
        hip_ops.render_batch({k: a.cpu() for k, a in gd.items()}, views(), 16, 16, 1)
    with pytest.raises(_C.GpnError, match="vis_mat"):
        hip_ops.render_batch(gd, dict(views(), cam=torch.zeros(1, 19, dtype=torch.float64, device=cuda)), 16, 16, 1)
