"""CPU: the inputs and the reference of tests/test_gpu_proposal_seams.py.  Every case of tests/proposal_cases.py has the property
it is named for (recomputed here from the reference), the reference of tests/proposal_ref.py equals the torch formulation of
the stage on the CPU oracle's operators, and assert_tables_equal rejects single-entry mutations of a correct result."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

from tests import proposal_cases as C
from tests import proposal_ref as R
from tests import rulebook_ref


@functools.lru_cache(maxsize=None)
def _ref(name, div="mul"):
    return R.build(*C.build_args(C.BUILD_CASES[name]()), div=div)


@functools.lru_cache(maxsize=None)
def _post_ref(name):
    c = C.POST_CASES[name]()
    return R.postprocess(c["score"], c["sizes"], c["proposal_offsets"], c["point_indices"], c["proposal_indices"], c["score_thr"],
                         c["min_points"], c["iou_thr"], live=c["live"])


def _set_sizes(ref, N):
    """sizes of the kept proposals of set A and of set B"""
    out = []
    for which in range(2):
        slots = ref["member_slot"][which * N:(which + 1) * N]
        out.append(ref["sizes"][np.unique(ref["proposal_indices"][slots[slots >= 0]])].tolist())
    return out


# ------------------------------------------------------------------------------------------------ the build cases
@pytest.mark.parametrize("name", list(C.BUILD_CASES))
def test_distances_keep_one_percent_from_the_radius(name):
    c = C.BUILD_CASES[name]()
    xyz = np.asarray(c["points"], np.float32)
    sets = (xyz.astype(np.float64), (xyz + c["offset_preds"]).astype(np.float64))
    assert xyz.shape[0] <= 6000
    key = c["batch_indices"].astype(np.int64) * 100 + c["sem_preds"]
    exact = 0
    for coords in sets:
        for k in np.unique(key):
            p = coords[key == k]
            d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
            close = np.abs(d - c["radius"]) < 0.01 * c["radius"]
            if c.get("exact_pairs"):
                assert (d[close] == c["radius"]).all(), "the deliberate exception: exactly one radius, nothing near it"
                exact += int(close.sum())
            else:
                assert not close.any(), float(np.abs(d - c["radius"]).min() / c["radius"])
    assert (exact > 0) == bool(c.get("exact_pairs"))


@pytest.mark.parametrize("name", [k for k in C.BUILD_CASES if "sizes_A" in C.BUILD_CASES[k]()])
def test_clusters_have_the_sizes_the_case_was_built_for(name):
    c, ref = C.BUILD_CASES[name](), _ref(name)
    if name in C.NONE_CASES:
        assert ref is None and c["sizes_A"] == [] and c["sizes_B"] == []
        return
    assert _set_sizes(ref, c["points"].shape[0]) == [c["sizes_A"], c["sizes_B"]]
    assert ref["dropped"] == 0 and ref["M"] == sum(c["sizes_A"]) + sum(c["sizes_B"])


def test_min_points_edges_has_clusters_on_both_sides_of_the_filter():
    c, ref = C.BUILD_CASES["min_points_edges"](), _ref("min_points_edges")
    valid = ref["valid_mask"]
    for labels, kept in zip(ref["_labels"], _set_sizes(ref, valid.shape[0])):
        every = np.unique(labels[valid], return_counts=True)[1]
        assert {c["min_points"] - 1, c["min_points"], c["min_points"] + 1} <= set(every.tolist())
        assert c["min_points"] - 1 not in kept and c["min_points"] in kept


def test_merge_and_split_changes_the_partition_between_the_sets():
    c, ref = C.BUILD_CASES["merge_and_split"](), _ref("merge_and_split")
    (la, lb), (a, b, cc) = ref["_labels"], c["rows"]
    assert la[a.start] != la[b.start] and lb[a.start] == lb[b.start], "merged in set B"
    assert la[cc.start] == la[cc.stop - 1] and lb[cc.start] != lb[cc.stop - 1], "split in set B"


def test_collapsed_blob_overflows_the_hit_list_of_every_query():
    c = C.BUILD_CASES["collapsed_blob"]()
    n = c["blob"]
    assert n == 3 * c["K2"] + 5 and n > 256
    shifted = (c["points"] + c["offset_preds"])[:n].astype(np.float64)
    d = np.sqrt(((shifted[:, None] - shifted[None]) ** 2).sum(-1))
    assert ((d < c["radius"]).sum(1) == n).all()
    assert c["sem_preds"][n] != c["sem_preds"][n - 1], "another class follows directly"
    ref = _ref("collapsed_blob")
    assert ref["_labels"][1][n + 7] == n + 7, "and another cluster of the blob's class behind it"


@pytest.mark.parametrize("name", ["same_place_other_class", "same_place_other_scene"])
def test_coincident_points_of_another_class_or_scene_do_not_merge(name):
    c, ref = C.BUILD_CASES[name](), _ref(name)
    a = c["rows"]
    assert np.array_equal(c["points"][a], c["points"][a.stop:])
    assert ref["P"] == 4 and (ref["_labels"][0][a.stop:] == a.stop).all()


def test_invalid_mix_depends_on_the_labels():
    with_labels, without = _ref("invalid_mix"), _ref("invalid_mix_no_labels")
    assert C.BUILD_CASES["invalid_mix_no_labels"]()["instance_labels"] is None and without["instance_labels"] is None
    assert with_labels["Q"] == 28 - 4 - 5 and without["Q"] == 28 - 4
    assert not with_labels["valid_mask"][[1, 4, 23]].any() and without["valid_mask"][[4, 23]].all()
    assert _set_sizes(with_labels, 28)[0] != _set_sizes(without, 28)[0]


def test_scene_cases_have_the_empty_scenes():
    c, ref = C.BUILD_CASES["scenes"](), _ref("scenes")
    scene, valid = c["batch_indices"], ref["valid_mask"]
    assert c["batch_size"] == 6 and sorted(set(scene.tolist())) == [0, 1, 2, 4]
    assert not valid[scene == 1].any() and valid[scene == 0].any() and valid[scene == 2].any()
    c, ref = C.BUILD_CASES["scenes_b4"](), _ref("scenes_b4")
    scene, valid = c["batch_indices"], ref["valid_mask"]
    assert c["batch_size"] == 4 and not valid[scene == 1].any() and all(valid[scene == s].all() for s in (0, 2, 3))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_point_counts_sit_on_the_workgroup_seam(n):
    c = C.BUILD_CASES["n_1_valid" if n == 1 else f"n_{n}"]()
    assert c["points"].shape[0] == n and _ref("n_1_valid" if n == 1 else f"n_{n}")["Q"] == n


@pytest.mark.parametrize("name", C.NONE_CASES)
def test_cases_without_valid_points_give_none(name):
    assert _ref(name) is None


def test_proposal_counts_and_sizes_on_the_kernel_seams():
    assert _ref("proposals_1100")["P"] == 1100 > 1024 and C.BUILD_CASES["proposals_1100"]()["min_points"] == 2
    sizes = _ref("sizes_63_64_65_128_129_257_513")["sizes"].tolist()
    assert sizes == list(C.SEAM_SIZES) * 2
    assert {63, 64, 65} <= set(sizes) and {257, 513} <= set(sizes), "64-point staging of the stats kernel, 256-point chunks of the place kernel"
    assert _ref("one_giant")["sizes"].tolist() == [600, 600] and C.BUILD_CASES["one_giant"]()["points"].shape[0] == 600


def test_degenerate_extents():
    c, ref = C.BUILD_CASES["degenerate_extent"](), _ref("degenerate_extent")
    b, e = ref["proposal_offsets"][:2]
    assert (ref["pt_xyz"][b:e] == ref["pt_xyz"][b]).all() and ref["_scale"][0] == np.float32(c["max_scale"]), "1 / 0, clamped"
    b, e = ref["proposal_offsets"][1:3]
    assert (ref["pt_xyz"][b:e, 2] == 0).all() and np.ptp(ref["pt_xyz"][b:e, 0]) > 0
    assert np.isfinite(ref["_scaled"]).all() and ref["dropped"] == 0


def test_strided_case_is_a_view_of_a_wider_matrix():
    a, b = C.BUILD_CASES["strided"](), C.BUILD_CASES["strided_contiguous"]()
    assert not a["points"].flags.c_contiguous and a["points"].strides[0] == 24 and b["points"].flags.c_contiguous
    assert np.array_equal(a["points"], b["points"])
    R.assert_tables_equal(_ref("strided"), _ref("strided_contiguous"))


@pytest.mark.parametrize("full", [7, 28, 30, 31, 32])
def test_fullscale_cases_sit_on_the_bitmap_seam(full):
    c, ref = C.BUILD_CASES[f"fullscale_{full}"](), _ref(f"fullscale_{full}")
    assert c["fullscale"] == full
    cells = (full + 1) ** 3
    assert (cells <= C.REVOX_MAX_CELLS) == (full <= 31) and (full != 31 or cells == C.REVOX_MAX_CELLS)
    assert ref["voxel_coords"][:, 1:].max() == full - 1, "the last cell of the grid is used"


@pytest.mark.parametrize("name", [k for k in C.BUILD_CASES if k not in C.NONE_CASES])
def test_coarse_rows_are_the_rulebook_builders_level_count(name):
    c, ref = C.BUILD_CASES[name](), _ref(name)
    assert ref["coarse"] == rulebook_ref.level_counts(ref["voxel_coords"], [c["fullscale"]] * 3, ref["P"], 1)[0]
    half = np.unique(np.concatenate([ref["voxel_coords"][:, :1], ref["voxel_coords"][:, 1:] // 2], axis=1), axis=0).shape[0]
    assert ref["coarse"] == half if c["fullscale"] % 2 == 0 else ref["coarse"] <= half


# ------------------------------------------------------------------------------------------------ build against torch
def _torch_stage(c):
    from gapartnet_amd import backend
    from gapartnet_amd.network.model import GAPartNet
    from oracle import torch_ops
    me = types.SimpleNamespace(use_fused_proposals=False, ball_query_radius=c["radius"], max_num_points_per_query=c["K1"],
                               max_num_points_per_query_shift=c["K2"], min_num_points_per_proposal=c["min_points"],
                               score_fullscale=c["fullscale"], score_scale=c["max_scale"],
                               revoxelize_jitter=tuple(torch.from_numpy(j) for j in c["jitter"]))
    N = c["points"].shape[0]
    inst = None if c["instance_labels"] is None else torch.from_numpy(c["instance_labels"].copy())
    with backend.using(torch_ops):
        return GAPartNet.proposal_clustering_and_revoxelize(
            me, torch.from_numpy(np.array(c["points"], order="C")),torch.from_numpy(c["batch_indices"].copy()), torch.zeros(N, 1),
            torch.from_numpy(c["sem_preds"].copy()), torch.from_numpy(c["offset_preds"].copy()), inst, batch_size=c["batch_size"])


@pytest.mark.parametrize("name", list(C.BUILD_CASES))
def test_build_equals_the_torch_formulation(name):
    c = C.BUILD_CASES[name]()
    ref = _ref(name, "true")
    vt, pid, props = _torch_stage(c)
    if ref is None:
        assert props is None
        return
    got = dict(valid_mask=props.valid_mask, valid_indices=props.valid_indices, sorted_indices=props.sorted_indices,
               proposal_indices=props.proposal_indices, batch_indices=props.batch_indices, pt_xyz=props.pt_xyz,
               sem_preds=props.sem_preds, instance_labels=props.instance_labels, sizes=props.num_points_per_proposal,
               proposal_offsets=props.proposal_offsets)
    got = {k: None if v is None else v.numpy() for k, v in got.items()}
    R.assert_tables_equal(got, {k: ref[k] for k in got})
    assert np.array_equal(got["valid_indices"][got["sorted_indices"]], ref["point_indices"])
    # voxel cells: equal, except points a float64 evaluation of the frame puts within 1e-3 of a cell face
    pid, coords = pid.numpy(), vt.indices.numpy()
    assert (pid >= 0).all() and ref["dropped"] == 0
    differ = (coords[pid] != ref["voxel_coords"][ref["pc_voxel_id"]]).any(1)
    if differ.any():
        off = ref["proposal_offsets"]
        near = np.zeros_like(differ)
        for p in range(ref["P"]):
            s = R.frame64(ref["pt_xyz"][off[p]:off[p + 1]], c["fullscale"], c["max_scale"], c["jitter"])
            near[off[p]:off[p + 1]] = (np.abs(s - np.round(s)) < 1e-3).any(1)
        assert not (differ & ~near).any(), f"row {int(np.flatnonzero(differ & ~near)[0])}: a cell differs away from every face"
        assert differ.sum() <= 0.01 * ref["M"], (int(differ.sum()), ref["M"])
    else:
        order, starts = vt.point_csr
        R.assert_tables_equal(dict(voxel_coords=coords, pc_voxel_id=pid, point_order=order.numpy(), voxel_point_start=starts.numpy(),
                                   V=coords.shape[0]),
                              {k: ref[k] for k in ("voxel_coords", "pc_voxel_id", "point_order", "voxel_point_start", "V")})


# ------------------------------------------------------------------------------------------------ the post-processing cases
@pytest.mark.parametrize("name", list(C.POST_CASES))
def test_postprocess_tables_are_consistent(name):
    c = C.POST_CASES[name]()
    N, slot = c["N"], c["member_slot"]
    M = c["point_indices"].shape[0]
    for which in range(2):
        s = slot[which * N:(which + 1) * N]
        rows = s[s >= 0]
        assert np.array_equal(c["point_indices"][rows], np.flatnonzero(s >= 0)) and (rows < M).all()
    assert c["proposal_offsets"][c["live"] or len(c["score"])] == M
    assert (np.diff(c["proposal_indices"]) >= 0).all() and c["proposal_indices"].max() < (c["live"] or len(c["score"]))
    if "want_kept" in c:
        assert _post_ref(name)["kept_ids"].tolist() == c["want_kept"]


def test_strict_cases_sit_on_their_thresholds():
    c = C.POST_CASES["strict_score"]()
    assert c["score"][0] == np.float32(c["score_thr"]) and c["score"][2] < c["score"][0] < c["score"][1]
    c = C.POST_CASES["strict_size"]()
    assert c["sizes"].tolist() == [c["min_points"], c["min_points"] + 1, c["min_points"] - 1]
    at, below = C.POST_CASES["strict_iou_at"](), C.POST_CASES["strict_iou_below"]()
    iou = R.iou32(5, 10, 10)
    assert np.float32(at["iou_thr"]) == iou and np.nextafter(np.float32(below["iou_thr"]), np.float32(1)) == iou
    assert _post_ref("strict_iou_at")["kept_ids"].tolist() == [0, 1] and _post_ref("strict_iou_below")["kept_ids"].tolist() == [0]


def test_chain_needs_forty_rounds():
    """a proposal is decided one round after its higher-scored neighbour: depth of the dependency chain"""
    c, ref = C.POST_CASES["chain_40"](), _post_ref("chain_40")
    order = np.argsort(-c["score"], kind="stable")
    assert order.tolist() == [v for j in range(40) for v in (j, 40 + j)], "alternating between the sets"
    assert ref["kept_ids"].tolist() == list(range(40)) and ref["_max_neighbours"] == 2
    assert len(order) // 2 >= 40


def test_ties_and_equal_scores():
    c = C.POST_CASES["ties"]()
    assert len(set(c["score"].tolist())) == 1
    assert len(set(C.POST_CASES["p_1025"]()["score"].tolist())) < 20, "the random cases have ties too"


def test_one_set_only_has_points_without_a_row_in_the_other_set():
    c = C.POST_CASES["one_set_only"]()
    a, b = c["member_slot"][:c["N"]], c["member_slot"][c["N"]:]
    assert ((a >= 0) & (b < 0)).any() and ((a < 0) & (b < 0)).any() and ((a >= 0) & (b >= 0)).any()


@pytest.mark.parametrize("n", [32, 33])
def test_neighbour_cases_sit_on_the_table(n):
    c, ref = C.POST_CASES[f"neighbours_{n}"](), _post_ref(f"neighbours_{n}")
    assert ref["_max_neighbours"] == n == c["degree"] and c["iou_thr"] == 0.0 and C.MAX_NBR == 32
    assert c["expect"] == ("equal" if n == 32 else "none")


@pytest.mark.parametrize("name,n", [("sharers_64", 64), ("sharers_65", 65), ("sharers_65_filtered", 65)])
def test_sharer_cases_sit_on_the_table(name, n):
    c, ref = C.POST_CASES[name](), _post_ref(name)
    ids = R.sharers(c["proposal_offsets"], c["point_indices"], c["proposal_indices"], c["member_slot"], c["hub"])
    assert len(ids) == n and len({i % C.TABLE for i in ids}) == 4, "ids collide modulo the table size: the insert probes"
    assert ref["_max_neighbours"] == 0, "no IoU above the threshold: only the sharers' table is loaded"
    live = sum(1 for i in ids if c["score"][i] > np.float32(c["score_thr"]))
    assert (live < n) == name.endswith("filtered") and (not name.endswith("filtered") or live <= C.TABLE)
    others = max(len(R.sharers(c["proposal_offsets"], c["point_indices"], c["proposal_indices"], c["member_slot"], p))
                 for p in range(1, len(c["score"])))
    assert others <= 2


def test_remaining_named_cases():
    assert _post_ref("none_survive")["kept_ids"].size == 0 and _post_ref("none_survive")["new_offsets"].tolist() == [0]
    for p in (1, 3, 4, 5, 1023, 1024, 1025):
        assert len(C.POST_CASES[f"p_{p}"]()["score"]) == p
    c = C.POST_CASES["live_lt_bound"]()
    assert c["live"] == 37 < len(c["score"]) == 50 and np.isnan(c["score"][37:]).all() and (c["sizes"][37:] > 1 << 39).all()
    for name in C.POST_CASES:
        c, ref = C.POST_CASES[name](), _post_ref(name)
        if c["expect"] == "equal":
            assert ref["_max_neighbours"] <= C.MAX_NBR


@pytest.mark.parametrize("name", list(C.POST_CASES))
def test_postprocess_equals_filter_and_nms_of_the_torch_formulation(name):
    from gapartnet_amd import backend
    from gapartnet_amd.network.grouping_utils import apply_nms, filter_invalid_proposals
    from gapartnet_amd.structure.instances import Instances
    from oracle import torch_ops
    c, ref = C.POST_CASES[name](), _post_ref(name)
    P = c["live"] or len(c["score"])
    M = c["point_indices"].shape[0]
    props = Instances(sorted_indices=torch.from_numpy(c["point_indices"].copy()), point_indices=torch.from_numpy(c["point_indices"].copy()),
                      pt_xyz=torch.arange(M), proposal_offsets=torch.from_numpy(c["proposal_offsets"][:P + 1].copy()),
                      proposal_indices=torch.from_numpy(c["proposal_indices"].copy()),
                      num_points_per_proposal=torch.from_numpy(c["sizes"][:P].copy()), score_preds=torch.from_numpy(c["score"][:P].copy()),
                      ious=torch.arange(P))  # (pt_xyz / ious carry the source row / the proposal id through the selections)
    with backend.using(torch_ops):
        props = filter_invalid_proposals(props, c["score_thr"], c["min_points"])
        if props.score_preds.shape[0]:
            props = apply_nms(props, c["iou_thr"], max_sets=2)
    got = dict(kept_ids=props.ious.numpy(), new_offsets=props.proposal_offsets.numpy(), src_row=props.pt_xyz.numpy())
    R.assert_tables_equal(got, ref)


# ------------------------------------------------------------------------------------------------ the comparison is sharp
def _mutations():
    def slot(r):
        i = int(np.flatnonzero(r["member_slot"] >= 0)[3])
        r["member_slot"][i] += 1

    def order(r):
        r["point_order"][[10, 11]] = r["point_order"][[11, 10]]

    def offsets(r):
        r["proposal_offsets"][2] += 1

    def voxels(r):
        r["V"] += 1
    return dict(member_slot=slot, point_order=order, proposal_offsets=offsets, V=voxels)


@pytest.mark.parametrize("table", list(_mutations()))
def test_assert_tables_equal_rejects_a_single_entry_mutation(table):
    want = _ref("min_points_edges")
    R.assert_tables_equal(copy.deepcopy(want), want)
    got = copy.deepcopy(want)
    _mutations()[table](got)
    with pytest.raises(AssertionError, match="^" + table + ":"):
        R.assert_tables_equal(got, want)


def test_assert_tables_equal_rejects_a_kept_id_and_a_missing_result():
    want = _post_ref("chain_40")
    R.assert_tables_equal(copy.deepcopy(want), want)
    got = copy.deepcopy(want)
    got["kept_ids"][7] += 1
    with pytest.raises(AssertionError, match="^kept_ids: 1 of 40 entries differ, first in row 7 "):
        R.assert_tables_equal(got, want)
    with pytest.raises(AssertionError, match="^result:"):
        R.assert_tables_equal(None, want)
    bits = copy.deepcopy(_ref("min_points_edges"))
    bits["pt_xyz"][5, 1] = np.nextafter(bits["pt_xyz"][5, 1], np.float32(9))
    with pytest.raises(AssertionError, match="^pt_xyz: 1 of .* first in row 5 "):
        R.assert_tables_equal(bits, _ref("min_points_edges"))
