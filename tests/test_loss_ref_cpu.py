"""No GPU: the float64 loss references of tests/loss_ref64.py against the project's own torch formulations (focal_loss, dice_loss,
the offset formulas, compute_npcs_loss_grouped, get_gt_scores + binary_cross_entropy_with_logits - which tests/golden pins to the
reference project), on the very inputs tests/test_gpu_losses.py gives the kernels (tests/loss_cases.py):

  * run in float64 the formulations agree with the references to 1e-12: a mistake in a new reference shows here;
  * run in fp32 their distance from the references is measured, printed as a table (pytest -s) and held against the recorded
    table loss_cases.FP32_ERR, from which the GPU tolerances are derived - nothing measured on a kernel enters them;
  * the conditions the GPU tolerances rest on: NPCS proposal / groups left out of the gradient comparison (a near-tie between
    differently-targeted candidates), the share of (point, candidate) pairs on the quadratic branch, the distance of the score
    IoUs from the two thresholds."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_cases as LC

AGREE = 1e-12


# ------------------------------------------------------------------------------------------------ the project's formulations
def point_torch(name, dtype):
    """focal_loss + dice_loss + the offset formulas of test_gpu_ops.test_fused_point_losses_match_the_torch_formulas, under the
    fused op's one-label contract (an ignored row is class-less for dice and off-part)"""
    from gapartnet_amd.network.losses import dice_loss, focal_loss
    c = LC.point_case(name)
    logits = torch.tensor(c["logits"], dtype=dtype).requires_grad_(True)
    offsets = torch.tensor(c["offsets"], dtype=dtype).requires_grad_(True)
    gt = torch.tensor(c["gt"], dtype=dtype)
    labels, inst = torch.tensor(c["labels"]), torch.tensor(c["inst"])
    M, C = logits.shape
    keep = labels != LC.IGNORE
    if bool(keep.all()):
        dice = dice_loss(logits[:, :, None, None], labels[:, None, None])
    else:
        y = torch.zeros((M, C), dtype=dtype).scatter_(1, labels.clamp(min=0)[:, None], 1.0) * keep[:, None] + 1e-6
        p = torch.softmax(logits, 1)
        dice = (1 - 2 * (p * y).sum(1) / ((p + y).sum(1) + 1e-8)).mean()
    on = (labels > 0) & (inst >= 0)
    cnt = on.sum()
    zero = offsets.new_zeros(())
    l_dist = torch.where(on, (offsets - gt).abs().sum(-1), zero).sum() / cnt
    gdir = gt / (torch.norm(gt, p=2, dim=-1)[:, None] + 1e-8)
    pdir = offsets / (torch.norm(offsets, p=2, dim=-1)[:, None] + 1e-8)
    l_dir = torch.where(on, -(gdir * pdir).sum(-1), zero).sum() / cnt
    values = torch.stack([focal_loss(logits, labels, gamma=2.0, ignore_index=LC.IGNORE), dice, l_dist, l_dir])
    w = torch.tensor(c["weights"], dtype=dtype)
    finite = ~torch.isnan(values.detach())
    d_logits, d_offsets = torch.autograd.grad((values[finite] * w[finite]).sum(), [logits, offsets], allow_unused=True)
    return values.detach(), d_logits, torch.zeros_like(offsets) if d_offsets is None else d_offsets


def npcs_torch(name, dtype):
    """the selection of network/model.py loss_proposal_npcs + compute_npcs_loss_grouped"""
    from gapartnet_amd.misc.info import get_symmetry_matrix
    from gapartnet_amd.network.grouping_utils import SymmetryTables, compute_npcs_loss_grouped
    c = LC.npcs_case(name)
    logits = torch.tensor(c["logits"], dtype=dtype).requires_grad_(True)
    gt = torch.tensor(c["gt"], dtype=dtype)
    sem_preds, sem_labels = torch.tensor(c["sem_preds"]).long(), torch.tensor(c["sem_labels"])
    valid_idx = torch.nonzero((sem_preds == sem_labels) & (gt != 0).any(dim=-1)).squeeze(1)
    per_class = logits[valid_idx].reshape(valid_idx.shape[0], logits.shape[1] // 3, 3)
    cls = sem_preds[valid_idx]
    preds = per_class.gather(1, (cls - 1)[:, None, None].expand(-1, 1, 3)).squeeze(1)
    tables = SymmetryTables(get_symmetry_matrix(), torch.device("cpu"))
    tables.flat = tables.flat.to(dtype)
    sym = torch.tensor(LC.SYM_OF_CLASS)[cls]
    loss = compute_npcs_loss_grouped(preds, gt[valid_idx], torch.tensor(c["prop"])[valid_idx], sym, tables, len(c["offsets"]) - 1)
    (d_logits,) = torch.autograd.grad(loss, [logits])
    return float(loss.detach()), d_logits


def score_torch(case, dtype):
    """the class selection of network/model.py + get_gt_scores (on the fp32 IoUs: the targets are the floats the reference forms,
    widened) + binary_cross_entropy_with_logits"""
    from gapartnet_amd.network.grouping_utils import get_gt_scores
    c = LC.score_case(*case)
    logits = torch.tensor(c["logits"], dtype=dtype).requires_grad_(True)
    cls = torch.tensor(c["cls"]).long()[torch.tensor(c["offsets"][:-1]).long()]
    sel = logits.gather(1, cls[:, None] - 1).squeeze(1)
    target = get_gt_scores(torch.tensor(c["ious"]).max(-1)[0], LC.FG, LC.BG).to(dtype)
    loss = F.binary_cross_entropy_with_logits(sel, target)
    (d_logits,) = torch.autograd.grad(loss, [logits])
    return float(loss.detach()), sel.detach().sigmoid(), d_logits


GOOD_SCORE_CASES = [c for c in LC.SCORE_CASES if c[4] is None]


# ------------------------------------------------------------------------------------------------ references == formulations
@pytest.mark.parametrize("name", LC.POINT_CASES)
def test_point_reference_is_the_torch_formulation_in_float64(name):
    errs = LC.point_errors(name, *point_torch(name, torch.float64))
    print(name, errs)
    assert all(e <= AGREE for e in errs.values()), errs
    ref, c = LC.point_ref(name), LC.point_case(name)
    if name.startswith("all_ignored"):
        assert float(ref["values"][0]) == 0.0
    if name == "all_ignored_focal_only":
        assert not ref["d_logits"].any() and not ref["d_offsets"].any()
    if name in ("all_ignored", "all_ignored_focal_only", "no_part", "C1"):
        assert torch.isnan(ref["values"][2:]).all() and not torch.isnan(ref["values"][:2]).any()
    if name == "one_part":
        assert int(((c["labels"] > 0) & (c["inst"] >= 0)).sum()) == 1
    if name == "C1":        # the smoothing constants alone
        assert abs(float(ref["values"][1]) + 4.95e-7) < 1e-9


@pytest.mark.parametrize("name", LC.NPCS_CASES)
def test_npcs_reference_is_the_torch_formulation_in_float64(name):
    loss, d_logits = npcs_torch(name, torch.float64)
    ref = LC.npcs_ref(name)
    rows, _, _ = LC.npcs_compared_rows(name)
    errs = {"loss": abs(loss - ref["loss"]) / max(abs(ref["loss"]), 1e-300) if ref["loss"] else abs(loss),
            "d_logits": LC.tensor_err(d_logits[rows], ref["d_logits"][rows])}
    print(name, errs)
    assert all(e <= AGREE for e in errs.values()), errs
    if name == "none_valid":
        assert ref["loss"] == 0.0 and not ref["d_logits"].any()
    if name == "type0":
        assert bool(torch.isinf(ref["gap"]).all())
    if name == "type1_axis":
        assert bool(torch.isinf(ref["gap"][ref["members"] > 0]).all())


@pytest.mark.parametrize("case", GOOD_SCORE_CASES)
def test_score_reference_is_the_torch_formulation_in_float64(case):
    loss, preds, d_logits = score_torch(case, torch.float64)
    errs = LC.score_errors(case, loss, preds, d_logits)
    print(case, errs)
    assert all(e <= AGREE for e in errs.values()), errs


def test_score_targets_are_the_floats_get_gt_scores_forms():
    from gapartnet_amd.network.grouping_utils import get_gt_scores
    from tests.loss_ref64 import score_targets_f32
    for case in LC.SCORE_CASES:
        top = LC.score_case(*case)["ious"].max(axis=1)
        assert np.array_equal(score_targets_f32(top, LC.FG, LC.BG), get_gt_scores(torch.tensor(top), LC.FG, LC.BG).numpy())
    assert score_targets_f32(np.float32([0.75, 0.25]), LC.FG, LC.BG).tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------ the tolerances' basis
@functools.lru_cache(maxsize=None)
def measured_fp32_errors():
    """{tolerance key: (largest error of the fp32 torch formulation over all cases, the case)}"""
    worst = {}

    def note(errs, case):
        for key, e in errs.items():
            if e > worst.get(key, (-1.0, None))[0]:
                worst[key] = (e, case)
    for name in LC.POINT_CASES:
        note(LC.point_errors(name, *point_torch(name, torch.float32)), name)
    for name in LC.NPCS_CASES:
        note(LC.npcs_errors(name, *npcs_torch(name, torch.float32)), name)
    for case in GOOD_SCORE_CASES:
        note(LC.score_errors(case, *score_torch(case, torch.float32)), case)
    return worst


def test_fp32_torch_formulations_lie_this_far_from_float64():
    worst = measured_fp32_errors()
    print("\nquantity              fp32 torch err  (worst case)          recorded    GPU tolerance")
    for key in LC.FP32_ERR:
        e, case = worst[key]
        print(f"{key:<21} {e:>14.3e}  {str(case):<22} {LC.FP32_ERR[key]:>10.3e}  {LC.tol(key):>10.3e}")
    assert set(worst) == set(LC.FP32_ERR)
    for key, recorded in LC.FP32_ERR.items():
        e = worst[key][0]
        assert np.isfinite(e) and e <= 4 * max(recorded, LC.EPS32 / 8), (key, e, recorded)
        # a recorded figure may not sit far above what is measured, unless the floor of 4 epsilons decides the tolerance anyway
        assert e >= recorded / 4 or 8 * recorded <= 4 * LC.EPS32, (key, e, recorded)
        assert LC.tol(key) <= 1e-5, "one to two orders under the earlier 1e-5 / 1e-4"


# ------------------------------------------------------------------------------------------------ input conditions
def test_npcs_near_ties_stay_under_the_cap():
    total_out = total = 0
    for name in LC.NPCS_CASES:
        _, left_out, has = LC.npcs_compared_rows(name)
        print(f"{name}: {left_out} of {has} proposal / groups left out of the gradient comparison")
        assert left_out <= LC.NPCS_MAX_LEFT_OUT * max(has, 1), name
        total_out, total = total_out + left_out, total + has
    print(f"all cases: {total_out} of {total}")


def test_npcs_cases_reach_the_quadratic_branch_and_the_shapes():
    share = {}
    for name in LC.NPCS_CASES:
        n, quad = LC.npcs_ref(name)["pairs"]
        share[name] = quad / max(n, 1)
        print(f"{name}: {100 * share[name]:.2f} % of {n} (point, candidate) pairs have d2 <= 0.01")
    assert share["sigma003"] > 0.02 and share["sigma008"] > 0.02
    sizes = np.diff(LC.npcs_case("sizes")["offsets"])
    assert sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1] and {1, 63, 64, 65, 128, 129, 1000} <= set(sizes.tolist())
    # mixed: proposals whose members span types inside group 0 and several groups
    ref, c = LC.npcs_ref("mixed"), LC.npcs_case("mixed")
    assert int(((ref["members"] > 0).sum(1) == 3).sum()) > 0
    types = np.asarray(LC.SYM_OF_CLASS)[c["sem_preds"]]
    first = c["offsets"][0:2]
    assert len(set(types[first[0]:first[1]][types[first[0]:first[1]] < 3].tolist())) > 1
    # proposals without a member exist where proposals are tiny
    assert int(((LC.npcs_ref("P2049")["members"] > 0).sum(1) == 0).sum()) > 0
    assert {int(t) for t in np.asarray(LC.SYM_OF_CLASS)[1:]} == {0, 1, 2, 3, 4}


def test_score_ious_keep_their_distance_from_the_thresholds():
    for case in LC.SCORE_CASES:
        c = LC.score_case(*case)
        top = c["ious"].max(axis=1).astype(np.float64)
        assert np.all(top[c["exact"] == 1] == 0.75) and np.all(top[c["exact"] == 2] == 0.25)
        rest = top[c["exact"] == 0]
        far = min(np.abs(rest - 0.75).min(), np.abs(rest - 0.25).min()) if rest.size else np.inf
        print(case, "exact fg / bg rows:", int((c["exact"] == 1).sum()), int((c["exact"] == 2).sum()), "nearest other:", far)
        assert far >= LC.SCORE_THRESHOLD_MARGIN
        if case[0] > 10:
            assert (c["exact"] == 1).any() and (c["exact"] == 2).any()
            first_cls = c["cls"][c["offsets"][:-1]]
            assert ((first_cls < 1) | (first_cls > case[2])).any() == (case[4] is not None)
