"""GPU: the three kernel families of csrc/losses.hip (per-point losses, NPCS loss, proposal score loss; forward and backward)
against the plain float64 references of tests/loss_ref64.py, on the shape and value edges of tests/loss_cases.py, and their
device-counted entry points against the host-counted ones.

Metrics (tests/loss_cases.py): a scalar by |got - ref| / max(|ref|, mean |per-point term|) (the dice value at C = 1, which is the
smoothing constants alone, absolutely); a tensor by max |got - ref| / max |ref|; rows whose reference gradient is exactly zero must
be exactly zero; every result must come out bit-equal a second time.

Tolerance of a quantity = 8 x the largest error of the project's fp32 TORCH formulation of it against float64 over all cases,
measured on the CPU by tests/test_loss_ref_cpu.py (which holds the recorded figures to its measurement), never below 4 fp32
epsilons.  Nothing measured on a kernel enters a tolerance.  The factor 8 is room for device expf / logf / sqrtf, another
summation order and the NPCS kernel's fp32 accumulation inside a wave.

  quantity            fp32 torch error (worst case)           tolerance   largest kernel error on an MI355X (case)
  point.focal         1.45e-07  (equal_offsets)               1.16e-06    8.59e-08 (M2)
  point.dice          9.67e-08  (M32769)                      7.74e-07    4.89e-08 (C3)
  point.dice_c1_abs   1.82e-08  (C1, absolute)                4.77e-07    1.82e-08 (C1)
  point.dist          1.06e-07  (M511)                        8.48e-07    3.97e-08 (third_ignored)
  point.dir           7.67e-08  (one_part)                    6.14e-07    7.67e-08 (one_part)
  point.d_logits      3.75e-07  (M524801)                     3.00e-06    7.60e-07 (scale60)
  point.d_offsets     7.99e-07  (one_part)                    6.39e-06    1.01e-06 (one_part)
  npcs.loss           1.32e-07  (P2049)                       1.06e-06    9.05e-08 (P1024)
  npcs.d_logits       4.29e-07  (sigma003)                    3.43e-06    4.62e-07 (P2049)
  score.loss          6.93e-08  (P 1000, I 64, C1 9)          5.54e-07    4.50e-08 (P 256, I 64)
  score.preds         8.20e-08  (P 1000, I 64, C1 9)          6.56e-07    8.51e-08 (P 256, I 1)
  score.d_logits      1.11e-07  (P 1000, I 2, C1 1)           8.88e-07    1.74e-07 (P 1000, I 64)

The NPCS candidate choice is a discontinuity: a proposal / group whose best two differently-targeted candidates lie within 1e-5
(relative, in float64) is left out of the gradient comparison, its loss value is still compared; test_loss_ref_cpu.py caps these
at 2 % per case (the present cases have none).  Every case is a few MB and no input row is out of range anywhere: a kernel that
reads rows it should not gets different numbers, never a bad address."""
import numpy as np
import pytest
import torch

from tests import loss_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from gapartnet_amd import hip_ops
    return hip_ops


def _dev(a, cuda):
    return torch.tensor(a, device=cuda)   # (a copy: the cases are read-only)


def _check(what, errs):
    for key, e in errs.items():
        print(f"{what} {key}: error {e:.3e}  tolerance {LC.tol(key):.3e}")
    for key, e in errs.items():
        assert e <= LC.tol(key), (what, key, e, LC.tol(key))


# ------------------------------------------------------------------------------------------------ per-point losses
def _point_run(cuda, name):
    from gapartnet_amd import functional as GF
    c = LC.point_case(name)
    logits = _dev(c["logits"], cuda).requires_grad_(True)
    offsets = _dev(c["offsets"], cuda).requires_grad_(True)
    args = (_dev(c["labels"], cuda), _dev(c["gt"], cuda), _dev(c["inst"], cuda), LC.IGNORE)
    assert GF.point_losses_available(logits)
    values = GF.point_losses(logits, offsets, *args)
    weights = _dev(c["weights"], cuda)
    finite = ~torch.isnan(values.detach())   # (a NaN offset loss - no point on a part - takes no part in the objective)
    d_logits, d_offsets = torch.autograd.grad((values[finite] * weights[finite]).sum(), [logits, offsets])
    return values.detach(), d_logits, d_offsets


@pytest.mark.parametrize("name", LC.POINT_CASES)
def test_point_losses_against_float64(cuda, name):
    """M = 1 .. 513 (one workgroup becomes two), 32768 / 32769 (64 / 65 workgroups: the finalize kernel's stride loop), 524288 + 513
    (the 1024-workgroup cap, three points per thread); C = 1 .. 32; saturated and equal logits, offset norms over seven decades,
    zero targets, offsets at the kinks of |o - g| and |o|, a zero weight; all / a third of the rows ignored, no / one point on a part"""
    values, d_logits, d_offsets = _point_run(cuda, name)
    ref = LC.point_ref(name)
    _check(name, LC.point_errors(name, values.cpu(), d_logits.cpu(), d_offsets.cpu()))
    assert LC.zero_rows_stay_zero(d_logits, ref["d_logits"]) and LC.zero_rows_stay_zero(d_offsets, ref["d_offsets"])
    again = _point_run(cuda, name)
    assert torch.equal(values.nan_to_num(7.0), again[0].nan_to_num(7.0)) and torch.equal(d_logits, again[1]) \
        and torch.equal(d_offsets, again[2]), "fixed summation order"
    if name.startswith("all_ignored"):
        assert float(values[0]) == 0.0
    if name == "all_ignored_focal_only":
        assert not d_logits.any() and not d_offsets.any()
    if name in ("all_ignored", "no_part", "C1"):
        assert torch.isnan(values[2:]).all() and not torch.isnan(d_logits).any() and not d_offsets.any()


def test_point_losses_refuse_more_than_32_classes(cuda):
    from gapartnet_amd import functional as GF
    assert GF.point_losses_available(torch.zeros(8, 32, device=cuda))
    assert not GF.point_losses_available(torch.zeros(8, 33, device=cuda))


@pytest.mark.parametrize("name", LC.POINT_METRICS_CASES)
def test_point_losses_with_metrics_are_the_plain_losses(cuda, name):
    from gapartnet_amd import functional as GF
    c = LC.point_case(name)
    args = (_dev(c["logits"], cuda), _dev(c["offsets"], cuda), _dev(c["labels"], cuda), _dev(c["gt"], cuda), _dev(c["inst"], cuda))
    plain = GF.point_losses(*args, LC.IGNORE)
    losses, preds, accu = GF.point_losses_with_metrics(*args, LC.IGNORE)
    assert not torch.isnan(plain).any() and torch.equal(losses, plain)
    assert torch.equal(preds, torch.argmax(args[0], dim=-1))


# ------------------------------------------------------------------------------------------------ NPCS loss
def _sym(cuda):
    sym = dict(LC.npcs_sym())
    sym["sym_of_class"] = sym["sym_of_class"].to(cuda)
    sym["mats"] = sym["mats"].to(cuda)
    return sym


def _npcs_run(cuda, c, sym, p_rows=None, m_rows=None, keep_p=None):
    """keep_p: truncate to the first keep_p proposals (and their points) for a host-counted call"""
    from gapartnet_amd import functional as GF
    offsets = c["offsets"] if keep_p is None else c["offsets"][:keep_p + 1]
    m = None if keep_p is None else int(offsets[-1])
    logits = _dev(c["logits"][:m], cuda).requires_grad_(True)
    loss = GF.npcs_loss(logits, _dev(c["gt"][:m], cuda), _dev(c["sem_preds"][:m], cuda), _dev(c["sem_labels"][:m], cuda),
                        _dev(offsets, cuda), _dev(c["prop"][:m], cuda), sym, p_rows=p_rows, m_rows=m_rows)
    (d_logits,) = torch.autograd.grad(loss * 1.7, [logits])
    return loss.detach(), d_logits


@pytest.mark.parametrize("name", LC.NPCS_CASES)
def test_npcs_loss_against_float64(cuda, name):
    """P = 1 .. 5 and 1023 .. 2049 (`per` = 1, 2, 3 proposals per thread of the finish kernel, partly filled four-wave
    workgroups), proposals of 0 / 1 / 63 .. 129 / 1000 points, predictions 0.03 - 0.3 from a candidate target (up to 19 % of the
    pairs on the quadratic branch), proposals mixing types and groups, exact candidate ties, invalid points, no valid point"""
    c, ref = LC.npcs_case(name), LC.npcs_ref(name)
    sym = _sym(cuda)
    loss, d_logits = _npcs_run(cuda, c, sym)
    _check(name, LC.npcs_errors(name, float(loss), d_logits.cpu() / 1.7))
    assert LC.zero_rows_stay_zero(d_logits, ref["d_logits"])
    again = _npcs_run(cuda, c, sym)
    assert torch.equal(loss, again[0]) and torch.equal(d_logits, again[1]), "fixed summation order"
    if name == "none_valid":
        assert float(loss) == 0.0 and not d_logits.any()


# ------------------------------------------------------------------------------------------------ score loss
def _score_run(cuda, c, rows=None, keep_p=None):
    from gapartnet_amd import functional as GF
    p = c["logits"].shape[0] if keep_p is None else keep_p
    logits = _dev(c["logits"][:p], cuda).requires_grad_(True)
    assert GF.score_loss_available(logits)
    loss, preds = GF.score_loss(logits, _dev(c["cls"], cuda), _dev(c["offsets"][:p + 1], cuda), _dev(c["ious"][:p], cuda),
                                LC.FG, LC.BG, rows=rows)
    assert not preds.requires_grad
    (d_logits,) = torch.autograd.grad(loss * 1.7, [logits])
    return loss.detach(), preds, d_logits


@pytest.mark.parametrize("case", LC.SCORE_CASES, ids=lambda c: "P{}-I{}-C{}-{}-{}".format(c[0], c[1], c[2], "i64" if c[3] else "i32", c[4]))
def test_score_loss_against_float64(cuda, case):
    """P around the workgroup's 256 threads, I = 1 / 2 / 64, C1 = 1 / 9, both class dtypes; logits N(0, 3) and +-1e-4 .. +-100; IoU row
    maxima exactly on both thresholds (targets 1 and 0 through the linear branch); a class outside 1..C1: the loss is NaN, that
    proposal's gradient row exactly zero, every other row as without it"""
    c, ref = LC.score_case(*case), LC.score_ref(*case)
    loss, preds, d_logits = _score_run(cuda, c)
    _check(str(case), LC.score_errors(case, float(loss), preds.cpu(), d_logits.cpu() / 1.7))
    assert LC.zero_rows_stay_zero(d_logits, ref["d_logits"])
    assert bool((d_logits.cpu()[ref["d_logits"] == 0] == 0).all()), "only the column of the proposal's class carries a gradient"
    again = _score_run(cuda, c)
    assert torch.equal(loss.nan_to_num(7.0), again[0].nan_to_num(7.0)) and torch.equal(preds, again[1]) and torch.equal(d_logits, again[2])
    if case[4] is not None:
        assert bool(ref["bad"].any()) and np.isnan(float(loss)) and not d_logits.cpu()[ref["bad"]].any()


# ------------------------------------------------------------------------------------------------ device-counted entry points
def _count(H, cuda, live, plan):
    return H.DevCount(torch.tensor([live], dtype=torch.int64, device=cuda), plan)


def _plans(live, bound):
    return sorted({0, 1, live, bound})


def _npcs_dev_check(H, cuda, c, sym, live, plans):
    bound_p, bound_m = len(c["offsets"]) - 1, c["logits"].shape[0]
    m_live = int(c["offsets"][live])
    want = _npcs_run(cuda, c, sym, keep_p=live) if live else None
    for plan in plans:
        m_plan = {0: 0, 1: 1, live: m_live, bound_p: bound_m}[plan]
        loss, d_logits = _npcs_run(cuda, c, sym, p_rows=_count(H, cuda, live, plan), m_rows=_count(H, cuda, m_live, m_plan))
        if live == 0:   # (no host-counted call on zero proposals exists: the two facts directly)
            assert float(loss) == 0.0 and d_logits[:m_live].numel() == 0, plan
        else:
            assert torch.equal(loss, want[0]) and torch.equal(d_logits[:m_live], want[1]), plan


@pytest.mark.parametrize("live", [0, 1, 700, 1500])
def test_device_counted_npcs_loss(H, cuda, live):
    """gpn_npcs_loss_fwd_dev / gpn_npcs_loss_bwd_dev, bound 1500 proposals of 1 - 8 points: `plan` only sizes grids, so for every plan
    the loss and the live gradient rows are those of the host-counted call on the truncated inputs, bit for bit"""
    c = LC.npcs_dev_case(1500, 1, 9, LC.N_CLS3)
    _npcs_dev_check(H, cuda, c, _sym(cuda), live, _plans(live, 1500))


def test_device_counted_npcs_loss_strides(H, cuda):
    """bound 6000 proposals / about 300k points, 5500 live, plan 1: above the 1024-workgroup floor of the device-counted grids in both
    kernels (4096 proposals, 262144 points), so waves and threads really walk their grid-stride loops"""
    c = LC.npcs_dev_case(6000, 40, 61, 6)
    live = 5500
    assert live > 4096 and int(c["offsets"][live]) > 262144
    _npcs_dev_check(H, cuda, c, _sym(cuda), live, [1])


@pytest.mark.parametrize("live", [0, 1, 600, 1000])
@pytest.mark.parametrize("is64", [True, False])
def test_device_counted_score_loss(H, cuda, live, is64):
    """gpn_score_loss_dev, bound 1000 proposals: loss, scores and gradient rows of the live proposals are those of the host-counted
    call on the truncated inputs; no live proposal gives loss 0"""
    bound = 1000
    c = LC.score_case(bound, 64, 9, is64, None)
    want = _score_run(cuda, c, keep_p=live) if live else None
    for plan in _plans(live, bound):
        loss, preds, d_logits = _score_run(cuda, c, rows=_count(H, cuda, live, plan))
        if live == 0:
            assert float(loss) == 0.0, plan
        else:
            assert torch.equal(loss, want[0]) and torch.equal(preds[:live], want[1]) and torch.equal(d_logits[:live], want[2]), plan
