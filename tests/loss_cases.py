"""Inputs for the loss kernels of csrc/losses.hip at their shape and value edges, their float64 references (tests/loss_ref64.py),
the error metrics and the tolerances.

Shared by tests/test_loss_ref_cpu.py (references == the project's torch formulations in float64; error of those formulations in
fp32 = the basis of the tolerances; the input conditions) and tests/test_gpu_losses.py (HIP kernels vs the references on the very
same inputs).  Every case and every reference is built once per process (lru_cache) and must be treated as read-only."""
import functools

import numpy as np
import torch

from tests import loss_ref64 as R

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
IGNORE = -100


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ------------------------------------------------------------------------------------------------ metrics
def scalar_err(got, ref, scale):
    """|got - ref| / max(|ref|, scale); scale = the mean absolute per-point term (the natural size of a mean of signed terms)"""
    return abs(float(got) - float(ref)) / max(abs(float(ref)), float(scale), 1e-300)


def tensor_err(got, ref, floor=0.0):
    """max |got - ref| / max(max |ref|, floor) (0 / 0 = 0): relative to the tensor's largest entry, not element-wise"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    if ref.numel() == 0:
        return 0.0
    top = max(float(ref.abs().max()), floor)
    err = float((got - ref).abs().max())
    return err / top if top > 0 else err


def zero_rows_stay_zero(got, ref):
    """rows whose reference gradient is exactly zero must be exactly zero"""
    got, ref = torch.as_tensor(got).cpu(), torch.as_tensor(ref).cpu()
    rows = (ref == 0).all(dim=1)
    return bool((got[rows] == 0).all())


# ------------------------------------------------------------------------------------------------ tolerances
# Largest error of the project's fp32 torch formulations (CPU) against the float64 references over all cases of a quantity, as
# tests/test_loss_ref_cpu.py measures and prints it (that test fails if a measurement leaves [recorded / 4, recorded * 4]).
# Nothing here was measured on a kernel.
FP32_ERR = {
    "point.focal": 1.45e-07,        # equal_offsets
    "point.dice": 9.67e-08,         # M32769
    "point.dice_c1_abs": 1.82e-08,  # C1 (absolute)
    "point.dist": 1.06e-07,         # M511
    "point.dir": 7.67e-08,          # one_part
    "point.d_logits": 3.75e-07,     # M524801
    "point.d_offsets": 7.99e-07,    # one_part
    "npcs.loss": 1.32e-07,          # P2049
    "npcs.d_logits": 4.29e-07,      # sigma003
    "score.loss": 6.93e-08,         # P = 1000, I = 64, C1 = 9
    "score.preds": 8.20e-08,        # P = 1000, I = 64, C1 = 9
    "score.d_logits": 1.11e-07,     # P = 1000, I = 2, C1 = 1
}


def tol(key):
    """8 x the fp32 torch formulation's own error (device expf / logf / sqrtf, another summation order, fp32 accumulation inside
    a wave), never below 4 fp32 epsilons"""
    return max(8.0 * FP32_ERR[key], 4.0 * EPS32)


# ------------------------------------------------------------------------------------------------ per-point losses
POINT_M = [1, 2, 255, 256, 257, 511, 512, 513, 32768, 32769, 524288 + 513]   # at C = 10
POINT_C = [1, 2, 3, 10, 31, 32]                                               # at M = 3000
POINT_VALUES = ["scale20", "scale60", "equal_rows", "lognorm", "zero_targets", "equal_offsets", "weight_zero"]
POINT_SELECTIONS = ["all_ignored", "all_ignored_focal_only", "third_ignored", "no_part", "one_part"]
POINT_CASES = [f"M{m}" for m in POINT_M] + [f"C{c}" for c in POINT_C] + POINT_VALUES + POINT_SELECTIONS
POINT_METRICS_CASES = ["M257", "M32769", "C32"]


@functools.lru_cache(maxsize=None)
def point_case(name):
    """-> dict(logits [M, C] f32, offsets [M, 3] f32, labels [M] i64, gt [M, 3] f32, inst [M] i32, weights [4] f32)
    base: logits 2 N(0,1), offsets and targets 0.1 N(0,1), labels uniform in [0, C), instance labels in [-1, 6), the first point
    on a part whenever C > 1"""
    M, C = 3000, 10
    if name[0] == "M" and name[1:].isdigit():
        M = int(name[1:])
    elif name[0] == "C" and name[1:].isdigit():
        C = int(name[1:])
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    scale = {"scale20": 20.0, "scale60": 60.0}.get(name, 2.0)
    logits = (rng.standard_normal((M, C)) * scale).astype(f32)
    offsets = (rng.standard_normal((M, 3)) * 0.1).astype(f32)
    gt = (rng.standard_normal((M, 3)) * 0.1).astype(f32)
    labels = rng.integers(0, C, M).astype(np.int64)
    inst = rng.integers(-1, 6, M).astype(np.int32)
    if C > 1:
        labels[0], inst[0] = C - 1, 0
    weights = np.array([0.7, 1.3, 0.9, 1.1], f32)
    if name == "equal_rows":            # softmax exactly uniform, also at a large common value
        logits[::4] = 0.0
        logits[1::8] = f32(37.5)
    elif name == "lognorm":             # norms log-uniform over 1e-7 .. 1: the + 1e-8 of the direction loss matters
        for a in (offsets, gt):
            d = rng.standard_normal((M, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            a[:] = (d * 10.0 ** rng.uniform(-7, 0, (M, 1))).astype(f32)
    elif name == "zero_targets":
        gt[::3] = 0.0
    elif name == "equal_offsets":       # |o - g| at its kink (sign 0) and |o| at its kink (subgradient 0)
        offsets[::4] = gt[::4]
        offsets[1::4] = 0.0
    elif name == "weight_zero":
        weights[2] = 0.0
    elif name in ("all_ignored", "all_ignored_focal_only"):
        labels[:] = IGNORE
        if name.endswith("focal_only"):
            weights = np.array([1.3, 0.0, 0.0, 0.0], f32)
    elif name == "third_ignored":
        labels[::3] = IGNORE
    elif name == "no_part":
        inst[labels > 0] = -1
    elif name == "one_part":
        inst[:] = -1
        inst[M // 2], labels[M // 2] = 3, 4
        # (roughly aligned with its target: a lone direction term near cos = 0 would itself be a cancellation)
        offsets[M // 2] = f32(1.5) * gt[M // 2] + f32(0.01)
    return _frozen(dict(logits=logits, offsets=offsets, labels=labels, gt=gt, inst=inst, weights=weights))


@functools.lru_cache(maxsize=None)
def point_ref(name):
    c = point_case(name)
    return R.point_losses_ref(c["logits"], c["offsets"], c["labels"], c["gt"], c["inst"], IGNORE, c["weights"])


POINT_VALUE_KEYS = ["point.focal", "point.dice", "point.dist", "point.dir"]


def point_errors(name, values, d_logits, d_offsets):
    """-> {tolerance key: error} of one result against the float64 reference; NaN values must be NaN on both sides (error 0,
    else inf); the dice value at C = 1 is a difference of numbers near 1 and is compared absolutely"""
    ref = point_ref(name)
    C = point_case(name)["logits"].shape[1]
    out = {}
    for k, key in enumerate(POINT_VALUE_KEYS):
        got, want = float(values[k]), float(ref["values"][k])
        if np.isnan(want) or np.isnan(got):
            out[key] = 0.0 if (np.isnan(want) and np.isnan(got)) else float("inf")
        elif key == "point.dice" and C == 1:
            out["point.dice_c1_abs"] = abs(got - want)
        else:
            out[key] = scalar_err(got, want, ref["scales"][k])
    # every row ignored: the dice term of a class-less row is constant in the logits (sum_c p_c = 1), so d logits is zero
    # analytically and what float64 autograd leaves (1e-23) is rounding noise; the error is then taken against the size of a
    # kept row's gradient, the largest weight / M
    case = point_case(name)
    floor = float(np.abs(case["weights"]).max()) / case["logits"].shape[0] if name.startswith("all_ignored") else 0.0
    out["point.d_logits"] = tensor_err(d_logits, ref["d_logits"], floor)
    out["point.d_offsets"] = tensor_err(d_offsets, ref["d_offsets"])
    return out


# ------------------------------------------------------------------------------------------------ NPCS loss
# the tests' own class -> symmetry type table: classes 1..9 cover all five types (class 0 is background)
SYM_OF_CLASS = [0, 1, 3, 3, 2, 0, 3, 2, 4, 1]
N_CLS3 = 27


@functools.lru_cache(maxsize=None)
def npcs_sym():
    from gapartnet_amd.misc.info import get_symmetry_matrix
    return R.npcs_sym_host(get_symmetry_matrix(), SYM_OF_CLASS)


NPCS_SMALL_P = [1, 3, 4, 5]
NPCS_LARGE_P = [1023, 1024, 1025, 2049]      # 1 - 8 points per proposal; `per` = 1, 2, 3 in the finish kernel
NPCS_SIZES = [0, 1, 63, 64, 0, 65, 128, 129, 1000, 0]
NPCS_SIGMAS = {"sigma003": 0.03, "sigma008": 0.08, "sigma03": 0.3}
NPCS_CASES = ([f"P{p}" for p in NPCS_SMALL_P + NPCS_LARGE_P] + ["sizes"] + list(NPCS_SIGMAS)
              + ["mixed", "type0", "type1_axis", "none_valid"])
NPCS_GAP = 1e-5         # a proposal / group whose best two differently-targeted candidates lie closer (relative) is a coin toss
NPCS_MAX_LEFT_OUT = 0.02


def _npcs_build(rng, sizes, sigma, classes, per_point_classes=False, wrong=0.1, zero=0.1, n_cls3=N_CLS3, axis_targets=False):
    sym = npcs_sym()
    sizes = np.asarray(sizes, np.int64)
    P, M = len(sizes), int(sizes.sum())
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    prop = np.repeat(np.arange(P), sizes)
    classes = np.asarray(classes)
    cls = rng.choice(classes, M) if per_point_classes else rng.choice(classes, P)[prop]
    gt = (rng.random((M, 3)) - 0.5).astype(f32)
    gt[np.abs(gt) < 1e-3] = f32(0.25)
    if axis_targets:
        gt[:, :2] = 0.0
    # prediction = (target under candidate j of the point's type) + 0.5 + sigma noise, j chosen per proposal
    mats = sym["mats"].numpy().astype(np.float64)
    types = np.asarray(SYM_OF_CLASS)[cls]
    j = rng.integers(0, 24, P)[prop] % np.asarray(sym["count"])[types]
    S = mats[np.asarray(sym["first"])[types] + j]
    target = np.einsum("na,nab->nb", gt.astype(np.float64), S)
    logits = rng.standard_normal((M, n_cls3)).astype(f32)
    pred = (target + 0.5 + sigma * rng.standard_normal((M, 3))).astype(f32)
    for a in range(3):
        logits[np.arange(M), 3 * (cls - 1) + a] = pred[:, a]
    labels = cls.astype(np.int64).copy()
    bad = rng.random(M) < wrong
    labels[bad] = labels[bad] % int(classes.max()) + 1 if len(classes) > 1 else 0
    gt[rng.random(M) < zero] = 0.0
    return _frozen(dict(logits=logits, gt=gt, sem_preds=cls.astype(np.int32), sem_labels=labels, offsets=offsets,
                        prop=prop.astype(np.int64)))


@functools.lru_cache(maxsize=None)
def npcs_case(name):
    """-> dict(logits [M, 27] f32, gt [M, 3] f32, sem_preds [M] i32, sem_labels [M] i64, offsets [P + 1] i32, prop [M] i64);
    about a tenth of the points have a wrong class and a tenth a zero target"""
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + 5)
    all_classes = np.arange(1, 10)
    if name[0] == "P" and name[1:].isdigit():
        P = int(name[1:])
        sizes = rng.integers(1, 9, P) if P > 100 else rng.integers(5, 60, P)
        return _npcs_build(rng, sizes, 0.08, all_classes)
    if name == "sizes":
        return _npcs_build(rng, NPCS_SIZES, 0.08, all_classes)
    if name in NPCS_SIGMAS:
        return _npcs_build(rng, rng.integers(5, 60, 40), NPCS_SIGMAS[name], all_classes)
    if name == "mixed":         # every proposal mixes classes: types 0 - 2 within group 0, and all three groups
        return _npcs_build(rng, rng.integers(20, 90, 30), 0.08, all_classes, per_point_classes=True)
    if name == "type0":         # two identical candidates: exact ties
        return _npcs_build(rng, rng.integers(5, 60, 20), 0.08, [5])
    if name == "type1_axis":    # targets on the z axis: rotating about z by pi leaves them where they are
        return _npcs_build(rng, rng.integers(5, 60, 20), 0.08, [1, 9], axis_targets=True)
    if name == "none_valid":
        return _npcs_build(rng, rng.integers(5, 60, 20), 0.08, all_classes, wrong=1.1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def npcs_ref(name):
    c = npcs_case(name)
    return R.npcs_loss_ref(c["logits"], c["gt"], c["sem_preds"], c["sem_labels"], c["offsets"], npcs_sym())


def npcs_compared_rows(name):
    """-> (bool [M]: the point's gradient row is compared, number of proposal / groups left out, number with members)
    left out: the float64 gap between the best candidate and the best differently-targeted one is below NPCS_GAP of the best mean"""
    c, ref = npcs_case(name), npcs_ref(name)
    has = ref["members"] > 0
    close = has & (ref["gap"] < NPCS_GAP * ref["best"].nan_to_num(0.0))
    sym = npcs_sym()
    group_of_class = torch.tensor([sym["group"][t] for t in SYM_OF_CLASS])
    point_group = group_of_class[torch.tensor(c["sem_preds"], dtype=torch.int64)]
    compared = ~close[torch.tensor(c["prop"]), point_group]
    return compared, int(close.sum()), int(has.sum())


def npcs_errors(name, loss, d_logits):
    ref = npcs_ref(name)
    rows, _, _ = npcs_compared_rows(name)
    scale = float(ref["best"].nan_to_num(0.0).sum() / max(int((ref["members"] > 0).sum()), 1))
    return {"npcs.loss": scalar_err(loss, ref["loss"], scale),
            "npcs.d_logits": tensor_err(torch.as_tensor(d_logits).cpu()[rows], ref["d_logits"][rows])}


@functools.lru_cache(maxsize=None)
def npcs_dev_case(bound, lo, hi, n_cls3):
    """a bound of `bound` proposals of lo .. hi - 1 points for the device-counted entry points: every row is valid data, so the rows
    past a live count differ from the live ones but are in range"""
    rng = np.random.default_rng(bound + hi)
    return _npcs_build(rng, rng.integers(lo, hi, bound), 0.08, np.arange(1, n_cls3 // 3 + 1), n_cls3=n_cls3)


# ------------------------------------------------------------------------------------------------ score loss
FG, BG = 0.75, 0.25
SCORE_SPECIAL = [1e-4, -1e-4, 17.0, -17.0, 40.0, -40.0, 100.0, -100.0]
# (P, I, C1, class source int64, classes outside 1..C1: None / "low" / "high")
SCORE_CASES = [(1, 1, 9, True, None), (1, 2, 1, False, None), (255, 2, 9, False, None), (256, 64, 9, True, None),
               (257, 1, 1, True, None), (1000, 64, 9, False, None), (1000, 2, 1, True, None),
               (257, 2, 9, True, "low"), (256, 1, 9, False, "high")]
SCORE_THRESHOLD_MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def score_case(P, I, C1, is64, bad):
    """-> dict(logits [P, C1] f32, cls [M] i64 / i32 (class of every proposal point), offsets [P + 1] i32, ious [P, I] f32,
    exact [P] i8: 1 / 2 where the row maximum is exactly fg / bg).  Logits N(0, 3); every fifth row holds one of SCORE_SPECIAL;
    rows 2, 12, 22.. have the maximum exactly 0.75, rows 7, 17, .. exactly 0.25; every other maximum keeps 1e-3 from both"""
    rng = np.random.default_rng(1000 * P + 10 * I + C1)
    sizes = rng.integers(1, 5, P)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cls = rng.integers(1, C1 + 1, int(sizes.sum())).astype(np.int64 if is64 else np.int32)
    if bad:
        for p in range(3, P, 50):
            cls[offsets[p]] = 0 if bad == "low" else C1 + 1
    logits = (rng.standard_normal((P, C1)) * 3).astype(f32)
    # (a single proposal takes +-1e-4 only: a lone saturated term is a loss of 1e-8, which no fp32 formulation resolves)
    for p in range(0, P, 5):
        logits[p] = f32(SCORE_SPECIAL[(p // 5 + P + I) % (2 if P == 1 else len(SCORE_SPECIAL))])
    ious = rng.random((P, I)).astype(f32)
    ious[::3] *= f32(0.2)
    ious[1::3, 0] = f32(0.9)
    exact = np.zeros(P, np.int8)
    if P > 1:
        for first, thr, mark in ((2, FG, 1), (7, BG, 2)):
            rows = np.arange(first, P, 10)
            ious[rows] = np.minimum(ious[rows], f32(thr))
            ious[rows, I - 1] = f32(thr)
            exact[rows] = mark
    top = ious.max(axis=1)
    near = (exact == 0) & ((np.abs(top - f32(FG)) < 2 * SCORE_THRESHOLD_MARGIN) | (np.abs(top - f32(BG)) < 2 * SCORE_THRESHOLD_MARGIN))
    ious[near] *= f32(0.9)
    return _frozen(dict(logits=logits, cls=cls, offsets=offsets, ious=ious, exact=exact))


@functools.lru_cache(maxsize=None)
def score_ref(P, I, C1, is64, bad):
    c = score_case(P, I, C1, is64, bad)
    return R.score_loss_ref(c["logits"], c["cls"][c["offsets"][:-1]], c["ious"], FG, BG)


def score_errors(case, loss, preds, d_logits):
    """the loss of a case with a class outside 1..C1 must be NaN (error 0, else inf); its score_preds are compared on the other rows"""
    ref = score_ref(*case)
    good = ~ref["bad"]
    if np.isnan(ref["loss"]):
        e_loss = 0.0 if np.isnan(float(loss)) else float("inf")
    else:
        e_loss = scalar_err(loss, ref["loss"], ref["scale"])
    return {"score.loss": e_loss, "score.preds": tensor_err(torch.as_tensor(preds).cpu()[good], ref["preds"][good]),
            "score.d_logits": tensor_err(d_logits, ref["d_logits"])}
