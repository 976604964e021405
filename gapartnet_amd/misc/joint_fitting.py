"""Joint axis, pivot and angle from two observations of one part, for a batch of pairs (include/gpn.h section JE).

Restates the reference's ``estimate_joint_angle`` (structure/gapartnet.py:819-963): both clouds are normalised by the second
one's mean M and largest extent S, ``sample_number`` rows of each are drawn, the samples are registered rigidly, and the
rotation and translation become an axis direction, a point on the axis and an angle.  The reference registers twice - RANSAC +
Umeyama (``estimate_pose_from_npcs(X, Y)``, :849) and Coherent Point Drift (``pycpd.RigidRegistration``, :862) - and returns the
first when ``visu=True`` and the second otherwise; here both legs are returned, named.

On GPU tensors the work is three launches of csrc/joint.hip (``gpn_joint_sample``, ``gpn_cpd_rigid`` - the whole EM loop of every
pair in one launch, one workgroup a pair - and ``gpn_joint_from_rigid``) plus the two of ``gpn_pose_fit``; nothing is read back
before the results.  On CPU tensors the torch formulation below runs the same contract: it documents the algorithm and is the
same-device baseline of tools/joint_bench.py (the pattern of ``pose_fitting_batched.py``).

CPD rigid (Myronenko & Song 2010, as pycpd runs it with its defaults), row convention TY = s Y R + t:
  start  R = I, t = 0, s = 1, sigma2 = sum_mn |x_n - y_m|^2 / (3 M N), q = diff = inf
  while iteration < max_iterations and diff > tolerance:
    P_mn = exp(-|x_n - TY_m|^2 / (2 sigma2)) / (max(sum_m exp(..), eps) + c),  c = (2 pi sigma2)^(3/2) w / (1 - w) M / N
    Np = sum P, muX = sum_n Pt1_n x_n / Np, muY = sum_m P1_m y_m / Np, A = sum_mn P_mn (x_n - muX)(y_m - muY)^T = U S V^T
    R = (U diag(1, 1, det(U V^T)) V^T)^T, s = tr(A R) / sum_m P1_m |y_m - muY|^2, t = muX - s R^T muY
    q' = (xPx - 2 s tr(A R) + s^2 YPY) / (2 sigma2) + 1.5 Np ln sigma2, diff = |q' - q|
    sigma2 = (xPx - s tr(A R)) / (3 Np), or tolerance / 10 when that is <= 0

Departures from the reference, all stated: a part with fewer than ``sample_number`` points is taken whole (the reference's
``random.sample`` raises); ``joint_type="prismatic"`` reads the translation (the reference accepts the argument and ignores it).
Quirk kept: X and Y are INDEPENDENT samples - row i of X does not correspond to row i of Y - so the RANSAC leg, which fits
correspondences, is only meaningful when the caller passes corresponding ``picks``.
"""
import argparse
import math
import os
import random
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .pose_fitting_batched import draw_picks, estimate_pose_from_npcs_batched

JOINT_COLOUR = (255, 0, 255)
_EPS = float(np.finfo(np.float64).eps)


@dataclass
class JointLeg:
    """one registration's reading of the joint: ``axis`` [B,3], ``pivot`` [B,3] (a point on the axis, camera frame), ``angle`` [B]
    (radians; the displacement for a prismatic joint), and the transform it came from (normalised frame)"""
    axis: torch.Tensor
    pivot: torch.Tensor
    angle: torch.Tensor
    scale: torch.Tensor
    rotation: torch.Tensor
    translation: torch.Tensor


@dataclass
class JointEstimate:
    """``cpd``: the Coherent Point Drift leg (what the reference returns with ``visu=False``); ``ransac``: the RANSAC + Umeyama leg
    (what it returns with ``visu=True``; NaN where that fit found no pose); ``iterations`` [B] i32 and ``sigma2`` [B] of the EM loop;
    ``norm`` [B,4] = (S, Mx, My, Mz)"""
    cpd: JointLeg
    ransac: JointLeg
    iterations: torch.Tensor
    sigma2: torch.Tensor
    norm: torch.Tensor


def draw_joint_picks(sizes1: Sequence[int], sizes2: Sequence[int], sample_number: int = 500):
    """-> (picks1 [B,K] i64, picks2 [B,K] i64, k1 [B] i32, k2 [B] i32), K = sample_number: ``random.sample(range(n), k)`` from
    Python's global generator, pair by pair, set 1 then set 2 - for an equal ``random.seed`` the rows the reference's
    ``random.sample(list(X), k)`` takes.  A part with fewer than ``sample_number`` points is taken whole (k = n; the reference raises)."""
    B, K = len(sizes1), int(sample_number)
    if len(sizes2) != B or K < 1:
        raise ValueError("one size per pair in both lists, and a positive sample_number")
    picks = np.zeros((2, B, K), dtype=np.int64)
    k = np.zeros((2, B), dtype=np.int32)
    for b in range(B):
        for side, n in enumerate((int(sizes1[b]), int(sizes2[b]))):
            k[side, b] = min(n, K)
            picks[side, b, :k[side, b]] = random.sample(range(n), int(k[side, b]))
    return torch.from_numpy(picks[0]), torch.from_numpy(picks[1]), torch.from_numpy(k[0]), torch.from_numpy(k[1])


def _need_hip(what: str):
    from .. import backend
    hip = backend.raw()
    if hip.name != "hip":
        raise RuntimeError(f"{what} on a GPU tensor needs the HIP library as the operator backend")
    return hip


def _maps(inst, what: str) -> torch.Tensor:
    """[V,H,W] (or [H,W], or a sequence of [H,W]) integer tensor"""
    if not torch.is_tensor(inst) and len(inst) > 0 and torch.is_tensor(inst[0]):
        inst = torch.stack(list(inst))
    inst = torch.as_tensor(inst)
    if inst.dim() == 2:
        inst = inst[None]
    if inst.dim() != 3 or inst.dtype.is_floating_point or inst.dtype == torch.bool:
        raise ValueError(f"{what} must be an integer [V,H,W] (or [H,W]) map")
    return inst


def _lists(values, V: int, what: str, cap: Optional[int] = None) -> list:
    """one 1-D tensor per frame (class lists, scores); a single frame may pass its list bare.  ``cap``: the longest list allowed"""
    if torch.is_tensor(values) or isinstance(values, np.ndarray):
        values = [values] if values.ndim == 1 else list(values)
    values = list(values)
    if V == 1 and all(np.ndim(c) == 0 for c in values):  # (a flat list of values, the empty one included)
        values = [values]
    if len(values) != V:
        raise ValueError(f"{what}: {V} frames need {V} lists, got {len(values)}")
    out = [c.reshape(-1) if torch.is_tensor(c) else torch.as_tensor(np.asarray(c).reshape(-1)) for c in values]
    if cap is not None and any(int(c.shape[0]) > cap for c in out):
        raise ValueError(f"{what}: at most {cap} parts a frame, got {max(int(c.shape[0]) for c in out)}")
    return out


# ------------------------------------------------------------------------------------------------------------ sampling
def _joint_sample_torch(pc1s, pc2s, picks1, picks2, k1, k2):
    B, K = picks1.shape
    f64 = torch.float64
    X, Y, norm = torch.zeros(B, K, 3, dtype=f64), torch.zeros(B, K, 3, dtype=f64), torch.zeros(B, 4, dtype=f64)
    for b in range(B):
        p1, p2 = pc1s[b].to(f64), pc2s[b].to(f64)
        if p2.shape[0] == 0:
            norm[b] = float("nan")
            X[b, :int(k1[b])] = float("nan")
            continue
        M = p2.mean(0)
        c = p2 - M
        S = (c.max(0).values - c.min(0).values).max()
        norm[b, 0], norm[b, 1:] = S, M
        X[b, :int(k1[b])] = (p1[picks1[b, :int(k1[b])]] - M) / S
        Y[b, :int(k2[b])] = (p2[picks2[b, :int(k2[b])]] - M) / S
    return X, Y, norm


# ------------------------------------------------------------------------------------------------------------ CPD rigid
def _cpd_rigid_torch(X, Y, nx, ny, max_iterations, tolerance, w, scale, want_trace):
    """the contract of the module docstring on dense [B, M, N] responsibilities, every pair at once; pairs that have stopped keep
    their state (a masked loop until every pair has stopped)"""
    dev, f64 = X.device, torch.float64
    B, K, _ = X.shape
    nan, inf = float("nan"), float("inf")
    ar = torch.arange(K, device=dev)
    mx, my = ar[None, :] < nx[:, None], ar[None, :] < ny[:, None]                    # live columns n / rows m
    pair = (my[:, :, None] & mx[:, None, :]).to(f64)                                 # [B, M, N]
    Nf, Mf = nx.to(f64), ny.to(f64)
    fmx, fmy = mx.to(f64)[:, :, None], my.to(f64)[:, :, None]
    d2 = ((X[:, None, :, :] - Y[:, :, None, :]) ** 2).sum(-1)
    sigma2 = (d2 * pair).sum((1, 2)) / (3.0 * Mf * Nf)
    s = torch.ones(B, dtype=f64, device=dev)
    R = torch.eye(3, dtype=f64, device=dev).repeat(B, 1, 1)
    t = torch.zeros(B, 3, dtype=f64, device=dev)
    q = torch.full((B,), inf, dtype=f64, device=dev)
    diff = torch.full((B,), inf, dtype=f64, device=dev)
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    trace = torch.full((B, max_iterations), nan, dtype=f64, device=dev) if want_trace else None
    degenerate = (nx <= 0) | (ny <= 0)
    active = (diff > tolerance) & ~degenerate
    flip = torch.ones(B, 3, dtype=f64, device=dev)
    k = 0
    while k < max_iterations and bool(active.any()):
        TY = s[:, None, None] * (Y @ R) + t[:, None, :]
        d2 = ((X[:, None, :, :] - TY[:, :, None, :]) ** 2).sum(-1)
        P = torch.exp(-d2 / (2.0 * sigma2)[:, None, None]) * pair
        c = (2.0 * math.pi * sigma2) ** 1.5 * (w / (1.0 - w)) * Mf / Nf
        P = P / (P.sum(1).clamp_min(_EPS) + c[:, None])[:, None, :]
        Pt1, P1 = P.sum(1), P.sum(2)
        Np = P1.sum(1)
        muX = (Pt1[:, :, None] * X).sum(1) / Np[:, None]
        muY = (P1[:, :, None] * Y).sum(1) / Np[:, None]
        Xh, Yh = (X - muX[:, None, :]) * fmx, (Y - muY[:, None, :]) * fmy
        A = Xh.transpose(1, 2) @ (P.transpose(1, 2) @ Yh)
        YPY = (P1 * (Yh * Yh).sum(-1)).sum(1)
        xPx = (Pt1 * (Xh * Xh).sum(-1)).sum(1)
        finite = torch.isfinite(A).all(-1).all(-1)
        U, _, Vh = torch.linalg.svd(torch.where(finite[:, None, None], A, torch.zeros_like(A)))
        flip[:, 2] = torch.linalg.det(U @ Vh)
        Rn = ((U * flip[:, None, :]) @ Vh).transpose(1, 2)
        trAR = (A * Rn.transpose(1, 2)).sum((1, 2))
        sn = trAR / YPY if scale else torch.ones_like(trAR)
        tn = muX - sn[:, None] * (Rn.transpose(1, 2) @ muY[:, :, None]).squeeze(-1)
        qn = (xPx - 2.0 * sn * trAR + sn * sn * YPY) / (2.0 * sigma2) + 1.5 * Np * torch.log(sigma2)
        dn = (qn - q).abs()
        s2n = (xPx - sn * trAR) / (3.0 * Np)
        s2n = torch.where(s2n <= 0, torch.full_like(s2n, tolerance / 10.0), s2n)
        s, q, diff, sigma2 = (torch.where(active, new, old) for new, old in ((sn, s), (qn, q), (dn, diff), (s2n, sigma2)))
        t = torch.where(active[:, None], tn, t)
        R = torch.where(active[:, None, None], Rn, R)
        iters = iters + active.to(torch.int32)
        if want_trace:
            trace[:, k] = torch.where(active, s2n, torch.full_like(s2n, nan))
        active = active & (dn > tolerance)   # (a NaN diff ends the pair's loop: NaN > tolerance is false)
        k += 1
    bad = degenerate
    out = {"s": s.masked_fill(bad, nan), "R": R.masked_fill(bad[:, None, None], nan), "t": t.masked_fill(bad[:, None], nan),
           "sigma2": sigma2.masked_fill(bad, nan), "q": q.masked_fill(bad, nan), "diff": diff.masked_fill(bad, nan), "iterations": iters}
    if want_trace:
        out["sigma2_trace"] = trace
    return out


@torch.no_grad()
def cpd_rigid_batched(X: torch.Tensor, Y: torch.Tensor, nx: torch.Tensor, ny: torch.Tensor, max_iterations: int = 100,
                      tolerance: float = 1e-3, w: float = 0.0, scale: bool = True, want_trace: bool = False,
                      formulation: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """CPD rigid registration of the moving sets Y [B,K,3] (ny[b] rows) onto the fixed sets X [B,K,3] (nx[b] rows) ->
    dict: s [B], R [B,3,3], t [B,3] (TY = s Y R + t), sigma2, q, diff [B], iterations [B] i32 (+ sigma2_trace [B,max_iterations]).
    GPU tensors go to ``gpn_cpd_rigid``; CPU tensors (or ``formulation="torch"``, the bench's baseline) run the torch formulation."""
    if not 0.0 <= w < 1.0:
        raise ValueError("w is in [0, 1)")
    nx, ny = nx.to(X.device), ny.to(X.device)
    if X.is_cuda and formulation != "torch":
        return _need_hip("cpd_rigid_batched").cpd_rigid(X, Y, nx, ny, max_iterations, tolerance, w, scale, want_trace)
    return _cpd_rigid_torch(X.double(), Y.double(), nx.long(), ny.long(), int(max_iterations), float(tolerance), float(w), bool(scale),
                            want_trace)


# ------------------------------------------------------------------------------------------------------------ joint from a transform
def _rotvec_from_matrix(m: torch.Tensor) -> torch.Tensor:
    """[G,3,3] -> [G,3], through the unit quaternion with w >= 0 (scipy's Rotation.from_matrix(..).as_rotvec())"""
    tr = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    choice = torch.stack([m[:, 0, 0], m[:, 1, 1], m[:, 2, 2], tr], 1).argmax(1)
    quat = torch.empty(m.shape[0], 4, dtype=m.dtype, device=m.device)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        cand = torch.empty_like(quat)
        cand[:, i] = 1.0 - tr + 2.0 * m[:, i, i]
        cand[:, j] = m[:, j, i] + m[:, i, j]
        cand[:, k] = m[:, k, i] + m[:, i, k]
        cand[:, 3] = m[:, k, j] - m[:, j, k]
        quat = torch.where((choice == i)[:, None], cand, quat)
    cand = torch.stack([m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1], 1.0 + tr], 1)
    quat = torch.where((choice == 3)[:, None], cand, quat)
    quat = quat / quat.norm(dim=1, keepdim=True)
    quat = torch.where((quat[:, 3] < 0)[:, None], -quat, quat)
    ang = 2.0 * torch.atan2(quat[:, :3].norm(dim=1), quat[:, 3])
    a2 = ang * ang
    sc = torch.where(ang <= 1e-3, 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0, ang / torch.sin(ang / 2.0))
    return sc[:, None] * quat[:, :3]


def _matrix_from_rotvec(rv: torch.Tensor) -> torch.Tensor:
    """[G,3] -> [G,3,3] (scipy's Rotation.from_rotvec(..).as_matrix())"""
    ang = rv.norm(dim=1)
    a2 = ang * ang
    sc = torch.where(ang <= 1e-3, 0.5 - a2 / 48.0 + a2 * a2 / 3840.0, torch.sin(ang / 2.0) / ang)
    x, y, z, w = sc * rv[:, 0], sc * rv[:, 1], sc * rv[:, 2], torch.cos(ang / 2.0)
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    rows = [x2 - y2 - z2 + w2, 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
            2.0 * (x * y + z * w), -x2 + y2 - z2 + w2, 2.0 * (y * z - x * w),
            2.0 * (x * z - y * w), 2.0 * (y * z + x * w), -x2 - y2 + z2 + w2]
    return torch.stack(rows, 1).reshape(-1, 3, 3)


@torch.no_grad()
def joint_from_rigid(rotation: torch.Tensor, translation: torch.Tensor, norm: torch.Tensor,
                     joint_type: str = "revolute") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """rotation [G,3,3], translation [G,3] (normalised frame), norm [G,4] = (S, Mx, My, Mz) -> (axis [G,3], pivot [G,3], angle [G]).
    Revolute (structure/gapartnet.py:850-856): angle = |rotvec|, axis = rotvec / angle (NaN at angle 0, as in the reference),
    r = matrix of the rotation vector (pi/2 - angle/2) axis, pivot = (t r / 2) / sin(angle / 2) * S + M.  Prismatic (an extension):
    axis = t / |t|, angle = |t| S (the displacement), pivot = M."""
    if joint_type not in ("revolute", "prismatic"):
        raise ValueError(f"joint_type is 'revolute' or 'prismatic', got {joint_type!r}")
    if rotation.is_cuda:
        return _need_hip("joint_from_rigid").joint_from_rigid(rotation, translation, norm, joint_type)
    rotation, translation, norm = rotation.double().reshape(-1, 3, 3), translation.double().reshape(-1, 3), norm.double().reshape(-1, 4)
    S, M = norm[:, 0], norm[:, 1:]
    if joint_type == "prismatic":
        length = translation.norm(dim=1)
        return translation / length[:, None], M.clone(), length * S
    rv = _rotvec_from_matrix(rotation)
    angle = rv.norm(dim=1)
    axis = rv / angle[:, None]
    r = _matrix_from_rotvec((math.pi / 2.0 - angle / 2.0)[:, None] * axis)
    half = torch.einsum("gi,gij->gj", translation, r) / 2.0
    pivot = half / torch.sin(angle / 2.0)[:, None] * S[:, None] + M
    return axis, pivot, angle


# ------------------------------------------------------------------------------------------------------------ the whole estimate
@torch.no_grad()
def estimate_joints(pc1s: Sequence[torch.Tensor], pc2s: Sequence[torch.Tensor], sample_number: int = 500, picks=None,
                    ransac_picks: Optional[torch.Tensor] = None, joint_type: str = "revolute", max_iterations: int = 100,
                    tolerance: float = 1e-3, w: float = 0.0) -> JointEstimate:
    """``pc1s[b]`` [n1_b,3], ``pc2s[b]`` [n2_b,3]: one part before and after it moved, B pairs on one device.  ``picks`` = what
    ``draw_joint_picks`` returns (drawn when None); ``ransac_picks`` [B,H,5] = what ``draw_picks`` returns for the RANSAC leg, which
    is ``estimate_pose_from_npcs_batched(xyz=X, npcs=Y)`` - the argument order of structure/gapartnet.py:849 - over the first
    min(k1, k2) sampled rows of each pair (all ``sample_number`` of them unless a part is smaller).  A pair with an empty
    observation gives NaN in both legs and 0 iterations; the other pairs are not affected.  -> ``JointEstimate``."""
    B = len(pc1s)
    if B == 0 or len(pc2s) != B:
        raise ValueError("estimate_joints needs as many first as second observations, at least one")
    if joint_type not in ("revolute", "prismatic"):  # (before any work: the concatenation below is a device copy)
        raise ValueError(f"joint_type is 'revolute' or 'prismatic', got {joint_type!r}")
    f64 = torch.float64
    sizes1, sizes2 = [int(p.shape[0]) for p in pc1s], [int(p.shape[0]) for p in pc2s]
    return estimate_joints_packed(torch.cat([p.to(f64) for p in pc1s]), torch.cat([p.to(f64) for p in pc2s]), sizes1, sizes2,
                                  sample_number, picks, ransac_picks, joint_type, max_iterations, tolerance, w)


@torch.no_grad()
def estimate_joints_packed(pc1: torch.Tensor, pc2: torch.Tensor, sizes1: Sequence[int], sizes2: Sequence[int],
                           sample_number: int = 500, picks=None, ransac_picks: Optional[torch.Tensor] = None,
                           joint_type: str = "revolute", max_iterations: int = 100, tolerance: float = 1e-3,
                           w: float = 0.0) -> JointEstimate:
    """``estimate_joints`` on clouds that are already concatenated: ``pc1`` [sum sizes1, 3], ``pc2`` [sum sizes2, 3] f64, pair b =
    the next ``sizes1[b]`` / ``sizes2[b]`` rows (host ints) - the layout ``gpn_joint_sample`` reads and ``gpn_parts_gather`` writes."""
    B = len(sizes1)
    if B == 0 or len(sizes2) != B:
        raise ValueError("estimate_joints needs as many first as second observations, at least one")
    if joint_type not in ("revolute", "prismatic"):
        raise ValueError(f"joint_type is 'revolute' or 'prismatic', got {joint_type!r}")
    dev = pc1.device
    sizes1, sizes2 = [int(n) for n in sizes1], [int(n) for n in sizes2]
    if picks is None:
        picks = draw_joint_picks(sizes1, sizes2, sample_number)
    picks1, picks2, k1, k2 = picks
    K = int(picks1.shape[1])
    if dev.type == "cuda":
        hip = _need_hip("estimate_joints")
        off = [torch.tensor(np.concatenate([[0], np.cumsum(sz)]), dtype=torch.int64).to(dev, non_blocking=True) for sz in (sizes1, sizes2)]
        X, Y, norm = hip.joint_sample(pc1, pc2, off[0], off[1],
                                      picks1.to(dev, non_blocking=True), picks2.to(dev, non_blocking=True),
                                      k1.to(dev, non_blocking=True), k2.to(dev, non_blocking=True))
    else:
        X, Y, norm = _joint_sample_torch(torch.split(pc1, sizes1), torch.split(pc2, sizes2), picks1, picks2, k1, k2)
    reg = cpd_rigid_batched(X, Y, k1, k2, max_iterations, tolerance, w)
    # ---- the RANSAC leg: rows 0 .. min(k1, k2) of every pair as a ragged batch ----
    # (a pair with an empty observation enters as one padded row: a single-point proposal has no pose, so its leg is NaN, as the
    #  CPD leg of such a pair is by the kernel's contract; the other pairs of the batch are not affected)
    kmin = torch.minimum(k1, k2).long().clamp_min(1)
    if bool((kmin == K).all()):
        xyz, npcs = X.reshape(B * K, 3), Y.reshape(B * K, 3)
    else:
        rows = torch.cat([b * K + torch.arange(int(kmin[b])) for b in range(B)]).to(dev, non_blocking=True)
        xyz, npcs = X.reshape(B * K, 3)[rows], Y.reshape(B * K, 3)[rows]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(kmin, 0)])
    if ransac_picks is None:
        ransac_picks = draw_picks(kmin.tolist())
    fit = estimate_pose_from_npcs_batched(xyz, npcs, offsets, picks=ransac_picks)
    # ---- both legs' transforms -> joints, one call ----
    axis, pivot, angle = joint_from_rigid(torch.cat([reg["R"], fit["rotation"]]), torch.cat([reg["t"], fit["translation"]]),
                                          torch.cat([norm, norm]), joint_type)
    cpd = JointLeg(axis[:B], pivot[:B], angle[:B], reg["s"], reg["R"], reg["t"])
    ransac = JointLeg(axis[B:], pivot[B:], angle[B:], fit["scale"], fit["rotation"], fit["translation"])
    return JointEstimate(cpd, ransac, reg["iterations"], reg["sigma2"], norm)


@torch.no_grad()
def joints_from_frames(depth_a, depth_b, K, mask_a, mask_b, depth_scale: float = 1.0, flip: bool = False, **kwargs) -> JointEstimate:
    """two depth frames [H,W] (or B frame pairs [B,H,W]) and the part's mask in each -> ``estimate_joints`` of the back-projected
    masked pixels: the frame path of section FR with ``keep`` = the mask (xyz are the float32 rows that path produces).  On the GPU
    the valid pixel counts of all frames are read in ONE copy, to size the ragged clouds; the rows are then compacted by a stable
    sort of the validity bytes, which needs no further read.  An empty mask gives that pair NaN.  ``kwargs`` go to ``estimate_joints``."""
    from .. import inference
    sides = []
    for depth, mask in ((depth_a, mask_a), (depth_b, mask_b)):
        depth, _, Kc, keep = inference._check_frames(depth, None, K, torch.as_tensor(mask))
        V, H, W = (int(v) for v in depth.shape)
        rows, valid, counts = inference.backproject_frames(depth, None, Kc, keep.to(depth.device), depth_scale, flip)
        sides.append((rows[:, :3].reshape(V, H * W, 3), valid.reshape(V, H * W).bool(), counts))
    counts = torch.cat([s[2] for s in sides]).tolist()          # the one host read
    clouds = []
    for xyz, valid, _ in sides:
        V = xyz.shape[0]
        first = torch.argsort(~valid, dim=1, stable=True)       # the valid pixels first, in pixel order
        clouds.append([xyz[v][first[v, :counts[len(clouds) * V + v]]].double() for v in range(V)])
    return estimate_joints(clouds[0], clouds[1], **kwargs)


# ------------------------------------------------------------------------------------------------------------ drawing
def project_joint(K, axis, pivot) -> np.ndarray:
    """[2,2] f64 = the (u, v) pixels of pivot - axis and pivot + axis: rint(x fx / z + cx), rint(y fy / z + cy), half to even
    (structure/gapartnet.py:919-928); possibly non-finite"""
    K, axis, pivot = (np.asarray(torch.as_tensor(v).detach().cpu(), dtype=np.float64) for v in (K, axis, pivot))
    ends = np.stack([pivot - axis, pivot + axis])
    with np.errstate(all="ignore"):
        u = np.rint(ends[:, 0] * K[0, 0] / ends[:, 2] + K[0, 2])
        v = np.rint(ends[:, 1] * K[1, 1] / ends[:, 2] + K[1, 2])
    return np.stack([u, v], 1)


def draw_joint(rgb, K, axis, pivot) -> np.ndarray:
    """a copy of ``rgb`` [H,W,3] u8 with the joint drawn as the reference does (:929-930): one line from pivot - axis to pivot +
    axis, colour (255, 0, 255), thickness 2.  Host code: one line per pair, no hot path."""
    from ..inference import _draw_line_numpy
    img = np.array(torch.as_tensor(rgb).detach().cpu().numpy(), dtype=np.uint8, copy=True)
    a, b = project_joint(K, axis, pivot)
    _draw_line_numpy(img, a, b, JOINT_COLOUR, 2)
    return img


# ------------------------------------------------------------------------------------------------------------ command line
def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gapartnet_amd.misc.joint_fitting",
                                 description="joint axis, pivot and angle from two point clouds of one part (before / after it moved)")
    ap.add_argument("--pc1", required=True, help="[n,3] .npy: the part before")
    ap.add_argument("--pc2", required=True, help="[n,3] .npy: the part after")
    ap.add_argument("--rgb", help="image to draw the joint into (.png / .npy)")
    ap.add_argument("--intrinsics", help="3x3 camera matrix as text (needed with --rgb)")
    ap.add_argument("--sample_number", type=int, default=500)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--joint_type", default="revolute", choices=("revolute", "prismatic"))
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--out", required=True, help="output directory")
    args = ap.parse_args(argv)
    if args.rgb and not args.intrinsics:
        ap.error("--rgb needs --intrinsics")
    random.seed(args.seed)
    np.random.seed(args.seed)
    dev = torch.device(args.device)
    pcs = [torch.from_numpy(np.load(p).astype(np.float64).reshape(-1, 3)).to(dev) for p in (args.pc1, args.pc2)]
    est = estimate_joints([pcs[0]], [pcs[1]], sample_number=args.sample_number, joint_type=args.joint_type)
    os.makedirs(args.out, exist_ok=True)
    name = os.path.splitext(os.path.basename(args.pc1))[0]
    got = {"iterations": est.iterations, "sigma2": est.sigma2, "norm": est.norm}
    for leg_name, leg in (("cpd", est.cpd), ("ransac", est.ransac)):
        for field in ("axis", "pivot", "angle", "scale", "rotation", "translation"):
            got[f"{leg_name}_{field}"] = getattr(leg, field)
    path = os.path.join(args.out, f"{name}_joint.npz")
    np.savez(path, **{k: v.detach().cpu().numpy()[0] for k, v in got.items()})
    print(path)
    print(f"cpd: axis {est.cpd.axis[0].tolist()} pivot {est.cpd.pivot[0].tolist()} angle {float(est.cpd.angle[0]):.6f} "
          f"({int(est.iterations[0])} iterations)")
    if args.rgb:
        from ..inference import _read_image
        from PIL import Image
        K = np.loadtxt(args.intrinsics).reshape(3, 3)
        img = draw_joint(_read_image(args.rgb)[..., :3], K, est.cpd.axis[0], est.cpd.pivot[0])
        path = os.path.join(args.out, f"{name}_joint.png")
        Image.fromarray(img).save(path)
        print(path)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
