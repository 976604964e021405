"""An independent restatement of include/gpn.h section AR (articulation from two frames) in plain loops and dicts, one frame pair at
a time: a per-pixel overlap count, a greedy matching whose IoUs are ``fractions.Fraction``s, and a gather by ``np.flatnonzero``
per part.  Nothing here shares code with gapartnet_amd/misc/articulation.py or the kernels."""
from fractions import Fraction

import numpy as np


def member(inst, valid, n):
    """the part of every pixel of one frame as a list: p when valid and 0 <= inst == p < n, else None"""
    out = []
    for p, ok in zip(np.asarray(inst).reshape(-1).tolist(), np.asarray(valid).reshape(-1).tolist()):
        out.append(p if ok != 0 and 0 <= p < n else None)
    return out


def overlap(inst_a, valid_a, n_a, inst_b, valid_b, n_b):
    """-> (inter {(i, j): pixels}, area_a {i: pixels}, area_b {j: pixels}); absent keys are 0"""
    inter, area_a, area_b = {}, {}, {}
    for i, j in zip(member(inst_a, valid_a, n_a), member(inst_b, valid_b, n_b)):
        if i is not None:
            area_a[i] = area_a.get(i, 0) + 1
        if j is not None:
            area_b[j] = area_b.get(j, 0) + 1
        if i is not None and j is not None:
            inter[(i, j)] = inter.get((i, j), 0) + 1
    return inter, area_a, area_b


def match(inter, area_a, area_b, cls_a, cls_b, min_iou):
    """greedy one-to-one matching -> [(i, j, inter, union)] in the order the pairs are taken.  ``cls`` None: all classes equal."""
    eligible = []
    for (i, j), c in inter.items():
        u = area_a[i] + area_b[j] - c
        same = cls_a is None or cls_b is None or int(cls_a[i]) == int(cls_b[j])
        if same and c > 0 and float(c) >= float(min_iou) * float(u):
            eligible.append((i, j, c, u))
    taken, used_a, used_b = [], set(), set()
    while True:
        best = None
        for i, j, c, u in eligible:
            if i in used_a or j in used_b:
                continue
            key = (-Fraction(c, u), i, j)   # the largest IoU, then the smaller i, then the smaller j
            if best is None or key < best[0]:
                best = (key, (i, j, c, u))
        if best is None:
            return taken
        taken.append(best[1])
        used_a.add(best[1][0])
        used_b.add(best[1][1])


def tables(inst_a, valid_a, n_a, inst_b, valid_b, n_b, PA, PB):
    """the dicts of ``overlap`` as the dense tables of gpn_parts_overlap for one frame pair"""
    inter, area_a, area_b = overlap(inst_a, valid_a, n_a, inst_b, valid_b, n_b)
    ti, ta, tb = np.zeros((PA, PB), np.int32), np.zeros(PA, np.int32), np.zeros(PB, np.int32)
    for (i, j), c in inter.items():
        ti[i, j] = c
    for i, c in area_a.items():
        ta[i] = c
    for j, c in area_b.items():
        tb[j] = c
    return ti, ta, tb


def match_tables(taken, PA, PB):
    """the list of ``match`` as the outputs of gpn_parts_match for one frame pair"""
    ab, ba = np.full(PA, -1, np.int32), np.full(PB, -1, np.int32)
    mi, mu = np.zeros(PA, np.int32), np.zeros(PA, np.int32)
    for i, j, c, u in taken:
        ab[i], ba[j], mi[i], mu[i] = j, i, c, u
    return ab, ba, len(taken), mi, mu


def gather(xyz, inst, valid, n, p):
    """the member pixels of part p of one frame in ascending pixel order: xyz [HW,3] f32 -> [k,3] f64"""
    keys = np.array([-1 if k is None else k for k in member(inst, valid, n)], dtype=np.int64)
    return np.asarray(xyz)[np.flatnonzero(keys == p)].astype(np.float64)


def gather_all(xyz, inst, valid, n):
    """``gather`` for every part of the frame -> {p: [k,3] f64}"""
    keys = np.array([-1 if k is None else k for k in member(inst, valid, n)], dtype=np.int64)
    return {p: np.asarray(xyz)[np.flatnonzero(keys == p)].astype(np.float64) for p in range(n)}
