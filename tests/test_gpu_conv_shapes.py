"""Every sparse-conv kernel instantiation against the float64 reference (tests/conv_ref64.py).

A declarative case table (CASES) drives one parametrised test.  A case is one input set - a rulebook kind, a row count and the
channel widths - and the routing knobs it runs under (gpn_spconv_tiles_min_tiles, gpn_spconv_msplit, gpn_spconv_direct_split).
`route` restates the forward dispatch of csrc/spconv_fwd.hip (masked-tile -> masked tap-split -> direct / its tap-split form ->
lock-step) and of the weight gradient, so every route names the kernel instantiations it must launch; the test checks that
they are the ones that ran (torch.profiler), so a change of the dispatch heuristics fails here instead of quietly testing
another kernel.  tests/test_conv_instantiations.py (CPU) checks that the table reaches every instantiation the sources build.

Per case: forward through the one-call pack (conv_fwd) and through gpn_spconv_fwd_ordered in voxel and in tile order, dgrad
(transposed, tap-reversed pack), wgrad in both weight layouts.  Bounds: forward / dgrad max|got - ref| <= 1e-4 max(1, max|ref|),
wgrad <= 1e-4 max|ref|; rows without a pair exactly 0; repeated runs bit-equal; one forward written into a sentinel-filled
buffer must not touch anything past its n_dst x cout elements."""
import math
import os
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import pytest
import torch

import oracle as O
from tests import conv_ref64 as R64
from tests import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4

# ---------------------------------------------------------------------------------------------------- routing (restated)
TILES_CB = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14)
MSPLIT_CB = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14)
DIRECT_CB = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12)
OFF = 1 << 40


@dataclass(frozen=True)
class Knobs:
    min_tiles: int = 4096               # gpn_spconv_tiles_min_tiles
    ms: Tuple[int, int, int] = (1, 0, 0)  # gpn_spconv_msplit(mode, force_nt, force_sp)
    split: Tuple[int, int] = (12000, 0)   # gpn_spconv_direct_split(split4_below_units, split2_below_units)


DEFAULT = Knobs()


def cdiv(a, b):
    return -(-a // b)


def _fits32(K, n, cin, cout):
    return n * 8 * max(cin, cout) * 4 < (1 << 31) and K * n * 4 < (1 << 31)


def cols_per_wave(n_tiles, nt):
    for d in range(min(nt, 7), 0, -1):
        if nt % d == 0 and n_tiles * (nt // d) >= 1536:
            return d
    return 2 if nt % 2 == 0 and n_tiles * (nt // 2) >= 512 else 1


def pick_cut(K, n_tiles, CB, nt, fnt, fsp):
    sp = fsp if fsp in (4, 9) else 4
    if K < sp:
        sp = 4
    c_nt = 1
    for d in (4, 3, 2, 1):
        if nt % d == 0 and n_tiles * (nt // d) >= 384:
            c_nt = d
            break
    if 0 < fnt <= 4 and nt % fnt == 0:
        c_nt = fnt
    while sp == 9 and CB * (1 + c_nt) > 28:
        d = c_nt - 1
        while d > 1 and nt % d:
            d -= 1
        c_nt = d
    return c_nt, sp


def plan_fwd(K, n, cin, cout):
    nt, CB = cout // 16, cin // 16
    tiles = cdiv(n, 16)
    cw = 4 if CB % 4 == 0 else 2 if CB % 2 == 0 else 1
    wpb = 16 if tiles // 16 >= 512 else 8 if tiles // 8 >= 512 else 4
    row_wgs = cdiv(tiles, wpb)
    ntw = 1
    for w in (4, 3, 2):
        if w <= nt and row_wgs * cdiv(nt, w) >= 512:
            ntw = w
            break
    wgs = row_wgs * cdiv(nt, ntw)
    splits = min(cdiv(512, wgs), K) if wgs < 256 and K > 1 else 1
    tps = cdiv(K, splits)
    return ntw, cw, wpb, cdiv(K, tps)


def route(K, n, cin, cout, kn=DEFAULT):
    """the kernel instantiations one forward-form call (gpn_spconv_fwd_ordered) of this shape launches: [(family, args)]"""
    CB, nt = cin // 16, cout // 16
    fits = _fits32(K, n, cin, cout)
    if 1 <= K <= 27 and fits and cdiv(n, 16) >= max(kn.min_tiles, 16) and CB in TILES_CB:
        return [("tiles", (CB, cols_per_wave(cdiv(n, 16), nt), 1, False, False))]
    if kn.ms[0] and K in (27, 8) and fits and CB in MSPLIT_CB:
        c_nt, sp = pick_cut(K, cdiv(n, 16), CB, nt, kn.ms[1], kn.ms[2])
        return [("msplit", (CB, c_nt, sp, False, False))]
    if K in (27, 8, 1) and CB in DIRECT_CB and fits and cdiv(n, 16) >= 16:
        units = cdiv(n, 16) * nt
        if K >= 8 and units < kn.split[0]:
            return [("split", (K, CB, 4, False))]
        if K >= 8 and units < kn.split[1]:
            return [("split", (K, CB, 2, False))]
        return [("direct", (K, CB, False, False))]
    ntw, cw, wpb, splits = plan_fwd(K, n, cin, cout)
    ks = [("lockstep", (ntw, cw, cdiv(cw * ntw, wpb)))]
    return ks + [("reduce", ())] if splits > 1 else ks


def wgrad_chunks(cout):
    """column widths of the <= 128-column pieces hip_ops.conv_wgrad splits a weight gradient into"""
    nt = cout // 16
    n = cdiv(nt, 8)
    return [16 * (nt // n + (1 if i < nt % n else 0)) for i in range(n)]


def route_wgrad(cin, cout):
    return [("wgrad", (min(cin // 16, 4), c // 16)) for c in wgrad_chunks(cout)]


# ---------------------------------------------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Case:
    id: str
    kind: str        # "subm" (K = 27), "down" (K = 8, stride 2; its dgrad is the inverse conv), "ident" (K = 1), "holes" (subm
                     # with some rows cut out of every pair: rows without any pair)
    n: int           # destination rows of the forward (subm / ident / holes: = source rows; down: coarse rows)
    cin: int
    cout: int
    routes: Tuple[Knobs, ...] = (DEFAULT,)
    wgrad: bool = True
    sentinel: bool = False
    large: bool = False   # sampled-row float64 check of the forward only (the 32-bit guard cases)
    seed: int = 0

    @property
    def K(self):
        return {"subm": 27, "holes": 27, "down": 8, "ident": 1}[self.kind]

    @property
    def n_src(self):
        return down_fine_rows(self.n) if self.kind == "down" else self.n

    def expect(self, kn):
        """the instantiations one route must launch: forward, dgrad (the transposed map), wgrad"""
        ks = route(self.K, self.n, self.cin, self.cout, kn)
        if not self.large:
            ks = ks + route(self.K, self.n_src, self.cout, self.cin, kn)
        return ks


def down_fine_rows(n_coarse):
    return sum(1 + i % 8 for i in range(n_coarse))


LOW = Knobs(min_tiles=16)                      # the masked-tile kernel from 16 row tiles
NO_TILES = Knobs(min_tiles=OFF)


def _ms(nt, sp, mode=1):
    return Knobs(min_tiles=OFF, ms=(mode, nt, sp))


def _direct(ways):
    split = {1: (0, 0), 2: (0, OFF), 4: (OFF, 0)}[ways]
    return Knobs(min_tiles=OFF, ms=(0, 0, 0), split=split)


MS_OFF = Knobs(min_tiles=OFF, ms=(0, 0, 0))


def _cases():
    cs = []
    # masked-tile: every CB x every NT cols_per_wave picks (1536 row tiles, cout = 16 NT), k = 1; then k = 27 / 8 and the tile order
    for cb in TILES_CB:
        for nt in range(1, 8):
            cs.append(Case(f"tiles-cb{cb}-nt{nt}", "ident", 1536 * 16 - 7, 16 * cb, 16 * nt, (LOW,), wgrad=cb <= 4 and nt <= 2,
                           sentinel=(cb, nt) == (7, 7), seed=cb * 10 + nt))
    cs.append(Case("tiles-k27-16to224", "subm", 768 * 16 + 3, 16, 224, (LOW,), seed=1))  # NT = 7 at k = 27
    cs.append(Case("tiles-k27-48to64", "subm", 3000, 48, 64, (LOW,), seed=2))
    cs.append(Case("tiles-k8-32to64", "down", 2100, 32, 64, (LOW,), seed=3))
    cs.append(Case("tiles-holes-64to64", "holes", 2500, 64, 64, (LOW,), wgrad=False, seed=4))
    # masked tap-split: every CB x every legal forced (NT, SP) at cout = 192 (12 column tiles: NT 1 - 4 all divide); CB = 14 also at
    # 224 -> 256 (NT = 4) and its unforced cut; k = 8
    for cb in MSPLIT_CB:
        cuts = [(nt, sp) for sp in (4, 9) for nt in (1, 2, 3, 4) if sp == 4 or cb * (1 + nt) <= 28]
        cs.append(Case(f"msplit-cb{cb}", "subm", 300, 16 * cb, 192, tuple(_ms(nt, sp) for nt, sp in cuts) + (_ms(0, 0),),
                       wgrad=cb in (1, 4), sentinel=cb == 14, seed=100 + cb))
    cs.append(Case("msplit-224to256", "subm", 600, 224, 256, (_ms(4, 4), _ms(0, 0), _ms(1, 9)), seed=5))
    cs.append(Case("msplit-k8-96to192", "down", 400, 96, 192, (_ms(0, 0), _ms(3, 4), _ms(4, 4)), seed=6))
    cs.append(Case("msplit-holes-48to96", "holes", 700, 48, 96, (_ms(0, 0),), wgrad=False, seed=7))
    # direct kernel and its 2- / 4-way tap-split forms: every CB x k 27 / 8 / 1 x ways; rows at the 16-tile threshold
    for cb in DIRECT_CB:
        ways = (_direct(1), _direct(2), _direct(4))
        cs.append(Case(f"direct-k27-cb{cb}", "subm", 257, 16 * cb, 48, ways, wgrad=False, sentinel=cb == 12, seed=200 + cb))
        cs.append(Case(f"direct-k8-cb{cb}", "down", 256 + cb, 16 * cb, 32, ways, wgrad=False, seed=220 + cb))
        cs.append(Case(f"direct-k1-cb{cb}", "ident", 255, 16 * cb, 64, (_direct(1),), wgrad=False, seed=240 + cb))
    cs.append(Case("direct-k27-241", "subm", 241, 64, 64, (_direct(1), _direct(4)), seed=8))
    cs.append(Case("direct-holes-32to48", "holes", 600, 32, 48, (_direct(1), _direct(4)), wgrad=False, seed=9))
    # lock-step: input widths outside every list, k = 27 / 8 / 1, tap splits (+ the partial-sum reduce) and not, tiny and ragged row
    # counts, every (NTW, CW, NS) the plan can produce; the model widths below 16 row tiles with the masked tap-split kernel off
    for cin in (144, 176, 208, 240, 256):
        for n in (1, 15, 17, 255, 257):
            cs.append(Case(f"lock-k27-{cin}-n{n}", "subm", n, cin, 16 * (1 + n % 5), wgrad=n == 257, sentinel=n == 17, seed=cin + n))
    cs += [
        Case("lock-k8-144to48", "down", 300, 144, 48, seed=10),
        Case("lock-k8-176to80", "down", 40, 176, 80, seed=11),
        Case("lock-k1-144to80-n4k", "ident", 4000, 144, 80, sentinel=True, seed=12),
        Case("lock-k27-144to32-n4k", "subm", 4100, 144, 32, seed=13),
    ]
    # every (NTW, CW, NS) of the lock-step kernel: NS = ceil(CW NTW / waves per workgroup), 4 / 8 / 16 waves from 65536 / 131072 rows
    for ntw_cw_ns, n, cin, cout in (((2, 1, 1), 2000, 144, 496), ((2, 2, 1), 2000, 224, 496), ((2, 4, 2), 2000, 256, 496),
                                    ((3, 1, 1), 4000, 144, 400), ((3, 2, 2), 4000, 224, 400), ((3, 4, 3), 4000, 256, 400),
                                    ((4, 1, 1), 8000, 144, 272), ((4, 2, 2), 8000, 224, 272), ((4, 4, 4), 8000, 256, 272),
                                    ((1, 2, 1), 300, 224, 16), ((1, 4, 1), 300, 256, 16),
                                    ((2, 4, 1), 66000, 256, 32), ((3, 2, 1), 66000, 224, 48), ((3, 4, 2), 66000, 256, 48),
                                    ((4, 2, 1), 66000, 224, 64), ((4, 4, 2), 66000, 256, 64),
                                    ((3, 4, 1), 132000, 256, 48), ((4, 4, 1), 132000, 256, 64)):
        cs.append(Case("lock-k1-ntw{}-cw{}-ns{}".format(*ntw_cw_ns), "ident", n, cin, cout, (NO_TILES,), wgrad=n <= 8000,
                       seed=500 + n % 997 + cin))
    cs += [
        Case("lock-model-96to96-n200", "subm", 200, 96, 96, (MS_OFF,), seed=33),
        Case("lock-model-64to112-n150", "subm", 150, 64, 112, (MS_OFF,), seed=34),
        Case("lock-model-k8-48to64", "down", 100, 48, 64, (MS_OFF,), seed=35),
        Case("lock-holes-144to48", "holes", 300, 144, 48, wgrad=False, seed=36),
    ]
    # weight gradient: every (CT, NT), cout above 128 (split into <= 128-column pieces)
    for ct in (1, 2, 3, 4):
        for nt in range(1, 9):
            cs.append(Case(f"wgrad-ct{ct}-nt{nt}", "subm", 300, 16 * ct, 16 * nt, seed=300 + ct * 10 + nt))
    cs += [Case("wgrad-64to144", "subm", 400, 64, 144, seed=37), Case("wgrad-64to256", "subm", 400, 64, 256, seed=38),
           Case("wgrad-256to256", "subm", 200, 256, 256, seed=39), Case("wgrad-k8-32to144", "down", 300, 32, 144, seed=40)]
    # the 32-bit offset guards at C = 16, k = 27: the largest n_dst with n_dst 8 16 4 < 2^31 on the masked-tile kernel, one more
    # row on the lock-step kernel
    n_max = (1 << 31) // (8 * 16 * 4) - 1
    cs += [Case("guard-below", "subm", n_max, 16, 16, wgrad=False, large=True, seed=41),
           Case("guard-above", "subm", n_max + 1, 16, 16, wgrad=False, large=True, sentinel=True, seed=42)]
    return cs


CASES = _cases()


def expected_instantiations():
    """{(family, args)} the case table launches (imported by the CPU coverage check)"""
    out = set()
    for c in CASES:
        for kn in c.routes:
            out.update(c.expect(kn))
        if c.wgrad:
            out.update(route_wgrad(c.cin, c.cout))
    return out


# ---------------------------------------------------------------------------------------------------- inputs
def subm_indices(rng, n):
    side = max(4, int(round((4 * n) ** (1 / 3))) + 1)  # ~25 % occupancy: rows with few and with many neighbours
    return synth.random_sparse_indices(rng, 1, [side, side, side], n), [side, side, side]


def down_indices(rng, n_coarse):
    """fine indices whose stride-2 map has exactly n_coarse coarse rows; coarse row i (in key order) gets 1 + i % 8 children"""
    side = max(2, int(round((2 * n_coarse) ** (1 / 3))) + 1)
    coarse = synth.random_sparse_indices(rng, 1, [side] * 3, n_coarse)
    coarse = coarse[np.lexsort((coarse[:, 3], coarse[:, 2], coarse[:, 1], coarse[:, 0]))]
    bits = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)], np.int32)
    fine = []
    for i, c in enumerate(coarse):
        for ch in rng.permutation(8)[: 1 + i % 8]:
            fine.append([c[0], *(2 * c[1:] + bits[ch])])
    return np.array(fine, np.int32), [2 * side] * 3


class Inputs:
    """one input set of a case: host arrays, device tensors and rulebooks, float64 references (computed once)"""

    def __init__(self, case, cuda):
        from gapartnet_amd import hip_ops as H
        rng = np.random.default_rng(case.seed)
        K, cin, cout = case.K, case.cin, case.cout
        self.H = H
        self.case = case
        if case.kind in ("subm", "holes"):
            idx, shape = subm_indices(rng, case.n)
            self.rb = H.rulebook_subm3(torch.from_numpy(idx).to(cuda), shape)
            self.rb_t = self.rb
            if not case.large:
                self.pairs = O.rulebook_subm3(idx, shape)
                self.pairs_t = None
        elif case.kind == "down":
            idx, shape = down_indices(rng, case.n)
            _, _, self.rb, self.rb_t = H.rulebook_down(torch.from_numpy(idx).to(cuda), shape, 1)
            d = O.rulebook_down(idx, shape)
            assert d["out_indices"].shape[0] == case.n and idx.shape[0] == case.n_src
            self.pairs = d["fwd"]
        else:
            n = case.n
            self.rb = self.rb_t = H.rulebook_identity(n, cuda)
            self.pairs = (np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.array([[0, n]], np.int32))
        n_dst, n_src = case.n, case.n_src
        assert self.rb.n_dst == n_dst and self.rb.n_src == n_src
        self.f = rng.normal(size=(n_src, cin)).astype(np.float32)
        self.W = (rng.normal(size=(K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
        self.g = rng.normal(size=(n_dst, cout)).astype(np.float32)
        self.fd, self.Wd, self.gd = (torch.from_numpy(a).to(cuda) for a in (self.f, self.W, self.g))
        if case.kind == "holes":
            self._cut_holes(rng)
        # float64 references
        if case.large:
            self.rows = R64.sample_rows(rng, n_dst, 2048)
            cols = self.rb.nbr[: K * n_dst].view(K, n_dst)[:, torch.from_numpy(self.rows).to(cuda)].cpu().numpy()
            self.ref = R64.fwd_rows(self.f, self.W, cols, self.rows)
            self.empty = None
            return
        if case.kind == "holes":
            self.ref = R64.fwd_rows(self.f, self.W, self.nbr_host, np.arange(n_dst))
            Wt = np.ascontiguousarray(self.W[::-1].transpose(0, 2, 1))
            self.ref_d = R64.fwd_rows(self.g, Wt, self.nbr_host, np.arange(n_dst))
            self.empty, self.empty_d = self.hole_rows, self.hole_rows
            return
        self.ref = R64.fwd(self.f, self.W, self.pairs, n_dst)
        self.ref_d = R64.dgrad(self.g, self.W, self.pairs, n_src)
        src, dst, _ = self.pairs
        self.empty = np.setdiff1d(np.arange(n_dst), dst)
        self.empty_d = np.setdiff1d(np.arange(n_src), src)
        if case.wgrad:
            self.ref_w = R64.wgrad(self.f, self.g, self.pairs)

    def _cut_holes(self, rng):
        """rows D lose every pair, as destination and as source (the table stays the transpose of itself under tap reversal)"""
        K, n = self.case.K, self.case.n
        nbr = self.rb.nbr[: K * n].view(K, n).cpu().numpy().copy()
        D = np.unique(np.concatenate([rng.choice(n, size=max(1, n // 20), replace=False), [0, n - 1]]))
        nbr[:, D] = -1
        nbr[np.isin(nbr, D)] = -1
        self.nbr_host, self.hole_rows = nbr, D
        flat = torch.full((K * n + 1,), -1, dtype=torch.int32)
        flat[: K * n] = torch.from_numpy(nbr.reshape(-1))
        self.rb.nbr = flat.to(self.rb.nbr.device)
        self.rb.nbr_p = self.rb.perm = None


# ---------------------------------------------------------------------------------------------------- checks
def _knobs(L, kn):
    L.gpn_spconv_tiles_min_tiles(kn.min_tiles)
    L.gpn_spconv_msplit(*kn.ms)
    L.gpn_spconv_direct_split(*kn.split)


@pytest.fixture
def routing():
    """sets a route's knobs; the library defaults are restored however the test ends (tests/test_cabi.py asserts them)"""
    from gapartnet_amd import _C
    L = _C.lib()
    try:
        yield lambda kn: _knobs(L, kn)
    finally:
        _knobs(L, DEFAULT)


def _err(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref))) if ref.size else 0.0


def _check(what, got, ref, empty, names, bound=None):
    bound = TOL * max(1.0, float(np.max(np.abs(ref))) if ref.size else 0.0) if bound is None else bound
    e = _err(got, ref)
    assert e <= bound, f"{what}: max|got - ref64| = {e:.3e} > {bound:.3e}; kernels {names}"
    if empty is not None and len(empty):
        assert not np.any(got[empty]), f"{what}: rows without a pair are not 0; kernels {names}"


def _sentinel_fwd(inp, cuda, names):
    """gpn_spconv_fwd_ordered with `out` at the head of a larger sentinel-filled buffer: nothing past n_dst x cout may change"""
    from gapartnet_amd import _C
    from gapartnet_amd._C import i32, i64, ptr, szt
    H, c, rb = inp.H, inp.case, inp.rb
    L = _C.lib()
    packed = H.pack_weights(inp.Wd, 0)
    n_out = c.n * c.cout
    pad = 4096 + 17
    big = torch.empty((n_out + pad,), dtype=torch.float32, device=cuda)
    big.view(torch.int32).fill_(0x7FC0DEAD)  # (a NaN bit pattern no kernel produces)
    ws_bytes = L.gpn_spconv_fwd_ws_bytes(i32(c.K), i64(c.n), i32(c.cin), i32(c.cout))
    ws = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device=cuda)
    rc = L.gpn_spconv_fwd_ordered(ptr(inp.fd), ptr(packed), ptr(rb.nbr), ptr(rb.nbr_p), ptr(rb.perm), i32(c.K), i64(c.n), i32(c.cin),
                                  i32(c.cout), ptr(big), ptr(ws), szt(ws.numel()), H._stream())
    assert rc == 0, L.gpn_last_error().decode()
    tail = big[n_out:].view(torch.int32)
    assert bool((tail == 0x7FC0DEAD).all()), f"forward wrote past the end of its output; kernels {names}"
    return big[:n_out].view(c.n, c.cout)


def _ran(prof):
    ids = set()
    for e in prof.key_averages():
        k = R64.kernel_id(e.key)
        if k is not None:
            ids.add(k)
    return ids


def _run_route(inp, cuda, kn, with_wgrad):
    H, c, rb = inp.H, inp.case, inp.rb
    dgrad_flags = H.PACK_TRANSPOSE | (H.PACK_REVERSE if c.K == 27 else 0)
    out = {}
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        out["fwd"] = H.conv_fwd(inp.fd, inp.Wd, rb)
        out["fwd2"] = H.conv_fwd(inp.fd, inp.Wd, rb)
        out["fwd_ordered"] = H.conv_fwd_ordered(inp.fd, inp.Wd, rb)
        if not c.large:
            if c.kind == "holes":
                out["dgrad"] = H.conv_fwd_ordered(inp.gd, inp.Wd, rb, flags=dgrad_flags)
            else:
                out["dgrad"] = H.conv_dgrad(inp.gd, inp.Wd, rb, inp.rb_t, c.K == 27)
                out["dgrad_ordered"] = H.conv_fwd_ordered(inp.gd, inp.Wd, inp.rb_t, flags=dgrad_flags)
            out["dgrad2"] = H.conv_fwd_ordered(inp.gd, inp.Wd, inp.rb_t, flags=dgrad_flags)
        if with_wgrad:
            out["wgrad"] = H.conv_wgrad(inp.fd, inp.gd, rb)
            out["wgrad2"] = H.conv_wgrad(inp.fd, inp.gd, rb)
            out["wgrad_oki"] = H.conv_wgrad(inp.fd, inp.gd, rb, layout="oki")
        torch.cuda.synchronize()
    return out, _ran(prof)


def _tile_order(inp):
    H, c = inp.H, inp.case
    for rb in {id(inp.rb): inp.rb, id(inp.rb_t): inp.rb_t}.values():
        if rb.perm is None:
            rb.perm, rb.nbr_p = H.tile_order(rb.nbr, rb.K, rb.n_dst)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_conv_instantiation_vs_float64(cuda, routing, case):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    inp = Inputs(case, cuda)
    try:
        for r, kn in enumerate(case.routes):
            routing(kn)
            for ordered in ((False, True) if not case.large and case.kind != "holes" else (False,)):
                if ordered:
                    _tile_order(inp)
                with_wgrad = case.wgrad and r == 0 and not ordered
                expect = set(case.expect(kn)) | (set(route_wgrad(case.cin, case.cout)) if with_wgrad else set())
                out, ran = _run_route(inp, cuda, kn, with_wgrad)
                names = sorted(ran, key=str)
                missing = expect - ran
                assert not missing, f"route {kn}: expected {sorted(missing, key=str)} to run; ran {names}"
                if not ordered:
                    extra = ran - expect
                    assert not extra, f"route {kn}: unexpected conv kernels {sorted(extra, key=str)} (expected {sorted(expect, key=str)})"
                host = {k: v.cpu().numpy() for k, v in out.items()}
                assert torch.equal(out["fwd"], out["fwd2"]), f"forward not bit-reproducible; kernels {names}"
                if case.large:
                    for k in ("fwd", "fwd_ordered"):
                        _check(f"{case.id} {k}", host[k][inp.rows], inp.ref, None, names)
                    nbr = inp.rb.nbr[: case.K * case.n].view(case.K, case.n)
                    lonely = (nbr < 0).all(0)
                    assert not bool((out["fwd"][lonely] != 0).any()), f"rows without a pair are not 0; kernels {names}"
                else:
                    for k in ("fwd", "fwd_ordered"):
                        _check(f"{case.id} {k} ordered={ordered}", host[k], inp.ref, inp.empty, names)
                    for k in ("dgrad", "dgrad_ordered", "dgrad2"):
                        if k in host:
                            _check(f"{case.id} {k} ordered={ordered}", host[k], inp.ref_d, inp.empty_d, names)
                    assert torch.equal(out["dgrad2"], out["dgrad2"].clone()) and torch.equal(
                        out.get("dgrad_ordered", out["dgrad2"]), out["dgrad2"]), f"dgrad not bit-reproducible; kernels {names}"
                if "wgrad" in out:
                    ref_w = inp.ref_w
                    bound = TOL * float(np.max(np.abs(ref_w)))
                    _check(f"{case.id} wgrad", host["wgrad"], ref_w, None, names, bound)
                    _check(f"{case.id} wgrad oki", host["wgrad_oki"], ref_w.transpose(2, 0, 1), None, names, bound)
                    assert torch.equal(out["wgrad"], out["wgrad2"]), f"wgrad not bit-reproducible; kernels {names}"
                    assert torch.equal(out["wgrad"].permute(2, 0, 1), out["wgrad_oki"]), "the two layouts hold the same bits"
                if case.sentinel and not ordered:
                    got = _sentinel_fwd(inp, cuda, names)
                    assert torch.equal(got, out["fwd"] if inp.rb.perm is None else out["fwd_ordered"]), names
    finally:
        del inp
        torch.cuda.empty_cache()


def test_dropin_subm_conv_trains_at_256_output_channels(cuda):
    """spconv.SubMConv3d(64, 256) from the drop-in module: forward and backward (the weight gradient of cout > 128) against float64"""
    from gapartnet_amd.spconv import pytorch as spconv
    rng = np.random.default_rng(77)
    idx, shape = subm_indices(rng, 600)
    conv = spconv.SubMConv3d(64, 256, 3, padding=1, bias=False, indice_key="subm").to(cuda)
    with torch.no_grad():
        conv.weight.normal_(0.0, 1.0 / math.sqrt(27 * 64))
    f = rng.normal(size=(idx.shape[0], 64)).astype(np.float32)
    g = rng.normal(size=(idx.shape[0], 256)).astype(np.float32)
    x = torch.from_numpy(f).to(cuda).requires_grad_(True)
    y = conv(spconv.SparseConvTensor(x, torch.from_numpy(idx).to(cuda), shape, 1)).features
    (y * torch.from_numpy(g).to(cuda)).sum().backward()
    pairs = O.rulebook_subm3(idx, shape)
    W = _dropin_kio(conv.weight.detach().cpu().numpy())
    ref_y, ref_w = R64.fwd(f, W, pairs, idx.shape[0]), R64.wgrad(f, g, pairs)
    _check("drop-in forward", y.detach().cpu().numpy(), ref_y, None, "")
    got_w = _dropin_kio(conv.weight.grad.cpu().numpy())
    _check("drop-in weight gradient", got_w, ref_w, None, "", TOL * float(np.max(np.abs(ref_w))))


def _dropin_kio(w):
    """the drop-in module's weight (any of its layouts with 27 x 64 x 256 elements) as [K, Cin, Cout]"""
    from gapartnet_amd.spconv import pytorch as spconv  # noqa: F401
    if w.shape == (256, 3, 3, 3, 64):
        return np.ascontiguousarray(w.reshape(256, 27, 64).transpose(1, 2, 0))
    if w.shape == (3, 3, 3, 64, 256):
        return np.ascontiguousarray(w.reshape(27, 64, 256))
    raise AssertionError(f"unknown weight layout {w.shape}")
