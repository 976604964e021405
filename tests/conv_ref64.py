"""Float64 reference of the sparse convolution (forward, dgrad, wgrad) and the helpers of the conv instantiation tests.

The reference is the plain definition, evaluated in float64 from a rulebook's pair lists: per tap k, out[dst] += in[src] @ W[k]
(the pairs of one tap have distinct destinations).  It shares nothing with the kernels or the CPU oracle but the pair lists
(oracle.rulebook_subm3 / rulebook_down, bit-exact with the GPU's).  Pinned against torch's dense conv3d in
tests/test_conv_instantiations.py.

``kernel_id`` maps a profiler kernel name - demangled or Itanium-mangled - to (family, template arguments)."""
import re

import numpy as np

# ---------------------------------------------------------------------------------------------------- reference


def tap_pairs(pairs):
    """(src, dst, tile_off) of a rulebook -> [(src_k, dst_k)] per tap (tile_off[k] holds absolute offsets into the lists)"""
    src, dst, toff = pairs
    toff = np.asarray(toff)
    out = []
    for k in range(toff.shape[0]):
        a, b = int(toff[k, 0]), int(toff[k, -1])
        out.append((np.asarray(src[a:b], np.int64), np.asarray(dst[a:b], np.int64)))
    return out


def fwd(inp, W, pairs, n_dst):
    """out [n_dst, cout] float64 = sum_k in[src_k] @ W[k] scattered to dst_k; W [K, cin, cout]"""
    x, w = np.asarray(inp, np.float64), np.asarray(W, np.float64)
    out = np.zeros((n_dst, w.shape[2]), np.float64)
    for k, (s, d) in enumerate(tap_pairs(pairs)):
        if s.size:
            out[d] += x[s] @ w[k]  # (destinations of one tap are distinct: no lost updates)
    return out


def dgrad(dout, W, pairs, n_src):
    """din [n_src, cin] float64 = sum_k dout[dst_k] @ W[k]^T scattered to src_k"""
    g, w = np.asarray(dout, np.float64), np.asarray(W, np.float64)
    din = np.zeros((n_src, w.shape[1]), np.float64)
    for k, (s, d) in enumerate(tap_pairs(pairs)):
        if s.size:
            din[s] += g[d] @ w[k].T  # (sources of one tap are distinct as well)
    return din


def wgrad(inp, dout, pairs):
    """dW [K, cin, cout] float64 = sum over the pairs of tap k of in[src]^T dout[dst]"""
    x, g = np.asarray(inp, np.float64), np.asarray(dout, np.float64)
    tp = tap_pairs(pairs)
    dW = np.zeros((len(tp), x.shape[1], g.shape[1]), np.float64)
    for k, (s, d) in enumerate(tp):
        if s.size:
            dW[k] = x[s].T @ g[d]
    return dW


def fwd_rows(inp, W, nbr_rows, rows):
    """the forward at the destination rows ``rows`` only: ``nbr_rows`` [K, len(rows)] = the columns of those rows in a tap-major
    neighbour table (source row or -1), e.g. read from the GPU's table.  -> [len(rows), cout] float64"""
    w = np.asarray(W, np.float64)
    nbr_rows = np.asarray(nbr_rows)
    out = np.zeros((len(rows), w.shape[2]), np.float64)
    for k in range(w.shape[0]):
        have = nbr_rows[k] >= 0
        if have.any():
            out[have] += np.asarray(inp[nbr_rows[k][have]], np.float64) @ w[k]
    return out


def sample_rows(rng, n, count):
    """a seeded sample of destination rows that always holds the first and the last rows (the tile tails)"""
    fixed = np.array([0, 1, 15, 16, n - 17, n - 16, n - 2, n - 1], np.int64)
    fixed = fixed[(fixed >= 0) & (fixed < n)]
    return np.unique(np.concatenate([fixed, rng.choice(n, size=min(count, n), replace=False)]))


# ---------------------------------------------------------------------------------------------------- kernel names
FAMILIES = {
    "spconv_tiles_kernel": "tiles",          # <CB, NT, R, DEV, EP>
    "spconv_msplit_kernel": "msplit",        # <CB, NT, SP, DEV, EP>
    "spconv_fwd_direct_kernel": "direct",    # <KT, CB, DEV, EP>
    "spconv_fwd_split_kernel": "split",      # <KT, CB, SP, DEV>
    "spconv_fwd_kernel": "lockstep",         # <NTW, CW, NS>
    "reduce_partials_kernel": "reduce",      # (no template arguments)
    "spconv_wgrad_lds_kernel": "wgrad",      # <CT, NT>
}
_DEMANGLED = re.compile(r"(?<![A-Za-z0-9_])(" + "|".join(FAMILIES) + r")(?:<([^<>]*)>)?\s*\(")
_MANGLED = re.compile(r"\d+(" + "|".join(FAMILIES) + r")(I(?:L[ib]\d+E)*E)?")


def _arg(tok):
    tok = tok.strip()
    if tok in ("true", "false"):
        return tok == "true"
    return int(tok)


def kernel_id(name):
    """profiler kernel name -> (family, template args) or None for a kernel outside the conv families.
    "void (anonymous namespace)::spconv_msplit_kernel<14, 4, 4, false, false>(float const*, ...)" and
    "_ZN12_GLOBAL__N_120spconv_msplit_kernelILi14ELi4ELi4ELb0ELb0EEEvPKf..." both -> ("msplit", (14, 4, 4, False, False))"""
    m = _DEMANGLED.search(name)
    if m:
        args = m.group(2)
        return FAMILIES[m.group(1)], tuple(_arg(t) for t in args.split(",")) if args else ()
    m = _MANGLED.search(name)
    if m:
        # (the <length><identifier> prefix must be exactly the family's name, not a longer identifier ending in it)
        start = m.start(1)
        digits = re.search(r"(\d+)$", name[:start])
        if digits is None or not digits.group(1).endswith(str(len(m.group(1)))):  # ("_GLOBAL__N_1" + "24spconv_...")
            return None
        args = m.group(2) or ""
        vals = tuple(int(v) if t == "i" else bool(int(v)) for t, v in re.findall(r"L([ib])(\d+)E", args))
        return FAMILIES[m.group(1)], vals
    return None
