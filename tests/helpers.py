"""Shared test utilities: patterns, dense references (numpy), oracle wiring."""
import ctypes

import numpy as np

from oracle import oracle as orc
from smcp_amd import problems
from smcp_amd.symbolic import Symbolic


def edges_of(pat):
    n, cp, ri = pat
    cols = np.repeat(np.arange(n), np.diff(cp))
    return list(zip(ri.tolist(), cols.tolist()))


PATTERNS = {
    "band": lambda: problems.band_pattern(30, 3),
    "arrow": lambda: problems.block_arrow_pattern(6, 4, 5),
    "nested": lambda: problems.nested_block_arrow_pattern(nsub=2, nmid=3, nleaf_per_mid=2, leaf=(2, 4),
                                                          mid=(3, 5), top=(4, 6), root=8, seed=1),
    "rand1": lambda: problems.random_chordal_pattern(12, seed=1),
    "rand2": lambda: problems.random_chordal_pattern(25, max_nn=4, max_na=6, seed=2),
    "dense": lambda: problems.block_arrow_pattern(1, 7, 0) if False else problems.band_pattern(9, 8),
}


# the patterns of the GPU suite: the six small ones plus the shapes that select the device's other kernel classes
GPU_PATTERNS = dict(PATTERNS)
GPU_PATTERNS["arrow_big"] = lambda: problems.block_arrow_pattern(12, 64, 128)
GPU_PATTERNS["nested_mid"] = lambda: problems.nested_block_arrow_pattern(nsub=2, nmid=6, nleaf_per_mid=8, seed=3)
GPU_PATTERNS["dense200"] = lambda: problems.band_pattern(200, 199)
GPU_PATTERNS["arrow_thin"] = lambda: problems.block_arrow_pattern(6, 2, 150)   # thin cliques, separators beyond LDS
GPU_PATTERNS["diag"] = lambda: problems.band_pattern(15, 0)          # LP case: every clique is 1 x 1
# single fronts beyond the one-workgroup class (272 rows): the one-launch blocked Cholesky (front_flow.hip) factors the root
# (dense600; arrow_one's 310 x 310 root) and the 300 x 300 Y_AA block of arrow_one's only top front
GPU_PATTERNS["dense600"] = lambda: problems.band_pattern(600, 599)
GPU_PATTERNS["arrow_one"] = lambda: problems.nested_block_arrow_pattern(nsub=1, nmid=2, nleaf_per_mid=2, leaf=(3, 9), mid=(6, 20), top=(40, 300),
                                                                        root=310, seed=9)
# three top fronts in ONE level whose separators (300, 200 and 150 rows of a 310-column root) are beyond the one-workgroup class:
# their chol(Y_AA) runs side by side in one launch of the one-launch blocked Cholesky (front_flow.hip, gridDim.y = 3; orders 5 / 4 / 3
# tiles against a plan laid out for 5)
def _three_tops_pattern():
    root = np.arange(130, 440)
    cl = [(root, root)]
    for s_, na in enumerate((300, 200, 150)):
        own = np.arange(40 * s_, 40 * s_ + 40)
        sep = root[np.sort(np.random.default_rng(90 + s_).choice(len(root), size=na, replace=False))]
        cl.append((own, np.concatenate([own, sep])))
    cl.append((np.arange(120, 130), np.concatenate([np.arange(120, 130), root[:20]])))
    return problems._from_cliques(440, cl)


GPU_PATTERNS["three_tops"] = _three_tops_pattern
# families (front_fam.hip: small parents swept together with their childless children): largest member sizes,
# odd sizes with few children, and nine children per parent (one more than the waves of a workgroup: no family)
GPU_PATTERNS["fam_max"] = lambda: problems.nested_block_arrow_pattern(nsub=1, nmid=3, nleaf_per_mid=8, leaf=(16, 32),
                                                                      mid=(16, 64), top=(40, 50), root=60, seed=5)
GPU_PATTERNS["fam_odd"] = lambda: problems.nested_block_arrow_pattern(nsub=2, nmid=4, nleaf_per_mid=5, leaf=(3, 17),
                                                                      mid=(7, 33), top=(20, 30), root=40, seed=6)
GPU_PATTERNS["fam_nine"] = lambda: problems.nested_block_arrow_pattern(nsub=1, nmid=2, nleaf_per_mid=9, leaf=(2, 9),
                                                                       mid=(6, 20), top=(20, 20), root=30, seed=7)


# odd-sized families under top fronts beyond the LDS class (nf = 130 <= 198): the fused extend-add with three row tiles
GPU_PATTERNS["fam_top"] = lambda: problems.nested_block_arrow_pattern(nsub=2, nmid=5, nleaf_per_mid=3, leaf=(3, 17),
                                                                      mid=(7, 33), top=(30, 100), root=110, seed=8)


def make(name):
    pat = PATTERNS[name]()
    symb = Symbolic(pat)
    S = orc.Sym(symb)
    return pat, symb, S


def random_spd_on_V(S, seed=0):
    """Dense SPD matrix (permuted coordinates) whose sparsity pattern is exactly V:
    built as L L^T with L lower with pattern V (zero fill because V is chordal + PEO)."""
    rng = np.random.default_rng(seed)
    mask = np.tril(S.mask())
    L = np.where(mask, rng.standard_normal((S.n, S.n)) * 0.4, 0.0)
    L[np.diag_indices(S.n)] = 1.0 + rng.random(S.n)
    return L @ L.T, L


def proj(S, M):
    return np.where(S.mask(), M, 0.0)


# ---- shared by the tests of the dense-block products and the completions ---------------------------------------------
def two_components():
    """a band and a block arrow that share nothing"""
    band = [(np.array([j]), np.arange(j, min(20, j + 4))) for j in range(20)]
    arrow = [(np.arange(20 + 5 * b, 25 + 5 * b), np.concatenate([np.arange(20 + 5 * b, 25 + 5 * b), np.arange(35, 41)])) for b in range(3)]
    arrow.append((np.arange(35, 41), np.arange(35, 41)))
    return problems._from_cliques(41, band + arrow)


EXTRA = {"two_components": two_components, "one_clique": lambda: problems.band_pattern(33, 32),
         "wide_arrow": lambda: problems.block_arrow_pattern(150, 2, 6)}

SYMB = {}


def symb_of(name):
    """the Symbolic of a pattern of GPU_PATTERNS (host only), built once"""
    if name not in SYMB:
        SYMB[name] = Symbolic(GPU_PATTERNS[name]())
    return SYMB[name]


def padded(M, pad, fill=7.25):
    """the (k, n) device view of an n x k numpy block inside a tensor with `pad` padding columns, and that tensor"""
    import torch
    n, k = M.shape
    full = torch.full((k, n + pad), fill, dtype=torch.float64, device="cuda")
    view = full[:, :n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(M.T)))
    return view, full


def random_block(n, k, pad, seed):
    """(n x k numpy block, its (k, n) device view, the padded tensor behind the view)"""
    B = np.random.default_rng(seed).standard_normal((n, k))
    view, full = padded(B, pad)
    return B, view, full


def census_read(handle):
    """{pretty kernel name: launches} since the last read of a context's launch census (csp_census_read), which it clears"""
    from smcp_amd import _lib
    lib = _lib.lib()
    need = int(lib.csp_census_read(handle, None, 0))
    while True:
        assert need > 0, need
        buf = ctypes.create_string_buffer(need)
        got = int(lib.csp_census_read(handle, buf, need))
        if got <= need:
            break
        need = got
    out = {}
    for line in buf.value.decode().splitlines():
        _, pretty, count = line.split("\t")
        out[pretty] = out.get(pretty, 0) + int(count)
    return out


def kernel_census(symb, fn):
    """kernel FUNCTION name (k_ceigw_solve<true>: one per template instantiation) -> launches while fn() runs; launch_counts
    gives the same launches under the kernel ids, which stand for groups of kernels"""
    import torch
    from smcp_amd import _lib
    lib = _lib.lib()
    lib.csp_census_enable(symb.handle, 1)
    census_read(symb.handle)
    try:
        fn()
        torch.cuda.synchronize()
        return census_read(symb.handle)
    finally:
        lib.csp_census_enable(symb.handle, 0)


def launch_census(symb, fn):
    """(launch_counts, kernel_census) of ONE run of fn(): the launches under the kernel ids and under the kernel functions"""
    box = {}
    census = kernel_census(symb, lambda: box.update(counts=launch_counts(symb, fn)))
    return box["counts"], census


def pretty_kernel_name(mangled):
    """k_hess_down_fam<3, 2> of _ZN4smcp15k_hess_down_famILi3ELi2EEEv...: the demangled name without return type, namespace and
    parameter list (what csp_census_read writes)"""
    import ctypes.util
    cxx = ctypes.CDLL(ctypes.util.find_library("stdc++") or "libstdc++.so.6")
    libc = ctypes.CDLL(None)
    cxx.__cxa_demangle.restype = ctypes.c_void_p
    cxx.__cxa_demangle.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    libc.free.argtypes = [ctypes.c_void_p]
    status = ctypes.c_int(1)
    p = cxx.__cxa_demangle(mangled.encode(), None, None, ctypes.byref(status))
    s = ctypes.string_at(p).decode() if status.value == 0 and p else mangled
    if p:
        libc.free(p)
    s = s.replace("(anonymous namespace)::", "")
    depth, end = 0, len(s)
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            end = i
            break
    s, depth, begin = s[:end], 0, 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif depth == 0 and ch == " ":
            begin = i + 1
        elif depth == 0 and s[i:i + 2] == "::":
            begin = i + 2
    return s[begin:]


def kernel_universe(path=None):
    """{mangled: pretty} of every kernel instantiation the library holds: the kernel descriptors (symbols ending in .kd) of the
    gfx950 code object inside libsmcp_amd.so, read from the file's bytes (its string tables are not compressed)"""
    import re
    from smcp_amd import _lib
    with open(path or _lib.LIB_PATH, "rb") as f:
        data = f.read()
    names = sorted({m.group(1).decode() for m in re.finditer(rb"\x00([A-Za-z_][A-Za-z0-9_$.]*)\.kd(?=\x00)", data)})
    return {m: pretty_kernel_name(m) for m in names}


def kernel_function(pretty):
    """k_hess_down_fam of k_hess_down_fam<3, 2>"""
    return pretty.split("<")[0]


def launch_counts(symb, fn):
    """kernel name -> launches while fn() runs (csp_profile_*: every launch of the library is counted)"""
    import torch
    from smcp_amd import _lib
    lib = _lib.lib()
    h = symb.handle
    nk = int(lib.csp_profile_kinds())
    names = [lib.csp_profile_kernel_name(i).decode() for i in range(nk)]
    lib.csp_profile_filter(h, -1)
    lib.csp_profile_enable(h, 1)
    lib.csp_profile_read(h, None, None)
    try:
        fn()
        torch.cuda.synchronize()
        ms = (ctypes.c_double * nk)()
        cnt = (ctypes.c_int64 * nk)()
        lib.csp_profile_read(h, ms, cnt)
    finally:
        lib.csp_profile_enable(h, 0)
    return {names[i]: int(cnt[i]) for i in range(nk) if cnt[i]}
