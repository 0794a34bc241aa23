"""The rule of `lash dist --tree` in plain numpy, the Newick renderer, the cut, and ctypes access to lash_tree_* and to the
host functions the command line renders with.  A helper for test_newick.py, test_gpu_tree.py and test_gpu_dist_tree.py, not a test.

The model defines the result: per step an arg-min of (d, i, j) over the active upper triangle, the merge recorded with scipy node ids,
the new node living on in slot i, and one of three updates written with separately rounded float64 operations."""
import ctypes as C
import re

import numpy as np

AVERAGE, SINGLE, COMPLETE = 0, 1, 2
LINKAGES = {"average": AVERAGE, "single": SINGLE, "complete": COMPLETE}


# ---- the model -----------------------------------------------------------------------------------------------------------------------

def merges(dist, linkage):
    """dist: symmetric float64 [n][n] without NaN (the diagonal is never read).  -> list of (a, b, height, size), n - 1 of them."""
    D = np.array(dist, np.float64)
    n = D.shape[0]
    if n < 2:
        return []
    assert not np.isnan(D).any()
    # M: D on the active upper triangle, +inf elsewhere.  np.argmin takes the first minimum in row-major order: the smallest (i, j)
    M = np.where(np.triu(np.ones((n, n), bool), 1), D, np.inf)
    active = np.ones(n, bool)
    size = np.ones(n, np.int64)
    node = np.arange(n)
    out = []
    for s in range(n - 1):
        i, j = divmod(int(np.argmin(M)), n)
        assert i < j and active[i] and active[j]
        out.append((int(node[i]), int(node[j]), float(D[i, j]), int(size[i] + size[j])))
        if linkage == AVERAGE:
            wi, wj = np.float64(size[i]), np.float64(size[j])
            new = (wi * D[i] + wj * D[j]) / (wi + wj)          # two products, one sum, one quotient: numpy rounds each
        elif linkage == SINGLE:
            new = np.minimum(D[i], D[j])
        else:
            new = np.maximum(D[i], D[j])
        active[j] = False
        others = active.copy()
        others[i] = False
        D[i, others] = new[others]
        D[others, i] = new[others]
        size[i] += size[j]
        node[i] = n + s
        M[j, :] = np.inf
        M[:, j] = np.inf
        hi = others & (np.arange(n) > i)
        lo = others & (np.arange(n) < i)
        M[i, hi] = new[hi]
        M[lo, i] = new[lo]
    return out


def label(name):
    return "'" + name.replace("'", "''") + "'" if re.search(r"[()\[\]':;, \t\n\v\f\r]", name) else name


def newick(names, mg):
    """the text of --tree without its trailing newline"""
    n = len(names)
    if n == 0:
        return ";"
    height = [0.0] * n + [m[2] for m in mg]
    text = [label(x) for x in names] + [None] * len(mg)
    for s, (a, b, h, _) in enumerate(mg):
        text[n + s] = "(%s:%s,%s:%s)" % (text[a], "%.10g" % (h / 2 - height[a] / 2), text[b], "%.10g" % (h / 2 - height[b] / 2))
        text[a] = text[b] = None                               # (each node is a child once; keeps a chain linear in memory)
    return text[-1] + ";"


def cut(n, mg, max_height):
    """label[i] = the smallest leaf of i's component after exactly the merges with height <= max_height"""
    parent = list(range(n))
    leaf = list(range(n)) + [0] * len(mg)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for s, (a, b, h, _) in enumerate(mg):
        leaf[n + s] = leaf[a]
        if h <= max_height:
            ra, rb = find(leaf[a]), find(leaf[b])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return [find(i) for i in range(n)]


def render_clusters(names, lab):
    """the --cluster text: the header, then every name under its cluster's first name, in row order"""
    order = sorted(range(len(names)), key=lambda i: (lab[i], i))
    return "Representative\tMember\n" + "".join("%s\t%s\n" % (names[lab[i]], names[i]) for i in order)


# ---- the library's side ---------------------------------------------------------------------------------------------------------------

def _merge_array(mg):
    from lash_amd import _lib
    arr = (_lib.TreeMerge * max(len(mg), 1))()
    for s, (a, b, h, size) in enumerate(mg):
        arr[s].a, arr[s].b, arr[s].height, arr[s].size = a, b, h, size
    return arr


def _host():
    import host_lib as H
    lib = H.lib
    lib.lash_host_newick.restype = C.c_void_p
    lib.lash_host_newick.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_void_p]
    lib.lash_host_tree_cut.restype = C.c_int
    lib.lash_host_tree_cut.argtypes = [C.c_uint32, C.c_void_p, C.c_double, C.c_void_p]
    return lib


def host_newick(names, mg):
    """host/newick.cpp's renderer, the one the command line writes with; None when it refuses the merge list"""
    lib = _host()
    arr = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    marr = _merge_array(mg)
    p = lib.lash_host_newick(arr, len(names), C.addressof(marr))
    if not p:
        return None
    text = C.string_at(p).decode()
    lib.lash_host_free(p)
    return text


def host_cut(n, mg, max_height):
    lib = _host()
    out = np.zeros(max(n, 1), np.uint32)
    marr = _merge_array(mg)
    if lib.lash_host_tree_cut(n, C.addressof(marr), max_height, out.ctypes.data) != 0:
        return None
    return out[:n].tolist()


class TreeError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("lash error %d: %s" % (code, text))
        self.code, self.text = code, text


class Tree:
    """lash_tree on a lash_amd.Context"""

    def __init__(self, ctx, n):
        self._ctx, self._lib, self.n = ctx, ctx._lib, int(n)
        h = C.c_void_p()
        self._check(self._lib.lash_tree_create(ctx._h, self.n, C.byref(h)))
        self._h = h

    def _check(self, rc):
        if rc != 0:
            raise TreeError(rc, self._lib.lash_ctx_last_error(self._ctx._h).decode())

    def set_rows(self, r0, r1, dist):
        """rows [r0, r1) of a full matrix: the [r1 - r0][r1] block the entry reads (it looks at columns <= row only)"""
        block = np.ascontiguousarray(np.asarray(dist, np.float64)[r0:r1, :r1])
        self._check(self._lib.lash_tree_set_rows(self._ctx._h, self._h, int(r0), int(r1), block.ctypes.data if block.size else None))

    def get_rows(self, r0, r1):
        out = np.empty((r1 - r0, self.n), np.float64)
        self._check(self._lib.lash_tree_get_rows(self._ctx._h, self._h, int(r0), int(r1), out.ctypes.data if out.size else None))
        return out

    def build(self, linkage):
        """-> (list of (a, b, height, size), stats dict)"""
        from lash_amd import _lib
        arr = (_lib.TreeMerge * max(self.n - 1, 1))()
        st = _lib.TreeStats()
        self._check(self._lib.lash_tree_build(self._ctx._h, self._h, int(linkage), C.addressof(arr), C.byref(st)))
        mg = [(arr[s].a, arr[s].b, arr[s].height, arr[s].size) for s in range(max(self.n - 1, 0))]
        return mg, dict(steps=st.steps, rescanned_rows=st.rescanned_rows, bytes=st.bytes)

    def free(self):
        if getattr(self, "_h", None):
            self._lib.lash_tree_free(self._ctx._h, self._h)
        self._h = None


def bits(mg):
    """merges with the height as its 64 bits: equality is bit for bit"""
    return [(a, b, np.float64(h).view(np.uint64).item(), size) for a, b, h, size in mg]
