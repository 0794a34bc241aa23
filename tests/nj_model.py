"""The rule of `lash dist --tree --nj` in plain numpy, its Newick renderer, a split-set extractor, a generator of
additive trees, and ctypes access to lash_tree_build_nj and to the host renderer the command line writes with.  A helper for
test_nj_model.py, test_gpu_nj.py and test_gpu_dist_nj.py, not a test.

The model defines the result: row sums added up in column order and then carried, per step an arg-min of (Q, i, j) over the active
upper triangle with Q = ((w * D[i][j]) - R[i]) - R[j], the join recorded with scipy node ids, the new node living on in slot i, and
every update written with separately rounded float64 operations."""
import ctypes as C

import numpy as np

import tree_model as T


# ---- the model -----------------------------------------------------------------------------------------------------------------------

def joins_state(dist):
    """dist: symmetric finite float64 [n][n] (the diagonal is never read).  -> (records, R, D, slots): n - 1 records (a, b, len_a,
    len_b), the closing record last, and the state at the end: the carried row sums, the matrix and the two slots that are left."""
    D = np.array(dist, np.float64)
    n = D.shape[0]
    if n < 2:
        return [], np.zeros(n), D, np.arange(n)
    assert np.isfinite(D[~np.eye(n, dtype=bool)]).all()
    R = np.zeros(n)
    for c in range(n):                                         # columns ascending, one rounding per add, c = i skipped
        rows = np.arange(n) != c
        R[rows] = R[rows] + D[rows, c]
    slots = np.arange(n)                                       # the active slots, ascending: the labels that break ties
    node = np.arange(n)
    out = []
    for s in range(n - 2):
        r = len(slots)
        w = np.float64(r - 2)
        Q = (w * D[np.ix_(slots, slots)] - R[slots][:, None]) - R[slots][None, :]     # numpy rounds each of the three
        Q[np.tril_indices(r)] = np.inf
        a, b = divmod(int(np.argmin(Q)), r)                    # the first minimum in row-major order: the smallest (i, j)
        i, j = int(slots[a]), int(slots[b])
        dij = D[i, j]
        len_i = dij * 0.5 + (R[i] - R[j]) / (2.0 * w)
        len_j = dij - len_i
        out.append((int(node[i]), int(node[j]), float(len_i), float(len_j)))
        others = slots[(slots != i) & (slots != j)]
        v = ((D[i, others] + D[j, others]) - dij) * 0.5
        R[others] = ((R[others] - D[i, others]) - D[j, others]) + v
        D[i, others] = v
        D[others, i] = v
        R[i] = ((R[i] + R[j]) - np.float64(r) * dij) * 0.5
        node[i] = n + s
        slots = slots[slots != j]
    i, j = int(slots[0]), int(slots[1])
    out.append((int(node[i]), int(node[j]), float(D[i, j]), 0.0))
    return out, R, D, slots


def joins(dist):
    return joins_state(dist)[0]


def newick(names, jn):
    """the text of --tree --nj without its trailing newline"""
    n = len(names)
    if n == 0:
        return ";"
    if n == 1:
        return T.label(names[0]) + ";"
    x, y, L, _ = jn[-1]
    if n == 2:
        return "(%s:%s,%s:%s);" % (T.label(names[x]), "%.10g" % (L * 0.5), T.label(names[y]), "%.10g" % (L * 0.5))
    text = [T.label(nm) for nm in names] + [None] * (n - 2)
    for s, (a, b, la, lb) in enumerate(jn[:-1]):
        inner = "%s:%s,%s:%s" % (text[a], "%.10g" % la, text[b], "%.10g" % lb)
        text[a] = text[b] = None
        text[n + s] = inner if n + s == 2 * n - 3 else "(" + inner + ")"          # the root stays open for its third child
    other = y if x == 2 * n - 3 else x
    return "(%s,%s:%s);" % (text[2 * n - 3], text[other], "%.10g" % L)


def _side(leaves, n):
    """one name for the two sides of a split: the side without leaf 0"""
    return frozenset(range(n)) - leaves if 0 in leaves else leaves


def splits(n, jn):
    """the unrooted tree as {side of the split: branch length}, one entry per branch (2n - 3 of them for n >= 3)"""
    below = {i: frozenset([i]) for i in range(n)}
    out = {}
    for s, (a, b, la, lb) in enumerate(jn[:-1]):
        below[n + s] = below[a] | below[b]
        out[_side(below[a], n)] = la
        out[_side(below[b], n)] = lb
    if jn:
        x, y, L, _ = jn[-1]
        assert below[x] | below[y] == frozenset(range(n)) and _side(below[x], n) == _side(below[y], n)
        out[_side(below[y], n)] = L                            # one branch between the last two nodes
    return out


def additive(n, seed):
    """a random tree over n >= 2 leaves, made by joining two random groups at a time, every branch k/64 with 1 <= k <= 64; -> (its
    path-length matrix, exact in float64, and its splits as `splits` names them).  Every inner node has degree 3."""
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    groups = [(np.array([i]), np.zeros(1)) for i in range(n)]  # (leaves, their distance to the group's top node)
    truth = {}
    while len(groups) > 2:
        a, b = sorted(rng.choice(len(groups), 2, replace=False).tolist())
        (la, da), (lb, db) = groups[a], groups[b]
        ea, eb = rng.integers(1, 65) / 64.0, rng.integers(1, 65) / 64.0
        truth[_side(frozenset(la.tolist()), n)] = ea
        truth[_side(frozenset(lb.tolist()), n)] = eb
        between = (da + ea)[:, None] + (db + eb)[None, :]
        D[np.ix_(la, lb)] = between
        D[np.ix_(lb, la)] = between.T
        groups = [g for t, g in enumerate(groups) if t not in (a, b)] + [(np.concatenate([la, lb]), np.concatenate([da + ea, db + eb]))]
    (la, da), (lb, db) = groups
    e = rng.integers(1, 65) / 64.0
    truth[_side(frozenset(lb.tolist()), n)] = e
    between = (da + e)[:, None] + db[None, :]
    D[np.ix_(la, lb)] = between
    D[np.ix_(lb, la)] = between.T
    return D, truth


# ---- the library's side ---------------------------------------------------------------------------------------------------------------

def _join_array(jn):
    from lash_amd import _lib
    arr = (_lib.NjJoin * max(len(jn), 1))()
    for s, (a, b, la, lb) in enumerate(jn):
        arr[s].a, arr[s].b, arr[s].len_a, arr[s].len_b = a, b, la, lb
    return arr


def host_newick(names, jn):
    """host/newick.cpp's NJ renderer, the one the command line writes with; None when it refuses the join list"""
    import host_lib as H
    lib = H.lib
    lib.lash_host_newick_nj.restype = C.c_void_p
    lib.lash_host_newick_nj.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_void_p]
    arr = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    jarr = _join_array(jn)
    p = lib.lash_host_newick_nj(arr, len(names), C.addressof(jarr))
    if not p:
        return None
    text = C.string_at(p).decode()
    lib.lash_host_free(p)
    return text


def njbuild(tree):
    """lash_tree_build_nj on a tree_model.Tree -> (list of (a, b, len_a, len_b), stats dict)"""
    from lash_amd import _lib
    arr = (_lib.NjJoin * max(tree.n - 1, 1))()
    st = _lib.TreeStats()
    tree._check(tree._lib.lash_tree_build_nj(tree._ctx._h, tree._h, C.addressof(arr), C.byref(st)))
    jn = [(arr[s].a, arr[s].b, arr[s].len_a, arr[s].len_b) for s in range(max(tree.n - 1, 0))]
    return jn, dict(steps=st.steps, rescanned_rows=st.rescanned_rows, bytes=st.bytes)


def bits(jn):
    """records with both lengths as their 64 bits: equality is bit for bit"""
    return [(a, b, np.float64(la).view(np.uint64).item(), np.float64(lb).view(np.uint64).item()) for a, b, la, lb in jn]
