"""The numpy model of lash_tree_build_pcoa (csrc/dist_pcoa.hip): Gower centring, np.linalg.eigh, the K algebraically largest eigenpairs,
the sign rule and the coordinates; the inputs the tests share; and the binding of the entry on a tree_model.Tree."""
import ctypes as C

import numpy as np

SCALES = (8.0, 5.0, 3.0, 2.0, 1.2, 0.7, 0.4, 0.2)


def centre(dist):
    """B of the rule: A = -1/2 D o D, B = A - r_i - r_j + g"""
    a = -0.5 * np.asarray(dist, np.float64) ** 2
    r = a.mean(axis=1)
    return a - r[:, None] - r[None, :] + r.mean()


def spectrum(dist):
    """every eigenvalue of B, descending"""
    return np.linalg.eigvalsh(centre(dist))[::-1]


def sign_rule(v):
    """the column with its component of largest size positive (ties: the lowest row)"""
    i = int(np.argmax(np.abs(v)))
    return -v if v[i] < 0 else v


def pcoa(dist, k):
    """-> (eigenvalues [k], coords [n][k], trace): the k' = min(k, n - 1) algebraically largest eigenpairs of B, zeros beyond"""
    b = centre(dist)
    n = b.shape[0]
    w, v = np.linalg.eigh(b)
    w, v = w[::-1], v[:, ::-1]
    kk = min(k, n - 1)
    eig = np.zeros(k)
    coords = np.zeros((n, k))
    eig[:kk] = w[:kk]
    for a in range(kk):
        if w[a] > 0:
            coords[:, a] = sign_rule(v[:, a]) * np.sqrt(w[a])
    return eig, coords, float(np.trace(b))


def _distances(x):
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    d = 0.5 * (d + d.T)
    d[np.diag_indices(len(x))] = 0.0
    return d


def euclidean(n, seed):
    """Euclidean distances of n Gaussian points in R^8 with the axis scales SCALES"""
    rng = np.random.default_rng(seed)
    return _distances(rng.standard_normal((n, len(SCALES))) * np.array(SCALES))


def non_euclidean(n, seed):
    """euclidean(n, seed) with the three pairs among three rows replaced by distances far beyond the triangle inequality.  Stretching
    the pairs of a triangle {a, b, c} to lengths far above every other distance adds to B about -c_ab (e_a e_b^T + e_b e_a^T) - ... with
    c = d^2 / 2: one eigenvalue near -(c_ab + c_ac + c_bc) * 2 / 3 and two positive ones of about half that size, so the negative
    eigenvalue is the largest of all in size.  n = 3 is the triangle alone: lengths 1, 1 and 5."""
    if n == 3:
        return np.array([[0.0, 1.0, 5.0], [1.0, 0.0, 1.0], [5.0, 1.0, 0.0]])
    d = euclidean(n, seed)
    lam1 = spectrum(d)[0]
    rng = np.random.default_rng(seed + 1)
    a, b, c = sorted(rng.choice(n, 3, replace=False).tolist())
    for (i, j), f in (((a, b), 1.0), ((a, c), 1.6), ((b, c), 2.4)):
        d[i, j] = d[j, i] = np.sqrt(2.0 * f * lam1)
    return d


def line(n, seed):
    """all points on a line: B has one non-zero eigenvalue, every K > 1 is above the rank"""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.standard_normal(n)) * 3.0
    d = np.abs(x[:, None] - x[None, :])
    return d


def diagonal_negative(n, seed):
    """Gaussian points in R^3 (scales 8, 7, 2.5: lambda_3 is about a tenth of lambda_1) with nine diagonal cells set to sqrt(2 x lambda_1),
    x = 0.50 .. 0.58.  The entry reads the diagonal like any other cell, and -1/2 J diag(s) J has an eigenvalue near -s_i / 2 per set
    cell: nine negative eigenvalues five times lambda_3 in size, one more than the m - k' = 8 spare vectors of K = 3, and next to nothing
    else.  An iteration that ranks by size holds lambda_1, lambda_2 and the nine, and converges with lambda_3 left out."""
    rng = np.random.default_rng(seed)
    d = _distances(rng.standard_normal((n, 3)) * np.array([8.0, 7.0, 2.5]))
    lam1 = spectrum(d)[0]
    for t, i in enumerate(rng.choice(n, 9, replace=False)):
        d[i, i] = np.sqrt(2.0 * (0.50 + 0.01 * t) * lam1)
    return d


KINDS = {"euclidean": euclidean, "non_euclidean": non_euclidean, "line": line, "diagonal_negative": diagonal_negative}
SIZES = (2, 3, 15, 16, 17, 65, 257, 1000)
# per kind and n, a seed at which the leading axes stand at least 0.06 lambda_1 from every other eigenvalue and, for non_euclidean, the
# negative eigenvalue is larger in size than lambda_1 (searched on the CPU; test_pcoa_model.py and test_gpu_pcoa.py assert both)
SEEDS = {"euclidean": {2: 1, 3: 1, 15: 2, 16: 2, 17: 2, 65: 1, 257: 1, 1000: 1},
         "non_euclidean": {3: 0, 15: 8, 16: 7, 17: 1, 65: 1, 257: 2, 1000: 24},
         "line": {n: 5 for n in SIZES},
         "diagonal_negative": {65: 1, 257: 1}}


class PcoaError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("lash error %d: %s" % (code, text))
        self.code, self.text = code, text


def pcoabuild(tree, k, tol=0.0, max_iter=0, out=None):
    """lash_tree_build_pcoa on a tree_model.Tree -> (eigenvalues [k], coords [n][k], stats dict).  `out` = (eigenvalues, coords) arrays to
    write into instead of fresh ones (how a test sees that a failed call leaves them alone)."""
    from lash_amd import _lib
    k_arr = max(int(k), 1) if 0 < int(k) <= 64 else 1
    eig, coords = out if out is not None else (np.full(k_arr, np.nan), np.full((max(tree.n, 1), k_arr), np.nan))
    st = _lib.PcoaStats()
    rc = tree._lib.lash_tree_build_pcoa(tree._ctx._h, tree._h, int(k), float(tol), int(max_iter), eig.ctypes.data, coords.ctypes.data, C.byref(st))
    if rc != 0:
        raise PcoaError(rc, tree._lib.lash_ctx_last_error(tree._ctx._h).decode())
    return eig, coords[:tree.n], dict(iterations=st.iterations, products=st.products, bytes=st.bytes, worst_residual=st.worst_residual,
                                      shift=st.shift, trace=st.trace)
