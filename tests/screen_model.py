"""The numpy model of `lash screen` (include/lash_gfx950.h: lash_sketch_set_screen_wta; csrc/host/screen.cpp).

The registers come from spectrum_model.registers.  Reference i holds bucket b of a query iff the query's register there is not 0 and the
reference's equals it; a query's candidate list is ordered, position is priority, and a bucket goes to the first position that holds it.
Everything is equality, minimum and counting over integers, and the text of the command's table follows from numbers the ABI gives, so
both can be compared with ==."""
import numpy as np

from spectrum_model import M

NONE = 0xFFFFFFFF
HEADER = "Query\tReference\tShared\tWon\tBuckets\tDistance\tWtaDistance\n"


def holds(ref_regs, q, rows):
    """bool [len(rows), 16384]: position t of the list holds bucket b"""
    rows = np.asarray([int(r) for r in rows], dtype=np.intp)
    q = np.asarray(q)
    return (np.asarray(ref_regs)[rows].reshape(len(rows), M) == q[None, :]) & (q[None, :] != 0)


def winners(ref_regs, q, rows):
    """uint32 [16384]: the smallest position that holds the bucket, NONE where no candidate does"""
    h = holds(ref_regs, q, rows)
    if h.shape[0] == 0:
        return np.full(M, NONE, dtype=np.uint32)
    return np.where(h.any(axis=0), h.argmax(axis=0), NONE).astype(np.uint32)


def wta(ref_regs, q, rows):
    """(shared, won) of one query's list: uint32 [len(rows)] each"""
    h = holds(ref_regs, q, rows)
    w = winners(ref_regs, q, rows)
    shared = h.sum(axis=1).astype(np.uint32)
    won = np.array([int((w == t).sum()) for t in range(len(rows))], dtype=np.uint32)
    return shared, won


def screen(ref_regs, qry_regs, candidates):
    """what SketchSet.screen_wta returns: (shared, won), one uint32 array per query"""
    both = [wta(ref_regs, qry_regs[j], rows) for j, rows in enumerate(candidates)]
    return [s for s, _ in both], [w for _, w in both]


def priority(rows, d, card):
    """the rows of one query's candidates, best first: d ascending, then the reference's cardinality descending, then the row"""
    return [r for _, _, r in sorted((float(d[r]), -float(card[r]), int(r)) for r in rows)]


def fmt(d):
    """a distance as `lash dist` prints it"""
    return "NaN" if d != d else "%.6f" % d


def table(qnames, rnames, lists, shared, won, buckets, dist, wta_dist, max_dist, keep_losers=False):
    """the file `lash screen` writes.  lists[j]: query j's candidate rows, best first; shared[j][t] / won[j][t]: the counts of position t;
    buckets[r][j], dist[r][j]: the pair's N and its containment distance; wta_dist[j][t]: the distance recomputed with won for C"""
    out = [HEADER]
    for j, rows in enumerate(lists):
        for t, r in enumerate(rows):
            if keep_losers or wta_dist[j][t] <= max_dist:
                out.append("%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (qnames[j], rnames[r], int(shared[j][t]), int(won[j][t]), int(buckets[r][j]),
                                                             fmt(float(dist[r][j])), fmt(float(wta_dist[j][t]))))
    return "".join(out)
