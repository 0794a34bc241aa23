"""The model of `lash growth`: the orderings (splitmix64 + Fisher–Yates, restated from the rule the command documents) and the table, its
numbers taken the slow way — the images folded one at a time with merge_images, every prefix's cardinality from the host entry for a
single image (lash_amd.sketch.sketch_cardinality: lash_hmh_cardinality / lash_hll_cardinality / lash_ull_estimate)."""
import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


class SplitMix64:
    def __init__(self, state):
        self.state = state & M64

    def next(self):
        self.state = (self.state + GAMMA) & M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)


def order(n, o, seed):
    """order o of n rows: 0 = as they are, else the shuffle seeded with seed ^ (o * GAMMA)"""
    a = list(range(n))
    if o == 0:
        return a
    rng = SplitMix64(seed ^ ((o * GAMMA) & M64))
    for j in range(n - 1, 0, -1):
        r = (rng.next() * (j + 1)) >> 64
        a[j], a[r] = a[r], a[j]
    return a


def orders(n, n_orders, seed):
    return np.array([order(n, o, seed) for o in range(n_orders)], dtype=np.uint32).reshape(n_orders, n)


def fold(ctx, algo, p, images, idx):
    """the images of the prefixes of idx: [len(idx), image_bytes], each the merge_images fold of the ones before it with the next"""
    acc = images[idx[0]].copy().reshape(1, -1)
    out = [acc[0].copy()]
    for i in idx[1:]:
        ctx.merge_images(algo, p, acc, np.ascontiguousarray(images[i]).reshape(1, -1))
        out.append(acc[0].copy())
    return np.array(out)


def prefix_cardinalities(ctx, algo, p, images, order_rows, estimator="fgra", hll_bias=None):
    """float64 [n_orders, len]: sketch_cardinality of every folded prefix (raises LashError(ERANGE) where the host entry does)"""
    from lash_amd.sketch import sketch_cardinality
    out = np.zeros((len(order_rows), len(order_rows[0])), dtype=np.float64)
    for o, idx in enumerate(order_rows):
        for t, img in enumerate(fold(ctx, algo, p, images, [int(i) for i in idx])):
            out[o, t] = sketch_cardinality(algo, p, img, estimator=estimator, hll_bias=hll_bias)
    return out


def table(names, order_rows, card):
    """the text `lash growth` writes for these rows: names in row order, order_rows / card [n_orders, n]"""
    lines = ["Order\tStep\tName\tUnion\tNew\n"]
    for o, idx in enumerate(order_rows):
        for t, i in enumerate(idx):
            u = float(card[o][t])
            new = u - float(card[o][t - 1]) if t else u
            lines.append("%d\t%d\t%s\t%.3f\t%.3f\n" % (o, t + 1, names[int(i)], u, new))
    return "".join(lines)
