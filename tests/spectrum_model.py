"""The numpy model of `lash spectrum` (include/lash_gfx950.h: lash_sketch_set_group_spectrum; csrc/host/spectrum.cpp).

The registers of a HyperMinHash image are its bytes behind the layout's header, viewed as 16 384 u16 (big-endian under a layout that
says so).  A group's bins are max, equality and bincount over them; the derived numbers follow in the operation order the command line
documents, so the text of its tables can be compared with ==."""
import numpy as np

M = 16384


def registers(images, hdr=0, big_endian=False):
    """uint8 [n, image_bytes] -> the registers as integers [n, 16384]"""
    img = np.ascontiguousarray(images, dtype=np.uint8)
    if img.ndim == 1:
        img = img[None, :]
    regs = np.ascontiguousarray(img[:, hdr:hdr + 2 * M])
    assert regs.shape[1] == 2 * M
    return regs.view(">u2" if big_endian else "<u2").astype(np.uint32)


def hist(regs, members):
    """the n + 1 bins of one group (members: indices into regs, repeats count): uint32"""
    members = [int(m) for m in members]
    n = len(members)
    if n == 0:
        return np.array([M], dtype=np.uint32)
    sub = regs[members]
    top = sub.max(axis=0)
    holders = ((sub == top[None, :]) & (top[None, :] != 0)).sum(axis=0)
    return np.bincount(holders, minlength=n + 1).astype(np.uint32)


def occupied(h):
    return M - int(h[0])


def kmers(h, c, U):
    """K(c) = (double)hist[c] / (double)occupied * U"""
    return float(int(h[c])) / float(occupied(h)) * float(U)


def classes(h, U, core=0.95, cloud=0.15):
    """(Core, Shell, Cloud): the sums of K(c) in ascending c; count c of n members is core iff c >= core * n, cloud iff c < cloud * n"""
    n = len(h) - 1
    k = [0.0, 0.0, 0.0]
    if occupied(h) == 0:
        return tuple(k)
    for c in range(1, n + 1):
        if int(h[c]) == 0:
            continue
        which = 0 if float(c) >= core * float(n) else 2 if float(c) < cloud * float(n) else 1
        k[which] += kmers(h, c, U)
    return tuple(k)


def curves(h, U):
    """(pan[m - 1], core[m - 1]) for m = 1 .. n: the expectations over all m-subsets,
    core(m) = U/occupied * sum_c hist[c] * prod_{i<m} (c-i)/(n-i), pan(m) = U/occupied * sum_c hist[c] * (1 - prod_{i<m} (n-c-i)/(n-i)),
    the products carried from m to m + 1 by one multiply and one divide, the sums in ascending c"""
    n = len(h) - 1
    pan, core = [0.0] * n, [0.0] * n
    if occupied(h) == 0:
        return pan, core
    cs = [c for c in range(1, n + 1) if int(h[c])]
    in_all, in_none = [1.0] * len(cs), [1.0] * len(cs)
    scale = float(U) / float(occupied(h))
    for m in range(1, n + 1):
        i = m - 1
        s_core = s_pan = 0.0
        for x, c in enumerate(cs):
            in_all[x] = in_all[x] * float(c - i) / float(n - i) if c > i else 0.0
            in_none[x] = in_none[x] * float(n - c - i) / float(n - i) if n - c > i else 0.0
            s_core += float(int(h[c])) * in_all[x]
            s_pan += float(int(h[c])) * (1.0 - in_none[x])
        core[i] = scale * s_core
        pan[i] = scale * s_pan
    return pan, core


def spectrum_text(names, hists, unions):
    """{OUT}_spectrum.tsv"""
    out = ["Group\tMembers\tCount\tBuckets\tKmers\n"]
    for name, h, U in zip(names, hists, unions):
        n = len(h) - 1
        if occupied(h) == 0:
            continue
        for c in range(1, n + 1):
            if int(h[c]):
                out.append("%s\t%d\t%d\t%d\t%.3f\n" % (name, n, c, int(h[c]), kmers(h, c, U)))
    return "".join(out)


def groups_text(names, hists, unions, core=0.95, cloud=0.15):
    """{OUT}_groups.tsv"""
    out = ["Group\tMembers\tOccupied\tUnion\tCore\tShell\tCloud\n"]
    for name, h, U in zip(names, hists, unions):
        out.append("%s\t%d\t%d\t%.3f\t%.3f\t%.3f\t%.3f\n" % ((name, len(h) - 1, occupied(h), float(U)) + classes(h, U, core, cloud)))
    return "".join(out)
