#!/usr/bin/env python3
"""Generate tests/golden/hmh_rare_ranks.json: 32-bit HyperMinHash inputs of ranks that random genomes never reach.

HyperMinHash hashes (masked as u32).to_le_bytes() with XXH3-128 (utils.rs:397), which cannot be inverted — but there are only 2^32
inputs, so the oracle hashes all of them (oracle/lash_oracle.c lash_or_hmh_rank_search, about 5 s per (seed, variant) on 16 threads) and
this script keeps, per seed and per variant (x = the high or the low half of the hash), the inputs `w` with lzm1 = lz - 1 =
clz64((x << 14) ^ 0x3FFF) at or above a floor, plus a ladder of single inputs and same-bucket pairs around the kernels' thresholds:
    seed 42 (the default)   every w with lzm1 >= 20;
                            per lzm1 in 12 .. 19 (both threshold caps, 14 and 16, both REDO_BELOW values and the 18-bit fast form lie inside):
                            the first SINGLES inputs, and the first PAIRS pairs that share bucket and rank and differ in the signature
    seeds 0, 1, 11          every w with lzm1 >= 24 (seed 42 has nothing above 30; these have 32, 33, 35, 36 and 38: registers >= 0x8000)
The file holds ONLY the inputs, as hex; bucket, rank and signature are recomputed by whoever reads it (tests/test_hmh_rare_ranks.py checks
them with two independent hash restatements).  No test runs this script; rerunning it reproduces the committed file byte for byte.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O

BULK_SEED, BULK_FLOOR = 42, 20
RARE_SEEDS, RARE_FLOOR = (0, 1, 11), 24
LADDER = range(12, 20)
SINGLES, PAIRS = 4, 6
THREADS = 16


def hexes(ws):
    return " ".join("%08x" % int(w) for w in ws)


def main():
    groups = []
    for x in ("high", "low"):
        w, reg = O.hmh_rank_search(BULK_SEED, x == "low", LADDER[0], THREADS)
        lzm1 = ((reg >> 10) & 63).astype(np.int64) - 1
        groups.append(dict(seed=BULK_SEED, x=x, kind="floor", min_lzm1=BULK_FLOOR, w=hexes(w[lzm1 >= BULK_FLOOR])))
        for z in LADDER:
            at = np.flatnonzero(lzm1 == z)
            groups.append(dict(seed=BULK_SEED, x=x, kind="single", lzm1=z, w=hexes(w[at[:SINGLES]])))
            first, pairs = {}, []                      # bucket -> the first input seen there; a bucket gives one pair at the most
            for i in at:
                b, sig = int(reg[i]) >> 16, int(reg[i]) & 0x3FF
                if b not in first:
                    first[b] = i
                elif first[b] is not None and (int(reg[first[b]]) & 0x3FF) != sig:
                    pairs += [w[first[b]], w[i]]
                    first[b] = None
                    if len(pairs) == 2 * PAIRS:
                        break
            groups.append(dict(seed=BULK_SEED, x=x, kind="pair", lzm1=z, w=hexes(pairs)))
    for seed in RARE_SEEDS:
        for x in ("high", "low"):
            w, _ = O.hmh_rank_search(seed, x == "low", RARE_FLOOR, THREADS)
            groups.append(dict(seed=seed, x=x, kind="floor", min_lzm1=RARE_FLOOR, w=hexes(w)))
    path = os.path.join(HERE, "hmh_rare_ranks.json")
    with open(path, "w") as f:
        f.write('{"what":"xxh3_128 inputs (hex u32) of rare HyperMinHash ranks; made by make_hmh_rare_ranks.py; `pair`: two consecutive inputs",\n'
                ' "groups":[\n')
        f.write(",\n".join("  " + json.dumps(g, separators=(",", ":")) for g in groups))
        f.write("\n ]}\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
