"""The table DESIGN 23 chooses max_permille by, made with the checker (tests/fl_checker.py) on the CPU: for the flanks of
datagen.simulate_dataset's true cut, per bucket of m = min(a_i, a_j), the same-copy and different-copy rates 1000 * d / m,
and the components single linkage makes of them at --permille.

  python scripts/flank_rates.py toy_b tree_medium transposon_like --reach 256 128 --out rates.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fl_checker as fc                                   # noqa: E402
from repeatresolver_amd import datagen as dg              # noqa: E402


def side_flanks(cfg, side):
    pieces, piece_read, classes, copy = fc.true_flanks(cfg)
    nb = fc.neighbours(piece_read, classes)
    col = 1 if side == "left" else 3
    rows = [r for r in nb if r[col] >= 0]
    return pieces, [r[col] for r in rows], [r[col + 1] for r in rows], [copy[r[0]] for r in rows]


def rates(cfg, side, reach, min_len, permille):
    pieces, piece, mode, copy = side_flanks(cfg, side)
    a, dist = fc.distances(pieces, piece, mode, reach, min_len)
    keep = np.nonzero(np.diag(dist) == 0)[0]
    i, j = np.triu_indices(len(keep), 1)
    i, j = keep[i], keep[j]
    m = np.minimum(a[i], a[j]).astype(np.int64)
    rate = 1000 * dist[i, j].astype(np.int64) // m
    same = np.asarray(copy)[i] == np.asarray(copy)[j]
    edges = sorted({min_len, reach + 1} | {reach * k // 8 for k in range(4, 9) if reach * k // 8 > min_len})
    buckets = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (m >= lo) & (m < hi)
        s, d = rate[sel & same], rate[sel & ~same]
        buckets.append({"m": [int(lo), int(hi - 1)], "same_pairs": int(s.size), "diff_pairs": int(d.size),
                        "same_p50": int(np.percentile(s, 50)) if s.size else None,
                        "same_p99": int(np.percentile(s, 99)) if s.size else None,
                        "same_max": int(s.max()) if s.size else None,
                        "diff_p1": int(np.percentile(d, 1)) if d.size else None,
                        "diff_min": int(d.min()) if d.size else None})
    label = fc.cluster(a, dist, permille, 1)
    comps = {}
    for k in keep:
        comps.setdefault(int(label[k]), set()).add(copy[k])
    return {"side": side, "reach": reach, "min_len": min_len, "flanks": int(len(piece)), "kept": int(len(keep)),
            "copies_with_a_flank": len({copy[k] for k in keep}), "permille": permille, "components": len(comps),
            "mixed_components": sum(len(v) > 1 for v in comps.values()), "buckets": buckets}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+")
    ap.add_argument("--reach", type=int, nargs="+", default=[256])
    ap.add_argument("--min-len", type=int, default=100)
    ap.add_argument("--permille", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    for name in args.configs:
        for reach in args.reach:
            for side in ("left", "right"):
                t0 = time.time()
                r = rates(dg.CONFIGS[name], side, reach, args.min_len, args.permille)
                r["config"], r["checker_s"] = name, round(time.time() - t0, 1)
                print(json.dumps(r), flush=True)
                out.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
