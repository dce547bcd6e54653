"""The flank distances at the benchmark's size (not bench.py: the flagship workload is the realigner's): the flanks of
tree_default's true cut (tests/fl_checker.true_flanks), both sides, through flanks.FlankClusterer.distances on the GPU and
flanks.cluster at --permille.  Writes n, cells, kernel ms and call ms per side, the components against the 100 copies, and the
checker's one-core time EXTRAPOLATED from a sample of patterns (the file says so) to profiles/flank_bench.json.

  python scripts/flank_bench.py [--config tree_default] [--permille 400] [--sample 6] [--out profiles/flank_bench.json]
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
from repeatresolver_amd import flanks                     # noqa: E402


def checker_rate(pieces, piece, mode, reach, min_len, sample, seed=1):
    """cells per second of the checker on `sample` patterns drawn evenly from the sorted order, each against all its texts"""
    lens = np.array([len(pieces[p]) for p in piece])
    a = np.minimum(lens, reach)
    order = sorted((k for k in range(len(piece)) if lens[k] >= min_len), key=lambda k: (a[k], k))
    picks = sorted({int(v) for v in np.linspace(0, max(len(order) - 2, 0), sample)})
    cells, pairs, t = 0, 0, 0.0
    for pos in picks:
        i, rest = order[pos], order[pos + 1:]
        m = int(a[i])
        tl = [min(int(lens[j]), m + m // 4) for j in rest]
        T = np.full((len(rest), max(tl)), 200, dtype=np.uint8)
        for r, j in enumerate(rest):
            T[r, :tl[r]] = fc.anchored(pieces[piece[j]], mode[j])[:tl[r]]
        P = fc.anchored(pieces[piece[i]], mode[i])[:m]
        t0 = time.perf_counter()
        fc._last_rows(P, T)
        t += time.perf_counter() - t0
        cells += m * sum(tl)
        pairs += len(rest)
    return cells / t, pairs, len(picks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tree_default")
    ap.add_argument("--permille", type=int, default=400)
    ap.add_argument("--reach", type=int, default=256)
    ap.add_argument("--min-len", type=int, default=100)
    ap.add_argument("--sample", type=int, default=6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flank_bench.json"))
    args = ap.parse_args()
    cfg = dg.CONFIGS[args.config]
    t0 = time.time()
    pieces, piece_read, classes, copy = fc.true_flanks(cfg)
    nb = fc.neighbours(piece_read, classes)
    out = {"config": args.config, "copies": cfg.copies, "reach": args.reach, "min_len": args.min_len, "max_permille": args.permille,
           "pieces": len(pieces), "rows": len(nb), "simulate_s": round(time.time() - t0, 1), "sides": []}
    with flanks.FlankClusterer() as g:
        for side, col in (("left", 1), ("right", 3)):
            rows = [r for r in nb if r[col] >= 0]
            piece, mode, cp = [r[col] for r in rows], [r[col + 1] for r in rows], [copy[r[0]] for r in rows]
            g.distances(pieces, piece[:130], mode[:130], args.reach, args.min_len)             # warm-up: module load, first launch
            best = None
            for _ in range(args.repeat):
                before = g.stats()
                t1 = time.perf_counter()
                lens, dist = g.distances(pieces, piece, mode, args.reach, args.min_len)
                call_ms = (time.perf_counter() - t1) * 1e3
                st = g.stats()
                run = {"call_ms": round(call_ms, 2), "kernel_ms": round(st["kernel_ms"] - before["kernel_ms"], 3),
                       "cells": st["cells"] - before["cells"]}
                if best is None or run["kernel_ms"] < best["kernel_ms"]:
                    best = run
            a = np.minimum(lens, args.reach)
            t1 = time.perf_counter()
            label = flanks.cluster(a, dist, args.permille)
            cluster_ms = (time.perf_counter() - t1) * 1e3
            kept = [k for k in range(len(piece)) if lens[k] >= args.min_len]
            comps = {}
            for k in kept:
                comps.setdefault(int(label[k]), set()).add(cp[k])
            rate, pairs, npat = checker_rate(pieces, piece, mode, args.reach, args.min_len, args.sample)
            # spot check: the sampled patterns' first texts against the checker, entry for entry
            sub = kept[:: max(1, len(kept) // 40)][:40]
            _a, exp = fc.distances(pieces, [piece[k] for k in sub], [mode[k] for k in sub], args.reach, args.min_len)
            _l, got = g.distances(pieces, [piece[k] for k in sub], [mode[k] for k in sub], args.reach, args.min_len)
            side_out = {"side": side, "n": len(piece), "n_of_min_len": len(kept), "pairs": len(kept) * (len(kept) - 1) // 2, **best,
                        "cells_per_s": round(best["cells"] / (best["kernel_ms"] / 1e3)) if best["kernel_ms"] > 0 else None,
                        "cluster_ms": round(cluster_ms, 2), "components": len(comps), "copies_with_a_flank": len({cp[k] for k in kept}),
                        "mixed_components": sum(len(v) > 1 for v in comps.values()),
                        "checker_one_core_s_EXTRAPOLATED": round(best["cells"] / rate, 1),
                        "checker_sample": f"{npat} patterns evenly spaced in the sorted order, each against all its texts: {pairs} pairs; "
                                          "the total is cells / (sampled cells per second), not a measurement",
                        "spot_check_equal_to_checker": bool((got == exp).all()), "spot_check_flanks": len(sub)}
            print(json.dumps(side_out), flush=True)
            out["sides"].append(side_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
