"""The locus anchorer at the size it is meant for (not bench.py: the flagship workload is the realigner's): tree_default's 100
true loci (datagen.true_loci), their 200 flank patterns at --reach, both orientations, searched in a random assembly of --bases
bases in --contigs contigs with every locus planted once, + and - alternating.  Writes to profiles/anchor_bench.json: the time
of pla_open_text, of k_la_search (device events) and of the whole call, pattern rows x text columns per second, the same per
chunk size, whether every planted flank is the one hit of its pattern, and the numpy checker's one-core time EXTRAPOLATED by
cells from a sample (the file says so).

  python scripts/anchor_bench.py [--bases 100000000] [--contigs 100] [--reach 256] [--permille 50] [--chunks 512,1024,2048,4096,8192]
                                 [--out profiles/anchor_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import la_checker as la                                   # noqa: E402
from repeatresolver_amd import anchors                    # noqa: E402
from repeatresolver_amd import datagen as dg              # noqa: E402
from repeatresolver_amd.strands import reverse_complement  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="tree_default")
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--contigs", type=int, default=100)
    ap.add_argument("--reach", type=int, default=256)
    ap.add_argument("--permille", type=int, default=50)
    ap.add_argument("--chunks", default="512,1024,2048,4096,8192")
    ap.add_argument("--sample-columns", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_bench.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(26)
    text = lambda a: dg.ASCII[a].tobytes()
    loci = [tuple(text(p) for p in l) for l in dg.true_loci(dg.CONFIGS[args.config])]
    per = args.bases // args.contigs
    # contig j: random bases with the loci j, j + contigs, ... planted at even distances, every other one reverse-complemented
    contigs, truth = [], {}
    for j in range(args.contigs):
        mine = list(range(j, len(loci), args.contigs))
        room = per - sum(len(b"".join(loci[i])) for i in mine)
        gaps = [room // (len(mine) + 1)] * len(mine) + [room - room // (len(mine) + 1) * len(mine)]
        parts, at = [], 0
        for i, gap in zip(mine, gaps):
            parts.append(text(rng.integers(0, 4, size=gap, dtype=np.uint8)))
            at += gap
            left, copy, right = loci[i]
            whole = left + copy + right
            if i % 2:
                parts.append(reverse_complement(whole))
                truth[i] = (j, 1, at + len(right) + len(copy), at + len(right))
            else:
                parts.append(whole)
                truth[i] = (j, 0, at + len(left), at + len(left) + len(copy))
            at += len(whole)
        parts.append(text(rng.integers(0, 4, size=gaps[-1], dtype=np.uint8)))
        contigs.append((f"contig{j}", b"".join(parts)))
    anchored = [x for left, _copy, right in loci for x in (left[::-1], right)]
    side = [0, 1] * len(loci)
    out = {"config": args.config, "loci": len(loci), "patterns": len(anchored), "reach": args.reach, "max_permille": args.permille,
           "bases": sum(len(s) for _, s in contigs), "contigs": len(contigs), "text_layout": "one code per byte in the file's order, a lane reads its own chunk",
           "interleaved_layout": "not built: no number"}
    t0 = time.perf_counter()
    g = anchors.LocusAnchorer(contigs)
    out["open_text_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    runs = []
    for chunk in [int(c) for c in args.chunks.split(",")]:
        g.set_chunk(chunk)
        for rep in range(2):                                                        # (the first search at a chunk size makes the chunks)
            before = g.stats()
            t0 = time.perf_counter()
            hits = g.search(anchored, side, max_permille=args.permille, reach=args.reach, min_len=100)
            call = (time.perf_counter() - t0) * 1e3
            after = g.stats()
        cells, ms = after["cells"] - before["cells"], after["kernel_ms"] - before["kernel_ms"]
        want = sorted((2 * i + s, o, c, (bl, br)[s]) for i, (c, o, bl, br) in truth.items() for s in (0, 1))
        runs.append({"chunk": chunk, "k_la_search_ms": round(ms, 2), "call_ms": round(call, 1), "cells": cells,
                     "cells_per_second": round(cells / (ms * 1e-3)), "hits": len(hits),
                     "every_planted_flank_is_its_patterns_one_hit": [h[:4] for h in hits.rows()] == want})
        print(runs[-1], flush=True)
    g.close()
    out["runs"] = runs
    # the checker on a sample: two patterns against the first --sample-columns of a contig, extrapolated by cells
    sample = contigs[0][1][:args.sample_columns]
    t0 = time.perf_counter()
    la.search([sample], anchored[:2], side[:2], args.reach, 100, args.permille)
    took = time.perf_counter() - t0
    sample_cells = 2 * 2 * args.reach * len(sample)
    out["checker"] = {"sample_cells": sample_cells, "sample_seconds": round(took, 2),
                      "EXTRAPOLATED_seconds_for_all_cells": round(took * runs[0]["cells"] / sample_cells),
                      "note": "numpy on one core, extrapolated by cells from the sample: an estimate, not a measurement"}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["checker"]))


if __name__ == "__main__":
    main()
