#!/usr/bin/env python3
"""Measurement of the HIP group refinement (include/pgr.h) on one Window.py section of the benchmark MSA after one
realignment round: one JSON line.
    python3 scripts/gr_bench.py [--workload tree_default] [--rounds 1] [--von V --bis B | --section-width 5000] [--cpu-sig 3]
`value` = pairs (significant variation a, variation i of the window) scanned per second of the clique kernel: four bit-set
intersections each, and one hypergeometric tail where the intersection is large enough -- the per-pair arithmetic of
MaxCorrelation's k_mc_pairs (scripts/mc_bench.py), whose rate on the same MSA is measured alongside as the yardstick.
CPU baseline: the literal restatement tests/gr_checker.py on --cpu-sig significant variations of the same window (one
core, Python: a checker, not an optimised port), whose cliques must equal the device's.
"subdivision": the two drop-off subdivisions on the same window after the refinement (include/pgr.h, pgr_subdivide): the
exchange sort, the rest of stage 1, upload, k_gr_reldrop and the apply step, ms, and the kernel's time over k_gr_votes'
(votes_ms, which also holds the refinement's downloads).
"kmeans": the last stage on the same window (pgr_kmeans_subdivide): counts, the significance kernel k_km_pairs, the k-means
kernels and the host chain, ms, and k_km_pairs' pairs/s (a pair is evaluated from both of its sides) beside k_mc_pairs'."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tree_default")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--von", type=int, default=None)
    ap.add_argument("--bis", type=int, default=None)
    ap.add_argument("--section-width", type=int, default=5000)
    ap.add_argument("--cpu-sig", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd import group_refinement as gr
    from repeatresolver_amd.max_correlation import last_timing as mc_timing, max_correlations
    from repeatresolver_amd.pipeline import initial_msa
    from repeatresolver_amd.realigner import PWReAligner
    t0 = time.time()
    rows, info = initial_msa(dg.CONFIGS[a.workload])
    g = PWReAligner(rows, bandwidth=1000)
    g.trim_ends()
    for _ in range(a.rounds):
        g.realign_round()
    rows = g.export_rows()
    g.close()
    T, W = len(rows), len(rows[0])
    mc = max_correlations(rows, a.cov)
    mc = max_correlations(rows, a.cov)
    mct = mc_timing()
    prep_s = time.time() - t0
    von = a.von if a.von is not None else max(0, W // 2 - a.section_width // 2)
    bis = a.bis if a.bis is not None else min(W - 1, von + a.section_width - 1)
    walls = []
    for _ in range(2):
        t0 = time.time()
        res = gr.refine_groups(rows, mc, von, bis, a.cov)
        walls.append(time.time() - t0)
    tm = gr.last_timing()
    from repeatresolver_amd import subdivision as sdv
    for _ in range(2):
        t0 = time.time()
        sub = sdv.subdivide(rows, res, von, bis, a.cov)
        sub_wall = time.time() - t0
    st = sdv.last_timing()
    from repeatresolver_amd import kmeans_subdivision as kmv
    for _ in range(2):
        t0 = time.time()
        kms = kmv.kmeans_subdivide(rows, res, sub, von, bis, a.cov)
        km_wall = time.time() - t0
    kt = kmv.last_timing()
    out = {"metric": "group refinement clique pairs/sec", "value": tm["pairs"] / (tm["cliques_ms"] * 1e-3), "unit": "pairs/s",
           "workload": f"{a.workload}: pipeline MSA after {a.rounds} realignment round(s), {T} rows x {W} columns; window [{von}, {bis}], "
                       f"{int(res.kept.sum())} kept rows, {len(res.significant)} significant of {res.width * 5} variations, cov {a.cov}",
           "pairs": tm["pairs"], "timing_ms": {k: round(v, 2) for k, v in tm.items() if k != "pairs"}, "wall_s": round(min(walls), 3),
           "pairs_per_s_of_whole_call": tm["pairs"] / (tm["total_ms"] * 1e-3), "cutoff": res.cutoff,
           "refined": int((res.sizes > 5).sum()), "dropped": int((res.sizes <= 5).sum()),
           "k_mc_pairs_same_msa": {"pairs": mct["pairs"], "pairs_ms": round(mct["pairs_ms"], 1),
                                   "pairs_per_s": mct["pairs"] / (mct["pairs_ms"] * 1e-3)},
           "prepare_s": round(prep_s, 1),
           "subdivision": {"timing_ms": {k: round(v, 3) for k, v in st.items()}, "wall_s": round(sub_wall, 3), "selected": sub.selected,
                           "dropoff_parts": sub.dropoff_parts, "eligible": sub.eligible, "reldrop_parts": sub.reldrop_parts,
                           "k_gr_reldrop_over_k_gr_votes": round(st["kernel_ms"] / tm["votes_ms"], 3) if tm["votes_ms"] else None},
           "kmeans": {"timing_ms": {k: round(v, 3) for k, v in kt.items() if k != "pairs"}, "wall_s": round(km_wall, 3), "eligible": kms.eligible,
                      "parts": kms.parts, "varzahl": [len(v) for v in kms.vars][:16], "pairs": kt["pairs"],
                      "k_km_pairs_per_s": kt["pairs"] / (kt["pairs_ms"] * 1e-3) if kt["pairs_ms"] else None}}
    if a.cpu_sig and len(res.significant):
        import gr_checker as gc
        win = gc.Window(rows, mc, von, bis, a.cov)
        pick = np.linspace(0, len(res.significant) - 1, min(a.cpu_sig, len(res.significant))).astype(int)
        t0 = time.time()
        same = sum(list(res.cliques[s]) == win.cliquer(int(res.significant[s]))[0] for s in pick)
        cs = time.time() - t0
        out["cpu_baseline"] = {"value": len(pick) * (res.width * 5 - 1) / cs, "unit": "pairs/s", "cores": 1, "kind": "checker (Python)",
                               "sample": f"{len(pick)} significant variations of the same window, {cs:.1f} s; {same} of {len(pick)} cliques equal to the GPU's"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
