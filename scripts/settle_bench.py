#!/usr/bin/env python3
"""Measurement of the settled labelling (include/pgr.h, pgr_msa_settle) at the size of the benchmark, beside the same loop
composed from the existing public calls in the same process: one JSON document.
    python3 scripts/settle_bench.py [--workload tree_default] [--reps 5] [--out profiles/settle_bench.json]
Input: that of scripts/assign_bench.py -- the MSA datagen stacks from the true alignments of the workload's reads with the gaps at
the rows' ends turned into blanks, MaxCorrelation's vector of that MSA and the cutoff RepeatResolver defaults to (RR:3977), the whole
width as the window.  The labelling is degraded: only the rows that span the window of a sixth of the width in the middle of the
MSA carry their true copy as label, and a share of them (--wrong, a tenth) the label of another copy.  `settle` (free: the wrong
labels may move) and the loop consensus / assign / Assignment.labels from the same labelling; every field of the two results is
compared first (the script fails if they differ), then both run --reps times.  Reported: the median of every bucket of
pgr_last_settle_timing, the time per iteration of both (settle: its iterations bucket; the composition: the wall time of the loop,
and the sum of pgr_last_consensus_timing and pgr_last_assign_timing, which leaves out Python), the iterations, and the share of
the labelled rows on their true copy before and after.  The composition's calls are unchanged by pgr_msa_settle: its time is
what the loop cost before."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
FIELDS = ("compared", "best", "second", "best_mismatches", "second_mismatches")


def spread(v):
    return {"all": [round(x, 3) for x in v], "min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def composed(rs, msa, labels, mc, cutoff, min_compared, min_margin, max_iter, hold):
    """the loop of the header from the public calls; (result dict, wall ms of the loop, ms inside the two entries)"""
    import numpy as np
    lab, history, last, stop, inside = labels.copy(), [], None, "MAX_ITER", 0.0
    t0 = time.perf_counter()
    for _ in range(max_iter):
        con = rs.consensus(msa, lab, maxcorrs=mc, cutoff=cutoff)
        inside += rs.last_consensus_timing()["all_ms"]
        try:
            a = rs.assign(msa, con)
        except ValueError:
            stop = "NO_COLUMN"
            break
        inside += rs.last_assign_timing()["all_ms"]
        new = a.labels(min_compared, min_margin, keep=labels if hold else None)
        changed = int((new != lab).sum())
        history.append((changed, con.parts, len(a.columns)))
        last = a
        if changed == 0:
            stop = "CONVERGED"
            break
        if not (new >= 0).any():
            stop = "EMPTY"
            break
        lab = new
    wall = (time.perf_counter() - t0) * 1e3
    out = {"labels": lab, "stop": stop, "iterations": len(history), "changed": np.array([h[0] for h in history]),
           "parts_at": np.array([h[1] for h in history]), "ncolumns_at": np.array([h[2] for h in history])}
    for name in ("part_label", "columns") + FIELDS:
        out[name] = None if last is None else getattr(last, name)
    return out, wall, inside


def compare(got, exp):
    import numpy as np
    if (got.stop, got.iterations) != (exp["stop"], exp["iterations"]):
        raise SystemExit(f"settle stopped with {got.stop} after {got.iterations}, the composition with {exp['stop']} after {exp['iterations']}")
    for name in ("labels", "changed", "parts_at", "ncolumns_at", "part_label", "columns") + FIELDS:
        a, b = getattr(got, name), exp[name]
        if (a is None) != (b is None) or (a is not None and not np.array_equal(a, b)):
            raise SystemExit(f"{name} of settle and of the composition differ")


def share_true(labels, truth):
    inside = labels >= 0
    return {"rows_labelled": int(inside.sum()), "on_their_true_copy": round(float((labels[inside] == truth[inside]).mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tree_default")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--wrong", type=float, default=0.10, help="share of the labelled rows that start under another copy's label")
    ap.add_argument("--min-compared", type=int, default=100)
    ap.add_argument("--min-margin", type=int, default=4)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "settle_bench.json"))
    a = ap.parse_args()
    import numpy as np
    from assign_bench import trim_ends
    from repeatresolver_amd import _lib
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd import resolution as rs
    from repeatresolver_amd.max_correlation import max_correlations
    t0 = time.time()
    data = dg.simulate(dg.CONFIGS[a.workload])
    text = trim_ends(np.ascontiguousarray(dg.build_msa(data)))
    truth = np.array(data.copy_of, dtype=np.int32)
    T, W = text.shape
    mc = max_correlations([r.tobytes() for r in text], a.cov)
    cutoff = float(_lib.load().pgr_default_cutoff(ctypes.c_double(0.0), W))
    von = W // 2
    bis = von + W // 6
    spans = (text[:, von] != ord(" ")) & (text[:, bis] != ord(" "))
    labels = np.where(spans, truth, -1).astype(np.int32)
    rng = np.random.default_rng(1)
    copies = np.unique(truth)
    inside = np.nonzero(spans)[0]
    bad = rng.choice(inside, size=int(a.wrong * len(inside)), replace=False)
    labels[bad] = copies[(np.searchsorted(copies, truth[bad]) + rng.integers(1, len(copies), len(bad))) % len(copies)]
    prep_s = time.time() - t0
    nsel = int((mc.reshape(-1, 5).max(axis=1) > cutoff).sum())
    print(f"prepared in {prep_s:.0f} s: {T} x {W}, {len(copies)} copies, cutoff {cutoff:.3f}, {nsel} columns over it, {len(inside)} rows "
          f"labelled, {len(bad)} of them wrongly", file=sys.stderr, flush=True)
    kw = dict(min_compared=a.min_compared, min_margin=a.min_margin, max_iter=a.max_iter)
    out = {"metric": "pgr_msa_settle at the benchmark's size, beside the composition of pgr_msa_consensus and pgr_msa_assign",
           "unit": "ms, median of the repetitions", "reps": a.reps, "cutoff": cutoff, "prepare_s": round(prep_s, 1),
           "workload": f"{a.workload}: datagen's MSA of the true alignments, {T} rows x {W} columns, whole width, {nsel} selected columns; "
                       f"labelled: the {len(inside)} rows spanning [{von}, {bis}], {len(bad)} of them under another copy's label",
           "thresholds": kw, "before": share_true(labels, truth)}
    with rs.open_msa(text) as msa:
        for mode, hold in (("free", False), ("hold", True)):
            got = rs.settle(msa, labels, maxcorrs=mc, cutoff=cutoff, hold=hold, **kw)         # (the first call of the process: not timed)
            exp, _, _ = composed(rs, msa, labels, mc, cutoff, hold=hold, **kw)
            compare(got, exp)
            timing, wall, cwall, cinside = [], [], [], []
            for rep in range(a.reps):
                t = time.perf_counter()
                got = rs.settle(msa, labels, maxcorrs=mc, cutoff=cutoff, hold=hold, **kw)
                wall.append((time.perf_counter() - t) * 1e3)
                timing.append({k: round(v, 3) for k, v in rs.last_settle_timing().items()})
                exp, w, i = composed(rs, msa, labels, mc, cutoff, hold=hold, **kw)
                cwall.append(w)
                cinside.append(i)
                compare(got, exp)
                print(f"{mode}, rep {rep}: settle {timing[-1]}, composition {w:.1f} ms ({i:.1f} ms inside the entries)", file=sys.stderr, flush=True)
            n = got.iterations
            med = {k: statistics.median(t[k] for t in timing) for k in timing[0]}
            out[mode] = {"stop": got.stop, "iterations": n, "changed": got.changed.tolist(), "parts_at": got.parts_at.tolist(),
                         "ncolumns_at": got.ncolumns_at.tolist(), "after": share_true(got.labels, truth), "equal_to_the_composition": True,
                         "settle_timing_ms": timing, "settle_median_ms": {k: round(v, 3) for k, v in med.items()},
                         "settle_wall_ms_with_python": spread(wall), "settle_ms_per_iteration": round(med["iterations_ms"] / max(n, 1), 3),
                         "composition_wall_ms": spread(cwall), "composition_ms_inside_the_entries": spread(cinside),
                         "composition_ms_per_iteration": round(statistics.median(cwall) / max(n, 1), 3),
                         "composition_ms_per_iteration_inside_the_entries": round(statistics.median(cinside) / max(n, 1), 3),
                         "planes_bytes_resident": 32 * ((nsel + 63) // 64) * T}
        out["value"] = out["free"]["settle_ms_per_iteration"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("free", "hold")} |
                     {m: {k: out[m][k] for k in ("stop", "iterations", "after", "settle_median_ms", "settle_ms_per_iteration",
                                                 "composition_ms_per_iteration", "composition_ms_per_iteration_inside_the_entries")}
                      for m in ("free", "hold")}))


if __name__ == "__main__":
    main()
