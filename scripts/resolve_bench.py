#!/usr/bin/env python3
"""Measurement of the resolution of a whole repeat in one call (include/pgr.h, pgr_msa_resolve) against the same windows
through the per-window entry points, on the benchmark MSA after one realignment round: one JSON line.
    python3 scripts/resolve_bench.py [--workload tree_default] [--rounds 1] [--parts 6] [--reps 5]
Preparation as scripts/gr_bench.py (the pipeline's MSA, one realignment round, MaxCorrelation); the windows are the `parts`
sections of window.window_boundaries.  The two legs alternate, `reps` times each, in one process on one device:
  one_call     pgr_msa_open (the upload, reported separately) + pgr_msa_resolve over all windows, with the breakdown of
               pgr_last_resolve_timing of every repetition;
  per_window   for every window pgr_refine, pgr_read_window, pgr_subdivide, pgr_kmeans_subdivide on the same text: what a
               sequence of `-f` runs computes, without their file reading.
The labels of the two legs are compared before any time is reported (the script fails if they differ).  Reported per leg:
every repetition, minimum, median, maximum."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"all": [round(x, 2) for x in v], "min": round(min(v), 2), "median": round(statistics.median(v), 2), "max": round(max(v), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tree_default")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--parts", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    from repeatresolver_amd import _lib
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd import resolution as rs
    from repeatresolver_amd.max_correlation import max_correlations
    from repeatresolver_amd.pipeline import initial_msa
    from repeatresolver_amd.realigner import PWReAligner
    from repeatresolver_amd.window import window_boundaries
    t0 = time.time()
    rows, _info = initial_msa(dg.CONFIGS[a.workload])
    g = PWReAligner(rows, bandwidth=1000)
    g.trim_ends()
    for _ in range(a.rounds):
        g.realign_round()
    rows = g.export_rows()
    g.close()
    T, W = len(rows), len(rows[0])
    mc = max_correlations(rows, a.cov)
    sites = window_boundaries(rows, 0.90, a.parts)
    text = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(T, W)
    del rows
    prep_s = time.time() - t0
    print(f"prepared in {prep_s:.0f} s: {T} x {W}, sites {sites}", file=sys.stderr, flush=True)
    lib = _lib.load()
    tp = ctypes.cast(text.ctypes.data, ctypes.c_char_p)
    mp = mc.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def per_window():
        labels, stages = [], [0.0, 0.0, 0.0, 0.0]
        for von, bis in zip(sites[:-1], sites[1:]):
            res, win, sub, kms = _lib.PgrResult(), _lib.PgrWindow(), _lib.PgrSubdivision(), _lib.PgrKmeans()
            t = [time.perf_counter()]
            rc = lib.pgr_refine(T, W, tp, mp, von, bis, a.cov, 0.0, 0, ctypes.byref(res))
            t.append(time.perf_counter())
            rc = rc or lib.pgr_read_window(T, W, tp, von, bis, ctypes.byref(win))
            t.append(time.perf_counter())
            rc = rc or lib.pgr_subdivide(ctypes.byref(win), ctypes.byref(res), a.cov, 0, ctypes.byref(sub))
            t.append(time.perf_counter())
            rc = rc or lib.pgr_kmeans_subdivide(ctypes.byref(win), ctypes.byref(res), sub.reldrop_labels, a.cov, 0, ctypes.byref(kms))
            t.append(time.perf_counter())
            if rc:
                raise SystemExit(f"per-window leg failed: {rc}")
            labels.append([np.ctypeslib.as_array(p, shape=(T,)).copy() for p in (sub.dropoff_labels, sub.reldrop_labels, kms.labels)])
            for i in range(4):
                stages[i] += (t[i + 1] - t[i]) * 1e3
            lib.pgr_kmeans_free(ctypes.byref(kms)); lib.pgr_subdivision_free(ctypes.byref(sub))
            lib.pgr_window_free(ctypes.byref(win)); lib.pgr_free(ctypes.byref(res))
        return labels, stages

    one_ms, upload_ms, per_ms, breakdown, per_stages = [], [], [], [], []
    windows = None
    for rep in range(a.reps):
        t0 = time.perf_counter()
        msa = rs.open_msa(text)
        t1 = time.perf_counter()
        got = rs.resolve(msa, mc, sites, a.cov)
        t2 = time.perf_counter()
        msa.close()
        tm = rs.last_timing()
        t3 = time.perf_counter()
        labels, stages = per_window()
        t4 = time.perf_counter()
        if rep == 0:
            for w, l in zip(got, labels):
                if not (np.array_equal(w.dropoff_labels, l[0]) and np.array_equal(w.reldrop_labels, l[1]) and np.array_equal(w.kmeans_labels, l[2])):
                    raise SystemExit(f"the labels of the two legs differ in window [{w.von}, {w.bis}]")
            windows = [{"von": w.von, "bis": w.bis, "kept_rows": w.kept_rows, "parts": [w.dropoff_parts, w.reldrop_parts, w.kmeans_parts]} for w in got]
        upload_ms.append((t1 - t0) * 1e3); one_ms.append((t2 - t1) * 1e3); per_ms.append((t4 - t3) * 1e3)
        print(f"rep {rep}: upload {upload_ms[-1]:.0f} ms, one call {one_ms[-1]:.0f} ms, per window {per_ms[-1]:.0f} ms", file=sys.stderr, flush=True)
        breakdown.append({k: round(v, 2) for k, v in tm.items()})
        per_stages.append({k: round(v, 2) for k, v in zip(("refine_ms", "read_window_ms", "subdivide_ms", "kmeans_ms"), stages)})
    con = rs.connect([w.kmeans_labels for w in got]) if len(got) > 1 else None
    out = {"metric": "six-window resolution, one call over per-window calls", "value": statistics.median(per_ms) / statistics.median(one_ms),
           "unit": "x (median wall of the per-window leg / median wall of pgr_msa_resolve, upload excluded)",
           "workload": f"{a.workload}: pipeline MSA after {a.rounds} realignment round(s), {T} rows x {W} columns, {len(sites) - 1} windows "
                       f"of window_boundaries, cov {a.cov}",
           "sites": sites, "windows": windows, "labels_equal": True, "reps": a.reps,
           "one_call_ms": spread(one_ms), "upload_ms": spread(upload_ms), "per_window_ms": spread(per_ms),
           "resolve_timing_ms": breakdown, "per_window_stage_ms": per_stages, "prepare_s": round(prep_s, 1),
           "connection": None if con is None else {"shape": list(con.matrix.shape), "mutual": int(con.mutual.sum()),
                                                   "confidence_over_0.5": int((con.confidence > 0.5).sum())}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
