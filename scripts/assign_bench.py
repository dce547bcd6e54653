#!/usr/bin/env python3
"""Measurement of the assignment of every row to a copy (include/pgr.h, pgr_msa_assign) at the size of the benchmark, and the
table that guides the choice of Assignment.labels' two thresholds: one JSON document.
    python3 scripts/assign_bench.py [--workload tree_default] [--reps 5] [--out profiles/assign_bench.json]
Input: the MSA datagen stacks from the true alignments of the workload's reads (datagen.simulate + build_msa: the shape of the
benchmark's MSA, no aligner run needed) with the gaps at the rows' ends turned into blanks as PW_ReAligner's trim does, the
reads' true copy ids as the labelling, MaxCorrelation's vector of that MSA and the
cutoff RepeatResolver defaults to (RR:3977) for the selected columns; the whole width as the window.  `consensus`, then `assign`
once over the selected columns and once with all_columns=True.  Before any time is reported every field of one call is compared
with tests/as_checker.numpy_assign, column chunk by column chunk (the script fails if they differ).  Reported: the median of every
bucket of pgr_last_assign_timing; the bytes of the text the planes kernel reads per second of its time; the 64-bit operations
of the distance kernel (rows x parts x words x 8) per second of the distance and best kernels; and the time of the numpy
restatement on one core (threadpoolctl holds the BLAS to one thread) -- the baseline, never the code under test.

The threshold table: one window of a sixth of the width in the middle of the MSA (Window.py -p 6), labelled with the true copy
are only the rows that span it, as RepeatResolver's reader keeps them; `consensus` on the selected columns of the window, `assign`,
and over a grid of min_compared x min_margin: the share of the labelled rows whose best is their own copy (the same in every
cell), the rows recruited, and the share of the recruits whose true copy is the one they joined (the majority truth of a part
is its label here)."""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 8e12
FIELDS = ("compared", "best", "second", "best_mismatches", "second_mismatches")


def spread(v):
    return {"all": [round(x, 3) for x in v], "min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def trim_ends(text, step=1024):
    """build_msa fills a row with '-' from end to end; PW_ReAligner's first step turns the gaps before a row's first and behind
    its last base into blanks (pwr_trim_ends), and so does this: a read then covers what it covers"""
    import numpy as np
    W = text.shape[1]
    cols = np.arange(W)
    for at in range(0, len(text), step):
        part = text[at:at + step]
        base = part != ord("-")
        first, last = base.argmax(axis=1), W - 1 - base[:, ::-1].argmax(axis=1)
        part[(cols < first[:, None]) | (cols > last[:, None]) | ~base.any(axis=1)[:, None]] = ord(" ")
    return text


def one_thread():
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=1), 1
    except ImportError:
        return contextlib.nullcontext(), None


def numpy_baseline(text, codes, von, columns, chunk=8192):
    """as_checker.numpy_assign over chunks of columns (the one-hot matrices of all columns at once would not fit): the matrix of
    mismatches and compared add up over the chunks; best and second from the sums"""
    import numpy as np
    import as_checker as ac
    T, P = text.shape[0], codes.shape[0]
    mism, compared = np.zeros((T, P), dtype=np.int32), np.zeros(T, dtype=np.int32)
    for at in range(0, len(columns), chunk):
        part = ac.numpy_assign(text, codes, von, columns[at:at + chunk])
        mism += part["mismatches"]
        compared += part["compared"]
    order = np.argsort(mism, axis=1, kind="stable")                    # (stable: the lowest index among equals first)
    best, second = order[:, 0].astype(np.int32), (order[:, 1] if P > 1 else np.full(T, -1)).astype(np.int32)
    rows, none = np.arange(T), compared == 0
    return {"compared": compared, "best": np.where(none, -1, best), "second": np.where(none, -1, second),
            "best_mismatches": np.where(none, 0, mism[rows, best]), "second_mismatches": np.where(none | (second < 0), 0, mism[rows, second]),
            "mismatches": mism}


def measure(rs, msa, con, text, reps, all_columns, baseline):
    import numpy as np
    timing, wall = [], []
    for rep in range(reps):
        t = time.perf_counter()
        a = rs.assign(msa, con, all_columns=all_columns)
        wall.append((time.perf_counter() - t) * 1e3)
        timing.append({k: round(v, 3) for k, v in rs.last_assign_timing().items()})
        print(f"{'all' if all_columns else 'selected'} columns, rep {rep}: {timing[-1]}", file=sys.stderr, flush=True)
    full = rs.assign(msa, con, all_columns=all_columns, matrix=True)
    with_matrix = {k: round(v, 3) for k, v in rs.last_assign_timing().items()}
    T, P, C = text.shape[0], con.parts, len(a.columns)
    words = (C + 63) // 64
    base_s = threads = None
    if baseline:
        limit, threads = one_thread()
        with limit:
            t = time.perf_counter()
            exp = numpy_baseline(text, con.consensus, con.von, a.columns)
            base_s = time.perf_counter() - t
        for name in FIELDS:
            if not (np.array_equal(getattr(full, name), exp[name]) and np.array_equal(getattr(a, name), exp[name])):
                raise SystemExit(f"{name} of the device and of the numpy restatement differ")
        if not np.array_equal(full.mismatches, exp["mismatches"]):
            raise SystemExit("the mismatch matrices of the device and of the numpy restatement differ")
    med = {k: statistics.median(t[k] for t in timing) for k in timing[0]}
    return {"compared_columns": C, "words": words, "rows_per_range": min(T, (64 << 20) // (32 * words + 4 * P)),
            "timing_ms": timing, "median_ms": {k: round(v, 3) for k, v in med.items()}, "wall_ms_with_python": spread(wall),
            "timing_ms_with_matrix_downloaded": with_matrix,
            "planes_text_bytes": T * C, "planes_text_bytes_per_s": T * C / (med["planes_ms"] * 1e-3),
            "planes_share_of_hbm_rate_counting_one_byte_per_column": T * C / (med["planes_ms"] * 1e-3) / HBM_BYTES_PER_S,
            "dist_ops64": T * P * words * 8, "dist_ops64_per_s": T * P * words * 8 / (med["dist_best_ms"] * 1e-3),
            "numpy_one_core_s": None if base_s is None else round(base_s, 2), "numpy_blas_threads": threads,
            "equal_to_numpy": None if base_s is None else True,
            "rows_with_nothing_compared": int((a.compared == 0).sum()), "best_is_own_copy": None}, a


def threshold_table(rs, msa, text, truth, mc, cutoff, grid_compared, grid_margin):
    import numpy as np
    W = text.shape[1]
    von = W // 2
    bis = von + W // 6
    spans = (text[:, von] != ord(" ")) & (text[:, bis] != ord(" "))
    labels = np.where(spans, truth, -1).astype(np.int32)
    con = rs.consensus(msa, labels, von, bis, mc, cutoff)
    a = rs.assign(msa, con)
    index = {int(x): i for i, x in enumerate(con.part_label)}
    own = np.array([index.get(int(x), -2) for x in truth])
    inside = labels >= 0
    cells = []
    for c in grid_compared:
        for m in grid_margin:
            lab = a.labels(c, m, keep=labels)
            new = ~inside & (lab >= 0)
            cells.append({"min_compared": c, "min_margin": m, "recruited": int(new.sum()),
                          "recruits_in_their_true_copy": None if not new.any() else round(float((lab[new] == truth[new]).mean()), 4)})
    return {"window": [von, bis], "selected_columns": int(len(con.selected)), "compared_columns": int(len(a.columns)), "parts": con.parts,
            "rows_labelled": int(inside.sum()), "rows_unlabelled_with_something_compared": int((~inside & (a.compared > 0)).sum()),
            "labelled_rows_whose_best_is_their_own_copy": round(float((a.best[inside] == own[inside]).mean()), 4),
            "median_compared_of_the_unlabelled": int(np.median(a.compared[~inside & (a.compared > 0)])) if (~inside & (a.compared > 0)).any() else 0,
            "cells": cells}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tree_default")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--no-baseline", action="store_true", help="skip the numpy restatement (and with it the comparison)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_bench.json"))
    a = ap.parse_args()
    import numpy as np
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
    lib = _lib.load()
    cutoff = float(lib.pgr_default_cutoff(ctypes.c_double(0.0), W))
    prep_s = time.time() - t0
    colmax = mc.reshape(-1, 5).max(axis=1)
    print(f"prepared in {prep_s:.0f} s: {T} x {W}, {len(set(truth.tolist()))} copies, cutoff {cutoff:.3f}, {int((colmax > cutoff).sum())} columns "
          f"over it, largest MaxCorrs {float(np.nanmax(mc)):.3f}, {int(np.isnan(mc).sum())} NaN", file=sys.stderr, flush=True)
    if not (colmax > cutoff).any():
        raise SystemExit("no column is selected: nothing to measure")
    out = {"metric": "pgr_msa_assign at the benchmark's size", "unit": "ms per call, median of the repetitions",
           "workload": f"{a.workload}: datagen's MSA of the true alignments, {T} rows x {W} columns, the true copies as the labelling, whole width",
           "reps": a.reps, "cutoff": cutoff, "prepare_s": round(prep_s, 1)}
    with rs.open_msa(text) as msa:
        con = rs.consensus(msa, truth, maxcorrs=mc, cutoff=cutoff)
        index = {int(x): i for i, x in enumerate(con.part_label)}
        own = np.array([index[int(x)] for x in truth])
        out["parts"], out["selected_columns"] = con.parts, int(len(con.selected))
        for name, every in (("selected", False), ("all_columns", True)):
            out[name], got = measure(rs, msa, con, text, a.reps, every, not a.no_baseline)
            out[name]["best_is_own_copy"] = round(float((got.best == own).mean()), 4)
        out["value"] = out["all_columns"]["median_ms"]["all_ms"]
        out["thresholds"] = threshold_table(rs, msa, text, truth, mc, cutoff, (10, 30, 100, 300), (1, 2, 4, 8, 16))
    th = out["thresholds"]
    print(f"threshold table, window {th['window']}: {th['rows_labelled']} rows labelled, {th['labelled_rows_whose_best_is_their_own_copy']:.4f} "
          f"of them nearest to their own copy; {th['rows_unlabelled_with_something_compared']} unlabelled rows touch it", file=sys.stderr)
    for c in th["cells"]:
        print(f"  min_compared {c['min_compared']:4d}  min_margin {c['min_margin']:3d}  recruited {c['recruited']:6d}  in their true copy "
              f"{c['recruits_in_their_true_copy']}", file=sys.stderr)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("selected", "all_columns", "thresholds")} |
                     {n: out[n]["median_ms"] for n in ("selected", "all_columns")}))


if __name__ == "__main__":
    main()
