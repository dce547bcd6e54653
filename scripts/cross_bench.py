#!/usr/bin/env python3
"""Measurement of the segment-wise assignment and the crossovers (include/pgr.h, pgr_msa_crossovers) at the size of the benchmark,
and the table that guides the choice of Crossovers.rows' min_gain: one JSON document.
    python3 scripts/cross_bench.py [--workload tree_default] [--reps 3] [--out profiles/cross_bench.json]
Input: as scripts/assign_bench.py -- datagen's MSA of the true alignments with trimmed ends, the reads' true copy ids as the
labelling, its consensus over the whole width, the columns over RepeatResolver's default cutoff at which every copy has depth --
in 6 and in 64 segments of equally many compared columns.  After a warm-up call, the best of `reps`: the call's time with
Python around it and the buckets of pgr_last_crossover_timing, with the matrix downloaded and without.  The yardstick is the only
way to the same matrix without this entry: one assign_sequences(..., matrix=True) per segment, timed in the same process; before
any time is reported its matrices are compared with seg_mismatches, segment by segment, and the one-copy fields with those of one
assign over all columns (the script fails if they differ).  The numpy restatement (tests/cx_checker.numpy_crossovers, by the
definition: all (k, a, b)) runs on one core (threadpoolctl holds the BLAS to one thread) on a SAMPLE of the rows, is compared
field by field with the device on them, and its time is EXTRAPOLATED to all rows by the ratio of the row counts: the file says so.

The min_gain table: 1 % of the rows are spliced -- the row's own symbols left of a random compared column at which it has one,
and right of it those of a row of another copy that has a symbol there too --, the consensus stays that of the true copies, and
for min_side fixed and min_gain over a range: the spliced rows among Crossovers.rows(min_gain), those of them whose pair of copies
is the true one, and the unspliced rows flagged, at 6 and at 64 segments."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
SEGMENTS = (6, 64)


def best_of(reps, call, timing):
    """(the smallest wall time in ms, the timing buckets of that call, the last result)"""
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        got = call()
        ms = (time.perf_counter() - t) * 1e3
        if best is None or ms < best[0]:
            best = (ms, {k: round(v, 3) for k, v in timing().items()})
    return round(best[0], 3), best[1], got


def measure(rs, msa, con, text, nseg, min_side, reps, sample):
    import numpy as np
    import cx_checker as cx
    from assign_bench import one_thread
    first = rs.crossovers(msa, con, segments=nseg, min_side=min_side, matrix=True)      # warm-up; the columns and the segments' ends
    # both sides are handed the columns ready-made, as assign_sequences is below
    call = lambda matrix: rs.crossover_sequences(msa, con.von, con.consensus, first.columns, first.seg_end, min_side=min_side,
                                                 part_label=con.part_label, matrix=matrix)
    wall_m, timing_m, full = best_of(reps, lambda: call(True), rs.last_crossover_timing)
    wall, timing, got = best_of(reps, lambda: call(False), rs.last_crossover_timing)
    segs = full.segment_columns

    def per_segment():
        return [rs.assign_sequences(msa, con.von, con.consensus, cols, matrix=True) for cols in segs]
    per_segment()                                                      # warm-up
    kernels, inside = [], []

    def timed():
        out, k, lib_ms = [], 0.0, 0.0
        for cols in segs:
            out.append(rs.assign_sequences(msa, con.von, con.consensus, cols, matrix=True))
            t = rs.last_assign_timing()
            k += t["planes_ms"] + t["dist_best_ms"]
            lib_ms += t["all_ms"]
        kernels.append(k)
        inside.append(lib_ms)
        return out
    yard_wall, _, parts = best_of(reps, timed, lambda: {})
    for s, a in enumerate(parts):
        if not (np.array_equal(full.seg_mismatches[:, s, :], a.mismatches) and np.array_equal(full.seg_compared[:, s], a.compared)):
            raise SystemExit(f"segment {s}: the matrix of the single call and of assign_sequences differ")
    whole = rs.assign_sequences(msa, con.von, con.consensus, full.columns)
    for name in ("compared", "best", "second", "best_mismatches", "second_mismatches"):
        if not (np.array_equal(getattr(full, name), getattr(whole, name)) and np.array_equal(getattr(got, name), getattr(whole, name))):
            raise SystemExit(f"{name} of the crossovers and of the assignment differ")
    rows = np.sort(np.random.default_rng(1).choice(text.shape[0], size=min(sample, text.shape[0]), replace=False))
    limit, threads = one_thread()
    with limit:
        t = time.perf_counter()
        exp = cx.numpy_crossovers(text, con.consensus, con.von, full.columns, full.seg_end.tolist(), min_side, rows=rows)
        base_s = time.perf_counter() - t
    cx.same(full, exp, rows=rows)
    T, P = text.shape[0], con.parts
    words = int(sum((len(c) + 63) // 64 for c in segs))
    kernel_ms = timing_m["planes_ms"] + timing_m["dist_ms"] + timing_m["cross_best_ms"]
    numpy_all = base_s * T / len(rows)
    return {"segments": nseg, "compared_columns": int(len(full.columns)), "words_after_padding": words, "min_side": min_side,
            "rows_per_range": int(min(T, (64 << 20) // (32 * words + 4 * nseg * P + 8 * nseg + 40))),
            "with_matrix": {"wall_ms_with_python_best": wall_m, "timing_ms": timing_m},
            "without_matrix": {"wall_ms_with_python_best": wall, "timing_ms": timing},
            "kernels_ms": round(kernel_ms, 3),
            "yardstick_one_assign_per_segment": {"calls": nseg, "wall_ms_with_python_best": yard_wall, "inside_the_library_ms_best": round(min(inside), 3),
                                                 "kernels_ms_best": round(min(kernels), 3)},
            "ratio_yardstick_over_single_call_wall": round(yard_wall / wall_m, 2),
            "ratio_yardstick_over_single_call_inside_the_library": round(min(inside) / timing_m["all_ms"], 2),
            "ratio_yardstick_over_single_call_kernels": round(min(kernels) / kernel_ms, 2),
            "ratio_yardstick_kernels_over_planes_and_distances_alone": round(min(kernels) / (timing_m["planes_ms"] + timing_m["dist_ms"]), 2),
            "numpy_one_core": {"blas_threads": threads, "sampled_rows": int(len(rows)), "sample_s": round(base_s, 2),
                               "extrapolated_to_all_rows_s": round(numpy_all, 1), "note": "measured on the sample, extrapolated by rows / sampled rows",
                               "equal_to_the_device_on_the_sample": True},
            "ratio_numpy_extrapolated_over_single_call_wall": round(numpy_all * 1e3 / wall_m, 1),
            "rows_with_a_crossover": int((got.cross_split >= 0).sum())}


def splice(text, truth, columns, share, seed):
    """(the spliced copy of text, the spliced rows, the copy right of each splice, the splice columns)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = text.copy()
    rows, partner_copy, at = [], [], []
    blank = ord(" ")
    for r in rng.permutation(len(text))[:max(1, int(len(text) * share))]:
        has = columns[text[r, columns] != blank]
        if len(has) < 2:
            continue
        for _ in range(50):
            c, q = int(has[rng.integers(1, len(has))]), int(rng.integers(0, len(text)))
            if truth[q] != truth[r] and text[q, c] != blank:
                out[r, c:] = text[q, c:]
                rows.append(int(r)); partner_copy.append(int(truth[q])); at.append(c)
                break
    return out, np.array(rows), np.array(partner_copy), np.array(at)


def gain_table(rs, text, truth, con, min_side, gains, share, device_rows):
    import numpy as np
    columns = np.asarray(con.selected)[(con.depth[:, np.asarray(con.selected) - con.von] >= 1).all(axis=0)]
    spliced_text, rows, partner, at = splice(text, truth, columns, share, 2)
    index = {int(x): i for i, x in enumerate(con.part_label)}
    is_spliced = np.zeros(len(text), bool)
    is_spliced[rows] = True
    left_true, right_true = np.full(len(text), -1), np.full(len(text), -1)
    left_true[rows] = [index[int(truth[r])] for r in rows]
    right_true[rows] = [index[int(p)] for p in partner]
    out = {"spliced_rows": int(len(rows)), "unspliced_rows": int(len(text) - len(rows)), "min_side": min_side, "tables": []}
    with rs.open_msa(spliced_text) as msa:
        for nseg in SEGMENTS:
            x = rs.crossovers(msa, con, segments=nseg, min_side=min_side)
            cells = []
            for g in gains:
                flagged = np.zeros(len(text), bool)
                flagged[x.rows(g)] = True
                pair = flagged & is_spliced & (x.cross_left == left_true) & (x.cross_right == right_true)
                cells.append({"min_gain": g, "spliced_found": int((flagged & is_spliced).sum()), "of_them_with_the_true_pair_of_copies": int(pair.sum()),
                              "unspliced_flagged": int((flagged & ~is_spliced).sum())})
            out["tables"].append({"segments": nseg, "cells": cells})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tree_default")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--min-side", type=int, default=50)
    ap.add_argument("--sample", type=int, default=256, help="rows of the numpy restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_bench.json"))
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
    prep_s = time.time() - t0
    print(f"prepared in {prep_s:.0f} s: {T} x {W}, {len(set(truth.tolist()))} copies, cutoff {cutoff:.3f}", file=sys.stderr, flush=True)
    out = {"metric": "pgr_msa_crossovers at the benchmark's size", "unit": "ms per call, best of the repetitions after a warm-up",
           "workload": f"{a.workload}: datagen's MSA of the true alignments, {T} rows x {W} columns, the true copies as the labelling, whole width",
           "reps": a.reps, "cutoff": cutoff, "prepare_s": round(prep_s, 1), "runs": []}
    with rs.open_msa(text) as msa:
        con = rs.consensus(msa, truth, maxcorrs=mc, cutoff=cutoff)
        out["parts"], out["selected_columns"] = con.parts, int(len(con.selected))
        for nseg in SEGMENTS:
            out["runs"].append(measure(rs, msa, con, text, nseg, a.min_side, a.reps, a.sample))
            print(json.dumps(out["runs"][-1]), file=sys.stderr, flush=True)
    out["value"] = out["runs"][-1]["with_matrix"]["wall_ms_with_python_best"]
    out["min_gain"] = gain_table(rs, text, truth, con, a.min_side, (1, 2, 4, 8, 16, 32, 64, 128), 0.01, T)
    for tab in out["min_gain"]["tables"]:
        for c in tab["cells"]:
            print(f"  segments {tab['segments']:3d}  min_gain {c['min_gain']:4d}  spliced found {c['spliced_found']:4d} of {out['min_gain']['spliced_rows']}"
                  f"  (true pair {c['of_them_with_the_true_pair_of_copies']:4d})  unspliced flagged {c['unspliced_flagged']:6d}", file=sys.stderr)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("runs", "min_gain")} |
                     {f"segments_{r['segments']}": {"single_call_ms": r["with_matrix"]["wall_ms_with_python_best"],
                                                    "yardstick_ms": r["yardstick_one_assign_per_segment"]["wall_ms_with_python_best"]} for r in out["runs"]}))


if __name__ == "__main__":
    main()
