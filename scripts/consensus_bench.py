#!/usr/bin/env python3
"""Measurement of the per-copy consensus on the device-resident MSA (include/pgr.h, pgr_msa_consensus) at the size of the
benchmark: one JSON line.
    python3 scripts/consensus_bench.py [--workload tree_default] [--reps 5] [--no-baseline]
Input: the MSA datagen stacks from the true alignments of the workload's reads (datagen.simulate + build_msa: the shape of the
benchmark's MSA, no aligner run needed) with the reads' true copy ids as labels, the whole width as the window, every column
selected.  Reported: the fields of pgr_last_consensus_timing of every repetition; the bytes of the text the counts kernel reads
(labelled rows x width, every byte once) per second of its time, against the 8 TB/s of the HBM; and the time of the numpy
restatement of the same counts on one core (a code table lookup, then per part and symbol one comparison and one column sum) --
the baseline, never the code under test.  Before any time is reported the counts, consensus and depth of one call are compared
with that restatement (the script fails if they differ)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def spread(v):
    return {"all": [round(x, 3) for x in v], "min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def numpy_counts(text, labels):
    """counts[parts][width][5] as TransposonAssessment.py's Konsensus counts them, in numpy"""
    import numpy as np
    lut = np.full(256, 5, dtype=np.uint8)
    for chars, k in ((b"aA", 0), (b"cC", 1), (b"gG", 2), (b"tT", 3), (b"-_", 4)):
        for ch in chars:
            lut[ch] = k
    found = [x for x in range(int(labels.max()) + 1) if (labels == x).any()]
    counts = np.empty((len(found), text.shape[1], 5), dtype=np.int32)
    for p, x in enumerate(found):
        codes = lut[text[labels == x]]
        for k in range(5):
            counts[p, :, k] = (codes == k).sum(axis=0, dtype=np.int32)
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tree_default")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true", help="skip the numpy restatement (and with it the comparison)")
    a = ap.parse_args()
    import numpy as np
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd import resolution as rs
    t0 = time.time()
    data = dg.simulate(dg.CONFIGS[a.workload])
    text = np.ascontiguousarray(dg.build_msa(data))
    labels = np.array(data.copy_of, dtype=np.int32)
    T, W = text.shape
    prep_s = time.time() - t0
    print(f"prepared in {prep_s:.0f} s: {T} x {W}, {len(set(labels.tolist()))} copies", file=sys.stderr, flush=True)
    timing, wall = [], []
    with rs.open_msa(text) as msa:
        for rep in range(a.reps):
            t = time.perf_counter()
            con = rs.consensus(msa, labels)
            wall.append((time.perf_counter() - t) * 1e3)
            timing.append({k: round(v, 3) for k, v in rs.last_consensus_timing().items()})
            print(f"rep {rep}: {timing[-1]}", file=sys.stderr, flush=True)
        full = rs.consensus(msa, labels, counts=True)
        with_counts = {k: round(v, 3) for k, v in rs.last_consensus_timing().items()}
    baseline_s = None
    if not a.no_baseline:
        t = time.perf_counter()
        exp = numpy_counts(text, labels)
        baseline_s = time.perf_counter() - t
        if not (np.array_equal(full.counts, exp) and np.array_equal(full.depth, exp.sum(axis=2)) and
                np.array_equal(full.consensus, exp.argmax(axis=2)) and np.array_equal(con.consensus, full.consensus)):
            raise SystemExit("the counts of the device and of the numpy restatement differ")
    counts_ms = [t["counts_ms"] for t in timing]
    read = int((labels >= 0).sum()) * W
    rate = read / (statistics.median(counts_ms) * 1e-3)
    off = con.diff_all[~np.eye(con.parts, dtype=bool)]
    out = {"metric": "counts kernel of pgr_msa_consensus, share of the HBM rate", "value": rate / HBM_BYTES_PER_S,
           "unit": "bytes of the text read per second of k_cs_counts / 8 TB/s",
           "workload": f"{a.workload}: datagen's MSA of the true alignments, {T} rows x {W} columns, {con.parts} true copies of "
                       f"{int(con.part_rows.min())} to {int(con.part_rows.max())} rows, whole width",
           "reps": a.reps, "bytes_read": read, "counts_bytes_per_s": rate, "timing_ms": timing, "counts_ms": spread(counts_ms),
           "all_ms": spread([t["all_ms"] for t in timing]), "wall_ms_with_python": spread(wall), "timing_ms_with_counts_downloaded": with_counts,
           "numpy_one_core_s": None if baseline_s is None else round(baseline_s, 2), "equal_to_numpy": None if baseline_s is None else True,
           "smallest_diff_all": int(off.min()), "unique": rs.unique_parts(con.diff_all)[0], "prepare_s": round(prep_s, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
