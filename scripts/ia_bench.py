#!/usr/bin/env python3
"""Measurement of the HIP InitialAligner on the benchmark data set's reads: one JSON line.

    python3 scripts/ia_bench.py [--workload tree_default] [--reads N] [--repeats K] [--cpu-reads M]

The reads are the simulated data set's reads cut to their repeat part (what ReadCutter hands to InitialAligner), the
template is the repeat.  `value` = matrix cells of the reference (read length x template length per read, IA:300-328) per
second of pia_align wall time with reads on the host; `fill` = the same over the two kernel passes alone.  The CPU
baseline is the oracle's IntoAligner restatement on a few of the same reads (one core).

    python3 scripts/ia_bench.py --both-strands [--strand-seed S] [--repeats K]

measures pia_align_strands on the same reads with a seeded half turned against pia_align on the unturned reads, in one
process, the two calls interleaved, medians over K repeats of pia_get_timing's buckets.  Before any timing the turned run's
strands, distances and placements are compared with the forward run's, field for field."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def both_strands(a, g, reads, templ, bases, gen_s):
    import statistics
    from repeatresolver_amd.strands import seeded_mask, turn
    mask = seeded_mask(len(reads), a.strand_seed)
    mixed = turn(reads, mask)
    place0, dist0 = g.align(reads)                       # both calls once: the warm-up, and the comparison
    place1, dist1, strand1, other1 = g.align_strands(mixed)
    taken_back = [j for j in range(len(reads)) if int(strand1[j]) == mask[j]]
    for j in taken_back:                                 # the read in its original orientation: every field as pia_align gives it
        assert int(dist1[j]) == int(dist0[j]) and (place1[j] == place0[j]).all(), j
    rest = [j for j in range(len(reads)) if int(strand1[j]) != mask[j]]
    for j in rest:                                       # kept the other way round: only where that is at least as near
        assert int(dist1[j]) <= int(dist0[j]) and int(other1[j]) == int(dist0[j]), j
    keys = ("total", "upload", "pass1", "pass2_and_traceback", "download")
    fwd, both = {k: [] for k in keys + ("wall",)}, {k: [] for k in keys + ("wall",)}
    for _ in range(max(a.repeats, 5)):                   # interleaved: forward, both, forward, both ...
        for fn, arg, acc in ((g.align, reads, fwd), (g.align_strands, mixed, both)):
            t0 = time.time()
            fn(arg)
            acc["wall"].append((time.time() - t0) * 1e3)
            t = g.stats()["last_align_ms"]
            for k in keys:
                acc[k].append(t[k])
    med = lambda acc: {k: round(statistics.median(v), 2) for k, v in acc.items()}
    mf, mb = med(fwd), med(both)
    cells = bases * len(templ)
    return {"metric": "InitialAligner, both strands against forward only", "unit": "ms (medians)", "workload": a.workload,
            "reads": len(reads), "bases": bases, "template": len(templ), "turned": sum(mask), "strand_seed": a.strand_seed,
            "repeats": max(a.repeats, 5), "cells_forward": cells, "cells_both_pass1": 2 * cells,
            "compared": {"reads_equal_field_for_field": len(taken_back), "reads_kept_the_other_way_round": len(rest),
                         "longest_of_those": max((len(reads[j]) for j in rest), default=0),
                         "largest_distance_gain_of_those": max((int(dist0[j]) - int(dist1[j]) for j in rest), default=0)},
            "pia_align_ms": mf, "pia_align_strands_ms": mb,
            "ratio": {k: round(mb[k] / mf[k], 3) for k in mf if mf[k] > 0},
            "spread_ms": {"pia_align_pass1": [round(min(fwd["pass1"]), 2), round(max(fwd["pass1"]), 2)],
                          "pia_align_strands_pass1": [round(min(both["pass1"]), 2), round(max(both["pass1"]), 2)],
                          "pia_align_total": [round(min(fwd["total"]), 2), round(max(fwd["total"]), 2)],
                          "pia_align_strands_total": [round(min(both["total"]), 2), round(max(both["total"]), 2)]},
            "generate_s": round(gen_s, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tree_default")
    ap.add_argument("--reads", type=int, default=0, help="use only the first N reads (0 = all)")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cpu-reads", type=int, default=3)
    ap.add_argument("--mem-budget-gb", type=float, default=0, help="bytes of direction bits per batch of pass 2 (0 = the library's default)")
    ap.add_argument("--both-strands", action="store_true", help="pia_align_strands on the reads with a seeded half turned, against pia_align")
    ap.add_argument("--strand-seed", type=int, default=1)
    a = ap.parse_args()
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd.initial_aligner import InitialAligner
    t0 = time.time()
    cfg = dg.CONFIGS[a.workload]
    seq, _full, _starts, _cids, cut, _ = dg.simulate_dataset(cfg)
    templ = dg.ASCII[seq].tobytes()
    reads = [dg.ASCII[r].tobytes() for r in cut if r is not None and len(r) > 0]
    if a.reads:
        reads = reads[:a.reads]
    gen_s = time.time() - t0
    bases = sum(len(r) for r in reads)
    g = InitialAligner(templ)
    if a.mem_budget_gb:
        g.set_option("mem_budget", int(a.mem_budget_gb * 2**30))
    if a.both_strands:
        print(json.dumps(both_strands(a, g, reads, templ, bases, gen_s)))
        g.close()
        return
    walls = []
    for _ in range(a.repeats + 1):                       # the first call is the warm-up
        s0 = g.stats()
        t0 = time.time()
        place, dist = g.align(reads)
        walls.append(time.time() - t0)
        s1 = g.stats()
    cells = s1["cells"] - s0["cells"]
    fill_ms = s1["fill_ms"] - s0["fill_ms"]
    wall = min(walls[1:])
    out = {"metric": "InitialAligner matrix cells/sec", "value": cells / wall, "unit": "cells/s", "workload": a.workload,
           "reads": len(reads), "bases": bases, "template": len(templ), "cells": cells, "wall_s": wall, "fill_ms": fill_ms,
           "fill_cells_per_s": cells / (fill_ms * 1e-3), "mean_error": float((dist / [max(len(r), 1) for r in reads]).mean()),
           "generate_s": round(gen_s, 1), "last_align_ms": {k: round(v, 1) for k, v in s1["last_align_ms"].items()}}
    if a.cpu_reads:
        lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libiaoracle.so"))
        lib.iao_align.restype = ctypes.c_long
        lib.iao_align.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
        step = max(1, len(reads) // a.cpu_reads)
        sample = list(range(0, len(reads), step))[:a.cpu_reads]
        ccells, t0 = 0, time.time()
        for j in sample:
            r = reads[j]
            al = (ctypes.c_int * len(r))()
            codes = ctypes.create_string_buffer(len(r) * len(templ))
            d = lib.iao_align(r, len(r), templ, len(templ), al, None, codes)
            assert d == int(dist[j]) and list(al) == list(place[j]), j
            ccells += len(r) * len(templ)
        cs = time.time() - t0
        out["cpu_baseline"] = {"value": ccells / cs, "unit": "cells/s", "cores": 1, "kind": "port",
                               "sample": f"{len(sample)} reads of the same set, {ccells} cells, {cs:.1f} s; results equal to the GPU's"}
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
