#!/usr/bin/env python3
"""Measurement of the HIP ReadCutter on the benchmark data set's full reads: one JSON line.

    python3 scripts/rc_bench.py [--workload tree_default] [--repeats K] [--parts 60]

The reads are the simulated data set's *full* reads (datagen.write_dataset: flanks included), the template is the repeat.
`value` = DP cells of the reference (piece length x read length for each of the two pieces Occurrence maps, RC:600) per
second of kernel time (device events); `wall_s` = the drop-in binary end to end on the files (read, GPU, write), against
the reference's recorded wall time in tests/golden/rc_tree_default.json.

    python3 scripts/rc_bench.py --both-strands [--strand-seed S] [--repeats K]

measures prc_cut_strands on the same reads with a seeded half turned against prc_cut on the unturned reads, in one process,
the two calls interleaved, medians over K repeats.  Before any timing the turned run's cut points are compared with those of
the unturned reads, read by read."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def both_strands(a, g, reads, templ, gen_s):
    import statistics
    from repeatresolver_amd.strands import seeded_mask, turn
    mask = seeded_mask(len(reads), a.strand_seed)
    mixed = turn(reads, mask)
    plain = g.cut(reads, a.parts)                          # every call once: the warm-up, and the comparison
    own, nf0, nr0 = g.cut(reads, a.parts, both_strands=True)
    got, nf1, nr1 = g.cut(mixed, a.parts, both_strands=True)
    for j, r in enumerate(reads):                          # a turned read is cut where its mirror image is, and counts swap
        exp = [len(r) - int(c) for c in own[j][::-1]] if mask[j] else [int(c) for c in own[j]]
        assert [int(c) for c in got[j]] == exp, j
        assert (int(nf1[j]), int(nr1[j])) == ((int(nr0[j]), int(nf0[j])) if mask[j] else (int(nf0[j]), int(nr0[j]))), j
    cut_on_reverse = [j for j in range(len(reads)) if int(nr0[j])]
    for j in range(len(reads)):
        if not int(nr0[j]):
            assert [int(c) for c in own[j]] == [int(c) for c in plain[j]], j
    fwd, both = {"kernel": [], "wall": []}, {"kernel": [], "wall": []}
    for _ in range(max(a.repeats, 5)):                     # interleaved: forward, both, forward, both ...
        for kw, arg, acc in (({}, reads, fwd), ({"both_strands": True}, mixed, both)):
            k0 = g.stats()["kernel_ms"]
            t0 = time.time()
            g.cut(arg, a.parts, **kw)
            acc["wall"].append((time.time() - t0) * 1e3)
            acc["kernel"].append(g.stats()["kernel_ms"] - k0)
    med = lambda acc: {k: round(statistics.median(v), 2) for k, v in acc.items()}
    mf, mb = med(fwd), med(both)
    return {"metric": "ReadCutter, both strands against forward only", "unit": "ms (medians)", "workload": a.workload,
            "reads": len(reads), "bases": sum(len(r) for r in reads), "template": len(templ), "parts": a.parts,
            "turned": sum(mask), "strand_seed": a.strand_seed, "repeats": max(a.repeats, 5),
            "compared": {"reads": len(reads), "reads_also_cut_on_their_reverse_strand": len(cut_on_reverse),
                         "cut_points_forward_only": int(sum(len(c) for c in plain)), "cut_points_both": int(sum(len(c) for c in own))},
            "prc_cut_ms": mf, "prc_cut_strands_ms": mb, "ratio": {k: round(mb[k] / mf[k], 3) for k in mf},
            "spread_ms": {"prc_cut_kernel": [round(min(fwd["kernel"]), 2), round(max(fwd["kernel"]), 2)],
                          "prc_cut_strands_kernel": [round(min(both["kernel"]), 2), round(max(both["kernel"]), 2)]},
            "generate_s": round(gen_s, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="tree_default")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parts", type=int, default=60)
    ap.add_argument("--both-strands", action="store_true", help="prc_cut_strands on the reads with a seeded half turned, against prc_cut")
    ap.add_argument("--strand-seed", type=int, default=1)
    a = ap.parse_args()
    from repeatresolver_amd import datagen as dg
    from repeatresolver_amd.read_cutter import CLI_PATH, ReadCutter
    td = tempfile.mkdtemp(prefix="rc_bench_")
    try:
        t0 = time.time()
        _, full, _, _, _, _ = dg.simulate_dataset(dg.CONFIGS[a.workload])
        dg.write_dataset(os.path.join(td, "ds"), dg.CONFIGS[a.workload])
        os.replace(os.path.join(td, "ds_Template.fasta"), os.path.join(td, "dsTemplate.fasta"))
        gen_s = time.time() - t0
        templ = b"".join(l for l in open(os.path.join(td, "dsTemplate.fasta"), "rb").read().split(b"\n") if not l.startswith(b">"))
        reads = [dg.ASCII[r].tobytes() for r in full]
        g = ReadCutter(templ)
        if a.both_strands:
            print(json.dumps(both_strands(a, g, reads, templ, gen_s)))
            g.close()
            return
        kms, walls = [], []
        for _ in range(a.repeats + 1):                     # the first call is the warm-up
            s0 = g.stats()
            t1 = time.time()
            g.cut(reads, a.parts)
            walls.append(time.time() - t1)
            s1 = g.stats()
            kms.append(s1["kernel_ms"] - s0["kernel_ms"])
        cells = s1["cells"] - s0["cells"]
        g.close()
        km = min(kms[1:])
        e2e = []
        for _ in range(max(a.repeats, 1)):
            t1 = time.time()
            p = subprocess.run([CLI_PATH, "dsTemplate.fasta", "ds.fasta", "-p", str(a.parts)], cwd=td, capture_output=True)
            e2e.append(time.time() - t1)
            assert p.returncode == 0, p.stdout[-400:]
        out = {"metric": "ReadCutter DP cells/sec (kernel)", "value": cells / (km * 1e-3), "unit": "cells/s", "workload": a.workload,
               "reads": len(reads), "bases": sum(len(r) for r in reads), "template": len(templ), "parts": a.parts,
               "cells": cells, "kernel_ms": round(km, 2), "prc_cut_wall_s": round(min(walls[1:]), 3),
               "wall_s": round(min(e2e), 2), "generate_s": round(gen_s, 1)}
        ref = os.path.join(ROOT, "tests", "golden", "rc_tree_default.json")
        if a.workload == "tree_default" and a.parts == 60 and os.path.exists(ref):
            fx = json.load(open(ref))
            out["reference_wall_s"] = fx["reference_wall_s"]
            out["reference_host"] = fx["reference_host"]
            out["speedup_wall"] = round(fx["reference_wall_s"] / min(e2e), 1)
        print(json.dumps(out))
    finally:
        shutil.rmtree(td, ignore_errors=True)


if __name__ == "__main__":
    main()
