#!/usr/bin/env python3
"""TEST INFRASTRUCTURE.  Generates tests/golden/rr_kmeans_reference.json.gz: the KmeansSubdivisionOf_ file the *compiled
reference* RepeatResolver (oracle/_ref/repeat_resolver, the unmodified program text linked with oracle/gsl_standin.c, built by
`make -C oracle ref`) writes for every label case of tests/golden/rr_reference.json.gz and for the new inputs of
tests/km_cases.py.  Only data is committed: per case the name, the sha256 of the input, the arguments, the file's name and
its text verbatim; for a new case also the MaxCorrsOf_ non-zero lines and the two earlier label files, as rr_reference.json.gz
holds them for the others.  Runs only where the reference exists.

    python scripts/gen_km_fixtures.py          # rewrites the fixture, byte for byte reproducible
    python scripts/gen_km_fixtures.py --deep   # after oracle/gen_rr_fixtures.py --deep: adds the KmeansSubdivisionOf_ file to every
                                               # record of tests/golden/rr_deep_reference.json.gz (tests/deep_cases.py)

The existing cases are fed their recorded MaxCorrsOf_ lines (rr_cases.maxcorrs_lines); for the new ones the reference's
own MaxCorrelation writes the file first.  The condition for an exact comparison is asserted per case: the label conditions of
rr_cases.label_conditions, and in every eligible part no evaluated pair's Z by tests/km_checker.py within 1e-8 of the
cutoff.  A new case that fails gets another seed; an existing input that fails is recorded under "vars_only" (at most 2)."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gr_checker as gc  # noqa: E402
import km_cases as kc  # noqa: E402
import km_checker as km  # noqa: E402
import rr_cases as rc  # noqa: E402
import sd_checker as sd  # noqa: E402

MC = os.path.join(ROOT, "oracle", "_ref", "max_correlation")
RR = os.path.join(ROOT, "oracle", "_ref", "repeat_resolver")
MARGIN = 1e-8


def run_reference(name, case=None, old=None):
    """case / old: an input and its record of the first stages from elsewhere than km_cases / rr_reference.json.gz"""
    case = case or kc.case_input(name)
    rows, new = case["rows"], name in kc.NEW_BUILDERS
    args = kc.rr_args(case)
    rec = {"name": name, "input_sha256": rc.input_sha256(rows), "args": args, "rows": len(rows), "width": len(rows[0]),
           "cov": case["cov"], "von": case["von"], "bis": case["bis"]}
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, rc.MSA_NAME), "wb") as f:
            f.write(rc.msa_bytes(rows))
        mc_path = os.path.join(td, "MaxCorrsOf_" + rc.MSA_NAME)
        if new:
            subprocess.run([MC, rc.MSA_NAME, "-c", str(case["cov"]), "-p", "1"], cwd=td, capture_output=True, check=True, timeout=600)
            lines = open(mc_path).read().split("\n")[:-1]
            assert len(lines) == len(rows[0]) * 5
            rec["maxcorrs"] = {"lines": len(lines), "nonzero": [[i, l] for i, l in enumerate(lines) if l != "0.000000"]}
        else:
            with open(mc_path, "w") as f:
                f.write("".join(l + "\n" for l in rc.maxcorrs_lines(old or rc.load_fixture()[name])))
        subprocess.run([RR] + args, cwd=td, capture_output=True, check=True, timeout=600)
        names = sorted(n for n in os.listdir(td) if "SubdivisionOf_" in n)
        assert len(names) == 3 and names[1].startswith("Kmeans"), names
        text = {n: open(os.path.join(td, n)).read() for n in names}
    rec["kmeans"] = {"file": names[1], "text": text[names[1]]}
    if new:
        rec["dropoff"] = {"file": names[0], "text": text[names[0]]}
        rec["reldrop"] = {"file": names[2], "text": text[names[2]]}
    else:
        old = old or rc.load_fixture()[name]
        assert text[names[0]] == old["dropoff"]["text"] and text[names[2]] == old["reldrop"]["text"], name
    return rec, case


def condition(rec, first, case):
    """(margin of the checker's pair values from the cutoff, the checker's result)"""
    win = gc.Window(case["rows"], rc.maxcorrs_values(first), case["von"], case["bis"], case["cov"])
    ref = win.refine()
    rc.label_conditions(case, dict(first, name=rec["name"]), (win, ref))
    got = km.clustered(win, ref, sd.subdivide(win, ref, case["cov"])["reldrop_labels"], case["cov"])
    return km.margin(got["eligible"], win.cutoff), got


def main_deep():
    """the third label file of every record oracle/gen_rr_fixtures.py --deep wrote, fed that record's MaxCorrsOf_ lines"""
    import deep_cases as dc
    with gzip.open(dc.FIXTURE, "rb") as f:
        fixture = json.load(f)
    for first in fixture["cases"]:
        name = first["name"]
        rec, case = run_reference(name, dc.case_input(name), first)
        assert rec["input_sha256"] == first["input_sha256"] and rec["args"] == first["args"]["rr"]
        margin, got = condition(rec, first, case)
        same = sd.subdivision_bytes(got["labels"]) == rec["kmeans"]["text"].encode()
        print(f"{name}: {rec['rows']} x {rec['width']}, parts {got['parts_before']} -> {got['parts']}, eligible {len(got['eligible'])}, "
              f"varzahl {[p['varzahl'] for p in got['eligible']][:8]}, margin {margin:.3g}, checker {'equal' if same else 'DIFFERS'}", flush=True)
        assert margin > MARGIN, f"{name}: a pair {margin} from the cutoff: choose another seed"
        first["kmeans"] = rec["kmeans"]
    data = json.dumps(fixture, indent=0, sort_keys=True).encode()
    with open(dc.FIXTURE, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as f:
        f.write(data)
    print(f"{dc.FIXTURE}: {len(fixture['cases'])} cases, {len(data)} bytes of JSON, {os.path.getsize(dc.FIXTURE)} on disk")


def main():
    if not os.path.exists(RR) or not os.path.exists(MC):
        sys.exit(f"{RR} is missing: run `make -C oracle ref` where the reference sources exist")
    if sys.argv[1:] == ["--deep"]:
        return main_deep()
    cases, vars_only = [], []
    for name in kc.case_names():
        rec, case = run_reference(name)
        first = rec if name in kc.NEW_BUILDERS else rc.load_fixture()[name]
        margin, got = condition(rec, first, case)
        same = sd.subdivision_bytes(got["labels"]) == rec["kmeans"]["text"].encode()
        print(f"{name}: {rec['rows']} x {rec['width']}, parts {got['parts_before']} -> {got['parts']}, eligible {len(got['eligible'])}, "
              f"varzahl {[p['varzahl'] for p in got['eligible']][:8]}, margin {margin:.3g}, checker {'equal' if same else 'DIFFERS'}", flush=True)
        if margin <= MARGIN:
            assert name not in kc.NEW_BUILDERS, f"{name}: a pair {margin} from the cutoff: choose another seed"
            vars_only.append(name)
        cases.append(rec)
    assert len(vars_only) <= 2, vars_only
    data = json.dumps({"generator": "scripts/gen_km_fixtures.py", "msa_name": rc.MSA_NAME, "vars_only": vars_only, "cases": cases},
                      indent=0, sort_keys=True).encode()
    with open(kc.FIXTURE, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as f:
        f.write(data)
    print(f"{kc.FIXTURE}: {len(cases)} cases, vars_only {vars_only}, {len(data)} bytes of JSON, {os.path.getsize(kc.FIXTURE)} on disk")


if __name__ == "__main__":
    main()
