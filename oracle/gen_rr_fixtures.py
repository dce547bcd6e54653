#!/usr/bin/env python3
"""TEST INFRASTRUCTURE.  Generates tests/golden/rr_reference.json.gz by running the *compiled reference* MaxCorrelation and
RepeatResolver (oracle/_ref/max_correlation, oracle/_ref/repeat_resolver: the unmodified program text linked with
oracle/gsl_standin.c, built by `make -C oracle ref`) on the seeded inputs of tests/rr_cases.py.  Only data is committed:
per case the arguments, the sha256 of the input, the deterministic stdout lines, the MaxCorrsOf_ file (line count + the
non-zero lines) and the two label files verbatim with their names.  KmeansSubdivisionOf_* is not recorded.  Runs only where
the reference exists (the build container); the GPU box sees just the fixture.

    python oracle/gen_rr_fixtures.py            # rewrites tests/golden/rr_reference.json.gz, byte for byte reproducible
    python oracle/gen_rr_fixtures.py --deep     # the second case table, DEEP_LABEL_CASES of tests/deep_cases.py (more than
                                                # 2 047 kept rows), into tests/golden/rr_deep_reference.json.gz; then
                                                # scripts/gen_km_fixtures.py --deep adds the third label file to each record

The conditions that make an exact comparison of the labels legitimate are asserted here for every case with labels (and
again from the fixture by tests/test_rr_reference.py; rr_cases.label_conditions): no significant variation is `undecided`
(tests/gr_checker.py: two unequal candidate values closer than 1e-8 among the first 30, or one at the greedy threshold) and
no non-zero MaxCorrs value lies within 1e-5 of the cutoff.  A case that fails one gets another seed; the comparison is not
loosened.  Three inputs of the existing tests (kept64, kept65, rel5groups) hold one undecided variation each; they stay, since
those tests are built on them, under the condition rr_cases.clique_set_decided (the order within the clique is open, the
clique as a set and hence every label is not), and each has a reseeded sibling that meets the strict condition."""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gr_checker as gc  # noqa: E402
import rr_cases as rc  # noqa: E402

MC = os.path.join(HERE, "_ref", "max_correlation")
RR = os.path.join(HERE, "_ref", "repeat_resolver")
MC_LINES = re.compile(r"^(There are \d+ sequences\.|Siglength is \d+\.|Cutoff .*)$")
RR_LINES = re.compile(r"^(Of \d+ sequences, \d+ had full coverage\.|Siglength was .*|\d+ correlations make the cutoff\.|Cutoff .*|Maxcov: .*)$")


def run_reference(case):
    """one run of both programs in a fresh directory; returns the record without name and conditions"""
    rows, cov, von, bis = case["rows"], case["cov"], case["von"], case["bis"]
    inp = rc.msa_bytes(rows)
    mc_args = [rc.MSA_NAME, "-c", str(cov), "-p", "1"]
    rr_args = [rc.MSA_NAME, "-c", str(cov)] + (["-f", str(von), str(bis)] if von is not None else [])
    rec = {"cov": cov, "von": von, "bis": bis, "labels": case["labels"], "rows": len(rows), "width": len(rows[0]),
           "input_sha256": rc.input_sha256(rows), "args": {"mc": mc_args}, "stdout": {}}
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, rc.MSA_NAME), "wb") as f:
            f.write(inp)
        p = subprocess.run([MC] + mc_args, cwd=td, capture_output=True, check=True, timeout=600)
        rec["stdout"]["mc"] = [l for l in p.stdout.decode("latin1").splitlines() if MC_LINES.match(l)]
        text = open(os.path.join(td, "MaxCorrsOf_" + rc.MSA_NAME)).read()
        assert text.endswith("\n")
        lines = text.split("\n")[:-1]
        assert len(lines) == len(rows[0]) * 5
        rec["maxcorrs"] = {"lines": len(lines), "nonzero": [[i, l] for i, l in enumerate(lines) if l != "0.000000"]}
        if case["labels"]:
            # RepeatResolver needs MaxCorrsOf_MSA to exist: it dereferences the array before its NULL check (RR:3981)
            p = subprocess.run([RR] + rr_args, cwd=td, capture_output=True, check=True, timeout=600)
            rec["args"]["rr"] = rr_args
            rec["stdout"]["rr"] = [l for l in p.stdout.decode("latin1").splitlines() if RR_LINES.match(l)]
            names = sorted(n for n in os.listdir(td) if n.startswith(("DropoffSubdivisionOf_", "RelDropSubdivisionOf_")))
            assert len(names) == 2, names
            rec["dropoff"] = {"file": names[0], "text": open(os.path.join(td, names[0])).read()}
            rec["reldrop"] = {"file": names[1], "text": open(os.path.join(td, names[1])).read()}
    return rec


def split_parts(rec):
    """the stage-1 parts that stage 2 split, from the reference's two label files alone"""
    a = [int(v) for v in rec["dropoff"]["text"].split("\n")]
    b = [int(v) for v in rec["reldrop"]["text"].split("\n")]
    into = {}
    for x, y in zip(a, b):
        if x >= 0:
            into.setdefault(x, set()).add(y)
    return sorted(k for k, v in into.items() if len(v) > 1), max(a) + 1, max(b) + 1


REFERENCE_BUILD = "gcc -O2 -w -mcmodel=medium -Igsl_standin {MaxCorrelation,RepeatResolver}.c gsl_standin.c mc_oracle.c -lm -lpthread"


def record(name, case):
    """the reference's record of one case, its conditions asserted"""
    rec = {"name": name}
    rec.update(run_reference(case))
    msg = f"{name}: {rec['rows']} x {rec['width']}, {len(rec['maxcorrs']['nonzero'])} non-zero MaxCorrs"
    if case["labels"]:
        rec["condition"], sig, und = rc.label_conditions(case, rec)
        assert (rec["condition"] == "strict") == (name not in ("kept64", "kept65", "rel5groups")), (name, und)
        split, n1, n2 = split_parts(rec)
        msg += f", {sig} significant, undecided {und} ({rec['condition']}), parts {n1} -> {n2}, split {split}"
    print(msg, flush=True)
    return rec


def write_fixture(path, head, cases):
    data = json.dumps(dict(head, cases=cases), indent=0, sort_keys=True).encode()
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=raw, mtime=0) as f:
        f.write(data)
    print(f"{path}: {len(cases)} cases, {len(data)} bytes of JSON, {os.path.getsize(path)} on disk")


def main():
    for b in (MC, RR):
        if not os.path.exists(b):
            sys.exit(f"{b} is missing: run `make -C oracle ref` where the reference sources exist")
    if sys.argv[1:] == ["--deep"]:
        import deep_cases as dc
        cases = [record(name, dc.case_input(name)) for name in dc.DEEP_LABEL_CASES]
        write_fixture(dc.FIXTURE, {"generator": "oracle/gen_rr_fixtures.py --deep, then scripts/gen_km_fixtures.py --deep",
                                   "reference_build": REFERENCE_BUILD, "msa_name": rc.MSA_NAME}, cases)
        return
    cases = [record(name, rc.case_input(name)) for name in rc.BUILDERS]
    by = {c["name"]: c for c in cases}
    assert split_parts(by["stretched"])[0] == [40]                    # one pass of 64 parts is not enough: 192 parts ...
    deep = split_parts(by["stretched_deep"])[0]
    assert deep and all(k >= rc.KERNEL_TILE for k in deep), deep      # ... and here the splits lie beyond the first pass
    write_fixture(rc.FIXTURE, {"generator": "oracle/gen_rr_fixtures.py", "reference_build": REFERENCE_BUILD, "msa_name": rc.MSA_NAME}, cases)


if __name__ == "__main__":
    main()
