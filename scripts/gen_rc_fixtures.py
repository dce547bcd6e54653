#!/usr/bin/env python3
"""TEST INFRASTRUCTURE.  Generates the rc_* fixtures under tests/golden/ by running the *reference's own* ReadCutter (and,
for the chain case, its InitialAligner), compiled into a temporary directory outside the repository from the sources
where they lie ($RC_REFERENCE, default /root/reference).  Only data is committed: the inputs, the bytes of the files the
reference writes, its stdout and its exit code.  Runs only where the reference exists (the build container); the GPU box
sees just the fixtures.

    python scripts/gen_rc_fixtures.py            # the small cases: rc_cases.json + rc_*.gz
    python scripts/gen_rc_fixtures.py --full     # rc_tree_default.json: digests of the benchmark data set's full reads
"""
import gzip
import hashlib
import json
import os
import platform
import random
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from repeatresolver_amd import datagen as dg  # noqa: E402

REF = os.environ.get("RC_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

# the small Tree data set of the fixtures: reads with flanks, one repeat copy at most per read
TREE = dg.SimConfig(kind="Tree", copies=6, coverage=5, difference=0.01, repeat_len=3000, flank=1000, length_scale=0.2,
                    min_aligned=100, seed=61)


def compile_ref(td):
    rc_bin, ia_bin = os.path.join(td, "ReadCutter"), os.path.join(td, "InitialAligner")
    subprocess.run(["gcc", "-O2", "-w", os.path.join(REF, "ReadCutter.c"), "-o", rc_bin, "-lm"], check=True)
    subprocess.run(["gcc", "-O2", "-w", os.path.join(REF, "InitialAligner.c"), "-o", ia_bin, "-lpthread"], check=True)
    return rc_bin, ia_bin


def write_gz(path, data: bytes):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)


def run_rc(rc_bin, wd, templ_name, reads_name, args):
    """one reference run in wd; returns (exit code, stdout, Seq.fasta bytes or None, ReadSeqInfo bytes or None)"""
    for f in os.listdir(wd):
        if f.endswith(("Seq.fasta", "ReadSeqInfo")):
            os.remove(os.path.join(wd, f))
    p = subprocess.run([rc_bin, templ_name, reads_name, "-o", "out_Seq.fasta", "-r", "out_ReadSeqInfo"] + args, cwd=wd,
                       capture_output=True)
    rd = lambda f: open(os.path.join(wd, f), "rb").read() if os.path.exists(os.path.join(wd, f)) else None
    return p.returncode, p.stdout, rd("out_Seq.fasta"), rd("out_ReadSeqInfo")


def mutate(rng, s, rate):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            continue                                            # deletion
        if r < 2 * rate / 3:
            out.append(rng.choice("acgt"))                      # insertion
        out.append(rng.choice("acgt") if rate / 3 * 2 <= r < rate else ch)
    return "".join(out)


def fasta(records, width=100):
    out = []
    for r in records:
        out.append(">\n")
        out.extend(r[i:i + width] + "\n" for i in range(0, len(r), width))
    return "".join(out).encode()


def small_cases():
    cases, inputs = [], {}
    with tempfile.TemporaryDirectory() as td:
        rc_bin, ia_bin = compile_ref(td)
        wd = os.path.join(td, "wd")
        os.mkdir(wd)

        def add_input(name, templ_name, templ: bytes, reads: bytes):
            inputs[name] = templ_name
            with open(os.path.join(wd, templ_name), "wb") as f:
                f.write(templ)
            with open(os.path.join(wd, name + "_reads.fasta"), "wb") as f:
                f.write(reads)
            write_gz(os.path.join(OUT, f"rc_{name}.template.gz"), templ)
            write_gz(os.path.join(OUT, f"rc_{name}.reads.gz"), reads)

        def add(case, inp, args, note, again=False):
            r = run_rc(rc_bin, wd, inputs[inp], inp + "_reads.fasta", args)
            if again:                                               # undefined bytes of the reference: keep only if stable
                r2 = run_rc(rc_bin, wd, inputs[inp], inp + "_reads.fasta", args)
                if r2 != r:
                    print("dropped (two reference runs disagree):", case)
                    return None
            code, out, seq, info = r
            write_gz(os.path.join(OUT, f"rc_{case}.seq.gz"), seq if seq is not None else b"")
            write_gz(os.path.join(OUT, f"rc_{case}.info.gz"), info if info is not None else b"")
            cases.append({"name": case, "input": inp, "template_name": inputs[inp], "args": args, "exit_code": code,
                          "stdout": out.decode("latin1"), "note": note})
            print(case, code, len(seq or b""), (info or b"").count(b"\n"), "records")
            return r

        # a small Tree data set: flanks on both sides of one repeat copy per read
        with tempfile.TemporaryDirectory() as sd:
            dg.write_dataset(os.path.join(sd, "x"), TREE)
            add_input("tree", "treeTemplate.fasta", open(os.path.join(sd, "x_Template.fasta"), "rb").read(),
                      open(os.path.join(sd, "x.fasta"), "rb").read())
        add("tree", "tree", [], "defaults (-p 60)")
        for a, v in (("-p", "1"), ("-p", "2"), ("-p", "3"), ("-e", "0.15"), ("-w", "10")):
            add(f"tree_{a[1]}{v.replace('.', '')}", "tree", [a, v], f"same reads, {a} {v}")
        # overlap past the template's end: the last part reads bytes the reference never initialised
        add("tree_l80", "tree", ["-p", "60", "-l", "80"], "-l 80: the last part runs 80 bytes past the template", again=True)
        # chain: the reference's InitialAligner on the reference's Seq.fasta of the default case
        _, _, seq, _ = run_rc(rc_bin, wd, inputs["tree"], "tree_reads.fasta", [])
        with open(os.path.join(wd, "chain_Seq.fasta"), "wb") as f:
            f.write(seq)
        p = subprocess.run([ia_bin, inputs["tree"], "chain_Seq.fasta", "-o", "chain_MSA", "-s", "chain_SeqClass"], cwd=wd,
                           capture_output=True, check=True)
        write_gz(os.path.join(OUT, "rc_chain.msa.gz"), open(os.path.join(wd, "chain_MSA"), "rb").read())
        write_gz(os.path.join(OUT, "rc_chain.seqclass.gz"), open(os.path.join(wd, "chain_SeqClass"), "rb").read())
        print("chain", p.returncode, os.path.getsize(os.path.join(wd, "chain_MSA")))

        # several template copies per read with a short template: several cuts, the merge rules
        rng = random.Random(62)
        templ = "".join(rng.choice("acgt") for _ in range(300))
        reads = []
        for k in range(40):
            ncopy = rng.randrange(0, 7)
            parts = ["".join(rng.choice("acgt") for _ in range(rng.randrange(0, 500)))]
            for _ in range(ncopy):
                cp = templ[rng.randrange(0, 40):] if rng.random() < 0.3 else templ
                parts.append(mutate(rng, cp, rng.choice((0.0, 0.05, 0.12, 0.25))))
                if rng.random() < 0.4:
                    parts.append("".join(rng.choice("acgt") for _ in range(rng.randrange(0, 150))))
            parts.append("".join(rng.choice("acgt") for _ in range(rng.randrange(0, 500))))
            reads.append("".join(parts))
        add_input("copies", "copiesTemplate.fasta", b">t\n" + templ.encode() + b"\n", fasta(reads, 80))
        add("copies", "copies", [], "up to six copies per read, -p 60")
        add("copies_p4", "copies", ["-p", "4"], "up to six copies per read, -p 4")
        add("copies_p3e20", "copies", ["-p", "3", "-e", "0.2"], "-p 3 -e 0.2")

        # the reader's edge cases (template path without the Template.fasta suffix: default names are unprefixed)
        rng = random.Random(63)
        rs = lambda n: "".join(rng.choice("acgt") for _ in range(n))
        t2 = rs(400)
        a = rs(300) + mutate(rng, t2, 0.05) + rs(350)
        b = rs(200) + mutate(rng, t2, 0.05) + rs(600) + mutate(rng, t2, 0.04) + rs(250)
        edge = ("acgtNNacgt\n"                                         # lines before the first '>' join record 0
                + ">first read with header text\r\n" + a[:500].upper() + "\r\n" + a[500:].replace("a", "aN") + "\n"
                + ">\n"                                                # an empty record
                + ">mixed case, wrapped\n" + "\n".join(b[i:i + 61].swapcase() if i % 2 else b[i:i + 61] for i in range(0, len(b), 61)) + "\n"
                + ">x\n" + rs(40) + "\n"
                + ">longer than the one before it\n" + a + "\n"
                + ">shorter than the one before it\n" + rs(900) + mutate(rng, t2, 0.03) + rs(700) + "\n"
                + ">last, shorter than the one before it\n" + a[:700] + "\n")
        add_input("edge", "edge_t.fa", (">t2\r\n" + t2[:200] + "\r\n" + t2[200:].upper() + "\n").encode(), edge.encode())
        add("edge", "edge", ["-p", "8"], "N, mixed case, CRLF, wrapped lines, header text, empty record, lines before the first '>'")
        add_input("edge_longer", "edge_t.fa", (">t2\n" + t2 + "\n").encode(),
                  (">\n" + b + "\n>\n" + rs(100) + "\n>\n" + a + rs(500) + "\n>\n").encode())
        add("edge_longer", "edge_longer", ["-p", "8"], "a last record longer than the one before it, then a bare '>' line")
        add_input("one", "oneTemplate.fasta", (">t2\n" + t2 + "\n").encode(), (">\n" + a + "\n").encode())
        add("one", "one", ["-p", "8"], "a file with one record")
        add_input("empty", "emptyTemplate.fasta", (">t2\n" + t2 + "\n").encode(), b"")
        add("empty", "empty", [], "an empty reads file")
    with open(os.path.join(OUT, "rc_cases.json"), "w") as f:
        json.dump({"generator": "scripts/gen_rc_fixtures.py", "reference_build": "gcc -O2 ReadCutter.c -lm",
                   "tree_config": TREE.__dict__, "cases": cases}, f, indent=1)


def full():
    """the benchmark data set's full reads (write_dataset with CONFIGS['tree_default']): digests, stdout and wall time"""
    with tempfile.TemporaryDirectory() as td:
        rc_bin, _ = compile_ref(td)
        info = dg.write_dataset(os.path.join(td, "tree_default"), dg.CONFIGS["tree_default"])
        shutil.move(os.path.join(td, "tree_default_Template.fasta"), os.path.join(td, "tdTemplate.fasta"))
        t0 = time.time()
        code, out, seq, rsi = run_rc(rc_bin, td, "tdTemplate.fasta", "tree_default.fasta", [])
        wall = time.time() - t0
        reads = open(os.path.join(td, "tree_default.fasta"), "rb").read()
        fx = {"generator": "scripts/gen_rc_fixtures.py --full", "reference_build": "gcc -O2 ReadCutter.c -lm",
              "workload": "tree_default", "template_name": "tdTemplate.fasta", "args": [], "dataset": info,
              "reads_sha256": hashlib.sha256(reads).hexdigest(), "reads_bytes": len(reads),
              "exit_code": code, "stdout": out.decode("latin1"),
              "seq_sha256": hashlib.sha256(seq).hexdigest(), "seq_bytes": len(seq),
              "info_sha256": hashlib.sha256(rsi).hexdigest(), "info_bytes": len(rsi),
              "reference_wall_s": round(wall, 1), "reference_host": f"{platform.processor() or platform.machine()}, one core"}
    with open(os.path.join(OUT, "rc_tree_default.json"), "w") as f:
        json.dump(fx, f, indent=1)
    print({k: v for k, v in fx.items() if k != "stdout"})


if __name__ == "__main__":
    if "--full" in sys.argv[1:]:
        full()
    else:
        small_cases()
