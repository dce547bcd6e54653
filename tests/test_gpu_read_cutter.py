"""ReadCutter on the GPU: prc_occurrences against the CPU checker on random jobs, the drop-in CLI against every rc_* fixture of
the reference, the chain ReadCutter -> InitialAligner against the reference's MSA, and the benchmark data set's full reads
against the reference's digests (rc_tree_default.json)."""
import gzip
import hashlib
import json
import os
import random
import subprocess

import pytest

import rc_checker as ck
from repeatresolver_amd import datagen as dg
from repeatresolver_amd import initial_aligner, read_cutter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLDEN, "rc_cases.json")))["cases"]


def gz(name) -> bytes:
    with gzip.open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _mutate(rng, s, rate):
    out = []
    for ch in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice("acgt"))
        out.append(rng.choice("acgt") if r < rate else ch)
    return "".join(out)


@pytest.mark.gpu
@pytest.mark.parametrize("ln", [1, 31, 32, 33, 64, 500, 512, 513, 2049, 40000])
def test_occurrences_equal_checker(ln):
    """random jobs around the 32-row word and the 64 lanes of a wave; these lengths reach 1, 2 and 20 words per lane and
    G = 1, 2, 16, 32, 64: test_gpu_kernel_widths.py runs every width and every G"""
    rng = random.Random(ln)
    rs = lambda n: "".join(rng.choice("acgt") for _ in range(n))
    big = ln >= 2049
    # parts = 3: piece 0 and piece 2 of a template 3 * steps long; overlap > 0 runs the last piece past the template's end
    configs = ((3, 40),) if ln == 40000 else ((3, 0), (3, min(ln - 1, 40))) + (() if big else ((1, 0),))
    for parts, overlap in configs:
        steps = ln - overlap
        templ = rs(steps * parts)
        reads = ["", rs(1), rs(max(ln - 1, 1))]
        for k in range(3 if big else 10):
            segs = [rs(rng.randrange(0, max(2, ln // 2)))]
            for _ in range(rng.randrange(0 if not big else 1, 4)):
                src = ck.piece(templ, parts, overlap, rng.choice((0, parts - 1))).replace("N", "")
                segs.append(_mutate(rng, src, rng.choice((0.0, 0.05, 0.2, 0.4))))
                segs.append(rs(rng.randrange(0, ln + 5)))
            reads.append("".join(segs)[:ln + 3000 if big else 8 * ln + 2000])
        g = read_cutter.ReadCutter(templ.encode())
        try:
            got = {e: g.occurrences([r.encode() for r in reads], parts, overlap, e) for e in (0.30, 0.05)}
        finally:
            g.close()
        pieces = [ck.piece(templ, parts, overlap, q) for q in ((0, parts - 1) if parts > 1 else (0,))]
        for j, r in enumerate(reads):
            rows = [ck.last_row_myers(pc, r) for pc in pieces]
            for e in (0.30, 0.05):
                exp = [ck.scan(row, ln, int(ln * e)) for row in rows]
                assert [list(map(int, o)) for o in got[e][j]] == exp, (ln, parts, overlap, e, len(r))


@pytest.mark.gpu
def test_cut_many_runs_overflow_rerun():
    """a read with far more runs below the cutoff than the first launch has room for: re-run, nothing dropped"""
    rng = random.Random(3)
    templ = "".join(rng.choice("acgt") for _ in range(40))
    piece = templ[:20]
    read = "".join(piece + "".join(rng.choice("acgt") for _ in range(rng.randrange(3, 30))) for _ in range(60))
    g = read_cutter.ReadCutter(templ.encode())
    try:
        got = g.occurrences([read.encode()], 2, 0, 0.30)[0]
        cuts = g.cut([read.encode()], 2, 0, 0.30)[0]
    finally:
        g.close()
    exp = ck.occurrences(templ, read, 2, 0, 0.30)
    assert len(exp[0]) > 20
    assert [list(map(int, o)) for o in got] == exp
    assert list(map(int, cuts)) == ck.cut(templ, read, 2, 0, 0.30)


def _run_case(tmp_path, templ_name, templ, reads, args):
    """the drop-in run as the fixture generator ran the reference: in the directory of its inputs, with -o and -r"""
    (tmp_path / templ_name).write_bytes(templ)
    (tmp_path / "reads.fasta").write_bytes(reads)
    p = subprocess.run([read_cutter.CLI_PATH, templ_name, "reads.fasta", "-o", "out_Seq.fasta", "-r", "out_ReadSeqInfo"] + args,
                       cwd=str(tmp_path), capture_output=True, text=True)
    return p.returncode, p.stdout, (tmp_path / "out_Seq.fasta").read_bytes(), (tmp_path / "out_ReadSeqInfo").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_reproduces_reference(tmp_path, case):
    templ, reads = gz(f"rc_{case['input']}.template.gz"), gz(f"rc_{case['input']}.reads.gz")
    code, out, seq, info = _run_case(tmp_path, case["template_name"], templ, reads, case["args"])
    assert code == case["exit_code"]
    assert out == case["stdout"]
    assert seq == gz(f"rc_{case['name']}.seq.gz")
    assert info == gz(f"rc_{case['name']}.info.gz")


@pytest.mark.gpu
def test_chain_read_cutter_then_initial_aligner(tmp_path):
    case = next(c for c in CASES if c["name"] == "tree")
    code, _, seq, _ = _run_case(tmp_path, case["template_name"], gz("rc_tree.template.gz"), gz("rc_tree.reads.gz"), [])
    assert code == 0
    code, _ = initial_aligner.run_files(tmp_path / case["template_name"], tmp_path / "out_Seq.fasta", tmp_path / "MSA",
                                        tmp_path / "SeqClass")
    assert code == 0
    assert (tmp_path / "MSA").read_bytes() == gz("rc_chain.msa.gz")
    assert (tmp_path / "SeqClass").read_bytes() == gz("rc_chain.seqclass.gz")


@pytest.mark.gpu
def test_full_benchmark_reads_match_reference_digests(tmp_path):
    fx = json.load(open(os.path.join(GOLDEN, "rc_tree_default.json")))
    dg.write_dataset(str(tmp_path / "tree_default"), dg.CONFIGS["tree_default"])
    os.replace(tmp_path / "tree_default_Template.fasta", tmp_path / fx["template_name"])
    reads = (tmp_path / "tree_default.fasta").read_bytes()
    assert hashlib.sha256(reads).hexdigest() == fx["reads_sha256"]       # the data set itself has not drifted
    p = subprocess.run([read_cutter.CLI_PATH, fx["template_name"], "tree_default.fasta", "-o", "out_Seq.fasta", "-r",
                        "out_ReadSeqInfo"], cwd=str(tmp_path), capture_output=True, text=True)
    assert p.returncode == fx["exit_code"]
    assert p.stdout == fx["stdout"]
    seq, info = (tmp_path / "out_Seq.fasta").read_bytes(), (tmp_path / "out_ReadSeqInfo").read_bytes()
    assert (len(seq), hashlib.sha256(seq).hexdigest()) == (fx["seq_bytes"], fx["seq_sha256"])
    assert (len(info), hashlib.sha256(info).hexdigest()) == (fx["info_bytes"], fx["info_sha256"])
