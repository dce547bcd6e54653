"""dev: instructions per DP row of k_fill_v3 in a built libpwr.so:  row_instr_count.py <libpwr.so> [kernel substring]

The straight-line groups of the fast path are 16 copies of one row; every row ends with the store of its hand-over word (the
row marker: `global_store_dwordx2 ... sc1`; the builds that published two words per row end it with
`global_store_dwordx4 ... sc1`: set MARKER=global_store_dwordx4 in the environment for those).  The kernel's code is cut at these stores; a run of at least 12 pieces
whose lengths differ by at most one (a wait state more or less) is one straight-line group, and its most frequent length is
the row's instruction count; the s_nop among them are the wait states the compiler pads hazards with (a DPP operand two
instructions behind its VALU write, ...), which cost a lone wave an issue slot like any instruction.  The compiler lays the seven groups out in an order of its own, so they are named by size: the
three shortest are the warm-up's (no record) and the longest is the one with run-time flags; within the warm-up and within the
own part INTERIOR < LEFT < RIGHT (a guard costs a compare and a select per cell, RIGHT posts the row minimum as well).
Needs llvm-objdump of ROCm (no GPU)."""
import os
import re
import struct
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")
MARKER = os.environ.get("MARKER", "global_store_dwordx2")


def code_objects(path):
    """the AMDGPU ELF images inside the library's fat binary"""
    data = open(path, "rb").read()
    out, pos = [], 0
    while True:
        pos = data.find(b"\x7fELF\x02\x01\x01", pos)
        if pos < 0:
            return out
        machine = struct.unpack_from("<H", data, pos + 18)[0]
        if machine == 224:                                   # EM_AMDGPU
            shoff, = struct.unpack_from("<Q", data, pos + 40)
            shentsize, shnum = struct.unpack_from("<HH", data, pos + 58)
            out.append(data[pos:pos + shoff + shentsize * shnum])
        pos += 4


def kernel_lines(lib, want):
    for img in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(img)
            f.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        m = re.search(r"^[0-9a-f]+ <(%s)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)" % want, txt, re.S | re.M)
        if m:
            return [l.split("//")[0].strip() for l in m.group(2).splitlines() if l.strip() and not l.strip().endswith(":")]
    raise SystemExit("kernel %s not found in %s" % (want, lib))


def main():
    lib = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "_Z9k_fill_v3ILi5ELi4ELb0EEv6DState7JobBufs"
    ins = kernel_lines(lib, want)
    marks = [i for i, l in enumerate(ins) if l.startswith(MARKER) and "sc1" in l]
    gaps = [b - a for a, b in zip(marks, marks[1:])]
    groups, i = [], 0
    while i < len(gaps):
        j = i
        while j < len(gaps) and abs(gaps[j] - gaps[i]) <= 1:
            j += 1
        if j - i >= 12:
            n = max(set(gaps[i:j]), key=gaps[i:j].count)
            k = i + gaps[i:j].index(n)
            kinds = {"v": 0, "s": 0, "ds": 0, "mem": 0, "nop": 0}
            for l in ins[marks[k] + 1:marks[k + 1] + 1]:
                op = l.split()[0]
                kinds["nop"] += op == "s_nop"                # (counted among the scalar ones too)
                kinds["ds" if op.startswith("ds_") else "mem" if op.startswith(("global_", "buffer_", "flat_")) else "s" if op.startswith("s_") else "v"] += 1
            groups.append((n, kinds))
        i = max(j, i + 1)
    print("%s  %s: %d instructions, %d row markers" % (os.path.basename(lib), want, len(ins), len(marks)))
    names = {}
    if len(groups) == 7:
        order = sorted(range(7), key=lambda k: groups[k][0])
        for k, name in zip(order, ["warm-up INTERIOR", "warm-up LEFT", "warm-up RIGHT", "own INTERIOR", "own LEFT", "own RIGHT", "own run-time flags"]):
            names[k] = name
    for k in sorted(range(len(groups)), key=lambda k: groups[k][0]):
        n, kinds = groups[k]
        print("  %-20s %3d instructions per row (%d vector, %d scalar, %d LDS, %d store; %d of the scalar ones wait states)" % (names.get(k, "group %d" % k), n, kinds["v"], kinds["s"], kinds["ds"], kinds["mem"], kinds["nop"]))


if __name__ == "__main__":
    main()
