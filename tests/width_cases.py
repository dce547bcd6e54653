"""The case tables of test_width_cases.py (no GPU: what the tables reach and that their inputs mean something) and of
test_gpu_kernel_widths.py (every case against its checker): one input per compiled width of the three kernels that keep a
Myers/Hyyro bit-vector row in a lane's registers.  Test infrastructure only.

Each kernel is compiled once per number of 32-bit words a lane holds and the host picks the instance from a length; the three
rules are restated below, next to the line they restate, and the tables hold the first and the last length of every width.
"""
from __future__ import annotations

import functools
import random

import numpy as np

import strand_checker as sc

IA_MAXWPL, IA_MAX_TEMPLATE = 35, 70000          # pia_device.hip:44 IA_MAXWPL, include/pia.h PIA_MAX_LINE
RC_MAXWPL, RC_MAX_PART = 20, 40960              # prc_device.hip:43 RC_MAXWPL, include/prc.h PRC_MAX_PART
FL_MAXW, FL_MAX_REACH = 16, 512                 # pfl_device.hip FL_MAXW, include/pfl.h PFL_MAX_REACH


# ---- the three rules -------------------------------------------------------------------------------------------------

def ia_wpl(L2: int) -> int:
    # pia_device.hip:246  const int WPL = std::max(1, (templ_len + 2047) / 2048)
    return max(1, (L2 + 2047) // 2048)


def rc_geometry(ln: int):
    """(WPL, G) of a piece of ln rows"""
    # prc_device.hip:236-239  nwords = (len + 31) / 32; wpl = std::max(1, (nwords + 63) / 64); while (G * wpl < nwords) G *= 2
    nwords = (ln + 31) // 32
    wpl = max(1, (nwords + 63) // 64)
    G = 1
    while G * wpl < nwords:
        G *= 2
    return wpl, G


def fl_nw(length: int, reach: int) -> int:
    # pfl_device.hip:223 a = std::min(len, reach); :241 nw = (a + 31) / 32, so 32 * (NW - 1) < m <= 32 * NW (:62)
    return (min(length, reach) + 31) // 32


def _bases(rng, n: int) -> bytes:
    return bytes(rng.choice(b"acgt") for _ in range(n))


# ---- InitialAligner --------------------------------------------------------------------------------------------------

def ia_lengths(wpl: int):
    """the first and the last template length of the width (the first not below 300: the reads need a template to lie in)"""
    return max(300, 2048 * (wpl - 1) + 1), min(2048 * wpl, IA_MAX_TEMPLATE)


IA_CASES = [(wpl, L2) for wpl in range(1, IA_MAXWPL + 1) for L2 in ia_lengths(wpl)]
IA_READ_NAMES = ("last 200, exact", "across a lane boundary, exact", "across a lane boundary, 15 %", "first 300, 12 %",
                 "unrelated", "over the right end")


def ia_boundary(wpl: int, L2: int) -> int:
    """a column where one lane's 32 * wpl columns end and the next lane's begin, with 120 template bases or more behind it"""
    lw = 32 * wpl
    return lw * max(1, min(31, (L2 - 120) // lw))


@functools.lru_cache(maxsize=None)
def ia_case(wpl: int, L2: int):
    """(template, six reads of at most 400 bases).  With lw = 32 * wpl the columns of one lane and b a lane boundary inside
    the template: 0 the template's last 200 bases (the entry is the last column), 1 the 200 bases around b, 2 the 350 bases
    that end just behind b with 15 % errors (the band crosses b, the traceback changes lanes), 3 the first 300 bases with
    12 % errors (the traceback leaves through column 0), 4 unrelated (a wide band), 5 the last 150 bases and 100 more (it
    hangs over the right end)."""
    assert ia_wpl(L2) == wpl
    rng = random.Random(7919 * wpl + L2)
    templ = _bases(rng, L2)
    b = ia_boundary(wpl, L2)
    reads = [templ[-200:],
             templ[max(b - 100, 0):b + 100],
             sc.mutate(rng, templ[max(b - 340, 0):b + 10], 0.15)[:400],
             sc.mutate(rng, templ[:300], 0.12)[:400],
             _bases(rng, 130),
             templ[-150:] + _bases(rng, 100)]
    assert all(0 < len(r) <= 400 for r in reads)
    return templ, reads


# ---- ReadCutter ------------------------------------------------------------------------------------------------------

RC_PARTS = 3
RC_WIDTH_LENGTHS = [ln for wpl in range(1, RC_MAXWPL + 1) for ln in (2048 * (wpl - 1) + 1, 2048 * wpl)]
RC_SHORT_LENGTHS = [65, 128, 129, 256, 257]     # G = 4, 4, 8, 8, 16: several jobs per wave
RC_GROUP_LENGTHS = [20, 40, 1024]               # G = 1 (beside length 1), 2 and 32, which the two lists above leave out
RC_LENGTHS = sorted(RC_WIDTH_LENGTHS + RC_SHORT_LENGTHS + RC_GROUP_LENGTHS)
assert len(set(RC_LENGTHS)) == len(RC_LENGTHS) and RC_LENGTHS[-1] == RC_MAX_PART


def rc_overlap(ln: int) -> int:
    return 40 if ln > 41 else 0


def rc_piece(templ: str, overlap: int, i: int) -> str:
    """piece i of RC_PARTS without what lies past the template's end (rc_checker.piece pads that with 'N')"""
    steps = len(templ) // RC_PARTS
    return templ[i * steps:i * steps + steps + overlap]


def _mutate_counted(rng, seq: str, rate: float):
    """strand_checker.mutate's errors (a third each deletions, substitutions, insertions), and how many edits were made: the
    copy's edit distance to seq is that number at the most"""
    out, edits = [], 0
    for c in seq:
        u = rng.random()
        if u < rate / 3:
            edits += 1
            continue
        if u < 2 * rate / 3:
            new = rng.choice("acgt")
            edits += new != c
            out.append(new)
        elif u < rate:
            out += [c, rng.choice("acgt")]
            edits += 1
        else:
            out.append(c)
    return "".join(out), edits


@functools.lru_cache(maxsize=None)
def rc_case(ln: int):
    """(template, overlap, reads) for pieces of ln rows, parts = 3.  With an overlap the last piece runs 40 rows past the
    template's end (the V plane has zeros there).  Read 0 holds piece 0 at 5 % errors and piece 2 at 20 %, read 1 is random
    and half a piece long: it sits beside read 0 in a wave where G < 64 and nothing in it is below a cutoff.  A 5 % copy has
    about 0.046 * ln edits, which at a few thousand rows is as often above the 5 % cutoff as below it, so the copy of piece 0
    is drawn again until its edits are fewer than that cutoff (possible from 20 rows on, where the cutoff is 1).  The short
    lengths get eight more reads of seeded lengths up to 4 * ln, each a stretch of noise around a 10 % copy of piece 0 or
    piece 2: a wave then holds jobs of unequal length, and the last wave an unfilled slot."""
    rng = random.Random(104729 + ln)
    rs = lambda n: _bases(rng, n).decode()
    mut = lambda s, rate: _mutate_counted(rng, s, rate)[0]
    overlap = rc_overlap(ln)
    templ = rs((ln - overlap) * RC_PARTS)
    p0, p2 = rc_piece(templ, overlap, 0), rc_piece(templ, overlap, RC_PARTS - 1)
    assert len(p0) == ln and len(p2) == ln - overlap
    copy0, edits = _mutate_counted(rng, p0, 0.05)
    while ln >= 20 and edits >= int(ln * 0.05):
        copy0, edits = _mutate_counted(rng, p0, 0.05)
    reads = [rs(50) + copy0 + rs(70) + mut(p2, 0.20) + rs(30), rs(ln // 2 + 3)]
    if ln in RC_SHORT_LENGTHS:
        for k in range(8):
            n = rng.randrange(1, 4 * ln + 1)
            copy = mut(p2 if k & 1 else p0, 0.10)
            body = rs(rng.randrange(0, max(n - len(copy), 0) + 1)) + copy + rs(4 * ln)      # the whole copy where it fits
            reads.append(body[:n])
    return templ, overlap, reads


def rc_reads_both(ln: int):
    """the reads of the both-strands entry: every read, then every read's reverse complement"""
    reads = rc_case(ln)[2]
    return reads + [sc.rc(r) for r in reads]


# ---- flank distances -------------------------------------------------------------------------------------------------

FL_REACH, FL_MIN_LEN = 512, 1


def fl_pattern_lengths(nw: int):
    """the first m of the word count (row m - 1 is bit 0 of word nw - 1), the last but one and the last (bit 31)"""
    return [32 * (nw - 1) + 1, 32 * nw - 1, 32 * nw]


def fl_text_lengths(m: int):
    """texts for a pattern of m rows: no slack, the whole slack of m / 4, one base more, far more"""
    return [m, m + m // 4, m + m // 4 + 1, 2 * m + 7]


def fl_lengths():
    """Every pattern length once.  The four texts of all 48 patterns would be 240 flanks, and the numpy checker's time goes
    with the square of that, so the table stays under 130: the last m of every word count gets all four texts, the first m a
    second flank of its own length (a text without slack), and every pattern has every longer flank for a text anyway."""
    out = []
    for nw in range(1, FL_MAXW + 1):
        first, _mid, last = fl_pattern_lengths(nw)
        out += fl_pattern_lengths(nw) + fl_text_lengths(last) + [first]
    return out


@functools.lru_cache(maxsize=None)
def fl_case():
    """(pieces, piece, mode): noisy copies of three parents as test_gpu_flanks.family makes them, modes cycling 0..3"""
    from test_gpu_flanks import family
    lengths = fl_lengths()
    pieces = family(np.random.default_rng(2718), lengths)
    assert [len(p) for p in pieces] == lengths
    return pieces, list(range(len(pieces))), [k % 4 for k in range(len(pieces))]
