"""CPU checker for the ReadCutter port: a plain-Python restatement of ReadCutter.c ("RC:"), pinned to the reference by the
rc_* fixtures (scripts/gen_rc_fixtures.py).  Test infrastructure only; the product path is include/prc.h.

It holds the pieces the tests compare one by one: the reader's record semantics, the last DP row by Myers' bit-vector search
on Python ints (and by the literal matrix, for small inputs), the literal scan of that row, the cut selection, the writer and
the stdout lines.
"""
from __future__ import annotations

SENTINEL = 100000          # RC:527-528
_KEEP = {ord(c): c.lower() for c in "aAcCgGtT"}


def bases_of(line: bytes) -> str:
    return "".join(_KEEP[b] for b in line if b in _KEEP)


def read_template(data: bytes) -> str:
    """RC:169-185: lines not starting with '>' contribute their aAcCgGtT, lower-cased"""
    return "".join(bases_of(ln) for ln in data.split(b"\n") if not ln.startswith(b">"))


def read_records(data: bytes):
    """ReadCounter + ReadingFasta (RC:66-135, RC:858-872): returns (records, last) where records are the bases of each record
    ('>' lines start one; lines before the first join record 0) and `last` is what the reference analyses and writes for the
    last record: it meets EOF before a second '>' and keeps the previous record's length, over the previous record's bytes."""
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines = lines[:-1]
    recs, cur, seen = [], [], False
    for ln in lines:
        if ln.startswith(b">"):
            if seen:
                recs.append("".join(cur))
                cur = []
            seen = True
        else:
            cur.append(bases_of(ln))
    if not seen:
        return [], ""
    recs.append("".join(cur))
    if len(recs) == 1:
        return recs, ""
    prev, last = recs[-2], recs[-1]
    return recs, (last + prev[len(last):])[:len(prev)]


def last_row_dense(pat: str, read: str):
    """the literal matrix of Occurrence (RC:499-520), last row only kept; M(x,-1) = x + 1, M(-1,y) = 0"""
    m = len(pat)
    if m == 0:
        return [0] * len(read)
    col = list(range(1, m + 1))            # column -1: M(x,-1) = x + 1
    row = []
    for ch in read:
        new = [0] * m
        diag, up = 0, 0                     # M(-1, y-1) = M(-1, y) = 0
        for x in range(m):
            v = min(diag + (pat[x] != ch), up + 1, col[x] + 1)
            diag, up = col[x], v
            new[x] = v
        col = new
        row.append(col[-1])
    return row


def last_row_myers(pat: str, read: str):
    """the same row by Myers' bit-vector search on Python ints; pattern bytes that are not acgt match nothing"""
    m = len(pat)
    if m == 0:
        return [0] * len(read)
    mask, top = (1 << m) - 1, 1 << (m - 1)
    peq = {c: 0 for c in "acgt"}
    for i, c in enumerate(pat):
        if c in peq:
            peq[c] |= 1 << i
    pv, mv, score, row = mask, 0, m, []
    for ch in read:
        eq = peq.get(ch, 0)
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | (~(xh | pv) & mask)
        mh = pv & xh
        if ph & top:
            score += 1
        elif mh & top:
            score -= 1
        ph = (ph << 1) & mask
        mh = (mh << 1) & mask
        pv = mh | (~(xv | ph) & mask)
        mv = ph & xv
        row.append(score)
    return row


def scan(score, len1: int, cutoff: int):
    """RC:525-567, literally: the positions, in the reference's (descending) order"""
    on, lastmin, mn, ey, pos = 0, SENTINEL, SENTINEL, 0, []
    for i in range(len(score) - 1, 0, -1):
        if score[i] < cutoff:
            on = 1
        else:
            if on:
                if pos and pos[-1] - ey > len1 // 2:
                    pos.append(ey)
                elif pos and pos[-1] - ey <= len1 // 2:
                    if lastmin > mn:
                        pos[-1] = ey
                elif not pos:
                    pos.append(ey)
            on, lastmin, mn = 0, mn, SENTINEL
        if on and score[i] < mn:
            mn, ey = score[i], i
    return pos


def piece(templ: str, parts: int, overlap: int, i: int) -> str:
    """&Template[i * steps], len bytes (RC:601); past the template's end a byte that matches no base ('N')"""
    steps = len(templ) // parts
    ln = steps + overlap
    s = templ[i * steps:i * steps + ln]
    return s + "N" * (ln - len(s))


def params(templ: str, parts: int, overlap: int, e: float):
    ln = len(templ) // parts + overlap
    return ln, int(ln * e)                  # RC:583-585 ((int) truncates toward zero, as int() does)


def occurrences(templ: str, read: str, parts: int, overlap: int, e: float, row=last_row_myers):
    """Positions of piece 0 and piece parts-1 (piece 0 alone when parts == 1), RC:597-611"""
    ln, cutoff = params(templ, parts, overlap, e)
    out = [scan(row(piece(templ, parts, overlap, 0), read), ln, cutoff)]
    if parts > 1:
        out.append(scan(row(piece(templ, parts, overlap, parts - 1), read), ln, cutoff))
    return out


def select_cuts(parts: int, ln: int, T: int, readlen: int, pos0, posL):
    """RC:614-755: candidates by part index (indices 1 .. parts-2 hold piece 0's positions, RC:600-610), then the picks, in
    place as the reference makes them"""
    if parts == 1:
        return [p for p in sorted(pos0) if p > ln and readlen - p > ln]
    by_idx = lambda idx: sorted(posL) if idx == parts - 1 else sorted(pos0)
    a = []
    for idx, sh in ((parts - 1, 0), (0, -ln), (parts - 2, ln), (1, -2 * ln)):
        a += [p + sh for p in by_idx(idx) if p + sh > ln and readlen - (p + sh) > ln]
    n = 0
    for i in range(len(a)):
        if a[i] < T + T // 2:
            a[0] = a[i]
            n = 1
            break
    if n == 0:
        return []                           # (the reference reads CuttingPoints[-1] next: undefined, no candidate follows)
    for _ in range(60):
        for i in range(len(a)):
            if a[n - 1] + T // 2 < a[i] < a[n - 1] + T + T // 2:
                a[n] = a[i]
                n += 1
                break
        else:
            break
    return a[:n]


def cut(templ: str, read: str, parts: int, overlap: int, e: float):
    ln, _ = params(templ, parts, overlap, e)
    occ = occurrences(templ, read, parts, overlap, e)
    return select_cuts(parts, ln, len(templ), len(read), occ[0], occ[-1])


def write_record(read: str, cuts) -> str:
    """OutputOfCuts (RC:894-912)"""
    out, j = [">\n"], 0
    for i, ch in enumerate(read):
        if j < len(cuts) and i == cuts[j]:
            out.append("\n>\n")
            j += 1
        out.append(ch)
    out.append("\n")
    return "".join(out)


def parse_args(argv):
    """RC:985-1030 (argv without the program name; argv[0], argv[1] = template and reads paths)"""
    o = {"parts": 60, "overlap": 0, "e": 0.30, "w": 150, "seq": None, "info": None}
    for i, a in enumerate(argv):
        if len(a) < 2 or a[0] != "-" or i + 1 >= len(argv):
            continue
        v = argv[i + 1]
        if a[1] == "o":
            o["seq"] = v
        elif a[1] == "r":
            o["info"] = v
        elif a[1] == "p":
            o["parts"] = int(v)
        elif a[1] == "l":
            o["overlap"] = int(v)
        elif a[1] == "w":
            o["w"] = int(v)
        elif a[1] == "e":
            o["e"] = float(v)
    return o


def run(template_name: str, templ_data: bytes, reads_data: bytes, args, cut_fn=None):
    """main() (RC:939-1112) on data: returns (stdout, Seq.fasta bytes, ReadSeqInfo bytes).  cut_fn(read) -> cut points
    replaces the checker's own FullAnalysis (the tests feed it other implementations)."""
    o = parse_args([template_name, "reads"] + list(args))
    pre = template_name[:-len("Template.fasta")] if template_name.endswith("Template.fasta") else ""
    out = [f"outputfile: {pre}Seq.fasta", f"readseqfile: {pre}ReadSeqInfo",
           "parts %d, overlap %d, wiggleroom %d, error_cutoff %f" % (o["parts"], o["overlap"], o["w"], o["e"])]
    recs, last = read_records(reads_data)
    n = len(recs)
    out.append(f"read count {n}")
    templ = read_template(templ_data)
    out.append(f"template length {len(templ)}")
    cut_fn = cut_fn or (lambda r: cut(templ, r, o["parts"], o["overlap"], o["e"]))
    written = recs[:-1] + [last] if n >= 2 else ([""] if n == 1 else [])
    cuts = [cut_fn(r) for r in recs[:n - 2]] + ([cut_fn(last)] * 2 if n >= 2 else [[]] * n)
    counts = [len(c) for c in cuts[:n - 1]] + [0] if n else []
    prozent = 5
    for i in range(n):
        if i * 100 // n > prozent:
            out.append(f"{prozent} % done.")
            prozent += 5
    out.append("Outputting results.")
    seq = "".join(write_record(r, c) for r, c in zip(written, cuts))
    info, k = [], 0
    for c in counts:
        info.append("".join(f"{k + t} " for t in range(c + 1)) + "\n")
        k += c + 1
    return "\n".join(out) + "\n", seq.encode(), "".join(info).encode()
