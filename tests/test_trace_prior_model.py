"""CPU: a plain-Python model of k_trace_blk's pass over one chunk, with and without the prior.

A step of the trace is a function of (row, column): from arrival column y in row x, clamp y to the band's end, go left to the
first column whose A bit is clear, read the C bit there (1: diagonal, leave one column to the left; 0: 'up', stay).  The
prior of row x < L - 1 says: arrive in Way[x+1] - 1, find Way[x], step diagonally.  `intact[x]` is whether the record agrees,
worked out per row from at most LOOK columns; a pass that arrives at an intact row in its prior's column records the whole
run of intact rows below it at once.  The model restates both walks and holds them to each other: every recorded
(newcol, arrival), the 'up' count of the chunk's word, the exit column, the error, the rows recorded -- from every arrival
column, for a first pass and for a retrace that may merge into the first pass's record; and whole traces, chunk by chunk."""
import numpy as np
import pytest

TB_C, LOOK = 32, 8


class Rec:
    """A record: Way[], the A / C bits of every (row, column), the band."""

    def __init__(self, way, A, C, W, B, H):
        self.way, self.A, self.C, self.W, self.B, self.H, self.L = [int(w) for w in way], A, C, W, B, H, len(way)
        # left[x][c]: the highest column <= c whose A bit is clear (-1: none)
        idx = np.where(A == 0, np.arange(W)[None, :], -1)
        self.left = np.maximum.accumulate(idx, axis=1)

    def step(self, x, y):
        """-> (err, found, cbit); err 1: arrival left of the band, 2: no clear A bit down to the band's start"""
        a = max(0, self.way[x] - self.H)
        if y < a:
            return 1, 0, 0
        yc = min(y, a + min(self.B, self.W - a) - 1)
        f = int(self.left[x][yc]) if yc >= 0 else -1
        if f < a:
            return 2, 0, 0
        return 0, f, int(self.C[x][f])

    def intact(self, x):
        """the kernel's per-lane test, from the words of the row's own columns alone"""
        if x >= self.L - 1:
            return False
        w, ya = self.way[x], self.way[x + 1] - 1
        af = max(0, w - self.H)
        ycf = min(ya, af + min(self.B, self.W - af) - 1)
        if not (ya >= af and ycf >= w and ycf - w < LOOK and (w >= 1 or x == 0)):
            return False
        if self.A[x][w] != 0 or self.C[x][w] != 1:
            return False
        return all(self.A[x][w + k] == 1 for k in range(1, ycf - w + 1))


class Chunk:
    """The state a wave of k_trace_blk keeps for its chunk, and its pass."""

    def __init__(self, rec, c, prior):
        self.r, self.prior = rec, prior
        self.x_lo, self.x_top = c * TB_C, min(rec.L, c * TB_C + TB_C) - 1
        self.nc, self.yi = {}, {}
        self.xrec_lo = self.x_top + 1
        self.cnt_steps = 0                                  # kept step by step, as the kernel did before the prior
        self.yexit = 0
        self.mask = [prior and rec.intact(x) for x in range(self.x_lo, self.x_lo + TB_C)]

    def ups(self):
        """what the word carries now: a count over the recorded rows"""
        return sum(self.nc.get(x, 0) & 1 for x in range(self.xrec_lo, self.x_top + 1))

    def passs(self, y0, check_merge):
        r, x, y, e, merged = self.r, self.x_top, y0, 0, False
        while x >= self.x_lo and not e:
            if check_merge and x >= self.xrec_lo and self.yi[x] == y:
                merged = True
                break
            l = x - self.x_lo
            if self.mask[l] and y == r.way[x + 1] - 1:
                l0 = l
                while l0 > 0 and self.mask[l0 - 1]:
                    l0 -= 1
                for xx in range(self.x_lo + l0, x + 1):
                    if xx >= self.xrec_lo:
                        self.cnt_steps -= self.nc[xx] & 1
                    self.nc[xx], self.yi[xx] = r.way[xx] << 1, r.way[xx + 1] - 1
                y, x = r.way[self.x_lo + l0] - 1, self.x_lo + l0 - 1
                assert y >= 0 or x < 0
                continue
            e, f, cb = r.step(x, y)
            if e:
                break
            nv = (f << 1) | (cb ^ 1)
            if x >= self.xrec_lo:
                self.cnt_steps -= self.nc[x] & 1
            self.cnt_steps += nv & 1
            self.nc[x], self.yi[x] = nv, y
            y, x = f - cb, x - 1
            if x >= 0 and y < 0:
                e = 3
        if not merged:
            self.xrec_lo = min(self.xrec_lo, x + 1) if e else self.x_lo
        if not e and not merged:
            self.yexit = y
        return e, merged

    def state(self):
        rows = range(self.xrec_lo, self.x_top + 1)
        return ([(self.nc[x], self.yi[x]) for x in rows], self.xrec_lo, self.yexit, self.ups())


def make(L, kind, seed, H=40, gaps=None, broken=()):
    """kind 'all': every prior holds; 'none': none does; 'singles': all but the rows in `broken`; 'random': a random record.
    gaps: {row: columns between Way[row] and Way[row + 1]} (default: 1 .. 7, about 4.5 on average)."""
    rng = np.random.default_rng(seed)
    gap = rng.choice([1, 2, 3, 4, 5, 6, 7, 7, 6, 5], size=L)
    for x, g in (gaps or {}).items():
        gap[x] = g
    way = np.zeros(L, dtype=np.int64)
    way[0] = 3
    for x in range(1, L):
        way[x] = way[x - 1] + gap[x - 1]
    W, B = int(way.max()) + 12, 2 * H
    A = (rng.random((L, W)) < 0.7).astype(np.uint8)
    C = (rng.random((L, W)) < 0.6).astype(np.uint8)
    if kind != "random":
        for x in range(L - 1):
            w, nx = int(way[x]), int(way[x + 1])
            if kind == "none" or (kind == "singles" and x in broken):
                if rng.random() < 0.5:
                    A[x][w] = 1                                 # the row's base moves left
                else:
                    A[x][w], C[x][w] = 0, 0                     # ... or a column is opened
            elif nx > w:
                A[x][w], C[x][w] = 0, 1
                A[x][w + 1:min(nx, W)] = 1
    return Rec(way, A, C, W, B, H)


def _compare_chunks(rec, retrace_span=6):
    nch = (rec.L + TB_C - 1) // TB_C
    for c in range(nch):
        top = c == nch - 1
        guess = rec.W - 1 if top else rec.way[min(rec.L - 1, c * TB_C + TB_C)] - 1
        for y0 in range(0, rec.W):
            res = []
            for prior in (False, True):
                ch = Chunk(rec, c, prior)
                e, _ = ch.passs(y0, False)
                assert ch.cnt_steps == ch.ups()
                res.append((e,) + ch.state())
            assert res[0] == res[1], (c, y0)
        # a retrace that may merge, after a first pass from the guess
        for y1 in range(max(0, guess - retrace_span), min(rec.W, guess + retrace_span)):
            res = []
            for prior in (False, True):
                ch = Chunk(rec, c, prior)
                e0, _ = ch.passs(guess, False)
                e1, merged = ch.passs(y1, True)
                assert ch.cnt_steps == ch.ups()
                # (a walk that takes a run may pass the row the other one merges in: it then re-derives the same record, and its
                # exit is the one the first pass left)
                broke = bool(e1) or ch.xrec_lo > ch.x_lo
                res.append((broke,) + ch.state()[:2] + (None if broke else ch.yexit, ch.ups()))
            assert res[0] == res[1], (c, y1)


def _whole_trace(rec, prior, entry):
    """all chunks the way the launch settles them: the top one from the entry, every other from its guess and then, where
    the chunk above leaves in another column, again from there"""
    nch = (rec.L + TB_C - 1) // TB_C
    out, arr = {}, entry
    for c in range(nch - 1, -1, -1):
        ch = Chunk(rec, c, prior)
        if c == nch - 1:
            e, _ = ch.passs(arr, False)
        else:
            e, _ = ch.passs(rec.way[ch.x_top + 1] - 1, False)
            if rec.way[ch.x_top + 1] - 1 != arr:
                e, merged = ch.passs(arr, True)
                if merged and ch.xrec_lo > ch.x_lo:
                    e = 6
        if e or ch.xrec_lo > ch.x_lo:
            return out, ("err", c)
        for x in range(ch.x_lo, ch.x_top + 1):
            out[x] = (ch.nc[x], ch.yi[x])
        out[("cnt", c)] = ch.ups()
        arr = ch.yexit
    return out, arr


def _serial_trace(rec, entry):
    out, y = {}, entry
    cnt = {}
    for x in range(rec.L - 1, -1, -1):
        e, f, cb = rec.step(x, y)
        if e:
            return out, ("err", x // TB_C)
        out[x] = ((f << 1) | (cb ^ 1), y)
        cnt[x // TB_C] = cnt.get(x // TB_C, 0) + (cb ^ 1)
        y = f - cb
        if x > 0 and y < 0:
            return out, ("err", (x - 1) // TB_C)
    for c in range((rec.L + TB_C - 1) // TB_C):
        out[("cnt", c)] = cnt.get(c, 0)
    return out, y


LENGTHS = [31, 32, 33, 97, 130]


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("kind", ["all", "none", "singles", "random"])
def test_pass_with_runs_equals_serial_pass(L, kind):
    # single rows out: around the chunk boundaries (a run that ends on one, a run that starts under one) and around the
    # 16-row group boundaries
    broken = {x for x in (0, 15, 16, 31, 32, 47, 63, 64, 65, 80, 96, 111, 128) if x < L - 1}
    rec = make(L, kind, seed=L, broken=broken)
    n = sum(rec.intact(x) for x in range(L))
    if kind == "all":
        assert n == L - 1                                   # (row L - 1 has no prior)
    elif kind == "none":
        assert n == 0
    elif kind == "singles":
        assert n == L - 1 - len(broken)
    _compare_chunks(rec)


@pytest.mark.parametrize("L", LENGTHS)
def test_gaps_at_the_look_and_one_beyond(L):
    """A row whose base above sits LOOK columns away is the last the prior covers (it reads Way[x] .. Way[x] + LOOK - 1);
    one column more and the row is 'not intact' although its record agrees -- it is stepped, with the same result."""
    gaps = {5: LOOK, 6: LOOK + 1, 14: LOOK, 15: LOOK + 1, 20: 2 * LOOK, L - 2: LOOK + 1}
    if L > 40:
        gaps.update({31: LOOK, 32: LOOK + 1, 47: LOOK + 1, 64: LOOK})
    rec = make(L, "all", seed=100 + L, gaps=gaps)
    for x, g in gaps.items():
        assert rec.intact(x) == (g <= LOOK), (x, g)
    _compare_chunks(rec)


@pytest.mark.parametrize("L", LENGTHS)
def test_arrival_past_the_band_end_and_left_of_its_start(L):
    """A narrow band (B = 2 H = 6): the prior of row 9 arrives past the band's end (clamped, implicit moves to the left: still
    intact where the record agrees under the clamp); row 20 stands so far right of the row above it that its prior arrives left
    of the band's start (never intact; a walk that gets there reports it as ever)."""
    H = 3
    rec = make(L, "all", seed=200 + L, H=H, gaps={x: 1 + (x % 3) for x in range(L)} | {9: 5})
    assert rec.way[10] - 1 > rec.way[9] + H - 1 and rec.intact(9)
    rec.way[20] = rec.way[21] + H + 2
    rec = Rec(rec.way, rec.A, rec.C, rec.W, rec.B, rec.H)
    assert rec.way[21] - 1 < rec.way[20] - H and not rec.intact(20)
    _compare_chunks(rec, retrace_span=4)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("kind", ["all", "singles", "random"])
def test_whole_trace_chunk_by_chunk(L, kind):
    broken = {x for x in (3, 15, 31, 32, 40, 64, 70, 96) if x < L - 1}
    rec = make(L, kind, seed=300 + L, broken=broken)
    for entry in range(rec.way[-1] - 2, rec.W):
        exp = _serial_trace(rec, entry)
        for prior in (False, True):
            got = _whole_trace(rec, prior, entry)
            if isinstance(exp[1], tuple):                   # the trace breaks off: so does the chunked one
                assert isinstance(got[1], tuple), (entry, prior)
            else:
                assert got == exp, (entry, prior)
