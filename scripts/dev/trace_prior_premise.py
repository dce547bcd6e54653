"""dev (GPU box):  with_lib.py <libpwr.so> scripts/dev/trace_prior_premise.py  -- the premise of the trace prior on the benchmark's own input (bench.py's default: tree_default, pipeline input, bandwidth
1000, window as bench.py leaves it for one GPU): every 50th row of the first three rounds is realigned on its own and its
Way / newcol are read back; all other rows go through realign_rows as in the benchmark."""
import sys, time
import numpy as np
from repeatresolver_amd import datagen as dg
from repeatresolver_amd.pipeline import initial_msa
from repeatresolver_amd.realigner import PWReAligner

cfg = dg.CONFIGS["tree_default"]
cfg = dg.SimConfig(**{**cfg.__dict__, "seed": 1})
rows, _ = initial_msa(cfg, device=0)
T = len(rows)
g = PWReAligner(rows, bandwidth=1000, device=0)
g.trim_ends()
g.total_score()
EVERY, C = 50, 32
print(f"# input: tree_default, pipeline input, seed 1: {T} rows x {len(rows[0])} columns, bandwidth 1000; every {EVERY}th row sampled", flush=True)
print("# round  rows  bases  kept(newcol==way, no column opened)  chunks_with_no_moved_row  runs_of_moved_rows_per_row  rows_per_run  moved_in_worst_chunk(mean)  median  rows_with_worst>24", flush=True)
for rnd in range(1, 4):
    t0 = time.time()
    nb = kept = nch = clean = nrun = nmoved = 0
    worst = []
    k = 0
    while k < T:
        nxt = min(T, (k // EVERY + 1) * EVERY) if k % EVERY else k
        if k % EVERY == 0:
            g.realign_row(k)
            d = g.debug_last_job()
            L = d["L"]
            if L > 0:
                way = np.array(d["way"], dtype=np.int64)
                nc = np.array(d["newcol"], dtype=np.int64)
                moved = nc != (way << 1)
                nb += L; kept += int((~moved).sum()); nmoved += int(moved.sum())
                pad = np.zeros((L + C - 1) // C * C, dtype=bool); pad[:L] = moved
                per = pad.reshape(-1, C).sum(1)
                nch += len(per); clean += int((per == 0).sum()); worst.append(int(per.max()))
                nrun += int(moved[0]) + int((moved[1:] & ~moved[:-1]).sum())
            k += 1
        else:
            g.realign_rows(k, nxt - k)
            k = nxt
    w = np.array(worst)
    print(f"round {rnd}: {len(w)} rows, {nb} bases, kept {100.0 * kept / nb:.1f} %, clean chunks {100.0 * clean / nch:.1f} %, "
          f"runs per row {nrun / len(w):.1f}, rows per run {nmoved / max(1, nrun):.2f}, worst chunk mean {w.mean():.1f} of {C}, median {np.median(w):.0f}, "
          f"rows with worst > 24: {100.0 * (w > 24).mean():.0f} %   ({time.time() - t0:.0f} s)", flush=True)
g.close()
