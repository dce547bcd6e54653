"""The front of the RepeatResolver pipeline as the reference chains it (RepeatResolver.c:150-230, README run order):
DataSimulator -> ReadCutter -> InitialAligner -> PW_ReAligner.  `initial_msa` produces what PW_ReAligner is really fed:
the simulated reads, cut to their repeat part, aligned into the template by the InitialAligner (on the GPU, include/pia.h)
and stacked by Building_MSA (IA:553-663)."""
import os
import shutil
import tempfile
import time

import numpy as np

from . import datagen as dg
from .initial_aligner import InitialAligner
from .strands import seeded_mask, turn


def initial_msa(cfg: dg.SimConfig, device: int = 0, cutoff: float = 0.30, both_strands: bool = False, reverse_seed=None):
    """Returns (rows, info): rows = the lines of the `<ds>_MSA` file InitialAligner writes for the data set `cfg` describes
    (reads whose repeat part is shorter than cfg.min_aligned bases are left out: ReadCutter's mapping would not find them).
    both_strands: the reads may lie on either strand (InitialAligner.align_strands); info["strands"] is the strand taken per
    read handed to InitialAligner and info["reverse"] their count.  The simulator only ever samples the template's strand;
    reverse_seed (an int) hands the reads over as a sequencer would, a seeded half of them as their reverse complement
    (strands.seeded_mask(len(reads), reverse_seed), info["turned"])."""
    t0 = time.time()
    seq, _full, _starts, _cids, cut, _ = dg.simulate_dataset(cfg)
    templ = dg.ASCII[seq].tobytes()
    reads = [dg.ASCII[r].tobytes() for r in cut if r is not None and len(r) >= cfg.min_aligned]
    mask = None
    if reverse_seed is not None:
        mask = seeded_mask(len(reads), reverse_seed)
        reads = turn(reads, mask)
    t1 = time.time()
    g = InitialAligner(templ, device=device)
    strands = None
    if both_strands:
        place, dist, strands, _other = g.align_strands(reads)
        reads = g.turned(reads, strands)
    else:
        place, dist = g.align(reads)
    st = g.stats()
    t2 = time.time()
    tmp = tempfile.mkdtemp(prefix="pia_msa_")
    try:
        msa_path, cls_path = os.path.join(tmp, "MSA"), os.path.join(tmp, "SeqClass")
        g.build_msa(msa_path, cls_path, reads, place, dist, cutoff)
        with open(msa_path, "rb") as f:
            rows = f.read().split(b"\n")
        with open(cls_path) as f:
            classes = f.read().split()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        g.close()
    if rows and rows[-1] == b"":
        rows.pop()
    info = {"reads": len(reads), "bases": sum(len(r) for r in reads), "template": len(templ), "rows": len(rows),
            "rejected_by_cutoff": classes.count("l"), "cells": st["cells"], "align_ms": st["last_align_ms"],
            "simulate_s": round(t1 - t0, 1), "align_s": round(t2 - t1, 2), "build_msa_s": round(time.time() - t2, 1)}
    if mask is not None:
        info["turned"] = mask
    if strands is not None:
        info["strands"] = [int(v) for v in strands]
        info["reverse"] = int(sum(info["strands"]))
    return rows, info


def _front_from_reads(cfg, device, cutoff, parts, overlap, error_cutoff, both_strands):
    """What initial_msa_from_reads and flank_labels both need: ReadCutter and InitialAligner on the full reads.  Returns
    (rows, info, pieces, piece_read, classes): the pieces as Seq.fasta holds them (not turned), the read of each
    (ReadSeqInfo) and its SeqClass letter."""
    from .flanks import read_info
    from .initial_aligner import _clean
    from .read_cutter import run_files
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="prc_msa_")
    try:
        dg.write_dataset(os.path.join(tmp, "ds"), cfg)
        templ_path = os.path.join(tmp, "dsTemplate.fasta")
        os.replace(os.path.join(tmp, "ds_Template.fasta"), templ_path)
        seq_path, rsi_path = os.path.join(tmp, "cut_Seq.fasta"), os.path.join(tmp, "cut_ReadSeqInfo")
        t1 = time.time()
        code, out = run_files(templ_path, os.path.join(tmp, "ds.fasta"), seq_path, rsi_path, parts=parts, overlap=overlap,
                              error_cutoff=error_cutoff, device=device, both_strands=both_strands)
        if code != 0:
            raise RuntimeError(f"ReadCutter failed ({code}): {out[-500:]}")
        t2 = time.time()
        with open(templ_path, "rb") as f:
            templ = _clean(b"".join(ln for ln in f.read().split(b"\n") if not ln.startswith(b">")))
        with open(seq_path, "rb") as f:
            reads = [_clean(r) for r in f.read().split(b">")[1:]]
        pieces, piece_read = reads, read_info(rsi_path, len(reads))
        g = InitialAligner(templ, device=device)
        strands = None
        try:
            if both_strands:
                place, dist, strands, _other = g.align_strands(reads)
                reads = g.turned(reads, strands)
            else:
                place, dist = g.align(reads)
            st = g.stats()
            t3 = time.time()
            msa_path, cls_path = os.path.join(tmp, "MSA"), os.path.join(tmp, "SeqClass")
            g.build_msa(msa_path, cls_path, reads, place, dist, cutoff)
        finally:
            g.close()
        with open(msa_path, "rb") as f:
            rows = f.read().split(b"\n")
        with open(cls_path) as f:
            classes = f.read().split()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if rows and rows[-1] == b"":
        rows.pop()
    info = {"pieces": len(reads), "bases": sum(len(r) for r in reads), "template": len(templ), "rows": len(rows),
            "rejected_by_cutoff": classes.count("l"), "cells": st["cells"], "write_dataset_s": round(t1 - t0, 1),
            "read_cutter_s": round(t2 - t1, 2), "align_s": round(t3 - t2, 2), "build_msa_s": round(time.time() - t3, 1)}
    if strands is not None:
        info["strands"] = [int(v) for v in strands]
        info["reverse"] = int(sum(info["strands"]))
    return rows, info, pieces, piece_read, classes


def initial_msa_from_reads(cfg: dg.SimConfig, device: int = 0, cutoff: float = 0.30, parts: int = 60, overlap: int = 0,
                           error_cutoff: float = 0.30, both_strands: bool = False):
    """The reference pipeline's own way in, from the *full* reads (no ground truth): writes the data set's reads FASTA
    (datagen.write_dataset), runs the ReadCutter drop-in on it (GPU), then InitialAligner (GPU) on the Seq.fasta it wrote.
    Returns (rows, info) like initial_msa.  both_strands: ReadCutter looks for its cut points in both orientations of every
    read (`-b 1`) and InitialAligner takes each piece on the strand it aligns on; info["strands"] is the strand per piece."""
    return _front_from_reads(cfg, device, cutoff, parts, overlap, error_cutoff, both_strands)[:2]


def flank_labels(cfg: dg.SimConfig, device: int = 0, cutoff: float = 0.30, parts: int = 60, overlap: int = 0,
                 error_cutoff: float = 0.30, both_strands: bool = False, *, max_permille, reach: int = 256, min_len: int = 100,
                 min_size: int = 1):
    """initial_msa_from_reads, and what the connection of the windows lacks at both ends: the labelling of the rows by the
    unique sequence left and right of them, from ReadCutter's own pieces (flanks.flank_labels on the GPU; no ground truth).
    Returns (rows, info, left, right): left[t] / right[t] = the cluster of row t's flank on that side or -1, the shape
    resolution.connect takes in front of and behind the windows' labellings.  info gains "pieces_list", "piece_read" and
    "classes": the pieces as Seq.fasta holds them, the read of each and its SeqClass letter.  max_permille has no default."""
    from .flanks import flank_labels as labels_of
    rows, info, pieces, piece_read, classes = _front_from_reads(cfg, device, cutoff, parts, overlap, error_cutoff, both_strands)
    left, right = labels_of(pieces, piece_read, classes, info.get("strands"), max_permille=max_permille, reach=reach,
                            min_len=min_len, min_size=min_size, device=device)
    info.update(pieces_list=pieces, piece_read=piece_read, classes=classes)
    return rows, info, left, right


def refined_groups(rows, von=None, bis=None, cov: int = 30, cutoff: float = 0.0, device: int = 0):
    """The back of the chain: MaxCorrelation on the realigned MSA `rows` (MC:839-905), then RepeatResolver's group
    refinement on the window [von, bis] (RR:3948-4024).  Returns group_refinement.RefinedGroups."""
    from .group_refinement import refine_groups
    from .max_correlation import max_correlations
    return refine_groups(rows, max_correlations(rows, cov, device), von, bis, cov, cutoff, device)


def subdivided(rows, von=None, bis=None, cov: int = 30, cutoff: float = 0.0, device: int = 0):
    """refined_groups, then RepeatResolver's two drop-off subdivisions of the window's rows (RR:4026-4062).  Returns
    subdivision.Subdivision: per input row its part after each stage (-1: the row does not span the window)."""
    from .subdivision import subdivide
    return subdivide(rows, refined_groups(rows, von, bis, cov, cutoff, device), von, bis, cov, device)


def clustered(rows, von=None, bis=None, cov: int = 30, cutoff: float = 0.0, device: int = 0):
    """subdivided, then RepeatResolver's k-means subdivision (RR:4064-4075): the whole tool.  Returns (subdivision.Subdivision,
    kmeans_subdivision.KmeansSubdivision); the second's labels are the final partition of the rows into repeat copies."""
    from .kmeans_subdivision import kmeans_subdivide
    from .subdivision import subdivide
    refined = refined_groups(rows, von, bis, cov, cutoff, device)
    sub = subdivide(rows, refined, von, bis, cov, device)
    return sub, kmeans_subdivide(rows, refined, sub, von, bis, cov, device)


def _resolved(rows, parts, coverage, cov, cutoff, device, copies, recruit=None, settle=None, thread=None):
    from .max_correlation import max_correlations
    from .resolution import assign, connect, consensus, crossovers, open_msa, resolve
    from .resolution import settle as settle_labels
    from .resolution import thread as thread_labels
    from .window import window_boundaries
    assert not (recruit and settle)                                    # `assigned` or `settled`, one of them: each has its own return below
    sites = window_boundaries(rows, coverage, parts)
    mc = max_correlations(rows, cov, device)
    with open_msa(rows, device) as msa:
        windows = resolve(msa, mc, sites, cov, cutoff)
        cons = [consensus(msa, w.kmeans_labels, w.von, w.bis, mc, w.cutoff) if w.kept_rows > 0 else None
                for w in windows] if copies else None
        assignments = [None if c is None else assign(msa, c) for c in cons] if recruit else None
        settlements = [settle_labels(msa, w.kmeans_labels, w.von, w.bis, mc, w.cutoff, **settle) if w.kept_rows > 0 else None
                       for w in windows] if settle else None
        settled_labels = [w.kmeans_labels.copy() if s is None else s.labels for w, s in zip(windows, settlements)] if settle else None
        threads = whole = cross = None
        if thread and len(windows) > 1:                                # the whole copies, while the MSA is still on the device
            ends = thread.get("flanks")                                # `loci`: the flank labellings in front and behind
            threads = thread_labels(settled_labels if ends is None else [ends[0], *settled_labels, ends[1]])
            whole_labels = threads.labels()
            if (whole_labels >= 0).any() and ends is not None:         # the copies over the full width, flank to flank
                whole = consensus(msa, whole_labels, None, None, mc, min(w.cutoff for w in windows))
            elif (whole_labels >= 0).any():
                whole = consensus(msa, whole_labels, sites[0], sites[-1], mc, min(w.cutoff for w in windows))
                cut = dict(segments=thread["segments"]) if thread["segments"] is not None else dict(segment_sites=sites[:-1])
                cross = crossovers(msa, whole, min_side=thread["min_side"], **cut)
    con = connect([w.kmeans_labels for w in windows]) if len(windows) > 1 else None
    if settle:
        settled = sites, windows, con, cons, settlements, connect(settled_labels) if len(windows) > 1 else None
        return settled + (threads, whole, cross) if thread else settled
    if not recruit:
        return sites, windows, con, cons
    recruited = [w.kmeans_labels.copy() if a is None else a.labels(*recruit, keep=w.kmeans_labels) for w, a in zip(windows, assignments)]
    return sites, windows, con, cons, assignments, recruited, connect(recruited) if len(windows) > 1 else None


def resolved(rows, parts: int = 6, coverage: float = 0.90, cov: int = 30, cutoff: float = 0.0, device: int = 0):
    """The whole repeat as the reference README runs it: MaxCorrelation, Window.py's boundaries (`parts` windows over the
    columns covered by at least `coverage` of the mean), RepeatResolver on every window [b_p, b_{p+1}] from one device copy
    of the MSA, and the connection of the windows' k-means labellings.  Returns (boundaries, [resolution.ResolvedWindow],
    resolution.Connection or None for a single window)."""
    return _resolved(rows, parts, coverage, cov, cutoff, device, False)[:3]


def resolved_copies(rows, parts: int = 6, coverage: float = 0.90, cov: int = 30, cutoff: float = 0.0, device: int = 0):
    """resolved, and what a repeat is resolved for: the sequence of every copy.  Returns resolved's three values and a list with
    one resolution.Consensus per window (None for a window that keeps no row), made from the same device copy of the MSA for the
    window's k-means labels: resolution.consensus(msa, w.kmeans_labels, w.von, w.bis, maxcorrs, w.cutoff), the selected columns
    being those over the cutoff the window was resolved with (RR:3977).  Consensus.sequences() and resolution.write_copies
    turn it into sequences."""
    return _resolved(rows, parts, coverage, cov, cutoff, device, True)


def assigned(rows, parts: int = 6, coverage: float = 0.90, cov: int = 30, cutoff: float = 0.0, device: int = 0, *, min_compared,
             min_margin):
    """resolved_copies, and the way back from the copies to the reads.  A window's k-means labelling covers only the rows that
    span it; here every row of the MSA is compared with the window's per-copy consensus (resolution.assign, from the same
    device copy of the MSA, over the window's selected columns at which every copy has a consensus).  Returns resolved_copies'
    four values and
      * a list with one resolution.Assignment per window (None where the window has no consensus),
      * the recruited labellings a.labels(min_compared, min_margin, keep=w.kmeans_labels): the rows of the k-means labelling
        keep their label, a row outside it joins the copy it is nearest to where it has at least min_compared compared columns
        and the second nearest copy is at least min_margin mismatches further away (a window without an Assignment keeps its
        k-means labelling),
      * the resolution.Connection of the recruited labellings (None for a single window).
    The two thresholds depend on the read error rate and the number of selected columns: they have no default."""
    return _resolved(rows, parts, coverage, cov, cutoff, device, True, (min_compared, min_margin))


def settled(rows, parts: int = 6, coverage: float = 0.90, cov: int = 30, cutoff: float = 0.0, device: int = 0, *, min_compared,
            min_margin, max_iter, hold: bool = True):
    """resolved_copies, and every window's k-means labelling settled: `assigned` makes one pass from the copies to the reads and
    the recruited rows never feed back into the consensus they were judged against; here the loop runs until nothing moves
    (resolution.settle, on the device, from the same device copy of the MSA: the window's k-means labels over [w.von, w.bis],
    the selected columns being those over w.cutoff).  Returns resolved_copies' four values and
      * a list with one resolution.Settlement per window (None for a window that keeps no row),
      * the resolution.Connection of the settled labellings (None for a single window; a window without a Settlement stands
        there with its k-means labelling).
    hold (the default here): the rows of the k-means labelling keep their label, as in `assigned`; with max_iter = 1 the settled
    labellings are `assigned`'s recruited ones.  The thresholds and max_iter have no default."""
    return _resolved(rows, parts, coverage, cov, cutoff, device, True,
                     settle=dict(min_compared=min_compared, min_margin=min_margin, max_iter=max_iter, hold=hold))


def threaded(rows, parts: int = 6, coverage: float = 0.90, cov: int = 30, cutoff: float = 0.0, device: int = 0, *, min_compared,
             min_margin, max_iter, hold: bool = True, min_side, segments=None):
    """settled, and the windows' settled labellings turned into whole copies, from the same device copy of the MSA.  Returns
    settled's six values and
      * the resolution.Threads of the settled labellings (resolution.thread): a label of one window and a label of the next are
        linked where each is the other's first largest partner by shared rows, and a thread is a maximal chain of links,
      * the resolution.Consensus of Threads.labels() -- every row whose labels all lie on one thread that spans all windows --
        over [sites[0], sites[-1]], the selected columns being those over the smallest cutoff of the windows: the sequence of
        every whole copy,
      * the resolution.Crossovers of every row of the MSA against those whole copies (resolution.crossovers), the segments being
        the windows (segment_sites = sites[:-1]) or, with `segments`, that many of equally many compared columns: the rows that
        follow one copy up to a boundary and another behind it -- chimeric reads, misjoined rows, or two clusters joined
        wrongly between windows -- are Crossovers.rows(min_gain).
    A single window returns None for all three, no thread that spans all windows None for the last two.  min_side has no
    default, like the other thresholds."""
    return _resolved(rows, parts, coverage, cov, cutoff, device, True,
                     settle=dict(min_compared=min_compared, min_margin=min_margin, max_iter=max_iter, hold=hold),
                     thread=dict(min_side=min_side, segments=segments))


def loci(rows, left, right, left_fc, right_fc, parts: int = 6, coverage: float = 0.90, cov: int = 30, cutoff: float = 0.0,
         device: int = 0, *, min_compared, min_margin, max_iter, hold: bool = True, min_depth: int = 1):
    """threaded with the two flank labellings (flank_labels' left and right, one label per row) in front of and behind the
    settled ones, and every whole copy put back between its unique flanks.  Returns settled's six values and
      * the resolution.Threads of [left, *settled labellings, right],
      * the resolution.Consensus of Threads.labels() over the full width of the MSA (None where no thread spans from flank to
        flank),
      * the list of resolution.Locus that resolution.join_loci makes of them with left_fc and right_fc, the
        flanks.FlankConsensus of the two sides (flanks.flank_sequences): left flank + copy + right flank per whole copy, the
        copy over the columns of depth >= min_depth.
    No crossovers are looked for here: `threaded` does that, between the windows alone."""
    from .resolution import join_loci
    left, right = np.asarray(left, dtype=np.int32), np.asarray(right, dtype=np.int32)
    if left.shape != (len(rows),) or right.shape != (len(rows),):
        raise ValueError("one left and one right label per row")
    out = _resolved(rows, parts, coverage, cov, cutoff, device, True,
                    settle=dict(min_compared=min_compared, min_margin=min_margin, max_iter=max_iter, hold=hold),
                    thread=dict(min_side=None, segments=None, flanks=(left, right)))
    threads, whole = out[6], out[7]
    return out[:8] + ([] if whole is None else join_loci(threads, whole, left_fc, right_fc, min_depth),)


def anchored(rows, left, right, left_fc, right_fc, contigs, parts: int = 6, coverage: float = 0.90, cov: int = 30, cutoff: float = 0.0,
             device: int = 0, *, min_compared, min_margin, max_iter, hold: bool = True, min_depth: int = 1, anchor_permille, max_span,
             reach: int = 256, min_len: int = 100):
    """loci, and where its loci belong in an assembly (anchors.place_loci on the GPU: the `reach` bases of every locus's flanks
    nearest to the repeat, searched in `contigs` in both orientations).  Returns loci's nine values and
      * the anchors.Hits of the 2 n flank patterns (anchors.locus_patterns: 2 i is locus i's left flank, 2 i + 1 its right),
      * the list of anchors.Placement, one per locus: anchors.patch(contigs, placements, copies) is the patched assembly.
    anchor_permille (the search's max_permille) and max_span have no default."""
    from .anchors import place_loci
    out = loci(rows, left, right, left_fc, right_fc, parts, coverage, cov, cutoff, device, min_compared=min_compared,
               min_margin=min_margin, max_iter=max_iter, hold=hold, min_depth=min_depth)
    return out + place_loci(out[8], contigs, max_permille=anchor_permille, max_span=max_span, reach=reach, min_len=min_len, device=device)
