"""ctypes loader for csrc/libpwr.so (the C ABI of include/pwr.h).  There is no fallback: if the
HIP library is missing the import of the product path fails loudly."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpwr.so")


class PwrStats(ctypes.Structure):
    _fields_ = [("cells_reference", ctypes.c_uint64), ("cells_computed", ctypes.c_uint64),
                ("fill_launches", ctypes.c_uint64), ("fill_ms", ctypes.c_double),
                ("rows_committed", ctypes.c_uint64), ("rows_recomputed", ctypes.c_uint64),
                ("batches", ctypes.c_uint64), ("rows_changed", ctypes.c_uint64),
                ("reject_reason", ctypes.c_uint64 * 4), ("fill_launches_timed", ctypes.c_uint64),
                ("stalls", ctypes.c_uint64), ("rows_ahead", ctypes.c_uint64), ("rows_wide", ctypes.c_uint64),
                ("seg_jobs", ctypes.c_uint64), ("segs", ctypes.c_uint64), ("seg_fails", ctypes.c_uint64),
                ("rows_jumped", ctypes.c_uint64)]


# every symbol include/pwr.h declares
EXPORTS = ["pwr_create", "pwr_destroy", "pwr_trim_ends", "pwr_realign_row", "pwr_realign_round", "pwr_realign_rows",
           "pwr_total_score", "pwr_dims", "pwr_export_rows", "pwr_set_option", "pwr_get_option", "pwr_get_stats",
           "pwr_reset_stats", "pwr_strerror", "pwr_device_count", "pwr_read_msa_file",
           "pwr_write_msa_file", "pwr_run_file", "pwr_split_begin", "pwr_split_slot_bytes", "pwr_split_stage", "pwr_split_commit",
           "pwr_snapshot_begin", "pwr_snapshot_wait", "pwr_snapshot_free"]

# every symbol include/pia.h declares (the InitialAligner)
PIA_EXPORTS = ["pia_create", "pia_destroy", "pia_align", "pia_get_stats", "pia_set_option", "pia_get_timing", "pia_read_template", "pia_read_fasta",
               "pia_build_msa", "pia_run_files", "pia_align_strands", "pia_turn", "pia_run_files_strands"]

# every symbol include/prc.h declares (the ReadCutter, the pipeline's first tool)
PRC_EXPORTS = ["prc_create", "prc_destroy", "prc_occurrences", "prc_cut", "prc_get_stats", "prc_free", "prc_read_template",
               "prc_read_fasta", "prc_scan_dense", "prc_scan_runs", "prc_select_cuts", "prc_write_seq", "prc_write_info",
               "prc_run_files", "prc_occurrences_strands", "prc_cut_strands", "prc_merge_cuts", "prc_run_files_strands"]

# every symbol include/pmc.h declares (MaxCorrelation)
PMC_EXPORTS = ["pmc_maxcorrs", "pmc_last_timing", "pmc_read_msa", "pmc_write", "pmc_run_file", "pmc_tail_probe"]

# every symbol include/pgr.h declares (RepeatResolver's group refinement)
PGR_EXPORTS = ["pgr_refine", "pgr_free", "pgr_last_timing", "pgr_read_window", "pgr_window_free", "pgr_slice_maxcorrs",
               "pgr_read_maxcorrs_file", "pgr_default_cutoff", "pgr_restrict_coverage", "pgr_subdivide", "pgr_subdivision_free",
               "pgr_last_subdivision_timing", "pgr_dropoff_subdivision", "pgr_compress_labels", "pgr_complete_labels",
               "pgr_write_subdivision", "pgr_subdivision_name", "pgr_kmeans_subdivide", "pgr_kmeans_free", "pgr_kmeans_subdivide_pairs",
               "pgr_last_kmeans_timing", "pgr_kmeans_reassign", "pgr_msa_open", "pgr_msa_close", "pgr_msa_window", "pgr_msa_resolve",
               "pgr_resolution_free", "pgr_last_resolve_timing", "pgr_connect", "pgr_connection_free", "pgr_msa_consensus",
               "pgr_consensus_free", "pgr_last_consensus_timing", "pgr_resolvability", "pgr_msa_assign", "pgr_assignment_free",
               "pgr_last_assign_timing", "pgr_msa_settle", "pgr_settlement_free", "pgr_last_settle_timing", "pgr_tail_probe",
               "pgr_km_tail_probe", "pgr_msa_crossovers", "pgr_crossovers_free", "pgr_last_crossover_timing", "pgr_thread",
               "pgr_threads_free"]

# every symbol include/pfl.h declares (the flank labellings)
PFL_EXPORTS = ["pfl_create", "pfl_destroy", "pfl_neighbours", "pfl_distances", "pfl_cluster", "pfl_get_stats", "pfl_labels",
               "pfl_read_info", "pfl_free", "pfl_write_labels", "pfl_run_files", "pfl_place", "pfl_set_scratch_limit",
               "pfl_get_place_stats", "pfl_consensus", "pfl_consensus_free", "pfl_consensus_pack", "pfl_call", "pfl_write_flank_fasta",
               "pfl_run_files_consensus"]
PFL_MAX_REACH = 512
PFL_MAX_FLANKS = 30000
PFL_MAX_EXTENT = 8192


class PflConsensusResult(ctypes.Structure):
    """pfl_consensus_result (include/pfl.h)"""
    _fields_ = [("nclusters", ctypes.c_int), ("label", ctypes.POINTER(ctypes.c_int)), ("members", ctypes.POINTER(ctypes.c_int)),
                ("backbone", ctypes.POINTER(ctypes.c_int)), ("off", ctypes.POINTER(ctypes.c_longlong)), ("seq", ctypes.c_void_p),
                ("depth", ctypes.POINTER(ctypes.c_int))]

# every symbol include/pla.h declares (the locus anchorer)
PLA_EXPORTS = ["pla_create", "pla_destroy", "pla_open_text", "pla_close_text", "pla_set_option", "pla_search", "pla_hits_free",
               "pla_get_stats", "pla_read_contigs", "pla_contigs_free", "pla_read_loci", "pla_loci_free", "pla_place",
               "pla_status_name", "pla_write_placements", "pla_write_patched", "pla_run_files"]
PLA_MAX_REACH = 512
PLA_MAX_HITS = 1 << 22
PLA_MAX_PATTERNS = 65536
PLA_RUN_CAP = 4
PLA_STATUS_NAMES = ("NONE", "AMBIGUOUS", "LEFT_ONLY", "RIGHT_ONLY", "PLACED", "BRIDGE", "INCONSISTENT", "CONFLICT")
PLA_NONE, PLA_AMBIGUOUS, PLA_LEFT_ONLY, PLA_RIGHT_ONLY, PLA_PLACED, PLA_BRIDGE, PLA_INCONSISTENT, PLA_CONFLICT = range(8)


class PlaHits(ctypes.Structure):
    """pla_hits (include/pla.h)"""
    _fields_ = [("n", ctypes.c_int)] + [(name, ctypes.POINTER(ctypes.c_int)) for name in
                                        ("pattern", "orientation", "contig", "boundary", "lo", "hi", "distance")]


class PlaContigs(ctypes.Structure):
    """pla_contigs"""
    _fields_ = [("nc", ctypes.c_int), ("name", ctypes.POINTER(ctypes.c_char_p)), ("off", ctypes.POINTER(ctypes.c_longlong)),
                ("bases", ctypes.c_void_p)]


class PlaLoci(ctypes.Structure):
    """pla_loci"""
    _fields_ = [("n", ctypes.c_int), ("name", ctypes.POINTER(ctypes.c_char_p)), ("left_len", ctypes.POINTER(ctypes.c_int)),
                ("copy_len", ctypes.POINTER(ctypes.c_int)), ("right_len", ctypes.POINTER(ctypes.c_int)),
                ("off", ctypes.POINTER(ctypes.c_longlong)), ("seq", ctypes.c_void_p), ("aoff", ctypes.POINTER(ctypes.c_longlong)),
                ("anchored", ctypes.c_void_p), ("side", ctypes.POINTER(ctypes.c_int))]


class PlaPlacement(ctypes.Structure):
    """pla_placement"""
    _fields_ = [(name, ctypes.c_int) for name in
                ("status", "left_hits", "right_hits", "left_contig", "left_orientation", "left_boundary", "left_distance",
                 "right_contig", "right_orientation", "right_boundary", "right_distance", "lo", "hi", "has_span", "span")]


# constants of include/pgr.h that tests and scripts cite (pgr_cons_device.hip)
PGR_MAX_ROWS = 30000
PGR_CS_TILE = 1024            # window columns per work-group of k_cs_counts
PGR_CS_ROWS = 255             # rows of one part per work-group
PGR_CS_SCRATCH_INTS = 1 << 25  # count entries on the device at a time: a wider window goes through in column ranges
# (pgr_assign_device.hip)
PGR_AS_SCRATCH_BYTES = 64 << 20  # planes and mismatch matrix of one range of rows: more rows go through in several ranges
PGR_AS_TILE = 8               # parts per work-group of k_as_dist
# (pgr_settle_device.hip) pgr_settlement.stop
PGR_ST_CONVERGED, PGR_ST_MAX_ITER, PGR_ST_EMPTY, PGR_ST_NO_COLUMN = 0, 1, 2, 3
PGR_ST_NAMES = ("CONVERGED", "MAX_ITER", "EMPTY", "NO_COLUMN")
# (pgr_cross_device.hip)
PGR_CX_MAX_SEGMENTS = 1024    # most segments of one pgr_msa_crossovers


class PgrWindow(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("kept_rows", ctypes.c_int), ("von", ctypes.c_int), ("bis", ctypes.c_int),
                ("width", ctypes.c_int), ("sc", ctypes.c_int), ("kept", ctypes.POINTER(ctypes.c_ubyte)),
                ("groups", ctypes.POINTER(ctypes.c_uint64)), ("local_coverage", ctypes.POINTER(ctypes.c_uint64)),
                ("coverage", ctypes.POINTER(ctypes.c_int))]


class PgrResult(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("kept_rows", ctypes.c_int), ("width", ctypes.c_int), ("sc", ctypes.c_int),
                ("nsig", ctypes.c_int), ("cutoff", ctypes.c_double), ("kept", ctypes.POINTER(ctypes.c_ubyte)),
                ("maxcorrs", ctypes.POINTER(ctypes.c_double)), ("significant", ctypes.POINTER(ctypes.c_int)),
                ("sizes", ctypes.POINTER(ctypes.c_int)), ("cliques", ctypes.POINTER(ctypes.c_int)),
                ("cutoffs", ctypes.POINTER(ctypes.c_int)), ("drop_off", ctypes.POINTER(ctypes.c_double)),
                ("c_groups", ctypes.POINTER(ctypes.c_uint64)), ("c_coverage", ctypes.POINTER(ctypes.c_uint64))]


class PgrSubdivision(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("kept_rows", ctypes.c_int), ("dropoff_parts", ctypes.c_int),
                ("reldrop_parts", ctypes.c_int), ("selected", ctypes.c_int), ("eligible", ctypes.c_int),
                ("dropoff_labels", ctypes.POINTER(ctypes.c_int)), ("reldrop_labels", ctypes.POINTER(ctypes.c_int)),
                ("winner", ctypes.POINTER(ctypes.c_int)), ("winner_cutoff", ctypes.POINTER(ctypes.c_int))]


class PgrKmeans(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("kept_rows", ctypes.c_int), ("parts_before", ctypes.c_int), ("parts", ctypes.c_int),
                ("eligible", ctypes.c_int), ("labels", ctypes.POINTER(ctypes.c_int)), ("part", ctypes.POINTER(ctypes.c_int)),
                ("part_rows", ctypes.POINTER(ctypes.c_int)), ("row_offset", ctypes.POINTER(ctypes.c_int)),
                ("row", ctypes.POINTER(ctypes.c_int)), ("cluster_before", ctypes.POINTER(ctypes.c_int)),
                ("cluster_after", ctypes.POINTER(ctypes.c_int)), ("varzahl", ctypes.POINTER(ctypes.c_int)),
                ("var_offset", ctypes.POINTER(ctypes.c_int)), ("vars", ctypes.POINTER(ctypes.c_int)), ("pairs", ctypes.c_longlong),
                ("debug_pairs", ctypes.c_longlong), ("pair_part", ctypes.POINTER(ctypes.c_int)),
                ("pair_i", ctypes.POINTER(ctypes.c_int)), ("pair_j", ctypes.POINTER(ctypes.c_int)),
                ("pair_z", ctypes.POINTER(ctypes.c_double))]


class PgrResolvedWindow(ctypes.Structure):
    _fields_ = [("von", ctypes.c_int), ("bis", ctypes.c_int), ("kept_rows", ctypes.c_int), ("dropoff_parts", ctypes.c_int),
                ("reldrop_parts", ctypes.c_int), ("kmeans_parts", ctypes.c_int), ("cutoff", ctypes.c_double),
                ("dropoff_labels", ctypes.POINTER(ctypes.c_int)), ("reldrop_labels", ctypes.POINTER(ctypes.c_int)),
                ("kmeans_labels", ctypes.POINTER(ctypes.c_int))]


class PgrResolution(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("nwindows", ctypes.c_int), ("windows", ctypes.POINTER(PgrResolvedWindow))]


class PgrConnection(ctypes.Structure):
    _fields_ = [("k_first", ctypes.c_int), ("k_last", ctypes.c_int), ("matrix", ctypes.POINTER(ctypes.c_double)),
                ("best", ctypes.POINTER(ctypes.c_int)), ("confidence", ctypes.POINTER(ctypes.c_double)),
                ("mutual", ctypes.POINTER(ctypes.c_int))]


class PgrConsensus(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("von", ctypes.c_int), ("bis", ctypes.c_int), ("width", ctypes.c_int),
                ("parts", ctypes.c_int), ("part_label", ctypes.POINTER(ctypes.c_int)), ("part_rows", ctypes.POINTER(ctypes.c_int)),
                ("consensus", ctypes.POINTER(ctypes.c_ubyte)), ("depth", ctypes.POINTER(ctypes.c_int)),
                ("counts", ctypes.POINTER(ctypes.c_int)), ("nselected", ctypes.c_int), ("selected", ctypes.POINTER(ctypes.c_int)),
                ("diff", ctypes.POINTER(ctypes.c_int)), ("diff_all", ctypes.POINTER(ctypes.c_int))]


class PgrAssignment(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("parts", ctypes.c_int), ("ncolumns", ctypes.c_int), ("compared", ctypes.POINTER(ctypes.c_int)),
                ("best", ctypes.POINTER(ctypes.c_int)), ("second", ctypes.POINTER(ctypes.c_int)),
                ("best_mismatches", ctypes.POINTER(ctypes.c_int)), ("second_mismatches", ctypes.POINTER(ctypes.c_int)),
                ("mismatches", ctypes.POINTER(ctypes.c_int))]


class PgrSettlement(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("iterations", ctypes.c_int), ("stop", ctypes.c_int), ("parts", ctypes.c_int),
                ("part_label", ctypes.POINTER(ctypes.c_int)), ("labels", ctypes.POINTER(ctypes.c_int)),
                ("changed", ctypes.POINTER(ctypes.c_int)), ("parts_at", ctypes.POINTER(ctypes.c_int)),
                ("ncolumns_at", ctypes.POINTER(ctypes.c_int)), ("ncolumns", ctypes.c_int), ("columns", ctypes.POINTER(ctypes.c_int)),
                ("compared", ctypes.POINTER(ctypes.c_int)), ("best", ctypes.POINTER(ctypes.c_int)), ("second", ctypes.POINTER(ctypes.c_int)),
                ("best_mismatches", ctypes.POINTER(ctypes.c_int)), ("second_mismatches", ctypes.POINTER(ctypes.c_int))]


class PgrCrossovers(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("parts", ctypes.c_int), ("ncolumns", ctypes.c_int), ("nseg", ctypes.c_int)] + \
        [(name, ctypes.POINTER(ctypes.c_int)) for name in
         ("compared", "best", "second", "best_mismatches", "second_mismatches", "seg_compared", "seg_best", "cross_split", "cross_left",
          "cross_right", "cross_mismatches", "cross_left_compared", "seg_mismatches")]


class PgrThreads(ctypes.Structure):
    _fields_ = [("nres", ctypes.c_int), ("rows", ctypes.c_int), ("nthreads", ctypes.c_int), ("first", ctypes.POINTER(ctypes.c_int)),
                ("last", ctypes.POINTER(ctypes.c_int)), ("offset", ctypes.POINTER(ctypes.c_int)), ("thread_of", ctypes.POINTER(ctypes.c_int)),
                ("row_thread", ctypes.POINTER(ctypes.c_int)), ("row_conflict", ctypes.POINTER(ctypes.c_int))]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C repeatresolver_amd/csrc`.  There is no CPU fallback for the product path.")
    # Load order matters in a process that also uses torch: torch brings its own copy of the HIP runtime, libpwr.so is linked
    # against the system's, and the dynamic loader gives the process whichever copy came first under that name.  With the
    # system's first, torch.cuda later fails to initialise ("No HIP GPUs are available" -- found when a test module that touches
    # torch ran after modules that had loaded libpwr.so); with torch's first both work.  So torch goes first when it is there.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.pwr_create.restype = ci
    lib.pwr_create.argtypes = [ctypes.POINTER(vp), ci, ci, ctypes.c_char_p, ci, ci]
    lib.pwr_destroy.restype = None
    lib.pwr_destroy.argtypes = [vp]
    for n in ("pwr_trim_ends", "pwr_realign_round", "pwr_reset_stats"):
        getattr(lib, n).restype = ci
        getattr(lib, n).argtypes = [vp]
    lib.pwr_realign_row.restype = ci
    lib.pwr_realign_row.argtypes = [vp, ci]
    lib.pwr_realign_rows.restype = ci
    lib.pwr_realign_rows.argtypes = [vp, ci, ci]
    lib.pwr_total_score.restype = ci
    lib.pwr_total_score.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.pwr_dims.restype = ci
    lib.pwr_dims.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.pwr_export_rows.restype = ci
    lib.pwr_export_rows.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    lib.pwr_set_option.restype = ci
    lib.pwr_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_long]
    lib.pwr_get_option.restype = ci
    lib.pwr_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)]
    lib.pwr_get_stats.restype = ci
    lib.pwr_get_stats.argtypes = [vp, ctypes.POINTER(PwrStats)]
    lib.pwr_strerror.restype = ctypes.c_char_p
    lib.pwr_strerror.argtypes = [ci]
    lib.pwr_device_count.restype = ci
    lib.pwr_device_count.argtypes = []
    lib.pwr_split_begin.restype = ci
    lib.pwr_split_begin.argtypes = [vp, ci, ci, ci, ci]
    lib.pwr_split_slot_bytes.restype = ci
    lib.pwr_split_slot_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ci)]
    lib.pwr_split_stage.restype = ci
    lib.pwr_split_stage.argtypes = [vp, vp]
    lib.pwr_split_commit.restype = ci
    lib.pwr_split_commit.argtypes = [vp, vp, ctypes.POINTER(ci)]
    if hasattr(lib, "pwr_snapshot_begin"):
        lib.pwr_snapshot_begin.restype = ci
        lib.pwr_snapshot_begin.argtypes = [vp, ctypes.POINTER(vp)]
        lib.pwr_snapshot_wait.restype = ci
        lib.pwr_snapshot_wait.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ci), ctypes.POINTER(ci)]
        lib.pwr_snapshot_free.restype = None
        lib.pwr_snapshot_free.argtypes = [vp]
    lib.pwr_debug_last_job.restype = ci
    lib.pwr_debug_last_job.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci),
                                       ctypes.POINTER(ci), ctypes.POINTER(ci), ci]
    lib.pwr_debug_fill_clock.restype = ci
    lib.pwr_debug_fill_clock.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    lib.pwr_debug_row_columns.restype = ci
    lib.pwr_debug_row_columns.argtypes = [vp, ci, ctypes.POINTER(ci), ci]
    lib.pwr_debug_rounds.restype = ci
    lib.pwr_debug_rounds.argtypes = [vp]
    ll = ctypes.c_longlong
    lib.pia_create.restype = ci
    lib.pia_create.argtypes = [ctypes.POINTER(vp), ctypes.c_char_p, ci, ci]
    lib.pia_destroy.restype = None
    lib.pia_destroy.argtypes = [vp]
    lib.pia_align.restype = ci
    lib.pia_align.argtypes = [vp, ci, ctypes.c_char_p, ctypes.POINTER(ll), ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.pia_align_strands.restype = ci
    lib.pia_align_strands.argtypes = [vp, ci, ctypes.c_char_p, ctypes.POINTER(ll), ctypes.POINTER(ci), ctypes.POINTER(ci),
                                      ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_ubyte)]
    lib.pia_turn.restype = ci
    lib.pia_turn.argtypes = [ci, ctypes.c_char_p, ctypes.POINTER(ll), ctypes.POINTER(ctypes.c_ubyte), ctypes.c_char_p]
    lib.pia_get_stats.restype = ci
    lib.pia_get_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
    lib.pia_set_option.restype = ci
    lib.pia_set_option.argtypes = [vp, ctypes.c_char_p, ll]
    lib.pia_get_timing.restype = ci
    lib.pia_get_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    lib.pia_read_template.restype = ci
    lib.pia_read_template.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ci)]
    lib.pia_read_fasta.restype = ci
    lib.pia_read_fasta.argtypes = [ctypes.c_char_p, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]
    lib.pia_build_msa.restype = ci
    lib.pia_build_msa.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ci, ctypes.c_char_p, ctypes.POINTER(ll), ctypes.POINTER(ci),
                                  ctypes.POINTER(ci), ctypes.c_double, ci]
    lib.pmc_maxcorrs.restype = ci
    lib.pmc_maxcorrs.argtypes = [ci, ci, ctypes.c_char_p, ci, ci, ctypes.POINTER(ctypes.c_double)]
    lib.pmc_last_timing.restype = ci
    lib.pmc_last_timing.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.pmc_read_msa.restype = ci
    lib.pmc_read_msa.argtypes = [ctypes.c_char_p, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_void_p)]
    lib.pmc_write.restype = ci
    lib.pmc_write.argtypes = [ctypes.c_char_p, ci, ctypes.POINTER(ctypes.c_double)]
    pi, pll, cp = ctypes.POINTER(ci), ctypes.POINTER(ll), ctypes.c_char_p
    lib.prc_create.restype = ci
    lib.prc_create.argtypes = [ctypes.POINTER(vp), cp, ci, ci]
    lib.prc_destroy.restype = None
    lib.prc_destroy.argtypes = [vp]
    lib.prc_occurrences.restype = ci
    lib.prc_occurrences.argtypes = [vp, ci, cp, pll, ci, ci, ctypes.c_double, pll, ctypes.POINTER(vp)]
    lib.prc_cut.restype = ci
    lib.prc_cut.argtypes = [vp, ci, cp, pll, ci, ci, ctypes.c_double, pi, ctypes.POINTER(vp)]
    lib.prc_occurrences_strands.restype = ci
    lib.prc_occurrences_strands.argtypes = lib.prc_occurrences.argtypes
    lib.prc_cut_strands.restype = ci
    lib.prc_cut_strands.argtypes = [vp, ci, cp, pll, ci, ci, ctypes.c_double, pi, ctypes.POINTER(vp), pi, pi]
    lib.prc_merge_cuts.restype = ci
    lib.prc_merge_cuts.argtypes = [ci, ci, pi, ci, pi, pi]
    lib.prc_get_stats.restype = ci
    lib.prc_get_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)]
    lib.prc_free.restype = None
    lib.prc_free.argtypes = [vp]
    lib.prc_read_template.restype = ci
    lib.prc_read_template.argtypes = [cp, ctypes.POINTER(vp), pi]
    lib.prc_read_fasta.restype = ci
    lib.prc_read_fasta.argtypes = [cp, pi, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), pi]
    lib.prc_scan_dense.restype = ci
    lib.prc_scan_dense.argtypes = [pi, ci, ci, ci, pi]
    lib.prc_scan_runs.restype = ci
    lib.prc_scan_runs.argtypes = [pi, ci, ci, pi]
    lib.prc_select_cuts.restype = ci
    lib.prc_select_cuts.argtypes = [ci, ci, ci, ci, pi, ci, pi, ci, pi]
    lib.prc_write_seq.restype = ci
    lib.prc_write_seq.argtypes = [cp, ci, cp, pll, pi, pi]
    lib.prc_write_info.restype = ci
    lib.prc_write_info.argtypes = [cp, ci, pi]
    lib.prc_run_files.restype = ci
    lib.prc_run_files.argtypes = [cp, cp, cp, cp, ci, ci, ctypes.c_double, ci, ci, vp]
    pd = ctypes.POINTER(ctypes.c_double)
    lib.pgr_refine.restype = ci
    lib.pgr_refine.argtypes = [ci, ci, cp, pd, ci, ci, ci, ctypes.c_double, ci, ctypes.POINTER(PgrResult)]
    lib.pgr_free.restype = None
    lib.pgr_free.argtypes = [ctypes.POINTER(PgrResult)]
    lib.pgr_last_timing.restype = ci
    lib.pgr_last_timing.argtypes = [pd]
    lib.pgr_read_window.restype = ci
    lib.pgr_read_window.argtypes = [ci, ci, cp, ci, ci, ctypes.POINTER(PgrWindow)]
    lib.pgr_window_free.restype = None
    lib.pgr_window_free.argtypes = [ctypes.POINTER(PgrWindow)]
    lib.pgr_slice_maxcorrs.restype = ci
    lib.pgr_slice_maxcorrs.argtypes = [pd, ci, ci, ci, pd]
    lib.pgr_read_maxcorrs_file.restype = ci
    lib.pgr_read_maxcorrs_file.argtypes = [cp, ci, ci, ctypes.POINTER(vp), pi]
    lib.pgr_default_cutoff.restype = ctypes.c_double
    lib.pgr_default_cutoff.argtypes = [ctypes.c_double, ci]
    lib.pgr_restrict_coverage.restype = ci
    lib.pgr_restrict_coverage.argtypes = [ci, pi, pd, pi]
    lib.pgr_subdivide.restype = ci
    lib.pgr_subdivide.argtypes = [ctypes.POINTER(PgrWindow), ctypes.POINTER(PgrResult), ci, ci, ctypes.POINTER(PgrSubdivision)]
    lib.pgr_subdivision_free.restype = None
    lib.pgr_subdivision_free.argtypes = [ctypes.POINTER(PgrSubdivision)]
    lib.pgr_last_subdivision_timing.restype = ci
    lib.pgr_last_subdivision_timing.argtypes = [pd]
    lib.pgr_dropoff_subdivision.restype = ci
    lib.pgr_dropoff_subdivision.argtypes = [ctypes.POINTER(PgrResult), ci, pi, pi, pd]
    lib.pgr_compress_labels.restype = ci
    lib.pgr_compress_labels.argtypes = [ci, pi]
    lib.pgr_complete_labels.restype = ci
    lib.pgr_complete_labels.argtypes = [ci, ctypes.POINTER(ctypes.c_ubyte), pi, pi]
    lib.pgr_write_subdivision.restype = ci
    lib.pgr_write_subdivision.argtypes = [cp, pi, ci]
    lib.pgr_subdivision_name.restype = ci
    lib.pgr_subdivision_name.argtypes = [cp, ctypes.c_size_t, cp, ci, ci, cp]
    lib.pgr_kmeans_subdivide.restype = ci
    lib.pgr_kmeans_subdivide.argtypes = [ctypes.POINTER(PgrWindow), ctypes.POINTER(PgrResult), pi, ci, ci, ctypes.POINTER(PgrKmeans)]
    lib.pgr_kmeans_free.restype = None
    lib.pgr_kmeans_free.argtypes = [ctypes.POINTER(PgrKmeans)]
    lib.pgr_kmeans_subdivide_pairs.restype = ci
    lib.pgr_kmeans_subdivide_pairs.argtypes = lib.pgr_kmeans_subdivide.argtypes
    lib.pgr_last_kmeans_timing.restype = ci
    lib.pgr_last_kmeans_timing.argtypes = [pd]
    lib.pgr_kmeans_reassign.restype = ci
    lib.pgr_kmeans_reassign.argtypes = [ci, ctypes.POINTER(ctypes.c_ushort), ci, pi]
    lib.pgr_msa_open.restype = ci
    lib.pgr_msa_open.argtypes = [ci, ci, vp, ci, ctypes.POINTER(vp)]
    lib.pgr_msa_close.restype = None
    lib.pgr_msa_close.argtypes = [vp]
    lib.pgr_msa_window.restype = ci
    lib.pgr_msa_window.argtypes = [vp, ci, ci, ctypes.POINTER(PgrWindow)]
    lib.pgr_msa_resolve.restype = ci
    lib.pgr_msa_resolve.argtypes = [vp, pd, ci, pi, ci, ctypes.c_double, ctypes.POINTER(PgrResolution)]
    lib.pgr_resolution_free.restype = None
    lib.pgr_resolution_free.argtypes = [ctypes.POINTER(PgrResolution)]
    lib.pgr_last_resolve_timing.restype = ci
    lib.pgr_last_resolve_timing.argtypes = [pd]
    lib.pgr_connect.restype = ci
    lib.pgr_connect.argtypes = [ci, ci, pi, ctypes.POINTER(PgrConnection)]
    lib.pgr_connection_free.restype = None
    lib.pgr_connection_free.argtypes = [ctypes.POINTER(PgrConnection)]
    lib.pgr_msa_consensus.restype = ci
    lib.pgr_msa_consensus.argtypes = [vp, pi, ci, ci, pd, ctypes.c_double, ci, ctypes.POINTER(PgrConsensus)]
    lib.pgr_consensus_free.restype = None
    lib.pgr_consensus_free.argtypes = [ctypes.POINTER(PgrConsensus)]
    lib.pgr_last_consensus_timing.restype = ci
    lib.pgr_last_consensus_timing.argtypes = [pd]
    lib.pgr_resolvability.restype = ci
    lib.pgr_resolvability.argtypes = [ci, pi, pi, pi, pi]
    lib.pgr_msa_assign.restype = ci
    lib.pgr_msa_assign.argtypes = [vp, ci, ci, ci, vp, ci, pi, ci, ctypes.POINTER(PgrAssignment)]
    lib.pgr_assignment_free.restype = None
    lib.pgr_assignment_free.argtypes = [ctypes.POINTER(PgrAssignment)]
    lib.pgr_last_assign_timing.restype = ci
    lib.pgr_last_assign_timing.argtypes = [pd]
    lib.pgr_msa_settle.restype = ci
    lib.pgr_msa_settle.argtypes = [vp, pi, ci, ci, pd, ctypes.c_double, ci, ci, ci, ci, ci, ci, ctypes.POINTER(PgrSettlement)]
    lib.pgr_settlement_free.restype = None
    lib.pgr_settlement_free.argtypes = [ctypes.POINTER(PgrSettlement)]
    lib.pgr_last_settle_timing.restype = ci
    lib.pgr_last_settle_timing.argtypes = [pd]
    lib.pgr_msa_crossovers.restype = ci
    lib.pgr_msa_crossovers.argtypes = [vp, ci, ci, ci, vp, ci, pi, ci, pi, ci, ci, ctypes.POINTER(PgrCrossovers)]
    lib.pgr_crossovers_free.restype = None
    lib.pgr_crossovers_free.argtypes = [ctypes.POINTER(PgrCrossovers)]
    lib.pgr_last_crossover_timing.restype = ci
    lib.pgr_last_crossover_timing.argtypes = [pd]
    lib.pgr_thread.restype = ci
    lib.pgr_thread.argtypes = [ci, ci, pi, ctypes.POINTER(PgrThreads)]
    lib.pgr_threads_free.restype = None
    lib.pgr_threads_free.argtypes = [ctypes.POINTER(PgrThreads)]
    for n in ("pmc_tail_probe", "pgr_tail_probe", "pgr_km_tail_probe"):   # test hooks (tail_probe.py)
        getattr(lib, n).restype = ci
        getattr(lib, n).argtypes = [ci, pi, pd, ci, pd]
    pub = ctypes.POINTER(ctypes.c_ubyte)
    lib.pfl_create.restype = ci
    lib.pfl_create.argtypes = [ctypes.POINTER(vp), ci]
    lib.pfl_destroy.restype = None
    lib.pfl_destroy.argtypes = [vp]
    lib.pfl_neighbours.restype = ci
    lib.pfl_neighbours.argtypes = [ci, pi, cp, pub, pi, pi, pi, pi, pi, pi]
    lib.pfl_distances.restype = ci
    lib.pfl_distances.argtypes = [vp, ci, cp, pll, pi, pi, ci, ci, pi, pi]
    lib.pfl_cluster.restype = ci
    lib.pfl_cluster.argtypes = [ci, pi, pi, ci, ci, pi]
    lib.pfl_get_stats.restype = ci
    lib.pfl_get_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), pd]
    lib.pfl_labels.restype = ci
    lib.pfl_labels.argtypes = [vp, ci, cp, pll, pi, cp, pub, ci, ci, ci, ci, pi, pi, pi]
    lib.pfl_read_info.restype = ci
    lib.pfl_read_info.argtypes = [cp, pi, ctypes.POINTER(vp)]
    lib.pfl_free.restype = None
    lib.pfl_free.argtypes = [vp]
    lib.pfl_write_labels.restype = ci
    lib.pfl_write_labels.argtypes = [cp, ci, pi]
    lib.pfl_run_files.restype = ci
    lib.pfl_run_files.argtypes = [cp, cp, cp, cp, ci, ci, ci, ci, cp, cp, ci, vp]
    cll = ctypes.c_longlong
    pres = ctypes.POINTER(PflConsensusResult)
    lib.pfl_place.restype = ci
    lib.pfl_place.argtypes = [vp, ci, cp, pll, pi, pi, pi, ci, cp, pll, ci, ci, ci, pub, cll, pi, pi, pi]
    lib.pfl_set_scratch_limit.restype = ci
    lib.pfl_set_scratch_limit.argtypes = [vp, cll]
    lib.pfl_get_place_stats.restype = ci
    lib.pfl_get_place_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), pd, pd]
    lib.pfl_consensus.restype = ci
    lib.pfl_consensus.argtypes = [vp, ci, cp, pll, pi, pi, pi, ci, ci, ci, ci, ci, pres]
    lib.pfl_consensus_free.restype = None
    lib.pfl_consensus_free.argtypes = [pres]
    lib.pfl_consensus_pack.restype = ci
    lib.pfl_consensus_pack.argtypes = [ci, pi, pi, pi, ctypes.POINTER(cp), ctypes.POINTER(pi), pi, pres]
    lib.pfl_call.restype = ci
    lib.pfl_call.argtypes = [ci, pub, pub, pi, ci, cp, pi]
    lib.pfl_write_flank_fasta.restype = ci
    lib.pfl_write_flank_fasta.argtypes = [cp, cp, pres]
    lib.pfl_run_files_consensus.restype = ci
    lib.pfl_run_files_consensus.argtypes = [cp, cp, cp, cp, ci, ci, ci, ci, cp, cp, ci, ci, ci, ci, cp, cp, ci, vp]
    phits, pcon, ploci, ppl = ctypes.POINTER(PlaHits), ctypes.POINTER(PlaContigs), ctypes.POINTER(PlaLoci), ctypes.POINTER(PlaPlacement)
    lib.pla_create.restype = ci
    lib.pla_create.argtypes = [ctypes.POINTER(vp), ci]
    lib.pla_destroy.restype = None
    lib.pla_destroy.argtypes = [vp]
    lib.pla_open_text.restype = ci
    lib.pla_open_text.argtypes = [vp, ci, cp, pll]
    lib.pla_close_text.restype = None
    lib.pla_close_text.argtypes = [vp]
    lib.pla_set_option.restype = ci
    lib.pla_set_option.argtypes = [vp, cp, cll]
    lib.pla_search.restype = ci
    lib.pla_search.argtypes = [vp, ci, cp, pll, pi, ci, ci, ci, phits]
    lib.pla_hits_free.restype = None
    lib.pla_hits_free.argtypes = [phits]
    lib.pla_get_stats.restype = ci
    lib.pla_get_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), pd]
    lib.pla_read_contigs.restype = ci
    lib.pla_read_contigs.argtypes = [cp, pcon]
    lib.pla_contigs_free.restype = None
    lib.pla_contigs_free.argtypes = [pcon]
    lib.pla_read_loci.restype = ci
    lib.pla_read_loci.argtypes = [cp, ploci]
    lib.pla_loci_free.restype = None
    lib.pla_loci_free.argtypes = [ploci]
    lib.pla_place.restype = ci
    lib.pla_place.argtypes = [ci, pi, pi, phits, ci, ppl]
    lib.pla_status_name.restype = cp
    lib.pla_status_name.argtypes = [ci]
    lib.pla_write_placements.restype = ci
    lib.pla_write_placements.argtypes = [cp, ci, ctypes.POINTER(cp), ppl, pcon]
    lib.pla_write_patched.restype = ci
    lib.pla_write_patched.argtypes = [cp, pcon, ci, ppl, cp, pll]
    lib.pla_run_files.restype = ci
    lib.pla_run_files.argtypes = [cp, cp, ci, ci, ci, ci, cp, ci, vp]
    _lib = lib
    return lib
