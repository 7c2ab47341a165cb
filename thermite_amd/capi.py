"""ctypes binding of the C ABI in include/thermite.h (libthermite_amd.so).

This is host plumbing for tests and bench.py; the product is the shared
library.  There is no fallback: if the HIP library is missing, or no MI355X is
visible when an aligner is created, this raises.
"""
import ctypes as C
import os

import numpy as np

from .refdata import EXON_DT, REF_DT, SPAN_DT, TX_DT  # noqa: F401  (re-exported)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("THM_LIB") or os.path.join(_HERE, "_build", "libthermite_amd.so")

MEM_DT = np.dtype([("ref_idx", "<u8"), ("query_idx", "<u4"), ("len", "<u4")])
ALN_DT = np.dtype(
    [
        ("ystart", "<u8"),
        ("yend", "<u8"),
        ("ylen", "<u8"),
        ("ops_off", "<u8"),
        ("tx_ystart", "<u8"),
        ("tx_yend", "<u8"),
        ("tx_ylen", "<u8"),
        ("tx_ops_off", "<u8"),
        ("score", "<i4"),
        ("ref_id", "<u4"),
        ("xstart", "<u4"),
        ("xend", "<u4"),
        ("xlen", "<u4"),
        ("ops_len", "<u4"),
        ("tx_or_gene_idx", "<u4"),
        ("tx_score", "<i4"),
        ("tx_xstart", "<u4"),
        ("tx_xend", "<u4"),
        ("tx_ops_len", "<u4"),
        ("strand", "u1"),
        ("primary", "u1"),
        ("aln_type", "u1"),
        ("pad_", "u1"),
    ]
)
SWG_DT = np.dtype([("ops_off", "<u8"), ("ops_len", "<u4"), ("score", "<i4"), ("xend", "<u4"), ("yend", "<u4")])
# thm_lr_aln: one extend_left_right result (bio Alignment), include/thermite.h
LR_DT = np.dtype([("ystart", "<u8"), ("yend", "<u8"), ("ylen", "<u8"), ("ops_off", "<u8"), ("score", "<i4"),
                  ("xstart", "<u4"), ("xend", "<u4"), ("xlen", "<u4"), ("ops_len", "<u4"), ("pad_", "<u4")])
# thm_aln_digest: run-length CIGAR and counts of one alignment, include/thermite.h
DIGEST_DT = np.dtype([("cigar_off", "<u8"), ("ref_len", "<u8"), ("n_cigar", "<u4"), ("n_tx_cigar", "<u4"),
                      ("n_match", "<u4"), ("n_subst", "<u4"), ("n_not_yclip", "<u4"), ("flags", "<u4")])
DIGEST_LONG_RUN, DIGEST_MALFORMED = 1, 2
assert ALN_DT.itemsize == 112 and MEM_DT.itemsize == 16 and SWG_DT.itemsize == 24 and LR_DT.itemsize == 56
assert DIGEST_DT.itemsize == 40

N_COUNTERS = 16
COUNTER_NAMES = ["reads", "aligned", "unmapped", "alns", "exonic", "intronic", "intergenic", "smems", "hits",
                 "swg_calls", "dp_cells", "dp_cols", "op_bytes", "window_bytes"]
N_TIMINGS = 8
TIMING_NAMES = ["seed", "plan", "extend", "compact", "total", "cigar", "bam", "bgzf"]

OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_OUT_OF_CONTRACT, ERR_OOM, ERR_INTERNAL = (
    0, -1, -2, -3, -4, -5, -6, -7)


class ThermiteError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("thermite_amd error %d: %s" % (code, msg))
        self.code = code


class Opts(C.Structure):
    """thm_align_opts == AlignOpts (reference src/aligner.rs:452-464)."""

    _fields_ = [
        ("min_seed_len", C.c_uint64),
        ("min_aln_score_percent", C.c_float),
        ("min_aln_score", C.c_int32),
        ("multimap_score_range", C.c_uint64),
        ("intron_mode", C.c_int32),
        ("reserved", C.c_int32),
    ]


# reference defaults: src/main.rs:115-140, src/wrapper.rs:40-46
DEFAULT_OPTS = dict(min_seed_len=20, min_aln_score_percent=0.66, min_aln_score=30, multimap_score_range=1,
                    intron_mode=False)
# flags of the reference's chrM / chr21 runs: -k20 -s0 --intron-mode (data/Makefile:30,39)
CI_OPTS = dict(min_seed_len=20, min_aln_score_percent=0.0, min_aln_score=30, multimap_score_range=1, intron_mode=True)


class BatchView(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_alns", C.c_uint64), ("n_op_bytes", C.c_uint64),
                ("read_aln_off", C.c_void_p), ("alns", C.c_void_p), ("ops", C.c_void_p),
                ("n_failed_reads", C.c_uint64), ("read_status", C.c_void_p)]


class MemsView(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_mems", C.c_uint64), ("read_mem_off", C.c_void_p), ("mems", C.c_void_p)]


class SwgView(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_op_bytes", C.c_uint64), ("alns", C.c_void_p), ("ops", C.c_void_p)]


class LrView(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_op_bytes", C.c_uint64), ("alns", C.c_void_p), ("ops", C.c_void_p)]


class HitsView(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("n_op_bytes", C.c_uint64), ("alns", C.c_void_p), ("ops", C.c_void_p),
                ("n_failed_hits", C.c_uint64), ("hit_status", C.c_void_p)]


class AlnDigest(C.Structure):
    """thm_aln_digest"""

    _fields_ = [("cigar_off", C.c_uint64), ("ref_len", C.c_uint64), ("n_cigar", C.c_uint32), ("n_tx_cigar", C.c_uint32),
                ("n_match", C.c_uint32), ("n_subst", C.c_uint32), ("n_not_yclip", C.c_uint32), ("flags", C.c_uint32)]


class CigarView(C.Structure):
    """thm_cigar_view"""

    _fields_ = [("n_reads", C.c_uint64), ("n_alns", C.c_uint64), ("n_cigar_words", C.c_uint64),
                ("read_aln_off", C.c_void_p), ("alns", C.c_void_p), ("digests", C.c_void_p), ("cigar", C.c_void_p),
                ("n_failed_reads", C.c_uint64), ("read_status", C.c_void_p)]


class BamView(C.Structure):
    """thm_bam_view (include/thermite_io.h)"""

    _fields_ = [("n_reads", C.c_uint64), ("n_records", C.c_uint64), ("n_bytes", C.c_uint64), ("data", C.c_void_p),
                ("read_rec_off", C.c_void_p), ("n_failed_reads", C.c_uint64), ("read_status", C.c_void_p)]


class BgzfView(C.Structure):
    """thm_bgzf_view (include/thermite_io.h)"""

    _fields_ = [("n_reads", C.c_uint64), ("n_records", C.c_uint64), ("n_raw_bytes", C.c_uint64), ("n_blocks", C.c_uint64),
                ("n_bytes", C.c_uint64), ("data", C.c_void_p), ("block_off", C.c_void_p), ("n_failed_reads", C.c_uint64),
                ("read_status", C.c_void_p)]


class BamSortInfo(C.Structure):
    """thm_bam_sort_info (include/thermite_io.h)"""

    _fields_ = [("n_reads", C.c_uint64), ("n_records", C.c_uint64), ("n_bytes", C.c_uint64), ("total_records", C.c_uint64),
                ("total_bytes", C.c_uint64), ("n_failed_reads", C.c_uint64), ("read_status", C.c_void_p), ("add_ms", C.c_float)]


class BamSortedView(C.Structure):
    """thm_bam_sorted_view (include/thermite_io.h)"""

    _fields_ = [("total_records", C.c_uint64), ("total_raw_bytes", C.c_uint64), ("raw_offset", C.c_uint64), ("n_raw_bytes", C.c_uint64),
                ("n_blocks", C.c_uint64), ("n_bytes", C.c_uint64), ("data", C.c_void_p), ("block_off", C.c_void_p),
                ("gather_ms", C.c_float), ("deflate_ms", C.c_float)]


SORT_RAW = 1


class BaiView(C.Structure):
    """thm_bai_view (include/thermite_io.h)"""

    _fields_ = [("n_bytes", C.c_uint64), ("data", C.c_void_p), ("n_refs", C.c_uint64), ("n_bins", C.c_uint64), ("n_chunks", C.c_uint64),
                ("n_intervals", C.c_uint64), ("n_no_coor", C.c_uint64), ("index_ms", C.c_float)]


QUANT_GENE_DT = np.dtype([("exonic_unique", "<u8"), ("exonic_multi", "<u8"), ("intronic_unique", "<u8"), ("intronic_multi", "<u8")])
QUANT_JUNCTION_DT = np.dtype([("ref_id", "<u4"), ("strand", "<u4"), ("start", "<u8"), ("end", "<u8"), ("n_unique", "<u8"),
                              ("n_multi", "<u8"), ("max_overhang", "<u4"), ("pad", "<u4")])
assert QUANT_GENE_DT.itemsize == 32 and QUANT_JUNCTION_DT.itemsize == 48
QUANT_TOTAL_NAMES = ["n_reads", "n_failed_reads", "n_unmapped_reads", "n_unique_reads", "n_multi_reads", "n_alns",
                     "n_intergenic_unique", "n_intergenic_multi", "n_spliced_alns", "n_junction_hits", "n_long_run_alns"]


class QuantTotals(C.Structure):
    """thm_quant_totals (include/thermite_io.h)"""

    _fields_ = [(k, C.c_uint64) for k in QUANT_TOTAL_NAMES]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in QUANT_TOTAL_NAMES}


class QuantInfo(C.Structure):
    """thm_quant_info (include/thermite_io.h)"""

    _fields_ = [("batch", QuantTotals), ("n_junctions", C.c_uint64), ("held_bytes", C.c_uint64), ("add_ms", C.c_float)]


class QuantView(C.Structure):
    """thm_quant_view (include/thermite_io.h)"""

    _fields_ = [("n_genes", C.c_uint64), ("genes", C.c_void_p), ("n_junctions", C.c_uint64), ("junctions", C.c_void_p),
                ("totals", QuantTotals), ("fetch_ms", C.c_float)]


COV_STRANDED, COV_MULTI = 1, 2
COV_TILE = 4096               # cov::TILE of thermite_amd/csrc/coverage_device.h: the positions a fetch works on at a time
COV_MAX_DEPTH_WINDOW = 1 << 24
COV_RUN_DT = np.dtype([("ref_id", "<u4"), ("depth", "<u4"), ("start", "<u8"), ("end", "<u8")])
assert COV_RUN_DT.itemsize == 24
COV_TOTAL_NAMES = ["n_reads", "n_failed_reads", "n_alns", "n_skipped_multi", "n_long_run_alns"]
COV_TRACK_TOTAL_NAMES = ["n_alns", "n_blocks", "n_bases"]


class CovTrackTotals(C.Structure):
    """thm_cov_track_totals (include/thermite_io.h)"""

    _fields_ = [(k, C.c_uint64) for k in COV_TRACK_TOTAL_NAMES]


class CovTotals(C.Structure):
    """thm_cov_totals (include/thermite_io.h)"""

    _fields_ = [(k, C.c_uint64) for k in COV_TOTAL_NAMES] + [("track", CovTrackTotals * 4)]

    def as_dict(self):
        out = {k: int(getattr(self, k)) for k in COV_TOTAL_NAMES}
        out["track"] = [{k: int(getattr(t, k)) for k in COV_TRACK_TOTAL_NAMES} for t in self.track]
        return out


class CovInfo(C.Structure):
    """thm_cov_info (include/thermite_io.h)"""

    _fields_ = [("batch", CovTotals), ("held_bytes", C.c_uint64), ("add_ms", C.c_float)]


class CovView(C.Structure):
    """thm_cov_view (include/thermite_io.h)"""

    _fields_ = [("track", C.c_uint32), ("first_ref", C.c_uint32), ("n_refs", C.c_uint32), ("max_depth", C.c_uint32), ("n_runs", C.c_uint64),
                ("runs", C.c_void_p), ("n_covered", C.c_uint64), ("n_bases", C.c_uint64), ("totals", CovTotals), ("fetch_ms", C.c_float)]


class CovDepthView(C.Structure):
    """thm_cov_depth_view (include/thermite_io.h)"""

    _fields_ = [("n", C.c_uint64), ("depth", C.c_void_p), ("depth_ms", C.c_float)]


PILE_MULTI = 1
PILE_CHUNK = 8                # pile::CHUNK of thermite_amd/csrc/pileup_device.h: the SEQ bytes a lane compares at a time ...
PILE_GROUP = 16               # ... and pile::GROUP, the lanes that walk one alignment
PILE_MAX_WINDOW = 1 << 20
PILE_SITE_DT = np.dtype([("ref_id", "<u4"), ("ref_base", "u1"), ("pad_", "u1", (3,)), ("pos", "<u8"), ("depth", "<u4"), ("cnt", "<u4", (5,)),
                         ("del", "<u4"), ("ins", "<u4")])
assert PILE_SITE_DT.itemsize == 48
PILE_TOTAL_NAMES = ["n_reads", "n_failed_reads", "n_alns", "n_skipped_multi", "n_long_run_alns", "n_used_alns", "n_blocks", "n_m_bases",
                    "n_mismatches", "n_del_bases", "n_ins", "n_ins_bases"]


class PileTotals(C.Structure):
    """thm_pile_totals (include/thermite_io.h)"""

    _fields_ = [(k, C.c_uint64) for k in PILE_TOTAL_NAMES]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in PILE_TOTAL_NAMES}


class PileInfo(C.Structure):
    """thm_pile_info (include/thermite_io.h)"""

    _fields_ = [("batch", PileTotals), ("n_events", C.c_uint64), ("held_bytes", C.c_uint64), ("add_ms", C.c_float)]


class PileView(C.Structure):
    """thm_pile_view (include/thermite_io.h)"""

    _fields_ = [("first_ref", C.c_uint32), ("n_refs", C.c_uint32), ("min_alt", C.c_uint32), ("pad_", C.c_uint32), ("n_sites", C.c_uint64),
                ("sites", C.c_void_p), ("n_events", C.c_uint64), ("totals", PileTotals), ("fetch_ms", C.c_float)]


CELLS_INTRONIC = 1
CELLS_MAX_LEN = 16
CELL_DT = np.dtype([("n_reads", "<u8"), ("barcode", "<u4"), ("n_umis", "<u4"), ("n_genes", "<u4"), ("pad_", "<u4")])
CELL_ENTRY_DT = np.dtype([("cell", "<u4"), ("gene", "<u4"), ("n_umis", "<u4"), ("n_reads", "<u4")])
assert CELL_DT.itemsize == 24 and CELL_ENTRY_DT.itemsize == 16
CELLS_TOTAL_NAMES = ["n_reads", "n_failed_reads", "n_unmapped_reads", "n_multi_reads", "n_intergenic_reads", "n_intronic_skipped_reads",
                     "n_untagged_reads", "n_counted_reads"]


class CellsTotals(C.Structure):
    """thm_cells_totals (include/thermite_io.h)"""

    _fields_ = [(k, C.c_uint64) for k in CELLS_TOTAL_NAMES]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in CELLS_TOTAL_NAMES}


class CellsInfo(C.Structure):
    """thm_cells_info (include/thermite_io.h)"""

    _fields_ = [("batch", CellsTotals), ("n_molecules", C.c_uint64), ("n_pending", C.c_uint64), ("held_bytes", C.c_uint64), ("add_ms", C.c_float)]


class CellsView(C.Structure):
    """thm_cells_view (include/thermite_io.h)"""

    _fields_ = [("cb_len", C.c_uint32), ("umi_len", C.c_uint32), ("min_umis", C.c_uint32), ("pad_", C.c_uint32), ("n_cells", C.c_uint64),
                ("cells", C.c_void_p), ("n_entries", C.c_uint64), ("entries", C.c_void_p), ("n_molecules", C.c_uint64), ("n_barcodes", C.c_uint64),
                ("n_cells_below", C.c_uint64), ("totals", CellsTotals), ("fetch_ms", C.c_float)]


class FastqUploadInfo(C.Structure):
    """thm_fastq_upload_info (include/thermite_io.h)"""

    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_name_bytes", C.c_uint64), ("on_device", C.c_uint32),
                ("device_ms", C.c_float)]


class FastqBgzfInfo(C.Structure):
    """thm_fastq_bgzf_info (include/thermite_io.h)"""

    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_name_bytes", C.c_uint64), ("n_lines", C.c_uint64),
                ("n_members", C.c_uint64), ("n_inflated_bytes", C.c_uint64), ("tail", C.c_void_p), ("tail_len", C.c_uint64),
                ("inflated_on_device", C.c_uint32), ("parsed_on_device", C.c_uint32), ("inflate_ms", C.c_float),
                ("parse_ms", C.c_float)]


class GzipState(C.Structure):
    """thm_gzip_state (include/thermite_io.h): all zero = the start of a file"""

    _fields_ = [("window", C.c_uint8 * 32768), ("window_len", C.c_uint32), ("bit_offset", C.c_uint32), ("in_member", C.c_uint32),
                ("crc", C.c_uint32), ("member_len", C.c_uint64), ("n_members_done", C.c_uint64), ("stream_offset", C.c_uint64)]

    def key(self):
        """the fields that say where the stream stands, the window cut to its length"""
        return (bytes(self.window[: self.window_len]), self.window_len, self.bit_offset, self.in_member, self.crc, self.member_len,
                self.n_members_done, self.stream_offset)

    def copy(self):
        out = GzipState()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(GzipState))
        return out


class FastqGzipInfo(C.Structure):
    """thm_fastq_gzip_info (include/thermite_io.h)"""

    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_name_bytes", C.c_uint64), ("n_lines", C.c_uint64),
                ("n_inflated_bytes", C.c_uint64), ("tail", C.c_void_p), ("tail_len", C.c_uint64),
                ("inflated_on_device", C.c_uint32), ("parsed_on_device", C.c_uint32), ("inflate_ms", C.c_float),
                ("parse_ms", C.c_float), ("n_consumed_bytes", C.c_uint64), ("n_chunks", C.c_uint64), ("n_starts", C.c_uint64),
                ("decline_reason", C.c_uint32), ("reserved", C.c_uint32)]


BAM_NO_ANNOTATION_TAGS = 1

# every symbol include/thermite.h declares
ABI_SYMBOLS = [
    "thm_index_create_in_memory", "thm_index_free", "thm_index_text_len", "thm_index_suffix_array",
    "thm_index_idx_to_ref", "thm_build_suffix_array", "thm_aligner_create", "thm_aligner_free", "thm_last_error",
    "thm_aligner_set_opts", "thm_aligner_stream", "thm_align_batch", "thm_batch_upload", "thm_batch_run",
    "thm_batch_sync", "thm_batch_fetch", "thm_smems_batch", "thm_swg_extend_batch", "thm_counters_get",
    "thm_counters_reset", "thm_counters_device_ptr", "thm_timings_get", "thm_version", "thm_device_count",
    "thm_aligner_index", "thm_comm_unique_id", "thm_comm_create", "thm_comm_free", "thm_counters_allreduce",
    "thm_index_create_in_memory_ex", "thm_index_coord_bytes", "thm_index_suffix_array64", "thm_build_suffix_array64", "thm_build_suffix_array_gpu",
    "thm_extend_left_right_batch", "thm_align_seed_hits_batch",
    "thm_batch_fetch_cigars", "thm_align_batch_cigars", "thm_cigar_encode_batch",
]
# every symbol include/thermite_io.h declares
IO_ABI_SYMBOLS = [
    "thm_index_create_from_files", "thm_index_set_names", "thm_index_save", "thm_index_load", "thm_index_tables",
    "thm_index_contig_name", "thm_index_tx_id", "thm_index_gene_id", "thm_index_gene_name", "thm_fastq_open",
    "thm_fastq_next_batch", "thm_fastq_close", "thm_writer_create", "thm_writer_free", "thm_writer_header",
    "thm_writer_format_batch", "thm_writer_trailer", "thm_align_files", "thm_align_files_multi",
    "thm_writer_format_batch_cigars",
    "thm_batch_upload_reads", "thm_batch_fetch_bam", "thm_align_batch_bam", "thm_writer_wrap_bam",
    "thm_batch_fetch_bgzf", "thm_align_batch_bgzf",
    "thm_batch_upload_fastq", "thm_batch_fetch_reads",
    "thm_batch_upload_fastq_bgzf",
    "thm_batch_upload_fastq_gzip",
    "thm_bam_sorter_create", "thm_bam_sorter_add", "thm_bam_sorter_finish", "thm_bam_sorter_next", "thm_bam_sorter_free",
    "thm_writer_header_sorted",
    "thm_bam_sorter_index",
    "thm_quant_create", "thm_quant_free", "thm_quant_add", "thm_quant_add_view", "thm_quant_fetch", "thm_quant_reset",
    "thm_coverage_create", "thm_coverage_free", "thm_coverage_add", "thm_coverage_add_view", "thm_coverage_fetch", "thm_coverage_depth",
    "thm_coverage_reset",
    "thm_pileup_create", "thm_pileup_free", "thm_pileup_add", "thm_pileup_add_view", "thm_pileup_fetch", "thm_pileup_window", "thm_pileup_reset",
    "thm_cells_create", "thm_cells_free", "thm_cells_add", "thm_cells_add_view", "thm_cells_fetch", "thm_cells_reset",
]
ERR_IO, ERR_FORMAT = -8, -9
FMT_PAF, FMT_SAM, FMT_BAM = 0, 1, 2

_lib = None


def lib():
    """Load libthermite_amd.so; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ThermiteError(ERR_INTERNAL, "HIP library not built: %s is missing (run __graft_entry__.build())" % SO_PATH)
    L = C.CDLL(SO_PATH)
    vp, u64, i32, u32 = C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32
    L.thm_index_create_in_memory.restype = i32
    L.thm_index_create_in_memory.argtypes = [vp, u64, vp, u32, vp, u32, vp, u64, vp, u64, vp, u32, vp, u32, vp, vp]
    L.thm_index_create_in_memory_ex.restype = i32
    L.thm_index_create_in_memory_ex.argtypes = [vp, u64, vp, u32, vp, u32, vp, u64, vp, u64, vp, u32, vp, u32, vp, u32, u32, vp]
    L.thm_index_coord_bytes.restype = u32
    L.thm_index_coord_bytes.argtypes = [vp]
    L.thm_index_suffix_array64.restype = vp
    L.thm_index_suffix_array64.argtypes = [vp]
    L.thm_build_suffix_array64.restype = i32
    L.thm_build_suffix_array64.argtypes = [vp, u64, vp]
    L.thm_build_suffix_array_gpu.restype = i32
    L.thm_build_suffix_array_gpu.argtypes = [vp, u64, vp, u32]
    if hasattr(L, "thm_debug_check_lut"):
        L.thm_debug_check_lut.restype = i32
        L.thm_debug_check_lut.argtypes = [vp]
    if hasattr(L, "thm_debug_host_lut"):
        L.thm_debug_host_lut.restype = i32
        L.thm_debug_host_lut.argtypes = [vp, vp, vp, u64]
    L.thm_index_free.argtypes = [vp]
    L.thm_index_text_len.restype = u64
    L.thm_index_text_len.argtypes = [vp]
    L.thm_index_suffix_array.restype = vp
    L.thm_index_suffix_array.argtypes = [vp]
    L.thm_index_idx_to_ref.restype = i32
    L.thm_index_idx_to_ref.argtypes = [vp, u64, vp]
    L.thm_build_suffix_array.restype = i32
    L.thm_build_suffix_array.argtypes = [vp, u64, vp]
    L.thm_aligner_create.restype = i32
    L.thm_aligner_create.argtypes = [vp, vp, i32, vp]
    L.thm_aligner_free.argtypes = [vp]
    L.thm_last_error.restype = C.c_char_p
    L.thm_last_error.argtypes = [vp]
    L.thm_aligner_set_opts.restype = i32
    L.thm_aligner_set_opts.argtypes = [vp, vp]
    L.thm_aligner_stream.restype = vp
    L.thm_aligner_stream.argtypes = [vp]
    L.thm_align_batch.restype = i32
    L.thm_align_batch.argtypes = [vp, vp, vp, u64, vp]
    L.thm_batch_upload.restype = i32
    L.thm_batch_upload.argtypes = [vp, vp, vp, u64]
    for f in ("thm_batch_run", "thm_batch_sync", "thm_counters_reset"):
        getattr(L, f).restype = i32
        getattr(L, f).argtypes = [vp]
    L.thm_batch_fetch.restype = i32
    L.thm_batch_fetch.argtypes = [vp, vp]
    L.thm_batch_fetch_cigars.restype = i32
    L.thm_batch_fetch_cigars.argtypes = [vp, vp]
    L.thm_align_batch_cigars.restype = i32
    L.thm_align_batch_cigars.argtypes = [vp, vp, vp, u64, vp]
    L.thm_cigar_encode_batch.restype = i32
    L.thm_cigar_encode_batch.argtypes = [vp, vp, vp, u64, vp]
    L.thm_smems_batch.restype = i32
    L.thm_smems_batch.argtypes = [vp, vp, vp, u64, u64, vp]
    L.thm_swg_extend_batch.restype = i32
    L.thm_swg_extend_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u64, vp]
    L.thm_counters_get.restype = i32
    L.thm_extend_left_right_batch.restype = i32
    L.thm_extend_left_right_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, u64, vp]
    L.thm_align_seed_hits_batch.restype = i32
    L.thm_align_seed_hits_batch.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, vp, u32, vp]
    L.thm_counters_get.argtypes = [vp, vp]
    L.thm_counters_device_ptr.restype = vp
    L.thm_counters_device_ptr.argtypes = [vp]
    L.thm_timings_get.restype = i32
    L.thm_timings_get.argtypes = [vp, vp]
    L.thm_version.restype = C.c_char_p
    L.thm_device_count.restype = i32
    L.thm_aligner_index.restype = vp
    L.thm_aligner_index.argtypes = [vp]
    L.thm_comm_unique_id.restype = i32
    L.thm_comm_unique_id.argtypes = [vp]
    L.thm_comm_create.restype = i32
    L.thm_comm_create.argtypes = [vp, i32, i32, i32, vp]
    L.thm_comm_free.argtypes = [vp]
    L.thm_counters_allreduce.restype = i32
    L.thm_counters_allreduce.argtypes = [vp, vp]
    # ---- include/thermite_io.h ----
    cp = C.c_char_p
    L.thm_index_create_from_files.restype = i32
    L.thm_index_create_from_files.argtypes = [cp, cp, vp]
    L.thm_index_set_names.restype = i32
    L.thm_index_set_names.argtypes = [vp, vp, u32, vp, u32, vp, vp, u32]
    L.thm_index_save.restype = i32
    L.thm_index_save.argtypes = [vp, cp]
    L.thm_index_load.restype = i32
    L.thm_index_load.argtypes = [cp, vp]
    L.thm_index_tables.restype = i32
    L.thm_index_tables.argtypes = [vp, vp]
    for f in ("thm_index_contig_name", "thm_index_tx_id", "thm_index_gene_id", "thm_index_gene_name"):
        getattr(L, f).restype = cp
        getattr(L, f).argtypes = [vp, u32]
    L.thm_fastq_open.restype = i32
    L.thm_fastq_open.argtypes = [cp, vp]
    L.thm_fastq_next_batch.restype = i32
    L.thm_fastq_next_batch.argtypes = [vp, u64, vp]
    L.thm_fastq_close.argtypes = [vp]
    if hasattr(L, "thm_debug_deflate_block"):
        L.thm_debug_deflate_block.restype = i32
        L.thm_debug_deflate_block.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
    if hasattr(L, "thm_debug_gunzip_mt"):
        L.thm_debug_gunzip_mt.restype = i32
        L.thm_debug_gunzip_mt.argtypes = [C.c_char_p, u64, u32, vp, u64, C.POINTER(u64)]
    if hasattr(L, "thm_debug_gunzip"):
        L.thm_debug_gunzip.restype = i32
        L.thm_debug_gunzip.argtypes = [C.c_char_p, u64, vp, u64, C.POINTER(u64)]
    if hasattr(L, "thm_debug_fastq_blocks"):
        L.thm_debug_fastq_blocks.restype = i32
        L.thm_debug_fastq_blocks.argtypes = [vp, u64, vp]
    L.thm_writer_create.restype = i32
    L.thm_writer_create.argtypes = [vp, i32, u32, vp]
    L.thm_writer_free.argtypes = [vp]
    L.thm_writer_header.restype = i32
    L.thm_writer_header.argtypes = [vp, vp]
    L.thm_writer_trailer.restype = i32
    L.thm_writer_trailer.argtypes = [vp, vp]
    L.thm_writer_format_batch.restype = i32
    L.thm_writer_format_batch.argtypes = [vp, vp, vp, vp]
    L.thm_writer_format_batch_cigars.restype = i32
    L.thm_writer_format_batch_cigars.argtypes = [vp, vp, vp, vp]
    L.thm_batch_upload_reads.restype = i32
    L.thm_batch_upload_reads.argtypes = [vp, vp]
    L.thm_batch_fetch_bam.restype = i32
    L.thm_batch_fetch_bam.argtypes = [vp, u32, vp]
    L.thm_align_batch_bam.restype = i32
    L.thm_align_batch_bam.argtypes = [vp, vp, u32, vp]
    L.thm_batch_fetch_bgzf.restype = i32
    L.thm_batch_fetch_bgzf.argtypes = [vp, u32, vp]
    L.thm_align_batch_bgzf.restype = i32
    L.thm_align_batch_bgzf.argtypes = [vp, vp, u32, vp]
    L.thm_debug_bgzf_device.restype = i32
    L.thm_debug_bgzf_device.argtypes = [vp, vp, u64, vp, u64, vp, vp]
    L.thm_batch_upload_fastq.restype = i32
    L.thm_batch_upload_fastq.argtypes = [vp, vp, u64, cp, u64, i32, vp]
    L.thm_batch_fetch_reads.restype = i32
    L.thm_batch_fetch_reads.argtypes = [vp, vp]
    L.thm_debug_fastq_device_blocks.restype = i32
    L.thm_debug_fastq_device_blocks.argtypes = [vp, vp, vp]
    L.thm_batch_upload_fastq_bgzf.restype = i32
    L.thm_batch_upload_fastq_bgzf.argtypes = [vp, vp, u64, vp, u64, cp, u64, i32, vp]
    L.thm_debug_bgzf_inflate.restype = i32
    L.thm_debug_bgzf_inflate.argtypes = [vp, vp, u64, vp, u64, vp]
    L.thm_debug_fastq_bgzf_blocks.restype = i32
    L.thm_debug_fastq_bgzf_blocks.argtypes = [vp, vp]
    L.thm_batch_upload_fastq_gzip.restype = i32
    L.thm_batch_upload_fastq_gzip.argtypes = [vp, vp, vp, u64, vp, u64, cp, u64, i32, vp]
    L.thm_debug_gzip_inflate.restype = i32
    L.thm_debug_gzip_inflate.argtypes = [vp, vp, vp, u64, u32, i32, vp, u64, vp, vp, vp]
    L.thm_debug_fastq_gzip_blocks.restype = i32
    L.thm_debug_fastq_gzip_blocks.argtypes = [vp, vp]
    L.thm_debug_gzip_host_slice.restype = i32
    L.thm_debug_gzip_host_slice.argtypes = [vp, vp, u64, i32, vp, u64, vp, vp]
    L.thm_writer_wrap_bam.restype = i32
    L.thm_writer_wrap_bam.argtypes = [vp, vp, vp]
    L.thm_writer_header_sorted.restype = i32
    L.thm_writer_header_sorted.argtypes = [vp, vp]
    L.thm_bam_sorter_create.restype = i32
    L.thm_bam_sorter_create.argtypes = [vp, u64, vp]
    L.thm_bam_sorter_add.restype = i32
    L.thm_bam_sorter_add.argtypes = [vp, u32, vp]
    L.thm_bam_sorter_finish.restype = i32
    L.thm_bam_sorter_finish.argtypes = [vp, vp]
    L.thm_bam_sorter_next.restype = i32
    L.thm_bam_sorter_next.argtypes = [vp, u64, u32, vp]
    L.thm_bam_sorter_free.restype = None
    L.thm_bam_sorter_free.argtypes = [vp]
    L.thm_bam_sorter_index.restype = i32
    L.thm_bam_sorter_index.argtypes = [vp, u64, vp]
    L.thm_quant_create.restype = i32
    L.thm_quant_create.argtypes = [vp, vp]
    L.thm_quant_free.restype = None
    L.thm_quant_free.argtypes = [vp]
    L.thm_quant_add.restype = i32
    L.thm_quant_add.argtypes = [vp, vp]
    L.thm_quant_add_view.restype = i32
    L.thm_quant_add_view.argtypes = [vp, vp, vp]
    L.thm_quant_fetch.restype = i32
    L.thm_quant_fetch.argtypes = [vp, vp]
    L.thm_quant_reset.restype = i32
    L.thm_quant_reset.argtypes = [vp]
    L.thm_coverage_create.restype = i32
    L.thm_coverage_create.argtypes = [vp, C.c_uint32, C.c_uint64, vp]
    L.thm_coverage_free.restype = None
    L.thm_coverage_free.argtypes = [vp]
    L.thm_coverage_add.restype = i32
    L.thm_coverage_add.argtypes = [vp, vp]
    L.thm_coverage_add_view.restype = i32
    L.thm_coverage_add_view.argtypes = [vp, vp, vp]
    L.thm_coverage_fetch.restype = i32
    L.thm_coverage_fetch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.thm_coverage_depth.restype = i32
    L.thm_coverage_depth.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vp]
    L.thm_coverage_reset.restype = i32
    L.thm_coverage_reset.argtypes = [vp]
    L.thm_pileup_create.restype = i32
    L.thm_pileup_create.argtypes = [vp, C.c_uint32, C.c_uint64, vp]
    L.thm_pileup_free.restype = None
    L.thm_pileup_free.argtypes = [vp]
    L.thm_pileup_add.restype = i32
    L.thm_pileup_add.argtypes = [vp, vp]
    L.thm_pileup_add_view.restype = i32
    L.thm_pileup_add_view.argtypes = [vp, vp, vp, vp, vp]
    L.thm_pileup_fetch.restype = i32
    L.thm_pileup_fetch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.thm_pileup_window.restype = i32
    L.thm_pileup_window.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_uint64, vp]
    L.thm_pileup_reset.restype = i32
    L.thm_pileup_reset.argtypes = [vp]
    L.thm_cells_create.restype = i32
    L.thm_cells_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, vp]
    L.thm_cells_free.restype = None
    L.thm_cells_free.argtypes = [vp]
    L.thm_cells_add.restype = i32
    L.thm_cells_add.argtypes = [vp, vp]
    L.thm_cells_add_view.restype = i32
    L.thm_cells_add_view.argtypes = [vp, vp, vp, vp, vp]
    L.thm_cells_fetch.restype = i32
    L.thm_cells_fetch.argtypes = [vp, C.c_uint32, vp]
    L.thm_cells_reset.restype = i32
    L.thm_cells_reset.argtypes = [vp]
    L.thm_debug_bam_sorter_add_records.restype = i32
    L.thm_debug_bam_sorter_add_records.argtypes = [vp, vp, u64]
    L.thm_debug_bam_sorter_gather.restype = i32
    L.thm_debug_bam_sorter_gather.argtypes = [vp, i32]
    L.thm_align_files.restype = i32
    L.thm_align_files.argtypes = [vp, vp, u32, cp, i32, u64, u32, vp]
    L.thm_align_files_multi.restype = i32
    L.thm_align_files_multi.argtypes = [vp, u32, vp, u32, cp, i32, u64, u32, vp]
    if hasattr(L, "thm_debug_prof_get"):
        L.thm_debug_prof_get.restype = i32
        L.thm_debug_prof_get.argtypes = [vp, vp, i32]
    if hasattr(L, "thm_debug_set_pool_caps"):
        L.thm_debug_set_pool_caps.restype = i32
        L.thm_debug_set_pool_caps.argtypes = [vp, u64, u64, u64, vp]
    if hasattr(L, "thm_debug_host_table"):
        L.thm_debug_host_table.restype = i32
        L.thm_debug_host_table.argtypes = [vp, i32, vp, u64, vp]
    if hasattr(L, "thm_debug_smem_finish_stats"):
        L.thm_debug_smem_finish_stats.restype = i32
        L.thm_debug_smem_finish_stats.argtypes = [vp, vp]
    if hasattr(L, "thm_debug_set_flags"):
        L.thm_debug_set_flags.restype = i32
        L.thm_debug_set_flags.argtypes = [vp, C.c_uint32]
        L.thm_debug_set_band_clip.restype = i32
        L.thm_debug_set_band_clip.argtypes = [vp, C.c_uint32]
        L.thm_debug_tpr_stats.restype = i32
        L.thm_debug_tpr_stats.argtypes = [vp, vp]
    if hasattr(L, "thm_debug_seed_stats"):
        L.thm_debug_seed_stats.restype = i32
        L.thm_debug_seed_stats.argtypes = [vp, vp]
    if hasattr(L, "thm_debug_seed_direct_stats"):
        L.thm_debug_seed_direct_stats.restype = i32
        L.thm_debug_seed_direct_stats.argtypes = [vp, vp]
    if hasattr(L, "thm_debug_fetch_lut"):
        L.thm_debug_fetch_lut.restype = i32
        L.thm_debug_fetch_lut.argtypes = [vp, vp, u64]
    if hasattr(L, "thm_debug_knobs"):
        L.thm_debug_knobs.restype = i32
        L.thm_debug_knobs.argtypes = [vp, vp]
    if hasattr(L, "thm_debug_calib_gather"):
        L.thm_debug_calib_gather.restype = i32
        L.thm_debug_calib_gather.argtypes = [vp, i32, u64, vp]
    if hasattr(L, "thm_debug_wave_prims"):
        L.thm_debug_wave_prims.restype = i32
        L.thm_debug_wave_prims.argtypes = [vp, vp, vp]
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _copy(ptr, count, dtype, copy=True):
    if count == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    nbytes = int(count) * np.dtype(dtype).itemsize
    buf = (C.c_uint8 * nbytes).from_address(ptr)
    a = np.frombuffer(buf, dtype=dtype, count=int(count))
    return a.copy() if copy else a


def _u8(b):
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, np.uint8)
    return np.frombuffer(bytes(b), np.uint8)


def build_suffix_array_gpu(text, wide=False):
    """the suffix array of `text` built on the current HIP device (thm_build_suffix_array_gpu); raises ThermiteError
    with ERR_NO_DEVICE / ERR_OOM / ERR_UNSUPPORTED when the host builder has to do it"""
    text = np.ascontiguousarray(text, np.uint8)
    out = np.empty(len(text), "<u8" if wide else "<u4")
    rc = lib().thm_build_suffix_array_gpu(_ptr(text), len(text), _ptr(out), 8 if wide else 4)
    if rc != 0:
        raise ThermiteError(rc, _last_error())
    return out


def build_suffix_array(text, wide=False):
    """suffix array of `text`: u32 entries, or u64 (`wide`, any text length)"""
    t = _u8(text)
    sa = np.zeros(len(t), "<u8" if wide else "<u4")
    f = lib().thm_build_suffix_array64 if wide else lib().thm_build_suffix_array
    rc = f(_ptr(t), len(t), _ptr(sa))
    if rc != 0:
        raise ThermiteError(rc, "thm_build_suffix_array")
    return sa


INDEX_WIDE = 1


class TablesView(C.Structure):
    _fields_ = [("n_text", C.c_uint64), ("text", C.c_void_p), ("n_refs", C.c_uint32), ("refs", C.c_void_p),
                ("n_txs", C.c_uint32), ("txs", C.c_void_p), ("n_exons", C.c_uint64), ("exons", C.c_void_p),
                ("n_tx_seq", C.c_uint64), ("tx_seq", C.c_void_p), ("n_genes", C.c_uint32), ("genes", C.c_void_p),
                ("name_rank", C.c_void_p), ("n_contigs", C.c_uint32)]


class ReadBatch(C.Structure):
    """thm_read_batch"""

    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("bases", C.c_void_p), ("offsets", C.c_void_p),
                ("quals", C.c_void_p), ("names", C.c_void_p), ("name_off", C.c_void_p)]


class Text(C.Structure):
    _fields_ = [("data", C.c_void_p), ("len", C.c_uint64)]


class RunStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_aligned_reads", C.c_uint64), ("n_records", C.c_uint64),
                ("n_batches", C.c_uint64), ("n_output_bytes", C.c_uint64), ("parse_s", C.c_double),
                ("gpu_s", C.c_double), ("format_s", C.c_double), ("write_s", C.c_double), ("wall_s", C.c_double)]


def _last_error(h=None):
    return (lib().thm_last_error(h) or b"").decode()


def _cstr_array(strs):
    arr = (C.c_char_p * len(strs))(*[s.encode() if isinstance(s, str) else bytes(s) for s in strs])
    return arr


class Index:
    """thm_index: the in-memory index (stands for reference Index, src/index.rs:39-44)."""

    @classmethod
    def _wrap(cls, h):
        self = cls.__new__(cls)
        self.h = h
        self.tables = None
        return self

    @classmethod
    def from_files(cls, fasta_path, gtf_path):
        """Index::create_from_files (src/index.rs:52-223) in the native library."""
        h = C.c_void_p()
        rc = lib().thm_index_create_from_files(str(fasta_path).encode(), str(gtf_path).encode(), C.byref(h))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        return cls._wrap(h)

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        rc = lib().thm_index_load(str(path).encode(), C.byref(h))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        return cls._wrap(h)

    def save(self, path):
        rc = lib().thm_index_save(self.h, str(path).encode())
        if rc != 0:
            raise ThermiteError(rc, _last_error())

    def set_names(self, contig_names, tx_ids, gene_ids, gene_names):
        a, b, c, d = (_cstr_array(x) for x in (contig_names, tx_ids, gene_ids, gene_names))
        rc = lib().thm_index_set_names(self.h, a, len(contig_names), b, len(tx_ids), c, d, len(gene_ids))
        if rc != 0:
            raise ThermiteError(rc, _last_error())

    def native_tables(self):
        """Copy of the tables the native index holds, in the layout of refdata.build_tables."""
        v = TablesView()
        rc = lib().thm_index_tables(self.h, C.byref(v))
        if rc != 0:
            raise ThermiteError(rc, "thm_index_tables")
        L = lib()
        dec = lambda f, n: [f(self.h, i).decode() for i in range(n)]
        names = dec(L.thm_index_contig_name, v.n_contigs)
        refs = _copy(v.refs, v.n_refs, REF_DT)
        rank_per_ref = _copy(v.name_rank, v.n_refs, "<u4")
        name_rank = np.zeros(v.n_contigs, "<u4")
        if v.n_contigs:
            name_rank[refs["name_id"]] = rank_per_ref
        have = v.n_contigs > 0
        return dict(
            text=_copy(v.text, v.n_text, np.uint8), refs=refs, names=names, name_rank=name_rank,
            txs=_copy(v.txs, v.n_txs, TX_DT), exons=_copy(v.exons, v.n_exons, EXON_DT),
            tx_seq=_copy(v.tx_seq, v.n_tx_seq, np.uint8), genes=_copy(v.genes, v.n_genes, SPAN_DT),
            gene_ids=dec(L.thm_index_gene_id, v.n_genes) if have else [],
            gene_names=dec(L.thm_index_gene_name, v.n_genes) if have else [],
            tx_ids=dec(L.thm_index_tx_id, v.n_txs) if have else [],
        )

    def __init__(self, tables, sa=None, wide=False):
        """`wide`: 64-bit text positions and ranks inside the index even for a small text (a text of 2^31
        symbols or more is wide by itself; THM_FORCE_WIDE=1 in the environment forces it for every index)"""
        t = tables
        self.tables = t
        h = C.c_void_p()
        sa_arr, sa_bytes = None, 0
        if sa is not None:
            sa_bytes = 8 if np.asarray(sa).dtype.itemsize == 8 else 4
            sa_arr = np.ascontiguousarray(sa, "<u8" if sa_bytes == 8 else "<u4")
        rc = lib().thm_index_create_in_memory_ex(
            _ptr(t["text"]), len(t["text"]), _ptr(t["refs"]), len(t["refs"]), _ptr(t["txs"]), len(t["txs"]),
            _ptr(t["exons"]), len(t["exons"]), _ptr(t["tx_seq"]), len(t["tx_seq"]), _ptr(t["genes"]), len(t["genes"]),
            _ptr(t["name_rank"]), len(t["name_rank"]), _ptr(sa_arr), sa_bytes, INDEX_WIDE if wide else 0, C.byref(h),
        )
        if rc != 0:
            raise ThermiteError(rc, (lib().thm_last_error(None) or b"").decode())
        self.h = h
        if t.get("names") and "tx_ids" in t:
            self.set_names(t["names"], t["tx_ids"], t["gene_ids"], t["gene_names"])

    @property
    def coord_bytes(self):
        return lib().thm_index_coord_bytes(self.h)

    def suffix_array(self):
        n = lib().thm_index_text_len(self.h)
        if self.coord_bytes == 8:
            return _copy(lib().thm_index_suffix_array64(self.h), n, "<u8")
        return _copy(lib().thm_index_suffix_array(self.h), n, "<u4")

    def check_lut(self):
        """test hook: the k-mer table (built by counting) equals the one read off the suffix array"""
        return lib().thm_debug_check_lut(self.h) == 0

    def debug_host_lut(self):
        """test hook: the host's k-mer prefix table, 4^kt rows of (lo, hi) in the index's coordinate width"""
        kt = C.c_uint32()
        if lib().thm_debug_host_lut(self.h, C.byref(kt), None, 0) != 0:
            raise ThermiteError(ERR_INTERNAL, "thm_debug_host_lut")
        out = np.zeros((4 ** kt.value, 2), "<u8" if self.coord_bytes == 8 else "<u4")
        if lib().thm_debug_host_lut(self.h, C.byref(kt), _ptr(out), out.nbytes) != 0:
            raise ThermiteError(ERR_INTERNAL, "thm_debug_host_lut")
        return out

    HOST_TABLES = ("ref_bin", "ref_recs", "exon_grid_off", "exon_grid", "gene_grid_off", "gene_grid")

    def debug_host_table(self, name):
        """test hook: one of HOST_TABLES as the extend stage's kernels get it (raw bytes, the index's coordinate width)"""
        which = self.HOST_TABLES.index(name)
        n = C.c_uint64()
        if lib().thm_debug_host_table(self.h, which, None, 0, C.byref(n)) != 0:
            raise ThermiteError(ERR_INTERNAL, "thm_debug_host_table")
        out = np.zeros(n.value, np.uint8)
        if lib().thm_debug_host_table(self.h, which, _ptr(out), out.nbytes, C.byref(n)) != 0:
            raise ThermiteError(ERR_INTERNAL, "thm_debug_host_table")
        return out

    def idx_to_ref(self, idx):
        off = C.c_uint64()
        r = lib().thm_index_idx_to_ref(self.h, idx, C.byref(off))
        if r < 0:
            raise ThermiteError(r, "idx_to_ref")
        return r, off.value

    def close(self):
        if getattr(self, "h", None):
            lib().thm_index_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class BatchResult:
    """Canonical host result of one aligned batch: thm_batch_view copied out, or (copy=False) numpy views of the
    aligner's pinned result set itself -- what a C caller gets; valid until the second fetch after this one
    (include/thermite.h, thm_batch_view)."""

    def __init__(self, view, copy=True):
        self.n_reads = view.n_reads
        self.offsets = _copy(view.read_aln_off, view.n_reads + 1, "<u8", copy)
        self.alns = _copy(view.alns, view.n_alns, ALN_DT, copy)
        self.ops = _copy(view.ops, view.n_op_bytes, np.uint8, copy)
        self.n_failed = view.n_failed_reads
        # per-read status (0 = ok); None when every read is ok
        self.status = _copy(view.read_status, view.n_reads, "<i4", copy) if view.read_status else None


class CigarResult:
    """thm_cigar_view copied out, or (copy=False) numpy views of the aligner's pinned result set: records, one digest
    (DIGEST_DT) per alignment and the pool of BAM-encoded CIGAR words; no op bytes.  For cigar_encode_batch there are
    no reads and no records: one digest per stream."""

    def __init__(self, view, copy=True):
        self.n_reads = view.n_reads
        self.offsets = _copy(view.read_aln_off, view.n_reads + 1, "<u8", copy) if view.read_aln_off else None
        self.alns = _copy(view.alns, view.n_alns, ALN_DT, copy) if view.alns else None
        self.digests = _copy(view.digests, view.n_alns, DIGEST_DT, copy)
        self.cigar = _copy(view.cigar, view.n_cigar_words, "<u4", copy)
        self.n_failed = view.n_failed_reads
        self.status = _copy(view.read_status, view.n_reads, "<i4", copy) if view.read_status else None

    @property
    def nbytes(self):
        """bytes the fetch moved to the host"""
        return sum(a.nbytes for a in (self.offsets, self.alns, self.digests, self.cigar, self.status) if a is not None)

    def words(self, i, tx=False):
        """the genome (or transcript) CIGAR words of alignment i"""
        d = self.digests[i]
        o = int(d["cigar_off"]) + (int(d["n_cigar"]) if tx else 0)
        return self.cigar[o: o + int(d["n_tx_cigar"] if tx else d["n_cigar"])]


class BamResult:
    """thm_bam_view copied out, or (copy=False) numpy views of the aligner's pinned result set: the BAM records of the
    batch back to back (no header, no BGZF framing) and the byte offset of every read's first record."""

    def __init__(self, view, copy=True):
        self.n_reads = view.n_reads
        self.n_records = view.n_records
        self.data = _copy(view.data, view.n_bytes, np.uint8, copy)
        self.read_rec_off = _copy(view.read_rec_off, view.n_reads + 1, "<u8", copy)
        self.n_failed = view.n_failed_reads
        self.status = _copy(view.read_status, view.n_reads, "<i4", copy) if view.read_status else None

    @property
    def nbytes(self):
        """bytes the fetch moved to the host"""
        return sum(a.nbytes for a in (self.data, self.read_rec_off, self.status) if a is not None)

    def records(self, r):
        """the records of read r as byte strings, each beginning with its block_size"""
        b = self.data[int(self.read_rec_off[r]): int(self.read_rec_off[r + 1])].tobytes()
        out, at = [], 0
        while at < len(b):
            n = 4 + int.from_bytes(b[at: at + 4], "little")
            out.append(b[at: at + n])
            at += n
        return out


class BgzfResult:
    """thm_bgzf_view copied out, or (copy=False) numpy views of the aligner's pinned result set: the BAM records of the
    batch as complete BGZF members back to back (no BAM header, no end-of-file block) and the byte offset of every member."""

    def __init__(self, view, copy=True):
        self.n_reads = view.n_reads
        self.n_records = view.n_records
        self.n_raw_bytes = view.n_raw_bytes
        self.n_blocks = view.n_blocks
        self.data = _copy(view.data, view.n_bytes, np.uint8, copy)
        self.block_off = _copy(view.block_off, view.n_blocks + 1, "<u8", copy)
        self.n_failed = view.n_failed_reads
        self.status = _copy(view.read_status, view.n_reads, "<i4", copy) if view.read_status else None

    @property
    def nbytes(self):
        """bytes the fetch moved to the host"""
        return sum(a.nbytes for a in (self.data, self.block_off, self.status) if a is not None)

    def block(self, b):
        """member b as a byte string"""
        return self.data[int(self.block_off[b]): int(self.block_off[b + 1])].tobytes()


class SortedWindow:
    """thm_bam_sorted_view copied out: one window of the sorted stream, as BGZF members (block_off) or raw record bytes"""

    def __init__(self, view, copy=True):
        self.total_records, self.total_raw_bytes = view.total_records, view.total_raw_bytes
        self.raw_offset, self.n_raw_bytes = view.raw_offset, view.n_raw_bytes
        self.n_blocks, self.n_bytes = view.n_blocks, view.n_bytes
        self.data = _copy(view.data, view.n_bytes, np.uint8, copy)
        self.block_off = _copy(view.block_off, view.n_blocks + 1, "<u8", copy) if view.block_off else None
        self.gather_ms, self.deflate_ms = view.gather_ms, view.deflate_ms


class BamSorter:
    """thm_bam_sorter: the BAM records of every batch of a run kept on the aligner's device, sorted by coordinate at the
    end and handed out window by window.  Close it before its aligner."""

    def __init__(self, aligner, max_bytes=0):
        self.aligner = aligner
        h = C.c_void_p()
        rc = lib().thm_bam_sorter_create(aligner.h, max_bytes, C.byref(h))
        if rc != 0:
            raise ThermiteError(rc, (lib().thm_last_error(None) or b"").decode())
        self.h = h

    def add(self, flags=0):
        """thm_bam_sorter_add, after Aligner.run -> the info as a dict (`status`: the per-read statuses, or None)"""
        info = BamSortInfo()
        self.aligner._chk(lib().thm_bam_sorter_add(self.h, flags, C.byref(info)))
        out = {k: getattr(info, k) for k, _ in BamSortInfo._fields_ if k != "read_status"}
        out["status"] = _copy(info.read_status, info.n_reads, np.int32) if info.read_status else None
        return out

    def add_records(self, data):
        """test hook: caller-made records through the same key kernel and arena"""
        src = _u8(data)
        self.aligner._chk(lib().thm_debug_bam_sorter_add_records(self.h, _ptr(src) if len(src) else None, len(src)))

    def gather_shape(self, shape=None):
        """test / tuning hook: "pieces" (16 bytes a lane) or "records" (a wavefront per record) for the next windows (None
        only asks) -> the shape in use before the call; a new sorter starts with "records" unless THM_SORT_GATHER=pieces"""
        was = lib().thm_debug_bam_sorter_gather(self.h, {None: -1, "pieces": 0, "records": 1}[shape])
        return ("pieces", "records")[was]

    def finish(self):
        """thm_bam_sorter_finish -> the sort's milliseconds"""
        ms = C.c_float(0)
        self.aligner._chk(lib().thm_bam_sorter_finish(self.h, C.byref(ms)))
        return ms.value

    def next(self, max_raw_bytes=0, raw=False, copy=True):
        v = BamSortedView()
        self.aligner._chk(lib().thm_bam_sorter_next(self.h, max_raw_bytes, SORT_RAW if raw else 0, C.byref(v)))
        return SortedWindow(v, copy)

    def windows(self, max_raw_bytes=0, raw=False):
        """every window of the sorted stream that is left, in order"""
        while True:
            w = self.next(max_raw_bytes, raw)
            if w.n_raw_bytes == 0:
                return
            yield w

    def index(self, first_member_offset):
        """thm_bam_sorter_index, once the windows are exhausted -> (the .bai file's bytes, the view's counts and index_ms)"""
        v = BaiView()
        self.aligner._chk(lib().thm_bam_sorter_index(self.h, first_member_offset, C.byref(v)))
        info = {k: getattr(v, k) for k, _ in BaiView._fields_ if k != "data"}
        return _copy(v.data, v.n_bytes, np.uint8).tobytes(), info

    def close(self):
        if getattr(self, "h", None):
            lib().thm_bam_sorter_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class QuantResult:
    """thm_quant_view copied out: the gene table (QUANT_GENE_DT, one row per gene of the index), the junction table
    (QUANT_JUNCTION_DT, sorted) and the totals as a dict"""

    def __init__(self, view):
        self.genes = _copy(view.genes, view.n_genes, QUANT_GENE_DT)
        self.junctions = _copy(view.junctions, view.n_junctions, QUANT_JUNCTION_DT)
        self.totals = view.totals.as_dict()
        self.fetch_ms = view.fetch_ms


def _cigar_view(offsets, alns, digests, cigar, status):
    """caller-made arrays (ALN_DT, DIGEST_DT, CIGAR words) -> the CigarView over them, and the arrays it points into:
    they must stay alive while the view is used"""
    off = np.ascontiguousarray(offsets, dtype="<u8")
    al = np.ascontiguousarray(alns, dtype=ALN_DT)
    dg = np.ascontiguousarray(digests, dtype=DIGEST_DT)
    cg = np.ascontiguousarray(cigar, dtype="<u4")
    st = np.ascontiguousarray(status, dtype="<i4") if status is not None else None
    n_reads = max(len(off) - 1, 0)
    v = CigarView(n_reads, len(al), len(cg), _ptr(off) if len(off) else None, _ptr(al) if len(al) else None,
                  _ptr(dg) if len(dg) else None, _ptr(cg) if len(cg) else None,
                  int((st != 0).sum()) if st is not None else 0, _ptr(st) if st is not None and len(st) else None)
    return v, (off, al, dg, cg, st)


class _RunSummary:
    """What Quant, Coverage and Pileup share: the handle of an object that accumulates over the batches of its aligner.
    A subclass names its C functions (_NAME: thm_<_NAME>_create, _add, _add_view, _reset, _free), its info struct (_INFO)
    and the fields of that struct its add and add_view (through _add) return beside the batch's totals (_INFO_FIELDS)."""

    _NAME = _INFO = None
    _INFO_FIELDS = ()

    def __init__(self, aligner, *create_args):
        self.aligner = aligner
        h = C.c_void_p()
        rc = self._fn("create")(aligner.h, *create_args, C.byref(h))
        if rc != 0:
            raise ThermiteError(rc, (lib().thm_last_error(aligner.h) or b"").decode())
        self.h = h

    @classmethod
    def _fn(cls, what):
        return getattr(lib(), "thm_%s_%s" % (cls._NAME, what))

    def _add(self, what, *args):
        info = self._INFO()
        self.aligner._chk(self._fn(what)(self.h, *args, C.byref(info)))
        out = info.batch.as_dict()
        out.update({k: int(getattr(info, k)) for k in self._INFO_FIELDS}, held_bytes=int(info.held_bytes), add_ms=info.add_ms)
        return out

    def reset(self):
        self.aligner._chk(self._fn("reset")(self.h))

    def close(self):
        if getattr(self, "h", None):
            self._fn("free")(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Quant(_RunSummary):
    """thm_quant: gene and splice-junction count tables of a run, accumulated on the aligner's device batch by batch.
    Close it before its aligner."""

    _NAME, _INFO, _INFO_FIELDS = "quant", QuantInfo, ("n_junctions",)

    def __init__(self, aligner):
        super().__init__(aligner)

    def add(self):
        """thm_quant_add, after Aligner.run -> the batch's totals, n_junctions, held_bytes and add_ms as a dict"""
        return self._add("add")

    def add_view(self, offsets, alns, digests, cigar, status=None):
        """thm_quant_add_view: the same kernels over caller-made arrays (ALN_DT, DIGEST_DT, CIGAR words)"""
        v, _alive = _cigar_view(offsets, alns, digests, cigar, status)
        return self._add("add_view", C.byref(v))

    def fetch(self):
        v = QuantView()
        self.aligner._chk(lib().thm_quant_fetch(self.h, C.byref(v)))
        return QuantResult(v)


class CoverageResult:
    """thm_cov_view copied out: the runs (COV_RUN_DT, ascending by ref_id, start), max_depth, n_covered, n_bases and the
    object's totals as a dict"""

    def __init__(self, view):
        self.track, self.first_ref, self.n_refs = int(view.track), int(view.first_ref), int(view.n_refs)
        self.runs = _copy(view.runs, view.n_runs, COV_RUN_DT)
        self.max_depth, self.n_covered, self.n_bases = int(view.max_depth), int(view.n_covered), int(view.n_bases)
        self.totals = view.totals.as_dict()
        self.fetch_ms = view.fetch_ms


class Coverage(_RunSummary):
    """thm_coverage: per-base coverage tracks of a run, accumulated on the aligner's device batch by batch.  Close it
    before its aligner."""

    _NAME, _INFO = "coverage", CovInfo

    def __init__(self, aligner, flags=0, max_bytes=0):
        self.flags = flags
        self.n_tracks = (2 if flags & COV_STRANDED else 1) * (2 if flags & COV_MULTI else 1)
        super().__init__(aligner, flags, max_bytes)

    def add(self):
        """thm_coverage_add, after Aligner.run -> the batch's totals, held_bytes and add_ms as a dict"""
        return self._add("add")

    def add_view(self, offsets, alns, digests, cigar, status=None):
        """thm_coverage_add_view: the same kernels over caller-made arrays (ALN_DT, DIGEST_DT, CIGAR words)"""
        v, _alive = _cigar_view(offsets, alns, digests, cigar, status)
        return self._add("add_view", C.byref(v))

    def fetch(self, track, first_ref, n_refs):
        """thm_coverage_fetch: the runs of `track` on the @SQ entries [first_ref, first_ref + n_refs)"""
        v = CovView()
        self.aligner._chk(lib().thm_coverage_fetch(self.h, track, first_ref, n_refs, C.byref(v)))
        return CoverageResult(v)

    def depth(self, track, ref_id, start, n):
        """thm_coverage_depth -> uint32[n]; the call's depth_ms is left in self.depth_ms"""
        v = CovDepthView()
        self.aligner._chk(lib().thm_coverage_depth(self.h, track, ref_id, start, n, C.byref(v)))
        self.depth_ms = v.depth_ms
        return _copy(v.depth, v.n, np.dtype("<u4"))


class PileupResult:
    """thm_pile_view copied out: the sites (PILE_SITE_DT, ascending by ref_id, pos), n_events and the object's totals as a dict"""

    def __init__(self, view):
        self.first_ref, self.n_refs, self.min_alt = int(view.first_ref), int(view.n_refs), int(view.min_alt)
        self.sites = _copy(view.sites, view.n_sites, PILE_SITE_DT)
        self.n_events = int(view.n_events)
        self.totals = view.totals.as_dict()
        self.fetch_ms = view.fetch_ms


class Pileup(_RunSummary):
    """thm_pileup: per-base allele counts of a run, accumulated on the aligner's device batch by batch.  Close it before
    its aligner."""

    _NAME, _INFO, _INFO_FIELDS = "pileup", PileInfo, ("n_events",)

    def __init__(self, aligner, flags=0, max_bytes=0):
        self.flags = flags
        super().__init__(aligner, flags, max_bytes)

    def add(self):
        """thm_pileup_add, after Aligner.run -> the batch's totals, n_events, held_bytes and add_ms as a dict"""
        return self._add("add")

    def add_view(self, offsets, alns, digests, cigar, bases, base_off, status=None):
        """thm_pileup_add_view: the same kernels over caller-made arrays (ALN_DT, DIGEST_DT, CIGAR words) and the reads' bytes"""
        v, _alive = _cigar_view(offsets, alns, digests, cigar, status)
        bs = np.ascontiguousarray(bases, dtype=np.uint8)
        bo = np.ascontiguousarray(base_off, dtype="<u8")
        return self._add("add_view", C.byref(v), _ptr(bs) if len(bs) else None, _ptr(bo) if len(bo) else None)

    def fetch(self, first_ref, n_refs, min_alt=1):
        """thm_pileup_fetch: the sites of the @SQ entries [first_ref, first_ref + n_refs) with min_alt events or more"""
        v = PileView()
        self.aligner._chk(lib().thm_pileup_fetch(self.h, first_ref, n_refs, min_alt, C.byref(v)))
        return PileupResult(v)

    def window(self, ref_id, start, n):
        """thm_pileup_window: a row for every position of [start, start + n) of one contig"""
        v = PileView()
        self.aligner._chk(lib().thm_pileup_window(self.h, ref_id, start, n, C.byref(v)))
        return PileupResult(v)


class CellsResult:
    """thm_cells_view copied out: the cells (CELL_DT, ascending by barcode), the entries (CELL_ENTRY_DT, ascending by cell,
    gene), the object's counts and its totals as a dict"""

    def __init__(self, view):
        self.cb_len, self.umi_len, self.min_umis = int(view.cb_len), int(view.umi_len), int(view.min_umis)
        self.cells = _copy(view.cells, view.n_cells, CELL_DT)
        self.entries = _copy(view.entries, view.n_entries, CELL_ENTRY_DT)
        self.n_molecules, self.n_barcodes, self.n_cells_below = int(view.n_molecules), int(view.n_barcodes), int(view.n_cells_below)
        self.totals = view.totals.as_dict()
        self.fetch_ms = view.fetch_ms


class Cells(_RunSummary):
    """thm_cells: the cell-by-gene matrix of distinct molecules of a run, accumulated on the aligner's device batch by
    batch from the (barcode, UMI) tags of the read names.  Close it before its aligner."""

    _NAME, _INFO, _INFO_FIELDS = "cells", CellsInfo, ("n_molecules", "n_pending")

    def __init__(self, aligner, flags=0, cb_len=16, umi_len=12, max_bytes=0):
        self.flags, self.cb_len, self.umi_len = flags, cb_len, umi_len
        super().__init__(aligner, flags, cb_len, umi_len, max_bytes)

    def add(self):
        """thm_cells_add, after Aligner.run of a batch with names -> the batch's totals, n_molecules, n_pending, held_bytes
        and add_ms as a dict"""
        return self._add("add")

    def add_view(self, offsets, alns, digests, cigar, names, name_off, status=None):
        """thm_cells_add_view: the same kernels over caller-made arrays (ALN_DT, DIGEST_DT, CIGAR words) and the reads' names"""
        v, _alive = _cigar_view(offsets, alns, digests, cigar, status)
        nm = _u8(names)
        no = np.ascontiguousarray(name_off, dtype="<u8")
        return self._add("add_view", C.byref(v), _ptr(nm) if len(nm) else None, _ptr(no) if len(no) else None)

    def fetch(self, min_umis=1):
        """thm_cells_fetch: the cells with min_umis distinct molecules or more, and their (cell, gene) entries"""
        v = CellsView()
        self.aligner._chk(lib().thm_cells_fetch(self.h, min_umis, C.byref(v)))
        return CellsResult(v)


def cigar_text(words):
    """BAM CIGAR words -> SAM text ('*' when there are none)"""
    return "".join("%d%s" % (int(w) >> 4, "MIDNSHP=X"[int(w) & 15]) for w in words) or "*"


class Aligner:
    """thm_aligner: mirrors the reference's per-thread aligner handle
    (ThermiteAligner, src/wrapper.rs:20-27; align_read, src/aligner.rs:123)."""

    def __init__(self, index, opts=None, device=0):
        self.index = index
        o = dict(DEFAULT_OPTS)
        o.update(opts or {})
        self._opts = self._mk(o)
        h = C.c_void_p()
        rc = lib().thm_aligner_create(index.h, C.byref(self._opts), device, C.byref(h))
        if rc != 0:
            raise ThermiteError(rc, (lib().thm_last_error(None) or b"").decode())
        self.h = h

    @staticmethod
    def _mk(o):
        return Opts(o["min_seed_len"], o["min_aln_score_percent"], o["min_aln_score"], o["multimap_score_range"],
                    int(bool(o["intron_mode"])), 0)

    def _chk(self, rc):
        if rc != 0:
            raise ThermiteError(rc, (lib().thm_last_error(self.h) or b"").decode())

    def set_opts(self, opts):
        o = dict(DEFAULT_OPTS)
        o.update(opts)
        self._opts = self._mk(o)
        self._chk(lib().thm_aligner_set_opts(self.h, C.byref(self._opts)))

    @property
    def stream(self):
        return lib().thm_aligner_stream(self.h)

    def align_batch(self, bases, offsets, copy=True):
        bases, offsets = _u8(bases), np.ascontiguousarray(offsets, "<u8")
        v = BatchView()
        self._chk(lib().thm_align_batch(self.h, _ptr(bases), _ptr(offsets), len(offsets) - 1, C.byref(v)))
        return BatchResult(v, copy)

    def upload(self, bases, offsets):
        bases, offsets = _u8(bases), np.ascontiguousarray(offsets, "<u8")
        self._chk(lib().thm_batch_upload(self.h, _ptr(bases), _ptr(offsets), len(offsets) - 1))

    def run(self):
        self._chk(lib().thm_batch_run(self.h))

    def sync(self):
        self._chk(lib().thm_batch_sync(self.h))

    def fetch(self, copy=True):
        v = BatchView()
        self._chk(lib().thm_batch_fetch(self.h, C.byref(v)))
        return BatchResult(v, copy)

    def fetch_cigars(self, copy=True):
        """thm_batch_fetch_cigars: the run's records with digests and CIGAR words instead of op bytes"""
        v = CigarView()
        self._chk(lib().thm_batch_fetch_cigars(self.h, C.byref(v)))
        return CigarResult(v, copy)

    def align_batch_cigars(self, bases, offsets, copy=True):
        bases, offsets = _u8(bases), np.ascontiguousarray(offsets, "<u8")
        v = CigarView()
        self._chk(lib().thm_align_batch_cigars(self.h, _ptr(bases), _ptr(offsets), len(offsets) - 1, C.byref(v)))
        return CigarResult(v, copy)

    def upload_reads(self, batch):
        """thm_batch_upload_reads: `batch` is a dict as from FastqReader.next_batch (quals may be None)"""
        rb, keep = read_batch_struct(batch)
        self._chk(lib().thm_batch_upload_reads(self.h, C.byref(rb)))

    def fetch_bam(self, flags=0, copy=True):
        """thm_batch_fetch_bam: the run's BAM records, encoded on the device"""
        v = BamView()
        self._chk(lib().thm_batch_fetch_bam(self.h, flags, C.byref(v)))
        return BamResult(v, copy)

    def align_batch_bam(self, batch, flags=0, copy=True):
        rb, keep = read_batch_struct(batch)
        v = BamView()
        self._chk(lib().thm_align_batch_bam(self.h, C.byref(rb), flags, C.byref(v)))
        return BamResult(v, copy)

    def fetch_bgzf(self, flags=0, copy=True):
        """thm_batch_fetch_bgzf: the run's BAM records, encoded and BGZF-compressed on the device"""
        v = BgzfView()
        self._chk(lib().thm_batch_fetch_bgzf(self.h, flags, C.byref(v)))
        return BgzfResult(v, copy)

    def align_batch_bgzf(self, batch, flags=0, copy=True):
        rb, keep = read_batch_struct(batch)
        v = BgzfView()
        self._chk(lib().thm_align_batch_bgzf(self.h, C.byref(rb), flags, C.byref(v)))
        return BgzfResult(v, copy)

    def upload_fastq(self, raw, path=b"", first_line=1, last_block=True):
        """thm_batch_upload_fastq: a block of whole FASTQ records as raw bytes -> the info as a dict (on_device: 1 when the
        device parsed it, 0 when it went through the host parser)"""
        src = np.frombuffer(bytes(raw), np.uint8) if len(raw) else None
        info = FastqUploadInfo()
        self._chk(lib().thm_batch_upload_fastq(self.h, _ptr(src), len(raw), os.fsencode(path), first_line, int(bool(last_block)),
                                               C.byref(info)))
        return {k: getattr(info, k) for k, _ in FastqUploadInfo._fields_}

    def fetch_reads(self):
        """thm_batch_fetch_reads: the uploaded batch as the dict FastqReader.next_batch gives"""
        v = ReadBatch()
        self._chk(lib().thm_batch_fetch_reads(self.h, C.byref(v)))
        off = _copy(v.offsets, v.n_reads + 1, "<u8")
        noff = _copy(v.name_off, v.n_reads + 1, "<u8")
        return dict(bases=_copy(v.bases, v.n_bases, np.uint8), offsets=off,
                    quals=_copy(v.quals, v.n_bases, np.uint8) if v.quals else None,
                    names=_copy(v.names, int(noff[-1]), np.uint8), name_off=noff)

    def debug_fastq_device_blocks(self):
        """test hook: blocks upload_fastq (and the file driver with THM_FASTQ_DEVICE=1) parsed (on the device, on the host)"""
        d, h = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().thm_debug_fastq_device_blocks(self.h, C.byref(d), C.byref(h)))
        return d.value, h.value

    def upload_fastq_bgzf(self, members, head=b"", path=b"", first_line=1, last_block=True):
        """thm_batch_upload_fastq_bgzf: head ++ the inflated gzip members as a block of FASTQ -> the info as a dict, `tail`
        (the block's bytes behind the batch: the head of the next call) as bytes"""
        m = np.frombuffer(bytes(members), np.uint8) if len(members) else None
        h = np.frombuffer(bytes(head), np.uint8) if len(head) else None
        info = FastqBgzfInfo()
        self._chk(lib().thm_batch_upload_fastq_bgzf(self.h, _ptr(h), len(head), _ptr(m), len(members), os.fsencode(path), first_line,
                                                    int(bool(last_block)), C.byref(info)))
        out = {k: getattr(info, k) for k, _ in FastqBgzfInfo._fields_}
        out["tail"] = C.string_at(info.tail, info.tail_len) if info.tail_len else b""
        return out

    def upload_fastq_gzip(self, state, data, head=b"", path=b"", first_line=1, last_block=True):
        """thm_batch_upload_fastq_gzip: `data`, bytes of a gzip stream that begin where `state` (a GzipState, moved on in
        place) says -> the info as a dict, `tail` as bytes"""
        m = np.frombuffer(bytes(data), np.uint8) if len(data) else None
        h = np.frombuffer(bytes(head), np.uint8) if len(head) else None
        info = FastqGzipInfo()
        self._chk(lib().thm_batch_upload_fastq_gzip(self.h, C.byref(state), _ptr(h), len(head), _ptr(m), len(data), os.fsencode(path),
                                                    first_line, int(bool(last_block)), C.byref(info)))
        out = {k: getattr(info, k) for k, _ in FastqGzipInfo._fields_}
        out["tail"] = C.string_at(info.tail, info.tail_len) if info.tail_len else b""
        return out

    def debug_gzip_inflate(self, state, data, chunk_bytes=0, last_block=True, cap=None):
        """test hook: bytes of a gzip stream through the device inflater alone (no host inflater behind it), in chunks
        of chunk_bytes (0: the default) -> (the inflated bytes, n_consumed, (n_chunks, n_starts, refused starts, path
        flags)); `state` moves on in place; a stream the device declines raises"""
        src = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
        out = np.empty((16 * len(data) + 65536 if cap is None else cap) + 64, np.uint8)
        n, used = C.c_uint64(0), C.c_uint64(0)
        counts = (C.c_uint64 * 4)()
        self._chk(lib().thm_debug_gzip_inflate(self.h, C.byref(state), src.ctypes.data, len(data), chunk_bytes, int(bool(last_block)),
                                               out.ctypes.data, len(out), C.byref(n), C.byref(used), counts))
        return out[: n.value].tobytes(), used.value, tuple(int(x) for x in counts)

    def debug_fastq_gzip_blocks(self):
        """test hook: what upload_fastq_gzip did so far: (inflates on the device, on the host, parses on the device, on the host)"""
        c = (C.c_uint64 * 4)()
        self._chk(lib().thm_debug_fastq_gzip_blocks(self.h, c))
        return tuple(int(x) for x in c)

    def debug_bgzf_inflate(self, members, cap=None):
        """test hook: gzip members through the device inflater alone (no host inflater behind it) -> the inflated bytes;
        a chain the device does not take, or a member it declines, raises"""
        src = np.frombuffer(bytes(members), np.uint8) if len(members) else np.zeros(1, np.uint8)
        out = np.empty((65536 * (len(members) // 27 + 1) if cap is None else cap) + 64, np.uint8)
        n = C.c_uint64(0)
        self._chk(lib().thm_debug_bgzf_inflate(self.h, src.ctypes.data, len(members), out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].tobytes()

    def debug_fastq_bgzf_blocks(self):
        """test hook: what upload_fastq_bgzf did so far: (inflates on the device, on the host, parses on the device, on the host)"""
        c = (C.c_uint64 * 4)()
        self._chk(lib().thm_debug_fastq_bgzf_blocks(self.h, c))
        return tuple(int(x) for x in c)

    def debug_bgzf_device(self, data):
        """test hook: bytes through the device BGZF encoder -> (the members back to back, their number)"""
        src = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
        out = np.empty(len(data) + 31 * (len(data) // 0xff00 + 1) + 64, np.uint8)
        n, nb = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().thm_debug_bgzf_device(self.h, src.ctypes.data, len(data), out.ctypes.data, len(out), C.byref(n), C.byref(nb)))
        return out[: n.value].tobytes(), nb.value

    def cigar_encode_batch(self, ops, off):
        """thm_cigar_encode_batch: serialised op streams ops[off[i]:off[i+1]] -> CigarResult, one digest per stream"""
        ops, off = _u8(ops), np.ascontiguousarray(off, "<u8")
        v = CigarView()
        self._chk(lib().thm_cigar_encode_batch(self.h, _ptr(ops), _ptr(off), len(off) - 1, C.byref(v)))
        return CigarResult(v)

    def smems_batch(self, bases, offsets, min_seed_len):
        bases, offsets = _u8(bases), np.ascontiguousarray(offsets, "<u8")
        v = MemsView()
        self._chk(lib().thm_smems_batch(self.h, _ptr(bases), _ptr(offsets), len(offsets) - 1, min_seed_len, C.byref(v)))
        return _copy(v.read_mem_off, v.n_reads + 1, "<u8"), _copy(v.mems, v.n_mems, MEM_DT)

    def swg_extend_batch(self, x_bases, x_off, y_bases, y_off, bw, xd, max_bw):
        xb, yb = _u8(x_bases), _u8(y_bases)
        xo, yo = np.ascontiguousarray(x_off, "<u8"), np.ascontiguousarray(y_off, "<u8")
        bw, xd = np.ascontiguousarray(bw, "<u4"), np.ascontiguousarray(xd, "<i4")
        v = SwgView()
        self._chk(lib().thm_swg_extend_batch(self.h, _ptr(xb), _ptr(xo), _ptr(yb), _ptr(yo), _ptr(bw), _ptr(xd),
                                             max_bw, len(bw), C.byref(v)))
        return _copy(v.alns, v.n, SWG_DT), _copy(v.ops, v.n_op_bytes, np.uint8)

    def extend_left_right_batch(self, x_bases, x_off, y_bases, y_off, hits, bw, xd, max_bw):
        """extend_left_right (reference src/aligner.rs:352-407) per problem: read i = x_bases[x_off[i]:x_off[i+1]],
        reference sequence i = y_bases[y_off[i]:y_off[i+1]], hits[i] (MEM_DT, relative to both).  Returns (LR_DT
        records, op bytes); ops_off indexes the op bytes."""
        xb, yb = _u8(x_bases), _u8(y_bases)
        xo, yo = np.ascontiguousarray(x_off, "<u8"), np.ascontiguousarray(y_off, "<u8")
        hits = np.ascontiguousarray(hits, MEM_DT)
        bw, xd = np.ascontiguousarray(bw, "<u4"), np.ascontiguousarray(xd, "<i4")
        v = LrView()
        self._chk(lib().thm_extend_left_right_batch(self.h, _ptr(xb), _ptr(xo), _ptr(yb), _ptr(yo), _ptr(hits), _ptr(bw),
                                                    _ptr(xd), max_bw, len(bw), C.byref(v)))
        return _copy(v.alns, v.n, LR_DT), _copy(v.ops, v.n_op_bytes, np.uint8)

    def align_seed_hits(self, bases, offsets, hit_off, hits, band_width, x_drop, max_band_width):
        """align_seed_hit (reference src/aligner.rs:198-314) for each hit: hits[hit_off[r]:hit_off[r+1]] (MEM_DT,
        concatenated coordinates) belong to read r -- a smems_batch result passes unchanged.  Returns (ALN_DT records in
        hit order, op bytes, per-hit status int32 array: 0 = ok, ERR_OUT_OF_CONTRACT, ERR_UNSUPPORTED)."""
        bases, offsets = _u8(bases), np.ascontiguousarray(offsets, "<u8")
        hit_off, hits = np.ascontiguousarray(hit_off, "<u8"), np.ascontiguousarray(hits, MEM_DT)
        bw, xd = np.ascontiguousarray(band_width, "<u4"), np.ascontiguousarray(x_drop, "<i4")
        if not (len(hits) == len(bw) == len(xd)):
            raise ThermiteError(ERR_INVALID_ARG, "hits, band_width and x_drop differ in length")
        v = HitsView()
        self._chk(lib().thm_align_seed_hits_batch(self.h, _ptr(bases), _ptr(offsets), len(offsets) - 1, _ptr(hit_off),
                                                  _ptr(hits), len(hits), _ptr(bw), _ptr(xd), max_band_width, C.byref(v)))
        status = (_copy(v.hit_status, v.n_hits, "<i4") if v.hit_status else np.zeros(int(v.n_hits), "<i4"))
        return _copy(v.alns, v.n_hits, ALN_DT), _copy(v.ops, v.n_op_bytes, np.uint8), status

    def counters(self):
        out = np.zeros(N_COUNTERS, "<u8")
        self._chk(lib().thm_counters_get(self.h, _ptr(out)))
        return out

    def reset_counters(self):
        self._chk(lib().thm_counters_reset(self.h))

    def counters_allreduce(self, comm):
        """sum the device counters over all ranks of `comm` (RCCL), in place"""
        self._chk(lib().thm_counters_allreduce(self.h, comm.h))

    def counters_device_ptr(self):
        return lib().thm_counters_device_ptr(self.h)

    def timings(self):
        out = np.zeros(N_TIMINGS, "<f4")
        self._chk(lib().thm_timings_get(self.h, _ptr(out)))
        return dict(zip(TIMING_NAMES, out.tolist()))

    def debug_prof(self, reset=True):
        out = np.zeros(16, "<u8")
        self._chk(lib().thm_debug_prof_get(self.h, _ptr(out), int(reset)))
        return out

    def debug_set_pool_caps(self, smem_cap=0, cand_cap=0, ops_cap=0):
        """test hook: initial pool sizes for the next batches; returns the replay count so far"""
        n = C.c_uint32()
        self._chk(lib().thm_debug_set_pool_caps(self.h, smem_cap, cand_cap, ops_cap, C.byref(n)))
        return n.value

    def debug_set_flags(self, tpr=None, rounds=0, seed_infer=None, seed_stats=None, seed_direct=None, finish_exact=None,
                        finish_subst=None, seed_bounds=None):
        """test / tuning hook: tpr = False: every read takes the wave-per-read kernels, True: the problem-parallel path
        in front of them (None: keep); rounds = its request rounds (1..8, 0: keep); seed_infer = False: no seed probe
        is decided from its table entry and a neighbouring match (bit 2 of the word; True: bit 4, on again);
        seed_stats = True: the seed kernels count their probes for debug_seed_stats (bit 3; False: bit 5);
        seed_direct = False: a probe into a single-suffix bucket reads the suffix array although its table entry holds
        the text position (bit 6; True: bit 7, the position is used again); finish_exact = False: the finisher in front
        of the extend kernel leaves whole-read exact matches (class E) to it (bit 12; True: bit 13, it takes them);
        finish_subst: the same for reads with one substitution between two SMEMs (class S, bits 14 / 15);
        seed_bounds = False: the seed stage probes every inner position of a grid cell whose two grid points do not
        share a stored end, as it did before it used the bounds of the grid probes (bit 16; True: bit 17).  None: keep."""
        word = (0 if tpr is None else (2 if tpr else 1)) | (int(rounds) << 8)
        word |= 0 if seed_infer is None else (16 if seed_infer else 4)
        word |= 0 if seed_stats is None else (8 if seed_stats else 32)
        word |= 0 if seed_direct is None else (128 if seed_direct else 64)
        word |= 0 if finish_exact is None else (0x2000 if finish_exact else 0x1000)
        word |= 0 if finish_subst is None else (0x8000 if finish_subst else 0x4000)
        word |= 0 if seed_bounds is None else (0x20000 if seed_bounds else 0x10000)
        self._chk(lib().thm_debug_set_flags(self.h, word))

    def debug_seed_stats(self):
        """the last batch's seed probes (thm_debug_seed_stats): (decided from the table entry alone, run in full)"""
        out = np.zeros(2, "<u8")
        self._chk(lib().thm_debug_seed_stats(self.h, _ptr(out)))
        return int(out[0]), int(out[1])

    def debug_smem_finish_stats(self):
        """thm_debug_smem_finish_stats, the finisher in the last batch: (class E reads finished, reads of class E's shape
        left to the extend kernel, class S finished, class S left); zeros when it did not run"""
        out = np.zeros(4, "<u8")
        self._chk(lib().thm_debug_smem_finish_stats(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def debug_seed_direct_stats(self):
        """thm_debug_seed_direct_stats: (the device table holds text positions in its single-suffix entries, entries
        rewritten, full probes of the last batch that took the position from the entry, full probes into a single-suffix
        bucket that read the suffix array); the last two are counted while seed_stats is on"""
        out = np.zeros(4, "<u8")
        self._chk(lib().thm_debug_seed_direct_stats(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def debug_fetch_lut(self, like):
        """test hook: the device copy of the k-mer table as the kernels read it; `like` = Index.debug_host_lut()"""
        out = np.zeros_like(like)
        self._chk(lib().thm_debug_fetch_lut(self.h, _ptr(out), out.nbytes))
        return out

    def debug_set_band_clip(self, max_bw=None):
        """test hook: the register-resident kernels pretend to hold bands up to max_bw only (None: off)"""
        self._chk(lib().thm_debug_set_band_clip(self.h, 0 if max_bw is None else int(max_bw) + 1))

    def debug_tpr_stats(self):
        """the last run's problem-parallel path (thm_debug_tpr_stats)"""
        out = np.zeros(32, "<u8")
        self._chk(lib().thm_debug_tpr_stats(self.h, _ptr(out)))
        return out

    def debug_knobs(self):
        """what the run-time knobs resolved to in this process: the 16 words of thm_debug_knobs (knobs_dict names them)"""
        out = np.zeros(16, "<u4")
        self._chk(lib().thm_debug_knobs(self.h, _ptr(out)))
        return out

    def debug_calib_gather(self, pattern, n_threads):
        """profiling hook: a gather of known size (see tools/calib_fetch.py); returns the bytes requested"""
        b = C.c_uint64()
        self._chk(lib().thm_debug_calib_gather(self.h, pattern, n_threads, C.byref(b)))
        return b.value

    def debug_wave_prims(self, v):
        v = np.ascontiguousarray(v, "<i4")
        out = np.zeros(384, "<i4")
        self._chk(lib().thm_debug_wave_prims(self.h, _ptr(v), _ptr(out)))
        return out.reshape(6, 64)

    def close(self):
        if getattr(self, "h", None):
            lib().thm_aligner_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


KNOB_NAMES = {0: "seed_fill", 1: "compact_k", 2: "hit_gl", 11: "team_div_per_cu", 12: "swg_bpc", 13: "use_tpr", 14: "tpr_rounds",
              15: "n_cu"}


def knobs_dict(raw):
    """the 16 words of thm_debug_knobs by name"""
    d = {name: int(raw[i]) for i, name in KNOB_NAMES.items()}
    d["ext_minw"] = {(cpl, bool(wide)): int(raw[3 + 2 * (cpl - 1) + wide]) for cpl in (1, 2, 3, 4) for wide in (0, 1)}
    return d


def comm_unique_id():
    out = np.zeros(128, np.uint8)
    rc = lib().thm_comm_unique_id(_ptr(out))
    if rc != 0:
        raise ThermiteError(rc, _last_error())
    return out


class Comm:
    """thm_comm: RCCL communicator for the counter all-reduce (one rank per GPU)."""

    def __init__(self, unique_id, nranks, rank, device=0):
        uid = np.ascontiguousarray(unique_id, np.uint8)
        h = C.c_void_p()
        rc = lib().thm_comm_create(_ptr(uid), nranks, rank, device, C.byref(h))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().thm_comm_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def debug_deflate_block(data):
    """test hook: at most 65280 bytes through the BAM writer's own deflate -> one raw DEFLATE stream"""
    src = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    out = np.empty(len(data) + len(data) // 8 + 1024, np.uint8)
    n = C.c_uint64(0)
    rc = lib().thm_debug_deflate_block(src.ctypes.data, len(data), out.ctypes.data, len(out), C.byref(n))
    if rc != 0:
        raise ThermiteError(rc, _last_error())
    return out[: n.value].tobytes()


def debug_gunzip(path, chunk=1 << 20, cap=None, threads=1):
    """test hook: a gzip file through the library's own inflater, `chunk` bytes per call -> bytes
    (threads > 1: the chunk-parallel decoder, for files of at least four chunks of THM_INFLATE_CHUNK_KB)"""
    cap = cap if cap is not None else 64 * os.path.getsize(path) + (1 << 20)
    out = np.empty(cap, np.uint8)
    n = C.c_uint64(0)
    rc = lib().thm_debug_gunzip_mt(os.fsencode(str(path)), chunk, threads, out.ctypes.data, cap, C.byref(n))
    if rc != 0:
        raise ThermiteError(rc, _last_error())
    return out[: n.value].tobytes()


class FastqReader:
    """thm_fastq: FASTQ / FASTA batcher (needletail::parse_fastx_file, src/aligner.rs:51-56)."""

    def __init__(self, path):
        h = C.c_void_p()
        rc = lib().thm_fastq_open(str(path).encode(), C.byref(h))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        self.h = h

    def all_by_blocks(self, reads_per_block):
        """test hook: the whole file through the parallel driver's block cutter + block parser"""
        v = ReadBatch()
        rc = lib().thm_debug_fastq_blocks(self.h, reads_per_block, C.byref(v))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        off = _copy(v.offsets, v.n_reads + 1, "<u8")
        noff = _copy(v.name_off, v.n_reads + 1, "<u8")
        return dict(bases=_copy(v.bases, v.n_bases, np.uint8), offsets=off, quals=_copy(v.quals, v.n_bases, np.uint8),
                    names=_copy(v.names, int(noff[-1]), np.uint8), name_off=noff)

    def next_batch(self, max_reads):
        """-> dict(bases, offsets, quals (None for FASTA), names, name_off) or None at end of file"""
        v = ReadBatch()
        rc = lib().thm_fastq_next_batch(self.h, max_reads, C.byref(v))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        if v.n_reads == 0:
            return None
        off = _copy(v.offsets, v.n_reads + 1, "<u8")
        noff = _copy(v.name_off, v.n_reads + 1, "<u8")
        return dict(bases=_copy(v.bases, v.n_bases, np.uint8), offsets=off,
                    quals=_copy(v.quals, v.n_bases, np.uint8) if v.quals else None,
                    names=_copy(v.names, int(noff[-1]), np.uint8), name_off=noff)

    def close(self):
        if getattr(self, "h", None):
            lib().thm_fastq_close(self.h)
            self.h = None

    def __del__(self):
        self.close()


def read_batch_struct(batch):
    """dict from FastqReader.next_batch (or the same keys) -> (ReadBatch, keep-alive list)"""
    keep = [_u8(batch["bases"]), np.ascontiguousarray(batch["offsets"], "<u8"),
            None if batch.get("quals") is None else _u8(batch["quals"]), _u8(batch["names"]),
            np.ascontiguousarray(batch["name_off"], "<u8")]
    rb = ReadBatch(len(keep[1]) - 1, len(keep[0]), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4]))
    return rb, keep


class Writer:
    """thm_writer: SAM / PAF rendering (src/aln_writer.rs)."""

    def __init__(self, index, fmt=FMT_SAM, n_threads=1):
        h = C.c_void_p()
        rc = lib().thm_writer_create(index.h, fmt, n_threads, C.byref(h))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        self.h = h
        self.index = index

    def header(self):
        t = Text()
        rc = lib().thm_writer_header(self.h, C.byref(t))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        return bytes(_copy(t.data, t.len, np.uint8))

    def header_sorted(self):
        """thm_writer_header_sorted: the header with the @HD line of a coordinate-sorted file"""
        t = Text()
        rc = lib().thm_writer_header_sorted(self.h, C.byref(t))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        return bytes(_copy(t.data, t.len, np.uint8))

    def trailer(self):
        t = Text()
        rc = lib().thm_writer_trailer(self.h, C.byref(t))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        return bytes(_copy(t.data, t.len, np.uint8))

    def format_batch(self, batch, result):
        """batch: dict as from FastqReader.next_batch; result: BatchResult -> bytes"""
        rb, keep = read_batch_struct(batch)
        offs = np.ascontiguousarray(result.offsets, "<u8")
        v = BatchView(len(offs) - 1, len(result.alns), len(result.ops), _ptr(offs), _ptr(result.alns),
                      _ptr(result.ops), 0, None)
        t = Text()
        rc = lib().thm_writer_format_batch(self.h, C.byref(rb), C.byref(v), C.byref(t))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        return bytes(_copy(t.data, t.len, np.uint8))

    def format_batch_cigars(self, batch, result):
        """batch: dict as from FastqReader.next_batch; result: CigarResult -> bytes (what format_batch gives for the
        full result of the same batch)"""
        rb, keep = read_batch_struct(batch)
        offs = np.ascontiguousarray(result.offsets, "<u8")
        v = CigarView(len(offs) - 1, len(result.alns), len(result.cigar), _ptr(offs), _ptr(result.alns),
                      _ptr(result.digests), _ptr(result.cigar), 0, None)
        t = Text()
        rc = lib().thm_writer_format_batch_cigars(self.h, C.byref(rb), C.byref(v), C.byref(t))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        return bytes(_copy(t.data, t.len, np.uint8))

    def wrap_bam(self, result):
        """thm_writer_wrap_bam: a BamResult (or anything with data / read_rec_off) -> complete BGZF blocks"""
        data = _u8(result.data)
        offs = np.ascontiguousarray(result.read_rec_off, "<u8")
        v = BamView(len(offs) - 1, getattr(result, "n_records", 0), len(data), _ptr(data), _ptr(offs), 0, None)
        t = Text()
        rc = lib().thm_writer_wrap_bam(self.h, C.byref(v), C.byref(t))
        if rc != 0:
            raise ThermiteError(rc, _last_error())
        return bytes(_copy(t.data, t.len, np.uint8))

    def close(self):
        if getattr(self, "h", None):
            lib().thm_writer_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


def align_files(aligner, fastq_paths, output_path, fmt=FMT_SAM, batch_reads=0, n_threads=0):
    """align_reads_from_file (src/aligner.rs:22-120): FASTQ files -> one SAM / PAF / BAM file; returns the run stats.
    `aligner`: one Aligner, or a list of them (one per GPU, all over the same Index)."""
    paths = _cstr_array([str(p) for p in fastq_paths])
    st = RunStats()
    als = list(aligner) if isinstance(aligner, (list, tuple)) else [aligner]
    arr = (C.c_void_p * len(als))(*[a.h for a in als])
    rc = lib().thm_align_files_multi(arr, len(als), paths, len(fastq_paths), str(output_path).encode(), fmt, batch_reads, n_threads,
                                     C.byref(st))
    if rc != 0:
        raise ThermiteError(rc, _last_error())
    return {k: getattr(st, k) for k, _ in RunStats._fields_}


def debug_gzip_host_slice(state, data, last_block=True, cap=None):
    """test hook: the host side of upload_fastq_gzip's inflate (GzInflater's resume entry), no aligner needed -> (the
    inflated bytes of the blocks that end inside `data`, n_consumed); `state` moves on in place"""
    src = np.frombuffer(bytes(data), np.uint8) if len(data) else np.zeros(1, np.uint8)
    out = np.empty((1100 * len(data) + 65536 if cap is None else cap) + 64, np.uint8)
    n, used = C.c_uint64(0), C.c_uint64(0)
    rc = lib().thm_debug_gzip_host_slice(C.byref(state), src.ctypes.data, len(data), int(bool(last_block)), out.ctypes.data, len(out),
                                         C.byref(n), C.byref(used))
    if rc != 0:
        raise ThermiteError(rc, (lib().thm_last_error(None) or b"").decode(errors="replace"))
    return out[: n.value].tobytes(), used.value
