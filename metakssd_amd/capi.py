"""ctypes binding of libmetakssd_hip.so (include/metakssd_hip.h) -- the binding a Python caller of the
reference's sketching path would use.  No compute happens here and there is no fallback: if the
shared library is missing, import fails; if no HIP device is usable, Engine() raises.

Names follow the reference's domain: shuf, params, sketch, reads/rows, components.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MK_LIBRARY") or os.path.join(_HERE, "lib", "libmetakssd_hip.so")  # MK_LIBRARY: an experiment build (make tuning)

MK_OK = 0
MK_ERR_ARG, MK_ERR_NO_DEVICE, MK_ERR_HIP, MK_ERR_CROWDED = -1, -2, -3, -4
MK_ERR_STATE, MK_ERR_IO, MK_ERR_FORMAT, MK_ERR_NOMEM = -5, -6, -7, -8
MK_MODE_KOC, MK_MODE_SET, MK_MODE_UNIQ_SET, MK_MODE_OCC_SET = 0, 1, 2, 3
MK_ROWS_PACKED, MK_PACKED_PITCH, MK_PACKED_MAX_BASES = 0x80000000, 64, 152
MK_ROWS_WIDE, MK_WIDE_MAX_BASES = 0x40000000, 240
MK_OPT_SPARSE, MK_OPT_CAND_CAP, MK_OPT_RESULT_CAP, MK_OPT_DIRECT_HOST, MK_OPT_FRONT_BITS, MK_OPT_KEYLIST_CAP, MK_OPT_BATCH_TAB_BITS = 1, 2, 3, 4, 5, 6, 7
MK_BEGIN_NOTHING_FOLLOWS = 0x100  # mk_sketch_begin(mode | this): the last sketch of a run on split queues -- its tail on the whole device
MK_OPT_SPLIT_CUS = 10  # scan kernel on a queue of its own, the rest on this many compute units (two engines in turn: bench.py)
MK_OPT_BATCH_HOME_IDS = 11  # test hook: a cap on the ids that come home with a batch; mk_sketch_batch_end fetches the rest late


class MkError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("metakssd_hip error %d: %s" % (code, msg))
        self.code = code


class CrowdedError(MkError):
    """more than hashlimit distinct keys: the reference aborts with 'the context space is too crowd' (iseq2comem.c:708-709)"""


class ShufC(C.Structure):
    _fields_ = [("id", C.c_int32), ("k", C.c_int32), ("subk", C.c_int32), ("drlevel", C.c_int32),
                ("table", C.POINTER(C.c_int32)), ("len", C.c_uint64)]


class ParamsC(C.Structure):
    _fields_ = [("shuf_id", C.c_int32), ("k", C.c_int32), ("subk", C.c_int32), ("drlevel", C.c_int32),
                ("half_outctx_len", C.c_int32), ("TL", C.c_int32), ("crvsaddmove", C.c_int32),
                ("component_num", C.c_int32), ("comp_code_bits", C.c_int32),
                ("dim_start", C.c_int32), ("dim_end", C.c_int32),
                ("hashsize", C.c_uint32), ("hashlimit", C.c_uint32),
                ("tupmask", C.c_uint64), ("domask", C.c_uint64), ("undomask", C.c_uint64),
                ("shuf_table", C.POINTER(C.c_int32)), ("shuf_len", C.c_uint64), ("component_sz", C.c_int32), ("reserved", C.c_int32)]


class ComponentC(C.Structure):
    _fields_ = [("ids", C.POINTER(C.c_uint32)), ("counts", C.POINTER(C.c_uint16)), ("n", C.c_uint64)]


class ResultC(C.Structure):
    _fields_ = [("component_num", C.c_int32), ("total", C.c_uint64), ("components", C.POINTER(ComponentC))]


class ProfileC(C.Structure):
    _fields_ = [("scan_ms", C.c_double), ("scan_launches", C.c_uint64), ("resolve_ms", C.c_double), ("clear_ms", C.c_double),
                ("finish_ms", C.c_double), ("bases_scanned", C.c_uint64), ("rows_scanned", C.c_uint64), ("finish_side_ms", C.c_double)]


class FastaStateC(C.Structure):
    _fields_ = [("TL", C.c_uint32), ("in_header", C.c_uint32), ("fill", C.c_uint32), ("fresh", C.c_uint32),
                ("pending", C.c_uint8 * 4096)]


class FastqOptsC(C.Structure):
    _fields_ = [("occ", C.c_int32), ("qmin", C.c_int32), ("TL", C.c_int32), ("nthreads", C.c_int32), ("inflight", C.c_int32),
                ("chunk_bytes", C.c_uint64), ("drop_pages", C.c_int32), ("ahead", C.c_int32), ("packed", C.c_int32), ("fd", C.c_int32),
                ("early_chunks", C.c_int32), ("reserved2", C.c_int32), ("pool_bytes", C.c_uint64)]


class FastqStatsC(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("records", C.c_uint64), ("chunks", C.c_uint64), ("chunks_discarded", C.c_uint64),
                ("serial_rows", C.c_uint64), ("threads", C.c_uint32), ("t_setup_s", C.c_double), ("t_wait_frame_s", C.c_double),
                ("t_push_s", C.c_double), ("t_total_s", C.c_double), ("t_push_call_s", C.c_double), ("t_wait_call_s", C.c_double),
                ("t_push_call_max_s", C.c_double), ("t_first_push_call_s", C.c_double)]


_PUSH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64))
_WAIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64)
_ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
_RELEASE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t)
_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t)


class RowsSinkC(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("push", _PUSH_FN), ("wait", _WAIT_FN), ("alloc", _ALLOC_FN), ("release", _RELEASE_FN),
                ("ready", C.c_void_p)]


class BatchFileC(C.Structure):
    _fields_ = [("text", C.c_void_p), ("n", C.c_uint64)]


class DistOptsC(C.Structure):
    _fields_ = [("metric", C.c_int32), ("outfields", C.c_int32), ("correction", C.c_int32), ("num_neigb", C.c_int32),
                ("dthreshold", C.c_double)]


class BgzfBlockC(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("in_len", C.c_uint32), ("pay_off", C.c_uint32), ("pay_len", C.c_uint32),
                ("crc32", C.c_uint32), ("isize", C.c_uint32), ("reserved", C.c_uint32)]


class GzipInfoC(C.Structure):
    _fields_ = [("pay_off", C.c_uint64), ("pay_len", C.c_uint64), ("crc32", C.c_uint32), ("isize", C.c_uint32), ("is_single", C.c_int32),
                ("reserved", C.c_int32)]


class GzMemberC(C.Structure):
    _fields_ = [("pay_off", C.c_uint64), ("out_off", C.c_uint64), ("pay_len", C.c_uint32), ("isize", C.c_uint32), ("crc32", C.c_uint32),
                ("reserved", C.c_uint32)]


class GzMemberResultC(C.Structure):
    _fields_ = [("status", C.c_uint32), ("consumed", C.c_uint32), ("pos", C.c_uint32), ("crc32", C.c_uint32)]


class GzFileC(C.Structure):
    _fields_ = [("comp", C.c_void_p), ("n", C.c_uint64), ("info", GzipInfoC)]


class BgzfOptsC(C.Structure):
    _fields_ = [("chunk_bytes", C.c_uint64), ("reserved", C.c_uint64)]


class BgzfStatsC(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("chunks", C.c_uint64), ("comp_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("rows", C.c_uint64),
                ("inflate_ms", C.c_double), ("frame_ms", C.c_double), ("t_scan_s", C.c_double), ("t_read_s", C.c_double), ("t_total_s", C.c_double),
                ("bad_block", C.c_int64), ("bad_status", C.c_int32), ("reserved", C.c_int32)]


class GunzipOptsC(C.Structure):
    _fields_ = [("span_bytes", C.c_uint32), ("ratio", C.c_uint32), ("batch_spans", C.c_uint32), ("flags", C.c_uint32)]


class GunzipPieceC(C.Structure):
    _fields_ = [("start_bit", C.c_uint64), ("text_len", C.c_uint64)]


class GunzipPiecesC(C.Structure):
    _fields_ = [("v", C.POINTER(GunzipPieceC)), ("n", C.c_uint64)]


class GunzipStatsC(C.Structure):
    _fields_ = [("pieces", C.c_uint64), ("batches", C.c_uint64), ("comp_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("rows", C.c_uint64),
                ("find_ms", C.c_double), ("decode_ms", C.c_double), ("resolve_ms", C.c_double), ("frame_ms", C.c_double),
                ("t_read_s", C.c_double), ("t_total_s", C.c_double), ("bad_piece", C.c_int64), ("bad_status", C.c_int32), ("members", C.c_uint32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(make -C metakssd_amd/csrc)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, u8p, u64, u32, i32 = C.c_void_p, C.POINTER(C.c_uint8), C.c_uint64, C.c_uint32, C.c_int32
    sig = {
        "mk_shuf_read": [C.c_char_p, C.POINTER(ShufC)],
        "mk_shuf_generate": [i32, i32, i32, u64, C.POINTER(ShufC)],
        "mk_shuf_write": [C.POINTER(ShufC), C.c_char_p],
        "mk_params_init": [C.POINTER(ShufC), C.POINTER(ParamsC)],
        "mk_params_init_csz": [C.POINTER(ShufC), i32, C.POINTER(ParamsC)],
        "mk_device_count": [C.POINTER(C.c_int)],
        "mk_engine_create": [C.POINTER(ParamsC), C.c_int, C.POINTER(vp)],
        "mk_engine_destroy": [vp],
        "mk_engine_set_option": [vp, C.c_int, C.c_int64],
        "mk_engine_set_stream": [vp, vp],
        "mk_engine_use_own_stream": [vp],
        "mk_engine_share_scan_queue": [vp, vp],
        "mk_sketch_begin": [vp, C.c_int],
        "mk_sketch_begin_occ": [vp, C.c_int],
        "mk_sketch_push_reads": [vp, vp, u32, u64, u64],
        "mk_sketch_push_reads_device": [vp, vp, u32, u64, u64],
        "mk_sketch_push_reads_async": [vp, vp, u32, u64, u64, C.POINTER(u64)],
        "mk_sketch_push_wait": [vp, u64],
        "mk_sketch_push_stream": [vp, vp, u64, C.c_int],
        "mk_sketch_push_fastq_long": [vp, vp, u64, C.c_int],
        "mk_sketch_push_fastq_long_device": [vp, vp, u64, C.c_int],
        "mk_sketch_push_fastq_long_q": [vp, vp, u64, C.c_int, C.c_int32],
        "mk_sketch_push_fastq_long_q_device": [vp, vp, u64, C.c_int, C.c_int32],
        "mk_sketch_fastq_long_frame_ms": [vp, C.POINTER(C.c_double)],
        "mk_partial_count_begin": [vp],
        "mk_partial_export_async": [vp, vp, vp, vp, u64, C.POINTER(u64)],
        "mk_pack_rows_host": [vp, u32, u64, vp],
        "mk_params_packed_ok": [C.POINTER(ParamsC)],
        "mk_sketch_batch_begin": [vp, C.c_int, vp, u32],
        "mk_sketch_batch_begin_rows": [vp, C.c_int, u32, vp, u32],
        "mk_fasta_pack_rows": [vp, C.c_size_t, C.c_int32, u32, vp, u64, C.POINTER(u64)],
        "mk_sketch_batch_end": [vp, vp],
        "mk_sketch_batch_home_ids": [vp, C.POINTER(u64), C.POINTER(u64)],
        "mk_sketch_batch_begin_gz": [vp, C.c_int, C.POINTER(GzFileC), u32],
        "mk_sketch_batch_gz_status": [vp, vp, u32],
        "mk_sketch_batch_begin_gunzip": [vp, C.c_int, C.POINTER(GzFileC), u32, C.POINTER(GunzipOptsC)],
        "mk_sketch_batch_gz_pieces": [vp, vp, u32],
        "mk_inflate_members_split": [vp, vp, C.c_size_t, C.POINTER(GzMemberC), u32, C.POINTER(GunzipOptsC), vp, C.c_size_t,
                                     C.POINTER(GzMemberResultC), C.POINTER(GunzipPiecesC)],
        "mk_gzip_scan": [C.c_int, vp, C.c_size_t, C.POINTER(GzipInfoC)],
        "mk_gzip_scan_stream": [C.c_int, vp, C.c_size_t, C.POINTER(GzipInfoC)],
        "mk_inflate_stream": [vp, vp, C.c_size_t, C.POINTER(GzipInfoC), C.POINTER(GunzipOptsC), vp, C.c_size_t, C.POINTER(u64), C.POINTER(i32),
                              C.POINTER(GunzipPiecesC)],
        "mk_inflate_stream_members": [vp, C.POINTER(u64)],
        "mk_inflate_stream_repairs": [vp, C.POINTER(u64)],
        "mk_sketch_gunzip_repairs": [vp, C.POINTER(u64)],
        "mk_sketch_push_gzip": [vp, C.c_int, C.c_size_t, C.POINTER(GunzipOptsC), u64, C.POINTER(GunzipStatsC)],
        "mk_sketch_push_gzip_long": [vp, C.c_int, C.c_size_t, C.POINTER(GunzipOptsC), C.c_int, C.POINTER(GunzipStatsC)],
        "mk_sketch_push_gzip_long_q": [vp, C.c_int, C.c_size_t, C.POINTER(GunzipOptsC), C.c_int32, C.c_int, C.POINTER(GunzipStatsC)],
        "mk_sketch_push_gzip_q": [vp, C.c_int, C.c_size_t, C.POINTER(GunzipOptsC), i32, u64, C.POINTER(GunzipStatsC)],
        "mk_inflate_members": [vp, vp, C.c_size_t, C.POINTER(GzMemberC), u32, vp, C.c_size_t, C.POINTER(GzMemberResultC)],
        "mk_sketch_finish": [vp, C.POINTER(ResultC)],
        "mk_sketch_finish_keys": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)],
        "mk_sketch_finish_begin": [vp],
        "mk_sketch_finish_end": [vp, C.POINTER(ResultC)],
        "mk_result_release": [vp, C.POINTER(ResultC)],
        "mk_engine_sync": [vp],
        "mk_host_alloc": [C.POINTER(vp), C.c_size_t],
        "mk_host_free": [vp],
        "mk_host_arena_alloc": [C.POINTER(vp), C.c_size_t],
        "mk_host_arena_free": [vp, C.c_size_t],
        "mk_host_register": [vp, C.c_size_t],
        "mk_host_unregister": [vp],
        "mk_partial_count": [vp, C.POINTER(u64)],
        "mk_partial_export": [vp, vp, vp, vp, u64, C.POINTER(u64)],
        "mk_partial_import": [vp, vp, vp, vp, u64],
        "mk_partial_export_split": [vp, u32, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)],
        "mk_partial_export_split_async": [vp, u32, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)],
        "mk_partial_restart": [vp],
        "mk_partial_list_reserve": [vp, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)],
        "mk_partial_list_commit": [vp, u64],
        "mk_partial_list_adopt": [vp, vp, vp, vp, u64, u64],
        "mk_profile_enable": [vp, C.c_int],
        "mk_profile_reset": [vp],
        "mk_profile_get": [vp, C.POINTER(ProfileC)],
        "mk_synth_rows_host": [u64, u64, u64, u32, u32, vp],
        "mk_synth_rows_device": [C.c_int, vp, u64, u64, u64, u32, u32, vp],
        "mk_synth_fastq_write": [C.c_char_p, u64, u64, u64, u32],
        "mk_synth_fastq_write_mt": [C.c_char_p, u64, u64, u64, u32, C.c_int],
        "mk_fastq_stream": [vp, C.c_size_t, C.POINTER(FastqOptsC), C.POINTER(RowsSinkC), u64, C.POINTER(FastqStatsC)],
        "mk_sketch_push_fastq": [vp, vp, C.c_size_t, C.POINTER(FastqOptsC), u64, C.POINTER(FastqStatsC)],
        "mk_fastq_frame": [vp, C.c_size_t, C.c_int, vp, u32, u64, C.POINTER(u64), C.POINTER(C.c_size_t)],
        "mk_fastq_frame_q": [vp, C.c_size_t, C.c_int, i32, i32, u64, vp, u32, u64, C.POINTER(u64), C.POINTER(u64),
                             C.POINTER(C.c_size_t)],
        "mk_fastq_frame_mt": [vp, C.c_size_t, C.c_int, C.c_int, i32, i32, u64, vp, u32, u64, C.c_int, C.POINTER(u64), C.POINTER(u64),
                              C.POINTER(C.c_size_t)],
        "mk_fasta_window_init": [C.POINTER(FastaStateC), i32],
        "mk_fasta_window": [C.POINTER(FastaStateC), vp, C.c_size_t, C.c_int, vp, u32, u64, C.POINTER(u64),
                            C.POINTER(C.c_size_t)],
        "mk_setop_create": [C.c_int, C.POINTER(vp)],
        "mk_setop_destroy": [vp],
        "mk_setop_begin": [vp, C.c_int],
        "mk_setop_add": [vp, vp, u64],
        "mk_setop_add_device": [vp, vp, u64],
        "mk_setop_finish": [vp, C.POINTER(vp), C.POINTER(u64)],
        "mk_setop_result_device": [vp, C.POINTER(vp), C.POINTER(u64)],
        "mk_setop_join": [vp, vp, vp, u64, vp, u64, vp, u32, C.POINTER(vp), C.POINTER(u64), vp],
        "mk_setop_last_join_ms": [vp, C.POINTER(C.c_double)],
        "mk_mco_create": [C.c_int, C.POINTER(vp)],
        "mk_mco_destroy": [vp],
        "mk_mco_build": [vp, vp, vp, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)],
        "mk_mco_index_rows": [vp, u64, u64, vp],
        "mk_mco_sort_pairs": [vp, vp, vp, u64],
        "mk_mco_set_option": [vp, C.c_int, C.c_int64],
        "mk_mco_count_begin": [vp, u32, u32],
        "mk_mco_count_add": [vp, vp, u64, vp, vp, vp, vp, vp],
        "mk_mco_count_finish": [vp, vp],
        "mk_mco_last_kernel_ms": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "mk_abv_create": [C.c_int, C.POINTER(vp)],
        "mk_abv_destroy": [vp],
        "mk_abv_index": [vp, vp, u64, vp, u32, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)],
        "mk_abv_load": [vp, vp, u64, vp, u32, vp, u32],
        "mk_abv_search": [vp, C.c_int, u32, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)],
        "mk_abv_last_kernel_ms": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "mk_composite_create": [C.c_int, C.POINTER(vp)],
        "mk_composite_destroy": [vp],
        "mk_composite_load_begin": [vp, u32, u32],
        "mk_composite_load_component": [vp, u32, vp, vp],
        "mk_composite_query_begin": [vp, u32],
        "mk_composite_query_component": [vp, u32, vp, vp, vp],
        "mk_composite_query_sample_keys": [vp, u32, vp, vp, u64, u32],
        "mk_composite_query_finish": [vp, C.POINTER(vp), vp],
        "mk_composite_set_option": [vp, C.c_int, C.c_int64],
        "mk_composite_last_kernel_ms": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "mk_composite_last_counts": [vp, C.POINTER(u64), C.POINTER(u64)],
        "mk_byread_create": [C.c_int, C.POINTER(vp)],
        "mk_byread_destroy": [vp],
        "mk_byread_begin": [vp, C.POINTER(ParamsC)],
        "mk_byread_push_text": [vp, vp, u64, C.c_int],
        "mk_byread_take": [vp, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64)],
        "mk_byread_finish": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_double)],
        "mk_reverse_ids": [vp, vp, u64, u32, vp],
        "mk_byread_last_kernel_ms": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "mk_byread_write_stat": [C.c_char_p, C.POINTER(ParamsC), C.c_char_p],
        "mk_reverse_outname": [C.c_char_p, C.c_char_p, C.c_size_t],
        "mk_dist_print": [vp, C.POINTER(DistOptsC), i32, i32, u32, u32, vp, vp, vp, vp, vp],
        "mk_sketchdir_open": [C.c_char_p, C.POINTER(ParamsC), C.c_int, C.c_int, C.POINTER(vp)],
        "mk_sketchdir_add": [vp, C.c_char_p, C.POINTER(ResultC)],
        "mk_sketchdir_close": [vp],
        "mk_bgzf_scan": [C.c_int, vp, C.c_size_t, C.POINTER(C.POINTER(BgzfBlockC)), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int)],
        "mk_inflate_create": [C.c_int, C.POINTER(vp)],
        "mk_inflate_destroy": [vp],
        "mk_inflate_blocks": [vp, vp, C.c_size_t, C.POINTER(BgzfBlockC), u64, vp, C.c_size_t, vp],
        "mk_fastq_frame_device": [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.POINTER(u32), C.POINTER(u64), C.POINTER(C.c_size_t), C.POINTER(u32)],
        "mk_fastq_frame_q_device": [vp, vp, C.c_size_t, C.c_int, i32, u64, vp, C.c_size_t, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64),
                                    C.POINTER(C.c_size_t), C.POINTER(u32)],
        "mk_inflate_last_kernel_ms": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "mk_sketch_push_bgzf": [vp, C.c_int, C.c_size_t, C.POINTER(BgzfOptsC), u64, C.POINTER(BgzfStatsC)],
        "mk_sketch_push_bgzf_long": [vp, C.c_int, C.c_size_t, C.POINTER(BgzfOptsC), C.c_int, C.POINTER(BgzfStatsC)],
        "mk_sketch_push_bgzf_long_q": [vp, C.c_int, C.c_size_t, C.POINTER(BgzfOptsC), C.c_int32, C.c_int, C.POINTER(BgzfStatsC)],
        "mk_sketch_push_bgzf_q": [vp, C.c_int, C.c_size_t, C.POINTER(BgzfOptsC), i32, u64, C.POINTER(BgzfStatsC)],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.mk_shuf_free.argtypes = [C.POINTER(ShufC)]
    lib.mk_shuf_free.restype = None
    lib.mk_setop_last_error.argtypes = [vp]
    lib.mk_setop_last_error.restype = C.c_char_p
    lib.mk_mco_last_error.argtypes = [vp]
    lib.mk_mco_last_error.restype = C.c_char_p
    lib.mk_abv_last_error.argtypes = [vp]
    lib.mk_abv_last_error.restype = C.c_char_p
    lib.mk_composite_last_error.argtypes = [vp]
    lib.mk_composite_last_error.restype = C.c_char_p
    lib.mk_byread_last_error.argtypes = [vp]
    lib.mk_byread_last_error.restype = C.c_char_p
    lib.mk_inflate_last_error.argtypes = [vp]
    lib.mk_inflate_last_error.restype = C.c_char_p
    lib.mk_inflate_status_text.argtypes = [C.c_int]
    lib.mk_inflate_status_text.restype = C.c_char_p
    lib.mk_gunzip_status_text.argtypes = [C.c_int]
    lib.mk_gunzip_status_text.restype = C.c_char_p
    lib.mk_bgzf_last_error.argtypes = []
    lib.mk_bgzf_last_error.restype = C.c_char_p
    lib.mk_bgzf_free.argtypes = [C.POINTER(BgzfBlockC)]
    lib.mk_bgzf_free.restype = None
    lib.mk_gunzip_pieces_free.argtypes = [C.POINTER(GunzipPiecesC)]
    lib.mk_gunzip_pieces_free.restype = None
    lib.mk_setop_stream.argtypes = [vp]
    lib.mk_setop_stream.restype = vp
    lib.mk_last_error.argtypes = [vp]
    lib.mk_last_error.restype = C.c_char_p
    lib.mk_fasta_pack_bound.argtypes = [C.c_size_t, C.c_int32, u32]
    lib.mk_fasta_pack_bound.restype = u64
    return lib


lib = _load()


def _check(rc, eng=None):
    if rc == MK_OK:
        return
    msg = lib.mk_last_error(eng).decode(errors="replace") if (eng or rc in (MK_ERR_NO_DEVICE, MK_ERR_HIP, MK_ERR_NOMEM)) else ""
    raise (CrowdedError if rc == MK_ERR_CROWDED else MkError)(rc, msg)


class Shuf:
    """a .shuf dimension-shuffle table (command_shuffle.h:4-16)"""

    def __init__(self, c):
        self.c = c

    @classmethod
    def read(cls, path):
        c = ShufC()
        _check(lib.mk_shuf_read(os.fsencode(path), C.byref(c)))
        return cls(c)

    @classmethod
    def generate(cls, k, subk, drlevel, seed):
        c = ShufC()
        _check(lib.mk_shuf_generate(k, subk, drlevel, seed, C.byref(c)))
        return cls(c)

    def write(self, path):
        _check(lib.mk_shuf_write(C.byref(self.c), os.fsencode(path)))

    @property
    def table(self):
        return np.ctypeslib.as_array(self.c.table, shape=(self.c.len,))

    def params(self, component_sz=8):
        p = ParamsC()
        _check(lib.mk_params_init_csz(C.byref(self.c), component_sz, C.byref(p)))
        return p

    def __del__(self):
        try:
            lib.mk_shuf_free(C.byref(self.c))
        except Exception:
            pass


def device_count():
    n = C.c_int(0)
    rc = lib.mk_device_count(C.byref(n))
    return n.value if rc == MK_OK else 0


def synth_rows_host(seed, first_read, nreads, length, stride):
    rows = np.empty(nreads * stride, dtype=np.uint8)
    _check(lib.mk_synth_rows_host(seed, first_read, nreads, length, stride, rows.ctypes.data))
    return rows


def pack_rows_host(rows, stride):
    """ASCII rows -> 64-byte packed rows (mk_pack_rows_host); 16-byte aligned result"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n = rows.size // stride
    raw = np.zeros(n * MK_PACKED_PITCH + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    out = raw[off:off + n * MK_PACKED_PITCH]
    _check(lib.mk_pack_rows_host(rows.ctypes.data if n else None, stride, n, out.ctypes.data if n else None))
    return out


def fasta_pack_rows(text, TL, fmt=None):
    """a whole FASTA text -> its packed rows (mk_fasta_pack_rows; fmt MK_ROWS_PACKED or MK_ROWS_WIDE); -> (rows u8 [nrows * 64], 16-byte aligned, rc)"""
    fmt = MK_ROWS_PACKED if fmt is None else fmt
    b = np.frombuffer(bytes(text), dtype=np.uint8)
    bound = int(lib.mk_fasta_pack_bound(len(b), TL, fmt))
    raw = np.zeros(bound * MK_PACKED_PITCH + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    n = C.c_uint64(0)
    rc = lib.mk_fasta_pack_rows(b.ctypes.data if len(b) else None, len(b), TL, fmt, raw.ctypes.data + off, bound, C.byref(n))
    return raw[off:off + n.value * MK_PACKED_PITCH], rc


def fastq_frame(buf, stride, final=True, max_rows=None):
    """FASTQ bytes -> fixed-stride rows (numpy u8 [nrows*stride]); returns (rows, nrows, consumed, rc)"""
    b = np.frombuffer(buf, dtype=np.uint8)
    max_rows = max_rows if max_rows is not None else len(b) // 4 + 1
    rows = np.zeros(max(1, max_rows) * stride, dtype=np.uint8)
    n, used = C.c_uint64(0), C.c_size_t(0)
    rc = lib.mk_fastq_frame(b.ctypes.data if len(b) else None, len(b), 1 if final else 0, rows.ctypes.data, stride,
                            max_rows, C.byref(n), C.byref(used))
    return rows[: n.value * stride], n.value, used.value, rc


def fastq_frame_q(buf, stride, TL, qmin=0, final=True, records_before=0, max_rows=None):
    """FASTQ bytes -> rows the way fastq2co() reads them (quality mask, record rule, long-read windows);
    returns (rows, nrows, nrecords, consumed, rc)"""
    b = np.frombuffer(buf, dtype=np.uint8)
    max_rows = max_rows if max_rows is not None else len(b) // 4 + len(b) // max(1, stride - TL) + 2
    rows = np.zeros(max(1, max_rows) * stride, dtype=np.uint8)
    n, nrec, used = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
    rc = lib.mk_fastq_frame_q(b.ctypes.data if len(b) else None, len(b), 1 if final else 0, qmin, TL, records_before,
                              rows.ctypes.data, stride, max_rows, C.byref(n), C.byref(nrec), C.byref(used))
    return rows[: n.value * stride], n.value, nrec.value, used.value, rc


def fastq_frame_mt(buf, stride, nthreads, occ=False, TL=22, qmin=0, final=True, records_before=0, max_rows=None):
    """the threaded framer; returns (rows, nrows, nrecords, consumed, rc)"""
    b = np.frombuffer(buf, dtype=np.uint8)
    max_rows = max_rows if max_rows is not None else len(b) // 4 + len(b) // max(1, stride - TL) + 2
    rows = np.zeros(max(1, max_rows) * stride, dtype=np.uint8)
    n, nrec, used = C.c_uint64(0), C.c_uint64(0), C.c_size_t(0)
    rc = lib.mk_fastq_frame_mt(b.ctypes.data if len(b) else None, len(b), 1 if final else 0, 1 if occ else 0, qmin, TL, records_before,
                               rows.ctypes.data, stride, max_rows, nthreads, C.byref(n), C.byref(nrec), C.byref(used))
    return rows[: n.value * stride], n.value, nrec.value, used.value, rc


def fastq_stream(buf, nthreads=4, chunk_bytes=0, occ=False, TL=22, qmin=0, first_ordinal=0, inflight=2, drop_pages=False, packed=False, pool_bytes=0,
                 ready_log=None, via_fd=False, early_chunks=0):
    """the whole-file FASTQ stream (mk_fastq_stream) into host memory: returns (list of (rows u8 array, stride, nrows,
    first ordinal) in push order, stats, rc).  Buffers come from malloc here; the engine-bound form is Engine.push_fastq."""
    b = np.frombuffer(buf, dtype=np.uint8)
    pushes, keep = [], {}
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]

    def push(ctx, rows, stride, nrows, ord0, token):
        a = np.ctypeslib.as_array(C.cast(rows, C.POINTER(C.c_uint8)), shape=(nrows * (stride & ~MK_ROWS_PACKED),)).copy()
        pushes.append((a, stride, nrows, ord0))  # (stride & MK_ROWS_PACKED: 64-byte packed rows)
        token[0] = len(pushes)
        return 0

    def wait(ctx, token):
        return 0

    blocks = []

    def alloc(ctx, n):
        p = libc.malloc(n)
        blocks.append((p, n))
        return p

    def ready(ctx, rows, n):  # called on the framers' threads: a buffer has been written and waits for its push
        if ready_log is not None:
            ready_log.append((rows - blocks[-1][0], n))
    ready_fn = _READY_FN(ready)
    sink = RowsSinkC(None, _PUSH_FN(push), _WAIT_FN(wait), _ALLOC_FN(alloc), _RELEASE_FN(lambda ctx, p, n: libc.free(p)),
                     C.cast(ready_fn, C.c_void_p) if ready_log is not None else None)
    keep["sink"] = (sink, ready_fn)
    fd = -1
    if via_fd:  # the same bytes through a file descriptor: the framers pread pieces instead of reading a mapping (mk_fastq_opts.fd)
        import tempfile
        tf = tempfile.TemporaryFile()
        tf.write(bytes(buf))
        tf.flush()
        fd = tf.fileno()
        keep["file"] = tf
    o = FastqOptsC(1 if occ else 0, qmin, TL, nthreads, inflight, chunk_bytes, 1 if drop_pages else 0, 0, 1 if packed else 0, fd if via_fd else 0, early_chunks, 0, pool_bytes)
    if ready_log is not None:
        ready_log.append(blocks)
    st = FastqStatsC()
    rc = lib.mk_fastq_stream(None if via_fd or not len(b) else b.ctypes.data, len(b), C.byref(o), C.byref(sink), first_ordinal, C.byref(st))
    return pushes, st, rc


def fasta_windows(buf, TL, stride, chunk=None):
    """FASTA bytes -> overlapped fixed-stride rows; `chunk` feeds the input in pieces of that many bytes"""
    b = np.frombuffer(buf, dtype=np.uint8)
    st = FastaStateC()
    _check(lib.mk_fasta_window_init(C.byref(st), TL))
    out = []
    max_rows = 4096
    rows = np.zeros(max_rows * stride, dtype=np.uint8)
    pos, step = 0, (chunk or max(1, len(b)))
    while True:
        end = min(len(b), pos + step)
        final = end >= len(b)
        off = pos
        while True:
            n, used = C.c_uint64(0), C.c_size_t(0)
            ptr = b[off:end].ctypes.data if end > off else None
            _check(lib.mk_fasta_window(C.byref(st), ptr, end - off, 1 if final else 0, rows.ctypes.data, stride, max_rows,
                                       C.byref(n), C.byref(used)))
            if n.value:
                out.append(rows[: n.value * stride].copy())
            off += used.value
            if off >= end and n.value < max_rows:
                break
        pos = end
        if final:
            break
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)


class Engine:
    """one GPU's sketch engine (mk_engine): begin -> push_reads* -> finish"""

    def __init__(self, shuf, device=0, sparse=None, cand_cap=None, component_sz=8, front_bits=None):
        self.shuf = shuf  # keeps the host table alive
        self.params = shuf.params(component_sz)
        self.h = C.c_void_p()
        rc = lib.mk_engine_create(C.byref(self.params), device, C.byref(self.h))
        if rc != MK_OK:
            raise MkError(rc, lib.mk_last_error(None).decode(errors="replace"))
        self.device = device
        if sparse is not None:
            self.set_option(MK_OPT_SPARSE, int(sparse))
        if cand_cap is not None:
            self.set_option(MK_OPT_CAND_CAP, int(cand_cap))
        if front_bits is not None:
            self.set_option(MK_OPT_FRONT_BITS, int(front_bits))

    def set_option(self, option, value):
        """mk_engine_set_option: MK_OPT_SPARSE (-1/0/1), MK_OPT_CAND_CAP (records per scan wave); between sketches only"""
        _check(lib.mk_engine_set_option(self.h, option, value), self.h)

    def close(self):
        if self.h:
            lib.mk_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        """run the engine's work on this hipStream_t handle (0/None = HIP's default stream, e.g. torch's current stream)"""
        _check(lib.mk_engine_set_stream(self.h, C.c_void_p(stream_handle or None)), self.h)

    def use_own_stream(self):
        _check(lib.mk_engine_use_own_stream(self.h), self.h)

    def share_scan_queue(self, owner):
        """mk_engine_share_scan_queue: this engine's scans go to OWNER's scan queue (both with the same MK_OPT_SPLIT_CUS setting)"""
        _check(lib.mk_engine_share_scan_queue(self.h, owner.h), self.h)

    def begin(self, mode=MK_MODE_KOC):
        _check(lib.mk_sketch_begin(self.h, mode), self.h)

    def begin_occ(self, min_occurrence=1):
        """FASTQ without -A (fastq2co): ids of keys seen at least min_occurrence times"""
        _check(lib.mk_sketch_begin_occ(self.h, min_occurrence), self.h)

    def push_bgzf(self, path, chunk_bytes=0, first_ordinal=0, qmin=None):
        """a BGZF-compressed FASTQ file into the sketch in progress (mk_sketch_push_bgzf) -> BgzfStatsC; a damaged member or a
        long line raises MkError(MK_ERR_FORMAT) with the statistics in .stats"""
        o, st = BgzfOptsC(chunk_bytes, 0), BgzfStatsC()
        fd = os.open(path, os.O_RDONLY)
        try:
            if qmin is None:
                rc = lib.mk_sketch_push_bgzf(self.h, fd, os.fstat(fd).st_size, C.byref(o), first_ordinal, C.byref(st))
            else:
                rc = lib.mk_sketch_push_bgzf_q(self.h, fd, os.fstat(fd).st_size, C.byref(o), qmin, first_ordinal, C.byref(st))
        finally:
            os.close(fd)
        if rc:
            err = MkError(rc, (lib.mk_bgzf_last_error() or b"").decode())
            err.stats = st
            raise err
        return st

    def push_gzip(self, path, span_bytes=0, ratio=0, batch_spans=0, first_ordinal=0, members=False, qmin=None, repair=False):
        """a single-member gzip FASTQ file into the sketch in progress (mk_sketch_push_gzip) -> GunzipStatsC; an inflate status or
        a long line raises MkError(MK_ERR_FORMAT) with the statistics in .stats: the sketch is then to be begun anew.  repair:
        MK_GUNZIP_REPAIR, false piece starts are repaired; gunzip_repairs() says how many were dropped"""
        o, st = GunzipOptsC(span_bytes, ratio, batch_spans, _gunzip_flags(members, repair)), GunzipStatsC()
        fd = os.open(path, os.O_RDONLY)
        try:
            if qmin is None:
                rc = lib.mk_sketch_push_gzip(self.h, fd, os.fstat(fd).st_size, C.byref(o), first_ordinal, C.byref(st))
            else:
                rc = lib.mk_sketch_push_gzip_q(self.h, fd, os.fstat(fd).st_size, C.byref(o), qmin, first_ordinal, C.byref(st))
        finally:
            os.close(fd)
        if rc:
            err = MkError(rc, (lib.mk_bgzf_last_error() or b"").decode())
            err.stats = st
            raise err
        return st

    def push_gzip_q(self, path, qmin=0, span_bytes=0, ratio=0, batch_spans=0, first_ordinal=0, members=False):
        """the same for a sketch begun with begin_occ (mk_sketch_push_gzip_q): fastq2co's record rule and its -Q mask (its
        parameter list is pinned by tests/test_abi_gunzip_q.py: with the repair it is push_gzip(..., qmin=q, repair=True))"""
        return self.push_gzip(path, span_bytes, ratio, batch_spans, first_ordinal, members, qmin=qmin)

    def gunzip_repairs(self):
        """piece starts the last push_gzip* call on this engine dropped (mk_sketch_gunzip_repairs)"""
        n = C.c_uint64(0)
        _check(lib.mk_sketch_gunzip_repairs(self.h, C.byref(n)), self.h)
        return n.value

    def push_bgzf_q(self, path, qmin=0, chunk_bytes=0, first_ordinal=0):
        """the same for a sketch begun with begin_occ (mk_sketch_push_bgzf_q): fastq2co's record rule and its -Q mask"""
        return self.push_bgzf(path, chunk_bytes, first_ordinal, qmin=qmin)

    def push_reads(self, rows, stride, first_read_ordinal=0):
        """rows: host numpy u8 array of nreads*stride bytes (stride | MK_ROWS_PACKED: 64-byte packed rows)"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        pitch = stride & ~MK_ROWS_PACKED
        assert rows.size % pitch == 0
        n = rows.size // pitch
        if n:
            _check(lib.mk_sketch_push_reads(self.h, rows.ctypes.data, stride, n, first_read_ordinal), self.h)
        return n

    def push_fastq(self, buf, nthreads=8, chunk_bytes=0, occ=False, TL=22, qmin=0, first_ordinal=0, inflight=2, packed=False):
        """whole FASTQ text (bytes / numpy u8 / mmap) -> framed by host threads and pushed (mk_sketch_push_fastq); returns stats"""
        b = np.frombuffer(buf, dtype=np.uint8)
        o = FastqOptsC(1 if occ else 0, qmin, TL, nthreads, inflight, chunk_bytes, 0, 0, 1 if packed else 0)
        st = FastqStatsC()
        _check(lib.mk_sketch_push_fastq(self.h, b.ctypes.data if len(b) else None, len(b), C.byref(o), first_ordinal, C.byref(st)), self.h)
        return st

    def push_stream(self, text, final=True, piece=None):
        """FASTA text as it is in the file -> mk_sketch_push_stream; piece: push in pieces of that many bytes (the last one final)"""
        b = np.frombuffer(bytes(text), dtype=np.uint8)
        if not piece:
            _check(lib.mk_sketch_push_stream(self.h, b.ctypes.data if len(b) else None, len(b), 1 if final else 0), self.h)
            return
        at = 0
        while True:
            n = min(piece, len(b) - at)
            last = at + n >= len(b)
            part = np.ascontiguousarray(b[at:at + n])
            _check(lib.mk_sketch_push_stream(self.h, part.ctypes.data if n else None, n, 1 if (last and final) else 0), self.h)
            at += n
            if last:
                break

    def push_fastq_long(self, text, final=True, piece=None):
        """FASTQ text as it is in the file, lines of any length -> mk_sketch_push_fastq_long; piece: push in pieces of that many bytes
        (the last one final)"""
        b = np.frombuffer(bytes(text), dtype=np.uint8)
        if not piece:
            _check(lib.mk_sketch_push_fastq_long(self.h, b.ctypes.data if len(b) else None, len(b), 1 if final else 0), self.h)
            return
        at = 0
        while True:
            n = min(piece, len(b) - at)
            last = at + n >= len(b)
            part = np.ascontiguousarray(b[at:at + n])
            _check(lib.mk_sketch_push_fastq_long(self.h, part.ctypes.data if n else None, n, 1 if (last and final) else 0), self.h)
            at += n
            if last:
                break

    def push_fastq_long_device(self, dev_ptr, n, final=True):
        """n bytes of FASTQ text at dev_ptr, in the memory of the engine's device, any alignment -> mk_sketch_push_fastq_long_device;
        returns with the work queued: the memory stays untouched until the next call on this engine that waits"""
        _check(lib.mk_sketch_push_fastq_long_device(self.h, C.c_void_p(dev_ptr) if n else None, n, 1 if final else 0), self.h)

    def fastq_long_frame_ms(self):
        """device milliseconds of the long-read framing kernels since begin() (mk_sketch_fastq_long_frame_ms)"""
        ms = C.c_double(0)
        _check(lib.mk_sketch_fastq_long_frame_ms(self.h, C.byref(ms)), self.h)
        return ms.value

    def push_gzip_long(self, path, span_bytes=0, ratio=0, batch_spans=0, members=False, final=True, repair=False):
        """a single-member gzip FASTQ file (members=True: a concatenation) into the MK_MODE_KOC sketch in progress by the long-read
        rule (mk_sketch_push_gzip_long) -> GunzipStatsC; an inflate status raises MkError(MK_ERR_FORMAT) with the statistics in
        .stats: the sketch is then to be finished, dropped and begun anew"""
        o, st = GunzipOptsC(span_bytes, ratio, batch_spans, _gunzip_flags(members, repair)), GunzipStatsC()
        fd = os.open(path, os.O_RDONLY)
        try:
            rc = lib.mk_sketch_push_gzip_long(self.h, fd, os.fstat(fd).st_size, C.byref(o), 1 if final else 0, C.byref(st))
        finally:
            os.close(fd)
        if rc:
            err = MkError(rc, (lib.mk_bgzf_last_error() or b"").decode())
            err.stats = st
            raise err
        return st

    def push_bgzf_long(self, path, chunk_bytes=0, final=True):
        """a BGZF-compressed FASTQ file into the MK_MODE_KOC sketch in progress by the long-read rule (mk_sketch_push_bgzf_long) ->
        BgzfStatsC; a damaged member raises MkError(MK_ERR_FORMAT) with the statistics in .stats"""
        o, st = BgzfOptsC(chunk_bytes, 0), BgzfStatsC()
        fd = os.open(path, os.O_RDONLY)
        try:
            rc = lib.mk_sketch_push_bgzf_long(self.h, fd, os.fstat(fd).st_size, C.byref(o), 1 if final else 0, C.byref(st))
        finally:
            os.close(fd)
        if rc:
            err = MkError(rc, (lib.mk_bgzf_last_error() or b"").decode())
            err.stats = st
            raise err
        return st

    def push_fastq_long_q(self, text, qmin, final=True, piece=None):
        """FASTQ text as it is in the file, lines of any length, into the begin(occ=...) sketch in progress by fastq2co's rule: bases
        whose quality byte is below qmin masked (mk_sketch_push_fastq_long_q); piece: push in pieces of that many bytes (the last
        one final)"""
        b = np.frombuffer(bytes(text), dtype=np.uint8)
        if not piece:
            _check(lib.mk_sketch_push_fastq_long_q(self.h, b.ctypes.data if len(b) else None, len(b), 1 if final else 0, qmin), self.h)
            return
        at = 0
        while True:
            n = min(piece, len(b) - at)
            last = at + n >= len(b)
            part = np.ascontiguousarray(b[at:at + n])
            _check(lib.mk_sketch_push_fastq_long_q(self.h, part.ctypes.data if n else None, n, 1 if (last and final) else 0, qmin), self.h)
            at += n
            if last:
                break

    def push_fastq_long_q_device(self, dev_ptr, n, qmin, final=True):
        """n bytes of FASTQ text at dev_ptr, in the memory of the engine's device, any alignment -> mk_sketch_push_fastq_long_q_device;
        returns with the work queued: the memory stays untouched until the next call on this engine that waits"""
        _check(lib.mk_sketch_push_fastq_long_q_device(self.h, C.c_void_p(dev_ptr) if n else None, n, 1 if final else 0, qmin), self.h)

    def push_gzip_long_q(self, path, qmin, span_bytes=0, ratio=0, batch_spans=0, members=False, final=True, repair=False):
        """push_gzip_long for the MK_MODE_OCC_SET sketch in progress, bases below qmin masked (mk_sketch_push_gzip_long_q) ->
        GunzipStatsC; statuses as push_gzip_long"""
        o, st = GunzipOptsC(span_bytes, ratio, batch_spans, _gunzip_flags(members, repair)), GunzipStatsC()
        fd = os.open(path, os.O_RDONLY)
        try:
            rc = lib.mk_sketch_push_gzip_long_q(self.h, fd, os.fstat(fd).st_size, C.byref(o), qmin, 1 if final else 0, C.byref(st))
        finally:
            os.close(fd)
        if rc:
            err = MkError(rc, (lib.mk_bgzf_last_error() or b"").decode())
            err.stats = st
            raise err
        return st

    def push_bgzf_long_q(self, path, qmin, chunk_bytes=0, final=True):
        """push_bgzf_long for the MK_MODE_OCC_SET sketch in progress, bases below qmin masked (mk_sketch_push_bgzf_long_q) ->
        BgzfStatsC; statuses as push_bgzf_long"""
        o, st = BgzfOptsC(chunk_bytes, 0), BgzfStatsC()
        fd = os.open(path, os.O_RDONLY)
        try:
            rc = lib.mk_sketch_push_bgzf_long_q(self.h, fd, os.fstat(fd).st_size, C.byref(o), qmin, 1 if final else 0, C.byref(st))
        finally:
            os.close(fd)
        if rc:
            err = MkError(rc, (lib.mk_bgzf_last_error() or b"").decode())
            err.stats = st
            raise err
        return st

    def push_reads_async(self, rows, stride, first_read_ordinal=0):
        """queue the copies and the scan; `rows` (host numpy u8) must stay untouched until push_wait(ticket)"""
        assert rows.dtype == np.uint8 and rows.flags["C_CONTIGUOUS"] and rows.size % stride == 0
        t = C.c_uint64(0)
        _check(lib.mk_sketch_push_reads_async(self.h, rows.ctypes.data, stride, rows.size // stride, first_read_ordinal, C.byref(t)), self.h)
        return t.value

    def push_wait(self, ticket):
        _check(lib.mk_sketch_push_wait(self.h, ticket), self.h)

    def push_reads_device(self, dev_ptr, stride, nreads, first_read_ordinal=0):
        _check(lib.mk_sketch_push_reads_device(self.h, C.c_void_p(dev_ptr), stride, nreads, first_read_ordinal), self.h)

    def finish(self):
        """-> list over components of (ids u32 array, counts u16 array or None), copies of the engine-owned result"""
        r = ResultC()
        _check(lib.mk_sketch_finish(self.h, C.byref(r)), self.h)
        out = []
        for c in range(r.component_num):
            comp = r.components[c]
            n = comp.n
            ids = np.ctypeslib.as_array(comp.ids, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            cnt = None
            if comp.counts:
                cnt = np.ctypeslib.as_array(comp.counts, shape=(n,)).copy() if n else np.zeros(0, np.uint16)
            out.append((ids, cnt))
        self.last_total = r.total
        lib.mk_result_release(self.h, C.byref(r))
        return out

    def finish_keys(self):
        """the finish that ends at the key list (mk_sketch_finish_keys) -> (keys device pointer, counts device pointer, n): the
        engine's own arrays (u64 keys, u32 counts), valid until the next call that begins or finishes a sketch"""
        k, c, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        _check(lib.mk_sketch_finish_keys(self.h, C.byref(k), C.byref(c), C.byref(n)), self.h)
        return k.value or 0, c.value or 0, n.value

    def batch_begin(self, texts, mode=MK_MODE_SET, one_buffer=False):
        """mk_sketch_batch_begin over a list of byte strings (FASTA texts).  one_buffer: lay the texts into ONE
        buffer at 1 KiB-aligned offsets (the single-copy layout) instead of separate arrays.  The buffers are kept until batch_end()."""
        arrs = []
        if one_buffer:
            offs, at = [], 0
            for t in texts:
                offs.append(at)
                at += (len(t) + 1023) // 1024 * 1024
            buf = np.zeros(max(at, 1024), dtype=np.uint8)  # (pageable here; the command line uses a pinned buffer)
            for t, o in zip(texts, offs):
                buf[o:o + len(t)] = np.frombuffer(bytes(t), dtype=np.uint8)
            arrs = [buf[o:o + len(t)] for t, o in zip(texts, offs)]
            keep = [buf]
        else:
            arrs = [np.frombuffer(bytes(t), dtype=np.uint8).copy() for t in texts]
            keep = arrs
        files = (BatchFileC * len(texts))()
        for i, a in enumerate(arrs):
            files[i].text = (keep[0].ctypes.data + offs[i]) if one_buffer else (a.ctypes.data if a.size else None)
            files[i].n = a.size
        _check(lib.mk_sketch_batch_begin(self.h, mode, C.cast(files, C.c_void_p), len(texts)), self.h)
        self._batches = getattr(self, "_batches", [])
        self._batches.append((keep, len(texts)))

    def batch_begin_rows(self, row_arrays, mode=MK_MODE_SET, pinned=False, fmt=MK_ROWS_PACKED, gap=MK_PACKED_PITCH):
        """mk_sketch_batch_begin_rows over the files' packed rows (fasta_pack_rows).  pinned: the rows are laid into ONE registered buffer,
        file behind file with `gap` bytes of 0xA5 between them (never looked at) -- the layout the scan kernel reads in place; otherwise separate pageable arrays."""
        n = len(row_arrays)
        files = (BatchFileC * n)()
        if pinned:
            # (hipHostMalloc, not hipHostRegister on a numpy array: registering and unregistering pieces of the malloc heap left the
            # runtime with stale pinned ranges -- a pageable copy 44 fuzz cases later faulted on the device, tools/fuzz_parity.py seed 2010)
            total = sum(a.size + gap for a in row_arrays) + 4096
            p = C.c_void_p()
            _check(lib.mk_host_alloc(C.byref(p), total))
            buf = np.ctypeslib.as_array((C.c_uint8 * total).from_address(p.value))
            buf[:] = 0xA5
            at = 0
            for i, a in enumerate(row_arrays):
                buf[at:at + a.size] = a
                files[i].text = p.value + at
                files[i].n = a.size
                at += a.size + gap
            del buf
            keep = ("pinned", None, p.value)
        else:
            arrs = []
            for i, a in enumerate(row_arrays):
                raw = np.zeros(a.size + 64, dtype=np.uint8)
                off = (-raw.ctypes.data) % 64
                raw[off:off + a.size] = a
                arrs.append(raw)
                files[i].text = (raw.ctypes.data + off) if a.size else None
                files[i].n = a.size
            keep = arrs
        _check(lib.mk_sketch_batch_begin_rows(self.h, mode, fmt, C.cast(files, C.c_void_p), n), self.h)
        self._batches = getattr(self, "_batches", [])
        self._batches.append((keep, n))

    def batch_begin_gz(self, gz_files, mode=MK_MODE_SET, one_buffer=False, gunzip=None):
        """mk_sketch_batch_begin_gz over a list of byte strings, each a gzip file mk_gzip_scan accepts.  one_buffer: the files lie in ONE
        16-byte aligned buffer at 1 KiB-aligned offsets (copied from where they are) instead of separate arrays (packed into staging).
        gunzip: a dict of mk_gunzip_opts fields (span_bytes, ratio, flags; may be empty) -> mk_sketch_batch_begin_gunzip, many
        wavefronts per file."""
        n = len(gz_files)
        files = (GzFileC * n)()
        if one_buffer:
            offs, at = [], 0
            for t in gz_files:
                offs.append(at)
                at += (len(t) + 1023) // 1024 * 1024
            raw = np.zeros(at + 1024 + 16, dtype=np.uint8)
            base = (-raw.ctypes.data) % 16
            for t, o in zip(gz_files, offs):
                raw[base + o:base + o + len(t)] = np.frombuffer(bytes(t), dtype=np.uint8)
            ptrs = [raw.ctypes.data + base + o for o in offs]
            keep = [raw]
        else:
            keep = [np.frombuffer(bytes(t), dtype=np.uint8).copy() for t in gz_files]
            ptrs = [a.ctypes.data for a in keep]
        for i, t in enumerate(gz_files):
            files[i].comp = ptrs[i]
            files[i].n = len(t)
            _check(lib.mk_gzip_scan(-1, ptrs[i], len(t), C.byref(files[i].info)))
        if gunzip is None:
            _check(lib.mk_sketch_batch_begin_gz(self.h, mode, files, n), self.h)
        else:
            o = GunzipOptsC(gunzip.get("span_bytes", 0), gunzip.get("ratio", 0), gunzip.get("batch_spans", 0), gunzip.get("flags", 0))
            _check(lib.mk_sketch_batch_begin_gunzip(self.h, mode, files, n, C.byref(o)), self.h)
        self._batches = getattr(self, "_batches", [])
        self._batches.append((keep, n))

    def batch_gz_pieces(self, n):
        """pieces per file of the batch the last batch_end() handed out (zeros: not begun with gunzip=)"""
        np_ = np.zeros(max(1, n), dtype=np.uint32)
        _check(lib.mk_sketch_batch_gz_pieces(self.h, np_.ctypes.data, n), self.h)
        return [int(x) for x in np_[:n]]

    def batch_gz_status(self, n):
        """MK_INFL_* per file of the batch the last batch_end() handed out"""
        st = np.zeros(max(1, n), dtype=np.uint32)
        _check(lib.mk_sketch_batch_gz_status(self.h, st.ctypes.data, n), self.h)
        return [int(x) for x in st[:n]]

    def batch_home_ids(self):
        """-> (with_batch, late): ids of the batch the last batch_end() handed out that came home in the batch's own launch sequence,
        and ids mk_sketch_batch_end fetched by its late copy (mk_sketch_batch_home_ids)"""
        w, l = C.c_uint64(0), C.c_uint64(0)
        _check(lib.mk_sketch_batch_home_ids(self.h, C.byref(w), C.byref(l)), self.h)
        return w.value, l.value

    def batch_end(self, views=False):
        """-> per file (status, alone, [ids per component]) of the oldest batch in flight.  views: the id arrays are the engine's own
        memory, not copies: valid until the next batch_end() on this engine"""
        if not getattr(self, "_batches", None):  # nothing in flight: let the library say so
            _check(lib.mk_sketch_batch_end(self.h, C.cast((C.c_uint8 * 64)(), C.c_void_p)), self.h)
            raise MkError(MK_ERR_STATE, "mk_sketch_batch_end returned MK_OK without a batch in flight")
        keep, n = self._batches.pop(0)

        class BatchResultC(C.Structure):
            _fields_ = [("status", C.c_int32), ("alone", C.c_int32), ("r", ResultC)]
        out = (BatchResultC * n)()
        _check(lib.mk_sketch_batch_end(self.h, C.cast(out, C.c_void_p)), self.h)
        res = []
        for i in range(n):
            comps = []
            if out[i].status == MK_OK:
                for c in range(out[i].r.component_num):
                    comp = out[i].r.components[c]
                    a = np.ctypeslib.as_array(comp.ids, shape=(comp.n,)) if comp.n else np.zeros(0, np.uint32)
                    comps.append(a if views else a.copy())
            res.append((out[i].status, out[i].alone, comps))
        if isinstance(keep, tuple) and keep[0] == "pinned":
            lib.mk_host_free(keep[2])
        del keep
        return res

    def finish_raw(self):
        r = ResultC()
        _check(lib.mk_sketch_finish(self.h, C.byref(r)), self.h)
        return r

    def finish_begin(self):
        """first half of a finish: when it returns the next sketch may be begun and pushed; finish_end() hands out the result"""
        _check(lib.mk_sketch_finish_begin(self.h), self.h)

    def finish_end_raw(self):
        r = ResultC()
        _check(lib.mk_sketch_finish_end(self.h, C.byref(r)), self.h)
        return r

    def finish_end(self):
        r = self.finish_end_raw()
        out = []
        for c in range(r.component_num):
            comp = r.components[c]
            n = comp.n
            ids = np.ctypeslib.as_array(comp.ids, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
            cnt = None
            if comp.counts:
                cnt = np.ctypeslib.as_array(comp.counts, shape=(n,)).copy() if n else np.zeros(0, np.uint16)
            out.append((ids, cnt))
        self.last_total = r.total
        return out

    def sync(self):
        _check(lib.mk_engine_sync(self.h), self.h)

    def partial_count(self):
        n = C.c_uint64(0)
        _check(lib.mk_partial_count(self.h, C.byref(n)), self.h)
        return n.value

    def partial_export(self, keys_ptr, counts_ptr, ords_ptr, capacity):
        n = C.c_uint64(0)
        _check(lib.mk_partial_export(self.h, C.c_void_p(keys_ptr), C.c_void_p(counts_ptr), C.c_void_p(ords_ptr), capacity,
                                     C.byref(n)), self.h)
        return n.value

    def partial_import(self, keys_ptr, counts_ptr, ords_ptr, n):
        _check(lib.mk_partial_import(self.h, C.c_void_p(keys_ptr), C.c_void_p(counts_ptr), C.c_void_p(ords_ptr), n), self.h)

    # ---- the merge by key slices (include/metakssd_hip.h) ----
    def partial_export_split(self, nparts, keys_ptr, counts_ptr, ords_ptr, capacity):
        """the distinct list cut into nparts parts by key % nparts -> (n, [part sizes])"""
        n = C.c_uint64(0)
        parts = (C.c_uint64 * 16)()
        _check(lib.mk_partial_export_split(self.h, nparts, C.c_void_p(keys_ptr), C.c_void_p(counts_ptr), C.c_void_p(ords_ptr), capacity,
                                           parts, C.byref(n)), self.h)
        return n.value, [int(parts[g]) for g in range(nparts)]

    def partial_restart(self):
        _check(lib.mk_partial_restart(self.h), self.h)

    def partial_list_reserve(self, n):
        """device pointers (keys, counts, ords) of the engine's own key list, room for n entries"""
        k, c, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib.mk_partial_list_reserve(self.h, n, C.byref(k), C.byref(c), C.byref(o)), self.h)
        return k.value, c.value, o.value

    def partial_list_adopt(self, keys_ptr, counts_ptr, ords_ptr, n, offset):
        _check(lib.mk_partial_list_adopt(self.h, C.c_void_p(keys_ptr), C.c_void_p(counts_ptr), C.c_void_p(ords_ptr), n, offset), self.h)

    def partial_list_commit(self, n):
        _check(lib.mk_partial_list_commit(self.h, n), self.h)

    def profile_enable(self, on=True):
        _check(lib.mk_profile_enable(self.h, 1 if on else 0), self.h)

    def profile_reset(self):
        _check(lib.mk_profile_reset(self.h), self.h)

    def profile(self):
        p = ProfileC()
        _check(lib.mk_profile_get(self.h, C.byref(p)), self.h)
        return {f: getattr(p, f) for f, _ in ProfileC._fields_}


def synth_rows_device(device, stream, seed, first_read, nreads, length, stride, dev_ptr):
    _check(lib.mk_synth_rows_device(device, C.c_void_p(stream), seed, first_read, nreads, length, stride, C.c_void_p(dev_ptr)))


# ---- libmetakssd_multi.so (include/metakssd_multi.h): several engines in ONE process, the product's own exchange (RCCL) ----
MK_MULTI_ALLOW_DEVICE_COPIES, MK_MULTI_FORCE_DEVICE_COPIES = 1, 2
MK_MULTI_MERGE_AUTO, MK_MULTI_MERGE_GATHER, MK_MULTI_MERGE_SLICES = 0, 1, 2
MULTI_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libmetakssd_multi.so")
_mlib = None


class MultiTimesC(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("export_ms", "exchange_ms", "import_ms", "gather_ms", "finish_ms", "total_ms")]


def _load_multi():
    global _mlib
    if _mlib is not None:
        return _mlib
    if not os.path.exists(MULTI_LIB_PATH):
        raise ImportError("%s not built (needs rccl/rccl.h and librccl.so: make -C metakssd_amd/csrc)" % MULTI_LIB_PATH)
    m = C.CDLL(MULTI_LIB_PATH)  # (pulls in librccl.so: only callers of Multi pay for that)
    vp = C.c_void_p
    m.mk_multi_create_ex.argtypes = [C.POINTER(ParamsC), C.POINTER(C.c_int), C.c_int, C.c_uint, C.POINTER(vp)]
    m.mk_multi_destroy.argtypes = [vp]
    m.mk_multi_last_error.argtypes = [vp]
    m.mk_multi_last_error.restype = C.c_char_p
    m.mk_multi_count.argtypes = [vp]
    m.mk_multi_engine.argtypes = [vp, C.c_int]
    m.mk_multi_engine.restype = vp
    m.mk_multi_transport.argtypes = [vp]
    m.mk_multi_transport.restype = C.c_char_p
    m.mk_multi_begin.argtypes = [vp, C.c_int]
    m.mk_multi_begin_occ.argtypes = [vp, C.c_int]
    m.mk_multi_finish.argtypes = [vp, C.POINTER(ResultC), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    m.mk_multi_set_merge.argtypes = [vp, C.c_int]
    m.mk_multi_last_merge.argtypes = [vp]
    m.mk_multi_last_merge.restype = C.c_char_p
    m.mk_multi_last_times.argtypes = [vp, C.POINTER(MultiTimesC)]
    _mlib = m
    return m


class Multi:
    """one sketch over several engines of ONE process (mk_multi_*): what `metakssd dist --devices a,b,..` runs on"""

    def __init__(self, shuf, devices, flags=0, component_sz=8):
        self.m = _load_multi()
        self.params = shuf.params(component_sz)
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self.m.mk_multi_create_ex(C.byref(self.params), arr, len(devices), flags, C.byref(h))
        if rc != MK_OK:
            raise MkError(rc, self.m.mk_multi_last_error(None).decode(errors="replace"))
        self.h = h
        self.n = len(devices)
        self.devices = list(devices)

    def _check(self, rc):
        if rc != MK_OK:
            raise (CrowdedError if rc == MK_ERR_CROWDED else MkError)(rc, self.m.mk_multi_last_error(self.h).decode(errors="replace"))

    def engine(self, i):
        return self.m.mk_multi_engine(self.h, i)

    def transport(self):
        return self.m.mk_multi_transport(self.h).decode()

    def set_merge(self, how):
        self._check(self.m.mk_multi_set_merge(self.h, how))

    def begin(self, mode=MK_MODE_KOC):
        self._check(self.m.mk_multi_begin(self.h, mode))

    def begin_occ(self, min_occurrence):
        self._check(self.m.mk_multi_begin_occ(self.h, min_occurrence))

    def push_reads_device(self, i, dev_ptr, stride, nreads, first_read_ordinal):
        e = self.engine(i)
        _check(lib.mk_sketch_push_reads_device(e, C.c_void_p(dev_ptr), stride, nreads, first_read_ordinal), e)

    def push_reads(self, i, rows, stride, first_read_ordinal):
        e = self.engine(i)
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        _check(lib.mk_sketch_push_reads(e, rows.ctypes.data_as(C.c_void_p), stride, rows.size // stride, first_read_ordinal), e)

    def finish_raw(self):
        """-> (ResultC of engine 0, gather_ms, tail_ms)"""
        r = ResultC()
        g, t = C.c_double(0), C.c_double(0)
        self._check(self.m.mk_multi_finish(self.h, C.byref(r), C.byref(g), C.byref(t)))
        return r, g.value, t.value

    def finish(self):
        r, g, t = self.finish_raw()
        out = []
        for c in range(r.component_num):
            comp = r.components[c]
            ids = np.ctypeslib.as_array(comp.ids, shape=(comp.n,)).copy() if comp.n else np.zeros(0, np.uint32)
            cnt = (np.ctypeslib.as_array(comp.counts, shape=(comp.n,)).copy() if comp.n else np.zeros(0, np.uint16)) if comp.counts else None
            out.append((ids, cnt))
        return out

    def last_merge(self):
        return self.m.mk_multi_last_merge(self.h).decode()

    def last_times(self):
        t = MultiTimesC()
        self._check(self.m.mk_multi_last_times(self.h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in MultiTimesC._fields_}

    def close(self):
        if getattr(self, "h", None):
            self.m.mk_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


MK_SET_UNION, MK_SET_UNIQ_UNION = 0, 1


class SetOp:
    """`metakssd set -u / -q` dictionaries on the device (mk_setop_*)"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib.mk_setop_create(device, C.byref(self.h))
        if rc:
            raise MkError(rc, (lib.mk_setop_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc:
            raise MkError(rc, (lib.mk_setop_last_error(self.h) or b"").decode())

    def union(self, id_lists, uniq=False):
        """id_lists: iterable of uint32 numpy arrays -> ascending uint32 array"""
        self._check(lib.mk_setop_begin(self.h, MK_SET_UNIQ_UNION if uniq else MK_SET_UNION))
        for a in id_lists:
            a = np.ascontiguousarray(a, dtype=np.uint32)
            if a.size:
                self._check(lib.mk_setop_add(self.h, a.ctypes.data, a.size))
        out, n = C.c_void_p(), C.c_uint64(0)
        self._check(lib.mk_setop_finish(self.h, C.byref(out), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint32)), shape=(n.value,)).copy()

    def begin(self, uniq=False):
        self._check(lib.mk_setop_begin(self.h, MK_SET_UNIQ_UNION if uniq else MK_SET_UNION))

    def add_device(self, dev_ptr, n):
        self._check(lib.mk_setop_add_device(self.h, C.c_void_p(dev_ptr), n))

    def finish_count(self):
        out, n = C.c_void_p(), C.c_uint64(0)
        self._check(lib.mk_setop_finish(self.h, C.byref(out), C.byref(n)))
        return n.value

    def stream(self):
        return lib.mk_setop_stream(self.h)

    def join(self, qry_ids, qry_counts, ref_ids, bounds):
        """composite -q's join (mk_setop_join): the query's count for every reference position whose id the query holds, in reference
        order, and where each reference sketch's segment of them ends -> (counts uint32, bounds_out uint64)"""
        q = np.ascontiguousarray(qry_ids, dtype=np.uint32)
        qa = np.ascontiguousarray(qry_counts, dtype=np.uint16)
        r = np.ascontiguousarray(ref_ids, dtype=np.uint32)
        b = np.ascontiguousarray(bounds, dtype=np.uint64)
        bout = np.zeros(b.size, np.uint64)
        out, n = C.c_void_p(), C.c_uint64(0)
        self._check(lib.mk_setop_join(self.h, q.ctypes.data if q.size else None, qa.ctypes.data if qa.size else None, q.size,
                                      r.ctypes.data if r.size else None, r.size, b.ctypes.data if b.size else None, b.size,
                                      C.byref(out), C.byref(n), bout.ctypes.data if b.size else None))
        cts = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint32)), shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint32)
        return cts, bout

    def last_join_ms(self):
        ms = C.c_double(0.0)
        self._check(lib.mk_setop_last_join_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            lib.mk_setop_destroy(self.h)
            self.h = C.c_void_p()


class Mco:
    """stage II inverted index and shared-k-mer counting on the device (mk_mco_*)"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib.mk_mco_create(device, C.byref(self.h))
        if rc:
            raise MkError(rc, (lib.mk_mco_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc:
            raise MkError(rc, (lib.mk_mco_last_error(self.h) or b"").decode())

    def build(self, ids, index, copy=True):
        """ids: uint32 (one component's combco.N), index: uint64[cofnum + 1] -> (gids, row_ids, row_ends).
        copy=False: views of the library's pinned result buffers, as the C caller gets them (valid until the next build / close)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        index = np.ascontiguousarray(index, dtype=np.uint64)
        g, ri, re_ = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, nr = C.c_uint64(0), C.c_uint64(0)
        self._check(lib.mk_mco_build(self.h, ids.ctypes.data if ids.size else None, index.ctypes.data, index.size - 1, C.byref(g),
                                     C.byref(n), C.byref(ri), C.byref(re_), C.byref(nr)))

        def arr(p, ct, k):
            if not k:
                return np.zeros(0, ct)
            a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(k,))
            return a.copy() if copy else a
        return arr(g, C.c_uint32, n.value), arr(ri, C.c_uint32, nr.value), arr(re_, C.c_uint64, nr.value)

    def sort_pairs(self, keys, vals):
        """stable sort of (u32 key, u32 value) pairs by key on the device (the sort inside build()); returns new arrays"""
        k = np.ascontiguousarray(keys, dtype=np.uint32).copy()
        v = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        assert k.size == v.size
        self._check(lib.mk_mco_sort_pairs(self.h, k.ctypes.data if k.size else None, v.ctypes.data if v.size else None, k.size))
        return k, v

    def index_rows(self, row0, nrows, pinned=False):
        """rows [row0, row0 + nrows) of the dense index.  pinned=True: into a pinned buffer this object keeps (what the command line
        does, mk_host_alloc), returned as a view that the next pinned call overwrites -- the slab then crosses at PCIe speed"""
        if pinned and nrows:
            if getattr(self, "_slab_cap", 0) < nrows:
                if getattr(self, "_slab", None):
                    lib.mk_host_free(self._slab)
                self._slab, self._slab_cap = C.c_void_p(), 0
                rc = lib.mk_host_alloc(C.byref(self._slab), nrows * 8)
                if rc:
                    raise MkError(rc, "mk_host_alloc")
                self._slab_cap = nrows
            self._check(lib.mk_mco_index_rows(self.h, row0, nrows, self._slab))
            return np.ctypeslib.as_array(C.cast(self._slab, C.POINTER(C.c_uint64)), shape=(nrows,))
        out = np.empty(nrows, np.uint64)
        self._check(lib.mk_mco_index_rows(self.h, row0, nrows, out.ctypes.data if nrows else None))
        return out

    def count(self, ref_num, qry_index, qry_ctx_ct, components):
        """components: iterable of dicts {gids (or None: last build), qry_ids, ext_start, ext_end (or None: device row table)};
        qry_index per component inside the dict.  Returns the qry_num x ref_num uint32 matrix."""
        qry_num = len(qry_ctx_ct)
        self._check(lib.mk_mco_count_begin(self.h, ref_num, qry_num))
        ctx = np.ascontiguousarray(qry_ctx_ct, dtype=np.uint32)
        for comp in components:
            qi = np.ascontiguousarray(comp.get("qry_index", qry_index), dtype=np.uint64)
            gids = comp.get("gids")
            gids = None if gids is None else np.ascontiguousarray(gids, dtype=np.uint32)
            qids = comp.get("qry_ids")
            qids = None if qids is None else np.ascontiguousarray(qids, dtype=np.uint32)
            es, ee = comp.get("ext_start"), comp.get("ext_end")
            es = None if es is None else np.ascontiguousarray(es, dtype=np.uint64)
            ee = None if ee is None else np.ascontiguousarray(ee, dtype=np.uint64)
            self._check(lib.mk_mco_count_add(self.h, gids.ctypes.data if gids is not None and gids.size else (None if gids is None else 0),
                                             0 if gids is None else gids.size,
                                             qids.ctypes.data if qids is not None and qids.size else None,
                                             es.ctypes.data if es is not None else None, ee.ctypes.data if ee is not None else None,
                                             qi.ctypes.data, ctx.ctypes.data if ctx.size else None))
        ct = np.zeros((qry_num, ref_num), np.uint32)
        if ct.size:
            self._check(lib.mk_mco_count_finish(self.h, ct.ctypes.data))
        return ct

    def last_kernel_ms(self):
        """(radix sort of the last build, kernels of the last count_add) in ms, from the handle's HIP events"""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._check(lib.mk_mco_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.h:
            if getattr(self, "_slab", None):
                lib.mk_host_free(self._slab)
                self._slab, self._slab_cap = None, 0
            lib.mk_mco_destroy(self.h)
            self.h = C.c_void_p()


BINVEC = np.dtype([("ref_idx", "<i4"), ("pct", "<f4")])  # mk_binvec = binVec_t (command_composite.h:12-16), the records of a .abv


class Abv:
    """abundance-vector index and search on the device (mk_abv_*: `composite -i` / `composite -s`, command_composite.c:212-440)"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib.mk_abv_create(device, C.byref(self.h))
        if rc:
            raise MkError(rc, (lib.mk_abv_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc:
            raise MkError(rc, (lib.mk_abv_last_error(self.h) or b"").decode())

    def index(self, vectors, nref):
        """vectors: the files' BINVEC arrays in directory order -> (abm BINVEC[n], abmi int32[nref], yl2n float64[len(vectors)]),
        the contents of abundance_Vec.{abm,abmi,yl2n}.  MkError(MK_ERR_FORMAT) names the file of a species outside 0..nref-1."""
        vs = [np.ascontiguousarray(v).view(BINVEC) for v in vectors]
        ent = np.ascontiguousarray(np.concatenate(vs) if vs else np.zeros(0, BINVEC))
        ends = np.cumsum([len(v) for v in vs], dtype=np.uint64) if vs else np.zeros(0, np.uint64)
        abm, abmi, yl2n, bad = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(-1)
        self._check(lib.mk_abv_index(self.h, ent.ctypes.data if ent.size else None, ent.size, ends.ctypes.data if ends.size else None,
                                     len(vs), nref, C.byref(abm), C.byref(abmi), C.byref(yl2n), C.byref(bad)))

        def arr(p, dt, k):
            if not k:
                return np.zeros(0, dt)
            return np.frombuffer((C.c_char * (k * np.dtype(dt).itemsize)).from_address(p.value), dtype=dt).copy()
        return arr(abm, BINVEC, ent.size), arr(abmi, np.int32, nref), arr(yl2n, np.float64, len(vs))

    def load(self, abm, abmi, yl2n):
        """keep an index resident on the device (nsamples = len(yl2n))"""
        abm = np.ascontiguousarray(abm).view(BINVEC)
        abmi = np.ascontiguousarray(abmi, dtype=np.int32)
        yl2n = np.ascontiguousarray(yl2n, dtype=np.float64)
        self._check(lib.mk_abv_load(self.h, abm.ctypes.data if abm.size else None, abm.size, abmi.ctypes.data if abmi.size else None,
                                    abmi.size, yl2n.ctypes.data if yl2n.size else None, yl2n.size))

    def search(self, metric, queries):
        """metric 0 cosine / 1 L1 / 2 L2; queries: BINVEC arrays -> per query (sample ids int32, float32 measures) in the order
        the reference prints them (for L2 the measure is the sum of squares; it prints the sqrt)"""
        qs = [np.ascontiguousarray(q).view(BINVEC) for q in queries]
        ent = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0, BINVEC))
        ends = np.cumsum([len(q) for q in qs], dtype=np.uint64) if qs else np.zeros(0, np.uint64)
        oend = np.zeros(max(len(qs), 1), np.uint64)
        ids, ms, bad = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
        self._check(lib.mk_abv_search(self.h, metric, len(qs), ent.ctypes.data if ent.size else None, ends.ctypes.data if ends.size else None,
                                      oend.ctypes.data, C.byref(ids), C.byref(ms), C.byref(bad)))
        out, lo = [], 0
        for k in range(len(qs)):
            hi = int(oend[k])
            if hi > lo:
                i = np.frombuffer((C.c_char * (4 * hi)).from_address(ids.value), dtype=np.int32)[lo:hi].copy()
                m = np.frombuffer((C.c_char * (4 * hi)).from_address(ms.value), dtype=np.float32)[lo:hi].copy()
            else:
                i, m = np.zeros(0, np.int32), np.zeros(0, np.float32)
            out.append((i, m))
            lo = hi
        return out

    def last_kernel_ms(self):
        """(kernels of the last index, kernels of the last search) in ms, from the handle's HIP events"""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._check(lib.mk_abv_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.h:
            lib.mk_abv_destroy(self.h)
            self.h = C.c_void_p()


MK_BYREAD_MAX_PUSH = 8 << 20


MK_INFL_OK, MK_INFL_BAD_BLOCK, MK_INFL_BAD_LENGTHS, MK_INFL_BAD_CODE, MK_INFL_BAD_DISTANCE, MK_INFL_INPUT, MK_INFL_OUTPUT_LEN, MK_INFL_CRC = range(8)
MK_INFL_TRAILING, MK_INFL_MISSED, MK_INFL_CAPACITY, MK_INFL_BAD_MEMBER = 8, 9, 10, 11
MK_GUNZIP_MEMBERS = 1
MK_GUNZIP_REPAIR = 2
MK_GUNZIP_REPAIR_MERGES = 8


def _gunzip_flags(members, repair):
    return (MK_GUNZIP_MEMBERS if members else 0) | (MK_GUNZIP_REPAIR if repair else 0)
MK_GUNZIP_PIECE_MEMBER = 1 << 63
MK_CRC_SLICE = 16384
BGZF_FIELDS = ("in_off", "out_off", "in_len", "pay_off", "pay_len", "crc32", "isize")


# mk_composite_row: what get_species_abundance() computes per (sample, reference sketch) (command_composite.c:599-613)
COMPOSITE_ROW = np.dtype([("ref", "<u4"), ("kmer_num", "<i4"), ("sum", "<i4"), ("lastsum", "<i4"), ("lastn", "<i4"), ("median", "<i4"),
                          ("top", "<i4")])
MK_COMPOSITE_OPT_MAX_HITS = 1


class Composite:
    """`composite -r <markerdb> -q <sketch_dir>` with the marker database resident on the device (mk_composite_*)"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib.mk_composite_create(device, C.byref(self.h))
        if rc:
            raise MkError(rc, (lib.mk_composite_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc:
            raise MkError(rc, (lib.mk_composite_last_error(self.h) or b"").decode())

    def set_option(self, option, value):
        self._check(lib.mk_composite_set_option(self.h, option, value))

    def load(self, ref_num, components):
        """components: per component (ids uint32, index uint64[ref_num + 1]) = combco.c / combco.index.c of the database"""
        self._check(lib.mk_composite_load_begin(self.h, ref_num, len(components)))
        for c, (ids, index) in enumerate(components):
            ids = np.ascontiguousarray(ids, dtype=np.uint32)
            index = np.ascontiguousarray(index, dtype=np.uint64)
            assert index.size == ref_num + 1
            self._check(lib.mk_composite_load_component(self.h, c, ids.ctypes.data if ids.size else None, index.ctypes.data))

    def query_begin(self, nsamples):
        self._check(lib.mk_composite_query_begin(self.h, nsamples))

    def query_component(self, c, ids, counts, index):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint16)
        index = np.ascontiguousarray(index, dtype=np.uint64)
        self._check(lib.mk_composite_query_component(self.h, c, ids.ctypes.data if ids.size else None,
                                                     counts.ctypes.data if counts.size else None, index.ctypes.data))

    def query_sample_keys(self, k, keys_ptr, counts_ptr, n, comp_code_bits):
        """sample k of the batch as a device list of n distinct keys (u64) and their counts (u32): mk_composite_query_sample_keys"""
        self._check(lib.mk_composite_query_sample_keys(self.h, k, C.c_void_p(keys_ptr or None), C.c_void_p(counts_ptr or None), n, comp_code_bits))

    def query_finish(self, nsamples):
        """-> per sample a COMPOSITE_ROW array in print order"""
        out = C.c_void_p()
        ends = np.zeros(max(nsamples, 1), np.uint64)
        self._check(lib.mk_composite_query_finish(self.h, C.byref(out), ends.ctypes.data))
        total = int(ends[nsamples - 1]) if nsamples else 0
        if total:
            buf = (C.c_char * (total * COMPOSITE_ROW.itemsize)).from_address(out.value)
            rows = np.frombuffer(buf, dtype=COMPOSITE_ROW).copy()
        else:
            rows = np.zeros(0, COMPOSITE_ROW)
        return [rows[(int(ends[k - 1]) if k else 0):int(ends[k])] for k in range(nsamples)]

    def query(self, nsamples, components):
        """components: per component (ids, counts, index uint64[nsamples + 1]) of the batch -> query_finish()'s rows"""
        self.query_begin(nsamples)
        for c, (ids, counts, index) in enumerate(components):
            self.query_component(c, ids, counts, index)
        return self.query_finish(nsamples)

    def last_kernel_ms(self):
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._check(lib.mk_composite_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_counts(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(lib.mk_composite_last_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.h:
            lib.mk_composite_destroy(self.h)
            self.h = C.c_void_p()


def bgzf_scan(data=None, path=None):
    """mk_bgzf_scan over bytes or over a file: None when the input is not BGZF from its first byte to its last, else a list of
    dicts (BGZF_FIELDS), one per member.  Host code: no GPU needed."""
    tab, nb, total, is_b = C.POINTER(BgzfBlockC)(), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    if path is not None:
        fd = os.open(path, os.O_RDONLY)
        try:
            _check(lib.mk_bgzf_scan(fd, None, os.fstat(fd).st_size, C.byref(tab), C.byref(nb), C.byref(total), C.byref(is_b)))
        finally:
            os.close(fd)
    else:
        b = np.frombuffer(bytes(data), dtype=np.uint8)
        _check(lib.mk_bgzf_scan(-1, b.ctypes.data if len(b) else C.c_void_p(1), len(b), C.byref(tab), C.byref(nb), C.byref(total), C.byref(is_b)))
    if not is_b.value:
        return None
    out = [{f: int(getattr(tab[i], f)) for f in BGZF_FIELDS} for i in range(nb.value)]
    assert total.value == sum(x["isize"] for x in out)
    lib.mk_bgzf_free(tab)
    return out


def gzip_scan(data=None, path=None):
    """mk_gzip_scan over bytes or over a file -> dict(pay_off, pay_len, crc32, isize), or None when the file is not a single-member
    gzip file for the device route.  Host code: no GPU needed."""
    info = GzipInfoC()
    if path is not None:
        fd = os.open(path, os.O_RDONLY)
        try:
            _check(lib.mk_gzip_scan(fd, None, os.fstat(fd).st_size, C.byref(info)))
        finally:
            os.close(fd)
    else:
        b = np.frombuffer(bytes(data), dtype=np.uint8)
        _check(lib.mk_gzip_scan(-1, b.ctypes.data if len(b) else C.c_void_p(1), len(b), C.byref(info)))
    if not info.is_single:
        assert (info.pay_off, info.pay_len, info.crc32, info.isize) == (0, 0, 0, 0)
        return None
    return {"pay_off": int(info.pay_off), "pay_len": int(info.pay_len), "crc32": int(info.crc32), "isize": int(info.isize)}


def gzip_scan_stream(data=None, path=None, raw=False):
    """mk_gzip_scan_stream over bytes or over a file -> dict(pay_off, pay_len, crc32, isize) (raw: the GzipInfoC), or None when the
    file is not one gzip member.  Host code: no GPU needed."""
    info = GzipInfoC()
    if path is not None:
        fd = os.open(path, os.O_RDONLY)
        try:
            _check(lib.mk_gzip_scan_stream(fd, None, os.fstat(fd).st_size, C.byref(info)))
        finally:
            os.close(fd)
    else:
        b = np.frombuffer(bytes(data), dtype=np.uint8)
        _check(lib.mk_gzip_scan_stream(-1, b.ctypes.data if len(b) else C.c_void_p(1), len(b), C.byref(info)))
    if not info.is_single:
        assert (info.pay_off, info.pay_len, info.crc32, info.isize) == (0, 0, 0, 0)
        return None
    return info if raw else {"pay_off": int(info.pay_off), "pay_len": int(info.pay_len), "crc32": int(info.crc32), "isize": int(info.isize)}


class Inflate:
    """BGZF members inflated and FASTQ text framed on the device (mk_inflate_*), with copies back to the host for tests"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib.mk_inflate_create(device, C.byref(self.h))
        if rc:
            raise MkError(rc, (lib.mk_inflate_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc:
            raise MkError(rc, (lib.mk_inflate_last_error(self.h) or b"").decode())

    def blocks(self, comp, table):
        """comp: the file's bytes, table: bgzf_scan's entries (or hand-made ones) -> (text bytes, status per member)"""
        b = np.frombuffer(bytes(comp), dtype=np.uint8)
        n = len(table)
        arr = (BgzfBlockC * max(1, n))()
        for i, t in enumerate(table):
            for f in BGZF_FIELDS:
                setattr(arr[i], f, t[f])
        end = max([t["out_off"] + t["isize"] for t in table] + [0])
        out = np.zeros(max(1, end), dtype=np.uint8)
        st = np.full(max(1, n), 0xFFFFFFFF, dtype=np.uint32)
        self._check(lib.mk_inflate_blocks(self.h, b.ctypes.data, len(b), arr, n, out.ctypes.data, end, st.ctypes.data))
        return out[:end].tobytes(), [int(x) for x in st[:n]]

    def members(self, comp, table, split=None, fill=0):
        """mk_inflate_members.  comp: bytes, table: dicts (pay_off, pay_len, out_off, isize, crc32) ->
        (text bytes, [(status, consumed, pos, crc32) per member]).  split: a dict of mk_gunzip_opts fields (span_bytes, ratio, flags)
        -> mk_inflate_members_split, many wavefronts per member, and a third value: [(start bit, text length) per piece] per member.
        fill: the byte the text buffer holds where no member wrote."""
        b = np.frombuffer(bytes(comp), dtype=np.uint8)
        n = len(table)
        arr = (GzMemberC * max(1, n))()
        for i, t in enumerate(table):
            for f in ("pay_off", "pay_len", "out_off", "isize", "crc32"):
                setattr(arr[i], f, t[f])
        end = max([t["out_off"] + t["isize"] for t in table] + [0])
        out = np.full(max(1, end), fill, dtype=np.uint8)
        res = (GzMemberResultC * max(1, n))()
        if split is None:
            self._check(lib.mk_inflate_members(self.h, b.ctypes.data if len(b) else None, len(b), arr, n, out.ctypes.data, end, res))
            return out[:end].tobytes(), [(int(r.status), int(r.consumed), int(r.pos), int(r.crc32)) for r in res[:n]]
        o = GunzipOptsC(split.get("span_bytes", 0), split.get("ratio", 0), split.get("batch_spans", 0), split.get("flags", 0))
        lists = (GunzipPiecesC * max(1, n))()
        rc = lib.mk_inflate_members_split(self.h, b.ctypes.data if len(b) else None, len(b), arr, n, C.byref(o), out.ctypes.data, end, res, lists)
        pieces = [[(int(p.v[k].start_bit), int(p.v[k].text_len)) for k in range(p.n)] for p in lists[:n]]
        for i in range(n):
            lib.mk_gunzip_pieces_free(C.byref(lists[i]))
        self._check(rc)
        return out[:end].tobytes(), [(int(r.status), int(r.consumed), int(r.pos), int(r.crc32)) for r in res[:n]], pieces

    def stream(self, comp, span_bytes=0, ratio=0, batch_spans=0, cap=None, guard=64, members=False, repair=False):
        """mk_inflate_stream over a whole gzip file (bytes) -> (text or None, MK_INFL_* status, [(start bit, text length) per piece],
        text length).  The text buffer has cap bytes (default: ISIZE, which is the text's length for texts below 4 GiB) between two
        guards of `guard` bytes, which must come back untouched.  members: MK_GUNZIP_MEMBERS, the file may be a concatenation of
        members; a piece is then (start bit, kind, text length) with kind 1 where it starts at a member's header, and the members
        whose end was met come as a fifth value.  cap must then be given for a text that is not ISIZE bytes long.  repair:
        MK_GUNZIP_REPAIR; the piece starts the repair dropped come as one more value, behind the others."""
        info = gzip_scan_stream(comp, raw=True)
        if info is None:
            raise MkError(MK_ERR_ARG, "not a single-member gzip file")
        b = np.frombuffer(bytes(comp), dtype=np.uint8)
        cap = int(info.isize) if cap is None else cap
        buf = np.full(cap + 2 * guard, 0xC3, dtype=np.uint8)
        o, n, st, pieces = GunzipOptsC(span_bytes, ratio, batch_spans, _gunzip_flags(members, repair)), C.c_uint64(0), C.c_int32(-1), GunzipPiecesC()
        rc = lib.mk_inflate_stream(self.h, b.ctypes.data, len(b), C.byref(info), C.byref(o), buf.ctypes.data + guard, cap, C.byref(n),
                                   C.byref(st), C.byref(pieces))
        table = [(int(pieces.v[i].start_bit), int(pieces.v[i].text_len)) for i in range(pieces.n)]
        lib.mk_gunzip_pieces_free(C.byref(pieces))
        self._check(rc)
        assert (buf[:guard] == 0xC3).all() and (buf[guard + cap:] == 0xC3).all(), "a write outside the text buffer"
        text = buf[guard:guard + n.value].tobytes() if st.value == 0 else None
        out = (text, st.value, table, n.value)
        if members:
            table = [(s & ~MK_GUNZIP_PIECE_MEMBER, s >> 63, t) for s, t in table]
            nm = C.c_uint64(0)
            self._check(lib.mk_inflate_stream_members(self.h, C.byref(nm)))
            out = (text, st.value, table, n.value, nm.value)
        if repair:
            nr = C.c_uint64(0)
            self._check(lib.mk_inflate_stream_repairs(self.h, C.byref(nr)))
            out += (nr.value,)
        return out

    def frame(self, text, final=True):
        """mk_fastq_frame_device -> (rows u8 [nrows * stride], stride, nrows, consumed, longest line, rc)"""
        b = np.frombuffer(bytes(text), dtype=np.uint8)
        cap = (len(b) // 4 + 1) * 4096 if len(b) < (1 << 16) else len(b) * 4 + 4096
        rows = np.zeros(cap, dtype=np.uint8)
        stride, nrows, used, longest = C.c_uint32(0), C.c_uint64(0), C.c_size_t(0), C.c_uint32(0)
        rc = lib.mk_fastq_frame_device(self.h, b.ctypes.data if len(b) else None, len(b), 1 if final else 0, rows.ctypes.data, cap,
                                       C.byref(stride), C.byref(nrows), C.byref(used), C.byref(longest))
        return rows[: nrows.value * stride.value], stride.value, nrows.value, used.value, longest.value, rc

    def frame_q(self, text, qmin=0, final=True, records_before=0):
        """mk_fastq_frame_q_device -> (rows u8 [nrows * stride], stride, nrows, nrecords, consumed, longest line, rc)"""
        b = np.frombuffer(bytes(text), dtype=np.uint8)
        cap = (len(b) // 4 + 1) * 4096 if len(b) < (1 << 16) else len(b) * 4 + 4096
        rows = np.zeros(cap, dtype=np.uint8)
        stride, nrows, nrec, used, longest = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_size_t(0), C.c_uint32(0)
        rc = lib.mk_fastq_frame_q_device(self.h, b.ctypes.data if len(b) else None, len(b), 1 if final else 0, qmin, records_before,
                                         rows.ctypes.data, cap, C.byref(stride), C.byref(nrows), C.byref(nrec), C.byref(used), C.byref(longest))
        return rows[: nrows.value * stride.value], stride.value, nrows.value, nrec.value, used.value, longest.value, rc

    def kernel_ms(self):
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._check(lib.mk_inflate_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.h:
            lib.mk_inflate_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ByRead:
    """`dist --byread` and `reverse` on the device (mk_byread_*: reads2mco(), iseq2comem.c:88-214; command_reverse.c:148-368)"""

    def __init__(self, shuf, device=0, component_sz=8):
        self.h = C.c_void_p()
        rc = lib.mk_byread_create(device, C.byref(self.h))
        if rc:
            raise MkError(rc, (lib.mk_byread_last_error(None) or b"").decode())
        self.shuf = shuf  # the table must outlive the handle
        self.params = shuf.params(component_sz)
        self.begin()

    def _check(self, rc):
        if rc:
            raise MkError(rc, (lib.mk_byread_last_error(self.h) or b"").decode())

    def begin(self):
        self._check(lib.mk_byread_begin(self.h, C.byref(self.params)))
        C_ = self.params.component_num
        self._ids = [[] for _ in range(C_)]
        self._index = [[] for _ in range(C_)]

    def push_text(self, text, final=False):
        """the next bytes of the file (at most MK_BYREAD_MAX_PUSH); what the push added is taken and kept for finish()"""
        buf = np.frombuffer(bytes(text), dtype=np.uint8)
        self._check(lib.mk_byread_push_text(self.h, buf.ctypes.data if buf.size else None, buf.size, 1 if final else 0))
        for c in range(self.params.component_num):
            ids, idx, nid, nix = C.c_void_p(), C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
            self._check(lib.mk_byread_take(self.h, c, C.byref(ids), C.byref(nid), C.byref(idx), C.byref(nix)))
            if nid.value:
                self._ids[c].append(np.frombuffer((C.c_char * (4 * nid.value)).from_address(ids.value), dtype=np.uint32).copy())
            if nix.value:
                self._index[c].append(np.frombuffer((C.c_char * (8 * nix.value)).from_address(idx.value), dtype=np.uint64).copy())

    def finish(self):
        """-> (ids per component uint32, index per component uint64 [records + 1], records, kernel ms)"""
        rec, tot, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
        self._check(lib.mk_byread_finish(self.h, C.byref(rec), C.byref(tot), C.byref(ms)))
        ids = [np.concatenate(x) if x else np.zeros(0, np.uint32) for x in self._ids]
        index = [np.concatenate(x) if x else np.zeros(0, np.uint64) for x in self._index]
        assert sum(len(i) for i in ids) == tot.value
        return ids, index, rec.value, ms.value

    def run(self, text, pieces=None):
        """a whole text: begin, pushes of `pieces` bytes each (default MK_BYREAD_MAX_PUSH; a list gives the cut points), finish"""
        self.begin()
        text = bytes(text)
        if isinstance(pieces, (list, tuple)):
            cuts = [0] + list(pieces) + [len(text)]
        else:
            step = pieces or MK_BYREAD_MAX_PUSH
            cuts = list(range(0, len(text), step)) + [len(text)]
            if len(cuts) == 1:
                cuts = [0, 0]
        for i in range(len(cuts) - 1):
            self.push_text(text[cuts[i]:cuts[i + 1]], final=i == len(cuts) - 2)
        return self.finish()

    def reverse_ids(self, ids, component):
        """the text `reverse` prints for these ids of one component: lines of 2k letters + newline, as bytes"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.empty(ids.size * (self.params.TL + 1), np.uint8)
        self._check(lib.mk_reverse_ids(self.h, ids.ctypes.data if ids.size else None, ids.size, component, out.ctypes.data if out.size else None))
        return out.tobytes()

    def last_kernel_ms(self):
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._check(lib.mk_byread_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.h:
            lib.mk_byread_destroy(self.h)
            self.h = C.c_void_p()


def reverse_ids(shuf, ids, component, device=0):
    """one-shot form of ByRead.reverse_ids"""
    b = ByRead(shuf, device)
    try:
        return b.reverse_ids(ids, component)
    finally:
        b.close()


def dist_print(path, ref_ctx_ct, qry_ctx_ct, refnames, qrynames, ct, kmerlen, dim_rd_len, metric=0, outfields=2, correction=0,
               num_neigb=0, dthreshold=1.0):
    """write distance.out through mk_dist_print (host code: needs no GPU); names: lists of str"""
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]

    def pack(names):
        b = bytearray(256 * len(names))
        for i, nm in enumerate(names):
            e = nm.encode()[:255]
            b[256 * i:256 * i + len(e)] = e
        return bytes(b)
    rn, qn = pack(refnames), pack(qrynames)
    rc_, qc_ = np.ascontiguousarray(ref_ctx_ct, dtype=np.uint32), np.ascontiguousarray(qry_ctx_ct, dtype=np.uint32)
    ct = np.ascontiguousarray(ct, dtype=np.uint32)
    o = DistOptsC(metric, outfields, correction, num_neigb, dthreshold)
    fp = libc.fopen(path.encode(), b"w")
    if not fp:
        raise OSError("cannot open %s" % path)
    rc = lib.mk_dist_print(fp, C.byref(o), kmerlen, dim_rd_len, rc_.size, qc_.size, rc_.ctypes.data if rc_.size else None,
                           qc_.ctypes.data if qc_.size else None, rn, qn, ct.ctypes.data if ct.size else None)
    libc.fclose(fp)
    return rc
