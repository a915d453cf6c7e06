"""ctypes binding of libhophip.so (include/hophip.h) for tests/ and bench.py.

This is plumbing, not the product: the product is the shared library and the C++ host mirror in
hevc-hop_amd/host/.  There is no CPU fallback here or in the library -- loading fails loudly when the
library has not been built, and every hot-path call fails with HOP_ERR_DEVICE without a gfx950 GPU.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libhophip.so")
STAMPS_LIB_PATH = os.path.join(HERE, "libhophip_stamps.so")      # the diagnostic build with the walks' stage stamps: HOP_LIB=<this> (Context.walk_stamps)

HOP_STAGE_INT, HOP_STAGE_FRAC, HOP_STAGE_GT = 1, 2, 3
HOP_ERR_ARG, HOP_ERR_STATE = -1, -3
HOP_FLAG_FEN, HOP_FLAG_HADME = 1, 2
HOP_TU_RD_TS, HOP_TU_RD_KEEP = 1, 2
HOP_DIST_SAD, HOP_DIST_SSE, HOP_DIST_HADS = 0, 1, 2


class PuJob(ctypes.Structure):
    _fields_ = [("pu_x", ctypes.c_int32), ("pu_y", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("rng_left", ctypes.c_int32), ("rng_right", ctypes.c_int32), ("rng_top", ctypes.c_int32), ("rng_bottom", ctypes.c_int32),
                ("off_x", ctypes.c_int32), ("off_y", ctypes.c_int32), ("pred_x", ctypes.c_int32), ("pred_y", ctypes.c_int32),
                ("lambda_cost", ctypes.c_uint32), ("n_amvp", ctypes.c_int32), ("amvp", ctypes.c_int32 * 4), ("flags", ctypes.c_int32)]


class PuResult(ctypes.Structure):
    _fields_ = [("mv_int", ctypes.c_int32 * 2), ("sad", ctypes.c_uint32), ("not_valid", ctypes.c_int32),
                ("half", ctypes.c_int32 * 2), ("qter", ctypes.c_int32 * 2), ("frac_cost", ctypes.c_uint32),
                ("gt_flag", ctypes.c_int32), ("gt", ctypes.c_int32 * 8), ("cost", ctypes.c_uint32),
                ("mv_final", ctypes.c_int32 * 2), ("half_final", ctypes.c_int32 * 2), ("qter_final", ctypes.c_int32 * 2)]


class PredJob(ctypes.Structure):
    _fields_ = [("pu_x", ctypes.c_int32), ("pu_y", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("mv_x", ctypes.c_int32), ("mv_y", ctypes.c_int32), ("use_gt", ctypes.c_int32), ("gt", ctypes.c_int32 * 8), ("dst_row_off", ctypes.c_int32)]


class DistJob(ctypes.Structure):
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("comp", ctypes.c_int32), ("kind", ctypes.c_int32)]


class TuJob(ctypes.Structure):
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("comp", ctypes.c_int32), ("log2_size", ctypes.c_int32),
                ("use_dst", ctypes.c_int32), ("transform_skip", ctypes.c_int32), ("qp_scaled", ctypes.c_int32), ("is_i_slice", ctypes.c_int32),
                ("sign_hide", ctypes.c_int32), ("scan_idx", ctypes.c_int32)]


class TuResult(ctypes.Structure):
    _fields_ = [("abs_sum", ctypes.c_uint32), ("sse", ctypes.c_uint32)]


class IntraJob(ctypes.Structure):
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("size", ctypes.c_int32), ("strong", ctypes.c_int32), ("flags", ctypes.c_uint8 * 68)]


RDOQ_JOB_DTYPE = np.dtype([("log2_size", "<i4"), ("comp", "<i4"), ("is_intra", "<i4"), ("scan_idx", "<i4"), ("tr_depth", "<i4"), ("qp_scaled", "<i4"),
                           ("bit_depth", "<i4"), ("sign_hide", "<i4"), ("lambda", "<f8"), ("coeff_offset", "<i8"), ("estbits_index", "<i4"), ("reserved", "<i4")])
ESTBITS_INTS = 4 + 84 + 32 + 32 + 48 + 12 + 24 + 8       # hop_estbits as a flat int32 array
COEFF_BITS_JOB_DTYPE = np.dtype([("log2_size", "<i4"), ("comp", "<i4"), ("scan_idx", "<i4"), ("sign_hide", "<i4"), ("use_ts", "<i4"), ("ts_flag", "<i4"),
                                 ("ctx_index", "<i4"), ("cbf_ctx_plus1", "<i4"), ("coeff_offset", "<i8")])
CABAC_CTX_BYTES = 152
TU_RD_JOB_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("comp", "<i4"), ("log2_size", "<i4"), ("qp_scaled", "<i4"), ("tr_depth", "<i4"), ("ctx_index", "<i4"),
                            ("sign_hide", "<i4"), ("use_ts", "<i4"), ("bit_depth", "<i4"), ("is_intra", "<i4"), ("scan_idx", "<i4"), ("use_dst", "<i4"), ("flags", "<i4"),
                            ("lambda_rdoq", "<f8"), ("lambda_rd", "<f8"), ("dist_weight", "<f8")])
RQT_JOB_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("log2_cu", "<i4"), ("qp_scaled", "<i4", (3,)), ("ctx_index", "<i4"), ("sign_hide", "<i4"), ("use_ts", "<i4"),
                          ("log2_max_tu", "<i4"), ("log2_min_tu_in_cu", "<i4"), ("inter_split_flag", "<i4"), ("lambda_rd", "<f8"), ("lambda_rdoq", "<f8", (3,)),
                          ("dist_weight", "<f8", (2,))])
RQT_RESULT_DTYPE = np.dtype([("cost", "<f8"), ("bits", "<u4"), ("dist", "<u4"), ("zero_dist", "<u4"), ("pad", "<u4"), ("tr_idx", "u1", (256,)), ("cbf", "u1", (3, 256)),
                             ("tskip", "u1", (3, 256))])
CABAC_CU_CTX_BYTES = 20
CU_SYNTAX_DTYPE = np.dtype([("part_size", "<i4"), ("n_pu", "<i4"), ("skip_flag", "<i4"), ("skip_ctx", "<i4"), ("amp_acc", "<i4"), ("is_min_cu", "<i4"), ("max_merge_cand", "<i4"),
                            ("pu", [("merge_flag", "<i4"), ("merge_idx", "<i4"), ("mvd", "<i4", (2,)), ("mvp_idx", "<i4"), ("gt_flag", "<i4"), ("gt", "<i4", (8,))], (4,))])
INTRA_MODES_JOB_DTYPE = np.dtype([("preds", "<i4", (3,)), ("pred_num", "<i4"), ("mpm_cand", "<i4"), ("num_full_rd", "<i4"), ("ctx_state", "<i4"), ("frac_left", "<i4"), ("sqrt_lambda", "<f8")])
INTRA_MODES_RESULT_DTYPE = np.dtype([("n", "<u4"), ("modes", "<u4", (11,)), ("costs", "<f8", (8,))])
INTRA_CU_SYNTAX_DTYPE = np.dtype([("part_nxn", "<i4"), ("skip_flag", "<i4"), ("skip_ctx", "<i4"), ("is_min_cu", "<i4"), ("luma_dir", "<i4", (4,)), ("preds", "<i4", (4, 3)),
                                  ("pred_num", "<i4", (4,)), ("chroma_is_dm", "<i4"), ("chroma_dir", "<i4"), ("tr_depth", "<i4"), ("part", "<i4"), ("b_luma", "<i4"), ("b_chroma", "<i4")])
INTRA_RQT_OPT_DTYPE = np.dtype([("check_first", "<i4"), ("ts_fast", "<i4"), ("strong", "<i4"), ("pad", "<i4"), ("avail", "<u8", (341,))])   # hop_intra_rqt_opt
INTRA_SEARCH_JOB_DTYPE = np.dtype([("left_dir", "<i4", (4,)), ("above_dir", "<i4", (4,)), ("rough_flags", "u1", (4, 68)), ("sqrt_lambda", "<f8"), ("num_full_rd", "<i4"),
                                   ("pad", "<i4")])                                                   # hop_intra_search_job
INTRA_SEARCH_RESULT_DTYPE = np.dtype([("best_dir", "<i4", (4,)), ("n_cand", "<i4", (4,)), ("dist", "<u4"), ("pad", "<u4")])
TU_RD_RESULT_DTYPE = np.dtype([("abs_sum", "<u4"), ("cbf", "<u4"), ("dist", "<u4"), ("zero_dist", "<u4"), ("nonzero_dist", "<u4"), ("bits", "<u4"),
                               ("null_bits", "<u4"), ("pad", "<u4"), ("cost", "<f8")])
TU_JOB_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("comp", "<i4"), ("log2_size", "<i4"), ("use_dst", "<i4"), ("transform_skip", "<i4"),
                         ("qp_scaled", "<i4"), ("is_i_slice", "<i4"), ("sign_hide", "<i4"), ("scan_idx", "<i4")])
INTRA_JOB_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("size", "<i4"), ("strong", "<i4"), ("flags", "u1", (68,))])
assert TU_JOB_DTYPE.itemsize == ctypes.sizeof(TuJob) and INTRA_JOB_DTYPE.itemsize == ctypes.sizeof(IntraJob)
PU_JOB_DTYPE = np.dtype([("pu_x", "<i4"), ("pu_y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("rng_left", "<i4"), ("rng_right", "<i4"),
                         ("rng_top", "<i4"), ("rng_bottom", "<i4"), ("off_x", "<i4"), ("off_y", "<i4"), ("pred_x", "<i4"), ("pred_y", "<i4"),
                         ("lambda_cost", "<u4"), ("n_amvp", "<i4"), ("amvp", "<i4", (4,)), ("flags", "<i4")])
PU_RESULT_DTYPE = np.dtype([("mv_int", "<i4", (2,)), ("sad", "<u4"), ("not_valid", "<i4"), ("half", "<i4", (2,)), ("qter", "<i4", (2,)),
                            ("frac_cost", "<u4"), ("gt_flag", "<i4"), ("gt", "<i4", (8,)), ("cost", "<u4"), ("mv_final", "<i4", (2,)),
                            ("half_final", "<i4", (2,)), ("qter_final", "<i4", (2,))])
assert PU_JOB_DTYPE.itemsize == ctypes.sizeof(PuJob) and PU_RESULT_DTYPE.itemsize == ctypes.sizeof(PuResult)

CU_PART_DTYPE = np.dtype([("depth", "u1"), ("pred_mode", "u1"), ("part_size", "u1"), ("skip", "u1"), ("merge_flag", "u1"), ("merge_idx", "u1"), ("gt_flag", "u1"), ("inter_dir", "u1"),
                          ("ref_idx", "i1"), ("mvp_idx", "i1"), ("mvp_num", "i1"), ("luma_dir", "u1"), ("chroma_dir", "u1"), ("tr_idx", "u1"), ("cbf", "u1", 3), ("tskip", "u1", 3),
                          ("mv", "<i2", 2), ("mvd", "<i2", 2), ("gt", "<i2", 8)])                           # hop_cu_part


class EncParams(ctypes.Structure):       # hop_enc_params
    _fields_ = [("qp", ctypes.c_int32), ("mi_size", ctypes.c_int32), ("first_ctus", ctypes.c_int32), ("wpp", ctypes.c_int32), ("wavefront_lag", ctypes.c_int32),
                ("plain_intra", ctypes.c_int32), ("streams", ctypes.c_int32), ("trace_path", ctypes.c_char_p)]


SAO_PARAM_DTYPE = np.dtype([("mode", "i1"), ("type", "i1"), ("aux", "i1"), ("pad", "i1"), ("offset", "i1", 32)])          # hop_sao_param


class SaoParams(ctypes.Structure):       # hop_sao_params
    _fields_ = [("lambda", ctypes.c_double * 3), ("enabled", ctypes.c_int32 * 3), ("slice_type", ctypes.c_int32), ("qp", ctypes.c_int32), ("rd_fraction", ctypes.c_uint32)]


class DeblockParams(ctypes.Structure):   # hop_deblock_params
    _fields_ = [("qp", ctypes.c_int32), ("beta_offset_div2", ctypes.c_int32), ("tc_offset_div2", ctypes.c_int32), ("cb_qp_offset", ctypes.c_int32), ("cr_qp_offset", ctypes.c_int32),
                ("disable", ctypes.c_int32)]


class QuantMode(ctypes.Structure):       # hop_quant_mode
    _fields_ = [("rdoq", ctypes.c_int32), ("rdoq_ts", ctypes.c_int32), ("i_slice", ctypes.c_int32)]


class DecParams(ctypes.Structure):       # hop_dec_params
    _fields_ = [("qp", ctypes.c_int32), ("cb_qp_offset", ctypes.c_int32), ("cr_qp_offset", ctypes.c_int32), ("plain_intra", ctypes.c_int32), ("schedule", ctypes.c_int32)]


HOP_K_ENTROPY_CTX, HOP_K_ENTROPY = 21, 22          # hop_profile_read ids of hop_slice_data_write's context pass and coding pass
HOP_K_PARSE = 23                                   # ... and of hop_slice_data_parse's launches
HOP_K_ESCAPE, HOP_K_PICHASH = 24, 25               # ... of the emulation-prevention launches and the checksum pass (hop_access_unit_write, hop_rbsp_escape, hop_picture_hash)
HOP_K_UNESCAPE = 26                                # ... of the count, scan and compact launches that remove emulation prevention (hop_rbsp_unescape, hop_access_unit_read / _decode)
HOP_K_WALK_INTER, HOP_K_WALK_INTRA, HOP_K_WALK_INTRA_NXN = 12, 16, 20   # ... of the candidate walks (+ log2 CU size - 3 for the first two)

# the stage stamps of the candidate walks (hop_walk_stamps_*: libhophip_stamps.so, loaded with HOP_LIB): stages, stamped kernels
HOP_WS_COUNT = 15
(HOP_WS_LEAF_FORWARD, HOP_WS_LEAF_ESTBITS, HOP_WS_LEAF_RDOQ, HOP_WS_LEAF_BITS, HOP_WS_LEAF_WAIT, HOP_WS_LEAF_INVERSE, HOP_WS_LEAF_DECIDE, HOP_WS_NODE_BEGIN, HOP_WS_NODE_SINGLE,
 HOP_WS_NODE_CLOSE, HOP_WS_PREDICT, HOP_WS_COPY, HOP_WS_TAIL, HOP_WS_CU_BITS, HOP_WS_OTHER) = range(HOP_WS_COUNT)
HOP_WSK_NAMES = ("k_inter_walk", "k_iw_begin", "k_iw_cand", "k_iw_pick", "k_iw_chroma", "k_iw_finish", "k_intra_walk")
HOP_WSK_INTER_WALK, HOP_WSK_IW_BEGIN, HOP_WSK_IW_CAND, HOP_WSK_IW_PICK, HOP_WSK_IW_CHROMA, HOP_WSK_IW_FINISH, HOP_WSK_INTRA_WALK = range(7)
HOP_WSK_COUNT = 7


class WalkStampsTotal(ctypes.Structure):   # hop_walk_stamps_total
    _fields_ = [("workgroups", ctypes.c_uint64), ("cycles", ctypes.c_uint64), ("realtime_ticks", ctypes.c_uint64), ("max_realtime_ticks", ctypes.c_uint64)]


def walk_stamps_stage_names(L):
    """hop_walk_stamps_stage_name for every stage, in the order of HOP_WS_*"""
    L.hop_walk_stamps_stage_name.argtypes = [ctypes.c_int]; L.hop_walk_stamps_stage_name.restype = ctypes.c_char_p
    return [L.hop_walk_stamps_stage_name(s).decode() for s in range(HOP_WS_COUNT)]


PARSE_GUARD = 256   # bytes behind each output of the slice-data parser that must come back untouched


def _parse_io(n, data, sizes, with_levels, with_sao):
    """the parser's input as an exact-length copy, its outputs with PARSE_GUARD bytes of 0xA5 behind each"""
    data = np.frombuffer(bytes(data), np.uint8).copy() if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8).copy()
    sizes = np.ascontiguousarray(sizes, np.uint32)
    assert int(sizes.astype(np.uint64).sum()) == data.size, "the substream sizes do not add up to the data"
    if data.size == 0:
        data = np.zeros(1, np.uint8)
    out = [np.full(nbytes + PARSE_GUARD, 0xA5, np.uint8) if on else None
           for nbytes, on in ((n * 256 * CU_PART_DTYPE.itemsize, True), (n * 6144 * 4, with_levels), (n * 3 * SAO_PARAM_DTYPE.itemsize, with_sao))]
    return data, sizes, out


def _parse_out(n, out, who):
    for b in out:
        assert b is None or np.all(b[-PARSE_GUARD:] == 0xA5), who + " stored past an output"
    parts = out[0][:-PARSE_GUARD].view(CU_PART_DTYPE).reshape(n, 256)
    levels = None if out[1] is None else out[1][:-PARSE_GUARD].view(np.int32).reshape(n, 6144)
    sao = None if out[2] is None else out[2][:-PARSE_GUARD].view(SAO_PARAM_DTYPE).reshape(n, 3)
    return parts, levels, sao


class SliceDataParams(ctypes.Structure):   # hop_slice_data_params
    _fields_ = [("qp", ctypes.c_int32), ("slice_type", ctypes.c_int32), ("wpp", ctypes.c_int32), ("plain_intra", ctypes.c_int32), ("sao_luma", ctypes.c_int32),
                ("sao_chroma", ctypes.c_int32), ("mi_size", ctypes.c_int32)]


class StreamParams(ctypes.Structure):   # hop_stream_params
    _fields_ = [("slice", SliceDataParams), ("poc", ctypes.c_int32), ("parameter_sets", ctypes.c_int32), ("hash", ctypes.c_int32)]


class StreamInfo(ctypes.Structure):   # hop_stream_info
    _fields_ = [("pic_w", ctypes.c_int32), ("pic_h", ctypes.c_int32), ("bit_depth", ctypes.c_int32), ("params", StreamParams), ("nal_type", ctypes.c_int32),
                ("n_substreams", ctypes.c_int32), ("header_bytes", ctypes.c_int32)]


_I16P = ctypes.POINTER(ctypes.c_int16)


class HopError(RuntimeError):
    pass


# every mirror of a hophip.h struct kept in this file, by the C name hop_sizeof() knows it under; load() refuses a library whose structs have another size
MIRRORS = {"hop_pu_job": PU_JOB_DTYPE, "hop_pu_result": PU_RESULT_DTYPE, "hop_pred_job": PredJob, "hop_dist_job": DistJob, "hop_tu_job": TU_JOB_DTYPE, "hop_tu_result": TuResult,
           "hop_intra_job": INTRA_JOB_DTYPE, "hop_rdoq_job": RDOQ_JOB_DTYPE, "hop_coeff_bits_job": COEFF_BITS_JOB_DTYPE, "hop_tu_rd_job": TU_RD_JOB_DTYPE,
           "hop_tu_rd_result": TU_RD_RESULT_DTYPE, "hop_intra_modes_job": INTRA_MODES_JOB_DTYPE, "hop_intra_modes_result": INTRA_MODES_RESULT_DTYPE, "hop_rqt_job": RQT_JOB_DTYPE,
           "hop_rqt_result": RQT_RESULT_DTYPE, "hop_cu_syntax": CU_SYNTAX_DTYPE, "hop_intra_cu_syntax": INTRA_CU_SYNTAX_DTYPE, "hop_intra_rqt_opt": INTRA_RQT_OPT_DTYPE,
           "hop_intra_search_job": INTRA_SEARCH_JOB_DTYPE, "hop_intra_search_result": INTRA_SEARCH_RESULT_DTYPE, "hop_cu_part": CU_PART_DTYPE, "hop_enc_params": EncParams,
           "hop_deblock_params": DeblockParams, "hop_sao_param": SAO_PARAM_DTYPE, "hop_sao_params": SaoParams, "hop_dec_params": DecParams,
           "hop_slice_data_params": SliceDataParams, "hop_stream_params": StreamParams, "hop_stream_info": StreamInfo, "hop_walk_stamps_total": WalkStampsTotal, "hop_quant_mode": QuantMode}


def mirror_size(m):
    return m.itemsize if isinstance(m, np.dtype) else ctypes.sizeof(m)


HOP_EVAL_INTER, HOP_EVAL_INTRA = 0, 1


def eval_expected_ms(L, cls):
    """hop_eval_expected_ms: the expected length of the chain of an evaluation group of class cls = (kind, log2 CU size, flag, candidates)"""
    L.hop_eval_expected_ms.argtypes = [ctypes.c_void_p]; L.hop_eval_expected_ms.restype = ctypes.c_double
    a = np.array(cls, np.int32)
    return float(L.hop_eval_expected_ms(a.ctypes.data))


def eval_place(L, cls, streams, pitch=16):
    """hop_eval_place: the evaluation stream a new group of class cls is issued on; streams[s] = the classes issued on stream s and not yet collected"""
    L.hop_eval_place.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]; L.hop_eval_place.restype = ctypes.c_int
    n_pending = np.array([len(q) for q in streams], np.int32)
    pending = np.full((len(streams), pitch, 4), -7, np.int32)              # (what lies beyond n_pending[s] is not a class and is not read)
    for s, q in enumerate(streams):
        for k, c in enumerate(q): pending[s, k] = c
    a = np.array(cls, np.int32)
    return int(L.hop_eval_place(a.ctypes.data, len(streams), n_pending.ctypes.data, pending.ctypes.data, pitch))


def load():
    global LIB_PATH
    if os.environ.get("HOP_LIB"): LIB_PATH = os.environ["HOP_LIB"]      # (development: a differently built library)
    if not os.path.exists(LIB_PATH):
        raise HopError("libhophip.so is not built (run `make -C hevc-hop_amd` or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    L.hop_sizeof.argtypes = [ctypes.c_char_p]
    for name, m in MIRRORS.items():
        if L.hop_sizeof(name.encode()) != mirror_size(m):
            raise HopError("%s: this binding lays the struct out in %d bytes, libhophip.so in %d" % (name, mirror_size(m), L.hop_sizeof(name.encode())))
    L.hop_last_error.restype = ctypes.c_char_p
    L.hop_last_error.argtypes = [ctypes.c_void_p]
    L.hop_version.restype = ctypes.c_char_p
    L.hop_stream.restype = ctypes.c_void_p
    L.hop_stream.argtypes = [ctypes.c_void_p]
    L.hop_component_bits.restype = ctypes.c_uint32
    L.hop_bits_gt.restype = ctypes.c_uint32
    for n in ("hop_ctx_destroy", "hop_sync", "hop_ssref_reset"):
        getattr(L, n).argtypes = [ctypes.c_void_p]
    L.hop_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)] + [ctypes.c_int] * 5
    L.hop_upload_orig.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.hop_ssref_commit_cus.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.hop_ssref_commit_cus_device.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.hop_ssref_download.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.hop_ssref_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.hop_pred_download.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.hop_me_search.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.hop_me_search_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.hop_pred_inter.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.hop_pred_inter_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.hop_distortion.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.hop_pred_jobs_from_results_device.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.hop_tu_roundtrip.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.hop_intra_rough.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.hop_rdoq.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 3
    L.hop_rdoq_device.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
    L.hop_rdoq.restype = L.hop_rdoq_device.restype = ctypes.c_int
    L.hop_tu_rd.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
    L.hop_tu_rd_device.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
    L.hop_tu_rd.restype = L.hop_tu_rd_device.restype = ctypes.c_int
    L.hop_intra_pred.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.hop_intra_pred_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.hop_intra_pred.restype = L.hop_intra_pred_device.restype = ctypes.c_int
    L.hop_cabac_init.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.hop_cabac_est_bits.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.hop_coeff_bits.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 3
    L.hop_coeff_bits_device.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
    for n in ("hop_cabac_init", "hop_cabac_est_bits", "hop_coeff_bits", "hop_coeff_bits_device"):
        getattr(L, n).restype = ctypes.c_int
    L.hop_tu_roundtrip_device.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.hop_intra_rough_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.hop_distortion_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    for n in ("hop_tu_roundtrip_device", "hop_intra_rough_device", "hop_distortion_device"):
        getattr(L, n).restype = ctypes.c_int
    for n in ("hop_recon_upload", "hop_recon_download", "hop_pred_upload"):
        getattr(L, n).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        getattr(L, n).restype = ctypes.c_int
    L.hop_tu_roundtrip.restype = ctypes.c_int
    L.hop_intra_rough.restype = ctypes.c_int
    L.hop_enumerate_ctu_jobs.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32,
                                                               ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.hop_profile_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.hop_profile_reset.argtypes = [ctypes.c_void_p]
    L.hop_profile_read.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for n in ("hop_ctx_create", "hop_sync", "hop_ssref_reset", "hop_upload_orig", "hop_ssref_commit_cus", "hop_ssref_commit_cus_device",
              "hop_ssref_download", "hop_ssref_upload", "hop_pred_download", "hop_me_search", "hop_me_search_device", "hop_pred_inter",
              "hop_pred_inter_device", "hop_distortion", "hop_pred_jobs_from_results_device", "hop_enumerate_ctu_jobs",
              "hop_profile_enable", "hop_profile_reset", "hop_profile_read"):
        getattr(L, n).restype = ctypes.c_int
    L.hop_set_search_range.argtypes = [ctypes.c_int] * 14 + [ctypes.POINTER(ctypes.c_int)]
    L.hop_me_finish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32,
                                ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    return L


class Context:
    """Thin RAII wrapper over hop_ctx_* for the tests and the bench."""

    def __init__(self, pic_w, pic_h, bit_depth=8, device=0, lib=None, pictures=1, slots=0):
        """pictures > 1: a stacked context (hop_ctx_set_stack) of that many independent pic_w x pic_h pictures; self.H is the height of the stack, self.sub_h / self.pitch
        the pictures' height and spacing, picture k at rows k * pitch."""
        self.L = lib or load()
        self.h = ctypes.c_void_p()
        self.pictures, self.sub_h, self.pitch = pictures, pic_h, 0
        if pictures > 1:
            self.pitch = self.L.hop_stack_pitch(pic_h)
            pic_h = (pictures - 1) * self.pitch + pic_h
        self.W, self.H, self.bit_depth = pic_w, pic_h, bit_depth
        r = self.L.hop_ctx_create(ctypes.byref(self.h), pic_w, pic_h, bit_depth, bit_depth, device)
        if r != 0:
            raise HopError("hop_ctx_create: %d %s" % (r, self.L.hop_last_error(None).decode()))
        if pictures > 1:
            self.L.hop_ctx_set_stack.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
            self._chk(self.L.hop_ctx_set_stack(self.h, self.sub_h, self.pitch), "hop_ctx_set_stack")
        self.slots = slots
        if slots:                     # candidate slots (hop_ctx_set_slots): hop_encode_frame evaluates the SS/GT candidates of a CU side by side
            self.L.hop_ctx_set_slots.argtypes = [ctypes.c_void_p, ctypes.c_int]
            self._chk(self.L.hop_ctx_set_slots(self.h, slots), "hop_ctx_set_slots")

    def stack(self, planes, chroma=False):
        """the pictures' planes (a list of arrays) laid out as the context's stack"""
        sh, pt = (self.sub_h >> 1, self.pitch >> 1) if chroma else (self.sub_h, self.pitch)
        out = np.zeros(((self.pictures - 1) * pt + sh, planes[0].shape[1]), np.int16)
        for k, a in enumerate(planes):
            out[k * pt:k * pt + sh] = a
        return out

    def unstack(self, plane, chroma=False):
        sh, pt = (self.sub_h >> 1, self.pitch >> 1) if chroma else (self.sub_h, self.pitch)
        return [plane[k * pt:k * pt + sh] for k in range(self.pictures)]

    def close(self):
        if self.h:
            self.L.hop_ctx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r, what):
        if r != 0:
            e = HopError("%s: %d %s" % (what, r, self.L.hop_last_error(self.h).decode()))
            e.code = r                  # HOP_ERR_*
            raise e

    def upload_orig(self, Y, Cb, Cr):
        Y, Cb, Cr = (np.ascontiguousarray(a, np.int16) for a in (Y, Cb, Cr))
        self._chk(self.L.hop_upload_orig(self.h, Y.ctypes.data, Y.shape[1], Cb.ctypes.data, Cr.ctypes.data, Cb.shape[1]), "hop_upload_orig")

    def ssref_reset(self):
        self._chk(self.L.hop_ssref_reset(self.h), "hop_ssref_reset")
        self._chk(self.L.hop_sync(self.h), "hop_sync")

    def ssref_commit(self, rects, recY, recCb, recCr):
        r4 = np.zeros((len(rects), 4), np.int32)
        r4[:, :3] = np.asarray(rects, np.int32).reshape(-1, 3)
        recY, recCb, recCr = (np.ascontiguousarray(a, np.int16) for a in (recY, recCb, recCr))
        self._chk(self.L.hop_ssref_commit_cus(self.h, len(rects), r4.ctypes.data, recY.ctypes.data, recCb.ctypes.data, recCr.ctypes.data), "hop_ssref_commit_cus")

    def ssref_download(self, comp):
        shape = (self.H + 160, self.W + 160) if comp == 0 else (self.H // 2 + 80, self.W // 2 + 80)
        a = np.empty(shape, np.int16)
        self._chk(self.L.hop_ssref_download(self.h, comp, a.ctypes.data), "hop_ssref_download")
        return a

    def ssref_upload(self, comp, buf):
        buf = np.ascontiguousarray(buf, np.int16)
        self._chk(self.L.hop_ssref_upload(self.h, comp, buf.ctypes.data), "hop_ssref_upload")

    def me_search(self, jobs, stage=HOP_STAGE_GT):
        jobs = np.ascontiguousarray(jobs, PU_JOB_DTYPE)
        res = np.zeros(len(jobs), PU_RESULT_DTYPE)
        self._chk(self.L.hop_me_search(self.h, len(jobs), jobs.ctypes.data, res.ctypes.data, stage), "hop_me_search")
        return res

    def pred_inter(self, jobs):
        n = len(jobs)
        arr = (PredJob * n)(*jobs)
        tot = sum(j.w * j.h for j in jobs)
        oy, ocb, ocr = np.empty(tot, np.int16), np.empty(tot // 4, np.int16), np.empty(tot // 4, np.int16)
        self._chk(self.L.hop_pred_inter(self.h, n, ctypes.addressof(arr), oy.ctypes.data, ocb.ctypes.data, ocr.ctypes.data), "hop_pred_inter")
        return oy, ocb, ocr

    def pred_download(self, comp):
        shape = (self.H, self.W) if comp == 0 else (self.H // 2, self.W // 2)
        a = np.empty(shape, np.int16)
        self._chk(self.L.hop_pred_download(self.h, comp, a.ctypes.data), "hop_pred_download")
        return a

    def distortion(self, jobs):
        n = len(jobs)
        arr = (DistJob * n)(*jobs)
        out = np.zeros(n, np.uint32)
        self._chk(self.L.hop_distortion(self.h, n, ctypes.addressof(arr), out.ctypes.data), "hop_distortion")
        return out

    def plane_upload(self, what, comp, a):
        a = np.ascontiguousarray(a, np.int16)
        self._chk(getattr(self.L, "hop_%s_upload" % what)(self.h, comp, a.ctypes.data), "hop_%s_upload" % what)

    def recon_download(self, comp):
        shape = (self.H, self.W) if comp == 0 else (self.H // 2, self.W // 2)
        a = np.empty(shape, np.int16)
        self._chk(self.L.hop_recon_download(self.h, comp, a.ctypes.data), "hop_recon_download")
        return a

    def encode_frame(self, qp=32, mi_size=16, first_ctus=0, trace_path=None, wpp=0, wavefront_lag=0, streams=0, plain_intra=0):
        """hop_encode_frame: the RD spine over the kernels for the resident original.  Returns per-CTU (cost, bits, dist), parts (n_ctu, 256) CU_PART_DTYPE, candidates."""
        L = self.L
        L.hop_encode_frame.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_void_p]
        assert L.hop_sizeof_cu_part() == CU_PART_DTYPE.itemsize
        n = ((self.W + 63) // 64) * ((self.sub_h + 63) // 64) * self.pictures      # a stacked context: picture k's CTUs at [k * n / pictures, ...)
        cost = np.zeros(n, np.float64); bits = np.zeros(n, np.uint32); dist = np.zeros(n, np.uint32); parts = np.zeros((n, 256), CU_PART_DTYPE)
        nc = ctypes.c_uint64(0)
        p = EncParams(qp, mi_size, first_ctus, wpp, wavefront_lag, plain_intra, streams, trace_path.encode() if trace_path else None)
        self._chk(L.hop_encode_frame(self.h, ctypes.byref(p), cost.ctypes.data, bits.ctypes.data, dist.ctypes.data, parts.ctypes.data, ctypes.byref(nc)), "hop_encode_frame")
        return cost, bits, dist, parts, int(nc.value)

    def encode_progress(self):
        """hop_encode_progress: CTUs the running (or last) hop_encode_frame has retired; callable from another thread"""
        v = ctypes.c_int64(0)
        self.L.hop_encode_progress.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_encode_progress(self.h, ctypes.byref(v)), "hop_encode_progress")
        return int(v.value)

    def encode_cancel(self):
        """hop_encode_cancel: the running hop_encode_frame (wavefront mode) starts no further CTU and returns what it has"""
        self.L.hop_encode_cancel.argtypes = [ctypes.c_void_p]
        self._chk(self.L.hop_encode_cancel(self.h), "hop_encode_cancel")

    def set_shard(self, rank, world, allgather=None):
        """hop_encode_set_shard: the next encode_frame (wavefront mode) codes the CTU rows r % world == rank of ONE picture and exchanges every step's finished CTUs through
        `allgather` (an object with a ctypes callback .fn of type shard.ALLGATHER_FN, e.g. shard.TorchAllgather); every rank ends with the whole picture"""
        self.L.hop_encode_set_shard.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        self._shard = allgather                      # (keeps the callback alive)
        fn = ctypes.cast(allgather.fn, ctypes.c_void_p) if allgather is not None else None
        self._chk(self.L.hop_encode_set_shard(self.h, rank, world, fn, None), "hop_encode_set_shard")

    def set_row_limit(self, on):
        """hop_ctx_set_row_limit: the searches, predictions and validity probes read the SS reference as raster order has it -- the sentinel from the bottom of the PU's CTU row on"""
        self.L.hop_ctx_set_row_limit.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self._chk(self.L.hop_ctx_set_row_limit(self.h, 1 if on else 0), "hop_ctx_set_row_limit")

    def set_exact(self, on):
        """hop_encode_set_exact (sticky): encode_frame in wavefront mode takes the raster-order decisions for any wavefront_lag >= 2 -- row limit below, waits on the row above"""
        self.L.hop_encode_set_exact.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self._chk(self.L.hop_encode_set_exact(self.h, 1 if on else 0), "hop_encode_set_exact")

    def levels_download(self):
        """hop_levels_download: (n_ctu, 6144) int32 -- per CTU 4096 luma + 1024 Cb + 1024 Cr levels in the reference's TComDataCU layout"""
        n = ((self.W + 63) // 64) * ((self.sub_h + 63) // 64) * self.pictures
        a = np.zeros((n, 6144), np.int32)
        self.L.hop_levels_download.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_levels_download(self.h, a.ctypes.data), "hop_levels_download")
        return a

    def deblock_frame(self, parts, qp, beta_offset_div2=0, tc_offset_div2=0, cb_qp_offset=0, cr_qp_offset=0, disable=0):
        """hop_deblock_frame: the deblocking filter over the resident reconstruction picture(s), in place; parts as encode_frame returned them"""
        parts = np.ascontiguousarray(parts)
        n = ((self.W + 63) // 64) * ((self.sub_h + 63) // 64) * self.pictures
        assert parts.nbytes == n * 256 * CU_PART_DTYPE.itemsize, (parts.shape, parts.dtype, n)
        p = DeblockParams(qp, beta_offset_div2, tc_offset_div2, cb_qp_offset, cr_qp_offset, disable)
        self.L.hop_deblock_frame.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_deblock_frame(self.h, ctypes.byref(p), parts.ctypes.data), "hop_deblock_frame")

    def _n_ctu(self):
        return ((self.W + 63) // 64) * ((self.sub_h + 63) // 64) * self.pictures

    def sao_stats(self):
        """hop_sao_stats: (n_ctu, 3, 5, 32, 2) int32 -- per CTU, component, type, class: count and sum of (original - reconstruction)"""
        a = np.zeros((self._n_ctu(), 3, 5, 32, 2), np.int32)
        self.L.hop_sao_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_sao_stats(self.h, a.ctypes.data), "hop_sao_stats")
        return a

    def sao_frame(self, lambdas, slice_type, qp, rd_fraction, enabled=(1, 1, 1)):
        """hop_sao_frame: statistics, decision, offsets for the resident picture(s); returns the coded parameters (n_ctu, 3) SAO_PARAM_DTYPE"""
        p = SaoParams((ctypes.c_double * 3)(*lambdas), (ctypes.c_int32 * 3)(*enabled), slice_type, qp, rd_fraction)
        coded = np.zeros((self._n_ctu(), 3), SAO_PARAM_DTYPE)
        self.L.hop_sao_frame.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_sao_frame(self.h, ctypes.byref(p), coded.ctypes.data), "hop_sao_frame")
        return coded

    def sao_frame_pictures(self, params):
        """hop_sao_frame_pictures: sao_frame with picture k decided under params[k] = (lambdas, slice_type, qp, rd_fraction[, enabled]) -- what the pictures of a stack coded
        at different QPs (set_picture_qps) need; returns the coded parameters (n_ctu, 3) SAO_PARAM_DTYPE of the stack"""
        assert len(params) == self.pictures, (len(params), self.pictures)
        arr = (SaoParams * len(params))()
        for k, q in enumerate(params):
            lambdas, slice_type, qp, rd_fraction = q[:4]
            enabled = q[4] if len(q) > 4 else (1, 1, 1)
            arr[k] = SaoParams((ctypes.c_double * 3)(*lambdas), (ctypes.c_int32 * 3)(*enabled), slice_type, qp, rd_fraction)
        coded = np.zeros((self._n_ctu(), 3), SAO_PARAM_DTYPE)
        self.L.hop_sao_frame_pictures.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_sao_frame_pictures(self.h, arr, coded.ctypes.data), "hop_sao_frame_pictures")
        return coded

    def set_picture_qps(self, qps):
        """hop_ctx_set_picture_qps (sticky): one QP per picture of the context; while set, encode_frame, deblock_frame, slice_data_write / parse, access_unit_write and
        decode_stack give picture k the QP qps[k] and ignore their own qp argument.  None (or an empty list) clears the table; so does hop_ctx_set_stack."""
        self.L.hop_ctx_set_picture_qps.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        if qps is None or len(qps) == 0:
            self._chk(self.L.hop_ctx_set_picture_qps(self.h, 0, None), "hop_ctx_set_picture_qps")
            return
        a = np.ascontiguousarray(qps, np.int32)
        self._chk(self.L.hop_ctx_set_picture_qps(self.h, len(a), a.ctypes.data), "hop_ctx_set_picture_qps")

    def set_quant_mode(self, rdoq=1, rdoq_ts=1, i_slice=0):
        """hop_ctx_set_quant_mode (sticky): a transform unit is quantised by RDOQ iff (its transform_skip_flag ? rdoq_ts : rdoq), otherwise by the reference's plain quantiser
        (offset 171 with i_slice, else 85) and its sign-bit hiding.  set_quant_mode(None) passes NULL: back to the default {1, 1, 0}.  encode_frame takes i_slice from its
        plain_intra, whatever was set here."""
        self.L.hop_ctx_set_quant_mode.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        if rdoq is None:
            self._chk(self.L.hop_ctx_set_quant_mode(self.h, None), "hop_ctx_set_quant_mode")
            return
        m = QuantMode(int(rdoq), int(rdoq_ts), int(i_slice))
        self._chk(self.L.hop_ctx_set_quant_mode(self.h, ctypes.byref(m)), "hop_ctx_set_quant_mode")

    def sao_apply(self, recon):
        recon = np.ascontiguousarray(recon)
        assert recon.nbytes == self._n_ctu() * 3 * SAO_PARAM_DTYPE.itemsize
        self.L.hop_sao_apply.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_sao_apply(self.h, recon.ctypes.data), "hop_sao_apply")

    def decode_frame(self, parts, levels, qp=32, cb_qp_offset=0, cr_qp_offset=0, plain_intra=0, schedule=0):
        """hop_decode_frame: the picture reconstructed from parts (n_ctu, 256) CU_PART_DTYPE and levels (n_ctu, 6144) int32 as encode_frame / levels_download give
        them; afterwards recon_download / ssref_download / deblock_frame / sao_apply work as after an encode.  schedule 0: dependency levels, 1: raster."""
        parts = np.ascontiguousarray(parts, CU_PART_DTYPE); levels = np.ascontiguousarray(levels, np.int32)
        n = self._n_ctu()
        if parts.size != n * 256 or levels.size != n * 6144:
            raise HopError("decode_frame: %d CTUs need (%d, 256) parts and (%d, 6144) levels" % (n, n, n))
        p = DecParams(qp, cb_qp_offset, cr_qp_offset, plain_intra, schedule)
        self.L.hop_decode_frame.argtypes = [ctypes.c_void_p] * 4
        self._chk(self.L.hop_decode_frame(self.h, ctypes.byref(p), parts.ctypes.data, levels.ctypes.data), "hop_decode_frame")

    def decode_stack(self, parts, levels, qp=32, cb_qp_offset=0, cr_qp_offset=0, plain_intra=0, schedule=0):
        """hop_decode_stack: decode_frame for every picture of a stacked context side by side -- parts and levels picture after picture, as encode_frame /
        levels_download / slice_data_parse give them for a stack.  On an unstacked context it is decode_frame."""
        parts = np.ascontiguousarray(parts, CU_PART_DTYPE); levels = np.ascontiguousarray(levels, np.int32)
        n = self._n_ctu()
        if parts.size != n * 256 or levels.size != n * 6144:
            raise HopError("decode_stack: %d CTUs need (%d, 256) parts and (%d, 6144) levels" % (n, n, n))
        p = DecParams(qp, cb_qp_offset, cr_qp_offset, plain_intra, schedule)
        self.L.hop_decode_stack.argtypes = [ctypes.c_void_p] * 4
        self._chk(self.L.hop_decode_stack(self.h, ctypes.byref(p), parts.ctypes.data, levels.ctypes.data), "hop_decode_stack")

    def access_units_decode(self, aus, active=None, want_outputs=True, want_levels=True):
        """hop_access_units_decode: a list of access units' bytes, one per picture of the context, to the pictures resident in it (recon_download, unstack).  Returns
        (StreamInfo per picture, hash_match per picture [3]: 1 equal, 0 different, -1 not checked, parts, levels, coded SAO parameters or None -- the stack's, picture after
        picture); want_outputs False: the three are not asked for (None); want_levels False: the levels alone are not (they then never leave the device)."""
        aus = [bytes(a) for a in aus]
        stream = np.frombuffer(b"".join(aus) or b"\0", np.uint8).copy()
        sizes = (ctypes.c_size_t * max(1, len(aus)))(*[len(a) for a in aus])
        n = self._n_ctu()
        infos = (StreamInfo * max(1, len(aus)))()
        match = np.full((max(1, len(aus)), 3), -2, np.int32)
        out = [np.full(nb + PARSE_GUARD, 0xA5, np.uint8) if want_outputs and on else None
               for nb, on in ((n * 256 * CU_PART_DTYPE.itemsize, True), (n * 6144 * 4, want_levels), (n * 3 * SAO_PARAM_DTYPE.itemsize, True))]
        self.L.hop_access_units_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 6
        r = self.L.hop_access_units_decode(self.h, stream.ctypes.data, sizes, len(aus), None if active is None else ctypes.byref(active), infos, match.ctypes.data,
                                           *[None if b is None else b.ctypes.data for b in out])
        for b in out:
            assert b is None or np.all(b[-PARSE_GUARD:] == 0xA5), "hop_access_units_decode stored past an output"
        if r != 0:
            e = HopError("hop_access_units_decode: %d %s" % (r, self.L.hop_last_error(self.h).decode()))
            e.code = r
            raise e
        infos = [StreamInfo.from_buffer_copy(bytes(i)) for i in infos][:len(aus)]
        if not want_outputs:
            return infos, match.tolist(), None, None, None
        parts = out[0][:-PARSE_GUARD].view(CU_PART_DTYPE).reshape(n, 256)
        levels = None if out[1] is None else out[1][:-PARSE_GUARD].view(np.int32).reshape(n, 6144)
        sl = infos[0].params.slice
        sao = out[2][:-PARSE_GUARD].view(SAO_PARAM_DTYPE).reshape(n, 3) if (sl.sao_luma or sl.sao_chroma) else None
        return infos, match.tolist(), parts, levels, sao

    def slice_data_write(self, parts, levels=None, sao_coded=None, qp=32, slice_type=3, wpp=0, plain_intra=0, sao_luma=None, sao_chroma=None, mi_size=16, capacity=None, guard=0):
        """hop_slice_data_write: the slice data of the context's picture(s) -- parts as encode_frame returned them, levels (n_ctu, 6144) int32 or None = the levels resident
        after encode_frame, sao_coded (n_ctu, 3) as sao_frame returned them or None (no SAO syntax; the flags default to whether it is given).  Returns (the substreams back to
        back as bytes, their sizes: uint32, n_substreams per picture each).  capacity: size of the output buffer (default: ample); guard: bytes behind it that must come back
        untouched (asserted).  An output that does not fit raises HopError with .needed = the bytes it takes."""
        parts = np.ascontiguousarray(parts, CU_PART_DTYPE)
        n = self._n_ctu()
        assert parts.size == n * 256
        if levels is not None:
            levels = np.ascontiguousarray(levels, np.int32); assert levels.size == n * 6144
        if sao_coded is not None:
            sao_coded = np.ascontiguousarray(sao_coded, SAO_PARAM_DTYPE); assert sao_coded.size == n * 3
        on = 0 if sao_coded is None else 1
        p = SliceDataParams(qp, slice_type, wpp, plain_intra, on if sao_luma is None else sao_luma, on if sao_chroma is None else sao_chroma, mi_size)
        cap = n * 16384 if capacity is None else capacity
        buf = np.full(cap + guard, 0xA5, np.uint8)
        sizes = np.zeros(self.pictures * ((self.sub_h + 63) // 64), np.uint32)
        nsub = ctypes.c_int32(0)
        self.L.hop_slice_data_write.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
        r = self.L.hop_slice_data_write(self.h, ctypes.byref(p), parts.ctypes.data, None if levels is None else levels.ctypes.data, None if sao_coded is None else sao_coded.ctypes.data,
                                        buf.ctypes.data, cap, sizes.ctypes.data, ctypes.byref(nsub))
        assert np.all(buf[cap:] == 0xA5), "hop_slice_data_write stored past out_capacity"
        if r != 0:
            e = HopError("hop_slice_data_write: %d %s" % (r, self.L.hop_last_error(self.h).decode()))
            e.code = r; e.needed = nsub.value
            raise e
        sizes = sizes[:self.pictures * nsub.value]
        return buf[:int(sizes.sum())].tobytes(), sizes, nsub.value

    def access_unit_write(self, parts, levels=None, sao_coded=None, qp=32, slice_type=3, wpp=0, plain_intra=0, sao_luma=None, sao_chroma=None, mi_size=16, poc=0,
                          parameter_sets=1, hash=1, capacity=None, guard=0):
        """hop_access_unit_write: the Annex B bytes of one access unit per picture of the context -- parts, levels (None = resident) and sao_coded as slice_data_write;
        poc 0: the IDR picture; parameter_sets 1: VPS, SPS, PPS in front; hash: 0 none, 1 MD5, 3 checksum of the resident reconstruction in a suffix SEI.  Returns (bytes,
        sizes per picture).  capacity / guard as slice_data_write; an output that does not fit raises HopError with .needed = the bytes it takes."""
        parts = np.ascontiguousarray(parts, CU_PART_DTYPE)
        n = self._n_ctu()
        assert parts.size == n * 256
        if levels is not None:
            levels = np.ascontiguousarray(levels, np.int32); assert levels.size == n * 6144
        if sao_coded is not None:
            sao_coded = np.ascontiguousarray(sao_coded, SAO_PARAM_DTYPE); assert sao_coded.size == n * 3
        on = 0 if sao_coded is None else 1
        p = StreamParams(SliceDataParams(qp, slice_type, wpp, plain_intra, on if sao_luma is None else sao_luma, on if sao_chroma is None else sao_chroma, mi_size),
                         poc, parameter_sets, hash)
        cap = n * 16384 + 1024 * self.pictures if capacity is None else capacity
        buf = np.full(cap + guard, 0xA5, np.uint8)
        sizes = (ctypes.c_size_t * self.pictures)()
        self.L.hop_access_unit_write.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]
        r = self.L.hop_access_unit_write(self.h, ctypes.byref(p), parts.ctypes.data, None if levels is None else levels.ctypes.data,
                                         None if sao_coded is None else sao_coded.ctypes.data, buf.ctypes.data, cap, sizes)
        assert np.all(buf[cap:] == 0xA5), "hop_access_unit_write stored past out_capacity"
        if r != 0:
            e = HopError("hop_access_unit_write: %d %s" % (r, self.L.hop_last_error(self.h).decode()))
            e.code = r; e.needed = int(sizes[0])
            raise e
        sizes = np.array(list(sizes), np.uint64)
        return buf[:int(sizes.sum())].tobytes(), sizes

    def rbsp_escape(self, data, segments=None, capacity=None, guard=0, want_counts=True):
        """hop_rbsp_escape: emulation prevention over the concatenation of the segments (byte lengths; default: one) of data, on the device.  Returns (bytes, per-segment
        counts of the segments alone or None).  An output that does not fit raises HopError with .needed."""
        return _rbsp_escape(self.L, self.L.hop_rbsp_escape, self.h, data, segments, capacity, guard, want_counts)

    def rbsp_unescape(self, data, segments=None, lookback=0, capacity=None, guard=0):
        """hop_rbsp_unescape: emulation prevention removed on the device -- data: `lookback` bytes only the predicate sees, then the segments (escaped byte lengths; default:
        one).  Returns (RBSP bytes, per segment its RBSP bytes, violations).  An output that does not fit raises HopError with .needed."""
        return _rbsp_unescape(self.L, self.L.hop_rbsp_unescape, self.h, data, segments, lookback, capacity, guard)

    def access_unit_read(self, au, active=None, max_substreams=None, capacity=None):
        """hop_access_unit_read: one access unit's Annex B bytes -> (StreamInfo, the slice data's RBSP as slice_data_parse takes it, the substreams' sizes, the SEI's digests
        (3, 16) uint8); active: the StreamInfo of an earlier access unit of the sequence.  HopError with .code (and .needed when the RBSP does not fit capacity)."""
        return _access_unit_read(self.L, self.L.hop_access_unit_read, self.h, au, active, max_substreams, capacity)

    def access_unit_decode(self, au, active=None, want_outputs=True):
        """hop_access_unit_decode: one access unit's bytes to the picture resident in the context (recon_download).  Returns (StreamInfo, hash_match [3]: 1 equal, 0
        different, -1 not checked, parts, levels, coded SAO parameters or None); want_outputs False: the three are not asked for (None)."""
        au = np.frombuffer(bytes(au), np.uint8).copy() if len(au) else np.zeros(1, np.uint8)
        n = self._n_ctu()
        info = StreamInfo(); match = (ctypes.c_int32 * 3)(-2, -2, -2)
        out = [np.full(nb + PARSE_GUARD, 0xA5, np.uint8) if want_outputs else None for nb in (n * 256 * CU_PART_DTYPE.itemsize, n * 6144 * 4, n * 3 * SAO_PARAM_DTYPE.itemsize)]
        self.L.hop_access_unit_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 6
        r = self.L.hop_access_unit_decode(self.h, au.ctypes.data, len(au), None if active is None else ctypes.byref(active), ctypes.byref(info), match,
                                          *[None if b is None else b.ctypes.data for b in out])
        for b in out:
            assert b is None or np.all(b[-PARSE_GUARD:] == 0xA5), "hop_access_unit_decode stored past an output"
        if r != 0:
            e = HopError("hop_access_unit_decode: %d %s" % (r, self.L.hop_last_error(self.h).decode()))
            e.code = r
            raise e
        if not want_outputs:
            return info, list(match), None, None, None
        parts, levels, sao = _parse_out(n, out, "hop_access_unit_decode")
        if not (info.params.slice.sao_luma or info.params.slice.sao_chroma):
            sao = None
        return info, list(match), parts, levels, sao

    def picture_hash(self, method):
        """hop_picture_hash: the decoded-picture hash of the resident reconstruction, (pictures, 3, 16) uint8 -- method 1 MD5, 3 checksum (4 bytes, then zeros)"""
        d = np.zeros((self.pictures, 3, 16), np.uint8)
        self.L.hop_picture_hash.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        self._chk(self.L.hop_picture_hash(self.h, method, d.ctypes.data), "hop_picture_hash")
        return d

    def slice_data_parse(self, data, sizes, n_substreams=None, qp=32, slice_type=3, wpp=0, plain_intra=0, sao_luma=1, sao_chroma=1, mi_size=16, want_levels=True):
        """hop_slice_data_parse: data (bytes) and sizes (uint32) as slice_data_write returned them -> (parts (n_ctu, 256) CU_PART_DTYPE, levels (n_ctu, 6144) int32 or None,
        sao_coded (n_ctu, 3) or None when both SAO flags are 0).  n_substreams: per picture (default: the CTU rows with wpp, 1 without).  The outputs have guard bytes
        behind them that must come back untouched (asserted).  An error raises HopError with .code; .outputs holds what was parsed."""
        n = self._n_ctu()
        sao_on = bool(sao_luma or sao_chroma)
        data, sizes, out = _parse_io(n, data, sizes, want_levels, sao_on)
        if n_substreams is None:
            n_substreams = (self.sub_h + 63) // 64 if wpp else 1
        p = SliceDataParams(qp, slice_type, wpp, plain_intra, sao_luma, sao_chroma, mi_size)
        self.L.hop_slice_data_parse.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int32] + [ctypes.c_void_p] * 3
        r = self.L.hop_slice_data_parse(self.h, ctypes.byref(p), data.ctypes.data, sizes.ctypes.data, n_substreams, *[None if b is None else b.ctypes.data for b in out])
        res = _parse_out(n, out, "hop_slice_data_parse")
        if r != 0:
            e = HopError("hop_slice_data_parse: %d %s" % (r, self.L.hop_last_error(self.h).decode()))
            e.code = r; e.outputs = res
            raise e
        return res

    def profile(self, on=None, reset=False, read=None):
        """hop_profile_enable / hop_profile_reset / hop_profile_read: on: switch the HIP events around the launches on or off; reset: clear the sums; read: a HOP_K_* id ->
        (launches, total ms, units) since the last reset"""
        if on is not None: self._chk(self.L.hop_profile_enable(self.h, 1 if on else 0), "hop_profile_enable")
        if reset: self._chk(self.L.hop_profile_reset(self.h), "hop_profile_reset")
        if read is None: return None
        la, ms, un = ctypes.c_uint64(0), ctypes.c_double(0), ctypes.c_uint64(0)
        self._chk(self.L.hop_profile_read(self.h, read, ctypes.byref(la), ctypes.byref(ms), ctypes.byref(un)), "hop_profile_read")
        return int(la.value), float(ms.value), int(un.value)

    def walk_stamps(self, kernel, log2_cu, nxn=0):
        """hop_walk_stamps_read (the stamps library only; the product raises with code HOP_ERR_STATE): one row of the stage table since the last reset -> (cycles
        (HOP_WS_COUNT,) uint64, visits (HOP_WS_COUNT,) uint64, {workgroups, cycles, realtime_ticks, max_realtime_ticks})"""
        cyc = np.zeros(HOP_WS_COUNT, np.uint64); vis = np.zeros(HOP_WS_COUNT, np.uint64); tot = WalkStampsTotal()
        self.L.hop_walk_stamps_read.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_walk_stamps_read(self.h, kernel, log2_cu, nxn, cyc.ctypes.data, vis.ctypes.data, ctypes.byref(tot)), "hop_walk_stamps_read")
        return cyc, vis, {n: int(getattr(tot, n)) for n, _ in WalkStampsTotal._fields_}

    def walk_stamps_reset(self):
        """hop_walk_stamps_reset: the whole table to zero"""
        self.L.hop_walk_stamps_reset.argtypes = [ctypes.c_void_p]
        self._chk(self.L.hop_walk_stamps_reset(self.h), "hop_walk_stamps_reset")

    def walk_stamps_probe(self):
        """hop_walk_stamps_probe -> {stamp_cycles: two stamps back to back, mark_cycles: what a stage boundary charges when the next follows at once, clock_mhz: the
        shader clock the stamps count, from the probe's span on both counters}"""
        out = np.zeros(4, np.uint64)
        self.L.hop_walk_stamps_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_walk_stamps_probe(self.h, out.ctypes.data), "hop_walk_stamps_probe")
        return {"stamp_cycles": int(out[0]), "mark_cycles": int(out[1]), "span_cycles": int(out[2]), "span_realtime_ticks": int(out[3]),
                "clock_mhz": float(out[2]) / max(1.0, float(out[3])) * 100.0}

    def sao_reconstruct_params(self, coded, bit_depth=None):
        """hop_sao_reconstruct_params for this context's picture: coded (n_ctu, 3) SAO_PARAM_DTYPE -> what sao_apply takes"""
        return sao_reconstruct_params(coded, (self.W + 63) // 64, bit_depth or self.bit_depth)

    def psnr(self):
        """hop_psnr: (ssd (pictures, 3) uint64, psnr (pictures, 3) float64) between the resident original and the reconstruction"""
        ssd = np.zeros((self.pictures, 3), np.uint64); ps = np.zeros((self.pictures, 3), np.float64)
        self.L.hop_psnr.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_psnr(self.h, ssd.ctypes.data, ps.ctypes.data), "hop_psnr")
        return ssd, ps

    def rd_fraction_download(self):
        """hop_rd_fraction_download: per CTU the fraction of a bit the RD search's counting coder carries when the CTU is done"""
        n = ((self.W + 63) // 64) * ((self.sub_h + 63) // 64) * self.pictures
        a = np.zeros(n, np.uint16)
        self.L.hop_rd_fraction_download.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_rd_fraction_download(self.h, a.ctypes.data), "hop_rd_fraction_download")
        return a

    def encode_stats(self):
        ms, calls = (ctypes.c_double * 16)(), (ctypes.c_double * 16)()
        self.L.hop_encode_stats(ms, calls)
        names = ("me_search", "pred_inter", "distortion", "valid_pattern", "inter_cu", "inter_cu_skip", "intra_cu", "recon_stash", "commit", "evaluation_wait")
        d = {k: {"ms": ms[i], "calls": int(calls[i])} for i, k in enumerate(names)}
        d["evaluation_handover"] = {"ms": ms[15], "calls": int(calls[13])}   # evaluation groups that waited for an earlier chain's end before they could be issued
        d["rendezvous"] = {"rounds": int(calls[14]), "requests": int(calls[15]), "serve_ms": float(ms[14]), "run_ms": float(ms[13]),
                           "searches_reaching_below": int(calls[10]), "first_ctu_reaching_below": int(ms[10]), "searches_reaching_above": int(calls[11]), "first_ctu_reaching_above": int(ms[11]),
                           "waits": int(calls[12]), "wait_ms": float(ms[12])}
        return d

    def tu_roundtrip(self, jobs, want_levels=True):
        n = len(jobs)
        arr = (TuJob * n)(*jobs)
        res = (TuResult * n)()
        tot = sum((1 << j.log2_size) ** 2 for j in jobs)
        lv = np.zeros(tot, np.int32) if want_levels else None
        self._chk(self.L.hop_tu_roundtrip(self.h, n, ctypes.addressof(arr), ctypes.addressof(res), lv.ctypes.data if want_levels else None), "hop_tu_roundtrip")
        return [(r.abs_sum, r.sse) for r in res], lv

    def intra_rough(self, jobs):
        n = len(jobs)
        arr = (IntraJob * n)(*jobs)
        out = np.zeros((n, 35), np.uint32)
        self._chk(self.L.hop_intra_rough(self.h, n, ctypes.addressof(arr), out.ctypes.data), "hop_intra_rough")
        return out

    def rdoq(self, jobs, tables, src):
        """jobs: RDOQ_JOB_DTYPE array; tables: (n_tables, ESTBITS_INTS) int32; src: all coefficients (int32) -> levels, abs_sum"""
        jobs = np.ascontiguousarray(jobs, RDOQ_JOB_DTYPE); tables = np.ascontiguousarray(tables, np.int32); src = np.ascontiguousarray(src, np.int32)
        assert tables.ndim == 2 and tables.shape[1] == ESTBITS_INTS
        dst = np.zeros(len(src), np.int32); asum = np.zeros(len(jobs), np.uint32)
        self._chk(self.L.hop_rdoq(self.h, len(jobs), jobs.ctypes.data, len(tables), tables.ctypes.data, len(src), src.ctypes.data, dst.ctypes.data,
                                  asum.ctypes.data), "hop_rdoq")
        return dst, asum

    def coeff_bits(self, jobs, ctx_in, coef, want_ctx=True):
        """jobs: COEFF_BITS_JOB_DTYPE; ctx_in: (n_ctx, 152) uint8 snapshots; coef: all levels (int32) -> bits (uint64, Q15), ctx after each TU"""
        jobs = np.ascontiguousarray(jobs, COEFF_BITS_JOB_DTYPE); ctx_in = np.ascontiguousarray(ctx_in, np.uint8); coef = np.ascontiguousarray(coef, np.int32)
        assert ctx_in.ndim == 2 and ctx_in.shape[1] == CABAC_CTX_BYTES
        bits = np.zeros(len(jobs), np.uint64); out = np.zeros((len(jobs), CABAC_CTX_BYTES), np.uint8) if want_ctx else None
        self._chk(self.L.hop_coeff_bits(self.h, len(jobs), jobs.ctypes.data, len(ctx_in), ctx_in.ctypes.data, len(coef), coef.ctypes.data, bits.ctypes.data,
                                        out.ctypes.data if want_ctx else None), "hop_coeff_bits")
        return bits, out

    def tu_rd(self, jobs, ctx_in):
        """jobs: TU_RD_JOB_DTYPE; ctx_in: (n_ctx, 152) uint8 -> results (TU_RD_RESULT_DTYPE), levels (all TUs, job order)"""
        jobs = np.ascontiguousarray(jobs, TU_RD_JOB_DTYPE); ctx_in = np.ascontiguousarray(ctx_in, np.uint8)
        res = np.zeros(len(jobs), TU_RD_RESULT_DTYPE); lv = np.zeros(int(np.sum(1 << (2 * jobs["log2_size"].astype(np.int64)))), np.int32)
        self._chk(self.L.hop_tu_rd(self.h, len(jobs), jobs.ctypes.data, len(ctx_in), ctx_in.ctypes.data, res.ctypes.data, lv.ctypes.data), "hop_tu_rd")
        return res, lv

    def rqt(self, jobs, ctx_in):
        """jobs: RQT_JOB_DTYPE; ctx_in: (n_ctx, 152) uint8 -> results (RQT_RESULT_DTYPE), chosen levels (1.5 * size^2 per CU, job order), coder states out"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); ctx_in = np.ascontiguousarray(ctx_in, np.uint8)
        res = np.zeros(len(jobs), RQT_RESULT_DTYPE); co = np.zeros(int(np.sum(3 << (2 * jobs["log2_cu"].astype(np.int64) - 1))), np.int32)
        cx = np.zeros((len(jobs), CABAC_CTX_BYTES), np.uint8)
        self.L.hop_rqt.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
        self._chk(self.L.hop_rqt(self.h, len(jobs), jobs.ctypes.data, len(ctx_in), ctx_in.ctypes.data, res.ctypes.data, co.ctypes.data, cx.ctypes.data), "hop_rqt")
        return res, co, cx

    def rqt_finish(self, jobs, res, coef, ctx_after):
        """the tail of encodeResAndCalcRdInterCU on the outputs of rqt(): returns (results, levels) updated in place where the zero residual
        wins, and per CU (root_cbf, dist Y, Cb, Cr); the reconstruction is in the context's reconstruction picture"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); res = np.ascontiguousarray(res, RQT_RESULT_DTYPE).copy(); coef = np.ascontiguousarray(coef, np.int32).copy()
        cx = np.ascontiguousarray(ctx_after, np.uint8); fin = np.zeros((len(jobs), 4), np.uint32)
        self.L.hop_rqt_finish.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
        self._chk(self.L.hop_rqt_finish(self.h, len(jobs), jobs.ctypes.data, res.ctypes.data, coef.ctypes.data, cx.ctypes.data, fin.ctypes.data), "hop_rqt_finish")
        return res, coef, fin

    def inter_cu_bits(self, jobs, syntax, res, coef, ctx_in, cu_ctx_in):
        """CU-level syntax bits (xAddSymbolBitsInter): returns bits, skipped, coder states (n, 152) and CU-level states (n, 20) afterwards"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); syntax = np.ascontiguousarray(syntax, CU_SYNTAX_DTYPE); res = np.ascontiguousarray(res, RQT_RESULT_DTYPE)
        coef = np.ascontiguousarray(coef, np.int32); ctx_in = np.ascontiguousarray(ctx_in, np.uint8); cu_ctx_in = np.ascontiguousarray(cu_ctx_in, np.uint8)
        n = len(jobs); bits = np.zeros(n, np.uint32); sk = np.zeros(n, np.uint32); cx = np.zeros((n, CABAC_CTX_BYTES), np.uint8); cu = np.zeros((n, CABAC_CU_CTX_BYTES), np.uint8)
        self.L.hop_inter_cu_bits.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 6
        self._chk(self.L.hop_inter_cu_bits(self.h, n, jobs.ctypes.data, syntax.ctypes.data, res.ctypes.data, coef.ctypes.data, len(ctx_in), ctx_in.ctypes.data, cu_ctx_in.ctypes.data,
                                           bits.ctypes.data, sk.ctypes.data, cx.ctypes.data, cu.ctypes.data), "hop_inter_cu_bits")
        return bits, sk, cx, cu

    def intra_modes(self, jobs, satd):
        jobs = np.ascontiguousarray(jobs, INTRA_MODES_JOB_DTYPE); satd = np.ascontiguousarray(satd, np.uint32); res = np.zeros(len(jobs), INTRA_MODES_RESULT_DTYPE)
        self.L.hop_intra_modes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_intra_modes(self.h, len(jobs), jobs.ctypes.data, satd.ctypes.data, res.ctypes.data), "hop_intra_modes")
        return res

    def intra_cu_bits(self, jobs, syntax, res, coef, ctx_in, cu_ctx_in):
        """xGetIntraBitsQT: returns bits, coder states (n, 152) and CU-level states (n, 20) afterwards"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); syntax = np.ascontiguousarray(syntax, INTRA_CU_SYNTAX_DTYPE); res = np.ascontiguousarray(res, RQT_RESULT_DTYPE)
        coef = np.ascontiguousarray(coef, np.int32); ctx_in = np.ascontiguousarray(ctx_in, np.uint8); cu_ctx_in = np.ascontiguousarray(cu_ctx_in, np.uint8)
        n = len(jobs); bits = np.zeros(n, np.uint32); cx = np.zeros((n, CABAC_CTX_BYTES), np.uint8); cu = np.zeros((n, CABAC_CU_CTX_BYTES), np.uint8)
        self.L.hop_intra_cu_bits.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 5
        self._chk(self.L.hop_intra_cu_bits(self.h, n, jobs.ctypes.data, syntax.ctypes.data, res.ctypes.data, coef.ctypes.data, len(ctx_in), ctx_in.ctypes.data, cu_ctx_in.ctypes.data,
                                           bits.ctypes.data, cx.ctypes.data, cu.ctypes.data), "hop_intra_cu_bits")
        return bits, cx, cu

    def intra_rqt(self, jobs, syntax, opts, ctx_in, cu_ctx_in):
        """xRecurIntraCodingQT (luma): returns results (RQT_RESULT_DTYPE), chosen levels (1.5 size^2 per job, the PU's luma partitions filled), coder states (n, 152)
        and CU-level states (n, 20) afterwards; the context's reconstruction picture holds the chosen trees"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); syntax = np.ascontiguousarray(syntax, INTRA_CU_SYNTAX_DTYPE); opts = np.ascontiguousarray(opts, INTRA_RQT_OPT_DTYPE)
        ctx_in = np.ascontiguousarray(ctx_in, np.uint8); cu_ctx_in = np.ascontiguousarray(cu_ctx_in, np.uint8)
        n = len(jobs); res = np.zeros(n, RQT_RESULT_DTYPE); cx = np.zeros((n, CABAC_CTX_BYTES), np.uint8); cu = np.zeros((n, CABAC_CU_CTX_BYTES), np.uint8)
        coef = np.zeros(int(sum((3 << (2 * int(j["log2_cu"]))) // 2 for j in jobs)), np.int32)
        self.L.hop_intra_rqt.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 6
        self._chk(self.L.hop_intra_rqt(self.h, n, jobs.ctypes.data, syntax.ctypes.data, opts.ctypes.data, len(ctx_in), ctx_in.ctypes.data, cu_ctx_in.ctypes.data, res.ctypes.data,
                                       coef.ctypes.data, cx.ctypes.data, cu.ctypes.data), "hop_intra_rqt")
        return res, coef, cx, cu

    def intra_luma_search(self, jobs, syntax, opts, sjobs, ctx_in, cu_ctx_in):
        """estIntraPredQT (luma): returns search results (INTRA_SEARCH_RESULT_DTYPE), arrays (RQT_RESULT_DTYPE), levels (1.5 size^2 per job, luma filled) and the CUs'
        luma reconstruction planes (size^2 per job); the context's reconstruction picture is updated as the reference updates it"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); syntax = np.ascontiguousarray(syntax, INTRA_CU_SYNTAX_DTYPE); opts = np.ascontiguousarray(opts, INTRA_RQT_OPT_DTYPE)
        sjobs = np.ascontiguousarray(sjobs, INTRA_SEARCH_JOB_DTYPE); ctx_in = np.ascontiguousarray(ctx_in, np.uint8); cu_ctx_in = np.ascontiguousarray(cu_ctx_in, np.uint8)
        n = len(jobs); sres = np.zeros(n, INTRA_SEARCH_RESULT_DTYPE); res = np.zeros(n, RQT_RESULT_DTYPE)
        coef = np.zeros(int(sum((3 << (2 * int(j["log2_cu"]))) // 2 for j in jobs)), np.int32); reco = np.zeros(int(sum(1 << (2 * int(j["log2_cu"])) for j in jobs)), np.int16)
        self.L.hop_intra_luma_search.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 6
        self._chk(self.L.hop_intra_luma_search(self.h, n, jobs.ctypes.data, syntax.ctypes.data, opts.ctypes.data, sjobs.ctypes.data, len(ctx_in), ctx_in.ctypes.data,
                                               cu_ctx_in.ctypes.data, sres.ctypes.data, res.ctypes.data, coef.ctypes.data, reco.ctypes.data), "hop_intra_luma_search")
        return sres, res, coef, reco

    def intra_chroma_search(self, jobs, syntax, opts, res, ctx_in, cu_ctx_in):
        """estIntraPredChromaQT: res holds tr_idx / tskip[0] of the luma search; returns (mode, dist) pairs, the arrays incl. cbf[1..2] / tskip[1..2], levels (1.5 size^2 per
        job, the chroma parts filled) and the chroma reconstruction planes (size^2 / 2 per job: Cb, Cr)"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); syntax = np.ascontiguousarray(syntax, INTRA_CU_SYNTAX_DTYPE); opts = np.ascontiguousarray(opts, INTRA_RQT_OPT_DTYPE)
        res = np.ascontiguousarray(res, RQT_RESULT_DTYPE).copy(); ctx_in = np.ascontiguousarray(ctx_in, np.uint8); cu_ctx_in = np.ascontiguousarray(cu_ctx_in, np.uint8)
        n = len(jobs); cres = np.zeros(n, np.dtype([("best_mode", "<i4"), ("dist", "<u4")]))
        coef = np.zeros(int(sum((3 << (2 * int(j["log2_cu"]))) // 2 for j in jobs)), np.int32); reco = np.zeros(int(sum((1 << (2 * int(j["log2_cu"]))) // 2 for j in jobs)), np.int16)
        self.L.hop_intra_chroma_search.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 6
        self._chk(self.L.hop_intra_chroma_search(self.h, n, jobs.ctypes.data, syntax.ctypes.data, opts.ctypes.data, len(ctx_in), ctx_in.ctypes.data, cu_ctx_in.ctypes.data,
                                                 res.ctypes.data, cres.ctypes.data, coef.ctypes.data, reco.ctypes.data), "hop_intra_chroma_search")
        return cres, res, coef, reco

    def intra_cu_total_bits(self, jobs, syntax, res, coef, dist, ctx_in, cu_ctx_in):
        """the counting part of xCheckRDCostIntra: returns bits, costs, coder states (n, 152) and CU-level states (n, 20) afterwards"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); syntax = np.ascontiguousarray(syntax, INTRA_CU_SYNTAX_DTYPE); res = np.ascontiguousarray(res, RQT_RESULT_DTYPE)
        coef = np.ascontiguousarray(coef, np.int32); dist = np.ascontiguousarray(dist, np.uint32); ctx_in = np.ascontiguousarray(ctx_in, np.uint8); cu_ctx_in = np.ascontiguousarray(cu_ctx_in, np.uint8)
        n = len(jobs); bits = np.zeros(n, np.uint32); cost = np.zeros(n, np.float64); cx = np.zeros((n, CABAC_CTX_BYTES), np.uint8); cu = np.zeros((n, CABAC_CU_CTX_BYTES), np.uint8)
        self.L.hop_intra_cu_total_bits.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] + [ctypes.c_void_p] * 6
        self._chk(self.L.hop_intra_cu_total_bits(self.h, n, jobs.ctypes.data, syntax.ctypes.data, res.ctypes.data, coef.ctypes.data, dist.ctypes.data, len(ctx_in), ctx_in.ctypes.data,
                                                 cu_ctx_in.ctypes.data, bits.ctypes.data, cost.ctypes.data, cx.ctypes.data, cu.ctypes.data), "hop_intra_cu_total_bits")
        return bits, cost, cx, cu

    def inter_cu_skip(self, jobs, syntax, ctx_in, cu_ctx_in):
        """encodeResAndCalcRdInterCU without residual: returns (n, 4) root_cbf | dist Y, Cb, Cr, bits, costs, coder states (n, 152), CU-level states (n, 20)"""
        jobs = np.ascontiguousarray(jobs, RQT_JOB_DTYPE); syntax = np.ascontiguousarray(syntax, CU_SYNTAX_DTYPE); ctx_in = np.ascontiguousarray(ctx_in, np.uint8); cu_ctx_in = np.ascontiguousarray(cu_ctx_in, np.uint8)
        n = len(jobs); fin = np.zeros((n, 4), np.uint32); bits = np.zeros(n, np.uint32); cost = np.zeros(n, np.float64)
        cx = np.zeros((n, CABAC_CTX_BYTES), np.uint8); cu = np.zeros((n, CABAC_CU_CTX_BYTES), np.uint8)
        self.L.hop_inter_cu_skip.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 7
        self._chk(self.L.hop_inter_cu_skip(self.h, n, jobs.ctypes.data, syntax.ctypes.data, len(ctx_in), ctx_in.ctypes.data, cu_ctx_in.ctypes.data, fin.ctypes.data, bits.ctypes.data,
                                           cost.ctypes.data, cx.ctypes.data, cu.ctypes.data), "hop_inter_cu_skip")
        return fin, bits, cost, cx, cu

    def intra_pred(self, jobs, modes):
        n = len(jobs)
        arr = (IntraJob * n)(*jobs); m = np.ascontiguousarray(modes, np.int32)
        self._chk(self.L.hop_intra_pred(self.h, n, ctypes.addressof(arr), m.ctypes.data), "hop_intra_pred")

    def intra_pred_chroma(self, jobs, modes):
        n = len(jobs)
        arr = (IntraJob * n)(*jobs); m = np.ascontiguousarray(modes, np.int32)
        self.L.hop_intra_pred_chroma.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_intra_pred_chroma(self.h, n, ctypes.addressof(arr), m.ctypes.data), "hop_intra_pred_chroma")

    def sync(self):
        self._chk(self.L.hop_sync(self.h), "hop_sync")

    # ---- the spine's byte-moving entries (csrc/k_spine.hip), as hop_encode_frame's backend calls them ----
    def valid_pattern(self, queries):
        """hop_valid_pattern: queries (n, 6) int32 -- x, y, w, h, mv_x, mv_y (quarter samples) -> (n,) uint8, 1 where both probes of isValidPattern hit committed samples"""
        q = np.ascontiguousarray(queries, np.int32).reshape(-1, 6)
        out = np.zeros(len(q), np.uint8)
        self.L.hop_valid_pattern.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self.L.hop_valid_pattern(self.h, len(q), q.ctypes.data, out.ctypes.data), "hop_valid_pattern")
        return out

    def recon_stash(self, rects, restore=False):
        """hop_recon_stash: rects (n, 4) int32 -- x, y (+ k * pic_h: copy k of the candidate slots), size, stash slot; the blocks of the reconstruction picture (and of
        the levels, once hop_encode_frame has run) put aside, or with restore brought back"""
        r = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
        self.L.hop_recon_stash.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        self._chk(self.L.hop_recon_stash(self.h, len(r), r.ctypes.data, 1 if restore else 0), "hop_recon_stash")

    def ssref_commit_recon(self, rects):
        """hop_ssref_commit_recon: rects (n, 3) -- x, y, size: the blocks of the resident reconstruction picture committed to the SS reference"""
        r4 = np.zeros((len(rects), 4), np.int32)
        r4[:, :3] = np.asarray(rects, np.int32).reshape(-1, 3)
        self.L.hop_ssref_commit_recon.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        self._chk(self.L.hop_ssref_commit_recon(self.h, len(r4), r4.ctypes.data), "hop_ssref_commit_recon")

    def recon_put_device(self, n, d_jobs, d_reco_y, d_reco_c):
        """hop_recon_put_device: n CUs of ONE size (RQT_JOB_DTYPE: x, y, log2_cu) from packed planes into the reconstruction picture; the arguments are device
        addresses, the copy is enqueued on the context's stream"""
        self.L.hop_recon_put_device.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
        self._chk(self.L.hop_recon_put_device(self.h, n, d_jobs, d_reco_y, d_reco_c), "hop_recon_put_device")

    def coef_put_device(self, n, d_jobs, d_coef):
        """hop_coef_put_device: the levels of the same CUs (1.5 size^2 per CU; d_coef None: CUs without residual) into the image of the levels, which exists once
        hop_encode_frame has run on the context"""
        self.L.hop_coef_put_device.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 2
        self._chk(self.L.hop_coef_put_device(self.h, n, d_jobs, d_coef), "hop_coef_put_device")


def decode_schedule(W, H, parts, schedule=0, lib=None):
    """hop_decode_schedule: (level of every CTU (n_ctu,) int32, number of levels) -- the launches hop_decode_frame makes; HopError for refused parts"""
    L = lib or load()
    parts = np.ascontiguousarray(parts, CU_PART_DTYPE)
    n = ((W + 63) // 64) * ((H + 63) // 64)
    if parts.size != n * 256:
        raise HopError("decode_schedule: %d CTUs need (%d, 256) parts" % (n, n))
    lv = np.zeros(n, np.int32); nl = ctypes.c_int32(0)
    L.hop_decode_schedule.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    r = L.hop_decode_schedule(W, H, parts.ctypes.data, schedule, lv.ctypes.data, ctypes.byref(nl))
    if r != 0:
        raise HopError("hop_decode_schedule: %d" % r)
    return lv, int(nl.value)


def decode_stack_schedule(W, sub_h, pictures, parts, schedule=0, lib=None):
    """hop_decode_stack_schedule: (level of every CTU (pictures, n_ctu) int32, number of levels) -- the launches hop_decode_stack makes for a stack of `pictures`
    pictures of W x sub_h; HopError, naming the picture, for refused parts"""
    L = lib or load()
    parts = np.ascontiguousarray(parts, CU_PART_DTYPE)
    n = ((W + 63) // 64) * ((sub_h + 63) // 64)
    if pictures < 1 or parts.size != pictures * n * 256:
        raise HopError("decode_stack_schedule: %d pictures of %d CTUs need (%d, 256) parts" % (pictures, n, pictures * n))
    lv = np.zeros((pictures, n), np.int32); nl = ctypes.c_int32(0)
    L.hop_decode_stack_schedule.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    r = L.hop_decode_stack_schedule(W, sub_h, pictures, parts.ctypes.data, schedule, lv.ctypes.data, ctypes.byref(nl))
    if r != 0:
        raise HopError("hop_decode_stack_schedule: %d %s" % (r, L.hop_last_error(None).decode()))
    return lv, int(nl.value)


def slice_data_write_host(W, H, parts, levels, sao_coded=None, bit_depth=8, qp=32, slice_type=3, wpp=0, plain_intra=0, sao_luma=None, sao_chroma=None, mi_size=16,
                          capacity=None, lib=None):
    """hop_slice_data_write_host: the host build of the slice-data writer (the yardstick of Context.slice_data_write), one picture, no device.  Returns (bytes, sizes, n_substreams);
    HopError (.code, .needed) as the device entry."""
    L = lib or load()
    n = ((W + 63) // 64) * ((H + 63) // 64)
    parts = np.ascontiguousarray(parts, CU_PART_DTYPE); levels = np.ascontiguousarray(levels, np.int32)
    assert parts.size == n * 256 and levels.size == n * 6144
    if sao_coded is not None:
        sao_coded = np.ascontiguousarray(sao_coded, SAO_PARAM_DTYPE); assert sao_coded.size == n * 3
    on = 0 if sao_coded is None else 1
    p = SliceDataParams(qp, slice_type, wpp, plain_intra, on if sao_luma is None else sao_luma, on if sao_chroma is None else sao_chroma, mi_size)
    cap = n * 16384 if capacity is None else capacity
    buf = np.zeros(cap, np.uint8); sizes = np.zeros((H + 63) // 64, np.uint32); nsub = ctypes.c_int32(0)
    L.hop_slice_data_write_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
    r = L.hop_slice_data_write_host(W, H, bit_depth, ctypes.byref(p), parts.ctypes.data, levels.ctypes.data, None if sao_coded is None else sao_coded.ctypes.data, buf.ctypes.data, cap,
                                    sizes.ctypes.data, ctypes.byref(nsub))
    if r != 0:
        e = HopError("hop_slice_data_write_host: %d" % r)
        e.code = r; e.needed = nsub.value
        raise e
    sizes = sizes[:nsub.value]
    return buf[:int(sizes.sum())].tobytes(), sizes, nsub.value


def _rbsp_escape(L, fn, ctx, data, segments, capacity, guard, want_counts):
    data = bytes(data)
    a = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
    seg = np.asarray([len(data)] if segments is None else segments, np.uint32)
    cap = len(data) * 3 // 2 + 2 if capacity is None else capacity
    buf = np.full(cap + guard, 0xA5, np.uint8); n = ctypes.c_size_t(0); cnt = np.zeros(max(1, len(seg)), np.uint32)
    tail = [a.ctypes.data, seg.ctypes.data, len(seg), buf.ctypes.data, cap, ctypes.byref(n), cnt.ctypes.data if want_counts else None]
    fn.argtypes = ([ctypes.c_void_p] if ctx is not None else []) + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    r = fn(*(([ctx] if ctx is not None else []) + tail))
    assert np.all(buf[cap:] == 0xA5), "hop_rbsp_escape stored past out_capacity"
    if r != 0:
        e = HopError("hop_rbsp_escape: %d %s" % (r, L.hop_last_error(ctx).decode() if ctx is not None else ""))
        e.code = r; e.needed = n.value
        raise e
    return buf[:n.value].tobytes(), (cnt[:len(seg)] if want_counts else None)


def rbsp_escape_host(data, segments=None, capacity=None, guard=0, want_counts=True, lib=None):
    """hop_rbsp_escape_host: the sequential rule on the host (the yardstick of Context.rbsp_escape); same results and HopError"""
    L = lib or load()
    return _rbsp_escape(L, L.hop_rbsp_escape_host, None, data, segments, capacity, guard, want_counts)


def _rbsp_unescape(L, fn, ctx, data, segments, lookback, capacity, guard):
    data = bytes(data)
    a = np.frombuffer(data, np.uint8).copy() if data else np.zeros(1, np.uint8)
    seg = np.asarray([len(data) - lookback] if segments is None else segments, np.uint32)
    assert int(seg.astype(np.uint64).sum()) + lookback == len(data), "lookback and the segment sizes do not add up to the data"
    cap = len(data) if capacity is None else capacity
    buf = np.full(cap + guard, 0xA5, np.uint8); n = ctypes.c_size_t(0); cnt = np.zeros(max(1, len(seg)), np.uint32); viol = ctypes.c_uint32(0)
    tail = [a.ctypes.data, seg.ctypes.data, len(seg), lookback, buf.ctypes.data, cap, ctypes.byref(n), cnt.ctypes.data, ctypes.byref(viol)]
    fn.argtypes = ([ctypes.c_void_p] if ctx is not None else []) + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 3
    r = fn(*(([ctx] if ctx is not None else []) + tail))
    assert np.all(buf[cap:] == 0xA5), "hop_rbsp_unescape stored past out_capacity"
    if r != 0:
        e = HopError("hop_rbsp_unescape: %d %s" % (r, L.hop_last_error(ctx).decode() if ctx is not None else ""))
        e.code = r; e.needed = n.value
        raise e
    return buf[:n.value].tobytes(), cnt[:len(seg)], int(viol.value)


def rbsp_unescape_host(data, segments=None, lookback=0, capacity=None, guard=0, lib=None):
    """hop_rbsp_unescape_host: the sequential rule on the host (the yardstick of Context.rbsp_unescape); same results and HopError"""
    L = lib or load()
    return _rbsp_unescape(L, L.hop_rbsp_unescape_host, None, data, segments, lookback, capacity, guard)


READ_GUARD = 64   # bytes of 0xA5 behind every output of the access-unit readers that must come back untouched


def _access_unit_read(L, fn, ctx, au, active, max_substreams, capacity):
    au = bytes(au)
    a = np.frombuffer(au, np.uint8).copy() if au else np.zeros(1, np.uint8)
    cap = len(au) if capacity is None else capacity
    nmax = 1024 if max_substreams is None else max_substreams
    G = READ_GUARD
    info = np.full(ctypes.sizeof(StreamInfo) + G, 0xA5, np.uint8); data = np.full(cap + G, 0xA5, np.uint8)
    sizes = np.full(4 * max(nmax, 0) + G, 0xA5, np.uint8); digest = np.full(48 + G, 0xA5, np.uint8); n = ctypes.c_size_t(0)
    fn.argtypes = ([ctypes.c_void_p] if ctx is not None else []) + [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2 + [ctypes.c_int32, ctypes.c_void_p]
    r = fn(*(([ctx] if ctx is not None else []) + [a.ctypes.data, len(au), None if active is None else ctypes.byref(active), info.ctypes.data, data.ctypes.data, cap,
                                                    ctypes.byref(n), sizes.ctypes.data, nmax, digest.ctypes.data]))
    for b in (info, data, sizes, digest):
        assert np.all(b[-G:] == 0xA5), "hop_access_unit_read stored past an output"
    if r != 0:
        e = HopError("hop_access_unit_read: %d %s" % (r, L.hop_last_error(ctx).decode() if ctx is not None else ""))
        e.code = r; e.needed = n.value
        raise e
    si = StreamInfo.from_buffer_copy(info[:ctypes.sizeof(StreamInfo)].tobytes())
    return si, data[:n.value].tobytes(), sizes[:4 * si.n_substreams].view(np.uint32).copy(), digest[:48].reshape(3, 16).copy()


def access_unit_read_host(au, active=None, max_substreams=None, capacity=None, lib=None):
    """hop_access_unit_read_host: the host build of the stream reader (the yardstick of Context.access_unit_read), no device; same results and HopError"""
    L = lib or load()
    return _access_unit_read(L, L.hop_access_unit_read_host, None, au, active, max_substreams, capacity)


def annexb_access_units(stream, lib=None):
    """hop_annexb_access_unit, repeated: the access units of an Annex B stream as a list of bytes"""
    L = lib or load()
    stream = bytes(stream)
    a = np.frombuffer(stream, np.uint8).copy() if stream else np.zeros(1, np.uint8)
    L.hop_annexb_access_unit.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    out, at = [], 0
    while at < len(stream):
        n = ctypes.c_size_t(0)
        r = L.hop_annexb_access_unit(a.ctypes.data + at, len(stream) - at, ctypes.byref(n))
        if r != 0 or n.value == 0:
            raise HopError("hop_annexb_access_unit: %d at byte %d" % (r, at))
        out.append(stream[at:at + n.value]); at += n.value
    return out


def parameter_sets_write(W, H, bit_depth=8, qp=32, slice_type=3, wpp=0, plain_intra=0, sao=1, mi_size=16, lib=None):
    """hop_parameter_sets_write: the VPS, SPS and PPS NAL units with their start codes, as bytes"""
    L = lib or load()
    p = StreamParams(SliceDataParams(qp, slice_type, wpp, plain_intra, sao, sao, mi_size), 0, 1, 0)
    buf = np.zeros(256, np.uint8); n = ctypes.c_size_t(0)
    L.hop_parameter_sets_write.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_void_p]
    r = L.hop_parameter_sets_write(W, H, bit_depth, ctypes.byref(p), buf.ctypes.data, buf.size, ctypes.byref(n))
    if r != 0:
        raise HopError("hop_parameter_sets_write: %d" % r)
    return buf[:n.value].tobytes()


def access_unit_write_host(W, H, parts, levels, sao_coded=None, rec=None, bit_depth=8, qp=32, slice_type=3, wpp=0, plain_intra=0, sao_luma=None, sao_chroma=None, mi_size=16,
                           poc=0, parameter_sets=1, hash=1, capacity=None, lib=None):
    """hop_access_unit_write_host: the host build of the outer layer over slice_data_write_host (the yardstick of Context.access_unit_write), one picture, no device; rec: the
    final reconstruction planes [Y, Cb, Cr], None iff hash == 0.  Returns the access unit's bytes; HopError (.code, .needed) as the device entry."""
    L = lib or load()
    n = ((W + 63) // 64) * ((H + 63) // 64)
    parts = np.ascontiguousarray(parts, CU_PART_DTYPE); levels = np.ascontiguousarray(levels, np.int32)
    assert parts.size == n * 256 and levels.size == n * 6144
    if sao_coded is not None:
        sao_coded = np.ascontiguousarray(sao_coded, SAO_PARAM_DTYPE); assert sao_coded.size == n * 3
    on = 0 if sao_coded is None else 1
    p = StreamParams(SliceDataParams(qp, slice_type, wpp, plain_intra, on if sao_luma is None else sao_luma, on if sao_chroma is None else sao_chroma, mi_size),
                     poc, parameter_sets, hash)
    planes = None
    if rec is not None:
        keep = [np.ascontiguousarray(a, np.int16) for a in rec]
        planes = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in keep])
    cap = n * 16384 + 1024 if capacity is None else capacity
    buf = np.zeros(cap, np.uint8); size = ctypes.c_size_t(0)
    L.hop_access_unit_write_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p]
    r = L.hop_access_unit_write_host(W, H, bit_depth, ctypes.byref(p), parts.ctypes.data, levels.ctypes.data, None if sao_coded is None else sao_coded.ctypes.data, planes,
                                     buf.ctypes.data, cap, ctypes.byref(size))
    if r != 0:
        e = HopError("hop_access_unit_write_host: %d" % r)
        e.code = r; e.needed = size.value
        raise e
    return buf[:size.value].tobytes()


def slice_data_parse_host(W, H, data, sizes, n_substreams=None, bit_depth=8, qp=32, slice_type=3, wpp=0, plain_intra=0, sao_luma=1, sao_chroma=1, mi_size=16, want_levels=True,
                          lib=None):
    """hop_slice_data_parse_host: the host build of the slice-data parser (the yardstick of Context.slice_data_parse), one picture, no device.  Returns (parts, levels, sao_coded)
    as the device entry; HopError (.code, .outputs) likewise."""
    L = lib or load()
    n = ((W + 63) // 64) * ((H + 63) // 64)
    data, sizes, out = _parse_io(n, data, sizes, want_levels, bool(sao_luma or sao_chroma))
    if n_substreams is None:
        n_substreams = (H + 63) // 64 if wpp else 1
    p = SliceDataParams(qp, slice_type, wpp, plain_intra, sao_luma, sao_chroma, mi_size)
    L.hop_slice_data_parse_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_int32] + [ctypes.c_void_p] * 3
    r = L.hop_slice_data_parse_host(W, H, bit_depth, ctypes.byref(p), data.ctypes.data, sizes.ctypes.data, n_substreams, *[None if b is None else b.ctypes.data for b in out])
    res = _parse_out(n, out, "hop_slice_data_parse_host")
    if r != 0:
        e = HopError("hop_slice_data_parse_host: %d" % r)
        e.code = r; e.outputs = res
        raise e
    return res


def decode_footprint(W, H, job, lib=None):
    """hop_decode_footprint: the CTUs (ascending raster addresses) whose samples the predictor of one PU (a PredJob) reads"""
    L = lib or load()
    L.hop_decode_footprint.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    out = np.zeros(((W + 63) // 64) * ((H + 63) // 64), np.int32)
    r = L.hop_decode_footprint(W, H, ctypes.byref(job), out.ctypes.data, out.size)
    if r < 0:
        raise HopError("hop_decode_footprint: %d" % r)
    return out[:r]


def sao_reconstruct_params(coded, ctus_per_row, bit_depth, lib=None):
    """hop_sao_reconstruct_params: coded SAO parameters (n_ctu, 3) SAO_PARAM_DTYPE -> the reconstructed ones hop_sao_apply takes"""
    L = lib or load()
    coded = np.ascontiguousarray(coded, SAO_PARAM_DTYPE)
    recon = np.zeros_like(coded)
    L.hop_sao_reconstruct_params.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    r = L.hop_sao_reconstruct_params(coded.size // 3, ctus_per_row, bit_depth, coded.ctypes.data, recon.ctypes.data)
    if r != 0:
        raise HopError("hop_sao_reconstruct_params: %d" % r)
    return recon


def quant_flat_tu_host(coef, bit_depth=8, qp_scaled=32, i_slice=0, sign_hide=1, scan_idx=0, nlanes=256, descending=0, lib=None):
    """hop_quant_flat_tu_host: the leaf step's quantiser for a unit that does not use RDOQ (csrc/k_quant_flat_dev.inl on the host) on one N x N block of coefficients, its
    phases over `nlanes` emulated lanes; returns (levels (N, N) int32, abs_sum)"""
    L = lib or load()
    c = np.ascontiguousarray(coef, np.int32)
    N = c.shape[0]
    assert c.shape == (N, N) and N in (4, 8, 16, 32)
    lev = np.zeros((N, N), np.int32); a = ctypes.c_uint32(0)
    L.hop_quant_flat_tu_host.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    r = L.hop_quant_flat_tu_host(bit_depth, qp_scaled, i_slice, N.bit_length() - 1, sign_hide, scan_idx, c.ctypes.data, lev.ctypes.data, ctypes.byref(a), nlanes, descending)
    if r != 0:
        raise HopError("hop_quant_flat_tu_host: %d" % r)
    return lev, int(a.value)
