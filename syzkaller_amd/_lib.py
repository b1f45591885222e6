"""ctypes binding of libsyzsig.so (include/syzsig.h).

The library is the product: HIP kernels for gfx950 behind a C-ABI.  There is
no CPU fallback -- if the shared object is missing or no MI355X is present,
calls fail loudly (ImportError here, SyzSigError from compute calls).
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SG_LIB_PATH") or os.path.join(_HERE, "libsyzsig.so")  # override: diagnostics builds

SG_OK = 0
SG_EINVAL = -1
SG_EHIP = -2
SG_ENOMEM = -3
SG_ENODEV = -4

TIN_OK = 0  # sg_triage_runs_from_kcov's statuses (include/syzsig.h SG_TIN_*)
TIN_NO_NEW = 1
TIN_NOT_EXECUTED = 2
TIN_FLAKY = 3

MP_OK = 0  # sg_minimize_pred_from_kcov's statuses (include/syzsig.h SG_MP_*)
MP_NOT_EXECUTED = 1
MP_LOST = 2

OP_DIFFERENCE = 0
OP_SYMDIFF = 1
OP_UNION = 2
OP_INTERSECT = 3

P32 = POINTER(c_uint32)
P64 = POINTER(c_uint64)
P8 = POINTER(c_uint8)
PSZ = POINTER(c_size_t)
PINT = POINTER(c_int)
PF = POINTER(c_float)
PI32 = POINTER(c_int32)

# name -> (restype, argtypes); mirrors include/syzsig.h one to one.
SIGNATURES = {
    "sg_version": (c_char_p, []),
    "sg_last_error": (c_char_p, []),
    "sg_ctx_create": (c_int, [c_int, POINTER(c_void_p)]),
    "sg_ctx_destroy": (None, [c_void_p]),
    "sg_ctx_sync": (c_int, [c_void_p]),
    "sg_ctx_set_stream": (c_int, [c_void_p, c_void_p]),
    "sg_ctx_reset_stream": (c_int, [c_void_p]),
    "sg_ctx_stream": (c_void_p, [c_void_p]),
    "sg_ctx_timing": (c_int, [c_void_p, c_int]),
    "sg_ctx_kernel_time": (c_int, [c_void_p, c_char_p, POINTER(c_double), P64]),
    "sg_ctx_counter": (c_int, [c_void_p, c_char_p, P64]),
    "sg_ctx_set_option": (c_int, [c_void_p, c_char_p, c_int64]),
    "sg_ctx_get_option": (c_int, [c_void_p, c_char_p, POINTER(c_int64)]),
    "sg_ctx_marker": (c_int, [c_void_p, c_int, c_uint32]),
    "sg_set_create": (c_int, [c_void_p, POINTER(c_void_p)]),
    "sg_set_destroy": (None, [c_void_p]),
    "sg_set_clear": (c_int, [c_void_p]),
    "sg_set_count": (c_int, [c_void_p, P64]),
    "sg_set_export": (c_int, [c_void_p, P32, c_size_t, PSZ]),
    "sg_set_add": (c_int, [c_void_p, P32, c_size_t]),
    "sg_set_new": (c_int, [c_void_p, P32, c_size_t, PINT]),
    "sg_set_diff": (c_int, [c_void_p, P32, c_size_t, P32, PSZ]),
    "sg_set_device_words": (c_void_p, [c_void_p]),
    "sg_set_wrap_dev": (c_int, [c_void_p, c_void_p, POINTER(c_void_p)]),
    "sg_set_or_dev": (c_int, [c_void_p, c_void_p]),
    "sg_set_copy": (c_int, [c_void_p, c_void_p]),
    "sg_set_or_new_dev": (c_int, [c_void_p, c_void_p, c_void_p]),
    "sg_set_count_missing_dev": (c_int, [c_void_p, c_void_p, c_uint64, P64]),
    "sg_triage_batch": (c_int, [c_void_p, c_void_p, c_void_p, P32, P64, c_size_t, P8, P32, P64, P64]),
    "sg_triage_batch_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64,
                                    c_void_p, c_void_p, c_void_p]),
    "sg_triage_traces": (c_int, [c_void_p, c_void_p, c_void_p, P32, P64, c_size_t, P8]),
    "sg_triage_traces_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p]),
    "sg_shard_of": (c_int, [c_uint32, c_uint32]),
    "sg_shard_candidates_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_uint64,
                                        c_uint32, c_void_p, c_void_p]),
    "sg_shard_owners_dev": (c_int, [c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p]),
    "sg_shard_flags_dev": (c_int, [c_void_p, c_void_p, c_uint32, c_uint64, c_uint64, c_uint64, c_void_p]),
    "sg_set_add_dev": (c_int, [c_void_p, c_void_p, c_uint64]),
    "sg_set_add_new_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64]),
    "sg_set_del_dev": (c_int, [c_void_p, c_void_p, c_uint64]),
    "sg_prefix_cands_dev": (c_int, [c_void_p, c_uint32, c_void_p, c_uint64]),
    "sg_bitmap_prefix_or_dev": (c_int, [c_void_p, c_void_p, c_uint32, c_uint64, c_void_p, c_void_p]),
    "sg_bitmap_prefix_or_rank_dev": (c_int, [c_void_p, c_void_p, c_uint32, c_uint64, c_uint32, c_void_p, c_void_p]),
    "sg_set_or_new_or_dev": (c_int, [c_void_p, c_void_p, c_void_p]),
    "sg_prefix_begin_dev": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64]),
    "sg_prefix_end_dev": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sg_prefix_flags_dev": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]),
    "sg_prefix_begin_form_dev": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64,
                                         c_uint64, c_void_p]),
    "sg_add_inputs": (c_int, [c_void_p, c_void_p, c_void_p, P32, P64, c_size_t]),
    "sg_triage_newsig": (c_int, [c_void_p, c_void_p, P32, P64, c_size_t, P32, P64]),
    "sg_triage_intersect": (c_int, [c_void_p, P32, P64, P32, P64, c_size_t, P64]),
    "sg_triage_subset": (c_int, [c_void_p, P32, P64, P32, P64, c_size_t, P8]),
    "sg_accept_batch": (c_int, [c_void_p, c_void_p, c_void_p, P32, P64, P32, P64, c_size_t, P8]),
    "sg_merge_poll": (c_int, [c_void_p, c_void_p, P32, P64, c_size_t, P32, P64]),
    "sg_minimize": (c_int, [c_void_p, P32, P64, c_size_t, P32, P32, PSZ]),
    "sg_minimize_order": (c_int, [P64, c_size_t, P32]),
    "sg_delta_encode_batch": (c_int, [c_void_p, P32, P64, c_size_t, P8, c_size_t, P64]),
    "sg_delta_decode_batch": (c_int, [c_void_p, P8, P64, c_size_t, P32, c_size_t, P64]),
    "sg_set_encode": (c_int, [c_void_p, P8, c_size_t, PSZ]),
    "sg_set_decode_add": (c_int, [c_void_p, P8, c_size_t, P64]),
    "sg_sancov_batch": (c_int, [c_void_p, P32, P64, c_size_t, P8]),
    "sg_canonicalize": (c_int, [c_void_p, P32, c_size_t, PSZ]),
    "sg_canonicalize_batch": (c_int, [c_void_p, P32, P64, c_size_t, P64]),
    "sg_merge": (c_int, [c_void_p, c_int, P32, c_size_t, P32, c_size_t, P32, PSZ]),
    "sg_merge_batch": (c_int, [c_void_p, c_int, P32, c_size_t, P64, P64, P32, c_size_t, P64, P64, c_size_t, P32,
                               c_size_t, P64, P64]),
    "sg_union_fold": (c_int, [c_void_p, P32, P64, c_size_t, P32, c_size_t, P32, c_size_t, P64]),
    "sg_has_difference": (c_int, [c_void_p, P32, c_size_t, P32, c_size_t, PINT]),
    "sg_has_difference_batch": (c_int, [c_void_p, P32, c_size_t, P64, P64, P32, c_size_t, P64, P64, c_size_t,
                                        c_void_p]),
    "sg_exec_signal": (c_int, [c_void_p, P32, P64, P64, c_size_t, P32, P64]),
    "sg_exec_signal_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_uint64, c_void_p,
                                   c_void_p]),
    "sg_exec_signal_queued_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_uint64, c_void_p,
                                          c_void_p, c_void_p]),
    "sg_triage_traces_queued": (c_int, [c_void_p, c_void_p, c_void_p, P32, P64, P64, c_size_t, P8, P32, P64]),
    "sg_exec_comps": (c_int, [c_void_p, P64, P64, c_size_t, P64, P64, c_size_t, P64, P32, c_size_t]),
    "sg_exec_comps_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p,
                                  c_void_p, c_uint64]),
    "sg_exec_cover": (c_int, [c_void_p, P64, P64, c_size_t, c_int, P64, P32, c_size_t]),
    "sg_exec_cover_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_int, c_void_p, c_void_p, c_uint64]),
    "sg_triage_runs_from_kcov": (c_int, [c_void_p, c_void_p, P32, P64, c_size_t, P32, P8, c_uint32, P64, P64, P64,
                                         POINTER(c_int32), P64, P32, c_size_t, P64, P32, c_size_t]),
    "sg_triage_runs_from_kcov_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p,
                                             c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64,
                                             c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64]),
    "sg_minimize_pred_from_kcov": (c_int, [c_void_p, c_void_p, c_void_p, P32, P64, c_size_t, P32, P32, c_size_t, P64, P64,
                                           P64, POINTER(c_int32), P8, P64, P32, c_size_t]),
    "sg_minimize_pred_from_kcov_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64,
                                               c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint64,
                                               c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64]),
    "sg_gen_zipf_traces_dev": (c_int, [c_void_p, c_uint64, c_uint64, c_double, c_uint32, c_uint64, c_uint64, c_uint32,
                                       c_uint32, c_void_p]),
    "sg_gen_population_traces_dev": (c_int, [c_void_p, c_uint64, c_uint64, c_uint64, c_uint64, c_double, c_double,
                                             c_uint32, c_uint64, c_uint64, c_uint32, c_uint32, c_void_p]),
    "sg_cover_uncovered": (c_int, [c_void_p, P32, c_size_t, c_uint32, P64, P64, c_size_t, P64, c_size_t, P64, PSZ]),
    "sg_cover_table_create": (c_int, [c_void_p, P64, P64, c_size_t, P64, c_size_t, P64, c_size_t, P64, P32, P32, P32,
                                      c_uint32, c_uint32, POINTER(c_void_p)]),
    "sg_cover_table_destroy": (None, [c_void_p]),
    "sg_cover_table_slots": (c_int, [c_void_p, P64]),
    "sg_cover_lines": (c_int, [c_void_p, P32, c_size_t, c_uint32, P64, P32, P8, P8, P64, P64, PSZ]),
    "sg_cover_lines_set": (c_int, [c_void_p, c_void_p, c_uint32, P64, P32, P8, P8, P64, P64, PSZ]),
    "sg_src_table_create": (c_int, [c_void_p, P8, P8, P64, c_uint32, POINTER(c_void_p)]),
    "sg_src_table_destroy": (None, [c_void_p]),
    "sg_src_table_counts": (c_int, [c_void_p, P64, P64]),
    "sg_src_table_export": (c_int, [c_void_p, P64, P8]),
    "sg_cover_pages": (c_int, [c_void_p, c_void_p, P32, c_size_t, c_uint32, P64, P32, P8, P8, P64, P64, PSZ, P64, P32, P8,
                               c_size_t, PSZ, P32]),
    "sg_cover_pages_set": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, P64, P32, P8, P8, P64, P64, PSZ, P64, P32, P8,
                                   c_size_t, PSZ, P32]),
    "sg_prio_table_create": (c_int, [c_void_p, c_uint32, c_uint32, PF, P8, POINTER(c_void_p)]),
    "sg_prio_table_destroy": (None, [c_void_p]),
    "sg_prio_table_clear": (c_int, [c_void_p]),
    "sg_prio_table_add": (c_int, [c_void_p, P32, P64, c_size_t]),
    "sg_prio_table_add_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64]),
    "sg_prio_table_counts": (c_int, [c_void_p, P64]),
    "sg_call_prios": (c_int, [c_void_p, PF, PF, PI32]),
    "sg_call_prios_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "sg_call_prios_from_progs": (c_int, [c_void_p, P32, P64, c_size_t, PF, PF, PI32]),
    "sg_prog_hashes": (c_int, [c_void_p, P8, P64, c_size_t, P8, P8]),  # (hex: char*, bound as bytes)
    "sg_prog_hashes_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p]),
    "sg_sigset_create": (c_int, [c_void_p, c_uint64, POINTER(c_void_p)]),
    "sg_sigset_destroy": (None, [c_void_p]),
    "sg_sigset_clear": (c_int, [c_void_p]),
    "sg_sigset_count": (c_int, [c_void_p, P64]),
    "sg_sigset_export": (c_int, [c_void_p, P8, c_size_t, PSZ]),
    "sg_sigset_contains": (c_int, [c_void_p, P8, c_size_t, P8]),
    "sg_sigset_add_new": (c_int, [c_void_p, P8, c_size_t, P8]),
    "sg_sigset_add_progs": (c_int, [c_void_p, P8, P64, c_size_t, P8, P8]),
    "sg_hub_sync": (c_int, [c_void_p, P8, P64, c_size_t, P8, P8, P8, c_size_t, PSZ]),
    "sg_sigset_remove": (c_int, [c_void_p, P8, c_size_t, P8]),
    "sg_nametab_create": (c_int, [c_void_p, POINTER(c_void_p)]),
    "sg_nametab_destroy": (None, [c_void_p]),
    "sg_nametab_count": (c_int, [c_void_p, P64]),
    "sg_nametab_add": (c_int, [c_void_p, P8, P64, c_size_t, P32]),
    "sg_call_sets": (c_int, [c_void_p, c_void_p, P8, P64, c_size_t, P8, P64, P64, P32, P32, c_size_t, PSZ]),
    "sg_call_sets_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_uint64]),
    "sg_hubcorpus_create": (c_int, [c_void_p, c_void_p, POINTER(c_void_p)]),
    "sg_hubcorpus_destroy": (None, [c_void_p]),
    "sg_hubcorpus_count": (c_int, [c_void_p, P64]),
    "sg_hubcorpus_export": (c_int, [c_void_p, P8, P64, P64, P32, c_size_t, c_size_t, PSZ, PSZ]),
    "sg_hubcorpus_add": (c_int, [c_void_p, c_void_p, P8, P64, c_size_t, P64, P8, P8, P8, P64, P32, c_size_t, PSZ]),
    "sg_hubcorpus_pending": (c_int, [c_void_p, c_void_p, c_uint64, c_uint64, P64, c_size_t, c_uint64, P8, P64, c_size_t,
                                     PSZ, P64, P64]),
    "sg_hubcorpus_purge": (c_int, [c_void_p, POINTER(c_void_p), c_size_t, P8, c_size_t, PSZ]),
    "sg_inflate_batch": (c_int, [c_void_p, P8, P64, c_size_t, P8, P64, P64, P8, c_size_t, PSZ]),
    "sg_inflate_batch_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_uint64]),
    "sg_db_scan": (c_int, [P8, c_size_t, P64, P32, P64, P64, P32, c_size_t, PSZ, PINT]),
    "sg_db_open": (c_int, [c_void_p, P8, c_size_t, POINTER(c_void_p)]),
    "sg_db_destroy": (None, [c_void_p]),
    "sg_db_counts": (c_int, [c_void_p, P64]),
    "sg_db_export": (c_int, [c_void_p, P64, P8, P64, P64, P8]),
    "sg_db_device": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p)]),
    "sg_db_verify": (c_int, [c_void_p, c_void_p, P8, P64]),
    "sg_deflate_bound": (c_size_t, [c_size_t]),
    "sg_deflate_host": (c_int, [P8, P64, c_size_t, P64, P8, c_size_t, PSZ]),
    "sg_deflate_batch": (c_int, [c_void_p, P8, P64, c_size_t, P64, P8, c_size_t, PSZ]),
    "sg_deflate_batch_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_uint64]),
    "sg_db_serialize": (c_int, [c_void_p, P8, P64, P64, P8, P64, c_size_t, c_int, P8, c_size_t, PSZ]),
    "sg_db_compact": (c_int, [c_void_p, P8, c_size_t, PSZ]),
    "sg_objdump_pcs": (c_int, [c_void_p, P8, c_size_t, P8, c_size_t, P8, c_size_t, P64, c_size_t, PSZ, P32, P64]),
    "sg_objdump_pcs_dev": (c_int, [c_void_p, c_void_p, c_uint64, P8, c_size_t, P8, c_size_t, c_void_p, c_uint64,
                                   c_void_p]),
    "sg_nm_symbols": (c_int, [c_void_p, P8, c_size_t, P64, POINTER(c_int64), P64, P32, P64, P64, P32, c_size_t, PSZ, P32,
                              P64]),
    "sg_nm_symbols_dev": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_uint64, c_void_p]),
    "sg_addr2line_frames": (c_int, [c_void_p, P8, c_size_t, c_size_t, P64, P64, P32, POINTER(c_int64), P32, c_size_t, P64,
                                    P32, P64, P32, c_uint32, P64]),
    "sg_cover_table_from_text": (c_int, [c_void_p, P8, c_size_t, P64, c_size_t, P8, c_size_t, c_size_t, c_uint32, P64, P32,
                                         P64, P32, c_size_t, P64, POINTER(c_void_p)]),
    "sg_addr2line_frames_dev": (c_int, [c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
    "sg_ipc_parse": (c_int,[c_void_p, P32, P64, P64, P32, c_size_t, POINTER(c_int64), P8, POINTER(c_int32), P64, P32,
                             P64, P32]),
    "sg_ipc_parse_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sg_ipc_comps": (c_int, [c_void_p, P32, P64, P64, P32, c_size_t, POINTER(c_int32), P64, P64, c_size_t]),
    "sg_ipc_comps_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p,
                                 c_void_p, c_void_p, c_uint64]),
    "sg_hints_replacers": (c_int, [c_void_p, P64, P64, c_size_t, P64, P64, P64, P64, c_size_t]),
    "sg_hints_replacers_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_void_p,
                                       c_void_p, c_uint64]),
    "sg_comps_pairs": (c_int, [c_void_p, P64, P64, c_size_t, POINTER(c_int32), P64, P64, c_size_t]),
    "sg_comps_pairs_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p,
                                   c_uint64]),
    "sg_hints_from_kcov": (c_int, [c_void_p, P64, P64, c_size_t, P64, P64, POINTER(c_int32), P64, P64, c_size_t]),
    "sg_hints_from_kcov_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_uint64,
                                       c_void_p, c_void_p, c_void_p, c_uint64]),
    "sg_crash_scan": (c_int, [c_void_p, P8, P64, c_size_t, P8, P32, P64, P64, P32, P64, c_size_t, PSZ, P64]),
    "sg_crash_scan_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_uint64, c_void_p, c_void_p]),
    "sg_crash_parse": (c_int, [c_void_p, P8, P64, c_size_t, P64, P64, PI32, P64, P64, P64, P64, P64, P8, c_size_t, PSZ,
                               P64]),
    "sg_crash_parse_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_uint64,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64,
                                   c_void_p]),
    "sg_console_output": (c_int, [c_void_p, P8, P64, c_size_t, P64, P8, c_size_t, PSZ, P64]),
    "sg_console_output_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_void_p, c_void_p, c_uint64,
                                      c_void_p]),
}


class SyzSigError(RuntimeError):
    def __init__(self, fn, rc, msg):
        super().__init__(f"{fn} failed ({rc}): {msg}")
        self.rc = rc


def _preload_torch_hip_runtime():
    """One HIP runtime per process: when PyTorch-ROCm is installed, bind
    libsyzsig to the libamdhip64 that torch ships (torch loads it by the name
    `libamdhip64.so`, we by the soname `libamdhip64.so.7`; loading ours first
    would put two runtimes in the process).  Does not import torch."""
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(rt):
                ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)
    except OSError:
        pass


def _load():
    _preload_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C syzkaller_amd` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(fn_name, rc):
    if rc != SG_OK:
        msg = lib.sg_last_error()
        raise SyzSigError(fn_name, rc, msg.decode() if msg else "")
    return rc


def call(fn_name, *args):
    return check(fn_name, getattr(lib, fn_name)(*args))
