"""ctypes declarations for include/tad.h — field for field what a cgo `import "C"` block sees."""
import ctypes as C
import os

from . import build as _build

u64, i64, i32, u32, f64, f32 = C.c_uint64, C.c_int64, C.c_int32, C.c_uint32, C.c_double, C.c_float

TAD_ABI_VERSION = 13
TAD_KEY_SKIP = (1 << 64) - 1
TAD_OK = 0
TAD_ERR_INVALID_ARGUMENT, TAD_ERR_NO_DEVICE, TAD_ERR_OUT_OF_MEMORY, TAD_ERR_HIP = -1, -2, -3, -4
TAD_ERR_KEY_RANGE, TAD_ERR_GRID_TOO_LARGE, TAD_ERR_BUSY = -5, -6, -7
TAD_ALGO = {"EWMA": 0, "ARIMA": 1, "DBSCAN": 2, "DROP": 3}
TAD_AGG = {"": 0, None: 0, "None": 0, "pod": 1, "svc": 2, "external": 3}
TAD_OP = {"auto": 0, "max": 1, "sum": 2}
TAD_MEM_HOST, TAD_MEM_DEVICE = 0, 1
TAD_FLAG_EMIT_ALL_POINTS = 1
TAD_FLAG_KEY_U32, TAD_FLAG_TIME_U32 = 2, 4   # narrow input columns: uint32 key ids / uint32 DateTime seconds (tad.h, tad_columns)
TAD_KEY_SKIP32 = (1 << 32) - 1
TAD_FEATURE_NARROW_COLUMNS = 1               # tad_features() bit: the library honours the two flags above
TAD_FEATURE_STREAM_DBSCAN = 2                # tad_features() bit: tad_state_create_ex(TAD_STATE_HISTORY), tad_run_stream with DBSCAN
TAD_STATE_HISTORY = 1                        # tad_state_create_ex flag: keep every key's aggregated point values (sorted)
TAD_FEATURE_STREAM_ARIMA = 4                 # tad_features() bit: tad_state_create_ex(TAD_STATE_SERIES), tad_run_stream with ARIMA
TAD_STATE_SERIES = 2                         # tad_state_create_ex flag: keep every key's aggregated point values (time order)
TAD_FEATURE_STREAM_TRIM = 8                  # tad_features() bit: TAD_STATE_TIMES, tad_state_trim, tad_state_bytes, export / import of times
TAD_STATE_TIMES = 8                          # tad_state_create_ex flag (with TAD_STATE_SERIES): keep every series point's flowEndSeconds
TAD_FEATURE_STATE_RUN = 16                   # tad_features() bit: tad_run_state, the batch job's rows over everything a state holds
TAD_FEATURE_STATE_MERGE = 32                 # tad_features() bit: tad_state_merge, a batch placed by time (late, re-sent and split rows)
TAD_FEATURE_STATE_REPLACE = 65536            # tad_features() bit: tad_state_replace, a batch that replaces (re-read windows that must not double)
TAD_REPLACE_RANGE = 1                        # tad_state_replace flag: erase every point of the state inside [from_t, to_t) that the batch does not name
TAD_FEATURE_STATE_WINDOW = 64                # tad_features() bit: tad_run_state_window, tad_run_state over a time range of the state, read-only
TAD_FEATURE_KEY_DICT = 128                   # tad_features() bit: tad_keydict, a persistent tuple -> key id dictionary on the device
TAD_FEATURE_KEY_RETIRE = 256                 # tad_features() bit: tad_state_compact / tad_keydict_compact, dead keys dropped and the rest renumbered
TAD_FEATURE_STATE_DROP = 512                 # tad_features() bit: tad_drop_state / tad_drop_stream, the drop detector on a series state
TAD_FEATURE_DROP_ROWS = 1024                 # tad_features() bit: tad_drop_select, flow rows -> the drop job's (endpoint, direction, day, count) rows
TAD_FEATURE_KEY_SELECT = 2048                # tad_features() bit: tad_keydict_select, tad_run_state_keys, tad_drop_state_keys: jobs over selected keys of a state
TAD_FEATURE_STRING_DICT = 4096               # tad_features() bit: tad_strdict, a persistent string -> code dictionary on the device, with match masks
TAD_FEATURE_DICT_DECODE = 8192               # tad_features() bit: tad_keydict_gather, tad_strdict_decode: ids -> tuples and codes -> strings on the device
TAD_FEATURE_STRING_RETIRE = 16384            # tad_features() bit: tad_keydict_mark_codes, tad_strdict_compact, tad_keydict_recode: dead strings dropped, codes renumbered
TAD_FEATURE_STRING_LIKE = 32768              # tad_features() bit: tad_strdict_like: LIKE / ilike patterns with % and _ matched on the device
TAD_FEATURE_STATE_ALERTS = 131072            # tad_features() bit: tad_state_merge_changes / tad_state_replace_changes: what a merge or a replace changed; tad_run_state_since / tad_drop_state_since
TAD_FEATURE_STATE_BUCKETS = 262144           # tad_features() bit: tad_run_state_buckets: a state's window judged in time buckets
TAD_FEATURE_STATE_ROLLUP = 524288            # tad_features() bit: tad_state_rollup: a state's old points folded into time buckets, in place
TAD_NO_CHANGE = (1 << 63) - 1              # tad_changes.key_since: the key's series did not change
TAD_LIKE_NOCASE = 1                          # tad_strdict_like flags: compare after folding 'A'..'Z' to 'a'..'z' (ilike)
TAD_CODE_NONE = -1                           # tad_strdict_lookup: the string is not in the dictionary
TAD_STR_EQUAL, TAD_STR_CONTAINS_NOCASE = 0, 1   # tad_strdict_match: the value is the pattern / the pattern occurs in it, ASCII letters without case


class Plan(C.Structure):
    """tad_plan: plan overrides, every field 0 = the engine decides (tests and A/B measurements set them)."""
    _fields_ = [("stage0", i32), ("partition_pass", i32), ("histogram", i32), ("sparse", i32), ("sparse_classes", i32),
                ("ewma_emit", i32), ("ewma_emit_rows", u32), ("reserved0", i32), ("tile_cells", i32), ("sparse_sort", i32), ("reserved1", i32)]


PLAN_VALUES = {   # symbolic values accepted by TadEngine(plan=...) / TadEngine.plan(...)
    "stage0": {"auto": 0, "v1": 1, "v2": 2}, "partition_pass": {"auto": 0, "sort": 1, "wc": 2, "wc_sectors": 3}, "histogram": {"auto": 0, "exact": 1, "sampled": 2},
    "sparse": {"auto": 0, "never": 1, "always": 2}, "sparse_classes": {"auto": 0, "always": 1}, "ewma_emit": {"auto": 0, "staged": 0, "lane": 1}, "tile_cells": {"auto": 0, "wide": 1},
    "sparse_sort": {"auto": 0, "lsd": 1, "partition": 2},
}


def make_plan(**kw):
    p = Plan()
    for name, v in kw.items():
        if name not in dict((f[0], 1) for f in Plan._fields_):
            raise ValueError("unknown tad_plan field %r" % name)
        if isinstance(v, str):
            v = PLAN_VALUES[name][v]
        setattr(p, name, int(v))
    return p


class KeyColumns(C.Structure):
    """tad_key_columns: the key tuples of a batch for tad_factorize (up to 8 int64 columns, optional keep masks, optional second side)."""
    _fields_ = [("n_rows", u64), ("n_cols", i32), ("cols_a", C.POINTER(C.c_void_p)), ("keep_a", C.c_void_p),
                ("cols_b", C.POINTER(C.c_void_p)), ("keep_b", C.c_void_p), ("memory", C.c_int)]


class StringColumn(C.Structure):
    """tad_string_column: one Arrow string column (offsets + bytes + optional validity bitmap) for tad_encode_strings."""
    _fields_ = [("n_rows", u64), ("offsets", C.c_void_p), ("offset_bits", i32), ("data", C.c_void_p), ("data_bytes", u64),
                ("validity", C.c_void_p), ("validity_offset", u64), ("memory", C.c_int)]


class EngineOpts(C.Structure):
    _fields_ = [("device", i32), ("stream", C.c_void_p), ("workspace_limit", u64), ("plan", Plan), ("max_jobs_in_flight", i32), ("reserved", i32)]


class Job(C.Structure):
    _fields_ = [("algo", C.c_int), ("agg_flow", C.c_int), ("value_op", C.c_int),
                ("start_time", i64), ("end_time", i64), ("ewma_alpha", f64), ("dbscan_eps", f64),
                ("dbscan_min_samples", i32), ("arima_maxiter", i32), ("drop_nsigma", f64), ("drop_min_samples", i32),
                ("flags", u32), ("id", C.c_char * 64)]


TAD_KEY_HIST_BYTES = 256 * 16384 * 4


class KeyHist(C.Structure):
    """tad_key_hist: tad_factorize_hist's by-product (key-bin histogram per Stage-0 workgroup); bins is device memory of TAD_KEY_HIST_BYTES."""
    _fields_ = [("n_rows", u64), ("num_keys", u64), ("chunk_rows", u64), ("workgroups", u32), ("nbins", u32), ("shift", u32), ("sides", u32),
                ("bins", C.c_void_p)]


class Columns(C.Structure):
    _fields_ = [("n_rows", u64), ("key_id", C.c_void_p), ("key_id2", C.c_void_p),
                ("flow_end_s", C.c_void_p), ("flow_start_s", C.c_void_p), ("value", C.c_void_p),
                ("num_keys", u64), ("memory", C.c_int), ("t0", i64), ("step", i64), ("n_buckets", u64), ("key_hist", C.POINTER(KeyHist))]


class Stats(C.Structure):
    _fields_ = [("rows_in", u64), ("rows_used", u64), ("n_keys", u64), ("n_points", u64),
                ("n_anomalies", u64), ("keys_no_result", u64), ("kalman_steps", u64),
                ("arima_fits", u64), ("arima_nan_fits", u64), ("pts_mean", f64), ("pts_m2", f64), ("t0", i64), ("step", i64), ("n_buckets", u64),
                ("ms_meta", f32), ("ms_stage0", f32), ("ms_scatter", f32), ("ms_detect", f32),
                ("ms_total", f32), ("stage0_path", i32), ("stage0_attempts", i32), ("hist_sampled", i32), ("host_syncs", i32),
                ("job_context", i32), ("arima_relaunches", i32)]


class Result(C.Structure):
    _fields_ = [("n_rows", u64), ("key_id", C.c_void_p), ("flow_end_s", C.c_void_p),
                ("throughput", C.c_void_p), ("algo_calc", C.c_void_p), ("stddev", C.c_void_p),
                ("anomaly", C.c_void_p), ("memory", C.c_int), ("stats", Stats), ("id", C.c_char * 64)]


class MergeStats(C.Structure):
    """tad_merge_stats: what one tad_state_merge call did with the batch's points."""
    _fields_ = [("rows_in", u64), ("rows_used", u64), ("batch_points", u64), ("points_too_old", u64), ("points_appended", u64),
                ("points_inserted", u64), ("points_combined", u64), ("keys_touched", u64), ("keys_replayed", u64),
                ("stage0_path", i32), ("stage0_attempts", i32), ("job_context", i32), ("reserved", i32),
                ("ms_stage0", f32), ("ms_merge", f32), ("ms_total", f32), ("reserved1", f32)]


class ReplaceStats(C.Structure):
    """tad_replace_stats: what one tad_state_replace call did with the batch's points and with the points the state held."""
    _fields_ = [("rows_in", u64), ("rows_used", u64), ("batch_points", u64), ("points_too_old", u64), ("points_appended", u64),
                ("points_inserted", u64), ("points_replaced", u64), ("points_erased", u64), ("keys_emptied", u64), ("keys_touched", u64),
                ("keys_replayed", u64), ("stage0_path", i32), ("stage0_attempts", i32), ("job_context", i32), ("reserved", i32),
                ("ms_stage0", f32), ("ms_replace", f32), ("ms_total", f32), ("reserved1", f32)]


class Changes(C.Structure):
    """tad_changes: the change report of tad_state_merge_changes / tad_state_replace_changes."""
    _fields_ = [("key_since", C.c_void_p), ("len", u64), ("memory", C.c_int), ("keys_changed", u64), ("points_changed", u64),
                ("min_t", i64), ("max_t", i64)]


class ReportWindow(C.Structure):
    """tad_report_window: the window, the key mask and the since rules of tad_run_state_since / tad_drop_state_since."""
    _fields_ = [("from_t", i64), ("to_t", i64), ("keep_points", u64), ("key_keep", C.c_void_p), ("key_since", C.c_void_p), ("since_t", i64),
                ("num_keys", u64), ("key_memory", C.c_int)]


class BucketWindow(C.Structure):
    """tad_bucket_window: tad_report_window plus the bucket length, origin and folding operation of tad_run_state_buckets."""
    _fields_ = ReportWindow._fields_ + [("bucket_s", i64), ("bucket_origin", i64), ("bucket_op", C.c_int)]


class RollupStats(C.Structure):
    """tad_rollup_stats: what one tad_state_rollup call folded."""
    _fields_ = [("points_before", u64), ("points_after", u64), ("points_rolled", u64), ("buckets", u64), ("keys_changed", u64), ("before_t", i64),
                ("ms_total", f64), ("job_context", i32)]


class CompactStats(C.Structure):
    """tad_compact_stats: what one tad_state_compact call retired and moved."""
    _fields_ = [("keys_before", u64), ("keys_after", u64), ("num_keys", u64), ("keys_unseen", u64), ("keys_idle", u64), ("points_dropped", u64),
                ("series_points_moved", u64), ("history_points_moved", u64), ("bytes_before", u64), ("bytes_after", u64),
                ("job_context", i32), ("reserved", i32), ("ms_total", f32), ("reserved1", f32)]


class StrdictCompactStats(C.Structure):
    """tad_strdict_compact_stats: what one tad_strdict_compact call retired and what the dictionary holds before and after."""
    _fields_ = [("values_before", u64), ("values_after", u64), ("bytes_before", u64), ("bytes_after", u64), ("arena_used_before", u64),
                ("arena_used_after", u64), ("job_context", i32), ("reserved", i32), ("ms_total", f32), ("reserved1", f32)]


class Points(C.Structure):
    _fields_ = [("n_points", u64), ("key_id", C.c_void_p), ("flow_end_s", C.c_void_p), ("value", C.c_void_p),
                ("memory", C.c_int), ("stats", Stats)]


class DropFlowColumns(C.Structure):
    """tad_drop_flow_columns: the ten flow-table columns tad_drop_select reads (two UInt8 actions, the times, six dictionary-code columns, keep)."""
    _fields_ = [("n_rows", u64), ("ingress_action", C.c_void_p), ("egress_action", C.c_void_p), ("flow_start_s", C.c_void_p), ("flow_end_s", C.c_void_p),
                ("src_ip", C.c_void_p), ("src_pod_ns", C.c_void_p), ("src_pod_name", C.c_void_p),
                ("dst_ip", C.c_void_p), ("dst_pod_ns", C.c_void_p), ("dst_pod_name", C.c_void_p),
                ("src_pod_null", i64), ("dst_pod_null", i64), ("keep", C.c_void_p), ("flags", u32), ("memory", C.c_int)]


class DropRows(C.Structure):
    """tad_drop_rows: tad_drop_select's result, one row per selected flow row in input order; owned by the library."""
    _fields_ = [("n_rows", u64), ("endpoint_kind", C.c_void_p), ("endpoint_ns", C.c_void_p), ("endpoint_name", C.c_void_p), ("direction", C.c_void_p),
                ("day_s", C.c_void_p), ("count", C.c_void_p), ("row", C.c_void_p), ("memory", C.c_int)]


# every symbol include/tad.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "tad_abi_version": (C.c_int, []),
    "tad_features": (C.c_int, []),
    "tad_engine_create": (C.c_int, [C.POINTER(EngineOpts), C.POINTER(C.c_void_p)]),
    "tad_engine_destroy": (None, [C.c_void_p]),
    "tad_engine_set_plan": (C.c_int, [C.c_void_p, C.POINTER(Plan)]),
    "tad_last_error": (C.c_char_p, [C.c_void_p]),
    "tad_run": (C.c_int, [C.c_void_p, C.POINTER(Job), C.POINTER(Columns), C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_result_free": (None, [C.c_void_p, C.POINTER(Result)]),
    "tad_state_create": (C.c_int, [C.c_void_p, u64, C.POINTER(C.c_void_p)]),
    "tad_state_destroy": (None, [C.c_void_p, C.c_void_p]),
    "tad_state_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_state_resize": (C.c_int, [C.c_void_p, C.c_void_p, u64]),
    "tad_state_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_state_create_ex": (C.c_int, [C.c_void_p, u64, u32, C.POINTER(C.c_void_p)]),
    "tad_state_history_points": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(u64)]),
    "tad_state_export_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_state_import_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_state_series_points": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(u64)]),
    "tad_state_export_series": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_state_import_series": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_state_trim": (C.c_int, [C.c_void_p, C.c_void_p, u64, i64, f64, C.POINTER(u64)]),
    "tad_state_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(u64)]),
    "tad_state_rollup": (C.c_int, [C.c_void_p, C.c_void_p, i64, i64, i64, C.c_int, f64, C.POINTER(RollupStats)]),
    "tad_state_export_times": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_state_import_times": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_run_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(Columns), C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_run_state": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_state_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(Columns), i64, C.POINTER(MergeStats)]),
    "tad_state_replace": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(Columns), C.c_uint32, i64, i64, i64, C.POINTER(ReplaceStats)]),
    "tad_state_merge_changes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(Columns), i64, C.POINTER(MergeStats), C.POINTER(Changes)]),
    "tad_state_replace_changes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(Columns), C.c_uint32, i64, i64, i64, C.POINTER(ReplaceStats),
                                            C.POINTER(Changes)]),
    "tad_run_state_window": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), i64, i64, u64, C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_window_history_by_sort": (C.c_int, [u64, u64]),
    "tad_aggregate": (C.c_int, [C.c_void_p, C.POINTER(Job), C.POINTER(Columns), C.c_int, C.POINTER(C.POINTER(Points))]),
    "tad_points_free": (None, [C.c_void_p, C.POINTER(Points)]),
    "tad_shard_rows": (C.c_int, [C.c_void_p, C.POINTER(Columns), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_factorize": (C.c_int, [C.c_void_p, C.POINTER(KeyColumns), C.c_void_p, C.c_void_p, C.c_void_p, u64, C.POINTER(u64)]),
    "tad_factorize_hist": (C.c_int, [C.c_void_p, C.POINTER(KeyColumns), C.c_void_p, C.c_void_p, C.c_void_p, u64, C.POINTER(u64), C.POINTER(KeyHist)]),
    "tad_keydict_create": (C.c_int, [C.c_void_p, i32, u64, C.POINTER(C.c_void_p)]),
    "tad_keydict_destroy": (None, [C.c_void_p, C.c_void_p]),
    "tad_keydict_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(KeyColumns), C.c_void_p, C.c_void_p, C.c_void_p, u64, C.POINTER(u64), C.POINTER(u64)]),
    "tad_keydict_lookup": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(KeyColumns), C.c_void_p, C.c_void_p]),
    "tad_keydict_num_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(u64)]),
    "tad_keydict_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(u64)]),
    "tad_keydict_export": (C.c_int, [C.c_void_p, C.c_void_p, u64, u64, C.POINTER(C.c_void_p), C.c_void_p]),
    "tad_keydict_import": (C.c_int, [C.c_void_p, C.c_void_p, u64, C.POINTER(C.c_void_p), C.c_void_p]),
    "tad_strdict_create": (C.c_int, [C.c_void_p, u64, u64, C.POINTER(C.c_void_p)]),
    "tad_strdict_destroy": (None, [C.c_void_p, C.c_void_p]),
    "tad_strdict_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StringColumn), C.c_void_p, C.c_void_p, u64, C.POINTER(u64), C.POINTER(u64)]),
    "tad_strdict_lookup": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StringColumn), C.c_void_p]),
    "tad_strdict_num_values": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(u64)]),
    "tad_strdict_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(u64)]),
    "tad_strdict_export": (C.c_int, [C.c_void_p, C.c_void_p, u64, u64, C.c_void_p, C.c_void_p, u64, C.POINTER(u64)]),
    "tad_strdict_import": (C.c_int, [C.c_void_p, C.c_void_p, u64, C.c_void_p, C.c_void_p]),
    "tad_strdict_match": (C.c_int, [C.c_void_p, C.c_void_p, i32, C.c_void_p, u64, C.c_void_p, u64, C.c_int, C.POINTER(u64)]),
    "tad_strdict_like": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64, C.c_uint32, C.c_void_p, u64, C.c_int, C.POINTER(u64)]),
    "tad_keydict_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "tad_strdict_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64, C.c_int, C.c_void_p, C.c_void_p, u64, C.c_int, C.POINTER(u64)]),
    "tad_keydict_mark_codes": (C.c_int, [C.c_void_p, C.c_void_p, i32, i32, C.c_void_p, u64, C.c_int, C.POINTER(u64)]),
    "tad_strdict_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64, C.c_int, C.c_void_p, C.c_int, C.POINTER(StrdictCompactStats)]),
    "tad_keydict_recode": (C.c_int, [C.c_void_p, C.c_void_p, i32, C.POINTER(i32), C.POINTER(C.c_void_p), C.POINTER(u64), C.c_int, C.POINTER(u64)]),
    "tad_state_compact": (C.c_int, [C.c_void_p, C.c_void_p, i64, C.c_void_p, C.c_int, C.POINTER(CompactStats)]),
    "tad_keydict_compact": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64, C.c_int, C.POINTER(u64)]),
    "tad_drop_state": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), i64, i64, u64, C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_keydict_select": (C.c_int, [C.c_void_p, C.c_void_p, i32, C.POINTER(i32), C.POINTER(C.c_void_p), C.POINTER(u64), i32, C.c_void_p, u64, C.c_int, C.POINTER(u64)]),
    "tad_run_state_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), i64, i64, u64, C.c_void_p, u64, C.c_int, C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_drop_state_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), i64, i64, u64, C.c_void_p, u64, C.c_int, C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_run_state_since": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(ReportWindow), C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_drop_state_since": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(ReportWindow), C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_run_state_buckets": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(BucketWindow), C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_drop_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Job), C.POINTER(Columns), C.c_int, C.POINTER(C.POINTER(Result))]),
    "tad_drop_select": (C.c_int, [C.c_void_p, C.POINTER(DropFlowColumns), i64, i64, C.c_int, C.POINTER(C.POINTER(DropRows))]),
    "tad_drop_rows_free": (None, [C.c_void_p, C.POINTER(DropRows)]),
    "tad_encode_strings": (C.c_int, [C.c_void_p, C.POINTER(StringColumn), C.c_void_p, C.c_void_p, u64, C.POINTER(u64)]),
    "tad_widen_column": (C.c_int, [C.c_void_p, C.c_void_p, i32, i32, C.c_int, u64, C.c_void_p, u64, C.c_void_p]),
    "tad_mask_rows": (C.c_int, [C.c_void_p, u64, i32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(u64), i32, C.c_void_p]),
    "tad_host_alloc": (C.c_int, [C.c_void_p, u64, C.POINTER(C.c_void_p)]),
    "tad_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tad_progress": (C.c_int, [C.c_void_p, C.POINTER(i32), C.POINTER(i32)]),
    "tad_job_progress": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(i32), C.POINTER(i32)]),
    "tad_jobs_in_flight": (C.c_int, [C.c_void_p]),
    "tad_series_ewma": (C.c_int, [C.c_void_p, C.c_void_p, u64, f64, C.c_void_p]),
    "tad_series_ewma_anomaly": (C.c_int, [C.c_void_p, C.c_void_p, u64, f64, C.c_int, f64, C.c_void_p]),
    "tad_series_stddev": (C.c_int, [C.c_void_p, C.c_void_p, u64, C.POINTER(C.c_int), C.POINTER(f64)]),
    "tad_series_dbscan_anomaly": (C.c_int, [C.c_void_p, C.c_void_p, u64, f64, C.c_int, C.c_void_p]),
    "tad_series_drop": (C.c_int, [C.c_void_p, C.c_void_p, u64, f64, C.c_int, C.POINTER(C.c_int), C.POINTER(f64), C.POINTER(f64), C.c_void_p]),
    "tad_series_arima": (C.c_int, [C.c_void_p, C.c_void_p, u64, C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    "tad_series_arima_anomaly": (C.c_int, [C.c_void_p, C.c_void_p, u64, C.c_int, C.c_int, f64, C.c_void_p, C.POINTER(u64)]),
    "tad_synth_generate": (C.c_int, [C.c_void_p, u64, u64, u64, u64, u64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tad_device_alloc": (C.c_int, [C.c_void_p, u64, C.POINTER(C.c_void_p)]),
    "tad_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tad_copy_to_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64]),
    "tad_copy_to_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64]),
}

_libs = {}


def load_library(build_if_missing=True, path=None):
    """dlopen theia_amd/lib/libtad_mi355x.so (building it in-tree first if needed).  `path` (or TAD_LIBRARY_PATH) names another build
    of the library — measurement variants of tools/build_variants.py; one handle per path, so two builds can run in one process."""
    path = path or os.environ.get("TAD_LIBRARY_PATH") or _build.LIB_PATH   # override: A/B two builds of the library
    path = os.path.abspath(path)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        if not build_if_missing or path != os.path.abspath(_build.LIB_PATH):
            raise OSError("%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        _build.build_library()
    lib = C.CDLL(path)
    shipped = path == os.path.abspath(_build.LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        if not shipped and not hasattr(lib, name):     # an older build loaded for an A/B measurement may lack the newest entry points
            continue
        fn = getattr(lib, name)  # AttributeError here = the library does not export the header's symbol
        fn.restype = res
        fn.argtypes = args
    if lib.tad_abi_version() != TAD_ABI_VERSION:
        raise OSError("%s ABI %d != binding ABI %d" % (os.path.basename(path), lib.tad_abi_version(), TAD_ABI_VERSION))
    _libs[path] = lib
    return lib
