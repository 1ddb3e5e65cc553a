/*
 * tad.h — C ABI of libtad_mi355x.so, the MI355X (gfx950) throughput-anomaly-detection engine.
 *
 * This is the drop-in boundary for ONE path of antrea-io/theia: the Throughput Anomaly
 * Detection job.  The reference has no FFI for it — the boundary there is a process boundary:
 *   - pkg/controller/anomalydetector/controller.go:525-698 builds the job's argument vector
 *     (--algo, --start_time, --end_time, --agg-flow, --pod-label, ... --id) and launches a
 *     SparkApplication;
 *   - plugins/anomaly-detection/anomaly_detection.py:647-710 (anomaly_detection) runs it:
 *     ClickHouse GROUP BY (:507-614) -> per-key series + stddev_samp (:664-684) ->
 *     EWMA / ARIMA / DBSCAN per key (:146-349) -> explode + keep anomalies (:352-421) ->
 *     append to default.tadetector (:713-726).
 * A cgo host (theia-manager) binds exactly the entry points below instead of launching Spark;
 * INTEGRATION.md shows that binding.  Every struct is plain C: pointers, sizes, enums.  No
 * callbacks, no retained caller pointers after return, no exceptions across the boundary.
 *
 * Strings never cross the boundary: the host dictionary-encodes the mode's key columns
 * (anomaly_detection.py:109-137 DF_GROUP_COLUMNS / DF_AGG_GRP_COLUMNS_*) into dense uint64
 * key ids and evaluates the string predicates of the SQL (:507-614); a row the predicates reject
 * carries TAD_KEY_SKIP.
 */
#ifndef THEIA_TAD_H
#define THEIA_TAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAD_ABI_VERSION 13
#define TAD_KEY_SKIP UINT64_MAX /* row (or its second key) does not take part */

/* ---- error codes (0 = ok, negative = failure; text via tad_last_error) ---- */
enum {
  TAD_OK = 0,
  TAD_ERR_INVALID_ARGUMENT = -1, /* maps to the controller's illegal-argument FAILED state,
                                    controller.go:505-514 */
  TAD_ERR_NO_DEVICE = -2,        /* no gfx950 device / HIP runtime failure at create */
  TAD_ERR_OUT_OF_MEMORY = -3,
  TAD_ERR_HIP = -4,              /* a HIP call or kernel failed */
  TAD_ERR_KEY_RANGE = -5,        /* a key id >= num_keys (and != TAD_KEY_SKIP) */
  TAD_ERR_GRID_TOO_LARGE = -6,   /* num_keys x time-lattice does not fit the workspace limit */
  TAD_ERR_BUSY = -7
};

/* --algo, controller.go:527-533 ("EWMA" | "ARIMA" | "DBSCAN"); anomaly_detection.py:697-709 */
/* TAD_ALGO_DROP: the abnormal-traffic-drop detector of the reference's Snowflake backend
 * (snowflake/udfs/udfs/drop_detection/drop_detection_udf.py:42-56): per key mean / sample std of the aggregated counts,
 * anomaly outside mean +- drop_nsigma * std, keys with fewer than drop_min_samples points yield nothing.
 * Result rows: throughput = the count, algo_calc = the key's mean, stddev = its std. */
typedef enum { TAD_ALGO_EWMA = 0, TAD_ALGO_ARIMA = 1, TAD_ALGO_DBSCAN = 2, TAD_ALGO_DROP = 3 } tad_algo;

/* --agg-flow, controller.go:560-620; anomaly_detection.py:617-628 (aggType literal).
 * NONE  : per-connection keys, max(throughput)   (anomaly_detection.py:52-61)
 * POD / SVC / EXTERNAL : sum(throughput)         (:63-106)                              */
typedef enum { TAD_AGG_NONE = 0, TAD_AGG_POD = 1, TAD_AGG_SVC = 2, TAD_AGG_EXTERNAL = 3 } tad_agg_flow;

/* Stage-0 aggregate over rows that share (key, flowEndSeconds). UInt64 semantics of ClickHouse:
 * SUM wraps mod 2^64, MAX is unsigned (create_table.sh:74 `throughput UInt64`). */
typedef enum { TAD_OP_AUTO = 0, TAD_OP_MAX = 1, TAD_OP_SUM = 2 } tad_value_op;

typedef enum { TAD_MEM_HOST = 0, TAD_MEM_DEVICE = 1 } tad_mem;

/* tad_job.flags */
#define TAD_FLAG_EMIT_ALL_POINTS 1u /* result = every point (plotDF before the filter of :394),
                                       with its verdict in tad_result.anomaly; for inspection/tests */
#define TAD_FLAG_KEY_U32  2u /* key_id / key_id2 point to uint32_t[n_rows]; TAD_KEY_SKIP32 = row does not take part (tad_columns) */
#define TAD_FLAG_TIME_U32 4u /* flow_end_s / flow_start_s point to uint32_t[n_rows]: DateTime, unsigned epoch seconds (tad_columns) */
#define TAD_KEY_SKIP32 UINT32_MAX

/* tad_features(): what this build of the library understands beyond TAD_ABI_VERSION */
#define TAD_FEATURE_NARROW_COLUMNS 1u /* TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32 are honoured */
#define TAD_FEATURE_STREAM_DBSCAN 2u  /* tad_state_create_ex(TAD_STATE_HISTORY) and tad_run_stream with TAD_ALGO_DBSCAN */
#define TAD_FEATURE_STREAM_ARIMA 4u   /* tad_state_create_ex(TAD_STATE_SERIES) and tad_run_stream with TAD_ALGO_ARIMA */
#define TAD_FEATURE_STREAM_TRIM 8u    /* TAD_STATE_TIMES, tad_state_trim, tad_state_bytes, tad_state_export_times / import_times */
#define TAD_FEATURE_STATE_RUN 16u     /* tad_run_state: the batch job's rows over everything a series + times state holds */

typedef struct tad_engine tad_engine; /* opaque; one per GPU; runs up to max_jobs_in_flight jobs concurrently (ABI 12) */

/* Plan overrides (ABI 7).  Every field 0 = the engine decides from the shape of the batch, which is what a production host
 * passes.  A non-zero field forces one of the strategies the engine would otherwise choose between: the parity tests run
 * every strategy on the same table, A/B measurements time them on the same box.  ABI <= 6 read TAD_* environment variables
 * per job for this — process-global state that a host with several workers (controller.go:199-201) cannot scope to a job
 * or an engine; since ABI 7 the library reads no environment variable at all. */
typedef struct {
  int32_t stage0;            /* 1 = direct atomic scatter into the grid, 2 = partition + LDS tiles whatever the batch size */
  int32_t partition_pass;    /* 1 = sort-by-tile pass B, 2 = write-combining pass B whenever its queues fit LDS, 3 = as 2 but 64-byte sectors even where whole 128-byte lines fit (A/B) */
  int32_t histogram;         /* 1 = exact per-workgroup histogram in pass A (regions of pass B never sized from a sample), 2 = sampled wherever possible (A/B) */
  int32_t sparse;            /* 1 = never, 2 = always the sort-based Stage 0 for sparse tables */
  int32_t sparse_classes;    /* 1 = always run a sparse table as length classes of keys */
  int32_t ewma_emit;         /* 1 = lane-per-key emit for the EWMA job instead of the LDS-staged one */
  uint32_t ewma_emit_rows;   /* LDS rows per wavefront of the staged EWMA emit (<= 4096); 0 = sized from the row count */
  int32_t reserved0;         /* must be 0 (ABI 8-11: one_sync — the one-synchronisation form of a job was removed in ABI 12: a placement-neutral
                                A/B put it at 1.0 % of a C2 / C4 job, profiles/r6_a1_ab1_*.log) */
  int32_t tile_cells;        /* 1 = 8-byte tile cells in the settle mode of DBSCAN jobs with `max` (ABI 8; default: 32-bit cells, value + 1) */
  int32_t sparse_sort;       /* sparse tables (ABI 9; was `reserved`): 1 = always the LSD radix sort, 2 = the partition pass + LDS sort wherever its plan fits
                                (0: when pass A ran with its key-bin histogram, i.e. >= 2^22 rows) */
  int32_t reserved1;         /* must be 0 (ABI 11: placement — the placement search of pass B's record buffer was removed in ABI 12: 7-21 ms per
                                search to win <= 0.04 ms per job on the SAME column buffers; a controller brings new columns with every job,
                                profiles/r6_a1_cold_*.log) */
} tad_plan;

typedef struct {
  int32_t device;            /* HIP device ordinal */
  void *stream;              /* hipStream_t to run on, or NULL: the engine creates its own */
  uint64_t workspace_limit;  /* bytes of HBM ONE job may use for its grid and Stage-0 buffers; 0 = 3/4 of what is free at create.  Per job in
                                flight: contexts keep their (grow-only) buffers between jobs, and when an allocation fails the idle contexts'
                                buffers are given back to the device before the job fails */
  tad_plan plan;             /* all zero in production */
  int32_t max_jobs_in_flight;/* ABI 12: job contexts (own HIP stream, events, workspace) the engine may create — tad_run calls from that many
                                threads run concurrently on the GPU, further callers wait for a context.  0 = 4 (controller.go:199-201 runs four
                                workers; Spark ran one pod per job), 1 = jobs serialise (ABI <= 11), max 16.  Forced to 1 when `stream` is
                                given.  Contexts are created on demand: a serial caller only ever uses the first */
  int32_t reserved;          /* must be 0 */
} tad_engine_opts;

/* Mirrors the job's argument vector (anomaly_detection.py:781-870). */
typedef struct {
  tad_algo algo;
  tad_agg_flow agg_flow;
  tad_value_op value_op;     /* AUTO: MAX for TAD_AGG_NONE, SUM otherwise */
  int64_t start_time;        /* epoch seconds; 0 = unset. Row kept iff flow_start_s >= start_time
                                (:581-583). Ignored when columns.flow_start_s is NULL. */
  int64_t end_time;          /* epoch seconds; 0 = unset. Row kept iff flow_end_s < end_time (:584-586) */
  double ewma_alpha;         /* 0 -> 0.5 (:157) */
  double dbscan_eps;         /* 0 -> 250000000 (:342) */
  int32_t dbscan_min_samples;/* 0 -> 4 (:342) */
  int32_t arima_maxiter;     /* 0 -> 50 (statsmodels fit() default) */
  double drop_nsigma;        /* 0 -> 3 (drop_detection_udf.py:49-50) */
  int32_t drop_min_samples;  /* 0 -> 3 (:44) */
  uint32_t flags;            /* TAD_FLAG_* */
  char id[64];               /* --id, echoed into the result (tadetector.id, :503) */
} tad_job;

/* By-product of tad_factorize_hist (ABI 12): how many of each Stage-0 workgroup's rows fall into each key bin — what pass A of tad_run would
 * otherwise count with a second read of the key column when it sizes pass B's regions exactly (many-key tables: DBSCAN on 1e6 keys spends
 * 0.19 ms and 0.89 GB of its 1.55 ms there).  The factorisation has every row's id in registers when it writes key_id; counting there is
 * free.  `bins` is DEVICE memory of TAD_KEY_HIST_BYTES bytes supplied by the caller; the other fields are filled in by tad_factorize_hist
 * and checked by tad_run against its own plan — a histogram that does not belong to the batch (other row count, key count, sides) or that
 * the job cannot use (a time-window filter drops rows the histogram counted; a small batch has no pass A) is ignored.  A histogram of the right
 * shape whose COUNTS are another batch's (a stale one) costs an attempt, never memory or rows: pass B writes nothing past a region, reports the
 * region it found full, and the job is redone with pass A's own count (tad_stats.stage0_attempts).  The counts must be those tad_factorize_hist
 * wrote: their sum is not checked against n_rows. */
#define TAD_KEY_HIST_BYTES ((uint64_t)256 * 16384 * 4)
typedef struct {
  uint64_t n_rows, num_keys;   /* the batch it was taken from */
  uint64_t chunk_rows;         /* rows per workgroup */
  uint32_t workgroups, nbins, shift, sides;
  uint32_t *bins;              /* DEVICE [workgroups][nbins]: rows of workgroup g whose key id >> shift == b */
} tad_key_hist;

/* One columnar batch of flow rows (the columns the SQL of :507-614 touches, after the host's
 * dictionary encoding).  All arrays have n_rows entries; memory says where they live.
 *
 * Narrow columns (tad_job.flags): every column below is 8 bytes wide by default.  The data a host holds is often narrower —
 * flowEndSeconds / flowStartSeconds are ClickHouse DateTime (UInt32, create_table.sh:34), dictionary codes and dense key ids fit
 * 32 bits — and Stage 0 is bound by the bytes it reads, so the engine reads such columns at their own width instead of asking the
 * host to widen them first:
 *   TAD_FLAG_KEY_U32:  key_id and key_id2 point to uint32_t[n_rows]; TAD_KEY_SKIP32 marks a row (side) that does not take part;
 *                      num_keys must be < 2^32 - 1 (else TAD_ERR_INVALID_ARGUMENT).
 *   TAD_FLAG_TIME_U32: flow_end_s and flow_start_s point to uint32_t[n_rows], unsigned epoch seconds, ZERO-extended
 *                      (4000000000, year 2096, is a valid time, not a negative one).
 * Either flag, both or neither; host or device memory; tad_run, tad_aggregate and tad_run_stream.  value stays UInt64, and
 * start_time / end_time, the lattice fields (t0, step) and every output (tad_result, tad_points, the stream state) stay 64-bit.
 * Host columns are staged at their own width.  Results are bit-identical to the same table passed in 8-byte columns.  The
 * vector loads of Stage 0 need 16-byte aligned columns whatever their width; a narrow column that is only 4-byte aligned is read
 * row by row, as an 8-byte column that is only 8-byte aligned is.  The struct below is unchanged (the pointers are typed for the
 * default); cast a narrow column's pointer.
 * A library older than these flags ignores them and would misread the columns: check tad_features() & TAD_FEATURE_NARROW_COLUMNS
 * before setting either flag (an older library does not export tad_features at all, so a cgo link or dlsym fails instead).
 * tad_shard_rows, tad_factorize and tad_widen_column do not take narrow columns: their outputs stay 8 bytes wide. */
typedef struct {
  uint64_t n_rows;
  const uint64_t *key_id;       /* dense id of the row's key, < num_keys, or TAD_KEY_SKIP */
  const uint64_t *key_id2;      /* optional (NULL): second key of the same row — pod mode's
                                   UNION ALL of inbound + outbound (:556-565) */
  const int64_t *flow_end_s;    /* flowEndSeconds, epoch seconds (DateTime) */
  const int64_t *flow_start_s;  /* optional (NULL): flowStartSeconds for the start_time filter */
  const uint64_t *value;        /* throughput (UInt64) — or any UInt64 column, e.g. octetDeltaCount */
  uint64_t num_keys;            /* size of the key dictionary (ids are 0..num_keys-1) */
  tad_mem memory;
  /* Optional time lattice: flow_end_s = t0 + step*bucket, bucket < n_buckets.  n_buckets == 0:
   * the engine derives (min, gcd of differences, max) itself with one extra pass over flow_end_s. */
  int64_t t0;
  int64_t step;
  uint64_t n_buckets;
  const tad_key_hist *key_hist; /* optional (NULL): tad_factorize_hist's by-product for THIS batch (ABI 12) */
} tad_columns;

/* Per-run counters and stage timings (for CompletedStages/TotalStages-style progress and bench). */
typedef struct {
  uint64_t rows_in;        /* n_rows */
  uint64_t rows_used;      /* rows that passed the filters (each key of a 2-key row counts) */
  uint64_t n_keys;         /* keys with >= 1 point */
  uint64_t n_points;       /* distinct (key, flowEndSeconds) points = P */
  uint64_t n_anomalies;    /* A (0 => caller writes the sentinel row, :395-420) */
  uint64_t keys_no_result; /* ARIMA keys that yield no rows (n<=3, x<=0, constant; :232-234,260-264) */
  uint64_t kalman_steps;   /* ARIMA: filter time-steps over all likelihood evaluations */
  uint64_t arima_fits;     /* ARIMA: number of (key,t) fits */
  uint64_t arima_nan_fits; /* ARIMA: fits whose prediction is not finite (the optimiser walked into a non-finite likelihood: Box-Cox
                              with a strongly negative lambda next to the 1e6 diffuse prior).  Python's abs(x - nan) > sigma is False,
                              so such a point is never an anomaly (anomaly_detection.py:306-307) — counted so that an operator can
                              tell voided fits from clean ones */
  double pts_mean;         /* mean and sum of squared deviations (M2) of the aggregated point values of */
  double pts_m2;           /* this shard: (n_points, mean, M2) triples Chan-merge across GPUs into the global
                              mean / sigma the multi-GPU host reports (telemetry; the reference has none) */
  int64_t t0, step;        /* the time lattice used.  stage0_path >= 4 (sparse tables) does not place rows on a lattice: there t0 is the
                              smallest flowEndSeconds, and step / n_buckets are the caller's hint or pass A's (min, max, gcd) estimate,
                              reported for information — rows are never rejected for being off it (the dense path does reject) */
  uint64_t n_buckets;
  float ms_meta;           /* lattice derivation pass */
  float ms_stage0;         /* Stage 0 after the lattice pass: v1 grid clear + k_scatter; v2 offsets +
                              k_partition + k_tile_aggregate */
  float ms_scatter;        /* the dominant Stage-0 kernel alone: k_scatter (v1) or k_partition (v2) */
  float ms_detect;         /* per-key sigma + detector + compaction */
  float ms_total;          /* device time of the whole run, HIP events on the engine stream */
  int32_t stage0_path;     /* 1 = direct atomic scatter, 2 = partition (sort-by-tile pass B) + LDS tiles, 3 = partition (write-combining pass B) + LDS tiles,
                              4 = sparse table: sort by (key, time) + rank grid (time proportional to the rows, not to keys x lattice),
                              (5 was the two-level partition of ABI 6: measured no faster than the single-level plan, removed)
                              6 = sparse table with skewed series lengths: as 4, then one job per length class of keys (<= 16, <= 64, ... points),
                                  rows merged back in key order (the K x longest-series rank grid would not fit the workspace),
                              7 = tad_aggregate on such a table: the sorted unique points are the result, no grid at all,
                              8 / 9 / 10 (ABI 9) = as 4 / 6 / 7 with the rows sorted through the key-block partition pass + one LDS sort per key sub-range
                                  instead of the LSD radix sort (big sparse tables: the columns are read once, 8-byte records move through HBM once) */
  int32_t stage0_attempts; /* times Stage 0 ran before it settled: 1 normally; more after a wrong lattice hint, a sampled lattice or
                              a sampled histogram that proved too optimistic (every fallback is exact), an overflow-list fallback */
  int32_t hist_sampled;    /* 1: pass B's regions were sized from a SAMPLE of the key column (1/16 of pass A's reads); 2 (ABI 12): from the
                              caller's tad_key_hist (exact; pass A only sampled the time lattice); 0: from pass A's own exact histogram */
  int32_t host_syncs;      /* host synchronisations of the attempt that produced the result: 3 = lattice derivation, row count, result;
                              2 with a lattice hint (or an empty batch) */
  int32_t job_context;     /* ABI 12: index of the job context (stream + workspace) that ran the job; 0 for a serial caller */
  int32_t arima_relaunches;/* ABI 12: times this job's ARIMA fit kernel was relaunched after its wavefronts had retired early to make room for
                              another job's whole-CU workgroups (pass B / pass C need 1024 threads and up to 156 KB of LDS per workgroup and
                              cannot be placed beside the fit's long-lived wavefronts); 0 when the job ran alone.  Results do not depend on it */
} tad_stats;

/* Anomalous points only (anomaly_detection.py:394), ordered by (key_id, flow_end_s).
 * Columns = what the mode-independent part of a tadetector row needs (create_table.sh:363-384):
 * flowEndSeconds, throughputStandardDeviation, algoCalc, throughput; the host expands key_id
 * back into the mode's string columns and adds aggType / algoType / id / anomaly="true". */
typedef struct {
  uint64_t n_rows;         /* rows in the arrays below: stats.n_anomalies, or stats.n_points with
                              TAD_FLAG_EMIT_ALL_POINTS */
  uint64_t *key_id;
  int64_t *flow_end_s;
  double *throughput;      /* float(x): correctly rounded uint64 -> double (:161) */
  double *algo_calc;       /* EWMA value / ARIMA prediction / 0.0 for DBSCAN (:312-322) */
  double *stddev;          /* the key's stddev_samp (:674-684) */
  uint8_t *anomaly;        /* NULL unless TAD_FLAG_EMIT_ALL_POINTS: verdict per emitted point */
  tad_mem memory;          /* where the arrays live (same as the request's out_memory) */
  tad_stats stats;
  char id[64];
} tad_result;

/* ---- engine life cycle ---- */
int tad_abi_version(void);
/* TAD_FEATURE_* bits this library understands; needs no device */
int tad_features(void);
int tad_engine_create(const tad_engine_opts *opts, tad_engine **out);
void tad_engine_destroy(tad_engine *e);
/* Replace the engine's plan overrides (NULL = all zero); serialised with the jobs, takes effect with the next one. */
int tad_engine_set_plan(tad_engine *e, const tad_plan *plan);
/* Thread-safe; the returned string is owned by the engine (or static when e == NULL). */
const char *tad_last_error(tad_engine *e);

/* ---- the job: replaces the SparkApplication run (anomaly_detection.py:647-710) ----
 * Callable from several OS threads (controller.go:199-201 runs 4 workers): each call takes one of the engine's job contexts and runs
 * on that context's stream, so up to max_jobs_in_flight jobs overlap on the GPU (a short EWMA job does not queue behind a long ARIMA
 * job: ARIMA jobs run on a low-priority stream); callers beyond that wait for a context.  Results are bit-identical to a serial run
 * (contexts share no buffers).  out_memory selects host or device result arrays. */
int tad_run(tad_engine *e, const tad_job *job, const tad_columns *cols, tad_mem out_memory,
            tad_result **out);
void tad_result_free(tad_engine *e, tad_result *r);
/* ---- Stage 0 alone: the GROUP BY the reference pushes into ClickHouse (anomaly_detection.py:507-614) ----
 * Aggregated points ordered by (key_id, flow_end_s); value keeps the full UInt64 (sum wraps, max unsigned).
 * Used by row-sharded multi-GPU ingest: every GPU pre-aggregates its slice of the rows, the partial points travel to
 * the key owners (one all-to-all), and tad_run over the partials with the same value_op gives bit-identical
 * aggregates (integer add / max are associative).  job->algo and the detector parameters are ignored. */
typedef struct {
  uint64_t n_points;
  uint64_t *key_id;
  int64_t *flow_end_s;
  uint64_t *value;
  tad_mem memory;
  tad_stats stats;       /* rows_in, rows_used, n_keys, n_points, lattice, stage timings */
} tad_points;
int tad_aggregate(tad_engine *e, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_points **out);
void tad_points_free(tad_engine *e, tad_points *p);

/* ---- row-sharded ingest: bucket rows by the owner of their key for ONE all-to-all(v) ----
 * The reference has no such call: Spark's shuffle (anomaly_detection.py:664-684, groupby(key)) plays this role.  With G
 * GPUs, key k is owned by rank k mod G under the local id k / G.  tad_shard_rows writes the rows of `cols` grouped by
 * destination rank — destination 0's rows first — with LOCAL key ids, into three DEVICE arrays of cols->n_rows elements
 * each, and the rows per destination into counts[world] (HOST): the send splits of the all-to-all(v).  Rows whose key is
 * TAD_KEY_SKIP are dropped.  cols->memory must be TAD_MEM_DEVICE; key_id2 / flow_start_s must be NULL (pre-aggregate pod-mode
 * tables with tad_aggregate first: its points have one key).  The order of rows inside a destination is unspecified
 * (Stage 0 aggregates with commutative operators).  1 <= world <= 1024. */
int tad_shard_rows(tad_engine *e, const tad_columns *cols, uint32_t world, uint64_t *out_key_id, int64_t *out_flow_end_s,
                   uint64_t *out_value, uint64_t *counts);

/* ---- ingest: the GROUP BY key tuples of the job factorised on the GPU (ABI 8) ----
 * The reference groups in ClickHouse over string / integer columns (anomaly_detection.py:52-137, 507-614); the engine wants dense
 * key ids.  The host evaluates the SQL's string predicates on the distinct values of each string column (keep masks) and hands the
 * rows' key TUPLES over as n_cols (<= 8) columns of 8-byte integers: dictionary codes of the string columns, ports, protocol,
 * flowStartSeconds.  Out: key_id[i] = dense id of row i's tuple, ids in order of FIRST APPEARANCE (what pandas.factorize gives:
 * the GPU path and the host path of theia_amd/anomaly_detection.py:prepare_columns produce identical ids and key tables),
 * TAD_KEY_SKIP where keep[i] == 0; first_row[k] (k < first_row_cap) = the virtual row where key k first appears — the host reads
 * the key's column values there; *num_keys.
 * Pod mode (the UNION ALL of the inbound and the outbound view, :556-565) passes a second tuple per row (cols_b / keep_b, ids into
 * key_id2): ids are assigned over the virtual rows [side a: 0 .. n) ++ [side b: n .. 2n) and the side is part of the tuple.
 * n_rows * sides must be < 2^32 - 1.  All arrays (inputs and outputs) live in kc->memory. */
typedef struct {
  uint64_t n_rows;
  int32_t n_cols;                /* 1..8 */
  const int64_t *const *cols_a;  /* n_cols pointers to n_rows values each */
  const uint8_t *keep_a;         /* NULL = every row */
  const int64_t *const *cols_b;  /* NULL = one tuple per row */
  const uint8_t *keep_b;
  tad_mem memory;
} tad_key_columns;
int tad_factorize(tad_engine *e, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2, uint64_t *first_row,
                  uint64_t first_row_cap, uint64_t *num_keys);
/* ... and the same with the key-bin histogram of the ids as a by-product (tad_key_hist above): hist->bins must point to TAD_KEY_HIST_BYTES
 * bytes of DEVICE memory (whatever kc->memory is); the other fields are outputs.  hist->n_rows == 0 afterwards: no histogram (empty batch,
 * or more than 2^32 - 1 row slots). */
int tad_factorize_hist(tad_engine *e, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2, uint64_t *first_row,
                       uint64_t first_row_cap, uint64_t *num_keys, tad_key_hist *hist);

/* ---- ingest, one step earlier (ABI 10): an Arrow string column -> dictionary codes on the GPU ----
 * ClickHouse delivers the job's GROUP BY columns (sourcePodName, destinationPodName, pod labels, namespaces, destinationIP,
 * destinationServicePortName: anomaly_detection.py:52-137, 507-614) as strings; tad_factorize above wants integer columns.  The host's
 * dictionary encode (theia_amd/clickhouse.py:query_columns) was the slowest stage of a 1e8-row job.  In: one column in Arrow's layout —
 * n_rows + 1 offsets (int32 for `string`, int64 for `large_string`; pass the pointer already advanced by a sliced array's offset) into
 * `data`, an optional validity bitmap (a null row encodes like the empty string, which is what the host path did).  Out: codes[i] = id of
 * row i's string, ids in order of FIRST APPEARANCE (what Arrow's dictionary_encode and pandas.factorize give: same codes and
 * dictionaries as the host path); first_row[k] (k < first_row_cap) = the row where value k first appears — the host reads the
 * dictionary's strings there; *num_values.  n_rows < 2^32 - 1.  All arrays live in col->memory.  Offsets that decrease or point beyond
 * data_bytes are TAD_ERR_INVALID_ARGUMENT (checked on the device while the rows are read). */
typedef struct {
  uint64_t n_rows;
  const void *offsets;        /* n_rows + 1 */
  int32_t offset_bits;        /* 32 or 64 */
  const uint8_t *data;
  uint64_t data_bytes;        /* bytes behind `data` that offsets may address */
  const uint8_t *validity;    /* NULL = no nulls; else bit (validity_offset + i) of the bitmap is row i */
  uint64_t validity_offset;
  tad_mem memory;
} tad_string_column;
int tad_encode_strings(tad_engine *e, const tad_string_column *col, int64_t *codes, uint64_t *first_row, uint64_t first_row_cap,
                       uint64_t *num_values);

/* ---- ingest, columnar (ABI 12): Arrow record batches in host memory -> the 8-byte device columns of tad_factorize / tad_run ----
 * ClickHouse's HTTP interface (the reference's JDBC URL points at it, anomaly_detection.py:730-731) streams the raw rows as Arrow record
 * batches; with `toLowCardinality(col)` and output_format_arrow_low_cardinality_as_dictionary = 1 the string columns arrive as Arrow
 * DICTIONARY arrays, a dictionary per batch.  The host maps each batch's dictionary (its distinct values only) into the column's job-wide
 * one and evaluates the SQL's string predicates (anomaly_detection.py:507-614) on the distinct values; the rows are touched on the GPU:
 * tad_widen_column: dst[i] = table ? table[src[i]] : src[i], for i < n.  src holds n integers of src_bits (8 / 16 / 32 / 64) bits, sign-extended
 *   when src_signed, in HOST (staged by the call) or DEVICE memory; table (int64[table_len], DEVICE) and dst (int64[n], DEVICE).  Covers the
 *   dictionary indices of a batch (table = the batch's remap), UInt32 DateTime and UInt16 port columns (table NULL) and gathers of a device
 *   column at the rows tad_factorize reports in first_row (src = first_row, table = the column).  An index outside the table is
 *   TAD_ERR_INVALID_ARGUMENT.
 * tad_mask_rows: keep[i] = AND over t < n_terms of (masks[t][codes[t][i]] != 0), ANDed into the previous keep[i] when combine != 0.  codes[t]
 *   (int64[n]), masks[t] (uint8[mask_len[t]]) and keep (uint8[n]) are DEVICE memory; the pointer arrays themselves are host memory.  n_terms <= 8.
 * tad_host_alloc / tad_host_free: page-locked host memory (a reader receives the HTTP body straight into it; copies from it run at PCIe rate). */
int tad_widen_column(tad_engine *e, const void *src, int32_t src_bits, int32_t src_signed, tad_mem src_memory, uint64_t n, const int64_t *table,
                     uint64_t table_len, int64_t *dst);
int tad_mask_rows(tad_engine *e, uint64_t n, int32_t n_terms, const int64_t *const *codes, const uint8_t *const *masks, const uint64_t *mask_len,
                  int32_t combine, uint8_t *keep);
int tad_host_alloc(tad_engine *e, uint64_t bytes, void **ptr);
int tad_host_free(tad_engine *e, void *ptr);

/* ---- streaming EWMA: per-key running state kept in HBM between batches ----
 * The batch job re-reads the whole window and judges every point against the stddev_samp of the WHOLE series
 * (anomaly_detection.py:664-684, 168-212).  A long-running detector appends: tad_state holds, per key, Spark's streaming
 * moments (n, avg, m2 — the same update as the batch job), the last EWMA value and the last
 * flowEndSeconds seen.  tad_run_stream aggregates ONE new batch (Stage 0 as in tad_run), continues both recurrences over
 * the key's new points in time order and emits the points with |x - ewma| > stddev_samp(points seen so far, this one
 * included) — the running sigma, the only one an append-only detector can know.  After the last batch the state equals
 * what the batch job computes over the concatenated table bit for bit (same operations in the same order): n, avg, m2
 * give its stddev_samp, ewma its last EWMA value.  A row not newer than its key's last_t is rejected
 * (TAD_ERR_INVALID_ARGUMENT) and the state is left untouched.  job->algo must be TAD_ALGO_EWMA (or TAD_ALGO_DBSCAN on a state
 * with history, TAD_ALGO_ARIMA on a state with a series, below), and cols->num_keys must
 * EQUAL the num_keys the state holds (a batch addresses the state's whole key space; keys without rows in the batch keep
 * their state) — anything else is TAD_ERR_INVALID_ARGUMENT.
 * ABI 13: a batch takes the Stage 0 rule of tad_run (tad_plan.sparse / sparse_sort / stage0 included), so second-resolution
 * flowEndSeconds and a big key space are fine: a sparse batch (tad_stats.stage0_path 4 or 8) sorts its rows by (key, time)
 * and walks the sorted points per key — no K x span grid, no length classes.  Its cost follows the batch's rows plus about
 * 82 B of device traffic per state key; one key's serial chain is at most the batch's span in seconds.
 * tad_state_resize (ABI 13) grows the key space (a host that numbers keys in order of first appearance appends new ids):
 * new_num_keys >= num_keys, the added keys are unseen; smaller is TAD_ERR_INVALID_ARGUMENT; if allocation fails the state
 * is unchanged.  tad_state_import (ABI 13) is the inverse of tad_state_export: HOST arrays of num_keys entries each, none
 * NULL; a key with n == 0 is stored as unseen (all zeros), any other as seen — a state survives a restart of the host. */
typedef struct tad_state tad_state;
int tad_state_create(tad_engine *e, uint64_t num_keys, tad_state **out);
void tad_state_destroy(tad_engine *e, tad_state *s);
/* copies the state to HOST arrays of num_keys entries each (any may be NULL) */
int tad_state_export(tad_engine *e, const tad_state *s, uint32_t *n, double *avg, double *m2, double *ewma, int64_t *last_t);
int tad_state_resize(tad_engine *e, tad_state *s, uint64_t new_num_keys);
int tad_state_import(tad_engine *e, tad_state *s, const uint32_t *n, const double *avg, const double *m2, const double *ewma,
                     const int64_t *last_t);
int tad_run_stream(tad_engine *e, tad_state *s, const tad_job *job, const tad_columns *cols, tad_mem out_memory,
                   tad_result **out);

/* ---- streaming DBSCAN: a state WITH HISTORY (TAD_FEATURE_STREAM_DBSCAN; check tad_features() before calling these) ----
 * tad_state_create_ex(e, num_keys, TAD_STATE_HISTORY, &s) makes a state that keeps, on top of (n, avg, m2, ewma, last_t), every
 * aggregated point value it has seen, sorted ascending per key, in HBM.  flags 0 is tad_state_create.
 * tad_run_stream with job->algo == TAD_ALGO_DBSCAN on a history state, for one batch:
 *   1. aggregates the batch with Stage 0 exactly as an EWMA batch does (dense grid or sparse sort, tad_run's rule and plan overrides);
 *   2. advances the moments and last_t exactly as an EWMA batch does (a row not newer than its key's last_t fails the batch);
 *   3. merges the batch's new point values into the history and judges ONLY the batch's new points.
 * The rows of batch b are exactly the rows tad_run(DBSCAN), run with the same job parameters on the concatenation of batches 1..b,
 * emits for the points of batch b: key_id, flow_end_s, throughput, algo_calc = 0.0 and stddev, in the same order, bit for bit.  stddev
 * is the key's stddev_samp over everything seen through batch b (from the post-batch moments).  With TAD_FLAG_EMIT_ALL_POINTS the rows
 * are all of batch b's points with their verdict in `anomaly`.  DBSCAN verdicts depend only on the multiset of a key's values, which is
 * why this form is exact where the EWMA stream has to use a running sigma.  Consequences:
 *   - every point of a key with fewer than min_samples points so far is noise, as in the batch job;
 *   - dbscan_eps and dbscan_min_samples may differ from batch to batch: each batch is judged with its own, against the raw values;
 *   - points judged in earlier batches are not judged again.  A point can stop being noise once later points arrive; the stream
 *     reports each point once, when it arrives.
 * An EWMA batch on a history state appends to the history too; its rows and moments are those of the same batch on a plain state.
 * DBSCAN on a plain state is TAD_ERR_INVALID_ARGUMENT (state unchanged); ARIMA needs a state with a series (below); DROP is
 * refused here and streams through tad_drop_stream (further below).
 * Invariant: after every successful call the history of key k holds n[k] values; a failed batch (late row, key out of range, out of
 * memory) leaves the history unchanged as well as the state.  A batch never evicts: the history grows with the points seen (8 bytes
 * each, twice over: a batch merges into a second copy), and tad_state_history_points is how a caller watches it; a state that also has
 * a series is bounded by tad_state_trim (below).  A batch costs an
 * EWMA stream batch, plus a rewrite of the history (about 16 B per history point), plus the sort and verdicts of its new points.
 * tad_state_resize gives the added keys empty histories.  tad_state_export / tad_state_import / tad_state_destroy are unchanged. */
#define TAD_STATE_HISTORY 1u           /* keep every key's aggregated point values (sorted) */
int tad_state_create_ex(tad_engine *e, uint64_t num_keys, uint32_t flags, tad_state **out);   /* flags 0 == tad_state_create */
/* total values in the history (0 for a plain state) */
int tad_state_history_points(tad_engine *e, const tad_state *s, uint64_t *n_points);
/* HOST arrays: len[num_keys] and values[n_points], ascending per key, keys in order */
int tad_state_export_history(tad_engine *e, const tad_state *s, uint64_t *len, uint64_t *values);
/* the inverse of tad_state_export_history, after tad_state_import of the moments: TAD_ERR_INVALID_ARGUMENT with the state unchanged
 * unless the state has history, len[k] == n[k] of the state for every k, and every key's values are ascending */
int tad_state_import_history(tad_engine *e, tad_state *s, const uint64_t *len, const uint64_t *values);

/* ---- streaming ARIMA: a state WITH A SERIES (TAD_FEATURE_STREAM_ARIMA; check tad_features() before calling these) ----
 * tad_state_create_ex(e, num_keys, TAD_STATE_SERIES, &s) makes a state that keeps every key's aggregated point values IN TIME ORDER,
 * in HBM, double-buffered with the moments: the series becomes current only when a batch succeeds.  TAD_STATE_HISTORY | TAD_STATE_SERIES
 * (flags 3) keeps both, and every batch appends to both.  Unknown flag bits are TAD_ERR_INVALID_ARGUMENT.
 * tad_run_stream with job->algo == TAD_ALGO_ARIMA on a series state, for one batch:
 *   1. aggregates the batch with Stage 0 exactly as an EWMA batch does (dense grid or sparse sort, tad_run's rule and plan overrides);
 *   2. advances the moments and last_t exactly as an EWMA batch does (a late row fails the batch: state, history and series unchanged);
 *   3. appends the batch's new points to each key's series;
 *   4. for every key with new points and a result: lambda and the Box-Cox transform over the key's whole series, and the predictions of
 *      the NEW points only.  A new point at position p < 3 gets inv_boxcox(y_p); one at p >= 3 the walk-forward fit on y[0..p).  The
 *      verdict is |x - pred| > stddev, stddev the key's stddev_samp from the post-batch moments;
 *   5. emits the batch's new points in (key, time) order: throughput, algo_calc = the prediction, stddev (with TAD_FLAG_EMIT_ALL_POINTS
 *      every new point of a key that has a result, with its verdict in `anomaly`).
 * The rows of batch b are exactly the rows tad_run(ARIMA), run with the same job parameters on the concatenation of batches 1..b,
 * emits for the points of batch b, bit for bit and in the same order, whatever Stage-0 path either side takes.  Consequences:
 *   - a key with <= 3 points so far has no result, so its points are never reported; the same holds for a key whose series is
 *     constant, contains a value <= 0, or whose Box-Cox fit fails;
 *   - points reported in earlier batches are not revised (their predictions and lambda are those of their own batch);
 *   - arima_maxiter may differ from batch to batch.
 * The batch's stats: arima_fits = the fits this batch ran (new points at p >= 3 of keys with a result), keys_no_result = keys with new
 * points that have no result; kalman_steps, arima_nan_fits and arima_relaunches as in tad_run.  A batch costs an EWMA stream batch, a
 * rewrite of the series (about 16 B per series point), the Box-Cox fit over the touched keys' series and one ARIMA fit per new point:
 * the fits of earlier points are never run again.  Its workspace follows the touched series (packed), not keys x longest series.
 * An EWMA or DBSCAN batch on a series state appends to the series too; its rows are those of the same batch without a series.
 * ARIMA on a plain or history-only state and DROP on any state are TAD_ERR_INVALID_ARGUMENT (state unchanged; DROP: tad_drop_stream).
 * Invariant: after every successful call the series of key k holds n[k] values.  tad_state_resize gives the added keys empty series. */
#define TAD_STATE_SERIES 2u            /* keep every key's aggregated point values (time order) */
#define TAD_STATE_TIMES 8u             /* with TAD_STATE_SERIES only: keep every series point's flowEndSeconds too (tad_state_trim, below) */
/* total values in the series (0 for a state without a series) */
int tad_state_series_points(tad_engine *e, const tad_state *s, uint64_t *n_points);
/* HOST arrays: len[num_keys] and values[n_points], each key's values in time order, keys in order */
int tad_state_export_series(tad_engine *e, const tad_state *s, uint64_t *len, uint64_t *values);
/* the inverse of tad_state_export_series, after tad_state_import of the moments: TAD_ERR_INVALID_ARGUMENT with the state unchanged
 * unless the state has a series and len[k] == n[k] of the state for every k */
int tad_state_import_series(tad_engine *e, tad_state *s, const uint64_t *len, const uint64_t *values);

/* ---- trimming a streaming state (TAD_FEATURE_STREAM_TRIM; check tad_features() before calling these) ----
 * A long-running detector judges against a window, as the batch job does with start_time / end_time: "the last 24 h" or "the last N
 * points of each key".  TAD_STATE_TIMES (valid only with TAD_STATE_SERIES; without it TAD_ERR_INVALID_ARGUMENT, as is bit 4u, which
 * stays unknown) makes the state keep
 * every series point's flowEndSeconds beside its value (int64, same offsets, double-buffered and grown like the series: 8 more bytes
 * per point, twice over).  States without it are unchanged.
 * tad_state_trim keeps, of every key's series in time order:
 *   - with keep_from_t != 0, only the points with flow_end_s >= keep_from_t (needs TAD_STATE_TIMES, else TAD_ERR_INVALID_ARGUMENT);
 *   - with keep_points != 0, only the newest keep_points of those;
 *   - both 0: a no-op (TAD_OK).  *dropped (may be NULL) = the points removed.
 * Contract: afterwards the state is bit for bit the state a fresh state with the same flags and num_keys holds after tad_run_stream of
 * only the retained points, with EWMA parameter ewma_alpha (0 -> 0.5, as in tad_job):
 *   - a key that lost points has n, avg, m2 and ewma replayed over its retained values in time order from the zero state, with the very
 *     step of the stream batches; last_t = its newest retained point's time; a key that lost all of them is unseen (all zeros);
 *   - a key that lost nothing keeps its state as it is, so the contract holds when its batches used ewma_alpha too;
 *   - the series (and its times) is every key's retained suffix; the history, if the state has one, the sorted multiset of the retained
 *     values (the history must be the series' values sorted, which every batch keeps; an import that breaks this voids the contract).
 * Consequences: a DBSCAN or ARIMA batch after a trim emits exactly what tad_run emits over the retained points and the later batches for the
 * batch's new points; an EWMA batch emits exactly what the fresh state would.  A trim needs a series (a history alone does not know
 * which values are oldest): on a plain or history-only state it is TAD_ERR_INVALID_ARGUMENT.  It writes only the candidate copies and
 * swaps them in when everything succeeded: any failure, allocation included, leaves state, history, series and times as they were.
 * An arena left below a quarter of its capacity is allocated anew at twice its length, so the memory shrinks.  A trim costs about 16 B
 * of traffic per series point (values and times), 16 B per history point plus the sort of the evicted values, and a serial replay per
 * key that lost points, as long as the key's retained series.  Lock order: the state, then a job context, as a batch.
 * tad_state_export_times / tad_state_import_times: HOST arrays of tad_state_series_points entries, in the order of
 * tad_state_export_series.  Import after tad_state_import and tad_state_import_series (which leaves a times state refusing batches,
 * trims and exports of the times until its times are imported): TAD_ERR_INVALID_ARGUMENT with the state unchanged unless the state has
 * times, every key's times ascend strictly and every non-empty key's last time equals its last_t.
 * tad_state_bytes: the device bytes the state holds — both moment blocks, the offsets and every arena at its capacity (the state's own
 * memory only: the job contexts' workspace, such as the history scratch arena of tad_state_merge below, is not in it). */
int tad_state_trim(tad_engine *e, tad_state *s, uint64_t keep_points, int64_t keep_from_t, double ewma_alpha, uint64_t *dropped);
int tad_state_bytes(tad_engine *e, const tad_state *s, uint64_t *bytes);
int tad_state_export_times(tad_engine *e, const tad_state *s, int64_t *t);
int tad_state_import_times(tad_engine *e, tad_state *s, const int64_t *t);

/* ---- the window's batch verdicts from the state alone (TAD_FEATURE_STATE_RUN; check tad_features() before calling this) ----
 * The batch job judges every point of the window against the window as a whole (anomaly_detection.py:647-710).  The stream cannot give
 * that answer: its EWMA verdicts use the running sigma, and its DBSCAN and ARIMA batches report each point once, when it arrives.  A
 * state created with TAD_STATE_SERIES | TAD_STATE_TIMES already holds what Stage 0 would produce for the window — every key's aggregated
 * points in time order with their flowEndSeconds, and moments (n, avg, m2) that are the batch job's bit for bit; with TAD_STATE_HISTORY
 * each key's values sorted as well — so "stream the batches, trim, ask for the window's verdicts" needs no raw row read twice.
 * Contract: let W be the table with one row per series point the state holds, (key, flow_end_s, value).  tad_run_state returns exactly
 * the rows tad_run returns for W with the same algo, detector parameters and TAD_FLAG_EMIT_ALL_POINTS (any value op: a single-row group
 * aggregates to itself): key_id, flow_end_s, throughput, algo_calc, stddev (and anomaly with the flag), in the same (key, time) order,
 * bit for bit, whatever Stage-0 path tad_run takes for W.  The state is read only: after the call, successful or not, moments, history,
 * series and times are unchanged.
 * What the state must hold (anything else is TAD_ERR_INVALID_ARGUMENT): EWMA and ARIMA need TAD_STATE_SERIES | TAD_STATE_TIMES, DBSCAN
 * needs TAD_STATE_HISTORY as well; a state whose times are stale (series imported, times not yet) is refused, as a batch is.
 * Fields of tad_job that are honoured: algo, ewma_alpha, dbscan_eps, dbscan_min_samples, arima_maxiter, flags & TAD_FLAG_EMIT_ALL_POINTS
 * and id; zero means the default, as in tad_run.  agg_flow and value_op are ignored: the points are already aggregated.  Refused with
 * TAD_ERR_INVALID_ARGUMENT: start_time or end_time non-zero (the window is what the state holds; narrow it with tad_state_trim),
 * TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32 (there are no input columns), and TAD_ALGO_DROP, whose window call is tad_drop_state.
 * The contract rests on the state's invariants — the moments are those of the series, the history is the series' values sorted — which
 * every batch and every trim keep; an import that breaks them voids the contract.
 *   - EWMA: stddev = n >= 2 ? sqrt(m2 / (n - 1.0)) : 0.0 from the state's moments; the EWMA value is replayed from 0 over the key's series
 *     with the job's alpha (the state's stored ewma is not used: it may come from another alpha); verdict n >= 2 && |x - e| > stddev.
 *   - DBSCAN: every series point is judged against its key's history; algo_calc = 0.0, stddev as above.
 *   - ARIMA: lambda and Box-Cox over the whole series, every position predicted; keys with no result emit nothing.
 * tad_stats of the result: rows_in = rows_used = n_points = the series points; n_keys = keys with at least one point; n_anomalies; for
 * ARIMA keys_no_result, arima_fits, kalman_steps, arima_nan_fits and arima_relaunches as tad_run over W reports them; pts_mean / pts_m2
 * merged from the per-key moments as tad_run merges them; t0 = the smallest retained time, step = n_buckets = 0; stage0_path =
 * stage0_attempts = 0 and ms_meta = ms_stage0 = ms_scatter = 0 (no Stage 0 ran); ms_detect, ms_total, job_context.  An empty state gives
 * TAD_OK with zero rows.  A call costs one walk of the series (two without TAD_FLAG_EMIT_ALL_POINTS for EWMA: count, then emit) plus
 * the rows; DBSCAN adds the verdicts' binary searches in the history, ARIMA runs the job's fits.
 * tad_plan.ewma_emit / ewma_emit_rows choose and size its staged EWMA emit as they do tad_run's (tests, A/B measurements).
 * Lock order: the state, then a job context, as a batch and a trim; calls on one state are serial, tad_job_progress finds the job by id. */
int tad_run_state(tad_engine *e, tad_state *s, const tad_job *job, tad_mem out_memory, tad_result **out);

/* ---- a batch placed by time: late rows, re-sent rows, rows of a group split over batches (TAD_FEATURE_STATE_MERGE; check tad_features()
 * before calling this) ----
 * tad_run_stream appends: one row not newer than its key's last flowEndSeconds fails the whole batch.  Flow records do not arrive in that
 * order (the flows table is ordered and expired by timeInserted, the exporters lag by node), and the only remedy was to rebuild the state
 * from the window's raw rows.  A state created with TAD_STATE_SERIES | TAD_STATE_TIMES holds what it needs to repair itself: every key's
 * aggregated points in time order with their flowEndSeconds; Stage 0's operators (sum mod 2^64, unsigned max) are associative and
 * commutative.  tad_state_merge aggregates the batch with Stage 0 exactly as a stream batch does and places its points BY TIME.
 * Contract: let W be the table with one row per series point the state holds, (key, flow_end_s, value) — tad_run_state's W — and B the
 * batch's rows after the job's filters, without the points whose flow_end_s < keep_from_t when keep_from_t != 0.  After a successful call
 * the state — n, avg, m2, ewma, last_t, series, times, and the history if it has one — is bit for bit the state a fresh state of the same
 * flags and num_keys holds after ONE tad_run_stream EWMA batch over the rows W ++ B with the job's value op and ewma_alpha (0 -> 0.5).
 * Consequences:
 *   - cut a table into batches anyhow, in any row order, and feed every batch through tad_state_merge with the same value op: the state
 *     is the one a single batch over the whole table leaves, so tad_run_state afterwards returns exactly tad_run over the whole table
 *     (rows, order, bits) for EWMA, DBSCAN (history states) and ARIMA;
 *   - a point at a time the key already holds is combined with Stage 0's own operator, sum wrapping mod 2^64 or unsigned max.  The state
 *     does not remember which op built it: use the same value op for every batch of a state (there is nothing to check it against);
 *   - re-sending a batch is idempotent under max and doubles the values under sum: it is a merge, not a de-duplication (a re-read that
 *     must not double goes through tad_state_replace, below);
 *   - tad_run_stream batches and merges mix freely on one state: the invariants (the moments are the series', the history is the series'
 *     values sorted, times ascend strictly, last_t is the newest time) hold after every merge, so a later DBSCAN / ARIMA stream batch
 *     emits what tad_run over the merged window plus the batch emits for the batch's points.  tad_run_stream itself still refuses late rows;
 *   - the call emits no rows: the verdicts of a merged window come from tad_run_state.  job->algo and the detector parameters other than
 *     ewma_alpha are ignored;
 *   - moments: a key with at least one inserted or combined point is replayed from the zero state over its merged series in time order
 *     with the very step of the stream batches; a key that only had points appended continues from its stored state exactly as a stream
 *     batch does (so, as for tad_state_trim, the contract holds for it when its earlier batches used the same ewma_alpha); an untouched
 *     key is copied.
 * Fields of tad_job that are honoured: agg_flow / value_op, start_time / end_time (Stage 0's row filter), ewma_alpha, TAD_FLAG_KEY_U32 /
 * TAD_FLAG_TIME_U32 and id (tad_job_progress).  TAD_FLAG_EMIT_ALL_POINTS is TAD_ERR_INVALID_ARGUMENT (there are no rows).  The batch takes
 * Stage 0 as a stream batch does: dense grid or sparse sort, tad_plan overrides included, host or device columns; cols->num_keys must
 * equal the state's.  The state needs TAD_STATE_SERIES | TAD_STATE_TIMES: a plain, history-only or series-without-times state, a state
 * whose times are stale and ewma_alpha outside [0, 1] are TAD_ERR_INVALID_ARGUMENT.
 * Atomic: only the candidate copies (moments, offsets, arenas) and job-context workspace are written, and they become current together;
 * any failure — a key out of range (TAD_ERR_KEY_RANGE), allocation, a HIP error — leaves moments, history, series and times as they were.
 * An empty batch, or one whose points are all too old, is TAD_OK with the state untouched.  A batch without an inserted, combined or
 * too-old point takes the append path of a stream batch (keys_replayed == 0).  Otherwise a merge costs a rewrite of the series and times
 * (about 32 B per series point), for a history state the history rewritten once (twice when a point combined: the old values leave,
 * then the new ones enter), and a serial replay per key with an inserted or combined point, as long as its merged series.
 * The append path needs a batch without a too-old point as well: with keep_from_t set, ONE point under the cut sends an otherwise in-order
 * batch through the full rewrite.  Memory outside the state: a merge that combines a point on a history state passes the history through
 * a scratch arena of the job context that runs it — 8 B per history point, grow-only like all context workspace, kept by every context
 * that ever ran such a merge (at most max_jobs_in_flight of them) and NOT counted by tad_state_bytes.
 * Lock order: the state, then a job context, as a batch, a trim and tad_run_state. */
#define TAD_FEATURE_STATE_MERGE 32u   /* tad_state_merge: a batch placed by time — late rows, re-sent rows, rows of a group split over batches */
typedef struct {
  uint64_t rows_in;                  /* as tad_stats */
  uint64_t rows_used;
  uint64_t batch_points;             /* distinct (key, flowEndSeconds) points Stage 0 made of the batch, before keep_from_t */
  uint64_t points_too_old;           /* of those: flow_end_s < keep_from_t, dropped */
  uint64_t points_appended;          /* newer than everything their key held (what tad_run_stream would have taken) */
  uint64_t points_inserted;          /* a new time before the key's last_t */
  uint64_t points_combined;          /* a time the key already held: value = op(old, new) */
  uint64_t keys_touched;             /* keys with >= 1 appended / inserted / combined point */
  uint64_t keys_replayed;            /* of those: keys whose moments were replayed from the zero state (>= 1 inserted or combined point) */
  int32_t stage0_path;               /* as tad_stats */
  int32_t stage0_attempts;
  int32_t job_context;
  int32_t reserved;
  float ms_stage0;                   /* HIP events, as tad_stats */
  float ms_merge;                    /* everything after Stage 0 */
  float ms_total;
  float reserved1;
} tad_merge_stats;
int tad_state_merge(tad_engine *e, tad_state *s, const tad_job *job, const tad_columns *cols, int64_t keep_from_t,
                    tad_merge_stats *stats /* may be NULL */);

/* ---- a batch that replaces: re-read windows, retried polls, restarts (TAD_FEATURE_STATE_REPLACE; check tad_features() before calling
 * this) ----
 * A poller delivers at least once: it re-reads the last minutes because exporters lag by node, it re-reads after a restart, it retries
 * after a timeout.  Through tad_state_merge every such re-read doubles, under sum, each point it saw twice.  tad_state_replace says "for
 * these seconds, this batch is the truth": the poll loop becomes re-read [watermark - lag, now), replace, move the watermark, and is
 * idempotent by construction under both value ops.
 * Contract, a pure function of W.  Let W be the table with one row per series point the state holds, (key, flow_end_s, value) —
 * tad_run_state's W.  Let B be Stage 0's points of the batch: the job's filters and value op, exactly as tad_state_merge aggregates a
 * batch, without the points whose flow_end_s < keep_from_t when keep_from_t != 0.  Let R be empty without TAD_REPLACE_RANGE, and with it
 * R = {t : (from_t == 0 || t >= from_t) && (to_t == 0 || t < to_t)} — the half-open rule of tad_run_state_window; from_t = to_t = 0 is
 * every time.  Let W' = {w in W : time(w) not in R and (key, time)(w) not a point of B} ++ B.  After a successful call the state — n, avg,
 * m2, ewma, last_t, series, times, and the history if it has one — is bit for bit the state a fresh state of the same flags and num_keys
 * holds after ONE tad_run_stream EWMA batch over W' with ewma_alpha (0 -> 0.5).
 * Consequences:
 *   - the same call twice leaves the same bits: the second call replaces every point of B with itself and erases nothing;
 *   - a point of B at a time its key already holds takes B's value; the old value is never combined with it;
 *   - a key whose points all fall in R and that has none in B becomes an unseen key (all zeros, empty series);
 *   - the erase acts on EVERY key of the state, not only on the keys of the batch: R says the batch holds all rows of those seconds;
 *   - the value op only aggregates rows inside the batch (several rows of one (key, second)); it never meets a value of the state;
 *   - without TAD_REPLACE_RANGE nothing is erased: the call is a merge whose combined points take the new value;
 *   - replaces, merges, stream batches, trims and compacts mix freely on one state: the state's invariants hold after every replace, so
 *     tad_run_state afterwards returns exactly tad_run over W', and a later DBSCAN / ARIMA stream batch emits what tad_run over W' plus
 *     that batch emits for its points;
 *   - the call emits no rows; job->algo and the detector parameters other than ewma_alpha are ignored;
 *   - moments: a key with an inserted, replaced or erased point is replayed from the zero state over its new series in time order (an
 *     emptied key is left at the zero state, the bits of an unseen key); a key that only had points appended continues from its stored
 *     state; an untouched key is copied.
 * Arguments and refusals (TAD_ERR_INVALID_ARGUMENT with a message, state unchanged): everything tad_state_merge refuses — a state
 * without TAD_STATE_SERIES | TAD_STATE_TIMES, stale times, TAD_FLAG_EMIT_ALL_POINTS, ewma_alpha outside [0, 1], cols->num_keys other than
 * the state's, the column checks — and: unknown bits in flags; a non-zero from_t or to_t without TAD_REPLACE_RANGE; from_t > to_t with
 * both non-zero.  from_t == to_t non-zero is an empty R.  The honoured tad_job fields are tad_state_merge's.
 * Atomic like a merge: only the candidate copies and job-context workspace are written, and the candidates become current together;
 * any failure — a key out of range (TAD_ERR_KEY_RANGE), allocation, a HIP error — leaves the state as it was.
 * Two differences from tad_state_merge: an empty batch (no row, or no row that passes the filters, or every point too old) with a
 * non-empty R is not a no-op — it erases R; and the append path of a stream batch (keys_replayed == 0) needs a batch without a replaced,
 * inserted, too-old or erased point.  Otherwise a replace costs what a merge costs — a rewrite of the series and times, the history
 * rewritten once, twice when a point was replaced or erased, a serial replay per key with an inserted, replaced or erased point — plus,
 * with a range, two binary searches per key of the state and a second host round trip for the erased total.  After a
 * replace that erased, an arena left below a quarter of its capacity is allocated anew at twice its length, tad_state_trim's rule.
 * Memory outside the state: tad_state_merge's, and the packed values the history loses (16 B per replaced or erased point).
 * Lock order: the state, then a job context, as a merge. */
#define TAD_FEATURE_STATE_REPLACE 65536u /* tad_state_replace: a batch that replaces the points it names and, ranged, erases the seconds it covers */
#define TAD_REPLACE_RANGE 1u             /* erase every point of the state with from_t <= flow_end_s < to_t (0 = no bound) that the batch does not name */
typedef struct {
  uint64_t rows_in;                  /* as tad_stats */
  uint64_t rows_used;
  uint64_t batch_points;             /* distinct (key, flowEndSeconds) points Stage 0 made of the batch, before keep_from_t */
  uint64_t points_too_old;           /* of those: flow_end_s < keep_from_t, dropped */
  uint64_t points_appended;          /* newer than everything their key held before the call */
  uint64_t points_inserted;          /* a new time before the key's last_t */
  uint64_t points_replaced;          /* a time the key already held: value = the batch's */
  uint64_t points_erased;            /* points the state held inside R that the batch does not name: removed */
  uint64_t keys_emptied;             /* keys that held points before the call and hold none after it */
  uint64_t keys_touched;             /* keys whose moments changed: >= 1 appended / inserted / replaced / erased point */
  uint64_t keys_replayed;            /* of those: replayed from the zero state (>= 1 inserted, replaced or erased point) */
  int32_t stage0_path;               /* as tad_stats */
  int32_t stage0_attempts;
  int32_t job_context;
  int32_t reserved;
  float ms_stage0;                   /* HIP events, as tad_stats */
  float ms_replace;                  /* everything after Stage 0 */
  float ms_total;
  float reserved1;
} tad_replace_stats;
int tad_state_replace(tad_engine *e, tad_state *s, const tad_job *job, const tad_columns *cols, uint32_t flags, int64_t from_t, int64_t to_t,
                      int64_t keep_from_t, tad_replace_stats *stats /* may be NULL */);

/* ---- what a merge or a replace changed: the change report (TAD_FEATURE_STATE_ALERTS; check tad_features() before calling these) ----
 * tad_state_merge and tad_state_replace take rows in any order and any number of times, emit nothing and do not say which keys they
 * changed.  The *_changes forms are the same calls — the same batch, contract, atomicity, stats, refusals, lock order and append path —
 * and also fill a report.  A NULL report makes them tad_state_merge / tad_state_replace, which are these calls with a NULL report.
 * Contract: let W be the state's table of points before the call and W' the table after it, as in the two contracts above.  A point of
 * key k is CHANGED iff it is in exactly one of W and W', or in both with different values: appended and inserted points, the points a
 * range erased, and combined / replaced points whose stored value differs.  key_since[k] = the smallest flow_end_s of key k's changed
 * points, TAD_NO_CHANGE when it has none.  What does NOT change a key: a sum merge of value 0 at a held time, a max merge of a value not
 * above the held one, a replace by the held value — so the same replace twice reports keys_changed == 0 the second time, and a poll
 * loop that alerts on the report is idempotent, not only its state.  keys_changed <= stats.keys_touched always (a touched key may have
 * been rewritten with the bits it held).  An empty or all-too-old batch without a range is TAD_OK with every entry TAD_NO_CHANGE and the
 * counters 0.
 * The report's memory: key_since is int64[len] in host or device memory (memory), 8-byte aligned, len == the state's num_keys; or NULL
 * with len == 0 for the counters alone.  Refused (TAD_ERR_INVALID_ARGUMENT, state unchanged): len other than num_keys with an array, a
 * NULL array with a non-zero len, a misaligned array, a memory that is neither TAD_MEM_HOST nor TAD_MEM_DEVICE.  On any failure the
 * state is unchanged as without a report, the counters are 0 and the array's content is unspecified (a device array is written in
 * place while the call runs; a host array is staged in job-context workspace, 8 B per key, and copied out only on success).
 * Cost: one more lane-per-key fill before and one lane-per-key pass after the series kernel, which reduces the changed elements'
 * smallest time per wavefront (one 64-bit atomic minimum per 2048-element chunk with a changed element) — and nothing at all, not
 * even compiled into the kernels it runs, for a call with a NULL report.  No further host round trip: the counters ride on the
 * call's last copy. */
#define TAD_FEATURE_STATE_ALERTS 131072u /* tad_state_merge_changes / tad_state_replace_changes, tad_run_state_since / tad_drop_state_since */
#define TAD_NO_CHANGE INT64_MAX
typedef struct {
  int64_t *key_since;                /* out, int64[len]: the smallest flow_end_s at which key k's series changed; TAD_NO_CHANGE = unchanged.
                                        May be NULL with len == 0: counters only */
  uint64_t len;                      /* must equal the state's num_keys when key_since != NULL */
  tad_mem memory;                    /* host or device, any 8-byte aligned address */
  uint64_t keys_changed;             /* out: keys with key_since != TAD_NO_CHANGE */
  uint64_t points_changed;           /* out: points added + points removed + points whose value changed */
  int64_t min_t;                     /* out: smallest changed flow_end_s; 0 when points_changed == 0 */
  int64_t max_t;                     /* out: largest changed flow_end_s; 0 when points_changed == 0 */
} tad_changes;
int tad_state_merge_changes(tad_engine *e, tad_state *s, const tad_job *job, const tad_columns *cols, int64_t keep_from_t,
                            tad_merge_stats *stats /* may be NULL */, tad_changes *ch /* NULL: tad_state_merge */);
int tad_state_replace_changes(tad_engine *e, tad_state *s, const tad_job *job, const tad_columns *cols, uint32_t flags, int64_t from_t,
                              int64_t to_t, int64_t keep_from_t, tad_replace_stats *stats /* may be NULL */,
                              tad_changes *ch /* NULL: tad_state_replace */);

/* Judge the window, report from a time on (TAD_FEATURE_STATE_ALERTS as well).  tad_run_state_keys / tad_drop_state_keys return every row of
 * the window again at every call; after a merge or a replace only the points from each changed key's first changed time on are news.
 * tad_run_state_since (EWMA, DBSCAN, ARIMA) and tad_drop_state_since (DROP) judge the window exactly as the *_keys calls do and REPORT a
 * part of it.  The report window: from_t / to_t / keep_points are tad_run_state_window's window, key_keep tad_run_state_keys' mask (NULL:
 * every key); key_since is one int64 per key or NULL — a change report's array as it stands — and since_t one time for all keys (0 =
 * none); num_keys is the length of the arrays that are given and must equal the state's; key_memory is where both arrays live.
 * Contract: a point is REPORTED iff it lies in the window, its key is selected, (since_t == 0 || flow_end_s >= since_t) and (key_since ==
 * NULL || flow_end_s >= key_since[key]).  A key with key_since[k] == TAD_NO_CHANGE counts as NOT SELECTED: the effective mask is key_keep
 * AND (key_since != TAD_NO_CHANGE), such a key gets an empty window and costs nothing after the bounds.  The call returns exactly the
 * rows of tad_run_state_keys / tad_drop_state_keys with the same window and the effective mask, restricted to the reported points: the
 * same order, bit for bit, TAD_FLAG_EMIT_ALL_POINTS included.  Every selected key is still judged over its WHOLE window — EWMA's
 * recurrence and stddev, DBSCAN's neighbourhood, ARIMA's lambda and fits' histories, DROP's mean and std.  With no since at all (key_since
 * NULL, since_t 0) the call IS the *_keys call.  Read-only: the state is bit for bit what it was.  A changed key's points BEFORE its
 * first changed time may have changed verdict too (a late point moves the stddev of the whole key); they are not reported — the stream's
 * rule, "each point once, when it arrives"; the *_keys calls give the whole answer.
 * Refusals: the *_keys calls' (algorithm family, start_time / end_time, narrow-column flags, parameter ranges, what the state must
 * keep, stale times, from_t > to_t, an array in neither memory) plus: a NULL report window, num_keys other than the state's with an
 * array given, a key_since that is not 8-byte aligned.
 * tad_stats: rows_in, rows_used, n_points, n_keys and t0 are over the JUDGED points, as the *_keys calls report them; n_anomalies,
 * keys_no_result and the ARIMA counters cover the keys with at least one reported point, and arima_fits counts the fits actually run —
 * those of the reported points.  For tad_drop_state_since with a since pts_mean / pts_m2 are 0 (only the keys with a reported point get
 * their mean and std computed).  host_syncs: tad_run_state_window's — 2, and 3 when bounds, a key_keep or a key_since are set on a
 * non-empty state — plus one with a since for DBSCAN, ARIMA and DROP (the number of reported points is read before their block is
 * sized; not when the judged window is empty); EWMA needs none.
 * How: times ascend per key, so a key's reported points are a suffix of its view segment.  One lane per key finds the suffix's first
 * index by a lower bound over the view's times; EWMA walks every series as before and counts or emits from that index on; for the
 * others the suffixes are packed (key, time, value; 24 B per reported point of context workspace, plus about 40 B per key) and go to
 * the stream batches' detectors as the batch of new points. */
typedef struct {
  int64_t from_t;                    /* tad_run_state_window's window */
  int64_t to_t;
  uint64_t keep_points;
  const uint8_t *key_keep;           /* tad_run_state_keys' mask or NULL */
  const int64_t *key_since;          /* per key or NULL */
  int64_t since_t;                   /* 0 = none */
  uint64_t num_keys;                 /* length of the arrays that are given; must equal the state's */
  tad_mem key_memory;                /* of both arrays */
} tad_report_window;
int tad_run_state_since(tad_engine *e, tad_state *s, const tad_job *job, const tad_report_window *w, tad_mem out_memory, tad_result **out);
int tad_drop_state_since(tad_engine *e, tad_state *s, const tad_job *job, const tad_report_window *w, tad_mem out_memory, tad_result **out);

/* ---- a state judged in time buckets (TAD_FEATURE_STATE_BUCKETS; check tad_features() before calling this) ----
 * A state keeps every key's series at the resolution of flow_end_s, one second, and every read-only job above judges those per-second
 * points.  Throughput is looked at per interval (the reference's dashboards group by $__timeInterval(flowEndSeconds)); this call judges
 * the state at that resolution without the rows leaving the device: the report window of tad_run_state_since plus a bucket length, an
 * origin and the operation that folds a bucket's points.
 * Contract: let W' be the rows tad_run_state_keys judges for the same from_t / to_t / keep_points and key_keep — one row per point; the
 * window is applied FIRST, on the raw points, and keep_points counts points, not buckets.  Let W'' be W' with flow_end_s replaced by
 *     bucket_origin + bucket_s * floor((flow_end_s - bucket_origin) / bucket_s)
 * (FLOOR division: a time below the origin, below zero too, rounds down).  The call returns exactly the rows tad_run returns for W''
 * with value_op = bucket_op and the same algo, detector parameters and TAD_FLAG_EMIT_ALL_POINTS: the same (key, time) order, bit for bit.
 * The bucket's start stands in flow_end_s; a bucket cut by from_t / to_t / keep_points holds only the window's points.  bucket_s = 1
 * with bucket_origin = 0 therefore IS the *_keys call (through the bucket kernels).  Integer sums wrap mod 2^64 and maxima are unsigned,
 * as in Stage 0, so the fold does not depend on any order.  Read-only: whether the call succeeds or not, the state is bit for bit what
 * it was.  Domain of the time arithmetic: |flow_end_s| < 2^62 and bucket_s <= 2^40; outside it the bucket starts wrap (defined, and the
 * same on host and device: csrc/tad_bucket.h), they are no longer the mathematical floor.
 * The since rule (key_since / since_t as in tad_report_window): the threshold of key k is the larger of since_t and key_since[k]; a
 * BUCKET is reported iff its start >= the start of the threshold's bucket — so every bucket that holds a point at or after the
 * threshold is reported, whole.  TAD_NO_CHANGE deselects the key.  The rows are those of the same call without a since, restricted to
 * the reported buckets, bit for bit; every selected key is still judged over all its buckets.
 * Refusals: everything tad_run_state_since refuses, plus a NULL bucket window, bucket_s < 1, bucket_origin outside [0, bucket_s), a
 * bucket_op other than TAD_OP_SUM / TAD_OP_MAX (TAD_OP_AUTO too: a state does not remember which of the two built it) and TAD_ALGO_DROP
 * (the drop job buckets by day in tad_drop_select).
 * tad_stats: rows_in = rows_used = the window's RAW points; n_points = the buckets; n_keys and t0 are over the buckets (t0: the smallest
 * bucket start); the moments and the ARIMA counters as tad_run over W'' reports them.  host_syncs: 2 on an empty state, 3 when the
 * window is empty, else 4 — tad_run_state_keys' 3 plus one, the bucket total being read before the view is sized — plus the since's one
 * for DBSCAN and ARIMA.  Unlike the *_keys calls a window that leaves every key whole, or no window at all, still builds a view.
 * How: times ascend per key, so a bucket is a contiguous run of a key's window range — a segmented fold and a compaction, no sort, no
 * hash.  Two passes over the window's chunks of 2048 points (heads per chunk, then the fold: ballot ranks and a segmented scan by
 * shuffles per 64 points; a run that crosses a chunk edge is combined by 64-bit integer atomics), straight from the state's arrays: no
 * unbucketed copy of the window is written.  Moments: a key with a point cut or folded away is replayed over its buckets, as for a
 * window.  DBSCAN's history: the buckets' values sorted per key.
 * Memory outside the state (job-context workspace, as tad_run_state_window's): 16 B per bucket, 8 B more for DBSCAN, 12 B per chunk
 * (one chunk per key and per 2048 points of the state) and about 100 B per key. */
#define TAD_FEATURE_STATE_BUCKETS 262144u /* tad_run_state_buckets: a state's window judged in time buckets, read-only */
typedef struct {
  int64_t from_t;                    /* tad_run_state_window's window, on the RAW points, applied first */
  int64_t to_t;
  uint64_t keep_points;
  const uint8_t *key_keep;           /* tad_run_state_keys' mask or NULL */
  const int64_t *key_since;          /* tad_run_state_since's report rule, per key, or NULL */
  int64_t since_t;                   /* 0 = none */
  uint64_t num_keys;                 /* as tad_report_window */
  tad_mem key_memory;
  int64_t bucket_s;                  /* >= 1 */
  int64_t bucket_origin;             /* 0 <= bucket_origin < bucket_s */
  tad_value_op bucket_op;            /* TAD_OP_SUM or TAD_OP_MAX (TAD_OP_AUTO is refused) */
} tad_bucket_window;
int tad_run_state_buckets(tad_engine *e, tad_state *s, const tad_job *job, const tad_bucket_window *w, tad_mem out_memory, tad_result **out);

/* ---- a state's old points folded into time buckets, in place (TAD_FEATURE_STATE_ROLLUP; check tad_features() before calling this) ----
 * A state keeps one point per key and second, and tad_state_trim can only delete old points.  tad_state_rollup coarsens them instead:
 * "seven days of context, the newest day at full resolution" costs a day of seconds plus six days of minutes, not a week of seconds.
 * The transformation.  Let W be the table of points the state holds (tad_run_state's W) and
 *     b = bucket_origin + bucket_s * floor((before_t - bucket_origin) / bucket_s)
 * the bound FLOORED to a bucket start (FLOOR division, csrc/tad_bucket.h), so that no bucket straddles it; b is reported in
 * stats->before_t.  Let Wr be W with flow_end_s replaced by its bucket's start (tad_run_state_buckets' formula) for every point with
 * flow_end_s < b; the points at or after b are untouched, those in [b, before_t) too.
 * Contract.  After a successful call the state — n, avg, m2, ewma, last_t, series, times, and the history if it has one — is bit for
 * bit what a fresh state of the same flags and num_keys holds after ONE tad_run_stream EWMA batch over Wr with value_op = bucket_op and
 * ewma_alpha (0 -> 0.5): tad_state_trim's shape of contract.  In detail:
 *   - series and times: Stage 0 of Wr per key — the points of one key and bucket fold into one point at the bucket's start, sums wrapping
 *     mod 2^64, maxima unsigned; times still ascend strictly (bucket starts below b are distinct and below b);
 *   - the history, if any: every key's new values sorted;
 *   - a key that lost no point keeps n, avg, m2 and ewma as they are — also when the times of its old points moved to their bucket
 *     starts — so, as for a trim, the contract holds for it when its batches used the same ewma_alpha; a key that lost a point is
 *     replayed from the zero state over its new series with the very step of the stream batches;
 *   - last_t becomes the key's newest time AFTERWARDS.  Unlike a trim this can change it: a key whose newest point lies below b gets
 *     that point's bucket start.
 * Consequences:
 *   - idempotent: the same call twice leaves the same bits;
 *   - composable: with bucket_s dividing bucket_s' and bucket_origin' congruent to bucket_origin mod bucket_s, a roll-up at bucket_s
 *     followed by one at bucket_s' over the same bound b — both calls floor to it, so b is a bucket start of the coarser call — equals
 *     the one at bucket_s' alone (sum and max buckets compose);
 *   - tiers commute: "older than 7 d at 3600 s" and "older than 1 d at 60 s" may run in either order;
 *   - tad_run_state_buckets at a multiple of bucket_s with a congruent origin and the same op returns, on the rolled state, the rows it
 *     returns on the raw state, bit for bit — over the whole state and over any window whose from_t / to_t are bucket starts of that
 *     call.  keep_points counts POINTS, which the roll-up made fewer: a window with keep_points differs;
 *   - a stream batch after the roll-up is accepted iff it is newer than the NEW last_t: a point inside a key's last, rolled bucket is
 *     taken (it sits beside the bucket's point), one at the bucket's start is late;
 *   - late rows merged (tad_state_merge) into the rolled region sit beside the bucket's point and are still right at bucket
 *     resolution; a later roll-up folds them;
 *   - a ranged tad_state_replace whose from_t lies inside the rolled region and is not a bucket start erases the seconds from from_t
 *     on but not the bucket's point before it, which already holds their old values: it double-counts.  This is the caller's duty
 *     (the Python layer refuses it).
 * Arguments and refusals (TAD_ERR_INVALID_ARGUMENT with a message, state unchanged): a NULL engine or state; a state without
 * TAD_STATE_SERIES | TAD_STATE_TIMES; stale times; bucket_s < 1 or bucket_origin outside [0, bucket_s); a bucket_op other than
 * TAD_OP_SUM / TAD_OP_MAX; ewma_alpha outside [0, 1]; |before_t| >= 2^62.  An empty state, or a state with no point below b, is
 * TAD_OK with the state untouched (points_rolled == 0).
 * Atomic like a trim: only the candidate copies (moments, offsets, arenas) and job-context workspace are written, and the candidates
 * become current together; any failure — the workspace limit (TAD_ERR_GRID_TOO_LARGE), an allocation, a HIP error — leaves moments,
 * history, series and times bit for bit as they were; the limit and the allocations are checked before any candidate is written.  The
 * arenas shrink by tad_state_trim's rule (below a quarter of its capacity an arena is allocated anew at twice its length), so
 * tad_state_bytes falls.
 * How: tad_run_state_buckets' two passes over every key's whole segment with a piecewise bucket function (a point at or after b is a
 * bucket of its own): heads per chunk of 2048 points, one scan, then the fold written straight into the candidate arenas — no packed
 * copy of the state in between.  A chunk wholly at or after b is a plain coalesced copy.  The history is re-sorted per key.
 * Memory outside the state: 12 B per chunk (one per key and per 2048 points) and about 30 B per key of job-context workspace.
 * Lock order: the state, then a job context, as a trim. */
#define TAD_FEATURE_STATE_ROLLUP 524288u /* tad_state_rollup: a state's points below a bound folded into time buckets, in place */
typedef struct {
  uint64_t points_before;                 /* series points of the state before the call */
  uint64_t points_after;                  /* ... and after it */
  uint64_t points_rolled;                 /* raw points that lay below the bound */
  uint64_t buckets;                       /* points the state holds below the bound afterwards */
  uint64_t keys_changed;                  /* keys that lost at least one point */
  int64_t  before_t;                      /* the bound that was applied (floored, above) */
  double   ms_total;                      /* HIP events; 0 when nothing ran */
  int32_t  job_context;
} tad_rollup_stats;
int tad_state_rollup(tad_engine *e, tad_state *s, int64_t before_t, int64_t bucket_s, int64_t bucket_origin,
                     tad_value_op bucket_op, double ewma_alpha, tad_rollup_stats *stats /* may be NULL */);

/* ---- the batch verdicts over a time range of a state (TAD_FEATURE_STATE_WINDOW; check tad_features() before calling this) ----
 * tad_run_state judges everything the state holds, and tad_state_trim narrows a state for good and at its old end only.  A state that
 * keeps seven days can answer "the last 24 h" or "everything up to the last complete hour" with this call: read-only, any window the
 * state covers.  Cost: tad_run_state's over the window plus the view (below).  Measured on 24 h states of 1e5 and 1e6 keys it is below
 * tad_run over the same points in device columns for EWMA on every window tried and for DBSCAN except in one corner: a state of very many
 * short keys (1e6 keys, about 100 points each) and a window that keeps nearly all of it, where the call took 1.14x tad_run's time — the
 * view copies almost the whole state and rewrites its history.
 * The window.  Of every key's series, in time order: (1) the points with flow_end_s >= from_t, when from_t != 0; (2) and flow_end_s <
 * to_t, when to_t != 0 — the half-open rule of tad_job.end_time (anomaly_detection.py:584-586); (3) then only the newest keep_points of
 * those, when keep_points != 0.  (1) and (3) are tad_state_trim's rules.  All three zero is the whole state.  BOTH bounds act on
 * flowEndSeconds: the state holds no flowStartSeconds, so from_t is NOT the reference's start_time filter, which tests flowStartSeconds
 * (anomaly_detection.py:581-583); a caller that needs that filter applies it to the rows before they reach the state.
 * Contract: let W be tad_run_state's W and W' its rows inside the window.  The call returns exactly the rows tad_run returns for W' with
 * the same algo, detector parameters and TAD_FLAG_EMIT_ALL_POINTS: key_id, flow_end_s, throughput, algo_calc, stddev (and anomaly with the
 * flag), in the same (key, time) order, bit for bit, whatever Stage-0 path tad_run takes for W'.  Equivalently, with to_t == 0: the rows
 * of tad_run_state on a copy of the state after tad_state_trim(keep_points, from_t).  The state is read only: after the call,
 * successful or not, moments, history, series and times are unchanged.
 * Arguments: the honoured tad_job fields, the refusals and what the state must hold are tad_run_state's — start_time / end_time in the
 * job stay refused (the window is this call's arguments), as do TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32 and TAD_ALGO_DROP; EWMA and ARIMA
 * need TAD_STATE_SERIES | TAD_STATE_TIMES, DBSCAN needs TAD_STATE_HISTORY as well; stale times are refused.  from_t > to_t with both
 * non-zero is TAD_ERR_INVALID_ARGUMENT; from_t == to_t is an empty window; an empty window or an empty state is TAD_OK with zero rows.
 * tad_stats: as tad_run_state, over W' — rows_in = rows_used = n_points = the window's points, n_keys = keys with a point in the window,
 * t0 = the smallest time in the window, pts_mean / pts_m2 merged from the window's per-key moments, the ARIMA counters as tad_run over
 * W' reports them, the Stage-0 fields zero; host_syncs is 3 when bounds are set on a non-empty state (one more than tad_run_state: the
 * window's size is read before the view is allocated) and 2 for the all-zero window or an empty state.
 * How: a key cut by the window has its (n, avg, m2) replayed from the zero state over its window values with the very step of the
 * stream and of tad_state_trim — one lane's serial chain as long as the cut key's window, as for a trim; a key wholly inside takes the
 * state's moments (bit-identical by the state's invariants).  DBSCAN judges against the window's values sorted per key, not the state's
 * history: when 2 * (window points) <= (state points) the window's values are sorted, otherwise the excluded values are sorted and
 * removed from the state's history — the same bits either way, so "everything but the newest hour" does not sort 99 % of the state to
 * remove 1 %.  ARIMA's lambda, Box-Cox and fits run over the window's subseries.  When the window leaves every key whole the state's own
 * arrays are judged and the call costs tad_run_state plus the bounds.
 * Memory outside the state: the window's view lives in the workspace of the job context that runs the call — about 16 B per window point
 * (values and times), 8 B more per window point for DBSCAN's sorted values, 16 B per excluded point on the subtract path (packed and
 * sorted), about 80 B per key, and the sort's scratch; sized from the window, not the state; grow-only like all context workspace, kept
 * by every context that ever ran such a call (at most max_jobs_in_flight of them) and NOT counted by tad_state_bytes.  Any failure,
 * allocation included, returns an error with no result and the state untouched.
 * Lock order: the state, then a job context, as tad_run_state; calls on one state are serial, tad_job_progress finds the job by id. */
#define TAD_FEATURE_STATE_WINDOW 64u  /* tad_run_state_window: tad_run_state over a time range / newest points of the state, read-only */
int tad_run_state_window(tad_engine *e, tad_state *s, const tad_job *job, int64_t from_t, int64_t to_t,
                         uint64_t keep_points, tad_mem out_memory, tad_result **out);
/* the rule of DBSCAN's window history, the very function the call uses: 1 = the window's values are sorted, 0 = the excluded values are
 * sorted and subtracted from the state's history.  Needs no device. */
int tad_window_history_by_sort(uint64_t window_points, uint64_t state_points);

/* ---- key ids that stay the same from batch to batch: a key dictionary kept in HBM (TAD_FEATURE_KEY_DICT; check tad_features() before
 * calling these) ----
 * Every streaming call above takes dense key ids: cols->num_keys must equal the state's, and key k must be the same flow key in every
 * batch for as long as the state lives.  tad_factorize numbers the keys of ONE call (its table is scratch, a match is confirmed against
 * that call's input rows), so a streaming host had to keep its own tuple -> id map in front of the engine.  tad_keydict is that map on
 * the device: it maps key tuples to dense ids, hands out new ids in order of first appearance, and outlives the call.
 * tad_keydict_create: n_cols (1..8) is the tuple width for the dictionary's life.  expected_keys sizes the first table (0 = a default
 * that stays in the caches, 2^20 slots); 1 gives the smallest table the implementation allows (64 slots, 32 key records).  The dictionary
 * grows by itself whatever was given here.
 * tad_keydict_encode, one batch: kc is tad_factorize's argument — host or device memory (all arrays, inputs and outputs, live in
 * kc->memory), keep masks, an optional second tuple per row — and kc->n_cols must equal the dictionary's.  The side (0 = a, 1 = b) is
 * part of the tuple, as in tad_factorize; a batch without cols_b is side 0, and one dictionary takes one-sided and two-sided batches alike.
 *   - a tuple the dictionary holds gets the id it holds for it;
 *   - new tuples get the ids *num_keys_before, *num_keys_before + 1, ... in order of first appearance over the batch's kept virtual rows
 *     [side a: 0 .. n) ++ [side b: n .. 2n);
 *   - rows that are not kept get TAD_KEY_SKIP;
 *   - new_first_row[j] (j < new_first_row_cap) = the virtual row of THIS batch where key *num_keys_before + j first appears — the host
 *     reads the new key's strings there, as with tad_factorize's first_row.  A cap below the number of new keys caps the list, never the ids;
 *   - *num_keys_before and *num_keys (either may be NULL) = the keys held before and after the call.
 * One-sided batches: after batches 1..b the ids of batch b's rows equal what tad_factorize returns for those rows when called once on the
 * concatenation of batches 1..b.  Two-sided batches are numbered in the sequential order b1.a, b1.b, b2.a, b2.b, ...  Ids are never
 * reused or moved, except by tad_keydict_compact (below), which the caller asks for.  The values of a string column move only through tad_keydict_recode (further below), after its vocabulary was compacted.  Limits: n_rows * sides < 2^32 - 1 per batch, fewer than 2^32 - 1 keys per dictionary.  An empty batch is TAD_OK.
 * tad_keydict_lookup is tad_keydict_encode read-only: an unknown tuple gets TAD_KEY_SKIP and the dictionary is unchanged.
 * tad_keydict_export writes the tuples of the keys [first_key, first_key + n_keys) into n_cols HOST arrays of n_keys entries (cols[c][i] =
 * column c of key first_key + i) and their sides into side[n_keys] (HOST, may be NULL).  tad_keydict_import fills an EMPTY dictionary so
 * that key i is tuple i (side NULL = every key on side 0): a restart, as tad_state_import is.  A duplicate tuple, a dictionary that holds
 * keys, or a side > 1 is TAD_ERR_INVALID_ARGUMENT and leaves the dictionary unchanged.
 * Strings: the dictionary holds integers.  A host with string key columns passes codes that are stable across batches — one vocabulary
 * per column, kept for the life of the dictionary.
 * Atomic: everything that can fail happens before the dictionary is touched — argument checks, the workspace limit, every allocation,
 * growth of the table into a fresh table, growth of the key records — so any failure leaves num_keys, the ids and the exported tuples
 * as they were.  (Growth may have taken place: it changes the capacity, never the contents.)
 * How: an open-addressing table of 8-byte slots, fingerprint << 32 | id, and one record per key with its tuple (side + n_cols words,
 * padded to a multiple of 16 bytes), against which a fingerprint match is confirmed (theia_amd/csrc/tad_keydict.hip).  A batch probes
 * the table once; a batch of known tuples ends there with one synchronisation.  Rows with unknown tuples are factorised among
 * themselves by tad_factorize's kernels, one lane per new key appends its record and claims a slot, and the new ids are written.  The
 * table is kept at a load of at most 1/2: when new keys would pass that, a table of the next power of two is filled from the records
 * and swapped in.
 * Memory: tad_keydict_bytes = the device bytes the dictionary holds (table and key records at their capacity).  Scratch is job-context
 * workspace and is checked against tad_engine_opts.workspace_limit (TAD_ERR_GRID_TOO_LARGE): V bytes of miss flags for the V = n_rows *
 * sides virtual rows, plus the staged columns, masks and ids of a host batch; a batch with unknown tuples adds 8 V bytes of local ids,
 * 8 bytes per miss row and tad_factorize's scratch for V virtual rows.
 * Lock order: the dictionary, then a job context; calls on one dictionary are serial. */
#define TAD_FEATURE_KEY_DICT 128u     /* tad_keydict: a persistent tuple -> key id dictionary on the device */
typedef struct tad_keydict tad_keydict;
int tad_keydict_create(tad_engine *e, int32_t n_cols, uint64_t expected_keys, tad_keydict **out);
void tad_keydict_destroy(tad_engine *e, tad_keydict *d);
int tad_keydict_encode(tad_engine *e, tad_keydict *d, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2,
                       uint64_t *new_first_row, uint64_t new_first_row_cap, uint64_t *num_keys_before, uint64_t *num_keys);
int tad_keydict_lookup(tad_engine *e, const tad_keydict *d, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2);
int tad_keydict_num_keys(tad_engine *e, const tad_keydict *d, uint64_t *num_keys);
int tad_keydict_bytes(tad_engine *e, const tad_keydict *d, uint64_t *bytes);
int tad_keydict_export(tad_engine *e, const tad_keydict *d, uint64_t first_key, uint64_t n_keys, int64_t *const *cols, uint8_t *side);
int tad_keydict_import(tad_engine *e, tad_keydict *d, uint64_t n_keys, const int64_t *const *cols, const uint8_t *side);

/* ---- retiring dead keys: a state and its dictionary compacted (TAD_FEATURE_KEY_RETIRE; check tad_features() before calling these) ----
 * Key ids are handed out in order of first appearance, and with per-connection keys (TAD_AGG_NONE: the tuple carries ports and
 * flowStartSeconds) every new connection is a new key.  A state trimmed to "the last 24 h" still kept moments, offsets, a key record and
 * table slots for every connection it ever saw, and every stream batch walked all of them.  These two calls take the dead keys out: one
 * drops them from a state and renumbers the survivors densely, the other applies the same renumbering to the dictionary.  Nothing is
 * recomputed: what a survivor holds is moved, bit for bit.
 * tad_state_compact, on every kind of state (plain, history, series, series + times, all of them):
 *   - key k survives iff n[k] > 0 and (retire_before_t == 0 or last_t[k] >= retire_before_t); 0 means "no time rule", as keep_from_t
 *     does in tad_state_trim.  So an unseen key (never fed, or emptied by a trim) always goes, an idle key goes by its newest time;
 *   - a survivor's new id is the number of survivors below it: the relative order — order of first appearance — is kept;
 *   - remap (required; keys_before = the state's num_keys entries, in remap_memory): remap[k] = the new id of old key k, or
 *     TAD_KEY_SKIP for a retired key.  The host maps its own key table and any key ids it still holds through it;
 *   - afterwards the state is bit for bit a fresh state with the same flags and max(m, 1) keys (m survivors; a state never holds fewer
 *     than one key) into which the survivors' exports were imported — moments, history, series and times: survivor j holds old key k's
 *     entries unchanged.  With m == 0 the one remaining key is unseen;
 *   - so any later tad_run_stream, tad_state_merge, tad_state_trim or tad_run_state(_window) on the compacted state, with key ids passed
 *     through remap, gives what the same call gives on the uncompacted state, minus the retired keys' rows.
 * Atomic, like a trim: only candidate copies and job-context workspace are written, and they are swapped in together; any failure —
 * allocation, workspace over workspace_limit (TAD_ERR_GRID_TOO_LARGE), a HIP error — leaves the state exactly as it was.  A state whose
 * times are stale is refused, as a trim refuses it.  When nothing is retired the call is TAD_OK, remap is the identity, the state is
 * untouched and nothing is reallocated.  When only unseen keys go (points_dropped == 0) every arena already holds exactly the survivors'
 * segments in order: no arena element is moved, only the moment blocks and the offsets are rebuilt at the new key count.  Otherwise the
 * arenas are gathered into the candidates and the trim's shrink rule applies: below a quarter of its capacity an arena is allocated anew
 * at twice its length.  Workspace: about 68 B per key of the state before the call, plus 8 B per key for a remap in host memory.
 * Lock order: the state, then a job context.
 * tad_keydict_compact applies a remap to the dictionary: remap_len must equal the dictionary's num_keys (resize the state to the
 * dictionary's keys first, as the ingest recipe does), and the entries that are not TAD_KEY_SKIP must be exactly 0, 1, ..., m - 1,
 * strictly increasing with k (checked on the device).  Any other remap — a wrong length, a swapped pair, a duplicate, a gap — is
 * TAD_ERR_INVALID_ARGUMENT and the dictionary stays unchanged.  Afterwards the dictionary is what a fresh one holds after
 * tad_keydict_import of the surviving tuples (sides included) in new-id order: a survivor encodes and looks up to remap[old id], a
 * retired tuple looks up to TAD_KEY_SKIP, and tad_keydict_encode gives a retired tuple that returns a new id at the end (m, m + 1, ...).
 * The table and the key records are rebuilt at the size tad_keydict_create(expected_keys = 2 m) would pick (the minimum for m == 0) and
 * never larger than before, so tad_keydict_bytes does not grow.  Fresh allocations are filled first and swapped in last: any failure
 * leaves the dictionary as it was.  *num_keys (may be NULL) = the keys held afterwards.  Lock order: the dictionary, then a job context. */
#define TAD_FEATURE_KEY_RETIRE 256u   /* tad_state_compact / tad_keydict_compact: dead keys dropped, the survivors renumbered densely */
typedef struct {
  uint64_t keys_before;              /* the state's num_keys at entry */
  uint64_t keys_after;               /* surviving keys m */
  uint64_t num_keys;                 /* the state's num_keys at exit: max(m, 1) — a state never holds fewer than one key */
  uint64_t keys_unseen;              /* retired because n == 0 */
  uint64_t keys_idle;                /* retired because last_t < retire_before_t (n > 0) */
  uint64_t points_dropped;           /* sum of n over the idle-retired keys */
  uint64_t series_points_moved;      /* arena elements copied; 0 when points_dropped == 0 */
  uint64_t history_points_moved;
  uint64_t bytes_before;             /* tad_state_bytes at entry ... */
  uint64_t bytes_after;              /* ... and at exit */
  int32_t job_context;
  int32_t reserved;
  float ms_total;                    /* HIP events */
  float reserved1;
} tad_compact_stats;
int tad_state_compact(tad_engine *e, tad_state *s, int64_t retire_before_t, uint64_t *remap, tad_mem remap_memory,
                      tad_compact_stats *stats /* may be NULL */);
int tad_keydict_compact(tad_engine *e, tad_keydict *d, const uint64_t *remap, uint64_t remap_len, tad_mem remap_memory,
                        uint64_t *num_keys /* may be NULL */);

/* ---- the drop detector on a state (TAD_FEATURE_STATE_DROP; check tad_features() before calling these) ----
 * TAD_ALGO_DROP is the abnormal-traffic-drop detector of the reference's Snowflake backend (drop_detection_udf.py): per key, mean and
 * pandas' sample std over the key's daily counts, a day is anomalous when it lies more than drop_nsigma std from the mean.  The reference
 * runs it as an "initial" job over the whole table and names a "periodical" job it does not have (dropDetection.go:282).  These two calls
 * are that job on a streaming state: tad_drop_stream adds a batch and judges the batch's points against everything the state then holds,
 * tad_drop_state returns the batch verdicts of a window of the state.  tad_run_stream, tad_run_state and tad_run_state_window keep
 * refusing TAD_ALGO_DROP; for both calls here job->algo must be TAD_ALGO_DROP (anything else is TAD_ERR_INVALID_ARGUMENT).
 * pandas sums pairwise (numpy's pairwise_sum_DOUBLE), which running moments cannot reproduce bit for bit; a state created with
 * TAD_STATE_SERIES holds every key's aggregated values in time order, and both sums are taken over that series in numpy's order.
 * tad_drop_state, read-only.  The window is tad_run_state_window's: from_t, to_t and keep_points with the same three rules; all zero is
 * the whole state; from_t > to_t with both non-zero is TAD_ERR_INVALID_ARGUMENT; an empty window or an empty state is TAD_OK with zero
 * rows.  Contract: with W' the table of one row per series point inside the window, the call returns exactly the rows of
 * tad_run(TAD_ALGO_DROP) over W' with the same drop_nsigma, drop_min_samples (0 = the defaults 3 and 3) and TAD_FLAG_EMIT_ALL_POINTS:
 * key_id, flow_end_s, throughput, algo_calc (the key's mean), stddev (pandas' sample std) and anomaly (with the flag), bit for bit, in
 * (key, time) order, whatever Stage-0 path tad_run takes for W'.  A key has a result iff n >= drop_min_samples && n >= 2, n its points
 * inside the window; the other keys with points emit nothing and count in keys_no_result.  The state needs TAD_STATE_SERIES |
 * TAD_STATE_TIMES; no history is needed.  Refused as tad_run_state refuses them: stale times, start_time / end_time non-zero, the
 * narrow-column flags, a negative drop_nsigma or drop_min_samples.  tad_stats: rows_in = rows_used = n_points = the window's points;
 * n_keys, n_anomalies, keys_no_result, t0 and host_syncs as tad_run_state_window; the Stage-0 fields zero; pts_mean / pts_m2 merged from
 * the per-key pairwise mean and sum of squared deviations (equal to tad_run's up to rounding).  After the call, successful or not, the
 * state is bit for bit what it was.  A window that cuts keys builds tad_run_state_window's view, values and times only — DROP reads no
 * moments, so none are replayed; a window that leaves every key whole judges the state's own arrays.
 * tad_drop_stream, the periodical job: one batch.  Its effect on the state is exactly that of tad_run_stream with TAD_ALGO_EWMA and the
 * same job fields on the same state: the same Stage-0 rule and plan overrides, agg_flow, value_op, start_time / end_time, ewma_alpha and
 * the narrow flags; moments, ewma, last_t, series, times and history are bit for bit those of the EWMA batch; a late row, a key out of
 * range or a failed allocation fails the batch and leaves everything as it was; cols->num_keys must equal the state's.  The state needs
 * TAD_STATE_SERIES; times and history are optional and are appended to when present.  Rows: for the batch's new points only, in (key,
 * time) order — the rows tad_drop_state with the all-zero window would return after the batch, restricted to the batch's points;
 * equivalently what tad_run(TAD_ALGO_DROP) over everything the state now holds emits for these points.  Mean and std are taken over the
 * key's whole post-batch series.  A touched key without a result emits nothing and counts in keys_no_result; untouched keys are not read
 * at all.  Points of earlier batches are not judged again: each point once, when it arrives, as the DBSCAN and ARIMA streams do.
 * drop_nsigma / drop_min_samples may differ from batch to batch.  The remaining stats are a DBSCAN stream batch's.
 * Cost and memory: two passes over the judged keys' series (a lane per key, a wavefront per key of at least 512 points, or of 8 times
 * the mean length above 8192 keys), no K x T grid and no K x T workspace; about 29 B per key and 13 B per judged point of job-context
 * workspace, grow-only.  Not yet measured on an MI355X.
 * Lock order: the state, then a job context, as the calls above; calls on one state are serial, tad_job_progress finds the job by id. */
#define TAD_FEATURE_STATE_DROP 512u   /* tad_drop_state / tad_drop_stream: the drop detector on a series state */
int tad_drop_state(tad_engine *e, tad_state *s, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points,
                   tad_mem out_memory, tad_result **out);
int tad_drop_stream(tad_engine *e, tad_state *s, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_result **out);

/* ---- the drop job's flow-row query (TAD_FEATURE_DROP_ROWS; check tad_features() before calling these) ----
 * The three forms of the drop detector start from per-endpoint daily drop counts.  The reference gets those from the query that
 * snowflake/cmd/dropDetection.go:36-190 builds over the flow table: it filters on the two network-policy rule actions (:65-72, the time bounds :85-105), picks
 * endpoint and direction per row (the CASE at :131-148), takes to_date(flowStartSeconds) and count(*) per nine-column group (:59-62, :119-128), then SUM per
 * (endpoint, direction, date) (:155-165).  tad_drop_select is that query up to the sums, on columns held in HBM (fetch_flows_device,
 * tad_encode_strings, tad_widen_column, tad_mask_rows): it selects the dropped rows, chooses a side per row, buckets by day and hands over
 * compact columns; tad_factorize / tad_keydict_encode over the four tuple columns and Stage 0 (tad_run / tad_drop_stream with TAD_OP_SUM
 * over key id, day_s, count) do the rest.
 * Row rule.  Row i is selected iff (ia in {2,3} || ea in {2,3}) && (start_time == 0 || flow_start_s >= start_time) &&
 * (end_time == 0 || flow_end_s < end_time) && (keep == NULL || keep[i] != 0); ia / ea are ingress_action / egress_action, the
 * ingressNetworkPolicyRuleAction / egressNetworkPolicyRuleAction UInt8 columns (create_table.sh:63,68; 2 = Drop, 3 = Reject).  The row
 * is on the INGRESS side iff ia in {2,3} — ingress wins when both actions drop, as the CASE has it — else on the egress side.  Ingress
 * rows describe the destination, egress rows the source.  On the chosen side the endpoint is a pod when pod_name != <side>_pod_null and
 * an IP otherwise.  Output, one row per selected row, in INPUT ORDER (so the ids tad_factorize and tad_keydict_encode then hand out are
 * the ids a host path over the same rows gives):
 *   pod endpoint: endpoint_kind = 1, endpoint_ns = pod_ns, endpoint_name = pod_name;   IP endpoint: endpoint_kind = 0, endpoint_ns = 0,
 *   endpoint_name = ip;   direction: 0 ingress, 1 egress;   day_s = floor(flow_start_s / 86400) * 86400 (floor, not truncation: -1 is day
 *   -86400);   count = 1;   row = i.
 * Comparing the (kind, ns, name) tuples equals comparing the reference's endpoint strings — CONCAT(ns, '/', name) for a pod, the IP string
 * otherwise — as long as no namespace or pod name contains '/', which Kubernetes forbids (both are DNS labels / subdomains), and an IP string
 * contains none either: the kind column keeps a pod from colliding with an IP whose code happens to be equal.  Summing count by
 * (tuple, day_s) equals the query's two GROUP BYs composed: the first groups by (endpoint, direction, date) AND further columns, so its
 * extra columns only split groups that the second, which sums the first's counts by (endpoint, direction, date) alone, merges again —
 * the sum of the parts' count(*) is the count(*) of the whole.
 * Columns.  All of one memory space (cols->memory); the code columns are int64 dictionary codes of any one dictionary per column pair
 * (src_ip / dst_ip share one, as do the namespaces and the pod names, if the tuples are to compare across sides).  flags: 0 or
 * TAD_FLAG_TIME_U32 — flow_start_s / flow_end_s point to uint32_t[n_rows], zero-extended; start_time, end_time and day_s stay 64-bit.
 * Columns need only their natural alignment (1, 8 or 4 bytes): a device slice at any offset is accepted; 16-byte aligned action columns
 * are read with 16-byte loads.  The call reads its inputs only; two calls on the same inputs give the same result.  It leases a job
 * context as the other ingest calls do, so it runs beside jobs.  The result belongs to the library, as tad_points does: free it with
 * tad_drop_rows_free.  n_rows == 0 returns an empty result (n_rows = 0, NULL columns).
 * TAD_ERR_INVALID_ARGUMENT, a message in tad_last_error and no result: a NULL engine, cols or out; a mandatory column NULL with
 * n_rows > 0; end_time != 0 with flow_end_s == NULL; a flag other than TAD_FLAG_TIME_U32.
 * Cost: two launches with a scan between them and two host synchronisations (the host reads the total to size the result).  About
 * 2.25 B a row for the action columns and the row bitmask, plus the sectors the selected rows touch and 56 B written per selected row;
 * n_rows / 8 B + 12 B per 4096 rows of job-context workspace, grow-only; a host table is staged whole.  Not yet measured on an MI355X
 * (DESIGN.md §5). */
#define TAD_FEATURE_DROP_ROWS 1024u   /* tad_drop_select: flow rows -> the drop job's (endpoint, direction, day, count) rows */
typedef struct {
  uint64_t n_rows;
  const uint8_t *ingress_action;                    /* UInt8, create_table.sh:63 */
  const uint8_t *egress_action;                     /* UInt8, create_table.sh:68 */
  const int64_t *flow_start_s;                      /* mandatory: the date and the start filter */
  const int64_t *flow_end_s;                        /* optional (NULL) */
  const int64_t *src_ip;                            /* dictionary codes, these six */
  const int64_t *src_pod_ns;
  const int64_t *src_pod_name;
  const int64_t *dst_ip;
  const int64_t *dst_pod_ns;
  const int64_t *dst_pod_name;
  int64_t src_pod_null;                             /* the pod-name code that means NULL / '' on that side; -1 = none */
  int64_t dst_pod_null;
  const uint8_t *keep;                              /* optional (NULL): tad_mask_rows' output, e.g. the clusterUUID predicate */
  uint32_t flags;                                   /* TAD_FLAG_TIME_U32 only */
  tad_mem memory;
} tad_drop_flow_columns;

typedef struct {
  uint64_t n_rows;                                  /* m */
  int64_t *endpoint_kind;                           /* the key tuple, these four: ready for tad_key_columns.cols_a */
  int64_t *endpoint_ns;
  int64_t *endpoint_name;
  int64_t *direction;
  int64_t *day_s;
  uint64_t *count;
  uint64_t *row;
  tad_mem memory;
} tad_drop_rows;

int tad_drop_select(tad_engine *e, const tad_drop_flow_columns *cols, int64_t start_time, int64_t end_time,
                    tad_mem out_memory, tad_drop_rows **out);
void tad_drop_rows_free(tad_engine *e, tad_drop_rows *r);

/* ---- key-filtered jobs on a streaming state (TAD_FEATURE_KEY_SELECT; check tad_features() before calling these) ----
 * The job's argument vector carries --pod-name, --pod-namespace, --pod-label, --external-ip and --svc-port-name.  On the batch path they
 * are row predicates ahead of Stage 0 (tad_mask_rows).  Every one of them tests key columns of the mode (destinationIP in external mode,
 * destinationServicePortName in svc mode, namespace / name / labels per side in pod mode), so on a state they are KEY selections, and the
 * detectors are per key: the tuples are in the dictionary, the selection is computed where they live, and the window calls leave the
 * keys that are not selected empty.  Filters that test other columns (the namespace ignore list over both sides, flowStartSeconds) are
 * applied to the rows before they reach the state.
 * tad_keydict_select, read-only.  key_keep[k] = 1 iff (side < 0 || key k's side == side) and, for every term t < n_terms,
 * masks[t][tuple_k[term_col[t]]] != 0; otherwise 0 — tad_mask_rows' rule on the dictionary's records instead of on rows.  n_terms is
 * 0 .. 8 (0: the side test alone); a column may appear in several terms; side is -1 (either), 0 (a) or 1 (b); term_col[t] is in
 * [0, n_cols); any non-zero mask byte selects.  key_keep_len must equal the dictionary's num_keys — a stale length is refused, never a
 * short write.  `memory` says where masks[t] and key_keep live; term_col, mask_len and the pointer array masks are host memory; host
 * masks and a host key_keep are staged by the call; device pointers need no alignment.  *n_selected (may be NULL) = the keys selected.
 * An empty dictionary is TAD_OK with *n_selected = 0.  TAD_ERR_INVALID_ARGUMENT, a message in tad_last_error: a NULL engine or
 * dictionary; n_terms outside 0 .. 8 or its arrays NULL; side outside -1 .. 1; term_col out of range; a NULL mask of non-zero length;
 * key_keep NULL with a non-zero length; key_keep_len != num_keys; and a key whose value in a term's column lies outside
 * [0, mask_len[t]) — raised from a device flag after the kernel ran, as tad_widen_column raises an index outside its table; key_keep is
 * then unspecified.  The dictionary is never changed.  Lock order: the dictionary, then a job context.
 * Cost: one launch, one host synchronisation; per key one record (16 .. 80 B), one mask byte per term and one byte written; a host call
 * stages the masks and num_keys bytes of job-context workspace, grow-only.
 * tad_run_state_keys / tad_drop_state_keys, read-only: tad_run_state_window / tad_drop_state over the selected keys.  With W' the
 * window's rows of those calls (same from_t, to_t, keep_points) and W'' the rows of W' whose key has key_keep[key] != 0, the call returns
 * exactly the rows tad_run returns for W'' — equivalently the rows of the window call whose key_id is selected, in the same order, bit
 * for bit.  Key ids are the state's own; nothing is renumbered.  key_keep == NULL with key_keep_len == 0 is the window call itself;
 * otherwise key_keep_len must equal the state's num_keys.  The mask may be host memory (staged into job-context workspace) or device
 * memory at any alignment (key_memory); any non-zero byte selects.  An empty selection is TAD_OK with zero rows.  Every refusal of the
 * window call holds (tad_run_state_keys refuses TAD_ALGO_DROP, tad_drop_state_keys anything else; stale times; from_t > to_t;
 * start_time / end_time; the narrow-column flags; parameters out of range; a state without series and times, or without history for
 * DBSCAN), plus: key_keep NULL with a non-zero length, a length that is not num_keys, key_memory neither host nor device.  After the
 * call, successful or not, the state is bit for bit what it was.
 * tad_stats are over W'': rows_in = rows_used = n_points = the selected points inside the window; n_keys = the selected keys with a
 * point there; t0 = the smallest selected time; n_anomalies, keys_no_result and the ARIMA counters (arima_fits, kalman_steps,
 * arima_nan_fits) are what tad_run over W'' reports — a key that is not selected costs no fit; pts_mean / pts_m2 are merged from the
 * selected keys' moments, equal to tad_run's up to rounding (as tad_run_state's are).  host_syncs is 3 whenever a
 * mask is given and the state holds a point (the mask is a window of its own: the all-zero-window shortcut is not taken).
 * How: the bounds kernel reads one mask byte per key; a key that is not selected gets an empty window with all its points excluded and
 * skips both searches; the view, the moments and DBSCAN's history rule (tad_window_history_by_sort with the SELECTED window points) are
 * the window call's.  When the selection and the window keep every point the state holds, the state's own arrays are judged.  Cost: an
 * O(num_keys) pass of 33 B a key, then the window call's cost over the selected points; on DBSCAN's subtract side (more than half the
 * state's points selected) the excluded points are packed and sorted as for any window.  Not yet measured on an MI355X.
 * Lock order: the state, then a job context; calls on one state are serial; tad_job_progress finds the job by id. */
#define TAD_FEATURE_KEY_SELECT 2048u  /* tad_keydict_select, tad_run_state_keys, tad_drop_state_keys: jobs over selected keys of a state */
int tad_keydict_select(tad_engine *e, const tad_keydict *d, int32_t n_terms, const int32_t *term_col, const uint8_t *const *masks,
                       const uint64_t *mask_len, int32_t side, uint8_t *key_keep, uint64_t key_keep_len, tad_mem memory,
                       uint64_t *n_selected /* may be NULL */);
int tad_run_state_keys(tad_engine *e, tad_state *s, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points,
                       const uint8_t *key_keep, uint64_t key_keep_len, tad_mem key_memory, tad_mem out_memory, tad_result **out);
int tad_drop_state_keys(tad_engine *e, tad_state *s, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points,
                        const uint8_t *key_keep, uint64_t key_keep_len, tad_mem key_memory, tad_mem out_memory, tad_result **out);

/* ---- a string dictionary that outlives the call (TAD_FEATURE_STRING_DICT; check tad_features() before calling these) ----
 * tad_encode_strings numbers the strings of ONE call; the key dictionary above wants, for a string key column, codes that are stable
 * across batches.  A tad_strdict is that vocabulary, held in HBM: to tad_encode_strings what tad_keydict is to tad_factorize.  One per
 * string column (or per group of columns that share codes), kept for the life of the key dictionary behind it.
 * tad_strdict_create: expected_values sizes the first table and records, expected_bytes the first arena of bytes (0 = the defaults,
 * 2^20 slots / 2^16 values / 4 MiB; 1 = the smallest, 64 slots / 32 values / 16 bytes); all three grow on demand.
 * tad_strdict_encode, one batch.  col is tad_encode_strings' argument, unchanged: 32- or 64-bit offsets, an optional validity bitmap with
 * an offset — a null row encodes like the empty string, even when it still owns bytes —, host or device memory; codes (int64[n_rows]) and
 * new_first_row live in col->memory.  A string the dictionary holds gets the code it holds for it; new strings get *num_before,
 * *num_before + 1, ... in order of FIRST APPEARANCE over the batch's rows; new_first_row[j] (j < new_first_row_cap) = the row of this
 * batch where value *num_before + j first appears — the host reads the new strings there, and only there.  A cap below the number of new
 * values caps the list, never the codes.  *num_before / *num_values (either may be NULL) = the values held before / after the call.
 * After batches 1..b the codes of batch b's rows equal what tad_encode_strings returns for those rows when called once on the
 * concatenation of batches 1..b (the one-sided tad_keydict contract, on strings).  Codes are never reused or moved.  The one exception is
 * tad_strdict_compact (further below), which the caller asks for: it drops values and renumbers the rest.  An empty batch is
 * TAD_OK.  Limits: n_rows < 2^32 - 1 per batch, fewer than 2^32 - 1 values per dictionary, one string shorter than 2^32 bytes; the arena
 * of bytes is addressed with 64 bits.
 * tad_strdict_lookup is encode read-only: an unknown string gets TAD_CODE_NONE and the dictionary is unchanged.
 * Atomic, as tad_keydict is: everything that can fail happens before the dictionary is touched — the argument checks; malformed
 * offsets (they decrease or point beyond data_bytes), found on the device while every row's span is read in the probe pass:
 * TAD_ERR_INVALID_ARGUMENT, also when earlier rows of the same batch held new strings; the workspace limit (TAD_ERR_GRID_TOO_LARGE);
 * every allocation; the growth of the table, the records and the arena into fresh allocations.  Any failure leaves num_values, the
 * codes and the exported strings as they were; codes / new_first_row are unspecified then.
 * tad_strdict_export writes the values [first_code, first_code + n_values) in Arrow's layout into HOST memory: offsets[n_values + 1]
 * starting at 0 and the bytes packed in data.  *data_bytes (may be NULL) is always the bytes needed; offsets == NULL && data == NULL is
 * the size query; a data_cap that is too small is TAD_ERR_INVALID_ARGUMENT with nothing written but *data_bytes.
 * tad_strdict_import fills an EMPTY dictionary so that value i is string i (what export returned, after a restart).  Refused with
 * TAD_ERR_INVALID_ARGUMENT, the dictionary unchanged: two strings are equal; the dictionary already holds values; the offsets decrease
 * or do not start at 0.
 * tad_strdict_match, read-only.  mask[c] = 1 iff value c satisfies op with the pattern, else 0.  mask_len must equal num_values — a
 * stale length is refused, never a short write.  `memory` says where mask lives; the pattern is host memory, pattern_len <= 1024;
 * *n_matched may be NULL.  TAD_STR_EQUAL: the value's bytes are the pattern's bytes (an empty pattern selects "" alone).
 * TAD_STR_CONTAINS_NOCASE: the pattern occurs in the value (an empty pattern selects everything), compared after folding 'A'..'Z' to
 * 'a'..'z' and nothing else: a byte >= 0x80 matches only itself, so no Unicode case folding and no % / _ wildcards (those are
 * tad_strdict_like's, further below).  That is enough for the job's filters: Kubernetes restricts namespaces, pod names, label keys
 * and values and service port names to ASCII, and `ilike '%label%'` with a pattern free of %, _ and \ is exactly this operation on
 * ASCII strings; equality (--pod-name, --pod-namespace, --external-ip, --svc-port-name) is TAD_STR_EQUAL.  The mask is ready for
 * tad_keydict_select (masks[t]) and tad_mask_rows in device memory: no string is hashed, compared or matched on the host between the
 * Arrow buffer and the state.
 * tad_strdict_bytes: the device bytes held — table, records and arena at their capacity.  tad_strdict_num_values: the values held.
 * Every call on a NULL engine is TAD_ERR_INVALID_ARGUMENT without a device and writes nothing; tad_strdict_destroy(NULL, NULL) is a no-op.
 * Cost.  A batch of known strings: one launch (the probe pass) and one host synchronisation; it reads the offsets (4 or 8 B a row) and the
 * bytes once, in whole lines, one table word (8 B) and one record (16 B) per row plus ceil(len / 16) aligned 16-byte words of the arena,
 * and writes 8 B of code and 1 B of flag a row.  With misses: tad_encode_strings' passes over the miss rows, a scan, the append, the fix —
 * three more synchronisations at most, plus one per growth.  Job-context workspace, grow-only and bounded by workspace_limit:
 * n_rows + 256 B (miss flags), tad_encode_strings' scratch for n_rows rows (8 B a table slot — 2^20, 2^24 or 2 n_rows slots — + 4 B a row +
 * n_rows / 4 B of bitmaps), 20 B per miss row (first rows, lengths, offsets) and the scan's scratch; a host batch is staged whole
 * (offsets, bytes + 16, validity, codes).  export stages 12 B a value and the packed bytes; match stages the pattern and, for a host
 * mask, num_values bytes.  Measured once on an MI355X: 1e7 rows of known strings in 0.66 - 0.98 ms.
 * Lock order: the dictionary, then a job context; calls on one dictionary are serial. */
#define TAD_FEATURE_STRING_DICT 4096u /* tad_strdict: a persistent string -> code dictionary on the device, with match masks */
#define TAD_CODE_NONE (-1)            /* tad_strdict_lookup: the string is not in the dictionary */
typedef struct tad_strdict tad_strdict;
int tad_strdict_create(tad_engine *e, uint64_t expected_values, uint64_t expected_bytes, tad_strdict **out);
void tad_strdict_destroy(tad_engine *e, tad_strdict *d);
int tad_strdict_encode(tad_engine *e, tad_strdict *d, const tad_string_column *col, int64_t *codes, uint64_t *new_first_row,
                       uint64_t new_first_row_cap, uint64_t *num_before, uint64_t *num_values);
int tad_strdict_lookup(tad_engine *e, const tad_strdict *d, const tad_string_column *col, int64_t *codes);
int tad_strdict_num_values(tad_engine *e, const tad_strdict *d, uint64_t *num_values);
int tad_strdict_bytes(tad_engine *e, const tad_strdict *d, uint64_t *bytes);
int tad_strdict_export(tad_engine *e, const tad_strdict *d, uint64_t first_code, uint64_t n_values, int64_t *offsets, uint8_t *data,
                       uint64_t data_cap, uint64_t *data_bytes);
int tad_strdict_import(tad_engine *e, tad_strdict *d, uint64_t n_values, const int64_t *offsets, const uint8_t *data);
#define TAD_STR_EQUAL 0            /* the value's bytes are the pattern's bytes */
#define TAD_STR_CONTAINS_NOCASE 1  /* the pattern occurs in the value, ASCII letters compared without case */
int tad_strdict_match(tad_engine *e, const tad_strdict *d, int32_t op, const uint8_t *pattern, uint64_t pattern_len, uint8_t *mask,
                      uint64_t mask_len, tad_mem memory, uint64_t *n_matched);

/* ---- decoding on the device: key ids -> tuples, string codes -> strings (TAD_FEATURE_DICT_DECODE; check tad_features() before calling these) ----
 * The two dictionaries above turn strings into codes and code tuples into key ids; the state calls return result rows that carry key
 * ids.  These two calls go the other way, for ARBITRARY ids and codes — the export calls read a contiguous range only — so a host keeps
 * no table of its keys: it gathers the tuples of the keys its result rows name and decodes their codes, and nothing else crosses the link.
 * Both calls only read the dictionary.
 * tad_keydict_gather: cols[c][i] = column c of key key_id[i] and side[i] = its side (0 = a, 1 = b), for i < n: for every i what the
 * dictionary's export gives for first_key = key_id[i], n_keys = 1.  `memory` says where key_id, every cols[c] and side live; the pointer
 * array cols itself is host memory with n_cols entries, and a NULL entry skips that column; side may be NULL.  Ids may repeat and come in
 * any order.  n == 0 is TAD_OK.  An id >= num_keys — TAD_KEY_SKIP is one — is TAD_ERR_INVALID_ARGUMENT, raised from a device flag after
 * the kernel ran, as the select call raises a code outside its mask; the outputs are unspecified then.  One launch (one lane per id: the
 * record in 16-byte loads, the stores column by column) and one synchronisation; it reads 8 B of id and one record (8 (n_cols + 1) B,
 * rounded up to 16) and writes 8 B per asked column and 1 B of side, per id.  A host call stages the ids and the outputs in job-context
 * workspace (8 B an id, 8 B an id and asked column, 1 B a side), checked against workspace_limit (TAD_ERR_GRID_TOO_LARGE) before anything
 * runs.  Limit: n < 2^32 - 1.
 * tad_strdict_decode: Arrow's layout, as the dictionary's export writes it, for arbitrary codes: offsets[n + 1] starting at 0, and in
 * data the bytes of value codes[0], codes[1], ... packed behind each other.  codes_memory says where codes live, out_memory where offsets
 * and data live, independently: the useful chain is device codes from a gather into host strings.  *data_bytes (may be NULL) is always the
 * bytes needed; offsets == NULL && data == NULL is the size query; a data_cap that is too small is TAD_ERR_INVALID_ARGUMENT with nothing
 * written but *data_bytes.  A code outside [0, num_values) — TAD_CODE_NONE is one — is TAD_ERR_INVALID_ARGUMENT with nothing written to
 * offsets or data: the lengths pass finds it before any byte is copied.  Device codes and offsets are 8-byte aligned; a device data
 * pointer may have any byte alignment, and no byte outside [data, data + *data_bytes) is written.  No validity is produced: a code is a
 * value.  Limits: n < 2^32 - 1; the total bytes are addressed with 64 bits.
 * Cost of a decode.  Three launches and two synchronisations (the total is read between the lengths and the copy): the lengths pass reads
 * 8 B of code and one 16-byte record a row, the scan turns 4 B a row into 8 B a row, the copy reads the record again and the value's
 * ceil(len / 16) aligned 16-byte words of the arena and writes the bytes once, in whole lines: a workgroup assembles the bytes of 256
 * consecutive rows in 16 KiB of LDS, laid out as the destination's 16-byte words, and stores them with aligned 16-byte stores; a tile over
 * 16 KiB is copied string by string, a wavefront each.  Job-context workspace, grow-only and bounded by workspace_limit: 12 B a row
 * (lengths, offsets), the scan's scratch, 8 B a row for host codes, the packed bytes for a host output.  Measured once on an MI355X
 * (DESIGN.md §5): 1e7 codes of 30-byte values, device to device, in 0.36 - 0.87 ms, 0.15 - 0.34 of a copy of the same bytes.
 * Every call on a NULL engine or dictionary is TAD_ERR_INVALID_ARGUMENT without a device and writes nothing.  The ABI stays 13 and no
 * struct grows.  Lock order: the dictionary, then a job context. */
#define TAD_FEATURE_DICT_DECODE 8192u /* tad_keydict_gather, tad_strdict_decode: ids -> tuples and codes -> strings on the device */
int tad_keydict_gather(tad_engine *e, const tad_keydict *d, const uint64_t *key_id, uint64_t n, tad_mem memory, int64_t *const *cols,
                       uint8_t *side /* may be NULL */);
int tad_strdict_decode(tad_engine *e, const tad_strdict *d, const int64_t *codes, uint64_t n, tad_mem codes_memory, int64_t *offsets,
                       uint8_t *data, uint64_t data_cap, tad_mem out_memory, uint64_t *data_bytes /* may be NULL */);

/* ---- retiring dead strings: a string dictionary compacted, its key dictionary recoded (TAD_FEATURE_STRING_RETIRE; check tad_features()
 * before calling these) ----
 * A streaming host keeps a state, a key dictionary and one string dictionary per string key column on the device.  The state and the
 * key dictionary shed their dead keys (the key-retire calls above); the string dictionaries kept a table slot, a record and padded
 * arena bytes for every string ever met: pod names, label sets and external IPs churn, and the match masks, the key selections and
 * every table growth walked all of them.  Three calls close that: which codes do the keys still use, drop the others from the
 * vocabulary, rewrite the keys' columns through the renumbering.  Key ids are untouched throughout, so a state needs no call.
 * The chain, after the state and the key dictionary were compacted: per vocabulary one mark call per column that shares it (accumulate
 * from the second on), one compact with the mask as keep, and ONE recode with every column's remap at the end.  Masks and remaps may stay
 * in device memory from call to call.  Between the first compact and the recode the key dictionary still holds OLD codes: no encode,
 * lookup, select or gather may run in between, and a recode that fails leaves the pair inconsistent (the vocabularies cannot be
 * uncompacted) — restore both from an export taken before the chain.
 * tad_keydict_mark_codes, read-only: used[c] = 1 iff some key of the dictionary holds value c in column col, on either side, else 0;
 * accumulate != 0 ORs into what used holds instead of writing it whole (columns that share one vocabulary).  *n_used (may be NULL) = the
 * ones in used after the call.  `memory` says where used lives.  col outside [0, n_cols) is refused before anything runs.  A key whose
 * value lies outside [0, used_len) is TAD_ERR_INVALID_ARGUMENT, raised from a device flag after the kernel ran, as the select call raises
 * a value outside its mask; used is unspecified then.  An empty dictionary is TAD_OK with used all zero (untouched when accumulating).
 * One lane per key loads the record in 16-byte loads and stores one byte; a second pass counts.  A host used is staged in job-context
 * workspace (used_len bytes), checked against workspace_limit (TAD_ERR_GRID_TOO_LARGE) before anything runs.
 * tad_strdict_compact: keep_len must equal num_values — a stale length is refused, never a short read.  Value c survives iff
 * keep[c] != 0; its new code is the number of survivors below it, so the order of first appearance is kept.  remap (required, keep_len
 * entries in remap_memory; keep lives in keep_memory, at any byte alignment): remap[c] = the new code, or TAD_CODE_NONE for a retired
 * value.  Afterwards the dictionary is what a fresh one holds after an import of the m survivors in new-code order: export, decode,
 * match, lookup and encode behave identically, a retired string looks up to TAD_CODE_NONE, and a retired string that returns in a later
 * encode gets a new code at the end (m, m + 1, ... in order of first appearance).  Records, table and arena are rebuilt at the size a
 * create with expected_values = 2 m and expected_bytes = twice the survivors' padded bytes picks, never below the minimum sizes of
 * create and never larger than before, so tad_strdict_bytes never grows.  The new arena is packed: survivor j starts where the
 * survivors 0 .. j - 1 end, every string 16-byte aligned and zero-padded to a multiple of 16.  Atomic: candidate arrays are filled
 * first and swapped in last; an allocation that fails, workspace over workspace_limit (TAD_ERR_GRID_TOO_LARGE) or a HIP error leaves the
 * dictionary exactly as it was (remap is unspecified then).  When nothing is retired the call is TAD_OK, remap is the identity and
 * nothing is reallocated or moved.  m == 0 leaves an empty dictionary of minimum size that takes an import again.  stats may be NULL.
 * How: survivor flags and padded lengths (in 16-byte units) are scanned into new codes and new arena offsets; one lane per old value
 * writes remap and a survivor's new record; the bytes move in whole aligned 16-byte words — a workgroup takes 256 consecutive survivors,
 * whose destination is contiguous, its lanes walk the destination's words in order and find their row by a search in LDS (whole lines
 * out, a gather in), a survivor over 4 KiB is copied by the wavefronts in turn —; the fresh table is filled from the old table's slots
 * and the remap, no string is read or hashed.  Workspace: 32 B a value before the call, the scan's scratch, 1 B a value for a host keep
 * and 8 B a value for a host remap.  Two synchronisations.
 * tad_keydict_recode: for every term t, every key's value v in column term_col[t] becomes remaps[t][v].  The pointer arrays term_col,
 * remaps and remap_len are host memory with n_terms (0..8) entries; the remaps themselves live in `memory`.  Key ids, sides and the
 * other columns stay as they are.  TAD_ERR_INVALID_ARGUMENT with the dictionary unchanged: a value outside [0, remap_len[t]); a value
 * mapped to TAD_CODE_NONE — a key still uses a retired string —; a column named twice; two keys whose recoded tuples are equal (found
 * while the fresh table is built).  Fresh records and a fresh table of the current sizes are filled and swapped in last.  With
 * n_terms == 0, or identity remaps only, the dictionary is untouched.  Afterwards an encode or a lookup of a tuple written in NEW codes
 * gives the key's old id, and export and gather return the new codes.  *num_keys (may be NULL) = the keys held.  A host call stages its
 * remaps in job-context workspace (8 B an entry), checked against workspace_limit before anything runs.
 * Every call on a NULL engine or dictionary is TAD_ERR_INVALID_ARGUMENT without a device and writes nothing.  The ABI version does not
 * change and no struct grows.  Lock order: the dictionary, then a job context; calls on one dictionary are serial.  What it costs
 * against the export / select / import round trip: DESIGN.md §5, tools/strdict_retire_bench.py. */
#define TAD_FEATURE_STRING_RETIRE 16384u /* tad_keydict_mark_codes, tad_strdict_compact, tad_keydict_recode: dead strings dropped, codes renumbered */
typedef struct {
  uint64_t values_before;            /* num_values at entry */
  uint64_t values_after;             /* surviving values m */
  uint64_t bytes_before;             /* tad_strdict_bytes at entry ... */
  uint64_t bytes_after;              /* ... and at exit */
  uint64_t arena_used_before;        /* padded bytes of the values held at entry ... */
  uint64_t arena_used_after;         /* ... and of the survivors */
  int32_t job_context;
  int32_t reserved;
  float ms_total;                    /* HIP events */
  float reserved1;
} tad_strdict_compact_stats;
int tad_keydict_mark_codes(tad_engine *e, const tad_keydict *d, int32_t col, int32_t accumulate, uint8_t *used, uint64_t used_len,
                           tad_mem memory, uint64_t *n_used /* may be NULL */);
int tad_strdict_compact(tad_engine *e, tad_strdict *d, const uint8_t *keep, uint64_t keep_len, tad_mem keep_memory, int64_t *remap,
                        tad_mem remap_memory, tad_strdict_compact_stats *stats /* may be NULL */);
int tad_keydict_recode(tad_engine *e, tad_keydict *d, int32_t n_terms, const int32_t *term_col, const int64_t *const *remaps,
                       const uint64_t *remap_len, tad_mem memory, uint64_t *num_keys /* may be NULL */);

/* ---- LIKE patterns with % and _ on a string dictionary (TAD_FEATURE_STRING_LIKE; check tad_features() before calling this) ----
 * The job's label filter is ilike(labels, '%label%') with the user's text in the middle, and the reference's own example label,
 * "test_key":"test_value", holds a wildcard: _ is legal in Kubernetes label keys and values and matches any one character in a LIKE
 * pattern.  The match call above knows no wildcard, so such a job exported every label string to the host and ran a regex over them.
 * tad_strdict_like evaluates the whole pattern language on the device instead, one lane per value.
 * The language (theia_amd/csrc/tad_like.h holds it, compile step and matcher, for host and device): \ followed by a byte makes that byte
 * a literal, and \ as the last byte is a literal backslash; % matches any run of bytes, the empty run included, and %% is %; _ matches
 * exactly one character; every other byte is a literal.  The pattern matches the WHOLE value — it is anchored at both ends, so a
 * substring search is '%text%' — and % and _ also match a newline.  An empty pattern selects "" alone.  With TAD_LIKE_NOCASE the
 * literals (escaped ones included) and the value's bytes are compared after folding 'A'..'Z' to 'a'..'z' and nothing else.  One
 * character is the byte at the position, whatever it is, and every byte 0x80..0xBF that follows it: one code point on well-formed UTF-8.
 * The place a % retries from advances by the same step.  This is what the batch job's regex (anomaly_detection.py: _like_regex) decides,
 * with the two differences of the case-folded substring operation: no Unicode case folding, and Python's re.IGNORECASE lets k, s and i
 * match U+212A, U+017F, U+0130 and U+0131, which no byte fold does.
 * The call, read-only: mask[c] = 1 iff the pattern matches value c, else 0.  mask_len must equal num_values — a stale length is refused
 * and the mask left untouched, never a short write.  `memory` says where mask lives; the pattern is host memory, pattern_len <= 1024;
 * *n_matched may be NULL.  A flag bit other than TAD_LIKE_NOCASE is refused.  An empty dictionary is TAD_OK.  A NULL engine is
 * TAD_ERR_INVALID_ARGUMENT without a device and writes nothing.  The mask is ready for the key selection and the row mask calls in device
 * memory, as the match call's is.
 * How: the host compiles the pattern into at most 1024 two-byte tokens and the least value length a match needs; the kernel holds the
 * tokens in LDS, answers a shorter value from its record, and reads a value's bytes as aligned 16-byte words of the arena, the word under
 * the cursor held in registers.  The matcher is iterative and keeps ONE backtrack point, the last % met.  Cost: one launch and one
 * synchronisation; per value one 16-byte record and its bytes once per pass — worst case value length x pattern length steps per value
 * ('%a%a%a%b' on a long run of a), against value length for a pattern whose literals rarely begin to match.  A wildcard-free
 * substring search is cheaper through TAD_STR_CONTAINS_NOCASE, which compares eight bytes a step.  Job-context workspace, grow-only and
 * bounded by workspace_limit: the staged program (2 KiB) and, for a host mask, num_values bytes.  The ABI stays 13 and no struct grows.
 * Lock order: the dictionary, then a job context; calls on one dictionary are serial.  Measured once (DESIGN.md §5,
 * tools/strdict_like_bench.py): 1e7 label sets of 87 bytes on average in 2.8 - 3.3 ms, 3.0 times the substring search on the same literal. */
#define TAD_FEATURE_STRING_LIKE 32768u /* tad_strdict_like: LIKE / ilike patterns with % and _ matched on the device */
#define TAD_LIKE_NOCASE 1u             /* flags: compare after folding 'A'..'Z' to 'a'..'z' (ilike) */
int tad_strdict_like(tad_engine *e, const tad_strdict *d, const uint8_t *pattern, uint64_t pattern_len, uint32_t flags,
                     uint8_t *mask, uint64_t mask_len, tad_mem memory, uint64_t *n_matched /* may be NULL */);

/* Stage counter for Status.CompletedStages / TotalStages (controller.go:426-453); callable while
 * tad_run executes on another thread.  tad_progress: the sum over the jobs in flight (with none: the job that finished last).
 * tad_job_progress (ABI 12): the job whose tad_job.id equals `id`; *total = 0 when no such job is in flight (finished or not yet
 * admitted).  tad_jobs_in_flight: contexts busy right now. */
int tad_progress(tad_engine *e, int32_t *done, int32_t *total);
int tad_job_progress(tad_engine *e, const char *id, int32_t *done, int32_t *total);
int tad_jobs_in_flight(tad_engine *e);

/* ---- per-series entry points: the reference's pure functions, one key, values in time order.
 * Same device kernels as tad_run (a 1-key series table).  x, out arrays are HOST memory. ---- */
/* calculate_ewma (:146-165): out[n]. */
int tad_series_ewma(tad_engine *e, const uint64_t *x, uint64_t n, double alpha, double *out);
/* calculate_ewma_anomaly (:168-212): verdict[n] in {0,1}. has_stddev == 0 models stddev None. */
int tad_series_ewma_anomaly(tad_engine *e, const uint64_t *x, uint64_t n, double alpha,
                            int has_stddev, double stddev, uint8_t *verdict);
/* stddev_samp over the series (:674-684). *has_stddev = 0 when n < 2 (Spark returns null). */
int tad_series_stddev(tad_engine *e, const uint64_t *x, uint64_t n, int *has_stddev, double *stddev);
/* calculate_dbscan_anomaly (:325-349): verdict[n] = (label == -1). */
int tad_series_dbscan_anomaly(tad_engine *e, const uint64_t *x, uint64_t n, double eps,
                              int min_samples, uint8_t *verdict);
/* DropDetection.end_partition (drop_detection_udf.py:42-56) on one partition: *has_result = 0 when n < min_samples. */
int tad_series_drop(tad_engine *e, const uint64_t *x, uint64_t n, double nsigma, int min_samples, int *has_result,
                    double *mean, double *stddev, uint8_t *verdict);
/* calculate_arima (:215-264): out[n]; *has_result = 0 reproduces the `return None` cases. */
int tad_series_arima(tad_engine *e, const uint64_t *x, uint64_t n, int maxiter, int *has_result,
                     double *out);
/* calculate_arima_anomaly (:267-309): verdict[n]; *n_verdict = 1 and verdict[0] = 0 when ARIMA
 * returned None (:284-287). */
int tad_series_arima_anomaly(tad_engine *e, const uint64_t *x, uint64_t n, int maxiter,
                             int has_stddev, double stddev, uint8_t *verdict, uint64_t *n_verdict);

/* ---- deterministic synthetic flow table, generated straight into HBM ----
 * Rows [first_row, first_row + n_rows) of the table (seed, num_keys, n_buckets); the three output
 * arrays are DEVICE memory with n_rows entries.  Definition: theia_amd/csrc/tad_synth.hip. */
int tad_synth_generate(tad_engine *e, uint64_t seed, uint64_t first_row, uint64_t n_rows,
                       uint64_t num_keys, uint64_t n_buckets, uint64_t *key_id,
                       int64_t *flow_end_s, uint64_t *value);

/* ---- device memory helpers for hosts without a HIP binding (cgo) ---- */
int tad_device_alloc(tad_engine *e, uint64_t bytes, void **ptr);
int tad_device_free(tad_engine *e, void *ptr);
int tad_copy_to_device(tad_engine *e, void *dst, const void *src, uint64_t bytes);
int tad_copy_to_host(tad_engine *e, void *dst, const void *src, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* THEIA_TAD_H */
