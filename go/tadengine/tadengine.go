// Package tadengine is the cgo binding of libtad_mi355x.so (include/tad.h) for theia-manager.
//
// STATUS: written against include/tad.h but NOT compiled or tested here — this build image has no
// Go toolchain (`go version`: not found).  The identical C ABI is exercised by the ctypes binding
// (theia_amd/_capi.py), tests/test_capi_abi.py and the C driver tools/capi_driver.c.
//
// It replaces the SparkApplication launch of
// pkg/controller/anomalydetector/controller.go:525-698 (startSparkApplication) with an in-process
// call: the controller reads the job's columns from ClickHouse, dictionary-encodes the key columns,
// calls Engine.Run, and inserts the returned rows into default.tadetector.
package tadengine

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../theia_amd/lib -ltad_mi355x -Wl,-rpath,${SRCDIR}/../../theia_amd/lib
#include <stdlib.h>
#include <string.h>
#include "tad.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"math"
	"runtime"
	"sync"
	"unsafe"
)

// KeySkip marks a row (or its second key) that the SQL predicates reject.
const KeySkip = ^uint64(0)

type Algo int

const (
	EWMA   Algo = C.TAD_ALGO_EWMA
	ARIMA  Algo = C.TAD_ALGO_ARIMA
	DBSCAN Algo = C.TAD_ALGO_DBSCAN
	Drop   Algo = C.TAD_ALGO_DROP // abnormal-traffic-drop detector (snowflake/udfs/udfs/drop_detection)
)

type AggFlow int

const (
	AggNone     AggFlow = C.TAD_AGG_NONE
	AggPod      AggFlow = C.TAD_AGG_POD
	AggSvc      AggFlow = C.TAD_AGG_SVC
	AggExternal AggFlow = C.TAD_AGG_EXTERNAL
)

// IllegalArgument mirrors illeagelArguementError (controller.go:505-514): the job is marked FAILED
// and not retried.
type IllegalArgument struct{ Msg string }

func (e IllegalArgument) Error() string { return e.Msg }

// Engine owns one GPU.  Run may be called from the controller's 4 workers concurrently
// (controller.go:199-201): each call takes one of the engine's job contexts (own HIP stream and workspace, tad.h ABI 12), so up
// to MaxJobsInFlight jobs overlap on the GPU; further callers wait inside the library.
type Engine struct{ h *C.tad_engine }

// Plan mirrors tad_plan (tad.h, ABI 12): plan overrides of an engine, every field 0 = the engine decides — what the controller
// uses.  Tests and A/B measurements force a strategy with it; the library reads no environment variable.  A Go struct, not
// C.tad_plan: cgo types are private to this package, callers in other packages could not construct one.
type Plan struct {
	Stage0        int32  // 1 = direct atomic scatter, 2 = partition + LDS tiles whatever the batch size
	PartitionPass int32  // 1 = sort-by-tile pass B, 2 = write-combining pass B, 3 = write-combining with 64-byte sectors only
	Histogram     int32  // 1 = exact per-workgroup histogram in pass A
	Sparse        int32  // 1 = never, 2 = always the sort-based Stage 0 for sparse tables
	SparseClasses int32  // 1 = always run a sparse table as length classes of keys
	EwmaEmit      int32  // 1 = lane-per-key emit for the EWMA job
	EwmaEmitRows  uint32 // LDS rows per wavefront of the staged EWMA emit (<= 4096)
	TileCells     int32  // 1 = 8-byte tile cells in the settle mode of DBSCAN jobs with max
	SparseSort    int32  // sparse tables: 1 = always the LSD radix sort, 2 = the partition pass + LDS sort wherever its plan fits (ABI 9)
}

func (p Plan) c() C.tad_plan {
	return C.tad_plan{stage0: C.int32_t(p.Stage0), partition_pass: C.int32_t(p.PartitionPass), histogram: C.int32_t(p.Histogram),
		sparse: C.int32_t(p.Sparse), sparse_classes: C.int32_t(p.SparseClasses), ewma_emit: C.int32_t(p.EwmaEmit),
		ewma_emit_rows: C.uint32_t(p.EwmaEmitRows), tile_cells: C.int32_t(p.TileCells), sparse_sort: C.int32_t(p.SparseSort)}
}

func NewEngine(device int) (*Engine, error) { return NewEngineWithPlan(device, Plan{}) }

// NewEngineWithPlan creates the engine with plan overrides in tad_engine_opts.plan and the default number of job contexts (4).
func NewEngineWithPlan(device int, plan Plan) (*Engine, error) { return NewEngineWithOptions(device, plan, 0) }

// NewEngineWithOptions: maxJobsInFlight = tad_engine_opts.max_jobs_in_flight (0 = 4, the controller's worker count; 1 = jobs serialise).
func NewEngineWithOptions(device int, plan Plan, maxJobsInFlight int) (*Engine, error) {
	// the header this file was compiled against and the library the process loaded must be the same ABI (struct layouts!)
	if v := int(C.tad_abi_version()); v != int(C.TAD_ABI_VERSION) {
		return nil, fmt.Errorf("libtad_mi355x.so ABI %d != tad.h ABI %d", v, int(C.TAD_ABI_VERSION))
	}
	opts := C.tad_engine_opts{device: C.int32_t(device), plan: plan.c(), max_jobs_in_flight: C.int32_t(maxJobsInFlight)}
	var h *C.tad_engine
	if rc := C.tad_engine_create(&opts, &h); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_engine_create: %s (code %d)", C.GoString(C.tad_last_error(nil)), int(rc))
	}
	e := &Engine{h: h}
	runtime.SetFinalizer(e, func(e *Engine) { e.Close() })
	return e, nil
}

// SetPlan replaces the engine's plan overrides; takes effect with the next job.
func (e *Engine) SetPlan(p Plan) error {
	cp := p.c()
	if rc := C.tad_engine_set_plan(e.h, &cp); rc != C.TAD_OK {
		return fmt.Errorf("tad_engine_set_plan: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return nil
}

func (e *Engine) Close() {
	if e.h != nil {
		C.tad_engine_destroy(e.h)
		e.h = nil
	}
}

// Job mirrors the SparkApplication argument vector (controller.go:526-623).
type Job struct {
	Algo      Algo
	AggFlow   AggFlow
	StartTime int64 // epoch seconds, 0 = unset (Spec.StartInterval)
	EndTime   int64 // epoch seconds, 0 = unset (Spec.EndInterval)
	ID        string
	// DBSCAN parameters (tad_job.dbscan_eps / dbscan_min_samples): 0 = the reference's eps = 250000000, min_samples = 4
	DBSCANEps        float64
	DBSCANMinSamples int32
	// ARIMA parameter (tad_job.arima_maxiter): 0 = statsmodels' maxiter = 50
	ARIMAMaxIter int32
}

// Columns is one batch of flow rows after dictionary encoding; all slices have the same length.
// The key and the time columns may instead come as 32-bit slices, read by the engine at that width (tad.h, TAD_FLAG_KEY_U32 /
// TAD_FLAG_TIME_U32): KeyID32 / KeyID2_32 replace KeyID / KeyID2 (TAD_KEY_SKIP32 = the row does not take part; NumKeys < 2^32 - 1),
// FlowEndS32 / FlowStartS32 replace FlowEndS / FlowStartS (ClickHouse DateTime: unsigned epoch seconds).  Set one form per column pair.
type Columns struct {
	KeyID        []uint64
	KeyID2       []uint64 // pod mode only (inbound/outbound UNION ALL), else nil
	FlowEndS     []int64
	FlowStartS   []int64 // nil unless StartTime is set
	Value        []uint64
	NumKeys      uint64
	KeyHist      *KeyHist // optional: FactorizeHist's by-product for THIS batch (Stage 0 then does not count the key column again)
	KeyID32      []uint32 // optional 32-bit form of KeyID
	KeyID2_32    []uint32 // optional 32-bit form of KeyID2
	FlowEndS32   []uint32 // optional 32-bit form of FlowEndS
	FlowStartS32 []uint32 // optional 32-bit form of FlowStartS
}

// KeyHist is tad_key_hist (tad.h, ABI 12): the key-bin histogram of a factorised batch per Stage-0 workgroup.  The bins live in device
// memory (TAD_KEY_HIST_BYTES, allocated by FactorizeHist, released by Free); the struct itself is C memory so that tad_columns may point to it.
type KeyHist struct{ c *C.tad_key_hist }

func (h *KeyHist) Valid() bool { return h != nil && h.c != nil && h.c.n_rows != 0 }

func (h *KeyHist) Free(e *Engine) {
	if h != nil && h.c != nil {
		C.tad_device_free(e.h, unsafe.Pointer(h.c.bins))
		C.free(unsafe.Pointer(h.c))
		h.c = nil
	}
}

// Row is the mode-independent part of one tadetector row (create_table.sh:363-384).
type Row struct {
	KeyID      uint64
	FlowEndS   int64
	Throughput float64
	AlgoCalc   float64
	StdDev     float64
}

type Stats struct {
	RowsIn, RowsUsed, Keys, Points, Anomalies, KeysNoResult uint64
	ArimaNanFits                                             uint64 // ARIMA fits voided by a non-finite likelihood (tad.h: tad_stats.arima_nan_fits)
	MsTotal                                                  float32
	Stage0Path                                               int32 // how Stage 0 ran (tad.h: tad_stats.stage0_path), for the controller's logs
	HostSyncs                                                int32 // host synchronisations of the job (tad.h: tad_stats.host_syncs): 3, or 2 with a lattice hint
	JobContext                                               int32 // which of the engine's job contexts ran it (tad.h: tad_stats.job_context, ABI 12)
	ArimaRelaunches                                          int32 // times the ARIMA fit yielded to other jobs' whole-CU kernels and was relaunched (tad_stats.arima_relaunches)
}

// cColumn copies a Go slice into C memory: cgo forbids handing Go pointers nested in a C struct, and the
// library stages host columns to the GPU anyway.  A production binding would read ClickHouse blocks
// straight into C/pinned buffers instead of Go slices.
func cColumn[T uint64 | int64 | uint32](s []T) unsafe.Pointer {
	if len(s) == 0 {
		return nil
	}
	var z T
	n := C.size_t(len(s) * int(unsafe.Sizeof(z)))
	p := C.malloc(n)
	C.memcpy(p, unsafe.Pointer(&s[0]), n)
	return p
}

var narrowOnce sync.Once
var narrowOK bool

// columnBuffers copies the batch's columns into C memory: key, key2, flow end, flow start, value (nil where absent), the row count
// and the narrow-column flags of tad_job.  32-bit slices are only handed over once the library has said it reads them
// (tad_features): a library that predates the flags would ignore them and misread the columns.
func columnBuffers(cols Columns) ([]unsafe.Pointer, int, C.uint32_t, error) {
	if (cols.KeyID32 != nil && cols.KeyID != nil) || (cols.FlowEndS32 != nil && cols.FlowEndS != nil) ||
		(cols.KeyID2_32 != nil && cols.KeyID2 != nil) || (cols.FlowStartS32 != nil && cols.FlowStartS != nil) ||
		(cols.KeyID2_32 != nil && cols.KeyID32 == nil) || (cols.KeyID2 != nil && cols.KeyID32 != nil) ||
		(cols.FlowStartS32 != nil && cols.FlowEndS32 == nil) || (cols.FlowStartS != nil && cols.FlowEndS32 != nil) {
		return nil, 0, 0, errors.New("tadengine: set either the 64-bit or the 32-bit form of the key (time) columns")
	}
	var flags C.uint32_t
	if cols.KeyID32 != nil || cols.FlowEndS32 != nil {
		narrowOnce.Do(func() { narrowOK = C.tad_features()&C.TAD_FEATURE_NARROW_COLUMNS != 0 })
		if !narrowOK {
			return nil, 0, 0, errors.New("tadengine: libtad_mi355x.so does not read 32-bit columns (TAD_FEATURE_NARROW_COLUMNS)")
		}
	}
	n := len(cols.KeyID)
	bufs := []unsafe.Pointer{cColumn(cols.KeyID), cColumn(cols.KeyID2), cColumn(cols.FlowEndS), cColumn(cols.FlowStartS), cColumn(cols.Value)}
	if cols.KeyID32 != nil {
		n = len(cols.KeyID32)
		bufs[0], bufs[1] = cColumn(cols.KeyID32), cColumn(cols.KeyID2_32)
		flags |= C.TAD_FLAG_KEY_U32
	}
	if cols.FlowEndS32 != nil {
		bufs[2], bufs[3] = cColumn(cols.FlowEndS32), cColumn(cols.FlowStartS32)
		flags |= C.TAD_FLAG_TIME_U32
	}
	lens := []int{len(cols.KeyID2) + len(cols.KeyID2_32), len(cols.FlowEndS) + len(cols.FlowEndS32), len(cols.FlowStartS) + len(cols.FlowStartS32), len(cols.Value)}
	for i, m := range lens {
		if m != n && (i == 1 || i == 3 || m != 0) {
			freeBuffers(bufs)
			return nil, 0, 0, errors.New("tadengine: columns differ in length")
		}
	}
	return bufs, n, flags, nil
}

func freeBuffers(bufs []unsafe.Pointer) {
	for _, p := range bufs {
		if p != nil {
			C.free(p)
		}
	}
}

// Run replaces one SparkApplication run (anomaly_detection.py:647-710).  An empty result means the caller
// writes the "NO ANOMALY DETECTED" sentinel row (anomaly_detection.py:395-420).
func (e *Engine) Run(job Job, cols Columns) ([]Row, Stats, error) {
	var st Stats
	bufs, n, narrow, err := columnBuffers(cols)
	if err != nil {
		return nil, st, err
	}
	defer freeBuffers(bufs)
	var cj C.tad_job
	cj.flags = narrow
	cj.algo = C.tad_algo(job.Algo)
	cj.agg_flow = C.tad_agg_flow(job.AggFlow)
	cj.value_op = C.TAD_OP_AUTO
	cj.dbscan_eps = C.double(job.DBSCANEps)
	cj.dbscan_min_samples = C.int32_t(job.DBSCANMinSamples)
	cj.arima_maxiter = C.int32_t(job.ARIMAMaxIter)
	cj.start_time = C.int64_t(job.StartTime)
	cj.end_time = C.int64_t(job.EndTime)
	id := []byte(job.ID)
	if len(id) > 63 {
		id = id[:63]
	}
	for i, b := range id {
		cj.id[i] = C.char(b)
	}
	var cc C.tad_columns
	cc.n_rows = C.uint64_t(n)
	cc.num_keys = C.uint64_t(cols.NumKeys)
	cc.memory = C.TAD_MEM_HOST
	cc.key_id = (*C.uint64_t)(bufs[0])
	cc.key_id2 = (*C.uint64_t)(bufs[1])
	cc.flow_end_s = (*C.int64_t)(bufs[2])
	cc.flow_start_s = (*C.int64_t)(bufs[3])
	cc.value = (*C.uint64_t)(bufs[4])
	if cols.KeyHist.Valid() {
		cc.key_hist = cols.KeyHist.c // C memory: no Go pointer inside the struct handed to C
	}

	var res *C.tad_result
	rc := C.tad_run(e.h, &cj, &cc, C.TAD_MEM_HOST, &res)
	if rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, st, IllegalArgument{msg}
		}
		return nil, st, fmt.Errorf("tad_run: %s (code %d)", msg, int(rc))
	}
	defer C.tad_result_free(e.h, res)
	a := int(res.n_rows)
	rows := make([]Row, a)
	if a > 0 {
		k := unsafe.Slice((*uint64)(unsafe.Pointer(res.key_id)), a)
		t := unsafe.Slice((*int64)(unsafe.Pointer(res.flow_end_s)), a)
		x := unsafe.Slice((*float64)(unsafe.Pointer(res.throughput)), a)
		c := unsafe.Slice((*float64)(unsafe.Pointer(res.algo_calc)), a)
		s := unsafe.Slice((*float64)(unsafe.Pointer(res.stddev)), a)
		for i := range rows {
			rows[i] = Row{k[i], t[i], x[i], c[i], s[i]}
		}
	}
	st = Stats{uint64(res.stats.rows_in), uint64(res.stats.rows_used), uint64(res.stats.n_keys), uint64(res.stats.n_points),
		uint64(res.stats.n_anomalies), uint64(res.stats.keys_no_result), uint64(res.stats.arima_nan_fits), float32(res.stats.ms_total),
		int32(res.stats.stage0_path), int32(res.stats.host_syncs), int32(res.stats.job_context), int32(res.stats.arima_relaunches)}
	return rows, st, nil
}

// Point is one aggregated (key, flowEndSeconds) point of Stage 0 (tad_aggregate): the GROUP BY the reference pushes
// into ClickHouse, with the full UInt64 aggregate.  Row-sharded ingest across several GPUs aggregates each slice
// with Aggregate, routes the points to the engine that owns the key, and calls Run on the partial points.
type Point struct {
	KeyID    uint64
	FlowEndS int64
	Value    uint64
}

func (e *Engine) Aggregate(job Job, cols Columns) ([]Point, error) {
	bufs, n, narrow, err := columnBuffers(cols)
	if err != nil {
		return nil, err
	}
	defer freeBuffers(bufs)
	var cj C.tad_job
	cj.flags = narrow
	cj.agg_flow = C.tad_agg_flow(job.AggFlow)
	cj.value_op = C.TAD_OP_AUTO
	cj.start_time = C.int64_t(job.StartTime)
	cj.end_time = C.int64_t(job.EndTime)
	var cc C.tad_columns
	cc.n_rows = C.uint64_t(n)
	cc.num_keys = C.uint64_t(cols.NumKeys)
	cc.memory = C.TAD_MEM_HOST
	cc.key_id = (*C.uint64_t)(bufs[0])
	cc.key_id2 = (*C.uint64_t)(bufs[1])
	cc.flow_end_s = (*C.int64_t)(bufs[2])
	cc.flow_start_s = (*C.int64_t)(bufs[3])
	cc.value = (*C.uint64_t)(bufs[4])
	var pts *C.tad_points
	if rc := C.tad_aggregate(e.h, &cj, &cc, C.TAD_MEM_HOST, &pts); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_aggregate: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	defer C.tad_points_free(e.h, pts)
	m := int(pts.n_points)
	out := make([]Point, m)
	if m > 0 {
		k := unsafe.Slice((*uint64)(unsafe.Pointer(pts.key_id)), m)
		t := unsafe.Slice((*int64)(unsafe.Pointer(pts.flow_end_s)), m)
		v := unsafe.Slice((*uint64)(unsafe.Pointer(pts.value)), m)
		for i := range out {
			out[i] = Point{k[i], t[i], v[i]}
		}
	}
	return out, nil
}

// ShardRows buckets device-resident rows by the owner of their key (owner = key mod world, local id = key / world) for
// the all-to-all(v) of row-sharded multi-GPU ingest (tad_shard_rows).  key, flowEnd, value and the three outputs are
// DEVICE pointers to n 8-byte elements each (AllocDevice); the returned counts are the rows per destination rank.
func (e *Engine) ShardRows(key, flowEnd, value unsafe.Pointer, n uint64, world uint32, outKey, outFlowEnd, outValue unsafe.Pointer) ([]uint64, error) {
	var cc C.tad_columns
	cc.n_rows = C.uint64_t(n)
	cc.memory = C.TAD_MEM_DEVICE
	cc.key_id = (*C.uint64_t)(key)
	cc.flow_end_s = (*C.int64_t)(flowEnd)
	cc.value = (*C.uint64_t)(value)
	if world == 0 {
		return nil, fmt.Errorf("tad_shard_rows: world must be >= 1")
	}
	counts := make([]uint64, world)
	if rc := C.tad_shard_rows(e.h, &cc, C.uint32_t(world), (*C.uint64_t)(outKey), (*C.int64_t)(outFlowEnd), (*C.uint64_t)(outValue),
		(*C.uint64_t)(unsafe.Pointer(&counts[0]))); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_shard_rows: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return counts, nil
}

// Factorize turns the rows' GROUP BY key tuples — dictionary codes of the string columns, ports, protocol, flowStartSeconds: up to
// eight int64 columns (anomaly_detection.py:52-137) — into dense key ids in order of first appearance on the GPU (tad_factorize).
// keep (nil = every row) marks the rows the SQL's predicates accept; the others get KeySkip.  colsB / keepB: the second tuple of
// every row in pod mode (the outbound view of the UNION ALL, :556-565), ids into the second return value.  firstRow[k] = the virtual
// row (i for side a, n + i for side b) where key k first appears: the caller reads the key's column values there.
func (e *Engine) Factorize(colsA [][]int64, keepA []byte, colsB [][]int64, keepB []byte) (keyID, keyID2, firstRow []uint64, err error) {
	keyID, keyID2, firstRow, _, err = e.factorize(colsA, keepA, colsB, keepB, false)
	return
}

// FactorizeHist is Factorize plus the key-bin histogram of the ids (tad_factorize_hist): put it into Columns.KeyHist of the job over the
// same rows and Stage 0 sizes its partition regions from it instead of reading the key column a second time.  Free it after the job.
func (e *Engine) FactorizeHist(colsA [][]int64, keepA []byte, colsB [][]int64, keepB []byte) (keyID, keyID2, firstRow []uint64, hist *KeyHist, err error) {
	return e.factorize(colsA, keepA, colsB, keepB, true)
}

func (e *Engine) factorize(colsA [][]int64, keepA []byte, colsB [][]int64, keepB []byte, withHist bool) (keyID, keyID2, firstRow []uint64, hist *KeyHist, err error) {
	if len(colsA) < 1 || len(colsA) > 8 || (colsB != nil && len(colsB) != len(colsA)) {
		return nil, nil, nil, nil, errors.New("tadengine: 1..8 key columns, the same number on both sides")
	}
	n := len(colsA[0])
	sides := 1
	if colsB != nil {
		sides = 2
	}
	var bufs []unsafe.Pointer
	defer func() {
		for _, p := range bufs {
			if p != nil {
				C.free(p)
			}
		}
	}()
	ptrs := func(cols [][]int64) *unsafe.Pointer {
		arr := (*[8]unsafe.Pointer)(C.malloc(C.size_t(8 * unsafe.Sizeof(unsafe.Pointer(nil)))))
		bufs = append(bufs, unsafe.Pointer(arr))
		for c, col := range cols {
			if len(col) != n {
				return nil
			}
			arr[c] = cColumn(col)
			bufs = append(bufs, arr[c])
		}
		return &arr[0]
	}
	mask := func(m []byte) unsafe.Pointer {
		if m == nil {
			return nil
		}
		p := C.CBytes(m)
		bufs = append(bufs, p)
		return p
	}
	var kc C.tad_key_columns
	kc.n_rows = C.uint64_t(n)
	kc.n_cols = C.int32_t(len(colsA))
	kc.memory = C.TAD_MEM_HOST
	pa := ptrs(colsA)
	if pa == nil || (keepA != nil && len(keepA) != n) || (keepB != nil && len(keepB) != n) {
		return nil, nil, nil, nil, errors.New("tadengine: key columns and masks differ in length")
	}
	kc.cols_a = (**C.int64_t)(unsafe.Pointer(pa))
	kc.keep_a = (*C.uint8_t)(mask(keepA))
	if colsB != nil {
		pb := ptrs(colsB)
		if pb == nil {
			return nil, nil, nil, nil, errors.New("tadengine: key columns differ in length")
		}
		kc.cols_b = (**C.int64_t)(unsafe.Pointer(pb))
		kc.keep_b = (*C.uint8_t)(mask(keepB))
	}
	keyID = make([]uint64, n)
	firstRow = make([]uint64, n*sides)
	var k2 *C.uint64_t
	if colsB != nil {
		keyID2 = make([]uint64, n)
		if n > 0 {
			k2 = (*C.uint64_t)(unsafe.Pointer(&keyID2[0]))
		}
	}
	if n == 0 {
		return keyID, keyID2, firstRow[:0], nil, nil
	}
	var nk C.uint64_t
	if withHist {
		hist = &KeyHist{c: (*C.tad_key_hist)(C.calloc(1, C.size_t(unsafe.Sizeof(C.tad_key_hist{}))))}
		var bins unsafe.Pointer
		if rc := C.tad_device_alloc(e.h, C.uint64_t(C.TAD_KEY_HIST_BYTES), &bins); rc != C.TAD_OK {
			C.free(unsafe.Pointer(hist.c))
			return nil, nil, nil, nil, fmt.Errorf("tad_device_alloc: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
		}
		hist.c.bins = (*C.uint32_t)(bins)
		if rc := C.tad_factorize_hist(e.h, &kc, (*C.uint64_t)(unsafe.Pointer(&keyID[0])), k2, (*C.uint64_t)(unsafe.Pointer(&firstRow[0])),
			C.uint64_t(len(firstRow)), &nk, hist.c); rc != C.TAD_OK {
			hist.Free(e)
			return nil, nil, nil, nil, fmt.Errorf("tad_factorize_hist: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
		}
		return keyID, keyID2, firstRow[:int(nk)], hist, nil
	}
	if rc := C.tad_factorize(e.h, &kc, (*C.uint64_t)(unsafe.Pointer(&keyID[0])), k2, (*C.uint64_t)(unsafe.Pointer(&firstRow[0])),
		C.uint64_t(len(firstRow)), &nk); rc != C.TAD_OK {
		return nil, nil, nil, nil, fmt.Errorf("tad_factorize: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return keyID, keyID2, firstRow[:int(nk)], nil, nil
}


// EncodeStrings turns one string column of a batch — in Arrow's layout, what clickhouse-go's column-oriented block API and the
// Arrow Go reader both hand out: n+1 offsets into a byte slice — into dictionary codes on the GPU (tad.h: tad_encode_strings, ABI 10):
// codes[i] = id of row i's string in order of first appearance, firstRow[k] = the row where value k first appears (the host reads
// the dictionary's strings there, evaluates the job's string predicates on them and passes the codes on to Factorize).
// validity may be nil (no nulls); a null row encodes like "".
func (e *Engine) EncodeStrings(offsets []int32, data []byte, validity []byte) (codes []int64, firstRow []uint64, err error) {
	if len(offsets) == 0 {
		return nil, nil, errors.New("tadengine: offsets hold n + 1 entries")
	}
	n := len(offsets) - 1
	codes = make([]int64, n)
	firstRow = make([]uint64, n)
	if n == 0 {
		return codes, firstRow, nil
	}
	// sc is Go memory that HOLDS Go pointers (offsets, data, validity).  cgo only accepts that when the pointed-to memory is pinned
	// ("cgo argument has Go pointer to unpinned Go pointer" otherwise, with the default cgocheck): the three slices are pinned for
	// the duration of the call (runtime.Pinner, Go >= 1.21) — the column's bytes stay zero-copy, unlike Factorize's small id columns,
	// which are copied into C memory.  codes and firstRow are passed directly and hold no pointers.
	var pin runtime.Pinner
	defer pin.Unpin()
	var sc C.tad_string_column
	sc.n_rows = C.uint64_t(n)
	pin.Pin(&offsets[0])
	sc.offsets = unsafe.Pointer(&offsets[0])
	sc.offset_bits = 32
	if len(data) > 0 {
		pin.Pin(&data[0])
		sc.data = (*C.uint8_t)(unsafe.Pointer(&data[0]))
	}
	sc.data_bytes = C.uint64_t(len(data))
	if validity != nil {
		if len(validity)*8 < n {
			return nil, nil, errors.New("tadengine: validity bitmap shorter than the column")
		}
		pin.Pin(&validity[0])
		sc.validity = (*C.uint8_t)(unsafe.Pointer(&validity[0]))
	}
	sc.memory = C.TAD_MEM_HOST
	var nv C.uint64_t
	if rc := C.tad_encode_strings(e.h, &sc, (*C.int64_t)(unsafe.Pointer(&codes[0])), (*C.uint64_t)(unsafe.Pointer(&firstRow[0])),
		C.uint64_t(len(firstRow)), &nv); rc != C.TAD_OK {
		return nil, nil, fmt.Errorf("tad_encode_strings: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return codes, firstRow[:int(nv)], nil
}

// AllocDevice / FreeDevice / CopyToDevice / CopyToHost: device buffers for hosts without a HIP binding of their own (what ShardRows and a
// device-resident Run take).
// ---- columnar ingest (tad.h ABI 12): Arrow buffers -> the engine's 8-byte device columns ----

// AllocHost returns page-locked host memory (tad_host_alloc): a reader receives ClickHouse's ArrowStream body straight into it and copies from
// it to the device run at PCIe rate.  Keep and reuse the buffers between jobs: pinning is slow.
func (e *Engine) AllocHost(bytes uint64) (unsafe.Pointer, error) {
	var p unsafe.Pointer
	if rc := C.tad_host_alloc(e.h, C.uint64_t(bytes), &p); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_host_alloc: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return p, nil
}

func (e *Engine) FreeHost(p unsafe.Pointer) { C.tad_host_free(e.h, p) }

// WidenColumn writes dst[i] = table[src[i]] (table != nil: the dictionary indices of one Arrow record batch through the batch's remap into the
// column's job-wide dictionary; or a gather of a device column at Factorize's first rows) or src[i] widened (UInt32 DateTime, UInt16 ports)
// for i < n.  src: n integers of srcBits (8 / 16 / 32 / 64) bits in C / page-locked host memory (srcOnDevice false) or device memory; table and
// dst: device memory (int64).  Pointers are plain C pointers: nothing of Go's heap crosses the boundary.
func (e *Engine) WidenColumn(src unsafe.Pointer, srcBits int, srcSigned, srcOnDevice bool, n uint64, table unsafe.Pointer, tableLen uint64, dst unsafe.Pointer) error {
	signed, mem := C.int32_t(0), C.tad_mem(C.TAD_MEM_HOST)
	if srcSigned {
		signed = 1
	}
	if srcOnDevice {
		mem = C.TAD_MEM_DEVICE
	}
	if rc := C.tad_widen_column(e.h, src, C.int32_t(srcBits), signed, mem, C.uint64_t(n), (*C.int64_t)(table), C.uint64_t(tableLen), (*C.int64_t)(dst)); rc != C.TAD_OK {
		return fmt.Errorf("tad_widen_column: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return nil
}

// MaskRows writes keep[i] = AND over t of masks[t][codes[t][i]] (ANDed into the previous keep[i] when combine): the SQL's string predicates
// (anomaly_detection.py:507-614), evaluated by the host on the DISTINCT values of each column, applied to the rows on the GPU.  codes[t]
// (int64[n]), masks[t] (uint8[maskLen[t]]) and keep (uint8[n]) are device pointers; at most 8 terms.
func (e *Engine) MaskRows(n uint64, codes, masks []unsafe.Pointer, maskLen []uint64, combine bool, keep unsafe.Pointer) error {
	k := len(codes)
	if k > 8 || len(masks) != k || len(maskLen) != k {
		return errors.New("tadengine: MaskRows takes at most 8 terms, one mask and one length per code column")
	}
	// the two pointer arrays live in C memory for the call (cgo may not pass Go memory that holds pointers)
	carr := (*[8]unsafe.Pointer)(C.malloc(C.size_t(8 * unsafe.Sizeof(unsafe.Pointer(nil)))))
	marr := (*[8]unsafe.Pointer)(C.malloc(C.size_t(8 * unsafe.Sizeof(unsafe.Pointer(nil)))))
	larr := (*[8]C.uint64_t)(C.malloc(C.size_t(8 * 8)))
	defer C.free(unsafe.Pointer(carr))
	defer C.free(unsafe.Pointer(marr))
	defer C.free(unsafe.Pointer(larr))
	for t := 0; t < k; t++ {
		carr[t], marr[t], larr[t] = codes[t], masks[t], C.uint64_t(maskLen[t])
	}
	comb := C.int32_t(0)
	if combine {
		comb = 1
	}
	if rc := C.tad_mask_rows(e.h, C.uint64_t(n), C.int32_t(k), (**C.int64_t)(unsafe.Pointer(&carr[0])), (**C.uint8_t)(unsafe.Pointer(&marr[0])),
		&larr[0], comb, (*C.uint8_t)(keep)); rc != C.TAD_OK {
		return fmt.Errorf("tad_mask_rows: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return nil
}

var dropRowsOnce sync.Once
var dropRowsOK bool

// hasDropRows: the library knows tad_drop_select (tad_features); an older one would not export the call.
func hasDropRows() bool {
	dropRowsOnce.Do(func() { dropRowsOK = C.tad_features()&C.TAD_FEATURE_DROP_ROWS != 0 })
	return dropRowsOK
}

// DropFlowColumns are the flow-table columns of the drop job's query, all DEVICE pointers to N elements (AllocDevice, the ingest
// calls): UInt8 rule actions and keep, int64 epoch seconds (uint32 with TimeU32), int64 dictionary codes.  FlowEnd and Keep may be nil.
type DropFlowColumns struct {
	N                                                   uint64
	IngressAction, EgressAction                         unsafe.Pointer
	FlowStart, FlowEnd                                  unsafe.Pointer
	SrcIP, SrcPodNs, SrcPodName, DstIP, DstPodNs, DstPodName unsafe.Pointer
	SrcPodNull, DstPodNull                              int64 // the pod-name code that means "no pod" on that side; -1 = none
	Keep                                                unsafe.Pointer
	TimeU32                                             bool
}

// DropRows is DropSelect's result: seven DEVICE columns of N rows, one per selected flow row in input order.  The first four are the key
// tuple for Factorize-style calls on device columns; DayS and Count go to the job with the key ids.  The library owns the memory: Close.
type DropRows struct {
	e                                                *Engine
	h                                                *C.tad_drop_rows
	N                                                uint64
	EndpointKind, EndpointNs, EndpointName, Direction unsafe.Pointer
	DayS, Count, Row                                 unsafe.Pointer
}

func (r *DropRows) Close() {
	if r.h != nil {
		C.tad_drop_rows_free(r.e.h, r.h)
		r.h = nil
	}
}

// DropSelect is the flow-row query of the drop job on the device (tad_drop_select; snowflake/cmd/dropDetection.go:36-190 up to the
// sums): the rows whose ingress or egress rule action is 2 or 3 and that pass startTime <= flowStart, flowEnd < endTime (0 = no bound)
// and Keep, each as (endpoint kind, namespace code, name or IP code, direction, day, count 1, input row).
func (e *Engine) DropSelect(cols DropFlowColumns, startTime, endTime int64) (*DropRows, error) {
	if !hasDropRows() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no tad_drop_select (TAD_FEATURE_DROP_ROWS)")
	}
	var fc C.tad_drop_flow_columns
	fc.n_rows = C.uint64_t(cols.N)
	fc.ingress_action = (*C.uint8_t)(cols.IngressAction)
	fc.egress_action = (*C.uint8_t)(cols.EgressAction)
	fc.flow_start_s = (*C.int64_t)(cols.FlowStart)
	fc.flow_end_s = (*C.int64_t)(cols.FlowEnd)
	fc.src_ip, fc.src_pod_ns, fc.src_pod_name = (*C.int64_t)(cols.SrcIP), (*C.int64_t)(cols.SrcPodNs), (*C.int64_t)(cols.SrcPodName)
	fc.dst_ip, fc.dst_pod_ns, fc.dst_pod_name = (*C.int64_t)(cols.DstIP), (*C.int64_t)(cols.DstPodNs), (*C.int64_t)(cols.DstPodName)
	fc.src_pod_null, fc.dst_pod_null = C.int64_t(cols.SrcPodNull), C.int64_t(cols.DstPodNull)
	fc.keep = (*C.uint8_t)(cols.Keep)
	if cols.TimeU32 {
		fc.flags = C.TAD_FLAG_TIME_U32
	}
	fc.memory = C.TAD_MEM_DEVICE
	var dr *C.tad_drop_rows
	if rc := C.tad_drop_select(e.h, &fc, C.int64_t(startTime), C.int64_t(endTime), C.TAD_MEM_DEVICE, &dr); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_drop_select: %s (code %d)", msg, int(rc))
	}
	return &DropRows{e: e, h: dr, N: uint64(dr.n_rows), EndpointKind: unsafe.Pointer(dr.endpoint_kind), EndpointNs: unsafe.Pointer(dr.endpoint_ns),
		EndpointName: unsafe.Pointer(dr.endpoint_name), Direction: unsafe.Pointer(dr.direction), DayS: unsafe.Pointer(dr.day_s),
		Count: unsafe.Pointer(dr.count), Row: unsafe.Pointer(dr.row)}, nil
}

func (e *Engine) AllocDevice(bytes uint64) (unsafe.Pointer, error) {
	var p unsafe.Pointer
	if rc := C.tad_device_alloc(e.h, C.uint64_t(bytes), &p); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_device_alloc: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return p, nil
}

func (e *Engine) FreeDevice(p unsafe.Pointer) { C.tad_device_free(e.h, p) }

func (e *Engine) CopyToDevice(dst unsafe.Pointer, src []byte) error {
	if len(src) == 0 {
		return nil
	}
	if rc := C.tad_copy_to_device(e.h, dst, unsafe.Pointer(&src[0]), C.uint64_t(len(src))); rc != C.TAD_OK {
		return fmt.Errorf("tad_copy_to_device: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return nil
}

func (e *Engine) CopyToHost(dst []byte, src unsafe.Pointer) error {
	if len(dst) == 0 {
		return nil
	}
	if rc := C.tad_copy_to_host(e.h, unsafe.Pointer(&dst[0]), src, C.uint64_t(len(dst))); rc != C.TAD_OK {
		return fmt.Errorf("tad_copy_to_host: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return nil
}

// State is the per-key running EWMA state of a long-running detector (tad.h: tad_state, SURVEY.md 8f rank 3): Spark's streaming moments
// (n, avg, m2), the last EWMA value and the last flowEndSeconds of every key, kept in HBM between batches.  A state made by
// NewStateWithHistory also keeps every key's aggregated point values, sorted, for the streaming DBSCAN detector; one made by
// NewStateWithSeries keeps them in time order, for the streaming ARIMA detector.
type State struct {
	e       *Engine
	h       *C.tad_state
	history bool
	series  bool
	times   bool
}

var streamDBSCANOnce sync.Once
var streamDBSCANOK bool

// hasStreamDBSCAN: the library knows history states and streaming DBSCAN (tad_features); an older one would not export the calls.
func hasStreamDBSCAN() bool {
	streamDBSCANOnce.Do(func() { streamDBSCANOK = C.tad_features()&C.TAD_FEATURE_STREAM_DBSCAN != 0 })
	return streamDBSCANOK
}

// NewStateWithHistory makes a state that also keeps every key's aggregated point values (tad_state_create_ex with TAD_STATE_HISTORY):
// RunStream then takes Job.Algo == DBSCAN, and each batch's rows are those the batch job emits for the batch's points over everything
// seen so far.  The history grows with the points seen (HistoryPoints).
func (e *Engine) NewStateWithHistory(numKeys uint64) (*State, error) {
	if !hasStreamDBSCAN() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no streaming DBSCAN (TAD_FEATURE_STREAM_DBSCAN)")
	}
	var h *C.tad_state
	if rc := C.tad_state_create_ex(e.h, C.uint64_t(numKeys), C.TAD_STATE_HISTORY, &h); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_state_create_ex: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return &State{e: e, h: h, history: true}, nil
}

// HistoryPoints is the number of values the state's history holds (tad_state_history_points); 0 for a state without history.
func (s *State) HistoryPoints() (uint64, error) {
	if !s.history {
		return 0, nil
	}
	var n C.uint64_t
	if rc := C.tad_state_history_points(s.e.h, s.h, &n); rc != C.TAD_OK {
		return 0, fmt.Errorf("tad_state_history_points: %s (code %d)", C.GoString(C.tad_last_error(s.e.h)), int(rc))
	}
	return uint64(n), nil
}

// ExportHistory copies the history to the host (tad_state_export_history): per key its number of values, and every key's values
// ascending, keys in order.
func (s *State) ExportHistory(numKeys uint64) (length []uint64, values []uint64, err error) {
	if !s.history {
		return nil, nil, errors.New("tadengine: the state has no history")
	}
	total, err := s.HistoryPoints()
	if err != nil {
		return nil, nil, err
	}
	length, values = make([]uint64, numKeys), make([]uint64, total)
	if numKeys == 0 {
		return
	}
	var pv *C.uint64_t
	if total > 0 {
		pv = (*C.uint64_t)(unsafe.Pointer(&values[0]))
	}
	if rc := C.tad_state_export_history(s.e.h, s.h, (*C.uint64_t)(unsafe.Pointer(&length[0])), pv); rc != C.TAD_OK {
		err = fmt.Errorf("tad_state_export_history: %s (code %d)", C.GoString(C.tad_last_error(s.e.h)), int(rc))
	}
	return
}

// ImportHistory restores what ExportHistory returned (tad_state_import_history), after Import of the moments: length[k] must equal
// the key's n and every key's values must be ascending, else the state is left as it was.
func (s *State) ImportHistory(length []uint64, values []uint64) error {
	if !s.history {
		return errors.New("tadengine: the state has no history")
	}
	if len(length) == 0 {
		return errors.New("tadengine: empty state")
	}
	var pv *C.uint64_t
	if len(values) > 0 {
		pv = (*C.uint64_t)(unsafe.Pointer(&values[0]))
	}
	if rc := C.tad_state_import_history(s.e.h, s.h, (*C.uint64_t)(unsafe.Pointer(&length[0])), pv); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return IllegalArgument{msg}
		}
		return fmt.Errorf("tad_state_import_history: %s (code %d)", msg, int(rc))
	}
	return nil
}

var streamARIMAOnce sync.Once
var streamARIMAOK bool

// hasStreamARIMA: the library knows series states and streaming ARIMA (tad_features); an older one would not export the calls.
func hasStreamARIMA() bool {
	streamARIMAOnce.Do(func() { streamARIMAOK = C.tad_features()&C.TAD_FEATURE_STREAM_ARIMA != 0 })
	return streamARIMAOK
}

// NewStateWithSeries makes a state that also keeps every key's aggregated point values in time order (tad_state_create_ex with
// TAD_STATE_SERIES; withHistory adds TAD_STATE_HISTORY): RunStream then takes Job.Algo == ARIMA, and each batch's rows are those the
// batch job emits for the batch's points over everything seen so far.  The series grows with the points seen (SeriesPoints).
func (e *Engine) NewStateWithSeries(numKeys uint64, withHistory bool) (*State, error) {
	if !hasStreamARIMA() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no streaming ARIMA (TAD_FEATURE_STREAM_ARIMA)")
	}
	flags := C.uint32_t(C.TAD_STATE_SERIES)
	if withHistory {
		flags |= C.TAD_STATE_HISTORY
	}
	var h *C.tad_state
	if rc := C.tad_state_create_ex(e.h, C.uint64_t(numKeys), flags, &h); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_state_create_ex: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return &State{e: e, h: h, history: withHistory, series: true}, nil
}

// SeriesPoints is the number of values the state's series holds (tad_state_series_points); 0 for a state without a series.
func (s *State) SeriesPoints() (uint64, error) {
	if !s.series {
		return 0, nil
	}
	var n C.uint64_t
	if rc := C.tad_state_series_points(s.e.h, s.h, &n); rc != C.TAD_OK {
		return 0, fmt.Errorf("tad_state_series_points: %s (code %d)", C.GoString(C.tad_last_error(s.e.h)), int(rc))
	}
	return uint64(n), nil
}

// ExportSeries copies the series to the host (tad_state_export_series): per key its number of values, and every key's values in
// time order, keys in order.
func (s *State) ExportSeries(numKeys uint64) (length []uint64, values []uint64, err error) {
	if !s.series {
		return nil, nil, errors.New("tadengine: the state has no series")
	}
	total, err := s.SeriesPoints()
	if err != nil {
		return nil, nil, err
	}
	length, values = make([]uint64, numKeys), make([]uint64, total)
	if numKeys == 0 {
		return
	}
	var pv *C.uint64_t
	if total > 0 {
		pv = (*C.uint64_t)(unsafe.Pointer(&values[0]))
	}
	if rc := C.tad_state_export_series(s.e.h, s.h, (*C.uint64_t)(unsafe.Pointer(&length[0])), pv); rc != C.TAD_OK {
		err = fmt.Errorf("tad_state_export_series: %s (code %d)", C.GoString(C.tad_last_error(s.e.h)), int(rc))
	}
	return
}

// ImportSeries restores what ExportSeries returned (tad_state_import_series), after Import of the moments: length[k] must equal the
// key's n, else the state is left as it was.
func (s *State) ImportSeries(length []uint64, values []uint64) error {
	if !s.series {
		return errors.New("tadengine: the state has no series")
	}
	if len(length) == 0 {
		return errors.New("tadengine: empty state")
	}
	var pv *C.uint64_t
	if len(values) > 0 {
		pv = (*C.uint64_t)(unsafe.Pointer(&values[0]))
	}
	if rc := C.tad_state_import_series(s.e.h, s.h, (*C.uint64_t)(unsafe.Pointer(&length[0])), pv); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return IllegalArgument{msg}
		}
		return fmt.Errorf("tad_state_import_series: %s (code %d)", msg, int(rc))
	}
	return nil
}

var streamTrimOnce sync.Once
var streamTrimOK bool

// hasStreamTrim: the library knows states with times and tad_state_trim (tad_features); an older one would not export the calls.
func hasStreamTrim() bool {
	streamTrimOnce.Do(func() { streamTrimOK = C.tad_features()&C.TAD_FEATURE_STREAM_TRIM != 0 })
	return streamTrimOK
}

// NewStateWithTimes makes a series state that also keeps every series point's flowEndSeconds (tad_state_create_ex with
// TAD_STATE_SERIES | TAD_STATE_TIMES; withHistory adds TAD_STATE_HISTORY), so that Trim can keep a window of time.
func (e *Engine) NewStateWithTimes(numKeys uint64, withHistory bool) (*State, error) {
	if !hasStreamTrim() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no state trim (TAD_FEATURE_STREAM_TRIM)")
	}
	flags := C.uint32_t(C.TAD_STATE_SERIES | C.TAD_STATE_TIMES)
	if withHistory {
		flags |= C.TAD_STATE_HISTORY
	}
	var h *C.tad_state
	if rc := C.tad_state_create_ex(e.h, C.uint64_t(numKeys), flags, &h); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_state_create_ex: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return &State{e: e, h: h, history: withHistory, series: true, times: true}, nil
}

// Trim drops every key's oldest points (tad_state_trim): it keeps the points with flowEndSeconds >= keepFrom (0: no time rule; needs a
// state made by NewStateWithTimes), then at most the newest keepPoints (0: no count rule).  The state becomes that of a fresh state
// streamed only the retained points with EWMA parameter alpha (0 -> 0.5).  Returns the number of points dropped.
func (s *State) Trim(keepPoints uint64, keepFrom int64, alpha float64) (uint64, error) {
	if !hasStreamTrim() {
		return 0, errors.New("tadengine: libtad_mi355x.so has no state trim (TAD_FEATURE_STREAM_TRIM)")
	}
	if !s.series {
		return 0, IllegalArgument{"tadengine: a trim needs a state with a series (NewStateWithSeries or NewStateWithTimes)"}
	}
	if keepFrom != 0 && !s.times {
		return 0, IllegalArgument{"tadengine: a trim by time needs a state made by NewStateWithTimes"}
	}
	var dropped C.uint64_t
	if rc := C.tad_state_trim(s.e.h, s.h, C.uint64_t(keepPoints), C.int64_t(keepFrom), C.double(alpha), &dropped); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return 0, IllegalArgument{msg}
		}
		return 0, fmt.Errorf("tad_state_trim: %s (code %d)", msg, int(rc))
	}
	return uint64(dropped), nil
}

// Bytes is the device memory the state holds (tad_state_bytes): both moment blocks, the offsets and every arena at its capacity.
func (s *State) Bytes() (uint64, error) {
	if !hasStreamTrim() {
		return 0, errors.New("tadengine: libtad_mi355x.so has no tad_state_bytes (TAD_FEATURE_STREAM_TRIM)")
	}
	var n C.uint64_t
	if rc := C.tad_state_bytes(s.e.h, s.h, &n); rc != C.TAD_OK {
		return 0, fmt.Errorf("tad_state_bytes: %s (code %d)", C.GoString(C.tad_last_error(s.e.h)), int(rc))
	}
	return uint64(n), nil
}

// ExportTimes copies every series point's flowEndSeconds to the host (tad_state_export_times), in the order of ExportSeries.
func (s *State) ExportTimes() ([]int64, error) {
	if !s.times || !hasStreamTrim() {
		return nil, errors.New("tadengine: the state has no times")
	}
	total, err := s.SeriesPoints()
	if err != nil {
		return nil, err
	}
	t := make([]int64, total)
	if total == 0 {
		return t, nil
	}
	if rc := C.tad_state_export_times(s.e.h, s.h, (*C.int64_t)(unsafe.Pointer(&t[0]))); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_state_export_times: %s (code %d)", C.GoString(C.tad_last_error(s.e.h)), int(rc))
	}
	return t, nil
}

// ImportTimes restores what ExportTimes returned (tad_state_import_times), after Import and ImportSeries: one time per series point,
// every key's times strictly ascending and ending at its last_t, else the state is left as it was.
func (s *State) ImportTimes(t []int64) error {
	if !s.times || !hasStreamTrim() {
		return errors.New("tadengine: the state has no times")
	}
	total, err := s.SeriesPoints()
	if err != nil {
		return err
	}
	if uint64(len(t)) != total {
		return IllegalArgument{fmt.Sprintf("tadengine: %d times, the series holds %d points", len(t), total)}
	}
	var pt *C.int64_t
	if len(t) > 0 {
		pt = (*C.int64_t)(unsafe.Pointer(&t[0]))
	}
	if rc := C.tad_state_import_times(s.e.h, s.h, pt); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return IllegalArgument{msg}
		}
		return fmt.Errorf("tad_state_import_times: %s (code %d)", msg, int(rc))
	}
	return nil
}

var stateRunOnce sync.Once
var stateRunOK bool

// hasStateRun: the library knows tad_run_state (tad_features); an older one would not export the call.
func hasStateRun() bool {
	stateRunOnce.Do(func() { stateRunOK = C.tad_features()&C.TAD_FEATURE_STATE_RUN != 0 })
	return stateRunOK
}

// Run judges every point the state holds against the window as a whole (tad_run_state): the rows are exactly those the batch job
// returns over the state's points with job.Algo and its detector parameters, computed from the state alone — no flow row is read again.
// The state must be made by NewStateWithTimes (with history for DBSCAN); it is left unchanged.  job.StartTime / EndTime must be 0: the
// window is what the state holds, and Trim narrows it.  job.AggFlow is ignored (the points are already aggregated).
func (s *State) Run(job Job) ([]Row, error) {
	if !hasStateRun() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no tad_run_state (TAD_FEATURE_STATE_RUN)")
	}
	if !s.series || !s.times {
		return nil, IllegalArgument{"tadengine: Run needs a state made by NewStateWithTimes"}
	}
	if job.Algo == DBSCAN && !s.history {
		return nil, IllegalArgument{"tadengine: Run with DBSCAN needs a state made by NewStateWithTimes with history"}
	}
	var cj C.tad_job
	cj.algo = C.tad_algo(job.Algo)
	cj.start_time = C.int64_t(job.StartTime)
	cj.end_time = C.int64_t(job.EndTime)
	// the detector parameters (0 = the reference's defaults, as in Run and RunStream)
	cj.dbscan_eps = C.double(job.DBSCANEps)
	cj.dbscan_min_samples, cj.arima_maxiter = C.int32_t(job.DBSCANMinSamples), C.int32_t(job.ARIMAMaxIter)
	id := []byte(job.ID)
	if len(id) > 63 {
		id = id[:63]
	}
	for i, b := range id {
		cj.id[i] = C.char(b)
	}
	var res *C.tad_result
	if rc := C.tad_run_state(s.e.h, s.h, &cj, C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_run_state: %s (code %d)", msg, int(rc))
	}
	defer C.tad_result_free(s.e.h, res)
	a := int(res.n_rows)
	rows := make([]Row, a)
	if a > 0 {
		k := unsafe.Slice((*uint64)(unsafe.Pointer(res.key_id)), a)
		t := unsafe.Slice((*int64)(unsafe.Pointer(res.flow_end_s)), a)
		x := unsafe.Slice((*float64)(unsafe.Pointer(res.throughput)), a)
		c := unsafe.Slice((*float64)(unsafe.Pointer(res.algo_calc)), a)
		sd := unsafe.Slice((*float64)(unsafe.Pointer(res.stddev)), a)
		for i := range rows {
			rows[i] = Row{k[i], t[i], x[i], c[i], sd[i]}
		}
	}
	return rows, nil
}

var stateWindowOnce sync.Once
var stateWindowOK bool

// hasStateWindow: the library knows tad_run_state_window (tad_features); an older one would not export the call.
func hasStateWindow() bool {
	stateWindowOnce.Do(func() { stateWindowOK = C.tad_features()&C.TAD_FEATURE_STATE_WINDOW != 0 })
	return stateWindowOK
}

// RunWindow is Run over a window of what the state holds, read-only (tad_run_state_window): of every key's series the points with
// flowEndSeconds >= fromT and < toT (0 = no bound on that side), then the newest keepPoints of those (0 = all).  The rows are exactly
// those the batch job returns over these points.  Both bounds act on flowEndSeconds: fromT is not the reference's start_time filter,
// which tests flowStartSeconds.  job.StartTime / EndTime must be 0, as for Run; the state is left unchanged.
func (s *State) RunWindow(job Job, fromT, toT int64, keepPoints uint64) ([]Row, error) {
	if !hasStateWindow() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no tad_run_state_window (TAD_FEATURE_STATE_WINDOW)")
	}
	if !s.series || !s.times {
		return nil, IllegalArgument{"tadengine: RunWindow needs a state made by NewStateWithTimes"}
	}
	if job.Algo == DBSCAN && !s.history {
		return nil, IllegalArgument{"tadengine: RunWindow with DBSCAN needs a state made by NewStateWithTimes with history"}
	}
	var cj C.tad_job
	cj.algo = C.tad_algo(job.Algo)
	cj.start_time = C.int64_t(job.StartTime)
	cj.end_time = C.int64_t(job.EndTime)
	cj.dbscan_eps = C.double(job.DBSCANEps)
	cj.dbscan_min_samples, cj.arima_maxiter = C.int32_t(job.DBSCANMinSamples), C.int32_t(job.ARIMAMaxIter)
	id := []byte(job.ID)
	if len(id) > 63 {
		id = id[:63]
	}
	for i, b := range id {
		cj.id[i] = C.char(b)
	}
	var res *C.tad_result
	if rc := C.tad_run_state_window(s.e.h, s.h, &cj, C.int64_t(fromT), C.int64_t(toT), C.uint64_t(keepPoints), C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_run_state_window: %s (code %d)", msg, int(rc))
	}
	defer C.tad_result_free(s.e.h, res)
	a := int(res.n_rows)
	rows := make([]Row, a)
	if a > 0 {
		k := unsafe.Slice((*uint64)(unsafe.Pointer(res.key_id)), a)
		t := unsafe.Slice((*int64)(unsafe.Pointer(res.flow_end_s)), a)
		x := unsafe.Slice((*float64)(unsafe.Pointer(res.throughput)), a)
		c := unsafe.Slice((*float64)(unsafe.Pointer(res.algo_calc)), a)
		sd := unsafe.Slice((*float64)(unsafe.Pointer(res.stddev)), a)
		for i := range rows {
			rows[i] = Row{k[i], t[i], x[i], c[i], sd[i]}
		}
	}
	return rows, nil
}

var stateMergeOnce sync.Once
var stateMergeOK bool

// hasStateMerge: the library knows tad_state_merge (tad_features); an older one would not export the call.
func hasStateMerge() bool {
	stateMergeOnce.Do(func() { stateMergeOK = C.tad_features()&C.TAD_FEATURE_STATE_MERGE != 0 })
	return stateMergeOK
}

// MergeStats is what one Merge did with the batch's points (tad_merge_stats).
type MergeStats struct {
	RowsIn, RowsUsed uint64
	BatchPoints      uint64 // distinct (key, flowEndSeconds) points of the batch
	PointsTooOld     uint64 // older than keepFrom: dropped
	PointsAppended   uint64 // newer than everything their key held
	PointsInserted   uint64 // a new time before the key's last one
	PointsCombined   uint64 // a time the key already held: value = op(old, new)
	KeysTouched      uint64
	KeysReplayed     uint64 // keys whose moments were replayed from the zero state
	MsTotal          float32
}

// Merge places ONE batch by time into the state (tad_state_merge): late rows, re-sent rows and rows of a (key, flowEndSeconds) group split
// over batches, which RunStream refuses.  Afterwards the state is the one a fresh state holds after one RunStream EWMA batch over its
// window's points plus this batch (without the points older than keepFrom, when that is not 0).  The state must be made by
// NewStateWithTimes; a poller streams its in-order batches with RunStream, merges whatever trails in, trims, and asks Run for the window's
// verdicts.  No rows are returned.  The value op follows job.AggFlow as in RunStream: keep it the same for every batch of a state.
func (s *State) Merge(job Job, cols Columns, keepFrom int64) (MergeStats, error) {
	if !hasStateMerge() {
		return MergeStats{}, errors.New("tadengine: libtad_mi355x.so has no tad_state_merge (TAD_FEATURE_STATE_MERGE)")
	}
	if !s.series || !s.times {
		return MergeStats{}, IllegalArgument{"tadengine: Merge needs a state made by NewStateWithTimes"}
	}
	cj, cc, free, err := batchCall(job, cols)
	if err != nil {
		return MergeStats{}, err
	}
	defer free()
	var ms C.tad_merge_stats
	if rc := C.tad_state_merge(s.e.h, s.h, &cj, &cc, C.int64_t(keepFrom), &ms); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return MergeStats{}, IllegalArgument{msg}
		}
		return MergeStats{}, fmt.Errorf("tad_state_merge: %s (code %d)", msg, int(rc))
	}
	return MergeStats{RowsIn: uint64(ms.rows_in), RowsUsed: uint64(ms.rows_used), BatchPoints: uint64(ms.batch_points),
		PointsTooOld: uint64(ms.points_too_old), PointsAppended: uint64(ms.points_appended), PointsInserted: uint64(ms.points_inserted),
		PointsCombined: uint64(ms.points_combined), KeysTouched: uint64(ms.keys_touched), KeysReplayed: uint64(ms.keys_replayed),
		MsTotal: float32(ms.ms_total)}, nil
}

var stateReplaceOnce sync.Once
var stateReplaceOK bool

// hasStateReplace: the library knows tad_state_replace (tad_features); an older one would not export the call.
func hasStateReplace() bool {
	stateReplaceOnce.Do(func() { stateReplaceOK = C.tad_features()&C.TAD_FEATURE_STATE_REPLACE != 0 })
	return stateReplaceOK
}

// ReplaceStats is what one Replace did with the batch's points and with the points the state held (tad_replace_stats).
type ReplaceStats struct {
	RowsIn, RowsUsed uint64
	BatchPoints      uint64 // distinct (key, flowEndSeconds) points of the batch
	PointsTooOld     uint64 // older than keepFrom: dropped
	PointsAppended   uint64 // newer than everything their key held
	PointsInserted   uint64 // a new time before the key's last one
	PointsReplaced   uint64 // a time the key already held: value = the batch's
	PointsErased     uint64 // points the state held inside the range that the batch does not name
	KeysEmptied      uint64 // keys that held points and hold none afterwards
	KeysTouched      uint64
	KeysReplayed     uint64 // keys whose moments were replayed from the zero state
	MsTotal          float32
}

// Replace makes ONE batch the truth for the points it names (tad_state_replace): a point at a time its key already holds takes the
// batch's value instead of being combined with it, so a re-read of the same rows leaves the same state under sum as under max.  With
// ranged the batch is ALL rows with fromT <= flowEndSeconds < toT (0 = no bound on that side): every point of the state inside that
// range that the batch does not name is erased, on every key, and an empty batch still erases the range.  A poller re-reads
// [watermark - lag, now), calls Replace with that range and moves the watermark: the turn is idempotent.  The state must be made by
// NewStateWithTimes.  No rows are returned.  The value op follows job.AggFlow as in RunStream and only aggregates rows inside the batch.
func (s *State) Replace(job Job, cols Columns, ranged bool, fromT, toT, keepFrom int64) (ReplaceStats, error) {
	if !hasStateReplace() {
		return ReplaceStats{}, errors.New("tadengine: libtad_mi355x.so has no tad_state_replace (TAD_FEATURE_STATE_REPLACE)")
	}
	if !s.series || !s.times {
		return ReplaceStats{}, IllegalArgument{"tadengine: Replace needs a state made by NewStateWithTimes"}
	}
	cj, cc, free, err := batchCall(job, cols)
	if err != nil {
		return ReplaceStats{}, err
	}
	defer free()
	var flags C.uint32_t
	if ranged {
		flags = C.TAD_REPLACE_RANGE
	}
	var rs C.tad_replace_stats
	if rc := C.tad_state_replace(s.e.h, s.h, &cj, &cc, flags, C.int64_t(fromT), C.int64_t(toT), C.int64_t(keepFrom), &rs); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return ReplaceStats{}, IllegalArgument{msg}
		}
		return ReplaceStats{}, fmt.Errorf("tad_state_replace: %s (code %d)", msg, int(rc))
	}
	return ReplaceStats{RowsIn: uint64(rs.rows_in), RowsUsed: uint64(rs.rows_used), BatchPoints: uint64(rs.batch_points),
		PointsTooOld: uint64(rs.points_too_old), PointsAppended: uint64(rs.points_appended), PointsInserted: uint64(rs.points_inserted),
		PointsReplaced: uint64(rs.points_replaced), PointsErased: uint64(rs.points_erased), KeysEmptied: uint64(rs.keys_emptied),
		KeysTouched: uint64(rs.keys_touched), KeysReplayed: uint64(rs.keys_replayed), MsTotal: float32(rs.ms_total)}, nil
}

var keyDictOnce sync.Once
var keyDictOK bool

// hasKeyDict: the library knows the persistent key dictionary (tad_features); an older one would not export the calls.
func hasKeyDict() bool {
	keyDictOnce.Do(func() { keyDictOK = C.tad_features()&C.TAD_FEATURE_KEY_DICT != 0 })
	return keyDictOK
}

// KeyDict is a key dictionary kept in HBM that outlives the call (tad_keydict): key tuples -> dense ids that stay the same from batch
// to batch, new ids in order of first appearance.  It is what gives a poller the key ids of RunStream / Merge: Encode every batch,
// State.Resize when NumKeys grew, then RunStream or Merge with Columns.NumKeys = the dictionary's.
type KeyDict struct {
	e     *Engine
	h     *C.tad_keydict
	nCols int
}

// NewKeyDict makes a dictionary for tuples of nCols (1..8) int64 columns.  expectedKeys sizes the first table (0 = the default).
func (e *Engine) NewKeyDict(nCols int, expectedKeys uint64) (*KeyDict, error) {
	if !hasKeyDict() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no key dictionary (TAD_FEATURE_KEY_DICT)")
	}
	var h *C.tad_keydict
	if rc := C.tad_keydict_create(e.h, C.int32_t(nCols), C.uint64_t(expectedKeys), &h); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_keydict_create: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return &KeyDict{e: e, h: h, nCols: nCols}, nil
}

func (d *KeyDict) Close() {
	if d.h != nil {
		C.tad_keydict_destroy(d.e.h, d.h)
		d.h = nil
	}
}

// keyBatch copies the key tuples of one batch into C memory (no Go pointer is stored in the struct) and fills the tad_key_columns.
// release frees the copies.
func keyBatch(nCols int, colsA [][]int64, keepA []byte, colsB [][]int64, keepB []byte) (kb *C.tad_key_columns, n int, release func(), err error) {
	if len(colsA) != nCols || (colsB != nil && len(colsB) != nCols) {
		return nil, 0, nil, IllegalArgument{fmt.Sprintf("tadengine: %d key columns on every side", nCols)}
	}
	n = len(colsA[0])
	var bufs []unsafe.Pointer
	release = func() {
		for _, p := range bufs {
			if p != nil {
				C.free(p)
			}
		}
	}
	ptrs := func(cols [][]int64) *unsafe.Pointer {
		arr := (*[8]unsafe.Pointer)(C.malloc(C.size_t(8 * unsafe.Sizeof(unsafe.Pointer(nil)))))
		bufs = append(bufs, unsafe.Pointer(arr))
		for c, col := range cols {
			if len(col) != n {
				return nil
			}
			arr[c] = cColumn(col)
			bufs = append(bufs, arr[c])
		}
		return &arr[0]
	}
	mask := func(m []byte) unsafe.Pointer {
		if m == nil {
			return nil
		}
		p := C.CBytes(m)
		bufs = append(bufs, p)
		return p
	}
	kb = (*C.tad_key_columns)(C.calloc(1, C.size_t(unsafe.Sizeof(C.tad_key_columns{}))))
	bufs = append(bufs, unsafe.Pointer(kb))
	kb.n_rows = C.uint64_t(n)
	kb.n_cols = C.int32_t(nCols)
	kb.memory = C.TAD_MEM_HOST
	pa := ptrs(colsA)
	if pa == nil || (keepA != nil && len(keepA) != n) || (keepB != nil && len(keepB) != n) {
		release()
		return nil, 0, nil, IllegalArgument{"tadengine: key columns and masks differ in length"}
	}
	kb.cols_a = (**C.int64_t)(unsafe.Pointer(pa))
	kb.keep_a = (*C.uint8_t)(mask(keepA))
	if colsB != nil {
		pb := ptrs(colsB)
		if pb == nil {
			release()
			return nil, 0, nil, IllegalArgument{"tadengine: key columns differ in length"}
		}
		kb.cols_b = (**C.int64_t)(unsafe.Pointer(pb))
		kb.keep_b = (*C.uint8_t)(mask(keepB))
	}
	return kb, n, release, nil
}

// Encode maps one batch's key tuples to ids (tad_keydict_encode).  colsA / keepA / colsB / keepB as in Factorize.  Tuples the
// dictionary holds keep their ids; new ones get numKeysBefore, numKeysBefore + 1, ... in order of first appearance over the virtual
// rows [side a ++ side b]; rows the masks reject get KeySkip.  newFirstRow[j] = the virtual row of THIS batch where key
// numKeysBefore + j first appears: the caller reads the new key's strings there.
func (d *KeyDict) Encode(colsA [][]int64, keepA []byte, colsB [][]int64, keepB []byte) (keyID, keyID2, newFirstRow []uint64, numKeysBefore uint64, err error) {
	if !hasKeyDict() {
		return nil, nil, nil, 0, errors.New("tadengine: libtad_mi355x.so has no key dictionary (TAD_FEATURE_KEY_DICT)")
	}
	kb, n, release, err := keyBatch(d.nCols, colsA, keepA, colsB, keepB)
	if err != nil {
		return nil, nil, nil, 0, err
	}
	defer release()
	sides := 1
	if colsB != nil {
		sides = 2
	}
	keyID = make([]uint64, n)
	newFirstRow = make([]uint64, n*sides)
	var k1, k2, fr *C.uint64_t
	if colsB != nil {
		keyID2 = make([]uint64, n)
	}
	if n > 0 {
		k1 = (*C.uint64_t)(unsafe.Pointer(&keyID[0]))
		fr = (*C.uint64_t)(unsafe.Pointer(&newFirstRow[0]))
		if colsB != nil {
			k2 = (*C.uint64_t)(unsafe.Pointer(&keyID2[0]))
		}
	}
	var before, after C.uint64_t
	if rc := C.tad_keydict_encode(d.e.h, d.h, kb, k1, k2, fr, C.uint64_t(len(newFirstRow)), &before, &after); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(d.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, nil, nil, 0, IllegalArgument{msg}
		}
		return nil, nil, nil, 0, fmt.Errorf("tad_keydict_encode: %s (code %d)", msg, int(rc))
	}
	return keyID, keyID2, newFirstRow[:int(after-before)], uint64(before), nil
}

// Lookup is Encode read-only (tad_keydict_lookup): an unknown tuple gets KeySkip and the dictionary is unchanged.
func (d *KeyDict) Lookup(colsA [][]int64, keepA []byte, colsB [][]int64, keepB []byte) (keyID, keyID2 []uint64, err error) {
	if !hasKeyDict() {
		return nil, nil, errors.New("tadengine: libtad_mi355x.so has no key dictionary (TAD_FEATURE_KEY_DICT)")
	}
	kb, n, release, err := keyBatch(d.nCols, colsA, keepA, colsB, keepB)
	if err != nil {
		return nil, nil, err
	}
	defer release()
	keyID = make([]uint64, n)
	var k1, k2 *C.uint64_t
	if colsB != nil {
		keyID2 = make([]uint64, n)
	}
	if n > 0 {
		k1 = (*C.uint64_t)(unsafe.Pointer(&keyID[0]))
		if colsB != nil {
			k2 = (*C.uint64_t)(unsafe.Pointer(&keyID2[0]))
		}
	}
	if rc := C.tad_keydict_lookup(d.e.h, d.h, kb, k1, k2); rc != C.TAD_OK {
		return nil, nil, fmt.Errorf("tad_keydict_lookup: %s (code %d)", C.GoString(C.tad_last_error(d.e.h)), int(rc))
	}
	return keyID, keyID2, nil
}

// NumKeys is the number of keys the dictionary holds (tad_keydict_num_keys): Columns.NumKeys of the next RunStream / Merge.
func (d *KeyDict) NumKeys() (uint64, error) {
	if !hasKeyDict() {
		return 0, errors.New("tadengine: libtad_mi355x.so has no key dictionary (TAD_FEATURE_KEY_DICT)")
	}
	var n C.uint64_t
	if rc := C.tad_keydict_num_keys(d.e.h, d.h, &n); rc != C.TAD_OK {
		return 0, fmt.Errorf("tad_keydict_num_keys: %s (code %d)", C.GoString(C.tad_last_error(d.e.h)), int(rc))
	}
	return uint64(n), nil
}

// Bytes is the device memory the dictionary holds: the table and the key records at their capacity (tad_keydict_bytes).
func (d *KeyDict) Bytes() (uint64, error) {
	if !hasKeyDict() {
		return 0, errors.New("tadengine: libtad_mi355x.so has no key dictionary (TAD_FEATURE_KEY_DICT)")
	}
	var n C.uint64_t
	if rc := C.tad_keydict_bytes(d.e.h, d.h, &n); rc != C.TAD_OK {
		return 0, fmt.Errorf("tad_keydict_bytes: %s (code %d)", C.GoString(C.tad_last_error(d.e.h)), int(rc))
	}
	return uint64(n), nil
}

// Export returns the tuples of the keys [firstKey, firstKey + nKeys) column by column, and their sides (tad_keydict_export).
func (d *KeyDict) Export(firstKey, nKeys uint64) (cols [][]int64, side []byte, err error) {
	if !hasKeyDict() {
		return nil, nil, errors.New("tadengine: libtad_mi355x.so has no key dictionary (TAD_FEATURE_KEY_DICT)")
	}
	cols = make([][]int64, d.nCols)
	side = make([]byte, nKeys)
	// the pointer array and the columns it names live in C memory for the call (no Go pointer inside C memory)
	arr := (*[8]*C.int64_t)(C.calloc(8, C.size_t(unsafe.Sizeof(unsafe.Pointer(nil)))))
	defer C.free(unsafe.Pointer(arr))
	for c := range cols {
		cols[c] = make([]int64, nKeys)
		arr[c] = (*C.int64_t)(C.calloc(C.size_t(nKeys)+1, 8))
		defer C.free(unsafe.Pointer(arr[c]))
	}
	var sp *C.uint8_t
	if nKeys > 0 {
		sp = (*C.uint8_t)(unsafe.Pointer(&side[0]))
	}
	if rc := C.tad_keydict_export(d.e.h, d.h, C.uint64_t(firstKey), C.uint64_t(nKeys), &arr[0], sp); rc != C.TAD_OK {
		return nil, nil, fmt.Errorf("tad_keydict_export: %s (code %d)", C.GoString(C.tad_last_error(d.e.h)), int(rc))
	}
	for c := range cols {
		copy(cols[c], unsafe.Slice((*int64)(unsafe.Pointer(arr[c])), nKeys))
	}
	return cols, side, nil
}

// Import fills an EMPTY dictionary so that key i is tuple i (tad_keydict_import): what Export returned, after a restart of the host.
// side nil = every key on side a.  A duplicate tuple, a dictionary that holds keys or a side > 1 is an IllegalArgument.
func (d *KeyDict) Import(cols [][]int64, side []byte) error {
	if !hasKeyDict() {
		return errors.New("tadengine: libtad_mi355x.so has no key dictionary (TAD_FEATURE_KEY_DICT)")
	}
	kb, n, release, err := keyBatch(d.nCols, cols, side, nil, nil)
	if err != nil {
		return err
	}
	defer release()
	if rc := C.tad_keydict_import(d.e.h, d.h, C.uint64_t(n), kb.cols_a, kb.keep_a); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(d.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return IllegalArgument{msg}
		}
		return fmt.Errorf("tad_keydict_import: %s (code %d)", msg, int(rc))
	}
	return nil
}

var keyRetireOnce sync.Once
var keyRetireOK bool

// hasKeyRetire: the library knows tad_state_compact / tad_keydict_compact (tad_features); an older one would not export the calls.
func hasKeyRetire() bool {
	keyRetireOnce.Do(func() { keyRetireOK = C.tad_features()&C.TAD_FEATURE_KEY_RETIRE != 0 })
	return keyRetireOK
}

// KeySkip is remap's entry for a retired key (TAD_KEY_SKIP).
const KeySkip = ^uint64(0)

// CompactStats is what one State.Compact retired and moved (tad_compact_stats).
type CompactStats struct {
	KeysBefore, KeysAfter uint64 // keys held at entry; survivors
	NumKeys               uint64 // keys held at exit: max(survivors, 1)
	KeysUnseen, KeysIdle  uint64 // retired without a point; retired because the newest point is older than retireBefore
	PointsDropped         uint64 // the points of the idle keys
	SeriesPointsMoved     uint64
	HistoryPointsMoved    uint64
	BytesBefore           uint64
	BytesAfter            uint64
	MsTotal               float32
}

// Compact drops the dead keys of the state and renumbers the survivors densely, order kept (tad_state_compact).  A key survives iff it
// holds points and, with retireBefore != 0, its newest point is at or after retireBefore.  numKeys = the keys the state holds now.
// remap[k] = the new id of old key k, or KeySkip: pass it to KeyDict.Compact and apply it to the host's key table.  The state then holds
// CompactStats.NumKeys keys.  On a tick after Trim, not per batch.
func (s *State) Compact(numKeys uint64, retireBefore int64) (remap []uint64, st CompactStats, err error) {
	if !hasKeyRetire() {
		return nil, CompactStats{}, errors.New("tadengine: libtad_mi355x.so has no tad_state_compact (TAD_FEATURE_KEY_RETIRE)")
	}
	if numKeys == 0 {
		return nil, CompactStats{}, IllegalArgument{"tadengine: Compact needs the state's key count"}
	}
	// the remap lives in C memory for the call (the library writes it from its own stream)
	buf := (*C.uint64_t)(C.calloc(C.size_t(numKeys), 8))
	if buf == nil {
		return nil, CompactStats{}, errors.New("tadengine: out of memory")
	}
	defer C.free(unsafe.Pointer(buf))
	var cs C.tad_compact_stats
	if rc := C.tad_state_compact(s.e.h, s.h, C.int64_t(retireBefore), buf, C.TAD_MEM_HOST, &cs); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, CompactStats{}, IllegalArgument{msg}
		}
		return nil, CompactStats{}, fmt.Errorf("tad_state_compact: %s (code %d)", msg, int(rc))
	}
	if uint64(cs.keys_before) != numKeys {
		return nil, CompactStats{}, IllegalArgument{fmt.Sprintf("tadengine: Compact was told %d keys, the state held %d", numKeys, uint64(cs.keys_before))}
	}
	remap = make([]uint64, numKeys)
	copy(remap, unsafe.Slice((*uint64)(unsafe.Pointer(buf)), numKeys))
	return remap, CompactStats{KeysBefore: uint64(cs.keys_before), KeysAfter: uint64(cs.keys_after), NumKeys: uint64(cs.num_keys),
		KeysUnseen: uint64(cs.keys_unseen), KeysIdle: uint64(cs.keys_idle), PointsDropped: uint64(cs.points_dropped),
		SeriesPointsMoved: uint64(cs.series_points_moved), HistoryPointsMoved: uint64(cs.history_points_moved),
		BytesBefore: uint64(cs.bytes_before), BytesAfter: uint64(cs.bytes_after), MsTotal: float32(cs.ms_total)}, nil
}

// Compact applies the remap of State.Compact to the dictionary (tad_keydict_compact): a survivor's tuple now encodes to remap[old id], a
// retired tuple is forgotten and gets a new id at the end when it returns.  len(remap) must be the dictionary's NumKeys; a remap that is
// not the one State.Compact writes is an IllegalArgument and leaves the dictionary unchanged.  Returns the keys held afterwards.
func (d *KeyDict) Compact(remap []uint64) (uint64, error) {
	if !hasKeyRetire() {
		return 0, errors.New("tadengine: libtad_mi355x.so has no tad_keydict_compact (TAD_FEATURE_KEY_RETIRE)")
	}
	buf := (*C.uint64_t)(cColumn(remap))
	defer C.free(unsafe.Pointer(buf))
	var n C.uint64_t
	if rc := C.tad_keydict_compact(d.e.h, d.h, buf, C.uint64_t(len(remap)), C.TAD_MEM_HOST, &n); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(d.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return 0, IllegalArgument{msg}
		}
		return 0, fmt.Errorf("tad_keydict_compact: %s (code %d)", msg, int(rc))
	}
	return uint64(n), nil
}

var stateDropOnce sync.Once
var stateDropOK bool

// hasStateDrop: the library knows tad_drop_state / tad_drop_stream (tad_features); an older one would not export the calls.
func hasStateDrop() bool {
	stateDropOnce.Do(func() { stateDropOK = C.tad_features()&C.TAD_FEATURE_STATE_DROP != 0 })
	return stateDropOK
}

// dropJob: the tad_job of the two drop calls.  nSigma / minSamples 0 = the reference's 3 and 3.
func dropJob(job Job, nSigma float64, minSamples int32) C.tad_job {
	var cj C.tad_job
	cj.algo = C.TAD_ALGO_DROP
	cj.agg_flow = C.tad_agg_flow(job.AggFlow)
	cj.start_time = C.int64_t(job.StartTime)
	cj.end_time = C.int64_t(job.EndTime)
	cj.drop_nsigma = C.double(nSigma)
	cj.drop_min_samples = C.int32_t(minSamples)
	id := []byte(job.ID)
	if len(id) > 63 {
		id = id[:63]
	}
	for i, b := range id {
		cj.id[i] = C.char(b)
	}
	return cj
}

// resultRows copies a host result's rows and frees it.
func (s *State) resultRows(res *C.tad_result) []Row {
	defer C.tad_result_free(s.e.h, res)
	a := int(res.n_rows)
	rows := make([]Row, a)
	if a > 0 {
		k := unsafe.Slice((*uint64)(unsafe.Pointer(res.key_id)), a)
		t := unsafe.Slice((*int64)(unsafe.Pointer(res.flow_end_s)), a)
		x := unsafe.Slice((*float64)(unsafe.Pointer(res.throughput)), a)
		c := unsafe.Slice((*float64)(unsafe.Pointer(res.algo_calc)), a)
		sd := unsafe.Slice((*float64)(unsafe.Pointer(res.stddev)), a)
		for i := range rows {
			rows[i] = Row{k[i], t[i], x[i], c[i], sd[i]}
		}
	}
	return rows
}

// DropWindow is the drop detector's batch job over a window of what the state holds, read-only (tad_drop_state): the window is
// RunWindow's; the rows are exactly those Run with Algo Drop returns over the window's points — AlgoCalc is the key's mean, Stddev
// pandas' sample std.  job.Algo is ignored (the call is the drop detector's), job.StartTime / EndTime must be 0.  Needs a state made
// by NewStateWithTimes.
func (s *State) DropWindow(job Job, nSigma float64, minSamples int32, fromT, toT int64, keepPoints uint64) ([]Row, error) {
	if !hasStateDrop() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no tad_drop_state (TAD_FEATURE_STATE_DROP)")
	}
	if !s.series || !s.times {
		return nil, IllegalArgument{"tadengine: DropWindow needs a state made by NewStateWithTimes"}
	}
	cj := dropJob(job, nSigma, minSamples)
	var res *C.tad_result
	if rc := C.tad_drop_state(s.e.h, s.h, &cj, C.int64_t(fromT), C.int64_t(toT), C.uint64_t(keepPoints), C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_drop_state: %s (code %d)", msg, int(rc))
	}
	return s.resultRows(res), nil
}

// DropStream is one batch of the periodical drop job (tad_drop_stream): the state advances exactly as under RunStream with EWMA; the
// rows are those Run with Algo Drop over everything the state now holds returns for this batch's points.  cols.NumKeys must equal
// the state's key count.  Needs a state made by NewStateWithSeries or NewStateWithTimes.
func (s *State) DropStream(job Job, nSigma float64, minSamples int32, cols Columns) ([]Row, error) {
	if !hasStateDrop() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no tad_drop_stream (TAD_FEATURE_STATE_DROP)")
	}
	if !s.series {
		return nil, IllegalArgument{"tadengine: DropStream needs a state made by NewStateWithSeries"}
	}
	bufs, n, narrow, err := columnBuffers(cols)
	if err != nil {
		return nil, err
	}
	defer freeBuffers(bufs)
	cj := dropJob(job, nSigma, minSamples)
	cj.flags = narrow
	cj.value_op = C.TAD_OP_AUTO
	var cc C.tad_columns
	cc.n_rows = C.uint64_t(n)
	cc.num_keys = C.uint64_t(cols.NumKeys)
	cc.memory = C.TAD_MEM_HOST
	cc.key_id = (*C.uint64_t)(bufs[0])
	cc.flow_end_s = (*C.int64_t)(bufs[2])
	cc.value = (*C.uint64_t)(bufs[4])
	var res *C.tad_result
	if rc := C.tad_drop_stream(s.e.h, s.h, &cj, &cc, C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_drop_stream: %s (code %d)", msg, int(rc))
	}
	return s.resultRows(res), nil
}

func (e *Engine) NewState(numKeys uint64) (*State, error) {
	var h *C.tad_state
	if rc := C.tad_state_create(e.h, C.uint64_t(numKeys), &h); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_state_create: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return &State{e: e, h: h}, nil
}

func (s *State) Close() {
	if s.h != nil {
		C.tad_state_destroy(s.e.h, s.h)
		s.h = nil
	}
}

// RunStream aggregates ONE new batch and continues every key's recurrences over its new points (tad_run_stream): the rows are the points
// with |x - ewma| > the running stddev_samp.  cols.NumKeys must equal the state's key count; job.Algo must be EWMA, DBSCAN on a state
// made by NewStateWithHistory (the rows are then the batch's points the batch job over everything seen so far calls noise), or ARIMA on
// a state made by NewStateWithSeries (the batch's points the batch job over everything seen so far calls anomalous).
func (s *State) RunStream(job Job, cols Columns) ([]Row, error) {
	bufs, n, narrow, err := columnBuffers(cols)
	if err != nil {
		return nil, err
	}
	defer freeBuffers(bufs)
	if job.Algo == DBSCAN && !s.history {
		return nil, IllegalArgument{"tadengine: streaming DBSCAN needs a state made by NewStateWithHistory"}
	}
	if job.Algo == ARIMA && !s.series {
		return nil, IllegalArgument{"tadengine: streaming ARIMA needs a state made by NewStateWithSeries"}
	}
	var cj C.tad_job
	cj.flags = narrow
	cj.algo = C.tad_algo(job.Algo)
	cj.agg_flow = C.tad_agg_flow(job.AggFlow)
	cj.value_op = C.TAD_OP_AUTO
	cj.dbscan_eps = C.double(job.DBSCANEps)
	cj.dbscan_min_samples = C.int32_t(job.DBSCANMinSamples)
	cj.arima_maxiter = C.int32_t(job.ARIMAMaxIter)
	var cc C.tad_columns
	cc.n_rows = C.uint64_t(n)
	cc.num_keys = C.uint64_t(cols.NumKeys)
	cc.memory = C.TAD_MEM_HOST
	cc.key_id = (*C.uint64_t)(bufs[0])
	cc.flow_end_s = (*C.int64_t)(bufs[2])
	cc.value = (*C.uint64_t)(bufs[4])
	var res *C.tad_result
	if rc := C.tad_run_stream(s.e.h, s.h, &cj, &cc, C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_run_stream: %s (code %d)", msg, int(rc))
	}
	defer C.tad_result_free(s.e.h, res)
	a := int(res.n_rows)
	rows := make([]Row, a)
	if a > 0 {
		k := unsafe.Slice((*uint64)(unsafe.Pointer(res.key_id)), a)
		t := unsafe.Slice((*int64)(unsafe.Pointer(res.flow_end_s)), a)
		x := unsafe.Slice((*float64)(unsafe.Pointer(res.throughput)), a)
		c := unsafe.Slice((*float64)(unsafe.Pointer(res.algo_calc)), a)
		sd := unsafe.Slice((*float64)(unsafe.Pointer(res.stddev)), a)
		for i := range rows {
			rows[i] = Row{k[i], t[i], x[i], c[i], sd[i]}
		}
	}
	return rows, nil
}

// Export copies the state to the host: per key the point count, Spark's avg and m2, the last EWMA value and the last flowEndSeconds.
func (s *State) Export(numKeys uint64) (n []uint32, avg, m2, ewma []float64, lastT []int64, err error) {
	n, avg, m2, ewma, lastT = make([]uint32, numKeys), make([]float64, numKeys), make([]float64, numKeys), make([]float64, numKeys), make([]int64, numKeys)
	if numKeys == 0 {
		return
	}
	if rc := C.tad_state_export(s.e.h, s.h, (*C.uint32_t)(unsafe.Pointer(&n[0])), (*C.double)(unsafe.Pointer(&avg[0])), (*C.double)(unsafe.Pointer(&m2[0])),
		(*C.double)(unsafe.Pointer(&ewma[0])), (*C.int64_t)(unsafe.Pointer(&lastT[0]))); rc != C.TAD_OK {
		err = fmt.Errorf("tad_state_export: %s (code %d)", C.GoString(C.tad_last_error(s.e.h)), int(rc))
	}
	return
}

// Resize grows the state's key space to numKeys (tad_state_resize, ABI 13): the added keys are unseen.  Fewer keys than the state
// holds is an error and leaves the state as it was; so does a failed allocation.
func (s *State) Resize(numKeys uint64) error {
	if rc := C.tad_state_resize(s.e.h, s.h, C.uint64_t(numKeys)); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return IllegalArgument{msg}
		}
		return fmt.Errorf("tad_state_resize: %s (code %d)", msg, int(rc))
	}
	return nil
}

// Import restores what Export returned (tad_state_import, ABI 13): one entry per key of the state in every slice; a key with
// n == 0 is stored as unseen.  A detector that restarts picks up every key's running sigma and EWMA where it left off.
func (s *State) Import(n []uint32, avg, m2, ewma []float64, lastT []int64) error {
	k := len(n)
	if len(avg) != k || len(m2) != k || len(ewma) != k || len(lastT) != k {
		return errors.New("tadengine: state slices differ in length")
	}
	if k == 0 {
		return errors.New("tadengine: empty state")
	}
	if rc := C.tad_state_import(s.e.h, s.h, (*C.uint32_t)(unsafe.Pointer(&n[0])), (*C.double)(unsafe.Pointer(&avg[0])), (*C.double)(unsafe.Pointer(&m2[0])),
		(*C.double)(unsafe.Pointer(&ewma[0])), (*C.int64_t)(unsafe.Pointer(&lastT[0]))); rc != C.TAD_OK {
		return fmt.Errorf("tad_state_import: %s (code %d)", C.GoString(C.tad_last_error(s.e.h)), int(rc))
	}
	return nil
}

// Progress feeds Status.CompletedStages / TotalStages (controller.go:426-453): the sum over the jobs in flight.
func (e *Engine) Progress() (done, total int) {
	var d, t C.int32_t
	C.tad_progress(e.h, &d, &t)
	return int(d), int(t)
}

// JobProgress is Progress for ONE job: the one whose Job.ID is id (Status.SparkApplication, controller.go:622); total == 0 when no
// such job is in flight.
func (e *Engine) JobProgress(id string) (done, total int) {
	cid := C.CString(id)
	defer C.free(unsafe.Pointer(cid))
	var d, t C.int32_t
	C.tad_job_progress(e.h, cid, &d, &t)
	return int(d), int(t)
}

// JobsInFlight: job contexts busy right now.
func (e *Engine) JobsInFlight() int { return int(C.tad_jobs_in_flight(e.h)) }

var keySelectOnce sync.Once
var keySelectOK bool

// hasKeySelect: the library knows tad_keydict_select / tad_run_state_keys / tad_drop_state_keys (tad_features); an older one would not
// export the calls.
func hasKeySelect() bool {
	keySelectOnce.Do(func() { keySelectOK = C.tad_features()&C.TAD_FEATURE_KEY_SELECT != 0 })
	return keySelectOK
}

// SelectTerm is one term of KeyDict.Select: the key is kept iff Mask[tuple[Col]] != 0.
type SelectTerm struct {
	Col  int32
	Mask []byte
}

// Select computes a key mask from the dictionary's tuples (tad_keydict_select): keep[k] = 1 iff key k's side is `side` (-1 = either) and
// every term's mask byte at the key's code is not 0.  numKeys must be the dictionary's NumKeys.  Up to 8 terms; a code outside a term's
// mask is an IllegalArgument.  The dictionary is only read.  The result is what State.RunKeys / State.DropKeys take.
func (d *KeyDict) Select(terms []SelectTerm, side int32, numKeys uint64) (keep []byte, selected uint64, err error) {
	if !hasKeySelect() {
		return nil, 0, errors.New("tadengine: libtad_mi355x.so has no tad_keydict_select (TAD_FEATURE_KEY_SELECT)")
	}
	if len(terms) > 8 {
		return nil, 0, IllegalArgument{"tadengine: Select takes at most 8 terms"}
	}
	// the three term arrays live in C memory for the call; the masks they name are pinned Go slices
	var pin runtime.Pinner
	defer pin.Unpin()
	ptrs := (*[8]*C.uint8_t)(C.calloc(8, C.size_t(unsafe.Sizeof(unsafe.Pointer(nil)))))
	defer C.free(unsafe.Pointer(ptrs))
	lens := (*[8]C.uint64_t)(C.calloc(8, 8))
	defer C.free(unsafe.Pointer(lens))
	colv := (*[8]C.int32_t)(C.calloc(8, 4))
	defer C.free(unsafe.Pointer(colv))
	for i, t := range terms {
		colv[i] = C.int32_t(t.Col)
		lens[i] = C.uint64_t(len(t.Mask))
		if len(t.Mask) > 0 {
			pin.Pin(&t.Mask[0])
			ptrs[i] = (*C.uint8_t)(unsafe.Pointer(&t.Mask[0]))
		}
	}
	keep = make([]byte, numKeys)
	var kp *C.uint8_t
	if numKeys > 0 {
		kp = (*C.uint8_t)(unsafe.Pointer(&keep[0]))
	}
	var n C.uint64_t
	if rc := C.tad_keydict_select(d.e.h, d.h, C.int32_t(len(terms)), &colv[0], &ptrs[0], &lens[0], C.int32_t(side), kp, C.uint64_t(numKeys),
		C.TAD_MEM_HOST, &n); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(d.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, 0, IllegalArgument{msg}
		}
		return nil, 0, fmt.Errorf("tad_keydict_select: %s (code %d)", msg, int(rc))
	}
	return keep, uint64(n), nil
}

// keysJob: the tad_job of a detector over selected keys of a state (RunKeys, RunSince).
func keysJob(job Job) C.tad_job {
	var cj C.tad_job
	cj.algo = C.tad_algo(job.Algo)
	cj.start_time = C.int64_t(job.StartTime)
	cj.end_time = C.int64_t(job.EndTime)
	cj.dbscan_eps = C.double(job.DBSCANEps)
	cj.dbscan_min_samples, cj.arima_maxiter = C.int32_t(job.DBSCANMinSamples), C.int32_t(job.ARIMAMaxIter)
	id := []byte(job.ID)
	if len(id) > 63 {
		id = id[:63]
	}
	for i, b := range id {
		cj.id[i] = C.char(b)
	}
	return cj
}

// RunKeys is RunWindow over the keys keyKeep selects, read-only (tad_run_state_keys): one byte per key of the state, any non-zero byte
// selects; nil is RunWindow itself.  The rows are exactly those of RunWindow whose key is selected, with the state's own key ids; a key
// that is not selected costs no fit.
func (s *State) RunKeys(job Job, fromT, toT int64, keepPoints uint64, keyKeep []byte) ([]Row, error) {
	if !hasKeySelect() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no tad_run_state_keys (TAD_FEATURE_KEY_SELECT)")
	}
	if !s.series || !s.times {
		return nil, IllegalArgument{"tadengine: RunKeys needs a state made by NewStateWithTimes"}
	}
	if job.Algo == DBSCAN && !s.history {
		return nil, IllegalArgument{"tadengine: RunKeys with DBSCAN needs a state made by NewStateWithTimes with history"}
	}
	cj := keysJob(job)
	var kp *C.uint8_t
	if len(keyKeep) > 0 {
		kp = (*C.uint8_t)(unsafe.Pointer(&keyKeep[0]))
	}
	var res *C.tad_result
	if rc := C.tad_run_state_keys(s.e.h, s.h, &cj, C.int64_t(fromT), C.int64_t(toT), C.uint64_t(keepPoints), kp, C.uint64_t(len(keyKeep)),
		C.TAD_MEM_HOST, C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_run_state_keys: %s (code %d)", msg, int(rc))
	}
	return s.resultRows(res), nil
}

// DropKeys is DropWindow over the keys keyKeep selects, read-only (tad_drop_state_keys); keyKeep as for RunKeys.
func (s *State) DropKeys(job Job, nSigma float64, minSamples int32, fromT, toT int64, keepPoints uint64, keyKeep []byte) ([]Row, error) {
	if !hasKeySelect() {
		return nil, errors.New("tadengine: libtad_mi355x.so has no tad_drop_state_keys (TAD_FEATURE_KEY_SELECT)")
	}
	if !s.series || !s.times {
		return nil, IllegalArgument{"tadengine: DropKeys needs a state made by NewStateWithTimes"}
	}
	cj := dropJob(job, nSigma, minSamples)
	var kp *C.uint8_t
	if len(keyKeep) > 0 {
		kp = (*C.uint8_t)(unsafe.Pointer(&keyKeep[0]))
	}
	var res *C.tad_result
	if rc := C.tad_drop_state_keys(s.e.h, s.h, &cj, C.int64_t(fromT), C.int64_t(toT), C.uint64_t(keepPoints), kp, C.uint64_t(len(keyKeep)),
		C.TAD_MEM_HOST, C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_drop_state_keys: %s (code %d)", msg, int(rc))
	}
	return s.resultRows(res), nil
}

var stateAlertsOnce sync.Once
var stateAlertsOK bool

// hasStateAlerts: the library knows the change report and the since calls (tad_features); an older one would not export them.
func hasStateAlerts() bool {
	stateAlertsOnce.Do(func() { stateAlertsOK = C.tad_features()&C.TAD_FEATURE_STATE_ALERTS != 0 })
	return stateAlertsOK
}

var errNoStateAlerts = errors.New("tadengine: libtad_mi355x.so has no change report (TAD_FEATURE_STATE_ALERTS)")

// NoChange marks a key of Changes.KeySince whose series did not change (TAD_NO_CHANGE).
const NoChange = int64(math.MaxInt64)

// Changes is what a MergeChanges or a ReplaceChanges changed (tad_changes): KeySince[k] is the smallest flowEndSeconds at which key k's
// series changed — a point added, erased, or given another value — and NoChange where it did not.  A sum of 0, a maximum not above the
// held value and a replace by the held value change nothing: the same Replace twice reports KeysChanged == 0 the second time.
type Changes struct {
	KeySince      []int64
	KeysChanged   uint64
	PointsChanged uint64
	MinT, MaxT    int64 // 0, 0 when PointsChanged == 0
}

// batchCall: the tad_job and tad_columns of a merge or a replace — Merge, Replace and their *Changes forms; free releases the column buffers.
func batchCall(job Job, cols Columns) (cj C.tad_job, cc C.tad_columns, free func(), err error) {
	bufs, n, narrow, err := columnBuffers(cols)
	if err != nil {
		return cj, cc, func() {}, err
	}
	cj.flags = narrow
	cj.algo = C.TAD_ALGO_EWMA
	cj.agg_flow = C.tad_agg_flow(job.AggFlow)
	cj.value_op = C.TAD_OP_AUTO
	cj.start_time = C.int64_t(job.StartTime)
	cj.end_time = C.int64_t(job.EndTime)
	id := []byte(job.ID)
	if len(id) > 63 {
		id = id[:63]
	}
	for i, b := range id {
		cj.id[i] = C.char(b)
	}
	cc.n_rows = C.uint64_t(n)
	cc.num_keys = C.uint64_t(cols.NumKeys)
	cc.memory = C.TAD_MEM_HOST
	cc.key_id = (*C.uint64_t)(bufs[0])
	cc.key_id2 = (*C.uint64_t)(bufs[1])
	cc.flow_end_s = (*C.int64_t)(bufs[2])
	cc.flow_start_s = (*C.int64_t)(bufs[3])
	cc.value = (*C.uint64_t)(bufs[4])
	return cj, cc, func() { freeBuffers(bufs) }, nil
}

// newChanges: a report with one entry per key of the batch's key space (which must be the state's), in C memory so that the library
// may write it; done copies it out and frees it.
func newChanges(numKeys uint64) (ch C.tad_changes, done func() Changes) {
	var p unsafe.Pointer
	if numKeys > 0 {
		p = C.malloc(C.size_t(numKeys * 8))
	}
	ch.key_since = (*C.int64_t)(p)
	ch.len = C.uint64_t(numKeys)
	ch.memory = C.TAD_MEM_HOST
	return ch, func() Changes {
		out := Changes{KeySince: make([]int64, numKeys), KeysChanged: uint64(ch.keys_changed), PointsChanged: uint64(ch.points_changed),
			MinT: int64(ch.min_t), MaxT: int64(ch.max_t)}
		if numKeys > 0 {
			copy(out.KeySince, unsafe.Slice((*int64)(p), numKeys))
			C.free(p)
		}
		return out
	}
}

// MergeChanges is Merge that also reports what it changed (tad_state_merge_changes).
func (s *State) MergeChanges(job Job, cols Columns, keepFrom int64) (MergeStats, Changes, error) {
	if !hasStateAlerts() {
		return MergeStats{}, Changes{}, errNoStateAlerts
	}
	if !s.series || !s.times {
		return MergeStats{}, Changes{}, IllegalArgument{"tadengine: MergeChanges needs a state made by NewStateWithTimes"}
	}
	cj, cc, free, err := batchCall(job, cols)
	if err != nil {
		return MergeStats{}, Changes{}, err
	}
	defer free()
	ch, done := newChanges(cols.NumKeys)
	var ms C.tad_merge_stats
	rc := C.tad_state_merge_changes(s.e.h, s.h, &cj, &cc, C.int64_t(keepFrom), &ms, &ch)
	changes := done()
	if rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return MergeStats{}, Changes{}, IllegalArgument{msg}
		}
		return MergeStats{}, Changes{}, fmt.Errorf("tad_state_merge_changes: %s (code %d)", msg, int(rc))
	}
	return MergeStats{RowsIn: uint64(ms.rows_in), RowsUsed: uint64(ms.rows_used), BatchPoints: uint64(ms.batch_points),
		PointsTooOld: uint64(ms.points_too_old), PointsAppended: uint64(ms.points_appended), PointsInserted: uint64(ms.points_inserted),
		PointsCombined: uint64(ms.points_combined), KeysTouched: uint64(ms.keys_touched), KeysReplayed: uint64(ms.keys_replayed),
		MsTotal: float32(ms.ms_total)}, changes, nil
}

// ReplaceChanges is Replace that also reports what it changed (tad_state_replace_changes): the poll loop's alerts come from RunSince
// with the report's KeySince, and a turn made twice reports no changed key the second time.
func (s *State) ReplaceChanges(job Job, cols Columns, ranged bool, fromT, toT, keepFrom int64) (ReplaceStats, Changes, error) {
	if !hasStateAlerts() {
		return ReplaceStats{}, Changes{}, errNoStateAlerts
	}
	if !s.series || !s.times {
		return ReplaceStats{}, Changes{}, IllegalArgument{"tadengine: ReplaceChanges needs a state made by NewStateWithTimes"}
	}
	cj, cc, free, err := batchCall(job, cols)
	if err != nil {
		return ReplaceStats{}, Changes{}, err
	}
	defer free()
	var flags C.uint32_t
	if ranged {
		flags = C.TAD_REPLACE_RANGE
	}
	ch, done := newChanges(cols.NumKeys)
	var rs C.tad_replace_stats
	rc := C.tad_state_replace_changes(s.e.h, s.h, &cj, &cc, flags, C.int64_t(fromT), C.int64_t(toT), C.int64_t(keepFrom), &rs, &ch)
	changes := done()
	if rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return ReplaceStats{}, Changes{}, IllegalArgument{msg}
		}
		return ReplaceStats{}, Changes{}, fmt.Errorf("tad_state_replace_changes: %s (code %d)", msg, int(rc))
	}
	return ReplaceStats{RowsIn: uint64(rs.rows_in), RowsUsed: uint64(rs.rows_used), BatchPoints: uint64(rs.batch_points),
		PointsTooOld: uint64(rs.points_too_old), PointsAppended: uint64(rs.points_appended), PointsInserted: uint64(rs.points_inserted),
		PointsReplaced: uint64(rs.points_replaced), PointsErased: uint64(rs.points_erased), KeysEmptied: uint64(rs.keys_emptied),
		KeysTouched: uint64(rs.keys_touched), KeysReplayed: uint64(rs.keys_replayed), MsTotal: float32(rs.ms_total)}, changes, nil
}

// ReportWindow says which of the state's points a RunSince / DropSince judges and which of those it reports (tad_report_window):
// the window and the key mask of RunKeys; KeySince (one entry per key, or nil) and SinceT (0 = none) name the reported points — those
// with flowEndSeconds >= SinceT and >= KeySince[key].  A key whose KeySince is NoChange is not selected at all.
type ReportWindow struct {
	FromT, ToT int64
	KeepPoints uint64
	KeyKeep    []byte
	KeySince   []int64
	SinceT     int64
}

func (w ReportWindow) c() (C.tad_report_window, error) {
	var cw C.tad_report_window
	cw.from_t, cw.to_t, cw.keep_points, cw.since_t = C.int64_t(w.FromT), C.int64_t(w.ToT), C.uint64_t(w.KeepPoints), C.int64_t(w.SinceT)
	cw.key_memory = C.TAD_MEM_HOST
	if len(w.KeyKeep) > 0 && len(w.KeySince) > 0 && len(w.KeyKeep) != len(w.KeySince) {
		return cw, IllegalArgument{"tadengine: KeyKeep and KeySince must have one entry per key of the state each"}
	}
	if len(w.KeyKeep) > 0 {
		cw.key_keep = (*C.uint8_t)(unsafe.Pointer(&w.KeyKeep[0]))
		cw.num_keys = C.uint64_t(len(w.KeyKeep))
	}
	if len(w.KeySince) > 0 {
		cw.key_since = (*C.int64_t)(unsafe.Pointer(&w.KeySince[0]))
		cw.num_keys = C.uint64_t(len(w.KeySince))
	}
	return cw, nil
}

// RunSince judges the window as RunKeys does and reports from a time on, read-only (tad_run_state_since): exactly the rows of RunKeys
// with the same window and the effective mask, restricted to the reported points.  Points of a changed key before its first changed
// time may have changed verdict and are not reported: RunKeys gives the whole answer.
func (s *State) RunSince(job Job, w ReportWindow) ([]Row, error) {
	if !hasStateAlerts() {
		return nil, errNoStateAlerts
	}
	if !s.series || !s.times {
		return nil, IllegalArgument{"tadengine: RunSince needs a state made by NewStateWithTimes"}
	}
	if job.Algo == DBSCAN && !s.history {
		return nil, IllegalArgument{"tadengine: RunSince with DBSCAN needs a state made by NewStateWithTimes with history"}
	}
	cj := keysJob(job)
	cw, err := w.c()
	if err != nil {
		return nil, err
	}
	var pin runtime.Pinner // (the struct points into Go memory: cgo passes &cw, the slices it names are pinned for the call)
	defer pin.Unpin()
	if len(w.KeyKeep) > 0 {
		pin.Pin(&w.KeyKeep[0])
	}
	if len(w.KeySince) > 0 {
		pin.Pin(&w.KeySince[0])
	}
	var res *C.tad_result
	if rc := C.tad_run_state_since(s.e.h, s.h, &cj, &cw, C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_run_state_since: %s (code %d)", msg, int(rc))
	}
	return s.resultRows(res), nil
}

// DropSince is DropKeys that reports from a time on, read-only (tad_drop_state_since); w as for RunSince.
func (s *State) DropSince(job Job, nSigma float64, minSamples int32, w ReportWindow) ([]Row, error) {
	if !hasStateAlerts() {
		return nil, errNoStateAlerts
	}
	if !s.series || !s.times {
		return nil, IllegalArgument{"tadengine: DropSince needs a state made by NewStateWithTimes"}
	}
	cj := dropJob(job, nSigma, minSamples)
	cw, err := w.c()
	if err != nil {
		return nil, err
	}
	var pin runtime.Pinner
	defer pin.Unpin()
	if len(w.KeyKeep) > 0 {
		pin.Pin(&w.KeyKeep[0])
	}
	if len(w.KeySince) > 0 {
		pin.Pin(&w.KeySince[0])
	}
	var res *C.tad_result
	if rc := C.tad_drop_state_since(s.e.h, s.h, &cj, &cw, C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_drop_state_since: %s (code %d)", msg, int(rc))
	}
	return s.resultRows(res), nil
}

var stateBucketsOnce sync.Once
var stateBucketsOK bool

// hasStateBuckets: the library knows tad_run_state_buckets (tad_features); an older one would not export it.
func hasStateBuckets() bool {
	stateBucketsOnce.Do(func() { stateBucketsOK = C.tad_features()&C.TAD_FEATURE_STATE_BUCKETS != 0 })
	return stateBucketsOK
}

var errNoStateBuckets = errors.New("tadengine: libtad_mi355x.so has no bucketed state job (TAD_FEATURE_STATE_BUCKETS)")

// ValueOp is how the points of one bucket are folded (tad_value_op): OpSum wraps mod 2^64, OpMax is the unsigned maximum.
type ValueOp int

const (
	OpMax ValueOp = ValueOp(C.TAD_OP_MAX)
	OpSum ValueOp = ValueOp(C.TAD_OP_SUM)
)

// BucketWindow is a ReportWindow whose judged points are folded into time buckets (tad_bucket_window): a point of second t lies in the
// bucket that starts at Origin + BucketS*floor((t-Origin)/BucketS), the points of a bucket are summed (mod 2^64) or, with Op == OpMax,
// reduced to their maximum, and the bucket's start stands in the rows' FlowEndS.  BucketS >= 1, 0 <= Origin < BucketS; Op is OpSum or
// OpMax.  The window (FromT, ToT, KeepPoints, KeyKeep) acts on the raw points, first; a bucket is reported iff it starts at or after the
// start of the bucket that holds the since threshold.
type BucketWindow struct {
	ReportWindow
	BucketS int64
	Origin  int64
	Op      ValueOp
}

// RunBuckets judges the state's window in time buckets, read-only (tad_run_state_buckets): exactly the rows Engine.Run returns for the
// window's rows with their times floored to the bucket starts and ValueOp = w.Op.  BucketS == 1 is RunKeys / RunSince.
func (s *State) RunBuckets(job Job, w BucketWindow) ([]Row, error) {
	if !hasStateBuckets() {
		return nil, errNoStateBuckets
	}
	if !s.series || !s.times {
		return nil, IllegalArgument{"tadengine: RunBuckets needs a state made by NewStateWithTimes"}
	}
	if job.Algo == DBSCAN && !s.history {
		return nil, IllegalArgument{"tadengine: RunBuckets with DBSCAN needs a state made by NewStateWithTimes with history"}
	}
	if w.BucketS < 1 || w.Origin < 0 || w.Origin >= w.BucketS {
		return nil, IllegalArgument{"tadengine: BucketS must be >= 1 and 0 <= Origin < BucketS"}
	}
	cj := keysJob(job)
	rw, err := w.ReportWindow.c()
	if err != nil {
		return nil, err
	}
	var cw C.tad_bucket_window
	cw.from_t, cw.to_t, cw.keep_points, cw.since_t = rw.from_t, rw.to_t, rw.keep_points, rw.since_t
	cw.key_keep, cw.key_since, cw.num_keys, cw.key_memory = rw.key_keep, rw.key_since, rw.num_keys, rw.key_memory
	cw.bucket_s, cw.bucket_origin, cw.bucket_op = C.int64_t(w.BucketS), C.int64_t(w.Origin), C.tad_value_op(w.Op)
	var pin runtime.Pinner // (the struct points into Go memory: cgo passes &cw, the slices it names are pinned for the call)
	defer pin.Unpin()
	if len(w.KeyKeep) > 0 {
		pin.Pin(&w.KeyKeep[0])
	}
	if len(w.KeySince) > 0 {
		pin.Pin(&w.KeySince[0])
	}
	var res *C.tad_result
	if rc := C.tad_run_state_buckets(s.e.h, s.h, &cj, &cw, C.TAD_MEM_HOST, &res); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, IllegalArgument{msg}
		}
		return nil, fmt.Errorf("tad_run_state_buckets: %s (code %d)", msg, int(rc))
	}
	return s.resultRows(res), nil
}

var stateRollupOnce sync.Once
var stateRollupOK bool

// hasStateRollup: the library knows tad_state_rollup (tad_features); an older one would not export it.
func hasStateRollup() bool {
	stateRollupOnce.Do(func() { stateRollupOK = C.tad_features()&C.TAD_FEATURE_STATE_ROLLUP != 0 })
	return stateRollupOK
}

var errNoStateRollup = errors.New("tadengine: libtad_mi355x.so has no state roll-up (TAD_FEATURE_STATE_ROLLUP)")

// RollupStats is what one Rollup call folded (tad_rollup_stats).
type RollupStats struct {
	PointsBefore uint64  // series points of the state before and
	PointsAfter  uint64  // after the call
	PointsRolled uint64  // raw points that lay below the bound
	Buckets      uint64  // points the state holds below the bound afterwards
	KeysChanged  uint64  // keys that lost at least one point
	BeforeT      int64   // the bound that was applied: Before floored to a bucket start
	MsTotal      float64 // HIP events
	JobContext   int32
}

// Rollup folds every key's points older than before into time buckets, in place (tad_state_rollup): before is floored to a bucket start
// b; below b the points of one key and bucket become one point at the bucket's start (op: OpSum, wrapping, or OpMax), at or after b
// nothing changes.  The state becomes that of a fresh state streamed the folded points with EWMA parameter alpha (0 -> 0.5); a key whose
// newest point lay below b gets that point's bucket start as its last time.  Idempotent; RunBuckets at a multiple of bucketS with a
// congruent origin and the same op returns what it returned before the roll-up.  Needs a state made by NewStateWithTimes.
func (s *State) Rollup(before, bucketS, origin int64, op ValueOp, alpha float64) (RollupStats, error) {
	if !hasStateRollup() {
		return RollupStats{}, errNoStateRollup
	}
	if !s.series || !s.times {
		return RollupStats{}, IllegalArgument{"tadengine: Rollup needs a state made by NewStateWithTimes"}
	}
	if bucketS < 1 || origin < 0 || origin >= bucketS {
		return RollupStats{}, IllegalArgument{"tadengine: bucketS must be >= 1 and 0 <= origin < bucketS"}
	}
	var ru C.tad_rollup_stats
	if rc := C.tad_state_rollup(s.e.h, s.h, C.int64_t(before), C.int64_t(bucketS), C.int64_t(origin), C.tad_value_op(op), C.double(alpha), &ru); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(s.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return RollupStats{}, IllegalArgument{msg}
		}
		return RollupStats{}, fmt.Errorf("tad_state_rollup: %s (code %d)", msg, int(rc))
	}
	return RollupStats{PointsBefore: uint64(ru.points_before), PointsAfter: uint64(ru.points_after), PointsRolled: uint64(ru.points_rolled),
		Buckets: uint64(ru.buckets), KeysChanged: uint64(ru.keys_changed), BeforeT: int64(ru.before_t), MsTotal: float64(ru.ms_total),
		JobContext: int32(ru.job_context)}, nil
}

var stringDictOnce sync.Once
var stringDictOK bool

// hasStringDict: the library knows the persistent string dictionary (tad_features); an older one would not export the calls.
func hasStringDict() bool {
	stringDictOnce.Do(func() { stringDictOK = C.tad_features()&C.TAD_FEATURE_STRING_DICT != 0 })
	return stringDictOK
}

var errNoStringDict = errors.New("tadengine: libtad_mi355x.so has no string dictionary (TAD_FEATURE_STRING_DICT)")

// Match operations of StringDict.Match (TAD_STR_*).
const (
	StrEqual          int32 = 0 // the value's bytes are the pattern's bytes
	StrContainsNoCase int32 = 1 // the pattern occurs in the value; 'A'..'Z' fold to 'a'..'z', every other byte matches only itself
)

// CodeNone is what Lookup gives a string the dictionary does not hold (TAD_CODE_NONE).
const CodeNone int64 = -1

// StringDict is a string dictionary kept in HBM that outlives the call (tad_strdict): the strings of a key column -> codes that stay the
// same from batch to batch, new codes in order of first appearance.  One per string key column, in front of the KeyDict: Encode every
// batch's column, hand the codes to KeyDict.Encode, and build the job filters' masks with Match.
type StringDict struct {
	e *Engine
	h *C.tad_strdict
}

// NewStringDict makes an empty dictionary.  expectedValues sizes the first table and records, expectedBytes the first arena (0 = the defaults).
func (e *Engine) NewStringDict(expectedValues, expectedBytes uint64) (*StringDict, error) {
	if !hasStringDict() {
		return nil, errNoStringDict
	}
	var h *C.tad_strdict
	if rc := C.tad_strdict_create(e.h, C.uint64_t(expectedValues), C.uint64_t(expectedBytes), &h); rc != C.TAD_OK {
		return nil, fmt.Errorf("tad_strdict_create: %s (code %d)", C.GoString(C.tad_last_error(e.h)), int(rc))
	}
	return &StringDict{e: e, h: h}, nil
}

func (d *StringDict) Close() {
	if d.h != nil {
		C.tad_strdict_destroy(d.e.h, d.h)
		d.h = nil
	}
}

func (d *StringDict) fail(call string, rc C.int) error {
	msg := C.GoString(C.tad_last_error(d.e.h))
	if rc == C.TAD_ERR_INVALID_ARGUMENT {
		return IllegalArgument{msg}
	}
	return fmt.Errorf("%s: %s (code %d)", call, msg, int(rc))
}

// stringBatch copies one Arrow string column — offsets (n + 1, starting anywhere) and the bytes they address — into C memory (no Go
// pointer is stored in the struct) and fills the tad_string_column.  release frees the copies.
func stringBatch(offsets []int64, data []byte) (sb *C.tad_string_column, n int, release func(), err error) {
	if len(offsets) == 0 {
		return nil, 0, nil, IllegalArgument{"tadengine: a string column has n + 1 offsets"}
	}
	n = len(offsets) - 1
	var bufs []unsafe.Pointer
	release = func() {
		for _, p := range bufs {
			if p != nil {
				C.free(p)
			}
		}
	}
	sb = (*C.tad_string_column)(C.calloc(1, C.size_t(unsafe.Sizeof(C.tad_string_column{}))))
	bufs = append(bufs, unsafe.Pointer(sb))
	off := cColumn(offsets)
	bufs = append(bufs, off)
	sb.n_rows = C.uint64_t(n)
	sb.offsets = off
	sb.offset_bits = 64
	if len(data) > 0 {
		p := C.CBytes(data)
		bufs = append(bufs, p)
		sb.data = (*C.uint8_t)(p)
	}
	sb.data_bytes = C.uint64_t(len(data))
	sb.memory = C.TAD_MEM_HOST
	return sb, n, release, nil
}

// Encode maps one batch's strings to codes (tad_strdict_encode): row i is data[offsets[i]:offsets[i+1]].  Strings the dictionary holds
// keep their codes; new ones get numBefore, numBefore + 1, ... in order of first appearance; newFirstRow[j] = the row of THIS batch
// where value numBefore + j first appears: the caller reads the new string there.
func (d *StringDict) Encode(offsets []int64, data []byte) (codes []int64, newFirstRow []uint64, numBefore uint64, err error) {
	if !hasStringDict() {
		return nil, nil, 0, errNoStringDict
	}
	sb, n, release, err := stringBatch(offsets, data)
	if err != nil {
		return nil, nil, 0, err
	}
	defer release()
	codes = make([]int64, n)
	newFirstRow = make([]uint64, n)
	var cp *C.int64_t
	var fr *C.uint64_t
	if n > 0 {
		cp = (*C.int64_t)(unsafe.Pointer(&codes[0]))
		fr = (*C.uint64_t)(unsafe.Pointer(&newFirstRow[0]))
	}
	var before, after C.uint64_t
	if rc := C.tad_strdict_encode(d.e.h, d.h, sb, cp, fr, C.uint64_t(n), &before, &after); rc != C.TAD_OK {
		return nil, nil, 0, d.fail("tad_strdict_encode", rc)
	}
	return codes, newFirstRow[:int(after-before)], uint64(before), nil
}

// Lookup is Encode read-only (tad_strdict_lookup): an unknown string gets CodeNone and the dictionary is unchanged.
func (d *StringDict) Lookup(offsets []int64, data []byte) (codes []int64, err error) {
	if !hasStringDict() {
		return nil, errNoStringDict
	}
	sb, n, release, err := stringBatch(offsets, data)
	if err != nil {
		return nil, err
	}
	defer release()
	codes = make([]int64, n)
	var cp *C.int64_t
	if n > 0 {
		cp = (*C.int64_t)(unsafe.Pointer(&codes[0]))
	}
	if rc := C.tad_strdict_lookup(d.e.h, d.h, sb, cp); rc != C.TAD_OK {
		return nil, d.fail("tad_strdict_lookup", rc)
	}
	return codes, nil
}

// NumValues is the number of values the dictionary holds (tad_strdict_num_values): the length of a Match mask.
func (d *StringDict) NumValues() (uint64, error) {
	if !hasStringDict() {
		return 0, errNoStringDict
	}
	var n C.uint64_t
	if rc := C.tad_strdict_num_values(d.e.h, d.h, &n); rc != C.TAD_OK {
		return 0, d.fail("tad_strdict_num_values", rc)
	}
	return uint64(n), nil
}

// Bytes is the device memory the dictionary holds: table, records and arena at their capacity (tad_strdict_bytes).
func (d *StringDict) Bytes() (uint64, error) {
	if !hasStringDict() {
		return 0, errNoStringDict
	}
	var n C.uint64_t
	if rc := C.tad_strdict_bytes(d.e.h, d.h, &n); rc != C.TAD_OK {
		return 0, d.fail("tad_strdict_bytes", rc)
	}
	return uint64(n), nil
}

// Export returns the values [firstCode, firstCode + nValues) in Arrow's layout (tad_strdict_export): nValues + 1 offsets starting at 0
// and the packed bytes — what Import takes after a restart, and where the host reads the strings of result rows.
func (d *StringDict) Export(firstCode, nValues uint64) (offsets []int64, data []byte, err error) {
	if !hasStringDict() {
		return nil, nil, errNoStringDict
	}
	var need C.uint64_t
	if rc := C.tad_strdict_export(d.e.h, d.h, C.uint64_t(firstCode), C.uint64_t(nValues), nil, nil, 0, &need); rc != C.TAD_OK {
		return nil, nil, d.fail("tad_strdict_export", rc)
	}
	offsets = make([]int64, nValues+1)
	data = make([]byte, uint64(need))
	var dp *C.uint8_t
	if len(data) > 0 {
		dp = (*C.uint8_t)(unsafe.Pointer(&data[0]))
	}
	if rc := C.tad_strdict_export(d.e.h, d.h, C.uint64_t(firstCode), C.uint64_t(nValues), (*C.int64_t)(unsafe.Pointer(&offsets[0])), dp, need, &need); rc != C.TAD_OK {
		return nil, nil, d.fail("tad_strdict_export", rc)
	}
	return offsets, data, nil
}

// Import fills this EMPTY dictionary so that value i is data[offsets[i]:offsets[i+1]] (tad_strdict_import): what Export returned.
// Two equal strings, offsets that do not start at 0 or decrease, or a dictionary that holds values are refused; nothing changes then.
func (d *StringDict) Import(offsets []int64, data []byte) error {
	if !hasStringDict() {
		return errNoStringDict
	}
	if len(offsets) == 0 {
		return IllegalArgument{"tadengine: a string column has n + 1 offsets"}
	}
	var dp *C.uint8_t
	if len(data) > 0 {
		dp = (*C.uint8_t)(unsafe.Pointer(&data[0]))
	}
	if rc := C.tad_strdict_import(d.e.h, d.h, C.uint64_t(len(offsets)-1), (*C.int64_t)(unsafe.Pointer(&offsets[0])), dp); rc != C.TAD_OK {
		return d.fail("tad_strdict_import", rc)
	}
	return nil
}

// Match evaluates one string predicate on every value (tad_strdict_match): mask[c] = 1 iff value c satisfies op (StrEqual,
// StrContainsNoCase) with the pattern (at most 1024 bytes).  The mask is a term of KeyDict.Select.
func (d *StringDict) Match(op int32, pattern []byte) (mask []byte, matched uint64, err error) {
	if !hasStringDict() {
		return nil, 0, errNoStringDict
	}
	n, err := d.NumValues()
	if err != nil {
		return nil, 0, err
	}
	mask = make([]byte, n)
	var mp, pp *C.uint8_t
	if n > 0 {
		mp = (*C.uint8_t)(unsafe.Pointer(&mask[0]))
	}
	if len(pattern) > 0 {
		pp = (*C.uint8_t)(unsafe.Pointer(&pattern[0]))
	}
	var hit C.uint64_t
	if rc := C.tad_strdict_match(d.e.h, d.h, C.int32_t(op), pp, C.uint64_t(len(pattern)), mp, C.uint64_t(n), C.TAD_MEM_HOST, &hit); rc != C.TAD_OK {
		return nil, 0, d.fail("tad_strdict_match", rc)
	}
	return mask, uint64(hit), nil
}

var stringLikeOnce sync.Once
var stringLikeOK bool

// hasStringLike: the library matches LIKE patterns on the device (tad_features); an older one would not export the call.  Like the rest
// of this binding the method below is never compiled in the project's checks (no Go toolchain runs there): it is written against
// include/tad.h and read by tests/test_string_like_abi.py as text.
func hasStringLike() bool {
	stringLikeOnce.Do(func() { stringLikeOK = C.tad_features()&C.TAD_FEATURE_STRING_LIKE != 0 })
	return stringLikeOK
}

var errNoStringLike = errors.New("tadengine: libtad_mi355x.so matches no LIKE patterns (TAD_FEATURE_STRING_LIKE)")

// Like evaluates a LIKE pattern on every value (tad_strdict_like): mask[c] = 1 iff the pattern (at most 1024 bytes) matches the WHOLE of
// value c.  % matches any run of bytes, _ exactly one character, \ makes the next byte a literal; nocase folds 'A'..'Z' to 'a'..'z'
// (ilike).  The job's label filter is Like([]byte("%"+label+"%"), true).  The mask is a term of KeyDict.Select.
func (d *StringDict) Like(pattern []byte, nocase bool) (mask []byte, matched uint64, err error) {
	if !hasStringLike() {
		return nil, 0, errNoStringLike
	}
	n, err := d.NumValues()
	if err != nil {
		return nil, 0, err
	}
	mask = make([]byte, n)
	var mp, pp *C.uint8_t
	if n > 0 {
		mp = (*C.uint8_t)(unsafe.Pointer(&mask[0]))
	}
	if len(pattern) > 0 {
		pp = (*C.uint8_t)(unsafe.Pointer(&pattern[0]))
	}
	var flags C.uint32_t
	if nocase {
		flags = C.TAD_LIKE_NOCASE
	}
	var hit C.uint64_t
	if rc := C.tad_strdict_like(d.e.h, d.h, pp, C.uint64_t(len(pattern)), flags, mp, C.uint64_t(n), C.TAD_MEM_HOST, &hit); rc != C.TAD_OK {
		return nil, 0, d.fail("tad_strdict_like", rc)
	}
	return mask, uint64(hit), nil
}

var dictDecodeOnce sync.Once
var dictDecodeOK bool

// hasDictDecode: the library decodes on the device (tad_features); an older one would not export the two calls.
func hasDictDecode() bool {
	dictDecodeOnce.Do(func() { dictDecodeOK = C.tad_features()&C.TAD_FEATURE_DICT_DECODE != 0 })
	return dictDecodeOK
}

var errNoDictDecode = errors.New("tadengine: libtad_mi355x.so has no device decode (TAD_FEATURE_DICT_DECODE)")

// Gather returns the tuples of arbitrary keys column by column, and their sides (tad_keydict_gather): cols[c][i] is column c of key
// keyID[i].  Ids may repeat and come in any order; an id that is not below NumKeys is an IllegalArgument.
func (d *KeyDict) Gather(keyID []uint64) (cols [][]int64, side []byte, err error) {
	if !hasDictDecode() {
		return nil, nil, errNoDictDecode
	}
	n := len(keyID)
	cols = make([][]int64, d.nCols)
	side = make([]byte, n)
	// the pointer array and the columns it names live in C memory for the call (no Go pointer inside C memory)
	arr := (*[8]*C.int64_t)(C.calloc(8, C.size_t(unsafe.Sizeof(unsafe.Pointer(nil)))))
	defer C.free(unsafe.Pointer(arr))
	for c := range cols {
		cols[c] = make([]int64, n)
		arr[c] = (*C.int64_t)(C.calloc(C.size_t(n)+1, 8))
		defer C.free(unsafe.Pointer(arr[c]))
	}
	var kp *C.uint64_t
	var sp *C.uint8_t
	if n > 0 {
		kp = (*C.uint64_t)(unsafe.Pointer(&keyID[0]))
		sp = (*C.uint8_t)(unsafe.Pointer(&side[0]))
	}
	if rc := C.tad_keydict_gather(d.e.h, d.h, kp, C.uint64_t(n), C.TAD_MEM_HOST, &arr[0], sp); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(d.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, nil, IllegalArgument{msg}
		}
		return nil, nil, fmt.Errorf("tad_keydict_gather: %s (code %d)", msg, int(rc))
	}
	for c := range cols {
		copy(cols[c], unsafe.Slice((*int64)(unsafe.Pointer(arr[c])), n))
	}
	return cols, side, nil
}

// Decode returns the values of arbitrary codes in Arrow's layout (tad_strdict_decode): len(codes) + 1 offsets starting at 0 and the
// packed bytes — value codes[i] is data[offsets[i]:offsets[i+1]].  A code that is not in [0, NumValues) is an IllegalArgument.
func (d *StringDict) Decode(codes []int64) (offsets []int64, data []byte, err error) {
	if !hasDictDecode() {
		return nil, nil, errNoDictDecode
	}
	n := len(codes)
	var cp *C.int64_t
	if n > 0 {
		cp = (*C.int64_t)(unsafe.Pointer(&codes[0]))
	}
	var need C.uint64_t
	if rc := C.tad_strdict_decode(d.e.h, d.h, cp, C.uint64_t(n), C.TAD_MEM_HOST, nil, nil, 0, C.TAD_MEM_HOST, &need); rc != C.TAD_OK {
		return nil, nil, d.fail("tad_strdict_decode", rc)
	}
	offsets = make([]int64, n+1)
	data = make([]byte, uint64(need))
	var dp *C.uint8_t
	if len(data) > 0 {
		dp = (*C.uint8_t)(unsafe.Pointer(&data[0]))
	}
	if rc := C.tad_strdict_decode(d.e.h, d.h, cp, C.uint64_t(n), C.TAD_MEM_HOST, (*C.int64_t)(unsafe.Pointer(&offsets[0])), dp, need, C.TAD_MEM_HOST, &need); rc != C.TAD_OK {
		return nil, nil, d.fail("tad_strdict_decode", rc)
	}
	return offsets, data, nil
}

var stringRetireOnce sync.Once
var stringRetireOK bool

// hasStringRetire: the library retires strings (tad_features); an older one would not export the three calls.  Like the rest of this
// binding the three methods below are never compiled in the project's checks (no Go toolchain runs there): they are written against
// include/tad.h and read by tests/test_string_retire_abi.py as text.
func hasStringRetire() bool {
	stringRetireOnce.Do(func() { stringRetireOK = C.tad_features()&C.TAD_FEATURE_STRING_RETIRE != 0 })
	return stringRetireOK
}

var errNoStringRetire = errors.New("tadengine: libtad_mi355x.so retires no strings (TAD_FEATURE_STRING_RETIRE)")

// CodeNone is remap's entry for a retired value (TAD_CODE_NONE).
const CodeNone = int64(-1)

// StrdictCompactStats is what one StringDict.Compact retired (tad_strdict_compact_stats).
type StrdictCompactStats struct {
	ValuesBefore, ValuesAfter       uint64
	BytesBefore, BytesAfter         uint64 // tad_strdict_bytes at entry and at exit
	ArenaUsedBefore, ArenaUsedAfter uint64 // padded bytes of the values held
	MsTotal                         float32
}

// UsedCodes says which codes of key column col the keys still hold (tad_keydict_mark_codes): used[c] = 1 iff some key, on either side,
// holds value c there.  nValues = the NumValues of the column's StringDict.  into (nil, or nValues bytes of an earlier call) is ORed
// into: columns that share one vocabulary.  The mask crosses in C memory.
func (d *KeyDict) UsedCodes(col int32, nValues uint64, into []byte) (used []byte, nUsed uint64, err error) {
	if !hasStringRetire() {
		return nil, 0, errNoStringRetire
	}
	if into != nil && uint64(len(into)) != nValues {
		return nil, 0, IllegalArgument{"tadengine: UsedCodes: into holds one byte per value"}
	}
	buf := (*C.uint8_t)(C.calloc(C.size_t(nValues)+1, 1))
	if buf == nil {
		return nil, 0, errors.New("tadengine: out of memory")
	}
	defer C.free(unsafe.Pointer(buf))
	acc := C.int32_t(0)
	if into != nil {
		acc = 1
		copy(unsafe.Slice((*byte)(unsafe.Pointer(buf)), nValues), into)
	}
	var n C.uint64_t
	if rc := C.tad_keydict_mark_codes(d.e.h, d.h, C.int32_t(col), acc, buf, C.uint64_t(nValues), C.TAD_MEM_HOST, &n); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(d.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return nil, 0, IllegalArgument{msg}
		}
		return nil, 0, fmt.Errorf("tad_keydict_mark_codes: %s (code %d)", msg, int(rc))
	}
	used = make([]byte, nValues)
	copy(used, unsafe.Slice((*byte)(unsafe.Pointer(buf)), nValues))
	return used, uint64(n), nil
}

// Compact drops the values whose keep byte is 0 and renumbers the survivors densely, order kept (tad_strdict_compact).  len(keep) must
// be NumValues.  remap[c] = the new code of old value c, or CodeNone: pass it to KeyDict.Recode.  Any failure leaves the dictionary as
// it was.  keep and remap cross in C memory.
func (d *StringDict) Compact(keep []byte) (remap []int64, st StrdictCompactStats, err error) {
	if !hasStringRetire() {
		return nil, StrdictCompactStats{}, errNoStringRetire
	}
	n := len(keep)
	kbuf := (*C.uint8_t)(C.calloc(C.size_t(n)+1, 1))
	rbuf := (*C.int64_t)(C.calloc(C.size_t(n)+1, 8))
	defer C.free(unsafe.Pointer(kbuf))
	defer C.free(unsafe.Pointer(rbuf))
	if kbuf == nil || rbuf == nil {
		return nil, StrdictCompactStats{}, errors.New("tadengine: out of memory")
	}
	copy(unsafe.Slice((*byte)(unsafe.Pointer(kbuf)), n), keep)
	var scs C.tad_strdict_compact_stats
	if rc := C.tad_strdict_compact(d.e.h, d.h, kbuf, C.uint64_t(n), C.TAD_MEM_HOST, rbuf, C.TAD_MEM_HOST, &scs); rc != C.TAD_OK {
		return nil, StrdictCompactStats{}, d.fail("tad_strdict_compact", rc)
	}
	remap = make([]int64, n)
	copy(remap, unsafe.Slice((*int64)(unsafe.Pointer(rbuf)), n))
	return remap, StrdictCompactStats{ValuesBefore: uint64(scs.values_before), ValuesAfter: uint64(scs.values_after), BytesBefore: uint64(scs.bytes_before),
		BytesAfter: uint64(scs.bytes_after), ArenaUsedBefore: uint64(scs.arena_used_before), ArenaUsedAfter: uint64(scs.arena_used_after),
		MsTotal: float32(scs.ms_total)}, nil
}

// Recode rewrites key columns through code remaps (tad_keydict_recode): every key's value v in column cols[t] becomes remaps[t][v] —
// what StringDict.Compact returned for the column's vocabulary.  Key ids and sides stay.  A value outside its remap, a value mapped
// to CodeNone, a column named twice or two keys that collide afterwards are an IllegalArgument and leave the dictionary unchanged.
// The remaps and the three arrays that name them cross in C memory.  Returns the keys held.
func (d *KeyDict) Recode(cols []int32, remaps [][]int64) (uint64, error) {
	if !hasStringRetire() {
		return 0, errNoStringRetire
	}
	nt := len(cols)
	if nt != len(remaps) || nt > 8 {
		return 0, IllegalArgument{"tadengine: Recode takes one remap per column, at most 8"}
	}
	colArr := (*[8]C.int32_t)(C.calloc(8, 4))
	ptrArr := (*[8]*C.int64_t)(C.calloc(8, C.size_t(unsafe.Sizeof(unsafe.Pointer(nil)))))
	lenArr := (*[8]C.uint64_t)(C.calloc(8, 8))
	defer C.free(unsafe.Pointer(colArr))
	defer C.free(unsafe.Pointer(ptrArr))
	defer C.free(unsafe.Pointer(lenArr))
	for t := 0; t < nt; t++ {
		colArr[t] = C.int32_t(cols[t])
		lenArr[t] = C.uint64_t(len(remaps[t]))
		ptrArr[t] = (*C.int64_t)(cColumn(remaps[t]))
		defer C.free(unsafe.Pointer(ptrArr[t]))
	}
	var n C.uint64_t
	if rc := C.tad_keydict_recode(d.e.h, d.h, C.int32_t(nt), &colArr[0], &ptrArr[0], &lenArr[0], C.TAD_MEM_HOST, &n); rc != C.TAD_OK {
		msg := C.GoString(C.tad_last_error(d.e.h))
		if rc == C.TAD_ERR_INVALID_ARGUMENT {
			return 0, IllegalArgument{msg}
		}
		return 0, fmt.Errorf("tad_keydict_recode: %s (code %d)", msg, int(rc))
	}
	return uint64(n), nil
}
