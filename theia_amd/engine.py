"""TadEngine — Python host over the C ABI (include/tad.h).  Plumbing only: every number is computed
by the HIP kernels in libtad_mi355x.so; there is no CPU fallback and no import of oracle/.

Columns may be numpy arrays (host memory), torch CUDA tensors or DeviceArray objects (device
memory).  torch is optional here: it is only touched when the caller hands in tensors.
"""
import ctypes as C

import numpy as np

from . import _capi as capi

SYNTH_SEED = 0x7AD05EED


class TadError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("tad error %d: %s" % (code, message))
        self.code = code
        self.message = message


class DeviceArray:
    """n 8-byte elements in HBM, owned by an engine (tad_device_alloc / tad_device_free)."""

    def __init__(self, engine, n, dtype):
        self.engine = engine
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        ptr = C.c_void_p()
        engine._check(engine._lib.tad_device_alloc(engine._h, self.n * self.dtype.itemsize, C.byref(ptr)))
        self.ptr = ptr.value

    @classmethod
    def from_host(cls, engine, array):
        """device copy of an 8-byte numpy array (tad_device_alloc + tad_copy_to_device)"""
        a = np.ascontiguousarray(array)
        d = cls(engine, a.size, a.dtype)
        if a.size:
            engine._check(engine._lib.tad_copy_to_device(engine._h, d.ptr, a.ctypes.data, a.nbytes))
        return d

    _base = None     # a view's owner: the memory is the owner's, which stays alive with the view

    @classmethod
    def view_of(cls, engine, ptr, n, dtype, base):
        """n elements of dtype at device address ptr, inside memory `base` owns (a DeviceArray, a result): nothing is allocated or freed"""
        d = object.__new__(cls)
        d.engine, d.n, d.dtype, d.ptr, d._base = engine, int(n), np.dtype(dtype), ptr, base
        return d

    def view(self, byte_offset, n, dtype):
        """n elements of dtype starting byte_offset bytes into this array (a device slice; shares the memory)"""
        dt = np.dtype(dtype)
        if byte_offset < 0 or byte_offset + int(n) * dt.itemsize > self.n * self.dtype.itemsize:
            raise ValueError("view of %d x %d bytes at %d does not fit %d bytes" % (n, dt.itemsize, byte_offset, self.n * self.dtype.itemsize))
        return DeviceArray.view_of(self.engine, self.ptr + int(byte_offset), n, dt, self)

    def to_host(self):
        out = np.empty(self.n, dtype=self.dtype)
        if self.n:
            self.engine._check(self.engine._lib.tad_copy_to_host(self.engine._h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self._base is None and self.ptr is not None and self.engine._h is not None:
            self.engine._lib.tad_device_free(self.engine._h, self.ptr)
        self.ptr = None
        self._base = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostBuffer:
    """Page-locked host memory owned by an engine (tad_host_alloc): a reader receives an HTTP body straight into `view`, and
    copies from it to the device run at PCIe rate.  Kept and reused by the ingest client between jobs (pinning is slow)."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = int(nbytes)
        ptr = C.c_void_p()
        engine._check(engine._lib.tad_host_alloc(engine._h, self.nbytes, C.byref(ptr)))
        self.ptr = ptr.value
        self.view = memoryview((C.c_ubyte * self.nbytes).from_address(self.ptr)).cast("B")

    def free(self):
        if self.ptr is not None and self.engine._h is not None:
            self.view = None
            self.engine._lib.tad_host_free(self.engine._h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _as_column(x, dtype, n_expected=None, narrow=None):
    """-> (pointer, n, is_device, keepalive).  narrow = "key" / "time": a 4-byte column is passed at its own width (_narrow_of)."""
    if x is None:
        return None, 0, None, None
    if narrow is not None and _narrow_of(x, narrow):
        if hasattr(x, "data_ptr") and hasattr(x, "is_cuda"):
            x = x.contiguous()
            if x.is_cuda:
                return x.data_ptr(), x.numel(), True, x
            x = x.numpy()
        a = np.ascontiguousarray(x).view(np.uint32)     # (a key id as its bits: -1 of an int32 column is TAD_KEY_SKIP32)
        return a.ctypes.data, a.size, False, a
    if isinstance(x, DeviceArray):
        return x.ptr, x.n, True, x
    if hasattr(x, "data_ptr") and hasattr(x, "is_cuda"):  # torch tensor
        if not x.is_contiguous():
            x = x.contiguous()
        if x.element_size() != 8:
            raise TypeError("tensor columns must be 8-byte integers")
        if x.is_cuda:
            return x.data_ptr(), x.numel(), True, x
        x = x.numpy()
    a = np.ascontiguousarray(x)
    if a.dtype != np.dtype(dtype):
        if a.dtype.kind in "iu" and a.dtype.itemsize == 8:
            a = a.view(dtype)
        else:
            a = a.astype(dtype)
    return a.ctypes.data, a.size, False, a


def _narrow_of(x, kind):
    """Whether column x goes to the engine as a narrow (4-byte) column: 4-byte integer key columns (numpy or torch), uint32 numpy
    time columns and 4-byte torch time tensors (an int32 tensor is read as UInt32 DateTime bits).  A numpy int32 time column keeps
    the 8-byte path (sign-extended), as it always had."""
    if x is None or isinstance(x, DeviceArray):
        return False
    if hasattr(x, "data_ptr") and hasattr(x, "is_cuda"):
        return x.element_size() == 4 and not x.is_floating_point() and not x.is_complex()
    dt = getattr(x, "dtype", None)
    if dt is None or not isinstance(x, np.ndarray):
        return False
    if kind == "key":
        return dt.kind in "iu" and dt.itemsize == 4
    return dt == np.dtype(np.uint32)


def _narrow_flags(lib, key_id, key_id2, flow_end_s, flow_start_s):
    """TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32 for these columns; the key (time) columns of a job must all be narrow or all be wide."""
    nk = [_narrow_of(c, "key") for c in (key_id, key_id2) if c is not None]
    nt = [_narrow_of(c, "time") for c in (flow_end_s, flow_start_s) if c is not None]
    if len(set(nk)) > 1 or len(set(nt)) > 1:
        raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "key_id / key_id2 (flow_end_s / flow_start_s) must have the same width")
    flags = (capi.TAD_FLAG_KEY_U32 if nk and nk[0] else 0) | (capi.TAD_FLAG_TIME_U32 if nt and nt[0] else 0)
    if flags and not (getattr(lib, "tad_features", None) and lib.tad_features() & capi.TAD_FEATURE_NARROW_COLUMNS):
        raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "this build of libtad_mi355x.so does not take 4-byte columns (no tad_features / "
                       "TAD_FEATURE_NARROW_COLUMNS): pass 8-byte columns or rebuild the library")
    return flags


class KeyHistogram:
    """tad_factorize_hist's by-product: the key-bin histogram of a batch per Stage-0 workgroup, in HBM.  Hand it to TadEngine.run(key_hist=...)
    with the SAME batch: Stage 0 then sizes pass B's regions from it instead of reading the key column a second time."""

    def __init__(self, engine):
        self.engine = engine
        self.bins = DeviceArray(engine, capi.TAD_KEY_HIST_BYTES // 8, np.uint64)
        self.c = capi.KeyHist(bins=self.bins.ptr)

    @property
    def valid(self):
        return self.c.n_rows != 0

    def free(self):
        self.bins.free()


class PreparedJob:
    """TadEngine.prepare(...): one job over one set of live columns, ready to be submitted any number of times."""

    def __init__(self, engine, job, cols, out_memory, keep):
        self._engine, self._job, self._cols, self._out, self._keep = engine, job, cols, out_memory, keep
        self._jref, self._cref = C.byref(job), C.byref(cols)

    def run(self):
        res = C.POINTER(capi.Result)()
        e = self._engine
        e._check(e._lib.tad_run(e._h, self._jref, self._cref, self._out, C.byref(res)))
        return TadResult(e, res)


class TadResult:
    """Anomalous points ordered by (key_id, flow_end_s) + the run's counters and stage timings."""

    FIELDS = (("key_id", np.uint64), ("flow_end_s", np.int64), ("throughput", np.float64),
              ("algo_calc", np.float64), ("stddev", np.float64))

    def __init__(self, engine, res_ptr):
        self._engine = engine
        self._ptr = res_ptr
        r = res_ptr.contents
        self.n_rows = int(r.n_rows)
        self.memory = "device" if r.memory == capi.TAD_MEM_DEVICE else "host"
        self.id = r.id.decode()
        self.stats = {name: getattr(r.stats, name) for name, _ in capi.Stats._fields_}
        self._host = None
        if self.memory == "host":
            self._host = self._copy_host(r, direct=True)
            self.close()

    def _copy_host(self, r, direct):
        out = {}
        n = self.n_rows
        cols = list(self.FIELDS) + ([("anomaly", np.uint8)] if r.anomaly else [])
        for name, dt in cols:
            arr = np.empty(n, dtype=dt)
            src = getattr(r, name)
            if n:
                if direct:
                    C.memmove(arr.ctypes.data, src, arr.nbytes)
                else:
                    self._engine._check(self._engine._lib.tad_copy_to_host(self._engine._h, arr.ctypes.data, src, arr.nbytes))
            out[name] = arr
        return out

    def device_pointers(self):
        if self._ptr is None or self.memory != "device":
            raise ValueError("no live device result")
        r = self._ptr.contents
        return {name: getattr(r, name) for name, _ in self.FIELDS + (("anomaly", np.uint8),)}

    def to_host(self):
        """dict of numpy arrays: key_id, flow_end_s, throughput, algo_calc, stddev (, anomaly)."""
        if self._host is None:
            self._host = self._copy_host(self._ptr.contents, direct=False)
        return self._host

    def __getitem__(self, name):
        return self.to_host()[name]

    def close(self):
        if self._ptr is not None and self._engine._h is not None:
            self._engine._lib.tad_result_free(self._engine._h, self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TadPoints:
    """Stage-0 output (tad_aggregate): aggregated points ordered by (key_id, flow_end_s), values as raw uint64."""

    FIELDS = (("key_id", np.uint64), ("flow_end_s", np.int64), ("value", np.uint64))

    def __init__(self, engine, ptr):
        self._engine = engine
        self._ptr = ptr
        p = ptr.contents
        self.n_points = int(p.n_points)
        self.memory = "device" if p.memory == capi.TAD_MEM_DEVICE else "host"
        self.stats = {name: getattr(p.stats, name) for name, _ in capi.Stats._fields_}
        self._host = None
        if self.memory == "host":
            self._host = self._copy(direct=True)
            self.close()

    def _copy(self, direct):
        p = self._ptr.contents
        out = {}
        for name, dt in self.FIELDS:
            arr = np.empty(self.n_points, dtype=dt)
            if self.n_points:
                if direct:
                    C.memmove(arr.ctypes.data, getattr(p, name), arr.nbytes)
                else:
                    self._engine._check(self._engine._lib.tad_copy_to_host(self._engine._h, arr.ctypes.data, getattr(p, name), arr.nbytes))
            out[name] = arr
        return out

    def device_pointers(self):
        if self._ptr is None or self.memory != "device":
            raise ValueError("no live device points")
        p = self._ptr.contents
        return {name: getattr(p, name) for name, _ in self.FIELDS}

    def to_host(self):
        if self._host is None:
            self._host = self._copy(direct=False)
        return self._host

    def __getitem__(self, name):
        return self.to_host()[name]

    def close(self):
        if self._ptr is not None and self._engine._h is not None:
            self._engine._lib.tad_points_free(self._engine._h, self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TadDropRows:
    """tad_drop_select's result: seven columns, one row per selected flow row in input order.  Iterates as (endpoint_kind, endpoint_ns,
    endpoint_name, direction, day_s, count, row); each is a numpy array (out="host") or a DeviceArray view into the library's block
    (out="device"), which lives as long as this object or any of the views."""

    FIELDS = (("endpoint_kind", np.int64), ("endpoint_ns", np.int64), ("endpoint_name", np.int64), ("direction", np.int64),
              ("day_s", np.int64), ("count", np.uint64), ("row", np.uint64))

    def __init__(self, engine, ptr):
        self._engine = engine
        self._ptr = ptr
        p = ptr.contents
        self.n_rows = int(p.n_rows)
        self.memory = "device" if p.memory == capi.TAD_MEM_DEVICE else "host"
        self._cols = {}
        for name, dt in self.FIELDS:
            if self.memory == "device":
                self._cols[name] = DeviceArray.view_of(engine, getattr(p, name), self.n_rows, dt, self)
            else:
                arr = np.empty(self.n_rows, dtype=dt)
                if self.n_rows:
                    C.memmove(arr.ctypes.data, getattr(p, name), arr.nbytes)
                self._cols[name] = arr
        if self.memory == "host":
            self.close()

    def __getitem__(self, name):
        return self._cols[name]

    def __iter__(self):
        return iter(self._cols[name] for name, _ in self.FIELDS)

    def __len__(self):
        return len(self.FIELDS)

    def tuple_columns(self):
        """the four key-tuple columns, as factorize / KeyDict.encode take them"""
        return [self._cols[name] for name, _ in self.FIELDS[:4]]

    def to_host(self):
        return {name: (c.to_host() if isinstance(c, DeviceArray) else c) for name, c in self._cols.items()}

    def close(self):
        if self._ptr is not None and self._engine._h is not None:
            self._engine._lib.tad_drop_rows_free(self._engine._h, self._ptr)
        self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TadState:
    """Per-key running state of the streaming detectors (tad_state), resident in HBM.  history=True: the state also keeps every
    aggregated point value it has seen, sorted per key (TAD_STATE_HISTORY), which the streaming DBSCAN detector needs.  series=True:
    it keeps them in time order (TAD_STATE_SERIES), which the streaming ARIMA detector needs.  times=True (with series=True): it keeps
    every series point's flowEndSeconds too (TAD_STATE_TIMES), so that trim() can cut by time."""

    def __init__(self, engine, num_keys, history=False, series=False, times=False):
        self._engine = engine
        self.num_keys = int(num_keys)
        self.history = bool(history)
        self.series = bool(series)
        self.times = bool(times)
        h = C.c_void_p()
        if self.times:
            if not engine._lib.tad_features() & capi.TAD_FEATURE_STREAM_TRIM:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "this build of the library has no state trim (TAD_FEATURE_STREAM_TRIM)")
            flags = (capi.TAD_STATE_HISTORY if self.history else 0) | (capi.TAD_STATE_SERIES if self.series else 0) | capi.TAD_STATE_TIMES
            engine._check(engine._lib.tad_state_create_ex(engine._h, self.num_keys, flags, C.byref(h)))
        elif self.history or self.series:
            if self.history and not engine._lib.tad_features() & capi.TAD_FEATURE_STREAM_DBSCAN:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "this build of the library has no streaming DBSCAN (TAD_FEATURE_STREAM_DBSCAN)")
            if self.series and not engine._lib.tad_features() & capi.TAD_FEATURE_STREAM_ARIMA:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "this build of the library has no streaming ARIMA (TAD_FEATURE_STREAM_ARIMA)")
            flags = (capi.TAD_STATE_HISTORY if self.history else 0) | (capi.TAD_STATE_SERIES if self.series else 0)
            engine._check(engine._lib.tad_state_create_ex(engine._h, self.num_keys, flags, C.byref(h)))
        else:
            engine._check(engine._lib.tad_state_create(engine._h, self.num_keys, C.byref(h)))
        self._h = h

    def history_points(self):
        """values held in the history (tad_state_history_points; 0 for a plain state)"""
        n = capi.u64()
        self._engine._check(self._engine._lib.tad_state_history_points(self._engine._h, self._h, C.byref(n)))
        return int(n.value)

    def export_history(self):
        """(len uint64[num_keys], values uint64[history_points()]): every key's values ascending, keys in order"""
        ln = np.zeros(self.num_keys, np.uint64)
        vals = np.zeros(self.history_points(), np.uint64)
        self._engine._check(self._engine._lib.tad_state_export_history(self._engine._h, self._h, ln.ctypes.data,
                                                                       vals.ctypes.data if vals.size else None))
        return ln, vals

    def load_history(self, len, values):
        """Restore what export_history() returned (tad_state_import_history), after load() of the moments: len[k] must equal n[k]."""
        ln = np.ascontiguousarray(len, dtype=np.uint64)
        vals = np.ascontiguousarray(values, dtype=np.uint64)
        if ln.shape != (self.num_keys,):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "load_history: len has %d entries, the state holds %d keys" % (ln.size, self.num_keys))
        self._engine._check(self._engine._lib.tad_state_import_history(self._engine._h, self._h, ln.ctypes.data,
                                                                       vals.ctypes.data if vals.size else None))

    def series_points(self):
        """values held in the series (tad_state_series_points; 0 for a state without a series)"""
        n = capi.u64()
        self._engine._check(self._engine._lib.tad_state_series_points(self._engine._h, self._h, C.byref(n)))
        return int(n.value)

    def export_series(self):
        """(len uint64[num_keys], values uint64[series_points()]): every key's values in time order, keys in order"""
        ln = np.zeros(self.num_keys, np.uint64)
        vals = np.zeros(self.series_points(), np.uint64)
        self._engine._check(self._engine._lib.tad_state_export_series(self._engine._h, self._h, ln.ctypes.data,
                                                                      vals.ctypes.data if vals.size else None))
        return ln, vals

    def load_series(self, len, values):
        """Restore what export_series() returned (tad_state_import_series), after load() of the moments: len[k] must equal n[k]."""
        ln = np.ascontiguousarray(len, dtype=np.uint64)
        vals = np.ascontiguousarray(values, dtype=np.uint64)
        if ln.shape != (self.num_keys,):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "load_series: len has %d entries, the state holds %d keys" % (ln.size, self.num_keys))
        self._engine._check(self._engine._lib.tad_state_import_series(self._engine._h, self._h, ln.ctypes.data,
                                                                      vals.ctypes.data if vals.size else None))

    def export_times(self):
        """int64[series_points()]: every series point's flowEndSeconds, in the order of export_series() (tad_state_export_times)"""
        t = np.zeros(self.series_points(), np.int64)
        self._engine._check(self._engine._lib.tad_state_export_times(self._engine._h, self._h, t.ctypes.data if t.size else None))
        return t

    def load_times(self, t):
        """Restore what export_times() returned (tad_state_import_times), after load() and load_series(): every key's times must
        ascend strictly and end at its last_t."""
        tt = np.ascontiguousarray(t, dtype=np.int64)
        if tt.shape != (self.series_points(),):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "load_times: %d times, the series holds %d points" % (tt.size, self.series_points()))
        self._engine._check(self._engine._lib.tad_state_import_times(self._engine._h, self._h, tt.ctypes.data if tt.size else None))

    def trim(self, keep_points=0, keep_from=0, alpha=0.0):
        """Drop every key's oldest points (tad_state_trim): keep those with flow_end_s >= keep_from (needs times=True; 0 = no time
        rule), then at most the newest keep_points (0 = no count rule).  The state becomes that of a fresh state streamed only the
        retained points with EWMA parameter alpha (0 -> 0.5).  Returns the number of points dropped."""
        dropped = capi.u64()
        self._engine._check(self._engine._lib.tad_state_trim(self._engine._h, self._h, int(keep_points), int(keep_from), float(alpha),
                                                             C.byref(dropped)))
        return int(dropped.value)

    def rollup(self, before, bucket_s, origin=0, op="sum", alpha=0.0):
        """Fold every key's points older than `before` into time buckets of bucket_s seconds, in place (tad_state_rollup): `before` is
        floored to a bucket start b, the points of one key and bucket below b become one point at the bucket's start (op: "sum" wrapping,
        or "max"), the points at or after b stay.  The state becomes that of a fresh state streamed the folded points with EWMA parameter
        alpha (0 -> 0.5); a key's last_t can move to its last bucket's start.  Returns the fields of tad_rollup_stats as a dict."""
        eng = self._engine
        _need_feature(eng._lib, "STATE_ROLLUP", "tad_state_rollup")
        if op not in ("sum", "max"):
            raise ValueError("op must be 'sum' or 'max'")
        rs = capi.RollupStats()
        eng._check(eng._lib.tad_state_rollup(eng._h, self._h, int(before), int(bucket_s), int(origin), capi.TAD_OP[op], float(alpha), C.byref(rs)))
        return {name: getattr(rs, name) for name, _ in capi.RollupStats._fields_}

    def compact(self, retire_before=0, out="host"):
        """Drop the dead keys and renumber the survivors densely, order kept (tad_state_compact): a key survives iff it has points and,
        with retire_before != 0, its newest point is at or after retire_before.  What a survivor holds is unchanged.  Returns (remap,
        stats): remap[k] = the new id of old key k or TAD_KEY_SKIP — a numpy array, or a DeviceArray with out="device" — and the
        fields of tad_compact_stats as a dict.  num_keys becomes max(survivors, 1)."""
        eng = self._engine
        if not (getattr(eng._lib, "tad_features", None) and eng._lib.tad_features() & capi.TAD_FEATURE_KEY_RETIRE):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "this build of the library has no tad_state_compact (TAD_FEATURE_KEY_RETIRE)")
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device'")
        if out == "device":
            remap = DeviceArray(eng, self.num_keys, np.uint64)
            ptr, mem = remap.ptr, capi.TAD_MEM_DEVICE
        else:
            remap = np.empty(self.num_keys, dtype=np.uint64)
            ptr, mem = remap.ctypes.data, capi.TAD_MEM_HOST
        cs = capi.CompactStats()
        eng._check(eng._lib.tad_state_compact(eng._h, self._h, int(retire_before), ptr, mem, C.byref(cs)))
        self.num_keys = int(cs.num_keys)
        return remap, {name: getattr(cs, name) for name, _ in capi.CompactStats._fields_ if not name.startswith("reserved")}

    def nbytes(self):
        """device bytes the state holds: both moment blocks, the offsets and every arena at its capacity (tad_state_bytes)"""
        n = capi.u64()
        self._engine._check(self._engine._lib.tad_state_bytes(self._engine._h, self._h, C.byref(n)))
        return int(n.value)

    def export(self):
        """dict of numpy arrays: n, avg, m2, ewma, last_t (one entry per key)."""
        K = self.num_keys
        out = {"n": np.zeros(K, np.uint32), "avg": np.zeros(K), "m2": np.zeros(K), "ewma": np.zeros(K), "last_t": np.zeros(K, np.int64)}
        self._engine._check(self._engine._lib.tad_state_export(self._engine._h, self._h, *(out[f].ctypes.data for f in
                                                                                             ("n", "avg", "m2", "ewma", "last_t"))))
        return out

    def resize(self, num_keys):
        """Grow the key space to num_keys (tad_state_resize): the added keys are unseen; fewer keys than now is an error."""
        self._engine._check(self._engine._lib.tad_state_resize(self._engine._h, self._h, int(num_keys)))
        self.num_keys = int(num_keys)

    def load(self, state):
        """Restore what export() returned (tad_state_import): one entry per key of this state; keys with n == 0 are unseen."""
        K = self.num_keys
        cols = []
        for f, dt in (("n", np.uint32), ("avg", np.float64), ("m2", np.float64), ("ewma", np.float64), ("last_t", np.int64)):
            a = np.ascontiguousarray(state[f], dtype=dt)
            if a.shape != (K,):
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "load: %s has %d entries, the state holds %d keys" % (f, a.size, K))
            cols.append(a)
        self._engine._check(self._engine._lib.tad_state_import(self._engine._h, self._h, *(a.ctypes.data for a in cols)))

    def close(self):
        if self._h is not None and self._engine._h is not None:
            self._engine._lib.tad_state_destroy(self._engine._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _key_columns(engine, what, n_cols, cols_a, keep_a, cols_b, keep_b):
    """The tad_key_columns of one batch of key tuples (KeyDict): -> (kc, n, sides, is_device, what must stay alive until the call returns)."""
    if len(cols_a) != n_cols or (cols_b is not None and len(cols_b) != n_cols):
        raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "%s: %d key columns on every side" % (what, n_cols))
    keepalive = []

    def col(x):
        p, n, dev, keep = _as_column(x, np.int64)
        keepalive.append(keep)
        return p, n, dev

    pa = [col(c) for c in cols_a]
    n, dev = pa[0][1], pa[0][2]
    pb = [col(c) for c in cols_b] if cols_b is not None else None
    if any(q[1] != n or q[2] != dev for q in pa + (pb or [])):
        raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "%s: columns must have equal length and live in the same memory" % what)

    def mask(m):
        if m is None:
            return None
        if isinstance(m, DeviceArray):
            return m.ptr
        a = np.ascontiguousarray(np.asarray(m).astype(np.uint8, copy=False))
        if a.size != n:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "%s: mask length" % what)
        if dev:
            d = DeviceArray.from_host(engine, np.frombuffer(a.tobytes() + b"\0" * (-a.size % 8), dtype=np.uint64))
            keepalive.append(d)
            return d.ptr
        keepalive.append(a)
        return a.ctypes.data

    ka, kb = mask(keep_a), mask(keep_b)
    arr_a = (C.c_void_p * n_cols)(*[q[0] for q in pa])
    arr_b = (C.c_void_p * n_cols)(*[q[0] for q in pb]) if pb is not None else None
    kc = capi.KeyColumns(n_rows=n, n_cols=n_cols, cols_a=arr_a, keep_a=ka, cols_b=arr_b, keep_b=kb,
                         memory=capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST)
    keepalive += [arr_a, arr_b]
    return kc, n, 2 if pb is not None else 1, dev, keepalive


def _string_column(column, what):
    """An Arrow string column in any of the forms TadEngine.encode_strings takes -> (tad_string_column, n_rows, is_device, keepalive)"""
    keepalive = []
    validity, voff = None, 0
    if hasattr(column, "combine_chunks") and hasattr(column, "chunks"):     # a pyarrow ChunkedArray: one contiguous column first
        column = column.combine_chunks() if column.num_chunks != 1 else column.chunk(0)
    if hasattr(column, "buffers") and hasattr(column, "type"):        # a pyarrow Array
        import pyarrow as pa
        t = column.type
        if pa.types.is_string(t) or pa.types.is_binary(t):
            bits = 32
        elif pa.types.is_large_string(t) or pa.types.is_large_binary(t):
            bits = 64
        else:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, what + ": not a string / binary column: %s" % t)
        vbuf, obuf, dbuf = column.buffers()
        n, dev = len(column), False
        off_ptr = obuf.address + column.offset * (bits // 8) if obuf is not None else None
        data_ptr, data_bytes = (dbuf.address, dbuf.size) if dbuf is not None else (None, 0)
        if vbuf is not None and column.null_count:
            validity, voff = vbuf.address, column.offset
        keepalive.append(column)
        if n and off_ptr is None:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, what + ": the column has no offsets buffer")
    else:
        offsets, data = column[0], column[1]
        if isinstance(offsets, DeviceArray):
            dev, bits, n = True, offsets.dtype.itemsize * 8, offsets.n - 1
            off_ptr, data_ptr, data_bytes = offsets.ptr, data.ptr, data.n * data.dtype.itemsize
            if len(column) > 2 and column[2] is not None:
                validity, voff = column[2].ptr, int(column[3]) if len(column) > 3 else 0
        else:
            dev = False
            offsets = np.ascontiguousarray(offsets)
            if offsets.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, what + ": offsets must be int32 or int64")
            data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data)
            bits, n = offsets.dtype.itemsize * 8, offsets.size - 1
            off_ptr, data_ptr, data_bytes = offsets.ctypes.data, (data.ctypes.data if data.size else None), data.size
            if len(column) > 2 and column[2] is not None:
                v = np.ascontiguousarray(column[2], dtype=np.uint8)
                keepalive.append(v)
                validity, voff = v.ctypes.data, int(column[3]) if len(column) > 3 else 0
        keepalive += [offsets, data]
    if n < 0:
        raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, what + ": the offsets hold n + 1 entries")
    sc = capi.StringColumn(n_rows=n, offsets=off_ptr, offset_bits=bits, data=data_ptr, data_bytes=data_bytes, validity=validity,
                           validity_offset=voff, memory=capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST)
    return sc, n, dev, keepalive


def _need_feature(lib, feature, what):
    """a library of before `feature` (or of before tad_features) has no `what`: refused before it is touched"""
    if not (getattr(lib, "tad_features", None) and lib.tad_features() & getattr(capi, "TAD_FEATURE_" + feature)):
        raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "this build of the library has no %s (TAD_FEATURE_%s)" % (what, feature))


def _out_array(eng, dev, n, dtype, room=None):
    """-> (array, pointer): a call's output of n values — a DeviceArray (dev) or a numpy array — allocated with room for `room` values"""
    room = n if room is None else room
    if dev:
        a = DeviceArray(eng, room, dtype)
        a.n = n
        return a, a.ptr
    a = np.empty(room, dtype=dtype)
    return a[:n], a.ctypes.data


def _out_mask(eng, dev, K):
    """-> (mask, pointer): K bytes, one per key or value, zeroed on the host or allocated on the device (in 8-byte elements); the pointer
    is None for K == 0"""
    if dev:
        m = DeviceArray(eng, (K + 7) // 8 if K else 1, np.uint64)
        return m, (m.ptr if K else None)
    m = np.zeros(K, np.uint8)
    return m, (m.ctypes.data if K else None)


class KeyDict:
    """A key dictionary that lives in HBM and outlives the call (tad_keydict): key tuples -> dense ids that stay the same from batch to
    batch, new ids in order of first appearance — what the streaming states want for their key ids.  n_cols: the tuple width;
    expected_keys sizes the first table (0 = the default, 1 = the smallest)."""

    def __init__(self, engine, n_cols, expected_keys=0):
        self._engine = engine
        self._h = None
        self.n_cols = int(n_cols)
        _need_feature(engine._lib, "KEY_DICT", "key dictionary")
        h = C.c_void_p()
        engine._check(engine._lib.tad_keydict_create(engine._h, self.n_cols, int(expected_keys), C.byref(h)))
        self._h = h

    def encode(self, cols_a, keep_a=None, cols_b=None, keep_b=None, max_new=None):
        """One batch.  cols_a / keep_a / cols_b / keep_b: as TadEngine.factorize (numpy arrays on the host, or DeviceArrays all on the
        device).  Returns (key_id u64[n], key_id2 u64[n] or None, new_first_row, num_keys_before), in the memory the inputs live in:
        known tuples keep their ids, new ones get num_keys_before, num_keys_before + 1, ... in order of first appearance over the
        virtual rows [side a ++ side b], TAD_KEY_SKIP where the mask is 0; new_first_row[j] = the virtual row of this batch where key
        num_keys_before + j first appears (at most max_new entries; None = all of them)."""
        eng = self._engine
        kc, n, sides, dev, keepalive = _key_columns(eng, "KeyDict.encode", self.n_cols, cols_a, keep_a, cols_b, keep_b)
        cap = int(max_new) if max_new is not None else n * sides
        before, after = capi.u64(), capi.u64()
        key1, p1 = _out_array(eng, dev, n, np.uint64)
        key2, p2 = _out_array(eng, dev, n, np.uint64) if sides == 2 else (None, None)
        first, pf = _out_array(eng, dev, max(cap, 1), np.uint64)
        rc = eng._lib.tad_keydict_encode(eng._h, self._h, C.byref(kc), p1, p2, pf, cap, C.byref(before), C.byref(after))
        del keepalive
        eng._check(rc)
        listed = min(int(after.value - before.value), cap)
        if dev:
            first.n = listed
        else:
            first = first[:listed]
        return key1, key2, first, int(before.value)

    def lookup(self, cols_a, keep_a=None, cols_b=None, keep_b=None):
        """encode() read-only (tad_keydict_lookup): (key_id, key_id2 or None); an unknown tuple gets TAD_KEY_SKIP, the dictionary is unchanged"""
        eng = self._engine
        kc, n, sides, dev, keepalive = _key_columns(eng, "KeyDict.lookup", self.n_cols, cols_a, keep_a, cols_b, keep_b)
        key1, p1 = _out_array(eng, dev, n, np.uint64)
        key2, p2 = _out_array(eng, dev, n, np.uint64) if sides == 2 else (None, None)
        rc = eng._lib.tad_keydict_lookup(eng._h, self._h, C.byref(kc), p1, p2)
        del keepalive
        eng._check(rc)
        return key1, key2

    def select(self, terms=(), side=None, out="device"):
        """A key mask from the dictionary's tuples (tad_keydict_select): keep[k] = 1 iff key k's side is `side` (None = either) and, for
        every term (col, mask), mask[tuple_k[col]] != 0 — TadEngine.mask_rows' rule on the keys instead of on rows.  Up to 8 terms; a
        column may appear in several; each mask is a uint8 array indexed by the column's codes (numpy arrays, or DeviceArrays of bytes
        when out == "device").  Returns (keep, n_selected): keep a DeviceArray of num_keys bytes (out="device": what run_state_keys
        takes without a copy) or a numpy uint8 array (out="host").  A key whose code lies outside a term's mask is refused; the
        dictionary is only read."""
        eng = self._engine
        _need_feature(eng._lib, "KEY_SELECT", "tad_keydict_select")
        if out not in ("device", "host"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.select: out must be device or host")
        terms = list(terms)
        dev = out == "device"
        keepalive, ptrs, lens = [], [], []
        for _, m in terms:
            if isinstance(m, DeviceArray):
                if not dev:
                    raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.select: device masks need out=\"device\"")
                ptrs.append(m.ptr)
                lens.append(m.n * np.dtype(m.dtype).itemsize)
                continue
            a = np.ascontiguousarray(np.asarray(m).astype(np.uint8, copy=False)).reshape(-1)
            if dev and a.size:
                d = DeviceArray.from_host(eng, np.frombuffer(a.tobytes() + b"\0" * (-a.size % 8), dtype=np.uint64))
                keepalive.append(d)
                ptrs.append(d.ptr)
            else:
                keepalive.append(a)
                ptrs.append(a.ctypes.data if a.size else None)
            lens.append(a.size)
        nt = len(terms)
        K = self.num_keys()
        keep, keep_ptr = _out_mask(eng, dev, K)
        n_sel = capi.u64()
        rc = eng._lib.tad_keydict_select(eng._h, self._h, nt, (capi.i32 * max(nt, 1))(*[int(c) for c, _ in terms]),
                                         (C.c_void_p * max(nt, 1))(*ptrs), (capi.u64 * max(nt, 1))(*lens), -1 if side is None else int(side),
                                         keep_ptr, K, capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST, C.byref(n_sel))
        del keepalive
        eng._check(rc)
        if dev:
            keep = keep.view(0, K, np.uint8)
        return keep, int(n_sel.value)

    def num_keys(self):
        """keys held (tad_keydict_num_keys)"""
        n = capi.u64()
        self._engine._check(self._engine._lib.tad_keydict_num_keys(self._engine._h, self._h, C.byref(n)))
        return int(n.value)

    def nbytes(self):
        """device bytes the dictionary holds: the table and the key records at their capacity (tad_keydict_bytes)"""
        n = capi.u64()
        self._engine._check(self._engine._lib.tad_keydict_bytes(self._engine._h, self._h, C.byref(n)))
        return int(n.value)

    def compact(self, remap):
        """Apply the remap of TadState.compact() (tad_keydict_compact): a survivor's tuple now encodes to remap[old id], a retired tuple
        is forgotten (a lookup gives TAD_KEY_SKIP, an encode a new id at the end).  remap: a numpy array or a DeviceArray with one entry
        per key held.  Returns the keys held afterwards."""
        eng = self._engine
        _need_feature(eng._lib, "KEY_RETIRE", "tad_keydict_compact")
        n = capi.u64()
        if isinstance(remap, DeviceArray):
            rc = eng._lib.tad_keydict_compact(eng._h, self._h, remap.ptr, remap.n, capi.TAD_MEM_DEVICE, C.byref(n))
        else:
            a = np.ascontiguousarray(remap, dtype=np.uint64)
            rc = eng._lib.tad_keydict_compact(eng._h, self._h, a.ctypes.data if a.size else None, a.size, capi.TAD_MEM_HOST, C.byref(n))
        eng._check(rc)
        return int(n.value)

    def used_codes(self, col, n_values, into=None, out="device"):
        """Which codes of key column col the keys still hold (tad_keydict_mark_codes): used[c] = 1 iff some key, on either side, holds
        value c in that column.  n_values: the entries of the mask — the num_values() of the column's StringDict; a key whose value
        is not below it is refused.  into: a mask of an earlier call (a numpy uint8 array, or a DeviceArray of n_values bytes) to OR
        into, for columns that share one vocabulary; None = a fresh mask.  Returns (used, n_used): used a DeviceArray of n_values
        bytes (out="device": what StringDict.compact takes without a copy) or a numpy uint8 array (out="host"); with `into`, the memory
        `into` lives in.  The dictionary is only read."""
        eng = self._engine
        _need_feature(eng._lib, "STRING_RETIRE", "tad_keydict_mark_codes")
        if out not in ("device", "host"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.used_codes: out must be device or host")
        K = int(n_values)
        if into is None:
            dev = out == "device"
            used, ptr = _out_mask(eng, dev, K)
        elif isinstance(into, DeviceArray):
            dev, used, ptr = True, into, (into.ptr if K else None)
            if into.n * np.dtype(into.dtype).itemsize < K:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.used_codes: into holds fewer than %d bytes" % K)
        else:
            dev = False
            used = np.ascontiguousarray(into, dtype=np.uint8).reshape(-1)
            if used.size != K:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.used_codes: into holds %d entries, not %d" % (used.size, K))
            ptr = used.ctypes.data if K else None
        n = capi.u64()
        rc = eng._lib.tad_keydict_mark_codes(eng._h, self._h, int(col), 0 if into is None else 1, ptr, K,
                                             capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST, C.byref(n))
        eng._check(rc)
        if dev and into is None:
            used = used.view(0, K, np.uint8)
        return used, int(n.value)

    def recode(self, remaps):
        """Rewrite key columns through code remaps (tad_keydict_recode): remaps = {col: remap}; every key's value v in column col
        becomes remap[v] — what StringDict.compact returned for the column's vocabulary.  The remaps are numpy int64 arrays, or all
        DeviceArrays.  Key ids, sides and the other columns stay.  Refused with the dictionary unchanged: a value outside its remap,
        a value mapped to TAD_CODE_NONE (a key still uses a retired string), two keys whose recoded tuples are equal.  Returns the
        keys held."""
        eng = self._engine
        _need_feature(eng._lib, "STRING_RETIRE", "tad_keydict_recode")
        items = list(remaps.items()) if hasattr(remaps, "items") else list(remaps)
        dev = bool(items) and all(isinstance(r, DeviceArray) for _, r in items)
        if not dev and any(isinstance(r, DeviceArray) for _, r in items):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.recode: the remaps are all numpy arrays or all DeviceArrays")
        keepalive, ptrs, lens = [], [], []
        for _, r in items:
            if dev:
                ptrs.append(r.ptr if r.n else None)
                lens.append(r.n)
            else:
                a = np.ascontiguousarray(r, dtype=np.int64).reshape(-1)
                keepalive.append(a)
                ptrs.append(a.ctypes.data if a.size else None)
                lens.append(a.size)
        nt = len(items)
        n = capi.u64()
        rc = eng._lib.tad_keydict_recode(eng._h, self._h, nt, (capi.i32 * max(nt, 1))(*[int(c) for c, _ in items]), (C.c_void_p * max(nt, 1))(*ptrs),
                                         (capi.u64 * max(nt, 1))(*lens), capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST, C.byref(n))
        del keepalive
        eng._check(rc)
        return int(n.value)

    def export(self, first_key=0, n_keys=None):
        """(cols: list of n_cols int64 arrays, side uint8 array) of the keys [first_key, first_key + n_keys) (tad_keydict_export);
        n_keys None = up to the last key"""
        if n_keys is None:
            n_keys = max(self.num_keys() - int(first_key), 0)
        cols = [np.zeros(int(n_keys), np.int64) for _ in range(self.n_cols)]
        side = np.zeros(int(n_keys), np.uint8)
        ptrs = (C.c_void_p * self.n_cols)(*[c.ctypes.data for c in cols])
        self._engine._check(self._engine._lib.tad_keydict_export(self._engine._h, self._h, int(first_key), int(n_keys), ptrs, side.ctypes.data))
        return cols, side

    def gather(self, key_id, cols=None, out="host"):
        """The tuples of arbitrary keys (tad_keydict_gather): key_id a numpy array or a DeviceArray of uint64 ids, in any order and with
        repeats; cols the tuple columns wanted (None = all of them).  Returns (columns, side): columns a list of int64 arrays, one per
        entry of cols, with column c of key key_id[i] at i, and side a uint8 array (0 = side a, 1 = side b) — numpy arrays
        (out="host") or DeviceArrays (out="device": what StringDict.decode takes without a copy).  The call runs on the device arrays
        when key_id or the outputs live there.  An id that is not below num_keys() is refused."""
        eng = self._engine
        _need_feature(eng._lib, "DICT_DECODE", "tad_keydict_gather")
        if out not in ("host", "device"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.gather: out must be host or device")
        want = list(range(self.n_cols)) if cols is None else [int(c) for c in cols]
        if any(c < 0 or c >= self.n_cols for c in want) or len(set(want)) != len(want):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.gather: cols names each of the %d key columns at most once" % self.n_cols)
        ids = key_id
        if not isinstance(ids, DeviceArray):
            ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
            if out == "device":
                n_ids = ids.size
                ids = DeviceArray.from_host(eng, ids if n_ids else np.zeros(1, np.uint64))
                ids.n = n_ids
        dev = isinstance(ids, DeviceArray)
        n = ids.n if dev else ids.size
        outs = {c: _out_array(eng, dev, n, np.int64, room=max(n, 1)) for c in want}
        if dev:
            side = DeviceArray(eng, (n + 7) // 8 if n else 1, np.uint64)
            side_ptr = side.ptr
        else:
            side = np.zeros(n, np.uint8)
            side_ptr = side.ctypes.data if n else None
        ptrs = (C.c_void_p * self.n_cols)(*[outs[c][1] if c in outs else None for c in range(self.n_cols)])
        rc = eng._lib.tad_keydict_gather(eng._h, self._h, (ids.ptr if dev else (ids.ctypes.data if n else None)), n,
                                         capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST, ptrs, side_ptr)
        eng._check(rc)
        columns = [outs[c][0] for c in want]
        if dev:
            side = side.view(0, n, np.uint8)
            if out == "host":
                columns = [c.to_host() for c in columns]
                side = side.to_host()
        return columns, side

    def load(self, cols, side=None):
        """Fill this EMPTY dictionary so that key i is tuple i (tad_keydict_import): what export() returned, after a restart.
        side None = every key on side 0."""
        if len(cols) != self.n_cols:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.load: %d key columns" % self.n_cols)
        arrs = [np.ascontiguousarray(c, dtype=np.int64) for c in cols]
        n = arrs[0].size
        sd = np.ascontiguousarray(side, dtype=np.uint8) if side is not None else None
        if any(a.shape != (n,) for a in arrs) or (sd is not None and sd.shape != (n,)):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "KeyDict.load: columns and side must have equal length")
        ptrs = (C.c_void_p * self.n_cols)(*[a.ctypes.data for a in arrs])
        self._engine._check(self._engine._lib.tad_keydict_import(self._engine._h, self._h, n, ptrs, sd.ctypes.data if sd is not None else None))

    def close(self):
        if self._h is not None and self._engine._h is not None:
            self._engine._lib.tad_keydict_destroy(self._engine._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StringDict:
    """A string dictionary that lives in HBM and outlives the call (tad_strdict): the strings of an Arrow column -> codes that stay the
    same from batch to batch, new codes in order of first appearance — the stable vocabulary a KeyDict wants for a string key column.
    expected_values sizes the first table, expected_bytes the first arena (0 = the defaults, 1 = the smallest)."""

    def __init__(self, engine, expected_values=0, expected_bytes=0):
        self._engine = engine
        self._h = None
        _need_feature(engine._lib, "STRING_DICT", "string dictionary")
        h = C.c_void_p()
        engine._check(engine._lib.tad_strdict_create(engine._h, int(expected_values), int(expected_bytes), C.byref(h)))
        self._h = h

    def _out(self, out, x):
        """x (a numpy array or a DeviceArray: the call's result, in the memory the column lives in) in the memory `out` names"""
        if out == "device":
            return x if isinstance(x, DeviceArray) else DeviceArray.from_host(self._engine, x)
        return x.to_host() if isinstance(x, DeviceArray) else x

    def encode(self, column, out="host", max_new=None):
        """One batch.  column: every form TadEngine.encode_strings takes (a pyarrow string / binary array, or (offsets, data[, validity,
        validity_offset]) as numpy arrays or DeviceArrays; a null encodes like "").  The call runs in the memory the column lives in; the
        results are handed over in the memory `out` names ("host": numpy arrays, "device": DeviceArrays).  Returns (codes int64[n], new_first_row, num_before): a string the dictionary holds keeps its code, new
        strings get num_before, num_before + 1, ... in order of first appearance; new_first_row[j] = the row of this batch where value
        num_before + j first appears (at most max_new entries; None = all of them)."""
        eng = self._engine
        if out not in ("host", "device"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "StringDict.encode: out must be host or device")
        sc, n, dev, keepalive = _string_column(column, "StringDict.encode")
        cap = int(max_new) if max_new is not None else n
        before, after = capi.u64(), capi.u64()
        codes, pc = _out_array(eng, dev, n, np.int64, room=max(n, 1))
        first, pf = _out_array(eng, dev, max(cap, 1), np.uint64)
        rc = eng._lib.tad_strdict_encode(eng._h, self._h, C.byref(sc), pc, pf, cap, C.byref(before), C.byref(after))
        del keepalive
        eng._check(rc)
        listed = min(int(after.value - before.value), cap)
        if dev:
            first.n = listed
        else:
            first = first[:listed]
        return self._out(out, codes), self._out(out, first), int(before.value)

    def lookup(self, column, out="host"):
        """encode() read-only (tad_strdict_lookup): codes; an unknown string gets TAD_CODE_NONE (-1), the dictionary is unchanged"""
        eng = self._engine
        if out not in ("host", "device"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "StringDict.lookup: out must be host or device")
        sc, n, dev, keepalive = _string_column(column, "StringDict.lookup")
        codes, pc = _out_array(eng, dev, n, np.int64, room=max(n, 1))
        rc = eng._lib.tad_strdict_lookup(eng._h, self._h, C.byref(sc), pc)
        del keepalive
        eng._check(rc)
        return self._out(out, codes)

    def num_values(self):
        """values held (tad_strdict_num_values)"""
        n = capi.u64()
        self._engine._check(self._engine._lib.tad_strdict_num_values(self._engine._h, self._h, C.byref(n)))
        return int(n.value)

    def nbytes(self):
        """device bytes the dictionary holds: table, records and arena at their capacity (tad_strdict_bytes)"""
        n = capi.u64()
        self._engine._check(self._engine._lib.tad_strdict_bytes(self._engine._h, self._h, C.byref(n)))
        return int(n.value)

    def compact(self, keep, out="host"):
        """Drop values and renumber the survivors densely, order kept (tad_strdict_compact): value c survives iff keep[c] != 0.  keep: a
        numpy array, or a DeviceArray of num_values() bytes (what KeyDict.used_codes returns).  Returns (remap, stats): remap[c] = the
        new code of old value c or TAD_CODE_NONE (-1) — a numpy int64 array, or a DeviceArray with out="device" (what KeyDict.recode
        takes without a copy) — and the fields of tad_strdict_compact_stats as a dict.  Afterwards the dictionary is what a fresh one
        holds after load() of the survivors; any failure leaves it as it was."""
        eng = self._engine
        _need_feature(eng._lib, "STRING_RETIRE", "tad_strdict_compact")
        if out not in ("host", "device"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "StringDict.compact: out must be host or device")
        if isinstance(keep, DeviceArray):
            K = keep.n * np.dtype(keep.dtype).itemsize
            kptr, kmem = (keep.ptr if K else None), capi.TAD_MEM_DEVICE
        else:
            keep = np.asarray(keep)
            if keep.dtype != np.uint8:                 # survives iff keep[c] != 0, whatever the type: 256 and 0.5 keep their value
                keep = keep != 0
            keep = np.ascontiguousarray(keep.astype(np.uint8, copy=False)).reshape(-1)
            K = keep.size
            kptr, kmem = (keep.ctypes.data if K else None), capi.TAD_MEM_HOST
        remap, rptr = _out_array(eng, out == "device", K, np.int64, room=max(K, 1))
        cs = capi.StrdictCompactStats()
        rc = eng._lib.tad_strdict_compact(eng._h, self._h, kptr, K, kmem, rptr, capi.TAD_MEM_DEVICE if out == "device" else capi.TAD_MEM_HOST, C.byref(cs))
        eng._check(rc)
        return remap, {name: getattr(cs, name) for name, _ in capi.StrdictCompactStats._fields_ if not name.startswith("reserved")}

    def export(self, first=0, n=None):
        """(offsets int64[n + 1], data uint8[...]) of the values [first, first + n) in Arrow's layout (tad_strdict_export); n None = up
        to the last value"""
        eng = self._engine
        if n is None:
            n = max(self.num_values() - int(first), 0)
        need = capi.u64()
        eng._check(eng._lib.tad_strdict_export(eng._h, self._h, int(first), int(n), None, None, 0, C.byref(need)))
        offsets = np.zeros(int(n) + 1, dtype=np.int64)
        data = np.zeros(int(need.value), dtype=np.uint8)
        eng._check(eng._lib.tad_strdict_export(eng._h, self._h, int(first), int(n), offsets.ctypes.data, data.ctypes.data if data.size else None, data.size,
                                               C.byref(need)))
        return offsets, data

    def values(self, first=0, n=None):
        """the values [first, first + n) as a pyarrow large_string array (n None = up to the last value): the strings the host needs for
        decoding result rows"""
        import pyarrow as pa
        offsets, data = self.export(first, n)
        return pa.Array.from_buffers(pa.large_string(), offsets.size - 1, [None, pa.py_buffer(offsets), pa.py_buffer(data)])

    def decode(self, codes, out="host"):
        """The strings of arbitrary codes in Arrow's layout (tad_strdict_decode): codes a numpy array or a DeviceArray of int64 (what
        KeyDict.gather returns for a string key column), in any order and with repeats.  Returns (offsets int64[n + 1], data uint8[...]):
        the bytes of value codes[i] are data[offsets[i]:offsets[i + 1]] — numpy arrays (out="host") or DeviceArrays (out="device"),
        wherever the codes live.  A code that is not in [0, num_values()) is refused: TAD_CODE_NONE decodes to nothing."""
        eng = self._engine
        _need_feature(eng._lib, "DICT_DECODE", "tad_strdict_decode")
        if out not in ("host", "device"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "StringDict.decode: out must be host or device")
        dev_in = isinstance(codes, DeviceArray)
        if not dev_in:
            codes = np.ascontiguousarray(codes, dtype=np.int64).reshape(-1)
        n = codes.n if dev_in else codes.size
        cptr = codes.ptr if dev_in else (codes.ctypes.data if n else None)
        cmem = capi.TAD_MEM_DEVICE if dev_in else capi.TAD_MEM_HOST
        need = capi.u64()
        eng._check(eng._lib.tad_strdict_decode(eng._h, self._h, cptr, n, cmem, None, None, 0, capi.TAD_MEM_HOST, C.byref(need)))
        total = int(need.value)
        if out == "device":
            offsets = DeviceArray(eng, n + 1, np.int64)
            room = DeviceArray(eng, max((total + 7) // 8, 1), np.uint64)
            data, optr, dptr, omem = room.view(0, total, np.uint8), offsets.ptr, room.ptr, capi.TAD_MEM_DEVICE
        else:
            offsets = np.zeros(n + 1, dtype=np.int64)
            data = np.zeros(total, dtype=np.uint8)
            optr, dptr, omem = offsets.ctypes.data, (data.ctypes.data if total else None), capi.TAD_MEM_HOST
        eng._check(eng._lib.tad_strdict_decode(eng._h, self._h, cptr, n, cmem, optr, dptr if total else None, total, omem, C.byref(need)))
        return offsets, data

    def take(self, codes):
        """the values of arbitrary codes as a pyarrow large_string array (decode on the host side of the link): values() for the codes a
        result names, not for the whole vocabulary"""
        offsets, data = self.decode(codes, out="host")
        import pyarrow as pa
        return pa.Array.from_buffers(pa.large_string(), offsets.size - 1, [None, pa.py_buffer(offsets), pa.py_buffer(data)])

    def load(self, values):
        """Fill this EMPTY dictionary so that value i is string i (tad_strdict_import): what values() / export() returned, after a
        restart.  values: a pyarrow string array, a sequence of str / bytes, or (offsets, data) as export() returns them.  Two equal
        strings, or a dictionary that already holds values, are refused and nothing changes."""
        eng = self._engine
        if isinstance(values, tuple) and len(values) == 2 and hasattr(values[0], "dtype"):
            offsets, data = np.ascontiguousarray(values[0], dtype=np.int64), np.ascontiguousarray(values[1], dtype=np.uint8)
        else:
            if hasattr(values, "to_pylist"):
                values = values.to_pylist()
            raw = [v if isinstance(v, (bytes, bytearray)) else ("" if v is None else str(v)).encode("utf-8") for v in values]
            offsets = np.zeros(len(raw) + 1, dtype=np.int64)
            np.cumsum([len(r) for r in raw], out=offsets[1:])
            data = np.frombuffer(b"".join(raw), dtype=np.uint8)
        n = offsets.size - 1
        eng._check(eng._lib.tad_strdict_import(eng._h, self._h, n, offsets.ctypes.data if n else None, data.ctypes.data if data.size else None))

    def match(self, op, pattern, out="host"):
        """One byte per value (tad_strdict_match): mask[c] = 1 iff value c satisfies op with the pattern — capi.TAD_STR_EQUAL (the same
        bytes) or capi.TAD_STR_CONTAINS_NOCASE (the pattern occurs in the value; 'A'..'Z' fold to 'a'..'z', every other byte matches
        only itself).  pattern: str (UTF-8) or bytes, at most 1024 bytes.  Returns (mask, n_matched): mask a numpy uint8 array
        (out="host") or a DeviceArray of num_values bytes (out="device": what KeyDict.select and TadEngine.mask_rows take)."""
        eng = self._engine
        if out not in ("host", "device"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "StringDict.match: out must be host or device")
        pat = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
        buf = (C.c_ubyte * max(len(pat), 1)).from_buffer_copy(pat or b"\0")
        K = self.num_values()
        dev = out == "device"
        mask, ptr = _out_mask(eng, dev, K)
        hit = capi.u64()
        rc = eng._lib.tad_strdict_match(eng._h, self._h, int(op), C.cast(buf, C.c_void_p) if pat else None, len(pat), ptr, K,
                                        capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST, C.byref(hit))
        eng._check(rc)
        if dev:
            mask = mask.view(0, K, np.uint8)
        return mask, int(hit.value)

    def like(self, pattern, nocase=False, out="host"):
        """One byte per value (tad_strdict_like): mask[c] = 1 iff the LIKE pattern matches the WHOLE of value c.  % matches any run of
        bytes, _ exactly one character, \\ makes the next byte a literal; a substring search is '%text%'.  nocase: ilike — 'A'..'Z'
        fold to 'a'..'z', every other byte matches only itself.  pattern: str (UTF-8) or bytes, at most 1024 bytes.  Returns
        (mask, n_matched) as match() does: a numpy uint8 array (out="host") or a DeviceArray of num_values bytes (out="device")."""
        eng = self._engine
        _need_feature(eng._lib, "STRING_LIKE", "tad_strdict_like")
        if out not in ("host", "device"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "StringDict.like: out must be host or device")
        pat = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
        buf = (C.c_ubyte * max(len(pat), 1)).from_buffer_copy(pat or b"\0")
        K = self.num_values()
        dev = out == "device"
        mask, ptr = _out_mask(eng, dev, K)
        hit = capi.u64()
        rc = eng._lib.tad_strdict_like(eng._h, self._h, C.cast(buf, C.c_void_p) if pat else None, len(pat), capi.TAD_LIKE_NOCASE if nocase else 0, ptr, K,
                                       capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST, C.byref(hit))
        eng._check(rc)
        if dev:
            mask = mask.view(0, K, np.uint8)
        return mask, int(hit.value)

    def close(self):
        if self._h is not None and self._engine._h is not None:
            self._engine._lib.tad_strdict_destroy(self._engine._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TadEngine:
    """One engine per GPU.  Thread-safe: up to max_jobs_in_flight jobs (0 = the library's default, 4) run concurrently, each on its own
    job context (HIP stream + workspace) inside the library; further callers wait."""

    def __init__(self, device=0, stream=None, workspace_limit=0, plan=None, library_path=None, max_jobs_in_flight=0):
        """plan: dict of tad_plan overrides (include/tad.h), e.g. {"stage0": "v2", "partition_pass": "sort"}; None = the
        engine decides everything (production).  library_path: another build of the library (A/B measurements, tools/ab_plans.py)."""
        self._lib = capi.load_library(path=library_path)
        self._h = None
        self.device = int(device)
        self._plan = dict(plan or {})
        opts = capi.EngineOpts(device=int(device), stream=C.c_void_p(stream) if stream else None,
                               workspace_limit=int(workspace_limit), plan=capi.make_plan(**self._plan),
                               max_jobs_in_flight=int(max_jobs_in_flight))
        h = C.c_void_p()
        rc = self._lib.tad_engine_create(C.byref(opts), C.byref(h))
        if rc != capi.TAD_OK:
            raise TadError(rc, (self._lib.tad_last_error(None) or b"").decode())
        self._h = h

    # ---- plumbing ----
    def _check(self, rc):
        if rc != capi.TAD_OK:
            raise TadError(rc, (self._lib.tad_last_error(self._h) or b"").decode())

    def set_plan(self, **overrides):
        """Replace the engine's plan overrides (tad_engine_set_plan); no arguments = back to automatic."""
        p = capi.make_plan(**overrides)
        self._check(self._lib.tad_engine_set_plan(self._h, C.byref(p)))
        self._plan = dict(overrides)

    def plan(self, **overrides):
        """Context manager: the jobs inside run with these overrides ON TOP of the current ones, which are restored after."""
        engine = self

        class _Scope:
            def __enter__(self_inner):
                self_inner.saved = dict(engine._plan)
                merged = dict(engine._plan)
                merged.update(overrides)
                engine.set_plan(**merged)
                return engine

            def __exit__(self_inner, *exc):
                engine.set_plan(**self_inner.saved)
                return False
        return _Scope()

    def close(self):
        if self._h is not None:
            self._lib.tad_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def progress(self):
        d, t = capi.i32(), capi.i32()
        self._lib.tad_progress(self._h, C.byref(d), C.byref(t))
        return d.value, t.value

    def job_progress(self, job_id):
        """(done, total) of the job in flight whose id is job_id; (0, 0) when there is none"""
        d, t = capi.i32(), capi.i32()
        self._lib.tad_job_progress(self._h, job_id.encode()[:63], C.byref(d), C.byref(t))
        return d.value, t.value

    def jobs_in_flight(self):
        return int(self._lib.tad_jobs_in_flight(self._h))

    # ---- the job (anomaly_detection.py:647-710) ----
    def run(self, algo, key_id, flow_end_s, value, num_keys, agg_flow="", value_op="auto", key_id2=None,
            flow_start_s=None, start_time=0, end_time=0, lattice=None, emit_all=False, out="host", job_id="",
            alpha=0.0, eps=0.0, min_samples=0, maxiter=0, drop_nsigma=0.0, drop_min_samples=0, key_hist=None, _prepare_only=False):
        if algo not in capi.TAD_ALGO:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "algo must be EWMA, ARIMA, DBSCAN or DROP")
        if agg_flow not in capi.TAD_AGG:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "agg_flow must be '', pod, svc or external")
        narrow = _narrow_flags(self._lib, key_id, key_id2, flow_end_s, flow_start_s)
        pk, n, dev, keep1 = _as_column(key_id, np.uint64, narrow="key")
        pt, nt, dev_t, keep2 = _as_column(flow_end_s, np.int64, narrow="time")
        pv, nv, dev_v, keep3 = _as_column(value, np.uint64)
        pk2, nk2, dev_k2, keep4 = _as_column(key_id2, np.uint64, narrow="key")
        ps, ns, dev_s, keep5 = _as_column(flow_start_s, np.int64, narrow="time")
        for m, d in ((nt, dev_t), (nv, dev_v)) + (((nk2, dev_k2),) if key_id2 is not None else ()) + \
                (((ns, dev_s),) if flow_start_s is not None else ()):
            if m != n or d != dev:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "columns must have equal length and live in the same memory")
        job = capi.Job(algo=capi.TAD_ALGO[algo], agg_flow=capi.TAD_AGG[agg_flow], value_op=capi.TAD_OP[value_op],
                       start_time=int(start_time), end_time=int(end_time), ewma_alpha=float(alpha),
                       dbscan_eps=float(eps), dbscan_min_samples=int(min_samples), arima_maxiter=int(maxiter),
                       drop_nsigma=float(drop_nsigma), drop_min_samples=int(drop_min_samples),
                       flags=(capi.TAD_FLAG_EMIT_ALL_POINTS if emit_all else 0) | narrow, id=job_id.encode()[:63])
        cols = capi.Columns(n_rows=n, key_id=pk, key_id2=pk2, flow_end_s=pt, flow_start_s=ps, value=pv,
                            num_keys=int(num_keys), memory=capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST)
        if lattice is not None:
            cols.t0, cols.step, cols.n_buckets = int(lattice[0]), int(lattice[1]), int(lattice[2])
        if key_hist is not None and key_hist.valid:
            cols.key_hist = C.pointer(key_hist.c)
        if _prepare_only:
            return PreparedJob(self, job, cols, capi.TAD_MEM_DEVICE if out == "device" else capi.TAD_MEM_HOST,
                               (keep1, keep2, keep3, keep4, keep5, key_hist))
        res = C.POINTER(capi.Result)()
        rc = self._lib.tad_run(self._h, C.byref(job), C.byref(cols),
                               capi.TAD_MEM_DEVICE if out == "device" else capi.TAD_MEM_HOST, C.byref(res))
        del keep1, keep2, keep3, keep4, keep5
        self._check(rc)
        return TadResult(self, res)

    def prepare(self, *args, **kw):
        """Same arguments as run(): the tad_job / tad_columns structs built ONCE, for a host that submits the same job over the
        same (live) columns repeatedly — PreparedJob.run() is then the bare tad_run call (a cgo host pays no more either; building
        the two structs and inspecting five column objects in Python costs ~15 us per call, 1 % of a C2 job)."""
        return self.run(*args, _prepare_only=True, **kw)

    # ---- streaming EWMA / DBSCAN: one new batch against the per-key running state ----
    def state_create(self, num_keys, history=False, series=False, times=False):
        """history=True: a state for streaming DBSCAN too (tad_state_create_ex with TAD_STATE_HISTORY); series=True: for streaming
        ARIMA too (TAD_STATE_SERIES); times=True (with series=True): the series keeps its points' times, for TadState.trim by time
        (TAD_STATE_TIMES)"""
        return TadState(self, num_keys, history=history, series=series, times=times)

    def _stream_columns(self, state, key_id, flow_end_s, value, key_id2, num_keys, lattice):
        """The tad_columns of one batch on `state` (run_stream, merge_stream): narrow columns, device arrays, the second key column of pod
        mode.  Returns (cols, narrow flags, what must stay alive until the call returns)."""
        narrow = _narrow_flags(self._lib, key_id, key_id2, flow_end_s, None)
        pk, n, dev, keep1 = _as_column(key_id, np.uint64, narrow="key")
        pt, nt, dev_t, keep2 = _as_column(flow_end_s, np.int64, narrow="time")
        pv, nv, dev_v, keep3 = _as_column(value, np.uint64)
        pk2, nk2, dev_k2, keep4 = _as_column(key_id2, np.uint64, narrow="key")
        if nt != n or nv != n or dev_t != dev or dev_v != dev or (key_id2 is not None and (nk2 != n or dev_k2 != dev)):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "columns must have equal length and live in the same memory")
        cols = capi.Columns(n_rows=n, key_id=pk, key_id2=pk2, flow_end_s=pt, value=pv, num_keys=state.num_keys if num_keys is None else int(num_keys),
                            memory=capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST)
        if lattice is not None:
            cols.t0, cols.step, cols.n_buckets = int(lattice[0]), int(lattice[1]), int(lattice[2])
        return cols, narrow, (keep1, keep2, keep3, keep4)

    # ---- what the jobs on a state share: the feature gate, the detector's tad_job, the out memory, the call itself ----
    def _need(self, feature, what):
        _need_feature(self._lib, feature, what)

    @staticmethod
    def _detector_job(algo, alpha=0.0, eps=0.0, min_samples=0, maxiter=0, nsigma=0.0, emit_all=False, job_id="", agg_flow="", value_op="auto"):
        """the tad_job of a detector on a state; min_samples is DROP's drop_min_samples, else dbscan_min_samples"""
        if algo not in capi.TAD_ALGO:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "algo must be EWMA, ARIMA, DBSCAN or DROP")
        drop = algo == "DROP"
        return capi.Job(algo=capi.TAD_ALGO[algo], agg_flow=capi.TAD_AGG[agg_flow], value_op=capi.TAD_OP[value_op], ewma_alpha=float(alpha),
                        dbscan_eps=float(eps), dbscan_min_samples=0 if drop else int(min_samples), arima_maxiter=int(maxiter),
                        drop_nsigma=float(nsigma), drop_min_samples=int(min_samples) if drop else 0,
                        flags=capi.TAD_FLAG_EMIT_ALL_POINTS if emit_all else 0, id=job_id.encode()[:63])

    @staticmethod
    def _out_mem(out):
        return capi.TAD_MEM_DEVICE if out == "device" else capi.TAD_MEM_HOST

    def _state_rows(self, call, state, job, out, *args):
        """lib.<call>(engine, state, job, *args, out memory, &result) -> TadResult; the caller keeps alive what args point to"""
        res = C.POINTER(capi.Result)()
        self._check(getattr(self._lib, call)(self._h, state._h, C.byref(job), *args, self._out_mem(out), C.byref(res)))
        return TadResult(self, res)

    def run_stream(self, state, key_id, flow_end_s, value, agg_flow="", value_op="auto", lattice=None, emit_all=False, out="host",
                   alpha=0.0, job_id="", num_keys=None, key_id2=None, algo="EWMA", eps=0.0, min_samples=0, maxiter=0):
        """One batch of a streaming detector on `state` (tad_run_stream).  key_id2: the second key column of pod mode.  algo="DBSCAN"
        needs a state with history, algo="ARIMA" (maxiter: arima_maxiter) a state with a series: the rows are those tad_run emits for
        this batch's points over everything seen so far."""
        job = self._detector_job(algo, alpha, eps, min_samples, maxiter, emit_all=emit_all, job_id=job_id, agg_flow=agg_flow, value_op=value_op)
        cols, narrow, keep = self._stream_columns(state, key_id, flow_end_s, value, key_id2, num_keys, lattice)
        job.flags |= narrow
        return self._state_rows("tad_run_stream", state, job, out, C.byref(cols))

    def _changes(self, state, changes):
        """-> (tad_changes or None, its key_since array or None) for changes in (None, "host", "device", "counters")"""
        if changes is None:
            return None, None
        if changes not in ("host", "device", "counters"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "changes must be None, 'host', 'device' or 'counters'")
        self._need("STATE_ALERTS", "tad_state_merge_changes / tad_state_replace_changes")
        if changes == "counters":
            return capi.Changes(key_since=None, len=0, memory=capi.TAD_MEM_HOST), None
        arr, ptr = _out_array(self, changes == "device", state.num_keys, np.int64)
        return capi.Changes(key_since=ptr, len=state.num_keys, memory=self._out_mem(changes)), arr

    @staticmethod
    def _with_changes(stats, ch, arr):
        """the stats dict of a merge or a replace, carrying the change report when one was asked for"""
        if ch is not None:
            stats.update(key_since=arr, keys_changed=ch.keys_changed, points_changed=ch.points_changed, min_t=ch.min_t, max_t=ch.max_t)
        return stats

    def merge_stream(self, state, key_id, flow_end_s, value, agg_flow="", value_op="auto", lattice=None, alpha=0.0, keep_from=0, job_id="",
                     num_keys=None, key_id2=None):
        """One batch placed BY TIME into `state` (tad_state_merge): late rows, re-sent rows, rows of a (key, flowEndSeconds) group split
        over batches.  Afterwards the state is the one a fresh state holds after one run_stream EWMA batch over its window's points plus
        this batch (without the points older than keep_from, when that is not 0).  Needs a state with series=True and times=True; use
        the same value_op for every batch of a state.  No rows: ask run_state for the window's verdicts.  Returns the call's
        tad_merge_stats as a dict.  merge_stream_changes is this call with a report of what it changed."""
        return self._merge(state, key_id, flow_end_s, value, agg_flow, value_op, lattice, alpha, keep_from, job_id, num_keys, key_id2, None)

    def merge_stream_changes(self, state, key_id, flow_end_s, value, changes="host", **kw):
        """merge_stream (whose other arguments go through **kw) with the change report (tad_state_merge_changes): the returned dict also
        carries key_since — one int64 per key of the state, a numpy array (changes="host") or a DeviceArray ("device"): the smallest
        flowEndSeconds at which the key's series changed, capi.TAD_NO_CHANGE where it did not — and keys_changed, points_changed, min_t,
        max_t; changes="counters": those four alone (key_since None).  A point is changed when it was added, or combined into another
        value: a sum of 0 and a maximum not above the held value change nothing."""
        if changes is None:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "changes must be 'host', 'device' or 'counters'")
        return self._merge(state, key_id, flow_end_s, value, changes=changes, **kw)

    def _merge(self, state, key_id, flow_end_s, value, agg_flow="", value_op="auto", lattice=None, alpha=0.0, keep_from=0, job_id="",
               num_keys=None, key_id2=None, changes=None):
        if not self._lib.tad_features() & capi.TAD_FEATURE_STATE_MERGE:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "this build of the library has no tad_state_merge (TAD_FEATURE_STATE_MERGE)")
        cols, narrow, keep = self._stream_columns(state, key_id, flow_end_s, value, key_id2, num_keys, lattice)
        job = capi.Job(algo=capi.TAD_ALGO["EWMA"], agg_flow=capi.TAD_AGG[agg_flow], value_op=capi.TAD_OP[value_op], ewma_alpha=float(alpha),
                       flags=narrow, id=job_id.encode()[:63])
        stats = capi.MergeStats()
        ch, arr = self._changes(state, changes)
        if ch is None:
            rc = self._lib.tad_state_merge(self._h, state._h, C.byref(job), C.byref(cols), int(keep_from), C.byref(stats))
        else:
            rc = self._lib.tad_state_merge_changes(self._h, state._h, C.byref(job), C.byref(cols), int(keep_from), C.byref(stats), C.byref(ch))
        del keep
        self._check(rc)
        return self._with_changes({name: getattr(stats, name) for name, _ in capi.MergeStats._fields_ if not name.startswith("reserved")}, ch, arr)

    def replace_stream(self, state, key_id, flow_end_s, value, from_t=0, to_t=0, ranged=False, agg_flow="", value_op="auto", lattice=None,
                       alpha=0.0, keep_from=0, job_id="", num_keys=None, key_id2=None):
        """One batch that REPLACES what `state` holds (tad_state_replace): a point at a time its key already holds takes the batch's
        value instead of being combined with it, so a re-read of the same rows leaves the same state under sum as under max.
        ranged=True: the batch is ALL rows with from_t <= flowEndSeconds < to_t (0 = no bound on that side), and every point of the
        state inside that range that the batch does not name is erased, on every key; an empty batch then still erases the range.
        The other arguments are merge_stream's.  Returns the call's tad_replace_stats as a dict.  replace_stream_changes is this call
        with a report of what it changed."""
        return self._replace(state, key_id, flow_end_s, value, from_t, to_t, ranged, agg_flow, value_op, lattice, alpha, keep_from, job_id, num_keys,
                             key_id2, None)

    def replace_stream_changes(self, state, key_id, flow_end_s, value, changes="host", **kw):
        """replace_stream (whose other arguments go through **kw) with the change report (tad_state_replace_changes), carried by the
        returned dict as by merge_stream_changes'.  Changed points: added, erased by the range, or replaced by another value — a
        replace by the held value changes nothing, so the same re-read twice reports keys_changed == 0 the second time."""
        if changes is None:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "changes must be 'host', 'device' or 'counters'")
        return self._replace(state, key_id, flow_end_s, value, changes=changes, **kw)

    def _replace(self, state, key_id, flow_end_s, value, from_t=0, to_t=0, ranged=False, agg_flow="", value_op="auto", lattice=None,
                 alpha=0.0, keep_from=0, job_id="", num_keys=None, key_id2=None, changes=None):
        self._need("STATE_REPLACE", "tad_state_replace")
        cols, narrow, keep = self._stream_columns(state, key_id, flow_end_s, value, key_id2, num_keys, lattice)
        job = capi.Job(algo=capi.TAD_ALGO["EWMA"], agg_flow=capi.TAD_AGG[agg_flow], value_op=capi.TAD_OP[value_op], ewma_alpha=float(alpha),
                       flags=narrow, id=job_id.encode()[:63])
        stats = capi.ReplaceStats()
        ch, arr = self._changes(state, changes)
        args = (self._h, state._h, C.byref(job), C.byref(cols), capi.TAD_REPLACE_RANGE if ranged else 0, int(from_t), int(to_t), int(keep_from),
                C.byref(stats))
        rc = self._lib.tad_state_replace(*args) if ch is None else self._lib.tad_state_replace_changes(*args, C.byref(ch))
        del keep
        self._check(rc)
        return self._with_changes({name: getattr(stats, name) for name, _ in capi.ReplaceStats._fields_ if not name.startswith("reserved")}, ch, arr)

    def run_state(self, state, algo="EWMA", alpha=0.0, eps=0.0, min_samples=0, maxiter=0, emit_all=False, out="host", job_id=""):
        """The batch job's verdicts over everything `state` holds, from the state alone (tad_run_state): exactly the rows run() returns
        for the table of the state's series points with the same algo and parameters.  Needs a state with series=True and times=True
        (and history=True for DBSCAN); the state is left unchanged.  Narrow the window with TadState.trim first."""
        job = self._detector_job(algo, alpha, eps, min_samples, maxiter, emit_all=emit_all, job_id=job_id)
        self._need("STATE_RUN", "tad_run_state")
        return self._state_rows("tad_run_state", state, job, out)

    def run_state_window(self, state, from_t=0, to_t=0, keep_points=0, algo="EWMA", alpha=0.0, eps=0.0, min_samples=0, maxiter=0, emit_all=False,
                         out="host", job_id=""):
        """run_state over a window of what `state` holds, read-only (tad_run_state_window): of every key's series the points with
        flow_end_s >= from_t and < to_t (0 = no bound on that side), then the newest keep_points of those (0 = all).  Exactly the rows
        run() returns for the table of those points; the state is left unchanged.  Both bounds act on flowEndSeconds."""
        job = self._detector_job(algo, alpha, eps, min_samples, maxiter, emit_all=emit_all, job_id=job_id)
        self._need("STATE_WINDOW", "tad_run_state_window")
        return self._state_rows("tad_run_state_window", state, job, out, int(from_t), int(to_t), int(keep_points))

    # ---- the drop detector on a state (tad_drop_state / tad_drop_stream) ----
    def drop_state(self, state, from_t=0, to_t=0, keep_points=0, nsigma=0.0, min_samples=0, emit_all=False, out="host", job_id=""):
        """The drop detector's batch verdicts over a window of what `state` holds, read-only (tad_drop_state): exactly the rows
        run("DROP") returns for the table of the window's series points with the same nsigma / min_samples (0 = the defaults 3 and 3).
        The window is run_state_window's; all zero is the whole state.  Needs a state with series=True and times=True."""
        self._need("STATE_DROP", "tad_drop_state")
        job = self._detector_job("DROP", nsigma=nsigma, min_samples=min_samples, emit_all=emit_all, job_id=job_id)
        return self._state_rows("tad_drop_state", state, job, out, int(from_t), int(to_t), int(keep_points))

    def drop_stream(self, state, key_id, flow_end_s, value, agg_flow="", value_op="auto", lattice=None, nsigma=0.0, min_samples=0, alpha=0.0,
                    emit_all=False, out="host", job_id="", num_keys=None, key_id2=None):
        """One batch of the periodical drop job on `state` (tad_drop_stream): the state advances exactly as under run_stream with EWMA;
        the rows are those run("DROP") over everything the state now holds emits for this batch's points.  Needs a state with
        series=True (times and history are kept up when present)."""
        self._need("STATE_DROP", "tad_drop_stream")
        if agg_flow not in capi.TAD_AGG:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "agg_flow must be '', pod, svc or external")
        job = self._detector_job("DROP", alpha=alpha, nsigma=nsigma, min_samples=min_samples, emit_all=emit_all, job_id=job_id, agg_flow=agg_flow,
                                 value_op=value_op)
        cols, narrow, keep = self._stream_columns(state, key_id, flow_end_s, value, key_id2, num_keys, lattice)
        job.flags |= narrow
        return self._state_rows("tad_drop_stream", state, job, out, C.byref(cols))

    # ---- the window calls over selected keys (tad_run_state_keys / tad_drop_state_keys) ----
    @staticmethod
    def _key_mask(key_keep):
        """-> (pointer, length, tad_mem, what must stay alive) of a key mask: None, a DeviceArray of bytes, or anything numpy reads"""
        if key_keep is None:
            return None, 0, capi.TAD_MEM_HOST, None
        if isinstance(key_keep, DeviceArray):
            return key_keep.ptr, key_keep.n * np.dtype(key_keep.dtype).itemsize, capi.TAD_MEM_DEVICE, key_keep
        a = np.ascontiguousarray(np.asarray(key_keep).astype(np.uint8, copy=False)).reshape(-1)
        return (a.ctypes.data if a.size else None), a.size, capi.TAD_MEM_HOST, a

    def run_state_keys(self, state, key_keep, from_t=0, to_t=0, keep_points=0, algo="EWMA", alpha=0.0, eps=0.0, min_samples=0, maxiter=0,
                       emit_all=False, out="host", job_id=""):
        """run_state_window over the keys `key_keep` selects, read-only (tad_run_state_keys): key_keep has one byte per key of the state
        (a numpy array, or a DeviceArray such as KeyDict.select returns; any non-zero byte selects; None = every key).  Exactly the rows
        of run_state_window whose key is selected, with the state's own key ids; the stats and the ARIMA counters are those of a job
        over the selected points alone."""
        job = self._detector_job(algo, alpha, eps, min_samples, maxiter, emit_all=emit_all, job_id=job_id)
        self._need("KEY_SELECT", "tad_run_state_keys")
        ptr, n, mem, alive = self._key_mask(key_keep)
        return self._state_rows("tad_run_state_keys", state, job, out, int(from_t), int(to_t), int(keep_points), ptr, n, mem)

    def drop_state_keys(self, state, key_keep, from_t=0, to_t=0, keep_points=0, nsigma=0.0, min_samples=0, emit_all=False, out="host", job_id=""):
        """drop_state over the keys `key_keep` selects, read-only (tad_drop_state_keys); key_keep as for run_state_keys"""
        self._need("KEY_SELECT", "tad_drop_state_keys")
        ptr, n, mem, alive = self._key_mask(key_keep)
        job = self._detector_job("DROP", nsigma=nsigma, min_samples=min_samples, emit_all=emit_all, job_id=job_id)
        return self._state_rows("tad_drop_state_keys", state, job, out, int(from_t), int(to_t), int(keep_points), ptr, n, mem)

    # ---- judge the window, report from a time on (tad_run_state_since / tad_drop_state_since) ----
    def _report_window(self, state, since_t, key_since, key_keep, from_t, to_t, keep_points):
        """-> (tad_report_window, what must stay alive): both arrays in one memory — when one is a DeviceArray the other is copied there"""
        alive = []
        dev = isinstance(key_since, DeviceArray) or isinstance(key_keep, DeviceArray)

        def place(x, dtype, what):
            if x is None:
                return None
            if isinstance(x, DeviceArray):
                n = x.n * x.dtype.itemsize // np.dtype(dtype).itemsize
                if dtype == np.int64 and x.dtype.itemsize != 8:
                    raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "%s on the device must hold 8-byte elements" % what)
                if n < state.num_keys:
                    raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "%s has room for %d entries, the state holds %d keys" % (what, n, state.num_keys))
                alive.append(x)
                return x.ptr
            a = np.ascontiguousarray(np.asarray(x).astype(dtype, copy=False)).reshape(-1)
            if a.size != state.num_keys:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "%s has %d entries, the state holds %d keys" % (what, a.size, state.num_keys))
            if dev:   # (a byte mask travels in 8-byte elements, as KeyDict.select's does)
                pad = np.zeros((a.nbytes + 7) // 8 * 8 if a.nbytes else 8, np.uint8)
                pad[:a.nbytes] = a.view(np.uint8)
                a = DeviceArray.from_host(self, pad.view(np.uint64))
                alive.append(a)
                return a.ptr
            alive.append(a)
            return a.ctypes.data if a.size else None
        w = capi.ReportWindow(from_t=int(from_t), to_t=int(to_t), keep_points=int(keep_points), key_keep=place(key_keep, np.uint8, "key_keep"),
                              key_since=place(key_since, np.int64, "key_since"), since_t=int(since_t), num_keys=state.num_keys,
                              key_memory=capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST)
        return w, alive

    def run_state_since(self, state, since_t=0, key_since=None, key_keep=None, from_t=0, to_t=0, keep_points=0, algo="EWMA", alpha=0.0, eps=0.0,
                        min_samples=0, maxiter=0, emit_all=False, out="host", job_id=""):
        """run_state_keys that reports from a time on, read-only (tad_run_state_since): the window (from_t, to_t, keep_points) and the
        keys (key_keep) are judged exactly as run_state_keys judges them, and of its rows the call returns those with flow_end_s >=
        since_t (0 = no such bound) and >= key_since[key] — one int64 per key, a numpy array or a DeviceArray such as
        merge_stream_changes / replace_stream_changes return; a key whose entry is capi.TAD_NO_CHANGE is not selected at all.  Same
        order, same bits.  A changed key's points before its first changed time may have changed verdict and are not reported: that is
        the stream's rule, run_state_keys gives the whole answer."""
        job = self._detector_job(algo, alpha, eps, min_samples, maxiter, emit_all=emit_all, job_id=job_id)
        self._need("STATE_ALERTS", "tad_run_state_since")
        w, alive = self._report_window(state, since_t, key_since, key_keep, from_t, to_t, keep_points)
        res = self._state_rows("tad_run_state_since", state, job, out, C.byref(w))
        del alive
        return res

    def drop_state_since(self, state, since_t=0, key_since=None, key_keep=None, from_t=0, to_t=0, keep_points=0, nsigma=0.0, min_samples=0,
                         emit_all=False, out="host", job_id=""):
        """drop_state_keys that reports from a time on, read-only (tad_drop_state_since); the arguments are run_state_since's"""
        self._need("STATE_ALERTS", "tad_drop_state_since")
        job = self._detector_job("DROP", nsigma=nsigma, min_samples=min_samples, emit_all=emit_all, job_id=job_id)
        w, alive = self._report_window(state, since_t, key_since, key_keep, from_t, to_t, keep_points)
        res = self._state_rows("tad_drop_state_since", state, job, out, C.byref(w))
        del alive
        return res

    # ---- a state judged in time buckets (tad_run_state_buckets) ----
    def run_state_buckets(self, state, bucket_s, origin=0, op="sum", from_t=0, to_t=0, keep_points=0, key_keep=None, key_since=None, since_t=0,
                          algo="EWMA", alpha=0.0, eps=0.0, min_samples=0, maxiter=0, emit_all=False, out="host", job_id=""):
        """run_state_since over the window's points folded into time buckets, read-only (tad_run_state_buckets): exactly the rows run()
        returns with value_op=op ("sum" or "max") for the window's rows — from_t / to_t / keep_points and key_keep act on the raw points,
        first — with flow_end_s replaced by origin + bucket_s * floor((flow_end_s - origin) / bucket_s); the bucket's start stands in
        flow_end_s.  key_since / since_t: a bucket is reported iff it starts at or after the start of the threshold's bucket, so the
        bucket holding the first changed second is reported whole.  bucket_s=1 is run_state_keys."""
        job = self._detector_job(algo, alpha, eps, min_samples, maxiter, emit_all=emit_all, job_id=job_id)
        self._need("STATE_BUCKETS", "tad_run_state_buckets")
        if op not in ("sum", "max"):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "op must be sum or max")
        rw, alive = self._report_window(state, since_t, key_since, key_keep, from_t, to_t, keep_points)
        w = capi.BucketWindow(bucket_s=int(bucket_s), bucket_origin=int(origin), bucket_op=capi.TAD_OP[op])
        for name, _ in capi.ReportWindow._fields_:
            setattr(w, name, getattr(rw, name))
        res = self._state_rows("tad_run_state_buckets", state, job, out, C.byref(w))
        del alive
        return res

    # ---- the drop job's flow-row query (tad_drop_select) ----
    def drop_select(self, ingress_action, egress_action, flow_start_s, src_ip, src_pod_ns, src_pod_name, dst_ip, dst_pod_ns, dst_pod_name,
                    flow_end_s=None, src_pod_null=-1, dst_pod_null=-1, start_time=0, end_time=0, keep=None, out="device"):
        """Flow rows -> the drop job's rows (tad_drop_select): the rows whose ingress or egress rule action is 2 or 3 (and that pass
        start_time <= flow_start_s, flow_end_s < end_time and keep), each with its endpoint tuple (kind, ns, name), direction, day,
        count 1 and input row, in input order.  Columns: numpy arrays on the host, or DeviceArrays / CUDA tensors all on the device —
        uint8 actions and keep, int64 (or uint32: DateTime) times, int64 dictionary codes; *_pod_null: the pod-name code that means "no
        pod" on that side.  Returns a TadDropRows: the seven columns as DeviceArrays (out="device") or numpy arrays (out="host")."""
        if not (getattr(self._lib, "tad_features", None) and self._lib.tad_features() & capi.TAD_FEATURE_DROP_ROWS):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "this build of the library has no tad_drop_select (TAD_FEATURE_DROP_ROWS)")
        keepalive = []

        def col(x, dtype, what):
            """-> (pointer, n, on the device, element size)"""
            if x is None:
                return None, None, None, 0
            if isinstance(x, DeviceArray):
                p, n, dev, size = x.ptr, x.n, True, x.dtype.itemsize
                keepalive.append(x)
            elif hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and x.is_cuda:
                x = x.contiguous()
                p, n, dev, size = x.data_ptr(), x.numel(), True, x.element_size()
                keepalive.append(x)
            else:
                a = np.asarray(x.numpy() if hasattr(x, "data_ptr") else x)
                if not (dtype == np.int64 and what.startswith("flow_") and a.dtype == np.dtype(np.uint32)) and a.dtype != np.dtype(dtype):
                    a = a.astype(dtype)
                a = np.ascontiguousarray(a)
                p, n, dev, size = a.ctypes.data, a.size, False, a.dtype.itemsize
                keepalive.append(a)
            ok = (1,) if dtype == np.uint8 else ((4, 8) if what.startswith("flow_") else (8,))
            if size not in ok:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "drop_select: %s has %d-byte elements" % (what, size))
            return p, n, dev, size

        named = [("ingress_action", ingress_action, np.uint8), ("egress_action", egress_action, np.uint8), ("flow_start_s", flow_start_s, np.int64),
                 ("flow_end_s", flow_end_s, np.int64), ("src_ip", src_ip, np.int64), ("src_pod_ns", src_pod_ns, np.int64),
                 ("src_pod_name", src_pod_name, np.int64), ("dst_ip", dst_ip, np.int64), ("dst_pod_ns", dst_pod_ns, np.int64),
                 ("dst_pod_name", dst_pod_name, np.int64)]
        got = {name: col(x, dt, name) for name, x, dt in named}
        n, dev = got["ingress_action"][1], got["ingress_action"][2]
        present = [v for v in got.values() if v[1] is not None]
        if n is None or any(v[1] != n or v[2] != dev for v in present):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "drop_select: columns must have equal length and live in the same memory")
        widths = set(got[name][3] for name in ("flow_start_s", "flow_end_s") if got[name][1] is not None)
        if len(widths) > 1:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "drop_select: flow_start_s / flow_end_s must have the same width")
        pkeep = None
        if keep is not None:
            if not isinstance(keep, DeviceArray) and not (hasattr(keep, "is_cuda") and keep.is_cuda):
                a = np.ascontiguousarray(np.asarray(keep).astype(np.uint8, copy=False))
                if dev:       # a host mask over device columns is uploaded
                    padded = np.frombuffer(a.tobytes() + b"\0" * (-a.size % 8 or 8), dtype=np.uint64)
                    keep = DeviceArray.from_host(self, padded).view(0, a.size, np.uint8)
                else:
                    keep = a
            pkeep, nk, devk, _ = col(keep, np.uint8, "keep")
            if nk != n or devk != dev:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "drop_select: keep must have one byte per row and live where the columns live")
        fc = capi.DropFlowColumns(n_rows=n, src_pod_null=int(src_pod_null), dst_pod_null=int(dst_pod_null), keep=pkeep,
                                  flags=capi.TAD_FLAG_TIME_U32 if widths == {4} else 0, memory=capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST)
        for name, _, _ in named:
            setattr(fc, name, got[name][0])
        res = C.POINTER(capi.DropRows)()
        rc = self._lib.tad_drop_select(self._h, C.byref(fc), int(start_time), int(end_time),
                                       capi.TAD_MEM_DEVICE if out == "device" else capi.TAD_MEM_HOST, C.byref(res))
        del keepalive
        self._check(rc)
        return TadDropRows(self, res)

    # ---- row-sharded ingest: bucket device rows by owner = key mod world (tad_shard_rows) ----
    def shard_rows(self, key_id, flow_end_s, value, world):
        """Device columns (torch CUDA tensors or DeviceArray) -> ((key_local, flow_end_s, value) DeviceArrays grouped by
        destination rank, counts per destination): the payload and the send splits of the all-to-all(v)."""
        pk, n, dev, keep1 = _as_column(key_id, np.uint64)
        pt, nt, dev_t, keep2 = _as_column(flow_end_s, np.int64)
        pv, nv, dev_v, keep3 = _as_column(value, np.uint64)
        if nt != n or nv != n or not (dev and dev_t and dev_v):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "shard_rows: three device columns of equal length")
        outs = (DeviceArray(self, n, np.uint64), DeviceArray(self, n, np.int64), DeviceArray(self, n, np.uint64))
        counts = np.zeros(int(world), dtype=np.uint64)
        cols = capi.Columns(n_rows=n, key_id=pk, flow_end_s=pt, value=pv, num_keys=0, memory=capi.TAD_MEM_DEVICE)
        rc = self._lib.tad_shard_rows(self._h, C.byref(cols), int(world), outs[0].ptr, outs[1].ptr, outs[2].ptr, counts.ctypes.data)
        del keep1, keep2, keep3
        self._check(rc)
        return outs, [int(c) for c in counts]

    # ---- columnar ingest: Arrow buffers -> 8-byte device columns (tad_widen_column / tad_mask_rows) ----
    def widen_into(self, dst, dst_offset, src_ptr, bits, signed, n, src_device=False, table=None):
        """dst[dst_offset + i] = table[src[i]] (table: DeviceArray of int64) or src[i] widened, for i < n.  dst: DeviceArray of 8-byte
        elements; src_ptr: address of n integers of `bits` bits in host memory (or device memory with src_device)."""
        if dst_offset < 0 or dst_offset + n > dst.n:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "widen_into: rows %d..%d do not fit a column of %d" % (dst_offset, dst_offset + n, dst.n))
        self._check(self._lib.tad_widen_column(self._h, src_ptr, int(bits), 1 if signed else 0, capi.TAD_MEM_DEVICE if src_device else capi.TAD_MEM_HOST,
                                               int(n), table.ptr if table is not None else None, table.n if table is not None else 0,
                                               dst.ptr + 8 * int(dst_offset)))

    def gather(self, column, rows):
        """column[rows] for a device column (DeviceArray of 8-byte elements) and device row numbers (DeviceArray u64) -> numpy array"""
        out = DeviceArray(self, max(rows.n, 1), column.dtype)
        out.n = rows.n
        if rows.n:
            self._check(self._lib.tad_widen_column(self._h, rows.ptr, 64, 0, capi.TAD_MEM_DEVICE, rows.n, column.ptr, column.n, out.ptr))
        host = out.to_host()
        out.free()
        return host

    def mask_rows(self, n, terms, keep=None):
        """terms: list of (codes DeviceArray int64[n], mask numpy bool[D]) -> DeviceArray uint8-as-bytes keep[n] = AND of mask[codes[i]] (ANDed into
        `keep` when one is given).  The masks are per DISTINCT value (the host evaluated the SQL's string predicates on the dictionaries)."""
        if not 0 <= len(terms) <= 8:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "mask_rows: at most 8 terms")
        combine = keep is not None
        if keep is None:
            keep = DeviceArray(self, (n + 7) // 8 + 1, np.uint64)     # n bytes, allocated in 8-byte elements
        masks = []
        for _, m in terms:
            a = np.ascontiguousarray(np.asarray(m, dtype=bool).astype(np.uint8))
            masks.append((DeviceArray.from_host(self, np.frombuffer(a.tobytes() + b"\0" * (-a.size % 8 or 8), dtype=np.uint64)), a.size))
        k = len(terms)
        codes_p = (C.c_void_p * max(k, 1))(*[c.ptr for c, _ in terms])
        masks_p = (C.c_void_p * max(k, 1))(*[d.ptr for d, _ in masks])
        lens = (capi.u64 * max(k, 1))(*[ln for _, ln in masks])
        if k == 0 and not combine:      # no predicate: every row is kept
            ones = np.ones(((n + 7) // 8 + 1) * 8, dtype=np.uint8)
            self._check(self._lib.tad_copy_to_device(self._h, keep.ptr, ones.ctypes.data, ones.size))
        elif k:
            self._check(self._lib.tad_mask_rows(self._h, int(n), k, codes_p, masks_p, lens, 1 if combine else 0, keep.ptr))
        for d, _ in masks:
            d.free()
        return keep

    # ---- ingest: key tuples -> dense ids in order of first appearance (tad_factorize) ----
    def factorize(self, cols_a, keep_a=None, cols_b=None, keep_b=None, max_keys=None, with_hist=False):
        """cols_a: list of 1..8 equally long int64 arrays (numpy on the host, or DeviceArray / device pointers all on the device) —
        the key tuple of every row; keep_a: bool / uint8 mask (None = every row); cols_b / keep_b: the second tuple of every row
        (pod mode).  Returns (key_id u64[n], key_id2 u64[n] or None, first_row u64[num_keys]) — ids in order of first appearance over
        the virtual rows [side a ++ side b], TAD_KEY_SKIP where the mask is 0 — in the memory the inputs live in.  with_hist: a fourth
        return value, the KeyHistogram of the ids (tad_factorize_hist) for TadEngine.run(key_hist=...) on the same batch."""
        ncol = len(cols_a)
        if not 1 <= ncol <= 8 or (cols_b is not None and len(cols_b) != ncol):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "factorize: 1..8 key columns, the same number on both sides")
        keepalive = []

        def col(x, dtype):
            p, n, dev, keep = _as_column(x, dtype)
            keepalive.append(keep)
            return p, n, dev

        pa = [col(c, np.int64) for c in cols_a]
        n, dev = pa[0][1], pa[0][2]
        pb = [col(c, np.int64) for c in cols_b] if cols_b is not None else None
        if any(q[1] != n or q[2] != dev for q in pa + (pb or [])):
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "factorize: columns must have equal length and live in the same memory")

        def mask(m):
            if m is None:
                return None
            if isinstance(m, DeviceArray):
                return m.ptr
            a = np.ascontiguousarray(np.asarray(m).astype(np.uint8, copy=False))
            if a.size != n:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "factorize: mask length")
            if dev:
                d = DeviceArray.from_host(self, np.frombuffer(a.tobytes() + b"\0" * (-a.size % 8), dtype=np.uint64))
                keepalive.append(d)
                return d.ptr
            keepalive.append(a)
            return a.ctypes.data

        ka, kb = mask(keep_a), mask(keep_b)
        arr_a = (C.c_void_p * ncol)(*[q[0] for q in pa])
        arr_b = (C.c_void_p * ncol)(*[q[0] for q in pb]) if pb is not None else None
        sides = 2 if pb is not None else 1
        cap = int(max_keys) if max_keys is not None else n * sides
        kc = capi.KeyColumns(n_rows=n, n_cols=ncol, cols_a=arr_a, keep_a=ka, cols_b=arr_b, keep_b=kb,
                             memory=capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST)
        nk = capi.u64()
        hist = KeyHistogram(self) if with_hist else None

        def call(k1, k2, fr):
            if hist is not None:
                return self._lib.tad_factorize_hist(self._h, C.byref(kc), k1, k2, fr, cap, C.byref(nk), C.byref(hist.c))
            return self._lib.tad_factorize(self._h, C.byref(kc), k1, k2, fr, cap, C.byref(nk))
        if dev:
            key1 = DeviceArray(self, n, np.uint64)
            key2 = DeviceArray(self, n, np.uint64) if pb is not None else None
            first = DeviceArray(self, max(cap, 1), np.uint64)
            rc = call(key1.ptr, key2.ptr if key2 is not None else None, first.ptr)
            del keepalive
            self._check(rc)
            first.n = min(int(nk.value), cap)
            return (key1, key2, first, hist) if with_hist else (key1, key2, first)
        key1 = np.empty(n, dtype=np.uint64)
        key2 = np.empty(n, dtype=np.uint64) if pb is not None else None
        first = np.empty(max(cap, 1), dtype=np.uint64)
        rc = call(key1.ctypes.data, key2.ctypes.data if key2 is not None else None, first.ctypes.data)
        del keepalive
        self._check(rc)
        first = first[:min(int(nk.value), cap)]
        return (key1, key2, first, hist) if with_hist else (key1, key2, first)

    # ---- ingest for the streaming states: key ids that stay the same from batch to batch (tad_keydict) ----
    def key_dict(self, n_cols, expected_keys=0):
        """A persistent key dictionary for tuples of n_cols int64 columns (KeyDict): encode every batch through it, resize the state
        when num_keys grew, then run_stream / merge_stream with num_keys = the dictionary's."""
        return KeyDict(self, n_cols, expected_keys)

    def string_dict(self, expected_values=0, expected_bytes=0):
        """A persistent string dictionary (StringDict): encode every batch's string key column through it and hand the codes to the
        KeyDict; its match() masks are KeyDict.select's terms."""
        return StringDict(self, expected_values, expected_bytes)

    # ---- ingest, one step earlier: an Arrow string column -> dictionary codes (tad_encode_strings) ----
    def encode_strings(self, column, max_values=None):
        """column: a pyarrow string / large_string / binary / large_binary Array (host memory; slices and nulls are fine: a null encodes like
        ""), or a tuple (offsets, data) / (offsets, data, validity, validity_offset) — numpy arrays on the host (offsets int32 or int64, data
        uint8), or DeviceArrays on the device (offsets as int32 / int64 elements).  Returns (codes int64[n], first_row u64[num_values]): codes
        in order of first appearance (pyarrow.compute.dictionary_encode's, pandas.factorize's), first_row[k] = the row where value k
        first appears — in the memory the input lives in."""
        sc, n, dev, keepalive = _string_column(column, "encode_strings")
        cap = int(max_values) if max_values is not None else n
        nv = capi.u64()
        if dev:
            codes = DeviceArray(self, max(n, 1), np.int64)
            first = DeviceArray(self, max(cap, 1), np.uint64)
            rc = self._lib.tad_encode_strings(self._h, C.byref(sc), codes.ptr, first.ptr, cap, C.byref(nv))
            del keepalive
            self._check(rc)
            codes.n, first.n = n, min(int(nv.value), cap)
            return codes, first
        codes = np.empty(n, dtype=np.int64)
        first = np.empty(max(cap, 1), dtype=np.uint64)
        rc = self._lib.tad_encode_strings(self._h, C.byref(sc), codes.ctypes.data, first.ctypes.data, cap, C.byref(nv))
        del keepalive
        self._check(rc)
        return codes, first[:min(int(nv.value), cap)]

    # ---- Stage 0 alone: the GROUP BY (anomaly_detection.py:507-614) ----
    def aggregate(self, key_id, flow_end_s, value, num_keys, agg_flow="", value_op="auto", key_id2=None, flow_start_s=None,
                  start_time=0, end_time=0, lattice=None, out="host"):
        if agg_flow not in capi.TAD_AGG:
            raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "agg_flow must be '', pod, svc or external")
        narrow = _narrow_flags(self._lib, key_id, key_id2, flow_end_s, flow_start_s)
        pk, n, dev, keep1 = _as_column(key_id, np.uint64, narrow="key")
        pt, nt, dev_t, keep2 = _as_column(flow_end_s, np.int64, narrow="time")
        pv, nv, dev_v, keep3 = _as_column(value, np.uint64)
        pk2, nk2, dev_k2, keep4 = _as_column(key_id2, np.uint64, narrow="key")
        ps, ns, dev_s, keep5 = _as_column(flow_start_s, np.int64, narrow="time")
        for m, d in ((nt, dev_t), (nv, dev_v)) + (((nk2, dev_k2),) if key_id2 is not None else ()) + \
                (((ns, dev_s),) if flow_start_s is not None else ()):
            if m != n or d != dev:
                raise TadError(capi.TAD_ERR_INVALID_ARGUMENT, "columns must have equal length and live in the same memory")
        job = capi.Job(algo=0, agg_flow=capi.TAD_AGG[agg_flow], value_op=capi.TAD_OP[value_op],
                       start_time=int(start_time), end_time=int(end_time), flags=narrow)
        cols = capi.Columns(n_rows=n, key_id=pk, key_id2=pk2, flow_end_s=pt, flow_start_s=ps, value=pv,
                            num_keys=int(num_keys), memory=capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST)
        if lattice is not None:
            cols.t0, cols.step, cols.n_buckets = int(lattice[0]), int(lattice[1]), int(lattice[2])
        res = C.POINTER(capi.Points)()
        rc = self._lib.tad_aggregate(self._h, C.byref(job), C.byref(cols),
                                     capi.TAD_MEM_DEVICE if out == "device" else capi.TAD_MEM_HOST, C.byref(res))
        del keep1, keep2, keep3, keep4, keep5
        self._check(rc)
        return TadPoints(self, res)

    # ---- the reference's per-series pure functions, on the GPU ----
    @staticmethod
    def _series(x):
        a = np.ascontiguousarray(np.asarray([int(v) for v in x] if not isinstance(x, np.ndarray) else x, dtype=np.uint64))
        return a

    def series_ewma(self, x, alpha=0.0):
        a = self._series(x)
        out = np.empty(a.size, dtype=np.float64)
        self._check(self._lib.tad_series_ewma(self._h, a.ctypes.data, a.size, float(alpha), out.ctypes.data))
        return out

    def series_ewma_anomaly(self, x, stddev, alpha=0.0):
        a = self._series(x)
        out = np.zeros(a.size, dtype=np.uint8)
        self._check(self._lib.tad_series_ewma_anomaly(self._h, a.ctypes.data, a.size, float(alpha),
                                                      0 if stddev is None else 1, 0.0 if stddev is None else float(stddev),
                                                      out.ctypes.data))
        return out.astype(bool)

    def series_stddev(self, x):
        a = self._series(x)
        has, sd = C.c_int(), capi.f64()
        self._check(self._lib.tad_series_stddev(self._h, a.ctypes.data, a.size, C.byref(has), C.byref(sd)))
        return sd.value if has.value else None

    def series_dbscan_anomaly(self, x, eps=0.0, min_samples=0):
        a = self._series(x)
        out = np.zeros(a.size, dtype=np.uint8)
        self._check(self._lib.tad_series_dbscan_anomaly(self._h, a.ctypes.data, a.size, float(eps), int(min_samples), out.ctypes.data))
        return out.astype(bool)

    def series_drop(self, x, nsigma=0.0, min_samples=0):
        """DropDetection.end_partition on one partition -> None (too few samples) or (mean, std, verdict bool[n])."""
        a = self._series(x)
        out = np.zeros(max(a.size, 1), dtype=np.uint8)
        has, mean, sd = C.c_int(), capi.f64(), capi.f64()
        self._check(self._lib.tad_series_drop(self._h, a.ctypes.data, a.size, float(nsigma), int(min_samples), C.byref(has),
                                              C.byref(mean), C.byref(sd), out.ctypes.data))
        return (mean.value, sd.value, out[:a.size].astype(bool)) if has.value else None

    def series_arima(self, x, maxiter=0):
        a = self._series(x)
        out = np.empty(a.size, dtype=np.float64)
        has = C.c_int()
        self._check(self._lib.tad_series_arima(self._h, a.ctypes.data, a.size, int(maxiter), C.byref(has), out.ctypes.data))
        return out if has.value else None

    def series_arima_anomaly(self, x, stddev, maxiter=0):
        a = self._series(x)
        out = np.zeros(max(a.size, 1), dtype=np.uint8)
        nv = capi.u64()
        self._check(self._lib.tad_series_arima_anomaly(self._h, a.ctypes.data, a.size, int(maxiter),
                                                       0 if stddev is None else 1, 0.0 if stddev is None else float(stddev),
                                                       out.ctypes.data, C.byref(nv)))
        return out[:nv.value].astype(bool)

    # ---- synthetic table straight into HBM ----
    def synth(self, first_row, n_rows, num_keys, n_buckets, seed=SYNTH_SEED, into=None):
        """Returns (key_id, flow_end_s, value) as DeviceArray, or fills the 3 given torch CUDA tensors."""
        if into is None:
            cols = (DeviceArray(self, n_rows, np.uint64), DeviceArray(self, n_rows, np.int64), DeviceArray(self, n_rows, np.uint64))
            ptrs = [c.ptr for c in cols]
        else:
            cols = into
            ptrs = [t.data_ptr() for t in into]
        self._check(self._lib.tad_synth_generate(self._h, int(seed), int(first_row), int(n_rows), int(num_keys), int(n_buckets), *ptrs))
        return cols
