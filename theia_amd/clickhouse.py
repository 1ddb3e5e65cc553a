"""ClickHouse transport for the Throughput Anomaly Detection host.

The reference job reads `default.flows` and appends to `default.tadetector` through Spark's JDBC source over one
connection (anomaly_detection.py:651-662, 713-726; URL `jdbc:clickhouse://clickhouse-clickhouse.flow-visibility.svc:8123`,
:730-731; credentials in CH_USERNAME / CH_PASSWORD, controller.go:649-658).  Port 8123 is ClickHouse's HTTP interface,
which speaks columnar formats directly: this module POSTs the query with `FORMAT ArrowStream` and hands the Arrow
record batches to numpy without a row-by-row decode, and appends results with `INSERT ... FORMAT ArrowStream` (column
dicts; `FORMAT JSONEachRow` for the few-row case such as the sentinel row).
Only the standard library (urllib) and pyarrow are used.

Two ways to read (both end in the same numbers):
  * raw rows  — SELECT of the mode's key columns, flowEndSeconds, flowStartSeconds, throughput with the WHERE clause
    of the reference SQL; the GPU engine does the GROUP BY (Stage 0).  `rows_query`.
  * pushdown  — the reference's own SQL (generate_tad_sql_query): ClickHouse aggregates, the engine receives points.
    Re-aggregating points with the same operator is the identity, so tad_run works unchanged on them.

Not verified against a live ClickHouse server (none in the build image): tests/test_clickhouse_http.py runs it
against an in-process HTTP server that speaks the same two formats.
"""
import base64
import io
import json
import os
import urllib.parse
import urllib.request

import numpy as np

DEFAULT_JDBC_URL = "jdbc:clickhouse://clickhouse-clickhouse.flow-visibility.svc:8123"   # anomaly_detection.py:730-731
FLOWS_TABLE = "default.flows"
RESULT_TABLE = "default.tadetector"


def jdbc_to_http(url):
    """'jdbc:clickhouse://host:8123[/db]' -> 'http://host:8123'; http(s) URLs pass through."""
    if url.startswith("jdbc:clickhouse://"):
        rest = url[len("jdbc:clickhouse://"):]
        return "http://" + rest.split("/", 1)[0]
    if url.startswith("http://") or url.startswith("https://"):
        return url.rstrip("/")
    raise ValueError("Please provide a valid JDBC url for ClickHouse database")   # anomaly_detection.py:823-829


# string-column bytes handed to one tad_encode_strings call (query_columns(engine=...)): below Arrow's 2 GB limit of int32 offsets, and large
# because every chunk after a column's first pays a gather that maps its codes into the column's unified dictionary
STRING_CHUNK_BYTES = 1 << 30


class ClickHouseHTTP:
    def __init__(self, url=DEFAULT_JDBC_URL, user=None, password=None, timeout=600):
        self.base = jdbc_to_http(url)
        self.user = user if user is not None else os.getenv("CH_USERNAME")
        self.password = password if password is not None else os.getenv("CH_PASSWORD")
        self.timeout = timeout

    def _request(self, params, body):
        req = urllib.request.Request(self.base + "/?" + urllib.parse.urlencode(params), data=body, method="POST")
        if self.user:
            token = base64.b64encode(("%s:%s" % (self.user, self.password or "")).encode()).decode()
            req.add_header("Authorization", "Basic " + token)
        return urllib.request.urlopen(req, timeout=self.timeout)

    def _post(self, params, body):
        with self._request(params, body) as resp:
            return resp.read()

    def query_columns(self, sql, dict_strings=False, params=None, engine=None):
        """Run a SELECT, return {column name: numpy array}.  `params`: values of the statement's `{name:Type}` placeholders, sent as
        `param_<name>` URL parameters (the HTTP interface's query parameters: the value never becomes SQL text).
        `engine` (with dict_strings): plain string columns are dictionary-encoded ON THE GPU (TadEngine.encode_strings = tad_encode_strings,
        include/tad.h) in chunks of ~STRING_CHUNK_BYTES (1 GB) of column bytes instead of by Arrow on one host core per record batch — the same
        codes and dictionaries (first-appearance order per chunk, unified over the chunks exactly as the batch dictionaries are).  DateTime -> int64 epoch seconds, String -> str — or, with
        dict_strings=True, String -> theia_amd.anomaly_detection.DictColumn (integer codes per row + the distinct values, one
        dictionary per column unified over the record batches): no Python object per row is ever created, which is what makes
        the host side of a 1e8-row job tractable (prepare_columns evaluates the string predicates on the distinct values).
        The ArrowStream response is consumed record batch by record batch straight from the socket (the raw-rows read of
        a large `flows` table is tens of GB: no whole-response buffer), strings are decoded through Arrow's dictionary
        encoding (one Python object per DISTINCT value per batch, not per row)."""
        import pyarrow as pa
        import pyarrow.compute as pc
        import pyarrow.ipc as ipc
        parts = {}
        vocab = {}     # dict_strings: column -> {string: code}
        settings = {"output_format_arrow_string_as_string": 1}
        for pname, pvalue in (params or {}).items():
            settings["param_" + pname] = pvalue
        with self._request(settings, (sql.rstrip() + " FORMAT ArrowStream").encode()) as resp:
            if not resp.peek(1):           # a truly empty body: a result without rows carries no schema
                return {}
            # anything else must be an Arrow stream: a proxy's error page or exception text after the headers raises
            # pa.ArrowInvalid here instead of turning into a job on zero rows that reports "no anomalies"
            reader = ipc.open_stream(resp)
            def stringish(t):   # plain strings / binaries, and dictionary-typed columns of them (LowCardinality sent as Arrow dictionaries)
                if pa.types.is_dictionary(t):
                    t = t.value_type
                return pa.types.is_binary(t) or pa.types.is_large_binary(t) or pa.types.is_string(t) or pa.types.is_large_string(t)
            for name, t in zip(reader.schema.names, reader.schema.types):   # a schema without batches: empty typed columns
                is_str = stringish(t)
                if is_str and dict_strings:
                    vocab.setdefault(name, {})      # only columns that go through the string branch get a dictionary
                if is_str:
                    parts[name] = [np.zeros(0, dtype=np.int64 if dict_strings else str)]
                elif pa.types.is_floating(t) or pa.types.is_decimal(t):
                    parts[name] = [np.zeros(0, dtype=np.float64)]
                elif pa.types.is_boolean(t):
                    parts[name] = [np.zeros(0, dtype=bool)]
                else:
                    parts[name] = [np.zeros(0, dtype=np.int64)]
            pending = {}   # engine: column -> [raw Arrow string arrays of the current chunk, their bytes]

            def flush(name):
                arrays, _ = pending.pop(name)
                arr = arrays[0] if len(arrays) == 1 else pa.concat_arrays(arrays)
                codes, first = engine.encode_strings(arr)
                dvals = arr.take(pa.array(first.astype(np.int64))).fill_null("").to_pylist()
                voc = vocab.setdefault(name, {})
                remap = np.fromiter((voc.setdefault(v, len(voc)) for v in dvals), dtype=np.int64, count=len(dvals))
                if remap.size and not np.array_equal(remap, np.arange(remap.size)):      # (a column's first chunk IS its dictionary: no gather)
                    codes = remap[codes]
                parts.setdefault(name, []).append(codes if remap.size else np.zeros(0, dtype=np.int64))

            for batch in reader:
                for name, col in zip(batch.schema.names, batch.columns):
                    t = col.type
                    if pa.types.is_timestamp(t) or pa.types.is_date(t):
                        arr = col.cast(pa.timestamp("s")).cast(pa.int64()).to_numpy(zero_copy_only=False)
                    elif stringish(t):
                        if pa.types.is_dictionary(t):     # already dictionary-encoded by the server: keep its indices, no re-encode
                            d = col
                            if not (pa.types.is_string(t.value_type) or pa.types.is_large_string(t.value_type)):
                                d = pa.DictionaryArray.from_arrays(col.indices, col.dictionary.cast(pa.string()))
                            idx = d.indices.fill_null(0).to_numpy(zero_copy_only=False) if d.indices.null_count == 0 else None
                            if idx is None:               # null rows read as '' like the plain-string path
                                d = pc.dictionary_encode(d.cast(pa.string()).fill_null(""))
                                idx = d.indices.to_numpy(zero_copy_only=False)
                        else:
                            if pa.types.is_binary(t) or pa.types.is_large_binary(t):
                                col = col.cast(pa.string() if pa.types.is_binary(t) else pa.large_string())
                            if engine is not None and dict_strings:
                                # raw offsets + bytes wait for the GPU: a chunk is encoded once it holds enough bytes (bounded host
                                # memory, int32 offsets never overflow), its codes join the column's parts in row order
                                pend = pending.setdefault(name, [[], 0])
                                pend[0].append(col)
                                pend[1] += col.nbytes
                                if pend[1] >= STRING_CHUNK_BYTES:
                                    flush(name)
                                continue
                            d = pc.dictionary_encode(col.fill_null(""))
                            idx = d.indices.to_numpy(zero_copy_only=False)
                        dvals = ["" if v is None else v for v in d.dictionary.to_pylist()]
                        if dict_strings:      # remap this batch's dictionary into the column's unified one: per-row work is one integer gather
                            voc = vocab.setdefault(name, {})
                            remap = np.fromiter((voc.setdefault(v, len(voc)) for v in dvals), dtype=np.int64, count=len(dvals))
                            arr = remap[idx] if remap.size else np.zeros(0, dtype=np.int64)
                        else:
                            values = np.asarray(dvals, dtype=object).astype(str)
                            arr = values[idx] if values.size else np.zeros(0, dtype=str)
                    elif pa.types.is_decimal(t):
                        arr = col.cast(pa.float64()).to_numpy(zero_copy_only=False)
                    else:                     # integers, floats, bool: passed through unchanged
                        arr = col.to_numpy(zero_copy_only=False)
                    parts.setdefault(name, []).append(arr)
            for name in list(pending):
                flush(name)
        out = {name: (np.concatenate(v[1:]) if len(v) > 2 else (v[1] if len(v) == 2 else v[0])) for name, v in parts.items()}
        if dict_strings:
            from .anomaly_detection import DictColumn
            for name, voc in vocab.items():
                values = np.empty(len(voc), dtype=object)
                for v, c in voc.items():
                    values[c] = v
                out[name] = DictColumn(np.asarray(out[name], dtype=np.int64), values.astype(str) if len(voc) else np.zeros(0, dtype=str))
        return out

    def command(self, sql):
        """Run a statement without a result set (e.g. cleanupTADetector's ALTER TABLE ... DELETE, controller.go:396)."""
        self._post({}, sql.encode())

    def insert_rows(self, rows, table=RESULT_TABLE):
        """Append dict rows (INSERT ... FORMAT JSONEachRow); columns a row lacks take the table defaults."""
        if not rows:
            return 0
        body = "\n".join(json.dumps(r) for r in rows).encode()
        self._post({"query": "INSERT INTO %s FORMAT JSONEachRow" % table, "date_time_input_format": "best_effort"}, body)
        return len(rows)

    def insert_columns(self, columns, table=RESULT_TABLE):
        """Append a column dict (INSERT ... FORMAT ArrowStream): the result columns go out the way the flow columns came
        in.  DateTime columns (flowEndSeconds / flowStartSeconds) travel as UInt32 epoch seconds, which ClickHouse accepts
        for DateTime; columns the dict lacks take the table defaults."""
        import pyarrow as pa
        import pyarrow.ipc as ipc
        if not columns:
            return 0
        n = len(next(iter(columns.values())))
        arrays = {}
        for name, v in columns.items():
            v = np.asarray(v)
            kind = TADETECTOR_COLUMNS.get(name)          # explicit per-column types: nothing is narrowed by dtype guesswork
            if kind is None:
                raise ValueError("insert_columns: %r is not a column of %s (create_table.sh:363-384)" % (name, RESULT_TABLE))
            if kind == "datetime":
                arrays[name] = pa.array(v.astype(np.uint32), pa.uint32())
            elif kind == "f64":
                arrays[name] = pa.array(v.astype(np.float64), pa.float64())
            elif kind in ("u16", "u8"):
                lim = 65535 if kind == "u16" else 255
                if v.size and (v.astype(np.int64).min() < 0 or v.astype(np.int64).max() > lim):
                    raise ValueError("insert_columns: %s out of range for %s" % (name, kind))
                arrays[name] = pa.array(v.astype(np.uint16 if kind == "u16" else np.uint8), pa.uint16() if kind == "u16" else pa.uint8())
            else:
                arrays[name] = pa.array([str(x) for x in v.tolist()], pa.string())
        table_ = pa.table(arrays)
        sink = io.BytesIO()
        with ipc.new_stream(sink, table_.schema) as w:
            w.write_table(table_)
        cols = ", ".join(table_.column_names)
        self._post({"query": "INSERT INTO %s (%s) FORMAT ArrowStream" % (table, cols)}, sink.getvalue())
        return n


# default.tadetector (create_table.sh:363-384): column -> wire type of the ArrowStream insert
TADETECTOR_COLUMNS = {
    "sourceIP": "str", "sourceTransportPort": "u16", "destinationIP": "str", "destinationTransportPort": "u16",
    "protocolIdentifier": "u16", "flowStartSeconds": "datetime", "podNamespace": "str", "podLabels": "str", "podName": "str",
    "destinationServicePortName": "str", "direction": "str", "flowEndSeconds": "datetime", "throughputStandardDeviation": "f64",
    "aggType": "str", "algoType": "str", "algoCalc": "f64", "throughput": "f64", "anomaly": "str", "id": "str",
}

# raw columns each mode needs (create_table.sh:31-85)
_RAW_COLUMNS = {
    "": ["sourceIP", "sourceTransportPort", "destinationIP", "destinationTransportPort", "protocolIdentifier",
         "flowStartSeconds", "flowEndSeconds", "throughput", "sourcePodNamespace", "destinationPodNamespace"],
    "external": ["destinationIP", "flowType", "flowStartSeconds", "flowEndSeconds", "throughput", "sourcePodNamespace",
                 "destinationPodNamespace"],
    "svc": ["destinationServicePortName", "flowStartSeconds", "flowEndSeconds", "throughput", "sourcePodNamespace",
            "destinationPodNamespace"],
    "pod": ["sourcePodNamespace", "destinationPodNamespace", "sourcePodLabels", "destinationPodLabels", "sourcePodName",
            "destinationPodName", "flowStartSeconds", "flowEndSeconds", "throughput"],
}


# the string columns of default.flows the job reads (create_table.sh:31-85: all plain `String`)
STRING_COLUMNS = ("sourceIP", "destinationIP", "sourcePodNamespace", "destinationPodNamespace", "sourcePodLabels", "destinationPodLabels",
                  "sourcePodName", "destinationPodName", "destinationServicePortName")
# settings of the dictionary read: LowCardinality columns leave ClickHouse as Arrow DICTIONARY arrays (a dictionary per block), and blocks are
# large so that a block's dictionary (the distinct values the host looks at) is small against its rows
DICTIONARY_SETTINGS = {"output_format_arrow_low_cardinality_as_dictionary": 1, "output_format_arrow_string_as_string": 1, "max_block_size": 4194304}


def shard_expr(agg_flow, shards):
    """`cityHash64(...) % shards`: which of `shards` parallel reads a row belongs to (the same expression shards the rows
    over GPUs).  Hashing the connection tuple spreads every mode's rows evenly; which read delivers a row does not enter the result (the
    engine's Stage 0 is commutative)."""
    return "cityHash64(sourceIP, sourceTransportPort, destinationIP, destinationTransportPort, flowStartSeconds, flowEndSeconds) %% %d" % int(shards)


def rows_query(start_time, end_time, ns_ignore_list, agg_flow=None, pod_label=None, external_ip=None, svc_port_name=None,
               pod_name=None, pod_namespace=None, dictionary=False, shard=None, count_only=False):
    """SELECT of the raw rows the job needs: the WHERE clause of the reference SQL (anomaly_detection.py:507-614) without
    its GROUP BY.  Pod mode keeps a row if EITHER side passes its condition (the UNION ALL of :556-565 reads each
    side separately); the host applies the per-side predicates again when it builds the two keys.
    dictionary: string columns as `toLowCardinality(c) AS c` (with DICTIONARY_SETTINGS they arrive as Arrow dictionary arrays), and only
    the columns the mode's job reads.  shard = (g, G): the rows of read g of G (`AND cityHash64(...) % G = g`).  count_only: the rows per
    shard instead of the rows (`SELECT <shard expr> AS shard, count() AS rows ... GROUP BY shard`; shard = (None, G))."""
    mode = agg_flow if agg_flow in ("pod", "external", "svc") else ""
    where = []
    if ns_ignore_list:
        quoted = ", ".join("'{}'".format(x) for x in ns_ignore_list)
        where.append("sourcePodNamespace NOT IN ({0}) AND destinationPodNamespace NOT IN ({0})".format(quoted))
    if mode == "pod":
        sides = []
        for side in ("destination", "source"):
            if pod_label:
                cond = "ilike({}PodLabels, '%{}%')".format(side, pod_label)
            elif pod_name:
                cond = "{}PodName = '{}'".format(side, pod_name)
            else:
                cond = "{}PodLabels <> ''".format(side)
            if (pod_label or pod_name) and pod_namespace:
                cond = "({} AND {}PodNamespace = '{}')".format(cond, side, pod_namespace)
            sides.append(cond)
        where.append("(" + " OR ".join(sides) + ")")   # the pod SQL has no time-window predicate (:556-565)
    else:
        if start_time:
            where.append("flowStartSeconds >= '{}'".format(start_time))
        if end_time:
            where.append("flowEndSeconds < '{}'".format(end_time))
        if mode == "external":
            where.append("flowType = 3")
            if external_ip:
                where.append("destinationIP = '{}'".format(external_ip))
        elif mode == "svc":
            where.append("destinationServicePortName = '{}'".format(svc_port_name) if svc_port_name
                         else "destinationServicePortName <> ''")
    columns = list(_RAW_COLUMNS[mode])
    if dictionary:
        # only what prepare_columns_device reads: pod mode has no time filter (flowStartSeconds unused) and keys on names OR labels; the
        # other modes need flowStartSeconds for the start_time filter (mode None: it is part of the key) and the namespaces for ns-ignore
        if mode == "pod":
            by_name = bool(pod_name) and not pod_label
            columns = [c for c in columns if c != "flowStartSeconds" and not c.endswith("PodName" if not by_name else "PodLabels")]
        else:
            if not start_time and mode != "":
                columns = [c for c in columns if c != "flowStartSeconds"]
            if not ns_ignore_list:
                columns = [c for c in columns if not c.endswith("PodNamespace")]
        columns = ["toLowCardinality({0}) AS {0}".format(c) if c in STRING_COLUMNS else c for c in columns]
    if shard is not None and not count_only:
        where.append("{} = {}".format(shard_expr(mode, shard[1]), int(shard[0])))
    if count_only:
        sql = "SELECT {} AS shard, count() AS rows FROM {}".format(shard_expr(mode, shard[1]), FLOWS_TABLE)
    else:
        sql = "SELECT {} FROM {}".format(", ".join(columns), FLOWS_TABLE)
    if where:
        sql += " WHERE " + " AND ".join(where)
    if count_only:
        sql += " GROUP BY shard"
    return sql


def stream_rows_query(agg_flow, pod_ident="labels", ns_ignore_list=(), from_t=0, to_t=0, dictionary=False):
    """SELECT of the raw rows a StreamingAnomalyDetection(agg_flow, pod_ident, ns_ignore_list) reads in `feed`, for the seconds
    from_t <= flowEndSeconds < to_t (epoch seconds; 0 = no bound on that side): the rows of a `poll`.  The WHERE clause is the instance's
    ROW predicates — the namespace ignore list, flowType = 3 in external mode, the `<> ''` rule of the mode's key column (pod mode: a row
    stays when either side passes, the feed tests each side again) — and the range.  No key filter (the jobs select keys on the
    device) and no flowStartSeconds test (the state holds flowEndSeconds alone).  Only the columns `feed` reads are selected;
    dictionary: the string columns as `toLowCardinality(c) AS c`, for a read with DICTIONARY_SETTINGS."""
    if agg_flow not in ("pod", "external", "svc"):
        raise ValueError("aggregated flow type should be 'pod' or 'external' or 'svc'")
    if pod_ident not in ("labels", "name"):
        raise ValueError("pod_ident should be 'labels' or 'name'")
    from_t, to_t = int(from_t), int(to_t)
    where = []
    if ns_ignore_list:
        quoted = ", ".join("'{}'".format(x) for x in ns_ignore_list)
        where.append("sourcePodNamespace NOT IN ({0}) AND destinationPodNamespace NOT IN ({0})".format(quoted))
    namespaces = ["sourcePodNamespace", "destinationPodNamespace"]
    if agg_flow == "pod":
        ident = "PodName" if pod_ident == "name" else "PodLabels"
        where.append("(destination{0} <> '' OR source{0} <> '')".format(ident))
        columns = namespaces + ["source" + ident, "destination" + ident]
    elif agg_flow == "external":
        where.append("flowType = 3")
        columns = ["destinationIP", "flowType"] + (namespaces if ns_ignore_list else [])
    else:
        where.append("destinationServicePortName <> ''")
        columns = ["destinationServicePortName"] + (namespaces if ns_ignore_list else [])
    if from_t:
        where.append("flowEndSeconds >= toDateTime({})".format(from_t))
    if to_t:
        where.append("flowEndSeconds < toDateTime({})".format(to_t))
    columns += ["flowEndSeconds", "throughput"]
    if dictionary:
        columns = ["toLowCardinality({0}) AS {0}".format(c) if c in STRING_COLUMNS else c for c in columns]
    return "SELECT {} FROM {} WHERE {}".format(", ".join(columns), FLOWS_TABLE, " AND ".join(where))


def stream_rows_columns(agg_flow, pod_ident="labels", ns_ignore_list=()):
    """the column names stream_rows_query selects, in its order (an empty read still needs them)"""
    sql = stream_rows_query(agg_flow, pod_ident, ns_ignore_list)
    return sql[len("SELECT "):sql.index(" FROM ")].split(", ")


def fetch_flows(client, start_time="", end_time="", ns_ignore_list=(), agg_flow="", pod_label="", external_ip="",
                svc_port_name="", pod_name="", pod_namespace="", engine=None):
    """Raw-rows read: the column dict theia_amd.anomaly_detection.prepare_columns expects.  With `engine` the string columns are
    dictionary-encoded on the GPU (tad_encode_strings)."""
    kw = {"engine": engine} if engine is not None else {}
    flows = client.query_columns(rows_query(start_time, end_time, list(ns_ignore_list), agg_flow, pod_label, external_ip,
                                            svc_port_name, pod_name, pod_namespace), dict_strings=True, **kw)
    if not flows:   # empty result: ArrowStream carries no batch
        mode = agg_flow if agg_flow in ("pod", "external", "svc") else ""
        flows = {c: np.zeros(0, dtype=np.int64 if c.endswith("Seconds") or c in ("flowType", "throughput") else str)
                 for c in _RAW_COLUMNS[mode]}
    if "throughput" in flows:
        flows["throughput"] = np.asarray(flows["throughput"]).astype(np.uint64)
    return flows


class DeviceDictColumn:
    """A string column on the device: codes int64[n] in HBM (DeviceArray) + the distinct values on the host (numpy str[D]).  What
    fetch_flows_device delivers for every string column; theia_amd.anomaly_detection.prepare_columns_device evaluates the SQL's predicates
    on `values` and applies them to the rows with tad_mask_rows."""

    def __init__(self, codes, values):
        self.codes = codes
        self.values = np.asarray(values).astype(str)

    def __len__(self):
        return self.codes.n


class _Vocabulary:
    """The job-wide dictionary of one string column, shared by the reader threads: a record batch's dictionary (its distinct values) is
    mapped into it with one vectorised lookup; values it has not seen are appended in order of appearance."""

    def __init__(self):
        import threading
        import pyarrow as pa
        self.arr = pa.array([], pa.string())
        self.lock = threading.Lock()

    @property
    def values(self):
        return self.arr.to_pylist()

    def remap(self, batch_dictionary):
        """pyarrow string array (the batch's dictionary, nulls read as '') -> int64[len]: position of every value in the job-wide dictionary"""
        import pyarrow as pa
        import pyarrow.compute as pc
        d = batch_dictionary.fill_null("")
        with self.lock:
            pos = pc.index_in(d, value_set=self.arr) if len(self.arr) else pa.nulls(len(d), pa.int32())
            if pos.null_count:
                self.arr = pa.concat_arrays([self.arr, pc.unique(d.filter(pc.is_null(pos)))])
                pos = pc.index_in(d, value_set=self.arr)
        return np.ascontiguousarray(pos.to_numpy(zero_copy_only=False), dtype=np.int64)


def fetch_flows_device(client, engine, start_time="", end_time="", ns_ignore_list=(), agg_flow="", pod_label="", external_ip="",
                       svc_port_name="", pod_name="", pod_namespace="", connections=8, pinned=None, timings=None):
    """The raw-rows read, straight into HBM (the reference pulls the GROUP BY result through ONE JDBC connection,
    anomaly_detection.py:655-662 — its own bottleneck, not reproduced):

      * `connections` parallel reads, read g taking the rows with `cityHash64(...) % G = g` (rows_query(shard=...)); one count query
        first gives every read its place in the device columns, so the readers write disjoint row ranges and nothing is concatenated;
      * string columns as Arrow DICTIONARY arrays (toLowCardinality + DICTIONARY_SETTINGS): per record batch the host looks at the
        batch's dictionary only (_Vocabulary.remap), the rows' indices go to the device as they are and become job-wide codes there
        (tad_widen_column with the batch's remap as table);
      * every response is received into ONE buffer (page-locked when `pinned`: a pool kept by the client between jobs) and parsed in
        place — Arrow IPC is zero-copy over a buffer — so the column buffers are copied host -> device exactly once.

    Returns {column: DeviceArray (8-byte integers) | DeviceDictColumn} with `n` rows, in shard-major row order.  Raises if the table
    changed between the count and the reads (the caller falls back to fetch_flows)."""
    import threading
    import time
    import pyarrow as pa
    import pyarrow.ipc as ipc
    from .engine import DeviceArray, HostBuffer
    G = max(1, int(connections))
    args = (start_time, end_time, list(ns_ignore_list), agg_flow, pod_label, external_ip, svc_port_name, pod_name, pod_namespace)
    t_begin = time.perf_counter()
    counts = client.query_columns(rows_query(*args, dictionary=True, shard=(None, G), count_only=True))
    rows_of = np.zeros(G, dtype=np.int64)
    if counts:
        rows_of[np.asarray(counts["shard"]).astype(np.int64)] = np.asarray(counts["rows"]).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(rows_of)])
    n = int(offsets[-1])
    sql0 = rows_query(*args, dictionary=True, shard=(0, G))
    names = [c.split(" AS ")[-1] for c in sql0[len("SELECT "):sql0.index(" FROM ")].split(", ")]
    is_string = {c: c in STRING_COLUMNS for c in names}
    columns = {c: DeviceArray(engine, max(n, 1), np.int64 if c != "throughput" else np.uint64) for c in names}
    for c in columns.values():
        c.n = n
    vocab = {c: _Vocabulary() for c in names if is_string[c]}
    errors = []
    t_count = time.perf_counter()
    stage = {"read_s": 0.0, "parse_upload_s": 0.0, "bytes": 0}
    lock = threading.Lock()
    pool = client.__dict__.setdefault("_pinned_pool", []) if pinned else None

    def take_buffer(cap):
        if not pinned:
            b = bytearray(max(cap, 1))
            return b, memoryview(b)
        with lock:
            for i, b in enumerate(pool):
                if b.nbytes >= cap:
                    pool.pop(i)
                    return b, b.view
        b = HostBuffer(engine, max(cap, 1))
        return b, b.view

    def read_body(resp):
        """the whole response body in ONE buffer (page-locked when asked): (memoryview of the body, its owner)"""
        length = resp.headers.get("Content-Length")
        buf, view = take_buffer(int(length) if length is not None else (64 << 20))
        got = 0
        while True:
            if got == len(view):
                if length is not None:
                    break
                nbuf, nview = take_buffer(2 * len(view))      # chunked transfer and the guess was too small
                nview[:got] = view[:got]
                if pinned:
                    with lock:
                        pool.append(buf)
                buf, view = nbuf, nview
            k = resp.readinto(view[got:])
            if not k:
                break
            got += k
        return view[:got], buf

    def reader(g):
        try:
            t0 = time.perf_counter()
            settings = dict(DICTIONARY_SETTINGS)
            with client._request(settings, (rows_query(*args, dictionary=True, shard=(g, G)) + " FORMAT ArrowStream").encode()) as resp:
                body, owner = read_body(resp)
            t1 = time.perf_counter()
            at = int(offsets[g])
            end = int(offsets[g + 1])
            if len(body):
                for batch in ipc.open_stream(pa.py_buffer(body)):
                    k = batch.num_rows
                    if at + k > end:
                        raise RuntimeError("shard %d of %d delivered more rows than its count query announced (%d)" % (g, G, end - int(offsets[g])))
                    for name, col in zip(batch.schema.names, batch.columns):
                        if name not in columns:
                            continue
                        t = col.type
                        if pa.types.is_dictionary(t):
                            idx = col.indices
                            if idx.null_count:
                                raise RuntimeError("column %s: null dictionary indices" % name)
                            d = col.dictionary
                            if not pa.types.is_string(d.type):
                                d = d.cast(pa.string())
                            table = DeviceArray.from_host(engine, vocab[name].remap(d))
                            bits = idx.type.bit_width
                            engine.widen_into(columns[name], at, idx.buffers()[1].address + idx.offset * (bits // 8), bits,
                                              pa.types.is_signed_integer(idx.type), k, table=table)
                            table.free()
                        elif is_string[name]:      # a server that ignored the dictionary settings: encode on the GPU, map like a batch dictionary
                            codes, first = engine.encode_strings(col)
                            dvals = col.take(pa.array(first.astype(np.int64))).fill_null("")
                            table = DeviceArray.from_host(engine, vocab[name].remap(dvals))
                            engine.widen_into(columns[name], at, codes.ctypes.data, 64, True, k, table=table)
                            table.free()
                        else:
                            if pa.types.is_timestamp(t) or pa.types.is_date(t):
                                col = col.cast(pa.timestamp("s")).cast(pa.int64()) if not (pa.types.is_timestamp(t) and t.unit == "s") else col.cast(pa.int64())
                                t = col.type
                            if col.null_count:
                                raise RuntimeError("column %s: nulls in an integer column" % name)
                            bits = t.bit_width
                            engine.widen_into(columns[name], at, col.buffers()[1].address + col.offset * (bits // 8), bits,
                                              pa.types.is_signed_integer(t), k)
                    at += k
            if at != end:
                raise RuntimeError("shard %d of %d delivered %d rows, its count query announced %d" % (g, G, at - int(offsets[g]), end - int(offsets[g])))
            t2 = time.perf_counter()
            with lock:
                stage["read_s"] = max(stage["read_s"], t1 - t0)
                stage["parse_upload_s"] = max(stage["parse_upload_s"], t2 - t1)
                stage["bytes"] += len(body)
                if pinned:
                    pool.append(owner)
        except Exception as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=reader, args=(g,)) for g in range(G)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        for c in columns.values():
            c.free()
        raise errors[0]
    out = {}
    for c in names:
        if is_string[c]:
            vals = vocab[c].values
            out[c] = DeviceDictColumn(columns[c], np.asarray(vals, dtype=object).astype(str) if vals else np.zeros(0, dtype=str))
        else:
            out[c] = columns[c]
    if timings is not None:
        timings.update({"count_query_s": t_count - t_begin, "slowest_read_s": stage["read_s"], "slowest_parse_upload_s": stage["parse_upload_s"],
                        "total_s": time.perf_counter() - t_begin, "bytes": stage["bytes"], "rows": n, "connections": G})
    return out


def fetch_points(client, sql, agg_flow="", pod_name=""):
    """Pushdown read: run the reference's GROUP BY SQL, return the aggregated points as a column dict shaped like raw
    rows, so that prepare_columns / tad_run treat them as (already aggregated) rows.  The aggregate column
    `max(throughput)` / `sum(throughput)` becomes `throughput`."""
    cols = client.query_columns(sql)
    for agg in ("max(throughput)", "sum(throughput)"):
        if agg in cols:
            cols["throughput"] = np.asarray(cols.pop(agg)).astype(np.uint64)
    if agg_flow == "pod" and cols:
        # the SQL already produced (podNamespace, podLabels | podName, direction): present them as the inbound /
        # outbound halves prepare_columns looks for, a row belonging to exactly one half
        ident = "podName" if "podName" in cols else "podLabels"
        inbound = np.asarray(cols["direction"]).astype(str) == "inbound"
        ns, idv = np.asarray(cols["podNamespace"]).astype(str), np.asarray(cols[ident]).astype(str)
        tail = ident[3:]   # Name | Labels
        miss = "\x00not-this-side"   # never equals a pod name, never matches a label pattern ... and is not ''
        cols["destinationPodNamespace"] = np.where(inbound, ns, "")
        cols["sourcePodNamespace"] = np.where(inbound, "", ns)
        cols["destinationPod" + tail] = np.where(inbound, idv, miss if tail == "Name" else "")
        cols["sourcePod" + tail] = np.where(inbound, miss if tail == "Name" else "", idv)
        other = "Labels" if tail == "Name" else "Name"
        cols["destinationPod" + other] = np.full(ns.size, "")
        cols["sourcePod" + other] = np.full(ns.size, "")
        cols["flowStartSeconds"] = np.asarray(cols["flowEndSeconds"], dtype=np.int64)
    return cols
