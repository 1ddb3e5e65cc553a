"""Host-side mirror of the reference's abnormal-traffic-drop UDF, computed on the MI355X engine.

Reference: /root/reference/snowflake/udfs/udfs/drop_detection/drop_detection_udf.py (cited as `ref:`) — a Snowflake UDTF
partitioned by (endpoint, direction): `process` collects (date, drop_number) pairs (ref:25-40), `end_partition` yields one
row per anomalous day (ref:42-56).  Same class and method names here; `end_partition` calls tad_series_drop through the C
ABI, `drop_detection_table` runs every partition of an aggregated table in ONE tad_run (algo DROP).  No CPU fallback.
`PeriodicalDropDetection` is the "periodical" job the reference names and does not have (snowflake/cmd/dropDetection.go:282): the
partitions' daily counts live in a streaming state on the device, a feed judges the new days against everything kept.
`drop_detection_from_flows` and `PeriodicalDropDetection.feed_flows` start one step earlier, from the flow rows themselves: the query
that dropDetection.go:36-190 builds runs on the device (TadEngine.drop_select, then factorize / the key dictionary and Stage 0's sum).
Only the UDTF's call protocol is mirrored (a thin adaptor); the reference's Result helper class is not reproduced.
"""
import datetime
import uuid

import numpy as np

from . import anomaly_detection as _ad


RESULT_COLUMNS = ("job_type", "detection_id", "time_created", "endpoint", "direction", "avg_drop", "stdev_drop",
                  "anomaly_drop_date", "anomaly_drop_number")      # the UDTF's output row (ref:6-19, 55-56)


class DropDetection:
    """Thin adaptor with the UDTF's call protocol (ref:21-56: one instance per (endpoint, direction) partition,
    `process` once per row, `end_partition` yields the anomalous days as RESULT_COLUMNS tuples).  The partition's
    statistics and verdicts come from the engine (tad_series_drop); nothing is computed here."""

    def __init__(self, engine=None):
        self._engine = engine
        self._partition = None            # (job_type, detection_id, endpoint, direction), constant within a partition
        self._dates, self._drops = [], []

    def process(self, job_type, detection_id, endpoint, direction, date, drop_number):
        if job_type != "initial":         # ref:33
            raise AssertionError("drop detection supports job_type 'initial' only")
        self._partition = (job_type, detection_id, endpoint, direction)
        self._dates.append(date)
        self._drops.append(int(drop_number))
        yield None

    def end_partition(self):
        if len(self._drops) < 3:          # ref:44-45
            return
        out = (self._engine or _ad.get_engine()).series_drop(self._drops)
        if out is None:
            return
        mean, std, verdict = out
        job_type, detection_id, endpoint, direction = self._partition
        for i in np.flatnonzero(verdict):   # a fresh id PER ROW when none was given, as Result.__init__ does (ref:8-11)
            yield (job_type, detection_id or str(uuid.uuid4()), datetime.datetime.now(), endpoint, direction, mean, std,
                   self._dates[i], self._drops[i])


def drop_detection_table(endpoint, direction, date, drop_number, detection_id=None, job_type="initial", engine=None):
    """All partitions at once: columns of the `aggregated_flows` CTE (snowflake/cmd/dropDetection.go:151-162) ->
    list of result tuples in (endpoint, direction, date) order.  `date` may be strings (YYYY-MM-DD) or day numbers."""
    import pandas as pd
    endpoint, direction = np.asarray(endpoint).astype(str), np.asarray(direction).astype(str)
    codes, uniq = pd.MultiIndex.from_arrays([endpoint, direction]).factorize()
    d = np.asarray(date)
    if d.dtype.kind in "USO":
        day = np.asarray(pd.to_datetime(d).values.astype("datetime64[D]").astype(np.int64))
    else:
        day = d.astype(np.int64)
    eng = engine or _ad.get_engine()
    # one lattice bucket per day; Stage 0 sums the drop numbers of equal (key, day)
    res = eng.run("DROP", codes.astype(np.uint64), day, np.asarray(drop_number, dtype=np.uint64), max(len(uniq), 1),
                  agg_flow="svc", value_op="sum")
    now = datetime.datetime.now()
    host = res.to_host()
    rows = []
    for k, t, x, mean, std in zip(host["key_id"].tolist(), host["flow_end_s"].tolist(), host["throughput"].tolist(),
                                  host["algo_calc"].tolist(), host["stddev"].tolist()):
        ep, di = uniq[int(k)]
        dd = str(np.datetime64(int(t), "D")) if d.dtype.kind in "USO" else int(t)
        rows.append((job_type, detection_id or str(uuid.uuid4()), now, ep, di, mean, std, dd, int(x)))   # (ref:8-11: id per row)
    return rows


FLOW_COLUMNS = ("ingress_action", "egress_action", "flow_start_s", "src_ip", "src_pod_ns", "src_pod_name", "dst_ip", "dst_pod_ns", "dst_pod_name")
DIRECTIONS = ("ingress", "egress")


def _select_flows(engine, columns, dictionaries, start_time, end_time, keep):
    """TadEngine.drop_select over a dict of flow columns; the pod-name code that means "no pod" is the dictionary's '' unless the
    columns name one (src_pod_null / dst_pod_null)"""
    names = list(dictionaries["pod_name"])
    null = names.index("") if "" in names else -1
    return engine.drop_select(*[columns[c] for c in FLOW_COLUMNS], flow_end_s=columns.get("flow_end_s"),
                              src_pod_null=columns.get("src_pod_null", null), dst_pod_null=columns.get("dst_pod_null", null),
                              start_time=start_time, end_time=end_time, keep=keep, out="device")


def _decode_keys(engine, rows, first, dictionaries):
    """the (endpoint, direction) strings of the keys whose first rows (into `rows`) are `first`: ns/name for a pod, the IP otherwise"""
    kind, ns, name, direction = (engine.gather(c, first).tolist() for c in rows.tuple_columns())
    ips, nss, pods = dictionaries["ip"], dictionaries["pod_ns"], dictionaries["pod_name"]
    return [("%s/%s" % (nss[n], pods[m]) if k else str(ips[m]), DIRECTIONS[d]) for k, n, m, d in zip(kind, ns, name, direction)]


def drop_detection_from_flows(engine, columns, dictionaries, start_time=0, end_time=0, keep=None, detection_id=None, job_type="initial"):
    """The drop job from flow rows to result rows on the device.  columns: dict of the flow table's columns (FLOW_COLUMNS, optionally
    flow_end_s, src_pod_null, dst_pod_null) — uint8 rule actions, epoch-second times and int64 dictionary codes, numpy arrays or
    DeviceArrays; dictionaries: {"ip": [...], "pod_ns": [...], "pod_name": [...]}, code -> string.  start_time / end_time / keep: the
    query's flowStartSeconds >=, flowEndSeconds < and clusterUUID predicates (keep: one byte per row, e.g. TadEngine.mask_rows').
    drop_select -> factorize over (kind, ns, name, direction) -> run("DROP", value_op="sum") over (key id, day, 1): the rows
    drop_detection_table returns for the query's aggregated counts, in (key by first appearance among the dropped rows, date) order."""
    eng = engine or _ad.get_engine()
    rows = _select_flows(eng, columns, dictionaries, start_time, end_time, keep)
    if rows.n_rows == 0:
        return []
    key, _, first = eng.factorize(rows.tuple_columns())
    keys = _decode_keys(eng, rows, first, dictionaries)
    res = eng.run("DROP", key, rows["day_s"], rows["count"], max(len(keys), 1), agg_flow="svc", value_op="sum")
    now = datetime.datetime.now()
    host = res.to_host()
    out = []
    for k, t, x, mean, std in zip(host["key_id"].tolist(), host["flow_end_s"].tolist(), host["throughput"].tolist(),
                                  host["algo_calc"].tolist(), host["stddev"].tolist()):
        ep, di = keys[int(k)]
        out.append((job_type, detection_id or str(uuid.uuid4()), now, ep, di, mean, std, str(np.datetime64(int(t), "s").astype("datetime64[D]")), int(x)))
    return out


def _days(date):
    """dates (YYYY-MM-DD strings, datetime64 or day numbers) -> (int64 day numbers, whether they were dates)"""
    import pandas as pd
    d = np.asarray(date)
    if d.dtype.kind in "USOM":
        return np.asarray(pd.to_datetime(d).values.astype("datetime64[D]").astype(np.int64)), True
    return d.astype(np.int64), False


class PeriodicalDropDetection:
    """The periodical drop job: `feed` adds a batch of (endpoint, direction, date, drop_number) rows — the new days — and returns the
    anomalous ones among them, judged against every day fed so far (mean and std over the partition's whole series, as an "initial"
    job over the concatenation would compute them); `window` returns the verdicts of a range of days of what is kept.  Owns a series +
    times state on the engine (TadEngine.drop_stream / drop_state) and the (endpoint, direction) -> key id table, ids in order of first
    appearance; the state is resized as partitions appear.  A partition's days must arrive in order: a feed with a day that is not
    newer than the partition's newest fails as a whole and changes nothing — unless the feed is made with partial=True, which adds the
    counts to the days the state holds and judges the changed partitions again from their first changed day on (TadEngine
    .merge_stream_changes + drop_state_since).  Nothing is computed on the host."""

    def __init__(self, engine=None):
        self._engine = engine or _ad.get_engine()
        self._ids = {}                    # (endpoint, direction) -> key id
        self._keys = []                   # key id -> (endpoint, direction)
        self._state = None
        self._dates = False               # the feeds carried dates (rows report dates) or day numbers
        self._seconds = False             # the state's times are epoch seconds (feed_flows) rather than day numbers (feed)
        self._dict = None                 # feed_flows: the (kind, ns, name, direction) -> key id dictionary on the device
        self._namespaces = []             # feed_flows: the namespace dictionary of the newest feed (code -> string)

    @property
    def state(self):
        return self._state

    def _key_ids(self, endpoint, direction):
        out = np.empty(len(endpoint), dtype=np.uint64)
        for i, key in enumerate(zip(endpoint.tolist(), direction.tolist())):
            k = self._ids.get(key)
            if k is None:
                k = self._ids[key] = len(self._keys)
                self._keys.append(key)
            out[i] = k
        return out

    def _rows(self, res, job_type, detection_id):
        now = datetime.datetime.now()
        host = res.to_host()
        rows = []
        for k, t, x, mean, std in zip(host["key_id"].tolist(), host["flow_end_s"].tolist(), host["throughput"].tolist(),
                                      host["algo_calc"].tolist(), host["stddev"].tolist()):
            ep, di = self._keys[int(k)]
            if self._seconds:
                dd = str(np.datetime64(int(t), "s").astype("datetime64[D]"))
            else:
                dd = str(np.datetime64(int(t), "D")) if self._dates else int(t)
            rows.append((job_type, detection_id or str(uuid.uuid4()), now, ep, di, mean, std, dd, int(x)))
        return rows

    def _judge(self, key, day, count, partial, detection_id):
        """the batch into the state, and its rows.  Whole days (the default): drop_stream, which refuses a day that is not newer than its
        partition's newest.  partial: the counts are ADDED to what the state holds for their days (merge_stream_changes with "sum"), and
        drop_state_since judges every changed partition over everything kept and reports its days from the first changed one on — a
        day whose count grew is judged again."""
        eng = self._engine
        if not partial:
            return self._rows(eng.drop_stream(self._state, key, day, count, agg_flow="svc", value_op="sum"), "periodical", detection_id)
        stats = eng.merge_stream_changes(self._state, key, day, count, "device", agg_flow="svc", value_op="sum")
        since = stats["key_since"]
        try:
            if stats["keys_changed"] == 0:
                return []
            res = eng.drop_state_since(self._state, key_since=since)
        finally:
            since.free()
        return self._rows(res, "periodical", detection_id)

    def feed(self, endpoint, direction, date, drop_number, detection_id=None, partial=False):
        """One batch -> its anomalous days as RESULT_COLUMNS tuples with job_type "periodical", in (partition, date) order.
        partial=True: the batch may hold PART of a day's drops, and a day may be split over any number of feeds, in any order: the
        counts add up, and the feed returns the anomalous days among each changed partition's days from its first changed day on,
        judged over everything kept.  A partition's earlier days are not reported again (their verdicts may have moved with the
        partition's mean and std: `window` gives the whole answer)."""
        if self._dict is not None:
            raise ValueError("this instance is fed flow rows (feed_flows): its key ids come from the device dictionary")
        endpoint, direction = np.asarray(endpoint).astype(str), np.asarray(direction).astype(str)
        day, self._dates = _days(date)
        key = self._key_ids(endpoint, direction)
        n_keys = max(len(self._keys), 1)
        if self._state is None:
            self._state = self._engine.state_create(n_keys, series=True, times=True)
        elif n_keys > self._state.num_keys:
            self._state.resize(n_keys)
        return self._judge(key, day, np.asarray(drop_number, dtype=np.uint64), partial, detection_id)

    def feed_flows(self, columns, dictionaries, start_time=0, end_time=0, keep=None, detection_id=None, partial=False):
        """One batch of FLOW ROWS -> its anomalous days, as `feed` returns them for the batch's aggregated counts: drop_select -> this
        instance's key dictionary (KeyDict over kind, ns, name, direction: ids stay the same from feed to feed) -> drop_stream with
        value_op="sum" over (key id, day, 1).  columns / dictionaries / start_time / end_time / keep: as drop_detection_from_flows; the
        dictionaries must keep their codes from feed to feed (they may grow).  By default a feed must hold WHOLE DAYS: the stream judges
        a day when it arrives, so a day split over two feeds is a late row in the second and that feed is refused as a whole, as `feed`
        refuses it.  partial=True takes a day in any number of feeds, as `feed` with partial=True does.  An instance is fed either
        counts (`feed`) or flow rows, not both; dates come back as YYYY-MM-DD."""
        if self._keys and self._dict is None:
            raise ValueError("this instance is fed daily counts (feed): its key ids come from the host table")
        eng = self._engine
        rows = _select_flows(eng, columns, dictionaries, start_time, end_time, keep)
        if rows.n_rows == 0:
            return []
        if self._dict is None:
            self._dict = eng.key_dict(4)
        self._dates = self._seconds = True
        self._namespaces = [str(x) for x in dictionaries["pod_ns"]]
        key, _, first, _ = self._dict.encode(rows.tuple_columns())
        self._keys += _decode_keys(eng, rows, first, dictionaries)
        n_keys = max(len(self._keys), 1)
        if self._state is None:
            self._state = eng.state_create(n_keys, series=True, times=True)
        elif n_keys > self._state.num_keys:
            self._state.resize(n_keys)
        return self._judge(key, rows["day_s"], rows["count"], partial, detection_id)

    def window(self, from_date=None, to_date=None, detection_id=None, direction=None, namespace=None):
        """The anomalous days with from_date <= date < to_date (None = no bound) of everything kept, each partition judged over its days
        inside the range: the rows of an "initial" job over those days.  direction ("ingress" / "egress") and namespace (the pod
        endpoints of that namespace) narrow the job to the partitions they name — an instance fed flow rows only: the partitions are
        selected on its (kind, ns, name, direction) dictionary (KeyDict.select) and only they are judged (TadEngine.drop_state_keys);
        the rows are those of the unfiltered call for these partitions."""
        if (direction is not None or namespace is not None) and self._dict is None and (self._keys or self._state is not None):
            raise ValueError("direction / namespace select partitions on the device dictionary of an instance fed flow rows (feed_flows); "
                             "this one is fed daily counts (feed)")
        if direction is not None and direction not in DIRECTIONS:
            raise ValueError("direction should be 'ingress' or 'egress'")
        if self._state is None:
            return []
        bound = lambda d: 0 if d is None else int(_days([d])[0][0]) * (86400 if self._seconds else 1)
        if direction is None and namespace is None:
            res = self._engine.drop_state(self._state, bound(from_date), bound(to_date))
            return self._rows(res, "periodical", detection_id)
        terms = []
        if direction is not None:
            terms.append((3, np.arange(2) == DIRECTIONS.index(direction)))
        if namespace is not None:          # a pod endpoint (kind 1) whose namespace code names this string
            terms += [(0, np.array([0, 1], np.uint8)), (1, np.asarray([s == namespace for s in self._namespaces], dtype=np.uint8))]
        keep, _ = self._dict.select(terms, out="device")
        res = self._engine.drop_state_keys(self._state, keep, bound(from_date), bound(to_date))
        return self._rows(res, "periodical", detection_id)
