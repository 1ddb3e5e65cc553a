"""Throughput anomaly detection on a long-lived streaming state: the TAD twin of drop_detection.PeriodicalDropDetection.

`anomaly_detection` (anomaly_detection.py) answers one job from the flow table: it reads the rows, applies the job's filters and runs
the batch job.  A `StreamingAnomalyDetection` is fed the flow rows as they arrive — in any order — and answers the same jobs from what it
keeps on the device: a key dictionary (KeyDict: the mode's key tuples -> stable ids), a series state (TadState with history and times,
fed through TadEngine.merge_stream, or TadEngine.replace_stream for a re-read: `feed(flows, replace=...)`, `poll`) and one string dictionary per string key column (StringDict: strings -> stable codes, in HBM as
well).  Nothing grows on the host: a job's result rows name key ids, and those ids alone are decoded — KeyDict.gather gives their code
tuples, StringDict.decode the codes' strings (_KeyColumn) — so `snapshot()` / `restore()` of the three device structures is all a restart
needs.  `retire(idle_before)` keeps all three bounded: it drops the idle keys from the state and the key dictionary and the strings no
surviving key uses from the string dictionaries, on the device, so an instance can run indefinitely.

The job's name filters (--pod-name, --pod-namespace, --pod-label, --external-ip, --svc-port-name) are predicates on KEY columns of the
mode, so a job is a key selection: the filter is evaluated once per distinct string of the vocabulary, on the device (StringDict.match:
equality, and ilike '%label%' as a case-folded substring search; StringDict.like: a label with the LIKE wildcards % and _ or an
escape), KeyDict.select turns the vocabulary masks into a key mask there, and
TadEngine.run_state_keys judges the selected keys only.  The predicates that are NOT key predicates — the namespace ignore list (it tests
both namespaces of a row), flowType = 3 in external mode, the `<> ''` rules — are applied to the rows in `feed`, before they reach the
state.  Mode None (no aggregation) has no key filter to serve and is not offered.
"""
import numpy as np

from . import _capi
from . import anomaly_detection as _ad
from .engine import TadError

MODES = ("svc", "external", "pod")


def _arrow(strings):
    """a numpy array of str -> (offsets int64[n + 1], data uint8[...]): the column in Arrow's layout, UTF-8"""
    raw = np.char.encode(np.asarray(strings).astype(str), "utf-8")
    offsets = np.zeros(raw.size + 1, dtype=np.int64)
    np.cumsum(np.char.str_len(raw), out=offsets[1:])
    return offsets, np.frombuffer(b"".join(raw.tolist()), dtype=np.uint8)


def _strings(flows, name):
    c = _ad._str_col(flows, name)
    return c.materialise() if isinstance(c, _ad.DictColumn) else c


def _encode(vocab, flows, name):
    """the rows' codes (int64[n], host) of a string column through its StringDict: a DictColumn is encoded through its distinct values
    and mapped, a plain column goes to the device as it is.  No string is hashed or compared on the host."""
    c = _ad._str_col(flows, name)
    if isinstance(c, _ad.DictColumn):
        if not c.values.size:
            return np.zeros(c.codes.size, dtype=np.int64)
        return vocab.encode(_arrow(c.values))[0][c.codes]
    return vocab.encode(_arrow(c))[0]


def _code_of(vocab, s):
    """the code the dictionary holds for s, or -1"""
    return int(vocab.lookup(_arrow([s]))[0])


def _strings_of(offsets, data):
    """a decoded column (Arrow's layout, UTF-8) -> an object array of str"""
    n = offsets.size - 1
    try:
        import pyarrow as pa
    except ImportError:      # the same strings, one slice at a time
        raw, vals = data.tobytes(), np.empty(n, dtype=object)
        vals[:] = [raw[a:b].decode("utf-8") for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]
        return vals
    return pa.Array.from_buffers(pa.large_string(), n, [None, pa.py_buffer(offsets), pa.py_buffer(data)]).to_numpy(zero_copy_only=False)


def _release(x):
    """free a DeviceArray now — for a view, the array it is a slice of"""
    base = x._base
    x.free()
    if base is not None:
        base.free()


class _KeyDecoder:
    """What a job's key table shares: one KeyDict.gather of the unique ids the result rows name (the code tuples stay on the device) and
    one StringDict.decode per string column, made when the first column is asked and kept for the others."""

    def __init__(self, key_dict, vocab):
        self.key_dict, self.vocab = key_dict, vocab
        self._kid = self._cols = None

    def columns(self, kid):
        """kid: the rows' key ids -> [the strings of key column 0, of column 1, ..., the sides], one entry per row"""
        kid = np.ascontiguousarray(np.asarray(kid).astype(np.uint64))
        if self._kid is None or self._kid.shape != kid.shape or not np.array_equal(self._kid, kid):
            if kid.size < 2 or bool((kid[1:] >= kid[:-1]).all()):      # every key once (a key has many result rows); rows in key order need no sort
                first = np.ones(kid.size, dtype=bool)
                first[1:] = kid[1:] != kid[:-1]
                uniq, inv = kid[first], np.cumsum(first) - 1
            else:
                uniq, inv = np.unique(kid, return_inverse=True)
            codes, side = self.key_dict.gather(uniq, out="device")
            cols = []
            for c, v in zip(codes, self.vocab):
                cols.append(_strings_of(*v.decode(c, out="host"))[inv])
                c.free()
            cols.append(side.to_host()[inv])
            side.free()
            self._kid, self._cols = kid, cols
        return self._cols


class _KeyColumn:
    """One column of a streaming job's key table, decoded ON DEMAND from the dictionaries on the device — what DeviceKeyColumn is to the
    batch path's device ingest: `col[kid]` gives the column's values for the rows' key ids.  which: the index of a string key column, or
    "direction" (from the key's side: side a = inbound)."""

    def __init__(self, decoder, which):
        self.decoder, self.which = decoder, which

    def __len__(self):
        return self.decoder.key_dict.num_keys()

    def __getitem__(self, kid):
        if np.asarray(kid).size == 0:
            return np.zeros(0, dtype=object)
        cols = self.decoder.columns(kid)
        if self.which == "direction":
            return np.where(cols[-1] == 1, "outbound", "inbound").astype(object)
        return cols[self.which]

    def __array__(self, dtype=None, copy=None):
        a = self[np.arange(len(self), dtype=np.uint64)]
        return a if dtype is None else a.astype(dtype)


class StreamingAnomalyDetection:
    """agg_flow: "svc", "external" or "pod".  pod_ident (pod mode): "labels" keys the pods by (namespace, labels, direction) and serves
    the jobs with --pod-label and the ones without a pod filter; "name" keys them by (namespace, name, direction) and serves the jobs
    with --pod-name — the two key sets of the reference's pod query.  ns_ignore_list is fixed for the instance: it is applied to the
    rows as they are fed.  `job` returns what anomaly_detection returns for the same arguments over all rows fed so far.  One
    difference at the edge: in pod mode the feed drops the rows of a side whose labels / name are '' (the query's `<> ''` rule for a
    job without a pod filter), while the batch query with a pod_label or pod_name filter applies only that filter — so a pattern that
    matches the empty string, such as pod_label='%', finds the '' keys in the batch job and not here.  The label filter runs on the
    device when pod_label is ASCII and free of %, _ and \\ (StringDict.match folds the bytes 'A'..'Z' to 'a'..'z' and nothing else: on
    ASCII strings, which is what Kubernetes allows in labels, exactly ilike '%label%').  Any other ASCII pod_label of at most 1022
    bytes — one with the wildcards % and _ or an escape, such as the documented "test_key":"test_value" — runs on the device as well:
    StringDict.like('%' + pod_label + '%', nocase=True) evaluates the LIKE pattern with the same byte fold.  Only a non-ASCII
    pattern (Unicode case folding) or a longer one is evaluated on the host over the exported label strings, with the regex the
    batch job uses."""

    def __init__(self, engine=None, agg_flow="svc", pod_ident="labels", ns_ignore_list=()):
        if agg_flow not in MODES:
            raise ValueError("aggregated flow type should be 'pod' or 'external' or 'svc'")
        if pod_ident not in ("labels", "name"):
            raise ValueError("pod_ident should be 'labels' or 'name'")
        self._engine = engine or _ad.get_engine()
        self.agg_flow = agg_flow
        self.pod_ident = pod_ident
        self.ns_ignore_list = tuple(ns_ignore_list or ())
        self.mode = ("podname" if pod_ident == "name" else "pod") if agg_flow == "pod" else agg_flow
        self._vocab = [self._engine.string_dict() for _ in range(2 if agg_flow == "pod" else 1)]     # pod: namespaces, labels / names
        self._dict = self._engine.key_dict(len(self._vocab))
        self._state = None
        self.watermark = 0       # poll: the `now` of the last turn (0: no turn yet); carried by snapshot() / restore()
        self._broken = None      # why the instance can no longer be used (retire)
        self._tiers = []         # rollup: (the bound as applied, bucket_s, bucket_op) per tier; carried by snapshot() / restore()

    @property
    def state(self):
        return self._state

    @property
    def num_keys(self):
        return self._dict.num_keys()

    def feed(self, flows, replace=None):
        """One batch of flow rows (a column dict as anomaly_detection takes it), in any order; rows of a (key, flowEndSeconds) group may
        be split over feeds.  Returns the merge's statistics (TadEngine.merge_stream), or None when no row passed the row predicates.

        replace=(from_t, to_t): `flows` are ALL rows of this instance with from_t <= flowEndSeconds < to_t (0 = no bound on that
        side) — a re-read.  They replace what the instance holds for those seconds instead of being added to it
        (TadEngine.replace_stream with ranged=True): feeding the same range again, or an overlapping one, leaves every point once,
        where the default feed would double it.  A re-read in which no row passes the row predicates still erases the range.
        Returns the replace's statistics (None only when there is no state yet and nothing to erase)."""
        return self._feed(flows, replace, None)

    def _feed(self, flows, replace, changes):
        """feed; changes: None, or where the change report of the merge / replace goes (TadEngine.merge_stream_changes)"""
        self._usable()
        if replace is not None:
            self._check_replace(int(replace[0]))
        eng = self._engine
        n = len(flows["flowEndSeconds"])
        if n == 0 and replace is not None:
            return self._erase(replace, changes)
        keep = np.ones(n, dtype=bool)
        if self.ns_ignore_list:
            ign = np.asarray(list(self.ns_ignore_list), dtype=str)
            keep &= ~np.isin(_strings(flows, "sourcePodNamespace"), ign) & ~np.isin(_strings(flows, "destinationPodNamespace"), ign)
        flow_end = np.asarray(flows["flowEndSeconds"], dtype=np.int64)
        value = np.asarray(flows["throughput"], dtype=np.uint64)
        if self.agg_flow == "pod":
            ident = "PodName" if self.pod_ident == "name" else "PodLabels"
            sides = []
            for side in ("destination", "source"):                 # side a = inbound, side b = outbound
                codes = [_encode(self._vocab[0], flows, side + "PodNamespace"), _encode(self._vocab[1], flows, side + ident)]
                sides.append((codes, keep & (codes[1] != _code_of(self._vocab[1], ""))))
            if not (sides[0][1].any() or sides[1][1].any()):
                return self._erase(replace, changes)
            key, key2, _, _ = self._dict.encode(sides[0][0], sides[0][1], sides[1][0], sides[1][1], max_new=0)
        else:
            name = "destinationIP" if self.agg_flow == "external" else "destinationServicePortName"
            codes = _encode(self._vocab[0], flows, name)
            if self.agg_flow == "external":
                keep &= np.asarray(flows["flowType"]).astype(np.int64) == 3
            else:
                keep &= codes != _code_of(self._vocab[0], "")
            if not keep.any():
                return self._erase(replace, changes)
            key, key2, _, _ = self._dict.encode([codes], keep, max_new=0)
        num_keys = self.num_keys
        if self._state is None:
            self._state = eng.state_create(num_keys, history=True, series=True, times=True)
        elif num_keys > self._state.num_keys:
            self._state.resize(num_keys)
        if replace is not None:
            kw = dict(from_t=int(replace[0]), to_t=int(replace[1]), ranged=True, agg_flow=self.agg_flow, key_id2=key2)
            if changes:
                return eng.replace_stream_changes(self._state, key, flow_end, value, changes, **kw)
            return eng.replace_stream(self._state, key, flow_end, value, **kw)
        if changes:
            return eng.merge_stream_changes(self._state, key, flow_end, value, changes, agg_flow=self.agg_flow, key_id2=key2)
        return eng.merge_stream(self._state, key, flow_end, value, agg_flow=self.agg_flow, key_id2=key2)

    def _erase(self, replace, changes=None):
        """a feed without a live row: nothing to merge; a re-read of a range still says that the range holds nothing"""
        if replace is None or self._state is None:
            return None
        none = np.zeros(0, dtype=np.uint64)
        kw = dict(from_t=int(replace[0]), to_t=int(replace[1]), ranged=True, agg_flow=self.agg_flow)
        if changes:
            return self._engine.replace_stream_changes(self._state, none, np.zeros(0, dtype=np.int64), none, changes, **kw)
        return self._engine.replace_stream(self._state, none, np.zeros(0, dtype=np.int64), none, **kw)

    def feed_alerts(self, flows, algo_type, tad_id, replace=None, pod_label="", pod_name="", pod_namespace="", external_ip="", svc_port_name="",
                    bucket_s=0, bucket_op="sum"):
        """feed, and what it made anomalous -> (the feed's statistics with the change report's counters, list of result rows).  The
        feed runs with a change report on the device (TadEngine.merge_stream_changes / replace_stream_changes): per key, the smallest
        flowEndSeconds at which the key's series changed.  Then TadEngine.run_state_since judges the keys that changed AND pass the
        job's name filters (KeyDict.select, as `job`) over everything they hold, and reports every changed key's points from its
        first changed time on.  The rows have `job`'s shape and are decoded on the device as `job`'s are; there is NO sentinel row: no
        anomaly is an empty list.  The same re-read fed twice changes nothing the second time and returns no rows.

        What is not reported: a changed key's points BEFORE its first changed time.  A late point moves the whole key's stddev (and
        DBSCAN's neighbourhoods, ARIMA's lambda), so their verdicts may have changed as well; that is the stream's rule — each point
        once, when it arrives or changes — and `job` gives the whole answer.

        bucket_s > 0: the changed keys are judged per bucket as `job(bucket_s=...)` judges them (TadEngine.run_state_buckets), and
        every changed key's buckets are reported from the one that holds its first changed second on, whole."""
        if algo_type not in _ad.VALID_ALGOS:
            raise ValueError("Algorithm should be in {}".format(" or ".join(_ad.VALID_ALGOS)))
        bucket_s = self._bucket_args(bucket_s, bucket_op)
        self._check_job_buckets(0, bucket_s, bucket_op)      # (the changed keys are judged over everything they hold)
        filters = (pod_label or "", pod_name or "", pod_namespace or "", external_ip or "", svc_port_name or "")
        self._terms(*filters)      # (a filter this instance does not serve is refused before the feed changes anything)
        stats = self._feed(flows, replace, "device")
        if stats is None:
            return None, []
        since = stats.pop("key_since")
        try:
            if stats["keys_changed"] == 0:
                return stats, []
            keep, _ = self._dict.select(self._terms(*filters), out="device")      # (the masks: over the vocabularies as the feed left them)
            if bucket_s:
                res = self._engine.run_state_buckets(self._state, bucket_s, 0, bucket_op, key_keep=keep, key_since=since, algo=algo_type,
                                                     job_id=str(tad_id or ""))
            else:
                res = self._engine.run_state_since(self._state, key_since=since, key_keep=keep, algo=algo_type, job_id=str(tad_id or ""))
        finally:
            since.free()
        if res.n_rows == 0:
            return stats, []
        decoder = _KeyDecoder(self._dict, self._vocab)
        table = {name: _KeyColumn(decoder, "direction" if name == "direction" else i) for i, name in enumerate(_ad.KEY_COLUMNS[self.mode])}
        prep = _ad.PreparedColumns(self.mode, None, None, None, None, None, table, 0, 0)
        return stats, _ad.result_rows(prep, res, algo_type, self.agg_flow, tad_id)

    def poll_alerts(self, client, now, lag_s, algo_type, tad_id, bucket_s=0, bucket_op="sum", **filters):
        """One turn of `poll` that also returns what the turn made anomalous -> (statistics, rows) as feed_alerts: the lagged range is
        re-read and REPLACES those seconds, so a turn made twice (a timeout, a restart) returns no rows the second time.  bucket_s /
        bucket_op: feed_alerts'."""
        return self._poll(client, now, lag_s, lambda flows, replace: self.feed_alerts(flows, algo_type, tad_id, replace=replace, bucket_s=bucket_s,
                                                                                      bucket_op=bucket_op, **filters))

    def poll(self, client, now, lag_s):
        """One turn of the poll loop against the flow table: read the instance's rows with watermark - lag_s <= flowEndSeconds < now
        (clickhouse.stream_rows_query through `client`, a ClickHouseHTTP), feed them with replace, move the watermark to `now`.  The
        exporters lag by node and the table is ordered by insertion time, so rows of the last lag_s seconds may still have been
        missing at the previous turn: they are read again, and because the read REPLACES those seconds a row seen twice counts once.
        The turn is idempotent: after a timeout or a restart (the watermark travels in snapshot() / restore()) it can simply be made
        again.  The first turn reads everything before `now`.  Returns the replace's statistics (None: nothing held, nothing read)."""
        return self._poll(client, now, lag_s, lambda flows, replace: self.feed(flows, replace=replace))

    def _poll(self, client, now, lag_s, feed):
        from . import clickhouse as _ch
        now, lag_s = int(now), int(lag_s)
        if lag_s < 0:
            raise ValueError("lag_s must not be negative")
        from_t = self._floor_to_tiers(max(self.watermark - lag_s, 0))
        if from_t >= now:
            raise ValueError("now (%d) must lie after the watermark less the lag (%d)" % (now, from_t))
        flows = client.query_columns(_ch.stream_rows_query(self.agg_flow, self.pod_ident, list(self.ns_ignore_list), from_t, now), dict_strings=True)
        if not flows:      # an empty result carries no batch
            flows = {c: np.zeros(0, dtype=np.int64 if c.endswith("Seconds") or c in ("flowType", "throughput") else str)
                     for c in _ch.stream_rows_columns(self.agg_flow, self.pod_ident, list(self.ns_ignore_list))}
        flows["throughput"] = np.asarray(flows["throughput"]).astype(np.uint64)
        out = feed(flows, (from_t, now))
        self.watermark = now
        return out

    def _equal(self, col, s):
        return col, self._vocab[col].match(_capi.TAD_STR_EQUAL, s, out="device")[0]

    def _terms(self, pod_label, pod_name, pod_namespace, external_ip, svc_port_name):
        """the job's name filters as (key column, vocabulary mask) terms of KeyDict.select; the masks are computed on the device"""
        if self.agg_flow == "external":
            return [self._equal(0, external_ip)] if external_ip else []
        if self.agg_flow == "svc":
            return [self._equal(0, svc_port_name)] if svc_port_name else []
        by_name = bool(pod_name) and not pod_label
        if by_name != (self.pod_ident == "name"):
            raise ValueError("this instance keys the pods by their %s: it serves jobs %s" %
                             (self.pod_ident, "with pod_name" if self.pod_ident == "name" else "with pod_label or without a pod filter"))
        if pod_label:
            if pod_label.isascii() and not any(c in pod_label for c in "%_\\") and len(pod_label) <= 1024:
                terms = [(1, self._vocab[1].match(_capi.TAD_STR_CONTAINS_NOCASE, pod_label, out="device")[0])]
            elif pod_label.isascii() and len(pod_label) <= 1022:     # %, _ or \ in ASCII text: the whole LIKE pattern on the device
                terms = [(1, self._vocab[1].like("%" + pod_label + "%", nocase=True, out="device")[0])]
            else:                                                  # non-ASCII case folding, or a pattern over the limit: the batch job's regex over the exported labels
                rx = _ad._like_regex("%" + pod_label + "%")
                labels = self._vocab[1].values().to_pylist()
                terms = [(1, np.fromiter((1 if rx.match(s) is not None else 0 for s in labels), dtype=np.uint8, count=len(labels)))]
        elif pod_name:
            terms = [self._equal(1, pod_name)]
        else:
            return []
        if pod_namespace:
            terms.append(self._equal(0, pod_namespace))
        return terms

    @staticmethod
    def _bucket_args(bucket_s, bucket_op):
        bucket_s = int(bucket_s)
        if bucket_s < 0:
            raise ValueError("bucket_s must not be negative")
        if bucket_s and bucket_op not in ("sum", "max"):
            raise ValueError("bucket_op should be 'sum' or 'max'")
        return bucket_s

    # ---- retention: old points folded into time buckets (TadState.rollup) ----
    def rollup(self, before, bucket_s, bucket_op="sum"):
        """Fold everything older than `before` into buckets of bucket_s seconds, on the device (TadState.rollup, origin 0): the instance
        keeps its context at bucket resolution instead of per second, and device_bytes() falls.  `before` is floored to a multiple of
        bucket_s.  Returns the roll-up's statistics (None: nothing held yet).  The instance remembers its tiers — (the bound as applied,
        bucket_s, bucket_op), carried by snapshot() / restore() — and from then on guards what a rolled region cannot answer: `job` (and
        feed_alerts / poll_alerts) over it needs a bucket_s that is a multiple of every tier's it reaches, with that tier's bucket_op;
        feed(replace=(from_t, to_t)) with from_t inside a rolled region must start on that tier's bucket start (a re-read from the middle
        of a bucket would count the bucket's older seconds twice) — `poll` / `poll_alerts` floor their re-read's start to it instead."""
        bucket_s = self._bucket_args(bucket_s, bucket_op)
        if bucket_s < 1:
            raise ValueError("bucket_s must be at least 1")
        self._usable()
        if self._state is None:
            return None
        stats = self._state.rollup(int(before), bucket_s, 0, bucket_op)
        tier = (int(stats["before_t"]), bucket_s, bucket_op)
        same = [i for i, t in enumerate(self._tiers) if t[1:] == tier[1:]]
        if same:      # the same resolution again, further on: one tier
            self._tiers[same[0]] = max(self._tiers[same[0]], tier)
        else:
            self._tiers.append(tier)
        return stats

    @property
    def tiers(self):
        """the roll-ups made so far: [(the bound as applied, bucket_s, bucket_op)]"""
        return list(self._tiers)

    def _tiers_at(self, t):
        """the tiers whose rolled region (everything before their bound) holds the time t (0: before everything)"""
        return [tier for tier in getattr(self, "_tiers", ()) if t < tier[0]]

    def _check_replace(self, from_t):
        if from_t == 0:      # no lower bound: the re-read erases the rolled region with everything else
            return
        for bound, bucket_s, _ in self._tiers_at(from_t):
            if from_t % bucket_s:
                raise ValueError("replace from %d starts inside a bucket of the region rolled up to %d at %d s: a re-read must start on a "
                                 "bucket start there (%d)" % (from_t, bound, bucket_s, from_t // bucket_s * bucket_s))

    def _floor_to_tiers(self, from_t):
        """from_t, moved down to a bucket start of every tier whose rolled region holds it"""
        while from_t:
            low = min([from_t // bucket_s * bucket_s for _, bucket_s, _ in self._tiers_at(from_t)], default=from_t)
            if low == from_t:
                break
            from_t = low
        return from_t

    def _check_job_buckets(self, from_t, bucket_s, bucket_op):
        """a job over a window from from_t (0: the beginning) on: every tier it reaches must divide bucket_s and share bucket_op"""
        for bound, tier_s, tier_op in self._tiers_at(from_t):
            if bucket_s == 0 or bucket_s % tier_s or bucket_op != tier_op:
                raise ValueError("the points before %d are rolled up to %d s buckets by %s: a job that reaches them needs a bucket_s that is a "
                                 "multiple of %d and bucket_op=%r" % (bound, tier_s, tier_op, tier_s, tier_op))

    def job(self, algo_type, tad_id, end_time="", pod_label="", pod_name="", pod_namespace="", external_ip="", svc_port_name="", bucket_s=0,
            bucket_op="sum", complete_before=None):
        """One job over everything fed so far -> (stats dict, list of result rows): what anomaly_detection(algo_type, all rows fed, "",
        end_time, tad_id, ns_ignore_list, agg_flow, the same filters) returns, the sentinel row included.  end_time bounds
        flowEndSeconds in svc and external mode; the pod query has no time filter.

        bucket_s > 0: the job judges throughput per bucket of bucket_s seconds, not per second (TadEngine.run_state_buckets, on the
        device): the rows are those of anomaly_detection over everything fed with flowEndSeconds floored to a multiple of bucket_s,
        the points of a bucket folded by bucket_op ("sum", what the aggregated flow types do, or "max"); a row's flowEndSeconds is its
        bucket's start.  end_time, if given, must then be a multiple of bucket_s (a bucket cut by it would hold a part of its rows).
        complete_before=now: judge only the buckets that lie wholly before `now` — the window ends at the start of now's bucket, so
        the half-filled newest bucket is not judged as a drop.  bucket_s=0 is the job as it always was."""
        if algo_type not in _ad.VALID_ALGOS:
            raise ValueError("Algorithm should be in {}".format(" or ".join(_ad.VALID_ALGOS)))
        bucket_s = self._bucket_args(bucket_s, bucket_op)
        if complete_before is not None and not bucket_s:
            raise ValueError("complete_before needs bucket_s")
        self._usable()
        self._check_job_buckets(0, bucket_s, bucket_op)
        terms = self._terms(pod_label or "", pod_name or "", pod_namespace or "", external_ip or "", svc_port_name or "")
        decoder = _KeyDecoder(self._dict, self._vocab)      # the key table: decoded on demand, for the keys with result rows
        table = {name: _KeyColumn(decoder, "direction" if name == "direction" else i) for i, name in enumerate(_ad.KEY_COLUMNS[self.mode])}
        prep = _ad.PreparedColumns(self.mode, None, None, None, None, None, table, 0, 0)
        if self._state is None:
            return {}, [_ad._sentinel_row(algo_type, self.agg_flow, tad_id)]
        keep, _ = self._dict.select(terms, out="device")
        to_t = _ad._epoch(end_time) if self.agg_flow != "pod" else 0
        if not bucket_s:
            res = self._engine.run_state_keys(self._state, keep, to_t=to_t, algo=algo_type, job_id=str(tad_id or ""))
            return res.stats, _ad.result_rows(prep, res, algo_type, self.agg_flow, tad_id)
        if to_t % bucket_s:
            raise ValueError("end_time must be a multiple of bucket_s (%d)" % bucket_s)
        if complete_before is not None:
            edge = (int(complete_before) // bucket_s) * bucket_s
            to_t = min(to_t, edge) if to_t else edge
            if to_t == 0:      # (0 means "no bound" to the engine; nothing fed lies before the epoch's first bucket)
                return {}, [_ad._sentinel_row(algo_type, self.agg_flow, tad_id)]
        res = self._engine.run_state_buckets(self._state, bucket_s, 0, bucket_op, to_t=to_t, key_keep=keep, algo=algo_type, job_id=str(tad_id or ""))
        return res.stats, _ad.result_rows(prep, res, algo_type, self.agg_flow, tad_id)

    def snapshot(self):
        """Everything the instance holds, as a dict of numpy arrays (np.savez takes it as it is): the state's exports (moments, history,
        series, times), the key dictionary's tuples and sides, and every string dictionary's values in Arrow's layout.  `restore` builds
        an instance from it that continues as this one would."""
        self._usable()
        snap = {"mode": np.asarray([self.mode]), "num_keys": np.asarray([self.num_keys], dtype=np.uint64),
                "watermark": np.asarray([self.watermark], dtype=np.int64)}
        cols, side = self._dict.export()
        for c, col in enumerate(cols):
            snap["key_col%d" % c] = col
        snap["key_side"] = side
        for i, v in enumerate(self._vocab):
            snap["vocab%d_offsets" % i], snap["vocab%d_data" % i] = v.export()
        if self._state is not None:
            for name, a in self._state.export().items():
                snap["state_" + name] = a
            snap["state_history_len"], snap["state_history"] = self._state.export_history()
            snap["state_series_len"], snap["state_series"] = self._state.export_series()
            snap["state_times"] = self._state.export_times()
        if getattr(self, "_tiers", None):      # (an instance that never rolled up snapshots exactly what it always did)
            snap["rollup_tiers"] = np.asarray([(b, s, 1 if op == "max" else 0) for b, s, op in self._tiers], dtype=np.int64).reshape(-1, 3)
        return snap

    @classmethod
    def restore(cls, engine, snapshot, agg_flow="svc", pod_ident="labels", ns_ignore_list=()):
        """A new instance holding what `snapshot()` returned (after a restart: np.load of the saved dict).  agg_flow / pod_ident must be
        the snapshot's; ns_ignore_list applies to the rows fed from here on."""
        self = cls(engine, agg_flow, pod_ident, ns_ignore_list)
        try:
            if str(np.asarray(snapshot["mode"]).reshape(-1)[0]) != self.mode:
                raise ValueError("the snapshot was taken in mode %r, not %r" % (str(np.asarray(snapshot["mode"]).reshape(-1)[0]), self.mode))
            for i, v in enumerate(self._vocab):
                v.load((np.asarray(snapshot["vocab%d_offsets" % i]), np.asarray(snapshot["vocab%d_data" % i])))
            self._dict.load([snapshot["key_col%d" % c] for c in range(len(self._vocab))], snapshot["key_side"])
            if "watermark" in snapshot:      # (a snapshot of before the poll loop has none)
                self.watermark = int(np.asarray(snapshot["watermark"]).reshape(-1)[0])
            if "rollup_tiers" in snapshot:   # (a snapshot of an instance that never rolled up, or of before the roll-up, has none)
                self._tiers = [(int(b), int(s), "max" if op else "sum") for b, s, op in np.asarray(snapshot["rollup_tiers"]).reshape(-1, 3).tolist()]
            if "state_n" in snapshot:
                st = self._engine.state_create(len(snapshot["state_n"]), history=True, series=True, times=True)
                self._state = st
                st.load({f: snapshot["state_" + f] for f in ("n", "avg", "m2", "ewma", "last_t")})
                st.load_history(snapshot["state_history_len"], snapshot["state_history"])
                st.load_series(snapshot["state_series_len"], snapshot["state_series"])
                st.load_times(snapshot["state_times"])
        except Exception:
            self.close()
            raise
        return self

    def _usable(self):
        if self._broken:
            raise RuntimeError("this instance is inconsistent (%s): restore one from a snapshot taken before the retire" % self._broken)

    def device_bytes(self):
        """the device bytes of everything the instance holds: the state, the key dictionary and every string dictionary"""
        return (self._state.nbytes() if self._state is not None else 0) + self._dict.nbytes() + sum(v.nbytes() for v in self._vocab)

    def retire(self, idle_before=0):
        """Shed what is dead, on the device: the keys whose newest flowEndSeconds lies before idle_before (0 = no time rule; a key
        without points always goes), and every string no surviving key uses.  The chain: TadState.compact -> KeyDict.compact with its
        remap; per vocabulary KeyDict.used_codes; then per vocabulary StringDict.compact with that mask; then ONE KeyDict.recode with
        every column's remap.  Masks and remaps stay on the device.  Jobs and feeds afterwards give what an instance gives that was
        fed only the rows of the surviving keys; a retired name that returns is a new string and a new key.

        Failure.  Each call of the chain is atomic; two PAIRS of calls are not, and a failure between the two halves of a pair leaves
        an instance that is NOT consistent.  (1) The state is compacted first and the key dictionary takes its remap second: if
        KeyDict.compact fails after a state compaction that retired keys, the state holds renumbered keys and the dictionary still
        hands out the ids of before.  (2) The vocabularies are compacted before the keys are recoded: if the recode fails (it
        allocates fresh records and a fresh table), or a StringDict.compact fails after an earlier vocabulary was compacted, the keys
        hold codes of before, and a compacted vocabulary cannot be brought back.  In both cases the call raises, and the instance
        refuses every later feed, job, snapshot and retire with a RuntimeError: it must be replaced by `restore` of a snapshot
        taken before the call.  Every other failure raises with the instance consistent and usable — the state's own compaction,
        a mask (every mask is computed before the first vocabulary is compacted), a StringDict.compact before any vocabulary moved:
        the keys are then retired or not, the strings not yet, and the next retire finishes the work.  The masks and remaps of the
        call are released on every path.

        Returns a dict: keys_before / keys_after, values_before / values_after (a list, one entry per vocabulary), bytes_before /
        bytes_after (device_bytes())."""
        self._usable()
        lib = self._engine._lib
        if not (getattr(lib, "tad_features", None) and lib.tad_features() & _capi.TAD_FEATURE_STRING_RETIRE):
            raise TadError(_capi.TAD_ERR_INVALID_ARGUMENT, "this build of the library has no tad_strdict_compact (TAD_FEATURE_STRING_RETIRE)")
        out = {"keys_before": self.num_keys, "values_before": [v.num_values() for v in self._vocab], "bytes_before": self.device_bytes()}
        if self._state is not None:
            if self.num_keys > self._state.num_keys:      # (a remap has one entry per key of the dictionary)
                self._state.resize(self.num_keys)
            remap, cs = self._state.compact(int(idle_before), out="device")
            try:
                if cs["keys_after"] != cs["keys_before"]:
                    self._dict.compact(remap)
            except Exception as exc:                      # the state is renumbered, the dictionary is not
                self._broken = "retire failed between the state and the key dictionary: %s" % exc
                raise
            finally:
                _release(remap)
            if cs["keys_after"] == 0:                     # nothing is left: as before the first feed
                self._state.close()
                self._state = None
        held, compacted = [], False                       # the call's device masks and remaps
        try:
            masks, remaps = [], {}
            for i, v in enumerate(self._vocab):
                masks.append(self._dict.used_codes(i, v.num_values(), out="device")[0])
                held.append(masks[i])
            for i, v in enumerate(self._vocab):
                remaps[i], st = v.compact(masks[i], out="device")
                held.append(remaps[i])
                compacted = compacted or st["values_after"] != st["values_before"]
            self._dict.recode(remaps)
        except Exception as exc:
            if compacted:
                self._broken = "retire failed between the vocabularies and the keys: %s" % exc
            raise
        finally:
            for x in held:
                _release(x)
        out.update(keys_after=self.num_keys, values_after=[v.num_values() for v in self._vocab], bytes_after=self.device_bytes())
        return out

    def close(self):
        if self._state is not None:
            self._state.close()
            self._state = None
        self._dict.close()
        for v in self._vocab:
            v.close()
