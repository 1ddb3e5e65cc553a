"""Throughput anomaly detection on a long-lived streaming state: the TAD twin of drop_detection.PeriodicalDropDetection.

`anomaly_detection` (anomaly_detection.py) answers one job from the flow table: it reads the rows, applies the job's filters and runs
the batch job.  A `StreamingAnomalyDetection` is fed the flow rows as they arrive — in any order — and answers the same jobs from what it
keeps on the device: a key dictionary (KeyDict: the mode's key tuples -> stable ids), a series state (TadState with history and times,
fed through TadEngine.merge_stream) and, on the host, one vocabulary per string column and the key table.

The job's name filters (--pod-name, --pod-namespace, --pod-label, --external-ip, --svc-port-name) are predicates on KEY columns of the
mode, so a job is a key selection: the filter is evaluated once per distinct string of the vocabulary (equality is one code, ilike
goes over the distinct label strings), KeyDict.select turns the vocabulary masks into a key mask on the device, and
TadEngine.run_state_keys judges the selected keys only.  The predicates that are NOT key predicates — the namespace ignore list (it tests
both namespaces of a row), flowType = 3 in external mode, the `<> ''` rules — are applied to the rows in `feed`, before they reach the
state.  Mode None (no aggregation) has no key filter to serve and is not offered.
"""
import numpy as np

from . import anomaly_detection as _ad

MODES = ("svc", "external", "pod")


class _Vocabulary:
    """string -> code; a string keeps the code it was first given (new strings of a batch get the next codes in their sorted order)"""

    def __init__(self):
        self.code = {}
        self.values = []

    def encode(self, strings):
        uniq, inv = np.unique(np.asarray(strings).astype(str), return_inverse=True)
        codes = np.empty(uniq.size, dtype=np.int64)
        for i, s in enumerate(uniq.tolist()):
            c = self.code.get(s)
            if c is None:
                c = self.code[s] = len(self.values)
                self.values.append(s)
            codes[i] = c
        return codes[inv]

    def mask(self, predicate):
        """one byte per code: predicate(string)"""
        return np.fromiter((1 if predicate(s) else 0 for s in self.values), dtype=np.uint8, count=len(self.values))


def _strings(flows, name):
    c = _ad._str_col(flows, name)
    return c.materialise() if isinstance(c, _ad.DictColumn) else c


class StreamingAnomalyDetection:
    """agg_flow: "svc", "external" or "pod".  pod_ident (pod mode): "labels" keys the pods by (namespace, labels, direction) and serves
    the jobs with --pod-label and the ones without a pod filter; "name" keys them by (namespace, name, direction) and serves the jobs
    with --pod-name — the two key sets of the reference's pod query.  ns_ignore_list is fixed for the instance: it is applied to the
    rows as they are fed.  `job` returns what anomaly_detection returns for the same arguments over all rows fed so far.  One
    difference at the edge: in pod mode the feed drops the rows of a side whose labels / name are '' (the query's `<> ''` rule for a
    job without a pod filter), while the batch query with a pod_label or pod_name filter applies only that filter — so a pattern that
    matches the empty string, such as pod_label='%', finds the '' keys in the batch job and not here."""

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
        self._vocab = [_Vocabulary() for _ in range(2 if agg_flow == "pod" else 1)]     # pod: namespaces, labels / names
        self._dict = self._engine.key_dict(len(self._vocab))
        self._state = None
        self._keys = [[] for _ in _ad.KEY_COLUMNS[self.mode]]      # the host key table: key id -> the mode's key columns

    @property
    def state(self):
        return self._state

    @property
    def num_keys(self):
        return len(self._keys[0])

    def feed(self, flows):
        """One batch of flow rows (a column dict as anomaly_detection takes it), in any order; rows of a (key, flowEndSeconds) group may
        be split over feeds.  Returns the merge's statistics (TadEngine.merge_stream), or None when no row passed the row predicates."""
        eng = self._engine
        n = len(flows["flowEndSeconds"])
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
                col = _strings(flows, side + ident)
                sides.append(([self._vocab[0].encode(_strings(flows, side + "PodNamespace")), self._vocab[1].encode(col)], keep & (col != "")))
            if not (sides[0][1].any() or sides[1][1].any()):
                return None
            key, key2, first, _ = self._dict.encode(sides[0][0], sides[0][1], sides[1][0], sides[1][1])
            for v in np.asarray(first).tolist():
                b = v >= n
                cols = sides[1 if b else 0][0]
                row = v - n if b else v
                self._keys[0].append(self._vocab[0].values[cols[0][row]])
                self._keys[1].append(self._vocab[1].values[cols[1][row]])
                self._keys[2].append("outbound" if b else "inbound")
        else:
            name = "destinationIP" if self.agg_flow == "external" else "destinationServicePortName"
            col = _strings(flows, name)
            if self.agg_flow == "external":
                keep &= np.asarray(flows["flowType"]).astype(np.int64) == 3
            else:
                keep &= col != ""
            if not keep.any():
                return None
            codes = self._vocab[0].encode(col)
            key, key2, first, _ = self._dict.encode([codes], keep)
            self._keys[0] += [self._vocab[0].values[codes[v]] for v in np.asarray(first).tolist()]
        if self._state is None:
            self._state = eng.state_create(self.num_keys, history=True, series=True, times=True)
        elif self.num_keys > self._state.num_keys:
            self._state.resize(self.num_keys)
        return eng.merge_stream(self._state, key, flow_end, value, agg_flow=self.agg_flow, key_id2=key2)

    def _terms(self, pod_label, pod_name, pod_namespace, external_ip, svc_port_name):
        """the job's name filters as (key column, vocabulary mask) terms of KeyDict.select"""
        if self.agg_flow == "external":
            return [(0, self._vocab[0].mask(lambda s: s == external_ip))] if external_ip else []
        if self.agg_flow == "svc":
            return [(0, self._vocab[0].mask(lambda s: s == svc_port_name))] if svc_port_name else []
        by_name = bool(pod_name) and not pod_label
        if by_name != (self.pod_ident == "name"):
            raise ValueError("this instance keys the pods by their %s: it serves jobs %s" %
                             (self.pod_ident, "with pod_name" if self.pod_ident == "name" else "with pod_label or without a pod filter"))
        if pod_label:
            rx = _ad._like_regex("%" + pod_label + "%")
            terms = [(1, self._vocab[1].mask(lambda s: rx.match(s) is not None))]
        elif pod_name:
            terms = [(1, self._vocab[1].mask(lambda s: s == pod_name))]
        else:
            return []
        if pod_namespace:
            terms.append((0, self._vocab[0].mask(lambda s: s == pod_namespace)))
        return terms

    def job(self, algo_type, tad_id, end_time="", pod_label="", pod_name="", pod_namespace="", external_ip="", svc_port_name=""):
        """One job over everything fed so far -> (stats dict, list of result rows): what anomaly_detection(algo_type, all rows fed, "",
        end_time, tad_id, ns_ignore_list, agg_flow, the same filters) returns, the sentinel row included.  end_time bounds
        flowEndSeconds in svc and external mode; the pod query has no time filter."""
        if algo_type not in _ad.VALID_ALGOS:
            raise ValueError("Algorithm should be in {}".format(" or ".join(_ad.VALID_ALGOS)))
        terms = self._terms(pod_label or "", pod_name or "", pod_namespace or "", external_ip or "", svc_port_name or "")
        prep = _ad.PreparedColumns(self.mode, None, None, None, None, None,
                                   {name: np.asarray(vals, dtype=object) for name, vals in zip(_ad.KEY_COLUMNS[self.mode], self._keys)}, 0, 0)
        if self._state is None:
            return {}, [_ad._sentinel_row(algo_type, self.agg_flow, tad_id)]
        keep, _ = self._dict.select(terms, out="device")
        to_t = _ad._epoch(end_time) if self.agg_flow != "pod" else 0
        res = self._engine.run_state_keys(self._state, keep, to_t=to_t, algo=algo_type, job_id=str(tad_id or ""))
        return res.stats, _ad.result_rows(prep, res, algo_type, self.agg_flow, tad_id)

    def close(self):
        if self._state is not None:
            self._state.close()
            self._state = None
        self._dict.close()
