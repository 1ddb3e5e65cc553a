"""Two host forms of the drop job's flow-row query (include/tad.h, tad_drop_select) — a HELPER of the tests, not a test and not product code.

`query_pandas` restates the query on STRING columns, literally in its three stages (filtered -> processed -> aggregated): the rows whose
ingress or egress rule action is 2 or 3 inside the time bounds, counted per (six endpoint columns, start date, two actions); then endpoint
and direction chosen per group; then the counts summed per (endpoint, direction, date).  `select_rows` is the row rule of tad_drop_select
on dictionary CODES, written directly in numpy: the seven output columns in input order.  `sum_selected` sums its counts per
(tuple, day) and decodes the tuples, which is what the engine's path computes; tests/test_drop_select_abi.py holds the two forms against
each other (the two GROUP BYs compose), tests/test_gpu_drop_select.py holds the engine against both.  Both are written from the rule, not
from the reference's query text."""
import numpy as np

DAY = 86400
DROP_ACTIONS = (2, 3)
OUT_FIELDS = ("endpoint_kind", "endpoint_ns", "endpoint_name", "direction", "day_s", "count", "row")
DIRECTIONS = ("ingress", "egress")


def strings_of(codes, dictionaries):
    """code columns -> the string table `query_pandas` reads ('' = no pod)"""
    ips, nss, pods = (np.asarray(dictionaries[k], dtype=object) for k in ("ip", "pod_ns", "pod_name"))
    return {"sourceIP": ips[codes["src_ip"]], "sourcePodNamespace": nss[codes["src_pod_ns"]], "sourcePodName": pods[codes["src_pod_name"]],
            "destinationIP": ips[codes["dst_ip"]], "destinationPodNamespace": nss[codes["dst_pod_ns"]], "destinationPodName": pods[codes["dst_pod_name"]]}


def query_pandas(strings, ingress_action, egress_action, flow_start_s, flow_end_s=None, start_time=0, end_time=0, keep=None):
    """-> DataFrame(endpoint, direction, date 'YYYY-MM-DD', dropNumber), sorted by (endpoint, direction, date)"""
    import pandas as pd
    t = pd.DataFrame(dict(strings))
    t["ingressAction"] = np.asarray(ingress_action).astype(np.int64)
    t["egressAction"] = np.asarray(egress_action).astype(np.int64)
    t["flowStartSeconds"] = np.asarray(flow_start_s).astype(np.int64)
    if flow_end_s is not None:
        t["flowEndSeconds"] = np.asarray(flow_end_s).astype(np.int64)
    # stage 1, filtered: WHERE ... GROUP BY the nine columns, count(*)
    where = t["ingressAction"].isin(DROP_ACTIONS) | t["egressAction"].isin(DROP_ACTIONS)
    if start_time:
        where &= t["flowStartSeconds"] >= start_time
    if end_time:
        where &= t["flowEndSeconds"] < end_time
    if keep is not None:
        where &= np.asarray(keep).astype(bool)
    f = t[where].copy()
    f["flowStartDate"] = pd.to_datetime(f["flowStartSeconds"], unit="s").dt.floor("D")
    nine = ["sourceIP", "sourcePodName", "sourcePodNamespace", "destinationIP", "destinationPodName", "destinationPodNamespace", "flowStartDate",
            "ingressAction", "egressAction"]
    filtered = f.groupby(nine, sort=False, dropna=False).size().reset_index(name="flowNumber")
    # stage 2, processed: endpoint and direction per group
    ing = filtered["ingressAction"].isin(DROP_ACTIONS)
    dst_pod, src_pod = filtered["destinationPodName"] != "", filtered["sourcePodName"] != ""
    dst = np.where(dst_pod, filtered["destinationPodNamespace"] + "/" + filtered["destinationPodName"], filtered["destinationIP"])
    src = np.where(src_pod, filtered["sourcePodNamespace"] + "/" + filtered["sourcePodName"], filtered["sourceIP"])
    processed = pd.DataFrame({"endpoint": np.where(ing, dst, src), "direction": np.where(ing, "ingress", "egress"),
                              "date": filtered["flowStartDate"], "dropNumber": filtered["flowNumber"]})
    # stage 3, aggregated: SUM per (endpoint, direction, date)
    agg = processed.groupby(["endpoint", "direction", "date"], sort=True)["dropNumber"].sum().reset_index()
    agg["date"] = agg["date"].dt.strftime("%Y-%m-%d")
    return agg


def select_rows(ingress_action, egress_action, flow_start_s, src_ip, src_pod_ns, src_pod_name, dst_ip, dst_pod_ns, dst_pod_name, flow_end_s=None,
                src_pod_null=-1, dst_pod_null=-1, start_time=0, end_time=0, keep=None):
    """The row rule on codes -> dict of the seven output columns (OUT_FIELDS), rows in input order.  uint32 times are zero-extended."""
    ia, ea = np.asarray(ingress_action).astype(np.int64), np.asarray(egress_action).astype(np.int64)
    ts = np.asarray(flow_start_s).astype(np.int64)
    ing = (ia == 2) | (ia == 3)
    sel = ing | (ea == 2) | (ea == 3)
    if start_time:
        sel &= ts >= start_time
    if end_time:
        sel &= np.asarray(flow_end_s).astype(np.int64) < end_time
    if keep is not None:
        sel &= np.asarray(keep) != 0
    row = np.flatnonzero(sel)
    ing = ing[row]
    pick = lambda d, s: np.where(ing, np.asarray(d, dtype=np.int64)[row], np.asarray(s, dtype=np.int64)[row])
    pod = pick(dst_pod_name, src_pod_name)
    is_pod = pod != np.where(ing, np.int64(dst_pod_null), np.int64(src_pod_null))
    return {"endpoint_kind": is_pod.astype(np.int64),
            "endpoint_ns": np.where(is_pod, pick(dst_pod_ns, src_pod_ns), 0).astype(np.int64),
            "endpoint_name": np.where(is_pod, pod, pick(dst_ip, src_ip)).astype(np.int64),
            "direction": np.where(ing, 0, 1).astype(np.int64),
            "day_s": np.floor_divide(ts[row], DAY) * DAY,          # floor, also below zero
            "count": np.ones(row.size, dtype=np.uint64),
            "row": row.astype(np.uint64)}


def sum_selected(sel, dictionaries):
    """select_rows' output summed per (tuple, day) and decoded -> DataFrame like query_pandas'"""
    import pandas as pd
    ips, nss, pods = (np.asarray(dictionaries[k], dtype=object) for k in ("ip", "pod_ns", "pod_name"))
    t = pd.DataFrame({k: sel[k] for k in OUT_FIELDS[:6]})
    g = t.groupby(list(OUT_FIELDS[:5]), sort=False)["count"].sum().reset_index()
    endpoint = [nss[n] + "/" + pods[m] if k else ips[m] for k, n, m in zip(g["endpoint_kind"], g["endpoint_ns"], g["endpoint_name"])]
    out = pd.DataFrame({"endpoint": endpoint, "direction": np.asarray(DIRECTIONS, dtype=object)[g["direction"].to_numpy()],
                        "date": pd.to_datetime(g["day_s"], unit="s").dt.strftime("%Y-%m-%d"), "dropNumber": g["count"].astype(np.int64)})
    return out.sort_values(["endpoint", "direction", "date"]).reset_index(drop=True)
