"""The read-back query (theia_amd/rest.py): tadetector rows -> ThroughputAnomalyDetectorStats, every field in Go's string form.

CPU: rest_test.go's Test_getTadetectorResult restated (pkg/apiserver/registry/intelligence/throughputanomalydetector/rest_test.go:229-380),
Go's string forms of the scanned columns, the garbage collection of stale rows (controller.go:232-276).  GPU: the reference's e2e result map
(test/e2e/throughputanomalydetection_test.go:191-243: throughput prefix, verdict, field count per aggregation type) on the rows a job of the
MI355X engine wrote: run -> COMPLETED -> getTADetectorResult's SELECT.  (The REST verbs and the CLI's retrieve table are SURVEY.md section 2
#6 / #7, out of scope: their round-4 restatement was removed.)"""
import uuid
from datetime import datetime, timezone

import numpy as np
import pyarrow as pa
import pytest

from theia_amd import controller as ctl
from theia_amd import rest

NS = "flow-visibility"


class StubClickHouse:
    """query_columns answers with a prepared column dict (what sqlmock.NewRows does in rest_test.go); records statements."""

    def __init__(self, columns=None, fail=None):
        self.columns, self.fail, self.queries, self.commands = columns or {}, fail, [], []

    def query_columns(self, sql, dict_strings=False, params=None):
        self.queries.append((sql, params))
        if self.fail:
            raise IOError(self.fail)
        return {k: np.asarray(v, dtype=object) for k, v in self.columns.items()}

    def command(self, sql):
        self.commands.append(sql)


MOCK = {"id": "mock_Id", "sourceIP": "mock_SourceIP", "sourceTransportPort": "mock_SourceTransportPort", "destinationIP": "mock_DestinationIP",
        "destinationTransportPort": "mock_DestinationTransportPort", "flowStartSeconds": "mock_FlowStartSeconds",
        "flowEndSeconds": "mock_FlowEndSeconds", "throughput": "mock_Throughput", "aggType": "mock_AggType", "algoType": "mock_AlgoType",
        "algoCalc": "mock_AlgoCalc", "anomaly": "mock_Anomaly", "podNamespace": "mock_PodNamespace", "podLabels": "mock_PodLabels",
        "podName": "mock_PodName", "direction": "mock_Direction", "destinationServicePortName": "mock_DestinationServicePortName"}


@pytest.mark.parametrize("agg_flow,pod_name,n_cols", [("", "", 12), ("external", "", 8), ("pod", "", 10), ("pod", "mock_PodName", 10), ("svc", "", 8)])
def test_get_tad_result_scans_the_columns_of_its_query(agg_flow, pod_name, n_cols):
    """Test_getTadetectorResult (rest_test.go:229-380): one mock row per query kind; exactly the selected fields are filled."""
    cols = rest.result_columns(agg_flow, pod_name)
    assert len(cols) == n_cols
    client = StubClickHouse({c: [MOCK[c]] for c in cols})
    stats = rest.get_tad_result(client, "mock_Id", agg_flow, pod_name)
    assert len(stats) == 1
    want = rest.ThroughputAnomalyDetectorStats(**{c: MOCK[c] for c in cols})
    assert stats[0] == want
    assert {f for f, v in vars(stats[0]).items() if v != ""} == set(cols)          # nothing else is filled
    sql, params = client.queries[0]
    assert params == {"id": "mock_Id"} and "mock_Id" not in sql
    # the reference's statement, token for token (queryMap, rest.go:59-123), with its positional placeholder
    assert sql.replace("({id:String})", "(?);") == rest.reference_result_query(agg_flow, pod_name)
    assert sql.startswith("SELECT id, ") and sql.endswith("FROM tadetector WHERE id = ({id:String})")


def test_reference_queries_column_for_column():
    assert rest.reference_result_query("") == ("SELECT id, sourceIP, sourceTransportPort, destinationIP, destinationTransportPort, flowStartSeconds, "
                                               "flowEndSeconds, throughput, aggType, algoType, algoCalc, anomaly FROM tadetector WHERE id = (?);")
    assert rest.reference_result_query("pod", "p") == ("SELECT id, podNamespace, podName, direction, flowEndSeconds, throughput, aggType, algoType, "
                                                       "algoCalc, anomaly FROM tadetector WHERE id = (?);")
    assert rest.query_kind("pod", "") == "podLabel" and rest.query_kind("anything", "") == "tad"


@pytest.mark.parametrize("v,want", [
    # strconv.FormatFloat(v, 'g', -1, 64)
    (4005703059.0, "4.005703059e+09"), (1e6, "1e+06"), (999999.0, "999999"), (100000.0, "100000"), (123456.5, "123456.5"), (1.5, "1.5"), (3.0, "3"),
    (0.0001, "0.0001"), (0.00001234, "1.234e-05"), (12345678.9, "1.23456789e+07"), (1e21, "1e+21"), (4005277824.2, "4.0052778242e+09"),
    (-2.5, "-2.5"), (0.0, "0"), (5e-324, "5e-324"), (1.7976931348623157e308, "1.7976931348623157e+308"), (float("nan"), "NaN"), (float("inf"), "+Inf"),
    (1000000000.0, "1e+09"), (5000000000.0, "5e+09"), (2500000000.0, "2.5e+09")])
def test_go_format_float(v, want):
    assert rest.go_format_float(v) == want


def test_go_string_of_the_column_types():
    assert rest.go_string(np.uint16(5201)) == "5201" and rest.go_string(58076) == "58076"
    assert rest.go_string(np.float64(4005703059)) == "4.005703059e+09"
    assert rest.go_string(datetime(2022, 8, 11, 7, 26, 54, tzinfo=timezone.utc)) == "2022-08-11T07:26:54Z"
    assert rest.go_string(np.datetime64("2022-08-11T07:26:54")) == "2022-08-11T07:26:54Z"
    assert rest.go_string(b"abc") == "abc" and rest.go_string("x") == "x" and rest.go_string(None) == "" and rest.go_string(True) == "true"


def new_tad(**spec):
    return ctl.ThroughputAnomalyDetector(name="tad-" + str(uuid.uuid4()), namespace=NS, spec=ctl.ThroughputAnomalyDetectorSpec(**spec))


def test_stale_rows_are_collected_and_running_jobs_resynced():
    """handleStaleResources (controller.go:232-276) + HandleStaleDbEntries (util.go:239-270)."""
    import threading
    gate = threading.Event()
    orphan, broken = str(uuid.uuid4()), "not-a-uuid"
    c = None
    try:
        client = StubClickHouse()
        c = ctl.AnomalyDetectorController(clickhouse=client, run_job=lambda args, t: gate.wait(10), progress=lambda: (1, 4), resync_period=0.01)
        t = new_tad(jobType="EWMA")
        c.create(t)
        c.wait(NS, t.name, states=(ctl.STATE_RUNNING,), timeout=10)
        client.columns = {"id": [t.name[4:], orphan, broken]}
        with c._lock:
            c._periodic.clear()                                   # as after a restart of the manager
        errors = c.handle_stale_resources(NS)
        assert client.commands == [ctl.cleanup_query(orphan)]      # the live job's rows stay, the orphan's go
        assert len(errors) == 1 and errors[0].startswith(broken)   # reported, did not stop the others
        assert c._periodic == {(NS, t.name): True}
        assert client.queries[-1][0] == "SELECT DISTINCT id FROM tadetector"
        gate.set()
        assert c.wait(NS, t.name, timeout=10).status.state == ctl.STATE_COMPLETED     # ... and the resync carries it to the end
    finally:
        gate.set()
        if c is not None:
            c.shutdown()


# ---- the e2e result map (throughputanomalydetection_test.go:191-243) on the engine's rows ----
E2E_RESULT_MAP = {     # result_map (:192-221): throughput prefix -> "true"; "1.005" for ARIMA: tests/test_gpu_job.py:E2E_RESULT_MAP's note
    "ARIMA": {"4.005", "1.000", "5.000", "2.500", "5.002", "2.003", "2.002", "1.005"},
    "EWMA": {"4.004", "4.005", "4.006", "5.000", "2.002", "2.003", "2.500"},
    "DBSCAN": {"1.000", "1.005", "5.000", "3.260", "2.058", "5.002", "5.027", "2.500", "1.029", "1.630"},
}
E2E_ASSERT = {         # assert_variable_map (:222-243)
    "None": dict(n=12, anomaly=11, throughput=7), "podName": dict(n=10, anomaly=9, throughput=5), "podLabel": dict(n=9, anomaly=8, throughput=4),
    "external": dict(n=8, anomaly=7, throughput=3), "svc": dict(n=8, anomaly=7, throughput=3)}


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["EWMA", "DBSCAN", "ARIMA"])
@pytest.mark.parametrize("agg_type", ["None", "podName", "podLabel", "external", "svc"])
def test_e2e_result_map_on_the_engine(engine, golden, algo, agg_type):
    """executeRetrieveTest's checks (throughputanomalydetection_test.go:222-300): run the job, wait for COMPLETED, read the job's rows the way
    getTADetectorResult does, and check per row the field count of the aggregation type, the verdict and the throughput prefix — here through
    ClickHouse's HTTP interface (in-process), the controller, `tad_run` on the GPU, the INSERT, the handler's SELECT and Go's string forms."""
    from theia_amd import clickhouse as ch
    from fake_clickhouse import FakeClickHouse, arrow_table
    from job_helpers import e2e_flows
    spec = {"None": {}, "podName": dict(aggFlow="pod", podName="test_podName"), "podLabel": dict(aggFlow="pod", podLabel="test_key"),
            "external": dict(aggFlow="external"), "svc": dict(aggFlow="svc")}[agg_type]
    server = FakeClickHouse()
    c = None
    try:
        flows = e2e_flows(golden)
        sql = ch.rows_query("", "", [], spec.get("aggFlow", ""), spec.get("podLabel", ""), "", "", spec.get("podName", ""), "")
        cols = sql[len("SELECT "):sql.index(" FROM ")].split(", ")
        server.responses[sql] = arrow_table({name: flows[name] for name in cols})
        client = ch.ClickHouseHTTP(server.url, user="", password="")
        c = ctl.AnomalyDetectorController(clickhouse=client, engine=engine)
        t = new_tad(jobType=algo, **spec)
        c.create(t)
        done = c.wait(NS, t.name, timeout=180)
        assert done.status.state == ctl.STATE_COMPLETED, done.status.errorMsg
        stats = rest.get_tad_result(client, done.status.sparkApplication, spec.get("aggFlow", ""), spec.get("podName", ""))
        assert len(stats) >= 2
        a = E2E_ASSERT[agg_type]
        fields = rest.result_columns(spec.get("aggFlow", ""), spec.get("podName", ""))
        for s in stats:
            # the e2e splits the printed line on white space (strings.Fields, :276-283): an empty value is no field.  podLabel mode: the test
            # flows' labels `{test_key:test_value}` are no JSON, remove_meaningless_labels turns them into "" (anomaly_detection.py:107-131),
            # which is why assert_variable_map counts 9 fields there for the SELECT's 10 columns
            f = [v for v in (getattr(s, name) for name in fields) if v != ""]
            assert len(f) == a["n"], f
            assert f[a["throughput"]][:5] in E2E_RESULT_MAP[algo] and f[a["anomaly"]] == "true", f
            assert f[0] == t.name[4:]
        c.delete(NS, t.name)
        assert rest.get_tad_result(client, t.name[4:], spec.get("aggFlow", ""), spec.get("podName", "")) == []     # cleaned up
    finally:
        if c is not None:
            c.shutdown()
        server.close()


def test_go_format_float_round_trips_and_switches_form_where_strconv_does():
    """Properties of strconv.FormatFloat(v, 'g', -1, 64) on random doubles: the text parses back to the same bits (shortest digits), the %e form is
    used exactly when the decimal exponent is < -4 or >= 6, its exponent has a sign and at least two digits, and there is never a trailing '.' or
    a superfluous zero in the mantissa."""
    import struct
    rng = np.random.default_rng(7)
    raw = rng.integers(0, 1 << 63, size=20000, dtype=np.uint64)
    vals = [struct.unpack("<d", struct.pack("<Q", int(r)))[0] for r in raw]
    vals += [float(x) for x in rng.integers(0, 1 << 40, size=2000)] + [x / 8 for x in range(-50, 50)] + [10.0 ** k for k in range(-12, 25)]
    for v in vals:
        if v != v or v in (float("inf"), float("-inf")):
            continue
        s = rest.go_format_float(v)
        assert float(s) == v, (v, s)
        if v == 0:
            continue
        from decimal import Decimal
        x = Decimal(repr(v)).adjusted()      # decimal exponent of the leading digit
        if "e" in s:
            mant, ex = s.split("e")
            assert x < -4 or x >= 6, (v, s)
            assert ex[0] in "+-" and len(ex) >= 3 and int(ex) == x, (v, s)
        else:
            mant = s
            assert -4 <= x < 6, (v, s)
        assert not mant.endswith(".") and not (("." in mant) and mant.endswith("0")), (v, s)
