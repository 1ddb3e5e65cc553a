"""A ClickHouse HTTP server in a thread, for the tests of the client, the controller and the REST API: it answers each SELECT of
theia_amd.clickhouse with the Arrow stream registered for its SQL text and records the inserts; `arrow_table` makes such a stream's
table from flow columns, `server` is the fixture that starts and closes one."""
import io
import json
import threading
import urllib.parse
from http.server import BaseHTTPRequestHandler, HTTPServer

import numpy as np
import pyarrow as pa
import pyarrow.ipc as ipc
import pytest

from theia_amd import clickhouse as ch


class FakeClickHouse:
    """Answers a SELECT by looking the SQL text up in `responses` (exact match), records INSERTed rows."""

    def __init__(self):
        self.responses = {}
        self.queries, self.inserted, self.auth, self.commands = [], [], [], []
        owner = self

        class Handler(BaseHTTPRequestHandler):
            def log_message(self, *a):
                pass

            def do_POST(self):
                body = self.rfile.read(int(self.headers.get("Content-Length", 0)))
                params = urllib.parse.parse_qs(urllib.parse.urlparse(self.path).query)
                owner.auth.append(self.headers.get("Authorization"))
                if "query" in params and params["query"][0].startswith("INSERT INTO"):
                    if params["query"][0].endswith("FORMAT ArrowStream"):
                        rows = ipc.open_stream(io.BytesIO(body)).read_all().to_pylist()
                    else:
                        rows = [json.loads(l) for l in body.decode().splitlines() if l]
                    owner.inserted.append((params["query"][0], rows))
                    self.send_response(200); self.end_headers(); return
                sql = body.decode()
                if sql.startswith("ALTER TABLE"):                      # a statement without a result set
                    owner.commands.append(sql)
                    self.send_response(200); self.end_headers(); return
                owner.queries.append(sql)
                assert sql.endswith(" FORMAT ArrowStream"), sql
                key = sql[: -len(" FORMAT ArrowStream")]
                if " FROM tadetector" in key:                          # the result table: answered from what has been inserted
                    table = owner.select_tadetector(key, {k[6:]: v[0] for k, v in params.items() if k.startswith("param_")})
                    sink = io.BytesIO()
                    with ipc.new_stream(sink, table.schema) as w:
                        w.write_table(table)
                    self.send_response(200); self.end_headers(); self.wfile.write(sink.getvalue()); return
                known = {k.rstrip(): v for k, v in owner.responses.items()}   # the client strips the SQL's trailing blank
                if key not in known:
                    self.send_response(404); self.end_headers(); self.wfile.write(b"unknown query"); return
                table = known[key]
                sink = io.BytesIO()
                with ipc.new_stream(sink, table.schema) as w:
                    w.write_table(table)
                self.send_response(200); self.end_headers(); self.wfile.write(sink.getvalue())

        self.httpd = HTTPServer(("127.0.0.1", 0), Handler)
        self.url = "http://127.0.0.1:%d" % self.httpd.server_address[1]
        self.thread = threading.Thread(target=self.httpd.serve_forever, daemon=True)
        self.thread.start()

    def select_tadetector(self, sql, params):
        """`SELECT <columns> FROM tadetector WHERE id = ({id:String})` / `SELECT DISTINCT id FROM tadetector` over the inserted rows, with
        the column types of create_table.sh:363-384 (a column an INSERT did not name holds the type's default; rows a
        `ALTER TABLE ... DELETE WHERE id = ('<id>')` named are gone)."""
        deleted = {c.split("('")[1].split("')")[0] for c in self.commands if "DELETE WHERE id = ('" in c}
        rows = [r for _, rs in self.inserted for r in rs if r.get("id") not in deleted]
        if sql.startswith("SELECT DISTINCT id FROM tadetector"):
            return pa.table({"id": pa.array(sorted({r["id"] for r in rows}), pa.string())})
        cols = sql[len("SELECT "):sql.index(" FROM ")].split(", ")
        assert sql.endswith("WHERE id = ({id:String})") and "id" in params, (sql, params)
        rows = [r for r in rows if r.get("id") == params["id"]]
        arrays = {}
        for c in cols:
            kind = ch.TADETECTOR_COLUMNS[c]
            if kind == "datetime":
                arrays[c] = pa.array(np.asarray([r.get(c) or 0 for r in rows], dtype="int64").astype("datetime64[s]"), pa.timestamp("s"))
            elif kind == "f64":
                arrays[c] = pa.array([float(r.get(c) or 0.0) for r in rows], pa.float64())
            elif kind in ("u16", "u8"):
                arrays[c] = pa.array([int(r.get(c) or 0) for r in rows], pa.uint16())
            else:
                arrays[c] = pa.array([str(r.get(c) or "") for r in rows], pa.string())
        return pa.table(arrays)

    def close(self):
        self.httpd.shutdown()


def arrow_table(cols):
    """column dict -> Arrow table typed the way ClickHouse types default.flows (create_table.sh:31-85)."""
    arrays = {}
    for name, v in cols.items():
        v = np.asarray(v)
        if name.endswith("Seconds"):
            arrays[name] = pa.array(v.astype("datetime64[s]"), pa.timestamp("s"))      # DateTime
        elif name in ("throughput", "max(throughput)", "sum(throughput)"):
            arrays[name] = pa.array(v.astype(np.uint64), pa.uint64())
        elif v.dtype.kind in "iu":
            arrays[name] = pa.array(v.astype(np.uint16), pa.uint16())
        else:
            arrays[name] = pa.array(v.astype(str).tolist(), pa.string())
    return pa.table(arrays)


@pytest.fixture()
def server():
    s = FakeClickHouse()
    yield s
    s.close()
