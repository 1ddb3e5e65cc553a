"""A host model of the streaming-state API (include/tad.h) and seeded operation scripts over it — a helper module, no tests in it.

include/tad.h defines every call on a streaming state as a pure function of the table W of points the state holds.  StateModel keeps W
as three numpy arrays in (key, time) order and restates each call's rule over it; what a call must return comes from the oracles
(oracle.tad_oracle, oracle.stream_oracle, oracle.drop_oracle, oracle.arima_oracle).  No engine call is needed on this side.

make_script(seed) draws a list of operations with every argument fixed and every precondition decided, by running the model alone: a
script can be built, inspected and replayed without a device.  tests/test_state_model.py checks the model and the seed set on the host,
tests/test_gpu_state_sequences.py runs the scripts on a state and compares after every operation.

Not covered here: the dictionaries (tad_keydict / tad_strdict: tests/dict_model.py holds their model and their scripts), pod-mode
key_id2 batches, concurrent calls on one state, workspace-limit refusals."""
import numpy as np

from oracle import stream_oracle as sorc
from oracle import tad_oracle as orc
from state_helpers import HIST, I64, SER, STATE_FIELDS, TIMES, U64, drop_oracle_rows, expected_counts

KEY_SKIP = U64(orc.MASK64)
SEEDS = tuple(range(32))
N_OPS = 12
CEILING = 40000                # points held at any time
MAX_ARIMA_CHECKS = 3           # per sequence: the exact oracle costs seconds per few hundred fits
ARIMA_MAX_SERIES = 40
# the detectors' parameters: the sets of tests/test_gpu_random.py and tests/test_gpu_drop.py (0 = the default)
ALPHAS = (0.0, 0.3, 1 / 3, 0.05)
DBSCAN_PARAMS = ((0.0, 0), (5e5, 4), (4e9, 12), (0.5, 2), (2.0**64, 1))
DROP_PARAMS = ((0.0, 0), (2.5, 0), (1.0, 5), (3.0, 10))
KINDS = ("append", "late", "merge", "trim", "compact", "resize", "restart", "refused")
REFUSALS = ("dbscan_stream_without_history", "run_state_dbscan_without_history", "from_after_to", "start_time_in_run_state", "num_keys_differs")
CLASSES = ("many", "few-long", "arima", "grow-shrink-grow")


def _empty():
    return np.zeros(0, U64), np.zeros(0, I64), np.zeros(0, U64)


def _cat(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def _dbscan(x, eps, min_samples):
    """the quadratic definition on short keys, the sorted route (tests/test_oracle.py holds the two together) on long ones"""
    return (orc.dbscan_noise_sorted if x.size > 1024 else orc.dbscan_noise_1d)(x, eps, min_samples)


def _member(k, t, bk, bt):
    """mask over the points (k, t): the point is one of (bk, bt)"""
    if k.size == 0 or bk.size == 0:
        return np.zeros(k.size, bool)
    times = np.unique(np.concatenate([t, bt]))
    pack = lambda kk, tt: (kk.astype(U64) << U64(32)) | np.searchsorted(times, tt).astype(U64)
    return np.isin(pack(k, t), pack(bk, bt))


class StateModel:
    """W and the rules of include/tad.h over it.  One value op ("sum" / "max") and one ewma_alpha hold for the life of the state: the
    contracts of tad_state_trim and tad_state_merge are conditional on exactly that."""

    def __init__(self, num_keys, flags, op, alpha):
        assert op in ("sum", "max") and flags & SER and flags & TIMES
        self.num_keys, self.flags, self.op, self.alpha = int(num_keys), int(flags), op, float(alpha)
        self.key, self.t, self.value = _empty()
        self._snap = None

    # ---- W ----
    @property
    def alpha_eff(self):
        return self.alpha or 0.5            # tad_job.ewma_alpha: 0 -> 0.5

    def points(self):
        return self.key, self.t, self.value

    def _set(self, k, t, v):
        self.key, self.t, self.value = k.astype(U64), t.astype(I64), v.astype(U64)
        self._snap = None

    def per_key(self):
        """(n, last_t) per key, zeros for a key without points"""
        n = np.bincount(self.key.astype(I64), minlength=self.num_keys)
        last = np.zeros(self.num_keys, I64)
        end = np.cumsum(n) - 1
        last[n > 0] = self.t[end[n > 0]]
        return n, last

    # ---- the calls that change W ----
    def append(self, k, t, v):
        """tad_run_stream / tad_drop_stream: W <- stage0(W ++ stage0(batch)); a point not newer than its key's last_t fails the batch
        (ValueError, W unchanged).  Returns the batch's points."""
        bk, bt, bv = orc.stage0(k, t, v, self.op)
        n, last = self.per_key()
        i = bk.astype(I64)
        if ((n[i] > 0) & (bt <= last[i])).any():
            raise ValueError("late row")
        self._set(*orc.stage0(*_cat(self.points(), (bk, bt, bv)), self.op))
        return bk, bt, bv

    def merge(self, k, t, v, keep_from=0):
        """tad_state_merge: as append, placed by time, without the batch's points under keep_from.  Returns the tad_merge_stats counters."""
        counts = expected_counts(self.points(), (k, t, v), self.op, keep_from)
        counts["rows_in"] = counts["rows_used"] = int(np.asarray(k).size)
        bk, bt, bv = orc.stage0(k, t, v, self.op)
        if keep_from:
            keep = bt >= keep_from
            bk, bt, bv = bk[keep], bt[keep], bv[keep]
        if bk.size:
            self._set(*orc.stage0(*_cat(self.points(), (bk, bt, bv)), self.op))
        return counts

    def window_mask(self, from_t=0, to_t=0, keep_points=0):
        """tad_run_state_window's three rules in tad.h's order: >= from_t, then < to_t, then the newest keep_points per key"""
        m = np.ones(self.key.size, bool)
        if from_t:
            m &= self.t >= from_t
        if to_t:
            m &= self.t < to_t
        if keep_points:
            ki = self.key.astype(I64)
            per_key = np.bincount(ki, minlength=self.num_keys)
            inside = np.bincount(ki, weights=m, minlength=self.num_keys).astype(I64)     # per key, after rules (1) and (2)
            upto = np.cumsum(m)                                                           # points inside, this one included
            before_key = np.concatenate([[0], upto])[np.cumsum(per_key) - per_key]        # ... before the key's first point
            m &= inside[ki] - (upto - before_key[ki]) < keep_points                       # points of the key inside and newer than this one
        return m

    def trim(self, keep_points=0, keep_from=0):
        """tad_state_trim: rules (1) and (3) of the window, for good.  Returns the points dropped."""
        m = self.window_mask(keep_from, 0, keep_points)
        dropped = int((~m).sum())
        if dropped:
            self._set(self.key[m], self.t[m], self.value[m])
        return dropped

    def compact(self, retire_before=0):
        """tad_state_compact: key k survives iff n > 0 and (retire_before == 0 or last_t >= retire_before); the key count afterwards is
        max(m, 1).  Returns the remap and the counters of tad_compact_stats."""
        n, last = self.per_key()
        unseen = n == 0
        idle = ~unseen & (last < retire_before) if retire_before else np.zeros(self.num_keys, bool)
        alive = ~unseen & ~idle
        remap = np.where(alive, (np.cumsum(alive) - 1).astype(U64), KEY_SKIP)
        m = int(alive.sum())
        out = {"remap": remap, "keys_before": self.num_keys, "keys_after": m, "num_keys": max(m, 1), "keys_unseen": int(unseen.sum()),
               "keys_idle": int(idle.sum()), "points_dropped": int(n[idle].sum())}
        if m < self.num_keys:
            keep = alive[self.key.astype(I64)]
            self.num_keys = max(m, 1)
            self._set(remap[self.key[keep].astype(I64)], self.t[keep], self.value[keep])
        return out

    def resize(self, n):
        assert n >= self.num_keys
        self.num_keys = int(n)
        self._snap = None

    # ---- what the state must hold ----
    def expected_snapshot(self):
        """moments: the stream oracle on a fresh state over W in one batch; series = the values, times, history = the values sorted per key"""
        if self._snap is None:
            k, t, v = self.points()
            os_ = sorc.StreamState(self.num_keys)
            if k.size:
                sorc.run_stream(os_, k, t, v, op=self.op, alpha=self.alpha_eff)
            ln = np.bincount(k.astype(I64), minlength=self.num_keys).astype(U64)
            self._snap = {"state": {f: getattr(os_, f) for f in STATE_FIELDS}, "series": (ln, v.copy()), "times": t.copy() if k.size else None,
                          "history": (ln, v[np.lexsort((v, k))]) if self.flags & HIST else None}
        return self._snap

    # ---- expected rows ----
    def job(self, algo, mask=None, emit_all=False, judged=None, alpha=0.0, eps=0.0, min_samples=0, nsigma=0.0, drop_min_samples=0):
        """the rows and counters of the batch job over W' = W[mask] (tad_run_state, _window, _keys, tad_drop_state), restricted to the
        points of `judged` (a mask over W') for a stream batch.  -> (rows, counters)"""
        k, t, v = self.points()
        if mask is not None:
            k, t, v = k[mask], t[mask], v[mask]
        if algo == "DROP":
            rows, no_result = drop_oracle_rows((k, t, v), nsigma or 3.0, drop_min_samples or 3, emit_all, judged)
            n_anom = int(rows["anomaly"].sum()) if emit_all else int(rows["key_id"].size)
            return rows, {"n_anomalies": n_anom, "n_keys": int(np.unique(k).size), "n_points": int(k.size), "keys_no_result": no_result}
        want = orc.run_job(algo, k, t, v, op="sum", alpha=alpha or 0.5, eps=eps or 250000000.0, min_samples=min_samples or 4, dbscan_fn=_dbscan)
        n = np.diff(want["ptr"])
        sel = np.ones(k.size, bool) if emit_all else want["anomaly_all"].copy()
        if algo == "ARIMA":                                  # keys without a result emit nothing
            sel &= np.repeat(np.array([r is not None for r in want["arima_results"]], bool), n)
        if judged is not None:
            sel &= judged
        rows = {"key_id": k[sel], "flow_end_s": t[sel], "throughput": orc.u64_to_f64(v)[sel], "algo_calc": want["calc_all"][sel],
                "stddev": np.repeat(want["sigma"], n)[sel]}
        if emit_all:
            rows["anomaly"] = want["anomaly_all"][sel].astype(np.uint8)
        counters = {f: want[f] for f in ("n_anomalies", "n_keys", "n_points", "keys_no_result")}
        if algo == "ARIMA":
            counters["kalman_steps"] = want["kalman_steps"]
        return rows, counters

    def ewma_stream_rows(self, before, bk, bt, bv, emit_all):
        """an EWMA stream batch: the stream oracle continued from the state `before` (the `state` part of a snapshot) over the batch's
        points.  With emit_all every point carries its EWMA value, the running stddev (0.0 below two points) and its verdict."""
        st = sorc.StreamState(before["n"].size)
        for f in STATE_FIELDS:
            getattr(st, f)[:] = before[f]
        st.seen[:] = before["n"] > 0
        if not emit_all:
            return sorc.run_stream(st, bk, bt, bv, op=self.op, alpha=self.alpha_eff)
        a = self.alpha_eff
        x = orc.u64_to_f64(bv)
        calc, sig, verdict = np.zeros(x.size), np.zeros(x.size), np.zeros(x.size, np.uint8)
        cur = None
        for i, (kk, xv) in enumerate(zip(bk.tolist(), x.tolist())):
            if kk != cur:
                cur, cnt, avg, m2, e = kk, float(before["n"][kk]), float(before["avg"][kk]), float(before["m2"][kk]), float(before["ewma"][kk])
            cnt = cnt + 1.0
            d = xv - avg
            dn = d / cnt
            avg = avg + dn
            m2 = m2 + d * (d - dn)
            e = (1 - a) * e + a * xv
            calc[i] = e
            if cnt >= 2.0:
                sig[i] = float(np.sqrt(np.float64(m2 / (cnt - 1.0))))
                verdict[i] = abs(xv - e) > sig[i]
        return {"key_id": bk, "flow_end_s": bt, "throughput": x, "algo_calc": calc, "stddev": sig, "anomaly": verdict}

    def stream_rows(self, before, batch_points, algo, emit_all, params):
        """the rows of a stream batch, W already holding the batch.  EWMA: the running form; DBSCAN / ARIMA / DROP: the job over W
        restricted to the batch's new (key, time) points."""
        bk, bt, bv = batch_points
        if algo == "EWMA":
            return self.ewma_stream_rows(before, bk, bt, bv, emit_all)
        return self.job(algo, emit_all=emit_all, judged=_member(self.key, self.t, bk, bt), **params)[0]

    def check_mask(self, check):
        """the points of W a read-only check judges: its window, then its key mask"""
        m = self.window_mask(*check.get("win", (0, 0, 0)))
        if check.get("mask") is not None:
            m &= np.asarray(check["mask"])[self.key.astype(I64)] != 0
        return m

    def check_expect(self, check):
        return self.job(check["algo"], self.check_mask(check), check["emit_all"], **check["params"])


def apply(model, op, rows=True):
    """Advance `model` by one operation of a script.  -> what the call must return: {"raises": True} for a call that must fail with the
    state unchanged, else the call's own outputs (rows / stats / dropped / remap).  rows=False leaves a stream batch's rows out (the
    generator needs W alone)."""
    kind = op["kind"]
    if kind == "append":
        before = model.expected_snapshot()["state"] if rows and op["algo"] == "EWMA" else None
        pts = model.append(op["k"], op["t"], op["v"])
        return {"rows": model.stream_rows(before, pts, op["algo"], op["emit_all"], op["params"])} if rows else {}
    if kind == "late":
        try:
            model.append(op["k"], op["t"], op["v"])
        except ValueError:
            return {"raises": True}
        raise AssertionError("the script's late batch is not late")
    if kind == "merge":
        return {"stats": model.merge(op["k"], op["t"], op["v"], op["keep_from"])}
    if kind == "trim":
        return {"dropped": model.trim(op["keep_points"], op["keep_from"])}
    if kind == "compact":
        out = model.compact(op["retire_before"])
        return {"remap": out.pop("remap"), "stats": out}
    if kind == "resize":
        model.resize(op["n"])
        return {}
    if kind == "restart":
        return {}
    if kind == "refused":
        return {"raises": True}
    raise ValueError(kind)


# ---- scripts ----
def _lattice_buckets(t):
    """the buckets of the lattice (min, gcd of the differences, max) Stage 0 derives for a batch"""
    t = np.unique(t)
    if t.size < 2:
        return 1
    return int((t[-1] - t[0]) // np.gcd.reduce(np.diff(t))) + 1


class _Gen:
    """the draws of one script; `m` is the model the script is generated against"""

    def __init__(self, seed):
        self.rng = rng = np.random.default_rng(77000 + seed)
        self.seed = seed
        self.cls = CLASSES[seed % 4] if seed < 16 else CLASSES[int(rng.integers(4))]
        self.flags = SER | TIMES | (HIST if seed % 4 != 3 - (seed // 4) % 4 else 0)      # three seeds in four keep a history
        self.op = ("sum", "max")[int(rng.integers(2))]
        self.alpha = ALPHAS[int(rng.integers(len(ALPHAS)))]
        self.big = bool(rng.random() < 0.4)
        self.step = int(rng.choice([1, 7, 60]))
        self.t_base = 1_600_000_000 + int(rng.integers(0, 90_000_000))
        if self.cls in ("many", "grow-shrink-grow"):
            K = int(rng.choice([63, 64, 65, 700, 3000] if self.cls == "many" else [64, 65, 700]))
        elif self.cls == "few-long":
            K = int(rng.choice([1, 2, 3]))
        else:
            K = int(rng.choice([3, 8, 12]))
        self.K0 = K
        self.m = StateModel(K, self.flags, self.op, self.alpha)
        self.cursor = 0                    # the first bucket no point has reached yet
        self.base = 100_000_000 + rng.integers(0, 1_400_000_000, size=max(K, 3000) + 200)     # per key id, whatever the id comes to mean
        self.last_batch = None
        self.arima_left = MAX_ARIMA_CHECKS
        self.max_held = 0
        self.refusals = 0

    # -- pieces --
    def time_of(self, bucket):
        return self.t_base + self.step * np.asarray(bucket, I64)

    def values(self, keys):
        rng = self.rng
        v = self.base[keys.astype(I64) % self.base.size] + rng.integers(-300_000_000, 300_000_000, size=keys.size)
        spike = rng.random(keys.size) < 0.03
        v = np.where(spike, v * 2 + 400_000_000, v)
        v = np.clip(v, 1, 1 << 31).astype(U64)
        if self.big:
            big = rng.random(keys.size) < 0.03
            v = np.where(big, rng.integers(1 << 50, (1 << 64) - 1, size=keys.size, dtype=U64, endpoint=True), v)
        return v

    def rows_of_points(self, pk, pb):
        """raw rows of the points (key, bucket): one or two rows per point, shuffled"""
        rng = self.rng
        twice = rng.random(pk.size) < 0.3
        k = np.concatenate([pk, pk[twice]]).astype(U64)
        b = np.concatenate([pb, pb[twice]])
        o = rng.permutation(k.size)
        k, b = k[o], b[o]
        return k, self.time_of(b), self.values(k)

    def per_key_points(self, lo=None, all_keys=False):
        """(keys, points per key) of a batch the class appends; None: no room under the ceiling (or the ARIMA class's series limit)"""
        rng, K = self.rng, self.m.num_keys
        room = CEILING - self.m.key.size
        if self.cls == "few-long":
            per = int(rng.choice([5, 130, 300, 600]))
            keys = np.flatnonzero(rng.random(K) < 0.8)
        elif self.cls == "arima":
            n, _ = self.m.per_key()
            per = int(rng.integers(1, 9))
            keys = np.flatnonzero(rng.random(K) < 0.8)
            keys = keys[n[keys] + per <= ARIMA_MAX_SERIES]
        else:
            per = int(rng.integers(1, 31)) if lo is None else lo
            keys = np.arange(K) if all_keys else np.flatnonzero(rng.random(K) < float(rng.choice([1.0, 0.6, 0.15])))
            room = min(room, 12000)
        if keys.size == 0:
            keys = np.array([int(rng.integers(K))])
            if self.cls == "arima" and self.m.per_key()[0][keys[0]] + per > ARIMA_MAX_SERIES:
                return None
        per = min(per, room // keys.size)
        if per < 1:
            keys, per = keys[:room], 1
        return (keys, per) if keys.size else None

    def inorder_batch(self, lo=None, all_keys=False, exact=False):
        """rows newer than everything the state holds: each key between 1 and `per` points (exact: `per`) at buckets from the cursor on"""
        got = self.per_key_points(lo, all_keys)
        if got is None:
            return None
        keys, per = got
        rng = self.rng
        span = per if rng.random() < 0.3 else per * 2 + 1
        cnt = np.full(keys.size, per) if exact or self.cls == "few-long" else rng.integers(1, per + 1, size=keys.size)
        pick = np.argsort(rng.random((keys.size, span)), axis=1)
        take = np.arange(span)[None, :] < cnt[:, None]
        return self.rows_of_points(np.repeat(keys, cnt), self.cursor + pick[take])

    def columns(self, t):
        """where and how wide the batch's columns are, and the plan overrides it runs under"""
        rng = self.rng
        cols = str(rng.choice(["host8", "host4", "device"])) if t.size else "host8"
        sparse = ["auto", "always"] + (["never"] if _lattice_buckets(t) <= 4096 else [])
        return cols, {"sparse": str(rng.choice(sparse)), "stage0": str(rng.choice(["v1", "v2"]))}

    def batch_op(self, kind, rows, **more):
        k, t, v = rows
        cols, plan = self.columns(t)
        return dict(kind=kind, k=k, t=t, v=v, cols=cols, plan=plan, **more)

    def stream_algo(self, arima=True):
        rng = self.rng
        algo = str(rng.choice(["EWMA", "DROP"] + (["DBSCAN"] if self.flags & HIST else [])))
        if arima and self.cls == "arima" and self.arima_left and rng.random() < 0.5:
            algo = "ARIMA"
            self.arima_left -= 1
        return algo, bool(rng.random() < 0.5), self.params(algo, stream=True)

    def params(self, algo, stream=False):
        rng = self.rng
        if algo == "EWMA":
            return {} if stream else {"alpha": ALPHAS[int(rng.integers(len(ALPHAS)))]}       # a stream batch runs with the state's alpha
        if algo == "DBSCAN":
            eps, ms = DBSCAN_PARAMS[int(rng.integers(len(DBSCAN_PARAMS)))]
            return {"eps": eps, "min_samples": ms}
        if algo == "DROP":
            ns, ms = DROP_PARAMS[int(rng.integers(len(DROP_PARAMS)))]
            return {"nsigma": ns, "drop_min_samples": ms}
        return {}

    def quantile_time(self, q):
        t = self.m.t
        return int(np.sort(t)[min(int(q * t.size), t.size - 1)]) if t.size else int(self.time_of(self.cursor))

    # -- the operations --
    def append(self, lo=None, all_keys=False, exact=False):
        rows = self.inorder_batch(lo, all_keys, exact)
        if rows is None:
            return self.trim("count")
        algo, emit_all, params = self.stream_algo()
        return self.batch_op("append", rows, algo=algo, emit_all=emit_all, params=params)

    def late(self):
        n, last = self.m.per_key()
        rows = self.inorder_batch()
        if rows is None or not (n > 0).any():
            return self.append()
        rng = self.rng
        key = int(rng.choice(np.flatnonzero(n > 0)))
        variant = ("eq", "lt")[int(rng.integers(2))]
        lt = int(last[key]) - (0 if variant == "eq" else self.step * int(rng.integers(1, 4)))
        k, t, v = rows
        at = int(rng.integers(k.size + 1))
        k, t, v = np.insert(k, at, U64(key)), np.insert(t, at, lt), np.insert(v, at, U64(12345))
        algo, emit_all, params = self.stream_algo(arima=False)
        return self.batch_op("late", (k, t, v), algo=algo, emit_all=emit_all, params=params, variant=variant)

    def merge(self, variant=None):
        rng, m = self.rng, self.m
        variant = variant or str(rng.choice(["range", "range", "range_keep", "range_keep", "resend", "inorder", "inorder_keep"]))
        if variant == "resend" and self.last_batch is None:
            variant = "range"
        keep_from = 0
        if variant == "resend":
            rows = self.last_batch
        elif variant in ("inorder", "inorder_keep"):
            rows = self.inorder_batch()
            if rows is None:
                return self.trim("count")
            if variant == "inorder_keep":                          # the points at the batch's first buckets fall under the cut
                keep_from = int(self.time_of(self.cursor + 1 + int(rng.integers(3))))
        else:
            # rows over a range that starts before the oldest point and ends after the newest
            n, _ = m.per_key()
            lo = int((m.t.min() - self.t_base) // self.step) - 3 if m.t.size else self.cursor
            hi = self.cursor + 3
            nk = max(1, min(m.num_keys, 300, (CEILING - m.key.size) // 8))
            keys = rng.choice(m.num_keys, size=nk, replace=False) if CEILING - m.key.size >= 8 else np.zeros(0, I64)
            per = 1 + int(rng.integers(6)) if self.cls != "arima" else 1
            if self.cls == "arima":
                keys = keys[n[keys] + 1 <= ARIMA_MAX_SERIES]
            pk = np.repeat(keys, per)
            pb = rng.integers(lo, hi + 1, size=pk.size)
            if m.t.size and pk.size:                               # some rows at times their key already holds: they combine
                own = rng.integers(0, m.key.size, size=max(1, pk.size // 4))
                pk = np.concatenate([pk, m.key[own].astype(I64)])
                pb = np.concatenate([pb, (m.t[own] - self.t_base) // self.step])
            rows = self.rows_of_points(pk, pb)
            if variant == "range_keep":
                keep_from = int(self.time_of(lo + int(rng.integers(1, max(2, (hi - lo) // 2)))))
        return self.batch_op("merge", rows, keep_from=keep_from, variant=variant)

    def trim(self, variant=None):
        rng, m = self.rng, self.m
        variant = variant or str(rng.choice(["time", "count", "both", "neither", "hard"]))
        keep_points = keep_from = 0
        if variant in ("time", "both"):
            keep_from = self.quantile_time(float(rng.choice([0.2, 0.5, 0.8])))
        if variant in ("count", "both"):
            n, _ = m.per_key()
            keep_points = max(1, int(rng.integers(1, max(2, int(n.max()) if n.size else 2))))
        if variant == "hard":                                      # keeps under a quarter of the points
            keep_from = self.quantile_time(0.85)
        return dict(kind="trim", keep_points=keep_points, keep_from=keep_from, variant=variant)

    def compact(self, variant=None):
        rng = self.rng
        variant = variant or str(rng.choice(["unseen", "unseen", "time", "time", "everything"], p=[0.25, 0.25, 0.2, 0.2, 0.1]))
        retire = 0
        if variant == "time":
            _, last = self.m.per_key()
            seen = last[last > 0]
            retire = int(np.sort(seen)[int(rng.integers(seen.size))]) if seen.size else int(self.time_of(self.cursor))
        elif variant == "everything":
            retire = int(self.time_of(self.cursor + 1))
        return dict(kind="compact", retire_before=retire, variant=variant)

    def resize(self):
        K = self.m.num_keys
        cap = {"few-long": 3, "arima": 12}.get(self.cls, 3200)
        n = min(K + int(self.rng.choice([0, 1, 5, 64, 100])), max(cap, K))
        return dict(kind="resize", n=n)

    def refused(self):
        rng, m = self.rng, self.m
        ok = [v for v in REFUSALS if "without_history" not in v or not self.flags & HIST]
        if not self.flags & HIST and not self.refusals:       # the two refusals only a state without history has: one per such script
            ok = [ok[(self.seed // 4) % 2]]
        self.refusals += 1
        variant = str(rng.choice(ok))
        op = dict(kind="refused", variant=variant)
        if variant in ("dbscan_stream_without_history", "num_keys_differs"):
            rows = self.inorder_batch()
            if rows is None:
                variant = op["variant"] = "start_time_in_run_state"
            else:
                op = self.batch_op("refused", rows, variant=variant, emit_all=False)
                if variant == "num_keys_differs":
                    op["num_keys"] = m.num_keys + (1 if m.num_keys == 1 or rng.random() < 0.5 else -1)
        if variant == "from_after_to":
            a = self.quantile_time(0.3)
            op.update(call=str(rng.choice(["window", "drop_state"])), win=(a + 1 + int(rng.integers(100)), a, 0))
        if variant == "start_time_in_run_state":
            op.update(start_time=self.quantile_time(0.5))
        return op

    # -- the read-only checks after an operation --
    def checks(self):
        rng, m = self.rng, self.m
        algos = ["EWMA"] + (["DBSCAN"] if self.flags & HIST else [])
        first = str(rng.choice(algos))
        if self.cls == "arima" and self.arima_left and rng.random() < 0.15:
            first = "ARIMA"
            self.arima_left -= 1
        one = dict(call="run_state", algo=first, emit_all=bool(rng.random() < 0.5), params=self.params(first))
        call = str(rng.choice(["window", "keys", "drop_state", "drop_state_keys"]))
        algo = "DROP" if call.startswith("drop") else str(rng.choice(algos))
        shape = str(rng.choice(["whole", "from", "to", "both", "keep", "from_keep", "all_but_newest", "newest", "empty"],
                               p=[0.16, 0.1, 0.1, 0.12, 0.1, 0.1, 0.14, 0.12, 0.06]))
        f = t = kp = 0
        if shape in ("from", "both", "from_keep"):
            f = self.quantile_time(float(rng.choice([0.1, 0.4, 0.7])))
        if shape in ("to", "both"):
            t = max(self.quantile_time(float(rng.choice([0.5, 0.8, 0.95]))), f)
        if shape in ("keep", "from_keep"):
            kp = int(rng.choice([1, 2, 5, 20, 200]))
        if shape == "all_but_newest":
            t = self.quantile_time(0.97)
        if shape == "newest":
            f = self.quantile_time(0.9)
        if shape == "empty":
            f = t = self.quantile_time(0.5)
        two = dict(call=call, algo=algo, emit_all=bool(rng.random() < 0.5), params=self.params(algo), win=(f, t, kp), shape=shape)
        if call.endswith("keys"):
            K = m.num_keys
            how = str(rng.choice(["ones", "zeros", "half", "one", "none"], p=[0.2, 0.2, 0.3, 0.2, 0.1]))
            two["mask_kind"] = how
            two["mask"] = {"ones": np.ones(K, np.uint8), "zeros": np.zeros(K, np.uint8), "half": (rng.random(K) < 0.5).astype(np.uint8),
                           "one": (np.arange(K) == int(rng.integers(K))).astype(np.uint8), "none": None}[how]
        wm = m.window_mask(f, t, kp)
        two["info"] = {"window_points": int(wm.sum()), "state_points": int(m.key.size), "cut": bool(m.key.size and not wm.all()),
                       "whole": bool(m.key.size and wm.all())}
        return [one, two]

    # -- the script --
    def plan(self):
        """the kinds of the script's operations, in order"""
        rng = self.rng
        if self.cls == "grow-shrink-grow":
            kinds = ["append_few", "append_few", "append_few", "hard_trim", "compact_unseen", "resize_back", "append_all", "append_all", "append_all"]
            kinds += [str(rng.choice(KINDS[1:])) for _ in range(N_OPS - len(kinds))]
            if not self.flags & HIST:
                kinds[-1 - (self.seed // 4) % 3] = "refused"
            return kinds
        kinds = [str(rng.choice(KINDS, p=[0.22, 0.1, 0.2, 0.12, 0.1, 0.08, 0.08, 0.1])) for _ in range(N_OPS)]
        if self.seed % 4:
            kinds[0] = "append"            # one script in four starts on the empty state with whatever was drawn
        if not self.flags & HIST:
            kinds[-1 - (self.seed // 4) % 3] = "refused"
        return kinds

    def draw(self, kind):
        if kind == "hard_trim":
            return self.trim("hard")
        if kind == "compact_unseen":
            return self.compact("unseen")
        if kind == "append_few":
            return self.append(lo=8)
        if kind == "append_all":
            return self.append(lo=30, all_keys=True, exact=True)
        if kind == "resize_back":
            return dict(kind="resize", n=max(self.K0, self.m.num_keys) + (5 if self.cls in ("many", "grow-shrink-grow") else 0))
        return getattr(self, kind)() if kind != "restart" else dict(kind="restart")

    def script(self):
        ops = []
        for kind in self.plan():
            m = self.m
            if m.num_keys * 2 < self.K0 and kind != "resize_back":       # a compaction took most keys: the host's new keys get new ids
                kind = "resize_back"
            op = self.draw(kind)
            n0, _ = m.per_key()
            held0 = m.key.size
            out = apply(m, op, rows=False)
            op["info"] = info = {"held_before": int(held0), "keys_before": int(n0.size)}
            if op["kind"] in ("append", "merge") and op["k"].size:
                self.cursor = max(self.cursor, int((op["t"].max() - self.t_base) // self.step) + 1)
                self.last_batch = (op["k"], op["t"], op["v"])
            if op["kind"] == "merge":
                info.update(out["stats"])
            if op["kind"] == "trim":
                n1, _ = m.per_key()
                info.update(dropped=out["dropped"], keys_emptied=int(((n0 > 0) & (n1 == 0)).sum()))
            if op["kind"] == "compact":
                info.update(out["stats"])
                self.last_batch = None                       # its key ids are the old numbering's
            info["held_after"] = int(m.key.size)
            self.max_held = max(self.max_held, m.key.size)
            assert m.key.size <= CEILING
            op["checks"] = self.checks()
            ops.append(op)
        return ops


def make_script(seed):
    """-> {"seed", "class", "num_keys", "flags", "op", "alpha", "ops"}: a function of the seed alone"""
    g = _Gen(seed)
    ops = g.script()
    return {"seed": seed, "class": g.cls, "num_keys": g.K0, "flags": g.flags, "op": g.op, "alpha": g.alpha, "ops": ops}


def describe(op):
    """an operation without its columns, for assertion messages"""
    return {k: (v if not isinstance(v, np.ndarray) else "%s[%d]" % (v.dtype, v.size)) for k, v in op.items() if k not in ("checks", "info")}
