"""GPU: streaming EWMA (tad_run_stream) on second-resolution batches.  A stream batch takes the sparse Stage 0 where tad_run
would (tad_stats.stage0_path 4 = LSD sort, 8 = partition pass + LDS sort) and k_stream_points walks the sorted unique points per
key: no K x span grid, no length classes.  Rows must equal oracle/stream_oracle.py batch by batch, and after the last batch the
state must equal the batch job's statistics over the concatenated table bit for bit (as tests/test_gpu_stream.py).  The state
grows (tad_state_resize) and survives a restart (tad_state_export -> tad_state_import)."""
import numpy as np
import pytest

from oracle import stream_oracle as so
from oracle import tad_oracle as orc
from theia_amd import TadEngine, TadError
from state_helpers import ROW_FIELDS, STATE_FIELDS, T_BASE

pytestmark = pytest.mark.gpu

PLANS = ({"sparse": "never"}, {"sparse": "always", "sparse_sort": "lsd"}, {"sparse": "always", "sparse_sort": "partition", "stage0": "v2"})


def second_table(K, pts_per_key, rows_per_point, seed, span=86400, t_base=T_BASE):
    """second-resolution timestamps anywhere in `span` seconds (gcd 1), a few rows per (key, second), rows shuffled"""
    rng = np.random.default_rng(seed)
    pts = np.broadcast_to(np.asarray(pts_per_key, dtype=np.int64), (K,))
    pk = np.repeat(np.arange(K, dtype=np.uint64), pts)
    pt = t_base + rng.integers(0, span, size=pk.size).astype(np.int64)
    base = 1_000_000_000 + (orc.mix64(pk + np.uint64(5)) % np.uint64(3_000_000_000)).astype(np.int64)
    k = np.repeat(pk, rows_per_point)
    t = np.repeat(pt, rows_per_point)
    v = (np.repeat(base, rows_per_point) + rng.integers(-1_000_000, 1_000_000, size=k.size)).astype(np.uint64)
    v = np.where(rng.random(k.size) < 2e-3, v * np.uint64(7), v)
    order = rng.permutation(k.size)
    return k[order], t[order], v[order]


def cut(t, width, t_base=T_BASE):
    """batch index of every row: consecutive windows of `width` seconds"""
    return (t - t_base) // width


def oracle_batches(K, batches, op="sum"):
    ost = so.StreamState(K)
    rows = [so.run_stream(ost, k, t, v, op) for k, t, v in batches]
    return rows, ost


def assert_result_rows(got, want, what=""):
    assert got.n_rows == want["key_id"].size, (what, got.n_rows, want["key_id"].size)
    for f in ROW_FIELDS:
        assert (got[f] == want[f]).all(), (what, f)


def assert_state(state, ost):
    for f in STATE_FIELDS:
        assert (state[f] == getattr(ost, f)).all(), f


def assert_batch_job_stats(state, k, t, v, op="sum"):
    """the state equals the batch job's stddev_samp and final EWMA over the concatenated table (tests/test_gpu_stream.py)"""
    pk, pt, pv = orc.stage0(k, t, v, op)
    keys, ptr = orc.series_offsets(pk)
    xf = orc.u64_to_f64(pv)
    sigma, has = orc.stddev_samp_all(xf, ptr)
    ew = orc.ewma_all(xf, ptr)
    kk = keys.astype(np.int64)
    n = state["n"][kk].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        stream_sigma = np.sqrt(state["m2"][kk] / (n - 1.0))
    assert (np.diff(ptr) == state["n"][kk]).all()
    assert (stream_sigma[has] == sigma[has]).all()
    assert (state["ewma"][kk] == ew[ptr[1:] - 1]).all()


def stream_all(engine, K, batches, agg_flow="svc", **kw):
    st = engine.state_create(K)
    res = [engine.run_stream(st, k, t, v, agg_flow=agg_flow, **kw) for k, t, v in batches]
    state = st.export()
    st.close()
    return res, state


# ---- a day of 20 000 keys (50 points a key, 3 rows a point) in 24 hourly batches ----
@pytest.fixture(scope="module")
def day():
    K = 20000
    k, t, v = second_table(K, 50, 3, seed=31)
    b = cut(t, 3600)
    batches = [(k[b == h], t[b == h], v[b == h]) for h in range(24)]
    rows, ost = oracle_batches(K, batches)
    return K, (k, t, v), batches, rows, ost


def test_day_in_hourly_batches(engine, day):
    K, (k, t, v), batches, want, ost = day
    st = engine.state_create(K)
    for h, ((bk, bt, bv), w) in enumerate(zip(batches, want)):
        got = engine.run_stream(st, bk, bt, bv, agg_flow="svc")
        assert got.stats["stage0_path"] in (4, 8), (h, got.stats["stage0_path"])
        assert got.stats["step"] == 1 and got.stats["t0"] == bt.min() and got.stats["n_buckets"] == bt.max() - bt.min() + 1
        assert got.stats["n_points"] == np.unique(np.stack([bk.astype(np.int64), bt]), axis=1).shape[1]
        assert_result_rows(got, w, h)
    state = st.export()
    st.close()
    assert_state(state, ost)
    assert_batch_job_stats(state, k, t, v)


def test_whole_day_batch_where_the_dense_grid_does_not_fit(day):
    """20 000 keys x 86 400 s: the dense stream grid needs 15.6 GB; the sparse sort buffers (32 B a row slot) fit 512 MB"""
    K, (k, t, v), _, _, _ = day
    want_state = so.StreamState(K)
    want = so.run_stream(want_state, k, t, v, "sum")
    eng = TadEngine(device=0, workspace_limit=512 << 20)
    try:
        st = eng.state_create(K)
        got = eng.run_stream(st, k, t, v, agg_flow="svc")
        assert got.stats["stage0_path"] in (4, 8)
        assert_result_rows(got, want)
        assert_state(st.export(), want_state)
        st.close()
    finally:
        eng.close()


def test_forced_forms_agree_on_second_batches(engine):
    K = 3000
    k, t, v = second_table(K, 20, 3, seed=32, span=6 * 3600)
    b = cut(t, 3600)
    batches = [(k[b == h], t[b == h], v[b == h]) for h in range(6)]
    want, ost = oracle_batches(K, batches)
    outs = []
    for plan, paths in zip(PLANS, ((1, 2, 3), (4,), (8,))):
        with engine.plan(**plan):
            res, state = stream_all(engine, K, batches)
        for h, (r, w) in enumerate(zip(res, want)):
            assert r.stats["stage0_path"] in paths, (plan, h, r.stats["stage0_path"])
            assert_result_rows(r, w, (plan, h))
        assert_state(state, ost)
        outs.append(state)
    for f in STATE_FIELDS:
        assert (outs[0][f] == outs[1][f]).all() and (outs[0][f] == outs[2][f]).all()


@pytest.mark.parametrize("n_rows,K,T,cuts", [(60000, 200, 120, (40, 80)), (500000, 3000, 250, (50, 51, 200)), (3000, 7, 64, (1, 2, 3, 60))])
def test_forced_forms_agree_on_lattice_batches(engine, n_rows, K, T, cuts):
    """the lattice tables of tests/test_gpu_stream.py under the three forms: identical rows and state"""
    k, t, v = orc.synth_rows(0, n_rows, K, T)
    bucket = (t - orc.SYNTH_T_BASE) // orc.SYNTH_T_STEP
    edges = (0,) + tuple(cuts) + (T,)
    batches = [(k[(bucket >= lo) & (bucket < hi)], t[(bucket >= lo) & (bucket < hi)], v[(bucket >= lo) & (bucket < hi)])
               for lo, hi in zip(edges[:-1], edges[1:])]
    runs = []
    for plan in PLANS:
        with engine.plan(**plan):
            runs.append(stream_all(engine, K, batches))
    (r0, s0) = runs[0]
    for res, state in runs[1:]:
        assert all(r.stats["stage0_path"] in (4, 8) for r in res)
        for a, b in zip(r0, res):
            assert a.n_rows == b.n_rows and all((a[f] == b[f]).all() for f in ROW_FIELDS)
        for f in STATE_FIELDS:
            assert (s0[f] == state[f]).all(), f
    assert_batch_job_stats(s0, k, t, v)


def test_skewed_lengths_take_no_length_classes():
    """one key with a point every second of the hour next to 1e5 keys with 1..3 points, 1 GB of workspace: tad_run's rank grid
    (1e5 x 3600 x 17 B = 6.1 GB) would need length classes and the dense stream grid (3.2 GB) does not fit"""
    rng = np.random.default_rng(33)
    K = 100_001
    n_k = rng.integers(1, 4, size=K)
    n_k[777] = 3600
    pk = np.repeat(np.arange(K, dtype=np.uint64), n_k)
    pt = np.concatenate([np.arange(3600) if n == 3600 else rng.choice(3600, size=n, replace=False) for n in n_k]).astype(np.int64) + T_BASE
    v = (2_000_000_000 + rng.integers(-3_000_000, 3_000_000, size=pk.size)).astype(np.uint64)
    v = np.where(rng.random(pk.size) < 0.01, v * np.uint64(6), v)
    order = rng.permutation(pk.size)
    k, t, v = pk[order], pt[order], v[order]
    # a first batch an hour earlier for half the keys: the running state carries into the skewed batch
    k0, t0, v0 = k[::2], t[::2] - 3600, v[::2]
    want, ost = oracle_batches(K, [(k0, t0, v0), (k, t, v)])
    eng = TadEngine(device=0, workspace_limit=1 << 30)
    try:
        st = eng.state_create(K)
        for (bk, bt, bv), w in zip([(k0, t0, v0), (k, t, v)], want):
            got = eng.run_stream(st, bk, bt, bv, agg_flow="svc")
            assert got.stats["stage0_path"] in (4, 8)
            assert_result_rows(got, w)
        assert_state(st.export(), ost)
        st.close()
    finally:
        eng.close()


def test_big_batch_takes_the_partition_path_unforced(engine):
    """>= 2^22 rows: pass A's key-bin histogram, the partition pass + LDS sort (stage0_path 8) without any plan override"""
    K = 100_000
    k, t, v = second_table(K, 15, 3, seed=34, span=3600)
    assert k.size >= 1 << 22
    want, ost = oracle_batches(K, [(k, t, v)])
    st = engine.state_create(K)
    got = engine.run_stream(st, k, t, v, agg_flow="svc")
    assert got.stats["stage0_path"] == 8
    assert_result_rows(got, want[0])
    assert_state(st.export(), ost)
    st.close()


@pytest.mark.parametrize("plan", PLANS[1:], ids=["lsd", "partition"])
def test_pod_mode_two_keys_per_row(engine, plan):
    K = 2000
    k, t, v = second_table(K, 30, 2, seed=35, span=3 * 3600)
    k2 = np.random.default_rng(36).integers(0, K, size=k.size).astype(np.uint64)
    b = cut(t, 3600)
    sel = [b == h for h in range(3)]
    # the oracle sees every row twice: once under each of its keys
    want, ost = oracle_batches(K, [(np.concatenate([k[s], k2[s]]), np.concatenate([t[s], t[s]]), np.concatenate([v[s], v[s]])) for s in sel])
    with engine.plan(**plan):
        st = engine.state_create(K)
        for s, w in zip(sel, want):
            got = engine.run_stream(st, k[s], t[s], v[s], agg_flow="pod", key_id2=k2[s])
            assert got.stats["stage0_path"] in (4, 8)
            assert_result_rows(got, w)
        assert_state(st.export(), ost)
        st.close()


def test_emit_all_points(engine, day):
    K, _, batches, want, _ = day
    with engine.plan(sparse="always"):
        st = engine.state_create(K)
        for (bk, bt, bv), w in list(zip(batches, want))[:4]:
            got = engine.run_stream(st, bk, bt, bv, agg_flow="svc", emit_all=True)
            pk, pt, pv = orc.stage0(bk, bt, bv, "sum")
            assert got.n_rows == pk.size                                      # one row per new point, (key, time) order
            assert (got["key_id"] == pk).all() and (got["flow_end_s"] == pt).all() and (got["throughput"] == orc.u64_to_f64(pv)).all()
            a = got["anomaly"].astype(bool)
            assert a.sum() == w["key_id"].size
            for f in ROW_FIELDS:
                assert (got[f][a] == w[f]).all(), f
        st.close()


@pytest.mark.parametrize("plan", PLANS[1:], ids=["lsd", "partition"])
def test_late_first_point_rejected_state_kept(engine, plan):
    K = 3000
    k, t, v = second_table(K, 20, 2, seed=37, span=7200)
    b = cut(t, 3600)
    with engine.plan(**plan):
        st = engine.state_create(K)
        engine.run_stream(st, k[b == 0], t[b == 0], v[b == 0], agg_flow="svc")
        before = st.export()
        bk, bt, bv = k[b == 1], t[b == 1], v[b == 1]
        # a seen key's first point of the batch is no newer than its last_t (every other point of the batch is newer)
        kk = int(np.flatnonzero(before["n"] > 0)[7])
        late = (np.array([kk], np.uint64), np.array([before["last_t"][kk]], np.int64), np.array([5], np.uint64))
        with pytest.raises(TadError) as ei:
            engine.run_stream(st, np.concatenate([bk, late[0]]), np.concatenate([bt, late[1]]), np.concatenate([bv, late[2]]), agg_flow="svc")
        assert ei.value.code == -1 and "not newer" in ei.value.message
        assert all((st.export()[f] == before[f]).all() for f in STATE_FIELDS)
        engine.run_stream(st, k[:0], t[:0], v[:0], agg_flow="svc")          # an empty batch changes nothing
        assert all((st.export()[f] == before[f]).all() for f in STATE_FIELDS)
        got = engine.run_stream(st, bk, bt, bv, agg_flow="svc")             # the batch without the late row is fine
        assert got.stats["stage0_path"] in (4, 8)
        st.close()
    want, _ = oracle_batches(K, [(k[b == 0], t[b == 0], v[b == 0]), (bk, bt, bv)])
    assert_result_rows(got, want[1])


def test_resize_as_keys_appear(engine):
    """ids in order of first appearance: key k first shows in hour k * 12 // K; the state grows before every batch and ends equal to
    a state sized to the final key space from the start"""
    K = 6000
    k, t, v = second_table(K, 40, 2, seed=38, span=12 * 3600)
    b = cut(t, 3600)
    keep = b >= (k.astype(np.int64) * 12 // K)
    k, t, v, b = k[keep], t[keep], v[keep], b[keep]
    batches = [(k[b == h], t[b == h], v[b == h]) for h in range(12)]
    want, ost = oracle_batches(K, batches)
    with engine.plan(sparse="always"):
        st = engine.state_create(int(batches[0][0].max()) + 1)
        for h, ((bk, bt, bv), w) in enumerate(zip(batches, want)):
            old = st.num_keys
            st.resize(max(old, int(bk.max()) + 1))
            if st.num_keys > old:
                with pytest.raises(TadError) as ei:                              # a batch that still declares the old key space
                    engine.run_stream(st, bk[:0], bt[:0], bv[:0], agg_flow="svc", num_keys=old)
                assert ei.value.code == -1 and "must be equal" in ei.value.message
            got = engine.run_stream(st, bk, bt, bv, agg_flow="svc")
            assert_result_rows(got, w, h)
        assert st.num_keys == K
        before = st.export()
        with pytest.raises(TadError) as ei:                                      # a state never shrinks
            st.resize(K - 1)
        assert ei.value.code == -1 and st.num_keys == K
        assert all((st.export()[f] == before[f]).all() for f in STATE_FIELDS)
        assert_state(before, ost)
        st.close()


def test_export_import_round_trip(day):
    """stream half the day, export, close the engine; a fresh engine loads the state and streams the rest: rows and final state equal
    those of an uninterrupted run"""
    K, (k, t, v), batches, want, ost = day
    eng = TadEngine(device=0)
    st = eng.state_create(K)
    for (bk, bt, bv), w in zip(batches[:12], want[:12]):
        assert_result_rows(eng.run_stream(st, bk, bt, bv, agg_flow="svc"), w)
    saved = st.export()
    st.close()
    eng.close()
    eng = TadEngine(device=0)
    try:
        st = eng.state_create(K)
        st.load(saved)
        assert all((st.export()[f] == saved[f]).all() for f in STATE_FIELDS)
        for (bk, bt, bv), w in zip(batches[12:], want[12:]):
            assert_result_rows(eng.run_stream(st, bk, bt, bv, agg_flow="svc"), w)
        assert_state(st.export(), ost)
        st.close()
    finally:
        eng.close()


def test_imported_unseen_keys(engine):
    """keys imported with n == 0 are unseen whatever the other fields say: stored as zeros, their first batch is not late"""
    K = 500
    k, t, v = second_table(K, 20, 2, seed=39, span=7200)
    b = cut(t, 3600)
    batches = [(k[b == h], t[b == h], v[b == h]) for h in range(2)]
    ref = engine.state_create(K)
    engine.run_stream(ref, *batches[0], agg_flow="svc")
    saved = ref.export()
    ref.close()
    odd = np.arange(K) % 2 == 1
    fresh = so.StreamState(K)                                          # the odd keys start over in the oracle
    doctored = {f: saved[f].copy() for f in STATE_FIELDS}
    doctored["n"][odd] = 0
    doctored["avg"][odd], doctored["ewma"][odd], doctored["last_t"][odd] = 1e300, -3.0, np.int64(1) << 62
    st = engine.state_create(K)
    st.load(doctored)
    got_state = st.export()
    for f in STATE_FIELDS:
        assert (got_state[f][odd] == 0).all() and (got_state[f][~odd] == saved[f][~odd]).all(), f
    for f in STATE_FIELDS:
        getattr(fresh, f)[~odd] = saved[f][~odd]
    fresh.seen[:] = fresh.n > 0
    w = so.run_stream(fresh, *batches[1], "sum")
    assert_result_rows(engine.run_stream(st, *batches[1], agg_flow="svc"), w)
    assert_state(st.export(), fresh)
    st.close()
