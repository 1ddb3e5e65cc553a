"""GPU: every Stage 0 reader of the caller's rows judges a row alike (theia_amd/csrc/tad_rows.h).  One seeded table holds every kind of
row — a skip key on either side and on both, a second key column with skips of its own, rows before start_time and at or after end_time,
duplicates of one (key, time), a value >= 2^40 for `max` — and goes through Stage 0 alone (engine.aggregate) under each plan of
test_gpu_narrow_columns.PLANS, for sum and max, at 64/64-bit and 32/32-bit columns, as device columns 16-byte aligned and offset by one
element, and as host columns, with and without the time window.  Points and rows_used equal a numpy group-by written here, bit for bit; stage0_path shows
that the forced path ran; one row with key = num_keys makes the job TAD_ERR_KEY_RANGE; a lattice hint that misses one row gives the points
of no hint."""
import numpy as np
import pytest

from theia_amd import TadError
from theia_amd import _capi as capi
from job_helpers import PLANS, SKIP64, narrow_key, plan  # noqa: F401  (plan: the fixture)

pytestmark = pytest.mark.gpu

# 256 workgroups of pass A / pass B get 392 rows each (the last one 41): ragged tiles everywhere and, the count being odd, the single last
# row of the 16-byte readers; 391 blocks of k_meta / k_scatter / k_sparse_keys.  (A full tile of pass B needs 2048 rows per workgroup:
# test_gpu_dense_boundaries has those.)
N, K, T, T0, STEP = 100_001, 3000, 120, 1_700_000_000, 60
START, END = T0 + 10 * STEP, T0 + 100 * STEP          # the window: flowStartSeconds >= START and flowEndSeconds < END


def make_table(op):
    rng = np.random.default_rng(20)
    k = rng.integers(0, K, N, dtype=np.uint64)
    k2 = rng.integers(0, K, N, dtype=np.uint64)
    kind = rng.random(N)
    k[kind < 0.10] = SKIP64                              # skip on the first side only,
    k2[(kind >= 0.05) & (kind < 0.30)] = SKIP64          # on both (0.05 .. 0.10), on the second only
    t = (T0 + STEP * rng.integers(0, T - 1, N)).astype(np.int64)
    ts = (t - STEP * rng.integers(0, 12, N)).astype(np.int64)   # some start before START, some rows end at or after END
    v = rng.integers(0, 1 << 40, N, dtype=np.uint64)
    dup = rng.integers(0, N, 2000)                       # duplicates of one (key, time), beyond those chance brings
    k[dup[1000:]], k2[dup[1000:]], t[dup[1000:]] = k[dup[:1000]], k2[dup[:1000]], t[dup[:1000]]
    # the first and the last bucket exist, the last one in exactly ONE row (what a lattice hint one bucket short misses); its start time
    # lies before the window, so the windowed job drops it
    t[7], ts[7], k[7], k2[7] = T0, T0, 5, 6
    t[N - 2], ts[N - 2], k[N - 2], k2[N - 2] = T0 + STEP * (T - 1), T0, 17, SKIP64
    k[N - 1], k2[N - 1] = 2999, 0                        # the single last row is live on both sides
    # edges of the window and of the key range
    t[100], ts[100] = END, START
    t[101], ts[101] = END - STEP, START
    t[102], ts[102] = END - STEP, START - 1
    k[103], k2[104] = K - 1, K - 1
    if op == "max":                                      # values that fit no packed record (overflow list), and the first that may not
        v[[11, 5000, N - 1]] = np.array([1 << 40, (1 << 63) + 5, (1 << 64) - 1], dtype=np.uint64)
        v[[12, 5001]] = np.array([(1 << 32) - 2, (1 << 32) - 1], dtype=np.uint64)
    return dict(key_id=k, key_id2=k2, flow_end_s=t, flow_start_s=ts, value=v)


def group_by(tab, op, window):
    """GROUP BY (key, flowEndSeconds) in numpy: points sorted by (key, t), and the number of (row, side) slots that took part."""
    keep = np.ones(N, dtype=bool)
    if window:
        keep &= (tab["flow_start_s"] >= START) & (tab["flow_end_s"] < END)
    sides = [keep & (tab[c] != SKIP64) for c in ("key_id", "key_id2")]
    kk = np.concatenate([tab[c][m] for c, m in zip(("key_id", "key_id2"), sides)])
    tt = np.concatenate([tab["flow_end_s"][m] for m in sides])
    vv = np.concatenate([tab["value"][m] for m in sides])
    order = np.lexsort((tt, kk))
    kk, tt, vv = kk[order], tt[order], vv[order]
    first = np.ones(kk.size, dtype=bool)
    first[1:] = (kk[1:] != kk[:-1]) | (tt[1:] != tt[:-1])
    starts = np.flatnonzero(first)
    with np.errstate(over="ignore"):
        agg = np.add.reduceat(vv, starts) if op == "sum" else np.maximum.reduceat(vv, starts)
    assert starts.size < kk.size                         # there are duplicates to fold
    return kk[starts], tt[starts], agg.astype(np.uint64), int(kk.size)


_cache = {}


def reference(op, window):
    """The table of `op` and its points with / without the window: computed once, never written to."""
    if op not in _cache:
        tab = make_table(op)
        for a in tab.values():
            a.setflags(write=False)
        _cache[op] = (tab, {w: group_by(tab, op, w) for w in (False, True)})
    tab, refs = _cache[op]
    return tab, refs[window]


def at_width(name, a, bits):
    if bits == 32 and name in ("key_id", "key_id2"):
        return narrow_key(a)
    if bits == 32 and name in ("flow_end_s", "flow_start_s"):
        return a.astype(np.uint32)
    return a


def host_columns(tab, bits):
    """numpy columns at 64/64 or 32/32 bits: the engine stages them into its own (16-byte aligned) device buffers.  These cases need no
    torch device, so they also run on a library that executes the kernels on the host."""
    return {name: at_width(name, a, bits).copy() for name, a in tab.items()}


def device_columns(tab, bits, off):
    """torch CUDA columns at 64/64 or 32/32 bits; off = 1: every column starts one element into its allocation (no 16-byte alignment)."""
    import torch
    out = {}
    for name, a in tab.items():
        a = at_width(name, a, bits)
        dt = {8: (np.int64, torch.int64), 4: (np.int32, torch.int32)}[a.dtype.itemsize]
        buf = torch.zeros(N + off, dtype=dt[1], device="cuda")
        buf[off:] = torch.from_numpy(a.view(dt[0]).copy()).cuda()
        assert (buf[off:].data_ptr() % 16 == 0) == (off == 0)
        out[name] = buf[off:]
    torch.cuda.synchronize()         # (the copies ran on torch's stream; the engine reads on its own)
    return out


def expected_paths(p, op, aligned):
    """tad_stats.stage0_path of the plan (tad.h): 1 scatter, 2 sort-by-tile pass B, 3 write-combining pass B, 4 LSD sort, 8 partition sort,
    7 the LSD sort's point list handed out as it is (tad_aggregate on a table run by length classes)."""
    if p.get("sparse_classes") == "always":
        return {7}                                       # (no stage0=v2 in that plan: no pass A, so no partition sort)
    if p.get("sparse") == "always":
        if p.get("sparse_sort") == "partition":
            # needs the write-combining pass B (16-byte loads); a value that fits no record hands the job to the LSD sort
            return {8} if aligned and op == "sum" else ({8, 4} if aligned else {4})
        return {4}
    if p.get("stage0") == "v2":
        pp = p.get("partition_pass")
        if pp == "sort":
            return {2}
        if pp in ("wc", "wc_sectors"):
            return {3} if aligned else {2}               # unaligned columns: the row-by-row sort-by-tile pass
        return {2, 3} if aligned else {2}                # the plan picks the pass from the shape
    return {1}                                           # 100 001 rows on a 3000 x 120 grid: dense, below the v2 threshold


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("op", ["sum", "max"])
@pytest.mark.parametrize("p", PLANS, ids=lambda p: "-".join("%s=%s" % kv for kv in p.items()) or "auto")
def test_every_reader_judges_every_kind_of_row_alike(engine, plan, p, op, mem):
    plan(**p)
    for bits in (64, 32):
        for off in ((0, 1) if mem == "device" else (0,)):
            tab0 = reference(op, False)[0]
            cols = device_columns(tab0, bits, off) if mem == "device" else host_columns(tab0, bits)
            for window in (False, True):
                tab, (pk, pt, pv, used) = reference(op, window)
                what = (bits, off, window)
                kw = dict(num_keys=K, agg_flow="pod", value_op=op, **cols)
                if window:
                    kw.update(start_time=START, end_time=END)
                got = engine.aggregate(**kw)
                assert got.n_points == pk.size, what
                assert np.array_equal(got["key_id"], pk) and np.array_equal(got["flow_end_s"], pt) and np.array_equal(got["value"], pv), what
                assert got.stats["rows_used"] == used, what
                assert got.stats["stage0_path"] in expected_paths(p, op, off == 0), (what, got.stats["stage0_path"])
                # a hint one bucket short misses the one row of the last bucket (without the window; the window drops that row itself)
                hinted = engine.aggregate(lattice=(T0, STEP, T - 1), **kw)
                assert hinted.n_points == pk.size and hinted.stats["rows_used"] == used, what
                assert np.array_equal(hinted["key_id"], pk) and np.array_equal(hinted["flow_end_s"], pt) and np.array_equal(hinted["value"], pv), what


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("p", PLANS, ids=lambda p: "-".join("%s=%s" % kv for kv in p.items()) or "auto")
def test_one_key_out_of_range_fails_every_plan(engine, plan, p, mem):
    plan(**p)
    for side, row in (("key_id", 40_000), ("key_id2", N - 1)):
        bad = {name: a.copy() for name, a in reference("sum", False)[0].items()}
        bad[side][row] = K                               # = num_keys
        bad["flow_end_s"][row], bad["flow_start_s"][row] = END - STEP, START      # inside the window
        for bits, off in ((64, 0), (32, 1)):
            cols = device_columns(bad, bits, off) if mem == "device" else host_columns(bad, bits)
            for kw in ({}, dict(start_time=START, end_time=END)):
                with pytest.raises(TadError) as e:
                    engine.aggregate(num_keys=K, agg_flow="pod", value_op="sum", **cols, **kw)
                assert e.value.code == capi.TAD_ERR_KEY_RANGE, (side, bits, off, kw)
