"""A numpy model of tad_run_state_buckets' view (include/tad.h): the floor of the times, the fold of every key's runs and the since rule,
written independently of both the kernels and the oracle's Stage 0.  tests/test_buckets_model.py holds it against oracle.tad_oracle.stage0
over the floored rows; the GPU tests use it for the host-side numbers every case asserts before the engine is asked."""
import numpy as np
from state_helpers import I64, U64

NO_CHANGE = (1 << 63) - 1


def bucket_start(t, bucket_s, origin=0):
    """origin + bucket_s * floor((t - origin) / bucket_s); numpy's // on int64 is the floor division"""
    t = np.asarray(t, I64)
    return I64(origin) + I64(bucket_s) * ((t - I64(origin)) // I64(bucket_s))


def run_lengths(k, t, bucket_s, origin=0):
    """rows in (key, time) order -> (index of every run's first row, the runs' lengths): a run = the rows of one key in one bucket"""
    k = np.asarray(k, U64)
    b = bucket_start(t, bucket_s, origin)
    if k.size == 0:
        return np.zeros(0, I64), np.zeros(0, I64)
    head = np.ones(k.size, bool)
    head[1:] = (k[1:] != k[:-1]) | (b[1:] != b[:-1])
    first = np.flatnonzero(head)
    return first, np.diff(np.append(first, k.size))


def fold(k, t, v, bucket_s, origin=0, op="sum"):
    """rows in (key, time) order, one per point -> the buckets (key, bucket start, folded value) in (key, time) order.  sum wraps mod
    2^64, max is unsigned"""
    k, v = np.asarray(k, U64), np.asarray(v, U64)
    first, _ = run_lengths(k, t, bucket_s, origin)
    if first.size == 0:
        return np.zeros(0, U64), np.zeros(0, I64), np.zeros(0, U64)
    with np.errstate(over="ignore"):
        val = np.add.reduceat(v, first) if op == "sum" else np.maximum.reduceat(v, first)
    return k[first], bucket_start(t, bucket_s, origin)[first], val.astype(U64)


def reported(k, bstart, bucket_s, origin=0, since_t=0, key_since=None):
    """the since rule on buckets (key, bucket start): reported iff the start >= the start of the threshold's bucket, the threshold being the
    larger of since_t (0: none) and key_since[key] (None: none; NO_CHANGE: the key is not selected)"""
    k = np.asarray(k, U64)
    bstart = np.asarray(bstart, I64)
    m = np.ones(k.size, bool)
    if since_t:
        m &= bstart >= bucket_start(since_t, bucket_s, origin)
    if key_since is not None:
        ks = np.asarray(key_since, I64)[k.astype(I64)]
        sel = ks != NO_CHANGE
        thr = bucket_start(np.where(sel, ks, 0), bucket_s, origin)
        m &= sel & (bstart >= thr)
    return m
