// tad_bucket.h — the time arithmetic of tad_run_state_buckets and tad_state_rollup (include/tad.h), in one place: the kernels of
// tad_window.hip, the host checks of tad_capi_view.cpp and tad_capi_state.cpp and two stand-alone programs (tests/test_bucket_host.py,
// tests/test_rollup_host.py) all include this header and nothing else computes a bucket.  Plain C++: no HIP, no engine types.
//
// A bucket is [start, start + bucket_s) with start = origin + bucket_s * floor((t - origin) / bucket_s): FLOOR division, so a time below
// the origin (below zero too) rounds down, never towards zero.  Documented domain: |t| < 2^62, 1 <= bucket_s <= 2^40, 0 <= origin <
// bucket_s; inside it the result is the mathematical floor.  Outside it nothing is undefined: the subtraction and everything after it are
// done in uint64_t, so the result wraps mod 2^64 (and is then whatever that gives, consistently on host and device).
#ifndef THEIA_TAD_BUCKET_H
#define THEIA_TAD_BUCKET_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TAD_BUCKET_FN __host__ __device__ inline
#else
#define TAD_BUCKET_FN inline
#endif

namespace tad {

static constexpr int64_t kBucketMaxSeconds = (int64_t)1 << 40;   // the largest bucket_s of the documented domain

// what tad_run_state_buckets refuses of the two numbers (bucket_s above kBucketMaxSeconds is accepted: the result wraps, see above)
TAD_BUCKET_FN bool bucket_args_ok(int64_t bucket_s, int64_t origin) { return bucket_s >= 1 && origin >= 0 && origin < bucket_s; }

// the start of t's bucket; bucket_s >= 1 (a caller's check: 0 would divide by zero)
TAD_BUCKET_FN int64_t bucket_start(int64_t t, int64_t bucket_s, int64_t origin) {
  const uint64_t b = (uint64_t)bucket_s;
  const uint64_t d = (uint64_t)t - (uint64_t)origin;   // t - origin, two's complement, no signed overflow
  const bool below = (d >> 63) != 0;                   // t < origin
  const uint64_t m = below ? 0 - d : d;                // |t - origin|
  // (both under 2^32 — every real flowEndSeconds with a bucket of seconds to years: a 32-bit remainder, a fraction of the 64-bit one's cost)
  const uint64_t r = ((m | b) >> 32) == 0 ? (uint64_t)((uint32_t)m % (uint32_t)b) : m % b;
  const uint64_t back = below ? (r != 0 ? b - r : 0) : r;   // how far t lies above its bucket's start
  return (int64_t)((uint64_t)t - back);
}

// tad_state_rollup's piecewise bucket function: a time below the bound b moves to its bucket's start, a time at or after it stays.  b is
// itself a bucket start (the caller floors it), so no bucket straddles it: every image of a time below b is below b, and a key's strictly
// ascending times stay strictly ascending once equal images are folded into one point
TAD_BUCKET_FN int64_t rollup_start(int64_t t, int64_t b, int64_t bucket_s, int64_t origin) { return t < b ? bucket_start(t, bucket_s, origin) : t; }

}  // namespace tad

#endif  // THEIA_TAD_BUCKET_H
