// tad_drop_state.hip — the drop detector on a streaming state's series (include/tad.h: tad_drop_state / tad_drop_stream).
//
// A state with a series holds every key's aggregated values in time order (CSR: soff[K + 1], sval[]).  The batch kernel k_drop_detect
// (tad_drop.hip) compacts a K x T grid into a K x T workspace of doubles and gives one lane a whole key; here the series is already
// packed, the squared deviations are formed on the fly, and a long key has a wavefront of its own:
//   k_ds_route       (stream batches) the TOUCHED keys with >= coop_min points, listed; tad_drop_state takes k_win_route's list;
//   k_ds_stats_lane  one lane per key shorter than coop_min: mean = pairwise(x) / n, m2 = pairwise((mean - x)^2), std = sqrt(m2 / (n - 1));
//   k_ds_stats_wave  one wavefront per listed key, the same two sums with the additions of the same tree;
//   k_ds_verdict     one lane per judged point: x > mean + nsigma std || x < mean - nsigma std, and the rows it emits;
//   k_ds_emit        the rows at the scan of those counts, algo_calc = the key's mean, stddev = its std.
//
// The order of every sum is numpy's pairwise_sum_DOUBLE (pandas' Series.mean / Series.std), as pairwise_sum in tad_drop.hip restates
// it: below 8 elements left to right; up to 128 eight interleaved accumulators r[j] += a[i + j], ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
// then the tail; above 128 split at n2 = n/2 - (n/2) % 8 and add the halves.  The build's -ffp-contract=off keeps d * d and the add
// apart, so summing (mean - x)^2 as it is formed gives the bits of k_drop_detect's store-then-sum.
//
// The wavefront shape.  The tree depends on n alone; above 128 elements its leaves are contiguous runs of 64 to 128 elements that
// start at a multiple of 8 from the segment's start.  Lane 0 walks the tree (a stack of pending right halves, at most 32 deep below
// 2^32 elements) and writes up to 64 leaf descriptors a round into LDS: start, length, and the number of internal nodes that are
// complete once the leaf is.  Eight lanes then take one leaf — lane j holds accumulator j, so every step of a leaf reads one 64-byte
// line — and combine with three xor-shuffles (the operands of every add are those of the fixed tree; an add is commutative bit for
// bit); the leaf's first lane adds the tail and parks the sum in LDS.  Lane 0 folds the round in leaf order on a value stack: push,
// then `merges` times pop the right half, pop the left, push left + right.  Lanes only change who does an addition, never which.
#include <stdint.h>

#include "tad_internal.h"

namespace tad {

static constexpr int kDsBlock = 256;
static constexpr int kDsLeaves = 64;   // leaf descriptors per round of the wavefront shape (8 leaves a step, 8 steps)
static constexpr int kDsDepth = 40;    // pending halves / values on the fold's stack: at most 32 below 2^32 elements

template <bool SQ> __device__ __forceinline__ double ds_elem(unsigned long long raw, double mean) {
  const double x = (double)raw;
  if (!SQ) return x;
  const double d = mean - x;
  return d * d;
}

// numpy pairwise_sum_DOUBLE over the elements of a[0 .. n) (SQ: their squared deviations from mean)
template <bool SQ> __device__ double ds_pairwise(const unsigned long long *__restrict__ a, unsigned long long n, double mean) {
  if (n < 8) {
    double r = 0.0;
    for (unsigned long long i = 0; i < n; ++i) r += ds_elem<SQ>(a[i], mean);
    return r;
  }
  if (n <= 128) {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = ds_elem<SQ>(a[j], mean);
    unsigned long long i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] += ds_elem<SQ>(a[i + j], mean);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += ds_elem<SQ>(a[i], mean);
    return res;
  }
  unsigned long long n2 = n / 2;
  n2 -= n2 % 8;
  return ds_pairwise<SQ>(a, n2, mean) + ds_pairwise<SQ>(a + n2, n - n2, mean);
}

__device__ __forceinline__ void ds_store(const DropStateKeys &o, uint64_t k, unsigned long long n, double sum, double m2, uint32_t min_samples) {
  const bool ok = n >= min_samples && n >= 2;
  o.n[k] = (uint32_t)n;
  o.mean[k] = n ? sum / (double)n : 0.0;
  o.m2[k] = m2;
  o.std[k] = n >= 2 ? sqrt(m2 / (double)(n - 1)) : 0.0;
  o.ok[k] = ok ? 1 : 0;
}

// the touched keys (poff[k + 1] > poff[k]) with >= coop_min points, ballot-compacted: one atomic per wavefront
__global__ __launch_bounds__(kDsBlock) void k_ds_route(uint64_t K, const unsigned long long *__restrict__ soff, const unsigned long long *__restrict__ poff,
                                                      unsigned long long coop_min, uint32_t *__restrict__ list, unsigned int *__restrict__ count) {
  const uint64_t k = (uint64_t)blockIdx.x * kDsBlock + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  bool is_long = false;
  if (k < K) is_long = poff[k + 1] > poff[k] && soff[k + 1] - soff[k] >= coop_min;
  const unsigned long long m = __ballot(is_long);
  if (m) {
    const int first = __ffsll((long long)m) - 1;
    unsigned int base = 0;
    if ((int)lane == first) base = atomicAdd(count, (unsigned int)__popcll(m));
    base = (unsigned int)__shfl((int)base, first);
    if (is_long) list[base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)k;
  }
}

// One lane per key.  poff == NULL: every key is judged (an empty one gets n = 0); else only the touched keys are read or written.
// A key with points and no result counts in keys_no_result — here for the keys of the wavefront shape too (their lengths are known).
__global__ __launch_bounds__(kDsBlock) void k_ds_stats_lane(uint64_t K, const unsigned long long *__restrict__ soff, const unsigned long long *__restrict__ sval,
                                                           const unsigned long long *__restrict__ poff, unsigned long long coop_min, uint32_t min_samples,
                                                           DropStateKeys o, DevCounters *ctr) {
  const uint64_t k = (uint64_t)blockIdx.x * kDsBlock + threadIdx.x;
  unsigned skip = 0;
  if (k < K && (poff == nullptr || poff[k + 1] > poff[k])) {
    const unsigned long long p0 = soff[k], n = soff[k + 1] - p0;
    skip = (n > 0 && !(n >= min_samples && n >= 2)) ? 1u : 0u;
    if (n < coop_min) {   // (the others are k_ds_stats_wave's)
      double sum = 0.0, m2 = 0.0;
      if (n) {
        sum = ds_pairwise<false>(sval + p0, n, 0.0);
        const double mean = sum / (double)n;
        m2 = ds_pairwise<true>(sval + p0, n, mean);
      }
      ds_store(o, k, n, sum, m2, min_samples);
    }
  } else if (k < K) {
    o.ok[k] = 0;   // untouched: no verdict reads it, but the flag is defined
  }
  for (int d = 32; d >= 1; d >>= 1) skip += __shfl_down(skip, d);
  if ((threadIdx.x & 63) == 0 && skip) atomicAdd(&ctr->keys_no_result, (unsigned long long)skip);
}

// One leaf of 8 .. 128 elements (or fewer than 8: left to right) by the eight lanes j = 0 .. 7 of a group; the sum is valid in lane j == 0.
template <bool SQ> __device__ __forceinline__ double ds_leaf(const unsigned long long *__restrict__ a, uint32_t n, double mean, unsigned j) {
  if (n < 8) {
    double r = 0.0;
    for (uint32_t i = 0; i < n; ++i) r += ds_elem<SQ>(a[i], mean);
    return r;
  }
  const uint32_t full = n - (n % 8);
  double r = ds_elem<SQ>(a[j], mean);
  for (uint32_t i = 8; i < full; i += 8) r += ds_elem<SQ>(a[i + j], mean);
  r = r + __shfl_xor(r, 1);   // lane 0: r0 + r1, lane 2: r2 + r3, ...
  r = r + __shfl_xor(r, 2);   // lane 0: (r0 + r1) + (r2 + r3), lane 4: (r4 + r5) + (r6 + r7)
  r = r + __shfl_xor(r, 4);   // lane 0: the fixed tree
  for (uint32_t i = full; i < n; ++i) r += ds_elem<SQ>(a[i], mean);
  return r;
}

struct DsWave {   // LDS of one wavefront
  double leaf_sum[kDsLeaves];
  double val[kDsDepth];                  // the fold's value stack
  unsigned long long leaf_start[kDsLeaves];
  unsigned long long pend_start[kDsDepth];
  unsigned long long pend_n[kDsDepth];
  uint32_t pend_m[kDsDepth];
  uint32_t leaf_n[kDsLeaves];
  uint32_t leaf_m[kDsLeaves];
  uint32_t leaves;                       // descriptors of the running round
  double result;
};

// the pairwise sum over a[0 .. n) by one wavefront (block of 64); the result in every lane
template <bool SQ> __device__ double ds_wave_sum(DsWave &w, const unsigned long long *__restrict__ a, unsigned long long n, double mean) {
  const unsigned lane = threadIdx.x & 63u;
  int np = 0, nv = 0;   // lane 0's: pending halves, values
  if (lane == 0) { w.pend_start[0] = 0; w.pend_n[0] = n; w.pend_m[0] = 0; np = 1; }
  for (;;) {
    if (lane == 0) {   // the next round's leaves, in the tree's order
      uint32_t c = 0;
      while (c < (uint32_t)kDsLeaves && np > 0) {
        --np;
        unsigned long long s0 = w.pend_start[np], len = w.pend_n[np];
        uint32_t m = w.pend_m[np];
        while (len > 128) {   // the right half waits; it completes this node (one merge) and whatever this node completes
          unsigned long long n2 = len / 2;
          n2 -= n2 % 8;
          w.pend_start[np] = s0 + n2; w.pend_n[np] = len - n2; w.pend_m[np] = m + 1;
          ++np;
          len = n2;
          m = 0;
        }
        w.leaf_start[c] = s0; w.leaf_n[c] = (uint32_t)len; w.leaf_m[c] = m;
        ++c;
      }
      w.leaves = c;
    }
    __syncthreads();
    const uint32_t leaves = w.leaves;
    if (leaves == 0) break;   // (wavefront-uniform)
    for (uint32_t base = 0; base < leaves; base += 8) {
      const uint32_t l = base + (lane >> 3);
      // (a leaf's shuffles stay inside its own eight lanes, which all take the same path; a group without a leaf sums an empty one)
      const bool has = l < leaves;
      const double r = ds_leaf<SQ>(a + (has ? w.leaf_start[l] : 0ull), has ? w.leaf_n[l] : 0u, mean, lane & 7u);
      if (has && (lane & 7u) == 0) w.leaf_sum[l] = r;
    }
    __syncthreads();
    if (lane == 0) {
      for (uint32_t l = 0; l < leaves; ++l) {
        w.val[nv++] = w.leaf_sum[l];
        for (uint32_t m = w.leaf_m[l]; m; --m) {
          const double right = w.val[--nv], left = w.val[--nv];
          w.val[nv++] = left + right;
        }
      }
    }
  }
  if (lane == 0) w.result = w.val[0];
  __syncthreads();
  const double res = w.result;
  __syncthreads();   // (the next sum writes the same LDS)
  return res;
}

// One wavefront (workgroup of 64) per listed key, the wavefronts striding over the list.
__global__ __launch_bounds__(64) void k_ds_stats_wave(const uint32_t *__restrict__ list, const unsigned int *__restrict__ count,
                                                      const unsigned long long *__restrict__ soff, const unsigned long long *__restrict__ sval,
                                                      uint32_t min_samples, DropStateKeys o) {
  __shared__ DsWave w;
  const unsigned int cnt = *count;
  for (unsigned int i = blockIdx.x; i < cnt; i += gridDim.x) {   // (block-uniform)
    const uint64_t k = list[i];
    const unsigned long long p0 = soff[k], n = soff[k + 1] - p0;
    const double sum = ds_wave_sum<false>(w, sval + p0, n, 0.0);
    const double mean = sum / (double)n;
    const double m2 = ds_wave_sum<true>(w, sval + p0, n, mean);
    if ((threadIdx.x & 63u) == 0) ds_store(o, k, n, sum, m2, min_samples);
  }
}

// One lane per judged point i (key nk[i], value nv[i]): flag[i] = the verdict, cnt[i] = the rows it emits (0 for a key without a
// result, else 1 with all_points, else the verdict); lanes in [*P_dev, P_cap) write cnt = 0 so that the scan may run over P_cap.
// (upper / lower: k_drop_detect forms them once per key; the same two operations per point give the same bits.)
__global__ __launch_bounds__(kDsBlock) void k_ds_verdict(const unsigned long long *__restrict__ nk, const unsigned long long *__restrict__ nv,
                                                        const unsigned long long *__restrict__ P_dev, uint64_t P_cap, DropStateKeys o, double n_sigma,
                                                        bool all_points, uint8_t *__restrict__ flag, uint32_t *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * kDsBlock + threadIdx.x;
  if (i >= P_cap) return;
  if (i >= *P_dev) { cnt[i] = 0; return; }
  const uint64_t k = nk[i];
  if (!o.ok[k]) { flag[i] = 0; cnt[i] = 0; return; }
  const double mean = o.mean[k], std = o.std[k];
  const double upper = mean + n_sigma * std, lower = mean - n_sigma * std;
  const double x = (double)nv[i];
  const bool z = x > upper || x < lower;
  flag[i] = z ? 1 : 0;
  cnt[i] = (all_points || z) ? 1u : 0u;
}

__global__ __launch_bounds__(kDsBlock) void k_ds_emit(const unsigned long long *__restrict__ nk, const long long *__restrict__ nt,
                                                     const unsigned long long *__restrict__ nv, const unsigned long long *__restrict__ P_dev,
                                                     const uint8_t *__restrict__ flag, const uint32_t *__restrict__ cnt,
                                                     const unsigned long long *__restrict__ row, const double *__restrict__ mean,
                                                     const double *__restrict__ std, bool all_points, OutRows out) {
  const uint64_t i = (uint64_t)blockIdx.x * kDsBlock + threadIdx.x;
  if (i >= *P_dev || cnt[i] == 0) return;
  const uint64_t k = nk[i];
  const unsigned long long at = row[i];
  out.key_id[at] = k;
  out.flow_end_s[at] = nt[i];
  out.throughput[at] = (double)nv[i];
  out.algo_calc[at] = mean[k];
  out.stddev[at] = std[k];
  if (all_points) out.anomaly[at] = flag[i];
}

// ---- launchers ----
static inline unsigned ds_blocks(uint64_t lanes) { return (unsigned)((lanes + kDsBlock - 1) / kDsBlock); }

void launch_ds_route(hipStream_t s, uint64_t K, const unsigned long long *soff, const unsigned long long *poff, unsigned long long coop_min, uint32_t *list,
                     unsigned int *count) {
  hipMemsetAsync(count, 0, sizeof(unsigned int), s);
  if (K == 0) return;
  hipLaunchKernelGGL(k_ds_route, dim3(ds_blocks(K)), dim3(kDsBlock), 0, s, K, soff, poff, coop_min, list, count);
}

void launch_ds_stats(hipStream_t s, uint64_t K, const unsigned long long *soff, const unsigned long long *sval, const unsigned long long *poff,
                     unsigned long long coop_min, const uint32_t *list, const unsigned int *count, int min_samples, DropStateKeys d, DevCounters *ctr) {
  if (K == 0) return;
  const uint32_t ms = (uint32_t)(min_samples < 0 ? 0 : min_samples);
  hipLaunchKernelGGL(k_ds_stats_lane, dim3(ds_blocks(K)), dim3(kDsBlock), 0, s, K, soff, sval, poff, coop_min, ms, d, ctr);
  // the listed keys: the list's length stays on the device, the wavefronts stride over it
  const unsigned waves = (unsigned)(K < 4096 ? K : 4096);
  hipLaunchKernelGGL(k_ds_stats_wave, dim3(waves), dim3(64), 0, s, list, count, soff, sval, ms, d);
}

void launch_ds_verdict(hipStream_t s, const unsigned long long *nk, const unsigned long long *nv, const unsigned long long *P_dev, uint64_t P_cap,
                       DropStateKeys d, double n_sigma, bool all_points, uint8_t *flag, uint32_t *cnt) {
  if (P_cap == 0) return;
  hipLaunchKernelGGL(k_ds_verdict, dim3(ds_blocks(P_cap)), dim3(kDsBlock), 0, s, nk, nv, P_dev, P_cap, d, n_sigma, all_points, flag, cnt);
}

void launch_ds_emit(hipStream_t s, const unsigned long long *nk, const long long *nt, const unsigned long long *nv, const unsigned long long *P_dev,
                    uint64_t P_cap, const uint8_t *flag, const uint32_t *cnt, const unsigned long long *row, DropStateKeys d, bool all_points, OutRows out) {
  if (P_cap == 0) return;
  hipLaunchKernelGGL(k_ds_emit, dim3(ds_blocks(P_cap)), dim3(kDsBlock), 0, s, nk, nt, nv, P_dev, flag, cnt, row, d.mean, d.std, all_points, out);
}

// one kernel of this translation unit: tad_engine_create resolves it so that the unit's code object is loaded before the first job
const void *code_anchor_drop_state() { return reinterpret_cast<const void *>(&k_ds_stats_wave); }

}  // namespace tad
