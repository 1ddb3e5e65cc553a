// tad_drop_select.hip — the drop job's flow-row query (snowflake/cmd/dropDetection.go:36-190): flow rows -> the compact
// (endpoint tuple, direction, day, count, row) columns that tad_factorize / tad_keydict and Stage 0 take from there (tad.h, tad_drop_select).
//
// Dropped flows are a few per thousand of a flow table, so the select reads the two UInt8 action columns of every row and everything
// else only where a row survives.  Two launches with the project's scan (launch_scan) between them, no signalling between workgroups:
//   k_dsel_flags  a workgroup of 256 lanes owns a tile of kDselTileRows = 4096 rows, a lane kDselLaneRows = 16 consecutive ones.  The lane reads
//                 its 16 bytes of each action column with the widest loads the column's address allows (one 16-byte load when the column
//                 is 16-byte aligned: every lane's address then is; 8- or 4-byte loads or single bytes otherwise — the two action columns
//                 and the bitmask word need not share a misalignment, so the rows are never shifted to suit one of them), the ragged last
//                 lane of the table bytewise.  It forms the 16-bit "an action drops" mask with byte-parallel arithmetic, reads flow_start_s
//                 / flow_end_s / keep only for the set bits and only when that filter is on, writes its 16-bit word of the row bitmask
//                 (n / 8 bytes) and the workgroup writes the tile's count.
//   k_dsel_emit   a workgroup per tile again: 512 B of bitmask, a popcount per lane, a prefix over the workgroup (shuffles inside a
//                 wavefront, four partial sums through LDS), then every selected row is written at off[tile] + rank — input order — with
//                 the action byte, the start time and the three code columns of its side gathered for that row alone.  A tile without
//                 a selected row returns after two loads.
// Byte model (not a measurement): (2 + 1/8 + 1/8) N read and written for the action columns and the bitmask, the sectors the m selected
// rows touch (up to 6 sectors of 32 B a row when the rows lie far apart), 56 m written.
#include <hip/hip_runtime.h>

#include "tad_internal.h"

namespace tad {

namespace {
constexpr int kDselBlock = 256;
static_assert(kDselLaneRows == 16, "a lane's rows are one 16-byte load and one 16-bit word of the bitmask");
static_assert(kDselBlock * kDselLaneRows == kDselTileRows, "256 lanes own one tile");

// bit j = byte j of w is 2 or 3 (the two rule actions that drop)
__device__ __forceinline__ uint32_t drop_bits4(uint32_t w) {
  const uint32_t t = (w ^ 0x02020202u) & 0xFEFEFEFEu;                              // a zero byte where the action drops
  const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);        // 0x80 in every zero byte (no carry leaves a byte)
  return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;                                  // bits 0 / 8 / 16 / 24 -> bits 0..3
}

__device__ __forceinline__ uint32_t drop_bits16(uint4 v) {
  return drop_bits4(v.x) | (drop_bits4(v.y) << 4) | (drop_bits4(v.z) << 8) | (drop_bits4(v.w) << 12);
}

// the lane's 16 action bytes at p; mis = the column's address mod 16 (the same for every lane), avail = rows from p to the table's end
__device__ __forceinline__ uint4 load_actions(const uint8_t *__restrict__ p, unsigned mis, uint64_t avail) {
  if (avail >= (uint64_t)kDselLaneRows) {
    if (mis == 0) return *reinterpret_cast<const uint4 *>(p);
    if ((mis & 7u) == 0) {
      const uint2 a = reinterpret_cast<const uint2 *>(p)[0], b = reinterpret_cast<const uint2 *>(p)[1];
      return make_uint4(a.x, a.y, b.x, b.y);
    }
    if ((mis & 3u) == 0) {
      const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
      return make_uint4(q[0], q[1], q[2], q[3]);
    }
  }
  const int k = avail < (uint64_t)kDselLaneRows ? (int)avail : kDselLaneRows;
  uint32_t w[4] = {0u, 0u, 0u, 0u};          // rows beyond the table read as action 0: never selected
#pragma unroll
  for (int j = 0; j < kDselLaneRows; ++j)
    if (j < k) w[j >> 2] |= (uint32_t)p[j] << ((j & 3) * 8);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ long long time_at(const void *__restrict__ col, int t32, uint64_t i) {
  return t32 ? (long long)static_cast<const uint32_t *>(col)[i] : static_cast<const long long *>(col)[i];   // DateTime: zero-extended
}

__global__ __launch_bounds__(kDselBlock) void k_dsel_flags(DselIn A, uint16_t *__restrict__ bits, uint32_t *__restrict__ cnt) {
  const uint64_t base = (uint64_t)blockIdx.x * kDselTileRows + (uint64_t)threadIdx.x * kDselLaneRows;
  uint32_t m = 0;
  if (base < A.n) {
    const uint64_t avail = A.n - base;
    const uint4 ia = load_actions(A.ia + base, (unsigned)(reinterpret_cast<uintptr_t>(A.ia) & 15u), avail);
    const uint4 ea = load_actions(A.ea + base, (unsigned)(reinterpret_cast<uintptr_t>(A.ea) & 15u), avail);
    m = drop_bits16(ia) | drop_bits16(ea);
    if (A.start_time != 0 || A.end_time != 0 || A.keep != nullptr) {
      for (uint32_t left = m; left != 0; left &= left - 1) {
        const int j = __builtin_ctz(left);
        const uint64_t i = base + (uint64_t)j;
        bool ok = true;
        if (A.start_time != 0) ok = time_at(A.ts, A.t32, i) >= A.start_time;
        if (ok && A.end_time != 0) ok = time_at(A.te, A.t32, i) < A.end_time;
        if (ok && A.keep != nullptr) ok = A.keep[i] != 0;
        if (!ok) m &= ~(1u << j);
      }
    }
    bits[base / kDselLaneRows] = (uint16_t)m;
  }
  uint32_t c = (uint32_t)__popc(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  __shared__ uint32_t wave_sum[kDselBlock / 64];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

__global__ __launch_bounds__(kDselBlock) void k_dsel_emit(DselIn A, const uint16_t *__restrict__ bits, const unsigned long long *__restrict__ off, DselOut O) {
  const unsigned long long tile_off = off[blockIdx.x];
  if (off[blockIdx.x + 1] == tile_off) return;           // (the whole workgroup: nothing selected in this tile)
  const uint64_t base = (uint64_t)blockIdx.x * kDselTileRows + (uint64_t)threadIdx.x * kDselLaneRows;
  const uint32_t m = base < A.n ? (uint32_t)bits[base / kDselLaneRows] : 0u;
  const uint32_t c = (uint32_t)__popc(m);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  __shared__ uint32_t wave_sum[kDselBlock / 64];
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  uint32_t rank = inc - c;
  for (int w = 0; w < wave; ++w) rank += wave_sum[w];
  unsigned long long o = tile_off + rank;
  for (uint32_t left = m; left != 0; left &= left - 1, ++o) {
    const uint64_t i = base + (uint64_t)__builtin_ctz(left);
    const bool ingress = (A.ia[i] & 0xFEu) == 2u;        // ingress wins when both actions drop; ingress rows describe the destination
    const long long pod = ingress ? A.dst_pod[i] : A.src_pod[i];
    const bool is_pod = pod != (ingress ? A.dst_null : A.src_null);
    long long ns = 0, name = pod;
    if (is_pod) ns = ingress ? A.dst_ns[i] : A.src_ns[i];
    else name = ingress ? A.dst_ip[i] : A.src_ip[i];
    const long long t = time_at(A.ts, A.t32, i);
    long long day = t / 86400;
    if (t % 86400 < 0) --day;                            // floor, not truncation
    O.kind[o] = is_pod ? 1 : 0;
    O.ns[o] = ns;
    O.name[o] = name;
    O.dir[o] = ingress ? 0 : 1;
    O.day[o] = day * 86400;
    O.count[o] = 1ull;
    O.row[o] = i;
  }
}
}  // namespace

uint64_t dsel_tiles(uint64_t n) { return (n + kDselTileRows - 1) / kDselTileRows; }

// bits: (n + 15) / 16 words, cnt: dsel_tiles(n) counts; every pointer DEVICE
void launch_dsel_flags(hipStream_t s, const DselIn &A, uint16_t *bits, uint32_t *cnt) {
  if (A.n == 0) return;
  hipLaunchKernelGGL(k_dsel_flags, dim3((unsigned)dsel_tiles(A.n)), dim3(kDselBlock), 0, s, A, bits, cnt);
}

// off: the exclusive scan of cnt (dsel_tiles(n) + 1 entries); the columns of O hold off[tiles] rows
void launch_dsel_emit(hipStream_t s, const DselIn &A, const uint16_t *bits, const unsigned long long *off, const DselOut &O) {
  if (A.n == 0) return;
  hipLaunchKernelGGL(k_dsel_emit, dim3((unsigned)dsel_tiles(A.n)), dim3(kDselBlock), 0, s, A, bits, off, O);
}

// one kernel of this translation unit: tad_engine_create resolves it so that the unit's code object is loaded before the first job
const void *code_anchor_drop_select() { return reinterpret_cast<const void *>(&k_dsel_flags); }

}  // namespace tad
