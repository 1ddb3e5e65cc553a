// tad_dev_err.h — the error bits a kernel raises in DevCounters::err: shared by the device code (tad_internal.h) and the host's retry
// rules (tad_stage0_retry.h).  Plain C++: no HIP.
#ifndef THEIA_TAD_DEV_ERR_H
#define THEIA_TAD_DEV_ERR_H

#include <stdint.h>

namespace tad {

enum : uint32_t { DEV_ERR_KEY_RANGE = 1u, DEV_ERR_OFF_LATTICE = 2u, DEV_ERR_OVERFLOW_LIST = 4u, DEV_ERR_LATE_ROW = 8u,
                  DEV_ERR_REGION_FULL = 16u,   // Stage 0 v2 with a SAMPLED histogram: a (workgroup, partition) region was sized too small
                  // (32u was DEV_ERR_SPEC of the one-synchronisation job, ABI 8-11: removed in round 6, see docs/HISTORY.md)
                  DEV_ERR_SPARSE_ROUND = 64u };  // sparse Stage 0 through the partition pass: one key bin holds more records than a workgroup sorts in LDS (the LSD sort takes over)

}  // namespace tad

#endif  // THEIA_TAD_DEV_ERR_H
