// K2 of a five-tick pass (chip_api.hip coalesce_submit).  A translation unit of its own: topk_merge<3> in kernels.hip keeps the registers
// profiles/project.md records for it (a second caller of the merge's helpers next to it changes its allocation).
#include "chip_internal.h"
#include "topk_merge.h"

namespace chip {

// K2 of a five-tick pass, one workgroup per tick.  The pass fills every CU's register file, so what follows it on the ctx stream runs in
// the gap between two passes, and a gap takes about five small launches: tick_rescore and one topk_merge per tick are six, the last tick of
// every pass then finishes a whole pass late, the caller's window of ticks in flight runs short and the next pass leaves with four
// (profiles/tick_coalesce_ab.md, last section).  Same function, same arguments as topk_merge<3> on the tick's block of lists: same record.
__global__ __launch_bounds__(512) void pass_merge(PassMergeArgs a)
{
    __shared__ __attribute__((aligned(16))) char smem[kMergeSmem];
    const int t = blockIdx.x;
    merge_sorted_lists<3>(a.in + (size_t)t * 3 * a.K, 1, 3, 0, a.K, nullptr, a.result[t], a.l[t], a.locality[t], a.thresh[t], smem);
}

int launch_pass_merge(Ctx *c, hipStream_t s, const PassMergeArgs &a, int n_ticks)
{
    if (n_ticks < 1 || n_ticks > kPassMaxTicks || a.K > CHIP_MAX_TOPK) return CHIP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pass_merge, dim3(n_ticks), dim3(512), 0, s, a);
    CHIP_HIP(c, hipGetLastError());
    return CHIP_OK;
}

}  // namespace chip
