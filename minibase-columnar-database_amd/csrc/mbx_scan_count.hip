// mbx_scan_count.hip -- COUNT scans (mode_launch<kModeCount>), launch_scan's
// dispatch to the three MODEs, the grid choice, and k_finalize: the
// deterministic fixed-order reduction of per-block partials.
#include "mbx_scan_mode.hpp"

namespace mbx {

extern template void mode_launch<kModeBitmap>(const ScanLaunch&, dim3, hipStream_t);  // mbx_scan_bitmap.hip
extern template void mode_launch<kModeAgg>(const ScanLaunch&, dim3, hipStream_t);     // mbx_scan_agg.hip

// --------------------------------------------------------------- finalize

__global__ __launch_bounds__(kBlock) void k_finalize(const Partial* __restrict__ parts, int64_t n,
                                                     int32_t agg_kind, AggOut* out, int64_t* count_out,
                                                     int32_t* nan_flag) {
  // its own launch, its own registers: 16 partials in flight per thread
  // (4096 blocks' partials in one memory round trip instead of four)
  finalize_block<false, false, 16>(parts, n, agg_kind, out, count_out, nan_flag);
}

int64_t choose_tiles_per_block(int64_t nrows) {
  const int64_t ntiles = (nrows + kTileRows - 1) / kTileRows;
  // ~1024 blocks (4 per CU on 256 CUs, 16 waves/CU) for large inputs,
  // >= 4 tiles per block
  int64_t tpb = (ntiles + 1023) / 1024;
  return tpb < 4 ? 4 : tpb;
}

hipError_t launch_scan(const ScanLaunch& L, hipStream_t s) {
  const dim3 grid((unsigned)grid_blocks(L.nrows, L.tiles_per_block));
  switch (L.mode) {
    case kModeCount: mode_launch<kModeCount>(L, grid, s); break;
    case kModeBitmap: mode_launch<kModeBitmap>(L, grid, s); break;
    default: mode_launch<kModeAgg>(L, grid, s); break;
  }
  return hipGetLastError();
}

hipError_t launch_finalize(const Partial* partials, int64_t nblocks, int32_t agg_kind, AggOut* out,
                           int64_t* count_out, int32_t* nan_flag, hipStream_t s) {
  hipLaunchKernelGGL(k_finalize, dim3(1), dim3(kBlock), 0, s, partials, nblocks, agg_kind, out, count_out,
                     nan_flag);
  return hipGetLastError();
}

}  // namespace mbx
