// mbx_scan_agg.hip -- COUNT+SUM+MIN+MAX scans (mode_launch<kModeAgg>, called by launch_scan).
#include "mbx_scan_mode.hpp"

namespace mbx {

template void mode_launch<kModeAgg>(const ScanLaunch&, dim3, hipStream_t);

}  // namespace mbx
