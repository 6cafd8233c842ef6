// mbx_scan_bitmap.hip -- BitSet scans (mode_launch<kModeBitmap>, called by launch_scan).
#include "mbx_scan_mode.hpp"

namespace mbx {

template void mode_launch<kModeBitmap>(const ScanLaunch&, dim3, hipStream_t);

}  // namespace mbx
