// Tile kernels for 8x8 interrogation windows (see xcorr_tile.hpp): the candidate pass of precision "exact" and the peak-stage
// test hook.  The 8x8 passes themselves run one window per lane (xcorr_w8.hip).
#include "xcorr_tile.hpp"
namespace tpiv {
hipError_t launch_xcorr_cand_ws8(const PassParams& p, int n_cu, hipStream_t stream) {
    return launch_xcorr_tile_cand_ws<8>(p, n_cu, stream);
}
hipError_t launch_peak_debug_ws8(const PassParams& p, const float* maps, int n_maps, int planar, hipStream_t stream) {
    return launch_peak_debug<8>(p, maps, n_maps, planar, stream);
}
}  // namespace tpiv
