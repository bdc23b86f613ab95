// shade_launch.h — what the two shade families' launch code shares (shade_lambert.hip, shade_general.hip); private to them.
#pragma once
#include "shade_common.h"

namespace phx {

// launch_shade (shade_general.hip) hands a sc.diffuse_only scene to the Lambert family (shade_lambert.hip)
uint64_t launch_shade_lambert(hipStream_t stream, const DevScene& sc, const PassBuffers& pb, int q, int sq, uint32_t capacity, uint32_t sample0, int camera_rays, bool lens);

// One shade launch and the bit of phx_stats::shade_kernels that names it: both come from the same template arguments, so the bit reports
// the kernel that ran and not a second reading of the scene's flags.
template <bool FIRST, bool LENS> constexpr uint32_t shade_pass() {
  static_assert(FIRST || !LENS, "the lens bends camera rays only");
  return LENS ? PHX_SHADE_PASS_LENS : FIRST ? PHX_SHADE_PASS_CAMERA : PHX_SHADE_PASS_LATER;
}
// (camera_rays, lens) -> the three legal (FIRST, LENS) pairs: the lens bends camera rays only
template <typename F> static auto with_pass(bool camera_rays, bool lens, F&& f) {
  if (camera_rays) return with_flag(lens, [&](auto LENS) { return f(std::true_type{}, LENS); });
  return f(std::false_type{}, std::false_type{});
}

}  // namespace phx
