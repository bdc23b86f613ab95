// host_film_checks.cpp — the corner cases of the one film-layout rule (csrc/film_checks.h: film_layout_invalid) as a stand-alone program, for
// a run under AddressSanitizer / UBSan (tests/test_film_checks.py): every combination of the corner values below, asked as the denoiser and the
// two films of an accumulation ask, and as the outlier clamp asks of its film (m2 optional, and no normals whatever the line's are).  Prints,
// per line, "xstride normals m2 samples" and the four answers (the field's index, or -1).
#include "../../phosphorus_mk2_amd/csrc/accumulate_check.h"
#include "../../phosphorus_mk2_amd/csrc/film_checks.h"
#include "../../phosphorus_mk2_amd/csrc/outlier_clamp_check.h"

#include <cstdio>

using namespace phx;

int main() {
  const uint32_t strides[] = {0u, 5u, 6u, 7u, 12u, 24u, 25u, 0xffffffffu};
  const uint32_t offsets[] = {0u, 2u, 3u, 5u, 6u, 9u, 11u, 12u, 21u, 23u, 24u, 0xfffffffeu, 0xffffffffu};
  const uint32_t max_xstride = (uint32_t)PHX_ACCUMULATE_MAX_XSTRIDE;
  for (uint32_t xs : strides)
    for (uint32_t n : offsets)
      for (uint32_t m2 : offsets)
        for (uint32_t s : offsets)
          std::printf("%u %u %u %u %d %d %d %d\n", xs, n, m2, s, film_layout_invalid(xs, n, m2, s, 6u, ~0u, false), film_layout_invalid(xs, n, m2, s, 7u, max_xstride, true),
                      film_layout_invalid(xs, n, m2, s, 6u, max_xstride, false), film_layout_invalid(xs, 0u, m2, s, 3u, (uint32_t)PHX_OUTLIER_MAX_XSTRIDE, false, false));
  return 0;
}
