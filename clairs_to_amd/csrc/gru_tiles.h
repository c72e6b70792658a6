// Tile heights of the BiGRU launches.  Plain C++ with no HIP in it, so that a host compiler sees the rule (tests/host/gru_tiles_check.cpp).
#pragma once
#include <stdint.h>
#include <type_traits>

namespace cto {

// Tile height per launch.  A workgroup owns (MS*16 sites, one direction) for all 33 steps, so a launch is a whole number of
// "rounds" of one workgroup per CU.  32-site tiles use every weight fragment for twice as many MFMAs and are used for every
// full round (a multiple of 16 * CUs sites); what is left over runs as 32-site tiles if it still fills most of a round (more
// than 3/4 of it), else as 16-site tiles, whose workgroups finish in ~0.83x the time (the weight stream per workgroup is the
// same, the MFMA work is half) and which spread a small batch over twice as many CUs: measured 1.45 -> 1.20 ms for B <= 2048,
// -3 % for B = 10 000.
// Calls launch(begin, end, std::integral_constant<int, MS>) for each non-empty site range of a batch of B, in order, and stops
// at the first status that is not 0.
template <class F>
int for_each_gru_tile_range(int64_t B, int cus, F&& launch) {
    const int64_t round32 = int64_t(16) * cus;                   // sites of one round of 32-site tiles (2 directions)
    const int64_t full = (B / round32) * round32;
    const int64_t rest = B - full;
    if (full > 0)
        if (const int rc = launch(int64_t(0), full, std::integral_constant<int, 2>{})) return rc;
    if (rest == 0) return 0;
    if (rest * 4 > round32 * 3) return launch(full, B, std::integral_constant<int, 2>{});
    return launch(full, B, std::integral_constant<int, 1>{});
}

}  // namespace cto
