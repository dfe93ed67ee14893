// fv3net_amd — which kord <= 7 remap kernel a launch runs (mappm.hip): the thresholds and
// one pure function of the call's size, the device's CU count and the A/B knobs.  No HIP
// types, so the CPU suite asks the same function (tests/native/mappm_host.cpp,
// tests/test_mappm_oracle.py).
#pragma once

#include <cstdint>
#include <cstdlib>

namespace fv3 {

// The level-parallel kernel (one block per column) against one lane per column, one field
// (tools/ab.py, kord 1 79->79): C48 (13,824 columns) 142 -> 38 us, C96 (55,296) 168 ->
// 118 us; at C384 the serial kernel (0.70 ms) wins.
constexpr int64_t kLevelsMaxCols = 65536;

// Pairs of fields: the pair kernel on two or three lanes per column beats the
// level-parallel kernel (one field per launch) from ~10,000 columns
// (tools/ab.py, profiles/r05zr_mappm_small_lanes.log and
// r05zs_mappm_small_lanes.log, two fields, levels / three lanes: 6,912 columns 47 / 59 us,
// 10,368 63 / 59 us, C48 13,824 77 / 60 us, C96 55,296 252 / 86 us)
constexpr int64_t kLevelsMaxColsPairs = 10240;

// Where two lanes per column pay for a pair (tools/ab.py, one box, interleaved; one lane
// per column vs two).  With whole-column sortedness scans up front
// (profiles/r05r_mappm_split.log): 65,536 columns 142.7 vs 115.4 us, 110,592 (one rank's
// C384 band at world 8) 165.7 vs 161.5 us, 147,456 213 vs 228 us, C384 0.78 vs 1.06 ms.
// With the start layer searched and the checks on the streamed edges
// (profiles/r05zi_mappm_split.log): 65,536 columns 142.7 vs 99 us, 110,592 165.8 vs
// 142 us, 147,456 215 vs 215 us, 221,184 262 vs 280 us, C384 0.78 vs 0.93 ms.
constexpr int64_t kSplitMaxCols = 147456;
// Three lanes (profiles/r05zq_mappm_split3.log, one / two / three lanes): 65,536 columns
// 142.7 / 99 / 86.5 us, 110,592 166 / 141 / 150.5 us, 147,456 214 / 213 / 194 us.  The
// pair's split kernels hold 4 waves per SIMD (124-126 VGPRs); three lanes pay while all
// their waves are resident at once (3 ncol / 64 <= 4 waves x 4 SIMDs x CUs), which 110,592
// columns exceed.
constexpr int kSplitWavesPerSimd = 4;

// One field on the split kernels (profiles/r05zw_mappm_single_lanes.log, levels / one lane
// / two / three lanes, us): 13,824 columns 38.6 / 105 / 70 / 49.6, 27,648 67.8 / 108 / 76
// / 56.6, C96 55,296 126 / 110 / 81 / 70, 82,944 184 / 127 / 113 / 98, 110,592 242 / 128 /
// 115 / 119, 147,456 320 / 152 / 139 / 149, 221,184 589 / 190 / 204 / 210.  The one-field
// split kernels hold 5 waves per SIMD (91 VGPRs): three lanes while all their waves are
// resident (3 ncol / 64 <= 5 x 4 SIMDs x CUs), then two while theirs are, from 20,480
// columns (the level-parallel kernel below).
constexpr int64_t kSplit1MinCols = 20480;
constexpr int kSplit1WavesPerSimd = 5;

// the four kord <= 7 kernels: a lane per level, or one, two or three lanes per column
enum PpmKernel { kPpmLevels = 0, kPpmLanes1 = 1, kPpmLanes2 = 2, kPpmLanes3 = 3 };

// The A/B knobs' values (NULL: unset), for tests and tools:
//   FV3_MAPPM_PATH=serial|levels   never / always (km, kn <= 1000) the level-parallel kernel
//   FV3_MAPPM_SPLIT=0|1|3          a pair on one / two / three lanes
//   FV3_MAPPM_SPLIT1=0|2|3         one field on none / two / three lanes of the split kernel
struct PpmKnobs {
    const char* path;
    const char* split;
    const char* split1;
};

// the level-parallel kernel while one lane per column leaves the chip mostly idle; its
// LDS layout bounds km and kn
inline bool ppm_levels_serves(const PpmKnobs& knobs, int64_t ncol, int km, int kn, int64_t max_cols)
{
    if (knobs.path && knobs.path[0] == 's') return false;
    if (km > 1000 || kn > 1000) return false;
    if (knobs.path && knobs.path[0] == 'l') return true;
    return ncol < max_cols;
}

// The kernel of a launch of `fields` (1 or 2) fields over ncol columns, km -> kn levels,
// on a device of n_cu CUs.  For two fields kPpmLevels means that the fields go one per
// launch, each through this function with fields = 1.
inline PpmKernel ppm_kernel_choice(int fields, int64_t ncol, int km, int kn, int n_cu, const PpmKnobs& knobs)
{
    if (fields == 2) {
        if (ppm_levels_serves(knobs, ncol, km, kn, kLevelsMaxColsPairs)) return kPpmLevels;
        int lanes = ncol < kSplitMaxCols ? 2 : 1;
        if (lanes == 2 && 3 * ncol <= (int64_t)64 * kSplitWavesPerSimd * 4 * n_cu) lanes = 3;
        if (knobs.split && knobs.split[0] == '0') lanes = 1;
        if (knobs.split && knobs.split[0] == '1') lanes = 2;
        if (knobs.split && knobs.split[0] == '3') lanes = 3;
        if (lanes == 3 && kn < 3) lanes = 2;
        if (lanes == 2 && kn < 2) lanes = 1;
        return (PpmKernel)lanes;
    }
    if (kn >= 2) {  // the split kernels first; a forced FV3_MAPPM_PATH keeps its kernel
        int lanes = 0;
        if (knobs.split1) {
            lanes = atoi(knobs.split1);
        } else if (!knobs.path && ncol >= kSplit1MinCols) {
            const int64_t resident = (int64_t)64 * kSplit1WavesPerSimd * 4 * n_cu;
            lanes = 3 * ncol <= resident ? 3 : (2 * ncol <= resident ? 2 : 0);
        }
        if (lanes == 3 && kn < 3) lanes = 2;
        if (lanes == 2 || lanes == 3) return (PpmKernel)lanes;
    }
    return ppm_levels_serves(knobs, ncol, km, kn, kLevelsMaxCols) ? kPpmLevels : kPpmLanes1;
}

}  // namespace fv3
