// bitset_tiles.hpp — the dense tiles' geometry, as far as more than one file
// needs it: the kernels (bitset.hip), the build that pads the rows for them
// (bitset_build.hip), and the plan and cost model that enumerate the tiles
// (matrix_step.hip).
#pragma once

#include <cstdint>

namespace gdist {

constexpr int BT = 128;                 // tile edge (sets)
// A block's last row tile holding RR <= kPartialMaxRR sixteen-row groups gets
// its own launches with RR accumulator rows (RR = 7 saves less than the two
// launches cost: C2, 104 rows, 4.51 vs 4.27 ms)
constexpr int kPartialMaxRR = 6;
constexpr int KC = 16;                  // bitsets are padded to whole multiples of KC words
constexpr int MT = 256;                       // MFMA tile edge (sets)
constexpr int64_t kMfmaMinWords = 64;         // dense words from which the MFMA tiles run (option bitset_mfma)

}  // namespace gdist
