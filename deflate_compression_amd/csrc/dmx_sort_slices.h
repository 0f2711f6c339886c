// Which wave of K1's workgroup ranks which 2048 positions in the counting sort
// (count_sort_positions in dmx_kernels.hip), as host and device code, so that the map can be
// checked on the CPU (tests/test_sort_slice_map.py).
//
// Slice s = 4g + r is positions [2048 s, 2048 s + 2048): it belongs to group g = s >> 2 (a
// counter array and a 16-bit field of it) and is ranked in round r = s & 3, so a group's
// rounds run in position order.  Wave 4g + ((g + r) & 3) runs it: the four waves of a round
// then have four different w & 3, which is the SIMD they sit on when the hardware places wave
// w of a workgroup on SIMD w mod 4 (with wave = slice they would share one).
#ifndef DMX_SORT_SLICES_H
#define DMX_SORT_SLICES_H
#include <stdint.h>
#include "dmx_extbits.h"   // DMX_HD

#define DMX_SORT_SLICES 16u

DMX_HD uint32_t dmx_sort_slice_group(uint32_t s) { return s >> 2; }
DMX_HD uint32_t dmx_sort_slice_round(uint32_t s) { return s & 3u; }
DMX_HD uint32_t dmx_sort_wave_of_slice(uint32_t s) {
    const uint32_t g = s >> 2, r = s & 3u;
    return (g << 2) | ((g + r) & 3u);
}
DMX_HD uint32_t dmx_sort_slice_of_wave(uint32_t w) {
    const uint32_t g = w >> 2;
    return (g << 2) | ((w - g) & 3u);
}
#endif
