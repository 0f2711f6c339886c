/*
 * sort_slices.cpp -- prints the counting sort's slice map (csrc/dmx_sort_slices.h) as the host
 * compiles it, one line per index i = 0..15:
 *   i  wave_of_slice(i)  slice_of_wave(i)  slice_group(i)  slice_round(i)
 * tests/test_sort_slice_map.py reads the table and checks the map's properties.
 */
#include <cstdio>
#include "dmx_sort_slices.h"

int main() {
    for (uint32_t i = 0; i < DMX_SORT_SLICES; i++)
        printf("%u %u %u %u %u\n", i, dmx_sort_wave_of_slice(i), dmx_sort_slice_of_wave(i), dmx_sort_slice_group(i),
               dmx_sort_slice_round(i));
    return 0;
}
