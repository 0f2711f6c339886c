// The walk of one 32-position segment of K1's greedy path (match_block's W1, Jacobi rounds, W2
// and W3 in dmx_kernels.hip), as host and device code, so that it can be checked against a
// position-by-position walk in a stand-alone host program (tests/c/walk_model.cpp).
#ifndef DMX_WALK_H
#define DMX_WALK_H
#include "dmx_extbits.h"

#define DMX_WALK_TRIPS 33   // fixed loop bound: a trip that does not end the walk takes a match (>= 3 positions)

// Walk segment [lo, lo + 32) of a block of bn positions from entry e >= lo.  lw holds the
// segment's literal bits (bits of positions >= bn may be set: the lazy rule sets them), len_at(p)
// reads the length - 3 of the match at p.  One trip takes the literal run at p (it may be empty;
// clipped at min(lo + 32, bn)), adds its bits, stops at the segment end, else adds the match's
// bit, reads its length once and advances: one read, waited for once, per trip.
// Returns the exit (the first position >= min(lo + 32, bn) the path reaches) and the path word.
// MERGE: m is the segment's current path word and x its exit.  When the walk meets a position
// of m -- inside a literal run or at a match -- the rest coincides with m (the next-function is
// deterministic): the word is the new head plus m's tail from there, the exit is x, merged is set.
// trips, if given, receives the number of loop trips.
template <bool MERGE, class LenAt>
DMX_HD uint32_t dmx_walk_segment(uint32_t lo, uint32_t e, uint32_t bn, uint32_t lw, uint32_t m, uint32_t x,
                                 LenAt len_at, uint32_t& word, bool& merged, uint32_t* trips = nullptr) {
    const uint32_t end = dmx_minu(lo + 32u, bn);
    uint32_t nm = 0, p = e, t = 0;
    merged = false;
    if (p < end) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (; t < DMX_WALK_TRIPS;) {
            t++;
            const uint32_t sh = p - lo;
            const uint32_t run = dmx_minu(dmx_ffbl(~(lw >> sh)), end - p);
            const uint32_t rm = (run >= 32u ? ~0u : ((1u << run) - 1u)) << sh;
            if (MERGE && (m & rm)) {
                const uint32_t below = (1u << dmx_ffbl(m & rm)) - 1u;   // below the first shared position
                nm |= (rm & below) | (m & ~below);
                merged = true;
                p = x;
                break;
            }
            nm |= rm;
            p += run;
            if (p >= end) break;
            const uint32_t bit = 1u << (p - lo);
            if (MERGE && (m & bit)) {
                nm |= m & ~(bit - 1u);
                merged = true;
                p = x;
                break;
            }
            nm |= bit;
            p += len_at(p) + 3u;
            if (p >= end) break;
        }
    }
    if (trips) *trips = t;
    word = nm;
    return p;
}
#endif
