// exact_sum.h -- the exact sum of double square roots that expos.hip's whole-frame statistics use, host side.
// sqrt of an integer in 1 .. 3 * 255^2 is a double in [1, 442): in units of 2^-52 it is an integer below 2^61.  The kernel splits that
// integer into a 32-bit low limb and a 29-bit high limb and adds each limb into a 64-bit counter of its own (room for 2^32 pixels);
// here the two counters become T = hi * 2^32 + lo in 128 bits and the sum is (double)T * 2^-52: ONE correct rounding
// (round to nearest, ties to even), whatever the order the pixels were added in.
#pragma once
#include <math.h>
#include <stdint.h>

#define MIS_EXACT_SCALE 4503599627370496.0   /* 2^52 */

// Round a 128-bit unsigned integer to the nearest double, ties to even, written out so that the result does not depend on the
// runtime's conversion routine.
static inline double mis_u128_to_double(unsigned __int128 t) {
    if (t < ((unsigned __int128)1 << 53)) return (double)(uint64_t)t;
    int top = 127;
    while (!((t >> top) & 1)) top--;
    const int drop = top - 52;                                     // bits below the 53 kept ones
    uint64_t m = (uint64_t)(t >> drop);                            // 53 bits
    const unsigned __int128 rem = t & (((unsigned __int128)1 << drop) - 1), half = (unsigned __int128)1 << (drop - 1);
    if (rem > half || (rem == half && (m & 1))) m++;               // m may become 2^53: still exact as a double
    return ldexp((double)m, drop);
}

static inline double mis_limbs_to_double(uint64_t lo, uint64_t hi) {
    const unsigned __int128 t = ((unsigned __int128)hi << 32) + lo;
    return ldexp(mis_u128_to_double(t), -52);
}
