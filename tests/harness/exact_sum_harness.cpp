// exact_sum_harness.cpp -- the host half of the exact sum of norms (image_stitching_amd/csrc/exact_sum.h) as a shared object for
// tests/test_refimpl_expos_family_cpu.py: two 64-bit limb counters -> one correctly rounded double.  Plain C++, no HIP.
#include "../../image_stitching_amd/csrc/exact_sum.h"

extern "C" double harness_limbs_to_double(uint64_t lo, uint64_t hi) { return mis_limbs_to_double(lo, hi); }

// the kernel's split of one norm: sqrt(ss) * 2^52 as an integer, added to the two counters
extern "C" void harness_add_norm(int ss, uint64_t* lo, uint64_t* hi) {
    const uint64_t t = (uint64_t)(sqrt((double)ss) * MIS_EXACT_SCALE);
    *lo += t & 0xffffffffull;
    *hi += t >> 32;
}
