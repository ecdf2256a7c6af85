// Resident workgroups per compute unit of the ORB kernels whose residency is argued from their declarations (diagnostics, not part
// of the library): what the runtime computes from the code object's registers and LDS, not what the source suggests.  The kernels
// live in orb.hip's anonymous namespace, so this file is that translation unit plus a main(); build it with the library's flags:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Iimage_stitching_amd/csrc -Iinclude tools/micro/orb_occupancy.hip \
//         -Limage_stitching_amd -lmistitch -Wl,-rpath,'$ORIGIN/../../../image_stitching_amd' -o tools/micro/_bin/orb_occupancy
#include "../../image_stitching_amd/csrc/orb.hip"
#include <cstdio>

template <typename K>
static int report(const char* name, K kernel, int block) {
    hipFuncAttributes a;
    int blocks = 0;
    if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel)) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, block, 0) != hipSuccess) {
        printf("%s: %s\n", name, hipGetErrorString(hipGetLastError()));
        return 1;
    }
    printf("%-24s block %4d  registers %3d  static LDS %6zu B  resident workgroups per CU %2d  (waves per SIMD %d)\n", name, block, a.numRegs,
           a.sharedSizeBytes, blocks, blocks * (block / 64) / 4);
    return 0;
}

int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
    printf("%s: %d CUs, %zu B of LDS per workgroup at most\n", p.gcnArchName, p.multiProcessorCount, p.sharedMemPerBlock);
    int rc = report("fast_nms_kernel", fast_nms_kernel, 256);
    rc |= report("describe_direct_kernel", describe_direct_kernel, 256);
    rc |= report("harris_kernel", harris_kernel, 256);
    rc |= report("select_rank_kernel", select_rank_kernel, 1024);
    return rc;
}
