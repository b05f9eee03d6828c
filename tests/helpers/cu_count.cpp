// cu_count.cpp -- prints the number of compute units of device 0 (what mk_codec_create reads to size the grids of its kernels), for
// tests that must build an input larger than one sweep of such a grid.  Host code only.
#include <hip/hip_runtime_api.h>
#include <stdio.h>

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    printf("%d\n", prop.multiProcessorCount);
    return 0;
}
