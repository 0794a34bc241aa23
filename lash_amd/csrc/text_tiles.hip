// text_tiles.hip — the one kernel of text_tiles.h: the single-workgroup scan of a table of per-tile or per-record counts, for the record index
// (u32, out of place) and for the coordinate, window and translate tables (u64, in place).
#include "text_tiles.h"

namespace lash {

template <typename T>
__global__ void __launch_bounds__(1024) tile_scan_kernel(const T *in, T *out, uint32_t n)
{
    __shared__ T part[1024];
    run_scan_1024(in, out, n, part, out + n);
}

hipError_t launch_tile_scan(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(tile_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, stream, d_in, d_out, n);
    return hipGetLastError();
}

hipError_t launch_tile_scan(const uint64_t *d_in, uint64_t *d_out, uint32_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(tile_scan_kernel<uint64_t>, dim3(1), dim3(1024), 0, stream, d_in, d_out, n);
    return hipGetLastError();
}

}  // namespace lash
