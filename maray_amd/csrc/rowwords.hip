// rowwords.hip — maray_jit_rowscan_apply (product code): one work-item per guard rectangle; see rowwords.hpp.  Not specific to a
// program: compiled with the library, not by hiprtc.
#include <hip/hip_runtime.h>

#include "rowwords.hpp"

extern "C" __global__ void __launch_bounds__(256) maray_jit_rowscan_apply(const unsigned long long *__restrict__ in, const unsigned char *__restrict__ changed,
                                                            unsigned long long *__restrict__ out, unsigned n_rects, unsigned nw, unsigned yrows,
                                                            unsigned threshold, unsigned long long flag, unsigned *__restrict__ n_set)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;                  // (the host keeps the rectangles of a launch below 2^32)
    if (i >= n_rects) return;
    if (maray::rowwords_rect(in + (size_t)i * nw, changed + (size_t)i * yrows, out + (size_t)i * nw, nw, yrows, threshold, flag)) atomicAdd(n_set, 1u);
}

namespace maray {

int rowwords_apply_launch(const unsigned long long *in, const unsigned char *changed, unsigned long long *out, unsigned n_rects, unsigned nw, unsigned yrows,
                          unsigned threshold, unsigned long long flag, unsigned *n_set, void *stream)
{
    if (!n_rects) return 0;
    hipLaunchKernelGGL(maray_jit_rowscan_apply, dim3((n_rects + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, in, changed, out, n_rects, nw, yrows, threshold, flag, n_set);
    return (int)hipGetLastError();
}

}   // namespace maray
