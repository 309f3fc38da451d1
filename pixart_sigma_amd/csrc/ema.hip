// Exponential moving average of the flat fp32 master weights, and the in-place exchange that lets a sampler run on it
// (the reference's ema_update / state_dict_ema: diffusion/utils/checkpoint.py:11-20,45 and the `ema_rate` of configs/PixArt_xl2_internal.py):
//   ema_update : ema <- ema + (1 - decay) (p - ema), one pass behind the optimizer step (12 bytes per element); skipped, like the step itself, when the
//                loss scaler's device record says this step overflowed - no host synchronisation, the EMA counts applied steps
//   swap       : a <-> b for two disjoint buffers, so that sampling from the EMA needs no third copy of the weights
// Both are shaped like adamw_kernel (optim.hip): 256 threads, one 16-byte access per stream per thread, grid-stride, at most 4096 blocks.
#include "common.h"
#include "../../include/pixart_hip.h"

namespace {
using namespace pxa;

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float decay,
                                                         const float* __restrict__ scaler) {
  if (scaler && scaler[2] != 0.f) return;                          // adamw_kernel's rule: the step was skipped on overflow
  const float om = 1.f - decay;
  const long n4 = n / 4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 pv = ld_f4(p + 4 * i);
    float4 ev = ld_f4(ema + 4 * i);
    ev.x = fmaf(om, pv.x - ev.x, ev.x);
    ev.y = fmaf(om, pv.y - ev.y, ev.y);
    ev.z = fmaf(om, pv.z - ev.z, ev.z);
    ev.w = fmaf(om, pv.w - ev.w, ev.w);
    st_f4(ema + 4 * i, ev);
  }
}

__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
  const long n4 = n / 4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 av = ld_f4(a + 4 * i);
    const float4 bv = ld_f4(b + 4 * i);
    st_f4(a + 4 * i, bv);
    st_f4(b + 4 * i, av);
  }
}
inline int grid_for(long n4) { long g = (n4 + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }
}  // namespace

extern "C" int pxa_ema_update(float* ema, const float* p, long n, float decay, const float* scaler, hipStream_t stream) {
  PXA_CHECK(ema && p, "pxa_ema_update: null pointer");
  PXA_CHECK(n > 0 && n % 4 == 0, "pxa_ema_update: n must be a positive multiple of 4");
  PXA_CHECK(((uintptr_t)ema % 16) == 0 && ((uintptr_t)p % 16) == 0, "pxa_ema_update: pointers must be 16-byte aligned");
  PXA_CHECK(decay >= 0.f && decay < 1.f, "pxa_ema_update: decay must lie in [0, 1)");
  PXA_CHECK(ema + n <= p || p + n <= ema, "pxa_ema_update: ema and p are the same buffer or overlap");
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for(n / 4)), dim3(256), 0, stream, ema, p, n, decay, scaler);
  PXA_LAUNCH_CHECK();
  return 0;
}

extern "C" int pxa_swap_f32(float* a, float* b, long n, hipStream_t stream) {
  PXA_CHECK(a && b, "pxa_swap_f32: null pointer");
  PXA_CHECK(n > 0 && n % 4 == 0, "pxa_swap_f32: n must be a positive multiple of 4");
  PXA_CHECK(((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0, "pxa_swap_f32: pointers must be 16-byte aligned");
  PXA_CHECK(a + n <= b || b + n <= a, "pxa_swap_f32: the two ranges overlap");
  hipLaunchKernelGGL(swap_kernel, dim3(grid_for(n / 4)), dim3(256), 0, stream, a, b, n);
  PXA_LAUNCH_CHECK();
  return 0;
}
