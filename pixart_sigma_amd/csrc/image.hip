// Image side of the feature pipeline (include/pixart_hip.h, "Images"): Pillow's 8-bit separable resampler restated for one uint8 HWC RGB image, and the
// float -> uint8 conversion of torchvision.utils.save_image.  Integer arithmetic throughout the resampler: the 22-bit fixed-point coefficient tables come from
// the host (pixart_sigma_amd/data/images.py, float64 exactly as Pillow computes them), so every byte is the byte Image.resize gives.
//
// pxa_image_resample is two kernels, as Pillow's two passes: the horizontal pass writes a uint8 intermediate, the vertical pass reads it.  Both work on the crop
// window only: the horizontal pass computes the window's columns of the source rows [row0, row0 + rows) that the window's vertical taps reach, the vertical pass
// the window's pixels.  A pass whose size does not change is not launched: the other one then reads the source or writes the output directly, and with neither
// the vertical kernel copies the window (no taps).
//
// Mapping: one thread per output PIXEL (three int32 accumulators), 256 consecutive x per workgroup, one image row per blockIdx.y.
//   vertical:   the tap row of output row y is the same for the whole workgroup (uniform address: scalar loads), a wave reads 192 contiguous source bytes per tap
//               and writes 256 contiguous bytes per fp32 plane.
//   horizontal: lane x reads taps xmin(x) .. xmin(x) + n(x): neighbouring lanes' windows overlap and are `scale` pixels apart, so a wave's loads of one tap fall
//               into a few cache lines that the next taps hit again in L1.  The coefficient table is stored TAP-major ([tap][x]) so that a wave's coefficient load
//               is one contiguous 256 bytes.  The source segment is not staged in LDS: measured numbers in DESIGN.md section 4g.
// Tap loops run to n from the bounds table (clamped to the table's row length and the source size, so a wrong table reads nothing out of bounds).
#include "common.h"
#include "pixart_hip.h"

namespace {

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> 22;                      // arithmetic shift: the accumulator can be negative (negative lobes of bicubic / lanczos)
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One finished pixel: fp32 planes through the 256-entry table (slot base `outf`, plane pitch `plane`, row pitch cw) or uint8 HWC (row pitch `pitch` bytes).
__device__ __forceinline__ void put_pixel(int r, int g, int b, int y, int x, int cw, float* __restrict__ outf, long plane, const float* lut,
                                          uint8_t* __restrict__ out8, long pitch) {
  if (outf) {
    float* o = outf + (long)y * cw + x;
    o[0] = lut[r];
    o[plane] = lut[g];
    o[2 * plane] = lut[b];
  } else {
    uint8_t* o = out8 + (long)y * pitch + 3L * x;
    o[0] = (uint8_t)r;
    o[1] = (uint8_t)g;
    o[2] = (uint8_t)b;
  }
}

// Columns [cx, cx + cw) of the resized rows y0 .. y0 + gridDim.y - 1 of the source (w pixels per row); output row index = blockIdx.y.
__global__ __launch_bounds__(256) void image_hpass_kernel(const uint8_t* __restrict__ src, long src_pitch, int w, int y0, const int* __restrict__ hk,
                                                         const int* __restrict__ hb, int ksize, int Wr, int cx, int cw, float* __restrict__ outf, long plane,
                                                         const float* __restrict__ lut_g, uint8_t* __restrict__ out8, long pitch) {
  __shared__ float lut[256];
  if (outf) {
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
  }
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= cw) return;
  const int xx = cx + x;
  int xmin = hb[2 * xx], n = hb[2 * xx + 1];
  xmin = xmin < 0 ? 0 : (xmin > w ? w : xmin);
  n = n > ksize ? ksize : n;
  n = n > w - xmin ? w - xmin : n;
  const uint8_t* p = src + (long)(y0 + (int)blockIdx.y) * src_pitch + 3L * xmin;
  const int* k = hk + xx;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  for (int t = 0; t < n; t++) {
    const int kk = k[(long)t * Wr];
    a0 += p[0] * kk;
    a1 += p[1] * kk;
    a2 += p[2] * kk;
    p += 3;
  }
  put_pixel(clip8(a0), clip8(a1), clip8(a2), blockIdx.y, x, cw, outf, plane, lut, out8, pitch);
}

// Rows [cy, cy + gridDim.y) of the vertically resized image.  `in` holds in_rows rows (pitch in_pitch) of which the first is row in_row0 of the pass's source; its
// column 0 is column -in_col0 of the window (in_col0 = cx when `in` is the source itself, 0 when it is the intermediate).  vk == NULL: no taps, row cy + y is copied.
__global__ __launch_bounds__(256) void image_vpass_kernel(const uint8_t* __restrict__ in, long in_pitch, int in_row0, int in_rows, int in_col0,
                                                         const int* __restrict__ vk, const int* __restrict__ vb, int ksize, int cy, int cw,
                                                         float* __restrict__ outf, long plane, const float* __restrict__ lut_g, uint8_t* __restrict__ out8,
                                                         long pitch) {
  __shared__ float lut[256];
  if (outf) {
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
  }
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= cw) return;
  const int yy = cy + blockIdx.y;
  int r = (vk ? vb[2 * yy] : yy) - in_row0, n = vk ? vb[2 * yy + 1] : 1;
  r = r < 0 ? 0 : (r > in_rows ? in_rows : r);
  n = n > in_rows - r ? in_rows - r : n;
  const uint8_t* p = in + (long)r * in_pitch + 3L * (in_col0 + x);
  int c0, c1, c2;
  if (vk) {
    n = n > ksize ? ksize : n;
    const int* k = vk + (long)yy * ksize;
    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int t = 0; t < n; t++) {
      const int kk = k[t];
      a0 += p[0] * kk;
      a1 += p[1] * kk;
      a2 += p[2] * kk;
      p += in_pitch;
    }
    c0 = clip8(a0); c1 = clip8(a1); c2 = clip8(a2);
  } else {
    c0 = n > 0 ? p[0] : 0; c1 = n > 0 ? p[1] : 0; c2 = n > 0 ? p[2] : 0;
  }
  put_pixel(c0, c1, c2, blockIdx.y, x, cw, outf, plane, lut, out8, pitch);
}

// save_image(normalize=True, value_range=(-1, 1)): clamp, (x + 1) / 2, * 255 + 0.5, clamp, truncate - each step rounded to fp32 by itself (no fused
// multiply-add: torch does them as separate passes over the tensor).
template <typename T>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const T* __restrict__ x, uint8_t* __restrict__ out, long hw, long total) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long b = i / hw, p = i - b * hw;
    const T* s = x + b * 3 * hw + p;
    uint8_t* o = out + 3 * i;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float v = (float)s[c * hw];
      v = fminf(fmaxf(v, -1.f), 1.f);
      v = __fdiv_rn(__fadd_rn(v, 1.f), 2.f);
      v = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);
      v = fminf(fmaxf(v, 0.f), 255.f);
      o[c] = (uint8_t)(int)v;
    }
  }
}
}  // namespace

extern "C" long pxa_image_resample_ws_bytes(int rows, int cw) {
  if (rows < 1 || cw < 1) return -1;
  return (long)rows * cw * 3;
}

extern "C" int pxa_image_resample(const void* src, long src_pitch, int h, int w, const int* hk, const int* hb, int hksize, int Wr, const int* vk, const int* vb,
                                  int vksize, int Hr, int cy, int cx, int ch, int cw, int row0, int rows, void* ws, long ws_bytes, float* out_f32,
                                  const float* lut, void* out_u8, long out_pitch, hipStream_t stream) {
  PXA_CHECK(src && h >= 1 && w >= 1 && h <= 65535 && w <= 65535 && src_pitch >= 3L * w, "pxa_image_resample: need a source of 1 .. 65535 pixels a side and a row pitch >= 3 w");
  PXA_CHECK((hk != nullptr) == (hb != nullptr) && (vk != nullptr) == (vb != nullptr), "pxa_image_resample: coefficients and bounds of an axis come together");
  PXA_CHECK(hk ? (hksize >= 1 && Wr >= 1 && Wr <= 65535) : Wr == w, "pxa_image_resample: no horizontal tables means Wr == w (got Wr %d, w %d, ksize %d)", Wr, w, hksize);
  PXA_CHECK(vk ? (vksize >= 1 && Hr >= 1 && Hr <= 65535) : Hr == h, "pxa_image_resample: no vertical tables means Hr == h (got Hr %d, h %d, ksize %d)", Hr, h, vksize);
  PXA_CHECK(ch >= 1 && cw >= 1 && cy >= 0 && cx >= 0 && cy + ch <= Hr && cx + cw <= Wr, "pxa_image_resample: window (%d, %d, %d, %d) outside the resized image %d x %d",
            cy, cx, ch, cw, Hr, Wr);
  PXA_CHECK((out_f32 != nullptr) != (out_u8 != nullptr), "pxa_image_resample: exactly one of out_f32 and out_u8");
  PXA_CHECK(out_f32 ? (lut != nullptr && ((uintptr_t)out_f32 % 4) == 0 && ((uintptr_t)lut % 4) == 0) : out_pitch >= 3L * cw,
            "pxa_image_resample: out_f32 needs the 256-entry table, out_u8 a row pitch >= 3 cw");
  PXA_CHECK(((uintptr_t)hk % 4) == 0 && ((uintptr_t)hb % 4) == 0 && ((uintptr_t)vk % 4) == 0 && ((uintptr_t)vb % 4) == 0, "pxa_image_resample: unaligned table");
  if (!vk) row0 = cy, rows = ch;                 // without a vertical pass the rows the window needs are its own
  PXA_CHECK(row0 >= 0 && rows >= 1 && row0 + rows <= h, "pxa_image_resample: source rows [%d, %d) outside the image (h = %d)", row0, row0 + rows, h);
  const uint8_t* s8 = (const uint8_t*)src;
  const long plane = (long)ch * cw;
  const dim3 block(256);
  const unsigned gx = (unsigned)((cw + 255) / 256);
  if (hk && vk) {
    PXA_CHECK(ws && ws_bytes >= pxa_image_resample_ws_bytes(rows, cw), "pxa_image_resample: workspace of %ld bytes, need %ld", ws_bytes,
              pxa_image_resample_ws_bytes(rows, cw));
    const long wp = 3L * cw;
    hipLaunchKernelGGL(image_hpass_kernel, dim3(gx, (unsigned)rows), block, 0, stream, s8, src_pitch, w, row0, hk, hb, hksize, Wr, cx, cw, (float*)nullptr, 0L,
                       (const float*)nullptr, (uint8_t*)ws, wp);
    hipLaunchKernelGGL(image_vpass_kernel, dim3(gx, (unsigned)ch), block, 0, stream, (const uint8_t*)ws, wp, row0, rows, 0, vk, vb, vksize, cy, cw, out_f32, plane, lut,
                       (uint8_t*)out_u8, out_pitch);
  } else if (hk) {
    hipLaunchKernelGGL(image_hpass_kernel, dim3(gx, (unsigned)ch), block, 0, stream, s8, src_pitch, w, cy, hk, hb, hksize, Wr, cx, cw, out_f32, plane, lut,
                       (uint8_t*)out_u8, out_pitch);
  } else {                                       // vertical pass on the source itself, or (no tables at all) the window copied
    hipLaunchKernelGGL(image_vpass_kernel, dim3(gx, (unsigned)ch), block, 0, stream, s8, src_pitch, 0, h, cx, vk, vb, vksize, cy, cw, out_f32, plane, lut,
                       (uint8_t*)out_u8, out_pitch);
  }
  PXA_LAUNCH_CHECK();
  return 0;
}

extern "C" int pxa_image_to_u8(const void* x, int is_f16, long B, int H, int W, void* out_u8, hipStream_t stream) {
  PXA_CHECK(x && out_u8 && B >= 1 && H >= 1 && W >= 1, "pxa_image_to_u8: null pointer or empty image");
  PXA_CHECK(((uintptr_t)x % (is_f16 ? 2 : 4)) == 0, "pxa_image_to_u8: unaligned input");
  const long hw = (long)H * W, total = B * hw;
  const long blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
  if (is_f16) hipLaunchKernelGGL(image_to_u8_kernel<_Float16>, grid, dim3(256), 0, stream, (const _Float16*)x, (uint8_t*)out_u8, hw, total);
  else hipLaunchKernelGGL(image_to_u8_kernel<float>, grid, dim3(256), 0, stream, (const float*)x, (uint8_t*)out_u8, hw, total);
  PXA_LAUNCH_CHECK();
  return 0;
}
