// LoRA adapters on the block linears (include/pixart_hip.h, "LoRA adapters"): the merge of s B A into the 16-bit operand copy of a weight, and the adapter
// gradients dA = s u^T x, dBt = s t^T dy with t = x A^T, u = dy Bt^T - two rank-r products per side, dW is never formed.
//
// pxa_lora_bwd is a kernel PAIR per row chunk plus one reduce, not one fused kernel.  t needs every column of a row of x before that row of dy can be used for
// dBt, and dA / dBt need every row for a column: a fused kernel either keeps r x (K + N) fp32 accumulators per workgroup (295 KB at r = 16, K + N = 4608) or
// writes them out per row tile (as many bytes as it read).  So the projection kernel writes t and u (transposed, 16-bit: 2 r M values, 0.7 % of x + dy) and the
// gradient kernel reads x and dy a second time.  The host can walk M in chunks of PXA_LORA_CHUNK_MB of x + dy, projection then gradient per chunk, so that
// the second touch finds the rows in the 256 MB Infinity Cache; measured at M = 65,536, r = 16 that buys nothing (one pair 0.316 / 0.386 ms at (K, N) =
// (1152, 3456) / (4608, 1152), 128 MB chunks 0.320 / 0.400, 48 MB chunks 0.448 / 0.534: the small launches fill the chip worse than the cache helps), so the
// default is one pair over all rows.
//
// MFMA: v_mfma_f32_16x16x32 (common.h: A[i = l&15][k = 8 (l>>4) + j], B[k][n = l&15], C: col = l&15, row = 4 (l>>4) + g).  Projection: i = token row, n = rank
// index, k = feature - both operands are 16-byte global loads.  Gradient: i = rank index, n = feature column, k = token row: the A operand is a 16-byte load of
// the transposed t / u, the B operand needs 8 ROWS of one column per lane, so the 128 x 64 tile of x / dy goes through LDS (row pitch 68 elements: the four
// 16-lane groups read 8 rows apart = 16 banks apart, conflict-free) and is read back column-wise.
#include <stdlib.h>

#include "common.h"
#include "pixart_hip.h"

namespace {
using namespace pxa;

constexpr int SPLIT_ROWS = 1024;              // rows per gradient workgroup = per fp32 partial slab
constexpr long CHUNK_BYTES = 1L << 40;        // x + dy bytes per projection / gradient pair: by default one pair over all rows (measured, see the header)
constexpr int TILE_ROWS = 128;                // token rows per LDS tile of the gradient kernel: four 16-byte loads per thread in flight
constexpr int TILE_PITCH = 68;                // LDS row pitch of that 128 x 64 tile, in elements

// 16 bytes at p when ok, zeros otherwise.  The caller passes an address that is valid either way (its index clamped into range): the load is unconditional and the
// result selected, so no pointer to a private copy of the zeros is formed (that made the load a flat one through scratch).
__device__ __forceinline__ uint4 ld16_or_zero(const bf16_t* p, bool ok) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const float* __restrict__ master, long ld, int lo, int hi, int K, const float* __restrict__ A,
                                                        const float* __restrict__ Bt, long ldbt, int r, float s, bf16_t* __restrict__ dst, long ld_dst,
                                                        bf16_t* __restrict__ dst2, long ld_dst2, int mul_lo, int mul_hi, float mul, float* dstf) {
  const int k4 = K / 4;
  const long total = (long)(hi - lo) * k4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int nl = (int)(i / k4), k = (int)(i % k4) * 4;
    const long n = lo + nl;
    const float4 w = *reinterpret_cast<const float4*>(master + n * ld + k);
    // The sum and the final add run in fp64, j ascending: the same bits whatever the grid.  fp32 would do for most elements, but where s B A cancels W the
    // fp32 error of the sum (a few 1e-8 of |W|) is many 16-bit steps of the small result; in fp64 the result is the exact value rounded to fp32 - what dst_f32
    // receives - and from there once to the operand type (the second rounding shows only on an exact 16-bit tie of the fp32 value: 2^-16 / 2^-13 of elements).
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    for (int j = 0; j < r; j++) {
      const double b = (double)Bt[(long)j * ldbt + nl];
      const float4 a = *reinterpret_cast<const float4*>(A + (long)j * K + k);
      a0 = fma(b, (double)a.x, a0); a1 = fma(b, (double)a.y, a1); a2 = fma(b, (double)a.z, a2); a3 = fma(b, (double)a.w, a3);
    }
    const double sd = (double)s;
    const double d0 = fma(sd, a0, (double)w.x), d1 = fma(sd, a1, (double)w.y), d2 = fma(sd, a2, (double)w.z), d3 = fma(sd, a3, (double)w.w);
    float4 v = make_float4((float)d0, (float)d1, (float)d2, (float)d3);
    // v is pinned as an fp32 value: left alone, the compiler folds (operand type)(float)(double) into one conversion from fp64, and the prescaled copy at s = 0
    // would no longer be bit for bit what pxa_scale_copy_f32 makes of the master (fp32 product, one rounding) - nor dst16 the rounding of dst_f32.
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    *reinterpret_cast<uint2*>(dst + n * ld_dst + k) = pack_bf16x4(v.x, v.y, v.z, v.w);
    if (dst2) {
      const float m = (n >= mul_lo && n < mul_hi) ? mul : 1.f;
      *reinterpret_cast<uint2*>(dst2 + n * ld_dst2 + k) = pack_bf16x4(v.x * m, v.y * m, v.z * m, v.w * m);
    }
    if (dstf) *reinterpret_cast<float4*>(dstf + n * ld + k) = v;
  }
}

// t^T / u^T of token rows [m0, m0 + 16 gridDim.x) (all below Mpad): blockIdx.y = 0: t = x A16^T, 1: u = dy Bt16^T.  One workgroup per 16 rows; its four waves
// take the 64-feature steps round robin and their fp32 accumulators are summed through LDS in wave order (a chunk of 10,000 rows is then 5,000 waves with two
// 16-byte loads each in flight: one wave per 16 rows left the memory system with a quarter of that and the call at 1.3 TB/s).  Rows at or past M and rank indices
// at or past r are never read (ld16_or_zero): their operands are zeros, and zeros are what lands in the padded part of t^T / u^T.
template <int NB>
__global__ __launch_bounds__(256) void lora_proj_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ dy, long lddy,
                                                       const bf16_t* __restrict__ A16, const bf16_t* __restrict__ Bt16, long M, long Mpad, int K, int N, int r,
                                                       long m0, bf16_t* __restrict__ tT, bf16_t* __restrict__ uT) {
  __shared__ f32x4 red[3][NB][64];
  const bool second = blockIdx.y != 0;
  const bf16_t* X = second ? dy : x;
  const long ld = second ? lddy : ldx;
  const bf16_t* W = second ? Bt16 : A16;
  const int C = second ? N : K;
  bf16_t* out = second ? uT : tT;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, q = lane >> 4;
  const long row0 = m0 + blockIdx.x * 16L;
  const long row = row0 + li;
  const bool rok = row < M;
  const bf16_t* xp = X + (rok ? row : M - 1) * ld + 8 * q;          // a row past M: row M - 1 is loaded and dropped
  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; nb++) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 64 * wave; k0 < C; k0 += 256) {
    const uint4 av0 = ld16_or_zero(xp + k0, rok), av1 = ld16_or_zero(xp + k0 + 32, rok);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = k0 + 32 * h;
      const bf16x8 a = __builtin_bit_cast(bf16x8, h ? av1 : av0);
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        const int rr = nb * 16 + li;
        const uint4 bv = ld16_or_zero(W + (long)(rr < r ? rr : r - 1) * C + k + 8 * q, rr < r);
        acc[nb] = mfma16(a, __builtin_bit_cast(bf16x8, bv), acc[nb]);
      }
    }
  }
  if (wave) {
#pragma unroll
    for (int nb = 0; nb < NB; nb++) red[wave - 1][nb][lane] = acc[nb];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {     // waves 0 + 1 + 2 + 3 in that order, then the one rounding of t / u; lane: rows row0 + 4 q + g of rank index 16 nb + li
      const f32x4 v = ((acc[nb] + red[0][nb][lane]) + red[1][nb][lane]) + red[2][nb][lane];
      *reinterpret_cast<uint2*>(out + (long)(nb * 16 + li) * Mpad + row0 + 4 * q) = pack_bf16x4(v[0], v[1], v[2], v[3]);
    }
  }
}

// One 64-column tile of dA (blockIdx.x < K / 64: u^T x) or of dBt (the others: t^T dy) over the rows of split `split0 + blockIdx.y`: fp32 partial
// part[split][RP][K + N], every element written by exactly one lane.
template <int NB>
__global__ __launch_bounds__(256) void lora_grad_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ dy, long lddy,
                                                       const bf16_t* __restrict__ tT, const bf16_t* __restrict__ uT, long M, long Mpad, int K, int N, int split0,
                                                       float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[2][TILE_ROWS * TILE_PITCH];
  const int kt = K / 64;
  const bool isA = (int)blockIdx.x < kt;
  const bf16_t* X = isA ? x : dy;
  const long ld = isA ? ldx : lddy;
  const int c0 = (isA ? (int)blockIdx.x : (int)blockIdx.x - kt) * 64;
  const bf16_t* P = isA ? uT : tT;
  const int split = split0 + blockIdx.y;
  const long mb = (long)split * SPLIT_ROWS;
  const long me = mb + SPLIT_ROWS < Mpad ? mb + SPLIT_ROWS : Mpad;
  const int iters = (int)((me - mb) / TILE_ROWS);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int seg = tid & 7, lrow = tid >> 3;                 // this thread's four 16-byte pieces of a tile: rows lrow + 32 i, columns 8 seg ...
  const bf16_t* xg = X + c0 + 8 * seg;
  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; nb++) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto gload = [&](long m, uint4 (&v)[4]) {                 // rows at or past M: row M - 1 is loaded and dropped, nothing past M is read
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const long rw = m + lrow + 32 * i;
      v[i] = ld16_or_zero(xg + (rw < M ? rw : M - 1) * ld, rw < M);
    }
  };
  auto lstore = [&](int buf, const uint4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint2* p = reinterpret_cast<uint2*>(&tile[buf][(lrow + 32 * i) * TILE_PITCH + 8 * seg]);
      p[0] = make_uint2(v[i].x, v[i].y);
      p[1] = make_uint2(v[i].z, v[i].w);
    }
  };
  uint4 v[4];
  gload(mb, v);
  lstore(0, v);
  __syncthreads();
  for (int it = 0; it < iters; it++) {
    const long m = mb + (long)TILE_ROWS * it;
    if (it + 1 < iters) gload(m + TILE_ROWS, v);
    const bf16_t* tl = &tile[it & 1][16 * wave + li];
    uint4 av[TILE_ROWS / 32][NB];
#pragma unroll
    for (int h = 0; h < TILE_ROWS / 32; h++)
#pragma unroll
      for (int nb = 0; nb < NB; nb++) av[h][nb] = *reinterpret_cast<const uint4*>(P + (long)(nb * 16 + li) * Mpad + m + 32 * h + 8 * q);
#pragma unroll
    for (int h = 0; h < TILE_ROWS / 32; h++) {
      bf16x8 b;
#pragma unroll
      for (int j = 0; j < 8; j++) b[j] = tl[(32 * h + 8 * q + j) * TILE_PITCH];
#pragma unroll
      for (int nb = 0; nb < NB; nb++) acc[nb] = mfma16(__builtin_bit_cast(bf16x8, av[h][nb]), b, acc[nb]);
    }
    if (it + 1 < iters) lstore((it + 1) & 1, v);
    __syncthreads();
  }
  const int RP = NB * 16, CT = K + N;
  float* o = part + (long)split * RP * CT + (isA ? c0 : K + c0) + 16 * wave + li;
#pragma unroll
  for (int nb = 0; nb < NB; nb++)
#pragma unroll
    for (int g = 0; g < 4; g++) o[(long)(nb * 16 + 4 * q + g) * CT] = acc[nb][g];
}

__global__ __launch_bounds__(256) void lora_reduce_kernel(const float* __restrict__ part, int nsplit, int RP, int r, int K, int N, float s, float* __restrict__ dA,
                                                         float* __restrict__ dBt) {
  const int CT = K + N;
  const long total = (long)r * CT;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int rr = (int)(i / CT), c = (int)(i % CT);
    float sum = 0.f;
    for (int sp = 0; sp < nsplit; sp++) sum += part[((long)sp * RP + rr) * CT + c];      // split order: the same bits from call to call
    if (c < K) dA[(long)rr * K + c] += s * sum;
    else dBt[(long)rr * N + (c - K)] += s * sum;
  }
}

inline long round_up(long v, long a) { return (v + a - 1) / a * a; }
inline long proj_bytes(long M, int r) { return round_up(2 * round_up(r, 16) * round_up(M, TILE_ROWS) * 2, 256); }
}  // namespace

extern "C" int pxa_lora_merge(const float* master, long ld, int lo, int hi, int K, const float* A, const float* Bt, long ldbt, int r, float s, void* dst16,
                              long ld_dst, void* dst2_16, long ld_dst2, int mul_lo, int mul_hi, float mul, float* dst_f32, hipStream_t stream) {
  PXA_CHECK(master && A && Bt && dst16, "pxa_lora_merge: null pointer");
  PXA_CHECK(lo >= 0 && hi > lo && K > 0 && K % 4 == 0 && r >= 1 && r <= 64, "pxa_lora_merge: need 0 <= lo < hi, K a positive multiple of 4, 1 <= r <= 64");
  PXA_CHECK(ld >= K && ld % 4 == 0 && ld_dst >= K && ld_dst % 4 == 0 && ldbt >= hi - lo && (!dst2_16 || (ld_dst2 >= K && ld_dst2 % 4 == 0)),
            "pxa_lora_merge: row pitches must cover a row and be multiples of 4");
  PXA_CHECK(((uintptr_t)master % 16) == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)dst16 % 8) == 0 && ((uintptr_t)dst2_16 % 8) == 0 &&
            ((uintptr_t)dst_f32 % 16) == 0 && ((uintptr_t)Bt % 4) == 0, "pxa_lora_merge: unaligned pointer");
  const long blocks = ((long)(hi - lo) * (K / 4) + 255) / 256;
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, stream, master, ld, lo, hi, K, A, Bt, ldbt, r, s,
                     (bf16_t*)dst16, ld_dst, (bf16_t*)dst2_16, ld_dst2, mul_lo, mul_hi, mul, dst_f32);
  PXA_LAUNCH_CHECK();
  return 0;
}

extern "C" long pxa_lora_bwd_ws_bytes(long M, int K, int N, int r) {
  if (M < 1 || K < 1 || N < 1 || r < 1 || r > 64) return -1;
  const long nsplit = (M + SPLIT_ROWS - 1) / SPLIT_ROWS;
  return proj_bytes(M, r) + nsplit * round_up(r, 16) * ((long)K + N) * 4;
}

extern "C" int pxa_lora_bwd(const void* x, long ldx, const void* dy, long lddy, const void* A16, const void* Bt16, long M, int K, int N, int r, float s,
                            float* dA, float* dBt, void* ws, long ws_bytes, hipStream_t stream) {
  PXA_CHECK(x && dy && A16 && Bt16 && dA && dBt && ws, "pxa_lora_bwd: null pointer");
  PXA_CHECK(M >= 1 && M < (1L << 31) - 2048 && r >= 1 && r <= 64, "pxa_lora_bwd: need 1 <= M < 2^31 - 2048 and 1 <= r <= 64 (got M %ld, r %d)", M, r);
  PXA_CHECK(K > 0 && N > 0 && K % 64 == 0 && N % 64 == 0, "pxa_lora_bwd: K and N must be positive multiples of 64 (got %d, %d)", K, N);
  PXA_CHECK(ldx >= K && lddy >= N && ldx % 8 == 0 && lddy % 8 == 0, "pxa_lora_bwd: row pitches must cover a row and be multiples of 8");
  PXA_CHECK(((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)A16 % 16) == 0 && ((uintptr_t)Bt16 % 16) == 0 && ((uintptr_t)ws % 256) == 0 &&
            ((uintptr_t)dA % 4) == 0 && ((uintptr_t)dBt % 4) == 0, "pxa_lora_bwd: unaligned pointer");
  PXA_CHECK(ws_bytes >= pxa_lora_bwd_ws_bytes(M, K, N, r), "pxa_lora_bwd: workspace of %ld bytes, need %ld", ws_bytes, pxa_lora_bwd_ws_bytes(M, K, N, r));
  const int NB = (r + 15) / 16, RP = NB * 16;
  const long Mpad = round_up(M, TILE_ROWS);
  const int nsplit = (int)((M + SPLIT_ROWS - 1) / SPLIT_ROWS);
  bf16_t* tT = (bf16_t*)ws;
  bf16_t* uT = tT + (long)RP * Mpad;
  float* part = (float*)((char*)ws + proj_bytes(M, r));
  const bf16_t *xb = (const bf16_t*)x, *dyb = (const bf16_t*)dy, *Ab = (const bf16_t*)A16, *Bb = (const bf16_t*)Bt16;
  long chunk_bytes = CHUNK_BYTES;
  if (const char* e = getenv("PXA_LORA_CHUNK_MB")) {                 // A/B: a value larger than x + dy = one projection and one gradient launch over all rows
    const long mb = atol(e);
    if (mb > 0) chunk_bytes = mb << 20;
  }
  long per = chunk_bytes / (((long)K + N) * 2) / SPLIT_ROWS;         // splits per chunk
  if (per < 1) per = 1;
  for (long sp0 = 0; sp0 < nsplit; sp0 += per) {
    const int ns = (int)(sp0 + per < nsplit ? per : nsplit - sp0);
    const long m0 = sp0 * SPLIT_ROWS;
    const long m1 = m0 + (long)ns * SPLIT_ROWS < Mpad ? m0 + (long)ns * SPLIT_ROWS : Mpad;
    const dim3 gp((unsigned)((m1 - m0) / 16), 2), gg((unsigned)(K / 64 + N / 64), (unsigned)ns);
#define PXA_LORA_PAIR(NB_)                                                                                                                          \
  hipLaunchKernelGGL(lora_proj_kernel<NB_>, gp, dim3(256), 0, stream, xb, ldx, dyb, lddy, Ab, Bb, M, Mpad, K, N, r, m0, tT, uT);                        \
  hipLaunchKernelGGL(lora_grad_kernel<NB_>, gg, dim3(256), 0, stream, xb, ldx, dyb, lddy, (const bf16_t*)tT, (const bf16_t*)uT, M, Mpad, K, N, (int)sp0, part)
    switch (NB) {
      case 1: PXA_LORA_PAIR(1); break;
      case 2: PXA_LORA_PAIR(2); break;
      case 3: PXA_LORA_PAIR(3); break;
      default: PXA_LORA_PAIR(4); break;
    }
#undef PXA_LORA_PAIR
    PXA_LAUNCH_CHECK();
  }
  const long blocks = ((long)r * ((long)K + N) + 255) / 256;
  hipLaunchKernelGGL(lora_reduce_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, (const float*)part, nsplit, RP, r, K, N, s, dA, dBt);
  PXA_LAUNCH_CHECK();
  return 0;
}
