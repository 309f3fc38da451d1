// FP8 (OCP e4m3fn) weight storage for the T5 encoder: the row quantiser, the row dequantiser and a weight-streaming W8A16 GEMM.
//
// Format.  A weight matrix W (N, K) is held as q (N, K), one e4m3fn byte per element, and scale (N,) fp32 with W ~ scale[n] * q[n][k].  The project's quantiser
// (pxa_fp8_quant_rows) takes scale[n] = 2^ceil(log2(amax_n / 448)) (1 for an all-zero row, never below 2^-126) and q = e4m3fn(w / scale), round to nearest even,
// clamped to +-448 in fp32 before the conversion, so the NaN codes 0x7F / 0xFF are never produced.  The scale is a power of two: w / scale is exact, scale * q is
// exactly representable in bf16 (and in fp16 inside its normal range), so the dequantised matrix (pxa_fp8_dequant_rows -> pxa_gemm) and the streamed one
// (pxa_gemm_w8) are the same numbers.  The scale is computed on the bits of amax (exponent e, mantissa f: amax / 448 = (f / 1.75) 2^(e - 8), so the exponent is
// e - 8, or e - 7 where f > 1.75): no logarithm is evaluated.
//
// pxa_gemm_w8: C[m][n] = scale[n] * sum_k A[m][k] q[n][k], NT.  The FP8 bytes are widened to the operand type in registers (v_cvt_scalef32_pk_{bf16,f16}_fp8 with
// scale 1: exact in both types, e4m3 spans 2^-9 .. 448) and multiplied on v_mfma_f32_16x16x32; the activations are not quantised; scale[n] multiplies the fp32
// accumulator in the epilogue.
//
// Decomposition.  A workgroup of 4 waves owns 64 rows of A and 64 NB columns (NB = 1 or 2); a wave owns 16 NB columns and all 64 rows.  The weights of a wave are
// its own: they go straight from global memory to registers, 16 bytes per lane and load (lane (t, g) = (l & 15, l >> 4) takes row n0 + t, bytes k0 + 16 g ..
// k0 + 16 g + 15: 64-byte row segments, two loads cover a 128-byte line), two k-chunks of 128 ahead of the MFMAs that use them (a ring of three register sets).  The
// A tile (64 x 128) is shared by the four waves and re-read by every column tile: it goes through LDS in full 256-byte rows (16-byte pieces, staged in registers
// and loaded two chunks ahead; row pitch 272 bytes, so the 16 rows of a fragment read fall on 16 different 16-byte bank groups), two buffers, one barrier per chunk.  Which k a lane's fragment element
// stands for is free as long as both operands agree: MFMA step (h, s) of a chunk uses bytes 8 s .. 8 s + 7 of weight load h, k = k0 + 64 h + 16 g + 8 s + j, and
// reads the A fragment from that column of the LDS row.  The product is written transposed (a = W fragment, b = A fragment), so a lane owns 4 consecutive columns
// of one row: 8-byte 16-bit stores, 16-byte fp32 read-modify-writes, one float4 of scales.
// No K split: every output element is summed by one lane in one fixed order, so two launches give the same bits; no atomics, no workspace, no workgroup waits for
// another.  The M / 64 row tiles of one column tile re-read its weights; consecutive workgroup ids of one XCD (id mod 8) take the row tiles of one column tile, so
// the re-read is served by that XCD's L2.  NB = 1 is taken where NB = 2 would leave fewer workgroups than CUs.
// Ragged edges: rows at or past M and columns at or past N are clamped at the load (nothing outside the operands is read) and not stored; a k piece at or past K
// (K % 16 == 0: a piece is wholly inside or outside) is read from the last piece of its row instead, and its weights are zero at the MFMA.
#include "common.h"
#include "../../include/pixart_hip.h"

#include <cstdio>
#include <type_traits>

namespace {
using namespace pxa;

constexpr int W8_MAX_M = 2048;
constexpr int W8_BM = 64, W8_BK = 128, W8_WAVES = 4;
constexpr int W8_PITCH = W8_BK * 2 + 16;                 // bytes of an LDS row of the A tile
constexpr int W8_STAGE = W8_BM * W8_PITCH;
constexpr int W8_CUS = 256;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// two FP8 bytes (the low or high half of `v`) -> two operand-type values, exact
__device__ __forceinline__ bf16x2 fp8x2_to_operand(uint32_t v, bool hi) {
#ifdef PXA_OPERAND_F16
  return hi ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)v, 1.0f, false);
#else
  return hi ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, false);
#endif
}
__device__ __forceinline__ bf16x8 fp8x8_to_operand(uint32_t lo, uint32_t hi) {
  const bf16x2 a = fp8x2_to_operand(lo, false), b = fp8x2_to_operand(lo, true), c = fp8x2_to_operand(hi, false), d = fp8x2_to_operand(hi, true);
  bf16x8 r;
  r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1]; r[4] = c[0]; r[5] = c[1]; r[6] = d[0]; r[7] = d[1];
  return r;
}
__device__ __forceinline__ void fp8x4_to_f32(uint32_t v, float (&f)[4]) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v, true);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
}

// ------------------------------------------------------------------------------------------------ quantiser
template <bool F32>
__device__ __forceinline__ void quant_load16(const void* row, int c, float (&f)[16]) {
  if (F32) {
    const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(row) + c);
#pragma unroll
    for (int i = 0; i < 4; i++) { const float4 v = p[i]; f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w; }
  } else {
    const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(row) + c);
    float lo[8], hi[8];
    unpack_bf16x8(p[0], lo);
    unpack_bf16x8(p[1], hi);
#pragma unroll
    for (int i = 0; i < 8; i++) { f[i] = lo[i]; f[8 + i] = hi[i]; }
  }
}

// One workgroup per row, two sweeps: the maximum, then the codes (the second sweep re-reads the row from L2, as t5_rmsnorm_kernel does).
template <bool F32>
__global__ __launch_bounds__(256) void fp8_quant_rows_kernel(const void* __restrict__ src, long ld, int K, uint8_t* __restrict__ q, long ldq, float* __restrict__ scale) {
  __shared__ float part[4];
  const long n = blockIdx.x;
  const void* row = F32 ? (const void*)(reinterpret_cast<const float*>(src) + n * ld) : (const void*)(reinterpret_cast<const bf16_t*>(src) + n * ld);
  float amax = 0.f;
  for (int c = threadIdx.x * 16; c < K; c += 256 * 16) {
    float f[16];
    quant_load16<F32>(row, c, f);
#pragma unroll
    for (int i = 0; i < 16; i++) amax = fmaxf(amax, fabsf(f[i]));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
  // scale = 2^ceil(log2(amax / 448)) from the bits of amax; 448 = 1.75 * 2^8
  const uint32_t bits = __builtin_bit_cast(uint32_t, amax);
  int se = (int)(bits >> 23) - 127 - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
  se = max(se, -126);
  if (amax == 0.f) se = 0;
  const float s = __builtin_bit_cast(float, (uint32_t)(se + 127) << 23), inv = __builtin_bit_cast(float, (uint32_t)(127 - se) << 23);
  if (threadIdx.x == 0) scale[n] = s;
  for (int c = threadIdx.x * 16; c < K; c += 256 * 16) {
    float f[16];
    quant_load16<F32>(row, c, f);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = fminf(fmaxf(f[4 * i + j] * inv, -448.f), 448.f);      // * inv = / s exactly: s is a power of two
      int r = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
      r = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], r, true);
      w[i] = (uint32_t)r;
    }
    *reinterpret_cast<uint4*>(q + n * ldq + c) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// dst[n][k] = round16(scale[n] * q[n][k]): 16 bytes in, 32 bytes out per thread and step.
__global__ __launch_bounds__(256) void fp8_dequant_rows_kernel(const uint8_t* __restrict__ q, long ldq, const float* __restrict__ scale, int N, int K,
                                                               bf16_t* __restrict__ dst, long ld) {
  const long per_row = K / 16, total = (long)N * per_row;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long n = i / per_row;
    const int c = (int)(i - n * per_row) * 16;
    const float s = scale[n];
    const uint4 v = *reinterpret_cast<const uint4*>(q + n * ldq + c);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float f[4];
      fp8x4_to_f32(w[j], f);
      o[2 * j] = pack_bf16x2(f[0] * s, f[1] * s);
      o[2 * j + 1] = pack_bf16x2(f[2] * s, f[3] * s);
    }
    uint4* d = reinterpret_cast<uint4*>(dst + n * ld + c);
    d[0] = make_uint4(o[0], o[1], o[2], o[3]);
    d[1] = make_uint4(o[4], o[5], o[6], o[7]);
  }
}

// ------------------------------------------------------------------------------------------------ the GEMM
struct W8Params {
  const bf16_t* A; long lda;
  const uint8_t* q; long ldq;
  const float* scale;
  int M, N, K;
  const bf16_t* aux; long ldaux;
  bf16_t* out16; long ld_out;
  float* out_f32; long ld_f32;
  int m_tiles, n_tiles;
};

// a thread's four 16-byte pieces of an A tile.  Native vectors, not uint4: copies of the HIP struct type become memcpy calls between address spaces, and the
// staging sets then stay in scratch memory.
struct A4 { nt_u4 p0, p1, p2, p3; };

enum { W8_STORE = 0, W8_GELU = 1, W8_MUL_AUX = 2, W8_ADD_F32 = 3 };

template <int NB, int EPI>
__global__ __launch_bounds__(256) void gemm_w8_kernel(const W8Params p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * W8_STAGE];
  // id -> (column tile, row tile): ids of one XCD (id & 7) walk the row tiles of a column tile first
  const int bid = blockIdx.x, r8 = bid >> 3;
  const int mt = r8 % p.m_tiles, nt = (r8 / p.m_tiles) * 8 + (bid & 7);
  if (nt >= p.n_tiles) return;                                       // the whole workgroup: no barrier is left behind
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t = lane & 15, g = lane >> 4;
  const int m0 = mt * W8_BM, n0 = nt * (W8_WAVES * 16 * NB) + wave * 16 * NB;
  const int M = p.M, N = p.N, K = p.K;

  // A staging: 64 rows x 16 pieces of 16 bytes; thread takes pieces tid + 256 i: row (tid >> 4) + 16 i, piece tid & 15
  const int a_pc = tid & 15;
  const bf16_t* a_src[4];
  int a_dst[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int row = (tid >> 4) + 16 * i;
    a_src[i] = p.A + (long)min(m0 + row, M - 1) * p.lda + a_pc * 8;
    a_dst[i] = row * W8_PITCH + a_pc * 16;
  }
  const uint8_t* w_src[NB];
#pragma unroll
  for (int nb = 0; nb < NB; nb++) w_src[nb] = p.q + (long)min(n0 + nb * 16 + t, N - 1) * p.ldq + 16 * g;

  // Every load is unconditional, so that it stays in flight until its first use (a load under a condition is joined with its zero right behind it, which
  // waits for it): a piece at or past K is read from the last piece of the same row instead.  Its weights are zeroed where they are used, and an A value
  // that meets a zero weight is a real element of the same row - if that one is not finite, the row's true result is not finite either.
  auto load_a = [&](int k0, A4& ar) {
    const int k = min(k0 + a_pc * 8, K - 8) - a_pc * 8;
    ar.p0 = *reinterpret_cast<const nt_u4*>(a_src[0] + k);
    ar.p1 = *reinterpret_cast<const nt_u4*>(a_src[1] + k);
    ar.p2 = *reinterpret_cast<const nt_u4*>(a_src[2] + k);
    ar.p3 = *reinterpret_cast<const nt_u4*>(a_src[3] + k);
  };
  auto load_w = [&](int k0, uint4 (&wr)[NB][2]) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = min(k0 + 64 * h + 16 * g, K - 16);
#pragma unroll
      for (int nb = 0; nb < NB; nb++) wr[nb][h] = *reinterpret_cast<const uint4*>(w_src[nb] + (k - 16 * g));
    }
  };
  auto store_a = [&](char* st, const A4& ar) {
    *reinterpret_cast<nt_u4*>(st + a_dst[0]) = ar.p0;
    *reinterpret_cast<nt_u4*>(st + a_dst[1]) = ar.p1;
    *reinterpret_cast<nt_u4*>(st + a_dst[2]) = ar.p2;
    *reinterpret_cast<nt_u4*>(st + a_dst[3]) = ar.p3;
  };

  f32x4 acc[4][NB];
#pragma unroll
  for (int mb = 0; mb < 4; mb++)
#pragma unroll
    for (int nb = 0; nb < NB; nb++) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Software pipeline, all of it in compiler-tracked loads (no wait is written by hand): at step c the weights of chunk c + 2 start towards ring slot
  // (c + 2) % 3 and the A pieces of chunk c + 2 towards staging set c & 1, the MFMAs of chunk c read LDS buffer c & 1 and ring slot c % 3, then the A pieces of
  // chunk c + 1 (in flight since step c - 1) go to LDS buffer (c + 1) & 1 - which every wave left at the barrier of step c - 1.  The slots are compile-time
  // indices: the loop is unrolled by 6 = lcm(2, 3).
  A4 a0, a1;
  uint4 w0[NB][2], w1[NB][2], w2[NB][2];
  load_a(0, a0);
  load_w(0, w0);
  load_a(W8_BK, a1);
  load_w(W8_BK, w1);
  store_a(smem, a0);
  __syncthreads();

  const int nchunks = (K + W8_BK - 1) / W8_BK;
  const int frag_off = t * W8_PITCH + 32 * g;                         // byte offset of (row t, k = 16 g) in a tile
  // step c: w_use = chunk c's weights, w_fill / a_fill take chunk c + 2, a_store holds chunk c + 1; ja = c & 1
  auto step = [&](uint4 (&w_use)[NB][2], uint4 (&w_fill)[NB][2], A4& a_fill, A4& a_store, auto id, int c) __attribute__((always_inline)) {
    constexpr int ja = decltype(id)::value & 1;
    const char* st = smem + ja * W8_STAGE;
    load_a((c + 2) * W8_BK, a_fill);
    load_w((c + 2) * W8_BK, w_fill);
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
      for (int s = 0; s < 2; s++) {
        bf16x8 af[4];
#pragma unroll
        for (int mb = 0; mb < 4; mb++) af[mb] = *reinterpret_cast<const bf16x8*>(st + frag_off + mb * 16 * W8_PITCH + 128 * h + 16 * s);
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
          uint4 w = w_use[nb][h];
          if (c * W8_BK + 64 * h + 16 * g >= K) w = make_uint4(0, 0, 0, 0);          // the ragged end of K: these 16 weights do not exist
          const bf16x8 wf = s == 0 ? fp8x8_to_operand(w.x, w.y) : fp8x8_to_operand(w.z, w.w);
#pragma unroll
          for (int mb = 0; mb < 4; mb++) acc[mb][nb] = mfma16(wf, af[mb], acc[mb][nb]);
        }
      }
    }
    store_a(smem + (1 - ja) * W8_STAGE, a_store);                      // chunk c + 1 (past the last chunk: never read)
    __syncthreads();
    // A different last statement in each of the six copies: identical tails would be merged into one block that picks its register set through a
    // pointer, and the staging sets would then live in scratch memory.
    asm volatile("; gemm_w8 step %0" ::"n"(decltype(id)::value));
  };
  for (int c = 0; c < nchunks; c += 6) {                               // every condition is uniform over the workgroup
    step(w0, w2, a0, a1, std::integral_constant<int, 0>{}, c);
    if (c + 1 < nchunks) step(w1, w0, a1, a0, std::integral_constant<int, 1>{}, c + 1);
    if (c + 2 < nchunks) step(w2, w1, a0, a1, std::integral_constant<int, 2>{}, c + 2);
    if (c + 3 < nchunks) step(w0, w2, a1, a0, std::integral_constant<int, 3>{}, c + 3);
    if (c + 4 < nchunks) step(w1, w0, a0, a1, std::integral_constant<int, 4>{}, c + 4);
    if (c + 5 < nchunks) step(w2, w1, a1, a0, std::integral_constant<int, 5>{}, c + 5);
  }

  // lane (t, g): row m0 + 16 mb + t, columns n0 + 16 nb + 4 g .. + 3 (N % 8 == 0: the four are inside together or outside together)
#pragma unroll
  for (int nb = 0; nb < NB; nb++) {
    const int n = n0 + nb * 16 + 4 * g;
    if (n >= N) continue;
    const float4 sc = *reinterpret_cast<const float4*>(p.scale + n);
#pragma unroll
    for (int mb = 0; mb < 4; mb++) {
      const long m = m0 + mb * 16 + t;
      if (m >= M) continue;
      float v[4] = {acc[mb][nb][0] * sc.x, acc[mb][nb][1] * sc.y, acc[mb][nb][2] * sc.z, acc[mb][nb][3] * sc.w};
      if (EPI == W8_ADD_F32) {
        float4* o = reinterpret_cast<float4*>(p.out_f32 + m * p.ld_f32 + n);
        const float4 x = *o;
        *o = make_float4(x.x + v[0], x.y + v[1], x.z + v[2], x.w + v[3]);
      } else {
        if (EPI == W8_GELU) {
#pragma unroll
          for (int j = 0; j < 4; j++) v[j] = gelu_tanh(v[j]);
        }
        if (EPI == W8_MUL_AUX) {
          const uint2 x = *reinterpret_cast<const uint2*>(p.aux + m * p.ldaux + n);
          float f[4];
          unpack_bf16x2(x.x, f[0], f[1]);
          unpack_bf16x2(x.y, f[2], f[3]);
#pragma unroll
          for (int j = 0; j < 4; j++) v[j] *= f[j];
        }
        *reinterpret_cast<uint2*>(p.out16 + m * p.ld_out + n) = pack_bf16x4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

struct W8Plan {
  int nb, epi, m_tiles, n_tiles, grid;
};

// Every refusal of pxa_gemm_w8, before any HIP call; pxa_gemm_w8_plan runs the same code.
int w8_plan(const pxa_gemm_w8_args* a, const char* who, W8Plan* pl) {
  PXA_CHECK(a, "%s: null pointer (args)", who);
  PXA_CHECK(a->M >= 1 && a->M <= W8_MAX_M, "%s: M=%d out of range (1 .. %d)", who, a->M, W8_MAX_M);
  PXA_CHECK(a->N >= 8 && a->N % 8 == 0, "%s: N=%d must be a positive multiple of 8", who, a->N);
  PXA_CHECK(a->K >= 16 && a->K % 16 == 0, "%s: K=%d must be a positive multiple of 16", who, a->K);
  PXA_CHECK(a->A && a->q && a->scale, "%s: null pointer (A, q, scale)", who);
  PXA_CHECK(a->lda >= a->K && a->lda % 8 == 0, "%s: lda=%ld must be >= K and a multiple of 8", who, a->lda);
  PXA_CHECK(a->ldq >= a->K && a->ldq % 16 == 0, "%s: ldq=%ld must be >= K and a multiple of 16 (bytes)", who, a->ldq);
  PXA_CHECK(((uintptr_t)a->A | (uintptr_t)a->q | (uintptr_t)a->scale) % 16 == 0, "%s: A, q, scale must be 16-byte aligned", who);
  PXA_CHECK(a->act == 0 || a->act == 1 || a->act == 4, "%s: act=%d is not built (0 none, 1 GELU(tanh), 4 multiply by aux)", who, a->act);
  PXA_CHECK((a->out16 != nullptr) != (a->out_f32 != nullptr), "%s: exactly one of out16 and out_f32 must be given", who);
  int epi;
  if (a->out_f32) {
    PXA_CHECK(a->act == 0, "%s: out_f32 (the accumulating fp32 residual) takes act 0, got %d", who, a->act);
    PXA_CHECK(a->ld_f32 >= a->N && a->ld_f32 % 8 == 0, "%s: ld_f32=%ld must be >= N and a multiple of 8", who, a->ld_f32);
    PXA_CHECK((uintptr_t)a->out_f32 % 16 == 0, "%s: out_f32 must be 16-byte aligned", who);
    epi = W8_ADD_F32;
  } else {
    PXA_CHECK(a->ld_out >= a->N && a->ld_out % 8 == 0, "%s: ld_out=%ld must be >= N and a multiple of 8", who, a->ld_out);
    PXA_CHECK((uintptr_t)a->out16 % 16 == 0, "%s: out16 must be 16-byte aligned", who);
    epi = a->act == 1 ? W8_GELU : a->act == 4 ? W8_MUL_AUX : W8_STORE;
    if (a->act == 4) {
      PXA_CHECK(a->aux, "%s: act 4 needs aux", who);
      PXA_CHECK(a->ldaux >= a->N && a->ldaux % 8 == 0, "%s: ldaux=%ld must be >= N and a multiple of 8", who, a->ldaux);
      PXA_CHECK((uintptr_t)a->aux % 16 == 0, "%s: aux must be 16-byte aligned", who);
    }
  }
  pl->epi = epi;
  pl->m_tiles = (a->M + W8_BM - 1) / W8_BM;
  const int wide = (a->N + 127) / 128;
  pl->nb = (long)wide * pl->m_tiles >= W8_CUS ? 2 : 1;
  pl->n_tiles = (a->N + 64 * pl->nb - 1) / (64 * pl->nb);
  pl->grid = (pl->n_tiles + 7) / 8 * 8 * pl->m_tiles;
  return 0;
}

template <int NB>
void w8_launch(int epi, int grid, hipStream_t stream, const W8Params& p) {
  switch (epi) {
    case W8_STORE: hipLaunchKernelGGL((gemm_w8_kernel<NB, W8_STORE>), dim3(grid), dim3(256), 0, stream, p); break;
    case W8_GELU: hipLaunchKernelGGL((gemm_w8_kernel<NB, W8_GELU>), dim3(grid), dim3(256), 0, stream, p); break;
    case W8_MUL_AUX: hipLaunchKernelGGL((gemm_w8_kernel<NB, W8_MUL_AUX>), dim3(grid), dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL((gemm_w8_kernel<NB, W8_ADD_F32>), dim3(grid), dim3(256), 0, stream, p); break;
  }
}
}  // namespace

extern "C" int pxa_gemm_w8_max_m(void) { return W8_MAX_M; }

extern "C" int pxa_gemm_w8_plan(const pxa_gemm_w8_args* a, char* out, int out_len) {
  W8Plan pl;
  const int rc = w8_plan(a, "pxa_gemm_w8_plan", &pl);
  if (rc) return rc;
  PXA_CHECK(out && out_len > 0, "pxa_gemm_w8_plan: no output buffer");
  snprintf(out, (size_t)out_len, "gemm_w8_kernel<%d,%d> split=1 bm=%d bn=%d bk=%d m_tiles=%d n_tiles=%d grid=%d", pl.nb, pl.epi, W8_BM, 64 * pl.nb, W8_BK, pl.m_tiles,
           pl.n_tiles, pl.grid);
  return 0;
}

extern "C" int pxa_gemm_w8(const pxa_gemm_w8_args* a, hipStream_t stream) {
  W8Plan pl;
  const int rc = w8_plan(a, "pxa_gemm_w8", &pl);
  if (rc) return rc;
  W8Params p;
  p.A = (const bf16_t*)a->A; p.lda = a->lda;
  p.q = (const uint8_t*)a->q; p.ldq = a->ldq;
  p.scale = a->scale;
  p.M = a->M; p.N = a->N; p.K = a->K;
  p.aux = (const bf16_t*)a->aux; p.ldaux = a->ldaux;
  p.out16 = (bf16_t*)a->out16; p.ld_out = a->ld_out;
  p.out_f32 = a->out_f32; p.ld_f32 = a->ld_f32;
  p.m_tiles = pl.m_tiles; p.n_tiles = pl.n_tiles;
  if (pl.nb == 2) w8_launch<2>(pl.epi, pl.grid, stream, p);
  else w8_launch<1>(pl.epi, pl.grid, stream, p);
  PXA_LAUNCH_CHECK();
  return 0;
}

extern "C" int pxa_fp8_quant_rows(const void* src, int src_is_f32, long ld, int N, int K, void* q, long ldq, float* scale, hipStream_t stream) {
  PXA_CHECK(src && q && scale, "pxa_fp8_quant_rows: null pointer");
  PXA_CHECK(N >= 1, "pxa_fp8_quant_rows: bad N=%d", N);
  PXA_CHECK(K >= 16 && K % 16 == 0, "pxa_fp8_quant_rows: K=%d must be a positive multiple of 16", K);
  PXA_CHECK(ld >= K && ld % 8 == 0, "pxa_fp8_quant_rows: ld=%ld must be >= K and a multiple of 8", ld);
  PXA_CHECK(ldq >= K && ldq % 16 == 0, "pxa_fp8_quant_rows: ldq=%ld must be >= K and a multiple of 16 (bytes)", ldq);
  PXA_CHECK(((uintptr_t)src | (uintptr_t)q) % 16 == 0, "pxa_fp8_quant_rows: src and q must be 16-byte aligned");
  if (src_is_f32) hipLaunchKernelGGL(fp8_quant_rows_kernel<true>, dim3(N), dim3(256), 0, stream, src, ld, K, (uint8_t*)q, ldq, scale);
  else hipLaunchKernelGGL(fp8_quant_rows_kernel<false>, dim3(N), dim3(256), 0, stream, src, ld, K, (uint8_t*)q, ldq, scale);
  PXA_LAUNCH_CHECK();
  return 0;
}

extern "C" int pxa_fp8_dequant_rows(const void* q, long ldq, const float* scale, int N, int K, void* dst, long ld, hipStream_t stream) {
  PXA_CHECK(q && scale && dst, "pxa_fp8_dequant_rows: null pointer");
  PXA_CHECK(N >= 1, "pxa_fp8_dequant_rows: bad N=%d", N);
  PXA_CHECK(K >= 16 && K % 16 == 0, "pxa_fp8_dequant_rows: K=%d must be a positive multiple of 16", K);
  PXA_CHECK(ld >= K && ld % 8 == 0, "pxa_fp8_dequant_rows: ld=%ld must be >= K and a multiple of 8", ld);
  PXA_CHECK(ldq >= K && ldq % 16 == 0, "pxa_fp8_dequant_rows: ldq=%ld must be >= K and a multiple of 16 (bytes)", ldq);
  PXA_CHECK(((uintptr_t)q | (uintptr_t)dst) % 16 == 0, "pxa_fp8_dequant_rows: q and dst must be 16-byte aligned");
  const long total = (long)N * (K / 16);
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(fp8_dequant_rows_kernel, dim3(grid), dim3(256), 0, stream, (const uint8_t*)q, ldq, scale, N, K, (bf16_t*)dst, ld);
  PXA_LAUNCH_CHECK();
  return 0;
}
