// The T5 v1.1 text encoder's own kernels (reference: diffusion/model/t5.py:87,106-111 - transformers.T5EncoderModel in bf16, last_hidden_state): the embedding
// gather, the T5LayerNorm rows and the self-attention.  The projections and the gated feed-forward are pxa_gemm calls (csrc/gemm.hip); the o and wo products add
// straight into the fp32 residual stream (out_f32 + accumulate), so no kernel here carries a residual argument.
//
// pxa_t5_attn: O[b,h] = softmax(Q K^T + bias[h][j - i] + keymask_b) V, head_dim 64, no softmax scale.  The shape is csrc/vae_attn.hip's with C = 64: a workgroup
// of 4 waves owns 64 query rows of one (sample, head), a wave 16 of them, keys stream in tiles of 32 with an online softmax; both products are written TRANSPOSED
// on v_mfma_f32_16x16x32 (layout in common.h) so that the lane which owns a score owns its query's statistics and its slice of the output:
//   S^T = K Q^T   A = K tile rows (ds_read_b128), B = the wave's Q rows (2 register fragments): lane (t = l & 15, g4 = l >> 4) gets S[query t][key 16 u + 4 g4 + j]
//   O^T = V^T P^T A = V tile read transposed (ds_read_b64_tr_b16), B = P straight from the accumulator order; lane gets O[query t][channel 16 n + 4 g4 + j], n = 0..3
// Streaming and not keys-resident, although one head's K and V would fit in LDS at L <= 512: the key loop ends at kv_len[b] (a padded caption of 20 tokens reads one
// tile, not L rows), the LDS image stays at 16 KiB + the bias window, so eight workgroups share a CU and hide each other's tile latency, and the online rescale
// touches 16 accumulator registers per lane - it is skipped wave-wide once no maximum moves.
//
// Bias.  The encoder is bidirectional, so the bucket of (query i, key j) depends on j - i alone: bias is [H][2L - 1] fp32 indexed by (j - i) + L - 1.  A workgroup
// needs the window of offsets (key 0 - its last query) .. (key L - 1 - its first query): at most L + 63 floats, staged once in LDS, already times log2 e.
//
// LDS image of a K or V tile: [32 rows][64] with plain 128-byte rows (two rows per 256-byte bank row); 16-byte chunk c of row r sits at chunk position c ^ sw(r),
// sw(r) = {0, 2, 5, 7, 4, 6, 1, 3}[(r >> 1) & 7].  Written by LDS-DMA (one 1 KiB instruction per wave and tile; the swizzle is applied to the SOURCE address) and
// double-buffered.  K rows (ds_read_b128: groups of 16 lanes mix rows {0-3, 12-15} of chunk c with rows {4-11} of chunk c ^ 1): sw over the first set is
// {0, 2, 1, 3}, over the second ^ 1 {4, 6, 5, 7}, and the row's parity picks the half of the bank row - 16 distinct 16-byte slots.  V blocks (ds_read_b64_tr_b16:
// halves of 32 lanes = 8 rows x 32 bytes): sw >> 1 over rows 0-7 and over rows 8-15 takes four values, times the row's parity - 8 distinct 32-byte slots.
// Every lane takes part in every LDS read (the transposed read needs EXEC all ones): query rows beyond L are clamped to row L - 1 of the sample at the load and not
// stored; key rows at or beyond kv_len[b] are clamped to row kv_len[b] - 1 at the load - whatever lies behind the valid keys, NaN included, is never read - and
// their scores are -inf before the maximum.  Every query row below L is computed, rows of padded positions included, as T5EncoderModel does.
#include "common.h"
#include "../../include/pixart_hip.h"

#include <cmath>

namespace {
using namespace pxa;

constexpr int T5_WAVES = 4;
constexpr int T5_BM = 16 * T5_WAVES;     // query rows of a workgroup
constexpr int T5_BN = 32;                // keys of a tile
constexpr int T5_HD = 64;                // head width
constexpr int T5_MAX_L = 512;
constexpr int T5_MAX_H = 64;
constexpr int T5_ROWB = 2 * T5_HD;       // bytes of a tile row
constexpr int T5_TILE_B = T5_BN * T5_ROWB;
constexpr int T5_STAGE_B = 2 * T5_TILE_B;  // K tile, then V tile
constexpr int T5_BIAS_N = T5_MAX_L + T5_BM + T5_BN;   // the window, and a tile of slack: a masked key's entry may be read ahead of the select

__device__ __forceinline__ int t5_sw(int r) { return (0x31647520u >> (4 * ((r >> 1) & 7))) & 7; }

// One [32][64] tile of `base` (rows row0 .. row0 + 31 of a sample, clamped to its last valid key) into the swizzled image at `lds`: one DMA instruction per wave.
__device__ __forceinline__ void t5_dma_tile(char* lds, const bf16_t* __restrict__ base, long ld, int row0, int kl, int wave, int lane) {
  const int slot = wave * 64 + lane, r = slot >> 3, c = (slot & 7) ^ t5_sw(r);
  const long gr = min(row0 + r, kl - 1);
  lds_dma16(base + gr * ld + c * 8, lds + wave * 1024);
}

__global__ __launch_bounds__(256) void t5_attn_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ldq, long ldk,
                                                      long ldv, bf16_t* __restrict__ o, long ldo, const float* __restrict__ bias, const int* __restrict__ kv_len,
                                                      int H, int L) {
  constexpr int KK = T5_HD / 32, NB = T5_HD / 16;
  __shared__ __attribute__((aligned(16))) char smem[2 * T5_STAGE_B];
  __shared__ float sbias[T5_BIAS_N];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = lane & 15, g4 = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const long row_b = (long)b * L;                                  // first row of this sample
  const int kl = min(max(kv_len[b], 1), L);                        // valid keys (the host checked 1 <= kv_len <= L; no address depends on a value outside)
  const bf16_t* kb = k + row_b * ldk + h * T5_HD;
  const bf16_t* vb = v + row_b * ldv + h * T5_HD;
  const int q0 = blockIdx.x * T5_BM, qmax = min(q0 + T5_BM - 1, L - 1);
  const int qrow = q0 + wave * 16 + t, qc = min(qrow, L - 1);

  bf16x8 qf[KK];
  {
    const bf16_t* qp = q + (row_b + qc) * ldq + h * T5_HD + g4 * 8;
#pragma unroll
    for (int kk = 0; kk < KK; kk++) qf[kk] = *reinterpret_cast<const bf16x8*>(qp + kk * 32);
  }
  t5_dma_tile(smem, kb, ldk, 0, kl, wave, lane);
  t5_dma_tile(smem + T5_TILE_B, vb, ldv, 0, kl, wave, lane);
  // bias window: entry e stands for offset (key - query) = e - qmax, e = 0 .. (kl - 1) - q0 + qmax; bias index (key - query) + L - 1 stays inside [0, 2L - 2]
  {
    const float* bh = bias + (long)h * (2 * L - 1) + (L - 1 - qmax);
    const int n_e = kl - q0 + qmax;
    for (int e = threadIdx.x; e < n_e; e += 64 * T5_WAVES) sbias[e] = bh[e] * 1.4426950408889634f;
  }
  // wait for the Q rows here: left to their first use the compiler's vmcnt, which does not count the DMA, would sit inside the tile loop
#pragma unroll
  for (int kk = 0; kk < KK; kk++) asm volatile("" : "+v"(qf[kk]));

  f32x4 acc[NB];
#pragma unroll
  for (int n = 0; n < NB; n++) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;

  int k_off[KK], v_off[NB];
  const int v_row = 4 * g4 + (t >> 2);
#pragma unroll
  for (int kk = 0; kk < KK; kk++) k_off[kk] = t * T5_ROWB + (((4 * kk + g4) ^ t5_sw(t)) << 4);
#pragma unroll
  for (int n = 0; n < NB; n++) v_off[n] = T5_TILE_B + v_row * T5_ROWB + 8 * (t & 1) + (((2 * n + ((t & 3) >> 1)) ^ t5_sw(v_row)) << 4);
  const int e0 = qmax - qc + 4 * g4;                                // window entry of (this lane's query, key 4 g4)

  const int nkt = (kl + T5_BN - 1) / T5_BN;
  for (int kt = 0; kt < nkt; kt++) {
    const char* st = smem + (kt & 1) * T5_STAGE_B;
    lds_dma_wait<0>();                                              // this wave's pieces of tile kt (nothing younger is in flight)
    __syncthreads();                                                // every wave's pieces (and, at kt = 0, the bias window); every wave is past tile kt - 1
    if (kt + 1 < nkt) {
      char* nx = smem + ((kt + 1) & 1) * T5_STAGE_B;
      t5_dma_tile(nx, kb, ldk, (kt + 1) * T5_BN, kl, wave, lane);
      t5_dma_tile(nx + T5_TILE_B, vb, ldv, (kt + 1) * T5_BN, kl, wave, lane);
    }

    // S^T = K Q^T: two 16-key blocks
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
      const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(st + k_off[kk]);
      const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(st + k_off[kk] + 16 * T5_ROWB);
      s0 = mfma16(k0, qf[kk], s0);
      s1 = mfma16(k1, qf[kk], s1);
    }

    // (score + bias) log2 e of the lane's query over its 8 keys of this tile; keys at or beyond kv_len are -inf before the maximum (and their window entry is not read)
    float s[8];
    const int key0 = kt * T5_BN + 4 * g4, eb = e0 + kt * T5_BN;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      s[j] = key0 + j < kl ? fmaf(s0[j], 1.4426950408889634f, sbias[eb + j]) : -INFINITY;
      s[4 + j] = key0 + 16 + j < kl ? fmaf(s1[j], 1.4426950408889634f, sbias[eb + 16 + j]) : -INFINITY;
    }
    float mx = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7])));
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);                               // finite: key kt * 32 of every tile is a valid key
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);          // 0 in the first tile (m = -inf)
    m = m_new;
    float p[8];
#pragma unroll
    for (int j = 0; j < 8; j++) p[j] = __builtin_amdgcn_exp2f(s[j] - m_new);
    lsum = lsum * alpha + (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])));
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 8; j++) pf[j] = f2bf(p[j]);
    if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {          // wave-uniform
#pragma unroll
      for (int n = 0; n < NB; n++) acc[n] *= alpha;
    }

    // O^T += V^T P^T: 16 channels per MFMA
#pragma unroll
    for (int n = 0; n < NB; n++) {
      const bf16x8 vf = concat_tr(lds_tr_read(st + v_off[n]), lds_tr_read(st + v_off[n] + 16 * T5_ROWB));
      acc[n] = mfma16(vf, pf, acc[n]);
    }
  }

  lsum += __shfl_xor(lsum, 16);
  lsum += __shfl_xor(lsum, 32);
  const float inv = 1.0f / lsum;                                     // lsum >= 1: the row's maximum contributes exp2(0)
  if (qrow < L) {
    bf16_t* op = o + (row_b + qrow) * ldo + h * T5_HD + 4 * g4;
#pragma unroll
    for (int n = 0; n < NB; n++)
      *reinterpret_cast<uint2*>(op + n * 16) = pack_bf16x4(acc[n][0] * inv, acc[n][1] * inv, acc[n][2] * inv, acc[n][3] * inv);
  }
}

// x[r][:] = float(table[clamp(ids[r])][:]): one workgroup per row, 8 elements per thread and step.
__global__ __launch_bounds__(256) void t5_embed_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ table, float* __restrict__ x, int D, int vocab) {
  const long r = blockIdx.x;
  const int id = min(max(ids[r], 0), vocab - 1);
  const bf16_t* src = table + (long)id * D;
  float* dst = x + r * D;
  for (int c = threadIdx.x * 8; c < D; c += 256 * 8) {
    float f[8];
    unpack_bf16x8(*reinterpret_cast<const uint4*>(src + c), f);
    *reinterpret_cast<float4*>(dst + c) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(dst + c + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}

// T5LayerNorm: y = x / sqrt(mean(x^2) + eps) * w.  One workgroup per row; the second sweep re-reads the row (16 KiB at D = 4096: it is in L2).
__global__ __launch_bounds__(256) void t5_rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w, bf16_t* __restrict__ y_bf16,
                                                         float* __restrict__ y_f32, int D, float eps) {
  __shared__ float part[4];
  const long r = blockIdx.x;
  const float* xr = x + r * D;
  float ss = 0.f;
  for (int c = threadIdx.x * 4; c < D; c += 256 * 4) {
    const float4 a = *reinterpret_cast<const float4*>(xr + c);
    ss += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float tot = (part[0] + part[1]) + (part[2] + part[3]);
  const float rs = 1.0f / sqrtf(tot / (float)D + eps);
  for (int c = threadIdx.x * 4; c < D; c += 256 * 4) {
    const float4 a = *reinterpret_cast<const float4*>(xr + c);
    const float4 g = *reinterpret_cast<const float4*>(w + c);
    const float4 y = make_float4(a.x * rs * g.x, a.y * rs * g.y, a.z * rs * g.z, a.w * rs * g.w);
    if (y_bf16) *reinterpret_cast<uint2*>(y_bf16 + r * D + c) = pack_bf16x4(y.x, y.y, y.z, y.w);
    if (y_f32) *reinterpret_cast<float4*>(y_f32 + r * D + c) = y;
  }
}
}  // namespace

extern "C" int pxa_t5_embed(const int* ids, const void* table, float* x, int R, int D, int vocab, hipStream_t stream) {
  PXA_CHECK(ids && table && x, "pxa_t5_embed: null pointer");
  PXA_CHECK(R >= 1 && vocab >= 1, "pxa_t5_embed: bad R=%d / vocab=%d", R, vocab);
  PXA_CHECK(D >= 8 && D % 8 == 0, "pxa_t5_embed: D=%d must be a positive multiple of 8", D);
  PXA_CHECK(((uintptr_t)table | (uintptr_t)x) % 16 == 0, "pxa_t5_embed: table and x must be 16-byte aligned");
  hipLaunchKernelGGL(t5_embed_kernel, dim3(R), dim3(256), 0, stream, ids, (const bf16_t*)table, x, D, vocab);
  PXA_LAUNCH_CHECK();
  return 0;
}

extern "C" int pxa_t5_rmsnorm(const float* x, const float* w, void* y_bf16, float* y_f32, int R, int D, float eps, hipStream_t stream) {
  PXA_CHECK(x && w, "pxa_t5_rmsnorm: null pointer (x, w)");
  PXA_CHECK(y_bf16 || y_f32, "pxa_t5_rmsnorm: null pointer (both outputs)");
  PXA_CHECK(R >= 1, "pxa_t5_rmsnorm: bad R=%d", R);
  PXA_CHECK(D >= 8 && D % 8 == 0, "pxa_t5_rmsnorm: D=%d must be a positive multiple of 8", D);
  PXA_CHECK(eps > 0.f && eps < 1.f, "pxa_t5_rmsnorm: eps=%g out of range", (double)eps);
  PXA_CHECK(((uintptr_t)x | (uintptr_t)w | (uintptr_t)y_bf16 | (uintptr_t)y_f32) % 16 == 0, "pxa_t5_rmsnorm: x, w, y must be 16-byte aligned");
  hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3(R), dim3(256), 0, stream, x, w, (bf16_t*)y_bf16, y_f32, D, eps);
  PXA_LAUNCH_CHECK();
  return 0;
}

extern "C" int pxa_t5_attn(const pxa_t5_attn_args* a, hipStream_t stream) {
  PXA_CHECK(a, "pxa_t5_attn: null pointer (args)");
  PXA_CHECK(a->q && a->k && a->v && a->o && a->bias && a->kv_len, "pxa_t5_attn: null pointer");
  PXA_CHECK(a->head_dim == T5_HD, "pxa_t5_attn: head_dim=%d is not built (64)", a->head_dim);
  PXA_CHECK(a->L >= 1 && a->L <= T5_MAX_L, "pxa_t5_attn: L=%d out of range (1 .. %d)", a->L, T5_MAX_L);
  PXA_CHECK(a->H >= 1 && a->H <= T5_MAX_H, "pxa_t5_attn: H=%d out of range (1 .. %d)", a->H, T5_MAX_H);
  PXA_CHECK(a->B >= 1 && a->B <= 65535, "pxa_t5_attn: B=%d out of range (1 .. 65535)", a->B);
  const long width = (long)a->H * T5_HD;
  PXA_CHECK(a->ldq >= width && a->ldk >= width && a->ldv >= width && a->ldo >= width, "pxa_t5_attn: row strides ld (%ld, %ld, %ld, %ld) must be >= H*64=%ld",
            a->ldq, a->ldk, a->ldv, a->ldo, width);
  PXA_CHECK(a->ldq % 8 == 0 && a->ldk % 8 == 0 && a->ldv % 8 == 0 && a->ldo % 8 == 0, "pxa_t5_attn: row strides ld (%ld, %ld, %ld, %ld) must be multiples of 8",
            a->ldq, a->ldk, a->ldv, a->ldo);
  PXA_CHECK(((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o) % 16 == 0, "pxa_t5_attn: q, k, v, o must be 16-byte aligned");
  hipLaunchKernelGGL(t5_attn_kernel, dim3((a->L + T5_BM - 1) / T5_BM, a->H, a->B), dim3(64 * T5_WAVES), 0, stream, (const bf16_t*)a->q, (const bf16_t*)a->k,
                     (const bf16_t*)a->v, a->ldq, a->ldk, a->ldv, (bf16_t*)a->o, a->ldo, a->bias, a->kv_len, a->H, a->L);
  PXA_LAUNCH_CHECK();
  return 0;
}
