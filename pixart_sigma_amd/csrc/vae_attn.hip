// Mid-block attention of the SDXL-VAE / SD-VAE (diffusers AutoencoderKL: encoder.mid_block.attentions[0], decoder.mid_block.attentions[0]) as ONE streaming
// launch: O[b] = softmax(scale * Q[b] K[b]^T) V[b] for B images of HW tokens, one head of width C (512, or 256 in the small test configs).  Call site of the
// whole decode in the reference: scripts/inference.py:136 (diffusers routes this attention through SDPA).  It replaces, per image, the fp32 HW x HW score GEMM,
// pxa_vae_softmax_rows and the P V GEMM of AutoencoderKL._attention: no score or probability matrix exists, no scratch, no allocation.
//
// Shape.  A workgroup of 4 waves owns 64 query rows, a wave 16 of them; keys come in tiles of 32.  Both products are written TRANSPOSED so that the lane which
// owns a score also owns the softmax statistics of its query and the matching slice of the output (v_mfma_f32_16x16x32, layout in common.h):
//   S^T = K Q^T   A = K tile rows (ds_read_b128), B = the wave's Q rows (registers for the whole kernel: C/32 fragments of 8 elements)
//                 lane (t = l & 15, g4 = l >> 4) gets S[query t][key 16 u + 4 g4 + j], u = 0..1, j = 0..3
//   O^T = V^T P^T A = V tile read transposed (ds_read_b64_tr_b16), B = P: the MFMA's reduction index k = 8 g4 + j' stands for key 16 (j' >> 2) + 4 g4 + (j' & 3),
//                 which is exactly the order the lane's eight scores are already in - P goes from the accumulator to the operand without leaving the lane
//                 lane gets O[query t][channel 16 n + 4 g4 + j]: C/16 accumulators of 4 = 128 registers at C = 512
// Row maximum: 8 values in the lane, then lanes t, t+16, t+32, t+48 (two xor-shuffles).  The row sum stays a per-lane partial (every lane of a query scales it by
// the same factor) and is folded once at the end.  Scores and statistics are fp32 (exp2 with scale * log2 e folded in), P is rounded to the operand type in
// front of its MFMA, O is accumulated in fp32, divided by the fp32 row sum and rounded once at the store.
//
// LDS image.  A K or V tile is [32 rows][C] with plain 2C-byte rows; 16-byte chunk c of row r sits at chunk position c ^ (2 (r & 7)).  It is written by LDS-DMA
// (the swizzle is applied to the SOURCE address: a DMA instruction writes 1 KiB linearly) and double-buffered: 2 x (K + V) = 128 KiB at C = 512, 64 KiB at 256.
//   K rows (ds_read_b128, groups of 16 lanes that mix rows {0-3, 12-15} of one g4 with rows {4-11} of g4 ^ 1): positions (4 kk + g4) ^ 2 (r & 7) - the eight rows
//   of one g4 take the eight even or the eight odd positions of a 256-byte bank row, the other g4 the other parity: 16 distinct 16-byte slots, conflict-free.
//   V blocks (ds_read_b64_tr_b16, halves of 32 lanes = 8 rows x 32 bytes): a row's chunk pair (2 n, 2 n + 1) moves to (2 (n ^ (r & 7)), + 1) - eight distinct
//   32-byte slots of the 256-byte bank row, conflict-free.
// Every lane takes part in every LDS read (the transposed read needs EXEC all ones): rows and keys beyond HW are CLAMPED to the image's last row at the load
// - no address at or beyond row B * HW is formed - tail keys are set to -inf before the maximum, tail query rows are not stored.
#include "common.h"
#include "../../include/pixart_hip.h"

#include <cmath>

namespace {
using namespace pxa;

constexpr int VA_WAVES = 4;
constexpr int VA_BM = 16 * VA_WAVES;   // query rows of a workgroup
constexpr int VA_BN = 32;              // keys of a tile

template <int C> struct VaGeom {
  static constexpr int CH = C / 8;                            // 16-byte chunks of a row
  static constexpr int ROWB = 2 * C;                          // bytes of a tile row
  static constexpr int TILE_B = VA_BN * ROWB;                 // one K or one V tile
  static constexpr int STAGE_B = 2 * TILE_B;                  // K tile, then V tile
  static constexpr int LDS_B = 2 * STAGE_B;                   // two stages
  static constexpr int NDMA = TILE_B / (VA_WAVES * 1024);     // DMA instructions per wave and tile: 8 (C = 512), 4 (C = 256)
};

// One [32][C] tile of `base` (rows row0 .. row0 + 31 of an image of HW rows, clamped to its last row) into the swizzled image at `lds`.
template <int C>
__device__ __forceinline__ void va_dma_tile(char* lds, const bf16_t* __restrict__ base, long ld, int row0, int HW, int wave, int lane) {
  using G = VaGeom<C>;
#pragma unroll
  for (int i = 0; i < G::NDMA; i++) {
    const int slot = (i * VA_WAVES + wave) * 64 + lane, r = slot / G::CH, pos = slot % G::CH;
    const int c = pos ^ (2 * (r & 7));
    const long gr = min(row0 + r, HW - 1);
    lds_dma16(base + gr * ld + c * 8, lds + (i * VA_WAVES + wave) * 1024);
  }
}

template <int C>
__global__ __launch_bounds__(256) void vae_attn_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, long ldq,
                                                       long ldk, long ldv, bf16_t* __restrict__ o, long ldo, int HW, float scale_log2e) {
  using G = VaGeom<C>;
  constexpr int KK = C / 32, NB = C / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = lane & 15, g4 = lane >> 4;
  const long img = (long)blockIdx.y * HW;                       // first row of this image
  const bf16_t* kb = k + img * ldk;
  const bf16_t* vb = v + img * ldv;
  const int qrow = blockIdx.x * VA_BM + wave * 16 + t;

  bf16x8 qf[KK];
  {
    const bf16_t* qp = q + (img + min(qrow, HW - 1)) * ldq + g4 * 8;
#pragma unroll
    for (int kk = 0; kk < KK; kk++) qf[kk] = *reinterpret_cast<const bf16x8*>(qp + kk * 32);
  }
  va_dma_tile<C>(smem, kb, ldk, 0, HW, wave, lane);
  va_dma_tile<C>(smem + G::TILE_B, vb, ldv, 0, HW, wave, lane);
  // wait for the Q rows here: left to their first use the compiler's vmcnt, which does not count the DMA, would sit inside the tile loop
#pragma unroll
  for (int kk = 0; kk < KK; kk++) asm volatile("" : "+v"(qf[kk]));

  f32x4 acc[NB];
#pragma unroll
  for (int n = 0; n < NB; n++) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;

  // per-lane LDS offsets (see the image above).  The swizzle touches chunk bits 1..3 only, so the C/32 K reads need 4 distinct lane offsets and the C/16 V reads 8:
  // everything else is an immediate (256 bytes per 4 K steps / 8 channel blocks).
  const int k_sw = g4 ^ (2 * (t & 7));
  const int v_row = 4 * g4 + (t >> 2), v_sw = ((t & 3) >> 1) ^ (2 * (v_row & 7));
  int k_off[4], v_off[8];
#pragma unroll
  for (int j = 0; j < 4; j++) k_off[j] = t * G::ROWB + (((4 * j) ^ k_sw) << 4);
#pragma unroll
  for (int j = 0; j < 8; j++) v_off[j] = G::TILE_B + v_row * G::ROWB + 8 * (t & 1) + (((2 * j) ^ v_sw) << 4);

  const int nkt = (HW + VA_BN - 1) / VA_BN;
  for (int kt = 0; kt < nkt; kt++) {
    const char* st = smem + (kt & 1) * G::STAGE_B;
    lds_dma_wait<0>();                                          // this wave's pieces of tile kt (nothing younger is in flight)
    __syncthreads();                                            // every wave's pieces; and every wave is past tile kt - 1, whose stage is refilled now
    if (kt + 1 < nkt) {
      char* nx = smem + ((kt + 1) & 1) * G::STAGE_B;
      va_dma_tile<C>(nx, kb, ldk, (kt + 1) * VA_BN, HW, wave, lane);
      va_dma_tile<C>(nx + G::TILE_B, vb, ldv, (kt + 1) * VA_BN, HW, wave, lane);
    }

    // S^T = K Q^T: two 16-key blocks
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
      const int off = k_off[kk & 3] + (kk >> 2) * 256;
      const bf16x8 k0 = *reinterpret_cast<const bf16x8*>(st + off);
      const bf16x8 k1 = *reinterpret_cast<const bf16x8*>(st + off + 16 * G::ROWB);
      s0 = mfma16(k0, qf[kk], s0);
      s1 = mfma16(k1, qf[kk], s1);
    }

    // online softmax of the lane's query over its 8 keys of this tile; keys beyond HW are -inf before the maximum
    float s[8];
    const int key0 = kt * VA_BN + 4 * g4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      s[j] = key0 + j < HW ? s0[j] * scale_log2e : -INFINITY;
      s[4 + j] = key0 + 16 + j < HW ? s1[j] * scale_log2e : -INFINITY;
    }
    float mx = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7])));
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m, mx);                           // finite: key kt * 32 of every tile is inside the image
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);      // 0 in the first tile (m = -inf)
    m = m_new;
    float p[8];
#pragma unroll
    for (int j = 0; j < 8; j++) p[j] = __builtin_amdgcn_exp2f(s[j] - m_new);
    lsum = lsum * alpha + (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])));
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 8; j++) pf[j] = f2bf(p[j]);
    if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {      // wave-uniform: once no maximum of the 16 rows moves, the 128 multiplies go
#pragma unroll
      for (int n = 0; n < NB; n++) acc[n] *= alpha;
    }

    // O^T += V^T P^T: 16 channels per MFMA
#pragma unroll
    for (int n = 0; n < NB; n++) {
      const int off = v_off[n & 7] + (n >> 3) * 256;
      const bf16x8 vf = concat_tr(lds_tr_read(st + off), lds_tr_read(st + off + 16 * G::ROWB));
      acc[n] = mfma16(vf, pf, acc[n]);
    }
  }

  lsum += __shfl_xor(lsum, 16);
  lsum += __shfl_xor(lsum, 32);
  const float inv = 1.0f / lsum;                                 // >= 1: the row's maximum contributes exp2(0)
  if (qrow < HW) {
    bf16_t* op = o + (img + qrow) * ldo + 4 * g4;
#pragma unroll
    for (int n = 0; n < NB; n++)
      *reinterpret_cast<uint2*>(op + n * 16) = pack_bf16x4(acc[n][0] * inv, acc[n][1] * inv, acc[n][2] * inv, acc[n][3] * inv);
  }
}

template <int C>
int va_launch(const void* q, const void* k, const void* v, long ldq, long ldk, long ldv, void* o, long ldo, int B, int HW, float scale, hipStream_t stream) {
  using G = VaGeom<C>;
  const hipError_t e = lds_optin(reinterpret_cast<const void*>(vae_attn_kernel<C>), G::LDS_B);
  if (e != hipSuccess) { pxa_set_error("hipFuncSetAttribute(vae_attn<%d>, %d): %s", C, G::LDS_B, hipGetErrorString(e)); return -3; }
  hipLaunchKernelGGL(vae_attn_kernel<C>, dim3((HW + VA_BM - 1) / VA_BM, B), dim3(64 * VA_WAVES), G::LDS_B, stream, (const bf16_t*)q, (const bf16_t*)k,
                     (const bf16_t*)v, ldq, ldk, ldv, (bf16_t*)o, ldo, HW, scale * 1.4426950408889634f);
  PXA_LAUNCH_CHECK();
  return 0;
}
}  // namespace

extern "C" int pxa_vae_attn(const void* q, const void* k, const void* v, long ldq, long ldk, long ldv, void* o, long ldo, int B, int HW, int C, float scale,
                            hipStream_t stream) {
  PXA_CHECK(q && k && v && o, "pxa_vae_attn: null pointer");
  PXA_CHECK(C == 512 || C == 256, "pxa_vae_attn: C=%d is not built (512 or 256)", C);
  PXA_CHECK(B >= 1 && B <= 65535 && HW >= 1, "pxa_vae_attn: bad B=%d / HW=%d", B, HW);
  PXA_CHECK(ldq >= C && ldk >= C && ldv >= C && ldo >= C, "pxa_vae_attn: row strides (%ld, %ld, %ld, %ld) must be >= C=%d", ldq, ldk, ldv, ldo, C);
  PXA_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "pxa_vae_attn: row strides (%ld, %ld, %ld, %ld) must be multiples of 8 (16-byte accesses)",
            ldq, ldk, ldv, ldo);
  PXA_CHECK(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 == 0, "pxa_vae_attn: q, k, v, o must be 16-byte aligned");
  PXA_CHECK(std::isfinite(scale), "pxa_vae_attn: scale is not finite");
  return C == 512 ? va_launch<512>(q, k, v, ldq, ldk, ldv, o, ldo, B, HW, scale, stream) : va_launch<256>(q, k, v, ldq, ldk, ldv, o, ldo, B, HW, scale, stream);
}
