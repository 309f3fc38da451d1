// Attention kernels that NO default call reaches (a part of attn.hip's translation unit: included there behind the helpers, knobs and launcher enums it uses; not a header of its own).  Each runs only where an environment
// variable, a missing workspace or an A/B build asks for it; what selects it and what keeps it in the tree:
//   attn_bwd_dq_kernel     round-2 dQ kernel (compiler-scheduled).  PXA_ATTN_DQ=0, or a build with -DATTN_FOLD_DELTA=0 (the kernels that replaced it
//                          need the delta fold).  Kept by: the mode-matrix tests (tests/test_kernels_gpu.py, PXA_ATTN_DQ=0 as the A/B partner of dq2 / dq4).
//   attn_bwd_dkv_kernel    round-2 dK/dV kernel (lse / delta on the VALU).  PXA_ATTN_DKV=0, or a caller that passes no bwd_stats workspace: the ABI promise
//                          of pxa_attn_bwd (include/pixart_hip.h).  Kept by: that promise, test_attention_dkv_kernel_modes, and
//                          test_attention_full_grid_b16, which uses it as the independent cross-check of the default kernels.
//   attn_bwd_dkv3_kernel   dK/dV as a phase ping-pong of two waves per SIMD.  PXA_ATTN_DKV=3.  Measured no faster than dkv2 (comment at the kernel);
//                          kept for the record and by test_attention_dkv_kernel_modes.
//   attn_bwd_dkv5_kernel   attn_bwd_dkv4_kernel with the second products on 16-row MFMAs.  PXA_ATTN_DKV=5.  Faster alone, slower inside the training step
//                          (the rule in attn.hip choose_dkv): an open measurement question.  Kept by: test_attention_dkv_kernel_modes and the static ISA
//                          tests (tests/test_isa_static.py).
// (attn_bwd_dkv2_kernel<0>, PXA_ATTN_DKV=1, is the fifth such kernel: an instance stays with its template in attn.hip.)
// A later decision on any of them is a change to this file and to the cases of attn.hip that name it.
namespace {
// ------------------------------------------------------------------------------------------------ backward: dQ (round 2)
__global__ __launch_bounds__(256, ATTN_BWD_WAVES) void attn_bwd_dq_kernel(AttnParams p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_B];   // 2 stages x {K, V}
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hi = lane >> 5;
  int bx, h, b;
  block_coords(p, bx, h, b);
  const int q = bx * 128 + wave * 32 + (lane & 31);
  const bool qvalid = q < p.Nq;
  long kbase, vbase, d0_, d1_; int kvlen;
  kv_range(p, b, kbase, vbase, d0_, d1_, kvlen);
  const bf16_t* Kp = p.K + kbase + (long)h * p.k_hs;
  const bf16_t* Vp = p.V + vbase + (long)h * p.v_hs;
  const int kts = (int)p.k_ts, vts = (int)p.v_ts;

  bf16x8 qf[KSTEPS], dof[KSTEPS];
  load_row_frags(qf, p.Q + (long)b * p.q_bs + (long)q * p.q_ts + (long)h * p.q_hs, qvalid, hi);
  load_row_frags(dof, p.dO + (long)b * p.o_bs + (long)q * p.o_ts + (long)h * p.o_hs, qvalid, hi);
  settle(qf);
  settle(dof);
  const long sidx = ((long)b * p.H + h) * p.Nq + q;
  const float lse = qvalid ? p.LSE[sidx] : 0.f;
  const float delta = qvalid ? p.Delta[sidx] : 0.f;
  if (ATTN_FOLD_DELTA && hi == 1) {                             // slots 72 .. 74 of this lane's dO row (k-step 4, upper half: d = 72 .. 79)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 w = __builtin_bit_cast(u32x4, dof[KSTEPS - 1]);
    const uint2 d3 = split3(delta);
    w[0] = d3.x; w[1] = d3.y;
    dof[KSTEPS - 1] = __builtin_bit_cast(bf16x8, w);
  }
  DmaPlan pl;
  dma_plan(pl, wave, lane);
  FragAddr fa;
  frag_addr(fa, lane);

  for (int st = 0; st < 4; st++) init_pads(smem + st * TILE_B, (ATTN_FOLD_DELTA && (st & 1)) ? 2 : 0, tid);   // odd tiles = V: -1.0 in slots 72 .. 74
  Acc16 dq;
  zero16(dq);
  Tr16Addr ta;
  tr16_addr(ta, lane);
  const float c = p.scale_log2;
  auto tile = [&](auto tailc, const char* sK, const char* sV, int kv0) {
    constexpr bool TAIL = decltype(tailc)::value;
    f32x16 s[2], dp[2];
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
#pragma unroll
      for (int g = 0; g < 16; g++) { s[sub][g] = 0.f; dp[sub][g] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ks++) {
        s[sub] = mfma32(rowfrag(sK, fa, sub, ks), qf[ks], s[sub]);
        dp[sub] = mfma32(rowfrag(sV, fa, sub, ks), dof[ks], dp[sub]);
      }
    }
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int g = 0; g < 16; g++) {
        float pr = __builtin_amdgcn_exp2f(s[sub][g] * c - lse);
        if (TAIL && kv0 + sub * 32 + (g & 3) + 8 * (g >> 2) + 4 * hi >= kvlen) pr = 0.f;
        s[sub][g] = ATTN_FOLD_DELTA ? pr * dp[sub][g] : pr * (dp[sub][g] - delta);  // dS^T (without the softmax scale, applied at the end)
      }
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      bf16x8 dx, dy;
      pack_xy(s[sub], dx, dy);
      mma16(dq, sK, ta, sub, dx, dy);
    }
  };
  const int Tfull = kvlen / BKV, rem = kvlen - Tfull * BKV, T = Tfull + (rem ? 1 : 0);
  auto issue = [&](int t) {                // DMA of tile t into stage t&1
    char* nx = smem + (t & 1) * 2 * TILE_B;
    if (t < Tfull) {
      dma_tile<true>(nx, Kp, kts, t * BKV, kvlen, pl, wave);
      dma_tile<true>(nx + TILE_B, Vp, vts, t * BKV, kvlen, pl, wave);
    } else {
      dma_tile<false>(nx, Kp, kts, t * BKV, kvlen, pl, wave);
      dma_tile<false>(nx + TILE_B, Vp, vts, t * BKV, kvlen, pl, wave);
    }
  };
  if (T > 0) issue(0);
  for (int t = 0; t < Tfull; t++) {
    tile_sync();                           // own DMA drained (vmcnt(0)) + stage hand-over; ONE barrier per tile
    if (t + 1 < T) issue(t + 1);
    const char* st = smem + (t & 1) * 2 * TILE_B;
    tile(BoolC<false>{}, st, st + TILE_B, t * BKV);
  }
  if (rem) {                               // ragged last tile: the only place that pays for masking
    tile_sync();
    const char* st = smem + (Tfull & 1) * 2 * TILE_B;
    tile(BoolC<true>{}, st, st + TILE_B, Tfull * BKV);
  }
  const int q0w = bx * 128 + wave * 32;
  const bool ok0 = q0w + (lane & 15) < p.Nq, ok1 = q0w + 16 + (lane & 15) < p.Nq;
  store_rows16(p.dQ + (long)b * p.dq_bs + (long)q0w * p.dq_ts + (long)h * p.dq_hs, p.dq_ts, dq, p.scale, p.scale, ok0, ok1, lane);
  if (p.dq_colsum) colsum_rows16(p.dq_colsum + (b % PXA_COLSUM_SLOTS) * p.colsum_stride + h * DH, dq, p.scale, ok0, ok1, lane);
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
__global__ __launch_bounds__(256, ATTN_BWD_WAVES) void attn_bwd_dkv_kernel(AttnParams p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_B + 4 * BKV * 4];   // 2 stages x {Q, dO} + 2 stages x {lse, delta}
  float* ldsL = reinterpret_cast<float*>(smem + 4 * TILE_B);                      // [2][2][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hi = lane >> 5;
  int bx, h, b;
  block_coords(p, bx, h, b);
  long kbase, vbase, dkbase, dvbase; int kvlen;
  kv_range(p, b, kbase, vbase, dkbase, dvbase, kvlen);
  if (bx * 128 >= kvlen) return;  // whole block beyond this sample's keys (uniform across the block)
  const int kv = bx * 128 + wave * 32 + (lane & 31);
  const bool kvvalid = kv < kvlen;
  // A wave whose 32 keys all lie beyond the sample's length (text keys: 300 = 128 + 128 + 32 + 12) still serves the block's LDS-DMA and
  // barriers but issues no MFMA / softmax work: the matrix pipe of its SIMD is left to the co-resident workgroup's wave.
  const bool wave_active = bx * 128 + wave * 32 < kvlen;

  bf16x8 kf[KSTEPS], vf[KSTEPS];
  load_row_frags(kf, p.K + kbase + (long)kv * p.k_ts + (long)h * p.k_hs, kvvalid, hi);
  load_row_frags(vf, p.V + vbase + (long)kv * p.v_ts + (long)h * p.v_hs, kvvalid, hi);
  settle(kf);
  settle(vf);
  const bf16_t* Qp = p.Q + (long)b * p.q_bs + (long)h * p.q_hs;
  const bf16_t* Dp = p.dO + (long)b * p.o_bs + (long)h * p.o_hs;
  const float* Lp = p.LSE + ((long)b * p.H + h) * p.Nq;
  const float* Dl = p.Delta + ((long)b * p.H + h) * p.Nq;
  const int qts = (int)p.q_ts, ots = (int)p.o_ts;
  DmaPlan pl;
  dma_plan(pl, wave, lane);
  FragAddr fa;
  frag_addr(fa, lane);

  for (int st = 0; st < 4; st++) init_pads(smem + st * TILE_B, 0, tid);
  f32x16 dk[3], dv[3];
  zero3(dk);
  zero3(dv);
  const float c = p.scale_log2;
  const int T = (p.Nq + BKV - 1) / BKV;
  float rl = INFINITY, rdl = 0.f;
  auto fetch_stats = [&](int q0) {
    if (tid < BKV) {
      const bool ok = q0 + tid < p.Nq;
      rl = ok ? Lp[q0 + tid] : INFINITY;    // +inf -> P = exp2(-inf) = 0 for rows beyond Nq
      rdl = ok ? Dl[q0 + tid] : 0.f;
    }
  };
  const int Tfull = p.Nq / BKV;
  auto issue = [&](int t) {
    char* nx = smem + (t & 1) * 2 * TILE_B;
    if (t < Tfull) {
      dma_tile<true>(nx, Qp, qts, t * BKV, p.Nq, pl, wave);
      dma_tile<true>(nx + TILE_B, Dp, ots, t * BKV, p.Nq, pl, wave);
    } else {
      dma_tile<false>(nx, Qp, qts, t * BKV, p.Nq, pl, wave);
      dma_tile<false>(nx + TILE_B, Dp, ots, t * BKV, p.Nq, pl, wave);
    }
    fetch_stats(t * BKV);
  };
  issue(0);
  for (int t = 0; t < T; t++) {
    const char* sQ = smem + (t & 1) * 2 * TILE_B;
    const char* sD = sQ + TILE_B;
    float* sL = ldsL + (t & 1) * 2 * BKV;
    if (tid < BKV) { sL[tid] = rl; sL[BKV + tid] = rdl; }   // buffer (t&1) was last read two iterations ago
    tile_sync();
    if (!(ATTN_ABL & 16) && t + 1 < T) issue(t + 1);
    if (!wave_active) continue;
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      f32x16 s, dp;
#pragma unroll
      for (int g = 0; g < 16; g++) { s[g] = 0.f; dp[g] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ks++) {
        const bf16x8 qa = (ATTN_ABL & 8) ? vf[(ks + sub) % KSTEPS] : rowfrag(sQ, fa, sub, ks);
        const bf16x8 da = (ATTN_ABL & 8) ? kf[(ks + sub) % KSTEPS] : rowfrag(sD, fa, sub, ks);
        if (ATTN_ABL & 4) {
          s[ks] += (float)qa[0] + (float)kf[ks][1];
          dp[ks] += (float)da[0] + (float)vf[ks][1];
        } else {
          s = mfma32(qa, kf[ks], s);    // S[q][kv], col = kv (lane), rows = q
          dp = mfma32(da, vf[ks], dp);  // dP[q][kv]
        }
      }
#pragma unroll
      for (int qd = 0; qd < 4; qd++) {
        const int ql = sub * 32 + 8 * qd + 4 * hi;
        const float4 L4 = *reinterpret_cast<const float4*>(&sL[ql]);
        const float4 D4 = *reinterpret_cast<const float4*>(&sL[BKV + ql]);
        const float Lv[4] = {L4.x, L4.y, L4.z, L4.w}, Dv[4] = {D4.x, D4.y, D4.z, D4.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          if (ATTN_ABL & 1) continue;        // ablation: no softmax arithmetic (packs S, dP as they are)
          const float pr = __builtin_amdgcn_exp2f(s[qd * 4 + e] * c - Lv[e]);
          s[qd * 4 + e] = pr;
          dp[qd * 4 + e] = pr * (dp[qd * 4 + e] - Dv[e]);
        }
      }
#pragma unroll
      for (int uu = 0; uu < 2; uu++) {
        const bf16x8 pb = pack8(s, 8 * uu), db = pack8(dp, 8 * uu);
        const int u = sub * 2 + uu;
#pragma unroll
        for (int dt = 0; dt < 3; dt++) {
          const bf16x8 dot = (ATTN_ABL & 8) ? kf[dt + uu] : trfrag(sD, fa, dt, u);
          const bf16x8 qt = (ATTN_ABL & 8) ? vf[dt + uu] : trfrag(sQ, fa, dt, u);
          if (ATTN_ABL & 2) {
            dv[dt][u] += (float)dot[0] * (float)pb[dt];
            dk[dt][u] += (float)qt[0] * (float)db[dt];
          } else {
            dv[dt] = mfma32(dot, pb, dv[dt]);
            dk[dt] = mfma32(qt, db, dk[dt]);
          }
        }
      }
    }
  }
  if (kvvalid) {
    store_rows(p.dK + dkbase + (long)kv * p.dk_ts + (long)h * p.dk_hs, dk, p.dk_scale, hi);
    store_rows(p.dV + dvbase + (long)kv * p.dv_ts + (long)h * p.dv_hs, dv, 1.f, hi);
  }
  if (p.dk_colsum) colsum_rows(p.dk_colsum + (b % PXA_COLSUM_SLOTS) * p.colsum_stride + h * DH, dk, p.dk_scale, kvvalid, hi, lane);
  if (p.dv_colsum) colsum_rows(p.dv_colsum + (b % PXA_COLSUM_SLOTS) * p.colsum_stride + h * DH, dv, 1.f, kvvalid, hi, lane);
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV as a phase ping-pong (round 3, second form)
// What the hand-placed kernel above could not fix: its two waves per SIMD come from different workgroups, are in-order and uncoordinated - each blocks
// on the matrix pipe while the partner's MFMA runs and cannot issue its softmax meanwhile (47 cycles per MFMA against a 32-cycle floor).  Here ONE
// 512-thread workgroup (256 keys) owns the CU: waves w and w + 4 share a SIMD and alternate, in lock-step through s_barrier, between
//     phase M: C(j) + A(j+1) - 22 MFMAs with their LDS reads, no VALU        and        phase V: B(j+1) - the softmax, no MFMA
// with waves 4-7 one phase behind waves 0-3, so on every SIMD one wave is in M while the other is in V: the MFMAs of the two never collide and the
// softmax sits entirely in the partner's matrix phase (the persistent GEMM's two-phase scheme, csrc/gemm.hip).  S / dP are updated in place (B(j) is
// complete before A(j+1) issues), one packed P / dS set.  The Q / dO tiles are shared by 8 waves (half the LDS-DMA traffic per key).
//   per wave and tile t:  V: B(2t) | M: C(2t), A(2t+1) | V: B(2t+1) | M: C(2t+1), A(2t+2)      four barriers; group 1 (waves 4-7) runs one phase later
// MEASURED (profiles/r03o_attn_dkv_modes.txt, r03p_dkv3_depth.txt): parity green on the first run, bit-reproducible on all 256 heads at B = 16 - and
// 2.56 ms against 2.51 ms for the kernel above: no faster.  Nor does the prefetch distance of its matrix phase matter (2 / 3 / 4 / 6 fragments:
// 2.666 / 2.666 / 2.682 / 2.691 ms on one box).  Two uncoordinated waves, a hand-placed pipeline and a lock-step ping-pong all land within 3 % of each
// other: the kernel is not waiting for issue slots or LDS latency, it sits at the chip's POWER limit for this instruction mix (effective clock 1.75 GHz,
// DESIGN.md section 4 fact 2) - what moved the time this round was removing work (the stats rows: -6 %), not re-ordering it.  Kept as PXA_ATTN_DKV=3 for
// the record; mode 2 stays the default.
//   ring: tile t+2 -> stage (t+2) % 3 is issued at global phase 4t+1 (group 0: start of its first M, group 1: start of its first V - every wave has left
//   tile t-1 by then) and waited for (vmcnt(0), each wave its own pieces) in front of the barrier that ends global phase 4t+6, one phase before group 0
//   first reads it.
template <int DK>     // DK = prefetch distance of the matrix phase in fragments (DK + 1 fragment register quads)
__global__ __launch_bounds__(512, 2) void attn_bwd_dkv3_kernel(AttnParams p) {
  constexpr int NF = DK + 1;
  __shared__ __attribute__((aligned(16))) char smem[NSTAGE * STAGE_B];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hi = lane >> 5;
  const int grp = wave >> 2;
  int bx, h, b;
  block_coords(p, bx, h, b);
  long kbase, vbase, dkbase, dvbase; int kvlen;
  kv_range(p, b, kbase, vbase, dkbase, dvbase, kvlen);
  if (bx * 256 >= kvlen) return;  // whole block beyond this sample's keys (uniform across the block)
  const int kv = bx * 256 + wave * 32 + (lane & 31);
  const bool kvvalid = kv < kvlen;
  const bool wave_active = bx * 256 + wave * 32 < kvlen;

  bf16x8 kf[KSTEPS], vf[KSTEPS];
  load_row_frags(kf, p.K + kbase + (long)kv * p.k_ts + (long)h * p.k_hs, kvvalid, hi);
  load_row_frags(vf, p.V + vbase + (long)kv * p.v_ts + (long)h * p.v_hs, kvvalid, hi);
  settle(kf);
  settle(vf);
  if (hi == 1) {                                            // k-slots 72 .. 74: -1.0 against the stats rows' {hi, mid, lo}
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 w = __builtin_bit_cast(u32x4, kf[KSTEPS - 1]);
    w[0] = PXA_OPERAND_MINUS_ONE_X2; w[1] = PXA_OPERAND_MINUS_ONE_X1;
    kf[KSTEPS - 1] = __builtin_bit_cast(bf16x8, w);
    w = __builtin_bit_cast(u32x4, vf[KSTEPS - 1]);
    w[0] = PXA_OPERAND_MINUS_ONE_X2; w[1] = PXA_OPERAND_MINUS_ONE_X1;
    vf[KSTEPS - 1] = __builtin_bit_cast(bf16x8, w);
  }
  const bf16_t* Qp = p.Q + (long)b * p.q_bs + (long)h * p.q_hs;
  const bf16_t* Dp = p.dO + (long)b * p.o_bs + (long)h * p.o_hs;
  const bf16_t* Ls = p.stats + ((long)b * p.H + h) * p.Nq64 * 8;
  const bf16_t* Ds = Ls + (long)p.B * p.H * p.Nq64 * 8;
  const int qts = (int)p.q_ts, ots = (int)p.o_ts;
  FragAddr fa;
  frag_addr(fa, lane);
  int r4[2];
#pragma unroll
  for (int sub = 0; sub < 2; sub++) r4[sub] = hi ? TILE_B + (sub * 32 + (lane & 31)) * 16 : fa.rb[0] + 2 * 64 + sub * 32 * ROWB;
  // DMA: the 24 one-KiB pieces of a {Q, dO} tile pair over 8 waves: wave w takes pieces w, w + 8, w + 16 (0..11 = Q tile, 12..23 = dO tile)
  constexpr int DOFF = TILE_B + STAT_B;                    // dO tile relative to the Q tile of its stage
  int prow[3], pcoff[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int g = i * 8 + wave, piece = g % 12, pp = piece * 64 + lane, r = pp / 12, cl = pp - r * 12, cc = cl ^ ((r >> 2) & 3);
    prow[i] = r;
    pcoff[i] = cc < NCH ? cc * 8 : -1;
  }
  const int T = (p.Nq + BKV - 1) / BKV;
  auto issue = [&](int t, char* st) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int g = i * 8 + wave;                           // wave-uniform: which tile, which piece
      const bool isd = g >= 12;
      const int gr = min(t * BKV + prow[i], p.Nq - 1);
      if (pcoff[i] >= 0)
        lds_dma16((isd ? Dp : Qp) + (long)gr * (isd ? ots : qts) + pcoff[i], st + (isd ? DOFF : 0) + (g % 12) * 1024);
    }
    if (wave < 2) lds_dma16((wave == 0 ? Ls : Ds) + ((long)t * BKV + lane) * 8, st + (wave == 0 ? TILE_B : 2 * TILE_B + STAT_B));
  };
  for (int st = 0; st < NSTAGE; st++) {
    init_pads(smem + st * STAGE_B, 0, tid);
    init_pads(smem + st * STAGE_B + DOFF, 0, tid);
  }
  auto bar = [&]() { __builtin_amdgcn_s_barrier(); };
  auto stage = [&](int i) -> char* { return smem + i * STAGE_B; };
  issue(0, stage(0));
  if (T > 1) issue(1, stage(1));
  lds_dma_wait<0>();
  __syncthreads();                                          // tiles 0 and 1 have landed, pads written
  if (!wave_active) {                                       // DMA, waits and barriers only, in the group's rhythm
    if (grp == 1) bar();
    bar();
    int in2 = 2;
    for (int t = 0; t < T; t++) {
      if (grp == 1 && t + 2 < T) issue(t + 2, stage(in2));  // group 1: start of its first V
      bar();
      if (grp == 0 && t + 2 < T) issue(t + 2, stage(in2));  // group 0: start of its first M
      if (grp == 1) lds_dma_wait<0>();
      bar();
      if (grp == 0) lds_dma_wait<0>();
      bar();
      bar();
      in2 = in2 == NSTAGE - 1 ? 0 : in2 + 1;
    }
    if (grp == 0) bar();
    return;
  }
  f32x16 dk[3], dv[3];
  zero3(dk);
  zero3(dv);
  const float c = p.scale_log2;
  const unsigned lds0 = (unsigned)(uintptr_t)LDS_PTR(char, smem);
  f32x16 s, dp;
  bf16x8 pb[2], db[2], f[NF];
  struct Bases { unsigned r0, r1, r40, r41, t0, t1; };
  auto bases = [&](unsigned st) -> Bases { return Bases{st + (unsigned)fa.rb[0], st + (unsigned)fa.rb[1], st + (unsigned)r4[0], st + (unsigned)r4[1],
                                                        st + (unsigned)fa.tb[0], st + (unsigned)fa.tb[1]}; };
  auto rd_row = [&](auto subc, auto kc, bf16x8& d, const Bases& bs) {
    constexpr int sub = decltype(subc)::value, k = decltype(kc)::value, ks = k >> 1, w = k & 1;
    if constexpr (ks < KSTEPS - 1) lds_row_asm<w * DOFF + sub * 32 * ROWB + (ks >> 1) * 64>(d, (ks & 1) ? bs.r1 : bs.r0);
    else lds_row_asm<w * DOFF>(d, sub ? bs.r41 : bs.r40);
  };
  auto rd_tr = [&](auto subc, auto kc, bf16x8& d, const Bases& bs) {
    constexpr int sub = decltype(subc)::value, k = decltype(kc)::value, uu = k / 6, dt = (k % 6) >> 1, w = k & 1;
    lds_tr_asm<(w ? 0 : DOFF) + (sub * 2 + uu) * 16 * ROWB + dt * 64>(d, bs.t0, bs.t1);
  };
  // phase M as ONE chain of 22 fragments: 12 transpose fragments of C(sub CSUB of the stage behind cb; 2 reads each), then 10 row fragments of A(sub ASUB
  // of the stage behind ab; 1 read each).  Fragment i sits in f[i % NF]; the first D = NF - 1 are in flight on entry (issued by the V phase before);
  // slot k = {wait for fragment k: the reads issued after it are those of fragments k+1 .. k+D-1; MFMA k; issue fragment k+D}.  Nothing in flight after.
  auto frag_issue = [&](auto ic_, auto csubc, auto asubc, const Bases& cb, const Bases& ab) {
    constexpr int i = decltype(ic_)::value;
    if constexpr (i < 12) rd_tr(csubc, IntC<i>{}, f[i % NF], cb);
    else if constexpr (i < 22) rd_row(asubc, IntC<i - 12>{}, f[i % NF], ab);
  };
  auto mChain = [&](auto csubc, auto asubc, const Bases& cb, const Bases& ab) {
    static_for<22>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      constexpr int nafter = [] { int n = 0; for (int i = k + 1; i < k + DK && i < 22; i++) n += i < 12 ? 2 : 1; return n; }();
      lds_wait<nafter>(f[k % NF]);
      if constexpr (k < 12) {
        constexpr int uu = k / 6, dt = (k % 6) >> 1;
        if constexpr (k & 1) dk[dt] = mfma32(f[k % NF], db[uu], dk[dt]);
        else dv[dt] = mfma32(f[k % NF], pb[uu], dv[dt]);
      } else {
        constexpr int j = k - 12;
        if constexpr (j == 0) { f32x16 z; for (int g = 0; g < 16; g++) z[g] = 0.f; s = mfma32(f[k % NF], kf[0], z); }
        else if constexpr (j == 1) { f32x16 z; for (int g = 0; g < 16; g++) z[g] = 0.f; dp = mfma32(f[k % NF], vf[0], z); }
        else if constexpr (j & 1) dp = mfma32(f[k % NF], vf[j >> 1], dp);
        else s = mfma32(f[k % NF], kf[j >> 1], s);
      }
      frag_issue(IntC<k + DK>{}, csubc, asubc, cb, ab);
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  // A alone (prologue): row fragments only, cold
  auto mA0 = [&](const Bases& ab) {
    static_for<DK>([&](auto ic_) { rd_row(IntC<0>{}, ic_, f[decltype(ic_)::value % NF], ab); });
    __builtin_amdgcn_sched_barrier(0);
    static_for<10>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      constexpr int nafter = (k + DK - 1 < 10 ? DK - 1 : 9 - k);
      lds_wait<nafter>(f[k % NF]);
      if constexpr (k == 0) { f32x16 z; for (int g = 0; g < 16; g++) z[g] = 0.f; s = mfma32(f[k % NF], kf[0], z); }
      else if constexpr (k == 1) { f32x16 z; for (int g = 0; g < 16; g++) z[g] = 0.f; dp = mfma32(f[k % NF], vf[0], z); }
      else if constexpr (k & 1) dp = mfma32(f[k % NF], vf[k >> 1], dp);
      else s = mfma32(f[k % NF], kf[k >> 1], s);
      if constexpr (k + DK < 10) rd_row(IntC<0>{}, IntC<k + DK>{}, f[(k + DK) % NF], ab);
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  // phase V: B in place, then the first D fragments of the M phase that follows (C of sub CSUB of the stage behind cb)
  auto vB = [&](auto csubc, const Bases& cb) {
#pragma unroll
    for (int g = 0; g < 16; g++) {
      const float pr = __builtin_amdgcn_exp2f(s[g] * c);
      s[g] = pr;
      dp[g] = pr * dp[g];
    }
#pragma unroll
    for (int uu = 0; uu < 2; uu++) { pb[uu] = pack8(s, 8 * uu); db[uu] = pack8(dp, 8 * uu); }
    asm volatile("" : "+v"(pb[0]), "+v"(pb[1]), "+v"(db[0]), "+v"(db[1]));
    __builtin_amdgcn_sched_barrier(0);
    static_for<DK>([&](auto ic_) { rd_tr(csubc, ic_, f[decltype(ic_)::value % NF], cb); });
    __builtin_amdgcn_sched_barrier(0);
  };

  if (grp == 1) bar();                                      // group 1 sits out the phase in which group 0 computes its A(0, 0)
  mA0(bases(lds0));
  bar();
  int ic = 0;
  for (int t = 0; t < T; t++) {
    const int in = ic == NSTAGE - 1 ? 0 : ic + 1, in2 = in == NSTAGE - 1 ? 0 : in + 1;
    unsigned cst = lds0 + ic * STAGE_B;
    asm volatile("" : "+s"(cst));                           // per-stage lane addresses are rebuilt where they are used, not carried through the loop
    // ---- V: B(2t)
    if (grp == 1 && t + 2 < T) issue(t + 2, stage(in2));
    vB(IntC<0>{}, bases(cst));
    bar();
    // ---- M: C(2t), A(2t+1)
    if (grp == 0 && t + 2 < T) issue(t + 2, stage(in2));
    {
      const Bases cb = bases(cst);
      mChain(IntC<0>{}, IntC<1>{}, cb, cb);
    }
    if (grp == 1) lds_dma_wait<0>();
    bar();
    // ---- V: B(2t+1)
    asm volatile("" : "+s"(cst));
    vB(IntC<1>{}, bases(cst));
    if (grp == 0) lds_dma_wait<0>();
    bar();
    // ---- M: C(2t+1), A(2t+2) (the last tile re-reads its own first sub-tile: unused)
    {
      unsigned nst = lds0 + ((t + 1 < T) ? in : ic) * STAGE_B;
      asm volatile("" : "+s"(cst), "+s"(nst));
      const Bases cb = bases(cst), nb = bases(nst);
      mChain(IntC<1>{}, IntC<0>{}, cb, nb);
    }
    bar();
    ic = in;
  }
  if (grp == 0) bar();                                      // group 1's last phase
  if (kvvalid) {
    store_rows(p.dK + dkbase + (long)kv * p.dk_ts + (long)h * p.dk_hs, dk, p.dk_scale, hi);
    store_rows(p.dV + dvbase + (long)kv * p.dv_ts + (long)h * p.dv_hs, dv, 1.f, hi);
  }
  if (p.dk_colsum) colsum_rows(p.dk_colsum + (b % PXA_COLSUM_SLOTS) * p.colsum_stride + h * DH, dk, p.dk_scale, kvvalid, hi, lane);
  if (p.dv_colsum) colsum_rows(p.dv_colsum + (b % PXA_COLSUM_SLOTS) * p.colsum_stride + h * DH, dv, 1.f, kvvalid, hi, lane);
}

// attn_bwd_dkv4_kernel with the SECOND products (dV^T = dO^T P, dK^T = Q^T dS: head_dim as output rows) on v_mfma_f32_16x16x32: 72 rows pad to 80 (5 tiles of 16)
// instead of 96 (3 of 32) - 40 MFMAs of 16 cycles per sub-tile instead of 24 of 32 (640 against 768 matrix-pipe cycles; the whole step 1280 against 1408), in
// the shape the power limit favours (common.h mfma16).  Round 2 measured this 3-7 % SLOWER in the two-wave kernel - issue-bound: the 16-cycle MFMAs left the
// partner wave's softmax too few slots; the one-wave kernel has them (ablation r4_17: its vector and LDS work fit with room).  P and dS take pack_xy's
// lane exchange (4 v_permlane16_swap per 32 x 32 block), the A operands are trfrag16 reads; dK^T / dV^T leave through store_rows16 (PXA_ATTN_DKV=5).
// Alone 2.5 % faster than attn_bwd_dkv4_kernel, inside the training step 2.4 ms per step slower (profiles/r4_34_step_ab_attention.txt): an A/B partner, not the default.
template <bool PRE>     // PRE: q arrives as (scale log2 e) x queries (pxa_attn_args.q_prescaled): S needs no multiply in front of exp2
__global__ __launch_bounds__(256, 1) void attn_bwd_dkv5_kernel(AttnParams p) {
  __shared__ __attribute__((aligned(16))) char smem[DKV4_STAGES * STAGE_B];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hi = lane >> 5;
  int bx, h, b;
  block_coords(p, bx, h, b);
  const long kbase = (long)b * p.k_bs, vbase = (long)b * p.v_bs, dkbase = (long)b * p.dk_bs, dvbase = (long)b * p.dv_bs;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

  const bf16_t* Qp = p.Q + (long)b * p.q_bs + (long)h * p.q_hs;
  const bf16_t* Dp = p.dO + (long)b * p.o_bs + (long)h * p.o_hs;
  const bf16_t* Ls = p.stats + ((long)b * p.H + h) * p.Nq64 * 8;
  const bf16_t* Ds = Ls + (long)p.B * p.H * p.Nq64 * 8;
  const int qts = (int)p.q_ts, ots = (int)p.o_ts;
  const int T = p.Nq / BKV;                                        // full 64-query tiles (checked by the launcher)
  const float c = p.scale_log2;

  // LDS-DMA plan (saddr form: wave-uniform tile base + per-lane byte offset; Q and dO piece i share their lane mask)
  DmaPlan pl;
  dma_plan(pl, wave, lane);
  unsigned offQ[NDMA], offD[NDMA];
  unsigned long long dmask[NDMA];
#pragma unroll
  for (int i = 0; i < NDMA; i++) {
    offQ[i] = (unsigned)(pl.row[i] * qts + pl.coff[i]) * 2u;
    offD[i] = (unsigned)(pl.row[i] * ots + pl.coff[i]) * 2u;
    dmask[i] = __builtin_amdgcn_ballot_w64(pl.coff[i] >= 0);
  }
  const unsigned lds0 = (unsigned)(uintptr_t)LDS_PTR(char, smem);
  const unsigned wbase = __builtin_amdgcn_readfirstlane(wave * 1024);          // (stage addresses are added per fetch)
  const long qstep = (long)BKV * qts, ostep = (long)BKV * ots;
  const unsigned stat_off = (unsigned)lane * 16u;                  // statistics rows: 64 x 16 B per tile, one piece; waves 0 / 2 fetch L, waves 1 / 3 D
  const bf16_t* statp = (wave & 1) ? Ds : Ls;
  const unsigned stat_dst = __builtin_amdgcn_readfirstlane((wave & 1) ? 2 * TILE_B + STAT_B : TILE_B);
  // tile fetch, in four parts (three {Q, dO} piece pairs + the statistics piece) so that the loop can spread them over MFMA gaps; the source pointers
  // are running ones (qnext / dnext / snext: the next tile to fetch, clamped to the last one - past it a harmless re-fetch keeps every wave's piece
  // count, and with it the counted vmcnt, uniform)
  const bf16_t* qnext = Qp;
  const bf16_t* dnext = Dp;
  const bf16_t* snext = statp;
  auto issue_part = [&](auto pc, unsigned sb) {                    // sb = LDS byte address of the stage
    constexpr int P = decltype(pc)::value;
    const unsigned wb = wbase + sb, so = stat_off, sd = stat_dst + sb;
    const bf16_t* sn = snext;
    if constexpr (P == 0) dma_pair<0, TILE_B + STAT_B>(dmask[0], wb, offQ[0], qnext, offD[0], dnext);
    if constexpr (P == 1) dma_pair<4096, TILE_B + STAT_B + 4096>(dmask[1], wb, offQ[1], qnext, offD[1], dnext);
    if constexpr (P == 2) dma_pair<8192, TILE_B + STAT_B + 8192>(dmask[2], wb, offQ[2], qnext, offD[2], dnext);
    if constexpr (P == 3) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(sd), "v"(so), "s"(sn) : "memory");
  };
  int tfetch = 0;                                                  // tile index behind qnext / dnext / snext
  auto advance = [&]() {
    const bool more = tfetch + 1 < T;
    qnext += more ? qstep : 0; dnext += more ? ostep : 0; snext += more ? (long)BKV * 8 : 0;
    tfetch++;
  };
  auto issue = [&](unsigned sb) { issue_part(IntC<0>{}, sb); issue_part(IntC<1>{}, sb); issue_part(IntC<2>{}, sb); issue_part(IntC<3>{}, sb); advance(); };

  // fragment addressing inside a stage: per-lane bases + instruction immediates (see attn_bwd_dkv2_kernel); `cur` = stage of tile t, `nxt` = of tile t+1
  FragAddr fa;
  frag_addr(fa, lane);
  int r4[2];
#pragma unroll
  for (int sub = 0; sub < 2; sub++) r4[sub] = hi ? TILE_B + (sub * 32 + (lane & 31)) * 16 : fa.rb[0] + 2 * 64 + sub * 32 * ROWB;
  Tr16Addr ta;
  tr16_addr(ta, lane);
  struct Bases { unsigned r0, r1, r40, r41, t00, t01, t10, t11; };
  auto bases = [&](unsigned st) -> Bases { return Bases{st + (unsigned)fa.rb[0], st + (unsigned)fa.rb[1], st + (unsigned)r4[0], st + (unsigned)r4[1],
                                                        st + (unsigned)ta.tb[0][0], st + (unsigned)ta.tb[0][1], st + (unsigned)ta.tb[1][0], st + (unsigned)ta.tb[1][1]}; };
  constexpr int DOFF = TILE_B + STAT_B;

  for (int st = 0; st < DKV4_STAGES; st++) {
    init_pads(smem + st * STAGE_B, 0, tid);
    init_pads(smem + st * STAGE_B + DOFF, 0, tid);
  }
  Acc16 dk[2], dv[2];                                              // [kb]: dK^T / dV^T in 16-row tiles: lane (R, c): d = 16 t + 4 R + g, key c (half 0) / 16 + c (half 1)
#pragma unroll
  for (int kb = 0; kb < 2; kb++) {
    zero16(dk[kb]); zero16(dv[kb]);
#pragma unroll
    for (int tt = 0; tt < NT16; tt++) { to_agpr(dk[kb].v[tt][0]); to_agpr(dk[kb].v[tt][1]); to_agpr(dv[kb].v[tt][0]); to_agpr(dv[kb].v[tt][1]); }
  }
  f32x16 S[2][2], dP[2];                                           // S[buffer][kb] (S'(j) in buffer j & 1; E(j) leaves P there), dP[kb]
  u32x4 pxu[2], pyu[2], dxu[2], dyu[2];                            // [kb]: P / dS of the sub-tile's 32 queries, packed and lane-exchanged (pack_xy): keys 0-15 / 16-31 of the block
  bf16x8 f[4];                                                     // fragment quads

  // fragment i of step (SUB): 0..4 Q rows of the next sub-tile (k-step i), 5..9 dO rows, 10..14 dO^T (16-row tile t), 15..19 Q^T (tile t); i >= 20: the
  // next step's fragments (look-ahead).  cb = this tile's stage, nb = the next tile's.
  auto rd_frag = [&](auto subc, auto ic, bf16x8& d, const Bases& cb, const Bases& nb) {
    constexpr int SUB = decltype(subc)::value, I = decltype(ic)::value;
    if constexpr (I >= 20) {                                       // next step: its fragments 0..3 are looked ahead (Q rows, k-steps 0..3)
      constexpr int ks = I - 20;
      static_assert(ks < KSTEPS - 1, "look-ahead reaches the statistics fragment");
      // next step = (SUB ^ 1): its S block reads the sub-tile after it: SUB == 0 -> next step is sub 1 of this tile, reads (t+1, sub 0); SUB == 1 -> next
      // step is sub 0 of tile t+1, reads (t+1, sub 1)
      lds_row_asm<(SUB ? 32 * ROWB : 0) + (ks >> 1) * 64>(d, (ks & 1) ? nb.r1 : nb.r0);
    } else if constexpr (I < 5) {
      constexpr int ks = I;
      if constexpr (SUB == 0) {                                    // (t, sub 1)
        if constexpr (ks < KSTEPS - 1) lds_row_asm<32 * ROWB + (ks >> 1) * 64>(d, (ks & 1) ? cb.r1 : cb.r0);
        else lds_row_asm<0>(d, cb.r41);
      } else {                                                     // (t+1, sub 0)
        if constexpr (ks < KSTEPS - 1) lds_row_asm<(ks >> 1) * 64>(d, (ks & 1) ? nb.r1 : nb.r0);
        else lds_row_asm<0>(d, nb.r40);
      }
    } else if constexpr (I < 10) {
      constexpr int ks = I - 5;
      if constexpr (ks < KSTEPS - 1) lds_row_asm<DOFF + SUB * 32 * ROWB + (ks >> 1) * 64>(d, (ks & 1) ? cb.r1 : cb.r0);
      else lds_row_asm<DOFF>(d, SUB ? cb.r41 : cb.r40);
    } else {
      constexpr int tt = (I - 10) % 5, isq = I >= 15;               // trfrag16: rows of the sub-tile's 32 queries, 16 head dims
      lds_tr_asm<(isq ? 0 : DOFF) + SUB * 32 * ROWB + (tt >> 1) * 64>(d, (tt & 1) ? cb.t01 : cb.t00, (tt & 1) ? cb.t11 : cb.t10);
    }
  };

  // ---- prologue: tiles 0, 1, 2 in flight; S'(0); look-ahead fragments 0, 1 of step 0
  issue(lds0);
  issue(lds0 + STAGE_B);
  issue(lds0 + 2 * STAGE_B);
  // (the stationary rows are fetched BEHIND the first tiles' DMA: the two latencies overlap)
  // stationary operands: K / V rows of this wave's 2 x 32 keys (B operands: lane = key), -1.0 in k-slots 72..74 against the statistics rows
  int kv[2];
  bf16x8 kf[2][KSTEPS], vf[2][KSTEPS];
#pragma unroll
  for (int kb = 0; kb < 2; kb++) {
    kv[kb] = bx * 256 + wave * 64 + kb * 32 + (lane & 31);
    const bool kvok = kv[kb] < p.Nk;                               // Nk % 64 == 0: a key block is whole or absent (its waves then carry zeros and store nothing)
    load_row_frags(kf[kb], p.K + kbase + (long)kv[kb] * p.k_ts + (long)h * p.k_hs, kvok, hi);
    load_row_frags(vf[kb], p.V + vbase + (long)kv[kb] * p.v_ts + (long)h * p.v_hs, kvok, hi);
    settle(kf[kb]);
    settle(vf[kb]);
    if (hi == 1) {
      u32x4 w = __builtin_bit_cast(u32x4, kf[kb][KSTEPS - 1]);
      w[0] = PXA_OPERAND_MINUS_ONE_X2; w[1] = PXA_OPERAND_MINUS_ONE_X1;
      kf[kb][KSTEPS - 1] = __builtin_bit_cast(bf16x8, w);
      w = __builtin_bit_cast(u32x4, vf[kb][KSTEPS - 1]);
      w[0] = PXA_OPERAND_MINUS_ONE_X2; w[1] = PXA_OPERAND_MINUS_ONE_X1;
      vf[kb][KSTEPS - 1] = __builtin_bit_cast(bf16x8, w);
    }
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) to_agpr(vf[kb][ks]);
  }
  lds_dma_wait<14>();
  __syncthreads();
  {
    const Bases cb = bases(lds0);
    static_for<5>([&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      if constexpr (ks < KSTEPS - 1) lds_row_asm<(ks >> 1) * 64>(f[ks & 3], (ks & 1) ? cb.r1 : cb.r0);
      else lds_row_asm<0>(f[0], cb.r40);
      if constexpr (ks == 3) { lds_wait<0>(f[0]); }                // (quad 0 is reused by k-step 4: settle k-step 0 first)
      if constexpr (ks == 3) { mfma32_vv_first(S[0][0], f[0], kf[0][0]); mfma32_vv_first(S[0][1], f[0], kf[1][0]); }
    });
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
    mfma32_vv(S[0][0], f[1], kf[0][1]); mfma32_vv(S[0][1], f[1], kf[1][1]);
    mfma32_vv(S[0][0], f[2], kf[0][2]); mfma32_vv(S[0][1], f[2], kf[1][2]);
    mfma32_vv(S[0][0], f[3], kf[0][3]); mfma32_vv(S[0][1], f[3], kf[1][3]);
    mfma32_vv(S[0][0], f[0], kf[0][4]); mfma32_vv(S[0][1], f[0], kf[1][4]);
    mfma_drain();
#pragma unroll
    for (int kb = 0; kb < 2; kb++)
#pragma unroll
      for (int g = 0; g < 16; g++) if (!PRE) S[0][kb][g] *= c;     // (inside the loop the next step's scores are scaled under the dK MFMAs)
    static_for<4>([&](auto ic) { rd_frag(IntC<0>{}, ic, f[decltype(ic)::value], cb, cb); });   // step 0 (tile 0, sub 0): fragments 0..3 = Q rows of (0, sub 1)
  }

  // ---- one step = one 32-query sub-tile: 20 fragments (quad of fragment i = i & 3), consumed in pairs behind ONE counted wait, re-read four ahead.
  // MFMA gaps: 0..19 S(j+1) / dP(j) (v_mfma_f32_32x32x16, two per row fragment: key blocks 0, 1), 20..39 dV(j), 40..59 dK(j) (v_mfma_f32_16x16x32, four per
  // transposed fragment: {kb 0, kb 1} x {keys 0-15, keys 16-31}).  Vector work, a producer always at least one MFMA in front of its consumer:
  //   gaps  0..15  exp2 of S'(j) c (2 scores per gap) -> P;  cvt_pk two gaps behind;  the four lane swaps of key block 0 in gaps 13 / 14, of 1 in 18 / 19
  //   gaps 20..35  dS = P dP' (2 per gap);  cvt_pk two gaps behind (.. 37);  swaps of key block 0 in gaps 30 / 31, of key block 1 in 38 / 39
  //   gaps 40..59  S'(j+1) *= c
  int t = 0;
  auto step = [&](auto subc, const Bases& cb, const Bases& nb, unsigned fst) {      // fst: LDS address of the stage tile t+3 is fetched into
    constexpr int SUB = decltype(subc)::value, CUR = SUB, NXT = SUB ^ 1;
    // pair pr = 0..15 of a 32-score block set (kb = pr >> 3, scores g = 2 (pr & 7), + 1) -> word of ua (-> x) or ub (-> y), pack_xy's layout
    auto cvt_pair = [&](auto prc, f32x16 (&src)[2], u32x4 (&xu)[2], u32x4 (&yu)[2]) {
      constexpr int pr = decltype(prc)::value;
      if constexpr (pr >= 0 && pr < 16) {
        constexpr int kb = pr >> 3, g = 2 * (pr & 7), w = (g >> 3) * 2 + ((g & 3) >> 1);
        constexpr bool isb = (g & 4) != 0;
        unsigned v = (DKV4_ABL & 2) ? __builtin_bit_cast(unsigned, src[kb][g]) : pack_bf16x2(src[kb][g], src[kb][g + 1]);
        asm volatile("" : "+v"(v));
        if constexpr (isb) yu[kb][w] = v; else xu[kb][w] = v;
      }
    };
    auto swap2 = [&](auto kbc, auto w0c, u32x4 (&xu)[2], u32x4 (&yu)[2]) {
      constexpr int kb = decltype(kbc)::value, w0 = decltype(w0c)::value;
      static_for<2>([&](auto wc) {
        constexpr int w = w0 + decltype(wc)::value;
        if (!(DKV4_ABL & 2)) { const auto r = __builtin_amdgcn_permlane16_swap(xu[kb][w], yu[kb][w], false, false); xu[kb][w] = r[0]; yu[kb][w] = r[1]; }
        asm volatile("" : "+v"(xu[kb][w]), "+v"(yu[kb][w]));
      });
    };
    auto valu = [&](auto gic) {
      constexpr int gi = decltype(gic)::value;
      if constexpr (gi < 20) {
        if constexpr (gi < 16) static_for<2>([&](auto ec) {
          constexpr int e = 2 * gi + decltype(ec)::value;
          if (!(DKV4_ABL & 1)) S[CUR][e >> 4][e & 15] = __builtin_amdgcn_exp2f(S[CUR][e >> 4][e & 15]);
          asm volatile("" : "+v"(S[CUR][e >> 4][e & 15]));
        });
        cvt_pair(IntC<gi - 2>{}, S[CUR], pxu, pyu);
        if constexpr (gi == 13) swap2(IntC<0>{}, IntC<0>{}, pxu, pyu);
        if constexpr (gi == 14) swap2(IntC<0>{}, IntC<2>{}, pxu, pyu);
        if constexpr (gi == 18) swap2(IntC<1>{}, IntC<0>{}, pxu, pyu);
        if constexpr (gi == 19) swap2(IntC<1>{}, IntC<2>{}, pxu, pyu);
      } else if constexpr (gi < 40) {
        if constexpr (gi < 36) static_for<2>([&](auto ec) {
          constexpr int e = 2 * (gi - 20) + decltype(ec)::value;
          if (!(DKV4_ABL & 4)) dP[e >> 4][e & 15] *= S[CUR][e >> 4][e & 15];
          asm volatile("" : "+v"(dP[e >> 4][e & 15]));
        });
        cvt_pair(IntC<gi - 22>{}, dP, dxu, dyu);
        if constexpr (gi == 30) swap2(IntC<0>{}, IntC<0>{}, dxu, dyu);
        if constexpr (gi == 31) swap2(IntC<0>{}, IntC<2>{}, dxu, dyu);
        if constexpr (gi == 38) swap2(IntC<1>{}, IntC<0>{}, dxu, dyu);
        if constexpr (gi == 39) swap2(IntC<1>{}, IntC<2>{}, dxu, dyu);
      } else if constexpr (gi < 56) {
        static_for<2>([&](auto ec) {
          constexpr int e = 2 * (gi - 40) + decltype(ec)::value;
          if (!PRE && !(DKV4_ABL & 4)) S[NXT][e >> 4][e & 15] *= c;     // (a plain `if` on the template constant: `if constexpr` here loses the lambda's capture of S)
          asm volatile("" : "+v"(S[NXT][e >> 4][e & 15]));
        });
      }
    };
    // MFMA m of fragment i (row fragments: m = kb; transposed ones: m = 2 kb + half); W >= 0: behind the counted wait
    auto mma = [&](auto ic, auto mc, auto wc) {
      constexpr int i = decltype(ic)::value, m = decltype(mc)::value, W = decltype(wc)::value, q = i & 3;
      if constexpr (DKV4_ABL & 32) { if constexpr (W >= 0) lds_wait<(W >= 0 ? W : 0)>(f[q]); return; }
      if constexpr (i < 5) { if constexpr (i == 0) mfma32_vv_first<W>(S[NXT][m], f[q], kf[m][0]); else mfma32_vv<W>(S[NXT][m], f[q], kf[m][i]); }
      else if constexpr (i < 10) { if constexpr (i == 5) mfma32_va_first<W>(dP[m], f[q], vf[m][0]); else mfma32_va<W>(dP[m], f[q], vf[m][i - 5]); }
      else {
        constexpr int kb = m >> 1, half = m & 1, tt = (i - 10) % 5;
        if constexpr (W >= 0) lds_wait<(W >= 0 ? W : 0)>(f[q]);
        if constexpr (i < 15) mfma16_acc(dv[kb].v[tt][half], f[q], __builtin_bit_cast(bf16x8, half ? pyu[kb] : pxu[kb]));
        else mfma16_acc(dk[kb].v[tt][half], f[q], __builtin_bit_cast(bf16x8, half ? dyu[kb] : dxu[kb]));
      }
    };
    auto nrd = [](int i) { const int k = ((i % 20) + 20) % 20; return k < 10 ? 1 : 2; };
    static_for<10>([&](auto kc) {
      constexpr int i = 2 * decltype(kc)::value;
      constexpr int G0 = i < 10 ? 2 * i : 20 + 4 * (i - 10);       // gap index of the pair's first MFMA
      if constexpr (SUB == 0 && i == 16) {                         // the tile's barrier, in front of the first look-ahead read into tile t+1
        lds_dma_wait<7>();
        __syncthreads();
        if constexpr (!(DKV4_ABL & 16)) issue_part(IntC<0>{}, fst);
      }
      if constexpr (SUB == 0 && i == 18 && !(DKV4_ABL & 16)) issue_part(IntC<1>{}, fst);
      if constexpr (SUB == 1 && i == 0 && !(DKV4_ABL & 16)) issue_part(IntC<2>{}, fst);
      if constexpr (SUB == 1 && i == 2 && !(DKV4_ABL & 16)) { issue_part(IntC<3>{}, fst); advance(); }
      constexpr int W = nrd(i + 2) + nrd(i + 3);
      if constexpr (i < 10) {                                      // row fragments: two MFMAs each
        mma(IntC<i>{}, IntC<0>{}, IntC<W>{});
        __builtin_amdgcn_sched_barrier(0);
        valu(IntC<G0>{});
        __builtin_amdgcn_sched_barrier(0);
        mma(IntC<i>{}, IntC<1>{}, IntC<-1>{});
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!(DKV4_ABL & 8)) rd_frag(subc, IntC<i + 4>{}, f[i & 3], cb, nb);
        valu(IntC<G0 + 1>{});
        __builtin_amdgcn_sched_barrier(0);
        mma(IntC<i + 1>{}, IntC<0>{}, IntC<-1>{});
        __builtin_amdgcn_sched_barrier(0);
        valu(IntC<G0 + 2>{});
        __builtin_amdgcn_sched_barrier(0);
        mma(IntC<i + 1>{}, IntC<1>{}, IntC<-1>{});
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!(DKV4_ABL & 8)) rd_frag(subc, IntC<i + 5>{}, f[(i + 1) & 3], cb, nb);
        valu(IntC<G0 + 3>{});
        __builtin_amdgcn_sched_barrier(0);
      } else {                                                     // transposed fragments: four MFMAs each
        static_for<8>([&](auto mc) {
          constexpr int mm = decltype(mc)::value, fi = i + (mm >> 2), m = mm & 3;
          mma(IntC<fi>{}, IntC<m>{}, IntC<(mm == 0 ? W : -1)>{});
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (m == 3 && !(DKV4_ABL & 8)) rd_frag(subc, IntC<fi + 4>{}, f[fi & 3], cb, nb);
          valu(IntC<G0 + mm>{});
          __builtin_amdgcn_sched_barrier(0);
        });
      }
    });
  };
  // stage rotation without per-tile multiplies: cur / nx / (the stage of tile t+3 = the one of tile t-1) walk the ring by additions
  unsigned cur = lds0, nx = lds0 + STAGE_B, fst = lds0 + 3 * STAGE_B;
  Bases cb = bases(cur);
  for (t = 0; t < T; t++) {
    const Bases nb = bases(nx);
    step(IntC<0>{}, cb, nb, fst);
    step(IntC<1>{}, cb, nb, fst);
    cb = nb;
    fst = cur;
    cur = nx;
    nx = nx + STAGE_B == lds0 + DKV4_STAGES * STAGE_B ? lds0 : nx + STAGE_B;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
  lds_dma_wait<0>();                                               // the clamped re-fetches must not land in a later workgroup's LDS
  mfma_drain();
#pragma unroll
  for (int kb = 0; kb < 2; kb++) {
    const long k0 = (long)bx * 256 + wave * 64 + kb * 32;          // first key of the block: lane (R, c) stores rows k0 + c and k0 + 16 + c
    const bool kvok = k0 < p.Nk;                                   // whole block or none (Nk % 64 == 0)
    store_rows16(p.dK + dkbase + k0 * p.dk_ts + (long)h * p.dk_hs, p.dk_ts, dk[kb], p.dk_scale, p.dk_scale, kvok, kvok, lane);
    store_rows16(p.dV + dvbase + k0 * p.dv_ts + (long)h * p.dv_hs, p.dv_ts, dv[kb], 1.f, 1.f, kvok, kvok, lane);
    if (p.dk_colsum) colsum_rows16(p.dk_colsum + (b % PXA_COLSUM_SLOTS) * p.colsum_stride + h * DH, dk[kb], p.dk_scale, kvok, kvok, lane);
    if (p.dv_colsum) colsum_rows16(p.dv_colsum + (b % PXA_COLSUM_SLOTS) * p.colsum_stride + h * DH, dv[kb], 1.f, kvok, kvok, lane);
  }
}

int launch_dq_ab(AttnParams p, hipStream_t stream) {
  int qpb = 0;
  if (int rc = dq_grid(AttnDq::r2, p, qpb)) return rc;
  hipLaunchKernelGGL(attn_bwd_dq_kernel, dim3(p.nx * p.H * p.B), dim3(256), 0, stream, p);
  PXA_LAUNCH_CHECK();
  return 0;
}

int launch_dkv_ab(AttnDkv k, bool prescaled, AttnParams p, int max_k, hipStream_t stream) {
  if (int rc = dkv_grid(k, p, max_k)) return rc;
  if (p.nx > 0) {
    const dim3 grid(p.nx * p.H * p.B);
    if (k == AttnDkv::dkv5 && prescaled) hipLaunchKernelGGL(attn_bwd_dkv5_kernel<true>, grid, dim3(256), 0, stream, p);
    else if (k == AttnDkv::dkv5) hipLaunchKernelGGL(attn_bwd_dkv5_kernel<false>, grid, dim3(256), 0, stream, p);
    else if (k == AttnDkv::dkv3) hipLaunchKernelGGL(attn_bwd_dkv3_kernel<2>, grid, dim3(512), 0, stream, p);   // prefetch distances 3 / 4 / 6 measured the same
    else hipLaunchKernelGGL(attn_bwd_dkv_kernel, grid, dim3(256), 0, stream, p);
  }
  PXA_LAUNCH_CHECK();
  return 0;
}
}  // namespace
