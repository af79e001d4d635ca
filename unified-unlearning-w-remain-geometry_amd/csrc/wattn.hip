// Fused self-attention for wide heads (hd 160 / 256), forward and backward: O = softmax(scale Q K^T) V per (sample, head) over T keys,
// T a multiple of 64 up to 1024.  The DDPM AttnBlocks (one head of width 256 over 256 tokens) and the 16x16 / 8x8 / middle attn1 of the
// SD v1 UNet (8 heads of width 160) ran as batched products + softmax with the fp32 scores and bf16 probabilities in HBM; here neither
// leaves the chip.  csrc/attn.hip stops at width 80: K and V of one head no longer fit in LDS beside each other (128 KB each at
// T = hd = 256), so every kernel of this file streams its second operand in chunks of 64 rows.
//
// Lane maps are those of csrc/xattn.hip.  S^T = K Q^T on v_mfma_f32_16x16x32_bf16 with K the row operand: a lane holds
// S[query r][key 16 kb + 4 g + j] (r = lane & 15, g = lane >> 4), the softmax of a query row is spread over lanes r, r + 16, r + 32, r + 48.
// The same registers, rounded to bf16, are the column operand of O^T = V^T P^T: contraction slots 8 g .. 8 g + 7 of the 32-key step s stand
// for keys 32 s + 4 g + 0..3 and 32 s + 16 + 4 g + 0..3, and the V^T fragment is read from LDS in that order.  Both widths are multiples
// of 32: no fragment is padded.
//
// LDS images: row images [64][hd + 8] (a row is 336 / 528 bytes: the 16 rows of a ds_read_b128 fall on 16 different 16-byte slots of the
// bank row) and transposed images [hd][64 + 8] (144-byte rows: the 16 rows of a ds_read_b64 fall on 16 different 8-byte slots).
//
//   k_wattn_fwd      one workgroup of four waves per (sample, head, tile of 64 queries), 16 query rows per wave; K rows and V^T of 64 keys
//                    per chunk; fp32 online softmax (running m, l; the O accumulator, 16 x hd fp32 per wave, is rescaled by
//                    exp(m_old - m_new) per chunk); the next chunk's K / V are loaded into registers under the current chunk's products
//                    and written to LDS after it.  lse = m + log(l) is stored when the caller passes a pointer; O does not depend on that.
//   k_wattn_bwd_dq   the same decomposition; per chunk of 64 keys P = exp(scale S - lse), dP^T = V dO^T, dS = scale P o (dP - delta) in
//                    registers and dQ^T += K^T dS^T.  delta = rowsum(dO o O) is formed here (the diagonal of O dO^T on the matrix core) and
//                    stored to the caller's workspace for
//   k_wattn_bwd_dkv  one workgroup per (sample, head, tile of 64 keys), K / V rows of the tile resident; per chunk of 64 queries phase 1 is
//                    k_wattn_bwd_dq's (wave w = queries 16 w .. 16 w + 15) with P and dS going as bf16 to [key][query] images, phase 2
//                    dV^T += dO^T P, dK^T += Q^T dS with the hd/16 x 4 output tiles dealt round-robin to the four waves, whose fp32
//                    accumulators (2 x hd/4 registers per lane) live across the chunks.  The workgroup owns its 64 keys: it rounds and stores
//                    dK / dV itself, there are no partial sums between workgroups.
// Every sum runs in a fixed order and nothing is accumulated with atomics: two calls give the same bits.  Global offsets are 64-bit.
#include "common.h"
#include "../../include/sfron.h"

namespace {

constexpr int WA_WAVES = 4, WA_NT = WA_WAVES * 64, WA_ROWS = 64, WA_LDT = WA_ROWS + 8;
constexpr int WA_TMIN = 64, WA_TMAX = 1024;

// 1-D grid, XCD-contiguous: workgroup ids go round-robin over the 8 XCDs, id -> (id & 7) * (n / 8) + (id >> 3) gives each XCD one contiguous
// run of (sample, head, tile) triples -- the tiles of a head stream the same K / V through ONE L2 (csrc/attn.hip k_attn_fwd)
__device__ __forceinline__ int wa_wgid() {
  const int n = gridDim.x, id = blockIdx.x;
  return (n & 7) == 0 ? (id & 7) * (n >> 3) + (id >> 3) : id;
}

// 64 rows of a head slice: global -> registers -> the row image [64][HD + 8]
template <int HD>
struct WaRows {
  static constexpr int C8 = HD / 8, LDS_ = HD + 8, N = 64 * C8 / WA_NT;      // 5 / 8 pieces per thread, exactly
  bf16x8 rg[N];
  __device__ __forceinline__ void load(const __bf16* src, int64_t ld, int tid) {
#pragma unroll
    for (int it = 0; it < N; ++it) {
      const int e = tid + WA_NT * it, row = e / C8, c = e - row * C8;
      rg[it] = *reinterpret_cast<const bf16x8*>(src + (int64_t)row * ld + 8 * c);
    }
  }
  __device__ __forceinline__ void store(__bf16* dst, int tid) const {
#pragma unroll
    for (int it = 0; it < N; ++it) {
      const int e = tid + WA_NT * it, row = e / C8, c = e - row * C8;
      *reinterpret_cast<bf16x8*>(dst + row * LDS_ + 8 * c) = rg[it];
    }
  }
};
// 64 rows of a head slice -> the transposed image [HD][WA_LDT].  A thread takes 8 columns of two neighbouring rows and writes eight
// 4-byte pairs; the 32 lanes of a half wave take the 32 row pairs of one column piece: consecutive dwords of eight image rows.
template <int HD>
struct WaTrans {
  static constexpr int C8 = HD / 8, NE = 32 * C8, N = (NE + WA_NT - 1) / WA_NT;      // 640 / 1024 (row pair, piece) items
  bf16x8 rg[2 * N];
  __device__ __forceinline__ void load(const __bf16* src, int64_t ld, int tid) {
#pragma unroll
    for (int it = 0; it < N; ++it) {
      const int e = tid + WA_NT * it, rp = e & 31, c = e >> 5;
      if (e < NE) {
        rg[2 * it] = *reinterpret_cast<const bf16x8*>(src + (int64_t)(2 * rp) * ld + 8 * c);
        rg[2 * it + 1] = *reinterpret_cast<const bf16x8*>(src + (int64_t)(2 * rp + 1) * ld + 8 * c);
      }
    }
  }
  __device__ __forceinline__ void store(__bf16* dst, int tid) const {
#pragma unroll
    for (int it = 0; it < N; ++it) {
      const int e = tid + WA_NT * it, rp = e & 31, c = e >> 5;
      if (e < NE) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<bf16x2*>(dst + (8 * c + i) * WA_LDT + 2 * rp) = bf16x2{rg[2 * it][i], rg[2 * it + 1][i]};
      }
    }
  }
};

template <int HD>
constexpr int wa_rows_elems() { return 64 * (HD + 8); }
template <int HD>
constexpr int wa_trans_elems() { return HD * WA_LDT; }

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(WA_NT) void k_wattn_fwd(const __bf16* __restrict__ q, int64_t ldq, const __bf16* __restrict__ k, int64_t ldk,
                                                    const __bf16* __restrict__ v, int64_t ldv, __bf16* __restrict__ o, int64_t ldo,
                                                    float* __restrict__ lse, int T, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  constexpr int LDKS = HD + 8, KST = HD / 32, NDB = HD / 16;
  __bf16* ks = smem;                                 // [64][LDKS]   K rows of the chunk
  __bf16* vt = smem + wa_rows_elems<HD>();           // [HD][WA_LDT] V^T of the chunk
  const int ntile = T / WA_ROWS, nchunk = T / 64;
  const int wid = wa_wgid(), bh = wid / ntile, tile = wid - bh * ntile;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qrow = tile * WA_ROWS + 16 * wave + r;
  const int64_t grow = (int64_t)b * T + qrow;
  const __bf16* kb_ = k + (int64_t)b * T * ldk + h * HD;
  const __bf16* vb_ = v + (int64_t)b * T * ldv + h * HD;
  bf16x8 qf[KST];
#pragma unroll
  for (int s = 0; s < KST; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(q + grow * ldq + h * HD + 32 * s + 8 * g);
  f32x4 acc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                      // l: this lane's share of the row sum (keys 4 g + j of every 16-key block)
  WaRows<HD> kr;
  WaTrans<HD> vr;
  kr.load(kb_, ldk, tid);
  vr.load(vb_, ldv, tid);
  for (int c = 0; c < nchunk; ++c) {
    __syncthreads();                                 // the previous chunk's products have read both images
    kr.store(ks, tid);
    vr.store(vt, tid);
    __syncthreads();
    if (c + 1 < nchunk) {                            // in flight under this chunk's products
      kr.load(kb_ + (int64_t)(c + 1) * 64 * ldk, ldk, tid);
      vr.load(vb_ + (int64_t)(c + 1) * 64 * ldv, ldv, tid);
    }
    f32x4 sc[4];
    float mc = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      sc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KST; ++s) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + (16 * kb + r) * LDKS + 32 * s + 8 * g);
        sc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], sc[kb], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[kb][j] *= scale;
        mc = fmaxf(mc, sc[kb][j]);
      }
    }
    mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
    mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
    const float mn = fmaxf(m, mc);                   // finite from the first chunk on (no key is masked)
    const float alpha = __expf(m - mn);              // first chunk: exp(-inf) = 0 on l = 0, acc = 0
    m = mn;
    l *= alpha;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[kb][j] = __expf(sc[kb][j] - mn);
        l += sc[kb][j];
      }
    }
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[db] *= alpha;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf[j] = f2bf(sc[2 * st][j]);
        pf[4 + j] = f2bf(sc[2 * st + 1][j]);
      }
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const __bf16* vrow = vt + (db * 16 + r) * WA_LDT + 32 * st + 4 * g;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow), hi = *reinterpret_cast<const bf16x4*>(vrow + 16);
        const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[db], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.0f / l;
  __bf16* orow = o + grow * ldo + h * HD;
#pragma unroll
  for (int db = 0; db < NDB; ++db) *reinterpret_cast<bf16x4*>(orow + db * 16 + 4 * g) = f2bf4(acc[db] * inv);
  if (lse != nullptr && g == 0) lse[(int64_t)bh * T + qrow] = m + __logf(l);
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// The rows of Q / dO (and O) a wave works on, as MFMA column operands straight from global memory, and delta of query row r on every lane:
// delta = rowsum(dO o O) as the diagonal of O dO^T -- fp32 sums of the exact bf16 products in dP's own slot order (csrc/xattn.hip).
template <int HD, bool DELTA>
__device__ __forceinline__ float wa_load_q_do(bf16x8 (&qf)[HD / 32], bf16x8 (&dof)[HD / 32], const __bf16* qp, const __bf16* dop, const __bf16* op,
                                              int r, int g) {
  f32x4 dd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < HD / 32; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(qp + 32 * s + 8 * g);
    dof[s] = *reinterpret_cast<const bf16x8*>(dop + 32 * s + 8 * g);
    if constexpr (DELTA) {
      const bf16x8 of = *reinterpret_cast<const bf16x8*>(op + 32 * s + 8 * g);
      dd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(of, dof[s], dd, 0, 0, 0);
    }
  }
  if (!DELTA) return 0.f;
  const float dsel = (r & 2) ? ((r & 1) ? dd[3] : dd[2]) : ((r & 1) ? dd[1] : dd[0]);
  return __shfl(dsel, 16 * (r >> 2) + r, 64);         // element [row r][column r] sits in lane 16 (r >> 2) + r, register r & 3
}

// P and dS (bf16) of query r against keys 16 kb + 4 g + 0..3 of the staged K / V row images
template <int HD>
__device__ __forceinline__ void wa_p_ds(const __bf16* ks, const __bf16* vs, const bf16x8 (&qf)[HD / 32], const bf16x8 (&dof)[HD / 32], int kb, int r,
                                        int g, float scale, float ls, float dl, bf16x4& pb, bf16x4& dsb) {
  constexpr int LDKS = HD + 8;
  f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < HD / 32; ++s) {
    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + (16 * kb + r) * LDKS + 32 * s + 8 * g);
    const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vs + (16 * kb + r) * LDKS + 32 * s + 8 * g);
    sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], sc, 0, 0, 0);
    dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[s], dp, 0, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float p = __expf(sc[j] * scale - ls);
    pb[j] = f2bf(p);
    dsb[j] = f2bf(scale * p * (dp[j] - dl));
  }
}

template <int HD>
__global__ __launch_bounds__(WA_NT) void k_wattn_bwd_dq(const __bf16* __restrict__ q, int64_t ldq, const __bf16* __restrict__ k, int64_t ldk,
                                                       const __bf16* __restrict__ v, int64_t ldv, const __bf16* __restrict__ o, int64_t ldo,
                                                       const __bf16* __restrict__ d_o, int64_t lddo, const float* __restrict__ lse,
                                                       __bf16* __restrict__ dq, int64_t lddq, float* __restrict__ delta, int T, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  constexpr int KST = HD / 32, NDB = HD / 16;
  __bf16* ks = smem;                                 // [64][HD + 8]
  __bf16* vs = ks + wa_rows_elems<HD>();             // [64][HD + 8]
  __bf16* kt = vs + wa_rows_elems<HD>();             // [HD][WA_LDT]  K^T of the chunk
  const int ntile = T / WA_ROWS, nchunk = T / 64;
  const int wid = wa_wgid(), bh = wid / ntile, tile = wid - bh * ntile;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qrow = tile * WA_ROWS + 16 * wave + r;
  const int64_t grow = (int64_t)b * T + qrow;
  const __bf16* kb_ = k + (int64_t)b * T * ldk + h * HD;
  const __bf16* vb_ = v + (int64_t)b * T * ldv + h * HD;
  bf16x8 qf[KST], dof[KST];
  const float dl = wa_load_q_do<HD, true>(qf, dof, q + grow * ldq + h * HD, d_o + grow * lddo + h * HD, o + grow * ldo + h * HD, r, g);
  const float ls = lse[(int64_t)bh * T + qrow];
  if (g == 0) delta[(int64_t)bh * T + qrow] = dl;
  f32x4 acc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nchunk; ++c) {
    __syncthreads();                                 // the previous chunk's products have read the three images
    {
      WaRows<HD> rg;
      rg.load(kb_ + (int64_t)c * 64 * ldk, ldk, tid); rg.store(ks, tid);
      rg.load(vb_ + (int64_t)c * 64 * ldv, ldv, tid); rg.store(vs, tid);
      WaTrans<HD> tg;
      tg.load(kb_ + (int64_t)c * 64 * ldk, ldk, tid); tg.store(kt, tid);
    }
    __syncthreads();
    bf16x4 dsb[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      bf16x4 pb;
      wa_p_ds<HD>(ks, vs, qf, dof, kb, r, g, scale, ls, dl, pb, dsb[kb]);
    }
    // dQ^T += K^T dS^T, contraction slots as in the forward's O^T = V^T P^T
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const bf16x8 df = {dsb[2 * st][0], dsb[2 * st][1], dsb[2 * st][2], dsb[2 * st][3],
                         dsb[2 * st + 1][0], dsb[2 * st + 1][1], dsb[2 * st + 1][2], dsb[2 * st + 1][3]};
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const __bf16* krow = kt + (db * 16 + r) * WA_LDT + 32 * st + 4 * g;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(krow), hi = *reinterpret_cast<const bf16x4*>(krow + 16);
        const bf16x8 kf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, df, acc[db], 0, 0, 0);
      }
    }
  }
  __bf16* drow = dq + grow * lddq + h * HD;
#pragma unroll
  for (int db = 0; db < NDB; ++db) *reinterpret_cast<bf16x4*>(drow + db * 16 + 4 * g) = f2bf4(acc[db]);
}

template <int HD>
__global__ __launch_bounds__(WA_NT) void k_wattn_bwd_dkv(const __bf16* __restrict__ q, int64_t ldq, const __bf16* __restrict__ k, int64_t ldk,
                                                        const __bf16* __restrict__ v, int64_t ldv, const __bf16* __restrict__ d_o, int64_t lddo,
                                                        const float* __restrict__ lse, const float* __restrict__ delta, __bf16* __restrict__ dk,
                                                        int64_t lddk, __bf16* __restrict__ dv, int64_t lddv, int T, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  constexpr int KST = HD / 32, NDB = HD / 16;        // NDB * 4 output tiles of dK^T / dV^T, NDB per wave
  __bf16* ks = smem;                                 // [64][HD + 8]   K rows of this workgroup's keys (resident)
  __bf16* vs = ks + wa_rows_elems<HD>();             // [64][HD + 8]   V rows
  __bf16* qt = vs + wa_rows_elems<HD>();             // [HD][WA_LDT]   Q^T of the query chunk
  __bf16* dot = qt + wa_trans_elems<HD>();           // [HD][WA_LDT]   dO^T
  __bf16* pT = dot + wa_trans_elems<HD>();           // [64 keys][WA_LDT queries]
  __bf16* dsT = pT + 64 * WA_LDT;
  const int ntile = T / 64, nchunk = T / WA_ROWS;
  const int wid = wa_wgid(), bh = wid / ntile, tile = wid - bh * ntile;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t krow0 = (int64_t)b * T + tile * 64;
  {
    WaRows<HD> rg;
    rg.load(k + krow0 * ldk + h * HD, ldk, tid); rg.store(ks, tid);
    rg.load(v + krow0 * ldv + h * HD, ldv, tid); rg.store(vs, tid);
  }
  f32x4 acck[NDB], accv[NDB];
#pragma unroll
  for (int i = 0; i < NDB; ++i) acck[i] = accv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nchunk; ++c) {
    const int64_t grow0 = (int64_t)b * T + c * WA_ROWS;
    __syncthreads();                                 // K / V rows staged; the previous chunk's phase 2 has read qt / dot / pT / dsT
    {
      WaTrans<HD> tg;
      tg.load(q + grow0 * ldq + h * HD, ldq, tid); tg.store(qt, tid);
      tg.load(d_o + grow0 * lddo + h * HD, lddo, tid); tg.store(dot, tid);
    }
    // ---- phase 1: wave w = queries 16 w .. 16 w + 15 of the chunk against the 64 keys
    {
      const int qrow = c * WA_ROWS + 16 * wave + r;
      const int64_t grow = (int64_t)b * T + qrow;
      bf16x8 qf[KST], dof[KST];
      wa_load_q_do<HD, false>(qf, dof, q + grow * ldq + h * HD, d_o + grow * lddo + h * HD, nullptr, r, g);
      const float ls = lse[(int64_t)bh * T + qrow], dl = delta[(int64_t)bh * T + qrow];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        bf16x4 pb, dsb;
        wa_p_ds<HD>(ks, vs, qf, dof, kb, r, g, scale, ls, dl, pb, dsb);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pT[(16 * kb + 4 * g + j) * WA_LDT + 16 * wave + r] = pb[j];
          dsT[(16 * kb + 4 * g + j) * WA_LDT + 16 * wave + r] = dsb[j];
        }
      }
    }
    __syncthreads();
    // ---- phase 2: dV^T[c][key] += sum_n dO^T[c][n] P[n][key], dK^T[c][key] += sum_n Q^T[c][n] dS[n][key]
#pragma unroll
    for (int i = 0; i < NDB; ++i) {
      const int t2 = wave + WA_WAVES * i, kb = t2 / NDB, db = t2 - kb * NDB;
#pragma unroll
      for (int s = 0; s < WA_ROWS / 32; ++s) {
        const int ca = (16 * db + r) * WA_LDT + 32 * s + 8 * g, cb = (16 * kb + r) * WA_LDT + 32 * s + 8 * g;
        accv[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(dot + ca), *reinterpret_cast<const bf16x8*>(pT + cb),
                                                          accv[i], 0, 0, 0);
        acck[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(qt + ca), *reinterpret_cast<const bf16x8*>(dsT + cb),
                                                          acck[i], 0, 0, 0);
      }
    }
  }
  // a lane holds columns 16 db + 4 g + 0..3 of key 16 kb + r
#pragma unroll
  for (int i = 0; i < NDB; ++i) {
    const int t2 = wave + WA_WAVES * i, kb = t2 / NDB, db = t2 - kb * NDB;
    const int64_t row = krow0 + 16 * kb + r;
    *reinterpret_cast<bf16x4*>(dk + row * lddk + h * HD + 16 * db + 4 * g) = f2bf4(acck[i]);
    *reinterpret_cast<bf16x4*>(dv + row * lddv + h * HD + 16 * db + 4 * g) = f2bf4(accv[i]);
  }
}

template <int HD> constexpr size_t wa_lds_fwd() { return (size_t)(wa_rows_elems<HD>() + wa_trans_elems<HD>()) * sizeof(__bf16); }
template <int HD> constexpr size_t wa_lds_dq() { return (size_t)(2 * wa_rows_elems<HD>() + wa_trans_elems<HD>()) * sizeof(__bf16); }
template <int HD> constexpr size_t wa_lds_dkv() {
  return (size_t)(2 * wa_rows_elems<HD>() + 2 * wa_trans_elems<HD>() + 2 * 64 * WA_LDT) * sizeof(__bf16);
}
static_assert(wa_lds_dkv<256>() <= 160 * 1024 && wa_lds_dq<256>() <= 160 * 1024 && wa_lds_fwd<256>() <= 160 * 1024, "LDS budget");

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per function and per device
template <typename K>
inline int wa_allow_lds(K kern, size_t lds) {
  if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return (int)hipGetLastError();
  return SFRON_OK;
}

template <int HD>
int launch_wattn_fwd(const __bf16* q, int ldq, const __bf16* k, int ldk, const __bf16* v, int ldv, __bf16* o, int ldo, float* lse, int B, int T,
                     int H, float scale, hipStream_t s) {
  const size_t lds = wa_lds_fwd<HD>();
  const int st = wa_allow_lds(&k_wattn_fwd<HD>, lds);
  if (st != SFRON_OK) return st;
  hipLaunchKernelGGL((k_wattn_fwd<HD>), dim3((unsigned)((int64_t)B * H * (T / WA_ROWS))), dim3(WA_NT), lds, s, q, (int64_t)ldq, k, (int64_t)ldk, v,
                     (int64_t)ldv, o, (int64_t)ldo, lse, T, H, scale);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

template <int HD>
int launch_wattn_bwd(const __bf16* q, int ldq, const __bf16* k, int ldk, const __bf16* v, int ldv, const __bf16* o, int ldo, const __bf16* d_o,
                     int lddo, const float* lse, __bf16* dq, int lddq, __bf16* dk, int lddk, __bf16* dv, int lddv, float* delta, int B, int T, int H,
                     float scale, hipStream_t s) {
  int st = wa_allow_lds(&k_wattn_bwd_dq<HD>, wa_lds_dq<HD>());
  if (st != SFRON_OK) return st;
  st = wa_allow_lds(&k_wattn_bwd_dkv<HD>, wa_lds_dkv<HD>());
  if (st != SFRON_OK) return st;
  const dim3 grid((unsigned)((int64_t)B * H * (T / WA_ROWS)));
  hipLaunchKernelGGL((k_wattn_bwd_dq<HD>), grid, dim3(WA_NT), wa_lds_dq<HD>(), s, q, (int64_t)ldq, k, (int64_t)ldk, v, (int64_t)ldv, o, (int64_t)ldo,
                     d_o, (int64_t)lddo, lse, dq, (int64_t)lddq, delta, T, H, scale);
  SFRON_LAUNCH_STATUS();
  hipLaunchKernelGGL((k_wattn_bwd_dkv<HD>), grid, dim3(WA_NT), wa_lds_dkv<HD>(), s, q, (int64_t)ldq, k, (int64_t)ldk, v, (int64_t)ldv, d_o,
                     (int64_t)lddo, lse, delta, dk, (int64_t)lddk, dv, (int64_t)lddv, T, H, scale);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

inline bool wa_shape_ok(int T, int hd) { return (hd == 160 || hd == 256) && T >= WA_TMIN && T <= WA_TMAX && T % 64 == 0; }
inline bool wa_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// grid and row counts formed in int; offsets in the kernels are 64-bit
inline bool wa_counts_ok(int B, int T, int H) { return (int64_t)B * H * (T / WA_ROWS) < (1ll << 31) && (int64_t)B * H * T < (1ll << 31); }

}  // namespace

extern "C" {

int sfron_wattn_supported(int T, int hd) { return wa_shape_ok(T, hd) ? 1 : 0; }

int sfron_wattn_fwd(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, uint16_t* o, int ldo, float* lse, int B,
                    int T, int H, int hd, float scale, void* stream) {
  SFRON_CHECK_ARG(q && k && v && o && B > 0 && T > 0 && H > 0 && hd > 0);
  if (!wa_shape_ok(T, hd)) return SFRON_ERR_UNSUPPORTED;
  const int64_t C = (int64_t)H * hd;
  SFRON_CHECK_ARG(ldq >= C && ldk >= C && ldv >= C && ldo >= C && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0);
  SFRON_CHECK_ARG(wa_al16(q) && wa_al16(k) && wa_al16(v) && wa_al16(o) && (((uintptr_t)lse) & 3) == 0);
  SFRON_CHECK_ARG(wa_counts_ok(B, T, H));
  const __bf16 *qb = (const __bf16*)q, *kb = (const __bf16*)k, *vb = (const __bf16*)v;
  hipStream_t s = (hipStream_t)stream;
  if (hd == 160) return launch_wattn_fwd<160>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, lse, B, T, H, scale, s);
  return launch_wattn_fwd<256>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, lse, B, T, H, scale, s);
}

int64_t sfron_wattn_bwd_ws_bytes(int B, int T, int H, int hd) {
  if (B <= 0 || T <= 0 || H <= 0 || hd <= 0) return 0;
  return (((int64_t)B * H * T * (int64_t)sizeof(float)) + 15) & ~(int64_t)15;      // delta, fp32 [B*H*T]
}

int sfron_wattn_bwd(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, const uint16_t* o, int ldo,
                    const uint16_t* d_o, int ldd_o, const float* lse, uint16_t* dq, int lddq, uint16_t* dk, int lddk, uint16_t* dv, int lddv, int B,
                    int T, int H, int hd, float scale, void* ws, int64_t ws_bytes, void* stream) {
  SFRON_CHECK_ARG(q && k && v && o && d_o && lse && dq && dk && dv && ws && B > 0 && T > 0 && H > 0 && hd > 0);
  if (!wa_shape_ok(T, hd)) return SFRON_ERR_UNSUPPORTED;
  const int64_t C = (int64_t)H * hd;
  SFRON_CHECK_ARG(ldq >= C && ldk >= C && ldv >= C && ldo >= C && ldd_o >= C && lddq >= C && lddk >= C && lddv >= C);
  SFRON_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && ldd_o % 8 == 0 && lddq % 8 == 0 && lddk % 8 == 0 && lddv % 8 == 0);
  SFRON_CHECK_ARG(wa_al16(q) && wa_al16(k) && wa_al16(v) && wa_al16(o) && wa_al16(d_o) && wa_al16(dq) && wa_al16(dk) && wa_al16(dv) && wa_al16(ws) &&
                  (((uintptr_t)lse) & 3) == 0);
  SFRON_CHECK_ARG(wa_counts_ok(B, T, H));
  SFRON_CHECK_ARG(ws_bytes >= sfron_wattn_bwd_ws_bytes(B, T, H, hd));
  const __bf16 *qb = (const __bf16*)q, *kb = (const __bf16*)k, *vb = (const __bf16*)v, *ob = (const __bf16*)o, *gb = (const __bf16*)d_o;
  __bf16 *dqb = (__bf16*)dq, *dkb = (__bf16*)dk, *dvb = (__bf16*)dv;
  hipStream_t s = (hipStream_t)stream;
  if (hd == 160)
    return launch_wattn_bwd<160>(qb, ldq, kb, ldk, vb, ldv, ob, ldo, gb, ldd_o, lse, dqb, lddq, dkb, lddk, dvb, lddv, (float*)ws, B, T, H, scale, s);
  return launch_wattn_bwd<256>(qb, ldq, kb, ldk, vb, ldv, ob, ldo, gb, ldd_o, lse, dqb, lddq, dkb, lddk, dvb, lddv, (float*)ws, B, T, H, scale, s);
}

}  // extern "C"
