// Fused cross-attention: the forward for inference (the sampling loop of sfron.ddim), the same forward keeping the row statistic
// lse = m + log(l) for training, and the backward that recomputes P from it (k_xattn_bwd below).  Forward: O = softmax(scale Q K^T) V per (sample, head) with at
// most 128 keys -- SD v1's 77 context tokens padded to 80.  The scores and probabilities of UNetModel._mha (fp32 [B h N][Lk] written,
// read by the softmax, bf16 probabilities written and read again) never leave the chip here.
//
// One workgroup of four waves per (sample, head, tile of 128 query rows).  K (rows >= Lv zero) and V^T (keys >= Lv zero) of the head are
// staged in LDS once per workgroup; every wave then takes 16-row query tiles.  Lane maps as in k_attn_causal (csrc/text.hip):
// S^T = K Q^T on v_mfma_f32_16x16x32_bf16 with K the row operand, so a lane holds S[query r][key 16 kb + 4 g + j] (r = lane & 15,
// g = lane >> 4) and the softmax of a query row is spread over lanes r, r + 16, r + 32, r + 48.  The same registers, rounded to bf16, are
// the column operand of O^T = V^T P^T: contraction slots 8 g .. 8 g + 7 of the 32-key step s stand for keys 32 s + 4 g + 0..3 and
// 32 s + 16 + 4 g + 0..3, and the V^T fragment is read from LDS in that order.  The head width (40 / 80 / 160) is no multiple of the
// MFMA's 32-element contraction step: the K and Q fragments of the slots at or beyond hd are zero registers, and V^T is padded with
// zero rows to a multiple of 16 in LDS.  All global offsets are 64-bit.
#include "common.h"
#include "../../include/sfron.h"

namespace {

constexpr int XA_LMAX = 128, XA_ROWS = 128, XA_WAVES = 4;       // keys at most; query rows per workgroup; waves per workgroup

// LSE: one more store per live query row, lse[(b H + h) N + n] = m + log(l) over the scaled, masked scores (what k_xattn_bwd rebuilds P
// from); the arithmetic that forms O is the same instruction for instruction.
template <int HD, bool LSE>
__global__ __launch_bounds__(XA_WAVES * 64) void k_xattn(const __bf16* __restrict__ q, int64_t ldq, const __bf16* __restrict__ k, int64_t ldk,
                                                        const __bf16* __restrict__ v, int64_t ldv, __bf16* __restrict__ o, int64_t ldo,
                                                        float* __restrict__ lse, int N, int Lk, int Lv, int H, float scale, int ntile) {
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  constexpr int LDKS = HD + 8;                    // K row: 96 / 176 / 336 bytes
  constexpr int KST = (HD + 31) / 32;             // 32-element contraction steps of Q K^T
  constexpr int NDB = (HD + 15) / 16;             // 16-row blocks of V^T (output columns)
  constexpr int C8 = HD / 8;                      // 16-byte pieces of a head row
  const int nkb = (Lk + 15) >> 4, nst = (nkb + 1) >> 1;
  const int LDV = 32 * nst + 8;
  __bf16* ks = smem;                              // [16 nkb][LDKS]
  __bf16* vt = smem + 16 * nkb * LDKS;            // [16 NDB][LDV]
  const int bh = blockIdx.x / ntile, tile = blockIdx.x - bh * ntile;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x;
  bf16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (__bf16)0.0f;
  const __bf16* kb_ = k + (int64_t)b * Lk * ldk + h * HD;
  const __bf16* vb_ = v + (int64_t)b * Lk * ldv + h * HD;
  for (int e = tid; e < 16 * nkb * C8; e += XA_WAVES * 64) {
    const int key = e / C8, c = e - key * C8;
    const bf16x8 kv = key < Lv ? *reinterpret_cast<const bf16x8*>(kb_ + (int64_t)key * ldk + 8 * c) : z;
    *reinterpret_cast<bf16x8*>(ks + key * LDKS + 8 * c) = kv;
  }
  for (int e = tid; e < 32 * nst * 2 * NDB; e += XA_WAVES * 64) {
    const int key = e / (2 * NDB), c = e - key * (2 * NDB);
    const bf16x8 vv = (key < Lv && c < C8) ? *reinterpret_cast<const bf16x8*>(vb_ + (int64_t)key * ldv + 8 * c) : z;
#pragma unroll
    for (int i = 0; i < 8; ++i) vt[(8 * c + i) * LDV + key] = vv[i];
  }
  __syncthreads();
  const int lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int t = wave; t < XA_ROWS / 16; t += XA_WAVES) {
    const int q0 = tile * XA_ROWS + t * 16;
    if (q0 >= N) break;
    const int qrow = q0 + r;
    const bool live = qrow < N;
    const __bf16* qp = q + ((int64_t)b * N + qrow) * ldq + h * HD;
    bf16x8 qf[KST];
#pragma unroll
    for (int s = 0; s < KST; ++s) qf[s] = (live && 32 * s + 8 * g < HD) ? *reinterpret_cast<const bf16x8*>(qp + 32 * s + 8 * g) : z;
    f32x4 sc[XA_LMAX / 16];
    float m = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < XA_LMAX / 16; ++kb) {
      sc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (kb < nkb) {
#pragma unroll
        for (int s = 0; s < KST; ++s) {
          const bf16x8 kf = (32 * s + 8 * g < HD) ? *reinterpret_cast<const bf16x8*>(ks + (16 * kb + r) * LDKS + 32 * s + 8 * g) : z;
          sc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], sc[kb], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sc[kb][j] = (16 * kb + 4 * g + j < Lv) ? sc[kb][j] * scale : -INFINITY;
          m = fmaxf(m, sc[kb][j]);
        }
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));                   // key 0 is always valid (Lv >= 1): m is finite
    float l = 0.f;
#pragma unroll
    for (int kb = 0; kb < XA_LMAX / 16; ++kb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[kb][j] = kb < nkb ? __expf(sc[kb][j] - m) : 0.0f;
        l += sc[kb][j];
      }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    f32x4 acc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < XA_LMAX / 32; ++st) {
      if (st < nst) {
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pf[j] = f2bf(sc[2 * st][j]);
          pf[4 + j] = f2bf(sc[2 * st + 1][j]);
        }
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const __bf16* vrow = vt + (db * 16 + r) * LDV + 32 * st + 4 * g;
          const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow), hi = *reinterpret_cast<const bf16x4*>(vrow + 16);
          const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[db], 0, 0, 0);
        }
      }
    }
    if (live) {
      const float inv = 1.0f / l;
      __bf16* orow = o + ((int64_t)b * N + qrow) * ldo + h * HD;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
        if (db * 16 + 4 * g < HD) *reinterpret_cast<bf16x4*>(orow + db * 16 + 4 * g) = f2bf4(acc[db] * inv);
      if (LSE && g == 0) lse[(int64_t)bh * N + qrow] = m + __logf(l);
    }
  }
}

template <int HD, bool LSE>
int launch_xattn(const __bf16* q, int ldq, const __bf16* k, int ldk, const __bf16* v, int ldv, __bf16* o, int ldo, float* lse, int B, int N,
                 int Lk, int Lv, int H, float scale, hipStream_t s) {
  const int nkb = (Lk + 15) / 16, nst = (nkb + 1) / 2;
  const size_t lds = ((size_t)16 * nkb * (HD + 8) + (size_t)16 * ((HD + 15) / 16) * (32 * nst + 8)) * sizeof(__bf16);
  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per function and per device: hd 160 with more than 80 keys passes 64 KiB
  if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_xattn<HD, LSE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return (int)hipGetLastError();
  const int ntile = cdiv(N, XA_ROWS);
  hipLaunchKernelGGL((k_xattn<HD, LSE>), dim3((unsigned)((int64_t)B * H * ntile)), dim3(XA_WAVES * 64), lds, s, q, (int64_t)ldq, k, (int64_t)ldk, v,
                     (int64_t)ldv, o, (int64_t)ldo, lse, N, Lk, Lv, H, scale, ntile);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}


// ---- backward ----------------------------------------------------------------------------------------------------------------------
// Per (sample, head): P = exp(scale Q K^T - lse) (keys >= Lv: 0), delta = rowsum(dO o O), dP = dO V^T, dS = scale P o (dP - delta),
// dQ = dS K, dK = dS^T Q, dV = P^T dO.  P and dS are rounded to bf16 where they become MFMA operands, accumulation is fp32; scores, P, dP
// and dS never reach global memory.
//
// A workgroup of four waves owns one (sample, head) and a CHUNK of consecutive 64-row query tiles.  Every product is X Y^T with the
// contraction index contiguous in both operands' LDS images (or registers):
//   phase 1, wave w = query rows 16 w .. 16 w + 15 of the tile, the forward's lane map (query r on the lane, keys 16 kb + 4 g + j in the
//            registers): S^T = K Q^T and dP^T = V dO^T from the K / V row images; P, dS go as bf16 to the [key][query] images pT / dsT, and
//            dS stays in registers as the column operand of
//   phase 2a dQ^T = K^T dS^T (the forward's O^T = V^T P^T with the K^T image), stored by the wave that owns the rows;
//   phase 2b dV^T = dO^T P^T and dK^T = Q^T dS^T, contracted over the tile's 64 queries: the 16 x 16 tiles (column block db, key block kb)
//            are dealt round-robin to the four waves, which keep their fp32 accumulators in registers across the tiles of the chunk.
// At the end of its chunk a workgroup writes its fp32 partial dK / dV as a slab [2][Lk][HD] of the workspace; k_xattn_bwd_finish sums the
// slabs of a (sample, head) in chunk order -- a fixed order, no atomics: two calls give the same bits -- and rounds once to bf16.  The
// chunk length is chosen on the host so that about XB_TARGET_WG workgroups exist whatever B H is (bwd_chunks).  Rows Lv .. Lk - 1 of
// dK / dV come out as exact zeros (P and dS are 0 there) and the K / V values of those rows are never read.
// RESTAGE (hd 160 with more than 80 keys): K, V, K^T, Q^T, dO^T, pT and dsT together pass 160 KB, so K^T / Q^T / dO^T take the place of the
// K / V row images in phase 2 and K / V are staged again for every tile; otherwise the three K / V images are staged once per workgroup.
constexpr int XB_ROWS = 64, XB_LDQ = XB_ROWS + 8, XB_TARGET_WG = 1024;

struct XbLayout { int ks, vs, kt, qt, dot, pt, dst, total; };      // element (bf16) offsets into the dynamic LDS
template <int HD, bool RESTAGE>
__host__ __device__ inline XbLayout xb_layout(int Lk) {
  constexpr int NDB = (HD + 15) / 16;
  const int nkb = (Lk + 15) >> 4, nst = (nkb + 1) >> 1;
  const int szK = 16 * nkb * (HD + 8), szKT = 16 * NDB * (32 * nst + 8), szQT = 16 * NDB * XB_LDQ, szP = 16 * nkb * XB_LDQ;
  XbLayout L;
  L.ks = 0; L.vs = szK;
  if (RESTAGE) {
    L.kt = 0; L.qt = szKT; L.dot = szKT + szQT;
    const int a = 2 * szK, b = szKT + 2 * szQT;
    L.pt = a > b ? a : b;
  } else {
    L.kt = 2 * szK; L.qt = L.kt + szKT; L.dot = L.qt + szQT; L.pt = L.dot + szQT;
  }
  L.dst = L.pt + szP; L.total = L.dst + szP;
  return L;
}

// rows [16 nkb][HD + 8] of a K / V head slice (rows >= Lv zero, never read)
template <int HD>
__device__ __forceinline__ void xb_stage_rows(__bf16* dst, const __bf16* src, int64_t ld, int nkb, int Lv, int tid) {
  constexpr int C8 = HD / 8, LDKS = HD + 8;
  bf16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (__bf16)0.0f;
  for (int e = tid; e < 16 * nkb * C8; e += XA_WAVES * 64) {
    const int key = e / C8, c = e - key * C8;
    const bf16x8 kv = key < Lv ? *reinterpret_cast<const bf16x8*>(src + (int64_t)key * ld + 8 * c) : z;
    *reinterpret_cast<bf16x8*>(dst + key * LDKS + 8 * c) = kv;
  }
}
// the transposed image [16 NDB][ldt] of `nrow` rows of a head slice (rows >= nlive and columns >= HD zero)
template <int HD>
__device__ __forceinline__ void xb_stage_t(__bf16* dst, int ldt, const __bf16* src, int64_t ld, int nrow, int nlive, int tid) {
  constexpr int C8 = HD / 8, NDB = (HD + 15) / 16;
  bf16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (__bf16)0.0f;
  for (int e = tid; e < nrow * 2 * NDB; e += XA_WAVES * 64) {
    const int row = e / (2 * NDB), c = e - row * (2 * NDB);
    const bf16x8 vv = (row < nlive && c < C8) ? *reinterpret_cast<const bf16x8*>(src + (int64_t)row * ld + 8 * c) : z;
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[(8 * c + i) * ldt + row] = vv[i];
  }
}

template <int HD, bool RESTAGE>
__global__ __launch_bounds__(XA_WAVES * 64) void k_xattn_bwd(const __bf16* __restrict__ q, int64_t ldq, const __bf16* __restrict__ k, int64_t ldk,
                                                            const __bf16* __restrict__ v, int64_t ldv, const __bf16* __restrict__ o, int64_t ldo,
                                                            const __bf16* __restrict__ d_o, int64_t lddo, const float* __restrict__ lse,
                                                            __bf16* __restrict__ dq, int64_t lddq, float* __restrict__ ws, int N, int Lk, int Lv,
                                                            int H, float scale, int ntile, int nchunk, int tpc) {
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  constexpr int LDKS = HD + 8, KST = (HD + 31) / 32, NDB = (HD + 15) / 16;
  constexpr int NKB = (HD == 160 && !RESTAGE) ? 5 : XA_LMAX / 16;           // key blocks at most (the launcher sends hd 160, Lk > 80 to RESTAGE)
  // (db, kb) tiles of dK^T / dV^T per wave at most; RESTAGE chunks are one tile long and store each product as it is formed
  constexpr int MAXT = (NDB * NKB + XA_WAVES - 1) / XA_WAVES, NACC = RESTAGE ? 1 : MAXT;
  const int nkb = (Lk + 15) >> 4, nst = (nkb + 1) >> 1;
  const int LDV = 32 * nst + 8;
  const XbLayout L = xb_layout<HD, RESTAGE>(Lk);
  __bf16 *ks = smem + L.ks, *vs = smem + L.vs, *kt = smem + L.kt, *qt = smem + L.qt, *dot = smem + L.dot, *pT = smem + L.pt, *dsT = smem + L.dst;
  const int bh = blockIdx.x / nchunk, chunk = blockIdx.x - bh * nchunk;
  const int b = bh / H, h = bh - b * H;
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  bf16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (__bf16)0.0f;
  const __bf16* kb_ = k + (int64_t)b * Lk * ldk + h * HD;
  const __bf16* vb_ = v + (int64_t)b * Lk * ldv + h * HD;
  f32x4 acck[NACC], accv[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acck[i] = accv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float* slab = ws + ((int64_t)bh * nchunk + chunk) * 2 * Lk * HD;   // this chunk's fp32 [2 (dK, dV)][Lk][HD]
  if (!RESTAGE) {
    xb_stage_rows<HD>(ks, kb_, ldk, nkb, Lv, tid);
    xb_stage_rows<HD>(vs, vb_, ldv, nkb, Lv, tid);
    xb_stage_t<HD>(kt, LDV, kb_, ldk, 32 * nst, Lv, tid);
  }
  const int t_end = min(ntile, (chunk + 1) * tpc);
  for (int tile = chunk * tpc; tile < t_end; ++tile) {
    const int q0 = tile * XB_ROWS;
    if (RESTAGE) {
      xb_stage_rows<HD>(ks, kb_, ldk, nkb, Lv, tid);
      xb_stage_rows<HD>(vs, vb_, ldv, nkb, Lv, tid);
    }
    __syncthreads();                                  // K / V rows staged; the previous tile's phase 2 has left qt / dot / pT / dsT
    // ---- phase 1
    const int qrow = q0 + 16 * wave + r;
    const bool live = qrow < N;
    const int64_t grow = (int64_t)b * N + qrow;
    bf16x8 qf[KST], dof[KST];
    // delta = rowsum(dO o O) as the diagonal of O dO^T on the matrix core: fp32 sums of the exact bf16 products, in the same slot order
    // as dP's own chain (with one key, O = v and dP - delta is exactly 0).  Element [row r][column r] sits in lane 16 (r >> 2) + r,
    // register r & 3.
    f32x4 dd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KST; ++s) {
      const bool in = live && 32 * s + 8 * g < HD;
      qf[s] = in ? *reinterpret_cast<const bf16x8*>(q + grow * ldq + h * HD + 32 * s + 8 * g) : z;
      dof[s] = in ? *reinterpret_cast<const bf16x8*>(d_o + grow * lddo + h * HD + 32 * s + 8 * g) : z;
      const bf16x8 of = in ? *reinterpret_cast<const bf16x8*>(o + grow * ldo + h * HD + 32 * s + 8 * g) : z;
      dd = __builtin_amdgcn_mfma_f32_16x16x32_bf16(of, dof[s], dd, 0, 0, 0);
    }
    const float dsel = (r & 2) ? ((r & 1) ? dd[3] : dd[2]) : ((r & 1) ? dd[1] : dd[0]);
    const float dl = __shfl(dsel, 16 * (r >> 2) + r, 64);           // delta of query row r
    const float ls = live ? lse[(int64_t)bh * N + qrow] : 0.f;
    bf16x4 dsb[2 * ((NKB + 1) / 2)];
#pragma unroll
    for (int kb = 0; kb < 2 * ((NKB + 1) / 2); ++kb) {
      dsb[kb] = bf16x4{(__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};
      if (kb < nkb) {
        f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KST; ++s) {
          const bool in = 32 * s + 8 * g < HD;
          const bf16x8 kf = in ? *reinterpret_cast<const bf16x8*>(ks + (16 * kb + r) * LDKS + 32 * s + 8 * g) : z;
          const bf16x8 vf = in ? *reinterpret_cast<const bf16x8*>(vs + (16 * kb + r) * LDKS + 32 * s + 8 * g) : z;
          sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], sc, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[s], dp, 0, 0, 0);
        }
        bf16x4 pb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = (live && 16 * kb + 4 * g + j < Lv) ? __expf(sc[j] * scale - ls) : 0.0f;
          pb[j] = f2bf(p);
          dsb[kb][j] = f2bf(scale * p * (dp[j] - dl));
          pT[(16 * kb + 4 * g + j) * XB_LDQ + 16 * wave + r] = pb[j];
          dsT[(16 * kb + 4 * g + j) * XB_LDQ + 16 * wave + r] = dsb[kb][j];
        }
      }
    }
    __syncthreads();                                  // pT / dsT complete; with RESTAGE the K / V rows are no longer needed
    if (RESTAGE) xb_stage_t<HD>(kt, LDV, kb_, ldk, 32 * nst, Lv, tid);
    xb_stage_t<HD>(qt, XB_LDQ, q + ((int64_t)b * N + q0) * ldq + h * HD, ldq, XB_ROWS, min(XB_ROWS, N - q0), tid);
    xb_stage_t<HD>(dot, XB_LDQ, d_o + ((int64_t)b * N + q0) * lddo + h * HD, lddo, XB_ROWS, min(XB_ROWS, N - q0), tid);
    __syncthreads();
    // ---- phase 2a: dQ^T = K^T dS^T, contraction slots as in the forward's O^T = V^T P^T
    {
      f32x4 acc[NDB];
#pragma unroll
      for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < (NKB + 1) / 2; ++st) {
        if (st < nst) {
          const bf16x8 df = {dsb[2 * st][0], dsb[2 * st][1], dsb[2 * st][2], dsb[2 * st][3],
                             dsb[2 * st + 1][0], dsb[2 * st + 1][1], dsb[2 * st + 1][2], dsb[2 * st + 1][3]};
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const __bf16* krow = kt + (db * 16 + r) * LDV + 32 * st + 4 * g;
            const bf16x4 lo = *reinterpret_cast<const bf16x4*>(krow), hi = *reinterpret_cast<const bf16x4*>(krow + 16);
            const bf16x8 kf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, df, acc[db], 0, 0, 0);
          }
        }
      }
      if (live) {
        __bf16* drow = dq + grow * lddq + h * HD;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
          if (db * 16 + 4 * g < HD) *reinterpret_cast<bf16x4*>(drow + db * 16 + 4 * g) = f2bf4(acc[db]);
      }
    }
    // ---- phase 2b: dV^T[c][key] += sum_n dO^T[c][n] P[n][key], dK^T[c][key] += sum_n Q^T[c][n] dS[n][key]
#pragma unroll
    for (int i = 0; i < MAXT; ++i) {
      const int t2 = wave + XA_WAVES * i;
      if (t2 < NDB * nkb) {
        const int kb = t2 / NDB, db = t2 - kb * NDB;
        f32x4 av = RESTAGE ? f32x4{0.f, 0.f, 0.f, 0.f} : accv[RESTAGE ? 0 : i], ak = RESTAGE ? f32x4{0.f, 0.f, 0.f, 0.f} : acck[RESTAGE ? 0 : i];
#pragma unroll
        for (int s = 0; s < XB_ROWS / 32; ++s) {
          const int ca = (16 * db + r) * XB_LDQ + 32 * s + 8 * g, cb = (16 * kb + r) * XB_LDQ + 32 * s + 8 * g;
          av = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(dot + ca), *reinterpret_cast<const bf16x8*>(pT + cb), av, 0, 0, 0);
          ak = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(qt + ca), *reinterpret_cast<const bf16x8*>(dsT + cb), ak, 0, 0, 0);
        }
        if (RESTAGE) {
          const int key = 16 * kb + r, c = 16 * db + 4 * g;
          if (key < Lk && c < HD) {
            *reinterpret_cast<f32x4*>(slab + (int64_t)key * HD + c) = ak;
            *reinterpret_cast<f32x4*>(slab + ((int64_t)Lk + key) * HD + c) = av;
          }
        } else {
          accv[RESTAGE ? 0 : i] = av; acck[RESTAGE ? 0 : i] = ak;
        }
      }
    }
    __syncthreads();                                  // phase 2 has read every image before the next tile's staging overwrites them
  }
  // ---- this chunk's slab: a lane holds columns 16 db + 4 g + 0..3 of key 16 kb + r
  if (RESTAGE) return;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int t2 = wave + XA_WAVES * i;
    if (t2 < NDB * nkb) {
      const int kb = t2 / NDB, db = t2 - kb * NDB;
      const int key = 16 * kb + r, c = 16 * db + 4 * g;
      if (key < Lk && c < HD) {
        *reinterpret_cast<f32x4*>(slab + (int64_t)key * HD + c) = acck[i];
        *reinterpret_cast<f32x4*>(slab + ((int64_t)Lk + key) * HD + c) = accv[i];
      }
    }
  }
}

// dk / dv [B Lk][ld] (head h in columns h HD ..) = bf16(sum over the chunks, in chunk order, of the slabs); one thread per 4 columns
__global__ __launch_bounds__(256) void k_xattn_bwd_finish(const float* __restrict__ ws, __bf16* __restrict__ dk, int64_t lddk, __bf16* __restrict__ dv,
                                                         int64_t lddv, int64_t total, int Lk, int H, int hd, int nchunk) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int c4 = hd / 4;
  int64_t t = e;
  const int c = (int)(t % c4) * 4; t /= c4;
  const int key = (int)(t % Lk); t /= Lk;
  const int which = (int)(t & 1); t >>= 1;
  const int h = (int)(t % H);
  const int64_t b = t / H;
  const float* p = ws + (((b * H + h) * nchunk) * 2 + which) * (int64_t)Lk * hd + (int64_t)key * hd + c;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int ch = 0; ch < nchunk; ++ch) a += *reinterpret_cast<const f32x4*>(p + (int64_t)ch * 2 * Lk * hd);
  __bf16* out = which ? dv + (b * Lk + key) * lddv : dk + (b * Lk + key) * lddk;
  *reinterpret_cast<bf16x4*>(out + (int64_t)h * hd + c) = f2bf4(a);
}

// tiles per chunk and chunks per (sample, head): about XB_TARGET_WG workgroups whatever B H is, every chunk non-empty (one_tile: the
// RESTAGE kernel, hd 160 with more than 80 keys, takes one tile per chunk)
inline void bwd_chunks(int64_t BH, int N, bool one_tile, int* tpc, int* nchunk) {
  const int ntile = cdiv(N, XB_ROWS);
  int64_t n0 = one_tile ? ntile : (XB_TARGET_WG + BH - 1) / BH;
  if (n0 > ntile) n0 = ntile;
  if (n0 < 1) n0 = 1;
  *tpc = cdiv(ntile, n0);
  *nchunk = cdiv(ntile, *tpc);
}

template <int HD, bool RESTAGE>
int launch_xattn_bwd(const __bf16* q, int ldq, const __bf16* k, int ldk, const __bf16* v, int ldv, const __bf16* o, int ldo, const __bf16* d_o,
                     int lddo, const float* lse, __bf16* dq, int lddq, __bf16* dk, int lddk, __bf16* dv, int lddv, float* ws, int B, int N, int Lk,
                     int Lv, int H, float scale, hipStream_t s) {
  const size_t lds = (size_t)xb_layout<HD, RESTAGE>(Lk).total * sizeof(__bf16);
  if (lds > 160 * 1024) return SFRON_ERR_UNSUPPORTED;
  if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_xattn_bwd<HD, RESTAGE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds) != hipSuccess)
    return (int)hipGetLastError();
  int tpc, nchunk;
  bwd_chunks((int64_t)B * H, N, RESTAGE, &tpc, &nchunk);
  hipLaunchKernelGGL((k_xattn_bwd<HD, RESTAGE>), dim3((unsigned)((int64_t)B * H * nchunk)), dim3(XA_WAVES * 64), lds, s, q, (int64_t)ldq, k,
                     (int64_t)ldk, v, (int64_t)ldv, o, (int64_t)ldo, d_o, (int64_t)lddo, lse, dq, (int64_t)lddq, ws, N, Lk, Lv, H, scale,
                     cdiv(N, XB_ROWS), nchunk, tpc);
  SFRON_LAUNCH_STATUS();
  const int64_t total = (int64_t)B * H * 2 * Lk * (HD / 4);
  hipLaunchKernelGGL(k_xattn_bwd_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ws, dk, (int64_t)lddk, dv, (int64_t)lddv, total, Lk,
                     H, HD, nchunk);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

bool xattn_shape_ok(int Lk, int hd) { return (hd == 40 || hd == 80 || hd == 160) && Lk <= XA_LMAX && Lk % 8 == 0; }

}  // namespace

extern "C" {

int sfron_xattn_fwd(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, uint16_t* o, int ldo, int B, int N,
                    int Lk, int Lv, int H, int hd, float scale, void* stream) {
  SFRON_CHECK_ARG(q && k && v && o && B > 0 && N > 0 && H > 0 && Lk > 0 && Lv > 0 && Lv <= Lk && hd > 0);
  if ((hd != 40 && hd != 80 && hd != 160) || Lk > XA_LMAX || Lk % 8 != 0) return SFRON_ERR_UNSUPPORTED;
  const int64_t C = (int64_t)H * hd;
  SFRON_CHECK_ARG(ldq >= C && ldk >= C && ldv >= C && ldo >= C && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0);
  SFRON_CHECK_ARG((((uintptr_t)q) & 15) == 0 && (((uintptr_t)k) & 15) == 0 && (((uintptr_t)v) & 15) == 0 && (((uintptr_t)o) & 7) == 0);
  SFRON_CHECK_ARG((int64_t)B * H * cdiv(N, XA_ROWS) < (1ll << 31) && (int64_t)B * N < (1ll << 31));   // grid; offsets in the kernel are 64-bit
  const __bf16 *qb = (const __bf16*)q, *kb = (const __bf16*)k, *vb = (const __bf16*)v;
  hipStream_t s = (hipStream_t)stream;
  if (hd == 40) return launch_xattn<40, false>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, nullptr, B, N, Lk, Lv, H, scale, s);
  if (hd == 80) return launch_xattn<80, false>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, nullptr, B, N, Lk, Lv, H, scale, s);
  return launch_xattn<160, false>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, nullptr, B, N, Lk, Lv, H, scale, s);
}

int sfron_xattn_fwd_lse(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, uint16_t* o, int ldo, int B, int N,
                        int Lk, int Lv, int H, int hd, float scale, float* lse, void* stream) {
  SFRON_CHECK_ARG(q && k && v && o && lse && B > 0 && N > 0 && H > 0 && Lk > 0 && Lv > 0 && Lv <= Lk && hd > 0);
  if (!xattn_shape_ok(Lk, hd)) return SFRON_ERR_UNSUPPORTED;
  const int64_t C = (int64_t)H * hd;
  SFRON_CHECK_ARG(ldq >= C && ldk >= C && ldv >= C && ldo >= C && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0);
  SFRON_CHECK_ARG((((uintptr_t)q) & 15) == 0 && (((uintptr_t)k) & 15) == 0 && (((uintptr_t)v) & 15) == 0 && (((uintptr_t)o) & 7) == 0 &&
                  (((uintptr_t)lse) & 3) == 0);
  SFRON_CHECK_ARG((int64_t)B * H * cdiv(N, XA_ROWS) < (1ll << 31) && (int64_t)B * N < (1ll << 31));   // grid; offsets in the kernel are 64-bit
  const __bf16 *qb = (const __bf16*)q, *kb = (const __bf16*)k, *vb = (const __bf16*)v;
  hipStream_t s = (hipStream_t)stream;
  if (hd == 40) return launch_xattn<40, true>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, lse, B, N, Lk, Lv, H, scale, s);
  if (hd == 80) return launch_xattn<80, true>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, lse, B, N, Lk, Lv, H, scale, s);
  return launch_xattn<160, true>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, lse, B, N, Lk, Lv, H, scale, s);
}

int64_t sfron_xattn_bwd_ws_bytes(int B, int N, int Lk, int H, int hd) {
  if (B <= 0 || N <= 0 || Lk <= 0 || H <= 0 || hd <= 0) return 0;
  int tpc, nchunk;
  bwd_chunks((int64_t)B * H, N, hd == 160 && Lk > 80, &tpc, &nchunk);
  return (int64_t)B * H * nchunk * 2 * Lk * hd * (int64_t)sizeof(float);
}

int sfron_xattn_bwd(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, const uint16_t* o, int ldo,
                    const uint16_t* d_o, int ldd_o, const float* lse, uint16_t* dq, int lddq, uint16_t* dk, int lddk, uint16_t* dv, int lddv, int B,
                    int N, int Lk, int Lv, int H, int hd, float scale, void* ws, int64_t ws_bytes, void* stream) {
  SFRON_CHECK_ARG(q && k && v && o && d_o && lse && dq && dk && dv && ws && B > 0 && N > 0 && H > 0 && Lk > 0 && Lv > 0 && Lv <= Lk && hd > 0);
  if (!xattn_shape_ok(Lk, hd)) return SFRON_ERR_UNSUPPORTED;
  const int64_t C = (int64_t)H * hd;
  SFRON_CHECK_ARG(ldq >= C && ldk >= C && ldv >= C && ldo >= C && ldd_o >= C && lddq >= C && lddk >= C && lddv >= C);
  SFRON_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && ldd_o % 8 == 0 && lddq % 4 == 0 && lddk % 4 == 0 && lddv % 4 == 0);
  SFRON_CHECK_ARG(((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)o) | ((uintptr_t)d_o) | ((uintptr_t)ws)) & 15) == 0);
  SFRON_CHECK_ARG(((((uintptr_t)dq) | ((uintptr_t)dk) | ((uintptr_t)dv)) & 7) == 0 && (((uintptr_t)lse) & 3) == 0);
  SFRON_CHECK_ARG(ws_bytes >= sfron_xattn_bwd_ws_bytes(B, N, Lk, H, hd));
  // grids and row counts; offsets in the kernels are 64-bit
  SFRON_CHECK_ARG((int64_t)B * H * cdiv(N, XB_ROWS) < (1ll << 31) && (int64_t)B * N < (1ll << 31) && (int64_t)B * H * 2 * Lk * (hd / 4) < (1ll << 39));
  const __bf16 *qb = (const __bf16*)q, *kb = (const __bf16*)k, *vb = (const __bf16*)v, *ob = (const __bf16*)o, *gb = (const __bf16*)d_o;
  __bf16 *dqb = (__bf16*)dq, *dkb = (__bf16*)dk, *dvb = (__bf16*)dv;
  hipStream_t s = (hipStream_t)stream;
  if (hd == 40)
    return launch_xattn_bwd<40, false>(qb, ldq, kb, ldk, vb, ldv, ob, ldo, gb, ldd_o, lse, dqb, lddq, dkb, lddk, dvb, lddv, (float*)ws, B, N, Lk, Lv, H, scale, s);
  if (hd == 80)
    return launch_xattn_bwd<80, false>(qb, ldq, kb, ldk, vb, ldv, ob, ldo, gb, ldd_o, lse, dqb, lddq, dkb, lddk, dvb, lddv, (float*)ws, B, N, Lk, Lv, H, scale, s);
  if (Lk <= 80)
    return launch_xattn_bwd<160, false>(qb, ldq, kb, ldk, vb, ldv, ob, ldo, gb, ldd_o, lse, dqb, lddq, dkb, lddk, dvb, lddv, (float*)ws, B, N, Lk, Lv, H, scale, s);
  return launch_xattn_bwd<160, true>(qb, ldq, kb, ldk, vb, ldv, ob, ldo, gb, ldd_o, lse, dqb, lddq, dkb, lddk, dvb, lddv, (float*)ws, B, N, Lk, Lv, H, scale, s);
}

}  // extern "C"
