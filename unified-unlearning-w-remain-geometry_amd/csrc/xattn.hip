// Fused cross-attention forward for inference (the sampling loop of sfron.ddim): O = softmax(scale Q K^T) V per (sample, head) with at
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

template <int HD>
__global__ __launch_bounds__(XA_WAVES * 64) void k_xattn(const __bf16* __restrict__ q, int64_t ldq, const __bf16* __restrict__ k, int64_t ldk,
                                                        const __bf16* __restrict__ v, int64_t ldv, __bf16* __restrict__ o, int64_t ldo,
                                                        int N, int Lk, int Lv, int H, float scale, int ntile) {
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
    }
  }
}

template <int HD>
int launch_xattn(const __bf16* q, int ldq, const __bf16* k, int ldk, const __bf16* v, int ldv, __bf16* o, int ldo, int B, int N, int Lk, int Lv,
                 int H, float scale, hipStream_t s) {
  const int nkb = (Lk + 15) / 16, nst = (nkb + 1) / 2;
  const size_t lds = ((size_t)16 * nkb * (HD + 8) + (size_t)16 * ((HD + 15) / 16) * (32 * nst + 8)) * sizeof(__bf16);
  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per function and per device: hd 160 with more than 80 keys passes 64 KiB
  if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_xattn<HD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return (int)hipGetLastError();
  const int ntile = cdiv(N, XA_ROWS);
  hipLaunchKernelGGL(k_xattn<HD>, dim3((unsigned)((int64_t)B * H * ntile)), dim3(XA_WAVES * 64), lds, s, q, (int64_t)ldq, k, (int64_t)ldk, v,
                     (int64_t)ldv, o, (int64_t)ldo, N, Lk, Lv, H, scale, ntile);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

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
  if (hd == 40) return launch_xattn<40>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, B, N, Lk, Lv, H, scale, s);
  if (hd == 80) return launch_xattn<80>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, B, N, Lk, Lv, H, scale, s);
  return launch_xattn<160>(qb, ldq, kb, ldk, vb, ldv, (__bf16*)o, ldo, B, N, Lk, Lv, H, scale, s);
}

}  // extern "C"
