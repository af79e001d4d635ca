// BASELINE config 5: the four token GEMMs of a DiT block (DiT/models.py:108-121 forward) on the CDNA4 fp8 matrix core.
//
// Both MFMA operands must be fp8 (v_mfma_scale_f32_16x16x128_f8f6f4 has no bf16 x fp8 form, and a bf16 A tile of a 128-deep step
// would not fit a ring in LDS), so
//   weights      live as fp32 masters (the optimizer's arena) + an e4m3 shadow, one power-of-two scale per tensor
//                (scale = 2^floor(log2(224 / amax)): exact to apply and to undo, 2x headroom under the 448 maximum), re-quantised
//                after every optimizer step in ONE pass with the scale of the previous step's amax (delayed scaling: a weight moves
//                by at most lr per step) while the pass collects the new amax (integer atomicMax on the float bits: order-free);
//   activations  are quantised where they are PRODUCED, with static power-of-two scales per kind: LayerNorm+modulate writes its
//                bf16 output (the backward pass's operand) and the e4m3 copy, the fc1 epilogue writes h in bf16 and e4m3, the
//                attention output gets one cast kernel.
// The backward pass keeps bf16 operands (the quantisation is a straight-through estimator, as in oracle/fp8_ref.py) unless the caller arms
// the fp8 dgrads (sfron_aux_set_fp8_dgrad): the four input-gradient products of a block then multiply an MX-scaled e4m3 dY (one E8M0 scale
// per 32 consecutive elements of a row, sfron_cast_mx8) by a TRANSPOSED copy of the e4m3 weight shadow (sfron_fp8_transpose_shadow) on the
// same scaled MFMA, the dY scales fed per lane.  The fp8 weight gradients (sfron_aux_set_fp8_wgrad, independent of both) take dY and X MX-scaled
// along the TOKENS (k_mx8_cast_t) and multiply them on the 192 x 192 tile of k_wgrad8, both scales fed per lane.
// e4m3 = OCP e4m3fn (gfx950's v_cvt_pk_fp8_f32), round to nearest even, saturating at +-448.
//
// GEMM kernel: C[M][N] = deq * (A8[M][K] . B8[N][K]^T) with the 256 x 128 x 128-byte tile of tools/probes/fp8_gemm_probe.hip
// (three LDS slots, both operands staged by buffer_load ... lds with the XOR swizzle on the source address, 8 waves of 32 x 128;
// exact-integer verified there), plus the epilogues the block needs: bias -> bf16 (qkv); bias, GELU-tanh, pre-activation + bf16 + e4m3
// outputs (fc1); bias, gate, residual -> fp32 stream + bf16 branch output (proj, fc2).
#include "common.h"
#include <string.h>
#include "../../include/sfron.h"
#include <atomic>

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((address_space(3))) void lptr8_t;

constexpr int TPB = 256;

// ---- how much of the e4m3 range the ACTIVATIONS use: the activation scales are static (engine.py: 8 / 32 / 16), the conversion saturates, and
// nothing else would tell a run on real weights that its LN + modulate outputs left the range.  Every kernel that quantises an activation
// keeps the maximum of |x * scale| per thread (one v_max per value), a wave reduces it and ONE lane per wave raises the site's word with
// atomicMax on the bit pattern (non-negative floats order like unsigned integers).  sfron_fp8_activation_amax reads (and resets) the three
// words: a value above 448 means that values were clipped since the last reset.  The three words belong to the CALLER (round 6: a device
// array handed to every quantising entry point, NULL = no tracking; rounds 4-5 kept them in a __device__ global of the library).
// site 0 = LN + modulate output (the A operand of qkv / fc1), 1 = sfron_cast_e4m3 (attention output -> proj), 2 = GELU output (-> fc2)
__device__ __forceinline__ void amax4(float& m, float a, float b, float c, float d) {
  m = fmaxf(m, fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d))));
}
__device__ __forceinline__ void amax_report(unsigned int* words, int site, float m) {
  if (!words) return;                          // kernel-uniform
  m = wave_max(m);
  // the atomic only when this wave would RAISE the word: thousands of waves hitting one address serialise in L2 (the unconditional form cost
  // config 5 six ms per step); a stale read of the word can only cause a surplus atomic, never a lost maximum
  if ((threadIdx.x & 63) == 0 && m > __uint_as_float(__builtin_nontemporal_load(&words[site])))
    atomicMax(&words[site], __float_as_uint(m));
}

// ---- MX (block-scaled) e4m3 of a dY operand: one E8M0 byte per 32 consecutive elements of a row (include/sfron.h states the rule).
// X = ceil(log2(amax / 448)) from the exponent of amax: amax = f 2^e, f in [0.5, 1), 448 = 0.875 2^9 -> X = e - 9 if f <= 0.875, else e - 8
// (exact: no division, no log); clamped to [-127, 127], an all-zero block gets -127, an infinite amax 127 (the clamp of +inf).  The element
// is e4m3(x 2^-X): |x 2^-X| <= 448.  X <= 120 for any finite bf16 amax; 2^-X is built from its bits, 2^-127 as the subnormal it is.  Blocks
// holding a NaN are outside the rule (fmaxf drops the NaN from amax; the NaN itself converts to an e4m3 NaN).
__device__ __forceinline__ int mx_exp(float amax) {
  if (!(amax > 0.f)) return -127;
  if (isinf(amax)) return 127;
  int e;
  const float f = frexpf(amax, &e);
  const int x = f <= 0.875f ? e - 9 : e - 8;
  return x < -127 ? -127 : (x > 127 ? 127 : x);
}
__device__ __forceinline__ float mx_inv(int x) {                                                                  // 2^-x, x in [-127, 127]
  return x < 127 ? __uint_as_float((uint32_t)(127 - x) << 23) : __uint_as_float(0x00400000u);
}
__device__ __forceinline__ float amax4v(f32x4 v) { return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))); }

// ---------------------------------------------------------------- weights: per-tensor amax / quantisation
struct TensorRange { long long off, n; };   // element range of one tensor inside the arena (off, n multiples of 8)

// mode 0: amax only.  mode 1: dst = e4m3(p * scale[t]) AND amax.  grid (chunks, tensors)
__global__ __launch_bounds__(TPB) void k_fp8_quant_tensors(const float* __restrict__ p, const TensorRange* __restrict__ tab,
                                                           const float* __restrict__ scales, unsigned* __restrict__ amax_bits,
                                                           uint8_t* __restrict__ dst, int mode) {
  const int t = blockIdx.y;
  const TensorRange r = tab[t];
  const float s = mode ? scales[t] : 1.0f;
  const float4* src = reinterpret_cast<const float4*>(p + r.off);
  uint32_t* out = reinterpret_cast<uint32_t*>(dst + r.off);
  const long long n4 = r.n >> 2;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n4; i += (long long)gridDim.x * TPB) {
    const float4 v = src[i];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    if (mode) out[i] = pack_e4m3(v.x * s, v.y * s, v.z * s, v.w * s);
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(amax_bits + t, __float_as_uint(m));   // non-negative floats order like their bits
}

// scale = 2^floor(log2(224 / amax)) (1 for an all-zero tensor); amax is cleared for the next pass
__global__ void k_fp8_update_scales(unsigned* __restrict__ amax_bits, int n, float* __restrict__ scales) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float a = __uint_as_float(amax_bits[t]);
  float s = 1.0f;
  if (a > 0.f && isfinite(a)) {
    int e;
    (void)frexpf(224.0f / a, &e);            // 224 / a = f * 2^e, f in [0.5, 1)  ->  floor(log2) = e - 1
    e -= 1;
    e = e < -60 ? -60 : (e > 60 ? 60 : e);
    s = ldexpf(1.0f, e);
  }
  scales[t] = s;
  amax_bits[t] = 0u;
}

__global__ __launch_bounds__(TPB) void k_cast_e4m3_bf16(const __bf16* __restrict__ src, int64_t n, float scale, uint8_t* __restrict__ dst, unsigned int* amax) {
  const int64_t n8 = n >> 3;
  float am = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n8; i += (int64_t)gridDim.x * TPB) {
    const bf16x8 v = reinterpret_cast<const bf16x8*>(src)[i];
    const float f0 = bf2f(v[0]) * scale, f1 = bf2f(v[1]) * scale, f2 = bf2f(v[2]) * scale, f3 = bf2f(v[3]) * scale;
    const float f4 = bf2f(v[4]) * scale, f5 = bf2f(v[5]) * scale, f6 = bf2f(v[6]) * scale, f7 = bf2f(v[7]) * scale;
    amax4(am, f0, f1, f2, f3); amax4(am, f4, f5, f6, f7);
    uint2 o;
    o.x = pack_e4m3(f0, f1, f2, f3);
    o.y = pack_e4m3(f4, f5, f6, f7);
    reinterpret_cast<uint2*>(dst)[i] = o;
  }
  amax_report(amax, 1, am);
}
__global__ __launch_bounds__(TPB) void k_cast_e4m3_f32(const float* __restrict__ src, int64_t n, float scale, uint8_t* __restrict__ dst, unsigned int* amax) {
  const int64_t n4 = n >> 2;
  float am = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * TPB) {
    const float4 v = reinterpret_cast<const float4*>(src)[i];
    amax4(am, v.x * scale, v.y * scale, v.z * scale, v.w * scale);
    reinterpret_cast<uint32_t*>(dst)[i] = pack_e4m3(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
  }
  amax_report(amax, 1, am);
}

// bf16 [n] (rows of N, N % 32 == 0: the flat index of a 32-block is its scale's index in [M][N / 32]) -> MX e4m3 + E8M0 bytes.  Eight elements
// per lane, a block = the four lanes of a DPP quad (the grid-stride loop keeps quads together: n / 8 is a multiple of 4)
__global__ __launch_bounds__(TPB) void k_cast_mx8(const __bf16* __restrict__ src, int64_t n, uint8_t* __restrict__ dst, uint8_t* __restrict__ sc) {
  const int64_t n8 = n >> 3;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n8; i += (int64_t)gridDim.x * TPB) {
    const bf16x8 v = reinterpret_cast<const bf16x8*>(src)[i];
    const f32x4 a = {bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])}, b = {bf2f(v[4]), bf2f(v[5]), bf2f(v[6]), bf2f(v[7])};
    float am = fmaxf(amax4v(a), amax4v(b));
    am = fmaxf(am, dpp_get<0xB1, 0xf>(am));       // quad_perm [1,0,3,2]
    am = fmaxf(am, dpp_get<0x4E, 0xf>(am));       // quad_perm [2,3,0,1]: the block's amax in all four lanes
    const int x = mx_exp(am);
    const float s = mx_inv(x);
    uint2 o;
    o.x = pack_e4m3(a[0] * s, a[1] * s, a[2] * s, a[3] * s);
    o.y = pack_e4m3(b[0] * s, b[1] * s, b[2] * s, b[3] * s);
    reinterpret_cast<uint2*>(dst)[i] = o;
    if ((i & 3) == 0) sc[i >> 2] = (uint8_t)(x + 127);
  }
}

// e4m3 weight shadow -> its transpose: dst[dst_off + c * R + r] = src[src_off + r * C + c] for every matrix of the table (rows of four int64:
// src_off, dst_off, R, C; offsets, R and C multiples of 8 -- a row that is not is skipped).  64 x 64-byte tiles through LDS: 8-byte loads
// along the source rows, 8-byte stores along the destination rows.  grid (workgroups per matrix, matrices)
__global__ __launch_bounds__(TPB) void k_fp8_transpose_shadow(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const int64_t* __restrict__ tab) {
  __shared__ uint8_t tile[64][64 + 8];
  const int64_t* t = tab + 4 * blockIdx.y;
  const int64_t so = t[0], dof = t[1], R = t[2], C = t[3];
  if (((so | dof | R | C) & 7) != 0 || R <= 0 || C <= 0) return;            // workgroup-uniform
  const int64_t tr = (R + 63) >> 6, tc = (C + 63) >> 6;
  for (int64_t tile_i = blockIdx.x; tile_i < tr * tc; tile_i += gridDim.x) {
    const int64_t r0 = (tile_i / tc) * 64, c0 = (tile_i % tc) * 64;
    __syncthreads();                                                         // the previous tile's readers are done
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = threadIdx.x + TPB * j, rr = idx >> 3, ch = (idx & 7) * 8;
      uint2 v = make_uint2(0u, 0u);
      if (r0 + rr < R && c0 + ch < C) v = *reinterpret_cast<const uint2*>(src + so + (r0 + rr) * C + c0 + ch);
      *reinterpret_cast<uint2*>(&tile[rr][ch]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = threadIdx.x + TPB * j, cc = idx >> 3, rc = (idx & 7) * 8;
      if (c0 + cc < C && r0 + rc < R) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          lo |= (uint32_t)tile[rc + k][cc] << (8 * k);
          hi |= (uint32_t)tile[rc + 4 + k][cc] << (8 * k);
        }
        *reinterpret_cast<uint2*>(dst + dof + (c0 + cc) * R + r0 + rc) = make_uint2(lo, hi);
      }
    }
  }
}

// bf16 src [M][W] -> MX e4m3 of its TRANSPOSE: dst [W][M] + scales [W][M / 32] (= k_cast_mx8 of src^T bit for bit: the same amax, exponent,
// multiply and conversion).  One workgroup per 32-token x 256-column tile: 16-byte loads along the source rows into an fp32 LDS image, then
// one thread per column takes its 32 values (stride 257: conflict-free), their amax, and stores its 32 codes as two 16-byte pieces and one
// scale byte.  grid (M / 32, ceil(W / 256)); M % 32 == 0, W % 8 == 0.
__global__ __launch_bounds__(TPB) void k_mx8_cast_t(const __bf16* __restrict__ src, int M, int W, uint8_t* __restrict__ dst,
                                                     uint8_t* __restrict__ sc) {
  __shared__ float tile[32][TPB + 1];
  const int m0 = blockIdx.x * 32, w0 = blockIdx.y * TPB, t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = t + TPB * j, r = c >> 5, c8 = (c & 31) * 8;
    if (w0 + c8 < W) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (size_t)(m0 + r) * W + w0 + c8);
#pragma unroll
      for (int i = 0; i < 8; ++i) tile[r][c8 + i] = bf2f(v[i]);
    }
  }
  __syncthreads();
  const int w = w0 + t;
  if (w >= W) return;
  float v[32];
  float am = 0.f;
#pragma unroll
  for (int r = 0; r < 32; ++r) { v[r] = tile[r][t]; am = fmaxf(am, fabsf(v[r])); }
  const int x = mx_exp(am);
  const float s = mx_inv(x);
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = pack_e4m3(v[4 * i] * s, v[4 * i + 1] * s, v[4 * i + 2] * s, v[4 * i + 3] * s);
  uint4* const d = reinterpret_cast<uint4*>(dst + (size_t)w * M + m0);
  d[0] = make_uint4(o[0], o[1], o[2], o[3]);
  d[1] = make_uint4(o[4], o[5], o[6], o[7]);
  sc[(size_t)w * (M >> 5) + (m0 >> 5)] = (uint8_t)(x + 127);
}

// ---------------------------------------------------------------- LayerNorm + modulate with the e4m3 copy (norm.hip's k_ln_mod_fwd + one store)
constexpr int NCHQ = 5;            // row chunks of 256 floats: D <= 1280
// (as norm.hip k_ln_mod_fwd: one-row buffer descriptors -- branch-free --, RPW rows of one sample per wave, every load before the first use,
// the sample's shift / scale rows fetched once per wave)
typedef unsigned int q_u32x2 __attribute__((ext_vector_type(2)));
template <int RPW>
__global__ __launch_bounds__(TPB) void k_ln_mod_fwd_q(const float* __restrict__ x, const float* __restrict__ shift,
                                                      const float* __restrict__ scale, int ldmod, int T, int M, int D,
                                                      __bf16* __restrict__ out, uint8_t* __restrict__ out8, float s8,
                                                      float* __restrict__ mean_out, float* __restrict__ rstd_out, unsigned int* amax) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = (blockIdx.x * 4 + wave) * RPW;
  if (row0 >= M) return;
  float am = 0.f;
  float4 v[RPW][NCHQ], sh[NCHQ], sc[NCHQ];
  {
    const int b = row0 / T;
    const __amdgpu_buffer_rsrc_t rh = row_rsrc(shift + (size_t)b * ldmod, D * 4), rc = row_rsrc(scale + (size_t)b * ldmod, D * 4);
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      const int row = row0 + k < M ? row0 + k : M - 1;
      const __amdgpu_buffer_rsrc_t rx = row_rsrc(x + (size_t)row * D, D * 4);
#pragma unroll
      for (int i = 0; i < NCHQ; ++i) v[k][i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, lane * 16 + 1024 * i, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < NCHQ; ++i) {
      sh[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rh, lane * 16 + 1024 * i, 0, 0));
      sc[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rc, lane * 16 + 1024 * i, 0, 0));
    }
  }
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int row = row0 + k;
    if (row >= M) break;                           // wave-uniform
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCHQ; ++i) s += v[k][i].x + v[k][i].y + v[k][i].z + v[k][i].w;      // zeros past the row end
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCHQ; ++i) {
      const float live = lane + 64 * i < (D >> 2) ? 1.0f : 0.0f;
      const float a = v[k][i].x - mean, b = v[k][i].y - mean, c = v[k][i].z - mean, d = v[k][i].w - mean;
      q += live * (a * a + b * b + c * c + d * d);
    }
    const float var = wave_sum(q) / (float)D;
    const float rstd = 1.0f / sqrtf(var + 1e-6f);
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    const __amdgpu_buffer_rsrc_t ro = row_rsrc(out + (size_t)row * D, D * 2), r8 = row_rsrc(out8 + (size_t)row * D, D);
#pragma unroll
    for (int i = 0; i < NCHQ; ++i) {
      const float4 h = sh[i], g = sc[i];
      const float o0 = (v[k][i].x - mean) * rstd * (1.0f + g.x) + h.x, o1 = (v[k][i].y - mean) * rstd * (1.0f + g.y) + h.y;
      const float o2 = (v[k][i].z - mean) * rstd * (1.0f + g.z) + h.z, o3 = (v[k][i].w - mean) * rstd * (1.0f + g.w) + h.w;
      const bf16x4 o = {f2bf(o0), f2bf(o1), f2bf(o2), f2bf(o3)};
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(q_u32x2, o), ro, lane * 8 + 512 * i, 0, 0);
      if (lane + 64 * i < (D >> 2)) amax4(am, o0 * s8, o1 * s8, o2 * s8, o3 * s8);        // (lanes past the row end hold the shift, not data)
      __builtin_amdgcn_raw_buffer_store_b32(pack_e4m3(o0 * s8, o1 * s8, o2 * s8, o3 * s8), r8, lane * 4 + 256 * i, 0, 0);
    }
  }
  amax_report(amax, 0, am);
}

// ---------------------------------------------------------------- fp8 x fp8 GEMM
struct Gemm8Args {
  const uint8_t* A; const uint8_t* B;     // [M][K], [N][K] e4m3
  int M, N, K;
  const float* w_scale;                   // device scalar: the weight tensor's quantisation scale
  float a_scale;                          // the activation's (static)
  const float* bias;                      // [N] fp32 or null
  __bf16* Cb; int ldcb;                   // bf16 output (EPI_BF16: result; EPI_GELU: gelu(result))
  __bf16* aux; int ldaux;                 // EPI_GELU: pre-activation; EPI_GATE_RES: branch output
  uint8_t* C8; float c8_scale;            // EPI_GELU: e4m3(gelu(result) * c8_scale) -- the A operand of fc2
  float* Cf; int ldcf; const float* resid;      // EPI_GATE_RES: Cf = resid + gate * result
  const float* gate; int ldgate; int T;
  unsigned int* act_amax;                 // the caller's activation-range words (site 2 is raised by EPI_GELU's e4m3 output), or null
  int aux_q;                              // EPI_GELU: aux = GELU'(pre-activation) as one byte per element (common.h geluq_pack4), uint8 [M][ldaux]
                                          // E8_DG_GELU: aux holds those codes (aux_q = 1) or the bf16 pre-activation
  const uint8_t* a_sc;                    // E8_DG_*: A's E8M0 scales [M][K / 32] (MX dY)
  uint8_t* c8_sc;                         // E8_DG_GELU: the MX copy of Cb goes to C8 [M][N] + c8_sc [M][N / 32]
  float* colpart;                         // E8_DG_GELU: [M / 256][N] column sums of each tile row's result (fp32), or null
};
// E8_DG_BF16 / E8_DG_GELU: the dgrad form -- A = MX e4m3 dY with one scale byte per lane and 32-block, B = the transposed weight shadow
enum { E8_BF16 = 0, E8_GELU = 2, E8_GATE_RES = 3, E8_DG_BF16 = 4, E8_DG_GELU = 5 };

constexpr int FBM = 256, BKB = 128, NW = 8, NSLOT8 = 3;
constexpr int A_BYTES = FBM * BKB, NA = FBM * 8 / 64 / NW;
// NTL = 16-column n-tiles per workgroup tile: 8 (256 x 128) or 9 (256 x 144 -- a [8192 x 1152] output is then exactly 256 tiles, as
// for the bf16 kernels; its 18 B-tile DMA instructions do not divide by the 8 waves: the waves without a third share send theirs
// through a zero-length descriptor to a dummy LDS kilobyte, so every wave issues the same number and the counted vmcnt waits hold)
template <int NTL> struct Tile8 {
  static constexpr int FBN = NTL * 16, B_BYTES = FBN * BKB, SLOT = A_BYTES + B_BYTES;
  static constexpr int NB_TOTAL = FBN * 8 / 64, NB = (NB_TOTAL + NW - 1) / NW, NDMA = NA + NB;
  static constexpr bool EVEN = NB_TOTAL % NW == 0;
  static constexpr size_t LDS = (size_t)NSLOT8 * SLOT + (EVEN ? 0 : 1024);
};

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// one dword per lane (LDS: lane * 4 from dst)
__device__ __forceinline__ void dma4b(__amdgpu_buffer_rsrc_t rsrc, uint8_t* dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr8_t*)dst, 4, voff, soff, 0, 0);
}
__device__ __forceinline__ void dma16b(__amdgpu_buffer_rsrc_t rsrc, uint8_t* dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr8_t*)dst, 16, voff, soff, 0, 0);
}
// 32 consecutive k-bytes of row `row`, k group g: chunks 2g and 2g + 1 of the 128-byte row, chunk ^= row & 7
__device__ __forceinline__ i32x8 frag32(const uint8_t* img, int row, int g) {
  const i32x4 lo = *reinterpret_cast<const i32x4*>(img + row * 128 + (((2 * g) ^ (row & 7)) << 4));
  const i32x4 hi = *reinterpret_cast<const i32x4*>(img + row * 128 + (((2 * g + 1) ^ (row & 7)) << 4));
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// The 16x16x128 f8 MFMA takes lane group g's 32 bytes as k = 16 g .. 16 g + 15 (first four registers) and 64 + 16 g .. 64 + 16 g + 15 (last
// four), and its per-lane scale of group j covers k = 32 j .. 32 j + 31 (measured: tests/test_gpu_fp8_backward.py lane-map test).  frag32's
// chunks 2g, 2g + 1 are a consistent K permutation -- harmless with unit scales -- but would put two 32-blocks under one scale; the MX form
// loads chunks g and g + 4 so that the matrix core's k IS the memory k and group j's scale byte is that of the row's 32-block j.
__device__ __forceinline__ i32x8 frag32_mx(const uint8_t* img, int row, int g) {
  const i32x4 lo = *reinterpret_cast<const i32x4*>(img + row * 128 + ((g ^ (row & 7)) << 4));
  const i32x4 hi = *reinterpret_cast<const i32x4*>(img + row * 128 + (((g + 4) ^ (row & 7)) << 4));
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

}  // namespace

// NL > 0: NL extra LOADER waves issue every LDS-DMA piece of the ring; the eight multiplying waves none (as csrc/gemm.hip k_gemm_pipe NL;
// tools/probes/persist_gemm_probe.hip measured this compiler-scheduled loop 13-22 % faster that way in bf16).  Twelve waves: <= 168
// registers, so the consumers fetch the bias after the main loop.  With e4m3 operands a K-step carries half the DMA pieces per FLOP
// and the split bought nothing in the step (g_fp8_loader_waves): kept as a switchable form, off by default.
template <int EPI, int NTL, int NL = 0>
__global__ __launch_bounds__(512 + 64 * NL) void k_gemm8(Gemm8Args g) {
  using TL = Tile8<NTL>;
  // dgrad form: a slot also holds the A tile's scale bytes, [256 rows][4 32-blocks], sent by waves 0..3 (one dword per lane and row); waves
  // 4..7 send theirs through the zero-length descriptor to the dummy kilobyte, so every wave issues NDMA8 pieces per k-step
  constexpr bool MX = EPI == E8_DG_BF16 || EPI == E8_DG_GELU;
  static_assert(!MX || NL == 0, "dgrad form: shared-wave tiles only");
  static_assert(EPI != E8_DG_GELU || NTL == 8, "MX output: 32-blocks must not straddle tiles");
  constexpr int FBN = TL::FBN, SLOT = TL::SLOT + (MX ? 1024 : 0), NT8 = NTL;
  constexpr int NWD = NL > 0 ? NL : NW;                                  // waves that issue LDS-DMA
  constexpr int NA_ = FBM * 8 / 64 / NWD, NB = (TL::NB_TOTAL + NWD - 1) / NWD, NDMA8 = NA_ + NB + (MX ? 1 : 0);
  constexpr bool EVEN_ = TL::NB_TOTAL % NWD == 0;
  constexpr size_t DUMMY_AT = (size_t)NSLOT8 * SLOT;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem8[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = g.N / FBN;
  int id;
  {
    const int nblk = gridDim.x, b = blockIdx.x, q = nblk >> 3, r = nblk & 7, x = b & 7, y = b >> 3;
    id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + y;
  }
  const int tm = id / ntn, tn = id - tm * ntn, m0 = tm * FBM, n0 = tn * FBN;
  const int K = g.K, nk = K / BKB;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, g.M * K, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)g.B, 0, g.N * K, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsNull = __builtin_amdgcn_make_buffer_rsrc((void*)g.B, 0, 0, 0x00020000);
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t rsS =
      __builtin_amdgcn_make_buffer_rsrc((void*)(MX ? g.a_sc : g.B), 0, MX ? g.M * (K >> 5) : 0, 0x00020000);
  uint8_t* const dummy = smem8 + DUMMY_AT;
  const int lc16 = ((lane & 7) ^ ((lane >> 3) & 7)) << 4;
  const int dwave = NL > 0 ? wave - NW : wave;                       // (consumers of the loader form never use their plan)
  int a_off[NA_], b_off[NB];
#pragma unroll
  for (int i = 0; i < NA_; ++i) a_off[i] = (m0 + (dwave + i * NWD) * 8 + (lane >> 3)) * K + lc16;
#pragma unroll
  for (int i = 0; i < NB; ++i) b_off[i] = (n0 + (dwave + i * NWD) * 8 + (lane >> 3)) * K + lc16;
  [[maybe_unused]] const int s_off = (m0 + (dwave & 3) * 64 + lane) * (K >> 5);
  auto issue = [&](int slot, int k0) {
    uint8_t* iA = smem8 + slot * SLOT;
    uint8_t* iB = iA + A_BYTES;
#pragma unroll
    for (int i = 0; i < NA_; ++i) dma16b(rsA, iA + (dwave + i * NWD) * 1024, a_off[i], k0);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      if constexpr (EVEN_) dma16b(rsB, iB + (dwave + i * NWD) * 1024, b_off[i], k0);
      else {
        const bool ok = dwave + i * NWD < TL::NB_TOTAL;             // wave-uniform
        dma16b(ok ? rsB : rsNull, ok ? iB + (dwave + i * NWD) * 1024 : dummy, b_off[i], k0);
      }
    }
    if constexpr (MX) {
      if (dwave < 4) dma4b(rsS, iB + TL::B_BYTES + dwave * 256, s_off, k0 >> 5);     // wave-uniform
      else dma4b(rsNull, dummy, 0, 0);
    }
  };
  if constexpr (NL > 0) {
    if (wave >= NW) {                                                // ---- loader wave
      if (nk > 0) issue(0, 0);
      if (nk > 1) issue(1, BKB);
      int slot2 = 2;
      for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) wait_vm<NDMA8>(); else wait_vm<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + 2 < nk) issue(slot2, (kt + 2) * BKB);
        slot2 = slot2 == 2 ? 0 : slot2 + 1;
      }
      return;
    }
  }
  f32x4 acc[2][NT8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NT8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fg = lane >> 4;
  // this lane's output columns: bias fetched ahead of the main loop (loader form: behind it, the registers are short)
  float4 bias_v[NT8];
  auto load_bias = [&]() {
#pragma unroll
    for (int nt = 0; nt < NT8; ++nt)
      bias_v[nt] = g.bias ? *reinterpret_cast<const float4*>(g.bias + n0 + nt * 16 + 4 * fg) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  if constexpr (NL == 0 && !MX) load_bias();
  const float deq = 1.0f / (g.a_scale * *g.w_scale);
  if constexpr (NL == 0) {
    if (nk > 0) issue(0, 0);
    if (nk > 1) issue(1, BKB);
  }
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if constexpr (NL == 0) { if (kt + 1 < nk) wait_vm<NDMA8>(); else wait_vm<0>(); }
    __builtin_amdgcn_s_barrier();
    if constexpr (NL == 0) { if (kt + 2 < nk) issue(slot >= 1 ? slot - 1 : 2, (kt + 2) * BKB); }
    const uint8_t* iA = smem8 + slot * SLOT;
    const uint8_t* iB = iA + A_BYTES;
    if constexpr (MX) {
      // this lane's scale operand: the E8M0 byte of 32-block fg of rows wave * 32 + fr (+ 16)
      const i32x8 fa0 = frag32_mx(iA, wave * 32 + fr, fg), fa1 = frag32_mx(iA, wave * 32 + 16 + fr, fg);
      const uint8_t* iS = iB + TL::B_BYTES;
      const int sa0 = iS[(wave * 32 + fr) * 4 + fg], sa1 = iS[(wave * 32 + 16 + fr) * 4 + fg];
#pragma unroll
      for (int nt = 0; nt < NT8; ++nt) {
        const i32x8 fb = frag32_mx(iB, nt * 16 + fr, fg);
        acc[0][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb, fa0, acc[0][nt], 0, 0, 0, 127, 0, sa0);
        acc[1][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb, fa1, acc[1][nt], 0, 0, 0, 127, 0, sa1);
      }
    } else {
    const i32x8 fa0 = frag32(iA, wave * 32 + fr, fg), fa1 = frag32(iA, wave * 32 + 16 + fr, fg);
#pragma unroll
    for (int nt = 0; nt < NT8; ++nt) {
      const i32x8 fb = frag32(iB, nt * 16 + fr, fg);
      // cbsz = blgp = 0: both operands e4m3; block scales 2^(127 - 127) = 1 (the tensor scales are undone in the epilogue)
      acc[0][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb, fa0, acc[0][nt], 0, 0, 0, 127, 0, 127);
      acc[1][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb, fa1, acc[1][nt], 0, 0, 0, 127, 0, 127);
    }
    }
    slot = slot == 2 ? 0 : slot + 1;
  }
  constexpr bool BIAS_BY_HALF = NL > 0 && EPI == E8_GATE_RES;       // (that epilogue also holds gate + residual words: bias with them, half a row at a time)
  if constexpr (NL > 0 && !BIAS_BY_HALF) load_bias();
  // lane holds C[m0 + 32 wave + 16 mt + fr][n0 + 16 nt + 4 fg .. +3]
  if constexpr (EPI == E8_DG_GELU) {
    // fc2 dgrad * GELU' (as csrc/gemm.hip EPI_DGELU / EPI_DGELUQ): d_hpre in bf16, its MX e4m3 copy quantised from the bf16-ROUNDED values
    // (= sfron_cast_mx8 of the bf16 output, bit for bit), and the column sums of the fp32 values per tile row (fc1.bias gradient partials).
    // A 32-block of a row = tiles 2 np, 2 np + 1 of the four lanes fg that hold that row.
    const int colp = n0 + pair_col(fg);
    f32x4 cs[NT8];
#pragma unroll
    for (int nt = 0; nt < NT8; ++nt) cs[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int row = m0 + wave * 32 + mt * 16 + fr;
      f32x4 gp[NT8];
      if (g.aux_q) {                                                          // kernel-uniform
        const uint8_t* const aq = reinterpret_cast<const uint8_t*>(g.aux) + (size_t)row * g.ldaux;
#pragma unroll
        for (int np = 0; np < NT8 / 2; ++np) {
          unsigned a, b;
          pair_unpack8(*reinterpret_cast<const uint2*>(aq + colp + np * 32), a, b);
          gp[2 * np] = geluq_unpack4(a); gp[2 * np + 1] = geluq_unpack4(b);
        }
      } else {
        const __bf16* const ap = g.aux + (size_t)row * g.ldaux + n0 + 4 * fg;
#pragma unroll
        for (int nt = 0; nt < NT8; ++nt) gp[nt] = gelu_tanh_grad4(bf2f4(*reinterpret_cast<const bf16x4*>(ap + nt * 16)));
      }
      bf16x4 ob[NT8];
      unsigned c8[NT8];
      unsigned scw = 0;
#pragma unroll
      for (int nt = 0; nt < NT8; ++nt) {
        const f32x4 r = (acc[mt][nt] * deq) * gp[nt];
        cs[nt] += r;
        ob[nt] = f2bf4(r);
      }
#pragma unroll
      for (int np = 0; np < NT8 / 2; ++np) {
        const f32x4 h0 = bf2f4(ob[2 * np]), h1 = bf2f4(ob[2 * np + 1]);
        float am = fmaxf(amax4v(h0), amax4v(h1));
        am = fmaxf(am, __shfl_xor(am, 16, 64));
        am = fmaxf(am, __shfl_xor(am, 32, 64));
        const int x = mx_exp(am);
        const float s = mx_inv(x);
        c8[2 * np] = pack_e4m3(h0[0] * s, h0[1] * s, h0[2] * s, h0[3] * s);
        c8[2 * np + 1] = pack_e4m3(h1[0] * s, h1[1] * s, h1[2] * s, h1[3] * s);
        scw |= (unsigned)(x + 127) << (8 * np);
      }
      __bf16* const r = g.Cb + (size_t)row * g.ldcb;
#pragma unroll
      for (int np = 0; np < NT8 / 2; ++np) *reinterpret_cast<uint4*>(r + colp + np * 32) = pair_pack(ob[2 * np], ob[2 * np + 1]);
      uint8_t* const r8 = g.C8 + (size_t)row * g.N;
#pragma unroll
      for (int np = 0; np < NT8 / 2; ++np) *reinterpret_cast<uint2*>(r8 + colp + np * 32) = pair_pack8(c8[2 * np], c8[2 * np + 1]);
      if (fg == 0) *reinterpret_cast<uint32_t*>(g.c8_sc + (size_t)row * (g.N >> 5) + (n0 >> 5)) = scw;
    }
    if (g.colpart) {                                                          // kernel-uniform
      // the 16 lanes that share fg hold the same 4 columns: row16_sum, then the 8 waves meet in LDS (free: every wave is past the main
      // loop after the barrier) and are added in wave order
#pragma unroll
      for (int nt = 0; nt < NT8; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[nt][j] = row16_sum(cs[nt][j]);
      __syncthreads();
      float* red = reinterpret_cast<float*>(smem8);                         // [NW][FBN]
      if (fr == 0) {
#pragma unroll
        for (int nt = 0; nt < NT8; ++nt) *reinterpret_cast<f32x4*>(red + wave * FBN + nt * 16 + 4 * fg) = cs[nt];
      }
      __syncthreads();
      for (int c = tid; c < FBN; c += NW * 64) {
        float x = red[c];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) x += red[w2 * FBN + c];
        g.colpart[(size_t)tm * g.N + n0 + c] = x;
      }
    }
    return;
  }
  [[maybe_unused]] float act_am = 0.f;          // E8_GELU: max |gelu * c8_scale| of this thread's values (g_act_amax site 2)
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int row = m0 + wave * 32 + mt * 16 + fr;
    // gated residual: the row's gate and residual words are fetched for all NT8 tiles before the first store (resid may alias Cf, so hipcc
    // keeps each load behind the previous store: one exposed latency per tile otherwise)
    // (in two halves: 2 x NT8 float4 on top of the accumulators do not fit the 168 registers of the loader form)
    constexpr int NH = (NT8 + 1) / 2;
    float4 gtv[EPI == E8_GATE_RES ? NH : 1], xrv[EPI == E8_GATE_RES ? NH : 1];
    bf16x4 ob[NT8], ab[NT8];
    unsigned c8[NT8];
    [[maybe_unused]] unsigned q8[EPI == E8_GELU ? NT8 : 1];
#pragma unroll
    for (int nt = 0; nt < NT8; ++nt) {
      if constexpr (EPI == E8_GATE_RES) {
        if (nt % NH == 0) {
#pragma unroll
          for (int u = 0; u < NH; ++u) {
            if (nt + u < NT8) {
              const int colu = n0 + (nt + u) * 16 + 4 * fg;
              gtv[u] = *reinterpret_cast<const float4*>(g.gate + (size_t)(row / g.T) * g.ldgate + colu);
              xrv[u] = *reinterpret_cast<const float4*>(g.resid + (size_t)row * g.ldcf + colu);
              if constexpr (BIAS_BY_HALF) bias_v[u] = g.bias ? *reinterpret_cast<const float4*>(g.bias + colu) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
          }
        }
      }
      const int col = n0 + nt * 16 + 4 * fg;
      f32x4 v = acc[mt][nt] * deq;
      if constexpr (!MX) {
        const float4 bv = bias_v[BIAS_BY_HALF ? nt % NH : nt];
        v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
      }
      // bf16 / e4m3 results are kept per tile and leave in PAIRS of tiles after the loop (common.h pair_pack: 16-byte bf16 pieces, 8-byte
      // e4m3 pieces; the store tail is issue-bound)
      if constexpr (EPI == E8_BF16 || EPI == E8_DG_BF16) {
        ob[nt] = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      } else if constexpr (EPI == E8_GELU) {
        float h0, h1, h2, h3;
        if (g.aux_q) {                              // kernel-uniform: the backward pass reads GELU'(v) as bytes (SFRON_EPI_DGELU_Q)
          f32x4 y, dy;
          gelu_tanh_both4(v, y, dy);
          h0 = y[0]; h1 = y[1]; h2 = y[2]; h3 = y[3];
          q8[nt] = geluq_pack4(dy);
        } else {
          ab[nt] = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
          h0 = gelu_tanh(v[0]); h1 = gelu_tanh(v[1]); h2 = gelu_tanh(v[2]); h3 = gelu_tanh(v[3]);
        }
        ob[nt] = bf16x4{f2bf(h0), f2bf(h1), f2bf(h2), f2bf(h3)};
        amax4(act_am, h0 * g.c8_scale, h1 * g.c8_scale, h2 * g.c8_scale, h3 * g.c8_scale);
        c8[nt] = pack_e4m3(h0 * g.c8_scale, h1 * g.c8_scale, h2 * g.c8_scale, h3 * g.c8_scale);
      } else {
        ab[nt] = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
        const float4 gt = gtv[nt % NH];
        float4 x = xrv[nt % NH];
        x.x += gt.x * v[0]; x.y += gt.y * v[1]; x.z += gt.z * v[2]; x.w += gt.w * v[3];
        *reinterpret_cast<float4*>(g.Cf + (size_t)row * g.ldcf + col) = x;
      }
    }
    const int colp = n0 + pair_col(fg);
    auto put = [&](__bf16* base, int ld, const bf16x4 (&t)[NT8]) {
      __bf16* const r = base + (size_t)row * ld;
      if ((ld & 7) == 0) {
#pragma unroll
        for (int np = 0; np < NT8 / 2; ++np) *reinterpret_cast<uint4*>(r + colp + np * 32) = pair_pack(t[2 * np], t[2 * np + 1]);
        if constexpr (NT8 & 1) *reinterpret_cast<bf16x4*>(r + n0 + (NT8 - 1) * 16 + 4 * fg) = t[NT8 - 1];
      } else {
#pragma unroll
        for (int nt = 0; nt < NT8; ++nt) *reinterpret_cast<bf16x4*>(r + n0 + nt * 16 + 4 * fg) = t[nt];
      }
    };
    if constexpr (EPI == E8_BF16 || EPI == E8_GELU || EPI == E8_DG_BF16) put(g.Cb, g.ldcb, ob);
    if constexpr (EPI == E8_GATE_RES) put(g.aux, g.ldaux, ab);
    if constexpr (EPI == E8_GELU) {
      if (g.aux_q) {
        uint8_t* const rq = reinterpret_cast<uint8_t*>(g.aux) + (size_t)row * g.ldaux;
#pragma unroll
        for (int np = 0; np < NT8 / 2; ++np) *reinterpret_cast<uint2*>(rq + colp + np * 32) = pair_pack8(q8[2 * np], q8[2 * np + 1]);
        if constexpr (NT8 & 1) *reinterpret_cast<uint32_t*>(rq + n0 + (NT8 - 1) * 16 + 4 * fg) = q8[NT8 - 1];
      } else put(g.aux, g.ldaux, ab);
    }
    if constexpr (EPI == E8_GELU) {
      uint8_t* const r8 = g.C8 + (size_t)row * g.N;
#pragma unroll
      for (int np = 0; np < NT8 / 2; ++np) {
        unsigned x = c8[2 * np], y = c8[2 * np + 1];
        permlane16_swap(x, y);                       // this lane: 8 contiguous e4m3 columns of the pair (the same piece map as the bf16 form)
        *reinterpret_cast<uint2*>(r8 + colp + np * 32) = make_uint2(x, y);
      }
      if constexpr (NT8 & 1) *reinterpret_cast<uint32_t*>(r8 + n0 + (NT8 - 1) * 16 + 4 * fg) = c8[NT8 - 1];
    }
  }
  if constexpr (EPI == E8_GELU) amax_report(g.act_amax, 2, act_am);
}
template __global__ void k_gemm8<E8_BF16, 8>(Gemm8Args);
template __global__ void k_gemm8<E8_GELU, 8>(Gemm8Args);
template __global__ void k_gemm8<E8_GATE_RES, 8>(Gemm8Args);
template __global__ void k_gemm8<E8_BF16, 9>(Gemm8Args);
template __global__ void k_gemm8<E8_GELU, 9>(Gemm8Args);
template __global__ void k_gemm8<E8_GATE_RES, 9>(Gemm8Args);
template __global__ void k_gemm8<E8_BF16, 8, 4>(Gemm8Args);
template __global__ void k_gemm8<E8_GELU, 8, 4>(Gemm8Args);
template __global__ void k_gemm8<E8_GATE_RES, 8, 4>(Gemm8Args);
template __global__ void k_gemm8<E8_BF16, 9, 4>(Gemm8Args);
template __global__ void k_gemm8<E8_GELU, 9, 4>(Gemm8Args);
template __global__ void k_gemm8<E8_GATE_RES, 9, 4>(Gemm8Args);
template __global__ void k_gemm8<E8_DG_BF16, 8>(Gemm8Args);
template __global__ void k_gemm8<E8_DG_BF16, 9>(Gemm8Args);
template __global__ void k_gemm8<E8_DG_GELU, 8>(Gemm8Args);

// ---------------------------------------------------------------- fp8 weight gradients (sfron_fp8_wgrad)
// C[N][K] fp32 = A[N][Mr] . B[K][Mr]^T, both operands MX e4m3 along the reduction Mr (the tokens): [rows][Mr] codes + [rows][Mr / 32] E8M0
// bytes (k_mx8_cast_t of dY and X).  The 192 x 192 output tile of the bf16 weight-gradient GEMM (so the sum-of-squares partials keep their
// count), 128-byte k-steps through three LDS slots filled by buffer_load ... lds (the swizzle of k_gemm8), 8 waves as 2 x 4 of 96 x 48 each.
// A slot: A image 24 KB, B image 24 KB, then the k-step's scale bytes [192 A rows][4] and [192 B rows][4] (six 256-byte DMA pieces: waves
// 0..5 one each, waves 6 and 7 send theirs through the zero-length descriptor to the dummy kilobyte, so every wave issues WG_NDMA pieces).
// Both operands are read in the MX form (frag32_mx: chunks g and g + 4, lane group g's scale byte = that of 32-block g), each with its own
// per-lane scale operand.
struct Wgrad8Args {
  const uint8_t *A, *a_sc, *B, *b_sc;
  int N, K, Mr;
  float* C; int ldc;
  const uint8_t* sq_mask;                 // over C (element (n, k) at n * ldc + k) or null
  double* sq_out;                         // one fp64 partial per tile (tile index tm * (K / 192) + tn), or null
};
constexpr int WG_T = 192, WG_NW = 8, WG_IMG = WG_T * BKB, WG_SLOT = 2 * WG_IMG + 2 * WG_T * 4;
constexpr int WG_NP = WG_T * BKB / 1024 / WG_NW, WG_NDMA = 2 * WG_NP + 1;        // 3 + 3 16-byte pieces + 1 scale piece per wave
constexpr size_t WG_LDS = (size_t)NSLOT8 * WG_SLOT + 1024;

__global__ __launch_bounds__(512) void k_wgrad8(Wgrad8Args g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem8[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = g.K / WG_T;
  int id;
  {
    const int nblk = gridDim.x, b = blockIdx.x, q = nblk >> 3, r = nblk & 7, x = b & 7, y = b >> 3;
    id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + y;
  }
  const int tm = id / ntn, tn = id - tm * ntn, m0 = tm * WG_T, n0 = tn * WG_T;
  const int Mr = g.Mr, nk = Mr / BKB, ssz = Mr >> 5;
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, g.N * Mr, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)g.B, 0, g.K * Mr, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsSA = __builtin_amdgcn_make_buffer_rsrc((void*)g.a_sc, 0, g.N * ssz, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsSB = __builtin_amdgcn_make_buffer_rsrc((void*)g.b_sc, 0, g.K * ssz, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsNull = __builtin_amdgcn_make_buffer_rsrc((void*)g.B, 0, 0, 0x00020000);
  uint8_t* const dummy = smem8 + (size_t)NSLOT8 * WG_SLOT;
  const int lc16 = ((lane & 7) ^ ((lane >> 3) & 7)) << 4;
  int a_off[WG_NP], b_off[WG_NP];
#pragma unroll
  for (int i = 0; i < WG_NP; ++i) {
    a_off[i] = (m0 + (wave + i * WG_NW) * 8 + (lane >> 3)) * Mr + lc16;
    b_off[i] = (n0 + (wave + i * WG_NW) * 8 + (lane >> 3)) * Mr + lc16;
  }
  // scale piece of wave w < 3: A rows 64 w .. 64 w + 63; 3 <= w < 6: B rows 64 (w - 3) ..; LDS: A's [192][4] then B's [192][4]
  const int s_off = wave < 3 ? (m0 + wave * 64 + lane) * ssz : (n0 + (wave - 3) * 64 + lane) * ssz;
  auto issue = [&](int slot, int k0) {
    uint8_t* iA = smem8 + slot * WG_SLOT;
    uint8_t* iB = iA + WG_IMG;
#pragma unroll
    for (int i = 0; i < WG_NP; ++i) dma16b(rsA, iA + (wave + i * WG_NW) * 1024, a_off[i], k0);
#pragma unroll
    for (int i = 0; i < WG_NP; ++i) dma16b(rsB, iB + (wave + i * WG_NW) * 1024, b_off[i], k0);
    if (wave < 3) dma4b(rsSA, iB + WG_IMG + wave * 256, s_off, k0 >> 5);                // wave-uniform
    else if (wave < 6) dma4b(rsSB, iB + WG_IMG + wave * 256, s_off, k0 >> 5);
    else dma4b(rsNull, dummy, 0, 0);
  };
  const int fr = lane & 15, fg = lane >> 4;
  const int wr = wave >> 2, wc = wave & 3;          // this wave: rows wr * 96 .. + 95, columns wc * 48 .. + 47 of the tile
  f32x4 acc[6][3];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk > 0) issue(0, 0);
  if (nk > 1) issue(1, BKB);
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) wait_vm<WG_NDMA>(); else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < nk) issue(slot >= 1 ? slot - 1 : 2, (kt + 2) * BKB);
    const uint8_t* iA = smem8 + slot * WG_SLOT;
    const uint8_t* iB = iA + WG_IMG;
    const uint8_t* iSA = iB + WG_IMG;
    const uint8_t* iSB = iSA + WG_T * 4;
    i32x8 fb[3];
    int sb[3];
#pragma unroll
    for (int nt = 0; nt < 3; ++nt) {
      const int rb = wc * 48 + nt * 16 + fr;
      fb[nt] = frag32_mx(iB, rb, fg);
      sb[nt] = iSB[rb * 4 + fg];
    }
    // every A fragment of the k-step is requested before the first MFMA: left to itself, hipcc sinks each mt's LDS read to its three MFMAs
    // and waits for it there (lgkmcnt(0) six times per k-step); the scheduling barrier keeps the reads in front
    i32x8 fa[6];
    int sa[6];
#pragma unroll
    for (int mt = 0; mt < 6; ++mt) {
      const int ra = wr * 96 + mt * 16 + fr;
      fa[mt] = frag32_mx(iA, ra, fg);
      sa[mt] = iSA[ra * 4 + fg];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mt = 0; mt < 6; ++mt)
#pragma unroll
      for (int nt = 0; nt < 3; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[nt], fa[mt], acc[mt][nt], 0, 0, 0, sb[nt], 0, sa[mt]);
    slot = slot == 2 ? 0 : slot + 1;
  }
  // lane holds C[m0 + 96 wr + 16 mt + fr][n0 + 48 wc + 16 nt + 4 fg .. +3]
  float sq = 0.f;
  const bool sq_on = g.sq_out != nullptr;                                  // kernel-uniform
#pragma unroll
  for (int mt = 0; mt < 6; ++mt) {
    const int row = m0 + wr * 96 + mt * 16 + fr;
    uchar4 mk[3];
    if (sq_on) {
#pragma unroll
      for (int nt = 0; nt < 3; ++nt)
        mk[nt] = g.sq_mask ? *reinterpret_cast<const uchar4*>(g.sq_mask + (size_t)row * g.ldc + n0 + wc * 48 + nt * 16 + 4 * fg)
                           : make_uchar4(1, 1, 1, 1);
    }
#pragma unroll
    for (int nt = 0; nt < 3; ++nt) {
      const f32x4 v = acc[mt][nt];
      *reinterpret_cast<f32x4*>(g.C + (size_t)row * g.ldc + n0 + wc * 48 + nt * 16 + 4 * fg) = v;
      if (sq_on) {
        const uchar4 m4 = mk[nt];
        sq += (m4.x ? v[0] * v[0] : 0.f) + (m4.y ? v[1] * v[1] : 0.f) + (m4.z ? v[2] * v[2] : 0.f) + (m4.w ? v[3] * v[3] : 0.f);
      }
    }
  }
  if (sq_on) {
    // (as the bf16 weight-gradient tile: fp64 from the wave sums on, the waves added in wave order -- bitwise reproducible)
    const double d = wave_sum_d((double)sq);
    __syncthreads();                                                       // every wave is past the main loop: the slots are free
    double* red = reinterpret_cast<double*>(smem8);
    if (lane == 0) red[wave] = d;
    __syncthreads();
    if (tid == 0) {
      double t = red[0];
#pragma unroll
      for (int w2 = 1; w2 < WG_NW; ++w2) t += red[w2];
      g.sq_out[id] = t;
    }
  }
}

int g_fp8_loader_waves = 0;     // process-wide form of the fp8 tiles: 4 = loader waves (sfron_gemm_loader_waves(9)); measured in the config-5 step:
                                // 65.2 / 64.0 / 64.8 ms against 63.5 / 64.1 / 64.1 for the shared-wave form -- off

namespace {
template <int EPI, int NTL, int NL>
int launch8t(const Gemm8Args& g, hipStream_t s) {
  constexpr bool MX = EPI == E8_DG_BF16 || EPI == E8_DG_GELU;
  const size_t lds = (size_t)NSLOT8 * (Tile8<NTL>::SLOT + (MX ? 1024 : 0)) + 1024;      // (+ the dummy kilobyte of uneven DMA plans)
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if ((done.fetch_or(bit) & bit) == 0) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm8<EPI, NTL, NL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return (int)hipGetLastError();
  }
  hipLaunchKernelGGL((k_gemm8<EPI, NTL, NL>), dim3((g.M / FBM) * (g.N / (NTL * 16))), dim3(512 + 64 * NL), lds, s, g);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}
// tile width: the one that fills the last round of 256 CUs better (ties: the wider tile, fewer operand bytes per FLOP)
inline int pick_ntl(int M, int N) {
  auto eff = [&](int w) {
    if (N % w) return 0.0;
    const long tiles = (long)(M / FBM) * (N / w);
    return (double)tiles / (double)(((tiles + 255) / 256) * 256);
  };
  const double e8 = eff(128), e9 = eff(144);
  return e9 >= e8 && e9 > 0.0 ? 9 : 8;
}
template <int EPI>
int launch8(const Gemm8Args& g, hipStream_t s) {
  if (g_fp8_loader_waves == 4) return pick_ntl(g.M, g.N) == 9 ? launch8t<EPI, 9, 4>(g, s) : launch8t<EPI, 8, 4>(g, s);
  return pick_ntl(g.M, g.N) == 9 ? launch8t<EPI, 9, 0>(g, s) : launch8t<EPI, 8, 0>(g, s);
}
inline int grid_for(int64_t items) { int64_t b = (items + TPB - 1) / TPB; return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b)); }
}  // namespace

extern "C" {

int sfron_fp8_gemm_supported(int M, int N, int K) {
  return (M > 0 && N > 0 && K > 0 && M % FBM == 0 && (N % 128 == 0 || N % 144 == 0) && K % BKB == 0) ? 1 : 0;
}

int sfron_fp8_gemm(const sfron_fp8_gemm_desc* d, void* stream) {
  SFRON_CHECK_ARG(d && d->A && d->B && d->w_scale && d->a_scale > 0.f);
  if (!sfron_fp8_gemm_supported(d->M, d->N, d->K)) return SFRON_ERR_UNSUPPORTED;
  SFRON_CHECK_ARG((long)d->M * d->K < (1L << 31) && (long)d->N * d->K < (1L << 31));        // 32-bit buffer offsets
  SFRON_CHECK_ARG((((uintptr_t)d->A | (uintptr_t)d->B) & 15) == 0);
  Gemm8Args g{};
  g.A = d->A; g.B = d->B; g.M = d->M; g.N = d->N; g.K = d->K; g.w_scale = d->w_scale; g.a_scale = d->a_scale; g.bias = d->bias;
  g.Cb = (__bf16*)d->c_bf16; g.ldcb = d->ldc_bf16; g.aux = (__bf16*)d->aux; g.ldaux = d->ldaux; g.C8 = d->c_e4m3; g.c8_scale = d->c_e4m3_scale;
  g.Cf = d->c_f32; g.ldcf = d->ldc_f32; g.resid = d->resid ? d->resid : d->c_f32; g.gate = d->gate; g.ldgate = d->ldgate;
  g.T = d->tokens > 0 ? d->tokens : 1;
  g.act_amax = d->act_amax;
  g.aux_q = d->aux_q;
  if (d->aux_q) SFRON_CHECK_ARG(d->epilogue == SFRON_EPI_GELU && d->ldaux % 8 == 0 && ((uintptr_t)d->aux & 7) == 0);
  hipStream_t s = (hipStream_t)stream;
  switch (d->epilogue) {
    case SFRON_EPI_BF16:
      SFRON_CHECK_ARG(g.Cb && g.ldcb % 4 == 0);
      return launch8<E8_BF16>(g, s);
    case SFRON_EPI_GELU:
      SFRON_CHECK_ARG(g.Cb && g.aux && g.C8 && g.c8_scale > 0.f && g.ldcb % 4 == 0 && g.ldaux % 4 == 0);
      return launch8<E8_GELU>(g, s);
    case SFRON_EPI_GATE_RES:
      SFRON_CHECK_ARG(g.Cf && g.aux && g.gate && g.ldcf % 4 == 0 && g.ldaux % 4 == 0 && g.ldgate % 4 == 0);
      return launch8<E8_GATE_RES>(g, s);
    default:
      return SFRON_ERR_UNSUPPORTED;
  }
}

int sfron_fp8_dgrad(const sfron_fp8_dgrad_desc* d, void* stream) {
  SFRON_CHECK_ARG(d && d->A && d->a_scales && d->B && d->w_scale && d->c_bf16);
  if (!sfron_fp8_gemm_supported(d->M, d->N, d->K)) return SFRON_ERR_UNSUPPORTED;
  SFRON_CHECK_ARG((long)d->M * d->K < (1L << 31) && (long)d->N * d->K < (1L << 31));        // 32-bit buffer offsets
  SFRON_CHECK_ARG((((uintptr_t)d->A | (uintptr_t)d->B) & 15) == 0 && ((uintptr_t)d->a_scales & 3) == 0);
  SFRON_CHECK_ARG(d->tile_hint == 0 || d->tile_hint == 8 || d->tile_hint == 9);
  Gemm8Args g{};
  g.A = d->A; g.B = d->B; g.M = d->M; g.N = d->N; g.K = d->K; g.w_scale = d->w_scale; g.a_scale = 1.0f; g.a_sc = d->a_scales;
  g.Cb = (__bf16*)d->c_bf16; g.ldcb = d->ldc_bf16;
  hipStream_t s = (hipStream_t)stream;
  if (d->epilogue == SFRON_EPI_BF16) {
    SFRON_CHECK_ARG(g.ldcb % 4 == 0 && g.ldcb >= g.N);
    const int ntl = d->tile_hint ? d->tile_hint : pick_ntl(g.M, g.N);
    if (g.N % (ntl * 16)) return SFRON_ERR_UNSUPPORTED;
    return ntl == 9 ? launch8t<E8_DG_BF16, 9, 0>(g, s) : launch8t<E8_DG_BF16, 8, 0>(g, s);
  }
  if (d->epilogue == SFRON_EPI_DGELU || d->epilogue == SFRON_EPI_DGELU_Q) {
    // 256 x 128 tiles only: a 32-block of the MX output must not straddle two tiles
    if (g.N % 128 || d->tile_hint == 9) return SFRON_ERR_UNSUPPORTED;
    SFRON_CHECK_ARG(d->aux && d->c_e4m3 && d->c_scales && g.ldcb % 8 == 0 && g.ldcb >= g.N && d->ldaux >= g.N);
    SFRON_CHECK_ARG(((uintptr_t)d->c_bf16 & 15) == 0 && ((uintptr_t)d->c_e4m3 & 7) == 0 && ((uintptr_t)d->c_scales & 3) == 0);
    g.aux_q = d->epilogue == SFRON_EPI_DGELU_Q;
    if (g.aux_q) SFRON_CHECK_ARG(d->ldaux % 8 == 0 && ((uintptr_t)d->aux & 7) == 0);
    else SFRON_CHECK_ARG(d->ldaux % 4 == 0 && ((uintptr_t)d->aux & 7) == 0);
    g.aux = (__bf16*)d->aux; g.ldaux = d->ldaux; g.C8 = d->c_e4m3; g.c8_sc = d->c_scales; g.colpart = d->col_partials;
    return launch8t<E8_DG_GELU, 8, 0>(g, s);
  }
  return SFRON_ERR_UNSUPPORTED;
}

int sfron_cast_mx8(const uint16_t* src, int M, int N, uint8_t* dst, uint8_t* scales, void* stream) {
  SFRON_CHECK_ARG(src && dst && scales && M > 0 && N > 0 && N % 32 == 0 && (((uintptr_t)src) & 15) == 0 && ((uintptr_t)dst & 7) == 0);
  const int64_t n = (int64_t)M * N;
  hipLaunchKernelGGL(k_cast_mx8, dim3(grid_for(n >> 3)), dim3(TPB), 0, (hipStream_t)stream, (const __bf16*)src, n, dst, scales);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_cast_mx8_t(const uint16_t* src, int M, int W, uint8_t* dst, uint8_t* scales, void* stream) {
  SFRON_CHECK_ARG(src && dst && scales && M > 0 && W > 0 && M % 32 == 0 && W % 8 == 0);
  SFRON_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && (W + TPB - 1) / TPB <= 65535);
  hipLaunchKernelGGL(k_mx8_cast_t, dim3(M / 32, (W + TPB - 1) / TPB), dim3(TPB), 0, (hipStream_t)stream, (const __bf16*)src, M, W, dst, scales);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_fp8_wgrad_supported(int N, int K, int M) {
  return (N > 0 && K > 0 && M > 0 && N % WG_T == 0 && K % WG_T == 0 && M % BKB == 0 && (long)N * M < (1L << 31) &&
          (long)K * M < (1L << 31)) ? 1 : 0;
}

int sfron_fp8_wgrad(const sfron_fp8_wgrad_desc* d, void* stream) {
  SFRON_CHECK_ARG(d && d->A && d->a_scales && d->B && d->b_scales && d->c_f32);
  if (!sfron_fp8_wgrad_supported(d->N, d->K, d->M)) return SFRON_ERR_UNSUPPORTED;
  SFRON_CHECK_ARG(d->ldc >= d->K && d->ldc % 4 == 0 && ((uintptr_t)d->c_f32 & 15) == 0);
  SFRON_CHECK_ARG((((uintptr_t)d->A | (uintptr_t)d->B) & 15) == 0 && (((uintptr_t)d->a_scales | (uintptr_t)d->b_scales) & 3) == 0);
  SFRON_CHECK_ARG(!d->sumsq_mask || d->sumsq_partials);
  if (d->sumsq_mask) SFRON_CHECK_ARG(((uintptr_t)d->sumsq_mask & 3) == 0);
  Wgrad8Args g{};
  g.A = d->A; g.a_sc = d->a_scales; g.B = d->B; g.b_sc = d->b_scales; g.N = d->N; g.K = d->K; g.Mr = d->M;
  g.C = d->c_f32; g.ldc = d->ldc; g.sq_mask = d->sumsq_mask; g.sq_out = d->sumsq_partials;
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if ((done.fetch_or(bit) & bit) == 0) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wgrad8), hipFuncAttributeMaxDynamicSharedMemorySize, (int)WG_LDS) != hipSuccess)
      return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(k_wgrad8, dim3((d->N / WG_T) * (d->K / WG_T)), dim3(WG_NW * 64), WG_LDS, (hipStream_t)stream, g);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_fp8_transpose_shadow(const uint8_t* w8, uint8_t* w8t, const int64_t* table, int n_matrices, void* stream) {
  SFRON_CHECK_ARG(w8 && w8t && table && n_matrices > 0 && n_matrices <= 65535 && (((uintptr_t)w8 | (uintptr_t)w8t) & 7) == 0);
  hipLaunchKernelGGL(k_fp8_transpose_shadow, dim3(256, n_matrices), dim3(TPB), 0, (hipStream_t)stream, w8, w8t, table);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_fp8_quant_tensors(const float* params, const int64_t* table, int n_tensors, const float* scales, uint32_t* amax_bits,
                            uint8_t* dst, int mode, void* stream) {
  SFRON_CHECK_ARG(params && table && amax_bits && n_tensors > 0 && (mode == 0 || (mode == 1 && scales && dst)));
  SFRON_CHECK_ARG((((uintptr_t)params) & 15) == 0 && (!dst || ((uintptr_t)dst & 3) == 0));
  static_assert(sizeof(TensorRange) == 2 * sizeof(int64_t), "table layout");
  hipLaunchKernelGGL(k_fp8_quant_tensors, dim3(64, n_tensors), dim3(TPB), 0, (hipStream_t)stream, params, (const TensorRange*)table, scales,
                     amax_bits, dst, mode);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_fp8_update_scales(uint32_t* amax_bits, int n_tensors, float* scales, void* stream) {
  SFRON_CHECK_ARG(amax_bits && scales && n_tensors > 0);
  hipLaunchKernelGGL(k_fp8_update_scales, dim3(cdiv(n_tensors, 64)), dim3(64), 0, (hipStream_t)stream, amax_bits, n_tensors, scales);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_fp8_activation_amax(uint32_t* act_amax, float* out3, int reset, void* stream) {
  SFRON_CHECK_ARG(act_amax && out3);
  hipStream_t s = (hipStream_t)stream;
  unsigned int bits[3] = {0u, 0u, 0u};
  if (hipMemcpyAsync(bits, act_amax, sizeof(bits), hipMemcpyDeviceToHost, s) != hipSuccess) return (int)hipGetLastError();
  if (hipStreamSynchronize(s) != hipSuccess) return (int)hipGetLastError();
  for (int i = 0; i < 3; ++i) { float f; memcpy(&f, &bits[i], sizeof(f)); out3[i] = f; }
  if (reset && hipMemsetAsync(act_amax, 0, sizeof(bits), s) != hipSuccess) return (int)hipGetLastError();
  return SFRON_OK;
}

int sfron_cast_e4m3(const void* src, int src_is_bf16, int64_t n, float scale, uint8_t* dst, uint32_t* act_amax, void* stream) {
  SFRON_CHECK_ARG(src && dst && n >= 0 && n % 8 == 0 && scale > 0.f && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0);
  if (src_is_bf16)
    hipLaunchKernelGGL(k_cast_e4m3_bf16, dim3(grid_for(n >> 3)), dim3(TPB), 0, (hipStream_t)stream, (const __bf16*)src, n, scale, dst, act_amax);
  else
    hipLaunchKernelGGL(k_cast_e4m3_f32, dim3(grid_for(n >> 2)), dim3(TPB), 0, (hipStream_t)stream, (const float*)src, n, scale, dst, act_amax);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_ln_modulate_fwd_q(const float* x, const float* shift, const float* scale, int ldmod, int tokens, int M, int D, uint16_t* out,
                            uint8_t* out_e4m3, float e4m3_scale, float* mean, float* rstd, uint32_t* act_amax, void* stream) {
  SFRON_CHECK_ARG(x && shift && scale && out && out_e4m3 && mean && rstd && M > 0 && tokens > 0 && e4m3_scale > 0.f);
  SFRON_CHECK_ARG(D % 4 == 0 && D <= 64 * 4 * NCHQ && ldmod % 4 == 0);
  SFRON_CHECK_ARG((((uintptr_t)x | (uintptr_t)shift | (uintptr_t)scale) & 15) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)out_e4m3 & 3) == 0);
  if (M >= 8192 && tokens % 4 == 0)
    hipLaunchKernelGGL(k_ln_mod_fwd_q<4>, dim3(cdiv(M, 16)), dim3(TPB), 0, (hipStream_t)stream, x, shift, scale, ldmod, tokens, M, D, (__bf16*)out,
                     out_e4m3, e4m3_scale, mean, rstd, act_amax);
  else if (M >= 4096 && tokens % 2 == 0)
    hipLaunchKernelGGL(k_ln_mod_fwd_q<2>, dim3(cdiv(M, 8)), dim3(TPB), 0, (hipStream_t)stream, x, shift, scale, ldmod, tokens, M, D, (__bf16*)out,
                     out_e4m3, e4m3_scale, mean, rstd, act_amax);
  else
    hipLaunchKernelGGL(k_ln_mod_fwd_q<1>, dim3(cdiv(M, 4)), dim3(TPB), 0, (hipStream_t)stream, x, shift, scale, ldmod, tokens, M, D, (__bf16*)out,
                     out_e4m3, e4m3_scale, mean, rstd, act_amax);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
