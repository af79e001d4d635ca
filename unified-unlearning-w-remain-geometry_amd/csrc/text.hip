// The CLIP text encoder of SD v1 (FrozenCLIPEmbedder, SD/ldm/modules/encoders/modules.py:230-266: transformers CLIPTextModel,
// last_hidden_state), forward only: token + position embedding, causal self-attention of short sequences (77 tokens), and the final
// LayerNorm with fp32 output.  The projections run on sfron_gemm_bf16 (fc1 with SFRON_EPI_QUICK_GELU), the per-layer LayerNorms on
// sfron_layernorm_fwd.
#include "common.h"
#include "../../include/sfron.h"

namespace {

constexpr int TPB_ROWS = 256;

// ---- embedding: one wave per token row, out[row] = tok[id] + pos[row % T]; an id outside [0, vocab) is never read: its row is
// written as zeros and *err is set
__global__ __launch_bounds__(TPB_ROWS) void k_clip_embed(const int64_t* __restrict__ ids, int rows, int T, const float* __restrict__ tok,
                                                         int vocab, const float* __restrict__ pos, int D, float* __restrict__ out,
                                                         int* __restrict__ err) {
  const int row = blockIdx.x * (TPB_ROWS / WAVE) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int64_t id = ids[row];
  const bool ok = id >= 0 && id < vocab;
  if (!ok && lane == 0) atomicOr(err, 1);
  const float* tr = tok + (ok ? id : 0) * (int64_t)D;
  const float* pr = pos + (int64_t)(row % T) * D;
  float* orow = out + (int64_t)row * D;
  for (int i = lane; i < D; i += WAVE) orow[i] = ok ? tr[i] + pr[i] : 0.0f;
}

// ---- LayerNorm(D, eps, affine) with fp32 output, one wave per row (CLIPTextTransformer.final_layer_norm)
__global__ __launch_bounds__(TPB_ROWS) void k_layernorm_f32(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int64_t rows, int D, float eps,
                                                            float* __restrict__ y) {
  const int64_t row = (int64_t)blockIdx.x * (TPB_ROWS / WAVE) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * D;
  float s = 0.f;
  for (int i = lane; i < D; i += WAVE) s += xr[i];
  const float m = wave_sum(s) / D;
  float q = 0.f;
  for (int i = lane; i < D; i += WAVE) { const float d = xr[i] - m; q += d * d; }
  const float r = rsqrtf(wave_sum(q) / D + eps);
  for (int i = lane; i < D; i += WAVE) y[row * D + i] = (xr[i] - m) * r * gamma[i] + beta[i];
}

// ---- causal attention, T <= 128, head_dim 64: one workgroup of eight waves per (sample, head), wave w = query rows 16 w .. 16 w + 15.
// V^T of the head sits in LDS (keys beyond T zero); q and k fragments come straight from global memory.  S^T = K Q^T on
// v_mfma_f32_16x16x32_bf16 (K the row operand): a lane holds S[query 16 w + (lane & 15)][key 16 kb + 4 (lane >> 4) + j], so the softmax of
// a query row is spread over the four lanes r, r + 16, r + 32, r + 48.  Those same registers are the column operand of O^T = V^T P^T: the
// contraction slots 8 g .. 8 g + 7 of a 32-key step s stand for keys 32 s + 4 g + 0..3 and 32 s + 16 + 4 g + 0..3 (the order of a
// contraction is free as long as both operands agree), and the V^T fragment is read from LDS in that order.  Key blocks after the wave's
// last query row are not formed; keys after the query row or at or beyond T are masked before the max is taken.
constexpr int CA_TMAX = 128, CA_HD = 64, CA_LDV = CA_TMAX + 8;     // V^T rows padded to 272 B

__global__ __launch_bounds__(512) void k_attn_causal(const __bf16* __restrict__ qkv, __bf16* __restrict__ o, int T, int H, float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 vt[CA_HD * CA_LDV];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int D = H * CA_HD, ld = 3 * D;
  const __bf16* base = qkv + (size_t)b * T * ld + h * CA_HD;
  const int tid = threadIdx.x;
  bf16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (__bf16)0.0f;
  for (int e = tid; e < CA_TMAX * 8; e += 512) {
    const int key = e >> 3, c = e & 7;
    const bf16x8 v = key < T ? *reinterpret_cast<const bf16x8*>(base + (size_t)key * ld + 2 * D + 8 * c) : z;
#pragma unroll
    for (int i = 0; i < 8; ++i) vt[(8 * c + i) * CA_LDV + key] = v[i];
  }
  __syncthreads();
  const int lane = tid & 63, r = lane & 15, g = lane >> 4;
  const int qb = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (qb * 16 >= T) return;
  const int qrow = qb * 16 + r;
  bf16x8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = qrow < T ? *reinterpret_cast<const bf16x8*>(base + (size_t)qrow * ld + 8 * g + 32 * ks) : z;
  const int nkb = qb + 1;                                  // key blocks 0 .. qb
  f32x4 s[8];
  float m = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) {
    s[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kb < nkb) {
      const int key = kb * 16 + r;
      bf16x8 k0 = z, k1 = z;
      if (key < T) {
        k0 = *reinterpret_cast<const bf16x8*>(base + (size_t)key * ld + D + 8 * g);
        k1 = *reinterpret_cast<const bf16x8*>(base + (size_t)key * ld + D + 8 * g + 32);
      }
      s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[0], s[kb], 0, 0, 0);
      s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[1], s[kb], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kj = kb * 16 + 4 * g + j;
        s[kb][j] = (kj <= qrow && kj < T) ? s[kb][j] * scale : -INFINITY;
        m = fmaxf(m, s[kb][j]);
      }
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));                     // key 0 is always valid: m is finite
  float l = 0.f;
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) {
    if (kb < nkb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[kb][j] = __expf(s[kb][j] - m); l += s[kb][j]; }
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  f32x4 acc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    if (2 * st < nkb) {
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pf[j] = f2bf(s[2 * st][j]);
        pf[4 + j] = f2bf(2 * st + 1 < nkb ? s[2 * st + 1][j] : 0.0f);
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const __bf16* vrow = vt + (db * 16 + r) * CA_LDV + 32 * st + 4 * g;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vrow), hi = *reinterpret_cast<const bf16x4*>(vrow + 16);
        const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[db], 0, 0, 0);
      }
    }
  }
  if (qrow < T) {
    const float inv = 1.0f / l;
    __bf16* orow = o + ((size_t)b * T + qrow) * D + h * CA_HD;
#pragma unroll
    for (int db = 0; db < 4; ++db) *reinterpret_cast<bf16x4*>(orow + db * 16 + 4 * g) = f2bf4(acc[db] * inv);
  }
}

}  // namespace

extern "C" {

int sfron_clip_embed(const int64_t* ids, int B, int T, const float* tok_emb, int vocab, const float* pos_emb, int D, float* out, int* err,
                     void* stream) {
  SFRON_CHECK_ARG(ids && tok_emb && pos_emb && out && err && B > 0 && T > 0 && vocab > 0 && D > 0);
  SFRON_CHECK_ARG((int64_t)B * T < (1ll << 31));        // the row count is an `int`; the kernel's offsets are 64-bit (no byte limit)
  const int rows = B * T;
  hipLaunchKernelGGL(k_clip_embed, dim3(cdiv(rows, TPB_ROWS / WAVE)), dim3(TPB_ROWS), 0, (hipStream_t)stream, ids, rows, T, tok_emb, vocab,
                     pos_emb, D, out, err);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_attn_causal_fwd(const uint16_t* qkv, uint16_t* o, int B, int T, int H, int hd, void* stream) {
  SFRON_CHECK_ARG(qkv && o && B > 0 && H > 0 && (int64_t)B * H < (1ll << 31));      // grid; offsets in the kernel are size_t (no byte limit)
  if (hd != CA_HD || T < 1 || T > CA_TMAX) return SFRON_ERR_UNSUPPORTED;
  SFRON_CHECK_ARG((((uintptr_t)qkv) & 15) == 0 && (((uintptr_t)o) & 7) == 0);
  hipLaunchKernelGGL(k_attn_causal, dim3(B * H), dim3(512), 0, (hipStream_t)stream, (const __bf16*)qkv, (__bf16*)o, T, H,
                     1.0f / sqrtf((float)hd));
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, int64_t rows, int D, float eps, float* y, void* stream) {
  SFRON_CHECK_ARG(x && gamma && beta && y && rows > 0 && D > 0);
  hipLaunchKernelGGL(k_layernorm_f32, dim3((unsigned)((rows + 3) / 4)), dim3(TPB_ROWS), 0, (hipStream_t)stream, x, gamma, beta, rows, D, eps, y);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
