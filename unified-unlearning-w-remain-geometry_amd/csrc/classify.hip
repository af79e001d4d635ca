// The classifier evaluators' own kernels (resnet.py / classify.py): the 7x7 stride-2 stem's patch matrix, ReLU, the 3x3 stride-2 max-pool,
// the pooled fp32 head and the per-row metrics (softmax, entropy, top-k) of DDPM/classifier_evaluation.py and
// SD/eval-scripts/imageclassify.py.  Every other convolution of the two ResNets is sfron_conv_fwd; the stem is this patch matrix on the
// plain GEMM.  All kernels: 64-bit element offsets, no allocation, no synchronisation, LDS for the block reductions of the metrics only.
#include "common.h"
#include "../../include/sfron.h"

namespace {

constexpr int CTPB = 256;
constexpr int STEM_TAPS = 7, STEM_COLS = STEM_TAPS * STEM_TAPS * 3;      // 147 live columns of the patch matrix

inline int cgrid(int64_t n, int per_block = CTPB) {
  int64_t g = (n + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > (1 << 20) ? (1 << 20) : g));
}

// ---- the stem's im2col ----------------------------------------------------------------------------------------------------------------
// ToTensor + Normalize on the fly: bf16_rne((x / 255.0f - mean[c]) / std[c]), the arithmetic of k_image_u8_to_rows (rows.hip)
struct SrcU8 {
  const uint8_t* img; int H, W; float m0, m1, m2, s0, s1, s2;
  __device__ __forceinline__ float at(int64_t b, int c, int h, int w) const {
    const float v = (float)img[((b * H + h) * W + w) * 3 + c];
    const float m = c == 0 ? m0 : (c == 1 ? m1 : m2), s = c == 0 ? s0 : (c == 1 ? s1 : s2);
    return (v / 255.0f - m) / s;
  }
};
struct SrcNCHW {
  const float* x; int H, W;
  __device__ __forceinline__ float at(int64_t b, int c, int h, int w) const { return x[((b * 3 + c) * H + h) * W + w]; }
};

// rows [B * Ho * Wo][kp8 * 8]: column (kh * 7 + kw) * 3 + c = pixel (2 ho + kh - 3, 2 wo + kw - 3), 0 outside the image and from
// column 147 on.  A thread writes 8 columns: one 16-byte store.
template <class S>
__global__ __launch_bounds__(CTPB) void k_patches7(S src, int B, int Ho, int Wo, int kp8, __bf16* __restrict__ rows) {
  const int64_t n = (int64_t)B * Ho * Wo * kp8;
  for (int64_t i = (int64_t)blockIdx.x * CTPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CTPB) {
    const int g = (int)(i % kp8);
    int64_t p = i / kp8;
    const int wo = (int)(p % Wo); p /= Wo;
    const int ho = (int)(p % Ho);
    const int64_t b = p / Ho;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = g * 8 + j;
      float val = 0.0f;
      if (col < STEM_COLS) {
        const int tap = col / 3, c = col - tap * 3, kh = tap / STEM_TAPS, kw = tap - kh * STEM_TAPS;
        const int h = ho * 2 + kh - 3, w = wo * 2 + kw - 3;
        if (h >= 0 && h < src.H && w >= 0 && w < src.W) val = src.at(b, c, h, w);
      }
      v[j] = f2bf(val);
    }
    *reinterpret_cast<bf16x8*>(rows + i * 8) = v;
  }
}

// ---- ReLU and the max-pool --------------------------------------------------------------------------------------------------------------
// max(x, 0) as torch's clamp_min: -0.0 and NaN pass through
__device__ __forceinline__ float relu1(float x) { return x < 0.0f ? 0.0f : x; }

// y[b][ho][wo][c] = max over the in-bounds pixels of the 3x3 window at (2 ho - 1, 2 wo - 1); V channels (a multiple of 4) per thread
template <int V>
__global__ __launch_bounds__(CTPB) void k_relu_maxpool3s2(const float* __restrict__ x, int ld, int B, int H, int W, int C, int Ho, int Wo, int relu,
                                                          __bf16* __restrict__ yb, float* __restrict__ yf) {
  const int cg = C / V;
  const int64_t n = (int64_t)B * Ho * Wo * cg;
  for (int64_t i = (int64_t)blockIdx.x * CTPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CTPB) {
    const int g = (int)(i % cg);
    const int64_t p = i / cg;
    const int wo = (int)(p % Wo);
    const int64_t t = p / Wo;
    const int ho = (int)(t % Ho);
    const int64_t b = t / Ho;
    float m[V];
#pragma unroll
    for (int j = 0; j < V; ++j) m[j] = -__builtin_inff();
#pragma unroll
    for (int dh = 0; dh < 3; ++dh) {
      const int h = ho * 2 + dh - 1;
      if (h < 0 || h >= H) continue;
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) {
        const int w = wo * 2 + dw - 1;
        if (w < 0 || w >= W) continue;
        const float4* r = reinterpret_cast<const float4*>(x + ((b * H + h) * W + w) * ld + (int64_t)g * V);
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
          const float4 a = r[q];
          m[4 * q] = fmaxf(m[4 * q], a.x); m[4 * q + 1] = fmaxf(m[4 * q + 1], a.y);
          m[4 * q + 2] = fmaxf(m[4 * q + 2], a.z); m[4 * q + 3] = fmaxf(m[4 * q + 3], a.w);
        }
      }
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < V; ++j) m[j] = relu1(m[j]);
    }
    const int64_t o = p * C + (int64_t)g * V;
    if (yf) {
#pragma unroll
      for (int q = 0; q < V / 4; ++q) reinterpret_cast<float4*>(yf + o)[q] = make_float4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
    }
    if (yb) {
      if constexpr (V == 8) {
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = f2bf(m[j]);
        *reinterpret_cast<bf16x8*>(yb + o) = v;
      } else {
        *reinterpret_cast<bf16x4*>(yb + o) = bf16x4{f2bf(m[0]), f2bf(m[1]), f2bf(m[2]), f2bf(m[3])};
      }
    }
  }
}

// the tail of every block: x fp32 [rows][ld] -> y_f32 [rows][ld] (may be x itself: a thread reads its 4 values before it writes them)
// and / or y_bf16 [rows][C]
__global__ __launch_bounds__(CTPB) void k_relu_rows(const float* x, int ld, int64_t rows, int C, __bf16* __restrict__ yb, float* yf) {
  const int c4 = C / 4;
  const int64_t n = rows * c4;
  for (int64_t i = (int64_t)blockIdx.x * CTPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CTPB) {
    const int64_t r = i / c4;
    const int c = (int)(i - r * c4) * 4;
    const float4 a = *reinterpret_cast<const float4*>(x + r * ld + c);
    const float4 y = make_float4(relu1(a.x), relu1(a.y), relu1(a.z), relu1(a.w));
    if (yf) *reinterpret_cast<float4*>(yf + r * ld + c) = y;
    if (yb) *reinterpret_cast<bf16x4*>(yb + r * C + c) = bf16x4{f2bf(y.x), f2bf(y.y), f2bf(y.z), f2bf(y.w)};
  }
}

// ---- the head ---------------------------------------------------------------------------------------------------------------------------
// pooled[b][c] = (sum over the HW rows of sample b, in row order) / HW: a thread per (b, c), neighbours read neighbouring channels
__global__ __launch_bounds__(CTPB) void k_pool_mean(const float* __restrict__ x, int ld, int B, int HW, int C, float* __restrict__ pooled) {
  const int64_t n = (int64_t)B * C;
  for (int64_t i = (int64_t)blockIdx.x * CTPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CTPB) {
    const int64_t b = i / C;
    const int c = (int)(i - b * C);
    const float* r = x + b * HW * ld + c;
    float s = 0.0f;
    for (int k = 0; k < HW; ++k) s += r[(int64_t)k * ld];
    pooled[i] = s / (float)HW;
  }
}
// logits[b][n] = sum_c w[n][c] pooled[b][c] + bias[n]: a wave per logit; lane l adds the products of columns 4 l + 256 k .. + 3 in
// ascending order, then the fixed-order wave sum -- the same bits every call
__global__ __launch_bounds__(CTPB) void k_fc(const float* __restrict__ pooled, const float* __restrict__ w, const float* __restrict__ bias, int B, int C,
                                             int n_cls, float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)B * n_cls;
  for (int64_t i = (int64_t)blockIdx.x * (CTPB / WAVE) + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * (CTPB / WAVE)) {
    const int64_t b = i / n_cls;
    const int cls = (int)(i - b * n_cls);
    const float* f = pooled + b * C;
    const float* wr = w + (int64_t)cls * C;
    float s = 0.0f;
    for (int c = lane * 4; c < C; c += WAVE * 4) {
      const float4 a = *reinterpret_cast<const float4*>(f + c), q = *reinterpret_cast<const float4*>(wr + c);
      s += a.x * q.x; s += a.y * q.y; s += a.z * q.z; s += a.w * q.w;
    }
    s = wave_sum(s);
    if (lane == 0) logits[i] = s + (bias ? bias[cls] : 0.0f);
  }
}

// ---- the metrics ------------------------------------------------------------------------------------------------------------------------
// block reductions over CTPB threads (4 waves): every thread gets the result
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
// (p, index) order of the ranking: larger p first, equal p by the lower index
__device__ __forceinline__ bool ranks_before(float pa, int ia, float pb, int ib) { return pa > pb || (pa == pb && ia < ib); }

__device__ __forceinline__ float prob_of(float x, float mx, float denom) { return expf(x - mx) / denom; }

// One workgroup per row: p = softmax(logits) (exp and the division in fp32, the two sums in fp64), entropy = -sum p log p with the
// p == 0 terms counted as 0 (the limit; the reference's expression gives NaN there), p[target], and the topk largest p with their indices.
__global__ __launch_bounds__(CTPB) void k_classify_metrics(const float* __restrict__ logits, int ld, int n_cls, int target, int topk,
                                                           float* __restrict__ probs, float* __restrict__ entropy, float* __restrict__ p_target,
                                                           int* __restrict__ argmax, float* __restrict__ topk_p, int* __restrict__ topk_i) {
  __shared__ float sh_f[4];
  __shared__ int sh_i[4];
  __shared__ double sh_d[4];
  const int64_t row = blockIdx.x;
  const float* x = logits + row * ld;
  const int tid = threadIdx.x;
  float mx = -__builtin_inff();
  for (int c = tid; c < n_cls; c += CTPB) mx = fmaxf(mx, x[c]);
  mx = block_max(mx, sh_f);
  double sum = 0.0;
  for (int c = tid; c < n_cls; c += CTPB) sum += (double)expf(x[c] - mx);
  const float denom = (float)block_sum_d(sum, sh_d);
  double ent = 0.0;
  for (int c = tid; c < n_cls; c += CTPB) {
    const float p = prob_of(x[c], mx, denom);
    if (probs) probs[row * n_cls + c] = p;
    if (p > 0.0f) ent -= (double)p * (double)logf(p);
    if (c == target && p_target) p_target[row] = p;
  }
  ent = block_sum_d(ent, sh_d);
  if (tid == 0 && entropy) entropy[row] = (float)ent;
  // the ranking: pick after pick, each the best (p, index) that ranks after the previous pick
  float prev_p = __builtin_inff();
  int prev_i = -1;
  const int picks = topk > 1 ? topk : 1;
  for (int k = 0; k < picks; ++k) {
    float bp = -1.0f;          // below every probability
    int bi = 0x7fffffff;
    for (int c = tid; c < n_cls; c += CTPB) {
      const float p = prob_of(x[c], mx, denom);
      if (ranks_before(prev_p, prev_i, p, c) && ranks_before(p, c, bp, bi)) { bp = p; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float op = __shfl_xor(bp, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ranks_before(op, oi, bp, bi)) { bp = op; bi = oi; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { sh_f[tid >> 6] = bp; sh_i[tid >> 6] = bi; }
    __syncthreads();
    bp = sh_f[0]; bi = sh_i[0];
#pragma unroll
    for (int wv = 1; wv < 4; ++wv)
      if (ranks_before(sh_f[wv], sh_i[wv], bp, bi)) { bp = sh_f[wv]; bi = sh_i[wv]; }
    if (tid == 0) {
      if (k == 0 && argmax) argmax[row] = bi;
      if (k < topk) { if (topk_p) topk_p[row * topk + k] = bp; if (topk_i) topk_i[row * topk + k] = bi; }
    }
    prev_p = bp; prev_i = bi;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int patches7_geom(int B, int H, int W, int k_pad, const void* rows, int& Ho, int& Wo) {
  SFRON_CHECK_ARG(rows && B > 0 && H > 0 && W > 0 && k_pad >= 152 && k_pad % 8 == 0 && aligned16(rows));
  Ho = (H + 6 - 7) / 2 + 1; Wo = (W + 6 - 7) / 2 + 1;
  SFRON_CHECK_ARG(sfron_fits31((int64_t)B * Ho * Wo * k_pad * 2));
  return SFRON_OK;
}

}  // namespace

extern "C" {

int sfron_image_u8_patches7(const uint8_t* img, int B, int H, int W, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                            int k_pad, uint16_t* rows, void* stream) {
  int Ho, Wo;
  SFRON_CHECK_ARG(img);
  const int rc = patches7_geom(B, H, W, k_pad, rows, Ho, Wo); if (rc) return rc;
  SFRON_CHECK_ARG(sfron_fits31((int64_t)B * H * W * 3));
  const SrcU8 src{img, H, W, mean0, mean1, mean2, std0, std1, std2};
  hipLaunchKernelGGL(k_patches7<SrcU8>, dim3(cgrid((int64_t)B * Ho * Wo * (k_pad / 8))), dim3(CTPB), 0, (hipStream_t)stream, src, B, Ho, Wo, k_pad / 8,
                     (__bf16*)rows);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_nchw_patches7(const float* x, int B, int H, int W, int k_pad, uint16_t* rows, void* stream) {
  int Ho, Wo;
  SFRON_CHECK_ARG(x);
  const int rc = patches7_geom(B, H, W, k_pad, rows, Ho, Wo); if (rc) return rc;
  SFRON_CHECK_ARG(sfron_fits31((int64_t)B * H * W * 3 * 4));
  const SrcNCHW src{x, H, W};
  hipLaunchKernelGGL(k_patches7<SrcNCHW>, dim3(cgrid((int64_t)B * Ho * Wo * (k_pad / 8))), dim3(CTPB), 0, (hipStream_t)stream, src, B, Ho, Wo, k_pad / 8,
                     (__bf16*)rows);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_relu_maxpool3s2(const float* x, int ld, int B, int H, int W, int C, int relu, uint16_t* y_bf16, float* y_f32, void* stream) {
  SFRON_CHECK_ARG(x && (y_bf16 || y_f32) && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0);
  SFRON_CHECK_ARG(aligned16(x) && aligned16(y_f32) && ((uintptr_t)y_bf16 & 7) == 0);
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent((int64_t)B * H * W, ld, C, 4)) && sfron_fits31((int64_t)B * Ho * Wo * C * 4));
  hipStream_t s = (hipStream_t)stream;
  if (C % 8 == 0 && aligned16(y_bf16))
    hipLaunchKernelGGL(k_relu_maxpool3s2<8>, dim3(cgrid((int64_t)B * Ho * Wo * (C / 8))), dim3(CTPB), 0, s, x, ld, B, H, W, C, Ho, Wo, relu,
                       (__bf16*)y_bf16, y_f32);
  else
    hipLaunchKernelGGL(k_relu_maxpool3s2<4>, dim3(cgrid((int64_t)B * Ho * Wo * (C / 4))), dim3(CTPB), 0, s, x, ld, B, H, W, C, Ho, Wo, relu,
                       (__bf16*)y_bf16, y_f32);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_relu_rows(const float* x, int ld, int64_t rows, int C, uint16_t* y_bf16, float* y_f32, void* stream) {
  SFRON_CHECK_ARG(x && (y_bf16 || y_f32) && rows > 0 && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0);
  SFRON_CHECK_ARG(aligned16(x) && aligned16(y_f32) && ((uintptr_t)y_bf16 & 7) == 0);
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent(rows, ld, C, 4)));
  hipLaunchKernelGGL(k_relu_rows, dim3(cgrid(rows * (C / 4))), dim3(CTPB), 0, (hipStream_t)stream, x, ld, rows, C, (__bf16*)y_bf16, y_f32);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_pool_fc(const float* x, int ld, int B, int HW, int C, const float* w, const float* bias, int n_cls, float* pooled, float* logits,
                  void* stream) {
  SFRON_CHECK_ARG(x && w && pooled && logits && B > 0 && HW > 0 && C > 0 && n_cls > 0 && C % 4 == 0 && ld >= C);
  SFRON_CHECK_ARG(aligned16(w) && aligned16(pooled));
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent((int64_t)B * HW, ld, C, 4)) && sfron_fits31((int64_t)n_cls * C * 4) &&
                  sfron_fits31((int64_t)B * n_cls * 4) && sfron_fits31((int64_t)B * C * 4));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pool_mean, dim3(cgrid((int64_t)B * C)), dim3(CTPB), 0, s, x, ld, B, HW, C, pooled);
  SFRON_LAUNCH_STATUS();
  hipLaunchKernelGGL(k_fc, dim3(cgrid((int64_t)B * n_cls, CTPB / WAVE)), dim3(CTPB), 0, s, pooled, w, bias, B, C, n_cls, logits);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_classify_metrics(const float* logits, int ld, int B, int n_cls, int target, int topk, float* probs, float* entropy, float* p_target,
                           int32_t* argmax, float* topk_p, int32_t* topk_i, void* stream) {
  SFRON_CHECK_ARG(logits && B > 0 && n_cls > 0 && ld >= n_cls && topk >= 0 && topk <= 8 && topk <= n_cls);
  SFRON_CHECK_ARG(!p_target || (target >= 0 && target < n_cls));
  SFRON_CHECK_ARG(topk == 0 || (topk_p && topk_i));
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent(B, ld, n_cls, 4)));
  hipLaunchKernelGGL(k_classify_metrics, dim3(B), dim3(CTPB), 0, (hipStream_t)stream, logits, ld, n_cls, target, topk, probs, entropy, p_target,
                     argmax, topk_p, topk_i);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
