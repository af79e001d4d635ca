// The FID Inception-v3's own kernels (inception.py / fid.py): the patch matrix of a general (kh, kw, stride, pad_h, pad_w) convolution, the
// TF1 bilinear resize + normalise of the input bytes, the three 3x3 pools and the global average with an output leading dimension (a branch
// writes its columns straight into the concatenated row), and the fp64 feature statistics (mean and covariance) FID is computed from.
// The products themselves are sfron_conv_fwd and the batched GEMM.  All kernels: 64-bit element offsets, no allocation, no
// synchronisation.  The patch, resize and pool kernels only move data (LDS unused); the covariance is a plain LDS-tiled fp64 product.
#include "common.h"
#include "../../include/sfron.h"

namespace {

constexpr int ITPB = 256;

inline int igrid(int64_t n, int per_block = ITPB) {
  int64_t g = (n + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > (1 << 20) ? (1 << 20) : g));
}
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }
inline int out_size(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }

// ---- patch matrix ----------------------------------------------------------------------------------------------------------------------
// rows [B * Ho * Wo][kh * kw * C]: columns (i * kw + j) * C .. + C - 1 = the C channels of pixel (ho * s + i - ph, wo * s + j - pw), zero
// outside the image.  A thread moves 8 channels: one 16-byte load, one 16-byte store.
__global__ __launch_bounds__(ITPB) void k_patch_rows(const __bf16* __restrict__ x, int ld, int B, int H, int W, int C, int kh, int kw, int s, int ph,
                                                     int pw, int Ho, int Wo, __bf16* __restrict__ rows) {
  const int c8 = C / 8, taps = kh * kw;
  const int64_t n = (int64_t)B * Ho * Wo * taps * c8;
  for (int64_t i = (int64_t)blockIdx.x * ITPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * ITPB) {
    const int g = (int)(i % c8);
    int64_t p = i / c8;
    const int tap = (int)(p % taps); p /= taps;
    const int wo = (int)(p % Wo); p /= Wo;
    const int ho = (int)(p % Ho);
    const int64_t b = p / Ho;
    const int h = ho * s + tap / kw - ph, w = wo * s + tap % kw - pw;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (h >= 0 && h < H && w >= 0 && w < W) v = *reinterpret_cast<const uint4*>(x + ((b * H + h) * W + w) * ld + g * 8);
    *reinterpret_cast<uint4*>(rows + i * 8) = v;
  }
}

// ---- TF1 bilinear resize + normalise ---------------------------------------------------------------------------------------------------
// tf.image.resize_bilinear(align_corners=False) of TF1: src = dst * (in / out) -- no half-pixel offset --, lo = floor(src), hi =
// min(lo + 1, in - 1), frac = src - lo.  fp32, one IEEE operation per step in this order (no contraction):
//   top = tl + (tr - tl) * fx;  bot = bl + (br - bl) * fx;  v = top + (bot - top) * fy;  y = (v - 128) / 128;  bf16_rne(y)
// A thread writes one pixel: channels 0 .. 2 and zeros up to c_pad = 8 (one 16-byte store).
__global__ __launch_bounds__(ITPB) void k_resize_tf1(const uint8_t* __restrict__ img, int B, int H, int W, int Ho, int Wo, __bf16* __restrict__ rows) {
  const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
  const int64_t n = (int64_t)B * Ho * Wo;
  for (int64_t i = (int64_t)blockIdx.x * ITPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * ITPB) {
    const int wo = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int ho = (int)(t % Ho);
    const int64_t b = t / Ho;
    const float fy0 = (float)ho * sh, fx0 = (float)wo * sw;
    int y0 = (int)floorf(fy0), x0 = (int)floorf(fx0);
    y0 = y0 > H - 1 ? H - 1 : y0; x0 = x0 > W - 1 ? W - 1 : x0;
    const int y1 = y0 + 1 > H - 1 ? H - 1 : y0 + 1, x1 = x0 + 1 > W - 1 ? W - 1 : x0 + 1;
    const float fy = fy0 - (float)y0, fx = fx0 - (float)x0;
    const uint8_t* base = img + b * H * W * 3;
    const uint8_t *ptl = base + ((int64_t)y0 * W + x0) * 3, *ptr_ = base + ((int64_t)y0 * W + x1) * 3;
    const uint8_t *pbl = base + ((int64_t)y1 * W + x0) * 3, *pbr = base + ((int64_t)y1 * W + x1) * 3;
    bf16x8 v;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tl = (float)ptl[c], tr = (float)ptr_[c], bl = (float)pbl[c], br = (float)pbr[c];
      const float top = tl + (tr - tl) * fx;
      const float bot = bl + (br - bl) * fx;
      const float val = top + (bot - top) * fy;
      v[c] = f2bf((val - 128.0f) / 128.0f);
    }
#pragma unroll
    for (int c = 3; c < 8; ++c) v[c] = f2bf(0.0f);
    *reinterpret_cast<bf16x8*>(rows + i * 8) = v;
  }
}

// ---- pools -----------------------------------------------------------------------------------------------------------------------------
// four channels of a row: fp32 (16 bytes) or bf16 (8 bytes) in, the same choice out
__device__ __forceinline__ f32x4 load4(const void* x, int64_t off, int is_bf16) {
  if (is_bf16) return bf2f4(*reinterpret_cast<const bf16x4*>((const __bf16*)x + off));
  return as4(*reinterpret_cast<const float4*>((const float*)x + off));
}
__device__ __forceinline__ void store4(void* y, int64_t off, int is_bf16, f32x4 v) {
  if (is_bf16) *reinterpret_cast<bf16x4*>((__bf16*)y + off) = f2bf4(v);
  else *reinterpret_cast<float4*>((float*)y + off) = make_float4(v[0], v[1], v[2], v[3]);
}

// KIND 0: max 3x3 stride 2 pad 0 (floor);  1: max 3x3 stride 1 pad 1 (padding is -inf);  2: average 3x3 stride 1 pad 1 over the in-bounds
// pixels: the window sum in fp64 (exact for nine fp32 values up to its last bit), rounded to fp32 once, divided in fp32 by their number
template <int KIND>
__global__ __launch_bounds__(ITPB) void k_pool3(const void* __restrict__ x, int x_bf16, int ld, int B, int H, int W, int C, int Ho, int Wo,
                                                void* __restrict__ y, int y_bf16, int ld_out) {
  constexpr int S = KIND == 0 ? 2 : 1, P = KIND == 0 ? 0 : 1;
  const int c4 = C / 4;
  const int64_t n = (int64_t)B * Ho * Wo * c4;
  for (int64_t i = (int64_t)blockIdx.x * ITPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * ITPB) {
    const int g = (int)(i % c4);
    const int64_t p = i / c4;
    const int wo = (int)(p % Wo);
    const int64_t t = p / Wo;
    const int ho = (int)(t % Ho);
    const int64_t b = t / Ho;
    f32x4 m = splat4(-__builtin_inff());
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int cnt = 0;
#pragma unroll
    for (int dh = 0; dh < 3; ++dh) {
      const int h = ho * S + dh - P;
      if (h < 0 || h >= H) continue;
#pragma unroll
      for (int dw = 0; dw < 3; ++dw) {
        const int w = wo * S + dw - P;
        if (w < 0 || w >= W) continue;
        const f32x4 a = load4(x, ((b * H + h) * W + w) * ld + (int64_t)g * 4, x_bf16);
        if constexpr (KIND == 2) { s0 += (double)a[0]; s1 += (double)a[1]; s2 += (double)a[2]; s3 += (double)a[3]; ++cnt; }
        else m = f32x4{fmaxf(m[0], a[0]), fmaxf(m[1], a[1]), fmaxf(m[2], a[2]), fmaxf(m[3], a[3])};
      }
    }
    if constexpr (KIND == 2) {
      const float d = (float)cnt;
      m = f32x4{(float)s0 / d, (float)s1 / d, (float)s2 / d, (float)s3 / d};
    }
    store4(y, p * ld_out + (int64_t)g * 4, y_bf16, m);
  }
}

// y[b][c] = (sum over the HW rows of sample b, in row order, fp32) / HW: a thread per (b, c)
__global__ __launch_bounds__(ITPB) void k_global_avg(const void* __restrict__ x, int x_bf16, int ld, int B, int HW, int C, float* __restrict__ y) {
  const int64_t n = (int64_t)B * C;
  for (int64_t i = (int64_t)blockIdx.x * ITPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * ITPB) {
    const int64_t b = i / C;
    const int c = (int)(i - b * C);
    const int64_t o = b * HW * ld + c;
    float s = 0.0f;
    if (x_bf16) for (int k = 0; k < HW; ++k) s += bf2f(((const __bf16*)x)[o + (int64_t)k * ld]);
    else for (int k = 0; k < HW; ++k) s += ((const float*)x)[o + (int64_t)k * ld];
    y[i] = s / (float)HW;
  }
}

// ---- feature statistics ----------------------------------------------------------------------------------------------------------------
// mu[d] = (sum_n x[n][d]) / N in fp64.  A workgroup owns 4 columns; thread t adds rows t, t + 256, ... in ascending order, then the
// fixed butterfly over the wave and the four wave sums in order: one owner, one order.
__global__ __launch_bounds__(ITPB) void k_feature_mean(const float* __restrict__ x, int64_t N, int ld, double* __restrict__ mu) {
  __shared__ double sh[4][4];
  const int c = blockIdx.x * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = threadIdx.x; r < N; r += ITPB) {
    const float4 a = *reinterpret_cast<const float4*>(x + r * ld + c);
    s[0] += (double)a.x; s[1] += (double)a.y; s[2] += (double)a.z; s[3] += (double)a.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = wave_sum_d(s[j]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[threadIdx.x >> 6][j] = s[j];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int j = threadIdx.x;
    mu[c + j] = (((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j]) / (double)N;
  }
}

// sigma[i][j] = (sum_n (x[n][i] - mu[i]) (x[n][j] - mu[j])) * (1 / (N - 1)) in fp64 (np.cov multiplies by the reciprocal).  A workgroup
// owns a 64 x 64 tile with tile column >= tile row and writes its mirror too; a thread owns 4 x 4 of it and adds the rows in ascending
// order with fma: one owner, one order.  The centred rows of both column ranges go through LDS, CK rows at a time; a column >= D or a
// row >= N is staged as 0 and adds nothing.
constexpr int CT = 64, CK = 16;
__global__ __launch_bounds__(ITPB) void k_feature_cov(const float* __restrict__ x, int64_t N, int D, int ld, const double* __restrict__ mu,
                                                      double* __restrict__ sigma) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;
  __shared__ double sa[CK][CT], sb[CK][CT];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  // staging: thread -> (row tid / 16 of the chunk, columns 4 (tid % 16) .. + 3) of either range
  const int lr = tid >> 4, lc = (tid & 15) * 4;
  const int ca = ti * CT + lc, cb = tj * CT + lc;
  double ma[4] = {0, 0, 0, 0}, mb[4] = {0, 0, 0, 0};
  if (ca < D) { ma[0] = mu[ca]; ma[1] = mu[ca + 1]; ma[2] = mu[ca + 2]; ma[3] = mu[ca + 3]; }
  if (cb < D) { mb[0] = mu[cb]; mb[1] = mu[cb + 1]; mb[2] = mu[cb + 2]; mb[3] = mu[cb + 3]; }
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (int64_t n0 = 0; n0 < N; n0 += CK) {
    const int64_t r = n0 + lr;
    double va[4] = {0, 0, 0, 0}, vb[4] = {0, 0, 0, 0};
    if (r < N) {
      if (ca < D) {
        const float4 q = *reinterpret_cast<const float4*>(x + r * ld + ca);
        va[0] = (double)q.x - ma[0]; va[1] = (double)q.y - ma[1]; va[2] = (double)q.z - ma[2]; va[3] = (double)q.w - ma[3];
      }
      if (cb < D) {
        const float4 q = *reinterpret_cast<const float4*>(x + r * ld + cb);
        vb[0] = (double)q.x - mb[0]; vb[1] = (double)q.y - mb[1]; vb[2] = (double)q.z - mb[2]; vb[3] = (double)q.w - mb[3];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) { sa[lr][lc + j] = va[j]; sb[lr][lc + j] = vb[j]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CK; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[j] = sa[k][ty * 4 + j]; b[j] = sb[k][tx * 4 + j]; }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_fma(a[p], b[q], acc[p][q]);
    }
  }
  const double rn = 1.0 / (double)(N - 1);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = ti * CT + ty * 4 + p;
    if (i >= D) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = tj * CT + tx * 4 + q;
      if (j >= D) continue;
      const double v = acc[p][q] * rn;
      sigma[(int64_t)i * D + j] = v;
      if (tj > ti) sigma[(int64_t)j * D + i] = v;
    }
  }
}

}  // namespace

extern "C" {

int sfron_patch_rows(const uint16_t* x, int ld, int B, int H, int W, int C, int kh, int kw, int stride, int pad_h, int pad_w, uint16_t* rows,
                     void* stream) {
  SFRON_CHECK_ARG(x && rows && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && ld >= C && ld % 8 == 0 && al16(x) && al16(rows));
  SFRON_CHECK_ARG(kh > 0 && kw > 0 && kh <= 7 && kw <= 7 && stride > 0 && stride <= 2 && pad_h >= 0 && pad_w >= 0 && pad_h < kh && pad_w < kw);
  SFRON_CHECK_ARG(H + 2 * pad_h >= kh && W + 2 * pad_w >= kw);
  const int Ho = out_size(H, kh, stride, pad_h), Wo = out_size(W, kw, stride, pad_w);
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent((int64_t)B * H * W, ld, C, 2)) && sfron_fits31((int64_t)B * Ho * Wo * kh * kw * C * 2));
  hipLaunchKernelGGL(k_patch_rows, dim3(igrid((int64_t)B * Ho * Wo * kh * kw * (C / 8))), dim3(ITPB), 0, (hipStream_t)stream, (const __bf16*)x, ld, B,
                     H, W, C, kh, kw, stride, pad_h, pad_w, Ho, Wo, (__bf16*)rows);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_resize_tf1_u8(const uint8_t* img, int B, int H, int W, int Ho, int Wo, int c_pad, uint16_t* rows, void* stream) {
  SFRON_CHECK_ARG(img && rows && B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && c_pad == 8 && al16(rows));
  SFRON_CHECK_ARG(sfron_fits31((int64_t)B * H * W * 3) && sfron_fits31((int64_t)B * Ho * Wo * c_pad * 2));
  hipLaunchKernelGGL(k_resize_tf1, dim3(igrid((int64_t)B * Ho * Wo)), dim3(ITPB), 0, (hipStream_t)stream, img, B, H, W, Ho, Wo, (__bf16*)rows);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_pool3(const void* x, int x_bf16, int ld, int B, int H, int W, int C, int kind, void* y, int y_bf16, int ld_out, void* stream) {
  SFRON_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ld >= C && ld % 4 == 0 && ld_out >= C && ld_out % 4 == 0);
  SFRON_CHECK_ARG(kind >= SFRON_POOL_MAX_S2 && kind <= SFRON_POOL_AVG_S1 && (x_bf16 ? al8(x) : al16(x)) && (y_bf16 ? al8(y) : al16(y)));
  SFRON_CHECK_ARG(kind != SFRON_POOL_MAX_S2 || (H >= 3 && W >= 3));
  const int Ho = kind == SFRON_POOL_MAX_S2 ? (H - 3) / 2 + 1 : H, Wo = kind == SFRON_POOL_MAX_S2 ? (W - 3) / 2 + 1 : W;
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent((int64_t)B * H * W, ld, C, x_bf16 ? 2 : 4)) &&
                  sfron_fits31(sfron_extent((int64_t)B * Ho * Wo, ld_out, C, y_bf16 ? 2 : 4)));
  const dim3 grid(igrid((int64_t)B * Ho * Wo * (C / 4)));
  hipStream_t s = (hipStream_t)stream;
  if (kind == SFRON_POOL_MAX_S2) hipLaunchKernelGGL(k_pool3<0>, grid, dim3(ITPB), 0, s, x, x_bf16, ld, B, H, W, C, Ho, Wo, y, y_bf16, ld_out);
  else if (kind == SFRON_POOL_MAX_S1) hipLaunchKernelGGL(k_pool3<1>, grid, dim3(ITPB), 0, s, x, x_bf16, ld, B, H, W, C, Ho, Wo, y, y_bf16, ld_out);
  else hipLaunchKernelGGL(k_pool3<2>, grid, dim3(ITPB), 0, s, x, x_bf16, ld, B, H, W, C, Ho, Wo, y, y_bf16, ld_out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_global_avgpool(const void* x, int x_bf16, int ld, int B, int HW, int C, float* y, void* stream) {
  SFRON_CHECK_ARG(x && y && B > 0 && HW > 0 && C > 0 && ld >= C);
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent((int64_t)B * HW, ld, C, x_bf16 ? 2 : 4)) && sfron_fits31((int64_t)B * C * 4));
  hipLaunchKernelGGL(k_global_avg, dim3(igrid((int64_t)B * C)), dim3(ITPB), 0, (hipStream_t)stream, x, x_bf16, ld, B, HW, C, y);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_feature_stats(const float* x, int64_t N, int D, int ld, double* mu, double* sigma, void* stream) {
  SFRON_CHECK_ARG(x && mu && sigma && N >= 2 && D > 0 && D <= 2048 && D % 4 == 0 && ld >= D && ld % 4 == 0 && al16(x) && al8(mu) && al8(sigma));
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent(N, ld, D, 4)));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_feature_mean, dim3(D / 4), dim3(ITPB), 0, s, x, N, ld, mu);
  SFRON_LAUNCH_STATUS();
  const int t = (D + CT - 1) / CT;
  hipLaunchKernelGGL(k_feature_cov, dim3(t, t), dim3(ITPB), 0, s, x, N, D, ld, (const double*)mu, sigma);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
