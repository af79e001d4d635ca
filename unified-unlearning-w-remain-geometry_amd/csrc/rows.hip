// Row-wise and elementwise pieces of the convolutional U-Net / transformer blocks on [rows][C] matrices.
//
// Replaces, for /root/reference/DDPM/models/diffusion.py and the ldm BasicTransformerBlock:
//   NCHW <-> NHWC rows and the image-byte loaders / writers;  softmax of the single-head attention (:168-186) -> k_softmax_fwd / k_softmax_bwd;
//   LayerNorm, GEGLU (SD/ldm/modules/attention.py);  per-sample column sums, the guidance mix, the backward of the nearest x2 upsampling;
//   fp32 -> bf16 casts (+ column sums), column copies (channel concatenation), dropout masks;
//   get_timestep_embedding (:17-35); classes_emb / null_classes_emb select (:370-376).
#include "common.h"
#include "../../include/sfron.h"
#include "unet_host.h"

namespace {

// rows per workgroup of the row-vectorised elementwise kernels: about 2048 workgroups over (column blocks x row chunks), >= 4 rows
inline int rows_chunk(int64_t rows, int C) {
  const int64_t cb = (C + 255) / 256;
  int64_t chunks = 2048 / cb; if (chunks < 1) chunks = 1;
  int64_t r = (rows + chunks - 1) / chunks;
  r = (r + 3) / 4 * 4;
  return (int)(r < 4 ? 4 : r);
}

// ---- layout: NCHW fp32 image <-> NHWC rows
__global__ __launch_bounds__(TPB) void k_nchw_to_rows(const float* __restrict__ x, int B, int C, int HW, int Cp, __bf16* __restrict__ rows) {
  const int64_t n = (int64_t)B * HW * Cp;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int c = (int)(i % Cp); const int64_t p = i / Cp; const int hw = (int)(p % HW); const int b = (int)(p / HW);
    rows[i] = c < C ? f2bf(x[((int64_t)b * C + c) * HW + hw]) : (__bf16)0.0f;
  }
}
// uint8 HWC images (the PIL loader's arrays) -> bf16 rows [B*H*W][Cp], Cp % 8 == 0, channels 3.. zero: ToTensor + Normalize(0.5, 0.5)
// as DiT/forget.py:200-205 computes it, (x / 255 - 0.5) / 0.5 in fp32 with true divisions, then RNE; flip[b] != 0 mirrors sample b
// (RandomHorizontalFlip: output column w reads source column W-1-w).  One thread per pixel, 16-byte stores.
__global__ __launch_bounds__(TPB) void k_image_u8_to_rows(const uint8_t* __restrict__ img, int B, int H, int W, const uint8_t* __restrict__ flip,
                                                          int Cp, __bf16* __restrict__ rows) {
  const int64_t n = (int64_t)B * H * W;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < n; p += (int64_t)gridDim.x * TPB) {
    const int w = (int)(p % W); const int64_t bh = p / W; const int b = (int)(bh / H);
    const int ws = (flip && flip[b]) ? W - 1 - w : w;
    const uint8_t* px = img + (bh * W + ws) * 3;
    bf16x8 v;
    for (int c = 0; c < 8; ++c) v[c] = (__bf16)0.0f;
    for (int c = 0; c < 3; ++c) v[c] = f2bf(((float)px[c] / 255.0f - 0.5f) / 0.5f);
    bf16x8* out = reinterpret_cast<bf16x8*>(rows + p * Cp);
    out[0] = v;
    bf16x8 z;
    for (int c = 0; c < 8; ++c) z[c] = (__bf16)0.0f;
    for (int g = 1; g < Cp / 8; ++g) out[g] = z;
  }
}
// The VAE decoder's tail: fp32 rows [B*H*W][ld] (channels 0..2 of conv_out) -> uint8 RGB, every step a separately rounded fp32 op
// (the library builds with -ffp-contract=off):
//   mode 0 (torchvision make_grid(normalize=True, value_range=(lo, hi)) + save_image):  common.h save_image_u8
//   mode 1 (diffusers / SD generate-images.py):  v = min(max(x / 2 + 0.5, 0), 1);  u = rint(v * 255)  (half to even)
//   mode 2 (DiT/sample_ddp.py:132):  u = trunc(min(max(127.5 * x + 128, 0), 255))  (the product, then the sum)
// The rows hold samples b0 .. b0+B-1 of a batch of n.  nrow == 0: out = [n][H][W][3], this launch writes its B samples.  nrow > 0: out =
// the make_grid canvas [Hc][Wc][3] (xmaps = min(nrow, n) columns, cells (H+p) x (W+p) behind a p-pixel border, n == 1: the bare image);
// one thread per canvas pixel, each launch writes the pixels of its own samples and the launch with b0 == 0 also the pad pixels (byte 0).
__device__ __forceinline__ uint8_t img_u8(float x, int mode, float lo, float hi) {
  if (mode == 0) return save_image_u8(x, lo, hi);
  if (mode == SFRON_IMAGE_TRUNC) {
    float t = 127.5f * x;
    t = t + 128.0f;
    t = fminf(fmaxf(t, 0.0f), 255.0f);
    return (uint8_t)(int)t;
  }
  float v = x / 2.0f + 0.5f;
  v = fminf(fmaxf(v, 0.0f), 1.0f);
  return (uint8_t)(int)rintf(v * 255.0f);
}
__global__ __launch_bounds__(TPB) void k_rows_to_image_u8(const float* __restrict__ rows, int ld, int B, int H, int W, int mode, float lo,
                                                          float hi, int xmaps, int pad, int Hc, int Wc, int b0, int n,
                                                          uint8_t* __restrict__ out) {
  const int64_t npx = (int64_t)Hc * Wc;
  const int ch = H + pad, cw = W + pad;
  for (int64_t q = (int64_t)blockIdx.x * TPB + threadIdx.x; q < npx; q += (int64_t)gridDim.x * TPB) {
    int k, iy, ix;
    if (xmaps == 0) {                                 // [n][H][W][3]: canvas = the B samples of this launch, one after the other
      k = b0 + (int)(q / ((int64_t)H * W));
      const int r = (int)(q % ((int64_t)H * W));
      iy = r / W; ix = r - iy * W;
    } else {
      const int y = (int)(q / Wc) - pad, x = (int)(q % Wc) - pad;
      bool img = y >= 0 && x >= 0;
      k = -1; iy = ix = 0;
      if (img) {
        const int cy = y / ch, cx = x / cw;
        iy = y - cy * ch; ix = x - cx * cw;
        k = cy * xmaps + cx;
        img = iy < H && ix < W && cx < xmaps && k < n;
      }
      if (!img) {
        if (b0 == 0) { uint8_t* o = out + q * 3; o[0] = 0; o[1] = 0; o[2] = 0; }
        continue;
      }
      if (k < b0 || k >= b0 + B) continue;
    }
    const float* px = rows + ((int64_t)(k - b0) * H * W + (int64_t)iy * W + ix) * ld;
    const int64_t at = xmaps == 0 ? ((int64_t)k * H * W + (int64_t)iy * W + ix) * 3 : q * 3;
    out[at + 0] = img_u8(px[0], mode, lo, hi);
    out[at + 1] = img_u8(px[1], mode, lo, hi);
    out[at + 2] = img_u8(px[2], mode, lo, hi);
  }
}
__global__ __launch_bounds__(TPB) void k_rows_to_nchw(const float* __restrict__ rows, int ld, int B, int C, int HW, float* __restrict__ x) {
  const int64_t n = (int64_t)B * C * HW;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int hw = (int)(i % HW); const int c = (int)((i / HW) % C); const int b = (int)(i / ((int64_t)HW * C));
    x[i] = rows[((int64_t)b * HW + hw) * ld + c];
  }
}
__global__ __launch_bounds__(TPB) void k_nchw_to_rows_f32(const float* __restrict__ x, int B, int C, int HW, int ld, float* __restrict__ rows) {
  const int64_t n = (int64_t)B * HW * ld;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int c = (int)(i % ld); const int64_t p = i / ld; const int hw = (int)(p % HW); const int b = (int)(p / HW);
    rows[i] = c < C ? x[((int64_t)b * C + c) * HW + hw] : 0.f;
  }
}


// ---- softmax over rows of length n (fp32 in, bf16 out), one wave per row; backward dS = scale * P * (dP - sum(P dP))
// rows of `n` stored elements of which the first `nv` are keys (the rest is padding of the context length: probability 0)
__global__ __launch_bounds__(TPB) void k_softmax_fwd(const float* __restrict__ s, int64_t rows, int n, int nv, float scale, __bf16* __restrict__ p) {
  const int64_t row = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* sr = s + row * n;
  float mx = -INFINITY;
  for (int i = lane; i < nv; i += 64) mx = fmaxf(mx, sr[i] * scale);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int i = lane; i < nv; i += 64) sum += __expf(sr[i] * scale - mx);
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  for (int i = lane; i < n; i += 64) p[row * n + i] = i < nv ? f2bf(__expf(sr[i] * scale - mx) * inv) : (__bf16)0.0f;
}
__global__ __launch_bounds__(TPB) void k_softmax_bwd(const __bf16* __restrict__ p, const float* __restrict__ dp, int64_t rows, int n,
                                                     float scale, __bf16* __restrict__ ds) {
  const int64_t row = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  float dot = 0.f;
  for (int i = lane; i < n; i += 64) dot += bf2f(p[row * n + i]) * dp[row * n + i];
  dot = wave_sum(dot);
  for (int i = lane; i < n; i += 64) ds[row * n + i] = f2bf(scale * bf2f(p[row * n + i]) * (dp[row * n + i] - dot));
}

// ---- LayerNorm(D, eps, affine) on rows, one wave per row (BasicTransformerBlock.norm1..3, SD/ldm/modules/attention.py:223-225)
__global__ __launch_bounds__(TPB) void k_layernorm_fwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       int64_t rows, int D, float eps, __bf16* __restrict__ y, float* __restrict__ mean,
                                                       float* __restrict__ rstd) {
  const int64_t row = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s += xr[i];
  const float m = wave_sum(s) / D;
  float q = 0.f;
  for (int i = lane; i < D; i += 64) { const float d = xr[i] - m; q += d * d; }
  const float r = rsqrtf(wave_sum(q) / D + eps);
  for (int i = lane; i < D; i += 64) y[row * D + i] = f2bf((xr[i] - m) * r * gamma[i] + beta[i]);
  if (lane == 0) { mean[row] = m; rstd[row] = r; }
}
// the same with the row in registers as float4 chunks (one 16-byte load per chunk, D <= 256 * NC, D % 4 == 0)
template <int NC>
__global__ __launch_bounds__(TPB) void k_layernorm_fwd_r(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         int64_t rows, int D, float eps, __bf16* __restrict__ y, float* __restrict__ mean,
                                                         float* __restrict__ rstd) {
  const int64_t row = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63, D4 = D >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + row * D);
  float4 v[NC];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < D4 ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  }
  const float m = wave_sum(s) / D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (lane + 64 * j < D4) {
      const float a = v[j].x - m, b = v[j].y - m, c2 = v[j].z - m, d = v[j].w - m;
      q += (a * a + b * b) + (c2 * c2 + d * d);
    }
  const float r = rsqrtf(wave_sum(q) / D + eps);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = lane + 64 * j;
    if (c < D4) {
      const float4 g4 = reinterpret_cast<const float4*>(gamma)[c], b4 = reinterpret_cast<const float4*>(beta)[c];
      reinterpret_cast<bf16x4*>(y + row * D)[c] = bf16x4{f2bf((v[j].x - m) * r * g4.x + b4.x), f2bf((v[j].y - m) * r * g4.y + b4.y),
                                                         f2bf((v[j].z - m) * r * g4.z + b4.z), f2bf((v[j].w - m) * r * g4.w + b4.w)};
    }
  }
  if (lane == 0) { mean[row] = m; rstd[row] = r; }
}
// dx (+)= d LayerNorm; pg / pb [nblk][D]: per-workgroup (4 rows) partial sums of dy * xhat and dy, written with plain stores
__global__ __launch_bounds__(TPB) void k_layernorm_bwd(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd, int64_t rows, int D,
                                                       float* __restrict__ dx, int accumulate, float* __restrict__ pg, float* __restrict__ pb,
                                                       int rows_per_block, const float* __restrict__ extra) {
  extern __shared__ float sh[];                     // [4 waves][2][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* ag = sh + (size_t)wave * 2 * D;
  float* ab = ag + D;
  for (int i = lane; i < D; i += 64) { ag[i] = 0.f; ab[i] = 0.f; }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  for (int64_t row = r0 + wave; row < r0 + rows_per_block && row < rows; row += TPB / 64) {
    const float m = mean[row], r = rstd[row];
    const float* xr = x + row * D;
    const float* dr = dy + row * D;
    float s1 = 0.f, s2 = 0.f;
    for (int i = lane; i < D; i += 64) {
      const float xh = (xr[i] - m) * r, d = dr[i] * gamma[i];
      s1 += d; s2 += d * xh;
      ag[i] += dr[i] * xh; ab[i] += dr[i];          // a lane owns its columns: no conflict inside the wave
    }
    s1 = wave_sum(s1) / D; s2 = wave_sum(s2) / D;
    for (int i = lane; i < D; i += 64) {
      const float xh = (xr[i] - m) * r;
      const float v = r * (dr[i] * gamma[i] - s1 - xh * s2);
      float* o = dx + row * D + i;
      if (extra) { const float e = extra[row * D + i]; *o = v + (accumulate ? *o + e : e); }     // (dx + extra) + this layer's gradient
      else *o = accumulate ? *o + v : v;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += TPB) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < TPB / 64; ++w) { a += sh[(size_t)w * 2 * D + i]; b += sh[(size_t)w * 2 * D + D + i]; }
    pg[(size_t)blockIdx.x * D + i] = a; pb[(size_t)blockIdx.x * D + i] = b;
  }
}
// the same with the row and the per-column accumulators in registers, a lane owning float4 column chunks (16-byte loads): x and dy are
// read once, nothing but the final per-wave sums goes through LDS.
template <int NC>      // float4 chunks per lane: D <= 256 * NC, D % 4 == 0
__global__ __launch_bounds__(TPB) void k_layernorm_bwd_r(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd, int64_t rows, int D,
                                                         float* __restrict__ dx, int accumulate, float* __restrict__ pg, float* __restrict__ pb,
                                                         int rows_per_block, const float* __restrict__ extra) {
  extern __shared__ float sh[];                     // [4 waves][2][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D4 = D >> 2;
  float4 ag[NC], ab[NC], gm[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    ag[j] = make_float4(0.f, 0.f, 0.f, 0.f); ab[j] = ag[j];
    const int c = lane + 64 * j;
    gm[j] = c < D4 ? reinterpret_cast<const float4*>(gamma)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  for (int64_t row = r0 + wave; row < r0 + rows_per_block && row < rows; row += TPB / 64) {
    const float m = mean[row], r = rstd[row];
    const float4* xr = reinterpret_cast<const float4*>(x + row * D);
    const float4* dr = reinterpret_cast<const float4*>(dy + row * D);
    float4 xh[NC], dv[NC];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = lane + 64 * j;
      const bool in = c < D4;
      const float4 xv = in ? xr[c] : make_float4(m, m, m, m);
      dv[j] = in ? dr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      xh[j] = make_float4((xv.x - m) * r, (xv.y - m) * r, (xv.z - m) * r, (xv.w - m) * r);
      // the order of k_layernorm_bwd within a lane differs (columns grouped by fours): sums are fixed-order, results reproducible
      const float d0 = dv[j].x * gm[j].x, d1 = dv[j].y * gm[j].y, d2 = dv[j].z * gm[j].z, d3 = dv[j].w * gm[j].w;
      s1 += (d0 + d1) + (d2 + d3);
      s2 += (d0 * xh[j].x + d1 * xh[j].y) + (d2 * xh[j].z + d3 * xh[j].w);
      ag[j].x += dv[j].x * xh[j].x; ag[j].y += dv[j].y * xh[j].y; ag[j].z += dv[j].z * xh[j].z; ag[j].w += dv[j].w * xh[j].w;
      ab[j].x += dv[j].x; ab[j].y += dv[j].y; ab[j].z += dv[j].z; ab[j].w += dv[j].w;
    }
    s1 = wave_sum(s1) / D; s2 = wave_sum(s2) / D;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int c = lane + 64 * j;
      if (c < D4) {
        float4 v = make_float4(r * (dv[j].x * gm[j].x - s1 - xh[j].x * s2), r * (dv[j].y * gm[j].y - s1 - xh[j].y * s2),
                               r * (dv[j].z * gm[j].z - s1 - xh[j].z * s2), r * (dv[j].w * gm[j].w - s1 - xh[j].w * s2));
        float4* o = reinterpret_cast<float4*>(dx + row * D) + c;
        if (extra) {                 // (dx + extra) + this layer's gradient: the bits of a separate dx (+)= extra pass before this one
          float4 e = reinterpret_cast<const float4*>(extra + row * D)[c];
          if (accumulate) { const float4 p = *o; e.x += p.x; e.y += p.y; e.z += p.z; e.w += p.w; }
          v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
        } else if (accumulate) { const float4 p = *o; v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w; }
        *o = v;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int c = lane + 64 * j;
    if (c < D4) {
      reinterpret_cast<float4*>(sh + (size_t)wave * 2 * D)[c] = ag[j];
      reinterpret_cast<float4*>(sh + (size_t)wave * 2 * D + D)[c] = ab[j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += TPB) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < TPB / 64; ++w) { a += sh[(size_t)w * 2 * D + i]; b += sh[(size_t)w * 2 * D + D + i]; }
    pg[(size_t)blockIdx.x * D + i] = a; pb[(size_t)blockIdx.x * D + i] = b;
  }
}
// GEGLU (attention.py:37-45): h [rows][2F] = value || gate -> out = bf16(value * gelu(gate)), exact (erf) GELU as F.gelu
__global__ __launch_bounds__(TPB) void k_geglu_fwd(const float* __restrict__ h, int64_t rows, int F, __bf16* __restrict__ out) {
  const int64_t n = rows * F;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int64_t r = i / F; const int c = (int)(i % F);
    const float a = h[r * 2 * F + c], gt = h[r * 2 * F + F + c];
    out[i] = f2bf(a * 0.5f * gt * (1.0f + erff(gt * 0.70710678118654752f)));
  }
}
// dh [rows][2F] bf16: d value = d_out * gelu(gate), d gate = d_out * value * gelu'(gate)
__global__ __launch_bounds__(TPB) void k_geglu_bwd(const float* __restrict__ d_out, const float* __restrict__ h, int64_t rows, int F,
                                                   __bf16* __restrict__ dh) {
  const int64_t n = rows * F;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int64_t r = i / F; const int c = (int)(i % F);
    const float a = h[r * 2 * F + c], gt = h[r * 2 * F + F + c], d = d_out[i];
    const float cdf = 0.5f * (1.0f + erff(gt * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * gt * gt);
    dh[r * 2 * F + c] = f2bf(d * gt * cdf);
    dh[r * 2 * F + F + c] = f2bf(d * a * (cdf + gt * pdf));
  }
}
// the same on float4 column quads, rows walked by the workgroup's y index (no per-element 64-bit division): F % 4 == 0
__global__ __launch_bounds__(TPB) void k_geglu_fwd4(const float* __restrict__ h, int64_t rows, int F, int rows_per_block, __bf16* __restrict__ out) {
  const int c = (blockIdx.x * TPB + threadIdx.x) * 4;
  if (c >= F) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  for (int64_t r = r0; r < r1; ++r) {
    const float4 a = *reinterpret_cast<const float4*>(h + r * 2 * F + c), gt = *reinterpret_cast<const float4*>(h + r * 2 * F + F + c);
    const float av[4] = {a.x, a.y, a.z, a.w}, gv[4] = {gt.x, gt.y, gt.z, gt.w};
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = f2bf(av[e] * 0.5f * gv[e] * (1.0f + erff(gv[e] * 0.70710678118654752f)));
    *reinterpret_cast<bf16x4*>(out + r * F + c) = o;
  }
}
__global__ __launch_bounds__(TPB) void k_geglu_bwd4(const float* __restrict__ d_out, const float* __restrict__ h, int64_t rows, int F, int rows_per_block,
                                                    __bf16* __restrict__ dh) {
  const int c = (blockIdx.x * TPB + threadIdx.x) * 4;
  if (c >= F) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  for (int64_t r = r0; r < r1; ++r) {
    const float4 a = *reinterpret_cast<const float4*>(h + r * 2 * F + c), gt = *reinterpret_cast<const float4*>(h + r * 2 * F + F + c);
    const float4 d4 = *reinterpret_cast<const float4*>(d_out + r * F + c);
    const float av[4] = {a.x, a.y, a.z, a.w}, gv[4] = {gt.x, gt.y, gt.z, gt.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
    bf16x4 o1, o2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float cdf = 0.5f * (1.0f + erff(gv[e] * 0.70710678118654752f));
      const float pdf = 0.3989422804014327f * expf(-0.5f * gv[e] * gv[e]);
      o1[e] = f2bf(dv[e] * gv[e] * cdf);
      o2[e] = f2bf(dv[e] * av[e] * (cdf + gv[e] * pdf));
    }
    *reinterpret_cast<bf16x4*>(dh + r * 2 * F + c) = o1;
    *reinterpret_cast<bf16x4*>(dh + r * 2 * F + F + c) = o2;
  }
}

// ---- small pieces
// out[b][c] = sum_{p < HW} x[(b * HW + p) * ld + c]  (per-sample column sums: gradient of a per-sample broadcast vector)
// one workgroup per (64-column slice, sample): the 4 waves stride over the rows (coalesced 256-B row reads), partial sums meet in LDS
// in a fixed order
// gridDim.z row chunks per sample (chunk z takes rows [HW z / nz, HW (z + 1) / nz)): with nz > 1 `out` is the partial buffer
// [B][nz][C] (ldo = C) that k_reduce_chunks adds per sample in a fixed order
__global__ __launch_bounds__(TPB) void k_sample_colsum(const float* __restrict__ x, int ld, int HW, int C, float* __restrict__ out, int ldo) {
  __shared__ float sh[TPB / 64][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int nz = gridDim.z, z = blockIdx.z;
  const int p0 = (int)((long)HW * z / nz), p1 = (int)((long)HW * (z + 1) / nz);
  float s = 0.f;
  if (c < C) {
    const float* xb = x + (size_t)b * HW * ld + c;
    for (int p = p0 + wave; p < p1; p += TPB / 64) s += xb[(size_t)p * ld];
  }
  sh[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < C) {
    float a = 0.f;
    for (int w = 0; w < TPB / 64; ++w) a += sh[w][lane];
    out[((size_t)b * nz + z) * ldo + c] = a;
  }
}
// out = alpha * a + beta * b   (classifier-free guidance mix (1 + s) cond - s null, models/diffusion.py:340-357)
__global__ __launch_bounds__(TPB) void k_axpby(const float* __restrict__ a, const float* __restrict__ b, float alpha, float beta, int64_t n,
                                               float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) out[i] = alpha * a[i] + beta * b[i];
}
// nearest x2 upsampling backward: dx[b][h][w][c] (+)= sum of the 2x2 block of dy ([B][2H][2W][C])
__global__ __launch_bounds__(TPB) void k_pool2_sum(const float* __restrict__ dy, int B, int H, int W, int C, float* __restrict__ dx, int accumulate) {
  const int64_t n = (int64_t)B * H * W * C;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int c = (int)(i % C); int64_t p = i / C; const int w = (int)(p % W); p /= W; const int h = (int)(p % H); const int b = (int)(p / H);
    const float* s = dy + (((int64_t)b * 2 * H + 2 * h) * 2 * W + 2 * w) * C + c;
    const float v = s[0] + s[C] + s[(int64_t)2 * W * C] + s[(int64_t)2 * W * C + C];
    dx[i] = accumulate ? dx[i] + v : v;
  }
}
__global__ __launch_bounds__(TPB) void k_cast_rows(const float* __restrict__ x, int ldx, int64_t rows, int C, __bf16* __restrict__ y) {
  const int64_t n = rows * C;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
    y[i] = f2bf(x[(i / C) * ldx + (i % C)]);
}
// the same with a lane per float4 of a row (no per-element division), optionally with the column sums of x (the bias gradient of
// the layer whose output gradient is being cast): grid = (ceil(C / 256), row chunks); the 4 waves of a workgroup take rows
// r0 + wave, + 4, ... and meet in LDS in a fixed order; partials[chunk][C] are added by k_reduce_chunks
template <bool SUM>
__global__ __launch_bounds__(TPB) void k_cast_rows4(const float* __restrict__ x, int ldx, int64_t rows, int C, int rows_per_block,
                                                    __bf16* __restrict__ y, float* __restrict__ partials) {
  __shared__ float sh[3][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + lane) * 4;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (col < C)
    for (int64_t r = r0 + wave; r < r1; r += TPB / 64) {
      const float4 v = *reinterpret_cast<const float4*>(x + r * ldx + col);
      *reinterpret_cast<bf16x4*>(y + r * C + col) = bf16x4{f2bf(v.x), f2bf(v.y), f2bf(v.z), f2bf(v.w)};
      if (SUM) { a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w; }
    }
  if (!SUM) return;
  if (wave > 0) { sh[wave - 1][0][lane] = a0; sh[wave - 1][1][lane] = a1; sh[wave - 1][2][lane] = a2; sh[wave - 1][3][lane] = a3; }
  __syncthreads();
  if (wave == 0 && col < C) {
    float* o = partials + (size_t)blockIdx.y * C + col;
    o[0] = ((a0 + sh[0][0][lane]) + sh[1][0][lane]) + sh[2][0][lane];
    o[1] = ((a1 + sh[0][1][lane]) + sh[1][1][lane]) + sh[2][1][lane];
    o[2] = ((a2 + sh[0][2][lane]) + sh[1][2][lane]) + sh[2][2][lane];
    o[3] = ((a3 + sh[0][3][lane]) + sh[1][3][lane]) + sh[2][3][lane];
  }
}
__global__ __launch_bounds__(TPB) void k_copy_cols4(const float* __restrict__ x, int ldx, int64_t rows, int C, float* __restrict__ y, int ldy,
                                                    int accumulate, int rows_per_block) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + lane) * 4;
  if (col >= C) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  for (int64_t r = r0 + wave; r < r1; r += TPB / 64) {
    float4 v = *reinterpret_cast<const float4*>(x + r * ldx + col);
    float4* o = reinterpret_cast<float4*>(y + r * ldy + col);
    if (accumulate) { const float4 c = *o; v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w; }
    *o = v;
  }
}
// Two column copies in ONE launch (blockIdx.z = piece): the channel concatenation torch.cat([h, skip], dim=1) of the up path (two sources into
// the column halves of one destination) and its backward (the column halves of one source into two gradient buffers, each with its own
// accumulate flag) were two launches of k_copy_cols4 each -- 5 us apiece on a chain that is bound by its launch count.
struct CopyPiece { const float* x; int ldx; float* y; int ldy; int C; int accumulate; };
__global__ __launch_bounds__(TPB) void k_copy_cols4x2(CopyPiece p0, CopyPiece p1, int64_t rows, int rows_per_block) {
  const CopyPiece p = blockIdx.z ? p1 : p0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + lane) * 4;
  if (col >= p.C) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  for (int64_t r = r0 + wave; r < r1; r += TPB / 64) {
    float4 v = *reinterpret_cast<const float4*>(p.x + r * p.ldx + col);
    float4* o = reinterpret_cast<float4*>(p.y + r * p.ldy + col);
    if (p.accumulate) { const float4 c = *o; v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w; }
    *o = v;
  }
}
// Bernoulli keep mask of nn.Dropout(p) in one launch (torch.rand >= p -> uint8 takes three): element i of mask (seed, call, salt) is
// kept when 16 bits of splitmix64(seed, counter, salt, i / 4) reach p * 65536.  `counter` lives on the device and is advanced by the
// caller once per pass, so a captured graph draws fresh masks at every replay.
__global__ __launch_bounds__(TPB) void k_dropout_mask(uint64_t seed, const int64_t* __restrict__ counter, int64_t salt, int64_t n, unsigned thresh16,
                                                      uint8_t* __restrict__ out) {
  const uint64_t base = seed ^ ((uint64_t)counter[0] * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)salt * 0xD1B54A32D192ED03ull);
  const int64_t nq = (n + 3) >> 2;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < nq; i += (int64_t)gridDim.x * TPB) {
    uint64_t z = base + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    uchar4 m;
    m.x = (unsigned)(z & 0xffff) >= thresh16; m.y = (unsigned)((z >> 16) & 0xffff) >= thresh16;
    m.z = (unsigned)((z >> 32) & 0xffff) >= thresh16; m.w = (unsigned)(z >> 48) >= thresh16;
    if (4 * i + 3 < n) *reinterpret_cast<uchar4*>(out + 4 * i) = m;
    else { const uint8_t e[4] = {m.x, m.y, m.z, m.w}; for (int k = 0; 4 * i + k < n; ++k) out[4 * i + k] = e[k]; }
  }
}
// Every dropout mask of a pass in ONE launch: item j = mask (salt, n elements) at byte offset `off` of one buffer (int64 triples [salt, n, off],
// off % 4 == 0); blockIdx.y = item.  Bit for bit the masks k_dropout_mask draws for the same (seed, counter, salt): a U-Net pass asked for one
// launch per ResnetBlock (44 launches of 5 us per DDPM SFR-on step).
__global__ __launch_bounds__(TPB) void k_dropout_mask_batch(uint64_t seed, const int64_t* __restrict__ counter, const int64_t* __restrict__ items,
                                                            unsigned thresh16, uint8_t* __restrict__ base_out) {
  const int64_t salt = items[3 * blockIdx.y], n = items[3 * blockIdx.y + 1];
  uint8_t* const out = base_out + items[3 * blockIdx.y + 2];
  const uint64_t base = seed ^ ((uint64_t)counter[0] * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)salt * 0xD1B54A32D192ED03ull);
  const int64_t nq = (n + 3) >> 2;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < nq; i += (int64_t)gridDim.x * TPB) {
    uint64_t z = base + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    uchar4 m;
    m.x = (unsigned)(z & 0xffff) >= thresh16; m.y = (unsigned)((z >> 16) & 0xffff) >= thresh16;
    m.z = (unsigned)((z >> 32) & 0xffff) >= thresh16; m.w = (unsigned)(z >> 48) >= thresh16;
    if (4 * i + 3 < n) *reinterpret_cast<uchar4*>(out + 4 * i) = m;
    else { const uint8_t e[4] = {m.x, m.y, m.z, m.w}; for (int k = 0; 4 * i + k < n; ++k) out[4 * i + k] = e[k]; }
  }
}
// y[rows][ld_y] column slice <- x[rows][C] (channel concatenation) and back (+=)
__global__ __launch_bounds__(TPB) void k_copy_cols(const float* __restrict__ x, int ldx, int64_t rows, int C, float* __restrict__ y, int ldy,
                                                   int accumulate) {
  const int64_t n = rows * C;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int64_t r = i / C; const int c = (int)(i % C);
    float* o = y + r * ldy + c;
    const float v = x[r * ldx + c];
    *o = accumulate ? *o + v : v;
  }
}
// DDPM get_timestep_embedding (models/diffusion.py:17-35): sin || cos, freq_j = exp(-ln(1e4) * j / (half - 1)); t is float
__global__ __launch_bounds__(TPB) void k_ddpm_temb(const float* __restrict__ t, int n, int dim, __bf16* __restrict__ out) {
  const int half = dim / 2;
  const float e = logf(10000.0f) / (float)(half - 1);
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n * dim; i += gridDim.x * TPB) {
    const int b = i / dim, j = i % dim;
    float v = 0.f;
    if (j < 2 * half) {
      const int jj = j < half ? j : j - half;
      const float a = t[b] * expf(-e * (float)jj);
      v = j < half ? sinf(a) : cosf(a);
    }
    out[i] = f2bf(v);
  }
}
// cemb_in[b] = keep[b] ? table[c[b]] : null_emb   (models/diffusion.py:370-376); labels outside the table read the null row
__global__ __launch_bounds__(TPB) void k_class_embed(const float* __restrict__ table, const float* __restrict__ null_emb,
                                                     const int64_t* __restrict__ c, const uint8_t* __restrict__ keep, int n_classes,
                                                     int n, int D, __bf16* __restrict__ out) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n * D; i += gridDim.x * TPB) {
    const int b = i / D, j = i % D;
    const int64_t lab = c[b];
    const bool use = (!keep || keep[b]) && lab >= 0 && lab < n_classes;
    out[i] = f2bf(use ? table[lab * D + j] : null_emb[j]);
  }
}
// d_table[c[b]] += d[b] (kept samples), d_null += d[b] (dropped): serial over the batch per column (deterministic)
__global__ __launch_bounds__(TPB) void k_class_embed_bwd(const float* __restrict__ d, const int64_t* __restrict__ c,
                                                         const uint8_t* __restrict__ keep, int n_classes, int n, int D,
                                                         float* __restrict__ d_table, float* __restrict__ d_null) {
  const int j = blockIdx.x * TPB + threadIdx.x;
  if (j >= D) return;
  float nul = 0.f;
  for (int b = 0; b < n; ++b) {
    const int64_t lab = c[b];
    const bool use = (!keep || keep[b]) && lab >= 0 && lab < n_classes;
    const float g = d[(size_t)b * D + j];
    if (use) d_table[lab * D + j] += g; else nul += g;
  }
  d_null[j] = nul;
}

}  // namespace

extern "C" {

int sfron_nchw_to_rows_bf16(const float* x, int B, int C, int HW, int c_pad, uint16_t* rows, void* stream) {
  SFRON_CHECK_ARG(x && rows && c_pad >= C);
  hipLaunchKernelGGL(k_nchw_to_rows, dim3(grid_for((int64_t)B * HW * c_pad)), dim3(TPB), 0, (hipStream_t)stream, x, B, C, HW, c_pad, (__bf16*)rows);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_image_u8_to_rows_bf16(const uint8_t* img, int B, int H, int W, const uint8_t* flip, int c_pad, uint16_t* rows, void* stream) {
  SFRON_CHECK_ARG(img && rows && B > 0 && H > 0 && W > 0 && c_pad >= 8 && c_pad % 8 == 0 && ((uintptr_t)rows & 15) == 0);
  hipLaunchKernelGGL(k_image_u8_to_rows, dim3(grid_for((int64_t)B * H * W)), dim3(TPB), 0, (hipStream_t)stream, img, B, H, W, flip, c_pad,
                     (__bf16*)rows);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_nchw_to_rows_f32(const float* x, int B, int C, int HW, int ld, float* rows, void* stream) {
  SFRON_CHECK_ARG(x && rows && ld >= C);
  hipLaunchKernelGGL(k_nchw_to_rows_f32, dim3(grid_for((int64_t)B * HW * ld)), dim3(TPB), 0, (hipStream_t)stream, x, B, C, HW, ld, rows);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_rows_to_image_u8(const float* rows, int ld, int B, int H, int W, int mode, float lo, float hi, int nrow, int padding, int b0, int n,
                           uint8_t* out, void* stream) {
  SFRON_CHECK_ARG(rows && out && ld >= 3 && B > 0 && H > 0 && W > 0 && (mode == SFRON_IMAGE_SAVE_IMAGE || mode == SFRON_IMAGE_ROUND || mode == SFRON_IMAGE_TRUNC));
  SFRON_CHECK_ARG(nrow >= 0 && padding >= 0 && b0 >= 0 && n >= b0 + B && (mode != SFRON_IMAGE_SAVE_IMAGE || hi > lo));
  int xmaps = 0, pad = 0;
  int64_t Hc, Wc;
  if (nrow > 0 && n > 1) {                      // make_grid: n == 1 returns the image itself
    xmaps = nrow < n ? nrow : n;
    const int ymaps = (n + xmaps - 1) / xmaps;
    pad = padding;
    Hc = (int64_t)ymaps * (H + pad) + pad; Wc = (int64_t)xmaps * (W + pad) + pad;
  } else if (nrow > 0) {
    xmaps = 1; Hc = H; Wc = W;                  // one cell, no border (b0 == 0, B == 1)
  } else {
    Hc = (int64_t)B * H; Wc = W;                // the B samples of this launch
  }
  SFRON_CHECK_ARG(Hc * Wc * 3 < (1ll << 31) && Hc < (1 << 30) && Wc < (1 << 30));
  hipLaunchKernelGGL(k_rows_to_image_u8, dim3(grid_for(Hc * Wc)), dim3(TPB), 0, (hipStream_t)stream, rows, ld, B, H, W, mode, lo, hi, xmaps,
                     pad, (int)Hc, (int)Wc, b0, n, out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_rows_to_nchw(const float* rows, int ld, int B, int C, int HW, float* x, void* stream) {
  SFRON_CHECK_ARG(x && rows && ld >= C);
  hipLaunchKernelGGL(k_rows_to_nchw, dim3(grid_for((int64_t)B * C * HW)), dim3(TPB), 0, (hipStream_t)stream, rows, ld, B, C, HW, x);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

// No 2 GiB limit: k_softmax_fwd / k_softmax_bwd take the row index as int64_t and form row * n in 64-bit; one wave per row, four rows per
// workgroup, so the only 32-bit quantity is the grid (rows / 4 < 2^31).  tests/test_gpu_large_shapes.py runs a score matrix above 2 GiB.
int sfron_softmax_fwd(const float* s, int64_t rows, int n, int n_valid, float scale, uint16_t* p, void* stream) {
  SFRON_CHECK_ARG(s && p && rows > 0 && n > 0 && n_valid > 0 && n_valid <= n && (rows + 3) / 4 < (1ll << 31));
  hipLaunchKernelGGL(k_softmax_fwd, dim3((unsigned)((rows + 3) / 4)), dim3(TPB), 0, (hipStream_t)stream, s, rows, n, n_valid, scale, (__bf16*)p);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_layernorm_fwd(const float* x, const float* gamma, const float* beta, int64_t rows, int D, float eps, uint16_t* y, float* mean,
                        float* rstd, void* stream) {
  SFRON_CHECK_ARG(x && gamma && beta && y && mean && rstd && rows > 0 && D > 0);
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bool v4 = D % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)gamma) | ((uintptr_t)beta)) & 15) == 0 && (((uintptr_t)y) & 7) == 0;
  if (v4 && D <= 512)       hipLaunchKernelGGL(k_layernorm_fwd_r<2>, grid, dim3(TPB), 0, (hipStream_t)stream, x, gamma, beta, rows, D, eps, (__bf16*)y, mean, rstd);
  else if (v4 && D <= 768)  hipLaunchKernelGGL(k_layernorm_fwd_r<3>, grid, dim3(TPB), 0, (hipStream_t)stream, x, gamma, beta, rows, D, eps, (__bf16*)y, mean, rstd);
  else if (v4 && D <= 1280) hipLaunchKernelGGL(k_layernorm_fwd_r<5>, grid, dim3(TPB), 0, (hipStream_t)stream, x, gamma, beta, rows, D, eps, (__bf16*)y, mean, rstd);
  else hipLaunchKernelGGL(k_layernorm_fwd, grid, dim3(TPB), 0, (hipStream_t)stream, x, gamma, beta, rows, D, eps, (__bf16*)y, mean, rstd);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
// rows per workgroup of the backward pass (= rows per partial parameter-gradient row): about 512 workgroups, 16 .. 64 rows each
int sfron_layernorm_rows_per_block(int64_t rows) {
  int64_t r = ((rows + 511) / 512 + 3) / 4 * 4;
  return (int)(r < 16 ? 16 : (r > 64 ? 64 : r));
}
int sfron_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, int64_t rows, int D, float* dx,
                        int accumulate, float* part_gamma, float* part_beta, void* stream) {
  return sfron_layernorm_bwd_res(dy, x, gamma, mean, rstd, rows, D, dx, accumulate, nullptr, part_gamma, part_beta, stream);
}
int sfron_layernorm_bwd_res(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, int64_t rows, int D, float* dx,
                            int accumulate, const float* extra, float* part_gamma, float* part_beta, void* stream) {
  // D <= 2048: the [4 waves][2][D] fp32 accumulators are dynamic LDS, 64 KiB at D = 2048 -- the most a launch gets without raising
  // MaxDynamicSharedMemorySize, which this launcher does not do (no model here has a wider LayerNorm)
  SFRON_CHECK_ARG(dy && x && gamma && mean && rstd && dx && part_gamma && part_beta && rows > 0 && D > 0 && D <= 2048);
  SFRON_CHECK_ARG(extra != dx);
  const int rpb = sfron_layernorm_rows_per_block(rows);
  const dim3 grid((unsigned)((rows + rpb - 1) / rpb));
  const size_t lds = (size_t)(TPB / 64) * 2 * D * sizeof(float);
  const bool v4 = D % 4 == 0 && ((((uintptr_t)dy) | ((uintptr_t)x) | ((uintptr_t)dx) | ((uintptr_t)gamma) | ((uintptr_t)extra)) & 15) == 0;
  if (v4 && D <= 512)       hipLaunchKernelGGL(k_layernorm_bwd_r<2>, grid, dim3(TPB), lds, (hipStream_t)stream, dy, x, gamma, mean, rstd, rows, D, dx, accumulate, part_gamma, part_beta, rpb, extra);
  else if (v4 && D <= 768)  hipLaunchKernelGGL(k_layernorm_bwd_r<3>, grid, dim3(TPB), lds, (hipStream_t)stream, dy, x, gamma, mean, rstd, rows, D, dx, accumulate, part_gamma, part_beta, rpb, extra);
  else if (v4 && D <= 1280) hipLaunchKernelGGL(k_layernorm_bwd_r<5>, grid, dim3(TPB), lds, (hipStream_t)stream, dy, x, gamma, mean, rstd, rows, D, dx, accumulate, part_gamma, part_beta, rpb, extra);
  else hipLaunchKernelGGL(k_layernorm_bwd, grid, dim3(TPB), lds, (hipStream_t)stream, dy, x, gamma, mean, rstd, rows, D, dx, accumulate, part_gamma, part_beta, rpb, extra);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_geglu_fwd(const float* h, int64_t rows, int F, uint16_t* out, void* stream) {
  SFRON_CHECK_ARG(h && out && rows > 0 && F > 0);
  if (F % 4 == 0 && ((((uintptr_t)h)) & 15) == 0 && (((uintptr_t)out) & 7) == 0) {
    const int cb = (F / 4 + TPB - 1) / TPB;
    int64_t chunks = 4096 / cb; if (chunks > rows) chunks = rows; if (chunks < 1) chunks = 1;
    const int rpb = (int)((rows + chunks - 1) / chunks);
    hipLaunchKernelGGL(k_geglu_fwd4, dim3(cb, (unsigned)((rows + rpb - 1) / rpb)), dim3(TPB), 0, (hipStream_t)stream, h, rows, F, rpb, (__bf16*)out);
    SFRON_LAUNCH_STATUS();
    return SFRON_OK;
  }
  hipLaunchKernelGGL(k_geglu_fwd, dim3(grid_for(rows * F)), dim3(TPB), 0, (hipStream_t)stream, h, rows, F, (__bf16*)out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_geglu_bwd(const float* d_out, const float* h, int64_t rows, int F, uint16_t* dh, void* stream) {
  SFRON_CHECK_ARG(d_out && h && dh && rows > 0 && F > 0);
  if (F % 4 == 0 && ((((uintptr_t)h) | ((uintptr_t)d_out)) & 15) == 0 && (((uintptr_t)dh) & 7) == 0) {
    const int cb = (F / 4 + TPB - 1) / TPB;
    int64_t chunks = 4096 / cb; if (chunks > rows) chunks = rows; if (chunks < 1) chunks = 1;
    const int rpb = (int)((rows + chunks - 1) / chunks);
    hipLaunchKernelGGL(k_geglu_bwd4, dim3(cb, (unsigned)((rows + rpb - 1) / rpb)), dim3(TPB), 0, (hipStream_t)stream, d_out, h, rows, F, rpb, (__bf16*)dh);
    SFRON_LAUNCH_STATUS();
    return SFRON_OK;
  }
  hipLaunchKernelGGL(k_geglu_bwd, dim3(grid_for(rows * F)), dim3(TPB), 0, (hipStream_t)stream, d_out, h, rows, F, (__bf16*)dh);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_softmax_bwd(const uint16_t* p, const float* dp, int64_t rows, int n, float scale, uint16_t* ds, void* stream) {
  SFRON_CHECK_ARG(p && dp && ds && rows > 0 && n > 0 && (rows + 3) / 4 < (1ll << 31));
  hipLaunchKernelGGL(k_softmax_bwd, dim3((unsigned)((rows + 3) / 4)), dim3(TPB), 0, (hipStream_t)stream, (const __bf16*)p, dp, rows, n, scale, (__bf16*)ds);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_axpby(const float* a, const float* b, float alpha, float beta, int64_t n, float* out, void* stream) {
  SFRON_CHECK_ARG(a && b && out);
  hipLaunchKernelGGL(k_axpby, dim3(grid_for(n)), dim3(TPB), 0, (hipStream_t)stream, a, b, alpha, beta, n, out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_sample_colsum(const float* x, int ld, int B, int HW, int C, float* out, int ld_out, float* scratch, int64_t scratch_floats,
                        void* stream) {
  SFRON_CHECK_ARG(x && out && ld_out >= C && B > 0 && HW > 0 && C > 0);
  // few (column block, sample) pairs and many rows: chunk the rows, partial sums [B][nz][C] in the caller's scratch, fixed-order add
  int nz = 512 / (((C + 63) / 64) * B);
  if (nz > 32) nz = 32;
  if (nz > HW / 16) nz = HW / 16;
  if (scratch && nz > 1 && (int64_t)B * nz * C <= scratch_floats) {
    hipLaunchKernelGGL(k_sample_colsum, dim3((C + 63) / 64, B, nz), dim3(TPB), 0, (hipStream_t)stream, x, ld, HW, C, scratch, C);
    SFRON_LAUNCH_STATUS();
    return sfron_reduce_chunks(scratch, B, nz, C, out, ld_out, 0, stream);
  }
  hipLaunchKernelGGL(k_sample_colsum, dim3((C + 63) / 64, B, 1), dim3(TPB), 0, (hipStream_t)stream, x, ld, HW, C, out, ld_out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_pool2_sum(const float* dy, int B, int H, int W, int C, float* dx, int accumulate, void* stream) {
  SFRON_CHECK_ARG(dy && dx);
  hipLaunchKernelGGL(k_pool2_sum, dim3(grid_for((int64_t)B * H * W * C)), dim3(TPB), 0, (hipStream_t)stream, dy, B, H, W, C, dx, accumulate);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
// No 2 GiB limit: k_cast_rows / k_cast_rows4 (and the k_copy_cols family below) carry the row as int64_t and form r * ldx in 64-bit; the
// row-chunk grid stays below 65536.  tests/test_gpu_large_shapes.py casts an activation above 2 GiB.
int sfron_cast_rows_bf16(const float* x, int ldx, int64_t rows, int C, uint16_t* y, void* stream) {
  SFRON_CHECK_ARG(x && y && ldx >= C);
  if (C % 4 == 0 && ldx % 4 == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)y) & 7) == 0) {
    const int rpb = rows_chunk(rows, C);
    hipLaunchKernelGGL((k_cast_rows4<false>), dim3((C + 255) / 256, (unsigned)((rows + rpb - 1) / rpb)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, rows, C,
                       rpb, (__bf16*)y, (float*)nullptr);
    SFRON_LAUNCH_STATUS();
    return SFRON_OK;
  }
  hipLaunchKernelGGL(k_cast_rows, dim3(grid_for(rows * C)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, rows, C, (__bf16*)y);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
/* y = bf16(x) and colsum[c] = sum_r x[r][c] in one pass over x (the output gradient of a layer: its bf16 GEMM operand and its bias
 * gradient); partials: scratch of at least max_partials * C floats */
int sfron_cast_rows_colsum(const float* x, int ldx, int64_t rows, int C, uint16_t* y, float* partials, int max_partials, float* colsum,
                           void* stream) {
  SFRON_CHECK_ARG(colsum);
  int chunks = 0;
  const int rc = sfron_cast_rows_colsum_partials(x, ldx, rows, C, y, partials, max_partials, &chunks, stream);
  if (rc) return rc;
  return sfron_reduce_chunks(partials, 1, chunks, C, colsum, C, 0, stream);
}
int sfron_cast_rows_colsum_partials(const float* x, int ldx, int64_t rows, int C, uint16_t* y, float* partials, int max_partials,
                                    int* chunks_out, void* stream) {
  SFRON_CHECK_ARG(x && y && partials && chunks_out && rows > 0 && C > 0 && ldx >= C && max_partials > 0);
  SFRON_CHECK_ARG(C % 4 == 0 && ldx % 4 == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)y) & 7) == 0);
  // about 512 workgroups over (column blocks x row chunks), at least 32 rows per chunk, within the caller's scratch
  int64_t chunks = 512 / ((C + 255) / 256);
  if (chunks > (rows + 31) / 32) chunks = (rows + 31) / 32;
  if (chunks > max_partials) chunks = max_partials;
  if (chunks < 1) chunks = 1;
  const int rpb = (int)((rows + chunks - 1) / chunks);
  chunks = (rows + rpb - 1) / rpb;
  hipLaunchKernelGGL((k_cast_rows4<true>), dim3((C + 255) / 256, (unsigned)chunks), dim3(TPB), 0, (hipStream_t)stream, x, ldx, rows, C, rpb, (__bf16*)y,
                     partials);
  SFRON_LAUNCH_STATUS();
  *chunks_out = (int)chunks;
  return SFRON_OK;
}
int sfron_dropout_mask(uint64_t seed, const int64_t* counter, int64_t salt, int64_t n, float p, uint8_t* mask, void* stream) {
  SFRON_CHECK_ARG(counter && mask && n > 0 && p >= 0.f && p < 1.f && (((uintptr_t)mask) & 3) == 0);
  const unsigned thresh = (unsigned)(p * 65536.0f + 0.5f);
  hipLaunchKernelGGL(k_dropout_mask, dim3(grid_for((n + 3) / 4)), dim3(TPB), 0, (hipStream_t)stream, seed, counter, salt, n, thresh, mask);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_dropout_mask_batch(uint64_t seed, const int64_t* counter, const int64_t* items_dev, int n_items, int64_t max_n, float p, uint8_t* mask_base,
                             void* stream) {
  SFRON_CHECK_ARG(counter && items_dev && mask_base && n_items > 0 && n_items <= 65535 && max_n > 0 && p >= 0.f && p < 1.f &&
                  (((uintptr_t)mask_base) & 3) == 0);
  const unsigned thresh = (unsigned)(p * 65536.0f + 0.5f);
  int gx = grid_for((max_n + 3) / 4);
  if (gx > 64) gx = 64;                         // n_items rows of workgroups fill the chip
  hipLaunchKernelGGL(k_dropout_mask_batch, dim3(gx, n_items), dim3(TPB), 0, (hipStream_t)stream, seed, counter, items_dev, thresh, mask_base);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_copy_cols(const float* x, int ldx, int64_t rows, int C, float* y, int ldy, int accumulate, void* stream) {
  SFRON_CHECK_ARG(x && y && ldx >= C && ldy >= C);
  if (C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0) {
    const int rpb = rows_chunk(rows, C);
    hipLaunchKernelGGL(k_copy_cols4, dim3((C + 255) / 256, (unsigned)((rows + rpb - 1) / rpb)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, rows, C, y, ldy,
                       accumulate, rpb);
    SFRON_LAUNCH_STATUS();
    return SFRON_OK;
  }
  hipLaunchKernelGGL(k_copy_cols, dim3(grid_for(rows * C)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, rows, C, y, ldy, accumulate);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_copy_cols2(const float* x0, int ldx0, int C0, float* y0, int ldy0, int acc0, const float* x1, int ldx1, int C1, float* y1, int ldy1,
                     int acc1, int64_t rows, void* stream) {
  SFRON_CHECK_ARG(x0 && y0 && x1 && y1 && rows > 0 && C0 > 0 && C1 > 0 && ldx0 >= C0 && ldy0 >= C0 && ldx1 >= C1 && ldy1 >= C1);
  const bool wide = ((C0 | C1 | ldx0 | ldx1 | ldy0 | ldy1) & 3) == 0 &&
                    ((((uintptr_t)x0) | ((uintptr_t)y0) | ((uintptr_t)x1) | ((uintptr_t)y1)) & 15) == 0;
  if (!wide) {                                   // unaligned shapes: the two plain launches
    const int rc = sfron_copy_cols(x0, ldx0, rows, C0, y0, ldy0, acc0, stream);
    return rc != SFRON_OK ? rc : sfron_copy_cols(x1, ldx1, rows, C1, y1, ldy1, acc1, stream);
  }
  const int Cm = C0 > C1 ? C0 : C1;
  const int rpb = rows_chunk(rows, Cm);
  hipLaunchKernelGGL(k_copy_cols4x2, dim3((Cm + 255) / 256, (unsigned)((rows + rpb - 1) / rpb), 2), dim3(TPB), 0, (hipStream_t)stream,
                     CopyPiece{x0, ldx0, y0, ldy0, C0, acc0}, CopyPiece{x1, ldx1, y1, ldy1, C1, acc1}, rows, rpb);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_ddpm_timestep_embed(const float* t, int n, int dim, uint16_t* out, void* stream) {
  SFRON_CHECK_ARG(t && out && dim >= 4);
  hipLaunchKernelGGL(k_ddpm_temb, dim3(grid_for((int64_t)n * dim)), dim3(TPB), 0, (hipStream_t)stream, t, n, dim, (__bf16*)out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_class_embed_fwd(const float* table, const float* null_emb, const int64_t* c, const uint8_t* keep, int n_classes, int n, int D,
                          uint16_t* out, void* stream) {
  SFRON_CHECK_ARG(table && null_emb && c && out);
  hipLaunchKernelGGL(k_class_embed, dim3(grid_for((int64_t)n * D)), dim3(TPB), 0, (hipStream_t)stream, table, null_emb, c, keep, n_classes, n, D,
                     (__bf16*)out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_class_embed_bwd(const float* d, const int64_t* c, const uint8_t* keep, int n_classes, int n, int D, float* d_table, float* d_null,
                          void* stream) {
  SFRON_CHECK_ARG(d && c && d_table && d_null);
  hipLaunchKernelGGL(k_class_embed_bwd, dim3((D + TPB - 1) / TPB), dim3(TPB), 0, (hipStream_t)stream, d, c, keep, n_classes, n, D, d_table, d_null);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
