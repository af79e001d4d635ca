// GroupNorm of the convolutional U-Net blocks (DDPM Conditional_Model; the same blocks serve the LDM UNetModel and the VAE).
//
// Replaces, for /root/reference/DDPM/models/diffusion.py:
//   GroupNorm(32, eps 1e-6) (+ swish, + dropout) forward / backward (:43-46,38-40,126-131)
// in three forms on NHWC fp32 rows: one workgroup per (sample, group) (k_gn_fwd / k_gn_bwd: odd shapes), the row-coalesced two-phase
// pair (k_gn2_*), and one launch per direction (k_gn3_*), which can also take its input as the unfinished split-K slabs of the
// convolution in front of it (sfron_split_src; conv.hip sfron_conv_fwd leaves them, sfron_split_finish is the plain finish).
#include "common.h"
#include <cstdlib>
#include "../../include/sfron.h"
#include "unet_host.h"

namespace {

// ---- GroupNorm(G groups, eps) (+ swish) (+ dropout mask) on NHWC rows, one workgroup per (sample, group)
// y = bf16( act(xhat * gamma + beta) * (mask ? mask * drop_scale : 1) ), xhat = (x - mean) * rstd; saves mean / rstd
__global__ __launch_bounds__(TPB) void k_gn_fwd(const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, int HW, int C, int G, float eps, int swish,
                                                const uint8_t* __restrict__ mask, float drop_scale, __bf16* __restrict__ y,
                                                float* __restrict__ mean, float* __restrict__ rstd) {
  __shared__ double red[2][TPB / 64];
  __shared__ float stat[2];
  const int b = blockIdx.x / G, gi = blockIdx.x % G, cg = C / G;
  const float* xb = x + (size_t)b * HW * ldx + gi * cg;
  const int n = HW * cg;
  // thread (slot, c) = (tid / cg, tid % cg) walks the pixels slot, slot + tpc, ... of its channel (no per-element division)
  const int tpc = TPB / cg, slot = threadIdx.x / cg, c = threadIdx.x - slot * cg;
  double s = 0.0, ss = 0.0;
  if (slot < tpc)
    for (int p = slot; p < HW; p += tpc) {
      const float v = xb[(size_t)p * ldx + c];
      s += v; ss += (double)v * v;
    }
  s = wave_sum_d(s); ss = wave_sum_d(ss);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = ss; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0, q = 0;
    for (int w = 0; w < TPB / 64; ++w) { a += red[0][w]; q += red[1][w]; }
    const double m = a / n;
    double var = q / n - m * m;                 // biased variance, as torch.nn.GroupNorm
    var = var < 0 ? 0 : var;
    stat[0] = (float)m; stat[1] = (float)(1.0 / sqrt(var + (double)eps));
    mean[blockIdx.x] = stat[0]; rstd[blockIdx.x] = stat[1];
  }
  __syncthreads();
  const float m = stat[0], r = stat[1];
  __bf16* yb = y + (size_t)b * HW * C + gi * cg;
  const uint8_t* mb = mask ? mask + (size_t)b * HW * C + gi * cg : nullptr;
  if (slot < tpc) {
    const float ga = gamma[gi * cg + c], be = beta[gi * cg + c];
    for (int p = slot; p < HW; p += tpc) {
      float z = (xb[(size_t)p * ldx + c] - m) * r * ga + be;
      if (swish) z = silu(z);
      if (mb) z = mb[(size_t)p * C + c] ? z * drop_scale : 0.f;
      yb[(size_t)p * C + c] = f2bf(z);
    }
  }
}
// backward: dy = gradient wrt the bf16 output (fp32 rows, ld = C); dx (+)= d GroupNorm; per-sample partial parameter
// gradients pg[b][C], pb[b][C] (summed over the batch by sfron_reduce_chunks: fixed order)
__global__ __launch_bounds__(TPB) void k_gn_bwd(const float* __restrict__ dy, const float* __restrict__ x, int ldx,
                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                const float* __restrict__ mean, const float* __restrict__ rstd, int HW, int C, int G,
                                                int swish, const uint8_t* __restrict__ mask, float drop_scale,
                                                float* __restrict__ dx, int lddx, int accumulate, float* __restrict__ pg,
                                                float* __restrict__ pb) {
  extern __shared__ float sh[];                 // [TPB/64][2] wave partials + per-channel [2][cg] accumulators
  const int b = blockIdx.x / G, gi = blockIdx.x % G, cg = C / G;
  float* chs = sh + 2 * (TPB / 64);             // [2][cg]: sum dz * xhat, sum dz   per channel
  const float m = mean[blockIdx.x], r = rstd[blockIdx.x];
  const float* xb = x + (size_t)b * HW * ldx + gi * cg;
  const float* dyb = dy + (size_t)b * HW * C + gi * cg;
  const uint8_t* mb = mask ? mask + (size_t)b * HW * C + gi * cg : nullptr;
  const int n = HW * cg;
  // pass 1: dz = dy * act'(z) (* dropout); group sums of dz * gamma and dz * gamma * xhat; per-channel sums.
  // Thread (slot, c) = (tid / cg, tid % cg) owns channel c and visits the pixels slot, slot + tpc, ... (tpc = TPB / cg slots; the
  // TPB - tpc * cg surplus threads idle here): consecutive threads still read consecutive addresses of a pixel's cg-channel run, and
  // every per-channel sum is formed in a fixed order (no atomics: bitwise reproducible for any channels-per-group <= TPB).
  float s1 = 0.f, s2 = 0.f;
  float ca = 0.f, cb = 0.f;
  const int tpc = TPB / cg, slot = threadIdx.x / cg, c = threadIdx.x - slot * cg;
  if (slot < tpc) {
    const float ga = gamma[gi * cg + c], be = beta[gi * cg + c];
    for (int p = slot; p < HW; p += tpc) {
      const float xh = (xb[(size_t)p * ldx + c] - m) * r;
      float d = dyb[(size_t)p * C + c];
      if (mb) d = mb[(size_t)p * C + c] ? d * drop_scale : 0.f;
      if (swish) d *= silu_grad(xh * ga + be);
      s1 += d * ga; s2 += d * ga * xh;
      ca += d * xh; cb += d;
    }
  }
  float* tmp = sh + 2 * (TPB / 64) + 2 * cg;     // [2][TPB]
  tmp[threadIdx.x] = ca; tmp[TPB + threadIdx.x] = cb;
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = s1; sh[TPB / 64 + (threadIdx.x >> 6)] = s2; }
  __syncthreads();
  if (threadIdx.x < cg) {
    float a = 0.f, q = 0.f;
    for (int j = threadIdx.x; j < tpc * cg; j += cg) { a += tmp[j]; q += tmp[TPB + j]; }
    chs[threadIdx.x] = a; chs[cg + threadIdx.x] = q;
  }
  float t1 = 0.f, t2 = 0.f;
  for (int w = 0; w < TPB / 64; ++w) { t1 += sh[w]; t2 += sh[TPB / 64 + w]; }
  __syncthreads();
  if (threadIdx.x < cg) {
    pg[(size_t)b * C + gi * cg + threadIdx.x] = chs[threadIdx.x];
    pb[(size_t)b * C + gi * cg + threadIdx.x] = chs[cg + threadIdx.x];
  }
  const float inv = 1.0f / (float)n;
  const float k1 = t1 * inv, k2 = t2 * inv;
  float* dxb = dx + (size_t)b * HW * lddx + gi * cg;
  if (slot < tpc) {
    const float ga = gamma[gi * cg + c], be = beta[gi * cg + c];
    for (int p = slot; p < HW; p += tpc) {
      const float xh = (xb[(size_t)p * ldx + c] - m) * r;
      float d = dyb[(size_t)p * C + c];
      if (mb) d = mb[(size_t)p * C + c] ? d * drop_scale : 0.f;
      if (swish) d *= silu_grad(xh * ga + be);
      const float v = r * (d * ga - k1 - xh * k2);
      float* o = dxb + (size_t)p * lddx + c;
      *o = accumulate ? *o + v : v;
    }
  }
}

// ---- GroupNorm, row-coalesced two-phase form (the production path; the per-(sample, group) kernels above serve odd shapes).
// NHWC rows: a (sample, group) slab is HW runs of cg floats, 4 * C bytes apart -- a workgroup per slab touches 16..40 useful bytes of
// every 128-B line.  Here a workgroup owns a CHUNK OF PIXELS of one sample and all C channels: threads read whole rows as float4
// (thread = (row replica r, quad lane q); C / 4 quads per row, up to three quads per thread for C > 1024), so every load is a
// full-line stream.  Phase 1 leaves per-chunk partial sums, phase 2 (same chunking) combines them in a fixed order in its
// prologue and applies the normalisation; all per-channel / per-group sums are formed in a fixed order (bitwise reproducible).
constexpr int GNB = 1024;                       // 16 waves per workgroup: with one workgroup per (sample, chunk) the chip is only full this way
constexpr int GN_MAXQ = 1;                      // quads per thread: C <= 4 * GNB = 4096
struct GnMap {
  int qpr, qw, rpp, r, ql, nq;                  // quads per row, quad lanes, rows per pass, this thread's row replica / lane, its quads
  __device__ __forceinline__ void init(int C) {
    qpr = C >> 2; qw = qpr < GNB ? qpr : GNB; rpp = GNB / qw;
    r = threadIdx.x / qw; ql = threadIdx.x - r * qw; nq = (qpr - ql + qw - 1) / qw;
    if (r >= rpp) nq = 0;
  }
};
__host__ __device__ inline int gn_chunks(int B, int HW) {
  int n = (512 + B - 1) / B;
  if (n > 32) n = 32;
  if (n > HW / 8) n = HW / 8;
  return n < 1 ? 1 : n;
}

// phase 1 forward: partial (sum, sum of squares) per (sample, chunk, group), fp64
__global__ __launch_bounds__(GNB) void k_gn2_stats(const float* __restrict__ x, int ldx, int HW, int C, int G, int nchunk, double* __restrict__ part) {
  extern __shared__ double shd[];               // [rpp][C][2]
  const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk, cg = C / G;
  const int p0 = (int)((long)HW * ch / nchunk), p1 = (int)((long)HW * (ch + 1) / nchunk);
  GnMap m; m.init(C);
  double s[GN_MAXQ][4], ss[GN_MAXQ][4];
#pragma unroll
  for (int j = 0; j < GN_MAXQ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) { s[j][e] = 0.0; ss[j][e] = 0.0; }
  const float* xb = x + (size_t)b * HW * ldx;
  for (int p = p0 + m.r; p < p1; p += m.rpp) {
#pragma unroll
    for (int j = 0; j < GN_MAXQ; ++j)
      if (j < m.nq) {
        const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx + 4 * (m.ql + j * m.qw));
        s[j][0] += v.x; ss[j][0] += (double)v.x * v.x; s[j][1] += v.y; ss[j][1] += (double)v.y * v.y;
        s[j][2] += v.z; ss[j][2] += (double)v.z * v.z; s[j][3] += v.w; ss[j][3] += (double)v.w * v.w;
      }
  }
  if (m.r < m.rpp) {
#pragma unroll
    for (int j = 0; j < GN_MAXQ; ++j)
      if (j < m.nq)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * (m.ql + j * m.qw) + e;
          shd[((size_t)m.r * C + c) * 2] = s[j][e]; shd[((size_t)m.r * C + c) * 2 + 1] = ss[j][e];
        }
  }
  __syncthreads();
  // one wave per group at a time: lane l adds the words l, l + 64, ... of the group's [rpp][cg] block in index order, then a butterfly
  // over the lanes -- a fixed order (bitwise reproducible).  (Was: G threads walking rpp * cg words each, 256 dependent LDS reads
  // = most of the kernel at the small levels.)
  const int lane = threadIdx.x & 63, nw = GNB / 64, per = m.rpp * cg;
  for (int g = threadIdx.x >> 6; g < G; g += nw) {
    double a = 0.0, q = 0.0;
    for (int i = lane; i < per; i += 64) {
      const int r = i / cg, c = g * cg + (i - r * cg);
      a += shd[((size_t)r * C + c) * 2]; q += shd[((size_t)r * C + c) * 2 + 1];
    }
    a = wave_sum_d(a); q = wave_sum_d(q);
    if (lane == 0) { double* o = part + (((size_t)b * nchunk + ch) * G + g) * 2; o[0] = a; o[1] = q; }
  }
}
// phase 2 forward: mean / rstd from the partials (every workgroup of a sample forms them the same way; chunk 0 stores them), apply
__global__ __launch_bounds__(GNB) void k_gn2_apply(const float* __restrict__ x, int ldx, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   int HW, int C, int G, float eps, int swish, const uint8_t* __restrict__ mask, float drop_scale,
                                                   int nchunk, const double* __restrict__ part, __bf16* __restrict__ y, float* __restrict__ mean,
                                                   float* __restrict__ rstd) {
  __shared__ float st[2][64];
  __shared__ double sp[32 * 64 * 2];            // [chunk][group][2]: every partial of the sample, fetched by nchunk * G threads at once
  const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk, cg = C / G;
  for (int i = threadIdx.x; i < nchunk * G * 2; i += GNB) sp[i] = part[(size_t)b * nchunk * G * 2 + i];
  __syncthreads();
  if (threadIdx.x < G) {
    double a = 0.0, q = 0.0;
    for (int k = 0; k < nchunk; ++k) { const double* o = sp + ((size_t)k * G + threadIdx.x) * 2; a += o[0]; q += o[1]; }
    const double n = (double)HW * cg, mu = a / n;
    double var = q / n - mu * mu;                 // biased variance, as torch.nn.GroupNorm
    var = var < 0 ? 0 : var;
    st[0][threadIdx.x] = (float)mu; st[1][threadIdx.x] = (float)(1.0 / sqrt(var + (double)eps));
    if (ch == 0) { mean[b * G + threadIdx.x] = st[0][threadIdx.x]; rstd[b * G + threadIdx.x] = st[1][threadIdx.x]; }
  }
  __syncthreads();
  const int p0 = (int)((long)HW * ch / nchunk), p1 = (int)((long)HW * (ch + 1) / nchunk);
  GnMap m; m.init(C);
  float mu[GN_MAXQ][4], rs[GN_MAXQ][4], ga[GN_MAXQ][4], be[GN_MAXQ][4];
#pragma unroll
  for (int j = 0; j < GN_MAXQ; ++j)
    if (j < m.nq)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * (m.ql + j * m.qw) + e, gi = c / cg;
        mu[j][e] = st[0][gi]; rs[j][e] = st[1][gi]; ga[j][e] = gamma[c]; be[j][e] = beta[c];
      }
  const float* xb = x + (size_t)b * HW * ldx;
  __bf16* yb = y + (size_t)b * HW * C;
  const uint8_t* mb = mask ? mask + (size_t)b * HW * C : nullptr;
  for (int p = p0 + m.r; p < p1; p += m.rpp) {
#pragma unroll
    for (int j = 0; j < GN_MAXQ; ++j)
      if (j < m.nq) {
        const int c0 = 4 * (m.ql + j * m.qw);
        const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx + c0);
        float z[4] = {v.x, v.y, v.z, v.w};
        uchar4 mk = make_uchar4(1, 1, 1, 1);
        if (mb) mk = *reinterpret_cast<const uchar4*>(mb + (size_t)p * C + c0);
        const uint8_t mke[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = (z[e] - mu[j][e]) * rs[j][e] * ga[j][e] + be[j][e];
          if (swish) t = silu(t);
          if (mb) t = mke[e] ? t * drop_scale : 0.f;
          z[e] = t;
        }
        *reinterpret_cast<bf16x4*>(yb + (size_t)p * C + c0) = bf16x4{f2bf(z[0]), f2bf(z[1]), f2bf(z[2]), f2bf(z[3])};
      }
  }
}
// phase 1 backward: per (sample, chunk, channel) partial sums of dz * xhat and dz, dz = dy * act'(z) (* dropout)
__global__ __launch_bounds__(GNB) void k_gn2_bwd_stats(const float* __restrict__ dy, const float* __restrict__ x, int ldx,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd, int HW, int C, int G,
                                                       int swish, const uint8_t* __restrict__ mask, float drop_scale, int nchunk,
                                                       float* __restrict__ part) {
  extern __shared__ float shf[];                // [rpp][C][2]
  const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk, cg = C / G;
  const int p0 = (int)((long)HW * ch / nchunk), p1 = (int)((long)HW * (ch + 1) / nchunk);
  GnMap m; m.init(C);
  float mu[GN_MAXQ][4], rs[GN_MAXQ][4], ga[GN_MAXQ][4], be[GN_MAXQ][4], ca[GN_MAXQ][4], cb[GN_MAXQ][4];
#pragma unroll
  for (int j = 0; j < GN_MAXQ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ca[j][e] = 0.f; cb[j][e] = 0.f;
      if (j < m.nq) {
        const int c = 4 * (m.ql + j * m.qw) + e, gi = c / cg;
        mu[j][e] = mean[b * G + gi]; rs[j][e] = rstd[b * G + gi]; ga[j][e] = gamma[c]; be[j][e] = beta[c];
      }
    }
  const float* xb = x + (size_t)b * HW * ldx;
  const float* dyb = dy + (size_t)b * HW * C;
  const uint8_t* mb = mask ? mask + (size_t)b * HW * C : nullptr;
  for (int p = p0 + m.r; p < p1; p += m.rpp) {
#pragma unroll
    for (int j = 0; j < GN_MAXQ; ++j)
      if (j < m.nq) {
        const int c0 = 4 * (m.ql + j * m.qw);
        const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx + c0);
        const float4 dv = *reinterpret_cast<const float4*>(dyb + (size_t)p * C + c0);
        uchar4 mk = make_uchar4(1, 1, 1, 1);
        if (mb) mk = *reinterpret_cast<const uchar4*>(mb + (size_t)p * C + c0);
        const float xv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {dv.x, dv.y, dv.z, dv.w};
        const uint8_t mke[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = (xv[e] - mu[j][e]) * rs[j][e];
          float d = dd[e];
          if (mb) d = mke[e] ? d * drop_scale : 0.f;
          if (swish) d *= silu_grad(xh * ga[j][e] + be[j][e]);
          ca[j][e] += d * xh; cb[j][e] += d;
        }
      }
  }
  if (m.r < m.rpp) {
#pragma unroll
    for (int j = 0; j < GN_MAXQ; ++j)
      if (j < m.nq)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * (m.ql + j * m.qw) + e;
          shf[((size_t)m.r * C + c) * 2] = ca[j][e]; shf[((size_t)m.r * C + c) * 2 + 1] = cb[j][e];
        }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += GNB) {
    float a = 0.f, q = 0.f;
    for (int r = 0; r < m.rpp; ++r) { a += shf[((size_t)r * C + c) * 2]; q += shf[((size_t)r * C + c) * 2 + 1]; }
    float* o = part + (((size_t)b * nchunk + ch) * C + c) * 2;
    o[0] = a; o[1] = q;
  }
}
// phase 2 backward: per-channel sums over the chunks -> (chunk 0) the per-sample parameter-gradient partials, the group means
// k1 = mean(dz gamma), k2 = mean(dz gamma xhat); dx (+)= rstd (dz gamma - k1 - xhat k2)
__global__ __launch_bounds__(GNB) void k_gn2_bwd_apply(const float* __restrict__ dy, const float* __restrict__ x, int ldx,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd, int HW, int C, int G,
                                                       int swish, const uint8_t* __restrict__ mask, float drop_scale, int nchunk,
                                                       const float* __restrict__ part, float* __restrict__ dx, int lddx, int accumulate,
                                                       float* __restrict__ pg, float* __restrict__ pb, const float* __restrict__ extra,
                                                       int ldextra, __bf16* __restrict__ dx16, float* __restrict__ colpart) {
  // dx16 / colpart (sfron_groupnorm_bwd_cast): the gradient also (or only: dx == nullptr) as the bf16 GEMM operand [rows][C] of the
  // convolution that produced x, and its column sums per (sample, chunk) -- that layer's bias gradient and, per sample, the gradient
  // of a per-sample vector added to x -- which a cast pass and two column-sum passes over an fp32 dx would form otherwise
  extern __shared__ float shf[];                // [C][2] channel sums, then [G][2] group means
  const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk, cg = C / G;
  float* kk = shf + 2 * C;
  float* sg = kk + 2 * G;                       // gamma, staged for the group sums below
  for (int c = threadIdx.x; c < C; c += GNB) {
    float a = 0.f, q = 0.f;
    sg[c] = gamma[c];
    for (int k0 = 0; k0 < nchunk; k0 += 8) {    // eight partial pairs in flight (a load-use loop pays one L2 latency per chunk)
      float2 t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + u < nchunk ? k0 + u : nchunk - 1;
        t[u] = *reinterpret_cast<const float2*>(part + (((size_t)b * nchunk + k) * C + c) * 2);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u < nchunk) { a += t[u].x; q += t[u].y; }
    }
    shf[2 * c] = a; shf[2 * c + 1] = q;
    if (ch == 0) { pg[(size_t)b * C + c] = a; pb[(size_t)b * C + c] = q; }
  }
  __syncthreads();
  if (threadIdx.x < G) {
    float t1 = 0.f, t2 = 0.f;
    for (int c = threadIdx.x * cg; c < (threadIdx.x + 1) * cg; ++c) { const float g1 = sg[c]; t1 += g1 * shf[2 * c + 1]; t2 += g1 * shf[2 * c]; }
    const float inv = 1.0f / ((float)HW * (float)cg);
    kk[2 * threadIdx.x] = t1 * inv; kk[2 * threadIdx.x + 1] = t2 * inv;
  }
  __syncthreads();
  const int p0 = (int)((long)HW * ch / nchunk), p1 = (int)((long)HW * (ch + 1) / nchunk);
  GnMap m; m.init(C);
  float mu[GN_MAXQ][4], rs[GN_MAXQ][4], ga[GN_MAXQ][4], be[GN_MAXQ][4], k1[GN_MAXQ][4], k2[GN_MAXQ][4];
#pragma unroll
  for (int j = 0; j < GN_MAXQ; ++j)
    if (j < m.nq)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * (m.ql + j * m.qw) + e, gi = c / cg;
        mu[j][e] = mean[b * G + gi]; rs[j][e] = rstd[b * G + gi]; ga[j][e] = gamma[c]; be[j][e] = beta[c];
        k1[j][e] = kk[2 * gi]; k2[j][e] = kk[2 * gi + 1];
      }
  const float* xb = x + (size_t)b * HW * ldx;
  const float* dyb = dy + (size_t)b * HW * C;
  const uint8_t* mb = mask ? mask + (size_t)b * HW * C : nullptr;
  float* dxb = dx ? dx + (size_t)b * HW * lddx : nullptr;
  __bf16* d16b = dx16 ? dx16 + (size_t)b * HW * C : nullptr;
  const float* exb = extra ? extra + (size_t)b * HW * ldextra : nullptr;
  float cs[GN_MAXQ][4];
#pragma unroll
  for (int j = 0; j < GN_MAXQ; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) cs[j][e] = 0.f;
  for (int p = p0 + m.r; p < p1; p += m.rpp) {
#pragma unroll
    for (int j = 0; j < GN_MAXQ; ++j)
      if (j < m.nq) {
        const int c0 = 4 * (m.ql + j * m.qw);
        const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx + c0);
        const float4 dv = *reinterpret_cast<const float4*>(dyb + (size_t)p * C + c0);
        uchar4 mk = make_uchar4(1, 1, 1, 1);
        if (mb) mk = *reinterpret_cast<const uchar4*>(mb + (size_t)p * C + c0);
        const float xv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {dv.x, dv.y, dv.z, dv.w};
        const uint8_t mke[4] = {mk.x, mk.y, mk.z, mk.w};
        float4* op = dxb ? reinterpret_cast<float4*>(dxb + (size_t)p * lddx + c0) : nullptr;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (accumulate) { const float4 c = *op; o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w; }
        if (exb) {             // the term a separate dx (+)= extra pass would have added first: (dx + extra) + this layer's gradient
          const float4 c = *reinterpret_cast<const float4*>(exb + (size_t)p * ldextra + c0);
          o[0] += c.x; o[1] += c.y; o[2] += c.z; o[3] += c.w;
        }
        const bool acc = accumulate || exb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = (xv[e] - mu[j][e]) * rs[j][e];
          float d = dd[e];
          if (mb) d = mke[e] ? d * drop_scale : 0.f;
          if (swish) d *= silu_grad(xh * ga[j][e] + be[j][e]);
          const float vv = rs[j][e] * (d * ga[j][e] - k1[j][e] - xh * k2[j][e]);
          o[e] = acc ? o[e] + vv : vv;
        }
        if (op) *op = make_float4(o[0], o[1], o[2], o[3]);
        if (d16b) *reinterpret_cast<bf16x4*>(d16b + (size_t)p * C + c0) = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
        if (colpart) {
#pragma unroll
          for (int e = 0; e < 4; ++e) cs[j][e] += o[e];
        }
      }
  }
  if (colpart) {                                // the row replicas' column sums meet in LDS in replica order (fixed order)
    float* red = shf + 3 * C + 2 * G;           // [rpp][C]
    if (m.r < m.rpp) {
#pragma unroll
      for (int j = 0; j < GN_MAXQ; ++j)
        if (j < m.nq)
#pragma unroll
          for (int e = 0; e < 4; ++e) red[(size_t)m.r * C + 4 * (m.ql + j * m.qw) + e] = cs[j][e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += GNB) {
      float a = 0.f;
      for (int r = 0; r < m.rpp; ++r) a += red[(size_t)r * C + c];
      colpart[((size_t)b * nchunk + ch) * C + c] = a;
    }
  }
}

// ---- GroupNorm in ONE launch per direction (round 6): a workgroup owns one sample and a block of `gpb` whole groups = Cs = gpb * C / G
// consecutive channels over ALL pixels -- statistics and normalisation never leave the workgroup, so the two phases of the k_gn2 pair (and the
// ~5 us boundary between two dependent launches, which at the 16 x 16 ... 4 x 4 levels of the DDPM U-Net is as long as either phase) become
// two passes of one kernel over a slab of at most 128 KB that the second pass finds in L2.  B * G / gpb workgroups (DDPM batch 64: 256 .. 1024):
// the chip stays full, which one workgroup per sample (round 5, profiles/r05_ab_log.txt) did not manage.  Rows are runs of Cs floats
// (>= 64 bytes), read as float4 by (row replica r, quad q) threads.  The same arithmetic per element as k_gn2_*; the sums run over this
// workgroup's rows in a fixed order (replica r takes rows r, r + rpp, ...; replicas, then channels, are added in index order): bitwise
// reproducible, not bit-identical to the chunked pair.
constexpr int GN3_T = 1024;
// the GroupNorm INPUT (forward: x, backward: dy) as the still unfinished result of a split-K product (round 6): n slabs [rows][C] to be added in
// index order, + bias[c] + vec[sample][c] + resid[row][c] -- element for element what k_split_finish4 writes.  The one-launch kernels form each
// element in their first pass, store it to the tensor the finish launch would have filled (their own second pass and every later reader find
// it there), and the finish launch between the product and the GroupNorm no longer exists.  slabs == nullptr: the input is a finished tensor.
struct Gn3Src {
  const float* slabs; int n; int64_t stride;
  const float* bias; const float* vec; int ldvec; const float* resid; int ldresid;
};
__device__ __forceinline__ float4 gn3_src_quad(const Gn3Src& s, int64_t row, int b, int c, int C) {
  const float* p = s.slabs + row * C + c;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  int sl = 0;
  for (; sl + 4 <= s.n; sl += 4) {                // four slab loads in flight, added in slab order
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(p + (sl + u) * s.stride);
#pragma unroll
    for (int u = 0; u < 4; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
  }
  for (; sl < s.n; ++sl) { const float4 v = *reinterpret_cast<const float4*>(p + sl * s.stride); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
  float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s.bias) b4 = *reinterpret_cast<const float4*>(s.bias + c);
  a.x += b4.x; a.y += b4.y; a.z += b4.z; a.w += b4.w;
  if (s.vec) { const float4 v = *reinterpret_cast<const float4*>(s.vec + (int64_t)b * s.ldvec + c); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
  if (s.resid) { const float4 v = *reinterpret_cast<const float4*>(s.resid + row * s.ldresid + c); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
  return a;
}
struct Gn3Map {
  int b, g0, c0, Cs, qpr, rpp, q, r;
  bool on;
  __device__ __forceinline__ void init(int C, int G, int gpb) {
    const int ncb = G / gpb, cg = C / G;
    b = blockIdx.x / ncb;
    g0 = (blockIdx.x - b * ncb) * gpb; c0 = g0 * cg; Cs = gpb * cg; qpr = Cs >> 2; rpp = GN3_T / qpr;
    r = threadIdx.x / qpr; q = threadIdx.x - r * qpr; on = r < rpp;
  }
};
template <bool SRC>
__global__ __launch_bounds__(GN3_T) void k_gn3_fwd(const float* __restrict__ x, int ldx, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   int HW, int C, int G, int gpb, float eps, int swish, const uint8_t* __restrict__ mask,
                                                   float drop_scale, __bf16* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
                                                   Gn3Src src) {
  __shared__ double shd[GN3_T * 4 * 2];         // [rpp][Cs][2], rpp * Cs <= 4 * GN3_T
  __shared__ float st[2][64];
  Gn3Map m; m.init(C, G, gpb);
  const int cg = C / G;
  const float* xb = x + (size_t)m.b * HW * ldx + m.c0 + 4 * m.q;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
  if (SRC && m.on) {                              // x is still S slabs: finish it here (ldx == C), this thread's quads, for its own second pass
    float* xw = const_cast<float*>(xb);
#pragma unroll 2
    for (int p = m.r; p < HW; p += m.rpp) {
      const float4 v = gn3_src_quad(src, (int64_t)m.b * HW + p, m.b, m.c0 + 4 * m.q, C);
      *reinterpret_cast<float4*>(xw + (size_t)p * ldx) = v;
      s[0] += v.x; ss[0] += (double)v.x * v.x; s[1] += v.y; ss[1] += (double)v.y * v.y;
      s[2] += v.z; ss[2] += (double)v.z * v.z; s[3] += v.w; ss[3] += (double)v.w * v.w;
    }
  } else if (!SRC && m.on) {
#pragma unroll 8
    for (int p = m.r; p < HW; p += m.rpp) {
      const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx);
      s[0] += v.x; ss[0] += (double)v.x * v.x; s[1] += v.y; ss[1] += (double)v.y * v.y;
      s[2] += v.z; ss[2] += (double)v.z * v.z; s[3] += v.w; ss[3] += (double)v.w * v.w;
    }
  }
  if (m.on) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      shd[((size_t)m.r * m.Cs + 4 * m.q + e) * 2] = s[e]; shd[((size_t)m.r * m.Cs + 4 * m.q + e) * 2 + 1] = ss[e];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, per = m.rpp * cg;
  for (int g = threadIdx.x >> 6; g < gpb; g += GN3_T / 64) {      // one wave per group at a time, as k_gn2_stats
    double a = 0.0, q = 0.0;
    for (int i = lane; i < per; i += 64) {
      const int r = i / cg, c = g * cg + (i - r * cg);
      a += shd[((size_t)r * m.Cs + c) * 2]; q += shd[((size_t)r * m.Cs + c) * 2 + 1];
    }
    a = wave_sum_d(a); q = wave_sum_d(q);
    if (lane == 0) {
      const double n = (double)HW * cg, mu = a / n;
      double var = q / n - mu * mu;                 // biased variance, as torch.nn.GroupNorm
      var = var < 0 ? 0 : var;
      st[0][g] = (float)mu; st[1][g] = (float)(1.0 / sqrt(var + (double)eps));
      mean[m.b * G + m.g0 + g] = st[0][g]; rstd[m.b * G + m.g0 + g] = st[1][g];
    }
  }
  __syncthreads();
  if (!m.on) return;
  float mu[4], rs[4], ga[4], be[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * m.q + e, gi = c / cg;
    mu[e] = st[0][gi]; rs[e] = st[1][gi]; ga[e] = gamma[m.c0 + c]; be[e] = beta[m.c0 + c];
  }
  __bf16* yb = y + (size_t)m.b * HW * C + m.c0 + 4 * m.q;
  const uint8_t* mb = mask ? mask + (size_t)m.b * HW * C + m.c0 + 4 * m.q : nullptr;
#pragma unroll 8
  for (int p = m.r; p < HW; p += m.rpp) {
    const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx);
    float z[4] = {v.x, v.y, v.z, v.w};
    uchar4 mk = make_uchar4(1, 1, 1, 1);
    if (mb) mk = *reinterpret_cast<const uchar4*>(mb + (size_t)p * C);
    const uint8_t mke[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float t = (z[e] - mu[e]) * rs[e] * ga[e] + be[e];
      if (swish) t = silu(t);
      if (mb) t = mke[e] ? t * drop_scale : 0.f;
      z[e] = t;
    }
    *reinterpret_cast<bf16x4*>(yb + (size_t)p * C) = bf16x4{f2bf(z[0]), f2bf(z[1]), f2bf(z[2]), f2bf(z[3])};
  }
}
// backward of the same decomposition: pass 1 = per-channel sums of dz xhat and dz over the sample (the parameter-gradient partials pg / pb of
// this sample, complete here) -> the group means k1, k2; pass 2 = dx (+)= rstd (dz gamma - k1 - xhat k2), every output form of k_gn2_bwd_apply
// (fp32 with accumulate / extra, bf16 operand copy, per-sample column sums: colpart keeps the caller's [B][nchunk][C] layout -- chunk 0 gets the
// sample's sum, the other chunks zeros)
template <bool SRC>
__global__ __launch_bounds__(GN3_T) void k_gn3_bwd(const float* __restrict__ dy, const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                   int HW, int C, int G, int gpb, int swish, const uint8_t* __restrict__ mask, float drop_scale,
                                                   float* __restrict__ dx, int lddx, int accumulate, float* __restrict__ pg, float* __restrict__ pb,
                                                   const float* __restrict__ extra, int ldextra, __bf16* __restrict__ dx16,
                                                   float* __restrict__ colpart, int nchunk, Gn3Src src) {
  __shared__ float shf[GN3_T * 4 * 2];          // [rpp][Cs][2]; afterwards [rpp][Cs] column sums
  __shared__ float chs[GN3_T * 4 * 2 / (GN3_T / 256)];          // [Cs][2] channel sums, Cs <= 1024
  __shared__ float kk[2 * 64];
  Gn3Map m; m.init(C, G, gpb);
  const int cg = C / G;
  float mu[4], rs[4], ga[4], be[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * m.q + e, gi = m.g0 + c / cg;
    mu[e] = 0.f; rs[e] = 0.f; ga[e] = 0.f; be[e] = 0.f;
    if (m.on) { mu[e] = mean[m.b * G + gi]; rs[e] = rstd[m.b * G + gi]; ga[e] = gamma[m.c0 + c]; be[e] = beta[m.c0 + c]; }
  }
  const float* xb = x + (size_t)m.b * HW * ldx + m.c0 + 4 * m.q;
  const float* dyb = dy + (size_t)m.b * HW * C + m.c0 + 4 * m.q;
  const uint8_t* mb = mask ? mask + (size_t)m.b * HW * C + m.c0 + 4 * m.q : nullptr;
  if (m.on) {
    float ca[4] = {0.f, 0.f, 0.f, 0.f}, cb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll SRC ? 2 : 8
    for (int p = m.r; p < HW; p += m.rpp) {
      const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx);
      float4 dv;
      if constexpr (SRC) {                          // dy is still S slabs (an input-gradient convolution): finished here, stored for pass 2
        dv = gn3_src_quad(src, (int64_t)m.b * HW + p, m.b, m.c0 + 4 * m.q, C);
        *reinterpret_cast<float4*>(const_cast<float*>(dyb) + (size_t)p * C) = dv;
      } else
        dv = *reinterpret_cast<const float4*>(dyb + (size_t)p * C);
      uchar4 mk = make_uchar4(1, 1, 1, 1);
      if (mb) mk = *reinterpret_cast<const uchar4*>(mb + (size_t)p * C);
      const float xv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {dv.x, dv.y, dv.z, dv.w};
      const uint8_t mke[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xv[e] - mu[e]) * rs[e];
        float d = dd[e];
        if (mb) d = mke[e] ? d * drop_scale : 0.f;
        if (swish) d *= silu_grad(xh * ga[e] + be[e]);
        ca[e] += d * xh; cb[e] += d;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      shf[((size_t)m.r * m.Cs + 4 * m.q + e) * 2] = ca[e]; shf[((size_t)m.r * m.Cs + 4 * m.q + e) * 2 + 1] = cb[e];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < m.Cs; c += GN3_T) {
    float a = 0.f, q = 0.f;
    for (int r = 0; r < m.rpp; ++r) { a += shf[((size_t)r * m.Cs + c) * 2]; q += shf[((size_t)r * m.Cs + c) * 2 + 1]; }
    chs[2 * c] = a; chs[2 * c + 1] = q;
    pg[(size_t)m.b * C + m.c0 + c] = a; pb[(size_t)m.b * C + m.c0 + c] = q;
  }
  __syncthreads();
  if (threadIdx.x < gpb) {
    float t1 = 0.f, t2 = 0.f;
    for (int c = threadIdx.x * cg; c < (threadIdx.x + 1) * cg; ++c) { const float g1 = gamma[m.c0 + c]; t1 += g1 * chs[2 * c + 1]; t2 += g1 * chs[2 * c]; }
    const float inv = 1.0f / ((float)HW * (float)cg);
    kk[2 * threadIdx.x] = t1 * inv; kk[2 * threadIdx.x + 1] = t2 * inv;
  }
  __syncthreads();
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  if (m.on) {
    float k1[4], k2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int gi = (4 * m.q + e) / cg; k1[e] = kk[2 * gi]; k2[e] = kk[2 * gi + 1]; }
    float* dxb = dx ? dx + (size_t)m.b * HW * lddx + m.c0 + 4 * m.q : nullptr;
    __bf16* d16b = dx16 ? dx16 + (size_t)m.b * HW * C + m.c0 + 4 * m.q : nullptr;
    const float* exb = extra ? extra + (size_t)m.b * HW * ldextra + m.c0 + 4 * m.q : nullptr;
#pragma unroll 4
    for (int p = m.r; p < HW; p += m.rpp) {
      const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * ldx);
      const float4 dv = *reinterpret_cast<const float4*>(dyb + (size_t)p * C);
      uchar4 mk = make_uchar4(1, 1, 1, 1);
      if (mb) mk = *reinterpret_cast<const uchar4*>(mb + (size_t)p * C);
      const float xv[4] = {v.x, v.y, v.z, v.w}, dd[4] = {dv.x, dv.y, dv.z, dv.w};
      const uint8_t mke[4] = {mk.x, mk.y, mk.z, mk.w};
      float4* op = dxb ? reinterpret_cast<float4*>(dxb + (size_t)p * lddx) : nullptr;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (accumulate) { const float4 c = *op; o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w; }
      if (exb) {
        const float4 c = *reinterpret_cast<const float4*>(exb + (size_t)p * ldextra);
        o[0] += c.x; o[1] += c.y; o[2] += c.z; o[3] += c.w;
      }
      const bool acc = accumulate || exb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xv[e] - mu[e]) * rs[e];
        float d = dd[e];
        if (mb) d = mke[e] ? d * drop_scale : 0.f;
        if (swish) d *= silu_grad(xh * ga[e] + be[e]);
        const float vv = rs[e] * (d * ga[e] - k1[e] - xh * k2[e]);
        o[e] = acc ? o[e] + vv : vv;
      }
      if (op) *op = make_float4(o[0], o[1], o[2], o[3]);
      if (d16b) *reinterpret_cast<bf16x4*>(d16b + (size_t)p * C) = bf16x4{f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
      if (colpart) {
#pragma unroll
        for (int e = 0; e < 4; ++e) cs[e] += o[e];
      }
    }
  }
  if (colpart) {
    __syncthreads();                            // every reader of shf's channel partials is done
    if (m.on) {
#pragma unroll
      for (int e = 0; e < 4; ++e) shf[(size_t)m.r * m.Cs + 4 * m.q + e] = cs[e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < m.Cs; c += GN3_T) {
      float a = 0.f;
      for (int r = 0; r < m.rpp; ++r) a += shf[(size_t)r * m.Cs + c];
      colpart[((size_t)m.b * nchunk) * C + m.c0 + c] = a;
      for (int k = 1; k < nchunk; ++k) colpart[((size_t)m.b * nchunk + k) * C + m.c0 + c] = 0.f;
    }
  }
}


}  // namespace

extern "C" {

// debug build only (tools/ A-B runs): SFRON_GN_ONE_LAUNCH=0 in the environment keeps every GroupNorm on the two-phase pair
static bool gn3_off() {
#ifdef SFRON_DEBUG_KNOBS
  static const bool v = [] { const char* e = getenv("SFRON_GN_ONE_LAUNCH"); return e && e[0] == '0'; }();
  return v;
#else
  return false;
#endif
}
/* scratch (bytes) the row-coalesced GroupNorm needs for a [B][HW][C] activation: per-chunk partial sums (forward fp64 per group,
 * backward fp32 per channel) */
int64_t sfron_groupnorm_scratch_bytes(int B, int HW, int C, int groups) {
  if (B <= 0 || HW <= 0 || C <= 0 || groups <= 0) return 0;
  const int64_t n = gn_chunks(B, HW);
  const int64_t f = (int64_t)B * n * groups * 2 * sizeof(double), bw = (int64_t)B * n * C * 2 * sizeof(float);
  return f > bw ? f : bw;
}
// 2 GiB rule for the GroupNorm family: the kernels step through x / y / dy / dx with size_t offsets, but the chunk and workgroup
// bookkeeping (B * chunks, rows per chunk) is `int` and nothing runs them above the line -- a [B][HW][ld] fp32 activation of 2^31 bytes
// or more is refused (its bf16 result is half that)
static bool gn_fits31(int B, int HW, int ld) { return sfron_fits31((int64_t)B * HW * ld * 4); }
static bool gn2_ok(int ldx, int ld2, int C, int groups, const void* scratch) {
  return scratch && C % 4 == 0 && ldx % 4 == 0 && ld2 % 4 == 0 && C <= GN_MAXQ * 4 * GNB && groups <= 64 && ((uintptr_t)scratch & 15) == 0;
}
// groups per workgroup of the one-launch form (k_gn3_*), 0 = the two-phase pair: whole groups whose channels form float4 quads and runs that are
// multiples of half a cache line (a 96-byte run straddles lines: measured 1.7x slower than the pair), at least 192 workgroups, and a slab of at
// most 128 KB per workgroup (its second pass is an L2 hit) -- or, with eight groups in whole-line runs, up to 512 KB (second pass from the
// Infinity Cache, as the pair's)
static int gn3_gpb(int B, int HW, int C, int groups) {
  if (gn3_off()) return 0;
  const int cg = C / groups;
  for (const int gpb : {8, 4, 2, 1}) {
    if (groups % gpb) continue;
    const int Cs = gpb * cg;
    if (Cs % 16 || Cs > 1024) continue;
    if ((int64_t)HW * Cs * 4 > (128 << 10)) continue;
    if ((int64_t)B * (groups / gpb) < 192) continue;
    return gpb;
  }
  if (groups % 8 == 0) {
    const int Cs = 8 * cg;
    if (Cs % 32 == 0 && Cs <= 1024 && (int64_t)HW * Cs * 4 <= (512 << 10) && (int64_t)B * (groups / 8) >= 192) return 8;
  }
  return 0;
}
static size_t gn2_lds(int C, int elem) {
  const int qpr = C / 4, qw = qpr < GNB ? qpr : GNB, rpp = GNB / qw;
  return (size_t)rpp * C * 2 * elem;
}
int sfron_groupnorm_fwd(const float* x, int ldx, const float* gamma, const float* beta, int B, int HW, int C, int groups, float eps,
                        int swish, const uint8_t* drop_mask, float drop_scale, uint16_t* y, float* mean, float* rstd, void* scratch,
                        void* stream) {
  SFRON_CHECK_ARG(x && gamma && beta && y && mean && rstd && groups > 0 && C % groups == 0 && ldx >= C && C / groups <= TPB);
  SFRON_CHECK_ARG(B > 0 && HW > 0 && gn_fits31(B, HW, ldx));
  if (gn2_ok(ldx, C, C, groups, scratch) && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 7) == 0 && (!drop_mask || ((uintptr_t)drop_mask & 3) == 0)) {
    if (const int gpb = gn3_gpb(B, HW, C, groups)) {
      hipLaunchKernelGGL(k_gn3_fwd<false>, dim3(B * (groups / gpb)), dim3(GN3_T), 0, (hipStream_t)stream, x, ldx, gamma, beta, HW, C, groups, gpb, eps, swish,
                         drop_mask, drop_scale, (__bf16*)y, mean, rstd, Gn3Src{});
      SFRON_LAUNCH_STATUS();
      return SFRON_OK;
    }
    const int nchunk = gn_chunks(B, HW);
    hipLaunchKernelGGL(k_gn2_stats, dim3(B * nchunk), dim3(GNB), gn2_lds(C, sizeof(double)), (hipStream_t)stream, x, ldx, HW, C, groups, nchunk,
                       (double*)scratch);
    SFRON_LAUNCH_STATUS();
    hipLaunchKernelGGL(k_gn2_apply, dim3(B * nchunk), dim3(GNB), 0, (hipStream_t)stream, x, ldx, gamma, beta, HW, C, groups, eps, swish, drop_mask,
                       drop_scale, nchunk, (const double*)scratch, (__bf16*)y, mean, rstd);
    SFRON_LAUNCH_STATUS();
    return SFRON_OK;
  }
  hipLaunchKernelGGL(k_gn_fwd, dim3(B * groups), dim3(TPB), 0, (hipStream_t)stream, x, ldx, gamma, beta, HW, C, groups, eps, swish, drop_mask,
                     drop_scale, (__bf16*)y, mean, rstd);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_groupnorm_bwd(const float* dy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                        const float* rstd, int B, int HW, int C, int groups, int swish, const uint8_t* drop_mask, float drop_scale,
                        float* dx, int lddx, int accumulate, float* part_gamma, float* part_beta, void* scratch, void* stream) {
  return sfron_groupnorm_bwd_res(dy, x, ldx, gamma, beta, mean, rstd, B, HW, C, groups, swish, drop_mask, drop_scale, dx, lddx, accumulate, nullptr, 0,
                                 part_gamma, part_beta, scratch, stream);
}
int sfron_groupnorm_bwd_res(const float* dy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                            const float* rstd, int B, int HW, int C, int groups, int swish, const uint8_t* drop_mask, float drop_scale,
                            float* dx, int lddx, int accumulate, const float* extra, int ld_extra, float* part_gamma, float* part_beta,
                            void* scratch, void* stream) {
  SFRON_CHECK_ARG(dy && x && gamma && beta && mean && rstd && dx && part_gamma && part_beta && groups > 0 && C % groups == 0);
  SFRON_CHECK_ARG(ldx >= C && lddx >= C);
  SFRON_CHECK_ARG(B > 0 && HW > 0 && gn_fits31(B, HW, ldx) && gn_fits31(B, HW, lddx) && gn_fits31(B, HW, C));
  const int cg = C / groups;
  SFRON_CHECK_ARG(cg <= TPB);
  SFRON_CHECK_ARG(!extra || (ld_extra >= C && extra != dx));
  const bool fused = gn2_ok(ldx, lddx, C, groups, scratch) && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0 &&
                     (!drop_mask || ((uintptr_t)drop_mask & 3) == 0);
  if (extra && !(fused && ld_extra % 4 == 0 && ((uintptr_t)extra & 15) == 0)) {       // the same sum as two passes
    const int rc = sfron_copy_cols(extra, ld_extra, (int64_t)B * HW, C, dx, lddx, accumulate, stream);
    if (rc) return rc;
    extra = nullptr; accumulate = 1;
  }
  if (fused) {
    if (const int gpb = gn3_gpb(B, HW, C, groups)) {
      hipLaunchKernelGGL(k_gn3_bwd<false>, dim3(B * (groups / gpb)), dim3(GN3_T), 0, (hipStream_t)stream, dy, x, ldx, gamma, beta, mean, rstd, HW, C, groups, gpb,
                         swish, drop_mask, drop_scale, dx, lddx, accumulate, part_gamma, part_beta, extra, ld_extra, (__bf16*)nullptr, (float*)nullptr, 1,
                         Gn3Src{});
      SFRON_LAUNCH_STATUS();
      return SFRON_OK;
    }
    const int nchunk = gn_chunks(B, HW);
    hipLaunchKernelGGL(k_gn2_bwd_stats, dim3(B * nchunk), dim3(GNB), gn2_lds(C, sizeof(float)), (hipStream_t)stream, dy, x, ldx, gamma, beta, mean, rstd,
                       HW, C, groups, swish, drop_mask, drop_scale, nchunk, (float*)scratch);
    SFRON_LAUNCH_STATUS();
    hipLaunchKernelGGL(k_gn2_bwd_apply, dim3(B * nchunk), dim3(GNB), (size_t)(3 * C + 2 * groups) * sizeof(float), (hipStream_t)stream, dy, x, ldx, gamma,
                       beta, mean, rstd, HW, C, groups, swish, drop_mask, drop_scale, nchunk, (const float*)scratch, dx, lddx, accumulate,
                       part_gamma, part_beta, extra, ld_extra, (__bf16*)nullptr, (float*)nullptr);
    SFRON_LAUNCH_STATUS();
    return SFRON_OK;
  }
  const size_t lds = (2 * (TPB / 64) + 2 * cg + 2 * TPB) * sizeof(float);
  hipLaunchKernelGGL(k_gn_bwd, dim3(B * groups), dim3(TPB), lds, (hipStream_t)stream, dy, x, ldx, gamma, beta, mean, rstd, HW, C, groups, swish,
                     drop_mask, drop_scale, dx, lddx, accumulate, part_gamma, part_beta);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_groupnorm_chunks(int B, int HW) { return (B > 0 && HW > 0) ? gn_chunks(B, HW) : 0; }
int sfron_groupnorm_bwd_cast_ok(int ldx, int C, int groups) {
  return C > 0 && groups > 0 && C % groups == 0 && C % 4 == 0 && ldx % 4 == 0 && C <= 2048 && C <= GN_MAXQ * 4 * GNB && groups <= 64;
}
int sfron_groupnorm_bwd_cast(const float* dy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                             const float* rstd, int B, int HW, int C, int groups, int swish, const uint8_t* drop_mask, float drop_scale,
                             uint16_t* dx_bf16, float* col_partials, float* part_gamma, float* part_beta, void* scratch, void* stream) {
  SFRON_CHECK_ARG(dy && x && gamma && beta && mean && rstd && dx_bf16 && col_partials && part_gamma && part_beta && scratch);
  SFRON_CHECK_ARG(sfron_groupnorm_bwd_cast_ok(ldx, C, groups) && ldx >= C && B > 0 && HW > 0 && gn_fits31(B, HW, ldx));
  SFRON_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)scratch) & 15) == 0 && ((uintptr_t)dx_bf16 & 7) == 0 &&
                  (!drop_mask || ((uintptr_t)drop_mask & 3) == 0));
  const int nchunk = gn_chunks(B, HW);
  if (const int gpb = gn3_gpb(B, HW, C, groups)) {
    hipLaunchKernelGGL(k_gn3_bwd<false>, dim3(B * (groups / gpb)), dim3(GN3_T), 0, (hipStream_t)stream, dy, x, ldx, gamma, beta, mean, rstd, HW, C, groups, gpb,
                       swish, drop_mask, drop_scale, (float*)nullptr, C, 0, part_gamma, part_beta, (const float*)nullptr, 0, (__bf16*)dx_bf16,
                       col_partials, nchunk, Gn3Src{});
    SFRON_LAUNCH_STATUS();
    return SFRON_OK;
  }
  hipLaunchKernelGGL(k_gn2_bwd_stats, dim3(B * nchunk), dim3(GNB), gn2_lds(C, sizeof(float)), (hipStream_t)stream, dy, x, ldx, gamma, beta, mean, rstd,
                     HW, C, groups, swish, drop_mask, drop_scale, nchunk, (float*)scratch);
  SFRON_LAUNCH_STATUS();
  const size_t lds = (size_t)(3 * C + 2 * groups + 4 * GNB) * sizeof(float);          // + [rows per pass][C] for the column sums
  hipLaunchKernelGGL(k_gn2_bwd_apply, dim3(B * nchunk), dim3(GNB), lds, (hipStream_t)stream, dy, x, ldx, gamma, beta, mean, rstd, HW, C, groups, swish,
                     drop_mask, drop_scale, nchunk, (const float*)scratch, (float*)nullptr, C, 0, part_gamma, part_beta, (const float*)nullptr, 0,
                     (__bf16*)dx_bf16, col_partials);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

// ---- the GroupNorm input as an unfinished split-K result (sfron_split_src)
static Gn3Src gn3_src(const sfron_split_src* s) {
  return Gn3Src{s->slabs, s->n_slabs, s->slab_stride, s->bias, s->sample_vec, s->ld_vec, s->resid, s->ld_resid};
}
int sfron_groupnorm_one_launch(int B, int HW, int C, int groups) {
  return B > 0 && HW > 0 && C > 0 && groups > 0 && C % groups == 0 && C % 4 == 0 && groups <= 64 && gn3_gpb(B, HW, C, groups) > 0;
}
int sfron_groupnorm_fwd_src(const sfron_split_src* src, float* x, const float* gamma, const float* beta, int B, int HW, int C, int groups, float eps,
                            int swish, const uint8_t* drop_mask, float drop_scale, uint16_t* y, float* mean, float* rstd, void* stream) {
  SFRON_CHECK_ARG(x && gamma && beta && y && mean && rstd && groups > 0 && C % groups == 0 && split_src_ok(src, C));
  SFRON_CHECK_ARG(B > 0 && HW > 0 && gn_fits31(B, HW, C));
  SFRON_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 7) == 0 && (!drop_mask || ((uintptr_t)drop_mask & 3) == 0) && groups <= 64);
  SFRON_CHECK_ARG(!src->resid || (const float*)x != src->resid);
  const int gpb = gn3_gpb(B, HW, C, groups);
  if (!gpb) return SFRON_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_gn3_fwd<true>, dim3(B * (groups / gpb)), dim3(GN3_T), 0, (hipStream_t)stream, (const float*)x, C, gamma, beta, HW, C, groups, gpb,
                     eps, swish, drop_mask, drop_scale, (__bf16*)y, mean, rstd, gn3_src(src));
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_groupnorm_bwd_res_src(const sfron_split_src* src, float* dy, const float* x, int ldx, const float* gamma, const float* beta,
                                const float* mean, const float* rstd, int B, int HW, int C, int groups, int swish, const uint8_t* drop_mask,
                                float drop_scale, float* dx, int lddx, int accumulate, const float* extra, int ld_extra, float* part_gamma,
                                float* part_beta, void* stream) {
  SFRON_CHECK_ARG(dy && x && gamma && beta && mean && rstd && dx && part_gamma && part_beta && groups > 0 && C % groups == 0 && split_src_ok(src, C));
  SFRON_CHECK_ARG(ldx >= C && lddx >= C);
  SFRON_CHECK_ARG(B > 0 && HW > 0 && gn_fits31(B, HW, ldx) && gn_fits31(B, HW, lddx) && gn_fits31(B, HW, C));
  SFRON_CHECK_ARG(ldx % 4 == 0 && lddx % 4 == 0 && groups <= 64 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0 &&
                  (!drop_mask || ((uintptr_t)drop_mask & 3) == 0) && dy != dx);
  SFRON_CHECK_ARG(!extra || (ld_extra >= C && extra != dx && ld_extra % 4 == 0 && ((uintptr_t)extra & 15) == 0));
  const int gpb = gn3_gpb(B, HW, C, groups);
  if (!gpb) return SFRON_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_gn3_bwd<true>, dim3(B * (groups / gpb)), dim3(GN3_T), 0, (hipStream_t)stream, (const float*)dy, x, ldx, gamma, beta, mean, rstd, HW,
                     C, groups, gpb, swish, drop_mask, drop_scale, dx, lddx, accumulate, part_gamma, part_beta, extra, ld_extra, (__bf16*)nullptr,
                     (float*)nullptr, 1, gn3_src(src));
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_groupnorm_bwd_cast_src(const sfron_split_src* src, float* dy, const float* x, int ldx, const float* gamma, const float* beta,
                                 const float* mean, const float* rstd, int B, int HW, int C, int groups, int swish, const uint8_t* drop_mask,
                                 float drop_scale, uint16_t* dx_bf16, float* col_partials, float* part_gamma, float* part_beta, void* stream) {
  SFRON_CHECK_ARG(dy && x && gamma && beta && mean && rstd && dx_bf16 && col_partials && part_gamma && part_beta && split_src_ok(src, C));
  SFRON_CHECK_ARG(sfron_groupnorm_bwd_cast_ok(ldx, C, groups) && ldx >= C && B > 0 && HW > 0 && gn_fits31(B, HW, ldx));
  SFRON_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy) & 15) == 0 && ((uintptr_t)dx_bf16 & 7) == 0 && (!drop_mask || ((uintptr_t)drop_mask & 3) == 0));
  const int gpb = gn3_gpb(B, HW, C, groups);
  if (!gpb) return SFRON_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_gn3_bwd<true>, dim3(B * (groups / gpb)), dim3(GN3_T), 0, (hipStream_t)stream, (const float*)dy, x, ldx, gamma, beta, mean, rstd, HW,
                     C, groups, gpb, swish, drop_mask, drop_scale, (float*)nullptr, C, 0, part_gamma, part_beta, (const float*)nullptr, 0,
                     (__bf16*)dx_bf16, col_partials, gn_chunks(B, HW), gn3_src(src));
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
