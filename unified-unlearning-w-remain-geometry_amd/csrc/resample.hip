// Pillow's antialiased resize of an 8-bit RGB image with the centre crop folded in (the Resize + CenterCrop of
// SD/train-scripts/dataset.py:23-33 on a PIL image: Image.resize, Pillow's separable fixed-point convolution, PRECISION_BITS = 22).
// The filter is evaluated on the host (sfron.resample.resample_tables, float64 -> int32 coefficients); the device only does the integer
// arithmetic, so the result is specified bit for bit:  ss = 2^21 + sum_x src[xmin + x] * k[x] in int32, out = clamp(ss >> 22, 0, 255).
// Horizontal pass first, to uint8 (that rounding is part of the result), then the vertical pass over it.
//
// Both kernels clamp every bound they read from the tables into the extents they were given (source width / height, taps per output,
// rows of tmp): a table that does not belong to the image gives wrong pixels, never an access outside src / tmp / dst.
#include "common.h"
#include "../../include/sfron.h"

namespace {

constexpr int RS_TPB = 256;
constexpr int RS_SPAN = 32768;          // bytes of one source row a workgroup stages in LDS (10922 pixels); a longer span is read from global
constexpr int RS_SHIFT = 22;            // Pillow's PRECISION_BITS for 8-bit images

__device__ __forceinline__ int rs_clamp(int64_t v, int64_t lo, int64_t hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }
__device__ __forceinline__ uint8_t rs_clip8(int ss) {
  const int v = ss >> RS_SHIFT;          // arithmetic shift, as Pillow's clip8
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// rows [y0, y0 + nrows) of the source that the window's output rows read: the union of by (its entries ascend), cut to Hs and to tmp
__device__ __forceinline__ void rs_rows(const int32_t* __restrict__ by, int Ho, int Hs, int tmp_rows, int& y0, int& nrows) {
  y0 = rs_clamp(by[0], 0, Hs - 1);
  const int y1 = rs_clamp((int64_t)by[2 * (Ho - 1)] + by[2 * (Ho - 1) + 1], y0, Hs);
  nrows = min(y1 - y0, tmp_rows);
}

// ---- horizontal pass: workgroup = one source row x RS_TPB output columns; the span of source pixels those columns read is staged in
// LDS (neighbouring outputs read overlapping windows), a thread forms the three channels of one output pixel.  Source rows are
// 3 * Ws bytes, so their starts are not dword-aligned for odd Ws: head bytes up to the first aligned address, dwords, tail bytes.
__global__ __launch_bounds__(RS_TPB) void k_resample_h(const uint8_t* __restrict__ src, int Hs, int Ws, const int32_t* __restrict__ kx,
                                                       const int32_t* __restrict__ bx, int ksx, const int32_t* __restrict__ by, int Ho,
                                                       int Wo, uint8_t* __restrict__ tmp, int tmp_rows) {
  __shared__ uint32_t span32[RS_SPAN / 4 + 2];
  uint8_t* span = reinterpret_cast<uint8_t*>(span32);
  int y0, nrows;
  rs_rows(by, Ho, Hs, tmp_rows, y0, nrows);
  const int r = blockIdx.x;
  if (r >= nrows) return;                                              // uniform over the workgroup
  const int x0 = blockIdx.y * RS_TPB, xe = min(x0 + RS_TPB, Wo) - 1;
  const int lo = rs_clamp(bx[2 * x0], 0, Ws);
  const int hi = rs_clamp((int64_t)bx[2 * xe] + bx[2 * xe + 1], lo, Ws);
  const int nbytes = (hi - lo) * 3;
  const bool staged = nbytes <= RS_SPAN;
  const uint8_t* row = src + ((int64_t)(y0 + r) * Ws) * 3;
  const uint8_t* p = row + (int64_t)lo * 3;
  const int a = (int)((uintptr_t)p & 3);                                // byte i of the span lives at span[a + i]: dwords align on both sides
  if (staged) {
    const int head = min((4 - a) & 3, nbytes);
    const int ndw = (nbytes - head) >> 2;
    const int tail0 = head + 4 * ndw;
    if ((int)threadIdx.x < head) span[a + threadIdx.x] = p[threadIdx.x];
    const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p + head);
    uint32_t* s32 = span32 + ((a + head) >> 2);
    for (int i = threadIdx.x; i < ndw; i += RS_TPB) s32[i] = p32[i];
    if ((int)threadIdx.x < nbytes - tail0) span[a + tail0 + threadIdx.x] = p[tail0 + threadIdx.x];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= Wo) return;
  const int xmin = rs_clamp(bx[2 * x], 0, Ws);
  const int n = rs_clamp(bx[2 * x + 1], 0, min(ksx, Ws - xmin));
  const int32_t* k = kx + (int64_t)x * ksx;
  int s0 = 1 << (RS_SHIFT - 1), s1 = s0, s2 = s0;
  if (staged && xmin >= lo && xmin + n <= hi) {
    const uint8_t* q = span + a + (xmin - lo) * 3;
    for (int i = 0; i < n; ++i) {
      const int c = k[i];
      s0 += q[3 * i] * c, s1 += q[3 * i + 1] * c, s2 += q[3 * i + 2] * c;
    }
  } else {
    const uint8_t* q = row + (int64_t)xmin * 3;
    for (int i = 0; i < n; ++i) {
      const int c = k[i];
      s0 += q[3 * i] * c, s1 += q[3 * i + 1] * c, s2 += q[3 * i + 2] * c;
    }
  }
  uint8_t* o = tmp + ((int64_t)r * Wo + x) * 3;
  o[0] = rs_clip8(s0), o[1] = rs_clip8(s1), o[2] = rs_clip8(s2);
}

// ---- vertical pass: workgroup = one output row x RS_TPB bytes of it; a thread forms one byte (a channel of a pixel).  Loads run along
// the row (coalesced), the row's coefficients and bounds are the same for every thread (scalar loads).
__global__ __launch_bounds__(RS_TPB) void k_resample_v(const uint8_t* __restrict__ tmp, int tmp_rows, int Hs, const int32_t* __restrict__ ky,
                                                       const int32_t* __restrict__ by, int ksy, int Ho, int Wo, uint8_t* __restrict__ dst) {
  const int yy = blockIdx.x;
  const int64_t w3 = (int64_t)Wo * 3;
  const int64_t j = (int64_t)blockIdx.y * RS_TPB + threadIdx.x;
  if (j >= w3) return;
  int y0, nrows;
  rs_rows(by, Ho, Hs, tmp_rows, y0, nrows);
  const int ymin = rs_clamp((int64_t)by[2 * yy] - y0, 0, nrows);
  const int n = rs_clamp(by[2 * yy + 1], 0, min(ksy, nrows - ymin));
  const int32_t* k = ky + (int64_t)yy * ksy;
  const uint8_t* q = tmp + (int64_t)ymin * w3 + j;
  int ss = 1 << (RS_SHIFT - 1);
  for (int i = 0; i < n; ++i) ss += q[(int64_t)i * w3] * k[i];
  dst[(int64_t)yy * w3 + j] = rs_clip8(ss);
}

}  // namespace

extern "C" {

int sfron_image_resample_u8(const uint8_t* src, int Hs, int Ws, const int32_t* kx, const int32_t* bx, int ksx, const int32_t* ky,
                            const int32_t* by, int ksy, int Wo, int Ho, uint8_t* tmp, int64_t tmp_bytes, uint8_t* dst, void* stream) {
  SFRON_CHECK_ARG(src && kx && bx && ky && by && tmp && dst);
  SFRON_CHECK_ARG(Hs > 0 && Ws > 0 && Wo > 0 && Ho > 0 && ksx >= 1 && ksy >= 1);
  SFRON_CHECK_ARG((int64_t)Ws * 3 < (1ll << 31) && (int64_t)Wo * 3 < (1ll << 31));      // a row's byte count is an `int`; offsets are 64-bit
  const int64_t w3 = (int64_t)Wo * 3;
  SFRON_CHECK_ARG(tmp_bytes >= w3);                                    // at least one row; the row count itself is in the device tables
  const int tmp_rows = (int)(tmp_bytes / w3 < Hs ? tmp_bytes / w3 : Hs);
  const unsigned xt = (unsigned)cdiv(Wo, RS_TPB), bt = (unsigned)((w3 + RS_TPB - 1) / RS_TPB);
  SFRON_CHECK_ARG(xt <= 65535u && bt <= 65535u);
  hipLaunchKernelGGL(k_resample_h, dim3((unsigned)tmp_rows, xt), dim3(RS_TPB), 0, (hipStream_t)stream, src, Hs, Ws, kx, bx, ksx, by, Ho, Wo, tmp,
                     tmp_rows);
  SFRON_LAUNCH_STATUS();
  hipLaunchKernelGGL(k_resample_v, dim3((unsigned)Ho, bt), dim3(RS_TPB), 0, (hipStream_t)stream, (const uint8_t*)tmp, tmp_rows, Hs, ky, by, ksy, Ho,
                     Wo, dst);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
