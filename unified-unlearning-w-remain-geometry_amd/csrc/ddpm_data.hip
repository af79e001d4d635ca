// DDPM training batches from a dataset that lives on the device (sfron.ddpm_data.DDPMBatchLoader): one launch does what the reference
// does per batch on the host -- DataLoader's collate, the upload, RandomHorizontalFlip, ToTensor, data_transform
// (DDPM/dataset/__init__.py:241-255) and the antithetic timestep draw of the runner's loops.
//   sfron_ddpm_batch_u8   uint8 [N][C][H][W] + int64 idx [B] (+ flip flags, u, n, image_mean, t_half)  ->  x0 fp32, c int64, t int64
// Arithmetic: one separately rounded fp32 operation per torch op of the reference, in its order.  The library is built with
// -ffp-contract=off, so X / 256 * 255 + u / 256 and X + n * 0.01 stay two roundings each, and x / 255.0f is hipcc's correctly rounded
// fp32 division (its default; x * (1 / 255.0f) differs from it for 126 of the 256 byte values).  Every form but the logit therefore has
// the bits of the torch expression; the logit form differs by the error of logf / log1pf.
//
// Launch- and latency-bound (3.5 MB moved per CIFAR batch of 128): one workgroup per (image, chunk of 1024 elements of C*H*W), no LDS.
// W % 4 == 0 and aligned operands: a lane loads four pixels as one dword and stores 16 bytes; a flipped image mirrors the dword's place
// in its row and reverses its bytes.  Anything else: one pixel per access, the same arithmetic.  Every element offset is 64-bit.
// idx lives on the device and cannot be refused by the host: an index outside [0, N) reads nothing, the row is NaN and its label -1.
#include <math.h>

#include "../../include/sfron.h"
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK = 4 * TPB;        // elements of one image per workgroup

struct Form {
  int uniform, gaussian, mode;
};

// data_transform of one pixel: v is the byte as fp32 (ToTensor's division is the first operation)
__device__ __forceinline__ float transform(float v, float u, float n, float mean, bool has_mean, Form f) {
  float x = v / 255.0f;                                              // ToTensor
  if (f.uniform) x = x / 256.0f * 255.0f + u / 256.0f;               // X / 256.0 * 255.0 + rand_like(X) / 256.0
  if (f.gaussian) x = x + n * 0.01f;                                 // X + randn_like(X) * 0.01
  if (f.mode == SFRON_DDPM_DATA_RESCALED) {
    x = 2.0f * x - 1.0f;
  } else if (f.mode == SFRON_DDPM_DATA_LOGIT) {                      // logit_transform, lam = 1e-6
    const float lam = 1e-6f, scale = (float)(1.0 - 2.0 * 1e-6);
    x = lam + scale * x;
    x = logf(x) - log1pf(-x);
  }
  if (has_mean) x = x - mean;
  return x;
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void k_ddpm_batch_u8(const uint8_t* __restrict__ images, const int64_t* __restrict__ labels, int64_t N,
                                                       int chw, int W, int chunks, const int64_t* __restrict__ idx,
                                                       const uint8_t* __restrict__ flip, int B, Form f, const float* __restrict__ u,
                                                       const float* __restrict__ n, const float* __restrict__ mean,
                                                       const int64_t* __restrict__ t_half, int T, float* __restrict__ x0,
                                                       int64_t* __restrict__ c, int64_t* __restrict__ t) {
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int64_t src = idx[b];
  const bool ok = src >= 0 && src < N;
  if (chunk == 0 && threadIdx.x == 0) {
    c[b] = ok ? labels[src] : (int64_t)-1;
    if (t) {                                                         // cat(t_half, T - t_half - 1)[:B], t_half of B / 2 + 1 entries
      const int half = B / 2 + 1;
      t[b] = b < half ? t_half[b] : (int64_t)T - t_half[b - half] - 1;
    }
  }
  const bool fl = flip && flip[b] != 0;
  const size_t ob = (size_t)b * chw;
  const uint8_t* img = images + (size_t)(ok ? src : 0) * chw;
  const float nan = __builtin_nanf("");
  if constexpr (VEC) {
    const int e = chunk * CHUNK + threadIdx.x * 4;                   // four pixels of one row: W % 4 == 0
    if (e >= chw) return;
    float4 o = make_float4(nan, nan, nan, nan);
    if (ok) {
      const int col = e % W;
      const int s = fl ? e - col + (W - 4 - col) : e;
      uint32_t px = *reinterpret_cast<const uint32_t*>(img + s);
      if (fl) px = __builtin_bswap32(px);
      float4 uu = make_float4(0.f, 0.f, 0.f, 0.f), nn = uu, mm = uu;
      if (f.uniform) uu = *reinterpret_cast<const float4*>(u + ob + e);
      if (f.gaussian) nn = *reinterpret_cast<const float4*>(n + ob + e);
      if (mean) mm = *reinterpret_cast<const float4*>(mean + e);
      o.x = transform((float)(px & 0xffu), uu.x, nn.x, mm.x, mean != nullptr, f);
      o.y = transform((float)((px >> 8) & 0xffu), uu.y, nn.y, mm.y, mean != nullptr, f);
      o.z = transform((float)((px >> 16) & 0xffu), uu.z, nn.z, mm.z, mean != nullptr, f);
      o.w = transform((float)(px >> 24), uu.w, nn.w, mm.w, mean != nullptr, f);
    }
    *reinterpret_cast<float4*>(x0 + ob + e) = o;
  } else {
#pragma unroll
    for (int k = 0; k < CHUNK / TPB; ++k) {
      const int e = chunk * CHUNK + k * TPB + threadIdx.x;
      if (e >= chw) return;
      float o = nan;
      if (ok) {
        const int col = e % W;
        const int s = fl ? e - col + (W - 1 - col) : e;
        o = transform((float)img[s], f.uniform ? u[ob + e] : 0.f, f.gaussian ? n[ob + e] : 0.f, mean ? mean[e] : 0.f, mean != nullptr, f);
      }
      x0[ob + e] = o;
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int sfron_ddpm_batch_u8(const uint8_t* images, const int64_t* labels, int64_t N, int C, int H, int W, const int64_t* idx,
                        const uint8_t* flip, int B, int uniform_deq, const float* u, int gaussian_deq, const float* n, int mode,
                        const float* image_mean, const int64_t* t_half, int T, float* x0, int64_t* c, int64_t* t, void* stream) {
  SFRON_CHECK_ARG(images && labels && idx && x0 && c);
  SFRON_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && B > 0 && T > 0);
  SFRON_CHECK_ARG((int64_t)B * C * H * W < (1ll << 31));
  SFRON_CHECK_ARG((!uniform_deq || u) && (!gaussian_deq || n));
  SFRON_CHECK_ARG((t_half == nullptr) == (t == nullptr));
  SFRON_CHECK_ARG(mode == SFRON_DDPM_DATA_PLAIN || mode == SFRON_DDPM_DATA_RESCALED || mode == SFRON_DDPM_DATA_LOGIT);
  const int chw = C * H * W, chunks = cdiv(chw, CHUNK);              // B * chunks <= B * chw < 2^31
  const Form f{uniform_deq != 0, gaussian_deq != 0, mode};
  const bool vec = W % 4 == 0 && aligned(images, 4) && aligned(x0, 16) && (!uniform_deq || aligned(u, 16)) &&
                   (!gaussian_deq || aligned(n, 16)) && (!image_mean || aligned(image_mean, 16));
  const dim3 grid((unsigned)(B * chunks)), block(TPB);
  if (vec)
    hipLaunchKernelGGL(k_ddpm_batch_u8<true>, grid, block, 0, (hipStream_t)stream, images, labels, N, chw, W, chunks, idx, flip, B, f, u, n,
                       image_mean, t_half, T, x0, c, t);
  else
    hipLaunchKernelGGL(k_ddpm_batch_u8<false>, grid, block, 0, (hipStream_t)stream, images, labels, N, chw, W, chunks, idx, flip, B, f, u, n,
                       image_mean, t_half, T, x0, c, t);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
