// DDPM guided sampling (sfron.ddpm.DDPMSampler, sfron.ddpm_sample): the per-step update behind one guided forward pass, the device-side
// step counter that lets ONE captured graph replay for every step, and the per-image normalised bytes of the runner's PNG files.
//   sfron_ddpm_guided_step      classifier-free guidance + the generalized update of DDPM/functions/denoising.py:72-95, coefficients read
//                               from a device table through a device step index
//   sfron_ddpm_sampler_advance  t <- tseq[k + 1], k <- k + 1 (one workgroup, a launch of its own behind the step kernel)
//   sfron_images_normalize_u8   tvu.save_image(x[k], path, normalize=True) for every image of a batch: per-image min / max, then the byte
//                               arithmetic of sfron_rows_to_image_u8 in SFRON_IMAGE_SAVE_IMAGE mode
// Built with -ffp-contract=off like the rest of the library: no product is fused into a sum, so the step kernel gives the bits of
// sfron_axpby followed by sfron_ddim_step.
#include <math.h>

#include "../../include/sfron.h"
#include "common.h"

namespace {

constexpr int TPB = 256;

// e = (1 + s) e_c + (-s) e_n as k_axpby forms it (alpha * a + beta * b, two rounded products and one rounded sum), then k_ddim_step's
//   x0 = (x - e s1) / s2;  x_next = (s3 x0 + c1 nz) + c2 e        (IEEE division; nz = 0 without a noise tensor)
// with (s1, s2, s3, c1, c2) = row clamp(*step, 0, steps - 1) of coef.  Every workgroup reads the index; nobody writes it here (the advance
// kernel does, in a launch behind this one).  x_next may be x: an element is read before it is written, by the same thread.
__global__ __launch_bounds__(TPB) void k_ddpm_guided_step(const float* x, const float* __restrict__ ec, const float* __restrict__ en,
                                                          const float* __restrict__ noise, float alpha, float beta,
                                                          const float* __restrict__ coef, int steps, const int* __restrict__ step, long n,
                                                          float* x_next, float* __restrict__ x0_pred) {
  int k = *step;
  k = k < 0 ? 0 : (k >= steps ? steps - 1 : k);
  const float* r = coef + 5 * (long)k;
  const float s1 = r[0], s2 = r[1], s3 = r[2], c1 = r[3], c2 = r[4];
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
    float e = ec[i];
    if (en) e = alpha * e + beta * en[i];
    const float x0 = (x[i] - e * s1) / s2;
    const float nz = noise ? noise[i] : 0.0f;
    x_next[i] = (s3 * x0 + c1 * nz) + c2 * e;
    if (x0_pred) x0_pred[i] = x0;
  }
}

// One workgroup.  Every thread reads the index, the barrier separates those reads from thread 0's write.  The index stops at `steps`
// (one past the last row: the step kernel clamps it back); the timestep of a step past the end is the last one's.
__global__ __launch_bounds__(TPB) void k_ddpm_sampler_advance(const float* __restrict__ tseq, int steps, int* step, float* __restrict__ t,
                                                              int nt) {
  int k = *step;
  k = k < 0 ? 0 : (k >= steps ? steps - 1 : k);
  const int next = k + 1;
  const float v = tseq[next < steps ? next : steps - 1];
  __syncthreads();
  for (int i = threadIdx.x; i < nt; i += TPB) t[i] = v;
  if (threadIdx.x == 0) *step = next;
}

// One workgroup (4 waves of 64 lanes) per image.  x fp32 [B][3][HW] -> out uint8 [B][HW][3].  Pass 1: min / max of the image's 3 HW values
// (a strided loop per thread, a 64-lane xor butterfly per wave, the 4 wave results through LDS).  hi = max(hi, lo + 1e-5) is formed in
// double and rounded once, as sfron.images.make_grid_u8 hands it to sfron_rows_to_image_u8.  Pass 2: one thread per output byte.
// ONE divergence from that pair: where hi == lo is left after the rounding (a constant image with |lo| >= 128, where lo + 1e-5 rounds
// back to lo) or the image holds no finite value, sfron_rows_to_image_u8 refuses (hi > lo is an argument check there); a kernel that owns
// a whole batch cannot refuse one image, so that image's bytes are all 0 -- what torchvision's (x - lo) / max(hi - lo, 1e-5) gives for a
// constant image.
__global__ __launch_bounds__(TPB) void k_images_normalize_u8(const float* __restrict__ x, int HW, uint8_t* __restrict__ out) {
  __shared__ float sh_lo[TPB / WAVE], sh_hi[TPB / WAVE];
  const long n = 3l * HW;
  const float* xi = x + (long)blockIdx.x * n;
  uint8_t* oi = out + (long)blockIdx.x * n;
  float lo = INFINITY, hi = -INFINITY;
  for (long i = threadIdx.x; i < n; i += TPB) {
    const float v = xi[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, WAVE));
    hi = fmaxf(hi, __shfl_xor(hi, o, WAVE));
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    sh_lo[threadIdx.x / WAVE] = lo;
    sh_hi[threadIdx.x / WAVE] = hi;
  }
  __syncthreads();
  lo = sh_lo[0]; hi = sh_hi[0];
#pragma unroll
  for (int w = 1; w < TPB / WAVE; ++w) {
    lo = fminf(lo, sh_lo[w]);
    hi = fmaxf(hi, sh_hi[w]);
  }
  hi = (float)fmax((double)hi, (double)lo + 1e-5);
  const bool ok = hi > lo;            // false only where lo + 1e-5 rounds back to lo (|lo| >= 128) or the image holds no finite value
  for (long o = threadIdx.x; o < n; o += TPB) {
    const long p = o / 3;
    const int c = (int)(o - 3 * p);
    oi[o] = ok ? save_image_u8(xi[(long)c * HW + p], lo, hi) : (uint8_t)0;
  }
}

}  // namespace

extern "C" {

int sfron_ddpm_guided_step(const float* x, const float* eps_cond, const float* eps_null, const float* noise, double cond_scale,
                           const float* coef, int steps, const int32_t* step, int64_t n, float* x_next, float* x0_pred, void* stream) {
  SFRON_CHECK_ARG(x && eps_cond && coef && step && x_next && n > 0 && steps > 0 && isfinite(cond_scale));
  SFRON_CHECK_ARG(x0_pred != x && x0_pred != x_next);                // only x_next may alias x
  long gx = (n + TPB - 1) / TPB;                                     // 64-bit element index in the kernel: no byte limit
  if (gx > 4096) gx = 4096;
  // the two factors exactly as the callers of sfron_axpby form them: 1.0 + s and -s in double (the scale arrives as the caller's double),
  // each rounded ONCE to fp32 -- the same bits for every scale, not only those fp32 holds exactly
  const float alpha = (float)(1.0 + cond_scale), beta = (float)(-cond_scale);
  hipLaunchKernelGGL(k_ddpm_guided_step, dim3((int)gx), dim3(TPB), 0, (hipStream_t)stream, x, eps_cond, eps_null, noise, alpha, beta, coef,
                     steps, (const int*)step, (long)n, x_next, x0_pred);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_ddpm_sampler_advance(const float* tseq, int steps, int32_t* step, float* t, int nt, void* stream) {
  SFRON_CHECK_ARG(tseq && step && t && steps > 0 && nt > 0);
  hipLaunchKernelGGL(k_ddpm_sampler_advance, dim3(1), dim3(TPB), 0, (hipStream_t)stream, tseq, steps, (int*)step, t, nt);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_images_normalize_u8(const float* x, int B, int H, int W, uint8_t* out, void* stream) {
  SFRON_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0);
  SFRON_CHECK_ARG((int64_t)H * W < (1ll << 29) && (int64_t)B * H * W * 3 < (1ll << 31));
  hipLaunchKernelGGL(k_images_normalize_u8, dim3(B), dim3(TPB), 0, (hipStream_t)stream, x, H * W, out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
