// DiT guided sampling (sfron.dit_sample.DiTSampler, sfron.diffusion.GaussianDiffusion.ddim_*): the per-step update behind one forward pass
// and the device-side step counter that lets the loop run without a host tensor per step.
//   sfron_dit_sample_step      forward_with_cfg's guidance mix (DiT/models.py:250-266) + one step of DiT/diffusion/gaussian_diffusion.py:
//                              p_sample (:376-421), ddim_sample (:513-560) or ddim_reverse_sample (:562-598), per-row table index
//   sfron_dit_sampler_advance  t_idx <- order[k + 1], t_model <- timestep_map[t_idx], k <- k + 1 (one workgroup, a launch of its own behind
//                              the step kernel)
// Built with -ffp-contract=off like the rest of the library: no product is fused into a sum, so in mode DDPM the step kernel gives, on the
// n rows, the bits of sfron_cfg_combine followed by sfron_p_sample (csrc/loss.hip k_cfg_combine, k_p_sample) on the same inputs.
#include <math.h>

#include "../../include/sfron.h"
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int STAB = 11;        // columns of the sampler table: k_p_sample's eight, then alphas_cumprod, _prev, _next

// Grid (gx, n): workgroup row blockIdx.y owns sample n, as in k_p_sample; the row's table entries and everything derived from them alone
// (sigma, the square roots) are uniform over the workgroup.  Streaming, HBM-bound: x, one or two rows of model_out and the noise in, one
// to three tensors out; no LDS.  sample may be x (each element is read before it is written, by the same thread): x carries no __restrict__.
template <int MODE, bool GUIDED>
__global__ __launch_bounds__(TPB) void k_dit_sample_step(const float* x, const float* __restrict__ out, const int64_t* __restrict__ t,
                                                         const float* __restrict__ stab, const float* __restrict__ noise, int nb, int chw,
                                                         int n_guided_hw, float s, float eta, int clip, float* sample,
                                                         float* __restrict__ dup, float* __restrict__ pred) {
  const int n = blockIdx.y;
  const int64_t tn = t[n];
  const float* row = stab + (size_t)tn * STAB;
  const float sra = row[2], srm1 = row[3], c1 = row[4], c2 = row[5], min_log = row[6], max_log = row[7];
  const float nz = tn != 0 ? 1.0f : 0.0f;
  // the per-row scalars of ddim_sample / ddim_reverse_sample, each a separately rounded fp32 operation in the reference's order
  float ca = 0.0f, cb = 0.0f, sig = 0.0f;
  if (MODE == SFRON_DIT_SAMPLE_DDIM) {
    const float ab = row[8], abp = row[9];
    const float sigma = (eta * sqrtf((1.0f - abp) / (1.0f - ab))) * sqrtf(1.0f - ab / abp);
    ca = sqrtf(abp);
    cb = sqrtf((1.0f - abp) - sigma * sigma);
    sig = nz * sigma;
  } else if (MODE == SFRON_DIT_SAMPLE_DDIM_REVERSE) {
    const float abn = row[10];
    ca = sqrtf(abn);
    cb = sqrtf(1.0f - abn);
  }
  const size_t xb = (size_t)n * chw, ob = (size_t)n * 2 * chw, ub = (size_t)(n + nb) * 2 * chw;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < chw; i += gridDim.x * TPB) {
    const float xv = x[xb + i], v = out[ob + chw + i];
    float eps = out[ob + i];
    if (GUIDED && i < n_guided_hw) {
      const float u = out[ub + i];
      eps = u + s * (eps - u);                          // k_cfg_combine
    }
    float px = sra * xv - srm1 * eps;                   // k_p_sample
    if (clip) px = fminf(fmaxf(px, -1.0f), 1.0f);
    float r;
    if (MODE == SFRON_DIT_SAMPLE_DDPM) {
      const float frac = (v + 1.0f) / 2.0f;
      const float lv = frac * max_log + (1.0f - frac) * min_log;
      const float mean = c1 * px + c2 * xv;
      r = mean + (nz * expf(0.5f * lv)) * noise[xb + i];
    } else {
      const float e2 = (sra * xv - px) / srm1;          // _predict_eps_from_xstart
      const float mean = px * ca + cb * e2;
      r = MODE == SFRON_DIT_SAMPLE_DDIM ? mean + sig * (noise ? noise[xb + i] : 0.0f) : mean;
    }
    sample[xb + i] = r;
    if (dup) dup[xb + i] = r;
    if (pred) pred[xb + i] = px;
  }
}

// One workgroup.  Every thread reads the index, the barrier separates those reads from thread 0's write.  The index stops at `steps` (one
// past the last entry: the next launch clamps it back); a launch past the end repeats the last entry.
__global__ __launch_bounds__(TPB) void k_dit_sampler_advance(const int64_t* __restrict__ order, const int64_t* __restrict__ tmap, int steps,
                                                             int map_len, int* step, int64_t* __restrict__ t_idx, int n,
                                                             int64_t* __restrict__ t_model, int rows) {
  int k = *step;
  k = k < 0 ? 0 : (k >= steps ? steps - 1 : k);
  const int next = k + 1;
  int64_t i = order[next < steps ? next : steps - 1];
  i = i < 0 ? 0 : (i >= map_len ? map_len - 1 : i);
  const int64_t tm = tmap[i];
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += TPB) t_idx[j] = i;
  for (int j = threadIdx.x; j < rows; j += TPB) t_model[j] = tm;
  if (threadIdx.x == 0) *step = next;
}

template <int MODE>
void launch_step(bool guided, dim3 grid, hipStream_t st, const float* x, const float* out, const int64_t* t, const float* stab,
                 const float* noise, int n, int chw, int ngh, float s, float eta, int clip, float* sample, float* dup, float* pred) {
  if (guided)
    hipLaunchKernelGGL((k_dit_sample_step<MODE, true>), grid, dim3(TPB), 0, st, x, out, t, stab, noise, n, chw, ngh, s, eta, clip, sample, dup, pred);
  else
    hipLaunchKernelGGL((k_dit_sample_step<MODE, false>), grid, dim3(TPB), 0, st, x, out, t, stab, noise, n, chw, ngh, s, eta, clip, sample, dup, pred);
}

}  // namespace

extern "C" {

int sfron_dit_sample_step(const float* x, const float* model_out, const int64_t* t, const float* stab, const float* noise, int n, int c,
                          int hw, int guided, int n_guided, float cfg_scale, int mode, float eta, int clip_denoised, float* sample,
                          float* sample_dup, float* pred_xstart, void* stream) {
  SFRON_CHECK_ARG(x && model_out && t && stab && sample && n > 0 && c > 0 && hw > 0);
  SFRON_CHECK_ARG(n_guided >= 0 && n_guided <= c && isfinite(cfg_scale) && isfinite(eta));
  SFRON_CHECK_ARG(mode == SFRON_DIT_SAMPLE_DDPM || mode == SFRON_DIT_SAMPLE_DDIM || mode == SFRON_DIT_SAMPLE_DDIM_REVERSE);
  SFRON_CHECK_ARG(mode != SFRON_DIT_SAMPLE_DDIM_REVERSE || eta == 0.0f);
  SFRON_CHECK_ARG(noise || mode == SFRON_DIT_SAMPLE_DDIM_REVERSE || (mode == SFRON_DIT_SAMPLE_DDIM && eta == 0.0f));
  SFRON_CHECK_ARG(!pred_xstart || (pred_xstart != x && pred_xstart != sample && pred_xstart != sample_dup));   // only sample may alias x
  SFRON_CHECK_ARG(!sample_dup || (sample_dup != x && sample_dup != sample));
  SFRON_CHECK_ARG((int64_t)n * c * hw < (1ll << 31) && n <= 65535);          // chw and n_guided * hw are int; n is the grid's y extent
  const int chw = c * hw;
  int gx = cdiv(chw, TPB);
  if (gx > 64) gx = 64;
  const dim3 grid(gx, n);
  const hipStream_t st = (hipStream_t)stream;
  const bool g = guided != 0;
  const int ngh = n_guided * hw, clip = clip_denoised != 0;
  if (mode == SFRON_DIT_SAMPLE_DDPM)
    launch_step<SFRON_DIT_SAMPLE_DDPM>(g, grid, st, x, model_out, t, stab, noise, n, chw, ngh, cfg_scale, eta, clip, sample, sample_dup, pred_xstart);
  else if (mode == SFRON_DIT_SAMPLE_DDIM)
    launch_step<SFRON_DIT_SAMPLE_DDIM>(g, grid, st, x, model_out, t, stab, noise, n, chw, ngh, cfg_scale, eta, clip, sample, sample_dup, pred_xstart);
  else
    launch_step<SFRON_DIT_SAMPLE_DDIM_REVERSE>(g, grid, st, x, model_out, t, stab, noise, n, chw, ngh, cfg_scale, eta, clip, sample, sample_dup,
                                               pred_xstart);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_dit_sampler_advance(const int64_t* order, const int64_t* timestep_map, int steps, int map_len, int32_t* step, int64_t* t_idx, int n,
                              int64_t* t_model, int rows, void* stream) {
  SFRON_CHECK_ARG(order && timestep_map && step && t_idx && t_model && steps > 0 && map_len > 0 && n > 0 && rows > 0);
  hipLaunchKernelGGL(k_dit_sampler_advance, dim3(1), dim3(TPB), 0, (hipStream_t)stream, order, timestep_map, steps, map_len, (int*)step, t_idx,
                     n, t_model, rows);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
