// DiT likelihood evaluation (sfron.diffusion.GaussianDiffusion._vb_terms_bpd / _prior_bpd / calc_bpd_loop, sfron.dit_bpd.DiTBpdEvaluator):
// the forward-only term of the variational bound behind one forward pass, for the LEARNED_RANGE / EPSILON model.
//   sfron_dit_bpd_step    one term of DiT/diffusion/gaussian_diffusion.py calc_bpd_loop (:827-844): _vb_terms_bpd (:682-713) over
//                         p_mean_variance (:285-293,310-323) and q_posterior_mean_variance (:232-252), then the x_0 mse and the mse of
//                         the epsilon RE-DERIVED from the (possibly clamped) pred_xstart (_predict_eps_from_xstart, :341-344); the same
//                         launch writes q_sample (:215-230) of the NEXT step into the model's input buffer
//   sfron_dit_prior_bpd   _prior_bpd (:789-803)
// normal_kl / approx_standard_normal_cdf / discretized_gaussian_log_likelihood: diffusion_utils.py:10-44,62-88, expression for expression.
// Built with -ffp-contract=off like the rest of the library: x_t = sa * x0 + s1 * noise is k_q_sample's expression (csrc/loss.hip) and has
// its bits.  Unlike k_dit_loss nothing is frozen and no gradient is written.
//
// One workgroup per sample: streaming, HBM-bound, no LDS beyond the 3 x 4 doubles of the reduction.  Per-thread partial sums are kept in
// fp64, reduced over the wave by shuffles and over the four waves in a fixed order by thread 0: no floating-point atomics, the same inputs
// give the same bits.  Every element offset is 64-bit.
#include <math.h>

#include "../../include/sfron.h"
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr double LN2 = 0.6931471805599453;

__device__ __forceinline__ float cdf_ref(float x) {          // diffusion_utils.py:44; th.pow(x, 3) is (x * x) * x
  return 0.5f * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * ((x * x) * x))));
}

// thread 0 returns the three sums over the workgroup (every thread must call)
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c) {
  __shared__ double sh[3][TPB / 64];
  a = wave_sum_d(a), b = wave_sum_d(b), c = wave_sum_d(c);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; sh[2][threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = b = c = 0.0;
    for (int i = 0; i < TPB / 64; ++i) { a += sh[0][i]; b += sh[1][i]; c += sh[2][i]; }
  }
}

// xt_in == nullptr: x_t is recomputed from the noise; noise == nullptr: no epsilon mse (mse_out is null then).  A table index outside
// [0, T) -- t lives on the device, the host cannot refuse it -- reads no table row: the row's outputs are NaN.  The output column is
// *step when step is given (the loop form), else col; a device counter outside [0, ld) writes no term.
__global__ __launch_bounds__(TPB) void k_dit_bpd_step(const float* __restrict__ x0, const float* __restrict__ xt_in,
                                                      const float* __restrict__ noise, const float* __restrict__ out,
                                                      const int64_t* __restrict__ t, const float* __restrict__ tab, int T, int chw, int clip,
                                                      float* __restrict__ vb_out, float* __restrict__ xs_out, float* __restrict__ mse_out,
                                                      int ld, const int* __restrict__ step, int col, float* __restrict__ pred,
                                                      const float* __restrict__ next_noise, const int64_t* __restrict__ order, int steps,
                                                      float* __restrict__ next_xt) {
  const int n = blockIdx.x;
  const int k = step ? *step : col;
  const int64_t tn = t[n];
  const bool t_ok = tn >= 0 && tn < T;
  const float* row = tab + (size_t)(t_ok ? tn : 0) * 8;
  const float sa = row[0], s1 = row[1], sra = row[2], srm1 = row[3], c1 = row[4], c2 = row[5];
  const float min_log = row[6], max_log = row[7];
  // the next step's q_sample coefficients: order[k + 1], nothing past the last step
  float nsa = 0.0f, ns1 = 0.0f;
  bool has_next = false;
  if (next_xt && k >= 0 && k + 1 < steps) {
    const int64_t i = order[k + 1];
    if (i >= 0 && i < T) { nsa = tab[(size_t)i * 8], ns1 = tab[(size_t)i * 8 + 1]; has_next = true; }
  }
  const size_t xb = (size_t)n * chw, ob = (size_t)n * 2 * chw;
  double acc_vb = 0.0, acc_xs = 0.0, acc_mse = 0.0;
  for (int i = threadIdx.x; i < chw; i += TPB) {
    const float x = x0[xb + i];
    const float e = noise ? noise[xb + i] : 0.0f;
    const float eh = out[ob + i], vv = out[ob + chw + i];
    const float xt = xt_in ? xt_in[xb + i] : sa * x + s1 * e;                 // k_q_sample
    const float frac = (vv + 1.0f) / 2.0f;
    const float lv = frac * max_log + (1.0f - frac) * min_log;
    float px = sra * xt - srm1 * eh;                                          // _predict_xstart_from_eps
    if (clip) px = fminf(fmaxf(px, -1.0f), 1.0f);
    const float mu_t = c1 * px + c2 * xt;                                     // model mean
    const float mu_q = c1 * x + c2 * xt;                                      // true posterior mean
    float term;
    if (tn == 0) {                                                            // decoder NLL
      const float cx = x - mu_t;
      const float inv_std = expf(-(0.5f * lv));
      const float cdf_plus = cdf_ref(inv_std * (cx + (float)(1.0 / 255.0)));
      const float cdf_min = cdf_ref(inv_std * (cx - (float)(1.0 / 255.0)));
      const float q = x < -0.999f ? cdf_plus : (x > 0.999f ? 1.0f - cdf_min : cdf_plus - cdf_min);
      term = -logf(fmaxf(q, 1e-12f));
    } else {                                                                  // normal_kl(mu_q, min_log, mu_t, lv)
      const float dmu = mu_q - mu_t;
      term = 0.5f * ((((-1.0f + lv) - min_log) + expf(min_log - lv)) + (dmu * dmu) * expf(-lv));
    }
    acc_vb += (double)term;
    const float dx = px - x;
    acc_xs += (double)(dx * dx);
    if (noise) {
      const float de = (sra * xt - px) / srm1 - e;                            // _predict_eps_from_xstart
      acc_mse += (double)(de * de);
    }
    if (pred) pred[xb + i] = px;
    if (has_next) next_xt[xb + i] = nsa * x + ns1 * next_noise[xb + i];       // k_q_sample at order[k + 1]
  }
  block_sum3(acc_vb, acc_xs, acc_mse);
  if (threadIdx.x == 0 && k >= 0 && k < ld) {
    const size_t o = (size_t)n * ld + k;
    const float bad = __builtin_nanf("");
    if (vb_out) vb_out[o] = t_ok ? (float)(acc_vb / chw / LN2) : bad;
    if (xs_out) xs_out[o] = t_ok ? (float)(acc_xs / chw) : bad;
    if (mse_out) mse_out[o] = t_ok ? (float)(acc_mse / chw) : bad;
  }
}

// normal_kl(mean1 = sa * x0, logvar1 = lv1, 0, 0) = 0.5 * (-1 + 0 - lv1 + exp(lv1 - 0) + (mean1 - 0)^2 * exp(-0))
__global__ __launch_bounds__(TPB) void k_dit_prior_bpd(const float* __restrict__ x0, int chw, float sa, float lv1, float* __restrict__ out) {
  const int n = blockIdx.x;
  const size_t xb = (size_t)n * chw;
  const float head = ((-1.0f + 0.0f) - lv1) + expf(lv1 - 0.0f);
  double acc = 0.0, z0 = 0.0, z1 = 0.0;
  for (int i = threadIdx.x; i < chw; i += TPB) {
    const float m = sa * x0[xb + i];
    acc += (double)(0.5f * (head + (m * m) * 1.0f));
  }
  block_sum3(acc, z0, z1);
  if (threadIdx.x == 0) out[n] = (float)(acc / chw / LN2);
}

}  // namespace

extern "C" {

int sfron_dit_bpd_step(const float* x0, const float* x_t, const float* noise, const float* model_out, const int64_t* t, const float* tab,
                       int T, int n, int c, int hw, int clip_denoised, float* vb, float* xstart_mse, float* mse, int ld, const int32_t* step,
                       int col, float* pred_xstart, const float* next_noise, const int64_t* order, int steps, float* next_xt, void* stream) {
  SFRON_CHECK_ARG(x0 && model_out && t && tab && vb && (x_t || noise) && T > 0 && n > 0 && c > 0 && hw > 0);
  SFRON_CHECK_ARG(!mse || noise);                                            // the epsilon mse needs this step's noise
  SFRON_CHECK_ARG(ld > 0 && (step || (col >= 0 && col < ld)));               // the output column lies inside the [n][ld] matrices
  SFRON_CHECK_ARG((int64_t)n * c * hw < (1ll << 31) && (int64_t)n * ld < (1ll << 31));
  SFRON_CHECK_ARG(!next_xt || (next_noise && order && step && steps > 0 && steps <= ld));
  SFRON_CHECK_ARG(!next_xt || (next_xt != x0 && next_xt != x_t && next_xt != noise && next_xt != next_noise && next_xt != pred_xstart));
  SFRON_CHECK_ARG(!pred_xstart || (pred_xstart != x0 && pred_xstart != x_t && pred_xstart != noise));
  hipLaunchKernelGGL(k_dit_bpd_step, dim3(n), dim3(TPB), 0, (hipStream_t)stream, x0, x_t, noise, model_out, t, tab, T, c * hw,
                     clip_denoised != 0, vb, xstart_mse, mse, ld, (const int*)step, col, pred_xstart, next_noise, order, steps, next_xt);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_dit_prior_bpd(const float* x0, int n, int c, int hw, float sqrt_ac_last, float log_one_minus_ac_last, float* prior_bpd,
                        void* stream) {
  SFRON_CHECK_ARG(x0 && prior_bpd && n > 0 && c > 0 && hw > 0 && (int64_t)n * c * hw < (1ll << 31));
  SFRON_CHECK_ARG(isfinite(sqrt_ac_last) && isfinite(log_one_minus_ac_last));
  hipLaunchKernelGGL(k_dit_prior_bpd, dim3(n), dim3(TPB), 0, (hipStream_t)stream, x0, c * hw, sqrt_ac_last, log_one_minus_ac_last,
                     prior_bpd);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
