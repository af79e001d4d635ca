// The ldm PLMS sampler (sfron.plms.PLMSSampler; SD/ldm/models/diffusion/plms.py): the per-step update behind one guided UNet call, and the
// inpainting blend in front of it.
//   sfron_plms_cfg_step   classifier-free guidance + the pseudo linear multistep combination of the last (up to) four predictions + the
//                         eta = 0 DDIM update, one pass
//   sfron_inpaint_blend   q_sample(x0, t) * mask + (1 - mask) * img with a [B or 1][C or 1][hw] mask, one pass
// Built with -ffp-contract=off like the rest of the library, and these kernels rely on it: every step below is ONE rounded fp32 operation in
// the reference's left-to-right order, so the results are the bits torch gives on the CPU.  fp32 only, 64-bit element index, a grid-stride
// loop over a capped grid.
#include <math.h>

#include "../../include/sfron.h"
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr long MAX_BLOCKS = 4096;

// e = eu + g (ec - eu) (ec == NULL: e = eu), kept in e_out when given;  e' by ORDER (plms.py:363-378; the divisions are IEEE divisions):
//   ORDER1  e                         ORDER3  ((23 e - 16 o1) + 5 o2) / 12
//   ORDER2  (3 e - o1) / 2            ORDER4  (((55 e - 59 o1) + 37 o2) - 9 o3) / 24
//   MEAN    (o1 + e) / 2: the second half of the first step (o1 = that step's e_t, e = e_t_next)
// pred = (x - s1 e') / s2;  x_prev = s3 pred + dir e'.
// x_prev may be x and e_out may be a history buffer: a thread reads all of an element's operands before it writes any of its results, and
// no other thread touches that element (hence no __restrict__ here).
template <int ORDER>
__global__ __launch_bounds__(TPB) void k_plms_cfg_step(const float* x, const float* eu, const float* ec, const float* o1, const float* o2,
                                                       const float* o3, long n, float g, float s1, float s2, float s3, float dir, float* e_out,
                                                       float* x_prev, float* pred_x0) {
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
    const float xi = x[i];
    float e = eu[i];
    if (ec) e = e + g * (ec[i] - e);
    float ep = e;
    if (ORDER == SFRON_PLMS_ORDER2) {
      ep = (3.0f * e - o1[i]) / 2.0f;
    } else if (ORDER == SFRON_PLMS_ORDER3) {
      const float a = o1[i], b = o2[i];
      ep = ((23.0f * e - 16.0f * a) + 5.0f * b) / 12.0f;
    } else if (ORDER == SFRON_PLMS_ORDER4) {
      const float a = o1[i], b = o2[i], c = o3[i];
      ep = (((55.0f * e - 59.0f * a) + 37.0f * b) - 9.0f * c) / 24.0f;
    } else if (ORDER == SFRON_PLMS_MEAN) {
      ep = (o1[i] + e) / 2.0f;
    }
    const float pred = (xi - s1 * ep) / s2;
    const float xp = s3 * pred + dir * ep;
    if (e_out) e_out[i] = e;
    x_prev[i] = xp;
    if (pred_x0) pred_x0[i] = pred;
  }
}

// plms.py:228-233 with q_sample's two products and one sum (ddpm.py:424-445):  orig = sa x0 + sb noise;  out = orig m + (1 - m) img.
// i runs over [B][C][hw]; the mask is [mb][mc][hw] with mb in {1, B}, mc in {1, C}.  out may be img (read before written, same thread).
__global__ __launch_bounds__(TPB) void k_inpaint_blend(const float* img, const float* x0, const float* noise, const float* mask, long n, int C,
                                                       long hw, int mb, int mc, float sa, float sb, float* out) {
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long)gridDim.x * TPB) {
    const long bc = i / hw, p = i - bc * hw;
    const long b = bc / C, c = bc - b * C;
    const float m = mask[((mb == 1 ? 0 : b) * mc + (mc == 1 ? 0 : c)) * hw + p];
    const float orig = sa * x0[i] + sb * noise[i];
    const float v = orig * m + (1.0f - m) * img[i];
    out[i] = v;
  }
}

int capped_grid(long n) {
  long gx = (n + TPB - 1) / TPB;
  return (int)(gx > MAX_BLOCKS ? MAX_BLOCKS : gx);
}

}  // namespace

extern "C" {

int sfron_plms_cfg_step(const float* x, const float* eps_uncond, const float* eps_cond, const float* old1, const float* old2,
                        const float* old3, int order, int64_t n, float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_a_prev,
                        float dir_coef, float* e_out, float* x_prev, float* pred_x0, void* stream) {
  SFRON_CHECK_ARG(x && eps_uncond && x_prev && n > 0 && sqrt_at != 0.0f && isfinite(guidance));
  SFRON_CHECK_ARG(order >= SFRON_PLMS_ORDER1 && order <= SFRON_PLMS_MEAN);
  SFRON_CHECK_ARG(order == SFRON_PLMS_ORDER1 || old1);
  SFRON_CHECK_ARG((order != SFRON_PLMS_ORDER3 && order != SFRON_PLMS_ORDER4) || old2);
  SFRON_CHECK_ARG(order != SFRON_PLMS_ORDER4 || old3);
  const dim3 grid(capped_grid((long)n)), block(TPB);                 // 64-bit element index in the kernel: no byte limit
  const hipStream_t s = (hipStream_t)stream;
#define PLMS_LAUNCH(ORD)                                                                                                                  \
  hipLaunchKernelGGL(k_plms_cfg_step<ORD>, grid, block, 0, s, x, eps_uncond, eps_cond, old1, old2, old3, (long)n, guidance, sqrt_one_minus_at, \
                     sqrt_at, sqrt_a_prev, dir_coef, e_out, x_prev, pred_x0)
  switch (order) {
    case SFRON_PLMS_ORDER1: PLMS_LAUNCH(SFRON_PLMS_ORDER1); break;
    case SFRON_PLMS_ORDER2: PLMS_LAUNCH(SFRON_PLMS_ORDER2); break;
    case SFRON_PLMS_ORDER3: PLMS_LAUNCH(SFRON_PLMS_ORDER3); break;
    case SFRON_PLMS_ORDER4: PLMS_LAUNCH(SFRON_PLMS_ORDER4); break;
    default: PLMS_LAUNCH(SFRON_PLMS_MEAN); break;
  }
#undef PLMS_LAUNCH
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_inpaint_blend(const float* img, const float* x0, const float* noise, const float* mask, int B, int C, int64_t hw, int mask_b,
                        int mask_c, float sqrt_ac, float sqrt_one_minus_ac, float* out, void* stream) {
  SFRON_CHECK_ARG(img && x0 && noise && mask && out && B > 0 && C > 0 && hw > 0);
  SFRON_CHECK_ARG((mask_b == 1 || mask_b == B) && (mask_c == 1 || mask_c == C));
  SFRON_CHECK_ARG(hw <= INT64_MAX / ((int64_t)B * C));
  const long n = (long)B * C * hw;
  hipLaunchKernelGGL(k_inpaint_blend, dim3(capped_grid(n)), dim3(TPB), 0, (hipStream_t)stream, img, x0, noise, mask, n, C, (long)hw, mask_b,
                     mask_c, sqrt_ac, sqrt_one_minus_ac, out);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
