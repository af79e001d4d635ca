/* sfron.h -- C ABI of libsfron.so: the MI355X (gfx950) SFR-on unlearning hot path.
 *
 * The reference (K1nght/Unified-Unlearning-w-Remain-Geometry) is 100 % Python and has no FFI:
 * its "operator interface" for this path is the PyTorch op sequences inside
 *   DiT/forget.py:256-322, DiT/diffusion/gaussian_diffusion.py:715-787, DiT/models.py:233-248.
 * Each entry point below replaces one of those sequences (cited per function) and is what a
 * ctypes / cffi binding on the reference side would call (INTEGRATION.md shows the stubs).
 *
 * Conventions: plain pointers and sizes only (no torch types); every pointer is a DEVICE pointer
 * unless stated; `stream` is a hipStream_t passed as void* (NULL = default stream); all launches
 * are asynchronous on `stream`; return 0 on success, a hipError_t value or SFRON_ERR_* (>= 1001)
 * on failure; nothing throws.  bf16 tensors are passed as uint16_t*.
 *
 * State: every tensor, workspace, stream and event belongs to the caller or to a handle the caller creates (sfron_aux_create,
 * sfron_probe_create); entry points are re-entrant per stream.  Process-wide state is limited to (a) three SCHEDULE switches --
 * sfron_gemm_loader_waves, sfron_attn_fwd_form, sfron_attn_bwd_form: each picks between schedules that give the same bits (the tests
 * compare them), so no result depends on them (sfron_attn_bwd_form: the same values to fp32 rounding); not thread-safe, meant for tests
 * and A-B timing -- and (b) since ABI 15 a per-device FREE LIST of weight-gradient stream pairs: sfron_aux_destroy returns a handle's two HIP
 * streams to it (drained) and the next sfron_aux_create on that device takes them instead of creating new ones, so that a process that builds
 * one engine after another keeps running on the same streams (the runtime maps streams onto four hardware queues; a later handle with fresh
 * streams can land on a queue another stream of the step uses: measured 4 ms per step, profiles/r06_fp8_leg.txt).  Two live handles never
 * share a pair.  The fp8 activation-range counters (rounds 4-5: a __device__ global) are a caller-owned device array since ABI 15
 * (sfron_fp8_activation_amax).  One host thread per device drives the library.
 */
#ifndef SFRON_H
#define SFRON_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ version / probing */
int sfron_abi_version(void);            /* bumps when a signature changes */
const char* sfron_build_arch(void);     /* "gfx950" */

/* ------------------------------------------------------------------ parameter sweep (sweep.hip)
 * Flat fp32 arenas: params, grads, exp_avg, exp_avg_sq, ema share offsets; mask is 1 byte/element
 * (torch.bool storage, 0/1); w_bf16 is the bf16 shadow the GEMMs read. */

/* length (in doubles) the `partials` scratch of sfron_sumsq_masked must have */
int sfron_sweep_partials_len(void);

/* partial sums of (mask ? g : 0)^2; first half of clip_grad_norm_ after `grad *= mask`
 * (DiT/forget.py:289-298).  mask may be NULL.  *nblk_out (HOST int) = number of partials written.
 * g2 (may be NULL): a second gradient arena added element-wise first (g + g2): the two micro-batch chains of a
 * step write disjoint arenas so they never have to order their weight-gradient GEMMs against each other. */
int sfron_sumsq_masked(const float* g, const float* g2, const uint8_t* mask, int64_t n, double* partials, int* nblk_out,
                       void* stream);

/* the same partial sums over a table of element ranges: ranges (DEVICE) int64 [n_ranges][2] = {offset, length} into g / mask (multiples of 4;
 * a range is summed by ONE workgroup: split tensors above ~64 K elements); partials[r] = sum over range r of (mask ? g : 0)^2.  What the clip
 * norm still reads when the weight-gradient GEMMs leave their own sums (sfron_gemm_desc.sumsq_partials, sfron_aux_arm_sumsq). */
int sfron_sumsq_masked_ranges(const float* g, const uint8_t* mask, const int64_t* ranges, int n_ranges, double* partials, void* stream);

/* stats[0] = ||g||_2, stats[1] = min(1, max_norm / (norm + 1e-6)), stats[2] = sum of squares
 * (torch.nn.utils.clip_grad_norm_ semantics; DiT/forget.py:293-298) */
int sfron_clip_coef(const double* partials, int nblk, float max_norm, float* stats, void* stream);

/* fused: g' = (mask ? g : 0) * stats[1]; Adam/AdamW single-tensor update of (p, m, v) with
 * host-computed (double, rounded to fp32 exactly where torch rounds) step_size = lr / (1 - beta1^step),
 * bc2_sqrt = sqrt(1 - beta2^step),
 * decay_mul = 1 - lr * weight_decay (1.0 for the reference's wd = 0); optional bf16 shadow write;
 * optional fused EMA of the NEW p: ema_mode 0 none, 1 DiT (ema*d + (1-d)*p, DiT/forget.py:52-62),
 * 2 DDPM ((1-mu)*p + mu*shadow, DDPM/models/ema.py:17-24).  mask / stats / w_bf16 / ema may be NULL.
 * (DiT/forget.py:289-299,320; DDPM/runners/diffusion.py:1126-1138,1169-1180) */
int sfron_masked_clip_adam(float* p, const float* g, const float* g2 /* NULL or second arena, see above */, float* m, float* v,
                           const uint8_t* mask, const float* stats,
                           int64_t n, double beta1, double beta2, double eps, double step_size, double bc2_sqrt,
                           double decay_mul, uint16_t* w_bf16, float* ema, double ema_decay, int ema_mode, void* stream);

/* the same sweep on at most max_workgroups workgroups of 256 threads (0 = as many as the range offers, capped at 2048): a
 * sweep issued on a second stream BESIDE a GEMM chain takes a bounded share of the chip's wave slots and HBM queue */
int sfron_masked_clip_adam_wg(float* p, const float* g, const float* g2, float* m, float* v, const uint8_t* mask, const float* stats,
                              int64_t n, double beta1, double beta2, double eps, double step_size, double bc2_sqrt,
                              double decay_mul, uint16_t* w_bf16, float* ema, double ema_decay, int ema_mode, int max_workgroups,
                              void* stream);

/* config 5: the sweep over ONE weight tensor (+ its bias) that also writes the e4m3 shadow of the new values, w_e4m3[i] =
 * e4m3(p_new[i] * *w_e4m3_scale) (device scalar from sfron_fp8_update_scales): the optimizer step re-quantises what it touches, no
 * second pass over the masters.  n % 4 == 0; max_workgroups as sfron_masked_clip_adam_wg. */
int sfron_masked_clip_adam_q(float* p, const float* g, float* m, float* v, const uint8_t* mask, const float* stats, int64_t n, double beta1,
                             double beta2, double eps, double step_size, double bc2_sqrt, double decay_mul, uint16_t* w_bf16, float* ema,
                             double ema_decay, int ema_mode, uint8_t* w_e4m3, const float* w_e4m3_scale, int max_workgroups, void* stream);

/* The same two sweeps over a weight matrix W [NM][D] (p / m / v / mask / w_bf16 / ema point at ITS first element) whose gradient is
 * a rank-R product dW[n][k] = sum_{b < R} dmod[b][n] * sc[b][k] (bf16 factors, fp32 accumulation in index order), formed inside
 * the sweep instead of by a weight-gradient GEMM that writes NM*D floats for the sweep to read back: the adaLN_modulation Linears
 * of all DiT blocks (DiT/models.py:113-116,131-134: input silu(c) [batch][D], a third of DiT-XL/2's parameters; R = batch).
 * NM % 8 == 0, D % 4 == 0.  sumsq: *nblk_out partials (NM / 8), to be combined with the other ranges' by sfron_clip_coef. */
int sfron_sumsq_lowrank(const uint16_t* dmod, const uint16_t* sc, int R, int NM, int D, const uint8_t* mask, double* partials,
                        int* nblk_out, void* stream);
int sfron_adam_lowrank(float* p, float* m, float* v, const uint8_t* mask, const float* stats, const uint16_t* dmod, const uint16_t* sc, int R,
                       int NM, int D, double beta1, double beta2, double eps, double step_size, double bc2_sqrt, double decay_mul,
                       uint16_t* w_bf16, float* ema, double ema_decay, int ema_mode, void* stream);

/* stand-alone EMA (frozen parameters such as pos_embed; DiT/forget.py:60-62) */
int sfron_ema_update(float* ema, const float* p, int64_t n, double decay, int ema_mode, void* stream);

/* F += g^2 / n_iters (DiT/generate_fisher.py:236-239, on device instead of .cpu()) */
int sfron_fisher_accum(float* fisher, const float* g, int64_t n, float n_iters, void* stream);

/* F += ((g [+ g2]) * stats[1])^2 / n_iters: the DDPM variant squares the gradient AFTER clip_grad_norm_
 * (DDPM/runners/diffusion.py:1271-1281); stats from sfron_clip_coef (NULL = no clipping), g2 NULL or a second arena added first */
int sfron_fisher_accum_clipped(float* fisher, const float* g, const float* g2, const float* stats, int64_t n, float n_iters, void* stream);

/* mask = ((F_f + 1e-15) / (F_r + 1e-15)) >= th, IEEE fp32, bit-exact with torch
 * (DiT/generate_mask.py:34-35, DDPM/generate_fisher_mask.py:39-46) */
int sfron_mask_from_fisher(const float* forget_fisher, const float* remain_fisher, int64_t n, float th,
                           uint8_t* mask, void* stream);

/* fp32 -> bf16 (RNE) */
int sfron_cast_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------ diffusion loss (loss.hip)
 * tab: [T][8] fp32 rows = { sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod,
 *   sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1,
 *   posterior_mean_coef2, posterior_log_variance_clipped, log(betas) }
 * (DiT/diffusion/gaussian_diffusion.py:167-201, gathered as fp32 like _extract_into_tensor :861-873) */
#define SFRON_TAB_COLS 8

/* x_t = sqrt_ac[t] * x0 + sqrt_1m_ac[t] * noise   (gaussian_diffusion.py:215-230); t is int64 [n] */
int sfron_q_sample(const float* x0, const float* noise, const int64_t* t, const float* tab, int n, int chw, float* x_t,
                   void* stream);

/* model_out [n, 2c, hw] -> mse[n], vb[n] (loss = mse + vb) and
 * d_model_out = d( grad_scale * sum_i loss_i ) / d model_out      (gaussian_diffusion.py:746-783, 682-713)
 * grad_scale = (+/- forget_alpha or 1) / global_batch reproduces `(alpha * -loss.mean()).backward()`
 * (DiT/forget.py:272,286-288,311). */
int sfron_dit_loss_fwd_bwd(const float* x0, const float* noise, const float* model_out, const int64_t* t,
                           const float* tab, int n, int c, int hw, float grad_scale, float* mse, float* vb,
                           float* d_model_out, void* stream);

/* One ancestral sampling step, gaussian_diffusion.py:376-421 over :254-332 (LEARNED_RANGE variance, EPSILON mean):
 * sample = posterior_mean(pred_x0, x) + (t != 0) * exp(0.5 * log_var) * noise; pred_xstart may be NULL.  t indexes `tab`
 * (the respaced schedule); model_out [n][2c][hw] was evaluated by the caller at the mapped original timestep. */
int sfron_p_sample(const float* x, const float* model_out, const int64_t* t, const float* tab, const float* noise, int n, int c,
                   int hw, int clip_denoised, float* sample, float* pred_xstart, void* stream);
/* classifier-free guidance mix of DiT.forward_with_cfg (DiT/models.py:258-266), in place on model_out [n_total][cout][hw]:
 * for the first n_guided channels, rows i and i + n_total/2 both become uncond + cfg_scale * (cond - uncond). */
int sfron_cfg_combine(float* model_out, int n_total, int cout, int hw, int n_guided, float cfg_scale, void* stream);

/* ---- DDPM (CIFAR-10) epsilon loss: DDPM/functions/losses.py:22-38 (sum over C,H,W, mean over the batch), :49-69 (adaptive
 * "adaga" weights), :32 (alphas_cumprod recomputed from fp32 betas). */
/* abar[t] = prod_{s<=t} (1 - betas[s]), running product in double, rounded to fp32 per entry (= torch CPU cumprod) */
int sfron_ddpm_alphas_cumprod(const float* betas, int T, float* abar, void* stream);
/* x_t = x0 * sqrt(abar[t]) + e * sqrt(1 - abar[t])   (correctly rounded sqrt; losses.py:33-34) */
int sfron_ddpm_q_sample(const float* x0, const float* e, const int64_t* t, const float* abar, int n, int chw, float* x_t,
                        void* stream);
/* per_sample[i] = sum_{chw} (e - model_out)^2         (losses.py:36-38 with keepdim=True) */
int sfron_ddpm_sample_loss(const float* e, const float* model_out, int n, int chw, float* per_sample, void* stream);
/* mode 0 "simple": loss = sum_local(per)/n_global, coef_i = 2*scale/n_global.
 * mode 1 "adaga":  w_i = 1/(per_i^lambd + 1e-8); W = sum_i w_i, written to *wsum (use_wsum = 0) or taken from *wsum
 *                  (use_wsum = 1: the caller all-reduced it over the data-parallel ranks); loss = sum_local(w_i per_i)/W,
 *                  coef_i = 2*scale*w_i/W.     d(scale*loss)/d model_out_i = coef_i * (model_out_i - e_i) */
int sfron_ddpm_loss_coef(const float* per_sample, int n, int mode, float lambd, float scale, int n_global, float* wsum,
                         int use_wsum, float* coef, float* loss, void* stream);
int sfron_ddpm_loss_bwd(const float* e, const float* model_out, const float* coef, int n, int chw, float* d_model_out,
                        void* stream);
/* one step of DDPM/functions/denoising.py:72-95 (generalized / DDIM update, same timestep for the whole batch):
 * x0_pred = (x - eps*s1)/s2, x_next = s3*x0_pred + c1*noise + c2*eps; noise may be NULL when c1 == 0, x0_pred may be NULL */
int sfron_ddim_step(const float* x, const float* eps, const float* noise, int64_t n, float s1, float s2, float s3, float c1,
                    float c2, float* x_next, float* x0_pred, void* stream);
/* classifier-free guidance + one DDIM update of SD/ldm/models/diffusion/ddim.py:326-372 in one pass, fp32, in the reference's order:
 * e = eps_uncond + guidance*(eps_cond - eps_uncond) (eps_cond NULL: e = eps_uncond); pred_x0 = (x - sqrt_one_minus_at*e)/sqrt_at;
 * x_prev = (sqrt_a_prev*pred_x0 + dir_coef*e) + sigma*noise.  noise may be NULL when sigma == 0, pred_x0 may be NULL, x_prev may be x. */
int sfron_ddim_cfg_step(const float* x, const float* eps_uncond, const float* eps_cond, const float* noise, int64_t n, float guidance,
                        float sqrt_one_minus_at, float sqrt_at, float sqrt_a_prev, float dir_coef, float sigma, float* x_prev, float* pred_x0,
                        void* stream);

/* ------------------------------------------------------------------ ldm PLMS sampler (plms.hip)
 * classifier-free guidance + the pseudo linear multistep combination + the eta = 0 update of SD/ldm/models/diffusion/plms.py:311-312,
 * 349-380 in one pass over n elements; fp32, every step one IEEE operation in the reference's left-to-right order:
 *   e  = eps_uncond + guidance*(eps_cond - eps_uncond)   (eps_cond NULL: e = eps_uncond);   e_out[i] = e when e_out is given
 *   e' = e | (3e - old1)/2 | (23e - 16 old1 + 5 old2)/12 | (55e - 59 old1 + 37 old2 - 9 old3)/24 | (old1 + e)/2   by `order`
 *        (true divisions; MEAN is the second half of the first step: old1 = that step's e_t, e = e_t_next)
 *   pred_x0 = (x - sqrt_one_minus_at*e')/sqrt_at;   x_prev = sqrt_a_prev*pred_x0 + dir_coef*e'
 * pred_x0 and e_out may be NULL.  x_prev may be x, and e_out may be the oldest history buffer the call reads (a three-slot ring is
 * overwritten in place): an element is read before it is written, by the same thread.  SFRON_ERR_ARG before any launch for a NULL x,
 * eps_uncond or x_prev, n <= 0, sqrt_at == 0, an unknown order, a NULL history pointer the order reads, a guidance that is not finite. */
enum { SFRON_PLMS_ORDER1 = 0, SFRON_PLMS_ORDER2 = 1, SFRON_PLMS_ORDER3 = 2, SFRON_PLMS_ORDER4 = 3, SFRON_PLMS_MEAN = 4 };
int sfron_plms_cfg_step(const float* x, const float* eps_uncond, const float* eps_cond, const float* old1, const float* old2,
                        const float* old3, int order, int64_t n, float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_a_prev,
                        float dir_coef, float* e_out, float* x_prev, float* pred_x0, void* stream);
/* the inpainting blend of plms.py:228-233 in one launch: orig = sqrt_ac*x0 + sqrt_one_minus_ac*noise (q_sample at the step's timestep);
 * out = orig*m + (1 - m)*img.  img, x0, noise, out fp32 [B][C][hw]; m from a mask [mask_b][mask_c][hw] with mask_b 1 or B and mask_c 1
 * or C (the broadcasts of a [B,1,H,W] or [1,1,H,W] mask).  out may be img.  Any other extent, a NULL pointer or a size <= 0:
 * SFRON_ERR_ARG. */
int sfron_inpaint_blend(const float* img, const float* x0, const float* noise, const float* mask, int B, int C, int64_t hw, int mask_b,
                        int mask_c, float sqrt_ac, float sqrt_one_minus_ac, float* out, void* stream);

/* ------------------------------------------------------------------ bf16 MFMA GEMM (gemm.hip)
 * C[M,N] = alpha * op(A)[M,K] · op(B)[K,N] (+ bias[N]) with a fused epilogue; fp32 accumulation.
 *   a_transposed = 0: A is [M][K] row-major (lda), contraction contiguous      (activations, forward / dgrad)
 *   a_transposed = 1: A is [K][M] row-major (lda), i.e. the operand is A^T of a row-major tensor (wgrad)
 *   b_transposed = 0: B is [N][K] row-major (ldb): nn.Linear weight layout, Y = X W^T
 *   b_transposed = 1: B is [K][N] row-major (ldb): dgrad (dX = dY W) and wgrad (dW = dY^T X)
 * Replaces the GEMMs behind nn.Linear / Conv2d(k=s=p) fwd+bwd of DiT/models.py:108-121,138-142,169.
 * Requirements: K % 8 == 0, N % 4 == 0, lda/ldb % 8 == 0, 16-byte aligned A/B; transposed operands need
 * their non-contraction extent % 8 == 0.  Rows/cols beyond M/N and k >= K are handled (zero-filled / masked). */
enum {
  SFRON_EPI_BF16 = 0,     /* c_bf16 = result                                                               */
  SFRON_EPI_F32 = 1,      /* c_f32 = result (+= if accumulate)                  -- wgrad into the grad arena */
  SFRON_EPI_GELU = 2,     /* aux = bf16(result) (pre-activation), c_bf16 = gelu_tanh(result)   -- Mlp.fc1+act */
  SFRON_EPI_GATE_RES = 3, /* aux = bf16(result); c_f32[row,col] = resid[row,col] + gate[row/tokens, col] * result
                             -- x = x + gate * branch(x)  (DiT/models.py:120-121)                          */
  SFRON_EPI_DGELU = 4,    /* c_bf16 = result * gelu_tanh'(aux)                           -- fc2 dgrad + act' */
  SFRON_EPI_POS = 5,      /* c_f32 = result + pos[row % tokens, col]    -- x_embedder(x) + pos_embed (:240) */
  /* Round 6: the GELU pair with `aux` = gelu_tanh'(result) as ONE BYTE per element instead of the bf16 pre-activation: `aux` then points to a
   * uint8 [M][ldaux] array, code = round((g' + 0.15) * 196), g' = code / 196 - 0.15 (GELU'_tanh lies in [-0.129, 1.129]; step 0.0051, i.e.
   * <= 0.0026 absolute -- the size of what the bf16 rounding of the pre-activation does to GELU').  fc1 writes 113 instead of 151 MB per
   * block at DiT-XL/2, the fc2 dgrad reads half as much and evaluates no exp.  Only where sfron_gemm_gelu_q_supported(M, N, K) (the 256 x 192
   * pipelined tile: M % 256 == 0, N % 192 == 0, K % 128 == 0, ldc_bf16 % 8 == 0, ldaux % 8 == 0), otherwise SFRON_ERR_UNSUPPORTED; a forward
   * pass that wrote codes must be followed by the _Q dgrad (the two arrays are not interchangeable). */
  SFRON_EPI_GELU_Q = 7,   /* aux(u8) = code(gelu_tanh'(result)), c_bf16 = gelu_tanh(result)          -- Mlp.fc1+act */
  SFRON_EPI_DGELU_Q = 8,  /* c_bf16 = result * decode(aux(u8))                                 -- fc2 dgrad + act' */
  SFRON_EPI_QUICK_GELU = 9 /* c_bf16 = r * sigmoid(1.702 r), r = result + bias; no aux (forward only) -- CLIP text encoder fc1 + quick_gelu.
                              Forward layout only (a_transposed = b_transposed = 0), no split, no accumulate; any M: the 128 x 128 tile where
                              M % 128 == N % 128 == K % 64 == 0, the generic kernel otherwise */
};
typedef struct sfron_gemm_desc {
  const uint16_t* A; const uint16_t* B;
  int M, N, K, lda, ldb;
  int a_transposed, b_transposed;
  int epilogue;
  float alpha;
  const float* bias;                 /* [N] fp32 or NULL */
  uint16_t* c_bf16; int ldc_bf16;
  float* c_f32; int ldc_f32;
  uint16_t* aux; int ldaux;
  const float* gate; int ldgate;
  const float* pos;
  int tokens;                        /* tokens per sample (row -> sample / position) */
  int accumulate;
  const float* resid;                /* EPI_GATE_RES: c_f32 = resid + gate * result; NULL = in place (resid = c_f32) */
  int split_k;                       /* > 1 (EPI_F32 only, no bias): split s writes its partial product to
                                        c_f32 + s * split_stride; sum the slabs with sfron_reduce_chunks */
  long split_stride;
  int tile_hint;                     /* 0 = auto; -1 = generic kernel; fast tiles 1 = 128x128, 2 = 256x192, 3 = 256x256, 4 = 384x192; further
                                        tuning values in csrc/gemm.hip pick_fast_tile (tests/test_gemm_paths_cpu.py lists them).  Every accepted
                                        value gives the same product: a tile that does not fit the shape, and any unknown value, runs the
                                        generic kernel.  21 / 22 (timing ablations that skip work) exist in the SFRON_DEBUG_KNOBS build only. */
  float* a_rowsum;                   /* weight-gradient layout only (a_transposed = b_transposed = 1, EPI_F32, no split): fp32 [M],
                                        a_rowsum[m] = sum_k op(A)[m][k] -- the bias gradient sum_rows dY of the same nn.Linear
                                        (DiT/models.py:108-121 backward), taken from the dY tiles the GEMM already holds in LDS
                                        (extra MFMAs against a ones fragment, shared by the workgroups of a tile row).  Only shapes
                                        sfron_gemm_rowsum_supported accepts. */
  float* rowsum_ws;                  /* with a_rowsum: fp32 scratch [(N / 192) * M] for the per-tile-column partial sums, added in a
                                        fixed order by a small reduction launch on the same stream */
  float* col_partials;               /* SFRON_EPI_DGELU only: fp32 [sfron_gemm_dgelu_colpart_rows(M, N, K)][N]; row r = the column
                                        sums of output rows 256 r .. 256 r + 255 (fp32, before the bf16 rounding): partials of the fc1
                                        bias gradient sum_rows d_hpre, formed where d_hpre is produced instead of by a second pass
                                        over it (sum them with sfron_reduce_chunks).  NULL = not wanted. */
  const uint8_t* sumsq_mask;         /* with sumsq_partials: byte mask over the OUTPUT (same layout as c_f32: element (m, n) at m * ldc_f32 + n) or NULL */
  double* sumsq_partials;            /* weight-gradient layout only (a_transposed = b_transposed = 1, EPI_F32, no split, no a_rowsum): fp64
                                        [sfron_gemm_sumsq_partials(M, N, K)], partial t = sum over output tile t of (mask ? c : 0)^2 -- the masked
                                        sum of squares clip_grad_norm_ needs (DiT/forget.py:289-298), formed where the gradient is produced
                                        instead of by a pass over the gradient arena; combine with sfron_clip_coef.  NULL = not wanted. */
} sfron_gemm_desc;
int sfron_gemm_bf16(const sfron_gemm_desc* desc /* HOST pointer */, void* stream);
/* number of partial rows an EPI_DGELU product of this shape writes to col_partials (M / 256), 0 = shape unsupported: use sfron_colsum */
int sfron_gemm_dgelu_colpart_rows(int M, int N, int K);
/* 1 when a weight-gradient GEMM dW[M][N] = dY[K][M]^T X[K][N] of this shape can also produce a_rowsum (else use sfron_colsum) */
int sfron_gemm_gelu_q_supported(int M, int N, int K);     /* 1 = SFRON_EPI_GELU_Q / _DGELU_Q take this (rows, hidden, contraction) shape */
int sfron_gemm_rowsum_supported(int M, int N, int K);
/* Finish of a split-K product (sfron_gemm_desc.split_k > 1 leaves n_splits fp32 slabs, split_stride elements apart): the slabs summed in index
 * order (bitwise reproducible) and written (a) as bf16 [n] -- an input gradient that the next product reads as its operand (autograd of the
 * nn.Linear layers, DiT/models.py:108-121) -- or (b) through the gated-residual epilogue of the forward proj / fc2 products (models.py:120-121):
 * v = sum + bias; branch (bf16 [M][N]) = v; out (fp32 [M][N]) = resid + gate[(row / tokens) * ldgate + col] * v.  n_splits <= 8.  What the
 * few-tile products of a small batch * tokens (BASELINE config 2: DiT-B/4, 2048 token rows) use to fill the chip (csrc/dit_engine.hip). */
int sfron_split_sum_bf16(const float* slabs, int n_splits, int64_t n, int64_t split_stride, uint16_t* out, void* stream);
int sfron_split_gate_res(const float* slabs, int n_splits, int64_t split_stride, const float* bias, const float* gate, int ldgate, int tokens,
                         const float* resid, float* out, uint16_t* branch, int M, int N, void* stream);

/* number of fp64 partials a weight-gradient GEMM dW[M][N] = dY[K][M]^T X[K][N] of this shape writes to sumsq_partials, 0 = shape unsupported */
int sfron_gemm_sumsq_partials(int M, int N, int K);


/* ------------------------------------------------------------------ fp8 (e4m3) forward GEMMs (fp8.hip) -- BASELINE config 5
 * "DiT-XL/2 fp8 weights + bf16 activations on the CDNA4 fp8 MFMA": the four token GEMMs of a DiT block forward
 * (DiT/models.py:108-121) on v_mfma_scale_f32_16x16x128_f8f6f4.  The reference has no fp8 path; tolerance is stated against the bf16
 * path (config 3) in tests/test_gpu_fp8.py.  e4m3 = OCP e4m3fn, round to nearest even, saturating at +-448.
 * Weights: fp32 masters + e4m3 shadow arena (same offsets, 1 byte / element) + ONE power-of-two scale per tensor;
 * activations: quantised by their producers with static power-of-two scales. */

/* table [n_tensors][2] int64 (DEVICE): element offset and length (multiples of 8) of each quantised tensor inside the arena.
 * mode 0: amax_bits[t] = max(amax_bits[t], bits(max |p|)) only.  mode 1: dst[off + i] = e4m3(p[off + i] * scales[t]) and the same amax
 * (delayed scaling: quantise with the scale derived from the PREVIOUS pass's amax while collecting the next one). */
int sfron_fp8_quant_tensors(const float* params, const int64_t* table, int n_tensors, const float* scales, uint32_t* amax_bits,
                            uint8_t* dst, int mode, void* stream);
/* scales[t] = 2^floor(log2(224 / amax_t)) (2x headroom under 448; 1 for an all-zero tensor); clears amax_bits */
int sfron_fp8_update_scales(uint32_t* amax_bits, int n_tensors, float* scales, void* stream);
/* How much of the e4m3 range the ACTIVATIONS of config 5 used since the last reset: out3[site] (HOST out) = max |x * scale| over every value
 * quantised at site 0 = sfron_ln_modulate_fwd_q's output, 1 = sfron_cast_e4m3, 2 = the e4m3 GELU output of sfron_fp8_gemm (c_e4m3).  The
 * conversion saturates at 448: a value above it means values WERE clipped (the reference has no fp8 path: nothing there to mirror).  The
 * three words are the CALLER's (round 6): a zero-initialised DEVICE uint32 [3] handed as `act_amax` to every quantising entry point
 * (sfron_ln_modulate_fwd_q, sfron_cast_e4m3, sfron_fp8_gemm_desc.act_amax, sfron_dit_fp8_operands.act_amax; NULL there = no tracking); this call
 * copies them to the host (synchronises `stream`) and, with reset != 0, clears them. */
int sfron_fp8_activation_amax(uint32_t* act_amax, float* out3 /* HOST out, 3 floats */, int reset, void* stream);

/* dst[i] = e4m3(src[i] * scale); src bf16 (src_is_bf16 = 1) or fp32; n % 8 == 0 */
int sfron_cast_e4m3(const void* src, int src_is_bf16, int64_t n, float scale, uint8_t* dst, uint32_t* act_amax /* DEVICE [3] or NULL */,
                    void* stream);
/* sfron_ln_modulate_fwd that also writes out_e4m3 = e4m3(value * e4m3_scale) from the fp32 value (the A operand of the next GEMM) */
int sfron_ln_modulate_fwd_q(const float* x, const float* shift, const float* scale, int ldmod, int tokens, int M, int D, uint16_t* out,
                            uint8_t* out_e4m3, float e4m3_scale, float* mean, float* rstd, uint32_t* act_amax /* DEVICE [3] or NULL */,
                            void* stream);

/* C[M][N] = (A8[M][K] . B8[N][K]^T) / (a_scale * *w_scale) + bias with one of the block's epilogues:
 *   SFRON_EPI_BF16      c_bf16 = result                                                   (qkv)
 *   SFRON_EPI_GELU      aux = result (pre-activation, bf16), c_bf16 = gelu_tanh(result),
 *                       c_e4m3 = e4m3(gelu_tanh(result) * c_e4m3_scale) [M][N]            (fc1: h for the backward pass AND for fc2)
 *   SFRON_EPI_GATE_RES  aux = result (bf16), c_f32 = resid + gate[row / tokens] * result  (proj, fc2)
 * Shapes: M % 256 == 0, N % 128 == 0 or N % 144 == 0 (256 x 128 / 256 x 144 tiles, the one that fills the CUs better), K % 128 == 0
 * (sfron_fp8_gemm_supported). */
typedef struct sfron_fp8_gemm_desc {
  const uint8_t* A; const uint8_t* B;
  int M, N, K;
  const float* w_scale;              /* DEVICE scalar: the scale B was quantised with (sfron_fp8_update_scales output) */
  float a_scale;                     /* the scale A was quantised with */
  int epilogue;
  const float* bias;
  uint16_t* c_bf16; int ldc_bf16;
  uint16_t* aux; int ldaux;
  uint8_t* c_e4m3; float c_e4m3_scale;
  float* c_f32; int ldc_f32;
  const float* resid;                /* NULL = in place */
  const float* gate; int ldgate;
  int tokens;
  uint32_t* act_amax;                /* DEVICE uint32 [3] or NULL: the caller's activation-range words (sfron_fp8_activation_amax); the e4m3
                                        GELU output (c_e4m3) raises word 2 */
  int aux_q;                         /* SFRON_EPI_GELU only, 1 = `aux` receives gelu_tanh'(result) as one byte per element (uint8 [M][ldaux],
                                        the code of SFRON_EPI_GELU_Q) instead of the bf16 pre-activation: for a backward pass on
                                        SFRON_EPI_DGELU_Q */
} sfron_fp8_gemm_desc;
int sfron_fp8_gemm_supported(int M, int N, int K);
int sfron_fp8_gemm(const sfron_fp8_gemm_desc* desc /* HOST pointer */, void* stream);

/* fp8 BACKWARD (opt-in, sfron_aux_set_fp8_dgrad): the four input-gradient products dX[M][in] = dY[M][out] . W[out][in] of a DiT block on
 * the same scaled MFMA.  dY is MX-scaled: one E8M0 scale byte per 32 consecutive elements of a row, [M][N / 32] beside the e4m3 [M][N]:
 *   X    = ceil(log2(amax / 448)) over the 32 values (amax of their magnitudes), clamped to [-127, 127]; an all-zero block gets X = -127
 *   byte = X + 127
 *   code = e4m3fn_RNE(x * 2^-X)            (|x * 2^-X| <= 448: nothing saturates; x * 2^-X is exact in fp32)
 * (for finite input; an infinite amax gets X = 127, and blocks holding a NaN are outside the rule)
 * No global amax, no delayed-scaling state: every scale is local to its 32 values.  W is read as its TRANSPOSED e4m3 shadow [in][out] (the
 * same codes and per-tensor scale as the forward shadow; sfron_fp8_transpose_shadow), one scale of 1 per block, its tensor scale undone in
 * the epilogue. */
/* bf16 src [M][N] -> MX e4m3 dst [M][N] + scales [M][N / 32] by the rule above; N % 32 == 0 */
int sfron_cast_mx8(const uint16_t* src, int M, int N, uint8_t* dst, uint8_t* scales, void* stream);
/* e4m3 weight shadow -> transposed copy, one launch for n_matrices matrices: table = DEVICE int64 [n_matrices][4] rows (src_off, dst_off,
 * R, C), w8t[dst_off + c * R + r] = w8[src_off + r * C + c].  Offsets, R and C multiples of 8 (a row that is not is skipped). */
int sfron_fp8_transpose_shadow(const uint8_t* w8, uint8_t* w8t, const int64_t* table, int n_matrices, void* stream);
/* C[M][N] = (A[M][K] with its MX scales) . B[N][K]^T / *w_scale, B = the transposed shadow of W, with
 *   SFRON_EPI_BF16      c_bf16 = result                                                        (qkv, proj, fc1 dgrads)
 *   SFRON_EPI_DGELU     r = result * gelu_tanh'(aux: bf16 pre-activation [M][ldaux])           (fc2 dgrad)
 *   SFRON_EPI_DGELU_Q   r = result * decode(aux: uint8 GELU' codes [M][ldaux], SFRON_EPI_GELU_Q)
 *                       for both: c_bf16 = bf16(r); c_e4m3 [M][N] + c_scales [M][N / 32] = the MX form of the bf16-ROUNDED c_bf16 (equal to
 *                       sfron_cast_mx8(c_bf16) bit for bit); col_partials (or NULL) fp32 [M / 256][N]: row t = column sums of r over
 *                       output rows 256 t .. 256 t + 255 (sum them with sfron_reduce_chunks)
 * Shapes as sfron_fp8_gemm_supported; the DGELU forms need N % 128 == 0.  tile_hint: 0 = auto, 8 = 256 x 128, 9 = 256 x 144 tiles. */
typedef struct sfron_fp8_dgrad_desc {
  const uint8_t* A;                  /* MX e4m3 dY [M][K] */
  const uint8_t* a_scales;           /* its E8M0 bytes [M][K / 32] */
  const uint8_t* B;                  /* transposed e4m3 weight [N][K] */
  int M, N, K;
  const float* w_scale;              /* DEVICE scalar: the scale W was quantised with */
  int epilogue;
  uint16_t* c_bf16; int ldc_bf16;
  const uint16_t* aux; int ldaux;
  uint8_t* c_e4m3;
  uint8_t* c_scales;
  float* col_partials;
  int tile_hint;
} sfron_fp8_dgrad_desc;
int sfron_fp8_dgrad(const sfron_fp8_dgrad_desc* desc /* HOST pointer */, void* stream);

/* fp8 WEIGHT GRADIENTS (opt-in, sfron_aux_set_fp8_wgrad): dW[N][K] = dY[M][N]^T . X[M][K] reduces over the M tokens, so BOTH operands are
 * MX-scaled along the tokens -- the rule above applied to the transposed matrices: one E8M0 byte per 32 consecutive tokens of a column.
 * bf16 src [M][W] -> MX e4m3 of src^T: dst [W][M] + scales [W][M / 32]; sfron_cast_mx8_t(x) == sfron_cast_mx8(x^T) bit for bit.
 * M % 32 == 0, W % 8 == 0. */
int sfron_cast_mx8_t(const uint16_t* src, int M, int W, uint8_t* dst, uint8_t* scales, void* stream);
/* c_f32[N][K] (row stride ldc, fp32, overwritten) = (A[N][M] with its MX scales) . (B[K][M] with its MX scales)^T: A = sfron_cast_mx8_t(dY),
 * B = sfron_cast_mx8_t(X); each operand's scale bytes go to the MFMA per lane.  192 x 192 output tiles (those of the bf16 weight-gradient
 * GEMM): sumsq_partials / sumsq_mask as in sfron_gemm_desc -- fp64 [sfron_gemm_sumsq_partials(N, K, M)], partial t = sum over output tile t
 * of (mask ? c : 0)^2, mask over the output (element (n, k) at n * ldc + k) or NULL.  sfron_fp8_wgrad_supported: N % 192 == K % 192 == 0,
 * M % 128 == 0, N * M and K * M < 2^31. */
typedef struct sfron_fp8_wgrad_desc {
  const uint8_t* A;                  /* MX e4m3 dY^T [N][M] */
  const uint8_t* a_scales;           /* its E8M0 bytes [N][M / 32] */
  const uint8_t* B;                  /* MX e4m3 X^T [K][M] */
  const uint8_t* b_scales;           /* its E8M0 bytes [K][M / 32] */
  int N, K, M;
  float* c_f32; int ldc;
  const uint8_t* sumsq_mask;
  double* sumsq_partials;
} sfron_fp8_wgrad_desc;
int sfron_fp8_wgrad_supported(int N, int K, int M);
int sfron_fp8_wgrad(const sfron_fp8_wgrad_desc* desc /* HOST pointer */, void* stream);

/* ------------------------------------------------------------------ convolutional U-Net blocks (conv.hip, groupnorm.hip, rows.hip)
 * Replaces the Conv2d / GroupNorm / bmm-softmax sequences of DDPM/models/diffusion.py:43-192,283-413 (Conditional_Model) forward
 * and backward.  Activations are NHWC: a [batch * H * W][C] row-major matrix (bf16 where they feed a GEMM, fp32 elsewhere). */

/* batched GEMM on the generic 128x128 tile: C[z] = alpha * op(A[z]) op(B[z]) (+ bias) (+ resid) (+ per-sample row vector),
 * z < batch, operands advanced by the element strides; layouts as sfron_gemm_desc.  Exactly one of c_bf16 / c_f32 is set.
 * a_transposed = 1 needs b_transposed = 1: A^T against a B that is not transposed is refused with SFRON_ERR_ARG, like every
 * other rule on the arguments (N % 4, lda / ldb / strides % 8, 16-byte aligned operands, each matrix below 2 GiB). */
typedef struct sfron_bgemm_desc {
  const uint16_t* A; const uint16_t* B;
  int M, N, K, lda, ldb;
  int a_transposed, b_transposed;
  int batch;
  long stride_a, stride_b, stride_c;
  int batch2;                      /* inner batch (0 / 1 = none): attention heads that are column slices of one matrix */
  long stride_a2, stride_b2, stride_c2;
  float alpha;
  const float* bias;               /* [N] or NULL */
  uint16_t* c_bf16; float* c_f32; int ldc;
  const float* resid;              /* fp32 [M][ldc] added to the result (c_f32 only), or NULL */
  const float* sample_vec;         /* fp32 vec[(row / rows_per_sample) * ld_vec + col] added (c_f32 only), or NULL */
  int ld_vec, rows_per_sample;
  int accumulate;                  /* c_f32 += result */
  float* split_ws; int split_ws_slabs;   /* optional: fp32 scratch [split_ws_slabs][M * N] -- a plain weight gradient (both operands
                                      transposed, batch 1, ldc == N, no epilogue extras) then splits its contraction over the
                                      chip and adds the slabs in a fixed order */
} sfron_bgemm_desc;
int sfron_bgemm_bf16(const sfron_bgemm_desc* desc /* HOST pointer */, void* stream);

/* implicit-GEMM convolution.  The GEMM rows are the pixels of an (h_out x w_out) grid per sample; row p = (b, ho, wo) reads, for
 * tap (kh, kw), the source pixel (ho * stride + kh - pad, wo * stride + kw - pad) of a [batch][h_src][w_src][c_src] bf16 image:
 *   upsample = 1: through a nearest x2 upsampling (F.interpolate(scale_factor=2) + conv, models/diffusion.py:56-60)
 *   dilate   = 1: as a zero-dilated x2 image (the input gradient of a stride-2 convolution)
 * and zero outside it (padding; the (0,1,0,1) pad of Downsample, :76-80, is the bottom / right edge of a pad-0 stride-2 conv). */
typedef struct sfron_conv_desc {
  int batch, h_src, w_src, c_src;   /* c_src % 8 == 0 */
  int h_out, w_out;
  int n_out;                        /* GEMM N: output channels (forward) / input channels (input gradient) */
  int taps, stride, pad, upsample, dilate;
  const float* bias;                /* [n_out] or NULL */
  const float* resid;               /* fp32 [rows][ld_out] added (out_f32 only) or NULL */
  const float* sample_vec;          /* fp32 [batch][ld_vec] added per sample (out_f32 only) or NULL */
  int ld_vec;
  uint16_t* out_bf16; float* out_f32; int ld_out;
  int accumulate;
  float* split_ws; int split_ws_slabs;   /* optional fp32 scratch [split_ws_slabs][rows * n_out]: a forward / input-gradient conv with few
                                       output tiles and a deep contraction then splits the contraction over the chip */
  int* split_pending;               /* optional HOST int (ABI 16): when the call splits its contraction (and ld_out == n_out) it leaves
                                       *split_pending (> 0) slabs [rows * n_out] in split_ws and does NOT launch the pass that adds them and
                                       applies bias / sample_vec / resid -- the caller hands them to a GroupNorm that finishes the sum itself
                                       (sfron_split_src, sfron_groupnorm_*_src) or to sfron_split_finish; 0 = the output is complete.
                                       NULL = always complete.  Needs out_f32: with out_bf16 set the call is refused (SFRON_ERR_ARG)
                                       before any launch, *split_pending = 0 and neither the output nor split_ws is written. */
} sfron_conv_desc;
/* out[p][n] = sum_{tap, c} src[src(p, tap)][c] * w[n][tap][c]; w bf16 [n_out][taps][c_src] (sfron_conv_wprep's "fwd" layout;
 * the input gradient calls this on dY with the "dgrad" layout) */
int sfron_conv_fwd(const sfron_conv_desc* desc, const uint16_t* src, const uint16_t* w, void* stream);
/* dw_gemm fp32 [splits][n_out][taps * c_src]: slab s = sum over the s-th range of pixels p of dy[p][n] * src[src(p, tap)][c]
 * (dy bf16 [rows][ld_dy]); splits = sfron_conv_wgrad_splits(desc) >= 1 = the number of slabs WRITTEN (the contraction over all pixels is split
 * over the chip; size dw_gemm for it and pass it to sfron_conv_wgrad_scatter) */
int sfron_conv_wgrad_splits(const sfron_conv_desc* desc);
int sfron_conv_wgrad(const sfron_conv_desc* desc, const uint16_t* dy, int ld_dy, const uint16_t* src, float* dw_gemm, void* stream);
/* fp32 OIHW master weights -> bf16 operands: w_fwd [c_out_p][taps][c_in_p] (zero padded), w_dgrad [c_in][taps flipped][c_out_p] or NULL */
int sfron_conv_wprep(const float* w_oihw, int c_out, int c_in, int taps, int c_out_p, int c_in_p, uint16_t* w_fwd, uint16_t* w_dgrad,
                     void* stream);
/* the same for every 3x3 kernel of a model in one launch: a device-resident table, item i owning the tile ids
 * [tile0, tile0 + sfron_conv_wprep_tiles(c_out_p, c_in_p)) of the grid (tile0 ascending, n_tiles = their total) */
typedef struct sfron_wprep_item {
  const float* w;         /* OIHW fp32 master [c_out][c_in][3][3] */
  uint16_t* fwd;          /* bf16 [c_out_p][9][c_in_p] */
  uint16_t* dgr;          /* bf16 [c_in][9 flipped][c_out_p], or NULL */
  int32_t co, ci, co_p, ci_p, tile0, pad_;
} sfron_wprep_item;
int sfron_conv_wprep_tiles(int c_out_p, int c_in_p);
int sfron_conv_wprep_batch(const sfron_wprep_item* items_dev, int n_items, int n_tiles, void* stream);
/* dw_gemm [n_slabs][c_out_p..][taps][c_in_p] -> OIHW gradient [c_out][c_in][taps] (overwrite; the slabs are added in order) */
int sfron_conv_wgrad_scatter(const float* dw_gemm, int c_out, int c_in, int taps, int c_in_p, int n_slabs, int64_t slab_stride,
                             float* dw_oihw, void* stream);
/* The scatters of MANY kernel gradients in ONE launch (round 6): item i is sfron_conv_wgrad_scatter(dw_gemm, c_out, c_in, taps, c_in_p, n_slabs,
 * slab_stride, dw_oihw), bit for bit.  `items` is a HOST array (the items travel by value in the kernel arguments, 80 per launch; capturable).
 * A U-Net backward pass keeps each layer's slabs in a buffer of the layer's own and issues the scatters once, behind its last product. */
typedef struct sfron_wgrad_scatter_item {
  const float* dw_gemm; float* dw_oihw; int64_t slab_stride; int c_out, c_in, taps, c_in_p, n_slabs, reserved;
} sfron_wgrad_scatter_item;
int sfron_conv_wgrad_scatter_batch(const sfron_wgrad_scatter_item* items /* HOST */, int n_items, void* stream);

int sfron_nchw_to_rows_bf16(const float* x, int B, int C, int HW, int c_pad, uint16_t* rows, void* stream);
int sfron_nchw_to_rows_f32(const float* x, int B, int C, int HW, int ld, float* rows, void* stream);
/* uint8 HWC images [B][H][W][3] -> bf16 rows [B*H*W][c_pad] (c_pad % 8 == 0, channels 3.. zero): ToTensor + Normalize(0.5, 0.5), i.e.
 * bf16_rne((x / 255.0f - 0.5f) / 0.5f) with true fp32 divisions (DiT/forget.py:200-205); flip (uint8 [B] or NULL): flip[b] != 0 reads
 * column W-1-w of sample b (RandomHorizontalFlip).  rows 16-byte aligned. */
int sfron_image_u8_to_rows_bf16(const uint8_t* img, int B, int H, int W, const uint8_t* flip, int c_pad, uint16_t* rows, void* stream);
int sfron_rows_to_nchw(const float* rows, int ld, int B, int C, int HW, float* x, void* stream);
/* VAE decoder tail: fp32 rows [B*H*W][ld] (ld >= 3; channels 0..2 read) -> uint8 RGB, every step a separately rounded fp32 operation.
 *   SFRON_IMAGE_SAVE_IMAGE (torchvision make_grid(normalize=True, value_range=(lo, hi)) + save_image; hi > lo):
 *     v = (clamp(x, lo, hi) - lo) / (hi - lo);  u = trunc(clamp(v * 255 + 0.5, 0, 255))   (v * 255 and + 0.5 rounded in that order)
 *   SFRON_IMAGE_ROUND (diffusers / SD generate-images.py; lo, hi unused):  v = clamp(x / 2 + 0.5, 0, 1);  u = rint_half_even(v * 255)
 * The rows hold samples b0 .. b0+B-1 of a batch of n (n >= b0 + B; a chunked decode launches once per chunk).
 *   nrow == 0: out = [n][H][W][3]; this launch writes its B samples.
 *   nrow > 0:  out = the make_grid canvas [Hc][Wc][3]: xmaps = min(nrow, n) columns, ceil(n / xmaps) rows, cells (H + padding) x
 *              (W + padding) behind a padding-pixel outer border, Hc = rows * (H + padding) + padding (Wc alike); pad pixels and empty
 *              cells are byte 0 and are written by the launch with b0 == 0.  n == 1 gives the bare H x W image.
 * Hc * Wc * 3 (or B * H * W * 3) < 2^31. */
enum { SFRON_IMAGE_SAVE_IMAGE = 0, SFRON_IMAGE_ROUND = 1 };
/*   SFRON_IMAGE_TRUNC (DiT/sample_ddp.py:132; lo, hi unused):  u = trunc(clamp(127.5f * x + 128.0f, 0, 255))   (product, then sum) */
enum { SFRON_IMAGE_TRUNC = 2 };
int sfron_rows_to_image_u8(const float* rows, int ld, int B, int H, int W, int mode, float lo, float hi, int nrow, int padding, int b0, int n,
                           uint8_t* out, void* stream);

/* y = bf16( act(GroupNorm(x; groups, eps) * gamma + beta) [* drop_mask * drop_scale] ), act = swish when `swish`; x fp32 rows
 * [B * HW][ldx]; mean / rstd [B][groups] saved for the backward pass (models/diffusion.py:43-46,126-131) */
int sfron_groupnorm_fwd(const float* x, int ldx, const float* gamma, const float* beta, int B, int HW, int C, int groups, float eps,
                        int swish, const uint8_t* drop_mask, float drop_scale, uint16_t* y, float* mean, float* rstd,
                        void* scratch /* sfron_groupnorm_scratch_bytes(), 16-B aligned; NULL = per-(sample, group) kernels */, void* stream);
/* dy fp32 [B * HW][C] = gradient wrt y; dx (+)= gradient wrt x; part_gamma / part_beta [B][C] per-sample partial sums.  x rows ldx >= C
 * and dx rows lddx >= C elements apart, in every backward entry point below (SFRON_ERR_ARG otherwise, before any launch) */
int sfron_groupnorm_bwd(const float* dy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                        const float* rstd, int B, int HW, int C, int groups, int swish, const uint8_t* drop_mask, float drop_scale,
                        float* dx, int lddx, int accumulate, float* part_gamma, float* part_beta, void* scratch, void* stream);
/* the same with one more term: dx (+)= extra + gradient wrt x, extra fp32 [B * HW][ld_extra] (the residual branch's share of x's
 * gradient -- ResnetBlock `x + h`, DDPM/models/diffusion.py:145 -- that a separate pass would add; same bits as
 * sfron_copy_cols(extra -> dx, accumulate) followed by sfron_groupnorm_bwd(accumulate = 1)).  extra == NULL: sfron_groupnorm_bwd. */
int sfron_groupnorm_bwd_res(const float* dy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                            const float* rstd, int B, int HW, int C, int groups, int swish, const uint8_t* drop_mask, float drop_scale,
                            float* dx, int lddx, int accumulate, const float* extra, int ld_extra, float* part_gamma, float* part_beta,
                            void* scratch, void* stream);
/* the backward pass for an x with ONE consumer whose gradient feeds a GEMM: dx leaves as the bf16 operand [B * HW][C] (no fp32 copy),
 * with its column sums per (sample, pixel chunk): col_partials fp32 [B][sfron_groupnorm_chunks(B, HW)][C] -- summed over everything
 * the bias gradient of the layer that produced x, summed per sample the gradient of a per-sample vector added to x (the
 * temb / class-embedding projection of ResnetBlock, DDPM/models/diffusion.py:120-124): sfron_reduce_chunks finishes both.  Replaces
 * sfron_groupnorm_bwd + sfron_cast_rows_colsum + sfron_sample_colsum over an fp32 dx.  Needs sfron_groupnorm_bwd_cast_ok(). */
int sfron_groupnorm_bwd_cast(const float* dy, const float* x, int ldx, const float* gamma, const float* beta, const float* mean,
                             const float* rstd, int B, int HW, int C, int groups, int swish, const uint8_t* drop_mask, float drop_scale,
                             uint16_t* dx_bf16, float* col_partials, float* part_gamma, float* part_beta, void* scratch, void* stream);

/* The GroupNorm INPUT as an unfinished split-K result (round 6, ABI 16): element (row, c) = sum_{s < n_slabs} slabs[s * slab_stride + row * C + c]
 * (in index order) + bias[c] + sample_vec[(row / (rows per sample)) * ld_vec + c] + resid[row * ld_resid + c] -- what the finish launch of a
 * split convolution (sfron_conv_desc.split_pending) would have written.  The one-launch GroupNorm (sfron_groupnorm_one_launch(B, HW, C, groups)
 * != 0: a workgroup per sample and block of whole groups) forms each element in its first pass and STORES it to the tensor the finish would have
 * filled (x of the forward pass / dy of the backward pass, row stride C: every later reader finds it there), so that launch no longer exists:
 * the same bits as sfron_split_finish followed by sfron_groupnorm_fwd / _bwd_res / _bwd_cast.  Returns SFRON_ERR_UNSUPPORTED (nothing launched)
 * when the shape does not take the one-launch form: the caller then calls sfron_split_finish and the plain entry point. */
typedef struct sfron_split_src {
  const float* slabs; int n_slabs; int64_t slab_stride;
  const float* bias; const float* sample_vec; int ld_vec; const float* resid; int ld_resid;    /* each optional */
} sfron_split_src;
int sfron_split_finish(const sfron_split_src* src /* HOST */, int64_t rows, int C, int rows_per_sample, float* out_f32, uint16_t* out_bf16,
                       int ld_out, void* stream);
int sfron_groupnorm_one_launch(int B, int HW, int C, int groups);
int sfron_groupnorm_fwd_src(const sfron_split_src* src /* HOST */, float* x /* [B * HW][C], written */, const float* gamma, const float* beta, int B,
                            int HW, int C, int groups, float eps, int swish, const uint8_t* drop_mask, float drop_scale, uint16_t* y, float* mean,
                            float* rstd, void* stream);
int sfron_groupnorm_bwd_res_src(const sfron_split_src* src /* HOST */, float* dy /* [B * HW][C], written */, const float* x, int ldx,
                                const float* gamma, const float* beta, const float* mean, const float* rstd, int B, int HW, int C, int groups,
                                int swish, const uint8_t* drop_mask, float drop_scale, float* dx, int lddx, int accumulate, const float* extra,
                                int ld_extra, float* part_gamma, float* part_beta, void* stream);
int sfron_groupnorm_bwd_cast_src(const sfron_split_src* src /* HOST */, float* dy /* [B * HW][C], written */, const float* x, int ldx,
                                 const float* gamma, const float* beta, const float* mean, const float* rstd, int B, int HW, int C, int groups,
                                 int swish, const uint8_t* drop_mask, float drop_scale, uint16_t* dx_bf16, float* col_partials,
                                 float* part_gamma, float* part_beta, void* stream);
int sfron_groupnorm_bwd_cast_ok(int ldx, int C, int groups);
int sfron_groupnorm_chunks(int B, int HW);
int64_t sfron_groupnorm_scratch_bytes(int B, int HW, int C, int groups);
/* p = bf16(softmax(scale * s)) over rows of length n; ds = bf16(scale * p * (dp - sum(p * dp)))   (AttnBlock, :168-186) */
int sfron_softmax_fwd(const float* s, int64_t rows, int n, int n_valid /* keys; columns beyond get probability 0 */, float scale, uint16_t* p,
                      void* stream);
/* y = bf16(LayerNorm(x; eps) * gamma + beta) on fp32 rows [rows][D]; backward: dx (+)=, per-block partial sums of d gamma / d beta
 * [ceil(rows / sfron_layernorm_rows_per_block(rows))][D] (BasicTransformerBlock.norm1..3, SD/ldm/modules/attention.py:223-225).
 * The backward entries take D <= 2048 (their per-wave column accumulators fill the 64 KiB of dynamic LDS a launch gets by default
 * there) and return SFRON_ERR_ARG above it, as they do for extra == dx, with nothing written. */
int sfron_layernorm_fwd(const float* x, const float* gamma, const float* beta, int64_t rows, int D, float eps, uint16_t* y, float* mean,
                        float* rstd, void* stream);
int sfron_layernorm_rows_per_block(int64_t rows);
int sfron_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, int64_t rows, int D, float* dx,
                        int accumulate, float* part_gamma, float* part_beta, void* stream);
/* the same with one more term of x's gradient, extra fp32 [rows][D] (the residual stream's share, x + attn(norm(x)),
 * SD/ldm/modules/attention.py:271-273): dx (+)= extra + gradient, the bits of a separate dx (+)= extra pass followed by sfron_layernorm_bwd */
int sfron_layernorm_bwd_res(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, int64_t rows, int D, float* dx,
                            int accumulate, const float* extra, float* part_gamma, float* part_beta, void* stream);
/* GEGLU (attention.py:37-45): h fp32 [rows][2F] = value || gate; out = bf16(value * gelu_erf(gate)); backward dh bf16 [rows][2F] */
int sfron_geglu_fwd(const float* h, int64_t rows, int F, uint16_t* out, void* stream);
int sfron_geglu_bwd(const float* d_out, const float* h, int64_t rows, int F, uint16_t* dh, void* stream);
int sfron_softmax_bwd(const uint16_t* p, const float* dp, int64_t rows, int n, float scale, uint16_t* ds, void* stream);
/* out[b][c] = sum over the HW rows of sample b of x[row][c] */
int sfron_sample_colsum(const float* x, int ld, int B, int HW, int C, float* out, int ld_out,
                        float* scratch /* optional row-chunk partials, >= B * 32 * C floats */, int64_t scratch_floats, void* stream);
/* out = alpha * a + beta * b (guidance mix (1 + s) * cond - s * null of _forward_with_cond_scale, :340-357) */
int sfron_axpby(const float* a, const float* b, float alpha, float beta, int64_t n, float* out, void* stream);
/* backward of nearest x2 upsampling: dx[b][h][w][c] (+)= sum of the 2x2 block of dy [B][2H][2W][C] */
int sfron_pool2_sum(const float* dy, int B, int H, int W, int C, float* dx, int accumulate, void* stream);
int sfron_cast_rows_bf16(const float* x, int ldx, int64_t rows, int C, uint16_t* y, void* stream);
/* y = bf16(x) and colsum[c] = sum over rows of x[.][c] in one pass (output gradient -> GEMM operand + bias gradient, `Conv2d` /
 * `Linear` backward); partials: scratch of max_partials * C floats */
int sfron_cast_rows_colsum(const float* x, int ldx, int64_t rows, int C, uint16_t* y, float* partials, int max_partials, float* colsum,
                           void* stream);
/* The first half of sfron_cast_rows_colsum alone (round 6): y and the column-sum partials [*chunks_out][C]; the caller finishes with
 * sfron_reduce_chunks(partials, 1, *chunks_out, C, colsum, C, 0) -- or collects that finish into a sfron_reduce_batch launch. */
int sfron_cast_rows_colsum_partials(const float* x, int ldx, int64_t rows, int C, uint16_t* y, float* partials, int max_partials,
                                    int* chunks_out /* HOST */, void* stream);
/* y[r][0..C) (+)= x[r][0..C): channel-slice copies of torch.cat(dim=1) and its backward (:404) */
/* keep mask of nn.Dropout(p) (DDPM/models/diffusion.py:131), 1 = kept with probability 1 - p: a counter-based draw keyed by
 * (seed, counter[0] on the device, salt, element); the caller advances the device counter once per pass */
int sfron_dropout_mask(uint64_t seed, const int64_t* counter, int64_t salt, int64_t n, float p, uint8_t* mask, void* stream);
/* The same masks for n_items (salt, n) pairs in one launch: items_dev = DEVICE int64 triples [salt, n, byte offset into mask_base]
 * (offsets multiples of 4), max_n = the largest n.  Bit for bit what n_items calls of sfron_dropout_mask write (the nn.Dropout of every
 * ResnetBlock of a pass, DDPM/models/diffusion.py:131). */
int sfron_dropout_mask_batch(uint64_t seed, const int64_t* counter, const int64_t* items_dev, int n_items, int64_t max_n, float p,
                             uint8_t* mask_base, void* stream);
int sfron_copy_cols(const float* x, int ldx, int64_t rows, int C, float* y, int ldy, int accumulate, void* stream);
/* Two such copies in one launch: y0[rows][ldy0] columns [0, C0) (+)= x0, y1 columns [0, C1) (+)= x1 -- the up path's torch.cat([h, skip], dim=1)
 * (DDPM/models/diffusion.py:403, openaimodel.py:791) with y0 / y1 the two column halves of the concatenated tensor, and its backward with x0 / x1
 * the halves of its gradient. */
int sfron_copy_cols2(const float* x0, int ldx0, int C0, float* y0, int ldy0, int accumulate0, const float* x1, int ldx1, int C1, float* y1,
                     int ldy1, int accumulate1, int64_t rows, void* stream);
/* get_timestep_embedding (:17-35): bf16 [n][dim] = sin(t f) || cos(t f), f_j = exp(-ln(1e4) j / (dim/2 - 1)); t float */
int sfron_ddpm_timestep_embed(const float* t, int n, int dim, uint16_t* out, void* stream);
/* out[b] = keep[b] ? table[c[b]] : null_emb (:370-376; keep NULL = all kept); backward accumulates into d_table (+=), writes d_null */
int sfron_class_embed_fwd(const float* table, const float* null_emb, const int64_t* c, const uint8_t* keep, int n_classes, int n, int D,
                          uint16_t* out, void* stream);
int sfron_class_embed_bwd(const float* d, const int64_t* c, const uint8_t* keep, int n_classes, int n, int D, float* d_table, float* d_null,
                          void* stream);

/* ------------------------------------------------------------------ adaLN-Zero elementwise (norm.hip)
 * mod buffers are fp32 [batch][ldmod]; shift/scale/gate pointers already include the column offset of the
 * chunk (DiT/models.py:119 .chunk(6, dim=1)).  `tokens` = tokens per sample (row / tokens = sample). */

/* rows per reduction chunk of the *_bwd kernels' partial buffers (one workgroup's rows: 16 when 16 | tokens) */
int sfron_rows_per_chunk(int tokens);

/* out = bf16( LayerNorm(x; eps 1e-6, no affine) * (1 + scale) + shift ), saves mean / rstd per row
 * (modulate(norm(x), shift, scale), DiT/models.py:19-20,120-121,139-140) */
int sfron_ln_modulate_fwd(const float* x, const float* shift, const float* scale, int ldmod, int tokens, int M, int D,
                          uint16_t* out, float* mean, float* rstd, void* stream);

/* backward of the above: dx (+)= dLN; p_shift/p_scale [M / rows_per_chunk][D] = per-chunk column sums of
 * d_out and d_out * xhat (finish with sfron_reduce_chunks -> d shift / d scale of the adaLN Linear) */
int sfron_ln_modulate_bwd(const uint16_t* d_out, const float* x, const float* mean, const float* rstd, const float* scale,
                          int ldmod, int tokens, int M, int D, float* dx, int dx_accumulate, float* p_shift,
                          float* p_scale, void* stream);

/* backward of x + gate * branch (DiT/models.py:120-121): d_branch = bf16(dy * gate);
 * p_gate / p_dy [M / rows_per_chunk][D] = per-chunk column sums of dy * branch and of dy */
int sfron_gate_bwd(const float* dy, const uint16_t* branch, const float* gate, int ldmod, int tokens, int M, int D,
                   uint16_t* d_branch, float* p_gate, float* p_dy, void* stream);

/* sfron_ln_modulate_bwd followed by sfron_gate_bwd of the NEXT (earlier) branch on the freshly accumulated dx rows, in
 * one pass (saves the fp32 re-read of dx): DiT/models.py:120-121 backward, branch k's LN + branch k-1's gate. */
int sfron_ln_gate_bwd(const uint16_t* d_out, const float* x, const float* mean, const float* rstd, const float* scale,
                      int ldmod, int tokens, int M, int D, float* dx, int dx_accumulate, float* p_shift, float* p_scale,
                      const uint16_t* branch, const float* gate, int ldgate, uint16_t* d_branch, float* p_gate, float* p_dy,
                      void* stream);

/* out[g * ldout + c] (+)= sum_{j < per_group} partials[(g * per_group + j) * D + c]   (fixed order, reproducible) */
int sfron_reduce_chunks(const float* partials, int groups, int per_group, int D, float* out, int ldout, int accumulate,
                        void* stream);
/* MANY fixed-order reductions in ONE launch (round 6): item i computes out[g * ldout + c] = sum_{j < per_group} partials[(g * per_group + j) * D + c]
 * for g < groups, c < D -- exactly what sfron_reduce_chunks(partials, groups, per_group, D, out, ldout, 0) computes, in the same order, bit for
 * bit.  `items` is a HOST array: the items travel by value in the kernel arguments (120 per launch), so there is no device table to build or to
 * keep alive and the call may be captured into a graph.  The parameter-gradient finishes of a U-Net backward pass (GroupNorm / LayerNorm affine
 * gradients, bias gradients, per-sample projection gradients: ~190 launches of ~5 us per DDPM step) are collected by the tape and issued once. */
typedef struct sfron_reduce_item { const float* partials; float* out; int groups, per_group, D, ldout; } sfron_reduce_item;
int sfron_reduce_batch(const sfron_reduce_item* items /* HOST */, int n_items, void* stream);
/* two partial buffers in one launch: out0[g*ld0 + c] = sum_j p0[(g*per_group + j)*D + c], out1 likewise from p1 */
int sfron_reduce2(const float* p0, const float* p1, int groups, int per_group, int D, float* out0, int ld0, float* out1,
                  int ld1, void* stream);
/* bias gradients behind the adaLN gates of all blocks at once (proj.bias: which = 0, fc2.bias: which = 1):
 * out[l*out_stride + out_which{0,1} + c] = sum_b gate[b*ldg + l*gate_stride + which*gate_which + c] * S[((2l+which)*B + b)*D + c]
 * where S holds the per-sample token sums of the upstream gradient (second output of sfron_gate_bwd, reduced). */
int sfron_gated_bias_grads(const float* S, const float* gate, int ldg, long gate_stride, long gate_which, int layers, int B,
                           int D, float* out, long out_stride, long out_which0, long out_which1, void* stream);
/* Deferred reduction of a whole backward pass in ONE launch.  parts holds n_slots slots of slot_stride floats; slot
 * s = layer*8 + kind*2 + buf is a [groups*per_group][D] partial buffer written by sfron_gate_bwd / sfron_ln_modulate_bwd.
 * out: dst_base[kind*2+buf][layer*dst_layer_stride[..] + g*dst_ld[..] + c] = sum_j slot[(g*per_group + j)*D + c].
 * The three arrays are HOST arrays of length 8. */
int sfron_reduce_slots(const float* parts, long slot_stride, int n_slots, int groups, int per_group, int D,
                       float* const* dst_base, const long* dst_layer_stride, const int* dst_ld, void* stream);
/* out[c] = sum_g w[g * ldw + c] * sum_j partials[(g * per_group + j) * D + c]      (bias grad behind a gate) */
int sfron_weighted_reduce(const float* partials, int groups, int per_group, int D, const float* w, int ldw, float* out,
                          void* stream);
/* out[c] = sum_r X[r][c]; X bf16 (is_bf16 = 1) or fp32; partials scratch [max_partials][N]      (bias grads) */
int sfron_colsum(const void* X, int is_bf16, int M, int N, int ld, float* partials, int max_partials, float* out,
                 void* stream);

/* ------------------------------------------------------------------ conditioning / layout (embed.hip) */
/* out[b] = bf16( cos(t*f) || sin(t*f) ), f_j = exp(-ln(1e4) j / (dim/2))    (DiT/models.py:41-59) */
int sfron_timestep_embed(const int64_t* t, int n, int dim, uint16_t* out, int ld, void* stream);
int sfron_silu_fwd(const float* x, int64_t n, uint16_t* y_bf16, void* stream);
int sfron_silu_bwd(const float* dy, const float* x, int64_t n, uint16_t* dx_bf16, float* dx_f32, void* stream);
/* c = t_emb + table[drop ? num_classes : y];  silu_c = bf16(silu(c))   (DiT/models.py:78-94,243; drop may be NULL) */
int sfron_cond_fwd(const float* t_emb, const float* table, const int64_t* y, const uint8_t* drop, int num_classes, int n,
                   int D, float* c, uint16_t* silu_c, void* stream);
/* d_c = d_silu_c * silu'(c); d_table[label] += d_c  (d_table must be zeroed by the caller) */
int sfron_cond_bwd(const float* d_silu_c, const float* c, const int64_t* y, const uint8_t* drop, int num_classes, int n,
                   int D, float* d_c, float* d_table, void* stream);
/* step guard (fail-loud checks without host syncs; guard.py polls `flags` behind an event).  flags: fp32 [4] =
 * {non-finite loss, non-finite gradient norm, label outside [0, num_classes), timestep outside [0, num_timesteps)}, accumulated.
 * guard_inputs: y_safe / t_safe = the inputs clamped into range (what the kernels then index with), flags[2] / [3] += number of
 * clamped entries -- where the reference's nn.Embedding / table gather raise IndexError (DiT/models.py:89-93,
 * gaussian_diffusion.py:861-873).  guard_finite: a (and optional b, c, d) are per-sample loss terms [n]; stats (optional) =
 * the clip statistics of sfron_clip_coef, stats[0] = gradient norm (the values DiT/forget.py:329-336 logs). */
int sfron_guard_inputs(const int64_t* y, const int64_t* t, int n, int num_classes, int num_timesteps, int64_t* y_safe, int64_t* t_safe,
                       float* flags, void* stream);
int sfron_guard_finite(const float* a, const float* b, const float* c, const float* d, int n, const float* stats, float* flags, void* stream);
/* latent front-end: out [n][c][hw] = (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) * scale from cached VAE posterior moments
 * [n][2c][hw] = mean || logvar -- vae.encode(x).latent_dist.sample().mul_(0.18215) of DiT/forget.py:265-267,305-307 with the
 * encoder's output cached offline (diffusers' DiagonalGaussianDistribution.sample; diffusers is absent here: parity unpinned) */
int sfron_latent_sample(const float* moments, const float* eps, int n, int c, int hw, float scale, float* out, void* stream);
/* VAE encoder tail: quant_conv over the fp32 conv_out rows [B*hw][ld] (z2 = 2z <= 16 columns read): m[o] = bias[o] + sum_i w[o][i] x[i] as
 * fp32 FMAs in ascending i (w = quant_conv.weight [z2][z2][1][1]).  Writes the posterior moments NCHW [B][z2][hw] (mean || logvar) to
 * moments_f32 and / or moments_f16 (RNE); with eps [B][z2/2][hw] also latent [B][z2/2][hw] = sfron_latent_sample of the fp32 moments, bit
 * for bit (eps and latent both NULL or both set). */
int sfron_vae_moments(const float* rows, int ld, int B, int hw, int z2, const float* w, const float* bias, float* moments_f32,
                      uint16_t* moments_f16, const float* eps, float scale, float* latent, void* stream);
/* VAE decoder head: post_quant_conv(z / scale) over the NCHW fp32 latents z [B][zc][hw] (zc <= 16): x = z / scale (correctly rounded
 * fp32 division), y[p][o] = bias[o] + sum_{c = 0..zc-1} w[o][c] * x[c] in that order, each product and sum rounded separately (w =
 * post_quant_conv.weight [zc][zc][1][1]).  Writes bf16 rows [B*hw][c_pad] (RNE; c_pad >= zc, c_pad % 8 == 0, channels zc.. zero) -- what
 * conv_in reads -- and, when rows_f32 is set, the same values [B*hw][c_pad] in fp32 before the rounding.  Both 16-byte aligned. */
int sfron_vae_latent_in(const float* z, int B, int zc, int hw, const float* w, const float* bias, float scale, int c_pad, uint16_t* rows,
                        float* rows_f32, void* stream);
/* NCHW fp32 image -> bf16 token rows [n*T][C*p*p]; chan_last 0: k = c*p*p + ph*p + pw (Conv2d weight order,
 * timm PatchEmbed); 1: k = (ph*p + pw)*C + c (unpatchify order, DiT/models.py:218-231) */
int sfron_patchify(const float* img, int n, int C, int H, int W, int p, int chan_last, uint16_t* rows, int ld, void* stream);
int sfron_unpatchify(const float* rows, int ld, int n, int C, int H, int W, int p, float* img, void* stream);

/* ------------------------------------------------------------------ attention (attn.hip)
 * qkv [B*T][3*H*hd] bf16 (column = which*D + head*hd + d), o / d_o [B*T][H*hd] bf16, lse [B][H][T] fp32.
 * softmax(q k^T * hd^-0.5) v, non-causal (timm Attention as used at DiT/models.py:108,120).
 * Supported: T % 64 == 0 with head_dim a multiple of 8 up to 80 (DiT 64 / 72; the LDM UNet's 40 / 80) on the tiled kernels; T < 64
 * (any T, head_dim <= 128: the patch-8 DiT models at 256 px have 16 tokens) on plain-FMA kernels, one workgroup per (batch, head). */
int sfron_attn_fwd(const uint16_t* qkv, uint16_t* o, float* lse, int B, int T, int H, int hd, void* stream);
/* dqkv [B*T][3*H*hd] bf16 = gradient wrt qkv; delta_scratch fp32 [B*H*T] (used by the two-kernel form only).
 * T = 128 / 256: ONE kernel, one 8-wave workgroup per (batch, head): S and dP are formed once per (query chunk, key block),
 * dV and dK accumulate from registers, dS crosses LDS once and dQ is formed from that image -- 5 products, no atomics.
 * Other T (multiples of 64): dQ kernel + dK/dV kernel (7 products). */
int sfron_attn_bwd(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse, float* delta_scratch,
                   uint16_t* dqkv, int B, int T, int H, int hd, void* stream);
/* the same backward pass (one-kernel form only: sfron_attn_bwd_bias_supported(T)) that also leaves the qkv.bias gradient partials:
 * bias_partials fp32 [B][3*H*hd], row b = sum over the T tokens of sample b of dqkv (fp32, before the bf16 rounding; fixed
 * summation order, no atomics) -- sum the B rows with sfron_reduce_chunks.  Replaces a second pass over dqkv (sfron_colsum):
 * the bias gradient of timm Attention.qkv (DiT/models.py:108,120 backward). */
int sfron_attn_bwd_bias_supported(int T);
int sfron_attn_bwd_bias(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse, uint16_t* dqkv, float* bias_partials,
                        int B, int T, int H, int hd, void* stream);

/* test hook: 2 = always the two-kernel backward, 0 = default; returns the previous setting (process-wide, not thread-safe) */
int sfron_attn_bwd_form(int form);
/* test / A-B hook: 0 (default) = by rule (eight waves of 16 query rows per workgroup for sequences of 512 tokens or more, four waves of 32
 * rows below), 4 / 8 / 16 = force the four-wave / eight-wave 16-row / eight-wave 32-row (one workgroup per 256 query rows; measured slower)
 * form, 2 (round 6) = four waves walking BOTH 128-row query blocks of a head as one chunk stream where the sequence is a multiple of 256 rows
 * (measured: not faster) -- each where the sequence length allows it (bit-identical results); returns the previous setting */
int sfron_attn_fwd_form(int form);
/* Process-wide form of the three-slot GEMM tiles (256 x 144 forward / dgrad, 192 x 192 weight gradient): 4 = four extra LOADER waves per
 * workgroup issue every LDS-DMA piece and the eight multiplying waves none (csrc/gemm.hip k_gemm_pipe NL; taken by the dgrad and
 * weight-gradient layouts, where it measured faster) -- the default; 0 = every wave issues its share (5 / 6: weight gradients / dgrad
 * only, 9: the fp8 tiles in their loader form too -- for A-B runs).  The pipelined convolution tiles (csrc/conv.hip k_cgemm / k_cgemm_t,
 * contractions of >= 8 K-tiles) follow: loader form unless n == 0 (10 / 11 / 12: as 4 with none / only k_cgemm / only k_cgemm_t of
 * them in the loader form).  Same results bit for bit (same products, same summation order).  Returns the previous value.
 * The product build accepts 0, 4, 9 and 10 (what the form-equivalence tests use) and ignores any other value; the A-B values 5..8, 11, 12
 * exist in the debug-knob build (make dbg: libsfron_dbg.so, tools/ only). */
int sfron_gemm_loader_waves(int n);

/* ------------------------------------------------------------------ whole-model DiT pass (dit_engine.hip)
 * Replaces autograd over DiT.forward (DiT/models.py:233-248) inside the SFR-on step (DiT/forget.py:271-288,310-319).
 * Parameters live in ONE arena (fp32 master, bf16 shadow and fp32 grads share offsets); sfron_dit_param_layout
 * reports the offsets so the host can expose every tensor under its reference state_dict key. */
typedef struct sfron_dit_cfg {
  int batch;          /* per-GPU batch */
  int in_channels;    /* 4 */
  int input_size;     /* latent side, 32 for 256 px */
  int patch;          /* 2 / 4 / 8 */
  int hidden;         /* D */
  int depth;          /* L */
  int heads;          /* H; head_dim = D / H must be 64 or 72 */
  int mlp_hidden;     /* 4 D */
  int num_classes;    /* table has num_classes + 1 rows (CFG null class) */
  int freq_dim;       /* 256 */
  int out_channels;   /* 8 with learn_sigma */
} sfron_dit_cfg;

/* out[SFRON_DIT_LAYOUT_LEN] (element offsets into the arena): total, trainable, pe_w, pe_b, t0_w, t0_b, t2_w, t2_b,
 * table, ada_w, ada_b, blocks, blk_stride, then offsets inside a block: qkv_w, qkv_b, proj_w, proj_b, fc1_w, fc1_b,
 * fc2_w, fc2_b, then fin_w, fin_b, pos.  ada_w is [(6*depth+2)*D][D]: block l rows [6lD, 6(l+1)D), final layer last. */
#define SFRON_DIT_LAYOUT_LEN 24
int sfron_dit_param_layout(const sfron_dit_cfg* cfg, int64_t* out, int n_out);
int64_t sfron_dit_workspace_bytes(const sfron_dit_cfg* cfg);   /* < 0 on unsupported cfg */

/* Config 5 operands of the forward pass: the four block GEMMs on the fp8 matrix core.  params_e4m3: e4m3 shadow arena (same offsets as
 * params); w_scales: DEVICE fp32 [depth][4] = quantisation scales of {qkv, proj, fc1, fc2}.weight of each block; act_scales: static scales
 * of {LayerNorm+modulate output, attention output, gelu(fc1)}, by value, all three > 0; act_amax: the caller's activation-range words
 * (sfron_fp8_activation_amax), NULL = no tracking; workspace_e4m3: sfron_dit_fp8_workspace_bytes. */
int64_t sfron_dit_fp8_workspace_bytes(const sfron_dit_cfg* cfg);
typedef struct sfron_dit_fp8_operands {
  const uint8_t* params_e4m3;
  const float* w_scales;       /* DEVICE [depth][4] */
  float act_scales[3];
  uint32_t* act_amax;          /* DEVICE [3] or NULL */
  void* workspace_e4m3;
} sfron_dit_fp8_operands;

/* `phase` of sfron_dit_fwd */
enum { SFRON_DIT_PASS_WHOLE = 0,             /* prologue + blocks + final layer */
       SFRON_DIT_PASS_PROLOGUE = 1,          /* everything in front of block 0 */
       SFRON_DIT_PASS_BLOCKS = 2,            /* blocks + final layer on a workspace a prologue filled */
       SFRON_DIT_PASS_PROLOGUE_NO_ADA = 3,   /* prologue without the adaLN product */
       SFRON_DIT_PASS_ADA = 4 };             /* the adaLN product alone */

/* One forward pass: out [B][out_channels][S][S] fp32 = DiT(x_t, t, y).  Saves activations in `workspace` for sfron_dit_backward -- the same
 * bf16 activations with and without `fp8`, so the backward pass follows unchanged (straight-through estimator).  params, params_bf16, x_t,
 * t, y, workspace and out must be set in every phase; everything is checked before the first launch (SFRON_ERR_ARG). */
typedef struct sfron_dit_fwd {
  const sfron_dit_cfg* cfg;
  const float* params; const uint16_t* params_bf16;
  void* workspace;               /* sfron_dit_workspace_bytes */
  const float* x_t; const int64_t* t; const int64_t* y;
  const uint8_t* drop;           /* [B] uint8 (1 = replace label by the null class) or NULL */
  float* out;
  /* hipEvent_t [depth], NULL entries skipped, or NULL: block l first waits (hipStreamWaitEvent on `stream`) for block_ready[l].  The
   * optimizer sweep of the previous stage may still be rewriting the LATER blocks' weights on another stream while the first blocks already
   * run (DiT/forget.py:299 -> :310: the remain forward needs block l's new weights only at block l). */
  void* const* block_ready;
  /* sfron_probe_create, or NULL: HIP events recorded (on `stream`) around the fc1 GEMM of block 0 -- the dominant kernel class -- for
   * bench.py's live roofline measurement.  With `fp8` set nothing is recorded into it. */
  void* probe;
  /* SFRON_DIT_PASS_*: the pass in several calls with the same descriptor (round 6).  PROLOGUE = only what stands in front of block 0 --
   * patch embedding, timestep / label embedders, the adaLN modulation of every block: the "conditioning prologue", a chain of ten small
   * dependent launches; BLOCKS = only the blocks and the final layer, on the workspace the PROLOGUE call filled.  A caller whose optimizer
   * sweep of the block ranges runs beside the pass on another stream (block_ready) starts that sweep BETWEEN the two calls: beside a
   * bandwidth-heavy sweep every boundary between two small dependent launches costs 60-100 us instead of ~5
   * (profiles/r06_stage_boundary.txt).  PROLOGUE_NO_ADA = PROLOGUE without its last launch -- the adaLN product silu(c) W_ada^T + b, the only
   * launch in front of block 0 that reads the adaLN_modulation matrix (DiT/models.py:113-116,119) -- and ADA = that launch alone (ABI 16): a
   * caller whose optimizer sweep of that matrix runs on another stream issues PROLOGUE_NO_ADA beside it, orders `stream` behind the sweep,
   * then ADA and BLOCKS.  The phases that stop in front of block 0 (PROLOGUE, PROLOGUE_NO_ADA, ADA) ignore block_ready, probe and out.
   * Same workspace, same results as WHOLE. */
  int phase;
  /* NULL = bf16 block GEMMs.  Set: SFRON_ERR_UNSUPPORTED when a block GEMM shape is not a multiple of the fp8 tile
   * (sfron_fp8_gemm_supported). */
  const sfron_dit_fp8_operands* fp8;
} sfron_dit_fwd;
int sfron_dit_forward(const sfron_dit_fwd* pass, void* stream);
int sfron_probe_create(int max_samples, void** probe /* HOST out */);
int sfron_probe_reset(void* probe);
int sfron_probe_read(void* probe, int* n_samples, double* total_ms);   /* synchronises on the recorded events */
int sfron_probe_destroy(void* probe);

/* One backward pass over the workspace a forward pass filled: grads (arena layout, trainable part fully overwritten) = d loss / d params
 * given d_out = d loss / d out.  (Reference: autograd's loss.backward(), DiT/forget.py:288.) */
typedef struct sfron_dit_bwd {
  const sfron_dit_cfg* cfg;
  const float* params; const uint16_t* params_bf16;
  void* workspace;
  const float* d_out; const int64_t* y;
  const uint8_t* drop;           /* as in the forward pass, or NULL */
  float* grads;
  /* from sfron_aux_create, or NULL: a side HIP stream + events; the weight-gradient GEMMs and bias column sums then run concurrently with
   * the dgrad / elementwise chain and join `stream` before the call's work ends. */
  void* aux;
  /* Data-parallel form (either may be NULL; block_events needs aux).  block_events: L hipEvent_t handles (entries may be NULL), event l is
   * recorded on the aux handle's weight-gradient stream once every gradient inside block l's arena range is final except proj.bias and fc2.bias;
   * late_bias: fp32 [L][2][D] that receives those two instead of the arena.  The host can then all-reduce block ranges while the backward
   * pass is still running, all-reduce late_bias and the non-block ranges at the end, and call sfron_dit_scatter_late_bias to put the
   * reduced biases into the arena.  (Reference: nn.DataParallel reduces after loss.backward(), DiT/forget.py:193,288.) */
  void* const* block_events;
  float* late_bias;
  /* Both or neither.  Set: the adaLN_modulation weight gradient (all blocks + final layer, [(6L+2)D][D], a third of the arena) is NOT
   * computed; instead its two bf16 factors dmod [B][(6L+2)D] and silu(c) [B][D] are copied out, so that the host all-gathers them over the
   * ranks and forms dmod_all^T silu(c)_all with one sfron_gemm_bf16 over the global batch. */
  uint16_t* ada_dmod_out; uint16_t* ada_sc_out;
} sfron_dit_bwd;
int sfron_dit_backward(const sfron_dit_bwd* pass, void* stream);
int sfron_dit_scatter_late_bias(const sfron_dit_cfg* cfg, const float* late_bias, float* grads, void* stream);
int sfron_aux_create(void** aux /* HOST out */);
/* attach a probe (sfron_probe_create; NULL detaches): the backward pass then records an event pair on the weight-gradient
 * stream around each of the four weight-gradient GEMMs (qkv, proj, fc1, fc2) of every 9th block -- the kernel that holds the
 * largest share of GPU time -- for bench.py's live roofline figure */
int sfron_aux_set_probe(void* aux, void* probe);
/* One-shot: the NEXT sfron_dit_backward call through this handle also leaves the masked sum of squares of every block weight gradient
 * (qkv / proj / fc1 / fc2 weights of all blocks) in `partials` -- fp64 [sfron_dit_sumsq_partials_len(cfg)], one per 192 x 192 output tile, every
 * entry rewritten by the pass -- taken from the accumulators of the weight-gradient GEMMs (sfron_gemm_desc.sumsq_partials).  mask_arena: byte mask
 * indexed like the parameter / gradient arena (NULL = no mask).  The clip norm of DiT/forget.py:289-298 then needs a pass only over what is left
 * (biases, embedders, final layer: sfron_sumsq_masked_ranges) plus sfron_clip_coef.  Single-process runs only: a data-parallel run must take the
 * norm of the REDUCED gradient.  sfron_dit_sumsq_partials_len returns 0 when a block shape does not run on the 192 x 192 weight-gradient tile.
 * partials == NULL DISARMS the handle (a caller whose pass failed between arming and the backward pass must not leave the pointer behind). */
int sfron_dit_sumsq_partials_len(const sfron_dit_cfg* cfg);
int sfron_aux_arm_sumsq(void* aux, const uint8_t* mask_arena, double* partials);
/* Orders `stream` behind the point of the LAST backward pass run with this handle after which the adaLN_modulation matrix (weights, bf16
 * shadow) is not read and its gradient factors (sfron_dit_bwd: ada_dmod_out / ada_sc_out) are complete: the dgrad through that
 * Linear.  What remains of the pass is the embedders' backward; the clip norm's share of the adaLN matrix (sfron_sumsq_lowrank) may run
 * beside it on another stream (the host mirror does: -0.12 ms per step; sweeping the matrix itself there measured slower).  No-op before
 * the first backward pass.  Replaces nothing in the reference: scheduling of DiT/forget.py:293-298. */
int sfron_aux_wait_ada(void* aux, void* stream);
/* Orders `stream` behind the point of the LAST sfron_dit_backward call with ada_dmod_out / ada_sc_out through this handle at which those two
 * factors are complete (earlier than sfron_aux_wait_ada: the dgrad through the adaLN Linear is still to come).  sfron_sumsq_lowrank reads
 * nothing else.  No-op before the first such pass. */
int sfron_aux_wait_ada_factors(void* aux, void* stream);
/* The handle's two weight-gradient streams (hipStream_t, owned by the library: read-only use).  For callers that put work of their own beside a
 * backward pass -- a gradient exchange, a sweep -- and must pick a stream that does NOT share a hardware queue with these two: the runtime maps
 * streams onto four hardware queues and two streams on one queue serialise (profiles/r06_hw_queues.txt; the host mirror probes: streams.py). */
int sfron_aux_streams(void* aux, void** side /* HOST out */, void** side2 /* HOST out */);
/* Arms the handle for the fp8 backward: every sfron_dit_backward call through it then runs the four dgrads of each block on the fp8
 * matrix core (sfron_fp8_dgrad) -- dY cast by sfron_cast_mx8 (d_br, d_br2, dqkv) or by the fc2 dgrad's epilogue (d_hpre); the weight
 * gradients keep reading the bf16 tensors.  w8t: the transposed e4m3 shadow of the block weights, indexed like the block range of the arena
 * (matrix j of block l at its arena offset minus the offset of block 0 rounded down to a multiple of 256); w_scales: fp32 [L][4] (qkv, proj, fc1, fc2), the forward pass's
 * shadow scales; mx_workspace: sfron_dit_fp8_dgrad_workspace_bytes(cfg) bytes.  The caller keeps w8t equal to the transpose of the shadow
 * the forward pass read.  w8t == NULL disarms.  A backward pass on an armed handle returns SFRON_ERR_UNSUPPORTED for shapes the fp8 tiles
 * do not take. */
int64_t sfron_dit_fp8_dgrad_workspace_bytes(const sfron_dit_cfg* cfg);
int sfron_aux_set_fp8_dgrad(void* aux, const uint8_t* w8t, const float* w_scales, void* mx_workspace);
/* Arms the handle for fp8 weight gradients: every sfron_dit_backward call through it then forms the qkv, proj, fc1 and fc2 weight
 * gradients of each block with sfron_fp8_wgrad -- dY and the forward input X (xmod1 / o / xmod2 / h) cast by sfron_cast_mx8_t on the
 * weight-gradient stream itself, into this handle's workspace (one operand pair per weight-gradient stream: reuse follows that stream's
 * order).  Biases, adaLN, the embedders and the final layer are unchanged.  Independent of the fp8 forward and of the fp8 dgrads.
 * workspace: sfron_dit_fp8_wgrad_workspace_bytes(cfg) bytes, 16-byte aligned; NULL disarms.  A backward pass on an armed handle returns
 * SFRON_ERR_UNSUPPORTED for block shapes sfron_fp8_wgrad_supported refuses. */
int64_t sfron_dit_fp8_wgrad_workspace_bytes(const sfron_dit_cfg* cfg);
int sfron_aux_set_fp8_wgrad(void* aux, void* workspace);
int sfron_aux_destroy(void* aux);

/* ------------------------------------------------------------------ CLIP text encoder (text.hip)
 * SD v1's FrozenCLIPEmbedder (SD/ldm/modules/encoders/modules.py:230-266: CLIPTextModel(input_ids).last_hidden_state), forward only.  The
 * residual stream is fp32 rows [B*T][D]; the per-layer LayerNorms are sfron_layernorm_fwd (bf16 out), q / k / v one sfron_gemm_bf16
 * (SFRON_EPI_BF16) into [B*T][3D], out_proj and fc2 SFRON_EPI_F32 with bias and accumulate = 1 into the residual stream, fc1
 * SFRON_EPI_QUICK_GELU. */
/* out fp32 [B*T][D] = tok_emb[ids[b][t]] + pos_emb[t] (ids int64 [B][T], tok_emb fp32 [vocab][D], pos_emb fp32 [>= T][D]).  An id outside
 * [0, vocab) is not read: its row is written as zeros and *err (a caller-owned device int, zeroed by the caller) gets bit 0 set. */
int sfron_clip_embed(const int64_t* ids, int B, int T, const float* tok_emb, int vocab, const float* pos_emb, int D, float* out, int* err,
                     void* stream);
/* causal softmax(q k^T * hd^-0.5) v: qkv / o in the layout of sfron_attn_fwd (qkv bf16 [B*T][3*H*hd], column = which*D + head*hd + d;
 * o bf16 [B*T][H*hd]); key j > query i is masked.  T <= 128 and hd == 64 only (else SFRON_ERR_UNSUPPORTED); one workgroup per (sample, head).
 * qkv 16-byte, o 8-byte aligned.  Rows at or beyond T are neither read nor written. */
int sfron_attn_causal_fwd(const uint16_t* qkv, uint16_t* o, int B, int T, int H, int hd, void* stream);
/* fused cross-attention forward (csrc/xattn.hip; inference: nothing is kept for a backward pass): o = softmax(scale q k^T) v per (sample,
 * head), bf16 operands as the batched products of the UNet take them: q [B*N][ldq], k / v [B*Lk][ldk / ldv], o [B*N][ldo], head h in
 * columns h*hd .. h*hd + hd - 1.  Keys Lv <= j < Lk are padding with probability 0 (their rows are never read).  hd 40 / 80 / 160,
 * 1 <= Lv <= Lk <= 128, Lk % 8 == 0, any N >= 1 (else SFRON_ERR_UNSUPPORTED).  q / k / v 16-byte aligned with leading dimensions that are
 * multiples of 8, o 8-byte aligned with ldo % 4 == 0.  No scores or probabilities reach global memory; offsets are 64-bit. */
int sfron_xattn_fwd(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, uint16_t* o, int ldo, int B, int N,
                    int Lk, int Lv, int H, int hd, float scale, void* stream);
/* sfron_xattn_fwd for training: the same kernel (o is bit-identical) with one more store per query row, lse fp32 [B*H*N],
 * lse[(b*H + h)*N + n] = m + log(l) = log sum_j exp(scale q_n . k_j) over the keys j < Lv -- what sfron_xattn_bwd rebuilds P from. */
int sfron_xattn_fwd_lse(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, uint16_t* o, int ldo, int B, int N,
                        int Lk, int Lv, int H, int hd, float scale, float* lse, void* stream);
/* fused cross-attention backward (csrc/xattn.hip), shapes and layouts of sfron_xattn_fwd: with P = exp(scale q k^T - lse) (keys >= Lv: 0),
 * delta = rowsum(d_o o o), dP = d_o v^T and dS = scale P o (dP - delta):  dq [B*N][lddq] = dS k,  dk [B*Lk][lddk] = dS^T q,
 * dv [B*Lk][lddv] = P^T d_o (bf16, head h in columns h*hd ..; the layouts the batched products of UNetModel._mha write).  P and dS are
 * rounded to bf16 as MFMA operands, sums are fp32, outputs are rounded once; no score-sized matrix reaches global memory.  Rows Lv .. Lk-1
 * of dk / dv are written as exact zeros and those rows of k / v are never read; rows of dq at or beyond B*N and columns at or beyond H*hd
 * of any output are not touched.  dk / dv are summed over the queries in a fixed order (fp32 partial slabs in ws, one per chunk of 64-row
 * query tiles, then a finishing kernel that adds them in chunk order): no atomics, two calls give the same bits.
 * ws: caller-owned, 16-byte aligned, at least sfron_xattn_bwd_ws_bytes(B, N, Lk, H, hd) bytes, contents undefined before and after.
 * q / k / v / o / d_o 16-byte aligned with leading dimensions % 8 == 0; dq / dk / dv 8-byte aligned with leading dimensions % 4 == 0.
 * Unsupported hd / Lk: SFRON_ERR_UNSUPPORTED; anything else wrong (ws too small included): SFRON_ERR_ARG; both before any launch. */
int64_t sfron_xattn_bwd_ws_bytes(int B, int N, int Lk, int H, int hd);
int sfron_xattn_bwd(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, const uint16_t* o, int ldo,
                    const uint16_t* d_o, int ldd_o, const float* lse, uint16_t* dq, int lddq, uint16_t* dk, int lddk, uint16_t* dv, int lddv, int B,
                    int N, int Lk, int Lv, int H, int hd, float scale, void* ws, int64_t ws_bytes, void* stream);
/* fused self-attention for wide heads (csrc/wattn.hip): o = softmax(scale q k^T) v per (sample, head) over the T tokens of the sample
 * itself, bf16 operands by address + leading dimension as sfron_xattn_fwd takes them: q / k / v / o [B*T][ld], head h in columns
 * h*hd .. h*hd + hd - 1 (one [B*T][3*H*hd] qkv matrix serves as three column slices).  hd 160 or 256, T a multiple of 64 with
 * 64 <= T <= 1024 -- sfron_wattn_supported(T, hd) returns 1 for exactly these -- anything else SFRON_ERR_UNSUPPORTED.  lse may be NULL
 * (inference); otherwise fp32 [B*H*T], lse[(b*H + h)*T + t] = m + log(l) = log sum_j exp(scale q_t . k_j), what sfron_wattn_bwd rebuilds
 * P from.  o is bit-identical with and without lse.  K / V stream through LDS in chunks of 64 keys under an fp32 online softmax; no
 * scores or probabilities reach global memory; offsets are 64-bit.  Every pointer 16-byte aligned (lse: 4), every leading dimension a
 * multiple of 8 and >= H*hd; a refusal (SFRON_ERR_UNSUPPORTED for the shape, SFRON_ERR_ARG for anything else) comes before any launch. */
int sfron_wattn_supported(int T, int hd);
int sfron_wattn_fwd(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, uint16_t* o, int ldo, float* lse, int B,
                    int T, int H, int hd, float scale, void* stream);
/* backward of sfron_wattn_fwd, same shapes and layouts: with P = exp(scale q k^T - lse), delta = rowsum(d_o o o), dP = d_o v^T and
 * dS = scale P o (dP - delta):  dq = dS k,  dk = dS^T q,  dv = P^T d_o (bf16 [B*T][ld], head h in columns h*hd ..).  P and dS are rounded
 * to bf16 as MFMA operands, sums are fp32, outputs are rounded once.  Two kernels: one over query tiles (delta -> ws, dq), one over key
 * tiles (dk, dv; a workgroup owns its 64 keys and walks the queries in order): no atomics, no partial sums between workgroups, two
 * calls give the same bits.  ws: caller-owned, 16-byte aligned, at least sfron_wattn_bwd_ws_bytes(B, T, H, hd) bytes (delta, fp32
 * [B*H*T]), contents undefined before and after.  Refusals as sfron_wattn_fwd; a workspace that is too small is SFRON_ERR_ARG. */
int64_t sfron_wattn_bwd_ws_bytes(int B, int T, int H, int hd);
int sfron_wattn_bwd(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv, const uint16_t* o, int ldo,
                    const uint16_t* d_o, int ldd_o, const float* lse, uint16_t* dq, int lddq, uint16_t* dk, int lddk, uint16_t* dv, int lddv, int B,
                    int T, int H, int hd, float scale, void* ws, int64_t ws_bytes, void* stream);
/* y fp32 [rows][D] = LayerNorm(x; eps) * gamma + beta (the final LayerNorm: last_hidden_state is fp32) */
int sfron_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, int64_t rows, int D, float eps, float* y, void* stream);
/* Pillow's antialiased Image.resize of one 8-bit RGB image with a crop window folded in (csrc/resample.hip), bit for bit:
 * src uint8 [Hs][Ws][3] -> dst uint8 [Ho][Wo][3], the window of the resized image.  The filter lives in host-made tables
 * (sfron.resample.resample_tables: Pillow's 8-bit path, PRECISION_BITS 22): kx int32 [Wo][ksx] / bx int32 [Wo][2] = (xmin, count) for the
 * window's columns, ky [Ho][ksy] / by [Ho][2] for its rows (tables already sliced to the window by the caller; all four in device memory).
 * Per pass, pixel and channel: ss = 2^21 + sum_{x < count} in[xmin + x] * k[x] in int32, out = clamp(ss >> 22, 0, 255) (arithmetic
 * shift).  The horizontal pass runs first, over the window's columns and only the source rows the window's rows read, and writes uint8
 * (that rounding is part of the result) into tmp, uint8 [rows y0..y1)[Wo][3] with [y0, y1) the union of by; the vertical pass reads tmp.
 * An axis that keeps its size is a table of one tap of exactly 2^22.  Two launches on `stream`, no allocation, no synchronisation
 * (graph-capturable); offsets are 64-bit; src rows need no alignment (3 * Ws bytes each).
 * Who checks what.  This entry point sees the scalars and the addresses, not the tables' contents: SFRON_ERR_ARG, before any launch and
 * with tmp / dst untouched, for a null pointer, a non-positive extent, ksx or ksy < 1, a row of 2 GiB or more, or tmp_bytes below one row
 * (Wo * 3).  The tables are the caller's host data before they are uploaded, so the checks that need their contents belong to the
 * wrapper (sfron.resample.image_resample_u8, same status code, before the upload): every bound inside the source (0 <= xmin,
 * count >= 0, xmin + count <= Ws, count <= ksx; rows likewise against Hs), ascending row bounds, and tmp_bytes >= (y1 - y0) * Wo * 3.
 * Behind that, the kernels clamp each bound they read into [0, Ws] / [0, Hs] / the taps per output / the rows tmp_bytes holds, so a
 * table that slipped past gives wrong pixels, never an access outside src, tmp or dst. */
int sfron_image_resample_u8(const uint8_t* src, int Hs, int Ws, const int32_t* kx, const int32_t* bx, int ksx, const int32_t* ky,
                            const int32_t* by, int ksy, int Wo, int Ho, uint8_t* tmp, int64_t tmp_bytes, uint8_t* dst, void* stream);
/* The batched form (csrc/resample.hip): chains of such resizes -- ADM's center_crop_arr is BOX halvings, then BICUBIC, then the crop,
 * sfron.resample.center_crop_plan -- for a whole batch of images of different sizes, in a number of launches that does not depend on the
 * batch.  The arithmetic per pass is exactly that of sfron_image_resample_u8, and the device code is shared with it.
 *   pool .... device bytes holding the sources, each uint8 [h][w][3] at its own byte offset (any alignment)
 *   tables .. device int32 blob of n_tables words holding every coefficient table [n][ksize] and bounds table [n][2] the passes use
 *   passes .. device array of n_passes records, one per image, stage and axis, grouped by level
 *   work .... device bytes for everything between a source and a result; out: device bytes the last vertical pass of each image writes
 * A stage is a horizontal pass (level 2s) and a vertical pass over its result (level 2s + 1); an image counts its stages from its own
 * first one, so an image with fewer stages finishes in an earlier level.  One launch per level: n_levels = 2 * (most stages of an image).
 * level_first / level_rows / level_cols are HOST arrays, read during the call: level l holds passes level_first[l] ..
 * level_first[l + 1] - 1 (level_first has n_levels + 1 entries, from 0 to n_passes, strictly ascending); level_rows[l] is the largest
 * row count of its passes (horizontal: nrows; vertical: n_out) and level_cols[l] the largest extent along a row (horizontal: n_out
 * pixels; vertical: 3 * in_w bytes).  The grid of a level spans them and a workgroup beyond its own pass's extents exits.
 * No allocation, no synchronisation (graph-capturable), 64-bit offsets, plain vector stores.
 * Who checks what, as for sfron_image_resample_u8.  SFRON_ERR_ARG before any launch, with work / out untouched: a null pointer, a
 * non-positive count or size, an odd n_levels, a level list that does not ascend from 0 to n_passes, a level of more than 65535 passes
 * or 65535 * 256 columns, or a pool / work / out below what the largest extents imply (pool: 3 * level_rows[0]; work: 3 * the larger
 * extent of every horizontal level; out: 3 * level_rows and level_cols of the last level).  The records are device data: the wrapper
 * (sfron.resample.image_resample_batch_u8, same status, before the upload) checks bounds inside their input, ascending row bounds,
 * offsets and extents inside pool / work / out / tables, and that no pass reads or writes what another pass of its level writes.
 * Behind that the kernels clamp every offset, extent and bound they read from a record or a table into the buffer it addresses. */
enum { SFRON_RESAMPLE_POOL = 0, SFRON_RESAMPLE_WORK = 1, SFRON_RESAMPLE_OUT = 2 };
typedef struct sfron_resample_pass {     /* 16 x int64 */
  int64_t in_buf, in_off;                /* input: SFRON_RESAMPLE_POOL (horizontal passes only) or _WORK, and its byte offset there */
  int64_t in_w, in_h;                    /* pixels per row and rows of the input held at in_off (a window of the previous stage, or a source) */
  int64_t out_buf, out_off;              /* output: _WORK, or _OUT (vertical passes only), and its byte offset; rows are packed */
  int64_t n_out;                         /* outputs along the axis: columns of a horizontal pass, rows of a vertical one */
  int64_t org;                           /* the index the bounds count from: the first column (horizontal) / row (vertical) held at in_off */
  int64_t row0, nrows;                   /* horizontal: the input rows it resamples, [row0, row0 + nrows) of in_h, written as rows 0 .. nrows - 1 */
  int64_t k_off, b_off, ksize;           /* word offsets of coefficients [n_out][ksize] and bounds [n_out][2] in tables */
  int64_t reserved[3];
} sfron_resample_pass;
int sfron_image_resample_batch_u8(const uint8_t* pool, int64_t pool_bytes, const int32_t* tables, int64_t n_tables,
                                  const sfron_resample_pass* passes, int n_passes, const int32_t* level_first, const int32_t* level_rows,
                                  const int32_t* level_cols, int n_levels, uint8_t* work, int64_t work_bytes, uint8_t* out, int64_t out_bytes,
                                  void* stream);

/* ------------------------------------------------------------------ DDPM guided sampling (ddpm_sample.hip)
 * Classifier-free guidance + one generalized step of DDPM/functions/denoising.py:72-95 in one pass:
 *   e = (1 + cond_scale) * eps_cond + (-cond_scale) * eps_null   (eps_null NULL: e = eps_cond, the reference's cond_scale == 0 case, or a
 *                                                                 model that hands over the combined epsilon)
 *   x0_pred = (x - e*s1)/s2;  x_next = (s3*x0_pred + c1*noise) + c2*e
 * with (s1, s2, s3, c1, c2) = coef[k], k = *step clamped into [0, steps): coef is a DEVICE table float [steps][5] in the meaning of
 * sfron_ddim_step, step a DEVICE int32, so a captured graph replays unchanged for every step.  Bit-equal to sfron_axpby(eps_cond,
 * eps_null, 1.0 + cond_scale, -cond_scale) followed by sfron_ddim_step with that row, for every scale: cond_scale is a double, and
 * 1.0 + cond_scale and -cond_scale are each rounded once to fp32, as a caller's double expressions are on their way into sfron_axpby.  noise may be NULL where every c1 is 0 (a NULL
 * noise counts as zeros), x0_pred may be NULL, x_next may be x; 64-bit element count.  The table's contents are the caller's: a row with
 * s2 == 0 is refused where the table is built on the host (sfron.ddpm.generalized_coefficients).  SFRON_ERR_ARG before any launch for a
 * null pointer, n or steps < 1, a cond_scale that is not finite, or an x0_pred that aliases x or x_next. */
int sfron_ddpm_guided_step(const float* x, const float* eps_cond, const float* eps_null, const float* noise, double cond_scale,
                           const float* coef, int steps, const int32_t* step, int64_t n, float* x_next, float* x0_pred, void* stream);
/* The step counter of a sampling loop, one workgroup: k = *step clamped into [0, steps); t[0 .. nt) = tseq[min(k + 1, steps - 1)] (the
 * model's float timestep input for the next step, tseq a device table float [steps]); *step = k + 1.  A launch of its own behind the
 * step kernel: a step kernel that incremented the index itself would race with its own workgroups that have not read it yet. */
int sfron_ddpm_sampler_advance(const float* tseq, int steps, int32_t* step, float* t, int nt, void* stream);
/* The bytes of torchvision save_image(x[k], path, normalize=True) for every image of a batch in one launch: x fp32 [B][3][H][W] -> out
 * uint8 [B][H][W][3], each image scaled by its OWN minimum lo and maximum hi, hi = max(hi, lo + 1e-5), then exactly the byte arithmetic
 * of sfron_rows_to_image_u8 in SFRON_IMAGE_SAVE_IMAGE mode.  One workgroup per image; B*H*W*3 < 2^31 (else SFRON_ERR_ARG, nothing
 * launched).  An image for which hi > lo does not hold after that rule (a constant image with |lo| >= 128, or no finite value), which
 * sfron_rows_to_image_u8 would refuse, gets bytes of 0. */
int sfron_images_normalize_u8(const float* x, int B, int H, int W, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ DiT guided sampling (dit_sample.hip)
 * One sampling step of DiT/diffusion/gaussian_diffusion.py behind ONE forward pass, with forward_with_cfg's guidance (DiT/models.py:250-266)
 * folded in.  fp32, 64-bit element offsets, one launch.
 *   x         [n][C][hw]
 *   model_out [rows][2C][hw]: guided != 0: rows = 2n, row i the conditional and row i + n the null pass of sample i; else rows = n.
 *             Channels 0..C-1 are epsilon, C..2C-1 the variance interpolation v.
 *   t         DEVICE int64 [n]: PER-ROW indices into the sampler table (the respaced index, as for sfron_p_sample)
 *   stab      DEVICE float [T][11]: the eight columns of sfron_p_sample's table in their order (sqrt_ac, sqrt_1m_ac, sqrt_recip_ac,
 *             sqrt_recipm1_ac, post_coef1, post_coef2, post_logvar_clipped, log_beta), then alphas_cumprod, alphas_cumprod_prev,
 *             alphas_cumprod_next: each the fp64 table value rounded once to fp32
 *   noise     [n][C][hw]; may be NULL in mode DDIM with eta == 0 and in mode DDIM_REVERSE (NULL counts as zeros)
 *   sample    [n][C][hw] (may be x: an element is read before it is written, by the same thread); sample_dup (may be NULL) receives the same
 *             values -- the second half of the next guided model input; pred_xstart may be NULL.
 * Guidance (guided != 0): epsilon channels < n_guided become u + s * (c - u) (c = conditional, u = null, s = cfg_scale), the expression of
 * sfron_cfg_combine; epsilon channels >= n_guided and every variance channel are the conditional row's -- the reference's quirk of guiding
 * three channels only, which the first half of its batch then carries.
 * Variance, pred_xstart = sra * x - srm1 * eps and its clamp to [-1, 1] (clip_denoised) are sfron_p_sample's expressions.
 *   SFRON_DIT_SAMPLE_DDPM          sfron_p_sample's update: sample = (c1 * pred + c2 * x) + ((t != 0) * exp(0.5 * log_var)) * noise
 *   SFRON_DIT_SAMPLE_DDIM          ddim_sample (:513-560), in the reference's operation order:
 *                                    eps = (sra * x - pred) / srm1                     (re-derived, also without the clamp)
 *                                    sigma = eta * sqrt((1 - ab_prev) / (1 - ab)) * sqrt(1 - ab / ab_prev)
 *                                    sample = (pred * sqrt(ab_prev) + sqrt(1 - ab_prev - sigma * sigma) * eps) + ((t != 0) * sigma) * noise
 *   SFRON_DIT_SAMPLE_DDIM_REVERSE  ddim_reverse_sample (:562-598), eta must be 0:
 *                                    sample = pred * sqrt(ab_next) + sqrt(1 - ab_next) * eps
 * The library builds with -ffp-contract=off, so in mode DDPM the result is BIT-EQUAL, on the n rows, to sfron_cfg_combine(model_out, 2n, 2C,
 * hw, n_guided, cfg_scale) followed by sfron_p_sample on the first n rows of x / model_out / t / noise (unguided: to sfron_p_sample alone).
 * SFRON_ERR_ARG before any launch, outputs untouched, for: a null required pointer (noise where the mode needs one), a non-positive
 * extent, n_guided outside [0, C], a cfg_scale or eta that is not finite, an unknown mode, mode DDIM_REVERSE with eta != 0, a pred_xstart or
 * sample_dup that aliases x or sample (or each other), n * C * hw >= 2^31 or n > 65535 (the grid's second dimension). */
enum { SFRON_DIT_SAMPLE_DDPM = 0, SFRON_DIT_SAMPLE_DDIM = 1, SFRON_DIT_SAMPLE_DDIM_REVERSE = 2 };
int sfron_dit_sample_step(const float* x, const float* model_out, const int64_t* t, const float* stab, const float* noise, int n, int c,
                          int hw, int guided, int n_guided, float cfg_scale, int mode, float eta, int clip_denoised, float* sample,
                          float* sample_dup, float* pred_xstart, void* stream);
/* The step counter of a DiT sampling loop, one workgroup: k = *step clamped into [0, steps); i = order[min(k + 1, steps - 1)] clamped into
 * [0, map_len); t_idx[0 .. n) = i (the table index sfron_dit_sample_step reads at the next step); t_model[0 .. rows) = timestep_map[i] (the
 * ORIGINAL timestep the DiT engine reads, respace.py:117-129); *step = k + 1.  order (int64 [steps]) and timestep_map (int64 [map_len])
 * are DEVICE tables: the host uploads nothing per step.  A launch of its own behind the step kernel, for the reason given at
 * sfron_ddpm_sampler_advance.  SFRON_ERR_ARG before any launch for a null pointer or a non-positive extent. */
int sfron_dit_sampler_advance(const int64_t* order, const int64_t* timestep_map, int steps, int map_len, int32_t* step, int64_t* t_idx, int n,
                              int64_t* t_model, int rows, void* stream);

/* ------------------------------------------------------------------ DiT likelihood evaluation (dit_bpd.hip)
 * One term of calc_bpd_loop (DiT/diffusion/gaussian_diffusion.py:805-858) for the LEARNED_RANGE / EPSILON model, forward only: nothing is
 * frozen, no gradient is written.  fp32 in the reference's operation order, 64-bit element offsets, one workgroup per sample, one launch.
 *   x0        [n][C][hw]
 *   x_t       [n][C][hw] or NULL: NULL recomputes x_t = sqrt_ac * x0 + sqrt_1m_ac * noise in registers, the expression (and, the library
 *             being built with -ffp-contract=off, the bits) of sfron_q_sample
 *   noise     [n][C][hw] this step's noise; may be NULL when x_t is given (then mse must be NULL).  One of x_t / noise is required.
 *   model_out [n][2C][hw]: channels 0..C-1 epsilon, C..2C-1 the variance interpolation v
 *   t         DEVICE int64 [n]: PER-ROW indices into tab
 *   tab       DEVICE float [T][8]: sfron_dit_loss_fwd_bwd's table
 *   vb, xstart_mse, mse   row-major [n][ld] matrices (xstart_mse and mse may be NULL); sample i's terms go to element [i][k], k = *step
 *             when step (DEVICE int32, the counter sfron_dit_sampler_advance keeps) is given, else col.  In calc_bpd_loop ld = T and
 *             column 0 is t = T - 1, as the reference stacks them.
 *     vb          mean_flat(normal_kl(true posterior, model)) / ln 2, or for a row with t == 0 the discretized decoder NLL (:699-712,
 *                 diffusion_utils.py:62-88: the 1e-12 clamp and the +-0.999 edges); pred_xstart = sqrt_recip_ac * x_t - sqrt_recipm1_ac *
 *                 eps_hat is clamped to [-1, 1] before the model mean when clip_denoised != 0, as p_mean_variance does
 *     xstart_mse  mean_flat((pred_xstart - x0)^2)
 *     mse         mean_flat((eps - noise)^2), eps = (sqrt_recip_ac * x_t - pred_xstart) / sqrt_recipm1_ac: _predict_eps_from_xstart of
 *                 the (possibly clamped) pred_xstart, NOT the raw model output
 *     The per-sample sums are accumulated and reduced in fp64 in a fixed order (no atomics): the same inputs give the same bits.
 *   pred_xstart   [n][C][hw] or NULL
 *   next_xt   [n][C][hw] or NULL.  Given (with next_noise [n][C][hw], order DEVICE int64 [steps], step, steps <= ld): when k + 1 < steps
 *             the launch also writes next_xt = sqrt_ac[i] * x0 + sqrt_1m_ac[i] * next_noise, i = order[k + 1] -- sfron_q_sample's bits, the
 *             model input of the next step, so x0 is read once per step; at the last step (k + 1 == steps) nothing is written.
 * t, *step and order live on the device, so the host cannot refuse their values: a row whose t is outside [0, T) reads no table row and
 * gets NaN terms (its pred_xstart is unspecified), a counter outside [0, ld) writes no term, an order entry outside [0, T) no next_xt.
 * SFRON_ERR_ARG before any launch, outputs untouched, for: a null required pointer (x0, model_out, t, tab, vb; both of x_t and noise; mse
 * without noise; next_xt without next_noise / order / step), a non-positive extent or T, ld <= 0, without step a col outside [0, ld), with
 * next_xt a steps outside [1, ld], n * C * hw >= 2^31 or n * ld >= 2^31, a next_xt that aliases an input or pred_xstart, a pred_xstart
 * that aliases x0, x_t or noise. */
int sfron_dit_bpd_step(const float* x0, const float* x_t, const float* noise, const float* model_out, const int64_t* t, const float* tab,
                       int T, int n, int c, int hw, int clip_denoised, float* vb, float* xstart_mse, float* mse, int ld, const int32_t* step,
                       int col, float* pred_xstart, const float* next_noise, const int64_t* order, int steps, float* next_xt, void* stream);
/* _prior_bpd (:789-803): prior_bpd[i] = mean_flat(normal_kl(sqrt_ac_last * x0, log_one_minus_ac_last, 0, 0)) / ln 2 -- the two scalars are
 * sqrt_alphas_cumprod[T - 1] and log(1 - alphas_cumprod[T - 1]), the fp64 table values rounded once to fp32, passed by value.
 * SFRON_ERR_ARG before any launch for a null pointer, a non-positive extent, n * C * hw >= 2^31 or a scalar that is not finite. */
int sfron_dit_prior_bpd(const float* x0, int n, int c, int hw, float sqrt_ac_last, float log_one_minus_ac_last, float* prior_bpd,
                        void* stream);

/* ------------------------------------------------------------------ classifier evaluation (classify.hip)
 * What the ResNet-34 / ResNet-50 forward passes of DDPM/classifier_evaluation.py and SD/eval-scripts/imageclassify.py need beside
 * sfron_conv_fwd and the GEMM.  Every entry point: SFRON_ERR_ARG before any launch for a null pointer, a non-positive extent or an
 * operand of 2 GiB or more; 64-bit element offsets; no allocation, no synchronisation.
 *
 * The im2col matrix of the 7x7 / stride 2 / pad 3 stem: img uint8 [B][H][W][3] -> bf16 rows [B * Ho * Wo][k_pad], Ho = (H + 6 - 7) / 2 + 1
 * (Wo alike).  Column (kh * 7 + kw) * 3 + c = bf16_rne((x / 255.0f - mean[c]) / std[c]) of pixel (2 ho + kh - 3, 2 wo + kw - 3), true
 * fp32 divisions (the arithmetic of sfron_image_u8_to_rows_bf16: with mean = std = 0.5 the same bits); a pixel outside the image is 0 in
 * NORMALISED space (Conv2d pads after Normalize), as are columns 147 .. k_pad - 1.  k_pad % 8 == 0, k_pad >= 152, rows 16-byte aligned. */
int sfron_image_u8_patches7(const uint8_t* img, int B, int H, int W, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                            int k_pad, uint16_t* rows, void* stream);
/* the same matrix from a float [B][3][H][W] tensor that is already normalised: bf16_rne(x) */
int sfron_nchw_patches7(const float* x, int B, int H, int W, int k_pad, uint16_t* rows, void* stream);
/* MaxPool2d(3, 2, 1) over fp32 rows [B * H * W][ld] (C channels; C % 4 == 0, ld % 4 == 0, x 16-byte aligned) -> [B * Ho * Wo][C] as bf16
 * (y_bf16), fp32 (y_f32) or both (either may be NULL, not both): the maximum over the IN-BOUNDS pixels of the window (padding is -inf,
 * not 0), then, with relu != 0, clamped at 0 -- ReLU and the pool commute. */
int sfron_relu_maxpool3s2(const float* x, int ld, int B, int H, int W, int C, int relu, uint16_t* y_bf16, float* y_f32, void* stream);
/* max(x, 0) of fp32 rows [rows][ld] (C % 4 == 0, ld % 4 == 0): y_f32 [rows][ld] (may be x), y_bf16 [rows][C], or both. -0.0 stays -0.0. */
int sfron_relu_rows(const float* x, int ld, int64_t rows, int C, uint16_t* y_bf16, float* y_f32, void* stream);
/* AdaptiveAvgPool2d(1) + Linear in fp32: pooled[b][c] = (sum over the HW rows of sample b, in row order) / HW; logits[b][n] =
 * sum_c w[n][c] * pooled[b][c] + bias[n] (bias may be NULL).  x fp32 rows [B * HW][ld], w fp32 [n_cls][C] (C % 4 == 0, w and pooled 16-byte
 * aligned), pooled fp32 [B][C] (written), logits fp32 [B][n_cls].  A fixed summation order: the same call gives the same bits. */
int sfron_pool_fc(const float* x, int ld, int B, int HW, int C, const float* w, const float* bias, int n_cls, float* pooled, float* logits,
                  void* stream);
/* Per row of logits [B][ld] (n_cls used), one workgroup each: probs [B][n_cls] = softmax; entropy [B] = -sum p log p where a term with
 * p == 0 counts as 0; p_target [B] = p[target]; argmax [B]; topk_p / topk_i [B][topk] = the topk <= 8 largest probabilities and their
 * indices, descending, equal values by the lower index.  Every output is optional (NULL), topk_p and topk_i only when topk == 0. */
int sfron_classify_metrics(const float* logits, int ld, int B, int n_cls, int target, int topk, float* probs, float* entropy, float* p_target,
                           int32_t* argmax, float* topk_p, int32_t* topk_i, void* stream);

/* ------------------------------------------------------------------ DDPM training batches from a resident dataset (ddpm_data.hip)
 * One launch makes the inputs of a DDPMSFRon stage from a uint8 dataset that lives on the device: what DataLoader's collate, the
 * upload, ToTensor, RandomHorizontalFlip, data_transform (DDPM/dataset/__init__.py:241-255) and the antithetic timestep draw
 * (DDPM/runners/diffusion.py) do per batch on the host.
 *   images ... uint8 [N][C][H][W];  labels int64 [N]
 *   idx ...... DEVICE int64 [B]: image b of the batch is images[idx[b]]
 *   flip ..... DEVICE uint8 [B] or NULL: non-zero mirrors image b left to right (x0[.., w] = image[.., W - 1 - w])
 *   u, n ..... fp32 [B][C][H][W], the torch.rand_like / torch.randn_like draws; read only when uniform_deq / gaussian_deq != 0
 *   mode ..... SFRON_DDPM_DATA_PLAIN, _RESCALED (2 X - 1) or _LOGIT (logit_transform, lam = 1e-6)
 *   image_mean fp32 [C][H][W] or NULL (subtracted last)
 *   t_half ... DEVICE int64 [B / 2 + 1] with t int64 [B], or both NULL: t = cat(t_half, T - t_half - 1)[:B]
 *   x0 fp32 [B][C][H][W], c int64 [B] = labels[idx[b]]
 * Arithmetic: fp32, one IEEE operation per torch op in the reference's order and no contraction: X = byte / 255 (a correctly rounded
 * division), X / 256 * 255 + u / 256, X + n * 0.01f, 2 X - 1 or lam + (1 - 2 lam) X followed by log(X) - log1p(-X), X - mean.  Every form
 * but _LOGIT gives the bits of the torch expression; _LOGIT differs from it by the error of the device's logf / log1pf.
 * idx is device data and cannot be refused: an idx[b] outside [0, N) reads nothing, its x0 row becomes NaN and c[b] = -1.
 * When W % 4 == 0 and images / u / n / image_mean / x0 are 4 / 16-byte aligned a lane moves four pixels (one dword in, 16 bytes out);
 * any other width or alignment takes a one-pixel path with the same bits.  64-bit offsets.
 * SFRON_ERR_ARG before any launch, outputs untouched: a null required pointer (images, labels, idx, x0, c; u or n where its flag is
 * set; one of t_half / t without the other), a non-positive N, C, H, W or B, B * C * H * W >= 2^31, T <= 0, an unknown mode. */
enum { SFRON_DDPM_DATA_PLAIN = 0, SFRON_DDPM_DATA_RESCALED = 1, SFRON_DDPM_DATA_LOGIT = 2 };
int sfron_ddpm_batch_u8(const uint8_t* images, const int64_t* labels, int64_t N, int C, int H, int W, const int64_t* idx,
                        const uint8_t* flip, int B, int uniform_deq, const float* u, int gaussian_deq, const float* n, int mode,
                        const float* image_mean, const int64_t* t_half, int T, float* x0, int64_t* c, int64_t* t, void* stream);

/* ------------------------------------------------------------------ FID Inception-v3 and feature statistics (inception.hip)
 * What the forward pass of the FID Inception-v3 (inception.py) and the Frechet distance (fid.py) need beside sfron_conv_fwd, the batched
 * GEMM and sfron_relu_rows.  Every entry point: SFRON_ERR_ARG before any launch for a null pointer, a non-positive extent or an operand
 * of 2 GiB or more; 64-bit element offsets; no allocation, no synchronisation.
 *
 * The im2col matrix of a general convolution: bf16 NHWC rows x [B * H * W][ld] (C channels used) -> bf16 rows [B * Ho * Wo][kh * kw * C],
 * Ho = (H + 2 pad_h - kh) / stride + 1 (Wo alike); columns (i * kw + j) * C .. + C - 1 = pixel (ho * stride + i - pad_h, wo * stride + j -
 * pad_w), zero outside the image.  Pure data movement: the bits of x.  C % 8 == 0, ld % 8 == 0, x and rows 16-byte aligned, kh, kw <= 7,
 * stride 1 or 2, pad_h < kh, pad_w < kw. */
int sfron_patch_rows(const uint16_t* x, int ld, int B, int H, int W, int C, int kh, int kw, int stride, int pad_h, int pad_w, uint16_t* rows,
                     void* stream);
/* TF1's legacy tf.image.resize_bilinear(align_corners=False) of uint8 [B][H][W][3] to Ho x Wo, then (v - 128) / 128, as bf16 rows
 * [B * Ho * Wo][c_pad] (c_pad == 8: channels 0..2, then zeros -- what sfron_patch_rows reads).  src = dst * (in / out) with no half-pixel
 * offset, lo = floor(src), hi = min(lo + 1, in - 1), frac = src - lo; fp32 throughout, one IEEE operation per step, in this order:
 *   top = tl + (tr - tl) * fx;  bot = bl + (br - bl) * fx;  v = top + (bot - top) * fy;  y = (v - 128) / 128;  rows = bf16_rne(y). */
int sfron_resize_tf1_u8(const uint8_t* img, int B, int H, int W, int Ho, int Wo, int c_pad, uint16_t* rows, void* stream);
/* 3x3 pools over NHWC rows x [B * H * W][ld] (C channels; fp32, or bf16 with x_bf16 != 0) -> y [B * Ho * Wo][ld_out] (fp32, or bf16 with
 * y_bf16 != 0): ld_out > C writes a column slice of a wider (concatenated) row.  C, ld, ld_out % 4 == 0; fp32 operands 16-byte, bf16
 * operands 8-byte aligned.
 *   SFRON_POOL_MAX_S2  MaxPool2d(3, 2): stride 2, no padding, floor mode (H, W >= 3)
 *   SFRON_POOL_MAX_S1  MaxPool2d(3, 1, 1): padding counts as -inf
 *   SFRON_POOL_AVG_S1  AvgPool2d(3, 1, 1, count_include_pad=False): the window's in-bounds values summed in fp64, rounded to fp32 once,
 *                      divided in fp32 by their number (4 in a corner, 6 on an edge, 9 inside) */
enum { SFRON_POOL_MAX_S2 = 0, SFRON_POOL_MAX_S1 = 1, SFRON_POOL_AVG_S1 = 2 };
int sfron_pool3(const void* x, int x_bf16, int ld, int B, int H, int W, int C, int kind, void* y, int y_bf16, int ld_out, void* stream);
/* y[b][c] = (sum over the HW rows of sample b, in row order, in fp32) / HW -> fp32 [B][C]: the same call gives the same bits */
int sfron_global_avgpool(const void* x, int x_bf16, int ld, int B, int HW, int C, float* y, void* stream);
/* np.mean(x, axis=0) and np.cov(x, rowvar=False) of fp32 activations x [N][ld] (D columns) in fp64: mu[d] = (sum_n x[n][d]) / N, then
 * sigma[i][j] = (sum_n (x[n][i] - mu[i]) (x[n][j] - mu[j])) * (1 / (N - 1)) -- two passes, centred, numpy's reciprocal factor.  Every
 * output element has one owning thread that adds its terms in a fixed order: the same call gives the same bits; sigma is symmetric bit
 * for bit.  N >= 2, D % 4 == 0, D <= 2048, ld % 4 == 0, x 16-byte aligned; mu fp64 [D] and sigma fp64 [D][D] are both written. */
int sfron_feature_stats(const float* x, int64_t N, int D, int ld, double* mu, double* sigma, void* stream);

/* ------------------------------------------------------------------ precision / recall and the Inception Score (manifold.hip)
 * DDPM/evaluator.py's ManifoldEstimator / DistanceBlock and compute_inception_score over one fp32 NT tile kernel on the exact fp32-input
 * matrix core instruction.  Every dot product is a blocked sum in one fixed order -- the products of 128 consecutive k are a k-ordered
 * fmaf chain from 0 (one rounding per product), the block sums are added in block order -- the same order wherever the element falls in
 * a tile, so the same rows give the same bits at any position, in any batch, and the error is a blocked product's, not a K-long chain's.  Operands are fp32 rows [n][ld] holding D columns:
 * D % 4 == 0, ld % 4 == 0, ld >= D, 16-byte aligned, under 2 GiB.  Every entry point: SFRON_ERR_ARG before any launch, outputs
 * untouched, for a null pointer, a misaligned operand, a non-positive extent, an operand of 2 GiB or more or a workspace that is too
 * small; no allocation, no synchronisation, no scratch.
 *
 * C[i][j] = sum_k A[i][k] * B[j][k]: A [M][lda], B [N][ldb], K columns each, C fp32 [M][ldc] (4-byte aligned, ldc >= N, any N). */
int sfron_gemm_nt_f32(const float* A, int M, int lda, const float* B, int N, int ldb, int K, float* C, int ldc, void* stream);
/* radii[i][a] = the nhood[a]-th smallest of d(i, .) over ALL N rows, i itself included (its distance is exactly 0):
 * np.partition(row, arange(kmax + 1))[nhood].  d(i, j) = max((n_i - 2 dot(i, j)) + n_j, 0) in fp32, the reference's fp32 branch, n = the
 * squared row norm summed in the product's own blocked order (so d(i, i) is exactly 0).  nhood: HOST array of n_nhood (1 .. 4) sizes, each 1 .. 7; N > max(nhood) (np.partition
 * raises there).  radii fp32 [N][n_nhood].  The N x N matrix is never stored: a query keeps its 8 smallest distances in registers and
 * only those go through the workspace (sfron_manifold_radii_workspace bytes, 16-byte aligned; contents undefined before and after).
 * _batched runs the reference's schedule -- queries row_batch at a time against col_batch candidates per launch -- with the same bits
 * as the one-batch form (a batch size <= 0 or > N means N).  The 2 GiB rule applies to a batch of rows, the operand of a launch: X as a
 * whole may be larger. */
int64_t sfron_manifold_radii_workspace(int64_t N, int64_t row_batch, int64_t col_batch);
int sfron_manifold_radii(const float* X, int64_t N, int D, int ld, const int* nhood, int n_nhood, float* radii, void* workspace,
                         int64_t workspace_bytes, void* stream);
int sfron_manifold_radii_batched(const float* X, int64_t N, int D, int ld, int64_t row_batch, int64_t col_batch, const int* nhood, int n_nhood,
                                 float* radii, void* workspace, int64_t workspace_bytes, void* stream);
/* DistanceBlock.less_thans fused into the tile, set 1 as U: with d(i, j) = max((n1_i - 2 dot) + n2_j, 0),
 *   in1[i][b] |= any_j d(i, j) <= r2[j][b]      in2[j][a] |= any_i d(i, j) <= r1[i][a]
 * r1 fp32 [N1][K1], r2 fp32 [N2][K2] (K1, K2 in 1 .. 4; 4-byte aligned), in1 uint8 [N1][K2], in2 uint8 [N2][K1], zeroed by the caller
 * (or carrying the flags of earlier calls on other row ranges): a flag is only ever turned on, so the result does not depend on order. */
int sfron_manifold_pr(const float* X1, int64_t N1, const float* r1, int K1, const float* X2, int64_t N2, const float* r2, int K2, int D, int ld1,
                      int ld2, uint8_t* in1, uint8_t* in2, void* stream);
/* Per split of split_size rows of logits [N][ld] (C used; the last split may be short), three launches: the rows' softmax in fp32
 * (exp(x - max) / sum, IN PLACE: logits holds the probabilities afterwards), the column means over the split in fp64, and
 * scores[s] = exp((1 / n) sum_i sum_c p (log p - log mean_c)) in fp64.  A probability that underflowed to 0 contributes 0, its limit (the
 * rule of sfron_classify_metrics' entropy; numpy gives NaN there).  scores fp64 [ceil(N / split_size)]; workspace of
 * sfron_inception_score_workspace bytes, 16-byte aligned.  Fixed summation orders: the same call gives the same bits. */
int64_t sfron_inception_score_workspace(int64_t N, int C, int split_size);
int sfron_inception_score(float* logits, int64_t N, int C, int ld, int split_size, double* scores, void* workspace, int64_t workspace_bytes,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFRON_H */
