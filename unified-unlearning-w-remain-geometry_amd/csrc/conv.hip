// Convolutions of the U-Net building blocks (DDPM Conditional_Model; the same blocks serve the LDM UNetModel) and the batched GEMM.
//
// Replaces, for /root/reference/DDPM/models/diffusion.py:
//   Conv2d 3x3 / 1x1 forward, input gradient and weight gradient (:49-82 Upsample / Downsample, :85-145 ResnetBlock,
//   :148-192 AttnBlock, :283-327 conv_in / conv_out)              -> k_bgemm: implicit-GEMM convolution on NHWC bf16
//   single-head attention bmm (:168-186)                          -> batched k_bgemm (its softmax: rows.hip)
//   nearest-neighbour upsampling (:56-57) and the (0,1,0,1) pad + stride-2 conv (:76-80) are address arithmetic of the
//   im2col loader (no copies).
// GroupNorm lives in groupnorm.hip; layouts, softmax, LayerNorm, GEGLU, casts, dropout masks and the embeddings in rows.hip.
//
// Activations are NHWC: a [B*H*W][C] row-major matrix, so a 3x3 convolution is the GEMM
//   Y[p][co] = sum_{tap, ci} X[src(p, tap)][ci] * W[co][tap][ci]
// whose A operand is never materialised: the staging loader computes src(p, tap) (stride, padding, nearest-upsampled or
// zero-dilated source) per 16-byte chunk and zero-fills what falls outside the image.
//   forward   A = X (im2col),  B = W   [Cout][taps*Cin]
//   dgrad     A = dY (im2col, flipped taps; stride-2 convs read a zero-dilated dY),  B = W^T re-laid [Cin][taps*Cout]
//   wgrad     A = dY^T [pixels][Cout] (transposed read),  B = X (im2col, transposed read)  -> fp32 [Cout][taps*Cin]
// Tile 128x128x64, 4 waves, mfma_f32_16x16x32_bf16 issued as D^T = B^T A^T (lane owns 4 consecutive output columns), LDS
// images XOR-swizzled as in gemm.hip (tile.h).  The U-Net is 5 % of the DiT step's FLOPs per sample: k_bgemm is the generic
// (register-staged) tile; k_cgemm / k_cgemm_t below are the LDS-DMA pipeline for the shapes that qualify.
#include "common.h"
#include "tile.h"
#include <atomic>
#include <cstdlib>
#include "../../include/sfron.h"
#include "unet_host.h"

namespace {

struct ConvGeom {
  int Hs, Ws, C;          // source image (per sample) and its channel count
  int Ho, Wo;             // output grid that indexes the GEMM rows (forward output pixels / dgrad input pixels)
  int stride, pad;
  int up;                 // source is read through a nearest x2 upsampling (virtual extent 2Hs x 2Ws)
  int dil;                // source is read as a zero-dilated x2 image (transposed stride-2 convolution)
  int taps;               // 9 or 1
  int flip;               // dgrad: tap index runs over the flipped kernel (the weights were re-laid to match)
};

struct BGemmArgs {
  const __bf16* A; const __bf16* B;
  int M, N, K, lda, ldb;
  long sA, sB, sC;        // batch strides (elements); grid.y = batch
  long sA2, sB2, sC2;     // inner batch strides; grid.z = inner batch (attention heads: column offsets inside one matrix)
  __bf16* Cb; int ldcb;
  float* Cf; int ldcf;
  const float* bias;      // [N] or null
  const float* resid;     // [M][ldcf] fp32 added to the result, or null
  const float* vec;       // per-sample row vector vec[(row / T) * ldvec + col], or null
  int ldvec, T;
  float alpha;
  int accumulate;
  int kchunk;             // split-K (weight gradients: few output tiles, a contraction over all pixels): grid.y = split, split s
                          // takes k in [s * kchunk, (s + 1) * kchunk) and writes its own fp32 slab Cf + s * sC (0 = no split)
  int ksplit;             // split-K of a BATCHED product (k_bgemm only): grid.x = tiles * ksplit; split s of batch (y, z) writes the
                          // contiguous fp32 slab Cf[((s * gridDim.y + y) * gridDim.z + z)][M][N]; k_bsplit_finish adds the splits
  ConvGeom cg;
};

constexpr int BM = 128, BN = 128, BK = 64, NT = 256, TILE_ELEMS = 128 * 64;
enum { EPI_BF16 = 0, EPI_RES = 1 };
enum { CONV_NONE = 0, CONV_A = 1, CONV_B = 2 };

// source pixel (row index of the NHWC matrix) of output pixel (b, ho, wo) under tap `tap`; false = zero padding
__device__ __forceinline__ bool conv_src(const ConvGeom& c, int b, int ho, int wo, int tap, int& pix) {
  int kh = 0, kw = 0;
  if (c.taps == 9) { kh = tap / 3; kw = tap - 3 * kh; }
  int hi = ho * c.stride + kh - c.pad, wi = wo * c.stride + kw - c.pad;
  const int Hv = (c.up | c.dil) ? 2 * c.Hs : c.Hs, Wv = (c.up | c.dil) ? 2 * c.Ws : c.Ws;
  if (hi < 0 || wi < 0 || hi >= Hv || wi >= Wv) return false;
  if (c.dil) { if ((hi | wi) & 1) return false; }
  if (c.up | c.dil) { hi >>= 1; wi >>= 1; }
  pix = (b * c.Hs + hi) * c.Ws + wi;
  return true;
}

// ---- global -> register staging (128 x 64 direct image or 64 x 128 transposed-read image, 4 chunks of 16 B per thread)
template <bool TR, bool CONV>
struct Stager {
  const __bf16* P;
  int ld, dim;
  int lds_off[4];
  // plain: element offset of the chunk at k = 0 (direct: row * ld + ch * 8; TR: col), validity
  long base[4];
  bool valid[4];
  // conv direct: (b, ho, wo) of the 4 rows, k offset of this thread's chunk; conv TR: (tap, ci) of the 4... one column chunk
  int pb[4], ph[4], pw[4];
  int kch;                 // direct: k offset inside the tile (same for the 4 chunks); TR: first k-row of the thread
  int tap, ci;             // conv TR: fixed per thread
  __device__ __forceinline__ void init(const __bf16* P_, int ld_, int dim_, int d0, int tid, const ConvGeom& cg) {
    P = P_; ld = ld_; dim = dim_;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + NT * i;
      if (!TR) {
        const int row = c >> 3, ch = c & 7;
        const int gr = d0 + row;
        valid[i] = gr < dim;
        lds_off[i] = off_direct(row, ch);
        kch = ch * 8;
        if (!CONV) base[i] = (long)(valid[i] ? gr : 0) * ld + ch * 8;
        else {
          const int g2 = valid[i] ? gr : 0;
          pw[i] = g2 % cg.Wo; const int t = g2 / cg.Wo; ph[i] = t % cg.Ho; pb[i] = t / cg.Ho;
        }
      } else {
        const int krow = c >> 4, ch = c & 15;
        const int col = d0 + ch * 8;
        valid[i] = col < dim;
        lds_off[i] = off_tr(krow, ch);
        if (i == 0) kch = krow;
        if (!CONV) base[i] = (long)krow * ld + (valid[i] ? col : 0);
        else { const int cc = valid[i] ? col : 0; tap = cc / cg.C; ci = cc - tap * cg.C; }
      }
    }
  }
  __device__ __forceinline__ void load(uint4 (&r)[4], int k0, int K, const ConvGeom& cg) const {
    const uint4 z = make_uint4(0, 0, 0, 0);
    if (!TR) {
      const int k = k0 + kch;
      int t = 0, c0 = 0;
      if (CONV) { t = k / cg.C; c0 = k - t * cg.C; if (cg.flip) t = cg.taps - 1 - t; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bool ok = valid[i] && k < K;
        const __bf16* p = P;
        if (!CONV) p = P + base[i] + k0;
        else {
          int pix = 0;
          ok = ok && conv_src(cg, pb[i], ph[i], pw[i], t, pix);
          p = P + (long)pix * ld + c0;
        }
        r[i] = ok ? *reinterpret_cast<const uint4*>(p) : z;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kr = k0 + kch + 16 * i;            // contraction index = token / pixel row
        bool ok = valid[i] && kr < K;
        const __bf16* p = P;
        if (!CONV) p = P + base[i] + (long)k0 * ld;
        else {
          const int kk = ok ? kr : 0;
          const int wo = kk % cg.Wo; const int t2 = kk / cg.Wo; const int ho = t2 % cg.Ho; const int b = t2 / cg.Ho;
          int pix = 0;
          ok = ok && conv_src(cg, b, ho, wo, tap, pix);
          p = P + (long)pix * ld + ci;
        }
        r[i] = ok ? *reinterpret_cast<const uint4*>(p) : z;
      }
    }
  }
  __device__ __forceinline__ void store(__bf16* img, const uint4 (&r)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(img + lds_off[i]) = r[i];
  }
};

template <int EPI>
__device__ __forceinline__ void epi_store(const BGemmArgs& g, int row, int col, f32x4 v) {
  v = v * g.alpha;
  if (g.bias) { const float4 b = *reinterpret_cast<const float4*>(g.bias + col); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
  if (EPI == EPI_BF16) {
    bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    *reinterpret_cast<bf16x4*>(g.Cb + (size_t)row * g.ldcb + col) = o;
  } else {
    if (g.vec) { const float4 b = *reinterpret_cast<const float4*>(g.vec + (size_t)(row / g.T) * g.ldvec + col); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
    if (g.resid) { const float4 b = *reinterpret_cast<const float4*>(g.resid + (size_t)row * g.ldcf + col); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
    float4* dst = reinterpret_cast<float4*>(g.Cf + (size_t)row * g.ldcf + col);
    float4 o = make_float4(v[0], v[1], v[2], v[3]);
    if (g.accumulate) { const float4 c = *dst; o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w; }
    *dst = o;
  }
}

}  // namespace

template <bool A_TR, bool B_TR, int EPI, int CONV>
__global__ __launch_bounds__(NT) void k_bgemm(BGemmArgs g) {
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  __bf16* sA = smem;
  __bf16* sB = smem + 2 * TILE_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = (g.N + BN - 1) / BN;
  int tile = blockIdx.x, split = 0;
  if (g.ksplit > 1) { const int nt = ((g.M + BM - 1) / BM) * ntn; split = tile / nt; tile -= split * nt; }
  const int tm = tile / ntn, tn = tile % ntn;
  const int m0 = tm * BM, n0 = tn * BN;
  const long bz = blockIdx.y, bi = blockIdx.z;
  int kbeg = 0, kend = g.K;
  if (g.ksplit > 1) { kbeg = split * g.kchunk; kend = min(g.K, kbeg + g.kchunk); g.A += bz * g.sA; g.B += bz * g.sB; }
  else if (g.kchunk > 0) { kbeg = (int)bz * g.kchunk; kend = min(g.K, kbeg + g.kchunk); }
  else { g.A += bz * g.sA; g.B += bz * g.sB; }
  g.A += bi * g.sA2; g.B += bi * g.sB2;
  if (g.ksplit > 1) {
    g.Cf += (((long)split * gridDim.y + bz) * gridDim.z + bi) * ((long)g.M * g.N);
  } else {
    const long co = bz * g.sC + bi * g.sC2;
    if (g.Cb) g.Cb += co;
    if (g.Cf) g.Cf += co;
    if (g.resid) g.resid += co;
  }

  Stager<A_TR, CONV == CONV_A> stA;
  Stager<B_TR, CONV == CONV_B> stB;
  stA.init(g.A, g.lda, g.M, m0, tid, g.cg);
  stB.init(g.B, g.ldb, g.N, n0, tid, g.cg);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (kend - kbeg + BK - 1) / BK;
  uint4 ra[4], rb[4];
  stA.load(ra, kbeg, kend, g.cg);
  stB.load(rb, kbeg, kend, g.cg);
  stA.store(sA, ra);
  stB.store(sB, rb);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) {
      stA.load(ra, kbeg + (kt + 1) * BK, kend, g.cg);
      stB.load(rb, kbeg + (kt + 1) * BK, kend, g.cg);
    }
    const __bf16* iA = sA + cur * TILE_ELEMS;
    const __bf16* iB = sB + cur * TILE_ELEMS;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        if (!A_TR) fa[mt] = frag_direct(iA, wm * 64 + mt * 16 + (lane & 15), ks * 4 + (lane >> 4));
        else       fa[mt] = frag_tr(iA, wm * 64 + mt * 16, ks * 32, lane);
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        if (!B_TR) fb[nt] = frag_direct(iB, wn * 64 + nt * 16 + (lane & 15), ks * 4 + (lane >> 4));
        else       fb[nt] = frag_tr(iB, wn * 64 + nt * 16, ks * 32, lane);
      }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[nt], fa[mt], acc[mt][nt], 0, 0, 0);
    }
    if (more) {
      stA.store(sA + (cur ^ 1) * TILE_ELEMS, ra);
      stB.store(sB + (cur ^ 1) * TILE_ELEMS, rb);
    }
    __syncthreads();
  }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int row = m0 + wm * 64 + mt * 16 + (lane & 15);
    if (row >= g.M) continue;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int col = n0 + wn * 64 + nt * 16 + 4 * (lane >> 4);
      if (col >= g.N) continue;
      epi_store<EPI>(g, row, col, acc[mt][nt]);
    }
  }
}

template __global__ void k_bgemm<false, false, EPI_BF16, CONV_NONE>(BGemmArgs);
template __global__ void k_bgemm<false, false, EPI_RES, CONV_NONE>(BGemmArgs);
template __global__ void k_bgemm<false, true, EPI_BF16, CONV_NONE>(BGemmArgs);
template __global__ void k_bgemm<false, true, EPI_RES, CONV_NONE>(BGemmArgs);
template __global__ void k_bgemm<true, true, EPI_BF16, CONV_NONE>(BGemmArgs);
template __global__ void k_bgemm<true, true, EPI_RES, CONV_NONE>(BGemmArgs);
template __global__ void k_bgemm<false, false, EPI_BF16, CONV_A>(BGemmArgs);
template __global__ void k_bgemm<false, false, EPI_RES, CONV_A>(BGemmArgs);
template __global__ void k_bgemm<true, true, EPI_RES, CONV_B>(BGemmArgs);

// =================================================================================================
// LDS-DMA pipelined tile for the large direct-operand products (3x3 / 1x1 convolution forward and input gradient, Linear forward):
// 256 x (NT_ * 16) x 64, 8 waves as 4 x 2 (64 x NT_*8 each), THREE LDS slots (two K-tiles in flight per CU, the
// operands of a U-Net pass are cold in L2), operands staged by `buffer_load_dwordx4 ... lds` with the XOR swizzle applied on the
// SOURCE address (the LDS image is lane-linear).  The im2col gather is address arithmetic of the A-operand DMA: a lane owns four
// output pixels (b, ho, wo); per K-tile the tap (kh, kw) and the channel offset are wave-uniform (C % 64 == 0), the lane adds the
// tap to its pixel, and a source outside the image (zero padding, odd positions of a zero-dilated gradient) becomes an
// out-of-range buffer offset, for which the DMA writes zeros.  NT_ = 10 (160 columns) tiles the 320 / 640 / 1280-wide outputs of
// the LDM UNet exactly, NT_ = 8 serves the DDPM widths (128 / 256) and ragged N (rows of B past N read as zeros through the
// descriptor's size, the epilogue skips their columns).  Needs M % 256 == 0 and K % 64 == 0; everything else stays on k_bgemm.
template <int NT_>
struct CTile {
  static constexpr int FBM = 256, FBN = NT_ * 16, NW = 8, NSLOT = 3;
  static constexpr int A_ELEMS = FBM * 64, B_ELEMS = FBN * 64, SLOT = A_ELEMS + B_ELEMS;
  static constexpr int NA = FBM * 8 / 64 / NW;           // A wave-instructions per wave and tile (4)
  static constexpr int NB_TOT = FBN * 8 / 64;            // B wave-instructions per tile
  static constexpr int NB = (NB_TOT + NW - 1) / NW;
  static constexpr bool EVEN = NB_TOT % NW == 0;         // NT_ = 10: 20 instructions on 8 waves -- waves 4..7 send a no-op third
  static constexpr int NDMA = NA + NB;
  static constexpr size_t LDS = (size_t)NSLOT * SLOT * sizeof(__bf16) + (EVEN ? 0 : 1024);
};

// NL > 0: NL extra waves (8 .. 8 + NL - 1) issue every LDS-DMA and do the im2col address arithmetic; the 8 MFMA waves only wait at
// the barrier (the loader / consumer split of gemm.hip k_gemm_pipe)
template <int NT_, int EPI, bool CONV, int NL = 0>
__global__ __launch_bounds__(512 + 64 * NL) void k_cgemm(BGemmArgs g, unsigned a_bytes, unsigned b_bytes) {
  using CT = CTile<NT_>;
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = (g.N + CT::FBN - 1) / CT::FBN;
  // workgroups of one XCD (blockIdx % 8) take consecutive tile ids: the column tiles of one row panel share that XCD's L2
  int id;
  {
    const int nblk = gridDim.x, b = blockIdx.x, q = nblk >> 3, r = nblk & 7, x = b & 7, y = b >> 3;
    id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + y;
  }
  const int tm = id / ntn, tn = id - tm * ntn;
  const int m0 = tm * CT::FBM, n0 = tn * CT::FBN;
  int kbeg = 0, kend = g.K;
  if (g.kchunk > 0) {
    kbeg = (int)blockIdx.y * g.kchunk; kend = min(g.K, kbeg + g.kchunk);
    const long co = (long)blockIdx.y * g.sC;
    if (g.Cf) g.Cf += co;
  }
  const int nk = (kend - kbeg) / BK;

  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)g.A, 0, (int)a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)g.B, 0, (int)b_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)g.B, 0, 0, 0x00020000);
  __bf16* dummy = smem + CT::NSLOT * CT::SLOT;

  constexpr int NWD = NL ? NL : CT::NW;                       // waves that issue DMA
  constexpr int NA_ = CT::FBM * 8 / 64 / NWD, NB_ = (CT::NB_TOT + NWD - 1) / NWD, NDMA_ = NA_ + NB_;
  constexpr bool EVEN_ = CT::NB_TOT % NWD == 0;
  static_assert(NL == 0 || EVEN_, "loader waves: no dummy slot");
  const bool loader = NL && wave >= CT::NW;
  const int dwave = NL ? (wave - CT::NW) & (NWD - 1) : wave;
  const int lc8 = ((lane & 7) ^ ((lane >> 3) & 7)) << 3;      // logical 8-element chunk this lane fetches (rows start at multiples of 8)
  int a_off[NA_], a_h0[NA_], a_w0[NA_], a_pb[NA_], b_off[NB_];
#pragma unroll
  for (int i = 0; i < NA_; ++i) {
    const int gr = m0 + (dwave + i * NWD) * 8 + (lane >> 3);
    if (!CONV) a_off[i] = 2 * (gr * g.lda + lc8);
    else {
      const int wo = gr % g.cg.Wo, t = gr / g.cg.Wo, ho = t % g.cg.Ho, b = t / g.cg.Ho;
      a_h0[i] = ho * g.cg.stride - g.cg.pad; a_w0[i] = wo * g.cg.stride - g.cg.pad; a_pb[i] = b * g.cg.Hs * g.cg.Ws;
    }
  }
#pragma unroll
  for (int i = 0; i < NB_; ++i) b_off[i] = 2 * ((n0 + (dwave + i * NWD) * 8 + (lane >> 3)) * g.ldb + lc8);

  const int Hv = (g.cg.up | g.cg.dil) ? 2 * g.cg.Hs : g.cg.Hs, Wv = (g.cg.up | g.cg.dil) ? 2 * g.cg.Ws : g.cg.Ws;
  // tile kt -> slot: the A source of a convolution advances tap by tap, channel block by channel block
  int tap = 0, c0 = 0;
  if (CONV) { tap = kbeg / g.cg.C; c0 = kbeg - tap * g.cg.C; }
  auto issue = [&](int slot, int k0) {
    __bf16* iA = smem + slot * CT::SLOT;
    __bf16* iB = iA + CT::A_ELEMS;
    int kh = 0, kw = 0;
    if (CONV && g.cg.taps == 9) { const int tt = g.cg.flip ? 8 - tap : tap; kh = (tt * 11) >> 5; kw = tt - 3 * kh; }
#pragma unroll
    for (int i = 0; i < NA_; ++i) {
      int voff = 0;
      if (!CONV) voff = a_off[i];
      else {
        int hi = a_h0[i] + kh, wi = a_w0[i] + kw;
        bool ok = (unsigned)hi < (unsigned)Hv && (unsigned)wi < (unsigned)Wv;
        if (g.cg.dil) ok = ok && !((hi | wi) & 1);
        if (g.cg.up | g.cg.dil) { hi >>= 1; wi >>= 1; }
        voff = ok ? 2 * ((a_pb[i] + hi * g.cg.Ws + wi) * g.lda + lc8) : 0x7ffffff0;
      }
      dma16(rsA, iA + (dwave + i * NWD) * 512, voff, 2 * (CONV ? c0 : k0));
    }
#pragma unroll
    for (int i = 0; i < NB_; ++i) {
      if (EVEN_ || i + 1 < NB_) {
        dma16(rsB, iB + (dwave + i * NWD) * 512, b_off[i], 2 * k0);
      } else {
        const bool ok = dwave + i * NWD < CT::NB_TOT;     // wave-uniform
        dma16(ok ? rsB : rs0, ok ? iB + (dwave + i * NWD) * 512 : dummy, b_off[i], 2 * k0);
      }
    }
    if (CONV) { c0 += BK; if (c0 >= g.cg.C) { c0 = 0; ++tap; } }
  };

  // 4 x 2 waves of 64 x (NT_ / 2 * 16): per K-step a wave reads (4 + NT_ / 2) fragments for 4 * NT_ / 2 MFMAs -- a quarter less LDS traffic
  // per FLOP than 8 x 1 waves of 32 x NT_ * 16 (measured 6-7 % on every shape, tools/probes/persist_gemm_probe.hip)
  constexpr int WNT = NT_ / 2;
  static_assert(NT_ % 2 == 0, "two wave columns");
  const int wm = wave >> 1, wn = wave & 1;
  f32x4 acc[4][WNT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fg = lane >> 4;
  auto compute = [&](int slot) {
    const __bf16* iA = smem + slot * CT::SLOT;
    const __bf16* iB = iA + CT::A_ELEMS;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) fa[mt] = frag_direct(iA, wm * 64 + mt * 16 + fr, ks * 4 + fg);
#pragma unroll
      for (int nt = 0; nt < WNT; ++nt) {
        const bf16x8 fb = frag_direct(iB, wn * WNT * 16 + nt * 16 + fr, ks * 4 + fg);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa[mt], acc[mt][nt], 0, 0, 0);
      }
    }
  };

  if (NL) {
    if (loader) {
      if (nk > 0) issue(0, kbeg);
      if (nk > 1) issue(1, kbeg + BK);
      int slot = 0;
      for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) wait_vmcnt<NDMA_>();
        else             wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + 2 < nk) issue(slot >= 1 ? slot - 1 : 2, kbeg + (kt + 2) * BK);
        slot = slot == 2 ? 0 : slot + 1;
      }
      return;
    }
    int slot = 0;
    for (int kt = 0; kt < nk; ++kt) {
      __builtin_amdgcn_s_barrier();
      compute(slot);
      slot = slot == 2 ? 0 : slot + 1;
    }
  } else {
    if (nk > 0) issue(0, kbeg);
    if (nk > 1) issue(1, kbeg + BK);
    int slot = 0;
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) wait_vmcnt<NDMA_>();
      else             wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      if (kt + 2 < nk) issue(slot >= 1 ? slot - 1 : 2, kbeg + (kt + 2) * BK);       // (kt + 2) % 3
      compute(slot);
      slot = slot == 2 ? 0 : slot + 1;
    }
  }

#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int row = m0 + wm * 64 + mt * 16 + fr;
#pragma unroll
    for (int nt = 0; nt < WNT; ++nt) {
      const int col = n0 + wn * WNT * 16 + nt * 16 + 4 * fg;
      if (col < g.N) epi_store<EPI>(g, row, col, acc[mt][nt]);
    }
  }
}

template __global__ void k_cgemm<8, EPI_BF16, false>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<8, EPI_RES, false>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<8, EPI_BF16, true>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<8, EPI_RES, true>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<10, EPI_BF16, false>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<10, EPI_RES, false>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<10, EPI_BF16, true>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<10, EPI_RES, true>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<8, EPI_BF16, false, 4>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<8, EPI_RES, false, 4>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<8, EPI_BF16, true, 4>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<8, EPI_RES, true, 4>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<10, EPI_BF16, false, 4>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<10, EPI_RES, false, 4>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<10, EPI_BF16, true, 4>(BGemmArgs, unsigned, unsigned);
template __global__ void k_cgemm<10, EPI_RES, true, 4>(BGemmArgs, unsigned, unsigned);

// ---- the same pipeline for the products with a TRANSPOSED-READ operand (contraction index = matrix row):
//   T[p][q] = sum_k P[.][.] Q[k][q],  tile 256 (p) x 128 (q) x 64 (k), 8 waves as 4 x 2 (64 x 64 each), three slots
//   P_TR = false: P direct [p][k] (Linear input gradient  dX = dY W : P = dY, Q = W [k = out][q = in])
//   P_TR = true : P read transposed [k][p] (weight gradients; contraction over pixels / tokens)
//     CONVP: P is the im2col view of an NHWC image ([k = output pixel][p = (tap, ci)]): a lane's column chunk fixes its tap, per
//            K-tile it decodes its pixel rows (magic-number division) and shifts them by the tap
//     SWAP : the result is stored transposed, C[q][p] (convolution weight gradient [Co][taps * Ci] with the 256-wide tile on
//            the long (tap, ci) axis and the 128-wide one on Co: 320 / 640 / 1280 and 128 / 256 outputs tile without waste)
// Transposed fragments are ds_read_b64_tr_b16 through inline asm (hipcc would drain vmcnt(0) before the builtin while an
// LDS-DMA is in flight, tile.h); their completion is waited for explicitly (lds_reads_done()).
struct TTile {
  static constexpr int FBP = 256, FBQ = 128, NW = 8, NSLOT = 3;
  static constexpr int P_ELEMS = FBP * 64, Q_ELEMS = FBQ * 64, SLOT = P_ELEMS + Q_ELEMS;
  static constexpr int NP = 4, NQ = 2, NDMA = NP + NQ;
  static constexpr size_t LDS = (size_t)NSLOT * SLOT * sizeof(__bf16);
};

template <bool P_TR, bool CONVP, bool SWAP, int EPI, int NL = 0>        // NL: loader waves, as k_cgemm
__global__ __launch_bounds__(512 + 64 * NL) void k_cgemm_t(BGemmArgs g, unsigned p_bytes, unsigned q_bytes, unsigned magic_w, unsigned magic_h) {
  using TT = TTile;
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wp = (wave >> 1) & 3, wq = wave & 1;
  constexpr int NWD = NL ? NL : TT::NW;                       // waves that issue DMA
  constexpr int NP_ = TT::NP * TT::NW / NWD, NQ_ = TT::NQ * TT::NW / NWD, NDMA_ = NP_ + NQ_;
  const bool loader = NL && wave >= TT::NW;
  const int dwave = NL ? (wave - TT::NW) & (NWD - 1) : wave;
  // P / Q roles: the descriptor's A is P unless SWAP (then its B -- the im2col operand -- is P and the output is stored transposed)
  const __bf16* Pp = SWAP ? g.B : g.A;
  const __bf16* Qp = SWAP ? g.A : g.B;
  const int ldp = SWAP ? g.ldb : g.lda, ldq = SWAP ? g.lda : g.ldb;
  const int NPd = SWAP ? g.N : g.M, NQd = SWAP ? g.M : g.N;        // extents of the p and q axes
  const int ntq = (NQd + TT::FBQ - 1) / TT::FBQ;
  int id;
  {
    const int nblk = gridDim.x, b = blockIdx.x, qq = nblk >> 3, r = nblk & 7, x = b & 7, y = b >> 3;
    id = (x < r ? x * (qq + 1) : r * (qq + 1) + (x - r) * qq) + y;
  }
  const int tp = id / ntq, tq = id - tp * ntq;
  const int p0 = tp * TT::FBP, q0 = tq * TT::FBQ;
  int kbeg = 0, kend = g.K;
  if (g.kchunk > 0) {
    kbeg = (int)blockIdx.y * g.kchunk; kend = min(g.K, kbeg + g.kchunk);
    if (g.Cf) g.Cf += (long)blockIdx.y * g.sC;
  }
  const int nk = (kend - kbeg) / BK;

  const __amdgpu_buffer_rsrc_t rsP = __builtin_amdgcn_make_buffer_rsrc((void*)Pp, 0, (int)p_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)Qp, 0, (int)q_bytes, 0x00020000);

  // ---- DMA plan.  Direct P image [256 p][64 k] (8 chunks per row, chunk ^= row & 7); transposed-read images [64 k][256 | 128]
  // (32 | 16 chunks per row, low four chunk bits ^= swz_tr(k row)).  Out-of-range columns of a ragged last tile read the next
  // row's data or zeros; their outputs are never stored.
  int p_off[NP_], q_off[NQ_];
  int p_kh[NP_], p_kw[NP_], p_ci[NP_];           // CONVP: tap and channel offset of the lane's column chunk (tap < 0: none)
#pragma unroll
  for (int i = 0; i < NP_; ++i) {
    const int j = dwave + i * NWD;
    if (!P_TR) {
      const int row = j * 8 + (lane >> 3);
      p_off[i] = 2 * ((p0 + row) * ldp + (((lane & 7) ^ ((lane >> 3) & 7)) << 3));
    } else {
      const int krow = 2 * j + (lane >> 5), pch = lane & 31;
      const int lc = (pch & ~15) | ((pch & 15) ^ swz_tr(krow));
      const int col = p0 + (lc << 3);
      if (!CONVP) p_off[i] = 2 * (krow * ldp + col);
      else {
        const int tap = col / g.cg.C;
        p_ci[i] = col - tap * g.cg.C;
        const int tt = tap < g.cg.taps ? tap : -64;
        const int kh = g.cg.taps == 9 ? (tt >= 0 ? (tt * 11) >> 5 : -64) : (tt >= 0 ? 0 : -64);
        p_kh[i] = kh; p_kw[i] = g.cg.taps == 9 ? tt - 3 * ((tt * 11) >> 5) : 0;
        p_off[i] = krow;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NQ_; ++i) {
    const int j = dwave + i * NWD;
    const int krow = 4 * j + (lane >> 4), pch = lane & 15;
    q_off[i] = 2 * (krow * ldq + q0 + ((pch ^ swz_tr(krow)) << 3));
  }
  const int Hv = (g.cg.up | g.cg.dil) ? 2 * g.cg.Hs : g.cg.Hs, Wv = (g.cg.up | g.cg.dil) ? 2 * g.cg.Ws : g.cg.Ws;
  auto issue = [&](int slot, int k0) {
    __bf16* iP = smem + slot * TT::SLOT;
    __bf16* iQ = iP + TT::P_ELEMS;
#pragma unroll
    for (int i = 0; i < NP_; ++i) {
      int voff = p_off[i], soff = 0;
      if (!P_TR) soff = 2 * k0;
      else if (!CONVP) soff = 2 * k0 * ldp;
      else {
        const unsigned px = (unsigned)(k0 + p_off[i]);                  // output pixel of this lane's k row
        const unsigned t = __umulhi(px, magic_w), wo = px - t * g.cg.Wo;
        const unsigned b = __umulhi(t, magic_h), ho = t - b * g.cg.Ho;
        int hi = (int)ho * g.cg.stride + p_kh[i] - g.cg.pad, wi = (int)wo * g.cg.stride + p_kw[i] - g.cg.pad;
        bool ok = (unsigned)hi < (unsigned)Hv && (unsigned)wi < (unsigned)Wv;
        if (g.cg.dil) ok = ok && !((hi | wi) & 1);
        if (g.cg.up | g.cg.dil) { hi >>= 1; wi >>= 1; }
        voff = ok ? 2 * (((int)b * g.cg.Hs * g.cg.Ws + hi * g.cg.Ws + wi) * ldp + p_ci[i]) : 0x7ffffff0;
      }
      dma16(rsP, iP + (dwave + i * NWD) * 512, voff, soff);
    }
#pragma unroll
    for (int i = 0; i < NQ_; ++i) dma16(rsQ, iQ + (dwave + i * NWD) * 512, q_off[i], 2 * k0 * ldq);
  };

  // ---- fragment addresses (bytes, relative to the slot): transposed-read fragments of 16 columns x 32 k
  const int fg = lane >> 4, fi = lane & 15, fq = fi >> 2, fp = fi & 3;
  const int r0 = 8 * fg + fq;                               // k row (+4 for the upper half, + 32 for the second k-step)
  const int sw_lo = swz_tr(r0), sw_hi = swz_tr(r0 + 4);
  unsigned pa[4][2], qa[4][2];                              // P: [mt][lo/hi] (direct P: [.][k-step]); Q: [nt][lo/hi]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (P_TR) {
      const int ch = ((wp * 64 + t * 16) >> 3) + (fp >> 1);
      pa[t][0] = 2 * (r0 * 256 + (((ch & ~15) | ((ch & 15) ^ sw_lo)) << 3) + 4 * (fp & 1));
      pa[t][1] = 2 * ((r0 + 4) * 256 + (((ch & ~15) | ((ch & 15) ^ sw_hi)) << 3) + 4 * (fp & 1));
    } else {
      const int row = wp * 64 + t * 16 + fi;
      pa[t][0] = 2 * (row * 64 + (((0 + fg) ^ (row & 7)) << 3));
      pa[t][1] = 2 * (row * 64 + (((4 + fg) ^ (row & 7)) << 3));
    }
    const int chq = ((wq * 64 + t * 16) >> 3) + (fp >> 1);
    qa[t][0] = 2 * TT::P_ELEMS + 2 * (r0 * 128 + ((chq ^ sw_lo) << 3) + 4 * (fp & 1));
    qa[t][1] = 2 * TT::P_ELEMS + 2 * ((r0 + 4) * 128 + ((chq ^ sw_hi) << 3) + 4 * (fp & 1));
  }
  const unsigned smem_base = lds_addr(smem);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int slot) {
    const unsigned sb = smem_base + (unsigned)slot * (TT::SLOT * 2);
    bf16x8 fpv[2][4], fqv[2][4];
    static_for<2>([&](auto KS) {
      constexpr int ks = decltype(KS)::value;
      static_for<4>([&](auto T) {
        constexpr int t = decltype(T)::value;
        if constexpr (P_TR) {
          const bf16x4 lo = asm_read_tr_off<ks * 32 * 256 * 2>(sb + pa[t][0]);
          const bf16x4 hi = asm_read_tr_off<ks * 32 * 256 * 2>(sb + pa[t][1]);
          fpv[ks][t] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        } else {
          fpv[ks][t] = asm_read_b128_off<0>(sb + pa[t][ks]);
        }
        const bf16x4 lo = asm_read_tr_off<ks * 32 * 128 * 2>(sb + qa[t][0]);
        const bf16x4 hi = asm_read_tr_off<ks * 32 * 128 * 2>(sb + qa[t][1]);
        fqv[ks][t] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      });
      lds_reads_done();
      static_for<4>([&](auto MT) {
        constexpr int mt = decltype(MT)::value;
        static_for<4>([&](auto NTI) {
          constexpr int nt = decltype(NTI)::value;
          if constexpr (SWAP) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fpv[ks][mt], fqv[ks][nt], acc[mt][nt], 0, 0, 0);
          else                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fqv[ks][nt], fpv[ks][mt], acc[mt][nt], 0, 0, 0);
        });
      });
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  if (NL) {
    if (loader) {
      if (nk > 0) issue(0, kbeg);
      if (nk > 1) issue(1, kbeg + BK);
      int slot = 0;
      for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) wait_vmcnt<NDMA_>();
        else             wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + 2 < nk) issue(slot >= 1 ? slot - 1 : 2, kbeg + (kt + 2) * BK);
        slot = slot == 2 ? 0 : slot + 1;
      }
      return;
    }
    int slot = 0;
    for (int kt = 0; kt < nk; ++kt) {
      __builtin_amdgcn_s_barrier();
      compute(slot);
      slot = slot == 2 ? 0 : slot + 1;
    }
  } else {
    if (nk > 0) issue(0, kbeg);
    if (nk > 1) issue(1, kbeg + BK);
    int slot = 0;
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) wait_vmcnt<NDMA_>();
      else             wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      if (kt + 2 < nk) issue(slot >= 1 ? slot - 1 : 2, kbeg + (kt + 2) * BK);
      compute(slot);
      slot = slot == 2 ? 0 : slot + 1;
    }
  }

  if constexpr (SWAP) {
    // lane holds T[p = 4 fg + r][q = fi] of each 16 x 16 block: four consecutive p -> one float4 of row q of the transposed result
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int pc = p0 + wp * 64 + mt * 16 + 4 * fg;
      if (pc >= NPd) continue;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int qr = q0 + wq * 64 + nt * 16 + fi;
        if (qr >= NQd) continue;
        float4* dst = reinterpret_cast<float4*>(g.Cf + (size_t)qr * g.ldcf + pc);
        const f32x4 v = acc[mt][nt] * g.alpha;
        float4 o = make_float4(v[0], v[1], v[2], v[3]);
        if (g.accumulate) { const float4 c = *dst; o.x += c.x; o.y += c.y; o.z += c.z; o.w += c.w; }
        *dst = o;
      }
    }
  } else {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int row = p0 + wp * 64 + mt * 16 + fi;
      if (row >= NPd) continue;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int col = q0 + wq * 64 + nt * 16 + 4 * fg;
        if (col < NQd) epi_store<EPI>(g, row, col, acc[mt][nt]);
      }
    }
  }
}

template __global__ void k_cgemm_t<false, false, false, EPI_BF16>(BGemmArgs, unsigned, unsigned, unsigned, unsigned);
template __global__ void k_cgemm_t<false, false, false, EPI_RES>(BGemmArgs, unsigned, unsigned, unsigned, unsigned);
template __global__ void k_cgemm_t<true, false, false, EPI_RES>(BGemmArgs, unsigned, unsigned, unsigned, unsigned);
template __global__ void k_cgemm_t<true, true, true, EPI_RES>(BGemmArgs, unsigned, unsigned, unsigned, unsigned);
template __global__ void k_cgemm_t<false, false, false, EPI_BF16, 4>(BGemmArgs, unsigned, unsigned, unsigned, unsigned);
template __global__ void k_cgemm_t<false, false, false, EPI_RES, 4>(BGemmArgs, unsigned, unsigned, unsigned, unsigned);
template __global__ void k_cgemm_t<true, false, false, EPI_RES, 4>(BGemmArgs, unsigned, unsigned, unsigned, unsigned);
template __global__ void k_cgemm_t<true, true, true, EPI_RES, 4>(BGemmArgs, unsigned, unsigned, unsigned, unsigned);

int g_conv_loader_waves = 3;       // sfron_gemm_loader_waves(): bit 0 k_cgemm, bit 1 k_cgemm_t in the loader-wave form (0 = every wave issues its own DMA)
namespace {

// ---- weights: fp32 OIHW master -> bf16 GEMM operands.
// fwd  [Co_p][taps][Ci_p]   (rows beyond Cout and channels beyond Cin are zero)
// dgr  [Ci][taps][Co_p]     with the tap index flipped (tap' = taps - 1 - tap): B operand of the input-gradient GEMM
__global__ __launch_bounds__(TPB) void k_conv_wprep(const float* __restrict__ w, int Co, int Ci, int taps, int Co_p, int Ci_p,
                                                    __bf16* __restrict__ fwd, __bf16* __restrict__ dgr) {
  const int64_t nf = (int64_t)Co_p * taps * Ci_p;
  const int64_t nd = dgr ? (int64_t)Ci * taps * Co_p : 0;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < nf + nd; i += (int64_t)gridDim.x * TPB) {
    if (i < nf) {
      const int ci = (int)(i % Ci_p); const int t = (int)((i / Ci_p) % taps); const int co = (int)(i / ((int64_t)Ci_p * taps));
      fwd[i] = (co < Co && ci < Ci) ? f2bf(w[((int64_t)co * Ci + ci) * taps + t]) : (__bf16)0.0f;
    } else {
      const int64_t j = i - nf;
      const int co = (int)(j % Co_p); const int t = (int)((j / Co_p) % taps); const int ci = (int)(j / ((int64_t)Co_p * taps));
      dgr[j] = co < Co ? f2bf(w[((int64_t)co * Ci + ci) * taps + (taps - 1 - t)]) : (__bf16)0.0f;
    }
  }
}
// the same for the large 3x3 kernels of the LDM UNet through an LDS tile of 32 output x 32 input channels (bf16 [32][32][9]): the OIHW
// master is read in contiguous runs of 32 * 9 floats, the forward operand is written in runs of 32 input channels per (co, tap),
// the input-gradient operand in runs of 32 output channels per (ci, flipped tap).  grid = (ceil(Ci_p / 32), ceil(Co_p / 32)).
__device__ __forceinline__ void wprep9_tile(const float* __restrict__ w, int Co, int Ci, int Co_p, int Ci_p, __bf16* __restrict__ fwd,
                                            __bf16* __restrict__ dgr, int ci0, int co0, __bf16 (*t)[32 * 9 + 2]) {
  for (int i = threadIdx.x; i < 32 * 288; i += TPB) {
    const int co = i / 288, k = i - co * 288, ci = k / 9;
    const bool in = co0 + co < Co && ci0 + ci < Ci;
    t[co][k] = in ? f2bf(w[((int64_t)(co0 + co) * Ci + ci0) * 9 + k]) : (__bf16)0.0f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 32 * 9 * 32; i += TPB) {          // fwd [Co_p][9][Ci_p]
    const int ci = i & 31, tp = (i >> 5) % 9, co = i / 288;
    if (co0 + co < Co_p && ci0 + ci < Ci_p) fwd[((int64_t)(co0 + co) * 9 + tp) * Ci_p + ci0 + ci] = t[co][ci * 9 + tp];
  }
  if (dgr)
    for (int i = threadIdx.x; i < 32 * 9 * 32; i += TPB) {        // dgr [Ci][9 flipped][Co_p]
      const int co = i & 31, tp = (i >> 5) % 9, ci = i / 288;
      if (co0 + co < Co_p && ci0 + ci < Ci) dgr[((int64_t)(ci0 + ci) * 9 + tp) * Co_p + co0 + co] = t[co][ci * 9 + (8 - tp)];
    }
}
__global__ __launch_bounds__(TPB) void k_conv_wprep9(const float* __restrict__ w, int Co, int Ci, int Co_p, int Ci_p, __bf16* __restrict__ fwd,
                                                     __bf16* __restrict__ dgr) {
  __shared__ __bf16 t[32][32 * 9 + 2];
  wprep9_tile(w, Co, Ci, Co_p, Ci_p, fwd, dgr, blockIdx.x * 32, blockIdx.y * 32, t);
}
// every 3x3 kernel of a model in ONE launch: block b serves tile (b - item.tile0) of the item whose tile range holds it
__global__ __launch_bounds__(TPB) void k_conv_wprep9_batch(const sfron_wprep_item* __restrict__ items, int n_items) {
  __shared__ __bf16 t[32][32 * 9 + 2];
  int lo = 0, hi = n_items - 1;
  const int b = blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items[mid].tile0 <= b) lo = mid; else hi = mid - 1; }
  const sfron_wprep_item it = items[lo];
  const int local = b - it.tile0, tx = (it.ci_p + 31) / 32;
  wprep9_tile(it.w, it.co, it.ci, it.co_p, it.ci_p, (__bf16*)it.fwd, (__bf16*)it.dgr, (local % tx) * 32, (local / tx) * 32, t);
}
// weight gradient fp32 [nslab][Co_p][taps][Ci_p] (GEMM output, split-K slabs) -> OIHW gradient (overwrite; slabs added in order)
__device__ __forceinline__ void wgrad_scatter_block(const float* __restrict__ g, int Co, int Ci, int taps, int Ci_p, int nslab,
                                                    int64_t slab_stride, float* __restrict__ dw, int co, int ci0, float* sh) {
  // one workgroup per (64 input channels, output channel): thread (tap group tg, channel c) sums the slabs of taps tg, tg + 4, tg + 8
  // (reads coalesced along ci), the [ci][tap] block is turned through LDS (row stride = taps, odd: no bank conflicts) and leaves as
  // one contiguous run of the OIHW gradient
  constexpr int CB = 64, TG = TPB / CB;
  const int c = threadIdx.x % CB, tg = threadIdx.x / CB;
  const int nci = min(CB, Ci - ci0);
  if (c < nci)
    for (int t = tg; t < taps; t += TG) {
      const float* p = g + ((int64_t)co * taps + t) * Ci_p + ci0 + c;
      float a = 0.f;
      int sl = 0;
      for (; sl + 8 <= nslab; sl += 8) {          // eight strided loads in flight, added in slab order (a load-use loop pays one
        float v8[8];                              // memory latency per slab: 38 us for 64 slabs of a 128 x 128 kernel)
#pragma unroll
        for (int u = 0; u < 8; ++u) v8[u] = p[(int64_t)(sl + u) * slab_stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v8[u];
      }
      for (; sl < nslab; ++sl) a += p[(int64_t)sl * slab_stride];
      sh[c * taps + t] = a;
    }
  __syncthreads();
  float* o = dw + ((int64_t)co * Ci + ci0) * taps;
  for (int k = threadIdx.x; k < nci * taps; k += TPB) o[k] = sh[k];
}
__global__ __launch_bounds__(TPB) void k_conv_wgrad_scatter(const float* __restrict__ g, int Co, int Ci, int taps, int Ci_p, int nslab,
                                                            int64_t slab_stride, float* __restrict__ dw) {
  __shared__ float sh[64 * 9];
  wgrad_scatter_block(g, Co, Ci, taps, Ci_p, nslab, slab_stride, dw, blockIdx.y, blockIdx.x * 64, sh);
}
// the scatters of MANY kernel gradients in one launch (round 6): the items travel by value in the kernel arguments, as k_reduce_batch's
constexpr int WS_ITEMS = 80;                     // 80 x 48 bytes of the 4 KB of kernel arguments
struct ScatterPack { sfron_wgrad_scatter_item it[WS_ITEMS]; };
__global__ __launch_bounds__(TPB) void k_conv_wgrad_scatter_batch(ScatterPack pack) {
  __shared__ float sh[64 * 9];
  const sfron_wgrad_scatter_item it = pack.it[blockIdx.y];
  const int ncb = (it.c_in + 63) / 64;
  if ((int)blockIdx.x >= ncb * it.c_out) return;                  // uniform per workgroup
  const int co = blockIdx.x / ncb, ci0 = (blockIdx.x - co * ncb) * 64;
  wgrad_scatter_block(it.dw_gemm, it.c_out, it.c_in, it.taps, it.c_in_p, it.n_slabs, it.slab_stride, it.dw_oihw, co, ci0, sh);
}


// finish of a batched split-K product: out[y][z][m][n] (bf16, strides sC / sC2 / ldc) = sum_s slab[s][y][z][m][n]
__global__ __launch_bounds__(TPB) void k_bsplit_finish(const float* __restrict__ slabs, int nsplit, int ny, int nz, int M, int N, __bf16* __restrict__ out,
                                                       long sC, long sC2, int ldc) {
  const int64_t per = (int64_t)M * N, n = (int64_t)ny * nz * per;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int64_t b = i / per, r = i - b * per;
    const int y = (int)(b / nz), z = (int)(b - (int64_t)y * nz), m = (int)(r / N), c = (int)(r - (int64_t)m * N);
    float a = 0.f;
    for (int sl = 0; sl < nsplit; ++sl) a += slabs[sl * n + i];
    out[y * sC + z * sC2 + (int64_t)m * ldc + c] = f2bf(a);
  }
}
// split-K finish: out[row][col] = sum_s slab[s][row][col] (+ bias) (+ per-sample vector) (+ resid), bf16 or fp32 -- the epilogue of
// k_bgemm applied after the slabs of a split contraction are added in order
__global__ __launch_bounds__(TPB) void k_split_finish(const float* __restrict__ slabs, int nsl, int64_t slab_stride, int M, int N,
                                                      const float* __restrict__ bias, const float* __restrict__ vec, int ldvec, int T,
                                                      const float* __restrict__ resid, float* __restrict__ of, __bf16* __restrict__ ob, int ldo) {
  const int64_t n = (int64_t)M * N;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const int col = (int)(i % N); const int64_t row = i / N;
    float a = 0.f;
    for (int sl = 0; sl < nsl; ++sl) a += slabs[sl * slab_stride + i];
    if (bias) a += bias[col];
    if (vec) a += vec[(row / T) * ldvec + col];
    if (resid) a += resid[row * ldo + col];
    if (of) of[row * ldo + col] = a; else ob[row * ldo + col] = f2bf(a);
  }
}

// the same on float4 column quads with the rows walked per workgroup (no per-element 64-bit division): N % 4 == 0, ldo % 4 == 0
__global__ __launch_bounds__(TPB) void k_split_finish4(const float* __restrict__ slabs, int nsl, int64_t slab_stride, int M, int N,
                                                       const float* __restrict__ bias, const float* __restrict__ vec, int ldvec, int T,
                                                       const float* __restrict__ resid, float* __restrict__ of, __bf16* __restrict__ ob, int ldo,
                                                       int rows_per_block) {
  const int c = (blockIdx.x * TPB + threadIdx.x) * 4;
  if (c >= N) return;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
  float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) b4 = *reinterpret_cast<const float4*>(bias + c);
  for (int r = r0; r < r1; ++r) {
    const float* p = slabs + (int64_t)r * N + c;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sl = 0; sl < nsl; ++sl) { const float4 v = *reinterpret_cast<const float4*>(p + sl * slab_stride); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    a.x += b4.x; a.y += b4.y; a.z += b4.z; a.w += b4.w;
    if (vec) { const float4 v = *reinterpret_cast<const float4*>(vec + (int64_t)(r / T) * ldvec + c); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    if (resid) { const float4 v = *reinterpret_cast<const float4*>(resid + (int64_t)r * ldo + c); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    if (of) *reinterpret_cast<float4*>(of + (int64_t)r * ldo + c) = a;
    else *reinterpret_cast<bf16x4*>(ob + (int64_t)r * ldo + c) = bf16x4{f2bf(a.x), f2bf(a.y), f2bf(a.z), f2bf(a.w)};
  }
}

// splits of the contraction for a weight-gradient GEMM: enough workgroups for the chip (about two rounds of 256 CUs), at least
// 512 contraction rows per split, at most `cap`
inline int plan_splits(int M, int N, int K, int cap) {
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int s = 512 / (tiles > 0 ? tiles : 1);
  if (s > K / 512) s = K / 512;
  if (s > cap) s = cap;
  return s < 1 ? 1 : s;
}

template <bool A_TR, bool B_TR, int EPI, int CONV>
int launch_bgemm(const BGemmArgs& g, int nbatch, hipStream_t s, int ninner = 1) {
  const size_t lds = 4 * TILE_ELEMS * sizeof(__bf16);
  const int ntm = (g.M + BM - 1) / BM, ntn = (g.N + BN - 1) / BN;
  hipLaunchKernelGGL((k_bgemm<A_TR, B_TR, EPI, CONV>), dim3(ntm * ntn * (g.ksplit > 1 ? g.ksplit : 1), nbatch, ninner), dim3(NT), lds, s, g);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}

// debug build only (tools/ A-B runs): SFRON_NO_CGEMM=1 keeps every product on the generic k_bgemm tile; bit i of SFRON_NO_CGEMM
// disables: 1 direct tile, 2 Linear input gradient, 4 plain weight gradient, 8 convolution weight gradient
inline int cgemm_off() {
#ifdef SFRON_DEBUG_KNOBS
  static const int v = [] { const char* e = getenv("SFRON_NO_CGEMM"); return e ? atoi(e) : 0; }();
  return v;
#else
  return 0;
#endif
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per function AND per device
inline bool need_attr(std::atomic<uint64_t>& mask) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  return (mask.fetch_or(bit) & bit) == 0;
}
template <int NT_, int EPI, bool CONV, int NL>
int launch_cgemm_nl(const BGemmArgs& g, unsigned a_bytes, unsigned b_bytes, int nsplit, hipStream_t s) {
  using CT = CTile<NT_>;
  static std::atomic<uint64_t> done{0};        // per instantiation, one bit per device
  if (need_attr(done)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cgemm<NT_, EPI, CONV, NL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CT::LDS) !=
        hipSuccess)
      return (int)hipGetLastError();
  }
  const int ntm = g.M / CT::FBM, ntn = (g.N + CT::FBN - 1) / CT::FBN;
  hipLaunchKernelGGL((k_cgemm<NT_, EPI, CONV, NL>), dim3(ntm * ntn, nsplit), dim3(512 + 64 * NL), CT::LDS, s, g, a_bytes, b_bytes);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}
template <int NT_, int EPI, bool CONV>
int launch_cgemm_t(const BGemmArgs& g, unsigned a_bytes, unsigned b_bytes, int nsplit, hipStream_t s) {
  // a short contraction is all prologue: four loaders take twice as long to put the first two tiles in flight as eight waves do
  const int nk = (g.kchunk > 0 ? g.kchunk : g.K) / BK;
  return (g_conv_loader_waves & 1) && nk >= 8 ? launch_cgemm_nl<NT_, EPI, CONV, 4>(g, a_bytes, b_bytes, nsplit, s)
                                              : launch_cgemm_nl<NT_, EPI, CONV, 0>(g, a_bytes, b_bytes, nsplit, s);
}
// the pipelined tile when the product qualifies (-1: it does not, the caller launches k_bgemm)
int try_cgemm(const BGemmArgs& g, bool conv, size_t a_rows, int nsplit, hipStream_t s) {
  if (cgemm_off() & 1) return -1;
  if (g.M % 256 || g.K % BK || g.N % 4 || (g.kchunk > 0 && g.kchunk % BK)) return -1;
  if (conv && (g.cg.C % BK || (g.cg.taps != 9 && g.cg.taps != 1))) return -1;
  if ((((uintptr_t)g.A | (uintptr_t)g.B) & 15) || g.lda % 8 || g.ldb % 8) return -1;
  const size_t a_bytes = conv ? a_rows * g.lda * 2 : ((size_t)(g.M - 1) * g.lda + g.K) * 2;
  const size_t b_bytes = ((size_t)(g.N - 1) * g.ldb + g.K) * 2;
  if (a_bytes >= 0x7ffffff0ull || b_bytes >= 0x7ffffff0ull || (size_t)(g.N + 160) * g.ldb * 2 >= 0x7ffffff0ull) return -1;
  const bool bf = g.Cb != nullptr;
  const bool wide = g.N % 160 == 0;
#define SFRON_CG(NTV, CV) (bf ? launch_cgemm_t<NTV, EPI_BF16, CV>(g, (unsigned)a_bytes, (unsigned)b_bytes, nsplit, s) \
                              : launch_cgemm_t<NTV, EPI_RES, CV>(g, (unsigned)a_bytes, (unsigned)b_bytes, nsplit, s))
  if (conv) return wide ? SFRON_CG(10, true) : SFRON_CG(8, true);
  return wide ? SFRON_CG(10, false) : SFRON_CG(8, false);
#undef SFRON_CG
}

template <bool P_TR, bool CONVP, bool SWAP, int EPI, int NL>
int launch_cgemm_tt_nl(const BGemmArgs& g, size_t p_bytes, size_t q_bytes, unsigned mw, unsigned mh, int nsplit, hipStream_t s) {
  static std::atomic<uint64_t> done{0};
  if (need_attr(done)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cgemm_t<P_TR, CONVP, SWAP, EPI, NL>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)TTile::LDS) != hipSuccess)
      return (int)hipGetLastError();
  }
  const int np = SWAP ? g.N : g.M, nq = SWAP ? g.M : g.N;
  const int tiles = ((np + TTile::FBP - 1) / TTile::FBP) * ((nq + TTile::FBQ - 1) / TTile::FBQ);
  hipLaunchKernelGGL((k_cgemm_t<P_TR, CONVP, SWAP, EPI, NL>), dim3(tiles, nsplit), dim3(512 + 64 * NL), TTile::LDS, s, g, (unsigned)p_bytes, (unsigned)q_bytes, mw, mh);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}
template <bool P_TR, bool CONVP, bool SWAP, int EPI>
int launch_cgemm_tt(const BGemmArgs& g, size_t p_bytes, size_t q_bytes, unsigned mw, unsigned mh, int nsplit, hipStream_t s) {
  const int nk = (g.kchunk > 0 ? g.kchunk : g.K) / BK;
  return (g_conv_loader_waves & 2) && nk >= 8 ? launch_cgemm_tt_nl<P_TR, CONVP, SWAP, EPI, 4>(g, p_bytes, q_bytes, mw, mh, nsplit, s)
                                              : launch_cgemm_tt_nl<P_TR, CONVP, SWAP, EPI, 0>(g, p_bytes, q_bytes, mw, mh, nsplit, s);
}
// eligibility bound of the pipelined tiles' buffer resources: 16 bytes below the entry points' refusal line (common.h sfron_fits31)
inline bool fits31(size_t b) { return b < 0x7ffffff0ull; }
// Linear input gradient (A direct [M][K], B read transposed [K][N]) on the pipelined tile; -1 = not eligible
int try_cgemm_dt(const BGemmArgs& g, hipStream_t s) {
  if (cgemm_off() & 2) return -1;
  if (g.M % 256 || g.K % BK || g.N % 8 || g.lda % 8 || g.ldb % 8 || (((uintptr_t)g.A | (uintptr_t)g.B) & 15)) return -1;
  const size_t pb = ((size_t)(g.M - 1) * g.lda + g.K) * 2, qb = ((size_t)(g.K - 1) * g.ldb + g.N) * 2;
  if (!fits31(pb) || !fits31(qb) || !fits31((size_t)g.K * g.ldb * 2 + 4096)) return -1;
  return g.Cb ? launch_cgemm_tt<false, false, false, EPI_BF16>(g, pb, qb, 0, 0, 1, s) : launch_cgemm_tt<false, false, false, EPI_RES>(g, pb, qb, 0, 0, 1, s);
}
// plain weight gradient (both operands read transposed, contraction over the rows), fp32 result; -1 = not eligible
bool tt_ok(const BGemmArgs& g) {
  if (cgemm_off() & 4) return false;
  if (g.K % BK || g.M % 8 || g.N % 8 || g.lda % 8 || g.ldb % 8 || (((uintptr_t)g.A | (uintptr_t)g.B) & 15) || !g.Cf) return false;
  if (g.kchunk > 0 && g.kchunk % BK) return false;
  return fits31(((size_t)g.K * g.lda + 4096) * 2) && fits31(((size_t)g.K * g.ldb + 4096) * 2);
}
int try_cgemm_tt(const BGemmArgs& g, int nsplit, hipStream_t s) {
  if (!tt_ok(g)) return -1;
  const size_t pb = ((size_t)(g.K - 1) * g.lda + g.M) * 2, qb = ((size_t)(g.K - 1) * g.ldb + g.N) * 2;
  return launch_cgemm_tt<true, false, false, EPI_RES>(g, pb, qb, 0, 0, nsplit, s);
}
// workgroups of the weight-gradient tile (256 on the long axis, 128 on the other)
inline int tt_tiles(int np, int nq) { return ((np + TTile::FBP - 1) / TTile::FBP) * ((nq + TTile::FBQ - 1) / TTile::FBQ); }
inline int tt_splits(int tiles, int K, int cap, int64_t out_elems) {
  // time model (us): rounds of workgroups x K-tiles each walks (1.4 us per 64 contraction rows) + the fp32 slabs every split
  // writes and the scatter / reduction reads back (8 B per output element at ~4 TB/s)
  int best = 1;
  double best_t = 1e30;
  const int lim = K / 512 < cap ? K / 512 : cap;
  for (int sp = 1; sp <= (lim < 1 ? 1 : lim); ++sp) {
    const int rounds = (tiles * sp + 255) / 256;
    const double t = rounds * ((double)K / sp) * (1.4 / 64.0) + (sp > 1 ? sp : 0) * (double)out_elems * 2e-6;
    if (t < best_t) { best_t = t; best = sp; }
  }
  return best;
}

}  // namespace

extern "C" {

int sfron_bgemm_bf16(const sfron_bgemm_desc* d, void* stream) {
  SFRON_CHECK_ARG(d && d->A && d->B && d->M > 0 && d->N > 0 && d->K > 0 && d->batch >= 1);
  SFRON_CHECK_ARG(d->N % 4 == 0 && d->lda % 8 == 0 && d->ldb % 8 == 0 && (((uintptr_t)d->A | (uintptr_t)d->B) & 15) == 0);
  SFRON_CHECK_ARG(d->stride_a % 8 == 0 && d->stride_b % 8 == 0 && d->stride_c % 4 == 0);
  SFRON_CHECK_ARG(!d->a_transposed || d->b_transposed);          // no kernel reads A^T against a B that is not transposed
  if (!d->a_transposed || !d->b_transposed) SFRON_CHECK_ARG(d->K % 8 == 0);
  if (d->a_transposed) SFRON_CHECK_ARG(d->M % 8 == 0);
  if (d->b_transposed) SFRON_CHECK_ARG(d->N % 8 == 0);
  // 2 GiB rule, per matrix of the batch (the batch strides are 64-bit pointer steps): the pipelined tiles hold 32-bit byte offsets
  SFRON_CHECK_ARG(sfron_fits31(d->a_transposed ? sfron_extent(d->K, d->lda, d->M, 2) : sfron_extent(d->M, d->lda, d->K, 2)) &&
                  sfron_fits31(d->b_transposed ? sfron_extent(d->K, d->ldb, d->N, 2) : sfron_extent(d->N, d->ldb, d->K, 2)) &&
                  sfron_fits31(sfron_extent(d->M, d->ldc, d->N, d->c_f32 ? 4 : 2)));
  BGemmArgs g{};
  g.A = (const __bf16*)d->A; g.B = (const __bf16*)d->B;
  g.M = d->M; g.N = d->N; g.K = d->K; g.lda = d->lda; g.ldb = d->ldb;
  g.sA = d->stride_a; g.sB = d->stride_b; g.sC = d->stride_c;
  g.sA2 = d->stride_a2; g.sB2 = d->stride_b2; g.sC2 = d->stride_c2;
  const int ni = d->batch2 > 0 ? d->batch2 : 1;
  SFRON_CHECK_ARG(d->stride_a2 % 8 == 0 && d->stride_b2 % 8 == 0 && d->stride_c2 % 4 == 0);
  g.Cb = (__bf16*)d->c_bf16; g.ldcb = d->ldc; g.Cf = d->c_f32; g.ldcf = d->ldc;
  g.bias = d->bias; g.resid = d->resid; g.vec = d->sample_vec; g.ldvec = d->ld_vec; g.T = d->rows_per_sample > 0 ? d->rows_per_sample : 1;
  g.alpha = d->alpha; g.accumulate = d->accumulate;
  SFRON_CHECK_ARG((g.Cb != nullptr) != (g.Cf != nullptr) && d->ldc % 4 == 0);
  hipStream_t s = (hipStream_t)stream;
  const bool bf = g.Cb != nullptr;
  if (!d->a_transposed && !d->b_transposed) {
    if (d->batch == 1 && ni == 1) { const int rc = try_cgemm(g, false, 0, 1, s); if (rc >= 0) return rc; }
    return bf ? launch_bgemm<false, false, EPI_BF16, CONV_NONE>(g, d->batch, s, ni) : launch_bgemm<false, false, EPI_RES, CONV_NONE>(g, d->batch, s, ni);
  }
  if (!d->a_transposed && d->b_transposed) {
    if (d->batch == 1 && ni == 1) { const int rc = try_cgemm_dt(g, s); if (rc >= 0) return rc; }
    // a few rows against a deep contraction (the embedding projection's input gradient: 8 x 1280 over K = 28 000): split K over the chip
    if (!bf && d->split_ws && d->batch == 1 && ni == 1 && d->ldc == d->N && !d->bias && !d->resid && !d->sample_vec && !d->accumulate &&
        d->K >= 4096) {
      const int tiles = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
      int sp = 256 / (tiles > 0 ? tiles : 1);
      if (sp > g.K / 512) sp = g.K / 512;
      if (sp > d->split_ws_slabs) sp = d->split_ws_slabs;
      if (sp > 1) {
        g.kchunk = ((g.K + sp - 1) / sp + BK - 1) / BK * BK;
        const int used = (g.K + g.kchunk - 1) / g.kchunk;
        g.Cf = d->split_ws; g.sC = (long)d->M * d->N;
        const int rc = launch_bgemm<false, true, EPI_RES, CONV_NONE>(g, used, s, 1);
        if (rc) return rc;
        return sfron_reduce_chunks(d->split_ws, 1, used, d->M * d->N, d->c_f32, d->M * d->N, 0, stream);
      }
    }
    return bf ? launch_bgemm<false, true, EPI_BF16, CONV_NONE>(g, d->batch, s, ni) : launch_bgemm<false, true, EPI_RES, CONV_NONE>(g, d->batch, s, ni);
  }
  if (d->a_transposed && d->b_transposed) {
    const bool fast = !bf && d->batch == 1 && ni == 1 && tt_ok(g) && d->M >= 64 && d->N >= 64 && d->K >= 256;
    // a plain weight gradient (fp32 [M][N] contiguous, contraction over all rows): split-K through the caller's slab scratch
    if (!bf && d->split_ws && d->batch == 1 && ni == 1 && d->ldc == d->N && !d->bias && !d->resid && !d->sample_vec && !d->accumulate) {
      const int sp = fast ? tt_splits(tt_tiles(d->M, d->N), d->K, d->split_ws_slabs, (int64_t)d->M * d->N) : plan_splits(d->M, d->N, d->K, d->split_ws_slabs);
      if (sp > 1) {
        g.kchunk = ((g.K + sp - 1) / sp + BK - 1) / BK * BK;
        const int used = (g.K + g.kchunk - 1) / g.kchunk;
        g.Cf = d->split_ws; g.sC = (long)d->M * d->N;
        int rc = fast ? try_cgemm_tt(g, used, s) : -1;
        if (rc < 0) rc = launch_bgemm<true, true, EPI_RES, CONV_NONE>(g, used, s, 1);
        if (rc) return rc;
        return sfron_reduce_chunks(d->split_ws, 1, used, d->M * d->N, d->c_f32, d->M * d->N, 0, stream);
      }
    }
    if (fast) { const int rc = try_cgemm_tt(g, 1, s); if (rc >= 0) return rc; }
    // head-batched products with a single output tile each and a contraction over all tokens (dK, dV of the cross-attention): a
    // workgroup per (sample, head) leaves the chip three quarters empty and walks K = 4096 alone -- split the contraction
    if (bf && d->split_ws && (d->batch > 1 || ni > 1) && !d->bias && !d->resid && !d->sample_vec && !d->accumulate && d->alpha == 1.0f && g.K >= 1024) {
      const int tiles = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN) * d->batch * ni;
      int sp = 512 / (tiles > 0 ? tiles : 1);
      if (sp > g.K / 256) sp = g.K / 256;
      if (sp > 16) sp = 16;
      const int64_t per = (int64_t)d->batch * ni * d->M * d->N;
      if ((int64_t)sp * per > (int64_t)d->split_ws_slabs * d->M * d->N) sp = (int)((int64_t)d->split_ws_slabs * d->M * d->N / per);
      if (sp > 1) {
        BGemmArgs q = g;
        q.kchunk = ((g.K + sp - 1) / sp + BK - 1) / BK * BK;
        q.ksplit = (g.K + q.kchunk - 1) / q.kchunk;
        q.Cb = nullptr; q.Cf = d->split_ws; q.ldcf = d->N;
        int rc = launch_bgemm<true, true, EPI_RES, CONV_NONE>(q, d->batch, s, ni);
        if (rc) return rc;
        hipLaunchKernelGGL(k_bsplit_finish, dim3(grid_for(per)), dim3(TPB), 0, s, d->split_ws, q.ksplit, d->batch, ni, d->M, d->N, (__bf16*)d->c_bf16,
                           (long)d->stride_c, (long)d->stride_c2, d->ldc);
        SFRON_LAUNCH_STATUS();
        return SFRON_OK;
      }
    }
    return bf ? launch_bgemm<true, true, EPI_BF16, CONV_NONE>(g, d->batch, s, ni) : launch_bgemm<true, true, EPI_RES, CONV_NONE>(g, d->batch, s, ni);
  }
  return SFRON_ERR_UNSUPPORTED;
}

static int conv_geom(const sfron_conv_desc* d, ConvGeom& c, int src_c) {
  SFRON_CHECK_ARG(d->batch > 0 && d->h_src > 0 && d->w_src > 0 && d->h_out > 0 && d->w_out > 0 && (d->taps == 9 || d->taps == 1));
  SFRON_CHECK_ARG(d->stride == 1 || d->stride == 2);
  SFRON_CHECK_ARG(!(d->upsample && d->dilate) && src_c % 8 == 0);
  // 2 GiB rule: the GEMM row count batch * h_out * w_out and the source pixel index are formed in `int` and the pipelined tiles read the
  // source through a buffer resource (the generic tile they decline to is 64-bit in its offsets, but nothing runs it above the line)
  SFRON_CHECK_ARG(sfron_fits31((int64_t)d->batch * d->h_src * d->w_src * src_c * 2) && (int64_t)d->batch * d->h_out * d->w_out < (1ll << 31));
  c.Hs = d->h_src; c.Ws = d->w_src; c.C = src_c; c.Ho = d->h_out; c.Wo = d->w_out;
  c.stride = d->stride; c.pad = d->pad; c.up = d->upsample; c.dil = d->dilate; c.taps = d->taps; c.flip = 0;
  return SFRON_OK;
}

/* forward (and, with re-laid weights + flipped taps, input gradient): out[p][n] = sum_{tap, c} src[src(p, tap)][c] w[n][tap][c] */
int sfron_conv_fwd(const sfron_conv_desc* d, const uint16_t* src, const uint16_t* w, void* stream) {
  SFRON_CHECK_ARG(d && src && w && d->n_out % 4 == 0);
  if (d->split_pending) *d->split_pending = 0;
  // a pending split leaves fp32 slabs for a GroupNorm (or sfron_split_finish) to turn into the fp32 output: with out_bf16 nobody would write it
  SFRON_CHECK_ARG(!(d->split_pending && d->out_bf16));
  BGemmArgs g{};
  int rc = conv_geom(d, g.cg, d->c_src); if (rc) return rc;
  g.A = (const __bf16*)src; g.B = (const __bf16*)w;
  g.M = d->batch * d->h_out * d->w_out; g.N = d->n_out; g.K = d->taps * d->c_src;
  g.lda = d->c_src; g.ldb = g.K;
  g.Cb = (__bf16*)d->out_bf16; g.Cf = d->out_f32; g.ldcb = g.ldcf = d->ld_out;
  SFRON_CHECK_ARG((g.Cb != nullptr) != (g.Cf != nullptr) && d->ld_out % 4 == 0 && d->ld_out >= d->n_out);
  // the output (and `resid`, which shares its layout) and the weights, as the source in conv_geom
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent((int64_t)d->batch * d->h_out * d->w_out, d->ld_out, d->n_out, g.Cf ? 4 : 2)) &&
                  sfron_fits31((int64_t)d->n_out * d->taps * d->c_src * 2));
  g.bias = d->bias; g.resid = d->resid; g.vec = d->sample_vec; g.ldvec = d->ld_vec; g.T = d->h_out * d->w_out;
  g.alpha = 1.0f; g.accumulate = d->accumulate;
  // few output pixels, deep contraction (the 16x16 / 8x8 levels of the LDM UNet: 512 x 1280 outputs over K = 11520..23040): split the
  // contraction over the chip into fp32 slabs, then one pass adds them and applies the epilogue
  const size_t a_rows = (size_t)d->batch * d->h_src * d->w_src;
  // workgroups the launch would have: 256 x 160 | 128 tiles when the pipelined kernel takes it, 128 x 128 otherwise
  const bool pipelined = g.M % 256 == 0 && g.K % BK == 0 && d->c_src % BK == 0;
  const int tiles = pipelined ? (g.M / 256) * ((g.N + (g.N % 160 == 0 ? 160 : 128) - 1) / (g.N % 160 == 0 ? 160 : 128))
                              : ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
  if (d->split_ws && !d->accumulate && tiles < (pipelined ? 224 : 128) && g.K >= 2048) {
    int sp = 384 / tiles;
    if (sp > g.K / 512) sp = g.K / 512;
    if (pipelined) {
      // the time model of tt_splits: rounds of workgroups x K-tiles each walks + the slabs the finish kernel reads back
      int lim = g.K / 1024;
      if (lim > d->split_ws_slabs) lim = d->split_ws_slabs;
      double best_t = 1e30;
      sp = 1;
      for (int c = 1; c <= (lim < 1 ? 1 : lim); ++c) {
        const int rounds = (tiles * c + 255) / 256;
        const double t = rounds * ((double)g.K / c) * (1.3 / 64.0) + (c > 1 ? c + 1 : 0) * (double)g.M * g.N * 1e-6;
        if (t < best_t) { best_t = t; sp = c; }
      }
    }
    if (sp > d->split_ws_slabs) sp = d->split_ws_slabs;
    if (sp > 1) {
      BGemmArgs q = g;
      q.kchunk = ((g.K + sp - 1) / sp + BK - 1) / BK * BK;
      const int used = (g.K + q.kchunk - 1) / q.kchunk;
      q.Cb = nullptr; q.Cf = d->split_ws; q.ldcf = g.N; q.sC = (long)g.M * g.N;
      q.bias = nullptr; q.resid = nullptr; q.vec = nullptr;
      rc = try_cgemm(q, true, a_rows, used, (hipStream_t)stream);
      if (rc < 0) rc = launch_bgemm<false, false, EPI_RES, CONV_A>(q, used, (hipStream_t)stream);
      if (rc) return rc;
      const bool al = (((uintptr_t)d->split_ws | (uintptr_t)g.bias | (uintptr_t)g.vec | (uintptr_t)g.resid | (uintptr_t)g.Cf) & 15) == 0 &&
                      (((uintptr_t)g.Cb) & 7) == 0;
      const bool quads = g.N % 4 == 0 && d->ld_out % 4 == 0 && (!g.vec || g.ldvec % 4 == 0) && al;
      if (quads && d->split_pending && d->ld_out == g.N) {   // the caller's GroupNorm finishes the sum itself (sfron_groupnorm_*_src)
        *d->split_pending = used;
        return SFRON_OK;
      }
      if (quads) {
        const int cb = (g.N / 4 + TPB - 1) / TPB;
        int chunks = 2048 / cb; if (chunks > g.M) chunks = g.M; if (chunks < 1) chunks = 1;
        const int rpb = (g.M + chunks - 1) / chunks;
        hipLaunchKernelGGL(k_split_finish4, dim3(cb, (g.M + rpb - 1) / rpb), dim3(TPB), 0, (hipStream_t)stream, d->split_ws, used, (int64_t)g.M * g.N, g.M,
                           g.N, g.bias, g.vec, g.ldvec, g.T, g.resid, g.Cf, g.Cb, d->ld_out, rpb);
      } else
      hipLaunchKernelGGL(k_split_finish, dim3(grid_for((int64_t)g.M * g.N)), dim3(TPB), 0, (hipStream_t)stream, d->split_ws, used, (int64_t)g.M * g.N,
                         g.M, g.N, g.bias, g.vec, g.ldvec, g.T, g.resid, g.Cf, g.Cb, d->ld_out);
      SFRON_LAUNCH_STATUS();
      return SFRON_OK;
    }
  }
  rc = try_cgemm(g, true, a_rows, 1, (hipStream_t)stream);
  if (rc >= 0) return rc;
  return g.Cb ? launch_bgemm<false, false, EPI_BF16, CONV_A>(g, 1, (hipStream_t)stream)
              : launch_bgemm<false, false, EPI_RES, CONV_A>(g, 1, (hipStream_t)stream);
}

/* weight gradient: dw[n][tap][c] = sum_p dy[p][n] src[src(p, tap)][c]  (fp32 [n_out][taps * c_src], then k_conv_wgrad_scatter) */
static bool conv_wgrad_pipelined(const sfron_conv_desc* d) {
  if (cgemm_off() & 8) return false;
  const long K = (long)d->batch * d->h_out * d->w_out;
  return K % BK == 0 && K >= 256 && d->c_src % 8 == 0 && d->n_out % 8 == 0 && d->h_out >= 2 && d->w_out >= 2 && d->n_out >= 64 &&
         d->taps * d->c_src >= 64 && K < (1l << 21) && d->w_out <= 2048 && d->h_out <= 2048;
}
static int conv_wgrad_plan(const sfron_conv_desc* d) {
  const int K = d->batch * d->h_out * d->w_out;
  if (conv_wgrad_pipelined(d)) return tt_splits(tt_tiles(d->taps * d->c_src, d->n_out), K, 64, (int64_t)d->taps * d->c_src * d->n_out);
  return plan_splits(d->n_out, d->taps * d->c_src, K, 64);
}
// the number of slabs sfron_conv_wgrad WRITES (the planned split count, less the ones the rounding of the k range leaves without rows):
// the caller sizes dw_gemm for it and hands the same number to sfron_conv_wgrad_scatter -- nothing has to be zeroed
int sfron_conv_wgrad_splits(const sfron_conv_desc* d) {
  if (!d) return 0;
  const int sp = conv_wgrad_plan(d);
  if (sp <= 1) return sp;
  const int K = d->batch * d->h_out * d->w_out;
  const int kchunk = ((K + sp - 1) / sp + BK - 1) / BK * BK;
  return (K + kchunk - 1) / kchunk;
}
int sfron_conv_wgrad(const sfron_conv_desc* d, const uint16_t* dy, int ld_dy, const uint16_t* src, float* dw_gemm, void* stream) {
  SFRON_CHECK_ARG(d && dy && src && dw_gemm && d->n_out % 8 == 0 && ld_dy % 8 == 0);
  BGemmArgs g{};
  int rc = conv_geom(d, g.cg, d->c_src); if (rc) return rc;
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent((int64_t)d->batch * d->h_out * d->w_out, ld_dy, d->n_out, 2)) &&
                  sfron_fits31((int64_t)d->n_out * d->taps * d->c_src * 4));            // dy and one fp32 slab, as the source in conv_geom
  g.A = (const __bf16*)dy; g.B = (const __bf16*)src;
  g.M = d->n_out; g.N = d->taps * d->c_src; g.K = d->batch * d->h_out * d->w_out;
  g.lda = ld_dy; g.ldb = d->c_src;
  g.Cf = dw_gemm; g.ldcf = g.N; g.alpha = 1.0f; g.T = 1;
  // the contraction runs over every pixel of the batch and the output has few 128x128 tiles: split it; slab s of dw_gemm
  // ([splits][n_out][taps * c_src]) receives split s, sfron_conv_wgrad_scatter adds the slabs in order
  const int sp = conv_wgrad_plan(d);
  if (sp > 1) { g.kchunk = ((g.K + sp - 1) / sp + BK - 1) / BK * BK; g.sC = (long)g.M * g.N; }
  const int used = sp > 1 ? (g.K + g.kchunk - 1) / g.kchunk : 1;       // == sfron_conv_wgrad_splits(d)
  rc = -1;
  if (conv_wgrad_pipelined(d) && (ld_dy % 8) == 0 && (((uintptr_t)dy | (uintptr_t)src) & 15) == 0) {
    const size_t pb = (size_t)d->batch * d->h_src * d->w_src * d->c_src * 2, qb = ((size_t)(g.K - 1) * ld_dy + g.M) * 2;
    if (fits31(pb) && fits31(qb + (size_t)ld_dy * 2 * 64)) {
      const unsigned mw = (unsigned)(0x100000000ull / (unsigned)d->w_out) + 1u, mh = (unsigned)(0x100000000ull / (unsigned)d->h_out) + 1u;
      rc = launch_cgemm_tt<true, true, true, EPI_RES>(g, pb, qb, mw, mh, used, (hipStream_t)stream);
    }
  }
  if (rc < 0) rc = launch_bgemm<true, true, EPI_RES, CONV_B>(g, used, (hipStream_t)stream);
  return rc;
}

int sfron_conv_wprep(const float* w_oihw, int c_out, int c_in, int taps, int c_out_p, int c_in_p, uint16_t* w_fwd, uint16_t* w_dgrad,
                     void* stream) {
  SFRON_CHECK_ARG(w_oihw && w_fwd && c_out_p >= c_out && c_in_p >= c_in && (taps == 9 || taps == 1));
  if (taps == 9 && (int64_t)c_in_p * c_out_p >= 256 * 1024) {
    hipLaunchKernelGGL(k_conv_wprep9, dim3((c_in_p + 31) / 32, (c_out_p + 31) / 32), dim3(TPB), 0, (hipStream_t)stream, w_oihw, c_out, c_in, c_out_p,
                       c_in_p, (__bf16*)w_fwd, (__bf16*)w_dgrad);
    SFRON_LAUNCH_STATUS();
    return SFRON_OK;
  }
  const int64_t n = (int64_t)c_out_p * taps * c_in_p + (w_dgrad ? (int64_t)c_in * taps * c_out_p : 0);
  hipLaunchKernelGGL(k_conv_wprep, dim3(grid_for(n)), dim3(TPB), 0, (hipStream_t)stream, w_oihw, c_out, c_in, taps, c_out_p, c_in_p,
                     (__bf16*)w_fwd, (__bf16*)w_dgrad);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_conv_wprep_tiles(int c_out_p, int c_in_p) { return ((c_out_p + 31) / 32) * ((c_in_p + 31) / 32); }
int sfron_conv_wprep_batch(const sfron_wprep_item* items_dev, int n_items, int n_tiles, void* stream) {
  SFRON_CHECK_ARG(items_dev && n_items > 0 && n_tiles > 0);
  hipLaunchKernelGGL(k_conv_wprep9_batch, dim3(n_tiles), dim3(TPB), 0, (hipStream_t)stream, items_dev, n_items);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}
int sfron_conv_wgrad_scatter(const float* dw_gemm, int c_out, int c_in, int taps, int c_in_p, int n_slabs, int64_t slab_stride,
                             float* dw_oihw, void* stream) {
  SFRON_CHECK_ARG(dw_gemm && dw_oihw && n_slabs >= 1);
  SFRON_CHECK_ARG(taps <= 9);
  hipLaunchKernelGGL(k_conv_wgrad_scatter, dim3((c_in + 63) / 64, c_out), dim3(TPB), 0, (hipStream_t)stream, dw_gemm,
                     c_out, c_in, taps, c_in_p, n_slabs, slab_stride, dw_oihw);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int sfron_conv_wgrad_scatter_batch(const sfron_wgrad_scatter_item* items, int n_items, void* stream) {
  SFRON_CHECK_ARG(items && n_items > 0);
  for (int i = 0; i < n_items; ++i)
    SFRON_CHECK_ARG(items[i].dw_gemm && items[i].dw_oihw && items[i].n_slabs >= 1 && items[i].taps >= 1 && items[i].taps <= 9 && items[i].c_out > 0 &&
                    items[i].c_in > 0 && items[i].c_in_p >= items[i].c_in);
  for (int i0 = 0; i0 < n_items; i0 += WS_ITEMS) {
    const int n = n_items - i0 < WS_ITEMS ? n_items - i0 : WS_ITEMS;
    ScatterPack pack;
    long gx = 1;
    for (int i = 0; i < n; ++i) {
      pack.it[i] = items[i0 + i];
      const long need = (long)((items[i0 + i].c_in + 63) / 64) * items[i0 + i].c_out;
      gx = need > gx ? need : gx;
    }
    for (int i = n; i < WS_ITEMS; ++i) pack.it[i] = pack.it[0];
    SFRON_CHECK_ARG(gx <= 0x7fffffffL);
    hipLaunchKernelGGL(k_conv_wgrad_scatter_batch, dim3((unsigned)gx, n), dim3(TPB), 0, (hipStream_t)stream, pack);
    SFRON_LAUNCH_STATUS();
  }
  return SFRON_OK;
}

// the plain finish of the slabs sfron_conv_fwd left pending (a GroupNorm that takes them itself: groupnorm.hip sfron_groupnorm_*_src)
int sfron_split_finish(const sfron_split_src* src, int64_t rows, int C, int rows_per_sample, float* out_f32, uint16_t* out_bf16, int ld_out,
                       void* stream) {
  SFRON_CHECK_ARG(split_src_ok(src, C) && rows > 0 && rows <= 0x7fffffff && rows_per_sample > 0 && ((out_f32 != nullptr) != (out_bf16 != nullptr)) &&
                  ld_out >= C && ld_out % 4 == 0);
  SFRON_CHECK_ARG(!src->resid || src->ld_resid == ld_out);
  SFRON_CHECK_ARG((((uintptr_t)out_f32) & 15) == 0 && (((uintptr_t)out_bf16) & 7) == 0);
  const int cb = (C / 4 + TPB - 1) / TPB;
  int chunks = 2048 / cb; if (chunks > rows) chunks = (int)rows; if (chunks < 1) chunks = 1;
  const int rpb = (int)((rows + chunks - 1) / chunks);
  hipLaunchKernelGGL(k_split_finish4, dim3(cb, (unsigned)((rows + rpb - 1) / rpb)), dim3(TPB), 0, (hipStream_t)stream, src->slabs, src->n_slabs,
                     src->slab_stride, (int)rows, C, src->bias, src->sample_vec, src->ld_vec, rows_per_sample, src->resid, out_f32, (__bf16*)out_bf16,
                     ld_out, rpb);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

}  // extern "C"
