// Precision / recall manifolds and the Inception Score (DDPM/evaluator.py: ManifoldEstimator, DistanceBlock, compute_inception_score).
//
// One fp32 NT tile kernel on the exact fp32-input matrix core instruction (v_mfma_f32_32x32x2_f32): dot[i][j] = sum_k A[i][k] * B[j][k].
// The order of every element is fixed and the same wherever the element falls in a tile: the 128 products of a block of k (MT_FLUSH
// steps of MT_BK = 32) are a k-ordered chain that starts from 0, and the block sums are added in block order -- a blocked sum, whose
// error is a blocked product's, not that of one K-long chain.  A workgroup (4 waves) owns a 128 x 128 block, a wave 2 x 2 results of
// 32 x 32; both operands go through LDS k-major ([k][row], so a wave's operand read is 32 consecutive words), 32 columns of k per step,
// the next step's rows already in registers while the current one is multiplied.  Rows past the end and a k past K are staged as 0: a
// zero adds nothing to the chain.
//
// A lane of a 32 x 32 result owns ONE column (the B side) and 16 rows.  The three epilogues:
//   EPI_STORE  C[i][j] = dot                                                          (sfron_gemm_nt_f32: the Inception Score's head)
//   EPI_KNN    d = max((n_q - 2 dot) + n_c, 0) with the QUERY on the B side: a lane inserts its 16 distances per result into its own
//              sorted list of the MF_KEEP smallest; lanes l and l + 32 (same query, other rows) merge once per block, the two waves that
//              share the query merge through LDS, and the list goes to workspace[query][slot].  A second launch merges the slots.
//   EPI_PR     set 1 on the A side, set 2 on the B side: in2[j] |= d <= r1[i] is the lane's own OR, in1[i] |= d <= r2[j] one ballot per
//              row.  Flags are only ever turned on (same-value byte stores): the result does not depend on the order.
// The squared norms are summed from the staged tile by the first 128 threads for the A rows and the other 128 for the B rows (the same
// blocked order as the product, so d(i, i) is exactly 0, and the same bits for a row wherever and in whichever set it stands); no
// separate launch, so sfron_manifold_pr needs no workspace.  No N x N matrix is ever stored.
#include "common.h"
#include "../../include/sfron.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int MT = 128, MT_BK = 32, MT_LD = MT + 2, MT_TPB = 256;      // MT_LD % 8 == 2: the staging stores of a wave spread over the banks
constexpr int MT_FLUSH = 4;                                           // k steps per block of the blocked sum: 128 columns of k
constexpr int MF_KEEP = 8;                                            // max(nhood) + 1 <= 8 list entries per query
enum { EPI_STORE = 0, EPI_KNN = 1, EPI_PR = 2 };

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

struct MTArgs {
  const float* A; const float* B;
  int M, N, K, lda, ldb;
  float* C; int ldc;                                       // EPI_STORE
  float* lists; int slots, slot0, splits;                  // EPI_KNN: lists [N][slots][MF_KEEP]; this launch fills slot0 .. slot0 + splits - 1
  const float* r1; const float* r2; int K1, K2;            // EPI_PR: radii of the A rows [M][K1] and of the B rows [N][K2]
  uint8_t* in1; uint8_t* in2;                              //         in1 [M][K2], in2 [N][K1]
};

// v into the ascending list (the largest entry falls out)
__device__ __forceinline__ void list_insert(float (&l)[MF_KEEP], float v) {
#pragma unroll
  for (int t = 0; t < MF_KEEP; ++t) {
    const float lo = fminf(l[t], v);
    v = fmaxf(l[t], v);
    l[t] = lo;
  }
}

template <int EPI>
__global__ __launch_bounds__(MT_TPB) void k_nt_tile(const MTArgs g) {
  __shared__ float sA[MT_BK][MT_LD], sB[MT_BK][MT_LD];
  __shared__ float nA[MT], nB[MT];
  __shared__ float4 rA[EPI == EPI_PR ? MT : 1];              // the A rows' radii, -inf where there is none: one 16-byte read per row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, lc = lane & 31, lh = lane >> 5;
  const int64_t col0 = (int64_t)blockIdx.x * MT;           // B rows = columns of the result
  const int row_tiles = (g.M + MT - 1) / MT;
  // staging map: piece p = tid + 256 i, row p / 8, k columns 4 (p % 8) .. + 3
  const int sr = tid >> 3, sk = (tid & 7) * 4;

  float keep[2][MF_KEEP];
  unsigned flag2[2] = {0u, 0u};
  if constexpr (EPI == EPI_KNN) {
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int t = 0; t < MF_KEEP; ++t) keep[n][t] = __builtin_inff();
  }

  for (int rt = blockIdx.y; rt < row_tiles; rt += gridDim.y) {
    const int64_t row0 = (int64_t)rt * MT;
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
    f32x16 part[2][2];                                     // the running block's chain
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[m][n][r] = 0.0f;
    float nrm = 0.0f, pn = 0.0f;
    float4 pa[4], pb[4];
    auto fetch = [&](int k0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = sr + 32 * i, k = k0 + sk;
        pa[i] = (row0 + r < g.M && k < g.K) ? *reinterpret_cast<const float4*>(g.A + (row0 + r) * g.lda + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        pb[i] = (col0 + r < g.N && k < g.K) ? *reinterpret_cast<const float4*>(g.B + (col0 + r) * g.ldb + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < g.K; k0 += MT_BK) {
      __syncthreads();                                     // the previous step's reads (and the previous row tile's epilogue) are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = sr + 32 * i;
        sA[sk][r] = pa[i].x; sA[sk + 1][r] = pa[i].y; sA[sk + 2][r] = pa[i].z; sA[sk + 3][r] = pa[i].w;
        sB[sk][r] = pb[i].x; sB[sk + 1][r] = pb[i].y; sB[sk + 2][r] = pb[i].z; sB[sk + 3][r] = pb[i].w;
      }
      __syncthreads();
      if (k0 + MT_BK < g.K) fetch(k0 + MT_BK);
      if constexpr (EPI != EPI_STORE) {                      // the norm in the product's own order
        const float* col = tid < MT ? &sA[0][tid] : &sB[0][tid - MT];
#pragma unroll
        for (int k = 0; k < MT_BK; ++k) { const float v = col[k * MT_LD]; pn = __builtin_fmaf(v, v, pn); }
      }
#pragma unroll
      for (int kk = 0; kk < MT_BK / 2; ++kk) {
        float a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) a[m] = sA[2 * kk + lh][wm * 64 + m * 32 + lc];
#pragma unroll
        for (int n = 0; n < 2; ++n) b[n] = sB[2 * kk + lh][wn * 64 + n * 32 + lc];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n) part[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[n], part[m][n], 0, 0, 0);
      }
      if ((k0 / MT_BK) % MT_FLUSH == MT_FLUSH - 1 || k0 + MT_BK >= g.K) {       // the end of a block of MT_FLUSH k steps, or of K
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            acc[m][n] += part[m][n];
#pragma unroll
            for (int r = 0; r < 16; ++r) part[m][n][r] = 0.0f;
          }
        nrm += pn;
        pn = 0.0f;
      }
    }

    // a lane's result register r of (m, n): row wm 64 + m 32 + (r & 3) + 8 (r >> 2) + 4 lh, column wn 64 + n 32 + lc
    if constexpr (EPI == EPI_STORE) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int64_t j = col0 + wn * 64 + n * 32 + lc;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t i = row0 + wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (i < g.M && j < g.N) g.C[i * g.ldc + j] = acc[m][n][r];
          }
        }
    } else {
      __syncthreads();                                     // (nA / nB / rA of the previous row tile are no longer read)
      if (tid < MT) nA[tid] = nrm; else nB[tid - MT] = nrm;
      if constexpr (EPI == EPI_PR) {
        if (tid < MT) {
          float v[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) v[a] = (row0 + tid < g.M && a < g.K1) ? g.r1[(row0 + tid) * g.K1 + a] : -__builtin_inff();
          rA[tid] = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int cj = wn * 64 + n * 32 + lc;
        const int64_t j = col0 + cj;
        const float nq = nB[cj];
        float r2[4];
        if constexpr (EPI == EPI_PR) {
#pragma unroll
          for (int b = 0; b < 4; ++b) r2[b] = (j < g.N && b < g.K2) ? g.r2[j * g.K2 + b] : -__builtin_inff();
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ci = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int64_t i = row0 + ci;
            if constexpr (EPI == EPI_KNN) {
              // the reference's fp32 branch with the query as U: max(norm_u - 2 u.v + norm_v, 0)
              const float d = fmaxf((nq - 2.0f * acc[m][n][r]) + nA[ci], 0.0f);
              list_insert(keep[n], i < g.M ? d : __builtin_inff());
            } else {
              // set 1 (the A side) is U
              const float d = fmaxf((nA[ci] - 2.0f * acc[m][n][r]) + nq, 0.0f);
              const float4 ra = rA[ci];
              flag2[n] |= (d <= ra.x ? 1u : 0u) | (d <= ra.y ? 2u : 0u) | (d <= ra.z ? 4u : 0u) | (d <= ra.w ? 8u : 0u);
#pragma unroll
              for (int b = 0; b < 4; ++b) {
                if (b < g.K2) {
                  const unsigned long long any = __ballot(d <= r2[b]);
                  const unsigned half = lh ? (unsigned)(any >> 32) : (unsigned)any;
                  if (lc == 0 && half && i < g.M) g.in1[i * g.K2 + b] = 1;
                }
              }
            }
          }
        }
      }
    }
  }

  if constexpr (EPI == EPI_KNN) {
    // lanes l and l + 32 hold the same query's other rows; then the wave with wm = 1 hands its lists to the wave with wm = 0
    float (*ex)[MT][MF_KEEP + 1] = reinterpret_cast<float (*)[MT][MF_KEEP + 1]>(&sA[0][0]);      // 128 x 9 words: inside sA
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      float other[MF_KEEP];
#pragma unroll
      for (int t = 0; t < MF_KEEP; ++t) other[t] = __shfl_xor(keep[n][t], 32, 64);
#pragma unroll
      for (int t = 0; t < MF_KEEP; ++t) list_insert(keep[n], other[t]);
      if (wm == 1 && lh == 0) {
#pragma unroll
        for (int t = 0; t < MF_KEEP; ++t) (*ex)[wn * 64 + n * 32 + lc][t] = keep[n][t];
      }
    }
    __syncthreads();
    if (wm == 0 && lh == 0) {
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int cj = wn * 64 + n * 32 + lc;
        const int64_t j = col0 + cj;
#pragma unroll
        for (int t = 0; t < MF_KEEP; ++t) list_insert(keep[n], (*ex)[cj][t]);
        if (j < g.N) {
          float* o = g.lists + (j * g.slots + g.slot0 + blockIdx.y) * MF_KEEP;
          *reinterpret_cast<float4*>(o) = make_float4(keep[n][0], keep[n][1], keep[n][2], keep[n][3]);
          *reinterpret_cast<float4*>(o + 4) = make_float4(keep[n][4], keep[n][5], keep[n][6], keep[n][7]);
        }
      }
    }
  }
  if constexpr (EPI == EPI_PR) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const unsigned f = flag2[n] | (unsigned)__shfl_xor((int)flag2[n], 32, 64);
      const int64_t j = col0 + wn * 64 + n * 32 + lc;
      if (lh == 0 && j < g.N) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (a < g.K1 && (f >> a & 1u)) g.in2[j * g.K1 + a] = 1;
      }
    }
  }
}

struct Nhood { int k[4]; int n; };

// radii[q][a] = (merged ascending list of the query's slots)[nhood[a]]: a thread per query
__global__ __launch_bounds__(MT_TPB) void k_knn_select(const float* __restrict__ lists, int slots, int nq, Nhood nh, float* __restrict__ radii) {
  const int q = blockIdx.x * MT_TPB + threadIdx.x;
  if (q >= nq) return;
  float l[MF_KEEP];
#pragma unroll
  for (int t = 0; t < MF_KEEP; ++t) l[t] = __builtin_inff();
  const float* p = lists + (int64_t)q * slots * MF_KEEP;
  for (int s = 0; s < slots; ++s) {
    const float4 u = *reinterpret_cast<const float4*>(p + s * MF_KEEP), v = *reinterpret_cast<const float4*>(p + s * MF_KEEP + 4);
    list_insert(l, u.x); list_insert(l, u.y); list_insert(l, u.z); list_insert(l, u.w);
    list_insert(l, v.x); list_insert(l, v.y); list_insert(l, v.z); list_insert(l, v.w);
  }
  for (int a = 0; a < nh.n; ++a) {
    float v = l[0];
#pragma unroll
    for (int t = 1; t < MF_KEEP; ++t) v = nh.k[a] == t ? l[t] : v;
    radii[(int64_t)q * nh.n + a] = v;
  }
}

// ---- Inception Score ---------------------------------------------------------------------------------------------------------------
// p = exp(x - max) / sum in fp32, in place; a workgroup per row
__global__ __launch_bounds__(MT_TPB) void k_is_softmax(float* __restrict__ x, int C, int ld) {
  __shared__ float sh[4];
  float* row = x + (int64_t)blockIdx.x * ld;
  float m = -__builtin_inff();
  for (int c = threadIdx.x; c < C; c += MT_TPB) m = fmaxf(m, row[c]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  float s = 0.0f;
  for (int c = threadIdx.x; c < C; c += MT_TPB) { const float e = expf(row[c] - m); row[c] = e; s += e; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  for (int c = threadIdx.x; c < C; c += MT_TPB) row[c] = row[c] / s;
}

// logm[c] = log(mean over the n rows of p[.][c]) in fp64.  A workgroup owns IS_COLS columns; row group g of 16 adds rows g, g + 16, ... in
// ascending order, then the sixteen group sums in order.  Also re-arms the KL launch's arrival counter.
constexpr int IS_COLS = 16, IS_GROUPS = MT_TPB / IS_COLS;
__global__ __launch_bounds__(MT_TPB) void k_is_colmean(const float* __restrict__ p, int n, int C, int ld, double* __restrict__ logm,
                                                       unsigned* __restrict__ counter) {
  __shared__ double sh[IS_GROUPS][IS_COLS];
  const int lc = threadIdx.x % IS_COLS, g = threadIdx.x / IS_COLS, c = blockIdx.x * IS_COLS + lc;
  double s = 0.0;
  if (c < C) for (int r = g; r < n; r += IS_GROUPS) s += (double)p[(int64_t)r * ld + c];
  sh[g][lc] = s;
  __syncthreads();
  if (g == 0 && c < C) {
    double t = sh[0][lc];
#pragma unroll
    for (int k = 1; k < IS_GROUPS; ++k) t += sh[k][lc];
    logm[c] = log(t / (double)n);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter = 0u;
}

// part[b] = sum over rows 16 b .. 16 b + 15 and all columns of p (log p - logm) in fp64, p == 0 contributing 0; the workgroup that arrives
// last adds the parts in order: score = exp(sum / n)
constexpr int IS_ROWS = 16;
__global__ __launch_bounds__(MT_TPB) void k_is_kl(const float* __restrict__ p, int n, int C, int ld, const double* __restrict__ logm,
                                                  double* __restrict__ part, unsigned* __restrict__ counter, double* __restrict__ score) {
  __shared__ double sh[4];
  __shared__ bool last;
  const int r0 = blockIdx.x * IS_ROWS, r1 = min(n, r0 + IS_ROWS);
  double s = 0.0;
  for (int r = r0; r < r1; ++r)
    for (int c = threadIdx.x; c < C; c += MT_TPB) {
      const float v = p[(int64_t)r * ld + c];
      if (v > 0.0f) s += (double)v * (log((double)v) - logm[c]);
    }
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    __threadfence();
    last = atomicAdd(counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (last && threadIdx.x == 0) {
    __threadfence();
    double t = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) t += ((const volatile double*)part)[b];
    *score = exp(t / (double)n);
  }
}

int knn_splits(int64_t nq, int64_t nc) {                   // row tiles a workgroup column is split over: enough workgroups for the device
  const int64_t qt = (nq + MT - 1) / MT, ct = (nc + MT - 1) / MT;
  int64_t s = (1024 + qt - 1) / qt;
  return (int)(s < 1 ? 1 : (s > ct ? ct : s));
}

bool operand_ok(const float* p, int64_t rows, int cols, int ld) {
  return p && al16(p) && rows > 0 && rows < (1ll << 31) && cols > 0 && cols % 4 == 0 && ld >= cols && ld % 4 == 0 &&
         sfron_fits31(sfron_extent(rows, ld, cols, 4));
}

}  // namespace

extern "C" {

int sfron_gemm_nt_f32(const float* A, int M, int lda, const float* B, int N, int ldb, int K, float* C, int ldc, void* stream) {
  SFRON_CHECK_ARG(operand_ok(A, M, K, lda) && operand_ok(B, N, K, ldb) && C && al4(C) && ldc >= N && sfron_fits31(sfron_extent(M, ldc, N, 4)));
  MTArgs g = {};
  g.A = A; g.B = B; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.C = C; g.ldc = ldc;
  const int rt = cdiv(M, MT);
  hipLaunchKernelGGL(k_nt_tile<EPI_STORE>, dim3(cdiv(N, MT), rt > 65535 ? 65535 : rt), dim3(MT_TPB), 0, (hipStream_t)stream, g);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int64_t sfron_manifold_radii_workspace(int64_t N, int64_t row_batch, int64_t col_batch) {
  if (N <= 0) return 0;
  if (row_batch <= 0 || row_batch > N) row_batch = N;
  if (col_batch <= 0 || col_batch > N) col_batch = N;
  int64_t slots = 0;
  for (int64_t c0 = 0; c0 < N; c0 += col_batch) slots += knn_splits(row_batch, (N - c0 < col_batch ? N - c0 : col_batch));
  return row_batch * slots * MF_KEEP * 4;
}

int sfron_manifold_radii_batched(const float* X, int64_t N, int D, int ld, int64_t row_batch, int64_t col_batch, const int* nhood, int n_nhood,
                                 float* radii, void* workspace, int64_t workspace_bytes, void* stream) {
  SFRON_CHECK_ARG(N > 0 && N < (1ll << 31) && nhood && n_nhood >= 1 && n_nhood <= 4 && radii && al4(radii) && workspace && al16(workspace));
  {                                                        // the 2 GiB rule holds per launch: its operands are a query and a candidate batch
    const int64_t rb = row_batch <= 0 || row_batch > N ? N : row_batch, cb = col_batch <= 0 || col_batch > N ? N : col_batch;
    SFRON_CHECK_ARG(operand_ok(X, rb > cb ? rb : cb, D, ld));
  }
  Nhood nh = {};
  nh.n = n_nhood;
  for (int a = 0; a < n_nhood; ++a) {
    SFRON_CHECK_ARG(nhood[a] >= 1 && nhood[a] < MF_KEEP && N > nhood[a]);
    nh.k[a] = nhood[a];
  }
  if (row_batch <= 0 || row_batch > N) row_batch = N;
  if (col_batch <= 0 || col_batch > N) col_batch = N;
  SFRON_CHECK_ARG(workspace_bytes >= sfron_manifold_radii_workspace(N, row_batch, col_batch));
  int slots = 0;
  for (int64_t c0 = 0; c0 < N; c0 += col_batch) slots += knn_splits(row_batch, (N - c0 < col_batch ? N - c0 : col_batch));
  hipStream_t s = (hipStream_t)stream;
  for (int64_t q0 = 0; q0 < N; q0 += row_batch) {
    const int nq = (int)(N - q0 < row_batch ? N - q0 : row_batch);
    int slot0 = 0;
    for (int64_t c0 = 0; c0 < N; c0 += col_batch) {
      const int nc = (int)(N - c0 < col_batch ? N - c0 : col_batch);
      const int sp = knn_splits(row_batch, nc);
      MTArgs g = {};
      g.A = X + c0 * ld; g.M = nc; g.lda = ld;             // candidates on the row side
      g.B = X + q0 * ld; g.N = nq; g.ldb = ld;             // queries on the lane-owned side
      g.K = D; g.lists = (float*)workspace; g.slots = slots; g.slot0 = slot0; g.splits = sp;
      hipLaunchKernelGGL(k_nt_tile<EPI_KNN>, dim3(cdiv(nq, MT), sp), dim3(MT_TPB), 0, s, g);
      SFRON_LAUNCH_STATUS();
      slot0 += sp;
    }
    hipLaunchKernelGGL(k_knn_select, dim3(cdiv(nq, MT_TPB)), dim3(MT_TPB), 0, s, (const float*)workspace, slots, nq, nh, radii + q0 * n_nhood);
    SFRON_LAUNCH_STATUS();
  }
  return SFRON_OK;
}

int sfron_manifold_radii(const float* X, int64_t N, int D, int ld, const int* nhood, int n_nhood, float* radii, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  return sfron_manifold_radii_batched(X, N, D, ld, N, N, nhood, n_nhood, radii, workspace, workspace_bytes, stream);
}

int sfron_manifold_pr(const float* X1, int64_t N1, const float* r1, int K1, const float* X2, int64_t N2, const float* r2, int K2, int D, int ld1,
                      int ld2, uint8_t* in1, uint8_t* in2, void* stream) {
  SFRON_CHECK_ARG(operand_ok(X1, N1, D, ld1) && operand_ok(X2, N2, D, ld2) && r1 && r2 && al4(r1) && al4(r2) && in1 && in2);
  SFRON_CHECK_ARG(K1 >= 1 && K1 <= 4 && K2 >= 1 && K2 <= 4);
  MTArgs g = {};
  g.A = X1; g.M = (int)N1; g.lda = ld1; g.B = X2; g.N = (int)N2; g.ldb = ld2; g.K = D;
  g.r1 = r1; g.r2 = r2; g.K1 = K1; g.K2 = K2; g.in1 = in1; g.in2 = in2;
  const int rt = cdiv(N1, MT), ct = cdiv(N2, MT);
  int sp = (1024 + ct - 1) / ct;
  sp = sp > rt ? rt : sp;
  hipLaunchKernelGGL(k_nt_tile<EPI_PR>, dim3(ct, sp), dim3(MT_TPB), 0, (hipStream_t)stream, g);
  SFRON_LAUNCH_STATUS();
  return SFRON_OK;
}

int64_t sfron_inception_score_workspace(int64_t N, int C, int split_size) {
  if (N <= 0 || C <= 0 || split_size <= 0) return 0;
  const int64_t n = N < split_size ? N : split_size;
  return ((int64_t)C + (n + IS_ROWS - 1) / IS_ROWS) * 8 + 16;
}

int sfron_inception_score(float* logits, int64_t N, int C, int ld, int split_size, double* scores, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  SFRON_CHECK_ARG(logits && al16(logits) && N > 0 && N < (1ll << 31) && C > 0 && ld >= C && split_size > 0 && scores && ((uintptr_t)scores & 7) == 0 &&
                  workspace && al16(workspace));
  SFRON_CHECK_ARG(sfron_fits31(sfron_extent(N, ld, C, 4)) && workspace_bytes >= sfron_inception_score_workspace(N, C, split_size));
  unsigned* counter = (unsigned*)workspace;
  double* logm = (double*)((char*)workspace + 16);
  double* part = logm + C;
  hipStream_t s = (hipStream_t)stream;
  int k = 0;
  for (int64_t lo = 0; lo < N; lo += split_size, ++k) {
    const int n = (int)(N - lo < split_size ? N - lo : split_size);
    float* p = logits + lo * ld;
    hipLaunchKernelGGL(k_is_softmax, dim3(n), dim3(MT_TPB), 0, s, p, C, ld);
    SFRON_LAUNCH_STATUS();
    hipLaunchKernelGGL(k_is_colmean, dim3(cdiv(C, IS_COLS)), dim3(MT_TPB), 0, s, (const float*)p, n, C, ld, logm, counter);
    SFRON_LAUNCH_STATUS();
    hipLaunchKernelGGL(k_is_kl, dim3(cdiv(n, IS_ROWS)), dim3(MT_TPB), 0, s, (const float*)p, n, C, ld, (const double*)logm, part, counter, scores + k);
    SFRON_LAUNCH_STATUS();
  }
  return SFRON_OK;
}

}  // extern "C"
