// Pillow's antialiased resize of an 8-bit RGB image with the centre crop folded in (the Resize + CenterCrop of
// SD/train-scripts/dataset.py:23-33 on a PIL image: Image.resize, Pillow's separable fixed-point convolution, PRECISION_BITS = 22).
// The filter is evaluated on the host (sfron.resample.resample_tables, float64 -> int32 coefficients); the device only does the integer
// arithmetic, so the result is specified bit for bit:  ss = 2^21 + sum_x src[xmin + x] * k[x] in int32, out = clamp(ss >> 22, 0, 255).
// Horizontal pass first, to uint8 (that rounding is part of the result), then the vertical pass over it.
//
// sfron_image_resample_u8 runs one image in two launches; sfron_image_resample_batch_u8 runs chains of resizes (ADM's center_crop_arr:
// BOX halvings, BICUBIC, crop) for a whole batch in one launch per level, over the same two device functions.
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
// rs_h_tile is that workgroup's work, shared by the single-image and the batched kernel: `row` is the source row (Ws pixels held),
// `org` the index the bounds count from (the first column held; 0 for a whole image), `orow` the output row (Wo pixels).  Every thread
// of the workgroup calls it (it holds the barrier).
__device__ __forceinline__ void rs_h_tile(const uint8_t* row, int Ws, int org, const int32_t* kx, const int32_t* bx, int ksx, int Wo, int x0,
                                          uint8_t* orow, uint32_t* span32) {
  uint8_t* span = reinterpret_cast<uint8_t*>(span32);
  const int xe = min(x0 + RS_TPB, Wo) - 1;
  const int lo = rs_clamp((int64_t)bx[2 * x0] - org, 0, Ws);
  const int hi = rs_clamp((int64_t)bx[2 * xe] - org + bx[2 * xe + 1], lo, Ws);
  const int nbytes = (hi - lo) * 3;
  const bool staged = nbytes <= RS_SPAN;
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
  const int xmin = rs_clamp((int64_t)bx[2 * x] - org, 0, Ws);
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
  uint8_t* o = orow + (int64_t)x * 3;
  o[0] = rs_clip8(s0), o[1] = rs_clip8(s1), o[2] = rs_clip8(s2);
}

__global__ __launch_bounds__(RS_TPB) void k_resample_h(const uint8_t* __restrict__ src, int Hs, int Ws, const int32_t* __restrict__ kx,
                                                       const int32_t* __restrict__ bx, int ksx, const int32_t* __restrict__ by, int Ho,
                                                       int Wo, uint8_t* __restrict__ tmp, int tmp_rows) {
  __shared__ uint32_t span32[RS_SPAN / 4 + 2];
  int y0, nrows;
  rs_rows(by, Ho, Hs, tmp_rows, y0, nrows);
  const int r = blockIdx.x;
  if (r >= nrows) return;                                              // uniform over the workgroup
  rs_h_tile(src + ((int64_t)(y0 + r) * Ws) * 3, Ws, 0, kx, bx, ksx, Wo, blockIdx.y * RS_TPB, tmp + (int64_t)r * Wo * 3, span32);
}

// ---- vertical pass: workgroup = one output row x RS_TPB bytes of it; a thread forms one byte (a channel of a pixel).  Loads run along
// the row (coalesced), the row's coefficients and bounds are the same for every thread (scalar loads).  rs_v_byte is one thread's work,
// shared by both kernels: byte j of output row yy from the `nrows` rows of w3 bytes at `tmp`, whose first row has index `org`.
__device__ __forceinline__ void rs_v_byte(const uint8_t* tmp, int nrows, int64_t w3, int org, const int32_t* ky, const int32_t* by, int ksy,
                                          int yy, int64_t j, uint8_t* dst) {
  const int ymin = rs_clamp((int64_t)by[2 * yy] - org, 0, nrows);
  const int n = rs_clamp(by[2 * yy + 1], 0, min(ksy, nrows - ymin));
  const int32_t* k = ky + (int64_t)yy * ksy;
  const uint8_t* q = tmp + (int64_t)ymin * w3 + j;
  int ss = 1 << (RS_SHIFT - 1);
  for (int i = 0; i < n; ++i) ss += q[(int64_t)i * w3] * k[i];
  dst[(int64_t)yy * w3 + j] = rs_clip8(ss);
}

__global__ __launch_bounds__(RS_TPB) void k_resample_v(const uint8_t* __restrict__ tmp, int tmp_rows, int Hs, const int32_t* __restrict__ ky,
                                                       const int32_t* __restrict__ by, int ksy, int Ho, int Wo, uint8_t* __restrict__ dst) {
  const int64_t w3 = (int64_t)Wo * 3;
  const int64_t j = (int64_t)blockIdx.y * RS_TPB + threadIdx.x;
  if (j >= w3) return;
  int y0, nrows;
  rs_rows(by, Ho, Hs, tmp_rows, y0, nrows);
  rs_v_byte(tmp, nrows, w3, y0, ky, by, ksy, blockIdx.x, j, dst);
}

// ---- the batched form: one launch per level runs that pass of every image of a batch.  blockIdx.z picks the pass record (uniform over
// the workgroup: scalar loads); the grid is sized by the level's largest extents and a workgroup beyond its own pass's extents exits.
// The records are device data nobody on this side has checked, so every offset and extent read from one is clamped into the buffer it
// addresses before it is used: a bad record gives wrong pixels, never an access outside pool / work / out / tables.
struct rs_bufs {
  const uint8_t* pool; int64_t pool_bytes;
  uint8_t* work; int64_t work_bytes;
  uint8_t* out; int64_t out_bytes;
  const int32_t* tab; int64_t n_tab;
};
constexpr int64_t RS_INT_MAX = 2147483647;
constexpr int64_t RS_MAX_PIX = RS_INT_MAX / 3;                        // pixels of a row whose byte count is an `int`

__device__ __forceinline__ int64_t rs_clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the tables of a pass, cut to the blob: ksize >= 1, n_out outputs whose coefficients and bounds lie inside it
__device__ __forceinline__ void rs_pass_tables(const rs_bufs& B, const sfron_resample_pass& p, const int32_t*& k, const int32_t*& b, int& ks,
                                               int& n_out) {
  ks = (int)rs_clamp64(p.ksize, 1, RS_INT_MAX);
  const int64_t k_off = rs_clamp64(p.k_off, 0, B.n_tab), b_off = rs_clamp64(p.b_off, 0, B.n_tab);
  const int64_t fit = rs_clamp64((B.n_tab - k_off) / ks, 0, (B.n_tab - b_off) / 2);
  n_out = (int)rs_clamp64(p.n_out, 0, rs_clamp64(fit, 0, RS_MAX_PIX));
  k = B.tab + k_off, b = B.tab + b_off;
}

// rows of `pitch` bytes that fit between `off` (already inside [0, cap]) and cap
__device__ __forceinline__ int rs_rows_that_fit(int64_t want, int64_t off, int64_t cap, int64_t pitch) {
  return pitch > 0 ? (int)rs_clamp64(want, 0, rs_clamp64((cap - off) / pitch, 0, RS_INT_MAX)) : 0;
}

__global__ __launch_bounds__(RS_TPB) void k_resample_batch_h(rs_bufs B, const sfron_resample_pass* __restrict__ passes, int first) {
  __shared__ uint32_t span32[RS_SPAN / 4 + 2];
  const sfron_resample_pass p = passes[first + blockIdx.z];
  const bool from_pool = p.in_buf == SFRON_RESAMPLE_POOL;
  const uint8_t* in = from_pool ? B.pool : B.work;
  const int64_t in_cap = from_pool ? B.pool_bytes : B.work_bytes;
  const int64_t in_off = rs_clamp64(p.in_off, 0, in_cap);
  const int Ws = (int)rs_clamp64(p.in_w, 0, RS_MAX_PIX);
  const int in_h = rs_rows_that_fit(p.in_h, in_off, in_cap, (int64_t)Ws * 3);
  const int row0 = (int)rs_clamp64(p.row0, 0, in_h);
  const int32_t *k, *b;
  int ks, Wo;
  rs_pass_tables(B, p, k, b, ks, Wo);
  const int64_t out_off = rs_clamp64(p.out_off, 0, B.work_bytes);    // a horizontal pass writes the work buffer only
  const int nrows = rs_rows_that_fit(rs_clamp64(p.nrows, 0, in_h - row0), out_off, B.work_bytes, (int64_t)Wo * 3);
  const int r = blockIdx.x, x0 = blockIdx.y * RS_TPB;
  if (r >= nrows || x0 >= Wo) return;                                  // uniform over the workgroup
  const int org = (int)rs_clamp64(p.org, -RS_INT_MAX / 2, RS_INT_MAX / 2);
  rs_h_tile(in + in_off + (int64_t)(row0 + r) * Ws * 3, Ws, org, k, b, ks, Wo, x0, B.work + out_off + (int64_t)r * Wo * 3, span32);
}

__global__ __launch_bounds__(RS_TPB) void k_resample_batch_v(rs_bufs B, const sfron_resample_pass* __restrict__ passes, int first) {
  const sfron_resample_pass p = passes[first + blockIdx.z];
  const int64_t in_off = rs_clamp64(p.in_off, 0, B.work_bytes);      // a vertical pass reads the work buffer only
  const int64_t w3 = rs_clamp64(p.in_w, 0, RS_MAX_PIX) * 3;
  const int in_h = rs_rows_that_fit(p.in_h, in_off, B.work_bytes, w3);
  const int32_t *k, *b;
  int ks, Ho;
  rs_pass_tables(B, p, k, b, ks, Ho);
  const bool to_out = p.out_buf == SFRON_RESAMPLE_OUT;
  uint8_t* o = to_out ? B.out : B.work;
  const int64_t out_cap = to_out ? B.out_bytes : B.work_bytes;
  const int64_t out_off = rs_clamp64(p.out_off, 0, out_cap);
  Ho = rs_rows_that_fit(Ho, out_off, out_cap, w3);
  const int yy = blockIdx.x;
  const int64_t j = (int64_t)blockIdx.y * RS_TPB + threadIdx.x;
  if (yy >= Ho || j >= w3) return;
  const int org = (int)rs_clamp64(p.org, -RS_INT_MAX / 2, RS_INT_MAX / 2);
  rs_v_byte(B.work + in_off, in_h, w3, org, k, b, ks, yy, j, o + out_off);
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

int sfron_image_resample_batch_u8(const uint8_t* pool, int64_t pool_bytes, const int32_t* tables, int64_t n_tables,
                                  const sfron_resample_pass* passes, int n_passes, const int32_t* level_first, const int32_t* level_rows,
                                  const int32_t* level_cols, int n_levels, uint8_t* work, int64_t work_bytes, uint8_t* out, int64_t out_bytes,
                                  void* stream) {
  SFRON_CHECK_ARG(pool && tables && passes && level_first && level_rows && level_cols && work && out);
  SFRON_CHECK_ARG(pool_bytes > 0 && n_tables > 0 && n_passes > 0 && n_levels > 0 && work_bytes > 0 && out_bytes > 0);
  SFRON_CHECK_ARG(n_levels % 2 == 0);                                  // a stage is a horizontal and a vertical level
  SFRON_CHECK_ARG(level_first[0] == 0 && level_first[n_levels] == n_passes);
  for (int l = 0; l < n_levels; ++l) {
    SFRON_CHECK_ARG(level_first[l + 1] > level_first[l] && level_first[l + 1] - level_first[l] <= 65535);
    SFRON_CHECK_ARG(level_rows[l] > 0 && level_cols[l] > 0 && cdiv(level_cols[l], RS_TPB) <= 65535);
    // what the largest extents imply: some pass of the level has level_rows rows (of a pixel at least), some has level_cols columns
    const int64_t px = level_rows[l] > level_cols[l] ? level_rows[l] : level_cols[l];
    if (l % 2 == 0) SFRON_CHECK_ARG(work_bytes >= 3 * px);             // columns of a horizontal level are pixels it writes to work
    if (l == 0) SFRON_CHECK_ARG(pool_bytes >= 3ll * level_rows[0]);    // the first level reads its rows from the pool
    if (l == n_levels - 1) SFRON_CHECK_ARG(out_bytes >= 3ll * level_rows[l] && out_bytes >= level_cols[l]);   // (bytes of a row it writes to out)
  }
  const rs_bufs B = {pool, pool_bytes, work, work_bytes, out, out_bytes, tables, n_tables};
  for (int l = 0; l < n_levels; ++l) {
    const dim3 grid((unsigned)level_rows[l], (unsigned)cdiv(level_cols[l], RS_TPB), (unsigned)(level_first[l + 1] - level_first[l]));
    if (l % 2 == 0)
      hipLaunchKernelGGL(k_resample_batch_h, grid, dim3(RS_TPB), 0, (hipStream_t)stream, B, passes, level_first[l]);
    else
      hipLaunchKernelGGL(k_resample_batch_v, grid, dim3(RS_TPB), 0, (hipStream_t)stream, B, passes, level_first[l]);
    SFRON_LAUNCH_STATUS();
  }
  return SFRON_OK;
}

}  // extern "C"
