// Fused multi-head self-attention (non-causal, no dropout) forward and backward for the DiT block.
//
// Replaces timm Attention's softmax(q * hd^-0.5 @ k^T) @ v (used at /root/reference/DiT/models.py:108,120;
// timm is un-vendored: behaviour per SURVEY.md section 8c) and autograd's backward of it.
// Layout: qkv is the fused-QKV GEMM output [B*T][3*D] bf16 with column = which*D + head*hd + d
// (== reshape(B,N,3,H,hd)); o / d_o are [B*T][D] with column = head*hd + d (== transpose(1,2).reshape).
//
// Flash-style: scores never touch HBM.  All three kernels put the SOFTMAX ROW on the MFMA lane
// (S^T = K·Q^T is what the matrix core computes), so row max / row sum / rescale are lane-local, the
// probabilities feed the next MFMA straight from registers (k-slot permutation, no LDS round trip)
// and V / K / Q / dO tiles are consumed both row-wise (ds_read_b128) and column-wise
// (ds_read_b64_tr_b16) from ONE swizzled LDS image.
//   forward : grid (T / (64*QT), B*H); wave = 16*QT queries, streams 64-key chunks of K,V
//   dQ      : same decomposition; recomputes P from LSE
//   dK,dV   : wave = 16 keys, streams 64-query chunks of Q,dO; no cross-workgroup reduction
// 64-row chunks arrive by LDS-DMA (buffer_load ... lds, swizzle on the source address, pad columns never
// written) into a 3-slot ring: chunk c+2 is in flight while chunk c feeds the matrix cores, one raw
// s_barrier per chunk, counted vmcnt.
// head_dim 64 -> 128-B image rows, 2 k-steps, 4 d-tiles; head_dim 72 (DiT-XL) -> 192-B rows (96 columns,
// zero padded), 3 k-steps, 5 d-tiles.
#include "common.h"
#include "tile.h"
#include "../../include/sfron.h"

namespace {

constexpr int NT = 256, NWAVE = 4, NSLOT = 3;
constexpr float LOG2E = 1.4426950408889634f;

// chunk-index XOR of image row r (bank rules of MI355X_MICROARCH.md section LDS; both the ds_read_b128 row
// fragments and the transposed reads are conflict-free):
//   HDP 64 (128-B rows, 8 chunks):  ((r>>1)&3)<<1
//   HDP 96 (192-B rows, 12 chunks): perm[(r>>2)&3], perm = {0,2,3,1}  (stays inside each 4-chunk group)
template <int HDP> __device__ __forceinline__ int aswz(int row) {
  if (HDP == 64) return ((row >> 1) & 3) << 1;
  return (0x1320 >> (((row >> 2) & 3) * 4)) & 3;
}
template <int HDP> __device__ __forceinline__ int aoff(int row, int ch) { return row * HDP + ((ch ^ aswz<HDP>(row)) << 3); }

// LDS-DMA plan for one [64 rows][hd] chunk: per-lane byte offsets (loop invariant) + validity (pad chunks are
// never written: the images are zeroed once).  One wave-instruction fills 1 KiB of the lane-linear image.
template <int HDP>
struct ChunkDma {
  static constexpr int CPR = HDP / 8;                  // 16-B chunk positions per image row
  static constexpr int PER_WAVE = CPR / NWAVE;         // 64 rows * CPR chunks / 64 lanes / 4 waves
  static_assert(CPR % NWAVE == 0, "image rows must split over the waves");
  int off[PER_WAVE];
  bool valid[PER_WAVE];
  __device__ __forceinline__ void init(int ld, int hd, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int e = (wave + i * NWAVE) * 64 + lane;
      const int row = e / CPR, p = e % CPR;
      const int c = p ^ aswz<HDP>(row);                // source chunk that lives at position p
      valid[i] = c * 8 < hd;
      off[i] = 2 * (row * ld + c * 8);
    }
  }
  __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rsrc, int soff_bytes, __bf16* img, int wave) const {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i)
      if (valid[i])
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t*)(img + (wave + i * NWAVE) * 512), 16, off[i], soff_bytes, 0, 0);
  }
};

// Zero the PAD chunk positions (source chunk index >= hd/8) of n_img images that lie IMG_STEP images apart.  The DMA never writes them and
// writes nothing else than the valid positions, so zeroing and DMA touch disjoint LDS bytes and need no ordering between them.  One thread
// per image row writes that row's pad chunks directly (position = chunk ^ swizzle(row)): rounds 1-3 walked every chunk position of every
// image with a predicate -- 18 iterations of index arithmetic per thread, 2.0 of the 12.4 us a forward workgroup lives
// (tools/attn_probe.py, profiles/r04_attn_phases.txt).
// Which images need it: a ROW fragment of k-step hd/32 reaches into the pad columns, and 0 x garbage is NaN when the garbage is -- so every
// image read by rows (K; Q / dO / V in the backward kernels).  An image read only by COLUMN fragments (V in the forward pass) feeds pad
// columns into output columns >= hd, which are never stored: it needs no zeroing.
template <int HDP, int NTHR, int IMG_STEP = 1> __device__ __forceinline__ void zero_pads(__bf16* p, int n_img, int hd, int tid) {
  constexpr int CPR = HDP / 8;
  if (hd >= HDP) return;
  const uint4 z = make_uint4(0, 0, 0, 0);
  const int c0 = hd >> 3;
  for (int r = tid; r < n_img * 64; r += NTHR) {
    const int sw = aswz<HDP>(r & 63);
    uint4* const rowp = reinterpret_cast<uint4*>(p) + ((r >> 6) * IMG_STEP * 64 + (r & 63)) * CPR;
    for (int c = c0; c < CPR; ++c) rowp[c ^ sw] = z;
  }
}

// row fragment: lane holds X[row0 + (lane&15)][32*ks + 8*(lane>>4) + 0..7]
template <int HDP> __device__ __forceinline__ bf16x8 frag_rows(const __bf16* img, int row0, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + aoff<HDP>(row0 + (lane & 15), ks * 4 + (lane >> 4)));
}
// column fragment with the PERMUTED k-slot map used by the register-resident probabilities:
// lane holds X[rows r = rbase + 4g + j (j<4) and rbase + 16 + 4g + (j-4)][col0 + (lane&15)], g = lane>>4
template <int HDP> __device__ __forceinline__ bf16x8 frag_cols_perm(const __bf16* img, int rbase, int col0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int ch = (col0 >> 3) + (p >> 1);
  const int r0 = rbase + 4 * g + q;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + aoff<HDP>(r0, ch) + 4 * (p & 1)));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(img + aoff<HDP>(r0 + 16, ch) + 4 * (p & 1)));
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}
// Permuted column fragments (frag_cols_perm) as base register + immediate: for a lane, the chunk swizzle of its rows
// (4g + q and 16 + 4g + q of a 32-row step) is one constant, and XOR by it is affine in the d-tile index within a
// 4-chunk group (HDP 96: two base registers, even / odd d-tile) -- so the per-(d-tile, k-step, half) addresses that hipcc
// otherwise hoists out of the chunk loop and spills are immediates.
template <int HDP> struct ColPerm {
  static constexpr int NB = HDP == 96 ? 2 : HDP / 16;
  int b[NB];                                   // byte offsets inside an image
  __device__ __forceinline__ void init(int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
#pragma unroll
    for (int k = 0; k < NB; ++k) b[k] = 2 * (aoff<HDP>(4 * g + q, 2 * k + (p >> 1)) + 4 * (p & 1));
  }
  static constexpr int sel(int dt) { return HDP == 96 ? (dt & 1) : dt; }
  static constexpr int imm(int dt, int s2, int hi) { return 2 * ((HDP == 96 ? 32 * (dt >> 1) : 0) + (32 * s2 + 16 * hi) * HDP); }
};
template <int HDP, int DT, int S2> __device__ __forceinline__ bf16x8 col_frag(const unsigned (&a)[ColPerm<HDP>::NB]) {
  const bf16x4 lo = asm_read_tr_off<ColPerm<HDP>::imm(DT, S2, 0)>(a[ColPerm<HDP>::sel(DT)]);
  const bf16x4 hi = asm_read_tr_off<ColPerm<HDP>::imm(DT, S2, 1)>(a[ColPerm<HDP>::sel(DT)]);
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ void asm_write_b64(unsigned addr, bf16x4 v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// frag_cols_perm through the asm reads of tile.h (the builtin would serialise the 3-slot ring); the caller runs lds_reads_done()
template <int HDP> __device__ __forceinline__ bf16x8 frag_cols_perm_asm(const __bf16* img, int rbase, int col0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int ch = (col0 >> 3) + (p >> 1);
  const int r0 = rbase + 4 * g + q;
  const unsigned base = lds_addr(img);
  const bf16x4 lo = asm_read_tr(base + 2 * (aoff<HDP>(r0, ch) + 4 * (p & 1)));
  const bf16x4 hi = asm_read_tr(base + 2 * (aoff<HDP>(r0 + 16, ch) + 4 * (p & 1)));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ bf16x8 pack_perm(const f32x4& a, const f32x4& b) {
  bf16x8 r;
  r[0] = f2bf(a[0]); r[1] = f2bf(a[1]); r[2] = f2bf(a[2]); r[3] = f2bf(a[3]);
  r[4] = f2bf(b[0]); r[5] = f2bf(b[1]); r[6] = f2bf(b[2]); r[7] = f2bf(b[3]);
  return r;
}
// wave's own rows straight from global: lane holds X[row0 + (lane&15)][32*ks + 8*(lane>>4) + 0..7], zero beyond hd
__device__ __forceinline__ bf16x8 frag_rows_global(const __bf16* base, int ld, int row0, int ks, int hd, int lane) {
  const int d = 32 * ks + 8 * (lane >> 4);
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.0f;
  if (d >= hd) return z;
  return *reinterpret_cast<const bf16x8*>(base + (size_t)(row0 + (lane & 15)) * ld + d);
}
// over the 4 lane groups (lanes i, i + 16, i + 32, i + 48) that hold one softmax row.  (gfx950's v_permlane16_swap / v_permlane32_swap do
// the same in two vector operations per step instead of a ds_bpermute round trip; measured: no change -- forward 31.9 us either way -- and
// the instructions need care under hipcc 7.2, tools/probes/permlane_probe.hip; the shuffles stay.)
__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// One row block of NDT horizontally adjacent 16 x 16 bf16 tiles -> global: v[dt] = this lane's 4 columns (4 g ..) of tile dt.  Tile pairs
// leave as ONE 16-byte store per lane (common.h pair_pack: the store tail of these kernels is issue-bound), an odd last tile as 8 bytes;
// columns >= hd (hd % 8 == 0, so a piece is valid whole or not at all) are not written.  Every lane runs the swaps; only stores are masked.
template <int NDT> __device__ __forceinline__ void store_tiles(__bf16* row, const bf16x4 (&v)[NDT], int hd, int g) {
#pragma unroll
  for (int np = 0; np < NDT / 2; ++np) {
    const uint4 pk = pair_pack(v[2 * np], v[2 * np + 1]);
    const int c = 32 * np + pair_col(g);
    if (c < hd) *reinterpret_cast<uint4*>(row + c) = pk;
  }
  if constexpr (NDT & 1) {
    const int d = (NDT - 1) * 16 + 4 * g;
    if (d < hd) *reinterpret_cast<bf16x4*>(row + d) = v[NDT - 1];
  }
}
__device__ __forceinline__ bf16x4 to_bf16x4(const f32x4& v) { return bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])}; }

// Ring driver shared by the three kernels.  Two images (X0, X1) per slot.  Usage per chunk c:
//   ring_wait<...>(c, n) ; barrier ; ring_issue(c + 2) ; compute(slot c % 3)
template <int HDP>
struct Ring {
  static constexpr int IMG = 64 * HDP;                 // elements per image
  static constexpr int PER_CHUNK = 2 * ChunkDma<HDP>::PER_WAVE;   // DMA instructions per wave per chunk (2 images)
  __bf16* base;
  __device__ __forceinline__ __bf16* img(int slot, int which) const { return base + (slot * 2 + which) * IMG; }
};

constexpr int FNW = 8, FNT = FNW * 64;
// LDS-DMA plan for a group of 64-row images (each [64][hd] rows of a row-major tensor): instruction j of the group fills
// piece (j % CPR) of image (j / CPR); the FNW waves take j = wave + FNW * i.
template <int HDP, int NIMG>
struct GroupDma {
  static constexpr int CPR = HDP / 8;
  static constexpr int PER_WAVE = NIMG * CPR / FNW;
  static_assert((NIMG * CPR) % FNW == 0, "pieces must split over the waves");
  int off[PER_WAVE];
  bool valid[PER_WAVE];
  // ld_of(img) / base offset (elements) of image img are wave-uniform
  template <class LD> __device__ __forceinline__ void init(LD ld_of, int hd, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int j = wave + FNW * i, img = j / CPR, jj = j % CPR;
      const int e = jj * 64 + lane, row = e / CPR, p = e % CPR;
      const int c = p ^ aswz<HDP>(row);
      valid[i] = c * 8 < hd;
      off[i] = 2 * (row * ld_of(img) + c * 8);
    }
  }
};
}  // namespace (kernel templates have external linkage + explicit instantiations below: see gemm.hip)

#ifdef SFRON_DEBUG_KNOBS
// diagnostic build only (tools/attn_probe.py): per-workgroup phase stamps of the constant 100 MHz counter, [workgroup][8]; slot 7 = HW_ID.
// The stamps go to a buffer of their own; no output value depends on them.
__device__ long long* d_attn_clk = nullptr;
#define ATTN_STAMP(i) do { if (clk__) clk__[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#define ATTN_STAMP_INIT() long long* clk__ = (d_attn_clk && threadIdx.x == 0 && blockIdx.x < 4096) ? d_attn_clk + 8 * blockIdx.x : nullptr; \
  if (clk__) clk__[7] = (long long)__builtin_amdgcn_s_getreg(63492) | ((long long)__builtin_amdgcn_s_getreg(63508) << 32)
#if defined(SFRON_ATTN_PROBE) && SFRON_ATTN_PROBE == 2      // second stamp set: inside the prologue (slots 1..4), the loop's stamps off
#define ATTN_STAMP_P(i) ATTN_STAMP(i)
#define ATTN_STAMP_L(i) do { } while (0)
#else
#define ATTN_STAMP_P(i) do { } while (0)
#define ATTN_STAMP_L(i) ATTN_STAMP(i)
#endif
#else
#define ATTN_STAMP(i) do { } while (0)
#define ATTN_STAMP_P(i) do { } while (0)
#define ATTN_STAMP_L(i) do { } while (0)
#define ATTN_STAMP_INIT() do { } while (0)
#endif

// ------------------------------------------------------------------------------------- forward
// NWV = 4: a workgroup = 4 waves = 64 QT query rows.  NWV = 8 (round 4 experiment, sfron_attn_fwd_form(16)): eight waves = 128 QT rows = with
// QT = 2 the WHOLE head at T = 256, so its K / V chunks are brought in once, not once per query block (per CU the memory-bound start of a round
// moves 73 KB instead of 110, profiles/r04_attn_phases.txt).  Same products, same order per row: bit-identical -- and slower (one workgroup
// per CU instead of two, eight waves behind each chunk's barrier): kept as a form the tests compare, not taken by rule.
// NIT = 2 (round 6, sfron_attn_fwd_form(2); a form the tests compare, not the rule): ONE workgroup walks the NIT consecutive query blocks of a head as one stream of NIT * T / 64 chunks through
// the same ring -- the next block's first K / V chunks (the SAME K / V: L2 hits) arrive while the current block finishes, its Q fragments are
// requested under the current block's last chunk, and the current block's output stores drain under the next block's first chunk.  A launch is
// then one round of resident workgroups (DiT-XL/2: 512 = two per CU) instead of two rounds that each pay the memory-bound prologue
// (profiles/r04_attn_phases.txt: 2.6 of the 10.5 us a workgroup lives, + 0.9 us of epilogue).  Same products, same chunk order, same softmax
// arithmetic per row: bit-identical to NIT = 1.
template <int HDP, int KS, int NDT, int QT, int NWV = 4, int NIT = 1>
__global__ __launch_bounds__(NWV * 64) void k_attn_fwd(const __bf16* __restrict__ qkv, __bf16* __restrict__ o,
                                                       float* __restrict__ lse, int T, int H, int hd, float scale) {
  static_assert(NWV == 4 || NWV == FNW, "four or eight waves");
  static_assert(NIT == 1 || NWV == 4, "several query blocks per workgroup: four-wave form only");
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  Ring<HDP> ring{smem};
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  ATTN_STAMP_INIT(); ATTN_STAMP(0);
  // 1-D grid.  Workgroup ids go round-robin over the 8 XCDs: id -> (id & 7) * (n / 8) + (id >> 3) gives each XCD one contiguous run of
  // (batch, head, query block) triples, so the query blocks of a head (same K / V) and the neighbouring heads of a sample (neighbouring
  // 144-B column slices of the same rows: shared 128-B lines) meet in ONE L2
  const int nblk = gridDim.x, nqb = T / (NWV * 16 * QT * NIT);
  const int wid = (nblk & 7) == 0 ? (blockIdx.x & 7) * (nblk >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int bh = wid / nqb, b = bh / H, h = bh % H;
  const int D = H * hd, ld = 3 * D;
  const int qbase = (wid % nqb) * (NWV * 16 * QT * NIT) + wave * (16 * QT);        // + it * NWV * 16 * QT for query block `it` of this workgroup
  const __bf16* base = qkv + (size_t)b * T * ld + h * hd;
  const float c = scale * LOG2E;
  const int nchunk = T / 64, total = NIT * nchunk;                                  // chunks per query block / per workgroup

  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)(base + D), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(base + 2 * D), 0, 0x7fffffff, 0x00020000);
  ChunkDma<HDP> dma;                  // four waves: each wave fills its share of the K image, then of the V image
  GroupDma<HDP, 2> dma8;              // eight waves: the pieces of the (K, V) image pair dealt over the waves
  if constexpr (NWV == 4) dma.init(ld, hd, wave, lane);
  else dma8.init([&](int) { return ld; }, hd, wave, lane);
  constexpr int PER_CHUNK = NWV == 4 ? Ring<HDP>::PER_CHUNK : GroupDma<HDP, 2>::PER_WAVE;      // DMA instructions per wave and chunk
  auto issue = [&](int gch) {                          // gch: position in the workgroup's chunk stream; the K / V chunk is gch % nchunk
    const int slot = gch % NSLOT, soff = (NIT == 1 ? gch : gch % nchunk) * 64 * ld * 2;
    if constexpr (NWV == 4) {
      dma.issue(rsK, soff, ring.img(slot, 0), wave);
      dma.issue(rsV, soff, ring.img(slot, 1), wave);
    } else {
      constexpr int CPR = HDP / 8;
#pragma unroll
      for (int i = 0; i < GroupDma<HDP, 2>::PER_WAVE; ++i) {
        const int j = wave + FNW * i, img = j / CPR, jj = j % CPR;
        if (dma8.valid[i]) dma16(img ? rsV : rsK, ring.img(slot, img) + jj * 512, dma8.off[i], soff);
      }
    }
  };
  // the Q fragments go out BEFORE the LDS-DMA of the first two K / V chunks: vector-memory operations retire in order, so loads
  // issued behind the DMA would keep the first S = Q K^T waiting for chunk 1 as well
  bf16x8 fq[QT][KS], fqn[QT][KS];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fq[qi][ks] = frag_rows_global(base, ld, qbase + 16 * qi, ks, hd, lane);
  ATTN_STAMP_P(1);
  issue(0);                              // first two chunks stream in while the pads are zeroed
  if (total > 1) issue(1);
  ATTN_STAMP_P(2);
  zero_pads<HDP, NWV * 64, 2>(smem, NSLOT, hd, tid);       // the K images (even ring images); V is read by columns only
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // pad zeros written before the first barrier of the loop
  ATTN_STAMP_P(3);

  f32x4 oacc[QT][NDT];
  float m[QT], l[QT];
#pragma unroll 1
  for (int it = 0; it < NIT; ++it) {
  const int q0 = qbase + it * (NWV * 16 * QT);
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    m[qi] = -INFINITY; l[qi] = 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) oacc[qi][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int kc = 0; kc < nchunk; ++kc) {
    const int gc = it * nchunk + kc;
    // chunk gc has landed.  Younger vector-memory operations of this wave: the DMA of chunk gc + 1 and -- across a query-block boundary -- the
    // previous block's output stores and this block's Q fragments, all issued BEHIND that DMA; waiting until no more than one chunk's DMA
    // instructions are outstanding therefore only waits for more than is needed (operations retire in order)
    if (gc + 1 < total) wait_vmcnt<PER_CHUNK>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (gc == 0) ATTN_STAMP_P(4);
    if (gc < 5) ATTN_STAMP_L(1 + gc);
    if (gc + 2 < total) issue(gc + 2);
    if constexpr (NIT > 1) {
      if (kc == nchunk - 1 && it + 1 < NIT) {              // the next query block's Q fragments, requested under this block's last chunk
#pragma unroll
        for (int qi = 0; qi < QT; ++qi)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) fqn[qi][ks] = frag_rows_global(base, ld, q0 + NWV * 16 * QT + 16 * qi, ks, hd, lane);
      }
    }
    const __bf16* iK = ring.img(gc % NSLOT, 0);
    const __bf16* iV = ring.img(gc % NSLOT, 1);
    f32x4 s[QT][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      bf16x8 fk[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) fk[ks] = frag_rows<HDP>(iK, kt * 16, ks, lane);
#pragma unroll
      for (int qi = 0; qi < QT; ++qi) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk[ks], fq[qi][ks], a, 0, 0, 0);
        s[qi][kt] = a;     // S[q = q0+16qi+(lane&15)][key = 64kc + 16kt + 4g + j]
      }
    }
    bf16x8 pf[QT][2];
    bf16x8 fv0[NDT], fv1[NDT];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) fv0[dt] = frag_cols_perm_asm<HDP>(iV, 0, dt * 16, lane);   // in flight under the softmax
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[qi][kt][j]);
      mx = group_max(mx);
      const float mn = fmaxf(m[qi], mx);
      const float alpha = fast_exp2((m[qi] - mn) * c);
      m[qi] = mn;
      const float mc = mn * c;
      float ps = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = fast_exp2(__builtin_fmaf(s[qi][kt][j], c, -mc));
          s[qi][kt][j] = p;
          ps += p;
        }
      l[qi] = l[qi] * alpha + ps;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) oacc[qi][dt] *= alpha;
      pf[qi][0] = pack_perm(s[qi][0], s[qi][1]);
      pf[qi][1] = pack_perm(s[qi][2], s[qi][3]);
    }
    lds_reads_done();
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) fv1[dt] = frag_cols_perm_asm<HDP>(iV, 32, dt * 16, lane);  // ... and under the first PV half
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int qi = 0; qi < QT; ++qi)
        oacc[qi][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv0[dt], pf[qi][0], oacc[qi][dt], 0, 0, 0);
    lds_reads_done();
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int qi = 0; qi < QT; ++qi)
        oacc[qi][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv1[dt], pf[qi][1], oacc[qi][dt], 0, 0, 0);
  }
  ATTN_STAMP(5);
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    const float lt = group_sum(l[qi]);
    const float inv = 1.0f / lt;
    const int q = q0 + 16 * qi + (lane & 15);
    __bf16* orow = o + ((size_t)b * T + q) * D + h * hd;
    bf16x4 ov[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) ov[dt] = to_bf16x4(oacc[qi][dt] * inv);
    store_tiles<NDT>(orow, ov, hd, g);
    if (g == 0) lse[(size_t)bh * T + q] = m[qi] * scale + logf(lt);
  }
  if constexpr (NIT > 1) {
    if (it + 1 < NIT) {
#pragma unroll
      for (int qi = 0; qi < QT; ++qi)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) fq[qi][ks] = fqn[qi][ks];
    }
  }
  }   // query blocks of this workgroup
  ATTN_STAMP(6);
}

// ------------------------------------------------------------------------------------- dQ
template <int HDP, int KS, int NDT, int QT>
__global__ __launch_bounds__(NT) void k_attn_bwd_dq(const __bf16* __restrict__ qkv, const __bf16* __restrict__ o,
                                                    const __bf16* __restrict__ d_o, const float* __restrict__ lse,
                                                    float* __restrict__ delta, __bf16* __restrict__ dqkv, int T, int H, int hd,
                                                    float scale) {
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  Ring<HDP> ring{smem};
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = gridDim.x, nqb = T / (64 * QT);        // XCD-contiguous (batch, head, query block) order: see k_attn_fwd
  const int wid = (nblk & 7) == 0 ? (blockIdx.x & 7) * (nblk >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int bh = wid / nqb, b = bh / H, h = bh % H;
  const int D = H * hd, ld = 3 * D;
  const int q0 = (wid % nqb) * (64 * QT) + wave * (16 * QT);
  const __bf16* base = qkv + (size_t)b * T * ld + h * hd;
  const __bf16* dob = d_o + (size_t)b * T * D + h * hd;
  const __bf16* ob = o + (size_t)b * T * D + h * hd;
  const float c = scale * LOG2E;
  const int nchunk = T / 64;

  ChunkDma<HDP> dma;
  dma.init(ld, hd, wave, lane);
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)(base + D), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(base + 2 * D), 0, 0x7fffffff, 0x00020000);
  auto issue = [&](int ch) {
    const int slot = ch % NSLOT, soff = ch * 64 * ld * 2;
    dma.issue(rsK, soff, ring.img(slot, 0), wave);
    dma.issue(rsV, soff, ring.img(slot, 1), wave);
  };
  issue(0);
  if (nchunk > 1) issue(1);
  bf16x8 fq[QT][KS], fdo[QT][KS];
  float nl[QT], dl[QT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    // delta[q] = sum_d dO[q,d] * O[q,d] of this wave's own rows, from the same fragment layout as dO: a lane holds
    // 8 elements per k-step of row (lane & 15); the 4 lane groups of a row are summed with two shuffles.  Written out
    // for the dK/dV kernel, which runs after this one on the same stream (the separate delta kernel is gone).
    float dsum = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      fq[qi][ks] = frag_rows_global(base, ld, q0 + 16 * qi, ks, hd, lane);
      fdo[qi][ks] = frag_rows_global(dob, D, q0 + 16 * qi, ks, hd, lane);
      const bf16x8 fo = frag_rows_global(ob, D, q0 + 16 * qi, ks, hd, lane);
#pragma unroll
      for (int j = 0; j < 8; ++j) dsum += bf2f(fdo[qi][ks][j]) * bf2f(fo[j]);
    }
    const int q = q0 + 16 * qi + (lane & 15);
    nl[qi] = -lse[(size_t)bh * T + q] * LOG2E;
    dl[qi] = group_sum(dsum);
    if (lane < 16) delta[(size_t)bh * T + q] = dl[qi];
  }
  zero_pads<HDP, NT>(smem, NSLOT * 2, hd, tid);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  f32x4 dq[QT][NDT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dq[qi][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc = 0; kc < nchunk; ++kc) {
    if (kc + 1 < nchunk) wait_vmcnt<Ring<HDP>::PER_CHUNK>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (kc + 2 < nchunk) issue(kc + 2);
    const __bf16* iK = ring.img(kc % NSLOT, 0);
    const __bf16* iV = ring.img(kc % NSLOT, 1);
    bf16x8 ds[QT][2];
    f32x4 t[QT][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      bf16x8 fk[KS], fv[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) { fk[ks] = frag_rows<HDP>(iK, kt * 16, ks, lane); fv[ks] = frag_rows<HDP>(iV, kt * 16, ks, lane); }
#pragma unroll
      for (int qi = 0; qi < QT; ++qi) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk[ks], fq[qi][ks], a, 0, 0, 0);     // S
          p = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv[ks], fdo[qi][ks], p, 0, 0, 0);    // dP
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pr = fast_exp2(__builtin_fmaf(a[j], c, nl[qi]));
          a[j] = pr * (p[j] - dl[qi]) * scale;                                             // dS (incl. softmax scale)
        }
        t[qi][kt] = a;
      }
    }
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) { ds[qi][0] = pack_perm(t[qi][0], t[qi][1]); ds[qi][1] = pack_perm(t[qi][2], t[qi][3]); }
    {
      bf16x8 fk0[NDT], fk1[NDT];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) fk0[dt] = frag_cols_perm_asm<HDP>(iK, 0, dt * 16, lane);
      lds_reads_done();
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) fk1[dt] = frag_cols_perm_asm<HDP>(iK, 32, dt * 16, lane);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int qi = 0; qi < QT; ++qi)
          dq[qi][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk0[dt], ds[qi][0], dq[qi][dt], 0, 0, 0);
      lds_reads_done();
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int qi = 0; qi < QT; ++qi)
          dq[qi][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk1[dt], ds[qi][1], dq[qi][dt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    const int q = q0 + 16 * qi + (lane & 15);
    __bf16* row = dqkv + ((size_t)b * T + q) * ld + h * hd;
    bf16x4 ov[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) ov[dt] = to_bf16x4(dq[qi][dt]);
    store_tiles<NDT>(row, ov, hd, g);
  }
}

// ------------------------------------------------------------------------------------- dK, dV
// wave owns 16*KT keys; S / dP are computed with the KEY on the lane: S[q = 4g+j][key = lane&15]
template <int HDP, int KS, int NDT, int KT>
__global__ __launch_bounds__(NT) void k_attn_bwd_dkv(const __bf16* __restrict__ qkv, const __bf16* __restrict__ d_o,
                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                     __bf16* __restrict__ dqkv, int T, int H, int hd, float scale) {
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  Ring<HDP> ring{smem};
  float* s_lse = reinterpret_cast<float*>(smem + NSLOT * 2 * Ring<HDP>::IMG);     // [T] -lse*log2e, then [T] delta
  float* s_del = s_lse + T;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = gridDim.x, nkb = T / (64 * KT);        // XCD-contiguous (batch, head, key block) order: see k_attn_fwd
  const int wid = (nblk & 7) == 0 ? (blockIdx.x & 7) * (nblk >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int bh = wid / nkb, b = bh / H, h = bh % H;
  const int D = H * hd, ld = 3 * D;
  const int k0 = (wid % nkb) * (64 * KT) + wave * (16 * KT);
  const __bf16* base = qkv + (size_t)b * T * ld + h * hd;
  const __bf16* dob = d_o + (size_t)b * T * D + h * hd;
  const float c = scale * LOG2E;
  const int nchunk = T / 64;

  ChunkDma<HDP> dmaQ, dmaO;
  dmaQ.init(ld, hd, wave, lane);
  dmaO.init(D, hd, wave, lane);
  const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc((void*)dob, 0, 0x7fffffff, 0x00020000);
  auto issue = [&](int ch) {
    const int slot = ch % NSLOT;
    dmaQ.issue(rsQ, ch * 64 * ld * 2, ring.img(slot, 0), wave);
    dmaO.issue(rsO, ch * 64 * D * 2, ring.img(slot, 1), wave);
  };
  issue(0);
  if (nchunk > 1) issue(1);
  bf16x8 fk[KT][KS], fv[KT][KS];
#pragma unroll
  for (int ki = 0; ki < KT; ++ki)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      fk[ki][ks] = frag_rows_global(base + D, ld, k0 + 16 * ki, ks, hd, lane);
      fv[ki][ks] = frag_rows_global(base + 2 * D, ld, k0 + 16 * ki, ks, hd, lane);
    }
  for (int i = tid; i < T; i += NT) { s_lse[i] = -lse[(size_t)bh * T + i] * LOG2E; s_del[i] = delta[(size_t)bh * T + i]; }
  zero_pads<HDP, NT>(smem, NSLOT * 2, hd, tid);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  f32x4 dk[KT][NDT], dv[KT][NDT];
#pragma unroll
  for (int ki = 0; ki < KT; ++ki)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { dk[ki][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[ki][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  for (int qc = 0; qc < nchunk; ++qc) {
    if (qc + 1 < nchunk) wait_vmcnt<Ring<HDP>::PER_CHUNK>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (qc + 2 < nchunk) issue(qc + 2);
    const __bf16* iQ = ring.img(qc % NSLOT, 0);
    const __bf16* iO = ring.img(qc % NSLOT, 1);
    f32x4 pt[KT][4], st[KT][4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      bf16x8 fqr[KS], fdr[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) { fqr[ks] = frag_rows<HDP>(iQ, qt * 16, ks, lane); fdr[ks] = frag_rows<HDP>(iO, qt * 16, ks, lane); }
      const float4 l4 = *reinterpret_cast<const float4*>(s_lse + qc * 64 + qt * 16 + 4 * g);
      const float4 d4 = *reinterpret_cast<const float4*>(s_del + qc * 64 + qt * 16 + 4 * g);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq_[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int ki = 0; ki < KT; ++ki) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fqr[ks], fk[ki][ks], a, 0, 0, 0);    // S[q=4g+j][key=lane&15]
          p = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fdr[ks], fv[ki][ks], p, 0, 0, 0);    // dP
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pr = fast_exp2(__builtin_fmaf(a[j], c, lq[j]));
          a[j] = pr;
          p[j] = pr * (p[j] - dq_[j]) * scale;
        }
        pt[ki][qt] = a;
        st[ki][qt] = p;
      }
    }
    bf16x8 pp[KT][2], sp[KT][2];
#pragma unroll
    for (int ki = 0; ki < KT; ++ki) {
      pp[ki][0] = pack_perm(pt[ki][0], pt[ki][1]); pp[ki][1] = pack_perm(pt[ki][2], pt[ki][3]);
      sp[ki][0] = pack_perm(st[ki][0], st[ki][1]); sp[ki][1] = pack_perm(st[ki][2], st[ki][3]);
    }
    {
      bf16x8 cot[2], cqt[2], not_[2], nqt[2];       // dO^T / Q^T fragments of the current and the next d-tile
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) { cot[s2] = frag_cols_perm_asm<HDP>(iO, 32 * s2, 0, lane); cqt[s2] = frag_cols_perm_asm<HDP>(iQ, 32 * s2, 0, lane); }
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        lds_reads_done();
        if (dt + 1 < NDT) {
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            not_[s2] = frag_cols_perm_asm<HDP>(iO, 32 * s2, (dt + 1) * 16, lane);
            nqt[s2] = frag_cols_perm_asm<HDP>(iQ, 32 * s2, (dt + 1) * 16, lane);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int ki = 0; ki < KT; ++ki) {
            dv[ki][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cot[s2], pp[ki][s2], dv[ki][dt], 0, 0, 0);
            dk[ki][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cqt[s2], sp[ki][s2], dk[ki][dt], 0, 0, 0);
          }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) { cot[s2] = not_[s2]; cqt[s2] = nqt[s2]; }
      }
    }
  }
#pragma unroll
  for (int ki = 0; ki < KT; ++ki) {
    const int key = k0 + 16 * ki + (lane & 15);
    __bf16* row = dqkv + ((size_t)b * T + key) * ld + h * hd;
    bf16x4 ka[NDT], va[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { ka[dt] = to_bf16x4(dk[ki][dt]); va[dt] = to_bf16x4(dv[ki][dt]); }
    store_tiles<NDT>(row + D, ka, hd, g);
    store_tiles<NDT>(row + 2 * D, va, hd, g);
  }
}


// ------------------------------------------------------------------------------------- fused backward (dQ, dK, dV)
// One workgroup = 8 waves = one (batch, head); wave w owns the 16*KT keys [w*16*KT, (w+1)*16*KT) and keeps dK^T / dV^T of them
// in accumulators while the workgroup sweeps the queries in 64-row chunks (Q / dO chunks through the 3-slot LDS-DMA ring).
// S and dP are formed ONCE per (query chunk, key block) with the key on the MFMA lane: their accumulators, packed to bf16,
// are the B operands of dV^T += dO^T P and dK^T += Q^T dS straight from registers; dS crosses LDS once (a [keys][64 queries]
// bf16 image, 8-byte stores, conflict-free both ways) and dQ of the chunk = dS K is formed from that image and a resident
// K image by transposed reads -- 5 matrix products instead of the 7 of the two-kernel form, one prologue instead of two,
// no delta round trip through HBM (delta = rowsum(dO * O) is computed in the prologue into LDS).
// No float atomics: dQ of a chunk is summed over all keys inside one wave's accumulators (fixed order).
namespace {

// dS^T image [keys][64 queries], 128-B rows of 16 slots x 4 queries; slot ^= pi(key & 15), pi = bit permutation
// (b2 b1 | b3 b0): 16 consecutive keys x one slot -> 16 distinct slots (ds_write_b64, banks mod 32), and the 8 consecutive
// keys x 4 slots of one half-wave transposed read tile the 64 banks exactly (keys of equal parity share a bank half).
__device__ __forceinline__ int ds_pi(int key) { return (((key >> 1) & 3) << 2) | (key & 1) | (((key >> 3) & 1) << 1); }
__device__ __forceinline__ int ds_off(int key, int slot) { return key * 64 + ((slot ^ ds_pi(key)) << 2); }

}  // namespace

// ------------------------------------------------------------------------------------- forward, eight-wave form (round 4)
// The forward kernel above is latency-bound: per 64-key chunk a wave runs a dependent chain (S MFMAs -> row max -> exp -> sum -> pack -> PV
// MFMAs) and a CU holds eight such waves (two workgroups of four, 74 KB of LDS each).  Here a workgroup has EIGHT waves over the same K / V ring
// and the same 128 query rows -- 16 rows per wave (QT = 1) instead of 32 -- at no more than 128 registers, so a CU holds SIXTEEN waves, four per
// SIMD, with chains half as long.  Same products, same chunk order, same softmax arithmetic per row: bit-identical to k_attn_fwd.
template <int HDP, int KS, int NDT>
__global__ __launch_bounds__(512, 4) void k_attn_fwd8(const __bf16* __restrict__ qkv, __bf16* __restrict__ o,
                                                       float* __restrict__ lse, int T, int H, int hd, float scale) {
  constexpr int IMG = 64 * HDP, CPR = HDP / 8, PC = GroupDma<HDP, 2>::PER_WAVE;
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = gridDim.x, nqb = T / 128;
  const int wid = (nblk & 7) == 0 ? (blockIdx.x & 7) * (nblk >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int bh = wid / nqb, b = bh / H, h = bh % H;
  const int D = H * hd, ld = 3 * D;
  const int q0 = (wid % nqb) * 128 + wave * 16;
  const __bf16* base = qkv + (size_t)b * T * ld + h * hd;
  const float c = scale * LOG2E;
  const int nchunk = T / 64;

  GroupDma<HDP, 2> dma;                                  // one K / V chunk pair: image 0 = K, image 1 = V (same leading dimension)
  dma.init([&](int) { return ld; }, hd, wave, lane);
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)(base + D), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(base + 2 * D), 0, 0x7fffffff, 0x00020000);
  auto issue = [&](int ch) {
    __bf16* slot = smem + (ch % NSLOT) * 2 * IMG;
#pragma unroll
    for (int i = 0; i < PC; ++i) {
      const int j = wave + FNW * i, img = j / CPR, jj = j % CPR;
      if (dma.valid[i]) dma16(img ? rsV : rsK, slot + img * IMG + jj * 512, dma.off[i], ch * 64 * ld * 2);
    }
  };
  bf16x8 fq[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) fq[ks] = frag_rows_global(base, ld, q0, ks, hd, lane);
  issue(0);
  if (nchunk > 1) issue(1);
  zero_pads<HDP, 512, 2>(smem, NSLOT, hd, tid);          // pad chunk positions of the K images (never written by the DMA)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  f32x4 oacc[NDT];
  float m = -INFINITY, l = 0.f;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc = 0; kc < nchunk; ++kc) {
    if (kc + 1 < nchunk) wait_vmcnt<PC>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (kc + 2 < nchunk) issue(kc + 2);
    const __bf16* iK = smem + (kc % NSLOT) * 2 * IMG;
    const __bf16* iV = iK + IMG;
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows<HDP>(iK, kt * 16, ks, lane), fq[ks], a, 0, 0, 0);
      s[kt] = a;
    }
    // ONE set of V column fragments (the four-wave kernel keeps both halves in flight to cover the read latency itself; here three other
    // waves of the SIMD cover it and 128 registers do not hold two sets without spilling)
    bf16x8 fv[NDT];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) fv[dt] = frag_cols_perm_asm<HDP>(iV, 0, dt * 16, lane);
    __builtin_amdgcn_sched_barrier(0);
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[kt][j]);
    mx = group_max(mx);
    const float mn = fmaxf(m, mx);
    const float alpha = fast_exp2((m - mn) * c);
    m = mn;
    const float mc = mn * c;
    float ps = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float pr = fast_exp2(__builtin_fmaf(s[kt][j], c, -mc));
        s[kt][j] = pr;
        ps += pr;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) oacc[dt] *= alpha;
    const bf16x8 pf0 = pack_perm(s[0], s[1]), pf1 = pack_perm(s[2], s[3]);
    lds_reads_done();
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv[dt], pf0, oacc[dt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);          // (an MFMA reads its operands when it issues: the asynchronous reads below may reuse the registers)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) fv[dt] = frag_cols_perm_asm<HDP>(iV, 32, dt * 16, lane);
    lds_reads_done();
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv[dt], pf1, oacc[dt], 0, 0, 0);
  }
  const float lt = group_sum(l);
  const float inv = 1.0f / lt;
  const int q = q0 + (lane & 15);
  __bf16* orow = o + ((size_t)b * T + q) * D + h * hd;
  bf16x4 ov[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) ov[dt] = to_bf16x4(oacc[dt] * inv);
  store_tiles<NDT>(orow, ov, hd, g);
  if (g == 0) lse[(size_t)bh * T + q] = m * scale + logf(lt);
}

template <int HDP, int KS, int NDT, int KT>
__global__ __launch_bounds__(512) void k_attn_bwd_fused(const __bf16* __restrict__ qkv, const __bf16* __restrict__ o,
                                                        const __bf16* __restrict__ d_o, const float* __restrict__ lse,
                                                        __bf16* __restrict__ dqkv, int H, int hd, float scale,
                                                        float* __restrict__ bias_part) {
  constexpr int T = FNW * 16 * KT, NCH = T / 64, IMG = 64 * HDP;
  constexpr int ND0 = (NDT + 1) / 2, ND1 = NDT - ND0;       // d-tiles of the two wave groups in the dQ phase
  extern __shared__ __attribute__((aligned(16))) __bf16 smem[];
  __bf16* const ringb = smem;                                // [NSLOT][2][64][HDP]: Q / dO chunks
  __bf16* const imgK = smem + NSLOT * 2 * IMG;               // [T][HDP]
  __bf16* const imgS = imgK + NCH * IMG;                     // [T keys][64 queries]
  float* const s_lse = reinterpret_cast<float*>(imgS + T * 64);
  float* const s_del = s_lse + T;
  float* const s_dq = s_del + T;                             // [FNW][ND0 * 16]: token sums of this wave's dQ columns (qkv.bias partials)
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  ATTN_STAMP_INIT(); ATTN_STAMP(0);
  // neighbouring heads of one sample read neighbouring 144-B column slices of the same rows: keep them on one XCD's L2
  const int nblk = gridDim.x;
  const int bh = (nblk & 7) == 0 ? (blockIdx.x & 7) * (nblk >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const int b = bh / H, h = bh % H;
  const int D = H * hd, ld = 3 * D;
  const int k0 = wave * (16 * KT);
  const __bf16* base = qkv + (size_t)b * T * ld + h * hd;
  const __bf16* dob = d_o + (size_t)b * T * D + h * hd;
  const __bf16* ob = o + (size_t)b * T * D + h * hd;
  const float c = scale * LOG2E;

  GroupDma<HDP, 2> dmaC;        // one Q / dO chunk
  GroupDma<HDP, NCH> dmaK;      // the whole K image
  dmaC.init([&](int img) { return img ? D : ld; }, hd, wave, lane);
  dmaK.init([&](int) { return ld; }, hd, wave, lane);
  const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc((void*)dob, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)(base + D), 0, 0x7fffffff, 0x00020000);
  constexpr int CPR = HDP / 8, PC = GroupDma<HDP, 2>::PER_WAVE;
  auto issue_chunk = [&](int ch) {
    __bf16* slot = ringb + (ch % NSLOT) * 2 * IMG;
#pragma unroll
    for (int i = 0; i < PC; ++i) {
      const int j = wave + FNW * i, img = j / CPR, jj = j % CPR;
      if (dmaC.valid[i])
        dma16(img ? rsO : rsQ, slot + img * IMG + jj * 512, dmaC.off[i], ch * 64 * (img ? D : ld) * 2);
    }
  };
  // delta[q] = sum_d dO[q][d] O[q][d]: two threads per query row, each with a 16-byte-aligned run of the head's columns; ALL their
  // loads go out here, ahead of the LDS-DMA traffic (vector-memory operations retire in order: issued behind the 37 KB K image they
  // would wait for it, and a load-use loop would pay one memory latency per iteration)
  constexpr int NDC = HDP / 16;
  static_assert(T <= FNT / 2 || T == FNT / 2, "one query row per thread pair");
  bf16x8 d_dd[NDC], d_oo[NDC];
  const int d_q = tid >> 1, d_split = ((hd + 15) >> 4) << 3;
  const int d_beg = (tid & 1) ? d_split : 0, d_len = (tid & 1) ? hd - d_split : d_split;
#pragma unroll
  for (int j = 0; j < NDC; ++j) {
    const bool in = d_q < T && j * 8 < d_len;
    const size_t e = (size_t)(in ? d_q : 0) * D + (in ? d_beg + j * 8 : 0);
    d_dd[j] = *reinterpret_cast<const bf16x8*>(dob + e);
    d_oo[j] = *reinterpret_cast<const bf16x8*>(ob + e);
  }
#pragma unroll
  for (int i = 0; i < GroupDma<HDP, NCH>::PER_WAVE; ++i) {
    const int j = wave + FNW * i, img = j / CPR, jj = j % CPR;
    if (dmaK.valid[i])
      dma16(rsK, imgK + img * IMG + jj * 512, dmaK.off[i], img * 64 * ld * 2);
  }
  ATTN_STAMP_P(1);
  issue_chunk(0);
  if (NCH > 1) issue_chunk(1);

  // this wave's keys: the V row fragments stay in registers for the whole kernel; the K row fragments are re-read from the
  // resident K image (holding both costs 48 registers and spills at head_dim 72)
  bf16x8 fv[KT][KS];
#pragma unroll
  for (int ki = 0; ki < KT; ++ki)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fv[ki][ks] = frag_rows_global(base + 2 * D, ld, k0 + 16 * ki, ks, hd, lane);
  // -lse * log2(e), and delta from the operands fetched at the top
  for (int i = tid; i < T; i += FNT) s_lse[i] = -lse[(size_t)bh * T + i] * LOG2E;
  if (bias_part) for (int i = tid; i < FNW * ND0 * 16; i += FNT) s_dq[i] = 0.f;
  {
    float dsum = 0.f;
#pragma unroll
    for (int j = 0; j < NDC; ++j)
      if (d_q < T && j * 8 < d_len) {
#pragma unroll
        for (int e = 0; e < 8; ++e) dsum += bf2f(d_dd[j][e]) * bf2f(d_oo[j][e]);
      }
    dsum += __shfl_xor(dsum, 1, 64);
    if (!(tid & 1) && d_q < T) s_del[d_q] = dsum;
  }
  ATTN_STAMP_P(2);
  // pad columns of the ring and of the K image (never written by the DMA)
  zero_pads<HDP, FNT>(smem, NSLOT * 2 + NCH, hd, tid);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  ATTN_STAMP_P(3);

  f32x4 dk[KT][NDT], dv[KT][NDT];
#pragma unroll
  for (int ki = 0; ki < KT; ++ki)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { dk[ki][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[ki][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  const unsigned sbase = lds_addr(imgS);
  // dS^T stores: tile (ki, qt) -> row key = k0 + 16 ki + (lane & 15), logical slot 4 qt + g
  unsigned wr_addr[KT];
#pragma unroll
  for (int ki = 0; ki < KT; ++ki) wr_addr[ki] = sbase + 2 * ((k0 + 16 * ki + (lane & 15)) * 64);
  const int wr_pi = ds_pi(lane & 15);        // k0 + 16 ki is a multiple of 16
  // dQ phase: wave -> query tile qi of the chunk and a group of d-tiles
  const int qi = wave & 3, dgrp = wave >> 2;
  const int dt0 = dgrp ? ND0 : 0, nd = dgrp ? ND1 : ND0;
  ColPerm<HDP> cp;
  cp.init(lane);
  // transposed-read addresses of the K column fragments of this wave's d-tiles (key step 0) and of the dS^T fragment
  // (permuted k-slot map: rows 4g + q4 and 16 + 4g + q4 of a 32-key step)
  unsigned rdK[ND0], rdS[2];
  {
    const int i = lane & 15, q4 = i >> 2, p = i & 3;
#pragma unroll
    for (int k = 0; k < ND0; ++k)
      // a wave of the second group with fewer d-tiles (head_dim 72: tiles 3, 4) multiplies a surplus tile made of the zero pad
      // columns (or repeats its last tile) and never stores it
      rdK[k] = lds_addr(imgK) + 2 * (aoff<HDP>(4 * g + q4, 2 * ((dt0 + k) * 16 < HDP ? dt0 + k : dt0) + (p >> 1)) + 4 * (p & 1));
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int r = 16 * hh + 4 * g + q4;                  // key inside the 32-key step (step base is a multiple of 32)
      rdS[hh] = sbase + 2 * (r * 64 + (((4 * qi + p) ^ ds_pi(r)) << 2));
    }
  }

  bf16x8 fkr[KT][KS];
  for (int qc = 0; qc < NCH; ++qc) {
    // chunk qc has landed (younger: the next chunk's DMA and the dQ stores of the chunks since -- with the 16-byte pairs a wave issues as few
    // as ONE store per chunk, so only one is counted on; a smaller count only waits for more)
    if (qc == 0) wait_vmcnt<PC>();
    else if (qc + 1 < NCH) wait_vmcnt<PC + 1>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (qc == 0) { ATTN_STAMP_P(4); ATTN_STAMP_L(1); }
    if (qc + 2 < NCH) issue_chunk(qc + 2);
    const __bf16* iQ = ringb + (qc % NSLOT) * 2 * IMG;
    const __bf16* iO = iQ + IMG;
    if (qc == 0) {
      // this wave's K row fragments, once (the K image has landed with chunk 0): re-read per (query tile, key tile) they were 24 load-use
      // pairs per chunk in front of the S MFMAs (round 4: MFMA results in architectural VGPRs left the registers for them)
#pragma unroll
      for (int ki = 0; ki < KT; ++ki)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) fkr[ki][ks] = frag_rows<HDP>(imgK, k0 + 16 * ki, ks, lane);
    }
    bf16x8 pp[KT][2], sp[KT][2];          // P and dS of this chunk, bf16, in the k-slot order of the transposed fragments
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      bf16x8 fqr[KS], fdr[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) { fqr[ks] = frag_rows<HDP>(iQ, qt * 16, ks, lane); fdr[ks] = frag_rows<HDP>(iO, qt * 16, ks, lane); }
      const float4 l4 = *reinterpret_cast<const float4*>(s_lse + qc * 64 + qt * 16 + 4 * g);
      const float4 d4 = *reinterpret_cast<const float4*>(s_del + qc * 64 + qt * 16 + 4 * g);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq_[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int ki = 0; ki < KT; ++ki) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fqr[ks], fkr[ki][ks], a, 0, 0, 0);   // S[q = 4g+j][key = lane&15]
          p = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fdr[ks], fv[ki][ks], p, 0, 0, 0);    // dP
        }
        bf16x4 sv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pr = fast_exp2(__builtin_fmaf(a[j], c, lq[j]));
          const float dsv = pr * (p[j] - dq_[j]) * scale;                                  // dS (incl. softmax scale)
          pp[ki][qt >> 1][4 * (qt & 1) + j] = f2bf(pr);                                    // = pack_perm(tile 2h, tile 2h+1)
          sv[j] = f2bf(dsv);
          sp[ki][qt >> 1][4 * (qt & 1) + j] = sv[j];
        }
        // dS^T[key][16 qt + 4g .. +3] -> LDS (asm: invisible to hipcc's LDS-DMA alias bookkeeping)
        asm_write_b64(wr_addr[ki] + 8 * ((4 * qt + g) ^ wr_pi), sv);
      }
    }
    if (qc == 0) ATTN_STAMP_L(2);
    {
      // dV^T += dO^T P, dK^T += Q^T dS: dO^T / Q^T column fragments of d-tile dt + 1 are read under the MFMAs of d-tile dt
      unsigned aQ[ColPerm<HDP>::NB], aO[ColPerm<HDP>::NB];
#pragma unroll
      for (int k = 0; k < ColPerm<HDP>::NB; ++k) { aQ[k] = lds_addr(iQ) + cp.b[k]; aO[k] = lds_addr(iO) + cp.b[k]; }
      bf16x8 cot[2], cqt[2], not_[2], nqt[2];
      __builtin_amdgcn_sched_barrier(0);
      cot[0] = col_frag<HDP, 0, 0>(aO); cot[1] = col_frag<HDP, 0, 1>(aO);
      cqt[0] = col_frag<HDP, 0, 0>(aQ); cqt[1] = col_frag<HDP, 0, 1>(aQ);
      static_for<NDT>([&](auto dtc) {
        constexpr int dt = decltype(dtc)::value;
        lds_reads_done();
        if constexpr (dt + 1 < NDT) {
          not_[0] = col_frag<HDP, dt + 1, 0>(aO); not_[1] = col_frag<HDP, dt + 1, 1>(aO);
          nqt[0] = col_frag<HDP, dt + 1, 0>(aQ); nqt[1] = col_frag<HDP, dt + 1, 1>(aQ);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int ki = 0; ki < KT; ++ki) {
            dv[ki][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cot[s2], pp[ki][s2], dv[ki][dt], 0, 0, 0);
            dk[ki][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cqt[s2], sp[ki][s2], dk[ki][dt], 0, 0, 0);
          }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) { cot[s2] = not_[s2]; cqt[s2] = nqt[s2]; }
      });
    }
    // every wave's dS^T tiles of this chunk are in LDS
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (qc == 0) ATTN_STAMP_L(3);
    {
      // dQ[64 qc + 16 qi + ..][16 (dt0 + i) + ..] = sum over all T keys of dS[q][key] K[key][d]
      f32x4 dq[ND0];
#pragma unroll
      for (int i = 0; i < ND0; ++i) dq[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      // two fragment sets, selected by the parity of the (compile-time) key step: the reads of step kk + 1 go out under
      // the MFMAs of step kk, and no register is COPIED while an asynchronous read into it is still in flight
      bf16x8 fa[2][ND0];
      bf16x8 fb[2];
      auto read_step = [&](auto kkc, bf16x8 (&A)[ND0], bf16x8& Bf) {
        constexpr int kk = decltype(kkc)::value;
        const bf16x4 lo = asm_read_tr_off<kk * (32 * 64 * 2)>(rdS[0]), hi = asm_read_tr_off<kk * (32 * 64 * 2)>(rdS[1]);
        Bf = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int i = 0; i < ND0; ++i) {      // every wave reads / multiplies ND0 d-tiles: no branch around an asynchronous read
          const bf16x4 l2 = asm_read_tr_off<kk * (32 * HDP * 2)>(rdK[i]), h2 = asm_read_tr_off<kk * (32 * HDP * 2) + 16 * HDP * 2>(rdK[i]);
          A[i] = bf16x8{l2[0], l2[1], l2[2], l2[3], h2[0], h2[1], h2[2], h2[3]};
        }
      };
      read_step(std::integral_constant<int, 0>{}, fa[0], fb[0]);
      static_for<T / 32>([&](auto kkc) {
        constexpr int kk = decltype(kkc)::value, cur = kk & 1;
        lds_reads_done();
        if constexpr (kk + 1 < T / 32) read_step(std::integral_constant<int, kk + 1>{}, fa[cur ^ 1], fb[cur ^ 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < ND0; ++i) dq[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[cur][i], fb[cur], dq[i], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      });
      const int q = qc * 64 + 16 * qi + (lane & 15);
      __bf16* row = dqkv + ((size_t)b * T + q) * ld + h * hd;
      {
        bf16x4 ov[ND0];
#pragma unroll
        for (int i = 0; i < ND0; ++i) ov[i] = to_bf16x4(dq[i]);
#pragma unroll
        for (int i = 0; i + 1 < ND0; i += 2) {               // pairs of this wave's d-tiles as 16-byte pieces (all lanes swap, stores are masked)
          const uint4 pk = pair_pack(ov[i], ov[i + 1]);
          const int c = (dt0 + i) * 16 + pair_col(g), d = (dt0 + i) * 16 + 4 * g;
          if (i + 1 < nd) { if (c < hd) *reinterpret_cast<uint4*>(row + c) = pk; }
          else if (i < nd && d < hd) *reinterpret_cast<bf16x4*>(row + d) = ov[i];
        }
        if constexpr (ND0 & 1) {
          const int d = (dt0 + ND0 - 1) * 16 + 4 * g;
          if (ND0 - 1 < nd && d < hd) *reinterpret_cast<bf16x4*>(row + d) = ov[ND0 - 1];
        }
      }
      if (bias_part) {
        // qkv.bias gradient, Q part: sum of this chunk's 16 query rows (butterfly over lane & 15, all lanes active), added by
        // lane 16 g of the wave to its own LDS row -- no other lane or wave touches those words: no atomics, fixed order
#pragma unroll
        for (int i = 0; i < ND0; ++i) {
          f32x4 v = dq[i];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float x = v[j];
            x = row16_sum(x);
            v[j] = x;
          }
          if ((lane & 15) == 0) {
            f32x4* acc = reinterpret_cast<f32x4*>(s_dq + wave * (ND0 * 16) + i * 16 + 4 * g);
            *acc = *acc + v;
          }
        }
      }
    }
    if (qc == 0) ATTN_STAMP_L(4);
  }
  ATTN_STAMP(5);
#pragma unroll
  for (int ki = 0; ki < KT; ++ki) {
    const int key = k0 + 16 * ki + (lane & 15);
    __bf16* row = dqkv + ((size_t)b * T + key) * ld + h * hd;
    bf16x4 ka[NDT], va[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) { ka[dt] = to_bf16x4(dk[ki][dt]); va[dt] = to_bf16x4(dv[ki][dt]); }
    store_tiles<NDT>(row + D, ka, hd, g);
    store_tiles<NDT>(row + 2 * D, va, hd, g);
  }
  if (bias_part) {
    // K / V parts: this wave's 16 KT keys summed per column, then the eight waves meet in LDS.  The Q / dO ring is free: its last
    // reads were before the loop's mid-iteration barrier, which every wave has passed.
    float* const s_kv = reinterpret_cast<float*>(ringb);           // [FNW][2][NDT * 16]
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      f32x4 sk = dk[0][dt], sv = dv[0][dt];
#pragma unroll
      for (int ki = 1; ki < KT; ++ki) { sk += dk[ki][dt]; sv += dv[ki][dt]; }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float x = sk[j], y = sv[j];
        x = row16_sum(x);
        y = row16_sum(y);
        sk[j] = x; sv[j] = y;
      }
      if ((lane & 15) == 0) {
        *reinterpret_cast<f32x4*>(s_kv + (wave * 2 + 0) * (NDT * 16) + dt * 16 + 4 * g) = sk;
        *reinterpret_cast<f32x4*>(s_kv + (wave * 2 + 1) * (NDT * 16) + dt * 16 + 4 * g) = sv;
      }
    }
    __syncthreads();
    float* const out = bias_part + (size_t)b * ld + h * hd;          // row b of [B][3 D]
    for (int e = tid; e < 3 * hd; e += FNT) {
      const int which = e / hd, d = e % hd;
      float x;
      if (which == 0) {                                              // waves 4 dgrp + qi hold d-tiles dt0(dgrp) .. of query tile qi
        const int dt = d >> 4, grp = dt >= ND0 ? 1 : 0, i = dt - (grp ? ND0 : 0);
        const float* p = s_dq + (grp * 4) * (ND0 * 16) + i * 16 + (d & 15);
        x = ((p[0] + p[ND0 * 16]) + p[2 * ND0 * 16]) + p[3 * ND0 * 16];
      } else {
        const float* p = s_kv + (which - 1) * (NDT * 16) + d;
        x = p[0];
#pragma unroll
        for (int w2 = 1; w2 < FNW; ++w2) x += p[w2 * 2 * (NDT * 16)];
      }
      out[which * D + d] = x;
    }
  }
  ATTN_STAMP(6);
}

template __global__ void k_attn_bwd_fused<64, 2, 4, 2>(const __bf16*, const __bf16*, const __bf16*, const float*, __bf16*, int, int, float, float*);
template __global__ void k_attn_bwd_fused<64, 2, 3, 2>(const __bf16*, const __bf16*, const __bf16*, const float*, __bf16*, int, int, float, float*);
template __global__ void k_attn_bwd_fused<64, 2, 3, 1>(const __bf16*, const __bf16*, const __bf16*, const float*, __bf16*, int, int, float, float*);
template __global__ void k_attn_bwd_fused<96, 3, 5, 2>(const __bf16*, const __bf16*, const __bf16*, const float*, __bf16*, int, int, float, float*);
template __global__ void k_attn_bwd_fused<64, 2, 4, 1>(const __bf16*, const __bf16*, const __bf16*, const float*, __bf16*, int, int, float, float*);
template __global__ void k_attn_bwd_fused<96, 3, 5, 1>(const __bf16*, const __bf16*, const __bf16*, const float*, __bf16*, int, int, float, float*);

#define SFRON_INST_ATTN(HDP, KS, NDT)                                                                              \
  template __global__ void k_attn_fwd<HDP, KS, NDT, 1>(const __bf16*, __bf16*, float*, int, int, int, float);      \
  template __global__ void k_attn_fwd<HDP, KS, NDT, 2>(const __bf16*, __bf16*, float*, int, int, int, float);      \
  template __global__ void k_attn_fwd<HDP, KS, NDT, 2, 8>(const __bf16*, __bf16*, float*, int, int, int, float);   \
  template __global__ void k_attn_fwd<HDP, KS, NDT, 2, 4, 2>(const __bf16*, __bf16*, float*, int, int, int, float); \
  template __global__ void k_attn_bwd_dq<HDP, KS, NDT, 1>(const __bf16*, const __bf16*, const __bf16*, const float*, float*, __bf16*, int, int, int, float); \
  template __global__ void k_attn_bwd_dq<HDP, KS, NDT, 2>(const __bf16*, const __bf16*, const __bf16*, const float*, float*, __bf16*, int, int, int, float); \
  template __global__ void k_attn_bwd_dkv<HDP, KS, NDT, 1>(const __bf16*, const __bf16*, const float*, const float*, __bf16*, int, int, int, float);
SFRON_INST_ATTN(64, 2, 4)
SFRON_INST_ATTN(64, 2, 3)      // head_dim <= 48 (the LDM UNet's 40): three output d-tiles instead of four
SFRON_INST_ATTN(96, 3, 5)
#undef SFRON_INST_ATTN
template __global__ void k_attn_fwd8<64, 2, 4>(const __bf16*, __bf16*, float*, int, int, int, float);
template __global__ void k_attn_fwd8<64, 2, 3>(const __bf16*, __bf16*, float*, int, int, int, float);
template __global__ void k_attn_fwd8<96, 3, 5>(const __bf16*, __bf16*, float*, int, int, int, float);


// =================================================================================================
// Short sequences (T < 64, any T): the patch-8 entries of the reference's model registry at 256 px give 16 tokens
// (DiT/models.py:328-370).  One workgroup per (batch, head), everything in LDS as fp32, plain FMA loops -- the work is a few
// thousand multiply-adds per head; no MFMA tile would be filled.  Same math as the tiled kernels (softmax(q k^T hd^-0.5) v and
// its autograd), P and dS kept in fp32.  Fixed summation order, no atomics.
// =================================================================================================
namespace {
constexpr int SNT = 256;
__device__ __forceinline__ void small_load(const __bf16* base, int ld, int T, int hd, int HDS, float* dst, int tid) {
  for (int e = tid; e < T * hd; e += SNT) { const int i = e / hd, d = e % hd; dst[i * HDS + d] = bf2f(base[(size_t)i * ld + d]); }
}
}  // namespace

__global__ __launch_bounds__(256) void k_attn_small_fwd(const __bf16* __restrict__ qkv, __bf16* __restrict__ o, float* __restrict__ lse,
                                                         int T, int H, int hd, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int HDS = hd + 1;                                    // odd row stride: rows of K / V walk the banks
  float* q = sm; float* k = q + T * HDS; float* v = k + T * HDS; float* S = v + T * HDS;      // S [T][T + 1]
  const int TS = T + 1;
  const int tid = threadIdx.x, bh = blockIdx.x, b = bh / H, h = bh % H, D = H * hd, ld = 3 * D;
  const __bf16* base = qkv + (size_t)b * T * ld + h * hd;
  small_load(base, ld, T, hd, HDS, q, tid); small_load(base + D, ld, T, hd, HDS, k, tid); small_load(base + 2 * D, ld, T, hd, HDS, v, tid);
  __syncthreads();
  for (int e = tid; e < T * T; e += SNT) {
    const int i = e / T, j = e % T;
    float a = 0.f;
    for (int d = 0; d < hd; ++d) a += q[i * HDS + d] * k[j * HDS + d];
    S[i * TS + j] = a * scale;
  }
  __syncthreads();
  for (int i = tid; i < T; i += SNT) {
    float m = -INFINITY;
    for (int j = 0; j < T; ++j) m = fmaxf(m, S[i * TS + j]);
    float sum = 0.f;
    for (int j = 0; j < T; ++j) { const float e = __expf(S[i * TS + j] - m); S[i * TS + j] = e; sum += e; }
    const float inv = 1.0f / sum;
    for (int j = 0; j < T; ++j) S[i * TS + j] *= inv;
    lse[(size_t)bh * T + i] = m + __logf(sum);
  }
  __syncthreads();
  for (int e = tid; e < T * hd; e += SNT) {
    const int i = e / hd, d = e % hd;
    float a = 0.f;
    for (int j = 0; j < T; ++j) a += S[i * TS + j] * v[j * HDS + d];
    o[((size_t)b * T + i) * D + h * hd + d] = f2bf(a);
  }
}

__global__ __launch_bounds__(256) void k_attn_small_bwd(const __bf16* __restrict__ qkv, const __bf16* __restrict__ o,
                                                         const __bf16* __restrict__ d_o, const float* __restrict__ lse,
                                                         __bf16* __restrict__ dqkv, int T, int H, int hd, float scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int HDS = hd + 1, TS = T + 1;
  float* q = sm; float* k = q + T * HDS; float* v = k + T * HDS; float* dO = v + T * HDS;
  float* P = dO + T * HDS; float* dS = P + T * TS; float* delta = dS + T * TS;
  const int tid = threadIdx.x, bh = blockIdx.x, b = bh / H, h = bh % H, D = H * hd, ld = 3 * D;
  const __bf16* base = qkv + (size_t)b * T * ld + h * hd;
  const __bf16* dob = d_o + (size_t)b * T * D + h * hd;
  const __bf16* ob = o + (size_t)b * T * D + h * hd;
  small_load(base, ld, T, hd, HDS, q, tid); small_load(base + D, ld, T, hd, HDS, k, tid); small_load(base + 2 * D, ld, T, hd, HDS, v, tid);
  small_load(dob, D, T, hd, HDS, dO, tid);
  for (int i = tid; i < T; i += SNT) {
    float a = 0.f;
    for (int d = 0; d < hd; ++d) a += bf2f(dob[(size_t)i * D + d]) * bf2f(ob[(size_t)i * D + d]);
    delta[i] = a;
  }
  __syncthreads();
  for (int e = tid; e < T * T; e += SNT) {
    const int i = e / T, j = e % T;
    float a = 0.f, dp = 0.f;
    for (int d = 0; d < hd; ++d) { a += q[i * HDS + d] * k[j * HDS + d]; dp += dO[i * HDS + d] * v[j * HDS + d]; }
    const float p = __expf(a * scale - lse[(size_t)bh * T + i]);
    P[i * TS + j] = p;
    dS[i * TS + j] = p * (dp - delta[i]) * scale;
  }
  __syncthreads();
  __bf16* outb = dqkv + (size_t)b * T * ld + h * hd;
  for (int e = tid; e < T * hd; e += SNT) {
    const int i = e / hd, d = e % hd;
    float dq = 0.f, dk = 0.f, dv = 0.f;
    for (int j = 0; j < T; ++j) {
      dq += dS[i * TS + j] * k[j * HDS + d];
      dk += dS[j * TS + i] * q[j * HDS + d];
      dv += P[j * TS + i] * dO[j * HDS + d];
    }
    outb[(size_t)i * ld + d] = f2bf(dq);
    outb[(size_t)i * ld + D + d] = f2bf(dk);
    outb[(size_t)i * ld + 2 * D + d] = f2bf(dv);
  }
}

static int launch_small_fwd(const __bf16* qkv, __bf16* o, float* lse, int B, int T, int H, int hd, float scale, hipStream_t s) {
  const size_t lds = (size_t)(3 * T * (hd + 1) + T * (T + 1)) * sizeof(float);
  if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_small_fwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return (int)hipGetLastError();
  hipLaunchKernelGGL(k_attn_small_fwd, dim3(B * H), dim3(256), lds, s, qkv, o, lse, T, H, hd, scale);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}
static int launch_small_bwd(const __bf16* qkv, const __bf16* o, const __bf16* d_o, const float* lse, __bf16* dqkv, int B, int T, int H, int hd,
                            float scale, hipStream_t s) {
  const size_t lds = (size_t)(4 * T * (hd + 1) + 2 * T * (T + 1) + T) * sizeof(float);
  if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_small_bwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return (int)hipGetLastError();
  hipLaunchKernelGGL(k_attn_small_bwd, dim3(B * H), dim3(256), lds, s, qkv, o, d_o, lse, dqkv, T, H, hd, scale);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}

namespace {

// 0 / 1 = fused backward where the sequence length allows it; 2 = always the two-kernel form (tests compare the two)
int g_bwd_form = 0;

// process-wide: 0 = by rule (k_attn_fwd8 for sequences of 512 tokens or more -- the LDM UNet's 1024 / 4096: 467 -> 391 us at T = 4096; at the
// DiT's 256 tokens the eight-wave form is 9 % faster alone, 31.5 -> 28.6 us, and 0.4 ms per step SLOWER inside the step), 4 / 8 = force (A-B)
int g_fwd_form = 0;
template <int HDP> size_t lds_bytes(int extra_floats) { return NSLOT * 2 * 64 * HDP * sizeof(__bf16) + extra_floats * sizeof(float); }

template <typename K> int set_lds(K kern, size_t lds) {
  if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return (int)hipGetLastError();
  return SFRON_OK;
}

template <int HDP, int KS, int NDT>
int launch_fwd(const __bf16* qkv, __bf16* o, float* lse, int B, int T, int H, int hd, float scale, hipStream_t s) {
  const size_t lds = lds_bytes<HDP>(0);
  if (T % 128 == 0 && (g_fwd_form == 8 || (g_fwd_form == 0 && T >= 512))) {                 // eight waves of 16 query rows over the same ring: sixteen waves per CU
    int rc = set_lds(&k_attn_fwd8<HDP, KS, NDT>, lds); if (rc) return rc;
    hipLaunchKernelGGL((k_attn_fwd8<HDP, KS, NDT>), dim3(T / 128 * B * H), dim3(512), lds, s, qkv, o, lse, T, H, hd, scale);
  } else if (T % 256 == 0 && g_fwd_form == 16) {      // eight waves of 32 query rows (a whole head per workgroup at T = 256): measured, not the rule --
                                                       // 29.9 us against 27.3 alone, +0.2 ms in the step: one workgroup per CU, eight waves per barrier
    int rc = set_lds(&k_attn_fwd<HDP, KS, NDT, 2, 8>, lds); if (rc) return rc;
    hipLaunchKernelGGL((k_attn_fwd<HDP, KS, NDT, 2, 8>), dim3(T / 256 * B * H), dim3(512), lds, s, qkv, o, lse, T, H, hd, scale);
  } else if (T % 256 == 0 && g_fwd_form == 2) {        // round 6: both 128-row query blocks of a head in one workgroup (one resident round of 512 at
                                                       // DiT-XL/2): measured, not the rule -- 30.5 us against 27.5 alone, 62.26 / 62.74 against 62.63 / 62.79 ms
                                                       // per step (profiles/r06_ab_log.txt): with 1 024 workgroups the second round's prologues
                                                       // already run under the first round's last chunks
    int rc = set_lds(&k_attn_fwd<HDP, KS, NDT, 2, 4, 2>, lds); if (rc) return rc;
    hipLaunchKernelGGL((k_attn_fwd<HDP, KS, NDT, 2, 4, 2>), dim3(T / 256 * B * H), dim3(NT), lds, s, qkv, o, lse, T, H, hd, scale);
  } else if (T % 128 == 0) {
    int rc = set_lds(&k_attn_fwd<HDP, KS, NDT, 2>, lds); if (rc) return rc;
    hipLaunchKernelGGL((k_attn_fwd<HDP, KS, NDT, 2>), dim3(T / 128 * B * H), dim3(NT), lds, s, qkv, o, lse, T, H, hd, scale);
  } else {
    int rc = set_lds(&k_attn_fwd<HDP, KS, NDT, 1>, lds); if (rc) return rc;
    hipLaunchKernelGGL((k_attn_fwd<HDP, KS, NDT, 1>), dim3(T / 64 * B * H), dim3(NT), lds, s, qkv, o, lse, T, H, hd, scale);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}
template <int HDP, int KS, int NDT, int KT>
int launch_bwd_fused(const __bf16* qkv, const __bf16* o, const __bf16* d_o, const float* lse, __bf16* dqkv, int B, int H, int hd,
                     float scale, float* bias_part, hipStream_t s) {
  constexpr int T = FNW * 16 * KT;
  const size_t lds = (size_t)(NSLOT * 2 * 64 * HDP + T * HDP + T * 64) * sizeof(__bf16) + 2 * T * sizeof(float) +
                     FNW * ((NDT + 1) / 2) * 16 * sizeof(float);
  int rc = set_lds(&k_attn_bwd_fused<HDP, KS, NDT, KT>, lds); if (rc) return rc;
  SFRON_LAUNCH_EV((k_attn_bwd_fused<HDP, KS, NDT, KT>), dim3(B * H), dim3(FNT), lds, s, qkv, o, d_o, lse, dqkv, H, hd, scale, bias_part);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}

template <int HDP, int KS, int NDT>
int launch_bwd(const __bf16* qkv, const __bf16* o, const __bf16* d_o, const float* lse, float* delta, __bf16* dqkv, int B,
               int T, int H, int hd, float scale, hipStream_t s, float* bias_part = nullptr) {
  // one workgroup per (batch, head) with the whole sequence behind it: T = 256 (DiT-XL/2 ... DiT-S/2 at 256 px) and T = 128
  if (T == 256 && g_bwd_form != 2) return launch_bwd_fused<HDP, KS, NDT, 2>(qkv, o, d_o, lse, dqkv, B, H, hd, scale, bias_part, s);
  if (T == 128 && g_bwd_form != 2) return launch_bwd_fused<HDP, KS, NDT, 1>(qkv, o, d_o, lse, dqkv, B, H, hd, scale, bias_part, s);
  if (bias_part) return SFRON_ERR_UNSUPPORTED;
  const size_t lds = lds_bytes<HDP>(0), lds2 = lds_bytes<HDP>(2 * T);
  if (T % 128 == 0) {
    int rc = set_lds(&k_attn_bwd_dq<HDP, KS, NDT, 2>, lds); if (rc) return rc;
    hipLaunchKernelGGL((k_attn_bwd_dq<HDP, KS, NDT, 2>), dim3(T / 128 * B * H), dim3(NT), lds, s, qkv, o, d_o, lse, delta, dqkv, T, H, hd, scale);
  } else {
    int rc = set_lds(&k_attn_bwd_dq<HDP, KS, NDT, 1>, lds); if (rc) return rc;
    hipLaunchKernelGGL((k_attn_bwd_dq<HDP, KS, NDT, 1>), dim3(T / 64 * B * H), dim3(NT), lds, s, qkv, o, d_o, lse, delta, dqkv, T, H, hd, scale);
  }
  int rc = set_lds(&k_attn_bwd_dkv<HDP, KS, NDT, 1>, lds2); if (rc) return rc;
  hipLaunchKernelGGL((k_attn_bwd_dkv<HDP, KS, NDT, 1>), dim3(T / 64 * B * H), dim3(NT), lds2, s, qkv, d_o, lse, delta, dqkv, T, H, hd, scale);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SFRON_OK : (int)e;
}

}  // namespace

extern "C" {

int sfron_attn_fwd(const uint16_t* qkv, uint16_t* o, float* lse, int B, int T, int H, int hd, void* stream) {
  SFRON_CHECK_ARG(qkv && o && lse && B > 0 && H > 0 && T > 0 && hd > 0);
  const float scale = 1.0f / sqrtf((float)hd);
  hipStream_t s = (hipStream_t)stream;
  if (T < 64) return hd <= 128 ? launch_small_fwd((const __bf16*)qkv, (__bf16*)o, lse, B, T, H, hd, scale, s) : SFRON_ERR_UNSUPPORTED;
  if (T % 64 != 0) return SFRON_ERR_UNSUPPORTED;          // longer sequences run on 64-row tiles
  SFRON_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)o) & 15) == 0);
  // any head_dim that is a multiple of 8 up to 80 runs on the 64- or 96-column images with 3 / 4 / 5 output d-tiles (columns beyond
  // head_dim are zero padding): DiT 64 / 72, the LDM UNet's 40 and 80
  if (hd % 8 != 0 || hd < 8) return SFRON_ERR_UNSUPPORTED;
  if (hd <= 48) return launch_fwd<64, 2, 3>((const __bf16*)qkv, (__bf16*)o, lse, B, T, H, hd, scale, s);
  if (hd <= 64) return launch_fwd<64, 2, 4>((const __bf16*)qkv, (__bf16*)o, lse, B, T, H, hd, scale, s);
  if (hd <= 80) return launch_fwd<96, 3, 5>((const __bf16*)qkv, (__bf16*)o, lse, B, T, H, hd, scale, s);
  return SFRON_ERR_UNSUPPORTED;          // (88 / 96 would need a sixth output d-tile: rounds 1-3 accepted them and left columns 80.. unwritten)
}

#ifdef SFRON_DEBUG_KNOBS
/* diagnostic build: arm (out == null) or read back n_wg x 8 stamps (tools/attn_probe.py) */
int sfron_dbg_attn_clock(long long* out, int n_wg) {
  static long long* buf = nullptr;
  if (!buf) {
    if (hipMalloc(&buf, 4096 * 8 * sizeof(long long)) != hipSuccess) return (int)hipGetLastError();
    (void)hipMemset(buf, 0, 4096 * 8 * sizeof(long long));
    if (hipMemcpyToSymbol(HIP_SYMBOL(d_attn_clk), &buf, sizeof(buf)) != hipSuccess) return (int)hipGetLastError();
  }
  if (out) { (void)hipDeviceSynchronize(); if (hipMemcpy(out, buf, (size_t)(n_wg > 4096 ? 4096 : n_wg) * 8 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return (int)hipGetLastError(); }
  return SFRON_OK;
}
#endif

/* test hook: 2 = force the two-kernel backward (dQ, then dK/dV) for every T; 0 = default (fused where T is 128 or 256) */
int sfron_attn_bwd_form(int form) { const int old = g_bwd_form; g_bwd_form = form; return old; }
int sfron_attn_fwd_form(int form) { const int old = g_fwd_form; g_fwd_form = (form == 2 || form == 4 || form == 8 || form == 16) ? form : 0; return old; }

int sfron_attn_bwd(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse, float* delta_scratch,
                   uint16_t* dqkv, int B, int T, int H, int hd, void* stream) {
  SFRON_CHECK_ARG(qkv && o && d_o && lse && delta_scratch && dqkv && B > 0 && H > 0 && T > 0 && hd > 0);
  const float scale = 1.0f / sqrtf((float)hd);
  hipStream_t s = (hipStream_t)stream;
  if (T < 64)
    return hd <= 128 ? launch_small_bwd((const __bf16*)qkv, (const __bf16*)o, (const __bf16*)d_o, lse, (__bf16*)dqkv, B, T, H, hd, scale, s)
                     : SFRON_ERR_UNSUPPORTED;
  if (T % 64 != 0) return SFRON_ERR_UNSUPPORTED;
  SFRON_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)o | (uintptr_t)d_o | (uintptr_t)dqkv) & 15) == 0);
  if (hd % 8 != 0 || hd < 8) return SFRON_ERR_UNSUPPORTED;
  if (hd <= 48)
    return launch_bwd<64, 2, 3>((const __bf16*)qkv, (const __bf16*)o, (const __bf16*)d_o, lse, delta_scratch, (__bf16*)dqkv, B, T, H, hd, scale, s);
  if (hd <= 64)
    return launch_bwd<64, 2, 4>((const __bf16*)qkv, (const __bf16*)o, (const __bf16*)d_o, lse, delta_scratch, (__bf16*)dqkv, B, T, H, hd, scale, s);
  if (hd <= 80)
    return launch_bwd<96, 3, 5>((const __bf16*)qkv, (const __bf16*)o, (const __bf16*)d_o, lse, delta_scratch, (__bf16*)dqkv, B, T, H, hd, scale, s);
  return SFRON_ERR_UNSUPPORTED;
}

/* 1 when sfron_attn_bwd_bias accepts this sequence length (the one-kernel backward: T = 128 / 256) */
int sfron_attn_bwd_bias_supported(int T) { return (T == 256 || T == 128) && g_bwd_form != 2 ? 1 : 0; }

int sfron_attn_bwd_bias(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse, uint16_t* dqkv, float* bias_partials,
                        int B, int T, int H, int hd, void* stream) {
  SFRON_CHECK_ARG(qkv && o && d_o && lse && dqkv && bias_partials && B > 0 && H > 0 && T > 0);
  SFRON_CHECK_ARG((((uintptr_t)qkv | (uintptr_t)o | (uintptr_t)d_o | (uintptr_t)dqkv) & 15) == 0);
  if (!sfron_attn_bwd_bias_supported(T) || hd % 8 != 0 || hd < 8) return SFRON_ERR_UNSUPPORTED;
  const float scale = 1.0f / sqrtf((float)hd);
  hipStream_t s = (hipStream_t)stream;
  if (hd <= 48)
    return launch_bwd<64, 2, 3>((const __bf16*)qkv, (const __bf16*)o, (const __bf16*)d_o, lse, nullptr, (__bf16*)dqkv, B, T, H, hd, scale, s, bias_partials);
  if (hd <= 64)
    return launch_bwd<64, 2, 4>((const __bf16*)qkv, (const __bf16*)o, (const __bf16*)d_o, lse, nullptr, (__bf16*)dqkv, B, T, H, hd, scale, s, bias_partials);
  if (hd <= 80)
    return launch_bwd<96, 3, 5>((const __bf16*)qkv, (const __bf16*)o, (const __bf16*)d_o, lse, nullptr, (__bf16*)dqkv, B, T, H, hd, scale, s, bias_partials);
  return SFRON_ERR_UNSUPPORTED;
}

}  // extern "C"
