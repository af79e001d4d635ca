// LDS tile helpers of the matrix-core files (gemm.hip, conv.hip, attn.hip): the XOR-swizzled tile images, their fragment reads, the
// LDS-DMA issue and the hand-issued LDS reads.  One definition each: the swizzle has to agree between the staging store, the LDS-DMA
// source address and the fragment read.
#pragma once
#include "common.h"
#include <utility>

// ---- LDS images -------------------------------------------------------------------------------
// direct image: [128 rows][64 k], 128-B rows, 16-B chunk c of row r stored at chunk c ^ (r & 7)
__device__ __forceinline__ int off_direct(int row, int ch) { return row * 64 + ((ch ^ (row & 7)) << 3); }
// transposed-read image: [64 k-rows][128 cols], 256-B rows, chunk c of row r at c ^ (((r&3)<<2)|((r>>2)&3))
__device__ __forceinline__ int swz_tr(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }
__device__ __forceinline__ int off_tr(int krow, int ch) { return krow * 128 + ((ch ^ swz_tr(krow)) << 3); }

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef __attribute__((address_space(3))) void lptr_t;

__device__ __forceinline__ bf16x8 frag_direct(const __bf16* img, int row, int kchunk) {
  return *reinterpret_cast<const bf16x8*>(img + off_direct(row, kchunk));
}
// fragment for 16 consecutive columns starting at col0 (multiple of 16), k rows kr0 + 8*(lane>>4) + 0..7
__device__ __forceinline__ bf16x8 frag_tr(const __bf16* img, int col0, int kr0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int ch = (col0 >> 3) + (p >> 1);
  const int r0 = kr0 + 8 * g + q;
  const __bf16* a0 = img + off_tr(r0, ch) + 4 * (p & 1);
  const __bf16* a1 = img + off_tr(r0 + 4, ch) + 4 * (p & 1);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a0);
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a1);
  bf16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// ---- LDS-DMA ----------------------------------------------------------------------------------
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// one wave-instruction of LDS-DMA: 64 lanes x 16 B from rsrc[voff + soff] to the lane-linear KiB at `dst` (a __device__ helper:
// the builtin inside a kernel template's own lambda breaks hipcc's host pass; register-constraint asm lives in __device__ helpers for
// the same reason: inside a __global__ body the host pass rejects the "v" constraint)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, __bf16* dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t*)dst, 16, voff, soff, 0, 0);
}

// ---- LDS reads through inline asm -------------------------------------------------------------
// While an LDS-DMA is in flight hipcc puts `s_waitcnt vmcnt(0)` in front of every __builtin ds_read_tr16_b64 (it cannot prove the DMA
// does not alias the read), which serialises load and compute for the dgrad / wgrad layouts (wgrad fc1: 181 us = 112 us DMA-only +
// 125 us compute-only with almost no overlap).  An asm read is invisible to that bookkeeping; its completion is waited for explicitly:
// the caller must run lds_reads_done() (`s_waitcnt lgkmcnt(0)` + sched_barrier) before it uses the result.
__device__ __forceinline__ unsigned lds_addr(const __bf16* p) {
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)(const void*)p;
}
__device__ __forceinline__ bf16x4 asm_read_tr(unsigned addr) {
  bf16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
__device__ __forceinline__ bf16x8 asm_read_b128(unsigned addr) {
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
template <int OFF>
__device__ __forceinline__ bf16x4 asm_read_tr_off(unsigned addr) {
  bf16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
template <int OFF>
__device__ __forceinline__ bf16x8 asm_read_b128_off(unsigned addr) {
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
__device__ __forceinline__ void lds_reads_done() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{}) (immediate offsets of the reads above)
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }
