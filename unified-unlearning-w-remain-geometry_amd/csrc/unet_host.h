// Host helpers shared by the U-Net files (conv.hip, groupnorm.hip, rows.hip).  Not in common.h: fp8.hip, sweep.hip and embed.hip
// each keep a grid_for with a cap of their own, and a second one at global scope makes their calls ambiguous.
#pragma once
#include "common.h"
#include "../../include/sfron.h"

constexpr int TPB = 256;
static inline int grid_for(int64_t n, int per = TPB) {
  int64_t b = (n + per - 1) / per;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
// an unfinished split-K result (sfron_split_src) as the input of sfron_split_finish / sfron_groupnorm_*_src: float4-addressable
static inline bool split_src_ok(const sfron_split_src* s, int C) {
  return s && s->slabs && s->n_slabs >= 1 && s->slab_stride > 0 && C % 4 == 0 && (((uintptr_t)s->slabs | (uintptr_t)s->bias | (uintptr_t)s->sample_vec |
         (uintptr_t)s->resid) & 15) == 0 && s->slab_stride % 4 == 0 && (!s->sample_vec || s->ld_vec % 4 == 0) && (!s->resid || s->ld_resid % 4 == 0);
}
