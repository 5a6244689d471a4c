// loss_common.h -- what the label-loss files (losses.hip, xent_variants.hip) share: the tile of their passes, the cross-entropy term and
// its derivative, the fp64 finishing sum of the per-workgroup partials and the argument checks of their entry points.  Every pass runs
// on grid = (ceil(V / 1024), B) with 256 threads x 4 labels; a pass that reduces leaves one partial per workgroup and quantity
// ([quantity][workgroup]) and a one-workgroup finishing kernel sums them in a fixed order.
#pragma once
#include "common.h"
#include <math.h>

constexpr int TILE = 1024;          // labels of one row per workgroup

__device__ __forceinline__ float ce_term(float p, float y, float eps) { return -(y * logf(p + eps) + (1.0f - y) * logf(1.0f - p + eps)); }
__device__ __forceinline__ float ce_grad(float p, float y, float eps) { return -(y / (p + eps) - (1.0f - y) / (1.0f - p + eps)); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one workgroup of 1024 threads: t[q] = sum_i part[q * n + i] in fp64, fixed order; red: NQ * 16 doubles of LDS
template <int NQ>
__device__ __forceinline__ void finish_sums_1024(const float* __restrict__ part, int64_t n, double (&t)[NQ], double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += (double)part[(int64_t)q * n + i];
    s = wave_sum_d(s);
    if (lane == 0) red[q * 16 + w] = s;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double s = 0.0;
    for (int k = 0; k < 16; ++k) s += red[q * 16 + k];
    t[q] = s;
  }
}

__device__ __forceinline__ int64_t wg_index() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }
inline int64_t wg_count(int64_t B, int64_t V) { return B * ((V + TILE - 1) / TILE); }

#define YT8M_LOSS_REQUIRE_SHAPE(B, V)                                                       \
  YT8M_REQUIRE((B) > 0 && (V) > 0, YT8M_E_SHAPE, "empty batch: reduce_mean over 0 rows is undefined"); \
  YT8M_REQUIRE((B) <= 65535, YT8M_E_SHAPE, "B > 65535")
#define YT8M_LOSS_REQUIRE_LABELS(dt) \
  YT8M_REQUIRE((dt) == YT8M_LABEL_U8 || (dt) == YT8M_LABEL_F32, YT8M_E_BADARG, "label dtype")
