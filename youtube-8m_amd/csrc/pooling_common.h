// pooling_common.h -- what the attention pooling files (sigmoid_attention.hip, softmax_attention.hip) share beyond common.h: the
// deterministic finish of their per-workgroup weight-gradient partials and the switch over the compile-time head count.  Everything
// here has internal linkage: each including file gets its own copy of the two kernels.
#pragma once
#include "common.h"

namespace {

constexpr int SUM_GROUP = 32;              // partials per thread of the first summing kernel

// grid (ceil(n / 256), ceil(parts / SUM_GROUP)): dst[g, i] = sum of src[p, i] over the group's parts in the order of p
__global__ __launch_bounds__(256) void sum_groups_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int parts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p0 = blockIdx.y * SUM_GROUP, p1 = min(parts, p0 + SUM_GROUP);
  float r = 0.0f;
  for (int p = p0; p < p1; ++p) r += src[(size_t)p * n + i];
  dst[(size_t)blockIdx.y * n + i] = r;
}

// grid (ceil(n / 256)): the groups in their order; element i goes to d0[i] (i < n0) or d1[i - n0]; either may be null
__global__ __launch_bounds__(256) void sum_final_kernel(const float* __restrict__ src, float* __restrict__ d0, float* __restrict__ d1,
                                                        int n, int n0, int groups) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r = 0.0f;
  for (int g = 0; g < groups; ++g) r += src[(size_t)g * n + i];
  if (i < n0) {
    if (d0) d0[i] = r;
  } else if (d1) {
    d1[i - n0] = r;
  }
}

// parts [nparts, n] -> d0 [n0] | d1 [n - n0], no atomics: the parts in their order within a group of SUM_GROUP, then the groups in
// theirs.  groups: ceil(nparts / SUM_GROUP) * n floats of workspace.
inline int sum_parts(const float* parts, float* groups, int n, int nparts, float* d0, int n0, float* d1, hipStream_t s) {
  const int ngroups = (int)cdiv(nparts, SUM_GROUP);
  hipLaunchKernelGGL(sum_groups_kernel, dim3((unsigned)cdiv(n, 256), (unsigned)ngroups), dim3(256), 0, s, parts, groups, n, nparts);
  const int st = yt8m::launch_status("sum_groups_kernel");
  if (st != YT8M_OK) return st;
  hipLaunchKernelGGL(sum_final_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, groups, d0, d1, n, n0, ngroups);
  return yt8m::launch_status("sum_final_kernel");
}

}  // namespace

// CALL(N) with the run-time head count N (1 .. 8, checked by the caller's shape_ok) as a compile-time constant
#define YT8M_BY_HEADS(N, CALL)   \
  switch (N) {                   \
    case 1: CALL(1) break;       \
    case 2: CALL(2) break;       \
    case 3: CALL(3) break;       \
    case 4: CALL(4) break;       \
    case 5: CALL(5) break;       \
    case 6: CALL(6) break;       \
    case 7: CALL(7) break;       \
    default: CALL(8) break;      \
  }
