// xent_variants.hip -- the --loss_function branches of Z's CrossEntropyLoss.calculate_loss (Z/losses.py:64-168, Z = youtube-8m-zhangteng):
//   loss = mean_b sum_v -c + m,  e = eps, ce(q, t) = t log(q + e) + (1 - t) log(1 - q + e)
//   SQUARE   c = ce(p p, y)                                             WEIGHT   c = 10 y log(p + e) + (1 - y) log(1 - p + e)
//   SQRT     c = ce(sqrt p, y)                                          MARGIN   c = ce(p, y), m = -(pos - neg)         (below)
//   JSD      c = KL-like mix of p and y around d = (1 - a) y + a p      RELABEL  c = 0, m = ce on the labels plus each row's argmax
//   MIX      c = ce(p, y) + ce(y, p) - ce(p, p)                                  when the plain loss is not below 10    (below)
// The passes are those of losses.hip: grid = (ceil(V / 1024), B), 256 threads x 4 labels; a reducing pass leaves one partial per workgroup
// and quantity ([quantity][workgroup]) and a one-workgroup finishing kernel adds them in a fixed order in fp64.  No floating-point atomics,
// no host synchronisation: what the backward pass needs of the batch stays in a small device block ("stats") and, for RELABEL, in the
// rows' argmax ([B] int32).  VEC: V % 4 == 0 and 16-byte aligned operands -- a thread then owns four adjacent labels (one 16-byte load
// of p, one 16- or 4-byte load of the labels, one 16-byte store of dp); otherwise it owns columns t, t + 256, t + 512, t + 768.
#include "loss_common.h"
#include <limits.h>

using namespace yt8m;

namespace {

// stats: device float[YT8M_XV_STATS_FLOATS]
enum {
  XV_LOSS = YT8M_XV_STAT_LOSS,      // the loss itself (what loss_out receives)
  XV_PRE = YT8M_XV_STAT_PRE,        // mean_b sum_v of the plain cross entropy (MARGIN, RELABEL)
  XV_FLAG = YT8M_XV_STAT_FLAG,      // RELABEL: 1 when the relabelled branch was taken (pre < 10 is false), else 0
  XV_POS = YT8M_XV_STAT_POS,        // MARGIN: pos, neg
  XV_NEG = YT8M_XV_STAT_NEG,
  XV_KP,                            // MARGIN: mean_b(sum_v y) / sum(wp), sum(p wp) / sum(wp): d pos / d p_j = kp (d(p wp)_j - rp d(wp)_j)
  XV_RP,
  XV_KN,                            // likewise for neg
  XV_RN,
  XV_USED,
  XV_STATS = YT8M_XV_STATS_FLOATS
};
static_assert(XV_USED <= XV_STATS, "stats block too small");

// the four labels of this thread: columns (col[k] >= V: none), predictions and labels as floats
template <typename LT, bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, const LT* __restrict__ y, int64_t base, int64_t V, int64_t (&col)[4],
                                      float (&pv)[4], float (&yv)[4]) {
  if (VEC) {
    const int64_t c0 = (int64_t)blockIdx.x * TILE + threadIdx.x * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) { col[k] = c0 + k; pv[k] = 0.5f; yv[k] = 0.f; }
    if (c0 < V) {                                                              // V % 4 == 0: all four or none
      const float4 q = *reinterpret_cast<const float4*>(p + base + c0);
      pv[0] = q.x; pv[1] = q.y; pv[2] = q.z; pv[3] = q.w;
      if (sizeof(LT) == 4) {
        const float4 t = *reinterpret_cast<const float4*>(y + base + c0);
        yv[0] = t.x; yv[1] = t.y; yv[2] = t.z; yv[3] = t.w;
      } else {
        const uchar4 t = *reinterpret_cast<const uchar4*>(y + base + c0);
        yv[0] = (float)t.x; yv[1] = (float)t.y; yv[2] = (float)t.z; yv[3] = (float)t.w;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      col[k] = (int64_t)blockIdx.x * TILE + k * 256 + threadIdx.x;
      pv[k] = 0.5f;
      yv[k] = 0.f;
      if (col[k] < V) { pv[k] = p[base + col[k]]; yv[k] = (float)y[base + col[k]]; }
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ dp, int64_t base, int64_t V, const int64_t (&col)[4], const float (&g)[4]) {
  if (VEC) {
    if (col[0] < V) *reinterpret_cast<float4*>(dp + base + col[0]) = make_float4(g[0], g[1], g[2], g[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (col[k] < V) dp[base + col[k]] = g[k];
  }
}

// d/dp of p log(p + e) + (1 - p) log(1 - p + e)
__device__ __forceinline__ float self_entropy_grad(float p, float eps) {
  const float u = p + eps, w = 1.0f - p + eps;
  return (logf(u) + p / u) - (logf(w) + (1.0f - p) / w);
}

// -c of one element of a pointwise kind
template <int KIND>
__device__ __forceinline__ float xv_value(float p, float y, float a, float eps) {
  if (KIND == YT8M_XV_SQUARE) return ce_term(p * p, y, eps);
  if (KIND == YT8M_XV_SQRT) return ce_term(sqrtf(p), y, eps);
  if (KIND == YT8M_XV_JSD) {
    const float d = (1.0f - a) * y + a * p, l1 = logf(d + eps), l2 = logf(1.0f - d + eps);
    const float c1 = (1.0f - a) * p * l1 + (1.0f - a) * (1.0f - p) * l2 + a * y * l1 + a * (1.0f - y) * l2;
    const float c2 = (1.0f - a) * p * logf(p + eps) + (1.0f - a) * (1.0f - p) * logf(1.0f - p + eps);
    return -(c1 - c2);
  }
  if (KIND == YT8M_XV_MIX) {
    const float c2 = p * logf(y + eps) + (1.0f - p) * logf(1.0f - y + eps);
    const float c3 = p * logf(p + eps) + (1.0f - p) * logf(1.0f - p + eps);
    return ce_term(p, y, eps) - (c2 - c3);
  }
  if (KIND == YT8M_XV_WEIGHT) return -(y * logf(p + eps) * 10.0f + (1.0f - y) * logf(1.0f - p + eps));
  return ce_term(p, y, eps);                                                   // MARGIN, RELABEL: the plain term
}

// d(-c)/dp of one element of a pointwise kind
template <int KIND>
__device__ __forceinline__ float xv_grad(float p, float y, float a, float eps) {
  if (KIND == YT8M_XV_SQUARE) return ce_grad(p * p, y, eps) * (2.0f * p);
  if (KIND == YT8M_XV_SQRT) {
    const float q = sqrtf(p);
    return ce_grad(q, y, eps) * (0.5f / q);                                    // p = 0: what the formula gives
  }
  if (KIND == YT8M_XV_JSD) {
    const float d = (1.0f - a) * y + a * p, u = d + eps, w = 1.0f - d + eps;
    const float m1 = (1.0f - a) * p + a * y, m2 = (1.0f - a) * (1.0f - p) + a * (1.0f - y);
    const float dc1 = (1.0f - a) * (logf(u) - logf(w)) + a * (m1 / u - m2 / w);
    return -(dc1 - (1.0f - a) * self_entropy_grad(p, eps));
  }
  if (KIND == YT8M_XV_MIX) return ce_grad(p, y, eps) - ((logf(y + eps) - logf(1.0f - y + eps)) - self_entropy_grad(p, eps));
  if (KIND == YT8M_XV_WEIGHT) return -(10.0f * y / (p + eps) - (1.0f - y) / (1.0f - p + eps));
  return ce_grad(p, y, eps);
}

// ------------------------------------------------------------------------------------------------
// forward pass.  part: [NQ][G] floats; pointwise kinds and RELABEL: the sum of -c; MARGIN: seven sums (ce, p wp, wp, y, p wn, wn, 1 - y);
// RELABEL also [G] maxima of p and [G] int32 columns of the first of them (the lowest column wins a tie, as tf.arg_max).
template <int KIND, typename LT, bool VEC>
__global__ __launch_bounds__(256) void xv_fwd_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V, float a, float eps,
                                                     float* __restrict__ part, int64_t G) {
  constexpr int NQ = KIND == YT8M_XV_MARGIN ? 7 : 1;
  __shared__ float red[4 * NQ];
  __shared__ float best_v[4];
  __shared__ int best_c[4];
  const int64_t base = (int64_t)blockIdx.y * V;
  int64_t col[4];
  float pv[4], yv[4];
  load4<LT, VEC>(p, y, base, V, col, pv, yv);
  float v[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) v[q] = 0.f;
  float bv = -INFINITY;
  int bc = INT_MAX;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (col[k] < V) {
      v[0] += xv_value<KIND>(pv[k], yv[k], a, eps);
      if constexpr (KIND == YT8M_XV_MARGIN) {
        const float wp = (0.5f - logf(pv[k] + eps)) * yv[k], wn = (1.0f - yv[k]) * (0.5f - logf(1.0f - pv[k] + eps));
        v[1] += pv[k] * wp;
        v[2] += wp;
        v[3] += yv[k];
        v[4] += pv[k] * wn;
        v[5] += wn;
        v[6] += 1.0f - yv[k];
      }
      if (KIND == YT8M_XV_RELABEL && pv[k] > bv) { bv = pv[k]; bc = (int)col[k]; }     // columns rise with k: the first maximum stays
    }
  }
  block_sums_256<NQ>(v, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) part[(int64_t)q * G + wg_index()] = v[q];
  }
  if (KIND == YT8M_XV_RELABEL) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
    }
    if ((threadIdx.x & 63) == 0) { best_v[threadIdx.x >> 6] = bv; best_c[threadIdx.x >> 6] = bc; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w)
        if (best_v[w] > bv || (best_v[w] == bv && best_c[w] < bc)) { bv = best_v[w]; bc = best_c[w]; }
      part[G + wg_index()] = bv;
      reinterpret_cast<int*>(part)[2 * G + wg_index()] = bc;
    }
  }
}

// the stats block of a call: the named floats, zeros behind them (a forward call defines every float)
__device__ __forceinline__ void write_stats(float* __restrict__ stats, float* __restrict__ loss_out, float loss, float pre, float flag,
                                            float pos, float neg, float kp, float rp, float kn, float rn) {
  loss_out[0] = loss;
  stats[XV_LOSS] = loss;
  stats[XV_PRE] = pre;
  stats[XV_FLAG] = flag;
  stats[XV_POS] = pos;
  stats[XV_NEG] = neg;
  stats[XV_KP] = kp;
  stats[XV_RP] = rp;
  stats[XV_KN] = kn;
  stats[XV_RN] = rn;
  for (int i = XV_USED; i < XV_STATS; ++i) stats[i] = 0.f;
}

__global__ __launch_bounds__(1024) void xv_sum_finish_kernel(const float* __restrict__ part, int64_t G, double inv_rows,
                                                             float* __restrict__ stats, float* __restrict__ loss_out) {
  __shared__ double red[16];
  double t[1];
  finish_sums_1024<1>(part, G, t, red);
  if (threadIdx.x == 0) write_stats(stats, loss_out, (float)(t[0] * inv_rows), 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
}

// MARGIN: pos = sum(p wp) / sum(wp) mean_b(sum_v y), neg likewise over the negatives; no positive (or no negative) in the batch: 0 / 0
__global__ __launch_bounds__(1024) void xv_margin_finish_kernel(const float* __restrict__ part, int64_t G, double inv_rows,
                                                                float* __restrict__ stats, float* __restrict__ loss_out) {
  __shared__ double red[7 * 16];
  double t[7];
  finish_sums_1024<7>(part, G, t, red);
  if (threadIdx.x == 0) {
    const double pre = t[0] * inv_rows, my = t[3] * inv_rows, mn = t[6] * inv_rows;
    const double rp = t[1] / t[2], rn = t[4] / t[5];
    const double pos = rp * my, neg = rn * mn;
    write_stats(stats, loss_out, (float)(pre - (pos - neg)), (float)pre, 0.f, (float)pos, (float)neg, (float)(my / t[2]), (float)rp,
                (float)(mn / t[5]), (float)rn);
  }
}

// RELABEL: pre, the branch, the rows' argmax (the row's workgroups in column order: the first maximum stays) and the loss.  Adding the
// label at column a of a row turns that element's term from -(y log(p + e) + (1 - y) log(1 - p + e)) into -log(p + e): the relabelled
// loss is pre plus mean_b (1 - y_a) (log(1 - p_a + e) - log(p_a + e)).
template <typename LT>
__global__ __launch_bounds__(1024) void xv_relabel_finish_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t B,
                                                                 int64_t V, float eps, const float* __restrict__ part, int64_t G,
                                                                 int64_t wg_per_row, float* __restrict__ stats,
                                                                 int* __restrict__ argmax, float* __restrict__ loss_out) {
  __shared__ double red[16];
  double t[1];
  finish_sums_1024<1>(part, G, t, red);
  const int* part_c = reinterpret_cast<const int*>(part) + 2 * G;
  double extra = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += 1024) {
    float bv = -INFINITY;
    int bc = INT_MAX;
    for (int64_t j = 0; j < wg_per_row; ++j) {
      const float ov = part[G + b * wg_per_row + j];
      if (ov > bv) { bv = ov; bc = part_c[b * wg_per_row + j]; }
    }
    if (bc == INT_MAX) bc = 0;                                                 // a row of NaN: column 0
    argmax[b] = bc;
    const float pa = p[b * V + bc], ya = (float)y[b * V + bc];
    extra += (double)((1.0f - ya) * (logf(1.0f - pa + eps) - logf(pa + eps)));
  }
  extra = wave_sum_d(extra);
  __syncthreads();                                                             // red: read by every thread above
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = extra;
  __syncthreads();
  if (threadIdx.x == 0) {
    extra = 0.0;
    for (int k = 0; k < 16; ++k) extra += red[k];
    const double inv_rows = 1.0 / (double)B;
    const float pre = (float)(t[0] * inv_rows);
    const bool relabel = !(pre < 10.0f);                                       // tf.cond(tf.less(pre, 10), f1, f2)
    write_stats(stats, loss_out, relabel ? (float)((t[0] + extra) * inv_rows) : pre, pre, relabel ? 1.0f : 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
                0.f);
  }
}

// ------------------------------------------------------------------------------------------------
// backward: dL/dp in one pass over (p, y), for MARGIN and RELABEL also over the stats block (and the rows' argmax).
// inv_rows: the 1 / B of the batch mean; dscale: the upstream scalar of the host, times the device's.
template <int KIND, typename LT, bool VEC>
__global__ __launch_bounds__(256) void xv_bwd_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V, float a, float eps,
                                                     const float* __restrict__ stats, const int* __restrict__ argmax, float inv_rows,
                                                     float dscale, const float* __restrict__ up_dev, float* __restrict__ dp) {
  if (up_dev) dscale *= up_dev[0];
  const int64_t base = (int64_t)blockIdx.y * V;
  int64_t col[4];
  float pv[4], yv[4], g[4];
  load4<LT, VEC>(p, y, base, V, col, pv, yv);
  float kp = 0.f, rp = 0.f, kn = 0.f, rn = 0.f;
  int64_t added = -1;
  if (KIND == YT8M_XV_MARGIN) { kp = stats[XV_KP]; rp = stats[XV_RP]; kn = stats[XV_KN]; rn = stats[XV_RN]; }
  if (KIND == YT8M_XV_RELABEL && stats[XV_FLAG] != 0.f) added = argmax[blockIdx.y];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float pk = pv[k];
    float yk = yv[k];
    if (KIND == YT8M_XV_RELABEL && col[k] == added) yk = yk + (1.0f - yk);     // y' = y + add (1 - y)
    float gk = xv_grad<KIND>(pk, yk, a, eps) * inv_rows;
    if (KIND == YT8M_XV_MARGIN) {
      const float u = pk + eps, w = 1.0f - pk + eps;
      const float d_pwp = yk * (0.5f - logf(u) - pk / u), d_wp = -yk / u;      // d (p wp) / dp, d wp / dp
      const float d_pwn = (1.0f - yk) * (0.5f - logf(w) + pk / w), d_wn = (1.0f - yk) / w;
      gk += kn * (d_pwn - rn * d_wn) - kp * (d_pwp - rp * d_wp);
    }
    g[k] = gk * dscale;
  }
  store4<VEC>(dp, base, V, col, g);
}

inline bool kind_ok(int kind) { return kind >= YT8M_XV_SQUARE && kind <= YT8M_XV_RELABEL; }
inline bool vec_ok(const float* p, const void* labels, int label_dtype, const float* dp, int64_t V) {
  const bool lab = label_dtype == YT8M_LABEL_F32 ? aligned16(labels) : (reinterpret_cast<uintptr_t>(labels) & 3) == 0;
  return (V & 3) == 0 && aligned16(p) && lab && aligned16(dp);
}

// launches kernel<KIND, uint8_t or float, VEC>; the labels go in as the second kernel argument
#define XV_LAUNCH_KIND(kernel, KIND, vec, grid, s, p, labels, dt, ...)                                                          \
  do {                                                                                                                        \
    if ((dt) == YT8M_LABEL_U8) {                                                                                              \
      if (vec) hipLaunchKernelGGL((kernel<KIND, uint8_t, true>), grid, dim3(256), 0, s, p, static_cast<const uint8_t*>(labels), __VA_ARGS__); \
      else hipLaunchKernelGGL((kernel<KIND, uint8_t, false>), grid, dim3(256), 0, s, p, static_cast<const uint8_t*>(labels), __VA_ARGS__);   \
    } else {                                                                                                                  \
      if (vec) hipLaunchKernelGGL((kernel<KIND, float, true>), grid, dim3(256), 0, s, p, static_cast<const float*>(labels), __VA_ARGS__);    \
      else hipLaunchKernelGGL((kernel<KIND, float, false>), grid, dim3(256), 0, s, p, static_cast<const float*>(labels), __VA_ARGS__);       \
    }                                                                                                                         \
  } while (0)
#define XV_LAUNCH(kernel, kind, ...)                                                    \
  switch (kind) {                                                                       \
    case YT8M_XV_SQUARE: XV_LAUNCH_KIND(kernel, YT8M_XV_SQUARE, __VA_ARGS__); break;     \
    case YT8M_XV_SQRT: XV_LAUNCH_KIND(kernel, YT8M_XV_SQRT, __VA_ARGS__); break;         \
    case YT8M_XV_JSD: XV_LAUNCH_KIND(kernel, YT8M_XV_JSD, __VA_ARGS__); break;           \
    case YT8M_XV_MIX: XV_LAUNCH_KIND(kernel, YT8M_XV_MIX, __VA_ARGS__); break;           \
    case YT8M_XV_WEIGHT: XV_LAUNCH_KIND(kernel, YT8M_XV_WEIGHT, __VA_ARGS__); break;     \
    case YT8M_XV_MARGIN: XV_LAUNCH_KIND(kernel, YT8M_XV_MARGIN, __VA_ARGS__); break;     \
    default: XV_LAUNCH_KIND(kernel, YT8M_XV_RELABEL, __VA_ARGS__); break;                \
  }

}  // namespace

extern "C" int64_t yt8m_xent_variant_workspace_bytes(int64_t B, int64_t V) {
  if (B <= 0 || V <= 0) return 0;
  return 7 * wg_count(B, V) * (int64_t)sizeof(float);               // the widest set of partials: the seven sums of MARGIN
}

extern "C" int yt8m_xent_variant_fwd(int kind, const float* p, const void* labels, int label_dtype, float* loss_out, float* stats,
                                     int32_t* argmax, int64_t B, int64_t V, float c0, float eps, void* workspace, yt8m_stream_t stream) {
  YT8M_REQUIRE(kind_ok(kind), YT8M_E_BADARG, "loss kind");
  YT8M_LOSS_REQUIRE_SHAPE(B, V);
  YT8M_REQUIRE(V <= INT_MAX - TILE, YT8M_E_SHAPE, "V does not fit the int32 argmax");
  YT8M_REQUIRE(p && labels && loss_out && stats && workspace, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(kind != YT8M_XV_RELABEL || argmax, YT8M_E_BADARG, "null operand: loss_relabel needs the [B] argmax buffer");
  YT8M_LOSS_REQUIRE_LABELS(label_dtype);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  float* part = static_cast<float*>(workspace);
  const int64_t G = wg_count(B, V), per_row = (V + TILE - 1) / TILE;
  const dim3 grid((unsigned)per_row, (unsigned)B);
  const bool vec = vec_ok(p, labels, label_dtype, nullptr, V);
  const double inv_rows = 1.0 / (double)B;
  XV_LAUNCH(xv_fwd_kernel, kind, vec, grid, s, p, labels, label_dtype, V, c0, eps, part, G);
  if (kind == YT8M_XV_MARGIN) {
    hipLaunchKernelGGL(xv_margin_finish_kernel, dim3(1), dim3(1024), 0, s, (const float*)part, G, inv_rows, stats, loss_out);
  } else if (kind == YT8M_XV_RELABEL) {
    if (label_dtype == YT8M_LABEL_U8)
      hipLaunchKernelGGL((xv_relabel_finish_kernel<uint8_t>), dim3(1), dim3(1024), 0, s, p, static_cast<const uint8_t*>(labels), B, V, eps,
                         (const float*)part, G, per_row, stats, argmax, loss_out);
    else
      hipLaunchKernelGGL((xv_relabel_finish_kernel<float>), dim3(1), dim3(1024), 0, s, p, static_cast<const float*>(labels), B, V, eps,
                         (const float*)part, G, per_row, stats, argmax, loss_out);
  } else {
    hipLaunchKernelGGL(xv_sum_finish_kernel, dim3(1), dim3(1024), 0, s, (const float*)part, G, inv_rows, stats, loss_out);
  }
  return launch_status("xent_variant_fwd");
}

extern "C" int yt8m_xent_variant_bwd(int kind, const float* p, const void* labels, int label_dtype, const float* stats,
                                     const int32_t* argmax, const float* upstream_dev, float* dp, int64_t B, int64_t V, float c0, float eps,
                                     float upstream, yt8m_stream_t stream) {
  YT8M_REQUIRE(kind_ok(kind), YT8M_E_BADARG, "loss kind");
  YT8M_LOSS_REQUIRE_SHAPE(B, V);
  YT8M_REQUIRE(V <= INT_MAX - TILE, YT8M_E_SHAPE, "V does not fit the int32 argmax");
  YT8M_REQUIRE(p && labels && dp, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE((kind != YT8M_XV_MARGIN && kind != YT8M_XV_RELABEL) || stats, YT8M_E_BADARG,
               "null operand: loss_margin and loss_relabel need the stats of their forward call");
  YT8M_REQUIRE(kind != YT8M_XV_RELABEL || argmax, YT8M_E_BADARG, "null operand: loss_relabel needs the [B] argmax buffer");
  YT8M_LOSS_REQUIRE_LABELS(label_dtype);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)((V + TILE - 1) / TILE), (unsigned)B);
  const bool vec = vec_ok(p, labels, label_dtype, dp, V);
  XV_LAUNCH(xv_bwd_kernel, kind, vec, grid, s, p, labels, label_dtype, V, c0, eps, stats, argmax, 1.0f / (float)B, upstream, upstream_dev,
            dp);
  return launch_status("xv_bwd_kernel");
}
