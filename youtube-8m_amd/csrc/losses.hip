// losses.hip -- the label losses of W/losses.py beyond plain cross entropy (elementwise.hip: xent_kernel):
//   BatchAgreementCrossEntropyLoss (:281-320), TopKBatchAgreementCrossEntropyLoss (:322-356) and the pointwise
//   WeightedCrossEntropyLoss / MeanSquareErrorLoss / HingeLoss (:76-108, :132-148).
// Every pass runs on grid = (ceil(V / 1024), B) with 256 threads x 4 labels, as xent_kernel does; a pass that reduces leaves one
// partial per workgroup and quantity ([quantity][workgroup]) and a one-workgroup finishing kernel sums them in a fixed order (in
// fp64: counts stay exact past 2^24 elements).  No floating-point atomics, no host synchronisation: the batch statistics stay in a
// small device block ("stats") that the backward pass reads again.
#include "loss_common.h"

using namespace yt8m;

namespace {

constexpr int TOPK = 20;            // W/losses.py:331 -- k = 20 whatever `topk` says

// stats of BatchAgreementCrossEntropyLoss: device float[YT8M_BA_STATS_FLOATS]
enum {
  BA_MIN_PP = 0,   // min over the batch of p y + (1 - y)
  BA_MAX_NP,       // max over the batch of p (1 - y)
  BA_C_FN,         // centre of the false negatives, sum p fn / n_fn (NaN when there is none: W/losses.py:304)
  BA_C_FP,
  BA_K3,           // 3 / r, r = max(eps, max_np - min_pp)
  BA_WA,           // a n_fp / N: what sigmoid(3 (c_fp - p) / r) fn is weighted with
  BA_WB,           // a n_fn / N
  BA_INV_N_FN,     // 1 / n_fn, 1 / n_fp: d c / d p_j = mask_j / n
  BA_INV_N_FP,
  BA_INV_T_MAX,    // 1 / (number of elements that attain max_np), likewise min_pp: ties share the gradient of an extremum
  BA_INV_T_MIN,
  BA_G_CFP,        // dL/dc_fp, dL/dc_fn, dL/dr (0 where r is the clamp), each without the 1 / B of the batch mean
  BA_G_CFN,
  BA_G_R,
  BA_N_FN,         // the four counts themselves, as floats (exact below 2^24): not read by the kernels; for hosts and tests
  BA_N_FP,
  BA_T_MAX,
  BA_T_MIN,
  BA_SLOW,         // != 0: some statistic is not finite -- every element then goes through the whole formula, so that the NaN of an
                   // empty false-negative / false-positive set reaches every output as it does in the reference
  BA_STATS = YT8M_BA_STATS_FLOATS
};
static_assert(BA_SLOW < BA_STATS, "stats block too small");

__device__ __forceinline__ float pos_pred(float p, float y) { return p * y + (1.0f - y); }   // exact for y in {0, 1}
__device__ __forceinline__ float neg_pred(float p, float y) { return p * (1.0f - y); }

// ------------------------------------------------------------------------------------------------
// BatchAgreementCrossEntropyLoss, pass 1: the two extrema.  part: [2][G] (min_pp, max_np).
template <typename LT>
__global__ __launch_bounds__(256) void ba_extrema_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V,
                                                         float* __restrict__ part, int64_t G) {
  __shared__ float red[4];
  const int64_t base = (int64_t)blockIdx.y * V;
  float neg_min = -INFINITY, mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t l = (int64_t)blockIdx.x * TILE + k * 256 + threadIdx.x;
    if (l < V) {
      const float pv = p[base + l], yv = (float)y[base + l];
      neg_min = fmaxf(neg_min, -pos_pred(pv, yv));
      mx = fmaxf(mx, neg_pred(pv, yv));
    }
  }
  neg_min = block_max_256(neg_min, red);
  mx = block_max_256(mx, red);
  if (threadIdx.x == 0) {
    part[wg_index()] = -neg_min;
    part[G + wg_index()] = mx;
  }
}

__global__ __launch_bounds__(1024) void ba_extrema_finish_kernel(const float* __restrict__ part, int64_t G, float* __restrict__ stats) {
  __shared__ float red[2][16];
  float neg_min = -INFINITY, mx = -INFINITY;
  for (int64_t i = threadIdx.x; i < G; i += 1024) {
    neg_min = fmaxf(neg_min, -part[i]);
    mx = fmaxf(mx, part[G + i]);
  }
  neg_min = wave_max(neg_min);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = neg_min; red[1][threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) { neg_min = fmaxf(neg_min, red[0][k]); mx = fmaxf(mx, red[1][k]); }
    stats[BA_MIN_PP] = -neg_min;
    stats[BA_MAX_NP] = mx;
    for (int i = BA_SLOW + 1; i < BA_STATS; ++i) stats[i] = 0.f;           // the unused tail: a forward call defines every float
  }
}

// pass 2: counts, sums and tie counts.  part: [6][G] (n_fn, n_fp, sum p fn, sum p fp, #max_np, #min_pp); one workgroup's share of
// a count is at most 1024, exact in fp32.
template <typename LT>
__global__ __launch_bounds__(256) void ba_moments_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V,
                                                         const float* __restrict__ stats, float* __restrict__ part, int64_t G) {
  __shared__ float red[6 * 4];
  const float min_pp = stats[BA_MIN_PP], max_np = stats[BA_MAX_NP];
  const int64_t base = (int64_t)blockIdx.y * V;
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t l = (int64_t)blockIdx.x * TILE + k * 256 + threadIdx.x;
    if (l < V) {
      const float pv = p[base + l], yv = (float)y[base + l];
      const float fn = pv < max_np ? yv : 0.f, fp = pv > min_pp ? 1.0f - yv : 0.f;
      v[0] += fn;
      v[1] += fp;
      v[2] += pv * fn;
      v[3] += pv * fp;
      v[4] += neg_pred(pv, yv) == max_np ? 1.0f : 0.f;
      v[5] += pos_pred(pv, yv) == min_pp ? 1.0f : 0.f;
    }
  }
  block_sums_256<6>(v, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) part[(int64_t)q * G + wg_index()] = v[q];
  }
}

__global__ __launch_bounds__(1024) void ba_moments_finish_kernel(const float* __restrict__ part, int64_t G, float eps, float agreement,
                                                                 float batch_size, float* __restrict__ stats) {
  __shared__ double red[6 * 16];
  double t[6];
  finish_sums_1024<6>(part, G, t, red);
  if (threadIdx.x == 0) {
    const float c_fn = (float)(t[2] / t[0]), c_fp = (float)(t[3] / t[1]);          // 0 / 0 = NaN, as the reference
    const float r = fmaxf(eps, stats[BA_MAX_NP] - stats[BA_MIN_PP]);
    const float wa = agreement * ((float)t[1] / batch_size), wb = agreement * ((float)t[0] / batch_size);
    stats[BA_C_FN] = c_fn;
    stats[BA_C_FP] = c_fp;
    stats[BA_K3] = 3.0f / r;
    stats[BA_WA] = wa;
    stats[BA_WB] = wb;
    stats[BA_INV_N_FN] = (float)(1.0 / t[0]);
    stats[BA_INV_N_FP] = (float)(1.0 / t[1]);
    stats[BA_INV_T_MAX] = (float)(1.0 / t[4]);
    stats[BA_INV_T_MIN] = (float)(1.0 / t[5]);
    stats[BA_N_FN] = (float)t[0];
    stats[BA_N_FP] = (float)t[1];
    stats[BA_T_MAX] = (float)t[4];
    stats[BA_T_MIN] = (float)t[5];
    stats[BA_SLOW] = (isfinite(c_fn) && isfinite(c_fp) && isfinite(wa) && isfinite(wb) && t[0] > 0.0 && t[1] > 0.0) ? 0.f : 1.0f;
  }
}

// the weight of one element and what its derivative needs: w = 1 + wa s1 fn + wb s2 fp, d1 = wa fn s1 (1 - s1), d2 = wb fp s2 (1 - s2)
struct BaWeight { float w, d1, d2, u1, u2; };
__device__ __forceinline__ BaWeight ba_weight(float pv, float fn, float fp, float c_fn, float c_fp, float k3, float wa, float wb) {
  BaWeight o;
  o.u1 = c_fp - pv;
  o.u2 = pv - c_fn;
  const float s1 = sigmoidf_(o.u1 * k3), s2 = sigmoidf_(o.u2 * k3);
  o.w = 1.0f + (wa * s1 * fn + wb * s2 * fp);
  o.d1 = wa * fn * (s1 * (1.0f - s1));
  o.d2 = wb * fp * (s2 * (1.0f - s2));
  return o;
}

// pass 3: the loss and the three sums of the backward pass.  part: [4][G] (sum w ce, sum ce d1, sum ce d2, sum ce (d1 u1 + d2 u2)).
// An element that is neither a false negative nor a false positive has w = 1 exactly and adds nothing to the other sums.
template <typename LT>
__global__ __launch_bounds__(256) void ba_loss_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V, float eps,
                                                      const float* __restrict__ stats, float* __restrict__ part, int64_t G) {
  __shared__ float red[4 * 4];
  const float min_pp = stats[BA_MIN_PP], max_np = stats[BA_MAX_NP], c_fn = stats[BA_C_FN], c_fp = stats[BA_C_FP];
  const float k3 = stats[BA_K3], wa = stats[BA_WA], wb = stats[BA_WB];
  const bool slow = stats[BA_SLOW] != 0.f;
  const int64_t base = (int64_t)blockIdx.y * V;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t l = (int64_t)blockIdx.x * TILE + k * 256 + threadIdx.x;
    if (l < V) {
      const float pv = p[base + l], yv = (float)y[base + l];
      const float fn = pv < max_np ? yv : 0.f, fp = pv > min_pp ? 1.0f - yv : 0.f;
      const float ce = ce_term(pv, yv, eps);
      if (slow || fn != 0.f || fp != 0.f) {
        const BaWeight o = ba_weight(pv, fn, fp, c_fn, c_fp, k3, wa, wb);
        v[0] += o.w * ce;
        v[1] += ce * o.d1;
        v[2] += ce * o.d2;
        v[3] += ce * (o.d1 * o.u1 + o.d2 * o.u2);
      } else {
        v[0] += ce;
      }
    }
  }
  block_sums_256<4>(v, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) part[(int64_t)q * G + wg_index()] = v[q];
  }
}

__global__ __launch_bounds__(1024) void ba_loss_finish_kernel(const float* __restrict__ part, int64_t G, float eps, float inv_rows,
                                                              float* __restrict__ stats, float* __restrict__ loss_out) {
  __shared__ double red[4 * 16];
  double t[4];
  finish_sums_1024<4>(part, G, t, red);
  if (threadIdx.x == 0) {
    const double k3 = (double)stats[BA_K3];
    const bool open = stats[BA_MAX_NP] - stats[BA_MIN_PP] > eps;                    // tf.maximum: the clamp takes the gradient at eps
    loss_out[0] = (float)(t[0] * (double)inv_rows);
    stats[BA_G_CFP] = (float)(k3 * t[1]);
    stats[BA_G_CFN] = (float)(-k3 * t[2]);
    stats[BA_G_R] = open ? (float)(-(k3 * k3 / 3.0) * t[3]) : 0.f;                  // -3 / r^2
  }
}

// backward: dL/dp in one pass over (p, y) and the stats block
template <typename LT>
__global__ __launch_bounds__(256) void ba_bwd_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V, float eps,
                                                     const float* __restrict__ stats, float dscale, const float* __restrict__ up_dev,
                                                     float* __restrict__ dp) {
  const float min_pp = stats[BA_MIN_PP], max_np = stats[BA_MAX_NP], c_fn = stats[BA_C_FN], c_fp = stats[BA_C_FP];
  const float k3 = stats[BA_K3], wa = stats[BA_WA], wb = stats[BA_WB];
  const float g_cfp = stats[BA_G_CFP] * stats[BA_INV_N_FP], g_cfn = stats[BA_G_CFN] * stats[BA_INV_N_FN];
  const float g_max = stats[BA_G_R] * stats[BA_INV_T_MAX], g_min = stats[BA_G_R] * stats[BA_INV_T_MIN];
  const bool slow = stats[BA_SLOW] != 0.f;
  if (up_dev) dscale *= up_dev[0];
  const int64_t base = (int64_t)blockIdx.y * V;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t l = (int64_t)blockIdx.x * TILE + k * 256 + threadIdx.x;
    if (l < V) {
      const float pv = p[base + l], yv = (float)y[base + l];
      const float fn = pv < max_np ? yv : 0.f, fp = pv > min_pp ? 1.0f - yv : 0.f;
      float g = ce_grad(pv, yv, eps);
      if (slow || fn != 0.f || fp != 0.f) {
        const BaWeight o = ba_weight(pv, fn, fp, c_fn, c_fp, k3, wa, wb);
        g = o.w * g + ce_term(pv, yv, eps) * (o.d2 - o.d1) * k3 + g_cfp * fp + g_cfn * fn;
      }
      if (slow || neg_pred(pv, yv) == max_np) g += g_max * (1.0f - yv);
      if (slow || pos_pred(pv, yv) == min_pp) g -= g_min * yv;
      dp[base + l] = g * dscale;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// TopKBatchAgreementCrossEntropyLoss.  stats: float[1 + B] = min_pp, then the rows' thresholds tau_b (the 20th largest value).
// pass 1: tau_b by radix selection, one workgroup per row.  Floats map to keys whose unsigned order is the floats' order; four rounds
// fix the key of the k-th largest element eight bits at a time: a 256-bin histogram (integer LDS atomics) of the elements that share
// the bits fixed so far, suffix sums over the bins, the bin that holds the k-th.  The row (19 KB at V = 4716) is read four times, from
// cache after the first.  Equal values count as often as they occur, as in tf.nn.top_k.
__device__ __forceinline__ unsigned float_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ __launch_bounds__(256) void tk_threshold_kernel(const float* __restrict__ p, int64_t V, float* __restrict__ tau) {
  __shared__ unsigned hist[256];
  __shared__ unsigned wave_total[4];
  __shared__ unsigned sel[2];                                              // the chosen bin, and the rank left inside it
  const float* pr = p + (int64_t)blockIdx.x * V;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned prefix = 0, k = TOPK;
  for (int round = 0; round < 4; ++round) {
    const int shift = 24 - 8 * round;
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t c = threadIdx.x; c < V; c += 256) {
      const unsigned key = float_key(pr[c]);
      if (round == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned h = hist[threadIdx.x];                                  // thread t owns bin t
    unsigned incl = h;                                                     // the elements in bins >= t
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_down(incl, o, 64);
      if (lane + o < 64) incl += v;
    }
    if (lane == 0) wave_total[w] = incl;
    __syncthreads();
    for (int q = w + 1; q < 4; ++q) incl += wave_total[q];
    if (incl - h < k && k <= incl) {                                       // exactly one bin: the suffix sums fall from >= k to 0
      sel[0] = threadIdx.x;
      sel[1] = k - (incl - h);
    }
    __syncthreads();
    prefix = (prefix << 8) | sel[0];
    k = sel[1];
  }
  if (threadIdx.x == 0) tau[blockIdx.x] = key_float(prefix);
}

// pass 2: per-workgroup minima of p (y m) + 1 - (y m), m = [p >= tau_b].
template <typename LT>
__global__ __launch_bounds__(256) void tk_minpp_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V,
                                                       const float* __restrict__ stats, float* __restrict__ part) {
  __shared__ float red[4];
  const float tau = stats[1 + blockIdx.y];
  const int64_t base = (int64_t)blockIdx.y * V;
  float neg_min = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t l = (int64_t)blockIdx.x * TILE + k * 256 + threadIdx.x;
    if (l < V) {
      const float pv = p[base + l], yv = (float)y[base + l];
      neg_min = fmaxf(neg_min, -pos_pred(pv, pv >= tau ? yv : 0.f));
    }
  }
  neg_min = block_max_256(neg_min, red);
  if (threadIdx.x == 0) part[wg_index()] = -neg_min;
}

__global__ __launch_bounds__(1024) void tk_minpp_finish_kernel(const float* __restrict__ part, int64_t G, float* __restrict__ stats) {
  __shared__ float red[16];
  float neg_min = -INFINITY;
  for (int64_t i = threadIdx.x; i < G; i += 1024) neg_min = fmaxf(neg_min, -part[i]);
  neg_min = wave_max(neg_min);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = neg_min;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) neg_min = fmaxf(neg_min, red[k]);
    stats[0] = -neg_min;
  }
}

// the loss (partial != NULL) or its gradient (dp != NULL): w = 1 + a (fn + fp) is a constant of the differentiation (stop_gradient)
template <typename LT>
__global__ __launch_bounds__(256) void tk_loss_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V, float eps,
                                                      float agreement, const float* __restrict__ stats, float* __restrict__ partial,
                                                      float* __restrict__ dp, float dscale, const float* __restrict__ up_dev) {
  __shared__ float red[4];
  const float min_pp = stats[0], tau = stats[1 + blockIdx.y];
  if (up_dev) dscale *= up_dev[0];
  const int64_t base = (int64_t)blockIdx.y * V;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t l = (int64_t)blockIdx.x * TILE + k * 256 + threadIdx.x;
    if (l < V) {
      const float pv = p[base + l], yv = (float)y[base + l];
      const float fn = pv < tau ? yv : 0.f, fp = (pv >= tau && pv > min_pp) ? 1.0f - yv : 0.f;
      const float w = (fn + fp) * agreement + 1.0f;
      if (partial) s += w * ce_term(pv, yv, eps);
      if (dp) dp[base + l] = w * ce_grad(pv, yv, eps) * dscale;
    }
  }
  if (partial) {
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[wg_index()] = s;
  }
}

__global__ __launch_bounds__(1024) void loss_finish_kernel(const float* __restrict__ part, int64_t G, float inv_rows,
                                                           float* __restrict__ loss_out) {
  __shared__ double red[16];
  double t[1];
  finish_sums_1024<1>(part, G, t, red);
  if (threadIdx.x == 0) loss_out[0] = (float)(t[0] * (double)inv_rows);
}

// ------------------------------------------------------------------------------------------------
// The pointwise losses: value (partial != NULL) and / or gradient (dp != NULL) in one pass, as xent_kernel.
//   YT8M_LOSS_WEIGHTED_XENT: -(c0 y log(p + eps) + c1 (1 - y) log(1 - p + eps))     c0 / c1 = false negative / positive punishment
//   YT8M_LOSS_MSE:           (y - p)^2
//   YT8M_LOSS_HINGE:         max(0, c0 - (2 y - 1) p), subgradient 0 at the kink    c0 = b
template <int KIND, typename LT>
__global__ __launch_bounds__(256) void pointwise_loss_kernel(const float* __restrict__ p, const LT* __restrict__ y, int64_t V, float c0,
                                                             float c1, float eps, float* __restrict__ partial, float* __restrict__ dp,
                                                             float dscale, const float* __restrict__ up_dev) {
  __shared__ float red[4];
  if (up_dev) dscale *= up_dev[0];
  const int64_t base = (int64_t)blockIdx.y * V;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t l = (int64_t)blockIdx.x * TILE + k * 256 + threadIdx.x;
    if (l < V) {
      const float pv = p[base + l], yv = (float)y[base + l];
      float f, g;
      if (KIND == YT8M_LOSS_WEIGHTED_XENT) {
        const float a = pv + eps, c = 1.0f - pv + eps;
        f = -(c0 * yv * logf(a) + c1 * (1.0f - yv) * logf(c));
        g = -(c0 * yv / a - c1 * (1.0f - yv) / c);
      } else if (KIND == YT8M_LOSS_MSE) {
        const float d = yv - pv;
        f = d * d;
        g = -2.0f * d;
      } else {
        const float sign = 2.0f * yv - 1.0f, m = c0 - sign * pv;
        f = fmaxf(0.f, m);
        g = m > 0.f ? -sign : 0.f;
      }
      s += f;
      if (dp) dp[base + l] = g * dscale;
    }
  }
  if (partial) {
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[wg_index()] = s;
  }
}


// launches kernel<..., uint8_t> or kernel<..., float> on the labels' type; the labels go in as the second kernel argument
#define YT8M_LOSS_LAUNCH(kernel_u8, kernel_f32, grid, s, p, labels, dt, ...)                                                       \
  do {                                                                                                                             \
    if ((dt) == YT8M_LABEL_U8)                                                                                                     \
      hipLaunchKernelGGL(kernel_u8, grid, dim3(256), 0, s, p, static_cast<const uint8_t*>(labels), __VA_ARGS__);                   \
    else                                                                                                                           \
      hipLaunchKernelGGL(kernel_f32, grid, dim3(256), 0, s, p, static_cast<const float*>(labels), __VA_ARGS__);                    \
  } while (0)

}  // namespace

extern "C" int64_t yt8m_batch_agreement_workspace_bytes(int64_t B, int64_t V) {
  if (B <= 0 || V <= 0) return 0;
  return 6 * wg_count(B, V) * (int64_t)sizeof(float);               // the widest set of partials: the six moments
}

extern "C" int yt8m_batch_agreement_fwd(const float* p, const void* labels, int label_dtype, float* loss_out, float* stats,
                                        int64_t B, int64_t V, float eps, float agreement, float batch_size, void* workspace,
                                        yt8m_stream_t stream) {
  YT8M_LOSS_REQUIRE_SHAPE(B, V);
  YT8M_REQUIRE(p && labels && loss_out && stats && workspace, YT8M_E_BADARG, "null operand");
  YT8M_LOSS_REQUIRE_LABELS(label_dtype);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  float* part = static_cast<float*>(workspace);
  const int64_t G = wg_count(B, V);
  const dim3 grid((unsigned)((V + TILE - 1) / TILE), (unsigned)B);
  YT8M_LOSS_LAUNCH((ba_extrema_kernel<uint8_t>), (ba_extrema_kernel<float>), grid, s, p, labels, label_dtype, V, part, G);
  hipLaunchKernelGGL(ba_extrema_finish_kernel, dim3(1), dim3(1024), 0, s, part, G, stats);
  YT8M_LOSS_LAUNCH((ba_moments_kernel<uint8_t>), (ba_moments_kernel<float>), grid, s, p, labels, label_dtype, V, stats, part, G);
  hipLaunchKernelGGL(ba_moments_finish_kernel, dim3(1), dim3(1024), 0, s, part, G, eps, agreement, batch_size, stats);
  YT8M_LOSS_LAUNCH((ba_loss_kernel<uint8_t>), (ba_loss_kernel<float>), grid, s, p, labels, label_dtype, V, eps, stats, part, G);
  hipLaunchKernelGGL(ba_loss_finish_kernel, dim3(1), dim3(1024), 0, s, part, G, eps, 1.0f / (float)B, stats, loss_out);
  return launch_status("batch_agreement_fwd");
}

extern "C" int yt8m_batch_agreement_bwd(const float* p, const void* labels, int label_dtype, const float* stats,
                                        const float* upstream_dev, float* dp, int64_t B, int64_t V, float eps, float upstream,
                                        yt8m_stream_t stream) {
  YT8M_LOSS_REQUIRE_SHAPE(B, V);
  YT8M_REQUIRE(p && labels && stats && dp, YT8M_E_BADARG, "null operand");
  YT8M_LOSS_REQUIRE_LABELS(label_dtype);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)((V + TILE - 1) / TILE), (unsigned)B);
  YT8M_LOSS_LAUNCH((ba_bwd_kernel<uint8_t>), (ba_bwd_kernel<float>), grid, s, p, labels, label_dtype, V, eps, stats,
                   upstream / (float)B, upstream_dev, dp);
  return launch_status("ba_bwd_kernel");
}

extern "C" int yt8m_topk_batch_agreement_fwd(const float* p, const void* labels, int label_dtype, float* loss_out, float* stats,
                                             int64_t B, int64_t V, float eps, float agreement, void* workspace, yt8m_stream_t stream) {
  YT8M_LOSS_REQUIRE_SHAPE(B, V);
  YT8M_REQUIRE(V >= TOPK, YT8M_E_SHAPE, "V < 20: top_k(k = 20) needs 20 classes");
  YT8M_REQUIRE(p && labels && loss_out && stats && workspace, YT8M_E_BADARG, "null operand");
  YT8M_LOSS_REQUIRE_LABELS(label_dtype);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  float* part = static_cast<float*>(workspace);
  const int64_t G = wg_count(B, V);
  const dim3 grid((unsigned)((V + TILE - 1) / TILE), (unsigned)B);
  hipLaunchKernelGGL(tk_threshold_kernel, dim3((unsigned)B), dim3(256), 0, s, p, V, stats + 1);
  YT8M_LOSS_LAUNCH((tk_minpp_kernel<uint8_t>), (tk_minpp_kernel<float>), grid, s, p, labels, label_dtype, V, (const float*)stats, part);
  hipLaunchKernelGGL(tk_minpp_finish_kernel, dim3(1), dim3(1024), 0, s, part, G, stats);
  YT8M_LOSS_LAUNCH((tk_loss_kernel<uint8_t>), (tk_loss_kernel<float>), grid, s, p, labels, label_dtype, V, eps, agreement,
                   (const float*)stats, part, (float*)nullptr, 0.f, (const float*)nullptr);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(1024), 0, s, part, G, 1.0f / (float)B, loss_out);
  return launch_status("topk_batch_agreement_fwd");
}

extern "C" int yt8m_topk_batch_agreement_bwd(const float* p, const void* labels, int label_dtype, const float* stats,
                                             const float* upstream_dev, float* dp, int64_t B, int64_t V, float eps, float agreement,
                                             float upstream, yt8m_stream_t stream) {
  YT8M_LOSS_REQUIRE_SHAPE(B, V);
  YT8M_REQUIRE(V >= TOPK, YT8M_E_SHAPE, "V < 20: top_k(k = 20) needs 20 classes");
  YT8M_REQUIRE(p && labels && stats && dp, YT8M_E_BADARG, "null operand");
  YT8M_LOSS_REQUIRE_LABELS(label_dtype);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)((V + TILE - 1) / TILE), (unsigned)B);
  YT8M_LOSS_LAUNCH((tk_loss_kernel<uint8_t>), (tk_loss_kernel<float>), grid, s, p, labels, label_dtype, V, eps, agreement, stats,
                   (float*)nullptr, dp, upstream / (float)B, upstream_dev);
  return launch_status("tk_loss_kernel(bwd)");
}

extern "C" int64_t yt8m_pointwise_loss_workspace_bytes(int64_t B, int64_t V) {
  if (B <= 0 || V <= 0) return 0;
  return wg_count(B, V) * (int64_t)sizeof(float);
}

namespace {
int pointwise_launch(int kind, const float* p, const void* labels, int label_dtype, float c0, float c1, float eps, float* partial,
                     float* dp, float dscale, const float* up_dev, int64_t B, int64_t V, hipStream_t s) {
  const dim3 grid((unsigned)((V + TILE - 1) / TILE), (unsigned)B);
  switch (kind) {
    case YT8M_LOSS_WEIGHTED_XENT:
      YT8M_LOSS_LAUNCH((pointwise_loss_kernel<YT8M_LOSS_WEIGHTED_XENT, uint8_t>), (pointwise_loss_kernel<YT8M_LOSS_WEIGHTED_XENT, float>),
                       grid, s, p, labels, label_dtype, V, c0, c1, eps, partial, dp, dscale, up_dev);
      break;
    case YT8M_LOSS_MSE:
      YT8M_LOSS_LAUNCH((pointwise_loss_kernel<YT8M_LOSS_MSE, uint8_t>), (pointwise_loss_kernel<YT8M_LOSS_MSE, float>), grid, s, p,
                       labels, label_dtype, V, c0, c1, eps, partial, dp, dscale, up_dev);
      break;
    default:
      YT8M_LOSS_LAUNCH((pointwise_loss_kernel<YT8M_LOSS_HINGE, uint8_t>), (pointwise_loss_kernel<YT8M_LOSS_HINGE, float>), grid, s, p,
                       labels, label_dtype, V, c0, c1, eps, partial, dp, dscale, up_dev);
      break;
  }
  return launch_status("pointwise_loss_kernel");
}
}  // namespace

extern "C" int yt8m_pointwise_loss_fwd_bwd(int kind, const float* p, const void* labels, int label_dtype, float* loss_out, float* dp,
                                           int64_t B, int64_t V, float c0, float c1, float eps, float upstream, void* workspace,
                                           yt8m_stream_t stream) {
  YT8M_REQUIRE(kind == YT8M_LOSS_WEIGHTED_XENT || kind == YT8M_LOSS_MSE || kind == YT8M_LOSS_HINGE, YT8M_E_BADARG, "loss kind");
  YT8M_LOSS_REQUIRE_SHAPE(B, V);
  YT8M_REQUIRE(p && labels && loss_out && workspace, YT8M_E_BADARG, "null operand");
  YT8M_LOSS_REQUIRE_LABELS(label_dtype);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  float* partial = static_cast<float*>(workspace);
  const int rc = pointwise_launch(kind, p, labels, label_dtype, c0, c1, eps, partial, dp, upstream / (float)B, nullptr, B, V, s);
  if (rc != YT8M_OK) return rc;
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(1024), 0, s, partial, wg_count(B, V), 1.0f / (float)B, loss_out);
  return launch_status("loss_finish_kernel");
}

extern "C" int yt8m_pointwise_loss_bwd(int kind, const float* p, const void* labels, int label_dtype, const float* upstream_dev,
                                       float* dp, int64_t B, int64_t V, float c0, float c1, float eps, float upstream,
                                       yt8m_stream_t stream) {
  YT8M_REQUIRE(kind == YT8M_LOSS_WEIGHTED_XENT || kind == YT8M_LOSS_MSE || kind == YT8M_LOSS_HINGE, YT8M_E_BADARG, "loss kind");
  YT8M_LOSS_REQUIRE_SHAPE(B, V);
  YT8M_REQUIRE(p && labels && dp, YT8M_E_BADARG, "null operand");
  YT8M_LOSS_REQUIRE_LABELS(label_dtype);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  return pointwise_launch(kind, p, labels, label_dtype, c0, c1, eps, nullptr, dp, upstream / (float)B, upstream_dev, B, V, s);
}
