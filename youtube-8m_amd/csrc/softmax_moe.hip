// softmax_moe.hip -- the label-softmax mixture block of MoeSoftmaxModel (Z/video_level_models.py:877-960, the softmax part of sub_model)
// and Z's SoftmaxLoss (Z/losses.py:412-456), here SplitSoftmaxLoss (gfx950, wave64).
//
// The block, with S = vocab_size - softmax_bound + 1 labels (the last one stands for "none of the infrequent labels") and M mixtures:
//   Zg [rows, S (M + 1)] gate logits, column s (M + 1) + m;  Ze [rows, S M] expert logits, column s M + m;
//   g[s, :] = softmax over the M + 1 gates of label s;  e[:, m] = softmax OVER THE S LABELS of mixture m;
//   p[s] = sum_{m < M} g[s, m] e[s, m];  T = sum_s p[s];  q = p / T;  out[row] = [head[row] (V1 columns, copied) | q[0 .. S - 2]].
// One workgroup of 256 threads per row; thread t owns the labels t, t + 256, ..., so neighbouring lanes read neighbouring addresses
// (M or M + 1 floats each: single-element loads -- S (M + 1) is odd at the workload, 1717 * 5, so rows are not 16-byte aligned and no
// wide load is assumed).  fwd: column maxima, column sums, T -- three workgroup reductions -- then the write.  bwd: ONE reduction
// (D = sum dq q, A_m = sum e g dq, C_m = sum e g; 2 M + 1 values) and one writing pass:
//   dp_s = (dq_s - D) / T;  dZe[s, m] = e (g dp_s - (A_m - D C_m) / T), formed as (g e (dq_s - D) - e (A_m - D C_m)) / T;
//   dZg[s, m] = g dp_s (e [m < M] - p_s);  dq of the dropped label = 0.
// Reductions: per-thread sums in label order, the wave butterfly, the four waves' partials in the order 0..3: a fixed order, no atomics,
// reruns are bit-equal.  Every output element is written exactly once; bwd may write over the logits (each thread reads a label's
// logits before it writes that label's gradients, and the reduction's barrier lies between the last read of pass one and the first
// write).
//
// Register residency.  A thread keeps its labels between the reduction and the write -- fwd: exp(Ze - max) and p, M + 1 floats a label;
// bwd: g, e and dq, 2 M + 2 floats a label -- when it owns at most REG_LABELS(M) = 36 / (M + 1) labels (72 floats in bwd), that is for
//   S <= 256 * (36 / (M + 1)):  M = 1: 4608, 2: 3072, 3: 2304, 4: 1792 (S M <= 7168; the workload's S = 1717 is 7 labels, 70 floats),
//   5: 1536, 6: 1280, 7 and 8: 1024 (S M <= 8192).
// Above that each pass reads the row's logits again (34 KB + 27 KB at S = 1717: they hit L2, and L1 in part) and recomputes: the same
// expressions in the same order, so the two forms agree bit for bit where both apply.  yt8m_softmax_moe_supported: 2 <= S <= 65536,
// 1 <= M <= 8.
//
// -Rpass-analysis=kernel-resource-usage (ROCm 7, gfx950), VGPRs, no scratch in any instance:
//   softmax_moe_fwd_kernel<M, true>   M = 1 .. 8: 96, 72, 71, 69, 74, 78, 77, 91 (7 waves / SIMD at M = 4);   <M, false>: 32 .. 62
//   softmax_moe_bwd_kernel<M, true>   M = 1 .. 8: 140, 126, 126, 128, 124, 138, 140, 144 (3-4 waves / SIMD);  <M, false>: 27 .. 68
//   split_softmax_loss_kernel<LT>     30 for both label types;  split_softmax_loss_finish_kernel 17
//
// The loss, per row of p [B, V] read in place through a row pitch (p[b * ldp + c0 + v]) with V1 = bound:
//   sum_{v < V1} ce(p, y; 1e-5)  -  sum_{v >= V1} (n log(p + 1e-7) + (1 - n) log(1 - p + 1e-7))  -  (a log(o + 1e-7) + (1 - a) log(1 - o + 1e-7))
//   n = y / max(sum_{v >= V1} y, 1e-7),  a = 1 - max_{v >= V1} y,  o = max(1 - sum_{v >= V1} p, 0)  (the reference does not clamp: see
//   yt8m_hip.h), gradient of o as if unclamped.  n is linear in y, so ONE pass over the row gives the value: sum y log(p + e),
//   sum log(1 - p + e), sum y log(1 - p + e), sum y, max y, sum p and the cross entropy, reduced once (7 values).  The gradient needs the
//   row's three scalars first and reads the row a second time (19 KB at V = 4716: L1 / L2).  One workgroup per row leaves one partial;
//   a one-workgroup kernel sums them in fp64 in a fixed order, as csrc/losses.hip.  No host synchronisation.
#include <math.h>
#include "common.h"

using namespace yt8m;

namespace {

constexpr int MAX_M = 8;
constexpr int64_t MAX_S = 65536;
constexpr int reg_labels(int M) { return 36 / (M + 1); }

// N workgroup-wide maxima for blockDim.x == 256, as block_sums_256
template <int N>
__device__ __forceinline__ void block_maxes_256(float (&v)[N], float* red /* 4 N floats of LDS */) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_max(v[k]);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[w * N + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = fmaxf(fmaxf(red[k], red[N + k]), fmaxf(red[2 * N + k], red[3 * N + k]));
}

// f(i, s) for every label s of this thread; REG: slot i is a compile-time constant after unrolling (RL slots), else i = 0
template <bool REG, int RL, typename F>
__device__ __forceinline__ void for_labels(int S, F f) {
  if constexpr (REG) {
#pragma unroll
    for (int i = 0; i < RL; ++i) {
      const int s = (int)threadIdx.x + 256 * i;
      if (s < S) f(i, s);
    }
  } else {
    for (int s = (int)threadIdx.x; s < S; s += 256) f(0, s);
  }
}

// softmax over the M + 1 gate logits of one label
template <int M>
__device__ __forceinline__ void gate_softmax(const float* zg, float (&g)[M + 1]) {
  float mx = -INFINITY, sum = 0.f;
#pragma unroll
  for (int m = 0; m <= M; ++m) { g[m] = zg[m]; mx = fmaxf(mx, g[m]); }
#pragma unroll
  for (int m = 0; m <= M; ++m) { g[m] = expf(g[m] - mx); sum += g[m]; }
  const float r = 1.0f / sum;
#pragma unroll
  for (int m = 0; m <= M; ++m) g[m] *= r;
}

template <int M>
__device__ __forceinline__ float mix(const float (&g)[M + 1], const float (&e)[M]) {
  float p = 0.f;
#pragma unroll
  for (int m = 0; m < M; ++m) p += g[m] * e[m];
  return p;
}

// stats [rows, 2 M + 1]: the M column maxima, the M column sums of exp(Ze - max), T
template <int M, bool REG>
__global__ __launch_bounds__(256) void softmax_moe_fwd_kernel(const float* __restrict__ Zg, const float* __restrict__ Ze,
                                                              const float* __restrict__ head, float* __restrict__ out,
                                                              float* __restrict__ stats, int S, int V1) {
  constexpr int RL = REG ? reg_labels(M) : 1;
  __shared__ float red[4 * M];
  const int64_t row = blockIdx.x;
  const float* zg = Zg + row * ((int64_t)S * (M + 1));
  const float* ze = Ze + row * ((int64_t)S * M);
  float* o = out + row * ((int64_t)V1 + S - 1);
  if (head) {
    const float* h = head + row * (int64_t)V1;
    for (int c = threadIdx.x; c < V1; c += 256) o[c] = h[c];
  }
  float ex[RL][M], pv[RL];
  float mx[M], sum[M], inv[M];
#pragma unroll
  for (int m = 0; m < M; ++m) { mx[m] = -INFINITY; sum[m] = 0.f; }
  for_labels<REG, RL>(S, [&](int i, int s) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float v = ze[(int64_t)s * M + m];
      mx[m] = fmaxf(mx[m], v);
      if (REG) ex[i][m] = v;
    }
  });
  block_maxes_256<M>(mx, red);
  for_labels<REG, RL>(S, [&](int i, int s) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float x = expf((REG ? ex[i][m] : ze[(int64_t)s * M + m]) - mx[m]);
      sum[m] += x;
      if (REG) ex[i][m] = x;
    }
  });
  float keep[M];
#pragma unroll
  for (int m = 0; m < M; ++m) keep[m] = sum[m];
  block_sums_256<M>(keep, red);
#pragma unroll
  for (int m = 0; m < M; ++m) { sum[m] = keep[m]; inv[m] = 1.0f / sum[m]; }
  // p of one label: the same expressions wherever it is formed
  auto label_p = [&](int i, int s) {
    float g[M + 1], e[M];
    gate_softmax<M>(zg + (int64_t)s * (M + 1), g);
#pragma unroll
    for (int m = 0; m < M; ++m) e[m] = (REG ? ex[i][m] : expf(ze[(int64_t)s * M + m] - mx[m])) * inv[m];
    return mix<M>(g, e);
  };
  float T = 0.f;
  for_labels<REG, RL>(S, [&](int i, int s) {
    const float p = label_p(i, s);
    T += p;
    if (REG) pv[i] = p;
  });
  T = block_sum_256(T, red);
  for_labels<REG, RL>(S, [&](int i, int s) {
    if (s < S - 1) o[V1 + s] = (REG ? pv[i] : label_p(i, s)) / T;
  });
  if (threadIdx.x == 0) {
    float* st = stats + row * (2 * M + 1);
#pragma unroll
    for (int m = 0; m < M; ++m) { st[m] = mx[m]; st[M + m] = sum[m]; }
    st[2 * M] = T;
  }
}

// dout: dq of label s < S - 1 at dout[row * ldd + c0 + s].  dZg / dZe may be Zg / Ze themselves (no __restrict__ on the four).
template <int M, bool REG>
__global__ __launch_bounds__(256) void softmax_moe_bwd_kernel(const float* Zg, const float* Ze, const float* __restrict__ stats,
                                                              const float* __restrict__ dout, int64_t ldd, int64_t c0, float* dZg,
                                                              float* dZe, int S) {
  constexpr int RL = REG ? reg_labels(M) : 1;
  constexpr int NQ = 2 * M + 1;
  __shared__ float red[4 * NQ];
  const int64_t row = blockIdx.x;
  const float* zg = Zg + row * ((int64_t)S * (M + 1));
  const float* ze = Ze + row * ((int64_t)S * M);
  const float* dq = dout + row * ldd + c0;
  float* dzg = dZg + row * ((int64_t)S * (M + 1));
  float* dze = dZe + row * ((int64_t)S * M);
  const float* st = stats + row * NQ;
  float mx[M], inv[M];
#pragma unroll
  for (int m = 0; m < M; ++m) { mx[m] = st[m]; inv[m] = 1.0f / st[M + m]; }
  const float T = st[2 * M];
  float gv[RL][M + 1], ev[RL][M], qv[RL];
  auto label = [&](int s, float (&g)[M + 1], float (&e)[M]) {
    gate_softmax<M>(zg + (int64_t)s * (M + 1), g);
#pragma unroll
    for (int m = 0; m < M; ++m) e[m] = expf(ze[(int64_t)s * M + m] - mx[m]) * inv[m];
    return s < S - 1 ? dq[s] : 0.f;
  };
  float acc[NQ];                                                         // D, A_m, C_m
#pragma unroll
  for (int k = 0; k < NQ; ++k) acc[k] = 0.f;
  for_labels<REG, RL>(S, [&](int i, int s) {
    float g[M + 1], e[M];
    const float d = label(s, g, e);
    acc[0] += d * (mix<M>(g, e) / T);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float w = g[m] * e[m];
      acc[1 + m] = fmaf(w, d, acc[1 + m]);
      acc[1 + M + m] += w;
    }
    if (REG) {
      qv[i] = d;
#pragma unroll
      for (int m = 0; m < M; ++m) { gv[i][m] = g[m]; ev[i][m] = e[m]; }
      gv[i][M] = g[M];
    }
  });
  block_sums_256<NQ>(acc, red);
  const float D = acc[0], invT = 1.0f / T;
  // dZe = (w (dq - D) - e (A_m - D C_m)) / T with both differences formed by the SAME operations, fma(-D, c, a) on a = the rounded
  // w dq (A_m is a sum of such terms) and c = w: where one label holds a mixture's whole mass (e = 1, A_m = w dq, C_m = w) the two cancel
  // to an exact 0, as they do in the softmax's own backward form dy - sum(e dy); formed as g dp - K_m they leave an ulp of g dq / T
  float K[M];
#pragma unroll
  for (int m = 0; m < M; ++m) K[m] = fmaf(-D, acc[1 + M + m], acc[1 + m]);
  for_labels<REG, RL>(S, [&](int i, int s) {
    float g[M + 1], e[M], d;
    if (REG) {
      d = qv[i];
#pragma unroll
      for (int m = 0; m < M; ++m) { g[m] = gv[i][m]; e[m] = ev[i][m]; }
      g[M] = gv[i][M];
    } else {
      d = label(s, g, e);
    }
    const float dp = (d - D) * invT, p = mix<M>(g, e);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float w = g[m] * e[m];
      dze[(int64_t)s * M + m] = fmaf(-e[m], K[m], fmaf(-D, w, __fmul_rn(w, d))) * invT;
      dzg[(int64_t)s * (M + 1) + m] = (g[m] * dp) * (e[m] - p);
    }
    dzg[(int64_t)s * (M + 1) + M] = (g[M] * dp) * (0.f - p);
  });
}

template <int M>
void launch_fwd(bool reg, dim3 grid, hipStream_t s, const float* Zg, const float* Ze, const float* head, float* out, float* stats, int S,
                int V1) {
  if (reg) hipLaunchKernelGGL((softmax_moe_fwd_kernel<M, true>), grid, dim3(256), 0, s, Zg, Ze, head, out, stats, S, V1);
  else hipLaunchKernelGGL((softmax_moe_fwd_kernel<M, false>), grid, dim3(256), 0, s, Zg, Ze, head, out, stats, S, V1);
}

template <int M>
void launch_bwd(bool reg, dim3 grid, hipStream_t s, const float* Zg, const float* Ze, const float* stats, const float* dout, int64_t ldd,
                int64_t c0, float* dZg, float* dZe, int S) {
  if (reg) hipLaunchKernelGGL((softmax_moe_bwd_kernel<M, true>), grid, dim3(256), 0, s, Zg, Ze, stats, dout, ldd, c0, dZg, dZe, S);
  else hipLaunchKernelGGL((softmax_moe_bwd_kernel<M, false>), grid, dim3(256), 0, s, Zg, Ze, stats, dout, ldd, c0, dZg, dZe, S);
}

#define YT8M_SOFTMAX_MOE_DISPATCH(M, fn, ...) \
  switch (M) {                                \
    case 1: fn<1>(__VA_ARGS__); break;        \
    case 2: fn<2>(__VA_ARGS__); break;        \
    case 3: fn<3>(__VA_ARGS__); break;        \
    case 4: fn<4>(__VA_ARGS__); break;        \
    case 5: fn<5>(__VA_ARGS__); break;        \
    case 6: fn<6>(__VA_ARGS__); break;        \
    case 7: fn<7>(__VA_ARGS__); break;        \
    default: fn<8>(__VA_ARGS__); break;       \
  }

inline bool resident(int64_t S, int64_t M) { return S <= 256 * (int64_t)reg_labels((int)M); }

// ------------------------------------------------------------------------------------------------
// SplitSoftmaxLoss.  The value (partial != NULL) and / or the gradient (dp != NULL, [B, V] contiguous).
__device__ __forceinline__ float log_term(float y, float p, float eps) { return y * logf(p + eps) + (1.0f - y) * logf(1.0f - p + eps); }
__device__ __forceinline__ float log_grad(float y, float p, float eps) { return y / (p + eps) - (1.0f - y) / (1.0f - p + eps); }

template <typename LT>
__global__ __launch_bounds__(256) void split_softmax_loss_kernel(const float* __restrict__ p, int64_t ldp, int64_t c0,
                                                                 const LT* __restrict__ y, int V, int V1, float eps_ce, float eps_sm,
                                                                 float* __restrict__ partial, float* __restrict__ dp, float dscale,
                                                                 const float* __restrict__ up_dev) {
  __shared__ float red[4 * 6];
  const int64_t row = blockIdx.x;
  const float* pr = p + row * ldp + c0;
  const LT* yr = y + row * (int64_t)V;
  // ce, sum y log(p + e), sum log(1 - p + e), sum y log(1 - p + e), sum y, sum p; and max y
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ymax[1] = {-INFINITY};
  for (int c = threadIdx.x; c < V; c += 256) {
    const float pv = pr[c], yv = (float)yr[c];
    if (c < V1) {
      if (partial) v[0] -= log_term(yv, pv, eps_ce);
    } else {
      if (partial) {
        const float l1 = logf(1.0f - pv + eps_sm);
        v[1] += yv * logf(pv + eps_sm);
        v[2] += l1;
        v[3] += yv * l1;
      }
      v[4] += yv;
      v[5] += pv;
      ymax[0] = fmaxf(ymax[0], yv);
    }
  }
  block_sums_256<6>(v, red);
  block_maxes_256<1>(ymax, red);
  const float rys = 1.0f / fmaxf(v[4], eps_sm);                           // n = y / max(sum y, eps)
  const float a = 1.0f - ymax[0], o = fmaxf(1.0f - v[5], 0.f);            // the appended label and probability
  if (partial && threadIdx.x == 0) partial[row] = v[0] - ((v[1] - v[3]) * rys + v[2]) - log_term(a, o, eps_sm);
  if (dp) {
    if (up_dev) dscale *= up_dev[0];
    const float ga = log_grad(a, o, eps_sm);                              // d o / d p = -1 for every p of the softmax part
    float* dr = dp + row * (int64_t)V;
    for (int c = threadIdx.x; c < V; c += 256) {
      const float pv = pr[c], yv = (float)yr[c];
      dr[c] = (c < V1 ? -log_grad(yv, pv, eps_ce) : ga - log_grad(yv * rys, pv, eps_sm)) * dscale;
    }
  }
}

// one workgroup of 1024 threads: loss = (sum of the partials, fp64, fixed order) / rows
__global__ __launch_bounds__(1024) void split_softmax_loss_finish_kernel(const float* __restrict__ part, int64_t n, float inv_rows,
                                                                         float* __restrict__ loss_out) {
  __shared__ double red[16];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) s += (double)part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += red[k];
    loss_out[0] = (float)(t * (double)inv_rows);
  }
}

void loss_launch(const float* p, int64_t ldp, int64_t c0, const void* labels, int dt, int64_t B, int64_t V, int64_t V1, float eps_ce,
                 float eps_sm, float* partial, float* dp, float dscale, const float* up_dev, hipStream_t s) {
  const dim3 grid((unsigned)B), block(256);
  if (dt == YT8M_LABEL_U8)
    hipLaunchKernelGGL(split_softmax_loss_kernel<uint8_t>, grid, block, 0, s, p, ldp, c0, static_cast<const uint8_t*>(labels), (int)V, (int)V1,
                       eps_ce, eps_sm, partial, dp, dscale, up_dev);
  else
    hipLaunchKernelGGL(split_softmax_loss_kernel<float>, grid, block, 0, s, p, ldp, c0, static_cast<const float*>(labels), (int)V, (int)V1,
                       eps_ce, eps_sm, partial, dp, dscale, up_dev);
}

#define YT8M_SPLIT_LOSS_REQUIRE(B, V, V1, ldp, c0, dt)                                                                                 \
  YT8M_REQUIRE((B) > 0 && (B) <= 0x7fffffffLL, YT8M_E_SHAPE, "split_softmax_loss: empty batch (or more than 2^31 - 1 rows)");          \
  YT8M_REQUIRE((V) >= 2 && (V) <= 0x7fffffffLL && (V1) > 0 && (V1) < (V), YT8M_E_SHAPE, "split_softmax_loss: 0 < bound < V < 2^31");   \
  YT8M_REQUIRE((c0) >= 0 && (ldp) >= (c0) + (V), YT8M_E_BADARG, "split_softmax_loss: 0 <= c0 and c0 + V <= ldp");                      \
  YT8M_REQUIRE((dt) == YT8M_LABEL_U8 || (dt) == YT8M_LABEL_F32, YT8M_E_BADARG, "split_softmax_loss: label dtype")

}  // namespace

extern "C" int yt8m_softmax_moe_supported(int64_t S, int64_t M) { return S >= 2 && S <= MAX_S && M >= 1 && M <= MAX_M; }

extern "C" int yt8m_softmax_moe_resident(int64_t S, int64_t M) { return yt8m_softmax_moe_supported(S, M) && resident(S, M); }

extern "C" int yt8m_softmax_moe_fwd(const float* Zg, const float* Ze, const float* head, float* out, float* stats, int64_t rows, int64_t S,
                                    int64_t M, int64_t V1, yt8m_stream_t stream) {
  YT8M_REQUIRE(rows > 0 && rows <= 0x7fffffffLL, YT8M_E_SHAPE, "softmax_moe: rows must be positive (at most 2^31 - 1)");
  YT8M_REQUIRE(yt8m_softmax_moe_supported(S, M), YT8M_E_SHAPE, "softmax_moe: 2 <= S <= 65536 and 1 <= M <= 8");
  YT8M_REQUIRE(V1 >= 0 && V1 <= (1 << 24), YT8M_E_SHAPE, "softmax_moe: 0 <= V1 <= 2^24");
  YT8M_REQUIRE(Zg && Ze && out && stats, YT8M_E_BADARG, "softmax_moe: null operand (only head may be null)");
  YT8M_REQUIRE((V1 == 0) == (head == nullptr), YT8M_E_BADARG, "softmax_moe: head is given exactly when V1 > 0");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)rows);
  YT8M_SOFTMAX_MOE_DISPATCH(M, launch_fwd, resident(S, M), grid, s, Zg, Ze, head, out, stats, (int)S, (int)V1);
  return launch_status("softmax_moe_fwd_kernel");
}

extern "C" int yt8m_softmax_moe_bwd(const float* Zg, const float* Ze, const float* stats, const float* dout, int64_t ldd, int64_t c0,
                                    float* dZg, float* dZe, int64_t rows, int64_t S, int64_t M, yt8m_stream_t stream) {
  YT8M_REQUIRE(rows > 0 && rows <= 0x7fffffffLL, YT8M_E_SHAPE, "softmax_moe: rows must be positive (at most 2^31 - 1)");
  YT8M_REQUIRE(yt8m_softmax_moe_supported(S, M), YT8M_E_SHAPE, "softmax_moe: 2 <= S <= 65536 and 1 <= M <= 8");
  YT8M_REQUIRE(Zg && Ze && stats && dout && dZg && dZe, YT8M_E_BADARG, "softmax_moe: null operand");
  YT8M_REQUIRE(c0 >= 0 && ldd >= c0 + S - 1, YT8M_E_BADARG, "softmax_moe: 0 <= c0 and c0 + S - 1 <= ldd");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)rows);
  YT8M_SOFTMAX_MOE_DISPATCH(M, launch_bwd, resident(S, M), grid, s, Zg, Ze, stats, dout, ldd, c0, dZg, dZe, (int)S);
  return launch_status("softmax_moe_bwd_kernel");
}

extern "C" int64_t yt8m_split_softmax_loss_workspace_bytes(int64_t B) { return B > 0 ? B * (int64_t)sizeof(float) : 0; }

extern "C" int yt8m_split_softmax_loss_fwd_bwd(const float* p, int64_t ldp, int64_t c0, const void* labels, int label_dtype, float* loss_out,
                                               float* dp, int64_t B, int64_t V, int64_t bound, float eps_ce, float eps_sm, float upstream,
                                               void* workspace, yt8m_stream_t stream) {
  YT8M_SPLIT_LOSS_REQUIRE(B, V, bound, ldp, c0, label_dtype);
  YT8M_REQUIRE(p && labels && loss_out && workspace, YT8M_E_BADARG, "split_softmax_loss: null operand (only dp may be null)");
  YT8M_REQUIRE(eps_ce > 0.f && eps_sm > 0.f, YT8M_E_BADARG, "split_softmax_loss: both eps must be > 0");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  float* partial = static_cast<float*>(workspace);
  loss_launch(p, ldp, c0, labels, label_dtype, B, V, bound, eps_ce, eps_sm, partial, dp, upstream / (float)B, nullptr, s);
  hipLaunchKernelGGL(split_softmax_loss_finish_kernel, dim3(1), dim3(1024), 0, s, partial, B, 1.0f / (float)B, loss_out);
  return launch_status("split_softmax_loss_kernel");
}

extern "C" int yt8m_split_softmax_loss_bwd(const float* p, int64_t ldp, int64_t c0, const void* labels, int label_dtype,
                                           const float* upstream_dev, float* dp, int64_t B, int64_t V, int64_t bound, float eps_ce,
                                           float eps_sm, float upstream, yt8m_stream_t stream) {
  YT8M_SPLIT_LOSS_REQUIRE(B, V, bound, ldp, c0, label_dtype);
  YT8M_REQUIRE(p && labels && dp, YT8M_E_BADARG, "split_softmax_loss: null operand");
  YT8M_REQUIRE(eps_ce > 0.f && eps_sm > 0.f, YT8M_E_BADARG, "split_softmax_loss: both eps must be > 0");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  loss_launch(p, ldp, c0, labels, label_dtype, B, V, bound, eps_ce, eps_sm, nullptr, dp, upstream / (float)B, upstream_dev, s);
  return launch_status("split_softmax_loss_kernel(bwd)");
}
