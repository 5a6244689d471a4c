// multiscale.hip -- what joins a CNN to its LSTM and to the next, half-as-long scale in MultiscaleCnnLstmModel
// (W/all_frame_models/multiscale_cnn_lstm_model.py:38-45,114-131): slim.batch_norm over ALL F B rows, ReLU, and the max over frame
// pairs, on TIME-major rows (row t B + b) so that the CNN's output, the LSTM's input and the next scale's input never change layout.
//
//   yt8m_colmoments_f32          column mean / rstd of y [F B, C] (+ moving averages), or the moving statistics when not training
//   yt8m_bn_relu_pool2_tm_fwd    ONE pass over y: a = relu(bn(y)) [F,B,C] and p[j] = max(a[2j], a[2j+1]) [F/2,B,C]
//   yt8m_bn_relu_pool2_tm_bwd    two passes: column sums of da and da xhat (-> dgamma, dbeta), then dy
//
// Streaming kernels: every thread owns four columns (16-byte loads and stores) and walks rows; a workgroup is 64 column lanes (1 KiB
// of a row) x 4 row lanes.  Column reductions are per-workgroup partials in a workspace plus a finishing pass that adds them in a
// fixed order (in double: 256 terms per column cost nothing and leave the fp32 partials' rounding as the only error) -- no float
// atomics, results do not depend on scheduling.
//
// Tie rule of the pair maximum: tf.reduce_max splits the gradient between equal maxima, here the FIRST frame of the pair takes it.
// The two values of a pair are ReLU outputs: they are equal at 0, where the ReLU passes no gradient in TF and here, or on a set of
// measure zero -- the same function.
#include "common.h"

namespace yt8m {
namespace {

constexpr int MS_CL = 64;            // column lanes (float4 each) per workgroup
constexpr int MS_RL = 4;             // row lanes per workgroup
constexpr int MS_RED_BLOCKS = 256;   // row blocks of the reducing kernels (partials per column)
constexpr int MS_MAP_BLOCKS = 512;   // row blocks of the kernels that only map

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// sums over the 4 row lanes in a fixed order; valid on row lane 0
__device__ __forceinline__ float4 rowlane_sum(float4 v, float4 (*red)[MS_CL], int rl, int cl) {
  __syncthreads();
  red[rl][cl] = v;
  __syncthreads();
  return add4(add4(red[0][cl], red[1][cl]), add4(red[2][cl], red[3][cl]));
}

// partial[blockIdx.y][c] = sum over the block's rows of y[r][c] (CENTRED: of (y[r][c] - mean[c])^2)
template <bool CENTRED>
__global__ __launch_bounds__(256) void ms_colpartial_kernel(const float* __restrict__ y, int M, int C, long long ldy,
                                                            const float* __restrict__ mean, int rows_per_block,
                                                            float* __restrict__ partial) {
  __shared__ float4 red[MS_RL][MS_CL];
  const int cl = threadIdx.x & (MS_CL - 1), rl = threadIdx.x / MS_CL;
  const int c = (blockIdx.x * MS_CL + cl) * 4;
  const bool ok = c < C;
  float4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) {
    const float4 mu = CENTRED ? ld4(mean + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(r0 + rows_per_block, M);
    const float* p = y + c;
    auto term = [&](float4 v, float4& a) {
      if (CENTRED) {
        v.x -= mu.x; v.y -= mu.y; v.z -= mu.z; v.w -= mu.w;
        a.x += v.x * v.x; a.y += v.y * v.y; a.z += v.z * v.z; a.w += v.w * v.w;
      } else {
        a = add4(a, v);
      }
    };
    int r = r0 + rl;
    for (; r + 3 * MS_RL < r1; r += 4 * MS_RL) {                    // four rows in flight per thread
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ld4(p + (long long)(r + u * MS_RL) * ldy);
#pragma unroll
      for (int u = 0; u < 4; ++u) term(v[u], acc[u]);
    }
    for (; r < r1; r += MS_RL) term(ld4(p + (long long)r * ldy), acc[0]);
  }
  const float4 s = rowlane_sum(add4(add4(acc[0], acc[1]), add4(acc[2], acc[3])), red, rl, cl);
  if (rl == 0 && ok) st4(partial + (long long)blockIdx.y * C + c, s);
}

__device__ __forceinline__ double partial_total(const float* __restrict__ partial, int nblocks, int C, int c) {
  double s = 0.0;
  for (int i = 0; i < nblocks; ++i) s += (double)partial[(long long)i * C + c];
  return s;
}

__global__ __launch_bounds__(256) void ms_mean_finish_kernel(const float* __restrict__ partial, int nblocks, int C, int M,
                                                             float* __restrict__ mean) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) mean[c] = (float)(partial_total(partial, nblocks, C, c) / (double)M);
}

// biased variance (tf.nn.moments), rstd and the moving averages: yt8m_batchnorm_fwd's arithmetic (csrc/dbof.hip bn_stats_kernel)
__global__ __launch_bounds__(256) void ms_var_finish_kernel(const float* __restrict__ partial, int nblocks, int C, int M, float eps,
                                                            float decay, const float* __restrict__ mean, float* __restrict__ rstd,
                                                            float* __restrict__ moving_mean, float* __restrict__ moving_var) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float var = (float)(partial_total(partial, nblocks, C, c) / (double)M);
  rstd[c] = 1.0f / sqrtf(var + eps);
  moving_mean[c] = decay * moving_mean[c] + (1.0f - decay) * mean[c];
  moving_var[c] = decay * moving_var[c] + (1.0f - decay) * var;
}

__global__ __launch_bounds__(256) void ms_frozen_stats_kernel(const float* __restrict__ moving_mean, const float* __restrict__ moving_var,
                                                              int C, float eps, float* __restrict__ mean, float* __restrict__ rstd) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  mean[c] = moving_mean[c];
  rstd[c] = 1.0f / sqrtf(moving_var[c] + eps);
}

// bn_apply_kernel's expression (csrc/dbof.hip), then the ReLU
__device__ __forceinline__ float bn_relu(float v, float mu, float rs, float ga, float be) {
  return fmaxf((v - mu) * rs * ga + be, 0.f);
}
__device__ __forceinline__ float4 bn_relu4(const float4& v, const float4& mu, const float4& rs, const float4& ga, const float4& be) {
  return make_float4(bn_relu(v.x, mu.x, rs.x, ga.x, be.x), bn_relu(v.y, mu.y, rs.y, ga.y, be.y), bn_relu(v.z, mu.z, rs.z, ga.z, be.z),
                     bn_relu(v.w, mu.w, rs.w, ga.w, be.w));
}

// "pair row" r = j B + b stands for the rows (2j) B + b and (2j + 1) B + b of y: a workgroup owns both frames of a pair for its
// columns.  The last frame of an odd F has no partner (has1 false) and is not pooled.
__global__ __launch_bounds__(256) void ms_bn_relu_pool2_fwd_kernel(const float* __restrict__ y, long long ldy, int F, int B, int C,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float* __restrict__ a, long long lda, float* __restrict__ pooled,
                                                                   long long ldp, int rows_per_block) {
  const int cl = threadIdx.x & (MS_CL - 1), rl = threadIdx.x / MS_CL;
  const int c = (blockIdx.x * MS_CL + cl) * 4;
  if (c >= C) return;
  const float4 mu = ld4(mean + c), rs = ld4(rstd + c), ga = ld4(gamma + c), be = ld4(beta + c);
  const int NP = ((F + 1) / 2) * B;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(r0 + rows_per_block, NP);
#pragma unroll 2
  for (int r = r0 + rl; r < r1; r += MS_RL) {
    const int j = r / B;
    const long long row0 = (long long)r + (long long)j * B;       // (2j) B + b
    const bool has1 = 2 * j + 1 < F;
    const float4 v0 = ld4(y + row0 * ldy + c);
    float4 v1 = v0;
    if (has1) v1 = ld4(y + (row0 + B) * ldy + c);
    const float4 a0 = bn_relu4(v0, mu, rs, ga, be);
    st4(a + row0 * lda + c, a0);
    if (has1) {
      const float4 a1 = bn_relu4(v1, mu, rs, ga, be);
      st4(a + (row0 + B) * lda + c, a1);
      if (pooled) st4(pooled + (long long)r * ldp + c, make_float4(fmaxf(a0.x, a1.x), fmaxf(a0.y, a1.y), fmaxf(a0.z, a1.z), fmaxf(a0.w, a1.w)));
    }
  }
}

// gradient at the BN output for the two frames of a pair, a and xhat recomputed from y: the pooled gradient goes to the frame that
// attained the maximum (the first one on a tie), then the ReLU mask a > 0
__device__ __forceinline__ void pair_grad(float y0, float y1, float d0, float d1, float dp, float mu, float rs, float ga, float be,
                                          float& g0, float& g1, float& x0, float& x1) {
  x0 = (y0 - mu) * rs;
  x1 = (y1 - mu) * rs;
  const float v0 = x0 * ga + be, v1 = x1 * ga + be;
  const bool first = fmaxf(v0, 0.f) >= fmaxf(v1, 0.f);
  g0 = v0 > 0.f ? d0 + (first ? dp : 0.f) : 0.f;
  g1 = v1 > 0.f ? d1 + (first ? 0.f : dp) : 0.f;
}

struct PairGrad {
  float4 g0, g1, x0, x1;
};

__device__ __forceinline__ PairGrad load_pair_grad(const float* __restrict__ y, long long ldy, const float* da, long long ldda,
                                                   const float* __restrict__ dp, long long lddp, int r, long long row0, int B, bool has1,
                                                   int c, const float4& mu, const float4& rs, const float4& ga, const float4& be) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 y0 = ld4(y + row0 * ldy + c);
  const float4 d0 = da ? ld4(da + row0 * ldda + c) : z;
  float4 y1 = mu, d1 = z, p = z;
  if (has1) {
    y1 = ld4(y + (row0 + B) * ldy + c);
    if (da) d1 = ld4(da + (row0 + B) * ldda + c);
    if (dp) p = ld4(dp + (long long)r * lddp + c);
  }
  PairGrad o;
  pair_grad(y0.x, y1.x, d0.x, d1.x, p.x, mu.x, rs.x, ga.x, be.x, o.g0.x, o.g1.x, o.x0.x, o.x1.x);
  pair_grad(y0.y, y1.y, d0.y, d1.y, p.y, mu.y, rs.y, ga.y, be.y, o.g0.y, o.g1.y, o.x0.y, o.x1.y);
  pair_grad(y0.z, y1.z, d0.z, d1.z, p.z, mu.z, rs.z, ga.z, be.z, o.g0.z, o.g1.z, o.x0.z, o.x1.z);
  pair_grad(y0.w, y1.w, d0.w, d1.w, p.w, mu.w, rs.w, ga.w, be.w, o.g0.w, o.g1.w, o.x0.w, o.x1.w);
  if (!has1) o.g1 = z;
  return o;
}

// pass 1: partial[0][block][c] = sum g, partial[1][block][c] = sum g xhat over the block's pair rows
__global__ __launch_bounds__(256) void ms_bwd_reduce_kernel(const float* __restrict__ y, long long ldy, int F, int B, int C,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* da, long long ldda, const float* __restrict__ dp, long long lddp,
                                                            int rows_per_block, float* __restrict__ partial) {
  __shared__ float4 red[MS_RL][MS_CL];
  const int cl = threadIdx.x & (MS_CL - 1), rl = threadIdx.x / MS_CL;
  const int c = (blockIdx.x * MS_CL + cl) * 4;
  const bool ok = c < C;
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
  if (ok) {
    const float4 mu = ld4(mean + c), rs = ld4(rstd + c), ga = ld4(gamma + c), be = ld4(beta + c);
    const int NP = ((F + 1) / 2) * B;
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(r0 + rows_per_block, NP);
#pragma unroll 2
    for (int r = r0 + rl; r < r1; r += MS_RL) {
      const int j = r / B;
      const long long row0 = (long long)r + (long long)j * B;
      const PairGrad q = load_pair_grad(y, ldy, da, ldda, dp, lddp, r, row0, B, 2 * j + 1 < F, c, mu, rs, ga, be);
      s1.x += q.g0.x + q.g1.x; s1.y += q.g0.y + q.g1.y; s1.z += q.g0.z + q.g1.z; s1.w += q.g0.w + q.g1.w;
      s2.x += q.g0.x * q.x0.x + q.g1.x * q.x1.x; s2.y += q.g0.y * q.x0.y + q.g1.y * q.x1.y;
      s2.z += q.g0.z * q.x0.z + q.g1.z * q.x1.z; s2.w += q.g0.w * q.x0.w + q.g1.w * q.x1.w;
    }
  }
  const float4 t1 = rowlane_sum(s1, red, rl, cl);
  const float4 t2 = rowlane_sum(s2, red, rl, cl);
  if (rl == 0 && ok) {
    st4(partial + (long long)blockIdx.y * C + c, t1);
    st4(partial + ((long long)gridDim.y + blockIdx.y) * C + c, t2);
  }
}

// column sums from the partials; dgamma / dbeta with the accumulate convention of yt8m_batchnorm_bwd (beta_* = 0 overwrites)
__global__ __launch_bounds__(256) void ms_bwd_finish_kernel(const float* __restrict__ partial, int nblocks, int C, float* __restrict__ sums,
                                                            float* __restrict__ dgamma, float bg, float* __restrict__ dbeta, float bb) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float s1 = (float)partial_total(partial, nblocks, C, c);
  const float s2 = (float)partial_total(partial + (long long)nblocks * C, nblocks, C, c);
  sums[c] = s1;
  sums[C + c] = s2;
  if (dgamma) dgamma[c] = (bg != 0.f ? dgamma[c] : 0.f) + s2;
  if (dbeta) dbeta[c] = (bb != 0.f ? dbeta[c] : 0.f) + s1;
}

// pass 2: training: dy = gamma rstd (g - sum(g) / M - xhat sum(g xhat) / M); frozen statistics: dy = gamma rstd g.  dy may be da.
__global__ __launch_bounds__(256) void ms_bwd_apply_kernel(const float* __restrict__ y, long long ldy, int F, int B, int C,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* da, long long ldda, const float* __restrict__ dp, long long lddp,
                                                           const float* __restrict__ sums, int training, float* dy, long long lddy,
                                                           int rows_per_block) {
  const int cl = threadIdx.x & (MS_CL - 1), rl = threadIdx.x / MS_CL;
  const int c = (blockIdx.x * MS_CL + cl) * 4;
  if (c >= C) return;
  const float4 mu = ld4(mean + c), rs = ld4(rstd + c), ga = ld4(gamma + c), be = ld4(beta + c);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float invM = 1.0f / ((float)F * (float)B);
  float4 m1 = z, m2 = z;
  if (training) {
    m1 = ld4(sums + c);
    m2 = ld4(sums + C + c);
    m1.x *= invM; m1.y *= invM; m1.z *= invM; m1.w *= invM;
    m2.x *= invM; m2.y *= invM; m2.z *= invM; m2.w *= invM;
  }
  const float4 k = make_float4(ga.x * rs.x, ga.y * rs.y, ga.z * rs.z, ga.w * rs.w);
  const int NP = ((F + 1) / 2) * B;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(r0 + rows_per_block, NP);
#pragma unroll 2
  for (int r = r0 + rl; r < r1; r += MS_RL) {
    const int j = r / B;
    const long long row0 = (long long)r + (long long)j * B;
    const bool has1 = 2 * j + 1 < F;
    const PairGrad q = load_pair_grad(y, ldy, da, ldda, dp, lddp, r, row0, B, has1, c, mu, rs, ga, be);
    st4(dy + row0 * lddy + c, make_float4(k.x * (q.g0.x - m1.x - q.x0.x * m2.x), k.y * (q.g0.y - m1.y - q.x0.y * m2.y),
                                          k.z * (q.g0.z - m1.z - q.x0.z * m2.z), k.w * (q.g0.w - m1.w - q.x0.w * m2.w)));
    if (has1)
      st4(dy + (row0 + B) * lddy + c, make_float4(k.x * (q.g1.x - m1.x - q.x1.x * m2.x), k.y * (q.g1.y - m1.y - q.x1.y * m2.y),
                                                  k.z * (q.g1.z - m1.z - q.x1.z * m2.z), k.w * (q.g1.w - m1.w - q.x1.w * m2.w)));
  }
}


// rows per block so that at most max_blocks blocks cover `rows`; every row lane gets a few rows
inline int rows_per_block(int64_t rows, int max_blocks) {
  int64_t rpb = (rows + max_blocks - 1) / max_blocks;
  if (rpb < 4 * MS_RL) rpb = 4 * MS_RL;
  return (int)rpb;
}

inline unsigned col_groups(int64_t C) { return (unsigned)((C / 4 + MS_CL - 1) / MS_CL); }

}  // namespace
}  // namespace yt8m

using namespace yt8m;

extern "C" int64_t yt8m_multiscale_workspace_bytes(int64_t C) {
  if (C <= 0) return 0;
  return (2 * C + 2 * (int64_t)MS_RED_BLOCKS * C) * (int64_t)sizeof(float);
}

extern "C" int yt8m_colmoments_f32(const float* y, int64_t M, int64_t C, int64_t ldy, float* moving_mean, float* moving_var,
                                   int training, float eps, float decay, float* mean, float* rstd, void* workspace,
                                   int64_t workspace_bytes, yt8m_stream_t stream) {
  YT8M_REQUIRE(M >= 0 && C >= 0 && M < (1LL << 31) - 64 && C < (1LL << 31), YT8M_E_SHAPE, "bad dimension");
  if (M * C == 0) return YT8M_OK;
  YT8M_REQUIRE(C % 4 == 0, YT8M_E_SHAPE, "C must be a multiple of 4 (16-byte accesses)");
  YT8M_REQUIRE(ldy >= C && ldy % 4 == 0, YT8M_E_SHAPE, "ldy must be >= C and a multiple of 4");
  YT8M_REQUIRE(moving_mean && moving_var && mean && rstd, YT8M_E_BADARG, "null operand");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  if (!training) {
    hipLaunchKernelGGL(ms_frozen_stats_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, moving_mean, moving_var, (int)C, eps,
                       mean, rstd);
    return launch_status("ms_frozen_stats_kernel");
  }
  YT8M_REQUIRE(y && workspace, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(aligned16(y) && aligned16(mean) && aligned16(workspace), YT8M_E_BADARG, "y, mean and workspace must be 16-byte aligned");
  YT8M_REQUIRE(workspace_bytes >= yt8m_multiscale_workspace_bytes(C), YT8M_E_SHAPE, "workspace too small");
  const int rpb = rows_per_block(M, MS_RED_BLOCKS);
  const int nb = (int)((M + rpb - 1) / rpb);
  float* partial = static_cast<float*>(workspace) + 2 * C;
  const dim3 grid(col_groups(C), (unsigned)nb);
  hipLaunchKernelGGL(ms_colpartial_kernel<false>, grid, dim3(256), 0, s, y, (int)M, (int)C, (long long)ldy, (const float*)nullptr, rpb,
                     partial);
  hipLaunchKernelGGL(ms_mean_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, partial, nb, (int)C, (int)M, mean);
  hipLaunchKernelGGL(ms_colpartial_kernel<true>, grid, dim3(256), 0, s, y, (int)M, (int)C, (long long)ldy, (const float*)mean, rpb, partial);
  hipLaunchKernelGGL(ms_var_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, partial, nb, (int)C, (int)M, eps, decay,
                     (const float*)mean, rstd, moving_mean, moving_var);
  return launch_status("colmoments kernels");
}

static int pool2_check(int64_t F, int64_t B, int64_t C, int64_t ldy) {
  YT8M_REQUIRE(F >= 0 && B >= 0 && C >= 0 && C < (1LL << 31) && F < (1LL << 31) && B < (1LL << 31), YT8M_E_SHAPE, "bad dimension");
  YT8M_REQUIRE(F * B < (1LL << 31) - 64, YT8M_E_SHAPE, "too many frame rows");
  if (F * B * C == 0) return YT8M_OK;
  YT8M_REQUIRE(C % 4 == 0, YT8M_E_SHAPE, "C must be a multiple of 4 (16-byte accesses)");
  YT8M_REQUIRE(ldy >= C && ldy % 4 == 0, YT8M_E_SHAPE, "ldy must be >= C and a multiple of 4");
  return YT8M_OK;
}

extern "C" int yt8m_bn_relu_pool2_tm_fwd(const float* y, int64_t ldy, int64_t F, int64_t B, int64_t C, const float* gamma,
                                         const float* beta, const float* mean, const float* rstd, float* a, int64_t lda, float* pooled,
                                         int64_t ldp, yt8m_stream_t stream) {
  int rc = pool2_check(F, B, C, ldy);
  if (rc != YT8M_OK || F * B * C == 0) return rc;
  YT8M_REQUIRE(lda >= C && lda % 4 == 0 && (!pooled || (ldp >= C && ldp % 4 == 0)), YT8M_E_SHAPE,
               "lda / ldp must be >= C and a multiple of 4");
  YT8M_REQUIRE(y && gamma && beta && mean && rstd && a, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(aligned16(y) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(rstd) && aligned16(a) && aligned16(pooled),
               YT8M_E_BADARG, "operands must be 16-byte aligned");
  YT8M_REQUIRE(a != y && pooled != y && pooled != a, YT8M_E_BADARG, "outputs must not alias the input or each other");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int64_t NP = (F + 1) / 2 * B;
  const int rpb = rows_per_block(NP, MS_MAP_BLOCKS);
  hipLaunchKernelGGL(ms_bn_relu_pool2_fwd_kernel, dim3(col_groups(C), (unsigned)((NP + rpb - 1) / rpb)), dim3(256), 0, s, y, (long long)ldy,
                     (int)F, (int)B, (int)C, mean, rstd, gamma, beta, a, (long long)lda, pooled, (long long)ldp, rpb);
  return launch_status("ms_bn_relu_pool2_fwd_kernel");
}

extern "C" int yt8m_bn_relu_pool2_tm_bwd(const float* y, int64_t ldy, int64_t F, int64_t B, int64_t C, const float* gamma,
                                         const float* beta, const float* mean, const float* rstd, int training, const float* da,
                                         int64_t ldda, const float* dp, int64_t lddp, float* dy, int64_t lddy, float* dgamma,
                                         float dgamma_beta, float* dbeta, float dbeta_beta, void* workspace, int64_t workspace_bytes,
                                         yt8m_stream_t stream) {
  int rc = pool2_check(F, B, C, ldy);
  if (rc != YT8M_OK || F * B * C == 0) return rc;
  YT8M_REQUIRE((!da || (ldda >= C && ldda % 4 == 0)) && (!dp || (lddp >= C && lddp % 4 == 0)) && (!dy || (lddy >= C && lddy % 4 == 0)),
               YT8M_E_SHAPE, "ldda / lddp / lddy must be >= C and a multiple of 4");
  YT8M_REQUIRE(y && gamma && beta && mean && rstd && workspace && (da || dp), YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(aligned16(y) && aligned16(gamma) && aligned16(beta) && aligned16(mean) && aligned16(rstd) && aligned16(da) && aligned16(dp) &&
               aligned16(dy) && aligned16(workspace), YT8M_E_BADARG, "operands must be 16-byte aligned");
  YT8M_REQUIRE(dy != y && (!dy || dy != dp), YT8M_E_BADARG, "dy may replace da only");
  YT8M_REQUIRE(workspace_bytes >= yt8m_multiscale_workspace_bytes(C), YT8M_E_SHAPE, "workspace too small");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int64_t NP = (F + 1) / 2 * B;
  float* sums = static_cast<float*>(workspace);
  float* partial = sums + 2 * C;
  if (training || dgamma || dbeta) {
    const int rpb = rows_per_block(NP, MS_RED_BLOCKS);
    const int nb = (int)((NP + rpb - 1) / rpb);
    hipLaunchKernelGGL(ms_bwd_reduce_kernel, dim3(col_groups(C), (unsigned)nb), dim3(256), 0, s, y, (long long)ldy, (int)F, (int)B, (int)C,
                       mean, rstd, gamma, beta, da, (long long)ldda, dp, (long long)lddp, rpb, partial);
    hipLaunchKernelGGL(ms_bwd_finish_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const float*)partial, nb, (int)C, sums,
                       dgamma, dgamma_beta, dbeta, dbeta_beta);
  }
  if (dy) {
    const int rpb = rows_per_block(NP, MS_MAP_BLOCKS);
    hipLaunchKernelGGL(ms_bwd_apply_kernel, dim3(col_groups(C), (unsigned)((NP + rpb - 1) / rpb)), dim3(256), 0, s, y, (long long)ldy, (int)F,
                       (int)B, (int)C, mean, rstd, gamma, beta, da, (long long)ldda, dp, (long long)lddp, (const float*)sums, training, dy,
                       (long long)lddy, rpb);
  }
  return launch_status("bn_relu_pool2_tm_bwd kernels");
}
