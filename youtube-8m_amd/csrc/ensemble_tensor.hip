// ensemble_tensor.hip -- the two mixes of the ensemble stage that ens_combine (ensemble.hip) cannot express (gfx950, wave64):
//
// (1) E/all_ensemble_models/moe_model.py:51-54, the per-class [M, M] matrix over the methods:
//   g[b,v,l]  = sum_k x[b,v,k] W[v,k,l] + b[v,l];   p = softmax_l(g);   out[b,v] = sum_l p[b,v,l] x[b,v,l]
//   stat[0,b,v] = max_l g, stat[1,b,v] = 1 / sum_l exp(g - max)  (apart, as in ensemble.hip)
//   dg[b,v,l] = dout[b,v] p[b,v,l] (x[b,v,l] - out[b,v]);   dW[v,k,l] = sum_b x[b,v,k] dg[b,v,l];   db[v,l] = sum_b dg[b,v,l]
// Layouts: x is METHOD-MAJOR [M, B, V]; the weights travel v-innermost with the INPUT method k outermost: Wt [M(k), M(l), V], bt [M(l), V];
// out, dout [B, V]; stat [2, B, V].  A lane is one class v, so every access along v is a 256-byte line for any M and any alignment;
// nothing of size [B, V, M] is written.  2 B V M^2 FLOP each for g (forward; again backward) and dW: arithmetic and operand delivery
// bind, not HBM.
// forward: 4 waves x R rows of the same 64 classes; a thread keeps its R rows x[., v, :] in registers (MP = 16 / 48 / 80 padded methods,
//   R = 4 / 3 / 2: the register file decides), the workgroup streams Wt[:, l, v-tile] and bt[l] through LDS one l at a time (double
//   buffered, one barrier per l), and an online softmax over l with ONE exp and fp64 sums (ens_fwd_kernel's) finishes the row.
//   x[b,v,l], the value that l mixes, is loaded again (an L1 / L2 hit): indexing the register copy by l would put it in scratch.
// backward: a thread owns (v, l): Wt[:, l, v] and its dWt column in registers; 8 waves = 8 values of l over the same 64 classes walk ALL
//   B rows, two at a time (one with MP = 80), staged through LDS with their dout, stat and out (fetched into registers behind the arithmetic of the rows
//   before).  g is recomputed with the forward's own fmaf chain, so g <= max to the bit.  grid = (l groups, class tiles): one workgroup
//   sees every row, so there is no partial-sum buffer (yt8m_ens_tensor_bwd_workspace_bytes is 0), no atomics, and a second run gives the
//   same bits.
//
// (2) input_moe_model.py:33 / attention_moe_model.py:41, one mixing row per video:
//   out[b,v] = sum_k a[b,k] x[b,v,k];   da[b,k] = sum_v dout[b,v] x[b,v,k]
// forward: one streaming pass, the row's a wave-uniform, fp64 sums; backward: one workgroup per (row, method), fp64 sums finished in a
// fixed order (lanes by butterfly, then the 4 waves in order).
#include <math.h>
#include "common.h"

namespace {

constexpr int TENSOR_MAX_M = 80;
constexpr int BWD_WAVES = 8;

// grid (ceil(B / (4 R)), ceil(V / 64)); stat may be null
template <int MP, int R>
__global__ __launch_bounds__(256) void ens_tensor_fwd_kernel(const float* __restrict__ x, const float* __restrict__ Wt,
                                                             const float* __restrict__ bt, float* __restrict__ out,
                                                             float* __restrict__ stat, int B, int V, int M) {
  constexpr int ROWS = MP + 1, NPF = (ROWS + 3) / 4;                     // tile row MP is the bias
  __shared__ float ws[2][ROWS][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int vt = blockIdx.y * 64 + lane;
  const int v = min(vt, V - 1);                                          // idle lanes and rows repeat the last one, unstored
  const int b0 = (blockIdx.x * 4 + wave) * R;
  const size_t BV = (size_t)B * V;
  size_t at[R];
#pragma unroll
  for (int i = 0; i < R; ++i) at[i] = (size_t)min(b0 + i, B - 1) * V + v;
  float xr[R][MP];
#pragma unroll
  for (int k = 0; k < MP; ++k)
#pragma unroll
    for (int i = 0; i < R; ++i) xr[i][k] = k < M ? x[k * BV + at[i]] : 0.0f;

  float pf[NPF];
  auto fetch = [&](int l) {
#pragma unroll
    for (int jj = 0; jj < NPF; ++jj) {
      const int j = wave + 4 * jj;
      pf[jj] = j < M ? Wt[((size_t)j * M + l) * V + v] : (j == MP ? bt[(size_t)l * V + v] : 0.0f);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int jj = 0; jj < NPF; ++jj) {
      const int j = wave + 4 * jj;
      if (j < ROWS) ws[buf][j][lane] = pf[jj];
    }
  };
  fetch(0);
  stage(0);
  __syncthreads();
  float m[R];
  double s[R], acc[R];
  for (int l = 0; l < M; ++l) {
    const int cur = l & 1;
    if (l + 1 < M) fetch(l + 1);
    float xl[R], g[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      xl[i] = x[l * BV + at[i]];
      g[i] = ws[cur][MP][lane];
    }
#pragma unroll
    for (int k8 = 0; k8 < MP; k8 += 8) {
      if (k8 < M) {                                                      // (uniform) rows k >= M of the tile and of xr are zero
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const float w = ws[cur][k8 + kk][lane];
#pragma unroll
          for (int i = 0; i < R; ++i) g[i] = fmaf(xr[i][k8 + kk], w, g[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (l == 0) {
        m[i] = g[i];
        s[i] = 1.0;
        acc[i] = (double)xl[i];
      } else {
        const float d = g[i] - m[i];
        const float e = __expf(-fabsf(d));
        const bool up = d > 0.0f;                                        // a new maximum: the running sums shrink by e, the term weighs 1
        const double keep = up ? (double)e : 1.0, wgt = up ? 1.0 : (double)e;
        s[i] = fma(s[i], keep, wgt);
        acc[i] = fma(acc[i], keep, wgt * (double)xl[i]);
        m[i] = fmaxf(m[i], g[i]);
      }
    }
    if (l + 1 < M) stage(cur ^ 1);                                       // last read before the barrier that ended iteration l - 1
    __syncthreads();
  }
  if (vt < V) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (b0 + i < B) {
        out[at[i]] = (float)(acc[i] / s[i]);
        if (stat) {
          stat[at[i]] = m[i];
          stat[BV + at[i]] = (float)(1.0 / s[i]);
        }
      }
    }
  }
}

// grid (ceil(M / 8), ceil(V / 64)); wave = one l, lane = one class
template <int MP>
__global__ __launch_bounds__(64 * BWD_WAVES) void ens_tensor_bwd_kernel(const float* __restrict__ x, const float* __restrict__ Wt,
                                                                        const float* __restrict__ bt, const float* __restrict__ out,
                                                                        const float* __restrict__ stat, const float* __restrict__ dout,
                                                                        float* __restrict__ dWt, float* __restrict__ dbt, int B, int V,
                                                                        int M) {
  constexpr int BWD_RB = MP > 48 ? 1 : 2;                                // rows per tile: what the registers of the prefetch leave room for
  constexpr int ROWS = MP + 4, TILE = BWD_RB * ROWS, NPF = (TILE + BWD_WAVES - 1) / BWD_WAVES;   // tile rows MP..MP+3: dout, max, 1/sum, out
  __shared__ float xs[BWD_RB][ROWS][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int vt = blockIdx.y * 64 + lane, lt = blockIdx.x * BWD_WAVES + wave;
  const int v = min(vt, V - 1), l = min(lt, M - 1);                     // idle lanes and waves repeat the last one, unstored
  const size_t BV = (size_t)B * V;
  const size_t MV = (size_t)M * V, lv = (size_t)l * V + v;
  float w[MP], a[MP];
  {
    const float* wp = Wt + lv;
#pragma unroll
    for (int k = 0; k < MP; ++k, wp += MV) {
      w[k] = k < M ? *wp : 0.0f;
      a[k] = 0.0f;
    }
  }
  const float bias = bt[lv];
  float db = 0.0f;

  float pf[NPF];
  auto fetch = [&](int b0) {
#pragma unroll
    for (int jj = 0; jj < NPF; ++jj) {
      const int e = wave + BWD_WAVES * jj, r = e / ROWS, j = e - r * ROWS, b = b0 + r;
      float t = 0.0f;
      if (e < TILE && b < B) {
        const size_t at = (size_t)b * V + v;
        if (j < M) t = x[j * BV + at];
        else if (j == MP) t = dout[at];
        else if (j == MP + 1) t = stat[at];
        else if (j == MP + 2) t = stat[BV + at];
        else if (j == MP + 3) t = out[at];
      }
      pf[jj] = t;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int jj = 0; jj < NPF; ++jj) {
      const int e = wave + BWD_WAVES * jj, r = e / ROWS, j = e - r * ROWS;
      if (e < TILE) xs[r][j][lane] = pf[jj];
    }
  };
  fetch(0);
  stage();
  __syncthreads();
  for (int b0 = 0; b0 < B; b0 += BWD_RB) {
    const bool more = b0 + BWD_RB < B;
    if (more) fetch(b0 + BWD_RB);
#pragma unroll
    for (int r = 0; r < BWD_RB; ++r) {
      if (b0 + r < B) {                                                  // (uniform)
        float g = bias;
#pragma unroll
        for (int k8 = 0; k8 < MP; k8 += 8) {
          if (k8 < M) {
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) g = fmaf(xs[r][k8 + kk][lane], w[k8 + kk], g);
          }
        }
        const float p = __expf(g - xs[r][MP + 1][lane]) * xs[r][MP + 2][lane];
        const float dg = xs[r][MP][lane] * p * (xs[r][l][lane] - xs[r][MP + 3][lane]);
        db += dg;
#pragma unroll
        for (int k8 = 0; k8 < MP; k8 += 8) {
          if (k8 < M) {
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) a[k8 + kk] = fmaf(xs[r][k8 + kk][lane], dg, a[k8 + kk]);
          }
        }
      }
    }
    __syncthreads();                                                     // every wave is done with the tile
    if (more) stage();
    __syncthreads();
  }
  if (vt < V && lt < M) {
    float* ap = dWt + lv;
#pragma unroll
    for (int k = 0; k < MP; ++k, ap += MV)
      if (k < M) *ap = a[k];
    dbt[lv] = db;
  }
}

// grid B * ceil(V / (64 VW)), block 64
template <int VW>
__global__ __launch_bounds__(64) void ens_mix_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a, float* __restrict__ out,
                                                         int B, int V, int M, int tiles) {
  const int b = blockIdx.x / tiles;                                      // (uniform)
  const int v0 = ((blockIdx.x - b * tiles) * 64 + threadIdx.x) * VW;
  if (v0 >= V) return;
  const size_t BV = (size_t)B * V, at = (size_t)b * V + v0;
  double acc[VW];
#pragma unroll
  for (int c = 0; c < VW; ++c) acc[c] = 0.0;
  for (int k = 0; k < M; ++k) {
    const double ak = (double)a[(size_t)b * M + k];
    float xv[VW];
    ldv<VW>(x + k * BV + at, xv);
#pragma unroll
    for (int c = 0; c < VW; ++c) acc[c] = fma((double)xv[c], ak, acc[c]);
  }
  float o[VW];
#pragma unroll
  for (int c = 0; c < VW; ++c) o[c] = (float)acc[c];
  stv<VW>(out + at, o);
}

// grid B * M (method fastest: the workgroups of one row share its dout), block 256
__global__ __launch_bounds__(256) void ens_mix_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dout, float* __restrict__ da,
                                                          int B, int V, int M) {
  __shared__ double red[4];
  const int b = blockIdx.x / M, k = blockIdx.x - b * M;
  const float* xp = x + ((size_t)k * B + b) * V;
  const float* dp = dout + (size_t)b * V;
  double s = 0.0;
  for (int v = threadIdx.x; v < V; v += 256) s = fma((double)dp[v], (double)xp[v], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) da[(size_t)b * M + k] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

inline bool tensor_shape_ok(int64_t B, int64_t V, int64_t M) { return B <= (1 << 24) && V <= 64 * 65535; }
inline bool mix_shape_ok(int64_t B, int64_t V, int64_t M) {
  return V <= (1 << 24) && M <= (1 << 16) && B * M <= 0x7fffffffLL && B * cdiv(V, 64) <= 0x7fffffffLL;
}

template <int MP, int R>
void launch_tensor_fwd(const float* x, const float* Wt, const float* bt, float* out, float* stat, int B, int V, int M, hipStream_t s) {
  const dim3 grid((unsigned)cdiv(B, 4 * R), (unsigned)cdiv(V, 64)), block(256);
  hipLaunchKernelGGL((ens_tensor_fwd_kernel<MP, R>), grid, block, 0, s, x, Wt, bt, out, stat, B, V, M);
}

template <int MP>
void launch_tensor_bwd(const float* x, const float* Wt, const float* bt, const float* out, const float* stat, const float* dout, float* dWt,
                       float* dbt, int B, int V, int M, hipStream_t s) {
  const dim3 grid((unsigned)cdiv(M, BWD_WAVES), (unsigned)cdiv(V, 64)), block(64 * BWD_WAVES);
  hipLaunchKernelGGL((ens_tensor_bwd_kernel<MP>), grid, block, 0, s, x, Wt, bt, out, stat, dout, dWt, dbt, B, V, M);
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_ens_tensor_max_methods(void) { return TENSOR_MAX_M; }

extern "C" int yt8m_ens_tensor_fwd(const float* x, const float* Wt, const float* bt, float* out, float* stat, int64_t B, int64_t V,
                                   int64_t M, yt8m_stream_t stream) {
  YT8M_REQUIRE(x && Wt && bt && out, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(B > 0 && V > 0 && M > 0, YT8M_E_BADARG, "B, V, M must be positive");
  YT8M_REQUIRE(M <= TENSOR_MAX_M, YT8M_E_BADARG, "M <= yt8m_ens_tensor_max_methods() = 80");
  YT8M_REQUIRE(tensor_shape_ok(B, V, M), YT8M_E_SHAPE, "B <= 2^24, V <= 64 x 65535");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int b = (int)B, v = (int)V, m = (int)M;
  if (m <= 16) launch_tensor_fwd<16, 4>(x, Wt, bt, out, stat, b, v, m, s);
  else if (m <= 48) launch_tensor_fwd<48, 3>(x, Wt, bt, out, stat, b, v, m, s);
  else launch_tensor_fwd<80, 2>(x, Wt, bt, out, stat, b, v, m, s);
  return launch_status("ens_tensor_fwd_kernel");
}

extern "C" int64_t yt8m_ens_tensor_bwd_workspace_bytes(int64_t B, int64_t V, int64_t M) {
  if (B <= 0 || V <= 0 || M <= 0 || M > TENSOR_MAX_M || !tensor_shape_ok(B, V, M)) return -1;
  return 0;                                                              // one workgroup sees every row: no partial sums
}

extern "C" int yt8m_ens_tensor_bwd(const float* x, const float* Wt, const float* bt, const float* out, const float* stat, const float* dout,
                                   float* dWt, float* dbt, void* workspace, int64_t workspace_bytes, int64_t B, int64_t V, int64_t M,
                                   yt8m_stream_t stream) {
  YT8M_REQUIRE(x && Wt && bt && out && stat && dout && dWt && dbt, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(B > 0 && V > 0 && M > 0, YT8M_E_BADARG, "B, V, M must be positive");
  YT8M_REQUIRE(M <= TENSOR_MAX_M, YT8M_E_BADARG, "M <= yt8m_ens_tensor_max_methods() = 80");
  YT8M_REQUIRE(tensor_shape_ok(B, V, M), YT8M_E_SHAPE, "B <= 2^24, V <= 64 x 65535");
  const int64_t need = yt8m_ens_tensor_bwd_workspace_bytes(B, V, M);
  YT8M_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), YT8M_E_BADARG,
               "workspace smaller than yt8m_ens_tensor_bwd_workspace_bytes");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int b = (int)B, v = (int)V, m = (int)M;
  if (m <= 16) launch_tensor_bwd<16>(x, Wt, bt, out, stat, dout, dWt, dbt, b, v, m, s);
  else if (m <= 48) launch_tensor_bwd<48>(x, Wt, bt, out, stat, dout, dWt, dbt, b, v, m, s);
  else launch_tensor_bwd<80>(x, Wt, bt, out, stat, dout, dWt, dbt, b, v, m, s);
  return launch_status("ens_tensor_bwd_kernel");
}

extern "C" int yt8m_ens_mix_fwd(const float* x, const float* a, float* out, int64_t B, int64_t V, int64_t M, yt8m_stream_t stream) {
  YT8M_REQUIRE(x && a && out, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(B > 0 && V > 0 && M > 0, YT8M_E_BADARG, "B, V, M must be positive");
  YT8M_REQUIRE(mix_shape_ok(B, V, M), YT8M_E_SHAPE, "V <= 2^24, M <= 2^16, B M and B ceil(V / 64) below 2^31");
  const bool vec = (V & 3) == 0 && aligned16(x) && aligned16(out);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int tiles = (int)cdiv(V, vec ? 256 : 64);
  if (vec) hipLaunchKernelGGL(ens_mix_fwd_kernel<4>, dim3((unsigned)(B * tiles)), dim3(64), 0, s, x, a, out, (int)B, (int)V, (int)M, tiles);
  else hipLaunchKernelGGL(ens_mix_fwd_kernel<1>, dim3((unsigned)(B * tiles)), dim3(64), 0, s, x, a, out, (int)B, (int)V, (int)M, tiles);
  return launch_status("ens_mix_fwd_kernel");
}

extern "C" int yt8m_ens_mix_bwd(const float* x, const float* dout, float* da, int64_t B, int64_t V, int64_t M, yt8m_stream_t stream) {
  YT8M_REQUIRE(x && dout && da, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(B > 0 && V > 0 && M > 0, YT8M_E_BADARG, "B, V, M must be positive");
  YT8M_REQUIRE(mix_shape_ok(B, V, M), YT8M_E_SHAPE, "V <= 2^24, M <= 2^16, B M and B ceil(V / 64) below 2^31");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  hipLaunchKernelGGL(ens_mix_bwd_kernel, dim3((unsigned)(B * M)), dim3(256), 0, s, x, dout, da, (int)B, (int)V, (int)M);
  return launch_status("ens_mix_bwd_kernel");
}
