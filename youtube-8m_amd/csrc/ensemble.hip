// ensemble.hip -- the ensemble stage's combine (E/all_ensemble_models/*.py, E = youtube-8m-ensemble of the reference) in one streaming
// pass over the stacked predictions each way (gfx950, wave64; HBM-bound: x is 1.43 GB at B = 1024, V = 4716, M = 74):
//   logit[b,v,k] = sum_j gate[b,j] W[j,v,k]     (gate == nullptr: J = 1 and gate = 1)
//   out[b,v]     = sum_k softmax_k(logit)[k] t(x[b,v,k]);   stat[0,b,v] = max_k logit, stat[1,b,v] = 1 / sum_k exp(logit - max)
//   t = identity, or (xform 1) log((eps + x) / (1 + eps - x)), eps = 1e-5 (nonunit_matrix_regression_model.py:27)
//   dl[b,v,k]    = dout[b,v] exp(logit - max) / sum (t - out);   dW[j,v,k] = sum_b gate[b,j] dl;   dgate[b,j] = sum_{v,k} dl W[j,v,k]
// Layouts: x is METHOD-MAJOR [M, B, V] (a [B, V, M] view of strides (V, 1, B V)); the tables travel v-innermost, Wt [J, M, V]; out,
// dout [B, V]; stat [2, B, V]; gate, dgate [B, J]; dWt [J, M, V].  Every access along v is coalesced for any M, nothing of size [B, V, M] is written.
//
// forward: a thread owns VW columns (4 with 16-byte accesses where V % 4 == 0 and every pointer is 16-byte aligned, else 1) and FWD_ROWS
//   rows; k outermost, so the J table values of (k, v) are loaded once per FWD_ROWS elements; the rows' gate values are wave-uniform.  An
//   online softmax (m, s, acc) per element with ONE exp: e = exp(-|logit - m|) scales either the running sums or the new term.  s and acc
//   are fp64 (full-rate FMA on this chip): a serial fp32 sum of 74..130 terms errs by more than the softmax it sums.
// backward: with stat and out every (b, v, k) is independent.  (The maximum and the sum are saved apart, not as lse = max + log sum:
//   logits of +-80 round lse to 4e-6, a relative error of that size in every weight; logit - max is exact where it matters.)  A thread
//   owns VW columns x KR methods (table values and dW accumulators in
//   registers) and walks one chunk of rows; grid = (column tiles, method ranges, row chunks).  The chunk is ceil(B / min(8, ceil(B / 16))):
//   at most 8 chunks, so the per-chunk partials are at most 8 x the table (45 MB at J = 4, M = 74 against the 1.43 GB of x), summed in
//   chunk order by a second kernel; a single chunk writes dWt directly.  dgate comes from the same pass -- the table values are in
//   registers already: J FMAs per element, one wave butterfly per row, lane 0 writes the (tile, range) partial; a second kernel adds the
//   partials in a fixed order.  No atomics anywhere: a second run gives the same bits.
// moments: mean over the methods and, optionally, the unbiased variance, one pass, fp64 sums (sum x, sum x^2).
#include <math.h>
#include "common.h"

namespace {

constexpr int ENS_MAX_J = 4;
constexpr int FWD_ROWS = 4;
constexpr int BWD_MAX_CHUNKS = 8;
constexpr int BWD_MIN_CHUNK = 16;
constexpr float LOGIT_EPS = 1e-5f;

template <bool LOGIT>
__device__ __forceinline__ float xform(float x) {
  if (LOGIT) return logf(__fdividef(LOGIT_EPS + x, (1.0f + LOGIT_EPS) - x));
  return x;
}

// grid (ceil(V / (64 VW)), ceil(B / FWD_ROWS)); stat [2, B, V] may be null
template <int J, int VW, bool LOGIT>
__global__ __launch_bounds__(64) void ens_fwd_kernel(const float* __restrict__ x, const float* __restrict__ Wt, const float* __restrict__ gate,
                                                     float* __restrict__ out, float* __restrict__ stat, int B, int V, int M) {
  const int v0 = (blockIdx.x * 64 + threadIdx.x) * VW;
  if (v0 >= V) return;
  const int b0 = blockIdx.y * FWD_ROWS;
  const int nb = min(FWD_ROWS, B - b0);                                  // (uniform) rows past the tail repeat the last one, unstored
  const size_t BV = (size_t)B * V, MV = (size_t)M * V;
  int row[FWD_ROWS];
  float g[FWD_ROWS][J];
#pragma unroll
  for (int i = 0; i < FWD_ROWS; ++i) {
    row[i] = b0 + min(i, nb - 1);
#pragma unroll
    for (int j = 0; j < J; ++j) g[i][j] = gate ? gate[(size_t)row[i] * J + j] : 1.0f;
  }
  float m[FWD_ROWS][VW];
  double s[FWD_ROWS][VW], acc[FWD_ROWS][VW];
  for (int k = 0; k < M; ++k) {
    float w[J][VW];
#pragma unroll
    for (int j = 0; j < J; ++j) ldv<VW>(Wt + j * MV + (size_t)k * V + v0, w[j]);
    float xv[FWD_ROWS][VW];
#pragma unroll
    for (int i = 0; i < FWD_ROWS; ++i) ldv<VW>(x + k * BV + (size_t)row[i] * V + v0, xv[i]);
#pragma unroll
    for (int i = 0; i < FWD_ROWS; ++i) {
#pragma unroll
      for (int c = 0; c < VW; ++c) {
        float logit = g[i][0] * w[0][c];
#pragma unroll
        for (int j = 1; j < J; ++j) logit = fmaf(g[i][j], w[j][c], logit);
        const float t = xform<LOGIT>(xv[i][c]);
        if (k == 0) {
          m[i][c] = logit;
          s[i][c] = 1.0;
          acc[i][c] = (double)t;
        } else {
          const float d = logit - m[i][c];
          const float e = __expf(-fabsf(d));
          const bool up = d > 0.0f;                                      // a new maximum: the running sums shrink by e, the term weighs 1
          const double keep = up ? (double)e : 1.0, wgt = up ? 1.0 : (double)e;
          s[i][c] = fma(s[i][c], keep, wgt);
          acc[i][c] = fma(acc[i][c], keep, wgt * (double)t);
          m[i][c] = fmaxf(m[i][c], logit);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < FWD_ROWS; ++i) {
    if (i < nb) {
      float o[VW], l[VW];
#pragma unroll
      for (int c = 0; c < VW; ++c) {
        o[c] = (float)(acc[i][c] / s[i][c]);
        l[c] = (float)(1.0 / s[i][c]);
      }
      stv<VW>(out + (size_t)row[i] * V + v0, o);
      if (stat) {
        stv<VW>(stat + (size_t)row[i] * V + v0, m[i]);
        stv<VW>(stat + BV + (size_t)row[i] * V + v0, l);
      }
    }
  }
}

// grid (ceil(V / (64 VW)), ceil(M / KR), chunks); dWp [chunks, J, M, V] (dWt itself with one chunk); dgp [gridDim.y * gridDim.x, B, J]
template <int J, int VW, int KR, bool LOGIT, bool GATE>
__global__ __launch_bounds__(64) void ens_bwd_kernel(const float* __restrict__ x, const float* __restrict__ Wt, const float* __restrict__ gate,
                                                     const float* __restrict__ out, const float* __restrict__ stat,
                                                     const float* __restrict__ dout, float* __restrict__ dWp, float* __restrict__ dgp,
                                                     int B, int V, int M, int chunk) {
  const int vt = (blockIdx.x * 64 + threadIdx.x) * VW;
  const bool active = vt < V;                                            // idle lanes read column 0 and contribute nothing
  const int v0 = active ? vt : 0;
  const int k0 = blockIdx.y * KR;
  const int nk = min(KR, M - k0);                                        // (uniform)
  const int b0 = blockIdx.z * chunk, b1 = min(B, b0 + chunk);
  const size_t BV = (size_t)B * V, MV = (size_t)M * V;
  float w[J][KR][VW], a[J][KR][VW];
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int kk = 0; kk < KR; ++kk) {
      ldv<VW>(Wt + j * MV + (size_t)(k0 + min(kk, nk - 1)) * V + v0, w[j][kk]);
#pragma unroll
      for (int c = 0; c < VW; ++c) a[j][kk][c] = 0.0f;
    }
  const size_t part = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int b = b0; b < b1; ++b) {
    float go[VW], mx[VW], is[VW], ou[VW], xv[KR][VW], g[J], pg[J];
    ldv<VW>(dout + (size_t)b * V + v0, go);
    ldv<VW>(stat + (size_t)b * V + v0, mx);
    ldv<VW>(stat + BV + (size_t)b * V + v0, is);
    ldv<VW>(out + (size_t)b * V + v0, ou);
#pragma unroll
    for (int kk = 0; kk < KR; ++kk) ldv<VW>(x + (size_t)(k0 + min(kk, nk - 1)) * BV + (size_t)b * V + v0, xv[kk]);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      g[j] = GATE ? gate[(size_t)b * J + j] : 1.0f;
      pg[j] = 0.0f;
    }
#pragma unroll
    for (int kk = 0; kk < KR; ++kk) {
      if (kk < nk) {
#pragma unroll
        for (int c = 0; c < VW; ++c) {
          float logit = g[0] * w[0][kk][c];
#pragma unroll
          for (int j = 1; j < J; ++j) logit = fmaf(g[j], w[j][kk][c], logit);
          const float t = xform<LOGIT>(xv[kk][c]);
          const float p = __expf(logit - mx[c]) * is[c];
          const float diff = t - ou[c];
          const float dl = go[c] * p * diff;
#pragma unroll
          for (int j = 0; j < J; ++j) {
            a[j][kk][c] = fmaf(g[j], dl, a[j][kk][c]);
            if (GATE) pg[j] = fmaf(dl, w[j][kk][c], pg[j]);
          }
        }
      }
    }
    if (GATE) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const float r = wave_sum(active ? pg[j] : 0.0f);
        if (threadIdx.x == 0) dgp[(part * B + b) * J + j] = r;
      }
    }
  }
  if (active) {
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int kk = 0; kk < KR; ++kk)
        if (kk < nk) stv<VW>(dWp + ((size_t)blockIdx.z * J + j) * MV + (size_t)(k0 + kk) * V + v0, a[j][kk]);
  }
}

// dst[i] = sum_c src[c, i] in the order of c
__global__ __launch_bounds__(256) void ens_sum_parts_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n, int parts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float r = src[i];
  for (int c = 1; c < parts; ++c) r += src[(size_t)c * n + i];
  dst[i] = r;
}

// grid (ceil(V / (64 VW)), B); var may be null
template <int VW>
__global__ __launch_bounds__(64) void ens_moments_kernel(const float* __restrict__ x, float* __restrict__ mean, float* __restrict__ var,
                                                         int B, int V, int M) {
  const int v0 = (blockIdx.x * 64 + threadIdx.x) * VW;
  if (v0 >= V) return;
  const size_t BV = (size_t)B * V, at = (size_t)blockIdx.y * V + v0;
  double s1[VW], s2[VW];
#pragma unroll
  for (int c = 0; c < VW; ++c) s1[c] = s2[c] = 0.0;
  for (int k = 0; k < M; ++k) {
    float xv[VW];
    ldv<VW>(x + k * BV + at, xv);
#pragma unroll
    for (int c = 0; c < VW; ++c) {
      const double d = (double)xv[c];
      s1[c] += d;
      s2[c] = fma(d, d, s2[c]);
    }
  }
  float mu[VW], va[VW];
#pragma unroll
  for (int c = 0; c < VW; ++c) {
    const double mean64 = s1[c] / (double)M;
    mu[c] = (float)mean64;
    va[c] = (float)fmax((s2[c] - s1[c] * mean64) / (double)(M - 1), 0.0);
  }
  stv<VW>(mean + at, mu);
  if (var) stv<VW>(var + at, va);
}

inline int bwd_chunks(int64_t B) {
  const int64_t n = (B + BWD_MIN_CHUNK - 1) / BWD_MIN_CHUNK;
  return (int)(n < BWD_MAX_CHUNKS ? n : BWD_MAX_CHUNKS);
}

constexpr int KR4 = 4, KR1 = 8;          // methods per thread of the backward kernel on the 16-byte and on the single-element path

// floats of the dgate partials: the larger of the two paths' (tile, range) counts
inline int64_t dgate_parts(int64_t V, int64_t M) {
  const int64_t p1 = cdiv(V, 64) * cdiv(M, KR1), p4 = cdiv(V, 256) * cdiv(M, KR4);
  return p1 > p4 ? p1 : p4;
}

inline bool shape_ok(int64_t B, int64_t V, int64_t M) { return B <= 262140 && V <= (1 << 24) && M <= (1 << 16); }

template <int J, int VW, bool LOGIT>
void launch_fwd(const float* x, const float* Wt, const float* gate, float* out, float* stat, int B, int V, int M, hipStream_t s) {
  const dim3 grid((unsigned)cdiv(V, 64 * VW), (unsigned)cdiv(B, FWD_ROWS)), block(64);
  hipLaunchKernelGGL((ens_fwd_kernel<J, VW, LOGIT>), grid, block, 0, s, x, Wt, gate, out, stat, B, V, M);
}

template <int J, int VW, bool LOGIT, bool GATE>
void launch_bwd(const float* x, const float* Wt, const float* gate, const float* out, const float* stat, const float* dout, float* dWp,
                float* dgp, int B, int V, int M, int chunk, int chunks, hipStream_t s) {
  constexpr int KR = VW == 4 ? KR4 : KR1;
  const dim3 grid((unsigned)cdiv(V, 64 * VW), (unsigned)cdiv(M, KR), (unsigned)chunks), block(64);
  hipLaunchKernelGGL((ens_bwd_kernel<J, VW, KR, LOGIT, GATE>), grid, block, 0, s, x, Wt, gate, out, stat, dout, dWp, dgp, B, V, M, chunk);
}

template <int J, bool LOGIT>
void launch_fwd_vw(bool vec, const float* x, const float* Wt, const float* gate, float* out, float* stat, int B, int V, int M, hipStream_t s) {
  if (vec) launch_fwd<J, 4, LOGIT>(x, Wt, gate, out, stat, B, V, M, s);
  else launch_fwd<J, 1, LOGIT>(x, Wt, gate, out, stat, B, V, M, s);
}

template <int J, bool LOGIT, bool GATE>
void launch_bwd_vw(bool vec, const float* x, const float* Wt, const float* gate, const float* out, const float* stat, const float* dout,
                   float* dWp, float* dgp, int B, int V, int M, int chunk, int chunks, hipStream_t s) {
  if (vec) launch_bwd<J, 4, LOGIT, GATE>(x, Wt, gate, out, stat, dout, dWp, dgp, B, V, M, chunk, chunks, s);
  else launch_bwd<J, 1, LOGIT, GATE>(x, Wt, gate, out, stat, dout, dWp, dgp, B, V, M, chunk, chunks, s);
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_ens_max_gates(void) { return ENS_MAX_J; }

extern "C" int yt8m_ens_combine_fwd(const float* x, const float* Wt, const float* gate, int xform, float* out, float* stat, int64_t B,
                                    int64_t V, int64_t M, int J, yt8m_stream_t stream) {
  YT8M_REQUIRE(x && Wt && out, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(B > 0 && V > 0 && M > 0, YT8M_E_BADARG, "B, V, M must be positive");
  YT8M_REQUIRE(J >= 1 && J <= ENS_MAX_J, YT8M_E_BADARG, "1 <= J <= 4 tables");
  YT8M_REQUIRE(gate || J == 1, YT8M_E_BADARG, "no gate means one table");
  YT8M_REQUIRE(xform == 0 || xform == 1, YT8M_E_BADARG, "xform: 0 (identity) or 1 (logit)");
  YT8M_REQUIRE(shape_ok(B, V, M), YT8M_E_SHAPE, "B <= 262140, V <= 2^24, M <= 2^16");
  const bool vec = (V & 3) == 0 && aligned16(x) && aligned16(Wt) && aligned16(out) && aligned16(stat);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int b = (int)B, v = (int)V, m = (int)M;
#define ENS_FWD(JJ)                                                              \
  case JJ:                                                                       \
    if (xform) launch_fwd_vw<JJ, true>(vec, x, Wt, gate, out, stat, b, v, m, s);  \
    else launch_fwd_vw<JJ, false>(vec, x, Wt, gate, out, stat, b, v, m, s);       \
    break;
  switch (J) { ENS_FWD(1) ENS_FWD(2) ENS_FWD(3) ENS_FWD(4) }
#undef ENS_FWD
  return launch_status("ens_fwd_kernel");
}

extern "C" int64_t yt8m_ens_combine_bwd_workspace_bytes(int64_t B, int64_t V, int64_t M, int J) {
  if (B <= 0 || V <= 0 || M <= 0 || J < 1 || J > ENS_MAX_J || !shape_ok(B, V, M)) return -1;
  const int chunks = bwd_chunks(B);
  const int64_t dw = chunks > 1 ? (int64_t)chunks * J * M * V : 0;
  return (dw + dgate_parts(V, M) * B * J) * (int64_t)sizeof(float);
}

extern "C" int yt8m_ens_combine_bwd(const float* x, const float* Wt, const float* gate, int xform, const float* out, const float* stat,
                                    const float* dout, float* dWt, float* dgate, void* workspace, int64_t workspace_bytes, int64_t B,
                                    int64_t V, int64_t M, int J, yt8m_stream_t stream) {
  YT8M_REQUIRE(x && Wt && out && stat && dout && dWt, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(B > 0 && V > 0 && M > 0, YT8M_E_BADARG, "B, V, M must be positive");
  YT8M_REQUIRE(J >= 1 && J <= ENS_MAX_J, YT8M_E_BADARG, "1 <= J <= 4 tables");
  YT8M_REQUIRE(gate || J == 1, YT8M_E_BADARG, "no gate means one table");
  YT8M_REQUIRE((gate != nullptr) == (dgate != nullptr), YT8M_E_BADARG, "dgate goes with gate");
  YT8M_REQUIRE(xform == 0 || xform == 1, YT8M_E_BADARG, "xform: 0 (identity) or 1 (logit)");
  YT8M_REQUIRE(shape_ok(B, V, M), YT8M_E_SHAPE, "B <= 262140, V <= 2^24, M <= 2^16");
  const int64_t need = yt8m_ens_combine_bwd_workspace_bytes(B, V, M, J);
  YT8M_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), YT8M_E_BADARG, "workspace smaller than yt8m_ens_combine_bwd_workspace_bytes");
  const int chunks = bwd_chunks(B);
  const int chunk = (int)cdiv(B, chunks);
  const int64_t table = (int64_t)J * M * V;
  float* dWp = chunks > 1 ? static_cast<float*>(workspace) : dWt;
  float* dgp = static_cast<float*>(workspace) + (chunks > 1 ? chunks * table : 0);
  const bool vec = (V & 3) == 0 && aligned16(x) && aligned16(Wt) && aligned16(out) && aligned16(stat) && aligned16(dout) && aligned16(dWp);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int b = (int)B, v = (int)V, m = (int)M;
#define ENS_BWD(JJ, GG)                                                                                        \
  if (xform) launch_bwd_vw<JJ, true, GG>(vec, x, Wt, gate, out, stat, dout, dWp, dgp, b, v, m, chunk, chunks, s); \
  else launch_bwd_vw<JJ, false, GG>(vec, x, Wt, gate, out, stat, dout, dWp, dgp, b, v, m, chunk, chunks, s);
  if (!gate) {
    ENS_BWD(1, false)
  } else {
    switch (J) {
      case 1: ENS_BWD(1, true) break;
      case 2: ENS_BWD(2, true) break;
      case 3: ENS_BWD(3, true) break;
      case 4: ENS_BWD(4, true) break;
    }
  }
#undef ENS_BWD
  int st = launch_status("ens_bwd_kernel");
  if (st != YT8M_OK) return st;
  if (chunks > 1) {
    hipLaunchKernelGGL(ens_sum_parts_kernel, dim3((unsigned)cdiv(table, 256)), dim3(256), 0, s, dWp, dWt, table, chunks);
    st = launch_status("ens_sum_parts_kernel");
    if (st != YT8M_OK) return st;
  }
  if (gate) {
    const int64_t parts = vec ? cdiv(V, 256) * cdiv(M, KR4) : cdiv(V, 64) * cdiv(M, KR1);
    hipLaunchKernelGGL(ens_sum_parts_kernel, dim3((unsigned)cdiv(B * J, 256)), dim3(256), 0, s, dgp, dgate, B * J, (int)parts);
    st = launch_status("ens_sum_parts_kernel");
  }
  return st;
}

extern "C" int yt8m_ens_moments(const float* x, float* mean, float* var, int64_t B, int64_t V, int64_t M, yt8m_stream_t stream) {
  YT8M_REQUIRE(x && mean, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(B > 0 && V > 0 && M > 0, YT8M_E_BADARG, "B, V, M must be positive");
  YT8M_REQUIRE(!var || M >= 2, YT8M_E_BADARG, "the unbiased variance needs M >= 2");
  YT8M_REQUIRE(B <= 65535 && V <= (1 << 24) && M <= (1 << 16), YT8M_E_SHAPE, "B <= 65535, V <= 2^24, M <= 2^16");
  const bool vec = (V & 3) == 0 && aligned16(x) && aligned16(mean) && aligned16(var);
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  if (vec)
    hipLaunchKernelGGL(ens_moments_kernel<4>, dim3((unsigned)cdiv(V, 256), (unsigned)B), dim3(64), 0, s, x, mean, var, (int)B, (int)V, (int)M);
  else
    hipLaunchKernelGGL(ens_moments_kernel<1>, dim3((unsigned)cdiv(V, 64), (unsigned)B), dim3(64), 0, s, x, mean, var, (int)B, (int)V, (int)M);
  return launch_status("ens_moments_kernel");
}
