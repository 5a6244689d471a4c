// sigmoid_attention.hip -- the sigmoid attention pooling of W/all_frame_models/lstm_attention_model.py:61-73, lstm_attention_lstm_model.py:
// 78-92 and lstm_multi_attention_model.py:63-78 in one pass each way over the TIME-major tensors the LSTM stack leaves (gfx950, wave64;
// HBM-bound: src and vals are 157 MB each at F = 300, B = 128, H = 1024).  m[t,b] = 1 for t < clamp(num_frames[b], 0, F), else 0:
//   z[t,b,a]      = src[t,b,:] . Wa[:,a] + ba[a]          src [F,B,Hs] (row stride ld_src), Wa [Hs,A]
//   s[t,b,a]      = sigmoid(z) m[t,b];   den[b,a] = sum_t s + 1e-8;   att[b,t,a] = s / den        (att is BATCH-major [B,F,A])
//   pooled[b,a,:] = sum_t att[b,t,a] vals[t,b,:]          vals [F,B,Hv] (row stride ld_vals), or absent (Hv = 0)
// pooled = (sum_t s v) / den is linear in the values once the sigmoids are known, so nothing waits for den.
//
// forward: a workgroup (4 waves) owns TCH = 32 frames of one video.  Phase 1: a wave takes 8 rows of src; per 64 VW columns it loads
//   the VW x A block of Wa once (contiguous in [Hs,A]) and the 8 rows' pieces, 8 independent loads in flight; one butterfly per (row, a);
//   lane r finishes row r: s into LDS and, unnormalised, into att.  Phase 2: the 256 threads split the columns of vals and walk the
//   chunk's unmasked rows, RB at a time, with A x VW accumulators per column piece.  The chunk's sum of s and its unnormalised pooled rows
//   go to the workspace; sigattn_fwd_finish_kernel adds the chunks in chunk order, writes den, divides att in place and writes pooled.
//   Rows past num_frames are neither loaded nor multiplied: the mask does the work, not the data.
// backward: G = dpooled [B,A,Hv], E = datt [B,F,A], either may be absent.
//   dt[t,b,a] = E[b,t,a] + vals[t,b,:] . G[b,a,:];   inner[b,a] = sum_t att dt = pooled[b,a,:] . G[b,a,:] + sum_t att E  (a pre-pass over
//   small tensors);   dz = (dt - inner) att (1 - sig),  sig = att den   ( = (dt - inner) / den sig (1 - sig) );
//   dvals[t,b,:] = sum_a att G[b,a,:];  dsrc[t,b,:] = sum_a dz Wa[:,a];  dWa[:,a] = sum_{t,b} src dz;  dba[a] = sum_{t,b} dz.
//   The same two phases: phase 1 reads vals once (the dot products with G, dvals written from the same registers), phase 2 reads src
//   once (dsrc written, dWa accumulated per thread).  Every row of dsrc and dvals is written, the padding rows as exact zeros without a
//   load.  A workgroup's dWa | dba partial goes to the workspace; two kernels add the partials, 32 at a time, in a fixed order.
// No atomics anywhere: a second run gives the same bits.  16-byte accesses (VW = 4) where every operand is 16-byte aligned and every
// leading dimension is a multiple of 4, single elements (VW = 1) otherwise.
#include <math.h>
#include "pooling_common.h"

namespace {

constexpr int TCH = 32;                    // frames per workgroup
constexpr int NW = 4;                      // waves per workgroup
constexpr int RPW = TCH / NW;              // rows per wave in phase 1
constexpr int RB = 4;                      // rows in flight per thread in phase 2
constexpr int HMAX = 2048;
constexpr int AMAX = 8;
constexpr float DEN_EPS = 1e-8f;

// common.h's clamp_frames in 32-bit arithmetic: through the 64-bit form the two kernels below compile to other instructions
__device__ __forceinline__ int clamp_frames_i32(const int32_t* nf, int b, int F) { return min(max(nf[b], 0), F); }

// grid (B, ceil(F / TCH)); den_p [chunks, B, A]; pool_p [chunks, B, A, Hv] (unused with Hv == 0)
template <int A, int VW>
__global__ __launch_bounds__(256) void sigattn_fwd_kernel(const float* __restrict__ src, size_t ld_src, const float* __restrict__ vals,
                                                          size_t ld_vals, const float* __restrict__ Wa, const float* __restrict__ ba,
                                                          const int32_t* __restrict__ nf, float* __restrict__ att,
                                                          float* __restrict__ den_p, float* __restrict__ pool_p, int F, int B, int Hs,
                                                          int Hv) {
  constexpr int KV = HMAX / (256 * VW);
  __shared__ float s_sh[TCH][A];
  const int b = blockIdx.x, c = blockIdx.y, t0 = c * TCH;
  const int rows = min(TCH, F - t0);                                      // frames of this chunk
  const int live = max(0, min(rows, clamp_frames_i32(nf, b, F) - t0));        // ... of which unmasked
  const int lane = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * RPW;
  float z[RPW][A];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int a = 0; a < A; ++a) z[r][a] = 0.0f;
  if (r0 < live) {                                                        // (wave-uniform)
    for (int h = lane * VW; h < Hs; h += 64 * VW) {
      float w[VW * A];                                                    // Wa[h .. h + VW, :]: VW A contiguous floats
      if constexpr (VW == 4) {
#pragma unroll
        for (int a = 0; a < A; ++a) {
          const float4 q = *reinterpret_cast<const float4*>(Wa + (size_t)h * A + 4 * a);
          w[4 * a] = q.x; w[4 * a + 1] = q.y; w[4 * a + 2] = q.z; w[4 * a + 3] = q.w;
        }
      } else {
#pragma unroll
        for (int a = 0; a < A; ++a) w[a] = Wa[(size_t)h * A + a];
      }
      float x[RPW][VW];
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        if (r0 + r < live) {
          ldv<VW>(src + ((size_t)(t0 + r0 + r) * B + b) * ld_src + h, x[r]);
        } else {
#pragma unroll
          for (int k = 0; k < VW; ++k) x[r][k] = 0.0f;
        }
      }
#pragma unroll
      for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int k = 0; k < VW; ++k)
#pragma unroll
          for (int a = 0; a < A; ++a) z[r][a] = fmaf(x[r][k], w[k * A + a], z[r][a]);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int a = 0; a < A; ++a) z[r][a] = wave_sum(z[r][a]);
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int t = r0 + r;
    if (lane == r && t < rows) {
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const float s = t < live ? sigmoidf_(z[r][a] + ba[a]) : 0.0f;
        s_sh[t][a] = s;
        att[((size_t)b * F + t0 + t) * A + a] = s;                        // unnormalised: the finishing kernel divides in place
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < A) {
    float d = 0.0f;
    for (int t = 0; t < rows; ++t) d += s_sh[t][threadIdx.x];
    den_p[((size_t)c * B + b) * A + threadIdx.x] = d;
  }
  if (Hv == 0) return;
  float acc[KV][A][VW];
#pragma unroll
  for (int k = 0; k < KV; ++k)
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
      for (int e = 0; e < VW; ++e) acc[k][a][e] = 0.0f;
  for (int t = 0; t < live; t += RB) {
    float v[RB][KV][VW];
#pragma unroll
    for (int rr = 0; rr < RB; ++rr)
#pragma unroll
      for (int k = 0; k < KV; ++k) {
        const int col = (k * 256 + threadIdx.x) * VW;
        if (t + rr < live && col < Hv) {
          ldv<VW>(vals + ((size_t)(t0 + t + rr) * B + b) * ld_vals + col, v[rr][k]);
        } else {
#pragma unroll
          for (int e = 0; e < VW; ++e) v[rr][k][e] = 0.0f;
        }
      }
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
      if (t + rr < live) {
#pragma unroll
        for (int a = 0; a < A; ++a) {
          const float s = s_sh[t + rr][a];
#pragma unroll
          for (int k = 0; k < KV; ++k)
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[k][a][e] = fmaf(s, v[rr][k][e], acc[k][a][e]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int col = (k * 256 + threadIdx.x) * VW;
    if (col < Hv) {
#pragma unroll
      for (int a = 0; a < A; ++a) stv<VW>(pool_p + (((size_t)c * B + b) * A + a) * Hv + col, acc[k][a]);
    }
  }
}

// grid (B): den = sum of the chunks in chunk order + eps; att /= den in place; pooled = (sum of the chunks) / den.  pooled may be null
__global__ __launch_bounds__(256) void sigattn_fwd_finish_kernel(const float* __restrict__ den_p, const float* __restrict__ pool_p,
                                                                 float* __restrict__ att, float* __restrict__ den,
                                                                 float* __restrict__ pooled, int F, int B, int Hv, int A, int chunks) {
  __shared__ float d_sh[AMAX];
  const int b = blockIdx.x;
  if ((int)threadIdx.x < A) {
    float d = 0.0f;
    for (int c = 0; c < chunks; ++c) d += den_p[((size_t)c * B + b) * A + threadIdx.x];
    d += DEN_EPS;
    d_sh[threadIdx.x] = d;
    den[(size_t)b * A + threadIdx.x] = d;
  }
  __syncthreads();
  float* arow = att + (size_t)b * F * A;
  for (int i = threadIdx.x; i < F * A; i += 256) arow[i] = arow[i] / d_sh[i % A];
  if (!pooled) return;
  const size_t AH = (size_t)A * Hv;
  for (int i = threadIdx.x; i < (int)AH; i += 256) {
    float r = 0.0f;
    for (int c = 0; c < chunks; ++c) r += pool_p[((size_t)c * B + b) * AH + i];
    pooled[(size_t)b * AH + i] = r / d_sh[i / Hv];
  }
}

// grid (B): inner[b,a] = pooled[b,a,:] . G[b,a,:] + sum_t att[b,t,a] E[b,t,a]; G (with pooled) and E may each be null
__global__ __launch_bounds__(256) void sigattn_inner_kernel(const float* __restrict__ att, const float* __restrict__ pooled,
                                                            const float* __restrict__ G, const float* __restrict__ E,
                                                            float* __restrict__ inner, int F, int Hv, int A) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  for (int a = 0; a < A; ++a) {
    float v = 0.0f;
    if (G) {
      const size_t o = ((size_t)b * A + a) * Hv;
      for (int i = threadIdx.x; i < Hv; i += 256) v = fmaf(pooled[o + i], G[o + i], v);
    }
    if (E) {
      for (int t = threadIdx.x; t < F; t += 256) {
        const size_t o = ((size_t)b * F + t) * A + a;
        v = fmaf(att[o], E[o], v);
      }
    }
    v = block_sum_256(v, red);
    if (threadIdx.x == 0) inner[(size_t)b * A + a] = v;
  }
}

// grid (B, ceil(F / TCH)); parts [B * chunks, Hs A + A] (null: neither dWa nor dba is wanted); G, E, dvals may be null
template <int A, int VW>
__global__ __launch_bounds__(256) void sigattn_bwd_kernel(const float* __restrict__ src, size_t ld_src, const float* __restrict__ vals,
                                                          size_t ld_vals, const float* __restrict__ Wa, const int32_t* __restrict__ nf,
                                                          const float* __restrict__ att, const float* __restrict__ den,
                                                          const float* __restrict__ G, const float* __restrict__ E,
                                                          const float* __restrict__ inner, float* __restrict__ dsrc, size_t ld_dsrc,
                                                          float* __restrict__ dvals, size_t ld_dvals, float* __restrict__ parts, int F,
                                                          int B, int Hs, int Hv) {
  constexpr int KV = HMAX / (256 * VW);
  __shared__ float a_sh[TCH][A], dz_sh[TCH][A];
  const int b = blockIdx.x, c = blockIdx.y, t0 = c * TCH;
  const int rows = min(TCH, F - t0);
  const int live = max(0, min(rows, clamp_frames_i32(nf, b, F) - t0));
  const int lane = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * RPW;
  for (int i = threadIdx.x; i < rows * A; i += 256) {
    const size_t o = ((size_t)b * F + t0) * A + i;
    a_sh[i / A][i % A] = att[o];
    dz_sh[i / A][i % A] = E ? E[o] : 0.0f;
  }
  __syncthreads();
  // phase 1: vals . G per row, dvals from the same registers
  float d[RPW][A];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int a = 0; a < A; ++a) d[r][a] = 0.0f;
  if (r0 < rows && Hv > 0 && (G || dvals)) {                              // (wave-uniform)
    for (int h = lane * VW; h < Hv; h += 64 * VW) {
      float g[A][VW];
#pragma unroll
      for (int a = 0; a < A; ++a) {
        if (G) {
          ldv<VW>(G + ((size_t)b * A + a) * Hv + h, g[a]);
        } else {
#pragma unroll
          for (int k = 0; k < VW; ++k) g[a][k] = 0.0f;
        }
      }
      float x[RPW][VW];
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        if (r0 + r < live && G) {
          ldv<VW>(vals + ((size_t)(t0 + r0 + r) * B + b) * ld_vals + h, x[r]);
        } else {
#pragma unroll
          for (int k = 0; k < VW; ++k) x[r][k] = 0.0f;
        }
      }
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const int t = r0 + r;
        float o[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) o[k] = 0.0f;
        if (t < live && G) {
#pragma unroll
          for (int a = 0; a < A; ++a) {
            const float w = a_sh[t][a];
#pragma unroll
            for (int k = 0; k < VW; ++k) {
              d[r][a] = fmaf(x[r][k], g[a][k], d[r][a]);
              o[k] = fmaf(w, g[a][k], o[k]);
            }
          }
        }
        if (dvals && t < rows) stv<VW>(dvals + ((size_t)(t0 + t) * B + b) * ld_dvals + h, o);
      }
    }
    if (G) {
#pragma unroll
      for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int a = 0; a < A; ++a) d[r][a] = wave_sum(d[r][a]);
    }
  }
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int t = r0 + r;
    if (lane == r && t < rows) {
#pragma unroll
      for (int a = 0; a < A; ++a) {
        float dz = 0.0f;
        if (t < live) {
          const float w = a_sh[t][a];
          const float sg = w * den[(size_t)b * A + a];
          dz = (dz_sh[t][a] + d[r][a] - inner[(size_t)b * A + a]) * w * (1.0f - sg);
        }
        dz_sh[t][a] = dz;
      }
    }
  }
  __syncthreads();
  // phase 2: dsrc = dz . Wa^T per row; the chunk's share of dWa = src^T dz
  float w[KV][VW * A], acc[KV][VW * A];
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int col = (k * 256 + threadIdx.x) * VW;
#pragma unroll
    for (int j = 0; j < VW * A; ++j) {
      w[k][j] = col < Hs ? Wa[(size_t)col * A + j] : 0.0f;
      acc[k][j] = 0.0f;
    }
  }
  for (int t = 0; t < rows; t += RB) {
    float x[RB][KV][VW];
#pragma unroll
    for (int rr = 0; rr < RB; ++rr)
#pragma unroll
      for (int k = 0; k < KV; ++k) {
        const int col = (k * 256 + threadIdx.x) * VW;
        if (t + rr < live && col < Hs) {
          ldv<VW>(src + ((size_t)(t0 + t + rr) * B + b) * ld_src + col, x[rr][k]);
        } else {
#pragma unroll
          for (int e = 0; e < VW; ++e) x[rr][k][e] = 0.0f;
        }
      }
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
      if (t + rr < rows) {
        float dz[A];
#pragma unroll
        for (int a = 0; a < A; ++a) dz[a] = dz_sh[t + rr][a];             // 0 on the padding rows
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          const int col = (k * 256 + threadIdx.x) * VW;
          if (col < Hs) {
            float o[VW];
#pragma unroll
            for (int e = 0; e < VW; ++e) {
              o[e] = 0.0f;
#pragma unroll
              for (int a = 0; a < A; ++a) {
                o[e] = fmaf(dz[a], w[k][e * A + a], o[e]);
                acc[k][e * A + a] = fmaf(x[rr][k][e], dz[a], acc[k][e * A + a]);
              }
            }
            if (t + rr >= live) {
#pragma unroll
              for (int e = 0; e < VW; ++e) o[e] = 0.0f;                   // exact zeros whatever Wa holds
            }
            stv<VW>(dsrc + ((size_t)(t0 + t + rr) * B + b) * ld_dsrc + col, o);
          }
        }
      }
    }
  }
  if (!parts) return;
  const size_t n = (size_t)Hs * A + A;
  float* p = parts + ((size_t)b * gridDim.y + c) * n;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int col = (k * 256 + threadIdx.x) * VW;
    if (col < Hs) {
#pragma unroll
      for (int j = 0; j < VW * A; ++j) p[(size_t)col * A + j] = acc[k][j];
    }
  }
  if (threadIdx.x < A) {
    float s = 0.0f;
    for (int t = 0; t < rows; ++t) s += dz_sh[t][threadIdx.x];
    p[(size_t)Hs * A + threadIdx.x] = s;
  }
}

inline bool shape_ok(int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t A) {
  return B >= 1 && B <= 65536 && F >= 1 && F <= 65536 && B * cdiv(F, TCH) <= (1 << 21) && Hs >= 4 && Hs <= HMAX && (Hs & 3) == 0 &&
         Hv >= 0 && Hv <= HMAX && (Hv & 3) == 0 && A >= 1 && A <= AMAX;
}

struct Layout {                              // the workspace, in floats; every offset a multiple of 4
  int64_t chunks, parts, groups, n;
  int64_t fwd_pool, fwd_total;               // forward: den partials at 0, pooled partials at fwd_pool
  int64_t bwd_parts, bwd_groups, bwd_total;  // backward: inner at 0, the workgroups' dWa | dba at bwd_parts, their group sums behind
  int64_t bytes;                             // one size for both directions
  Layout(int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t A) {
    chunks = cdiv(F, TCH);
    parts = B * chunks;
    groups = cdiv(parts, SUM_GROUP);
    n = Hs * A + A;
    fwd_pool = up4(chunks * B * A);
    fwd_total = fwd_pool + up4(chunks * B * A * Hv);
    bwd_parts = up4(B * A);
    bwd_groups = bwd_parts + up4(parts * n);
    bwd_total = bwd_groups + up4(groups * n);
    bytes = (fwd_total > bwd_total ? fwd_total : bwd_total) * (int64_t)sizeof(float);
  }
};

template <int A>
void launch_fwd(bool vec, const float* src, int64_t ld_src, const float* vals, int64_t ld_vals, const float* Wa, const float* ba,
                const int32_t* nf, float* att, float* den_p, float* pool_p, int F, int B, int Hs, int Hv, hipStream_t s) {
  const dim3 grid((unsigned)B, (unsigned)cdiv(F, TCH)), block(256);
  if (vec)
    hipLaunchKernelGGL((sigattn_fwd_kernel<A, 4>), grid, block, 0, s, src, (size_t)ld_src, vals, (size_t)ld_vals, Wa, ba, nf, att, den_p,
                       pool_p, F, B, Hs, Hv);
  else
    hipLaunchKernelGGL((sigattn_fwd_kernel<A, 1>), grid, block, 0, s, src, (size_t)ld_src, vals, (size_t)ld_vals, Wa, ba, nf, att, den_p,
                       pool_p, F, B, Hs, Hv);
}

template <int A>
void launch_bwd(bool vec, const float* src, int64_t ld_src, const float* vals, int64_t ld_vals, const float* Wa, const int32_t* nf,
                const float* att, const float* den, const float* G, const float* E, const float* inner, float* dsrc, int64_t ld_dsrc,
                float* dvals, int64_t ld_dvals, float* parts, int F, int B, int Hs, int Hv, hipStream_t s) {
  const dim3 grid((unsigned)B, (unsigned)cdiv(F, TCH)), block(256);
  if (vec)
    hipLaunchKernelGGL((sigattn_bwd_kernel<A, 4>), grid, block, 0, s, src, (size_t)ld_src, vals, (size_t)ld_vals, Wa, nf, att, den, G, E,
                       inner, dsrc, (size_t)ld_dsrc, dvals, (size_t)ld_dvals, parts, F, B, Hs, Hv);
  else
    hipLaunchKernelGGL((sigattn_bwd_kernel<A, 1>), grid, block, 0, s, src, (size_t)ld_src, vals, (size_t)ld_vals, Wa, nf, att, den, G, E,
                       inner, dsrc, (size_t)ld_dsrc, dvals, (size_t)ld_dvals, parts, F, B, Hs, Hv);
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_sigattn_supported(int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t A) { return shape_ok(B, F, Hs, Hv, A) ? 1 : 0; }

extern "C" int64_t yt8m_sigattn_workspace_bytes(int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t A) {
  if (!shape_ok(B, F, Hs, Hv, A)) return -1;
  return Layout(B, F, Hs, Hv, A).bytes;
}

extern "C" int yt8m_sigattn_fwd(const float* src, int64_t ld_src, const float* vals, int64_t ld_vals, const float* Wa, const float* ba,
                                const int32_t* num_frames, float* att, float* den, float* pooled, void* workspace,
                                int64_t workspace_bytes, int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t A, yt8m_stream_t stream) {
  YT8M_REQUIRE(shape_ok(B, F, Hs, Hv, A), YT8M_E_SHAPE, "a shape yt8m_sigattn_supported refuses");
  YT8M_REQUIRE(src && Wa && ba && num_frames && att && den, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE((Hv > 0) == (vals != nullptr) && (Hv > 0) == (pooled != nullptr), YT8M_E_BADARG, "vals and pooled go with Hv > 0");
  YT8M_REQUIRE(ld_src >= Hs && (Hv == 0 || ld_vals >= Hv), YT8M_E_BADARG, "a leading dimension below its width");
  const Layout L(B, F, Hs, Hv, A);
  YT8M_REQUIRE(workspace && workspace_bytes >= L.bytes, YT8M_E_BADARG,
               "workspace smaller than yt8m_sigattn_workspace_bytes");
  float* den_p = static_cast<float*>(workspace);
  float* pool_p = den_p + L.fwd_pool;
  const bool vec = aligned16(src) && aligned16(Wa) && aligned16(workspace) && (ld_src & 3) == 0 &&
                   (Hv == 0 || (aligned16(vals) && (ld_vals & 3) == 0));
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int b = (int)B, f = (int)F, hs = (int)Hs, hv = (int)Hv;
#define SIGATTN_FWD(AA) launch_fwd<AA>(vec, src, ld_src, vals, ld_vals, Wa, ba, num_frames, att, den_p, pool_p, f, b, hs, hv, s);
  YT8M_BY_HEADS(A, SIGATTN_FWD)
#undef SIGATTN_FWD
  int st = launch_status("sigattn_fwd_kernel");
  if (st != YT8M_OK) return st;
  hipLaunchKernelGGL(sigattn_fwd_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, den_p, pool_p, att, den, pooled, f, b, hv, (int)A,
                     (int)L.chunks);
  return launch_status("sigattn_fwd_finish_kernel");
}

extern "C" int yt8m_sigattn_bwd(const float* src, int64_t ld_src, const float* vals, int64_t ld_vals, const float* Wa,
                                const int32_t* num_frames, const float* att, const float* den, const float* pooled, const float* G,
                                const float* E, float* dsrc, int64_t ld_dsrc, float* dvals, int64_t ld_dvals, float* dWa, float* dba,
                                void* workspace, int64_t workspace_bytes, int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t A,
                                yt8m_stream_t stream) {
  YT8M_REQUIRE(shape_ok(B, F, Hs, Hv, A), YT8M_E_SHAPE, "a shape yt8m_sigattn_supported refuses");
  YT8M_REQUIRE(src && Wa && num_frames && att && den && dsrc, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(Hv > 0 || (!G && !dvals), YT8M_E_BADARG, "G and dvals go with Hv > 0");
  YT8M_REQUIRE(!G || (vals && pooled), YT8M_E_BADARG, "G needs vals and pooled");
  YT8M_REQUIRE(ld_src >= Hs && ld_dsrc >= Hs && (!G || ld_vals >= Hv) && (!dvals || ld_dvals >= Hv), YT8M_E_BADARG,
               "a leading dimension below its width");
  const Layout L(B, F, Hs, Hv, A);
  YT8M_REQUIRE(workspace && workspace_bytes >= L.bytes, YT8M_E_BADARG,
               "workspace smaller than yt8m_sigattn_workspace_bytes");
  float* inner = static_cast<float*>(workspace);
  float* parts = (dWa || dba) ? static_cast<float*>(workspace) + L.bwd_parts : nullptr;
  float* groups = static_cast<float*>(workspace) + L.bwd_groups;
  const bool vec = aligned16(src) && aligned16(dsrc) && (ld_src & 3) == 0 && (ld_dsrc & 3) == 0 &&
                   (!G || (aligned16(G) && aligned16(vals) && (ld_vals & 3) == 0)) && (!dvals || (aligned16(dvals) && (ld_dvals & 3) == 0));
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int b = (int)B, f = (int)F, hs = (int)Hs, hv = (int)Hv;
  hipLaunchKernelGGL(sigattn_inner_kernel, dim3((unsigned)B), dim3(256), 0, s, att, pooled, G, E, inner, f, hv, (int)A);
  int st = launch_status("sigattn_inner_kernel");
  if (st != YT8M_OK) return st;
#define SIGATTN_BWD(AA) \
  launch_bwd<AA>(vec, src, ld_src, vals, ld_vals, Wa, num_frames, att, den, G, E, inner, dsrc, ld_dsrc, dvals, ld_dvals, parts, f, b, hs, hv, s);
  YT8M_BY_HEADS(A, SIGATTN_BWD)
#undef SIGATTN_BWD
  st = launch_status("sigattn_bwd_kernel");
  if (st != YT8M_OK || !parts) return st;
  return sum_parts(parts, groups, (int)L.n, (int)L.parts, dWa, (int)(Hs * A), dba, s);
}
