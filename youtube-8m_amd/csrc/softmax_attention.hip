// softmax_attention.hip -- the windowed softmax attention pooling of Z/frame_level_models.py:5218-5223 (LstmExtendModel) and :6059-6064
// (InputExtendModel) on the TIME-major tensors the LSTM stack leaves (gfx950, wave64; src and vals are 157 MB each at F = 300,
// B = 128, H = 1024).  Per head e of E:
//   z[t,b,e]      = src[t,b,:] . W1[:,e] + b1[e] + extra[b,t,e]      src [F,B,Hs] (row stride ld_src), W1 [Hs,E], extra [B,F,E] or absent
//   m[t,b,e]      = valid[b,t] (lo[b,e] <= t <= hi[b,e])             valid uint8 [B,F], lo / hi int32 [B,E] inclusive; each may be absent
//   att[b,t,e]    = m exp(z - M[b,e]) / sum_t' m exp(z[t'] - M[b,e]),  M[b,e] = max of z over the frames with m = 1   (att is [B,F,E])
//   pooled[b,e,:] = sum_t att[b,t,e] vals[t,b,:]                     vals [F,B,Hv] (row stride ld_vals); vals == src is the SHARED mode
// The reference writes softmax over all F frames, times the mask, divided by its sum; this is the same function and stays finite where
// that form underflows to 0 / 0.  A (b, e) with no unmasked frame gets att = 0 and pooled = 0 and neither receives nor sends a gradient.
//
// forward: a workgroup (4 waves) owns TCH = 64 frames of one video (32, as the sigmoid kernel takes, would double the pooled partials,
//   which are E times a row wide: 42 MB written and read back at E = 8 against the 157 MB of the rows).  Wave 0 makes the rows' head
//   masks; its one ballot says which rows any head unmasks: the others are never loaded.  Phase 1: a wave takes 8 rows of src at a
//   time; per 64 VW columns it loads the VW x E block of W1 once and the rows' pieces, 8 independent loads in flight; one butterfly per
//   (row, e); lane r finishes row r: z into LDS and into att.  Thread e then takes the chunk's max m_c over head e's unmasked rows,
//   turns z into exp(z - m_c) in LDS and adds them up to l_c.  Phase 2: the 256 threads split the columns of vals and walk the chunk's
//   unmasked rows, RB at a time, a column piece at a time, with E x VW accumulators and compensated sums.  m_c, l_c and the
//   unnormalised pooled rows go to the workspace; smattn_fwd_finish_kernel, a workgroup per (video, head), walks the chunks in chunk
//   order: M = max m_c, L = sum l_c exp(m_c - M), pooled = sum p_c exp(m_c - M) / L, and att is rewritten in place as m exp(z - M) / L.
//   A chunk without an unmasked frame for a head has l_c = 0 and is skipped, so exp(-inf - -inf) is never formed.
//   In the shared mode phase 2 reads again the 64 rows that phase 1 of the same workgroup has just read (256 KB at H = 1024): one
//   tensor is walked, not two, but the rows are NOT kept in registers or LDS between the phases; the second read follows the first
//   within one workgroup's lifetime and is left to the caches (L2, the memory-side cache).  How much of it they serve was not measured.
// backward, from G = dpooled [B,E,Hv] alone (att is not differentiable here):
//   dz[t,e] = att ((vals[t,b,:] - pooled[b,e,:]) . G[b,e,:])  ( = att (dt - inner), dt = vals . G, inner = pooled . G = sum_t att dt: the
//   difference is taken per element, before the sum, so a frame that holds all of a head's weight -- vals = pooled -- gets dz = 0 exactly
//   and the rounding of two long dot products of the size of 4 sqrt(Hv) never meets);
//   dsrc[t,b,:] = sum_e dz W1[:,e];  dvals[t,b,:] = sum_e att G[b,e,:];  dW1 = sum_{t,b} src dz;  dextra = dz;
//   db1 = sum_{t,b} dz = 0: b1[e] moves every logit of head e alike and a softmax does not see that (sum_t att (dt - inner) = inner -
//   inner), so db1 is written as exact zeros -- a float32 sum of dz would put rounding noise of the size of 1e-5 in its place.
//   A workgroup owns BT = 64 frames of one video (half the dW1 partials of 32: 21 MB at E = 8, H = 1024, B = 128, F = 300).  Phase 1
//   reads vals once (the dot products with G, dvals written from the same registers), phase 2 reads src once (dsrc written, dW1
//   accumulated per thread), a column piece at a time.  In the shared mode there is ONE gradient tensor: phase 2 writes sum_e dz
//   W1[:,e] + sum_e att G[b,e,:] into dsrc and phase 1 writes nothing; one tensor is read (phase 2 re-reads the workgroup's 64 rows as
//   in the forward) and one is written, each row once.  Every row of dsrc, dvals and dextra is written, the rows no head unmasks as
//   exact zeros without a load.  A workgroup's share of dW1 goes to the workspace; two kernels add the shares, 32 at a time, in a
//   fixed order.
// No atomics anywhere: a second run gives the same bits.  16-byte accesses (VW = 4) where every operand is 16-byte aligned and every
// leading dimension is a multiple of 4, single elements (VW = 1) otherwise.
#include <math.h>
#include "pooling_common.h"

namespace {

constexpr int TCH = 64;                    // frames per workgroup, forward (one wave's ballot)
constexpr int BT = 64;                     // frames per workgroup, backward (one wave's ballot)
constexpr int NW = 4;                      // waves per workgroup
constexpr int RPW = 8;                     // rows per wave and batch in phase 1
constexpr int RB = 4;                      // rows in flight per thread in phase 2
constexpr int HMAX = 2048;
constexpr int EMAX = 8;

// head e's window of video b clamped to the frames there are: [max(lo, 0), min(hi, F - 1)], empty where the first exceeds the second
__device__ __forceinline__ void window(const int32_t* lo, const int32_t* hi, int b, int e, int E, int F, int& l, int& h) {
  l = lo ? max(lo[(size_t)b * E + e], 0) : 0;
  h = hi ? min(hi[(size_t)b * E + e], F - 1) : F - 1;
}

// bit e: m[t,b,e]
template <int E>
__device__ __forceinline__ unsigned head_mask(const uint8_t* valid, const int32_t* lo, const int32_t* hi, int b, int t, int F) {
  if (valid && !valid[(size_t)b * F + t]) return 0u;
  unsigned bits = 0u;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    int l, h;
    window(lo, hi, b, e, E, F, l, h);
    if (l <= t && t <= h) bits |= 1u << e;
  }
  return bits;
}

// grid (B, ceil(F / TCH)); m_p, l_p [chunks, B, E]; pool_p [chunks, B, E, Hv]
template <int E, int VW>
__global__ __launch_bounds__(256) void smattn_fwd_kernel(const float* __restrict__ src, size_t ld_src, const float* vals, size_t ld_vals,
                                                         const float* __restrict__ W1, const float* __restrict__ b1,
                                                         const float* __restrict__ extra, const uint8_t* __restrict__ valid,
                                                         const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                         float* __restrict__ att, float* __restrict__ m_p, float* __restrict__ l_p,
                                                         float* __restrict__ pool_p, int F, int B, int Hs, int Hv) {
  constexpr int KV = HMAX / (256 * VW);
  __shared__ float p_sh[TCH][E];
  __shared__ unsigned mask_sh[TCH];
  __shared__ unsigned long long live_sh;
  const int b = blockIdx.x, c = blockIdx.y, t0 = c * TCH;
  const int rows = min(TCH, F - t0);                                      // frames of this chunk
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 64) {                                                 // (TCH is one wave's ballot)
    const unsigned bits = (int)threadIdx.x < rows ? head_mask<E>(valid, lo, hi, b, t0 + threadIdx.x, F) : 0u;
    mask_sh[threadIdx.x] = bits;
    const unsigned long long any = __ballot(bits != 0u);
    if (threadIdx.x == 0) live_sh = any;
  }
  __syncthreads();
  const unsigned long long live = live_sh;                                // bit t: some head unmasks row t of the chunk
  for (int r0 = wave * RPW; r0 < rows; r0 += NW * RPW) {                  // (wave-uniform)
    float z[RPW][E];
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int e = 0; e < E; ++e) z[r][e] = 0.0f;
    if ((live >> r0) & 0xffull) {
      for (int h = lane * VW; h < Hs; h += 64 * VW) {
        float w[VW * E];                                                  // W1[h .. h + VW, :]: VW E contiguous floats
        if constexpr (VW == 4) {
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const float4 q = *reinterpret_cast<const float4*>(W1 + (size_t)h * E + 4 * e);
            w[4 * e] = q.x; w[4 * e + 1] = q.y; w[4 * e + 2] = q.z; w[4 * e + 3] = q.w;
          }
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) w[e] = W1[(size_t)h * E + e];
        }
        float x[RPW][VW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          if ((live >> (r0 + r)) & 1ull) {
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
            for (int e = 0; e < E; ++e) z[r][e] = fmaf(x[r][k], w[k * E + e], z[r][e]);
      }
#pragma unroll
      for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e) z[r][e] = wave_sum(z[r][e]);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int t = r0 + r;
      if (lane == r && t < rows) {
        const size_t o = ((size_t)b * F + t0 + t) * E;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float zz = z[r][e] + b1[e] + (extra ? extra[o + e] : 0.0f);
          p_sh[t][e] = zz;
          att[o + e] = zz;                                                // the logit: the finishing kernel rewrites it in place
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < E) {
    const int e = threadIdx.x;
    float m = -INFINITY;
    for (int t = 0; t < rows; ++t)
      if ((mask_sh[t] >> e) & 1u) m = fmaxf(m, p_sh[t][e]);
    float l = 0.0f;
    for (int t = 0; t < rows; ++t) {
      const float p = ((mask_sh[t] >> e) & 1u) ? expf(p_sh[t][e] - m) : 0.0f;
      p_sh[t][e] = p;
      l += p;
    }
    m_p[((size_t)c * B + b) * E + e] = l > 0.0f ? m : 0.0f;               // l = 0: a chunk without an unmasked frame for this head
    l_p[((size_t)c * B + b) * E + e] = l;
  }
  __syncthreads();
  // phase 2, a column piece at a time.  The sums are compensated (Kahan): the backward takes (vals - pooled) . G, where what 64 plain
  // float32 additions lose in pooled, a few 1e-7 of it, comes back times sqrt(Hv) |G| in every dz of the head, with one sign, and does
  // not average out of the sums over the frames (dW1, and the plugins' gradient of b2 through dextra)
  const int tlo = live ? __builtin_ctzll(live) : 0, thi = live ? 64 - __builtin_clzll(live) : 0;
  for (int k = 0; k < KV; ++k) {
    const int col = (k * 256 + threadIdx.x) * VW;
    if (col >= Hv) break;
    float acc[E][VW], lost[E][VW];
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
      for (int j = 0; j < VW; ++j) acc[e][j] = lost[e][j] = 0.0f;
    for (int t = tlo; t < thi; t += RB) {
      float v[RB][VW];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        if (t + rr < thi && ((live >> (t + rr)) & 1ull)) {
          ldv<VW>(vals + ((size_t)(t0 + t + rr) * B + b) * ld_vals + col, v[rr]);
        } else {
#pragma unroll
          for (int j = 0; j < VW; ++j) v[rr][j] = 0.0f;
        }
      }
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        if (t + rr < thi && ((live >> (t + rr)) & 1ull)) {
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const float p = p_sh[t + rr][e];
#pragma unroll
            for (int j = 0; j < VW; ++j) {
              const float y = fmaf(p, v[rr][j], -lost[e][j]);
              const float s = acc[e][j] + y;
              lost[e][j] = (s - acc[e][j]) - y;
              acc[e][j] = s;
            }
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) stv<VW>(pool_p + (((size_t)c * B + b) * E + e) * Hv + col, acc[e]);
  }
}

// grid (B, E), a workgroup per video and head: the chunks in chunk order.  M = max m_c and L = sum l_c exp(m_c - M) over the chunks with
// l_c > 0; att = m exp(z - M) / L in place; pooled = (sum p_c exp(m_c - M)) / L.  L = 0 (no unmasked frame): att = 0, pooled = 0.  Every
// load in the chunk loops is unconditional (an empty chunk wrote m_c = 0 and zeros), so that they do not wait for one another
__global__ __launch_bounds__(256) void smattn_fwd_finish_kernel(const float* __restrict__ m_p, const float* __restrict__ l_p,
                                                                const float* __restrict__ pool_p, const uint8_t* __restrict__ valid,
                                                                const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                                float* __restrict__ att, float* __restrict__ pooled, int F, int B, int Hv,
                                                                int E, int chunks) {
  __shared__ float M_sh, L_sh;
  __shared__ int lo_sh, hi_sh;
  const int b = blockIdx.x, e = blockIdx.y;
  if (threadIdx.x == 0) {
    float M = -INFINITY, L = 0.0f;
    for (int c = 0; c < chunks; ++c) {
      const size_t o = ((size_t)c * B + b) * E + e;
      const float l = l_p[o], m = m_p[o];
      if (l > 0.0f) M = fmaxf(M, m);
    }
    for (int c = 0; c < chunks; ++c) {
      const size_t o = ((size_t)c * B + b) * E + e;
      const float l = l_p[o], m = m_p[o];
      if (l > 0.0f) L += l * expf(m - M);
    }
    M_sh = L > 0.0f ? M : 0.0f;
    L_sh = L;
    window(lo, hi, b, e, E, F, lo_sh, hi_sh);
  }
  __syncthreads();
  const float M = M_sh, L = L_sh;
  const int wl = lo_sh, wh = hi_sh;
  for (int t = threadIdx.x; t < F; t += 256) {
    const size_t o = ((size_t)b * F + t) * E + e;
    const bool on = L > 0.0f && wl <= t && t <= wh && (!valid || valid[(size_t)b * F + t]);
    att[o] = on ? expf(att[o] - M) / L : 0.0f;
  }
  for (int i = threadIdx.x; i < Hv; i += 256) {
    float r = 0.0f;
    if (L > 0.0f) {
      for (int c = 0; c < chunks; ++c) {
        const size_t o = ((size_t)c * B + b) * E + e;
        const float l = l_p[o], m = m_p[o], pc = pool_p[o * Hv + i];
        r = fmaf(pc, l > 0.0f ? expf(m - M) : 0.0f, r);
      }
      r = r / L;
    }
    pooled[((size_t)b * E + e) * Hv + i] = r;
  }
}

// grid (B, ceil(F / BT)); parts [B * gridDim.y, Hs E] (null: dW1 is not wanted); dvals (null in the shared mode) and
// dextra may be null.  SHARED: vals == src, dsrc takes both gradients
template <int E, int VW, bool SHARED>
__global__ __launch_bounds__(256) void smattn_bwd_kernel(const float* __restrict__ src, size_t ld_src, const float* vals, size_t ld_vals,
                                                         const float* __restrict__ W1, const uint8_t* __restrict__ valid,
                                                         const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                         const float* __restrict__ att, const float* __restrict__ pooled,
                                                         const float* __restrict__ G, float* __restrict__ dsrc, size_t ld_dsrc,
                                                         float* __restrict__ dvals, size_t ld_dvals, float* __restrict__ dextra,
                                                         float* __restrict__ parts, int F, int B, int Hs, int Hv) {
  constexpr int KV = HMAX / (256 * VW);
  __shared__ float a_sh[BT][E], dz_sh[BT][E];
  __shared__ unsigned mask_sh[BT];
  __shared__ unsigned long long live_sh;
  const int b = blockIdx.x, c = blockIdx.y, t0 = c * BT;
  const int rows = min(BT, F - t0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 64) {
    const unsigned bits = (int)threadIdx.x < rows ? head_mask<E>(valid, lo, hi, b, t0 + threadIdx.x, F) : 0u;
    mask_sh[threadIdx.x] = bits;
    const unsigned long long any = __ballot(bits != 0u);
    if (threadIdx.x == 0) live_sh = any;
  }
  for (int i = threadIdx.x; i < rows * E; i += 256) a_sh[i / E][i % E] = att[((size_t)b * F + t0) * E + i];
  __syncthreads();
  const unsigned long long live = live_sh;                                // bit t: some head unmasks row t of the workgroup's frames
  // phase 1: (vals - pooled) . G per row and head, dvals from the same registers; lane r of a wave finishes its row r: dz, dextra
  for (int r0 = wave * RPW; r0 < rows; r0 += NW * RPW) {                  // (wave-uniform)
    float d[RPW][E];
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int e = 0; e < E; ++e) d[r][e] = 0.0f;
    const bool any_live = ((live >> r0) & 0xffull) != 0;
    if (any_live || (!SHARED && dvals)) {
      for (int h = lane * VW; h < Hv; h += 64 * VW) {
        float g[E][VW], pl[E][VW];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          ldv<VW>(G + ((size_t)b * E + e) * Hv + h, g[e]);
          ldv<VW>(pooled + ((size_t)b * E + e) * Hv + h, pl[e]);
        }
        float x[RPW][VW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          if ((live >> (r0 + r)) & 1ull) {
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
          if ((live >> t) & 1ull) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const float w = a_sh[t][e];
#pragma unroll
              for (int k = 0; k < VW; ++k) {
                d[r][e] = fmaf(x[r][k] - pl[e][k], g[e][k], d[r][e]);     // (vals - pooled) . G: the difference first
                o[k] = fmaf(w, g[e][k], o[k]);
              }
            }
          }
          if constexpr (!SHARED) {
            if (dvals && t < rows) stv<VW>(dvals + ((size_t)(t0 + t) * B + b) * ld_dvals + h, o);
          }
        }
      }
      if (any_live) {
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
          for (int e = 0; e < E; ++e) d[r][e] = wave_sum(d[r][e]);
      }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int t = r0 + r;
      if (lane == r && t < rows) {
        const unsigned bits = mask_sh[t];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float dz = ((bits >> e) & 1u) ? a_sh[t][e] * d[r][e] : 0.0f;
          dz_sh[t][e] = dz;
          if (dextra) dextra[((size_t)b * F + t0 + t) * E + e] = dz;
        }
      }
    }
  }
  __syncthreads();
  // phase 2, a column piece at a time: dsrc = dz . W1^T (+ att . G in the shared mode) per row; the workgroup's share of dW1 = src^T dz
  float* p = parts ? parts + ((size_t)b * gridDim.y + c) * ((size_t)Hs * E) : nullptr;
  for (int k = 0; k < KV; ++k) {
    const int col = (k * 256 + threadIdx.x) * VW;
    if (col >= Hs) break;
    float w[VW * E], acc[VW * E], g[E][VW];
#pragma unroll
    for (int j = 0; j < VW * E; ++j) {
      w[j] = W1[(size_t)col * E + j];
      acc[j] = 0.0f;
    }
    if constexpr (SHARED) {
#pragma unroll
      for (int e = 0; e < E; ++e) ldv<VW>(G + ((size_t)b * E + e) * Hv + col, g[e]);
    }
    for (int t = 0; t < rows; t += RB) {
      float x[RB][VW];
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        if (t + rr < rows && ((live >> (t + rr)) & 1ull)) {
          ldv<VW>(src + ((size_t)(t0 + t + rr) * B + b) * ld_src + col, x[rr]);
        } else {
#pragma unroll
          for (int j = 0; j < VW; ++j) x[rr][j] = 0.0f;
        }
      }
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        if (t + rr < rows) {
          float o[VW];
#pragma unroll
          for (int j = 0; j < VW; ++j) o[j] = 0.0f;
          if ((live >> (t + rr)) & 1ull) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const float dz = dz_sh[t + rr][e];
#pragma unroll
              for (int j = 0; j < VW; ++j) {
                o[j] = fmaf(dz, w[j * E + e], o[j]);
                acc[j * E + e] = fmaf(x[rr][j], dz, acc[j * E + e]);
              }
              if constexpr (SHARED) {
                const float a = a_sh[t + rr][e];
#pragma unroll
                for (int j = 0; j < VW; ++j) o[j] = fmaf(a, g[e][j], o[j]);
              }
            }
          }
          stv<VW>(dsrc + ((size_t)(t0 + t + rr) * B + b) * ld_dsrc + col, o);      // exact zeros on the rows no head unmasks
        }
      }
    }
    if (p) {
#pragma unroll
      for (int j = 0; j < VW * E; ++j) p[(size_t)col * E + j] = acc[j];
    }
  }
}

inline bool shape_ok(int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t E) {
  return B >= 1 && B <= 65536 && F >= 1 && F <= 65536 && B * cdiv(F, 32) <= (1 << 21) && Hs >= 4 && Hs <= HMAX && (Hs & 3) == 0 &&
         Hv >= 4 && Hv <= HMAX && (Hv & 3) == 0 && E >= 1 && E <= EMAX;
}

struct Layout {                              // the workspace, in floats; every offset a multiple of 4
  int64_t chunks, parts, groups, n;
  int64_t fwd_l, fwd_pool, fwd_total;        // forward: m_c at 0, l_c at fwd_l, pooled partials at fwd_pool
  int64_t bwd_parts, bwd_groups, bwd_total;  // backward: the workgroups' shares of dW1 at bwd_parts, their group sums behind
  int64_t bytes;                             // one size for both directions
  Layout(int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t E) {
    chunks = cdiv(F, TCH);
    parts = B * cdiv(F, BT);
    groups = cdiv(parts, SUM_GROUP);
    n = Hs * E;
    fwd_l = up4(chunks * B * E);
    fwd_pool = 2 * fwd_l;
    fwd_total = fwd_pool + up4(chunks * B * E * Hv);
    bwd_parts = 0;
    bwd_groups = bwd_parts + up4(parts * n);
    bwd_total = bwd_groups + up4(groups * n);
    bytes = (fwd_total > bwd_total ? fwd_total : bwd_total) * (int64_t)sizeof(float);
  }
};

template <int E>
void launch_fwd(bool vec, const float* src, int64_t ld_src, const float* vals, int64_t ld_vals, const float* W1, const float* b1,
                const float* extra, const uint8_t* valid, const int32_t* lo, const int32_t* hi, float* att, float* m_p, float* l_p,
                float* pool_p, int F, int B, int Hs, int Hv, hipStream_t s) {
  const dim3 grid((unsigned)B, (unsigned)cdiv(F, TCH)), block(256);
  if (vec)
    hipLaunchKernelGGL((smattn_fwd_kernel<E, 4>), grid, block, 0, s, src, (size_t)ld_src, vals, (size_t)ld_vals, W1, b1, extra, valid, lo,
                       hi, att, m_p, l_p, pool_p, F, B, Hs, Hv);
  else
    hipLaunchKernelGGL((smattn_fwd_kernel<E, 1>), grid, block, 0, s, src, (size_t)ld_src, vals, (size_t)ld_vals, W1, b1, extra, valid, lo,
                       hi, att, m_p, l_p, pool_p, F, B, Hs, Hv);
}

template <int E, bool SHARED>
void launch_bwd(bool vec, const float* src, int64_t ld_src, const float* vals, int64_t ld_vals, const float* W1, const uint8_t* valid,
                const int32_t* lo, const int32_t* hi, const float* att, const float* pooled, const float* G, float* dsrc, int64_t ld_dsrc,
                float* dvals, int64_t ld_dvals, float* dextra, float* parts, int F, int B, int Hs, int Hv, hipStream_t s) {
  const dim3 grid((unsigned)B, (unsigned)cdiv(F, BT)), block(256);
  if (vec)
    hipLaunchKernelGGL((smattn_bwd_kernel<E, 4, SHARED>), grid, block, 0, s, src, (size_t)ld_src, vals, (size_t)ld_vals, W1, valid, lo, hi,
                       att, pooled, G, dsrc, (size_t)ld_dsrc, dvals, (size_t)ld_dvals, dextra, parts, F, B, Hs, Hv);
  else
    hipLaunchKernelGGL((smattn_bwd_kernel<E, 1, SHARED>), grid, block, 0, s, src, (size_t)ld_src, vals, (size_t)ld_vals, W1, valid, lo, hi,
                       att, pooled, G, dsrc, (size_t)ld_dsrc, dvals, (size_t)ld_dvals, dextra, parts, F, B, Hs, Hv);
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_smattn_supported(int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t E) { return shape_ok(B, F, Hs, Hv, E) ? 1 : 0; }

extern "C" int64_t yt8m_smattn_workspace_bytes(int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t E) {
  if (!shape_ok(B, F, Hs, Hv, E)) return -1;
  return Layout(B, F, Hs, Hv, E).bytes;
}

extern "C" int yt8m_smattn_fwd(const float* src, int64_t ld_src, const float* vals, int64_t ld_vals, const float* W1, const float* b1,
                               const float* extra, const uint8_t* valid, const int32_t* lo, const int32_t* hi, float* att, float* pooled,
                               void* workspace, int64_t workspace_bytes, int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t E,
                               yt8m_stream_t stream) {
  YT8M_REQUIRE(shape_ok(B, F, Hs, Hv, E), YT8M_E_SHAPE, "a shape yt8m_smattn_supported refuses");
  YT8M_REQUIRE(src && vals && W1 && b1 && att && pooled, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(ld_src >= Hs && ld_vals >= Hv, YT8M_E_BADARG, "a leading dimension below its width");
  YT8M_REQUIRE(vals != src || (Hv == Hs && ld_vals == ld_src), YT8M_E_BADARG, "the shared mode (vals == src) wants Hv == Hs, ld_vals == ld_src");
  const Layout L(B, F, Hs, Hv, E);
  YT8M_REQUIRE(workspace && workspace_bytes >= L.bytes, YT8M_E_BADARG, "workspace smaller than yt8m_smattn_workspace_bytes");
  float* m_p = static_cast<float*>(workspace);
  float* l_p = m_p + L.fwd_l;
  float* pool_p = m_p + L.fwd_pool;
  const bool vec = aligned16(src) && aligned16(vals) && aligned16(W1) && aligned16(workspace) && (ld_src & 3) == 0 && (ld_vals & 3) == 0;
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int b = (int)B, f = (int)F, hs = (int)Hs, hv = (int)Hv;
#define SMATTN_FWD(EE) launch_fwd<EE>(vec, src, ld_src, vals, ld_vals, W1, b1, extra, valid, lo, hi, att, m_p, l_p, pool_p, f, b, hs, hv, s);
  YT8M_BY_HEADS(E, SMATTN_FWD)
#undef SMATTN_FWD
  int st = launch_status("smattn_fwd_kernel");
  if (st != YT8M_OK) return st;
  hipLaunchKernelGGL(smattn_fwd_finish_kernel, dim3((unsigned)B, (unsigned)E), dim3(256), 0, s, m_p, l_p, pool_p, valid, lo, hi, att, pooled, f, b, hv,
                     (int)E, (int)L.chunks);
  return launch_status("smattn_fwd_finish_kernel");
}

extern "C" int yt8m_smattn_bwd(const float* src, int64_t ld_src, const float* vals, int64_t ld_vals, const float* W1, const uint8_t* valid,
                               const int32_t* lo, const int32_t* hi, const float* att, const float* pooled, const float* G, float* dsrc,
                               int64_t ld_dsrc, float* dvals, int64_t ld_dvals, float* dW1, float* db1, float* dextra, void* workspace,
                               int64_t workspace_bytes, int64_t B, int64_t F, int64_t Hs, int64_t Hv, int64_t E, yt8m_stream_t stream) {
  YT8M_REQUIRE(shape_ok(B, F, Hs, Hv, E), YT8M_E_SHAPE, "a shape yt8m_smattn_supported refuses");
  YT8M_REQUIRE(src && vals && W1 && att && pooled && G && dsrc, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(ld_src >= Hs && ld_vals >= Hv && ld_dsrc >= Hs && (!dvals || ld_dvals >= Hv), YT8M_E_BADARG,
               "a leading dimension below its width");
  const bool shared = vals == src;
  YT8M_REQUIRE(!shared || (Hv == Hs && ld_vals == ld_src && !dvals), YT8M_E_BADARG,
               "the shared mode (vals == src) wants Hv == Hs, ld_vals == ld_src and no dvals");
  const Layout L(B, F, Hs, Hv, E);
  YT8M_REQUIRE(workspace && workspace_bytes >= L.bytes, YT8M_E_BADARG, "workspace smaller than yt8m_smattn_workspace_bytes");
  float* parts = dW1 ? static_cast<float*>(workspace) + L.bwd_parts : nullptr;
  float* groups = static_cast<float*>(workspace) + L.bwd_groups;
  const bool vec = aligned16(src) && aligned16(vals) && aligned16(G) && aligned16(pooled) && aligned16(dsrc) && (ld_src & 3) == 0 && (ld_vals & 3) == 0 &&
                   (ld_dsrc & 3) == 0 && (!dvals || (aligned16(dvals) && (ld_dvals & 3) == 0));
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const int b = (int)B, f = (int)F, hs = (int)Hs, hv = (int)Hv;
  int st;
#define SMATTN_BWD(EE)                                                                                                                   \
  if (shared)                                                                                                                            \
    launch_bwd<EE, true>(vec, src, ld_src, vals, ld_vals, W1, valid, lo, hi, att, pooled, G, dsrc, ld_dsrc, dvals, ld_dvals, dextra, parts, \
                         f, b, hs, hv, s);                                                                                               \
  else                                                                                                                                   \
    launch_bwd<EE, false>(vec, src, ld_src, vals, ld_vals, W1, valid, lo, hi, att, pooled, G, dsrc, ld_dsrc, dvals, ld_dvals, dextra,    \
                          parts, f, b, hs, hv, s);
  YT8M_BY_HEADS(E, SMATTN_BWD)
#undef SMATTN_BWD
  st = launch_status("smattn_bwd_kernel");
  if (st == YT8M_OK && db1 && hipMemsetAsync(db1, 0, (size_t)E * sizeof(float), s) != hipSuccess) st = launch_status("the memset of db1");
  if (st != YT8M_OK || !parts) return st;
  return sum_parts(parts, groups, (int)L.n, (int)L.parts, dW1, (int)L.n, nullptr, s);
}
