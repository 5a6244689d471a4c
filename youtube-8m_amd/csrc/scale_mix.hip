// scale_mix.hip -- how the LstmMultiscale plugins combine their scales (Z/frame_level_models.py:2977-2985, :3149-3157), in one pass
// each way (gfx950, wave64).  For L planes p_l [rows, cols] (sub-predictions) and L planes z_l [rows, cols] (mix logits), 1 <= L <= 8:
//   fwd:  w_l = softmax over l of z_l (maximum subtracted, e_l / sum e),  out = sum_l w_l p_l
//   bwd:  w recomputed from z;  dp_l = w_l g,  dz_l = w_l (p_l - out) g  -- the difference per element, from the saved out
// i.e. tf.stack -> tf.nn.softmax(dim=1) -> multiply -> reduce_sum without the stacked [L, rows, cols] tensors in between.  Purely
// elementwise: the planes are contiguous, so a launch walks rows * cols elements whatever the row length.  The 2 L (fwd) or 4 L (bwd)
// plane pointers travel by value in the kernel arguments (as memory_link.hip's Segs): the loops over l are unrolled at compile time and
// read the table with scalar loads.  No reductions across threads, no atomics, no LDS: a second run gives the same bits.
// 16-byte accesses when every operand is 16-byte aligned (the last rows * cols % 4 elements one at a time), single elements otherwise.
// Grid-stride over a grid sized to the chip (256 CUs x 8 workgroups of 256), not to the element count.
#include <math.h>
#include "common.h"

namespace {

constexpr int MAX_L = 8;
constexpr int BLOCK = 256;
constexpr int MAX_GRID = 256 * 8;

struct MixIn {                           // by value
  const float* p[MAX_L];
  const float* z[MAX_L];
};
struct MixOut {                          // by value; a null entry is skipped
  float* dp[MAX_L];
  float* dz[MAX_L];
};

// e_l = exp(z_l - max z) in place, returns their sum (s >= 1: the maximum's own term is exp(0))
template <int L>
__device__ __forceinline__ float mix_exp(float (&e)[L]) {
  float m = e[0];
#pragma unroll
  for (int l = 1; l < L; ++l) m = fmaxf(m, e[l]);
  float s = 0.f;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    e[l] = expf(e[l] - m);
    s += e[l];
  }
  return s;
}

template <int L>
__device__ __forceinline__ float mix_fwd_one(const MixIn& a, int64_t i) {
  float e[L], p[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    e[l] = a.z[l][i];
    p[l] = a.p[l][i];
  }
  const float s = mix_exp<L>(e);
  float o = 0.f;
#pragma unroll
  for (int l = 0; l < L; ++l) o += (e[l] / s) * p[l];
  return o;
}

template <int L>
__device__ __forceinline__ void mix_bwd_one(const MixIn& a, const MixOut& d, const float* __restrict__ out, const float* __restrict__ g,
                                            int64_t i) {
  float e[L], p[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    e[l] = a.z[l][i];
    p[l] = a.p[l][i];
  }
  const float s = mix_exp<L>(e);
  const float o = out[i], gi = g[i];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const float w = e[l] / s;
    if (d.dp[l]) d.dp[l][i] = w * gi;
    if (d.dz[l]) d.dz[l][i] = w * (p[l] - o) * gi;
  }
}

// VEC: every operand 16-byte aligned.  n4 = n / 4 vectors, then the n % 4 elements behind them.
template <int L, bool VEC>
__global__ __launch_bounds__(BLOCK) void scale_mix_fwd_kernel(MixIn a, float* __restrict__ out, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x, step = (int64_t)gridDim.x * BLOCK;
  if (!VEC) {
    for (int64_t i = tid; i < n; i += step) out[i] = mix_fwd_one<L>(a, i);
    return;
  }
  const int64_t n4 = n >> 2;
  for (int64_t i = tid; i < n4; i += step) {
    float4 e[L], p[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      e[l] = reinterpret_cast<const float4*>(a.z[l])[i];
      p[l] = reinterpret_cast<const float4*>(a.p[l])[i];
    }
    float ex[L], ey[L], ez[L], ew[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      ex[l] = e[l].x; ey[l] = e[l].y; ez[l] = e[l].z; ew[l] = e[l].w;
    }
    const float sx = mix_exp<L>(ex), sy = mix_exp<L>(ey), sz = mix_exp<L>(ez), sw = mix_exp<L>(ew);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      o.x += (ex[l] / sx) * p[l].x;
      o.y += (ey[l] / sy) * p[l].y;
      o.z += (ez[l] / sz) * p[l].z;
      o.w += (ew[l] / sw) * p[l].w;
    }
    reinterpret_cast<float4*>(out)[i] = o;
  }
  const int64_t tail = (n4 << 2) + tid;                                   // fewer than 4 elements
  if (tail < n) out[tail] = mix_fwd_one<L>(a, tail);
}

template <int L, bool VEC>
__global__ __launch_bounds__(BLOCK) void scale_mix_bwd_kernel(MixIn a, MixOut d, const float* __restrict__ out, const float* __restrict__ g,
                                                              int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x, step = (int64_t)gridDim.x * BLOCK;
  if (!VEC) {
    for (int64_t i = tid; i < n; i += step) mix_bwd_one<L>(a, d, out, g, i);
    return;
  }
  const int64_t n4 = n >> 2;
  for (int64_t i = tid; i < n4; i += step) {
    float4 e[L], p[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      e[l] = reinterpret_cast<const float4*>(a.z[l])[i];
      p[l] = reinterpret_cast<const float4*>(a.p[l])[i];
    }
    const float4 o = reinterpret_cast<const float4*>(out)[i], gi = reinterpret_cast<const float4*>(g)[i];
    float ex[L], ey[L], ez[L], ew[L];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      ex[l] = e[l].x; ey[l] = e[l].y; ez[l] = e[l].z; ew[l] = e[l].w;
    }
    const float sx = mix_exp<L>(ex), sy = mix_exp<L>(ey), sz = mix_exp<L>(ez), sw = mix_exp<L>(ew);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const float4 w = make_float4(ex[l] / sx, ey[l] / sy, ez[l] / sz, ew[l] / sw);
      if (d.dp[l]) reinterpret_cast<float4*>(d.dp[l])[i] = make_float4(w.x * gi.x, w.y * gi.y, w.z * gi.z, w.w * gi.w);
      if (d.dz[l])
        reinterpret_cast<float4*>(d.dz[l])[i] = make_float4(w.x * (p[l].x - o.x) * gi.x, w.y * (p[l].y - o.y) * gi.y,
                                                            w.z * (p[l].z - o.z) * gi.z, w.w * (p[l].w - o.w) * gi.w);
    }
  }
  const int64_t tail = (n4 << 2) + tid;
  if (tail < n) mix_bwd_one<L>(a, d, out, g, tail);
}

inline bool shape_ok(int L, int64_t rows, int64_t cols) {
  return L >= 1 && L <= MAX_L && rows >= 1 && cols >= 1 && rows <= 0x7fffffffLL && cols <= 0x7fffffffLL && rows * cols <= (1LL << 40);
}

// workgroups for `work` threads' worth of elements or vectors: enough to cover them once, at most what fills the chip
inline unsigned grid_for(int64_t work) {
  const int64_t blocks = (work + BLOCK - 1) / BLOCK;
  return (unsigned)(blocks < 1 ? 1 : (blocks > MAX_GRID ? MAX_GRID : blocks));
}

template <int L>
void launch_fwd(bool vec, const MixIn& a, float* out, int64_t n, hipStream_t s) {
  if (vec)
    hipLaunchKernelGGL((scale_mix_fwd_kernel<L, true>), dim3(grid_for(n >> 2)), dim3(BLOCK), 0, s, a, out, n);
  else
    hipLaunchKernelGGL((scale_mix_fwd_kernel<L, false>), dim3(grid_for(n)), dim3(BLOCK), 0, s, a, out, n);
}

template <int L>
void launch_bwd(bool vec, const MixIn& a, const MixOut& d, const float* out, const float* g, int64_t n, hipStream_t s) {
  if (vec)
    hipLaunchKernelGGL((scale_mix_bwd_kernel<L, true>), dim3(grid_for(n >> 2)), dim3(BLOCK), 0, s, a, d, out, g, n);
  else
    hipLaunchKernelGGL((scale_mix_bwd_kernel<L, false>), dim3(grid_for(n)), dim3(BLOCK), 0, s, a, d, out, g, n);
}

#define MIX_DISPATCH(L, call)                                                                                                  \
  switch (L) {                                                                                                                 \
    case 1: call(1); break;                                                                                                    \
    case 2: call(2); break;                                                                                                    \
    case 3: call(3); break;                                                                                                    \
    case 4: call(4); break;                                                                                                    \
    case 5: call(5); break;                                                                                                    \
    case 6: call(6); break;                                                                                                    \
    case 7: call(7); break;                                                                                                    \
    default: call(8); break;                                                                                                   \
  }

}  // namespace

using namespace yt8m;

extern "C" int yt8m_scale_mix_supported(int L, int64_t rows, int64_t cols) { return shape_ok(L, rows, cols) ? 1 : 0; }

extern "C" int yt8m_scale_mix_fwd(int L, const float* const* p, const float* const* z, float* out, int64_t rows, int64_t cols,
                                  yt8m_stream_t stream) {
  YT8M_REQUIRE(shape_ok(L, rows, cols), YT8M_E_SHAPE, "1 <= L <= 8 planes of rows >= 1, cols >= 1 (< 2^31 each, <= 2^40 elements)");
  YT8M_REQUIRE(p && z && out, YT8M_E_BADARG, "null operand");
  MixIn a;
  bool vec = aligned16(out);
  for (int l = 0; l < MAX_L; ++l) a.p[l] = a.z[l] = nullptr;
  for (int l = 0; l < L; ++l) {
    YT8M_REQUIRE(p[l] && z[l], YT8M_E_BADARG, "null plane");
    a.p[l] = p[l];
    a.z[l] = z[l];
    vec = vec && aligned16(p[l]) && aligned16(z[l]);
  }
  const int64_t n = rows * cols;
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
#define MIX_FWD(LL) launch_fwd<LL>(vec, a, out, n, s)
  MIX_DISPATCH(L, MIX_FWD)
#undef MIX_FWD
  return launch_status("scale_mix_fwd_kernel");
}

extern "C" int yt8m_scale_mix_bwd(int L, const float* const* p, const float* const* z, const float* out, const float* g,
                                  float* const* dp, float* const* dz, int64_t rows, int64_t cols, yt8m_stream_t stream) {
  YT8M_REQUIRE(shape_ok(L, rows, cols), YT8M_E_SHAPE, "1 <= L <= 8 planes of rows >= 1, cols >= 1 (< 2^31 each, <= 2^40 elements)");
  YT8M_REQUIRE(p && z && out && g && dp && dz, YT8M_E_BADARG, "null operand");
  MixIn a;
  MixOut d;
  bool vec = aligned16(out) && aligned16(g), any = false;
  for (int l = 0; l < MAX_L; ++l) {
    a.p[l] = a.z[l] = nullptr;
    d.dp[l] = d.dz[l] = nullptr;
  }
  for (int l = 0; l < L; ++l) {
    YT8M_REQUIRE(p[l] && z[l], YT8M_E_BADARG, "null plane");
    a.p[l] = p[l];
    a.z[l] = z[l];
    d.dp[l] = dp[l];                                                      // null: this gradient is not wanted
    d.dz[l] = dz[l];
    any = any || dp[l] || dz[l];
    vec = vec && aligned16(p[l]) && aligned16(z[l]) && aligned16(dp[l]) && aligned16(dz[l]);
  }
  if (!any) return YT8M_OK;
  const int64_t n = rows * cols;
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
#define MIX_BWD(LL) launch_bwd<LL>(vec, a, d, out, g, n, s)
  MIX_DISPATCH(L, MIX_BWD)
#undef MIX_BWD
  return launch_status("scale_mix_bwd_kernel");
}
