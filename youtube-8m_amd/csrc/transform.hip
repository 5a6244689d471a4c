// transform.hip -- the ResolutionTransformer of W/all_feature_transform/resolution_transformer.py:7-29 on the reader's frames (gfx950,
// wave64; HBM-bound): x [B,F,D] -> y [B,F2,D] fp32 with F2 = F / r, row g of a video the mean of its frames [g r, (g + 1) r), then
// l2-normalised; frames from F2 r on are dropped and num_frames becomes num_frames / r (integer divisions).
//   bytes:  the frames are dequantised (utils.Dequantize) with the padding frames 0, so a group holding k < r real frames is
//           (the sum of k dequantised frames) / r, and one holding none is a zero row.  Summed as integers: (sc * sum + k * bias) / r.
//   floats: the plain mean of the r rows as they are (the reference averages whatever floats it is given).
// One wave owns an output row: lane l sums the V-unit column groups l, l + 64, ... over the group's input rows in registers, the
// row's sum of squares comes from wave shuffles, and the lane scales and stores what it holds.  No LDS and no atomics.
#include <algorithm>
#include <type_traits>
#include "common.h"

namespace {

// the frames of video b; every frame where no num_frames is given
__device__ __forceinline__ int64_t frames_of(const int32_t* nf, int64_t b, int64_t F) { return nf ? clamp_frames(nf, b, F) : F; }

// One load unit of a row: W elements of type E held as V, added element-wise into W accumulators of type A.
template <typename V> struct Unit;
template <> struct Unit<uint4> {                 // 16 bytes
  using A = unsigned int;
  static constexpr int W = 16, KEPT = 2;
  static __device__ __forceinline__ void add(A* a, const uint4& v) {
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) a[4 * i + k] += (w[i] >> (8 * k)) & 255u;
  }
};
template <> struct Unit<unsigned int> {          // 4 bytes
  using A = unsigned int;
  static constexpr int W = 4, KEPT = 8;
  static __device__ __forceinline__ void add(A* a, unsigned int v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += (v >> (8 * k)) & 255u;
  }
};
template <> struct Unit<uint8_t> {
  using A = unsigned int;
  static constexpr int W = 1, KEPT = 8;
  static __device__ __forceinline__ void add(A* a, uint8_t v) { a[0] += v; }
};
template <> struct Unit<float4> {
  using A = float;
  static constexpr int W = 4, KEPT = 8;
  static __device__ __forceinline__ void add(A* a, const float4& v) {
    a[0] += v.x;
    a[1] += v.y;
    a[2] += v.z;
    a[3] += v.w;
  }
};
template <> struct Unit<float> {
  using A = float;
  static constexpr int W = 1, KEPT = 8;
  static __device__ __forceinline__ void add(A* a, float v) { a[0] += v; }
};

constexpr int ROWS_PER_BLOCK = 4;                // waves per workgroup, one output row each

// x [B,F,nv] units -> y [B,F2,nv W] floats.  The lane keeps its first KEPT units of the row in registers (every unit of a row of up to
// 64 KEPT W elements: 2048 for the 16-byte and the float4 forms) and writes them once, scaled; units beyond those are stored
// unnormalised and scaled in place after the reduction, by the lane that wrote them.  bytes: mask and dequantise (see the top).
template <typename V, bool BYTES>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void resolution_mean_kernel(const V* __restrict__ x, const int32_t* __restrict__ nf,
                                                                              float* __restrict__ y, int32_t* __restrict__ nf_out,
                                                                              int64_t B, int64_t F, int64_t nv, int64_t r, int l2norm,
                                                                              float eps) {
  using U = Unit<V>;
  using A = typename U::A;
  constexpr int W = U::W, KEPT = U::KEPT;
  const int64_t F2 = F / r, rows = B * F2;
  if (nf_out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) nf_out[b] = (int32_t)(frames_of(nf, b, F) / r);
  }
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
  if (row >= rows || nv == 0) return;
  const int64_t b = row / F2, g = row - b * F2;
  int64_t k = r;                                                                   // input rows to add: bytes, the real frames only
  if (BYTES) k = std::min<int64_t>(std::max<int64_t>(frames_of(nf, b, F) - g * r, 0), r);
  const V* xr = x + (b * F + g * r) * nv;
  float* yr = y + row * nv * W;
  // bytes: (sc sum + k bias) / r with sc = 4/255 and bias = 4/512 - 2 = -255/128 is (512 sum - 65025 k) / (32640 r).  The numerator is
  // an exact integer (int32 while r <= 16384) and the l2-normalised row is numerator / sqrt(sum of squared numerators): formed in
  // fp64 and rounded to fp32 once, the output is the correctly rounded value of the reference's arithmetic (in fp32 term by term the
  // rounding of sc alone is ~15 ulp of a mean near 0, since sc sum and k bias nearly cancel).  The output is 1/r of the traffic and
  // the kernel is bound by its loads, so the fp64 arithmetic per output element is free.  floats: fp32 throughout.
  using R = typename std::conditional<BYTES, double, float>::type;
  const bool small = r <= 16384;
  const R unit = BYTES ? R(1) / (R(32640) * (R)r) : R(1) / (R)r;                  // value(a) * unit = the mean
  auto value = [&](A a) {
    if (!BYTES) return (R)a;
    return small ? (R)(512 * (int)a - 65025 * (int)k) : (R)(512ll * (long long)a - 65025ll * (long long)k);
  };

  A acc[KEPT][W];
#pragma unroll
  for (int u = 0; u < KEPT; ++u)
#pragma unroll
    for (int e = 0; e < W; ++e) acc[u][e] = A(0);
  // a kept unit past the row's end loads the row's last unit instead (no branch around a load: the loads of several input rows stay
  // in flight together); what it sums is neither counted nor stored
  int64_t col[KEPT];
#pragma unroll
  for (int u = 0; u < KEPT; ++u) col[u] = std::min<int64_t>(lane + 64 * u, nv - 1);
#pragma unroll 4
  for (int64_t j = 0; j < k; ++j) {
#pragma unroll
    for (int u = 0; u < KEPT; ++u) U::add(acc[u], xr[j * nv + col[u]]);
  }
  R ss = 0;
#pragma unroll
  for (int u = 0; u < KEPT; ++u)
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const R m = value(acc[u][e]);
      ss += lane + 64 * u < nv ? m * m : R(0);
    }
#pragma unroll 1
  for (int64_t c = lane + 64 * KEPT; c < nv; c += 64) {                            // rows wider than the registers hold
    A a[W];
#pragma unroll
    for (int e = 0; e < W; ++e) a[e] = A(0);
#pragma unroll 4
    for (int64_t j = 0; j < k; ++j) U::add(a, xr[j * nv + c]);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const R m = value(a[e]);
      yr[c * W + e] = (float)(m * unit);
      ss += m * m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const R norm2 = ss * unit * unit;                                                // the mean row's sum of squares
  const R scale = l2norm ? unit / (R)sqrt(norm2 > (R)eps ? norm2 : (R)eps) : unit;
#pragma unroll
  for (int u = 0; u < KEPT; ++u) {
    const int64_t c = lane + 64 * u;
    if (c < nv) {
      if (W % 4 == 0) {
#pragma unroll
        for (int e = 0; e < W; e += 4)
          *reinterpret_cast<float4*>(yr + c * W + e) = float4{(float)(value(acc[u][e]) * scale), (float)(value(acc[u][e + 1]) * scale),
                                                              (float)(value(acc[u][e + 2]) * scale), (float)(value(acc[u][e + 3]) * scale)};
      } else {
        yr[c] = (float)(value(acc[u][0]) * scale);
      }
    }
  }
  if (l2norm) {
    const float rescale = (float)(scale / unit);                                   // the stored tail is fp32 already: two roundings there
    for (int64_t c = lane + 64 * KEPT; c < nv; c += 64)
#pragma unroll
      for (int e = 0; e < W; ++e) yr[c * W + e] *= rescale;
  }
}

bool disjoint(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa + abytes <= pb || pb + bbytes <= pa;
}

template <typename V, bool BYTES>
void launch(const void* x, const int32_t* nf, float* y, int32_t* nf_out, int64_t B, int64_t F, int64_t nv, int64_t r, int l2norm, float eps,
            hipStream_t s) {
  const int64_t rows = B * (F / r);
  hipLaunchKernelGGL((resolution_mean_kernel<V, BYTES>), dim3((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)),
                     dim3(64 * ROWS_PER_BLOCK), 0, s, static_cast<const V*>(x), nf, y, nf_out, B, F, nv, r, l2norm, eps);
}

// the checks the two entry points share; elem = bytes per input element
int check_operands(const void* x, const int32_t* num_frames, const float* y, const int32_t* num_frames_out, int64_t B, int64_t F, int64_t D,
                   int64_t r, int64_t elem) {
  using namespace yt8m;
  YT8M_REQUIRE(B >= 0 && F >= 0 && D >= 0, YT8M_E_SHAPE, "negative dimension");
  YT8M_REQUIRE(r >= 1 && r <= F, YT8M_E_BADARG, "resolution must be in [1, F]");
  YT8M_REQUIRE(B * (F / r) <= (int64_t)0x7fffffff * ROWS_PER_BLOCK, YT8M_E_SHAPE, "too many output rows for one launch");
  if (B == 0) return YT8M_OK;
  YT8M_REQUIRE(D == 0 || (x && y), YT8M_E_BADARG, "null operand");
  const int64_t nx = B * F * D * elem, ny = B * (F / r) * D * 4;
  YT8M_REQUIRE(disjoint(x, nx, y, ny), YT8M_E_BADARG, "source and destination overlap (the means are written out of place)");
  if (num_frames_out)
    YT8M_REQUIRE(disjoint(num_frames_out, 4 * B, y, ny) && disjoint(num_frames_out, 4 * B, x, nx) &&
                     disjoint(num_frames_out, 4 * B, num_frames, 4 * B),
                 YT8M_E_BADARG, "num_frames_out overlaps another operand");
  return YT8M_OK;
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_resolution_mean_u8(const uint8_t* q, const int32_t* num_frames, float* y, int32_t* num_frames_out, int64_t B, int64_t F,
                                       int64_t D, int64_t resolution, int l2norm, float eps, yt8m_stream_t stream) {
  const int rc = check_operands(q, num_frames, y, num_frames_out, B, F, D, resolution, 1);
  if (rc != YT8M_OK || B == 0) return rc;
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, (double)(B * F * D) + 4.0 * (double)(B * (F / resolution) * D));
  const uintptr_t qa = reinterpret_cast<uintptr_t>(q), ya = reinterpret_cast<uintptr_t>(y);
  if (D % 16 == 0 && ((qa | ya) & 15) == 0) {
    launch<uint4, true>(q, num_frames, y, num_frames_out, B, F, D / 16, resolution, l2norm, eps, s);
  } else if (D % 4 == 0 && (qa & 3) == 0 && (ya & 15) == 0) {
    launch<unsigned int, true>(q, num_frames, y, num_frames_out, B, F, D / 4, resolution, l2norm, eps, s);
  } else {
    launch<uint8_t, true>(q, num_frames, y, num_frames_out, B, F, D, resolution, l2norm, eps, s);
  }
  return launch_status("resolution_mean_kernel<u8>");
}

extern "C" int yt8m_resolution_mean_f32(const float* x, const int32_t* num_frames, float* y, int32_t* num_frames_out, int64_t B, int64_t F,
                                        int64_t D, int64_t resolution, int l2norm, float eps, yt8m_stream_t stream) {
  const int rc = check_operands(x, num_frames, y, num_frames_out, B, F, D, resolution, 4);
  if (rc != YT8M_OK || B == 0) return rc;
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, 4.0 * (double)(B * F * D) + 4.0 * (double)(B * (F / resolution) * D));
  if (D % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0) {
    launch<float4, false>(x, num_frames, y, num_frames_out, B, F, D / 4, resolution, l2norm, eps, s);
  } else {
    launch<float, false>(x, num_frames, y, num_frames_out, B, F, D, resolution, l2norm, eps, s);
  }
  return launch_status("resolution_mean_kernel<f32>");
}
