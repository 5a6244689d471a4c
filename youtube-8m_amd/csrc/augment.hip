// augment.hip -- the training-time data augmenters of W/all_data_augmentation on the reader's frames (gfx950, wave64; HBM-bound).
//   HalfAugmenter      (half_augmenter.py:8-45):        [originals; first halves; second halves] of every video, 3B rows
//   HalfVideoAugmenter (half_video_augmenter.py:8-16):  the means of those 3B frame blocks, in one pass over the bytes
//   NoiseAugmenter     (noise_augmenter.py:8-12):       dequantise + N(0, sigma^2) over every element, padding frames included
// Half segments, per video b with n = num_frames[b] clamped to [0, F] and s = max(n / 2, 1) (integer division): segment i in {0, 1}
// holds source frames i s + t at positions t < s and zeros from s on (gather, pad to F, times sequence_mask(s, F)).  A source frame
// at or past F (only when F = 1) reads as zeros, as TF's GPU gather_nd does.
#include <algorithm>
#include "common.h"
#include "philox.h"

namespace {

__device__ __forceinline__ int64_t half_len(int64_t n) { return n / 2 > 1 ? n / 2 : 1; }

// [B,F,D] -> [3B,F,D]: V = a 16-byte vector (rows of a multiple of 16 bytes) or one element; nv = V units per frame row.  A grid-stride
// loop over (output row, vector) items, a row's vectors on adjacent threads (as reverse_u8_kernel).
template <typename V>
__global__ __launch_bounds__(256) void half_segments_kernel(const V* __restrict__ x, const int32_t* __restrict__ nf, V* __restrict__ y,
                                                            int32_t* __restrict__ nf_out, int64_t B, int64_t F, int64_t nv) {
  const int64_t stride = (int64_t)gridDim.x * 256, gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t r = gid; r < 3 * B; r += stride) {
    const int64_t part = r / B, b = r - part * B;
    nf_out[r] = part == 0 ? nf[b] : (int32_t)half_len(clamp_frames(nf, b, F));
  }
  const int64_t total = 3 * B * F * nv;
  for (int64_t i = gid; i < total; i += stride) {
    const int64_t row = i / nv, v = i - row * nv;              // row = r F + t
    const int64_t r = row / F, t = row - r * F;
    const int64_t part = r / B, b = r - part * B;
    int64_t src = t;                                           // originals: the whole row block as it is, padding included
    if (part > 0) {
      const int64_t s = half_len(clamp_frames(nf, b, F));
      src = t < s ? (part - 1) * s + t : F;                    // F: a zero row
    }
    y[i] = src < F ? x[(b * F + src) * nv + v] : V{};
  }
}

// [B,F,D] bytes -> x [3B,D]: per column the three integer sums over frames [0, n), [0, s) and [s, 2s) clipped to [0, n), one workgroup
// of MEANS_WAVES waves per video.  Phase 1: wave w sums frames w, w + MEANS_WAVES, ... of W-byte column groups (lane + 64 k) into
// registers, then adds them into the LDS totals (integer: exact, any order).  Phase 2 runs on the first 256 threads only and is
// dequant_mean_l2norm_kernel's (elementwise.hip) column loop, arithmetic and reduction order (block_sum_256 over waves 0-3): the
// whole-video rows come out bit for bit as yt8m_dequant_mean_l2norm_u8's.
constexpr int MEANS_MAX_D = 2048;
constexpr int MEANS_WAVES = 16;          // one workgroup per video: 16 waves keep enough loads in flight (4 waves: ~0.5 TB/s at B = 200)

// block_sum_256 (common.h) of threads 0-255 inside a larger workgroup: the same wave sums, added in the same order
__device__ __forceinline__ float low256_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0 && w < 4) red[w] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

template <int W>
__global__ __launch_bounds__(64 * MEANS_WAVES) void half_segment_means_kernel(const uint8_t* __restrict__ q, const int32_t* __restrict__ nf,
                                                                 float* __restrict__ x, int64_t B, int64_t F, int64_t D, int l2norm,
                                                                 float eps) {
  __shared__ unsigned int tot[3][MEANS_MAX_D];
  __shared__ float red[3][4];
  const int64_t b = blockIdx.x;
  const int64_t n = clamp_frames(nf, b, F), s = half_len(n);
  const uint8_t* qb = q + b * F * D;
  for (int64_t c = threadIdx.x; c < 3 * D; c += 64 * MEANS_WAVES) tot[c / D][c % D] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t groups = D / W;
  for (int64_t g = lane; g < groups; g += 64) {
    unsigned int a[3][W];
#pragma unroll
    for (int k = 0; k < W; ++k) a[0][k] = a[1][k] = a[2][k] = 0u;
    for (int64_t f = w; f < n; f += MEANS_WAVES) {
      unsigned int word;
      if (W == 4) word = *reinterpret_cast<const unsigned int*>(qb + f * D + 4 * g);
      else word = qb[f * D + g];
      const int seg = f < s ? 1 : (f < 2 * s ? 2 : 0);         // 0: in no segment
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const unsigned int v = (word >> (8 * k)) & 255u;
        a[0][k] += v;
        if (seg == 1) a[1][k] += v;
        if (seg == 2) a[2][k] += v;
      }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      atomicAdd(&tot[0][W * g + k], a[0][k]);
      atomicAdd(&tot[1][W * g + k], a[1][k]);
      atomicAdd(&tot[2][W * g + k], a[2][k]);
    }
  }
  __syncthreads();
  // a segment row averages s frames of which k = s (n >= 2, or segment 0 of n = 1) or k = 0 (the rest) are real: (sum of k frames) / s
  const bool seg_live[2] = {n >= 1, n >= 2};
  const float sc = 4.0f / 255.0f, bias = 4.0f / 512.0f - 2.0f;
  float ss0 = 0.f, ss1 = 0.f, ss2 = 0.f;
  float* x0 = x + b * D;
  float* x1 = x + (B + b) * D;
  float* x2 = x + (2 * B + b) * D;
  const bool low = threadIdx.x < 256;
  for (int64_t c = threadIdx.x; low && c < D; c += 256) {
    const float m0 = n > 0 ? fmaf((float)tot[0][c] / (float)n, sc, bias) : 0.f;
    const float m1 = seg_live[0] ? fmaf((float)tot[1][c] / (float)s, sc, bias) : 0.f;
    const float m2 = seg_live[1] ? fmaf((float)tot[2][c] / (float)s, sc, bias) : 0.f;
    x0[c] = m0;
    x1[c] = m1;
    x2[c] = m2;
    ss0 += m0 * m0;
    ss1 += m1 * m1;
    ss2 += m2 * m2;
  }
  if (!l2norm) return;
  ss0 = low256_sum(ss0, red[0]);
  ss1 = low256_sum(ss1, red[1]);
  ss2 = low256_sum(ss2, red[2]);
  const float r0 = rsqrtf(fmaxf(ss0, eps)), r1 = rsqrtf(fmaxf(ss1, eps)), r2 = rsqrtf(fmaxf(ss2, eps));
  for (int64_t c = threadIdx.x; low && c < D; c += 256) {
    x0[c] *= r0;
    x1[c] *= r1;
    x2[c] *= r2;
  }
}

// q [B,F,D] bytes -> y fp32: utils.Dequantize (an fp32 multiply, then an add) with the padding frames 0, plus stddev * N(0,1) with
// noise_kernel's (random.hip) Philox layout: one thread per block of 4 consecutive elements of the logical [B,F,D] tensor.  stddev = 0
// draws nothing (the plain dequantisation).  VEC: D % 4 == 0 (a block never straddles two frames), 4-byte loads, 16-byte stores.
template <bool VEC>
__global__ __launch_bounds__(256) void dequant_noise_kernel(const uint8_t* __restrict__ q, const int32_t* __restrict__ nf,
                                                            float* __restrict__ y, int64_t B, int64_t F, int64_t D, float stddev,
                                                            uint64_t seed) {
  const int64_t n = B * F * D;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t e0 = g * 4;
  if (e0 >= n) return;
  const float sc = 4.0f / 255.0f, bias = 4.0f / 512.0f - 2.0f;
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (stddev != 0.f) yt8m_rng::normal4(yt8m_rng::philox4x32_10((uint64_t)g, seed), z);
  if (VEC) {
    const int64_t row = e0 / D, b = row / F, f = row - b * F;
    const bool live = f < clamp_frames(nf, b, F);
    const unsigned int word = live ? *reinterpret_cast<const unsigned int*>(q + e0) : 0u;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = live ? __fadd_rn(__fmul_rn((float)((word >> (8 * k)) & 255u), sc), bias) : 0.f;
      v[k] = stddev != 0.f ? yt8m_rng::add_normal(d, stddev, z[k]) : d;
    }
    *reinterpret_cast<float4*>(y + e0) = float4{v[0], v[1], v[2], v[3]};
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t e = e0 + k;
    if (e < n) {
      const int64_t row = e / D, b = row / F, f = row - b * F;
      const float d = f < clamp_frames(nf, b, F) ? __fadd_rn(__fmul_rn((float)q[e], sc), bias) : 0.f;
      y[e] = stddev != 0.f ? yt8m_rng::add_normal(d, stddev, z[k]) : d;
    }
  }
}

unsigned copy_grid(int64_t items) {
  const int64_t blocks = (items + 255) / 256;
  return (unsigned)std::min<int64_t>(std::max<int64_t>(blocks, 1), 256 * 32);   // grid-stride beyond ~8 K blocks (32 per CU)
}

bool disjoint(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa + abytes <= pb || pb + bbytes <= pa;
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_half_segments_u8(const uint8_t* x, const int32_t* num_frames, uint8_t* y, int32_t* num_frames_out, int64_t B, int64_t F,
                                     int64_t D, yt8m_stream_t stream) {
  YT8M_REQUIRE(B >= 0 && F >= 0 && D >= 0, YT8M_E_SHAPE, "negative dimension");
  if (B == 0) return YT8M_OK;
  YT8M_REQUIRE(x && num_frames && y && num_frames_out, YT8M_E_BADARG, "null operand");
  const int64_t n = B * F * D;
  YT8M_REQUIRE(disjoint(x, n, y, 3 * n), YT8M_E_BADARG, "source and destination overlap (the segments are written out of place)");
  YT8M_REQUIRE(disjoint(num_frames_out, 12 * B, y, 3 * n) && disjoint(num_frames_out, 12 * B, num_frames, 4 * B), YT8M_E_BADARG,
               "num_frames_out overlaps another operand");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, 4.0 * (double)n);
  const bool vec = D % 16 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  if (vec) {
    const int64_t nv = D / 16;
    hipLaunchKernelGGL(half_segments_kernel<uint4>, dim3(copy_grid(3 * B * F * nv)), dim3(256), 0, s, reinterpret_cast<const uint4*>(x),
                       num_frames, reinterpret_cast<uint4*>(y), num_frames_out, B, F, nv);
  } else {
    hipLaunchKernelGGL(half_segments_kernel<uint8_t>, dim3(copy_grid(3 * B * F * D)), dim3(256), 0, s, x, num_frames, y, num_frames_out,
                       B, F, D);
  }
  return launch_status("half_segments_kernel<u8>");
}

extern "C" int yt8m_half_segments_f32(const float* x, const int32_t* num_frames, float* y, int32_t* num_frames_out, int64_t B, int64_t F,
                                      int64_t D, yt8m_stream_t stream) {
  YT8M_REQUIRE(B >= 0 && F >= 0 && D >= 0, YT8M_E_SHAPE, "negative dimension");
  if (B == 0) return YT8M_OK;
  YT8M_REQUIRE(x && num_frames && y && num_frames_out, YT8M_E_BADARG, "null operand");
  const int64_t n = B * F * D;
  YT8M_REQUIRE(disjoint(x, 4 * n, y, 12 * n), YT8M_E_BADARG, "source and destination overlap (the segments are written out of place)");
  YT8M_REQUIRE(disjoint(num_frames_out, 12 * B, y, 12 * n) && disjoint(num_frames_out, 12 * B, num_frames, 4 * B), YT8M_E_BADARG,
               "num_frames_out overlaps another operand");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, 16.0 * (double)n);
  const bool vec = D % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  if (vec) {
    const int64_t nv = D / 4;
    hipLaunchKernelGGL(half_segments_kernel<float4>, dim3(copy_grid(3 * B * F * nv)), dim3(256), 0, s, reinterpret_cast<const float4*>(x),
                       num_frames, reinterpret_cast<float4*>(y), num_frames_out, B, F, nv);
  } else {
    hipLaunchKernelGGL(half_segments_kernel<float>, dim3(copy_grid(3 * B * F * D)), dim3(256), 0, s, x, num_frames, y, num_frames_out,
                       B, F, D);
  }
  return launch_status("half_segments_kernel<f32>");
}

extern "C" int yt8m_half_segment_means_u8(const uint8_t* q, const int32_t* num_frames, float* x, int64_t B, int64_t F, int64_t D,
                                          int l2norm, float eps, yt8m_stream_t stream) {
  YT8M_REQUIRE(B >= 0 && F >= 0 && D >= 0, YT8M_E_SHAPE, "negative dimension");
  YT8M_REQUIRE(D <= MEANS_MAX_D, YT8M_E_SHAPE, "D must be <= 2048 (the column totals live in LDS)");
  if (B * D == 0) return YT8M_OK;
  YT8M_REQUIRE(q && num_frames && x, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(disjoint(q, B * F * D, x, 12 * B * D), YT8M_E_BADARG, "source and destination overlap");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, (double)(B * F * D) + 12.0 * (double)(B * D));
  if (D % 4 == 0 && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
    hipLaunchKernelGGL(half_segment_means_kernel<4>, dim3((unsigned)B), dim3(64 * MEANS_WAVES), 0, s, q, num_frames, x, B, F, D, l2norm, eps);
  } else {
    hipLaunchKernelGGL(half_segment_means_kernel<1>, dim3((unsigned)B), dim3(64 * MEANS_WAVES), 0, s, q, num_frames, x, B, F, D, l2norm, eps);
  }
  return launch_status("half_segment_means_kernel");
}

extern "C" int yt8m_dequant_noise_u8(const uint8_t* q, const int32_t* num_frames, float* y, int64_t B, int64_t F, int64_t D, float stddev,
                                     uint64_t seed, yt8m_stream_t stream) {
  YT8M_REQUIRE(B >= 0 && F >= 0 && D >= 0, YT8M_E_SHAPE, "negative dimension");
  YT8M_REQUIRE(stddev >= 0.f, YT8M_E_BADARG, "stddev must be >= 0");
  const int64_t n = B * F * D;
  if (n == 0) return YT8M_OK;
  YT8M_REQUIRE(q && num_frames && y, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(disjoint(q, n, y, 4 * n), YT8M_E_BADARG, "source and destination overlap");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, 5.0 * (double)n);
  const int64_t groups = (n + 3) / 4;
  const dim3 grid((unsigned)((groups + 255) / 256));
  if (D % 4 == 0 && ((reinterpret_cast<uintptr_t>(q) & 3) | (reinterpret_cast<uintptr_t>(y) & 15)) == 0) {
    hipLaunchKernelGGL(dequant_noise_kernel<true>, grid, dim3(256), 0, s, q, num_frames, y, B, F, D, stddev, seed);
  } else {
    hipLaunchKernelGGL(dequant_noise_kernel<false>, grid, dim3(256), 0, s, q, num_frames, y, B, F, D, stddev, seed);
  }
  return launch_status("dequant_noise_kernel");
}
