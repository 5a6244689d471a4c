// frame_pyramid.hip -- every coarse level of the multi-resolution LSTM plugin's input in ONE pass over the reader's bytes (gfx950, wave64;
// HBM-bound).  W/all_frame_models/multires_lstm_memory_deep_combine_chain_model.py:149-165 + :21 per level r = 2, 4, .., 2^levels:
// mean over every r dequantised frames (padding frames 0, the divisor always r), split by feature, every part l2-normalised.
//   q [B,F,D] uint8 -> y[l * nseg + s] [F / r, B, widths[s]] fp32, r = 2^(l+1): TIME-major, what the LSTM stack reads with no further copy
// The arithmetic is resolution_mean_kernel<.., BYTES>'s (csrc/transform.hip) per segment instead of per row: the integer numerator
// 512 S - 65025 k of the mean, the sum of squares and the quotient in fp64, rounded to fp32 once.
// One workgroup owns a block of R = 2^levels frames of one video, one wave per pair of frames (R / 2 waves).  A wave adds its two frames
// in registers (lane l holds the load units l, l + 64, ..: every load of the pair is in flight together, and a block's R / 2 waves walk
// its frames side by side instead of one wave down a dependent chain) and writes level 0's row; the integer sums then go up a tree
// through LDS (packed to 16 bits: a sum of 64 bytes is < 2^16), wave w of level l + 1 adding slots 2w and 2w + 1 in place.  Every byte is
// read once.  Per-lane sums in unit order, then the wave butterfly: a fixed order, no atomics -- a step replays bit for bit.
#include <math.h>
#include "common.h"

namespace {

constexpr int MAX_LEVELS = 5;              // R / 2 = 16 waves: the largest workgroup
constexpr int MAX_SEGS = 8;
constexpr int LDS_MAX = 64 * 1024;

struct Pyramid {                           // by value in the kernel arguments
  float* y[MAX_LEVELS * MAX_SEGS];         // level-major
  int32_t* nf_out[MAX_LEVELS];             // may be null
  int32_t off[MAX_SEGS + 1];               // first column of segment s; off[nseg] = D
};

// One load unit of a row: W bytes held as V, added element-wise into W integer accumulators; KEPT units per lane.
template <typename V> struct Unit;
template <> struct Unit<uint4> {
  static constexpr int W = 16, KEPT = 2;
  static __device__ __forceinline__ void add(unsigned int* a, const uint4& v) {
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) a[4 * i + k] += (w[i] >> (8 * k)) & 255u;
  }
};
template <> struct Unit<unsigned int> {
  static constexpr int W = 4, KEPT = 8;
  static __device__ __forceinline__ void add(unsigned int* a, unsigned int v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += (v >> (8 * k)) & 255u;
  }
};
template <> struct Unit<uint8_t> {
  static constexpr int W = 1, KEPT = 8;
  static __device__ __forceinline__ void add(unsigned int* a, uint8_t v) { a[0] += v; }
};

constexpr int packed_words(int W) { return (W + 1) / 2; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Row g of level l (resolution r = 2^(l+1)) of video b from the wave's integer sums: per segment the sum of squares, then the store.
// k: the real frames of the group.  VEC4: 16-byte stores (every width % 4 == 0, every output 16-byte aligned).
template <int W, int KEPT, bool VEC4>
__device__ __forceinline__ void write_row(const Pyramid& p, int nseg, int l, int64_t g, int64_t b, int64_t B, int k, int nv, int lane,
                                          const unsigned int (&acc)[KEPT][W], float eps) {
  const double unit = 1.0 / (32640.0 * (double)(2 << l));                          // value(a) * unit = the mean
  auto value = [&](unsigned int a) { return (double)(512 * (int)a - 65025 * k); }; // exact: a <= 255 * 64
  // the store converts the integer again instead of keeping the row's fp64 numerators alive across the reduction (2 registers each)
  auto again = [&](unsigned int a) {
    asm volatile("" : "+v"(a));
    return value(a);
  };
  for (int s = 0; s < nseg; ++s) {                                                 // wave-uniform
    const int lo = p.off[s], hi = p.off[s + 1];
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < KEPT; ++u) {
      const int c = (lane + 64 * u) * W;
      const bool in = lane + 64 * u < nv && c >= lo && c < hi;
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const double m = value(acc[u][e]);
        ss += in ? m * m : 0.0;
      }
    }
    ss = wave_sum_f64(ss);
    const double norm2 = ss * unit * unit;                                         // the mean part's sum of squares
    const double scale = unit / sqrt(norm2 > (double)eps ? norm2 : (double)eps);
    float* yr = p.y[l * nseg + s] + (g * B + b) * (int64_t)(hi - lo) - lo;
#pragma unroll
    for (int u = 0; u < KEPT; ++u) {
      const int c = (lane + 64 * u) * W;
      if (lane + 64 * u < nv && c >= lo && c < hi) {
        if (VEC4) {
#pragma unroll
          for (int e = 0; e < W; e += 4)
          {
            *reinterpret_cast<float4*>(yr + c + e) = float4{(float)(again(acc[u][e]) * scale), (float)(again(acc[u][e + 1]) * scale),
                                                            (float)(again(acc[u][e + 2]) * scale), (float)(again(acc[u][e + 3]) * scale)};
          }
        } else {
#pragma unroll
          for (int e = 0; e < W; ++e) yr[c + e] = (float)(again(acc[u][e]) * scale);
        }
      }
    }
  }
}

// x [B,F,nv] units.  Grid: B * nblk workgroups of 64 * R / 2 threads, nblk = ceil((F / 2) / (R / 2)); dynamic LDS: (R / 2) slots of
// upl * packed_words(W) * 64 words, upl = ceil(nv / 64) <= KEPT.  Groups past F / r of a level are not written.
template <typename V, bool VEC4>
__global__ __launch_bounds__(1024) void frame_pyramid_kernel(const V* __restrict__ x, const int32_t* __restrict__ nf, Pyramid p, int64_t B,
                                                             int64_t F, int nv, int levels, int nseg, int nblk, float eps) {
  using U = Unit<V>;
  constexpr int W = U::W, KEPT = U::KEPT, PW = packed_words(W);
  extern __shared__ unsigned int sums[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                  // wave-uniform
  const int64_t b = blockIdx.x / nblk;
  const int j = (int)(blockIdx.x - b * nblk);
  const int upl = (nv + 63) >> 6;
  int64_t n = F;
  if (nf) {
    n = __builtin_amdgcn_readfirstlane(nf[b]);
    n = n < 0 ? 0 : (n > F ? F : n);
  }
  if (j == 0 && threadIdx.x == 0) {
    for (int l = 0; l < levels; ++l) {
      int32_t* o = p.nf_out[l];
      if (o) o[b] = (int32_t)(n >> (l + 1));
    }
  }
  auto group_frames = [&](int64_t g, int l) {                                      // real frames of group g of level l
    const int64_t r = (int64_t)2 << l, k = n - g * r;
    return (int)(k < 0 ? 0 : (k > r ? r : k));
  };
  auto slot = [&](int sl, int u, int pw) { return sums + ((sl * upl + u) * PW + pw) * 64 + lane; };

  unsigned int acc[KEPT][W];
#pragma unroll
  for (int u = 0; u < KEPT; ++u)
#pragma unroll
    for (int e = 0; e < W; ++e) acc[u][e] = 0u;

  // level 0: the wave's pair of frames.  A unit past the row's end loads the row's last unit instead (no branch around a load); what it
  // sums is neither counted nor stored.
  int waves = (1 << levels) >> 1;
  int64_t g = (int64_t)j * waves + w;
  bool live = g < (F >> 1);
  if (live) {
    const int k = group_frames(g, 0);
    const V* xr = x + (b * F + 2 * g) * nv;
    V v[2][KEPT];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int u = 0; u < KEPT; ++u) {
        const int c = lane + 64 * u < nv ? lane + 64 * u : nv - 1;
        v[f][u] = f < k ? xr[(int64_t)f * nv + c] : V{};
      }
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int u = 0; u < KEPT; ++u) U::add(acc[u], v[f][u]);
    if (levels > 1) {
#pragma unroll
      for (int u = 0; u < KEPT; ++u)
        if (lane + 64 * u < nv)
#pragma unroll
          for (int pw = 0; pw < PW; ++pw) *slot(w, u, pw) = acc[u][2 * pw] | (2 * pw + 1 < W ? acc[u][(2 * pw + 1) % W] << 16 : 0u);
    }
    write_row<W, KEPT, VEC4>(p, nseg, 0, g, b, B, k, nv, lane, acc, eps);
  }
  for (int l = 1; l < levels; ++l) {                                               // uniform over the workgroup: every wave meets every barrier
    waves >>= 1;
    g = (int64_t)j * waves + w;
    live = w < waves && g < (F >> (l + 1));
    __syncthreads();
    if (live) {
#pragma unroll
      for (int u = 0; u < KEPT; ++u)
        if (lane + 64 * u < nv)
#pragma unroll
          for (int pw = 0; pw < PW; ++pw) {
            const unsigned int t = *slot(2 * w, u, pw) + *slot(2 * w + 1, u, pw);  // both halves stay below 2^16: no carry between them
            acc[u][2 * pw] = t & 0xffffu;
            if (2 * pw + 1 < W) acc[u][(2 * pw + 1) % W] = t >> 16;
          }
    }
    if (l + 1 < levels) {
      __syncthreads();                                                             // slots 2w, 2w + 1 are read: slot w may be overwritten
      if (live) {
#pragma unroll
        for (int u = 0; u < KEPT; ++u)
          if (lane + 64 * u < nv)
#pragma unroll
            for (int pw = 0; pw < PW; ++pw) *slot(w, u, pw) = acc[u][2 * pw] | (2 * pw + 1 < W ? acc[u][(2 * pw + 1) % W] << 16 : 0u);
      }
    }
    if (live) write_row<W, KEPT, VEC4>(p, nseg, l, g, b, B, group_frames(g, l), nv, lane, acc, eps);
  }
}

inline bool disjoint(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa + abytes <= pb || pb + bbytes <= pa;
}

// W of the widest unit the widths allow: 16, 4 or 1 bytes, so that no unit straddles a segment
inline int width_unit(int nseg, const int64_t* widths) {
  int W = 16;
  for (int s = 0; s < nseg; ++s) W = widths[s] % 16 == 0 ? W : (widths[s] % 4 == 0 ? (W < 4 ? W : 4) : 1);
  return W;
}

// the widths are a partition of D's columns into 1..MAX_SEGS positive parts
inline bool widths_ok(int64_t D, int nseg, const int64_t* widths) {
  if (nseg < 1 || nseg > MAX_SEGS || !widths) return false;
  int64_t sum = 0;
  for (int s = 0; s < nseg; ++s) {
    if (widths[s] <= 0 || widths[s] > 0x7fffffffLL) return false;
    sum += widths[s];
  }
  return sum == D;
}

inline int64_t lds_bytes(int64_t D, int W, int levels) {
  const int64_t upl = (D / W + 63) / 64;
  return ((int64_t)1 << (levels - 1)) * upl * packed_words(W) * 64 * 4;
}

// rows of D columns fit the lane's registers in units of W bytes, and the tree fits the LDS
inline bool fits(int64_t D, int W, int levels) {
  const int kept = W == 16 ? Unit<uint4>::KEPT : (W == 4 ? Unit<unsigned int>::KEPT : Unit<uint8_t>::KEPT);
  return D <= (int64_t)64 * kept * W && lds_bytes(D, W, levels) <= LDS_MAX;
}

template <typename V, bool VEC4>
void launch(const void* q, const int32_t* nf, const Pyramid& p, int64_t B, int64_t F, int64_t D, int levels, int nseg, float eps,
            hipStream_t s) {
  constexpr int W = Unit<V>::W;
  const int waves = 1 << (levels - 1);
  const int64_t nblk = ((F >> 1) + waves - 1) / waves;
  hipLaunchKernelGGL((frame_pyramid_kernel<V, VEC4>), dim3((unsigned)(B * nblk)), dim3(64 * waves), (size_t)lds_bytes(D, W, levels), s,
                     static_cast<const V*>(q), nf, p, B, F, (int)(D / W), levels, nseg, (int)nblk, eps);
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_frame_pyramid_supported(int64_t D, int nseg, const int64_t* widths, int levels) {
  if (D <= 0 || !widths_ok(D, nseg, widths) || levels < 1 || levels > MAX_LEVELS) return 0;
  return fits(D, width_unit(nseg, widths), levels) ? 1 : 0;
}

extern "C" int yt8m_frame_pyramid_u8(const uint8_t* q, const int32_t* num_frames, int64_t B, int64_t F, int64_t D, int levels, int nseg,
                                     const int64_t* widths, float* const* y, int32_t* const* num_frames_out, float eps,
                                     yt8m_stream_t stream) {
  YT8M_REQUIRE(B >= 0 && F >= 0 && D >= 0, YT8M_E_SHAPE, "negative dimension");
  YT8M_REQUIRE(levels >= 1 && levels <= 30 && ((int64_t)1 << levels) <= F, YT8M_E_BADARG, "levels must be >= 1 with 2^levels <= F");
  YT8M_REQUIRE(widths_ok(D, nseg, widths), YT8M_E_BADARG, "1 <= nseg <= 8 segments of positive widths that add up to D");
  YT8M_REQUIRE(eps > 0.f, YT8M_E_BADARG, "eps must be > 0");
  YT8M_REQUIRE(q && y, YT8M_E_BADARG, "null operand");
  for (int i = 0; i < levels * nseg; ++i) YT8M_REQUIRE(y[i], YT8M_E_BADARG, "null operand");
  const int64_t nblk = ((F >> 1) + ((int64_t)1 << (levels - 1)) - 1) >> (levels - 1);
  YT8M_REQUIRE(B * nblk <= 0x7fffffffLL && B * F <= ((int64_t)1 << 40), YT8M_E_SHAPE, "too many frames for one launch");
  if (B == 0) return YT8M_OK;
  // out of place: every output disjoint from the bytes, from num_frames and from every other output
  struct Span { const void* p; int64_t n; };
  Span spans[MAX_LEVELS * MAX_SEGS + MAX_LEVELS + 2];
  int ns = 0;
  bool shapes = levels <= MAX_LEVELS;
  for (int l = 0; l < levels && shapes; ++l) {
    for (int s = 0; s < nseg; ++s) spans[ns++] = Span{y[l * nseg + s], (F >> (l + 1)) * B * widths[s] * 4};
    if (num_frames_out && num_frames_out[l]) spans[ns++] = Span{num_frames_out[l], 4 * B};
  }
  const int nout = ns;
  spans[ns++] = Span{q, B * F * D};
  if (num_frames) spans[ns++] = Span{num_frames, 4 * B};
  for (int i = 0; i < nout; ++i)
    for (int k = i + 1; k < ns; ++k)
      YT8M_REQUIRE(disjoint(spans[i].p, spans[i].n, spans[k].p, spans[k].n), YT8M_E_BADARG,
                   "an output overlaps another operand (the pyramid is written out of place)");
  // the load unit the widths AND the operands' alignment allow
  int W = width_unit(nseg, widths);
  bool vec4 = W >= 4;
  for (int i = 0; shapes && i < levels * nseg; ++i) vec4 = vec4 && (reinterpret_cast<uintptr_t>(y[i]) & 15) == 0;
  const uintptr_t qa = reinterpret_cast<uintptr_t>(q);
  if (W == 16 && !(vec4 && (qa & 15) == 0)) W = 4;
  if (W == 4 && !(vec4 && (qa & 3) == 0)) W = 1;
  YT8M_REQUIRE(shapes && fits(D, W, levels), YT8M_E_SHAPE,
               "unsupported shape (see yt8m_frame_pyramid_supported; operands off a 16-byte line take narrower units)");
  Pyramid p;
  memset(&p, 0, sizeof(p));
  for (int l = 0; l < levels; ++l) {
    for (int s = 0; s < nseg; ++s) p.y[l * nseg + s] = y[l * nseg + s];
    p.nf_out[l] = num_frames_out ? num_frames_out[l] : nullptr;
  }
  for (int s = 0; s < nseg; ++s) p.off[s + 1] = p.off[s] + (int32_t)widths[s];
  hipStream_t s = as_stream(stream);
  double out_bytes = 0.0;
  for (int l = 0; l < levels; ++l) out_bytes += 4.0 * (double)((F >> (l + 1)) * B * D);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, (double)(B * F * D) + out_bytes);
  if (W == 16)
    launch<uint4, true>(q, num_frames, p, B, F, D, levels, nseg, eps, s);
  else if (W == 4)
    launch<unsigned int, true>(q, num_frames, p, B, F, D, levels, nseg, eps, s);
  else
    launch<uint8_t, false>(q, num_frames, p, B, F, D, levels, nseg, eps, s);
  return launch_status("frame_pyramid_kernel");
}
