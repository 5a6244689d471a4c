// memory_link.hip -- what turns the final memories of the multi-LSTM chain plugins' stacks into a stage's classifier input, in one pass
// each way (gfx950, wave64; launch-latency-bound: the tensors are [B, 1024..2304] and live in L2):
//   fwd:  y = [src_0 | src_1 | ...] (normalize = 0: an exact copy), or y = concat * rsqrt(max(sum concat^2, eps)) with
//         rinv[row] = +-r (sign: ss > eps), the definition of l2norm_fwd_kernel and chain_link.hip
//   bwd:  d = dy (normalize = 0), or R (dy - y (y.dy)) if rinv > 0 else R dy, R = |rinv| (from the output);
//         dsrc_s = the columns of segment s, written as a contiguous [rows, width_s] tensor -- the dc_final operands of
//         yt8m_lstm_stack_bwd
// i.e. torch.cat -> yt8m_l2norm_fwd_f32 and yt8m_l2norm_bwd_f32 -> one slice copy per segment without the concatenated tensors in between
// (call sites: W/all_frame_models/lstm_memory_deep_chain_model.py:72, distillchain_lstm_memory_deep_combine_chain_model.py:57,74,97,
// lstm_parallel_memory_model.py:62-65).  The segment table (<= 16 pointers and widths) travels by value in the kernel arguments.
// One workgroup of one wave per row; a row of up to 1024 columns stays in registers between the reduction and the write: one global read
// per element, 16-byte accesses where every width % 4 == 0 and every operand is 16-byte aligned (no access straddles a segment then).
// Wider rows are read twice.  Per-lane sums in pass order, then the wave butterfly: a fixed order, no atomics, no LDS.
#include <math.h>
#include "common.h"

namespace {

constexpr int MAX_SEGS = 16;
constexpr int REG_COLS = 1024;           // widest register-resident row: 16 floats per lane
constexpr int PASSES = REG_COLS / 64;    // single-element passes of a wave over such a row
constexpr int PASSES4 = REG_COLS / 256;  // 16-byte passes

struct Segs {                            // by value: segment s is [rows, width[s]] contiguous at p[s]; bwd: a null p[s] is skipped
  float* p[MAX_SEGS];
  int64_t width[MAX_SEGS];
};

// q with q[c] the row's element at concatenated column c (nullptr: a skipped segment).  The loop is wave-uniform: the table is read with
// scalar loads, a lane only selects.
__device__ __forceinline__ float* seg_at(const Segs& g, int nseg, int64_t row, int c) {
  uintptr_t q = reinterpret_cast<uintptr_t>(g.p[0]);
  if (q) q += (uintptr_t)(row * g.width[0]) * sizeof(float);
  int64_t off = g.width[0];
  for (int s = 1; s < nseg; ++s) {
    uintptr_t qs = reinterpret_cast<uintptr_t>(g.p[s]);
    if (qs) qs += (uintptr_t)(row * g.width[s] - off) * sizeof(float);
    q = (int64_t)c >= off ? qs : q;
    off += g.width[s];
  }
  return reinterpret_cast<float*>(q);
}


// VEC: every width % 4 == 0 and every segment, y 16-byte aligned (checked by the caller).  reps = 1 / sqrt(eps), rounded once on the host.
template <bool VEC>
__global__ __launch_bounds__(64) void memory_link_fwd_kernel(Segs g, int nseg, int normalize, float* __restrict__ y,
                                                             float* __restrict__ rinv, int cols, float eps, float reps) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  float* yr = y + row * cols;
  const int n4 = cols >> 2;
  if (!normalize) {                                                      // the concatenation itself
    if (VEC) {
      for (int c4 = lane; c4 < n4; c4 += 64)
        reinterpret_cast<float4*>(yr)[c4] = *reinterpret_cast<const float4*>(seg_at(g, nseg, row, 4 * c4) + 4 * c4);
    } else {
      for (int c = lane; c < cols; c += 64) yr[c] = seg_at(g, nseg, row, c)[c];
    }
    return;
  }
  float ss = 0.f;
  if (cols <= REG_COLS) {
    float a[PASSES];
    if (VEC) {
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < n4) q = *reinterpret_cast<const float4*>(seg_at(g, nseg, row, 4 * c4) + 4 * c4);
        a[4 * p] = q.x; a[4 * p + 1] = q.y; a[4 * p + 2] = q.z; a[4 * p + 3] = q.w;
        ss += (q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        const float v = c < cols ? seg_at(g, nseg, row, c)[c] : 0.f;
        a[p] = v;
        ss += v * v;
      }
    }
    ss = wave_sum(ss);
    const float r = link_r(ss, eps, reps);
    if (VEC) {
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        if (c4 < n4)
          reinterpret_cast<float4*>(yr)[c4] = make_float4(a[4 * p] * r, a[4 * p + 1] * r, a[4 * p + 2] * r, a[4 * p + 3] * r);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        if (c < cols) yr[c] = a[p] * r;
      }
    }
    if (lane == 0) rinv[row] = ss > eps ? r : -r;
    return;
  }
  // wide rows: the sources are read twice
  if (VEC) {
    for (int c4 = lane; c4 < n4; c4 += 64) {
      const float4 q = *reinterpret_cast<const float4*>(seg_at(g, nseg, row, 4 * c4) + 4 * c4);
      ss += (q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w);
    }
  } else {
    for (int c = lane; c < cols; c += 64) {
      const float v = seg_at(g, nseg, row, c)[c];
      ss += v * v;
    }
  }
  ss = wave_sum(ss);
  const float r = link_r(ss, eps, reps);
  if (VEC) {
    for (int c4 = lane; c4 < n4; c4 += 64) {
      const float4 q = *reinterpret_cast<const float4*>(seg_at(g, nseg, row, 4 * c4) + 4 * c4);
      reinterpret_cast<float4*>(yr)[c4] = make_float4(q.x * r, q.y * r, q.z * r, q.w * r);
    }
  } else {
    for (int c = lane; c < cols; c += 64) yr[c] = seg_at(g, nseg, row, c)[c] * r;
  }
  if (lane == 0) rinv[row] = ss > eps ? r : -r;
}

// VEC: every width % 4 == 0 and y, dy, every non-null segment 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(64) void memory_link_bwd_kernel(Segs g, int nseg, int normalize, const float* __restrict__ y,
                                                             const float* __restrict__ rinv, const float* __restrict__ dy, int cols) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* gr = dy + row * cols;
  const int n4 = cols >> 2;
  if (!normalize) {                                                      // the column windows of dy
    if (VEC) {
      for (int c4 = lane; c4 < n4; c4 += 64) {
        float* d = seg_at(g, nseg, row, 4 * c4);
        if (d) *reinterpret_cast<float4*>(d + 4 * c4) = reinterpret_cast<const float4*>(gr)[c4];
      }
    } else {
      for (int c = lane; c < cols; c += 64) {
        float* d = seg_at(g, nseg, row, c);
        if (d) d[c] = gr[c];
      }
    }
    return;
  }
  const float* yr = y + row * cols;
  const float ri = rinv[row], R = fabsf(ri);
  const bool unit = ri > 0.f;                                           // the row was divided by its own norm (ss > eps)
  float yg = 0.f;
  if (cols <= REG_COLS) {
    float yv[PASSES], gv[PASSES];
    if (VEC) {
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), q = a;
        if (c4 < n4) {
          a = reinterpret_cast<const float4*>(yr)[c4];
          q = reinterpret_cast<const float4*>(gr)[c4];
        }
        yv[4 * p] = a.x; yv[4 * p + 1] = a.y; yv[4 * p + 2] = a.z; yv[4 * p + 3] = a.w;
        gv[4 * p] = q.x; gv[4 * p + 1] = q.y; gv[4 * p + 2] = q.z; gv[4 * p + 3] = q.w;
        yg += (a.x * q.x + a.y * q.y) + (a.z * q.z + a.w * q.w);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        const bool in = c < cols;
        yv[p] = in ? yr[c] : 0.f;
        gv[p] = in ? gr[c] : 0.f;
        yg += yv[p] * gv[p];
      }
    }
    const float k = wave_sum(yg);
    float d[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) d[p] = unit ? R * (gv[p] - yv[p] * k) : R * gv[p];
    if (VEC) {
#pragma unroll
      for (int p = 0; p < PASSES4; ++p) {
        const int c4 = lane + 64 * p;
        if (c4 < n4) {
          float* o = seg_at(g, nseg, row, 4 * c4);
          if (o) *reinterpret_cast<float4*>(o + 4 * c4) = make_float4(d[4 * p], d[4 * p + 1], d[4 * p + 2], d[4 * p + 3]);
        }
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c = lane + 64 * p;
        if (c < cols) {
          float* o = seg_at(g, nseg, row, c);
          if (o) o[c] = d[p];
        }
      }
    }
    return;
  }
  // wide rows: y and dy are read twice
  if (VEC) {
    for (int c4 = lane; c4 < n4; c4 += 64) {
      const float4 a = reinterpret_cast<const float4*>(yr)[c4], q = reinterpret_cast<const float4*>(gr)[c4];
      yg += (a.x * q.x + a.y * q.y) + (a.z * q.z + a.w * q.w);
    }
  } else {
    for (int c = lane; c < cols; c += 64) yg += yr[c] * gr[c];
  }
  const float k = wave_sum(yg);
  if (VEC) {
    for (int c4 = lane; c4 < n4; c4 += 64) {
      float* o = seg_at(g, nseg, row, 4 * c4);
      if (!o) continue;
      const float4 a = reinterpret_cast<const float4*>(yr)[c4], q = reinterpret_cast<const float4*>(gr)[c4];
      *reinterpret_cast<float4*>(o + 4 * c4) = unit ? make_float4(R * (q.x - a.x * k), R * (q.y - a.y * k), R * (q.z - a.z * k), R * (q.w - a.w * k))
                                                    : make_float4(R * q.x, R * q.y, R * q.z, R * q.w);
    }
  } else {
    for (int c = lane; c < cols; c += 64) {
      float* o = seg_at(g, nseg, row, c);
      if (o) o[c] = unit ? R * (gr[c] - yr[c] * k) : R * gr[c];
    }
  }
}

// Fills the table; false: nseg or a width out of range, or more than INT_MAX columns.  *vec: every width % 4 == 0.
inline bool fill_widths(int nseg, const int64_t* widths, Segs* g, int64_t* cols, bool* vec) {
  if (nseg < 1 || nseg > MAX_SEGS || !widths) return false;
  *cols = 0;
  *vec = true;
  for (int s = 0; s < MAX_SEGS; ++s) {
    g->p[s] = nullptr;
    g->width[s] = 0;
  }
  for (int s = 0; s < nseg; ++s) {
    if (widths[s] <= 0 || widths[s] > 0x7fffffffLL) return false;
    g->width[s] = widths[s];
    *cols += widths[s];
    *vec = *vec && (widths[s] & 3) == 0;
  }
  return *cols <= 0x7fffffffLL;
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_memory_link_fwd(int nseg, const float* const* src, const int64_t* widths, int normalize, float* y, float* rinv,
                                    int64_t rows, float eps, yt8m_stream_t stream) {
  Segs g;
  int64_t cols = 0;
  bool vec = false;
  YT8M_REQUIRE(fill_widths(nseg, widths, &g, &cols, &vec), YT8M_E_BADARG, "1 <= nseg <= 16 segments of positive widths (< 2^31 columns in all)");
  YT8M_REQUIRE(src && y && (rinv || !normalize), YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(rows > 0, YT8M_E_BADARG, "rows must be positive");
  YT8M_REQUIRE(eps > 0.f, YT8M_E_BADARG, "eps must be > 0");
  YT8M_REQUIRE(rows <= 0x7fffffffLL, YT8M_E_SHAPE, "too many rows");
  vec = vec && aligned16(y);
  for (int s = 0; s < nseg; ++s) {
    YT8M_REQUIRE(src[s], YT8M_E_BADARG, "null operand");
    g.p[s] = const_cast<float*>(src[s]);                                 // (read only: the forward kernel loads through the table)
    vec = vec && aligned16(src[s]);
  }
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const float reps = (float)(1.0 / sqrt((double)eps));
  const dim3 grid((unsigned)rows), block(64);
  if (vec)
    hipLaunchKernelGGL(memory_link_fwd_kernel<true>, grid, block, 0, s, g, nseg, normalize != 0, y, rinv, (int)cols, eps, reps);
  else
    hipLaunchKernelGGL(memory_link_fwd_kernel<false>, grid, block, 0, s, g, nseg, normalize != 0, y, rinv, (int)cols, eps, reps);
  return launch_status("memory_link_fwd_kernel");
}

extern "C" int yt8m_memory_link_bwd(int nseg, const int64_t* widths, int normalize, const float* y, const float* rinv, const float* dy,
                                    float* const* dsrc, int64_t rows, float eps, yt8m_stream_t stream) {
  Segs g;
  int64_t cols = 0;
  bool vec = false;
  YT8M_REQUIRE(fill_widths(nseg, widths, &g, &cols, &vec), YT8M_E_BADARG, "1 <= nseg <= 16 segments of positive widths (< 2^31 columns in all)");
  YT8M_REQUIRE(dy && dsrc && ((y && rinv) || !normalize), YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(rows > 0, YT8M_E_BADARG, "rows must be positive");
  YT8M_REQUIRE(eps > 0.f, YT8M_E_BADARG, "eps must be > 0");
  YT8M_REQUIRE(rows <= 0x7fffffffLL, YT8M_E_SHAPE, "too many rows");
  vec = vec && aligned16(dy) && (!normalize || aligned16(y));
  bool any = false;
  for (int s = 0; s < nseg; ++s) {
    g.p[s] = dsrc[s];                                                    // null: this segment's gradient is not wanted
    any = any || dsrc[s];
    vec = vec && aligned16(dsrc[s]);
  }
  if (!any) return YT8M_OK;
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const dim3 grid((unsigned)rows), block(64);
  if (vec)
    hipLaunchKernelGGL(memory_link_bwd_kernel<true>, grid, block, 0, s, g, nseg, normalize != 0, y, rinv, dy, (int)cols);
  else
    hipLaunchKernelGGL(memory_link_bwd_kernel<false>, grid, block, 0, s, g, nseg, normalize != 0, y, rinv, dy, (int)cols);
  return launch_status("memory_link_bwd_kernel");
}
