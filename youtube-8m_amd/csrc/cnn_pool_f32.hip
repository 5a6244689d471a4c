// cnn_pool_f32.hip -- the backward of a max-pooled "einsum CNN" whose input is NOT data (gfx950, fp32): the chain of
// W/all_frame_models/lstm_cnn_deep_combine_chain_model.py reads the LSTM outputs x [F B rows (t B + b), D], so next to the filters' gradient
// (the fp32 twin of yt8m_u8_cnn_pool_dw) the input's gradient is needed.  d(loss)/d(cnn_output) is non-zero at ONE frame per (video,
// column) -- the argmax idx[b, n] the pooling kept -- so neither is a dense product:
//   yt8m_f32_cnn_pool_dw : dW[i D + d, n] = beta dW + sum_b g[b, n] x[(idx[b, n] - i) B + b, d]          (B gathered rows per (column, shift))
//   yt8m_f32_cnn_pool_dx : dx[(idx[b, n] - i) B + b, :] += g[b, n] W_k[i D : (i + 1) D, n]               (every CNN of the chain in ONE call)
// Bound: both are gathers of D-float rows from L2 / Infinity Cache: B sum_k fs_k N_k rows each (x rows for dw, rows of the transposed
// filters for dx); dx additionally writes its F B D output once.
#include "common.h"

namespace {

// block = (column n, shift i); thread = four consecutive features (a float4 of a frame row; D / 4 threads rounded up to whole waves).
// The B (coefficient, row) pairs of the column go through LDS first, as in u8_cnn_pool_dw_kernel; the sum over b runs in ascending b
// (blocks of eight products added up first, then onto the total): a fixed order, the same bits on every run.
__global__ __launch_bounds__(1024) void f32_cnn_pool_dw_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ idx,
                                                               const float* __restrict__ g, int64_t ldg, int B, int F, int D, int N,
                                                               float* __restrict__ dW, int64_t lddw, float beta) {
  __shared__ float s_coef[1024];
  __shared__ int s_row[1024];
  const int n = blockIdx.x, i = blockIdx.y;
  const int d4 = D >> 2, nt = (int)blockDim.x;
  const int t0 = threadIdx.x;
  const bool h0 = t0 < d4;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b0 = 0; b0 < B; b0 += nt) {
    const int b = b0 + t0;
    float coef = 0.f;
    int row = 0;
    if (b < B) {
      const int v = idx[(int64_t)b * ldg + n];
      const int t = v - i;                                            // the frame this shift read at the video's argmax
      if (t >= 0 && v < F) {                                          // (t < 0: the zero padding in front; v outside [0, F): no frame)
        coef = g[(int64_t)b * ldg + n];
        row = t * B + b;
      }
    }
    s_coef[t0] = coef;
    s_row[t0] = row;
    __syncthreads();
    const int nb = min(nt, B - b0);
    int j = 0;
    for (; j + 8 <= nb; j += 8) {                                     // eight independent row requests in flight per thread
      float4 u[8];
      float c[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        c[k] = s_coef[j + k];
        u[k] = h0 ? reinterpret_cast<const float4*>(x + (int64_t)s_row[j + k] * ldx)[t0] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      float4 p = make_float4(c[0] * u[0].x, c[0] * u[0].y, c[0] * u[0].z, c[0] * u[0].w);
#pragma unroll
      for (int k = 1; k < 8; ++k) {
        p.x += c[k] * u[k].x; p.y += c[k] * u[k].y; p.z += c[k] * u[k].z; p.w += c[k] * u[k].w;
      }
      a0.x += p.x; a0.y += p.y; a0.z += p.z; a0.w += p.w;
    }
    for (; j < nb; ++j) {
      const float c = s_coef[j];
      const float4 u = h0 ? reinterpret_cast<const float4*>(x + (int64_t)s_row[j] * ldx)[t0] : make_float4(0.f, 0.f, 0.f, 0.f);
      a0.x += c * u.x; a0.y += c * u.y; a0.z += c * u.z; a0.w += c * u.w;
    }
    __syncthreads();
  }
  if (h0) {
    float* col = dW + ((int64_t)i * D + 4 * t0) * lddw + n;
    const float v[4] = {a0.x, a0.y, a0.z, a0.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float* o = col + (int64_t)k * lddw;
      *o = beta != 0.f ? beta * *o + v[k] : v[k];
    }
  }
}

// Every filter of every CNN of the chain, in the column order of g / idx.  wt[k] = W_k^T [ncol[k] rows, fs[k] D]: row n holds the filter
// column n, so the walk over d of one (column, shift) term is contiguous.
constexpr int DX_MAX_FILTERS = 32;
struct DxDesc {
  int nfilt;
  int fs[DX_MAX_FILTERS], ncol[DX_MAX_FILTERS], cbase[DX_MAX_FILTERS];
  const float* wt[DX_MAX_FILTERS];
};

// block = (video b, group of WS feature slices of 128 floats) x WT frame classes: wave (ws, fc) owns the slice's two features per lane
// and the frames t = fc, fc + WT, ... -- a dx row slice has ONE owner, which adds its terms up in registers in a fixed order and writes
// it once (zeros where nothing points): no atomics, no accumulator in memory.
// Prologue (per block): the video's columns are sorted by key idx S + (S - fs) (S = the longest filter) -- counts with integer LDS atomics,
// a scan, then wave 0 places the columns chunk by chunk with ranks among equal keys taken in column order (a stable sort: the order of
// the terms of a row is a function of the inputs alone).  With that key the terms of frame t at shift i, the columns with idx = t + i and
// fs > i, are ONE contiguous range of the sorted list: [start[(t + i) S], start[(t + i) S + S - i]).
__global__ __launch_bounds__(1024) void f32_cnn_pool_dx_kernel(const int32_t* __restrict__ idx, const float* __restrict__ g, int64_t ldg, int B,
                                                               int F, int D, int S, int Ntot, DxDesc d, float* __restrict__ dx, int64_t lddx,
                                                               int WS, int WT) {
  extern __shared__ int4 dx_smem[];
  const int nkeys = F * S;
  const int nk4 = (nkeys + 1 + 3) & ~3;
  int* start = reinterpret_cast<int*>(dx_smem);                       // [nkeys + 1] entries with a smaller key
  int* cur = start + nk4;                                             // [nkeys] next free place of the key
  const float** rowp = reinterpret_cast<const float**>(cur + nk4);    // [Ntot] sorted: W^T row of the column
  float* coef = reinterpret_cast<float*>(rowp + Ntot);                // [Ntot] sorted: g[b, column]
  const int tid = threadIdx.x, nt = (int)blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int32_t* idx_b = idx + (int64_t)b * ldg;
  const float* g_b = g + (int64_t)b * ldg;

  auto key_of = [&](int c, int& k) -> int {                           // -1: the column contributes nothing
    k = 0;
    while (k + 1 < d.nfilt && c >= d.cbase[k + 1]) ++k;
    const int v = idx_b[c];
    return (v >= 0 && v < F) ? v * S + (S - d.fs[k]) : -1;
  };

  for (int j = tid; j <= nkeys; j += nt) start[j] = 0;
  __syncthreads();
  for (int c = tid; c < Ntot; c += nt) {
    int k;
    const int key = key_of(c, k);
    if (key >= 0) atomicAdd(&start[key + 1], 1);                      // (integer: the counts do not depend on the order)
  }
  __syncthreads();
  if (wave == 0) {                                                    // inclusive scan of start[1 .. nkeys], 64 at a time
    int carry = 0;
    for (int j0 = 1; j0 <= nkeys; j0 += 64) {
      const int j = j0 + lane;
      int v = j <= nkeys ? start[j] : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
      }
      v += carry;
      if (j <= nkeys) start[j] = v;
      carry = __shfl(v, 63, 64);
    }
  }
  __syncthreads();
  for (int j = tid; j < nkeys; j += nt) cur[j] = start[j];
  __syncthreads();
  if (wave == 0) {
    for (int c0 = 0; c0 < Ntot; c0 += 64) {
      const int c = c0 + lane;
      int k = 0;
      const int key = c < Ntot ? key_of(c, k) : -1;
      int rank = 0;
      bool last = true;                                               // no later column of this chunk has the key
      for (int l = 0; l < 64; ++l) {
        const int kl = __shfl(key, l, 64);
        rank += (kl == key && l < lane) ? 1 : 0;
        last = last && !(kl == key && l > lane);
      }
      if (key >= 0) {
        const int pos = cur[key] + rank;
        coef[pos] = g_b[c];
        rowp[pos] = d.wt[k] + (int64_t)(c - d.cbase[k]) * d.fs[k] * D;
        if (last) cur[key] = pos + 1;
      }
    }
  }
  __syncthreads();

  const int ws = wave % WS, fc = wave / WS;
  const int d0 = (blockIdx.y * WS + ws) * 128 + 2 * lane;
  if (fc >= WT || (blockIdx.y * WS + ws) * 128 >= D) return;          // (whole waves: nothing after this point synchronises)
  const bool live = d0 < D;                                           // D % 2 == 0: both features or none
  for (int t = fc; t < F; t += WT) {
    float2 acc = make_float2(0.f, 0.f);
    for (int i = 0; i < S && t + i < F; ++i) {
      const int kb = (t + i) * S;
      const int p1 = start[kb + S - i];
      const int64_t off = (int64_t)i * D + d0;
      int p = start[kb];
      for (; p + 4 <= p1; p += 4) {                                   // four independent row requests in flight per lane
        float c[4];
        float2 u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          c[k] = coef[p + k];
          u[k] = live ? *reinterpret_cast<const float2*>(rowp[p + k] + off) : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { acc.x += c[k] * u[k].x; acc.y += c[k] * u[k].y; }
      }
      for (; p < p1; ++p) {
        const float c = coef[p];
        const float2 u = live ? *reinterpret_cast<const float2*>(rowp[p] + off) : make_float2(0.f, 0.f);
        acc.x += c * u.x; acc.y += c * u.y;
      }
    }
    if (live) *reinterpret_cast<float2*>(dx + ((int64_t)t * B + b) * lddx + d0) = acc;
  }
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_f32_cnn_pool_dw(const float* x, int64_t ldx, const int32_t* idx, const float* g, int64_t ldg, int64_t B, int64_t F,
                                    int64_t D, int64_t N, int64_t fs, float* dW, int64_t lddw, float beta, yt8m_stream_t stream) {
  YT8M_REQUIRE(B >= 0 && F >= 1 && D >= 4 && N >= 0 && fs >= 1 && fs <= 16, YT8M_E_SHAPE, "bad dimension");
  if (N == 0) return YT8M_OK;
  YT8M_REQUIRE((D % 4) == 0 && D <= 4096 && (ldx % 4) == 0 && ldx >= D && ldg >= N && lddw >= N, YT8M_E_SHAPE,
               "D and ldx must be multiples of 4, D <= 4096, leading dimensions at least the row lengths");
  YT8M_REQUIRE(F * B < (int64_t)1 << 31, YT8M_E_SHAPE, "F B must fit 31 bits");
  YT8M_REQUIRE(beta == 0.f || beta == 1.f, YT8M_E_BADARG, "beta must be 0 or 1");
  YT8M_REQUIRE(dW && (B == 0 || (x && idx && g)), YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0, YT8M_E_BADARG, "x must be 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ProfScope prof(F_ELEMENTWISE, s);
  const unsigned nt = (unsigned)(((D / 4) + 63) / 64 * 64);
  hipLaunchKernelGGL(f32_cnn_pool_dw_kernel, dim3((unsigned)N, (unsigned)fs), dim3(nt), 0, s, x, ldx, idx, g, ldg, (int)B, (int)F, (int)D,
                     (int)N, dW, lddw, beta);
  return launch_status("f32_cnn_pool_dw_kernel");
}

extern "C" int yt8m_f32_cnn_pool_dx(const int32_t* idx, const float* g, int64_t ldg, int64_t B, int64_t F, int64_t D, int nfilt,
                                    const float* const* wt, const int32_t* fs, const int32_t* ncol, float* dx, int64_t lddx,
                                    yt8m_stream_t stream) {
  YT8M_REQUIRE(B >= 0 && F >= 1 && D >= 2 && nfilt >= 1 && nfilt <= DX_MAX_FILTERS && wt && fs && ncol, YT8M_E_SHAPE, "1..32 filters");
  DxDesc d;
  d.nfilt = nfilt;
  int S = 1;
  int64_t ntot = 0;
  for (int k = 0; k < DX_MAX_FILTERS; ++k) {
    if (k < nfilt) {
      YT8M_REQUIRE(fs[k] >= 1 && fs[k] <= 16 && ncol[k] >= 1, YT8M_E_SHAPE, "filter lengths 1..16, at least one column each");
      YT8M_REQUIRE(wt[k] && (reinterpret_cast<uintptr_t>(wt[k]) & 7) == 0, YT8M_E_BADARG, "null or misaligned transposed filter");
      d.fs[k] = fs[k]; d.ncol[k] = ncol[k]; d.cbase[k] = (int)ntot; d.wt[k] = wt[k];
      S = fs[k] > S ? fs[k] : S;
      ntot += ncol[k];
    } else {
      d.fs[k] = 1; d.ncol[k] = 0; d.cbase[k] = 0x7fffffff; d.wt[k] = nullptr;
    }
  }
  if (B == 0) return YT8M_OK;
  YT8M_REQUIRE((D % 2) == 0 && D <= 2048 && (lddx % 2) == 0 && lddx >= D && ldg >= ntot, YT8M_E_SHAPE,
               "D and lddx must be even, D <= 2048, leading dimensions at least the row lengths");
  YT8M_REQUIRE(F * B < (int64_t)1 << 31 && ntot < (int64_t)1 << 20, YT8M_E_SHAPE, "F B must fit 31 bits");
  YT8M_REQUIRE(idx && g && dx, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE((reinterpret_cast<uintptr_t>(dx) & 7) == 0, YT8M_E_BADARG, "dx must be 8-byte aligned");
  const int64_t nk4 = (F * S + 1 + 3) & ~(int64_t)3;
  const int64_t lds = 2 * nk4 * 4 + ntot * 12;
  YT8M_REQUIRE(lds <= 160 * 1024, YT8M_E_SHAPE, "F max(fs) and the number of columns do not fit the LDS (8 F max(fs) + 12 columns bytes <= 160 KiB)");
  const int nslice = (int)((D + 127) / 128);
  const int ny = (nslice + 3) / 4;                                    // at most four slices per block ...
  const int WS = (nslice + ny - 1) / ny;                              // ... shared out evenly
  const int WT = 16 / WS;                                             // frame classes: up to 16 waves per block
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  static DeviceOnce once;
  YT8M_HIP_CHECK(once.lds(reinterpret_cast<const void*>(f32_cnn_pool_dx_kernel), 160 * 1024));
  ProfScope prof(F_ELEMENTWISE, s);
  hipLaunchKernelGGL(f32_cnn_pool_dx_kernel, dim3((unsigned)B, (unsigned)ny), dim3((unsigned)(WS * WT * 64)), (size_t)lds, s, idx, g, ldg, (int)B,
                     (int)F, (int)D, S, (int)ntot, d, dx, lddx, WS, WT);
  return launch_status("f32_cnn_pool_dx_kernel");
}
