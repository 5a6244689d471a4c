// bigate_lstm.hip -- the scalar-gate LSTM cell of gate_lstm.hip as a recurrence that walks every video's frames in an order of its
// own while every time-indexed operand the caller sees stays in FRAME order (gfx950, wave64).  LstmBigluModel
// (Z/frame_level_models.py:887-1158) runs the cell of :975-1032 over tf.reverse_sequence(model_input, num_frames) and hands
// tf.reverse_sequence of its hidden outputs to a second cell (:1034-1101) that runs over the frames in order.  With
//       r(i, b) = n_b - 1 - i  while i < n_b,  else i          (n_b = num_frames[b] clamped to [0, F]: yt8m_reverse_sequence_u8's rule)
// -- for every b a bijection of 0..F-1 -- step i of row b reads its hoisted pre-activations at frame r(i, b) and writes its hidden
// output to y[r(i, b), b]: the first pass then needs no reversed copy of the frames and the second reads y as it lies.
// Per step there is one grouped-GEMM launch h_i . [Uog|Uc] into a contiguous [B, 2H] scratch (beta = 0: the rows of one step sit at
// different frames, so the product cannot accumulate into them) and one pointwise kernel, one workgroup per batch row, which adds the
// scratch row to the row at frame r and otherwise does what gate_lstm_fwd_kernel does.  The frame index is block-uniform: one scalar
// load and a compare per workgroup.
#include <stdlib.h>
#include "step_kernels.h"

namespace {

// frame that step i of row b visits; num_frames outside [0, F] is clamped as the reversal kernels of sequence.hip clamp it
__device__ __forceinline__ int64_t frame_of(const int32_t* __restrict__ nf, int64_t b, int64_t i, int64_t F, int reverse) {
  if (!reverse) return i;
  const int64_t n = clamp_frames(nf, b, F);
  return i < n ? n - 1 - i : i;
}

// One workgroup per batch row; PT = compile-time units per thread (H <= 256 PT, H % 256 == 0).  With r the row's frame at step i:
// the zv row [2H] at (r B + b) ldz arrives as x.[Wog|Wc] + [bog|bc], takes the row of rec = h_i . [Uog|Uc] and leaves as o | g; the
// zs row at (r B + b) lds arrives as x.[Wi|Wf] + [bi|bf] in columns 0, 1 and leaves as i | f (no other column of either row is
// touched).  y and hprev [F,B,H] are written at frame r, c_new / h_new [B,H] are the step-order states.  Everything the kernel reads is
// requested before the reduction.
template <int PT>
__global__ __launch_bounds__(256) void gate_frames_fwd_kernel(float* __restrict__ zv, int64_t ldz, float* __restrict__ zs, int64_t lds,
                                                              const float* __restrict__ rec, const float* __restrict__ Us,
                                                              const float* __restrict__ c_prev, const float* __restrict__ h_prev,
                                                              float* __restrict__ c_new, float* __restrict__ h_new,
                                                              float* __restrict__ y, float* __restrict__ hprev,
                                                              float* __restrict__ c_last, const int32_t* __restrict__ nf, int reverse,
                                                              int i, int64_t F, int64_t B, int64_t H) {
  __shared__ float red[8];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t row = frame_of(nf, b, i, F, reverse) * B + b;          // block-uniform
  float* zr = zv + row * ldz;
  float* sr = zs + row * lds;
  const float* rr = rec + b * 2 * H;
  const float zi = sr[0], zf = sr[1];
  const bool last = c_last && nf && (i + 1 == nf[b]);                  // block-uniform
  float zo[PT], zg[PT], cp[PT], hp[PT], ui[PT], uf[PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    const bool in = h < H;
    zo[p] = in ? zr[h] + rr[h] : 0.f;
    zg[p] = in ? zr[H + h] + rr[H + h] : 0.f;
    cp[p] = in ? c_prev[b * H + h] : 0.f;
    hp[p] = in ? h_prev[b * H + h] : 0.f;
    ui[p] = in ? Us[h] : 0.f;
    uf[p] = in ? Us[H + h] : 0.f;
  }
  float s[2] = {0.f, 0.f};                                             // h.Ui, h.Uf
#pragma unroll
  for (int p = 0; p < PT; ++p) { s[0] += hp[p] * ui[p]; s[1] += hp[p] * uf[p]; }
  block_sums_256<2>(s, red);
  const float ig = fast_sigmoid(zi + s[0]), fg = fast_sigmoid(zf + s[1]);
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) {
      const float o = fast_sigmoid(zo[p]), g = fast_tanh(zg[p]);
      const float cn = fg * cp[p] + ig * g;
      const float hn = o * fast_tanh(cn);
      zr[h] = o;
      zr[H + h] = g;
      c_new[b * H + h] = cn;
      h_new[b * H + h] = hn;
      y[row * H + h] = hn;
      hprev[row * H + h] = hp[p];
      if (last) c_last[b * H + h] = cn;
    }
  }
  if (tid == 0) { sr[0] = ig; sr[1] = fg; }
}

// The step's gradients: the dzv row [2H] (w.r.t. the pre-activations of o | g) goes to (r B + b) lddz and, for the step's product
// dz . [Uog|Uc]^T, to row b of the contiguous dzc [B, 2H]; the dzs row (w.r.t. those of i | f) to columns 0, 1 at (r B + b) ldds.  dy
// [F,B,H] (optional) is read at frame r; c_prev / c_new and the running gradients are step-order [B,H].  dh_prev receives the scalar
// gates' part; the caller adds dzc . [Uog|Uc]^T.  A row past its num_frames has dh = dc = 0 when nothing arrives through dy, and every
// product below is then exactly zero.
template <int PT>
__global__ __launch_bounds__(256) void gate_frames_bwd_kernel(const float* __restrict__ zv, int64_t ldz, const float* __restrict__ zs,
                                                              int64_t lds, const float* __restrict__ Us,
                                                              const float* __restrict__ c_prev, const float* __restrict__ c_new,
                                                              const float* __restrict__ dh_cur, const float* __restrict__ dc_cur,
                                                              const float* __restrict__ dy, const float* __restrict__ dc_last,
                                                              float* __restrict__ dzv, int64_t lddz, float* __restrict__ dzc,
                                                              float* __restrict__ dzs, int64_t ldds, float* __restrict__ dc_prev,
                                                              float* __restrict__ dh_prev, const int32_t* __restrict__ nf, int reverse,
                                                              int i, int64_t F, int64_t B, int64_t H) {
  __shared__ float red[8];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t row = frame_of(nf, b, i, F, reverse) * B + b;          // block-uniform
  const float* zr = zv + row * ldz;
  const float ig = zs[row * lds], fg = zs[row * lds + 1];
  const bool last = dc_last && nf && (i + 1 == nf[b]);                 // block-uniform
  float ov[PT], gv[PT], cpv[PT], cnv[PT], dhv[PT], dcv[PT], ui[PT], uf[PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    const bool in = h < H;
    ov[p] = in ? zr[h] : 0.f;
    gv[p] = in ? zr[H + h] : 0.f;
    cpv[p] = in ? c_prev[b * H + h] : 0.f;
    cnv[p] = in ? c_new[b * H + h] : 0.f;
    dhv[p] = in ? dh_cur[b * H + h] : 0.f;
    dcv[p] = in ? dc_cur[b * H + h] : 0.f;
    if (dy && in) dhv[p] += dy[row * H + h];
    if (last && in) dcv[p] += dc_last[b * H + h];
    ui[p] = in ? Us[h] : 0.f;
    uf[p] = in ? Us[H + h] : 0.f;
  }
  float s[2] = {0.f, 0.f};                                             // sum dc g, sum dc c_prev
  float* dzr = dzv + row * lddz;
  float* dcr = dzc + b * 2 * H;
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) {
      const float tc = fast_tanh(cnv[p]);
      const float dh = dhv[p], o = ov[p], g = gv[p];
      const float dc = dcv[p] + dh * o * (1.0f - tc * tc);
      const float dzo = dh * tc * o * (1.0f - o), dzg = dc * ig * (1.0f - g * g);
      dzr[h] = dzo;
      dzr[H + h] = dzg;
      dcr[h] = dzo;
      dcr[H + h] = dzg;
      dc_prev[b * H + h] = dc * fg;
      s[0] += dc * g;
      s[1] += dc * cpv[p];
    }
  }
  block_sums_256<2>(s, red);
  const float dzi = s[0] * ig * (1.0f - ig), dzf = s[1] * fg * (1.0f - fg);
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) dh_prev[b * H + h] = dzi * ui[p] + dzf * uf[p];
  }
  if (tid == 0) { dzs[row * ldds] = dzi; dzs[row * ldds + 1] = dzf; }
}

}  // namespace

using namespace yt8m;

// the shapes of yt8m_gate_lstm_supported: the same row-per-workgroup kernels
extern "C" int yt8m_gate_lstm_frames_supported(int64_t B, int64_t H) {
  return (B >= 1 && B < (1LL << 31) && H >= 256 && H % 256 == 0 && H <= 256 * ROW_PT) ? 1 : 0;
}

extern "C" int yt8m_gate_lstm_frames_fwd(float* zv, int64_t ldz, float* zs, int64_t lds, const float* Uv, int64_t ldu, const float* Us,
                                         float* y, float* hprev, float* cs, float* c_last, float* work, const int32_t* num_frames,
                                         int reverse, int64_t F, int64_t B, int64_t H, void* gemm_workspace,
                                         int64_t gemm_workspace_bytes, yt8m_stream_t stream) {
  YT8M_REQUIRE(F >= 0 && B >= 0 && H >= 0, YT8M_E_SHAPE, "negative dimension");
  if (F * B * H == 0) return YT8M_OK;
  YT8M_REQUIRE(zv && zs && Uv && Us && y && hprev && cs && work, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(reverse == 0 || reverse == 1, YT8M_E_BADARG, "reverse must be 0 or 1");
  YT8M_REQUIRE(num_frames || (!c_last && !reverse), YT8M_E_BADARG, "c_last and reverse need num_frames");
  YT8M_REQUIRE(ldz >= 2 * H && ldu >= 2 * H && lds >= 2, YT8M_E_SHAPE, "leading dimension too small");
  YT8M_REQUIRE(yt8m_gate_lstm_frames_supported(B, H), YT8M_E_SHAPE, "gate_lstm_frames supports H % 256 == 0, H <= 2048");
  hipStream_t s = as_stream(stream);
  const int64_t BH = B * H;
  if (c_last) YT8M_HIP_CHECK(hipMemsetAsync(c_last, 0, BH * sizeof(float), s));       // rows with num_frames < 1 (or > F) keep zeros
  // work: the step-order ping-pong of h [2, B, H] (h_0 = 0) and the recurrent product of one step [B, 2H]
  float* hb[2] = {work, work + BH};
  float* rec = work + 2 * BH;
  YT8M_HIP_CHECK(hipMemsetAsync(hb[0], 0, BH * sizeof(float), s));
  auto kfn = YT8M_ROW_KERNEL(gate_frames_fwd_kernel, H, 1);
  for (int64_t i = 0; i < F; ++i) {
    const float* h_cur = hb[i & 1];
    const yt8m_gemm_problem pr = {B, 2 * H, H, h_cur, H, Uv, ldu, rec, 2 * H, nullptr, 0.0f};            // rec = h_i . [Uog|Uc]
    int rc = yt8m_gemm_f32_grouped(0, 0, 1, &pr, gemm_workspace, gemm_workspace_bytes, stream);
    if (rc != YT8M_OK) return rc;
    ProfScope prof(F_LSTM, s);
    hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, zv, ldz, zs, lds, rec, Us, cs + i * BH, h_cur, cs + (i + 1) * BH,
                       hb[(i + 1) & 1], y, hprev, c_last, num_frames, reverse, (int)i, F, B, H);
  }
  return launch_status("gate_frames_fwd_kernel");
}

extern "C" int yt8m_gate_lstm_frames_bwd(const float* zv, int64_t ldz, const float* zs, int64_t lds, const float* Uv, int64_t ldu,
                                         const float* Us, const float* cs, const float* dy, const float* dc_last, float* dzv,
                                         int64_t lddz, float* dzs, int64_t ldds, float* work, const int32_t* num_frames, int reverse,
                                         int64_t F, int64_t B, int64_t H, void* gemm_workspace, int64_t gemm_workspace_bytes,
                                         yt8m_stream_t stream) {
  YT8M_REQUIRE(F >= 0 && B >= 0 && H >= 0, YT8M_E_SHAPE, "negative dimension");
  if (F * B * H == 0) return YT8M_OK;
  YT8M_REQUIRE(zv && zs && Uv && Us && cs && dzv && dzs && work, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(reverse == 0 || reverse == 1, YT8M_E_BADARG, "reverse must be 0 or 1");
  YT8M_REQUIRE(num_frames || (!dc_last && !reverse), YT8M_E_BADARG, "dc_last and reverse need num_frames");
  YT8M_REQUIRE(ldz >= 2 * H && lddz >= 2 * H && ldu >= 2 * H && lds >= 2 && ldds >= 2, YT8M_E_SHAPE,
               "leading dimension too small");
  YT8M_REQUIRE(yt8m_gate_lstm_frames_supported(B, H), YT8M_E_SHAPE, "gate_lstm_frames supports H % 256 == 0, H <= 2048");
  hipStream_t s = as_stream(stream);
  const int64_t BH = B * H;
  // work: the running gradients [4, B, H] and the contiguous copy of the step's dzv rows [B, 2H]
  StateGrads g(work, 0, BH);
  float* dzc = work + 4 * BH;
  YT8M_HIP_CHECK(seed_state(g.dh_cur, nullptr, BH, s));
  YT8M_HIP_CHECK(seed_state(g.dc_cur, nullptr, BH, s));
  // dzc . [Uog|Uc]^T as in yt8m_gate_lstm_layer_bwd: the packed step launcher where the workspace holds the packed weights,
  // YT8M_GATE_LSTM_PACKED_BWD=0 (read at every call) keeps the grouped GEMM
  const char* sw = getenv("YT8M_GATE_LSTM_PACKED_BWD");
  const bool packed = !(sw && atoi(sw) == 0) && packed_fits(B, H, 2, gemm_workspace, gemm_workspace_bytes);
  float* Wq = packed ? static_cast<float*>(gemm_workspace) : nullptr;
  if (packed) {
    int rc = cell_pack_scoped(Uv, ldu, nullptr, Wq, H, 2, s);
    if (rc != YT8M_OK) return rc;
  }
  const StepProduct rec = {Uv, ldu, nullptr, Wq, 2, B, H, gemm_workspace, gemm_workspace_bytes, stream};
  auto kfn = YT8M_ROW_KERNEL(gate_frames_bwd_kernel, H, 1);
  for (int64_t i = F - 1; i >= 0; --i, g.swap()) {
    {
      ProfScope prof(F_LSTM, s);
      hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, zv, ldz, zs, lds, Us, cs + i * BH, cs + (i + 1) * BH, g.dh_cur,
                         g.dc_cur, dy, dc_last, dzv, lddz, dzc, dzs, ldds, g.dc_prev, g.dh_prev, num_frames, reverse, (int)i, F, B, H);
    }
    int rc = rec.add_dzWt(dzc, g.dh_prev);                                                             // dh_prev += dzc . [Uog|Uc]^T
    if (rc != YT8M_OK) return rc;
  }
  return launch_status("gate_frames_bwd_kernel");
}
