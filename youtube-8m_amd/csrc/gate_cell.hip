// gate_cell.hip -- the scalar-gate LSTM cell of Z/frame_level_models.py:1583-1640 (LstmGateModel.create_recurrent_unit; the same unit
// in LstmGateMultilayerModel, :1733-1790, and in both passes of LstmBigluModel, :975-1101), in the generic per-step form of cells.hip
// (gfx950, wave64):
//       i = sigmoid(x.Wi + h.Ui + bi)      [B,1]        f = sigmoid(x.Wf + h.Uf + bf)      [B,1]
//       o = sigmoid(x.Wog + h.Uog + bog)   [B,H]        g = tanh(x.Wc + h.Uc + bc)         [B,H]
//       c' = f * c + i * g                               h' = o * tanh(c')
// The input and the forget gate are ONE scalar per video; the loop is a plain tf.while_loop over all max_frames steps (no dynamic_rnn:
// no copy-through, no masking), and the head reads the memory c gathered at frame num_frames - 1.
// The input halves of the four projections are hoisted by the caller; per step there is one grouped-GEMM launch for h.[Uog|Uc] and one
// pointwise kernel, one workgroup per batch row, which reduces h.Ui and h.Uf over the row (forward) or sum_h dc g and sum_h dc c_prev
// (backward) on one barrier pair.  ONE kernel pair in two compile-time forms:
//   step order (FRAMES = false, yt8m_gate_lstm_layer_*): step t of every row is frame t.  The kernels get pointers offset to the step,
//     and the recurrent product accumulates into the step's zv rows in place (beta = 1).
//   frame order (FRAMES = true, yt8m_gate_lstm_frames_*): the recurrence walks every video's frames in an order of its own while every
//     time-indexed operand the caller sees stays in FRAME order.  LstmBigluModel runs the cell over
//     tf.reverse_sequence(model_input, num_frames) and hands tf.reverse_sequence of its hidden outputs to a second cell that runs over
//     the frames in order.  With
//       r(i, b) = n_b - 1 - i  while i < n_b,  else i       (n_b = num_frames[b] clamped to [0, F]: yt8m_reverse_sequence_u8's rule)
//     -- for every b a bijection of 0..F-1 -- step i of row b reads its hoisted pre-activations at frame r(i, b) and writes its hidden
//     output to y[r(i, b), b]: the first pass then needs no reversed copy of the frames and the second reads y as it lies.  The rows
//     of one step sit at different frames, so the product cannot accumulate into them: it goes to a contiguous [B, 2H] scratch
//     (beta = 0) whose row the kernel adds.  The frame index is block-uniform: one scalar load and a compare per workgroup.
// Step order stays a form of its own, not reverse = 0 of the frame-order kernels: it is the faster of the two per step (README).
#include <type_traits>
#include "step_kernels.h"

namespace {

// What the frame-order kernels take beside the step-order argument list, as one trailing argument: the step-order instantiations keep
// the kernel arguments they always had (one list for both forms cost them 0.2-0.6 us per forward step, a third 64-byte line of
// arguments per workgroup: profiles/gate_cell_refactor.txt).
struct StepOrder {};
struct FwdFrames {
  int64_t ldz;              // row stride of zv
  const float* rec;         // [B,2H] h_t . [Uog|Uc]
  float *y, *hprev;         // [F,B,H]
  int reverse;
  int64_t F, B;
};
struct BwdFrames {
  int64_t ldz, lddz, ldds;  // row strides of zv, dzv, dzs
  float* dzc;               // [B,2H] the step's dzv rows, contiguous
  int reverse;
  int64_t F, B;
};

// frame that step i of row b visits; num_frames outside [0, F] is clamped as the reversal kernels of sequence.hip clamp it
__device__ __forceinline__ int64_t frame_of(const int32_t* __restrict__ nf, int64_t b, int64_t i, int64_t F, int reverse) {
  if (!reverse) return i;
  const int64_t n = clamp_frames(nf, b, F);
  return i < n ? n - 1 - i : i;
}

// One workgroup per batch row; PT = compile-time units per thread (H <= 256 PT, H % 256 == 0).  The zv row [2H] arrives as
// x.[Wog|Wc] + [bog|bc] (step order: + h.[Uog|Uc]; frame order: the kernel adds the row of rec = h_t . [Uog|Uc]) and leaves as o | g; the
// zs row arrives as x.[Wi|Wf] + [bi|bf] in columns 0, 1 and leaves as i | f (no other column of either row is touched).  c_prev,
// h_prev, c_new, h_new [B,H] are the states of step t.
// Step order: zv [B,2H] and zs [B,lds] are the rows of step t.
// Frame order: with r the row's frame at step t, the rows are (r B + b) of zv (stride fr.ldz) and zs (stride lds), and fr.y and fr.hprev
// take h_new and h_prev at frame r.
// Everything the kernel reads is requested before the reduction.
template <int PT, bool FRAMES>
__global__ __launch_bounds__(256) void gate_cell_fwd_kernel(float* __restrict__ zv, float* __restrict__ zs, int64_t lds,
                                                            const float* __restrict__ Us, const float* __restrict__ c_prev,
                                                            const float* __restrict__ h_prev, float* __restrict__ c_new,
                                                            float* __restrict__ h_new, float* __restrict__ c_last,
                                                            const int32_t* __restrict__ nf, int t, int64_t H,
                                                            std::conditional_t<FRAMES, FwdFrames, StepOrder> fr) {
  __shared__ float red[8];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  int64_t row = b, ldz = 2 * H;
  const float* rr = nullptr;
  if constexpr (FRAMES) {
    row = frame_of(nf, b, t, fr.F, fr.reverse) * fr.B + b;             // block-uniform
    ldz = fr.ldz;
    rr = fr.rec + b * 2 * H;
  }
  float* zr = zv + row * ldz;
  float* sr = zs + row * lds;
  const float zi = sr[0], zf = sr[1];
  const bool last = c_last && nf && (t + 1 == nf[b]);                  // block-uniform
  float zo[PT], zg[PT], cp[PT], hp[PT], ui[PT], uf[PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    const bool in = h < H;
    zo[p] = !in ? 0.f : FRAMES ? zr[h] + rr[h] : zr[h];
    zg[p] = !in ? 0.f : FRAMES ? zr[H + h] + rr[H + h] : zr[H + h];
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
      if constexpr (FRAMES) {
        fr.y[row * H + h] = hn;
        fr.hprev[row * H + h] = hp[p];
      }
      if (last) c_last[b * H + h] = cn;
    }
  }
  if (tid == 0) { sr[0] = ig; sr[1] = fg; }
}

// The step's gradients: the dzv row [2H] = gradient w.r.t. the pre-activations of o | g, the dzs row, columns 0, 1 = those of i | f;
// the running gradients of the step before go to dc_prev / dh_prev (dh_prev = the scalar gates' part; the caller adds
// dzv . [Uog|Uc]^T).  c_prev / c_new and the running gradients are the [B,H] of step t.
// Step order: zv, zs (stride lds), dout (optional), dzv [B,2H] and dzs (stride lds) are the rows of step t.
// Frame order: with r the row's frame at step t, the rows are (r B + b) of zv (stride fr.ldz), zs (lds), dzv (fr.lddz) and dzs
// (fr.ldds); dout [F,B,H] (optional) is read at frame r, and the dzv row also goes to row b of fr.dzc, for the step's product.
// A row past its num_frames has dh = dc = 0 when nothing arrives through dout, and every product below is then exactly zero.
template <int PT, bool FRAMES>
__global__ __launch_bounds__(256) void gate_cell_bwd_kernel(const float* __restrict__ zv, const float* __restrict__ zs, int64_t lds,
                                                            const float* __restrict__ Us, const float* __restrict__ c_prev,
                                                            const float* __restrict__ c_new, const float* __restrict__ dh_cur,
                                                            const float* __restrict__ dc_cur, const float* __restrict__ dout,
                                                            const float* __restrict__ dc_last, float* __restrict__ dzv,
                                                            float* __restrict__ dzs, float* __restrict__ dc_prev,
                                                            float* __restrict__ dh_prev, const int32_t* __restrict__ nf, int t,
                                                            int64_t H, std::conditional_t<FRAMES, BwdFrames, StepOrder> fr) {
  __shared__ float red[8];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  int64_t row = b, ldz = 2 * H, lddz = 2 * H, ldds = lds;
  if constexpr (FRAMES) {
    row = frame_of(nf, b, t, fr.F, fr.reverse) * fr.B + b;             // block-uniform
    ldz = fr.ldz;
    lddz = fr.lddz;
    ldds = fr.ldds;
  }
  const float* zr = zv + row * ldz;
  const float ig = zs[row * lds], fg = zs[row * lds + 1];
  const bool last = dc_last && nf && (t + 1 == nf[b]);                 // block-uniform
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
    if (dout && in) dhv[p] += dout[row * H + h];
    if (last && in) dcv[p] += dc_last[b * H + h];
    ui[p] = in ? Us[h] : 0.f;
    uf[p] = in ? Us[H + h] : 0.f;
  }
  float s[2] = {0.f, 0.f};                                             // sum dc g, sum dc c_prev
  float* dzr = dzv + row * lddz;
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
      if constexpr (FRAMES) {
        fr.dzc[b * 2 * H + h] = dzo;
        fr.dzc[b * 2 * H + H + h] = dzg;
      }
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

// what the step kernels handle: whole 256-unit slices per thread slot, up to ROW_PT of them; one workgroup per row
extern "C" int yt8m_gate_lstm_supported(int64_t B, int64_t H) {
  return (B >= 1 && B < (1LL << 31) && H >= 256 && H % 256 == 0 && H <= 256 * ROW_PT) ? 1 : 0;
}

extern "C" int yt8m_gate_lstm_frames_supported(int64_t B, int64_t H) { return yt8m_gate_lstm_supported(B, H); }

// ---- step order: a tape of h, the recurrent product added in place --------------------------------------------------------
extern "C" int yt8m_gate_lstm_layer_fwd(float* zv, float* zs, int64_t lds, const float* Uv, int64_t ldu, const float* Us, float* hs,
                                        float* cs, float* c_last, const int32_t* num_frames, int64_t F, int64_t B, int64_t H,
                                        void* gemm_workspace, int64_t gemm_workspace_bytes, yt8m_stream_t stream) {
  YT8M_REQUIRE(F >= 0 && B >= 0 && H >= 0, YT8M_E_SHAPE, "negative dimension");
  if (F * B * H == 0) return YT8M_OK;
  YT8M_REQUIRE(zv && zs && Uv && Us && hs && cs, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(num_frames || !c_last, YT8M_E_BADARG, "c_last needs num_frames");
  YT8M_REQUIRE(ldu >= 2 * H && lds >= 2, YT8M_E_SHAPE, "leading dimension too small");
  YT8M_REQUIRE(yt8m_gate_lstm_supported(B, H), YT8M_E_SHAPE, "gate LSTM supports H % 256 == 0, H <= 2048");
  hipStream_t s = as_stream(stream);
  const int64_t BH = B * H;
  if (c_last) YT8M_HIP_CHECK(hipMemsetAsync(c_last, 0, BH * sizeof(float), s));       // rows with num_frames < 1 (or > F) keep zeros
  const StepProduct rec = {Uv, ldu, nullptr, nullptr, 2, B, H, gemm_workspace, gemm_workspace_bytes, stream};
  auto kfn = YT8M_ROW_KERNEL(gate_cell_fwd_kernel, H, 1, false);
  for (int64_t t = 0; t < F; ++t) {
    float* zvt = zv + t * B * 2 * H;
    int rc = rec.add_hW(hs + t * BH, zvt);                                                             // zv_t += h . [Uog|Uc]
    if (rc != YT8M_OK) return rc;
    ProfScope prof(F_LSTM, s);
    hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, zvt, zs + t * B * lds, lds, Us, cs + t * BH, hs + t * BH,
                       cs + (t + 1) * BH, hs + (t + 1) * BH, c_last, num_frames, (int)t, H, StepOrder{});
  }
  return launch_status("gate_cell_fwd_kernel");
}

extern "C" int yt8m_gate_lstm_layer_bwd(const float* zv, const float* zs, int64_t lds, const float* Uv, int64_t ldu, const float* Us,
                                        const float* hs, const float* cs, const float* dout, const float* dc_last, float* dzv,
                                        float* dzs, float* work, const int32_t* num_frames, int64_t F, int64_t B, int64_t H,
                                        void* gemm_workspace, int64_t gemm_workspace_bytes, yt8m_stream_t stream) {
  YT8M_REQUIRE(F >= 0 && B >= 0 && H >= 0, YT8M_E_SHAPE, "negative dimension");
  if (F * B * H == 0) return YT8M_OK;
  YT8M_REQUIRE(zv && zs && Uv && Us && hs && cs && dzv && dzs && work, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE(num_frames || !dc_last, YT8M_E_BADARG, "dc_last needs num_frames");
  YT8M_REQUIRE(ldu >= 2 * H && lds >= 2, YT8M_E_SHAPE, "leading dimension too small");
  YT8M_REQUIRE(yt8m_gate_lstm_supported(B, H), YT8M_E_SHAPE, "gate LSTM supports H % 256 == 0, H <= 2048");
  (void)hs;                                            // part of the layer's tape; the weight gradients over it are the caller's
  hipStream_t s = as_stream(stream);
  const int64_t BH = B * H;
  StateGrads g(work, 0, BH);
  YT8M_HIP_CHECK(seed_state(g.dh_cur, nullptr, BH, s));
  YT8M_HIP_CHECK(seed_state(g.dc_cur, nullptr, BH, s));
  // dzv . [Uog|Uc]^T on the packed step launcher of lstm_fused.hip (cell_step_bwd, G = 2: the GRU gate block's form) where the
  // workspace holds the packed weights; YT8M_GATE_LSTM_PACKED_BWD=0 keeps the grouped GEMM
  const float* Wq;
  int rc = packed_bwd_weights("YT8M_GATE_LSTM_PACKED_BWD", Uv, ldu, B, H, 2, gemm_workspace, gemm_workspace_bytes, s, &Wq);
  if (rc != YT8M_OK) return rc;
  const StepProduct rec = {Uv, ldu, nullptr, Wq, 2, B, H, gemm_workspace, gemm_workspace_bytes, stream};
  auto kfn = YT8M_ROW_KERNEL(gate_cell_bwd_kernel, H, 1, false);
  for (int64_t t = F - 1; t >= 0; --t, g.swap()) {
    float* dzvt = dzv + t * B * 2 * H;
    {
      ProfScope prof(F_LSTM, s);
      hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, zv + t * B * 2 * H, zs + t * B * lds, lds, Us, cs + t * BH,
                         cs + (t + 1) * BH, g.dh_cur, g.dc_cur, dout ? dout + t * BH : nullptr, dc_last, dzvt, dzs + t * B * lds,
                         g.dc_prev, g.dh_prev, num_frames, (int)t, H, StepOrder{});
    }
    rc = rec.add_dzWt(dzvt, g.dh_prev);                                                                // dh_prev += dzv_t . [Uog|Uc]^T
    if (rc != YT8M_OK) return rc;
  }
  return launch_status("gate_cell_bwd_kernel");
}

// ---- frame order: a ping-pong of h, the recurrent product and the step's dzv rows in contiguous scratch --------------------
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
  auto kfn = YT8M_ROW_KERNEL(gate_cell_fwd_kernel, H, 1, true);
  const FwdFrames fr = {ldz, rec, y, hprev, reverse, F, B};
  for (int64_t i = 0; i < F; ++i) {
    const float* h_cur = hb[i & 1];
    const yt8m_gemm_problem pr = {B, 2 * H, H, h_cur, H, Uv, ldu, rec, 2 * H, nullptr, 0.0f};            // rec = h_i . [Uog|Uc]
    int rc = yt8m_gemm_f32_grouped(0, 0, 1, &pr, gemm_workspace, gemm_workspace_bytes, stream);
    if (rc != YT8M_OK) return rc;
    ProfScope prof(F_LSTM, s);
    hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, zv, zs, lds, Us, cs + i * BH, h_cur, cs + (i + 1) * BH, hb[(i + 1) & 1],
                       c_last, num_frames, (int)i, H, fr);
  }
  return launch_status("gate_cell_fwd_kernel");
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
  // dzc . [Uog|Uc]^T as in yt8m_gate_lstm_layer_bwd, under the same switch
  const float* Wq;
  int rc = packed_bwd_weights("YT8M_GATE_LSTM_PACKED_BWD", Uv, ldu, B, H, 2, gemm_workspace, gemm_workspace_bytes, s, &Wq);
  if (rc != YT8M_OK) return rc;
  const StepProduct rec = {Uv, ldu, nullptr, Wq, 2, B, H, gemm_workspace, gemm_workspace_bytes, stream};
  auto kfn = YT8M_ROW_KERNEL(gate_cell_bwd_kernel, H, 1, true);
  const BwdFrames fr = {ldz, lddz, ldds, dzc, reverse, F, B};
  for (int64_t i = F - 1; i >= 0; --i, g.swap()) {
    {
      ProfScope prof(F_LSTM, s);
      hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, zv, zs, lds, Us, cs + i * BH, cs + (i + 1) * BH, g.dh_cur, g.dc_cur,
                         dy, dc_last, dzv, dzs, g.dc_prev, g.dh_prev, num_frames, (int)i, H, fr);
    }
    rc = rec.add_dzWt(dzc, g.dh_prev);                                                                 // dh_prev += dzc . [Uog|Uc]^T
    if (rc != YT8M_OK) return rc;
  }
  return launch_status("gate_cell_bwd_kernel");
}
