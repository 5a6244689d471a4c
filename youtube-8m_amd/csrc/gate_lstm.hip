// gate_lstm.hip -- the scalar-gate LSTM cell of Z/frame_level_models.py:1583-1640 (LstmGateModel.create_recurrent_unit; the same unit
// in LstmGateMultilayerModel, :1733-1790), in the generic per-step form of cells.hip (gfx950, wave64):
//       i = sigmoid(x.Wi + h.Ui + bi)      [B,1]        f = sigmoid(x.Wf + h.Uf + bf)      [B,1]
//       o = sigmoid(x.Wog + h.Uog + bog)   [B,H]        g = tanh(x.Wc + h.Uc + bc)         [B,H]
//       c' = f * c + i * g                               h' = o * tanh(c')
// The input and the forget gate are ONE scalar per video; the loop is a plain tf.while_loop over all max_frames steps (no dynamic_rnn:
// no copy-through, no masking), and the head reads the memory c gathered at frame num_frames - 1.
// The input halves of the four projections are hoisted by the caller; per step there is one grouped-GEMM launch for h.[Uog|Uc] and one
// pointwise kernel, one workgroup per batch row, which reduces h.Ui and h.Uf over the row (forward) or sum_h dc g and sum_h dc c_prev
// (backward) on one barrier pair.
#include <stdlib.h>
#include "step_kernels.h"

namespace {


// One workgroup per batch row; PT = compile-time units per thread (H <= 256 PT, H % 256 == 0).  zv row [2H] arrives as
// x.[Wog|Wc] + [bog|bc] + h.[Uog|Uc] and leaves as o | g; zs row (stride lds) arrives as x.[Wi|Wf] + [bi|bf] in columns 0, 1 and leaves
// as i | f (the other columns are not touched).  Everything the kernel reads is requested before the reduction.
template <int PT>
__global__ __launch_bounds__(256) void gate_lstm_fwd_kernel(float* __restrict__ zv, float* __restrict__ zs, int64_t lds,
                                                            const float* __restrict__ Us, const float* __restrict__ c_prev,
                                                            const float* __restrict__ h_prev, float* __restrict__ c_new,
                                                            float* __restrict__ h_new, float* __restrict__ c_last,
                                                            const int32_t* __restrict__ nf, int t, int64_t H) {
  __shared__ float red[8];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  float* zr = zv + b * 2 * H;
  float* sr = zs + b * lds;
  const float zi = sr[0], zf = sr[1];
  const bool last = c_last && nf && (t + 1 == nf[b]);                  // block-uniform
  float zo[PT], zg[PT], cp[PT], hp[PT], ui[PT], uf[PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    const bool in = h < H;
    zo[p] = in ? zr[h] : 0.f;
    zg[p] = in ? zr[H + h] : 0.f;
    cp[p] = in ? c_prev[b * H + h] : 0.f;
    hp[p] = in ? h_prev[b * H + h] : 0.f;
    ui[p] = in ? Us[h] : 0.f;
    uf[p] = in ? Us[H + h] : 0.f;
  }
  float s[2] = {0.f, 0.f};                                             // h.Ui, h.Uf
#pragma unroll
  for (int p = 0; p < PT; ++p) { s[0] += hp[p] * ui[p]; s[1] += hp[p] * uf[p]; }
  block_sums_256<2>(s, red);
  const float i = fast_sigmoid(zi + s[0]), f = fast_sigmoid(zf + s[1]);
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) {
      const float o = fast_sigmoid(zo[p]), g = fast_tanh(zg[p]);
      const float cn = f * cp[p] + i * g;
      zr[h] = o;
      zr[H + h] = g;
      c_new[b * H + h] = cn;
      h_new[b * H + h] = o * fast_tanh(cn);
      if (last) c_last[b * H + h] = cn;
    }
  }
  if (tid == 0) { sr[0] = i; sr[1] = f; }
}

// dzv row [2H] = gradient w.r.t. the pre-activations of o | g, dzs row (stride lds) columns 0, 1 = those of i | f; the running
// gradients of the step before go to dc_prev / dh_prev (dh_prev = the scalar gates' part; the caller adds dzv . [Uog|Uc]^T).
// A row past its num_frames has dh = dc = 0 when nothing arrives through dout, and every product below is then exactly zero.
template <int PT>
__global__ __launch_bounds__(256) void gate_lstm_bwd_kernel(const float* __restrict__ zv, const float* __restrict__ zs, int64_t lds,
                                                            const float* __restrict__ Us, const float* __restrict__ c_prev,
                                                            const float* __restrict__ c_new, const float* __restrict__ dh_cur,
                                                            const float* __restrict__ dc_cur, const float* __restrict__ dout,
                                                            const float* __restrict__ dc_last, float* __restrict__ dzv,
                                                            float* __restrict__ dzs, float* __restrict__ dc_prev,
                                                            float* __restrict__ dh_prev, const int32_t* __restrict__ nf, int t,
                                                            int64_t H) {
  __shared__ float red[8];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* zr = zv + b * 2 * H;
  const float i = zs[b * lds], f = zs[b * lds + 1];
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
    if (dout && in) dhv[p] += dout[b * H + h];
    if (last && in) dcv[p] += dc_last[b * H + h];
    ui[p] = in ? Us[h] : 0.f;
    uf[p] = in ? Us[H + h] : 0.f;
  }
  float s[2] = {0.f, 0.f};                                             // sum dc g, sum dc c_prev
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) {
      const float tc = fast_tanh(cnv[p]);
      const float dh = dhv[p], o = ov[p], g = gv[p];
      const float dc = dcv[p] + dh * o * (1.0f - tc * tc);
      dcv[p] = dc;
      dzv[b * 2 * H + h] = dh * tc * o * (1.0f - o);
      dzv[b * 2 * H + H + h] = dc * i * (1.0f - g * g);
      dc_prev[b * H + h] = dc * f;
      s[0] += dc * g;
      s[1] += dc * cpv[p];
    }
  }
  block_sums_256<2>(s, red);
  const float dzi = s[0] * i * (1.0f - i), dzf = s[1] * f * (1.0f - f);
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) dh_prev[b * H + h] = dzi * ui[p] + dzf * uf[p];
  }
  if (tid == 0) { dzs[b * lds] = dzi; dzs[b * lds + 1] = dzf; }
}

}  // namespace

using namespace yt8m;

// what the two step kernels handle: whole 256-unit slices per thread slot, up to ROW_PT of them; one workgroup per row
extern "C" int yt8m_gate_lstm_supported(int64_t B, int64_t H) {
  return (B >= 1 && B < (1LL << 31) && H >= 256 && H % 256 == 0 && H <= 256 * ROW_PT) ? 1 : 0;
}

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
  auto kfn = YT8M_ROW_KERNEL(gate_lstm_fwd_kernel, H, 1);
  for (int64_t t = 0; t < F; ++t) {
    float* zvt = zv + t * B * 2 * H;
    int rc = rec.add_hW(hs + t * BH, zvt);                                                             // zv_t += h . [Uog|Uc]
    if (rc != YT8M_OK) return rc;
    ProfScope prof(F_LSTM, s);
    hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, zvt, zs + t * B * lds, lds, Us, cs + t * BH, hs + t * BH,
                       cs + (t + 1) * BH, hs + (t + 1) * BH, c_last, num_frames, (int)t, H);
  }
  return launch_status("gate_lstm_fwd_kernel");
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
  // workspace holds the packed weights; YT8M_GATE_LSTM_PACKED_BWD=0 (read at every call: an A/B switch for tools/ and tests) keeps
  // the grouped GEMM
  const char* sw = getenv("YT8M_GATE_LSTM_PACKED_BWD");
  const bool packed = !(sw && atoi(sw) == 0) && packed_fits(B, H, 2, gemm_workspace, gemm_workspace_bytes);
  float* Wq = packed ? static_cast<float*>(gemm_workspace) : nullptr;
  if (packed) {
    int rc = cell_pack_scoped(Uv, ldu, nullptr, Wq, H, 2, s);
    if (rc != YT8M_OK) return rc;
  }
  const StepProduct rec = {Uv, ldu, nullptr, Wq, 2, B, H, gemm_workspace, gemm_workspace_bytes, stream};
  auto kfn = YT8M_ROW_KERNEL(gate_lstm_bwd_kernel, H, 1);
  for (int64_t t = F - 1; t >= 0; --t, g.swap()) {
    float* dzvt = dzv + t * B * 2 * H;
    {
      ProfScope prof(F_LSTM, s);
      hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, zv + t * B * 2 * H, zs + t * B * lds, lds, Us, cs + t * BH,
                         cs + (t + 1) * BH, g.dh_cur, g.dc_cur, dout ? dout + t * BH : nullptr, dc_last, dzvt, dzs + t * B * lds,
                         g.dc_prev, g.dh_prev, num_frames, (int)t, H);
    }
    int rc = rec.add_dzWt(dzvt, g.dh_prev);                                                            // dh_prev += dzv_t . [Uog|Uc]^T
    if (rc != YT8M_OK) return rc;
  }
  return launch_status("gate_lstm_bwd_kernel");
}
