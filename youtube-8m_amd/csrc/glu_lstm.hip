// glu_lstm.hip -- the input-memory LSTM cell of Z/frame_level_models.py:695-792 (LstmGlu2Model.create_recurrent_unit; the same unit in
// LstmGlu2MultilayerModel, :848), in the generic per-step form of cells.hip (gfx950, wave64).  Beside h and c the cell carries a
// memory of the INPUT, xm (the reference's x_prev), and reads it l2-normalised, hx = xm * rsqrt(max(sum xm^2, 1e-12)):
//       s = sigmoid(x.Ws + hx.Vs + h.Us + bs)       [B,4] = i | f | ix | fx     (ONE scalar each per video)
//       o = sigmoid(x.Wog + hx.Vog + h.Uog + bog)   [B,H]        g = tanh(x.Wc + hx.Vc + h.Uc + bc)   [B,H]
//       c' = f c + i g        h' = o tanh(c')        xm' = fx xm + ix x
// The loop is a plain tf.while_loop over all max_frames steps (no copy-through, no masking); the head reads the memory c gathered at
// frame num_frames - 1.
// xm is a scalar-weighted running sum of the frames, so its projections are too: with pv_t = x_t.[Vog|Vc], ps_t = x_t.Vs (hoisted by the
// caller with the other input products), qv = xm.[Vog|Vc] and qs = xm.Vs obey
//       qv' = fx qv + ix pv_t        qs' = fx qs + ix ps_t        hx.V = r q,   r = rsqrt(max(n2, 1e-12)),   n2 = sum xm^2
// and are carried as states of their own: no product with K = D inside the time loop.  Per step there is one grouped-GEMM launch for
// h.[Uog|Uc] and one pointwise kernel, one workgroup per batch row: four (forward) or five (backward) block-wide row sums on one
// barrier pair, in the forward kernel a second pair for n2'.
// The kernels stay apart from the two-gate cell of gate_cell.hip: four scalar gates, the r q terms in every pre-activation, five sums
// on the barrier and the xm pass would each be a hook in a shared body, and the hooks would cost more than the lines they save.
#include "step_kernels.h"

namespace {

constexpr int GU_DMAX = 2048;                  // widest input
constexpr float GU_EPS = 1e-12f;               // tf.nn.l2_normalize's epsilon

// the frame of row b at step t, four values at d: float frames x [F,B,D], or the reader's bytes q [B,F,D] under the frame's scale
struct Frame {
  const float* xf;       // float frames: row t B + b (or null)
  const uint8_t* xq;     // bytes: row b F + t
  float rf;              // 1 / ||a0 q + c0|| of this frame, 0 on a padding frame
  __device__ __forceinline__ float4 at(int d) const {
    if (xf) return *reinterpret_cast<const float4*>(xf + d);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(xq + d);
    float4 v;
    v.x = rf * fmaf((float)(w & 255u), U8_A0, U8_C0);
    v.y = rf * fmaf((float)((w >> 8) & 255u), U8_A0, U8_C0);
    v.z = rf * fmaf((float)((w >> 16) & 255u), U8_A0, U8_C0);
    v.w = rf * fmaf((float)(w >> 24), U8_A0, U8_C0);
    return v;
  }
};

struct FwdArgs {
  float* zv;             // [B] rows of stride ldv: in x.[Wog|Wc] + [bog|bc] + h.[Uog|Uc], out o | g
  const float* pv;       // [B] rows of stride ldv: x.[Vog|Vc]
  int64_t ldv;
  float* zs;             // [B] rows of stride lds: columns 0..3 in x.Ws + bs, out i | f | ix | fx; columns 4..7 x.Vs (read only)
  int64_t lds;
  const float* Us;       // [4, H]
  const float *c_prev, *h_prev, *qv_prev, *qs_prev, *xm_prev, *n2_prev;
  float *c_new, *h_new, *qv_new, *qs_new, *xm_new, *n2_new;
  float* c_last;
  const int32_t* nf;
  const float* xf;       // float frames of this step [B, D], or null
  const uint8_t* xq;     // bytes [B, F, D] (whole tensor) with rframe [B] of this step
  const float* rframe;
  int64_t F, H, D;
  int t;
};

// One workgroup per batch row; PT = compile-time units per thread (H <= 256 PT, H % 256 == 0).
template <int PT>
__global__ __launch_bounds__(256) void glu_lstm_fwd_kernel(const FwdArgs a) {
  __shared__ float red[16];
  const int64_t b = blockIdx.x, H = a.H, D = a.D;
  const int tid = threadIdx.x;
  float* zr = a.zv + b * a.ldv;
  const float* pr = a.pv + b * a.ldv;
  float* sr = a.zs + b * a.lds;
  float zs[4], ps[4], qs[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { zs[k] = sr[k]; ps[k] = sr[4 + k]; qs[k] = a.qs_prev[b * 4 + k]; }
  const float r = rsqrtf(fmaxf(a.n2_prev[b], GU_EPS));
  const bool last = a.c_last && a.nf && (a.t + 1 == a.nf[b]);          // block-uniform
  float zo[PT], zg[PT], cp[PT], hp[PT], qo[PT], qg[PT], po[PT], pg[PT], u[4][PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    const bool in = h < H;
    zo[p] = in ? zr[h] : 0.f;
    zg[p] = in ? zr[H + h] : 0.f;
    po[p] = in ? pr[h] : 0.f;
    pg[p] = in ? pr[H + h] : 0.f;
    qo[p] = in ? a.qv_prev[b * 2 * H + h] : 0.f;
    qg[p] = in ? a.qv_prev[b * 2 * H + H + h] : 0.f;
    cp[p] = in ? a.c_prev[b * H + h] : 0.f;
    hp[p] = in ? a.h_prev[b * H + h] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k][p] = in ? a.Us[k * H + h] : 0.f;
  }
  float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p = 0; p < PT; ++p) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += hp[p] * u[k][p];
  }
  block_sums_256<4>(s, red);
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = fast_sigmoid(zs[k] + r * qs[k] + s[k]);
  const float gi = s[0], gf = s[1], ix = s[2], fx = s[3];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) {
      const float o = fast_sigmoid(zo[p] + r * qo[p]), g = fast_tanh(zg[p] + r * qg[p]);
      const float cn = gf * cp[p] + gi * g;
      zr[h] = o;
      zr[H + h] = g;
      a.c_new[b * H + h] = cn;
      a.h_new[b * H + h] = o * fast_tanh(cn);
      a.qv_new[b * 2 * H + h] = fx * qo[p] + ix * po[p];
      a.qv_new[b * 2 * H + H + h] = fx * qg[p] + ix * pg[p];
      if (last) a.c_last[b * H + h] = cn;
    }
  }
  if (tid < 4) {
    sr[tid] = s[tid];
    a.qs_new[b * 4 + tid] = fx * qs[tid] + ix * ps[tid];
  }
  // xm' = fx xm + ix x and its squared norm
  Frame fr;
  fr.xf = a.xf ? a.xf + b * D : nullptr;
  fr.xq = a.xq ? a.xq + (b * a.F + a.t) * D : nullptr;
  fr.rf = a.rframe ? a.rframe[b] : 0.f;
  float n2[1] = {0.f};
  for (int d = tid * 4; d < D; d += 1024) {
    const float4 x = fr.at(d);
    const float4 m = *reinterpret_cast<const float4*>(a.xm_prev + b * D + d);
    float4 y;
    y.x = fx * m.x + ix * x.x;
    y.y = fx * m.y + ix * x.y;
    y.z = fx * m.z + ix * x.z;
    y.w = fx * m.w + ix * x.w;
    *reinterpret_cast<float4*>(a.xm_new + b * D + d) = y;
    n2[0] += y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w;
  }
  block_sums_256<1>(n2, red);
  if (tid == 0) a.n2_new[b] = n2[0];
}

struct BwdArgs {
  const float* zv;       // o | g of this step, rows of stride ldv
  const float* pv;
  int64_t ldv;
  const float* zs;       // i | f | ix | fx | x.Vs, rows of stride lds
  int64_t lds;
  const float* Us;
  const float *c_prev, *c_new, *qv_prev, *qs_prev, *xm_prev, *xm_new, *n2_prev;   // the tape before / after this step
  const float *dh_cur, *dc_cur, *dout, *dc_last;
  float *dzv, *dpv;      // rows of stride lddv
  int64_t lddv;
  float* dzs;            // rows of stride lds: columns 0..3 dzs, 4..7 dps
  float* dav;            // [B, 2H] contiguous copy of dzv's rows for the packed product, or null
  float *dc_prev, *dh_prev;
  float *dqv, *dxm, *dsc;   // running gradients, updated in place: dqv [B,2H], dxm [B,D], dsc [B,8] = dqs[4] | dn2
  float* dxd;            // [B, D] of this step: ix dxm (float frames), or null
  const int32_t* nf;
  const float* xf;
  const uint8_t* xq;
  const float* rframe;
  int64_t F, H, D;
  int t;
};

// The gradients arriving at a row past its num_frames are all zero when nothing arrives through dout, and every product below is then
// exactly zero.
template <int PT>
__global__ __launch_bounds__(256) void glu_lstm_bwd_kernel(const BwdArgs a) {
  __shared__ float red[20];
  const int64_t b = blockIdx.x, H = a.H, D = a.D;
  const int tid = threadIdx.x;
  const float* zr = a.zv + b * a.ldv;
  const float* pr = a.pv + b * a.ldv;
  const float* sr = a.zs + b * a.lds;
  float s[4], ps[4], qs[4], dqs[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { s[k] = sr[k]; ps[k] = sr[4 + k]; qs[k] = a.qs_prev[b * 4 + k]; dqs[k] = a.dsc[b * 8 + k]; }
  const float dn2 = a.dsc[b * 8 + 4];
  const float n2p = a.n2_prev[b];
  const float r = rsqrtf(fmaxf(n2p, GU_EPS));
  const float gi = s[0], gf = s[1], ix = s[2], fx = s[3];
  const bool last = a.dc_last && a.nf && (a.t + 1 == a.nf[b]);         // block-uniform
  float ov[PT], gv[PT], cpv[PT], cnv[PT], dhv[PT], dcv[PT], qo[PT], qg[PT], po[PT], pg[PT], dqo[PT], dqg[PT], u[4][PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    const bool in = h < H;
    ov[p] = in ? zr[h] : 0.f;
    gv[p] = in ? zr[H + h] : 0.f;
    po[p] = in ? pr[h] : 0.f;
    pg[p] = in ? pr[H + h] : 0.f;
    qo[p] = in ? a.qv_prev[b * 2 * H + h] : 0.f;
    qg[p] = in ? a.qv_prev[b * 2 * H + H + h] : 0.f;
    dqo[p] = in ? a.dqv[b * 2 * H + h] : 0.f;
    dqg[p] = in ? a.dqv[b * 2 * H + H + h] : 0.f;
    cpv[p] = in ? a.c_prev[b * H + h] : 0.f;
    cnv[p] = in ? a.c_new[b * H + h] : 0.f;
    dhv[p] = in ? a.dh_cur[b * H + h] : 0.f;
    dcv[p] = in ? a.dc_cur[b * H + h] : 0.f;
    if (a.dout && in) dhv[p] += a.dout[b * H + h];
    if (last && in) dcv[p] += a.dc_last[b * H + h];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k][p] = in ? a.Us[k * H + h] : 0.f;
  }
  Frame fr;
  fr.xf = a.xf ? a.xf + b * D : nullptr;
  fr.xq = a.xq ? a.xq + (b * a.F + a.t) * D : nullptr;
  fr.rf = a.rframe ? a.rframe[b] : 0.f;
  // A padding frame of the byte path is a zero row of x, and everything that reads dpv_t / dps_t multiplies them by x_t: they are
  // written as zeros.  Their true values grow like r, up to 1e6 once xm has decayed below the l2-normalisation's epsilon, and would
  // set the one scale per matrix under which the byte path's weight-gradient product splits dzv | dpv.
  const float ixe = (a.xq && fr.rf == 0.f) ? 0.f : ix;
  // sums: 0 di = sum dct g, 1 df = sum dct c, 2 dix, 3 dfx, 4 <dav, qv>
  float sum[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) {
      const float tc = fast_tanh(cnv[p]);
      const float dh = dhv[p], o = ov[p], g = gv[p];
      const float dc = dcv[p] + dh * o * (1.0f - tc * tc);
      const float dao = dh * tc * o * (1.0f - o), dag = dc * gi * (1.0f - g * g);
      a.dzv[b * a.lddv + h] = dao;
      a.dzv[b * a.lddv + H + h] = dag;
      if (a.dav) {
        a.dav[b * 2 * H + h] = dao;
        a.dav[b * 2 * H + H + h] = dag;
      }
      a.dpv[b * a.lddv + h] = ixe * dqo[p];
      a.dpv[b * a.lddv + H + h] = ixe * dqg[p];
      a.dqv[b * 2 * H + h] = fx * dqo[p] + r * dao;
      a.dqv[b * 2 * H + H + h] = fx * dqg[p] + r * dag;
      a.dc_prev[b * H + h] = dc * gf;
      sum[0] += dc * g;
      sum[1] += dc * cpv[p];
      sum[2] += dqo[p] * po[p] + dqg[p] * pg[p];
      sum[3] += dqo[p] * qo[p] + dqg[p] * qg[p];
      sum[4] += dao * qo[p] + dag * qg[p];
    }
  }
  // the input memory: dxm += 2 dn2 xm'; its part of dix, dfx; what it hands to the frame and to the step before
  const float dn2x2 = 2.0f * dn2;
  for (int d = tid * 4; d < D; d += 1024) {
    const float4 x = fr.at(d);
    const float4 m0 = *reinterpret_cast<const float4*>(a.xm_prev + b * D + d);
    const float4 m1 = *reinterpret_cast<const float4*>(a.xm_new + b * D + d);
    float4 g = *reinterpret_cast<const float4*>(a.dxm + b * D + d);
    g.x += dn2x2 * m1.x;
    g.y += dn2x2 * m1.y;
    g.z += dn2x2 * m1.z;
    g.w += dn2x2 * m1.w;
    sum[2] += g.x * x.x + g.y * x.y + g.z * x.z + g.w * x.w;
    sum[3] += g.x * m0.x + g.y * m0.y + g.z * m0.z + g.w * m0.w;
    if (a.dxd) {
      float4 e;
      e.x = ix * g.x; e.y = ix * g.y; e.z = ix * g.z; e.w = ix * g.w;
      *reinterpret_cast<float4*>(a.dxd + b * D + d) = e;
    }
    g.x *= fx; g.y *= fx; g.z *= fx; g.w *= fx;
    *reinterpret_cast<float4*>(a.dxm + b * D + d) = g;
  }
  block_sums_256<5>(sum, red);
  float dix = sum[2], dfx = sum[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) { dix += dqs[k] * ps[k]; dfx += dqs[k] * qs[k]; }
  float das[4];
  das[0] = sum[0] * gi * (1.0f - gi);
  das[1] = sum[1] * gf * (1.0f - gf);
  das[2] = dix * ix * (1.0f - ix);
  das[3] = dfx * fx * (1.0f - fx);
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int64_t h = tid + p * 256;
    if (h < H) a.dh_prev[b * H + h] = das[0] * u[0][p] + das[1] * u[1][p] + das[2] * u[2][p] + das[3] * u[3][p];
  }
  if (tid < 4) {
    a.dzs[b * a.lds + tid] = das[tid];
    a.dzs[b * a.lds + 4 + tid] = ixe * dqs[tid];
    a.dsc[b * 8 + tid] = fx * dqs[tid] + r * das[tid];
  }
  if (tid == 0) {
    const float dr = sum[4] + das[0] * qs[0] + das[1] * qs[1] + das[2] * qs[2] + das[3] * qs[3];
    a.dsc[b * 8 + 4] = n2p > GU_EPS ? -0.5f * r * r * r * dr : 0.f;
  }
}

}  // namespace

using namespace yt8m;

// what the two step kernels handle: whole 256-unit slices per thread slot, up to ROW_PT of them; float4 / 4-byte reads of the frames
extern "C" int yt8m_glu_lstm_supported(int64_t B, int64_t H, int64_t D) {
  return (B >= 1 && B < (1LL << 31) && H >= 256 && H % 256 == 0 && H <= 256 * ROW_PT && D >= 4 && D % 4 == 0 && D <= GU_DMAX) ? 1 : 0;
}

extern "C" int yt8m_glu_lstm_layer_fwd(float* zv, float* pv, int64_t ldv, float* zs, int64_t lds, const float* Uv, int64_t ldu,
                                       const float* Us, const float* x, const uint8_t* xq, const float* xr, float* hs, float* cs,
                                       float* qv, float* qs, float* xm, float* n2, float* c_last, const int32_t* num_frames, int64_t F,
                                       int64_t B, int64_t H, int64_t D, void* gemm_workspace, int64_t gemm_workspace_bytes,
                                       yt8m_stream_t stream) {
  YT8M_REQUIRE(F >= 0 && B >= 0 && H >= 0 && D >= 0, YT8M_E_SHAPE, "negative dimension");
  if (F * B * H == 0) return YT8M_OK;
  YT8M_REQUIRE(zv && pv && zs && Uv && Us && hs && cs && qv && qs && xm && n2, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE((x != nullptr) != (xq != nullptr), YT8M_E_BADARG, "exactly one of the float frames and the byte frames");
  YT8M_REQUIRE(!xq || xr, YT8M_E_BADARG, "byte frames need their row scales");
  YT8M_REQUIRE(num_frames || !c_last, YT8M_E_BADARG, "c_last needs num_frames");
  YT8M_REQUIRE(ldu >= 2 * H && ldv >= 2 * H && lds >= 8, YT8M_E_SHAPE, "leading dimension too small");
  YT8M_REQUIRE(yt8m_glu_lstm_supported(B, H, D), YT8M_E_SHAPE, "glu_lstm supports H % 256 == 0, H <= 2048, D % 4 == 0, D <= 2048");
  YT8M_REQUIRE(aligned16(x) && aligned16(xm) && ((uintptr_t)xq & 3) == 0, YT8M_E_BADARG, "frames and xm must be 16-byte aligned (bytes: 4)");
  hipStream_t s = as_stream(stream);
  const int64_t BH = B * H, BD = B * D;
  if (c_last) YT8M_HIP_CHECK(hipMemsetAsync(c_last, 0, BH * sizeof(float), s));       // rows with num_frames < 1 (or > F) keep zeros
  auto kfn = YT8M_ROW_KERNEL(glu_lstm_fwd_kernel, H, 1);
  const StepProduct rec = {Uv, ldu, nullptr, nullptr, 2, B, H, gemm_workspace, gemm_workspace_bytes, stream, ldv};
  FwdArgs a;
  a.ldv = ldv; a.lds = lds; a.Us = Us; a.c_last = c_last; a.nf = num_frames; a.xq = xq; a.F = F; a.H = H; a.D = D;
  for (int64_t t = 0; t < F; ++t) {
    a.zv = zv + t * B * ldv;
    a.pv = pv + t * B * ldv;
    a.zs = zs + t * B * lds;
    int rc = rec.add_hW(hs + t * BH, a.zv);                                                            // zv_t += h . [Uog|Uc]
    if (rc != YT8M_OK) return rc;
    a.c_prev = cs + t * BH; a.h_prev = hs + t * BH; a.qv_prev = qv + t * 2 * BH; a.qs_prev = qs + t * B * 4; a.xm_prev = xm + t * BD;
    a.n2_prev = n2 + t * B;
    a.c_new = cs + (t + 1) * BH; a.h_new = hs + (t + 1) * BH; a.qv_new = qv + (t + 1) * 2 * BH; a.qs_new = qs + (t + 1) * B * 4;
    a.xm_new = xm + (t + 1) * BD; a.n2_new = n2 + (t + 1) * B;
    a.xf = x ? x + t * BD : nullptr;
    a.rframe = xr ? xr + t * B : nullptr;
    a.t = (int)t;
    ProfScope prof(F_LSTM, s);
    hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, a);
  }
  return launch_status("glu_lstm_fwd_kernel");
}

extern "C" int yt8m_glu_lstm_layer_bwd(const float* zv, const float* pv, int64_t ldv, const float* zs, int64_t lds, const float* Uv,
                                       int64_t ldu, const float* Us, const float* x, const uint8_t* xq, const float* xr,
                                       const float* hs, const float* cs, const float* qv, const float* qs, const float* xm,
                                       const float* n2, const float* dout, const float* dc_last, float* dzv, float* dpv, int64_t lddv,
                                       float* dzs, float* dx_direct, float* work, const int32_t* num_frames, int64_t F, int64_t B,
                                       int64_t H, int64_t D, void* gemm_workspace, int64_t gemm_workspace_bytes, yt8m_stream_t stream) {
  YT8M_REQUIRE(F >= 0 && B >= 0 && H >= 0 && D >= 0, YT8M_E_SHAPE, "negative dimension");
  if (F * B * H == 0) return YT8M_OK;
  YT8M_REQUIRE(zv && pv && zs && Uv && Us && hs && cs && qv && qs && xm && n2 && dzv && dpv && dzs && work, YT8M_E_BADARG, "null operand");
  YT8M_REQUIRE((x != nullptr) != (xq != nullptr), YT8M_E_BADARG, "exactly one of the float frames and the byte frames");
  YT8M_REQUIRE(!xq || xr, YT8M_E_BADARG, "byte frames need their row scales");
  YT8M_REQUIRE(num_frames || !dc_last, YT8M_E_BADARG, "dc_last needs num_frames");
  YT8M_REQUIRE(ldu >= 2 * H && ldv >= 2 * H && lddv >= 2 * H && lds >= 8, YT8M_E_SHAPE, "leading dimension too small");
  YT8M_REQUIRE(yt8m_glu_lstm_supported(B, H, D), YT8M_E_SHAPE, "glu_lstm supports H % 256 == 0, H <= 2048, D % 4 == 0, D <= 2048");
  YT8M_REQUIRE(aligned16(x) && aligned16(xm) && aligned16(dx_direct) && aligned16(work) && ((uintptr_t)xq & 3) == 0, YT8M_E_BADARG,
               "frames, xm, dx_direct and work must be 16-byte aligned (bytes: 4)");
  (void)hs;                                            // part of the layer's tape; the weight gradients over it are the caller's
  hipStream_t s = as_stream(stream);
  const int64_t BH = B * H, BD = B * D;
  // work: [4, B, H] running dh, dc (StateGrads) | dqv [B, 2H] | dav [B, 2H] | dxm [B, D] | dsc [B, 8]
  StateGrads g(work, 0, BH);
  float* dqv = work + 4 * BH;
  float* dav = dqv + 2 * BH;
  float* dxm = dav + 2 * BH;
  float* dsc = dxm + BD;
  YT8M_HIP_CHECK(seed_state(g.dh_cur, nullptr, BH, s));
  YT8M_HIP_CHECK(seed_state(g.dc_cur, nullptr, BH, s));
  YT8M_HIP_CHECK(seed_state(dqv, nullptr, 2 * BH, s));
  YT8M_HIP_CHECK(seed_state(dxm, nullptr, BD + 8 * B, s));
  // dzv . [Uog|Uc]^T on the packed step launcher of lstm_fused.hip (cell_step_bwd, G = 2) where the workspace holds the packed
  // weights, as in gate_cell.hip; the launcher reads contiguous rows, so the kernel leaves it a copy of dzv_t in work
  const float* Wq;
  int rc = packed_bwd_weights("YT8M_GLU_LSTM_PACKED_BWD", Uv, ldu, B, H, 2, gemm_workspace, gemm_workspace_bytes, s, &Wq);
  if (rc != YT8M_OK) return rc;
  const StepProduct rec = {Uv, ldu, nullptr, Wq, 2, B, H, gemm_workspace, gemm_workspace_bytes, stream, lddv};
  auto kfn = YT8M_ROW_KERNEL(glu_lstm_bwd_kernel, H, 1);
  BwdArgs a;
  a.ldv = ldv; a.lds = lds; a.Us = Us; a.dc_last = dc_last; a.lddv = lddv; a.dav = Wq ? dav : nullptr; a.dqv = dqv; a.dxm = dxm;
  a.dsc = dsc; a.nf = num_frames; a.xq = xq; a.F = F; a.H = H; a.D = D;
  for (int64_t t = F - 1; t >= 0; --t, g.swap()) {
    a.zv = zv + t * B * ldv;
    a.pv = pv + t * B * ldv;
    a.zs = zs + t * B * lds;
    a.c_prev = cs + t * BH; a.c_new = cs + (t + 1) * BH; a.qv_prev = qv + t * 2 * BH; a.qs_prev = qs + t * B * 4;
    a.xm_prev = xm + t * BD; a.xm_new = xm + (t + 1) * BD; a.n2_prev = n2 + t * B;
    a.dh_cur = g.dh_cur; a.dc_cur = g.dc_cur; a.dout = dout ? dout + t * BH : nullptr;
    a.dzv = dzv + t * B * lddv; a.dpv = dpv + t * B * lddv; a.dzs = dzs + t * B * lds;
    a.dc_prev = g.dc_prev; a.dh_prev = g.dh_prev;
    a.dxd = dx_direct ? dx_direct + t * BD : nullptr;
    a.xf = x ? x + t * BD : nullptr;
    a.rframe = xr ? xr + t * B : nullptr;
    a.t = (int)t;
    {
      ProfScope prof(F_LSTM, s);
      hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(256), 0, s, a);
    }
    rc = rec.add_dzWt(Wq ? dav : a.dzv, g.dh_prev);                                                // dh_prev += dzv_t . [Uog|Uc]^T
    if (rc != YT8M_OK) return rc;
  }
  return launch_status("glu_lstm_bwd_kernel");
}
