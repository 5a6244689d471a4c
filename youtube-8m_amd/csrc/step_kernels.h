// step_kernels.h -- the per-step recurrence launchers of lstm_fused.hip, declared once for the drivers that sequence them
// (sequence.hip, cells.hip, lstm_bf16.hip), and the small host pieces every time loop shares.  No launcher opens a ProfScope.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <initializer_list>
#include "common.h"

namespace yt8m {

// ---- lstm_fused.hip: packed-weight step products, one launch per product with the epilogue fused --------------------------
// G gates of H units (LSTM 4, GRU gate block 2, GRU candidate 1); Wp / Wq hold H * G*H floats each.
bool lstm_fused_supported(int64_t B, int64_t H, int64_t workspace_bytes);   // BasicLSTM: H % 128 == 0
bool cell_packed_supported(int64_t B, int64_t H);                           // the other cells: H % 256 == 0
int cell_pack(const float* Wh, int64_t ldw, float* Wp, float* Wq, int64_t H, int G, hipStream_t s);
int lstm_step_fwd(float* z, const float* Wp, const float* c_prev, const float* h_prev, float* c_new, float* h_new, float* out,
                  const int32_t* nf, int t, int64_t B, int64_t H, float fb, hipStream_t s);
int lstm_step_bwd_fused(const float* dz_t, const float* Wq, const float* dh_prev, const float* gates1, const float* c_prev1,
                        const float* c_new1, const float* dc_in, const float* dout1, float* dz1, float* dc_out, float* dh_out,
                        const int32_t* nf, int t, int64_t B, int64_t H, hipStream_t s);
int cell_step_add4(float* z, const float* Wp, const float* h_prev, int64_t B, int64_t H, hipStream_t s);
int cell_step_bwd(const float* dz, const float* Wq, float* dh_prev, int64_t B, int64_t H, int G, hipStream_t s);
int gru_step_gates(float* zg, const float* Wp_g, const float* h_prev, float* rh, int64_t B, int64_t H, hipStream_t s);
int gru_step_cand(float* zc, const float* Wp_c, const float* rh, const float* zg, const float* h_prev, float* h_new, float* out,
                  const int32_t* nf, int t, int64_t B, int64_t H, hipStream_t s);
int gru_step_bwd_cand(const float* dzc, const float* Wq_c, float* dh_prev, const float* zg, const float* h_prev, float* dzg,
                      const int32_t* nf, int t, int64_t B, int64_t H, hipStream_t s);

// ---- the recurrent product of one step: the packed launcher when packed weights are present, else one grouped fp32 GEMM ----
// (the GEMM takes host-side split-K decisions and opens its own ProfScope; a packed launch is counted under F_LSTM)
// The packed launchers read and write contiguous rows: a caller whose z / dz rows have another stride gives ldz and either no packed
// weights or a contiguous copy of the rows.
struct StepProduct {
  const float* Wh;          // [H, G*H], leading dimension ld
  int64_t ld;
  const float* Wp;          // packed forward weights (G = 4 only: cell_step_add4) or null
  const float* Wq;          // packed backward weights or null
  int G;
  int64_t B, H;
  void* ws;                 // GEMM workspace
  int64_t ws_bytes;
  yt8m_stream_t stream;
  int64_t ldz = G * H;      // row stride of z / dz on the GEMM route

  // z[B, G*H] += h[B, H] . Wh
  int add_hW(const float* h, float* z) const {
    if (Wp) {
      ProfScope prof(F_LSTM, as_stream(stream));
      return cell_step_add4(z, Wp, h, B, H, as_stream(stream));
    }
    yt8m_gemm_problem pr = {B, G * H, H, h, H, Wh, ld, z, ldz, nullptr, 1.0f};
    return yt8m_gemm_f32_grouped(0, 0, 1, &pr, ws, ws_bytes, stream);
  }
  // dh_prev[B, H] += dz[B, G*H] . Wh^T   (Wh stored [H, G*H] => transB).  in_scope: the caller's F_LSTM scope covers a packed launch
  int add_dzWt(const float* dz, float* dh_prev, bool in_scope = false) const {
    if (Wq && in_scope) return cell_step_bwd(dz, Wq, dh_prev, B, H, G, as_stream(stream));
    if (Wq) {
      ProfScope prof(F_LSTM, as_stream(stream));
      return cell_step_bwd(dz, Wq, dh_prev, B, H, G, as_stream(stream));
    }
    yt8m_gemm_problem pr = {B, H, G * H, dz, ldz, Wh, ld, dh_prev, H, nullptr, 1.0f};
    return yt8m_gemm_f32_grouped(0, 1, 1, &pr, ws, ws_bytes, stream);
  }
};

// ---- what every row-per-workgroup cell driver repeats (cells.hip's LN-LSTM, gate_cell.hip, glu_lstm.hip) ------------------
// whether the packed weights of G gates fit the workspace and the packed launchers take the shape; the environment switches that
// keep the grouped GEMM stay with each caller (cells.hip reads its own once per process) or with packed_bwd_weights below
inline bool packed_fits(int64_t B, int64_t H, int G, const void* ws, int64_t ws_bytes) {
  return ws && cell_packed_supported(B, H) && ws_bytes >= (int64_t)sizeof(float) * H * G * H;
}
// cell_pack under an F_LSTM scope of its own
inline int cell_pack_scoped(const float* Wh, int64_t ldw, float* Wp, float* Wq, int64_t H, int G, hipStream_t s) {
  ProfScope prof(F_LSTM, s);
  return cell_pack(Wh, ldw, Wp, Wq, H, G, s);
}
// The weights of a backward recurrence's product dz . Wh^T (StepProduct::Wq): *Wq = the head of the workspace, filled by cell_pack
// under an F_LSTM scope of its own, where packed_fits; *Wq = null (the grouped GEMM) where not, or where the environment switch
// `sw_name` is set to 0.  The switch is read at every call: an A/B switch for tools/ and tests.
inline int packed_bwd_weights(const char* sw_name, const float* Wh, int64_t ldw, int64_t B, int64_t H, int G, void* ws,
                              int64_t ws_bytes, hipStream_t s, const float** Wq) {
  const char* sw = getenv(sw_name);
  *Wq = nullptr;
  if ((sw && atoi(sw) == 0) || !packed_fits(B, H, G, ws, ws_bytes)) return YT8M_OK;
  *Wq = static_cast<float*>(ws);
  return cell_pack_scoped(Wh, ldw, nullptr, static_cast<float*>(ws), H, G, s);
}
// K<PT, ...>, the step kernel template K at the fewest units per thread that cover H with 256 threads: PT = MIN_PT (1 or 2), 2, 4 or
// ROW_PT; further template arguments of K follow MIN_PT
constexpr int ROW_PT = 8;                      // H <= 256 * ROW_PT
#define YT8M_ROW_KERNEL(K, H, MIN_PT, ...)                                                                                \
  ((H) <= 256 * (MIN_PT) ? K<MIN_PT, ##__VA_ARGS__> : (H) <= 512 ? K<2, ##__VA_ARGS__> : (H) <= 1024 ? K<4, ##__VA_ARGS__> \
                                                                                                     : K<yt8m::ROW_PT, ##__VA_ARGS__>)

// dst[n] = src[n], or zeros when there is no src (the gradients of the final state)
inline hipError_t seed_state(float* dst, const float* src, int64_t n, hipStream_t s) {
  return src ? hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s) : hipMemsetAsync(dst, 0, n * sizeof(float), s);
}

// the running gradients of a backward recurrence in work [4, B, H]: (dh, dc) of the step being processed and of the one before
// it.  They live in work[0], work[1] / work[2], work[3] when `phase` is 0 and the other way round when it is 1; every step swaps.
struct StateGrads {
  float *dh_cur, *dc_cur, *dh_prev, *dc_prev;
  StateGrads(float* work, int phase, int64_t BH)
      : dh_cur(work + (phase ? 2 : 0) * BH), dc_cur(dh_cur + BH), dh_prev(work + (phase ? 0 : 2) * BH), dc_prev(dh_prev + BH) {}
  void swap() {
    std::swap(dh_cur, dh_prev);
    std::swap(dc_cur, dc_prev);
  }
};

// key of a captured step chain: every pointer and integer the chain depends on (+ the bits of the forward's forget bias)
inline GraphKey graph_key(int kind, std::initializer_list<const void*> p, std::initializer_list<int64_t> v, float forget_bias = 0.f) {
  GraphKey key;
  memset(&key, 0, sizeof(key));
  key.kind = kind;
  std::copy(p.begin(), p.end(), key.p);
  std::copy(v.begin(), v.end(), key.v);
  memcpy(&key.v[7], &forget_bias, sizeof(float));
  return key;
}

}  // namespace yt8m
