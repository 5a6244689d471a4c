// persist_plan.h -- every host-side decision of the persistent recurrences (lstm_persist.hip, gru_persist.inl) as plain C++17 with no
// HIP dependency: the workspace layout, the environment knobs, the geometry and, per direction, ONE plan of a launch.  The launch
// entry points dispatch on a plan's fields and the query entry points read the same plan, so a query cannot disagree with the launch
// it describes; tests/test_persist_plan_host.py states the plans at every edge as a literal table on a machine without a GPU.
//
// plan_fwd and plan_bwd are pure: no HIP call, no global, no getenv.  The device's CU count, the caps of yt8m_lstm_persist_set_cus and
// the calling thread's tape-prefetch mode come in as arguments.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include "../../include/yt8m_hip.h"

namespace yt8m_persist {

// ---- workspace layout (shared with the kernels) ----------------------------------------------------------------------------
constexpr int CTL_HDR = 32;                    // control block: [0] error word, counters from word 32
constexpr int CTL_STICKY = 32;                 // words between the sticky error word (workspace word 0) and ctl[0]
// Arrival counter shards per tile, one 128-byte line each (the single polling wave of a workgroup reads all of them with one
// load instruction).  Measured at B = 128, H = 1024: 8 and 16 shards run alike (10.6 us / step forward), 64 are slower (12.4:
// the poll costs more than the shorter add queues save).
constexpr int NSH = 8;
constexpr int MAX_LOCAL_TILES = 64;            // 16-row tiles one workgroup may own (the geometry refuses larger batches)
constexpr int64_t DBG_BYTES = 65536;           // tail of the workspace: s_memtime stamps of the timing variant

// workspace head: [sticky error line, 128 B, never zeroed by a launch][control block: zeroed before every launch], padded to 256 B
inline int64_t ctl_bytes(int NT16) { return (int64_t)(CTL_HDR + NT16 * NSH * 32) * 4; }
inline int64_t ctl_padded(int NT16) { return ((int64_t)CTL_STICKY * 4 + ctl_bytes(NT16) + 255) / 256 * 256; }
// exchange images (of `width` = H forward, 4H backward) that fit in a workspace
inline int images_in(int64_t workspace_bytes, int NT16, int64_t width) {
  const int64_t n = (workspace_bytes - ctl_padded(NT16) - DBG_BYTES) / ((int64_t)NT16 * 16 * width * 4);
  return (int)std::min<int64_t>(n, 1 << 20);
}
// bytes of the scale words an H2 backward launch of T steps publishes (one word per step, tile, producer workgroup and row quad), 256-aligned
inline int64_t h2_scale_bytes(int NT16, int64_t H, int64_t T) { return ((T * NT16 * (H / 16) * 16 + 255) / 256) * 256; }
// control block + two alternating exchange images sized for the BACKWARD pass (dz is 4H wide): [2][NT16][4H/16][256] floats
inline int64_t workspace_bytes(int NT16, int64_t H) { return ctl_padded(NT16) + (int64_t)2 * NT16 * 16 * 4 * H * 4 + DBG_BYTES; }
// One exchange image per step of a T-step launch, forward and backward (+ the scale words of the f16 form of the backward recurrence)
// ... + two parities x tiles x H / 16 workgroups x 2 KiB that no launch uses any more (the hand-off slots of a removed K-split
// form; kept so that the size and the layout of the workspace do not move)
inline int64_t workspace_bytes_steps(int NT16, int64_t H, int64_t T) {
  const int64_t n = std::max<int64_t>(T, 2);
  return ctl_padded(NT16) + n * NT16 * 16 * 4 * H * 4 + h2_scale_bytes(NT16, H, n) + (int64_t)2 * NT16 * (H / 16) * 2048 + DBG_BYTES;
}
// GRU forward: the control block and ONE exchange image per half-step, 2T + 1 images of [NT16 16, H].  (Its size, 3 max(T, 1) + 3
// such images, still covers the T blocks of [NT16 16, 3H] of a persistent backward that has since been removed; kept so that the
// layout of a caller's workspace does not move.)
inline int64_t gru_workspace_bytes(int NT16, int64_t H, int64_t T) {
  return ctl_padded(NT16) + (3 * std::max<int64_t>(T, 1) + 3) * NT16 * 16 * H * 4 + DBG_BYTES;
}

// ---- environment knobs -----------------------------------------------------------------------------------------------------
// The library fills ONE PersistKnobs per process, on the first use of any persistent entry point.  (Each knob used to be read on the
// first use of the function it sat in.  Nothing sets these variables inside a running process -- the tests and tools that vary them
// start child processes -- so the moment is not observable.)
struct PersistKnobs {
  bool no_persist = false;      // YT8M_NO_PERSIST set (any value): no shape is supported
  bool no_persist_bwd = false;  // YT8M_NO_PERSIST_BWD set: no backward shape is supported
  bool x3 = true;               // YT8M_PERSIST_X3=0: the forward never leaves the fp32 pipe
  bool fwd_h2 = true;           // YT8M_PERSIST_FWD_H2=0: a forward h2 request is a plain request
  bool bwd_h2 = true;           // YT8M_PERSIST_BWD_H2=0: a backward h2 request is a plain request
  bool bwd_rot = true;          // YT8M_BWD_ROT=0: no rotated backward epilogue
  bool tape_prefetch = true;    // YT8M_PERSIST_TAPE_PREFETCH=0: off for threads in mode 0
  int cus = 0;                  // YT8M_PERSIST_CUS: CUs a forward launch may occupy (0: the whole chip)
  int cus_bwd = 128;            // YT8M_PERSIST_CUS_BWD: ... a backward launch
  bool gru = true;              // YT8M_GRU_PERSIST=0: no GRU shape is supported
  bool chain = false;           // YT8M_PERSIST_CHAIN set: the gate chains every launch (A/B)
  int reserved_cus = 0;         // YT8M_PERSIST_RESERVED_CUS: initial value of yt8m_lstm_persist_reserve_cus
};
inline PersistKnobs persist_knobs_from_env() {
  auto set = [](const char* n) { return getenv(n) != nullptr; };
  auto on = [](const char* n) { const char* v = getenv(n); return !(v && atoi(v) == 0); };
  auto num = [](const char* n, int dflt) { const char* v = getenv(n); return v ? atoi(v) : dflt; };
  PersistKnobs k;
  k.no_persist = set("YT8M_NO_PERSIST");
  k.no_persist_bwd = set("YT8M_NO_PERSIST_BWD");
  k.x3 = on("YT8M_PERSIST_X3");
  k.fwd_h2 = on("YT8M_PERSIST_FWD_H2");
  k.bwd_h2 = on("YT8M_PERSIST_BWD_H2");
  k.bwd_rot = on("YT8M_BWD_ROT");
  k.tape_prefetch = on("YT8M_PERSIST_TAPE_PREFETCH");
  k.cus = num("YT8M_PERSIST_CUS", 0);
  k.cus_bwd = num("YT8M_PERSIST_CUS_BWD", 128);
  k.gru = on("YT8M_GRU_PERSIST");
  k.chain = set("YT8M_PERSIST_CHAIN");
  k.reserved_cus = num("YT8M_PERSIST_RESERVED_CUS", 0);
  return k;
}

// ---- geometry --------------------------------------------------------------------------------------------------------------
// NQ: k-groups per matrix wave (H / 128 forward, H / 32 backward).  NU: unit groups = workgroups per row group (H / 8 forward,
// H / 16 backward).  RB: row groups.  NT16: 16-row tiles.  per: unit groups of a row group per XCD set (0: no such map).
// pf: items requested ahead (forward 0 / 1 / 2, backward 0 / 1).
struct PersistGeometry { int NQ, NU, RB, NT16, per, pf; };

// CUs a persistent launch may occupy: the whole chip, or `cap` of them (yt8m_lstm_persist_set_cus, -1: the environment's `knob`)
inline int cu_budget(int cus, int cap, int knob) {
  const int c = cap >= 0 ? cap : knob;
  return (c > 0 && c < cus) ? c : cus;
}
inline int xcd_per(int RB, int NU) { return (RB <= 8 && (8 % RB) == 0 && (NU % (8 / RB)) == 0) ? 8 / RB : 0; }

inline bool fwd_geometry(int cus, int cap_fwd, const PersistKnobs& k, int64_t B, int64_t H, PersistGeometry* geo) {
  if (k.no_persist || B < 1 || H < 128 || (H % 128) != 0 || H > 1024) return false;
  const int NQ = (int)(H / 128);
  // (NQ odd > 1 would split the register / LDS halves unevenly: not instantiated.  NQ = 1 -- H = 128, the audio stack of the
  // parallel rgb / audio models, lstm_parallel_finaloutput_model.py:13-73 -- keeps its single q-group per wave in LDS.)
  if (!(NQ == 1 || NQ == 2 || NQ == 4 || NQ == 6 || NQ == 8)) return false;
  const int NU = (int)(H / 8);
  if (cus < NU) return false;
  const int NT16 = (int)((B + 15) / 16);
  int RB = cu_budget(cus, cap_fwd, k.cus) / NU;
  if (RB > NT16) RB = NT16;
  if (RB > NT16 / 4) RB = NT16 / 4;                      // >= 4 tiles per workgroup when the batch allows: four independent chains
  if (RB < 1) RB = 1;                                    // hide the exchange latency (publish -> visible -> fetched ~ 2 item times)
  if ((NT16 + RB - 1) / RB > MAX_LOCAL_TILES) return false;   // lds_seen: tiles one workgroup may own
  const int nit_min = NT16 / RB;                          // the last row group has floor(NT16 / RB) or one more
  // two items ahead only with >= 8 chains: with 4 the producer of item k + 2 has barely published when it is requested
  if (geo) *geo = {NQ, NU, RB, NT16, xcd_per(RB, NU), nit_min >= 8 ? 2 : (nit_min >= 2 ? 1 : 0)};
  return true;
}

inline bool bwd_geometry(int cus, int cap_bwd, const PersistKnobs& k, int64_t B, int64_t H, PersistGeometry* geo) {
  if (k.no_persist || k.no_persist_bwd || B < 1 || H > 1024 || !(H == 128 || (H >= 256 && (H % 256) == 0))) return false;
  const int NQ = (int)(H / 32);                          // 4, 8, 16, 24 or 32
  const int NU = (int)(H / 16);
  if (cus < NU) return false;
  const int NT16 = (int)((B + 15) / 16);
  // default: HALF the chip.  With 16 units per workgroup the whole chip leaves two 16-row tiles (= two independent chains) per
  // workgroup at B = 128 and the exchange latency is exposed on every item (42 us / step measured); on 128 CUs a workgroup
  // owns four tiles, runs 24 us / step -- the per-step kernels' speed on the whole chip -- and the other 128 CUs stay free for
  // the weight-gradient GEMMs of the layer pipeline.
  int RB = cu_budget(cus, cap_bwd, k.cus_bwd) / NU;
  if (RB > NT16 / 2) RB = NT16 / 2;                      // >= 2 tiles per workgroup when the batch allows: one chain's exchange
  if (RB < 1) RB = 1;                                    // latency hides behind the other chain's matrix work
  if ((NT16 + RB - 1) / RB > MAX_LOCAL_TILES) return false;
  if (geo) *geo = {NQ, NU, RB, NT16, xcd_per(RB, NU), NT16 / RB >= 2 ? 1 : 0};
  return true;
}

// ---- plans -----------------------------------------------------------------------------------------------------------------
// What an entry point asks for.  A bf16 or h2 product is a permission: where the plan cannot grant it, its form is fp32.
struct PersistRequest {
  enum Product { fp32, bf16, h2 } product = fp32;   // h2: an absmax word of W_h is present
  bool images = false;                              // backward: operand images wanted (a member of yt8m_persist_bwd_images is set)
  bool maxima = false;                              // backward: row or launch maxima of dz wanted
  bool gru = false;                                 // forward: the GRU recurrence (its own support rule, workspace and T limit)
};

enum class FwdForm { fp32, x3_six, bf16_one_plane, h2_two_plane };
enum class FwdPack { plain, x3_three, x3_one, x3_two_f16 };   // hx_pack_kernel, hx_pack_x3_kernel<3>, <1>, <2, true>
enum class BwdForm { fp32, images, bf16, h2 };

struct FwdPlan {
  int code = YT8M_OK;           // YT8M_OK, or the refusal with its message
  const char* why = "";
  bool shape_ok = false;        // (B, H) is supported on this device: geo and grid are valid, whatever the workspace
  PersistGeometry geo = {0, 0, 0, 0, 0, 0};
  unsigned grid = 0;            // workgroups = CUs the launch occupies
  int nimg = 0;                 // exchange images of the fp32 width in the workspace
  FwdForm form = FwdForm::fp32;
  FwdPack pack = FwdPack::plain;
  bool SH = false;              // fp32 form: one image per step, XCD-L2-shared fetch
  int PD = 0;                   // fp32 form and GRU: items requested ahead
  int NKB = 0;                  // the three bf16-pipe forms: K blocks template argument (H / 256)
};

struct BwdPlan {
  int code = YT8M_OK;
  const char* why = "";
  bool shape_ok = false;
  PersistGeometry geo = {0, 0, 0, 0, 0, 0};
  unsigned grid = 0;
  int nimg = 0;                 // exchange images of 4H width in the workspace
  int images_rows = 0;          // rows of the column-sum partials of an images launch (4 per row group); 0: the shape cannot take images
  BwdForm form = BwdForm::fp32;
  bool SH = false, PF = false, ROT = false;
  bool TPF = false;             // h2 form: with the tape prefetch
  int64_t sc_offset = 0;        // h2 form: where the scale words sit in the workspace (between the last image and the debug tail) ...
  int64_t sc_bytes = 0;         // ... and their size
};

template <typename Plan>
inline Plan refuse(Plan p, int code, const char* why) { p.code = code; p.why = why; return p; }

inline FwdPlan plan_fwd(int cus, int cap_fwd, const PersistKnobs& k, int64_t B, int64_t H, int64_t T, int64_t workspace_bytes_given,
                        PersistRequest rq) {
  FwdPlan p;
  p.shape_ok = fwd_geometry(cus, cap_fwd, k, B, H, &p.geo) && (!rq.gru || (k.gru && p.geo.NQ >= 2));
  if (!p.shape_ok)
    return refuse(FwdPlan(), YT8M_E_SHAPE, rq.gru ? "shape not supported by the persistent GRU recurrence (see yt8m_gru_persist_supported)"
                                          : "shape not supported by the persistent recurrence (see yt8m_lstm_persist_supported)");
  const int NT16 = p.geo.NT16;
  p.grid = (unsigned)(p.geo.NU * p.geo.RB);
  p.PD = p.geo.pf;
  if (workspace_bytes_given < (rq.gru ? gru_workspace_bytes(NT16, H, T) : workspace_bytes(NT16, H)))
    return refuse(p, YT8M_E_SHAPE, "workspace too small");
  if (T >= (rq.gru ? 1 << 19 : 1 << 20)) return refuse(p, YT8M_E_SHAPE, "T too large");
  if (rq.gru) return p;                                  // fp32 products, plain pack, one image per half-step
  p.nimg = images_in(workspace_bytes_given, NT16, H);
  p.SH = p.nimg >= T;
  // the recurrent product on the bf16 pipe (lstm_persist_fwd_x3_kernel) when its preconditions hold: an exchange image (1.5x the
  // fp32 one) per step, >= 2 tiles per workgroup, H in {512, 1024}
  if (!(k.x3 && (H == 512 || H == 1024) && p.geo.pf >= 1 && images_in(workspace_bytes_given, NT16, H + H / 2) >= T)) return p;
  p.NKB = (int)(H / 256);
  if (rq.product == PersistRequest::h2 && k.fwd_h2) { p.form = FwdForm::h2_two_plane; p.pack = FwdPack::x3_two_f16; }   // image per step of the fp32 image's size
  else if (rq.product == PersistRequest::bf16) { p.form = FwdForm::bf16_one_plane; p.pack = FwdPack::x3_one; }
  else { p.form = FwdForm::x3_six; p.pack = FwdPack::x3_three; }
  return p;
}

// (cap_fwd: a backward launch needs the shape supported forward too, and that depends on the forward cap through MAX_LOCAL_TILES)
inline BwdPlan plan_bwd(int cus, int cap_fwd, int cap_bwd, int tape_prefetch_mode, const PersistKnobs& k, int64_t B, int64_t H, int64_t T,
                        int64_t workspace_bytes_given, PersistRequest rq) {
  BwdPlan p;
  p.shape_ok = fwd_geometry(cus, cap_fwd, k, B, H, nullptr) && bwd_geometry(cus, cap_bwd, k, B, H, &p.geo);
  if (!p.shape_ok)
    return refuse(BwdPlan(), YT8M_E_SHAPE, "shape not supported by the persistent backward recurrence (see yt8m_lstm_persist_bwd_supported)");
  const int NT16 = p.geo.NT16, RB = p.geo.RB;
  p.grid = (unsigned)(p.geo.NU * RB);
  p.PF = p.geo.pf != 0;
  // rotation needs a multiple of four tiles in EVERY workgroup (row group g owns tiles g, g + RB, ...) and the prefetching form
  p.ROT = k.bwd_rot && p.PF && (NT16 % (4 * RB)) == 0;
  p.images_rows = ((B % 16) == 0 && p.ROT) ? 4 * RB : 0;   // the images are written by the rotated epilogue, whole tiles only
  if (workspace_bytes_given < workspace_bytes(NT16, H)) return refuse(p, YT8M_E_SHAPE, "workspace too small");
  if (T >= (1 << 20)) return refuse(p, YT8M_E_SHAPE, "T too large");
  p.nimg = images_in(workspace_bytes_given, NT16, 4 * H);
  p.SH = p.nimg >= T;
  if (rq.maxima && (rq.images || !p.SH || !p.ROT))
    return refuse(p, YT8M_E_SHAPE, "row / launch maxima need the rotated backward epilogue on a per-step workspace (yt8m_lstm_persist_bwd_images_rows)");
  if (rq.images) {                                       // images win over a bf16 / h2 request
    if (!p.SH) return refuse(p, YT8M_E_SHAPE, "operand images need one exchange image per step");
    if (!p.ROT) return refuse(p, YT8M_E_SHAPE, "operand images need the rotated backward epilogue");
    p.form = BwdForm::images;
    return p;
  }
  if (!((H == 512 || H == 1024) && p.SH && p.ROT)) return p;   // the bf16 and f16 forms: instantiated for NQ 16 and 32, rotated, image per step
  if (rq.product == PersistRequest::bf16) p.form = BwdForm::bf16;
  if (rq.product == PersistRequest::h2 && k.bwd_h2) {
    // the scale words sit between the last exchange image and the debug tail; taken only when T images still fit in front of them
    const int64_t scb = h2_scale_bytes(NT16, H, T);
    if (scb < (1LL << 31) && images_in(workspace_bytes_given - scb, NT16, 4 * H) >= T) {
      p.form = BwdForm::h2;
      p.sc_offset = workspace_bytes_given - DBG_BYTES - scb;
      p.sc_bytes = scb;
      p.TPF = tape_prefetch_mode == 1 || (tape_prefetch_mode == 0 && k.tape_prefetch);
    }
  }
  return p;
}

// ---- queries ---------------------------------------------------------------------------------------------------------------
// What the (B, H) query entry points answer: reads of the plans above, nothing restated.  Those about a product form describe "a
// T-step launch on a workspace of yt8m_lstm_persist_workspace_bytes_steps(B, H, T)"; a form depends on T only through "T images
// fit", which that workspace guarantees for its T, so the plan of a one-step launch answers for every T.
struct PersistQueries {
  int supported, bwd_supported, gru_supported;   // yt8m_lstm_persist_supported, _bwd_supported, yt8m_gru_persist_supported
  int fwd_on_bf16_pipe;                          // a plain forward launch runs the six-product form
  int bwd_on_f16_pipe;                           // an h2 backward launch runs the f16 form
  int bwd_images_rows;
  int NT16;                                      // of a supported shape, for the workspace sizes
};
inline PersistQueries persist_queries(int cus, int cap_fwd, int cap_bwd, const PersistKnobs& k, int64_t B, int64_t H) {
  PersistRequest plain, h2, gru;
  h2.product = PersistRequest::h2;
  gru.gru = true;
  PersistQueries q = {0, 0, 0, 0, 0, 0, 0};
  const FwdPlan f = plan_fwd(cus, cap_fwd, k, B, H, 1, 0, plain);
  if (!f.shape_ok) return q;
  const int64_t steps = workspace_bytes_steps(f.geo.NT16, H, 1);
  const BwdPlan b = plan_bwd(cus, cap_fwd, cap_bwd, 0, k, B, H, 1, steps, h2);
  q.supported = 1;
  q.NT16 = f.geo.NT16;
  q.gru_supported = plan_fwd(cus, cap_fwd, k, B, H, 1, 0, gru).shape_ok ? 1 : 0;
  q.fwd_on_bf16_pipe = plan_fwd(cus, cap_fwd, k, B, H, 1, steps, plain).form == FwdForm::x3_six ? 1 : 0;
  q.bwd_supported = b.shape_ok ? 1 : 0;
  q.bwd_on_f16_pipe = b.form == BwdForm::h2 ? 1 : 0;
  q.bwd_images_rows = b.images_rows;
  return q;
}

}  // namespace yt8m_persist
