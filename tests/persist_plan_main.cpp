// Prints the plans of youtube-8m_amd/csrc/persist_plan.h for the cases on standard input (tests/test_persist_plan_host.py).
// One case per line:  fwd|bwd cus cap_fwd cap_bwd tape_mode B H T workspace_bytes product images maxima gru [knob=value ...]
// `env` instead prints the knobs as the environment gives them.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "persist_plan.h"

using namespace yt8m_persist;

static bool set_knob(PersistKnobs& k, const std::string& name, int v) {
  if (name == "no_persist") k.no_persist = v;
  else if (name == "no_persist_bwd") k.no_persist_bwd = v;
  else if (name == "x3") k.x3 = v;
  else if (name == "fwd_h2") k.fwd_h2 = v;
  else if (name == "bwd_h2") k.bwd_h2 = v;
  else if (name == "bwd_rot") k.bwd_rot = v;
  else if (name == "tape_prefetch") k.tape_prefetch = v;
  else if (name == "cus") k.cus = v;
  else if (name == "cus_bwd") k.cus_bwd = v;
  else if (name == "gru") k.gru = v;
  else if (name == "chain") k.chain = v;
  else if (name == "reserved_cus") k.reserved_cus = v;
  else return false;
  return true;
}

static void print_knobs(const PersistKnobs& k) {
  printf("no_persist=%d no_persist_bwd=%d x3=%d fwd_h2=%d bwd_h2=%d bwd_rot=%d tape_prefetch=%d cus=%d cus_bwd=%d gru=%d chain=%d reserved_cus=%d\n",
         k.no_persist, k.no_persist_bwd, k.x3, k.fwd_h2, k.bwd_h2, k.bwd_rot, k.tape_prefetch, k.cus, k.cus_bwd, k.gru, k.chain, k.reserved_cus);
}

int main() {
  static const char* fwd_forms[] = {"fp32", "x3_six", "bf16_one_plane", "h2_two_plane"};
  static const char* packs[] = {"plain", "x3_three", "x3_one", "x3_two_f16"};
  static const char* bwd_forms[] = {"fp32", "images", "bf16", "h2"};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string dir;
    if (!(in >> dir)) continue;
    if (dir == "env") { print_knobs(persist_knobs_from_env()); continue; }
    int cus, cap_fwd, cap_bwd, mode, product, images, maxima, gru;
    long long B, H, T, ws;
    if (!(in >> cus >> cap_fwd >> cap_bwd >> mode >> B >> H >> T >> ws >> product >> images >> maxima >> gru)) return 2;
    PersistKnobs k;
    std::string kv;
    while (in >> kv) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos || !set_knob(k, kv.substr(0, eq), atoi(kv.c_str() + eq + 1))) return 3;
    }
    PersistRequest rq;
    rq.product = (PersistRequest::Product)product; rq.images = images; rq.maxima = maxima; rq.gru = gru;
    const PersistQueries q = persist_queries(cus, cap_fwd, cap_bwd, k, B, H);
    if (dir == "fwd") {
      const FwdPlan p = plan_fwd(cus, cap_fwd, k, B, H, T, ws, rq);
      printf("code=%d ok=%d geo=%d,%d,%d,%d,%d,%d grid=%u", p.code, p.shape_ok, p.geo.NQ, p.geo.NU, p.geo.RB, p.geo.NT16, p.geo.per, p.geo.pf, p.grid);
      if (p.code == YT8M_OK)                            // (a refused plan's launch fields mean nothing)
        printf(" nimg=%d form=%s pack=%s SH=%d PD=%d NKB=%d", p.nimg, fwd_forms[(int)p.form], packs[(int)p.pack], p.SH, p.PD, p.NKB);
      printf(" | q=%d,%d,%d sizes=%lld,%lld,%lld | %s\n", q.supported, q.gru_supported, q.fwd_on_bf16_pipe,
             q.supported ? (long long)workspace_bytes(q.NT16, H) : 0LL, q.supported ? (long long)workspace_bytes_steps(q.NT16, H, T) : 0LL,
             q.supported ? (long long)gru_workspace_bytes(q.NT16, H, T) : 0LL, p.why);
    } else {
      const BwdPlan p = plan_bwd(cus, cap_fwd, cap_bwd, mode, k, B, H, T, ws, rq);
      printf("code=%d ok=%d geo=%d,%d,%d,%d,%d,%d grid=%u", p.code, p.shape_ok, p.geo.NQ, p.geo.NU, p.geo.RB, p.geo.NT16, p.geo.per, p.geo.pf, p.grid);
      if (p.code == YT8M_OK)
        printf(" nimg=%d form=%s SH=%d PF=%d ROT=%d TPF=%d sc=%lld,%lld", p.nimg, bwd_forms[(int)p.form], p.SH, p.PF, p.ROT, p.TPF,
               (long long)p.sc_offset, (long long)p.sc_bytes);
      printf(" | q=%d,%d,%d steps=%lld | %s\n", q.bwd_supported, q.bwd_on_f16_pipe, q.bwd_images_rows,
             q.supported ? (long long)workspace_bytes_steps(q.NT16, H, T) : 0LL, p.why);
    }
  }
  return 0;
}
