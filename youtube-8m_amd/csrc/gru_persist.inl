// gru_persist.inl -- the forward of tf.contrib.rnn.GRUCell under tf.nn.dynamic_rnn as ONE launch per (layer, time range), on the
// exchange protocol of the persistent LSTM recurrences (W/all_frame_models/gru_pooling_model.py:34-47, gru_with_pooling_model.py:34-38;
// VERDICT r5 #3).  Included by lstm_persist.hip inside its anonymous namespace: the control block, the sharded arrival counters,
// wait_tile / lds_wait_ge, the residency gate and the block -> (unit group, row group) map are the LSTM kernels' own.
//
// A GRU step is TWO dependent products -- [r|u] = sigmoid(zg + h . Wg_h), then c = tanh(zc + (r*h) . Wc_h) -- so a time step is two
// HALF-STEPS of the LSTM kernel's machine: half-step m reads exchange image m and its epilogue publishes image m + 1,
//   forward   m = 2 s     : A = h_{t-1}  (K = H), columns r|u of the workgroup's 8 units -> publishes r*h_{t-1}
//             m = 2 s + 1 : A = r*h      (K = H), columns c                             -> publishes h_t
// one exchange image per half-step (an address is written once and read after its tile's count is complete: plain L2-shared loads,
// see lstm_persist_fwd_kernel).  The products run on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 out: bit-compatible in kind with the
// per-step kernels of cells.hip / lstm_fused.hip; only the K summation order and the v_exp / v_rcp gate functions differ).
// Workgroup = 8 matrix waves (K split 8 ways, weights resident: half registers, half LDS) + 4 epilogue waves, as the LSTM kernel.
// The backward runs on the per-step kernels (yt8m_gru_layer_bwd): a persistent form of it needs two exchange rounds per step and
// ran at 29.0 us/step against their 20.3 (profiles/r6_gru_persist.txt); it was removed.

struct GruFwdArgs {
  float* zg;            // [F,B,2H] hoisted x . Wg_x + bg on entry; r | u activations on exit
  float* zc;            // [F,B,H]  hoisted x . Wc_x + bc on entry; c = tanh(..) on exit
  const float* Wg;      // [H, ldg]  recurrent rows of gates/weights (columns r: 0 .. H-1, u: H .. 2H-1)
  const float* Wc;      // [H, ldc]  recurrent rows of candidate/weights
  long long ldg, ldc;
  float* hs;            // [F+1,B,H] hs[t] = state before step t
  float* rh;            // [F,B,H]   r * h_{t-1} (operand of the candidate's weight gradient)
  float* out;           // [F,B,H] or null
  const int32_t* nf;    // [B] or null
  float* hx;            // exchange images [2T+1][NT16][H/16][256]
  unsigned* ctl;
  unsigned* stats;
  int t0, T, B, H;
  int NU, RB, NT16, per, pf;
};

template <int NQ, int PD>
__global__ __launch_bounds__(768) void gru_persist_fwd_kernel(GruFwdArgs a) {
  constexpr int HQ = NQ / 2;
  constexpr int NL = NQ - HQ;
  constexpr int HQA = HQ > 0 ? HQ : 1;
  __shared__ __attribute__((aligned(16))) float red[NSLOT][8][4][64];      // [slot][wave][acc reg][lane]: 32 KB
  __shared__ __attribute__((aligned(16))) float4 Wl[8][NL][2][64];         // LDS half of the slice: [tile 0 = r|u, tile 1 = c]
  __shared__ unsigned lds_cnt[NSLOT], lds_free[NSLOT];
  __shared__ unsigned lds_seen[MAX_LOCAL_TILES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int ug, g;
  {
    const int b = blockIdx.x;
    if (a.per > 0 && (a.NU % (4 * a.per)) == 0) {
      const int x = b & 7, sl = b >> 3;
      g = x / a.per;
      ug = ((sl >> 2) * a.per + (x % a.per)) * 4 + (sl & 3);
    } else if (a.per > 0) { const int x = b & 7; g = x / a.per; ug = (b >> 3) * a.per + (x % a.per); }
    else { g = b / a.NU; ug = b % a.NU; }
  }
  const int H = a.H, B = a.B, NT16 = a.NT16, RB = a.RB;
  const int n_it = (NT16 - g + RB - 1) / RB;
  const int HT = 2 * a.T;                                 // half-steps of this launch
  const int total = n_it * HT;
  const unsigned img_bytes = (unsigned)NT16 * (unsigned)H * 16u * 4u;
  const long long img_f = (long long)NT16 * H * 16;
  auto image = [&](int m) -> __amdgpu_buffer_rsrc_t { return make_rsrc(a.hx + m * img_f, img_bytes); };
  const int QH = H >> 4;
  const unsigned arrivals = (unsigned)a.NU;
  // B fragment of v_mfma_f32_16x16x4_f32: lane (n = lane & 15, kq = lane >> 4) supplies B[k = 16 q + 4 kq + e][n], e = 0..3 as a float4.
  // tile 0: column n <-> (unit n / 2, gate n % 2: r, u) -- the two gates of a unit are neighbouring result lanes;
  // tile 1: column n < 8 <-> candidate of unit n, columns 8-15 are zero.
  auto w_frag = [&](int qg, int ct) -> float4 {
    const int i16 = lane & 15, kq = lane >> 4;
    const long long k = (long long)(w * NQ + qg) * 16 + kq * 4;
    if (ct == 0) {
      const float* p = a.Wg + k * a.ldg + (long long)(i16 & 1) * H + ug * 8 + (i16 >> 1);
      return make_float4(p[0], p[a.ldg], p[2 * a.ldg], p[3 * a.ldg]);
    }
    if (i16 >= 8) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float* p = a.Wc + k * a.ldc + ug * 8 + i16;
    return make_float4(p[0], p[a.ldc], p[2 * a.ldc], p[3 * a.ldc]);
  };
  note_placement(a.ctl);
  if (tid < NSLOT) { lds_cnt[tid] = 0; lds_free[tid] = 0; }
  for (int i = tid; i < MAX_LOCAL_TILES; i += 768) lds_seen[i] = 0;
  if (w < 8) {
#pragma unroll
    for (int qq = 0; qq < NL; ++qq) {
      Wl[w][qq][0][lane] = w_frag(HQ + qq, 0);
      Wl[w][qq][1][lane] = w_frag(HQ + qq, 1);
    }
  }
  __syncthreads();

  if (w < 8) {
    // =============================== matrix waves ===============================
    const int i16 = lane & 15, kq = lane >> 4;
    float4 Wr[HQA][2];
#pragma unroll
    for (int qg = 0; qg < HQ; ++qg) { Wr[qg][0] = w_frag(qg, 0); Wr[qg][1] = w_frag(qg, 1); }
    const unsigned lane_off = (unsigned)(i16 * 16 + kq * 4) * 4u + (unsigned)(w * NQ) * 1024u;
    auto load_item = [&](float4 (&A)[NQ], int m, int T) {
      const __amdgpu_buffer_rsrc_t hxr = image(m);
      const unsigned base = (unsigned)(T * QH) * 1024u + lane_off;
#pragma unroll
      for (int qg = 0; qg < NQ; ++qg) A[qg] = as_f4(__builtin_amdgcn_raw_buffer_load_b128(hxr, (int)(base + (unsigned)qg * 1024u), 0, 0));
    };
    float4 A0[NQ], A1[NQ], A2[NQ];
    if (PD >= 1) load_item(A0, 0, g);
    if (PD >= 2 && total > 1) load_item(A1, n_it > 1 ? 0 : 1, n_it > 1 ? g + RB : g);   // (n_it >= 8 whenever PD == 2)
    int m_cur = 0, it_cur = 0;                             // item k = (half-step m_cur, local tile it_cur)
    auto item = [&](float4 (&A)[NQ], float4 (&Areq)[NQ], int k) {
      const int m = m_cur, T = g + it_cur * RB;
      const bool cand = (m & 1) != 0;
      int mr = m, Tr = T, itr = it_cur;
      unsigned pv = 0;
      if (PD >= 1) {
        itr = it_cur + PD;
        while (itr >= n_it) { itr -= n_it; ++mr; }
        const bool have = k + PD < total;
        Tr = have ? g + itr * RB : T;
        itr = have ? itr : it_cur;
        mr = have ? mr : m;
        if (w == 0 && lane < NSH)
          pv = __hip_atomic_load(a.ctl + CTL_HDR + (Tr * NSH + lane) * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        if (w == 0) {
          wait_tile(a.ctl, T, (unsigned)m * arrivals, lane);
          if (lane == 0) __hip_atomic_store(&lds_seen[it_cur], (unsigned)m * arrivals, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          lds_wait_ge(&lds_seen[it_cur], (unsigned)m * arrivals, a.ctl);
        }
        load_item(A, m, T);
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int qg = 0; qg < NQ; ++qg) {
        if (PD >= 1 && qg == NQ / 2) {                     // request point: the image of item k + PD must be complete now
          if (w == 0) {
            const unsigned tot = shard_sum(pv);
            if (tot < (unsigned)mr * arrivals) wait_tile(a.ctl, Tr, (unsigned)mr * arrivals, lane);
            if (lane == 0) __hip_atomic_store(&lds_seen[itr], (unsigned)mr * arrivals, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          } else {
            lds_wait_ge(&lds_seen[itr], (unsigned)mr * arrivals, a.ctl);
          }
          load_item(Areq, mr, Tr);
        }
        const float4 av = A[qg];
        float4 bv;
        if (qg < HQ) {
          const float4 b0 = Wr[qg < HQ ? qg : 0][0], b1 = Wr[qg < HQ ? qg : 0][1];
          bv = make_float4(cand ? b1.x : b0.x, cand ? b1.y : b0.y, cand ? b1.z : b0.z, cand ? b1.w : b0.w);
        } else {
          bv = Wl[w][qg - HQ][cand ? 1 : 0][lane];
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
      }
      const int slot = k & (NSLOT - 1);
      if (k >= NSLOT) lds_wait_ge(&lds_free[slot], (unsigned)(k / NSLOT), a.ctl);
      float* rw = &red[slot][w][0][lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) rw[r * 64] = acc[r];
      if (lane == 0) __hip_atomic_fetch_add(&lds_cnt[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (++it_cur == n_it) { it_cur = 0; ++m_cur; }
    };
    if (PD == 2) {
      for (int k = 0; k < total; k += 3) {
        item(A0, A2, k);
        if (k + 1 < total) item(A1, A0, k + 1);
        if (k + 2 < total) item(A2, A1, k + 2);
      }
    } else {
      for (int k = 0; k < total; k += 2) {
        item(A0, A1, k);
        if (k + 1 < total) item(A1, A0, k + 1);
      }
    }
    return;
  }

  // =============================== epilogue waves ===============================
  // wave ew owns the local tiles ew, ew + 4, .. for ALL half-steps: what it reloads (u, h_{t-1}) are its own earlier stores.
  const int ew = w - 8;
  const int eunit = lane & 7;
  __builtin_amdgcn_s_setprio(EPI_PRIO);
  for (int m = 0; m < HT; ++m) {
    const int s = m >> 1;
    const bool cand = (m & 1) != 0;
    const int t = a.t0 + s;
    for (int it = ew; it < n_it; it += NEPI) {
      const int k = m * n_it + it;
      const int T = g + it * RB;
      float z0[2], z1[2], hp[2];
      bool live[2], evalid[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int brow = T * 16 + 8 * j + (lane >> 3);
        evalid[j] = brow < B;
        const int br = evalid[j] ? brow : B - 1;
        const long long idx = ((long long)t * B + br) * H + ug * 8 + eunit;
        const float* zr = a.zg + ((long long)t * B + br) * 2 * H + ug * 8 + eunit;
        hp[j] = a.hs[idx];
        z1[j] = zr[H];                                     // gate half-step: u pre-activation; candidate half-step: u itself
        z0[j] = cand ? a.zc[idx] : zr[0];
        live[j] = a.nf ? (t < a.nf[br]) : true;
      }
      const int slot = k & (NSLOT - 1);
      lds_wait_ge(&lds_cnt[slot], 8u * (unsigned)(k / NSLOT + 1), a.ctl);
      // C layout of the 16x16 tile: column = lane & 15, row = 4 (lane >> 4) + reg.
      float s0[2], s1[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int erow = 8 * j + (lane >> 3);
        const int r = erow & 3, lb = (erow >> 2) * 16;
        s0[j] = 0.f; s1[j] = 0.f;
        if (!cand) {
#pragma unroll
          for (int wv = 0; wv < 8; ++wv) {
            const float2 p = *reinterpret_cast<const float2*>(&red[slot][wv][r][lb + 2 * eunit]);
            s0[j] += p.x; s1[j] += p.y;
          }
        } else {
#pragma unroll
          for (int wv = 0; wv < 8; ++wv) s0[j] += red[slot][wv][r][lb + eunit];
        }
      }
      if (lane == 0) __hip_atomic_fetch_add(&lds_free[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      float pub[2], va[2], vb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (!cand) {
          va[j] = fast_sigmoid(z0[j] + s0[j]);             // r
          vb[j] = fast_sigmoid(z1[j] + s1[j]);             // u
          pub[j] = va[j] * hp[j];                          // r * h_{t-1}
        } else {
          va[j] = fast_tanh(z0[j] + s0[j]);                // c
          const float u = z1[j];
          const float h1 = u * hp[j] + (1.0f - u) * va[j];
          vb[j] = live[j] ? h1 : hp[j];                    // dynamic_rnn copy-through
          pub[j] = vb[j];
        }
        if (!evalid[j]) pub[j] = 0.f;
      }
      if (m + 1 < HT) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float h1 = row_shl<1>(pub[j]), h2 = row_shl<2>(pub[j]), h3 = row_shl<3>(pub[j]);
          if ((eunit & 3) == 0) {
            u32x4 v;
            v.x = __float_as_uint(pub[j]); v.y = __float_as_uint(h1); v.z = __float_as_uint(h2); v.w = __float_as_uint(h3);
            const int erow = 8 * j + (lane >> 3);
            const unsigned off = ((unsigned)(T * QH + (ug >> 1)) * 256u + (unsigned)(erow * 16 + (ug & 1) * 8 + eunit)) * 4u;
            __builtin_amdgcn_raw_buffer_store_b128(v, image(m + 1), (int)off, 0, AUX_STORE);
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0)
          __hip_atomic_fetch_add(a.ctl + CTL_HDR + (T * NSH + (blockIdx.x & (NSH - 1))) * 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (evalid[j]) {
          const int brow = T * 16 + 8 * j + (lane >> 3);
          const long long idx = ((long long)t * B + brow) * H + ug * 8 + eunit;
          if (!cand) {
            float* zr = a.zg + ((long long)t * B + brow) * 2 * H + ug * 8 + eunit;
            zr[0] = va[j]; zr[H] = vb[j];
            a.rh[idx] = va[j] * hp[j];
          } else {
            a.zc[idx] = va[j];
            a.hs[idx + (long long)B * H] = vb[j];
            if (a.out) a.out[idx] = live[j] ? vb[j] : 0.f;
          }
        }
      }
    }
  }
  if (ew == 0 && lane == 0) { check_placement(a.ctl, a.stats); propagate_error(a.ctl); }
}
