// frame_subset.hip -- random half-frame inference (Z/frame_level_models.py:6189-6217 FrameRandomEvalModel, :6138-6167
// FrameAttentionEvalModel, :4038-4057 LstmRandomModel): E replicas of every video, each holding an order-preserving random K-subset of
// its F frames (gfx950, wave64).
//   draw:   index [E,K] -- ONE uniformly random K-subset of 0..F-1 per replica, ascending, shared by every video of the batch (the
//           reference shuffles the rows of an [F,B] tensor: one permutation per replica)
//   gather: y [B E, K, D] -- row b E + e holds frames index[e, :] of video b; a chosen frame at or past num_frames[b] is a zero row, so
//           the replica is a well-formed padded video of num_frames_out[b E + e] frames (the indices ascend: its real frames come first)
// TensorFlow's random stream is not reproduced; the distribution is: frame f of replica e takes a 32-bit Philox key and the subset is the
// K frames with the smallest (key, f) pairs -- the first K entries of the permutation that sorts the keys.
#include <algorithm>
#include "common.h"
#include "philox.h"

namespace {

constexpr int DRAW_MAX_F = 1024;         // one thread per frame and a replica's keys in LDS (4 KiB)

// One workgroup per replica e, thread f = frame f.  Key of frame f: the word of logical element e F4 + f (F4 = F rounded up to a multiple
// of 4) in random.hip's layout -- counter (element >> 2, 0), word element & 3, key = seed -- so a block of four words never straddles two
// replicas; the words at and past F are stored as 2^32 - 1, which no frame sorts behind (their position is above every f).  Frame f is
// chosen when fewer than K frames sort before it by (key, f): F compares, the keys read four to an LDS access, the same address in every
// lane.  Its output position is the number of chosen frames below it: the wave's ballot below the lane plus the counts of the waves
// before.  Counting only, no atomics: a rerun is bit-equal.
__global__ __launch_bounds__(DRAW_MAX_F) void frame_subset_draw_kernel(int32_t* __restrict__ index, int F, int K, uint64_t seed) {
  __shared__ uint4 key4[DRAW_MAX_F / 4];
  __shared__ int wave_chosen[DRAW_MAX_F / 64];
  const uint32_t* key = reinterpret_cast<const uint32_t*>(key4);
  const int e = blockIdx.x, groups = (F + 3) / 4, f = threadIdx.x, lane = f & 63, wave = f >> 6;
  if (f < groups) {
    const yt8m_rng::U4 r = yt8m_rng::philox4x32_10((uint64_t)e * (uint64_t)groups + (uint64_t)f, seed);
    const int o = 4 * f;
    key4[f] = uint4{r.x, o + 1 < F ? r.y : 0xFFFFFFFFu, o + 2 < F ? r.z : 0xFFFFFFFFu, o + 3 < F ? r.w : 0xFFFFFFFFu};
  }
  __syncthreads();
  bool chosen = false;
  if (f < F) {
    const uint32_t w = key[f];
    int rank = 0;
    for (int g = 0; g < groups; ++g) {
      const uint4 k = key4[g];
      const int o = 4 * g;
      rank += (k.x < w || (k.x == w && o < f)) + (k.y < w || (k.y == w && o + 1 < f)) + (k.z < w || (k.z == w && o + 2 < f)) +
              (k.w < w || (k.w == w && o + 3 < f));
    }
    chosen = rank < K;
  }
  const unsigned long long mask = __ballot(chosen);          // every thread of the workgroup gets here
  if (lane == 0) wave_chosen[wave] = __popcll(mask);
  __syncthreads();
  if (chosen) {
    int pos = __popcll(mask & ((1ull << lane) - 1ull));
    for (int v = 0; v < wave; ++v) pos += wave_chosen[v];
    index[(int64_t)e * K + pos] = f;     // the ranks are a permutation of 0..F-1: exactly K frames are chosen, pos < K
  }
}

// x [B,F,D] -> y [B E,K,D]: V = a 16-byte vector (rows of a multiple of 16 bytes) or one element; nv = V units per frame row.  A
// grid-stride loop over (output row, vector) items, a row's vectors on adjacent threads (as half_segments_kernel, augment.hip).  The item
// arithmetic is 32 bits wide: three divisions per 16-byte item, which in 64 bits would cost more issue slots than the copy has to spare
// (the launcher refuses shapes whose items or source offsets do not fit).  A chosen frame outside [0, n_b) -- padding, or an index
// outside [0, F) -- is written as zeros and x is not read there.  num_frames_out: one wave per output video, the lanes over its K indices.
template <typename V>
__global__ __launch_bounds__(256) void frame_subset_gather_kernel(const V* __restrict__ x, const int32_t* __restrict__ nf,
                                                                  const int32_t* __restrict__ index, V* __restrict__ y,
                                                                  int32_t* __restrict__ nf_out, uint32_t B, uint32_t F, uint32_t nv,
                                                                  uint32_t E, uint32_t K) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * 4, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  for (uint32_t r = wave; r < B * E; r += waves) {           // wave-uniform: every lane reaches the ballots
    const uint32_t b = r / E, e = r - b * E;
    const int32_t n = (int32_t)clamp_frames(nf, b, F);
    int count = 0;
    for (uint32_t j0 = 0; j0 < K; j0 += 64) {
      const uint32_t j = j0 + lane;
      const int32_t idx = j < K ? index[e * K + j] : -1;
      count += __popcll(__ballot(idx >= 0 && idx < n));
    }
    if (lane == 0) nf_out[r] = count;
  }
  const uint32_t total = B * E * K * nv, stride = gridDim.x * 256;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const uint32_t row = i / nv, v = i - row * nv;           // row = r K + j
    const uint32_t r = row / K, j = row - r * K;
    const uint32_t b = r / E, e = r - b * E;
    const int32_t idx = index[e * K + j];
    const bool live = idx >= 0 && idx < (int32_t)clamp_frames(nf, b, F);
    y[i] = live ? x[(b * F + (uint32_t)idx) * nv + v] : V{};
  }
}

unsigned copy_grid(int64_t items) {
  const int64_t blocks = (items + 255) / 256;
  return (unsigned)std::min<int64_t>(std::max<int64_t>(blocks, 1), 256 * 32);   // grid-stride beyond ~8 K blocks (32 per CU)
}

bool disjoint(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa + abytes <= pb || pb + bbytes <= pa;
}

// T: the element type; V16: its 16-byte vector
template <typename T, typename V16>
int gather_launch(const char* what, const T* x, const int32_t* num_frames, const int32_t* index, T* y, int32_t* num_frames_out, int64_t B,
                  int64_t F, int64_t D, int64_t E, int64_t K, yt8m_stream_t stream) {
  using namespace yt8m;
  YT8M_REQUIRE(B >= 0 && F >= 0 && D >= 0 && E >= 0 && K >= 0, YT8M_E_SHAPE, "negative dimension");
  if (B * E == 0) return YT8M_OK;
  YT8M_REQUIRE(x && num_frames && index && y && num_frames_out, YT8M_E_BADARG, "null operand");
  const int64_t sz = (int64_t)sizeof(T), nin = B * F * D * sz, nout = B * E * K * D * sz;
  YT8M_REQUIRE(disjoint(x, nin, y, nout), YT8M_E_BADARG, "source and destination overlap (the replicas are written out of place)");
  YT8M_REQUIRE(disjoint(num_frames_out, 4 * B * E, y, nout) && disjoint(num_frames_out, 4 * B * E, num_frames, 4 * B) &&
               disjoint(num_frames_out, 4 * B * E, index, 4 * E * K) && disjoint(index, 4 * E * K, y, nout), YT8M_E_BADARG,
               "num_frames_out or index overlaps an operand that is written");
  const int64_t per = 16 / sz;
  const bool vec = D % per == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const int64_t nv = vec ? D / per : D, items = B * E * K * nv;
  const dim3 grid(copy_grid(std::max<int64_t>(items, B * E * 64)));       // at least one wave's worth of threads per output video
  // the kernel counts in 32 bits: its loop variables go up to one grid stride past the last item (or video) before the loops end
  YT8M_REQUIRE(F <= INT32_MAX && std::max(std::max(items, B * E) + (int64_t)grid.x * 256, std::max(B * F * nv, E * K)) <= (int64_t)UINT32_MAX,
               YT8M_E_SHAPE, "more than 2^32 items (16-byte vectors, or elements where the rows are not 16-byte multiples)");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, 2.0 * (double)nout);
  const uint32_t b = (uint32_t)B, f = (uint32_t)F, n = (uint32_t)nv, e = (uint32_t)E, k = (uint32_t)K;
  if (vec) {
    hipLaunchKernelGGL(frame_subset_gather_kernel<V16>, grid, dim3(256), 0, s, reinterpret_cast<const V16*>(x), num_frames, index,
                       reinterpret_cast<V16*>(y), num_frames_out, b, f, n, e, k);
  } else {
    hipLaunchKernelGGL(frame_subset_gather_kernel<T>, grid, dim3(256), 0, s, x, num_frames, index, y, num_frames_out, b, f, n, e, k);
  }
  return launch_status(what);
}

}  // namespace

using namespace yt8m;

extern "C" int yt8m_frame_subset_draw(int32_t* index, int64_t E, int64_t F, int64_t K, uint64_t seed, yt8m_stream_t stream) {
  YT8M_REQUIRE(E >= 0 && E <= INT32_MAX, YT8M_E_SHAPE, "E must be in [0, 2^31)");
  YT8M_REQUIRE(F >= 2 && F <= DRAW_MAX_F, YT8M_E_SHAPE, "F must be in [2, 1024] (one thread per frame, a replica's keys in LDS)");
  YT8M_REQUIRE(K >= 1 && K <= F, YT8M_E_SHAPE, "K must be in [1, F]");
  if (E == 0) return YT8M_OK;
  YT8M_REQUIRE(index, YT8M_E_BADARG, "null operand");
  hipStream_t s = as_stream(stream);
  ProfScope prof(F_ELEMENTWISE, s, 0.0, 4.0 * (double)(E * K));
  hipLaunchKernelGGL(frame_subset_draw_kernel, dim3((unsigned)E), dim3(DRAW_MAX_F), 0, s, index, (int)F, (int)K, seed);
  return launch_status("frame_subset_draw_kernel");
}

extern "C" int yt8m_frame_subset_gather_u8(const uint8_t* x, const int32_t* num_frames, const int32_t* index, uint8_t* y,
                                           int32_t* num_frames_out, int64_t B, int64_t F, int64_t D, int64_t E, int64_t K,
                                           yt8m_stream_t stream) {
  return gather_launch<uint8_t, uint4>("frame_subset_gather_kernel<u8>", x, num_frames, index, y, num_frames_out, B, F, D, E, K, stream);
}

extern "C" int yt8m_frame_subset_gather_f32(const float* x, const int32_t* num_frames, const int32_t* index, float* y,
                                            int32_t* num_frames_out, int64_t B, int64_t F, int64_t D, int64_t E, int64_t K,
                                            yt8m_stream_t stream) {
  return gather_launch<float, float4>("frame_subset_gather_kernel<f32>", x, num_frames, index, y, num_frames_out, B, F, D, E, K, stream);
}
