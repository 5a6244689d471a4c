"""Restatement in numpy of random half-frame inference (Z/frame_level_models.py:6189-6217, Z = youtube-8m-zhangteng of the reference):
the draw, the gather and the counts of ops.frame_subset / csrc/frame_subset.hip.
    draw:   frame f of replica e takes the key w(e,f) = oracle.philox.words(E F4, seed)[e F4 + f] (F4 = F rounded up to a multiple of 4);
            a lexsort by (key, f), its first K entries, then a sort: one ascending K-subset of 0..F-1 per replica
    gather: y[b E + e, j] = x[b, index[e,j]] where 0 <= index[e,j] < clamp(num_frames[b], 0, F), else zeros
    counts: num_frames_out[b E + e] = the number of such j
TensorFlow's stream is not reproduced; the distribution is (a uniformly random K-subset per replica and call).
Shared by tests/test_frame_subset_host.py and tests/test_gpu_frame_subset.py; not a test module."""
import numpy as np

from oracle import philox


def draw(E, F, K, seed):
    """index [E,K] int32"""
    F4 = (F + 3) // 4 * 4
    w = philox.words(E * F4, seed).reshape(E, F4)[:, :F]
    f = np.arange(F)
    return np.stack([np.sort(np.lexsort((f, w[e]))[:K]) for e in range(E)]).astype(np.int32).reshape(E, K)


def gather(x, num_frames, index):
    """x [B,F,D], num_frames [B], index [E,K] -> (y [B E,K,D] of x's dtype, num_frames_out [B E] int32)"""
    B, F, D = x.shape
    E, K = index.shape
    n = np.clip(np.asarray(num_frames, dtype=np.int64), 0, F)
    y = np.zeros((B, E, K, D), dtype=x.dtype)
    count = np.zeros((B, E), dtype=np.int32)
    for b in range(B):
        for e in range(E):
            for j in range(K):
                i = int(index[e, j])
                if 0 <= i < n[b]:
                    y[b, e, j] = x[b, i]
                    count[b, e] += 1
    return y.reshape(B * E, K, D), count.reshape(B * E)


def frames(B, F, D, num_frames, dtype, seed=0, padding=0):
    """Frames as the reader pads them: random content in the real frames, `padding` in every element past num_frames (clamped)"""
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 256, size=(B, F, D)).astype(np.uint8) if dtype == np.uint8 else rs.randn(B, F, D).astype(np.float32)
    live = np.arange(F)[None, :] < np.clip(np.asarray(num_frames), 0, F)[:, None]
    x[~live] = padding
    return x
