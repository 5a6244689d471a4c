"""Not -m gpu: the data augmenters' host rules (W/data_augmentation.py, W/all_data_augmentation/*.py) and a numpy restatement of
half_augmenter.py / half_video_augmenter.py that the GPU tests (test_gpu_augment.py) hold the kernels to, checked here on cases worked
out by hand."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import yt8m_amd.data_augmentation as da
import yt8m_amd.train as train
from yt8m_amd.variables import AUGMENTER_CALL, Graph, random_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "youtube-8m_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


# ---- the restatement: TF's ops one by one on numpy arrays ------------------------------------------------------------------------
def half_augment_np(x, num_frames):
    """half_augmenter.py:15-45 on x [B,F,D] (the dequantised frames, or any array: the bytes), num_frames [B] -> ([3B,F,D], [3B]).
    seg_num_frames = max(num_frames / 2, 1) is int32 division; gather_nd past the frame axis reads zeros (TF's GPU kernel)."""
    x, nf = np.asarray(x), np.asarray(num_frames, dtype=np.int32)
    B, F, D = x.shape
    seg_length = max(F // 2, 1)
    seg_num_frames = np.maximum(nf // 2, 1)
    inputs, frames = [x], [nf]
    for i in range(2):
        frames_index = (seg_num_frames * i).reshape(-1, 1) + np.arange(seg_length).reshape(1, -1)       # [B, seg_length]
        seg = np.zeros((B, seg_length, D), dtype=x.dtype)
        for b in range(B):
            for t in range(seg_length):
                if frames_index[b, t] < F:
                    seg[b, t] = x[b, frames_index[b, t]]
        seg = np.concatenate([seg, np.zeros((B, F - seg_length, D), dtype=x.dtype)], axis=1)            # tf.pad
        mask = np.arange(F).reshape(1, -1) < seg_num_frames.reshape(-1, 1)                              # sequence_mask
        seg = np.where(mask[:, :, None], seg, np.zeros((), dtype=x.dtype))
        inputs.append(seg)
        frames.append(seg_num_frames.astype(np.int32))
    return np.concatenate(inputs, axis=0), np.concatenate(frames, axis=0)


def half_video_augment_np(x, num_frames):
    """half_video_augmenter.py:8-16: reduce_sum(frames, axis=1) / new_num_frames, in float64.  n = 0 gives 0/0 = nan as in the
    reference (the kernel writes 0 there)."""
    y, nf = half_augment_np(np.asarray(x, dtype=np.float64), num_frames)
    with np.errstate(invalid="ignore", divide="ignore"):
        return y.sum(axis=1) / nf.astype(np.float64).reshape(-1, 1), nf


def dequantize_np(q, num_frames):
    """utils.Dequantize in fp32 (a multiply, then an add) with the padding frames zero (readers.py resize_axis)."""
    q = np.asarray(q)
    F = q.shape[1]
    x = q.astype(np.float32) * np.float32(4.0 / 255.0) + np.float32(4.0 / 512.0 - 2.0)
    live = np.arange(F).reshape(1, -1) < np.asarray(num_frames).reshape(-1, 1)
    return np.where(live[:, :, None], x, np.float32(0.0)).astype(np.float32)


# frame f of every video holds the value f + 1 (one feature), padding frames 0: every output frame names its source
def _indexed(F, nf):
    x = np.zeros((len(nf), F, 1), dtype=np.float32)
    for b, n in enumerate(nf):
        x[b, :n, 0] = np.arange(1, n + 1)
    return x


def test_half_augmenter_restatement_on_hand_worked_cases():
    F = 5                                                                  # odd F: seg_length = 2
    nf = [0, 1, 2, 3, F - 1, F]
    y, nfo = half_augment_np(_indexed(F, nf), nf)
    assert list(nfo) == [0, 1, 2, 3, 4, 5] + [1, 1, 1, 1, 2, 2] * 2
    first = [[0, 0, 0, 0, 0],        # n = 0: s = 1, frame 0 is padding -> one zero frame
             [1, 0, 0, 0, 0],        # n = 1: frame 0
             [1, 0, 0, 0, 0],        # n = 2: s = 1
             [1, 0, 0, 0, 0],        # n = 3: s = 1
             [1, 2, 0, 0, 0],        # n = 4: s = 2
             [1, 2, 0, 0, 0]]        # n = 5: s = 2 (frame 5 is in neither half)
    second = [[0, 0, 0, 0, 0],       # n = 0: frame 1 is padding
              [0, 0, 0, 0, 0],       # n = 1: frame 1 is padding -> the zero frame the byte path cannot express
              [2, 0, 0, 0, 0],
              [2, 0, 0, 0, 0],
              [3, 4, 0, 0, 0],
              [3, 4, 0, 0, 0]]
    assert np.array_equal(y[:6, :, 0], _indexed(F, nf)[:, :, 0])
    assert np.array_equal(y[6:12, :, 0], np.array(first, dtype=np.float32))
    assert np.array_equal(y[12:, :, 0], np.array(second, dtype=np.float32))


def test_half_augmenter_restatement_at_even_F_and_full_videos():
    F = 8
    nf = [F, F - 1, 2]
    y, nfo = half_augment_np(_indexed(F, nf), nf)
    assert list(nfo) == [8, 7, 2, 4, 3, 1, 4, 3, 1]
    assert np.array_equal(y[3:6, :, 0], np.array([[1, 2, 3, 4, 0, 0, 0, 0], [1, 2, 3, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], np.float32))
    assert np.array_equal(y[6:, :, 0], np.array([[5, 6, 7, 8, 0, 0, 0, 0], [4, 5, 6, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0]], np.float32))


def test_half_video_augmenter_restatement_on_hand_worked_cases():
    F = 5
    nf = [0, 1, 2, 3, F - 1, F]
    m, nfo = half_video_augment_np(_indexed(F, nf), nf)
    m = m[:, 0]
    assert np.isnan(m[0])                                                  # the reference's 0/0 (the kernel pins 0)
    assert np.allclose(m[1:6], [1.0, 1.5, 2.0, 2.5, 3.0])                  # whole-video means
    assert np.allclose(m[6:12], [0.0, 1.0, 1.0, 1.0, 1.5, 1.5])            # first halves: n = 0 -> zero frame / 1
    assert np.allclose(m[12:], [0.0, 0.0, 2.0, 2.0, 3.5, 3.5])             # second halves: n < 2 -> zero row
    assert list(nfo) == [0, 1, 2, 3, 4, 5] + [1, 1, 1, 1, 2, 2] * 2


def test_restatement_keeps_the_bytes_as_bytes():
    rs = np.random.RandomState(0)
    q = rs.randint(0, 256, size=(3, 7, 4)).astype(np.uint8)
    nf = np.array([7, 4, 2], dtype=np.int32)
    y, _ = half_augment_np(q, nf)
    assert y.dtype == np.uint8 and y.shape == (9, 7, 4)
    assert np.array_equal(y[:3], q)
    assert np.array_equal(y[3, :3], q[0, :3]) and not y[3, 3:].any()
    assert np.array_equal(y[6, :3], q[0, 3:6]) and not y[6, 3:].any()


# ---- flags, lookup, host rules -----------------------------------------------------------------------------------------------------
def test_flag_defaults_and_lookup_by_name(flags):
    assert flags.data_augmenter == "DefaultAugmenter"
    assert flags.input_noise_level == 0.2
    for name in ("DefaultAugmenter", "NoiseAugmenter", "HalfAugmenter", "HalfVideoAugmenter"):
        assert train.find_class_by_name(name, [da]) is getattr(da, name)
    with pytest.raises(StopIteration):
        train.find_class_by_name("NoSuchAugmenter", [da])


def test_clipping_augmenter_lookup_says_why_it_is_missing():
    with pytest.raises(ValueError, match="cannot run"):
        train.find_class_by_name("ClippingAugmenter", [da])


def test_default_augmenter_is_the_identity():
    x, nf, y = torch.zeros(2, 3, 4, dtype=torch.uint8), torch.tensor([3, 1]), torch.ones(2, 5, dtype=torch.bool)
    out = da.DefaultAugmenter().augment(x, num_frames=nf, labels_batch=y)
    assert out[0] is x and out[1] is y and out[2] is nf


@pytest.mark.parametrize("cls", [da.HalfAugmenter, da.HalfVideoAugmenter])
def test_half_augmenters_refuse_video_level_input_weights_and_distillation_labels(cls):
    y, nf = torch.ones(2, 5, dtype=torch.bool), torch.tensor([3, 1])
    with pytest.raises(ValueError, match="frame features"):
        cls().augment(torch.zeros(2, 4), num_frames=nf, labels_batch=y)
    x = torch.zeros(2, 3, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="weights"):
        cls().augment(x, num_frames=nf, labels_batch=y, weights=torch.ones(2))
    with pytest.raises(ValueError, match="distillation"):
        cls().augment(x, num_frames=nf, labels_batch=y, distill_labels_batch=torch.zeros(2, 5))


def test_train_graph_holds_the_augmenter_and_build_graph_resolves_the_flag(flags):
    g = Graph(device="cpu")
    assert type(train.TrainGraph(object(), graph=g).augmenter) is da.DefaultAugmenter
    assert type(train.TrainGraph(object(), graph=g, augmenter_class=da.NoiseAugmenter).augmenter) is da.NoiseAugmenter
    flags.data_augmenter = "HalfAugmenter"
    tg = train.build_graph(object(), graph=g)
    assert type(tg.augmenter) is da.HalfAugmenter and tg.batch_size == flags.batch_size
    flags.data_augmenter = "ClippingAugmenter"
    with pytest.raises(ValueError):
        train.build_graph(object(), graph=g)


def test_augmenter_seed_differs_per_step_and_rank_and_from_the_models_own_random_ops():
    g = Graph(device="cpu", seed=3)
    s0 = g.augmenter_seed()
    assert s0 == random_seed(3, 0, 0, AUGMENTER_CALL)
    g._rng_step += 1                                                       # the next step
    assert g.augmenter_seed() != s0
    g.rank = 1
    assert g.augmenter_seed() != random_seed(3, 0, 1, AUGMENTER_CALL)
    assert s0 not in {random_seed(3, 0, 0, c) for c in range(64)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_augment_kernels_use_no_scratch():
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "--cuda-device-only", "-c", "augment.hip",
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    assert len(names) == 8 and len(scratch) == len(names), p.stderr[-2000:]
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
