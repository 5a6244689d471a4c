"""Training-time data augmenters (W/data_augmentation.py + W/all_data_augmentation/*.py), chosen by --data_augmenter through
train.find_class_by_name.  Each ``augment(model_input_raw, num_frames, labels_batch, **unused_params)`` returns
``(model_input, labels_batch, num_frames)``; TrainGraph.step calls it once per step, before the feature transformer, and never at
evaluation or inference ("will not persist in inference", W/train.py:337).

The reference augments the reader's dequantised floats.  Here frame-level batches are the reader's uint8 bytes, and the byte path
stays a byte path where it can: HalfAugmenter hands on a uint8 batch of 3B videos that every byte-path plugin consumes unchanged.
The kernels are in csrc/augment.hip."""
import torch

from . import ops
from .flags import DEFINE_string, DEFINE_float, FLAGS
from .variables import get_default_graph

# W/data_augmentation.py:3-6
DEFINE_string("data_augmenter", "DefaultAugmenter", "how to preprocess feature, defaults to identical, which means no transform")
DEFINE_float("input_noise_level", 0.2, "the standard deviation of normal noise added to input")


def _refuse_unpaired_rows(name, weights, distill_labels_batch):
    """The reference tiles only the labels (half_augmenter.py:36-43): per-video weights or distillation labels of B rows against a
    3B-row batch fail there with a shape error.  Here: a ValueError that names the conflict."""
    if weights is not None:
        raise ValueError("%s makes 3 rows of every video but does not tile the per-video weights (boosting): the two do not go "
                         "together" % name)
    if distill_labels_batch is not None:
        raise ValueError("%s makes 3 rows of every video but does not tile the distillation labels: the two do not go together" % name)


def _tile3(labels_batch):
    return None if labels_batch is None else torch.cat([labels_batch, labels_batch, labels_batch], dim=0)


def _require_frames(name, model_input_raw):
    if model_input_raw.dim() != 3:
        raise ValueError("%s only works with frame features [batch, frames, features] (got %d dimensions): set --frame_features "
                         "and a frame-level reader" % (name, model_input_raw.dim()))


def _short_videos(num_frames):
    """Does the batch hold a video of fewer than 2 frames?  The reader hands num_frames over on the host: no synchronisation then
    (a device tensor costs one)."""
    return bool((num_frames < 2).any())


class DefaultAugmenter(object):
    """W/all_data_augmentation/default_augmenter.py: the identity."""

    def augment(self, model_input_raw, num_frames, labels_batch, **unused_params):
        return model_input_raw, labels_batch, num_frames


class NoiseAugmenter(object):
    """W/all_data_augmentation/noise_augmenter.py:8-12: x + N(0, input_noise_level^2) over the WHOLE tensor, the padding frames of a
    frame batch included.  Video-level floats: ops.add_noise.  The reader's uint8 frames: dequantised and noised in one pass
    (ops.dequant_noise); noise on padding frames is no byte value, so the step continues on the plugins' float path, as in the
    reference.  seed: the Philox key (default: the graph's next random-op key; TrainGraph.step passes Graph.augmenter_seed())."""

    def augment(self, model_input_raw, num_frames, labels_batch, seed=None, **unused_params):
        stddev = float(FLAGS.input_noise_level)
        if seed is None:
            seed = get_default_graph().next_random_seed()
        if model_input_raw.dtype == torch.uint8:
            _require_frames("NoiseAugmenter on uint8 input", model_input_raw)
            return ops.dequant_noise(model_input_raw, num_frames, stddev, seed), labels_batch, num_frames
        return ops.add_noise(model_input_raw, stddev, seed=seed), labels_batch, num_frames


class HalfAugmenter(object):
    """W/all_data_augmentation/half_augmenter.py:8-45: [originals; first halves; second halves], 3B videos, labels tiled the same way,
    num_frames [n; s; s] with s = max(n // 2, 1).  uint8 frames stay uint8 (ops.half_segments on the bytes).  A video of fewer than
    2 frames gets a half whose one valid frame lies in the padding: the reference hands the model a ZERO FLOAT frame there, which no
    byte dequantises to -- such a batch is dequantised first (padding 0) and split on the float path."""

    name = "HalfAugmenter"

    def augment(self, model_input_raw, num_frames, labels_batch, weights=None, distill_labels_batch=None, **unused_params):
        _require_frames(self.name, model_input_raw)
        _refuse_unpaired_rows(self.name, weights, distill_labels_batch)
        x = model_input_raw
        if x.dtype == torch.uint8 and _short_videos(num_frames):
            x = ops.dequantize_frames(x, num_frames)
        y, nf = ops.half_segments(x, num_frames)
        return y, _tile3(labels_batch), nf


class HalfVideoAugmenter(object):
    """W/all_data_augmentation/half_video_augmenter.py:8-16: HalfAugmenter's 3B frame blocks averaged over the frames,
    reduce_sum(axis=1) / num_frames -> [3B, D], in one pass over the reader's bytes (ops.half_segment_means).  A block with no real
    frame gives a zero row; n = 0 (0/0 in the reference) gives 0 as ops.dequant_mean_l2norm does.  fold_l2norm: also apply the
    DefaultTransformer's L2 normalisation (TrainGraph passes it when that is the transformer)."""

    name = "HalfVideoAugmenter"

    def augment(self, model_input_raw, num_frames, labels_batch, weights=None, distill_labels_batch=None, fold_l2norm=False,
                **unused_params):
        _require_frames(self.name, model_input_raw)
        _refuse_unpaired_rows(self.name, weights, distill_labels_batch)
        if model_input_raw.dtype != torch.uint8:
            raise TypeError("HalfVideoAugmenter averages the reader's uint8 frames (got %s)" % model_input_raw.dtype)
        x = ops.half_segment_means(model_input_raw, num_frames, l2norm=fold_l2norm)
        nf = num_frames.to(torch.int32)
        s = torch.clamp(torch.div(nf.clamp(0, model_input_raw.shape[1]), 2, rounding_mode="floor"), min=1)
        return x, _tile3(labels_batch), torch.cat([nf, s, s], dim=0)


def __getattr__(name):
    # W/all_data_augmentation/clipping_augmenter.py cannot run in the reference (it reads an undefined FLAGS.frame_feature, :9, and
    # returns an undefined num_frames_new, :26): a lookup by its name says so instead of a bare StopIteration
    if name == "ClippingAugmenter":
        raise ValueError("ClippingAugmenter is not provided: the reference's own version cannot run (it reads the undefined flag "
                         "frame_feature and returns the undefined num_frames_new)")
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
