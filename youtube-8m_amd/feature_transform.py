"""Input transformers (W/feature_transform.py + W/all_feature_transform/*.py), chosen by --feature_transformer through
train.find_class_by_name.  Each ``transform(model_input_raw, num_frames)`` returns ``(model_input, num_frames)``; TrainGraph calls it
right behind the data augmenter in training steps and on the batch as it is in evaluation and inference."""
import torch

from . import ops
from .flags import DEFINE_integer, DEFINE_string, FLAGS

# W/feature_transform.py:3-8
DEFINE_string("feature_transformer", "DefaultTransformer", "how to preprocess feature, defaults to identical")
DEFINE_string("engineer_types", "identical,avg,std,diff", "EngineerTransformer's feature list (accepted; without effect, as in the reference)")
DEFINE_integer("time_resolution", 8, "ResolutionTransformer: how many consecutive frames are averaged into one")


def _require_frames(name, model_input_raw):
    if model_input_raw.dim() != 3:
        raise ValueError("%s only works with frame features [batch, frames, features] (got %d dimensions): set --frame_features "
                         "and a frame-level reader" % (name, model_input_raw.dim()))


class DefaultTransformer(object):
    """L2-normalise the feature axis.  uint8 inputs are the raw reader bytes: dequantise (W/utils.py:23-38),
    zero the padding rows (W/readers.py:178-187) and normalise in ONE pass over the uint8 block."""

    def transform(self, model_input_raw, num_frames, **unused_params):
        if model_input_raw.dtype == torch.uint8:
            return ops.dequant_l2norm(model_input_raw, num_frames), num_frames
        return ops.l2norm_fwd(model_input_raw), num_frames


class IdenticalTransformer(object):
    def transform(self, model_input_raw, num_frames, **unused_params):
        return model_input_raw, num_frames


class ResolutionTransformer(object):
    """W/all_feature_transform/resolution_transformer.py:7-29: the mean of every --time_resolution consecutive frames, l2-normalised,
    [B,F,D] -> [B, F // r, D]; the frames past (F // r) r are dropped and the num_frames it returns is num_frames // r (both the
    reference's integer divisions), so a video shorter than r frames reaches the model with num_frames = 0.  One pass over the frames
    (ops.resolution_mean): the reader's uint8 bytes are dequantised with the padding frames 0 and every mean divides by r, as the
    reference's reduce_mean over the zero-padded floats does; float frames are averaged as they are.
    After the augmenters: HalfAugmenter's 3B-row uint8 batch takes the byte kernel and NoiseAugmenter's float batch the float kernel,
    each unchanged in kind; HalfVideoAugmenter hands over 2-D rows, which are refused like any video-level input."""

    def transform(self, model_input_raw, num_frames, **unused_params):
        _require_frames("ResolutionTransformer", model_input_raw)
        return ops.resolution_mean(model_input_raw, num_frames, FLAGS.time_resolution, l2norm=True)


class AvgTransformer(object):
    """W/all_feature_transform/avg_transformer.py:4-12: frames [B,F,D] -> l2_normalize(reduce_sum(frames, 1) / num_frames) [B,D], with
    num_frames unchanged.  The reader's uint8 bytes: ops.dequant_mean_l2norm (one pass, padding frames 0).  Floats: the sum over ALL F
    frames, as there, over num_frames, then ops.l2norm_fwd.  A video with num_frames = 0 is 0/0 in the reference; here its row is pinned
    to 0 on both paths (the byte kernel already does that)."""

    def transform(self, model_input_raw, num_frames, **unused_params):
        _require_frames("AvgTransformer", model_input_raw)
        if model_input_raw.dtype == torch.uint8:
            return ops.dequant_mean_l2norm(model_input_raw, num_frames.to(model_input_raw.device)), num_frames
        n = num_frames.to(device=model_input_raw.device, dtype=torch.float32).unsqueeze(1)
        avg_pooled = torch.where(n > 0, model_input_raw.sum(dim=1) / n, torch.zeros((), device=model_input_raw.device))
        return ops.l2norm_fwd(avg_pooled), num_frames


class EngineerTransformer(DefaultTransformer):
    """W/all_feature_transform/engineer_transformer.py:9-24 as it actually computes: :23 concatenates ``model_input_raw``, not the
    ``feature_list`` built above it, so the avg / std / diff features are made and thrown away and the result is
    l2_normalize(model_input_raw) -- the DefaultTransformer.  --engineer_types is accepted and has no effect, as there.  The
    reference's ``mask_emb`` variable (:36, untrainable, read only by the discarded features) is not created.  As a subclass of
    DefaultTransformer it gets the byte-path fold of TrainGraph._transform for free: a plugin that accepts the reader's uint8 frames
    still sees them."""
