"""Input and training-step plumbing of the ensemble stage (E = youtube-8m-ensemble of the reference; E/train.py:222-250): the stacked
predictions of M single models, read from the per-model prediction dumps that inference.write_to_record writes, handed to the plugins
of ensemble_level_models.py.

Layout: E/train.py concatenates the M readers' [B, V] batches along a new last axis (tf.expand_dims + tf.concat, :236-247): an
interleaving copy, and a tensor whose fastest axis is the method.  Here every reader's batch is copied into ITS plane of one contiguous
method-major buffer [M, B, V] and the model sees the [B, V, M] permuted view of it, strides (V, 1, B V): no interleaving copy exists, and
in the kernels of csrc/ensemble.hip every access along v is coalesced for any M.
"""
import torch

from . import feature_transform, train
from .readers import YT8MAggregatedFeatureReader
from .variables import set_default_graph


class EnsembleInput(object):
    """M lists (or glob patterns) of dump shards, in the order of the .conf file, read in lockstep with YT8MAggregatedFeatureReader
    (feature "predictions", num_classes wide).  Labels come from the first method.  input_data_pattern (the --input_data_pattern reader
    of E/train.py:222-229) adds the video-level features `original_input` [B, D] of the same videos.

    A batch whose video ids differ between the methods (or between a method and the input features) RAISES.  The reference only logs the
    share of matching ids as the summary "model/id_match" (E/train.py:243-246) and trains on; a mismatch means that the stacked rows
    belong to different videos, which no ensemble survives, so here it is an error."""

    def __init__(self, method_files, num_classes=4716, input_data_pattern=None, input_feature_names=("mean_rgb", "mean_audio"),
                 input_feature_sizes=(1024, 128), feature_name="predictions"):
        self.method_files = list(method_files)
        if not self.method_files:
            raise ValueError("EnsembleInput needs at least one method")
        self.num_classes = num_classes
        self.num_methods = len(self.method_files)
        self.reader = YT8MAggregatedFeatureReader(num_classes=num_classes, feature_sizes=[num_classes], feature_names=[feature_name])
        self.input_data_pattern = input_data_pattern
        self.input_reader = None
        if input_data_pattern is not None:
            self.input_reader = YT8MAggregatedFeatureReader(num_classes=num_classes, feature_sizes=list(input_feature_sizes),
                                                            feature_names=list(input_feature_names))

    def batches(self, batch_size=1024, device=None, check_crc=True):
        """Yields (video_ids, model_input [n, V, M] method-major view, labels bool [n, V], original_input [n, D] or None)."""
        its = [self.reader.prepare_reader(files, batch_size=batch_size, device=device, check_crc=check_crc) for files in self.method_files]
        oit = None if self.input_reader is None else self.input_reader.prepare_reader(self.input_data_pattern, batch_size=batch_size,
                                                                                       device=device, check_crc=check_crc)
        M, V = self.num_methods, self.num_classes
        while True:
            parts = [next(it, None) for it in its]
            if all(p is None for p in parts):
                if oit is not None and next(oit, None) is not None:
                    raise ValueError("EnsembleInput: the input features go on after the last batch of the methods")
                return
            if any(p is None for p in parts):
                raise ValueError("EnsembleInput: method %d ran out of videos before the others" % [p is None for p in parts].index(True))
            ids, first, labels, _ = parts[0]
            n = first.shape[0]
            buf = torch.empty((M, n, V), dtype=torch.float32, device=first.device)
            for k, (ids_k, x_k, _, _) in enumerate(parts):
                if ids_k != ids:
                    bad = next((i for i, (a, b) in enumerate(zip(ids_k, ids)) if a != b), min(len(ids_k), len(ids)))
                    raise ValueError("EnsembleInput: video ids of method %d differ from method 0's (first at row %d of the batch)" % (k, bad))
                buf[k].copy_(x_k)
            original = None
            if oit is not None:
                o = next(oit, None)
                if o is None or o[0] != ids:
                    raise ValueError("EnsembleInput: video ids of the input features differ from the methods'")
                original = o[1]
            yield ids, buf.permute(1, 2, 0), labels, original


def stack_methods(planes):
    """[B, V, M] method-major view over M [B, V] tensors (tests, tools): each copied into its plane of one [M, B, V] buffer."""
    return torch.stack(list(planes), dim=0).permute(1, 2, 0)


class EnsembleTrainGraph(train.TrainGraph):
    """train.TrainGraph for the plugins of ensemble_level_models.py.  E/train.py applies no feature transformer and no data augmenter to
    the stacked predictions (the default transformer would l2-normalise them): IdenticalTransformer is fixed here.  step / forward /
    predict take original_input= and hand it to create_model (E/train.py:262-277); everything else is the parent's step."""

    def __init__(self, model, **kw):
        if kw.get("transformer_class") not in (None, feature_transform.IdenticalTransformer) or kw.get("augmenter_class") is not None:
            raise ValueError("the ensemble stage applies no feature transformer and no data augmenter")
        kw["transformer_class"] = feature_transform.IdenticalTransformer
        super(EnsembleTrainGraph, self).__init__(model, **kw)
        self._original_input = None

    def forward(self, model_input_raw, labels_batch=None, num_frames=None, is_training=True, fuse_loss=True,
                distillation_predictions=None, transformed=False, original_input=None):
        g = set_default_graph(self.graph)
        g.begin_step()
        if original_input is None:
            original_input = self._original_input                        # step() leaves it here for the parent's forward calls
        kw = {} if is_training else {"is_training": False}
        return self.model.create_model(model_input_raw, vocab_size=model_input_raw.shape[1], labels=labels_batch,
                                       original_input=original_input, **kw)

    def step(self, model_input_raw, labels_batch, original_input=None, weights=None):
        self._original_input = original_input
        try:
            return super(EnsembleTrainGraph, self).step(model_input_raw, labels_batch, weights=weights)
        finally:
            self._original_input = None

    @torch.no_grad()
    def predict(self, model_input_raw, original_input=None, vocab_size=None):
        return self.forward(model_input_raw, is_training=False, original_input=original_input)["predictions"]
