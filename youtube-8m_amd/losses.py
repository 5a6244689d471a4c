"""Label losses; names, flags and semantics mirror W/losses.py (W = /root/reference/youtube-8m-wangheda).

Here: CrossEntropyLoss, WeightedCrossEntropyLoss, MeanSquareErrorLoss, HingeLoss, MultiTaskCrossEntropyLoss,
BatchAgreementCrossEntropyLoss and TopKBatchAgreementCrossEntropyLoss, and from Z/losses.py SplitSoftmaxLoss and the --loss_function
branches of its CrossEntropyLoss.  Every one runs as HIP kernels (csrc/elementwise.hip for the plain cross entropy, csrc/softmax_moe.hip
for SplitSoftmaxLoss, csrc/xent_variants.hip for --loss_function, csrc/losses.hip for the others), forward and backward.

Left out of W/losses.py:
  PairwiseHingeLoss, MixedLoss                                  they unstack the batch by --batch_size and draw TF random integers
                                                                (tf.random_uniform, dtype int32), for which this repository has no
                                                                parity definition.
  SoftmaxLoss, MultiTaskCrossEntropyAndSoftmaxLoss              W's classes of these names put tf.nn.softmax over the PREDICTIONS and
                                                                no script of either submission uses them.  Z's SoftmaxLoss is a
                                                                different function under the same name: SplitSoftmaxLoss below.
  MultiTaskDivergenceCrossEntropyLoss,                          they take [batch, models, classes] support predictions from plugins
  MultiTaskDivergenceCrossEntropyAndMSELoss                     this repository does not have.
--label_loss with one of these names ends in StopIteration at train.find_class_by_name, as any unknown name does.

From Z/losses.py (Z = youtube-8m-zhangteng): calculate_loss_mix's default branch -- calculate_loss(predictions) + 0.1 *
calculate_loss(predictions_class, the labels tiled) -- is a training rule, not a loss class: train.TrainGraph._mix_loss.  Left out of it:
  its --support_type branches "class", "frequent", "encoder"    --support_type is W's flag here and has W's meaning; no model of the
                                                                final submission's list sets Z's.
  calculate_loss_mix2                                           it reads "predictions_encoder" and autoencoder files no plugin here has.
Z's SoftmaxLoss (Z/losses.py:412-456), the loss written for MoeSoftmaxModel, is here under the name SplitSoftmaxLoss (the name
SoftmaxLoss stays W's, above): --label_loss=SplitSoftmaxLoss; csrc/softmax_moe.hip.
Z's --loss_function (Z/losses.py:64-168) selects a branch inside CrossEntropyLoss.calculate_loss: loss_square, loss_sqrt, loss_jsd (with
--jsd_pi), loss_mix, loss_weight, loss_margin and loss_relabel are here (CrossEntropyLoss below); the final submission's entries 1 and
29.2 train MoeMix4Model under loss_relabel and loss_weight.  Left out of the rest of Z/losses.py:
  loss_smoothing                                                it reads ./resources/embedding_matrix.model, a file this repository has
                                                                no source for: --loss_function=loss_smoothing raises ValueError.
  calculate_loss_distill* (the whole family),                   they take distillation labels, negative samples or post-processing
  calculate_loss_negative, calculate_loss_max,                  inputs through call sites of Z/train.py that no plugin of the final
  calculate_loss_postprocess                                    submission's list here goes through.
  CrossEntropyLoss_weight                                       a class of its own that reads per-class weights from a file."""
import torch

from . import ops
from .flags import FLAGS, DEFINE_float, DEFINE_string, DEFINE_integer, DEFINE_bool

# W/losses.py:22-44
DEFINE_float("false_negative_punishment", 1.0, "punishment constant to 1 classified to 0")
DEFINE_float("false_positive_punishment", 1.0, "punishment constant to 0 classified to 1")
DEFINE_integer("num_classes", 4716, "number of classes")
DEFINE_float("support_loss_percent", 0.1, "the part that support loss (in multi-task scenario) take in the whole loss function.")
DEFINE_string("support_type", "vertical", "type of support label, vertical or frequent or vertical,frequent.")
DEFINE_integer("num_supports", 25, "Number of total support categories.")
DEFINE_integer("num_verticals", 25, "Number of total vertical categories.")
DEFINE_integer("num_frequents", 200, "Number of total frequent categories.")
DEFINE_string("vertical_file", "resources/vertical.tsv", "Location of label-vertical mapping file.")
DEFINE_float("batch_agreement", 0.1, "the batch_agreement parameter")
DEFINE_bool("label_smoothing", False, "whether do label smoothing")
DEFINE_float("label_smoothing_epsilon", 0.1, "whether do label smoothing")
# Z/losses.py:33-38
DEFINE_string("loss_function", None, "different loss functions used in CrossEntropyLoss.")
DEFINE_float("jsd_pi", 0.5, "weight used when loss function is loss_jsd.")

LOSS_FUNCTIONS = ("loss_square", "loss_sqrt", "loss_jsd", "loss_mix", "loss_weight", "loss_margin", "loss_relabel")


def smoothing(labels):
    """W/losses.py:46-54: y*(1-eps) + (sum_l y / K)*eps.  (Label preparation: not differentiated.)"""
    epsilon = FLAGS.label_smoothing_epsilon
    y = labels.to(torch.float32)
    prior = y.sum(dim=1, keepdim=True) / y.shape[1]
    return y * (1.0 - epsilon) + prior * epsilon


def load_vertical_mapping(path, num_classes, num_verticals):
    """W/losses.py:233-243: every line holding exactly two integers "class vertical" sets vm[class, vertical] = 1; other lines
    are skipped (a non-integer token raises, as in the reference).  Returns a float32 numpy array [num_classes, num_verticals]."""
    import numpy as np
    vm = np.zeros((num_classes, num_verticals), dtype=np.float32)
    with open(path) as fh:
        for line in fh:
            group = [int(t) for t in line.strip().split()]
            if len(group) == 2:
                x, y = group
                vm[x, y] = 1
    return vm


_VERTICAL_MAPPINGS = {}      # (file, num_classes, num_verticals, device) -> device tensor (the reference's untrainable variable "vm")


def _vertical_mapping(device):
    key = (FLAGS.vertical_file, FLAGS.num_classes, FLAGS.num_verticals, str(device))
    vm = _VERTICAL_MAPPINGS.get(key)
    if vm is None:
        vm = torch.from_numpy(load_vertical_mapping(FLAGS.vertical_file, FLAGS.num_classes, FLAGS.num_verticals)).to(device)
        _VERTICAL_MAPPINGS[key] = vm
    return vm


class BaseLoss(object):
    """W/losses.py:56-73."""

    def calculate_loss(self, unused_predictions, unused_labels, **unused_params):
        raise NotImplementedError()


class CrossEntropyLoss(BaseLoss):
    """W/losses.py:110-130: probability-space cross entropy, epsilon = 10e-6, sum over classes, mean over batch,
    optional per-example weights.

    --loss_function (Z/losses.py:64-168) replaces it, here as in Z and so for everything that calls this method (the mix loss, the
    frames loss and both terms of MultiTaskCrossEntropyLoss), by mean_b sum_v -c + m, with e = 10e-6 and
    ce(q, t) = t log(q + e) + (1 - t) log(1 - q + e):
      loss_square   c = ce(p p, y)                    loss_sqrt   c = ce(sqrt(p), y)
      loss_jsd      a = --jsd_pi, d = (1 - a) y + a p: c = (1 - a) p log(d + e) + (1 - a)(1 - p) log(1 - d + e) + a y log(d + e)
                    + a (1 - y) log(1 - d + e) - (1 - a) p log(p + e) - (1 - a)(1 - p) log(1 - p + e)
      loss_mix      c = ce(p, y) + p log(y + e) + (1 - p) log(1 - y + e) - p log(p + e) - (1 - p) log(1 - p + e)
      loss_weight   c = 10 y log(p + e) + (1 - y) log(1 - p + e)
      loss_margin   c = ce(p, y), m = -(pos - neg), pos = sum(p wp) / sum(wp) mean_b(sum_v y) with wp = (0.5 - log(p + e)) y and
                    neg = sum(p wn) / sum(wn) mean_b(sum_v (1 - y)) with wn = (1 - y)(0.5 - log(1 - p + e)), every sum over the whole
                    tensor of the call.  A batch without a positive is 0 / 0: NaN, as in the reference.
      loss_relabel  c = 0 (the reference multiplies it by 0.0); with pre = mean_b sum_v -ce(p, y): m = pre if pre < 10, else the same
                    on y' = y + add (1 - y), add the one-hot of the row's argmax of p (lowest index of a tie, over the whole row of the
                    call: one added label per L V-wide row of predictions_class).  The branch is taken on the device.
    The reference puts no stop_gradient in this chain: the gradient runs through every p above, both quotients of loss_margin
    included; the condition, the argmax and y' of loss_relabel carry none.  `scale` multiplies the whole result, m included.
    With --loss_function set: `weights` that are not None raise ValueError (Z defines none), so does --label_smoothing (neither
    reference defines the combination), loss_smoothing (above) and -- a deliberate difference: Z falls through to the plain cross
    entropy silently, and a typo must not train the wrong loss -- any other unknown value."""

    def calculate_loss(self, predictions, labels, weights=None, scale=1.0, **unused_params):
        kind = FLAGS.loss_function
        if kind is not None:
            if kind == "loss_smoothing":
                raise ValueError("--loss_function=loss_smoothing reads ./resources/embedding_matrix.model (Z/losses.py:144), "
                                 "a file this repository has no source for")
            if kind not in LOSS_FUNCTIONS:
                raise ValueError("unknown --loss_function=%r: one of %s" % (kind, ", ".join(LOSS_FUNCTIONS)))
            if weights is not None:
                raise ValueError("--loss_function=%s takes no per-example weights (Z/losses.py:64 defines none)" % kind)
            if FLAGS.label_smoothing:
                raise ValueError("--label_smoothing with --loss_function=%s: neither reference defines the combination" % kind)
            return ops.xent_variant(predictions, labels, kind, c0=FLAGS.jsd_pi, scale=scale)
        y = smoothing(labels) if FLAGS.label_smoothing else labels
        return ops.cross_entropy(predictions, y, weights, scale)


class WeightedCrossEntropyLoss(BaseLoss):
    """W/losses.py:76-93: cross entropy whose two terms carry --false_negative_punishment and --false_positive_punishment."""

    def calculate_loss(self, predictions, labels, **unused_params):
        y = smoothing(labels) if FLAGS.label_smoothing else labels
        return ops.pointwise_loss(predictions, y, "weighted_xent", FLAGS.false_negative_punishment, FLAGS.false_positive_punishment)


class MeanSquareErrorLoss(BaseLoss):
    """W/losses.py:96-108: mean_b sum_v (y - p)^2."""

    def calculate_loss(self, predictions, labels, **unused_params):
        y = smoothing(labels) if FLAGS.label_smoothing else labels
        return ops.pointwise_loss(predictions, y, "mse")


class HingeLoss(BaseLoss):
    """W/losses.py:132-148: mean_b sum_v max(0, b - (2y - 1) p); the subgradient at the kink is 0 (tf.maximum hands a tie's
    gradient to its first argument, the zeros).  No label smoothing, as in the reference."""

    def calculate_loss(self, predictions, labels, b=1.0, **unused_params):
        return ops.pointwise_loss(predictions, labels, "hinge", b)


class BatchAgreementCrossEntropyLoss(BaseLoss):
    """W/losses.py:281-320: cross entropy that weighs up the elements which break the batch-wide order.  With min_pp the smallest
    prediction of a positive and max_np the largest of a negative in the whole batch, a positive below max_np is a false negative,
    a negative above min_pp a false positive; n and c are the number and the mean prediction of either set, r = max(eps, max_np -
    min_pp), and

        w = 1 + a (sigmoid(3 (c_fp - p) / r) (n_fp / N) fn + sigmoid(3 (p - c_fn) / r) (n_fn / N) fp),   loss = mean_b sum_v w ce

    with a = --batch_agreement and N = float(--batch_size): the flag, not the number of rows (under data parallelism the statistics
    are those of the local batch, as with batch normalisation, and N is still the flag).  The reference puts no stop_gradient on w:
    the gradient also runs through w's own p, through both centres and through r into the positions of the two extrema (ties share
    it equally); the comparisons and counts carry none.  A batch without a false negative or without a false positive has c = 0/0:
    the loss is NaN there as it is in the reference (a perfectly separated batch ends the run; nothing is substituted).  Label
    smoothing and `weights` do not apply (the latter are swallowed like every unused parameter)."""

    def calculate_loss(self, predictions, labels, **unused_params):
        return ops.batch_agreement_cross_entropy(predictions, labels, FLAGS.batch_agreement, float(FLAGS.batch_size))


class TopKBatchAgreementCrossEntropyLoss(BaseLoss):
    """W/losses.py:322-356: with tau_b the 20th largest prediction of row b (k is 20 whatever `topk` says, as in the reference),
    m = [p >= tau_b] and min_pp the smallest prediction of a positive inside its row's top 20 (1 if there is none), a positive below
    tau_b is a false negative and a negative inside the top 20 and above min_pp a false positive: w = 1 + a (fn + fp) under
    stop_gradient, loss = mean_b sum_v w ce.  Fewer than 20 classes: ValueError (tf.nn.top_k refuses them)."""

    def calculate_loss(self, predictions, labels, topk=20, **unused_params):
        return ops.topk_batch_agreement_cross_entropy(predictions, labels, FLAGS.batch_agreement)


class SplitSoftmaxLoss(BaseLoss):
    """Z/losses.py:412-456, Z's SoftmaxLoss: cross entropy on the first --softmax_bound labels; the others' labels are divided by their
    row sum (at least 10e-8) with 1 - max appended, their predictions get 1 - sum appended, and the two-sided log loss with eps = 10e-8
    is summed over the row; the mean over the batch of both.  ops.split_softmax_loss (csrc/softmax_moe.hip).
    One deliberate difference from the reference: the appended probability is max(1 - sum, 0), its gradient taken as if unclamped.  In
    exact arithmetic it is MoeSoftmaxModel's dropped column q >= 0; in float32 the model's own output gives 1 - sum = -1.19e-7 < -10e-8
    whenever the dropped column holds little mass, and the reference's log returns NaN (as with MoeDistillChainNormModel's 0 / 0 rule,
    video_level_models.py).
    Z defines no `weights`: one that is not None raises ValueError.  Label smoothing does not apply (the labels are renormalised)."""

    def calculate_loss(self, predictions, labels, weights=None, scale=1.0, **unused_params):
        from . import video_level_models  # noqa: F401  (defines --softmax_bound and --moe_layers)
        if weights is not None:
            raise ValueError("SplitSoftmaxLoss takes no per-example weights (Z/losses.py:424 defines none)")
        return ops.split_softmax_loss(predictions, labels, int(FLAGS.softmax_bound), scale)

    def calculate_loss_mix(self, predictions, predictions_class, labels, weights=None, **unused_params):
        """Z/losses.py:448-456: calculate_loss(predictions) + 0.1 * sum_{i < --moe_layers} calculate_loss(predictions_class[:, i V:(i + 1) V]):
        the bound splits every V-wide piece, which is read in place."""
        from . import video_level_models  # noqa: F401
        V, layers = labels.shape[1], int(FLAGS.moe_layers)
        if predictions_class.shape[1] < layers * V:
            raise ValueError("predictions_class is %d wide for --moe_layers=%d pieces of %d labels" % (predictions_class.shape[1], layers, V))
        loss = self.calculate_loss(predictions, labels, weights=weights)
        for i in range(layers):
            loss = loss + self.calculate_loss(predictions_class[:, i * V:(i + 1) * V], labels, weights=weights, scale=0.1)
        return loss


class MultiTaskLoss(BaseLoss):
    """W/losses.py:216-257 (virtual)."""

    def calculate_loss(self, unused_predictions, unused_labels, **unused_params):
        raise NotImplementedError()

    def get_support(self, labels, support_type=None):
        if support_type is None:
            support_type = FLAGS.support_type
        if "," in support_type:
            return torch.cat([self.get_support(labels, st).to(torch.float32) for st in support_type.split(",")], dim=1)
        if support_type == "label":
            return labels.to(torch.float32)
        if support_type == "frequent":
            return labels[:, :FLAGS.num_frequents].to(torch.float32)
        if support_type == "vertical":
            # W/losses.py:229-246: labels . vm > 0.2 with vm the 0/1 class -> vertical table of --vertical_file (the file itself
            # comes from the reference's eda/ tooling, SURVEY.md 2.1: supply it; a missing file raises here as open() does there)
            float_labels = labels.to(torch.float32).contiguous()
            if float_labels.shape[1] != FLAGS.num_classes:
                raise ValueError("labels have %d classes, --num_classes is %d" % (float_labels.shape[1], FLAGS.num_classes))
            vertical_labels = ops.gemm(float_labels, _vertical_mapping(labels.device))
            return (vertical_labels > 0.2).to(torch.float32)
        raise NotImplementedError()


class MultiTaskCrossEntropyLoss(MultiTaskLoss):
    """W/losses.py:271-279: (1-s)*CE(pred, y) + s*CE(support_pred, support(y))."""

    def calculate_loss(self, predictions, support_predictions, labels, **unused_params):
        support_labels = self.get_support(labels)
        s = FLAGS.support_loss_percent
        ce = CrossEntropyLoss()
        kw = {k: v for k, v in unused_params.items() if k != "scale"}
        return (ce.calculate_loss(predictions, labels, scale=1.0 - s, **kw)
                + ce.calculate_loss(support_predictions, support_labels, scale=s, **kw))
