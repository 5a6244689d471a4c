"""The --loss_function branches of Z's CrossEntropyLoss.calculate_loss (Z/losses.py:64-168, Z = youtube-8m-zhangteng) in plain torch, in
the dtype of their input, branch for branch and with the reference's variable names.  float64 is the reference the kernels of
csrc/xent_variants.hip are judged against, float32 the composition from torch ops that sets their tolerance and serves as the baseline
of tools/loss_function_step.py.  No module of the package is imported here."""
import torch

epsilon = 10e-6
NAMES = ("loss_square", "loss_sqrt", "loss_jsd", "loss_mix", "loss_weight", "loss_margin", "loss_relabel")


def _finish(cross_entropy_loss, margin_loss):
    cross_entropy_loss = torch.neg(cross_entropy_loss)
    return torch.mean(torch.sum(cross_entropy_loss, 1)) + margin_loss


def loss_square(predictions, labels):
    float_labels = labels.to(predictions.dtype)
    predictions = predictions * predictions
    cross_entropy_loss = float_labels * torch.log(predictions + epsilon) + (
        1 - float_labels) * torch.log(1 - predictions + epsilon)
    return _finish(cross_entropy_loss, 0.0)


def loss_sqrt(predictions, labels):
    float_labels = labels.to(predictions.dtype)
    predictions = torch.sqrt(predictions)
    cross_entropy_loss = float_labels * torch.log(predictions + epsilon) + (
        1 - float_labels) * torch.log(1 - predictions + epsilon)
    return _finish(cross_entropy_loss, 0.0)


def loss_jsd(predictions, labels, jsd_pi=0.5):
    float_labels = labels.to(predictions.dtype)
    alpha = jsd_pi
    jsd_dis = (1 - alpha) * float_labels + alpha * predictions
    cross_entropy_loss_1 = (1 - alpha) * predictions * torch.log(jsd_dis + epsilon) + (1 - alpha) * (
        1 - predictions) * torch.log(1 - jsd_dis + epsilon) + alpha * float_labels * torch.log(jsd_dis + epsilon) + alpha * (
        1 - float_labels) * torch.log(1 - jsd_dis + epsilon)
    cross_entropy_loss_2 = (1 - alpha) * predictions * torch.log(predictions + epsilon) + (1 - alpha) * (
        1 - predictions) * torch.log(1 - predictions + epsilon)
    cross_entropy_loss = cross_entropy_loss_1 - cross_entropy_loss_2
    return _finish(cross_entropy_loss, 0.0)


def loss_mix(predictions, labels):
    float_labels = labels.to(predictions.dtype)
    cross_entropy_loss_1 = float_labels * torch.log(predictions + epsilon) + (
        1 - float_labels) * torch.log(1 - predictions + epsilon)
    cross_entropy_loss_2 = predictions * torch.log(float_labels + epsilon) + (
        1 - predictions) * torch.log(1 - float_labels + epsilon)
    cross_entropy_loss_3 = predictions * torch.log(predictions + epsilon) + (
        1 - predictions) * torch.log(1 - predictions + epsilon)
    cross_entropy_loss = cross_entropy_loss_1 + cross_entropy_loss_2 - cross_entropy_loss_3
    return _finish(cross_entropy_loss, 0.0)


def loss_weight(predictions, labels):
    float_labels = labels.to(predictions.dtype)
    cross_entropy_loss = float_labels * torch.log(predictions + epsilon) * 10 + (
        1 - float_labels) * torch.log(1 - predictions + epsilon)
    return _finish(cross_entropy_loss, 0.0)


def loss_margin(predictions, labels):
    float_labels = labels.to(predictions.dtype)
    predictions_pos = torch.sum(predictions * (0.5 - torch.log(predictions + epsilon)) * float_labels) \
        / torch.sum((0.5 - torch.log(predictions + epsilon)) * float_labels) * torch.mean(torch.sum(float_labels, 1))
    predictions_neg = torch.sum(predictions * (0.5 - torch.log(1 - predictions + epsilon)) * (1 - float_labels)) \
        / torch.sum((1 - float_labels) * (0.5 - torch.log(1 - predictions + epsilon))) * torch.mean(torch.sum(1 - float_labels, 1))
    margin_loss = torch.neg(predictions_pos - predictions_neg)
    cross_entropy_loss = float_labels * torch.log(predictions + epsilon) + (
        1 - float_labels) * torch.log(1 - predictions + epsilon)
    return _finish(cross_entropy_loss, margin_loss)


def relabel_parts(predictions, labels):
    """Every intermediate of the loss_relabel branch: margin_loss_pre, whether f2 (the relabelled branch) is taken (a bool tensor), max_index [B] (the
    first index of the row maximum, as tf.arg_max), the labels f2 uses and the loss."""
    float_labels = labels.to(predictions.dtype)
    cross_entropy_loss = float_labels * torch.log(predictions + epsilon) + (
        1 - float_labels) * torch.log(1 - predictions + epsilon)
    margin_loss_pre = torch.mean(torch.sum(torch.neg(cross_entropy_loss), 1))
    batch_size, vocab_size = float_labels.shape
    row_max = predictions.detach().amax(dim=1, keepdim=True)
    labels_temp = torch.arange(vocab_size, device=predictions.device).unsqueeze(0).repeat(batch_size, 1)
    max_index = torch.where(predictions.detach() == row_max, labels_temp, torch.full_like(labels_temp, vocab_size)).amin(dim=1).reshape(-1, 1)
    labels_add = torch.where(labels_temp == max_index, torch.ones_like(float_labels), torch.zeros_like(float_labels))
    float_labels_now = float_labels + labels_add * (1.0 - float_labels)
    cross_entropy_loss_now = float_labels_now * torch.log(predictions + epsilon) + (
        1 - float_labels_now) * torch.log(1 - predictions + epsilon)
    margin_loss_now = torch.mean(torch.sum(torch.neg(cross_entropy_loss_now), 1))
    take_pre = margin_loss_pre.detach() < 10.0                            # tf.cond(tf.less(margin_loss_pre, 10.0), f1, f2), on the device
    margin_loss = torch.where(take_pre, margin_loss_pre, margin_loss_now)
    cross_entropy_loss = cross_entropy_loss * 0.0
    return dict(loss=_finish(cross_entropy_loss, margin_loss), pre=margin_loss_pre, relabelled=~take_pre, max_index=max_index[:, 0],
                labels=float_labels_now)


def loss_relabel(predictions, labels):
    return relabel_parts(predictions, labels)["loss"]


FUNCTIONS = {"loss_square": loss_square, "loss_sqrt": loss_sqrt, "loss_jsd": loss_jsd, "loss_mix": loss_mix, "loss_weight": loss_weight,
             "loss_margin": loss_margin, "loss_relabel": loss_relabel}


def restatement(kind, predictions, labels, jsd_pi=0.5):
    if kind == "loss_jsd":
        return loss_jsd(predictions, labels, jsd_pi)
    return FUNCTIONS[kind](predictions, labels)
