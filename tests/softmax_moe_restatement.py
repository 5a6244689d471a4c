"""Restatement of Z's MoeSoftmaxModel (Z/video_level_models.py:877-1017; Z = youtube-8m-zhangteng of the reference), of its SoftmaxLoss
(Z/losses.py:412-456, here losses.SplitSoftmaxLoss) and of that loss's calculate_loss_mix, in plain torch, in the dtype of its inputs
(float64 for the reference values, float32 for the error bound), line for line and with the reference's variable names:
    gating_distribution = tf.nn.softmax(tf.reshape(gate_activations, [-1, num_mixtures + 1]))
    expert_distribution = tf.nn.softmax(tf.reshape(expert_activations, [-1, sub_vocab_size, num_mixtures]), dim=1)
    probabilities_by_subvocab = tf.reduce_sum(gating_distribution[:, :num_mixtures] * expert_distribution, 1), reshaped [-1, sub_vocab_size]
    probabilities_by_subvocab = probabilities_by_subvocab / tf.reduce_sum(probabilities_by_subvocab, axis=1, keep_dims=True)
    probabilities_by_softmax = probabilities_by_subvocab[:, :-1]
The reference's `channels` is the constant 1: its loop runs once.  The loss is the reference's own, WITHOUT the clamp of the appended
probability that the product adds (clamp=True restates the product's rule): the GPU tests choose inputs whose appended probability is
at least 0.05 and assert that the unclamped float32 restatement is finite.  Shared by tests/test_softmax_moe_host.py and
tests/test_gpu_softmax_moe.py; not a test module."""
import collections

import numpy as np
import torch

from ensemble_restatement import bound  # noqa: F401  (re-exported: the tests' bound)
from gate_lstm_restatement import cross_entropy, err, moe  # noqa: F401
from mix_chain_restatement import draw, elu, l2_normalize, link_scale, to_torch  # noqa: F401

NAME = "MoeSoftmaxModel"
EPSILON = 10e-8


# ---- the softmax part of sub_model -----------------------------------------------------------------------------------------------------
def softmax_part(gate_activations, expert_activations, sub_vocab_size, num_mixtures):
    """probabilities_by_softmax [B, sub_vocab_size - 1] from the two fully-connected outputs."""
    gating_distribution = torch.softmax(gate_activations.reshape(-1, num_mixtures + 1), dim=1)
    expert_distribution = torch.softmax(expert_activations.reshape(-1, sub_vocab_size, num_mixtures), dim=1)
    expert_distribution = expert_distribution.reshape(-1, num_mixtures)
    probabilities_by_subvocab = (gating_distribution[:, :num_mixtures] * expert_distribution).sum(1)
    probabilities_by_subvocab = probabilities_by_subvocab.reshape(-1, sub_vocab_size)
    probabilities_by_subvocab = probabilities_by_subvocab / probabilities_by_subvocab.sum(dim=1, keepdim=True)
    return probabilities_by_subvocab[:, :-1]


def _t(a, dtype, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).clone().requires_grad_(grad)


def kernel_with_grads(Zg, Ze, head, S, M, dout, dtype):
    """What csrc/softmax_moe.hip computes, from ITS operands, in the reference's form: out = [head | probabilities_by_softmax], and dZg,
    dZe, dhead by autograd in `dtype` from float32 numpy operands; the per-row statistics the kernel keeps beside them."""
    zg, ze = _t(Zg, dtype, True), _t(Ze, dtype, True)
    h = None if head is None else _t(head, dtype, True)
    q = softmax_part(zg, ze, S, M)
    out = q if h is None else torch.cat((h, q), dim=1)
    out.backward(_t(dout, dtype))
    z3 = ze.detach().reshape(-1, S, M)
    mx = z3.max(dim=1)[0]
    sums = torch.exp(z3 - mx[:, None, :]).sum(dim=1)
    g = torch.softmax(zg.detach().reshape(-1, S, M + 1), dim=2)
    T = (g[:, :, :M] * torch.softmax(z3, dim=1)).sum(dim=(1, 2))
    res = {"out": out.detach(), "dZg": zg.grad, "dZe": ze.grad, "stats": torch.cat((mx, sums, T[:, None]), dim=1)}
    if h is not None:
        res["dhead"] = h.grad
    return res


# ---- the loss ----------------------------------------------------------------------------------------------------------------------------
def softmax_loss(predictions, labels, bound_, clamp=False):
    """SoftmaxLoss.calculate_loss with vocab_size_1 = bound_.  clamp: the product's rule for predictions_append, max(., 0) with the
    gradient of the unclamped value."""
    epsilon = EPSILON
    vocab_size_1 = bound_
    float_labels = labels.to(predictions.dtype)
    labels_1 = float_labels[:, :vocab_size_1]
    predictions_1 = predictions[:, :vocab_size_1]
    cross_entropy_loss = cross_entropy(predictions_1, labels_1)
    lables_2 = float_labels[:, vocab_size_1:]
    predictions_2 = predictions[:, vocab_size_1:]
    label_rowsum = torch.clamp(lables_2.sum(1, keepdim=True), min=epsilon)
    label_append = 1.0 - lables_2.max(1, keepdim=True)[0]
    norm_float_labels = torch.cat((lables_2 / label_rowsum, label_append), dim=1)
    predictions_append = 1.0 - predictions_2.sum(1, keepdim=True)
    if clamp:
        predictions_append = predictions_append + (torch.clamp(predictions_append, min=0.0) - predictions_append).detach()
    softmax_outputs = torch.cat((predictions_2, predictions_append), dim=1)
    softmax_loss_ = norm_float_labels * torch.log(softmax_outputs + epsilon) + (1 - norm_float_labels) * torch.log(1 - softmax_outputs + epsilon)
    softmax_loss_ = -softmax_loss_.sum(1)
    return softmax_loss_.mean() + cross_entropy_loss


def softmax_loss_mix(predictions, predictions_class, labels, bound_, moe_layers, clamp=False):
    """SoftmaxLoss.calculate_loss_mix."""
    vocab_size = labels.shape[1]
    cross_entropy_class = 0.0
    for i in range(moe_layers):
        predictions_subclass = predictions_class[:, i * vocab_size:(i + 1) * vocab_size]
        cross_entropy_class = cross_entropy_class + softmax_loss(predictions_subclass, labels, bound_, clamp)
    cross_entropy_loss = softmax_loss(predictions, labels, bound_, clamp)
    return cross_entropy_loss + 0.1 * cross_entropy_class


def mix_loss(predictions, predictions_class, labels, layers):
    """Z's CrossEntropyLoss.calculate_loss_mix, the default branch (the reference's script trains MoeSoftmaxModel with it): the labels
    side by side `layers` times; a --moe_layers=0 result holds its one prediction under both keys."""
    float_labels = labels.to(predictions.dtype)
    return cross_entropy(predictions, float_labels) + 0.1 * cross_entropy(predictions_class, float_labels.repeat(1, max(layers, 1)))


def loss_with_grads(p, labels, bound_, dtype, clamp=False, scale=1.0):
    pt = _t(p, dtype, True)
    y = torch.from_numpy(np.ascontiguousarray(labels))
    loss = softmax_loss(pt, y, bound_, clamp) * scale
    loss.backward()
    return {"loss": loss.detach(), "dp": pt.grad}


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def block_shapes(name, d_in, V, V1, M):
    """sub_model(name=...)'s six Variables in creation order."""
    S = V - V1 + 1
    return collections.OrderedDict([
        ("gates%s/weights" % name, (d_in, V1 * (M + 1))), ("experts%s/weights" % name, (d_in, V1 * M)), ("experts%s/biases" % name, (V1 * M,)),
        ("class_gates-0%s/weights" % name, (d_in, S * (M + 1))), ("class_experts-0%s/weights" % name, (d_in, S * M)),
        ("class_experts-0%s/biases" % name, (S * M,))])


def variable_shapes(D, V, V1, M, C, layers):
    """{variable name: shape} of MoeSoftmaxModel in creation order."""
    s = block_shapes("pre", D, V, V1, M)
    for i in range(layers):
        s["class_inputs1-%d/weights" % i] = (V, C)
        s["class_inputs1-%d/biases" % i] = (C,)
        s["class_inputs2-%d/weights" % i] = (V, C)
        s["class_inputs2-%d/biases" % i] = (C,)
        s.update(block_shapes("-%d" % i, D + 2 * C * (i + 1), V, V1, M))
    return s


def sub_model(model_input, vocab_size, P, num_mixtures, bound_, name):
    vocab_size_1 = bound_
    probabilities_by_sigmoid = moe(model_input, P["gates%s/weights" % name], P["experts%s/weights" % name], P["experts%s/biases" % name],
                                   num_mixtures)
    vocab_size_2 = vocab_size - bound_
    sub_vocab_size = vocab_size_2 + 1
    gate_activations = model_input @ P["class_gates-0%s/weights" % name]
    expert_activations = model_input @ P["class_experts-0%s/weights" % name] + P["class_experts-0%s/biases" % name]
    probabilities_by_softmax = softmax_part(gate_activations, expert_activations, sub_vocab_size, num_mixtures)
    assert probabilities_by_sigmoid.shape[1] == vocab_size_1
    return torch.cat((probabilities_by_sigmoid, probabilities_by_softmax), dim=1)


def create_model(model_input, vocab_size, P, num_mixtures, class_size, moe_layers, bound_):
    """(predictions [B, V], predictions_class [B, max(moe_layers, 1) V])."""
    shape = model_input.shape[1]
    scale = torch.as_tensor(link_scale(class_size, shape)).to(model_input.dtype)
    probabilities_by_class = sub_model(model_input, vocab_size, P, num_mixtures, bound_, "pre")
    probabilities_by_vocab = probabilities_by_class
    vocab_input = model_input
    for i in range(moe_layers):
        class_input_1 = elu(probabilities_by_vocab @ P["class_inputs1-%d/weights" % i] + P["class_inputs1-%d/biases" % i])
        class_input_2 = elu((1 - probabilities_by_vocab) @ P["class_inputs2-%d/weights" % i] + P["class_inputs2-%d/biases" % i])
        class_input_1 = l2_normalize(class_input_1) * scale
        class_input_2 = l2_normalize(class_input_2) * scale
        vocab_input = torch.cat((vocab_input, class_input_1, class_input_2), dim=1)
        probabilities_by_vocab = sub_model(vocab_input, vocab_size, P, num_mixtures, bound_, "-%d" % i)
        if i < moe_layers - 1:
            probabilities_by_class = torch.cat((probabilities_by_class, probabilities_by_vocab), dim=1)
    return probabilities_by_vocab, probabilities_by_class


def reference(x, labels, P, M, C, layers, bound_, dtype, loss="CrossEntropyLoss", clamp=False):
    """The model on features x [B, D] and its training loss in `dtype` on the same float32 inputs: predictions, predictions_class, loss,
    the gradient of the loss for every variable and for x.  loss: "CrossEntropyLoss" (the mix rule) or "SplitSoftmaxLoss"
    (calculate_loss_mix)."""
    tp = to_torch(P, dtype)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    p, pc = create_model(xt, labels.shape[1], tp, M, C, layers, bound_)
    y = torch.from_numpy(labels)
    value = mix_loss(p, pc, y, layers) if loss == "CrossEntropyLoss" else softmax_loss_mix(p, pc, y, bound_, layers, clamp)
    value.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in tp.items()}
    return {"predictions": p.detach(), "predictions_class": pc.detach(), "loss": value.detach(), "grads": grads, "dx": xt.grad}
