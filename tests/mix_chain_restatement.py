"""Restatement of Z's combine chain heads (MoeMix4Model, Z/video_level_models.py:1872-2044, the moe_group=False path; MoeKnowledgeModel,
:1331-1438; Z = youtube-8m-zhangteng of the reference), of the tail of LstmExtendCombineModel (Z/frame_level_models.py:5911-5924) from
the pooled rows on, of the stage step ops.mix_link stands for and of the mix loss (Z/losses.py:280-313, the default branch), in plain
torch, in the dtype of its inputs (float64 for the reference values, float32 for the error bound), in the reference's form and with its
variable names -- two products, a materialised 1 - probabilities:
    class_input_1 = slim.fully_connected(probabilities_by_vocab, class_size, activation_fn=tf.nn.elu, scope="class_inputs1-%s" % i)
    class_input_2 = slim.fully_connected(1 - probabilities_by_vocab, class_size, activation_fn=tf.nn.elu, scope="class_inputs2-%s" % i)
    class_input_k = tf.nn.l2_normalize(class_input_k, dim=1) * tf.sqrt(tf.cast(class_size, dtype=tf.float32) / shape)
    vocab_input = tf.concat((vocab_input, class_input_1, class_input_2), axis=1);  gates-i / experts-i as MoeModel
The scale is a float32 value (sqrt in float32 of the float32 quotient) and an input of the float64 run as it is of the float32 one.
tf.nn.elu is exp(x) - 1 below zero.  Shared by tests/test_mix_chain_host.py and tests/test_gpu_mix_chain.py; not a test module."""
import collections

import numpy as np
import torch

from ensemble_restatement import bound  # noqa: F401  (re-exported: the tests' bound)
from gate_lstm_restatement import cross_entropy, err, moe  # noqa: F401

HEADS = ("MoeMix4Model", "MoeKnowledgeModel")


def elu(x):
    return torch.where(x > 0, x, torch.exp(torch.clamp(x, max=0.0)) - 1)


def l2_normalize(x, eps=1e-12):
    """tf.nn.l2_normalize(x, dim=1): x * rsqrt(max(sum x^2, eps))."""
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim=1, keepdim=True), min=eps))


def link_scale(class_size, shape):
    """tf.sqrt(tf.cast(class_size, tf.float32) / shape) as a float32 value."""
    return np.sqrt(np.float32(class_size) / np.float32(shape), dtype=np.float32)


# ---- the stage step -------------------------------------------------------------------------------------------------------------------
def mix_link(vocab_input, x1, x2, W1, b1, W2, b2, scale=None):
    """[vocab_input | class_input_1 | class_input_2] from the two layers' inputs x1 (probabilities) and x2 (1 - probabilities, or
    probabilities . seq).  scale None: no normalisation (--frame_features)."""
    class_input_1 = elu(x1 @ W1 + b1)
    class_input_2 = elu(x2 @ W2 + b2)
    if scale is not None:
        s = torch.as_tensor(np.float32(scale)).to(x1.dtype)
        class_input_1 = l2_normalize(class_input_1) * s
        class_input_2 = l2_normalize(class_input_2) * s
    return torch.cat((vocab_input, class_input_1, class_input_2), dim=1)


def _t(a, dtype, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).clone().requires_grad_(grad)


def kernel_with_grads(prev, z, u, plain, scale, dy, dtype):
    """What csrc/mix_link.hip computes, from ITS operands (z [rows, 2 C] and u [2 C]), in the reference's form: the pre-activations are
    z1 + u1 and z2 + u2 (plain) or u2 - z2 (complement).  out, dprev, dz by autograd in `dtype` from float32 numpy operands."""
    pt, zt, ut = _t(prev, dtype, True), _t(z, dtype, True), _t(u, dtype)
    C = z.shape[1] // 2
    pre1 = zt[:, :C] + ut[:C]
    pre2 = zt[:, C:] + ut[C:] if plain else ut[C:] - zt[:, C:]
    c1, c2 = elu(pre1), elu(pre2)
    if scale is not None:
        s = torch.as_tensor(np.float32(scale)).to(dtype)
        c1, c2 = l2_normalize(c1) * s, l2_normalize(c2) * s
    out = torch.cat((pt, c1, c2), dim=1)
    out.backward(_t(dy, dtype))
    return {"out": out.detach(), "dprev": pt.grad, "dz": zt.grad}


def link_with_grads(prev, p, q, W1, b1, W2, b2, scale, dy, dtype):
    """ops.mix_link from p on, in the reference's form (1 - p materialised; q given: the MoeKnowledge form): out and the gradients of
    prev, p, q and the four parameters."""
    names = ("prev", "p", "W1", "b1", "W2", "b2") + (("q",) if q is not None else ())
    t = {k: _t(v, dtype, True) for k, v in zip(names, (prev, p, W1, b1, W2, b2) + ((q,) if q is not None else ()))}
    out = mix_link(t["prev"], t["p"], (1 - t["p"]) if q is None else t["q"], t["W1"], t["b1"], t["W2"], t["b2"], scale)
    out.backward(_t(dy, dtype))
    res = {"out": out.detach()}
    res.update({"d" + k: v.grad for k, v in t.items()})
    return res


# ---- the heads ------------------------------------------------------------------------------------------------------------------------
def variable_shapes(name, D, V, M, C, layers, K=None):
    """{variable name: shape} of head `name` in creation order.  K: the columns of --class_file (MoeKnowledgeModel)."""
    s = collections.OrderedDict([("gates/weights", (D, V * (M + 1))), ("experts/weights", (D, V * M)), ("experts/biases", (V * M,))])
    for i in range(layers):
        w = D + 2 * C * (i + 1)
        s["class_inputs1-%d/weights" % i] = (V, C)
        s["class_inputs1-%d/biases" % i] = (C,)
        s["class_inputs2-%d/weights" % i] = (K if name == "MoeKnowledgeModel" else V, C)
        s["class_inputs2-%d/biases" % i] = (C,)
        s["gates-%d/weights" % i] = (w, V * (M + 1))
        s["experts-%d/weights" % i] = (w, V * M)
        s["experts-%d/biases" % i] = (V * M,)
    return s


def head(name, model_input, P, M, C, layers, normalize=True, seq=None):
    """create_model of head `name`: (predictions [B, V], predictions_class [B, layers V])."""
    shape = model_input.shape[1]
    scale = link_scale(C, shape) if (normalize or name == "MoeKnowledgeModel") else None
    probabilities_by_class = moe(model_input, P["gates/weights"], P["experts/weights"], P["experts/biases"], M)
    probabilities_by_vocab = probabilities_by_class
    vocab_input = model_input
    for i in range(layers):
        x2 = probabilities_by_vocab @ seq if name == "MoeKnowledgeModel" else 1 - probabilities_by_vocab
        vocab_input = mix_link(vocab_input, probabilities_by_vocab, x2, P["class_inputs1-%d/weights" % i], P["class_inputs1-%d/biases" % i],
                               P["class_inputs2-%d/weights" % i], P["class_inputs2-%d/biases" % i], scale)
        probabilities_by_vocab = moe(vocab_input, P["gates-%d/weights" % i], P["experts-%d/weights" % i], P["experts-%d/biases" % i], M)
        if i < layers - 1:
            probabilities_by_class = torch.cat((probabilities_by_class, probabilities_by_vocab), dim=1)
    return probabilities_by_vocab, probabilities_by_class


def extend_combine_tail(rnn_pooled, P, M, C, layers, num_extend):
    """LstmExtendCombineModel from rnn_pooled [B E, H] on: MoeMix4Model without normalisation (the scripts say --frame_features), then
    tf.reduce_max over a video's E rows of both results."""
    final_probabilities, probabilities_by_class = head("MoeMix4Model", rnn_pooled, P, M, C, layers, normalize=False)
    V = final_probabilities.shape[1]
    return (final_probabilities.view(-1, num_extend, V).max(dim=1)[0],
            probabilities_by_class.view(-1, num_extend, V * layers).max(dim=1)[0])


def mix_loss(predictions, predictions_class, labels, layers):
    """calculate_loss_mix, the default branch: the labels side by side `layers` times."""
    float_labels = labels.to(predictions.dtype)
    float_classes = float_labels
    for _ in range(layers - 1):
        float_classes = torch.cat((float_classes, float_labels), dim=1)
    return cross_entropy(predictions, float_labels) + 0.1 * cross_entropy(predictions_class, float_classes)


def draw(shapes, rs):
    """Gaussian weights at 1 / sqrt(fan-in) -- logits of order 1 at every width -- and biases at 0.1, float32."""
    P = {}
    for k, shp in shapes.items():
        P[k] = (rs.randn(*shp) * (1.0 / np.sqrt(shp[0]) if len(shp) == 2 else 0.1)).astype(np.float32)
    return P


def to_torch(P, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in P.items()}


def reference(name, x, labels, P, M, C, layers, dtype, normalize=True, seq=None, num_extend=None):
    """The head on features x [B, D] (num_extend: LstmExtendCombineModel's tail on x [B E, H]) and the mix loss in `dtype` on the same
    float32 inputs: predictions, predictions_class, loss, the gradient of the loss for every variable and for x."""
    tp = to_torch(P, dtype)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    if num_extend:
        p, pc = extend_combine_tail(xt, tp, M, C, layers, num_extend)
    else:
        p, pc = head(name, xt, tp, M, C, layers, normalize, None if seq is None else torch.from_numpy(seq).to(dtype))
    loss = mix_loss(p, pc, torch.from_numpy(labels), max(layers, 1))
    loss.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in tp.items()}
    return {"predictions": p.detach(), "predictions_class": pc.detach(), "loss": loss.detach(), "grads": grads, "dx": xt.grad}
