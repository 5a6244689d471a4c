"""Restatement of Z's cascade heads (Z/video_level_models.py:286-582, Z = youtube-8m-zhangteng of the reference) and of the two ops they
are built from, in plain torch, in the dtype of its inputs (float64 for the reference values, float32 for the error bound), in the
reference's form and with its variable names:
    class_input = slim.fully_connected(distill_labels, 256, relu or None, scope="class_inputs")
    class_input = class_input / tf.reduce_sum(distill_labels, axis=1, keep_dims=True);  class_input = tf.nn.l2_normalize(class_input, dim=1)
    model_input = tf.concat((model_input, class_input), axis=1);  gates / experts as MoeModel
    final_probabilities = final_probabilities * FLAGS.ensemble_w + distill_labels * (1.0 - FLAGS.ensemble_w)
One deliberate difference from the reference, the project's zero-sum rule: a row of distill_labels that sums to exactly 0 is 0 / 0 = NaN
in the reference's Norm heads; here its class part is zeros and its pre-activation gets a zero gradient.  ensemble_w is a float32 value
and 1 - ensemble_w is formed in float32 from it: both are inputs of the float64 run as they are of the float32 one.  Shared by tests/test_distill_head_host.py and
tests/test_gpu_distill_head.py; not a test module."""
import collections

import numpy as np
import torch

from ensemble_restatement import bound  # noqa: F401  (re-exported: the tests' bound)
from gate_lstm_restatement import NAMES as GATE_NAMES, cross_entropy, err, moe, rnn_gate, shapes as gate_shapes  # noqa: F401

CLASS_SIZE = 256
HEADS = ("MoeDistillChainModel", "MoeDistillChainNormModel", "MoeDistillChainNorm2Model", "MoeDistillSplitModel")
# head -> the mode of ops.distill_input; mode -> (l2-normalise x, relu, divide by the row sum, l2-normalise the class part)
MODE_OF = {"MoeDistillChainModel": "chain", "MoeDistillChainNormModel": "norm", "MoeDistillChainNorm2Model": "norm2",
           "MoeDistillSplitModel": "split"}
MODES = {"chain": (False, True, False, False), "norm": (True, False, True, True), "norm2": (True, True, True, True),
         "split": (False, True, False, False)}


def l2_normalize(x, eps=1e-12):
    """tf.nn.l2_normalize(x, dim=1): x * rsqrt(max(sum x^2, eps))."""
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim=1, keepdim=True), min=eps))


# ---- the ops --------------------------------------------------------------------------------------------------------------------------
def distill_input(x, z, t, mode, v0=0):
    """[x' | class part] from the head's input x [B,D], the class_inputs layer's pre-activation z [B,C] and the teacher's t [B,V]."""
    norm_x, relu, div, norm_c = MODES[mode]
    class_input = torch.relu(z) if relu else z
    if div:
        s = t[:, v0:].sum(dim=1, keepdim=True)
        live = s != 0                                                     # the zero-sum rule
        class_input = torch.where(live, class_input / torch.where(live, s, torch.ones_like(s)), torch.zeros_like(class_input))
    if norm_c:
        class_input = l2_normalize(class_input)
    model_input = l2_normalize(x) if norm_x else x
    return torch.cat((model_input, class_input), dim=1)


def distill_blend(p1, t, w, v1):
    """concat(p1, t[:, v1:]) * w + t * (1 - w); w: a float32 value (python float or 0-d tensor)."""
    w32 = torch.as_tensor(w, dtype=torch.float32)
    final_probabilities = torch.cat((p1, t[:, v1:]), dim=1)
    return final_probabilities * w32.to(p1.dtype) + t * (1.0 - w32).to(p1.dtype)


def _t(a, dtype, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).clone().requires_grad_(grad)


def distill_input_with_grads(x, z, t, mode, v0, dy, dtype):
    """y, dx, dz by autograd in `dtype` from float32 numpy operands."""
    xt, zt = _t(x, dtype, True), _t(z, dtype, True)
    y = distill_input(xt, zt, _t(t, dtype), mode, v0)
    y.backward(_t(dy, dtype))
    return {"y": y.detach(), "dx": xt.grad, "dz": zt.grad}


def distill_blend_with_grads(p1, t, w, dout, dtype):
    pt = _t(p1, dtype, True)
    out = distill_blend(pt, _t(t, dtype), np.float32(w), p1.shape[1])
    out.backward(_t(dout, dtype))
    return {"out": out.detach(), "dp1": pt.grad}


# ---- the heads ------------------------------------------------------------------------------------------------------------------------
def split_bound(name, V, softmax_bound):
    return softmax_bound if name == "MoeDistillSplitModel" else V


def variable_shapes(name, D, V, M, softmax_bound=1000):
    """{variable name: shape} of head `name` in creation order: slim.fully_connected under "class_inputs", then gates and experts."""
    v1 = split_bound(name, V, softmax_bound)
    v_t = V - v1 if name == "MoeDistillSplitModel" else V
    return collections.OrderedDict([("class_inputs/weights", (v_t, CLASS_SIZE)), ("class_inputs/biases", (CLASS_SIZE,)),
                                    ("gates/weights", (D + CLASS_SIZE, v1 * (M + 1))), ("experts/weights", (D + CLASS_SIZE, v1 * M)),
                                    ("experts/biases", (v1 * M,))])


def head(name, model_input, distill_labels, P, M, ensemble_w=1.0, softmax_bound=1000):
    """create_model of head `name`: predictions [B, V]."""
    V = distill_labels.shape[1]
    vocab_size_1 = split_bound(name, V, softmax_bound)
    v0 = vocab_size_1 if name == "MoeDistillSplitModel" else 0
    z = distill_labels[:, v0:] @ P["class_inputs/weights"] + P["class_inputs/biases"]
    model_input = distill_input(model_input, z, distill_labels, MODE_OF[name], v0)
    p1 = moe(model_input, P["gates/weights"], P["experts/weights"], P["experts/biases"], M)
    return distill_blend(p1, distill_labels, ensemble_w, vocab_size_1)


def draw(shapes, rs):
    """Gaussian weights at 1 / sqrt(fan-in) -- logits of order 1 at every width, so that the gates and the relu leave their linear
    range without saturating -- and biases at 0.1, float32."""
    P = {}
    for k, shp in shapes.items():
        P[k] = (rs.randn(*shp) * (1.0 / np.sqrt(shp[0]) if len(shp) == 2 else 0.1)).astype(np.float32)
    return P


def to_torch(P, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in P.items()}


def reference(name, x, t, labels, P, M, dtype, ensemble_w=1.0, softmax_bound=1000):
    """The head on features x [B,D] and CrossEntropyLoss in `dtype` on the same float32 inputs: predictions, loss, the gradient of the
    loss for every variable and for x."""
    tp = to_torch(P, dtype)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    p = head(name, xt, torch.from_numpy(t).to(dtype), tp, M, np.float32(ensemble_w), softmax_bound)
    loss = cross_entropy(p, torch.from_numpy(labels))
    loss.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in tp.items()}
    return {"predictions": p.detach(), "loss": loss.detach(), "grads": grads, "dx": xt.grad}


def gate_reference(name, x64, nf, t, labels, P, M, dtype, ensemble_w=1.0, softmax_bound=1000):
    """LstmGateModel (one scalar-gate layer under "lstm_forward") with head `name` behind it, on the frames' float meaning x64 [B,F,D]."""
    tp = to_torch(P, dtype)
    state, _ = rnn_gate(torch.from_numpy(x64).to(dtype), torch.from_numpy(nf), {n: tp["lstm_forward/" + n] for n in GATE_NAMES})
    p = head(name, state, torch.from_numpy(t).to(dtype), tp, M, np.float32(ensemble_w), softmax_bound)
    loss = cross_entropy(p, torch.from_numpy(labels))
    loss.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in tp.items()}
    return {"predictions": p.detach(), "loss": loss.detach(), "grads": grads}
