"""Ensemble-level models on stacked predictions model_input [B, V, M] (M methods); class names, flags, scopes and variable names mirror
E/ensemble_level_models.py + E/all_ensemble_models/ (E = youtube-8m-ensemble of the reference).

Eight plugins end in ops.ens_combine -- the softmax over the methods of gated logit tables and the weighted sum, one fused pass over the
predictions each way (csrc/ensemble.hip) or its composed torch form -- plus tiny differentiable torch ops on [J, V, M]-sized or smaller
tensors (the rank-R product of ensemble_weightx and ensemble_weighty, broadcasts of the per-method weights) and the gate's fully-connected
layers through video_level_models.fully_connected.  Three more mix in ways that ens_combine cannot express (csrc/ensemble_tensor.hip):
MoeModel's weights come from the predictions themselves through a per-class [M, M] matrix (ops.ens_tensor_moe; it is NOT the video-level
MoE head), InputMoeModel and AttentionMoeModel mix with one softmax row per video (ops.ens_mix).  Variables enter the torch ops through
ops.as_tensor, which lands their gradient in the arena.  tf.get_variable without an initializer: variables.glorot_uniform.

Left out, with the reason:
  AttentionRectifiedLinearModel   cannot run in the reference: `rel_gated_weight` (attention_rectified_linear_model.py:44) is undefined
  DeepCombineChainModel (the ensemble copy)
                                  cannot run in the reference: its first slim.fully_connected(..., reuse=True, scope="transform")
                                  (deep_combine_chain_model.py:30-36) asks for variables that nothing has created yet, and the `new_relu`
                                  it computes from each prediction (:62-68) is never fed back (prev_relu stays mean_relu)
  LogisticModel (the ensemble copy)
                                  slim.fully_connected over the 3-D model_input [B, V, M] (logistic_model.py:24-26) contracts the method
                                  axis only and yields [B, V, V] "predictions": not a model of this stage
  EnsembleFrameReader, the model-selection scripts
                                  offline tooling around the readers
"""
import torch

from . import models, ops
from . import video_level_models as vlm
from .flags import FLAGS, DEFINE_integer
from .variables import get_default_graph, glorot_uniform, xavier_uniform, zeros

# E/ensemble_level_models.py:40-45 (moe_num_mixtures: video_level_models.py)
DEFINE_integer("attention_matrix_rank", 3, "The rank of weight matrix used for AttentionMatrixModel.")
DEFINE_integer("attention_relu_cells", 128, "The number of relu cells of AttentionMoeMatrixModel's gate inputs.")


def _var(name, shape, l2=0.0):
    """tf.get_variable(name, shape=..., regularizer=slim.l2_regularizer(l2)) as a tensor of the autograd tape."""
    return ops.as_tensor(get_default_graph().get_variable(name, tuple(shape), glorot_uniform, l2=l2))


def _attention_gate(model_input, original_input, num_mixtures, l2_penalty, sub_scope):
    """[B, J] softmax FC "gates" + sub_scope over [l2_normalize(original_input) | mean over the methods] (attention_matrix_model.py:28-38)."""
    if original_input is None:
        raise ValueError("the attention ensemble models need original_input (--input_data_pattern)")
    mean_output, _ = ops.ens_moments(model_input)
    gate_input = torch.cat([ops.l2norm_fwd(original_input.to(torch.float32)), mean_output], dim=1)
    return torch.softmax(vlm.fully_connected(gate_input, num_mixtures, "gates" + sub_scope, l2_penalty=l2_penalty), dim=-1)


def _whole_l2_normalize(x, eps=1e-12):
    """tf.nn.l2_normalize(x) as attention_moe_matrix_model.py:43-45 calls it, WITHOUT `dim`.  Under TF 1.0 `dim` is a required argument
    and the call raises; under the later 1.x releases that give it the default None, reduce_sum(square(x), None) sums over EVERY axis,
    the batch axis included: the whole [B, cells] activation is divided by one number, its Frobenius norm (at least sqrt(1e-12)).  That is
    what runs here; it is not a per-row normalisation."""
    return x * torch.rsqrt(torch.clamp((x * x).sum(), min=eps))


class MeanModel(models.BaseModel):
    """mean_model.py: the mean over the methods; no variables."""

    def create_model(self, model_input, **unused_params):
        return {"predictions": ops.ens_moments(model_input)[0]}


class LinearRegressionModel(models.BaseModel):
    """linear_regression_model.py: softmax(ensemble_weight [M]) over the methods, the same for every class."""

    def create_model(self, model_input, vocab_size, l2_penalty=1e-8, original_input=None, **unused_params):
        V, M = model_input.shape[1:]
        weight = _var("ensemble_weight", (M,), l2_penalty)
        return {"predictions": ops.ens_combine(model_input, weight.view(1, 1, M).expand(1, V, M))}


class MatrixRegressionModel(models.BaseModel):
    """matrix_regression_model.py: per class, softmax over the methods of ensemble_weight2d [V, M] * ensemble_weight1d [M]; the l2
    penalty of the matrix is 10 x that of the vector."""

    def create_model(self, model_input, vocab_size, l2_penalty=1e-8, original_input=None, **unused_params):
        V, M = model_input.shape[1:]
        weight1d = _var("ensemble_weight1d", (M,), l2_penalty)
        weight2d = _var("ensemble_weight2d", (V, M), 10 * l2_penalty)
        return {"predictions": ops.ens_combine(model_input, (weight2d * weight1d).unsqueeze(0))}


class NonunitMatrixRegressionModel(models.BaseModel):
    """nonunit_matrix_regression_model.py: sigmoid of the softmax(ensemble_weight [V, M])-weighted sum of the predictions' logits
    log((eps + x) / (1 + eps - x)); the input is behind a stop_gradient."""

    def create_model(self, model_input, vocab_size, l2_penalty=1e-8, original_input=None, epsilon=1e-5, **unused_params):
        if float(epsilon) != ops.ENS_LOGIT_EPS:
            raise ValueError("NonunitMatrixRegressionModel: epsilon is fixed at 1e-5")
        V, M = model_input.shape[1:]
        weight = _var("ensemble_weight", (V, M), l2_penalty)
        return {"predictions": torch.sigmoid(ops.ens_combine(model_input.detach(), weight.unsqueeze(0), xform="logit"))}


class AttentionLinearModel(models.BaseModel):
    """attention_linear_model.py: the gate mixes --moe_num_mixtures rows of ensemble_weight [J, M]; one softmax over the methods per
    video, the same for every class."""

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, sub_scope="", original_input=None,
                     **unused_params):
        V, M = model_input.shape[1:]
        J = FLAGS.moe_num_mixtures
        gate = _attention_gate(model_input, original_input, J, l2_penalty, sub_scope)
        weight_var = _var("ensemble_weight", (J, M), l2_penalty)
        return {"predictions": ops.ens_combine(model_input, weight_var.unsqueeze(1).expand(J, V, M), gate)}


class AttentionMatrixModel(models.BaseModel):
    """attention_matrix_model.py: J rank-R tables ensemble_weightx [J, V, R] . ensemble_weighty [J, R, M], mixed by the gate."""

    def _table(self, J, V, M, l2_penalty):
        R = FLAGS.attention_matrix_rank
        weight_x = _var("ensemble_weightx", (J, V, R), l2_penalty)
        weight_y = _var("ensemble_weighty", (J, R, M), l2_penalty)
        return torch.einsum("ijl,ilk->ijk", weight_x, weight_y)

    def _gate(self, model_input, original_input, J, l2_penalty, sub_scope):
        return _attention_gate(model_input, original_input, J, l2_penalty, sub_scope)

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, sub_scope="", original_input=None,
                     **unused_params):
        V, M = model_input.shape[1:]
        J = FLAGS.moe_num_mixtures
        gate = self._gate(model_input, original_input, J, l2_penalty, sub_scope)
        return {"predictions": ops.ens_combine(model_input, self._table(J, V, M, l2_penalty), gate)}


class AttentionLinmatrixModel(AttentionMatrixModel):
    """attention_linmatrix_model.py: AttentionMatrixModel's tables plus ensemble_weight [J, 1, M] and ensemble_bias [J, 1, 1].  The bias
    adds, per video and class, the same number sum_j gate[b, j] b[j] to every method's logit: the softmax over the methods ignores it and
    its gradient is exactly zero.  The variable exists (checkpoints carry it) and is left out of the arithmetic."""

    def _table(self, J, V, M, l2_penalty):
        get_default_graph().get_variable("ensemble_bias", (J, 1, 1), glorot_uniform)
        weight_var = _var("ensemble_weight", (J, 1, M), l2_penalty)
        return super(AttentionLinmatrixModel, self)._table(J, V, M, l2_penalty) + weight_var


class AttentionMoeMatrixModel(AttentionMatrixModel):
    """attention_moe_matrix_model.py: AttentionMatrixModel with the gate computed from three relu layers of --attention_relu_cells --
    "relu-origin" over original_input as it is, "relu-mean" over the mean and "relu-std" over the unbiased variance of the methods --
    each normalised as the reference writes it (_whole_l2_normalize)."""

    def relu(self, model_input, relu_cells, l2_penalty=1e-8, sub_scope=""):
        return vlm.fully_connected(model_input, relu_cells, "relu-" + sub_scope, activation="relu", l2_penalty=l2_penalty)

    def _gate(self, model_input, original_input, J, l2_penalty, sub_scope):
        if original_input is None:
            raise ValueError("the attention ensemble models need original_input (--input_data_pattern)")
        num_relu = FLAGS.attention_relu_cells
        mean_input, std_input = ops.ens_moments(model_input, variance=True)
        relus = [_whole_l2_normalize(self.relu(t, num_relu, sub_scope=s))
                 for t, s in ((original_input.to(torch.float32), "origin"), (mean_input, "mean"), (std_input, "std"))]
        return torch.softmax(vlm.fully_connected(torch.cat(relus, dim=1), J, "gates" + sub_scope, l2_penalty=l2_penalty), dim=-1)


class MoeModel(models.BaseModel):
    """moe_model.py (the ensemble's own, not video_level_models.MoeModel): per class a matrix tensor_weight [V, M, M] and a bias
    tensor_bias [V, M] turn the M predictions of a (video, class) into M logits; their softmax mixes the same M predictions."""

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, sub_scope="", original_input=None,
                     **unused_params):
        V, M = model_input.shape[1:]
        tensor_weight = _var("tensor_weight", (V, M, M), l2_penalty)
        tensor_bias = ops.as_tensor(get_default_graph().get_variable("tensor_bias", (V, M), zeros, l2=l2_penalty))
        return {"predictions": ops.ens_tensor_moe(model_input, tensor_weight, tensor_bias)}


class InputMoeModel(models.BaseModel):
    """input_moe_model.py: one softmax row over the methods per video, FC "gates" over l2_normalize(original_input)."""

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, sub_scope="", original_input=None,
                     **unused_params):
        if original_input is None:
            raise ValueError("InputMoeModel needs original_input (--input_data_pattern)")
        M = model_input.shape[2]
        gate_input = ops.l2norm_fwd(original_input.to(torch.float32))
        gate_activations = torch.softmax(vlm.fully_connected(gate_input, M, "gates" + sub_scope, l2_penalty=l2_penalty), dim=-1)
        return {"predictions": ops.ens_mix(model_input, gate_activations)}


class AttentionMoeModel(models.BaseModel):
    """attention_moe_model.py: --attention_relu_cells relu cells over l2_normalize(original_input) ("relu-input") and over each method's
    predictions ("relu-sub<i>": method i's plane of the method-major buffer, no copy; the M layers are one grouped launch per direction
    and the planes, being data, get no gradient); "gate", an FC without bias over the (M + 1) cells, and its softmax mix the methods per
    video."""

    def relu(self, model_input, relu_cells, l2_penalty=1e-8, sub_scope=""):
        return vlm.fully_connected(model_input, relu_cells, "relu-" + sub_scope, activation="relu", l2_penalty=l2_penalty)

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, sub_scope="", original_input=None,
                     **unused_params):
        if original_input is None:
            raise ValueError("AttentionMoeModel needs original_input (--input_data_pattern)")
        g = get_default_graph()
        num_relu = FLAGS.attention_relu_cells
        V, M = model_input.shape[1:]
        relu_input = self.relu(ops.l2norm_fwd(original_input.to(torch.float32)), num_relu, sub_scope="input")
        spec = []
        for i in range(M):
            scope = "relu-sub%d" % i
            spec.append((g.get_variable(scope + "/weights", (V, num_relu), xavier_uniform, l2=1e-8), None,
                         g.get_variable(scope + "/biases", (num_relu,), zeros)))
        subs = ops.linear_group([model_input[:, :, i] for i in range(M)], spec)
        relu_units = torch.cat([relu_input, ops.activation(torch.cat(subs, dim=1), "relu")], dim=1)
        gate = torch.softmax(vlm.fully_connected(relu_units, M, "gate", use_bias=False, l2_penalty=l2_penalty), dim=-1)
        return {"predictions": ops.ens_mix(model_input, gate)}
