"""Video-level classifier heads on [B, D_in] features; class names, flags and TF variable names mirror
W/video_level_models.py + W/all_video_models/ (W = /root/reference/youtube-8m-wangheda).

create_model(model_input, vocab_size, **kw) -> {"predictions": [B, V] probabilities, ...}; tensors are
torch tensors on the MI355X and all arithmetic runs in libyt8m_hip.so (ops.py).
"""
import torch

from . import models, ops
from .flags import FLAGS, DEFINE_integer, DEFINE_string, DEFINE_bool, DEFINE_float
from .variables import get_default_graph, xavier_uniform, zeros

# W/video_level_models.py:19-47
DEFINE_integer("moe_num_mixtures", 2, "The number of mixtures (excluding the dummy 'expert') used for MoeModel.")
DEFINE_integer("deep_chain_layers", 3, "The number of layers used for DeepChainModel")
DEFINE_integer("deep_chain_relu_cells", 200, "The number of relu cells used for DeepChainModel")
DEFINE_string("deep_chain_relu_type", "relu", "The type of relu cells used for DeepChainModel (options are elu and relu)")
DEFINE_bool("deep_chain_use_length", False, "unused by DeepCombineChainModel (kept for flag compatibility)")
DEFINE_integer("moe_num_extend", 8, "The number of attention outputs, used for MoeExtendModel.")      # Z/video_level_models.py:31
DEFINE_float("ensemble_w", 1.0, "ensemble weight used in distill chain models.")                        # Z/video_level_models.py:52-58
DEFINE_integer("softmax_bound", 1000, "The number of labels to be a group, used for MoeSoftmaxModel and MoeDistillSplitModel.")
DEFINE_integer("moe_layers", 1, "The number of combine layers, used for combine related models.")      # Z/video_level_models.py:36-56
DEFINE_integer("class_size", 200, "The dimention of prediction projection, used for all chain models.")
DEFINE_bool("moe_group", False, "Whether to split the 4716 labels into different groups, used in MoeMix4Model (not built here)")
DEFINE_string("class_file", "./resources/labels_knowledge.out", "The label-to-class matrix [V, K] that MoeKnowledgeModel reads (np.loadtxt).")
# new: MoeModel may return its own "loss" (W/train.py:384-385 honours it) computed by the fused mixing+cross-entropy pass
DEFINE_bool("fused_head_loss", True, "MoeModel returns {'loss': CrossEntropyLoss(predictions, labels)} from a fused kernel "
            "when labels are given, --label_loss=CrossEntropyLoss, no label smoothing and no --multitask.")


def fully_connected(x, num_outputs, scope, activation=None, use_bias=True, l2_penalty=0.0):
    """slim.fully_connected: variables <scope>/weights [in, out] (xavier) and <scope>/biases (zeros)."""
    g = get_default_graph()
    W = g.get_variable(scope + "/weights", (x.shape[-1], num_outputs), xavier_uniform, l2=l2_penalty)
    b = g.get_variable(scope + "/biases", (num_outputs,), zeros) if use_bias else None
    y = ops.linear(x, W, b)
    return ops.activation(y, activation) if activation else y


def fully_connected_cat(parts, num_outputs, scope, activation=None, use_bias=True, l2_penalty=0.0, group_parts=()):
    """slim.fully_connected(tf.concat(parts + tiled group_parts, axis=-1), ...) without materialising the concatenation
    (same variables): group_parts are per-video vectors [B, K] that the reference tiles over the frame axis."""
    g = get_default_graph()
    width = sum(p.shape[-1] for p in parts) + sum(p.shape[-1] for p in group_parts)
    W = g.get_variable(scope + "/weights", (width, num_outputs), xavier_uniform, l2=l2_penalty)
    b = g.get_variable(scope + "/biases", (num_outputs,), zeros) if use_bias else None
    y = ops.linear_cat(list(parts), W, b, group_parts=tuple(group_parts))
    return ops.activation(y, activation) if activation else y


def moe_block(model_input, vocab_size, num_mixtures, l2_penalty, gate_scope, expert_scope, frozen_cols=0):
    """The MoE block shared by MoeModel, the chain models' sub_model and the attention model's sub_moe
    (W/all_video_models/moe_model.py:40-64).  Gate FC has no bias; column l*(M+1)+m = gate m of label l.
    frozen_cols: the leading columns of model_input that are data (ops.moe_head dx_from)."""
    g = get_default_graph()
    d_in = model_input.shape[-1]
    M = num_mixtures
    Wg = g.get_variable(gate_scope + "/weights", (d_in, vocab_size * (M + 1)), xavier_uniform, l2=l2_penalty)
    We = g.get_variable(expert_scope + "/weights", (d_in, vocab_size * M), xavier_uniform, l2=l2_penalty)
    be = g.get_variable(expert_scope + "/biases", (vocab_size * M,), zeros)
    p = ops.moe_head(model_input.reshape(-1, d_in), Wg, We, be, vocab_size, M, bf16=FLAGS.compute_dtype == "bfloat16", dx_from=frozen_cols)
    return p.view(-1, vocab_size)


def moe_scopes(sub_scope, hyphen=True):
    """(gate scope, expert scope): gates-<s> / experts-<s> for the stages of the chain and attention plugins, gates<s> / experts<s> for
    MoeModel and MultiscaleCnnLstmModel."""
    return ("gates-" + sub_scope, "experts-" + sub_scope) if hyphen else ("gates" + sub_scope, "experts" + sub_scope)


def moe_stage(model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, sub_scope="", dropout=False, keep_prob=None, frozen_cols=0,
              hyphen=True, **unused_params):
    """One MoE stage of a chain, attention or multiscale plugin: what the reference's sub_model / sub_moe / moe methods all are.  With
    `dropout`, tf.nn.dropout on the stage's whole input first (deep_combine_chain_model.py:57-58)."""
    if dropout:
        model_input = ops.dropout(model_input, 1.0 if keep_prob is None else keep_prob)
    return moe_block(model_input, vocab_size, num_mixtures or FLAGS.moe_num_mixtures, l2_penalty, *moe_scopes(sub_scope, hyphen),
                     frozen_cols=frozen_cols)


def composed_link(kind="relu", noise_level=None):
    """The link form activation -> [add_noise] -> l2_normalize as separate ops: a noise_level that is not None, 0.0 included, runs
    ops.add_noise and takes a seed."""
    def link(z):
        y = ops.activation(z, kind)
        if noise_level is not None:
            y = ops.add_noise(y, noise_level)
        return ops.l2_normalize(y)
    return link


def fused_link(kind="relu", noise_level=None):
    """The same link as one ops.chain_link: no noise and no seed for a noise_level of None or 0."""
    return lambda z: ops.chain_link(z, kind, noise_level)


def relu_kind():
    """--deep_chain_relu_type as the chain plugins read it: "elu", anything else is relu."""
    return "elu" if FLAGS.deep_chain_relu_type == "elu" else "relu"


def relu_link(x, relu_cells, scope, l2_penalty, link):
    """link(FC(x)) [B, relu_cells] under `scope`: mean-relu, distillrelu."""
    return link(fully_connected(x, relu_cells, scope, l2_penalty=l2_penalty))


def distill_link(distillation_predictions, relu_cells, l2_penalty, scope="distillrelu", link=None):
    """The link (fused_link("relu") unless given) over another model's predictions, [B, relu_cells] under `scope`: what the Distillchain
    plugins concatenate into their classifiers' inputs."""
    assert distillation_predictions is not None, "distillation feature must be used"
    return relu_link(distillation_predictions.to(torch.float32), relu_cells, scope, l2_penalty, link or fused_link("relu"))


def prediction_chain(sub_model, stage_input, link, links, vocab_size, l2_penalty=1e-8, sub_scope="", support_kwargs=None,
                     frozen_cols=lambda k: 0, support_pool=None):
    """The prediction chain of every chain plugin (W/all_video_models/deep_combine_chain_model.py:38-55 and its frame-level kin;
    DESIGN_LOG.md section 25).  Stage l: sub_model on the stage's input under "prediction-<l>" (gates-, experts- variables; support_kwargs,
    such as dropout, go to these stages only, never to "-main"), FC to --deep_chain_relu_cells under "relu-<l>", link(...) appended to
    `links`, THEN stage_input(l + 1, links) -- which may create the next stage's cnn / lstm variables -- and last the stage's entry of
    "support_predictions" (support_pool applied first where given).  The order of these calls is the order of the variables in the arena
    and of the graph's random keys: tests/test_chain_order_host.py pins it per plugin.
    stage_input(k, links) -> [B, width_k], called once per k in rising order; frozen_cols(k): the leading data columns of stage k's
    input; no "support_predictions" key without support stages."""
    num_layers, relu_cells = FLAGS.deep_chain_layers, FLAGS.deep_chain_relu_cells
    support_predictions = []
    next_input = stage_input(0, links)
    for layer in range(num_layers):
        sub_prediction = sub_model(next_input, vocab_size, sub_scope=sub_scope + "prediction-%d" % layer, frozen_cols=frozen_cols(layer),
                                   **(support_kwargs or {}))
        sub_activation = fully_connected(sub_prediction, relu_cells, sub_scope + "relu-%d" % layer, l2_penalty=l2_penalty)
        links.append(link(sub_activation))
        next_input = stage_input(layer + 1, links)
        support_predictions.append(sub_prediction if support_pool is None else support_pool(sub_prediction))
    res = {"predictions": sub_model(next_input, vocab_size, sub_scope=sub_scope + "-main", frozen_cols=frozen_cols(num_layers))}
    if support_predictions:
        res["support_predictions"] = torch.cat(support_predictions, dim=1)
    return res


class LogisticModel(models.BaseModel):
    """W/all_video_models/logistic_model.py:9-26: sigmoid(x.W + b), L2 1e-8 on W; scope "fully_connected"."""

    def create_model(self, model_input, vocab_size, l2_penalty=1e-8, original_input=None, **unused_params):
        output = fully_connected(model_input, vocab_size, "fully_connected", activation="sigmoid", l2_penalty=l2_penalty)
        return {"predictions": output}


class MoeModel(models.BaseModel):
    """W/all_video_models/moe_model.py:9-65: per-class softmax over (num_mixtures + 1) logistic experts."""

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, sub_scope="",
                     original_input=None, labels=None, fuse_loss=True, **unused_params):
        num_mixtures = num_mixtures or FLAGS.moe_num_mixtures
        fused = (labels is not None and fuse_loss and FLAGS.fused_head_loss and FLAGS.label_loss == "CrossEntropyLoss"
                 and not FLAGS.label_smoothing and not FLAGS.multitask and torch.is_grad_enabled()
                 and model_input.dim() == 2 and tuple(labels.shape) == (model_input.shape[0], vocab_size))
        gate_scope, expert_scope = moe_scopes(sub_scope, hyphen=False)
        if fused:
            g = get_default_graph()
            d_in, M = model_input.shape[-1], num_mixtures
            Wg = g.get_variable(gate_scope + "/weights", (d_in, vocab_size * (M + 1)), xavier_uniform, l2=l2_penalty)
            We = g.get_variable(expert_scope + "/weights", (d_in, vocab_size * M), xavier_uniform, l2=l2_penalty)
            be = g.get_variable(expert_scope + "/biases", (vocab_size * M,), zeros)
            p, loss = ops.moe_head_xent(model_input, Wg, We, be, labels, vocab_size, M, bf16=FLAGS.compute_dtype == "bfloat16")
            return {"predictions": p, "loss": loss}
        return {"predictions": moe_block(model_input, vocab_size, num_mixtures, l2_penalty, gate_scope, expert_scope)}


class DeepCombineChainModel(models.BaseModel):
    """W/all_video_models/deep_combine_chain_model.py:9-85: chain of MoE sub-predictions, each projected to
    relu cells, L2-normalised and concatenated to the input of the next stage (prediction_chain; composed links)."""

    def _first_input(self, model_input, l2_penalty, sub_scope, **unused_params):
        """What stage 0 reads: the model input."""
        return model_input

    def _link(self, noise_level):
        return composed_link(relu_kind(), noise_level)

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, sub_scope="",
                     original_input=None, dropout=False, keep_prob=None, noise_level=None, num_frames=None,
                     support_pool=None, **unused_params):
        """support_pool (this build's addition, None = the reference's behaviour): a callable applied to every stage's
        sub-prediction BEFORE the concatenation into "support_predictions" -- a caller that reduces the rows anyway (the attention
        composite takes the max over its A attention rows per video) then concatenates [B, V] pieces instead of [B * A, V] ones: the
        [B * A, L * V] copy (464 MB at B * A = 8192, L = 3) and the strided gradient slices it leaves behind disappear."""
        # the model input stays in front of every later stage's input (:66-70): when it is data, no head computes a gradient for it
        frozen = 0 if model_input.requires_grad else int(model_input.shape[1])
        grown = [self._first_input(model_input, l2_penalty, sub_scope, **unused_params)]

        def stage_input(k, links):                                  # the previous stage's input with the newest link behind it
            if k:
                grown[0] = torch.cat([grown[0], links[-1]], dim=1)
            return grown[0]

        return prediction_chain(self.sub_model, stage_input, self._link(noise_level), [], vocab_size, l2_penalty, sub_scope,
                                support_kwargs=dict(dropout=dropout, keep_prob=keep_prob, noise_level=noise_level),
                                frozen_cols=lambda k: frozen, support_pool=support_pool)

    def sub_model(self, model_input, vocab_size, **params):
        return moe_stage(model_input, vocab_size, **params)


class DistillchainDeepCombineChainModel(DeepCombineChainModel):
    """W/all_video_models/distillchain_deep_combine_chain_model.py:9-96: DeepCombineChainModel whose chain starts from
    [model_input | distill_norm], distill_norm = the l2-normalised relu projection (scope sub_scope + "distillrelu",
    --deep_chain_relu_cells wide here) of another model's predictions.  Every relu -> (noise) -> l2norm is one ops.chain_link."""

    def _first_input(self, model_input, l2_penalty, sub_scope, distillation_predictions=None, **unused_params):
        distill_norm = distill_link(distillation_predictions, FLAGS.deep_chain_relu_cells, l2_penalty, sub_scope + "distillrelu")
        return torch.cat([model_input, distill_norm], dim=1)

    def _link(self, noise_level):
        return fused_link(relu_kind(), noise_level)


# ---- Z = youtube-8m-zhangteng: the heads of the Extend attention plugins (frame_level_models.LstmExtendModel, InputExtendModel) ----
class MoeExtendModel(models.BaseModel):
    """Z/video_level_models.py:2272-2330: MoeModel's gates and experts (scopes "gates" and "experts") on the B E rows an Extend plugin
    hands over, E = --moe_num_extend consecutive rows per video, then the maximum over a video's E rows: predictions [B, V]."""

    def _rows(self, model_input, l2_penalty, **unused_params):
        """What the gates and experts read: the rows as they come."""
        return model_input

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, original_input=None, **unused_params):
        num_mixtures = num_mixtures or FLAGS.moe_num_mixtures
        num_extends = FLAGS.moe_num_extend
        assert model_input.shape[0] % num_extends == 0, "MoeExtendModel wants --moe_num_extend rows per video"
        rows = self._rows(model_input, l2_penalty, **unused_params)
        p = moe_block(rows, vocab_size, num_mixtures, l2_penalty, "gates", "experts")
        return {"predictions": ops.frame_pool(p.view(-1, num_extends, vocab_size), "max")}       # tf.reduce_max over a video's rows


class MoeExtendDistillChainModel(MoeExtendModel):
    """Z/video_level_models.py:2332-2400: MoeExtendModel whose rows carry, behind the input, class_input = relu(FC(another model's
    predictions)) under scope "class_inputs", of fixed width 256 and NOT l2-normalised (unlike distill_link), tiled over a video's E
    rows.  Without distillation predictions (the reference's distill_labels is None) it is MoeExtendModel."""
    CLASS_SIZE = 256

    def _rows(self, model_input, l2_penalty, distillation_predictions=None, **unused_params):
        if distillation_predictions is None:
            return model_input
        num_extends = FLAGS.moe_num_extend
        class_input = fully_connected(distillation_predictions.to(torch.float32), self.CLASS_SIZE, "class_inputs", activation="relu",
                                      l2_penalty=l2_penalty)
        B = class_input.shape[0]
        tiled = class_input.unsqueeze(1).expand(B, num_extends, self.CLASS_SIZE).reshape(B * num_extends, self.CLASS_SIZE)
        return torch.cat([model_input, tiled], dim=1)


# ---- Z's cascade heads: a MoeModel that also reads another model's predictions -------------------------------------------------------
def distill_chain_head(model_input, vocab_size, distillation_predictions, mode, num_mixtures=None, l2_penalty=1e-8, split=False):
    """The body of the four heads below.  t = distillation_predictions [B, V] (the reference's distill_labels), cast to fp32, is data.
    z = FC(t[:, v0:]) under "class_inputs", CLASS_SIZE = 256 wide; the MoE block (scopes "gates" and "experts") reads
    ops.distill_input(model_input, z, t, mode, v0) and predicts the first V1 labels; predictions = ops.distill_blend(p1, t, --ensemble_w,
    V1).  split: V1 = v0 = --softmax_bound, else V1 = V and v0 = 0.  Variables in the order class_inputs/weights, class_inputs/biases,
    gates/weights, experts/weights, experts/biases.  model_input is data in video-level use (no head gradient is computed for it) and an
    LSTM memory in frame-level use."""
    assert distillation_predictions is not None, "distillation feature must be used"
    t = distillation_predictions.detach().to(torch.float32)
    bound = vocab_size
    if split:
        bound = int(FLAGS.softmax_bound)
        assert 0 < bound < vocab_size, "MoeDistillSplitModel wants 0 < --softmax_bound = %d < %d labels" % (bound, vocab_size)
    v0 = bound if split else 0
    z = fully_connected(t[:, v0:] if v0 else t, MoeExtendDistillChainModel.CLASS_SIZE, "class_inputs", l2_penalty=l2_penalty)
    frozen = 0 if model_input.requires_grad else int(model_input.shape[1])
    head_input = ops.distill_input(model_input, z, t, mode, v0)
    p1 = moe_block(head_input, bound, num_mixtures or FLAGS.moe_num_mixtures, l2_penalty, "gates", "experts", frozen_cols=frozen)
    return {"predictions": ops.distill_blend(p1, t, FLAGS.ensemble_w, bound)}


class MoeDistillChainModel(models.BaseModel):
    """Z/video_level_models.py:286-357: MoeModel on [model_input | relu(FC(t))], t another model's predictions, FC under "class_inputs"
    (256 wide, no normalisation), then predictions * --ensemble_w + t * (1 - --ensemble_w).  Without t the reference dereferences None
    at its last line; here the assertion of distill_link is raised."""
    MODE, SPLIT = "chain", False

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, distillation_predictions=None,
                     original_input=None, **unused_params):
        return distill_chain_head(model_input, vocab_size, distillation_predictions, self.MODE, num_mixtures, l2_penalty, self.SPLIT)


class MoeDistillChainNormModel(MoeDistillChainModel):
    """Z/video_level_models.py:359-432: the head input is [l2norm(model_input) | l2norm(FC(t) / sum_v t)], no activation.  One deliberate
    difference from the reference: a row whose t sums to exactly 0 is 0 / 0 = NaN there; here its class part is zeros and its
    pre-activation receives a zero gradient (teacher predictions are sigmoid outputs: this never happens on real data)."""
    MODE = "norm"


class MoeDistillChainNorm2Model(MoeDistillChainModel):
    """Z/video_level_models.py:434-507: MoeDistillChainNormModel with relu before the division; the same zero-sum rule."""
    MODE = "norm2"


class MoeDistillSplitModel(MoeDistillChainModel):
    """Z/video_level_models.py:509-582: V1 = --softmax_bound.  "class_inputs" reads t[:, V1:], the MoE block on [model_input | relu(FC)]
    predicts the first V1 labels only, and predictions = concat(p1, t[:, V1:]) * --ensemble_w + t * (1 - --ensemble_w): the other labels
    are the teacher's own.  0 < V1 < V is asserted."""
    MODE, SPLIT = "split", True


# ---- Z's combine chain heads: MoE stages chained through a pair of elu "class inputs" per stage -------------------------------------
_CLASS_MATRICES = {}      # (file, device) -> device tensor [V, K] (the reference's tf.constant of np.loadtxt(--class_file))


def _class_matrix(device):
    """--class_file as a float32 [V, K] constant on `device`, loaded once per (file, device) as losses._vertical_mapping does."""
    key = (FLAGS.class_file, str(device))
    seq = _CLASS_MATRICES.get(key)
    if seq is None:
        import numpy as np
        seq = torch.from_numpy(np.atleast_2d(np.loadtxt(FLAGS.class_file)).astype(np.float32)).to(device).contiguous()
        _CLASS_MATRICES[key] = seq
    return seq


def mix_chain_head(model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, knowledge=False, normalize=True, support_pool=None,
                   block=None, first_name=""):
    """The body of the two heads below.  An MoE block under "gates" / "experts" gives p; for i < --moe_layers, ops.mix_link under
    "class_inputs1-<i>" and "class_inputs2-<i>" (--class_size wide each: c1 = elu(FC(p)), c2 = elu(FC(1 - p)), or elu(FC(p . seq)) with
    `knowledge`; with `normalize` each l2-normalised and multiplied by sqrt(class_size / D), D the width of the head's own input) grows
    the stage input to [previous input | c1 | c2], and the MoE block under "gates-<i>" / "experts-<i>" gives the next p.  Returns
    "predictions", the last p, and "predictions_class", the first --moe_layers of the --moe_layers + 1 predictions side by side
    (support_pool, where given, applied to each piece and to the predictions first, as DeepCombineChainModel's).  Variables in the
    reference's order: gates, experts, then per stage class_inputs1-i, class_inputs2-i, gates-i, experts-i; xavier weights under
    l2_penalty, zero biases, no bias on the gates.  model_input is data in video-level use (no head computes a gradient for its
    columns) and an attention-pooled LSTM output in frame-level use.
    block(stage_input, name, frozen_cols) -> [B, vocab_size], where given, stands for the MoE block and makes its own Variables under
    scopes that end in `name`: first_name for the first prediction, "-<i>" for stage i (MoeSoftmaxModel: "pre", then "-0", "-1", ...)."""
    g = get_default_graph()
    M = num_mixtures or FLAGS.moe_num_mixtures
    C, layers = int(FLAGS.class_size), int(FLAGS.moe_layers)
    D = int(model_input.shape[1])
    scale = float(torch.sqrt(torch.tensor(float(C), dtype=torch.float32) / D))       # tf.sqrt(tf.cast(class_size, tf.float32) / shape)
    frozen = 0 if model_input.requires_grad else D
    seq = _class_matrix(model_input.device) if knowledge else None
    if seq is not None and seq.shape[0] != vocab_size:
        raise ValueError("--class_file=%s holds %d rows for %d labels" % (FLAGS.class_file, seq.shape[0], vocab_size))
    pool = support_pool or (lambda t: t)
    if block is None:
        block = lambda x, name, frozen_cols: moe_block(x, vocab_size, M, l2_penalty, "gates" + name, "experts" + name, frozen_cols=frozen_cols)
    stage_input = model_input
    p = block(stage_input, first_name, frozen)
    pieces = []
    for i in range(layers):
        pieces.append(pool(p))
        W1 = g.get_variable("class_inputs1-%d/weights" % i, (vocab_size, C), xavier_uniform, l2=l2_penalty)
        b1 = g.get_variable("class_inputs1-%d/biases" % i, (C,), zeros)
        q = ops.matmul_const(p, seq) if knowledge else None
        W2 = g.get_variable("class_inputs2-%d/weights" % i, (vocab_size if q is None else q.shape[1], C), xavier_uniform, l2=l2_penalty)
        b2 = g.get_variable("class_inputs2-%d/biases" % i, (C,), zeros)
        stage_input = ops.mix_link(stage_input, p, W1, b1, W2, b2, q=q, norm=normalize, scale=scale, dx_from=frozen)
        p = block(stage_input, "-%d" % i, frozen)
    res = {"predictions": pool(p)}
    if pieces:
        res["predictions_class"] = pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=1)
    return res


class MoeMix4Model(models.BaseModel):
    """Z/video_level_models.py:1872-2044, the --moe_group=False path: mix_chain_head with c2 = elu(FC(1 - p)); the class inputs are
    normalised unless --frame_features.  Its result holds "predictions_class" [B, --moe_layers V], which train.TrainGraph trains by
    Z's mix loss (TrainGraph._mix_loss).  With --moe_layers=0 the reference returns its one prediction under both keys."""

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, original_input=None, support_pool=None,
                     **unused_params):
        if FLAGS.moe_group:
            raise NotImplementedError("MoeMix4Model --moe_group=True (label groups of --class_size) is not built: no script of the final "
                                      "submission's list sets it")
        frame_features = "frame_features" in FLAGS and FLAGS.frame_features
        res = mix_chain_head(model_input, vocab_size, num_mixtures, l2_penalty, normalize=not frame_features, support_pool=support_pool)
        res.setdefault("predictions_class", res["predictions"])
        return res


class MoeKnowledgeModel(models.BaseModel):
    """Z/video_level_models.py:1331-1438: MoeMix4Model's chain with c2 = elu(FC(p . seq)), seq [V, K] the constant matrix of
    np.loadtxt(--class_file); as in the reference its class inputs are normalised whatever --frame_features says."""

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, original_input=None, **unused_params):
        res = mix_chain_head(model_input, vocab_size, num_mixtures, l2_penalty, knowledge=True)
        res.setdefault("predictions_class", res["predictions"])
        return res


def softmax_moe_block(model_input, vocab_size, bound, num_mixtures, l2_penalty, name, frozen_cols=0):
    """MoeSoftmaxModel.sub_model (Z/video_level_models.py:879-960) under scopes that end in `name`: the MoE block for the first `bound`
    labels ("gates<name>", "experts<name>") and the label-softmax mixture for the other V - bound and one more that stands for none of
    them ("class_gates-0<name>", no bias; "class_experts-0<name>"): two products through ops.linear -- S (M + 1) is odd at the workload, so
    neither takes an N % 4 form -- and ops.softmax_moe, which writes the whole row [sigmoid part | q[:, :S - 1]].  The reference's
    `channels` is the constant 1; its loop is not generalised."""
    g = get_default_graph()
    d_in, M = model_input.shape[-1], num_mixtures
    S = vocab_size - bound + 1
    head = moe_block(model_input, bound, M, l2_penalty, "gates" + name, "experts" + name, frozen_cols=frozen_cols)
    Wg = g.get_variable("class_gates-0%s/weights" % name, (d_in, S * (M + 1)), xavier_uniform, l2=l2_penalty)
    We = g.get_variable("class_experts-0%s/weights" % name, (d_in, S * M), xavier_uniform, l2=l2_penalty)
    be = g.get_variable("class_experts-0%s/biases" % name, (S * M,), zeros)
    x = model_input.reshape(-1, d_in)
    return ops.softmax_moe(ops.linear(x, Wg), ops.linear(x, We, be), S, M, head=head, overwrite_logits=True)


class MoeSoftmaxModel(models.BaseModel):
    """Z/video_level_models.py:877-1017: the sigmoid MoE block predicts the first --softmax_bound labels and a mixture whose experts are
    a softmax over the labels predicts the others; the blocks are chained as MoeMix4Model's (mix_chain_head: "pre", then "-<i>" behind
    class_inputs1-<i> / class_inputs2-<i>, always normalised -- the reference has no --frame_features branch here).  The result holds
    "predictions_class", so train.TrainGraph trains it by the mix rule: under --label_loss=CrossEntropyLoss, the reference's script as
    committed, by TrainGraph._mix_loss; under SplitSoftmaxLoss by that class's calculate_loss_mix.  With --moe_layers=0 the one
    prediction is under both keys.  0 < --softmax_bound < vocab_size is asserted."""

    def create_model(self, model_input, vocab_size, num_mixtures=None, l2_penalty=1e-8, original_input=None, **unused_params):
        M, bound = num_mixtures or FLAGS.moe_num_mixtures, int(FLAGS.softmax_bound)
        assert 0 < bound < vocab_size, "MoeSoftmaxModel wants 0 < --softmax_bound = %d < %d labels" % (bound, vocab_size)
        block = lambda x, name, frozen_cols: softmax_moe_block(x, vocab_size, bound, M, l2_penalty, name, frozen_cols)
        res = mix_chain_head(model_input, vocab_size, num_mixtures, l2_penalty, block=block, first_name="pre")
        res.setdefault("predictions_class", res["predictions"])
        return res
