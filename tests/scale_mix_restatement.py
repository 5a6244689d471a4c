"""Restatement of the LstmMultiscale models, of their per-label mix of the scales and of the training rule they are trained under, in
plain torch, in the dtype of its inputs (float64 for the reference values, float32 for the error bound), in the reference's form and
with its variable names (Z = youtube-8m-zhangteng of the reference: Z/frame_level_models.py:2827-3373, Z/train.py:359-379, :418):
    final_probilities = tf.stack(..., axis=1); weight = tf.nn.softmax(tf.einsum("aij,ijk->aik", moe_inputs, weight2d), dim=1)
    predictions = tf.reduce_sum(final_probilities * weight, axis=1);  prediction_frames = tf.reshape(final_probilities, [-1, V])
the scale loop batch-major with tf.pad shifts, oracle.torch_ref.lstm_stack / batch_norm_train, the scalar-gate cell of
gate_lstm_restatement, and the loss on prediction_frames with literally tiled labels.  Shared by tests/test_scale_mix_host.py and
tests/test_gpu_scale_mix.py; not a test module."""
import numpy as np
import torch

from ensemble_restatement import bound  # noqa: F401  (re-exported: the GPU tests' bound)
from gate_lstm_restatement import NAMES as GATE_NAMES, cross_entropy, err, moe, rnn_gate, shapes as gate_shapes  # noqa: F401

BN_EPS, BN_DECAY = 1e-3, 0.999
FILTER_SIZES = (1, 2, 3)
CLASS_SIZE = 256
PLUGINS = ("LstmMultiscaleModel", "LstmMultiscale2Model", "LstmMultiscaleDitillChainModel")


# ---- the op ---------------------------------------------------------------------------------------------------------------------------
def scale_mix(ps, zs):
    """ps, zs: L tensors [B,V] each -> sum_l softmax_l(z)_l p_l, written as the reference writes it."""
    final_probilities = torch.stack(list(ps), dim=1)                       # [B, L, V]
    weight = torch.softmax(torch.stack(list(zs), dim=1), dim=1)
    return (final_probilities * weight).sum(dim=1)


def scale_mix_with_grads(ps, zs, g, dtype):
    """out, [dp_l], [dz_l] by autograd in `dtype` from float32 numpy planes ps, zs [L,B,V] and g [B,V]."""
    pt = [torch.from_numpy(np.ascontiguousarray(p)).to(dtype).requires_grad_(True) for p in ps]
    zt = [torch.from_numpy(np.ascontiguousarray(z)).to(dtype).requires_grad_(True) for z in zs]
    out = scale_mix(pt, zt)
    out.backward(torch.from_numpy(g).to(dtype))
    return out.detach(), [t.grad for t in pt], [t.grad for t in zt]


# ---- the models -----------------------------------------------------------------------------------------------------------------------
def num_filters(name, cnn_cells=256):
    return (cnn_cells, cnn_cells, 2 * cnn_cells) if name == "LstmMultiscaleDitillChainModel" else (256, 256, 512)


def variable_shapes(name, D, V, L, M, lstm_cells=1024, cnn_cells=256, distill=False):
    """{variable name: shape} of plugin `name`, written from Z/frame_level_models.py (cnn :2849-2861, rnn :2936-2947 -- a one-cell
    MultiRNNCell --, rnn_gate :3275-3276 with LstmGateModel.create_recurrent_unit, sub_moe :2890-2902 / :3053-3072, ensemble_weight2d
    :2979-2981 / :3151-3153 / :3366-3368)."""
    nfl = num_filters(name, cnn_cells)
    C, H = sum(nfl), lstm_cells
    want = {}
    for k in range(1, L + 1):
        d = D if k == 1 else C
        for fs, n in zip(FILTER_SIZES, nfl):
            want["cnn%dcnn-filter-len%d" % (k, fs)] = (d * fs, n)
        for n in ("gamma", "beta", "moving_mean", "moving_variance"):
            want["cnn%dcluster_bn/%s" % (k, n)] = (C,)
        if name == "LstmMultiscale2Model":
            for n, s in gate_shapes(C, H).items():
                want["rnn%dlstm_forward/%s" % (k, n)] = s
        else:
            want["RNN-rnn%d/multi_rnn_cell/cell_0/basic_lstm_cell/weights" % k] = (C + H, 4 * H)
            want["RNN-rnn%d/multi_rnn_cell/cell_0/basic_lstm_cell/biases" % k] = (4 * H,)
        extra = CLASS_SIZE if (distill and name == "LstmMultiscaleDitillChainModel") else 0
        if extra:
            want["class_inputsmoe%d/weights" % k] = (V, CLASS_SIZE)
            want["class_inputsmoe%d/biases" % k] = (CLASS_SIZE,)
        want["gatesmoe%d/weights" % k] = (H + extra, V * (M + 1))
        want["expertsmoe%d/weights" % k] = (H + extra, V * M)
        want["expertsmoe%d/biases" % k] = (V * M,)
    want["ensemble_weight2d"] = (L, H if name == "LstmMultiscaleDitillChainModel" else C, V)
    return want


def cnn(model_input, P, sub_scope):
    """LstmMultiscaleModel.cnn without its batch norm: tf.pad shifts, tf.concat, tf.einsum("ijk,kl->ijl")."""
    B, max_frames, num_features = model_input.shape
    shift_inputs = []
    for i in range(max(FILTER_SIZES)):
        if i == 0:
            shift_inputs.append(model_input)
        else:
            shift_inputs.append(torch.nn.functional.pad(model_input, (0, 0, i, 0))[:, :max_frames, :])
    cnn_outputs = []
    for fs in FILTER_SIZES:
        sub_input = torch.cat(shift_inputs[:fs], dim=2)
        cnn_outputs.append(torch.einsum("ijk,kl->ijl", sub_input, P[sub_scope + "cnn-filter-len%d" % fs]))
    return torch.cat(cnn_outputs, dim=2)


def batch_norm(x2, P, scope, training):
    """slim.batch_norm(center=True, scale=True) over the rows of x2 -> (y, batch mean, batch variance) (None, None at inference)."""
    from oracle import torch_ref
    if training:
        return torch_ref.batch_norm_train(x2, P[scope + "/gamma"], P[scope + "/beta"], eps=BN_EPS)
    y = P[scope + "/gamma"] * (x2 - P[scope + "/moving_mean"]) * torch.rsqrt(P[scope + "/moving_variance"] + BN_EPS) + P[scope + "/beta"]
    return y, None, None


def model(name, model_input, num_frames, P, L, M, distill_labels=None, training=True):
    """create_model of plugin `name` on float frames [B,F,D]: {"predictions", "prediction_frames", "moments": [(mean, var) per scale]}."""
    from oracle import torch_ref
    B = model_input.shape[0]
    pool_size = 2
    cnn_input = model_input
    final_probilities, moe_inputs, moments = [], [], []
    for layer in range(L):
        k = layer + 1
        num_t = cnn_input.shape[1]
        cnn_output = cnn(cnn_input, P, "cnn%d" % k)
        features_size = cnn_output.shape[2]
        y, mu, var = batch_norm(cnn_output.reshape(B * num_t, features_size), P, "cnn%dcluster_bn" % k, training)
        moments.append((mu, var))
        cnn_output = torch.relu(y).view(B, num_t, features_size)
        if name == "LstmMultiscale2Model":
            Pg = {n: P["rnn%dlstm_forward/%s" % (k, n)] for n in GATE_NAMES}
            cnn_multiscale, _ = rnn_gate(cnn_output, num_frames, Pg)
        else:
            s = "RNN-rnn%d/multi_rnn_cell/cell_0/basic_lstm_cell/" % k
            _, c, _ = torch_ref.lstm_stack(cnn_output, num_frames, [(P[s + "weights"], P[s + "biases"])])
            cnn_multiscale = c[0]
        moe_inputs.append(cnn_multiscale)
        moe_input = cnn_multiscale
        if name == "LstmMultiscaleDitillChainModel" and distill_labels is not None:
            class_input = torch.relu(distill_labels @ P["class_inputsmoe%d/weights" % k] + P["class_inputsmoe%d/biases" % k])
            moe_input = torch.cat((cnn_multiscale, class_input), dim=1)
        final_probilities.append(moe(moe_input, P["gatesmoe%d/weights" % k], P["expertsmoe%d/weights" % k], P["expertsmoe%d/biases" % k], M))
        num_t = pool_size * (num_t // pool_size)
        cnn_input = cnn_output[:, :num_t, :].reshape(B, num_t // pool_size, pool_size, features_size).amax(dim=2)
        num_frames = torch.clamp(num_frames // pool_size, min=1)
    final_probilities = torch.stack(final_probilities, dim=1)             # [B, L, V]
    moe_inputs = torch.stack(moe_inputs, dim=1)                            # [B, L, H]
    V = final_probilities.shape[2]
    if name == "LstmMultiscale2Model":
        predictions = final_probilities.mean(dim=1)
    else:
        weight = torch.softmax(torch.einsum("aij,ijk->aik", moe_inputs, P["ensemble_weight2d"]), dim=1)
        predictions = (final_probilities * weight).sum(dim=1)
    return {"predictions": predictions, "prediction_frames": final_probilities.reshape(-1, V), "moments": moments}


# ---- the training rule ----------------------------------------------------------------------------------------------------------------
def tile_labels(labels_batch, num_extend):
    """Z/train.py:361-362: tf.tile(tf.reshape(labels, [-1, 1, V]), [1, L, 1]) reshaped to [-1, V]."""
    B, V = labels_batch.shape
    return labels_batch.reshape(B, 1, V).repeat(1, num_extend, 1).reshape(-1, V)


def z_rule_loss(result, labels_batch, loss=cross_entropy):
    """Z/train.py:359-379, :418: label_loss * 0.0 + calculate_loss(prediction_frames, tiled labels)."""
    frames = result["prediction_frames"]
    L = frames.shape[0] // labels_batch.shape[0]
    return loss(result["predictions"], labels_batch) * 0.0 + loss(frames, tile_labels(labels_batch, L))


def adam_first_step(w, g, l2, lr=0.01, clip=1.0, b1=0.9, b2=0.999, eps=1e-8, reg_penalty=1.0):
    """What the first TrainGraph.step does to one variable (csrc/optim.hip): ge = g + l2 w, clipped to norm `clip` per tensor, TF Adam
    from m = v = 0.  Returns (w', m', v') in the dtype of w."""
    ge = g + (l2 * reg_penalty) * w
    norm = torch.sqrt((ge * ge).sum())
    ge = ge * (clip / torch.clamp(norm, min=clip))
    m, v = (1.0 - b1) * ge, (1.0 - b2) * ge * ge
    lr_t = lr * np.sqrt(1.0 - b2) / (1.0 - b1)
    return w - lr_t * m / (torch.sqrt(v) + eps), m, v


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def draw(shapes, rs, scale=0.03, filter_scale=0.1):
    """Weights for the small-shape comparisons (as tests/test_gpu_multiscale.py's _draw): a contractive recurrence, filters at the
    initialiser's 0.1, gamma near 1, beta around 0.2 so that a fair share of the ReLU inputs is positive, fresh moving averages, the gate
    cell's biases around the reference's constants, and an ensemble_weight2d large enough that the scales' weights differ."""
    P = {}
    for k, shp in shapes.items():
        leaf = k.split("/")[-1]
        if leaf == "gamma":
            P[k] = 1.0 + 0.1 * rs.randn(*shp)
        elif leaf == "beta":
            P[k] = 0.2 + 0.2 * rs.randn(*shp)
        elif leaf == "moving_mean":
            P[k] = np.zeros(shp)
        elif leaf == "moving_variance":
            P[k] = np.ones(shp)
        elif "cnn-filter" in k:
            P[k] = rs.randn(*shp) * filter_scale
        elif "lstm_forward/b" in k:
            P[k] = (1.0 if leaf == "bf" else 0.1) + 0.05 * rs.randn(*shp)
        elif k == "ensemble_weight2d":
            P[k] = rs.randn(*shp) * 0.5
        else:
            P[k] = rs.randn(*shp) * scale
    return {k: v.astype(np.float32) for k, v in P.items()}


def to_torch(P, dtype, device="cpu"):
    return {k: torch.from_numpy(np.asarray(v)).to(device=device, dtype=dtype).requires_grad_(not k.split("/")[-1].startswith("moving_"))
            for k, v in P.items()}


def reference(name, x, nf, labels, P, L, M, dtype, distill=None, device="cpu"):
    """The plugin and the Z-rule cross entropy in `dtype` on the same float32 inputs: predictions, prediction_frames, loss, the gradient of
    the loss for every trainable variable (zeros where it has none) and the batch moments."""
    tp = to_torch(P, dtype, device)
    xt = torch.from_numpy(x).to(device=device, dtype=dtype)
    d = None if distill is None else torch.from_numpy(distill).to(device=device, dtype=dtype)
    res = model(name, xt, torch.from_numpy(nf).to(device), tp, L, M, distill_labels=d)
    loss = z_rule_loss(res, torch.from_numpy(labels).to(device))
    loss.backward()
    grads = {k: (torch.zeros_like(t) if t.grad is None else t.grad).detach().cpu() for k, t in tp.items() if t.requires_grad}
    return {"predictions": res["predictions"].detach().cpu(), "prediction_frames": res["prediction_frames"].detach().cpu(),
            "loss": loss.detach().cpu(), "grads": grads, "moments": res["moments"]}
