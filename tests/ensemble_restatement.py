"""Restatements of the ensemble stage in plain torch, in the dtype of their inputs (float64 for the reference values, float32 for the
error bound), with variable names, shapes and einsum strings as E/all_ensemble_models/*.py writes them (E = youtube-8m-ensemble of the
reference).  Shared by tests/test_ensemble_host.py and tests/test_gpu_ensemble.py; not a test module."""
import numpy as np
import torch

EPSILON = 1e-5            # nonunit_matrix_regression_model.py:27


def xform(x, kind):
    return x if kind is None else torch.log((EPSILON + x) / (1.0 + EPSILON - x))


def combine(x, W, gate=None, kind=None):
    """(out [B, V], lse [B, V]) for x [B, V, M], W [J, V, M], gate [B, J] or None: gated_weight = einsum("ij,jkl->ikl", gate, W),
    weight = softmax(gated_weight), output = reduce_sum(weight * t(x), axis=2)."""
    B = x.shape[0]
    gated_weight = W[0].unsqueeze(0).expand(B, -1, -1) if gate is None else torch.einsum("ij,jkl->ikl", gate, W)
    weight = torch.softmax(gated_weight, dim=-1)
    return (weight * xform(x, kind)).sum(dim=2), torch.logsumexp(gated_weight, dim=-1)


def combine_with_grads(x, W, gate, kind, dout, dtype):
    """out, lse, dW [J, V, M], dgate [B, J] or None by autograd in `dtype` on the same float32 inputs."""
    x, W, dout = x.to(dtype), W.to(dtype).clone().requires_grad_(True), dout.to(dtype)
    gate = None if gate is None else gate.to(dtype).clone().requires_grad_(True)
    out, lse = combine(x, W, gate, kind)
    out.backward(dout)
    return out.detach(), lse.detach(), W.grad, None if gate is None else gate.grad


def moments(x):
    """(mean_input, std_input) of attention_moe_matrix_model.py:31-34: the mean over the methods and the sum of squared deviations over
    num_methods - 1."""
    mean_input = x.mean(dim=2)
    if x.shape[2] < 2:
        return mean_input, None
    return mean_input, ((x - mean_input.unsqueeze(2)) ** 2).sum(dim=2) / (x.shape[2] - 1)


def bound(ref32, ref64):
    """_bound of tests/test_gpu_distillchain.py: 4 x the error of the float32 restatement against the fp64 one, plus one float32 ulp of the
    largest reference magnitude."""
    big = float(ref64.abs().max()) if ref64.numel() else 0.0
    return 4.0 * float((ref32.double() - ref64).abs().max()) + float(np.spacing(np.float32(big)))


# ---- the plugins: P maps the reference's variable names to tensors --------------------------------------------------------------------
def _l2_normalize_rows(x):
    return x / torch.sqrt(torch.clamp((x * x).sum(dim=1, keepdim=True), min=1e-12))


def _l2_normalize_whole(x):
    """tf.nn.l2_normalize(x) with dim = None: reduce_sum over every axis."""
    return x / torch.sqrt(torch.clamp((x * x).sum(), min=1e-12))


def _attention_gate(model_input, original_input, P):
    original_input = _l2_normalize_rows(original_input)
    mean_output = model_input.mean(dim=2)
    return torch.softmax(torch.cat([original_input, mean_output], dim=1) @ P["gates/weights"] + P["gates/biases"], dim=-1)


def mean_model(model_input, original_input, P):
    return model_input.mean(dim=2)


def linear_regression_model(model_input, original_input, P):
    weight = torch.softmax(P["ensemble_weight"], dim=-1)
    return torch.einsum("ijk,k->ij", model_input, weight)


def matrix_regression_model(model_input, original_input, P):
    weight = torch.softmax(torch.einsum("ij,j->ij", P["ensemble_weight2d"], P["ensemble_weight1d"]), dim=-1)
    return torch.einsum("ijk,jk->ij", model_input, weight)


def nonunit_matrix_regression_model(model_input, original_input, P):
    log_model_input = torch.log((EPSILON + model_input) / (1.0 + EPSILON - model_input))
    weight = torch.softmax(P["ensemble_weight"], dim=-1)
    return torch.sigmoid(torch.einsum("ijk,jk->ij", log_model_input, weight))


def attention_linear_model(model_input, original_input, P):
    gate_activations = _attention_gate(model_input, original_input, P)
    gated_weight = torch.einsum("ij,jk->ik", gate_activations, P["ensemble_weight"])
    weight = torch.softmax(gated_weight, dim=-1)
    return torch.einsum("ik,ijk->ij", weight, model_input)


def attention_matrix_model(model_input, original_input, P, gate_activations=None, extra=0.0):
    if gate_activations is None:
        gate_activations = _attention_gate(model_input, original_input, P)
    weight_xy = torch.einsum("ijl,ilk->ijk", P["ensemble_weightx"], P["ensemble_weighty"]) + extra
    gated_weight_xy = torch.einsum("ij,jkl->ikl", gate_activations, weight_xy)
    weight = torch.softmax(gated_weight_xy, dim=-1)
    return (weight * model_input).sum(dim=2)


def attention_linmatrix_model(model_input, original_input, P):
    return attention_matrix_model(model_input, original_input, P, extra=P["ensemble_weight"] + P["ensemble_bias"])


def attention_moe_matrix_model(model_input, original_input, P):
    mean_input, std_input = moments(model_input)
    relu = lambda t, s: torch.relu(t @ P["relu-%s/weights" % s] + P["relu-%s/biases" % s])
    parts = [_l2_normalize_whole(relu(t, s)) for t, s in ((original_input, "origin"), (mean_input, "mean"), (std_input, "std"))]
    gate_activations = torch.softmax(torch.cat(parts, dim=1) @ P["gates/weights"] + P["gates/biases"], dim=-1)
    return attention_matrix_model(model_input, original_input, P, gate_activations=gate_activations)


PLUGINS = {"MeanModel": mean_model, "LinearRegressionModel": linear_regression_model, "MatrixRegressionModel": matrix_regression_model,
           "NonunitMatrixRegressionModel": nonunit_matrix_regression_model, "AttentionLinearModel": attention_linear_model,
           "AttentionMatrixModel": attention_matrix_model, "AttentionLinmatrixModel": attention_linmatrix_model,
           "AttentionMoeMatrixModel": attention_moe_matrix_model}


def plugin_shapes(name, V, M, D, J, R, cells):
    """The reference's variables of plugin `name`, in creation order."""
    gates = lambda width: [("gates/weights", (width, J)), ("gates/biases", (J,))]
    xy = [("ensemble_weightx", (J, V, R)), ("ensemble_weighty", (J, R, M))]
    return dict({
        "MeanModel": [],
        "LinearRegressionModel": [("ensemble_weight", (M,))],
        "MatrixRegressionModel": [("ensemble_weight1d", (M,)), ("ensemble_weight2d", (V, M))],
        "NonunitMatrixRegressionModel": [("ensemble_weight", (V, M))],
        "AttentionLinearModel": gates(D + V) + [("ensemble_weight", (J, M))],
        "AttentionMatrixModel": gates(D + V) + xy,
        "AttentionLinmatrixModel": gates(D + V) + [("ensemble_bias", (J, 1, 1)), ("ensemble_weight", (J, 1, M))] + xy,
        "AttentionMoeMatrixModel": [("relu-origin/weights", (D, cells)), ("relu-origin/biases", (cells,)), ("relu-mean/weights", (V, cells)),
                                    ("relu-mean/biases", (cells,)), ("relu-std/weights", (V, cells)), ("relu-std/biases", (cells,))]
        + gates(3 * cells) + xy,
    }[name])


def plugin_case(name, B, V, M, D, J, R, cells, seed):
    """(model_input [B, V, M] in (0, 1) as float32 numpy, original_input [B, D], parameters {name: float32 array}, coefficient [B, V])."""
    rs = np.random.RandomState(seed)
    x = rs.rand(B, V, M).astype(np.float32)
    orig = rs.randn(B, D).astype(np.float32)
    P = {k: (rs.randn(*s) * (1.0 if k.startswith("ensemble") else 0.5)).astype(np.float32) for k, s in plugin_shapes(name, V, M, D, J, R, cells).items()}
    return x, orig, P, rs.randn(B, V).astype(np.float32)


def plugin_reference(name, x, orig, P, coef):
    """fp64: predictions, and the gradient of sum(coef * predictions) for every variable."""
    tp = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for k, v in P.items()}
    pred = PLUGINS[name](torch.from_numpy(x.astype(np.float64)), torch.from_numpy(orig.astype(np.float64)), tp)
    if tp:
        (pred * torch.from_numpy(coef.astype(np.float64))).sum().backward()
    return pred.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in tp.items()}


# ---- the plugin itself ------------------------------------------------------------------------------------------------------------------
def run_plugin(name, x, orig, P, coef, device, J, rank, cells):
    """Predictions and {variable: gradient of sum(coef * predictions)} of plugin `name` with the parameters P on `device`."""
    import yt8m_amd.ensemble as ensemble
    import yt8m_amd.ensemble_level_models as elm
    from yt8m_amd.variables import reset_default_graph
    g = reset_default_graph(device=device, seed=0)
    model = getattr(elm, name)()
    xt = ensemble.stack_methods(torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))).to(device))
    assert xt.stride() == (x.shape[1], 1, x.shape[0] * x.shape[1]) or x.shape[0] == 1
    ot = torch.from_numpy(orig).to(device)
    g.begin_step()
    model.create_model(xt, vocab_size=x.shape[1], original_input=ot)
    assert [(k, tuple(v.data.shape)) for k, v in g.vars.items()] == list(plugin_shapes(name, x.shape[1], x.shape[2], orig.shape[1], J, rank, cells).items())
    g.finalize()
    for k, v in P.items():
        g.vars[k].data.copy_(torch.from_numpy(v).to(device))
    g.begin_step()
    pred = model.create_model(xt, vocab_size=x.shape[1], original_input=ot)["predictions"]
    if pred.requires_grad:
        (pred * torch.from_numpy(coef).to(device)).sum().backward()
    for v in g.trainable_variables():
        if not v.grad_written:
            v.grad.zero_()                                               # what TrainGraph.step does for variables the step did not touch
    return pred.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in g.vars.items()}, g
