"""Not -m gpu: --loss_function and --jsd_pi (Z/losses.py:33-38, :64-168) -- the flags and their defaults, the errors that
CrossEntropyLoss.calculate_loss raises under a set --loss_function, the torch restatement of the seven branches
(tests/loss_function_restatement.py) that tests/test_gpu_loss_function.py judges the kernels with, pinned here against values worked
out by hand on a 2 x 3 batch, and the C ABI of csrc/xent_variants.hip without a device."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import loss_function_restatement as R
from cabi_helpers import declared_bound_exported
from conftest import ROOT

E = 10e-6
SYMBOLS = ("yt8m_xent_variant_workspace_bytes", "yt8m_xent_variant_fwd", "yt8m_xent_variant_bwd")
# one positive per row; every value is its own
P = [[0.9, 0.2, 0.25], [0.3, 0.8, 0.1]]
Y = [[1, 0, 0], [1, 0, 0]]


def _t(rows):
    return torch.tensor(rows, dtype=torch.float64)


def _ce(q, t):
    return t * math.log(q + E) + (1 - t) * math.log(1 - q + E)


def _by_hand(c):
    """mean over the 2 rows of the sum over the 3 columns of -c(p, y)."""
    return sum(-c(p, y) for rp, ry in zip(P, Y) for p, y in zip(rp, ry)) / 2.0


# ---- flags and errors -------------------------------------------------------------------------------------------------------------------
def test_the_flags_exist_with_the_reference_defaults(flags):
    import yt8m_amd.losses as losses
    assert flags.loss_function is None and flags.jsd_pi == 0.5
    flags.parse(["--loss_function=loss_jsd", "--jsd_pi", "0.25"])
    assert flags.loss_function == "loss_jsd" and flags.jsd_pi == 0.25
    assert losses.LOSS_FUNCTIONS == R.NAMES
    import yt8m_amd.ops as ops
    assert tuple(ops.XENT_VARIANTS) == R.NAMES and sorted(ops.XENT_VARIANTS.values()) == list(range(7))


def test_a_set_loss_function_raises_what_it_cannot_serve(flags):
    import yt8m_amd._lib as L
    import yt8m_amd.losses as losses
    ce = losses.CrossEntropyLoss()
    p, y = torch.full((2, 3), 0.5), torch.zeros(2, 3, dtype=torch.bool)
    flags.loss_function = "loss_smoothing"
    with pytest.raises(ValueError, match=re.escape("./resources/embedding_matrix.model")):
        ce.calculate_loss(p, y)
    flags.loss_function = "loss_wieght"                                    # a typo must not train the plain cross entropy
    with pytest.raises(ValueError) as err:
        ce.calculate_loss(p, y)
    assert all(name in str(err.value) for name in R.NAMES)
    assert "typo" in losses.CrossEntropyLoss.__doc__ and "silently" in losses.CrossEntropyLoss.__doc__
    for name in R.NAMES:
        flags.loss_function = name
        with pytest.raises(ValueError, match="weights"):
            ce.calculate_loss(p, y, weights=torch.ones(2))
        flags.label_smoothing = True
        with pytest.raises(ValueError, match="label_smoothing"):
            ce.calculate_loss(p, y)
        flags.label_smoothing = False
        with pytest.raises(L.Yt8mHipError):                                # host tensors: no CPU or composed fallback
            ce.calculate_loss(p, y)
    # both terms of the multi-task loss go through the same method
    flags.loss_function, flags.support_type = "loss_wieght", "label"
    with pytest.raises(ValueError, match="loss_relabel"):
        losses.MultiTaskCrossEntropyLoss().calculate_loss(p, p, y)
    # every other --label_loss class ignores the flag: it reaches its own kernels' device check, not a ValueError
    with pytest.raises(L.Yt8mHipError):
        losses.MeanSquareErrorLoss().calculate_loss(p, y)
    import yt8m_amd.ops as ops
    with pytest.raises(ValueError, match="loss_margin"):
        ops.xent_variant(p, y, "loss_smoothing")


def test_the_documents_name_what_is_here_and_what_is_left_out():
    import yt8m_amd.losses as losses
    doc = losses.__doc__
    left = doc[doc.index("Left out of the rest of Z/losses.py"):]
    for name in ("loss_smoothing", "calculate_loss_distill", "calculate_loss_negative", "calculate_loss_max", "calculate_loss_postprocess",
                 "CrossEntropyLoss_weight"):
        assert name in left, name
    assert "loss_relabel" not in left and "loss_weight" not in left
    for name in R.NAMES:
        assert name in doc and name in losses.CrossEntropyLoss.__doc__, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--loss_function" in readme and all(name in readme for name in R.NAMES)


# ---- the restatements by hand -----------------------------------------------------------------------------------------------------------
def test_pointwise_restatements_by_hand():
    p, y = _t(P), _t(Y)
    assert abs(float(R.loss_square(p, y)) - _by_hand(lambda q, t: _ce(q * q, t))) < 1e-14
    assert abs(float(R.loss_sqrt(p, y)) - _by_hand(lambda q, t: _ce(math.sqrt(q), t))) < 1e-14
    assert abs(float(R.loss_weight(p, y)) - _by_hand(lambda q, t: 10 * t * math.log(q + E) + (1 - t) * math.log(1 - q + E))) < 1e-14

    def mix(q, t):
        return _ce(q, t) + q * math.log(t + E) + (1 - q) * math.log(1 - t + E) - q * math.log(q + E) - (1 - q) * math.log(1 - q + E)

    assert abs(float(R.loss_mix(p, y)) - _by_hand(mix)) < 1e-13
    for a in (0.5, 0.25):
        def jsd(q, t):
            d = (1 - a) * t + a * q
            return ((1 - a) * q * math.log(d + E) + (1 - a) * (1 - q) * math.log(1 - d + E) + a * t * math.log(d + E)
                    + a * (1 - t) * math.log(1 - d + E) - (1 - a) * q * math.log(q + E) - (1 - a) * (1 - q) * math.log(1 - q + E))
        assert abs(float(R.loss_jsd(p, y, a)) - _by_hand(jsd)) < 1e-14
        assert abs(float(R.restatement("loss_jsd", p, y, a)) - _by_hand(jsd)) < 1e-14
    # the 10 sits on the positives alone: the difference to the plain cross entropy is 9 times the positives' terms
    plain = _by_hand(_ce)
    assert abs(float(R.loss_weight(p, y)) - plain - 9 * (-math.log(0.9 + E) - math.log(0.3 + E)) / 2) < 1e-14
    # sqrt's derivative at p = 0 is what the formula gives: d/dp log(1 - sqrt(p) + e) = -1 / (1 + e) / (2 sqrt(0)) on a negative
    q = torch.tensor([[0.0, 0.5]], dtype=torch.float64, requires_grad=True)
    R.loss_sqrt(q, _t([[0, 1]])).backward()
    assert math.isinf(float(q.grad[0, 0])) and float(q.grad[0, 0]) > 0 and math.isfinite(float(q.grad[0, 1]))


def test_margin_restatement_by_hand():
    p, y = _t(P), _t(Y)
    wp = [0.5 - math.log(0.9 + E), 0.5 - math.log(0.3 + E)]                # the two positives
    pos = (0.9 * wp[0] + 0.3 * wp[1]) / (wp[0] + wp[1]) * 1.0              # one positive per row
    neg_p = [0.2, 0.25, 0.8, 0.1]
    wn = [0.5 - math.log(1 - q + E) for q in neg_p]
    neg = sum(q * w for q, w in zip(neg_p, wn)) / sum(wn) * 2.0            # two negatives per row
    assert abs(float(R.loss_margin(p, y)) - (_by_hand(_ce) - (pos - neg))) < 1e-14
    # no stop_gradient: the quotient of the positives reaches a positive's gradient
    q = p.clone().requires_grad_(True)
    R.loss_margin(q, y).backward()
    s = wp[0] + wp[1]
    d_pwp, d_wp = wp[0] - 0.9 / (0.9 + E), -1.0 / (0.9 + E)
    want = -(1.0 / (0.9 + E)) / 2.0 - (d_pwp - (0.9 * wp[0] + 0.3 * wp[1]) / s * d_wp) / s
    assert abs(float(q.grad[0, 0]) - want) < 1e-13
    # a batch without a positive: 0 / 0
    assert math.isnan(float(R.loss_margin(p, torch.zeros_like(y))))


def test_relabel_restatement_by_hand():
    p, y = _t(P), _t(Y)
    plain = _by_hand(_ce)
    parts = R.relabel_parts(p, y)
    assert plain < 10 and not bool(parts["relabelled"])
    assert float(parts["loss"]) == float(parts["pre"]) and abs(float(parts["pre"]) - plain) < 1e-14       # pre itself under 10
    assert parts["max_index"].tolist() == [0, 1]
    # positives predicted 0: -log(e) = 11.5 each, pre above 10.  Row 0: the maximum 0.25 is tied, columns 1 and 2, and the lowest index
    # takes the label; row 1: the maximum 0.8 sits on a positive and the row stays as it is
    p2, y2 = _t([[0.0, 0.25, 0.25], [0.0, 0.8, 0.1]]), _t([[1, 0, 0], [1, 1, 0]])
    parts = R.relabel_parts(p2, y2)
    pre = (-2 * math.log(E) - 2 * math.log(0.75 + E) - math.log(0.8 + E) - math.log(0.9 + E)) / 2
    assert pre > 10 and abs(float(parts["pre"]) - pre) < 1e-14 and bool(parts["relabelled"])
    assert parts["max_index"].tolist() == [1, 1]
    assert parts["labels"].tolist() == [[1, 1, 0], [1, 1, 0]]
    now = pre + (math.log(0.75 + E) - math.log(0.25 + E)) / 2
    assert abs(float(parts["loss"]) - now) < 1e-14 and abs(float(R.loss_relabel(p2, y2)) - now) < 1e-14
    # only the taken branch contributes, and the added label carries no gradient of its own
    q = p2.clone().requires_grad_(True)
    R.loss_relabel(q, y2).backward()
    assert abs(float(q.grad[0, 1]) - (-1.0 / (0.25 + E)) / 2) < 1e-14 and abs(float(q.grad[0, 2]) - (1.0 / (0.75 + E)) / 2) < 1e-14
    # float labels tiled along the columns, as the mix loss hands them over: one added label per whole row
    wide = R.relabel_parts(torch.cat([p2, p2 * 0.5, p2], dim=1), y2.repeat(1, 3))
    assert wide["max_index"].tolist() == [1, 1] and float((wide["labels"] - y2.repeat(1, 3)).sum()) == 1.0


def test_the_relabelled_kernel_cases_have_the_pre_they_are_known_by():
    """test_losses_host.case lands in the relabelled branch at every shape of the kernel tests, far from the threshold of 10."""
    from test_losses_host import SHAPES, case
    for (B, V), want in zip(SHAPES, (17.2, 37.0, 980.7, 4425.7, 4428.5)):
        p, y = case(B, V)
        parts = R.relabel_parts(p.double(), y.double())
        assert abs(float(parts["pre"]) - want) < 0.05 and bool(parts["relabelled"]), (B, V)


# ---- the C ABI on the host ------------------------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_the_symbols():
    import yt8m_amd._lib as L
    import yt8m_amd.ops as ops
    src, lib = declared_bound_exported(SYMBOLS, r"int(?:64_t)?")
    assert "Z/losses.py:64-168" in src
    assert L.ABI_VERSION == 4 and lib.yt8m_abi_version() == 4            # symbols were added, nothing else moved
    P_, i64, f, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    assert L.SIGNATURES["yt8m_xent_variant_fwd"] == (i, [i, P_, P_, i, P_, P_, P_, i64, i64, f, f, P_, P_])
    assert L.SIGNATURES["yt8m_xent_variant_bwd"] == (i, [i, P_, P_, i, P_, P_, P_, P_, i64, i64, f, f, f, P_])
    # the stats layout and the kinds: the header's named constants are ops.py's
    assert int(re.search(r"#define YT8M_XV_STATS_FLOATS (\d+)", src).group(1)) == ops.XV_STATS_FLOATS
    for key, name in (("loss", "LOSS"), ("pre", "PRE"), ("flag", "FLAG"), ("pos", "POS"), ("neg", "NEG")):
        assert int(re.search(r"#define YT8M_XV_STAT_%s (\d+)" % name, src).group(1)) == ops.XV_STATS[key]
    for kind, code in ops.XENT_VARIANTS.items():
        assert re.search(r"YT8M_XV_%s = %d\b" % (kind[len("loss_"):].upper(), code), src), kind


def test_c_abi_refuses_bad_arguments_without_a_device():
    """Every call here fails validation: nothing is launched and no device is needed."""
    import yt8m_amd._lib as L
    lib = L.lib()
    BADARG, SHAPE = -1, -2
    p = lambda k: ctypes.c_void_p(4096 * k)
    assert lib.yt8m_xent_variant_workspace_bytes(0, 5) == 0 and lib.yt8m_xent_variant_workspace_bytes(5, -1) == 0
    assert lib.yt8m_xent_variant_workspace_bytes(1024, 4716) == 4 * 7 * 1024 * 5       # seven partial sums per workgroup
    assert lib.yt8m_xent_variant_workspace_bytes(4, 3 * 4716) == 4 * 7 * 4 * 14

    def fwd(kind=0, pp=p(1), labels=p(2), dt=0, loss=p(3), stats=p(4), argmax=p(5), B=4, V=37, ws=p(6)):
        return lib.yt8m_xent_variant_fwd(kind, pp, labels, dt, loss, stats, argmax, B, V, 0.5, 1e-5, ws, None)

    def bwd(kind=0, pp=p(1), labels=p(2), dt=0, stats=p(3), argmax=p(4), dp=p(5), B=4, V=37):
        return lib.yt8m_xent_variant_bwd(kind, pp, labels, dt, stats, argmax, None, dp, B, V, 0.5, 1e-5, 1.0, None)

    for kind in range(7):
        for name in ("pp", "labels", "loss", "stats", "ws"):
            assert fwd(kind=kind, **{name: None}) == BADARG, (kind, name)
            assert b"null operand" in lib.yt8m_last_error()
        for name in ("pp", "labels", "dp"):
            assert bwd(kind=kind, **{name: None}) == BADARG, (kind, name)
        for f in (fwd, bwd):
            assert f(kind=kind, dt=2) == BADARG and f(kind=kind, dt=-1) == BADARG
            assert f(kind=kind, B=0) == SHAPE and f(kind=kind, V=0) == SHAPE and f(kind=kind, B=65536) == SHAPE
            assert f(kind=kind, V=(1 << 31) - 1024) == SHAPE                       # the argmax is an int32 column
    assert fwd(kind=7) == BADARG and fwd(kind=-1) == BADARG and bwd(kind=7) == BADARG and bwd(kind=-1) == BADARG
    assert b"loss kind" in lib.yt8m_last_error()
    # the argmax buffer goes with loss_relabel, the stats of the forward call with loss_margin and loss_relabel
    assert fwd(kind=6, argmax=None) == BADARG and bwd(kind=6, argmax=None) == BADARG
    assert bwd(kind=6, stats=None) == BADARG and bwd(kind=5, stats=None) == BADARG
    assert b"stats" in lib.yt8m_last_error()


# ---- the measurement tool -------------------------------------------------------------------------------------------------------------
def test_the_step_tool_plans_its_legs_and_prints_help_without_a_device(monkeypatch):
    tools = os.path.join(ROOT, "tools")
    monkeypatch.syspath_prepend(tools)
    import importlib
    mod = importlib.import_module("loss_function_step")
    assert mod.SHAPES == ((1024, 4716, 1), (128, 4716, 1), (1024, 4716, 3)) and mod.CALLS == 20
    assert vars(mod.parser().parse_args([])) == dict(steps=50, warmup=5, timeout=300, repeats=2, calls=20, out=None, child=None, legs=[])
    plans = []
    monkeypatch.setattr(mod.steplib, "drive", lambda script, plan, *args, **kw: plans.append(list(plan)) or 0)
    monkeypatch.setattr(sys, "argv", ["loss_function_step.py"])
    assert mod.main() == 0
    assert [leg for leg, _ in plans[0]] == ["kernels"] * 2 + ["mix4_loss_relabel", "mix4_loss_weight", "mix4_flag_unset"] * 2
    r = subprocess.run([sys.executable, os.path.join(tools, "loss_function_step.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 0 and "--steps" in r.stdout and "--calls" in r.stdout, r.stderr
    rows = [__import__("json").loads(line) for line in open(os.path.join(ROOT, "profiles", "loss_function_step.jsonl"))]
    timed = [row for row in rows if row.get("leg") == "kernel" and row["loss_function"] != "cross_entropy"]
    assert len(timed) == 2 * 3 * 2 * 7 and {row["loss_function"] for row in timed} == set(R.NAMES)
    assert {(row["B"], row["V"]) for row in timed} == {(1024, 4716), (128, 4716), (1024, 14148)}
    assert {row["leg"] for row in rows} >= {"mix4_loss_relabel", "mix4_loss_weight", "mix4_flag_unset"}
