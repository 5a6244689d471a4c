"""Not -m gpu: the label losses of losses.py beyond plain cross entropy -- names and flags, the torch restatement of their formulas
(W/losses.py:76-108, 132-148, 281-356) that tests/test_gpu_losses.py judges the kernels with, pinned here against values worked out
by hand, the inputs of the kernel cases, and the argument checks of the C ABI.

The restatements take the dtype of their input: float64 is the reference, float32 the composition from torch ops that sets the
tolerance of the kernel tests and serves as the baseline of tools/label_loss_step.py.  They write the positive predictions as
p y + (1 - y), which is p y + 1 - y without the rounding of (p y + 1) for a float32 p: exact for 0/1 labels in either dtype, so the
same float32 p gives the same comparisons in float32 and in float64."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

EPS = 10e-6
TOPK = 20
# (B, V) of the kernel cases: one row with every class inside the top 20; one workgroup with a ragged tail; two column blocks, the
# second with 6 elements; the real width; more partial sums (64 * 5 = 320) than one wave holds
SHAPES = [(1, 20), (3, 37), (5, 1030), (4, 4716), (64, 4716)]


def cross_entropy_terms(p, y):
    return -(y * torch.log(p + EPS) + (1 - y) * torch.log(1 - p + EPS))


def batch_agreement_parts(p, y, a, N):
    """Every intermediate of BatchAgreementCrossEntropyLoss; the masks are comparisons, the counts sums of masks: no gradient."""
    ce = cross_entropy_terms(p, y)
    min_pp = (p * y + (1.0 - y)).amin()
    max_np = (p * (1.0 - y)).amax()
    fn = (p < max_np).to(p.dtype) * y
    fp = (p > min_pp).to(p.dtype) * (1.0 - y)
    n_fn, n_fp = fn.sum(), fp.sum()
    c_fn, c_fp = (p * fn).sum() / n_fn, (p * fp).sum() / n_fp
    r = torch.clamp(max_np - min_pp, min=EPS)
    w_fn = torch.sigmoid((c_fp - p) / r * 3.0) * (n_fp / N) * fn
    w_fp = torch.sigmoid((p - c_fn) / r * 3.0) * (n_fn / N) * fp
    w = (w_fn + w_fp) * a + 1.0
    return dict(loss=(w * ce).sum(dim=1).mean(), w=w, fn=fn, fp=fp, n_fn=n_fn, n_fp=n_fp, c_fn=c_fn, c_fp=c_fp, r=r, min_pp=min_pp,
                max_np=max_np)


def batch_agreement_ref(p, y, a, N):
    return batch_agreement_parts(p, y, a, N)["loss"]


def topk_batch_agreement_parts(p, y, a):
    if p.shape[1] < TOPK:
        raise ValueError("top_k(k = 20) of %d classes" % p.shape[1])
    ce = cross_entropy_terms(p, y)
    tau = torch.topk(p.detach(), TOPK, dim=1).values[:, TOPK - 1:TOPK]
    m = (p >= tau).to(p.dtype)
    ym = y * m
    min_pp = (p * ym + (1.0 - ym)).amin().detach()
    fn = (p < tau).to(p.dtype) * y
    fp = (p > min_pp).to(p.dtype) * (1.0 - y) * m
    w = ((fn + fp) * a + 1.0).detach()
    return dict(loss=(w * ce).sum(dim=1).mean(), w=w, fn=fn, fp=fp, tau=tau[:, 0], min_pp=min_pp)


def topk_batch_agreement_ref(p, y, a):
    return topk_batch_agreement_parts(p, y, a)["loss"]


def weighted_xent_ref(p, y, c_fn, c_fp):
    return (-(c_fn * y * torch.log(p + EPS) + c_fp * (1 - y) * torch.log(1 - p + EPS))).sum(dim=1).mean()


def mse_ref(p, y):
    return ((y - p) ** 2).sum(dim=1).mean()


def hinge_ref(p, y, b=1.0):
    m = b - (2.0 * y - 1.0) * p
    return torch.where(m > 0, m, torch.zeros_like(m)).sum(dim=1).mean()          # gradient 0 at m == 0


def smoothing_ref(y, epsilon=0.1):
    return y * (1.0 - epsilon) + y.sum(dim=1, keepdim=True) / y.shape[1] * epsilon


def loss_and_grad(fn, p, *args, dtype=torch.float64, upstream=1.0):
    """(loss, dL/dp) of a restatement in `dtype`, as float64 numpy."""
    q = p.detach().to(dtype).requires_grad_(True)
    loss = fn(q, *[a.to(dtype) if torch.is_tensor(a) else a for a in args])
    (loss * upstream).backward()
    return float(loss.detach()), q.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def case(B, V):
    """The inputs of one kernel case: p uniform in (0.02, 0.98), labels about 10 % dense (made once, shared, never written to)."""
    rs = np.random.RandomState(1000 * B + V)
    p = torch.from_numpy((0.02 + 0.96 * rs.rand(B, V)).astype(np.float32))
    y = torch.from_numpy(rs.rand(B, V) < 0.1)
    if not y.any():
        y[0, 0] = True
    return p, y


def test_the_loss_names_resolve_and_the_flags_have_the_reference_defaults(flags):
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    for name in ["BatchAgreementCrossEntropyLoss", "TopKBatchAgreementCrossEntropyLoss", "WeightedCrossEntropyLoss", "MeanSquareErrorLoss",
                 "HingeLoss"]:
        cls = train.find_class_by_name(name, [losses])                    # train.py's own lookup of --label_loss
        assert cls is getattr(losses, name) and issubclass(cls, losses.BaseLoss)
    for name in ["PairwiseHingeLoss", "MixedLoss", "SoftmaxLoss", "MultiTaskCrossEntropyAndSoftmaxLoss",
                 "MultiTaskDivergenceCrossEntropyLoss", "MultiTaskDivergenceCrossEntropyAndMSELoss"]:
        assert name in losses.__doc__                                     # left out, with the reason
        with pytest.raises(StopIteration):
            train.find_class_by_name(name, [losses])
    assert flags.batch_agreement == 0.1 and flags.false_negative_punishment == 1.0 and flags.false_positive_punishment == 1.0
    flags.parse(["--label_loss=TopKBatchAgreementCrossEntropyLoss", "--batch_agreement=0.5", "--false_negative_punishment", "2"])
    assert flags.batch_agreement == 0.5 and flags.false_negative_punishment == 2.0
    assert type(train.find_class_by_name(flags.label_loss, [losses])()) is losses.TopKBatchAgreementCrossEntropyLoss


def test_build_graph_resolves_the_label_loss_flag(flags):
    import yt8m_amd.losses as losses
    import yt8m_amd.train as train
    from yt8m_amd.variables import Graph
    g = Graph(device="cpu")
    assert type(train.build_graph(object(), graph=g).label_loss_fn) is losses.CrossEntropyLoss
    for name in ("BatchAgreementCrossEntropyLoss", "TopKBatchAgreementCrossEntropyLoss", "HingeLoss"):
        flags.label_loss = name
        assert type(train.build_graph(object(), graph=g).label_loss_fn) is getattr(losses, name)
    given = losses.MeanSquareErrorLoss()
    assert train.build_graph(object(), label_loss_fn=given, graph=g).label_loss_fn is given
    flags.label_loss = "PairwiseHingeLoss"
    with pytest.raises(StopIteration):
        train.build_graph(object(), graph=g)


def test_topk_loss_refuses_fewer_than_20_classes(flags):
    import yt8m_amd.losses as losses
    import yt8m_amd.train                                                 # noqa: F401 (--batch_size is train.py's flag)
    import yt8m_amd._lib as L
    p, y = torch.full((2, 19), 0.5), torch.zeros(2, 19, dtype=torch.bool)
    with pytest.raises(ValueError, match="20"):
        losses.TopKBatchAgreementCrossEntropyLoss().calculate_loss(p, y)
    with pytest.raises(ValueError):
        topk_batch_agreement_ref(p.double(), y.double(), 0.1)
    with pytest.raises(L.Yt8mHipError):                                   # 20 classes on the host: no CPU fallback
        losses.TopKBatchAgreementCrossEntropyLoss().calculate_loss(torch.full((2, 20), 0.5), torch.zeros(2, 20, dtype=torch.bool))
    with pytest.raises(L.Yt8mHipError):
        losses.BatchAgreementCrossEntropyLoss().calculate_loss(p, y, weights=None)
    with pytest.raises(ValueError, match="shape"):
        losses.BatchAgreementCrossEntropyLoss().calculate_loss(p, y[:, :-1])


def _f(t):
    return float(t.detach())


def _ce(p, y):
    return -(math.log(p + EPS) if y else math.log(1 - p + EPS))


def test_batch_agreement_restatement_on_a_batch_worked_out_by_hand():
    """2 x 3, one positive per row.  Positives 0.9 and 0.3: min_pp = 0.3.  Negatives 0.2, 0.25, 0.8, 0.1: max_np = 0.8.  The positive
    0.3 lies below max_np (the false negative, c_fn = 0.3), the negative 0.8 above min_pp (the false positive, c_fp = 0.8); r = 0.5.
    With a = 0.1 and N = 4 both carry the weight 1 + 0.1 sigmoid(3 (0.8 - 0.3) / 0.5) (1 / 4) = 1 + 0.025 sigmoid(3)."""
    p = torch.tensor([[0.9, 0.2, 0.25], [0.3, 0.8, 0.1]], dtype=torch.float64)
    y = torch.tensor([[1, 0, 0], [1, 0, 0]], dtype=torch.float64)
    q = p.clone().requires_grad_(True)
    parts = batch_agreement_parts(q, y, 0.1, 4.0)
    assert parts["fn"].tolist() == [[0, 0, 0], [1, 0, 0]] and parts["fp"].tolist() == [[0, 0, 0], [0, 1, 0]]
    assert _f(parts["min_pp"]) == 0.3 and _f(parts["max_np"]) == 0.8 and abs(_f(parts["r"]) - 0.5) < 1e-15
    assert _f(parts["c_fn"]) == 0.3 and _f(parts["c_fp"]) == 0.8 and _f(parts["n_fn"]) == 1 and _f(parts["n_fp"]) == 1
    extra = 0.025 / (1.0 + math.exp(-3.0))
    plain = sum(_ce(v, l) for v, l in [(0.9, 1), (0.2, 0), (0.25, 0), (0.3, 1), (0.8, 0), (0.1, 0)])
    want = (plain + extra * (_ce(0.3, 1) + _ce(0.8, 0))) / 2.0
    assert abs(_f(parts["loss"]) - want) < 1e-14
    parts["loss"].backward()
    # an element outside both sets and off both extrema gets the gradient of its plain cross entropy, over the 2 rows
    assert abs(float(q.grad[0, 0]) - (-1.0 / (0.9 + EPS)) / 2.0) < 1e-14
    assert abs(float(q.grad[0, 1]) - (1.0 / (1 - 0.2 + EPS)) / 2.0) < 1e-14
    # N is a parameter of its own, not the row count: the extra term is inversely proportional to it
    assert abs(float(batch_agreement_ref(p, y, 0.1, 8.0)) - (plain + 0.5 * extra * (_ce(0.3, 1) + _ce(0.8, 0))) / 2.0) < 1e-14
    # a = 0: the plain cross entropy
    assert abs(float(batch_agreement_ref(p, y, 0.0, 4.0)) - plain / 2.0) < 1e-14


def test_batch_agreement_restatement_ties_and_the_separated_batch():
    """Two negatives at max_np and two positives at min_pp: the gradient through r reaches each of a pair with one half.  Read off as
    the difference to the same batch with the weight's r held constant.  A perfectly separated batch has no false negative and no
    false positive: 0 / 0, NaN, as the reference."""
    p = torch.tensor([[0.75, 0.25, 0.5, 0.125], [0.25, 0.75, 0.375, 0.625]], dtype=torch.float64)
    y = torch.tensor([[0, 1, 1, 0], [1, 0, 0, 1]], dtype=torch.float64)
    q = p.clone().requires_grad_(True)
    parts = batch_agreement_parts(q, y, 0.5, 2.0)
    assert _f(parts["max_np"]) == 0.75 and _f(parts["min_pp"]) == 0.25
    g = torch.autograd.grad(parts["loss"], [q, parts["r"]], retain_graph=True)
    dr = float(g[1])
    assert abs(dr) > 1e-3
    q2 = p.clone().requires_grad_(True)
    ce = cross_entropy_terms(q2, y)
    r0 = parts["r"].detach()
    fn, fp = parts["fn"].detach(), parts["fp"].detach()
    c_fn, c_fp = (q2 * fn).sum() / fn.sum(), (q2 * fp).sum() / fp.sum()
    w = (torch.sigmoid((c_fp - q2) / r0 * 3.0) * (fp.sum() / 2.0) * fn + torch.sigmoid((q2 - c_fn) / r0 * 3.0) * (fn.sum() / 2.0) * fp) * 0.5 + 1.0
    (g_fixed,) = torch.autograd.grad((w * ce).sum(dim=1).mean(), q2)
    through_r = (g[0] - g_fixed).tolist()
    want = [[dr / 2, -dr / 2, 0, 0], [-dr / 2, dr / 2, 0, 0]]
    assert np.abs(np.array(through_r) - np.array(want)).max() < 1e-14
    sep_p = torch.tensor([[0.9, 0.1, 0.2], [0.3, 0.8, 0.7]], dtype=torch.float64)
    sep_y = torch.tensor([[1, 0, 0], [0, 1, 1]], dtype=torch.float64)
    assert math.isnan(float(batch_agreement_ref(sep_p, sep_y, 0.1, 2.0)))


def test_topk_restatement_on_a_row_worked_out_by_hand():
    """One row of 21 classes, p_i = (i + 1) / 22: the top 20 are classes 1..20, tau = 2/22.  Class 0 is a positive outside the top 20
    (a false negative); class 10 (p = 0.5) the only positive inside, so min_pp = 0.5 and the negatives 11..20 are false positives."""
    p = torch.tensor([[(i + 1) / 22.0 for i in range(21)]], dtype=torch.float64)
    y = torch.zeros(1, 21, dtype=torch.float64)
    y[0, 0] = y[0, 10] = 1
    q = p.clone().requires_grad_(True)
    parts = topk_batch_agreement_parts(q, y, 0.25)
    assert _f(parts["tau"][0]) == 2 / 22.0 and _f(parts["min_pp"]) == 0.5
    assert parts["fn"][0].tolist() == [1.0] + [0.0] * 20 and parts["fp"][0].tolist() == [0.0] * 11 + [1.0] * 10
    plain = sum(_ce((i + 1) / 22.0, i in (0, 10)) for i in range(21))
    want = plain + 0.25 * (_ce(1 / 22.0, 1) + sum(_ce((i + 1) / 22.0, 0) for i in range(11, 21)))
    assert abs(_f(parts["loss"]) - want) < 1e-13
    parts["loss"].backward()                                              # w is a constant: 1.25 times the plain gradient
    assert abs(float(q.grad[0, 0]) - 1.25 * (-1.0 / (1 / 22.0 + EPS))) < 1e-12
    assert abs(float(q.grad[0, 20]) - 1.25 / (1 - 21 / 22.0 + EPS)) < 1e-12
    assert abs(float(q.grad[0, 5]) - 1.0 / (1 - 6 / 22.0 + EPS)) < 1e-12
    # no positive inside any top 20: min_pp = 1, no false positive
    y2 = torch.zeros(1, 21, dtype=torch.float64)
    y2[0, 0] = 1
    parts2 = topk_batch_agreement_parts(p, y2, 0.25)
    assert _f(parts2["min_pp"]) == 1.0 and _f(parts2["fp"].sum()) == 0 and _f(parts2["fn"].sum()) == 1


def test_pointwise_restatements_by_hand():
    p = torch.tensor([[0.25, 0.5], [1.0, 0.75]], dtype=torch.float64)
    y = torch.tensor([[1.0, 0.0], [1.0, 0.0]], dtype=torch.float64)
    assert abs(float(mse_ref(p, y)) - (0.75 ** 2 + 0.25 + 0 + 0.75 ** 2) / 2) < 1e-15
    # hinge, b = 1: 1 - p for a positive, 1 + p for a negative; p = 1 on a positive is the kink: value 0, gradient 0
    q = p.clone().requires_grad_(True)
    h = hinge_ref(q, y)
    assert abs(_f(h) - (0.75 + 1.5 + 0 + 1.75) / 2) < 1e-15
    h.backward()
    assert q.grad.tolist() == [[-0.5, 0.5], [0.0, 0.5]]
    want = -(2.0 * math.log(0.25 + EPS) + 3.0 * math.log(0.5 + EPS) + 2.0 * math.log(1 + EPS) + 3.0 * math.log(0.25 + EPS)) / 2
    assert abs(float(weighted_xent_ref(p, y, 2.0, 3.0)) - want) < 1e-14
    assert smoothing_ref(y).tolist() == [[0.9 + 0.05, 0.05], [0.9 + 0.05, 0.05]]


@pytest.mark.parametrize("B,V", SHAPES)
def test_the_kernel_cases_are_well_conditioned(B, V):
    """Every case has false negatives and false positives, a finite fp64 loss and gradient, a range near 0.9, and float32 makes the
    comparisons that float64 makes."""
    p, y = case(B, V)
    yf = y.to(torch.float32)
    ba = batch_agreement_parts(p.double(), yf.double(), 0.1, 1024.0)
    assert float(ba["n_fn"]) >= 1 and float(ba["n_fp"]) >= 1 and float(ba["r"]) > 0.5
    for fn, args in ((batch_agreement_ref, (yf, 0.1, 1024.0)), (topk_batch_agreement_ref, (yf, 0.1))):
        loss, dp = loss_and_grad(fn, p, *args)
        assert math.isfinite(loss) and np.isfinite(dp).all()
    ba32 = batch_agreement_parts(p, yf, 0.1, 1024.0)
    assert torch.equal(ba32["fn"].double(), ba["fn"]) and torch.equal(ba32["fp"].double(), ba["fp"])
    tk, tk32 = topk_batch_agreement_parts(p.double(), yf.double(), 0.1), topk_batch_agreement_parts(p, yf, 0.1)
    assert torch.equal(tk32["fn"].double(), tk["fn"]) and torch.equal(tk32["fp"].double(), tk["fp"])
    assert torch.equal(tk32["tau"].double(), tk["tau"])


def test_c_abi_refuses_bad_arguments_without_a_device():
    import yt8m_amd._lib as L
    lib = L.lib()
    one = ctypes.c_void_p(16)                                             # never dereferenced: validation fails first
    B, V = 4, 37
    assert lib.yt8m_batch_agreement_workspace_bytes(0, 5) == 0
    assert lib.yt8m_batch_agreement_workspace_bytes(1024, 4716) == 4 * 6 * 1024 * 5    # six partial sums per workgroup
    assert lib.yt8m_batch_agreement_workspace_bytes(4, 37) == 4 * 6 * 4
    assert lib.yt8m_pointwise_loss_workspace_bytes(3, 1030) == 4 * 6
    ba_f = lambda p, y, dt, loss, st, b, v, ws: lib.yt8m_batch_agreement_fwd(p, y, dt, loss, st, b, v, 1e-5, 0.1, 1024.0, ws, None)
    tk_f = lambda p, y, dt, loss, st, b, v, ws: lib.yt8m_topk_batch_agreement_fwd(p, y, dt, loss, st, b, v, 1e-5, 0.1, ws, None)
    for f in (ba_f, tk_f):
        assert f(one, one, 0, one, one, 0, V, one) == -2                  # empty batch
        assert f(one, one, 0, one, one, B, 0, one) == -2
        assert f(one, one, 0, one, one, 65536, V, one) == -2              # the grid's second dimension
        assert f(one, one, 2, one, one, B, V, one) == -1                  # label dtype
        for nul in range(5):
            ptrs = [one] * 5
            ptrs[nul] = None
            assert f(ptrs[0], ptrs[1], 0, ptrs[2], ptrs[3], B, V, ptrs[4]) == -1, nul
            assert b"null operand" in lib.yt8m_last_error()
    assert tk_f(one, one, 0, one, one, B, 19, one) == -2                   # V < 20
    assert b"20" in lib.yt8m_last_error()
    ba_b = lambda p, y, dt, st, dp, b, v: lib.yt8m_batch_agreement_bwd(p, y, dt, st, None, dp, b, v, 1e-5, 1.0, None)
    tk_b = lambda p, y, dt, st, dp, b, v: lib.yt8m_topk_batch_agreement_bwd(p, y, dt, st, None, dp, b, v, 1e-5, 0.1, 1.0, None)
    for f in (ba_b, tk_b):
        assert f(one, one, 0, one, one, 0, V) == -2
        assert f(one, one, 0, one, one, 65536, V) == -2
        assert f(one, one, 7, one, one, B, V) == -1
        for nul in range(4):
            ptrs = [one] * 4
            ptrs[nul] = None
            assert f(ptrs[0], ptrs[1], 1, ptrs[2], ptrs[3], B, V) == -1, nul
    assert tk_b(one, one, 0, one, one, B, 19) == -2
    pw_f = lambda kind, p, y, dt, loss, b, v, ws: lib.yt8m_pointwise_loss_fwd_bwd(kind, p, y, dt, loss, None, b, v, 1.0, 1.0, 1e-5, 1.0, ws, None)
    pw_b = lambda kind, p, y, dt, dp, b, v: lib.yt8m_pointwise_loss_bwd(kind, p, y, dt, None, dp, b, v, 1.0, 1.0, 1e-5, 1.0, None)
    assert pw_f(3, one, one, 0, one, B, V, one) == -1 and pw_b(-1, one, one, 0, one, B, V) == -1      # loss kind
    for kind in (0, 1, 2):
        assert pw_f(kind, one, one, 0, one, 0, V, one) == -2 and pw_b(kind, one, one, 0, one, 0, V) == -2
        assert pw_f(kind, one, one, 2, one, B, V, one) == -1 and pw_b(kind, one, one, 2, one, B, V) == -1
        assert pw_f(kind, None, one, 0, one, B, V, one) == -1 and pw_f(kind, one, None, 0, one, B, V, one) == -1
        assert pw_f(kind, one, one, 0, None, B, V, one) == -1 and pw_f(kind, one, one, 0, one, B, V, None) == -1
        assert pw_b(kind, None, one, 0, one, B, V) == -1 and pw_b(kind, one, one, 0, None, B, V) == -1
