"""The recorder that stands in for the native library in the host tests (no GPU): every call is noted with its arguments as plain
Python values and returns 0; only the pure host queries (HOST_QUERIES: shape arithmetic, no device) answer with the real library's
value.  install() puts it in front of yt8m_amd.ops and yt8m_amd.seq_ops for one test, with CPU tensors as operands.  _Graph / _Var
stand in for the graph and its variables; _tagged / _normalise turn a log into JSON values that name the operand behind each pointer."""
import ctypes

import torch

import yt8m_amd._lib as _lib
import yt8m_amd.ops as ops
import yt8m_amd.seq_ops as seq_ops

HOST_QUERIES = ("yt8m_x3_image_bytes", "yt8m_moe_mix_bwd_bf16_partial_rows", "yt8m_skinny_supported")
FIELDS = ("M", "N", "K", "A", "lda", "B", "ldb", "C", "ldc", "bias", "beta")


def _plain(a):
    """A ctypes argument as plain Python values, taken when the call is made."""
    if isinstance(a, ctypes.Array):
        if a._type_ is _lib.GemmProblem:
            return [{f: getattr(p, f) for f in FIELDS} for p in a]
        return [getattr(v, "value", v) for v in a]
    if isinstance(a, ctypes.c_void_p):
        return a.value
    return a


class Recorder(object):
    """plain: what turns each argument into the value the log keeps (default: _plain)."""

    def __init__(self, real, log, plain=_plain):
        self._real, self.log, self._plain = real, log, plain

    def __getattr__(self, name):
        if name in HOST_QUERIES:
            return getattr(self._real, name)

        def call(*args):
            self.log.append((name, [self._plain(a) for a in args]))
            return 0
        return call

    def calls(self, *names):
        return [(n, a) for n, a in self.log if n in names]


def install(monkeypatch, plain=_plain):
    """A Recorder in place of the library, and the device check, stream and workspace of ops (seq_ops holds the first two under its own
    names) in forms that CPU tensors pass; r.ws: the workspace."""
    r = Recorder(_lib.lib(), [], plain)
    ws = torch.empty(64, dtype=torch.float32)
    monkeypatch.setattr(_lib, "lib", lambda: r)
    for mod in (ops, seq_ops):
        monkeypatch.setattr(mod, "_dev", lambda *ts: None)
        monkeypatch.setattr(mod, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_workspace", lambda device: ws)
    r.ws = ws
    return r


class _Ptr(object):
    """A pointer argument, kept apart from the integers until the case's operands can name it."""
    __slots__ = ("value",)

    def __init__(self, value):
        self.value = value


def _tagged(a):
    """_plain with every pointer as a _Ptr."""
    if isinstance(a, ctypes.Array):
        if a._type_ is _lib.GemmProblem:
            return [{f: _Ptr(getattr(p, f)) if f in ("A", "B", "C", "bias") else getattr(p, f) for f in FIELDS} for p in a]
        if a._type_ is ctypes.c_void_p:
            return [_Ptr(v) for v in a]
        return [getattr(v, "value", v) for v in a]
    if isinstance(a, ctypes.c_void_p):
        return _Ptr(a.value)
    return a


class _Graph(object):
    def __init__(self, hook, token_grad):
        self.grad_ready_hook = hook
        self.device = torch.device("cpu")
        self.token = torch.zeros((), requires_grad=token_grad)


class _Var(object):
    def __init__(self, name, data, graph, log, frozen):
        self.name, self._graph, self._log = name, graph, log
        self.data, self.grad = data, None if frozen else torch.zeros(data.shape)
        self.trainable = True

    def grad_beta(self):
        return 0.0

    def grad_done(self):
        self._log.append(("grad_done", self.name))


def _normalise(log, named):
    """The log as JSON values: names without their yt8m_ prefix; pointers as the operand they point into (its name, "+bytes" behind its
    start), "*" (anything else) or None; a yt8m_gemm_problem as the list of its FIELDS."""
    def ptr(v):
        if v is None:
            return None
        for name, t in named.items():
            lo = t.untyped_storage().data_ptr()
            if lo <= v < lo + t.untyped_storage().nbytes():
                return name if v == t.data_ptr() else "%s+%d" % (name, v - t.data_ptr())
        return "*"

    def value(a):
        if isinstance(a, _Ptr):
            return ptr(a.value)
        if isinstance(a, list):
            return [value(v) for v in a]
        if isinstance(a, dict):
            return [value(a[f]) for f in FIELDS]
        return a

    return [[name, args] if name == "grad_done" else [name[len("yt8m_"):]] + [value(a) for a in args] for name, args in log]
