"""The recorder that stands in for the native library in the host tests (no GPU): every call is noted with its arguments as plain
Python values and returns 0; only the pure host queries (yt8m_x3_image_bytes, yt8m_moe_mix_bwd_bf16_partial_rows) answer with the real
library's value.  install() puts it in front of yt8m_amd.ops for one test, with CPU tensors as operands."""
import ctypes

import torch

import yt8m_amd._lib as _lib
import yt8m_amd.ops as ops

HOST_QUERIES = ("yt8m_x3_image_bytes", "yt8m_moe_mix_bwd_bf16_partial_rows")
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
    """A Recorder in place of the library, and ops' device check, stream and workspace in forms that CPU tensors pass; r.ws: the workspace."""
    r = Recorder(_lib.lib(), [], plain)
    ws = torch.empty(64, dtype=torch.float32)
    monkeypatch.setattr(_lib, "lib", lambda: r)
    monkeypatch.setattr(ops, "_dev", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_workspace", lambda device: ws)
    r.ws = ws
    return r
