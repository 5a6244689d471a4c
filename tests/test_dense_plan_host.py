"""CPU pin of what the dense products of the Python layer hand to the native library: ops.linear, ops.linear_cat,
seq_ops.attention_logits_u8, the hoisted input projections of gru_layer / lnlstm_layer / the frame-order scalar-gate layer on float
frames, and seq_ops.cnn_tm -- for every form their forward, weight-gradient and input-gradient products can take, the ordered library
calls of one forward and backward pass with their integer and float arguments, the yt8m_gemm_problem fields and the operand each pointer
is, and the grad_done() events between them.  Every op is driven through its public entry, on CPU zero tensors, with the library
replaced by the recorder of library_recorder.py and stand-in variables / graph; the normalised log of every case is compared with
tests/golden/dense_layer_calls.json, recorded before the forms were chosen in one plan (`python tests/test_dense_plan_host.py --record`
rewrites that file: only for a change that means to move a launch).  The cases put every predicate of the choice on both sides: see
_cases().

TABLE, further down, is the choice itself: what ops._dense_plan and ops._skinny_plan -- the one place where the forms are chosen --
answer at the same edges, as literals."""
import json
import os
import sys

import pytest
import torch

from conftest import ROOT

import yt8m_amd.ops as ops
import yt8m_amd.seq_ops as seq_ops
import yt8m_amd.wimg as wimg
from library_recorder import _Graph, _Var, _normalise, _tagged, install

EXPECTED = os.path.join(ROOT, "tests", "golden", "dense_layer_calls.json")
LIN = dict(op="linear", bf16=False, need_dx=True, bias="b", frozen=(), w_noncontig=False, knobs={})
CAT = dict(op="linear_cat", M=2048, N=8, full=(8, 12), group=(), rep=4, need_dx=None, bias="b", frozen=(), odd_part=None, knobs={})
ATT = dict(op="attn_u8", B=4, F=512, D=16, N=8, parts=("mean_x",), need_dx=True, bias="b", frozen=(), knobs={})
REC = dict(bf16=False, need_dx=True, frozen=(), knobs={})
CNN = dict(op="cnn_tm", M=512, B=8, D=512, filters=((1, 8), (2, 8)), need_dx=True, frozen=(), knobs={})


def _cases():
    """id -> the case.  frozen: variables without a gradient slot.  knobs: module knobs of ops flipped for the case."""
    cases = {}

    def add(name, base, **kw):
        assert name not in cases
        cases[name] = dict(base, **kw)

    # ops.linear, fp32 configuration: LINEAR_H2_MIN_ROWS / LINEAR_H2_MIN_MNK, N % 4 and K >= 512 forward, N >= 512 and K % 4 for dx
    add("lin-small", LIN, M=8, N=8, K=8)
    add("lin-h2", LIN, M=512, N=512, K=512)
    add("lin-rows511", LIN, M=511, N=512, K=512)
    add("lin-mnk-above", LIN, M=256, N=512, K=8192)                       # 2^30 >= 1e9 with M < 512
    add("lin-mnk-below", LIN, M=256, N=512, K=7616)                       # 998 244 352
    add("lin-n510", LIN, M=512, N=510, K=512)                             # N % 4 != 0 forward, N < 512 for dx
    add("lin-n514", LIN, M=512, N=514, K=512)                             # N % 4 != 0 forward only
    add("lin-k508", LIN, M=512, N=512, K=508)                             # K < 512 forward only
    add("lin-n508", LIN, M=512, N=508, K=512)                             # N < 512 for dx only
    add("lin-k513", LIN, M=512, N=512, K=513)                             # K % 4 != 0 for dx
    add("lin-w-noncontig", LIN, M=512, N=512, K=512, w_noncontig=True)
    add("lin-nodx", LIN, M=512, N=512, K=512, need_dx=False)
    add("lin-frozen-w", LIN, M=512, N=512, K=512, frozen=("W",))
    add("lin-frozen-b", LIN, M=512, N=512, K=512, frozen=("b",))
    add("lin-no-b", LIN, M=512, N=512, K=512, bias=None)
    add("lin-no-fwd-h2", LIN, M=512, N=512, K=512, knobs=dict(LINEAR_FWD_H2=False))
    add("lin-no-dx-h2", LIN, M=512, N=512, K=512, knobs=dict(LINEAR_DX_H2=False))
    # ops.linear, bf16 configuration: BF16_MIN_MACS = 2^27, BF16_MIN_ROWS = 512 where the weight is cast, an even reduction length per product
    B16 = dict(LIN, bf16=True)
    add("lin-bf16", B16, M=512, N=512, K=512)                             # exactly 2^27: three bf16 products, one dual cast of dy
    add("lin-bf16-macs-below", B16, M=512, N=511, K=512)                  # 2^27 - 2^18
    add("lin-bf16-rows510", B16, M=510, N=516, K=512)                     # >= 2^27, too few rows for the weight casts: dW alone is bf16
    add("lin-bf16-rows511", B16, M=511, N=512, K=512)
    add("lin-bf16-odd-k", B16, M=512, N=512, K=513)                       # forward h2 under bf16; dW and dx bf16
    add("lin-bf16-odd-n", B16, M=512, N=513, K=512)                       # dx h2-rows under bf16
    add("lin-bf16-odd-m", B16, M=513, N=512, K=512)                       # dW auto: no dual cast
    add("lin-bf16-nodx", B16, M=512, N=512, K=512, need_dx=False)
    add("lin-bf16-frozen-w", B16, M=512, N=512, K=512, frozen=("W",))
    add("lin-bf16-no-b", B16, M=512, N=512, K=512, bias=None)
    # a graph makes the gradient slots after its first forward pass: the forms chosen there hold when the slot appears before backward
    add("lin-bf16-late-slot", B16, M=512, N=512, K=512, frozen=("W", "b"), late_slot=True)
    add("lin-late-slot", LIN, M=512, N=512, K=512, frozen=("W", "b"), late_slot=True)
    # the narrow route of ops.linear: N <= 16 over SKINNY_MIN_ROWS rows goes to linear_cat
    for M in (2047, 2048):
        for N in (16, 17):
            add("lin-narrow-m%d-n%d" % (M, N), LIN, M=M, N=N, K=8)
    add("lin-narrow-rows-1", LIN, M=64, N=8, K=8, knobs=dict(SKINNY_MIN_ROWS=64))
    # ops.linear_cat: per full part the streaming kernels or the GEMM; per-group parts; bias on the first part only
    add("cat-skinny", CAT)
    add("cat-rows2047", CAT, M=2047, rep=1)
    add("cat-n17", CAT, N=17)
    add("cat-odd-k", CAT, full=(8, 6))                                    # K % 4 != 0: the second part on the GEMM
    add("cat-odd-k-first", CAT, full=(6, 8))                              # the part that carries the bias on the GEMM
    add("cat-k-too-long", CAT, full=(8, 4612))                            # yt8m_skinny_supported refuses: the weight image does not fit
    add("cat-misaligned", CAT, odd_part="misaligned")                     # second part 4 bytes off a 16-byte boundary
    add("cat-noncontig", CAT, odd_part="noncontig")                       # second part a column window: copied, then streamed
    add("cat-group", CAT, full=(8,), group=(4, 8))
    add("cat-group-nodx", CAT, full=(8, 12), group=(4,), need_dx=(True, False, False))
    add("cat-nodx-first", CAT, need_dx=(False, True))
    add("cat-nodx", CAT, need_dx=(False, False))
    add("cat-no-b", CAT, bias=None)
    add("cat-frozen-w", CAT, frozen=("W",))
    add("cat-frozen-b", CAT, full=(8,), group=(4,), frozen=("b",))
    # seq_ops.attention_logits_u8: the byte part writes y first; h [B,F,12] per frame, mean_x [B,16] per video
    for parts in ((), ("mean_x",), ("h", "mean_x"), ("h",)):
        name = "att-" + ("+".join(parts) or "bytes")
        add(name, ATT, parts=parts)
        add(name + "-no-b", ATT, parts=parts, bias=None)
        add(name + "-frozen-w", ATT, parts=parts, frozen=("W",))
    add("att-h+mean_x-nodx", ATT, parts=("h", "mean_x"), need_dx=False)
    add("att-h-odd-k", ATT, parts=("h6",))                                # K = 6: the per-frame part on the GEMM
    add("att-h-rows2044", ATT, F=511, parts=("h",))
    # hoisted input projections on float frames [F,B,D]: the size rule of the layers, never h2 under bf16; bf16 casts from K >= 32
    for op in ("gru", "lnlstm"):
        R = dict(REC, op=op)
        for bf in (False, True):
            s = "-bf16" if bf else ""
            add("%s-h2%s" % (op, s), R, F=4, B=128, D=512, H=512, bf16=bf)            # forward h2, dx h2-rows | bf16 casts
            add("%s-k256%s" % (op, s), R, F=4, B=128, D=256, H=512, bf16=bf)          # forward auto, dx h2-rows
            add("%s-h128%s" % (op, s), R, F=4, B=128, D=512, H=128, bf16=bf)          # forward h2, dx generic (N < 512) | below 2^27
        add("%s-rows511" % op, R, F=7, B=73, D=512, H=512)
        add("%s-nodx" % op, R, F=4, B=128, D=512, H=512, need_dx=False)
        add("%s-d510" % op, R, F=4, B=128, D=510, H=512)                              # K % 4 != 0 for dx, K < 512 forward
        add("%s-no-fwd-h2" % op, R, F=4, B=128, D=512, H=512, knobs=dict(LINEAR_FWD_H2=False))
        add("%s-no-dx-h2" % op, R, F=4, B=128, D=512, H=512, knobs=dict(LINEAR_DX_H2=False))
        add("%s-frozen-w" % op, R, F=4, B=128, D=512, H=512, frozen=("W", "Wg"))
    add("lnlstm-bf16-k16", dict(REC, op="lnlstm"), F=4, B=512, D=16, H=1024, bf16=True)   # 2^27 MACs forward, reduction length below 32
    add("lnlstm-bf16-k32", dict(REC, op="lnlstm"), F=4, B=512, D=32, H=1024, bf16=True)
    add("gru-bf16-odd-rows", dict(REC, op="gru"), F=3, B=171, D=512, H=512, bf16=True)    # 513 rows: dW's reduction length is odd
    for bf in (False, True):
        add("bigate-frame-order" + ("-bf16" if bf else ""), dict(REC, op="bigate"), F=4, B=128, D=512, H=512, bf16=bf)
    add("bigate-h128", dict(REC, op="bigate"), F=4, B=128, D=512, H=128)                   # y . Vv with K = H < 512: auto
    # seq_ops.cnn_tm: one grouped launch per shift; the group takes the h2 role only when every product in it passes the rule
    add("cnn-h2", CNN, M=520)                                             # shift 1 over 512 rows: h2 too
    add("cnn-shift1-511", CNN, M=519)
    add("cnn-shift1-small", CNN)                                          # shift 1 over 504 rows
    add("cnn-n6", CNN, filters=((1, 8), (2, 6)))                          # the second filter's N % 4 != 0 drops the role of both shifts
    add("cnn-n6-first", CNN, M=520, filters=((1, 6), (2, 8)))             # ... of shift 0 only
    add("cnn-d508", CNN, D=508)
    add("cnn-one-frame", CNN, B=512)                                      # B > M / 2: shift 1 has no rows
    add("cnn-nodx", CNN, need_dx=False)
    add("cnn-frozen", CNN, frozen=("f1",))
    add("cnn-no-fwd-h2", CNN, knobs=dict(LINEAR_FWD_H2=False))
    add("cnn-bf16", CNN, M=520, bf16=True)                                # the flag does not reach these products
    return cases


def _zeros(*shape, **kw):
    return torch.zeros(shape, **kw)


def _record(mp, case):
    """The normalised log of one case: the library calls and grad_done() events of a forward and a backward pass of the case's op."""
    c = _cases()[case]
    for k, v in c["knobs"].items():
        assert getattr(ops, k) != v, k                                    # flipped from its default
        mp.setattr(ops, k, v)
    mp.setattr(ops.FLAGS, "compute_dtype", "bfloat16" if c.get("bf16") else "float32")
    r = install(mp, plain=_tagged)
    mp.setattr(wimg, "BUFFERS", {})                                       # no resident weight images, whatever ran in this process before
    g = _Graph(None, True)
    named = {"ws": r.ws}
    inputs = []

    def var(name, *shape, data=None):
        v = _Var(name, _zeros(*shape) if data is None else data, g, r.log, name in c["frozen"])
        named[name] = v.data
        if v.grad is not None:
            named[name + ".grad"] = v.grad
        return v

    def inp(name, *shape, grad=True, data=None):
        t = (_zeros(*shape) if data is None else data).requires_grad_(bool(grad))
        named[name] = t
        if grad:
            inputs.append(t)
        return t

    op = c["op"]
    if op == "linear":
        M, N, K = c["M"], c["N"], c["K"]
        W = var("W", data=_zeros(K, 2 * N)[:, :N]) if c["w_noncontig"] else var("W", K, N)
        b = var("b", N) if c["bias"] else None
        outs = [ops.linear(inp("x", M, K, grad=c["need_dx"]), W, b, bf16=c["bf16"])]
        if c.get("late_slot"):
            for v in (W, b):
                v.grad = named[v.name + ".grad"] = torch.zeros(v.data.shape)
    elif op == "linear_cat":
        M, N = c["M"], c["N"]
        need = c["need_dx"] or (True,) * (len(c["full"]) + len(c["group"]))
        W = var("W", sum(c["full"]) + sum(c["group"]), N)
        b = var("b", N) if c["bias"] else None
        full = []
        for i, K in enumerate(c["full"]):
            data = None
            if i == 1 and c["odd_part"] == "misaligned":
                data = _zeros(M * K + 1)[1:].view(M, K)
                assert data.is_contiguous() and data.data_ptr() % 16 == 4
            elif i == 1 and c["odd_part"] == "noncontig":
                data = _zeros(M, K + 4)[:, :K]
            full.append(inp("p%d" % i, M, K, grad=need[i], data=data))
        group = [inp("g%d" % j, M // c["rep"], K, grad=need[len(full) + j]) for j, K in enumerate(c["group"])]
        outs = [ops.linear_cat(full, W, b, group_parts=group)]
    elif op == "attn_u8":
        B, F, D, N = c["B"], c["F"], c["D"], c["N"]
        q = torch.zeros(B, F, D, dtype=torch.uint8)
        rs = _zeros(B, F)
        named.update(q=q, rs=rs)
        shapes = dict(mean_x=(B, 16), h=(B, F, 12), h6=(B, F, 6))
        parts = [inp(p, *shapes[p], grad=c["need_dx"]) for p in c["parts"]]
        W = var("W", D + sum(p.shape[-1] for p in parts), N)
        b = var("b", N) if c["bias"] else None
        outs = [seq_ops.attention_logits_u8(q, rs, None, W, b, parts=parts)]
    elif op in ("gru", "lnlstm", "bigate"):
        F, B, D, H = c["F"], c["B"], c["D"], c["H"]
        x = inp("x", F, B, D, grad=c["need_dx"])
        nf = torch.full((B,), F, dtype=torch.int32)
        if op == "gru":
            outs = seq_ops.gru_layer(x, var("Wg", D + H, 2 * H), var("bg", 2 * H), var("Wc", D + H, H), var("bc", H), nf)
        elif op == "lnlstm":
            gammas = [var("gamma%d" % k, H) for k in range(5)]
            betas = [var("beta%d" % k, H) for k in range(5)]
            outs = seq_ops.lnlstm_layer(x, var("W", D + H, 4 * H), gammas, betas, nf)
        else:
            shapes = dict(Wv=(D, 4 * H), bv=(4 * H,), Ws=(D, 4), bs=(4,), Uv1=(H, 2 * H), Us1=(2, H), Vv=(H, 2 * H), Vs=(H, 2),
                          Uv2=(H, 2 * H), Us2=(2, H))
            params = [inp(k, *s) for k, s in shapes.items()]
            outs = seq_ops._BigateLstmLayer.apply(x, *params, nf, False)
    else:
        assert op == "cnn_tm"
        M, D = c["M"], c["D"]
        filters = [var("f%d" % k, fs * D, N) for k, (fs, N) in enumerate(c["filters"])]
        outs = [seq_ops.cnn_tm(inp("x", M, D, grad=c["need_dx"]), c["B"], filters)]
    r.log.append(("yt8m_backward", []))
    torch.autograd.backward(list(outs), [torch.zeros_like(o) for o in outs])
    assert all(t.grad is not None for t in inputs)
    return _normalise(r.log, named)


def _expected():
    """case -> its recorded log.  The file holds every distinct call or event once ("events", one per line) and each case as indices."""
    with open(EXPECTED) as f:
        rec = json.load(f)
    return {case: [rec["events"][i] for i in log] for case, log in rec["cases"].items()}


def _names(want, prefix, backward=None):
    """The calls of the cases whose id starts with `prefix`: all of them, or those before (False) / after (True) the backward mark."""
    seen = set()
    for case, log in want.items():
        if case.startswith(prefix):
            at = [e[0] for e in log].index("backward")
            seen |= {e[0] for e in (log if backward is None else log[at:] if backward else log[:at])}
    return seen


def test_the_cases_are_the_recorded_ones_and_reach_every_form():
    want = _expected()
    assert sorted(_cases()) == sorted(want)
    assert {"gemm_auto_grouped", "gemm_auto_grouped_ex", "h2_absmax", "h2_rowscales", "h2_split_rows", "gemm_h2_nt_ex", "cast_f32_bf16",
            "cast_f32_bf16_dual", "gemm_bf16_nt_grouped", "colsum_f32", "skinny_fwd_f32", "skinny_dw_f32", "skinny_dx_f32"} <= _names(want, "lin-")
    assert {"skinny_fwd_f32", "skinny_dw_f32", "skinny_dx_f32", "gemm_auto_grouped", "colsum_f32", "grad_done"} <= _names(want, "cat-")
    assert {"skinny_fwd_u8", "skinny_dw_u8", "skinny_fwd_f32", "skinny_dw_f32", "skinny_dx_f32", "gemm_auto_grouped", "colsum_f32",
            "grad_done"} <= _names(want, "att-")
    for op in ("gru", "lnlstm", "bigate"):
        assert {"gemm_auto_grouped", "cast_f32_bf16", "gemm_bf16_nt_grouped", "h2_rowscales", "gemm_h2_nt_ex"} <= _names(want, op + "-"), op
    assert {"gemm_auto_grouped", "grad_done"} <= _names(want, "cnn-")
    assert not any(e == ["grad_done", "W"] for case, log in want.items() if case.startswith("lin-") and "narrow" not in case for e in log)


@pytest.mark.parametrize("case", sorted(_cases()))
def test_library_calls_of_a_forward_and_backward_pass(monkeypatch, case):
    want = _expected()[case]
    got = json.loads(json.dumps(_record(monkeypatch, case)))              # tuples and floats as the file holds them
    assert got == want


# ---- the table itself: the plan functions at the same edges --------------------------------------------------------------------------
S = dict(M=512, N=512, K=512)                        # LINEAR_H2_MIN_ROWS / BF16_MIN_ROWS rows, exactly BF16_MIN_MACS = 2^27
BF = dict(S, bf16=True)
HO = dict(S, layer=False)                            # a hoisted / plain product
HB = dict(HO, bf16=True)
# (arguments of ops._dense_plan, knobs flipped) -> (fwd, dw, dy_dual, dx, xmax).  A change of a threshold or of a rule shows here.
TABLE = [
    # a layer, fp32 configuration: the h2 size rule, N % 4 == 0 and K >= 512 forward, N >= 512, K % 4 == 0 and a contiguous W for dx
    (dict(M=8, N=8, K=8), {},                          ("auto", "auto", False, "auto", False)),
    (S, {},                                            ("h2", "auto", False, "h2_rows", True)),
    (dict(S, M=511), {},                               ("auto", "auto", False, "auto", False)),
    (dict(M=256, N=512, K=8192), {},                   ("h2", "auto", False, "h2_rows", True)),       # LINEAR_H2_MIN_MNK: 2^30 >= 1e9
    (dict(M=256, N=512, K=7616), {},                   ("auto", "auto", False, "auto", False)),       # 998 244 352
    (dict(M=64, N=1024, K=16384), {},                  ("h2", "auto", False, "h2_rows", True)),
    (dict(S, N=510), {},                               ("auto", "auto", False, "auto", False)),
    (dict(S, N=514), {},                               ("auto", "auto", False, "h2_rows", False)),
    (dict(S, K=508), {},                               ("auto", "auto", False, "h2_rows", False)),
    (dict(S, N=508), {},                               ("h2", "auto", False, "auto", True)),
    (dict(S, K=513), {},                               ("h2", "auto", False, "auto", True)),
    (dict(S, w_contiguous=False), {},                  ("h2", "auto", False, "auto", True)),
    (dict(S, dy_contiguous=False), {},                 ("h2", "auto", False, "h2_rows", True)),       # a layer's dy is made contiguous
    (dict(S, need_dx=False), {},                       ("h2", "auto", False, None, True)),
    (dict(S, w_grad=False), {},                        ("h2", "auto", False, "h2_rows", True)),
    (S, dict(LINEAR_FWD_H2=False),                     ("auto", "auto", False, "h2_rows", False)),
    (S, dict(LINEAR_DX_H2=False),                      ("h2", "auto", False, "auto", True)),
    (dict(S, M=128), dict(LINEAR_H2_MIN_ROWS=128),     ("h2", "auto", False, "h2_rows", True)),
    (dict(S, M=511), dict(LINEAR_H2_MIN_MNK=1e8),      ("h2", "auto", False, "h2_rows", True)),
    # a layer, bf16 configuration: 2^27 MACs, an even reduction length per product, 512 rows where the weight is cast (forward, dx)
    (BF, {},                                           ("bf16_nt", "bf16_nt", True, "bf16_nt", False)),
    (dict(BF, N=511), {},                              ("auto", "auto", False, "auto", False)),       # 2^27 - 2^18; N % 4 != 0, N < 512
    (dict(BF, M=510, N=516), {},                       ("auto", "bf16_nt", False, "auto", False)),    # the weight casts want 512 rows
    (dict(BF, M=510, N=516, weight_cast=False), {},    ("bf16_nt", "bf16_nt", True, "bf16_nt", False)),
    (dict(BF, M=511), {},                              ("auto", "auto", False, "auto", False)),
    (dict(BF, K=513), {},                              ("h2", "bf16_nt", True, "bf16_nt", True)),     # h2 where the bf16 rule refuses
    (dict(BF, N=513), {},                              ("bf16_nt", "bf16_nt", False, "h2_rows", False)),
    (dict(BF, M=513), {},                              ("bf16_nt", "auto", False, "bf16_nt", False)),
    (dict(BF, need_dx=False), {},                      ("bf16_nt", "bf16_nt", False, None, False)),   # the dual cast of dy: exactly when
    (dict(BF, w_grad=False), {},                       ("bf16_nt", "bf16_nt", False, "bf16_nt", False)),  # dW and dx both read bf16 dy
    (BF, dict(BF16_MIN_MACS=(1 << 27) + 1),            ("h2", "auto", False, "h2_rows", True)),
    (dict(BF, M=64, N=2048, K=1024), dict(BF16_MIN_ROWS=64), ("bf16_nt", "bf16_nt", True, "bf16_nt", False)),
    # a hoisted / plain product, fp32 configuration: the layers' h2 rules, no shared max |x|; dy_contiguous matters here alone
    (HO, {},                                           ("h2", "auto", False, "h2_rows", False)),
    (dict(HO, M=511), {},                              ("auto", "auto", False, "auto", False)),
    (dict(HO, K=256), {},                              ("auto", "auto", False, "h2_rows", False)),
    (dict(HO, N=510), {},                              ("auto", "auto", False, "auto", False)),
    (dict(HO, dy_contiguous=False), {},                ("h2", "auto", False, "auto", False)),
    (dict(HO, w_contiguous=False), {},                 ("h2", "auto", False, "auto", False)),
    (HO, dict(LINEAR_FWD_H2=False),                    ("auto", "auto", False, "h2_rows", False)),
    (HO, dict(LINEAR_DX_H2=False),                     ("h2", "auto", False, "auto", False)),
    # ... bf16 configuration: never h2; the casts from 2^27 MACs, an even reduction length >= 32, whatever the row count; no dual cast
    (HB, {},                                           ("bf16_nt", "bf16_nt", False, "bf16_nt", False)),
    (dict(HB, N=511), {},                              ("auto", "auto", False, "auto", False)),       # below 2^27: generic, not h2
    (dict(HB, K=513), {},                              ("auto", "bf16_nt", False, "bf16_nt", False)), # a layer takes h2 here
    (dict(HB, N=513), {},                              ("bf16_nt", "bf16_nt", False, "auto", False)), # ... and h2_rows here
    (dict(HB, M=256, N=1024), {},                      ("bf16_nt", "bf16_nt", False, "bf16_nt", False)),
    (dict(HB, M=2048, N=4096, K=16), {},               ("auto", "bf16_nt", False, "bf16_nt", False)), # K < 32
    (dict(HB, M=2048, N=4096, K=32), {},               ("bf16_nt", "bf16_nt", False, "bf16_nt", False)),
    (dict(HB, M=4096, N=16, K=2048), {},               ("bf16_nt", "bf16_nt", False, "auto", False)), # dx reduces over N < 32
    (dict(HB, M=16, N=4096, K=2048), {},               ("bf16_nt", "auto", False, "bf16_nt", False)), # dW reduces over M < 32
]
# (M, N, K or None, SKINNY_MIN_ROWS) -> ops._skinny_plan: the narrow route of ops.linear (K None) and the shape rule of a full part
SKINNY = [((2048, 16, None, 2048), True), ((2047, 16, None, 2048), False), ((2048, 17, None, 2048), False), ((64, 8, None, 64), True),
          ((2048, 16, 8, 2048), True), ((2048, 16, 6, 2048), False), ((2047, 16, 8, 2048), False), ((2048, 17, 8, 2048), False)]


def _row_id(row):
    args, knobs, _ = row
    return ",".join("%s=%s" % kv for kv in sorted(args.items()) + sorted(knobs.items()))


@pytest.mark.parametrize("row", TABLE, ids=_row_id)
def test_plan_table(monkeypatch, row):
    args, knobs, want = row
    for k, v in knobs.items():
        assert getattr(ops, k) != v, k
        monkeypatch.setattr(ops, k, v)
    args = dict(args)
    plan = ops._dense_plan(args.pop("M"), args.pop("N"), args.pop("K"), args.pop("bf16", False), **args)
    assert tuple(plan) == want


def test_skinny_plan_table(monkeypatch):
    for (M, N, K, min_rows), want in SKINNY:
        monkeypatch.setattr(ops, "SKINNY_MIN_ROWS", min_rows)
        assert ops._skinny_plan(M, N, K) is want, (M, N, K, min_rows)


def test_the_plan_is_immutable_and_reads_no_library(monkeypatch):
    monkeypatch.setattr(ops._lib, "lib", lambda: pytest.fail("the plan asked the library"))
    plan = ops._dense_plan(512, 512, 512, True)
    ops._skinny_plan(2048, 8, 8)
    with pytest.raises(AttributeError):
        plan.fwd = "auto"


def _dump(obj):
    """The file's text: one distinct call or event per line, one case per line."""
    events = sorted({json.dumps(e, separators=(",", ":")) for log in obj.values() for e in log})
    at = {e: i for i, e in enumerate(events)}
    cases = ['  %s: %s' % (json.dumps(case), json.dumps([at[json.dumps(e, separators=(",", ":"))] for e in log], separators=(",", ":")))
             for case, log in sorted(obj.items())]
    return '{\n "events": [\n  %s\n ],\n "cases": {\n%s\n }\n}\n' % (",\n  ".join(events), ",\n".join(cases))


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_dense_plan_host.py --record"
    recorded = {}
    for case_id in _cases():
        with pytest.MonkeyPatch.context() as mp_:
            recorded[case_id] = _record(mp_, case_id)
    with open(EXPECTED, "w") as f:
        f.write(_dump(recorded))
    print("recorded %d cases" % len(recorded))
