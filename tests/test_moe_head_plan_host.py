"""CPU pin of what the MoE classifier head hands to the native library (yt8m_amd/ops.py: moe_head, moe_head_xent): for every form its
three products -- logits, dx, dW -- can take, the ordered library calls of one forward and backward pass with their integer and float
arguments, the yt8m_gemm_problem fields and the operand each pointer is, and the grad_done() events between them.  The head is driven
through its two public ops only, on CPU zero tensors, with the library replaced by the recorder of library_recorder.py and stand-in
variables / graph; the normalised log of every case is compared with tests/golden/moe_head_calls.json, recorded before the head's forms
were chosen in one plan (`python tests/test_moe_head_plan_host.py --record` rewrites that file: only for a change that means to move a
launch).  The cases put every predicate of the choice on both sides: see _cases().

TABLE, further down, is the choice itself: what ops._moe_head_plan -- the one place where the forms are chosen -- answers at the same
edges, as literals."""
import json
import os
import sys

import pytest
import torch

from conftest import ROOT

import yt8m_amd.ops as ops
import yt8m_amd.wimg as wimg
from library_recorder import _Graph, _Var, _normalise, _tagged, install

EXPECTED = os.path.join(ROOT, "tests", "golden", "moe_head_calls.json")
DEFAULT = dict(M=2, bf16=False, need_dx=True, dx_from=0, knobs={}, frozen=(), hook=False, w_noncontig=False, mode="train")
BIG = dict(B=2048, D=2048, V=598, bf16=True)         # 8 x 8 tiles of 256 x 256 over (B, Ng = 1794) and over (D, Ng): the image forms
SMALL = dict(B=512, D=64, V=10)                      # BF16_MIN_ROWS / MOE_LOGITS_H2_MIN_ROWS rows, too few tiles for the image forms


def _cases():
    """id -> the case.  mode: "train" (forward and backward), "no_grad" (forward under torch.no_grad(): the graph's token still asks
    for a gradient, as Graph.begin_step makes it), "inference" (forward with nothing that asks for a gradient, the token included).
    frozen: variables without a gradient slot.  knobs: module knobs of ops flipped for the case."""
    cases = {}

    def add(name, both=("head", "xent"), **kw):
        for op in both:
            cases["%s-%s" % (name, op)] = dict(DEFAULT, op=op, **kw)

    # bf16 configuration: _b1_ok forward over (B, Ng) and K = D, backward over (D, Ng) and K = B; M = 2 against 3; odd Ng / Ne
    for dx in (True, False):
        s = "" if dx else "-nodx"
        add("bf16-images-kept" + s, **dict(BIG, need_dx=dx))                       # forward images keep the other orientation
        add("bf16-images-d256" + s, **dict(BIG, D=256, need_dx=dx))                # (D, Ng): 1 x 8 tiles: plain images, row-major backward
        add("bf16-m3" + s, **dict(BIG, M=3, need_dx=dx))                           # mixing backward in place, then bf16 casts
        add("bf16-m3-odd" + s, **dict(BIG, V=599, M=3, need_dx=dx))                # Ng = 2396, Ne = 1797: no bf16 pairs for dx
    add("bf16-d254", **dict(BIG, D=254))                                           # K = D < 256
    add("bf16-7-tiles", **dict(BIG, V=596))                                        # Ng = 1788: 7 column tiles, 56 < 64
    add("bf16-m2-odd", **dict(BIG, V=599))                                         # M = 2, Ng = 1797 odd: images kept, casts backward
    add("bf16-no-images", **dict(BIG, knobs=dict(B1_IMAGES=False)))
    add("bf16-inference", **dict(BIG, mode="inference"))
    for B in (510, 512, 513):                                                      # BF16_MIN_ROWS, odd rows
        add("bf16-rows%d" % B, **dict(SMALL, B=B, bf16=True))
    add("bf16-odd-d", **dict(SMALL, D=63, bf16=True))
    add("bf16-min-rows-2", B=64, D=64, V=10, bf16=True, knobs=dict(BF16_MIN_ROWS=2))
    # bf16 logits (Z16_LOGITS): V % 4 == 0, 8 column tiles; training needs the image backward and both gradient slots
    Z = dict(BIG, V=600, knobs=dict(Z16_LOGITS=True))
    add("z16-off", **dict(BIG, V=600))
    add("z16-train", **Z)
    add("z16-no-grad", **dict(Z, mode="no_grad"))
    add("z16-inference", **dict(Z, mode="inference"))
    add("z16-frozen-gate", **dict(Z, frozen=("Wg",)))
    add("z16-d256", **dict(Z, D=256))
    add("z16-d256-no-grad", **dict(Z, D=256, mode="no_grad"))
    add("z16-d256-inference", **dict(Z, D=256, mode="inference"))
    add("z16-v598", **dict(Z, V=598))
    # fp32 configuration: MOE_LOGITS_H2_MIN_ROWS for the h2 logits and the h2 dx, D % 4, dx_from, weights that are not contiguous
    for B in (511, 512):
        add("fp32-rows%d" % B, **dict(SMALL, B=B))
        add("fp32-rows%d-nodx" % B, **dict(SMALL, B=B, need_dx=False))
        for k0 in (32, 33, 64, 96):                                                # 33: no 32-row group; 64, 96: not inside D
            add("fp32-rows%d-from%d" % (B, k0), both=("head",), **dict(SMALL, B=B, dx_from=k0))
    add("fp32-d66", **dict(SMALL, D=66))
    add("fp32-m3", **dict(SMALL, M=3, V=11))
    add("fp32-noncontig", **dict(SMALL, w_noncontig=True))
    add("fp32-noncontig-from32", both=("head",), **dict(SMALL, w_noncontig=True, dx_from=32))
    add("fp32-no-grad", **dict(SMALL, mode="no_grad"))
    add("fp32-no-h2-logits", **dict(SMALL, knobs=dict(MOE_LOGITS_H2=False)))
    add("fp32-h2-from-128-rows", **dict(SMALL, B=128, knobs=dict(MOE_LOGITS_H2_MIN_ROWS=128)))
    add("fp32-no-h2-dx", **dict(SMALL, knobs=dict(MOE_DX_H2=False)))
    for B in (511, 512):
        add("fp32-rows%d-no-dx-from" % B, both=("head",), **dict(SMALL, B=B, dx_from=32, knobs=dict(MOE_DX_FROM=False)))
    add("fp32-no-absmax", both=("xent",), **dict(SMALL, knobs=dict(MIX_BWD_ABSMAX=False)))
    add("bf16-m3-no-absmax", both=("xent",), **dict(SMALL, M=3, bf16=True, knobs=dict(MIX_BWD_ABSMAX=False)))
    # the weight-gradient tail of every backward form: missing gradient slots, a grad_ready_hook
    for name, kw in (("fp32", SMALL), ("bf16-rows", dict(SMALL, bf16=True)), ("bf16-casts", dict(SMALL, M=3, bf16=True)), ("bf16-images", BIG)):
        add(name + "-frozen-gate", **dict(kw, frozen=("Wg",)))
        add(name + "-frozen-gate-bias", **dict(kw, frozen=("Wg", "be")))
        add(name + "-hook", **dict(kw, hook=True))
    return cases


def _record(mp, case):
    """The normalised log of one case: the library calls and grad_done() events of a forward and (mode "train") a backward pass of the
    case's op."""
    c = _cases()[case]
    for k, v in c["knobs"].items():
        assert getattr(ops, k) != v, k                                    # flipped from its default
        mp.setattr(ops, k, v)
    r = install(mp, plain=_tagged)
    mp.setattr(wimg, "BUFFERS", {})                                       # no resident weight images, whatever ran in this process before
    B, D, V, M = c["B"], c["D"], c["V"], c["M"]
    Ng, Ne = V * (M + 1), V * M
    g = _Graph((lambda v: None) if c["hook"] else None, c["mode"] != "inference")
    wide = lambda n: torch.zeros(n, D).t() if c["w_noncontig"] else torch.zeros(D, n)
    Wg = _Var("Wg", wide(Ng), g, r.log, "Wg" in c["frozen"])
    We = _Var("We", wide(Ne), g, r.log, "We" in c["frozen"])
    be = _Var("be", torch.zeros(Ne), g, r.log, "be" in c["frozen"])
    x = torch.zeros(B, D, requires_grad=c["need_dx"] and c["mode"] != "inference")
    named = {"x": x, "Wg": Wg.data, "We": We.data, "be": be.data, "ws": r.ws}
    named.update({v.name + ".grad": v.grad for v in (Wg, We, be) if v.grad is not None})
    with torch.set_grad_enabled(c["mode"] != "no_grad"):
        if c["op"] == "head":
            out = ops.moe_head(x, Wg, We, be, V, M, bf16=c["bf16"], dx_from=c["dx_from"])
            up = torch.zeros(B, V)
        else:
            assert c["dx_from"] == 0
            _, out = ops.moe_head_xent(x, Wg, We, be, torch.zeros(B, V, dtype=torch.uint8), V, M, bf16=c["bf16"])
            up = torch.ones(())
    if c["mode"] == "train":
        r.log.append(("yt8m_backward", []))
        out.backward(up)
        assert (x.grad is not None) == c["need_dx"]
    return _normalise(r.log, named)


def _expected():
    """case -> its recorded log.  The file holds every distinct call or event once ("events", one per line) and each case as indices."""
    with open(EXPECTED) as f:
        rec = json.load(f)
    return {case: [rec["events"][i] for i in log] for case, log in rec["cases"].items()}


def test_the_cases_are_the_recorded_ones_and_reach_every_entry_point_of_the_head():
    want = _expected()
    assert sorted(_cases()) == sorted(want)
    for op in ("head", "xent"):
        seen = {e[0] for case, log in want.items() if case.endswith("-" + op) for e in log}
        assert {"gemm_b1_nt_grouped", "gemm_bf16_nt_grouped", "gemm_auto_grouped", "gemm_auto_grouped_ex",
                "gemm_h2_nt_ex", "h2_absmax", "bf16_image", "cast_f32_bf16", "cast_f32_bf16_dual",
                "moe_mix_bwd_bf16", "moe_mix_bwd_bf16_images", "colsum_f32", "grad_done"} <= seen, op
    seen = {e[0] for log in want.values() for e in log}
    assert {"moe_mix_fwd", "moe_mix_fwd_bf16z", "moe_mix_bwd", "gemm_b1_nt_grouped_bf16c", "moe_mix_bwd_bf16_images_z16",
            "moe_mix_xent_fwd", "moe_mix_xent_bwd", "moe_mix_xent_bwd_absmax"} <= seen


@pytest.mark.parametrize("case", sorted(_cases()))
def test_library_calls_of_a_forward_and_backward_pass(monkeypatch, case):
    want = _expected()[case]
    got = json.loads(json.dumps(_record(monkeypatch, case)))              # tuples and floats as the file holds them
    assert got == want


# ---- the table itself: the plan function at the same edges ---------------------------------------------------------------------------
def _plan(B, D, V, M=2, bf16=False, training=True, need_dx=True, **kw):
    return ops._moe_head_plan(B, D, V * (M + 1), V * M, V, M, bf16, training, need_dx, **kw)


INFER = dict(training=False, need_dx=False)
Z16 = dict(BIG, V=600, z16_allowed=True)
ON = dict(Z16_LOGITS=True)
# (arguments of _plan, knobs flipped) -> (logits, z16, backward, dx_bf16, dx, k0, absmax).  A change of a threshold or of a rule shows here.
TABLE = [
    # bf16 configuration: 64 tiles of 256 x 256 over (B, Ng) with K = D >= 256 forward, over (D, Ng) with K = B backward
    (BIG, {},                                          ("b1_keep", False, "fused_images", False, None, 0, False)),
    (dict(BIG, need_dx=False), {},                     ("b1_keep", False, "fused_images", False, None, 0, False)),
    (dict(BIG, dx_from=32), {},                        ("b1_keep", False, "fused_images", False, None, 0, False)),
    (dict(BIG, D=256), {},                             ("b1", False, "fused_rows", False, None, 0, False)),
    (dict(BIG, D=254), {},                             ("bf16_nt", False, "fused_rows", False, None, 0, False)),
    (dict(BIG, V=596), {},                             ("bf16_nt", False, "fused_rows", False, None, 0, False)),     # 7 column tiles
    (dict(BIG, M=3), {},                               ("b1", False, "casts", True, None, 0, True)),
    (dict(BIG, M=3, need_dx=False), {},                ("b1", False, "casts", False, None, 0, True)),
    (dict(BIG, M=3, V=599), {},                        ("b1", False, "casts", False, None, 0, True)),                # Ne = 1797
    (dict(BIG, V=599), {},                             ("b1_keep", False, "casts", False, None, 0, True)),           # Ng = 1797
    (dict(BIG, **INFER), {},                           ("b1", False, None, False, None, 0, False)),
    (BIG, dict(B1_IMAGES=False),                       ("bf16_nt", False, "fused_rows", False, None, 0, False)),
    (dict(BIG, M=3), dict(MIX_BWD_ABSMAX=False),       ("b1", False, "casts", True, None, 0, False)),
    # BF16_MIN_ROWS = 512 even rows, D even; below that the fp32 forms
    (dict(SMALL, B=510, bf16=True), {},                ("fp32", False, "fp32", False, "plain", 0, True)),
    (dict(SMALL, B=512, bf16=True), {},                ("bf16_nt", False, "fused_rows", False, None, 0, False)),
    (dict(SMALL, B=513, bf16=True), {},                ("h2", False, "fp32", False, "h2_rows", 0, True)),
    (dict(SMALL, D=63, bf16=True), {},                 ("h2", False, "fp32", False, "plain", 0, True)),
    (dict(SMALL, B=64, bf16=True), dict(BF16_MIN_ROWS=2), ("bf16_nt", False, "fused_rows", False, None, 0, False)),
    # bf16 logits: the knob, V % 4 == 0, an op that reads them, and the image backward into both gradient slots when one follows
    (Z16, {},                                          ("b1_keep", False, "fused_images", False, None, 0, False)),
    (Z16, ON,                                          ("b1_keep", True, "fused_images", False, None, 0, False)),
    (dict(Z16, **INFER), ON,                           ("b1", True, None, False, None, 0, False)),
    (dict(Z16, grad_slots=False), ON,                  ("b1_keep", False, "fused_images", False, None, 0, False)),
    (dict(Z16, D=256), ON,                             ("b1", False, "fused_rows", False, None, 0, False)),
    (dict(Z16, D=256, **INFER), ON,                    ("b1", True, None, False, None, 0, False)),
    (dict(Z16, V=598), ON,                             ("b1_keep", False, "fused_images", False, None, 0, False)),
    (dict(Z16, z16_allowed=False), ON,                 ("b1_keep", False, "fused_images", False, None, 0, False)),
    # fp32 configuration: MOE_LOGITS_H2_MIN_ROWS = 512 rows for the h2 logits and the h2 dx, D % 4, contiguous weights, dx_from
    (dict(SMALL, B=511), {},                           ("fp32", False, "fp32", False, "plain", 0, True)),
    (SMALL, {},                                        ("h2", False, "fp32", False, "h2_rows", 0, True)),
    (dict(SMALL, need_dx=False), {},                   ("h2", False, "fp32", False, None, 0, True)),
    (dict(SMALL, **INFER), {},                         ("h2", False, None, False, None, 0, False)),
    (dict(SMALL, M=3, V=11), {},                       ("h2", False, "fp32", False, "h2_rows", 0, True)),
    (dict(SMALL, D=66), {},                            ("h2", False, "fp32", False, "plain", 0, True)),
    (dict(SMALL, w_contiguous=False), {},              ("h2", False, "fp32", False, "plain", 0, True)),
    (dict(SMALL, w_contiguous=False, dx_from=32), {},  ("h2", False, "fp32", False, "window", 32, True)),
    (dict(SMALL, B=511, dx_from=32), {},               ("fp32", False, "fp32", False, "window", 32, True)),
    (dict(SMALL, B=511, dx_from=33), {},               ("fp32", False, "fp32", False, "plain", 0, True)),
    (dict(SMALL, B=511, dx_from=64), {},               ("fp32", False, "fp32", False, "plain", 0, True)),
    (dict(SMALL, dx_from=32), {},                      ("h2", False, "fp32", False, "h2_rows", 32, True)),
    (dict(SMALL, dx_from=33), {},                      ("h2", False, "fp32", False, "h2_rows", 0, True)),
    (dict(SMALL, dx_from=64), {},                      ("h2", False, "fp32", False, "h2_rows", 0, True)),
    (dict(SMALL, dx_from=96), {},                      ("h2", False, "fp32", False, "h2_rows", 0, True)),
    (dict(SMALL, dx_from=32, need_dx=False), {},       ("h2", False, "fp32", False, None, 0, True)),
    (SMALL, dict(MOE_LOGITS_H2=False),                 ("fp32", False, "fp32", False, "h2_rows", 0, True)),
    (dict(SMALL, B=128), dict(MOE_LOGITS_H2_MIN_ROWS=128), ("h2", False, "fp32", False, "h2_rows", 0, True)),
    (SMALL, dict(MOE_DX_H2=False),                     ("h2", False, "fp32", False, "plain", 0, True)),
    (dict(SMALL, dx_from=32), dict(MOE_DX_H2=False),   ("h2", False, "fp32", False, "window", 32, True)),
    (dict(SMALL, dx_from=32), dict(MOE_DX_FROM=False), ("h2", False, "fp32", False, "h2_rows", 0, True)),
    (dict(SMALL, B=511, dx_from=32), dict(MOE_DX_FROM=False), ("fp32", False, "fp32", False, "plain", 0, True)),
    (SMALL, dict(MIX_BWD_ABSMAX=False),                ("h2", False, "fp32", False, "h2_rows", 0, False)),
]


def _row_id(row):
    args, knobs, _ = row
    return ",".join("%s=%s" % kv for kv in sorted(args.items()) + sorted(knobs.items()))


@pytest.mark.parametrize("row", TABLE, ids=_row_id)
def test_plan_table(monkeypatch, row):
    args, knobs, want = row
    for k, v in knobs.items():
        assert getattr(ops, k) != v, k
        monkeypatch.setattr(ops, k, v)
    plan = _plan(**args)
    assert (plan.logits, plan.z16, plan.backward, plan.dx_bf16, plan.dx, plan.k0, plan.absmax) == want
    assert plan.need_dx == args.get("need_dx", True)


def test_plan_refuses_bf16_logits_without_the_image_backward(monkeypatch):
    """The plan function derives z16 from the backward form it chose, so it cannot pair bf16 logits with a pass that reads fp32 ones; a plan
    put together any other way is refused where it is built."""
    monkeypatch.setattr(ops, "Z16_LOGITS", True)
    plan = _plan(**Z16)
    assert plan.z16 and plan.backward == "fused_images"
    for backward in ("fused_rows", "casts", "fp32"):
        with pytest.raises(AssertionError, match="bf16 logits"):
            ops._HeadPlan(**dict(plan._asdict(), backward=backward))
    ops._HeadPlan(**dict(plan._asdict(), backward=None))                   # no backward pass follows: nothing reads fp32 logits


def _dump(obj):
    """The file's text: one distinct call or event per line, one case per line."""
    events =sorted({json.dumps(e, separators=(",", ":")) for log in obj.values() for e in log})
    at = {e: i for i, e in enumerate(events)}
    cases = ['  %s: %s' % (json.dumps(case), json.dumps([at[json.dumps(e, separators=(",", ":"))] for e in log], separators=(",", ":")))
             for case, log in sorted(obj.items())]
    return '{\n "events": [\n  %s\n ],\n "cases": {\n%s\n }\n}\n' % (",\n  ".join(events), ",\n".join(cases))


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_moe_head_plan_host.py --record"
    recorded = {}
    for case_id in _cases():
        with pytest.MonkeyPatch.context() as mp_:
            recorded[case_id] = _record(mp_, case_id)
    with open(EXPECTED, "w") as f:
        f.write(_dump(recorded))
    print("recorded %d cases" % len(recorded))
