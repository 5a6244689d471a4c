"""tools/steplib.py on the host: the leg driver against a stand-in child script, the timing helpers with counting stand-ins, and the
common arguments of the nine *_step.py tools against the defaults each tool had before they shared them.  No device is touched."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")

# the stand-in child: records its leg and its parent's command line, then does what the leg's name says
CHILD = r'''
import json, os, sys, time
leg = sys.argv[sys.argv.index("--child") + 1]
here = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(here, "started.txt"), "a") as f:
    f.write(leg + "\n")
with open("/proc/%d/cmdline" % os.getppid()) as f:
    parent = f.read().split("\0")
with open(os.path.join(here, "parent_cmd.json"), "w") as f:
    json.dump(parent, f)
print("not a row")
if leg == "fail":
    print(json.dumps(dict(leg=leg, n=0)))
    sys.exit(3)
if leg == "sleep":
    time.sleep(30)
if leg == "silent":
    sys.exit(0)
for n in range(2 if leg == "two" else 1):
    print(json.dumps(dict(leg=leg, n=n, env=os.environ.get("STEPLIB_TEST_ENV"), tail=sys.argv[sys.argv.index("--child") + 2:])))
'''


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.path.insert(0, TOOLS)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(TOOLS)
    return mod


steplib = _load("steplib")


@pytest.fixture
def stand_in(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    started = lambda: (tmp_path / "started.txt").read_text().split()
    out_rows = lambda: [json.loads(ln) for ln in (tmp_path / "out.jsonl").read_text().splitlines()]
    return str(script), str(tmp_path / "out.jsonl"), started, out_rows


def test_drive_keeps_every_row_of_every_leg_in_order(stand_in, capsys):
    script, out, started, out_rows = stand_in
    status = steplib.drive(script, ["one", "two", ("one", {"rep": 1})], ["--steps", "2"], 30, out,
                           env_of=lambda leg: {"STEPLIB_TEST_ENV": "of_" + leg},
                           summarise=lambda rows: rows[:1] + [dict(leg="summary", rows=len(rows))] + rows[1:])
    assert status == 0
    assert started() == ["one", "two", "one"]
    rows = out_rows()
    assert [(r["leg"], r.get("n")) for r in rows] == [("one", 0), ("summary", None), ("two", 0), ("two", 1), ("one", 0)]
    assert rows[1] == dict(leg="summary", rows=4)
    assert [r.get("rep") for r in rows] == [None, None, None, None, 1]
    assert [r["env"] for r in rows if "env" in r] == ["of_one", "of_two", "of_two", "of_one"]
    assert all(r["tail"] == ["--steps", "2"] for r in rows if "tail" in r)
    printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert printed == rows[:1] + rows[2:] + rows[1:2]                       # the legs' rows as they come, the summary row after the last leg


def test_drive_command_line_begins_with_the_time_limit(stand_in):
    script, out, started, out_rows = stand_in
    assert steplib.drive(script, ["one"], [], 17, out) == 0
    with open(os.path.join(os.path.dirname(script), "parent_cmd.json")) as f:
        parent = json.load(f)
    assert parent[:4] == ["timeout", "-k", "10", "17"]
    assert parent[4:8] == [sys.executable, script, "--child", "one"]


def test_drive_stops_at_the_first_failing_leg(stand_in, capsys):
    script, out, started, out_rows = stand_in
    assert steplib.drive(script, ["one", "two", "fail", "one"], [], 30, out) == 3
    assert started() == ["one", "two", "fail"]                              # the leg after the failure was never started
    assert [(r["leg"], r["n"]) for r in out_rows()] == [("one", 0), ("two", 0), ("two", 1)]
    assert "leg fail failed with exit status 3: stopping" in capsys.readouterr().out


def test_drive_treats_a_leg_without_a_row_as_failed(stand_in):
    script, out, started, out_rows = stand_in
    assert steplib.drive(script, ["one", "silent", "one"], [], 30, out) == 1
    assert started() == ["one", "silent"]
    assert [r["leg"] for r in out_rows()] == ["one"]


def test_drive_time_limit_ends_a_leg_and_the_plan(stand_in):
    script, out, started, out_rows = stand_in
    assert steplib.drive(script, ["one", "sleep", "one"], [], 1, out) == 124
    assert started() == ["one", "sleep"]
    assert [r["leg"] for r in out_rows()] == ["one"]


def test_median_is_the_upper_middle():
    for v in ([3.0, 1.0, 2.0], [4.0, 1.0, 3.0, 2.0], [5.0], [2.0, 1.0]):
        assert steplib.median(v) == sorted(v)[len(v) // 2]
    assert steplib.median([4.0, 1.0, 3.0, 2.0]) == 3.0


def test_spread_fields_names_and_rounding():
    us = steplib.spread_fields("fused", [3.14159, 1.006, 2.5], "us")
    assert list(us) == ["fused_us", "fused_us_min", "fused_us_max"]
    assert us == dict(fused_us=2.5, fused_us_min=1.01, fused_us_max=3.14)
    ms = steplib.spread_fields("fused", [3.14159, 1.0006, 2.5], "ms")
    assert list(ms) == ["fused_ms_per_step", "fused_ms_min", "fused_ms_max"]
    assert ms == dict(fused_ms_per_step=2.5, fused_ms_min=1.001, fused_ms_max=3.142)


def test_fused_against_composed_verdict():
    # fused 0.3 above composed; composed alone spreads 0.5 between its repeats: within
    within = steplib.fused_against_composed(dict(fused=[10.3, 10.3, 10.3], composed=[9.8, 10.0, 10.3]))
    assert within == dict(fused_minus_composed_ms=0.3, spread_between_repeats_ms=0.5, fused_within_spread_of_composed=True)
    # the same medians with repeats that agree to 0.1: beyond
    beyond = steplib.fused_against_composed(dict(fused=[10.3, 10.3, 10.4], composed=[10.0, 10.0, 10.1]))
    assert list(beyond) == ["fused_minus_composed_ms", "spread_between_repeats_ms", "fused_within_spread_of_composed"]
    assert beyond["fused_minus_composed_ms"] == 0.3 and beyond["spread_between_repeats_ms"] == 0.1
    assert beyond["fused_within_spread_of_composed"] is False
    # a faster fused form is within whatever the spread
    assert steplib.fused_against_composed(dict(fused=[9.0, 9.0], composed=[10.0, 10.0]))["fused_within_spread_of_composed"] is True


def test_alternate_warms_every_form_then_times_them_in_turn():
    calls = []
    forms = {"fused": lambda: calls.append("fused"), "composed": lambda: calls.append("composed"), "other": lambda: calls.append("other")}
    timed = []

    def timer(fn, iters):
        for _ in range(iters):
            fn()
        timed.append((calls[-1], iters))
        return float(len(timed))

    us = steplib.alternate(forms, 2, 3, timer=timer)
    names = list(forms)
    assert [t[0] for t in timed] == names + names * 3                       # every form once before any is timed, then in turn per repeat
    assert all(iters == 2 for _, iters in timed)                            # warmed up for as long as it is timed
    assert us == {"fused": [4.0, 7.0, 10.0], "composed": [5.0, 8.0, 11.0], "other": [6.0, 9.0, 12.0]}   # the warm-up times are dropped
    assert calls == [n for n in names for _ in range(2)] * 4


def test_steps_in_turn_visits_the_forms_in_turn_inside_every_repeat():
    seen = []
    ms = steplib.steps_in_turn(lambda form, n: seen.append((form, n)), {"fused": 1, "composed": 2, "parent": 3}, 4, 2)
    assert seen == [("fused", 4), ("composed", 4), ("parent", 4)] * 2
    assert list(ms) == ["fused", "composed", "parent"] and all(len(v) == 2 and min(v) >= 0.0 for v in ms.values())


def test_warm_up_checks_after_every_step_and_returns_the_first_loss():
    log = []
    losses = iter([4.0, 3.0, 2.0])

    def step():
        log.append("step")
        return {"loss": next(losses)}

    assert steplib.warm_up(step, 3, check=lambda: log.append("check")) == 4.0
    assert log == ["step", "check"] * 3
    assert steplib.warm_up(step, 0) is None


def test_plans_number_the_runs_of_a_leg():
    assert steplib.numbered(["link", "chain", "link"], "link", "leg_repeat") == [("link", {"leg_repeat": 0}), "chain", ("link", {"leg_repeat": 1})]
    assert steplib.repeated_plan(["a", "kernels", "b"], "kernels", 2) == ["kernels", ("a", {"rep": 0}), ("b", {"rep": 0}), ("a", {"rep": 1}),
                                                                           ("b", {"rep": 1})]
    assert steplib.repeated_plan(["a"], "kernels", 1) == [("a", {"rep": 0})]


def test_summary_hooks_place_their_rows():
    link = lambda n, below: dict(leg="link", fused_below_composed=below, leg_repeat=n)
    device = lambda n: dict(leg="device", leg_repeat=n)
    chain = dict(leg="chain", fused_ms_per_step=1.0)
    summary = lambda runs, rows, verdict: dict(leg="link_summary", leg_repeats=runs, rows=rows, fused_below_composed_everywhere=verdict, rule="r")
    hook = lambda rows: steplib.verdict_after(rows, "link", "leg_repeat", "r")
    assert hook([chain]) == [chain]
    first = [link(0, True), link(0, True), device(0)]
    assert hook(first) == first + [summary(1, 2, True)]
    second = first + [link(1, False), device(1)]
    assert hook(second + [chain]) == second + [summary(2, 3, False), chain]            # after the last run of the leg, before the later legs
    assert list(hook(first)[-1]) == ["leg", "leg_repeats", "rows", "fused_below_composed_everywhere", "rule"]
    rows = [dict(leg="kernel"), dict(leg="a", ms_per_step=3.0), dict(leg="b", ms_per_step=5.0), dict(leg="a", ms_per_step=1.0)]
    assert steplib.per_leg_medians(rows) == rows + [
        dict(leg="a_summary", ms_per_step_median=3.0, ms_per_step_min=1.0, ms_per_step_max=3.0, runs=2),
        dict(leg="b_summary", ms_per_step_median=5.0, ms_per_step_min=5.0, ms_per_step_max=5.0, runs=1)]


# steps, warmup, timeout and the tool's own arguments, as each tool had them before steplib
DEFAULTS = {
    "bilstm_step": dict(steps=20, warmup=3, timeout=300),
    "augment_step": dict(steps=20, warmup=3, timeout=300),
    "multiscale_step": dict(steps=10, warmup=3, timeout=300, min_seconds=1.0),
    "resolution_step": dict(steps=20, warmup=3, timeout=300, repeats=3, kernel_iters=50),
    "lstmcnn_step": dict(steps=10, warmup=3, timeout=300, min_seconds=1.0),
    "distillchain_step": dict(steps=20, warmup=3, timeout=420, repeats=5, kernel_iters=200),
    "multilstm_step": dict(steps=10, warmup=3, timeout=420, repeats=5, link_iters=200),
    "temporal_pool_step": dict(steps=5, warmup=2, timeout=420, repeats=5, pyramid_iters=50),
    "label_loss_step": dict(steps=50, warmup=5, timeout=300, repeats=5, kernel_iters=100),
}
# the legs a tool runs when none is named, in order
DEFAULT_PLANS = {
    "bilstm_step": ["lstm", "bilstm_seq", "bilstm_overlap", "biuni"],
    "augment_step": ["lstm_half", "lstm_tiled", "cnn_half", "cnn_tiled", "attn_half", "attn_tiled", "chain_halfvideo", "chain_tiled", "kernels"],
    "multiscale_step": ["fused", "generic", "fused", "generic", "lstm", "kernels"],
    "resolution_step": ["kernels"] + ["lstmmem_resolution_fused", "lstmmem_resolution_composed", "lstmmem_default"] * 3,
    "lstmcnn_step": ["pooled", "composed", "pooled", "composed", "pooled_chain", "parallel", "kernels"],
    "distillchain_step": ["kernels", "video", "parallel", "cnn", "attention"],
    "multilstm_step": ["link", "link", "chain", "distill", "parallel"],
    "temporal_pool_step": ["pyramid", "pyramid", "multires", "framehop"],
    "label_loss_step": ["kernels"] + ["moe_batch_agreement", "moe_topk_batch_agreement", "moe_cross_entropy_unfused"] * 5,
}


@pytest.mark.parametrize("tool", sorted(DEFAULTS))
def test_tool_defaults_and_default_plan(tool, monkeypatch):
    mod = _load(tool)
    a = mod.parser().parse_args([])
    expected = dict(DEFAULTS[tool], out=None, child=None, legs=[])
    assert vars(a) == expected
    plans = []
    monkeypatch.setattr(mod.steplib, "drive", lambda script, plan, *args, **kw: plans.append((script, list(plan), args[1])) or 0)
    monkeypatch.setattr(sys, "argv", [tool + ".py"])
    assert mod.main() == 0
    (script, plan, timeout), = plans
    assert os.path.samefile(script, os.path.join(TOOLS, tool + ".py"))
    assert [p[0] if isinstance(p, tuple) else p for p in plan] == DEFAULT_PLANS[tool]
    assert timeout == DEFAULTS[tool]["timeout"]


def test_unknown_legs_are_rejected(capsys):
    ap = steplib.arg_parser(20, 3, 300)
    assert steplib.parse_args(ap, ["a", "b"], ["b", "a"]).legs == ["b", "a"]
    for argv in (["a", "c"], ["--child", "c"]):
        with pytest.raises(SystemExit) as e:
            steplib.parse_args(ap, ["a", "b"], argv)
        assert e.value.code == 2
        assert "unknown leg 'c' (legs: a b)" in capsys.readouterr().err


def test_child_args_hand_the_arguments_on():
    ap = steplib.arg_parser(20, 3, 300)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args(["--steps", "7"])
    assert steplib.child_args(a, "repeats") == ["--steps", "7", "--warmup", "3", "--repeats", "5"]


@pytest.mark.parametrize("tool", sorted(DEFAULTS))
def test_tool_prints_help_without_a_device(tool):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, tool + ".py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr
    assert "--steps" in r.stdout and "--timeout" in r.stdout and "--out" in r.stdout
