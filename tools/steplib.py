"""What the *_step.py tools share: package and device set-up, device-event and whole-step timing, the random batch, the common
arguments and the leg driver.  A tool is its LEGS table, its flag settings, its row and what only it measures; the method -- every leg
in a fresh child process under `timeout -k 10`, nothing started after a leg that failed, --out rewritten after every leg, every form
warmed up for as long as it is timed, the forms in turn inside every repeat -- lives here.  Nothing here imports torch before a child
asks for the device, so the drivers and --help run without one."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 4716


def setup():
    """The package registered as yt8m_amd and cuda:0 made current.  No device: this raises, nothing falls back."""
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.load_package()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    return dev


def median(v):
    return sorted(v)[len(v) // 2]


def events_us(fn, iters):
    """us per call: hip events around `iters` back-to-back calls."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def alternate(forms, iters, repeats, timer=events_us):
    """forms: name -> callable.  Every form is warmed up for as long as it is timed, then the forms are timed in turn inside every
    repeat (all of them see the same machine).  Returns name -> [us per call of every repeat]."""
    for fn in forms.values():
        timer(fn, iters)
    us = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            us[k].append(timer(fn, iters))
    return us


def spread_fields(prefix, values, unit):
    """The median / min / max of the repeats under the tools' field names: unit "us" for kernel rows, "ms" for step rows."""
    first, digits = {"us": ("_us", 2), "ms": ("_ms_per_step", 3)}[unit]
    return {prefix + first: round(median(values), digits), "%s_%s_min" % (prefix, unit): round(min(values), digits),
            "%s_%s_max" % (prefix, unit): round(max(values), digits)}


def warm_up(step, warmup, check=None):
    """`warmup` steps, check() (the tool's seq_ops.check_persist_errors, where it reads it) after each; the first step's loss."""
    loss_first = None
    for _ in range(warmup):
        o = step()
        if check:
            check()
        if loss_first is None:
            loss_first = float(o["loss"])
    return loss_first


def timed_steps(step, steps, min_seconds=None):
    """Host clock around `steps` steps, device-synchronised at both ends: one such window, or with min_seconds whole windows until
    that long has been timed.  Nothing is read inside a window.  Returns (the last step's output, seconds, steps done)."""
    import torch
    done, elapsed, out = 0, 0.0, None
    while done == 0 if min_seconds is None else elapsed < min_seconds:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        torch.cuda.synchronize()
        elapsed += time.perf_counter() - t0
        done += steps
    return out, elapsed, done


def params_finite(graph):
    import torch
    return all(bool(torch.isfinite(v.data).all()) for v in graph.trainable_variables())


def steps_in_turn(run, forms, steps, repeats):
    """Several forms of a step in ONE process.  run(form, n) makes n steps of a form and ends in a device synchronise (the tool has
    warmed every form up with it); here the forms are timed in turn inside every repeat.  Returns name -> [ms / step of every repeat]."""
    ms = {k: [] for k in forms}
    for _ in range(repeats):
        for k in forms:
            t0 = time.perf_counter()
            run(k, steps)
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
    return ms


def fused_against_composed(ms):
    """fused - composed (medians) against the larger spread either form showed between its own repeats."""
    spread = max(max(ms["fused"]) - min(ms["fused"]), max(ms["composed"]) - min(ms["composed"]))
    diff = median(ms["fused"]) - median(ms["composed"])
    return dict(fused_minus_composed_ms=round(diff, 3), spread_between_repeats_ms=round(spread, 3),
                fused_within_spread_of_composed=bool(diff <= spread))


def random_batch(dev, B, F=None, num_frames="half", first_label=False, D=1152):
    """One random batch from seed 1, drawn in the order x, num_frames, labels: uint8 [B,F,D] frames, or float [B,D] features where F is
    None; num_frames "uniform" in 1..F, "half" in F//2..F, "ends" (uniform, then nf[0], nf[1] = F, 1) or "all" (F, nothing drawn);
    labels at 3.4 / V, with first_label class 0 set in every row.  Returns (x, y, num_frames or None, the generator for further draws)."""
    import torch
    gen = torch.Generator(device=dev).manual_seed(1)
    nf = None
    if F is None:
        x = torch.randn((B, D), device=dev, generator=gen)
    else:
        x = torch.randint(0, 256, (B, F, D), device=dev, generator=gen, dtype=torch.uint8)
        if num_frames == "all":
            nf = torch.full((B,), F, device=dev, dtype=torch.int32)
        else:
            nf = torch.randint(F // 2 if num_frames == "half" else 1, F + 1, (B,), device=dev, generator=gen, dtype=torch.int32)
            if num_frames == "ends":
                nf[0], nf[1] = F, 1
    y = torch.rand((B, V), device=dev, generator=gen) < 3.4 / V
    if first_label:
        y[:, 0] = True
    return x, y, nf, gen


def arg_parser(steps, warmup, timeout):
    """The arguments every tool has, at the tool's defaults; the tool adds its own to the parser."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--timeout", type=int, default=timeout, help="seconds per leg")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("legs", nargs="*")
    return ap


def parse_args(ap, known, argv=None):
    a = ap.parse_args(argv)
    for leg in a.legs + ([a.child] if a.child else []):
        if leg not in known:
            ap.error("unknown leg %r (legs: %s)" % (leg, " ".join(known)))
    return a


def child_args(a, *extras):
    """The command-line tail that hands a driver's arguments on to its children."""
    return [s for name in ("steps", "warmup") + extras for s in ("--" + name, str(getattr(a, name)))]


def repeated_plan(legs, once, repeats):
    """The plan of a tool whose step legs run `repeats` times in turn, their rows numbered by `rep`, after the `once` leg."""
    return [leg for leg in legs if leg == once] + [(leg, {"rep": rep}) for rep in range(repeats) for leg in legs if leg != once]


def numbered(legs, leg, field):
    """The plan of a tool that runs `leg` more than once: its n-th run writes field = n into its rows."""
    runs = iter(range(len(legs)))
    return [(entry, {field: next(runs)}) if entry == leg else entry for entry in legs]


def ms_by_leg(rows):
    by = {}
    for r in rows:
        if "ms_per_step" in r:
            by.setdefault(r["leg"], []).append(r["ms_per_step"])
    return by


def per_leg_medians(rows):
    """A summarise hook: the rows, then a `<leg>_summary` row per step leg over its runs."""
    return rows + [dict(leg=leg + "_summary", ms_per_step_median=median(v), ms_per_step_min=min(v), ms_per_step_max=max(v), runs=len(v))
                   for leg, v in ms_by_leg(rows).items()]


def verdict_after(rows, leg, field, rule):
    """The rows with a `<leg>_summary` row after the last run of a leg that numbered() counts in `field`: whether the fused median
    was below the composed one in every timed row of every run so far."""
    last = max((i for i, r in enumerate(rows) if field in r), default=None)
    if last is None:
        return rows
    timed = [r for r in rows if r.get("leg") == leg]
    summary = {"leg": leg + "_summary", field + "s": rows[last][field] + 1, "rows": len(timed),
               "fused_below_composed_everywhere": bool(all(r["fused_below_composed"] for r in timed)), "rule": rule}
    return rows[:last + 1] + [summary] + rows[last + 1:]


def drive(script, plan, child_args, timeout, out, env_of=None, summarise=None):
    """Runs every leg of the plan as `timeout -k 10 <timeout> python <script> --child <leg> <child_args>` in a fresh child process and
    keeps every line of its output that starts with `{` as a row.  A plan entry is a leg, or (leg, fields to add to its rows).  A leg
    that ends with a non-zero exit status, or without a row, ends the plan: nothing further is started and its status (1 if it was 0)
    is returned.  env_of(leg) -> environment variables of that leg's child.  summarise(rows) -> the rows to record, the tool's summary
    rows put in; --out is rewritten with them after every leg, and the summary rows are printed after the last one."""
    rows, record = [], []
    for entry in plan:
        leg, fields = entry if isinstance(entry, tuple) else (entry, {})
        cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(script), "--child", leg] + list(child_args)
        r = subprocess.run(cmd, env=dict(os.environ, **env_of(leg)) if env_of else None, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print("leg %s failed with exit status %d: stopping" % (leg, r.returncode), flush=True)
            return r.returncode or 1
        for ln in lines:
            rows.append(dict(json.loads(ln), **fields))
            print(json.dumps(rows[-1]), flush=True)
        record = summarise(rows) if summarise else rows
        if out:                                                          # after every leg: a later leg's failure keeps the earlier rows
            with open(out, "w") as f:
                for row in record:
                    f.write(json.dumps(row) + "\n")
    for row in record:
        if all(row is not r for r in rows):
            print(json.dumps(row), flush=True)
    return 0
