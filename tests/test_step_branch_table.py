"""Not -m gpu: keeps the branch table of tests/test_gpu_step_branches.py honest.

Every __global__ kernel of csrc/sequence.hip, csrc/lstm_fused.hip, csrc/lstm_bf16.hip and csrc/cells.hip is either in the list recorded
from a profiled run of that module (tests/golden/step_kernels_seen.txt; call counts per instantiation in
profiles/step_branches_kernel_stats.csv, both written by tools/step_kernel_list.py) or in EXCLUDED below with the test that covers it;
every kernel the table names exists in the sources and was seen, every instantiation it names was called; every extern "C" function of
lstm_fused.hip, lstm_bf16.hip and cells.hip and every yt8m_lstm_* function of sequence.hip has a row.  A kernel or an entry point added
to these files fails here until a branch case reaches it and the list is recorded again."""
import csv
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "youtube-8m_amd", "csrc")
SOURCES = ["sequence.hip", "lstm_fused.hip", "lstm_bf16.hip", "cells.hip"]
SEEN = os.path.join(ROOT, "tests", "golden", "step_kernels_seen.txt")
STATS = os.path.join(ROOT, "profiles", "step_branches_kernel_stats.csv")
N_ROWS = 56

# kernels of sequence.hip that belong to the streaming module's table or exclusions: the test that holds each
EXCLUDED = {
    "attn_softmax_fwd_kernel": "tests/test_streaming_branch_table.py::test_every_streaming_kernel_is_reached_or_excluded_by_name (the streaming table)",
    "attn_softmax_bwd_kernel": "tests/test_streaming_branch_table.py::test_every_streaming_kernel_is_reached_or_excluded_by_name (the streaming table)",
    "softmax_rows_fwd_kernel": "tests/test_streaming_branch_table.py::test_every_streaming_kernel_is_reached_or_excluded_by_name (the streaming table)",
    "softmax_rows_bwd_kernel": "tests/test_streaming_branch_table.py::test_every_streaming_kernel_is_reached_or_excluded_by_name (the streaming table)",
    "topk_rows_kernel": "tests/test_streaming_branch_table.py::test_every_streaming_kernel_is_reached_or_excluded_by_name (the streaming table)",
    "perr_rows_kernel": "tests/test_streaming_branch_table.py::test_every_streaming_kernel_is_reached_or_excluded_by_name (the streaming table)",
    "reverse_u8_kernel": "tests/test_streaming_branch_table.py::test_every_streaming_kernel_is_reached_or_excluded_by_name (the streaming table)",
    "reverse_f32_tm_kernel": "tests/test_streaming_branch_table.py::test_every_streaming_kernel_is_reached_or_excluded_by_name (the streaming table)",
}

# instantiations the table names that only the children of the branch module launch (YT8M_STEP_MODE is read once per process): modes
# 0, 1 and 3 of each class, and mode 2 where the default ("2122") is 1.  The profiler's record of the parent need not hold them.
_CHILD = "tests/test_gpu_step_branches.py::test_step_mode_and_switch_children"
STEP_CHILD = {}
for _g, _ep, _modes in ((4, 0, (0, 1, 3)), (4, 1, (0, 1, 3)), (2, 2, (0, 2, 3)), (1, 3, (0, 2, 3))):
    for _m in _modes:
        STEP_CHILD["lstm_step_fwd_kernel<%d, %d, %d>" % (_g, _ep, _m)] = _CHILD
for _bep in (0, 1, 2):
    for _m in (0, 1, 3):
        STEP_CHILD["lstm_step_bwd_kernel<%d, %d>" % (_bep, _m)] = _CHILD

# what the recorded run must show: the default-mode instantiations, the three PT of the row kernels, both bf16 backward forms
DEFAULT_RUN = ["lstm_step_fwd_kernel<4, 0, 2>", "lstm_step_fwd_kernel<4, 1, 2>", "lstm_step_fwd_kernel<2, 2, 1>", "lstm_step_fwd_kernel<1, 3, 1>",
               "lstm_step_bwd_kernel<0, 2>", "lstm_step_bwd_kernel<2, 2>", "lstm_step_bwd_kernel<1, 2>",
               "lnlstm_fwd_kernel<2>", "lnlstm_fwd_kernel<4>", "lnlstm_fwd_kernel<8>", "lnlstm_bwd_kernel<2>", "lnlstm_bwd_kernel<4>",
               "lnlstm_bwd_kernel<8>", "lstm_step_bwd16_kernel<true>", "lstm_step_bwd16_kernel<false>"]


def source_text(csrc=CSRC, files=SOURCES):
    return "\n".join(open(os.path.join(csrc, f)).read() for f in files)


def source_kernels(csrc=CSRC):
    return set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", source_text(csrc)))


def source_entry_points(csrc=CSRC):
    """every extern "C" function of lstm_fused.hip, lstm_bf16.hip and cells.hip, and the yt8m_lstm_* ones of sequence.hip"""
    pat = r'extern\s+"C"\s+[\w\s\*]*?\b(yt8m_\w+)\s*\('
    own = set(re.findall(pat, source_text(csrc, SOURCES[1:])))
    return own | {e for e in re.findall(pat, source_text(csrc, SOURCES[:1])) if e.startswith("yt8m_lstm_")}


def seen_kernels(path=SEEN):
    return {l.strip() for l in open(path) if l.strip()}


def branch_table(path=None):
    spec = importlib.util.spec_from_file_location("_step_branches", path or os.path.join(ROOT, "tests", "test_gpu_step_branches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.BRANCH_TABLE


def table_kernels(rows):
    """(base name, instantiation or None, left out) for every kernel a table row names."""
    out = []
    for row in rows:
        for base, targs in re.findall(r"(\w+_kernel)(<[^>]*>)?", row[2]):
            out.append((base, base + targs if targs else None, row[3].startswith("left out:")))
    return out


def uncovered(csrc=CSRC, seen_path=SEEN):
    return sorted(source_kernels(csrc) - seen_kernels(seen_path) - set(EXCLUDED))


def table_problems(rows, csrc=CSRC, seen_path=SEEN, stats_path=STATS):
    """Every way the table disagrees with the sources and the recorded run, as a list of sentences."""
    src, seen = source_kernels(csrc), seen_kernels(seen_path)
    calls = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(stats_path))}
    bad = []
    for base, inst, left_out in table_kernels(rows):
        if base not in src:
            bad.append("the table names %s, which is not in the sources" % base)
        elif base in EXCLUDED or left_out:
            continue
        elif base not in seen:
            bad.append("the table names %s, which the recorded run never launched" % base)
        elif inst and inst not in STEP_CHILD and calls.get(inst, 0) < 1:
            bad.append("instantiation %s was never called in the recorded run" % inst)
    named = {inst for _, inst, _ in table_kernels(rows) if inst} | {base for base, inst, _ in table_kernels(rows) if not inst}
    for k in sorted(src - set(EXCLUDED)):
        if not any(n == k or n.startswith(k + "<") for n in named):
            bad.append("kernel %s has no row" % k)
    for inst in sorted(set(DEFAULT_RUN) | set(STEP_CHILD)):
        if inst not in named:
            bad.append("instantiation %s has no row" % inst)
    for e in sorted(source_entry_points(csrc) - {r[0] for r in rows}):
        bad.append("entry point %s has no row" % e)
    for e in sorted({r[0] for r in rows} - source_entry_points(csrc)):
        bad.append("the table names entry point %s, which is not in the sources" % e)
    return bad


def _test_exists(where):
    path, test = where.split(" ")[0].split("::")
    return re.search(r"^def %s\(" % test, open(os.path.join(ROOT, path)).read(), re.M) is not None


def test_every_step_kernel_is_reached_or_excluded_by_name():
    src = source_kernels()
    assert len(src) >= 23
    assert {"lstm_gates_fwd_kernel", "lstm_gates_bwd_kernel"} <= seen_kernels()          # excluded by the streaming table: seen here
    assert not uncovered(), "kernels no branch case reaches (add the case and its table row, then record the list again): %s" % uncovered()
    assert not set(EXCLUDED) - src, "stale exclusions: %s" % sorted(set(EXCLUDED) - src)
    assert not set(EXCLUDED) & seen_kernels(), "excluded although seen: %s" % sorted(set(EXCLUDED) & seen_kernels())
    for where in list(EXCLUDED.values()) + list(STEP_CHILD.values()):
        assert _test_exists(where), where
    # the exclusions are the streaming module's: each is in its table or its own exclusions
    spec = importlib.util.spec_from_file_location("_streaming_table", os.path.join(ROOT, "tests", "test_streaming_branch_table.py"))
    st = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(st)
    held = st.seen_kernels() | set(st.EXCLUDED)
    assert set(EXCLUDED) <= held, sorted(set(EXCLUDED) - held)


def test_every_kernel_of_the_branch_table_exists_and_was_called():
    rows = branch_table()
    assert all(len(r) == 4 and all(isinstance(x, str) and x for x in r) for r in rows)
    # one row per arm, as read from the dispatchers when the run was recorded: a row that goes (or comes) changes this number with it
    assert len(rows) == N_ROWS and len(set(rows)) == N_ROWS, len(rows)
    assert len(table_kernels(rows)) > 60
    assert not table_problems(rows), "\n".join(table_problems(rows))
    calls = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(STATS))}
    assert {re.match(r"\w+", k).group(0) for k in calls} == seen_kernels()          # the two records come from the same run
    named = {inst for _, inst, _ in table_kernels(rows) if inst}
    assert set(STEP_CHILD) <= named
    for inst in DEFAULT_RUN:
        assert calls.get(inst, 0) >= 1, inst
    # the recorded run is the parent's, with the default YT8M_STEP_MODE: no other mode of a step kernel in it
    assert not set(STEP_CHILD) & set(calls), sorted(set(STEP_CHILD) & set(calls))


def test_the_check_notices_a_misspelt_kernel_a_deleted_row_a_new_kernel_and_a_new_entry_point(tmp_path):
    rows = branch_table()
    i = next(n for n, r in enumerate(rows) if "lnlstm_fwd_kernel<8>" in r[2])
    broken = rows[:i] + [(rows[i][0], rows[i][1], "lnlstm_fwdd_kernel<8>", rows[i][3])] + rows[i + 1:]
    assert any("lnlstm_fwdd_kernel" in p for p in table_problems(broken))
    renamed = rows[:i] + [(rows[i][0], rows[i][1], "lnlstm_fwd_kernel<16>", rows[i][3])] + rows[i + 1:]
    assert any("lnlstm_fwd_kernel<16> was never called" in p for p in table_problems(renamed))
    assert any("lnlstm_fwd_kernel<8> has no row" in p for p in table_problems(renamed))
    assert any("lnlstm_fwd_kernel<8> has no row" in p for p in table_problems(rows[:i] + rows[i + 1:]))
    j = next(n for n, r in enumerate(rows) if r[0] == "yt8m_lstm_packed_floats")
    assert any("yt8m_lstm_packed_floats has no row" in p for p in table_problems(rows[:j] + rows[j + 1:]))
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    for f in SOURCES:
        (csrc / f).write_text(open(os.path.join(CSRC, f)).read())
    with open(str(csrc / "cells.hip"), "a") as f:
        f.write('\n__global__ __launch_bounds__(256) void brand_new_kernel(float* p) { p[0] = 0.f; }\n'
                'extern "C" int yt8m_brand_new(float* p, yt8m_stream_t s) { return 0; }\n')
    with open(str(csrc / "sequence.hip"), "a") as f:
        f.write('\nextern "C" int yt8m_lstm_brand_new(float* p, yt8m_stream_t s) { return 0; }\n'
                'extern "C" int yt8m_topk_brand_new(float* p, yt8m_stream_t s) { return 0; }\n')
    assert uncovered(str(csrc)) == ["brand_new_kernel"]
    problems = table_problems(rows, str(csrc))
    assert any("yt8m_brand_new has no row" in p for p in problems) and any("yt8m_lstm_brand_new has no row" in p for p in problems)
    assert not any("yt8m_topk_brand_new" in p for p in problems)                       # the streaming module's half of sequence.hip
