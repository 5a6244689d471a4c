"""Not -m gpu: keeps the branch table of tests/test_gpu_gemm_branches.py honest.

Every __global__ kernel of csrc/gemm_f32.hip, csrc/gemm_bf16.hip, csrc/gemm_x3.hip and csrc/gemm_auto.hip is either named by a row of the
table or listed in NOT_GEMM_DISPATCH below with the test that owns it; every kernel a row names exists in those sources; every kernel
(and every instantiation) named by a row that is not marked "left out" is in the list recorded from a kernel-trace-only profiled run of
that module (tests/golden/gemm_kernels_seen.txt; call counts per instantiation in profiles/gemm_branches_kernel_stats.csv, both written
by tools/gemm_kernel_list.py); every case a row points at exists.  A kernel or a dispatch condition added to these files fails here
until it has its row, a case reaches it and the list is recorded again."""
import csv
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "youtube-8m_amd", "csrc")
SOURCES = ["gemm_f32.hip", "gemm_bf16.hip", "gemm_x3.hip", "gemm_auto.hip"]
MODULE = os.path.join(ROOT, "tests", "test_gpu_gemm_branches.py")
SEEN = os.path.join(ROOT, "tests", "golden", "gemm_kernels_seen.txt")
STATS = os.path.join(ROOT, "profiles", "gemm_branches_kernel_stats.csv")

# kernels of these files that are no arm of the fp32 / bf16 / image GEMM dispatch the table covers: other modules own them
NOT_GEMM_DISPATCH = {
    "gemm_b1_kernel": "tests/test_gpu_round4.py::test_interleaved_image_gemms_equal_the_round3_kernels_bit_for_bit (one-plane bf16 images, "
                      "yt8m_gemm_b1_nt_grouped: the bf16 configuration's products; the round-3 schedule)",
    "gemm_b1q_kernel": "tests/test_gpu_round3.py::test_b1_image_gemm_matches_row_major_bf16 (the default schedule of the same entry point)",
    "h2_rowscale_kernel": "tests/test_gpu_h2.py::test_h2_rows_keep_their_own_precision (per-row scales: the recurrences' operand passes)",
}


def source_kernels(csrc=CSRC):
    names = set()
    for f in SOURCES:
        names.update(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(csrc, f)).read()))
    return names


def seen_kernels(path=SEEN):
    return {l.strip() for l in open(path) if l.strip()}


def gpu_module():
    spec = importlib.util.spec_from_file_location("_gemm_branches", MODULE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def left_out(row):
    return row[3].startswith("left out:")


def table_kernels(rows):
    """(base name, instantiation or None, row) for every kernel a table row names."""
    out = []
    for row in rows:
        for base, targs in re.findall(r"(\w+_kernel)(<[^>]*>)?", row[2]):
            out.append((base, base + targs if targs else None, row))
    return out


def test_every_gemm_kernel_has_a_row_or_an_owner():
    src = source_kernels()
    rows = gpu_module().BRANCH_TABLE
    named = {base for base, _, _ in table_kernels(rows)}
    assert len(src) >= 15
    missing = sorted(src - named - set(NOT_GEMM_DISPATCH))
    assert not missing, "kernels without a row in BRANCH_TABLE (add the row and its case, then record the list again): %s" % missing
    assert not set(NOT_GEMM_DISPATCH) - src, "stale exclusions: %s" % sorted(set(NOT_GEMM_DISPATCH) - src)
    assert not set(NOT_GEMM_DISPATCH) & named, "excluded although a row names it: %s" % sorted(set(NOT_GEMM_DISPATCH) & named)
    assert not set(NOT_GEMM_DISPATCH) & seen_kernels(), "excluded although the recorded run launched it"
    for name, where in NOT_GEMM_DISPATCH.items():
        path, test = where.split(" ")[0].split("::")
        assert re.search(r"^def %s\(" % test, open(os.path.join(ROOT, path)).read(), re.M), where


def test_every_kernel_of_the_branch_table_exists_and_was_called():
    src, seen = source_kernels(), seen_kernels()
    calls = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(STATS))}
    rows = gpu_module().BRANCH_TABLE
    named = table_kernels(rows)
    assert len(named) > 60
    for base, inst, row in named:
        assert base in src, "the table names %s, which is not in the sources" % base
        if left_out(row):
            continue
        assert base in seen, "the table names %s, which the recorded run never launched" % base
        if inst:
            assert calls.get(inst, 0) >= 1, "instantiation %s was never called in the recorded run" % inst
    assert {re.match(r"\w+", k).group(0) for k in calls} == seen           # the two records come from the same run
    # every instantiation the run launched is named by a row: a new template argument comes with its row
    insts = {inst for _, inst, row in named if inst}
    bases_named_whole = {base for base, inst, row in named if inst is None}
    for k in calls:
        assert k in insts or ("<" not in k and k in bases_named_whole), "the recorded run launched %s, which no row names" % k


def test_every_row_is_complete_and_points_at_a_case_that_exists():
    mod = gpu_module()
    rows = mod.BRANCH_TABLE
    assert all(len(r) == 4 and all(isinstance(x, str) and x for x in r) for r in rows)
    text = open(MODULE).read()
    for row in rows:
        if left_out(row):
            assert len(row[3]) > len("left out: ") + 10, row               # the reason
        own = re.findall(r"(?<![\w/:])(test_\w+)", re.sub(r"tests/\w+\.py::\w+", "", row[3]))
        assert own or left_out(row), "row without a case: %s" % (row,)
        for name in own:
            assert hasattr(mod, name) and re.search(r"^def %s\(" % name, text, re.M), "%s names %s, which does not exist" % (row[0], name)
        for path, name in re.findall(r"(tests/\w+\.py)::(\w+)", row[3]):
            assert re.search(r"^def %s\(" % name, open(os.path.join(ROOT, path)).read(), re.M), (path, name)
    entries = {r[0] for r in rows}
    for e in ["yt8m_gemm_f32", "yt8m_gemm_f32_batched", "yt8m_gemm_f32_grouped", "yt8m_gemm_bf16_nt_grouped", "yt8m_gemm_x3_nt_grouped",
              "yt8m_gemm_h2_nt_grouped", "yt8m_gemm_auto_grouped", "yt8m_gemm_auto_grouped_ex"]:
        assert e in entries, e
    # every environment knob the four sources read has a row (static ones: left out; YT8M_BF16_BIG_MIN is read per call and is set by a case)
    knobs = set()
    for f in SOURCES:
        knobs.update(re.findall(r'getenv\("(\w+)"\)', open(os.path.join(CSRC, f)).read()))
    table_text = " ".join(" ".join(r) for r in rows)
    for k in sorted(knobs):
        assert k in table_text, "environment knob %s of the GEMM sources has no row" % k
