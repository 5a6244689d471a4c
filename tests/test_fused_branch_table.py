"""Not -m gpu: keeps the branch table of tests/test_gpu_fused_branches.py honest.

Every __global__ kernel of csrc/netvlad_fused.hip, csrc/gemm_skinny.hip, csrc/moe_bf16.hip, csrc/cnn_pool.hip and csrc/cnn_pool_f32.hip is
either in the list recorded from a profiled run of that module (tests/golden/fused_kernels_seen.txt; call counts per instantiation in
profiles/fused_branches_kernel_stats.csv, both written by tools/fused_kernel_list.py) or in EXCLUDED below with the test that covers it;
every kernel the table names exists in the sources and was seen, every instantiation it names was called; every extern "C" function of
the five files has a row.  A kernel or an entry point added to these files fails here until a branch case reaches it and the list is
recorded again."""
import csv
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "youtube-8m_amd", "csrc")
SOURCES = ["netvlad_fused.hip", "gemm_skinny.hip", "moe_bf16.hip", "cnn_pool.hip", "cnn_pool_f32.hip"]
SEEN = os.path.join(ROOT, "tests", "golden", "fused_kernels_seen.txt")
STATS = os.path.join(ROOT, "profiles", "fused_branches_kernel_stats.csv")

# kernels of these files that the branch module does not launch: an existing test already holds them to fp64 through the C ABI
EXCLUDED = {
    "f32_cnn_pool_dw_kernel": "tests/test_gpu_lstmcnn.py::test_gather_kernels_against_float64_index_add (one kernel, no dispatch)",
    "f32_cnn_pool_dx_kernel": "tests/test_gpu_lstmcnn.py::test_gather_kernels_against_float64_index_add (one kernel; WS = 1, 2, 3)",
}

# instantiations the table names that only the child process of the branch module launches (the 128-byte walk is a static read of the
# environment): the profiler's record of the parent need not hold them
P128_CHILD = {
    "vlad_rows_kernel<2, false, 1, true>": "tests/test_gpu_fused_branches.py::test_netvlad_p128_child_process",
    "vlad_rows_kernel<2, false, 5, true>": "tests/test_gpu_fused_branches.py::test_netvlad_p128_child_process",
    "vlad_rows_kernel<2, true, 1, true>": "tests/test_gpu_fused_branches.py::test_netvlad_p128_child_process",
    "vlad_rows_kernel<2, true, 5, true>": "tests/test_gpu_fused_branches.py::test_netvlad_p128_child_process",
}


def source_text(csrc=CSRC):
    return "\n".join(open(os.path.join(csrc, f)).read() for f in SOURCES)


def source_kernels(csrc=CSRC):
    return set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", source_text(csrc)))


def source_entry_points(csrc=CSRC):
    return set(re.findall(r'extern\s+"C"\s+[\w\s\*]*?\b(yt8m_\w+)\s*\(', source_text(csrc)))


def seen_kernels(path=SEEN):
    return {l.strip() for l in open(path) if l.strip()}


def branch_table(path=None):
    spec = importlib.util.spec_from_file_location("_fused_branches", path or os.path.join(ROOT, "tests", "test_gpu_fused_branches.py"))
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
        elif inst and inst not in P128_CHILD and calls.get(inst, 0) < 1:
            bad.append("instantiation %s was never called in the recorded run" % inst)
    for e in sorted(source_entry_points(csrc) - {r[0] for r in rows}):
        bad.append("entry point %s has no row" % e)
    for e in sorted({r[0] for r in rows} - source_entry_points(csrc)):
        bad.append("the table names entry point %s, which is not in the sources" % e)
    return bad


def _test_exists(where):
    path, test = where.split(" ")[0].split("::")
    return re.search(r"^def %s\(" % test, open(os.path.join(ROOT, path)).read(), re.M) is not None


def test_every_fused_kernel_is_reached_or_excluded_by_name():
    src = source_kernels()
    assert len(src) >= 19
    assert not uncovered(), "kernels no branch case reaches (add the case and its table row, then record the list again): %s" % uncovered()
    assert not set(EXCLUDED) - src, "stale exclusions: %s" % sorted(set(EXCLUDED) - src)
    assert not set(EXCLUDED) & seen_kernels(), "excluded although seen: %s" % sorted(set(EXCLUDED) & seen_kernels())
    for where in list(EXCLUDED.values()) + list(P128_CHILD.values()):
        assert _test_exists(where), where


def test_every_kernel_of_the_branch_table_exists_and_was_called():
    rows = branch_table()
    assert all(len(r) == 4 and all(isinstance(x, str) and x for x in r) for r in rows)
    assert len(table_kernels(rows)) > 100
    assert not table_problems(rows), "\n".join(table_problems(rows))
    calls = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(STATS))}
    assert {re.match(r"\w+", k).group(0) for k in calls} == seen_kernels()          # the two records come from the same run
    named = {inst for _, inst, _ in table_kernels(rows) if inst}
    assert set(P128_CHILD) <= named
    # what the recorded run must show: every rows kernel of the default walk, the byte kernel with the default JMAX, and the nine
    # mixing-backward instantiations the C ABI reaches
    for ns in (1, 2):
        for bwd in ("false", "true"):
            for nt in (1, 2, 3, 4, 5):
                assert calls.get("vlad_rows_kernel<%d, %s, %d, false>" % (ns, bwd, nt), 0) >= 1, (ns, bwd, nt)
    assert calls.get("skinny_fwd_kernel<8, unsigned char, 8>", 0) >= 1 and calls.get("skinny_fwd_kernel<8, unsigned char, 5>", 0) >= 1
    mix = {k for k in calls if k.startswith("moe_mix_bwd_bf16_kernel<")}
    assert len(mix) == 9 and not any(", false, unsigned short>" in k for k in mix), sorted(mix)


def test_the_check_notices_a_misspelt_kernel_a_new_kernel_and_a_new_entry_point(tmp_path):
    rows = branch_table()
    broken = [(rows[0][0], rows[0][1], "vlad_rowz_kernel<2, false, 1, false>", rows[0][3])] + rows[1:]
    assert any("vlad_rowz_kernel" in p for p in table_problems(broken))
    never = [(rows[0][0], rows[0][1], "vlad_rows_kernel<3, false, 1, false>", rows[0][3])] + rows[1:]
    assert any("never called" in p for p in table_problems(never))
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    for f in SOURCES:
        (csrc / f).write_text(open(os.path.join(CSRC, f)).read())
    with open(str(csrc / "cnn_pool.hip"), "a") as f:
        f.write('\n__global__ __launch_bounds__(256) void brand_new_kernel(float* p) { p[0] = 0.f; }\n'
                'extern "C" int yt8m_brand_new(float* p, yt8m_stream_t s) { return 0; }\n')
    assert uncovered(str(csrc)) == ["brand_new_kernel"]
    assert any("yt8m_brand_new has no row" in p for p in table_problems(rows, str(csrc)))
