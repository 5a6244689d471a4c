"""Not -m gpu: keeps the branch table of tests/test_gpu_optim_branches.py honest.

Every __global__ kernel of csrc/optim.hip is either in the list recorded from a profiled run of that module
(tests/golden/optim_kernels_seen.txt; call counts per instantiation in profiles/optim_branches_kernel_stats.csv, both written by
tools/optim_kernel_list.py) or in EXCLUDED below with the test that covers it; every kernel the table names exists in the source and was
seen, every instantiation it names was called; every extern "C" function of the file has a row.  A kernel or an entry point added to
optim.hip fails here until a branch case reaches it and the list is recorded again."""
import csv
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "youtube-8m_amd", "csrc")
SOURCES = ["optim.hip"]
SEEN = os.path.join(ROOT, "tests", "golden", "optim_kernels_seen.txt")
STATS = os.path.join(ROOT, "profiles", "optim_branches_kernel_stats.csv")

# kernels of the file that the branch module does not launch (none: it reaches all seven)
EXCLUDED = {}
# kernels of other files that the recorded run holds: what the module's set-up launches on the way to optim.hip
FOREIGN = {
    "h2_absmax_kernel": "csrc/gemm_x3.hip: wimg.WeightImages.refresh measures max |w| with it before the first build of an h2 image "
                        "(tests/test_gpu_optim_branches.py::test_h2_images checks the word it leaves)",
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
    spec = importlib.util.spec_from_file_location("_optim_branches", path or os.path.join(ROOT, "tests", "test_gpu_optim_branches.py"))
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
    """Every way the table disagrees with the source and the recorded run, as a list of sentences."""
    src, seen = source_kernels(csrc), seen_kernels(seen_path)
    calls = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(stats_path))}
    bad = []
    for base, inst, left_out in table_kernels(rows):
        if base not in src:
            bad.append("the table names %s, which is not in the source" % base)
        elif base in EXCLUDED or left_out:
            continue
        elif base not in seen:
            bad.append("the table names %s, which the recorded run never launched" % base)
        elif inst and calls.get(inst, 0) < 1:
            bad.append("instantiation %s was never called in the recorded run" % inst)
    for e in sorted(source_entry_points(csrc) - {r[0] for r in rows}):
        bad.append("entry point %s has no row" % e)
    for e in sorted({r[0] for r in rows} - source_entry_points(csrc)):
        bad.append("the table names entry point %s, which is not in the source" % e)
    return bad


def _test_exists(where):
    path, test = where.split(" ")[0].split("::")
    return re.search(r"^def %s\(" % test, open(os.path.join(ROOT, path)).read(), re.M) is not None


def test_every_optim_kernel_is_reached_or_excluded_by_name():
    src = source_kernels()
    assert len(src) == 7 and len(source_entry_points()) == 7
    assert not uncovered(), "kernels no branch case reaches (add the case and its table row, then record the list again): %s" % uncovered()
    assert not set(EXCLUDED) - src, "stale exclusions: %s" % sorted(set(EXCLUDED) - src)
    assert not set(EXCLUDED) & seen_kernels(), "excluded although seen: %s" % sorted(set(EXCLUDED) & seen_kernels())
    assert seen_kernels() == src | set(FOREIGN)                              # the recorded list holds all seven and nothing unexplained
    assert not set(FOREIGN) & src
    for where in EXCLUDED.values():
        assert _test_exists(where), where


def test_every_kernel_of_the_branch_table_exists_and_was_called():
    rows = branch_table()
    assert all(len(r) == 4 and all(isinstance(x, str) and x for x in r) for r in rows)
    assert len(table_kernels(rows)) >= 30
    assert not table_problems(rows), "\n".join(table_problems(rows))
    calls = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(STATS))}
    assert {re.match(r"\w+", k).group(0) for k in calls} == seen_kernels()          # the two records come from the same run
    named = {inst for _, inst, _ in table_kernels(rows) if inst}
    assert named == {"adam_tile_kernel<true>", "adam_tile_kernel<false>"}
    assert calls.get("adam_tile_kernel<true>", 0) >= 1 and calls.get("adam_tile_kernel<false>", 0) >= 1
    assert {base for base, _, _ in table_kernels(rows)} == source_kernels()
    # every row either names a case of the GPU module / a host test that exists, or begins with "left out:" and a reason
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_optim_branches.py")).read()
    for r in rows:
        if r[3].startswith("left out:"):
            assert len(r[3]) > 20, r
            continue
        tests = re.findall(r"\btest_\w+", r[3].replace("tests/test_optim_host.py", ""))
        assert tests, r
        host = open(os.path.join(ROOT, "tests", "test_optim_host.py")).read()
        for t in tests:
            assert re.search(r"^def %s\(" % t, gpu, re.M) or re.search(r"^def %s\(" % t, host, re.M), (r, t)


def test_the_check_notices_a_misspelt_kernel_a_new_kernel_and_a_new_entry_point(tmp_path):
    rows = branch_table()
    i = next(k for k, r in enumerate(rows) if "adam_tile_kernel<true>" in r[2])
    broken = rows[:i] + [(rows[i][0], rows[i][1], "adam_tyle_kernel<true>", rows[i][3])] + rows[i + 1:]
    assert any("adam_tyle_kernel" in p for p in table_problems(broken))
    never = rows[:i] + [(rows[i][0], rows[i][1], "adam_tile_kernel<2>", rows[i][3])] + rows[i + 1:]
    assert any("never called" in p for p in table_problems(never))
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    for f in SOURCES:
        (csrc / f).write_text(open(os.path.join(CSRC, f)).read())
    with open(str(csrc / "optim.hip"), "a") as f:
        f.write('\n__global__ __launch_bounds__(256) void brand_new_kernel(float* p) { p[0] = 0.f; }\n'
                'extern "C" int yt8m_brand_new(float* p, yt8m_stream_t s) { return 0; }\n')
    assert uncovered(str(csrc)) == ["brand_new_kernel"]
    assert any("yt8m_brand_new has no row" in p for p in table_problems(rows, str(csrc)))
