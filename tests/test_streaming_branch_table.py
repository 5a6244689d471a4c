"""Not -m gpu: keeps the branch table of tests/test_gpu_streaming_branches.py honest.

Every __global__ kernel of csrc/elementwise.hip, csrc/sequence.hip, csrc/dbof.hip and csrc/netvlad.hip is either in the list recorded from a
profiled run of that module (tests/golden/streaming_kernels_seen.txt; call counts per instantiation in
profiles/streaming_branches_kernel_stats.csv, both written by tools/streaming_kernel_list.py) or in EXCLUDED below with the test that covers
it; every kernel the table names exists in the sources and was seen, every instantiation it names was called.  A kernel added to these
files fails here until a branch case reaches it and the list is recorded again."""
import csv
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "youtube-8m_amd", "csrc")
SOURCES = ["elementwise.hip", "sequence.hip", "dbof.hip", "netvlad.hip"]
SEEN = os.path.join(ROOT, "tests", "golden", "streaming_kernels_seen.txt")
STATS = os.path.join(ROOT, "profiles", "streaming_branches_kernel_stats.csv")

# kernels of these files that the branch module does not launch: helpers with a test of their own
EXCLUDED = {
    "dequant_mean_l2norm_kernel": "tests/test_gpu_kernels.py::test_dequant_l2norm (one kernel, no dispatch)",
    "lstm_gates_fwd_kernel": "tests/test_gpu_kernels.py::test_lstm_layer_fwd_bwd (H = 4: the per-step path)",
    "lstm_gates_bwd_kernel": "tests/test_gpu_kernels.py::test_lstm_layer_fwd_bwd (H = 4: the per-step path)",
    "reverse_u8_kernel": "tests/test_gpu_bilstm.py::test_reverse_sequence_u8_is_a_gather_and_its_own_inverse",
    "reverse_f32_tm_kernel": "tests/test_gpu_bilstm.py::test_reverse_sequence_f32_tm_writes_only_its_column_window",
    "sample_gather_kernel": "tests/test_gpu_round2.py::test_sample_frames_bit_exact_vs_oracle",
}


def source_kernels(csrc=CSRC):
    names = set()
    for f in SOURCES:
        names.update(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(csrc, f)).read()))
    return names


def seen_kernels(path=SEEN):
    return {l.strip() for l in open(path) if l.strip()}


def branch_table():
    spec = importlib.util.spec_from_file_location("_streaming_branches", os.path.join(ROOT, "tests", "test_gpu_streaming_branches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.BRANCH_TABLE


def table_kernels():
    """(base name, instantiation or None) for every kernel a table row names."""
    out = []
    for row in branch_table():
        for base, targs in re.findall(r"(\w+_kernel)(<[^>]*>)?", row[2]):
            out.append((base, base + targs if targs else None))
    return out


def uncovered(csrc=CSRC, seen_path=SEEN):
    return sorted(source_kernels(csrc) - seen_kernels(seen_path) - set(EXCLUDED))


def test_every_streaming_kernel_is_reached_or_excluded_by_name():
    src = source_kernels()
    assert len(src) > 40
    assert not uncovered(), "kernels no branch case reaches (add the case and its table row, then record the list again): %s" % uncovered()
    assert not set(EXCLUDED) - src, "stale exclusions: %s" % sorted(set(EXCLUDED) - src)
    assert not set(EXCLUDED) & seen_kernels(), "excluded although seen: %s" % sorted(set(EXCLUDED) & seen_kernels())
    for name, where in EXCLUDED.items():
        path, test = where.split(" ")[0].split("::")
        assert re.search(r"^def %s\(" % test, open(os.path.join(ROOT, path)).read(), re.M), where


def test_every_kernel_of_the_branch_table_exists_and_was_called():
    src, seen = source_kernels(), seen_kernels()
    calls = {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(STATS))}
    named = table_kernels()
    assert len(named) > 80
    for base, inst in named:
        assert base in src, "the table names %s, which is not in the sources" % base
        assert base in seen, "the table names %s, which the recorded run never launched" % base
        if inst:
            assert calls.get(inst, 0) >= 1, "instantiation %s was never called in the recorded run" % inst
    assert {re.match(r"\w+", k).group(0) for k in calls} == seen           # the two records come from the same run
    # every listed entry point has at least one row, and every row has its four fields
    rows = branch_table()
    assert all(len(r) == 4 and all(isinstance(x, str) and x for x in r) for r in rows)
    entries = {r[0] for r in rows}
    for e in ["yt8m_l2norm_fwd_f32", "yt8m_l2norm_bwd_f32", "yt8m_act_fwd_f32", "yt8m_act_bwd_f32", "yt8m_moe_mix_fwd", "yt8m_moe_mix_bwd",
              "yt8m_moe_mix_xent_fwd", "yt8m_moe_mix_xent_bwd", "yt8m_moe_mix_xent_bwd_absmax", "yt8m_xent_fwd_bwd", "yt8m_xent_bwd",
              "yt8m_colsum_f32", "yt8m_colsum_weighted_f32", "yt8m_attn_softmax_fwd", "yt8m_attn_softmax_bwd", "yt8m_softmax_rows_fwd",
              "yt8m_softmax_rows_bwd", "yt8m_topk_rows", "yt8m_perr_rows", "yt8m_frame_pool_fwd", "yt8m_frame_pool_bwd", "yt8m_batchnorm_fwd",
              "yt8m_batchnorm_bwd", "yt8m_dequant_l2norm_u8", "yt8m_vlad_finish_fwd", "yt8m_vlad_finish_bwd", "yt8m_vlad_finish_q_fwd",
              "yt8m_vlad_finish_q_bwd", "yt8m_cast_f32_bf16", "yt8m_cast_f32_bf16_dual"]:
        assert e in entries, e
