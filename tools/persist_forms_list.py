"""Turns the kernel statistics of a kernel-trace-only profiled run of tests/test_gpu_persist_forms.py (no counters collected, the program
after `--`) into the committed records:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o forms -- python -m pytest tests/test_gpu_persist_forms.py -q -m gpu
    python tools/persist_forms_list.py OUT/.../forms_kernel_stats.csv

writes profiles/persist_forms_branches_kernel_stats.csv (instantiation, calls: the project's kernels only, parameter lists dropped) as
tools/streaming_kernel_list.py does, and from it tests/golden/persist_forms_seen.txt: the instantiations, template arguments included, of
the kernels of csrc/lstm_persist.hip and csrc/gru_persist.inl, which tests/test_persist_plan_host.py compares with its table."""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from streaming_kernel_list import CSRC, ROOT, main  # noqa: E402

if __name__ == "__main__":
    main(sys.argv[1], "persist_forms")
    os.remove(os.path.join(ROOT, "tests", "golden", "persist_forms_kernels_seen.txt"))       # base names: the table needs the arguments
    text = open(os.path.join(CSRC, "lstm_persist.hip")).read() + open(os.path.join(CSRC, "gru_persist.inl")).read()
    ours = set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", text)) - {"persist_fault_kernel"}
    rows = csv.DictReader(open(os.path.join(ROOT, "profiles", "persist_forms_branches_kernel_stats.csv")))
    with open(os.path.join(ROOT, "tests", "golden", "persist_forms_seen.txt"), "w") as f:
        for name in sorted(r["Name"] for r in rows if r["Name"].split("<")[0] in ours):
            f.write(name + "\n")
