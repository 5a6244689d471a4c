"""Turns the kernel statistics of a kernel-trace-only profiled run of tests/test_gpu_step_branches.py (no counters collected, the program
after `--`) into the two committed records:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o branches -- python -m pytest tests/test_gpu_step_branches.py -q -m gpu
    python tools/step_kernel_list.py OUT/.../branches_kernel_stats.csv

writes profiles/step_branches_kernel_stats.csv (instantiation, calls: the project's kernels only, parameter lists dropped) and
tests/golden/step_kernels_seen.txt (their base names), which tests/test_step_branch_table.py reads.  The statistics file is the one of
the pytest process; the children of test_step_mode_and_switch_children write their own, which are not recorded (the table test lists
their instantiations by name).  The trace lists the kernels of a replayed hipGraph like any other launch, so the run is recorded with
graph capture on.  The sibling of tools/streaming_kernel_list.py, whose name parsing it shares."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from streaming_kernel_list import main  # noqa: E402

if __name__ == "__main__":
    main(sys.argv[1], "step")
