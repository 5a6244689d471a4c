"""Turns the kernel statistics of a kernel-trace-only profiled run of tests/test_gpu_optim_branches.py (no counters collected) into the two
committed records:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o branches -- python -m pytest tests/test_gpu_optim_branches.py -q -m gpu
    python tools/optim_kernel_list.py OUT/.../branches_kernel_stats.csv

writes profiles/optim_branches_kernel_stats.csv (instantiation, calls: the project's kernels only, parameter lists dropped) and
tests/golden/optim_kernels_seen.txt (their base names), which tests/test_optim_branch_table.py reads.  The sibling of
tools/streaming_kernel_list.py, whose name parsing it shares."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from streaming_kernel_list import main  # noqa: E402

if __name__ == "__main__":
    main(sys.argv[1], "optim")
