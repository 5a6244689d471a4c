"""Turns the kernel statistics of a profiled run of tests/test_gpu_streaming_branches.py into the two committed records:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o branches -- python -m pytest tests/test_gpu_streaming_branches.py -q -m gpu
    python tools/streaming_kernel_list.py OUT/.../branches_kernel_stats.csv

writes profiles/streaming_branches_kernel_stats.csv (instantiation, calls: the project's kernels only, parameter lists dropped) and
tests/golden/streaming_kernels_seen.txt (their base names), which tests/test_streaming_branch_table.py reads."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "youtube-8m_amd", "csrc")


def project_kernels():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".inl", ".h")):
            names.update(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(CSRC, f)).read()))
    return names


def unmangled(name, ours):
    """The profiler leaves a name mangled when its demangler does not know a parameter type (_Float16: vlad_pack_kernel).  Such a name
    still spells the kernel as <length><name> and its literal template arguments as I L<type><value>E ... E: 'k<true>' from
    '_ZN12_GLOBAL__N_116vlad_pack_kernelILb1EEEv...' (bool and integer arguments, which is all these kernels take)."""
    for k in sorted(ours, key=len, reverse=True):
        head, sep, rest = name.partition("%d%s" % (len(k), k))
        if sep:
            m = re.match(r"I((?:L[a-z]n?\d+E)+)E", rest)
            if not m:
                return k
            args = [("true" if v != "0" else "false") if t == "b" else v.replace("n", "-")
                    for t, v in re.findall(r"L([a-z])(n?\d+)E", m.group(1))]
            return "%s<%s>" % (k, ", ".join(args))
    return name


def instantiation(name, ours=()):
    """'void (anonymous namespace)::k<1, float>(float const*, ...)' -> 'k<1, float>' (the first '(' outside angle brackets ends it)."""
    if name.startswith("_Z"):
        return unmangled(name, ours)
    s = re.sub(r"^void\s+", "", name.strip()).replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i].strip()
    return s.strip()


def main(path, stem="streaming"):
    """stem: which branch module the run was of (tools/gemm_kernel_list.py passes "gemm")."""
    ours = project_kernels()
    calls = {}
    for row in csv.DictReader(open(path)):
        inst = instantiation(row["Name"], ours)
        if re.match(r"\w+", inst).group(0) in ours and "::" not in inst.split("<")[0]:
            calls[inst] = calls.get(inst, 0) + int(row["Calls"])
    with open(os.path.join(ROOT, "profiles", "%s_branches_kernel_stats.csv" % stem), "w") as f:
        f.write('"Name","Calls"\n')
        for k in sorted(calls):
            f.write('"%s",%d\n' % (k, calls[k]))
    with open(os.path.join(ROOT, "tests", "golden", "%s_kernels_seen.txt" % stem), "w") as f:
        for k in sorted({re.match(r"\w+", k).group(0) for k in calls}):
            f.write(k + "\n")
    print("%d instantiations of %d kernels" % (len(calls), len({k.split("<")[0] for k in calls})))


if __name__ == "__main__":
    main(sys.argv[1])
