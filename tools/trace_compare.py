"""Compare two rocprofv3 --kernel-trace CSVs launch by launch: kernel name, grid and workgroup size, in start order.
usage: trace_compare.py PARENT_kernel_trace.csv BRANCH_kernel_trace.csv      (kernels of torch itself, at::..., are left out)"""
import csv, difflib, sys


def launches(path):
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    key = lambda r: "%s grid %s,%s,%s wg %s,%s,%s" % ((r["Kernel_Name"],) + tuple(r[f"{a}_Size_{x}"] for a in ("Grid", "Workgroup") for x in "XYZ"))
    return [key(r) for r in rows if "at::" not in r["Kernel_Name"]]


a, b = launches(sys.argv[1]), launches(sys.argv[2])
diff = [l for l in difflib.unified_diff(a, b, "parent", "branch", lineterm="", n=1)]
print(f"parent: {len(a)} launches, branch: {len(b)} launches, {sum(l[0] in '+-' and l[:3] not in ('+++', '---') for l in diff)} differing lines")
print("\n".join(diff) if diff else "identical: every launch has the same kernel, grid and workgroup size, in the same order")
