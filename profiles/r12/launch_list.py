"""kernel_trace.csv -> ordered launch list per stream: stream ordinal (by first appearance), kernel
name with its template arguments (no parameter list), grid, workgroup, LDS bytes.  Only the
library's own kernels (namespace ldpc) are listed.  Usage: launch_list.py run_kernel_trace.csv"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
key = "Stream_Id" if "Stream_Id" in rows[0] else "Queue_Id"
ids = {}
per = {}
for r in rows:
    s = ids.setdefault((r["Queue_Id"], r[key]), len(ids))
    g = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
    w = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
    name = r["Kernel_Name"].replace("(anonymous namespace)", "{anon}").split("(")[0]
    if "ldpc::" not in name:
        continue
    per.setdefault(s, []).append(f'{name} grid {g} wg {w} lds {r["LDS_Block_Size"]}')
for s in sorted(per):
    for line in per[s]:
        print(f"stream{s} {line}")
