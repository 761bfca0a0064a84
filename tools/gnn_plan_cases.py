"""Write the inputs of tests/test_gnn_plan_host.py as int32 records for tools/gnn_plan_tables_check.cpp
(the format is in that file's header).  usage: python3 tools/gnn_plan_cases.py OUT.bin"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402,F401  (import paths)
import test_gnn_plan_host as T  # noqa: E402

i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
rec = []
for vg, nv, cg, nc in T.group_cases().values():
    rec += [i32([0, len(vg), nv, nc]), i32(vg), i32(cg)]
E, v, c = T.csr_case()
rec.append(i32([1, E, len(v[1]), len(c[1])]))
for ptr, col, val in (v, c):
    rec += [i32(ptr), i32(col), np.ascontiguousarray(val, dtype=np.float32).view(np.int32)]
np.concatenate(rec).astype("<i4").tofile(sys.argv[1])
print(f"{len(T.group_cases()) + 1} cases -> {sys.argv[1]}")
