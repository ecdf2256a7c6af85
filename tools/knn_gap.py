"""The idle stretches around the Hamming 2-NN pass in a rocprofv3 kernel trace: python tools/knn_gap.py <kernel_trace.csv> [skip]

Per job step (one hamming_expand4_kernel each), in microseconds:
  orb->expand   end of the last describe_direct_kernel before it -> start of hamming_expand4_kernel
  knn->ratio    end of knn2_hamming_fp4_kernel -> start of the next ratio_union_kernel
  knn           duration of knn2_hamming_fp4_kernel
and the median, minimum and maximum of each over the steps after the first `skip` (default 4: warm-up).  One JSON line at the end."""
import csv
import json
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 4


def name(r):
    return r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]


ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name(r)) for r in rows)
desc_end = [e[1] for e in ev if e[2] == "describe_direct_kernel"]
expand = [e for e in ev if e[2] == "hamming_expand4_kernel"]
knn = [e for e in ev if e[2] == "knn2_hamming_fp4_kernel"]
ratio = [e for e in ev if e[2] == "ratio_union_kernel"]
steps = []
for x in expand:
    before = [t for t in desc_end if t <= x[0]]
    k = next((e for e in knn if e[0] >= x[1]), None)
    r = next((e for e in ratio if k and e[0] >= k[1]), None)
    if not before or not k or not r:
        continue
    steps.append(((x[0] - max(before)) / 1e3, (r[0] - k[1]) / 1e3, (k[1] - k[0]) / 1e3))
steps = steps[skip:]
for i, s in enumerate(steps):
    print("step %2d  orb->expand %7.1f us  knn->ratio %7.1f us  knn %7.1f us" % (i + skip, *s))
out = {"steps": len(steps)}
for col, key in enumerate(("orb_to_expand_us", "knn_to_ratio_us", "knn_us")):
    v = [s[col] for s in steps]
    out[key] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
print(json.dumps(out))
