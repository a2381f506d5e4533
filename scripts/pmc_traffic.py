"""HBM traffic per kernel dispatch from rocprofv3 --pmc passes (FETCH_SIZE and
WRITE_SIZE collected in separate passes, kernel-trace only), corrected as
MI355X_MICROARCH.md §HBM prescribes: FETCH_SIZE is in KB and counts half the
bytes of 16-B-per-lane streaming reads on gfx950 (x2); WRITE_SIZE (KB) is exact
for 16-B-per-lane stores.

    python scripts/pmc_traffic.py <fetch-pass-dir> <write-pass-dir> <out.json>
"""
import csv
import glob
import json
import os
import re
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temporal_inverse_kinematics_amd._build import source_digest  # noqa: E402


def per_kernel(d, counter):
    vals = defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != counter:
                continue
            name = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").strip()
            vals[name].append(float(r["Counter_Value"]))
    return vals


def main():
    fd, wd, out = sys.argv[1:4]
    fetch, write = per_kernel(fd, "FETCH_SIZE"), per_kernel(wd, "WRITE_SIZE")
    res = {}
    for k in sorted(set(fetch) | set(write)):
        fb = 2.0 * 1024.0 * sum(fetch.get(k, [0])) / max(1, len(fetch.get(k, [])))
        wb = 1024.0 * sum(write.get(k, [0])) / max(1, len(write.get(k, [])))
        res[k] = {"dispatches": len(fetch.get(k, [])), "fetch_bytes_per_dispatch": fb,
                  "write_bytes_per_dispatch": wb, "hbm_bytes_per_dispatch": fb + wb}
    json.dump({"source_digest": source_digest(), "method": "rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate passes) on "
                         "'bench.py --full --steps 3 --warmup 1'; FETCH_SIZE KB x 1024 x 2 (gfx950 half-count), "
                         "WRITE_SIZE KB x 1024; averaged over the kernel's dispatches",
               "kernels": res}, open(out, "w"), indent=1)
    for k, v in res.items():
        print(f"{k[:70]:<70} n={v['dispatches']:4d} fetch={v['fetch_bytes_per_dispatch'] / 1e6:9.1f} MB "
              f"write={v['write_bytes_per_dispatch'] / 1e6:9.1f} MB")


if __name__ == "__main__":
    main()
