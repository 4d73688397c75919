"""Per-launch statistics (mean, min, max over the last 200 launches) of the binning chain's kernels and of their per-frame sum, from
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline
--no-secondary` runs (ADGS_LIB picks the build):  python tools/binning_chain_stats.py OUT.json TAG=DIR [TAG=DIR ...]
(profiles/binning_scan/chain_stats.json)."""
import csv, glob, json, statistics, sys

CHAIN = ["cell_colscan_kernel", "cell_scan_kernel", "cell_scatter_kernel", "slab_sort_kernel", "slab_sort_slow_kernel", "tile_order", "preprocess_fwd_kernel"]
STEPS = 200


def key_of(name):
    for k in CHAIN:
        if k in name and not (k == "slab_sort_kernel" and "slow" in name):
            return k
    return None


out = {}
for arg in sys.argv[2:]:
    tag, d = arg.split("=")
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        out[tag] = {"error": "no kernel trace under " + d}
        continue
    per = {k: [] for k in CHAIN}
    total_all = 0.0
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        k = key_of(r["Kernel_Name"])
        if k:
            per[k].append(dur)
    res = {}
    last = {k: v[-STEPS:] for k, v in per.items() if v}
    for k, v in last.items():
        res[k] = {"launches": len(v), "mean_us": round(statistics.mean(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    n = min(len(v) for v in last.values())
    for name, ks in (("chain_without_preprocess", [k for k in last if k != "preprocess_fwd_kernel"]), ("chain_with_preprocess", list(last))):
        sums = [sum(last[k][-n + i] for k in ks) for i in range(n)]
        res[name] = {"frames": n, "mean_us": round(statistics.mean(sums), 2), "std_us": round(statistics.pstdev(sums), 2), "min_us": round(min(sums), 2), "max_us": round(max(sums), 2)}
    out[tag] = res
json.dump(out, open(sys.argv[1], "w"), indent=1)
for tag, res in out.items():
    print(tag)
    for k, v in res.items():
        print("   %-28s %s" % (k, v))
