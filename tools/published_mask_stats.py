"""Per-launch statistics (mean, min, max over the last 200 launches) of the kernels the published mask touches and of the per-frame sum of
ALL kernels, from `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 200 --warmup 20
--no-cpu-baseline --no-secondary` runs (ADGS_LIB picks the build):  python tools/published_mask_stats.py OUT.json TAG=DIR [TAG=DIR ...]
(profiles/published_mask/kernel_stats.json)."""
import csv, glob, json, statistics, sys

KERNELS = ["preprocess_bwd_kernel", "render_fwd_v2_kernel", "render_bwd_v2_kernel", "lin_param_grad", "preprocess_fwd_kernel", "sh0_rows_kernel"]
STEPS = 200

out = {}
for arg in sys.argv[2:]:
    tag, d = arg.split("=")
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        out[tag] = {"error": "no kernel trace under " + d}
        continue
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {k: [] for k in KERNELS}
    marks = []                                   # index of every preprocess_bwd launch: the last kernel family of a frame's rasterizer
    durs = []
    for i, r in enumerate(rows):
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        durs.append(dur)
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                per[k].append(dur)
                if k == "preprocess_bwd_kernel":
                    marks.append(i)
                break
    res = {}
    for k, v in per.items():
        v = v[-STEPS:]
        if v:
            res[k] = {"launches": len(v), "mean_us": round(statistics.mean(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    # a frame = the kernels from behind one preprocess_bwd launch up to and including the next
    marks = marks[-(STEPS + 1):]
    sums = [sum(durs[a + 1:b + 1]) for a, b in zip(marks[:-1], marks[1:])]
    if sums:
        res["frame_sum_of_all_kernels"] = {"frames": len(sums), "mean_us": round(statistics.mean(sums), 2), "std_us": round(statistics.pstdev(sums), 2),
                                           "min_us": round(min(sums), 2), "max_us": round(max(sums), 2)}
    out[tag] = res
json.dump(out, open(sys.argv[1], "w"), indent=1)
for tag, res in out.items():
    print(tag)
    for k, v in res.items():
        print("   %-28s %s" % (k, v))
