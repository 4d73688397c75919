"""Per-launch statistics (mean, min, max over the launches of the last 200 frames) of EVERY kernel of a frame and of the per-frame sum of all
kernels, from `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 200 --warmup 20
--no-cpu-baseline --no-secondary` runs (ADGS_LIB picks the build):  python tools/grad_prefill_stats.py OUT.json TAG=DIR [TAG=DIR ...]
Like tools/published_mask_stats.py, whose frame boundaries (the preprocess_bwd launches) it uses, without that tool's fixed list of kernels: a
kernel that one build launches and another does not (lin_param_grad_rows_kernel in place of deform_lin_param_grad_kernel) shows as such
(profiles/grad_prefill/kernel_stats_*.json)."""
import csv, glob, json, re, statistics, sys

STEPS = 200


def short(name):
    name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace(" [clone .kd]", ""))      # without the arguments
    m = re.search(r"([A-Za-z_0-9]+)(<.*>)?\s*$", name)
    return (m.group(1) + (m.group(2) or "")) if m else name


out = {}
for arg in sys.argv[2:]:
    tag, d = arg.split("=")
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        out[tag] = {"error": "no kernel trace under " + d}
        continue
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    marks = [i for i, r in enumerate(rows) if "preprocess_bwd_kernel" in r["Kernel_Name"]][-(STEPS + 1):]
    if len(marks) < 2:
        out[tag] = {"error": "fewer than two frames"}
        continue
    per = {}
    for i in range(marks[0] + 1, marks[-1] + 1):
        per.setdefault(short(rows[i]["Kernel_Name"]), []).append(durs[i])
    frames = len(marks) - 1
    res = {k: {"launches_per_frame": round(len(v) / frames, 2), "mean_us": round(statistics.mean(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
               "per_frame_us": round(sum(v) / frames, 2)} for k, v in per.items()}
    sums = [sum(durs[a + 1:b + 1]) for a, b in zip(marks[:-1], marks[1:])]
    res["frame_sum_of_all_kernels"] = {"frames": len(sums), "mean_us": round(statistics.mean(sums), 2), "std_us": round(statistics.pstdev(sums), 2),
                                       "min_us": round(min(sums), 2), "max_us": round(max(sums), 2)}
    out[tag] = res
json.dump(out, open(sys.argv[1], "w"), indent=1)
for tag, res in out.items():
    print(tag)
    for k, v in sorted(res.items(), key=lambda kv: -kv[1].get("per_frame_us", 1e9) if isinstance(kv[1], dict) else 0):
        if not isinstance(v, dict) or v.get("per_frame_us", 1e9) >= 3.0:
            print("   %-60s %s" % (k[:60], v))
