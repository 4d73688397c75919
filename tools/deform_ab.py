"""A/B of two builds of the library on the deformation pass: bits, then time.

    python tools/deform_ab.py PARENT.so NEW.so [--out DIR] [--rounds 3] [--samples 3] [--no-time] [--no-bits]

Every measurement runs in a fresh child process that loads ONE library through ADGS_LIB; the two are never in one process.

Bits: every "ok" case of tests/deform_cases.py, forward and backward on the same seeded inputs and upstream weights; all outputs and
parameter gradients are dumped and compared bit for bit.  The gradient of the background row is summed with float atomics across
workgroups and has no stable bits: the parent library runs twice, the largest difference between its two runs relative to the row's
largest magnitude is recorded per case, and new-vs-parent may differ by twice that (two independent orders are compared instead of
one), with a floor of 2^-22 of the largest magnitude where the parent's runs agree exactly.

Time: the C3 model, children alternating parent, new, parent, new, ...  Each child warms up, then takes `--samples` samples of
  geometry: forward / backward of get_deformed_pkg(flow_time) without the SH tensor -- the launches of a raw-SH training frame
  full:     the same with the [N,16,3] SH tensor materialised (the backward then launches deform_lin_param_grad_kernel)
each sample a loop long enough to last a fraction of a second, synchronised before and after; the backward loop replays one retained
graph.  These are wall-clock times between two device synchronisations, so they include the host's launch path (the kernels
themselves take 30-50 us); per-kernel device times come from
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/deform_ab.py --child frames --frames 200       (ADGS_LIB set)
one run per library.  Verdict: the new library's median must lie within the range of the parent's samples.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ATOMIC = "background_deform_param"


# ------------------------------------------------------------------ children (one library each)
def _load_library():
    """The loader insists on every declared entry point; the older of two builds may lack test hooks (adgs_test_*) declared since.
    Those, and only those, are dropped from the table (and named) before the first load, so that the same Python tree drives both
    builds; a build that lacks anything else fails to load as usual."""
    import ctypes
    import torch  # noqa: F401  (first: the loader's own rule)
    from adgs import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    missing = [name for name in _lib.SIGNATURES if name.startswith("adgs_test_") and not hasattr(handle, name)]
    for name in missing:
        del _lib.SIGNATURES[name]
    if missing:
        print("deform_ab: %s lacks %s" % (_lib.LIB_PATH, ", ".join(missing)), file=sys.stderr)
    _lib.lib()


def _case_model(case, raw):
    import numpy as np
    import torch
    from tests import deform_cases as dc

    class Model:
        pass
    m = Model()
    for name, v in raw.items():
        t = torch.from_numpy(np.array(v))
        if case.misaligned:          # a contiguous view one float into its buffer
            buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device="cuda")
            view = buf[1:1 + t.numel()].view(t.shape)
            view.copy_(t)
            p = view.detach()
        else:
            p = t.cuda()
        setattr(m, dc.attr_of(name), p.requires_grad_(name != "gs_time"))
    m.order_args, m.use_time_mask = dc.order_args(case), case.use_time_mask
    return m


def child_dump(path):
    import numpy as np
    import torch
    from adgs.deform import get_deformed_pkg
    from tests import deform_cases as dc
    out = {}
    for case in dc.CASES:
        if case.expect != "ok":
            continue
        raw = dc.raw_inputs(case)
        m = _case_model(case, raw)
        pkg = get_deformed_pkg(m, case.t, flow_time=case.flow_time)
        keys = sorted(k for k in pkg if pkg[k].numel())
        ws = dc.upstream_weights(case, {k: tuple(pkg[k].shape) for k in keys})
        torch.autograd.backward([pkg[k] for k in keys], [torch.tensor(ws[k], dtype=torch.float32).cuda() for k in keys])
        torch.cuda.synchronize()
        for k in keys:
            out["%s/out/%s" % (case.id, k)] = pkg[k].detach().cpu().numpy()
        for name in dc.RAW_NAMES:
            g = getattr(m, dc.attr_of(name)).grad
            if g is not None:
                out["%s/grad/%s" % (case.id, name)] = g.cpu().numpy()
    np.savez(path, **out)


def _c3_model():
    from adgs import synthetic
    from adgs.model import SyntheticGaussianModel, DEFAULT_ORDER_ARGS
    return SyntheticGaussianModel.from_scene(synthetic.make_config_scene("C3"), "cuda", seed=0, order_args=dict(DEFAULT_ORDER_ARGS))


def _passes(m, raw_sh):
    """(forward, backward) closures of one configuration; the backward replays one retained graph with fixed upstream gradients."""
    import torch
    from adgs import deform
    want = ("xyz", "rotation", "opacity", "scales") if raw_sh else ("xyz", "rotation", "shs", "opacity", "scales")
    fwd = lambda: deform.get_deformed_pkg(m, 0.37, want=want, flow_time=0.42)
    pkg = fwd()
    outs = [pkg[k] for k in sorted(pkg)]
    ups = [torch.ones_like(o) for o in outs]
    params = [p for p in m.parameters()]

    def bwd():
        for p in params:
            p.grad = None
        torch.autograd.backward(outs, ups, retain_graph=True)
    return fwd, bwd


def child_time(path, samples, min_seconds):
    import time
    import torch
    m = _c3_model()
    res = {}
    for tag, raw_sh in (("geometry", True), ("full", False)):
        for name, fn in zip(("fwd", "bwd"), _passes(m, raw_sh)):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            iters = max(20, int(min_seconds / ((time.perf_counter() - t0) / 20)) + 1)
            vals = []
            for _ in range(samples):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize()
                vals.append((time.perf_counter() - t0) / iters * 1e6)
            res["%s_%s_us" % (tag, name)] = vals
            res["%s_%s_iters" % (tag, name)] = iters
    json.dump(res, open(path, "w"))


def child_frames(frames):
    """`frames` forward + backward passes of the full configuration, for a kernel trace."""
    import torch
    fwd, bwd = _passes(_c3_model(), False)
    for _ in range(frames):
        fwd()
        bwd()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ parent: spawns, compares
def run_child(lib, args):
    env = dict(os.environ, ADGS_LIB=os.path.abspath(lib))
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, env=env, check=True, timeout=900)


def compare_bits(out_dir, parent, new):
    import numpy as np
    files = {}
    for tag, lib in (("parent_a", parent), ("parent_b", parent), ("new", new)):
        files[tag] = os.path.join(out_dir, "dump_%s.npz" % tag)
        run_child(lib, ["dump", "--file", files[tag]])
    d = {tag: np.load(f) for tag, f in files.items()}
    assert set(d["parent_a"].files) == set(d["parent_b"].files) == set(d["new"].files), "the libraries produced different sets of tensors"
    report, bad = {"tensors": len(d["new"].files), "atomic_rows": {}}, []
    for key in sorted(d["new"].files):
        a, b, n = d["parent_a"][key], d["parent_b"][key], d["new"][key]
        if key.endswith("/" + ATOMIC):
            scale = float(max(np.abs(a).max(), 1e-30))
            own = float(np.abs(a.astype(np.float64) - b).max() / scale)
            got = float(np.abs(n.astype(np.float64) - a).max() / scale)
            bound = 2.0 * own if own > 0.0 else 2.0 ** -22
            report["atomic_rows"][key.split("/")[0]] = {"parent_vs_parent": own, "new_vs_parent": got, "bound": bound}
            if got > bound:
                bad.append(key)
        elif not (np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), n.view(np.uint32))):
            bad.append(key + (" (the parent's own two runs differ)" if not np.array_equal(a.view(np.uint32), b.view(np.uint32)) else ""))
    report["differing"] = bad
    for f in files.values():
        os.remove(f)
    return report


def compare_time(out_dir, parent, new, rounds, samples, min_seconds):
    runs = {"parent": {}, "new": {}}
    for r in range(rounds):
        for tag, lib in (("parent", parent), ("new", new)):
            f = os.path.join(out_dir, "time_%s_%d.json" % (tag, r))
            run_child(lib, ["time", "--file", f, "--samples", str(samples), "--min-seconds", str(min_seconds)])
            for k, v in json.load(open(f)).items():
                if k.endswith("_us"):
                    runs[tag].setdefault(k, []).extend(v)
            os.remove(f)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {}
    for k in sorted(runs["parent"]):
        p, n = runs["parent"][k], runs["new"][k]
        summary[k] = {"parent": p, "new": n, "parent_median": med(p), "new_median": med(n), "parent_range": [min(p), max(p)],
                      "within_parent_range": min(p) <= med(n) <= max(p)}
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--child", choices=("dump", "time", "frames"))
    ap.add_argument("--file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_refactor"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--no-bits", action="store_true")
    a = ap.parse_args()
    if a.child:
        _load_library()
    if a.child == "dump":
        return child_dump(a.file)
    if a.child == "time":
        return child_time(a.file, a.samples, a.min_seconds)
    if a.child == "frames":
        return child_frames(a.frames)
    if len(a.libs) != 2:
        ap.error("two library paths: PARENT.so NEW.so")
    os.makedirs(a.out, exist_ok=True)
    ok = True
    if not a.no_bits:
        bits = compare_bits(a.out, *a.libs)
        json.dump(bits, open(os.path.join(a.out, "bits.json"), "w"), indent=1)
        print(json.dumps({"bits": {"tensors": bits["tensors"], "differing": bits["differing"], "atomic_rows": bits["atomic_rows"]}}))
        ok = ok and not bits["differing"]
    if not a.no_time:
        times = compare_time(a.out, a.libs[0], a.libs[1], a.rounds, a.samples, a.min_seconds)
        json.dump(times, open(os.path.join(a.out, "time.json"), "w"), indent=1)
        print(json.dumps({"time": {k: {f: v[f] for f in ("parent_median", "new_median", "parent_range", "within_parent_range")} for k, v in times.items()}}))
        ok = ok and all(v["within_parent_range"] for v in times.values())
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
