"""Code-object metadata of the blend backward's instantiations (render_bwd_v2_kernel<PPL, FULL, ABS>) of two builds of the library, side by
side: VGPRs, SGPRs, LDS bytes, scratch bytes, kernel-argument bytes and spills, read from the gfx950 code object inside libadgs_hip.so
(needs no GPU; uses llvm-objcopy / clang-offload-bundler / llvm-readelf of the ROCm LLVM and c++filt).

    python tools/bwd_code_objects.py OLD/libadgs_hip.so NEW/libadgs_hip.so [--llvm /opt/rocm/llvm/bin]

An instantiation of a build from before the ABS parameter existed (<PPL, FULL>) is matched with <PPL, FULL, false>: the check that the
kernels without the absolute-gradient sums are the code they were.
"""
import argparse
import os
import re
import subprocess
import tempfile


def metadata(lib, llvm):
    d = tempfile.mkdtemp(prefix="bwd_co_")
    fb = os.path.join(d, "fat.bin")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, lib, os.devnull])
    data = open(fb, "rb").read()
    offs = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
    res = {}
    for i, o in enumerate(offs):
        part, co = os.path.join(d, "b%d" % i), os.path.join(d, "co%d" % i)
        with open(part, "wb") as f:
            f.write(data[o:(offs[i + 1] if i + 1 < len(offs) else len(data))])
        r = subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True, text=True)
        if r.returncode or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
            if "render_bwd_v2_kernel" not in g("name"):
                continue
            dem = subprocess.run(["c++filt", g("name")], capture_output=True, text=True).stdout.strip()
            args = re.search(r"render_bwd_v2_kernel<([^>]*)>", dem).group(1).replace(" ", "").split(",")
            key = tuple(args + ["false"] * (3 - len(args)))
            res[key] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), lds=int(g("group_segment_fixed_size")),
                            scratch=int(g("private_segment_fixed_size")), kernarg=int(g("kernarg_segment_size")),
                            spills=int(g("vgpr_spill_count")) + int(g("sgpr_spill_count")))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--llvm", default="/opt/rocm/llvm/bin")
    a = ap.parse_args()
    old, new = metadata(a.old, a.llvm), metadata(a.new, a.llvm)
    fmt = lambda m: "-" if m is None else "%4d %4d %6d %7d %7d %6d" % (m["vgpr"], m["sgpr"], m["lds"], m["scratch"], m["kernarg"], m["spills"])
    print("%-22s | %-39s | %-39s |" % ("<PPL, FULL, ABS>", "old: vgpr sgpr    lds scratch kernarg spills", "new: vgpr sgpr    lds scratch kernarg spills"))
    for k in sorted(set(old) | set(new)):
        verdict = "" if k not in old else ("identical" if old[k] == new.get(k) else "DIFFERENT")
        print("%-22s | %-39s | %-39s | %s" % ("<%s>" % ", ".join(k), "     " + fmt(old.get(k)), "     " + fmt(new.get(k)), verdict))


if __name__ == "__main__":
    main()
