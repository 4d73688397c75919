"""What the evaluation pass (include/adgs_metrics.h, adgs.metrics) promises without a GPU: both entry points are declared, exported by
the cross-compiled library and bound; the ctypes mirror of adgs_metrics_desc has the C struct's size; every malformed call is refused
on the host, with a message, before anything is launched; the Python surface refuses CPU tensors.  The numerics are in
tests/test_gpu_metrics.py."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib, metrics
    header = open(os.path.join(ROOT, "include", "adgs_metrics.h")).read()
    assert re.search(r"\bsize_t\s+adgs_metrics_work_doubles\s*\(\s*int\s+regions\s*\)", header)
    assert re.search(r"\bint\s+adgs_metrics_accumulate\s*\(\s*const\s+adgs_metrics_desc\s*\*", header)
    for name, value in (("ADGS_METRICS_MAX_REGIONS", metrics.MAX_REGIONS), ("ADGS_METRICS_ROW", metrics.ROW)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, header).group(1)) == value
    assert _lib.SIGNATURES["adgs_metrics_work_doubles"] == (ctypes.c_size_t, [ctypes.c_int])
    res, args = _lib.SIGNATURES["adgs_metrics_accumulate"]
    assert res is ctypes.c_int and len(args) == 9              # eight parameters and the stream
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    assert lib.adgs_metrics_accumulate is not None and lib.adgs_metrics_work_doubles is not None
    assert ctypes.sizeof(metrics.MetricsDesc) == lib.adgs_test_abi_sizeof(10) == 28
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{(.*?)\} adgs_metrics_desc;", header, re.S).group(1), flags=re.S)
    members = [n.strip() for decl in re.findall(r"\bint\s+([\w\s,]+);", body) for n in decl.split(",")]
    assert members == [n for n, _ in metrics.MetricsDesc._fields_] and all(t is ctypes.c_int for _, t in metrics.MetricsDesc._fields_)
    slots = int(re.search(r"#define\s+ADGS_METRICS_SLOTS\s+(\d+)", header).group(1))
    for regions in range(5):
        assert lib.adgs_metrics_work_doubles(regions) == slots * (1 + regions) * metrics.ROW
    assert lib.adgs_metrics_work_doubles(-1) == 0 and lib.adgs_metrics_work_doubles(5) == 0


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched.  Without a GPU the pointers are made up (they are never
    followed); with one they are real buffers, large enough for any of the calls."""
    from adgs import _lib, metrics
    lib = _lib.lib()
    if torch.cuda.is_available():
        buf = torch.zeros(256 * 5 * 8 + 4 * 8 * 16 * 3, dtype=torch.float64, device="cuda")
        fake = buf.data_ptr()
    else:
        buf, fake = None, 0x1000

    def call(view=0, struct_bytes=None, image=fake, masks=fake, out=fake, **kw):
        f = dict(channels=3, H=8, W=16, regions=1, quantize=0, u8_mode=1)
        f.update(kw)
        d = metrics.MetricsDesc(ctypes.sizeof(metrics.MetricsDesc) if struct_bytes is None else struct_bytes, f["channels"], f["H"], f["W"], f["regions"],
                                f["quantize"], f["u8_mode"])
        return lib.adgs_metrics_accumulate(ctypes.byref(d), image, fake, masks, fake, fake, view, out, None)
    for what, code in (("channels 2", call(channels=2)), ("channels 0", call(channels=0)), ("channels 4", call(channels=4)),
                       ("five regions", call(regions=5)), ("negative regions", call(regions=-1)), ("regions without masks", call(masks=None)),
                       ("negative view index", call(view=-1)), ("H 0", call(H=0)), ("W 0", call(W=0)), ("negative W", call(W=-3)),
                       ("short struct", call(struct_bytes=24)), ("zero struct_bytes", call(struct_bytes=0)), ("u8_mode 3", call(u8_mode=3)),
                       ("u8_mode without out_u8", call(out=None)), ("quantize 2", call(quantize=2)), ("NULL image", call(image=None))):
        assert code < 0, what
        assert _lib.last_error().startswith("adgs_metrics_accumulate: "), (what, _lib.last_error())
    assert lib.adgs_metrics_accumulate(None, fake, fake, None, fake, fake, 0, None, None) < 0
    if buf is not None:
        torch.cuda.synchronize()
        assert not buf.any()


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    from adgs import metrics
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.Evaluator(4, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.to8b(torch.zeros(3, 4, 4))
    with pytest.raises(ValueError):
        metrics.to8b(torch.zeros(3, 4, 4), mode="nearest")
    assert metrics.U8_MODES == {None: 0, "round": 1, "truncate": 2}
