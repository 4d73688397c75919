"""The case table of the deformation launch paths, shared by tests/test_deform_dispatch_ref.py (CPU) and
tests/test_gpu_deform_dispatch.py (GPU).

The deformation entry points (csrc/deform.hip, csrc/deform_sh.hip) pick their kernels from the row lengths, the SH tensor shape,
the quaternion-spline order and the pointer alignment.  Every case below is built for some of those decisions; `labels(case)`
restates the predicates (plan_fwd / plan_bwd with pick_block and scene4_ok, launch_sh0's `aligned`, ADGS_NQ_SWITCH) on the case's
shapes, so the branch a case is meant to take is computed, not assumed, and REQUIRED_LABELS lists what the table must keep
covering.  `plan(case)` is compared with the library's own plan functions (adgs_test_deform_plan) in
tests/test_deform_dispatch_ref.py.

Two statements of the table's origin do not hold for the code as it is, and the mirror shows it:
  * an SH tensor with M = 4 has 12 floats per Gaussian, so N * M * 3 is always a multiple of 4 and deform_shs_fwd_kernel stores
    whole 16-byte words; its element-wise tail runs for M = 1 and M = 9 (rows of 3 / 27 floats), with and without a partial last
    word ("shs_generic_tail").  M = 4, N = 3 is in the table all the same.
  * an odd xyz row of 49 parameters has stride 147 and is staged at B = 64 (128 * 147 * 4 bytes is above 48 KiB); the odd rows
    staged at B = 128 have 17..31 parameters.  Both are in the table.
"""
import collections

import numpy as np

# ---- what the mirror restates of the library
MAX_STAGING_LDS = 156 * 1024          # csrc/kernels.h MAX_STAGING_LDS
LDS_OPT_IN = 48 * 1024                # above it a launch asks for hipFuncAttributeMaxDynamicSharedMemorySize first
MAX_QUAT = 8                          # include/adgs_deform.h ADGS_FUNC_MAX_QUAT
REFUSAL = "too large for the LDS staging buffer"

Case = collections.namedtuple("Case", "id xyz rotation shs background Ns No M use_time_mask t flow_time misaligned expect")
# expect: "ok"; "refuse": the forward refuses; "refuse_if_grad": the forward succeeds on inputs that need no gradient and refuses,
# at forward time, what the backward could not stage


def get_param_num(oa):
    return oa[0] + oa[2] + 2 * oa[3] + oa[4]


def pick_block(row_floats):
    """kernels.h pick_block: the largest block whose rows fit 48 KiB, else one wave."""
    for B in (256, 128, 64):
        if B * row_floats * 4 <= LDS_OPT_IN or B == 64:
            return B, B * row_floats * 4


def plan(c):
    """Block size, dynamic LDS, row path, scene path and refusal of the forward and backward geometry launches, as deform.hip's
    plan_fwd / plan_bwd compute them."""
    np_x, np_r = get_param_num(c.xyz), get_param_num(c.rotation)
    sx, sr = (3 * np_x) | 1, (4 * np_r) | 1
    aligned = not c.misaligned
    xyz_rows = c.No > 0 and np_x > 0 and np_x % 2 == 0 and aligned
    fB, flds = pick_block(sr if xyz_rows else max(sx, sr)) if c.No > 0 else (256, 0)
    if xyz_rows:
        flds = max(flds, 2 * np_x * 4)
    bB, blds = pick_block(max(sx, sr)) if c.No > 0 else (256, 0)
    if c.No > 0:
        blds = max(blds, bB * sx * 4 + 2 * np_x * 4)
    return dict(np_x=np_x, np_r=np_r, xyz_rows=xyz_rows, scene4=aligned, fwd_B=fB, fwd_lds=flds, bwd_B=bB, bwd_lds=blds,
                fwd_refused=flds > MAX_STAGING_LDS, bwd_refused=blds > MAX_STAGING_LDS)


def labels(c):
    """The launch decisions of deform.hip this case takes (forward and backward together)."""
    p = plan(c)
    out = set()
    N, np_s = c.Ns + c.No, get_param_num(c.shs)
    fwd_refused, bwd_refused = p["fwd_refused"], p["bwd_refused"]
    if fwd_refused:
        return {"refuse_fwd"}
    if bwd_refused:
        out.add("refuse_bwd_only")
    # SH tensor
    if c.M == 16:
        out.add("shs_m16")
        lin = np_s > 0
        if not lin:
            out.add("sh0_none")
        elif np_s % 4 == 0 and np_s <= 32 and not c.misaligned:
            out.add("sh0_rows_nv4=%d" % (np_s // 4))
            if 0 < c.Ns and c.No > 0 and (3 * c.Ns) % 256 != 0:
                out.add("sh0_rows_straddle")
        else:
            out.add("sh0_general")
            if np_s > 32:
                out.add("sh0_general_np>32")
            if np_s % 4 == 0 and np_s <= 32:
                out.add("sh0_general_misaligned")
    else:
        out.add("shs_generic")
        out.add("shs_generic_M=%d" % c.M)
        if (c.M * 3) % 4 != 0:
            out.add("shs_generic_tail")
            if (N * c.M * 3) % 4 != 0:
                out.add("shs_generic_partial_word")
    # quaternion spline
    out.add("nq=%d" % (c.rotation[5] + 1 if c.rotation[4] != 0 else 0))
    # geometry launches
    for side in ("fwd", "bwd"):
        if side == "bwd" and bwd_refused:
            continue
        B, lds = p[side + "_B"], p[side + "_lds"]
        if c.No > 0:
            out.add("%s_B=%d" % (side, B))
            if lds > LDS_OPT_IN:
                out.add("%s_lds>48k" % side)
            for d, name in ((-1, "B-1"), (0, "B"), (1, "B+1")):
                if c.No == B + d:
                    out.add("no=%s@%d" % (name, B))
    if c.Ns > 0:
        out.add("scene_generic" if c.misaligned else "scene4")
        out.add("ns%%4=%d" % (c.Ns % 4))
    if c.No > 0 and p["np_x"] > 0:
        if p["xyz_rows"]:
            out.add("xyz_rows")
        elif p["np_x"] % 2 == 0:
            out.add("xyz_staged_misaligned")
        else:
            out.add("xyz_staged_odd")
    return out


# every branch of the launchers that no other direct test compares with a reference (and the ones it does, where cheap)
REQUIRED_LABELS = (
    ["shs_generic_M=1", "shs_generic_M=4", "shs_generic_M=9", "shs_generic_tail", "shs_generic_partial_word"]
    + ["sh0_rows_nv4=%d" % k for k in (4, 5, 7, 8)] + ["sh0_rows_straddle", "sh0_general_np>32", "sh0_none", "sh0_general_misaligned"]
    + ["nq=%d" % k for k in range(MAX_QUAT + 1)]
    + ["fwd_lds>48k", "bwd_lds>48k", "refuse_fwd", "refuse_bwd_only", "fwd_B=64", "fwd_B=128", "fwd_B=256", "bwd_B=64", "bwd_B=128", "bwd_B=256"]
    + ["scene4", "scene_generic", "xyz_rows", "xyz_staged_odd", "xyz_staged_misaligned", "ns%4=2"]
    + ["no=%s@%d" % (n, B) for B in (64, 128) for n in ("B-1", "B", "B+1")])

Z = [0] * 6
XYZ28 = [16, 5, 0, 6, 0, 0]            # 28 parameters: even, direct rows
XYZ12 = [8, 3, 0, 2, 0, 0]             # 12: with a short rotation row the backward runs at B = 256
XYZ48 = [36, 3, 0, 6, 0, 0]            # 48: even, direct rows beside a B = 64 rotation
XYZ49 = [37, 3, 0, 6, 0, 0]            # 49: odd, staged, stride 147 -> B = 64
XYZ29 = [17, 4, 0, 6, 0, 0]            # 29: odd, staged, stride 87 -> B = 128
XYZ23K = [11, 3, 0, 6, 0, 0]           # 23: eight B-spline intervals (a knot at every multiple of 1/8)
XYZ206 = [194, 3, 0, 6, 0, 0]          # 206: the forward streams the rows, the backward would need 160 112 bytes
XYZ207 = [195, 3, 0, 6, 0, 0]          # 207: staged with stride 621 (158 976 bytes), the backward would need 160 632
ROT16 = [0, 0, 0, 0, 16, 5]            # 16: stride 65 -> B = 128
ROT52 = [40, 3, 0, 0, 12, 2]           # 52: stride 209 -> B = 64 and 53 504 bytes, the first launch above 48 KiB
ROT150 = [120, 3, 0, 0, 30, 3]         # 150: stride 601 -> 153 856 bytes, near the cap
ROT156 = [120, 3, 0, 0, 36, 3]         # 156: stride 625 -> 160 000 bytes, refused
ROT_LIN = [8, 3, 0, 4, 0, 0]           # no quaternion spline
Q0, Q2, Q6, Q7 = [0, 0, 0, 0, 4, 0], [0, 0, 0, 0, 6, 2], [0, 0, 0, 0, 9, 6], [0, 0, 0, 0, 10, 7]
Q0L, Q2L, Q6L, Q7L = [6, 2, 0, 2, 4, 0], [6, 3, 0, 3, 5, 2], [8, 3, 0, 2, 8, 6], [7, 3, 0, 3, 9, 7]     # with a B-spline and a Fourier part
Q1, Q4, Q2K = [0, 0, 0, 0, 5, 1], [0, 0, 0, 0, 9, 4], [0, 0, 0, 0, 10, 2]
SH12 = [0, 0, 0, 6, 0, 0]
SH_BY_NP = {0: Z, 16: [0, 0, 0, 8, 0, 0], 20: [8, 3, 0, 6, 0, 0], 28: [12, 3, 4, 6, 0, 0], 32: [16, 5, 4, 6, 0, 0], 36: [20, 4, 4, 6, 0, 0]}
BG = [5, 3, 2, 0, 0, 0]


def _c(id, xyz, rotation, shs, Ns, No, M, t, background=Z, mask=False, flow=None, misaligned=False, expect="ok"):
    return Case(id, list(xyz), list(rotation), list(shs), list(background), Ns, No, M, mask, t, flow, misaligned, expect)


_BASE = [
    # ---- SH tensor shape: M = 1, 4, 9 with and without an SH deformation (the generic SH kernels, forward and backward)
    _c("m1_sh", XYZ28, Q0, SH12, 6, 65, 1, 0.37, mask=True),
    _c("m1_nosh", XYZ29, Q0L, Z, 2, 63, 1, 1.0, background=BG),
    _c("m4_sh_n3", XYZ12, Q2, SH12, 1, 2, 4, 0.61),
    _c("m4_nosh", XYZ29, ROT_LIN, Z, 255, 64, 4, 0.0, mask=True, background=BG),
    _c("m9_sh", XYZ28, Q6L, SH12, 6, 63, 9, 0.83, flow=0.87),
    _c("m9_nosh", XYZ28, Q7, Z, 2, 127, 9, 0.25, mask=True),
    # ---- sh0 rows: NV4 = 4, 5, 7, 8, the general kernel above 32 parameters, no SH deformation; 3 Ns = 270 is no multiple of
    # 256, so block 1 of the rows kernel straddles the scene | object boundary
    _c("sh0_np16", XYZ28, Q7L, SH_BY_NP[16], 90, 200, 16, 0.43),
    _c("sh0_np20", XYZ28, Q2L, SH_BY_NP[20], 90, 200, 16, 0.0, mask=True),
    _c("sh0_np28", XYZ29, Q6, SH_BY_NP[28], 90, 200, 16, 0.71),
    _c("sh0_np32", XYZ28, ROT16, SH_BY_NP[32], 90, 200, 16, 1.0, mask=True),
    _c("sh0_np36", XYZ28, ROT_LIN, SH_BY_NP[36], 90, 200, 16, 0.19, background=BG),
    _c("sh0_np0", XYZ29, Q4, Z, 90, 200, 16, 0.55),
    # ---- row length: B = 64 and the launches above 48 KiB, No = B - 1, B, B + 1
    _c("rot52_xyz48", XYZ48, ROT52, SH12, 258, 64, 16, 0.37, mask=True, flow=0.4),
    _c("rot52_xyz49", XYZ49, ROT52, SH12, 6, 63, 16, 1.0, flow=0.0),
    _c("rot52_no65", XYZ28, ROT52, SH12, 1, 65, 16, 0.0, background=BG),
    _c("rot150_ns0", XYZ28, ROT150, SH12, 0, 65, 16, 0.52, mask=True),
    _c("rot52_no0", XYZ48, ROT52, SH12, 255, 0, 16, 0.3),
    # ---- B = 128: No = B - 1, B, B + 1, odd xyz rows staged at B = 128
    _c("b128_no127", XYZ29, Q1, SH12, 2, 127, 16, 0.66, mask=True),
    _c("b128_no128", XYZ28, ROT16, SH12, 6, 128, 16, 0.12),
    _c("b128_no129", XYZ28, ROT16, SH12, 258, 129, 16, 0.9, background=BG, flow=0.95),
    # ---- a time stamp exactly on a knot of the xyz B-spline and of the quaternion spline (eight intervals each: t * 8 = 3)
    _c("knot", XYZ23K, Q2K, SH12, 5, 70, 16, 0.375, flow=0.5),
    # ---- refusals
    _c("rot156_refused", XYZ28, ROT156, SH12, 6, 65, 16, 0.5, expect="refuse"),
    _c("xyz206_bwd_limit", XYZ206, ROT16, SH12, 6, 65, 16, 0.5, expect="refuse_if_grad"),
    _c("xyz207_bwd_limit", XYZ207, ROT16, SH12, 6, 65, 16, 0.5, expect="refuse_if_grad"),
]


def _twin(id):
    """The same case with every model tensor a view one float into its buffer (4-byte but not 16-byte aligned)."""
    base = next(c for c in _BASE if c.id == id)
    return base._replace(id=id + "_misaligned", misaligned=True)


# a plain case, one with a quaternion spline, one with even xyz rows, one with an f_shs of 16 parameters, one with Ns = 258
CASES = _BASE + [_twin("m4_nosh"), _twin("m9_sh"), _twin("rot52_xyz48"), _twin("sh0_np16"), _twin("b128_no129")]
IDS = [c.id for c in CASES]

RAW_NAMES = ("scene_xyz", "obj_xyz", "scene_shs_dc", "obj_shs_dc", "scene_shs_rest", "obj_shs_rest", "scene_scaling", "obj_scaling",
             "scene_rotation", "obj_rotation", "scene_opacity", "obj_opacity", "xyz_deform_param", "rotation_deform_param",
             "shs_deform_param_scene", "shs_deform_param_obj", "background_deform_param", "gs_time", "gs_time_sigma")


def order_args(c):
    return dict(xyz=c.xyz, rotation=c.rotation, shs=c.shs, background=c.background)


def attr_of(name):
    """The reference GaussianModel's attribute of a raw tensor."""
    return name if name.endswith("deform_param") or name.startswith("shs_deform") or name.startswith("gs_") else "_" + name


def raw_inputs(c):
    """The case's raw model tensors as float32 numpy arrays (the value ranges of tests/test_gpu_deform.py's fuzz test), read-only."""
    rng = np.random.RandomState(9000 + IDS.index(c.id.replace("_misaligned", "")))
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    Ns, No, M = c.Ns, c.No, c.M
    raw = dict(scene_xyz=r(Ns, 3) * 10, obj_xyz=r(No, 3) * 10, scene_shs_dc=r(Ns, 1, 3), obj_shs_dc=r(No, 1, 3),
               scene_shs_rest=r(Ns, M - 1, 3) * 0.1, obj_shs_rest=r(No, M - 1, 3) * 0.1, scene_scaling=r(Ns, 3) * 0.3 - 2,
               obj_scaling=r(No, 3) * 0.3 - 2, scene_rotation=r(Ns, 4), obj_rotation=r(No, 4), scene_opacity=r(Ns, 1), obj_opacity=r(No, 1),
               xyz_deform_param=r(No, 3, get_param_num(c.xyz)) * 0.1, rotation_deform_param=r(No, 4, get_param_num(c.rotation)) * 0.3,
               shs_deform_param_scene=r(Ns, 3, get_param_num(c.shs)) * 0.1, shs_deform_param_obj=r(No, 3, get_param_num(c.shs)) * 0.1,
               background_deform_param=r(1, 3, get_param_num(c.background)) * 0.1, gs_time=rng.rand(No, 1).astype(np.float32),
               gs_time_sigma=r(No, 2) * 0.3 - 1.0)
    for v in raw.values():
        v.setflags(write=False)
    return raw


OUTPUT_KEYS = ("xyz", "rotation", "shs", "opacity", "scales")


def upstream_weights(c, shapes):
    """Random upstream weights of the outputs (and of flow_xyz), the same on both sides of a comparison."""
    rng = np.random.RandomState(500 + IDS.index(c.id.replace("_misaligned", "")))
    return {k: rng.standard_normal(shapes[k]) for k in sorted(shapes)}
