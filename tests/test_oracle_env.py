"""The environment-map oracle against golden vectors from the reference's own scene/env.py (tests/golden/make_env_golden.py)."""
import os

import numpy as np
import pytest

from oracle import env_oracle

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_golden.npz"))
CASES = sorted({k.split("/")[0] for k in GOLD.files})


@pytest.mark.parametrize("case", CASES)
def test_background_and_gradient_match_reference(case):
    gm, R, focal = GOLD[case + "/grid_map"], GOLD[case + "/R"], float(GOLD[case + "/focal"])
    H, W = [int(v) for v in GOLD[case + "/HW"]]
    bg = env_oracle.background(gm, H, W, focal, R)
    ref = GOLD[case + "/bg"]
    # the sample position carries float32 rounding of the reference's ray arithmetic: ~1e-5 texel on these small maps
    assert np.abs(bg - ref).max() <= 2e-5, np.abs(bg - ref).max()
    g = env_oracle.background_grad(gm, H, W, focal, R, GOLD[case + "/w"])
    gref = GOLD[case + "/g_grid"]
    assert np.abs(g - gref).max() <= 5e-5 * max(np.abs(gref).max(), 1.0)


def test_zero_padding_and_finite_difference():
    rng = np.random.default_rng(1)
    gm = rng.standard_normal((3, 16, 16))
    R = np.eye(3)
    bg = env_oracle.background(gm, 9, 11, 20.0, R)
    assert bg.shape == (3, 9, 11) and np.all((bg > 0) & (bg < 1))
    w = rng.standard_normal(bg.shape)
    g = env_oracle.background_grad(gm, 9, 11, 20.0, R, w)
    idx = np.unravel_index(np.argmax(np.abs(g)), g.shape)
    d = np.zeros_like(gm); d[idx] = 1e-5
    fd = ((env_oracle.background(gm + d, 9, 11, 20.0, R) - env_oracle.background(gm - d, 9, 11, 20.0, R)) * w).sum() / 2e-5
    assert abs(fd - g[idx]) <= 1e-6 * max(1.0, abs(g[idx]))


# ---- the launch-geometry helpers the GPU path tests (tests/test_gpu_env_paths.py) assert their premises with

def test_mirrored_kernel_constants_equal_the_source():
    from tests import env_cases as ec
    assert ec.kernel_constants() == (ec.TEXCAP, ec.MAXC, ec.BLOCK_W, ec.BLOCK_H) == (2048, 8, 64, 4)
    ec.assert_mirrors_kernel()


def test_unstable_pixels_are_the_seam_column_and_the_pole_pixel():
    from tests import env_cases as ec
    u = env_oracle.unstable_pixels(6, 8, 20.0, ec.CAM_NEG_X, ec.EPS)               # even W: the centre column has ry = 0, rx < 0
    expect = np.zeros((6, 8), bool); expect[:, 4] = True
    assert np.array_equal(u, expect)
    assert not env_oracle.unstable_pixels(6, 9, 20.0, ec.CAM_NEG_X, ec.EPS).any()  # odd W: the seam passes between two columns
    assert not env_oracle.unstable_pixels(6, 8, 20.0, ec.CAM_FRONT, ec.EPS).any()  # rx > 0: ry = 0 is no seam
    u = env_oracle.unstable_pixels(6, 8, 20.0, ec.CAM_POLE, ec.EPS)
    expect = np.zeros((6, 8), bool); expect[3, 4] = True                            # the principal point only
    assert np.array_equal(u, expect)
    wide = env_oracle.unstable_pixels(6, 8, 20.0, ec.CAM_NEG_X, 0.06)              # eps reaches the neighbours (|ry| ~ 1 / focal)
    assert wide[:, 3:6].all() and wide.sum() == 18


def test_block_boxes_equal_the_extent_of_the_in_map_taps():
    from tests import env_cases as ec
    H, W, focal, Hm, Wm = 9, 70, 30.0, 16, 40
    for R in (ec.CAM_GENERIC, ec.CAM_NEG_X, ec.CAM_POLE):
        bb = env_oracle.block_boxes(H, W, focal, R, Hm, Wm)
        assert bb.box.shape == (3, 2, 4) and bb.area.shape == (3, 2) and not bb.empty.any()
        ix, iy = env_oracle.sample_coords(H, W, focal, R, Hm, Wm)
        taps = list(env_oracle._corners(ix, iy, Hm, Wm))
        for by in range(3):
            for bx in range(2):
                sl = (slice(by * 4, by * 4 + 4), slice(bx * 64, bx * 64 + 64))
                xs = np.concatenate([xx[sl][ok[sl]] for xx, yy, w, ok in taps]); ys = np.concatenate([yy[sl][ok[sl]] for xx, yy, w, ok in taps])
                assert tuple(bb.box[by, bx]) == (xs.min(), ys.min(), xs.max(), ys.max())
                assert bb.area[by, bx] == (xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1)
    # another block shape regroups the same pixels; a mask that leaves a block no pixel flags it empty
    one = env_oracle.block_boxes(H, W, focal, ec.CAM_GENERIC, Hm, Wm, bw=70, bh=9)
    assert one.box.shape == (1, 1, 4) and one.area[0, 0] >= env_oracle.block_boxes(H, W, focal, ec.CAM_GENERIC, Hm, Wm).area.max()
    mask = np.ones((H, W), bool); mask[:, 64:] = False
    masked = env_oracle.block_boxes(H, W, focal, ec.CAM_GENERIC, Hm, Wm, pixel_mask=mask)
    assert masked.empty[:, 1].all() and (masked.area[:, 1] == 0).all() and not masked.empty[:, 0].any()


def test_seam_camera_on_a_wide_map_has_blocks_on_both_sides_of_the_lds_capacity():
    from tests import env_cases as ec
    bb = env_oracle.block_boxes(16, 192, 100.0, ec.CAM_NEG_X, 2, 4096, bw=ec.BLOCK_W, bh=ec.BLOCK_H)      # the seam at column 96: inside block 1
    assert (bb.area > ec.TEXCAP).any() and ((bb.area <= ec.TEXCAP) & ~bb.empty).any()
    assert (bb.area[:, [0, 2]] <= ec.TEXCAP).all()          # away from the seam 64 pixels span ~420 texel columns of 2 rows
    assert (bb.area[:, 1] > 2 * 4000).all()                 # pixels on both sides of the seam: both ends of the 2 x 4096 map


def test_pair_classes_on_hand_made_configurations():
    from tests import env_cases as ec
    S, A, N, P = env_oracle.SAME, env_oracle.ADJACENT, env_oracle.NEITHER, env_oracle.PARTNER_INVALID
    Hm, Wm, focal, R, _ = ec.PAIR_CONFIGS["same"]
    assert (Hm, Wm) == (4, 8)
    c = env_oracle.pair_classes(16, 128, focal, R, Hm, Wm)
    assert c.shape == (16, 64) and (c == S).mean() > 0.9 and not (c == P).any()
    Hm, Wm, focal, R, _ = ec.PAIR_CONFIGS["neither"]
    assert (Hm, Wm) == (16, 4096)
    c = env_oracle.pair_classes(16, 64, focal, R, Hm, Wm)
    assert (c == N).all()                                    # ~10 texel columns per pixel
    Hm, Wm, focal, R, _ = ec.PAIR_CONFIGS["adjacent"]
    assert 0.55 <= (Wm - 1) / (2 * np.pi * focal) <= 0.65    # texels per pixel along a row
    c = env_oracle.pair_classes(16, 128, focal, R, Hm, Wm)
    assert (c == A).mean() >= 0.4 and (c == S).mean() >= 0.2 and (c == N).mean() <= 0.05
    # the classes are decided by x0, y0 alone: check them against the coordinates
    ix, iy = env_oracle.sample_coords(16, 128, focal, R, Hm, Wm)
    x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
    for r, j in ((0, 0), (7, 31), (15, 63), (3, 40)):
        same_row = y0[r, 2 * j] == y0[r, 2 * j + 1]
        want = S if same_row and x0[r, 2 * j + 1] == x0[r, 2 * j] else A if same_row and x0[r, 2 * j + 1] == x0[r, 2 * j] + 1 else N
        assert c[r, j] == want
    # the mirrored camera walks the columns downwards: the odd pixel is at x0 - 1, which the kernel does not merge
    c = env_oracle.pair_classes(16, 128, focal, R @ np.diag([-1.0, 1.0, 1.0]).astype(np.float32), Hm, Wm)
    assert not (c == A).any() and (c == N).mean() >= 0.4
    for W in (1, 63, 65, 127):
        for name, (Hm, Wm, focal, R, _) in ec.PAIR_CONFIGS.items():
            c = env_oracle.pair_classes(5, W, focal, R, Hm, Wm)
            assert c.shape == (5, (W + 1) // 2) and (c == P).sum() == 5 and (c[:, -1] == P).all(), (name, W)


def test_tap_footprint_is_the_support_of_the_gradient():
    from tests import env_cases as ec
    H, W, focal, Hm, Wm = 9, 70, 30.0, 16, 40
    for R in (ec.CAM_GENERIC, ec.CAM_NEG_X):
        fp = env_oracle.tap_footprint(H, W, focal, R, Hm, Wm)
        g = env_oracle.background_grad(np.zeros((1, Hm, Wm)), H, W, focal, R, np.ones((1, H, W)))[0]
        assert fp.shape == (Hm, Wm) and fp.any() and not fp.all()
        assert not (g != 0)[~fp].any()                       # nothing lands outside the footprint
        assert (g != 0)[fp].mean() > 0.95                    # (a tap of weight exactly 0 is in the footprint)
        mask = np.zeros((H, W), bool); mask[2, 5] = True
        one = env_oracle.tap_footprint(H, W, focal, R, Hm, Wm, pixel_mask=mask)
        ix, iy = env_oracle.sample_coords(H, W, focal, R, Hm, Wm)
        x0, y0 = int(np.floor(ix[2, 5])), int(np.floor(iy[2, 5]))
        assert one.sum() == 4 and one[y0:y0 + 2, x0:x0 + 2].all()
        wide = env_oracle.tap_footprint(H, W, focal, R, Hm, Wm, slack=0.5)
        assert wide[fp].all() and wide.sum() > fp.sum()
    # a map below the image's footprint: taps beyond its last row / column are not counted
    fp = env_oracle.tap_footprint(4, 4, 2.0, ec.CAM_NEG_X, 2, 2)
    assert fp.shape == (2, 2) and fp.all()
