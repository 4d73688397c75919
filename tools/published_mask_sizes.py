"""Size of the "published" set of the bench's frames: for every camera of the pool bench.py cycles through (default C3, 16 cameras) the
number of visible Gaussians, of published (tile, Gaussian) entries and of Gaussians the forward's published mask names
(include/adgs_testing.h: adgs_test_v2_published_mask).  python tools/published_mask_sizes.py OUT.json [CONFIG [CAMERAS]]
(profiles/published_mask/sizes_c3.json)."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bench                                                 # noqa: E402
from adgs import _lib, deform, synthetic                     # noqa: E402
from diff_gaussian_rasterization import _C                   # noqa: E402

out_path = sys.argv[1]
config = sys.argv[2] if len(sys.argv) > 2 else "C3"
n_cams = int(sys.argv[3]) if len(sys.argv) > 3 else 16
device = torch.device("cuda", 0)
cfg = dict(synthetic.CONFIGS[config])
sc = bench.build_scene(config)
pool = bench.camera_pool(cfg, n_cams)
frames = bench.frame_pool(sc, cfg, pool, device, True)
lib = _lib.lib()
rows = []
e = torch.empty(0, device=device)
for k, ((cam, t), f) in enumerate(zip(pool, frames)):
    s = bench.make_settings(cfg, cam, sc, device)
    with torch.no_grad():
        if isinstance(f, bench.DeformFrame):
            pkg = deform.get_deformed_pkg(f.model, t)
            flow = f.model.get_deformed_xyz(t + 0.05)
            ten = dict(means3D=pkg["xyz"], opacities=pkg["opacity"], scales=pkg["scales"], rotations=pkg["rotation"], shs=pkg["shs"])
        else:
            ten = {n: v.detach() for n, v in f.leaf.items()}
            flow = f.flow
        r = _C.rasterize_gaussians(s.bg, ten["means3D"], e, ten["opacities"], ten["scales"], ten["rotations"], s.scale_modifier, e, s.viewmatrix,
                                   s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, ten["shs"], flow, f.sem, s.sh_degree,
                                   s.campos, s.prefiltered, s.inv_depth, False)
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    P = ten["means3D"].shape[0]
    raw = np.zeros(P, np.uint8)
    assert lib.adgs_test_v2_published_mask(r[5].data_ptr(), P, raw.ctypes.data, None, st) == P
    bits = raw == 1
    vis = (r[4] > 0).cpu().numpy()
    assert not (bits & ~vis).any()
    g = lambda n: float(bits[:len(bits) // n * n].reshape(-1, n).any(1).mean())
    rows.append(dict(camera=k, t=round(t, 4), P=P, P_visible=int(vis.sum()), published_gaussians=int(bits.sum()),
                     published_entries=int(lib.adgs_test_v2_published_entries(r[7].data_ptr(), int(s.image_width), int(s.image_height), st)),
                     groups64_with_a_bit=round(g(64), 4), groups16_with_a_bit=round(g(16), 4), groups5_with_a_bit=round(g(5), 4)))
    print(rows[-1])
json.dump(dict(config=config, cameras=rows), open(out_path, "w"), indent=1)
