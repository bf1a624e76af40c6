"""The device error norms (csrc/d4est_hip_norms.hip) against one apply_aij on the same plan: tools/time_norms.py [level]
on config 2's mesh (level-4 brick, p = 7).  Prints one JSON line: microseconds per call (HIP events, steady state) of the error field,
the L2 norm, the L-infinity norm, the IP energy norm, a masked sum, and of one apply_aij."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disco4est_amd import Plan, mesh as M  # noqa: E402

spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)

L = int(sys.argv[1]) if len(sys.argv) > 1 else 4
dev = torch.device("cuda:0")
st = torch.cuda.current_stream()

m = M.BrickMesh(L, 7)
J, rst = m.geometry(None)
sides = m.build_sides(None)
p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=st)
p.set_geometry(J, rst)
p.set_energy_norm(0, 10.0)
p.set_faces(sides, 10.0, 0)
u = torch.from_numpy(m.field()).to(dev)
c = torch.from_numpy(M.splitmix64_uniform(3, m.local_nodes) - 0.5).to(dev)
skip = torch.from_numpy((np.arange(m.n_elements) % 3 == 0).astype(np.int32)).to(dev)
err, Au = torch.empty_like(u), torch.empty_like(u)
arr = torch.empty(m.n_elements, dtype=torch.float64, device=dev)
terms = torch.empty(3 * m.n_elements, dtype=torch.float64, device=dev)
one, sums = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
regions = {
    "norms_error_us": lambda: p.norms_error(u, c, err),
    "norm_l2_sqr_us": lambda: p.norm_l2_sqr(err, one, skip=skip, l2_array=arr),
    "norm_linfty_us": lambda: p.norm_linfty(err, one, skip=skip),
    "ip_energy_norm_sqr_us": lambda: p.ip_energy_norm_sqr(err, sums, elem_terms=terms),
    "masked_sum_us": lambda: p.masked_sum(arr, one, skip=skip),
    "apply_aij_us": lambda: p.apply_aij(u, Au),
}
out = {"tool": "time_norms", "level": L, "elements": int(m.n_elements), "dofs": int(m.local_nodes), "face_path": p.face_path()}
for name, fn in regions.items():
    out[name] = round(1e3 * bench.time_region(fn, 50, st, torch), 1)
torch.cuda.synchronize()
assert torch.isfinite(sums).all()
p.destroy()
print(json.dumps(out))
