"""The device error estimator (d4est_hip_estimator_bi) against one apply_aij on the same plan: tools/time_estimator.py [level]
  config2 : level-4 brick, p = 7 (config 2's mesh)
  config4 : level-4 brick, p = 3 ... 9 graded smoothly (bench.graded_degrees), every 64th octant refined once (hanging faces)
Prints one JSON line: per mesh the estimator's and apply_aij's microseconds per call (HIP events, steady state) and their ratio."""
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


def meshes():
    yield "config2", M.BrickMesh(L, 7)
    refine = np.zeros(8 ** L, dtype=bool)
    refine[::64] = True
    gd = bench.graded_degrees(L)
    deg = np.concatenate([np.full(8 if refine[b] else 1, gd[b]) for b in range(8 ** L)]).astype(np.int32)
    yield "config4", M.HangingBrickMesh(L, refine, deg)


out = {"tool": "time_estimator", "level": L}
for name, m in meshes():
    J, rst = m.geometry(None)
    sides = m.build_sides(None)
    p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=st)
    p.set_geometry(J, rst)
    p.set_estimator(7, 8, 9, 10.0)
    p.set_faces(sides, 10.0, 0)
    u = torch.from_numpy(m.field()).to(dev)
    r = torch.from_numpy(M.splitmix64_uniform(3, m.local_nodes) - 0.5).to(dev)
    bx = sides["bndry_xyz"]
    g = torch.from_numpy(np.ascontiguousarray(bx[0] * bx[1])).to(dev)
    diam = torch.full((m.n_elements,), float(np.sqrt(3.0)) / (1 << L), dtype=torch.float64, device=dev)
    eta2 = torch.empty(m.n_elements, dtype=torch.float64, device=dev)
    terms = torch.empty(4 * m.n_elements, dtype=torch.float64, device=dev)
    Au = torch.empty_like(u)
    t_est = bench.time_region(lambda: p.estimator_bi(u, r, diam, eta2, terms=terms, g=g), 50, st, torch)
    t_aij = bench.time_region(lambda: p.apply_aij(u, Au), 50, st, torch)
    torch.cuda.synchronize()
    assert torch.isfinite(eta2).all()
    out[name] = {"elements": int(m.n_elements), "dofs": int(m.local_nodes), "estimator_us": round(1e3 * t_est, 1),
                 "apply_aij_us": round(1e3 * t_aij, 1), "ratio": round(t_est / t_aij, 2), "face_path": p.face_path()}
    p.destroy()
print(json.dumps(out))
