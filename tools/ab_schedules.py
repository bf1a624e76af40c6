"""A/B timing of stiffness-kernel builds AND tuning values in ONE process, interleaved rounds: every entry is a library (the product's,
or a variant of tools/build_variant.sh) plus tuning values, all on the same mesh and input.  Medians of 12 rounds x 50 launches after a
warm-up; listing an entry twice gives the spread of a variant against itself.

usage: python tools/ab_schedules.py LEVEL DEG[:DEG_HI] COUNT ENTRY...     (COUNT 0 = the whole level; DEG:DEG_HI = degrees interleaved)
       ENTRY = label[@variant-name]:key=value,key=value      e.g.  parent:16=0  new:16=1  old16:1=12  nofwd@ab1:16=0"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from disco4est_amd import Plan, capi, mesh as M  # noqa: E402

level = int(sys.argv[1])
dlo, _, dhi = sys.argv[2].partition(":")
dlo, dhi = int(dlo), int(dhi or dlo)
count = int(sys.argv[3]) or None
total = 8 ** level
deg = dlo if dhi == dlo else dlo + (np.arange(total) * 3) % (dhi - dlo + 1)
m = M.BrickMesh(level, deg, count=count)
J, rst = m.geometry(None)
dev = torch.device("cuda:0")
du = torch.from_numpy(m.field()).to(dev)
out = torch.empty_like(du)

entries = []
default_lib = capi.load_library()
libs = {None: default_lib}
for arg in sys.argv[4:]:
    head, _, kv = arg.partition(":")
    label, _, variant = head.partition("@")
    variant = variant or None
    if variant not in libs:
        libs[variant] = capi.load_library(os.path.join(ROOT, "disco4est_amd", "variants", "libd4est_hip_%s.so" % variant))
    capi._lib = libs[variant]   # Plan() binds the library that is current when it is created
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=torch.cuda.current_stream())
    plan.set_geometry(J, rst)
    plan.set_tuning(7, 0)       # general path
    for pair in filter(None, kv.split(",")):
        k_, v_ = pair.split("=")
        plan.set_tuning(int(k_), int(v_))
    entries.append((label, arg, plan, []))
capi._lib = default_lib

ROUNDS, STEPS = 12, 50
for _ in range(3):   # clocks settle
    for _, _, plan, _ in entries:
        for _ in range(STEPS):
            plan.apply_stiffness_matrix(du, out)
torch.cuda.synchronize()
for rnd in range(ROUNDS):
    for _, _, plan, times in entries:
        for _ in range(5):
            plan.apply_stiffness_matrix(du, out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(STEPS):
            plan.apply_stiffness_matrix(du, out)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / STEPS * 1e3)
print("level %d  p = %s  %d elements  %d nodes;  us per apply over %d rounds x %d launches" % (level, sys.argv[2], m.n_elements, m.local_nodes, ROUNDS, STEPS))
for label, arg, plan, times in entries:
    t = sorted(times)
    med = 0.5 * (t[ROUNDS // 2 - 1] + t[ROUNDS // 2])
    print("  %-10s median %7.2f  min %7.2f  max %7.2f  %6.1f GDoF/s   %s   [%s]" %
          (label, med, t[0], t[-1], m.local_nodes / med / 1e3, plan.last_kernel(), arg))
