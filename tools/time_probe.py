"""Times the device point probes (d4est_hip_probe_*) on one GPU: 1, 1 000 and 1 000 000 random points on config 2's mesh (the brick at
level 4, p = 7: 4096 elements) and on the 13-tree cubed sphere (level 2, p = 7: 832 elements, compactified outer shell).

Per case: create with the points already on the device (allocations, the locate kernel, its synchronisation; a host clock), eval of one
field and eval + eval_gradient(physical) (medians of the timed calls, events on the plan's stream), and the only route there was before:
a device-to-host copy of u plus the numpy evaluation of tests/dense_probe.py on the located points (host clock; the host search is not
included -- a Python loop over points x elements is no comparator).  Also the bytes of u an eval reads, 8 N^3 per point, over its time.

    python tools/time_probe.py [--reps 20] [--host-points 1000000]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_us(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def _host_route(u_dev, ns, deg, rst, R, chunk=20000):
    """u to the host, then the numpy evaluation: (seconds value only, seconds value + physical gradient)"""
    from tests import dense_probe as dp
    t0 = time.perf_counter()
    u = u_dev.cpu().numpy()
    for s in range(0, ns.size, chunk):
        dp.evaluate(u, ns[s:s + chunk], deg[s:s + chunk], rst[s:s + chunk])
    t1 = time.perf_counter()
    for s in range(0, ns.size, chunk):
        g, _ = dp.gradient_ref(u, ns[s:s + chunk], deg[s:s + chunk], rst[s:s + chunk])
        dp.physical(g, R[s:s + chunk])
    t2 = time.perf_counter()
    return t1 - t0, (t1 - t0) + (t2 - t1)


def _case(name, plan, cells, root_len, n_trees, set_map, drdx, n_points, reps, host_points, dev):
    import torch
    from disco4est_amd import Probe, capi, mesh as M
    lib = capi.load_library()
    abc = M.splitmix64_uniform(31 + n_points, 3 * n_points).reshape(n_points, 3)
    tree = (M.splitmix64_uniform(7 + n_points, n_points) * n_trees).astype(np.int32)
    d_tree, d_abc = torch.from_numpy(tree).to(dev), torch.from_numpy(abc).to(dev)
    d_cells = [torch.from_numpy(np.ascontiguousarray(np.asarray(c).reshape(-1), dtype=np.int32)).to(dev) for c in cells]
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        h = lib.d4est_hip_probe_create(plan.handle, n_points, ptr(d_tree), ptr(d_abc), ptr(d_cells[0]), ptr(d_cells[1]), ptr(d_cells[2]),
                                       float(root_len), 1)
        ts.append(time.perf_counter() - t0)
        lib.d4est_hip_probe_destroy(h)
    create_us = min(ts) * 1e6
    pr = Probe(plan, tree, abc, cells, root_len)
    set_map(pr)
    err, elem, rst = pr.info()
    assert (err == 0).all()
    ns, deg = pr.element_info()
    u = torch.rand(plan.local_nodes, dtype=torch.float64, device=dev)
    out = torch.empty(n_points, dtype=torch.float64, device=dev)
    grad = torch.empty(3 * n_points, dtype=torch.float64, device=dev)
    val_us = _median_us(lambda: pr.eval(u, out), reps)

    def both():
        pr.eval(u, out)
        pr.eval_gradient(u, grad, physical=True)
    both_us = _median_us(both, reps)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())
    nh = min(n_points, host_points)
    hv, hb = _host_route(u, ns[:nh], deg[:nh], rst[:nh], drdx(tree[:nh], abc[:nh], elem[:nh]))
    scale = n_points / nh
    gbs = float(((deg.astype(np.int64) + 1) ** 3).sum()) * 8.0 / val_us * 1e-3
    print("| %s | %d | %.1f | %.1f | %.1f | %.0f | %.3g%s | %.3g%s |" % (name, n_points, create_us, val_us, both_us, gbs, hv * scale * 1e6,
                                                                       "" if nh == n_points else " (extrapolated from %d)" % nh, hb * scale * 1e6,
                                                                       "" if nh == n_points else " (extrapolated)"))
    pr.destroy()


def main():
    import torch
    from disco4est_amd import Plan, capi, forest as F, mesh as M
    from tests import dense_probe as dp
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-points", type=int, default=1000000, help="points the host route is timed on (fewer: extrapolated linearly)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("| mesh | points | create, points on the device (us) | eval (us) | eval + physical gradient (us) | u read by eval (GB/s) | "
          "copy u to the host + numpy value (us) | + numpy physical gradient (us) |")
    print("|---|---|---|---|---|---|---|---|")
    extents = (0., 1., 0., 1., 0., 1.)
    m = M.BrickMesh(4, 7)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
    dq = np.ones(m.n_elements)
    for n in (1, 1000, 1000000):
        _case("brick level 4, p = 7 (4096 elements)", plan, m.cells(), m.root_len, 1, lambda pr: pr.set_map(capi.GEOM_BRICK, extents),
              lambda tree, abc, elem: dp.drdx_brick(extents, dq[elem], m.root_len), n, args.reps, args.host_points, dev)
    plan.destroy()
    mp = F.CubedSphere13Map(1.0, 2.0, 6.0, compactify_outer=True)
    fm = F.ForestMesh(F.cubed_sphere_13tree_connectivity(), 2, 7, mp)
    plan = Plan(fm.deg, fm.deg_quad, fm.nodal_stride, fm.quad_stride, 0)

    def sphere_drdx(tree, abc, elem):
        D = np.empty((tree.size, 3, 3))
        for t in range(13):
            sel = np.nonzero(tree == t)[0]
            if sel.size:
                D[sel] = mp.jacobian(t, abc[sel]) * (0.5 * fm.size[elem[sel]] / fm.nf)[:, None, None]
        return np.linalg.inv(D)
    for n in (1, 1000, 1000000):
        _case("13-tree sphere level 2, p = 7 (832 elements)", plan, fm.cells(), fm.nf, 13, lambda pr: pr.set_map(mp.GEOM_TYPE, mp.params),
              sphere_drdx, n, args.reps, args.host_points, dev)
    plan.destroy()


if __name__ == "__main__":
    main()
