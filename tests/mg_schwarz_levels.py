"""Small device hierarchies with a Schwarz handle per level, shared by tests/test_vcycle_schwarz_gpu.py and tests/test_pc_gpu.py, and the
per-level callables of tests/ref_multigrid.py built from the DEVICE primitives (apply_lhs, Schwarz.iterate, the transfers): the
restatements then differ from the objects under test only in what those objects add -- the order of the calls, the workspace, the
fused kernels."""
import numpy as np

from tests import ref_multigrid as RM

RTOL = 1e-12          # the admitted difference per operator apply, as tests/test_vcycle_gpu.py
OVERLAP = 2


def t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _p_items(deg_c, deg_f):
    degh = np.zeros(8 * len(deg_f), dtype=np.int32)
    degh[0::8] = deg_f
    return np.zeros(len(deg_f), dtype=np.int32), np.asarray(deg_c, dtype=np.int32), degh


def meshes(kind):
    """(meshes coarsest first, transfer items per coarse level, SineMap amplitude).  'two': 64 elements p = 4 -> p = 2; 'three': the
    same and 8 elements p = 2 below (h-coarsened); 'mixed': p = 2..4 scattered -> p - 1; 'hanging': a level-1 brick with octants 1 and 6
    refined (the pattern of tests/test_schwarz_gpu.py), p = 2..4 -> p - 1 on the same elements"""
    from disco4est_amd import mesh as M
    if kind in ("two", "three"):
        d4, d2 = np.full(64, 4, np.int32), np.full(64, 2, np.int32)
        ms, items = [M.BrickMesh(2, d2), M.BrickMesh(2, d4)], [_p_items(d2, d4)]
        if kind == "three":
            d2c = np.full(8, 2, np.int32)
            ms.insert(0, M.BrickMesh(1, d2c))
            items.insert(0, (np.ones(8, np.int32), d2c, d2.copy()))
        return ms, items
    if kind == "mixed":
        df = (2 + (np.arange(64) * 7 % 3)).astype(np.int32)
        return [M.BrickMesh(2, df - 1), M.BrickMesh(2, df)], [_p_items(df - 1, df)]
    if kind == "hanging":
        refine = np.zeros(8, dtype=bool)
        refine[[1, 6]] = True
        n = M.HangingBrickMesh(1, refine, 2).n_elements
        df = (2 + (np.arange(n) % 3)).astype(np.int32)
        return [M.HangingBrickMesh(1, refine, df - 1), M.HangingBrickMesh(1, refine, df)], [_p_items(df - 1, df)]
    raise ValueError(kind)


class Levels:
    """plans, transfers and Schwarz objects of a hierarchy (level 0 = coarsest); sub = the subdomain CG options of every handle"""

    def __init__(self, kind, gpu, sub=(6, 1e-15, 1e-15), amplitude=0.03, coarse_prefactor=10.0, schwarz_levels=None):
        from disco4est_amd import Plan, Transfer, mesh as M
        from disco4est_amd.schwarz import Schwarz
        self.gpu, self.sub = gpu, sub
        self.mp = M.SineMap(amplitude)
        self.meshes, self.items = meshes(kind)
        self.n_levels = len(self.meshes)
        self.nodes = [m.local_nodes for m in self.meshes]
        self.plans, self.schwarz, self.geo = [], [], []
        for l, m in enumerate(self.meshes):
            J, rst = m.geometry(self.mp)
            sides = m.build_sides(self.mp)
            pref = 10.0 if l == self.n_levels - 1 else coarse_prefactor
            p = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0)
            p.set_geometry(J, rst)
            p.set_faces(sides, pref, 0)
            self.plans.append(p)
            self.geo.append((J, rst, sides, pref))
            want = schwarz_levels is None or l in schwarz_levels
            self.schwarz.append(self.new_schwarz(l) if want else None)
        self.transfers = [Transfer(h, dH, dh) for (h, dH, dh) in self.items]
        self.extra = []

    def new_schwarz(self, l, sub=None):
        from disco4est_amd.schwarz import Schwarz
        J, rst, sides, pref = self.geo[l]
        it, atol, rtol = sub or self.sub
        return Schwarz(self.meshes[l], sides, J, rst, OVERLAP, it, atol, rtol, pref, 0)

    def multigrid(self):
        from disco4est_amd import Multigrid
        mg = Multigrid(self.plans, self.transfers)
        self.extra.append(mg)
        return mg

    def problem(self, seed):
        from disco4est_amd import mesh as M
        n = self.nodes[-1]
        return M.splitmix64_uniform(seed, n) - 0.5, M.splitmix64_uniform(seed + 1, n) - 0.5

    # ---- the device primitives as numpy callables
    def apply(self, l, u, noise=None):
        import torch
        x = t(u, self.gpu)
        y = torch.empty_like(x)
        self.plans[l].apply_lhs(x, y)
        Au = y.cpu().numpy()
        if noise is not None:             # an admitted difference: relative-inf size RTOL
            Au = Au + RTOL * np.abs(Au).max() * (2.0 * noise.random(Au.size) - 1.0)
        return Au

    def schwarz_iterate(self, l, u, r):
        x = t(u, self.gpu)
        self.schwarz[l].iterate(x, t(r, self.gpu))
        return x.cpu().numpy()

    def prolong(self, l, x):
        import torch
        out = torch.empty(self.nodes[l + 1], dtype=torch.float64, device=self.gpu)
        self.transfers[l].prolong(t(x, self.gpu), out)
        return out.cpu().numpy()

    def restrict(self, l, x):
        import torch
        out = torch.empty(self.nodes[l], dtype=torch.float64, device=self.gpu)
        self.transfers[l].restrict(t(x, self.gpu), out)
        return out.cpu().numpy()

    def hierarchy(self, noise=None):
        return RM.Hierarchy(self.nodes, lambda l, u: self.apply(l, u, noise), None, None, self.prolong, self.restrict)

    def close(self):
        for o in self.extra:
            o.destroy()
        for z in self.schwarz:
            if z is not None:
                z.destroy()
        for x in self.transfers + self.plans:
            x.destroy()
