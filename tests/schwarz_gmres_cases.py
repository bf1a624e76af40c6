"""The meshes, right-hand sides and options shared by tests/test_ref_schwarz_gmres.py (CPU: the restatement on the oracle's subdomain
operator) and tests/test_schwarz_gmres_gpu.py (the device GMRES against the restatement on the device's own subdomain operator).

Meshes (name -> mesh, overlap):
    corner    brick level 1, p = 2, overlap 2: 8 subdomains of 8 elements, every face kind of a corner
    interior  brick level 2, p = 2, overlap 2: 64 subdomains, the interior ones have 27 copies.  (Overlap 1 cannot be built: the hat
              weights of d4est_solver_schwarz_operators.c:27-40 are 0 / 0 on a zero-width ramp and SchwarzMetadata refuses it; 2 is
              the smallest overlap there is.)
    mixed     brick level 1, degrees 2 / 3 alternating, overlap 2
    hanging   brick level 1 with octant 0 refined (hanging 1 <-> 4 faces), p = 2, overlap 2
"""
import numpy as np

NAMES = ("corner", "interior", "mixed", "hanging")
SEED = 4242                                  # the mesh residual of every case: splitmix64_uniform(SEED, nodes) - 0.5
FIXED = dict(mr=4, cycles=2, atol=1e-300, rtol=1e-300)            # case 1: fixed work, 8 inner steps
CONVERGENT = dict(mr=6, cycles=4, atol=1e-6, rtol=1e-6)           # case 2
MARGINAL = 1e-6                              # a subdomain with a stop test this close to its threshold may be excused
EXCUSED_SHARE = 0.10


def build(name):
    """(mesh, mapping, J, rst, sides, overlap)"""
    from disco4est_amd import mesh as M
    mp = M.SineMap(0.04)
    if name == "corner":
        m = M.BrickMesh(1, 2)
    elif name == "interior":
        m = M.BrickMesh(2, 2)
    elif name == "mixed":
        m = M.BrickMesh(1, (2 + np.arange(8) % 2).astype(np.int32))
    elif name == "hanging":
        refine = np.zeros(8, dtype=bool)
        refine[0] = True
        n = M.HangingBrickMesh(1, refine, 2).n_elements
        m = M.HangingBrickMesh(1, refine, np.full(n, 2, dtype=np.int32))
    else:
        raise KeyError(name)
    J, rst = m.geometry(mp)
    sides = m.build_sides(mp)
    return m, mp, J, rst, sides, 2


def residual(m):
    from disco4est_amd import mesh as M
    return M.splitmix64_uniform(SEED, m.local_nodes) - 0.5


def excused(results):
    """indices of the subdomains whose restatement run has a stop test within MARGINAL of its threshold"""
    return [s for s, r in enumerate(results) if r.min_margin() < MARGINAL]
