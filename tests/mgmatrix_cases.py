"""The case lists of tests/test_mgmatrix_sweep_gpu.py.  TEST INFRASTRUCTURE.  tests/test_mgmatrix_dense.py proves on the CPU, with the
rule restatements of tests/dense_mgmatrix.py, that these lists reach every launch shape of the matrix-operator kernels; if the library's
rule for cutting rows or columns into workgroups changes, that test goes red and the cases have to be picked again."""
import numpy as np


RTOL = 1e-12          # the tolerance of every matrix-operator test, relative to the max norm of the reference


# ---- the two hierarchies of tests/test_mgmatrix_gpu.py (shared with the CPU pins of the dense forms) -----------------------------
def hierarchy(kind):
    """list of meshes, finest first, and the transfer item lists between consecutive levels (coarse <- fine)"""
    from disco4est_amd import mesh as M
    if kind == "hp3":
        # level 2 brick (64 elements, p = 2..4 scattered so that the eight children of a parent differ) -> h-coarsened level 1 brick
        # (degH = the smallest child degree, d4est_solver_multigrid_callbacks.h:52-75) -> p-coarsened (deg - 1, :9-20)
        deg2 = (2 + (np.arange(64) * 7 + (np.arange(64) // 8)) % 3).astype(np.int32)
        deg1 = deg2.reshape(8, 8).min(axis=1).astype(np.int32)
        deg0 = np.maximum(deg1 - 1, 1).astype(np.int32)
        meshes = [M.BrickMesh(2, deg2, deg_quad_inc=1), M.BrickMesh(1, deg1, deg_quad_inc=1), M.BrickMesh(1, deg0, deg_quad_inc=1)]
        items = [(np.ones(8, np.int32), deg1, deg2.copy()),
                 (np.zeros(8, np.int32), deg0, np.ascontiguousarray(np.stack([deg1] + [np.zeros(8, np.int32)] * 7, axis=1).reshape(-1)))]
        return meshes, items
    if kind == "hanging2":
        # fine: level-1 brick with octants 1 and 6 refined (22 elements, hanging faces), p = 2 / 3; coarse: the level-1 brick -- the refined
        # octants coarsen (eight children -> parent), the others are copied (the reference's third case) or lose one degree
        refine = np.zeros(8, dtype=bool)
        refine[[1, 6]] = True
        n_el = 8 - 2 + 16
        degf = (2 + (np.arange(n_el) * 5) % 2).astype(np.int32)
        mf = M.HangingBrickMesh(1, refine, degf, deg_quad_inc=0)
        hrefine, degH, degh = [], [], []
        k = 0
        for b in range(8):
            dh = np.zeros(8, np.int32)
            if refine[b]:
                dh[:] = degf[k:k + 8]
                hrefine.append(1); degH.append(int(dh.min())); k += 8
            else:
                dh[0] = degf[k]
                hrefine.append(0); degH.append(int(degf[k]) - (1 if b % 2 == 0 else 0)); k += 1   # p-coarsened or copied
            degh.append(dh)
        degH = np.array(degH, np.int32)
        mc = M.BrickMesh(1, degH, deg_quad_inc=0)
        return [mf, mc], [(np.array(hrefine, np.int32), degH, np.concatenate(degh))]
    raise ValueError(kind)


def degrees(level, deg):
    """deg: an int (uniform) or a tuple of degrees dealt out to the 8^level elements in a fixed scattered pattern"""
    n = 8 ** level
    if isinstance(deg, int):
        return np.full(n, deg, dtype=np.int32)
    k = np.arange(n)
    return np.asarray(deg, dtype=np.int32)[(k * 7 + k // 8) % len(deg)]


def buckets(level, deg):
    """[(degree, number of elements)] of the plan's buckets (one per degree: deg_quad - deg is the same for every element)"""
    d = degrees(level, deg)
    return [(int(p), int((d == p).sum())) for p in sorted(set(d.tolist()))]


# ---- (a) block matvec: (name, level, deg, layout of the blocks) ------------------------------------------------------------------
# layout "consecutive": block_offset = None; "reversed": explicit offsets, the blocks stored in reverse element order; "shared":
# explicit offsets, every odd element reads the block of the element before it (a Schwarz subdomain plan's copies read the mesh
# element's block in the same way)
MATVEC_CASES = [
    ("l4-p1", 4, 1, "consecutive"),          # rows = 64, N3 = 8: fewer columns than lanes, one chunk shorter than rows
    ("l4-p2", 4, 2, "consecutive"),          # rows = 64, N3 = 27: four trips, the last one ragged
    ("l3-p4", 3, 4, "consecutive"),          # rows = 16, N3 = 125: last chunk 13 rows
    ("l3-p6", 3, 6, "consecutive"),          # rows = 32, N3 = 343: last chunk 23 rows
    ("l1-p1", 1, 1, "consecutive"),          # rows = 8 from here on
    ("l1-p5", 1, 5, "consecutive"),
    ("l1-p6", 1, 6, "consecutive"),          # last chunk 7 rows
    ("l1-p8", 1, 8, "consecutive"),          # last chunk 1 row
    ("l1-p9", 1, 9, "consecutive"),
    ("l1-p11", 1, 11, "consecutive"),
    ("l2-p2p3-reversed", 2, (2, 3), "reversed"),   # two buckets in one apply, explicit block_offset
    ("l1-p3-shared", 1, 3, "shared"),
]


def block_layout(deg, layout):
    """(block_offset or None, number of doubles in the block array) for per-element degrees deg"""
    n6 = (np.asarray(deg, dtype=np.int64) + 1) ** 6
    if layout == "consecutive":
        return None, int(n6.sum())
    if layout == "reversed":
        off = np.zeros(n6.size, dtype=np.int64)
        off[::-1] = np.concatenate([[0], np.cumsum(n6[::-1])[:-1]])
        return off, int(n6.sum())
    if layout == "shared":
        assert (n6 == n6[0]).all()
        return (np.arange(n6.size, dtype=np.int64) // 2) * n6[0], int(n6[0] * ((n6.size + 1) // 2))
    raise ValueError(layout)


# ---- (b) weighted mass blocks: (level, deg, deg_quad_inc); every case runs with Gauss and Lobatto quadrature, with and without a
# coefficient ------------------------------------------------------------------------------------------------------------------
MASS_CASES = [(1, p, inc) for p in (1, 2, 3, 5, 6, 7, 8, 9, 11) for inc in (0, 1, 2, 3)]
MASS_CASES += [(2, (2, 3, 4), 1),           # three buckets
               (4, 1, 1)]                   # 4096 elements: ONE workgroup per element loops over all eight columns


# ---- (c) Galerkin restriction of the blocks: name -> (hrefine, degH, degh[8 k + c]) ----------------------------------------------
def _h_items(n, dH, dh):
    dh = np.asarray(dh, dtype=np.int32)
    return np.ones(n, np.int32), np.full(n, dH, np.int32), np.tile(dh if dh.size == 8 else np.full(8, int(dh), np.int32), n)


def _p_items(n, dH, dh):
    degh = np.zeros(8 * n, np.int32)
    degh[0::8] = dh
    return np.zeros(n, np.int32), np.full(n, dH, np.int32), degh


def _concat(*parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


GALERKIN_CASES = {
    "h-p1": _h_items(2, 1, 1),
    "h-p5": _h_items(1, 5, 5),
    "h-p6": _h_items(1, 6, 6),
    "h-p8": _h_items(1, 8, 8),
    "h-p1to6": _h_items(2, 1, [1, 2, 3, 4, 5, 6, 3, 2]),                 # eight children of different degrees, degH = the minimum
    "p-6to5": _p_items(3, 5, 6),
    "p-9to8": _p_items(2, 8, 9),
    "p-11to7": _p_items(2, 7, 11),
    "h-p2-with-copied-p8": _concat(_h_items(1, 2, 2), _p_items(1, 8, 8)),   # small children under a large max_n
    "h-p2-512-items": _h_items(512, 2, 2),                               # a level-4 fine brick: several columns per workgroup
}


def galerkin_shape(case):
    """(n_items, n_children, max_n^3, [Nh^3 of every child]) of a case, as d4est_hip_transfer_create counts them"""
    hrefine, degH, degh = GALERKIN_CASES[case]
    nh3, max_n = [], 0
    for k in range(hrefine.size):
        for c in range(8 if hrefine[k] == 1 else 1):
            nh3.append(int(degh[8 * k + c] + 1) ** 3)
            max_n = max(max_n, int(degh[8 * k + c]) + 1, int(degH[k]) + 1)
    return int(hrefine.size), len(nh3), max_n ** 3, nh3
