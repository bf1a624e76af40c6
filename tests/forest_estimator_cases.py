"""Case lists of tests/test_forest_estimator_gpu.py (the estimator's and the energy norm's face kernels on faces BETWEEN trees) -- a plain
module so that tests/test_forest_estimator_dense.py can prove, without a GPU, what every list covers.  The (f_m, f_p, orientation) lists
themselves are those of tests/forest_whole_operator_cases.py, unchanged; here: which list runs at which degrees, the degree layouts, and
what a mesh's side tables say about its tree face.  Nothing here loads a library."""
import numpy as np

from tests import forest_whole_operator_cases as C

# ---- 1: conforming, level 0, two elements: (degree(s), deg_quad_inc, list, id) ---------------------------------------------------------------
# p = 2 over-integrated: NQ != N; p = 9: the p >= 8 buckets; [2, 3] / [3, 2]: a degree jump across the oriented face, deg_mq = max, either
# tree the higher one
CONFORMING = [(2, 1, "ALL", "p2q3-all"), (3, 0, "ALL", "p3-all"), (7, 0, "FIFTH", "p7-fifth"), (9, 0, "FIFTH", "p9-fifth"),
              ([2, 3], 1, "FIFTH", "p2p3-fifth"), ([3, 2], 1, "FIFTH", "p3p2-fifth")]

# mesh.SineMap displaces by sin(pi X) sin(pi Y) sin(pi Z): on the glued face X = 1 of two level-0 trees its Jacobian varies with
# sin(pi Y) sin(pi Z), which every flip and the transposition of the unit square map to itself -- the mortar factors (sj, n, dr/dx, h) of
# such a face look the same under all eight reorder codes, so these two-element meshes cannot see in which order est_geom_kernel reads
# the (+) side's dr/dx (tests/test_forest_estimator_dense.py::test_the_sine_map_is_symmetric_on_the_level0_face pins this; from level 1
# on, and on a hanging face, the sub-faces are off-centre and the order shows).  So the families in which the factor kernel's path
# changes -- NQ != N, the p >= 8 buckets, the degree jumps -- run a second time on a warp without that symmetry.
ASYMMETRIC = [(2, 1, "FIFTH", "p2q3-fifth-skew"), (9, 0, "FIFTH", "p9-fifth-skew"), ([2, 3], 1, "FIFTH", "p2p3-fifth-skew"),
              ([3, 2], 1, "FIFTH", "p3p2-fifth-skew")]


class SkewSineMap:
    """mesh.SineMap with unequal frequencies and phases, x = X + a sin(.7 pi X + .2) sin(.9 pi Y + .4) sin(.6 pi Z + .1) c: a smooth
    invertible warp of physical space (|grad| < 0.12 at a = 0.03) that has no symmetry on the plane X = 1 and bends that plane too"""

    def __init__(self, amplitude=0.03, c=(1.0, -0.7, 0.4), freq=(0.7, 0.9, 0.6), phase=(0.2, 0.4, 0.1)):
        self.a, self.c = amplitude, np.asarray(c, dtype=np.float64)
        self.k, self.ph = np.pi * np.asarray(freq, dtype=np.float64), np.asarray(phase, dtype=np.float64)

    def x(self, X, Y, Z):
        s = self.a * np.sin(self.k[0] * X + self.ph[0]) * np.sin(self.k[1] * Y + self.ph[1]) * np.sin(self.k[2] * Z + self.ph[2])
        return X + self.c[0] * s, Y + self.c[1] * s, Z + self.c[2] * s

    def jacobian(self, X, Y, Z):
        arg = [self.k[0] * X + self.ph[0], self.k[1] * Y + self.ph[1], self.k[2] * Z + self.ph[2]]
        sn, cs = [np.sin(v) for v in arg], [np.cos(v) for v in arg]
        g = self.a * np.stack([self.k[0] * cs[0] * sn[1] * sn[2], self.k[1] * sn[0] * cs[1] * sn[2], self.k[2] * sn[0] * sn[1] * cs[2]], axis=-1)
        DF = np.zeros(np.shape(X) + (3, 3), dtype=g.dtype)
        for i in range(3):
            DF[..., i, :] = self.c[i] * g
            DF[..., i, i] += 1.0
        return DF


# ---- 2: level 1, 16 elements, oriented and code-0 sides in one launch (also the pointwise estimator's list) --------------------------------
LEVEL1_DEG = 3

# ---- 3: the hanging face ON the tree boundary: C.HANGING x C.HANGING_REFINES ----------------------------------------------------------------
HANGING_DEG = 2      # the smallest base degree of tests/test_forest_gpu.py::test_apply_aij_hanging_across_trees


def hanging_degrees(trip, refine, n_elements):
    """The degree layout of test_apply_aij_hanging_across_trees: HANGING_DEG + (7 e mod 3) per element where the reference's re-orientation
    is geometric from the small sides' view; one degree elsewhere (sub-mortars of several quadrature degrees on such a face: faces_setup
    aborts: csrc/d4est_hip_faces_setup.hip, "plan_set_hanging: small side ...: its sub-mortars have different quadrature degrees")."""
    if C.geometric(C.hanging_small_view(trip, refine)):
        return HANGING_DEG + (np.arange(n_elements) * 7) % 3
    return np.full(n_elements, HANGING_DEG)


# ---- 4: one level-1 tree per rank -----------------------------------------------------------------------------------------------------------
GHOST_DEG = 3
GHOST_PARTS = [(0, 8), (8, 8)]

LISTS_USED = ("ALL", "FIFTH", "LEVEL1", "HANGING", "GHOST")


# ---- what a mesh's side tables say ----------------------------------------------------------------------------------------------------------
def ghost_sides(sides):
    """(side, None) of every side against a ghost element"""
    return [(int(s), None) for s in np.nonzero(np.asarray(sides["side_nbr"]) <= -2)[0]]


def view_geometric(trip, tree):
    """the reference's re-orientation is the geometric one as the element of ``tree`` (0 or 1) sees the glued face"""
    return C.geometric(trip if tree == 0 else (trip[1], trip[0], trip[2]))
