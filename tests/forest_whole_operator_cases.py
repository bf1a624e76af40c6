"""Case lists of tests/test_forest_whole_operator_gpu.py (the whole-operator kernels on faces BETWEEN trees) -- a plain module so that
tests/test_forest_whole_operator_cases.py can prove, without a GPU, that every list covers what the GPU module claims for it.

Every entry is ((f_m, f_p, orientation), (rot_a, rot_b)) out of tests.test_forest.TRIPLES: tree 0 of
forest.Connectivity.rotated_pair(rot_a, rot_b) sees its glued face as f_m, tree 1's as f_p, tree 1 sees the pair the other way round.
Nothing here loads a library: the reorder code comes from forest.face_reorder_code (held to the library's and the oracle's in
tests/test_forest.py)."""
from disco4est_amd import forest as F
from tests.test_forest import TRIPLES

SORTED = sorted(TRIPLES.items())


def code_of(trip):
    """the reorder code of the glued face (one code for both views: the reference expands the transform of (lower face, higher face))"""
    return F.face_reorder_code(*trip)


def geometric(trip):
    """the reference's re-orientation is the geometric one as seen from tree 0"""
    return F.reference_reorientation_is_consistent(*trip)


def geometric_both(trip):
    return geometric(trip) and F.reference_reorientation_is_consistent(trip[1], trip[0], trip[2])


def _completed(base, pool, key, wanted):
    """base plus the first entries of pool that bring a still missing value of key(trip) in"""
    out = list(base)
    have = {key(t) for t, _ in out}
    for t, r in pool:
        if key(t) in wanted and key(t) not in have:
            have.add(key(t))
            out.append((t, r))
    return out


# ---- 1: uniform degree, both trees in memory (kind 1), level 0 ------------------------------------------------------------------------------
ALL = SORTED
FIFTH = SORTED[::5]          # what test_forest_gpu.py samples for its larger degrees
# The triples are sorted with the orientation running fastest (period 4), so a stride of 10 only ever meets orientations 0 and 2 and with
# them the codes {0, 2, 4, 5}.  Every 10th triple it is -- plus the first triple of FIFTH for each of the codes a stride of 10 cannot reach.
TENTH = _completed(SORTED[::10], FIFTH, code_of, set(range(8)))

# (deg, deg_quad_inc, list) per kernel family; the (N, NQ) = (4, 6) instance stands for the deg_quad > deg pairs of D4EST_HIP_DIRECT_PAIRS
SINGLE_WAVE = [(1, 0, ALL), (3, 0, ALL), (7, 0, FIFTH), (3, 2, FIFTH)]
MULTI_WAVE = [(8, 0, FIFTH), (11, 0, FIFTH), (15, 0, TENTH)]


def _one_per_code(ok=lambda t: True, codes=range(8), spread=19):
    """one triple per code; the search for code c starts ``spread * c`` entries into the sorted list, so that the faces vary with the code"""
    out = []
    for c in codes:
        pool = SORTED[(spread * c) % len(SORTED):] + SORTED[:(spread * c) % len(SORTED)]
        out.append(next((t, r) for t, r in pool if code_of(t) == c and ok(t)))
    return out


# level 1, 16 elements: oriented sides (across the tree face) and code-0 sides (inside a tree) in one launch; one triple per code, and
# between them every face as f_m and as f_p
LEVEL1 = _one_per_code()

# ---- 2: Chebyshev with the fused update: the codes the cubed sphere does not have --------------------------------------------------------
CHEBY = _one_per_code(codes=(4, 5, 6), spread=31)

# ---- 3: one tree per rank (every ghost side is the tree face); tree 0's view is geometric, as in test_hybrid_ghost_gpu.py ------------------
# (rank 0's ghost sides see f_p, rank 1's see f_m as the neighbour's face: a face missing from both is brought in by one more triple)
GHOST = _one_per_code(geometric, spread=23)
GHOST += [next(e for e in SORTED if geometric_both(e[0]) and e[0][2] != 0 and f in e[0][:2])
          for f in range(6) if not any(f in t[:2] for t, _ in GHOST)]

# ---- 4: the hybrid operator's forms (degrees <= 7) ---------------------------------------------------------------------------------------
MIXED = LEVEL1
HANGING = FIFTH
HANGING_REFINES = ([1, 0], [0, 1])


def hanging_small_view(trip, refine):
    """the small sides' view of the hanging face (the refined tree's)"""
    return trip if list(refine) == [1, 0] else (trip[1], trip[0], trip[2])


def level1_degrees(conn_trees, high_tree, top):
    """16 degrees (two level-1 trees): ``top`` and ``top - 1`` in a checkerboard inside the tree ``high_tree``, two below that in the
    other -- every face of a tree has elements of either parity, so on the glued face elements of the top degree meet lower ones across it"""
    assert conn_trees == 2
    out = []
    for t in range(2):
        for i in range(8):
            par = bin(i).count("1") & 1
            out.append((top - par) if t == high_tree else (top - 2 - par))
    return out


def hanging_degrees(sides, n_elements, top, big_higher):
    """9 degrees of a two-tree mesh with one tree refined: the small elements ON the hanging face get ``top``, the other small elements
    ``top - 1``, the big element ``top`` (or ``top + 1``: then no small side can take the kind-2 override)"""
    deg = [top - 1] * n_elements
    for s in range(6 * n_elements):
        if sides["side_hang"][s] == 2:
            deg[s // 6] = top
        elif sides["side_hang"][s] == 1:
            deg[s // 6] = top + (1 if big_higher else 0)
    return deg


# ---- what a mesh's side tables say (both test modules read them through these) -----------------------------------------------------------
def interior_sides(m, sides):
    """(side, neighbour element) of every side against a local element"""
    return [(s, int(n)) for s, n in enumerate(sides["side_nbr"]) if n >= 0]


def tree_face_sides(m, sides):
    """the interior sides on the face between the two trees"""
    return [(s, n) for s, n in interior_sides(m, sides) if m.tree[s // 6] != m.tree[n]]


def coverage(m, sides, which):
    """codes, neighbour faces f_p, (d, dn) direction pairs, own face ends h and neighbour face ends of the listed (side, neighbour)s"""
    cov = dict(codes=set(), f_p=set(), d_dn=set(), h=set(), h_p=set())
    for s, _ in which:
        f, fp = s % 6, int(sides["side_nbr_face"][s])
        cov["codes"].add(int(sides["side_reorder"][s]))
        cov["f_p"].add(fp)
        cov["d_dn"].add((f // 2, fp // 2))
        cov["h"].add(f & 1)
        cov["h_p"].add(fp & 1)
    return cov


def merge(total, cov):
    for k, v in cov.items():
        total.setdefault(k, set()).update(v)
    return total


def clean_without_higher_neighbour(m, sides):
    """The hybrid operator's rule on a conforming one-rank plan with every degree <= 7 and deg_quad = deg (csrc/d4est_hip_faces_setup.hip,
    "the hybrid operator"): an element is clean -- the one-kernel path -- unless a neighbour has a HIGHER degree; a neighbour of lower
    degree is read from the trace array (mixed-aware form, override kind 2)."""
    clean = [True] * m.n_elements
    for s, n in interior_sides(m, sides):
        if m.deg[n] > m.deg[s // 6]:
            clean[s // 6] = False
    return clean


def mixed_aware_tree_face_codes(m, sides):
    """reorder codes of the tree-face sides that a CLEAN element owns against a neighbour of lower degree"""
    clean = clean_without_higher_neighbour(m, sides)
    return {int(sides["side_reorder"][s]) for s, n in tree_face_sides(m, sides) if clean[s // 6] and m.deg[n] < m.deg[s // 6]}
