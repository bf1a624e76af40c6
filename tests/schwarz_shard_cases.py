"""The sharded Schwarz cases shared by tests/test_schwarz_exchange_lists.py (CPU) and tests/test_schwarz_sharded_gpu.py: the brick and
hanging meshes tests/test_parallel_gpu.py uses for the Python composition (SchwarzShard), their partitions, and the per-rank exchange
lists of d4est_hip_schwarz_set_element_exchange built without a device."""
import numpy as np

# (world, level, degrees, overlap, curved)
BRICK = [(2, 2, [2], 2, False), (3, 2, [2, 3], 2, True), (4, 2, [3], 3, True)]
# (world, refined octants of the level-1 brick, degrees, overlap): tests/test_parallel_gpu.py::test_schwarz_virtual_ranks_hanging_mesh
HANGING = [(2, [0, 7], [2], 2), (3, [1, 2, 4], [2, 3], 2)]


def brick_case(world, level, deg_spec):
    from disco4est_amd import parallel as P
    n_global = 8 ** level
    deg_global = np.array([deg_spec[i % len(deg_spec)] for i in range(n_global)], dtype=np.int32)
    return deg_global, P.partition_by_dofs(deg_global, world)


def hanging_case(world, pattern, deg_spec):
    from disco4est_amd import mesh as M, parallel as P
    refine = np.zeros(8, dtype=bool)
    refine[pattern] = True
    n = M.HangingBrickMesh(1, refine, 2).n_elements
    deg_global = np.array([deg_spec[i % len(deg_spec)] for i in range(n)], dtype=np.int32)
    return refine, deg_global, P.partition_by_dofs(deg_global, world)


class RankLists:
    """extended mesh, ElementSchedule and the flat lists of one rank -- what SchwarzShard / SchwarzShardNative build, minus the device"""

    def __init__(self, level, deg_global, parts, rank, refine=None):
        from disco4est_amd import mesh as M, parallel as P
        from disco4est_amd.schwarz import ghost_layer, ghost_layer_hanging
        if refine is not None:
            own, ghosts, needed_by = ghost_layer_hanging(level, refine, parts, rank)
            self.mesh = M.HangingBrickMesh(level, refine, deg_global, elements=np.concatenate([own, ghosts]))
        else:
            own, ghosts, needed_by = ghost_layer(level, parts, rank)
            self.mesh = M.BrickMesh(level, deg_global, elements=np.concatenate([own, ghosts]))
        self.n_own = int(own.size)
        self.schedule = P.ElementSchedule(self.mesh, self.n_own, parts, needed_by)
        self.peers, self.send_first, self.send_elem, self.recv_first, self.recv_elem = P.element_exchange_lists(self.schedule, self.mesh.nodal_stride)
        self.n3 = (self.mesh.deg.astype(np.int64) + 1) ** 3
        self.own_nodes = int(self.n3[:self.n_own].sum())

    def segment(self, which, i):
        first, elem = (self.send_first, self.send_elem) if which == "send" else (self.recv_first, self.recv_elem)
        return elem[first[i]:first[i + 1]]


def corrected_by(lists):
    """per own element: how many peers send it a correction (= in how many ghost layers it lies)"""
    return np.bincount(lists.send_elem, minlength=lists.n_own)


def accumulate_csr(lists, u_own, u_ext, recv):
    """step 6 of an iterate in numpy, as schwarz_accumulate_kernel does it: per own element the offsets of its blocks in the backward
    receive buffer (the forward send layout), in ascending peer rank; u += u_ext[own], then the blocks in that order"""
    off = np.concatenate([[0], np.cumsum(lists.n3[lists.send_elem])])[:-1]
    per_elem = [[] for _ in range(lists.n_own)]
    for k, e in enumerate(lists.send_elem):          # the flat list runs peer after peer: appending keeps the peer order
        per_elem[int(e)].append(int(off[k]))
    out = np.array(u_own, dtype=np.float64, copy=True)
    stride = lists.mesh.nodal_stride
    for e in range(lists.n_own):
        s, n = int(stride[e]), int(lists.n3[e])
        acc = out[s:s + n] + u_ext[s:s + n]
        for o in per_elem[e]:
            acc = acc + recv[o:o + n]
        out[s:s + n] = acc
    return out
