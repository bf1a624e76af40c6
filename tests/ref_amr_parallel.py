"""numpy reference of the hp-AMR step on several ranks (d4est_hip_par_amr_stats_global, d4est_hip_par_amr_repartition[_field]).

Statistics: the mpisize > 1 branch of d4est_estimator_stats_compute_aux (src/Estimators/d4est_estimator_stats.c:252-274) by concatenating
the ranks' eta2 and sorting; rank_walk is a literal restatement of d4est_estimator_stats_get_global_percentile_parallel (:379-418) over
the chunks a parallel sort leaves on the ranks, which tests/test_ref_amr_parallel.py holds against sorted[G - k].

Repartition: the transfer of d4est_amr_load_balance (src/hpAMR/d4est_amr.c:773-864) by slicing global arrays with
global_first_quadrant."""
import numpy as np


def global_id_from_end(G, percentile):
    """d4est_estimator_stats.c:379: (int)((double)(global_size*percentile)/100.0)"""
    return int(float(int(G) * int(percentile)) / 100.0)


def stats_global(eta2_per_rank, percentile):
    """(total, mean, max, estimator_at_percentile) over all ranks: the total is the sum over ranks of each rank's running sum in element
    order (:265), the mean total / G (:266), the maximum the last entry of the sorted concatenation (:269), the percentile entry G - k of
    it (:379, :391); k = 0 (the reference aborts, :396) gives -1; G = 0 gives 0, -1, -1, -1 (:234-238)"""
    parts = [np.asarray(e, dtype=np.float64).reshape(-1) for e in eta2_per_rank]
    s = np.sort(np.concatenate(parts)) if parts else np.zeros(0)
    G = s.size
    if G == 0:
        return 0.0, -1.0, -1.0, -1.0
    total = 0.0
    for e in parts:
        local = 0.0
        for v in e:
            local += float(v)
        total += local
    k = global_id_from_end(G, percentile)
    return total, total / float(G), float(s[G - 1]), (float(s[G - k]) if k > 0 else -1.0)


def even_chunks(sorted_all, world):
    """the globally sorted array as a parallel sort leaves it: contiguous ascending chunks, rank after rank (sizes differ by at most 1)"""
    G = len(sorted_all)
    cuts = [(G * r) // world for r in range(world + 1)]
    return [np.asarray(sorted_all[cuts[r]:cuts[r + 1]], dtype=np.float64) for r in range(world)]


def rank_walk(chunks, percentile):
    """d4est_estimator_stats_get_global_percentile_parallel, :379-418, all ranks in one loop: `estimator` is a rank's chunk, the two
    sc_allreduce(MAX) calls are max() over the ranks' copies.  Returns None where the reference aborts (:396, :415).  As the reference
    it recognises a found value by `> 0`: the values must be positive."""
    world = len(chunks)
    local_size = [len(c) for c in chunks]
    global_size = sum(local_size)
    gid = global_id_from_end(global_size, percentile)                 # :379
    at = [-1.0] * world                                                 # :380, one copy per rank
    stride = [0] * world                                                # :381
    temp_rank = world - 1                                               # :382
    while not (at[0] > 0):                                              # :383 (the copies agree after every allreduce)
        for rank in range(world):
            if rank == temp_rank:                                       # :385
                if gid <= local_size[rank] + stride[rank]:              # :389
                    if gid != stride[rank]:                             # :390
                        at[rank] = float(chunks[rank][local_size[rank] - (gid - stride[rank])])   # :391
                    else:
                        return None                                     # :396
                else:
                    stride[rank] += local_size[rank]                    # :400
        at = [max(at)] * world                                          # :406
        stride = [max(stride)] * world                                  # :407
        if not (at[0] > 0):                                             # :409
            temp_rank -= 1                                              # :410
            if temp_rank == -1:                                         # :411
                return None                                             # :415
    return at[0]


# ---- repartition ----------------------------------------------------------------------------------------------------------------------------
def first_of(parts):
    """global_first_quadrant of a list of (first, count) ranges"""
    return np.asarray([f for f, _ in parts] + [parts[-1][0] + parts[-1][1]], dtype=np.int64)


def by_elements(n_global, world):
    """p4est_partition_ext without weights: equal element counts (p4est_partition_given's cut (n * r) / world)"""
    return np.asarray([(int(n_global) * r) // world for r in range(world + 1)], dtype=np.int64)


def node_offsets(deg):
    return np.concatenate([[0], np.cumsum((np.asarray(deg, dtype=np.int64) + 1) ** 3)])


def element_slices(first):
    """per rank the [lo, hi) range of global elements"""
    return [(int(first[r]), int(first[r + 1])) for r in range(len(first) - 1)]


def shard_elements(values, first):
    """a per-element global array cut by global_first_quadrant"""
    values = np.asarray(values)
    return [values[lo:hi].copy() for lo, hi in element_slices(first)]


def shard_nodes(field, deg_global, first):
    """a nodal global field cut by global_first_quadrant"""
    off = node_offsets(deg_global)
    field = np.asarray(field)
    return [field[off[lo]:off[hi]].copy() for lo, hi in element_slices(first)]


def messages(old_first, new_first):
    """(sender, receiver, global lo, global hi) of every non-empty message between DIFFERENT ranks: the intersection of the sender's old
    range with the receiver's new range (Morton-contiguous partitions: one slice each)"""
    out = []
    world = len(old_first) - 1
    for s in range(world):
        for r in range(world):
            lo, hi = max(int(old_first[s]), int(new_first[r])), min(int(old_first[s + 1]), int(new_first[r + 1]))
            if s != r and hi > lo:
                out.append((s, r, lo, hi))
    return out
