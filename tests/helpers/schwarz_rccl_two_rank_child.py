"""One rank of tests/test_schwarz_rccl_gpu.py::test_two_ranks (started by torch.distributed.run, one process per GPU): the Schwarz iterate
and smoother on a two-way split with both whole-element exchanges through d4est_hip_schwarz_set_rccl_exchange and the trace exchange
through d4est_hip_plan_set_rccl_exchange, against the one-rank smoother on the whole mesh (1e-10 of the correction, as
tests/test_schwarz_sharded_gpu.py).  The unique id travels over a gloo group (host)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    from disco4est_amd import Plan, mesh as M, parallel as P
    from disco4est_amd.schwarz import Schwarz, SchwarzShardNative
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)))
    dev = torch.device("cuda", torch.cuda.current_device())
    dist.init_process_group(backend="gloo")
    comm = P.RcclComm(rank, world)
    level, rs, sub = 2, 2, (10, 1e-15, 1e-15)
    deg_global = np.array([[2, 3][i % 2] for i in range(64)], dtype=np.int32)
    parts = P.partition_by_dofs(deg_global, world)
    mp = M.SineMap(0.04)
    stream = torch.cuda.current_stream()
    shard = SchwarzShardNative(level, deg_global, parts, rank, mp, rs, *sub, stream=stream)
    xs = P.attach_schwarz_rccl(shard, comm)
    m = M.BrickMesh(level, deg_global, first=parts[rank][0], count=parts[rank][1])
    J, rst = m.geometry(mp); sides = m.build_sides(mp)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, 0, stream=stream)
    plan.set_geometry(J, rst); plan.set_faces(sides, 10.0, 0)
    xp = P.attach_rccl(plan, m, sides, parts, comm)
    full = M.BrickMesh(level, deg_global)
    u0 = M.splitmix64_uniform(91, full.local_nodes) - 0.5
    rhs = M.splitmix64_uniform(92, full.local_nodes) - 0.5
    s0 = m.global_nodal_offset
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[s0:s0 + m.local_nodes])).to(dev)
    ui = t(u0)
    shard.iterate(ui, t(rhs))
    us, r = t(u0), torch.empty(m.local_nodes, dtype=torch.float64, device=dev)
    shard.schwarz.smooth(plan, us, t(rhs), r, 2)
    torch.cuda.synchronize()
    gathered = [None] * world if rank == 0 else None
    dist.gather_object((ui.cpu().numpy(), us.cpu().numpy(), r.cpu().numpy(), xs.count()), gathered, dst=0)
    ok = [True]
    if rank == 0:
        Jf, rstf = full.geometry(mp); sf = full.build_sides(mp)
        pf = Plan(full.deg, full.deg_quad, full.nodal_stride, full.quad_stride, 0, stream=stream)
        pf.set_geometry(Jf, rstf); pf.set_faces(sf, 10.0, 0)
        single = Schwarz(full, sf, Jf, rstf, rs, *sub, stream=stream)
        f = lambda a: torch.from_numpy(a.copy()).to(dev)
        ui_ref = f(u0); single.iterate(ui_ref, f(rhs))
        us_ref, r_ref = f(u0), torch.empty(full.local_nodes, dtype=torch.float64, device=dev)
        single.smooth(pf, us_ref, f(rhs), r_ref, 2)
        torch.cuda.synchronize()
        cat = lambda k: np.concatenate([g[k] for g in gathered])
        e_it = np.abs(cat(0) - ui_ref.cpu().numpy()).max() / np.abs(ui_ref.cpu().numpy() - u0).max()
        e_u = np.abs(cat(1) - us_ref.cpu().numpy()).max() / np.abs(us_ref.cpu().numpy() - u0).max()
        e_r = np.abs(cat(2) - r_ref.cpu().numpy()).max() / np.abs(r_ref.cpu().numpy()).max()
        rounds = [g[3] for g in gathered]
        print("Schwarz over RCCL: iterate %.2e, smoother u %.2e r %.2e, rounds %s" % (e_it, e_u, e_r, rounds), flush=True)
        ok = [bool(e_it <= 1e-10 and e_u <= 1e-10 and e_r <= 1e-10 and all(n == 2 * 3 for n in rounds))]   # two rounds per iterate
        single.destroy(); pf.destroy()
    xp.destroy(); plan.destroy(); shard.destroy()
    comm.destroy()
    dist.broadcast_object_list(ok, src=0)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        print("two-rank Schwarz RCCL check:", "ok" if ok[0] else "MISMATCH", flush=True)
    sys.exit(0 if ok[0] else 1)


if __name__ == "__main__":
    main()
