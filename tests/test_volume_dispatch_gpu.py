"""Which stiffness kernel apply_stiffness_matrix launches: one row per distinct outcome of stiffness_choice (d4est_hip_volume.hip) and one
per multi-bucket launch, each with the exact last_kernel() string.  The strings were recorded from the build BEFORE the dispatch was
split into stiffness_choice and one launcher per kernel (tools/launch_sequence.py --volume, profiles/refactor_volume_dispatch_launch_sequence.txt),
so a change of the choice or of a name shows here.  Numbers are checked elsewhere (test_volume_gpu.py, test_volume_cg_gpu.py, ...).

Level-1 bricks (8 elements); level 5 at p = 1 for the one row beyond the 8192-element threshold of the automatic choice."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PREFETCH, WAVE, BIGP, EO, AFFINE, STREAM, ENTRY = 0, 1, 4, 6, 7, 12, 16   # tuning keys
MFMA = " (512 threads, v_mfma_f64_16x16x4)"

# degree(s), deg_quad - deg, curved, level, tuning, last_kernel
ROWS = [
    # one wavefront per element group (deg_quad <= 7)
    (3, 0, True, 1, {ENTRY: 0}, "d4est_hip::stiffness_wave_eo_kernel<4,4,cg>"),
    (3, 0, True, 1, {ENTRY: 1}, "d4est_hip::stiffness_wave_eo_kernel<4,4,cg,entry2>"),
    (7, 0, True, 1, {}, "d4est_hip::stiffness_wave_eo_kernel<8,8,cg,entry2>"),
    (3, 0, False, 1, {}, "d4est_hip::stiffness_wave_eo_kernel<4,4,affine,cg>"),
    (3, 0, False, 1, {PREFETCH: 0, WAVE: 12}, "d4est_hip::stiffness_wave_eo_kernel<4,4,affine>"),
    (3, 0, True, 1, {PREFETCH: 0, WAVE: 12}, "d4est_hip::stiffness_wave_eo_kernel<4,4>"),
    (3, 1, True, 1, {}, "d4est_hip::stiffness_wave_eo_kernel<4,5>"),
    (3, 1, False, 1, {}, "d4est_hip::stiffness_wave_eo_kernel<4,5,affine>"),
    (5, 0, True, 1, {PREFETCH: 0, WAVE: 3}, "d4est_hip::stiffness_wave2_kernel<6,6>"),
    (5, 0, True, 1, {PREFETCH: 0, WAVE: 2}, "d4est_hip::stiffness_pair_kernel<6,6>"),
    (6, 0, True, 1, {PREFETCH: 0, WAVE: 2}, "d4est_hip::stiffness_wave_kernel<7,7,false>"),   # odd size: no pair kernel
    (6, 0, True, 1, {PREFETCH: 0, WAVE: 1}, "d4est_hip::stiffness_wave_kernel<7,7,false>"),
    (6, 0, True, 1, {PREFETCH: 1, WAVE: 1}, "d4est_hip::stiffness_wave_kernel<7,7,true>"),
    # three LDS fields
    (3, 0, True, 1, {PREFETCH: 0, WAVE: 0}, "d4est_hip::stiffness_kernel<4,4,false,eo>"),
    (3, 0, True, 1, {PREFETCH: 1, WAVE: 0}, "d4est_hip::stiffness_kernel<4,4,true,eo>"),
    (1, 0, True, 5, {}, "d4est_hip::stiffness_kernel<2,2,true,eo>"),   # 32768 elements: the automatic prefetch branch
    (11, 0, True, 1, {BIGP: 0}, "d4est_hip::stiffness_kernel<12,12,false,eo>"),
    (11, 0, True, 1, {BIGP: 0, EO: 0}, "d4est_hip::stiffness_kernel<12,12,false,plain>"),
    (8, 0, True, 1, {BIGP: 0, STREAM: 1}, "d4est_hip::stiffness_kernel<9,9,false,eo>"),
    # multi-wave workgroups, two LDS fields
    (7, 1, True, 1, {}, "d4est_hip::stiffness_wave_kernel<8,9,false,eo> (128 threads)"),
    (7, 2, False, 1, {}, "d4est_hip::stiffness_wave_kernel<8,10,false,eo,affine> (128 threads)"),
    (11, 0, True, 1, {}, "d4est_hip::stiffness_wave_kernel<12,12,false,eo> (192 threads)"),
    (11, 0, True, 1, {STREAM: 1}, "d4est_hip::stiffness_wave_kernel<12,12,false,eo> (192 threads)"),
    (11, 0, False, 1, {}, "d4est_hip::stiffness_wave_kernel<12,12,false,eo,affine> (192 threads)"),
    (11, 0, True, 1, {EO: 0}, "d4est_hip::stiffness_wave_kernel<12,12,false,plain> (192 threads)"),
    (15, 0, True, 1, {BIGP: 1}, "d4est_hip::stiffness_wave_kernel<16,16,false,eo> (256 threads)"),
    (16, 0, True, 1, {}, "d4est_hip::stiffness_wave_kernel<17,17,false,eo> (320 threads)"),
    (19, 0, False, 1, {}, "d4est_hip::stiffness_wave_kernel<20,20,false,eo,affine> (448 threads)"),
    (19, 0, True, 1, {EO: 0}, "d4est_hip::stiffness_wave_kernel<20,20,false,plain> (448 threads)"),
    # FP64 matrix cores
    (13, 0, True, 1, {BIGP: 2}, "d4est_hip::stiffness_mfma16_kernel<14>" + MFMA),
    (15, 0, True, 1, {}, "d4est_hip::stiffness_mfma16_kernel<16>" + MFMA),
    (15, 0, False, 1, {}, "d4est_hip::stiffness_mfma16_kernel<16,affine>" + MFMA),
    # no compiled pair
    (5, 1, True, 1, {}, "d4est_hip::generic_volume_kernel (N=6,NQ=7)"),
    (16, 0, True, 1, {BIGP: 0}, "d4est_hip::generic_volume_kernel (N=17,NQ=17)"),
    (20, 0, True, 0, {}, "d4est_hip::generic_volume_kernel (N=21,NQ=21)"),
    # several buckets in one launch
    ((3, 4), 0, True, 1, {}, "d4est_hip::stiffness_wave_eo_multi_kernel<general,cg> (2 buckets)"),
    ((3, 4), 0, False, 1, {}, "d4est_hip::stiffness_wave_eo_multi_kernel<affine,cg> (2 buckets)"),
    ((8, 10), 0, True, 1, {}, "d4est_hip::stiffness_mw_multi_kernel<128> (2 buckets)"),
    ((11, 12), 0, True, 1, {}, "d4est_hip::stiffness_mw_multi_kernel<192> (2 buckets)"),
    ((3, 9), 0, True, 1, {}, "d4est_hip::stiffness_all_multi_kernel<cg> (1 + 1 buckets)"),
    ((9, 11), 0, True, 1, {}, "d4est_hip::stiffness_wave_kernel<12,12,false,eo> (192 threads)"),   # 128 and 192 threads: one launch each
]


def _row_id(row):
    deg, inc, curved, level, tune, _ = row
    p = "p%d" % deg if np.isscalar(deg) else "p%d+p%d" % deg
    keys = "-".join("k%d=%d" % kv for kv in sorted(tune.items())) or "auto"
    return "%s+%d-%s-l%d-%s" % (p, inc, "curved" if curved else "straight", level, keys)


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_last_kernel(gpu, hiplib, row):
    import torch
    from disco4est_amd import Plan, mesh as M
    deg, inc, curved, level, tune, want = row
    if not np.isscalar(deg):
        deg = np.where(np.arange(8 ** level) % 2 == 0, deg[0], deg[1]).astype(np.int32)
    m = M.BrickMesh(level, deg, inc)
    J, rst = m.geometry(M.SineMap(0.05) if curved else None)
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    plan.set_geometry(J, rst)
    for key, value in tune.items():
        plan.set_tuning(key, value)
    u = torch.from_numpy(m.field()).to(gpu)
    out = torch.full_like(u, float("nan"))
    plan.apply_stiffness_matrix(u, out)
    torch.cuda.synchronize()
    got = plan.last_kernel()
    plan.destroy()
    assert got == want
    assert torch.isfinite(out).all()
