"""GPU tests of the estimator with the pointwise (strong-form) residual (d4est_hip_estimator_bi_pointwise; d4est_estimator_bi_new_compute
with use_pointwise_residual, src/Estimators/d4est_estimator_bi_new.c:386-567): term 0 against tests/dense_hessian.py's
h^2 / p^2 sum_q w J r_q^2, terms 1 - 3 and eta2 against tests/dense_estimator.py's face terms, the pipeline
r = f - hessian_trace(u) -> estimator end to end, and d4est_hip_estimator_bi's bits before and after the new call.  The meshes are the
locally refined brick and the mixed-degree brick of tests/test_estimator_gpu.py, built the same way."""
import numpy as np
import pytest

from tests import dense_estimator as DE
from tests import dense_hessian as DH

pytestmark = pytest.mark.gpu
RTOL = 1e-12          # tests/test_estimator_gpu.py's
RTOL_TERM0 = 1e-13    # a weighted sum of squares: no cancellation


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rfo():
    from disco4est_amd import capi
    lib = capi.load_library()
    return lambda a, b, c, d: int(lib.d4est_hip_reorient_face_order(a, b, c, d))


def _per_elem_rel(got, ref):
    scale = np.maximum(np.abs(ref), 1e-300)
    row = np.abs(ref).max(axis=-1, keepdims=True) if ref.ndim == 2 else np.abs(ref).max()
    return (np.abs(got - ref) / np.maximum(scale, 1e-10 * np.maximum(row, 1e-300))).max()


def _meshes():
    from disco4est_amd import mesh as M
    refine = np.zeros(8, dtype=bool)
    refine[[2, 5]] = True
    m0 = M.HangingBrickMesh(1, refine, 3)
    deg = 3 + (np.arange(m0.global_elements) * 5 % 7)
    return {"hanging": (M.HangingBrickMesh(1, refine, deg, deg_quad_inc=1), M.SineMap(0.04)),
            "mixed": (M.BrickMesh(1, np.array([3, 4, 5, 6, 7, 8, 9, 5]), deg_quad_inc=1), M.SineMap(0.04))}


_CACHE = {}


def _case(name):
    """mesh, factors, sides, field, Dirichlet data, sizes and the dense face terms of one mesh, computed once"""
    if name not in _CACHE:
        from disco4est_amd import mesh as M
        m, mp = _meshes()[name]
        J, rst = m.geometry(mp)
        sides = m.build_sides(mp)
        bx = sides["bndry_xyz"]
        g = np.cos(bx[0]) + bx[2]
        u = m.field(mp)
        diam = 0.5 + M.splitmix64_uniform(6, m.n_elements)
        dense = DE.DenseEstimator(m, J, rst, sides, _rfo(), (7, 8, 9), 10.0)
        face_terms, _ = dense.compute(u, np.zeros(m.local_nodes), diam, g=g)      # terms 1 - 3 do not depend on the residual
        _CACHE[name] = dict(m=m, mp=mp, J=J, rst=rst, sides=sides, g=g, u=u, diam=diam, face_terms=face_terms)
    return _CACHE[name]


def _plan(c):
    from disco4est_amd import Plan
    m = c["m"]
    plan = Plan(m.deg, m.deg_quad, m.nodal_stride, m.quad_stride, m.quad_type)
    plan.set_geometry(c["J"], c["rst"])
    plan.set_estimator(7, 8, 9, 10.0)
    plan.set_faces(c["sides"], 10.0, 0)
    return plan


def _pointwise(plan, c, gpu, r_quad):
    import torch
    ne = c["m"].n_elements
    eta2 = torch.full((ne,), float("nan"), dtype=torch.float64, device=gpu)
    terms = torch.full((4 * ne,), float("nan"), dtype=torch.float64, device=gpu)
    plan.estimator_bi_pointwise(_t(c["u"], gpu), r_quad, c["diam"], eta2, terms=terms, g=c["g"])
    torch.cuda.synchronize()
    return eta2.cpu().numpy(), terms.cpu().numpy().reshape(4, -1)


@pytest.mark.parametrize("name", ["hanging", "mixed"])
def test_parity_and_term0(gpu, hiplib, name):
    from disco4est_amd import mesh as M
    c = _case(name)
    m = c["m"]
    r = M.splitmix64_uniform(9, m.local_nodes_quad) - 0.5
    plan = _plan(c)
    eta2, terms = _pointwise(plan, c, gpu, _t(r, gpu))
    plan.destroy()
    ref = c["face_terms"].copy()
    ref[0] = DH.DenseHessian(m, "brick").pointwise_term0(r, c["J"], c["diam"])
    ref_eta2 = ((ref[0] + ref[1]) + ref[2]) + ref[3]
    rel0 = (np.abs(terms[0] - ref[0]) / ref[0]).max()
    print("%s: term0 rel %.3e, terms rel %.3e, eta2 rel %.3e" % (name, rel0, _per_elem_rel(terms, ref), _per_elem_rel(eta2, ref_eta2)))
    assert np.isfinite(eta2).all() and np.isfinite(terms).all() and ref[0].min() > 0
    assert rel0 <= RTOL_TERM0
    assert _per_elem_rel(terms, ref) <= RTOL
    assert _per_elem_rel(eta2, ref_eta2) <= RTOL


def test_end_to_end_poisson(gpu, hiplib):
    """r = f - Lap u_h for the manufactured solution u = sin(pi x) sin(pi y) sin(pi z) of Lap u = f on the curved mixed-degree brick,
    formed on the device by hessian_trace and fed to the estimator, against the same pipeline in numpy.  Term 0 inherits the rounding
    of Lap u_h: with B the bound of tests/test_hessian_gpu.py on |Lap u_h (device) - Lap u_h (long double)| and the float64 dense
    pipeline within B / 4 of the long-double one, r differs by at most 5 B / 4 <= 2 B per node, so term 0 by at most
    h^2 / p^2 sum_q w J (2 |r| (2 B) + (2 B)^2).
    Terms 1 - 3 do not depend on the residual and take the kernels of d4est_hip_estimator_bi: they must equal, bit for bit, what that
    entry gives for the same u (tests/test_estimator_gpu.py holds it to the dense estimator), and eta2 must be the fixed-order sum
    ((term0 + term1) + term2) + term3 of the four device terms.  (For this field the face terms are squares of jumps of a smooth
    interpolant, far below the traces they are differences of: a relative comparison with a dense evaluation would measure that
    cancellation, not the pipeline.)"""
    import torch
    c = _case("mixed")
    m, mp = c["m"], c["mp"]
    xyz = m.nodal_coords(mp)
    u = np.sin(np.pi * xyz[0]) * np.sin(np.pi * xyz[1]) * np.sin(np.pi * xyz[2])
    xq = DH.quad_coords(m, mp)
    f = -3.0 * np.pi ** 2 * np.sin(np.pi * xq[0]) * np.sin(np.pi * xq[1]) * np.sin(np.pi * xq[2])
    d64 = DH.DenseHessian(m, "numerical", xyz=xyz, rst=c["rst"])
    dld = DH.DenseHessian(m, "numerical", dtype=np.longdouble, xyz=xyz, rst=c["rst"])
    B, _, _ = DH.error_bound(d64, dld, u)
    r_ref = f - d64.trace(u, "reference")
    cc = dict(c, u=u)
    plan = _plan(c)
    plan.set_hessian_numerical(xyz, c["rst"])
    lap = torch.empty(m.local_nodes_quad, dtype=torch.float64, device=gpu)
    plan.hessian_trace(_t(u, gpu), lap)
    r_dev = _t(f, gpu) - lap
    eta2, terms = _pointwise(plan, cc, gpu, r_dev)
    weak_eta2 = torch.empty(m.n_elements, dtype=torch.float64, device=gpu)
    weak_terms = torch.full((4 * m.n_elements,), float("nan"), dtype=torch.float64, device=gpu)
    plan.estimator_bi(_t(u, gpu), torch.zeros(m.local_nodes, dtype=torch.float64, device=gpu), c["diam"], weak_eta2, terms=weak_terms, g=c["g"])
    torch.cuda.synchronize()
    weak_terms = weak_terms.cpu().numpy().reshape(4, -1)
    plan.destroy()
    ref0 = d64.pointwise_term0(r_ref, c["J"], c["diam"])
    slack = d64.pointwise_term0(np.sqrt(4.0 * np.abs(r_ref) * B + 4.0 * B * B), c["J"], c["diam"])
    err0 = np.abs(terms[0] - ref0)
    print("end to end: |r|_inf %.3e, hessian bound %.3e, term0 error / allowed max %.3e" % (np.abs(r_ref).max(), B, (err0 / (slack + RTOL_TERM0 * ref0)).max()))
    assert np.isfinite(eta2).all() and np.isfinite(terms).all() and ref0.min() > 0
    assert np.abs(r_dev.cpu().numpy() - r_ref).max() <= 2.0 * B
    assert (err0 <= slack + RTOL_TERM0 * ref0).all()
    assert np.array_equal(terms[1:], weak_terms[1:]) and np.abs(weak_terms[1:]).min() > 0
    assert np.array_equal(eta2, ((terms[0] + terms[1]) + terms[2]) + terms[3])


def test_estimator_bi_keeps_its_bits(gpu, hiplib):
    """d4est_hip_estimator_bi on the same plan before and after a pointwise call"""
    import torch
    from disco4est_amd import mesh as M
    c = _case("hanging")
    m = c["m"]
    plan = _plan(c)
    du = _t(c["u"], gpu)
    r = _t(M.splitmix64_uniform(5, m.local_nodes) - 0.5, gpu)

    def weak():
        eta2 = torch.full((m.n_elements,), float("nan"), dtype=torch.float64, device=gpu)
        terms = torch.full((4 * m.n_elements,), float("nan"), dtype=torch.float64, device=gpu)
        plan.estimator_bi(du, r, c["diam"], eta2, terms=terms, g=c["g"])
        torch.cuda.synchronize()
        return eta2.cpu().numpy(), terms.cpu().numpy()
    e0, t0 = weak()
    _pointwise(plan, c, gpu, _t(M.splitmix64_uniform(9, m.local_nodes_quad) - 0.5, gpu))
    e1, t1 = weak()
    plan.destroy()
    ref_terms, ref_eta2 = DE.DenseEstimator(m, c["J"], c["rst"], c["sides"], _rfo(), (7, 8, 9), 10.0).compute(
        c["u"], r.cpu().numpy(), c["diam"], g=c["g"])
    assert np.array_equal(e0, e1) and np.array_equal(t0, t1)
    assert _per_elem_rel(e0, ref_eta2) <= RTOL
