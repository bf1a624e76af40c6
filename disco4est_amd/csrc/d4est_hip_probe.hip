// Point probes on a plan: the value and the gradient of a nodal field at tree coordinates (include/d4est_hip.h "point probes").
//
// d4est_mesh_interpolate_at_tree_coord (src/Mesh/d4est_mesh.c:3294-3362) walks the quadrants of one tree, takes the first whose closed
// box contains abc, maps abc to the element's rst and calls d4est_operators_interpolate (src/dGMath/d4est_operators.c:2289-2340):
// three vectors of d4est_lgl_lagrange_1d (src/dGMath/d4est_lgl.c:59-68) and d4est_kron_vec1_o_vec2_o_vec3_dot_x_sum.  Here, for a
// batch of points:
//
//   probe_locate_kernel    one wavefront per point; lane l tests elements l, l + 64, ... against the element boxes (lo / hi = q / root_len,
//                          (q + dq) / root_len, formed once on the host in the reference's arithmetic, SoA: 7 streams of n_elements) and
//                          keeps the lowest matching id; a wave-wide minimum (six xor-shuffles) gives the first match in quadrant order.
//                          Lane 0 writes err, the element id, its nodal_stride and deg, and rst.
//   probe_eval_kernel      one wavefront per point.  Lanes 0 .. 3 N - 1 form the three basis vectors (lane = d N + i: the product of
//                          d4est_lgl_lagrange_1d, factor by factor in its order; with GRAD also its derivative, the sum over the left-out
//                          factor m of 1 / (x_i - x_m) times the remaining product) into LDS, once for all fields.  Then lane c, c + 64,
//                          ... owns the column (j, k) = (c % N, c / N), runs over i -- N contiguous doubles of u -- and weights the line
//                          sum(s) with l_k(t) l_j(s) (and the derivative combinations); the partials meet in a fixed xor-butterfly.
//                          GRAD with a map: every lane evaluates the tree map's Jacobian at the point (wave-uniform, d4est_hip_maps.h),
//                          scales it by dq / root_len / 2, inverts it and lane 0 stores the physical gradient.
//   probe_xyz_kernel       one thread per point: the tree map at (tree, abc).
//
// No atomics; every reduction has a fixed order, so results are bit-identical from call to call.  The basis functions are compiled
// without floating-point contraction: they are the reference's roundings, operation for operation.
// Bytes per point: locate reads 28 B and 7 streams of n_elements (4 + 48 B per element, from L2 after the first wave) and writes 40 B; eval
// reads 36 B of point data (76 B for the physical gradient), 8 N^3 B of u per field and 8 N B of nodes, and writes 8 B per field (24 B
// for the gradient).
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "d4est_hip_internal.h"
#include "d4est_hip_maps.h"
#include "d4est_hip_tables.h"

struct d4est_hip_probe {
  d4est_hip_plan* plan = nullptr;
  int n_points = 0, n_elements = 0;
  double root_len = 0.0;
  // points
  int* d_tree = nullptr;
  double* d_abc = nullptr;      // 3 n_points
  // elements (SoA)
  int* d_elem_tree = nullptr;
  double* d_lo = nullptr;       // 3 n_elements: lo[d * n_elements + e]
  double* d_hi = nullptr;
  double* d_half = nullptr;     // dq / root_len / 2
  int* d_elem_ns = nullptr;
  int* d_elem_deg = nullptr;
  // located points
  int* d_err = nullptr;
  int* d_elem = nullptr;
  int* d_ns = nullptr;
  int* d_deg = nullptr;
  double* d_rst = nullptr;      // 3 n_points
  double* d_xyz = nullptr;      // 3 n_points (probe_xyz)
  double* d_nodes = nullptr;    // kMaxN * (kMaxN + 1): Lobatto nodes of degree p at p * kMaxN
  std::vector<int> h_tree_found;   // tree of every found point (probe_set_map checks them against the map)
  // map
  int map = -1;                 // -1 none, 0 brick, else D4EST_HIP_GEOM_*
  d4est_hip::TreeMapParams P = {};
  double extents[6] = {0., 1., 0., 1., 0., 1.};
};

namespace d4est_hip {

constexpr int kProbeMaxN = 20;        // degrees 1 .. 19
constexpr int kProbeWaves = 4;        // wavefronts (points) per workgroup

__global__ __launch_bounds__(64 * kProbeWaves) void probe_locate_kernel(
    int n_points, int n_elements, const int* __restrict__ tree, const double* __restrict__ abc, const int* __restrict__ elem_tree,
    const double* __restrict__ lo, const double* __restrict__ hi, const int* __restrict__ elem_ns, const int* __restrict__ elem_deg,
    int* __restrict__ err, int* __restrict__ elem, int* __restrict__ ns, int* __restrict__ deg, double* __restrict__ rst) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * kProbeWaves + (threadIdx.x >> 6);
  if (p >= n_points) return;   // wave-uniform
  const int t = tree[p];
  const double a = abc[3 * p], b = abc[3 * p + 1], c = abc[3 * p + 2];
  int best = n_elements;
  for (int e = lane; e < n_elements; e += 64) {
    // d4est_mesh.c:3321-3327: (abc[d] <= amax) && (abc[d] >= amin) for all d; a NaN coordinate matches nothing
    const bool in = elem_tree[e] == t && a >= lo[e] && a <= hi[e] && b >= lo[n_elements + e] && b <= hi[n_elements + e] &&
                    c >= lo[2 * n_elements + e] && c <= hi[2 * n_elements + e];
    if (in) { best = e; break; }   // ascending e per lane: its first match is its lowest
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) best = min(best, __shfl_xor(best, s, 64));
  if (lane != 0) return;
  if (best >= n_elements) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    err[p] = 1; elem[p] = -1; ns[p] = 0; deg[p] = 0;
    rst[3 * p] = rst[3 * p + 1] = rst[3 * p + 2] = qnan;
    return;
  }
  err[p] = 0; elem[p] = best; ns[p] = elem_ns[best]; deg[p] = elem_deg[best];
  const double x[3] = {a, b, c};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double amin = lo[d * n_elements + best], amax = hi[d * n_elements + best];
    rst[3 * p + d] = 2 * (x[d] - amin) / (amax - amin) - 1;   // :3339
  }
}

// d4est_lgl_lagrange_1d (d4est_lgl.c:59-68): l = 1; for i != j: l *= (x - lgl[i]) / (lgl[j] - lgl[i])
__device__ inline double probe_lagrange(double x, const double* __restrict__ lgl, int j, int N) {
#pragma clang fp contract(off)
  double l = 1.;
  for (int i = 0; i < N; ++i)
    if (i != j) l *= (x - lgl[i]) / (lgl[j] - lgl[i]);
  return l;
}

// its derivative: sum over m != j of { 1 / (lgl[j] - lgl[m]) times the product above without the factor m }, m ascending
__device__ inline double probe_lagrange_deriv(double x, const double* __restrict__ lgl, int j, int N) {
#pragma clang fp contract(off)
  double d = 0.;
  for (int m = 0; m < N; ++m) {
    if (m == j) continue;
    double l = 1. / (lgl[j] - lgl[m]);
    for (int i = 0; i < N; ++i)
      if (i != j && i != m) l *= (x - lgl[i]) / (lgl[j] - lgl[i]);
    d = d + l;
  }
  return d;
}

__device__ inline double probe_wave_sum(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

struct ProbeMap {
  int map;            // -1 none (reference-space gradient), 0 brick, else the analytic type in P
  TreeMapParams P;
  double ex, ey, ez;  // brick: X1 - X0, ...
};

template <bool GRAD>
__global__ __launch_bounds__(64 * kProbeWaves) void probe_eval_kernel(
    int n_points, int n_fields, const int* __restrict__ err, const int* __restrict__ ns, const int* __restrict__ deg,
    const double* __restrict__ rst, const double* __restrict__ nodes, const double* __restrict__ u, long long field_stride,
    double* __restrict__ out, ProbeMap M, const int* __restrict__ tree, const double* __restrict__ abc, const int* __restrict__ elem,
    const double* __restrict__ half) {
  __shared__ double sh[kProbeWaves][(GRAD ? 6 : 3) * kProbeMaxN];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = blockIdx.x * kProbeWaves + w;
  const bool found = p < n_points && err[p] == 0;   // wave-uniform
  const int N = found ? deg[p] + 1 : 0;
  double* L = sh[w];                    // L[d * kProbeMaxN + i] = l_i(rst[d]);  GRAD: L[(3 + d) * kProbeMaxN + i] = l'_i(rst[d])
  if (lane < 3 * N) {
    const double* lgl = nodes + (N - 1) * kProbeMaxN;
    const int d = lane / N, i = lane - d * N;
    const double x = rst[3 * p + d];
    L[d * kProbeMaxN + i] = probe_lagrange(x, lgl, i, N);
    if (GRAD) L[(3 + d) * kProbeMaxN + i] = probe_lagrange_deriv(x, lgl, i, N);
  }
  __syncthreads();   // the only barrier: every wavefront of the workgroup reaches it, whatever its point
  if (p >= n_points) return;
  if (!found) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    if (lane == 0) {
      if (GRAD) out[p] = out[(size_t)n_points + p] = out[2 * (size_t)n_points + p] = qnan;
      else
        for (int f = 0; f < n_fields; ++f) out[(size_t)f * n_points + p] = qnan;
    }
    return;
  }
  const double* Lr = L;
  const double* Ls = L + kProbeMaxN;
  const double* Lt = L + 2 * kProbeMaxN;
  const size_t base = (size_t)ns[p];
  if (!GRAD) {
    for (int f = 0; f < n_fields; ++f) {
      const double* uf = u + (size_t)f * field_stride + base;
      double acc = 0.;
      for (int c = lane; c < N * N; c += 64) {
        const int j = c % N, k = c / N;
        const double* line = uf + (size_t)c * N;   // (k N + j) N
        double s = 0.;
        for (int i = 0; i < N; ++i) s += Lr[i] * line[i];
        acc += Lt[k] * Ls[j] * s;
      }
      acc = probe_wave_sum(acc);
      if (lane == 0) out[(size_t)f * n_points + p] = acc;
    }
    return;
  }
  const double* Dr = L + 3 * kProbeMaxN;
  const double* Ds = L + 4 * kProbeMaxN;
  const double* Dt = L + 5 * kProbeMaxN;
  double g0 = 0., g1 = 0., g2 = 0.;
  for (int c = lane; c < N * N; c += 64) {
    const int j = c % N, k = c / N;
    const double* line = u + base + (size_t)c * N;
    double s = 0., sd = 0.;
    for (int i = 0; i < N; ++i) {
      const double v = line[i];
      s += Lr[i] * v;
      sd += Dr[i] * v;
    }
    g0 += Lt[k] * Ls[j] * sd;
    g1 += Lt[k] * Ds[j] * s;
    g2 += Dt[k] * Ls[j] * s;
  }
  g0 = probe_wave_sum(g0);
  g1 = probe_wave_sum(g1);
  g2 = probe_wave_sum(g2);
  if (M.map >= 0) {
    // dx/dr at the point = dx/d(abc) dq / root_len / 2, inverted: R[i][d] = dr_i/dx_d (wave-uniform, every lane the same)
    const double h = half[elem[p]];
    double D[3][3], R[3][3];
    if (M.map == 0) {
      for (int i = 0; i < 3; ++i)
        for (int d = 0; d < 3; ++d) D[i][d] = 0.;
      D[0][0] = M.ex * h; D[1][1] = M.ey * h; D[2][2] = M.ez * h;
    } else {
      const double xi[3] = {abc[3 * p], abc[3 * p + 1], abc[3 * p + 2]};
      tree_map_dxdxi(M.P, tree[p], xi, D);
      for (int i = 0; i < 3; ++i)
        for (int d = 0; d < 3; ++d) D[i][d] *= h;
    }
    invert3(D, R);
    const double r0 = g0, r1 = g1, r2 = g2;
    g0 = r0 * R[0][0] + r1 * R[1][0] + r2 * R[2][0];
    g1 = r0 * R[0][1] + r1 * R[1][1] + r2 * R[2][1];
    g2 = r0 * R[0][2] + r1 * R[1][2] + r2 * R[2][2];
  }
  if (lane == 0) {
    out[p] = g0;
    out[(size_t)n_points + p] = g1;
    out[2 * (size_t)n_points + p] = g2;
  }
}

__global__ __launch_bounds__(256) void probe_xyz_kernel(int n_points, const int* __restrict__ err, const int* __restrict__ tree,
                                                        const double* __restrict__ abc, ProbeMap M, double x0, double y0, double z0,
                                                        double* __restrict__ xyz) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_points) return;
  double X[3];
  if (err[p] != 0) {
    X[0] = X[1] = X[2] = __longlong_as_double(0x7ff8000000000000LL);
  } else if (M.map == 0) {
    X[0] = x0 + M.ex * abc[3 * p]; X[1] = y0 + M.ey * abc[3 * p + 1]; X[2] = z0 + M.ez * abc[3 * p + 2];
  } else {
    const double xi[3] = {abc[3 * p], abc[3 * p + 1], abc[3 * p + 2]};
    tree_map_x(M.P, tree[p], xi, X);
  }
  xyz[3 * p] = X[0]; xyz[3 * p + 1] = X[1]; xyz[3 * p + 2] = X[2];
}

static ProbeMap probe_map_of(const d4est_hip_probe* pr, bool use) {
  ProbeMap M;
  M.map = use ? pr->map : -1;
  M.P = pr->P;
  M.ex = pr->extents[1] - pr->extents[0];
  M.ey = pr->extents[3] - pr->extents[2];
  M.ez = pr->extents[5] - pr->extents[4];
  return M;
}

template <class T>
static T* probe_alloc(size_t n) {
  T* d = nullptr;
  HIP_CHECK(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
  return d;
}

template <class T>
static std::vector<T> probe_to_host(const T* src, size_t n, int on_device) {
  std::vector<T> h(n);
  if (n == 0) return h;
  if (on_device) HIP_CHECK(hipMemcpy(h.data(), src, n * sizeof(T), hipMemcpyDeviceToHost));
  else std::copy(src, src + n, h.begin());
  return h;
}

}  // namespace d4est_hip

using namespace d4est_hip;

static void check_probe(const d4est_hip_probe_t* probe, const char* who) {
  if (!probe || !probe->plan) D4EST_HIP_ABORT("%s: NULL probe", who);
}

d4est_hip_probe_t* d4est_hip_probe_create(d4est_hip_plan_t* plan, int n_points, const int* tree, const double* abc, const int* elem_tree,
                                          const int* elem_q, const int* elem_dq, double root_len, int on_device) {
  const char* who = "probe_create";
  if (!plan) D4EST_HIP_ABORT("%s: NULL plan", who);
  if (n_points < 0) D4EST_HIP_ABORT("%s: n_points %d", who, n_points);
  if (n_points > 0 && (!tree || !abc)) D4EST_HIP_ABORT("%s: NULL point array", who);
  const int ne = plan->n_elements;
  if (ne > 0 && (!elem_tree || !elem_q || !elem_dq)) D4EST_HIP_ABORT("%s: NULL element array", who);
  if (!(root_len > 0.)) D4EST_HIP_ABORT("%s: root_len", who);
  d4est_hip_probe* pr = new d4est_hip_probe;
  pr->plan = plan;
  pr->n_points = n_points;
  pr->n_elements = ne;
  pr->root_len = root_len;
  // element boxes in the reference's arithmetic (d4est_mesh.c:3322-3325): amin = q, amax = q + dq (integers), both /= (double)root_len
  const std::vector<int> ht = probe_to_host(elem_tree, (size_t)ne, on_device), hq = probe_to_host(elem_q, (size_t)3 * ne, on_device),
                         hd = probe_to_host(elem_dq, (size_t)ne, on_device);
  std::vector<double> lo((size_t)3 * ne), hi((size_t)3 * ne), half((size_t)ne);
  for (int e = 0; e < ne; ++e) {
    if (hd[e] <= 0) D4EST_HIP_ABORT("%s: element %d has dq %d", who, e, hd[e]);
    if (plan->deg[e] < 1 || plan->deg[e] + 1 > kProbeMaxN) D4EST_HIP_ABORT("%s: element %d has degree %d (1 .. %d)", who, e, plan->deg[e], kProbeMaxN - 1);
    for (int d = 0; d < 3; ++d) {
      double amin = hq[3 * e + d], amax = hq[3 * e + d] + hd[e];
      amin /= root_len;
      amax /= root_len;
      lo[(size_t)d * ne + e] = amin;
      hi[(size_t)d * ne + e] = amax;
    }
    half[e] = 0.5 * (double)hd[e] / root_len;   // cell_dxdr (d4est_hip_maps.h)
  }
  std::vector<double> nodes((size_t)kProbeMaxN * kProbeMaxN, 0.);
  for (int p = 1; p < kProbeMaxN; ++p) {
    std::vector<double> x, w;
    Tables1D::lobatto(p, x, w);
    std::copy(x.begin(), x.end(), nodes.begin() + (size_t)p * kProbeMaxN);
  }
  pr->d_elem_tree = probe_alloc<int>(ne);
  pr->d_lo = probe_alloc<double>((size_t)3 * ne);
  pr->d_hi = probe_alloc<double>((size_t)3 * ne);
  pr->d_half = probe_alloc<double>(ne);
  pr->d_elem_ns = probe_alloc<int>(ne);
  pr->d_elem_deg = probe_alloc<int>(ne);
  pr->d_nodes = probe_alloc<double>(nodes.size());
  pr->d_tree = probe_alloc<int>(n_points);
  pr->d_abc = probe_alloc<double>((size_t)3 * n_points);
  pr->d_err = probe_alloc<int>(n_points);
  pr->d_elem = probe_alloc<int>(n_points);
  pr->d_ns = probe_alloc<int>(n_points);
  pr->d_deg = probe_alloc<int>(n_points);
  pr->d_rst = probe_alloc<double>((size_t)3 * n_points);
  pr->d_xyz = probe_alloc<double>((size_t)3 * n_points);
  HIP_CHECK(hipMemcpy(pr->d_nodes, nodes.data(), nodes.size() * sizeof(double), hipMemcpyHostToDevice));
  if (ne > 0) {
    HIP_CHECK(hipMemcpy(pr->d_elem_tree, ht.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pr->d_lo, lo.data(), lo.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pr->d_hi, hi.data(), hi.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pr->d_half, half.data(), half.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pr->d_elem_ns, plan->nodal_stride.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(pr->d_elem_deg, plan->deg.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice));
  }
  if (n_points > 0) {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIP_CHECK(hipMemcpy(pr->d_tree, tree, (size_t)n_points * sizeof(int), kind));
    HIP_CHECK(hipMemcpy(pr->d_abc, abc, (size_t)3 * n_points * sizeof(double), kind));
    const int blocks = (n_points + kProbeWaves - 1) / kProbeWaves;
    hipLaunchKernelGGL(probe_locate_kernel, dim3(blocks), dim3(64 * kProbeWaves), 0, plan->stream, n_points, ne, pr->d_tree, pr->d_abc,
                       pr->d_elem_tree, pr->d_lo, pr->d_hi, pr->d_elem_ns, pr->d_elem_deg, pr->d_err, pr->d_elem, pr->d_ns, pr->d_deg,
                       pr->d_rst);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(plan->stream));
    // the trees of the found points, for the check of probe_set_map
    std::vector<int> el((size_t)n_points);
    HIP_CHECK(hipMemcpy(el.data(), pr->d_elem, (size_t)n_points * sizeof(int), hipMemcpyDeviceToHost));
    pr->h_tree_found.reserve((size_t)n_points);
    for (int p = 0; p < n_points; ++p)
      if (el[p] >= 0) pr->h_tree_found.push_back(ht[el[p]]);
  }
  return pr;
}

void d4est_hip_probe_destroy(d4est_hip_probe_t* probe) {
  if (!probe) return;
  void* ptrs[] = {probe->d_tree, probe->d_abc, probe->d_elem_tree, probe->d_lo, probe->d_hi, probe->d_half, probe->d_elem_ns, probe->d_elem_deg,
                  probe->d_err, probe->d_elem, probe->d_ns, probe->d_deg, probe->d_rst, probe->d_xyz, probe->d_nodes};
  for (void* q : ptrs)
    if (q) HIP_CHECK(hipFree(q));
  delete probe;
}

int d4est_hip_probe_n_points(const d4est_hip_probe_t* probe) {
  check_probe(probe, "probe_n_points");
  return probe->n_points;
}

void d4est_hip_probe_info(const d4est_hip_probe_t* probe, int* err_host, int* elem_host, double* rst_host) {
  check_probe(probe, "probe_info");
  const size_t n = (size_t)probe->n_points;
  if (n == 0) return;
  HIP_CHECK(hipStreamSynchronize(probe->plan->stream));
  if (err_host) HIP_CHECK(hipMemcpy(err_host, probe->d_err, n * sizeof(int), hipMemcpyDeviceToHost));
  if (elem_host) HIP_CHECK(hipMemcpy(elem_host, probe->d_elem, n * sizeof(int), hipMemcpyDeviceToHost));
  if (rst_host) HIP_CHECK(hipMemcpy(rst_host, probe->d_rst, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
}

void d4est_hip_probe_element_info(const d4est_hip_probe_t* probe, int* nodal_stride_host, int* deg_host) {
  check_probe(probe, "probe_element_info");
  const size_t n = (size_t)probe->n_points;
  if (n == 0) return;
  HIP_CHECK(hipStreamSynchronize(probe->plan->stream));
  if (nodal_stride_host) HIP_CHECK(hipMemcpy(nodal_stride_host, probe->d_ns, n * sizeof(int), hipMemcpyDeviceToHost));
  if (deg_host) HIP_CHECK(hipMemcpy(deg_host, probe->d_deg, n * sizeof(int), hipMemcpyDeviceToHost));
}

void d4est_hip_probe_eval(d4est_hip_probe_t* probe, int n_fields, const double* u_dev, long long field_stride, double* out_dev) {
  check_probe(probe, "probe_eval");
  if (n_fields < 0) D4EST_HIP_ABORT("probe_eval: n_fields %d", n_fields);
  if (probe->n_points == 0 || n_fields == 0) return;
  if (!u_dev || !out_dev) D4EST_HIP_ABORT("probe_eval: NULL vector");
  if (n_fields > 1 && field_stride < 0) D4EST_HIP_ABORT("probe_eval: field_stride %lld", field_stride);
  const int blocks = (probe->n_points + kProbeWaves - 1) / kProbeWaves;
  hipLaunchKernelGGL(probe_eval_kernel<false>, dim3(blocks), dim3(64 * kProbeWaves), 0, probe->plan->stream, probe->n_points, n_fields,
                     probe->d_err, probe->d_ns, probe->d_deg, probe->d_rst, probe->d_nodes, u_dev, field_stride, out_dev,
                     probe_map_of(probe, false), probe->d_tree, probe->d_abc, probe->d_elem, probe->d_half);
  HIP_CHECK(hipGetLastError());
}

void d4est_hip_probe_set_map(d4est_hip_probe_t* probe, int geom_type, const double* params) {
  check_probe(probe, "probe_set_map");
  if (!params) D4EST_HIP_ABORT("probe_set_map: params is NULL");
  int max_tree = 0;
  if (geom_type == D4EST_HIP_GEOM_BRICK) {
    for (int d = 0; d < 3; ++d)
      if (!(params[2 * d + 1] > params[2 * d])) D4EST_HIP_ABORT("probe_set_map: brick extents must have X1 > X0 in every direction");
    std::copy(params, params + 6, probe->extents);
  } else {
    d4est_hipi_tree_map_params(geom_type, params, "probe_set_map", &probe->P);
    max_tree = tree_map_num_trees(geom_type) - 1;
  }
  for (int t : probe->h_tree_found)
    if (t < 0 || t > max_tree) D4EST_HIP_ABORT("probe_set_map: a point was found in tree %d, geometry type %d has trees 0 .. %d", t, geom_type, max_tree);
  probe->map = geom_type;
}

void d4est_hip_probe_eval_gradient(d4est_hip_probe_t* probe, const double* u_dev, double* grad_dev, int physical) {
  check_probe(probe, "probe_eval_gradient");
  if (physical && probe->map < 0) D4EST_HIP_ABORT("probe_eval_gradient: physical = 1 needs the map (d4est_hip_probe_set_map)");
  if (probe->n_points == 0) return;
  if (!u_dev || !grad_dev) D4EST_HIP_ABORT("probe_eval_gradient: NULL vector");
  const int blocks = (probe->n_points + kProbeWaves - 1) / kProbeWaves;
  hipLaunchKernelGGL(probe_eval_kernel<true>, dim3(blocks), dim3(64 * kProbeWaves), 0, probe->plan->stream, probe->n_points, 1, probe->d_err,
                     probe->d_ns, probe->d_deg, probe->d_rst, probe->d_nodes, u_dev, 0LL, grad_dev, probe_map_of(probe, physical != 0),
                     probe->d_tree, probe->d_abc, probe->d_elem, probe->d_half);
  HIP_CHECK(hipGetLastError());
}

void d4est_hip_probe_xyz(d4est_hip_probe_t* probe, double* xyz_host) {
  check_probe(probe, "probe_xyz");
  if (probe->map < 0) D4EST_HIP_ABORT("probe_xyz: needs the map (d4est_hip_probe_set_map)");
  if (probe->n_points == 0) return;
  if (!xyz_host) D4EST_HIP_ABORT("probe_xyz: NULL output");
  const int n = probe->n_points;
  hipLaunchKernelGGL(probe_xyz_kernel, dim3((n + 255) / 256), dim3(256), 0, probe->plan->stream, n, probe->d_err, probe->d_tree, probe->d_abc,
                     probe_map_of(probe, true), probe->extents[0], probe->extents[2], probe->extents[4], probe->d_xyz);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(probe->plan->stream));
  HIP_CHECK(hipMemcpy(xyz_host, probe->d_xyz, (size_t)3 * n * sizeof(double), hipMemcpyDeviceToHost));
}
