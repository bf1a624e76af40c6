// Element size parameters on the device: what d4est_mesh_init_element_size_parameters_local / _ghost compute per element after every
// refinement (src/Mesh/d4est_mesh.c:1620-1827, d4est_mesh_data_compute_volume_diam :3414-3468), and the h that
// d4est_mesh_calculate_mortar_h (:689-856) builds from them for every [mesh_parameters] face_h_type.  Everything sits on the Lobatto
// nodes of the element's own degree:
//   diam_volume            max over all node pairs of |x_i - x_j| (N^6 work per element), / sqrt(3) with VOL_H_EQ_CUBE_APPROX
//   diam_face[6]           the same over the N^2 nodes of a face
//   volume, area[6]        Lobatto inner product of 1 with J / with sj on the face
//   j_div_sj_min/mean/max  of J / sj over the face's Lobatto nodes, J and sj as d4est_mortars_compute_geometric_data_on_mortar gives
//                          them with COMPUTE_NORMAL_USING_JACOBIAN (the expressions of analytic_mortar_kernel, d4est_hip_faces_geometry.hip)
// Three kernels per degree, whatever the number of elements (local elements first, then the ghost elements of that degree):
//   size_xyz_kernel     brick / analytic map: node coordinates into a plan-owned array (the coordinates-only form reads the caller's)
//   size_diam_kernel    the pair distances.  A group of G threads (G = the power of two >= N^3, 8 ... 256) owns an element, 256 / G
//                       elements share a workgroup (p = 1: 32, p = 2: 8, p = 3: 4, p = 4: 2); a thread keeps K of its element's nodes
//                       in registers (K = 1 while N^3 <= 256, else 4) and walks the element's nodes j through LDS tiles of K G nodes
//                       (24 KB at K G = 1024: p >= 18 does not fit whole), every lane of a group reading the same j: a broadcast.
//                       Only tiles at or after the chunk of the thread's own nodes are visited (the distance is symmetric).  The
//                       running maximum is of the SQUARED distance, one sqrt at the end: sqrt is monotone and correctly rounded, so
//                       this is the reference's max of square roots.  Then the six faces, sliced from the same coordinates.
//   size_geom_kernel    brick / analytic map: volume, area and J / sj, one workgroup per element.
// No atomics; every reduction is a fixed tree over the workgroup: results are bit-identical from call to call.
#include <algorithm>
#include <cmath>

#include "d4est_hip_internal.h"
#include "d4est_hip_maps.h"
#include "d4est_hip_tables.h"

namespace d4est_hip {

namespace {

constexpr int kMaxN = Tables1D::kMaxDeg + 1;   // 24 nodes per direction

struct SizeItem {
  int xoff;    // first node of the element in a coordinate array (x at xoff, y and z one component stride further each)
  int index;   // where its results go: e, or n_elements + g
};

struct SizeBucket {
  int deg = 0, N = 0, first = 0, n_local = 0, n_ghost = 0;   // items [first, first + n_local) are local elements, the ghosts follow
};

struct SizeGeom {
  int brick;
  double ex, ey, ez;   // brick: widths of the domain
  TreeMapParams P;
  double root_len;
};

struct SizeHost {
  int n_ghost = 0;                 // ghost elements the item lists cover
  std::vector<SizeBucket> buckets;
  SizeItem* d_items = nullptr;
  double* d_tab = nullptr;         // per bucket: Lobatto nodes[kMaxN] | weights[kMaxN]
  CellDesc* h_cells = nullptr;     // pinned staging of the cell descriptions
  CellDesc* d_cells = nullptr;
  hipEvent_t copied = nullptr;     // the staging buffer is free again
  double* d_xyz = nullptr;         // x | y | z of the local + ghost elements' Lobatto nodes
  long long xyz_nodes = 0;
  double* arr[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // D4EST_HIP_SIZE_*
  MortarHUnit* d_units = nullptr;
  size_t units_cap = 0;
  bool have_diam = false, have_geom = false;
  int count = 0;                   // elements the arrays hold values for
};

// d x / d r of a cell at reference point r: the brick's is diagonal and constant (src/Geometry/d4est_geometry_brick.c:140-206)
__device__ inline void size_cell_dxdr(const SizeGeom& g, const CellDesc& cell, const double r[3], double dxdr[3][3]) {
  if (g.brick) {
    const double half = 0.5 * (double)cell.dq / g.root_len;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) dxdr[i][j] = 0.0;
    dxdr[0][0] = g.ex * half; dxdr[1][1] = g.ey * half; dxdr[2][2] = g.ez * half;
  } else {
    cell_dxdr(g.P, cell, g.root_len, r, dxdr);
  }
}

// node coordinates of the items' cells; the brick's are taken from the cell's own corner (every size parameter is translation invariant)
__global__ __launch_bounds__(256) void size_xyz_kernel(SizeGeom g, const CellDesc* __restrict__ cells, const SizeItem* __restrict__ items,
                                                       int n_items, int N, const double* __restrict__ nodes, long long cstride,
                                                       double* __restrict__ xyz) {
  const int N3 = N * N * N;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)n_items * N3) return;
  const SizeItem it = items[gid / N3];
  const int n = (int)(gid % N3);
  const CellDesc cell = cells[it.index];
  const double r[3] = {nodes[n % N], nodes[(n / N) % N], nodes[n / (N * N)]};
  double x[3];
  if (g.brick) {
    const double half = 0.5 * (double)cell.dq / g.root_len;
    x[0] = g.ex * half * (r[0] + 1.0); x[1] = g.ey * half * (r[1] + 1.0); x[2] = g.ez * half * (r[2] + 1.0);
  } else {
    cell_x(g.P, cell, g.root_len, r, x);
  }
  const size_t at = (size_t)it.xoff + n;
  xyz[at] = x[0];
  xyz[cstride + at] = x[1];
  xyz[2 * cstride + at] = x[2];
}

// max over a group of G consecutive threads (G a power of two dividing 256), a fixed tree; every thread of the workgroup calls it
__device__ inline double group_max(double v, double* red, int G, int lane) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = G >> 1; s > 0; s >>= 1) {
    if (lane < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const double r = red[threadIdx.x - lane];
  __syncthreads();
  return r;
}

template <int K>
__global__ __launch_bounds__(256) void size_diam_kernel(const double* __restrict__ xyz, long long cstride, const SizeItem* __restrict__ items,
                                                        int n_items, int N, int G, double volume_scale, double* __restrict__ diam_volume,
                                                        double* __restrict__ diam_face) {
  __shared__ double sx[1024], sy[1024], sz[1024];
  __shared__ double red[256];
  const int N2 = N * N, N3 = N2 * N;
  const int tile = K * G;                  // nodes per LDS tile of a group; 256 / G groups: at most 1024 nodes per workgroup
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  const int idx = blockIdx.x * (256 / G) + grp;
  const bool live = idx < n_items;
  const SizeItem it = items[live ? idx : n_items - 1];   // (an idle group repeats the last element and stores nothing)
  const double* x = xyz + it.xoff;
  const double* y = x + cstride;
  const double* z = y + cstride;
  double* tx = sx + grp * tile;
  double* ty = sy + grp * tile;
  double* tz = sz + grp * tile;
  double m = 0.0;
  for (int c0 = 0; c0 < N3; c0 += tile) {
    double ox[K], oy[K], oz[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int n = min(c0 + k * G + lane, N3 - 1);   // (past the end: the last node again, a real pair)
      ox[k] = x[n]; oy[k] = y[n]; oz[k] = z[n];
    }
    for (int t0 = c0; t0 < N3; t0 += tile) {
      const int cnt = min(tile, N3 - t0);
      __syncthreads();
      for (int n = lane; n < cnt; n += G) { tx[n] = x[t0 + n]; ty[n] = y[t0 + n]; tz[n] = z[t0 + n]; }
      __syncthreads();
      for (int j = 0; j < cnt; ++j) {
        const double xj = tx[j], yj = ty[j], zj = tz[j];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const double dx = ox[k] - xj, dy = oy[k] - yj, dz = oz[k] - zj;
          m = fmax(m, dx * dx + dy * dy + dz * dz);
        }
      }
    }
  }
  __syncthreads();
  m = group_max(m, red, G, lane);
  if (live && lane == 0) diam_volume[it.index] = sqrt(m) * volume_scale;
  // the faces: N^2 <= min(N^3, 576) nodes, one tile
  for (int f = 0; f < 6; ++f) {
    const int dir = f >> 1, fix = (f & 1) ? N - 1 : 0;
    for (int ab = lane; ab < N2; ab += G) {
      const int a = ab % N, b = ab / N;
      const int v = dir == 0 ? fix + N * (a + N * b) : (dir == 1 ? a + N * (fix + N * b) : a + N * (b + N * fix));
      tx[ab] = x[v]; ty[ab] = y[v]; tz[ab] = z[v];
    }
    __syncthreads();
    double mf = 0.0;
    for (int i = lane; i < N2; i += G) {
      const double xi = tx[i], yi = ty[i], zi = tz[i];
      for (int j = 0; j < N2; ++j) {
        const double dx = xi - tx[j], dy = yi - ty[j], dz = zi - tz[j];
        mf = fmax(mf, dx * dx + dy * dy + dz * dz);
      }
    }
    mf = group_max(mf, red, G, lane);   // (ends on a barrier: the tile may be overwritten)
    if (live && lane == 0) diam_face[6 * (size_t)it.index + f] = sqrt(mf);
  }
}

// fixed-tree reductions over the 256 threads of a workgroup; result in every thread
__device__ inline double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ inline double det3(const double A[3][3]) {
  return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) + A[0][1] * (A[1][2] * A[2][0] - A[1][0] * A[2][2]) +
         A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

__global__ __launch_bounds__(256) void size_geom_kernel(SizeGeom g, const CellDesc* __restrict__ cells, const SizeItem* __restrict__ items,
                                                        int n_items, int N, const double* __restrict__ tab, double* __restrict__ volume,
                                                        double* __restrict__ area, double* __restrict__ jmin, double* __restrict__ jmean,
                                                        double* __restrict__ jmax) {
  __shared__ double red[256];
  const double* t = tab;
  const double* w = tab + kMaxN;
  const int N2 = N * N, N3 = N2 * N;
  for (int ii = blockIdx.x; ii < n_items; ii += gridDim.x) {
    const int index = items[ii].index;
    const CellDesc cell = cells[index];
    double acc = 0.0;
    for (int n = threadIdx.x; n < N3; n += 256) {
      const int i = n % N, j = (n / N) % N, k = n / N2;
      const double r[3] = {t[i], t[j], t[k]};
      double dxdr[3][3];
      size_cell_dxdr(g, cell, r, dxdr);
      acc += w[i] * w[j] * w[k] * det3(dxdr);
    }
    const double vol = block_sum(acc, red);
    if (threadIdx.x == 0) volume[index] = vol;
    for (int f = 0; f < 6; ++f) {
      const int dir = f >> 1;
      double a_acc = 0.0, s_acc = 0.0, lo = INFINITY, hi = -INFINITY;
      for (int k = threadIdx.x; k < N2; k += 256) {
        const int a = k % N, b = k / N;
        double r[3], dxdr[3][3], inv[3][3];
        r[dir] = (f & 1) ? 1.0 : -1.0;
        r[dir == 0 ? 1 : 0] = t[a];
        r[dir == 2 ? 1 : 2] = t[b];
        size_cell_dxdr(g, cell, r, dxdr);
        const double J = invert3(dxdr, inv);
        const double v0 = J * (dir == 0 ? inv[0][0] : dir == 1 ? inv[1][0] : inv[2][0]);
        const double v1 = J * (dir == 0 ? inv[0][1] : dir == 1 ? inv[1][1] : inv[2][1]);
        const double v2 = J * (dir == 0 ? inv[0][2] : dir == 1 ? inv[1][2] : inv[2][2]);
        const double sj = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
        const double q = J / sj;
        a_acc += w[a] * w[b] * sj;
        s_acc += q;
        lo = fmin(lo, q);
        hi = fmax(hi, q);
      }
      const double ar = block_sum(a_acc, red);
      const double sm = block_sum(s_acc, red);
      const double mn = -group_max(-lo, red, 256, threadIdx.x);
      const double mx = group_max(hi, red, 256, threadIdx.x);
      if (threadIdx.x == 0) {
        const size_t at = 6 * (size_t)index + f;
        area[at] = ar;
        jmean[at] = sm / (double)N2;
        jmin[at] = mn;
        jmax[at] = mx;
      }
    }
  }
}

// d4est_mesh_calculate_mortar_h (src/Mesh/d4est_mesh.c:727-851) of one side of one mortar face
__device__ inline double side_h(int type, int one, int f, int n, const int* e, double tree_h, const double* volume, const double* area,
                                const double* diam_face, const double* jmin, const double* jmean, const double* jmax) {
  const size_t at = 6 * (size_t)one + f;
  switch (type) {
    case D4EST_HIP_FACE_H_EQ_J_DIV_SJ_MIN_LOBATTO: return jmin[at];
    case D4EST_HIP_FACE_H_EQ_J_DIV_SJ_MEAN_LOBATTO: return jmean[at];
    case D4EST_HIP_FACE_H_EQ_J_DIV_SJ_MAX_LOBATTO: return jmax[at];
    case D4EST_HIP_FACE_H_EQ_TREE_H: return tree_h;
    case D4EST_HIP_FACE_H_EQ_VOLUME_DIV_AREA: return volume[one] / area[at];
    case D4EST_HIP_FACE_H_EQ_FACE_DIAM: return diam_face[at];
    default: {   // FACE_H_EQ_TOTAL_VOLUME_DIV_TOTAL_AREA: summed in the side's element order
      double a = 0.0, v = 0.0;
      for (int i = 0; i < n; ++i) {
        a += area[6 * (size_t)e[i] + f];
        v += volume[e[i]];
      }
      return v / a;
    }
  }
}

__global__ __launch_bounds__(64) void mortar_h_kernel(const MortarHUnit* __restrict__ units, int n_units, int type,
                                                      const double* __restrict__ volume, const double* __restrict__ area,
                                                      const double* __restrict__ diam_face, const double* __restrict__ jmin,
                                                      const double* __restrict__ jmean, const double* __restrict__ jmax,
                                                      double* __restrict__ hm, double* __restrict__ hp) {
  for (int ui = blockIdx.x; ui < n_units; ui += gridDim.x) {
    const MortarHUnit* u = units + ui;
    const double vm = side_h(type, u->one_m, u->f_m, u->n_m, u->em, u->tree_h_m, volume, area, diam_face, jmin, jmean, jmax);
    const double vp = side_h(type, u->one_p, u->f_p, u->n_p, u->ep, u->tree_h_p, volume, area, diam_face, jmin, jmean, jmax);
    const size_t at = (size_t)u->at;
    for (int k = threadIdx.x; k < u->T; k += 64) {
      hm[at + k] = vm;
      hp[at + k] = vp;
    }
  }
}

void free_host(SizeHost* sh) {
  (void)hipFree(sh->d_items);
  (void)hipFree(sh->d_tab);
  (void)hipHostFree(sh->h_cells);
  (void)hipFree(sh->d_cells);
  if (sh->copied) (void)hipEventDestroy(sh->copied);
  (void)hipFree(sh->d_xyz);
  for (double* a : sh->arr) (void)hipFree(a);
  (void)hipFree(sh->d_units);
  delete sh;
}

// the item lists, tables and arrays for the local elements and n_ghost ghost elements: built on the first call, and again only when
// a later call covers more ghost elements
SizeHost* ensure(d4est_hip_plan* plan, int n_ghost) {
  SizeHost* sh = static_cast<SizeHost*>(plan->sizes);
  if (sh && sh->n_ghost >= n_ghost) return sh;
  if (sh) {
    HIP_CHECK(hipStreamSynchronize(plan->stream));
    free_host(sh);
    plan->sizes = nullptr;
  }
  if (n_ghost > 0 && (int)plan->ghost_deg.size() < n_ghost) D4EST_HIP_ABORT("size parameters: ghost elements need plan_set_faces first (ghost_deg)");
  sh = new SizeHost;
  sh->n_ghost = n_ghost;
  const int ne = plan->n_elements;
  long long ghost_nodes = 0;
  std::vector<int> deg_of((size_t)ne + n_ghost), xoff((size_t)ne + n_ghost);
  for (int e = 0; e < ne; ++e) { deg_of[e] = plan->deg[e]; xoff[e] = plan->nodal_stride[e]; }
  for (int gi = 0; gi < n_ghost; ++gi) {
    const int d = plan->ghost_deg[gi];
    deg_of[ne + gi] = d;
    if ((long long)plan->local_nodes + ghost_nodes + (long long)(d + 1) * (d + 1) * (d + 1) > 2147483647LL) D4EST_HIP_ABORT("size parameters: more than 2^31 nodes");
    xoff[ne + gi] = (int)(plan->local_nodes + ghost_nodes);
    ghost_nodes += (long long)(d + 1) * (d + 1) * (d + 1);
  }
  sh->xyz_nodes = (long long)plan->local_nodes + ghost_nodes;
  std::vector<SizeItem> items;
  std::vector<double> tab;
  for (int d = 0; d <= Tables1D::kMaxDeg; ++d) {
    SizeBucket bk;
    bk.deg = d; bk.N = d + 1; bk.first = (int)items.size();
    for (int i = 0; i < ne + n_ghost; ++i) {
      if (deg_of[i] != d) continue;
      items.push_back(SizeItem{xoff[i], i});
      ++(i < ne ? bk.n_local : bk.n_ghost);
    }
    if (bk.n_local + bk.n_ghost == 0) continue;
    if (d < 1) D4EST_HIP_ABORT("size parameters: degree %d", d);
    std::vector<double> x, w;
    Tables1D::lobatto(d, x, w);
    x.resize(kMaxN, 0.0); w.resize(kMaxN, 0.0);
    tab.insert(tab.end(), x.begin(), x.end());
    tab.insert(tab.end(), w.begin(), w.end());
    sh->buckets.push_back(bk);
  }
  if ((int)items.size() != ne + n_ghost) D4EST_HIP_ABORT("size parameters: a degree outside 1 ... %d", Tables1D::kMaxDeg);
  const size_t nc = std::max<size_t>((size_t)ne + n_ghost, 1);
  HIP_CHECK(hipMalloc(&sh->d_items, nc * sizeof(SizeItem)));
  HIP_CHECK(hipMalloc(&sh->d_tab, std::max<size_t>(tab.size(), 1) * sizeof(double)));
  if (!items.empty()) HIP_CHECK(hipMemcpy(sh->d_items, items.data(), items.size() * sizeof(SizeItem), hipMemcpyHostToDevice));
  if (!tab.empty()) HIP_CHECK(hipMemcpy(sh->d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&sh->h_cells), nc * sizeof(CellDesc)));
  HIP_CHECK(hipMalloc(&sh->d_cells, nc * sizeof(CellDesc)));
  HIP_CHECK(hipEventCreateWithFlags(&sh->copied, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(sh->copied, plan->stream));
  for (int a = 0; a < 7; ++a) {
    const size_t len = (a == D4EST_HIP_SIZE_DIAM_VOLUME || a == D4EST_HIP_SIZE_VOLUME ? 1 : 6) * nc;
    HIP_CHECK(hipMalloc(&sh->arr[a], len * sizeof(double)));
  }
  plan->sizes = sh;
  return sh;
}

void launch_diam(d4est_hip_plan* plan, SizeHost* sh, const SizeBucket& bk, int n, const double* xyz, long long cstride) {
  const int N3 = bk.N * bk.N * bk.N;
  int G = 8;
  while (G < N3 && G < 256) G <<= 1;
  const int per_wg = 256 / G;
  const dim3 grid((unsigned)((n + per_wg - 1) / per_wg));
  const double scale = plan->volume_h_type == D4EST_HIP_VOL_H_EQ_CUBE_APPROX ? 1. / std::sqrt(3.) : 1.0;
  if (N3 <= G)
    hipLaunchKernelGGL(size_diam_kernel<1>, grid, dim3(256), 0, plan->stream, xyz, cstride, sh->d_items + bk.first, n, bk.N, G, scale,
                       sh->arr[D4EST_HIP_SIZE_DIAM_VOLUME], sh->arr[D4EST_HIP_SIZE_DIAM_FACE]);
  else
    hipLaunchKernelGGL(size_diam_kernel<4>, grid, dim3(256), 0, plan->stream, xyz, cstride, sh->d_items + bk.first, n, bk.N, G, scale,
                       sh->arr[D4EST_HIP_SIZE_DIAM_VOLUME], sh->arr[D4EST_HIP_SIZE_DIAM_FACE]);
}

}  // namespace

void sizes_compute(d4est_hip_plan* plan, const TreeMapParams* P, const double* brick_extents, const std::vector<CellDesc>& cells,
                   int n_ghost, double root_len) {
  const int ne = plan->n_elements;
  if ((int)cells.size() != ne + n_ghost) D4EST_HIP_ABORT("size parameters: %zu cell descriptions for %d elements", cells.size(), ne + n_ghost);
  SizeHost* sh = ensure(plan, n_ghost);
  if (!sh->d_xyz) HIP_CHECK(hipMalloc(&sh->d_xyz, std::max<size_t>(3 * (size_t)sh->xyz_nodes, 1) * sizeof(double)));
  SizeGeom g{};
  g.root_len = root_len;
  if (brick_extents) {
    g.brick = 1;
    g.ex = brick_extents[1] - brick_extents[0]; g.ey = brick_extents[3] - brick_extents[2]; g.ez = brick_extents[5] - brick_extents[4];
  } else {
    g.P = *P;
  }
  HIP_CHECK(hipEventSynchronize(sh->copied));   // the previous call's copy has left the staging buffer
  if (!cells.empty()) {
    std::copy(cells.begin(), cells.end(), sh->h_cells);
    HIP_CHECK(hipMemcpyAsync(sh->d_cells, sh->h_cells, cells.size() * sizeof(CellDesc), hipMemcpyHostToDevice, plan->stream));
  }
  HIP_CHECK(hipEventRecord(sh->copied, plan->stream));
  for (size_t bi = 0; bi < sh->buckets.size(); ++bi) {
    const SizeBucket& bk = sh->buckets[bi];
    const int n = bk.n_local + (n_ghost > 0 ? bk.n_ghost : 0);
    if (n == 0) continue;
    // (ghosts of a bucket follow its local elements; a call without ghosts on lists built with them covers the local part)
    const double* tab = sh->d_tab + 2 * kMaxN * bi;
    const long long threads = (long long)n * bk.N * bk.N * bk.N;
    hipLaunchKernelGGL(size_xyz_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, plan->stream, g, sh->d_cells,
                       sh->d_items + bk.first, n, bk.N, tab, sh->xyz_nodes, sh->d_xyz);
    launch_diam(plan, sh, bk, n, sh->d_xyz, sh->xyz_nodes);
    hipLaunchKernelGGL(size_geom_kernel, dim3((unsigned)std::min(n, 16384)), dim3(256), 0, plan->stream, g, sh->d_cells, sh->d_items + bk.first,
                       n, bk.N, tab, sh->arr[D4EST_HIP_SIZE_VOLUME], sh->arr[D4EST_HIP_SIZE_AREA], sh->arr[D4EST_HIP_SIZE_J_DIV_SJ_MIN],
                       sh->arr[D4EST_HIP_SIZE_J_DIV_SJ_MEAN], sh->arr[D4EST_HIP_SIZE_J_DIV_SJ_MAX]);
  }
  HIP_CHECK(hipGetLastError());
  sh->have_diam = sh->have_geom = true;
  sh->count = ne + n_ghost;
}

void sizes_compute_diameters(d4est_hip_plan* plan, const double* xyz_lobatto) {
  if (!xyz_lobatto) D4EST_HIP_ABORT("plan_compute_diameters: NULL coordinate array");
  SizeHost* sh = ensure(plan, 0);
  for (const SizeBucket& bk : sh->buckets)
    if (bk.n_local > 0) launch_diam(plan, sh, bk, bk.n_local, xyz_lobatto, (long long)plan->local_nodes);
  HIP_CHECK(hipGetLastError());
  sh->have_diam = true;
  sh->have_geom = false;   // (whatever the other arrays held belongs to an earlier geometry)
  sh->count = plan->n_elements;
}

const double* sizes_array(const d4est_hip_plan* plan, int which, long long* count) {
  const SizeHost* sh = static_cast<const SizeHost*>(plan->sizes);
  if (which < 0 || which > D4EST_HIP_SIZE_J_DIV_SJ_MAX) D4EST_HIP_ABORT("plan_size_parameter: unknown array %d", which);
  const bool diam = which == D4EST_HIP_SIZE_DIAM_VOLUME || which == D4EST_HIP_SIZE_DIAM_FACE;
  if (!sh || !(diam ? sh->have_diam : sh->have_geom)) return nullptr;
  if (count) *count = (long long)sh->count * (which == D4EST_HIP_SIZE_DIAM_VOLUME || which == D4EST_HIP_SIZE_VOLUME ? 1 : 6);
  return sh->arr[which];
}

void sizes_fill_mortar_h(d4est_hip_plan* plan, const std::vector<MortarHUnit>& units, double* hm, double* hp) {
  SizeHost* sh = static_cast<SizeHost*>(plan->sizes);
  const int type = plan->face_h_type;
  if (type == D4EST_HIP_FACE_H_EQ_J_DIV_SJ_QUAD || units.empty()) return;
  if (type != D4EST_HIP_FACE_H_EQ_TREE_H && (!sh || !sh->have_geom)) D4EST_HIP_ABORT("mortar h: the size parameters have not been computed");
  if (!sh) sh = ensure(plan, 0);
  for (const MortarHUnit& u : units)
    for (int side = 0; side < 2; ++side) {
      const int n = side ? u.n_p : u.n_m, one = side ? u.one_p : u.one_m;
      const int* e = side ? u.ep : u.em;
      bool ok = one >= 0 && (type == D4EST_HIP_FACE_H_EQ_TREE_H || one < sh->count) && n >= 1 && n <= 4;
      for (int i = 0; ok && i < n; ++i) ok = e[i] >= 0 && (type == D4EST_HIP_FACE_H_EQ_TREE_H || e[i] < sh->count);
      if (!ok) D4EST_HIP_ABORT("mortar h: a mortar refers to an element without size parameters");
    }
  if (units.size() > sh->units_cap) {
    HIP_CHECK(hipStreamSynchronize(plan->stream));
    (void)hipFree(sh->d_units);
    HIP_CHECK(hipMalloc(&sh->d_units, units.size() * sizeof(MortarHUnit)));
    sh->units_cap = units.size();
  }
  HIP_CHECK(hipMemcpyAsync(sh->d_units, units.data(), units.size() * sizeof(MortarHUnit), hipMemcpyHostToDevice, plan->stream));
  hipLaunchKernelGGL(mortar_h_kernel, dim3((unsigned)std::min<size_t>(units.size(), 8192)), dim3(64), 0, plan->stream, sh->d_units,
                     (int)units.size(), type, sh->arr[D4EST_HIP_SIZE_VOLUME], sh->arr[D4EST_HIP_SIZE_AREA], sh->arr[D4EST_HIP_SIZE_DIAM_FACE],
                     sh->arr[D4EST_HIP_SIZE_J_DIV_SJ_MIN], sh->arr[D4EST_HIP_SIZE_J_DIV_SJ_MEAN], sh->arr[D4EST_HIP_SIZE_J_DIV_SJ_MAX], hm, hp);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(plan->stream));   // (the unit list is the caller's pageable vector)
}

void sizes_destroy(d4est_hip_plan* plan) {
  if (!plan->sizes) return;
  free_host(static_cast<SizeHost*>(plan->sizes));
  plan->sizes = nullptr;
}

}  // namespace d4est_hip
