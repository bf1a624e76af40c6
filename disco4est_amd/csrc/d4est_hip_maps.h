// Analytic tree maps evaluated ON THE DEVICE: x(tree, xi) for tree coordinates xi in [0,1]^3 and its
// Jacobian d x_i / d xi_j, for the geometries whose factors the engine can generate itself instead of receiving 96 B per
// quadrature node (volume) and 24 doubles per mortar node from the host.
//
//   D4EST_HIP_GEOM_CUBED_SPHERE_7TREE   [geometry] name = cubed_sphere_7tree: six wedges (trees 0..5) around a centre cube (tree 6),
//       d4est_geometry_cubed_sphere_7tree_X (src/Geometry/d4est_geometry_cubed_sphere.c:498-580), parameters R0, R1,
//       compactify_inner_shell; Clength = R0 / sqrt(3).  The reference evaluates DX from machine-generated closed forms
//       (:846-915, :1751-1830, GEOM_COMPUTE_ANALYTIC); here the Jacobian is the chain rule through the same map:
//       (a, b, c) = (2 xi0 - 1, 2 xi1 - 1, xi2 + 1), p = 2 - c, x = p a + (1-p) tan(pi a/4), y likewise,
//       S = 1 + (1-p)(tan^2 + tan^2) + 2 p, q = R(c) / sqrt(S), (X, Y, Z) = signed picks of (q x, q y, q) per wedge.
//
//   D4EST_HIP_GEOM_CUBED_SPHERE                    [geometry] name = cubed_sphere: 13 trees (p8est_connectivity_new_sphere) -- outer
//       wedges 0..5 on (R1, R2), inner wedges 6..11 on (R0, R1), the centre cube 12; d4est_geometry_cubed_sphere_X (:316-403).
//       Outer wedge: x = tan(pi a/4), y = tan(pi b/4), q = R(c) / sqrt(x^2 + y^2 + 1) with R linear between R1 and R2 or, with
//       compactify_outer_shell, R = m / (c - t), m = 1 / (1/R2 - 1/R1), t = (R1 - 2 R2) / (R1 - R2).  Inner wedge: the blended
//       form of the 7-tree map, R linear (compactify_inner_shell is REJECTED: the reference's X ignores it while its DX honours
//       it, so its factors would not be the Jacobian of its map).
//   D4EST_HIP_GEOM_CUBED_SPHERE_WITH_SPHERE_HOLE   12 trees (d4est_connectivity_new_sphere_with_hole): both shells in the
//       outer-wedge form, each with its own compactification flag (:407-497).
//   D4EST_HIP_GEOM_CUBED_SPHERE_WITH_CUBE_HOLE     the 13-tree map on the same 12 trees (:2243-2260): tree 12 never occurs.
//   params of the three: {R0, R1, R2, compactify_outer_shell, compactify_inner_shell}.
//
// One evaluation gives x and dx/dxi (wedge_blended / wedge_plain -> wedge_to_xyz); a caller that uses one of them leaves the
// other to dead-code elimination.  The same inline functions run on the host (d4est_hip_tree_map).
//
// Second derivatives d^2 x_i / d xi_j d xi_k (tree_map_d2, for the Hessian trace of d4est_hip_hessian.hip) are the chain rule through
// the same functions -- shell_radius_d2, wedge_blended_d2, wedge_plain_d2, the picks of wedge_to_xyz, zero on the centre cube -- so
// they are the derivatives of the map the factors come from, not a transcription of the reference's machine-generated closed forms
// (d4est_geometry_cubed_sphere.c:585-790, whose `c` is built from s instead of t at :629).
#pragma once
#include <hip/hip_runtime.h>

namespace d4est_hip {

struct TreeMapParams {
  int type;              // D4EST_HIP_GEOM_*
  int compactify;        // compactify_inner_shell
  int compactify_outer;  // compactify_outer_shell
  double R0, R1, R2, Clength;
};

// number of trees of the forest a geometry type lives on (0: unknown type)
__host__ __device__ inline int tree_map_num_trees(int type) {
  return type == 1 ? 7 : type == 2 ? 13 : (type == 3 || type == 4) ? 12 : 0;
}

// R(c) of a shell between Ra (c = 1) and Rb (c = 2) and dR/dc
__host__ __device__ inline void shell_radius(double Ra, double Rb, int compactify, double c, double& R, double& dR) {
  if (compactify) {
    const double m = 1.0 / (1.0 / Rb - 1.0 / Ra), t = (Ra - 2.0 * Rb) / (Ra - Rb);
    R = m / (c - t);
    dR = -m / ((c - t) * (c - t));
  } else {
    R = Ra * (2.0 - c) + Rb * (c - 1.0);
    dR = Rb - Ra;
  }
}

// The blended wedge (flat at c = 1 where it meets the cube, spherical at c = 2): v = (q x, q y, q) and g = d v / d xi.
__host__ __device__ inline void wedge_blended(double Ra, double Rb, int compactify, const double xi[3], double v[3], double g[3][3]) {
  const double kPi4 = 0.78539816339744830962;
  const double a = 2.0 * xi[0] - 1.0, b = 2.0 * xi[1] - 1.0, c = xi[2] + 1.0;
  double R, dR;
  shell_radius(Ra, Rb, compactify, c, R, dR);
  const double p = 2.0 - c;
  const double tx = tan(a * kPi4), ty = tan(b * kPi4);
  const double dtx = kPi4 * (1.0 + tx * tx), dty = kPi4 * (1.0 + ty * ty);
  const double x = p * a + (1.0 - p) * tx, y = p * b + (1.0 - p) * ty;
  const double S = 1.0 + (1.0 - p) * (tx * tx + ty * ty) + 2.0 * p;
  const double rs = 1.0 / sqrt(S), q = R * rs;
  // derivatives with respect to (a, b, c); dp/dc = -1
  const double dx[3] = {p + (1.0 - p) * dtx, 0.0, tx - a};
  const double dy[3] = {0.0, p + (1.0 - p) * dty, ty - b};
  const double dS[3] = {(1.0 - p) * 2.0 * tx * dtx, (1.0 - p) * 2.0 * ty * dty, (tx * tx + ty * ty) - 2.0};
  const double h = -0.5 * R * rs * rs * rs;
  const double dq[3] = {h * dS[0], h * dS[1], dR * rs + h * dS[2]};
  const double sc[3] = {2.0, 2.0, 1.0};   // d(a, b, c) / d xi
  for (int k = 0; k < 3; ++k) {           // rows: q x, q y, q
    g[0][k] = (dq[k] * x + q * dx[k]) * sc[k];
    g[1][k] = (dq[k] * y + q * dy[k]) * sc[k];
    g[2][k] = dq[k] * sc[k];
  }
  v[0] = q * x; v[1] = q * y; v[2] = q;
}

// The plain (equiangular) wedge of a shell: x = tan(pi a/4), y = tan(pi b/4), q = R(c) / sqrt(x^2 + y^2 + 1).
__host__ __device__ inline void wedge_plain(double Ra, double Rb, int compactify, const double xi[3], double v[3], double g[3][3]) {
  const double kPi4 = 0.78539816339744830962;
  const double a = 2.0 * xi[0] - 1.0, b = 2.0 * xi[1] - 1.0, c = xi[2] + 1.0;
  double R, dR;
  shell_radius(Ra, Rb, compactify, c, R, dR);
  const double x = tan(a * kPi4), y = tan(b * kPi4);
  const double dx = kPi4 * (1.0 + x * x), dy = kPi4 * (1.0 + y * y);
  const double S = x * x + y * y + 1.0;
  const double rs = 1.0 / sqrt(S), q = R * rs;
  const double h = -R * rs * rs * rs;                       // dq/dx = h x, dq/dy = h y
  const double dq[3] = {h * x * dx, h * y * dy, dR * rs};   // with respect to (a, b, c)
  g[0][0] = (dq[0] * x + q * dx) * 2.0; g[0][1] = dq[1] * x * 2.0;            g[0][2] = dq[2] * x;
  g[1][0] = dq[0] * y * 2.0;            g[1][1] = (dq[1] * y + q * dy) * 2.0; g[1][2] = dq[2] * y;
  g[2][0] = dq[0] * 2.0;                g[2][1] = dq[1] * 2.0;                g[2][2] = dq[2];
  v[0] = q * x; v[1] = q * y; v[2] = q;
}

// wedge -> (X, Y, Z): the six signed picks of (q x, q y, q), d4est_geometry_cubed_sphere.c:369-402 = :543-577
__host__ __device__ inline void wedge_to_xyz(int wedge, const double v[3], const double g[3][3], double X[3], double D[3][3]) {
  // row i of (X, D) is sg[i] times row pk[i] of (v, g); the picks are decoded into integers and the rows selected value by value
  // (a table or array indexed by the wedge would be a run-time index into private memory: scratch)
  const int pk0 = (wedge == 3 || wedge == 5) ? 2 : (wedge == 4 ? 1 : 0);
  const int pk1 = (wedge == 0 || wedge == 2) ? 2 : (wedge == 1 ? 1 : 0);
  const int pk2 = (wedge == 1 || wedge == 4) ? 2 : 1;
  const double sg0 = (wedge >= 4) ? -1.0 : 1.0;
  const double sg1 = (wedge == 1 || wedge == 2) ? 1.0 : -1.0;
  const double sg2 = (wedge >= 2 && wedge <= 4) ? -1.0 : 1.0;
  X[0] = sg0 * (pk0 == 0 ? v[0] : pk0 == 1 ? v[1] : v[2]);
  X[1] = sg1 * (pk1 == 0 ? v[0] : pk1 == 1 ? v[1] : v[2]);
  X[2] = sg2 * (pk2 == 1 ? v[1] : v[2]);
  for (int k = 0; k < 3; ++k) {
    const double g0 = g[0][k], g1 = g[1][k], g2 = g[2][k];
    D[0][k] = sg0 * (pk0 == 0 ? g0 : pk0 == 1 ? g1 : g2);
    D[1][k] = sg1 * (pk1 == 0 ? g0 : pk1 == 1 ? g1 : g2);
    D[2][k] = sg2 * (pk2 == 1 ? g1 : g2);
  }
}

__host__ __device__ inline void centre_cube(const TreeMapParams& P, const double xi[3], double X[3], double D[3][3]) {
  for (int i = 0; i < 3; ++i) {
    X[i] = (2.0 * xi[i] - 1.0) * P.Clength;
    for (int j = 0; j < 3; ++j) D[i][j] = (i == j) ? 2.0 * P.Clength : 0.0;
  }
}

// x(tree, xi) and d x_i / d xi_j of the map P.type; the caller has checked type, tree and flags (analytic_params_status)
__host__ __device__ inline void tree_map_eval(const TreeMapParams& P, int tree, const double xi[3], double X[3], double D[3][3]) {
  double v[3], g[3][3];
  if (P.type == 1) {                                   // cubed_sphere_7tree
    if (tree == 6) { centre_cube(P, xi, X, D); return; }
    wedge_blended(P.R0, P.R1, P.compactify, xi, v, g);
  } else if (tree < 6) {                               // outer shell of the 13-tree and holed spheres
    wedge_plain(P.R1, P.R2, P.compactify_outer, xi, v, g);
  } else if (tree == 12) {
    centre_cube(P, xi, X, D);
    return;
  } else if (P.type == 3) {                            // inner shell around a sphere hole
    wedge_plain(P.R0, P.R1, P.compactify, xi, v, g);
  } else {                                             // inner shell around the cube (or the cube hole)
    wedge_blended(P.R0, P.R1, 0, xi, v, g);
  }
  wedge_to_xyz(tree % 6, v, g, X, D);
}

__host__ __device__ inline void tree_map_dxdxi(const TreeMapParams& P, int tree, const double xi[3], double D[3][3]) {
  double X[3];
  tree_map_eval(P, tree, xi, X, D);
}

__host__ __device__ inline void tree_map_x(const TreeMapParams& P, int tree, const double xi[3], double X[3]) {
  double D[3][3];
  tree_map_eval(P, tree, xi, X, D);
}

// ---- second derivatives ----------------------------------------------------------------------------------------------------------
// d^2 R / dc^2 of shell_radius
__host__ __device__ inline double shell_radius_d2(double Ra, double Rb, int compactify, double c) {
  if (!compactify) return 0.0;
  const double m = 1.0 / (1.0 / Rb - 1.0 / Ra), t = (Ra - 2.0 * Rb) / (Ra - Rb);
  return 2.0 * m / ((c - t) * (c - t) * (c - t));
}

// Both wedges are v = (q x, q y, q) with q = R(c) / sqrt(S): from R, S, x, y and their first and second derivatives with respect to
// (a, b, c) -- the upper triangles of the second derivatives, [j][k] with j <= k -- the second derivatives of v with respect to xi,
// H[i][j][k] = d^2 v_i / d xi_j d xi_k.  The lower triangle is a copy of the upper: exactly symmetric.
__host__ __device__ inline void wedge_second(double R, double dR, double d2R, double S, const double dS[3], const double d2S[3][3],
                                             double x, const double dx[3], const double d2x[3][3], double y, const double dy[3],
                                             const double d2y[3][3], double H[3][3][3]) {
  const double rs = 1.0 / sqrt(S), rs3 = rs * rs * rs, rs5 = rs3 * rs * rs, q = R * rs;
  const double sc[3] = {2.0, 2.0, 1.0};   // d(a, b, c) / d xi
  double drs[3], dq[3];
  for (int k = 0; k < 3; ++k) {
    drs[k] = -0.5 * rs3 * dS[k];
    dq[k] = R * drs[k] + (k == 2 ? dR * rs : 0.0);
  }
  for (int j = 0; j < 3; ++j)
    for (int k = j; k < 3; ++k) {
      const double d2rs = 0.75 * rs5 * dS[j] * dS[k] - 0.5 * rs3 * d2S[j][k];
      double d2q = R * d2rs;
      if (j == 2) d2q += dR * drs[k];
      if (k == 2) d2q += dR * drs[j];
      if (j == 2 && k == 2) d2q += d2R * rs;
      const double s = sc[j] * sc[k];
      H[0][j][k] = H[0][k][j] = (d2q * x + dq[j] * dx[k] + dq[k] * dx[j] + q * d2x[j][k]) * s;
      H[1][j][k] = H[1][k][j] = (d2q * y + dq[j] * dy[k] + dq[k] * dy[j] + q * d2y[j][k]) * s;
      H[2][j][k] = H[2][k][j] = d2q * s;
    }
}

// second derivatives of wedge_blended's v with respect to xi
__host__ __device__ inline void wedge_blended_d2(double Ra, double Rb, int compactify, const double xi[3], double H[3][3][3]) {
  const double kPi4 = 0.78539816339744830962;
  const double a = 2.0 * xi[0] - 1.0, b = 2.0 * xi[1] - 1.0, c = xi[2] + 1.0;
  double R, dR;
  shell_radius(Ra, Rb, compactify, c, R, dR);
  const double d2R = shell_radius_d2(Ra, Rb, compactify, c);
  const double p = 2.0 - c;
  const double tx = tan(a * kPi4), ty = tan(b * kPi4);
  const double dtx = kPi4 * (1.0 + tx * tx), dty = kPi4 * (1.0 + ty * ty);
  const double d2tx = 2.0 * kPi4 * tx * dtx, d2ty = 2.0 * kPi4 * ty * dty;
  const double x = p * a + (1.0 - p) * tx, y = p * b + (1.0 - p) * ty;
  const double S = 1.0 + (1.0 - p) * (tx * tx + ty * ty) + 2.0 * p;
  // with respect to (a, b, c); dp/dc = -1
  const double dx[3] = {p + (1.0 - p) * dtx, 0.0, tx - a};
  const double dy[3] = {0.0, p + (1.0 - p) * dty, ty - b};
  const double dS[3] = {(1.0 - p) * 2.0 * tx * dtx, (1.0 - p) * 2.0 * ty * dty, (tx * tx + ty * ty) - 2.0};
  const double d2x[3][3] = {{(1.0 - p) * d2tx, 0.0, dtx - 1.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  const double d2y[3][3] = {{0.0, 0.0, 0.0}, {0.0, (1.0 - p) * d2ty, dty - 1.0}, {0.0, 0.0, 0.0}};
  const double d2S[3][3] = {{(1.0 - p) * 2.0 * (dtx * dtx + tx * d2tx), 0.0, 2.0 * tx * dtx},
                            {0.0, (1.0 - p) * 2.0 * (dty * dty + ty * d2ty), 2.0 * ty * dty},
                            {0.0, 0.0, 0.0}};
  wedge_second(R, dR, d2R, S, dS, d2S, x, dx, d2x, y, dy, d2y, H);
}

// second derivatives of wedge_plain's v with respect to xi
__host__ __device__ inline void wedge_plain_d2(double Ra, double Rb, int compactify, const double xi[3], double H[3][3][3]) {
  const double kPi4 = 0.78539816339744830962;
  const double a = 2.0 * xi[0] - 1.0, b = 2.0 * xi[1] - 1.0, c = xi[2] + 1.0;
  double R, dR;
  shell_radius(Ra, Rb, compactify, c, R, dR);
  const double d2R = shell_radius_d2(Ra, Rb, compactify, c);
  const double x = tan(a * kPi4), y = tan(b * kPi4);
  const double x1 = kPi4 * (1.0 + x * x), y1 = kPi4 * (1.0 + y * y);
  const double x2 = 2.0 * kPi4 * x * x1, y2 = 2.0 * kPi4 * y * y1;
  const double S = x * x + y * y + 1.0;
  const double dx[3] = {x1, 0.0, 0.0}, dy[3] = {0.0, y1, 0.0};
  const double dS[3] = {2.0 * x * x1, 2.0 * y * y1, 0.0};
  const double d2x[3][3] = {{x2, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  const double d2y[3][3] = {{0.0, 0.0, 0.0}, {0.0, y2, 0.0}, {0.0, 0.0, 0.0}};
  const double d2S[3][3] = {{2.0 * (x1 * x1 + x * x2), 0.0, 0.0}, {0.0, 2.0 * (y1 * y1 + y * y2), 0.0}, {0.0, 0.0, 0.0}};
  wedge_second(R, dR, d2R, S, dS, d2S, x, dx, d2x, y, dy, d2y, H);
}

// d^2 x_i / d xi_j d xi_k of the map P.type (same dispatch as tree_map_eval; the caller has checked type, tree and flags)
__host__ __device__ inline void tree_map_d2(const TreeMapParams& P, int tree, const double xi[3], double H[3][3][3]) {
  double h[3][3][3];
  bool cube = false;
  if (P.type == 1) {
    if (tree == 6) cube = true;
    else wedge_blended_d2(P.R0, P.R1, P.compactify, xi, h);
  } else if (tree < 6) {
    wedge_plain_d2(P.R1, P.R2, P.compactify_outer, xi, h);
  } else if (tree == 12) {
    cube = true;
  } else if (P.type == 3) {
    wedge_plain_d2(P.R0, P.R1, P.compactify, xi, h);
  } else {
    wedge_blended_d2(P.R0, P.R1, 0, xi, h);
  }
  if (cube) {   // centre_cube is linear
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) H[i][j][k] = 0.0;
    return;
  }
  // the signed picks of wedge_to_xyz
  const int wedge = tree % 6;
  const int pk0 = (wedge == 3 || wedge == 5) ? 2 : (wedge == 4 ? 1 : 0);
  const int pk1 = (wedge == 0 || wedge == 2) ? 2 : (wedge == 1 ? 1 : 0);
  const int pk2 = (wedge == 1 || wedge == 4) ? 2 : 1;
  const double sg0 = (wedge >= 4) ? -1.0 : 1.0;
  const double sg1 = (wedge == 1 || wedge == 2) ? 1.0 : -1.0;
  const double sg2 = (wedge >= 2 && wedge <= 4) ? -1.0 : 1.0;
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 3; ++k) {
      const double h0 = h[0][j][k], h1 = h[1][j][k], h2 = h[2][j][k];
      H[0][j][k] = sg0 * (pk0 == 0 ? h0 : pk0 == 1 ? h1 : h2);
      H[1][j][k] = sg1 * (pk1 == 0 ? h0 : pk1 == 1 ? h1 : h2);
      H[2][j][k] = sg2 * (pk2 == 1 ? h1 : h2);
    }
}

// inverse and determinant of a 3 x 3 matrix
__host__ __device__ inline double invert3(const double A[3][3], double I[3][3]) {
  const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2], c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
  const double det = A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02;
  const double r = 1.0 / det;
  I[0][0] = c00 * r; I[1][0] = c01 * r; I[2][0] = c02 * r;
  I[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * r;
  I[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * r;
  I[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * r;
  I[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * r;
  I[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * r;
  I[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * r;
  return det;
}

// a (possibly virtual) cell of the forest: tree, corner q (p4est integer coordinates), side dq
struct CellDesc {
  int tree, q[3], dq, face;
};

// d x / d r (element reference coordinates r in [-1,1]^3) of `cell` at reference point r
__host__ __device__ inline void cell_dxdr(const TreeMapParams& P, const CellDesc& cell, double root_len, const double r[3], double dxdr[3][3]) {
  double xi[3];
  for (int d = 0; d < 3; ++d) xi[d] = ((double)cell.q[d] + 0.5 * (double)cell.dq * (r[d] + 1.0)) / root_len;
  double D[3][3];
  tree_map_dxdxi(P, cell.tree, xi, D);
  const double s = 0.5 * (double)cell.dq / root_len;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) dxdr[i][j] = D[i][j] * s;
}

// x of `cell` at reference point r
__host__ __device__ inline void cell_x(const TreeMapParams& P, const CellDesc& cell, double root_len, const double r[3], double x[3]) {
  double xi[3];
  for (int d = 0; d < 3; ++d) xi[d] = ((double)cell.q[d] + 0.5 * (double)cell.dq * (r[d] + 1.0)) / root_len;
  tree_map_x(P, cell.tree, xi, x);
}

// d^2 x / d r d r of `cell` at reference point r: the tree-level second derivative times (dq / (2 root_len))^2
__host__ __device__ inline void cell_d2xdr(const TreeMapParams& P, const CellDesc& cell, double root_len, const double r[3],
                                           double d2[3][3][3]) {
  double xi[3];
  for (int d = 0; d < 3; ++d) xi[d] = ((double)cell.q[d] + 0.5 * (double)cell.dq * (r[d] + 1.0)) / root_len;
  double H[3][3][3];
  tree_map_d2(P, cell.tree, xi, H);
  const double s = 0.5 * (double)cell.dq / root_len, s2 = s * s;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) d2[i][j][k] = H[i][j][k] * s2;
}

}  // namespace d4est_hip
