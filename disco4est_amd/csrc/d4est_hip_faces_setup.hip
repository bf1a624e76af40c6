// Host set-up of the face part (d4est_hip_plan_set_faces): everything the trace / flux launchers of d4est_hip_faces.hip read -- the
// operator tables, the side, element and ghost-side descriptors, the mortar records of a mesh with hanging faces, and the decisions
// taken once per plan (uniform plan and direct tables, hp split, family split, the hybrid operator's clean / dirty classification).
#include <algorithm>
#include <map>
#include <tuple>

#include "d4est_hip_faces_host.h"
#include "d4est_hip_hybrid_buckets.h"
#include "d4est_hip_tables.h"
#include "d4est_hip_topology.h"

namespace d4est_hip {

namespace {
std::map<d4est_hip_plan*, FaceHost> g_face_host;
}
FaceHost& face_host(d4est_hip_plan* plan) { return g_face_host[plan]; }

// The 1-D operators of one table (face_ops or hp_ops), each built on first request and appended to `ops`: the members return offsets.
// child = -1: p-prolongation; 0 / 1: the hp-prolongation onto that half (the big side of a hanging face).
class FaceOpTable {
 public:
  explicit FaceOpTable(int quad_type) : qt(quad_type) {}
  std::vector<double> ops;

  // C: side (deg_side) -> mortar quadrature nodes (deg_mq): prolong to the Lobatto nodes of degree deg_mq, then Lobatto -> quadrature
  // nodes (d4est_laplacian_flux.c:635-694)
  int C(int deg_side, int deg_mq, int child = -1) {
    return memo(std::make_tuple(0, deg_side, deg_mq, 0, child), [&] {
      std::vector<double> P = prolong(deg_side, deg_mq, child);
      std::vector<double> I = Tables1D::quad_interp(qt, deg_mq, deg_mq);
      return Tables1D::matmul(I, P, deg_mq + 1, deg_mq + 1, deg_side + 1);
    });
  }
  // C * D: tangential derivative fused with the interpolation
  int CD(int deg_side, int deg_mq, int child = -1) {
    return memo(std::make_tuple(4, deg_side, deg_mq, 0, child), [&] {
      const int offC = C(deg_side, deg_mq, child);
      std::vector<double> Cm(ops.begin() + offC, ops.begin() + offC + (size_t)(deg_mq + 1) * (deg_side + 1));
      return Tables1D::matmul(Cm, Tables1D::dij(deg_side), deg_mq + 1, deg_side + 1, deg_side + 1);
    });
  }
  // E: mortar quadrature nodes (deg_mq) -> Lobatto nodes of deg_ml (V^T W, the galerkin integral) -> side (the prolongation transposed,
  // deg_m <- deg_ml): sipg.c:641-734
  int E(int deg_m, int deg_ml, int deg_mq, int child = -1) {
    return memo(std::make_tuple(1, deg_m, deg_ml, deg_mq, child), [&] {
      std::vector<double> I = Tables1D::quad_interp(qt, deg_ml, deg_mq);              // (mq+1) x (ml+1)
      std::vector<double> w = Tables1D::quad_weights(qt, deg_mq);
      std::vector<double> ItW = Tables1D::transpose(I, deg_mq + 1, deg_ml + 1);       // (ml+1) x (mq+1)
      for (int r = 0; r <= deg_ml; ++r)
        for (int c = 0; c <= deg_mq; ++c) ItW[(size_t)r * (deg_mq + 1) + c] *= w[c];
      std::vector<double> P = prolong(deg_m, deg_ml, child);                          // (ml+1) x (m+1)
      std::vector<double> Pt = Tables1D::transpose(P, deg_ml + 1, deg_m + 1);         // (m+1) x (ml+1)
      return Tables1D::matmul(Pt, ItW, deg_m + 1, deg_ml + 1, deg_mq + 1);
    });
  }
  // derivative matrices: unpadded (generic kernels) and zero-padded 8 x 8 (fast path, degrees <= 7)
  int D(int deg, bool padded) {
    return memo(std::make_tuple(padded ? 3 : 2, deg, 0, 0, -1), [&] {
      std::vector<double> Dm = Tables1D::dij(deg);
      if (!padded) return Dm;
      const int n = deg + 1;
      std::vector<double> P(64, 0.0);
      for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) P[r * 8 + c] = Dm[(size_t)r * n + c];
      return P;
    });
  }

 private:
  int qt;
  std::map<std::tuple<int, int, int, int, int>, int> index;   // (kind, deg_a, deg_b, deg_c, child) -> offset

  std::vector<double> prolong(int deg_from, int deg_to, int child) const {
    if (child < 0) return Tables1D::p_prolong(deg_from, deg_to);
    const int nh = deg_to + 1, nH = deg_from + 1;
    std::vector<double> P2 = Tables1D::hp_prolong(deg_from, deg_to);
    return std::vector<double>(P2.begin() + (size_t)child * nh * nH, P2.begin() + (size_t)(child + 1) * nh * nH);
  }
  // offsets follow the order of the requests (an operator that `make` requests itself comes first)
  template <typename Make>
  int memo(const std::tuple<int, int, int, int, int>& key, Make make) {
    auto it = index.find(key);
    if (it != index.end()) return it->second;
    const std::vector<double> m = make();
    const int off = (int)ops.size();
    ops.insert(ops.end(), m.begin(), m.end());
    index[key] = off;
    return off;
  }
};

// dGMath/d4est_reference.c:3-12, :84-110: index, in the (+) side's own order, of the sub-face that is i in (-) order
int reorient_face_order(int f_m, int f_p, int o, int i) {
  using namespace topo;   // d4est_hip_topology.h: the tables, pinned entry by entry to the reference's own by tests/test_topology_tables.py
  return d4est_perm_to_order[d4est_code_to_perm[d4est_FToF_code[f_m][f_p]][o]][i];
}

// The (flip0, flip1, transpose) code d4est_operators_reorient_face_data derives from a tree-boundary face pair
// (dGMath/d4est_operators.c:2031-2050): p8est's face transform of the pair (lower face number, higher face number, orientation)
// -- axes of the lower face's tangential directions, the axes they map to, and whether each is reversed
// (p4est_expand_face_transform: my_axis = ft[0..2], target_axis = ft[3..5], edge_reverse = ft[6..8]).
int face_reorder_code(int f_m, int f_p, int o) {
  const auto& refs = topo::face_permutation_refs;
  const int* ref0 = refs[0];
  const int lo = f_m <= f_p ? f_m : f_p, hi = f_m <= f_p ? f_p : f_m;
  int my_axis[2], target_axis[2], edge_reverse[2];
  my_axis[0] = lo < 2 ? 1 : 0;
  my_axis[1] = lo < 4 ? 2 : 1;
  const int swap_axes = ref0[lo] ^ ref0[hi] ^ ((o == 0 || o == 3) ? 1 : 0);
  target_axis[swap_axes] = hi < 2 ? 1 : 0;
  target_axis[!swap_axes] = hi < 4 ? 2 : 1;
  const int swap_rev = (refs[lo][hi] == 1);
  edge_reverse[swap_rev] = o & 1;
  edge_reverse[!swap_rev] = o >> 1;
  const int aligned = (my_axis[1] - my_axis[0]) * (target_axis[1] - target_axis[0]) > 0;
  return edge_reverse[0] | (edge_reverse[1] << 1) | ((!aligned) << 2);
}

// Small side of a hanging face, sub-face c in its own (= (-)) order.  The reference slices the WHOLE big face, re-orients it with the
// (flip0, flip1, transpose) code and hp-prolongs the result onto child c (dGMath/d4est_laplacian_flux.c:575-657): u on sub-mortar c
// comes from the big element's own child that the code maps onto c.  The gradient comes from the child
// d4est_reference_reorient_face_order names (:733-830, :858-900).  The two agree whenever the code is the geometric map between the
// faces; for a transposed pair with exactly one flip seen from the lower-numbered face (codes 5, 6) the reference's re-orientation is
// not geometric (forest.reference_reorientation_is_consistent) and they differ -- followed here as the reference computes it.
static int small_side_u_child(int code, int c) {
  int ha = (code & 4) ? (c >> 1) : (c & 1), hb = (code & 4) ? (c & 1) : (c >> 1);
  if (code & 2) hb ^= 1;
  if (code & 1) ha ^= 1;
  return ha + 2 * hb;
}
static const char* kNonGeometricMsg =
    "the reference's re-orientation of this tree-face pair is not geometric (transposed with one flip, seen from the lower face)";

// Mortar records of a mesh with hanging faces (plan->side_hang etc. set by d4est_hip_plan_set_hanging).
struct HpRecords {
  std::vector<HpMortar> rec;
  std::vector<HpGeomSrc> gsrc;
  std::vector<int> elem_first, side_first;   // first record of element e (ne + 1 entries) / of side s
  long long trace_doubles = 0;               // the records' trace blocks, in record order
  int max_fld = 1, maxN = 1;
};

// the records element by element, side by side, with their operators in `table` and their own trace blocks
static HpRecords hp_build_records(d4est_hip_plan* plan, FaceOpTable& table) {
  const int ne = plan->n_elements;
  const size_t ns = 6 * (size_t)ne;
  // element references: >= 0 local, <= -2 ghost g = -(ref + 2)
  auto valid_ref = [&](int ref) { return (ref >= 0 && ref < ne) || (ref <= -2 && -(ref + 2) < plan->n_ghost); };
  auto deg_of = [&](int ref) { return ref >= 0 ? plan->deg[ref] : plan->ghost_deg[-(ref + 2)]; };
  auto degq_of = [&](int ref) { return ref >= 0 ? plan->deg_quad[ref] : plan->ghost_deg_quad[-(ref + 2)]; };
  auto degq_mortar = [&](int em, int ep) { return std::max(degq_of(em), degq_of(ep)); };
  auto nodes2 = [](int deg) { return (deg + 1) * (deg + 1); };
  HpRecords R;
  std::vector<HpMortar>& rec = R.rec;
  std::vector<HpGeomSrc>& gsrc = R.gsrc;
  std::vector<int>&elem_first = R.elem_first, &side_first = R.side_first;
  elem_first.assign(ne + 1, 0);
  side_first.assign(ns, 0);
  long long& qoff = R.trace_doubles;
  int &max_fld = R.max_fld, &maxN = R.maxN;
  for (int e = 0; e < ne; ++e) {
    elem_first[e] = (int)rec.size();
    const int deg_m = plan->deg[e], degq_m = plan->deg_quad[e];
    maxN = std::max(maxN, deg_m + 1);
    for (int f = 0; f < 6; ++f) {
      const size_t s = 6 * (size_t)e + f;
      side_first[s] = (int)rec.size();
      plan->trace_offset[s] = qoff;
      const int hang = plan->side_hang[s], nbr = plan->side_nbr[s], f_p = plan->side_nbr_face[s], o = plan->side_orientation[s];
      if (hang < 0 || hang > 2) D4EST_HIP_ABORT("plan_set_hanging: side %zu has side_hang %d", s, hang);
      if (o < 0 || o > 3) D4EST_HIP_ABORT("plan_set_hanging: side %zu has orientation %d", s, o);
      const int n_sub = (hang == 1) ? 4 : 1;
      const int* n4 = &plan->side_nbr4[4 * s];
      if (hang != 0)
        for (int i = 0; i < 4; ++i)
          if (!valid_ref(n4[i])) D4EST_HIP_ABORT("plan_set_hanging: side %zu: side_nbr4[%d] = %d is neither a local nor a ghost element", s, i, n4[i]);
      if (hang == 2 && !valid_ref(nbr)) D4EST_HIP_ABORT("plan_set_hanging: small side %zu: (+) element %d is neither local nor ghost", s, nbr);
      // mortar sizes of the whole hanging face, in (-) order and in (+) order
      int T_m[4] = {0, 0, 0, 0}, T_p[4] = {0, 0, 0, 0};
      if (hang != 0) {
        for (int i = 0; i < 4; ++i) {
          T_m[i] = nodes2(hang == 1 ? degq_mortar(e, n4[i]) : degq_mortar(n4[i], nbr));
          T_p[reorient_face_order(f, f_p, o, i)] = T_m[i];
        }
      }
      for (int i = 0; i < n_sub; ++i) {
        HpMortar m{};
        HpGeomSrc g{};
        m.elem = e;
        m.face = f;
        m.code = plan->side_reorder[s];
        m.N = deg_m + 1;
        m.first = (i == 0);
        m.last = (i == n_sub - 1);
        m.fm = m.fp = m.w2 = 1.0;
        m.hang = (double)hang;
        int ep = -1, sub_m = 0;   // (+) element of this mortar; index of the mortar in the face's (-) order
        if (hang == 0) {
          if (nbr != -1 && !valid_ref(nbr)) D4EST_HIP_ABORT("plan_set_faces: side %zu neighbour %d out of range", s, nbr);
          m.kind = (nbr == -1) ? 0 : 1;
          ep = nbr;
        } else if (hang == 1) {
          m.kind = 1;
          ep = n4[i];
          sub_m = i;
          m.fm = 0.5;   // the big element's gradient on the half-size mortar
          m.w2 = 0.5;
        } else {
          m.kind = 1;
          ep = nbr;
          sub_m = plan->side_sub[s];
          if (sub_m < 0 || sub_m > 3 || n4[sub_m] != e) D4EST_HIP_ABORT("plan_set_hanging: small side %zu: side_sub %d does not point at the element in side_nbr4", s, sub_m);
          m.fp = 0.5;
        }
        if (m.kind != 0 && ep <= -2) m.kind = 2;
        const int deg_p = (m.kind == 0) ? deg_m : deg_of(ep);
        const int deg_mq = (m.kind == 0) ? degq_m : degq_mortar(e, ep);
        const int deg_ml = std::max(deg_m, deg_p);
        m.NQ = deg_mq + 1;
        const int ca = (hang == 1) ? (i & 1) : -1, cb = (hang == 1) ? (i >> 1) : -1;
        m.offCa = table.C(deg_m, deg_mq, ca);
        m.offCb = table.C(deg_m, deg_mq, cb);
        m.offCDa = table.CD(deg_m, deg_mq, ca);
        m.offCDb = table.CD(deg_m, deg_mq, cb);
        m.offEa = table.E(deg_m, deg_ml, deg_mq, ca);
        m.offEb = table.E(deg_m, deg_ml, deg_mq, cb);
        g.S = plan->side_mortar_stride[s];
        g.off = 0;
        g.off_p = 0;
        g.Ttot = nodes2(deg_mq);
        if (hang != 0) {
          g.Ttot = T_m[0] + T_m[1] + T_m[2] + T_m[3];
          for (int j = 0; j < sub_m; ++j) g.off += T_m[j];
          const int sub_p = reorient_face_order(f, f_p, o, sub_m);
          for (int j = 0; j < sub_p; ++j) g.off_p += T_p[j];
        }
        g.deg_m = deg_m;
        g.deg_p = deg_p;
        m.gidx = g.S + g.off;
        if ((long long)m.gidx + nodes2(deg_mq) > plan->total_mortar_nodes) D4EST_HIP_ABORT("plan_set_faces: side %zu mortar data exceeds total_mortar_nodes", s);
        m.qoff = qoff;
        qoff += 4LL * nodes2(deg_mq);
        max_fld = std::max(max_fld, std::max(m.NQ * m.NQ, m.NQ * m.N));
        rec.push_back(m);
        gsrc.push_back(g);
      }
    }
  }
  elem_first[ne] = (int)rec.size();
  return R;
}

// (+) blocks: local ones by record lookup; ghost ones get consecutive slots of the ghost trace buffer in record order; the plan's
// per-record and per-side offsets (the exchange reads them)
static void hp_link_records(d4est_hip_plan* plan, HpRecords& R) {
  std::vector<HpMortar>& rec = R.rec;
  const std::vector<int>& side_first = R.side_first;
  const size_t ns = side_first.size();
  long long goff = 0;
  plan->rec_qoff.assign(rec.size(), 0);
  plan->rec_goff.assign(rec.size(), -1);
  plan->rec_len.assign(rec.size(), 0);
  plan->side_first_rec.assign(side_first.begin(), side_first.end());
  plan->side_first_rec.push_back((int)rec.size());
  for (size_t r = 0; r < rec.size(); ++r) {
    HpMortar& m = rec[r];
    plan->rec_qoff[r] = m.qoff;
    plan->rec_len[r] = 4 * m.NQ * m.NQ;
    if (m.kind == 2) {
      m.nbr_qoff = goff;
      plan->rec_goff[r] = goff;
      goff += 4LL * m.NQ * m.NQ;
      const size_t sg = 6 * (size_t)m.elem + m.face;
      if (plan->side_hang[sg] == 2 &&
          small_side_u_child(m.code, plan->side_sub[sg]) != reorient_face_order(m.face, plan->side_nbr_face[sg], plan->side_orientation[sg], plan->side_sub[sg]))
        D4EST_HIP_ABORT("plan_set_hanging: small side %zu: %s, and the big element is on another rank", sg, kNonGeometricMsg);
      continue;
    }
    if (m.kind == 0) continue;
    const size_t s = 6 * (size_t)m.elem + m.face;
    const int hang = plan->side_hang[s], f_p = plan->side_nbr_face[s], o = plan->side_orientation[s];
    int ep, sub_p = 0;
    if (hang == 1) ep = plan->side_nbr4[4 * s + (int)(r - side_first[s])];
    else ep = plan->side_nbr[s];
    const size_t sp = 6 * (size_t)ep + f_p;
    const int hang_p = plan->side_hang[sp];
    if ((hang == 0 && hang_p != 0) || (hang == 1 && hang_p != 2) || (hang == 2 && hang_p != 1))
      D4EST_HIP_ABORT("plan_set_hanging: sides %zu and %zu disagree about the hanging face", s, sp);
    if (hang == 2) sub_p = reorient_face_order(m.face, f_p, o, plan->side_sub[s]);   // the big element's own sub-mortar index
    const HpMortar& mp = rec[side_first[sp] + sub_p];
    if (mp.NQ != m.NQ) D4EST_HIP_ABORT("plan_set_hanging: sides %zu and %zu disagree on the mortar degree", s, sp);
    m.nbr_qoff = mp.qoff;
    if (hang == 2) {
      const int sub_u = small_side_u_child(m.code, plan->side_sub[s]);
      if (sub_u != sub_p) {
        const HpMortar& mu = rec[side_first[sp] + sub_u];
        if (mu.NQ != m.NQ) D4EST_HIP_ABORT("plan_set_hanging: small side %zu: %s, and its sub-mortars have different quadrature degrees", s, kNonGeometricMsg);
        m.u_shift = (int)(mu.qoff - mp.qoff);
      }
    }
  }
  plan->local_trace_doubles = R.trace_doubles;
  plan->ghost_trace_doubles = goff;
  for (size_t s_ = 0; s_ < ns; ++s_) plan->ghost_trace_offset[s_] = plan->rec_goff[side_first[s_]];
}

static void faces_setup_hp(d4est_hip_plan* plan, FaceHost& fh) {
  FaceOpTable table(plan->quad_type);   // hp_ops: a table of its own, the records' offsets index it
  HpRecords R = hp_build_records(plan, table);
  hp_link_records(plan, R);
  const std::vector<HpMortar>& rec = R.rec;
  const std::vector<HpGeomSrc>& gsrc = R.gsrc;
  const std::vector<int>&elem_first = R.elem_first, &side_first = R.side_first;
  const int maxN = R.maxN, max_fld = std::max(R.max_fld, maxN * maxN);
  fh.hp = true;
  fh.n_rec = (int)rec.size();
  fh.hp_fld_stride = max_fld;
  fh.hp_lds_doubles = (size_t)12 * max_fld + (size_t)maxN * maxN * maxN + (size_t)maxN * maxN;
  if (fh.hp_lds_doubles * sizeof(double) > 160 * 1024) D4EST_HIP_ABORT("hanging-face kernels need %zu LDS doubles", fh.hp_lds_doubles);
  fh.d_rec = fh.upload(rec);
  fh.rec_host = rec;
  fh.d_gsrc = fh.upload(gsrc);
  fh.gsrc_host = gsrc;
  fh.d_elem_first = fh.upload(elem_first);
  {
    std::vector<int> sf(side_first.begin(), side_first.end());
    sf.push_back((int)rec.size());
    fh.d_side_first = fh.upload(sf);
  }
  fh.hp_max_N = maxN;
  fh.hp_max_NQ = 1;
  for (const HpMortar& m_ : rec) fh.hp_max_NQ = std::max(fh.hp_max_NQ, m_.NQ);
  fh.d_hp_ops = fh.upload(table.ops);
  plan->face_fast = false;
}

// ---- the stages of faces_setup, in the order they run: each reads the plan and the results of the stages before it

// per side sizes; the local trace block of side s is 4 T_s doubles in side order
struct SideSizes {
  bool hp = false;                        // the mesh has a hanging face
  std::vector<int> deg_mq_of, deg_p_of;   // per side: degree of the mortar's quadrature, degree of the (+) element
  std::vector<long long> ghost_u_off;     // per ghost element: its offset in the packed ghost vector
  int maxN = 1, maxNQ = 1;
  bool fast = true;                       // every N, NQ <= 8
};

static SideSizes side_sizes(d4est_hip_plan* plan) {
  const int ne = plan->n_elements;
  const size_t ns = 6 * (size_t)ne;
  SideSizes z;
  if (!plan->side_hang.empty())
    for (int v : plan->side_hang) z.hp = z.hp || (v != 0);
  plan->trace_offset.assign(ns, 0);
  plan->ghost_trace_offset.assign(ns, -1);
  z.ghost_u_off.assign(plan->n_ghost, 0);
  {
    long long o = 0;
    for (int g = 0; g < plan->n_ghost; ++g) {
      z.ghost_u_off[g] = o;
      const long long n = plan->ghost_deg[g] + 1;
      o += n * n * n;
    }
  }
  long long qoff = 0;
  for (int e = 0; e < ne; ++e) z.maxN = std::max(z.maxN, plan->deg[e] + 1);
  for (int g = 0; g < plan->n_ghost; ++g) z.maxN = std::max(z.maxN, plan->ghost_deg[g] + 1);
  // mortar degrees and offsets
  z.deg_mq_of.resize(ns);
  z.deg_p_of.resize(ns);
  for (int e = 0; e < ne; ++e)
    for (int f = 0; f < 6; ++f) {
      const size_t s = 6 * (size_t)e + f;
      const bool hanging = z.hp && plan->side_hang[s] != 0;
      // hanging sides are served by the mortar records (descriptor kind 3); a SMALL side still gets the degrees of its mortar with the
      // big element, so that the hp split can hand it to the conforming kernels (one mortar, p-prolongation only: it is one of theirs)
      const int nbr = hanging ? ((plan->side_hang[s] == 2 && plan->side_nbr[s] != -1) ? plan->side_nbr[s] : -1) : plan->side_nbr[s];
      const int deg_m = plan->deg[e], degq_m = plan->deg_quad[e];
      int deg_p = deg_m, degq_p = degq_m;
      if (nbr >= 0) {
        if (nbr >= ne) D4EST_HIP_ABORT("plan_set_faces: side %zu neighbour %d out of range", s, nbr);
        deg_p = plan->deg[nbr];
        degq_p = plan->deg_quad[nbr];
      } else if (nbr <= -2) {
        const int g = -(nbr + 2);
        if (g >= plan->n_ghost) D4EST_HIP_ABORT("plan_set_faces: side %zu ghost %d out of range", s, g);
        deg_p = plan->ghost_deg[g];
        degq_p = plan->ghost_deg_quad[g];
      }
      z.deg_mq_of[s] = (nbr == -1) ? degq_m : std::max(degq_m, degq_p);   // (max: also d4est's rule for a hanging face's mortars)
      z.deg_p_of[s] = deg_p;
      const long long T = (long long)(z.deg_mq_of[s] + 1) * (z.deg_mq_of[s] + 1);
      plan->trace_offset[s] = qoff;
      qoff += 4 * T;
      z.maxNQ = std::max(z.maxNQ, z.deg_mq_of[s] + 1);
    }
  plan->local_trace_doubles = qoff;
  z.fast = (z.maxN <= 8 && z.maxNQ <= 8);
  return z;
}

struct Descriptors {
  std::vector<SideDesc> sd;
  std::vector<ElemDesc> edv, edg;      // offD -> the padded 8 x 8 matrices where the p <= 7 kernels can serve the element / the unpadded ones
  std::vector<GhostSideDesc> gsides;
};

// the side, element and ghost-side descriptors with their operators in `table`, the ghost trace offsets, the LDS the generic kernels need
static Descriptors build_descriptors(d4est_hip_plan* plan, FaceHost& fh, const SideSizes& z, FaceOpTable& table) {
  const int ne = plan->n_elements;
  const size_t ns = 6 * (size_t)ne;
  const bool hp = z.hp;
  Descriptors D;
  D.sd.resize(ns);
  fh.side_deg_m.assign(ns, 0);
  fh.side_deg_p.assign(ns, 0);
  long long goff = 0;
  // D4EST_HIP_TUNE_GHOST_ALIAS: every ghost side reads block 0 (a constant ghost trace, e.g. the zero trace of a Schwarz subdomain plan)
  const bool ghost_alias = plan->tuning[D4EST_HIP_TUNE_GHOST_ALIAS] > 0 && !hp;
  long long ghost_alias_len = 0;
  int max_fld = 1;
  for (int e = 0; e < ne; ++e)
    for (int f = 0; f < 6; ++f) {
      const size_t s = 6 * (size_t)e + f;
      SideDesc d{};
      const bool hanging = hp && plan->side_hang[s] != 0;
      const int nbr = hanging ? -1 : plan->side_nbr[s];
      const int deg_m = plan->deg[e], deg_p = z.deg_p_of[s], deg_mq = z.deg_mq_of[s];
      const int deg_ml = std::max(deg_m, deg_p);
      d.kind = hanging ? 3 : ((nbr == -1) ? 0 : (nbr >= 0 ? 1 : 2));
      d.code = plan->side_reorder[s];
      d.NQ = deg_mq + 1;
      d.offC = table.C(deg_m, deg_mq);
      d.offCD = table.CD(deg_m, deg_mq);
      d.pad0 = 0;
      d.offE = table.E(deg_m, d.kind == 0 ? deg_m : deg_ml, deg_mq);
      d.geom = plan->side_mortar_stride[s];
      d.qoff = plan->trace_offset[s];
      d.nbr_qoff = 0;
      if (d.kind == 1 && !hp) {
        const size_t sp = 6 * (size_t)nbr + plan->side_nbr_face[s];
        if (z.deg_mq_of[sp] != deg_mq) D4EST_HIP_ABORT("plan_set_faces: sides %zu and %zu disagree on the mortar degree (non-conforming mortar?)", s, sp);
        d.nbr_qoff = plan->trace_offset[sp];
      } else if (d.kind == 2 && !hp) {
        const int g = -(nbr + 2);
        plan->ghost_trace_offset[s] = goff;
        d.nbr_qoff = goff;
        GhostSideDesc gs{};
        gs.N = plan->ghost_deg[g] + 1;
        gs.f = plan->side_nbr_face[s];
        gs.NQ = deg_mq + 1;
        gs.offC = table.C(plan->ghost_deg[g], deg_mq);
        gs.offD = table.D(plan->ghost_deg[g], false);
        gs.u_off = z.ghost_u_off[g];
        gs.goff = goff;
        D.gsides.push_back(gs);
        if (ghost_alias) ghost_alias_len = std::max(ghost_alias_len, 4LL * (deg_mq + 1) * (deg_mq + 1));
        else goff += 4LL * (deg_mq + 1) * (deg_mq + 1);
      }
      D.sd[s] = d;
      fh.side_deg_m[s] = deg_m;
      fh.side_deg_p[s] = deg_p;
      max_fld = std::max(max_fld, std::max(d.NQ * d.NQ, d.NQ * (deg_m + 1)));
      max_fld = std::max(max_fld, d.NQ * (deg_p + 1));
    }
  plan->ghost_trace_doubles = ghost_alias ? ghost_alias_len : goff;   // (hanging plans: overwritten by faces_setup_hp)
  max_fld = std::max(max_fld, z.maxN * z.maxN);
  fh.fld_stride = max_fld;
  fh.max_N = z.maxN;
  fh.max_NQ = z.maxNQ;
  fh.max_local_N = 1;
  for (int e = 0; e < ne; ++e) fh.max_local_N = std::max(fh.max_local_N, plan->deg[e] + 1);
  fh.n_ghost_sides = (int)D.gsides.size();
  plan->face_fast = z.fast;
  plan->max_face_lds_doubles = 12 * max_fld + z.maxN * z.maxN * z.maxN + z.maxN * z.maxN;
  if ((size_t)plan->max_face_lds_doubles * sizeof(double) > 160 * 1024) D4EST_HIP_ABORT("face kernels need %d LDS doubles", plan->max_face_lds_doubles);

  D.edv.resize(ne);
  D.edg.resize(ne);
  for (int e = 0; e < ne; ++e) {
    D.edv[e].N = D.edg[e].N = plan->deg[e] + 1;
    D.edv[e].ns = D.edg[e].ns = plan->nodal_stride[e];
    D.edg[e].offD = table.D(plan->deg[e], false);
    D.edv[e].offD = (z.fast || plan->deg[e] + 1 <= 8) ? table.D(plan->deg[e], true) : D.edg[e].offD;
    D.edv[e].pad = D.edg[e].pad = 0;
  }
  return D;
}

// uniform plan? (one degree, one mortar degree, contiguous element and trace strides) -- and, on one whose sides all see the local degree,
// the direct tables
static TraceUniform uniform_plan_and_direct_tables(d4est_hip_plan* plan, FaceHost& fh, const SideSizes& z, const Descriptors& D, const FaceOpTable& table) {
  const int ne = plan->n_elements;
  const size_t ns = 6 * (size_t)ne;
  const std::vector<SideDesc>& sd = D.sd;
  const std::vector<ElemDesc>& edv = D.edv;
  TraceUniform un{};
  if (ne > 0 && !z.hp) {
    bool uniform = true;
    const int N0 = edv[0].N, n3 = N0 * N0 * N0;
    for (int e = 0; e < ne && uniform; ++e) uniform = (edv[e].N == N0) && (edv[e].ns == edv[0].ns + e * n3);
    const long long qs = 4LL * sd[0].NQ * sd[0].NQ;
    for (size_t s_ = 0; s_ < ns && uniform; ++s_)
      uniform = (sd[s_].NQ == sd[0].NQ) && (sd[s_].offC == sd[0].offC) && (sd[s_].offCD == sd[0].offCD) && (sd[s_].qoff == sd[0].qoff + (long long)s_ * qs);
    if (uniform) {
      un.N = N0; un.NQ = sd[0].NQ; un.offC = sd[0].offC; un.offCD = sd[0].offCD; un.offD = edv[0].offD;
      un.ns0 = edv[0].ns; un.ns_stride = n3; un.q0 = sd[0].qoff; un.q_stride = qs;
    }
  }
  if (z.fast) fh.uni = un;   // (the uniform forms of the trace kernels exist for N, NQ <= 8 only)
  // the direct kernels (d4est_hip_direct.hip: one wavefront per element, deg_quad <= 7; d4est_hip_direct_mw.hip: one multi-wave
  // workgroup per element, deg = deg_quad = 8 ... 15) take over apply_aij on uniform conforming plans whose sides all see the local degree
  if (un.N > 0) {
    bool same = true;
    for (size_t s_ = 0; s_ < ns && same; ++s_) same = (sd[s_].offE == sd[0].offE) && (z.deg_p_of[s_] == plan->deg[0]) && sd[s_].kind != 3;
    if (same && sd[0].NQ >= un.N && (z.fast ? sd[0].NQ * sd[0].NQ <= 64 : true))
      direct_setup(plan, un.N, sd[0].NQ, un.ns0, un.ns_stride, table.ops.data() + un.offC, table.ops.data() + un.offCD, table.ops.data() + sd[0].offE);
  }
  return un;
}

static void upload_descriptors(d4est_hip_plan* plan, FaceHost& fh, const Descriptors& D, FaceOpTable& table) {
  table.ops.resize(table.ops.size() + 64, 0.0);  // slack: the fast kernels read 64-entry images
  plan->d_elem_desc = upload_vec(D.edv);
  fh.d_elem_desc_generic = fh.upload(D.edg);
  plan->d_side_desc = reinterpret_cast<int*>(upload_vec(D.sd));
  fh.sd_host = D.sd;
  plan->d_face_ops = upload_vec(table.ops);
  fh.d_side_deg_m = fh.upload(fh.side_deg_m);
  fh.d_side_deg_p = fh.upload(fh.side_deg_p);
  fh.d_side_bndry_stride = fh.upload(plan->side_bndry_stride);
  fh.d_ghost_sides = fh.upload(D.gsides);
}

// ---- hp split.  A mesh with hanging faces is mostly conforming (2:1 interfaces of a locally refined forest): where every degree is
// <= 7 the conforming sides go to the fast kernels of the conforming path (one wavefront per face, scalar-operand contractions) and
// only the hanging sides to the tiled mortar-record kernels, over the list of elements that have one.  Both families write the same
// trace array (offsets of the records: a conforming side's block is its single record's) and add into the same A u.  A hanging
// side keeps kind 3 in the conforming descriptors: the fast trace kernel fills its block with a pretend-conforming trace that the
// record kernel, launched after it, overwrites (the block is at least as long), the fast flux kernel reads zeros for it.
// Relabels the small sides it hands to the conforming kernels in `sd` (in place, also where the split is not taken in the end).
static void hp_split(d4est_hip_plan* plan, FaceHost& fh, const SideSizes& z, std::vector<SideDesc>& sd) {
  const int ne = plan->n_elements;
  // (degrees above 7 -- round 4: the conforming sides then go through the tiled 16 x 16 conforming kernels, or, family split below, through
  // both conforming families on lists; D4EST_HIP_HP_SPLIT_FAST_ONLY=1 keeps such plans on the record kernels throughout)
  const bool split_fast = z.fast && fh.hp_max_N <= 8 && fh.hp_max_NQ <= 8;
  const bool split_tiled = !split_fast && fh.hp_max_N <= 16 && fh.hp_max_NQ <= 16 && fh.max_N <= 16 && fh.max_NQ <= 16 && !std::getenv("D4EST_HIP_HP_SPLIT_FAST_ONLY");
  if (!(z.hp && (split_fast || split_tiled) && plan->tuning[D4EST_HIP_TUNE_HP_SPLIT] != 0 &&
        plan->tuning[D4EST_HIP_TUNE_FLUX_FAST] != 0 && plan->tuning[D4EST_HIP_TUNE_FLUX_FAST] != 1))
    return;
  std::vector<int> hang_elems;
  std::vector<HpMortar> rec = fh.rec_host;
  bool ok = true;
  for (int e = 0; e < ne && ok; ++e) {
    bool any = false;
    for (int f = 0; f < 6; ++f) {
      const size_t s_ = 6 * (size_t)e + f;
      SideDesc& d = sd[s_];
      d.qoff = plan->trace_offset[s_];
      const int hang = plan->side_hang[s_];
      if (hang == 2) {
        // a small side: ONE mortar, its own trace p-prolonged to the mortar nodes, the (+) block = the big element's sub-mortar, the
        // hanging factor folded into the geometric factors -- to the conforming kernels it is an ordinary interior side (unless
        // the reference's non-geometric re-orientation shifts the block it reads u from: those stay with the record kernel)
        HpMortar& m = rec[plan->side_first_rec[s_]];
        if ((m.kind == 1 || m.kind == 2) && m.u_shift == 0 && m.NQ == d.NQ && plan->side_first_rec[s_ + 1] == plan->side_first_rec[s_] + 1) {
          d.kind = m.kind;   // (2: the big element is a ghost -- its sub-mortar block arrives in the ghost trace buffer at the record's offset)
          d.geom = m.gidx;
          d.nbr_qoff = m.nbr_qoff;
          m.hang = 0.0;   // (the record kernel skips it)
          continue;
        }
      }
      if (hang != 0) { any = true; continue; }
      if (d.kind == 1) {
        const size_t sp = 6 * (size_t)plan->side_nbr[s_] + plan->side_nbr_face[s_];
        if (plan->side_hang[sp] != 0 || z.deg_mq_of[sp] != z.deg_mq_of[s_]) { ok = false; break; }
        d.nbr_qoff = plan->trace_offset[sp];
      } else if (d.kind == 2) {
        // a conforming side against a ghost: the exchanged block sits where the side's (single) record expects it
        const HpMortar& m = rec[plan->side_first_rec[s_]];
        if (m.kind != 2 || m.NQ != d.NQ || m.u_shift != 0) { ok = false; break; }
        d.nbr_qoff = m.nbr_qoff;
      }
    }
    if (any) hang_elems.push_back(e);
  }
  // measured (level-4 brick, p = 7, every 64th / 32nd / 16th / 8th / 3rd octant refined): apply_aij 203 -> 139, 236 -> 170, 292 -> 210,
  // 402 -> 292, 661 -> 448 us.  The record kernel's cost is per listed element (those with a BIG hanging side, or a small side the
  // conforming kernels cannot take): should they ever be more than half of the mesh, the split is not taken (tuning value 1 forces it)
  if (ok && plan->tuning[D4EST_HIP_TUNE_HP_SPLIT] < 0 && 2 * hang_elems.size() > (size_t)ne) ok = false;
  if (!ok) return;
  fh.hp_split = true;
  fh.hp_split_fast = split_fast;
  fh.hang_elems = fh.upload_list(hang_elems);
  // the units: per listed element its sides with a live record (D4EST_HIP_NO_HANG_UNITS=1 keeps the serial record kernels)
  if (!std::getenv("D4EST_HIP_NO_HANG_UNITS")) {
    std::vector<HangUnit> units;
    std::vector<int> unit_first(1, 0);
    bool units_ok = true;
    for (int e : hang_elems) {
      for (int f = 0; f < 6; ++f) {
        const size_t s_ = 6 * (size_t)e + f;
        const int r0 = plan->side_first_rec[s_], r1 = plan->side_first_rec[s_ + 1];
        int live = 0;
        for (int r = r0; r < r1; ++r) live += rec[r].hang != 0.0;
        if (live == 0) continue;
        if (live != r1 - r0 || r1 - r0 > 4) { units_ok = false; break; }
        units.push_back(HangUnit{e, f, r0, r1 - r0});
      }
      unit_first.push_back((int)units.size());
    }
    if (units_ok && !units.empty()) {
      fh.n_units = (int)units.size();
      fh.d_units = fh.upload(units);
      fh.d_unit_first = fh.upload(unit_first);
    }
  }
  if (!sd.empty()) HIP_CHECK(hipMemcpy(plan->d_side_desc, sd.data(), sd.size() * sizeof(SideDesc), hipMemcpyHostToDevice));
  if (!rec.empty()) HIP_CHECK(hipMemcpy(fh.d_rec, rec.data(), rec.size() * sizeof(HpMortar), hipMemcpyHostToDevice));
}

// the element's own degree and its six mortars all fit 8 x 8: one of the p <= 7 kernels' elements under the family split
static bool element_is_small(const d4est_hip_plan* plan, const SideSizes& z, int e) {
  bool sm = plan->deg[e] + 1 <= 8;
  for (int f = 0; f < 6 && sm; ++f) {
    const size_t s_ = 6 * (size_t)e + f;
    sm = z.deg_mq_of[s_] + 1 <= 8 && z.deg_p_of[s_] + 1 <= 8;
  }
  return sm;
}

// ---- family split of a conforming mixed-degree plan whose largest degree is above 7 (see FaceHost)
static void family_split(d4est_hip_plan* plan, FaceHost& fh, const SideSizes& z) {
  const int ne = plan->n_elements;
  if (!((!z.hp || (fh.hp_split && !fh.hp_split_fast)) && !z.fast && ne > 0 && fh.max_N <= 16 && fh.max_NQ <= 16 && plan->tuning[D4EST_HIP_TUNE_FLUX_FAST] != 0 &&
        plan->tuning[D4EST_HIP_TUNE_FLUX_FAST] != 1 && plan->tuning[D4EST_HIP_TUNE_GHOST_ALIAS] <= 0 && !std::getenv("D4EST_HIP_NO_FAMILY_SPLIT")))
    return;
  std::vector<int> small_e, big_e;
  for (int e = 0; e < ne; ++e) (element_is_small(plan, z, e) ? small_e : big_e).push_back(e);
  if (!big_e.empty() && 2 * small_e.size() >= (size_t)ne) {
    fh.family_split = true;
    fh.fam_small = fh.upload_list(small_e);
    fh.fam_big = fh.upload_list(big_e);
  }
}

// ---- the hybrid operator (d4est_hip_direct.hip): on mixed-degree / locally refined plans the CLEAN elements -- deg_quad = deg with a
// one-kernel instance, all six sides conforming against a local element of the same degree or the boundary -- take the trace-free
// whole-operator kernels of their degree bucket
struct HybridGate {
  bool on = false;
  // ghost-aware form (tuning value 2 on a plan with ghost sides; D4EST_HIP_HYBRID_NO_GHOST=1 switches it off): a conforming side against a
  // ghost element of the same degree does not make a (one-wavefront, N <= 8) element dirty -- the kernel reads the (+) block from the ghost
  // trace buffer (kind 4 -> kind 2 + DIRECT_KCF_GHOST).  The sender's trace kernel wrote that block at the mortar nodes in the sender's own
  // face order; the READING kernel re-orients it with the side's side_reorder code, as the two-phase flux kernel and the uniform direct
  // kernel do with a ghost block.  Race freedom by
  // construction: such an element is in the ring, so the trace kernel -- never a clean kernel -- writes the block the exchange packs, and
  // its own launch is queued on the plan's stream only after exchange phase 1 has returned there (apply_operator).  A ghost neighbour of
  // another degree, a hanging face cut by the shard boundary and every ghost side of a p >= 8 element leave the element dirty.
  bool ghost_aware = false;
  // hanging-aware form (hp split active): a hanging side does not make an element dirty -- the record kernels serve it (kind 3) or,
  // a small side the split handed to the conforming kernels, the direct kernel reads the big element's sub-mortar block from the trace
  // array and exports its own (kind 2); D4EST_HIP_HYBRID_NO_HANGING=1 keeps every element with a hanging side dirty
  // (plans with degrees above 7 under the generalised hp split: the elements of the one-wavefront buckets, N <= 8, only -- the multi-wave
  // whole-operator kernel has no hanging-aware instance)
  bool hang_aware = false;
  // mixed-aware form: a conforming side against a local element of LOWER degree does not make the (one-wavefront) element dirty either --
  // the mortar is the element's own (d4est's rule: the larger degree), its operators are the same-degree ones, and the (+) block, which the
  // lower-degree neighbour's trace kernel interpolates up to that mortar, is read from the trace array like a ghost block (kind 2; the
  // neighbour itself stays dirty: ITS side sees a mortar above its own degree).  D4EST_HIP_HYBRID_NO_MIXED=1 switches it off
  bool mixed_aware = false;
};

static HybridGate hybrid_gate(const d4est_hip_plan* plan, const FaceHost& fh, const SideSizes& z) {
  HybridGate g;
  g.ghost_aware = plan->n_ghost > 0 && plan->tuning[D4EST_HIP_TUNE_HYBRID] == 2 && !std::getenv("D4EST_HIP_HYBRID_NO_GHOST");
  // one rank without the direct tables -- or, tuning value 2, a shard: the ghost-aware form (a uniform-degree shard, which has the direct tables too, then takes this path instead)
  const bool plan_kind_fits = g.ghost_aware || (!plan->direct && plan->n_ghost == 0);
  // the tuning keys leave the hybrid operator, the fast two-phase kernels and the exchanged ghost traces on
  const bool keys_allow = plan->tuning[D4EST_HIP_TUNE_HYBRID] != 0 && plan->tuning[D4EST_HIP_TUNE_GHOST_ALIAS] <= 0 &&
                          plan->tuning[D4EST_HIP_TUNE_FLUX_FAST] != 0 && plan->tuning[D4EST_HIP_TUNE_FLUX_FAST] != 1;
  // plans whose two-phase kernels have list forms
  const bool lists_exist = z.hp ? (fh.hp_split || (fh.hp_max_N <= 16 && fh.hp_max_NQ <= 16)) : (z.fast || (fh.max_N <= 16 && fh.max_NQ <= 16));
  g.on = plan_kind_fits && plan->n_elements > 0 && keys_allow && lists_exist;
  g.hang_aware = z.hp && fh.hp_split && !std::getenv("D4EST_HIP_HYBRID_NO_HANGING") && plan->local_trace_doubles < (1LL << 31);
  g.mixed_aware = (!z.hp || fh.hp_split) && !std::getenv("D4EST_HIP_HYBRID_NO_MIXED") && plan->local_trace_doubles < (1LL << 31);
  return g;
}

struct HybridClasses {
  std::vector<char> bucket_ok, clean;     // per bucket: it has a one-kernel instance; per element: clean
  std::vector<int> bucket_of;             // per element: its degree bucket
  std::vector<HybridSideOverride> ov;     // per side, where a form above is on: what a clean element's side is to the direct kernel
  bool any_ov = false, any_hang_ov = false, any_mixed_ov = false;
  int n_clean = 0;
};

static HybridClasses hybrid_classify(const d4est_hip_plan* plan, const HybridGate& g, const SideSizes& z, const std::vector<SideDesc>& sd) {
  const int ne = plan->n_elements;
  const size_t ns = 6 * (size_t)ne;
  const bool hp = z.hp, hang_aware = g.hang_aware, mixed_aware = g.mixed_aware, hy_ghost = g.ghost_aware;
  const std::vector<int>& deg_mq_of = z.deg_mq_of;
  const std::vector<int>& deg_p_of = z.deg_p_of;
  HybridClasses c;
  c.bucket_ok.assign(plan->buckets.size(), 0);
  c.clean.assign(ne, 0);
  c.bucket_of.assign(ne, -1);
  std::vector<char>& bucket_ok = c.bucket_ok;
  std::vector<int>& bucket_of = c.bucket_of;
  std::vector<HybridSideOverride>& ov = c.ov;
  if (hang_aware || mixed_aware || hy_ghost) ov.assign(ns, HybridSideOverride{-1, 0, 0, 0});
  for (size_t b = 0; b < plan->buckets.size(); ++b) {
    const Bucket& bk = plan->buckets[b];
    bucket_ok[b] = bk.N == bk.NQ && bk.d_EBf && hybrid_pair_built(bk.N, bk.NQ);
    for (int i = 0; i < bk.n_elem; ++i) bucket_of[plan->elem_ids[bk.elem_offset + i]] = (int)b;
  }
  for (int e = 0; e < ne; ++e) {
    if (bucket_of[e] < 0 || !bucket_ok[bucket_of[e]]) continue;
    bool ok = true;
    for (int f = 0; f < 6 && ok; ++f) {
      const size_t s_ = 6 * (size_t)e + f;
      if (hp && plan->side_hang[s_] != 0) {
        if (!hang_aware || plan->buckets[bucket_of[e]].N > 8) { ok = false; break; }
        // (a hanging face cut by the shard boundary: the two-phase kernels)
        bool cut = plan->side_nbr[s_] <= -2;
        if (plan->side_hang[s_] == 1 && !plan->side_nbr4.empty())
          for (int k = 0; k < 4; ++k) cut = cut || plan->side_nbr4[4 * s_ + k] <= -2;
        if (cut) { ok = false; break; }
        const SideDesc& d = sd[s_];
        if (d.kind == 3) { ov[s_] = HybridSideOverride{3, 0, 0, 0}; continue; }   // (the element is on the record kernels' list)
        if (d.kind == 1 && plan->side_hang[s_] == 2 && d.NQ == plan->buckets[bucket_of[e]].NQ && deg_p_of[s_] == plan->deg[e]) {
          ov[s_] = HybridSideOverride{2, d.nbr_qoff, (int)d.qoff, d.geom};
          continue;
        }
        ok = false;
        break;
      }
      const int nbr = plan->side_nbr[s_];
      if (nbr == -1) continue;                                   // domain boundary
      if (nbr < 0) {                                             // ghost: the ghost-aware form, or dirty
        const int gh = -(nbr + 2);
        const Bucket& bk = plan->buckets[bucket_of[e]];
        if (hy_ghost && bk.N <= 8 && gh < plan->n_ghost && plan->ghost_deg[gh] == plan->deg[e] && plan->ghost_deg_quad[gh] == plan->deg_quad[e] &&
            deg_mq_of[s_] == plan->deg_quad[e] && sd[s_].kind == 2 && sd[s_].NQ == bk.NQ && plan->ghost_trace_offset[s_] >= 0 &&
            plan->ghost_trace_offset[s_] + 4LL * bk.NQ * bk.NQ <= plan->ghost_trace_doubles) {
          ov[s_] = HybridSideOverride{4, plan->ghost_trace_offset[s_], -1, plan->side_mortar_stride[s_]};
          continue;
        }
        ok = false;
        break;
      }
      const size_t sp = 6 * (size_t)nbr + plan->side_nbr_face[s_];
      if (mixed_aware && plan->buckets[bucket_of[e]].N <= 8 && plan->deg[nbr] < plan->deg[e] && plan->deg_quad[nbr] <= plan->deg_quad[e] &&
          deg_mq_of[s_] == plan->deg_quad[e] && !(hp && plan->side_hang[sp] != 0) && sd[s_].kind == 1 && sd[s_].NQ == plan->buckets[bucket_of[e]].NQ) {
        // (no export: the neighbour is dirty, so this element is in the ring and the trace kernel writes its block -- an export from the
        // clean kernel could race with the dirty flux kernel reading that block on another stream)
        ov[s_] = HybridSideOverride{2, sd[s_].nbr_qoff, -1, sd[s_].geom};
        continue;
      }
      ok = plan->deg[nbr] == plan->deg[e] && plan->deg_quad[nbr] == plan->deg_quad[e] && deg_mq_of[s_] == plan->deg_quad[e] &&
           !(hp && plan->side_hang[sp] != 0);
    }
    c.clean[e] = ok;
    c.n_clean += ok;
    if (ok && (hang_aware || mixed_aware || hy_ghost))
      for (int f = 0; f < 6; ++f) {
        const size_t s_ = 6 * (size_t)e + f;
        if (ov[s_].kind < 0) continue;
        c.any_ov = true;
        if (ov[s_].kind == 4) continue;   // (ghost-aware: not part of the form's label)
        if (hp && plan->side_hang[s_] != 0) c.any_hang_ov = true;
        else c.any_mixed_ov = true;
      }
  }
  return c;
}

// the bucket rule (d4est_hip_hybrid_buckets.h) on the classification: the elements of the buckets it does not keep go back to the two-phase lists
static HybridBucketChoice hybrid_apply_bucket_rule(const d4est_hip_plan* plan, HybridClasses& c) {
  const int ne = plan->n_elements;
  std::vector<int> cnt(plan->buckets.size(), 0);
  for (int e = 0; e < ne; ++e)
    if (c.clean[e]) ++cnt[c.bucket_of[e]];
  if (std::getenv("D4EST_HIP_DEBUG_HYBRID")) {
    std::fprintf(stderr, "[d4est_hip] hybrid classification: %d of %d elements clean, per bucket:", c.n_clean, ne);
    for (size_t b = 0; b < cnt.size(); ++b) std::fprintf(stderr, " N=%d:%d/%d", plan->buckets[b].N, cnt[b], plan->buckets[b].n_elem);
    std::fprintf(stderr, "\n");
  }
  const bool one_only = std::getenv("D4EST_HIP_HYBRID_ONE_BUCKET_ONLY") != nullptr;
  const HybridBucketChoice choice = hybrid_choose_buckets(cnt, ne, plan->tuning[D4EST_HIP_TUNE_HYBRID], one_only);
  if (choice.set_up)
    for (int e = 0; e < ne; ++e)
      if (c.clean[e] && !choice.keep[c.bucket_of[e]]) c.clean[e] = 0;
  return choice;
}

static void hybrid_operator(d4est_hip_plan* plan, FaceHost& fh, const SideSizes& z, const std::vector<SideDesc>& sd, FaceOpTable& table) {
  const HybridGate gate = hybrid_gate(plan, fh, z);
  if (!gate.on) return;
  HybridClasses c = hybrid_classify(plan, gate, z, sd);
  if (!hybrid_apply_bucket_rule(plan, c).set_up) return;
  const size_t nb = plan->buckets.size();
  std::vector<int> oC(nb, -1), oCD(nb, -1), oE(nb, -1);
  for (size_t b = 0; b < nb; ++b) {
    if (!c.bucket_ok[b]) continue;
    const int d = plan->buckets[b].deg, dq = plan->buckets[b].deg_quad;
    oC[b] = table.C(d, dq); oCD[b] = table.CD(d, dq); oE[b] = table.E(d, d, dq);
  }
  std::vector<const double*> pC(nb, nullptr), pCD(nb, nullptr), pE(nb, nullptr);
  for (size_t b = 0; b < nb; ++b)
    if (oC[b] >= 0) { pC[b] = table.ops.data() + oC[b]; pCD[b] = table.ops.data() + oCD[b]; pE[b] = table.ops.data() + oE[b]; }
  // (the flags describe the classification before the dominant-bucket rule demoted anybody: a label, not a contract)
  hybrid_setup(plan, c.clean, pC, pCD, pE, c.any_ov ? &c.ov : nullptr,
               c.any_hang_ov ? (c.any_mixed_ov ? "hanging-aware, mixed-aware" : "hanging-aware") : "mixed-aware");
  const int *dd, *dr;
  int nd_, nr_;
  hybrid_lists(plan, &dd, &nd_, &dr, &nr_);
  fh.hy_dirty_any = dd;
  if (!fh.family_split) return;
  // the ring and dirty lists of a family-split plan, split the same way
  const std::vector<int>*hd, *hr;
  hybrid_host_lists(plan, &hd, &hr);
  std::vector<int> rs, rb, ds, db;
  for (int e : *hr) (element_is_small(plan, z, e) ? rs : rb).push_back(e);
  for (int e : *hd) (element_is_small(plan, z, e) ? ds : db).push_back(e);
  fh.ring_small = fh.upload_list(rs);
  fh.ring_big = fh.upload_list(rb);
  fh.dirty_small = fh.upload_list(ds);
  fh.dirty_big = fh.upload_list(db);
  fh.hy_dirty = dd; fh.hy_ring = dr;
}

static void alloc_face_buffers(d4est_hip_plan* plan) {
  const size_t tm = std::max<size_t>((size_t)plan->total_mortar_nodes, 1);
  HIP_CHECK(hipMalloc(&plan->d_trace, std::max<size_t>((size_t)plan->local_trace_doubles, 1) * sizeof(double)));
  HIP_CHECK(hipMalloc(&plan->d_bndry, tm * sizeof(double)));  // Dirichlet data at the mortar quadrature nodes, by geom stride
  HIP_CHECK(hipMemset(plan->d_bndry, 0, tm * sizeof(double)));
  HIP_CHECK(hipMalloc(&plan->d_face_geom, 7 * tm * sizeof(double)));
}

// Runs ONCE per plan (d4est_hip_plan_set_faces refuses a second call; a new mesh gets a new plan): every stage starts from an empty
// FaceHost and nothing here frees or resets what an earlier run might have left.
void faces_setup(d4est_hip_plan* plan) {
  FaceHost& fh = face_host(plan);
  if (plan->has_faces || !fh.owned.empty()) D4EST_HIP_ABORT("plan_set_faces: the face set-up of this plan has already run (build a new plan per mesh)");
  FaceOpTable table(plan->quad_type);   // face_ops
  const SideSizes sizes = side_sizes(plan);
  Descriptors desc = build_descriptors(plan, fh, sizes, table);
  uniform_plan_and_direct_tables(plan, fh, sizes, desc, table);
  upload_descriptors(plan, fh, desc, table);
  if (sizes.hp) faces_setup_hp(plan, fh);
  hp_split(plan, fh, sizes, desc.sd);
  family_split(plan, fh, sizes);
  hybrid_operator(plan, fh, sizes, desc.sd, table);
  alloc_face_buffers(plan);
  plan->has_faces = true;
}

void faces_estimator_mortars(d4est_hip_plan* plan, std::vector<EstMortar>& out, std::vector<int>& elem_first, const double** face_ops,
                             const double** hp_ops) {
  FaceHost& fh = face_host(plan);
  const int ne = plan->n_elements;
  out.clear();
  elem_first.assign(ne + 1, 0);
  *face_ops = plan->d_face_ops;
  *hp_ops = fh.d_hp_ops;
  if (fh.hp) {
    // the records as faces_setup_hp built them (before the hp split re-labelled the small sides it hands to the conforming kernels)
    for (int e = 0; e < ne; ++e) {
      elem_first[e] = (int)out.size();
      for (int r = plan->side_first_rec[6 * (size_t)e]; r < plan->side_first_rec[6 * (size_t)e + 6]; ++r) {
        const HpMortar& m = fh.rec_host[r];
        const HpGeomSrc& g = fh.gsrc_host[r];
        const size_t s = 6 * (size_t)e + m.face;
        EstMortar x{};
        x.elem = e; x.kind = m.kind; x.code = m.code; x.NQ = m.NQ; x.gidx = m.gidx;
        x.S = g.S; x.off = g.off; x.off_p = g.off_p; x.Ttot = g.Ttot; x.deg_m = g.deg_m; x.deg_p = g.deg_p;
        x.N = m.N; x.offC = m.offCa; x.ops_hp = 1; x.bstride = plan->side_bndry_stride[s]; x.u_shift = m.u_shift;
        x.fm = m.fm; x.fp = m.fp; x.qoff = m.qoff; x.nbr_qoff = m.nbr_qoff;
        out.push_back(x);
      }
    }
  } else {
    for (int e = 0; e < ne; ++e) {
      elem_first[e] = (int)out.size();
      for (int f = 0; f < 6; ++f) {
        const size_t s = 6 * (size_t)e + f;
        const SideDesc& d = fh.sd_host[s];
        EstMortar x{};
        x.elem = e; x.kind = d.kind; x.code = d.code; x.NQ = d.NQ; x.gidx = d.geom;
        x.S = d.geom; x.off = 0; x.off_p = 0; x.Ttot = d.NQ * d.NQ; x.deg_m = fh.side_deg_m[s]; x.deg_p = fh.side_deg_p[s];
        x.N = plan->deg[e] + 1; x.offC = d.offC; x.ops_hp = 0; x.bstride = plan->side_bndry_stride[s]; x.u_shift = 0;
        x.fm = 1.0; x.fp = 1.0; x.qoff = d.qoff; x.nbr_qoff = d.nbr_qoff;
        out.push_back(x);
      }
    }
  }
  elem_first[ne] = (int)out.size();
}

void faces_destroy(d4est_hip_plan* plan) {
  estimator_destroy(plan);
  norms_destroy(plan);
  direct_destroy(plan);
  hybrid_destroy(plan);
  auto it = g_face_host.find(plan);
  if (it != g_face_host.end()) {
    it->second.release();
    g_face_host.erase(it);
  }
  (void)hipFree(plan->d_elem_desc);
  (void)hipFree(plan->d_side_desc); (void)hipFree(plan->d_face_ops);
  (void)hipFree(plan->d_face_geom); (void)hipFree(plan->d_bndry); (void)hipFree(plan->d_trace);
}

}  // namespace d4est_hip
