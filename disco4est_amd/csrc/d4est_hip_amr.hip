// One hp-AMR step's bookkeeping on the device: estimator statistics, smooth_pred marking, p-balance, and the transfer of a field from
// the old grid to the refined and balanced grid in ONE kernel.
//
// Replaces, of the reference's adaptive loop (d4est_amr_step, src/hpAMR/d4est_amr.c:852-1035):
//   d4est_estimator_stats_compute_aux, single-rank branch          (src/Estimators/d4est_estimator_stats.c:219-251)
//   ... its mpisize > 1 branch with the global percentile           (:252-274, :350-425), a radix select over ranks, no distributed sort
//   d4est_amr_load_balance: the transfer to a new partition         (src/hpAMR/d4est_amr.c:773-864; p4est_partition_ext stays on the host)
//   d4est_amr_smooth_pred_pre_refine_callback (fill, no checkpoint) (src/hpAMR/d4est_amr_smooth_pred.c:23-71)
//   d4est_amr_smooth_pred_mark_elements                             (:215-268)
//   the p-balance update of the log and of the predictor            (d4est_amr.c:973-981, d4est_amr_smooth_pred.c:132-168)
//   d4est_amr_smooth_pred_compute_post_h_balance_predictor          (d4est_amr_smooth_pred.c:73-129)
//   d4est_amr_interpolate_field                                     (d4est_amr.c:397-482)
// p4est_refine_ext, p4est_balance_ext and the p-balance face walk stay on the host; they exchange the refinement log, the balance log and
// the p_balance array (ints, one per element) with this object.
//
// The field transfer: the reference interpolates old -> auxiliary (refined, unbalanced) grid -> new grid, two loops through an auxiliary
// vector.  Here every FINAL element's 1-D operator per direction is the product of the two stages' tables
//   stage 1: identity | p_prolong(deg -> deg') | hp_prolong(deg -> deg')[bit]      stage 2: identity | hp_prolong(deg' -> deg')[bit]
// formed in fp64 when the balance log arrives, so one three-pass contraction takes the old element's block to the new element's: old +
// new bytes move instead of old + 2 aux + new.  One workgroup per AUXILIARY element: its source block is read once (a thread keeps its
// x-line in registers) and goes to the one or eight final elements the auxiliary element became.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "d4est_hip_internal.h"
#include "d4est_hip_tables.h"
#include "d4est_hip_transfer.h"
#include "d4est_hip_wave.h"

using d4est_hip::Tables1D;

namespace d4est_hip {

// compile-time instances of the fused transfer: source sizes NH = 2 .. 8 (degrees 1 .. 7), size differences 0, 1 and <= 3 (the instance
// classes of the multigrid transfer kernels); everything else runs the runtime-size kernel
constexpr int kAmrFastMaxNH = 8;
constexpr int kAmrFastMaxD = 3;
// largest degree: two (deg + 1)^3 fields in the 160 KB LDS (the runtime-size kernel), the limit d4est_hip_transfer_create states
static int amr_degree_limit() {
  int d = Tables1D::kMaxDeg;
  while ((size_t)2 * (d + 1) * (d + 1) * (d + 1) * sizeof(double) > 160 * 1024) --d;
  return d;
}

struct AmrLevel {
  int n = 0;
  long long nodes = 0;
  std::vector<int> deg;
  int* d_deg = nullptr;
  int* d_log = nullptr;
  int* d_pbal = nullptr;       // the host's p_balance array, uploaded per call
  double* d_pred = nullptr;
  double* d_sorted = nullptr;
  void* d_tmp = nullptr;       // rocPRIM radix sort temporary storage for n keys
  size_t tmp_bytes = 0;
};

}  // namespace d4est_hip

struct d4est_hip_amr {
  d4est_hip::AmrLevel cur, next;   // next: allocated by set_balance, made current by advance
  int max_degree = 0;
  double gamma_h = 1.0, gamma_p = 1.0;   // of the last mark call
  bool two_stage = false;
  hipStream_t stream = nullptr;
  std::vector<int> h_log;
  bool log_valid = false;      // h_log mirrors d_log (clipped)
  // ---- the state of one set_balance
  bool balanced = false;
  int n_aux = 0;
  long long aux_nodes = 0;
  int max_n = 1;
  int* d_aux_rec = nullptr;         // per auxiliary element: {NH, Nh, n_out, first output}
  long long* d_aux_src = nullptr;   // per auxiliary element: offset of its source block in the old field
  long long* d_out_off = nullptr;   // per final element: offset in the new field
  int* d_out_ops = nullptr;         // per final element: offsets of its x, y, z operators in d_opsT
  double* d_opsT = nullptr;         // composite operators, TRANSPOSED (NH x Nh row-major)
  int* d_lists = nullptr;
  struct List { int NH, dmax, first, n, n_out; };   // NH = 0: the runtime-size kernel
  std::vector<List> lists;
  int* d_adv_src = nullptr;         // per final element: the old element it came from
  int* d_adv_bal = nullptr;         // per final element: |balance_log| if it is a child of a balance split, else -1
  // D4EST_HIP_AMR_TWO_STAGE: the same transfer as two prolongations through an auxiliary vector
  d4est_hip_transfer_t* t1 = nullptr;
  d4est_hip_transfer_t* t2 = nullptr;
  double* d_aux_field = nullptr;
  // ---- several ranks (d4est_hip_par_amr_set_comm); world = 1 calls no hook
  int rank = 0, world = 1;
  d4est_hip_allreduce_fn allreduce = nullptr;
  d4est_hip_amr_sendrecv_fn sendrecv = nullptr;
  void* comm_ctx = nullptr;
  // the radix select of stats_global: the (prefix, remaining rank) state, the integer bins and the doubles the allreduce hook sums
  unsigned long long* d_sel = nullptr;   // [0], [1] key prefix of the percentile / the maximum; [2], [3] remaining rank; [4], [5] target valid
  unsigned int* d_bins = nullptr;        // two histograms of kSelBins
  double* d_red = nullptr;               // the bins as doubles, then the local sum and the local n
  // ---- the state of one repartition, for repartition_field
  struct Repart {
    bool valid = false, exchange = false;
    std::vector<int> peers;
    std::vector<long long> send_first, recv_first;   // per peer, in nodes: the send buffer is the old field without the part that stays
    long long old_nodes = 0, new_nodes = 0, n_send = 0, n_recv = 0;
    long long self_old = 0, self_new = 0, self_len = 0;   // the part that stays: offsets in the old and the new field, length
    double* d_send = nullptr;
    double* d_recv = nullptr;
  } rp;
};

namespace d4est_hip {

// ---- statistics -----------------------------------------------------------------------------------------------------------------------
// one workgroup: thread t sums entries t, t + 1024, ... in that order, the 1024 partial sums meet in a fixed binary tree
__global__ __launch_bounds__(1024) void amr_stats_kernel(const double* __restrict__ eta2, const double* __restrict__ sorted, int n, int idx,
                                                         double* __restrict__ stats) {
  __shared__ double s[1024];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < n; i += 1024) acc = __dadd_rn(acc, eta2[i]);
  s[t] = acc;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (t < w) s[t] = __dadd_rn(s[t], s[t + w]);
    __syncthreads();
  }
  if (t == 0) {
    if (n > 0) {
      stats[0] = s[0];
      stats[1] = __ddiv_rn(s[0], (double)n);
      stats[2] = sorted[n - 1];
      stats[3] = (idx >= 0 && idx < n) ? sorted[idx] : -1.0;
    } else {   // d4est_estimator_stats.c:234-238
      stats[0] = 0.0;
      stats[1] = stats[2] = stats[3] = -1.0;
    }
  }
}

// ---- statistics over ranks: radix select ------------------------------------------------------------------------------------------------
// The k-th smallest of all ranks' eta2 without a distributed sort.  A double maps to a 64-bit key of the same order (negatives: all bits
// flipped; non-negatives: sign bit set); kSelPasses digit passes from the most significant digit down.  Per pass: a histogram of the digit
// over the local keys that carry the prefix chosen so far (LDS integer atomics per workgroup, integer atomics into the global bins), the
// bins as doubles (exact below 2^53) through the allreduce hook, and a one-wavefront pick that chooses the digit and updates (prefix,
// remaining rank) on the device.  Two targets ride the same passes: rank G - k (the percentile) and rank G - 1 (the maximum).
constexpr int kSelBits = 8;
constexpr int kSelBins = 1 << kSelBits;
constexpr int kSelPasses = 64 / kSelBits;
constexpr int kSelRed = 2 * kSelBins + 2;   // doubles of the first round: two histograms, the local sum, the local n
constexpr unsigned long long kSignBit = 0x8000000000000000ull;

__device__ __forceinline__ unsigned long long amr_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b & kSignBit) ? ~b : (b | kSignBit);
}
__device__ __forceinline__ double amr_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k & kSignBit) ? (k ^ kSignBit) : ~k));
}

// the fixed-order local sum of amr_stats_kernel (thread t: entries t, t + 1024, ...; then a binary tree) and the local n
__global__ __launch_bounds__(1024) void amr_local_sum_kernel(const double* __restrict__ eta2, int n, double* __restrict__ red) {
  __shared__ double s[1024];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < n; i += 1024) acc = __dadd_rn(acc, eta2[i]);
  s[t] = acc;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (t < w) s[t] = __dadd_rn(s[t], s[t + w]);
    __syncthreads();
  }
  if (t == 0) {
    red[2 * kSelBins] = s[0];
    red[2 * kSelBins + 1] = (double)n;
  }
}

// grid-stride over n, kSelBins threads: bins[d] += keys with the percentile target's prefix and digit d, bins[kSelBins + d] likewise for
// the maximum's prefix.  Pass 0 has no prefix: sel is not read through the mask.
__global__ __launch_bounds__(kSelBins) void amr_sel_hist_kernel(const double* __restrict__ eta2, int n, int pass,
                                                                const unsigned long long* __restrict__ sel, unsigned int* __restrict__ bins) {
  __shared__ unsigned int h[2 * kSelBins];
  const int t = threadIdx.x;
  h[t] = 0u;
  h[kSelBins + t] = 0u;
  __syncthreads();
  const int shift = 64 - kSelBits * (pass + 1);
  const unsigned long long mask = pass == 0 ? 0ull : ~0ull << (shift + kSelBits);
  const unsigned long long p0 = sel[0], p1 = sel[1];
  for (long long i = (long long)blockIdx.x * kSelBins + t; i < n; i += (long long)gridDim.x * kSelBins) {
    const unsigned long long key = amr_key(eta2[i]);
    const int d = (int)((key >> shift) & (kSelBins - 1));
    if (((key ^ p0) & mask) == 0ull) atomicAdd(&h[d], 1u);
    if (((key ^ p1) & mask) == 0ull) atomicAdd(&h[kSelBins + d], 1u);
  }
  __syncthreads();
  if (h[t]) atomicAdd(&bins[t], h[t]);
  if (h[kSelBins + t]) atomicAdd(&bins[kSelBins + t], h[kSelBins + t]);
}

// the bins as doubles for the allreduce hook; the integer bins are zero again for the next pass
__global__ __launch_bounds__(2 * kSelBins) void amr_sel_convert_kernel(unsigned int* __restrict__ bins, double* __restrict__ red) {
  const int t = threadIdx.x;
  red[t] = (double)bins[t];
  bins[t] = 0u;
}

// One wavefront.  Pass 0 sets the targets from the global n and total (d4est_estimator_stats.c:379: k = (int)((double)(G * percentile) /
// 100.0), the percentile is entry G - k of the ascending order; k = 0 has no entry, the reference aborts at :396) and writes total and mean;
// every pass scans the summed bins (lane l: bins 4 l .. 4 l + 3, an exclusive prefix over the lanes through LDS), the lane that holds the
// target's rank appends the digit to the prefix; the last pass turns the keys back into doubles.
__global__ __launch_bounds__(64) void amr_sel_pick_kernel(const double* __restrict__ red, int pass, int percentile,
                                                          unsigned long long* __restrict__ sel, double* __restrict__ stats) {
  __shared__ unsigned long long s[64];
  const int t = threadIdx.x;
  constexpr int PER = kSelBins / 64;
  const int shift = 64 - kSelBits * (pass + 1);
  unsigned long long prefix[2], rank[2], valid[2];
  if (pass == 0) {
    const long long G = (long long)red[2 * kSelBins + 1];
    const long long k = (long long)((double)(G * (long long)percentile) / 100.0);
    prefix[0] = prefix[1] = 0ull;
    rank[0] = (unsigned long long)(G - k);
    rank[1] = (unsigned long long)(G - 1);
    valid[0] = (G > 0 && k > 0) ? 1ull : 0ull;
    valid[1] = G > 0 ? 1ull : 0ull;
    if (t == 0) {
      stats[0] = G > 0 ? red[2 * kSelBins] : 0.0;   // d4est_estimator_stats.c:234-238 where there is no element at all
      stats[1] = G > 0 ? __ddiv_rn(red[2 * kSelBins], (double)G) : -1.0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      prefix[j] = sel[j];
      rank[j] = sel[2 + j];
      valid[j] = sel[4 + j];
    }
  }
  const bool last = pass == kSelPasses - 1;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    unsigned long long c[PER], own = 0ull;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      c[q] = (unsigned long long)red[j * kSelBins + t * PER + q];
      own += c[q];
    }
    s[t] = own;
    __syncthreads();   // (also: every lane has read sel before a lane writes it)
    unsigned long long before = 0ull;
    for (int l = 0; l < t; ++l) before += s[l];
    __syncthreads();
    double* out = stats + (j == 0 ? 3 : 2);
    if (!valid[j]) {
      if (t == 0) {
        sel[j] = 0ull; sel[2 + j] = 0ull; sel[4 + j] = 0ull;
        if (last) *out = -1.0;
      }
    } else if (rank[j] >= before && rank[j] < before + own) {   // exactly one lane: the counts of the prefix sum up to more than the rank
      unsigned long long r = rank[j] - before;
      int q = 0;
#pragma unroll
      for (int u = 0; u < PER - 1; ++u)
        if (q == u && r >= c[u]) { r -= c[u]; q = u + 1; }
      const unsigned long long np = prefix[j] | ((unsigned long long)(t * PER + q) << shift);
      sel[j] = np; sel[2 + j] = r; sel[4 + j] = 1ull;
      if (last) *out = amr_unkey(np);
    }
  }
}

// ---- the load-balance transfer ------------------------------------------------------------------------------------------------------------
// A rank's elements all go somewhere: what is sent, in peer order, is the old array WITHOUT the part that stays (a gap of gap_len entries
// at gap_at), and what arrives is the new array without that part.  Degrees travel as doubles next to the predictor.
__device__ __forceinline__ long long amr_gap(long long i, long long gap_at, long long gap_len) { return i < gap_at ? i : i + gap_len; }

__global__ __launch_bounds__(256) void amr_state_pack_kernel(const int* __restrict__ deg, const double* __restrict__ pred, long long n_send,
                                                             long long gap_at, long long gap_len, double* __restrict__ buf) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_send; i += (long long)gridDim.x * 256) {
    const long long e = amr_gap(i, gap_at, gap_len);
    buf[2 * i] = (double)deg[e];
    buf[2 * i + 1] = pred[e];
  }
}

__global__ __launch_bounds__(256) void amr_state_unpack_kernel(const double* __restrict__ buf, long long n_recv, long long gap_at,
                                                               long long gap_len, int* __restrict__ deg, double* __restrict__ pred) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_recv; i += (long long)gridDim.x * 256) {
    const long long e = amr_gap(i, gap_at, gap_len);
    deg[e] = (int)buf[2 * i];
    pred[e] = buf[2 * i + 1];
  }
}

// unpack = 0: dst[i] = src[gap(i)] (the send buffer from the old field); 1: dst[gap(i)] = src[i] (the new field from the receive buffer)
__global__ __launch_bounds__(256) void amr_gap_copy_kernel(const double* __restrict__ src, double* __restrict__ dst, long long n,
                                                           long long gap_at, long long gap_len, int unpack) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long j = amr_gap(i, gap_at, gap_len);
    if (unpack) dst[j] = src[i];
    else dst[i] = src[j];
  }
}

// ---- marking --------------------------------------------------------------------------------------------------------------------------
// every product is a rounded multiplication, left to right (no contraction into a fused multiply-add): the predictor is the number a
// plain C evaluation of d4est_amr_smooth_pred.c:253-267 gives
__global__ __launch_bounds__(256) void amr_mark_kernel(const double* __restrict__ eta2, const double* __restrict__ threshold, double factor,
                                                       double gamma_h, double gamma_p, double gamma_n, const int* __restrict__ deg,
                                                       int max_degree, double* __restrict__ pred, int* __restrict__ log, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const double eta = eta2[e], p = pred[e];
  const int d = deg[e];
  if (eta >= __dmul_rn(factor, threshold[0])) {
    if (eta <= p && d < max_degree) {
      log[e] = min(d + 1, max_degree);
      pred[e] = __dmul_rn(gamma_p, eta);
    } else {
      log[e] = -d;
      pred[e] = __dmul_rn(__dmul_rn(__dmul_rn(gamma_h, eta), ldexp(1.0, -2 * d)), 0.125);   // .5^(2 deg) is exact
    }
  } else {
    log[e] = d;
    pred[e] = __dmul_rn(gamma_n, p);
  }
}

__global__ __launch_bounds__(256) void amr_p_balance_kernel(const int* __restrict__ pbal, int if_diff, const int* __restrict__ deg, int max_degree,
                                                            double gamma_p, double* __restrict__ pred, int* __restrict__ log, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (pbal[e] >= if_diff && deg[e] < max_degree - 1) {
    const int l = log[e];
    log[e] = l < 0 ? l - 1 : l + 1;
    pred[e] = __dmul_rn(gamma_p, pred[e]);
  }
}

__global__ __launch_bounds__(256) void amr_fill_kernel(double* __restrict__ x, double v, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) x[e] = v;
}

// d4est_amr_smooth_pred.c:88-126: children of a refined element inherit; children of a balance split are scaled (left to right)
__global__ __launch_bounds__(256) void amr_advance_kernel(const double* __restrict__ pred_old, const int* __restrict__ src, const int* __restrict__ bal,
                                                          double gamma_h, double* __restrict__ pred_new, int n_new) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_new) return;
  const double aux = pred_old[src[j]];
  const int h = bal[j];
  pred_new[j] = h < 0 ? aux : __dmul_rn(__dmul_rn(__dmul_rn(0.125, gamma_h), ldexp(1.0, -2 * h)), aux);
}

// ---- the fused field transfer ---------------------------------------------------------------------------------------------------------
template <int NH, int DMAX>
struct AmrCfg {
  static constexpr int NHM = NH + DMAX;
  static constexpr int THREADS = ((NHM * NHM + 63) / 64) * 64;
  static constexpr int LDS = NH * NH * (NHM | 1) + NH * NHM * NHM;   // B [NH][NH][Nh | 1], C [NH][Nh][Nh]
};

// Pass order x, y, z as in prolong_body (d4est_hip_transfer.hip): a thread owns a line along the contracted direction in registers, the
// operator rows are wave-uniform scalar loads (contract_n).  The x-line comes straight from memory ONCE and serves every output; the y-
// and z-lines are read with lds_ld (never paired into ds_read2_b64, d4est_hip_wave.h); the z-pass stores coalesced over the (x, y) plane.
template <int NH, int Nh>
__device__ __forceinline__ void amr_body(const double* __restrict__ src_e, double* __restrict__ dst, const long long* __restrict__ out_off,
                                         const int* __restrict__ out_ops, int n_out, const double* __restrict__ opsT, double* lds, int t) {
  constexpr int RSB = Nh | 1;
  double* B = lds;
  double* C = B + NH * NH * RSB;
  double x0[NH];
  if (t < NH * NH) {
#pragma unroll
    for (int a = 0; a < NH; ++a) x0[a] = src_e[t * NH + a];
  }
  for (int o = 0; o < n_out; ++o) {
    const double *px = opsT + out_ops[3 * o], *py = opsT + out_ops[3 * o + 1], *pz = opsT + out_ops[3 * o + 2];
    double* dst_e = dst + out_off[o];
    if (t < NH * NH) {                       // thread (b, k): the x-line
      double y[Nh];
      contract_n<NH, Nh>(px, x0, y);
#pragma unroll
      for (int a = 0; a < Nh; ++a) B[t * RSB + a] = y[a];
    }
    __syncthreads();
    if (t < Nh * NH) {                       // thread (aq, k): the y-line
      const int aq = t % Nh, k = t / Nh;
      double x[NH], y[Nh];
#pragma unroll
      for (int b = 0; b < NH; ++b) x[b] = lds_ld(&B[(k * NH + b) * RSB + aq]);
      contract_n<NH, Nh>(py, x, y);
#pragma unroll
      for (int b = 0; b < Nh; ++b) C[(k * Nh + b) * Nh + aq] = y[b];
    }
    __syncthreads();                         // (B is rewritten by the next output's x-pass only after this barrier)
    if (t < Nh * Nh) {                       // thread (aq, bq): the z-line; C is rewritten only after the next output's first barrier
      double x[NH], y[Nh];
#pragma unroll
      for (int k = 0; k < NH; ++k) x[k] = lds_ld(&C[k * Nh * Nh + t]);
      contract_n<NH, Nh>(pz, x, y);
#pragma unroll
      for (int k = 0; k < Nh; ++k) dst_e[k * Nh * Nh + t] = y[k];
    }
  }
}

template <int NH, int DMAX>
__global__ __launch_bounds__((AmrCfg<NH, DMAX>::THREADS)) void amr_fused_kernel(const double* __restrict__ field_old, double* __restrict__ field_new,
                                                                              const int* __restrict__ aux_rec,
                                                                              const long long* __restrict__ aux_src,
                                                                              const long long* __restrict__ out_off,
                                                                              const int* __restrict__ out_ops,
                                                                              const double* __restrict__ opsT, const int* __restrict__ list) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int a = list[blockIdx.x];
  const int* r = aux_rec + 4 * a;
  const int dN = r[1] - NH, n_out = r[2], first = r[3];
  const double* src_e = field_old + aux_src[a];
  const long long* oo = out_off + first;
  const int* op = out_ops + 3 * first;
  const int t = threadIdx.x;
  if (dN == 0) amr_body<NH, NH>(src_e, field_new, oo, op, n_out, opsT, smem, t);
  if constexpr (DMAX >= 1) { if (dN == 1) amr_body<NH, NH + 1>(src_e, field_new, oo, op, n_out, opsT, smem, t); }
  if constexpr (DMAX >= 2) { if (dN == 2) amr_body<NH, NH + 2>(src_e, field_new, oo, op, n_out, opsT, smem, t); }
  if constexpr (DMAX >= 3) { if (dN == 3) amr_body<NH, NH + 3>(src_e, field_new, oo, op, n_out, opsT, smem, t); }
}

// runtime sizes: one workgroup per auxiliary element in a grid-stride loop, the generic three-pass contraction of d4est_hip_transfer.h
// with the transposed composite tables
__global__ __launch_bounds__(256) void amr_generic_kernel(const double* __restrict__ field_old, double* __restrict__ field_new,
                                                          const int* __restrict__ aux_rec, const long long* __restrict__ aux_src,
                                                          const long long* __restrict__ out_off, const int* __restrict__ out_ops,
                                                          const double* __restrict__ opsT, const int* __restrict__ list, int n, int max_n3) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* a = smem;
  double* b = smem + max_n3;
  for (int ii = blockIdx.x; ii < n; ii += gridDim.x) {
    const int ax = list[ii];
    const int* r = aux_rec + 4 * ax;
    const int NH = r[0], Nh = r[1], n_out = r[2], first = r[3];
    const double* src_e = field_old + aux_src[ax];
    for (int o = 0; o < n_out; ++o) {
      const int* op = out_ops + 3 * (first + o);
      double* dst_e = field_new + out_off[first + o];
      for (int i = threadIdx.x; i < NH * NH * NH; i += blockDim.x) a[i] = src_e[i];   // (the contraction overwrites a)
      __syncthreads();
      tensor3<true>(opsT + op[0], opsT + op[1], opsT + op[2], NH, Nh, a, b);
      for (int i = threadIdx.x; i < Nh * Nh * Nh; i += blockDim.x) dst_e[i] = b[i];
      __syncthreads();
    }
  }
}

template <int NH, int DMAX>
static void go_amr(d4est_hip_amr* A, const double* fo, double* fn, const int* list, int n) {
  using C = AmrCfg<NH, DMAX>;
  const size_t lds = (size_t)C::LDS * sizeof(double);
  static_assert(C::LDS * sizeof(double) <= 64 * 1024, "the compile-time instances stay below the default dynamic LDS limit");
  hipLaunchKernelGGL((amr_fused_kernel<NH, DMAX>), dim3(n), dim3(C::THREADS), lds, A->stream, fo, fn, A->d_aux_rec, A->d_aux_src, A->d_out_off,
                     A->d_out_ops, A->d_opsT, list);
}

#define D4EST_HIP_AMR_NH(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

static void launch_amr_fused(d4est_hip_amr* A, const double* fo, double* fn, int NH, int dmax, const int* list, int n) {
#define X(N_)                                              \
  if (NH == N_) {                                          \
    if (dmax == 0) go_amr<N_, 0>(A, fo, fn, list, n);      \
    else if (dmax == 1) go_amr<N_, 1>(A, fo, fn, list, n); \
    else go_amr<N_, 3>(A, fo, fn, list, n);                \
    return;                                                \
  }
  D4EST_HIP_AMR_NH(X)
#undef X
  D4EST_HIP_ABORT("amr_interpolate_field: no compile-time kernel for %d source nodes per direction", NH);
}

// ---- host helpers ---------------------------------------------------------------------------------------------------------------------
template <typename T>
static T* dev_alloc(size_t n) {
  T* d = nullptr;
  HIP_CHECK(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
  return d;
}
template <typename T>
static T* dev_upload(const std::vector<T>& v, size_t pad = 0) {
  T* d = dev_alloc<T>(v.size() + pad);
  if (pad) HIP_CHECK(hipMemset(d, 0, (v.size() + pad) * sizeof(T)));
  if (!v.empty()) HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

static void level_free(AmrLevel& L) {
  (void)hipFree(L.d_deg); (void)hipFree(L.d_log); (void)hipFree(L.d_pbal); (void)hipFree(L.d_pred); (void)hipFree(L.d_sorted); (void)hipFree(L.d_tmp);
  L = AmrLevel();
}

static void level_alloc(AmrLevel& L, const std::vector<int>& deg) {
  level_free(L);
  L.n = (int)deg.size();
  L.deg = deg;
  L.nodes = 0;
  for (int d : deg) L.nodes += (long long)(d + 1) * (d + 1) * (d + 1);
  L.d_deg = dev_upload(deg);
  L.d_log = dev_alloc<int>(L.n);
  L.d_pbal = dev_alloc<int>(L.n);
  L.d_pred = dev_alloc<double>(L.n);
  L.d_sorted = dev_alloc<double>(L.n);
  if (L.n > 0) {
    HIP_CHECK(rocprim::radix_sort_keys(nullptr, L.tmp_bytes, (const double*)nullptr, (double*)nullptr, (size_t)L.n, 0u, 64u, (hipStream_t) nullptr));
    HIP_CHECK(hipMalloc(&L.d_tmp, std::max<size_t>(L.tmp_bytes, 16)));
  }
}

static void balance_free(d4est_hip_amr* A) {
  (void)hipFree(A->d_aux_rec); (void)hipFree(A->d_aux_src); (void)hipFree(A->d_out_off); (void)hipFree(A->d_out_ops); (void)hipFree(A->d_opsT);
  (void)hipFree(A->d_lists); (void)hipFree(A->d_adv_src); (void)hipFree(A->d_adv_bal); (void)hipFree(A->d_aux_field);
  A->d_aux_rec = A->d_out_ops = A->d_lists = A->d_adv_src = A->d_adv_bal = nullptr;
  A->d_aux_src = A->d_out_off = nullptr;
  A->d_opsT = A->d_aux_field = nullptr;
  if (A->t1) d4est_hip_transfer_destroy(A->t1);
  if (A->t2) d4est_hip_transfer_destroy(A->t2);
  A->t1 = A->t2 = nullptr;
  A->lists.clear();
  A->balanced = false;
}

static void repart_free(d4est_hip_amr* A) {
  (void)hipFree(A->rp.d_send); (void)hipFree(A->rp.d_recv);
  A->rp = d4est_hip_amr::Repart();
}

// d4est_amr.c:374-392: a code is -deg' (h-refine into children of degree deg' >= deg) or deg' >= deg
static void check_log(const d4est_hip_amr* A, const int* log, const char* who) {
  const int limit = amr_degree_limit();
  for (int e = 0; e < A->cur.n; ++e) {
    const int l = log[e], d = A->cur.deg[e];
    if (std::abs(l) < d)
      D4EST_HIP_ABORT("%s: element %d of degree %d has code %d: hp amr code should be >= deg or -deg, coarsening is currently not supported in amr",
                      who, e, d, l);
    if (std::abs(l) > limit) D4EST_HIP_ABORT("%s: element %d has code %d, beyond the transfer kernels' degree limit %d", who, e, l, limit);
  }
}

static void clip_log(const d4est_hip_amr* A, std::vector<int>& log) {   // d4est_amr.c:182-184
  for (int& l : log)
    if (l > A->max_degree) l = A->max_degree;
}

static void fetch_log(d4est_hip_amr* A) {
  if (A->log_valid) return;
  A->h_log.resize(A->cur.n);
  if (A->cur.n > 0) HIP_CHECK(hipMemcpyAsync(A->h_log.data(), A->cur.d_log, (size_t)A->cur.n * sizeof(int), hipMemcpyDeviceToHost, A->stream));
  HIP_CHECK(hipStreamSynchronize(A->stream));
  clip_log(A, A->h_log);
  A->log_valid = true;
}

static inline dim3 grid_for(int n) { return dim3((unsigned)((std::max(n, 1) + 255) / 256)); }

}  // namespace d4est_hip

using namespace d4est_hip;

extern "C" {

d4est_hip_amr_t* d4est_hip_amr_create(int n_elements, const int* deg, int max_degree, double initial_pred) {
  if (n_elements < 0 || (n_elements > 0 && !deg)) D4EST_HIP_ABORT("amr_create: bad arguments");
  const int limit = amr_degree_limit();
  if (max_degree < 1 || max_degree > limit)
    D4EST_HIP_ABORT("amr_create: max_degree %d outside 1 .. %d (two (deg + 1)^3 fields must fit the 160 KB LDS)", max_degree, limit);
  for (int e = 0; e < n_elements; ++e)
    if (deg[e] < 1 || deg[e] > limit) D4EST_HIP_ABORT("amr_create: element %d has degree %d outside 1 .. %d", e, deg[e], limit);
  d4est_hip_amr* A = new d4est_hip_amr();
  A->max_degree = max_degree;
  const char* ts = std::getenv("D4EST_HIP_AMR_TWO_STAGE");
  A->two_stage = ts && ts[0] && ts[0] != '0';
  level_alloc(A->cur, std::vector<int>(deg, deg + n_elements));
  A->d_sel = dev_upload(std::vector<unsigned long long>(8, 0ull));
  A->d_bins = dev_upload(std::vector<unsigned int>(2 * kSelBins, 0u));
  A->d_red = dev_upload(std::vector<double>(kSelRed, 0.0));
  if (n_elements > 0) {
    hipLaunchKernelGGL(amr_fill_kernel, grid_for(n_elements), dim3(256), 0, A->stream, A->cur.d_pred, initial_pred, n_elements);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(A->stream));
  }
  return A;
}

void d4est_hip_amr_destroy(d4est_hip_amr_t* A) {
  if (!A) return;
  balance_free(A);
  repart_free(A);
  level_free(A->cur);
  level_free(A->next);
  (void)hipFree(A->d_sel); (void)hipFree(A->d_bins); (void)hipFree(A->d_red);
  delete A;
}

void d4est_hip_amr_set_stream(d4est_hip_amr_t* A, void* hip_stream) {
  if (!A) D4EST_HIP_ABORT("amr_set_stream: NULL amr");
  A->stream = (hipStream_t)hip_stream;
  if (A->t1) d4est_hip_transfer_set_stream(A->t1, hip_stream);
  if (A->t2) d4est_hip_transfer_set_stream(A->t2, hip_stream);
}

int d4est_hip_amr_n_elements(const d4est_hip_amr_t* A) { return A ? A->cur.n : -1; }
long long d4est_hip_amr_local_nodes(const d4est_hip_amr_t* A) { return A ? A->cur.nodes : -1; }

void d4est_hip_amr_stats(d4est_hip_amr_t* A, const double* eta2_dev, int percentile, double* stats_dev) {
  if (!A || !stats_dev) D4EST_HIP_ABORT("amr_stats: NULL argument");
  if (percentile < 0 || percentile > 100) D4EST_HIP_ABORT("amr_stats: percentile %d outside 0 .. 100", percentile);
  const int n = A->cur.n;
  if (n > 0 && !eta2_dev) D4EST_HIP_ABORT("amr_stats: NULL eta2");
  // d4est_estimator_stats.c:249, in the reference's double arithmetic; percentile 0 gives n, one past the end: -1 is written instead
  const int idx = (int)(((double)n) * (1. - ((double)percentile / 100.0)));
  if (n > 0) {
    size_t bytes = A->cur.tmp_bytes;
    HIP_CHECK(rocprim::radix_sort_keys(A->cur.d_tmp, bytes, eta2_dev, A->cur.d_sorted, (size_t)n, 0u, 64u, A->stream));
  }
  hipLaunchKernelGGL(amr_stats_kernel, dim3(1), dim3(1024), 0, A->stream, eta2_dev, A->cur.d_sorted, n, idx, stats_dev);
  HIP_CHECK(hipGetLastError());
}

void d4est_hip_amr_mark_smooth_pred(d4est_hip_amr_t* A, const double* eta2_dev, const double* threshold_dev, double factor, double gamma_h,
                                    double gamma_p, double gamma_n) {
  if (!A) D4EST_HIP_ABORT("amr_mark_smooth_pred: NULL amr");
  A->gamma_h = gamma_h;
  A->gamma_p = gamma_p;
  A->log_valid = false;
  if (A->cur.n == 0) return;
  if (!eta2_dev || !threshold_dev) D4EST_HIP_ABORT("amr_mark_smooth_pred: NULL argument");
  hipLaunchKernelGGL(amr_mark_kernel, grid_for(A->cur.n), dim3(256), 0, A->stream, eta2_dev, threshold_dev, factor, gamma_h, gamma_p, gamma_n,
                     A->cur.d_deg, A->max_degree, A->cur.d_pred, A->cur.d_log, A->cur.n);
  HIP_CHECK(hipGetLastError());
}

void d4est_hip_amr_p_balance(d4est_hip_amr_t* A, const int* p_balance_host, int p_balance_if_diff) {
  if (!A) D4EST_HIP_ABORT("amr_p_balance: NULL amr");
  if (A->cur.n == 0) return;
  if (!p_balance_host) D4EST_HIP_ABORT("amr_p_balance: NULL p_balance");
  HIP_CHECK(hipMemcpyAsync(A->cur.d_pbal, p_balance_host, (size_t)A->cur.n * sizeof(int), hipMemcpyHostToDevice, A->stream));
  HIP_CHECK(hipStreamSynchronize(A->stream));   // the host array is the caller's again
  A->log_valid = false;
  hipLaunchKernelGGL(amr_p_balance_kernel, grid_for(A->cur.n), dim3(256), 0, A->stream, A->cur.d_pbal, p_balance_if_diff, A->cur.d_deg,
                     A->max_degree, A->gamma_p, A->cur.d_pred, A->cur.d_log, A->cur.n);
  HIP_CHECK(hipGetLastError());
}

void d4est_hip_amr_get_refinement_log(d4est_hip_amr_t* A, int* log_host) {
  if (!A || (A->cur.n > 0 && !log_host)) D4EST_HIP_ABORT("amr_get_refinement_log: NULL argument");
  fetch_log(A);
  if (A->cur.n > 0) memcpy(log_host, A->h_log.data(), (size_t)A->cur.n * sizeof(int));
}

void d4est_hip_amr_set_refinement_log(d4est_hip_amr_t* A, const int* log_host) {
  if (!A || (A->cur.n > 0 && !log_host)) D4EST_HIP_ABORT("amr_set_refinement_log: NULL argument");
  check_log(A, log_host, "amr_set_refinement_log");
  A->h_log.assign(log_host, log_host + A->cur.n);
  clip_log(A, A->h_log);
  check_log(A, A->h_log.data(), "amr_set_refinement_log");   // (a code clipped below the element's degree)
  if (A->cur.n > 0) HIP_CHECK(hipMemcpyAsync(A->cur.d_log, A->h_log.data(), (size_t)A->cur.n * sizeof(int), hipMemcpyHostToDevice, A->stream));
  HIP_CHECK(hipStreamSynchronize(A->stream));
  A->log_valid = true;
}

void d4est_hip_amr_get_predictor(d4est_hip_amr_t* A, double* pred_host) {
  if (!A || (A->cur.n > 0 && !pred_host)) D4EST_HIP_ABORT("amr_get_predictor: NULL argument");
  if (A->cur.n > 0) HIP_CHECK(hipMemcpyAsync(pred_host, A->cur.d_pred, (size_t)A->cur.n * sizeof(double), hipMemcpyDeviceToHost, A->stream));
  HIP_CHECK(hipStreamSynchronize(A->stream));
}

void d4est_hip_amr_set_balance(d4est_hip_amr_t* A, int n_aux, const int* balance_log_host) {
  if (!A || (n_aux > 0 && !balance_log_host)) D4EST_HIP_ABORT("amr_set_balance: NULL argument");
  fetch_log(A);
  check_log(A, A->h_log.data(), "amr_set_balance");
  // the auxiliary (refined, unbalanced) grid: d4est_amr.c:412-442
  const int n_old = A->cur.n;
  std::vector<int> aux_deg, aux_old, aux_child;
  for (int e = 0; e < n_old; ++e) {
    const int l = A->h_log[e];
    for (int c = 0; c < (l < 0 ? 8 : 1); ++c) {
      aux_deg.push_back(std::abs(l));
      aux_old.push_back(e);
      aux_child.push_back(l < 0 ? c : -1);
    }
  }
  if (n_aux != (int)aux_deg.size())
    D4EST_HIP_ABORT("amr_set_balance: n_aux = %d, but the refinement log makes %d auxiliary elements (8 per negative entry, 1 otherwise)", n_aux,
                    (int)aux_deg.size());
  for (int i = 0; i < n_aux; ++i)
    if (std::abs(balance_log_host[i]) != aux_deg[i])
      D4EST_HIP_ABORT("amr_set_balance: balance_log[%d] = %d, but auxiliary element %d has degree %d", i, balance_log_host[i], i, aux_deg[i]);
  balance_free(A);
  A->n_aux = n_aux;

  std::vector<long long> old_off(n_old + 1, 0);
  for (int e = 0; e < n_old; ++e) old_off[e + 1] = old_off[e] + (long long)(A->cur.deg[e] + 1) * (A->cur.deg[e] + 1) * (A->cur.deg[e] + 1);

  // composite 1-D operators, transposed: (deg, deg', stage 1: 0 p | 1 + bit hp, stage 2: 0 none | 1 + bit hp) -> offset
  std::vector<double> opsT;
  std::map<std::tuple<int, int, int, int>, int> index;
  auto half = [](const std::vector<double>& P, int h, int rows, int cols) {
    return std::vector<double>(P.begin() + (size_t)h * rows * cols, P.begin() + (size_t)(h + 1) * rows * cols);
  };
  auto get = [&](int d0, int d1, int s1, int s2) {
    const auto key = std::make_tuple(d0, d1, s1, s2);
    auto f = index.find(key);
    if (f != index.end()) return f->second;
    const int n0 = d0 + 1, n1 = d1 + 1;
    std::vector<double> T = s1 == 0 ? Tables1D::p_prolong(d0, d1) : half(Tables1D::hp_prolong(d0, d1), s1 - 1, n1, n0);   // n1 x n0
    if (s2 != 0) T = Tables1D::matmul(half(Tables1D::hp_prolong(d1, d1), s2 - 1, n1, n1), T, n1, n1, n0);
    const std::vector<double> TT = Tables1D::transpose(T, n1, n0);
    const int o = (int)opsT.size();
    opsT.insert(opsT.end(), TT.begin(), TT.end());
    index[key] = o;
    return o;
  };

  std::vector<int> aux_rec, out_ops, new_deg, adv_src, adv_bal;
  std::vector<long long> aux_src, out_off;
  long long no = 0, ao = 0;
  A->max_n = 1;
  for (int i = 0; i < n_aux; ++i) {
    const int e = aux_old[i], d0 = A->cur.deg[e], d1 = aux_deg[i], c1 = aux_child[i];
    const bool split = balance_log_host[i] < 0;   // d4est_amr.c:236-240: eight children of the same degree
    const int n_out = split ? 8 : 1;
    const int rec[4] = {d0 + 1, d1 + 1, n_out, (int)new_deg.size()};
    aux_rec.insert(aux_rec.end(), rec, rec + 4);
    aux_src.push_back(old_off[e]);
    A->max_n = std::max(A->max_n, d1 + 1);
    for (int c2 = 0; c2 < n_out; ++c2) {
      for (int dir = 0; dir < 3; ++dir) {   // child c = (cx, cy, cz) bits, d4est_operators.c:394-404
        const int s1 = c1 < 0 ? 0 : 1 + ((c1 >> dir) & 1), s2 = split ? 1 + ((c2 >> dir) & 1) : 0;
        out_ops.push_back(get(d0, d1, s1, s2));
      }
      out_off.push_back(no);
      no += (long long)(d1 + 1) * (d1 + 1) * (d1 + 1);
      new_deg.push_back(d1);
      adv_src.push_back(e);
      adv_bal.push_back(split ? d1 : -1);
    }
    ao += (long long)(d1 + 1) * (d1 + 1) * (d1 + 1);
  }
  A->aux_nodes = ao;

  // work lists: auxiliary elements by source size for the compile-time kernels, the rest for the runtime-size kernel
  {
    const bool no_fast = std::getenv("D4EST_HIP_TRANSFER_GENERIC") != nullptr;
    std::map<int, std::vector<int>> fl;
    std::map<int, int> fd, fo_;
    std::vector<int> gl;
    for (int i = 0; i < n_aux; ++i) {
      const int NH = aux_rec[4 * i], dN = aux_rec[4 * i + 1] - NH;
      if (!no_fast && NH >= 2 && NH <= kAmrFastMaxNH && dN <= kAmrFastMaxD) {
        fl[NH].push_back(i);
        fd[NH] = std::max(fd[NH], dN);
        fo_[NH] = std::max(fo_[NH], aux_rec[4 * i + 2]);
      } else {
        gl.push_back(i);
      }
    }
    std::vector<int> all;
    for (auto& kv : fl) {
      A->lists.push_back({kv.first, fd[kv.first], (int)all.size(), (int)kv.second.size(), fo_[kv.first]});
      all.insert(all.end(), kv.second.begin(), kv.second.end());
    }
    if (!gl.empty()) {
      A->lists.push_back({0, 0, (int)all.size(), (int)gl.size(), 0});
      all.insert(all.end(), gl.begin(), gl.end());
    }
    A->d_lists = dev_upload(all);
  }
  A->d_aux_rec = dev_upload(aux_rec);
  A->d_aux_src = dev_upload(aux_src);
  A->d_out_off = dev_upload(out_off);
  A->d_out_ops = dev_upload(out_ops);
  A->d_opsT = dev_upload(opsT, 16);
  A->d_adv_src = dev_upload(adv_src);
  A->d_adv_bal = dev_upload(adv_bal);
  level_alloc(A->next, new_deg);
  if (A->next.nodes != no) D4EST_HIP_ABORT("amr_set_balance: internal node count mismatch");

  if (A->two_stage) {   // the reference's two loops as two prolongations (d4est_amr.c:412-442, :449-479)
    std::vector<int> h1(n_old), dH1(n_old), dh1((size_t)8 * n_old, 0), h2(n_aux), dH2(n_aux), dh2((size_t)8 * n_aux, 0);
    for (int e = 0; e < n_old; ++e) {
      const int l = A->h_log[e];
      h1[e] = l < 0;
      dH1[e] = A->cur.deg[e];
      for (int c = 0; c < (l < 0 ? 8 : 1); ++c) dh1[8 * (size_t)e + c] = std::abs(l);
    }
    for (int i = 0; i < n_aux; ++i) {
      h2[i] = balance_log_host[i] < 0;
      dH2[i] = aux_deg[i];
      for (int c = 0; c < (h2[i] ? 8 : 1); ++c) dh2[8 * (size_t)i + c] = aux_deg[i];
    }
    A->t1 = d4est_hip_transfer_create(n_old, h1.data(), dH1.data(), dh1.data());
    A->t2 = d4est_hip_transfer_create(n_aux, h2.data(), dH2.data(), dh2.data());
    d4est_hip_transfer_set_stream(A->t1, (void*)A->stream);
    d4est_hip_transfer_set_stream(A->t2, (void*)A->stream);
    A->d_aux_field = dev_alloc<double>((size_t)ao);
  }
  A->balanced = true;
}

int d4est_hip_amr_new_n_elements(const d4est_hip_amr_t* A) {
  if (!A || !A->balanced) D4EST_HIP_ABORT("amr_new_n_elements: no balance log set");
  return A->next.n;
}

long long d4est_hip_amr_new_local_nodes(const d4est_hip_amr_t* A) {
  if (!A || !A->balanced) D4EST_HIP_ABORT("amr_new_local_nodes: no balance log set");
  return A->next.nodes;
}

void d4est_hip_amr_get_new_degrees(const d4est_hip_amr_t* A, int* deg_host) {
  if (!A || !A->balanced) D4EST_HIP_ABORT("amr_get_new_degrees: no balance log set");
  if (A->next.n > 0) {
    if (!deg_host) D4EST_HIP_ABORT("amr_get_new_degrees: NULL argument");
    memcpy(deg_host, A->next.deg.data(), (size_t)A->next.n * sizeof(int));
  }
}

void d4est_hip_amr_interpolate_field(d4est_hip_amr_t* A, const double* field_old_dev, double* field_new_dev) {
  if (!A || !A->balanced) D4EST_HIP_ABORT("amr_interpolate_field: no balance log set");
  if (A->n_aux == 0) return;
  if (!field_old_dev || !field_new_dev) D4EST_HIP_ABORT("amr_interpolate_field: NULL field");
  if (A->two_stage) {
    d4est_hip_transfer_prolong(A->t1, field_old_dev, A->d_aux_field);
    d4est_hip_transfer_prolong(A->t2, A->d_aux_field, field_new_dev);
    return;
  }
  for (const d4est_hip_amr::List& L : A->lists) {
    const int* list = A->d_lists + L.first;
    if (L.NH > 0) {
      launch_amr_fused(A, field_old_dev, field_new_dev, L.NH, L.dmax, list, L.n);
      continue;
    }
    const int n3 = A->max_n * A->max_n * A->max_n;
    const size_t lds = (size_t)2 * n3 * sizeof(double);
    if (lds > 160 * 1024) D4EST_HIP_ABORT("amr_interpolate_field: degree %d too high for the LDS-resident kernel", A->max_n - 1);
    set_lds_limit(amr_generic_kernel, lds);
    hipLaunchKernelGGL(amr_generic_kernel, dim3(std::min(L.n, 65536)), dim3(256), lds, A->stream, field_old_dev, field_new_dev, A->d_aux_rec,
                       A->d_aux_src, A->d_out_off, A->d_out_ops, A->d_opsT, list, L.n, n3);
  }
  HIP_CHECK(hipGetLastError());
}

int d4est_hip_amr_describe(const d4est_hip_amr_t* A, char* buf, int len) {
  if (!A) D4EST_HIP_ABORT("amr_describe: NULL amr");
  std::string s;
  char line[96];
  if (A->balanced) {
    if (A->two_stage) {
      snprintf(line, sizeof line, "-1 0 0 %d\n", A->n_aux);
      s += line;
    } else {
      for (const d4est_hip_amr::List& L : A->lists) {
        snprintf(line, sizeof line, "%d %d %d %d\n", L.NH, L.dmax, L.n_out, L.n);
        s += line;
      }
    }
  }
  if (buf && len > 0) {
    const size_t k = std::min(s.size(), (size_t)len - 1);
    memcpy(buf, s.data(), k);
    buf[k] = 0;
  }
  return (int)s.size();
}

void d4est_hip_amr_advance(d4est_hip_amr_t* A) {
  if (!A || !A->balanced) D4EST_HIP_ABORT("amr_advance: no balance log set");
  if (A->next.n > 0) {
    hipLaunchKernelGGL(amr_advance_kernel, grid_for(A->next.n), dim3(256), 0, A->stream, A->cur.d_pred, A->d_adv_src, A->d_adv_bal, A->gamma_h,
                       A->next.d_pred, A->next.n);
    HIP_CHECK(hipGetLastError());
  }
  // the kernel reads this step's tables: they are released only once it has run
  HIP_CHECK(hipStreamSynchronize(A->stream));
  std::swap(A->cur, A->next);
  balance_free(A);
  repart_free(A);
  level_free(A->next);
  A->h_log.clear();
  A->log_valid = false;
}

// ---- several ranks ------------------------------------------------------------------------------------------------------------------------
void d4est_hip_par_amr_set_comm(d4est_hip_amr_t* A, int rank, int world, d4est_hip_allreduce_fn allreduce, d4est_hip_amr_sendrecv_fn sendrecv,
                            void* ctx) {
  if (!A) D4EST_HIP_ABORT("amr_set_comm: NULL amr");
  if (world < 1 || rank < 0 || rank >= world) D4EST_HIP_ABORT("amr_set_comm: rank %d outside 0 .. world - 1 = %d", rank, world - 1);
  A->rank = rank;
  A->world = world;
  A->allreduce = allreduce;
  A->sendrecv = sendrecv;
  A->comm_ctx = ctx;
  repart_free(A);
}

void d4est_hip_par_amr_stats_global(d4est_hip_amr_t* A, const double* eta2_dev, int percentile, double* stats_dev) {
  if (!A || !stats_dev) D4EST_HIP_ABORT("amr_stats_global: NULL argument");
  if (percentile < 0 || percentile > 100) D4EST_HIP_ABORT("amr_stats_global: percentile %d outside 0 .. 100", percentile);
  const int n = A->cur.n;
  if (n > 0 && !eta2_dev) D4EST_HIP_ABORT("amr_stats_global: NULL eta2");
  if (A->world > 1 && !A->allreduce) D4EST_HIP_ABORT("amr_stats_global: world = %d, but no allreduce hook is set", A->world);
  hipLaunchKernelGGL(amr_local_sum_kernel, dim3(1), dim3(1024), 0, A->stream, eta2_dev, n, A->d_red);
  const unsigned blocks = (unsigned)std::min(std::max((n + kSelBins - 1) / kSelBins, 1), 1024);
  for (int pass = 0; pass < kSelPasses; ++pass) {
    hipLaunchKernelGGL(amr_sel_hist_kernel, dim3(blocks), dim3(kSelBins), 0, A->stream, eta2_dev, n, pass, A->d_sel, A->d_bins);
    hipLaunchKernelGGL(amr_sel_convert_kernel, dim3(1), dim3(2 * kSelBins), 0, A->stream, A->d_bins, A->d_red);
    HIP_CHECK(hipGetLastError());
    // one round per pass; the first also carries the local sum and the local n
    if (A->world > 1) A->allreduce(A->comm_ctx, A->d_red, pass == 0 ? kSelRed : 2 * kSelBins);
    hipLaunchKernelGGL(amr_sel_pick_kernel, dim3(1), dim3(64), 0, A->stream, A->d_red, pass, percentile, A->d_sel, stats_dev);
  }
  HIP_CHECK(hipGetLastError());
}

long long d4est_hip_par_amr_repartition(d4est_hip_amr_t* A, const long long* old_first, const long long* new_first) {
  if (!A || !old_first || !new_first) D4EST_HIP_ABORT("amr_repartition: NULL argument");
  if (A->balanced) D4EST_HIP_ABORT("amr_repartition: a balance log is set: repartition the level after d4est_hip_amr_advance");
  const int W = A->world, me = A->rank;
  if (old_first[0] != new_first[0] || old_first[W] != new_first[W])
    D4EST_HIP_ABORT("amr_repartition: the partitions cover different totals: old %lld .. %lld, new %lld .. %lld", old_first[0], old_first[W],
                    new_first[0], new_first[W]);
  for (int p = 0; p < W; ++p)
    if (old_first[p + 1] < old_first[p] || new_first[p + 1] < new_first[p])
      D4EST_HIP_ABORT("amr_repartition: the first-element arrays must be monotone (rank %d)", p);
  const long long olo = old_first[me], ohi = old_first[me + 1], nlo = new_first[me], nhi = new_first[me + 1];
  if (ohi - olo != (long long)A->cur.n)
    D4EST_HIP_ABORT("amr_repartition: the old partition gives rank %d %lld elements, the object holds %d", me, ohi - olo, A->cur.n);
  if (nhi - nlo > 0x7fffffffLL) D4EST_HIP_ABORT("amr_repartition: %lld elements on one rank", nhi - nlo);
  const int n_old = A->cur.n, n_new = (int)(nhi - nlo);
  const bool same = std::equal(old_first, old_first + W + 1, new_first);
  if (!same && !A->sendrecv) D4EST_HIP_ABORT("amr_repartition: world = %d, but no sendrecv hook is set", W);
  repart_free(A);
  d4est_hip_amr::Repart& R = A->rp;

  // rank me sends rank p the intersection of its old range with p's new range, and receives its new range's intersection with p's old one
  auto overlap = [](long long a0, long long a1, long long b0, long long b1) { return std::max(0LL, std::min(a1, b1) - std::max(a0, b0)); };
  std::vector<long long> se(1, 0), re(1, 0);   // per peer, in elements
  for (int p = 0; p < W; ++p) {
    if (p == me) continue;
    const long long ns = overlap(olo, ohi, new_first[p], new_first[p + 1]), nr = overlap(nlo, nhi, old_first[p], old_first[p + 1]);
    if (ns == 0 && nr == 0) continue;
    R.peers.push_back(p);
    se.push_back(se.back() + ns);
    re.push_back(re.back() + nr);
  }
  const long long self_n = overlap(olo, ohi, nlo, nhi);
  const long long self_old = self_n > 0 ? std::max(olo, nlo) - olo : 0, self_new = self_n > 0 ? std::max(olo, nlo) - nlo : 0;
  const long long n_send = n_old - self_n, n_recv = n_new - self_n;
  if (se.back() != n_send || re.back() != n_recv) D4EST_HIP_ABORT("amr_repartition: internal element count mismatch");
  const int np = (int)R.peers.size();

  // 1. degree and predictor to the new owner: one pack kernel, one round, one unpack kernel
  double* d_sbuf = dev_alloc<double>((size_t)2 * n_send);
  double* d_rbuf = dev_alloc<double>((size_t)2 * n_recv);
  int* d_ndeg = dev_alloc<int>((size_t)n_new);
  double* d_npred = dev_alloc<double>((size_t)n_new);
  auto grid_ll = [](long long n) { return dim3((unsigned)std::min<long long>(std::max<long long>((n + 255) / 256, 1), 65536)); };
  if (n_send > 0)
    hipLaunchKernelGGL(amr_state_pack_kernel, grid_ll(n_send), dim3(256), 0, A->stream, A->cur.d_deg, A->cur.d_pred, n_send, self_old, self_n,
                       d_sbuf);
  HIP_CHECK(hipGetLastError());
  if (!same) {   // every rank makes the round, also one without a peer: the hook may be a collective of the transport
    std::vector<long long> sf(se), rf(re);
    for (long long& v : sf) v *= 2;
    for (long long& v : rf) v *= 2;
    A->sendrecv(A->comm_ctx, np, R.peers.data(), d_sbuf, sf.data(), d_rbuf, rf.data());
  }
  if (n_recv > 0)
    hipLaunchKernelGGL(amr_state_unpack_kernel, grid_ll(n_recv), dim3(256), 0, A->stream, d_rbuf, n_recv, self_new, self_n, d_ndeg, d_npred);
  HIP_CHECK(hipGetLastError());
  if (self_n > 0) {
    HIP_CHECK(hipMemcpyAsync(d_ndeg + self_new, A->cur.d_deg + self_old, (size_t)self_n * sizeof(int), hipMemcpyDeviceToDevice, A->stream));
    HIP_CHECK(hipMemcpyAsync(d_npred + self_new, A->cur.d_pred + self_old, (size_t)self_n * sizeof(double), hipMemcpyDeviceToDevice, A->stream));
  }
  // 2. the received degrees
  std::vector<int> ndeg((size_t)n_new);
  if (n_new > 0) HIP_CHECK(hipMemcpyAsync(ndeg.data(), d_ndeg, (size_t)n_new * sizeof(int), hipMemcpyDeviceToHost, A->stream));
  HIP_CHECK(hipStreamSynchronize(A->stream));
  const int limit = amr_degree_limit();
  for (int e = 0; e < n_new; ++e)
    if (ndeg[e] < 1 || ndeg[e] > limit) D4EST_HIP_ABORT("amr_repartition: received degree %d for new element %d (outside 1 .. %d)", ndeg[e], e, limit);

  // node offsets of both element lists, for repartition_field
  auto nodes_of = [](int d) { return (long long)(d + 1) * (d + 1) * (d + 1); };
  std::vector<long long> opre((size_t)n_old + 1, 0), npre((size_t)n_new + 1, 0);
  for (int e = 0; e < n_old; ++e) opre[e + 1] = opre[e] + nodes_of(A->cur.deg[e]);
  for (int e = 0; e < n_new; ++e) npre[e + 1] = npre[e] + nodes_of(ndeg[e]);
  auto gap_e = [](long long i, long long at, long long len) { return i < at ? i : i + len; };   // buffer element -> local element
  R.send_first.assign(1, 0);
  R.recv_first.assign(1, 0);
  for (int i = 0; i < np; ++i) {
    long long ns = 0, nr = 0;
    if (se[i + 1] > se[i]) { const long long a = gap_e(se[i], self_old, self_n); ns = opre[a + (se[i + 1] - se[i])] - opre[a]; }
    if (re[i + 1] > re[i]) { const long long a = gap_e(re[i], self_new, self_n); nr = npre[a + (re[i + 1] - re[i])] - npre[a]; }
    R.send_first.push_back(R.send_first.back() + ns);
    R.recv_first.push_back(R.recv_first.back() + nr);
  }
  R.old_nodes = opre[n_old];
  R.new_nodes = npre[n_new];
  R.self_old = opre[self_old];
  R.self_new = npre[self_new];
  R.self_len = opre[self_old + self_n] - opre[self_old];
  if (R.self_len != npre[self_new + self_n] - npre[self_new]) D4EST_HIP_ABORT("amr_repartition: the part that stays changed its node count");
  R.n_send = R.old_nodes - R.self_len;
  R.n_recv = R.new_nodes - R.self_len;
  if (R.send_first.back() != R.n_send || R.recv_first.back() != R.n_recv) D4EST_HIP_ABORT("amr_repartition: internal node count mismatch");
  R.exchange = !same;
  R.d_send = dev_alloc<double>((size_t)R.n_send);
  R.d_recv = dev_alloc<double>((size_t)R.n_recv);

  // 3. the new local list becomes the current level
  level_alloc(A->next, ndeg);
  if (n_new > 0) HIP_CHECK(hipMemcpyAsync(A->next.d_pred, d_npred, (size_t)n_new * sizeof(double), hipMemcpyDeviceToDevice, A->stream));
  HIP_CHECK(hipStreamSynchronize(A->stream));
  std::swap(A->cur, A->next);
  level_free(A->next);
  (void)hipFree(d_sbuf); (void)hipFree(d_rbuf); (void)hipFree(d_ndeg); (void)hipFree(d_npred);
  A->h_log.clear();
  A->log_valid = false;
  R.valid = true;
  return A->cur.nodes;
}

void d4est_hip_par_amr_repartition_field(d4est_hip_amr_t* A, const double* field_old_dev, double* field_new_dev) {
  if (!A || !A->rp.valid) D4EST_HIP_ABORT("amr_repartition_field: no repartition since the last advance");
  const d4est_hip_amr::Repart& R = A->rp;
  if ((R.old_nodes > 0 && !field_old_dev) || (R.new_nodes > 0 && !field_new_dev)) D4EST_HIP_ABORT("amr_repartition_field: NULL field");
  auto grid_ll = [](long long n) { return dim3((unsigned)std::min<long long>(std::max<long long>((n + 255) / 256, 1), 65536)); };
  if (R.n_send > 0)
    hipLaunchKernelGGL(amr_gap_copy_kernel, grid_ll(R.n_send), dim3(256), 0, A->stream, field_old_dev, R.d_send, R.n_send, R.self_old, R.self_len, 0);
  HIP_CHECK(hipGetLastError());
  if (R.exchange)
    A->sendrecv(A->comm_ctx, (int)R.peers.size(), R.peers.data(), R.d_send, R.send_first.data(), R.d_recv, R.recv_first.data());
  if (R.n_recv > 0)
    hipLaunchKernelGGL(amr_gap_copy_kernel, grid_ll(R.n_recv), dim3(256), 0, A->stream, R.d_recv, field_new_dev, R.n_recv, R.self_new, R.self_len, 1);
  HIP_CHECK(hipGetLastError());
  if (R.self_len > 0)
    HIP_CHECK(hipMemcpyAsync(field_new_dev + R.self_new, field_old_dev + R.self_old, (size_t)R.self_len * sizeof(double), hipMemcpyDeviceToDevice,
                             A->stream));
}

}  // extern "C"
