// The hybrid operator's bucket rule: which degree buckets' clean elements get the one-kernel path, and whether the operator is set up at
// all.  Plain C++ (no HIP, no plan) so that the default rule can be tested on its own: tests/test_hybrid_bucket_rule.py.
#pragma once
#include <cstddef>
#include <vector>

namespace d4est_hip {

// a clean bucket is worth a launch of its own at size from this many clean elements on
constexpr int kHybridBucketMinClean = 2048;

struct HybridBucketChoice {
  std::vector<char> keep;    // per bucket: its clean elements stay clean (the other buckets' go to the two-phase lists); empty without set_up
  bool set_up = false;       // the hybrid operator is set up
  bool all_buckets = false;  // ... with every kept bucket as a launch of its own (the at-size rule)
};

// clean_per_bucket: clean elements per degree bucket; hybrid_tuning: tuning key 14 (> 0 forces the operator, < 0 is the default rule);
// one_bucket_only: D4EST_HIP_HYBRID_ONE_BUCKET_ONLY is set (it blocks both demotion rules).
//
// default: only where it was measured to pay -- ONE clean degree bucket holding at least half of the elements (a locally refined mesh of
// one degree: level 4, p = 7, every 64th octant refined 144 -> 125 us).  With several clean buckets every bucket is its own launch of
// a latency-structured kernel (25 - 40 us for a few hundred elements each, whatever their number): back to back they cost more than
// the two-phase kernels save, and on side streams the cross-queue event waits (about 50 us per fork / join on this runtime) eat the
// overlap (graded p = 3 ... 9, 4096 elements: 144 us two-phase, 275 us serial, 250 us forked) -- tuning value 1 still forces it
// (round 4: with several clean buckets the default keeps the LARGEST one where it holds at least half of the mesh -- a mesh with one
// dominant degree -- and leaves the other buckets' elements to the two-phase lists)
// ... and, at size, every clean bucket of at least 2048 clean elements (the smaller buckets' elements stay two-phase): with thousands of
// clean elements per bucket the buckets' launches fill the chip and their latency no longer matters (level 5, 32 768 elements, graded
// p = 3 ... 9: two-phase 756 us, hybrid 691 us; hanging + plateaus 1033 -> 894 us; at level 4, 385 clean elements per bucket: 275 against
// 126 us)
inline HybridBucketChoice hybrid_choose_buckets(const std::vector<int>& clean_per_bucket, int n_elements, int hybrid_tuning, bool one_bucket_only) {
  const std::vector<int>& cnt = clean_per_bucket;
  const size_t ne = (size_t)n_elements;
  HybridBucketChoice c;
  c.keep.assign(cnt.size(), 1);
  int clean_buckets = 0, best = -1, n_kept = 0;
  size_t n_clean = 0, kept_sum = 0;
  for (size_t b = 0; b < cnt.size(); ++b) {
    n_clean += (size_t)cnt[b];
    if (cnt[b] > 0) ++clean_buckets;
    if (best < 0 || cnt[b] > cnt[best]) best = (int)b;   // (a tie: the first largest)
    // the buckets that are worth a launch of their own at size
    if (cnt[b] >= kHybridBucketMinClean) { ++n_kept; kept_sum += (size_t)cnt[b]; }
  }
  const bool may_demote = hybrid_tuning < 0 && clean_buckets > 1 && !one_bucket_only;
  if (may_demote && n_kept >= 2 && 2 * kept_sum >= ne) {
    for (size_t b = 0; b < cnt.size(); ++b) c.keep[b] = cnt[b] >= kHybridBucketMinClean;   // (small buckets' elements: two-phase)
    n_clean = kept_sum;
    c.all_buckets = true;
  } else if (may_demote && best >= 0 && 2 * (size_t)cnt[best] >= ne) {
    for (size_t b = 0; b < cnt.size(); ++b) c.keep[b] = (int)b == best;
    n_clean = (size_t)cnt[best];
    clean_buckets = 1;
  }
  c.set_up = n_clean > 0 && (hybrid_tuning > 0 || c.all_buckets || (clean_buckets == 1 && 2 * n_clean >= ne));
  if (!c.set_up) c.keep.clear();
  return c;
}

}  // namespace d4est_hip
