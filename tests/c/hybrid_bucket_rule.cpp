// Stand-alone driver of the hybrid operator's bucket rule (disco4est_amd/csrc/d4est_hip_hybrid_buckets.h: plain C++, no HIP):
//   hybrid_bucket_rule N_ELEMENTS TUNING ONE_BUCKET_ONLY CLEAN_0 [CLEAN_1 ...]
// prints "set_up all_buckets: kept bucket numbers" for tests/test_hybrid_bucket_rule.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "d4est_hip_hybrid_buckets.h"

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s n_elements tuning one_bucket_only clean_per_bucket...\n", argv[0]);
    return 2;
  }
  std::vector<int> cnt;
  for (int i = 4; i < argc; ++i) cnt.push_back(std::atoi(argv[i]));
  const d4est_hip::HybridBucketChoice c = d4est_hip::hybrid_choose_buckets(cnt, std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]) != 0);
  if (c.set_up && c.keep.size() != cnt.size()) return 3;
  if (!c.set_up && !c.keep.empty()) return 3;
  std::printf("%d %d:", (int)c.set_up, (int)c.all_buckets);
  for (size_t b = 0; b < c.keep.size(); ++b)
    if (c.keep[b]) std::printf(" %zu", b);
  std::printf("\n");
  return 0;
}
