// spread_final_tool IN OUT -- the one-lane finalisation of the population statistics
// (pcl_tracking_amd/csrc/pft_spread_final.h, the very text k_spread_final compiles) run on the host, for
// tests/test_spread_host.py: fed the 29 sums, it must equal tests/spread_model.py byte for byte.
//
// IN:  any number of cases { double sums[29]; double max_pos_sigma, min_n_eff; float pivot[6]; float w_max;
//                            uint32 n, n_zero, i_max, after, prev_streak; }  (296 bytes, no padding)
// OUT: per case one pft_population_stats (688 bytes); `calls` is 0
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pft_spread_final.h"

struct Case {
  double sums[PFT_SPREAD_SUMS];
  double max_pos_sigma, min_n_eff;
  float pivot[6];
  float w_max;
  uint32_t n, n_zero, i_max, after, prev_streak;
};
static_assert(sizeof(Case) == 296, "case record");
static_assert(sizeof(pft_population_stats) == 688, "pft_population_stats");

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
    return 2;
  }
  Case c;
  while (fread(&c, sizeof(c), 1, in) == 1) {
    pft_population_stats r;
    memset(&r, 0, sizeof(r));
    r.streak = c.prev_streak;
    spread_finalize(c.sums, c.n, c.n_zero, c.w_max, c.i_max, c.pivot, c.max_pos_sigma, c.min_n_eff, c.after, &r);
    fwrite(&r, sizeof(r), 1, out);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  return 0;
}
