// segment_solve_tool IN OUT -- the one-lane tail of the plane refit (pcl_tracking_amd/csrc/pft_segment_solve.h, the very
// text k_sg_refit and k_sg_refit_top compile) run on the host, for tests/test_segment_refit_host.py.
//
// IN:  any number of cases { float accu[9]; uint32 m; }     the nine means and the count they were divided by
// OUT: per case one pft_segment_refit_debug (include/pft_segment.h)
#include <cstdint>
#include <cstdio>

#include "pft_segment_solve.h"

struct Case {
  float accu[9];
  uint32_t m;
};

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
  Case k;
  while (fread(&k, sizeof(k), 1, in) == 1) {
    pft_segment_refit_debug o = {};
    sg_refit_solve(k.accu, k.m, &o);
    if (fwrite(&o, sizeof(o), 1, out) != 1) return 1;
  }
  fclose(in);
  fclose(out);
  return 0;
}
