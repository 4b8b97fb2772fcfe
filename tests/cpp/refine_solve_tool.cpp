// refine_solve_tool IN OUT -- the one-lane part of the pose refinement (pcl_tracking_amd/csrc/pft_refine_solve.h, the very
// text k_refine_step compiles) run on the host, for tests/test_refine_host.py.
//
// IN:  any number of cases { double sums[17]; double c[3]; float start[12]; uint32 n; uint32 pad; }
// OUT: per case { double Q0[4], t0[3];            the state of `start` (refine_state_from_matrix)
//                 double Q[4], t[3];              the state after one refine_solve from it
//                 double dq[4], step2[2];
//                 float T[12];                    refine_transform of the new state
//                 uint32 sweeps, pad; }
#include <cstdint>
#include <cstdio>

#include "pft_refine_solve.h"

struct Case {
  double sums[PFT_REFINE_SUMS];
  double c[3];
  float start[12];
  uint32_t n, pad;
};
struct Out {
  double Q0[4], t0[3], Q[4], t[3], dq[4], step2[2];
  float T[12];
  uint32_t sweeps, pad;
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
    Out o = {};
    PftRefineState s;
    refine_state_from_matrix(k.start, &s);
    for (int i = 0; i < 4; i++) o.Q0[i] = s.Q[i];
    for (int i = 0; i < 3; i++) o.t0[i] = s.t[i];
    o.sweeps = refine_solve(k.sums, k.n, k.c, &s, o.dq, o.step2);
    for (int i = 0; i < 4; i++) o.Q[i] = s.Q[i];
    for (int i = 0; i < 3; i++) o.t[i] = s.t[i];
    refine_transform(&s, o.T);
    if (fwrite(&o, sizeof(o), 1, out) != 1) return 1;
  }
  fclose(in);
  fclose(out);
  return 0;
}
