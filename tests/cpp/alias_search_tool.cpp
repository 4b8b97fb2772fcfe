// alias_search_tool IN OUT -- the resample kernels' alias-table search (pcl_tracking_amd/csrc/pft_alias.h, the very text
// the kernels compile) run on the host, for tests/test_alias_search_host.py.
//
// IN:  any number of cases { uint32 n; float w[n]; }
// OUT: per case { uint32 n; uint32 variants; } then `variants` tables { int32 a[n]; double q[n]; }:
//        0  no coarse level (the plain one-level search: what k_alias_materialize runs)
//        1  the kernels' own strides, sD = ceil(m / 256), sE = ceil(nh / 256)
//        2.. forced strides 1, 2, 3, 7 and n for both arrays
//
// The prefix-sum form is built here sequentially from its specification (header comment of
// pft_population.hip), not by the kernels' scans: q_i = (double)(w_i * (float)n); the small list L (q < 1) and the large
// list H (q >= 1), both with the highest particle index first; D / E the inclusive running deficit (1 - q) over L /
// excess (q - 1) over H in double; pos[i] = position in its list | large << 31.  The coarse levels follow the kernels'
// formula c[t] = a[min((t + 1) * s, len) - 1] for t * s < len.  Every array has exactly the length in use, so that a
// sanitizer build sees any read past it.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "pft_alias.h"

static std::vector<double> coarse(const std::vector<double>& a, uint32_t s) {
  std::vector<double> c;
  const uint32_t len = (uint32_t)a.size();
  if (!len || !s) return c;
  for (uint32_t t = 0; (uint64_t)t * s < len; t++) c.push_back(a[min((uint64_t)(t + 1u) * s, (uint64_t)len) - 1u]);
  return c;
}

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
  const std::unique_ptr<double[]> none(new double[0]);
  uint32_t n;
  while (fread(&n, sizeof(n), 1, in) == 1) {
    std::vector<float> w(n);
    if (n && fread(w.data(), sizeof(float), n, in) != n) {
      fprintf(stderr, "truncated case\n");
      return 2;
    }
    std::vector<int32_t> L, H;
    std::vector<double> D, E;
    std::vector<uint32_t> pos(n);
    double d = 0.0, e = 0.0;
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t i = n - 1u - j;
      const double q = (double)(w[i] * (float)n);
      if (q < 1.0) {
        d += 1.0 - q;
        pos[i] = (uint32_t)L.size();
        L.push_back((int32_t)i);
        D.push_back(d);
      } else {
        e += q - 1.0;
        pos[i] = (uint32_t)H.size() | 0x80000000u;
        H.push_back((int32_t)i);
        E.push_back(e);
      }
    }
    AliasView v;
    v.L = L.data();
    v.H = H.data();
    v.D = D.data();
    v.E = E.data();
    v.pos = pos.data();
    v.m = (uint32_t)L.size();
    v.nh = (uint32_t)H.size();
    v.n = n;
    const uint32_t forced[5] = {1u, 2u, 3u, 7u, n};
    const uint32_t variants = 2u + 5u;
    fwrite(&n, sizeof(n), 1, out);
    fwrite(&variants, sizeof(variants), 1, out);
    std::vector<int32_t> a(n);
    std::vector<double> q(n);
    for (uint32_t var = 0; var < variants; var++) {
      std::vector<double> cD, cE;
      AliasView u = v;
      if (var >= 1u) {
        u.sD = var == 1u ? (v.m + 255u) / 256u : forced[var - 2u];
        u.sE = var == 1u ? (v.nh + 255u) / 256u : forced[var - 2u];
        cD = coarse(D, u.sD);
        cE = coarse(E, u.sE);
        // (the kernels hand over their LDS arrays whatever m and nh are: non-null, with nothing to read when a list is empty)
        u.cD = cD.empty() ? none.get() : cD.data();
        u.cE = cE.empty() ? none.get() : cE.data();
      }
      for (uint32_t k = 0; k < n; k++) {
        int32_t a_large;
        q[k] = alias_q(u, k, w[k], &a_large);
        a[k] = (u.pos[k] >> 31) ? a_large : alias_a_small(u, k);
      }
      fwrite(a.data(), sizeof(int32_t), n, out);
      fwrite(q.data(), sizeof(double), n, out);
    }
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  return 0;
}
