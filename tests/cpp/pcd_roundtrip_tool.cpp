// writes a raw array of 32-byte points as PCD (pft::io::writePCDFile, binary or ascii) and reads it back with
// pft::io::loadPCDFile; prints "ok <n>" when every binary point keeps its bits (ascii: x y z within 8 digits, rgba)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "pft/pcd_io.hpp"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const bool binary = std::string(argv[3]) == "binary";
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  pft::PointCloud<pft::PointXYZRGBA> c;
  pft::PointXYZRGBA q;
  while (std::fread(&q, sizeof(q), 1, f) == 1) c.points.push_back(q);
  std::fclose(f);
  c.width = (uint32_t)c.points.size();
  if (pft::io::writePCDFile(argv[2], c, binary) != 0) return 3;
  pft::PointCloud<pft::PointXYZRGBA> r;
  if (pft::io::loadPCDFile(argv[2], r) != 0 || r.points.size() != c.points.size()) return 4;
  for (size_t i = 0; i < c.points.size(); i++) {
    const pft::PointXYZRGBA &a = c.points[i], &b = r.points[i];
    if (a.rgba != b.rgba) return 5;
    const float va[3] = {a.x, a.y, a.z}, vb[3] = {b.x, b.y, b.z};
    for (int k = 0; k < 3; k++) {
      if (std::isnan(va[k]) != std::isnan(vb[k])) return 6;
      if (std::isnan(va[k])) continue;
      if (binary ? std::memcmp(&va[k], &vb[k], 4) != 0 : std::fabs(va[k] - vb[k]) > 1e-7f * std::fabs(va[k]) + 1e-30f)
        return 7;
    }
  }
  std::printf("ok %zu\n", c.points.size());
  return 0;
}
