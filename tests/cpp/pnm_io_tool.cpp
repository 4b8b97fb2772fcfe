// pnm_io_tool.cpp -- stand-alone check of pft/pnm_io.hpp (tests/test_depth_host.py builds it with
// -fsanitize=address,undefined and runs it on the CPU; it links nothing of the HIP library).  Every parse runs on a heap
// copy of exactly the bytes offered, so a read past the buffer is a sanitizer report.  Prints "ok" and returns 0, or the
// failed checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pft/pnm_io.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
      failures++;                                                     \
    }                                                                 \
  } while (0)

// the parser sees an allocation of exactly n bytes
static bool pgm(const uint8_t* p, size_t n, pft::DepthImage& img, std::string& err) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(copy.get(), p, n);
  return pft::parsePgm16(n ? copy.get() : nullptr, n, img, err);
}
static bool ppm(const uint8_t* p, size_t n, pft::ColorImage& img, std::string& err) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(copy.get(), p, n);
  return pft::parsePpm8(n ? copy.get() : nullptr, n, img, err);
}
static std::vector<uint8_t> bytes(const std::string& head, size_t payload, uint8_t fill = 7) {
  std::vector<uint8_t> v(head.begin(), head.end());
  v.insert(v.end(), payload, fill);
  return v;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::string err;
  pft::DepthImage d;
  d.width = 5;
  d.height = 3;
  for (int i = 0; i < 15; i++) d.data.push_back((uint16_t)(i == 0 ? 0 : (i == 1 ? 65535 : 256 * i + (255 - i))));
  pft::ColorImage c;
  c.width = 5;
  c.height = 3;
  for (int i = 0; i < 45; i++) c.data.push_back((uint8_t)(i * 5 + 1));

  // write / read round trip through files
  CHECK(pft::savePgm16(dir + "/t.pgm", d, err));
  CHECK(pft::savePpm8(dir + "/t.ppm", c, err));
  pft::DepthImage d2;
  pft::ColorImage c2;
  CHECK(pft::loadPgm16(dir + "/t.pgm", d2, err) && d2.width == 5 && d2.height == 3 && d2.data == d.data);
  CHECK(pft::loadPpm8(dir + "/t.ppm", c2, err) && c2.width == 5 && c2.height == 3 && c2.data == c.data);
  CHECK(!pft::loadPgm16(dir + "/missing.pgm", d2, err) && err.find("cannot open") != std::string::npos);
  CHECK(!pft::loadPgm16(dir + "/t.ppm", d2, err));  // the other kind
  CHECK(!pft::loadPpm8(dir + "/t.pgm", c2, err));
  pft::DepthImage bad_size = d;
  bad_size.data.pop_back();
  CHECK(!pft::savePgm16(dir + "/bad.pgm", bad_size, err));

  // samples are big-endian
  const std::vector<uint8_t> enc = pft::encodePgm16(d);
  const std::string head = "P5\n5 3\n65535\n";
  CHECK(enc.size() == head.size() + 30 && std::memcmp(enc.data(), head.data(), head.size()) == 0);
  CHECK(enc[head.size() + 4] == 0x02 && enc[head.size() + 5] == 0xfd);  // sample 2 = 0x02fd

  // comments and arbitrary header whitespace
  {
    const std::vector<uint8_t> v = bytes("P5 # a comment\n#another\n \t 2\r\n#c\n  2 # trailing\n65535\n", 8, 0x01);
    CHECK(pgm(v.data(), v.size(), d2, err) && d2.width == 2 && d2.height == 2 && d2.data[3] == 0x0101);
    const std::vector<uint8_t> w = bytes("P6\n# made by a camera\n2 1\n255 ", 6, 9);
    CHECK(ppm(w.data(), w.size(), c2, err) && c2.width == 2 && c2.height == 1 && c2.data.size() == 6 && c2.data[5] == 9);
    // a '#' right behind maxval starts a comment that swallows the separator: no header end, never a crash
    const std::vector<uint8_t> x = bytes("P5\n1 1\n65535#\n", 2);
    pgm(x.data(), x.size(), d2, err);
  }

  // refused: a maxval of 255 for depth, any other maxval, bad magic, bad sizes, junk
  const char* refused[] = {"P5\n2 2\n255\n", "P5\n2 2\n65534\n", "P5\n2 2\n65536\n", "P2\n2 2\n65535\n", "P6\n2 2\n65535\n",
                           "P5\n0 2\n65535\n", "P5\n2 0\n65535\n", "P5\n-2 2\n65535\n", "P5\n2 x\n65535\n",
                           "P5\n99999999999999999999 2\n65535\n", "P5\n16385 1\n65535\n", "P5\n2 2\n65535X", "P5", "P", "",
                           "P5\n2 2\n", "P5\n2 2\n65535", "P5\n#never ends"};
  for (const char* r : refused) {
    const std::vector<uint8_t> v = bytes(r, 64);
    err.clear();
    CHECK(!pgm(v.data(), std::strlen(r) < 4 ? std::strlen(r) : v.size(), d2, err) && !err.empty());
  }
  {
    const std::vector<uint8_t> v = bytes("P6\n2 2\n65535\n", 64);
    CHECK(!ppm(v.data(), v.size(), c2, err));
    const std::vector<uint8_t> ok255 = bytes("P6\n2 2\n255\n", 12);
    CHECK(ppm(ok255.data(), ok255.size(), c2, err));
  }

  // a file truncated at every byte: an error each time, the whole file parses
  const std::vector<uint8_t> full_d = pft::encodePgm16(d), full_c = pft::encodePpm8(c);
  for (size_t n = 0; n < full_d.size(); n++) {
    err.clear();
    CHECK(!pgm(full_d.data(), n, d2, err) && !err.empty());
  }
  CHECK(pgm(full_d.data(), full_d.size(), d2, err) && d2.data == d.data);
  for (size_t n = 0; n < full_c.size(); n++) {
    err.clear();
    CHECK(!ppm(full_c.data(), n, c2, err) && !err.empty());
  }
  CHECK(ppm(full_c.data(), full_c.size(), c2, err) && c2.data == c.data);
  // bytes behind the image are ignored
  {
    std::vector<uint8_t> more = full_d;
    more.push_back(0xee);
    CHECK(pgm(more.data(), more.size(), d2, err) && d2.data == d.data);
  }

  if (failures) return 1;
  std::puts("ok");
  return 0;
}
