// pnm_io.hpp -- the two image files of a depth frame (pft::InputFilter::setInputDepth), host only, no dependency:
//
//   depth   binary PGM  "P5", maxval 65535, two bytes per sample, most significant first (the Netpbm rule)
//   colour  binary PPM  "P6", maxval 255, three bytes per pixel: R, G, B
//
// Headers are read as Netpbm writes them: any whitespace between the fields, `#` comments up to the end of the line
// anywhere before the single whitespace byte that ends the header.  A file that is truncated or malformed is an error with
// a text, never a read past the buffer: every parser works on (pointer, size) and checks the size before it reads.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace pft {

struct DepthImage {  // millimetres unless the writer says otherwise; 0 = no measurement
  int width = 0, height = 0;
  std::vector<uint16_t> data;  // row-major, host byte order
};
struct ColorImage {
  int width = 0, height = 0;
  std::vector<uint8_t> data;  // row-major R, G, B
};

namespace pnm_detail {
constexpr int kMaxAxis = 16384;  // PFT_DEPTH_MAX_AXIS

// the next unsigned decimal field of a header; false at the end of the buffer, on another byte, or above `limit`
inline bool field(const uint8_t* p, size_t n, size_t& pos, long limit, long& out) {
  for (;;) {  // whitespace and comments in front of the field
    if (pos >= n) return false;
    const uint8_t c = p[pos];
    if (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f') {
      pos++;
    } else if (c == '#') {
      while (pos < n && p[pos] != '\n' && p[pos] != '\r') pos++;
    } else {
      break;
    }
  }
  if (p[pos] < '0' || p[pos] > '9') return false;
  long v = 0;
  while (pos < n && p[pos] >= '0' && p[pos] <= '9') {
    v = v * 10 + (p[pos] - '0');
    if (v > limit) return false;
    pos++;
  }
  out = v;
  return true;
}

// "P5" / "P6", width, height, maxval, one whitespace byte; pos ends on the first sample
inline bool header(const uint8_t* p, size_t n, char kind, long want_maxval, int& w, int& h, size_t& pos, std::string& err) {
  if (!p || n < 2 || p[0] != 'P' || p[1] != (uint8_t)kind) {
    err = std::string("not a binary P") + kind + " file";
    return false;
  }
  pos = 2;
  long lw = 0, lh = 0, mv = 0;
  if (!field(p, n, pos, kMaxAxis, lw) || !field(p, n, pos, kMaxAxis, lh) || lw < 1 || lh < 1) {
    err = "width and height must be 1 .. 16384";
    return false;
  }
  if (!field(p, n, pos, 65535, mv) || mv != want_maxval) {
    err = "maxval must be " + std::to_string(want_maxval);
    return false;
  }
  if (pos >= n || !(p[pos] == ' ' || p[pos] == '\t' || p[pos] == '\n' || p[pos] == '\r' || p[pos] == '\v' || p[pos] == '\f')) {
    err = "the header does not end in a whitespace byte";
    return false;
  }
  pos++;
  w = (int)lw;
  h = (int)lh;
  return true;
}

inline bool readFile(const std::string& path, std::vector<uint8_t>& out, std::string& err) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    err = "cannot open " + path;
    return false;
  }
  out.clear();
  uint8_t buf[65536];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
  const bool ok = !std::ferror(f);
  std::fclose(f);
  if (!ok) err = "cannot read " + path;
  return ok;
}

inline bool writeFile(const std::string& path, const std::vector<uint8_t>& bytes, std::string& err) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) {
    err = "cannot create " + path;
    return false;
  }
  const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
  if (std::fclose(f) != 0 || !ok) {
    err = "cannot write " + path;
    return false;
  }
  return true;
}
}  // namespace pnm_detail

// a P5 file with maxval 65535 in memory -> img.  A maxval of 255 (one byte per sample) is refused: it is no depth image
inline bool parsePgm16(const uint8_t* bytes, size_t n, DepthImage& img, std::string& err) {
  int w = 0, h = 0;
  size_t pos = 0;
  if (!pnm_detail::header(bytes, n, '5', 65535, w, h, pos, err)) return false;
  const size_t count = (size_t)w * (size_t)h;
  if (n - pos < count * 2) {
    err = "truncated: " + std::to_string(n - pos) + " bytes of samples, " + std::to_string(count * 2) + " needed";
    return false;
  }
  img.width = w;
  img.height = h;
  img.data.resize(count);
  const uint8_t* s = bytes + pos;
  for (size_t i = 0; i < count; i++) img.data[i] = (uint16_t)((unsigned)s[2 * i] << 8 | (unsigned)s[2 * i + 1]);
  return true;
}

// a P6 file with maxval 255 in memory -> img
inline bool parsePpm8(const uint8_t* bytes, size_t n, ColorImage& img, std::string& err) {
  int w = 0, h = 0;
  size_t pos = 0;
  if (!pnm_detail::header(bytes, n, '6', 255, w, h, pos, err)) return false;
  const size_t count = (size_t)w * (size_t)h * 3;
  if (n - pos < count) {
    err = "truncated: " + std::to_string(n - pos) + " bytes of samples, " + std::to_string(count) + " needed";
    return false;
  }
  img.width = w;
  img.height = h;
  img.data.assign(bytes + pos, bytes + pos + count);
  return true;
}

inline std::vector<uint8_t> encodePgm16(const DepthImage& img) {
  const std::string head = "P5\n" + std::to_string(img.width) + " " + std::to_string(img.height) + "\n65535\n";
  std::vector<uint8_t> out(head.begin(), head.end());
  const size_t count = (size_t)img.width * (size_t)img.height;
  out.reserve(out.size() + 2 * count);
  for (size_t i = 0; i < count && i < img.data.size(); i++) {
    out.push_back((uint8_t)(img.data[i] >> 8));
    out.push_back((uint8_t)(img.data[i] & 255u));
  }
  return out;
}

inline std::vector<uint8_t> encodePpm8(const ColorImage& img) {
  const std::string head = "P6\n" + std::to_string(img.width) + " " + std::to_string(img.height) + "\n255\n";
  std::vector<uint8_t> out(head.begin(), head.end());
  const size_t count = (size_t)img.width * (size_t)img.height * 3;
  out.insert(out.end(), img.data.begin(), img.data.begin() + (count < img.data.size() ? count : img.data.size()));
  return out;
}

inline bool loadPgm16(const std::string& path, DepthImage& img, std::string& err) {
  std::vector<uint8_t> bytes;
  if (!pnm_detail::readFile(path, bytes, err)) return false;
  if (parsePgm16(bytes.data(), bytes.size(), img, err)) return true;
  err = path + ": " + err;
  return false;
}

inline bool loadPpm8(const std::string& path, ColorImage& img, std::string& err) {
  std::vector<uint8_t> bytes;
  if (!pnm_detail::readFile(path, bytes, err)) return false;
  if (parsePpm8(bytes.data(), bytes.size(), img, err)) return true;
  err = path + ": " + err;
  return false;
}

inline bool savePgm16(const std::string& path, const DepthImage& img, std::string& err) {
  if (img.width < 1 || img.height < 1 || img.data.size() != (size_t)img.width * (size_t)img.height) {
    err = "savePgm16: the image does not hold width x height samples";
    return false;
  }
  return pnm_detail::writeFile(path, encodePgm16(img), err);
}

inline bool savePpm8(const std::string& path, const ColorImage& img, std::string& err) {
  if (img.width < 1 || img.height < 1 || img.data.size() != (size_t)img.width * (size_t)img.height * 3) {
    err = "savePpm8: the image does not hold width x height x 3 bytes";
    return false;
  }
  return pnm_detail::writeFile(path, encodePpm8(img), err);
}

}  // namespace pft
