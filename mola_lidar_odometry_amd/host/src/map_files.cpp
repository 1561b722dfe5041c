// map_files.cpp -- see map_files.h.
#include "map_files.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace mola_hip {

std::string slurp(const char* who, const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error(std::string(who) + ": cannot open '" + path + "'");
  std::stringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

void write_file(const char* who, const std::string& path, const std::string& bytes, std::ios::openmode mode) {
  std::ofstream out(path, std::ios::binary | mode);
  out.write(bytes.data(), (std::streamsize)bytes.size());
  out.close();
  if (!out) throw std::runtime_error(std::string(who) + ": cannot write '" + path + "'");
}

std::string g9(double v) {
  char buf[64];
  snprintf(buf, sizeof(buf), "%.9g", v);
  return buf;
}

std::string base_name(const std::string& path) { return path.substr(dir_of(path).size()); }

std::string dir_of(const std::string& path) {
  const size_t s = path.find_last_of('/');
  return s == std::string::npos ? "" : path.substr(0, s + 1);
}

bool yaml_line(const std::string& text, const std::string& key, std::string& rest) {
  bool found = false;
  std::istringstream in(text);
  for (std::string line; std::getline(in, line);)
    if (line.rfind(key, 0) == 0) {
      rest = line.substr(key.size());
      found = true;
    }
  return found;
}

std::string pgm_bytes(const uint8_t* plane, uint32_t nx, uint32_t ny, uint8_t (*byte)(uint8_t)) {
  std::string pgm = "P5\n" + std::to_string(nx) + " " + std::to_string(ny) + "\n255\n";
  const size_t head = pgm.size();
  pgm.resize(head + (size_t)nx * ny);
  for (uint32_t r = 0; r < ny; r++) {
    const uint8_t* src = plane + (size_t)(ny - 1 - r) * nx;
    for (uint32_t c = 0; c < nx; c++) pgm[head + (size_t)r * nx + c] = (char)(byte ? byte(src[c]) : src[c]);
  }
  return pgm;
}

bool pgm_plane(const std::string& s, uint32_t want_nx, uint32_t want_ny, uint32_t& nx, uint32_t& ny, std::vector<uint8_t>& plane) {
  unsigned px = 0, py = 0, maxv = 0;
  int used = 0;
  // (no white space behind the last number in the format: it would swallow pixels that happen to be 9 .. 13 or 32)
  if (sscanf(s.c_str(), "P5\n%u %u\n%u%n", &px, &py, &maxv, &used) != 3 || maxv != 255 || used <= 0 || px == 0 || py == 0) return false;
  if ((want_nx && px != want_nx) || (want_ny && py != want_ny)) return false;
  const size_t n = (size_t)px * py, head = (size_t)used + 1;
  if (s.size() != head + n || s[head - 1] != '\n') return false;
  nx = px;
  ny = py;
  plane.resize(n);
  for (uint32_t r = 0; r < ny; r++) memcpy(&plane[(size_t)(ny - 1 - r) * nx], &s[head + (size_t)r * nx], nx);
  return true;
}

}  // namespace mola_hip
