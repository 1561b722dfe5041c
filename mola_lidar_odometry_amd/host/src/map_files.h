// map_files.h -- what the grid files of OccupancyGrid.h, Traversability.h and NavCostmap.h share: whole files in and out, the
// "%.9g" text of a number, the two halves of a path prefix, "key: value" lines, and the binary PGM of a plane.  Internal to host/src.
// `who` is the calling function's name, as it stands in front of its refusals.
#pragma once
#include <cstdint>
#include <ios>
#include <string>
#include <vector>

namespace mola_hip {

std::string slurp(const char* who, const std::string& path);  // "<who>: cannot open '<path>'"
void write_file(const char* who, const std::string& path, const std::string& bytes, std::ios::openmode mode);  // "<who>: cannot write '<path>'"

std::string g9(double v);                         // "%.9g"
std::string base_name(const std::string& path);   // what follows the last '/'
std::string dir_of(const std::string& path);      // up to and including the last '/', or ""

// the rest of the last line of `text` that begins with `key`; false when there is none
bool yaml_line(const std::string& text, const std::string& key, std::string& rest);

// "P5\n<nx> <ny>\n255\n" and ny * nx bytes, row 0 of the image = the largest y.  `plane` is bottom-up; `byte` (optional) maps each one.
std::string pgm_bytes(const uint8_t* plane, uint32_t nx, uint32_t ny, uint8_t (*byte)(uint8_t) = nullptr);
// The reverse, of exactly that header and size; the plane comes back bottom-up.  want_nx, want_ny != 0: the image must have that size.
// false: `file` is not such an image.
bool pgm_plane(const std::string& file, uint32_t want_nx, uint32_t want_ny, uint32_t& nx, uint32_t& ny, std::vector<uint8_t>& plane);

}  // namespace mola_hip
