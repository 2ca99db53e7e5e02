/*
 * ImageWriter.hpp - an image of nx x ny doubles, pixel (ix, iy) at
 * ix * ny + iy, as a file: CCDImage::save, src/CCDImage.hpp:299-362. Shared
 * by the dusty mode's CCD image, the emission-line images and the sky maps
 * (nx = longitude pixels, ny = latitude pixels).
 */
#ifndef CMI_IMAGEWRITER_HPP
#define CMI_IMAGEWRITER_HPP

#include <algorithm>
#include <cmath>
#include <fstream>
#include <string>
#include <vector>

namespace cmi {

inline bool is_image_type(const std::string &type) {
  return type == "PGM" || type == "BinaryArray";
}

/* PGM (P2, 255 levels between the image's minimum and maximum, rows of
 * constant iy, unnormalised) into <name>.pgm, or the raw doubles of image x
 * normalization into <name>.dat (the extension is added unless it is there).
 * Returns the file's name. */
inline std::string write_image(std::string filename, const std::string &type,
                               const double *image, long long nx, long long ny,
                               double normalization) {
  auto ends_with = [](const std::string &s, const std::string &tail) {
    return s.size() >= tail.size() &&
           s.compare(s.size() - tail.size(), tail.size(), tail) == 0;
  };
  const size_t size = (size_t)nx * (size_t)ny;
  if (type == "PGM") {
    if (!ends_with(filename, ".pgm"))
      filename += ".pgm";
    double min_value = image[0], max_value = image[0];
    for (size_t i = 1; i < size; ++i) {
      min_value = std::min(min_value, image[i]);
      max_value = std::max(max_value, image[i]);
    }
    max_value -= min_value;
    std::ofstream file(filename);
    file << "P2\n" << nx << " " << ny << "\n" << 255 << "\n";
    for (long long iy = 0; iy < ny; ++iy) {
      for (long long ix = 0; ix < nx; ++ix) {
        unsigned long value = 0;
        if (max_value > 0.)
          value = (unsigned long)std::round(
              255 * (image[ix * ny + iy] - min_value) / max_value);
        file << (ix ? " " : "") << value;
      }
      file << "\n";
    }
  } else {
    if (!ends_with(filename, ".dat"))
      filename += ".dat";
    std::vector<double> copy(image, image + size);
    for (double &v : copy)
      v *= normalization;
    std::ofstream file(filename, std::ios::binary);
    file.write(reinterpret_cast<const char *>(copy.data()),
               copy.size() * sizeof(double));
  }
  return filename;
}

/* a cube of nchan images, [channel][ix][iy], as raw doubles into <name>.dat
 * (the extension is added unless it is there). Returns the file's name. */
inline std::string write_cube(const std::string &filename, const double *cube,
                              long long nchan, long long nx, long long ny) {
  return write_image(filename, "BinaryArray", cube, nchan * nx, ny, 1.);
}

} // namespace cmi

#endif
