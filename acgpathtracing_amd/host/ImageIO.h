// ImageIO.h — PPM / PNG writers with the conventions of the reference's sutil::saveImage
// (sutil/sutil.cpp:542-655): the buffer's row 0 is the BOTTOM row, files are written top-down
// (vertical flip), UNSIGNED_BYTE4 pixels are taken as already sRGB-encoded, alpha is dropped.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace acgpt {

// rgba: width*height*4 bytes, bottom-left origin.  Returns false on I/O failure or unknown suffix.
bool saveImage(const std::string& filename, const uint8_t* rgba, int width, int height);
bool savePPM(const std::string& filename, const uint8_t* rgba, int width, int height);
bool savePNG(const std::string& filename, const uint8_t* rgba, int width, int height);

// HDR readers for environment maps (pt_set_environment): Radiance .hdr (RGBE, flat or run-length encoded scanlines, "-Y H +X W"
// only) and .pfm (PF colour / Pf grey, either byte order).  rgb: height*width*3 linear floats, row 0 = the TOP row of the picture.
// false + why on a malformed or unsupported file.
bool loadHDR(const std::string& filename, std::vector<float>& rgb, int& width, int& height, std::string& err);
bool loadPFM(const std::string& filename, std::vector<float>& rgb, int& width, int& height, std::string& err);
bool loadEnvironment(const std::string& filename, std::vector<float>& rgb, int& width, int& height, std::string& err);   // by suffix

// .pfm writer (colour "PF", little-endian, scale -1.0).  pixels: height*width*channels linear floats, channels 3 or 4 (the fourth is
// dropped); row 0 of the buffer is the BOTTOM row, which is PFM's own order: no flip.  loadPFM(savePFM(x)) returns x's bits, rows
// reversed.  false on I/O failure.
bool savePFM(const std::string& filename, const float* pixels, int width, int height, int channels);

}  // namespace acgpt
