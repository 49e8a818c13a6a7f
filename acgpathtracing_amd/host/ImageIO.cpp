#include "ImageIO.h"

#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace acgpt {

static std::vector<uint8_t> flip_rgb(const uint8_t* rgba, int w, int h, bool with_filter_byte)
{
    const size_t stride = (size_t)w * 3 + (with_filter_byte ? 1 : 0);
    std::vector<uint8_t> out(stride * h);
    for (int y = 0; y < h; y++) {
        const uint8_t* src = rgba + (size_t)(h - 1 - y) * w * 4;      // file row y = buffer row h-1-y
        uint8_t* dst = out.data() + stride * y;
        if (with_filter_byte) *dst++ = 0;
        for (int x = 0; x < w; x++) { dst[3 * x] = src[4 * x]; dst[3 * x + 1] = src[4 * x + 1]; dst[3 * x + 2] = src[4 * x + 2]; }
    }
    return out;
}

bool savePPM(const std::string& filename, const uint8_t* rgba, int w, int h)
{
    FILE* f = fopen(filename.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P6\n%d %d\n255\n", w, h);
    std::vector<uint8_t> rgb = flip_rgb(rgba, w, h, false);
    const bool ok = fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
    fclose(f);
    return ok;
}

static uint32_t crc32(const uint8_t* p, size_t n, uint32_t crc = 0)
{
    static uint32_t table[256];
    static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; table[i] = c; }
        init = true;
    }
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 255] ^ (crc >> 8);
    return ~crc;
}

static void put32(std::vector<uint8_t>& v, uint32_t x) { v.push_back(x >> 24); v.push_back(x >> 16); v.push_back(x >> 8); v.push_back(x); }

static void chunk(FILE* f, const char* tag, const std::vector<uint8_t>& data)
{
    std::vector<uint8_t> buf;
    put32(buf, (uint32_t)data.size());
    buf.insert(buf.end(), tag, tag + 4);
    buf.insert(buf.end(), data.begin(), data.end());
    const uint32_t c = crc32(buf.data() + 4, buf.size() - 4);
    put32(buf, c);
    fwrite(buf.data(), 1, buf.size(), f);
}

// PNG with stored (uncompressed) deflate blocks: no zlib dependency.
bool savePNG(const std::string& filename, const uint8_t* rgba, int w, int h)
{
    FILE* f = fopen(filename.c_str(), "wb");
    if (!f) return false;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    fwrite(sig, 1, 8, f);
    std::vector<uint8_t> ihdr;
    put32(ihdr, (uint32_t)w); put32(ihdr, (uint32_t)h);
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);   // 8-bit RGB
    chunk(f, "IHDR", ihdr);
    const std::vector<uint8_t> raw = flip_rgb(rgba, w, h, true);
    std::vector<uint8_t> z;
    z.push_back(0x78); z.push_back(0x01);
    uint32_t a = 1, b = 0;
    size_t pos = 0;
    while (pos < raw.size() || raw.empty()) {
        const size_t n = raw.size() - pos > 65535 ? 65535 : raw.size() - pos;
        z.push_back(pos + n >= raw.size() ? 1 : 0);
        z.push_back(n & 255); z.push_back(n >> 8); z.push_back(~n & 255); z.push_back((~n >> 8) & 255);
        z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
        for (size_t i = 0; i < n; i++) { a = (a + raw[pos + i]) % 65521u; b = (b + a) % 65521u; }
        pos += n;
        if (raw.empty()) break;
    }
    put32(z, (b << 16) | a);
    chunk(f, "IDAT", z);
    chunk(f, "IEND", std::vector<uint8_t>());
    fclose(f);
    return true;
}

bool saveImage(const std::string& filename, const uint8_t* rgba, int w, int h)
{
    const size_t n = filename.size();
    if (n >= 4 && (filename.compare(n - 4, 4, ".ppm") == 0 || filename.compare(n - 4, 4, ".PPM") == 0)) return savePPM(filename, rgba, w, h);
    if (n >= 4 && (filename.compare(n - 4, 4, ".png") == 0 || filename.compare(n - 4, 4, ".PNG") == 0)) return savePNG(filename, rgba, w, h);
    return false;
}

// ---- HDR readers (environment maps) -----------------------------------------------------------------------------------------
static bool read_all(const std::string& filename, std::vector<uint8_t>& data, std::string& err)
{
    FILE* f = fopen(filename.c_str(), "rb");
    if (!f) { err = filename + ": cannot open"; return false; }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
    fclose(f);
    return true;
}
// the next '\n'-terminated line from pos (without the '\n'); false at the end of the data
static bool next_line(const std::vector<uint8_t>& d, size_t& pos, std::string& line)
{
    if (pos >= d.size()) return false;
    const size_t b = pos;
    while (pos < d.size() && d[pos] != '\n') pos++;
    line.assign((const char*)d.data() + b, pos - b);
    if (pos < d.size()) pos++;
    return true;
}
static bool valid_dims(int w, int h) { return w >= 1 && h >= 1 && w <= 65536 && h <= 65536; }

// Radiance RGBE: value = mantissa * 2^(e - 136), e = 0 is black (Greg Ward's rgbe.c)
static float rgbe_channel(uint8_t m, uint8_t e) { return e ? std::ldexp((float)m, (int)e - 136) : 0.0f; }

bool loadHDR(const std::string& filename, std::vector<float>& rgb, int& width, int& height, std::string& err)
{
    std::vector<uint8_t> d;
    if (!read_all(filename, d, err)) return false;
    size_t pos = 0;
    std::string line;
    if (!next_line(d, pos, line) || line.compare(0, 2, "#?") != 0) { err = filename + ": not a Radiance HDR file (no #? line)"; return false; }
    for (;;) {
        if (!next_line(d, pos, line)) { err = filename + ": header without an end"; return false; }
        if (line.empty()) break;
        if (line.compare(0, 7, "FORMAT=") == 0 && line != "FORMAT=32-bit_rle_rgbe") { err = filename + ": unsupported " + line; return false; }
    }
    char ys[3] = {0}, xs[3] = {0};
    int h = 0, w = 0;
    if (!next_line(d, pos, line) || sscanf(line.c_str(), "%2s %d %2s %d", ys, &h, xs, &w) != 4 || strcmp(ys, "-Y") != 0 || strcmp(xs, "+X") != 0 || !valid_dims(w, h)) {
        err = filename + ": unsupported resolution line (only \"-Y H +X W\")"; return false;
    }
    std::vector<uint8_t> px((size_t)w * h * 4);
    for (int y = 0; y < h; y++) {
        uint8_t* row = px.data() + (size_t)y * w * 4;
        const bool rle = w >= 8 && w < 32768 && pos + 4 <= d.size() && d[pos] == 2 && d[pos + 1] == 2 && ((d[pos + 2] << 8) | d[pos + 3]) == w && !(d[pos + 2] & 0x80);
        if (!rle) {                                    // flat scanline: w RGBE quadruples
            if (pos + (size_t)w * 4 > d.size()) { err = filename + ": truncated pixel data"; return false; }
            memcpy(row, d.data() + pos, (size_t)w * 4);
            pos += (size_t)w * 4;
            continue;
        }
        pos += 4;
        for (int c = 0; c < 4; c++) {                  // each component's run-length encoded plane
            int x = 0;
            while (x < w) {
                if (pos >= d.size()) { err = filename + ": truncated run-length data"; return false; }
                int n = d[pos++];
                if (n > 128) {
                    n -= 128;
                    if (x + n > w || pos >= d.size()) { err = filename + ": bad run-length data"; return false; }
                    const uint8_t v = d[pos++];
                    for (int k = 0; k < n; k++) row[4 * (x++) + c] = v;
                } else {
                    if (n == 0 || x + n > w || pos + n > d.size()) { err = filename + ": bad run-length data"; return false; }
                    for (int k = 0; k < n; k++) row[4 * (x++) + c] = d[pos++];
                }
            }
        }
    }
    rgb.resize((size_t)w * h * 3);
    for (size_t i = 0; i < (size_t)w * h; i++)
        for (int c = 0; c < 3; c++) rgb[3 * i + c] = rgbe_channel(px[4 * i + c], px[4 * i + 3]);
    width = w; height = h;
    return true;
}

bool loadPFM(const std::string& filename, std::vector<float>& rgb, int& width, int& height, std::string& err)
{
    std::vector<uint8_t> d;
    if (!read_all(filename, d, err)) return false;
    // three whitespace-separated tokens ("PF" / "Pf", "W H", scale), then ONE whitespace byte, then the floats, bottom row first
    size_t pos = 0;
    std::string tok[4];
    for (int t = 0; t < 4; t++) {
        while (pos < d.size() && isspace(d[pos])) pos++;
        while (pos < d.size() && !isspace(d[pos])) tok[t] += (char)d[pos++];
    }
    pos++;
    const int nc = tok[0] == "PF" ? 3 : tok[0] == "Pf" ? 1 : 0;
    const int w = atoi(tok[1].c_str()), h = atoi(tok[2].c_str());
    const double scale = atof(tok[3].c_str());
    if (nc == 0 || !valid_dims(w, h) || scale == 0.0) { err = filename + ": not a PFM file"; return false; }
    const size_t n = (size_t)w * h * nc;
    if (pos + n * 4 > d.size()) { err = filename + ": truncated pixel data"; return false; }
    uint32_t one = 1; uint8_t host_le = 0; memcpy(&host_le, &one, 1);
    const bool swap = (scale < 0.0) != (host_le != 0);      // negative scale: little-endian data
    rgb.resize((size_t)w * h * 3);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) {
                const uint8_t* p = d.data() + pos + 4 * (((size_t)(h - 1 - y) * w + x) * nc + (nc == 3 ? c : 0));
                uint8_t b[4] = {p[0], p[1], p[2], p[3]};
                if (swap) { std::swap(b[0], b[3]); std::swap(b[1], b[2]); }
                float v; memcpy(&v, b, 4);
                rgb[((size_t)y * w + x) * 3 + c] = v;
            }
    width = w; height = h;
    return true;
}

bool savePFM(const std::string& filename, const float* pixels, int width, int height, int channels)
{
    if (!pixels || !valid_dims(width, height) || (channels != 3 && channels != 4)) return false;
    FILE* f = fopen(filename.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "PF\n%d %d\n-1.0\n", width, height);
    uint32_t one = 1; uint8_t host_le = 0; memcpy(&host_le, &one, 1);
    std::vector<uint8_t> row((size_t)width * 12);
    bool ok = true;
    for (int y = 0; y < height && ok; y++) {
        for (int x = 0; x < width; x++)
            for (int c = 0; c < 3; c++) {
                uint8_t* b = row.data() + ((size_t)x * 3 + c) * 4;
                memcpy(b, pixels + ((size_t)y * width + x) * channels + c, 4);
                if (!host_le) { std::swap(b[0], b[3]); std::swap(b[1], b[2]); }
            }
        ok = fwrite(row.data(), 1, row.size(), f) == row.size();
    }
    return fclose(f) == 0 && ok;
}

bool loadEnvironment(const std::string& filename, std::vector<float>& rgb, int& width, int& height, std::string& err)
{
    const size_t n = filename.size();
    if (n >= 4 && (filename.compare(n - 4, 4, ".hdr") == 0 || filename.compare(n - 4, 4, ".HDR") == 0)) return loadHDR(filename, rgb, width, height, err);
    if (n >= 4 && (filename.compare(n - 4, 4, ".pfm") == 0 || filename.compare(n - 4, 4, ".PFM") == 0)) return loadPFM(filename, rgb, width, height, err);
    err = filename + ": unknown environment map format (.hdr or .pfm)";
    return false;
}

}  // namespace acgpt
