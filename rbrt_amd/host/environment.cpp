// environment.cpp — environment lighting on the host side (no counterpart in the reference): the PFM reader (and the writer
// of --radiance next to it) and the
// conversion of a latitude/longitude image into the octahedral node grid of rbrt_environment_t (include/rbrt_hip.h
// "Environment lighting"). The device looks the grid up with + - * / only; everything that needs atan2 / acos happens here,
// once, in double.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "rbrt.hpp"

namespace rbrt {
namespace {

constexpr double kPi = 3.14159265358979323846;

// One header token of a PFM file: bytes up to the next white space, which is consumed (exactly one byte of it: after the
// scale the pixel data starts right there).
bool pfm_token(const std::string& s, size_t& at, std::string& tok) {
    tok.clear();
    while (at < s.size() && tok.empty() && (s[at] == ' ' || s[at] == '\t' || s[at] == '\n' || s[at] == '\r')) ++at;  // leading space
    while (at < s.size() && !(s[at] == ' ' || s[at] == '\t' || s[at] == '\n' || s[at] == '\r')) tok += s[at++];
    if (at >= s.size() || tok.empty()) return false;
    ++at;
    return true;
}

bool parse_long(const std::string& t, long& out) {
    char* end = nullptr;
    out = std::strtol(t.c_str(), &end, 10);
    return end != t.c_str() && *end == '\0';
}

}  // namespace

PfmImage read_pfm(const std::string& path, bool any_value) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error("environment: cannot open \"" + path + "\"");
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string s = ss.str();
    const auto bad = [&](const std::string& why) { return Error("environment: \"" + path + "\" is not a colour PFM file: " + why); };
    size_t at = 0;
    std::string magic, tw, th, tscale;
    if (s.size() < 3 || !(s[0] == 'P' && (s[1] == 'F' || s[1] == 'f'))) throw bad("it does not start with PF");
    if (!pfm_token(s, at, magic)) throw bad("the header ends early");
    if (magic == "Pf") throw bad("it is a grey image (Pf); three channels (PF) are needed");
    if (magic != "PF") throw bad("it does not start with PF");
    if (!pfm_token(s, at, tw) || !pfm_token(s, at, th) || !pfm_token(s, at, tscale)) throw bad("the header ends early");
    long w = 0, h = 0;
    if (!parse_long(tw, w) || !parse_long(th, h)) throw bad("the size `" + tw + " " + th + "` is not two integers");
    if (w <= 0 || h <= 0 || w > 65536 || h > 65536) throw bad("the size " + tw + " x " + th + " is not between 1 and 65536");
    char* end = nullptr;
    const double scale = std::strtod(tscale.c_str(), &end);
    if (end == tscale.c_str() || *end != '\0' || !std::isfinite(scale) || scale == 0.0)
        throw bad("the scale `" + tscale + "` is not a finite non-zero number (its sign gives the byte order)");
    const size_t count = size_t(w) * size_t(h) * 3u;
    if (s.size() - at < count * 4u) throw bad("it is truncated: " + std::to_string(count * 4u) + " bytes of pixels expected, " + std::to_string(s.size() - at) + " present");
    if (s.size() - at > count * 4u) throw bad("it has " + std::to_string(s.size() - at - count * 4u) + " bytes after the pixels");
    const bool little = scale < 0.0;
    PfmImage img;
    img.width = uint32_t(w), img.height = uint32_t(h);
    img.rgb.resize(count);
    const unsigned char* p = reinterpret_cast<const unsigned char*>(s.data()) + at;
    for (uint32_t row = 0; row < img.height; ++row) {  // (the file's rows run bottom to top)
        const unsigned char* src = p + size_t(img.height - 1u - row) * img.width * 12u;
        float* dst = img.rgb.data() + size_t(row) * img.width * 3u;
        for (size_t k = 0; k < size_t(img.width) * 3u; ++k) {
            const unsigned char* b = src + 4u * k;
            const uint32_t bits = little ? uint32_t(b[0]) | uint32_t(b[1]) << 8 | uint32_t(b[2]) << 16 | uint32_t(b[3]) << 24
                                         : uint32_t(b[3]) | uint32_t(b[2]) << 8 | uint32_t(b[1]) << 16 | uint32_t(b[0]) << 24;
            float v;
            std::memcpy(&v, &bits, 4);
            if (!any_value && (!std::isfinite(v) || v < 0.0f))
                throw bad("the texel in row " + std::to_string(row) + " (from the top), column " + std::to_string(k / 3u) +
                          " has a component that is not finite or is negative");
            dst[k] = v;
        }
    }
    return img;
}

// The writer read_pfm(path, true) undoes bit for bit: `PF`, the size, scale -1.0 (little-endian), rows bottom to top.
void write_pfm(const std::string& path, const float* rgb, uint32_t width, uint32_t height) {
    if (width == 0u || height == 0u || width > 65536u || height > 65536u) throw Error("write_pfm: the size must be between 1 and 65536");
    std::string out = "PF\n" + std::to_string(width) + " " + std::to_string(height) + "\n-1.0\n";
    const size_t header = out.size(), row_bytes = size_t(width) * 12u;
    out.resize(header + row_bytes * height);
    unsigned char* p = reinterpret_cast<unsigned char*>(&out[header]);
    for (uint32_t row = 0; row < height; ++row) {
        const float* src = rgb + size_t(height - 1u - row) * width * 3u;
        for (size_t k = 0; k < size_t(width) * 3u; ++k) {
            uint32_t bits;
            std::memcpy(&bits, src + k, 4);
            unsigned char* b = p + size_t(row) * row_bytes + 4u * k;
            b[0] = uint8_t(bits), b[1] = uint8_t(bits >> 8), b[2] = uint8_t(bits >> 16), b[3] = uint8_t(bits >> 24);
        }
    }
    std::ofstream f(path, std::ios::binary);
    if (!f) throw Error("cannot write \"" + path + "\"");
    f.write(out.data(), std::streamsize(out.size()));
    f.close();
    if (!f) throw Error("cannot write \"" + path + "\"");
}

// Node (j, i) of an N-grid looks along the octahedral direction of (u, v) = ((2i - N) / N, (2j - N) / N) -- 2i/N - 1 with
// one rounding, so that u(N - i) = -u(i) exactly and the nodes the fold identifies compute the SAME direction -- and takes
// the bilinear sample of the latitude/longitude image there. All in double; the result is rounded to float once.
std::vector<float> environment_nodes_from_latlong(const PfmImage& img, uint32_t n, double rotation_deg, double intensity) {
    if (n == 0u || n > 4096u) throw Error("environment: resolution must be between 1 and 4096");
    if (!std::isfinite(intensity) || intensity < 0.0) throw Error("environment: intensity must be a finite number >= 0");
    if (!std::isfinite(rotation_deg)) throw Error("environment: rotation_deg must be finite");
    if (img.width == 0u || img.height == 0u || img.rgb.size() != size_t(img.width) * img.height * 3u) throw Error("environment: empty image");
    const double rotation = rotation_deg * kPi / 180.0;
    const double ws = double(img.width), hs = double(img.height), dn = double(n);
    std::vector<float> nodes(size_t(n + 1u) * (n + 1u) * 3u);
    for (uint32_t j = 0; j <= n; ++j)
        for (uint32_t i = 0; i <= n; ++i) {
            const double u = (2.0 * double(i) - dn) / dn, v = (2.0 * double(j) - dn) / dn;
            const double py = (1.0 - std::fabs(u)) - std::fabs(v);
            double px = u, pz = v;
            if (!(py >= 0.0)) {
                px = (1.0 - std::fabs(v)) * (u >= 0.0 ? 1.0 : -1.0);
                pz = (1.0 - std::fabs(u)) * (v >= 0.0 ? 1.0 : -1.0);
            }
            px += 0.0, pz += 0.0;  // (a zero is +0)
            const double len = std::sqrt((px * px + py * py) + pz * pz);
            const double dx = px / len, dy = py / len, dz = pz / len;
            const double phi = std::atan2(dx, -dz) - rotation;
            const double t = 0.5 + phi / (2.0 * kPi);
            const double u_ll = t - std::floor(t);
            const double v_ll = std::acos(dy < -1.0 ? -1.0 : dy > 1.0 ? 1.0 : dy) / kPi;
            const double sx = u_ll * ws - 0.5, sy = v_ll * hs - 0.5;
            const double x0f = std::floor(sx), y0f = std::floor(sy);
            const double fx = sx - x0f, fy = sy - y0f;
            const long wl = long(img.width), hl = long(img.height);
            const long x0 = ((long(x0f) % wl) + wl) % wl, x1 = (x0 + 1) % wl;  // columns wrap
            const long y0 = std::min(std::max(long(y0f), 0l), hl - 1), y1 = std::min(std::max(long(y0f) + 1, 0l), hl - 1);  // rows clamp
            for (int c = 0; c < 3; ++c) {
                const auto T = [&](long y, long x) { return double(img.rgb[(size_t(y) * img.width + size_t(x)) * 3u + c]); };
                const double top = T(y0, x0) + fx * (T(y0, x1) - T(y0, x0));
                const double bot = T(y1, x0) + fx * (T(y1, x1) - T(y1, x0));
                const double val = (top + fy * (bot - top)) * intensity;
                nodes[(size_t(j) * (n + 1u) + i) * 3u + c] = float(val < 0.0 ? 0.0 : val);
            }
        }
    return nodes;
}

Environment load_environment(const EnvironmentBlueprint& bp) {
    if (bp.resolution == 0u || bp.resolution > 4096u) throw Error("environment: resolution must be between 1 and 4096");
    if (!std::isfinite(bp.intensity) || bp.intensity < 0.0f) throw Error("environment: intensity must be a finite number >= 0");
    if (!std::isfinite(bp.rotation_deg)) throw Error("environment: rotation_deg must be finite");
    Environment e;
    e.file = bp.file, e.n = bp.resolution;
    e.nodes = environment_nodes_from_latlong(read_pfm(bp.file), bp.resolution, double(bp.rotation_deg), double(bp.intensity));
    for (float v : e.nodes)
        if (!std::isfinite(v)) throw Error("environment: \"" + bp.file + "\" times the intensity overflows float32");
    return e;
}

uint64_t environment_fingerprint(const Environment& e, uint64_t h) {
    if (e.n == 0u) return h;  // (a render without one keeps its checkpoints' fingerprint)
    const auto fnv = [&](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    };
    fnv("environment", 11);
    fnv(&e.n, sizeof(e.n));
    fnv(e.nodes.data(), e.nodes.size() * sizeof(float));
    return h;
}

}  // namespace rbrt
