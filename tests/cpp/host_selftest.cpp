// host_selftest.cpp — the CPU-side C++ (hand-rolled YAML / .obj parsers, PNG writer, scene assembly, the threaded BVH
// builder) exercised in one process so that it can run under AddressSanitizer + UBSan and under ThreadSanitizer
// (`make -C tests/cpp asan tsan`; GPU sanitizers are not available on this pool, and this code needs no GPU).
// Inputs: the two shipped scenes with a generated .obj, a set of malformed YAML / .obj texts that must be rejected
// with rbrt::Error (the reference panics there: blueprints.rs:80,87, mesh.rs:89) and never crash, and meshes large
// enough to take the builder's multi-threaded path (bvh.cpp splice).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <set>
#include <string>
#include <vector>

#include <atomic>
#include <chrono>
#include <thread>
#include <cstring>
#include "../../rbrt_amd/csrc/bvh.h"
#include "../../rbrt_amd/host/checkpoint.hpp"
#include "../../rbrt_amd/host/cli.hpp"
#include "../../rbrt_amd/host/rbrt.hpp"
#include "../../rbrt_amd/host/yaml_lite.hpp"

static int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

static std::string slurp(const std::string& p) {
    std::ifstream in(p);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static void write_obj(const std::string& path, int n_tris, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-0.1f, 0.1f);
    std::ofstream o(path);
    for (int i = 0; i < n_tris; ++i) {
        const float cx = u(rng), cy = u(rng), cz = u(rng);
        for (int k = 0; k < 3; ++k) o << "v " << cx + 0.01f * u(rng) << " " << cy + 0.01f * u(rng) << " " << cz + 0.01f * u(rng) << "\n";
    }
    for (int i = 0; i < n_tris; ++i) {
        if (i % 3 == 0)
            o << "f " << 3 * i + 1 << " " << 3 * i + 2 << " " << 3 * i + 3 << "\n";
        else if (i % 3 == 1)
            o << "f " << 3 * i + 1 << "/1/1 " << 3 * i + 2 << "//2 " << 3 * i + 3 << "/3\n";
        else
            o << "f " << -(3 * (n_tris - i)) << " " << -(3 * (n_tris - i)) + 1 << " " << -(3 * (n_tris - i)) + 2 << "\n";
    }
}

// One JSON string starting behind its opening quote; leaves `i` behind the closing one. (tests/golden/yaml_corpus.json is
// written with ensure_ascii: everything outside ASCII is a \u escape, surrogate pairs included.)
static std::string json_string(const std::string& j, size_t& i) {
    std::string out;
    auto utf8 = [&](uint32_t cp) {
        if (cp < 0x80) out += char(cp);
        else if (cp < 0x800) out += char(0xC0 | (cp >> 6)), out += char(0x80 | (cp & 0x3F));
        else if (cp < 0x10000) out += char(0xE0 | (cp >> 12)), out += char(0x80 | ((cp >> 6) & 0x3F)), out += char(0x80 | (cp & 0x3F));
        else out += char(0xF0 | (cp >> 18)), out += char(0x80 | ((cp >> 12) & 0x3F)), out += char(0x80 | ((cp >> 6) & 0x3F)), out += char(0x80 | (cp & 0x3F));
    };
    while (i < j.size() && j[i] != '"') {
        if (j[i] != '\\') {
            out += j[i++];
            continue;
        }
        const char e = j[i + 1];
        i += 2;
        if (e == 'u') {
            uint32_t cp = uint32_t(std::stoul(j.substr(i, 4), nullptr, 16));
            i += 4;
            if (cp >= 0xD800 && cp < 0xDC00 && j.compare(i, 2, "\\u") == 0) {
                cp = 0x10000 + ((cp - 0xD800) << 10) + (uint32_t(std::stoul(j.substr(i + 2, 4), nullptr, 16)) - 0xDC00);
                i += 6;
            }
            utf8(cp);
        } else {
            out += e == 'n' ? '\n' : e == 't' ? '\t' : e == 'r' ? '\r' : e == 'b' ? '\b' : e == 'f' ? '\f' : e;
        }
    }
    ++i;
    return out;
}

template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const rbrt::Error&) {
        return true;
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

static void check_bvh(const rbrt_mesh_t& m) {
    rbrt::BvhBuildResult r = rbrt::build_bvh(m);
    std::vector<int> seen(m.n_total, 0);
    size_t leaves = 0;
    for (const rbrt::BvhNode4& nd : r.nodes)
        for (int c = 0; c < 4; ++c) {
            const int32_t ch = nd.child[c];
            if (ch == rbrt::kNoChild || ch >= 0) continue;
            const uint32_t leaf = uint32_t(~ch), first = leaf >> rbrt::kLeafBits, cnt = (leaf & uint32_t(rbrt::kLeafMax - 1)) + 1u;
            CHECK(first + cnt <= r.tris.size());
            ++leaves;
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t idx = r.tris[first + k].index;
                if (idx != 0xFFFFFFFFu) {
                    CHECK(idx < m.n_total);
                    if (idx < m.n_total) ++seen[idx];
                }
            }
        }
    const uint32_t n_tested = (m.n_total / 8u) * 8u;
    // (a triangle cut by spatial splits is referenced from several leaves; one that the scan cannot return, from none)
    for (uint32_t i = 0; i < m.n_total; ++i) CHECK((i < n_tested && !m.is_padding[i]) ? seen[i] >= 1 : seen[i] == 0);
    CHECK(r.tris.size() <= rbrt::bvh_record_capacity(m.n_total));
    CHECK(r.max_depth <= uint32_t(rbrt::kMaxBvhDepth));
    CHECK(leaves == r.n_leaves || r.n_indexed <= uint32_t(rbrt::kLeafMax));
}

// The fixed scene of the checkpoint-fingerprint cases: one sphere, one from_triangles mesh, a camera from literal arguments; each
// feature on request.
struct FingerprintCase {
    rbrt::Camera cam;
    rbrt::Scene scene;
    rbrt_render_opts_t opts;
};
static FingerprintCase fingerprint_case(bool smooth, bool background, bool lens, bool env) {
    using rbrt::Vec3;
    FingerprintCase c{rbrt::Camera::create(Vec3(0.5f, 1.0f, 2.0f), Vec3(0.0f, -0.25f, -1.0f), Vec3(0.0f, 1.0f, 0.0f), 48, 64, 35.0f), rbrt::Scene(),
                      rbrt_render_opts_t()};
    std::memset(&c.opts, 0, sizeof(c.opts));
    if (lens) c.cam.set_lens(12.5f, 4.0f), c.opts.flags |= RBRT_FLAG_THIN_LENS;
    if (background) c.opts.flags |= RBRT_FLAG_CONSTANT_BACKGROUND, c.opts.bg[0] = 0.25f, c.opts.bg[1] = 0.5f, c.opts.bg[2] = 0.125f;
    c.scene.elements.push_back(rbrt::Sphere{Vec3(0.5f, -1.0f, -4.0f), 1.25f, rbrt::Material::metal(Vec3(0.75f, 0.5f, 0.25f), 0.125f)});
    const std::vector<std::array<Vec3, 3>> tris = {{Vec3(0, 0, -3), Vec3(1, 0, -3), Vec3(0, 1, -3)},
                                                   {Vec3(1, 0, -3), Vec3(1, 1, -3.5f), Vec3(0, 1, -3)},
                                                   {Vec3(-1, 0, -2), Vec3(0, 0, -3), Vec3(0, 1, -3)}};
    const std::vector<std::array<Vec3, 3>> normals = {{Vec3(0, 0, 1), Vec3(0.6f, 0, 0.8f), Vec3(0, 0.6f, 0.8f)},
                                                      {Vec3(0.6f, 0, 0.8f), Vec3(0, 1, 0), Vec3(0, 0.6f, 0.8f)},
                                                      {Vec3(-0.8f, 0, 0.6f), Vec3(0, 0, 1), Vec3(0, 0.6f, 0.8f)}};
    c.scene.triangle_meshes.push_back(
        rbrt::TriangleMesh::from_triangles(tris, rbrt::Material::lambertian(Vec3(0.5f, 0.25f, 0.75f)), smooth ? &normals : nullptr));
    if (env) {
        c.scene.environment.n = 2;
        for (int i = 0; i < 27; ++i) c.scene.environment.nodes.push_back(0.125f * float(i) + 0.5f);
    }
    return c;
}

static uint64_t fingerprint_of(bool smooth, bool background, bool lens, bool env, const std::string& path = "x.ckpt") {
    const FingerprintCase c = fingerprint_case(smooth, background, lens, env);
    const rbrt::Scene::AbiView v = c.scene.to_abi();
    return rbrt::checkpoint_fingerprint(path, c.cam.to_abi_lens(), c.opts, v.scene, v.shading_ptr(), c.scene.environment);
}

// The checkpoint file (rbrt_amd/host/checkpoint.cpp): a round trip, everything that must be refused, and the fingerprints.
static void check_checkpoint(const std::string& tmp) {
    const std::string path = tmp + "/selftest.ckpt";
    const rbrt::CheckpointHeader want = rbrt::checkpoint_header(136, 100, 10, 3, 6, 0x1234567890ABCDEFull);
    const std::vector<size_t> counts = {15, 0, 7};  // ragged, one rank without a pixel
    std::vector<std::vector<float>> sums(3);
    for (size_t r = 0; r < 3; ++r)
        for (size_t i = 0; i < counts[r]; ++i) sums[r].push_back(float(r) * 100.0f + float(i) + 0.25f);
    CHECK(rbrt::write_checkpoint(path, want, 4, sums));
    CHECK(slurp(path + ".tmp").empty());  // renamed, not copied
    const std::string good = slurp(path);
    CHECK(good.size() == sizeof(rbrt::CheckpointHeader) + 3 * 8 + (15 + 0 + 7) * sizeof(float));
    {
        const rbrt::CheckpointRead r = rbrt::read_checkpoint(path, want, counts);
        CHECK(r.found && r.samples_done == 4 && r.sums == sums);
    }
    const auto starts_over = [&](const std::string& bytes, const rbrt::CheckpointHeader& w, const std::vector<size_t>& cnts, bool found = true) {
        const std::string p = tmp + "/selftest_bad.ckpt";
        std::ofstream(p, std::ios::binary).write(bytes.data(), std::streamsize(bytes.size()));
        const rbrt::CheckpointRead r = rbrt::read_checkpoint(p, w, cnts);
        bool empty = r.samples_done == 0 && r.found == found;
        for (const auto& v : r.sums) empty = empty && v.empty();
        return empty;
    };
    CHECK(!starts_over(good, want, counts));  // (the helper itself: the good bytes resume)
    {   // no file at all: nothing found, start at 0
        const rbrt::CheckpointRead r = rbrt::read_checkpoint(tmp + "/does_not_exist.ckpt", want, counts);
        CHECK(!r.found && r.samples_done == 0);
    }
    {   // a wrong magic, a change in each single header field, samples_done of 0 and of spp
        std::string b = good;
        b[7] = '2';
        CHECK(starts_over(b, want, counts));
        using H = rbrt::CheckpointHeader;
        void (*const change[6])(H&) = {[](H& w) { w.width = 137; }, [](H& w) { w.height = 101; },        [](H& w) { w.spp = 11; },
                                       [](H& w) { w.world = 2; },   [](H& w) { w.seed = 7; }, [](H& w) { w.fingerprint ^= 1ull << 63; }};
        for (const auto& f : change) {
            H w = want;
            f(w);
            CHECK(std::memcmp(&w, &want, sizeof(w)) != 0);
            CHECK(starts_over(good, w, counts));
        }
        H two = want;
        two.world = 2;
        const std::vector<size_t> counts_of_two = {15, 0};
        CHECK(starts_over(good, two, counts_of_two));
        for (uint32_t done : {0u, 10u, 11u}) {
            rbrt::CheckpointHeader h = want;
            h.samples_done = done;
            b = good;
            std::memcpy(&b[0], &h, sizeof(h));
            CHECK(starts_over(b, want, counts));
        }
    }
    // a per-rank count that differs from the expected one, in the file and in the expectation, including 2^60
    const size_t count_at[3] = {sizeof(rbrt::CheckpointHeader), sizeof(rbrt::CheckpointHeader) + 8 + 15 * 4, sizeof(rbrt::CheckpointHeader) + 16 + 15 * 4};
    for (size_t r = 0; r < 3; ++r)
        for (uint64_t cnt : {uint64_t(counts[r] + 1), uint64_t(counts[r] - 1), uint64_t(1) << 60, ~uint64_t(0)}) {
            std::string b = good;
            std::memcpy(&b[count_at[r]], &cnt, sizeof(cnt));
            CHECK(starts_over(b, want, counts));
        }
    for (const std::vector<size_t>& other : {std::vector<size_t>{15, 0, 8}, std::vector<size_t>{14, 0, 7}, std::vector<size_t>{15, 1, 7}})
        CHECK(starts_over(good, want, other));
    // truncated: at the header (nothing found), in a count, in the middle of a rank's floats, one byte short of the end
    CHECK(starts_over(good.substr(0, 0), want, counts, false));
    CHECK(starts_over(good.substr(0, sizeof(rbrt::CheckpointHeader) - 1), want, counts, false));
    CHECK(starts_over(good.substr(0, sizeof(rbrt::CheckpointHeader)), want, counts));
    CHECK(starts_over(good.substr(0, count_at[0] + 3), want, counts));
    CHECK(starts_over(good.substr(0, count_at[0] + 8 + 30), want, counts));
    CHECK(starts_over(good.substr(0, count_at[2] + 5), want, counts));
    CHECK(starts_over(good.substr(0, good.size() - 1), want, counts));
    CHECK(!rbrt::write_checkpoint("/nonexistent_dir/x.ckpt", want, 4, sums));
    // Fingerprints: the literals are what the code BEFORE checkpoint.cpp existed gave for these scenes (render.cpp's inlined
    // fingerprint, run on this scene), so a checkpoint written by an older build still resumes. Never refresh them from
    // checkpoint_fingerprint itself.
    const uint64_t fps[7] = {fingerprint_of(false, false, false, false), fingerprint_of(true, false, false, false), fingerprint_of(false, true, false, false),
                             fingerprint_of(false, false, true, false),  fingerprint_of(false, false, false, true), fingerprint_of(false, false, true, true),
                             fingerprint_of(true, true, true, true)};
    const uint64_t expect[7] = {0x82785BBCB5E4D395ull, 0xE3C6F6411327AB30ull, 0x4AA9C19C5A330C66ull, 0xF96F44E083404CEFull,
                                0x9B00D435A4E59A30ull, 0x49339898107624AEull, 0x5DE63705418334B8ull};
    for (int i = 0; i < 7; ++i) {
        CHECK(fps[i] == expect[i]);
        for (int k = 0; k < i; ++k) CHECK(fps[i] != fps[k]);
    }
    CHECK(fingerprint_of(true, true, true, true, "") == 0);  // no path, no checkpoint to match
    CHECK(fingerprint_of(false, false, false, false, "other.ckpt") == expect[0]);
}

// ---- the command line's parser and checks, in-process: the code a few argvs return and what they left in the options ----
// (every refusal also writes its line to stderr; tests/test_cli_refusals_host.py pins those texts on the binary)
struct Cli {
    CliOptions o;
    int parsed, checked = CLI_RUN;
    Cli(std::vector<std::string> args) {
        std::vector<char*> argv{const_cast<char*>("rbrt")};
        for (std::string& a : args) argv.push_back(a.data());
        rbrt::PfmImage ref;
        parsed = parse_cli(int(argv.size()), argv.data(), o);
        if (parsed == CLI_RUN) checked = check_cli(o, ref);
    }
};

static void check_cli_parser() {
    CHECK(Cli({}).parsed == CLI_RUN && Cli({}).checked == CLI_RUN && Cli({}).o.samples == 5);
    CHECK(Cli({"-h", "--bogus"}).parsed == CLI_HELP && Cli({"--bogus", "-h"}).parsed == 2 && Cli({"bogus"}).parsed == 2);
    {  // one of each reader, in both spellings
        const Cli c({"-w", "7", "--height=9", "--denoise", "--denoise-radius", "10", "--denoise-strength=1e-3", "--background", "1,0,0.5", "--gather", "rccl",
                     "--tonemap=aces", "--compare-epsilon", "0.5", "--error-map", "e.png", "--compare", "missing.pfm", "--seed", "banana", "-t", "--noisy"});
        CHECK(c.parsed == CLI_RUN && c.o.width == 7 && c.o.height == 9 && c.o.denoise && c.o.denoise_radius == 10u && c.o.denoise_strength == 1e-3f);
        CHECK(c.o.constant_background && c.o.background[2] == 0.5f && c.o.gather == "rccl" && c.o.tone_curve == RBRT_TONE_ACES && c.o.seed == 0);
        CHECK(c.o.target == "--noisy" && c.o.noisy.empty() && c.o.error_map == "e.png");
        CHECK(c.checked == 2);  // the reference cannot be read
    }
    for (const char* last : {"--samples", "-c", "--glare", "--camera-step", "--shading", "--features"}) CHECK(Cli({"--denoise", last}).parsed == 2);
    for (const char* bad : {"--width=-1", "--width=4294967296", "--width=", "--denoise-radius=11", "--frames=0", "--glare=1.5", "--glare=nan", "--adaptive=inf",
                            "--camera-step=1,2", "--camera-step=1,2,inf", "--background=-1,0,0", "--shading=round", "--features=", "--denoise=1", "--exposure=128"})
        CHECK(Cli({bad}).parsed == 2);
    CHECK(Cli({"--despike=1", "--oversubscribe=1"}).o.despike && Cli({"--despike=1", "--oversubscribe=1"}).o.oversubscribe);
    CHECK(Cli({"--exposure", "auto"}).o.exposure == 0.0f && Cli({"--exposure=-1"}).o.exposure == 0.5f && Cli({"--white", "auto", "--tonemap", "reinhard"}).o.white == 0.0f);
    CHECK(std::signbit(*Cli({"--adaptive=-0"}).o.adaptive) && !std::signbit(*Cli({"--frames=2", "--temporal-depth=-0"}).o.temporal_depth));
    // the groups: the first conflict of the chain, --samples, the first dependant; what stands between and behind them
    CHECK(Cli({"--upscale", "2"}).checked == CLI_RUN && Cli({"--upscale", "2", "--sample-map", "m.png"}).checked == 2 && Cli({"--upscale", "2", "-s", "1"}).checked == 2);
    CHECK(Cli({"--upscale-depth", "0.1"}).checked == 2 && Cli({"--guided-no-demodulation"}).checked == 2 && Cli({"--noisy", "n.png", "--despike"}).checked == CLI_RUN);
    CHECK(Cli({"--frames", "2", "--camera-step", "3e38,0,0", "--shutter", "2"}).checked == 2 && Cli({"--frames", "2", "--camera-step", "1,0,0", "--shutter", "2"}).checked == CLI_RUN);
    CHECK(Cli({"--white", "2"}).checked == 2 && Cli({"--radiance", "r.png"}).checked == 2 && Cli({"--environment", "x.pfm", "--background", "0,0,0"}).checked == 2);
}

int main(int argc, char** argv) {
    check_cli_parser();
    const std::string root = argc > 1 ? argv[1] : ".";
    const std::string tmp = argc > 2 ? argv[2] : "/tmp";
    const std::string obj = tmp + "/selftest_bunny.obj";
    write_obj(obj, 2003, 1);
    // ---- the shipped scenes, through the YAML parser, the material factory, the .obj loader, SoA conversion ----
    for (const char* name : {"scenes/example_scene.yaml", "scenes/header_card.yaml"}) {
        std::string text = slurp(root + "/" + name);
        CHECK(!text.empty());
        size_t p;
        while ((p = text.find("bunny.obj")) != std::string::npos) text.replace(p, 9, obj.substr(0, obj.size() - 4) + "_X.obj");
        while ((p = text.find("_X.obj")) != std::string::npos) text.replace(p, 6, ".obj");
        rbrt::SceneBlueprint bp = rbrt::load_blueprints_from_yaml_text(text);
        rbrt::Scene sc = rbrt::create_scene_from_scene_blueprint(bp);
        CHECK(sc.triangle_meshes.size() == 1 && sc.triangle_meshes[0].num_triangles == 2003);
        CHECK(sc.elements.size() >= 4);
        rbrt::Camera cam = rbrt::Camera::create(bp.camera_blueprint.camera_position, bp.camera_blueprint.camera_look_at,
                                                bp.camera_blueprint.camera_up, 48, 64, bp.camera_blueprint.camera_focal_length_mm);
        CHECK(cam.to_abi().img_width_pix == 64);
        const rbrt::Scene::AbiView view = sc.to_abi();
        check_bvh(view.scene.meshes[0]);
    }
    // ---- malformed YAML: an error, never a crash or an out-of-bounds read ----
    const std::string good = slurp(root + "/scenes/example_scene.yaml");
    std::vector<std::string> bad = {"", "\n\n", "camera_blueprint:", "camera_blueprint:\n  camera_position:\n    x: a\n", "sphere_blueprints: [",
                                    "mesh_blueprints: []\nsphere_blueprints: []\n", "- - -\n", ":\n:\n", "camera_blueprint: {x: 1",
                                    std::string(5000, ' ') + "x", std::string("\t\tcamera_blueprint:\n"), "a: [1, 2, 3\nb: ]"};
    for (size_t cut : {10ul, 57ul, 200ul, 333ul, 700ul, 1200ul, 1900ul}) bad.push_back(good.substr(0, std::min(cut, good.size())));
    {   // single-character corruptions of the good text
        std::mt19937 rng(7);
        for (int k = 0; k < 300; ++k) {
            std::string t = good;
            const size_t pos = rng() % t.size();
            t[pos] = " :-[]{}#x\n\t0"[rng() % 12];
            bad.push_back(t);
        }
    }
    int rejected = 0;
    for (const std::string& t : bad) {
        try {
            rbrt::SceneBlueprint bp = rbrt::load_blueprints_from_yaml_text(t);
            (void)bp;  // some corruptions are still valid scenes: fine
        } catch (const std::exception&) {
            ++rejected;
        }
    }
    CHECK(rejected >= 20);
    // ---- every text of the differential corpus (tests/test_yaml_differential.py) through the reader alone ----
    {
        const std::string j = slurp(root + "/tests/golden/yaml_corpus.json");
        const std::string cls_key = "{\"cls\":\"", text_key = "\"text\":\"";
        int n_cases = 0, n_in_refused = 0, n_table_accepted = 0;
        for (size_t at = j.find(cls_key); at != std::string::npos; at = j.find(cls_key, at)) {
            at += cls_key.size();
            const std::string cls = json_string(j, at);
            at = j.find(text_key, at);
            CHECK(at != std::string::npos);
            if (at == std::string::npos) break;
            at += text_key.size();
            const std::string text = json_string(j, at);
            ++n_cases;
            bool refused = false;
            try {
                const yaml_lite::Node n = yaml_lite::parse(text);
                (void)n;
            } catch (const std::runtime_error&) {
                refused = true;
            }
            if (cls == "in" && refused) ++n_in_refused;
            if (cls == "bad-table" && !refused) ++n_table_accepted;
        }
        CHECK(n_cases >= 500);
        CHECK(n_in_refused == 0);
        CHECK(n_table_accepted == 0);
    }
    // ---- .obj statements that must be refused (tests/test_obj_differential.py's table) ----
    {
        const char* refused_objs[] = {"v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 0 2\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -4\n",
                                      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2abc 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1x 2 3\n",
                                      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/1/1/1 2 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3.0\n",
                                      "v 1 2\n", "v 1 2 3abc\n", "v 1.0.0 2 3\n", "v 0x10 0 0\n", "v 1,5 0 0\n", "v + 0 0\n", "v +-1 0 0\n",
                                      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf /1 2 3\n", "v 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nf 1 2 3junk\r\n", "v 1e", "f 1/"};
        for (const char* t : refused_objs) {
            const std::string p = tmp + "/selftest_refused.obj";
            std::ofstream(p) << t;
            CHECK(throws([&] { (void)rbrt::load_mesh_from_file(p, rbrt::Vec3(), rbrt::Vec3(0.1f, 0.2f, 0.3f), 1.0f, true); }));
        }
    }
    // ---- malformed .obj ----
    const char* bad_objs[] = {"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nf 1 1\n", "v a b c\nv 0 0 0\nv 1 1 1\nf 1 2 3\n",
                              "f 1 2 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -4 -1 -2\n",
                              "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/ 2/ 3/\n", "v 1e999 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n"};
    int n_bad_obj = 0;
    for (const char* t : bad_objs) {
        const std::string p = tmp + "/selftest_bad.obj";
        std::ofstream(p) << t;
        if (throws([&] { (void)rbrt::load_mesh_vertices_from_file(p, rbrt::Vec3(), rbrt::Vec3(), 1.0f); })) ++n_bad_obj;
    }
    CHECK(n_bad_obj >= 5);
    CHECK(throws([&] { (void)rbrt::load_mesh_vertices_from_file(tmp + "/does_not_exist.obj", rbrt::Vec3(), rbrt::Vec3(), 1.0f); }));
    // ---- PNG ----
    {
        std::vector<uint8_t> rgb(33 * 17 * 3);
        for (size_t i = 0; i < rgb.size(); ++i) rgb[i] = uint8_t(i * 7);
        rbrt::write_png(tmp + "/selftest.png", rgb.data(), 33, 17);
        CHECK(slurp(tmp + "/selftest.png").size() > 60);
        CHECK(throws([&] { rbrt::write_png("/nonexistent_dir/x.png", rgb.data(), 33, 17); }));
    }
    // ---- every image writer (src/main.rs:86: encoder by extension), odd sizes: row padding, run lengths ----
    {
        rbrt::ImageBuffer img;
        img.width = 31, img.height = 7;
        img.rgb.resize(size_t(img.width) * img.height * 3);
        for (size_t i = 0; i < img.rgb.size(); ++i) img.rgb[i] = uint8_t(i < 200 ? 17 : i * 13);
        for (const char* ext : {"png", "ppm", "pnm", "pam", "bmp", "tga", "tif", "tiff", "qoi"}) {
            const std::string p = tmp + "/selftest_img." + ext;
            img.save(p);
            CHECK(slurp(p).size() > 40);
        }
        CHECK(throws([&] { img.save(tmp + "/selftest_img.jpg"); }));
        CHECK(throws([&] { img.save(tmp + "/selftest_img"); }));
        CHECK(throws([&] { img.save("/nonexistent_dir/x.bmp"); }));
        rbrt::ImageBuffer one;
        one.width = one.height = 1;
        one.rgb = {1, 2, 3};
        one.save(tmp + "/selftest_one.qoi");
        one.save(tmp + "/selftest_one.bmp");
    }
    // ---- the checkpoint file and its fingerprint ----
    check_checkpoint(tmp);
    // ---- BasicTriangle elements and the element order in the ABI view (triangle.rs:9-34, scene.rs:23-31) ----
    {
        rbrt::Scene sc;
        sc.elements.push_back(rbrt::Sphere{rbrt::Vec3(0, 0, -5), 1.0f, rbrt::Material::lambertian(rbrt::Vec3(0.5f, 0.5f, 0.5f))});
        sc.basic_triangles.push_back(rbrt::BasicTriangle{{rbrt::Vec3(0, 0, -3), rbrt::Vec3(1, 0, -3), rbrt::Vec3(0, 1, -3)},
                                                         rbrt::Material::metal(rbrt::Vec3(1, 1, 1), 0.1f)});
        sc.element_order = {0x80000000u, 0u};
        const rbrt::Scene::AbiView v = sc.to_abi();
        CHECK(v.scene.n_spheres == 1 && v.scene.n_triangles == 1 && v.scene.element_order && v.scene.element_order[0] == 0x80000000u);
        CHECK(v.scene.triangles[0].corners[1][0] == 1.0f && v.scene.triangles[0].mat.kind == RBRT_MAT_METAL);
        sc.element_order = {0u};
        CHECK(throws([&] { (void)sc.to_abi(); }));
    }
    // ---- the threaded BVH build (>= 32768 triangles): splice of worker subtrees ----
    {
        write_obj(tmp + "/selftest_big.obj", 70003, 3);
        rbrt::TriangleMesh tm = rbrt::TriangleMesh::create(tmp + "/selftest_big.obj", rbrt::Vec3(1, 2, 3), rbrt::Vec3(0.1f, 0.2f, 0.3f), 45.0f,
                                                          rbrt::Material::lambertian(rbrt::Vec3(0.5f, 0.5f, 0.5f)));
        const rbrt_mesh_t m = tm.to_abi();
        check_bvh(m);
        // coincident triangles: no spatial split exists
        std::vector<std::array<rbrt::Vec3, 3>> same(5000, {rbrt::Vec3(0, 0, -5), rbrt::Vec3(1, 0, -5), rbrt::Vec3(0, 1, -5)});
        rbrt::TriangleMesh tm2 = rbrt::TriangleMesh::from_triangles(same, rbrt::Material::metal(rbrt::Vec3(1, 1, 1), 0.1f));
        check_bvh(tm2.to_abi());
        // ---- a build from records in another order (what a scene handle's background thread runs), and cancelling it ----
        const rbrt::BvhBuildResult ref = rbrt::build_bvh(m);
        std::vector<rbrt::BvhTri> recs;  // (one record per triangle, in another order: what the device builder hands over)
        {
            std::vector<char> have(m.n_total, 0);
            for (auto it = ref.tris.rbegin(); it != ref.tris.rend(); ++it)
                if (it->index < m.n_total && !have[it->index]) have[it->index] = 1, recs.push_back(*it);
        }
        const rbrt::BvhBuildResult again = rbrt::build_bvh_from_records(recs.data(), recs.size());
        CHECK(again.nodes.size() == ref.nodes.size() && again.tris.size() == ref.tris.size());
        CHECK(!std::memcmp(again.nodes.data(), ref.nodes.data(), ref.nodes.size() * sizeof(rbrt::BvhNode4)));
        CHECK(!std::memcmp(again.tris.data(), ref.tris.data(), ref.tris.size() * sizeof(rbrt::BvhTri)));
        // raised at every stage of the build (before it, inside the single-threaded top, among the workers, after them):
        // the build returns, flagged, without touching anything out of bounds; an unraised flag changes nothing
        for (int delay_us : {0, 50, 200, 1000, 3000, 8000, 20000, 1000000}) {
            std::atomic<bool> cancel{false};
            rbrt::BvhBuildOptions opt;
            opt.cancel = &cancel;
            std::thread raiser([&] {
                std::this_thread::sleep_for(std::chrono::microseconds(delay_us));
                if (delay_us < 1000000) cancel.store(true);
            });
            if (delay_us == 1000000) raiser.join();  // (never raised)
            const rbrt::BvhBuildResult r = rbrt::build_bvh_from_records(recs.data(), recs.size(), opt);
            if (raiser.joinable()) raiser.join();
            if (!r.cancelled) {
                CHECK(r.nodes.size() == ref.nodes.size() && !std::memcmp(r.nodes.data(), ref.nodes.data(), ref.nodes.size() * sizeof(rbrt::BvhNode4)));
            }
            CHECK(delay_us != 0 || r.cancelled);
            CHECK(delay_us != 1000000 || !r.cancelled);
        }
    }
    if (g_failed) {
        std::fprintf(stderr, "host_selftest: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("host_selftest ok\n");
    return 0;
}
