// bow_prog.cpp — the host build of the place-recognition arithmetic (sivo_amd/csrc/bow_math.hpp, bow_voc.hpp) as a stand-alone program:
// tests/test_bow_host.py builds it through tests/host_prog.py, compares what it writes with tests/bow_restatement.py bit for bit, also
// under the sanitizers, and feeds the loader malformed files.  tools/bow_probe.py times `bench` beside the device.
//   bow_prog load <voc.txt>                         -> "k L nodes words" on stdout; exit 2 and the message on stderr when rejected
//   bow_prog transform <voc.txt> <in> <out>         in: int64 n_sets, levelsup; per set int64 n, n x 32 bytes
//                                                   out: per set int64 n, nw, nf, m; word[n] node[n] bow_words[nw] fv_nodes[nf]
//                                                        fv_off[nf + 1] fv_feat[m] (int32), bow_values[nw] (double)
//   bow_prog query <in> <out>                       in: int64 n_slots; then n_slots + 1 vectors (the last is the query): int64 n,
//                                                       n int32 words, n double values;  out: per slot int32 common, first; double score
//   bow_prog bench <k> <L> <n> <n_stored> <n_vec>   a seeded full vocabulary: median microseconds of the transform of n features and
//                                                   of the query against n_stored vectors of n_vec words
#include <chrono>
#include <cstdio>
#include <iostream>

#include "blob_io.hpp"
#include "bow_voc.hpp"

using namespace sivo;

static int run_transform(const char *voc_path, const char *in, const char *out) {
    BowVocImage img;
    bow_load_text(voc_path, img);
    BlobReader r(in);
    const int64_t n_sets = r.one<int64_t>(), levelsup = r.one<int64_t>();
    BlobWriter f;
    for (int64_t s = 0; s < n_sets; ++s) {
        const int64_t n = r.one<int64_t>();
        if (n < 0 || n > BOW_SET_CAP) throw std::runtime_error("set size out of range");
        const std::vector<uint8_t> desc = r.many<uint8_t>(32 * (size_t)n);
        BowSet o;
        bow_transform_host(img.view(), desc.data(), (int)n, (int)levelsup, o);
        const int64_t head[4] = {n, (int64_t)o.bow_words.size(), (int64_t)o.fv_nodes.size(), (int64_t)o.fv_feat.size()};
        f.put(head, 4);
        f.put(o.word); f.put(o.node); f.put(o.bow_words); f.put(o.fv_nodes); f.put(o.fv_off); f.put(o.fv_feat); f.put(o.bow_values);
    }
    f.save(out);
    return 0;
}

struct Vec { std::vector<int32_t> w; std::vector<double> v; };

static int run_query(const char *in, const char *out) {
    BlobReader r(in);
    const int64_t n_slots = r.one<int64_t>();
    std::vector<Vec> vs((size_t)n_slots + 1);
    for (Vec &x : vs) {
        const int64_t n = r.one<int64_t>();
        x.w = r.many<int32_t>((size_t)n); x.v = r.many<double>((size_t)n);
        bow_check_vector(x.w.data(), x.v.data(), (int)n, 0x7FFFFFFF);
    }
    const Vec &q = vs.back();
    BlobWriter f;
    for (int64_t s = 0; s < n_slots; ++s) {
        int32_t cf[2];
        double score;
        bow_query_host(q.w.data(), q.v.data(), (int)q.w.size(), vs[(size_t)s].w.data(), vs[(size_t)s].v.data(), (int)vs[(size_t)s].w.size(), cf[0],
                       cf[1], score);
        f.put(cf, 2);
        f.put(&score, 1);
    }
    f.save(out);
    return 0;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

template <class Fn> static void time_it(const char *name, int reps, Fn fn) {
    std::vector<double> us;
    for (int i = 0; i < reps + 3; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        fn();
        const double d = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (i >= 3) us.push_back(d);
    }
    std::sort(us.begin(), us.end());
    std::printf("{\"what\": \"%s\", \"median_us\": %.1f, \"p10_us\": %.1f, \"p90_us\": %.1f, \"reps\": %d}\n", name, us[us.size() / 2],
                us[us.size() / 10], us[us.size() * 9 / 10], reps);
}

static int run_bench(int k, int L, int n, int n_stored, int n_vec) {
    std::vector<int32_t> parent;
    std::vector<uint8_t> leaf, desc;
    std::vector<double> weight;
    std::vector<int32_t> level{0};
    for (size_t p = 0; p < level.size(); ++p) {                       // breadth first: node p's children
        if (level[p] == L) continue;
        for (int c = 0; c < k; ++c) {
            parent.push_back((int32_t)p);
            level.push_back(level[p] + 1);
            leaf.push_back(level[p] + 1 == L);
            for (int b = 0; b < 32; ++b) desc.push_back((uint8_t)rnd());
            weight.push_back(level[p] + 1 == L ? 0.5 + (rnd() & 1023) / 256.0 : 0.0);
        }
    }
    BowVocImage img;
    bow_build_image(k, L, (int64_t)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data(), img);
    std::vector<uint8_t> f(32 * (size_t)n);
    for (uint8_t &b : f) b = (uint8_t)rnd();
    BowSet o;
    time_it("host_transform", 50, [&] { bow_transform_host(img.view(), f.data(), n, 4, o); });
    std::vector<Vec> vs((size_t)n_stored + 1);
    for (Vec &x : vs) {
        const int stride = std::max(1, img.n_words / n_vec);
        for (int i = 0; i < n_vec; ++i) {
            x.w.push_back(i * stride + (i % 3 == 0 ? 0 : (int)(rnd() % (uint32_t)stride)));      // a third of the words shared by all
            x.v.push_back(1.0 / n_vec);
        }
    }
    std::vector<double> sc((size_t)n_stored);
    time_it("host_query", 50, [&] {
        for (int s = 0; s < n_stored; ++s) {
            int32_t c, fw;
            bow_query_host(vs.back().w.data(), vs.back().v.data(), n_vec, vs[(size_t)s].w.data(), vs[(size_t)s].v.data(), n_vec, c, fw, sc[(size_t)s]);
        }
    });
    return o.word.size() == (size_t)n ? 0 : 1;
}

static int run(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "load" && argc == 3) {
        BowVocImage img;
        try {
            bow_load_text(argv[2], img);
        } catch (const std::invalid_argument &e) {            // a rejected file: the loader's message and 2, which the test asserts
            std::cerr << e.what() << "\n";
            return 2;
        }
        std::printf("%d %d %d %d\n", img.k, img.L, img.n_nodes(), img.n_words);
        return 0;
    }
    if (mode == "transform" && argc == 5) return run_transform(argv[2], argv[3], argv[4]);
    if (mode == "query" && argc == 4) return run_query(argv[2], argv[3]);
    if (mode == "bench" && argc == 7) return run_bench(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]));
    throw BlobUsage();
}

int main(int argc, char **argv) { return blob_main(argc, argv, "bow_prog load|transform|query|bench ...", run); }
