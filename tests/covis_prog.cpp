// covis_prog.cpp — the three covisibility entry points of include/sivo_hip.h on the host build of their arithmetic (covis_host_capi.hpp), as a
// stand-alone program: `covis_prog MODE IN OUT` reads a little-endian blob (tests/covis_cases.py writes it), makes the call and writes the
// return code and the outputs.  Built plain and with -fsanitize=address,undefined by tests/test_covis_host.py.
//
//   table : i32 n_kf, i32 n_points, i64 n_obs, obs_off i64[n_points + 1], obs_kf i32[n_obs], obs_level u8[n_obs], obs_stereo u8[n_obs],
//           point_bad u8[n_points]
//   count : table, i32 n_sets, set_off i64[n_sets + 1], set_point i32[..], set_self i32[n_sets]          -> i32 rc, counts i32[n_sets n_kf]
//   kfcull: table, i32 n_local, i32 monocular, local_kf i32[n], is_id0 u8[n], erasable u8[n], th_depth f32[n], slot_off i64[n + 1],
//           slot_point i32[..], slot_level u8[..], slot_depth f32[..]      -> i32 rc, n_mps i32[n], n_redundant i32[n], decision u8[n], bad_after u8[n_points]
//           (n_mps and n_redundant start at -7, decision at 255)
//   mpcull: i32 n, i32 monocular, i64 current, found i32[n], visible i32[n], first i64[n], n_obs i32[n], bad u8[n]           -> i32 rc, status u8[n]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "covis_host_capi.hpp"

namespace {

struct Reader {
    std::vector<char> buf;
    size_t at = 0;
    explicit Reader(const char *path) {
        FILE *f = std::fopen(path, "rb");
        if (!f) throw std::runtime_error("cannot open input");
        char tmp[1 << 16];
        size_t n;
        while ((n = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        std::fclose(f);
    }
    template <class T> T one() {
        T v;
        if (at + sizeof(T) > buf.size()) throw std::runtime_error("input too short");
        std::memcpy(&v, buf.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    template <class T> std::vector<T> many(size_t n) {
        std::vector<T> v(n);
        if (at + n * sizeof(T) > buf.size()) throw std::runtime_error("input too short");
        if (n) std::memcpy(v.data(), buf.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

struct Writer {
    std::vector<char> buf;
    template <class T> void put(const T *p, size_t n) {
        if (n) buf.insert(buf.end(), (const char *)p, (const char *)p + n * sizeof(T));
    }
    void save(const char *path) const {
        FILE *f = std::fopen(path, "wb");
        if (!f) throw std::runtime_error("cannot open output");
        if (!buf.empty() && std::fwrite(buf.data(), 1, buf.size(), f) != buf.size()) throw std::runtime_error("short write");
        std::fclose(f);
    }
};

struct Table {
    std::vector<int64_t> off;
    std::vector<int32_t> kf;
    std::vector<uint8_t> level, stereo, bad;
    SivoObsTable t;
    explicit Table(Reader &r) {
        t.n_kf = r.one<int32_t>(); t.n_points = r.one<int32_t>();
        const size_t n = (size_t)r.one<int64_t>(), P = (size_t)t.n_points;
        off = r.many<int64_t>(P + 1); kf = r.many<int32_t>(n); level = r.many<uint8_t>(n); stereo = r.many<uint8_t>(n); bad = r.many<uint8_t>(P);
        t.obs_off = off.data(); t.obs_kf = kf.data(); t.obs_level = level.data(); t.obs_stereo = stereo.data(); t.point_bad = bad.data();
    }
};

int run(const std::string &mode, const char *in, const char *out) {
    Reader r(in);
    Writer w;
    if (mode == "count") {
        Table T(r);
        const int32_t n_sets = r.one<int32_t>();
        const std::vector<int64_t> off = r.many<int64_t>((size_t)n_sets + 1);
        const std::vector<int32_t> pts = r.many<int32_t>((size_t)off[(size_t)n_sets]), self = r.many<int32_t>((size_t)n_sets);
        std::vector<int32_t> counts((size_t)n_sets * (size_t)T.t.n_kf, -7);
        const int32_t rc = sivo_covis_count(&T.t, n_sets, off.data(), pts.data(), self.data(), counts.data());
        w.put(&rc, 1); w.put(counts.data(), counts.size());
    } else if (mode == "kfcull") {
        Table T(r);
        const int32_t n = r.one<int32_t>(), mono = r.one<int32_t>();
        const size_t K = (size_t)n;
        const std::vector<int32_t> kf = r.many<int32_t>(K);
        const std::vector<uint8_t> id0 = r.many<uint8_t>(K), erasable = r.many<uint8_t>(K);
        const std::vector<float> th = r.many<float>(K);
        const std::vector<int64_t> off = r.many<int64_t>(K + 1);
        const size_t ns = (size_t)off[K];
        const std::vector<int32_t> pts = r.many<int32_t>(ns);
        const std::vector<uint8_t> lvl = r.many<uint8_t>(ns);
        const std::vector<float> dep = r.many<float>(ns);
        std::vector<int32_t> mps(K, -7), red(K, -7);
        std::vector<uint8_t> dec(K, 255), bad((size_t)T.t.n_points, 255);
        const int32_t rc = sivo_keyframe_culling(&T.t, n, kf.data(), id0.data(), erasable.data(), th.data(), off.data(), pts.data(), lvl.data(), dep.data(),
                                                 mono, mps.data(), red.data(), dec.data(), bad.data());
        w.put(&rc, 1); w.put(mps.data(), K); w.put(red.data(), K); w.put(dec.data(), K); w.put(bad.data(), bad.size());
    } else if (mode == "mpcull") {
        const int32_t n = r.one<int32_t>(), mono = r.one<int32_t>();
        const int64_t cur = r.one<int64_t>();
        const size_t N = (size_t)n;
        const std::vector<int32_t> found = r.many<int32_t>(N), visible = r.many<int32_t>(N);
        const std::vector<int64_t> first = r.many<int64_t>(N);
        const std::vector<int32_t> nobs = r.many<int32_t>(N);
        const std::vector<uint8_t> bad = r.many<uint8_t>(N);
        std::vector<uint8_t> status(N, 255);
        const int32_t rc = sivo_mappoint_culling(n, found.data(), visible.data(), first.data(), nobs.data(), bad.data(), cur, mono, status.data());
        w.put(&rc, 1); w.put(status.data(), N);
    } else {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    w.save(out);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: covis_prog count|kfcull|mpcull IN OUT\n");
        return 2;
    }
    try {
        return run(argv[1], argv[2], argv[3]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "covis_prog: %s\n", e.what());
        return 1;
    }
}
