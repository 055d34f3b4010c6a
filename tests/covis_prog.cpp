// covis_prog.cpp — the three covisibility entry points of include/sivo_hip.h on the host build of their arithmetic (covis_host_capi.hpp), as a
// stand-alone program: `covis_prog MODE IN OUT` reads a little-endian blob (tests/covis_cases.py writes it), makes the call and writes the
// return code and the outputs.  tests/test_covis_host.py builds it through tests/host_prog.py, plain and under the sanitizers.
//
//   table : i32 n_kf, i32 n_points, i64 n_obs, obs_off i64[n_points + 1], obs_kf i32[n_obs], obs_level u8[n_obs], obs_stereo u8[n_obs],
//           point_bad u8[n_points]
//   count : table, i32 n_sets, set_off i64[n_sets + 1], set_point i32[..], set_self i32[n_sets]          -> i32 rc, counts i32[n_sets n_kf]
//   kfcull: table, i32 n_local, i32 monocular, local_kf i32[n], is_id0 u8[n], erasable u8[n], th_depth f32[n], slot_off i64[n + 1],
//           slot_point i32[..], slot_level u8[..], slot_depth f32[..]      -> i32 rc, n_mps i32[n], n_redundant i32[n], decision u8[n], bad_after u8[n_points]
//           (n_mps and n_redundant start at -7, decision at 255)
//   mpcull: i32 n, i32 monocular, i64 current, found i32[n], visible i32[n], first i64[n], n_obs i32[n], bad u8[n]           -> i32 rc, status u8[n]
#include <cstdint>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "covis_host_capi.hpp"

namespace {

struct Table {
    std::vector<int64_t> off;
    std::vector<int32_t> kf;
    std::vector<uint8_t> level, stereo, bad;
    SivoObsTable t;
    explicit Table(BlobReader &r) {
        t.n_kf = r.one<int32_t>(); t.n_points = r.one<int32_t>();
        const size_t n = (size_t)r.one<int64_t>(), P = (size_t)t.n_points;
        off = r.many<int64_t>(P + 1); kf = r.many<int32_t>(n); level = r.many<uint8_t>(n); stereo = r.many<uint8_t>(n); bad = r.many<uint8_t>(P);
        t.obs_off = off.data(); t.obs_kf = kf.data(); t.obs_level = level.data(); t.obs_stereo = stereo.data(); t.point_bad = bad.data();
    }
};

int run(int argc, char **argv) {
    if (argc != 4) throw BlobUsage();
    const std::string mode = argv[1];
    BlobReader r(argv[2]);
    BlobWriter w;
    if (mode == "count") {
        Table T(r);
        const int32_t n_sets = r.one<int32_t>();
        const std::vector<int64_t> off = r.many<int64_t>((size_t)n_sets + 1);
        const std::vector<int32_t> pts = r.many<int32_t>((size_t)off[(size_t)n_sets]), self = r.many<int32_t>((size_t)n_sets);
        std::vector<int32_t> counts((size_t)n_sets * (size_t)T.t.n_kf, -7);
        const int32_t rc = sivo_covis_count(&T.t, n_sets, off.data(), pts.data(), self.data(), counts.data());
        w.put(&rc, 1); w.put(counts);
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
        w.put(&rc, 1); w.put(mps); w.put(red); w.put(dec); w.put(bad);
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
        w.put(&rc, 1); w.put(status);
    } else {
        throw BlobUsage();
    }
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "covis_prog count|kfcull|mpcull IN OUT", run); }
