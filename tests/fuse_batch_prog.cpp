// fuse_batch_prog.cpp — sivo_fuse_batch of include/sivo_hip.h on the host build of its arithmetic (fuse_batch_host_capi.hpp), as a
// stand-alone program: `fuse_batch_prog batch IN OUT` reads a little-endian blob (tests/fuse_batch_cases.py writes it), makes the call
// and writes the return code, the error text and the outputs.  tests/test_fuse_batch_host.py builds it through tests/host_prog.py,
// plain and under the sanitizers.
//
// Every array in the blob is an i64 length followed by that many items; the counts the call receives are the header's, so that a test
// can hand the call counts that do not fit the arrays' story.  null_mask: bit b makes the b-th pointer argument NULL, in the order of
// the prototype (kfs, cams, pos, normal, min_dist, max_dist, mp_desc, skip_point, skip_pair, best_idx, best_dist, status, u, v, ur,
// level); an empty skip array is NULL as well.
//   i32 n_kf, n_mp, f32 th, u32 null_mask, i64 pairs_out, i64 frames; per frame: i32 n, nlevels, device, has_right, is_null,
//   f32 bounds[4], x f32, y f32, octave i32, right f32, desc u8, scale f32, inv_sigma2 f32; then cams u8 (108 each), pos f32,
//   normal f32, min_dist f32, max_dist f32, mp_desc u8, skip_point u8, skip_pair u8
//   -> i32 rc, i32 len, text, best_idx i32[pairs], best_dist i32[pairs], status u8[pairs], u f32, v f32, ur f32, level i32
//      (best_idx / best_dist start at -7, status at 255, u / v / ur at -12345, level at -77)
#include <cstdint>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "fuse_batch_host_capi.hpp"

namespace {

template <class T> std::vector<T> arr(BlobReader &r) {
    const int64_t n = r.one<int64_t>();
    if (n < 0) throw std::runtime_error("negative array length");
    return r.many<T>((size_t)n);
}
template <class T> T *ptr(std::vector<T> &v, uint32_t mask, int bit) { return ((mask >> bit) & 1u) ? nullptr : v.data(); }

struct Frames {
    std::vector<sivo_mframe_t> h;
    ~Frames() { for (sivo_mframe_t f : h) sivo_mframe_destroy(f); }
};

int run(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "batch") throw BlobUsage();
    BlobReader r(argv[2]);
    BlobWriter w;
    const int32_t n_kf = r.one<int32_t>(), n_mp = r.one<int32_t>();
    const float th = r.one<float>();
    const uint32_t m = r.one<uint32_t>();
    const size_t pairs = (size_t)r.one<int64_t>();
    const int64_t frames = r.one<int64_t>();
    Frames F;
    for (int64_t k = 0; k < frames; ++k) {
        const int32_t n = r.one<int32_t>(), nlevels = r.one<int32_t>(), device = r.one<int32_t>(), has_right = r.one<int32_t>(), is_null = r.one<int32_t>();
        float b[4];
        r.get(b, 4);
        auto x = arr<float>(r), y = arr<float>(r);
        auto oct = arr<int32_t>(r);
        auto right = arr<float>(r);
        auto desc = arr<uint8_t>(r);
        auto scale = arr<float>(r), inv = arr<float>(r);
        if ((int32_t)x.size() != n || (int32_t)y.size() != n || (int32_t)oct.size() != n || desc.size() != 32 * (size_t)n ||
            (int32_t)scale.size() != nlevels || (int32_t)inv.size() != nlevels || (has_right && (int32_t)right.size() != n))
            throw std::runtime_error("a frame's arrays differ in length");
        if (is_null) { F.h.push_back(nullptr); continue; }
        std::vector<SivoKeyPoint> keys((size_t)n);
        for (int32_t i = 0; i < n; ++i) { keys[(size_t)i] = SivoKeyPoint{}; keys[(size_t)i].x = x[(size_t)i]; keys[(size_t)i].y = y[(size_t)i]; keys[(size_t)i].octave = oct[(size_t)i]; }
        sivo_mframe_t h = nullptr;
        sivo_mframe_create(keys.data(), n, has_right ? right.data() : nullptr, desc.data(), b[0], b[1], b[2], b[3], scale.data(), scale.data(),
                           inv.data(), nlevels, device, &h);
        F.h.push_back(h);
    }
    auto cam_bytes = arr<uint8_t>(r);
    if (cam_bytes.size() % sizeof(SivoFuseCamera)) throw std::runtime_error("the cameras are no whole records");
    std::vector<SivoFuseCamera> cams(cam_bytes.size() / sizeof(SivoFuseCamera));
    if (!cams.empty()) std::memcpy(cams.data(), cam_bytes.data(), cam_bytes.size());
    auto pos = arr<float>(r), normal = arr<float>(r), mn = arr<float>(r), mx = arr<float>(r);
    auto desc = arr<uint8_t>(r), skip_point = arr<uint8_t>(r), skip_pair = arr<uint8_t>(r);
    std::vector<int32_t> best(pairs, -7), dist(pairs, -7), level(pairs, -77);
    std::vector<uint8_t> status(pairs, 255);
    std::vector<float> u(pairs, -12345.0f), v(pairs, -12345.0f), ur(pairs, -12345.0f);
    const int32_t rc = sivo_fuse_batch(ptr(F.h, m, 0), ptr(cams, m, 1), n_kf, n_mp, ptr(pos, m, 2), ptr(normal, m, 3), ptr(mn, m, 4), ptr(mx, m, 5),
                                       ptr(desc, m, 6), skip_point.empty() ? nullptr : ptr(skip_point, m, 7),
                                       skip_pair.empty() ? nullptr : ptr(skip_pair, m, 8), th, ptr(best, m, 9), ptr(dist, m, 10), ptr(status, m, 11),
                                       ptr(u, m, 12), ptr(v, m, 13), ptr(ur, m, 14), ptr(level, m, 15));
    const std::string text = rc == SIVO_OK ? std::string() : std::string(sivo_last_error());
    const int32_t len = (int32_t)text.size();
    w.put(&rc, 1); w.put(&len, 1); w.put(text.data(), text.size());
    w.put(best); w.put(dist); w.put(status); w.put(u); w.put(v); w.put(ur); w.put(level);
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "fuse_batch_prog batch IN OUT", run); }
