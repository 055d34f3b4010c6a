// loop_correct_prog.cpp — sivo_loop_correct and sivo_gba_propagate of include/sivo_hip.h on the host build of their arithmetic
// (loop_correct_host_capi.hpp), as a stand-alone program: `loop_correct_prog MODE IN OUT` reads a little-endian blob
// (tests/loop_correct_cases.py writes it), makes the call and writes the return code, the error text and the outputs.
// tests/test_loop_correct_host.py builds it through tests/host_prog.py, plain and under the sanitizers.
//
// Every array in the blob is an i64 length followed by that many items; the counts the call receives are the header's, so that a test can
// hand the call counts that do not fit the arrays' story (negative ones).  null_mask: bit b makes the b-th pointer of the struct NULL, in
// the order of the struct's declaration.  k_out / p_out: how many keyframes / points the output arrays hold.
//   loop: i32 n_kf, cur, n_all, n_points, u32 null_mask, i64 k_out, p_out, tiw f32, twc_cur f32, scw f64, ow f32, slot_off i64,
//         slot_point i32, pos f32, skip u8, obs_off i64, obs_kf i32, ref_kf i32, level_scale f32, last_scale f32
//         -> i32 rc, i32 len, text, noncorrected f64[8 k], corrected f64[8 k], tiw_out f32[16 k], ow_out f32[3 k], corrected_by i32[p],
//            pos_out f32[3 p], normal f32[3 p], max_dist f32[p], min_dist f32[p], flags u8[p]      (numbers start at -7, flags at 255)
//   gba : i32 n_kf, n_origins, n_points, u32 null_mask, i64 k_out, p_out, origin i32, child_off i64, child_kf i32, tcw f32, tcw_gba f32,
//         in_gba u8, tcw_bef f32, pos f32, pos_gba f32, point_in_gba u8, point_bad u8, ref_kf i32
//         -> i32 rc, i32 len, text, tcw_gba f32[16 k], in_gba u8[k], tcw_bef f32[16 k], tcw_out f32[16 k], ow_out f32[3 k],
//            kf_reached u8[k], pos_out f32[3 p], point_status u8[p]                                (tcw_out .. start at -7 / 255)
// `loop_correct_prog loop_timed|gba_timed REPEATS IN OUT` makes the call REPEATS more times on the same inputs (tools/loop_correct_probe.py)
// and appends f64 the median time of a call in microseconds.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "loop_correct_host_capi.hpp"

namespace {

template <class T> std::vector<T> arr(BlobReader &r) {
    const int64_t n = r.one<int64_t>();
    if (n < 0) throw std::runtime_error("negative array length");
    return r.many<T>((size_t)n);
}
template <class T> T *ptr(std::vector<T> &v, uint32_t mask, int bit) { return (mask >> bit) & 1u ? nullptr : v.data(); }

// the median of `repeats` timed calls in microseconds; `reset` puts the in/out arrays back before each
template <class Reset, class Call> double median_us(int repeats, Reset reset, Call call) {
    std::vector<double> t;
    for (int i = 0; i < repeats; ++i) {
        reset();
        const auto t0 = std::chrono::steady_clock::now();
        call();
        t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(t.begin(), t.end());
    return t.empty() ? 0.0 : t[t.size() / 2];
}

void put_result(BlobWriter &w, int32_t rc) {
    const std::string text = rc == SIVO_OK ? std::string() : std::string(sivo_last_error());
    const int32_t len = (int32_t)text.size();
    w.put(&rc, 1); w.put(&len, 1); w.put(text.data(), text.size());
}

int run(int argc, char **argv) {
    if (argc != 4 && argc != 5) throw BlobUsage();
    std::string mode = argv[1];
    const bool timed = argc == 5;
    if (timed != (mode == "loop_timed" || mode == "gba_timed")) throw BlobUsage();
    const int repeats = timed ? std::atoi(argv[2]) : 0;
    if (timed) mode.resize(mode.size() - 6);
    BlobReader r(argv[argc - 2]);
    BlobWriter w;
    double us = 0.0;
    if (mode == "loop") {
        SivoLoopCorrect a{};
        a.n_kf = r.one<int32_t>(); a.cur = r.one<int32_t>(); a.n_all = r.one<int32_t>(); a.n_points = r.one<int32_t>();
        const uint32_t m = r.one<uint32_t>();
        const size_t K = (size_t)r.one<int64_t>(), P = (size_t)r.one<int64_t>();
        auto tiw = arr<float>(r), twc = arr<float>(r);
        auto scw = arr<double>(r);
        auto ow = arr<float>(r);
        auto slot_off = arr<int64_t>(r);
        auto slot_point = arr<int32_t>(r);
        auto pos = arr<float>(r);
        auto skip = arr<uint8_t>(r);
        auto obs_off = arr<int64_t>(r);
        auto obs_kf = arr<int32_t>(r), ref_kf = arr<int32_t>(r);
        auto level = arr<float>(r), last = arr<float>(r);
        std::vector<double> non(8 * K, -7.0), cor(8 * K, -7.0);
        std::vector<float> tiw_out(16 * K, -7.0f), ow_out(3 * K, -7.0f), pos_out(3 * P, -7.0f), normal(3 * P, -7.0f), mx(P, -7.0f), mn(P, -7.0f);
        std::vector<int32_t> by(P, -7);
        std::vector<uint8_t> flags(P, 255);
        a.tiw = ptr(tiw, m, 0); a.twc_cur = ptr(twc, m, 1); a.scw = ptr(scw, m, 2); a.ow = ptr(ow, m, 3); a.slot_off = ptr(slot_off, m, 4);
        a.slot_point = ptr(slot_point, m, 5); a.pos = ptr(pos, m, 6); a.skip = ptr(skip, m, 7); a.obs_off = ptr(obs_off, m, 8);
        a.obs_kf = ptr(obs_kf, m, 9); a.ref_kf = ptr(ref_kf, m, 10); a.level_scale = ptr(level, m, 11); a.last_scale = ptr(last, m, 12);
        a.noncorrected_siw = ptr(non, m, 13); a.corrected_siw = ptr(cor, m, 14); a.tiw_out = ptr(tiw_out, m, 15); a.ow_out = ptr(ow_out, m, 16);
        a.corrected_by = ptr(by, m, 17); a.pos_out = ptr(pos_out, m, 18); a.normal = ptr(normal, m, 19); a.max_dist = ptr(mx, m, 20);
        a.min_dist = ptr(mn, m, 21); a.flags = ptr(flags, m, 22);
        put_result(w, sivo_loop_correct(m >> 31 ? nullptr : &a));
        us = median_us(repeats, [] {}, [&] { sivo_loop_correct(&a); });
        w.put(non); w.put(cor); w.put(tiw_out); w.put(ow_out); w.put(by); w.put(pos_out); w.put(normal); w.put(mx); w.put(mn); w.put(flags);
    } else if (mode == "gba") {
        SivoGbaPropagate a{};
        a.n_kf = r.one<int32_t>(); a.n_origins = r.one<int32_t>(); a.n_points = r.one<int32_t>();
        const uint32_t m = r.one<uint32_t>();
        const size_t K = (size_t)r.one<int64_t>(), P = (size_t)r.one<int64_t>();
        auto origin = arr<int32_t>(r);
        auto child_off = arr<int64_t>(r);
        auto child_kf = arr<int32_t>(r);
        auto tcw = arr<float>(r), tcw_gba = arr<float>(r);
        auto in_gba = arr<uint8_t>(r);
        auto tcw_bef = arr<float>(r), pos = arr<float>(r), pos_gba = arr<float>(r);
        auto pin = arr<uint8_t>(r), pbad = arr<uint8_t>(r);
        auto ref_kf = arr<int32_t>(r);
        std::vector<float> tcw_out(16 * K, -7.0f), ow_out(3 * K, -7.0f), pos_out(3 * P, -7.0f);
        std::vector<uint8_t> reached(K, 255), status(P, 255);
        a.origin = ptr(origin, m, 0); a.child_off = ptr(child_off, m, 1); a.child_kf = ptr(child_kf, m, 2); a.tcw = ptr(tcw, m, 3);
        a.tcw_gba = ptr(tcw_gba, m, 4); a.in_gba = ptr(in_gba, m, 5); a.tcw_bef = ptr(tcw_bef, m, 6); a.pos = ptr(pos, m, 7);
        a.pos_gba = ptr(pos_gba, m, 8); a.point_in_gba = ptr(pin, m, 9); a.point_bad = ptr(pbad, m, 10); a.ref_kf = ptr(ref_kf, m, 11);
        a.tcw_out = ptr(tcw_out, m, 12); a.ow_out = ptr(ow_out, m, 13); a.kf_reached = ptr(reached, m, 14); a.pos_out = ptr(pos_out, m, 15);
        a.point_status = ptr(status, m, 16);
        const std::vector<float> gba0 = tcw_gba, bef0 = tcw_bef;
        const std::vector<uint8_t> in0 = in_gba;
        put_result(w, sivo_gba_propagate(m >> 31 ? nullptr : &a));
        // (assignment between vectors of one size keeps the storage: a's pointers hold; every call leaves what the first left)
        us = median_us(repeats, [&] { tcw_gba = gba0; tcw_bef = bef0; in_gba = in0; }, [&] { sivo_gba_propagate(&a); });
        tcw_gba.resize(16 * K); in_gba.resize(K); tcw_bef.resize(16 * K);
        w.put(tcw_gba); w.put(in_gba); w.put(tcw_bef); w.put(tcw_out); w.put(ow_out); w.put(reached); w.put(pos_out); w.put(status);
    } else {
        throw BlobUsage();
    }
    if (timed) w.put(&us, 1);
    w.save(argv[argc - 1]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "loop_correct_prog loop|gba IN OUT | loop_timed|gba_timed REPEATS IN OUT", run); }
