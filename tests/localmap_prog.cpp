// localmap_prog.cpp — the sivo_localmap_* entry points of include/sivo_hip.h on the host build of their arithmetic (localmap_host_capi.hpp), as a
// stand-alone program: `localmap_prog run IN OUT` reads a little-endian blob of operations on ONE handle (tests/localmap_cases.py writes it),
// makes the calls in order and writes what each returned.  tests/test_localmap_host.py builds it through tests/host_prog.py, plain and
// under the sanitizers.
//
//   array   : i64 n, then n values; n = -1 stands for a NULL pointer
//   tables  : i32 n_kf, i32 n_points, arrays obs_off i64, obs_kf i32, point_bad u8, kf_bad u8, slot_off i64, slot_point i32, covis_off i64,
//             covis_kf i32, child_off i64, child_kf i32, parent i32, kf_order i32
//   i32 1 (create) | 2 (replace), tables                                                                       -> i32 rc [, message]
//   i32 3 (set_bad), i32 n_points, i32 n_kf, arrays point_idx i32, point_val u8, kf_idx i32, kf_val u8          -> i32 rc [, message]
//   i32 4 (update), i32 n_slots, n_kf_premarked, n_point_premarked, n_prev, kf_capacity, point_capacity, null_mask (bit 0: voted, 1:
//             slot_cleared, 2: local_kf, 3: local_point are passed as NULL), arrays frame_point, kf_premarked, point_premarked, prev_local_kf i32
//             -> i32 rc [, message], i32 voted, n_local_kf, ref_kf, n_local_points (each starts at -7), slot_cleared u8[n_slots] (starts at
//             255), local_kf i32[kf_capacity], local_point i32[point_capacity], counts i32[n_kf of the handle] (start at -7)
//   i32 5 (timed update), i32 repetitions, then as 4 -> i32 rc of the last run [, message], f64 median microseconds of a run, i32 voted,
//             n_local_kf, ref_kf, n_local_points of the last run (tools/localmap_probe.py: the host build beside the device)
//   i32 0 ends the list.  message (only where rc != 0): i32 length, then the text of sivo_last_error().
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "localmap_host_capi.hpp"
#include "localmap_standins.hpp"

namespace {

void put_rc(BlobWriter &w, int32_t rc) {
    w.put(&rc, 1);
    if (rc == 0) return;
    const std::string msg = sivo_last_error();
    const int32_t n = (int32_t)msg.size();
    w.put(&n, 1);
    w.put(msg.data(), msg.size());
}

int run(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "run") throw BlobUsage();
    BlobReader r(argv[2]);
    BlobWriter w;
    sivo_localmap_t h = nullptr;
    int32_t K = 0;
    for (;;) {
        const int32_t op = r.one<int32_t>();
        if (op == 0) break;
        if (op == 1 || op == 2) {
            const LmBlobTables T(r);
            const SivoLocalMapTables t = T.table();
            int32_t rc;
            if (op == 1) {
                sivo_localmap_destroy(h);
                h = nullptr;
                rc = sivo_localmap_create(&t, &h);
            } else {
                rc = sivo_localmap_replace(h, &t);
            }
            if (rc == 0) K = t.n_kf;
            put_rc(w, rc);
        } else if (op == 3) {
            const int32_t np = r.one<int32_t>(), nk = r.one<int32_t>();
            const LmArr<int32_t> pi(r);
            const LmArr<uint8_t> pv(r);
            const LmArr<int32_t> ki(r);
            const LmArr<uint8_t> kv(r);
            put_rc(w, sivo_localmap_set_bad(h, np, pi.ptr(), pv.ptr(), nk, ki.ptr(), kv.ptr()));
        } else if (op == 4 || op == 5) {
            const int32_t reps = op == 5 ? r.one<int32_t>() : 1;
            int32_t a[7];
            r.get(a, 7);
            const LmArr<int32_t> fp(r), kp(r), pp(r), prev(r);
            int32_t res[4] = {-7, -7, -7, -7};
            std::vector<uint8_t> cleared((size_t)(a[0] > 0 ? a[0] : 0), 255);
            std::vector<int32_t> lkf((size_t)(a[4] > 0 ? a[4] : 0), -7), lpt((size_t)(a[5] > 0 ? a[5] : 0), -7), counts((size_t)K, -7);
            const int32_t mask = a[6];
            int32_t rc = 0;
            std::vector<double> us;
            for (int32_t i = 0; i < std::max(reps, 1); ++i) {
                const auto t0 = std::chrono::steady_clock::now();
                rc = sivo_localmap_update(h, a[0], fp.ptr(), a[1], kp.ptr(), a[2], pp.ptr(), a[3], prev.ptr(), mask & 1 ? nullptr : &res[0],
                                          mask & 2 ? nullptr : cleared.data(), a[4], mask & 4 ? nullptr : lkf.data(), &res[1], &res[2], a[5],
                                          mask & 8 ? nullptr : lpt.data(), &res[3], counts.data());
                us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            }
            put_rc(w, rc);
            if (op == 5) {
                std::sort(us.begin(), us.end());
                const double median = us[us.size() / 2];
                w.put(&median, 1); w.put(res, 4);
                continue;
            }
            w.put(res, 4); w.put(cleared); w.put(lkf); w.put(lpt); w.put(counts);
        } else {
            throw std::runtime_error("unknown operation");
        }
    }
    sivo_localmap_destroy(h);
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "localmap_prog run IN OUT", run); }
