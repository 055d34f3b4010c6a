// ba_window_prog.cpp — sivo_localmap_ba_window of include/sivo_hip.h on the host build of its arithmetic (ba_window_host_capi.hpp), as a
// stand-alone program: `ba_window_prog run IN OUT` reads a little-endian blob of operations on ONE handle (tests/ba_window_cases.py writes
// it), makes the calls in order and writes what each returned.  tests/test_ba_window_host.py builds it through tests/host_prog.py, plain
// and under the sanitizers.
//
//   array, tables, create (1) and set_bad (3): as in tests/localmap_prog.cpp
//   i32 6 (window), i32 n_cand, n_kf_local_pre, n_kf_fixed_pre, n_point_pre, kf_capacity, point_capacity, i64 edge_capacity, i32 null_mask
//             (bit 0: local_kf, 1: fixed_kf, 2: local_point, 3: edge_off, 4: edge_pose, 5: edge_slot, 6: counts are passed as NULL), arrays
//             cand_kf, kf_local_pre, kf_fixed_pre, point_pre i32
//             -> i32 rc [, message], counts i64[4], local_kf i32[kf_capacity], fixed_kf i32[kf_capacity], local_point i32[point_capacity],
//             edge_off i64[point_capacity + 1], edge_pose i32[edge_capacity], edge_slot i32[edge_capacity] (everything starts at -7)
//   i32 0 ends the list.  message (only where rc != 0): i32 length, then the text of sivo_last_error().
#include <cstdint>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "ba_window_host_capi.hpp"
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
    for (;;) {
        const int32_t op = r.one<int32_t>();
        if (op == 0) break;
        if (op == 1) {
            const LmBlobTables T(r);
            const SivoLocalMapTables t = T.table();
            sivo_localmap_destroy(h);
            h = nullptr;
            put_rc(w, sivo_localmap_create(&t, &h));
        } else if (op == 3) {
            const int32_t np = r.one<int32_t>(), nk = r.one<int32_t>();
            const LmArr<int32_t> pi(r);
            const LmArr<uint8_t> pv(r);
            const LmArr<int32_t> ki(r);
            const LmArr<uint8_t> kv(r);
            put_rc(w, sivo_localmap_set_bad(h, np, pi.ptr(), pv.ptr(), nk, ki.ptr(), kv.ptr()));
        } else if (op == 6) {
            int32_t a[6];
            r.get(a, 6);
            const int64_t ecap = r.one<int64_t>();
            const int32_t mask = r.one<int32_t>();
            const LmArr<int32_t> cand(r), kl(r), kx(r), pp(r);
            auto size = [](int64_t n) { return (size_t)(n > 0 ? n : 0); };
            std::vector<int64_t> counts(4, -7), eoff(size(a[5]) + 1, -7);
            std::vector<int32_t> lkf(size(a[4]), -7), fkf(size(a[4]), -7), lpt(size(a[5]), -7), epose(size(ecap), -7), eslot(size(ecap), -7);
            put_rc(w, sivo_localmap_ba_window(h, a[0], cand.ptr(), a[1], kl.ptr(), a[2], kx.ptr(), a[3], pp.ptr(), a[4], mask & 1 ? nullptr : lkf.data(),
                                              mask & 2 ? nullptr : fkf.data(), a[5], mask & 4 ? nullptr : lpt.data(), mask & 8 ? nullptr : eoff.data(), ecap,
                                              mask & 16 ? nullptr : epose.data(), mask & 32 ? nullptr : eslot.data(), mask & 64 ? nullptr : counts.data()));
            w.put(counts); w.put(lkf); w.put(fkf); w.put(lpt); w.put(eoff); w.put(epose); w.put(eslot);
        } else {
            throw std::runtime_error("unknown operation");
        }
    }
    sivo_localmap_destroy(h);
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "ba_window_prog run IN OUT", run); }
