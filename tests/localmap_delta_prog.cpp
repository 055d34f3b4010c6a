// localmap_delta_prog.cpp — sivo_localmap_apply, _sizes and _export beside the other sivo_localmap_* entry points, on the host build of their
// arithmetic (localmap_delta_host_capi.hpp), as a stand-alone program: `localmap_delta_prog run IN OUT` reads a little-endian blob of
// operations on ONE handle (tests/localmap_delta_cases.py writes it), makes the calls in order and writes what each returned.
// tests/test_localmap_delta_host.py builds it through tests/host_prog.py, plain and under the sanitizers.
//
//   arrays, tables, message and the operations 1 (create), 2 (replace), 3 (set_bad) and 4 (update): as in tests/localmap_prog.cpp
//   i32 6 (apply), i32 size (0: sizeof(SivoLocalMapDelta)), n_kf, n_points, n_point_rows, n_kf_rows, arrays point_idx i32, point_obs_off i64,
//             point_obs_kf i32, point_bad u8, kf_idx i32, kf_bad u8, kf_parent i32, kf_slot_off i64, kf_slot_point i32, kf_covis_off i64,
//             kf_covis_kf i32, kf_child_off i64, kf_child_kf i32, kf_order i32                                    -> i32 rc [, message]
//   i32 7 (export) -> i32 rc of sizes [, message], i64 sizes[6], i32 rc of export [, message], then the twelve arrays of the tables in the
//             struct's order, an offset array with rows + 1 entries (a single 0 where there are no rows)
//   i32 0 ends the list.
#include <cstdint>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "localmap_delta_host_capi.hpp"
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
        } else if (op == 4) {
            int32_t a[7];
            r.get(a, 7);
            const LmArr<int32_t> fp(r), kp(r), pp(r), prev(r);
            int32_t res[4] = {-7, -7, -7, -7};
            std::vector<uint8_t> cleared((size_t)(a[0] > 0 ? a[0] : 0), 255);
            std::vector<int32_t> lkf((size_t)(a[4] > 0 ? a[4] : 0), -7), lpt((size_t)(a[5] > 0 ? a[5] : 0), -7), counts((size_t)K, -7);
            const int32_t mask = a[6];
            put_rc(w, sivo_localmap_update(h, a[0], fp.ptr(), a[1], kp.ptr(), a[2], pp.ptr(), a[3], prev.ptr(), mask & 1 ? nullptr : &res[0],
                                           mask & 2 ? nullptr : cleared.data(), a[4], mask & 4 ? nullptr : lkf.data(), &res[1], &res[2], a[5],
                                           mask & 8 ? nullptr : lpt.data(), &res[3], counts.data()));
            w.put(res, 4); w.put(cleared); w.put(lkf); w.put(lpt); w.put(counts);
        } else if (op == 6) {
            int32_t a[5];
            r.get(a, 5);
            const LmArr<int32_t> pi(r);
            const LmArr<int64_t> po(r);
            const LmArr<int32_t> pk(r);
            const LmArr<uint8_t> pb(r);
            const LmArr<int32_t> ki(r);
            const LmArr<uint8_t> kb(r);
            const LmArr<int32_t> kp(r);
            const LmArr<int64_t> so(r);
            const LmArr<int32_t> sp(r);
            const LmArr<int64_t> co(r);
            const LmArr<int32_t> ck(r);
            const LmArr<int64_t> ho(r);
            const LmArr<int32_t> hk(r), order(r);
            SivoLocalMapDelta d;
            d.size = a[0] ? (uint32_t)a[0] : (uint32_t)sizeof(SivoLocalMapDelta);
            d.n_kf = a[1]; d.n_points = a[2]; d.n_point_rows = a[3]; d.n_kf_rows = a[4];
            d.point_idx = pi.ptr(); d.point_obs_off = po.ptr(); d.point_obs_kf = pk.ptr(); d.point_bad = pb.ptr();
            d.kf_idx = ki.ptr(); d.kf_bad = kb.ptr(); d.kf_parent = kp.ptr(); d.kf_slot_off = so.ptr(); d.kf_slot_point = sp.ptr();
            d.kf_covis_off = co.ptr(); d.kf_covis_kf = ck.ptr(); d.kf_child_off = ho.ptr(); d.kf_child_kf = hk.ptr(); d.kf_order = order.ptr();
            const int32_t rc = sivo_localmap_apply(h, &d);
            if (rc == 0) K = d.n_kf;
            put_rc(w, rc);
        } else if (op == 7) {
            int64_t n[6] = {0, 0, 0, 0, 0, 0};
            put_rc(w, sivo_localmap_sizes(h, n));
            w.put(n, 6);
            std::vector<int64_t> obs_off((size_t)n[1] + 1, 0), slot_off((size_t)n[0] + 1, 0), covis_off((size_t)n[0] + 1, 0), child_off((size_t)n[0] + 1, 0);
            std::vector<int32_t> obs_kf((size_t)n[2], -7), slot_point((size_t)n[3], -7), covis_kf((size_t)n[4], -7), child_kf((size_t)n[5], -7);
            std::vector<int32_t> parent((size_t)n[0], -7), kf_order((size_t)n[0], -7);
            std::vector<uint8_t> point_bad((size_t)n[1], 255), kf_bad((size_t)n[0], 255);
            SivoLocalMapTables t;
            t.n_kf = (int32_t)n[0]; t.n_points = (int32_t)n[1];
            t.obs_off = obs_off.data(); t.obs_kf = obs_kf.data(); t.point_bad = point_bad.data(); t.kf_bad = kf_bad.data();
            t.slot_off = slot_off.data(); t.slot_point = slot_point.data(); t.covis_off = covis_off.data(); t.covis_kf = covis_kf.data();
            t.child_off = child_off.data(); t.child_kf = child_kf.data(); t.parent = parent.data(); t.kf_order = kf_order.data();
            put_rc(w, sivo_localmap_export(h, &t));
            w.put(obs_off); w.put(obs_kf); w.put(point_bad); w.put(kf_bad); w.put(slot_off); w.put(slot_point); w.put(covis_off); w.put(covis_kf);
            w.put(child_off); w.put(child_kf); w.put(parent); w.put(kf_order);
        } else {
            throw std::runtime_error("unknown operation");
        }
    }
    sivo_localmap_destroy(h);
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "localmap_delta_prog run IN OUT", run); }
