// localmap_track_prog.cpp — the resident attribute store and sivo_localmap_search_local_points of include/sivo_hip.h on the host build of
// their arithmetic (localmap_track_host_capi.hpp), as a stand-alone program: `localmap_track_prog run IN OUT` reads a little-endian blob of
// operations on ONE handle and ONE frame (tests/localmap_track_cases.py writes it), makes the calls in order and writes what each
// returned.  tests/test_localmap_track_host.py builds it through tests/host_prog.py, plain and under the sanitizers.
//
//   array, tables: as tests/localmap_prog.cpp.  message (only where rc != 0): i32 length, then the text of sivo_last_error().
//   i32 1 (create) | 2 (replace), tables                                                                       -> i32 rc [, message]
//   i32 6 (set_points), i32 n_rows, arrays point_idx i32, pos, normal, min_dist, max_dist f32, desc u8, n_obs i32   -> i32 rc [, message]
//   i32 7 (get_points), i32 n_rows, i32 null_out, array point_idx i32 -> i32 rc [, message], for max(n_rows, 0) rows pos, normal (f32,
//             from -12345), min_dist, max_dist (f32, from -12345), desc (u8, from 238), n_obs (i32, from -7), is_set (u8, from 255)
//   i32 8 (append), i32 n_new: sivo_localmap_apply of a delta that appends n_new points nobody observes   -> i32 rc [, message]
//   i32 9 (frame), f32 mnMinX, mnMaxX, mnMinY, mnMaxY, i64 keys, SivoKeyPoint per key, mvRight f32 per key, descriptors 32 bytes per key, i32 levels, scale f32 per level
//   i32 11 (device), i32: the device the handle is said to be on (the frame is on device 0)
//   i32 10 (search), SivoFrustum, f32 th, nn_ratio, i32 composed, n_slots, n_kf_premarked, n_point_premarked, n_prev, n_seen, kf_capacity,
//             point_capacity, null_mask (bit 0 voted, 1 slot_cleared, 2 local_kf, 3 local_point, 4 status, 5 match, 6 frustum, 7 handle,
//             8 frame are passed as NULL), arrays frame_point, kf_premarked, point_premarked, prev_local_kf, seen_point i32.
//             composed = 0: sivo_localmap_search_local_points; 1: sivo_localmap_update, a gather of the stored rows by local_point on the
//             host, sivo_search_local_points of tests/frustum_host_capi.hpp — the pair the entry point is defined by.
//             -> i32 rc [, message], i32 voted, n_local_kf, ref_kf, n_local_points, n_to_match, n_matches (each from -7), slot_cleared
//             u8[n_slots] (from 255), local_kf i32[kf_capacity], local_point i32[point_capacity], counts i32[n_kf of the handle] (from -7),
//             status u8[point_capacity] (from 255), proj_x, proj_y, proj_xr, view_cos f32[point_capacity] (from -12345), level
//             i32[point_capacity] (from -77), match i32[keys of the frame] (from -9)
//   i32 0 ends the list.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "localmap_track_host_capi.hpp"
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

size_t pos_count(int32_t n) { return (size_t)(n > 0 ? n : 0); }

int run(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "run") throw BlobUsage();
    BlobReader r(argv[2]);
    BlobWriter w;
    sivo_localmap_t h = nullptr;
    sivo_mframe_t F = nullptr;
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
        } else if (op == 6) {
            const int32_t n = r.one<int32_t>();
            const LmArr<int32_t> idx(r);
            const LmArr<float> pos(r), normal(r), lo(r), hi(r);
            const LmArr<uint8_t> desc(r);
            const LmArr<int32_t> obs(r);
            put_rc(w, sivo_localmap_set_points(h, n, idx.ptr(), pos.ptr(), normal.ptr(), lo.ptr(), hi.ptr(), desc.ptr(), obs.ptr()));
        } else if (op == 7) {
            const int32_t n = r.one<int32_t>(), null_out = r.one<int32_t>();
            const LmArr<int32_t> idx(r);
            const size_t N = pos_count(n);
            std::vector<float> pos(3 * N, -12345.f), normal(3 * N, -12345.f), lo(N, -12345.f), hi(N, -12345.f);
            std::vector<uint8_t> desc(32 * N, 238), set(N, 255);
            std::vector<int32_t> obs(N, -7);
            put_rc(w, sivo_localmap_get_points(h, n, idx.ptr(), pos.data(), normal.data(), lo.data(), hi.data(), desc.data(), obs.data(),
                                               null_out ? nullptr : set.data()));
            w.put(pos); w.put(normal); w.put(lo); w.put(hi); w.put(desc); w.put(obs); w.put(set);
        } else if (op == 8) {
            const int32_t n_new = r.one<int32_t>();
            int64_t sizes[6] = {0, 0, 0, 0, 0, 0};
            sivo_localmap_sizes(h, sizes);
            std::vector<int32_t> idx(pos_count(n_new));
            for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int32_t)sizes[1] + (int32_t)i;
            const std::vector<int64_t> off(idx.size() + 1, 0);
            const std::vector<uint8_t> bad(idx.size() + 1, 0);
            const int32_t none = 0;
            SivoLocalMapDelta d;
            std::memset(&d, 0, sizeof d);
            d.size = sizeof d; d.n_kf = (int32_t)sizes[0]; d.n_points = (int32_t)sizes[1] + n_new; d.n_point_rows = n_new;
            d.point_idx = idx.data(); d.point_obs_off = off.data(); d.point_obs_kf = &none; d.point_bad = bad.data();
            put_rc(w, sivo_localmap_apply(h, &d));
        } else if (op == 9) {
            float bounds[4];
            r.get(bounds, 4);
            const int64_t nk = r.one<int64_t>();
            const std::vector<SivoKeyPoint> keys = r.many<SivoKeyPoint>((size_t)nk);
            const std::vector<float> right = r.many<float>((size_t)nk);
            const std::vector<uint8_t> desc = r.many<uint8_t>(32 * (size_t)nk);
            const int32_t levels = r.one<int32_t>();
            const std::vector<float> scale = r.many<float>(pos_count(levels));
            sivo_mframe_destroy(F);
            F = nullptr;
            if (sivo_mframe_create(keys.data(), (int)nk, right.data(), desc.data(), bounds[0], bounds[1], bounds[2], bounds[3], scale.data(), scale.data(), scale.data(), levels,
                                   0, &F) != SIVO_OK)
                throw std::runtime_error("sivo_mframe_create");
        } else if (op == 11) {
            localmap_track_host::map_device() = r.one<int32_t>();
        } else if (op == 10) {
            const SivoFrustum fr = r.one<SivoFrustum>();
            const float th = r.one<float>(), nn = r.one<float>();
            int32_t a[9];
            r.get(a, 9);
            const int32_t composed = a[0], S = a[1], KC = a[6], PC = a[7], mask = a[8];
            const LmArr<int32_t> fp(r), kp(r), pp(r), prev(r), seen(r);
            int32_t res[6] = {-7, -7, -7, -7, -7, -7};
            std::vector<uint8_t> cleared(pos_count(S), 255), status(pos_count(PC), 255);
            std::vector<int32_t> lkf(pos_count(KC), -7), lpt(pos_count(PC), -7), counts((size_t)K, -7), level(pos_count(PC), -77);
            std::vector<float> px(pos_count(PC), -12345.f), py(px), pxr(px), vc(px);
            std::vector<int32_t> match(F ? F->keys.size() : 0, -9);
            int32_t rc;
            if (!composed) {
                int nt = -7, nm = -7;
                rc = sivo_localmap_search_local_points(mask & 128 ? nullptr : h, mask & 256 ? nullptr : F, mask & 64 ? nullptr : &fr, S, fp.ptr(), a[2],
                                                       kp.ptr(), a[3], pp.ptr(), a[4], prev.ptr(), a[5], seen.ptr(), th, nn,
                                                       mask & 1 ? nullptr : &res[0], mask & 2 ? nullptr : cleared.data(), KC,
                                                       mask & 4 ? nullptr : lkf.data(), &res[1], &res[2], PC, mask & 8 ? nullptr : lpt.data(), &res[3],
                                                       counts.data(), mask & 16 ? nullptr : status.data(), px.data(), py.data(), pxr.data(), vc.data(),
                                                       level.data(), mask & 32 ? nullptr : match.data(), &nt, &nm);
                res[4] = nt; res[5] = nm;
            } else {
                rc = sivo_localmap_update(h, S, fp.ptr(), a[2], kp.ptr(), a[3], pp.ptr(), a[4], prev.ptr(), &res[0], cleared.data(), KC, lkf.data(),
                                          &res[1], &res[2], PC, lpt.data(), &res[3], counts.data());
                if (rc == SIVO_OK) {
                    const size_t n = (size_t)res[3], P = (size_t)h->t.n_points;
                    std::vector<int32_t> all(P);
                    for (size_t p = 0; p < P; ++p) all[p] = (int32_t)p;
                    std::vector<float> pos(3 * P + 1), normal(3 * P + 1), lo(P + 1), hi(P + 1);
                    std::vector<uint8_t> desc(32 * P + 1), set(P + 1);
                    std::vector<int32_t> obs(P + 1);
                    if (sivo_localmap_get_points(h, (int)P, all.data(), pos.data(), normal.data(), lo.data(), hi.data(), desc.data(), obs.data(),
                                                 set.data()) != SIVO_OK)
                        throw std::runtime_error("sivo_localmap_get_points");
                    std::vector<uint8_t> stamped(P + 1, 0), skip(n + 1), gdesc(32 * n + 1);
                    for (int32_t s = 0; s < S; ++s)
                        if (fp.v[(size_t)s] >= 0 && !cleared[(size_t)s]) stamped[(size_t)fp.v[(size_t)s]] = 1;
                    for (int32_t x : seen.v) stamped[(size_t)x] = 1;
                    std::vector<float> gpos(3 * n + 1), gnormal(3 * n + 1), glo(n + 1), ghi(n + 1);
                    std::vector<int32_t> gobs(n + 1), occ(match.size() + 1);
                    for (size_t i = 0; i < n; ++i) {
                        const size_t p = (size_t)lpt[i];
                        std::copy(pos.begin() + 3 * p, pos.begin() + 3 * p + 3, gpos.begin() + 3 * i);
                        std::copy(normal.begin() + 3 * p, normal.begin() + 3 * p + 3, gnormal.begin() + 3 * i);
                        std::copy(desc.begin() + 32 * p, desc.begin() + 32 * p + 32, gdesc.begin() + 32 * i);
                        glo[i] = lo[p]; ghi[i] = hi[p]; gobs[i] = obs[p]; skip[i] = stamped[p];
                    }
                    for (size_t k = 0; k < match.size(); ++k) {
                        const int32_t p = fp.v[k];
                        occ[k] = p >= 0 && !cleared[k] ? obs[(size_t)p] : -1;
                    }
                    int nt = -7, nm = -7;
                    if (sivo_search_local_points(F, &fr, (int)n, gpos.data(), gnormal.data(), glo.data(), ghi.data(), skip.data(), gdesc.data(), gobs.data(),
                                                 th, nn, occ.data(), match.data(), status.data(), px.data(), py.data(), pxr.data(), vc.data(),
                                                 level.data(), &nt, &nm) != SIVO_OK)
                        throw std::runtime_error(std::string("sivo_search_local_points: ") + frustum_host_last_error());
                    res[4] = nt; res[5] = nm;
                }
            }
            put_rc(w, rc);
            w.put(res, 6); w.put(cleared); w.put(lkf); w.put(lpt); w.put(counts); w.put(status); w.put(px); w.put(py); w.put(pxr); w.put(vc);
            w.put(level); w.put(match);
        } else {
            throw std::runtime_error("unknown operation");
        }
    }
    sivo_localmap_destroy(h);
    sivo_mframe_destroy(F);
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "localmap_track_prog run IN OUT", run); }
