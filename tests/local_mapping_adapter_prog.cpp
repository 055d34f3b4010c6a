// local_mapping_adapter_prog.cpp — SIVO::TriangulateMatches / SIVO::RefreshMapPoints (sivo_amd/api/orbslam/LocalMappingAdapter.h) over the
// stand-in SLAM types of local_mapping_standins.hpp; the tests compare what it writes with the Python path for the same scene.
//   prog gather IN OUT        (no device) IN as `local_mapping_prog tri` reads it.  Keyframe 1 holds match i's first keypoint as key i,
//                             keyframe 2 holds match i's second keypoint as key n - 1 - i; OUT: what gather_matches staged, in IN's layout.
//   prog triangulate IN OUT   (device) the same scene through TriangulateMatches.  OUT: count (i64), then per new point in creation order
//                             idx1, idx2 (i64), pos[3], max, min, normal[3] (f32), descriptor (32 bytes); then the slots of keyframe 1 (n bytes).
//   prog walk IN OUT          (no device) IN: a map (below).  The loop over the neighbours with a stand-in search (every free slot i of the current
//                             keyframe with i % (neighbour + 2) == 0 pairs with key i of the neighbour) and a stand-in triangulation (a pair
//                             with i % 3 == 0 becomes a point).  OUT per neighbour that was searched: neighbour (i64), F12 (9 f32), pair count
//                             (i64), the pairs (2 i64 each), new points (i64); `checks` bounds the checkNewKeyFrames() calls that say no.
//   prog create IN OUT        (device) SIVO::CreateNewMapPoints over the map.  OUT: nnew (i64), then per new point in creation order the
//                             neighbour, idx1, idx2 (i64), pos[3], max, min, normal[3] (f32), descriptor (32 bytes).
//   a map: neighbours (i64), checks (i64), state_cov (36 f64), th_confidence, th_entropy (f64), then the current keyframe and every neighbour:
//          SivoTriKeyFrame, keys (i64), per key x y (f32) octave (i32) r depth (f32) class (i32) entropy confidence (f64) node (i32) pad (i32),
//          then 32 descriptor bytes per key.
//   prog pinwalk IN OUT       (device) a map, then monocular (i64) and one f32 per neighbour (what its ComputeSceneMedianDepth returns): the loop
//                             over the neighbours with the scripted search of oracle/ref_localmapping_driver.cpp's `walk` (key i of the
//                             current keyframe pairs with key n - 1 - i of the neighbour where both slots are free and i % (neighbour + 2)
//                             == 1; during the search of the `checks`-th searched neighbour a keyframe arrives, so checkNewKeyFrames()
//                             says yes from then on) and SIVO::TriangulateMatches.  OUT in that program's layout: per searched neighbour
//                             neighbour (i64), F12 (9 f32), one byte per slot of the current keyframe (occupied at the search), pairs (i64),
//                             the pairs (2 i64 each), points (i64), per point idx1 idx2 (i64), then per point pos[3] (f32).
//   Built with -DSIVO_LM_ON_HOST, sivo_triangulate / sivo_mappoint_refresh are tests/local_mapping_host_capi.hpp (the host build of the
//   kernels' arithmetic): the modes marked (device) then need none.
//   prog refresh IN OUT       (device) IN as `local_mapping_prog refresh` reads it, then one byte per observation (1: its keyframe is bad).
//                             A point's reference keyframe is the observation whose camera centre equals the record's ref_ow.
//                             OUT per point: max, min, normal[3] (f32), descriptor (32 bytes).
#include <cstring>
#include <list>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "local_mapping_standins.hpp"
#ifdef SIVO_LM_ON_HOST
#include "local_mapping_host_capi.hpp"
#endif

static void key_descriptor(unsigned char *d, int frame, size_t i) {
    for (int b = 0; b < 32; ++b) d[b] = (unsigned char)((i * 37 + (size_t)b * 11 + (size_t)frame * 101 + ((i >> 3) * 7)) & 255);
}

struct Scene {
    LKeyFrame kf[2];                    // (one array: std::map<LKeyFrame *, size_t> walks keyframe 1 first)
    std::vector<std::pair<size_t, size_t> > pairs;
    float rf[2];
    double cov[36], th[2];
    int64_t n = 0;
    bool read(BlobReader &in) {
        SivoTriKeyFrame k[2];
        in.get(k, 2); in.get(rf, 2); in.get(cov, 36); in.get(th, 2);
        n = in.one<int64_t>();
        if (n < 0) return false;
        const std::vector<SivoTriMatch> m = in.many<SivoTriMatch>((size_t)n);
        for (int f = 0; f < 2; ++f) {
            LKeyFrame &K = kf[f];
            K.set(k[f]);
            K.mvKeysSemantic.resize((size_t)n); K.mvRight.resize((size_t)n); K.mvDepth.resize((size_t)n);
            K.mvpMapPoints.assign((size_t)n, nullptr);
            K.mDescriptorsSemantic = cv::Mat::zeros((int)(n > 0 ? n : 1), 32, CV_8UC1);
            K.numSemanticKeys = (int)n;
            for (size_t i = 0; i < (size_t)n; ++i) key_descriptor(K.mDescriptorsSemantic.ptr((int)i), f, i);
        }
        kf[0].mfScaleFactor = 1.2f;                  // (the scenes' ratio_factor is 1.5f * 1.2f)
        if (rf[0] != 1.5f * kf[0].mfScaleFactor) return false;
        std::memcpy(kf[0].cov.v, cov, sizeof cov);
        kf[0].mThConfidence = th[0]; kf[0].mThEntropyReduction = th[1];
        for (size_t i = 0; i < (size_t)n; ++i) {
            const SivoTriMatch &q = m[i];
            const size_t j = (size_t)n - 1 - i;
            kf[0].mvKeysSemantic[i] = cv::KeyPoint(q.x1, q.y1, 31.f, -1, 0, q.octave1);
            kf[0].mvRight[i] = q.r1; kf[0].mvDepth[i] = q.depth1;
            kf[1].mvKeysSemantic[j] = cv::KeyPoint(q.x2, q.y2, 31.f, -1, 0, q.octave2);
            kf[1].mvRight[j] = q.r2; kf[1].mvDepth[j] = q.depth2;
            const std::pair<int, int> p1((int)q.y1, (int)q.x1), p2((int)q.y2, (int)q.x2);
            kf[0].mEntropy.v[p1] = q.entropy1; kf[0].mConfidence.v[p1] = q.confidence1; kf[0].mClasses.v[p1] = q.class1;
            kf[1].mClasses.v[p2] = q.class2;
            pairs.push_back(std::make_pair(i, j));
        }
        return true;
    }
};

static int gather(BlobReader &in, BlobWriter &out) {
    Scene s;
    if (!s.read(in)) return 2;
    SivoTriProblem P;
    std::vector<SivoTriMatch> m;
    SIVO::local_mapping_detail::gather_matches(&s.kf[0], &s.kf[1], s.pairs, P, m);
    const float rf[2] = {P.ratio_factor, 0.f};
    const double th[2] = {P.th_confidence, P.th_entropy};
    const int64_t n = P.n;
    out.put(&P.kf1, 1); out.put(&P.kf2, 1); out.put(rf, 2); out.put(P.state_cov, 36); out.put(th, 2); out.put(&n, 1); out.put(m);
    return 0;
}

static void write_point(BlobWriter &out, const LMapPoint &p) {
    const float g[5] = {p.maxDistance, p.minDistance, p.normal.at<float>(0), p.normal.at<float>(1), p.normal.at<float>(2)};
    out.put(g, 5); out.put(p.desc.data, 32);
}

static int triangulate(BlobReader &in, BlobWriter &out) {
    Scene s;
    if (!s.read(in)) return 2;
    LMap map;
    std::list<LMapPoint *> recent;
    const int nnew = SIVO::TriangulateMatches(&s.kf[0], &s.kf[1], s.pairs, &map, recent);
    if ((size_t)nnew != map.points.size() || recent.size() != map.points.size()) return 4;
    const int64_t count = nnew;
    out.put(&count, 1);
    auto it = recent.begin();
    for (LMapPoint *p : map.points) {
        if (*it++ != p || p->ref != &s.kf[0] || p->observations.size() != 2) return 4;
        const int64_t idx[2] = {(int64_t)p->observations[&s.kf[0]], (int64_t)p->observations[&s.kf[1]]};
        if (s.kf[0].mvpMapPoints[(size_t)idx[0]] != p || s.kf[1].mvpMapPoints[(size_t)idx[1]] != p) return 4;
        out.put(idx, 2); out.put(p->pos.ptr<float>(), 3); write_point(out, *p);
    }
    std::vector<uint8_t> slots((size_t)s.n);
    for (size_t i = 0; i < slots.size(); ++i) slots[i] = s.kf[0].mvpMapPoints[i] != nullptr;
    out.put(slots);
    for (LMapPoint *p : map.points) delete p;
    return 0;
}

struct KeyRec { float x, y; int32_t octave; float r, depth; int32_t cls; double entropy, confidence; int32_t node, pad; };
static_assert(sizeof(KeyRec) == 48, "");

struct MapScene {
    std::vector<LKeyFrame> kf;          // [0] the current keyframe; one array: the observation maps walk it before the neighbours
    std::vector<LKeyFrame *> neigh;
    int64_t checks = 0;
    bool read(BlobReader &in) {
        const int64_t nk = in.one<int64_t>();
        checks = in.one<int64_t>();
        double cov[36], th[2];
        in.get(cov, 36); in.get(th, 2);
        if (nk < 0) return false;
        kf.resize((size_t)nk + 1);
        for (LKeyFrame &K : kf) {
            const SivoTriKeyFrame k = in.one<SivoTriKeyFrame>();
            const int64_t n = in.one<int64_t>();
            if (n < 0) return false;
            const std::vector<KeyRec> keys = in.many<KeyRec>((size_t)n);
            K.set(k);
            K.mfScaleFactor = 1.2f;
            K.numSemanticKeys = (int)n;
            K.mvpMapPoints.assign((size_t)n, nullptr);
            K.mDescriptorsSemantic = cv::Mat::zeros((int)(n > 0 ? n : 1), 32, CV_8UC1);
            in.get(K.mDescriptorsSemantic.data, 32 * (size_t)n);
            for (const KeyRec &q : keys) {
                const size_t i = K.mvKeysSemantic.size();
                K.mvKeysSemantic.push_back(cv::KeyPoint(q.x, q.y, 31.f, 0, 0, q.octave));
                K.mvRight.push_back(q.r); K.mvDepth.push_back(q.depth);
                const std::pair<int, int> px((int)q.y, (int)q.x);
                K.mEntropy.v[px] = q.entropy; K.mConfidence.v[px] = q.confidence; K.mClasses.v[px] = q.cls;
                K.mFeatVec[(unsigned)q.node].push_back((unsigned)i);
            }
        }
        std::memcpy(kf[0].cov.v, cov, sizeof cov);
        kf[0].mThConfidence = th[0]; kf[0].mThEntropyReduction = th[1];
        for (size_t i = 1; i < kf.size(); ++i) neigh.push_back(&kf[i]);
        return true;
    }
};

static int walk(BlobReader &in, BlobWriter &out) {
    MapScene s;
    if (!s.read(in)) return 2;
    LKeyFrame *cur = &s.kf[0];
    std::vector<LMapPoint *> made;
    int64_t calls = 0;
    SIVO::local_mapping_detail::walk_neighbours(
        cur, s.neigh, false, [&] { return ++calls > s.checks; },
        [&](LKeyFrame *pKF2, const cv::Mat &F12, std::vector<std::pair<size_t, size_t> > &pairs) {
            const int64_t k = pKF2 - &s.kf[1];
            for (size_t i = 0; i < cur->mvpMapPoints.size() && i < pKF2->mvpMapPoints.size(); ++i)
                if (!cur->mvpMapPoints[i] && !pKF2->mvpMapPoints[i] && i % (size_t)(k + 2) == 0) pairs.push_back(std::make_pair(i, i));
            out.put(&k, 1);
            for (int r = 0; r < 3; ++r) out.put(F12.ptr<float>(r), 3);
        },
        [&](LKeyFrame *pKF2, const std::vector<std::pair<size_t, size_t> > &pairs) {
            const int64_t np = (int64_t)pairs.size();
            out.put(&np, 1);
            int64_t nnew = 0;
            for (const auto &pr : pairs) {
                const int64_t ij[2] = {(int64_t)pr.first, (int64_t)pr.second};
                out.put(ij, 2);
                if (pr.first % 3) continue;
                made.push_back(new LMapPoint(cv::Mat::zeros(3, 1, CV_32F), cur, nullptr));
                cur->AddMapPoint(made.back(), pr.first); pKF2->AddMapPoint(made.back(), pr.second);
                ++nnew;
            }
            out.put(&nnew, 1);
            return (int)nnew;
        });
    for (LMapPoint *p : made) delete p;
    return 0;
}

static int pinwalk(BlobReader &in, BlobWriter &out) {
    MapScene s;
    if (!s.read(in)) return 2;
    const int64_t monocular = in.one<int64_t>();
    for (LKeyFrame *k : s.neigh) in.get(&k->medianDepth, 1);
    LKeyFrame *cur = &s.kf[0];
    const size_t n = cur->mvpMapPoints.size();
    LMap map;
    std::list<LMapPoint *> recent;
    int64_t searched = 0;
    bool arrived = false;
    SIVO::local_mapping_detail::walk_neighbours(
        cur, s.neigh, monocular != 0, [&] { return arrived; },
        [&](LKeyFrame *pKF2, const cv::Mat &F12, std::vector<std::pair<size_t, size_t> > &pairs) {
            const int64_t k = pKF2 - &s.kf[1];
            for (size_t i = 0; i < n; ++i)
                if (!cur->mvpMapPoints[i] && !pKF2->mvpMapPoints[n - 1 - i] && i % (size_t)(k + 2) == 1) pairs.push_back(std::make_pair(i, n - 1 - i));
            if (++searched == s.checks) arrived = true;
            out.put(&k, 1);
            for (int r = 0; r < 3; ++r) out.put(F12.ptr<float>(r), 3);
            std::vector<uint8_t> occupied(n);
            for (size_t i = 0; i < n; ++i) occupied[i] = cur->mvpMapPoints[i] != nullptr;
            out.put(occupied.data(), n);
        },
        [&](LKeyFrame *pKF2, const std::vector<std::pair<size_t, size_t> > &pairs) {
            const int64_t np = (int64_t)pairs.size();
            out.put(&np, 1);
            for (const auto &pr : pairs) {
                const int64_t ij[2] = {(int64_t)pr.first, (int64_t)pr.second};
                out.put(ij, 2);
            }
            const int nnew = SIVO::TriangulateMatches(cur, pKF2, pairs, &map, recent);
            std::vector<int64_t> made;
            std::vector<float> pos;
            for (const auto &pr : pairs) {
                LMapPoint *p = cur->mvpMapPoints[pr.first];
                if (!p || p != pKF2->mvpMapPoints[pr.second]) continue;
                made.push_back((int64_t)pr.first); made.push_back((int64_t)pr.second);
                for (int r = 0; r < 3; ++r) pos.push_back(p->pos.at<float>(r));
            }
            const int64_t count = (int64_t)(made.size() / 2);
            if (count != nnew) throw std::logic_error("pinwalk: the slots and TriangulateMatches' count disagree");
            out.put(&count, 1); out.put(made.data(), made.size()); out.put(pos.data(), pos.size());
            return nnew;
        });
    for (LMapPoint *p : map.points) delete p;
    return 0;
}

static int create(BlobReader &in, BlobWriter &out) {
    MapScene s;
    if (!s.read(in)) return 2;
    LMap map;
    std::list<LMapPoint *> recent;
    int64_t calls = 0;
    const int64_t nnew = SIVO::CreateNewMapPoints(&s.kf[0], s.neigh, &map, false, recent, [&] { return ++calls > s.checks; });
    if ((size_t)nnew != map.points.size() || recent.size() != map.points.size()) return 4;
    out.put(&nnew, 1);
    for (LMapPoint *p : map.points) {
        if (p->ref != &s.kf[0] || p->observations.size() != 2) return 4;
        auto other = p->observations.begin();
        if (other->first == &s.kf[0]) ++other;
        const int64_t rec[3] = {(int64_t)(other->first - &s.kf[1]), (int64_t)p->observations[&s.kf[0]], (int64_t)other->second};
        if (s.kf[0].mvpMapPoints[(size_t)rec[1]] != p || other->first->mvpMapPoints[(size_t)rec[2]] != p) return 4;
        out.put(rec, 3); out.put(p->pos.ptr<float>(), 3); write_point(out, *p);
    }
    for (LMapPoint *p : map.points) delete p;
    return 0;
}

static int refresh(BlobReader &in, BlobWriter &out) {
    const int64_t np = in.one<int64_t>();
    if (np < 0) return 2;
    const std::vector<int64_t> doff = in.many<int64_t>((size_t)np + 1), ooff = in.many<int64_t>((size_t)np + 1);
    const size_t nd = (size_t)doff[np], no = (size_t)ooff[np];
    const std::vector<uint8_t> desc = in.many<uint8_t>(32 * nd);
    const std::vector<float> ow = in.many<float>(3 * no), pt = in.many<float>(8 * (size_t)np);
    const std::vector<uint8_t> bad = in.many<uint8_t>(no);
    std::vector<LKeyFrame> kfs(no);                 // one keyframe per observation, in observation order (the map walks them by address)
    std::vector<LMapPoint *> points;
    size_t d = 0;
    for (int64_t p = 0; p < np; ++p) {
        cv::Mat pos(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) pos.at<float>(r) = pt[8 * p + r];
        LMapPoint *mp = new LMapPoint(pos, ooff[p + 1] > ooff[p] ? &kfs[(size_t)ooff[p]] : nullptr, nullptr);
        for (int64_t o = ooff[p]; o < ooff[p + 1]; ++o) {
            LKeyFrame &K = kfs[(size_t)o];
            for (int r = 0; r < 3; ++r) K.mOw.at<float>(r) = ow[3 * o + r];
            K.bad = bad[(size_t)o] != 0;
            K.mDescriptorsSemantic = cv::Mat::zeros(1, 32, CV_8UC1);
            if (!K.bad) std::memcpy(K.mDescriptorsSemantic.data, &desc[32 * d++], 32);
            K.mvKeysSemantic.assign(1, cv::KeyPoint(0, 0, 31.f, -1, 0, 0));
            K.mnScaleLevels = 2;
            K.mvScaleFactors = {pt[8 * p + 6], pt[8 * p + 7]};
            mp->AddObservation(&K, 0);
        }
        if (mp->ref) {             // the reference keyframe is the observation whose centre the record names: the first one, unless the scene walks
            mp->ref = nullptr;     // a point's observations in another order than they were added in
            for (int64_t o = ooff[p]; o < ooff[p + 1] && !mp->ref; ++o) {
                LKeyFrame &K = kfs[(size_t)o];
                if (K.mOw.at<float>(0) == pt[8 * p + 3] && K.mOw.at<float>(1) == pt[8 * p + 4] && K.mOw.at<float>(2) == pt[8 * p + 5]) mp->ref = &K;
            }
            if (!mp->ref) { delete mp; return 3; }
        }
        if ((int64_t)d != doff[p + 1]) return 3;
        points.push_back(mp);
    }
    points.insert(points.begin() + (np > 1 ? 1 : 0), nullptr);          // a null entry, skipped
    SIVO::RefreshMapPoints(points);
    for (LMapPoint *p : points)
        if (p) { write_point(out, *p); delete p; }
    return 0;
}

// exit codes beside blob_main's: 2 a count out of range, 3 a scene that contradicts itself, 4 what the adapter left contradicts its count
static int run(int argc, char **argv) {
    if (argc != 4) throw BlobUsage();
    const std::string mode = argv[1];
    BlobReader in(argv[2]);
    BlobWriter out;
    const int rc = mode == "gather" ? gather(in, out) : mode == "triangulate" ? triangulate(in, out) : mode == "refresh" ? refresh(in, out)
                   : mode == "walk" ? walk(in, out) : mode == "create" ? create(in, out) : mode == "pinwalk" ? pinwalk(in, out) : throw BlobUsage();
    out.save(argv[3]);
    return rc;
}

int main(int argc, char **argv) {
    return blob_main(argc, argv, "local_mapping_adapter_prog gather|triangulate|refresh|walk|create|pinwalk IN OUT", run);
}
