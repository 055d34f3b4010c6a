// ref_localmapping_driver.cpp — feeds the reference's own LocalMapping.cc and MapPoint.cc (compiled untouched, see the Makefile) the
// problems of tests/local_mapping_pin_cases.py and writes what the reference computes.  Keyframes are the data holders of
// ref_shims_localmapping/localmapping_standins.h, built from the records the tests already use (SivoTriKeyFrame / SivoTriMatch of
// include/sivo_hip.h, the CSR arrays of sivo_mappoint_refresh); mEntropy / mConfidence / mClasses are painted at the truncated keypoint
// pixels.  Exit code 3: two keypoints painted one pixel with different values (the scene's generator has to be fixed, not this file);
// 4: a threshold or the ratio factor is not what a float member can hold; 5: the neighbour was skipped for its baseline.
//   ref_localmapping tri <in> <out>
//       in:  kf1, kf2 (SivoTriKeyFrame), float ratio_factor, pad, double state_cov[36], th_confidence, th_entropy, int64 n, n SivoTriMatch,
//            n x 32 descriptor bytes of keyframe 1, of keyframe 2, n x 3 float wP (handed to CheckSemantics directly)
//       One CreateNewMapPoints() over the one neighbour; match k names keypoint k of either keyframe.
//       out: float F12[9] as SearchForTriangulation received it; uint8 created[n]; uint8 CheckSemantics(kf1, k, wP, true)[n];
//            uint8 CheckSemantics(kf2, k, wP, false)[n]; n x 8 float: mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance; n x 32
//            bytes mDescriptor (zeros where no point was created)
//   ref_localmapping refresh <in> <out>
//       in:  int64 n, reversed; int64 desc_off[n + 1], obs_off[n + 1]; descriptors; float obs_ow[3 per observation]; n x 8 float: pos,
//            ref_ow, level_scale, last_scale; uint8 per observation: its keyframe is bad; uint8 per point: the point is bad
//       One keyframe per observation, in ONE array: its address order is the observation order, or (reversed) the opposite, which is
//       then the order std::map<KeyFrame *, size_t> walks them in.  ComputeDistinctiveDescriptors() and UpdateNormalAndDepth() per point.
//       out: per point uint8 descriptor assigned, uint8 geometry assigned; n x 32 bytes mDescriptor; n x 5 float: mNormalVector,
//            mfMinDistance, mfMaxDistance (what the point held before where the reference leaves it untouched: zeros and -1)
//   ref_localmapping walk <in> <out>
//       in:  the map of tests/test_local_mapping_host.py (map_blob): int64 neighbours, checks, double state_cov[36], th_confidence,
//            th_entropy, then the current keyframe and every neighbour: SivoTriKeyFrame, int64 keys, per key x y (f32) octave (i32) r depth
//            (f32) class (i32) entropy confidence (f64) node pad (i32), 32 descriptor bytes per key; then int64 monocular and one float
//            per neighbour: what its ComputeSceneMedianDepth returns.
//       One CreateNewMapPoints() over all neighbours.  The scripted search pairs every key i of the current keyframe with key n - 1 - i of
//       the neighbour where both slots are free at the call and i % (neighbour + 2) == 1; during the search of the `checks`-th searched
//       neighbour a keyframe arrives in the queue, so the next CheckNewKeyFrames() says yes.
//       out: per searched neighbour: int64 neighbour, float F12[9], one byte per slot of the current keyframe (1: it held a point when the
//            search was called), int64 pairs, the pairs (2 int64 each), int64 points, per point int64
//            idx1, idx2 and float mWorldPos[3]
//   ref_localmapping neighbors <in> <out>
//       in:  int64 keyframes (keyframe 0 is the current one), monocular; per keyframe: int64 bad, mnFuseTargetForKF, then its ordered
//            covisible keyframes (int64 count, indices), then its slots (int64 count, per slot the index of a map point or -1); int64
//            points; per point: int64 bad, mnFuseCandidateForKF.  Keyframe i has mnId 10 + i; a point is observed where a slot names it.
//       One SearchInNeighbors().  out (text): `T` the keyframes handed to Fuse with the current keyframe's points, in order; `C` the
//       points handed to the last Fuse call (the fuse candidates), in order; `R` the current keyframe's points that were refreshed
//       afterwards, in slot order; `U` the number of UpdateConnections() calls on the current keyframe.
//   ref_localmapping cos <in> <out>
//       in: int64 n, n x (float mb, float depth);  out: n float: the expression of LocalMapping.cc:308 as this compiler resolves it here;
//       stdout: sizeof of that expression's type
// (the C and C++ library headers LocalMapping.cc itself pulls in before its first line of code, so that `cos` and `atan2` in run_cos see
// the overloads they see there; <cmath> and <mutex> come with the forced include)
#include <unistd.h>
#include <cstdlib>
#include <cstdio>

#include "include/orbslam/LocalMapping.h"

#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>

#include "../include/sivo_hip.h"

using namespace SIVO;

struct Reader {
    std::vector<char> b;
    size_t at = 0;
    explicit Reader(const char *path) {
        std::ifstream in(path, std::ios::binary);
        if (!in) throw std::runtime_error("cannot open the input");
        b.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    }
    void get(void *dst, size_t bytes) {
        if (at + bytes > b.size()) throw std::runtime_error("input file too short");
        if (bytes) std::memcpy(dst, b.data() + at, bytes);
        at += bytes;
    }
    template <class T> std::vector<T> vec(size_t n) { std::vector<T> v(n); get(v.data(), n * sizeof(T)); return v; }
    int64_t i64() { int64_t v; get(&v, 8); return v; }
};

struct Writer {
    std::FILE *f;
    explicit Writer(const char *path) : f(std::fopen(path, "wb")) { if (!f) throw std::runtime_error("cannot open the output"); }
    ~Writer() { std::fclose(f); }
    template <class T> void put(const std::vector<T> &v) { if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f); }
};

struct Quit { int code; };

static void set_pose(KeyFrame &kf, const SivoTriKeyFrame &k) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) kf.mTcw.at<float>(r, c) = k.Rcw[3 * r + c];
        kf.mTcw.at<float>(r, 3) = k.tcw[r];
        kf.mOw.at<float>(r) = k.Ow[r];
        for (int c = 0; c < 4; ++c) kf.mTwc.at<float>(r, c) = k.Twc[4 * r + c];
    }
    kf.fx = k.fx; kf.fy = k.fy; kf.cx = k.cx; kf.cy = k.cy; kf.invfx = k.invfx; kf.invfy = k.invfy; kf.mb = k.mb; kf.mbf = k.mbf;
    kf.mK.at<float>(0, 0) = k.fx; kf.mK.at<float>(1, 1) = k.fy; kf.mK.at<float>(0, 2) = k.cx; kf.mK.at<float>(1, 2) = k.cy;
    kf.mnScaleLevels = k.nlevels;
    kf.mvScaleFactors.assign(k.scale_factors, k.scale_factors + k.nlevels);
    kf.mvLevelSigma2.assign(k.level_sigma2, k.level_sigma2 + k.nlevels);
}

static void add_key(KeyFrame &kf, float x, float y, int octave, float right, float depth, const unsigned char *desc) {
    cv::KeyPoint kp;
    kp.pt.x = x; kp.pt.y = y; kp.octave = octave;
    kf.mvKeysSemantic.push_back(kp);
    kf.mvRight.push_back(right);
    kf.mvDepth.push_back(depth);
    kf.mvpMapPoints.push_back(nullptr);
    cv::Mat row(1, 32, CV_8U);
    std::memcpy(row.ptr<unsigned char>(), desc, 32);
    kf.mDescriptorsSemantic.push_back(row);
    kf.numSemanticKeys = (int)kf.mvKeysSemantic.size();
}

static void put_point(MapPoint *p, float *geom, unsigned char *desc) {
    for (int r = 0; r < 3; ++r) { geom[r] = p->mWorldPos.at<float>(r); geom[3 + r] = p->mNormalVector.at<float>(r); }
    geom[6] = p->mfMinDistance; geom[7] = p->mfMaxDistance;
    if (!p->mDescriptor.empty()) std::memcpy(desc, p->mDescriptor.ptr<unsigned char>(), 32);
}

static int run_tri(const char *in, const char *out) {
    Reader r(in);
    SivoTriKeyFrame k1, k2;
    r.get(&k1, sizeof k1); r.get(&k2, sizeof k2);
    float ratio[2];
    double cov[36], th[2];
    r.get(ratio, sizeof ratio); r.get(cov, sizeof cov); r.get(th, sizeof th);
    const size_t n = (size_t)r.i64();
    const std::vector<SivoTriMatch> m = r.vec<SivoTriMatch>(n);
    const std::vector<unsigned char> d1 = r.vec<unsigned char>(32 * n), d2 = r.vec<unsigned char>(32 * n);
    const std::vector<float> wP = r.vec<float>(3 * n);

    std::vector<KeyFrame> pair(2);                                       // one array: std::map<KeyFrame *, size_t> walks keyframe 1 first
    KeyFrame *kf1 = &pair[0], *kf2 = &pair[1];
    set_pose(*kf1, k1); set_pose(*kf2, k2);
    kf1->mnId = 1; kf2->mnId = 0;
    kf1->mfScaleFactor = ratio[0] / 1.5f;
    kf1->mThConfidence = (float)th[0]; kf1->mThEntropyReduction = (float)th[1];
    if (1.5f * kf1->mfScaleFactor != ratio[0] || (double)kf1->mThConfidence != th[0] || (double)kf1->mThEntropyReduction != th[1]) throw Quit{4};
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) kf1->mSigma(a, b) = cov[6 * a + b];
    kf2->mSigma = kf1->mSigma;
    MatcherScript &script = MatcherScript::get();
    for (size_t k = 0; k < n; ++k) {
        add_key(*kf1, m[k].x1, m[k].y1, m[k].octave1, m[k].r1, m[k].depth1, &d1[32 * k]);
        add_key(*kf2, m[k].x2, m[k].y2, m[k].octave2, m[k].r2, m[k].depth2, &d2[32 * k]);
        const int row1 = (int)m[k].y1, col1 = (int)m[k].x1, row2 = (int)m[k].y2, col2 = (int)m[k].x2;
        kf1->mEntropy.paint(row1, col1, m[k].entropy1);
        kf1->mConfidence.paint(row1, col1, m[k].confidence1);
        kf1->mClasses.paint(row1, col1, (int)m[k].class1);
        kf2->mClasses.paint(row2, col2, (int)m[k].class2);
        script.matches[kf2].push_back(std::make_pair(k, k));
    }
    if (kf1->mEntropy.conflict || kf1->mConfidence.conflict || kf1->mClasses.conflict || kf2->mClasses.conflict) throw Quit{3};
    kf1->ordered.push_back(kf2);

    Map map;
    LocalMapping lm(&map, false);
    lm.mpCurrentKeyFrame = kf1;
    lm.CreateNewMapPoints();
    if (script.searches.size() != 1) throw Quit{5};

    std::vector<float> F12(script.searches[0].F12, script.searches[0].F12 + 9), geom(8 * n, 0.f);
    std::vector<unsigned char> created(n, 0), c1(n), c2(n), desc(32 * n, 0);
    for (size_t k = 0; k < n; ++k) {
        MapPoint *p = kf1->mvpMapPoints[k];
        if (p) {
            if (p != kf2->mvpMapPoints[k]) throw std::runtime_error("the two keyframes hold different points in one match's slots");
            created[k] = 1;
            put_point(p, &geom[8 * k], &desc[32 * k]);
        }
        cv::Mat w(3, 1, CV_32F);
        for (int i = 0; i < 3; ++i) w.at<float>(i) = wP[3 * k + i];
        c1[k] = (unsigned char)lm.CheckSemantics(kf1, (int)k, w, true);
        c2[k] = (unsigned char)lm.CheckSemantics(kf2, (int)k, w, false);
    }
    if (map.added.size() != lm.mlpRecentAddedMapPoints.size()) throw std::runtime_error("map and recent list disagree");
    Writer o(out);
    o.put(F12); o.put(created); o.put(c1); o.put(c2); o.put(geom); o.put(desc);
    for (MapPoint *p : map.added) delete p;
    return 0;
}

static int run_refresh(const char *in, const char *out) {
    Reader r(in);
    const size_t n = (size_t)r.i64();
    const bool reversed = r.i64() != 0;
    const std::vector<int64_t> desc_off = r.vec<int64_t>(n + 1), obs_off = r.vec<int64_t>(n + 1);
    const size_t nd = (size_t)desc_off[n], no = (size_t)obs_off[n];
    const std::vector<unsigned char> desc = r.vec<unsigned char>(32 * nd);
    const std::vector<float> ow = r.vec<float>(3 * no), rec = r.vec<float>(8 * n);
    const std::vector<unsigned char> kf_bad = r.vec<unsigned char>(no), point_bad = r.vec<unsigned char>(n);

    std::vector<KeyFrame> pool(no + 1);                                  // the last one: the reference keyframe of a point nobody observes
    Map map;
    std::vector<unsigned char> touched(2 * n, 0), out_desc(32 * n, 0);
    std::vector<float> geom(5 * n, 0.f);
    const unsigned char zeros[32] = {0};
    for (size_t p = 0; p < n; ++p) {
        size_t next_desc = (size_t)desc_off[p];
        KeyFrame *first = &pool[no];
        std::vector<KeyFrame *> seen;
        for (size_t j = (size_t)obs_off[p]; j < (size_t)obs_off[p + 1]; ++j) {
            KeyFrame &kf = pool[reversed ? no - 1 - j : j];
            for (int i = 0; i < 3; ++i) kf.mOw.at<float>(i) = ow[3 * j + i];
            kf.mbBad = kf_bad[j] != 0;
            kf.mnScaleLevels = 2;
            kf.mvScaleFactors = {rec[8 * p + 6], rec[8 * p + 7]};
            add_key(kf, 0.f, 0.f, 0, -1.f, -1.f, kf.mbBad ? zeros : &desc[32 * next_desc]);
            if (!kf.mbBad) ++next_desc;
            if (j == (size_t)obs_off[p]) first = &kf;
            seen.push_back(&kf);
        }
        if (next_desc != (size_t)desc_off[p + 1]) throw std::runtime_error("descriptor offsets and bad keyframes disagree");
        cv::Mat pos(3, 1, CV_32F);
        for (int i = 0; i < 3; ++i) pos.at<float>(i) = rec[8 * p + i];
        MapPoint mp(pos, first, &map);
        for (KeyFrame *kf : seen) mp.AddObservation(kf, 0);
        mp.mbBad = point_bad[p] != 0;
        mp.mfMaxDistance = mp.mfMinDistance = -1.f;
        mp.ComputeDistinctiveDescriptors();
        mp.UpdateNormalAndDepth();
        touched[2 * p] = !mp.mDescriptor.empty();
        touched[2 * p + 1] = mp.mfMaxDistance != -1.f;
        float g[8];
        put_point(&mp, g, &out_desc[32 * p]);
        for (int i = 0; i < 5; ++i) geom[5 * p + i] = g[3 + i];
    }
    Writer o(out);
    o.put(touched); o.put(out_desc); o.put(geom);
    return 0;
}

struct KeyRec { float x, y; int32_t octave; float r, depth; int32_t cls; double entropy, confidence; int32_t node, pad; };
static_assert(sizeof(KeyRec) == 48, "");

struct Walk {
    std::vector<KeyFrame> kf;
    LocalMapping *lm = nullptr;
    int64_t checks = 0, searched = 0;
    KeyFrame arriving;
    static Walk *&current() { static Walk *w = nullptr; return w; }
    static void on_search(KeyFrame *kf2) {
        Walk &w = *current();
        KeyFrame &cur = w.kf[0];
        const size_t n = cur.mvpMapPoints.size(), k = (size_t)(kf2 - &w.kf[1]);
        std::vector<std::pair<size_t, size_t> > &pairs = MatcherScript::get().matches[kf2];
        pairs.clear();
        for (size_t i = 0; i < n; ++i)
            if (!cur.mvpMapPoints[i] && !kf2->mvpMapPoints[n - 1 - i] && i % (k + 2) == 1) pairs.push_back(std::make_pair(i, n - 1 - i));
        if (++w.searched == w.checks) w.lm->mlNewKeyFrames.push_back(&w.arriving);
    }
};

static int run_walk(const char *in, const char *out) {
    Reader r(in);
    Walk w;
    const size_t nk = (size_t)r.i64();
    w.checks = r.i64();
    double cov[36], th[2];
    r.get(cov, sizeof cov); r.get(th, sizeof th);
    w.kf.resize(nk + 1);
    for (KeyFrame &K : w.kf) {
        SivoTriKeyFrame k;
        r.get(&k, sizeof k);
        const std::vector<KeyRec> keys = r.vec<KeyRec>((size_t)r.i64());
        const std::vector<unsigned char> desc = r.vec<unsigned char>(32 * keys.size());
        set_pose(K, k);
        K.mfScaleFactor = 1.2f;
        for (size_t i = 0; i < keys.size(); ++i) {
            const KeyRec &q = keys[i];
            add_key(K, q.x, q.y, q.octave, q.r, q.depth, &desc[32 * i]);
            K.mEntropy.paint((int)q.y, (int)q.x, q.entropy);
            K.mConfidence.paint((int)q.y, (int)q.x, q.confidence);
            K.mClasses.paint((int)q.y, (int)q.x, (int)q.cls);
        }
        if (K.mEntropy.conflict || K.mConfidence.conflict || K.mClasses.conflict) throw Quit{3};
    }
    const bool monocular = r.i64() != 0;
    for (size_t i = 1; i <= nk; ++i) { r.get(&w.kf[i].medianDepth, 4); w.kf[0].ordered.push_back(&w.kf[i]); }
    KeyFrame &cur = w.kf[0];
    cur.mThConfidence = (float)th[0]; cur.mThEntropyReduction = (float)th[1];
    if ((double)cur.mThConfidence != th[0] || (double)cur.mThEntropyReduction != th[1]) throw Quit{4};
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) cur.mSigma(a, b) = cov[6 * a + b];
    Map map;
    LocalMapping lm(&map, monocular);
    lm.mpCurrentKeyFrame = &cur;
    w.lm = &lm;
    Walk::current() = &w;
    MatcherScript &script = MatcherScript::get();
    script.on_search = Walk::on_search;
    lm.CreateNewMapPoints();
    Writer o(out);
    for (const MatcherScript::Search &s : script.searches) {
        const std::vector<std::pair<size_t, size_t> > &pairs = script.matches[s.kf2];
        std::vector<int64_t> head{(int64_t)(s.kf2 - &w.kf[1])}, body{(int64_t)pairs.size()};
        for (const auto &pr : pairs) { body.push_back((int64_t)pr.first); body.push_back((int64_t)pr.second); }
        o.put(head);
        o.put(std::vector<float>(s.F12, s.F12 + 9));
        o.put(s.occupied1);
        o.put(body);
        std::vector<int64_t> made;
        std::vector<float> pos;
        for (const auto &pr : pairs) {
            MapPoint *p = cur.mvpMapPoints[pr.first];
            if (!p || p != s.kf2->mvpMapPoints[pr.second]) continue;
            made.push_back((int64_t)pr.first); made.push_back((int64_t)pr.second);
            for (int i = 0; i < 3; ++i) pos.push_back(p->mWorldPos.at<float>(i));
        }
        o.put(std::vector<int64_t>{(int64_t)(made.size() / 2)});
        o.put(made); o.put(pos);
    }
    for (MapPoint *p : map.added) delete p;
    return 0;
}

static int run_neighbors(const char *in, const char *out) {
    Reader r(in);
    const size_t nk = (size_t)r.i64();
    const bool monocular = r.i64() != 0;
    std::vector<KeyFrame> kf(nk);
    std::vector<std::vector<int64_t> > slots(nk);
    for (size_t i = 0; i < nk; ++i) {
        kf[i].mnId = 10 + i;
        kf[i].mbBad = r.i64() != 0;
        kf[i].mnFuseTargetForKF = (long unsigned int)r.i64();
        for (int64_t n = r.i64(); n > 0; --n) kf[i].ordered.push_back(&kf[(size_t)r.i64()]);
        slots[i] = r.vec<int64_t>((size_t)r.i64());
        kf[i].mnScaleLevels = 2;
        kf[i].mvScaleFactors = {1.0f, 1.2f};
        for (int c = 0; c < 3; ++c) kf[i].mOw.at<float>(c) = (float)((c + 1) * (double)(i + 1));
        for (size_t j = 0; j < slots[i].size(); ++j) {
            unsigned char d[32];
            for (int b = 0; b < 32; ++b) d[b] = (unsigned char)(i * 31 + j * 7 + (size_t)b * 3);
            add_key(kf[i], 0.f, 0.f, 0, -1.f, -1.f, d);
        }
    }
    Map map;
    const size_t np = (size_t)r.i64();
    std::vector<MapPoint *> points;
    for (size_t p = 0; p < np; ++p) {
        cv::Mat pos(3, 1, CV_32F);
        pos.at<float>(0) = (float)p; pos.at<float>(1) = -(float)p; pos.at<float>(2) = 10.f + (float)p;
        KeyFrame *first = &kf[0];
        for (size_t i = nk; i-- > 0;)
            for (int64_t id : slots[i]) if (id == (int64_t)p) first = &kf[i];
        points.push_back(new MapPoint(pos, first, &map));
        for (size_t i = 0; i < nk; ++i)
            for (size_t j = 0; j < slots[i].size(); ++j)
                if (slots[i][j] == (int64_t)p) { points[p]->AddObservation(&kf[i], j); kf[i].mvpMapPoints[j] = points[p]; }
        points[p]->mbBad = r.i64() != 0;
        points[p]->mnFuseCandidateForKF = (long unsigned int)r.i64();
        points[p]->mfMaxDistance = points[p]->mfMinDistance = -1.f;
    }
    LocalMapping lm(&map, monocular);
    lm.mpCurrentKeyFrame = &kf[0];
    lm.SearchInNeighbors();
    const MatcherScript &script = MatcherScript::get();
    if (script.fuses.empty()) throw std::runtime_error("Fuse was never called");
    std::FILE *o = std::fopen(out, "w");
    if (!o) return 1;
    std::fprintf(o, "T");
    for (size_t c = 0; c + 1 < script.fuses.size(); ++c) std::fprintf(o, " %td", script.fuses[c].kf - &kf[0]);
    std::fprintf(o, "\nC");
    if (script.fuses.back().kf != &kf[0]) throw std::runtime_error("the last Fuse call is not on the current keyframe");
    for (MapPoint *p : script.fuses.back().points) std::fprintf(o, " %td", std::find(points.begin(), points.end(), p) - points.begin());
    std::fprintf(o, "\nR");
    for (MapPoint *p : kf[0].mvpMapPoints)
        if (p && p->mfMaxDistance != -1.f && !p->mDescriptor.empty()) std::fprintf(o, " %td", std::find(points.begin(), points.end(), p) - points.begin());
    std::fprintf(o, "\nU %d\n", kf[0].nUpdateConnections);
    std::fclose(o);
    for (MapPoint *p : points) delete p;
    return 0;
}

static int run_cos(const char *in, const char *out) {
    Reader r(in);
    const size_t n = (size_t)r.i64();
    const std::vector<float> v = r.vec<float>(2 * n);
    std::vector<float> c(n);
    // the same operand types as the source's line: a float member halved by an int literal, an element of a std::vector<float>, an int
    // factor, unqualified names after `using namespace std`
    KeyFrame holder, *k = &holder;
    k->mvDepth.assign(1, 0.f);
    const int at = 0;
    for (size_t i = 0; i < n; ++i) {
        k->mb = v[2 * i]; k->mvDepth[at] = v[2 * i + 1];
        c[i] = cos(2 * atan2(k->mb / 2, k->mvDepth[at]));
    }
    std::printf("%zu\n", sizeof(decltype(cos(2 * atan2(k->mb / 2, k->mvDepth[at])))));
    Writer o(out);
    o.put(c);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 64;
    try {
        const std::string mode = argv[1];
        if (mode == "tri") return run_tri(argv[2], argv[3]);
        if (mode == "refresh") return run_refresh(argv[2], argv[3]);
        if (mode == "walk") return run_walk(argv[2], argv[3]);
        if (mode == "neighbors") return run_neighbors(argv[2], argv[3]);
        if (mode == "cos") return run_cos(argv[2], argv[3]);
        return 64;
    } catch (const Quit &q) {
        return q.code;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
