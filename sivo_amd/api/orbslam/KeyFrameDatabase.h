/**
 * SIVO::KeyFrameDatabase with the reference's interface (reference include/orbslam/KeyFrameDatabase.h, src/orbslam/KeyFrameDatabase.cc):
 * add, erase, clear, DetectLoopCandidates, DetectRelocalizationCandidates.  The members are templates over the SLAM types, like
 * OptimizerAdapter.h: they read mBowVec, mnId, GetConnectedKeyFrames(), GetBestCovisibilityKeyFrames(10) and write mnLoopQuery,
 * mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore under the reference's names.
 *
 * The stored BowVectors live on the device (sivo_bowdb_*, sivo_amd/csrc/bow.hip).  A detection is ONE sivo_bowdb_query over every stored
 * keyframe — shared-word count, smallest shared word and L1 score per keyframe — in place of the walk through the inverted file
 * (KeyFrameDatabase.cc:82-102, :211-229) and of the per-candidate score calls (:135, :259); the host logic after it restates the reference's
 * (:105-201, :231-321).  The reference meets the keyframes by ascending query word and, within a word's list, in order of add among
 * the keyframes still present, so the sharing keyframes are ordered by (smallest shared word, add sequence): the returned vector has
 * the reference's order.  Every query is expected to carry an id no earlier query of its kind carried (as the reference's callers do).
 */
#ifndef SIVO_AMD_API_KEYFRAMEDATABASE_H
#define SIVO_AMD_API_KEYFRAMEDATABASE_H

#include <algorithm>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "ORBVocabulary.h"

namespace SIVO {

class KeyFrameDatabase {
 public:
    explicit KeyFrameDatabase(const ORBVocabulary &voc) {
        if (sivo_bowdb_create(voc.handle(), &db_) != SIVO_OK) throw std::invalid_argument(sivo_last_error());
    }
    ~KeyFrameDatabase() { sivo_bowdb_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

    template <class KeyFrame>
    void add(KeyFrame *pKF) {
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<int32_t> w;
        std::vector<double> v;
        flatten(pKF->mBowVec, w, v);
        int32_t slot = -1;
        check(sivo_bowdb_add(db_, w.data(), v.data(), (int)w.size(), &slot));
        if ((size_t)slot != kf_.size()) throw std::logic_error("KeyFrameDatabase: slots out of step");
        kf_.push_back(pKF);
        slots_of_[pKF].push_back(slot);
    }

    template <class KeyFrame>
    void erase(KeyFrame *pKF) {
        std::unique_lock<std::mutex> lock(mMutex);
        std::map<void *, std::vector<int32_t> >::iterator it = slots_of_.find(pKF);
        if (it == slots_of_.end()) return;                             // (the reference finds it in no list)
        // A keyframe added more than once stands in its lists once per add, and :56-62 take the FIRST entry out of each list: the
        // earliest add goes, a later one keeps its place behind the keyframes added in between.
        const int32_t slot = it->second.front();
        check(sivo_bowdb_erase(db_, slot));
        kf_[(size_t)slot] = nullptr;
        it->second.erase(it->second.begin());
        if (it->second.empty()) slots_of_.erase(it);
    }

    void clear() {
        std::unique_lock<std::mutex> lock(mMutex);
        check(sivo_bowdb_clear(db_));
        kf_.clear();
        slots_of_.clear();
    }

    // KeyFrameDatabase.cc:72-202
    template <class KeyFrame>
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore) {
        const std::set<KeyFrame *> connected = pKF->GetConnectedKeyFrames();
        const unsigned long id = pKF->mnId;
        std::vector<Sharing<KeyFrame> > sharing;
        {
            std::unique_lock<std::mutex> lock(mMutex);
            std::vector<int32_t> common;
            std::vector<double> score;
            for (int32_t slot : query(pKF->mBowVec, common, score)) {
                KeyFrame *kf = static_cast<KeyFrame *>(kf_[(size_t)slot]);
                if (kf->mnLoopQuery == id) {                             // (an id used twice: the walk only goes on counting)
                    kf->mnLoopWords += common[(size_t)slot];
                } else if (connected.count(kf)) {
                    kf->mnLoopWords = 1;                                 // the walk resets the count at every shared word, then adds one
                } else {
                    kf->mnLoopQuery = id;
                    kf->mnLoopWords = common[(size_t)slot];
                    sharing.push_back(Sharing<KeyFrame>{kf, (float)score[(size_t)slot]});
                }
            }
        }
        int most = 0;
        for (const Sharing<KeyFrame> &e : sharing) most = std::max(most, (int)e.kf->mnLoopWords);
        const int enough = most * 0.8f;                                  // float product, truncated
        std::vector<Sharing<KeyFrame> > scored;
        for (const Sharing<KeyFrame> &e : sharing) {
            if (!(e.kf->mnLoopWords > enough)) continue;
            e.kf->mLoopScore = e.score;
            if (e.score >= minScore) scored.push_back(e);
        }
        return groups(scored, minScore, [&](KeyFrame *k) { return k->mnLoopQuery == id && k->mnLoopWords > enough; },
                      [](KeyFrame *k) { return k->mLoopScore; });
    }

    // KeyFrameDatabase.cc:204-322.  The keyframe type is not among the arguments: the call returns a value that runs the detection when
    // it is converted to the std::vector<KeyFrame *> the caller declares (Tracking.cc: `vector<KeyFrame *> v = db->Detect...(&frame);`).
    // Do NOT receive it with `auto` or discard it: nothing runs until the conversion, and a later conversion queries the database as it
    // is then.  A caller that wants no conversion names the type: RelocalizationCandidates<KeyFrame>(F).
    template <class Frame>
    struct RelocalizationQuery {
        KeyFrameDatabase *db;
        Frame *F;
        template <class KeyFrame>
        operator std::vector<KeyFrame *>() const { return db->template RelocalizationCandidates<KeyFrame>(F); }
    };
    template <class Frame>
    RelocalizationQuery<Frame> DetectRelocalizationCandidates(Frame *F) { return RelocalizationQuery<Frame>{this, F}; }

    template <class KeyFrame, class Frame>
    std::vector<KeyFrame *> RelocalizationCandidates(Frame *F) {
        const unsigned long id = F->mnId;
        std::vector<Sharing<KeyFrame> > sharing;
        {
            std::unique_lock<std::mutex> lock(mMutex);
            std::vector<int32_t> common;
            std::vector<double> score;
            for (int32_t slot : query(F->mBowVec, common, score)) {
                KeyFrame *kf = static_cast<KeyFrame *>(kf_[(size_t)slot]);
                if (kf->mnRelocQuery == id) {
                    kf->mnRelocWords += common[(size_t)slot];
                } else {
                    kf->mnRelocQuery = id;
                    kf->mnRelocWords = common[(size_t)slot];
                    sharing.push_back(Sharing<KeyFrame>{kf, (float)score[(size_t)slot]});
                }
            }
        }
        int most = 0;
        for (const Sharing<KeyFrame> &e : sharing) most = std::max(most, (int)e.kf->mnRelocWords);
        const int enough = most * 0.8f;
        std::vector<Sharing<KeyFrame> > scored;
        for (const Sharing<KeyFrame> &e : sharing) {
            if (!(e.kf->mnRelocWords > enough)) continue;
            e.kf->mRelocScore = e.score;
            scored.push_back(e);
        }
        // (a neighbour counts as soon as this query met it, whether or not it was scored: its mRelocScore is then what an earlier query left)
        return groups(scored, 0.f, [&](KeyFrame *k) { return k->mnRelocQuery == id; }, [](KeyFrame *k) { return k->mRelocScore; });
    }

 protected:
    static void check(int rc) {
        if (rc == SIVO_ERR_INVALID_ARGUMENT) throw std::invalid_argument(sivo_last_error());
        if (rc != SIVO_OK) throw std::runtime_error(sivo_last_error());
    }
    template <class Bow>
    static void flatten(const Bow &b, std::vector<int32_t> &w, std::vector<double> &v) {
        w.clear(); v.clear();
        for (typename Bow::const_iterator it = b.begin(); it != b.end(); ++it) {
            w.push_back((int32_t)it->first);
            v.push_back(it->second);
        }
    }
    // One launch over every stored keyframe; returns the slots that share a word with the query in the order the reference's walk
    // through the inverted file first meets them: (smallest shared word, add sequence).
    template <class Bow>
    std::vector<int32_t> query(const Bow &bow, std::vector<int32_t> &common, std::vector<double> &score) {
        std::vector<int32_t> w, first(kf_.size() + 1), order;
        std::vector<double> v;
        flatten(bow, w, v);
        common.assign(kf_.size() + 1, 0);
        score.assign(kf_.size() + 1, 0.0);
        int32_t n = 0;
        check(sivo_bowdb_query(db_, w.data(), v.data(), (int)w.size(), common.data(), first.data(), score.data(), &n));
        if ((size_t)n != kf_.size()) throw std::logic_error("KeyFrameDatabase: slots out of step");
        for (int32_t s = 0; s < n; ++s)
            if (common[(size_t)s] > 0 && kf_[(size_t)s]) order.push_back(s);
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            return first[(size_t)a] != first[(size_t)b] ? first[(size_t)a] < first[(size_t)b] : a < b;
        });
        return order;
    }
    template <class KeyFrame>
    struct Sharing { KeyFrame *kf; float score; };
    // :146-201, :268-321: every scored keyframe gathers the scores of those of its ten best covisible keyframes that `counts` admits
    // and is represented by the best-scoring member of that group; the groups whose total exceeds 0.75 of the best total (at least
    // `floor`) give their representatives, each once, in the order of `scored`.  Sums and comparisons in float, as the reference's.
    template <class KeyFrame, class Counts, class ScoreOf>
    static std::vector<KeyFrame *> groups(const std::vector<Sharing<KeyFrame> > &scored, float floor, Counts counts, ScoreOf score_of) {
        std::vector<Sharing<KeyFrame> > totals;
        float best_total = floor;
        for (const Sharing<KeyFrame> &e : scored) {
            float top = e.score, total = e.score;
            KeyFrame *representative = e.kf;
            for (KeyFrame *neighbour : e.kf->GetBestCovisibilityKeyFrames(10)) {
                if (!counts(neighbour)) continue;
                const float s = score_of(neighbour);
                total += s;
                if (s > top) { representative = neighbour; top = s; }
            }
            totals.push_back(Sharing<KeyFrame>{representative, total});
            if (total > best_total) best_total = total;
        }
        const float keep = 0.75f * best_total;
        std::vector<KeyFrame *> out;
        std::set<KeyFrame *> seen;
        for (const Sharing<KeyFrame> &t : totals)
            if (t.score > keep && seen.insert(t.kf).second) out.push_back(t.kf);
        return out;
    }

    sivo_bowdb_t db_ = nullptr;
    std::vector<void *> kf_;                 // slot -> keyframe (nullptr: erased); the slot is the add sequence
    std::map<void *, std::vector<int32_t> > slots_of_;   // the live slots of a keyframe, ascending: one per add not yet erased
    std::mutex mMutex;
};

}  // namespace SIVO

#endif  // SIVO_AMD_API_KEYFRAMEDATABASE_H
