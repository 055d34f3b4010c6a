/**
 * SIVO::ORBVocabulary with the members System.cc, Frame::ComputeBoW, KeyFrame::ComputeBoW and KeyFrameDatabase use of the reference's
 * typedef (reference include/orbslam/ORBVocabulary.h: DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>): loadFromTextFile
 * (TemplatedVocabulary.h:1338-1424), transform(features, BowVector &, FeatureVector &, levelsup) (:1126-1194), score (:1198-1203),
 * size, empty.  The descent, the sort by word and by node and the ordered L1 norm run on the device (sivo_bow_transform,
 * sivo_amd/csrc/bow.hip); the values are bit-identical to DBoW2's.  Only L1_NORM scoring with TF_IDF weighting (what ORBvoc.txt carries):
 * any other header makes loadFromTextFile return false with the library's text on stderr.
 *
 * DBoW2::BowVector / DBoW2::FeatureVector are std::map<unsigned, double> / std::map<unsigned, std::vector<unsigned>> here; with
 * -DSIVO_HAVE_DBOW2 the real container headers are included instead (they derive from the same maps).
 * Differences from the reference: INTEGRATION.md, "Place recognition".
 */
#ifndef SIVO_AMD_API_ORBVOCABULARY_H
#define SIVO_AMD_API_ORBVOCABULARY_H

#ifdef SIVO_HAVE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "../compat/cv_min.hpp"
#endif

#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/sivo_hip.h"

#ifdef SIVO_HAVE_DBOW2
#include "dependencies/DBoW2/DBoW2/BowVector.h"
#include "dependencies/DBoW2/DBoW2/FeatureVector.h"
#else
namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
typedef unsigned int NodeId;
typedef std::map<WordId, WordValue> BowVector;
typedef std::map<NodeId, std::vector<unsigned int> > FeatureVector;
}  // namespace DBoW2
#endif

namespace SIVO {

class ORBVocabulary {
 public:
    ORBVocabulary() {}
    ~ORBVocabulary() { sivo_voc_destroy(voc_); }
    ORBVocabulary(const ORBVocabulary &) = delete;
    ORBVocabulary &operator=(const ORBVocabulary &) = delete;

    bool loadFromTextFile(const std::string &filename) {
        sivo_voc_t v = nullptr;
        if (sivo_voc_create_from_text(filename.c_str(), &v) != SIVO_OK) {
            std::cerr << "Vocabulary loading failure: " << sivo_last_error() << std::endl;
            return false;
        }
        sivo_voc_destroy(voc_);
        voc_ = v;
        int64_t words = 0;
        sivo_voc_info(voc_, nullptr, nullptr, nullptr, &words);
        words_ = (unsigned)words;
        return true;
    }

    unsigned int size() const { return words_; }
    bool empty() const { return words_ == 0; }
    sivo_voc_t handle() const { return voc_; }

    // Frame::ComputeBoW / KeyFrame::ComputeBoW as written: one 1 x 32 CV_8U row per feature
    void transform(const std::vector<cv::Mat> &features, DBoW2::BowVector &v, DBoW2::FeatureVector &fv, int levelsup) const {
        std::vector<uint8_t> desc(32 * features.size());
        for (size_t i = 0; i < features.size(); ++i) {
            if (features[i].rows * features[i].cols != 32) throw std::invalid_argument("ORBVocabulary::transform: a descriptor is not 32 bytes");
            std::memcpy(&desc[32 * i], features[i].ptr<unsigned char>(0), 32);
        }
        run(desc.data(), (int)features.size(), v, fv, levelsup);
    }
    // the N x 32 descriptor matrix itself: ComputeBoW without Converter::toDescriptorVector
    void transform(const cv::Mat &descriptors, DBoW2::BowVector &v, DBoW2::FeatureVector &fv, int levelsup) const {
        if (descriptors.rows > 0 && descriptors.cols != 32) throw std::invalid_argument("ORBVocabulary::transform: the matrix is not N x 32");
        std::vector<uint8_t> desc(32 * (size_t)descriptors.rows);
        for (int r = 0; r < descriptors.rows; ++r) std::memcpy(&desc[32 * (size_t)r], descriptors.ptr<unsigned char>(r), 32);
        run(desc.data(), descriptors.rows, v, fv, levelsup);
    }

    // L1Scoring::score (ScoringObject.cpp:23-68) on the host: the same terms in the same order as sivo_bowdb_query
    double score(const DBoW2::BowVector &v1, const DBoW2::BowVector &v2) const {
        DBoW2::BowVector::const_iterator a = v1.begin(), b = v2.begin();
        double s = 0;
        while (a != v1.end() && b != v2.end()) {                        // both maps ascend: one walk in step meets the shared words in order
            if (a->first < b->first) { ++a; continue; }
            if (b->first < a->first) { ++b; continue; }
            s += std::fabs(a->second - b->second) - std::fabs(a->second) - std::fabs(b->second);
            ++a; ++b;
        }
        return -s / 2.0;
    }

 private:
    void run(const uint8_t *desc, int n, DBoW2::BowVector &v, DBoW2::FeatureVector &fv, int levelsup) const {
        v.clear();
        fv.clear();
        if (empty() || n == 0) return;                                  // :1134
        const size_t N = (size_t)n;
        std::vector<int32_t> i32(6 * N + 1);
        std::vector<double> values(N);
        int32_t *word = i32.data(), *node = word + N, *bw = node + N, *fn = bw + N, *ff = fn + N, *fo = ff + N;
        int32_t nw = 0, nf = 0;
        const int rc = sivo_bow_transform(voc_, desc, n, levelsup, word, node, bw, values.data(), &nw, fn, fo, ff, &nf);
        if (rc == SIVO_ERR_INVALID_ARGUMENT) throw std::invalid_argument(sivo_last_error());
        if (rc != SIVO_OK) throw std::runtime_error(sivo_last_error());
        for (int i = 0; i < nw; ++i) v.insert(v.end(), DBoW2::BowVector::value_type((unsigned)bw[i], values[(size_t)i]));
        for (int i = 0; i < nf; ++i)
            fv.insert(fv.end(), DBoW2::FeatureVector::value_type((unsigned)fn[i], std::vector<unsigned int>(ff + fo[i], ff + fo[i + 1])));
    }
    sivo_voc_t voc_ = nullptr;
    unsigned words_ = 0;
};

}  // namespace SIVO

#endif  // SIVO_AMD_API_ORBVOCABULARY_H
