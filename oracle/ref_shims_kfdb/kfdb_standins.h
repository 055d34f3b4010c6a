// Forced include (-include) of the oracle/_ref build of the reference's KeyFrameDatabase.cc.  Its own header KeyFrameDatabase.h is read
// where it lies, and ORBVocabulary.h with it: the vocabulary is DBoW2's real TemplatedVocabulary<FORB::TDescriptor, FORB>.  KeyFrame.h and
// Frame.h (Caffe, Eigen, the map graph, threads) are switched off through their include guards; the two data holders below carry what
// the database reads and writes, under the reference's names, with its types and its initial values.  <opencv2/core/core.hpp> is the
// stand-in of tests/bow_reference_shim, as for tests/golden/make_bow_reference.py.
#pragma once
#define KEYFRAME_H
#define FRAME_H

#include <list>
#include <set>
#include <vector>

#include "dependencies/DBoW2/DBoW2/BowVector.h"

namespace SIVO {

class KeyFrame {
 public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;                                 // (the reference leaves the two scores unset until a query writes them)
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;
    std::set<KeyFrame *> connected;                       // mConnectedKeyFrameWeights' keys
    std::vector<KeyFrame *> ordered;                      // mvpOrderedConnectedKeyFrames
    std::set<KeyFrame *> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) {
        return (int)ordered.size() < N ? ordered : std::vector<KeyFrame *>(ordered.begin(), ordered.begin() + N);
    }
};

class Frame {
 public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};

}  // namespace SIVO
