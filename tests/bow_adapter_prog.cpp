// bow_adapter_prog.cpp — SIVO::ORBVocabulary and SIVO::KeyFrameDatabase over stand-in KeyFrame / Frame types (bow_standins.hpp), run on a
// scene tests/test_gpu_bow.py writes: every keyframe's and frame's ComputeBoW, then a list of add / erase / clear / DetectLoopCandidates /
// DetectRelocalizationCandidates calls.  Writes the BowVectors, every returned candidate vector in its order and, at the end, the
// fields the detections leave in every keyframe, as text with hexadecimal floats (bit exact).
//   bow_adapter_prog <voc.txt> <scene.bin> <out.txt> [pin]
//   scene: int64 levelsup, n_kf; per keyframe: int64 n, n x 32 bytes, int64 n_connected, ids, int64 n_ordered, ids;
//          int64 n_frames; per frame: int64 n, n x 32 bytes; int64 n_ops; per op: int64 op (0 add, 1 erase, 2 loop, 3 reloc, 4 clear),
//          int64 index, double minScore
#include <cstdio>

#include "blob_io.hpp"
#include "bow_standins.hpp"
#ifdef SIVO_BOW_ON_HOST
#include "bow_host_capi.hpp"
#endif

struct SceneReader : BlobReader {
    using BlobReader::BlobReader;
    int64_t i64() { return one<int64_t>(); }
    template <class T>
    bool vector_kind(T &x) {                                            // pin scripts: true when the record was a BowVector
        if (i64() == 0) return false;
        const std::vector<int32_t> w = many<int32_t>((size_t)i64());
        const std::vector<double> v = many<double>(w.size());
        for (size_t i = 0; i < w.size(); ++i) x.mBowVec[(DBoW2::WordId)w[i]] = v[i];
        return true;
    }
    cv::Mat desc() {
        const int64_t n = i64();
        cv::Mat m((int)n, 32, CV_8UC1);
        for (int r = 0; r < (int)n; ++r) get(m.ptr<unsigned char>(r), 32);
        return m;
    }
};

template <class T>
static void compute_bow(const SIVO::ORBVocabulary &voc, T &x, int levelsup, bool rows) {
    if (!rows) {
        voc.transform(x.mDescriptorsSemantic, x.mBowVec, x.mFeatVec, levelsup);
        return;
    }
    std::vector<cv::Mat> v;                                             // Converter::toDescriptorVector
    for (int r = 0; r < x.mDescriptorsSemantic.rows; ++r) v.push_back(x.mDescriptorsSemantic.row(r));
    voc.transform(v, x.mBowVec, x.mFeatVec, levelsup);
}

static void print_bow(std::FILE *f, const char *tag, size_t i, const DBoW2::BowVector &b, const DBoW2::FeatureVector &fv) {
    std::fprintf(f, "%s %zu %zu", tag, i, b.size());
    for (DBoW2::BowVector::const_iterator it = b.begin(); it != b.end(); ++it) std::fprintf(f, " %u:%a", it->first, it->second);
    std::fprintf(f, "\n%sV %zu %zu", tag, i, fv.size());
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        std::fprintf(f, " %u:", it->first);
        for (size_t j = 0; j < it->second.size(); ++j) std::fprintf(f, "%s%u", j ? "," : "", it->second[j]);
    }
    std::fprintf(f, "\n");
}

static int run(int argc, char **argv) {
    if (argc != 4 && !(argc == 5 && std::string(argv[4]) == "pin")) throw BlobUsage();
    const bool pin = argc == 5;
    SIVO::ORBVocabulary voc;
    if (!voc.loadFromTextFile(argv[1])) return 2;
    SceneReader r(argv[2]);
    std::FILE *out = std::fopen(argv[3], "w");
    if (!out) throw std::runtime_error(std::string("cannot open ") + argv[3]);
    const int levelsup = (int)r.i64();
    std::vector<BKeyFrame> kfs((size_t)r.i64());
    for (size_t i = 0; i < kfs.size(); ++i) {
        BKeyFrame &k = kfs[i];
        k.mnId = i;
        const bool given = pin && r.vector_kind(k);
        if (!given) k.mDescriptorsSemantic = r.desc();
        for (int64_t n = r.i64(); n > 0; --n) k.connected.insert(&kfs[(size_t)r.i64()]);
        for (int64_t n = r.i64(); n > 0; --n) k.ordered.push_back(&kfs[(size_t)r.i64()]);
        if (!given) compute_bow(voc, k, levelsup, i % 2 == 0);
        print_bow(out, "B", i, k.mBowVec, k.mFeatVec);
    }
    std::vector<BFrame> frames((size_t)r.i64());
    for (size_t i = 0; i < frames.size(); ++i) {
        frames[i].mnId = 1000 + i;
        const bool given = pin && r.vector_kind(frames[i]);
        if (!given) frames[i].mDescriptorsSemantic = r.desc();
        if (!given) compute_bow(voc, frames[i], levelsup, i % 2 == 1);
        print_bow(out, "F", i, frames[i].mBowVec, frames[i].mFeatVec);
    }
    SIVO::KeyFrameDatabase db(voc);
    const int64_t n_ops = r.i64();
    for (int64_t o = 0; o < n_ops; ++o) {
        const int64_t op = r.i64(), idx = r.i64();
        const double min_score = r.one<double>();
        std::vector<BKeyFrame *> got;
        if (op == 0) db.add(&kfs[(size_t)idx]);
        else if (op == 1) db.erase(&kfs[(size_t)idx]);
        else if (op == 2) got = db.DetectLoopCandidates(&kfs[(size_t)idx], (float)min_score);
        else if (op == 3) { std::vector<BKeyFrame *> v = db.DetectRelocalizationCandidates(&frames[(size_t)idx]); got = v; }
        else if (op == 4) db.clear();
        if (pin) std::fprintf(out, "S %lld\n", (long long)o);
        if (op == 2 || op == 3) {
            std::fprintf(out, "Q %lld %zu", (long long)o, got.size());
            for (size_t i = 0; i < got.size(); ++i) std::fprintf(out, " %lu", got[i]->mnId);
            std::fprintf(out, "\n");
        }
        for (size_t i = 0; pin && i < kfs.size(); ++i)
            std::fprintf(out, "K %zu %lu %d %lu %d %a %a\n", i, kfs[i].mnLoopQuery, kfs[i].mnLoopWords, kfs[i].mnRelocQuery, kfs[i].mnRelocWords,
                         (double)kfs[i].mLoopScore, (double)kfs[i].mRelocScore);
    }
    for (size_t i = 0; !pin && i < kfs.size(); ++i)
        std::fprintf(out, "K %zu %lu %d %lu %d %a %a\n", i, kfs[i].mnLoopQuery, kfs[i].mnLoopWords, kfs[i].mnRelocQuery, kfs[i].mnRelocWords,
                     (double)kfs[i].mLoopScore, (double)kfs[i].mRelocScore);
    if (std::fclose(out) != 0) throw std::runtime_error(std::string("short write to ") + argv[3]);
    return 0;
}

int main(int argc, char **argv) { return blob_main(argc, argv, "bow_adapter_prog <voc.txt> <scene.bin> <out.txt> [pin]", run); }
