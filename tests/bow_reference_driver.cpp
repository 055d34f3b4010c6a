// bow_reference_driver.cpp — runs the reference's own DBoW2 (TemplatedVocabulary<FORB::TDescriptor, FORB>: loadFromTextFile, transform,
// score) on a vocabulary file and two feature sets and writes what it computes; tests/golden/make_bow_reference.py compiles it against
// the reference's sources in a temporary directory and records the output in tests/golden/bow_reference.npz.
//   bow_reference_driver <voc.txt> <in> <out>
//   in:  int64 n_levels, levelsup[n_levels]; two sets: int64 n, n x 32 bytes
//   out: per levelsup, for the first set: int64 n, nw, nf, m; word[n] node[n] bow_words[nw] fv_nodes[nf] fv_off[nf + 1] fv_feat[m]
//        (int32), bow_values[nw] (double); then double score(set 1, set 2), score(set 1, set 1)
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>

#include "FORB.h"
#include "TemplatedVocabulary.h"

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> Base;
struct Voc : Base {
    using Base::transform;                                            // (the per-feature form is protected)
};

static std::vector<char> raw;
static size_t at = 0;
static int64_t i64() { int64_t v; std::memcpy(&v, raw.data() + at, 8); at += 8; return v; }
static std::vector<cv::Mat> read_set() {
    std::vector<cv::Mat> f((size_t)i64());
    for (cv::Mat &m : f) {
        m.create(1, 32, CV_8U);
        std::memcpy(m.ptr<unsigned char>(), raw.data() + at, 32);
        at += 32;
    }
    return f;
}
template <class T> static void put(std::FILE *f, const std::vector<T> &v) { if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char **argv) {
    if (argc != 4) return 64;
    Voc voc;
    if (!voc.loadFromTextFile(argv[1])) return 2;
    {
        std::ifstream in(argv[2], std::ios::binary);
        raw.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    }
    std::vector<int64_t> levels((size_t)i64());
    for (int64_t &l : levels) l = i64();
    const std::vector<cv::Mat> a = read_set(), b = read_set();
    std::FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 1;
    for (int64_t lv : levels) {
        DBoW2::BowVector bow;
        DBoW2::FeatureVector fv;
        voc.transform(a, bow, fv, (int)lv);
        std::vector<int32_t> word, node, bw, fn, fo, ff;
        std::vector<double> bv;
        for (const cv::Mat &d : a) {                                  // the per-feature form (:1217-1259)
            DBoW2::WordId w;
            DBoW2::WordValue weight;
            DBoW2::NodeId nid;
            voc.transform(d, w, weight, &nid, (int)lv);
            word.push_back((int32_t)w);
            node.push_back((int32_t)nid);
        }
        for (DBoW2::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) { bw.push_back((int32_t)it->first); bv.push_back(it->second); }
        for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
            fn.push_back((int32_t)it->first);
            fo.push_back((int32_t)ff.size());
            for (unsigned i : it->second) ff.push_back((int32_t)i);
        }
        fo.push_back((int32_t)ff.size());
        const int64_t head[4] = {(int64_t)a.size(), (int64_t)bw.size(), (int64_t)fn.size(), (int64_t)ff.size()};
        std::fwrite(head, 8, 4, out);
        put(out, word); put(out, node); put(out, bw); put(out, fn); put(out, fo); put(out, ff); put(out, bv);
    }
    DBoW2::BowVector va, vb;
    DBoW2::FeatureVector fa, fb;
    voc.transform(a, va, fa, 0);
    voc.transform(b, vb, fb, 0);
    const double s[2] = {voc.score(va, vb), voc.score(va, va)};
    std::fwrite(s, 8, 2, out);
    std::fclose(out);
    return 0;
}
