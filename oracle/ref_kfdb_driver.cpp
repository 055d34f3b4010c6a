// ref_kfdb_driver.cpp — replays a script of add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates on the reference's
// own KeyFrameDatabase (KeyFrameDatabase.cc compiled untouched, see the Makefile) over DBoW2's real vocabulary, and writes what the
// reference leaves behind: every returned vector in its order and, after every operation, the six query members of every keyframe.
//   ref_kfdb <voc.txt> <script.bin> <out.txt> <asc|desc|mixed>
//   script: tests/bowdb_pin_cases.py (write_script): int64 levelsup, n_kf; per keyframe: a BoW source, int64 n_connected, ids,
//           int64 n_ordered, ids; int64 n_frames; per frame: a BoW source; int64 n_ops; per op: int64 op (0 add, 1 erase, 2 loop, 3 reloc,
//           4 clear), int64 index, double minScore.  A BoW source: int64 kind; 0: int64 n, n x 32 descriptor bytes (the vocabulary
//           transforms them); 1: int64 n, n int32 words, n double values (taken as they are).
//   The last argument decides where the keyframes lie: keyframe i at the i-th, the (n - 1 - i)-th or a scattered place of one array, so
//   that the order of their addresses is the id order, its reverse, or neither.
//   out: the text tests/bowdb_pin_cases.py (parse_output) reads; floats in hexadecimal.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>

#include "include/orbslam/KeyFrameDatabase.h"

struct Reader {
    std::vector<char> b;
    size_t at = 0;
    void get(void *dst, size_t bytes) {
        if (at + bytes > b.size()) throw std::runtime_error("script file too short");
        if (bytes) std::memcpy(dst, b.data() + at, bytes);
        at += bytes;
    }
    int64_t i64() { int64_t v; get(&v, 8); return v; }
    double f64() { double v; get(&v, 8); return v; }
};

static void read_bow(Reader &r, const SIVO::ORBVocabulary &voc, int levelsup, DBoW2::BowVector &bow) {
    const int64_t kind = r.i64(), n = r.i64();
    if (kind == 0) {
        std::vector<cv::Mat> f((size_t)n);
        for (cv::Mat &m : f) {
            m.create(1, 32, CV_8U);
            r.get(m.ptr<unsigned char>(), 32);
        }
        DBoW2::FeatureVector fv;
        voc.transform(f, bow, fv, levelsup);
        return;
    }
    std::vector<int32_t> w((size_t)n);
    std::vector<double> v((size_t)n);
    r.get(w.data(), 4 * w.size());
    r.get(v.data(), 8 * v.size());
    for (size_t i = 0; i < w.size(); ++i) bow[(DBoW2::WordId)w[i]] = v[i];
}

static void print_bow(std::FILE *f, const char *tag, size_t i, const DBoW2::BowVector &b) {
    std::fprintf(f, "%s %zu %zu", tag, i, b.size());
    for (DBoW2::BowVector::const_iterator it = b.begin(); it != b.end(); ++it) std::fprintf(f, " %u:%a", it->first, it->second);
    std::fprintf(f, "\n");
}

int main(int argc, char **argv) {
    if (argc != 5) return 64;
    try {
        SIVO::ORBVocabulary voc;
        if (!voc.loadFromTextFile(argv[1])) return 2;
        Reader r;
        {
            std::ifstream in(argv[2], std::ios::binary);
            r.b.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        }
        std::FILE *out = std::fopen(argv[3], "w");
        if (!out) return 1;
        const std::string where = argv[4];
        const int levelsup = (int)r.i64();
        const size_t n = (size_t)r.i64();
        std::vector<SIVO::KeyFrame> pool(n);
        std::vector<SIVO::KeyFrame *> kf(n);
        for (size_t i = 0; i < n; ++i) {
            size_t at = i;
            if (where == "desc") at = n - 1 - i;
            else if (where == "mixed") at = i % 2 ? n - 1 - i / 2 : i / 2;      // 0, n - 1, 1, n - 2, ...: a permutation
            else if (where != "asc") return 64;
            kf[i] = &pool[at];
        }
        for (size_t i = 0; i < n; ++i) {
            kf[i]->mnId = i;
            read_bow(r, voc, levelsup, kf[i]->mBowVec);
            for (int64_t m = r.i64(); m > 0; --m) kf[i]->connected.insert(kf[(size_t)r.i64()]);
            for (int64_t m = r.i64(); m > 0; --m) kf[i]->ordered.push_back(kf[(size_t)r.i64()]);
            print_bow(out, "B", i, kf[i]->mBowVec);
        }
        std::vector<SIVO::Frame> frames((size_t)r.i64());
        for (size_t i = 0; i < frames.size(); ++i) {
            frames[i].mnId = 1000 + i;
            read_bow(r, voc, levelsup, frames[i].mBowVec);
            print_bow(out, "F", i, frames[i].mBowVec);
        }
        SIVO::KeyFrameDatabase db(voc);
        const int64_t n_ops = r.i64();
        for (int64_t o = 0; o < n_ops; ++o) {
            const int64_t op = r.i64(), idx = r.i64();
            const double min_score = r.f64();
            std::vector<SIVO::KeyFrame *> got;
            if (op == 0) db.add(kf[(size_t)idx]);
            else if (op == 1) db.erase(kf[(size_t)idx]);
            else if (op == 2) got = db.DetectLoopCandidates(kf[(size_t)idx], (float)min_score);
            else if (op == 3) got = db.DetectRelocalizationCandidates(&frames[(size_t)idx]);
            else if (op == 4) db.clear();
            else throw std::runtime_error("unknown operation");
            std::fprintf(out, "S %lld\n", (long long)o);
            if (op == 2 || op == 3) {
                std::fprintf(out, "Q %lld %zu", (long long)o, got.size());
                for (size_t i = 0; i < got.size(); ++i) std::fprintf(out, " %lu", got[i]->mnId);
                std::fprintf(out, "\n");
            }
            for (size_t i = 0; i < n; ++i)
                std::fprintf(out, "K %zu %lu %d %lu %d %a %a\n", i, kf[i]->mnLoopQuery, kf[i]->mnLoopWords, kf[i]->mnRelocQuery,
                             kf[i]->mnRelocWords, (double)kf[i]->mLoopScore, (double)kf[i]->mRelocScore);
        }
        std::fclose(out);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
