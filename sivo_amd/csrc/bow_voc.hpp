// bow_voc.hpp — the vocabulary on the host: the image the device reads (bow_math.hpp's BowVocView over std::vectors), its two
// constructors — from arrays and from the text format of TemplatedVocabulary::loadFromTextFile (reference TemplatedVocabulary.h:1338-1424)
// — and the single-lane host path of the transform and the database query, the same arithmetic as the kernels.  Plain C++: g++ compiles
// it into tests/bow_prog.cpp, hipcc into bow_host.cpp.
//
// Two guards beyond the reference ("Place recognition"): empty lines are skipped (the reference's `while(!f.eof())`
// turns a trailing newline into a phantom child of the root), and every line is checked — a parent id that is not an earlier inner
// node, a parent with more than k children, a line with fewer than 35 fields, an inner node without children: std::invalid_argument.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "bow_math.hpp"

namespace sivo {

struct BowVocImage {
    int k = 0, L = 0, n_words = 0;
    std::vector<BowKids> kids;
    std::vector<uint32_t> cdesc;
    std::vector<int32_t> cnode, word;
    std::vector<double> weight;
    int n_nodes() const { return (int)kids.size(); }                 // the root included
    BowVocView view() const { return BowVocView{kids.data(), cdesc.data(), cnode.data(), word.data(), weight.data(), L}; }
};

inline void bow_check_header(int k, int L, int scoring, int weighting) {
    if (k < 0 || k > BOW_MAX_K || L < 1 || L > BOW_MAX_L || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3)
        throw std::invalid_argument("vocabulary: k outside 0 .. 20, L outside 1 .. 10 or an unknown scoring / weighting type");
    if (scoring != 0 || weighting != 0)
        throw std::invalid_argument("vocabulary: only L1_NORM scoring with TF_IDF weighting (header `k L 0 0`) is supported");
}

// Entry i of the arrays is node i + 1 (file order); n entries.
inline void bow_build_image(int k, int L, int64_t n, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc, const double *weight,
                            BowVocImage &img) {
    bow_check_header(k, L, 0, 0);
    if (n < 0 || n > (int64_t)1 << 30) throw std::invalid_argument("vocabulary: node count out of range");
    if (n > 0 && (!parent || !is_leaf || !desc || !weight)) throw std::invalid_argument("null argument");
    const int64_t N = n + 1;
    img = BowVocImage();
    img.k = k; img.L = L;
    img.kids.assign((size_t)N, BowKids{0, 0});
    img.word.assign((size_t)N, -1);
    img.weight.assign((size_t)N, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = i + 1, p = parent[i];
        if (p < 0 || p >= id || (p > 0 && is_leaf[p - 1]))
            throw std::invalid_argument("vocabulary: node " + std::to_string(id) + ": the parent id is not an earlier inner node");
        if (++img.kids[(size_t)p].count > k)
            throw std::invalid_argument("vocabulary: node " + std::to_string(p) + " has more than k children");
        img.weight[(size_t)id] = weight[i];
        if (is_leaf[i]) img.word[(size_t)id] = img.n_words++;        // :1408-1415: word ids in file order over the leaf lines
    }
    int32_t at = 0;
    for (int64_t p = 0; p < N; ++p) {
        if (img.word[(size_t)p] < 0 && img.kids[(size_t)p].count == 0)
            throw std::invalid_argument("vocabulary: inner node " + std::to_string(p) + " has no children");
        img.kids[(size_t)p].first = at;
        at += img.kids[(size_t)p].count;
    }
    img.cdesc.assign(8 * (size_t)n, 0u);
    img.cnode.assign((size_t)n, 0);
    std::vector<int32_t> fill((size_t)N, 0);
    for (int64_t i = 0; i < n; ++i) {                                 // ascending node id: a node's children keep file order
        const int32_t p = parent[i];
        const int32_t e = img.kids[(size_t)p].first + fill[(size_t)p]++;
        std::memcpy(&img.cdesc[8 * (size_t)e], desc + 32 * i, 32);
        img.cnode[(size_t)e] = (int32_t)(i + 1);
    }
}

inline void bow_parse_text(const char *text, size_t size, BowVocImage &img) {
    const char *p = text, *end = text + size;
    auto next_line = [&](const char *&b, const char *&e) {          // the next line that holds anything but white space
        while (p < end) {
            b = p;
            while (p < end && *p != '\n') ++p;
            e = p;
            if (p < end) ++p;
            for (const char *q = b; q < e; ++q)
                if (*q != ' ' && *q != '\t' && *q != '\r') return true;
        }
        return false;
    };
    const char *b, *e;
    if (!next_line(b, e)) throw std::invalid_argument("vocabulary: the file is empty");
    std::string line(b, e);
    long h[4];
    {
        char *q = &line[0];
        for (int i = 0; i < 4; ++i) {
            char *r;
            h[i] = std::strtol(q, &r, 10);
            if (r == q) throw std::invalid_argument("vocabulary: the header line is not `k L scoring weighting`");
            q = r;
        }
    }
    bow_check_header((int)std::max(-1L, std::min(h[0], 1000L)), (int)std::max(-1L, std::min(h[1], 1000L)), (int)std::max(-1L, std::min(h[2], 1000L)),
                     (int)std::max(-1L, std::min(h[3], 1000L)));
    std::vector<int32_t> parent;
    std::vector<uint8_t> leaf, desc;
    std::vector<double> weight;
    while (next_line(b, e)) {
        line.assign(b, e);
        char *q = &line[0], *r;
        long v[34];
        for (int i = 0; i < 34; ++i) {
            v[i] = std::strtol(q, &r, 10);
            if (r == q) throw std::invalid_argument("vocabulary: node line " + std::to_string(parent.size() + 1) + " is truncated");
            q = r;
        }
        const double w = std::strtod(q, &r);
        if (r == q) throw std::invalid_argument("vocabulary: node line " + std::to_string(parent.size() + 1) + " is truncated");
        parent.push_back((int32_t)std::max(-1L, std::min(v[0], 0x7FFFFFFFL)));
        leaf.push_back(v[1] > 0);
        for (int i = 0; i < 32; ++i) desc.push_back((uint8_t)v[2 + i]);
        weight.push_back(w);
    }
    bow_build_image((int)h[0], (int)h[1], (int64_t)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data(), img);
}

inline void bow_load_text(const char *path, BowVocImage &img) {
    if (!path) throw std::invalid_argument("null argument");
    std::FILE *f = std::fopen(path, "rb");
    if (!f) throw std::invalid_argument(std::string("vocabulary: cannot open ") + path);
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    std::fclose(f);
    bow_parse_text(text.data(), text.size(), img);
}

// ---------------------------------------------------------------------------------------------------------------------
// the host path: what the kernels compute, one lane
// ---------------------------------------------------------------------------------------------------------------------
struct BowSet {
    std::vector<int32_t> word, node;                 // per feature
    std::vector<int32_t> bow_words;                  // ascending
    std::vector<double> bow_values;
    std::vector<int32_t> fv_nodes, fv_off, fv_feat;  // CSR: nodes ascending, fv_off has fv_nodes.size() + 1 entries
};

inline void bow_transform_host(const BowVocView &v, const uint8_t *desc, int n, int levelsup, BowSet &o) {
    o = BowSet();
    o.word.resize((size_t)n); o.node.resize((size_t)n);
    std::vector<uint64_t> kw, kn;
    std::vector<int32_t> leaf((size_t)n);
    for (int i = 0; i < n; ++i) {
        uint32_t f[8];
        std::memcpy(f, desc + 32 * (size_t)i, 32);
        bow_descend(v, f, levelsup, leaf[(size_t)i], o.node[(size_t)i]);
        o.word[(size_t)i] = v.word[leaf[(size_t)i]];
        if (bow_stopped(v.weight[leaf[(size_t)i]])) continue;
        kw.push_back(((uint64_t)(uint32_t)o.word[(size_t)i] << 32) | (uint32_t)i);
        kn.push_back(((uint64_t)(uint32_t)o.node[(size_t)i] << 32) | (uint32_t)i);
    }
    std::sort(kw.begin(), kw.end());
    std::sort(kn.begin(), kn.end());
    const size_t m = kw.size();
    for (size_t i = 0; i < m;) {
        size_t j = i;
        while (j < m && (kw[j] >> 32) == (kw[i] >> 32)) ++j;
        o.bow_words.push_back((int32_t)(kw[i] >> 32));
        o.bow_values.push_back(bow_repeat_add(v.weight[leaf[(uint32_t)kw[i]]], (int)(j - i)));
        i = j;
    }
    const double norm = bow_l1_norm(o.bow_values.data(), (int)o.bow_values.size());
    if (norm > 0.0)
        for (double &x : o.bow_values) x /= norm;
    for (size_t i = 0; i < m; ++i) {
        if (i == 0 || (kn[i] >> 32) != (kn[i - 1] >> 32)) {
            o.fv_nodes.push_back((int32_t)(kn[i] >> 32));
            o.fv_off.push_back((int32_t)i);
        }
        o.fv_feat.push_back((int32_t)(uint32_t)kn[i]);
    }
    o.fv_off.push_back((int32_t)m);
}

// one stored vector against the query: shared words, the smallest of them (-1: none), the L1 score
inline void bow_query_host(const int32_t *qw, const double *qv, int nq, const int32_t *sw, const double *sv, int ns, int32_t &common,
                           int32_t &first_word, double &score) {
    common = 0; first_word = -1;
    double sum = 0.0;
    for (int i = 0, j = 0; i < nq && j < ns;) {                      // both ascend: one walk (the device looks each stored word up instead)
        if (qw[i] < sw[j]) { ++i; continue; }
        if (qw[i] > sw[j]) { ++j; continue; }
        if (!common++) first_word = sw[j];
        sum += bow_l1_term(qv[i], sv[j]);
        ++i; ++j;
    }
    score = bow_l1_finish(sum);
}

inline void bow_check_vector(const int32_t *words, const double *values, int n, int n_words) {
    if (n < 0 || n > BOW_SET_CAP) throw std::invalid_argument("bow vector: more than 8192 words, or a negative count");
    if (n > 0 && (!words || !values)) throw std::invalid_argument("null argument");
    for (int i = 0; i < n; ++i)
        if (words[i] < 0 || words[i] >= n_words || (i > 0 && words[i] <= words[i - 1]))
            throw std::invalid_argument("bow vector: word ids must ascend strictly and lie inside the vocabulary");
}

}  // namespace sivo

// The handle behind sivo_voc_t: the host image, and its copy on the device of the first call that needed one (bow.hip).
struct sivo_voc {
    sivo::BowVocImage img;
    std::mutex mutex;
    int device = -1;
    void *d_base = nullptr;
    sivo::BowVocView dev{};
};
