// bow_math.hpp — the arithmetic of DBoW2's bag-of-words transform and L1 score (reference dependencies/DBoW2/DBoW2/TemplatedVocabulary.h
// :1126-1259, FORB.cpp:81-101, BowVector.cpp:34-84, ScoringObject.cpp:23-68), compiled for the device (bow.hip) and, by g++, for the host
// (bow_voc.hpp, tests/bow_prog.cpp).  Every sum is in the reference's order: tests/bow_restatement.py restates it in numpy, bit for bit.
//   * distance: popcount of the XOR over eight 32-bit words (an int; the reference widens it to double only to compare it);
//   * the best child under strict `<`: the smallest (distance << 8 | child index) — k <= 20 and a distance <= 256 both fit;
//   * a word's value: the idf weight added once per occurrence (BowVector::addWeight), never weight * count;
//   * the L1 norm: |value| summed in ascending word order; each value divided by it when it is > 0;
//   * the L1 score: the terms |v - w| - |v| - |w| of the shared words added in ascending word order, then -sum / 2.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef SIVO_HD
#ifdef __HIPCC__
#define SIVO_HD __host__ __device__ inline
#else
#define SIVO_HD inline
#endif
#endif

namespace sivo {

constexpr int BOW_MAX_K = 20;            // TemplatedVocabulary.h:1359
constexpr int BOW_MAX_L = 10;
constexpr int BOW_SET_CAP = 8192;        // features of one set (the reference extracts 2000), words of one stored / query vector

// The vocabulary as the descent reads it.  Node 0 is the root; the children of node p are the entries kids[p].x .. kids[p].x + kids[p].y - 1
// of cdesc / cnode, in file order.
struct BowKids { int32_t first, count; };
struct BowVocView {
    const BowKids *kids;       // per node
    const uint32_t *cdesc;     // per child entry: 8 words (32 bytes), 32-byte aligned
    const int32_t *cnode;      // per child entry: the child's node id
    const int32_t *word;       // per node: word id, -1 for an inner node
    const double *weight;      // per node
    int32_t L;
};

SIVO_HD int bow_popcount(uint32_t v) { return __builtin_popcount(v); }

SIVO_HD int bow_distance(const uint32_t *a, const uint32_t *b) {
    int d = 0;
    for (int i = 0; i < 8; ++i) d += bow_popcount(a[i] ^ b[i]);
    return d;
}

SIVO_HD uint32_t bow_child_key(int dist, int child) { return ((uint32_t)dist << 8) | (uint32_t)child; }

// The node id reported for a feature: 0 when the requested level is the root's or above it, the node passed at that level, and the
// leaf's own id when the descent ended above the level (the reference leaves the value uninitialised there).
SIVO_HD void bow_descend(const BowVocView &v, const uint32_t *f, int levelsup, int32_t &leaf, int32_t &nid) {
    const int nid_level = v.L - levelsup;
    int32_t node = 0, at = nid_level <= 0 ? 0 : -1;
    int level = 0;
    for (;;) {
        const BowKids k = v.kids[node];
        if (k.count == 0) break;
        ++level;
        uint32_t best = 0xFFFFFFFFu;
        for (int c = 0; c < k.count; ++c) {
            const uint32_t key = bow_child_key(bow_distance(f, v.cdesc + 8 * (int64_t)(k.first + c)), c);
            best = key < best ? key : best;
        }
        node = v.cnode[k.first + (int)(best & 0xFFu)];
        if (level == nid_level) at = node;
    }
    leaf = node;
    nid = at < 0 ? node : at;
}

SIVO_HD bool bow_stopped(double weight) { return !(weight > 0); }

SIVO_HD double bow_repeat_add(double w, int count) {
    double v = w;
    for (int i = 1; i < count; ++i) v += w;
    return v;
}

SIVO_HD double bow_l1_norm(const double *values, int n) {
    double norm = 0.0;
    for (int i = 0; i < n; ++i) norm += fabs(values[i]);
    return norm;
}

// index of `w` in the ascending array `words`, or -1
SIVO_HD int bow_find(const int32_t *words, int n, int32_t w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (words[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && words[lo] == w ? lo : -1;
}

SIVO_HD double bow_l1_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }
SIVO_HD double bow_l1_finish(double sum) { return -sum / 2.0; }

}  // namespace sivo
