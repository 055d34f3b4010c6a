// bow_host_capi.hpp — the sivo_voc_* / sivo_bow_transform / sivo_bowdb_* entry points of include/sivo_hip.h over the HOST path of
// sivo_amd/csrc/bow_voc.hpp (bow_transform_host, bow_query_host: the arithmetic of the kernels, one lane), with the argument checks and the
// slot rules of sivo_amd/csrc/bow.hip.  tests/bow_adapter_prog.cpp built with -DSIVO_BOW_ON_HOST includes it in place of the library, so
// that SIVO::ORBVocabulary and SIVO::KeyFrameDatabase (sivo_amd/api/orbslam) run without a device: tests/test_pin_bow_database.py holds
// them to the reference's own KeyFrameDatabase.cc there.  This is NOT tests/bow_prog.cpp (that program's per-slot query is held to the
// reference by a test of its own); the slot and argument rules below restate bow.hip's and have to be kept in step with it by hand --
// what is under test through this header is bow_query_host / bow_transform_host and the adapter's host logic.
#pragma once
#include <string>

#include "../include/sivo_hip.h"
#include "bow_voc.hpp"

struct sivo_bowdb {
    int n_words = 0;
    struct Slot { std::vector<int32_t> w; std::vector<double> v; bool live; };
    std::vector<Slot> slots;
};

namespace bow_host_capi {
inline std::string &last_error() { static thread_local std::string s; return s; }
template <class Fn> int guarded(Fn fn) {
    try {
        return fn();
    } catch (const std::invalid_argument &e) {
        last_error() = e.what();
        return SIVO_ERR_INVALID_ARGUMENT;
    } catch (const std::exception &e) {
        last_error() = e.what();
        return SIVO_ERR_RUNTIME;
    }
}
}  // namespace bow_host_capi

extern "C" {

const char *sivo_last_error(void) { return bow_host_capi::last_error().c_str(); }

int sivo_voc_create_from_text(const char *path, sivo_voc_t *voc) {
    return bow_host_capi::guarded([&] {
        if (!voc) throw std::invalid_argument("null argument");
        *voc = nullptr;
        sivo_voc *v = new sivo_voc;
        try {
            sivo::bow_load_text(path, v->img);
        } catch (...) {
            delete v;
            throw;
        }
        *voc = v;
        return SIVO_OK;
    });
}

int sivo_voc_info(sivo_voc_t voc, int32_t *k, int32_t *L, int64_t *n_nodes, int64_t *n_words) {
    if (!voc) return SIVO_ERR_INVALID_ARGUMENT;
    if (k) *k = voc->img.k;
    if (L) *L = voc->img.L;
    if (n_nodes) *n_nodes = voc->img.n_nodes();
    if (n_words) *n_words = voc->img.n_words;
    return SIVO_OK;
}

int sivo_voc_destroy(sivo_voc_t voc) {
    delete voc;
    return SIVO_OK;
}

int sivo_bow_transform(sivo_voc_t voc, const uint8_t *desc, int n, int levelsup, int32_t *word, int32_t *node, int32_t *bow_words,
                       double *bow_values, int32_t *n_words, int32_t *fv_nodes, int32_t *fv_offsets, int32_t *fv_features, int32_t *n_fv_nodes) {
    return bow_host_capi::guarded([&] {
        if (!voc || !n_words || !n_fv_nodes) throw std::invalid_argument("null argument");
        if (n < 0 || n > sivo::BOW_SET_CAP || levelsup < 0) throw std::invalid_argument("feature count or levelsup out of range");
        sivo::BowSet o;
        sivo::bow_transform_host(voc->img.view(), desc, n, levelsup, o);
        std::copy(o.word.begin(), o.word.end(), word);
        std::copy(o.node.begin(), o.node.end(), node);
        std::copy(o.bow_words.begin(), o.bow_words.end(), bow_words);
        std::copy(o.bow_values.begin(), o.bow_values.end(), bow_values);
        std::copy(o.fv_nodes.begin(), o.fv_nodes.end(), fv_nodes);
        std::copy(o.fv_off.begin(), o.fv_off.end(), fv_offsets);
        std::copy(o.fv_feat.begin(), o.fv_feat.end(), fv_features);
        *n_words = (int32_t)o.bow_words.size();
        *n_fv_nodes = (int32_t)o.fv_nodes.size();
        return SIVO_OK;
    });
}

int sivo_bowdb_create(sivo_voc_t voc, sivo_bowdb_t *db) {
    if (!voc || !db) return SIVO_ERR_INVALID_ARGUMENT;
    *db = new sivo_bowdb;
    (*db)->n_words = voc->img.n_words;
    return SIVO_OK;
}

int sivo_bowdb_destroy(sivo_bowdb_t db) {
    delete db;
    return SIVO_OK;
}

int sivo_bowdb_add(sivo_bowdb_t db, const int32_t *words, const double *values, int n, int32_t *slot) {
    return bow_host_capi::guarded([&] {
        if (!db || !slot) throw std::invalid_argument("null argument");
        sivo::bow_check_vector(words, values, n, db->n_words);
        *slot = (int32_t)db->slots.size();
        db->slots.push_back(sivo_bowdb::Slot{std::vector<int32_t>(words, words + n), std::vector<double>(values, values + n), true});
        return SIVO_OK;
    });
}

int sivo_bowdb_erase(sivo_bowdb_t db, int32_t slot) {
    return bow_host_capi::guarded([&] {
        if (!db) throw std::invalid_argument("null argument");
        if (slot < 0 || (size_t)slot >= db->slots.size() || !db->slots[(size_t)slot].live)
            throw std::invalid_argument("keyframe database: no such slot");
        db->slots[(size_t)slot] = sivo_bowdb::Slot{{}, {}, false};       // a tombstone: no words
        return SIVO_OK;
    });
}

int sivo_bowdb_clear(sivo_bowdb_t db) {
    if (!db) return SIVO_ERR_INVALID_ARGUMENT;
    db->slots.clear();
    return SIVO_OK;
}

int sivo_bowdb_query(sivo_bowdb_t db, const int32_t *q_words, const double *q_values, int nq, int32_t *common, int32_t *first_word,
                     double *score, int32_t *n_slots) {
    return bow_host_capi::guarded([&] {
        if (!db || !n_slots) throw std::invalid_argument("null argument");
        sivo::bow_check_vector(q_words, q_values, nq, db->n_words);
        *n_slots = (int32_t)db->slots.size();
        if (db->slots.empty()) return SIVO_OK;
        if (!common || !first_word || !score) throw std::invalid_argument("null argument");
        for (size_t s = 0; s < db->slots.size(); ++s) {
            const sivo_bowdb::Slot &e = db->slots[s];
            sivo::bow_query_host(q_words, q_values, nq, e.w.data(), e.v.data(), (int)e.w.size(), common[s], first_word[s], score[s]);
        }
        return SIVO_OK;
    });
}

}  // extern "C"
