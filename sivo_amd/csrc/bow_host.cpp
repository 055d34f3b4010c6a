// bow_host.cpp — the vocabulary handle of the C ABI: the loader of DBoW2's text format and the constructor from arrays (bow_voc.hpp) behind
// sivo_voc_create*, sivo_voc_info, sivo_voc_destroy.  No device is touched here except to free the image bow.hip uploaded.
#include "bow_voc.hpp"
#include "common.hpp"

using namespace sivo;

extern "C" int sivo_voc_create_from_text(const char *path, sivo_voc_t *voc) {
    return guarded([&] {
        if (!voc) throw std::invalid_argument("null argument");
        *voc = nullptr;
        sivo_voc *v = new sivo_voc;
        try {
            bow_load_text(path, v->img);
        } catch (...) {
            delete v;
            throw;
        }
        *voc = v;
        return SIVO_OK;
    });
}

extern "C" int sivo_voc_create(int k, int L, int64_t n_nodes, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc,
                               const double *weight, sivo_voc_t *voc) {
    return guarded([&] {
        if (!voc) throw std::invalid_argument("null argument");
        *voc = nullptr;
        sivo_voc *v = new sivo_voc;
        try {
            bow_build_image(k, L, n_nodes, parent, is_leaf, desc, weight, v->img);
        } catch (...) {
            delete v;
            throw;
        }
        *voc = v;
        return SIVO_OK;
    });
}

extern "C" int sivo_voc_info(sivo_voc_t voc, int32_t *k, int32_t *L, int64_t *n_nodes, int64_t *n_words) {
    return guarded([&] {
        if (!voc) throw std::invalid_argument("null argument");
        if (k) *k = voc->img.k;
        if (L) *L = voc->img.L;
        if (n_nodes) *n_nodes = voc->img.n_nodes();
        if (n_words) *n_words = voc->img.n_words;
        return SIVO_OK;
    });
}

extern "C" int sivo_voc_destroy(sivo_voc_t voc) {
    return guarded([&] {
        if (!voc) return SIVO_OK;
        if (voc->d_base) {
            DeviceRestore keep;
            if (hipSetDevice(voc->device) == hipSuccess) (void)hipFree(voc->d_base);
        }
        delete voc;
        return SIVO_OK;
    });
}
