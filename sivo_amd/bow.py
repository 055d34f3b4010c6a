"""Python mirror of the place-recognition entry points of the C ABI: DBoW2's vocabulary and transform (reference
dependencies/DBoW2/DBoW2/TemplatedVocabulary.h:1126-1259, :1338-1424) and the stored BowVectors of KeyFrameDatabase
(src/orbslam/KeyFrameDatabase.cc:72-322).  The vocabulary loads on the host; sivo_bow_transform / sivo_bowdb_query run on the device."""
import ctypes as C
import os

import numpy as np

from ._lib import check, lib

SET_CAP = 8192


def _ptr(a):
    return a.ctypes.data if a.size else None


class Vocabulary:
    """A k-ary vocabulary tree of 32-byte descriptors (L1_NORM scoring, TF_IDF weighting: the header `k L 0 0`)."""

    def __init__(self, handle, L):
        self._L, self._h = L, handle
        k, lv, nodes, words = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        check(L.sivo_voc_info(handle, C.byref(k), C.byref(lv), C.byref(nodes), C.byref(words)))
        self.k, self.L, self.n_nodes, self.n_words = k.value, lv.value, nodes.value, words.value

    @classmethod
    def from_text(cls, path):
        """The text format of TemplatedVocabulary::loadFromTextFile (what ORBvoc.txt is)."""
        L, h = lib(), C.c_void_p()
        check(L.sivo_voc_create_from_text(os.fspath(path).encode(), C.byref(h)))
        return cls(h, L)

    @classmethod
    def from_arrays(cls, k, L_levels, parent, is_leaf, desc, weight):
        """Entry i describes node i + 1: its parent's id, whether it is a word, its 32 descriptor bytes and its weight."""
        parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
        n = parent.shape[0]
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8).reshape(-1)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, np.float64).reshape(-1)
        if not (is_leaf.shape[0] == desc.shape[0] == weight.shape[0] == n):
            raise ValueError("parent, is_leaf, desc and weight describe different node counts")
        L, h = lib(), C.c_void_p()
        check(L.sivo_voc_create(int(k), int(L_levels), n, _ptr(parent), _ptr(is_leaf), _ptr(desc), _ptr(weight), C.byref(h)))
        return cls(h, L)

    def __len__(self):
        return self.n_words

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.sivo_voc_destroy(self._h)
            self._h = None

    def transform_batch(self, sets, levelsup=4):
        """Several descriptor sets ((n_i, 32) uint8 each) in one call.  Returns one dict per set: words (ascending) and values (the
        BowVector), fv_nodes / fv_offsets / fv_features (the FeatureVector in CSR form), word and node (per feature)."""
        sets = [np.ascontiguousarray(s, np.uint8).reshape(-1, 32) for s in sets]
        S = len(sets)
        if S == 0:
            return []
        off = np.zeros(S + 1, np.int64)
        off[1:] = np.cumsum([s.shape[0] for s in sets])
        T = int(off[-1])
        desc = np.concatenate(sets) if T else np.zeros((0, 32), np.uint8)
        i32 = lambda n: np.zeros(max(n, 1), np.int32)
        word, node, bw, fn, ff, fo = i32(T), i32(T), i32(T), i32(T), i32(T), i32(T + S)
        bv = np.zeros(max(T, 1), np.float64)
        nw, nf = i32(S), i32(S)
        check(self._L.sivo_bow_transform_batch(self._h, _ptr(desc), off.ctypes.data, S, int(levelsup), word.ctypes.data, node.ctypes.data,
                                                bw.ctypes.data, bv.ctypes.data, nw.ctypes.data, fn.ctypes.data, fo.ctypes.data,
                                                ff.ctypes.data, nf.ctypes.data))
        out = []
        for s in range(S):
            o, e = int(off[s]), int(off[s + 1])
            offs = fo[o + s:o + s + nf[s] + 1].copy()
            out.append({"words": bw[o:o + nw[s]].copy(), "values": bv[o:o + nw[s]].copy(), "fv_nodes": fn[o:o + nf[s]].copy(),
                        "fv_offsets": offs, "fv_features": ff[o:o + int(offs[-1])].copy(), "word": word[o:e].copy(), "node": node[o:e].copy()})
        return out

    def transform(self, desc, levelsup=4):
        """transform(features, BowVector &, FeatureVector &, levelsup) for an (n, 32) uint8 descriptor matrix."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = desc.shape[0]
        i32 = lambda m: np.zeros(max(m, 1), np.int32)
        word, node, bw, fn, ff, fo = i32(n), i32(n), i32(n), i32(n), i32(n), i32(n + 1)
        bv = np.zeros(max(n, 1), np.float64)
        nw, nf = C.c_int32(), C.c_int32()
        check(self._L.sivo_bow_transform(self._h, _ptr(desc), n, int(levelsup), word.ctypes.data, node.ctypes.data, bw.ctypes.data,
                                          bv.ctypes.data, C.byref(nw), fn.ctypes.data, fo.ctypes.data, ff.ctypes.data, C.byref(nf)))
        offs = fo[:nf.value + 1].copy()
        return {"words": bw[:nw.value].copy(), "values": bv[:nw.value].copy(), "fv_nodes": fn[:nf.value].copy(), "fv_offsets": offs,
                "fv_features": ff[:int(offs[-1])].copy(), "word": word[:n].copy(), "node": node[:n].copy()}


class BowDatabase:
    """The BowVectors of the keyframes in the database, resident on the device; a query is one launch over all of them."""

    def __init__(self, voc):
        self._L, self._voc, self._h = voc._L, voc, C.c_void_p()
        check(self._L.sivo_bowdb_create(voc._h, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.sivo_bowdb_destroy(self._h)
            self._h = None

    def __len__(self):
        n = C.c_int32()
        check(self._L.sivo_bowdb_size(self._h, C.byref(n)))
        return n.value

    def add(self, words, values):
        """Stores one BowVector (word ids ascending); returns its slot."""
        words = np.ascontiguousarray(words, np.int32).reshape(-1)
        values = np.ascontiguousarray(values, np.float64).reshape(-1)
        if words.shape != values.shape:
            raise ValueError("words and values differ in length")
        slot = C.c_int32()
        check(self._L.sivo_bowdb_add(self._h, _ptr(words), _ptr(values), words.shape[0], C.byref(slot)))
        return slot.value

    def erase(self, slot):
        check(self._L.sivo_bowdb_erase(self._h, int(slot)))

    def clear(self):
        check(self._L.sivo_bowdb_clear(self._h))

    def query(self, words, values):
        """Per slot: common (shared words; 0 for an erased slot), first_word (the smallest shared word id, -1: none), score (float64)."""
        words = np.ascontiguousarray(words, np.int32).reshape(-1)
        values = np.ascontiguousarray(values, np.float64).reshape(-1)
        if words.shape != values.shape:
            raise ValueError("words and values differ in length")
        n = len(self)
        common, first, score = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
        got = C.c_int32()
        check(self._L.sivo_bowdb_query(self._h, _ptr(words), _ptr(values), words.shape[0], common.ctypes.data, first.ctypes.data,
                                        score.ctypes.data, C.byref(got)))
        return {"common": common[:got.value].copy(), "first_word": first[:got.value].copy(), "score": score[:got.value].copy()}
