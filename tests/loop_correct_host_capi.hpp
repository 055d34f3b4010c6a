// loop_correct_host_capi.hpp — sivo_loop_correct and sivo_gba_propagate of include/sivo_hip.h over the HOST build of the kernels' per-item
// bodies (sivo_amd/csrc/loopcorrect_math.hpp), with the argument checks of the library (the same functions of that header) and the results
// stored as loopcorrect.hip stores them (entries of untouched points and unreached keyframes left as the caller had them).  Sequential
// loops in place of the launches: no library, no device, so the programs that include it (tests/loop_correct_prog.cpp,
// tests/loop_correct_adapter_prog.cpp) can run under the sanitizers.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "loopcorrect_math.hpp"

namespace loop_correct_host {
inline std::string &error() { static std::string e; return e; }
inline int fail(const char *where, const char *what) { error() = std::string(where) + ": " + what; return SIVO_ERR_INVALID_ARGUMENT; }
inline long &calls() { static long n = 0; return n; }        // how many entry-point calls were made (the adapter's "one call" claims)
}  // namespace loop_correct_host

extern "C" {

const char *sivo_last_error(void) { return loop_correct_host::error().c_str(); }

int sivo_loop_correct(const SivoLoopCorrect *problem) {
    ++loop_correct_host::calls();
    if (const char *e = sivo::lc_check_loop_correct(problem)) return loop_correct_host::fail("sivo_loop_correct", e);
    const SivoLoopCorrect &a = *problem;
    const size_t K = (size_t)a.n_kf, P = (size_t)a.n_points;
    std::vector<double> cor_inv(8 * K);
    for (int i = 0; i < a.n_kf; ++i)
        sivo::lc_keyframe(a, i, a.noncorrected_siw + 8 * (size_t)i, a.corrected_siw + 8 * (size_t)i, cor_inv.data() + 8 * (size_t)i,
                          a.tiw_out + 16 * (size_t)i, a.ow_out + 3 * (size_t)i);
    // the ownership kernel: the largest n_kf - keyframe over the slots that hold the point
    std::vector<int32_t> code(P, 0);
    for (int i = 0; i < a.n_kf; ++i)
        for (int64_t s = a.slot_off[i]; s < a.slot_off[i + 1]; ++s) {
            const int32_t p = a.slot_point[s];
            if (p < 0 || a.skip[p]) continue;
            if (a.n_kf - i > code[(size_t)p]) code[(size_t)p] = a.n_kf - i;
        }
    for (size_t p = 0; p < P; ++p) {
        if (code[p] == 0) { a.corrected_by[p] = -1; continue; }
        const int32_t owner = a.n_kf - code[p];
        float pos[3], geom[5];
        const uint8_t f = sivo::lc_point(a, a.noncorrected_siw, cor_inv.data(), a.ow_out, owner, (int32_t)p, pos, geom);
        a.corrected_by[p] = owner;
        std::memcpy(a.pos_out + 3 * p, pos, 12);
        a.flags[p] = f;
        if (f & SIVO_MP_NO_OBSERVATION) continue;
        a.max_dist[p] = geom[0]; a.min_dist[p] = geom[1];
        std::memcpy(a.normal + 3 * p, geom + 2, 12);
    }
    return SIVO_OK;
}

int sivo_gba_propagate(const SivoGbaPropagate *problem) {
    ++loop_correct_host::calls();
    std::vector<int32_t> parent(problem && problem->n_kf > 0 && problem->n_kf <= (1 << 24) ? (size_t)problem->n_kf : 0);
    std::vector<uint8_t> kf_flags(parent.size());
    if (const char *e = sivo::lc_check_gba_propagate(problem, parent.data(), kf_flags.data())) return loop_correct_host::fail("sivo_gba_propagate", e);
    const SivoGbaPropagate &a = *problem;
    const size_t K = (size_t)a.n_kf, P = (size_t)a.n_points;
    std::vector<float> gba(16 * K), twc(16 * K);
    std::vector<uint8_t> reached(K), in_after(K);
    for (size_t k = 0; k < K; ++k)          // every keyframe from the inputs, as the kernel's threads do
        reached[k] = sivo::lc_tree_keyframe(a, parent.data(), kf_flags.data(), (int32_t)k, gba.data() + 16 * k, twc.data() + 16 * k, &in_after[k]);
    std::vector<float> pos(3 * P);
    std::vector<uint8_t> status(P);
    for (size_t p = 0; p < P; ++p) status[p] = sivo::lc_gba_point(a, reached.data(), twc.data(), in_after.data(), (int32_t)p, pos.data() + 3 * p);
    for (size_t k = 0; k < K; ++k) {
        a.kf_reached[k] = reached[k];
        if (!reached[k]) continue;
        float out[16];
        for (int i = 0; i < 16; ++i) out[i] = sivo::lc_canon(gba[16 * k + (size_t)i]);
        if (!a.in_gba[k] && in_after[k]) {
            std::memcpy(a.tcw_gba + 16 * k, out, 64);
            a.in_gba[k] = 1;
        }
        std::memcpy(a.tcw_bef + 16 * k, a.tcw + 16 * k, 64);
        std::memcpy(a.tcw_out + 16 * k, out, 64);
        for (int i = 0; i < 3; ++i) a.ow_out[3 * k + (size_t)i] = sivo::lc_canon(twc[16 * k + 4 * (size_t)i + 3]);
    }
    for (size_t p = 0; p < P; ++p) {
        a.point_status[p] = status[p];
        if (status[p] == SIVO_GBA_POINT_FROM_BA || status[p] == SIVO_GBA_POINT_CARRIED) std::memcpy(a.pos_out + 3 * p, pos.data() + 3 * p, 12);
    }
    return SIVO_OK;
}

}  // extern "C"
