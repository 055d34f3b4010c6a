// local_mapping_prog.cpp — the arithmetic of the triangulation and map-point-refresh kernels (sivo_amd/csrc/triangulate_math.hpp,
// mappoint_math.hpp) compiled for the host: tests/test_local_mapping_host.py builds it through tests/host_prog.py (g++ -ffp-contract=off,
// plain and under the sanitizers) and compares what it writes with the numpy restatements bit for bit.  No device, no library.
//   local_mapping_prog tri IN OUT       IN: kf1 kf2 (SivoTriKeyFrame), ratio_factor (f32), pad (4 bytes), state_cov (36 f64), th_confidence,
//                                       th_entropy (f64), n (i64), n SivoTriMatch.  OUT: n status, n class, 3 n wP words.
//   local_mapping_prog refresh IN OUT   IN: np (i64), desc_off, obs_off (np + 1 i64 each), descriptors (32 bytes each), camera centres
//                                       (3 f32 each), np records pos[3] ref_ow[3] level_scale last_scale.  OUT: np best_idx (i32, -1: none),
//                                       5 np words (max, min, normal), np flags.
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "mappoint_math.hpp"
#include "triangulate_math.hpp"

using namespace sivo;

static int tri(BlobReader &in, BlobWriter &out) {
    SivoTriKeyFrame k[2];
    float rf[2];
    double cov[36], th[2];
    in.get(k, 2); in.get(rf, 2); in.get(cov, 36); in.get(th, 2);
    const int64_t n = in.one<int64_t>();
    if (n < 0) return 2;
    const std::vector<SivoTriMatch> m = in.many<SivoTriMatch>((size_t)n);
    std::vector<uint8_t> status((size_t)n), cls((size_t)n);
    std::vector<uint32_t> w(3 * (size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (m[i].octave1 < 0 || m[i].octave1 >= k[0].nlevels || m[i].octave2 < 0 || m[i].octave2 >= k[1].nlevels) return 3;
        TrResult o;
        tr_match(k[0], k[1], rf[0], cov, th[0], th[1], m[i], o);
        status[i] = o.status; cls[i] = o.cls;
        for (int c = 0; c < 3; ++c) w[3 * i + c] = tr_float_bits(o.wP[c]);
    }
    out.put(status); out.put(cls); out.put(w);
    return 0;
}

static int refresh(BlobReader &in, BlobWriter &out) {
    const int64_t np = in.one<int64_t>();
    if (np < 0) return 2;
    const std::vector<int64_t> doff = in.many<int64_t>((size_t)np + 1), ooff = in.many<int64_t>((size_t)np + 1);
    const std::vector<uint64_t> desc = in.many<uint64_t>(4 * (size_t)doff[np]);
    const std::vector<float> ow = in.many<float>(3 * (size_t)ooff[np]), pt = in.many<float>(8 * (size_t)np);
    std::vector<int32_t> best((size_t)np, -1);
    std::vector<uint32_t> geom(5 * (size_t)np, 0);
    std::vector<uint8_t> flags((size_t)np);
    for (int64_t p = 0; p < np; ++p) {
        const int64_t N = doff[p + 1] - doff[p], M = ooff[p + 1] - ooff[p];
        if (M == 0) { flags[p] = SIVO_MP_NO_OBSERVATION | SIVO_MP_NO_DESCRIPTOR; continue; }
        flags[p] = N > 0 ? 0 : SIVO_MP_NO_DESCRIPTOR;
        int64_t key = INT64_MAX;
        for (int64_t i = 0; i < N; ++i) {
            const int64_t k = ((int64_t)mp_row_median(desc.data() + 4 * doff[p], N, i) << 32) | i;
            key = k < key ? k : key;
        }
        if (N > 0) best[p] = (int32_t)(key & 0xFFFFFFFFll);
        float o[5];
        mp_normal_depth(&pt[8 * p], ow.data() + 3 * ooff[p], M, &pt[8 * p + 3], pt[8 * p + 6], pt[8 * p + 7], o);
        for (int c = 0; c < 5; ++c) geom[5 * p + c] = tr_float_bits(o[c]);
    }
    out.put(best); out.put(geom); out.put(flags);
    return 0;
}

// exit codes beside blob_main's: 2 a negative count, 3 an octave outside its keyframe's levels
static int run(int argc, char **argv) {
    if (argc != 4) throw BlobUsage();
    const std::string mode = argv[1];
    BlobReader in(argv[2]);
    BlobWriter out;
    const int rc = mode == "tri" ? tri(in, out) : mode == "refresh" ? refresh(in, out) : throw BlobUsage();
    out.save(argv[3]);
    return rc;
}

int main(int argc, char **argv) { return blob_main(argc, argv, "local_mapping_prog tri|refresh IN OUT", run); }
