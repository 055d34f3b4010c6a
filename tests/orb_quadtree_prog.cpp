// orb_quadtree_prog.cpp — the device quadtree's steps (sivo_amd/csrc/orb_quadtree_math.hpp: the per-candidate and per-cell bodies and
// the driver that orders them, the very code the kernel of orb_quadtree.hip runs) walked one item after the other on the host, as a
// stand-alone program: `orb_quadtree_prog run IN OUT` reads a little-endian blob (tests/orb_quadtree_cases.py writes it) and writes
// what every set's list came to.  tests/test_orb_quadtree_host.py builds it through tests/host_prog.py, plain and under the
// sanitizers; every table has exactly the size the kernel gives it, so a step that leaves its table is a sanitizer report.
//
//   in : i32 n_sets, then per set: i32 n, i32 w, i32 h, i32 target, u32 words[n] (x:12 | y:12 | response:8)
//   out: per set: i32 status, i32 count, i32 rounds, i32 passes, i32 stop, u32 kept_words[count], i32 kept_index[count]
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "orb_quadtree_math.hpp"

namespace {

struct Walk {
    template <class F> void each(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    void zero(int32_t *p) { *p = 0; }
    uint32_t scan(uint32_t *a, int n) {
        uint32_t run = 0;
        for (int i = 0; i < n; ++i) { const uint32_t t = a[i]; a[i] = run; run += t; }
        return run;
    }
};

int run(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "run") throw BlobUsage();
    BlobReader r(argv[2]);
    BlobWriter w;
    const int32_t n_sets = r.one<int32_t>();
    for (int32_t s = 0; s < n_sets; ++s) {
        using namespace sivo;
        const int32_t n = r.one<int32_t>();
        QtSet set{};
        set.w = r.one<int32_t>(); set.h = r.one<int32_t>(); set.target = r.one<int32_t>();
        if (n < 0 || set.w < 1 || set.h < 1 || set.w > QT_MAX_EXTENT || set.h > QT_MAX_EXTENT) throw std::runtime_error("bad set");
        const std::vector<uint32_t> words = r.many<uint32_t>((size_t)n);
        set.n_ini = (int)std::round((float)set.w / set.h);
        set.h_x = set.n_ini > 0 ? (float)set.w / set.n_ini : 0.f;
        const size_t C = (size_t)QT_MAX_CELLS;
        std::vector<QtCell> cells0(C), cells1(C);
        std::vector<int32_t> cnt4(C * 4);
        std::vector<uint32_t> sc(C), sk(C);
        std::vector<uint16_t> g0(C), g1(C), srt(C), rk(C), cid((size_t)n);
        int32_t below = 0;
        QtState S{};
        S.word = words.data(); S.cid = cid.data(); S.n = n;
        S.cur = cells0.data(); S.nxt = cells1.data();
        S.cnt4 = reinterpret_cast<int32_t(*)[4]>(cnt4.data());
        S.sc = sc.data(); S.sk = sk.data(); S.grown = g0.data(); S.grown_nxt = g1.data(); S.srt = srt.data(); S.rk = rk.data();
        S.below = &below;
        Walk x;
        int32_t count = 0;
        int32_t status = qt_cell_bound(set.target, set.n_ini) > QT_MAX_CELLS ? (int32_t)QT_ERR_CELLS : qt_distribute(x, S, set, &count);
        if (status != QT_OK) count = 0;
        const int32_t head[5] = {status, count, S.rounds, S.passes, S.stop};
        w.put(head, 5);
        std::vector<uint32_t> kept((size_t)count);
        std::vector<int32_t> index((size_t)count);
        for (int32_t j = 0; j < count; ++j) { index[(size_t)j] = S.cnt4[j][1]; kept[(size_t)j] = words.at((size_t)S.cnt4[j][1]); }
        w.put(kept); w.put(index);
    }
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "orb_quadtree_prog run IN OUT", run); }
