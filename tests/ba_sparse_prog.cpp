// ba_sparse_prog.cpp — stand-alone: the sparse reduced camera system of the bundle adjustment planned, assembled, factored and solved on
// the host (tests/ba_sparse_host_capi.hpp) for tests/test_ba_sparse_host.py.
//   ba_sparse_prog solve IN OUT
// IN  (little-endian): int32 nP, nX, nE; f64 lambda; u8 fixed[nP]; u8 level[nE]; SivoEdge edges[nE]; f64 W[18 nE], Hll[9 nX], bl[3 nX],
//     Hpp[36 nF], bp[6 nF]  (nF = the poses that are not fixed, in pose order)
// OUT: int32 nF, n_own, nL - nF, levels, ok; int32 (row slot, col slot)[n_own]; f64 S[36 n_own], rhs[6 nF], x[6 nF]
#include <cstdint>
#include <cstring>

#include "ba_sparse_host_capi.hpp"
#include "blob_io.hpp"

static int run(int argc, char **argv) {
    if (argc != 4 || std::strcmp(argv[1], "solve") != 0) throw BlobUsage();
    BlobReader in(argv[2]);
    ba_sparse_host::Problem p;
    p.nP = in.one<int32_t>(); p.nX = in.one<int32_t>(); p.nE = in.one<int32_t>();
    if (p.nP < 0 || p.nX < 0 || p.nE < 0) throw std::runtime_error("negative count");
    p.lambda = in.one<double>();
    p.fixed = in.many<uint8_t>((size_t)p.nP);
    p.level = in.many<uint8_t>((size_t)p.nE);
    p.edges = in.many<SivoEdge>((size_t)p.nE);
    size_t nF = 0;
    for (uint8_t f : p.fixed) nF += f ? 0 : 1;
    p.W = in.many<double>(18 * (size_t)p.nE);
    p.Hll = in.many<double>(9 * (size_t)p.nX);
    p.bl = in.many<double>(3 * (size_t)p.nX);
    p.Hpp = in.many<double>(36 * nF);
    p.bp = in.many<double>(6 * nF);
    ba_sparse_host::Result R;
    ba_sparse_host::solve(p, R);
    BlobWriter out;
    const int32_t head[5] = {R.nF, (int32_t)R.plan.own_blk.size(), R.plan.pat.nL - R.nF, R.plan.pat.nlev, R.ok};
    out.put(head, 5);
    out.put(R.own_rc);
    out.put(R.S);
    out.put(R.rhs);
    out.put(R.x);
    out.save(argv[3]);
    return 0;
}

int main(int argc, char **argv) { return blob_main(argc, argv, "ba_sparse_prog solve IN OUT", run); }
