// bow_score_prog.cpp — SIVO::ORBVocabulary::score on the host (no device: the ordered L1 arithmetic over two std::maps), as a stand-alone
// program for tests/test_bow_host.py, built through tests/host_prog.py against libsivo_hip.
//   bow_score_prog <pairs.txt>      pairs of vectors: n, n x (word value-as-hex-float), twice per line group  -> one score per pair as %a
#include <cstdio>
#include "orbslam/ORBVocabulary.h"
int main(int argc, char **argv) {
    SIVO::ORBVocabulary voc;
    std::FILE *f = std::fopen(argv[argc - 1], "r");
    int n;
    while (f && std::fscanf(f, "%d", &n) == 1) {
        DBoW2::BowVector v[2];
        for (int k = 0; k < 2; ++k) {
            if (k && std::fscanf(f, "%d", &n) != 1) return 1;
            for (int i = 0; i < n; ++i) { unsigned w; double x; if (std::fscanf(f, "%u %la", &w, &x) != 2) return 1; v[k][w] = x; }
        }
        std::printf("%a\n", voc.score(v[0], v[1]));
    }
    return voc.empty() && voc.size() == 0 ? 0 : 1;
}
