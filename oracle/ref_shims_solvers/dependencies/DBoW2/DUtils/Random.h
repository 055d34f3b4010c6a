// Stand-in for DBoW2's DUtils/Random.h when the reference's PnPsolver.cc / Sim3Solver.cc are compiled for oracle/_ref: RandomInt
// reads the draw list the driver scripted for the solver it is about to call (value k of the list folded into [min, max], the
// rule of the SetDraw functors in tests/pnp_ransac_prog.cpp and tests/sim3_ransac_prog.cpp), so the reference and this
// repository's classes can be given the same samples.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace DUtils {
class Random {
 public:
    struct Script {
        std::vector<int> draws;
        size_t next = 0;
    };
    static Script *&current() { static Script *s = nullptr; return s; }
    static int RandomInt(int min, int max) {
        Script *s = current();
        if (!s || s->next >= s->draws.size()) { std::fprintf(stderr, "RandomInt: the scripted draws ran out\n"); std::exit(3); }
        return min + s->draws[s->next++] % (max - min + 1);
    }
};
}  // namespace DUtils
