// search_engine.hpp — what another translation unit needs of the search engine of search.hip: the engine's entry (run_search), the rule
// constructor and the interface of a producer that makes the queries on the device (DeviceQueries).  search.hip defines all of it;
// localmap_track.hip is the second user.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mframe.hpp"
#include "solver_host.hpp"

namespace sivo {

// the engine's regions a producer's kernel may write, valid from launch on
struct EngineRegions {
    SivoSearchQuery *q;        // nq records: a producer writes every one of them
    uint4 *qdesc;              // 2 per query: written by a producer whose device_inputs() holds, else the caller's upload
    uint8_t *blocked;          // one per keypoint of the frame: as qdesc
};

// Queries made on the device (sivo_search_local_points, sivo_localmap_search_local_points): the producer adds its inputs (copy regions)
// and its results (take regions) to the engine's layout, enqueues its kernel behind the upload — it writes all nq query records — and
// reads its own results from the mirror once the engine has synchronised.
// Contract: with nq > 0 the engine calls regions, launch and collect, once each and in that order; with nq <= 0 it returns before it
// takes any scratch and calls none of them (there is nothing to stage or collect).  scratch() may move the frame to a bigger slab, so
// the frame's view and its stream are valid only from launch on: launch takes them from the frame it is handed, never from a copy made
// before run_search.
// device_inputs(): the producer's kernel also writes the queries' descriptors and the blocked flags.  The engine then keeps the query
// records, the descriptors and the flags in device-only scratch behind the results: nothing of them is uploaded or copied back, and
// run_search's query_desc and blocked arguments are not read.
struct DeviceQueries {
    virtual void regions(Layout &L) = 0;
    virtual void launch(const sivo_mframe &F, const EngineRegions &r) = 0;
    virtual void collect(const Layout &L) = 0;
    virtual bool device_inputs() const { return false; }
    virtual ~DeviceQueries() {}
};

// The engine on host arrays: upload queries, rounds, finalize, download.  With `dq` the queries come from the device and `queries` is
// not read; without it nothing of the layout or the launches changes.
void run_search(sivo_mframe &F, const SivoSearchQuery *queries, const uint8_t *query_desc, int nq, const int32_t *cand_begin,
                const int32_t *cand_end, const int32_t *cand_idx, int n_cand, const SivoSearchRule &rule, const uint8_t *blocked,
                int32_t *match_query, int32_t *match_train, int32_t *best_dist, int32_t *second_dist, int *n_matches, int *rounds_out,
                DeviceQueries *dq = nullptr);

SivoSearchRule make_rule(int th, int gate_mode, int ratio_mode, float nn, bool ori, bool dynamic);

}  // namespace sivo
