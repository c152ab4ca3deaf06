// engine_group.h -- what engine_group.cpp shares with engine_serve.cpp: the group, the arena of
// staged arguments, the description of one grouped step with its one launcher, and the stages of
// the chunked optimize loop that stomp_group_optimize and stomp_group_serve are both made of.
#pragma once

#include "engine_internal.h"

#include <functional>

struct stomp_group {
    std::vector<stomp_engine*> e;
    std::vector<int> all;                 // 0 .. P - 1: the engines of a run's step and of a synchronize's flush
    int device = 0;
    hipStream_t stream = nullptr;
    int nt = 0;                           // weights tiles per engine
    stomp::NoiseArgs shape{};             // J, N, Nall of the reuse launches
    stomp::DevModel* d_models = nullptr;  // [P]
    bool state_terms = false;             // engines with terms accepted (stomp_group_create_with)
    stomp::TermsModel* d_tmodels = nullptr;   // [P] every engine's terms model (state_terms)
    int nterms = 0;                       // engines with terms
    int ncum = 0;                         // engines with cumulative costs (stomp_group_create_flags)
    size_t terms_lds = 0;                 // the largest terms_lds_bytes among them: k_terms_group's dynamic LDS
    // stomp_group_run / stomp_group_synchronize: one run's arguments, a take_step per iteration
    unsigned char* d_args = nullptr;
    size_t d_cap = 0;
    unsigned char* h_args = nullptr;      // pinned staging of one run's arguments
    size_t h_cap = 0;
    hipEvent_t staged = nullptr;          // the last upload from h_args is done
    // stomp_group_optimize / stomp_group_serve: two slots of one chunk's arguments each (pinned and
    // device), the engines' (stop, iterations) mirror with a pinned read-back per slot, all P track
    // arguments
    bool compact = false;                 // stopped engines leave the launches (STOMP_DEBUG_GROUP_COMPACT=1 / 0)
    unsigned char *h_opt = nullptr, *d_opt = nullptr;
    size_t opt_slot = 0;                  // bytes per slot
    int* d_mirror = nullptr;              // [P][2]
    int* h_mirror = nullptr;              // [2][P][2]
    stomp::TrackArgs* d_track_all = nullptr;   // [P]
    hipEvent_t opt_ev[2] = {nullptr, nullptr};
    // the retarget calls: one call's staging (pinned and device), held with a capacity; the
    // padding-collision flag each entry of d_models holds, so that an engine retargeted on its own
    // (stomp_engine_retarget knows no group) gets its entry refreshed before the next launch that
    // reads the list; the model epoch of every engine the group's lists were made from (an engine
    // whose model was replaced on its own since then leaves them stale: check_epochs)
    unsigned char *h_rq = nullptr, *d_rq = nullptr;
    size_t rq_cap = 0;
    std::vector<int> pad_flags;
    std::vector<long long> epochs;
    // stomp_group_serve: the result slab on the device, held with a capacity (bytes), and what
    // stomp_group_serve_info reports of the last call
    unsigned char* d_slab = nullptr;
    size_t slab_cap = 0;
    long long serve_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::string err;
};

namespace stomp {

int gfail(stomp_group* g, int code, const char* msg);

// A bump allocator over a staging buffer, `cap` bytes pinned at `h` and on the device at `d`:
// take(n, dev) hands out the next array of n T at a 256-byte aligned offset of both, the host side
// returned, the device side in `dev`.  The caller checks overflowed() before it fills.  With no
// buffers it only measures: used() after the takes is the capacity they need.
struct Arena {
    unsigned char *h = nullptr, *d = nullptr;
    size_t cap = ~(size_t)0, off = 0;
    template <class T>
    T* take(size_t n, const T*& dev)
    {
        const size_t o = off;
        off += align256(sizeof(T) * n);
        dev = d ? (const T*)(d + o) : nullptr;
        return h ? (T*)(h + o) : nullptr;
    }
    size_t used() const { return off; }
    bool overflowed() const { return off > cap; }
};

// the DevModel and TermsModel lists of a launch: the group's own over all P engines, or staged ones
struct ModelLists {
    const DevModel* models = nullptr;
    const TermsModel* tmodels = nullptr;
    int nx = 0;   // engines with terms among the launch's (0: no terms launch)
};

// One grouped step: what launch_step needs and nothing else, device pointers and counts.
struct StepLaunch {
    // the engines that run an iteration (each its own: CostArgs, TrackArgs::it): rollouts, weights, update
    const CostArgs* cas = nullptr; const WeightArgs* was = nullptr; const UpdateArgs* uas = nullptr;
    const ReuseRowArgs* ras = nullptr; const TermsArgs* xas = nullptr;
    ModelLists lists;
    // engines; the most rollout workgroups and the most totals blocks any of them has (engines in
    // lockstep: the common counts)
    int nm = 0, nro = 0, ntot = 0;
    bool reuse = false;              // an engine of the step reuses: the grouped reuse launch
    // the flush cohort: engines whose pending noiseless rollout alone is evaluated
    const CostArgs* ccs = nullptr; const TermsArgs* cxas = nullptr;
    ModelLists clists;
    int nc = 0;
    bool time_flush = true;          // the cohort's rollout launch is recorded on T_NOISELESS
    // k_track_group over ntrack entries, each with its own iteration index; ntrack == 0: no launch
    const TrackArgs* tas = nullptr;
    int ntrack = 0;
};

// The launches of one grouped step, in the order everything depends on; returns how many it made.
int launch_step(stomp_group* g, const StepLaunch& L);

int check_epochs(stomp_group* g);
TrackArgs track_args(const stomp_group* g, int p, int it = -1);

// ---- the chunked optimize loop's stages

// what the stages of one stomp_group_optimize or stomp_group_serve call share
struct OptimizeLoop {
    struct HostState { bool reused_next, extra_added; int row_set; };   // generateRollouts' on the host
    stomp_group* g = nullptr;
    std::vector<int> live;     // the engines staged from here on (all, or with g->compact the ones not seen stopped)
    int next = 1;              // the first step not staged yet
    int last_step = 0;         // the last step with work: the flush of the engines that end last
    // start[p]: the group step in which engine p runs its iteration 1 (stomp_group_optimize: 1 for
    // all; a slot of a serve loop: the first step staged after it took its request)
    std::vector<int> start;
    // after[p][it - 1]: engine p's state after iteration it, to restore for every engine the one
    // of the iteration the device stopped it at (stomp_engine_optimize's)
    std::vector<std::vector<HostState>> after;
    std::vector<int> main, main_it, cohort;    // the step being staged (main_it: each main engine's iteration)
    std::vector<StepLaunch> steps;    // the chunk being staged
    long long launches = 0;           // kernel launches enqueued so far
    // a serve loop: flag_unknown[p] != 0 -- the host copy of engine p's padding-collision flag is
    // behind the device's (a turnover's k_retarget made it); every model entry staged for p is
    // listed in flag_copies, for launch_serve_flags ahead of the chunk's steps
    const std::vector<char>* flag_unknown = nullptr;
    std::vector<FlagCopy> flag_copies;
};

// what a serve loop adds to a chunk: its own arguments into the arena once the steps are staged,
// its launches behind the upload and ahead of the steps'
struct ChunkExtra {
    std::function<int(Arena&)> stage;
    std::function<void()> launch;
};

size_t step_bytes(const stomp_group* g, int nm, int nc, bool track, bool lists);
// what a serve loop's chunk stages beside its steps, at most: every slot's turnover (TurnArgs,
// RequestArgs with the request's start and goal, the pregen's NoiseArgs) and a flag copy per model
// entry staged
inline size_t serve_chunk_bytes(int P, int J)
{
    return align256(sizeof(TurnArgs) * P) + align256(sizeof(RequestArgs) * P) + align256(sizeof(NoiseArgs) * P) +
           align256(sizeof(double) * 2 * J * P) + align256(sizeof(FlagCopy) * 2 * P * STOMP_GROUP_OPTIMIZE_CHUNK);
}
int optimize_prepare(stomp_group* g);
int optimize_enqueue_chunk(OptimizeLoop& o, int slot, const ChunkExtra* extra = nullptr);
// engine p stopped after `iterations` of the loop's iterations: its generateRollouts state put back
// to that iteration's (the steps staged past the stop were no-ops on the device)
void optimize_restore(OptimizeLoop& o, int p, int iterations);

}  // namespace stomp
