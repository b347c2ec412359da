// driver.h — what the host units behind the C ABI share (rayn_hip.hip: contexts, frames, post-process entries; probes.hip: the test
// probes): the context, its workers, and the scene / argument helpers rayn_hip.hip defines.  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/rayn_hip.h"
#include "kernels.h"

namespace rayn {

struct ProfRec { int cls; hipEvent_t a, b; };

struct Arena { // one device allocation carved into 256-byte aligned pieces; without memory (a dry run) it only counts
    char* base = nullptr; size_t cap = 0, off = 0;
    template <typename T> T* take(size_t n) {
        size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
        T* p = base ? (T*)(base + off) : nullptr;
        off += bytes;
        return p;
    }
};

// The counters of the instrumented kernels (rayn_hip_set_profiling's count_evals), per worker and summed per context.
struct Counters {
    unsigned long long evals[3] = {0, 0, 0}; // extend, shade_setup (normals), shadow
    unsigned long long iters[3] = {0, 0, 0}; // fold / orbit iterations of those evaluations
    unsigned long long elided[3] = {0, 0, 0}; // zero-throughput slots, shadow segments they would have parked, their samples that took the ordinary path
    unsigned long long stage_slots[2] = {0, 0}; // march_bulb.h: lane slots offered by the orbit / epilogue stage of k_shadow_bulb
    void clear() { *this = Counters(); }
    Counters& operator+=(const Counters& o) {
        for (int k = 0; k < 3; k++) { evals[k] += o.evals[k]; iters[k] += o.iters[k]; elided[k] += o.elided[k]; }
        for (int k = 0; k < 2; k++) stage_slots[k] += o.stage_slots[k];
        return *this;
    }
    // from the read-back of a worker's d_evals[16]: SDF evaluations of extend / shade setup / shadow in [0..2], the fold / orbit iterations they ran in
    // [4..6]; elision accounting of k_shade_setup in [3], [7], [8]; the stage slots in [12], [13]
    void decode(const unsigned long long h[16]) {
        for (int k = 0; k < 3; k++) { evals[k] = h[k]; iters[k] = h[4 + k]; }
        elided[0] = h[3]; elided[1] = h[7]; elided[2] = h[8];
        stage_slots[0] = h[12]; stage_slots[1] = h[13];
    }
};

// One worker = one HIP stream + its own slice of device memory, driven by its own host thread.  A frame's
// tiles are dealt to two workers so that one worker's HBM-bound kernels, queue-size readbacks and kernel
// tails run underneath the other's VALU-bound march kernels (measured: +6 % on config 2).
struct Worker {
    hipStream_t stream = nullptr;          // the stream this worker's frame share runs on: the CALLER's stream for worker 0, `own` for the others
    hipStream_t own = nullptr;             // created on first use by workers >= 1 (every further stream of a process costs 12-17 ms, the first ~100 ms)
    Arena arena;
    uint32_t* h_totals = nullptr;          // pinned
    DCtl* h_ctl = nullptr;                 // pinned: the control block read back once per frame share
    std::vector<DTile> h_tiles;            // staging of every batch's tile list (one upload per frame share)
    unsigned long long* d_evals = nullptr; // [16]: the device side of 'counters' (Counters::decode)
    DCtl* d_ctl = nullptr;                 // device control block (outside the arena: the arena may be re-allocated between frames)
    hipEvent_t done = nullptr;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> event_pool;
    rayn_stats stats;
    Counters counters;
    std::string err;
    int rc = 0;
};
constexpr int MAX_WORKERS = 4;

// What the setters of the ABI change.  One block per context; the entries of a multi-device context all read entry 0's (rayn_ctx::cfg),
// so a setter is one assignment and the entries cannot drift apart.
struct Settings {
    bool have_world = false;
    rayn_world_desc world;
    bool profiling = false, counting = false;
    size_t batch_paths = (size_t)1 << 28;   // per worker; also limited by the HBM budget and the 32-bit job refs (render_device)
    size_t two_worker_min_paths = (size_t)1 << 22;
    size_t cold_bytes = (size_t)44 << 30;   // arena bytes (all workers together) of a context's FIRST frame (render_device); 0 = full size at once
    int n_workers = 2;
    int fma_policy = 0; // 0: mul_add unfused (reference default build), 1: fused
};

} // namespace rayn

struct rayn_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    rayn::Settings own_cfg;
    rayn::Settings* cfg = &own_cfg;           // a peer of a multi-device context: entry 0's block (rayn_hip_create_multi)
    rayn::DScene* d_scene = nullptr;
    float4* d_rec = nullptr; size_t rec_cap = 0; // packed sample records (shared by the workers)
    rayn::Worker workers[rayn::MAX_WORKERS];
    hipEvent_t ev_fork = nullptr, ev_a = nullptr, ev_b = nullptr, ev_ma = nullptr, ev_mb = nullptr; // ev_m*: brackets of a multi-device frame
    rayn_stats stats;
    rayn::Counters counters;
    size_t small_share_paths = (size_t)1 << 27; // single-batch shares up to this size are split between two co-resident workers (render_device)
    uint64_t frames_rendered = 0;
    uint64_t table_broadcasts = 0;          // multi-device context: peer copies of the tables made so far (diagnostics, rayn_hip_table_broadcasts)
    size_t prewarm_bytes = 0;               // arena size worker 1 should get before the next frame starts (prewarm_second_worker); 0 = nothing pending
    float* host_stage = nullptr; size_t host_stage_cap = 0; // rayn_hip_render_frame: device copies of the caller's tables + film (grow-only)
    rayn::Tuning tun;                  // read from the environment at create (RAYN_HIP_ENV_TUNING), per entry
    std::vector<uint32_t> tile_subset; // rayn_hip_set_tile_subset: render only these tiles (sorted)
    std::vector<uint32_t> prog_host;   // rayn_hip_progressive_*: host side of the tile list upload and of the read-backs
    // ---- multi-device context (rayn_hip_create_multi): this ctx is entry 0 and owns the others; every peer is a complete
    // single-device ctx (own streams, workers, arenas) on its device.  A render deals the share's tiles to the entries, each
    // renders its list (RenderTarget::tiles), packs its pixels and sends them to device 0 with one peer copy (render_multi).
    std::vector<rayn_ctx*> peers;
    struct PeerBuf {
        float* tables = nullptr; size_t tables_cap = 0; float* packed = nullptr; size_t packed_cap = 0;
        // what the peer's copy of the tables was made from: the caller's four device pointers + the parameters that size and seed them.  A frame with the same key
        // skips the broadcast (r6: it was re-sent every frame, <= tens of MB per peer); rayn_hip_upload_world forgets the key.
        uint64_t tab_key[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; bool tab_valid = false;
    };
    std::vector<PeerBuf> peer_bufs;                       // on the peer's device
    float* gather_buf = nullptr; size_t gather_cap = 0;   // on device 0: the packed pixels of all peers
    rayn::DTile* gather_tiles = nullptr; size_t gather_tiles_cap = 0;
    int budget_share = 1;            // entries of a multi-device context that share this ctx's GPU: the HBM budget is split between them
    int trace_tile = -1;             // diagnostics: dump the packet order of this tile (rayn_hip_set_trace_tile)
    std::vector<uint32_t> trace;     // records of 6 u32: depth, object, tile x, tile y, sample, valid
    rayn_stats entry0_stats;         // multi-device context: what entry 0 (this ctx's own device) did in the last frame (ctx->stats then holds the sums)
    // rayn_hip_unpack_share_device: the DTile list of a share (film_base = the tile's first pixel in the packed planes), uploaded once per
    // (resolution, tile size, tile_first, tile_step) and kept - the steady-state unpack of a gathered block is ONE kernel launch
    struct UnpackPlan { uint32_t key[6]; rayn::DTile* d_tiles; uint32_t n_tiles; size_t pixels; };
    std::vector<UnpackPlan> unpack_plans;
    // (bits(min_radius^2), bits(fixed_radius^2)) pairs whose sphere-fold division was checked exhaustively on the device,
    // with the verdict (true = the 4-instruction division is exact for every reachable denominator)
    std::vector<std::pair<std::pair<uint32_t, uint32_t>, bool>> short_div_verdicts;
};

namespace rayn {

inline int fail(rayn_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; return code; }

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fail(ctx, RAYN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// rayn_hip.hip
int validate(rayn_ctx* ctx, const rayn_frame_params* p);
int build_scene(rayn_ctx* ctx, const rayn_world_desc& w, const rayn_frame_params& p, DScene* out);
int scene_march_kernels(const rayn_ctx* ctx, const DScene& hs, const rayn_frame_params& p, Tuning* tun);

} // namespace rayn
