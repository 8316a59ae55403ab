// mev_capi.cpp — the extern "C" boundary (include/marlenv.h): handle
// lifetime, route tables, device buffers and the host side of reset / step /
// state transfer.  Replaces the reference's pybind11 module MARLEnv
// (cpp/bindings.cpp:11-95); see INTEGRATION.md for the caller-side bindings.
#include "marlenv.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <rccl/rccl.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <mutex>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "mev_act.h"
#include "mev_kernels.h"
#include "mev_routes.h"
#include "mev_world.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(MEV_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// reference utils.py:29-52 default ego route mappings (IN_k -> OUT_m), as point indices
const int kMap3[12][2] = {{1, 4}, {2, 8}, {3, 12}, {4, 7}, {5, 11}, {6, 3},
                          {7, 10}, {8, 2}, {9, 6}, {10, 1}, {11, 5}, {12, 9}};
const int kMap2[7][2] = {{1, 3}, {2, 6}, {3, 5}, {4, 8}, {6, 2}, {7, 1}, {8, 4}};

template <class T>
hipError_t dalloc(T** p, size_t n) {
    return hipMalloc(reinterpret_cast<void**>(p), (n ? n : 1) * sizeof(T));
}

}  // namespace

// A state pool (mev_pool_create): one device block carved into the arrays of mev::PoolState.
struct mev_pool {
    mev_handle* h = nullptr;
    int32_t slots = 0;
    uint8_t* block = nullptr;
    mev::PoolState st{};
};

// A policy (mev_policy_create): its device block and where each layer lies in it (mev::PolicyNet).
struct mev_policy {
    mev_handle* h = nullptr;
    float* block = nullptr;
    mev::PolicyNet net{};
    bool has_value = false;  // a value head is attached (mev_policy_set_value_head): column 2 of the last layer's block
};

struct mev_handle {
    mev_config cfg{};
    int D = 0, lidar_slots = 0, P = 0, nroutes = 0;
    int route_cap = 0;  // routes the device route tables have room for (mev_add_route)
    std::vector<mev::LanePoint> pts;
    std::vector<float> h_paths, h_spawn;  // h_paths: [nroutes][row_pts][2] (mev_world.h)
    std::vector<int32_t> h_len;           // points of each route's path (2 .. MAX_PATH_LEN)
    // the table's row geometry (RouteTab::plen / row): PATH_LEN / ROUTE_PTS until a written
    // path longer than PATH_LEN is added, then that path's length rounded up to 16
    int plen = mev::PATH_LEN, row_pts = mev::ROUTE_PTS;
    std::vector<float> h_pbox;  // [nroutes][3][4] piece bounding boxes (RouteTab::pbox)
    std::vector<int32_t> h_intent;
    // route_hash[r]: FNV-1a of routes [0, r) (paths and intents), so a snapshot or a gather
    // peer can tell whether its route ids name the same routes here (routes are only appended)
    std::vector<uint64_t> route_hash{1469598103934665603ull};
    void extend_route_hash() {
        while (route_hash.size() <= size_t(nroutes)) {
            const size_t r = route_hash.size() - 1;
            uint64_t x = route_hash.back();
            auto mix = [&x](const void* p, size_t n) {
                const uint8_t* b = static_cast<const uint8_t*>(p);
                for (size_t i = 0; i < n; ++i) x = (x ^ b[i]) * 1099511628211ull;
            };
            // a path as its first max(n, PATH_LEN) row points, its last segment and, up to
            // PATH_LEN, the ROUTE_PTS row's zero tail: the same bytes whatever the row stride
            const float* row = &h_paths[r * 2 * size_t(row_pts)];
            const int n = std::max(h_len[r], mev::PATH_LEN);
            mix(row, 2 * size_t(n) * sizeof(float));
            mix(row + 2 * plen, 4 * sizeof(float));
            if (n == mev::PATH_LEN) {
                const float z[2 * (mev::ROUTE_PTS - mev::ROUTE_END - 2)] = {};
                mix(z, sizeof(z));
            }
            mix(&h_intent[r], sizeof(int32_t));
            route_hash.push_back(x);
        }
    }
    std::vector<int32_t> h_traffic;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;
    mev::SimParams sp{};
    mev::SimParams* d_sp = nullptr;  // device copy of sp read by k_step (refreshed when sp changes)
    mev::SimParams sp_dev{};         // what d_sp holds
    bool sp_valid = false;
    mev::Outputs internal{};
    mev::Outputs last{};  // where the most recent outputs were written
    float* d_actions = nullptr;
    int32_t* d_spawn = nullptr;
    uint8_t* d_stage = nullptr;  // the staging block of host-mode calls (Stage, below), grown to the largest call seen
    size_t stage_cap = 0;
    // mev_evaluate_leaves: the candidates' LiDAR hand-off (mev::LeafHand), grow-only up to kLeafHandCap
    uint8_t* d_leaf = nullptr;
    size_t leaf_cap = 0;
    int leaf_chunk = 0;  // MEV_LEAF_CHUNK at mev_create: candidates per chunk (0: as many as the cap holds)
    uint8_t* d_mask = nullptr;
    float* d_paths = nullptr;
    int32_t* d_rlen = nullptr;  // [route_cap] each path's own length (RouteTab::len)
    float* d_pbox = nullptr;
    float* d_spawn_tab = nullptr;
    int32_t* d_intent = nullptr;
    float* d_rel = nullptr;
    int32_t* d_traffic = nullptr;
    int32_t* d_reset_routes = nullptr;  // [nroutes]: pool for per-reset route draws
    uint64_t rng_counter = 0;
    // per-kernel timing (mev_kernel_timing): 3 events per step, folded into sums when the ring fills
    std::vector<hipEvent_t> tev;
    int tn = 0;
    int t_every = 1;       // record events on every t_every-th step
    int64_t t_phase = 0;   // steps since timing was enabled
    double t_cars_ms = 0.0, t_lidar_ms = 0.0;
    int64_t t_steps = 0;
    // multi-GPU gather (mev_comm_init): packed outputs, double buffered by step parity
    ncclComm_t comm = nullptr;
    int world = 1, rank = 0, root = 0, slots = 0;
    uint64_t pk_off[MEV_PK_FIELDS] = {};
    int gather_fmt = MEV_GATHER_F32;  // mev_set_gather_format
    std::vector<float> h_lidar_table;  // [256] decode table of the compact format (mev_lidar_decode_table)
    float* d_lidar_table = nullptr;
    uint64_t pk_bytes = 0;
    uint8_t* pk_buf[2] = {nullptr, nullptr};  // root: [world][pk_bytes]; other ranks: [pk_bytes]
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_step[2] = {nullptr, nullptr}, ev_gather[2] = {nullptr, nullptr};
    bool gather_pending[2] = {false, false};
    int64_t gathers = 0;  // gathered steps so far; the last one used buffer (gathers - 1) & 1
    // NPC-aware deal of the fused traffic kernel: valid while every step since the
    // last state change went through it (the rings then hold one entry per env)
    bool deal_valid = false;
    // the rings were built by a step with MEV_AUTO_RESET: an env that ended there is in class
    // 0 (no NPC slot loaded), which only the next step's auto-reset makes true
    bool deal_ar = false;
    bool deal_on = true;  // mev_set_env_deal (default: on unless MEV_NO_DEAL=1)
    int deal_ring = 0;

    template <class T>
    hipError_t alloc(T** p, size_t n) {
        hipError_t e = dalloc(p, n);
        if (e == hipSuccess) {
            allocs.push_back(*p);
            e = hipMemsetAsync(*p, 0, (n ? n : 1) * sizeof(T), stream);
        }
        return e;
    }
    hipError_t fold_timing() {
        if (tn == 0) return hipSuccess;
        hipError_t e = hipEventSynchronize(tev[size_t(3 * tn - 1)]);
        if (e != hipSuccess) return e;
        for (int i = 0; i < tn; ++i) {
            float a = 0.f, b = 0.f;
            if ((e = hipEventElapsedTime(&a, tev[size_t(3 * i)], tev[size_t(3 * i + 1)])) != hipSuccess) return e;
            if ((e = hipEventElapsedTime(&b, tev[size_t(3 * i + 1)], tev[size_t(3 * i + 2)])) != hipSuccess) return e;
            t_cars_ms += a;
            t_lidar_ms += b;
        }
        t_steps += tn;
        tn = 0;
        return hipSuccess;
    }
    void free_timing() {
        for (hipEvent_t ev : tev) (void)hipEventDestroy(ev);
        tev.clear();
        tn = 0;
    }
    void free_comm() {
        if (comm) (void)ncclCommDestroy(comm);
        comm = nullptr;
        for (int b = 0; b < 2; ++b) {
            if (pk_buf[b]) (void)hipFree(pk_buf[b]);
            if (ev_step[b]) (void)hipEventDestroy(ev_step[b]);
            if (ev_gather[b]) (void)hipEventDestroy(ev_gather[b]);
            pk_buf[b] = nullptr;
            ev_step[b] = ev_gather[b] = nullptr;
            gather_pending[b] = false;
        }
        if (comm_stream) (void)hipStreamDestroy(comm_stream);
        comm_stream = nullptr;
        world = 1; rank = root = 0; gathers = 0;
    }
    // Host-mode steps of a small handle (outputs <= kPinMax bytes): actions and
    // outputs in one block of host-mapped pinned memory that the kernels read
    // and write directly (zero-copy), so a step is one launch and one stream
    // synchronization instead of nine pageable copies (~150 us at 1 env).
    static constexpr size_t kPinMax = 256 * 1024;
    uint8_t* pin = nullptr;     // host address of the block (hipHostMalloc, mapped, coherent)
    uint8_t* pin_dev = nullptr; // its device address
    size_t pin_off[10] = {};    // actions, spawn, obs, reward, done, status, term, trunc, alive, step
    mev::Outputs pin_out{};     // device addresses of the pinned outputs
    // Persistent step server (k_serve, mev_set_serve): host-mode steps of a small
    // handle posted to a resident kernel through a mailbox in pinned memory
    int serve_mode = 1;                 // 0 off, 1 automatic
    mev::ServeBox* sbox = nullptr;      // host address of the mailbox (mapped, coherent)
    mev::ServeBox* sbox_dev = nullptr;  // its device address
    // (atomic: serve_slot reads other handles' flags, which their own threads write)
    std::atomic<bool> serve_running{false};  // an instance may be resident on `stream`
    int serve_wg = 0;                        // its workgroups
    uint32_t serve_seq = 0, serve_sid = 0;
    std::atomic<uint32_t> serve_epoch{0};
    uint64_t serve_steps = 0, serve_launches = 0;
    // Adaptive idle limit: a resident server makes every device-wide
    // wait of the process (hipDeviceSynchronize, torch.cuda.synchronize, some frees)
    // wait for its idle exit, so it stays only a few host gaps long: 8 x the moving
    // average of the host's time between an answer and the next post (each gap
    // counted up to 2 ms), within [0.2, 2] ms; it starts at the cap and follows the
    // host's pace.  Posts that keep finding the server gone (a device-wide wait, or
    // a host slower than 2 ms between steps) pause serving: the next kPausedSteps
    // host steps are launched.
    double serve_gap_us = 250.0;
    int serve_misses = 0;
    uint64_t serve_pause = 0;
    uint64_t serve_misses_total = 0;
    std::chrono::steady_clock::time_point serve_t_answer{};
    // steady-clock ns of the handle's last host-mode step (serve_slot: a slot's owner
    // that has made no host step for kServeStaleMs may lose it to another handle)
    std::atomic<int64_t> serve_last_ns{0};
    // the same in host steps of the whole process (g_host_tick): serve_last_tick is the
    // handle's last host-mode step, serve_mark the one before it (at first, the handle's
    // creation).  An owner that has stepped since another handle's mark keeps its slot
    // from that handle whatever the clock says: a pause of the whole process (a descheduled
    // or collecting host) between two steps of a round-robin makes nobody stale
    std::atomic<uint64_t> serve_last_tick{0};
    uint64_t serve_mark = 0;
    // the server's own stream: non-blocking, at the highest priority, whose hardware
    // queues are not the ones normal-priority streams share (GPU_MAX_HW_QUEUES of them):
    // a resident kernel holds back whatever another stream queues behind it on its queue
    hipStream_t serve_stream = nullptr;
    hipEvent_t serve_ev = nullptr;  // orders the server after the handle's stream
    uint8_t* gs_pin = nullptr;  // pinned staging of mev_get_state
    size_t gs_cap = 0;
    std::vector<mev_pool*> pools;  // the handle's state pools (mev_pool_create), released with it
    std::vector<mev_policy*> policies;  // the handle's policies (mev_policy_create), released with it
    ~mev_handle() {
        if (comm_stream) (void)hipStreamSynchronize(comm_stream);
        free_comm();
        free_timing();
        if (pin) (void)hipHostFree(pin);
        if (sbox) (void)hipHostFree(sbox);
        if (serve_ev) (void)hipEventDestroy(serve_ev);
        if (serve_stream) (void)hipStreamDestroy(serve_stream);
        if (gs_pin) (void)hipHostFree(gs_pin);
        if (d_stage) (void)hipFree(d_stage);
        if (d_leaf) (void)hipFree(d_leaf);
        for (mev_pool* q : pools) {
            if (q->block) (void)hipFree(q->block);
            delete q;
        }
        for (mev_policy* q : policies) {
            if (q->block) (void)hipFree(q->block);
            delete q;
        }
        for (void* p : allocs) (void)hipFree(p);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};

// a device block of the handle that only grows (the staging block, the leaf scratch): at least `need` bytes
static int grow_block(mev_handle* h, uint8_t** block, size_t* cap, size_t need) {
    if (need <= *cap) return MEV_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (*block) (void)hipFree(*block);
    *block = nullptr;
    *cap = 0;
    const hipError_t err = hipMalloc(reinterpret_cast<void**>(block), need);
    if (err != hipSuccess) return fail(MEV_E_NOMEM, std::string("device allocation failed: ") + hipGetErrorString(err));
    *cap = need;
    return MEV_OK;
}

// Stage: the caller's arrays of one call on the device.  The call names each array once, with the
// slot its kernel arguments read the device address from: in() what the device reads, out() what it
// writes; a null array makes its slot null.  upload(), after the arguments have been checked, lays
// the named arrays out in the handle's staging block (d_stage), each at a 256-byte boundary, grows
// the block to hold them, points the slots into it and enqueues the inputs' copies; download()
// enqueues the outputs' copies back and synchronises the stream.  fetch() adds an output that
// another device array holds.  With `dev` (MEV_DEVICE_PTRS) the slots receive the caller's own
// pointers, nothing is copied and download() does not synchronise: a call has no host / device
// branch of its own for its arrays.
// One block serves every call: a host-mode call that stages ends in download()'s synchronise, so
// the block is idle when the next one starts; device-mode calls never touch it; and a call's
// inputs and outputs lie side by side in one layout.
// Not staged: mev_step and mev_reset (the per-step path: d_actions, d_spawn, d_mask and the pinned
// zero-copy block, sized at mev_create), the unmasked mev_restore and mev_set_state (copies straight
// into the state arrays), mev_get_state (its pinned read-back) and the configuration calls.
struct Stage {
    Stage(mev_handle* h, bool dev) : h(h), dev(dev) {}
    template <class T>
    void in(const T** slot, const T* host, size_t n) { add(slot, host, n * sizeof(T), false); }
    template <class T>
    void out(T** slot, T* host, size_t n) { add(slot, host, n * sizeof(T), true); }
    void fetch(void* host, const void* d, size_t bytes) {
        if (!dev && host && bytes) items.push_back({nullptr, host, const_cast<void*>(d), 0, bytes, true});
    }
    int upload() {
        if (dev) return MEV_OK;
        if (int r = grow_block(h, &h->d_stage, &h->stage_cap, need)) return r;
        for (Item& it : items) {
            if (!it.slot) continue;
            it.d = h->d_stage + it.off;
            memcpy(it.slot, &it.d, sizeof(void*));
            if (!it.out) HIP_TRY(hipMemcpyAsync(it.d, it.host, it.bytes, hipMemcpyHostToDevice, h->stream));
        }
        return MEV_OK;
    }
    int download() {
        if (dev) return MEV_OK;
        for (const Item& it : items)
            if (it.out) HIP_TRY(hipMemcpyAsync(it.host, it.d, it.bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return MEV_OK;
    }

private:
    struct Item {
        void* slot;  // the address of the caller's pointer variable (null: fetch)
        void* host;
        void* d;
        size_t off, bytes;
        bool out;
    };
    // (the slot is written as bytes: it is a pointer variable of the array's own type)
    void add(void* slot, const void* host, size_t bytes, bool out) {
        if (dev || !host) {
            memcpy(slot, &host, sizeof(void*));
            return;
        }
        items.push_back({slot, const_cast<void*>(host), nullptr, need, bytes, out});
        need += (bytes + 255) & ~size_t(255);
    }
    mev_handle* h;
    bool dev;
    size_t need = 0;
    std::vector<Item> items;
};

extern "C" {

static int serve_stop(mev_handle* h);  // with mev_step: the resident step server leaves the stream
namespace {
void serve_unlist(mev_handle* h);  // (with mev_step) the handle leaves the resident-server list
std::atomic<uint64_t> g_host_tick{0};  // host-mode steps of small handles in this process (mev_handle::serve_mark)

// SimParams::beam_cull: the LiDAR's per-box beam culling models the offsets as
// rel[b] = rel[0] + b*d (to 1e-5 rad, the slack its 2e-4 rad margin covers) with d > 0 and
// the fan within one revolution, (R-1)*d <= 2*pi.  Any other list (a written
// Lidar.rel_angles, cpp/bindings.cpp:91: descending, constant, uneven, several turns) is
// simulated without the culling.
int beam_cull_ok(const float* rel, int R) {
    if (R <= 1) return 1;
    const double d = (double(rel[R - 1]) - double(rel[0])) / double(R - 1);
    if (!(d > 0.0) || double(R - 1) * d > 6.283185307179586 + 1.0e-4) return 0;
    for (int b = 1; b < R - 1; ++b)
        if (fabs(double(rel[b]) - (double(rel[0]) + b * d)) > 1.0e-5) return 0;
    return 1;
}
}  // namespace

const char* mev_last_error(void) { return g_err.c_str(); }
int mev_abi_version(void) { return MEV_ABI_VERSION; }
int mev_path_len(void) { return mev::PATH_LEN; }

int mev_device_count(int32_t* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    if (count) *count = n;
    return MEV_OK;
}

int mev_config_default(mev_config* c) {
    if (!c) return fail(MEV_E_INVALID, "null config");
    memset(c, 0, sizeof(*c));
    c->num_envs = 1;
    c->num_agents = 1;
    c->num_lanes = mev::kRefNumLanes;
    c->lidar_rays = 96;  // cpp/IntersectionEnv.cpp:113-116
    c->lidar_fov_deg = 360.0f;
    c->lidar_max_dist = mev::kRefLidarMaxDist;
    c->lidar_step = mev::kRefLidarStep;
    c->obs_dim = 0;
    c->traffic_flow = 0;
    c->traffic_density = 0.5f;  // cpp/IntersectionEnv.h:35
    c->use_team_reward = 0;
    c->respawn_enabled = 1;
    c->max_steps = 2000;
    const float rc[8] = {10.0f, 1.0f, -0.01f, -10.0f, -5.0f, 10.0f, -0.02f, 0.2f};  // cpp/Reward.h:5-14
    memcpy(c->reward, rc, sizeof(rc));
    c->max_npcs = 32;
    c->seed = 0;
    c->device = 0;
    return MEV_OK;
}

int mev_create(const mev_config* cfg, mev_handle** out) {
    if (!cfg || !out) return fail(MEV_E_INVALID, "null argument");
    const mev_config& c = *cfg;
    if (c.num_envs < 1) return fail(MEV_E_INVALID, "num_envs must be >= 1");
    if (c.num_agents < 1 || c.num_agents > 64) return fail(MEV_E_INVALID, "num_agents must be in [1, 64]");
    if (c.num_lanes < 1 || c.num_lanes > 8) return fail(MEV_E_INVALID, "num_lanes must be in [1, 8]");
    if (c.lidar_rays < 1 || c.lidar_rays > 1024) return fail(MEV_E_INVALID, "lidar_rays must be in [1, 1024]");
    if (!(c.lidar_step > 0.0f) || !(c.lidar_max_dist > 0.0f)) return fail(MEV_E_INVALID, "lidar step/max_dist must be > 0");
    if (c.max_npcs < 0 || c.max_npcs > 64) return fail(MEV_E_INVALID, "max_npcs must be in [0, 64]");
    const int D = c.obs_dim > 0 ? c.obs_dim : mev::OBS_HEAD + c.lidar_rays;
    if (D < mev::OBS_HEAD) return fail(MEV_E_INVALID, "obs_dim must be >= 31");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MEV_E_HIP, "no HIP device available");
    if (c.device < 0 || c.device >= ndev) return fail(MEV_E_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(c.device));
    // LiDAR probe distances exactly as Lidar.cpp:33 accumulates them (validated
    // before any allocation: this error path owns nothing)
    // (the world's derived values, the probe count among them: mev_refworld.h)
    const mev::WorldConsts wc = mev::world_consts(c.num_lanes, c.lidar_max_dist, c.lidar_step);
    if (wc.lidar_steps > mev::kMaxMarchProbes) return fail(MEV_E_INVALID, "lidar_max_dist / lidar_step too large");
    const bool dist_mul_exact = wc.dist_exact;
    std::vector<float> dists;
    dists.reserve(size_t(wc.lidar_steps));
    for (float dist = 0.0f; int(dists.size()) < wc.lidar_steps; dist += c.lidar_step) dists.push_back(dist);

    auto* h = new mev_handle();
    h->cfg = c;
    {
        const char* nd = getenv("MEV_NO_DEAL");
        h->deal_on = !(nd && nd[0] == '1');
        const char* nw = getenv("MEV_NO_WORLD_CONST");
        h->sp.no_world_const = nw && nw[0] == '1';
        const char* lc = getenv("MEV_LEAF_CHUNK");
        const long lcv = lc ? strtol(lc, nullptr, 10) : 0;
        h->leaf_chunk = lcv > 0 && lcv <= MEV_MAX_CANDIDATES ? int(lcv) : 0;
    }
    if (h->cfg.traffic_density < 0.0f) h->cfg.traffic_density = 0.0f;  // configure_traffic (:56-60)
    h->D = D;
    h->lidar_slots = std::min(c.lidar_rays, D - mev::OBS_HEAD);
    {  // the compact gather format's LiDAR codes -> floats (Lidar::normalized, Lidar.cpp:92-98)
        const float inv = wc.lidar_inv;
        h->h_lidar_table.assign(256, 0.0f);
        h->h_lidar_table[0] = c.lidar_max_dist * inv;  // no hit: max_dist
        for (size_t k = 0; k < dists.size() && k + 1 < size_t(mev::kLidarCodeDead); ++k)
            h->h_lidar_table[k + 1] = dists[k] * inv;  // hit at probe k
        h->h_lidar_table[mev::kLidarCodeDead] = 0.0f;  // dead agent
    }
    h->P = 8 * c.num_lanes;
    h->nroutes = h->P * h->P;
    h->route_cap = h->nroutes;
    h->pts = mev::build_lane_points(c.num_lanes);
    h->h_paths.resize(size_t(h->nroutes) * 2 * mev::ROUTE_PTS);
    h->h_len.assign(size_t(h->nroutes), mev::PATH_LEN);
    h->h_intent.resize(size_t(h->nroutes));
    h->h_spawn.resize(size_t(h->nroutes) * 3);
    for (int s = 0; s < h->P; ++s)
        for (int e = 0; e < h->P; ++e) {
            const int r = s * h->P + e;
            float* path = &h->h_paths[size_t(r) * 2 * mev::ROUTE_PTS];
            h->h_intent[size_t(r)] = mev::generate_route(h->pts, c.num_lanes, s, e, path);
            std::copy(path + 2 * (mev::PATH_LEN - 2), path + 2 * mev::PATH_LEN, path + 2 * mev::ROUTE_END);
            h->h_spawn[size_t(3 * r)] = h->pts[size_t(s)].x;
            h->h_spawn[size_t(3 * r + 1)] = h->pts[size_t(s)].y;
            h->h_spawn[size_t(3 * r + 2)] = mev::spawn_heading(path);
        }
    // each route's pieces [0, 50), [50, 110), [110, 160): bounding boxes of the float points
    h->h_pbox.resize(size_t(h->nroutes) * 12);
    for (int r = 0; r < h->nroutes; ++r) {
        const float* path = &h->h_paths[size_t(r) * 2 * mev::ROUTE_PTS];
        const int cut[4] = {0, 50, 110, mev::PATH_LEN};
        for (int q = 0; q < 3; ++q) {
            float x0 = path[2 * cut[q]], x1 = x0, y0 = path[2 * cut[q] + 1], y1 = y0;
            for (int i = cut[q]; i < cut[q + 1]; ++i) {
                x0 = std::min(x0, path[2 * i]); x1 = std::max(x1, path[2 * i]);
                y0 = std::min(y0, path[2 * i + 1]); y1 = std::max(y1, path[2 * i + 1]);
            }
            float* b = &h->h_pbox[size_t(r) * 12 + size_t(q) * 4];
            b[0] = x0; b[1] = x1; b[2] = y0; b[3] = y1;
        }
    }
    // LiDAR beam offsets, cpp/IntersectionEnv.cpp:119-127 (== Lidar.cpp:4-14)
    std::vector<float> rel(size_t(c.lidar_rays));
    {
        const float start_angle_deg = -c.lidar_fov_deg * 0.5f;
        const float step_deg = (c.lidar_rays > 1) ? (c.lidar_fov_deg / float(c.lidar_rays - 1)) : 0.0f;
        const float PI_F2 = 3.14159265358979323846f;
        for (int ii = 0; ii < c.lidar_rays; ++ii) {
            const float deg = start_angle_deg + float(ii) * step_deg;
            rel[size_t(ii)] = deg * PI_F2 / 180.0f;
        }
    }
    h->sp.beam_cull = beam_cull_ok(rel.data(), c.lidar_rays);
    h->sp.beams = mev::beam_model(rel.data(), c.lidar_rays);
    h->h_traffic = mev::default_traffic_routes(c.num_lanes);
    h->extend_route_hash();

    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(MEV_E_HIP, "hipStreamCreate failed");
    }
    h->stream = h->own_stream;
    const int E = c.num_envs, N = c.num_agents, K = std::max(1, c.max_npcs);
    const size_t EN = size_t(E) * size_t(N), EK = size_t(E) * size_t(K);
    mev::SimParams& p = h->sp;
    hipError_t err = hipSuccess;
    auto A = [&](auto** ptr, size_t n) { if (err == hipSuccess) err = h->alloc(ptr, n); };
    // state
    // the 4-byte fields of each SoA in one block, field k at k * stride (mev_kernels.h)
    const size_t ens = (EN + 63) & ~size_t(63), eks = (EK + 63) & ~size_t(63);
    float* eblk = nullptr;
    float* nblk = nullptr;
    A(&eblk, ens * mev::EF_COUNT);
    A(&nblk, eks * mev::NF_COUNT);
    if (err == hipSuccess) {
        float** ef[] = {&p.ego.x, &p.ego.y, &p.ego.v, &p.ego.h, &p.ego.acc, &p.ego.steer, &p.ego.prev_dist,
                        &p.ego.pa0, &p.ego.pa1, &p.ego.sx, &p.ego.sy, &p.ego.sv, &p.ego.sh};
        for (int k = 0; k < mev::EF_PIDX; ++k) *ef[k] = eblk + size_t(k) * ens;
        p.ego.pidx = reinterpret_cast<int32_t*>(eblk + size_t(mev::EF_PIDX) * ens);
        p.ego.route = reinterpret_cast<int32_t*>(eblk + size_t(mev::EF_ROUTE) * ens);
        p.ego.intent = reinterpret_cast<int32_t*>(eblk + size_t(mev::EF_INTENT) * ens);
        p.ego.stride = int64_t(ens);
        float** nf[] = {&p.npc.x, &p.npc.y, &p.npc.v, &p.npc.h, &p.npc.acc, &p.npc.steer};
        for (int k = 0; k < mev::NF_PIDX; ++k) *nf[k] = nblk + size_t(k) * eks;
        p.npc.pidx = reinterpret_cast<int32_t*>(nblk + size_t(mev::NF_PIDX) * eks);
        p.npc.route = reinterpret_cast<int32_t*>(nblk + size_t(mev::NF_ROUTE) * eks);
        p.npc.intent = reinterpret_cast<int32_t*>(nblk + size_t(mev::NF_INTENT) * eks);
        p.npc.stride = int64_t(eks);
    }
    A(&p.ego.alive, EN);
    A(&p.npc.alive, EK); A(&p.npc.count, size_t(E));
    A(&p.ego_dim, EN * 2); A(&p.npc_dim, EK * 2);  // car sizes (mev_set_car_dims), 54 x 24 until set
    A(&p.step_count, size_t(E)); A(&p.pending_reset, size_t(E)); A(&p.overflow, 3); A(&p.debug, size_t(E) * 8);
    A(&p.ob_box, size_t(E) * size_t(N + c.max_npcs)); A(&p.ob_cand, EN * 2);
    if (c.traffic_flow) {  // the fused traffic kernel's NPC-aware deal (mev_kernels.h, kDealLists)
        A(&p.deal_cnt, size_t(3) * mev::kDealRingInts);
        A(&p.deal_order, size_t(3) * mev::kDealLists * mev::kDealClasses * size_t(E));
    }
    // outputs
    A(&h->internal.obs, EN * size_t(D)); A(&h->internal.rew, EN); A(&h->internal.done, EN); A(&h->internal.status, EN);
    A(&h->internal.term, size_t(E)); A(&h->internal.trunc, size_t(E)); A(&h->internal.alive_cnt, size_t(E));
    A(&h->internal.step, size_t(E));
    // inputs & tables
    A(&h->d_actions, EN * 2); A(&h->d_spawn, size_t(E)); A(&h->d_mask, size_t(E));
    A(&h->d_paths, h->h_paths.size()); A(&h->d_rlen, h->h_len.size()); A(&h->d_pbox, h->h_pbox.size()); A(&h->d_spawn_tab, h->h_spawn.size()); A(&h->d_intent, h->h_intent.size());
    A(&h->d_rel, rel.size()); A(&h->d_traffic, size_t(h->P) * size_t(h->P));
    A(&h->d_reset_routes, size_t(h->P) * size_t(h->P));
    A(&h->d_lidar_table, size_t(256));
    A(reinterpret_cast<uint8_t**>(&h->d_sp), sizeof(mev::SimParams));
    float* d_dist = nullptr;
    if (!dist_mul_exact) A(&d_dist, dists.size());
    if (err != hipSuccess) {
        std::string m = hipGetErrorString(err);
        delete h;
        return fail(MEV_E_NOMEM, "device allocation failed: " + m);
    }
    h->internal.obs_ld = D;
    h->last = h->internal;
    // upload tables
    err = hipMemcpyAsync(h->d_paths, h->h_paths.data(), h->h_paths.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(h->d_spawn_tab, h->h_spawn.data(), h->h_spawn.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(h->d_pbox, h->h_pbox.data(), h->h_pbox.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(h->d_intent, h->h_intent.data(), h->h_intent.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(h->d_rlen, h->h_len.data(), h->h_len.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(h->d_rel, rel.data(), rel.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess && d_dist) err = hipMemcpyAsync(d_dist, dists.data(), dists.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess)
        err = hipMemcpyAsync(h->d_lidar_table, h->h_lidar_table.data(), 256 * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(h->d_traffic, h->h_traffic.data(), h->h_traffic.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    // every car of the reference's default size (Car.h:19-20); p.dims stays 0 while they all are
    std::vector<float> dflt(2 * std::max(EN, EK));
    for (size_t i = 0; i < dflt.size(); i += 2) { dflt[i] = mev::CAR_LENGTH; dflt[i + 1] = mev::CAR_WIDTH; }
    if (err == hipSuccess) err = hipMemcpyAsync(p.ego_dim, dflt.data(), EN * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(p.npc_dim, dflt.data(), EK * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream);
    // default ego routes: reference env.py:138-145 (mapping routes, cyclic)
    std::vector<int32_t> ego(EN);
    {
        const int L = c.num_lanes;
        const int (*map)[2] = (L == 2) ? kMap2 : kMap3;
        const int M = (L == 2) ? 7 : 12;
        std::vector<int32_t> valid;
        for (int k = 0; k < M; ++k) {
            const int s = map[k][0] - 1, e = 4 * L + map[k][1] - 1;
            if (map[k][0] <= 4 * L && map[k][1] <= 4 * L) valid.push_back(s * h->P + e);
        }
        if (valid.empty()) valid = h->h_traffic;
        for (size_t i = 0; i < EN; ++i) ego[i] = valid[(i % size_t(N)) % valid.size()];
    }
    if (err == hipSuccess) err = hipMemcpyAsync(p.ego.route, ego.data(), ego.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(h->stream);
    if (err != hipSuccess) {
        std::string m = hipGetErrorString(err);
        delete h;
        return fail(MEV_E_HIP, "table upload failed: " + m);
    }
    // parameters
    p.E = E; p.N = N; p.R = c.lidar_rays; p.K = c.max_npcs; p.D = D;
    p.lidar_slots = h->lidar_slots;
    p.num_lanes = wc.num_lanes;
    p.irw = wc.irw;
    p.line_stop = wc.line_stop;
    p.rw = wc.rw;
    p.use_team = c.use_team_reward;
    p.respawn = c.respawn_enabled;
    p.traffic = c.traffic_flow;
    p.max_steps = c.max_steps;
    p.k_prog = c.reward[0]; p.v_min = c.reward[1]; p.k_stuck = c.reward[2]; p.k_cv = c.reward[3];
    p.k_co = c.reward[4]; p.k_succ = c.reward[5]; p.k_sm = c.reward[6]; p.alpha = c.reward[7];
    p.max_progress = mev::world_max_progress();
    p.lidar_max = wc.lidar_max;
    p.lidar_step = wc.lidar_step;
    p.lidar_inv = wc.lidar_inv;
    p.lidar_steps = wc.lidar_steps;
    p.ob_stride = N + c.max_npcs;
    p.dist_tab = d_dist;
    p.seed = c.seed;
    p.rt.path = h->d_paths;
    p.rt.intent = h->d_intent;
    p.rt.spawn = h->d_spawn_tab;
    p.rt.pbox = reinterpret_cast<const float4*>(h->d_pbox);
    p.rt.nroutes = h->nroutes;
    p.rt.len = h->d_rlen;
    p.rt.plen = mev::PATH_LEN;
    p.rt.row = mev::ROUTE_PTS;
    p.rt.min_len = mev::PATH_LEN;
    p.rel_angles = h->d_rel;
    p.traffic_routes = h->d_traffic;
    p.n_traffic_routes = int(h->h_traffic.size());
    p.reset_routes = h->d_reset_routes;
    p.n_reset_routes = 0;
    // initial state = a reset (the reference env.py constructor ends with reset(), env.py:136)
    const int rc = mev_reset(h, nullptr, nullptr, 0);
    if (rc != MEV_OK) {
        const std::string m = g_err;
        delete h;
        *out = nullptr;
        return fail(rc, m);
    }
    h->serve_mark = g_host_tick.load(std::memory_order_relaxed);
    *out = h;
    return MEV_OK;
}

int mev_destroy(mev_handle* h) {
    if (!h) return MEV_OK;
    (void)hipSetDevice(h->cfg.device);
    (void)serve_stop(h);
    serve_unlist(h);
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return MEV_OK;
}

int mev_get_config(const mev_handle* h, mev_config* cfg) {
    if (!h || !cfg) return fail(MEV_E_INVALID, "null argument");
    *cfg = h->cfg;
    cfg->obs_dim = h->D;
    return MEV_OK;
}

int mev_obs_dim(const mev_handle* h, int32_t* d) {
    if (!h || !d) return fail(MEV_E_INVALID, "null argument");
    *d = h->D;
    return MEV_OK;
}

int mev_set_stream(mev_handle* h, void* stream) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));  // order the switch after outstanding work
    h->stream = static_cast<hipStream_t>(stream);  // NULL = the legacy default stream
    if (h->stream != h->own_stream) serve_unlist(h);  // (no server on a caller's stream: its slot goes)
    return MEV_OK;
}

int mev_use_own_stream(mev_handle* h) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->stream = h->own_stream;
    return MEV_OK;
}

int mev_debug_stamps(mev_handle* h, uint64_t* out) {
    if (!h || !out) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipMemcpyAsync(out, h->sp.debug, size_t(h->cfg.num_envs) * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MEV_OK;
}

int mev_sync(mev_handle* h) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MEV_OK;
}

int mev_configure(mev_handle* h, int32_t use_team, int32_t respawn, int32_t max_steps) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    h->cfg.use_team_reward = use_team;
    h->cfg.respawn_enabled = respawn;
    h->cfg.max_steps = max_steps;
    h->sp.use_team = use_team;
    h->sp.respawn = respawn;
    h->sp.max_steps = max_steps;
    return MEV_OK;
}

int mev_configure_traffic(mev_handle* h, int32_t enabled, float density) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (enabled && h->cfg.max_npcs == 0) return fail(MEV_E_INVALID, "traffic needs max_npcs > 0 (set at creation)");
    if (enabled && h->sp.step_kernel == 2) {
        mev::SimParams q = h->sp;
        q.traffic = 1;
        if (mev::plan_step(q).path == 0)
            return fail(MEV_E_INVALID, "the fused step kernel (mev_set_step_kernel 2) cannot hold this handle's NPC slots");
    }
    h->cfg.traffic_flow = enabled;
    h->deal_valid = false;
    h->cfg.traffic_density = density < 0.0f ? 0.0f : density;  // configure_traffic clamps (:56-60)
    h->sp.traffic = enabled;
    return MEV_OK;
}

int mev_set_reward(mev_handle* h, const float* rc) {
    if (!h || !rc) return fail(MEV_E_INVALID, "null argument");
    memcpy(h->cfg.reward, rc, sizeof(h->cfg.reward));
    mev::SimParams& p = h->sp;
    p.k_prog = rc[0]; p.v_min = rc[1]; p.k_stuck = rc[2]; p.k_cv = rc[3];
    p.k_co = rc[4]; p.k_succ = rc[5]; p.k_sm = rc[6]; p.alpha = rc[7];
    return MEV_OK;
}

int mev_car_update(float* kin, float throttle, float steer_input, float dt) {
    if (!kin) return fail(MEV_E_INVALID, "null argument");
    mev::Kin k{kin[0], kin[1], kin[2], kin[3], kin[4], kin[5]};
    float c, s;
    mev::car_update(k, throttle, steer_input, dt, &c, &s);
    kin[0] = k.x; kin[1] = k.y; kin[2] = k.v; kin[3] = k.h; kin[4] = k.acc; kin[5] = k.steer;
    return MEV_OK;
}

int mev_tanh(const float* x, float* y, int64_t n) {
    if (n < 0 || (n > 0 && (!x || !y))) return fail(MEV_E_INVALID, n < 0 ? "negative count" : "null argument");
    for (int64_t i = 0; i < n; ++i) y[i] = mev::tanh_c(x[i]);
    return MEV_OK;
}

static void box_corners(const float* b, float* cx, float* cy, float* c, float* s) {
    // Car::corners (cpp/Car.cpp:86-103) with the car's own length/width
    mev::sincosf(b[2], s, c);
    const float hx = b[4] * 0.5f, hy = b[3] * 0.5f;
    const float lx[4] = {hy, hy, -hy, -hy}, ly[4] = {hx, -hx, -hx, hx};
    for (int k = 0; k < 4; ++k) {
        cx[k] = b[0] + lx[k] * *c - ly[k] * *s;
        cy[k] = b[1] + lx[k] * *s + ly[k] * *c;
    }
}

int mev_car_check_collision(const float* a, const float* b, int32_t* collide) {
    if (!a || !b || !collide) return fail(MEV_E_INVALID, "null argument");
    float ax[4], ay[4], bx[4], by[4], ca, sa, cb, sb;
    box_corners(a, ax, ay, &ca, &sa);
    box_corners(b, bx, by, &cb, &sb);
    *collide = mev::sat_collide(ax, ay, ca, sa, bx, by, cb, sb) ? 1 : 0;
    return MEV_OK;
}

int mev_num_points(const mev_handle* h, int32_t* n) {
    if (!h || !n) return fail(MEV_E_INVALID, "null argument");
    *n = h->P;
    return MEV_OK;
}

int mev_point_xy(const mev_handle* h, int32_t point, float* xy) {
    if (!h || !xy) return fail(MEV_E_INVALID, "null argument");
    if (point < 0 || point >= h->P) return fail(MEV_E_RANGE, "lane point out of range");
    xy[0] = h->pts[size_t(point)].x;
    xy[1] = h->pts[size_t(point)].y;
    return MEV_OK;
}

int mev_route_id(const mev_handle* h, int32_t s, int32_t e, int32_t* route) {
    if (!h || !route) return fail(MEV_E_INVALID, "null argument");
    if (s < 0 || s >= h->P || e < 0 || e >= h->P) return fail(MEV_E_RANGE, "lane point out of range");
    *route = s * h->P + e;
    return MEV_OK;
}

int mev_route_len(const mev_handle* h, int32_t route, int32_t* npoints) {
    if (!h || !npoints) return fail(MEV_E_INVALID, "null argument");
    if (route < 0 || route >= h->nroutes) return fail(MEV_E_RANGE, "route out of range");
    *npoints = h->h_len[size_t(route)];
    return MEV_OK;
}

int mev_route_info(const mev_handle* h, int32_t route, float* path, int32_t* intent, float* spawn) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (route < 0 || route >= h->nroutes) return fail(MEV_E_RANGE, "route out of range");
    if (path) {  // max(n, PATH_LEN) points: a shorter path padded with its last point
        const int n = std::max(h->h_len[size_t(route)], mev::PATH_LEN);
        memcpy(path, &h->h_paths[size_t(route) * 2 * size_t(h->row_pts)], sizeof(float) * 2 * size_t(n));
    }
    if (intent) *intent = h->h_intent[size_t(route)];
    if (spawn) memcpy(spawn, &h->h_spawn[size_t(3 * route)], sizeof(float) * 3);
    return MEV_OK;
}

int mev_add_route(mev_handle* h, const float* path, int32_t intent, int32_t* route) {
    return mev_add_route_n(h, path, mev::PATH_LEN, intent, route);
}

namespace {
// a route-table row of `plen` points: the n points, padded with the last one, then the
// last segment at plen, plen + 1 and zeros up to plen + 16 (mev_world.h)
void fill_row(float* row, const float* pts, int n, int plen) {
    for (int i = 0; i < plen; ++i) {
        const int q = i < n ? i : n - 1;
        row[2 * i] = pts[2 * q];
        row[2 * i + 1] = pts[2 * q + 1];
    }
    std::copy(pts + 2 * (n - 2), pts + 2 * n, row + 2 * plen);
    std::fill(row + 2 * (plen + 2), row + 2 * (plen + 16), 0.0f);
}
}  // namespace

int mev_add_route_n(mev_handle* h, const float* path_in, int32_t npoints, int32_t intent, int32_t* route) {
    if (!h || !path_in || !route) return fail(MEV_E_INVALID, "null argument");
    if (intent < 0 || intent > 2) return fail(MEV_E_INVALID, "intent must be 0 (straight), 1 (left) or 2 (right)");
    if (npoints < 2 || npoints > mev::MAX_PATH_LEN) return fail(MEV_E_INVALID, "a route path has 2 .. 4096 points");
    for (int i = 0; i < 2 * npoints; ++i)
        if (!(fabsf(path_in[i]) < 1.0e6f)) return fail(MEV_E_INVALID, "path points must be finite (|coordinate| < 1e6)");
    if (h->nroutes >= 32767) return fail(MEV_E_INVALID, "too many routes (the state gather format ships i16 ids)");
    if (h->comm && h->gather_fmt == MEV_GATHER_STATE)  // every rank's route ids are decoded with the root's table
        return fail(MEV_E_INVALID, "routes cannot be added while a state-format gather communicator exists");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int r = h->nroutes;
    // a path longer than the rows re-lays the whole table out at the new length (rounded up to
    // 16 points, rows stay 128-B aligned); every row keeps its own n and its padding.  The
    // boxes of the other rows stay: their new padding is their last point, which their third
    // piece [110, old plen) already holds
    const int plen = npoints > h->plen ? (npoints + 15) & ~15 : h->plen;
    const int row_pts = plen + 16;
    const bool relayout = plen != h->plen;
    std::vector<float> old_paths;
    if (relayout) {
        old_paths.swap(h->h_paths);
        h->h_paths.resize(size_t(r) * 2 * size_t(row_pts));
        for (int q = 0; q < r; ++q)
            fill_row(&h->h_paths[size_t(q) * 2 * row_pts], &old_paths[size_t(q) * 2 * h->row_pts], h->h_len[size_t(q)],
                     plen);
    }
    h->h_paths.resize(size_t(r + 1) * 2 * size_t(row_pts));
    float* row = &h->h_paths[size_t(r) * 2 * row_pts];
    fill_row(row, path_in, npoints, plen);
    {  // the pieces [0, 50), [50, 110), [110, plen) of the padded row
        const int cut[4] = {0, 50, 110, plen};
        for (int q = 0; q < 3; ++q) {
            float x0 = row[2 * cut[q]], x1 = x0, y0 = row[2 * cut[q] + 1], y1 = y0;
            for (int i = cut[q]; i < cut[q + 1]; ++i) {
                x0 = std::min(x0, row[2 * i]); x1 = std::max(x1, row[2 * i]);
                y0 = std::min(y0, row[2 * i + 1]); y1 = std::max(y1, row[2 * i + 1]);
            }
            h->h_pbox.push_back(x0); h->h_pbox.push_back(x1); h->h_pbox.push_back(y0); h->h_pbox.push_back(y1);
        }
    }
    h->h_len.push_back(npoints);
    h->h_intent.push_back(intent);
    h->h_spawn.push_back(row[0]);  // add_car_with_route's spawn: the path's first point (RouteGen.cpp:111-205)
    h->h_spawn.push_back(row[1]);
    h->h_spawn.push_back(mev::spawn_heading(row));
    auto rollback = [&]() {
        if (relayout) h->h_paths.swap(old_paths);
        else h->h_paths.resize(size_t(r) * 2 * size_t(row_pts));
        h->h_len.pop_back();
        h->h_intent.pop_back();
        h->h_spawn.resize(h->h_spawn.size() - 3);
        h->h_pbox.resize(h->h_pbox.size() - 12);
    };
    // the five route tables: the new route's rows go into spare capacity; a full table (or a
    // re-laid-out one) is reallocated at twice the routes (so n added routes cost O(log n)
    // reallocations, each a hipFree that waits for the device) and uploaded whole
    const size_t per[5] = {2 * size_t(row_pts) * sizeof(float), sizeof(int32_t), 3 * sizeof(float), 12 * sizeof(float),
                           sizeof(int32_t)};
    const void* src[5] = {h->h_paths.data(), h->h_intent.data(), h->h_spawn.data(), h->h_pbox.data(), h->h_len.data()};
    const int cap = r >= h->route_cap ? std::min(32767, std::max(2 * h->route_cap, r + 1)) : h->route_cap;
    hipError_t e = hipSuccess;
    if (cap == h->route_cap && !relayout) {
        void* cur[5] = {h->d_paths, h->d_intent, h->d_spawn_tab, h->d_pbox, h->d_rlen};
        for (int k = 0; k < 5 && e == hipSuccess; ++k)
            e = hipMemcpy(static_cast<uint8_t*>(cur[k]) + size_t(r) * per[k],
                          static_cast<const uint8_t*>(src[k]) + size_t(r) * per[k], per[k], hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            rollback();
            return fail(MEV_E_HIP, std::string("route table: ") + hipGetErrorString(e));
        }
    } else {
        void* np[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; k < 5 && e == hipSuccess; ++k) {
            e = hipMalloc(&np[k], size_t(cap) * per[k]);
            if (e == hipSuccess) e = hipMemcpy(np[k], src[k], size_t(r + 1) * per[k], hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            for (void* q : np) if (q) (void)hipFree(q);
            rollback();
            return fail(MEV_E_NOMEM, std::string("route table: ") + hipGetErrorString(e));
        }
        void* old[5] = {h->d_paths, h->d_intent, h->d_spawn_tab, h->d_pbox, h->d_rlen};
        for (int k = 0; k < 5; ++k) {
            for (auto& a : h->allocs)
                if (a == old[k]) { (void)hipFree(a); a = np[k]; break; }
        }
        h->d_paths = static_cast<float*>(np[0]);
        h->d_intent = static_cast<int32_t*>(np[1]);
        h->d_spawn_tab = static_cast<float*>(np[2]);
        h->d_pbox = static_cast<float*>(np[3]);
        h->d_rlen = static_cast<int32_t*>(np[4]);
        h->route_cap = cap;
    }
    h->plen = plen;
    h->row_pts = row_pts;
    h->nroutes = r + 1;
    h->extend_route_hash();
    h->sp.rt.path = h->d_paths;
    h->sp.rt.intent = h->d_intent;
    h->sp.rt.spawn = h->d_spawn_tab;
    h->sp.rt.pbox = reinterpret_cast<const float4*>(h->d_pbox);
    h->sp.rt.len = h->d_rlen;
    h->sp.rt.nroutes = h->nroutes;  // (the next launch refreshes the device copy of the parameters)
    h->sp.rt.plen = plen;
    h->sp.rt.row = row_pts;
    h->sp.rt.min_len = std::min(h->sp.rt.min_len, int32_t(npoints));
    *route = r;
    return MEV_OK;
}

// ---- per-car sizes (reference Car::length / Car::width, cpp/Car.h:19-20, read-write
// through cpp/bindings.cpp:24-25): the SAT corners, the status corners and the LiDAR
// boxes of each car.  The device arrays always hold every car's size (54 x 24 until
// set); SimParams::dims says whether any differs, and only then do the steps run the
// runtime-layout kernels that read them (mev_kernels.hip, DIMS).
static bool all_default_dims(const float* d, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (d[2 * i] != mev::CAR_LENGTH || d[2 * i + 1] != mev::CAR_WIDTH) return false;
    return true;
}

int mev_set_car_dims(mev_handle* h, const float* ego_dims, const float* npc_dims) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    const size_t EN = size_t(h->cfg.num_envs) * size_t(h->cfg.num_agents);
    const size_t EK = size_t(h->cfg.num_envs) * size_t(h->cfg.max_npcs);
    for (int w = 0; w < 2; ++w) {
        const float* d = w ? npc_dims : ego_dims;
        const size_t n = 2 * (w ? EK : EN);
        if (d)
            for (size_t i = 0; i < n; ++i)
                if (!(fabsf(d[i]) <= 1.0e4f)) return fail(MEV_E_INVALID, "car length / width must be finite, |value| <= 1e4 px");
    }
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    if (ego_dims) HIP_TRY(hipMemcpyAsync(h->sp.ego_dim, ego_dims, EN * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (npc_dims && EK) HIP_TRY(hipMemcpyAsync(h->sp.npc_dim, npc_dims, EK * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    // the pools' slots were stored under the sizes' regime so far: none is valid under the next
    for (mev_pool* q : h->pools) HIP_TRY(hipMemsetAsync(q->st.valid, 0, size_t(q->slots), h->stream));
    // whether any car differs from 54 x 24: the arrays given, and the device's for the other
    std::vector<float> e(ego_dims ? 0 : EN * 2), k(npc_dims ? 0 : EK * 2);
    if (!e.empty()) HIP_TRY(hipMemcpyAsync(e.data(), h->sp.ego_dim, e.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (!k.empty()) HIP_TRY(hipMemcpyAsync(k.data(), h->sp.npc_dim, k.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const bool dflt = all_default_dims(ego_dims ? ego_dims : e.data(), EN) && all_default_dims(npc_dims ? npc_dims : k.data(), EK);
    h->sp.dims = dflt ? 0 : 1;  // (the next step refreshes the device copy of the parameters)
    h->deal_valid = false;      // (a dims handle runs another kernel: the deal restarts)
    return MEV_OK;
}

int mev_get_car_dims(mev_handle* h, float* ego_dims, float* npc_dims) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    const size_t EN = size_t(h->cfg.num_envs) * size_t(h->cfg.num_agents);
    const size_t EK = size_t(h->cfg.num_envs) * size_t(h->cfg.max_npcs);
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    if (ego_dims) HIP_TRY(hipMemcpyAsync(ego_dims, h->sp.ego_dim, EN * 2 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (npc_dims && EK) HIP_TRY(hipMemcpyAsync(npc_dims, h->sp.npc_dim, EK * 2 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MEV_OK;
}

int mev_car_dims_active(const mev_handle* h, int32_t* active) {
    if (!h || !active) return fail(MEV_E_INVALID, "null argument");
    *active = h->sp.dims;
    return MEV_OK;
}

// ---- LiDAR beam offsets (reference Lidar::rel_angles, cpp/Lidar.h:17, read-write through
// cpp/bindings.cpp:92): e.g. the first R angles of a longer beam list, which is what a
// reference Lidar whose `rays` was lowered casts (Lidar.cpp:24-25 indexes rel_angles up to
// rays).  The step's car-pair culling models the beams as rel[0] + b * (rel[R-1] - rel[0]) /
// (R - 1) with 2e-4 rad of margin (mev_kernels.hip phase 3b), so the offsets must be evenly
// spaced to 1e-5 rad; any other list is refused.
int mev_set_beam_angles(mev_handle* h, const float* rel) {
    if (!h || !rel) return fail(MEV_E_INVALID, "null argument");
    const int R = h->cfg.lidar_rays;
    for (int b = 0; b < R; ++b)
        if (!(fabsf(rel[b]) <= 1.0e3f)) return fail(MEV_E_INVALID, "beam angles must be finite, |angle| <= 1000 rad");
    h->sp.beam_cull = beam_cull_ok(rel, R);  // (any other list: no culling, SimParams::beam_cull)
    h->sp.beams = mev::beam_model(rel, R);   // (the step copies a changed SimParams to the device before it launches)
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->d_rel, rel, size_t(R) * sizeof(float), hipMemcpyHostToDevice));
    return MEV_OK;
}

int mev_get_beam_angles(mev_handle* h, float* rel) {
    if (!h || !rel) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(rel, h->d_rel, size_t(h->cfg.lidar_rays) * sizeof(float), hipMemcpyDeviceToHost));
    return MEV_OK;
}

int mev_set_ego_routes(mev_handle* h, const int32_t* routes) {
    if (!h || !routes) return fail(MEV_E_INVALID, "null argument");
    const size_t EN = size_t(h->cfg.num_envs) * size_t(h->cfg.num_agents);
    for (size_t i = 0; i < EN; ++i)
        if (routes[i] < 0 || routes[i] >= h->nroutes) return fail(MEV_E_RANGE, "ego route id out of range");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipMemcpyAsync(h->sp.ego.route, routes, EN * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MEV_OK;
}

int mev_set_traffic_routes(mev_handle* h, const int32_t* routes, int32_t count) {
    if (!h || (count > 0 && !routes)) return fail(MEV_E_INVALID, "null argument");
    if (count < 0 || count > h->P * h->P) return fail(MEV_E_INVALID, "bad traffic route count");
    for (int i = 0; i < count; ++i)
        if (routes[i] < 0 || routes[i] >= h->nroutes) return fail(MEV_E_RANGE, "traffic route id out of range");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    h->h_traffic.assign(routes, routes + count);
    if (count > 0)
        HIP_TRY(hipMemcpyAsync(h->d_traffic, routes, size_t(count) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->sp.n_traffic_routes = count;
    return MEV_OK;
}

int mev_default_traffic_routes(const mev_handle* h, int32_t* routes, int32_t* count) {
    if (!h || !count) return fail(MEV_E_INVALID, "null argument");
    const auto d = mev::default_traffic_routes(h->cfg.num_lanes);
    if (routes) memcpy(routes, d.data(), d.size() * sizeof(int32_t));
    *count = int32_t(d.size());
    return MEV_OK;
}

// (the caller's output pointers travel as a mev_step_args: its eight output fields, each optional)
static mev::Outputs resolve_outputs(mev_handle* h, const mev_step_args& a, bool device) {
    mev::Outputs o = h->internal;
    if (device) {
        if (a.obs) o.obs = a.obs;
        if (a.reward) o.rew = a.reward;
        if (a.done) o.done = a.done;
        if (a.status) o.status = a.status;
        if (a.terminated) o.term = a.terminated;
        if (a.truncated) o.trunc = a.truncated;
        if (a.agents_alive) o.alive_cnt = a.agents_alive;
        if (a.step) o.step = a.step;
    }
    return o;
}

static int copy_out(mev_handle* h, const mev::Outputs& src, const mev_step_args& a, hipMemcpyKind kind) {
    const size_t E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents);
    auto cp = [&](void* dst, const void* s, size_t bytes) -> hipError_t {
        if (!dst || dst == s) return hipSuccess;
        return hipMemcpyAsync(dst, s, bytes, kind, h->stream);
    };
    HIP_TRY(cp(a.obs, src.obs, EN * size_t(h->D) * sizeof(float)));
    HIP_TRY(cp(a.reward, src.rew, EN * sizeof(float)));
    HIP_TRY(cp(a.done, src.done, EN));
    HIP_TRY(cp(a.status, src.status, EN));
    HIP_TRY(cp(a.terminated, src.term, E));
    HIP_TRY(cp(a.truncated, src.trunc, E));
    HIP_TRY(cp(a.agents_alive, src.alive_cnt, E * sizeof(int32_t)));
    HIP_TRY(cp(a.step, src.step, E * sizeof(int32_t)));
    return MEV_OK;
}

// spawn probability, TrafficFlow.cpp:321-322 (host glibc expf, bit-identical to the reference)
static float spawn_prob(const mev_handle* h, float dt) { return 1.0f - expf(-h->cfg.traffic_density * dt); }

int mev_reset(mev_handle* h, const uint8_t* env_mask, float* obs, uint32_t flags) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const bool dev = (flags & MEV_DEVICE_PTRS) != 0;
    const uint8_t* d_mask = nullptr;
    if (env_mask) {
        if (dev) d_mask = env_mask;
        else {
            HIP_TRY(hipMemcpyAsync(h->d_mask, env_mask, size_t(h->cfg.num_envs), hipMemcpyHostToDevice, h->stream));
            d_mask = h->d_mask;
        }
    }
    mev::Outputs o = h->internal;
    if (dev && obs) o.obs = obs;
    h->deal_valid = false;  // NPC counts changed outside the step: the deal restarts
    HIP_TRY(mev::launch_reset(h->sp, d_mask, o, h->stream, h->rng_counter++));
    h->last.obs = o.obs;
    if (!dev) {
        if (obs) HIP_TRY(hipMemcpyAsync(obs, o.obs, size_t(h->cfg.num_envs) * size_t(h->cfg.num_agents) * size_t(h->D) * sizeof(float),
                                        hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return MEV_OK;
}

// the pinned zero-copy block of a small handle (created at its first host-mode step)
static bool pin_ready(mev_handle* h) {
    if (h->pin) return true;
    const size_t E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents);
    const size_t sz[10] = {EN * 2 * sizeof(float), E * sizeof(int32_t), EN * size_t(h->D) * sizeof(float),
                           EN * sizeof(float), EN, EN, E, E, E * sizeof(int32_t), E * sizeof(int32_t)};
    size_t off = 0;
    for (int k = 0; k < 10; ++k) {
        h->pin_off[k] = off;
        off += (sz[k] + 255) & ~size_t(255);
    }
    if (off - h->pin_off[2] > mev_handle::kPinMax) return false;  // large outputs: device buffers + DMA copies
    void* hp = nullptr;
    if (hipHostMalloc(&hp, off, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return false;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
        (void)hipHostFree(hp);
        return false;
    }
    h->pin = static_cast<uint8_t*>(hp);
    h->pin_dev = static_cast<uint8_t*>(dp);
    uint8_t* d = h->pin_dev;
    h->pin_out.obs = reinterpret_cast<float*>(d + h->pin_off[2]);
    h->pin_out.rew = reinterpret_cast<float*>(d + h->pin_off[3]);
    h->pin_out.done = d + h->pin_off[4];
    h->pin_out.status = d + h->pin_off[5];
    h->pin_out.term = d + h->pin_off[6];
    h->pin_out.trunc = d + h->pin_off[7];
    h->pin_out.alive_cnt = reinterpret_cast<int32_t*>(d + h->pin_off[8]);
    h->pin_out.step = reinterpret_cast<int32_t*>(d + h->pin_off[9]);
    h->pin_out.obs_ld = h->D;
    return true;
}

// ---- the persistent step server (k_serve; protocol in mev_kernels.h ServeBox) ----
namespace {
constexpr double kServeTimeoutMs = 10000.0;  // no answer within this: the call fails

inline void cpu_relax() {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
}

constexpr double kServeIdleMinUs = 200.0, kServeIdleMaxUs = 2000.0;
constexpr int kServeMissLimit = 4;        // consecutive posts that found the server gone ...
constexpr uint64_t kPausedSteps = 1024;  // ... pause serving for this many host steps

// the idle limit of the next instance, in ticks of s_memrealtime (100 MHz):
// MEV_SERVE_IDLE_MS fixes it (1..1000 ms); otherwise adaptive (mev_handle::serve_gap_us)
uint32_t serve_idle_ticks(const mev_handle* h) {
    static const int fixed_ms = [] {
        const char* v = getenv("MEV_SERVE_IDLE_MS");
        if (!v) return 0;
        const int m = atoi(v);
        return m < 1 ? 1 : (m > 1000 ? 1000 : m);
    }();
    if (fixed_ms > 0) return (uint32_t)fixed_ms * 100000u;
    double us = 8.0 * h->serve_gap_us;
    us = us < kServeIdleMinUs ? kServeIdleMinUs : (us > kServeIdleMaxUs ? kServeIdleMaxUs : us);
    return (uint32_t)(us * 100.0);
}

// post a command: the line's fields are written by the caller, then cmd, then seq (release)
void serve_post(mev_handle* h, uint32_t cmd) {
    volatile mev::ServeBox* b = h->sbox;
    b->cmd = cmd;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    b->seq = ++h->serve_seq;
    std::atomic_thread_fence(std::memory_order_seq_cst);
}

int serve_launch(mev_handle* h) {
    mev::ServeArgs sa{};
    sa.box = h->sbox_dev;
    sa.actions = reinterpret_cast<const float*>(h->pin_dev + h->pin_off[0]);
    sa.spawn_route = reinterpret_cast<const int32_t*>(h->pin_dev + h->pin_off[1]);
    sa.epoch = ++h->serve_epoch;
    sa.idle_ticks = serve_idle_ticks(h);
    HIP_TRY(hipEventRecord(h->serve_ev, h->stream));  // after whatever the handle's stream holds
    HIP_TRY(hipStreamWaitEvent(h->serve_stream, h->serve_ev, 0));
    HIP_TRY(mev::launch_serve(h->sp, h->d_sp, sa, h->pin_out, h->serve_stream));
    h->serve_running = true;
    h->serve_wg = h->sp.E;
    ++h->serve_launches;
    return MEV_OK;
}

// Resident servers per process are capped: their high-priority hardware queues are
// few, and a server launched behind another one's on a shared queue would wait for its
// idle exit.  Handles beyond the cap step launched (same results).  A slot belongs to
// the handle that took it -- across its server's idle exits and paused stretches --
// until the handle is closed, or has made no host step for kServeStaleMs, and none since
// the previous step (or the creation) of another handle that asks for a slot: which
// handles are served does not depend on the timing of idle exits or on pauses of the
// host (a round-robin over more handles than slots serves the first ones).
constexpr int kMaxResidentServers = 2;
constexpr int64_t kServeStaleMs = 50;
std::mutex g_serve_mu;
std::vector<mev_handle*> g_serving;  // the slots' owners (<= kMaxResidentServers)

int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// whether h's server is still resident (some workgroup has not yet left)
bool serve_resident(const mev_handle* h) {
    if (!h->serve_running) return false;
    const volatile mev::ServeBox* b = h->sbox;
    for (int w = 0; w < h->serve_wg; ++w)
        if (b->exited[w] != h->serve_epoch) return true;
    return false;
}

// h may keep or start a resident server: it owns a slot, or takes a free one (or
// one whose owner has stepped no host step for kServeStaleMs, none since h's step
// before this one -- `mark` -- and has no server left)
bool serve_slot(mev_handle* h, uint64_t mark) {
    std::lock_guard<std::mutex> lk(g_serve_mu);
    for (const mev_handle* x : g_serving)
        if (x == h) return true;
    if ((int)g_serving.size() >= kMaxResidentServers) {
        const int64_t t = now_ns();
        for (size_t i = 0; i < g_serving.size(); ++i) {
            const mev_handle* x = g_serving[i];
            if (!serve_resident(x) && x->serve_last_tick.load(std::memory_order_relaxed) <= mark &&
                t - x->serve_last_ns.load(std::memory_order_relaxed) > kServeStaleMs * 1000000) {
                g_serving.erase(g_serving.begin() + long(i));
                break;
            }
        }
    }
    if ((int)g_serving.size() >= kMaxResidentServers) return false;
    g_serving.push_back(h);
    return true;
}

void serve_unlist(mev_handle* h) {
    std::lock_guard<std::mutex> lk(g_serve_mu);
    for (size_t i = 0; i < g_serving.size(); ++i)
        if (g_serving[i] == h) {
            g_serving.erase(g_serving.begin() + long(i));
            break;
        }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

// Stop a resident server (every other call on the handle does this first): post
// STOP, wait until every workgroup has left, then the stream is free.
static int serve_stop(mev_handle* h) {
    if (!h->serve_running) return MEV_OK;
    serve_post(h, mev::kServeStop);
    volatile mev::ServeBox* b = h->sbox;
    const auto t0 = std::chrono::steady_clock::now();
    for (int w = 0; w < h->serve_wg; ++w)
        while (b->exited[w] != h->serve_epoch) {
            if (ms_since(t0) > kServeTimeoutMs) return fail(MEV_E_HIP, "step server: no stop within 10 s");
            cpu_relax();
        }
    h->serve_running = false;
    HIP_TRY(hipStreamSynchronize(h->serve_stream));  // the server's grid has drained
    return MEV_OK;
}

// whether a host-mode step of h (pinned block ready) goes to the server
static bool serve_wanted(mev_handle* h) {
    static const bool off = [] { const char* v = getenv("MEV_NO_SERVE"); return v && v[0] == '1'; }();
    // (only on the handle's own non-blocking stream: a resident server would hold back
    // whatever a caller queues behind it on a stream it shares)
    if (off || h->serve_mode == 0 || !h->tev.empty() || h->stream != h->own_stream || !mev::plan_step(h->sp).serve_fits)
        return false;
    if (h->serve_pause > 0) {  // repeated idle exits between posts: launched steps for a while
        --h->serve_pause;
        return false;
    }
    if (h->sbox) return true;
    if (!h->serve_stream || !h->serve_ev) {
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return false;
        if (hipStreamCreateWithPriority(&h->serve_stream, hipStreamNonBlocking, hi) != hipSuccess) {
            h->serve_stream = nullptr;
            return false;
        }
        if (hipEventCreateWithFlags(&h->serve_ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamDestroy(h->serve_stream);
            h->serve_stream = nullptr;
            h->serve_ev = nullptr;
            return false;
        }
    }
    void* hp = nullptr;
    if (hipHostMalloc(&hp, sizeof(mev::ServeBox), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return false;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) {
        (void)hipHostFree(hp);
        return false;
    }
    memset(hp, 0, sizeof(mev::ServeBox));
    h->sbox = static_cast<mev::ServeBox*>(hp);
    h->sbox_dev = static_cast<mev::ServeBox*>(dp);
    return true;
}

// one step through the server: post it (launching an instance if none is
// resident) and wait until every workgroup has answered.  A workgroup that left
// (idle) without answering: the instance is stopped, the same step (same sid) is
// posted again and a new instance launched; workgroups that had answered skip it.
static int serve_step(mev_handle* h, const mev::StepInputs& in) {
    volatile mev::ServeBox* b = h->sbox;
    if (h->serve_running) {  // the host gap since the last answer, and whether the server waited for it
        const double gap_us = 1000.0 * ms_since(h->serve_t_answer);
        h->serve_gap_us = 0.875 * h->serve_gap_us + 0.125 * (gap_us < kServeIdleMaxUs ? gap_us : kServeIdleMaxUs);
        if (b->exited[0] != h->serve_epoch) {  // still resident: a hit
            h->serve_misses = 0;
        } else {  // it left (idle) before this post
            ++h->serve_misses_total;
            if (++h->serve_misses >= kServeMissLimit) {
                h->serve_misses = 0;
                h->serve_pause = kPausedSteps;
            }
        }
    }
    const uint32_t sid = ++h->serve_sid;
    uint32_t u;
    b->sid = sid;
    memcpy(&u, &in.dt, 4);
    b->dt = u;
    memcpy(&u, &in.spawn_prob, 4);
    b->spawn_prob = u;
    b->auto_reset = (uint32_t)in.auto_reset;
    b->spawn = in.spawn_route ? 1u : 0u;
    b->rng_lo = (uint32_t)in.rng_counter;
    b->rng_hi = (uint32_t)(in.rng_counter >> 32);
    serve_post(h, mev::kServeStep);
    if (!h->serve_running)
        if (int r = serve_launch(h)) return r;
    const auto t0 = std::chrono::steady_clock::now();
    for (int w = 0; w < h->serve_wg; ++w) {
        while (b->done[w] != sid) {
            if (b->exited[w] == h->serve_epoch) {
                std::atomic_thread_fence(std::memory_order_seq_cst);
                if (b->done[w] == sid) break;  // answered, then left
                if (int r = serve_stop(h)) return r;
                serve_post(h, mev::kServeStep);  // the same step again
                if (int r = serve_launch(h)) return r;
                w = 0;
                continue;
            }
            if (ms_since(t0) > kServeTimeoutMs) return fail(MEV_E_HIP, "step server: no answer within 10 s");
            cpu_relax();
        }
    }
    std::atomic_thread_fence(std::memory_order_seq_cst);
    ++h->serve_steps;
    h->serve_t_answer = std::chrono::steady_clock::now();
    return MEV_OK;
}

int mev_set_serve(mev_handle* h, int32_t mode) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (mode != 0 && mode != 1) return fail(MEV_E_INVALID, "serve mode must be 0 (off) or 1 (automatic)");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;
    h->serve_mode = mode;
    if (mode == 0) serve_unlist(h);  // (its slot, if it owns one, goes to the next handle that asks)
    return MEV_OK;
}

int mev_serve_stats(const mev_handle* h, uint64_t* steps, uint64_t* launches, int32_t* running) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (steps) *steps = h->serve_steps;
    if (launches) *launches = h->serve_launches;
    if (running) *running = h->serve_running ? 1 : 0;
    return MEV_OK;
}

int mev_step(mev_handle* h, const mev_step_args* a) {
    if (!h || !a) return fail(MEV_E_INVALID, "null argument");
    if (!a->actions) return fail(MEV_E_INVALID, "actions required");
    const bool gather = (a->flags & MEV_GATHER_TO_ROOT) != 0;
    if (gather) {
        if (!h->comm) return fail(MEV_E_INVALID, "MEV_GATHER_TO_ROOT needs a communicator (mev_comm_init)");
        if (a->obs || a->reward || a->done || a->status || a->terminated || a->truncated)
            return fail(MEV_E_INVALID, "MEV_GATHER_TO_ROOT writes the outputs packed: pass NULL output pointers");
    }
    HIP_TRY(hipSetDevice(h->cfg.device));
    const bool dev = (a->flags & MEV_DEVICE_PTRS) != 0;
    const size_t E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents);
    mev::StepInputs in{};
    in.dt = a->dt;
    in.auto_reset = (a->flags & MEV_AUTO_RESET) ? 1 : 0;
    in.rng_counter = h->rng_counter++;
    const bool pinned = !dev && !gather && pin_ready(h);  // zero-copy host mode (small handles)
    const uint64_t mark = h->serve_mark;
    if (pinned) {  // (a slot owner keeps stepping)
        h->serve_last_ns.store(now_ns(), std::memory_order_relaxed);
        h->serve_mark = g_host_tick.fetch_add(1, std::memory_order_relaxed) + 1;
        h->serve_last_tick.store(h->serve_mark, std::memory_order_relaxed);
    }
    const bool serve = pinned && serve_wanted(h) && serve_slot(h, mark);  // ... answered by the resident step server
    if (!serve)
        if (int r = serve_stop(h)) return r;
    if (dev) {
        in.actions = a->actions;
        in.spawn_route = a->spawn_route;
    } else if (pinned) {
        // the previous host-mode step was synchronized: the block is free
        memcpy(h->pin + h->pin_off[0], a->actions, EN * 2 * sizeof(float));
        in.actions = reinterpret_cast<const float*>(h->pin_dev + h->pin_off[0]);
        if (a->spawn_route) {
            memcpy(h->pin + h->pin_off[1], a->spawn_route, E * sizeof(int32_t));
            in.spawn_route = reinterpret_cast<const int32_t*>(h->pin_dev + h->pin_off[1]);
        }
    } else {
        HIP_TRY(hipMemcpyAsync(h->d_actions, a->actions, EN * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        in.actions = h->d_actions;
        if (a->spawn_route) {
            HIP_TRY(hipMemcpyAsync(h->d_spawn, a->spawn_route, E * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            in.spawn_route = h->d_spawn;
        }
    }
    in.spawn_prob = spawn_prob(h, a->dt);
    mev::Outputs o = pinned ? h->pin_out : resolve_outputs(h, *a, dev);
    const int slot = int(h->gathers & 1);
    if (gather) {
        // this rank's packed slot: on the root its own row of the gather buffer
        // (no copy), elsewhere the send buffer; step t and t+2 share a buffer
        if (h->gather_pending[slot]) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_gather[slot], 0));
        uint8_t* base = h->pk_buf[slot] + (h->rank == h->root ? size_t(h->root) * h->pk_bytes : 0);
        o.obs = reinterpret_cast<float*>(base + h->pk_off[MEV_PK_OBS]);
        o.rew = reinterpret_cast<float*>(base + h->pk_off[MEV_PK_REWARD]);
        o.done = base + h->pk_off[MEV_PK_DONE];
        o.status = base + h->pk_off[MEV_PK_STATUS];
        o.term = base + h->pk_off[MEV_PK_TERMINATED];
        o.trunc = base + h->pk_off[MEV_PK_TRUNCATED];
        if (h->gather_fmt == MEV_GATHER_STATE) {  // post-step state + one LiDAR code per beam, no heads
            o.obs = nullptr;
            o.obs_ld = 0;
            o.lidar_u8 = base + h->pk_off[MEV_PK_LIDAR];
            o.state = base + h->pk_off[MEV_PK_STATE];
            o.state_n = int64_t(h->slots) * h->cfg.num_agents;
        } else if (h->gather_fmt == MEV_GATHER_LIDAR_U8) {  // heads [slots][N][31] + one LiDAR code per beam
            o.obs_ld = mev::OBS_HEAD;
            o.lidar_u8 = base + h->pk_off[MEV_PK_LIDAR];
        }
    }
    const hipEvent_t* ev = nullptr;
    if (!h->tev.empty() && (h->t_phase++ % h->t_every) == 0) {
        if (size_t(3 * (h->tn + 1)) > h->tev.size()) HIP_TRY(h->fold_timing());
        ev = &h->tev[size_t(3 * h->tn)];
        ++h->tn;
    }
    if (!h->sp_valid || memcmp(&h->sp, &h->sp_dev, sizeof(mev::SimParams)) != 0) {
        // parameters changed (configuration calls only): stream-ordered after the
        // launches that read the previous copy; waited for, so the host copy is free
        if (int r = serve_stop(h)) return r;
        HIP_TRY(hipMemcpyAsync(h->d_sp, &h->sp, sizeof(mev::SimParams), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        memcpy(&h->sp_dev, &h->sp, sizeof(mev::SimParams));
        h->sp_valid = true;
    }
    // the NPC-aware deal (fused traffic k_step only; mev_set_env_deal)
    const bool deal = !serve && h->sp.traffic && h->sp.deal_cnt && h->deal_on && mev::plan_step(h->sp).path == 2;
    // classes are NPC-slot counts the next step loads (mev_kernels.hip cars_pre): rings whose
    // ended envs were put in class 0 by an auto-resetting step are not a bound for a step
    // without the reset (the env keeps its NPCs), so such a step deals afresh
    if (h->deal_valid && h->deal_ar && !in.auto_reset) h->deal_valid = false;
    if (deal) {
        if (!h->deal_valid) {  // fresh rings: this step deals by the identity order and builds the next
            HIP_TRY(hipMemsetAsync(h->sp.deal_cnt, 0, size_t(3) * mev::kDealRingInts * sizeof(int32_t), h->stream));
            h->deal_ring = 0;
        }
        in.deal = 2 | (h->deal_valid ? 1 : 0);
        in.deal_ring = h->deal_ring;
    }
    if (serve) {
        if (int r = serve_step(h, in)) return r;
    } else {
        HIP_TRY(mev::launch_step(h->sp, h->d_sp, in, o, h->stream, ev));
    }
    h->deal_valid = deal;
    h->deal_ar = in.auto_reset != 0;
    if (deal) h->deal_ring = h->deal_ring == 2 ? 0 : h->deal_ring + 1;
    h->last = o;
    if (gather && h->world == 1) {
        ++h->gathers;  // a world of one: the root's row is written in place, nothing to move
    } else if (gather) {
        // one grouped send/recv on the communication stream, after the step
        HIP_TRY(hipEventRecord(h->ev_step[slot], h->stream));
        HIP_TRY(hipStreamWaitEvent(h->comm_stream, h->ev_step[slot], 0));
        {
            ncclResult_t nr = ncclGroupStart();
            if (h->rank == h->root) {
                for (int r = 0; r < h->world && nr == ncclSuccess; ++r)
                    if (r != h->root)
                        nr = ncclRecv(h->pk_buf[slot] + size_t(r) * h->pk_bytes, h->pk_bytes, ncclUint8, r, h->comm,
                                      h->comm_stream);
            } else {
                nr = ncclSend(h->pk_buf[slot], h->pk_bytes, ncclUint8, h->root, h->comm, h->comm_stream);
            }
            const ncclResult_t ne = ncclGroupEnd();
            if (nr == ncclSuccess) nr = ne;
            if (nr != ncclSuccess) return fail(MEV_E_HIP, std::string("RCCL gather: ") + ncclGetErrorString(nr));
        }
        HIP_TRY(hipEventRecord(h->ev_gather[slot], h->comm_stream));
        h->gather_pending[slot] = true;
        ++h->gathers;
    }
    if (pinned) {
        if (!serve) HIP_TRY(hipStreamSynchronize(h->stream));
        const size_t EN_ = EN, E_ = E;
        auto cp = [&](void* dst, int k, size_t bytes) {
            if (dst) memcpy(dst, h->pin + h->pin_off[k], bytes);
        };
        cp(a->obs, 2, EN_ * size_t(h->D) * sizeof(float));
        cp(a->reward, 3, EN_ * sizeof(float));
        cp(a->done, 4, EN_);
        cp(a->status, 5, EN_);
        cp(a->terminated, 6, E_);
        cp(a->truncated, 7, E_);
        cp(a->agents_alive, 8, E_ * sizeof(int32_t));
        cp(a->step, 9, E_ * sizeof(int32_t));
    } else if (!dev) {
        int r = copy_out(h, o, *a, hipMemcpyDeviceToHost);
        if (r) return r;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return MEV_OK;
}

// A window (mev_step_repeat, mev_step_sequence; include/marlenv.h): up to n sub-steps of every env
// in one launch, one LiDAR cast.  Each entry point checks its own arguments and describes its
// window; step_window runs it.
struct WindowArgs {
    int n;                // sub-steps, 1..MEV_MAX_REPEAT
    bool plan;            // step.actions is [n][E][N][2], a row per sub-step (else: one held [E][N][2] row)
    const float* dt_seq;  // optional [n], host (else step.dt in every sub-step)
    int32_t* substeps;    // optional [E]
    float* reward_seq;    // optional [n][E][N] rows of the sub-steps' own outputs (a plan's)
    uint8_t* done_seq;
    uint8_t* status_seq;
};

static int step_window(mev_handle* h, const mev_step_args* a, const WindowArgs& w) {
    static_assert(mev::kMaxSeq == MEV_MAX_REPEAT, "the kernel's by-value dt / spawn_prob rows");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    const bool dev = (a->flags & MEV_DEVICE_PTRS) != 0;
    const int n = w.n;
    const size_t E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents);
    // a held action: one row, and no rows for the kernel
    mev::SeqRows rows{};
    const size_t act_rows = w.plan ? size_t(n) : 1;
    const mev::SeqRows* krows = w.plan ? &rows : nullptr;
    // each row's dt and spawn probability (as mev_step), read from the caller's memory now; a
    // plan's travel by value with the kernel's arguments
    for (size_t s = 0; s < act_rows; ++s) {
        rows.dt[s] = w.dt_seq ? w.dt_seq[s] : a->dt;
        rows.spawn_prob[s] = spawn_prob(h, rows.dt[s]);
    }
    mev::StepInputs in{};
    in.dt = rows.dt[0];
    in.spawn_prob = rows.spawn_prob[0];
    in.auto_reset = (a->flags & MEV_AUTO_RESET) ? 1 : 0;
    in.rng_counter = h->rng_counter;  // sub-step s: + s (k_cars_repeat)
    int32_t* d_sub = nullptr;
    Stage st(h, dev);
    st.in(&in.actions, a->actions, act_rows * EN * 2);
    st.in(&in.spawn_route, a->spawn_route, size_t(n) * E);
    st.out(&d_sub, w.substeps, E);
    st.out(&rows.reward, w.reward_seq, size_t(n) * EN);
    st.out(&rows.done, w.done_seq, size_t(n) * EN);
    st.out(&rows.status, w.status_seq, size_t(n) * EN);
    if (int r = st.upload()) return r;
    h->rng_counter += uint64_t(n);
    const mev::Outputs o = resolve_outputs(h, *a, dev);
    h->deal_valid = false;  // NPC counts change outside the fused step: the deal restarts
    HIP_TRY(mev::launch_step_window(h->sp, in, o, n, krows, d_sub, h->stream));
    h->last = o;
    if (!dev)  // (the step's own outputs: from the handle's buffers, as mev_step)
        if (int r = copy_out(h, o, *a, hipMemcpyDeviceToHost)) return r;
    return st.download();
}

int mev_step_repeat(mev_handle* h, const mev_repeat_args* ra) {
    if (!h || !ra) return fail(MEV_E_INVALID, "null argument");
    const mev_step_args* a = &ra->step;
    if (!a->actions) return fail(MEV_E_INVALID, "actions required");
    if (ra->repeat < 1 || ra->repeat > MEV_MAX_REPEAT)
        return fail(MEV_E_INVALID, "repeat must be in 1.." + std::to_string(MEV_MAX_REPEAT));
    if (a->flags & MEV_GATHER_TO_ROOT) return fail(MEV_E_INVALID, "mev_step_repeat does not gather (MEV_GATHER_TO_ROOT)");
    return step_window(h, a, WindowArgs{ra->repeat, false, nullptr, ra->substeps, nullptr, nullptr, nullptr});
}

int mev_step_sequence(mev_handle* h, const mev_sequence_args* sa) {
    if (!h || !sa) return fail(MEV_E_INVALID, "null argument");
    const mev_step_args* a = &sa->step;
    if (!a->actions) return fail(MEV_E_INVALID, "actions required");
    if (sa->length < 1 || sa->length > MEV_MAX_REPEAT)
        return fail(MEV_E_INVALID, "length must be in 1.." + std::to_string(MEV_MAX_REPEAT));
    if (a->flags & MEV_GATHER_TO_ROOT) return fail(MEV_E_INVALID, "mev_step_sequence does not gather (MEV_GATHER_TO_ROOT)");
    return step_window(h, a, WindowArgs{sa->length, true, sa->dt_seq, sa->substeps, sa->reward_seq, sa->done_seq,
                                    sa->status_seq});
}

// ---- closed-loop policy rollouts (include/marlenv.h: mev_policy_*, mev_rollout_policy)
static int sync_internal(mev_handle* h);  // below, with mev_device_outputs
// A policy: one device block holding each used layer's transposed weights and bias row (mev::PolicyNet).
static int policy_shape(const mev_handle* h, const mev_policy_spec* spec, mev::PolicyNet* net) {
    if (spec->in_dim != h->D)
        return fail(MEV_E_INVALID, "policy in_dim must equal the handle's obs_dim (" + std::to_string(h->D) + ")");
    if (spec->hidden[0] < 1 || spec->hidden[0] > MEV_POLICY_MAX_WIDTH || spec->hidden[1] < 0 ||
        spec->hidden[1] > MEV_POLICY_MAX_WIDTH)
        return fail(MEV_E_INVALID, "policy hidden widths must be in 1.." + std::to_string(MEV_POLICY_MAX_WIDTH) +
                                       " (hidden[1] == 0: one hidden layer)");
    *net = mev::PolicyNet{};
    net->layers = spec->hidden[1] ? 3 : 2;
    const int widths[4] = {spec->in_dim, spec->hidden[0], spec->hidden[1] ? spec->hidden[1] : 2, 2};
    for (int l = 0; l < net->layers; ++l) {
        net->in[l] = widths[l];
        net->out[l] = widths[l + 1];
        net->ld[l] = (widths[l + 1] + mev::WAVE - 1) / mev::WAVE * mev::WAVE;
        if (!spec->w[l] || !spec->b[l]) return fail(MEV_E_INVALID, "policy layer " + std::to_string(l) + ": null weights or biases");
    }
    return MEV_OK;
}

// the spec's weights into the policy's block: staged (host pointers: checked finite first) and repacked on the stream
// (the activation bits: at creation only, kept by every update)
static_assert(MEV_POLICY_HIDDEN_TANH == (uint32_t)mev::kPolicyHiddenTanh && MEV_POLICY_OUT_TANH == (uint32_t)mev::kPolicyOutTanh,
              "the header's activation bits are PolicyNet::act's");
static int policy_load(mev_policy* p, const mev_policy_spec* spec, uint32_t flags) {
    mev_handle* h = p->h;
    constexpr uint32_t kAct = MEV_POLICY_HIDDEN_TANH | MEV_POLICY_OUT_TANH;
    const bool update = p->net.layers != 0;
    if (update && (flags & kAct))
        return fail(MEV_E_INVALID, "mev_policy_update: a policy's activations are fixed at creation (flags: MEV_DEVICE_PTRS or 0)");
    if (flags & ~(MEV_DEVICE_PTRS | (update ? 0u : kAct)))
        return fail(MEV_E_INVALID, update ? "policy flags: MEV_DEVICE_PTRS or 0"
                                          : "policy flags: MEV_DEVICE_PTRS, MEV_POLICY_HIDDEN_TANH, MEV_POLICY_OUT_TANH or 0");
    mev::PolicyNet net{};
    if (int r = policy_shape(h, spec, &net)) return r;
    net.act = update ? p->net.act : (int32_t)(flags & kAct);
    if (p->net.layers && (net.layers != p->net.layers || memcmp(net.out, p->net.out, sizeof net.out) != 0))
        return fail(MEV_E_INVALID, "mev_policy_update: the spec's shape differs from the policy's");
    const bool dev = (flags & MEV_DEVICE_PTRS) != 0;
    if (!dev)
        for (int l = 0; l < net.layers; ++l) {
            const size_t nw = size_t(net.in[l]) * size_t(net.out[l]);
            for (size_t i = 0; i < nw; ++i)
                if (!std::isfinite(spec->w[l][i])) return fail(MEV_E_INVALID, "policy layer " + std::to_string(l) + ": a weight is not finite");
            for (int i = 0; i < net.out[l]; ++i)
                if (!std::isfinite(spec->b[l][i])) return fail(MEV_E_INVALID, "policy layer " + std::to_string(l) + ": a bias is not finite");
        }
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    if (!p->block) {
        size_t floats = 0;
        for (int l = 0; l < net.layers; ++l) floats += size_t(net.in[l] + 1) * size_t(net.ld[l]);
        const hipError_t err = dalloc(&p->block, floats);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            return fail(MEV_E_NOMEM, std::string("device allocation failed: ") + hipGetErrorString(err));
        }
    }
    float* at = p->block;
    for (int l = 0; l < net.layers; ++l) {
        net.wt[l] = at;
        at += size_t(net.in[l] + 1) * size_t(net.ld[l]);
    }
    const float* w[3] = {nullptr, nullptr, nullptr};
    const float* b[3] = {nullptr, nullptr, nullptr};
    Stage st(h, dev);
    for (int l = 0; l < net.layers; ++l) {
        st.in(&w[l], spec->w[l], size_t(net.in[l]) * size_t(net.out[l]));
        st.in(&b[l], spec->b[l], size_t(net.out[l]));
    }
    if (int r = st.upload()) return r;
    HIP_TRY(mev::launch_policy_repack(net, w, b, p->has_value, h->stream));
    p->net = net;
    return st.download();
}

// mev_policy_set_value_head: the head's column of the last layer's block, staged and written on the stream
// as policy_load does the layers (which leave that column alone while a head is attached)
int mev_policy_set_value_head(mev_policy* p, const float* wv, const float* bv, uint32_t flags) {
    if (!p) return fail(MEV_E_INVALID, "null argument");
    mev_handle* h = p->h;
    if (flags & ~MEV_DEVICE_PTRS) return fail(MEV_E_INVALID, "policy flags: MEV_DEVICE_PTRS or 0");
    if (wv && !bv) return fail(MEV_E_INVALID, "value head: null bias");
    const bool dev = (flags & MEV_DEVICE_PTRS) != 0;
    const size_t n = size_t(p->net.in[p->net.layers - 1]);
    if (wv && !dev) {
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(wv[i])) return fail(MEV_E_INVALID, "value head: a weight is not finite");
        if (!std::isfinite(bv[0])) return fail(MEV_E_INVALID, "value head: the bias is not finite");
    }
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    const float *dw = nullptr, *db = nullptr;
    Stage st(h, dev);
    st.in(&dw, wv, n);
    st.in(&db, wv ? bv : nullptr, 1);
    if (int r = st.upload()) return r;
    HIP_TRY(mev::launch_value_head_repack(p->net, dw, db, h->stream));
    p->has_value = wv != nullptr;
    return st.download();
}

int mev_policy_has_value_head(const mev_policy* p, int32_t* has) {
    if (!p || !has) return fail(MEV_E_INVALID, "null argument");
    *has = p->has_value ? 1 : 0;
    return MEV_OK;
}

int mev_policy_get_activations(const mev_policy* p, uint32_t* flags) {
    if (!p || !flags) return fail(MEV_E_INVALID, "null argument");
    *flags = (uint32_t)p->net.act;
    return MEV_OK;
}

int mev_policy_create(mev_handle* h, const mev_policy_spec* spec, uint32_t flags, mev_policy** out) {
    if (!h || !spec || !out) return fail(MEV_E_INVALID, "null argument");
    *out = nullptr;
    mev_policy* p = new mev_policy;
    p->h = h;
    if (int r = policy_load(p, spec, flags)) {
        if (p->block) (void)hipFree(p->block);
        delete p;
        return r;
    }
    h->policies.push_back(p);
    *out = p;
    return MEV_OK;
}

int mev_policy_update(mev_policy* p, const mev_policy_spec* spec, uint32_t flags) {
    if (!p || !spec) return fail(MEV_E_INVALID, "null argument");
    return policy_load(p, spec, flags);
}

int mev_policy_destroy(mev_policy* p) {
    if (!p) return MEV_OK;
    mev_handle* h = p->h;
    (void)hipSetDevice(h->cfg.device);
    (void)serve_stop(h);
    (void)hipStreamSynchronize(h->stream);  // (a rollout in flight may still read it)
    for (size_t i = 0; i < h->policies.size(); ++i)
        if (h->policies[i] == p) {
            h->policies.erase(h->policies.begin() + long(i));
            break;
        }
    if (p->block) (void)hipFree(p->block);
    delete p;
    return MEV_OK;
}

static mev::RolloutPlan rollout_plan(const mev_handle* h, int hidden) {
    return mev::plan_rollout(mev::step_shape(h->sp), h->D, hidden);
}

int mev_get_rollout_row(const mev_handle* h, int32_t* row) {
    if (!h || !row) return fail(MEV_E_INVALID, "null argument");
    *row = rollout_plan(h, 2 * 64).row;
    return MEV_OK;
}

// mev_rollout_policy: T sub-steps of policy + fused step in one launch (k_rollout), along step_window's path.
// value_seq (mev_rollout_policy_values, checked there): non-null runs k_rollout's value instantiation.
// rep (mev_rollout_policy_repeat, checked there; null: the two calls above): T decisions of up to rep->repeat
// sub-steps each -- spawn_route staged as [T * n][E], the Philox counter advanced by T * n, spawn_prob once from
// dt as mev_step_repeat computes it -- through k_rollout's REPEAT instantiations.
// multi (mev_rollout_policies, checked there; a, value_seq and rep are its base's): the policy of a->policy gives
// way to multi's table, one entry per agent slot by `assign` (staged like every array) with its own sigma row --
// through k_rollout's MULTI instantiations, the scratch sized by the widest listed policy.
static int rollout(mev_handle* h, const mev_rollout_args* a, float* value_seq, const mev_rollout_repeat_args* rep = nullptr,
                   const mev_rollout_multi_args* multi = nullptr) {
    const mev_policy* pol = a->policy;
    int hidden = 0;  // the hidden widths summed: the LDS scratch
    auto hidden_of = [](const mev_policy* p) { return p->net.out[0] + (p->net.layers == 3 ? p->net.out[1] : 0); };
    if (multi) {
        for (int p = 0; p < multi->count; ++p) {
            const mev_policy* q = multi->policies[p];
            const std::string at = "mev_rollout_policies: policies[" + std::to_string(p) + "]";
            if (!q) return fail(MEV_E_INVALID, at + " is null");
            if (q->h != h) return fail(MEV_E_INVALID, at + " belongs to another handle");
            if (q->net.in[0] != h->D) return fail(MEV_E_INVALID, at + ": in_dim != obs_dim");
            if (value_seq && !q->has_value)
                return fail(MEV_E_INVALID, at + " has no value head (mev_policy_set_value_head)");
            for (int k = 0; k < 2; ++k)
                if (multi->sigma && !std::isfinite(multi->sigma[2 * p + k]))
                    return fail(MEV_E_INVALID, "mev_rollout_policies: sigma must be finite");
            hidden = std::max(hidden, hidden_of(q));
        }
    } else {
        if (!pol) return fail(MEV_E_INVALID, "mev_rollout_policy: policy required");
        if (pol->h != h) return fail(MEV_E_INVALID, "mev_rollout_policy: the policy belongs to another handle");
        if (pol->net.in[0] != h->D) return fail(MEV_E_INVALID, "mev_rollout_policy: policy in_dim != obs_dim");
        hidden = hidden_of(pol);
    }
    if (a->length < 1 || a->length > MEV_MAX_ROLLOUT)
        return fail(MEV_E_INVALID, "length must be in 1.." + std::to_string(MEV_MAX_ROLLOUT));
    if (a->flags & MEV_GATHER_TO_ROOT) return fail(MEV_E_INVALID, "mev_rollout_policy does not gather (MEV_GATHER_TO_ROOT)");
    if (a->flags & ~(MEV_DEVICE_PTRS | MEV_AUTO_RESET)) return fail(MEV_E_INVALID, "mev_rollout_policy: unknown flag");
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(a->lo[k]) || !std::isfinite(a->hi[k]) || a->lo[k] > a->hi[k])
            return fail(MEV_E_INVALID, "mev_rollout_policy: lo / hi must be finite with lo <= hi");
        if (a->sigma && !std::isfinite(a->sigma[k])) return fail(MEV_E_INVALID, "mev_rollout_policy: sigma must be finite");
    }
    const mev::RolloutPlan rp = rollout_plan(h, hidden);
    if (rp.row < 0)
        return fail(MEV_E_INVALID, "mev_rollout_policy: unsupported shape (the fused step kernel must hold the env, and obs_dim <= 31 + " +
                                       std::to_string(MEV_POLICY_MAX_WIDTH) + ")");
    const bool dev = (a->flags & MEV_DEVICE_PTRS) != 0;
    const size_t E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents), D = size_t(h->D);
    if (multi && !dev)  // (device pointers: the kernel reads an entry >= count as count - 1)
        for (size_t g = 0; g < EN; ++g)
            if (multi->assign[g] >= multi->count)
                return fail(MEV_E_RANGE, "assign[" + std::to_string(g) + "] = " + std::to_string(multi->assign[g]) +
                                             " is outside [0, " + std::to_string(multi->count) + ")");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    if (h->last.lidar_u8 || !h->last.obs)  // a compact gather row: obs_0 decoded into the handle's buffers
        if (int r = sync_internal(h)) return r;
    if (!h->sp_valid || memcmp(&h->sp, &h->sp_dev, sizeof(mev::SimParams)) != 0) {  // (as mev_step)
        HIP_TRY(hipMemcpyAsync(h->d_sp, &h->sp, sizeof(mev::SimParams), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        memcpy(&h->sp_dev, &h->sp, sizeof(mev::SimParams));
        h->sp_valid = true;
    }
    const int T = a->length;
    const size_t n = rep ? size_t(rep->repeat) : 1;  // sub-steps per row
    mev::RolloutMultiArgs ra{};  // (the calls without `multi` launch with its bases: what they passed before)
    ra.repeat = int32_t(n);
    ra.in.dt = a->dt;
    ra.in.spawn_prob = spawn_prob(h, a->dt);
    ra.in.auto_reset = (a->flags & MEV_AUTO_RESET) ? 1 : 0;
    ra.in.rng_counter = h->rng_counter;  // sub-step t: + t (k_rollout; REPEAT: sub-step s of decision t + t n + s)
    if (multi) {
        ra.P = multi->count;
        for (int p = 0; p < multi->count; ++p) {
            ra.nets[p] = multi->policies[p]->net;
            for (int k = 0; k < 2; ++k) ra.sigmas[p][k] = multi->sigma ? multi->sigma[2 * p + k] : 0.0f;
        }
    } else {
        ra.net = pol->net;
    }
    ra.T = T;
    ra.pol_off = rp.pol_off;
    ra.obs0 = h->last.obs;
    ra.act_scratch = h->d_actions;
    ra.noisy = (multi ? multi->sigma : a->sigma) ? 1 : 0;
    for (int k = 0; k < 2; ++k) {
        ra.sigma[k] = a->sigma ? a->sigma[k] : 0.0f;
        ra.lo[k] = a->lo[k];
        ra.hi[k] = a->hi[k];
    }
    ra.seed_lo = uint32_t(a->noise_seed);
    ra.seed_hi = uint32_t(a->noise_seed >> 32);
    ra.ctr_lo = uint32_t(a->noise_counter);
    ra.ctr_hi = uint32_t(a->noise_counter >> 32);
    Stage st(h, dev);
    st.in(&ra.in.spawn_route, a->spawn_route, size_t(T) * n * E);
    st.in(&ra.assign, multi ? multi->assign : nullptr, EN);
    st.out(&ra.obs_seq, a->obs_seq, size_t(T) * EN * D);
    st.out(&ra.actions_seq, a->actions_seq, size_t(T) * EN * 2);
    st.out(&ra.mean_seq, a->mean_seq, size_t(T) * EN * 2);
    st.out(&ra.reward_seq, a->reward_seq, size_t(T) * EN);
    st.out(&ra.done_seq, a->done_seq, size_t(T) * EN);
    st.out(&ra.status_seq, a->status_seq, size_t(T) * EN);
    st.out(&ra.term_seq, a->terminated_seq, size_t(T) * E);
    st.out(&ra.trunc_seq, a->truncated_seq, size_t(T) * E);
    st.out(&ra.value_seq, value_seq, size_t(T + 1) * EN);
    st.out(&ra.substeps_seq, rep ? rep->substeps_seq : nullptr, size_t(T) * E);
    if (int r = st.upload()) return r;
    h->rng_counter += uint64_t(T) * uint64_t(n);
    h->deal_valid = false;  // NPC counts change outside the dealt step: the deal restarts
    if (multi) HIP_TRY(mev::launch_rollout_multi(h->sp, h->d_sp, rp, ra, h->internal, h->stream));
    else if (rep) HIP_TRY(mev::launch_rollout_repeat(h->sp, h->d_sp, rp, ra, h->internal, h->stream));
    else HIP_TRY(mev::launch_rollout(h->sp, h->d_sp, rp, ra, h->internal, h->stream));
    // the last outputs: row T - 1.  Device pointers: tracked where the caller's arrays hold them, as after
    // mev_step.  Host pointers: the rows live in the staging block, so they are copied into the handle's buffers.
    const size_t t1 = size_t(T - 1);
    mev::Outputs last = h->internal;
    auto keep = [&](auto** slot, auto* seq, size_t per) -> hipError_t {
        if (!seq) return hipSuccess;
        if (dev) {
            *slot = seq + t1 * per;
            return hipSuccess;
        }
        return hipMemcpyAsync(*slot, seq + t1 * per, per * sizeof(**slot), hipMemcpyDeviceToDevice, h->stream);
    };
    HIP_TRY(keep(&last.obs, ra.obs_seq, EN * D));
    HIP_TRY(keep(&last.rew, ra.reward_seq, EN));
    HIP_TRY(keep(&last.done, ra.done_seq, EN));
    HIP_TRY(keep(&last.status, ra.status_seq, EN));
    HIP_TRY(keep(&last.term, ra.term_seq, E));
    HIP_TRY(keep(&last.trunc, ra.trunc_seq, E));
    h->last = last;
    return st.download();
}

int mev_rollout_policy(mev_handle* h, const mev_rollout_args* a) {
    if (!h || !a) return fail(MEV_E_INVALID, "null argument");
    return rollout(h, a, nullptr);
}

int mev_rollout_policy_values(mev_handle* h, const mev_rollout_values_args* va) {
    if (!h || !va) return fail(MEV_E_INVALID, "null argument");
    if (!va->value_seq) return fail(MEV_E_INVALID, "mev_rollout_policy_values: value_seq required");
    if (va->rollout.policy && !va->rollout.policy->has_value)
        return fail(MEV_E_INVALID, "mev_rollout_policy_values: the policy has no value head (mev_policy_set_value_head)");
    return rollout(h, &va->rollout, va->value_seq);
}

int mev_rollout_policy_repeat(mev_handle* h, const mev_rollout_repeat_args* ra) {
    if (!h || !ra) return fail(MEV_E_INVALID, "null argument");
    if (ra->repeat < 1 || ra->repeat > MEV_MAX_REPEAT)
        return fail(MEV_E_INVALID, "repeat must be in 1.." + std::to_string(MEV_MAX_REPEAT));
    if (int64_t(ra->rollout.length) * int64_t(ra->repeat) > MEV_MAX_ROLLOUT_SUBSTEPS)
        return fail(MEV_E_INVALID, "length * repeat must be at most " + std::to_string(MEV_MAX_ROLLOUT_SUBSTEPS));
    if (ra->value_seq && ra->rollout.policy && !ra->rollout.policy->has_value)
        return fail(MEV_E_INVALID, "mev_rollout_policy_repeat: the policy has no value head (mev_policy_set_value_head)");
    return rollout(h, &ra->rollout, ra->value_seq, ra);
}

// mev_rollout_policies: mev_rollout_policy_repeat with a policy per agent slot (rollout()'s `multi`)
int mev_rollout_policies(mev_handle* h, const mev_rollout_multi_args* ma) {
    static_assert(mev::kMaxRolloutPolicies == MEV_MAX_ROLLOUT_POLICIES, "the kernel's by-value policy table");
    if (!h || !ma) return fail(MEV_E_INVALID, "null argument");
    const mev_rollout_repeat_args* ra = &ma->base;
    if (ra->rollout.policy || ra->rollout.sigma)
        return fail(MEV_E_INVALID, "mev_rollout_policies: base.rollout.policy and base.rollout.sigma must be NULL");
    if (!ma->policies || !ma->assign) return fail(MEV_E_INVALID, "mev_rollout_policies: policies and assign required");
    if (ma->count < 1 || ma->count > MEV_MAX_ROLLOUT_POLICIES)
        return fail(MEV_E_INVALID, "count must be in 1.." + std::to_string(MEV_MAX_ROLLOUT_POLICIES));
    if (ra->repeat < 1 || ra->repeat > MEV_MAX_REPEAT)
        return fail(MEV_E_INVALID, "repeat must be in 1.." + std::to_string(MEV_MAX_REPEAT));
    if (int64_t(ra->rollout.length) * int64_t(ra->repeat) > MEV_MAX_ROLLOUT_SUBSTEPS)
        return fail(MEV_E_INVALID, "length * repeat must be at most " + std::to_string(MEV_MAX_ROLLOUT_SUBSTEPS));
    return rollout(h, &ra->rollout, ra->value_seq, ra, ma);
}

// mev_gae (include/marlenv.h): k_gae's reverse scan.  Reads and writes its arguments only; host pointers go
// through the handle's staging block.
int mev_gae(mev_handle* h, const mev_gae_args* ga) {
    if (!h || !ga) return fail(MEV_E_INVALID, "null argument");
    if (!ga->reward_seq || !ga->value_seq) return fail(MEV_E_INVALID, "mev_gae: reward_seq and value_seq required");
    if (!ga->advantages && !ga->returns && !ga->valid) return fail(MEV_E_INVALID, "mev_gae needs at least one output");
    if (ga->length < 1 || ga->length > MEV_MAX_ROLLOUT)
        return fail(MEV_E_INVALID, "length must be in 1.." + std::to_string(MEV_MAX_ROLLOUT));
    if (!std::isfinite(ga->gamma) || !std::isfinite(ga->lambda)) return fail(MEV_E_INVALID, "mev_gae: gamma and lambda must be finite");
    if (ga->flags & ~uint32_t(MEV_DEVICE_PTRS | MEV_GAE_MASK_RESET_STEPS)) return fail(MEV_E_INVALID, "mev_gae: unknown flag");
    const bool dev = (ga->flags & MEV_DEVICE_PTRS) != 0;
    const size_t T = size_t(ga->length), E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents);
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    mev::GaeArgs g{};
    g.T = ga->length; g.E = h->cfg.num_envs; g.N = h->cfg.num_agents;
    g.mask = (ga->flags & MEV_GAE_MASK_RESET_STEPS) ? 1 : 0;
    g.gamma = ga->gamma;
    const float c = ga->gamma * ga->lambda;  // (one f32 product)
    g.c = c;
    Stage st(h, dev);
    st.in(&g.reward, ga->reward_seq, T * EN);
    st.in(&g.value, ga->value_seq, (T + 1) * EN);
    st.in(&g.done, ga->done_seq, T * EN);
    st.in(&g.term, ga->terminated_seq, T * E);
    st.in(&g.trunc, ga->truncated_seq, T * E);
    st.in(&g.ended_before, g.mask ? ga->ended_before : nullptr, E);
    st.out(&g.adv, ga->advantages, T * EN);
    st.out(&g.ret, ga->returns, T * EN);
    st.out(&g.valid, ga->valid, T * EN);
    if (int r = st.upload()) return r;
    HIP_TRY(mev::launch_gae(g, h->stream));
    return st.download();
}

// mev_evaluate_plans (include/marlenv.h): the plan rollout's loop over C candidates that start from
// copies of live envs, nothing of the handle written.
// leaf_obs: mev_evaluate_leaves' [C][N][obs_dim] rows (null: mev_evaluate_plans).  The candidates'
// LiDAR hand-off lives in a per-handle scratch that only grows, to kLeafHandCap at the most: a call
// with more candidates than the cap holds (or than MEV_LEAF_CHUNK) goes through in chunks.
constexpr size_t kLeafHandCap = size_t(64) << 20;
// xp: mev_expand_plans' additions (null: the two evaluation calls) -- the candidates' roots are slots
// of xp->src when that is set, and their stop states go to slots xp->dst_slots of xp->dst.
// sm: mev_sample_plans' additions (null: the other calls) -- no actions array: the candidates draw
// their rows from sm->mean / sm->sigma, roots is [groups], and the rows go to sm->actions_out.
// Both (mev_sample_expand_plans): the [groups] roots are slots of xp->src when that is set.
static int evaluate(mev_handle* h, const mev_evaluate_args* ea, float* leaf_obs, const mev_expand_args* xp = nullptr,
                    const mev_sample_args* sm = nullptr) {
    const bool leaves = leaf_obs != nullptr;
    const char* fn = sm && xp ? "mev_sample_expand_plans" : sm ? "mev_sample_plans" : xp ? "mev_expand_plans"
                     : leaves ? "mev_evaluate_leaves" : "mev_evaluate_plans";
    if (xp) {
        if (!xp->dst || !xp->dst_slots) return fail(MEV_E_INVALID, "dst and dst_slots required");
        if (xp->dst->h != h || (xp->src && xp->src->h != h)) return fail(MEV_E_INVALID, "the pool belongs to another handle");
    }
    if (sm) {
        if (ea->actions) return fail(MEV_E_INVALID, std::string(fn) + " draws the actions: eval.actions must be NULL");
        if (!ea->roots || !sm->mean || !sm->sigma) return fail(MEV_E_INVALID, "roots, mean and sigma required");
        if (sm->groups < 1 || sm->samples < 1 || int64_t(sm->groups) * sm->samples != int64_t(ea->candidates))
            return fail(MEV_E_INVALID, "candidates must equal groups * samples (each at least 1)");
        for (int k = 0; k < 2; ++k)
            if (!std::isfinite(sm->lo[k]) || !std::isfinite(sm->hi[k]) || sm->lo[k] > sm->hi[k])
                return fail(MEV_E_INVALID, "lo and hi must be finite with lo[k] <= hi[k]");
        if (sm->sample_flags & ~uint32_t(MEV_SAMPLE_MEAN_FIRST))
            return fail(MEV_E_INVALID, "sample_flags takes MEV_SAMPLE_MEAN_FIRST only");
    } else if (!ea->actions || !ea->roots) {
        return fail(MEV_E_INVALID, "actions and roots required");
    }
    if (ea->candidates < 1 || ea->candidates > MEV_MAX_CANDIDATES)
        return fail(MEV_E_INVALID, "candidates must be in 1.." + std::to_string(MEV_MAX_CANDIDATES));
    if (ea->length < 1 || ea->length > MEV_MAX_REPEAT)
        return fail(MEV_E_INVALID, "length must be in 1.." + std::to_string(MEV_MAX_REPEAT));
    if (ea->flags & ~uint32_t(MEV_DEVICE_PTRS)) return fail(MEV_E_INVALID, std::string(fn) + " takes MEV_DEVICE_PTRS only");
    if (!xp && !leaves && !(sm && sm->actions_out) && !ea->returns && !ea->reward_seq && !ea->done_seq &&
        !ea->status_seq && !ea->substeps && !ea->terminated && !ea->truncated)
        return fail(MEV_E_INVALID, std::string(fn) + " needs at least one output");
    const bool dev = (ea->flags & MEV_DEVICE_PTRS) != 0;
    const size_t C = size_t(ea->candidates), T = size_t(ea->length), N = size_t(h->cfg.num_agents), CN = C * N;
    const int32_t n_roots = xp && xp->src ? xp->src->slots : h->cfg.num_envs;  // where a root may point
    const size_t R = sm ? size_t(sm->groups) : C;                              // entries of roots
    if (!dev)
        for (size_t c = 0; c < R; ++c)
            if (ea->roots[c] < 0 || ea->roots[c] >= n_roots)
                return fail(MEV_E_RANGE, "roots[" + std::to_string(c) + "] = " + std::to_string(ea->roots[c]) +
                                             " is outside [0, " + std::to_string(n_roots) + ")");
    if (xp && !dev) {
        // the slots that receive a state: in range, none twice, and in the roots' own pool none a root
        // (bitmaps over the pool's slots)
        const size_t S = size_t(xp->dst->slots);
        std::vector<bool> taken(S, false);
        for (size_t c = 0; c < C; ++c) {
            const int32_t d = xp->dst_slots[c];
            if (d < -1 || d >= xp->dst->slots)
                return fail(MEV_E_RANGE, "dst_slots[" + std::to_string(c) + "] = " + std::to_string(d) +
                                             " is outside [-1, " + std::to_string(S) + ")");
            if (d < 0) continue;
            if (taken[size_t(d)]) return fail(MEV_E_INVALID, "dst_slots names slot " + std::to_string(d) + " twice");
            taken[size_t(d)] = true;
        }
        if (xp->src == xp->dst)
            for (size_t c = 0; c < R; ++c)
                if (taken[size_t(ea->roots[c])])
                    return fail(MEV_E_INVALID, "slot " + std::to_string(ea->roots[c]) + " is a root and in dst_slots");
    }
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    if (xp && xp->src && !dev) {  // a root slot nothing was stored in: as a root out of range
        std::vector<uint8_t> valid(size_t(xp->src->slots));
        HIP_TRY(hipMemcpyAsync(valid.data(), xp->src->st.valid, valid.size(), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (size_t c = 0; c < R; ++c)
            if (!valid[size_t(ea->roots[c])])
                return fail(MEV_E_RANGE, "roots[" + std::to_string(c) + "] = " + std::to_string(ea->roots[c]) +
                                             ": nothing valid is stored in that slot");
    }
    mev::SeqRows rows{};
    for (size_t s = 0; s < T; ++s) {  // read from the caller's memory now; by value with the kernel's arguments
        rows.dt[s] = ea->dt_seq ? ea->dt_seq[s] : ea->dt;
        rows.spawn_prob[s] = spawn_prob(h, rows.dt[s]);
    }
    mev::StepInputs in{};
    in.dt = rows.dt[0];
    in.spawn_prob = rows.spawn_prob[0];
    in.rng_counter = h->rng_counter + (xp ? xp->counter_offset : 0);  // sub-step s: + s; the handle's counter stays
    mev::EvalOutputs eo{};
    eo.gamma = ea->gamma;
    const int32_t *d_roots = nullptr, *d_dst = nullptr;
    float* d_leaf_obs = nullptr;
    int chunk = 0;
    if (leaves) {
        // candidates per chunk: what the capped scratch holds (at least one), or MEV_LEAF_CHUNK
        const size_t per = mev::leaf_hand_bytes(h->sp, 1024) / 1024 + 1;
        size_t fit = kLeafHandCap / per;
        if (fit < 1) fit = 1;
        chunk = int(h->leaf_chunk ? size_t(h->leaf_chunk) : fit);
        if (size_t(chunk) > C) chunk = int(C);
        if (int r = grow_block(h, &h->d_leaf, &h->leaf_cap, mev::leaf_hand_bytes(h->sp, chunk))) return r;
    }
    mev::SampleIn si{};  // (sm) the device view of the sampling arguments
    Stage st(h, dev);
    if (sm) {
        si = mev::SampleIn{nullptr, nullptr, nullptr, {sm->lo[0], sm->lo[1]}, {sm->hi[0], sm->hi[1]},
                           sm->groups, sm->samples, uint32_t(sm->noise_seed), uint32_t(sm->noise_seed >> 32),
                           uint32_t(sm->noise_counter), uint32_t(sm->noise_counter >> 32),
                           (sm->sample_flags & MEV_SAMPLE_MEAN_FIRST) ? 1u : 0u};
        st.in(&si.mean, sm->mean, T * R * N * 2);
        st.in(&si.sigma, sm->sigma, T * R * N * 2);
        st.out(&si.actions_out, sm->actions_out, T * CN * 2);
    } else {
        st.in(&in.actions, ea->actions, T * CN * 2);
    }
    st.in(&d_roots, ea->roots, R);
    st.in(&in.spawn_route, ea->spawn_route, T * C);
    st.out(&eo.returns, ea->returns, CN);
    st.out(&rows.reward, ea->reward_seq, T * CN);
    st.out(&rows.done, ea->done_seq, T * CN);
    st.out(&rows.status, ea->status_seq, T * CN);
    st.out(&eo.substeps, ea->substeps, C);
    st.out(&eo.terminated, ea->terminated, C);
    st.out(&eo.truncated, ea->truncated, C);
    st.out(&d_leaf_obs, leaf_obs, CN * size_t(h->sp.D));
    if (xp) st.in(&d_dst, xp->dst_slots, C);
    if (int r = st.upload()) return r;
    const mev::PlanCall call{int(C), int(T), d_roots, &rows, eo, d_leaf_obs, h->d_leaf, chunk,
                             xp && xp->src ? &xp->src->st : nullptr, xp ? &xp->dst->st : nullptr, d_dst,
                             sm ? &si : nullptr};
    HIP_TRY(mev::launch_plans(h->sp, in, call, h->stream));
    return st.download();
}

int mev_evaluate_plans(mev_handle* h, const mev_evaluate_args* ea) {
    if (!h || !ea) return fail(MEV_E_INVALID, "null argument");
    return evaluate(h, ea, nullptr);
}

// mev_evaluate_leaves (include/marlenv.h): mev_evaluate_plans, and the observation of the state every
// candidate stopped at: the car kernel's LEAF mode, then k_lidar over the candidates' hand-off.
int mev_evaluate_leaves(mev_handle* h, const mev_leaf_args* la) {
    if (!h || !la) return fail(MEV_E_INVALID, "null argument");
    if (!la->leaf_obs) return fail(MEV_E_INVALID, "leaf_obs required");
    return evaluate(h, &la->eval, la->leaf_obs);
}

// ---- state pools (include/marlenv.h): env states outside the live batch, in the handle's own SoA
// layout over slots (mev::PoolState), and mev_expand_plans, the plan evaluation that reads and
// fills them.
namespace {
// one device block of `slots` states for h's shape, every array at a 256-byte boundary, all zero
// (the valid bytes with it); *block is the allocation
hipError_t pool_alloc(const mev_handle* h, int32_t slots, uint8_t** block, mev::PoolState* st) {
    const size_t S = size_t(slots), SN = S * size_t(h->cfg.num_agents), SK = S * size_t(h->cfg.max_npcs);
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t es = al(SN * 4) / 4, ns = al(SK * 4) / 4;  // the field strides, in elements
    size_t off = 0;
    auto take = [&off, &al](size_t bytes) {
        const size_t at = off;
        off += al(bytes ? bytes : 1);
        return at;
    };
    const size_t o_ego = take(es * 4 * mev::EF_COUNT), o_npc = take(ns * 4 * mev::NF_COUNT);
    const size_t o_ed = take(SN * 8), o_nd = take(SK * 8), o_nc = take(S * 4), o_sc = take(S * 4);
    const size_t o_ea = take(SN), o_na = take(SK), o_v = take(S);
    uint8_t* b = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&b), off);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(b, 0, off, h->stream);
    if (e != hipSuccess) {
        (void)hipFree(b);
        return e;
    }
    *block = b;
    *st = mev::PoolState{reinterpret_cast<float*>(b + o_ego), int64_t(es), reinterpret_cast<float*>(b + o_npc),
                         int64_t(ns), b + o_ea, b + o_na, reinterpret_cast<int32_t*>(b + o_nc),
                         reinterpret_cast<int32_t*>(b + o_sc), reinterpret_cast<float*>(b + o_ed),
                         reinterpret_cast<float*>(b + o_nd), b + o_v, slots};
    return hipSuccess;
}
}  // namespace

int mev_pool_create(mev_handle* h, int32_t slots, mev_pool** out) {
    if (!h || !out) return fail(MEV_E_INVALID, "null argument");
    *out = nullptr;
    if (slots < 1 || slots > MEV_MAX_POOL_SLOTS)
        return fail(MEV_E_INVALID, "slots must be in 1.." + std::to_string(MEV_MAX_POOL_SLOTS));
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    mev_pool* q = new mev_pool;
    q->h = h;
    q->slots = slots;
    const hipError_t err = pool_alloc(h, slots, &q->block, &q->st);
    if (err != hipSuccess) {
        delete q;
        (void)hipGetLastError();
        return fail(MEV_E_NOMEM, std::string("device allocation failed: ") + hipGetErrorString(err));
    }
    h->pools.push_back(q);
    *out = q;
    return MEV_OK;
}

int mev_pool_destroy(mev_pool* pool) {
    if (!pool) return MEV_OK;
    mev_handle* h = pool->h;
    (void)hipSetDevice(h->cfg.device);
    (void)serve_stop(h);
    (void)hipStreamSynchronize(h->stream);  // (calls in flight may still read or fill it)
    for (size_t i = 0; i < h->pools.size(); ++i)
        if (h->pools[i] == pool) {
            h->pools.erase(h->pools.begin() + long(i));
            break;
        }
    if (pool->block) (void)hipFree(pool->block);
    delete pool;
    return MEV_OK;
}

int mev_pool_slots(const mev_pool* pool, int32_t* slots) {
    if (!pool || !slots) return fail(MEV_E_INVALID, "null argument");
    *slots = pool->slots;
    return MEV_OK;
}

int mev_pool_capture(mev_handle* h, mev_pool* pool, const int32_t* envs, const int32_t* slots, int32_t count,
                     uint32_t flags) {
    if (!h || !pool || !envs || !slots) return fail(MEV_E_INVALID, "null argument");
    if (pool->h != h) return fail(MEV_E_INVALID, "the pool belongs to another handle");
    if (count < 1 || count > MEV_MAX_POOL_SLOTS)
        return fail(MEV_E_INVALID, "count must be in 1.." + std::to_string(MEV_MAX_POOL_SLOTS));
    if (flags & ~uint32_t(MEV_DEVICE_PTRS)) return fail(MEV_E_INVALID, "mev_pool_capture takes MEV_DEVICE_PTRS only");
    const bool dev = (flags & MEV_DEVICE_PTRS) != 0;
    if (!dev)
        for (int32_t i = 0; i < count; ++i) {
            if (envs[i] < 0 || envs[i] >= h->cfg.num_envs)
                return fail(MEV_E_RANGE, "envs[" + std::to_string(i) + "] = " + std::to_string(envs[i]) + " is outside [0, " +
                                             std::to_string(h->cfg.num_envs) + ")");
            if (slots[i] < 0 || slots[i] >= pool->slots)
                return fail(MEV_E_RANGE, "slots[" + std::to_string(i) + "] = " + std::to_string(slots[i]) + " is outside [0, " +
                                             std::to_string(pool->slots) + ")");
        }
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    const int32_t *d_envs = nullptr, *d_slots = nullptr;
    Stage st(h, dev);
    st.in(&d_envs, envs, size_t(count));
    st.in(&d_slots, slots, size_t(count));
    if (int r = st.upload()) return r;
    HIP_TRY(mev::launch_pool_copy(h->sp, mev::pool_of_live(h->sp), pool->st, d_envs, d_slots, count, h->stream));
    return st.download();
}

int mev_pool_get_state(mev_pool* pool, const int32_t* slots, int32_t count, const mev_state* s, float* ego_dims,
                       float* npc_dims, uint8_t* valid) {
    if (!pool || !slots || !s) return fail(MEV_E_INVALID, "null argument");
    if (count < 1 || count > MEV_MAX_POOL_SLOTS)
        return fail(MEV_E_INVALID, "count must be in 1.." + std::to_string(MEV_MAX_POOL_SLOTS));
    for (int32_t i = 0; i < count; ++i)
        if (slots[i] < 0 || slots[i] >= pool->slots)
            return fail(MEV_E_RANGE, "slots[" + std::to_string(i) + "] = " + std::to_string(slots[i]) + " is outside [0, " +
                                         std::to_string(pool->slots) + ")");
    mev_handle* h = pool->h;
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    // the asked slots gathered into a pool of `count` slots, row i = slot slots[i], then read field by field
    const int32_t* d_slots = nullptr;
    Stage st(h, false);
    st.in(&d_slots, slots, size_t(count));
    if (int r = st.upload()) return r;
    uint8_t* block = nullptr;
    mev::PoolState g{};
    const hipError_t err = pool_alloc(h, count, &block, &g);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return fail(MEV_E_NOMEM, std::string("device allocation failed: ") + hipGetErrorString(err));
    }
    const size_t S = size_t(count), SN = S * size_t(h->cfg.num_agents), SK = S * size_t(h->cfg.max_npcs);
    const hipError_t e = mev::launch_pool_copy(h->sp, pool->st, g, d_slots, nullptr, count, h->stream);
    void* const ego4[mev::EF_COUNT] = {s->x, s->y, s->v, s->heading, s->acc, s->steering, s->prev_dist,
                                      s->prev_a0, s->prev_a1, s->spawn_x, s->spawn_y, s->spawn_v,
                                      s->spawn_heading, s->path_index, s->route, s->intention};
    void* const npc4[mev::NF_COUNT] = {s->npc_x, s->npc_y, s->npc_v, s->npc_heading, s->npc_acc,
                                      s->npc_steering, s->npc_path_index, s->npc_route, s->npc_intention};
    for (int k = 0; k < mev::EF_COUNT; ++k) st.fetch(ego4[k], g.ego + g.ego_stride * k, SN * 4);
    for (int k = 0; k < mev::NF_COUNT; ++k) st.fetch(npc4[k], g.npc + g.npc_stride * k, SK * 4);
    st.fetch(s->alive, g.ego_alive, SN);
    st.fetch(s->npc_alive, g.npc_alive, SK);
    st.fetch(s->npc_count, g.npc_count, S * 4);
    st.fetch(s->step_count, g.step_count, S * 4);
    st.fetch(ego_dims, g.ego_dim, SN * 8);
    st.fetch(npc_dims, g.npc_dim, SK * 8);
    st.fetch(valid, g.valid, S);
    const int r = e == hipSuccess ? st.download() : fail(MEV_E_HIP, std::string("mev_pool_get_state: ") + hipGetErrorString(e));
    if (r) (void)hipStreamSynchronize(h->stream);  // (the gather may still be writing the block)
    (void)hipFree(block);
    return r;
}

int mev_expand_plans(mev_handle* h, const mev_expand_args* xa) {
    if (!h || !xa) return fail(MEV_E_INVALID, "null argument");
    return evaluate(h, &xa->eval, xa->leaf_obs, xa);
}

// mev_sample_plans (include/marlenv.h): the evaluation calls with the actions drawn by the
// candidates' own waves (the car kernel's SAMPLE mode).
int mev_sample_plans(mev_handle* h, const mev_sample_args* sa) {
    if (!h || !sa) return fail(MEV_E_INVALID, "null argument");
    return evaluate(h, &sa->eval, sa->leaf_obs, nullptr, sa);
}

// mev_sample_expand_plans (include/marlenv.h): mev_sample_plans whose groups may start from slots of a
// pool and whose candidates' stop states are kept in one (the car kernel's KEEP and SAMPLE modes at
// once): the sampled call's arguments, and the expansion's over them.
int mev_sample_expand_plans(mev_handle* h, const mev_sample_expand_args* xa) {
    if (!h || !xa) return fail(MEV_E_INVALID, "null argument");
    const mev_expand_args xp{xa->sample.eval, xa->sample.leaf_obs, xa->src, xa->dst, xa->dst_slots, xa->counter_offset};
    return evaluate(h, &xa->sample.eval, xa->sample.leaf_obs, &xp, &xa->sample);
}

// mev_update_plans (include/marlenv.h): the reduction over each group's candidates, k_update_plans.
// Reads and writes its arguments only; host pointers go through the handle's staging block.
int mev_update_plans(mev_handle* h, const mev_update_args* ua) {
    if (!h || !ua) return fail(MEV_E_INVALID, "null argument");
    if (!ua->actions || (!ua->scores && !ua->returns)) return fail(MEV_E_INVALID, "actions and scores or returns required");
    if (ua->groups < 1 || ua->samples < 1 || ua->samples > MEV_MAX_SAMPLES ||
        int64_t(ua->groups) * ua->samples > MEV_MAX_CANDIDATES)
        return fail(MEV_E_INVALID, "groups >= 1, samples in 1.." + std::to_string(MEV_MAX_SAMPLES) +
                                       ", groups * samples <= " + std::to_string(MEV_MAX_CANDIDATES));
    if (ua->length < 1 || ua->length > MEV_MAX_REPEAT)
        return fail(MEV_E_INVALID, "length must be in 1.." + std::to_string(MEV_MAX_REPEAT));
    if (ua->flags & ~uint32_t(MEV_DEVICE_PTRS)) return fail(MEV_E_INVALID, "mev_update_plans takes MEV_DEVICE_PTRS only");
    const bool elites = ua->mode == MEV_UPDATE_ELITES;
    if (!elites && ua->mode != MEV_UPDATE_SOFTMAX) return fail(MEV_E_INVALID, "mode must be MEV_UPDATE_ELITES or MEV_UPDATE_SOFTMAX");
    if (elites && (ua->elites < 1 || ua->elites > ua->samples)) return fail(MEV_E_INVALID, "elites must be in 1..samples");
    if (!elites && !(std::isfinite(ua->inv_temperature) && ua->inv_temperature >= 0.0f))
        return fail(MEV_E_INVALID, "inv_temperature must be finite and >= 0");
    if (std::isnan(ua->sigma_min)) return fail(MEV_E_INVALID, "sigma_min must not be NaN");
    if (!ua->new_mean && !ua->new_sigma && !ua->best && !ua->best_score && !(elites && ua->order) && !(!elites && ua->weights))
        return fail(MEV_E_INVALID, "mev_update_plans needs at least one output");
    const bool dev = (ua->flags & MEV_DEVICE_PTRS) != 0;
    const size_t G = size_t(ua->groups), K = size_t(ua->samples), C = G * K, T = size_t(ua->length);
    const size_t N = size_t(h->cfg.num_agents), M = size_t(elites ? ua->elites : 0);
    if (!dev)  // a non-finite score is refused here; with device pointers it ranks last
        for (size_t c = 0; c < C; ++c) {
            float sc = 0.0f;
            if (ua->scores) sc = ua->scores[c];
            else
                for (size_t i = 0; i < N; ++i) sc = sc + ua->returns[c * N + i];
            if (!std::isfinite(sc)) return fail(MEV_E_INVALID, "the score of candidate " + std::to_string(c) + " is not finite");
        }
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r = serve_stop(h)) return r;  // (the server holds the stream)
    mev::UpdateArgs u{};
    u.groups = ua->groups; u.samples = ua->samples; u.n = ua->length; u.N = int32_t(N);
    u.mode = ua->mode; u.elites = ua->elites; u.inv_temperature = ua->inv_temperature; u.sigma_min = ua->sigma_min;
    Stage st(h, dev);
    st.in(&u.actions, ua->actions, T * C * N * 2);
    st.in(&u.scores, ua->scores, C);
    st.in(&u.returns, ua->scores ? nullptr : ua->returns, C * N);  // (read when there are no scores)
    st.out(&u.new_mean, ua->new_mean, T * G * N * 2);
    st.out(&u.new_sigma, ua->new_sigma, T * G * N * 2);
    st.out(&u.best, ua->best, G);
    st.out(&u.best_score, ua->best_score, G);
    st.out(&u.order, elites ? ua->order : nullptr, G * M);
    st.out(&u.weights, elites ? nullptr : ua->weights, C);
    if (int r = st.upload()) return r;
    HIP_TRY(mev::launch_update_plans(u, h->stream));
    return st.download();
}

static int sync_internal(mev_handle* h);  // below, with mev_device_outputs

int mev_get_outputs(mev_handle* h, float* obs, float* rew, uint8_t* done, uint8_t* status, uint8_t* term,
                    uint8_t* trunc, int32_t* alive, int32_t* step, uint32_t flags) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const bool dev = (flags & MEV_DEVICE_PTRS) != 0;
    if (h->last.lidar_u8) {  // compact gather row: decoded into the handle's buffers first
        if (int r0 = sync_internal(h)) return r0;
    }
    mev_step_args a{};
    a.obs = obs; a.reward = rew; a.done = done; a.status = status;
    a.terminated = term; a.truncated = trunc; a.agents_alive = alive; a.step = step;
    int r = copy_out(h, h->last, a, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    if (r) return r;
    if (!dev) HIP_TRY(hipStreamSynchronize(h->stream));
    return MEV_OK;
}

#define STATE_FIELDS(X)                                                                                    \
    X(x, ego.x, EN, float) X(y, ego.y, EN, float) X(v, ego.v, EN, float) X(heading, ego.h, EN, float)      \
    X(acc, ego.acc, EN, float) X(steering, ego.steer, EN, float) X(prev_dist, ego.prev_dist, EN, float)    \
    X(prev_a0, ego.pa0, EN, float) X(prev_a1, ego.pa1, EN, float) X(spawn_x, ego.sx, EN, float)            \
    X(spawn_y, ego.sy, EN, float) X(spawn_v, ego.sv, EN, float) X(spawn_heading, ego.sh, EN, float)        \
    X(path_index, ego.pidx, EN, int32_t) X(route, ego.route, EN, int32_t)                                  \
    X(intention, ego.intent, EN, int32_t) X(alive, ego.alive, EN, uint8_t)                                 \
    X(npc_x, npc.x, EK, float) X(npc_y, npc.y, EK, float) X(npc_v, npc.v, EK, float)                        \
    X(npc_heading, npc.h, EK, float) X(npc_acc, npc.acc, EK, float) X(npc_steering, npc.steer, EK, float)  \
    X(npc_path_index, npc.pidx, EK, int32_t) X(npc_route, npc.route, EK, int32_t)                          \
    X(npc_intention, npc.intent, EK, int32_t) X(npc_alive, npc.alive, EK, uint8_t)                         \
    X(npc_count, npc.count, E, int32_t) X(step_count, step_count, E, int32_t)

int mev_get_state(mev_handle* h, const mev_state* s) {
    if (!h || !s) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const size_t E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents);
    const size_t EK = E * size_t(h->cfg.max_npcs);
    // Staged through pinned memory in at most six DMA copies: the 4-byte fields of the
    // ego and of the NPC SoA are one block each (field k at k * stride), then the alive
    // flags and the per-env counters; one pageable copy per field cost ~15 us each
    // (29 of them: env.py's traffic_cars read-back per step).
    void* const ego4[mev::EF_COUNT] = {s->x, s->y, s->v, s->heading, s->acc, s->steering, s->prev_dist,
                                      s->prev_a0, s->prev_a1, s->spawn_x, s->spawn_y, s->spawn_v,
                                      s->spawn_heading, s->path_index, s->route, s->intention};
    void* const npc4[mev::NF_COUNT] = {s->npc_x, s->npc_y, s->npc_v, s->npc_heading, s->npc_acc,
                                      s->npc_steering, s->npc_path_index, s->npc_route, s->npc_intention};
    bool want_e = false, want_n = false;
    for (void* q : ego4) want_e |= q != nullptr;
    for (void* q : npc4) want_n |= q != nullptr;
    const size_t es = size_t(h->sp.ego.stride) * 4, ns = size_t(h->sp.npc.stride) * 4;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t o_e = 0, o_n = o_e + al(es * mev::EF_COUNT), o_ea = o_n + al(ns * mev::NF_COUNT);
    const size_t o_na = o_ea + al(EN), o_nc = o_na + al(EK), o_sc = o_nc + al(E * 4), total = o_sc + al(E * 4);
    if (h->gs_cap < total) {
        if (h->gs_pin) (void)hipHostFree(h->gs_pin);
        h->gs_pin = nullptr;
        h->gs_cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->gs_pin), total, hipHostMallocDefault));
        h->gs_cap = total;
    }
    uint8_t* st = h->gs_pin;
    auto d2h = [&](size_t off, const void* src, size_t bytes) -> hipError_t {
        return bytes ? hipMemcpyAsync(st + off, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    };
    if (want_e) HIP_TRY(d2h(o_e, h->sp.ego.x, es * mev::EF_COUNT));
    if (want_n && EK) HIP_TRY(d2h(o_n, h->sp.npc.x, ns * mev::NF_COUNT));
    if (s->alive) HIP_TRY(d2h(o_ea, h->sp.ego.alive, EN));
    if (s->npc_alive) HIP_TRY(d2h(o_na, h->sp.npc.alive, EK));
    if (s->npc_count) HIP_TRY(d2h(o_nc, h->sp.npc.count, E * 4));
    if (s->step_count) HIP_TRY(d2h(o_sc, h->sp.step_count, E * 4));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int k = 0; k < mev::EF_COUNT; ++k)
        if (ego4[k]) memcpy(ego4[k], st + o_e + size_t(k) * es, EN * 4);
    for (int k = 0; k < mev::NF_COUNT; ++k)
        if (npc4[k] && EK) memcpy(npc4[k], st + o_n + size_t(k) * ns, EK * 4);
    if (s->alive) memcpy(s->alive, st + o_ea, EN);
    if (s->npc_alive && EK) memcpy(s->npc_alive, st + o_na, EK);
    if (s->npc_count) memcpy(s->npc_count, st + o_nc, E * 4);
    if (s->step_count) memcpy(s->step_count, st + o_sc, E * 4);
    return MEV_OK;
}

int mev_set_state(mev_handle* h, const mev_state* s) {
    if (!h || !s) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const size_t E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents);
    const size_t EK = E * size_t(h->cfg.max_npcs);
    if (s->route)
        for (size_t i = 0; i < EN; ++i)
            if (s->route[i] < 0 || s->route[i] >= h->nroutes) return fail(MEV_E_RANGE, "route id out of range");
    if (s->npc_count)
        for (size_t e = 0; e < E; ++e)
            if (s->npc_count[e] < 0 || s->npc_count[e] > h->cfg.max_npcs) return fail(MEV_E_RANGE, "npc_count out of range");
    if (s->npc_route)
        for (size_t i = 0; i < EK; ++i)
            if (s->npc_route[i] < 0 || s->npc_route[i] >= h->nroutes) return fail(MEV_E_RANGE, "npc route id out of range");
#define SET(f, dev, n, T) \
    if (s->f) HIP_TRY(hipMemcpyAsync(h->sp.dev, s->f, (n) * sizeof(T), hipMemcpyHostToDevice, h->stream));
    STATE_FIELDS(SET)
#undef SET
    HIP_TRY(hipMemsetAsync(h->sp.pending_reset, 0, E, h->stream));
    h->deal_valid = false;
    HIP_TRY(mev::launch_observe_reset_lidar(h->sp, h->internal, h->stream));
    h->last.obs = h->internal.obs;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MEV_OK;
}

// The handle's own output buffers made to hold the last outputs: a step that wrote
// elsewhere (caller buffers, the pinned host block of a host-mode step, a packed
// gather row) is copied in, stream-ordered, and h->last points back at them.
static int sync_internal(mev_handle* h) {
    const size_t E = size_t(h->cfg.num_envs), EN = E * size_t(h->cfg.num_agents);
    const mev::Outputs& L = h->last;
    const mev::Outputs& I = h->internal;
    auto pull = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        if (!src || src == dst) return hipSuccess;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, h->stream);
    };
    if (L.state)  // a state-format gather row: rebuild the heads, decode the LiDAR codes
        HIP_TRY(mev::launch_decode_state(h->sp, L.state, L.lidar_u8, 0, int(L.state_n / h->cfg.num_agents), int(E),
                                         h->d_lidar_table, I.obs, h->stream));
    else if (L.lidar_u8)  // a compact-format gather row: decode heads + LiDAR codes into the obs rows
        HIP_TRY(mev::launch_unpack_lidar_u8(L.obs, L.lidar_u8, h->d_lidar_table, I.obs, int(EN), h->D, h->lidar_slots,
                                            h->stream));
    else
        HIP_TRY(pull(I.obs, L.obs, EN * size_t(h->D) * sizeof(float)));
    HIP_TRY(pull(I.rew, L.rew, EN * sizeof(float)));
    HIP_TRY(pull(I.done, L.done, EN));
    HIP_TRY(pull(I.status, L.status, EN));
    HIP_TRY(pull(I.term, L.term, E));
    HIP_TRY(pull(I.trunc, L.trunc, E));
    HIP_TRY(pull(I.alive_cnt, L.alive_cnt, E * sizeof(int32_t)));
    HIP_TRY(pull(I.step, L.step, E * sizeof(int32_t)));
    h->last = h->internal;
    return MEV_OK;
}

int mev_device_outputs(mev_handle* h, float** obs, float** rew, uint8_t** done, uint8_t** status, uint8_t** term,
                       uint8_t** trunc) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    if (int r = sync_internal(h)) return r;
    if (obs) *obs = h->internal.obs;
    if (rew) *rew = h->internal.rew;
    if (done) *done = h->internal.done;
    if (status) *status = h->internal.status;
    if (term) *term = h->internal.term;
    if (trunc) *trunc = h->internal.trunc;
    return MEV_OK;
}

int mev_kernel_timing(mev_handle* h, int32_t enable) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (enable < 0) return fail(MEV_E_INVALID, "enable must be >= 0");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    if (!enable) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->free_timing();
        return MEV_OK;
    }
    if (h->tev.empty()) {
        const int ring = 4096;  // steps between host folds
        h->tev.resize(size_t(3 * ring), nullptr);
        for (auto& ev : h->tev) HIP_TRY(hipEventCreate(&ev));
    }
    h->tn = 0;
    h->t_every = enable;
    h->t_phase = 0;
    h->t_cars_ms = h->t_lidar_ms = 0.0;
    h->t_steps = 0;
    return MEV_OK;
}

int mev_kernel_times(mev_handle* h, double* cars_ms, double* lidar_ms, int64_t* steps) {
    if (!h || !cars_ms || !lidar_ms || !steps) return fail(MEV_E_INVALID, "null argument");
    if (h->tev.empty()) return fail(MEV_E_INVALID, "kernel timing is not enabled");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(h->fold_timing());
    *cars_ms = h->t_cars_ms;
    *lidar_ms = h->t_lidar_ms;
    *steps = h->t_steps;
    h->t_cars_ms = h->t_lidar_ms = 0.0;
    h->t_steps = 0;
    return MEV_OK;
}

int mev_set_step_kernel(mev_handle* h, int32_t kernel) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (kernel < 0 || kernel > 2) return fail(MEV_E_INVALID, "step kernel must be 0 (auto), 1 (two kernels) or 2 (fused)");
    mev::SimParams q = h->sp;
    q.step_kernel = kernel;
    if (mev::plan_step(q).path == 0)
        return fail(MEV_E_INVALID, "the fused step kernel does not support this configuration (traffic mode or too much LDS)");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->sp.step_kernel = kernel;
    return MEV_OK;
}

int mev_get_step_kernel(const mev_handle* h, int32_t* kernel) {
    if (!h || !kernel) return fail(MEV_E_INVALID, "null argument");
    *kernel = mev::plan_step(h->sp).path;
    return MEV_OK;
}

int mev_set_step_pack(mev_handle* h, int32_t envs_per_wave) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (envs_per_wave != 0 && envs_per_wave != 1 && envs_per_wave != 2 && envs_per_wave != 4 && envs_per_wave != 8)
        return fail(MEV_E_INVALID, "envs per wave must be 0 (auto), 1, 2, 4 or 8");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->sp.step_pack = envs_per_wave;
    return MEV_OK;
}

int mev_get_step_pack(const mev_handle* h, int32_t* envs_per_wave) {
    if (!h || !envs_per_wave) return fail(MEV_E_INVALID, "null argument");
    *envs_per_wave = mev::plan_step(h->sp).pack;
    return MEV_OK;
}

int mev_set_step_split(mev_handle* h, int32_t mode) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (mode < 0 || mode > 3)
        return fail(MEV_E_INVALID, "split mode must be 0 (auto), 1 (off), 2 (on) or 3 (early split)");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->sp.step_split = mode;
    h->deal_valid = false;  // (the traffic early split deals several envs per workgroup: restart the rings)
    return MEV_OK;
}

int mev_set_env_deal(mev_handle* h, int32_t on) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (on != 0 && on != 1) return fail(MEV_E_INVALID, "env deal must be 0 (off) or 1 (on)");
    h->deal_on = on != 0;
    h->deal_valid = false;  // the next step deals by the identity order (and rebuilds the rings)
    return MEV_OK;
}

int mev_get_step_split(const mev_handle* h, int32_t* split) {
    if (!h || !split) return fail(MEV_E_INVALID, "null argument");
    *split = mev::plan_step(h->sp).split;
    return MEV_OK;
}

int mev_get_step_row(const mev_handle* h, int32_t* step_row, int32_t* serve_row, int32_t* tab) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    const mev::StepPlan pl = mev::plan_step(h->sp);
    // (the pinned block of a small handle holds rows of the same width as the internal buffers)
    if (step_row) *step_row = mev::step_row(pl, mev::plain_rows(h->sp, h->internal));
    if (serve_row) *serve_row = mev::serve_row(pl);
    if (tab) *tab = h->sp.dist_tab ? 1 : 0;
    return MEV_OK;
}

int mev_set_reset_routes(mev_handle* h, const int32_t* routes, int32_t count) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (count < 0 || count > h->P * h->P)
        return fail(MEV_E_INVALID, "count must be in [0, number of lane-layout routes]");
    if (count > 0 && !routes) return fail(MEV_E_INVALID, "null routes");
    for (int32_t i = 0; i < count; ++i)
        if (routes[i] < 0 || routes[i] >= h->nroutes) return fail(MEV_E_RANGE, "route id out of range");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    if (count > 0) {
        HIP_TRY(hipMemcpyAsync(h->d_reset_routes, routes, size_t(count) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->sp.n_reset_routes = count;
    return MEV_OK;
}

// ---- device snapshots: header + every state field + the last outputs, each
// field [E][bytes per env] at a 256-B aligned offset
namespace {
struct SnapField {
    uint8_t* live;     // device field (state, or the outputs the snapshot reads)
    uint8_t* restore;  // where mev_restore writes it
    size_t bpe;        // bytes per env
};
struct SnapHeader {
    uint32_t magic, version;
    int32_t E, N, K, D, R, nfields;
    uint64_t rng_counter, total_bytes;
    int32_t dims;     // SimParams::dims of the snapshot's handle (some car not 54 x 24)
    int32_t nroutes;  // its route table's size (route ids must name the same routes on restore)
    uint64_t route_hash;  // mev_handle::route_hash[nroutes]
};
constexpr uint32_t kSnapVersion = 2;  // 2: car sizes, dims flag and route count
static_assert(sizeof(SnapHeader) == 64, "snapshot header");
constexpr uint32_t kSnapMagic = 0x5356454du;  // "MEVS"

static std::vector<SnapField> snap_fields(mev_handle* h) {
    const size_t N = size_t(h->cfg.num_agents), K = size_t(h->cfg.max_npcs), D = size_t(h->D);
    std::vector<SnapField> f;
    auto add = [&](void* live, void* restore, size_t bpe) {
        if (bpe) f.push_back({static_cast<uint8_t*>(live), static_cast<uint8_t*>(restore), bpe});
    };
#define SNAP(name, dev, n, T) add(h->sp.dev, h->sp.dev, (std::string(#n) == "EN" ? N : std::string(#n) == "EK" ? K : 1) * sizeof(T));
    STATE_FIELDS(SNAP)
#undef SNAP
    add(h->sp.pending_reset, h->sp.pending_reset, 1);
    add(h->sp.ego_dim, h->sp.ego_dim, N * 2 * sizeof(float));  // car sizes (mev_set_car_dims)
    add(h->sp.npc_dim, h->sp.npc_dim, K * 2 * sizeof(float));
    const mev::Outputs& L = h->last;
    const mev::Outputs& I = h->internal;
    add(L.obs ? L.obs : I.obs, I.obs, N * D * sizeof(float));
    add(L.rew ? L.rew : I.rew, I.rew, N * sizeof(float));
    add(L.done ? L.done : I.done, I.done, N);
    add(L.status ? L.status : I.status, I.status, N);
    add(L.term ? L.term : I.term, I.term, 1);
    add(L.trunc ? L.trunc : I.trunc, I.trunc, 1);
    add(L.alive_cnt ? L.alive_cnt : I.alive_cnt, I.alive_cnt, sizeof(int32_t));
    add(L.step ? L.step : I.step, I.step, sizeof(int32_t));
    return f;
}

size_t snap_offsets(const std::vector<SnapField>& f, size_t E, std::vector<size_t>* off) {
    size_t o = sizeof(SnapHeader);
    for (const SnapField& x : f) {
        o = (o + 255) & ~size_t(255);
        if (off) off->push_back(o);
        o += x.bpe * E;
    }
    return o;
}
}  // namespace

int mev_snapshot_size(mev_handle* h, uint64_t* bytes) {
    if (!h || !bytes) return fail(MEV_E_INVALID, "null argument");
    *bytes = snap_offsets(snap_fields(h), size_t(h->cfg.num_envs), nullptr);
    return MEV_OK;
}

int mev_snapshot(mev_handle* h, void* dst, uint32_t flags) {
    if (!h || !dst) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const bool dev = (flags & MEV_DEVICE_PTRS) != 0;
    const size_t E = size_t(h->cfg.num_envs);
    if (h->last.lidar_u8) {  // compact gather row: the snapshot stores plain obs rows
        if (int r0 = sync_internal(h)) return r0;
    }
    const std::vector<SnapField> f = snap_fields(h);
    std::vector<size_t> off;
    const size_t total = snap_offsets(f, E, &off);
    SnapHeader hd{};
    hd.magic = kSnapMagic; hd.version = kSnapVersion;
    hd.dims = h->sp.dims; hd.nroutes = h->nroutes; hd.route_hash = h->route_hash[size_t(h->nroutes)];
    hd.E = h->cfg.num_envs; hd.N = h->cfg.num_agents; hd.K = h->cfg.max_npcs; hd.D = h->D; hd.R = h->cfg.lidar_rays;
    hd.nfields = int32_t(f.size()); hd.rng_counter = h->rng_counter; hd.total_bytes = total;
    uint8_t* d = static_cast<uint8_t*>(dst);
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (dev) HIP_TRY(hipMemcpyAsync(d, &hd, sizeof(hd), hipMemcpyHostToDevice, h->stream));
    else memcpy(d, &hd, sizeof(hd));
    for (size_t i = 0; i < f.size(); ++i) HIP_TRY(hipMemcpyAsync(d + off[i], f[i].live, f[i].bpe * E, kind, h->stream));
    // the header copy reads host memory: always wait before returning in device mode too
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MEV_OK;
}

// A snapshot's header, checked against the handle before a restore touches it: a mismatched
// snapshot leaves the handle unchanged.  per_env: the restore goes through the per-env copy
// kernels (k_restore, k_restore_map) and their field table.
static int snap_read_header(mev_handle* h, const void* src, bool dev, bool per_env, SnapHeader& hd) {
    const size_t E = size_t(h->cfg.num_envs);
    if (dev) {
        HIP_TRY(hipMemcpyAsync(&hd, src, sizeof(hd), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    } else {
        memcpy(&hd, src, sizeof(hd));
    }
    {
        const mev::Outputs save_last = h->last;
        h->last = h->internal;  // the field table of a restore (its targets are the internal buffers)
        const std::vector<SnapField> f0 = snap_fields(h);
        h->last = save_last;
        const size_t total0 = snap_offsets(f0, E, nullptr);
        if (hd.magic == kSnapMagic && hd.version == 1)  // (no car sizes, no route count / hash to check ids by)
            return fail(MEV_E_INVALID, "snapshot format 1 is no longer supported (format 2 adds car sizes and the "
                                       "route table's hash): take the snapshot again with this library");
        if (hd.magic != kSnapMagic || hd.version != kSnapVersion || hd.E != h->cfg.num_envs || hd.N != h->cfg.num_agents ||
            hd.K != h->cfg.max_npcs || hd.D != h->D || hd.nfields != int32_t(f0.size()) || hd.total_bytes != total0)
            return fail(MEV_E_INVALID, "snapshot does not match this handle");
        // the snapshot's route ids index its handle's route table (lane-layout routes, then
        // mev_add_route's): a handle with fewer routes would read past the end of its tables
        if (hd.nroutes < 0 || hd.nroutes > h->nroutes || hd.route_hash != h->route_hash[size_t(hd.nroutes)])
            return fail(MEV_E_INVALID, "snapshot's routes differ from this handle's (mev_add_route)");
        if (per_env && f0.size() > size_t(mev::kMaxRestoreFields)) return fail(MEV_E_INVALID, "too many snapshot fields");
    }
    return MEV_OK;
}

static mev::RestoreTab restore_tab(const std::vector<SnapField>& f, const std::vector<size_t>& off) {
    mev::RestoreTab tab{};
    tab.n = int32_t(f.size());
    for (size_t i = 0; i < f.size(); ++i) {
        tab.dst[i] = f[i].restore;
        tab.src_off[i] = off[i];
        tab.bpe[i] = int32_t(f[i].bpe);
    }
    return tab;
}

int mev_restore(mev_handle* h, const void* src, const uint8_t* env_mask, uint32_t flags) {
    if (!h || !src) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const bool dev = (flags & MEV_DEVICE_PTRS) != 0;
    const size_t E = size_t(h->cfg.num_envs);
    SnapHeader hd{};
    if (int r = snap_read_header(h, src, dev, env_mask != nullptr, hd)) return r;
    // the live outputs are restored into the handle's own buffers; envs a masked
    // restore leaves alone keep their current outputs, so bring those in first
    if (env_mask) {
        if (int r = sync_internal(h)) return r;
    }
    h->last = h->internal;
    h->deal_valid = false;
    const std::vector<SnapField> f = snap_fields(h);
    std::vector<size_t> off;
    const size_t total = snap_offsets(f, E, &off);
    const uint8_t* s = static_cast<const uint8_t*>(src);
    Stage st(h, dev);  // (unmasked: nothing staged, the copies go straight into the state arrays)
    if (!env_mask) {
        const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        for (size_t i = 0; i < f.size(); ++i) HIP_TRY(hipMemcpyAsync(f[i].restore, s + off[i], f[i].bpe * E, kind, h->stream));
        h->rng_counter = hd.rng_counter;
        h->sp.dims = hd.dims;
    } else {
        const uint8_t *dsrc = nullptr, *dmask = nullptr;
        st.in(&dsrc, s, total);  // the per-env copy kernel reads the snapshot and the mask on the device
        st.in(&dmask, env_mask, E);
        if (int r = st.upload()) return r;
        HIP_TRY(mev::launch_restore(restore_tab(f, off), dsrc, dmask, h->cfg.num_envs, h->stream));
        h->sp.dims = h->sp.dims || hd.dims;  // (the sizes arrays hold valid entries either way)
    }
    return st.download();
}

int mev_restore_map(mev_handle* h, const void* src, const int32_t* env_map, uint32_t flags) {
    if (!h || !src || !env_map) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const bool dev = (flags & MEV_DEVICE_PTRS) != 0;
    const size_t E = size_t(h->cfg.num_envs);
    SnapHeader hd{};
    if (int r = snap_read_header(h, src, dev, true, hd)) return r;
    if (!dev) {  // (a device map's bad entries are skipped by the kernel)
        for (size_t e = 0; e < E; ++e)
            if (env_map[e] < -1 || env_map[e] >= int32_t(E))
                return fail(MEV_E_RANGE, "env_map[" + std::to_string(e) + "] = " + std::to_string(env_map[e]) +
                                             " is outside [-1, " + std::to_string(E) + ")");
    }
    // envs the map leaves alone keep their current outputs: bring those into the handle's own
    // buffers, the restore's targets, first (as a masked mev_restore)
    if (int r = sync_internal(h)) return r;
    h->last = h->internal;
    h->deal_valid = false;
    const std::vector<SnapField> f = snap_fields(h);
    std::vector<size_t> off;
    const size_t total = snap_offsets(f, E, &off);
    const uint8_t* dsrc = nullptr;
    const int32_t* dmap = nullptr;
    Stage st(h, dev);
    st.in(&dsrc, static_cast<const uint8_t*>(src), total);
    st.in(&dmap, env_map, E);
    if (int r = st.upload()) return r;
    HIP_TRY(mev::launch_restore_map(restore_tab(f, off), dsrc, dmap, h->cfg.num_envs, h->stream));
    h->sp.dims = h->sp.dims || hd.dims;  // (the sizes arrays hold valid entries either way)
    return st.download();
}

// ---- multi-GPU gather (include/marlenv.h) ----------------
int mev_packed_layout(int32_t slots, int32_t num_agents, int32_t obs_dim, uint64_t* offsets, uint64_t* bytes) {
    if (!offsets || !bytes) return fail(MEV_E_INVALID, "null argument");
    if (slots < 1 || num_agents < 1 || obs_dim < 1) return fail(MEV_E_INVALID, "slots, agents and obs_dim must be >= 1");
    const uint64_t C = uint64_t(slots), N = uint64_t(num_agents), D = uint64_t(obs_dim);
    const uint64_t sizes[MEV_PK_COUNT] = {C * N * D * 4, C * N * 4, C * N, C * N, C, C};
    uint64_t off = 0;
    for (int f = 0; f < MEV_PK_COUNT; ++f) {
        off = (off + 255) & ~uint64_t(255);
        offsets[f] = off;
        off += sizes[f];
    }
    *bytes = (off + 255) & ~uint64_t(255);
    return MEV_OK;
}

int mev_packed_layout2(int32_t slots, int32_t num_agents, int32_t obs_dim, int32_t lidar_slots, int32_t format,
                       uint64_t* offsets, uint64_t* bytes) {
    if (!offsets || !bytes) return fail(MEV_E_INVALID, "null argument");
    if (slots < 1 || num_agents < 1 || obs_dim < mev::OBS_HEAD || lidar_slots < 0 || lidar_slots > obs_dim - mev::OBS_HEAD)
        return fail(MEV_E_INVALID, "slots and agents must be >= 1, obs_dim >= 31, 0 <= lidar_slots <= obs_dim - 31");
    if (format != MEV_GATHER_F32 && format != MEV_GATHER_LIDAR_U8 && format != MEV_GATHER_STATE)
        return fail(MEV_E_INVALID, "unknown gather format");
    const uint64_t C = uint64_t(slots), N = uint64_t(num_agents);
    const bool codes = format != MEV_GATHER_F32, st = format == MEV_GATHER_STATE;
    const uint64_t row = st ? 0 : (codes ? uint64_t(mev::OBS_HEAD) : uint64_t(obs_dim));
    const uint64_t sizes[MEV_PK_FIELDS] = {C * N * row * 4, C * N * 4, C * N, C * N, C, C,
                                           codes ? C * N * uint64_t(lidar_slots) : 0,
                                           st ? C * N * uint64_t(mev::kStateBytesPerAgent) : 0};
    uint64_t off = 0;
    for (int f = 0; f < MEV_PK_FIELDS; ++f) {
        off = (off + 255) & ~uint64_t(255);
        offsets[f] = off;
        off += sizes[f];
    }
    *bytes = (off + 255) & ~uint64_t(255);
    return MEV_OK;
}

int mev_set_gather_format(mev_handle* h, int32_t format) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (format != MEV_GATHER_F32 && format != MEV_GATHER_LIDAR_U8 && format != MEV_GATHER_STATE)
        return fail(MEV_E_INVALID, "unknown gather format");
    if (h->comm) return fail(MEV_E_INVALID, "set the gather format before mev_comm_init");
    if (format != MEV_GATHER_F32 && h->sp.lidar_steps + 1 >= mev::kLidarCodeDead)
        return fail(MEV_E_INVALID, "the compact gather formats need at most 253 LiDAR march probes");
    if (format == MEV_GATHER_STATE && (h->cfg.traffic_flow || h->cfg.num_agents > 64))
        return fail(MEV_E_INVALID, "the state gather format is for handles without traffic (N <= 64)");
    h->gather_fmt = format;
    return MEV_OK;
}

int mev_lidar_decode_table(const mev_handle* h, float* table) {
    if (!h || !table) return fail(MEV_E_INVALID, "null argument");
    memcpy(table, h->h_lidar_table.data(), 256 * sizeof(float));
    return MEV_OK;
}

int mev_comm_unique_id(uint8_t* id) {
    if (!id) return fail(MEV_E_INVALID, "null argument");
    static_assert(sizeof(ncclUniqueId) == MEV_COMM_ID_BYTES, "unique id size");
    ncclUniqueId u;
    const ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return fail(MEV_E_HIP, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    memcpy(id, &u, sizeof(u));
    return MEV_OK;
}

int mev_comm_init(mev_handle* h, const uint8_t* id, int32_t world, int32_t rank, int32_t root, int32_t slots) {
    if (!h || !id) return fail(MEV_E_INVALID, "null argument");
    if (h->comm) return fail(MEV_E_INVALID, "the handle already has a communicator");
    if (world < 1 || rank < 0 || rank >= world || root < 0 || root >= world)
        return fail(MEV_E_INVALID, "bad world / rank / root");
    if (slots <= 0) slots = h->cfg.num_envs;
    if (slots < h->cfg.num_envs) return fail(MEV_E_INVALID, "slots must be >= num_envs");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    int rc = mev_packed_layout2(slots, h->cfg.num_agents, h->D, h->lidar_slots, h->gather_fmt, h->pk_off, &h->pk_bytes);
    if (rc) return rc;
    // the check buffer before the communicator: once ncclCommInitRank returned, every rank
    // must reach the exchange below (a rank that left early would hang its peers in it)
    constexpr int kChk = 5;  // nroutes, route hash, gather format, packed bytes, ok
    uint64_t* dchk = nullptr;
    if (world > 1) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&dchk), size_t(world + 1) * kChk * sizeof(uint64_t)));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    const ncclResult_t nr = ncclCommInitRank(&comm, world, u, rank);
    if (nr != ncclSuccess) {
        if (dchk) (void)hipFree(dchk);
        return fail(MEV_E_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(nr));
    }
    h->comm = comm;
    h->world = world; h->rank = rank; h->root = root; h->slots = slots; h->gathers = 0;
    hipError_t e = hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking);
    if (world > 1) {
        // Every rank, whatever its format or local errors: the packed layout (format and
        // bytes per rank) must agree, and with the state format the route tables too (the
        // root rebuilds every rank's observation heads from route ids with ITS table:
        // mev_add_route in the same order everywhere).  Local failures travel as ok = 0, so
        // every rank returns the same verdict.
        const uint64_t mine[kChk] = {uint64_t(h->nroutes), h->route_hash[size_t(h->nroutes)], uint64_t(h->gather_fmt),
                                     uint64_t(h->pk_bytes), e == hipSuccess ? 1u : 0u};
        std::vector<uint64_t> all(size_t(world) * kChk, 0);
        hipError_t ce = hipMemcpy(dchk, mine, sizeof(mine), hipMemcpyHostToDevice);
        const ncclResult_t ar = ncclAllGather(dchk, dchk + kChk, kChk, ncclUint64, comm, h->stream);
        if (ar == ncclSuccess) {
            const hipError_t se = hipStreamSynchronize(h->stream);
            if (ce == hipSuccess) ce = se;
            if (ce == hipSuccess) ce = hipMemcpy(all.data(), dchk + kChk, all.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
        }
        (void)hipFree(dchk);
        if (ar != ncclSuccess) {
            h->free_comm();
            return fail(MEV_E_HIP, std::string("RCCL layout check: ") + ncclGetErrorString(ar));
        }
        if (ce != hipSuccess) {
            h->free_comm();
            return fail(MEV_E_HIP, std::string("layout check: ") + hipGetErrorString(ce));
        }
        for (int r = 0; r < world; ++r) {
            const uint64_t* o = &all[size_t(r) * kChk];
            const char* why = nullptr;
            if (o[4] != 1) why = "a rank failed to create its communication stream";
            else if (o[2] != mine[2] || o[3] != mine[3])
                why = "the ranks' gather layouts differ (mev_set_gather_format, num_agents, obs_dim, slots)";
            else if (h->gather_fmt == MEV_GATHER_STATE && (o[0] != mine[0] || o[1] != mine[1]))
                why = "the ranks' route tables differ (mev_add_route): the state gather format decodes every "
                      "rank's route ids with the root's table";
            if (why) {
                h->free_comm();
                return fail(MEV_E_INVALID, why);
            }
        }
    }
    const size_t per = (rank == root) ? size_t(world) * h->pk_bytes : h->pk_bytes;
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = hipMalloc(reinterpret_cast<void**>(&h->pk_buf[b]), per);
        if (e == hipSuccess) e = hipMemsetAsync(h->pk_buf[b], 0, per, h->stream);  // unused slot tails stay 0
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_step[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_gather[b], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->free_comm();
        return fail(MEV_E_NOMEM, std::string("gather buffers: ") + hipGetErrorString(e));
    }
    return MEV_OK;
}

int mev_comm_destroy(mev_handle* h) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->comm_stream) HIP_TRY(hipStreamSynchronize(h->comm_stream));
    h->free_comm();
    return MEV_OK;
}

int mev_gather_result(mev_handle* h, void** stacked, uint64_t* bytes_per_rank, int32_t* world) {
    if (!h || !stacked || !bytes_per_rank || !world) return fail(MEV_E_INVALID, "null argument");
    if (!h->comm) return fail(MEV_E_INVALID, "no communicator (mev_comm_init)");
    if (h->rank != h->root) return fail(MEV_E_INVALID, "the gather result lives on the root rank");
    if (h->gathers == 0) return fail(MEV_E_INVALID, "no step has been gathered yet");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const int b = int((h->gathers - 1) & 1);
    if (h->gather_pending[b]) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_gather[b], 0));
    *stacked = h->pk_buf[b];
    *bytes_per_rank = h->pk_bytes;
    *world = h->world;
    return MEV_OK;
}

int mev_unpack_gathered(mev_handle* h, const void* stacked, int32_t world, float* obs) {
    if (!h || !stacked || !obs) return fail(MEV_E_INVALID, "null argument");
    if (!h->comm) return fail(MEV_E_INVALID, "no communicator (mev_comm_init): the layout is the handle's");
    if (world < 1 || world > h->world) return fail(MEV_E_INVALID, "world must be in [1, the communicator's world]");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const uint8_t* sb = static_cast<const uint8_t*>(stacked);
    const size_t C = size_t(h->slots), N = size_t(h->cfg.num_agents), D = size_t(h->D);
    const size_t rows = C * N;
    for (int r = 0; r < world; ++r) {
        const uint8_t* m = sb + size_t(r) * h->pk_bytes;
        float* o = obs + size_t(r) * rows * D;
        if (h->gather_fmt == MEV_GATHER_F32)
            HIP_TRY(hipMemcpyAsync(o, m + h->pk_off[MEV_PK_OBS], rows * D * sizeof(float), hipMemcpyDeviceToDevice,
                                   h->stream));
        else if (h->gather_fmt == MEV_GATHER_LIDAR_U8)
            HIP_TRY(mev::launch_unpack_lidar_u8(reinterpret_cast<const float*>(m + h->pk_off[MEV_PK_OBS]),
                                                m + h->pk_off[MEV_PK_LIDAR], h->d_lidar_table, o, int(rows), h->D,
                                                h->lidar_slots, h->stream));
    }
    if (h->gather_fmt == MEV_GATHER_STATE)  // one launch over every rank's envs
        HIP_TRY(mev::launch_decode_state(h->sp, sb + h->pk_off[MEV_PK_STATE], sb + h->pk_off[MEV_PK_LIDAR], h->pk_bytes,
                                         int(C), int(C) * world, h->d_lidar_table, obs, h->stream));
    return MEV_OK;
}

// A failed or stuck gather: abort the communicator (its kernels exit), then
// release the gather resources as free_comm does, without ncclCommDestroy; the
// outputs of later queries come from the handle's own buffers again.
static void abort_comm(mev_handle* h) {
    (void)ncclCommAbort(h->comm);
    h->comm = nullptr;
    if (h->last.obs != h->internal.obs) h->last = h->internal;  // h->last pointed into a packed row
    h->free_comm();
}

int mev_gather_wait(mev_handle* h, int32_t timeout_ms) {
    if (!h) return fail(MEV_E_INVALID, "null handle");
    if (!h->comm) return fail(MEV_E_INVALID, "no communicator (mev_comm_init)");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    const auto t0 = std::chrono::steady_clock::now();
    for (int b = 0; b < 2; ++b) {
        if (!h->gather_pending[b]) continue;
        for (;;) {
            const hipError_t q = hipEventQuery(h->ev_gather[b]);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return fail(MEV_E_HIP, std::string("gather: ") + hipGetErrorString(q));
            ncclResult_t ae = ncclSuccess;
            if (ncclCommGetAsyncError(h->comm, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) {
                abort_comm(h);
                return fail(MEV_E_HIP, std::string("RCCL gather failed: ") + ncclGetErrorString(ae));
            }
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (timeout_ms > 0 && ms > double(timeout_ms)) {
                abort_comm(h);  // a lost peer must not hang the caller
                return fail(MEV_E_HIP, "RCCL gather timed out (communicator aborted)");
            }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        h->gather_pending[b] = false;
    }
    return MEV_OK;
}

// ---- DLPack export of the internal output buffers ---------------------------
namespace {
struct DlBox {
    mev_dl_managed m;
    int64_t shape[3];
};
void dl_delete(mev_dl_managed* m) { delete reinterpret_cast<DlBox*>(m); }
}  // namespace

int mev_output_dlpack(mev_handle* h, int32_t which, mev_dl_managed** out) {
    if (!h || !out) return fail(MEV_E_INVALID, "null argument");
    const int64_t E = h->cfg.num_envs, N = h->cfg.num_agents, D = h->D;
    void* data = nullptr;
    int nd = 1;
    int64_t sh[3] = {E, 0, 0};
    mev_dl_dtype dt{1, 8, 1};  // u8
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    if (which != MEV_OUT_GATHERED) {
        if (int r = sync_internal(h)) return r;
    }
    const mev::Outputs& I = h->internal;
    switch (which) {
        case MEV_OUT_OBS: data = I.obs; nd = 3; sh[1] = N; sh[2] = D; dt = {2, 32, 1}; break;
        case MEV_OUT_REWARD: data = I.rew; nd = 2; sh[1] = N; dt = {2, 32, 1}; break;
        case MEV_OUT_DONE: data = I.done; nd = 2; sh[1] = N; break;
        case MEV_OUT_STATUS: data = I.status; nd = 2; sh[1] = N; break;
        case MEV_OUT_TERMINATED: data = I.term; break;
        case MEV_OUT_TRUNCATED: data = I.trunc; break;
        case MEV_OUT_AGENTS_ALIVE: data = I.alive_cnt; dt = {0, 32, 1}; break;
        case MEV_OUT_STEP: data = I.step; dt = {0, 32, 1}; break;
        case MEV_OUT_GATHERED:
            if (!h->comm || h->rank != h->root) return fail(MEV_E_INVALID, "the gather buffer lives on the root rank");
            {
                const int b = h->gathers > 0 ? int((h->gathers - 1) & 1) : 0;
                // as mev_gather_result: the handle's stream waits for the RCCL receives into it
                if (h->gather_pending[b]) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_gather[b], 0));
                data = h->pk_buf[b];
            }
            nd = 2; sh[0] = h->world; sh[1] = int64_t(h->pk_bytes);
            break;
        default: return fail(MEV_E_INVALID, "unknown output");
    }
    auto* box = new DlBox();
    for (int k = 0; k < 3; ++k) box->shape[k] = sh[k];
    mev_dl_tensor& t = box->m.dl_tensor;
    t.data = data;
    t.device = {10, h->cfg.device};  // kDLROCM
    t.ndim = nd;
    t.dtype = dt;
    t.shape = box->shape;
    t.strides = nullptr;
    t.byte_offset = 0;
    box->m.manager_ctx = nullptr;
    box->m.deleter = dl_delete;
    *out = &box->m;
    return MEV_OK;
}

int mev_npc_overflow(mev_handle* h, int64_t* count) {
    if (!h || !count) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, h->sp.overflow, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *count = int64_t(v);
    return MEV_OK;
}

int mev_npc_stats(mev_handle* h, int64_t* overflow, int64_t* sequential_turns) {
    if (!h || !overflow || !sequential_turns) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(v, h->sp.overflow, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *overflow = int64_t(v[0]);
    *sequential_turns = int64_t(v[1]);
    return MEV_OK;
}

int mev_decode_errors(mev_handle* h, int64_t* count) {
    if (!h || !count) return fail(MEV_E_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (int r_ = serve_stop(h)) return r_;  // (the server holds the stream)
    unsigned long long v[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(v, h->sp.overflow, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *count = int64_t(v[2]);
    return MEV_OK;
}

}  // extern "C"
