// extern "C" entry points of libbridges_hip.so (see include/bridges_hip.h).  Unity build: the kernel
// translation units are included here so one hipcc invocation produces the library.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "env_kernels.hip"
#include "ops_kernels.hip"
#include "dqn_kernels.hip"
#include "mlp_kernels.hip"
#include "conv_kernels.hip"
#include "conv_train_kernels.hip"
#include "replay_kernels.hip"
#include "hindsight_kernels.hip"
#include "fork_kernels.hip"
#include "beam_kernels.hip"
#include "soft_target_kernels.hip"
#include "munchausen_kernels.hip"

using namespace bridges;

static thread_local char g_err[512] = "";

static int fail_hip(hipError_t e, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return BRIDGES_E_HIP;
}
static int fail_arg(const char* what) {
    snprintf(g_err, sizeof(g_err), "bad argument: %s", what);
    return BRIDGES_E_ARG;
}
static int fail_arg(const char* who, const char* what) {
    snprintf(g_err, sizeof(g_err), "bad argument: %s: %s", who, what);
    return BRIDGES_E_ARG;
}
#define HIP_TRY(x)                                        \
    do {                                                  \
        hipError_t e_ = (x);                              \
        if (e_ != hipSuccess) return fail_hip(e_, #x);    \
    } while (0)

// Every kernel launch of the library: a failed launch is reported as `name`.
template <typename... P, typename... A>
static int launch(const char* name, void (*k)(P...), dim3 grid, dim3 block, size_t lds, void* stream, A... a) {
    hipLaunchKernelGGL(k, grid, block, lds, (hipStream_t)stream, a...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BRIDGES_OK : fail_hip(e, name);
}

// Every pointer a multiple of `bytes` (a power of two); null pointers pass.
template <typename... T>
static bool aligned(uintptr_t bytes, const T*... p) {
    return ((((uintptr_t)p) | ... | (uintptr_t)0) & (bytes - 1)) == 0;
}

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The grid of a grid-stride kernel: `blocks` clamped to [1, limit].
static int64_t clamp_grid(int64_t blocks, int64_t limit) {
    if (blocks < 1) blocks = 1;
    return blocks > limit ? limit : blocks;
}

// One wave per item, four per 256-thread workgroup.
static int grid_for_waves(int64_t n_items) { return (int)clamp_grid(ceil_div(n_items, 4), 2048); }

static int up2_splits(int64_t tiles, int* tps) {
    int per = (int)((tiles + 255) / 256);
    if (per < 1) per = 1;
    *tps = per;
    return (int)((tiles + per - 1) / per);
}

// k_c3 for one image width and channel chunk (CH 4 for 1..4 input channels, else 16), by epilogue.  If-chains in function
// templates rather than nested ?: in the caller keep the order in which the kernels are instantiated, and so the device code.
typedef void (*c3_fn)(const float*, const float*, const float*, const float*, const float*, float*, int, int, int, int, int);
template <int W, int CH>
static c3_fn c3_epilogue(int mode) {
    if (mode == C3_EPI_BIAS_RELU) return k_c3<W, CH, C3_EPI_BIAS_RELU>;
    if (mode == C3_EPI_MASK) return k_c3<W, CH, C3_EPI_MASK>;
    return k_c3<W, CH, C3_EPI_RAW>;
}
template <int W>
static c3_fn c3_kernel(int c_in, int mode) { return c_in <= 4 ? c3_epilogue<W, 4>(mode) : c3_epilogue<W, 16>(mode); }

struct bridges_gate {
    hipEvent_t last;           // completion of the most recent rasteriser launch attached to this gate (or null)
};

struct bridges_env {
    bridges_gate* gate;
    hipEvent_t raster_done;
    DevCtx ctx;
    TaskTable* tt_dev;
    int32_t* h_total;          // pinned: candidate count of the previous lock-step (sizes the raster / expand grids)
    int max_blocks;            // upper bound of a useful grid
    int max_faces;             // most 2-D faces among the task's candidate shapes (picks the rasteriser instantiation)
    // optional per-launch timing of the dominant kernel (k_raster) with HIP events on the launch stream
    hipEvent_t* ev_start;
    hipEvent_t* ev_stop;
    int ev_cap, ev_used;
    // per-env tasks (bridges_env_set_task_buffers): while attached, ctx.b.reward_map / reward_prefix point at the per-env tables
    bool has_tasks;
    bridges_task_buffers tasks;
    const float* fixed_reward_map;         // the fixed task's tables, restored when the buffers are detached
    const double* fixed_reward_prefix;
    // task family (bridges_env_set_task_family): family.family != BRIDGES_FAMILY_NONE while one is set
    bridges_task_family family;
    // its threshold table (bridges_env_set_family_thresholds): caller-owned device memory, NULL = the uniform draw
    const uint64_t* family_thr;
};

static void clear_family(bridges_env* env) {
    memset(&env->family, 0, sizeof(env->family));
    env->family_thr = nullptr;
}

// The previous lock-step's candidate count (+3 %, at least one per env), which sizes the grids over candidates.  Those
// kernels grid-stride, so a stale or low estimate costs time, never correctness.
static long long candidate_estimate(const bridges_env* env) {
    long long est = (long long)(*(volatile int32_t*)env->h_total);
    if (est < env->ctx.E) est = env->ctx.E;
    return est + est / 32 + 64;
}

extern "C" {

const char* bridges_last_error(void) { return g_err; }

#ifndef BRIDGES_SRC_HASH
#define BRIDGES_SRC_HASH "unstamped"
#endif
const char* bridges_source_hash(void) { return "BRIDGES_SRC_HASH=" BRIDGES_SRC_HASH; }

int bridges_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bridges_env_create(const bridges_task* t, const bridges_env_buffers* buf, bridges_env** out) {
    if (!t || !buf || !out) return fail_arg("null");
    if (t->n_envs <= 0) return fail_arg("n_envs");
    if (t->max_blocks <= 0 || t->max_blocks > BRIDGES_MAX_BLOCKS) return fail_arg("max_blocks > BRIDGES_MAX_BLOCKS");
    if (t->n_shapes <= 0 || t->n_shapes > 8) return fail_arg("n_shapes");
    if (t->n_groups <= 0 || t->n_groups > BRIDGES_MAX_GROUPS) return fail_arg("n_groups");
    if (t->n_ground < 0 || t->n_ground > 32 || t->n_offsets <= 0 || t->n_offsets > 8) return fail_arg("n_ground/n_offsets");
    if (t->n_targets < 0 || t->n_targets > BRIDGES_MAX_TARGETS) return fail_arg("n_targets");
    if (t->a_max <= 0) return fail_arg("a_max");
    if (t->img_size != 0 && (t->img_size < 2 || t->img_size > BRIDGES_IMG)) return fail_arg("img_size must be 0 (= 64) or 2..64");
    if (t->debug != 0) return fail_arg("debug must be 0");
    if (!buf->reward_prefix) return fail_arg("reward_prefix (float64 row prefix sums of reward_map) not given");
    if (buf->lp_ws_stride < (int64_t)BRIDGES_LP_WS_DOUBLES) return fail_arg("lp_ws_stride < BRIDGES_LP_WS_DOUBLES");
    static_assert(BRIDGES_LP_WS_DOUBLES == WARM_WS_DOUBLES, "header and device code disagree on the persistent tableau size");
    static_assert(BRIDGES_LP_SNAP_DOUBLES == WARM_HDR_DOUBLES + WARM_HALF, "header and device code disagree on the snapshot size");
    if (buf->lp_snap && buf->lp_snap_stride < (int64_t)BRIDGES_LP_SNAP_DOUBLES) return fail_arg("lp_snap_stride < BRIDGES_LP_SNAP_DOUBLES");
    for (int g = 0; g < t->n_groups; ++g) {
        if (t->group_shape[g] < 0 || t->group_shape[g] >= t->n_shapes) return fail_arg("group_shape");
        if (t->group_face[g] < 0 || t->group_face[g] >= t->shapes[t->group_shape[g]].nv) return fail_arg("group_face");
    }
    for (int s = 0; s < t->n_shapes; ++s)
        if (t->shapes[s].nv < 3 || t->shapes[s].nv > BRIDGES_MAX_VERTS) return fail_arg("shape nv");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        snprintf(g_err, sizeof(g_err), "no HIP device");
        return BRIDGES_E_NODEV;
    }
    bridges_env* env = new (std::nothrow) bridges_env();
    if (!env) return fail_arg("oom");
    TaskTable* host = new (std::nothrow) TaskTable();
    if (!host) { delete env; return fail_arg("oom"); }
    memset(host, 0, sizeof(TaskTable));
    memcpy(host->shapes, t->shapes, sizeof(bridges_shape) * t->n_shapes);
    memcpy(host->x_ground, t->x_ground, sizeof(double) * t->n_ground);
    memcpy(host->offsets, t->offsets, sizeof(double) * t->n_offsets);
    const int img = t->img_size ? t->img_size : IMG;
    for (int i = 0; i < IMG; ++i) {                      // lanes / rows >= img repeat the last grid value (never inside)
        host->grid_x[i] = t->grid_x[i < img ? i : img - 1];
        host->grid_y[i] = t->grid_y[i < img ? i : img - 1];
    }
    hipError_t e = hipMalloc((void**)&env->tt_dev, sizeof(TaskTable));
    if (e == hipSuccess) e = hipMemcpy(env->tt_dev, host, sizeof(TaskTable), hipMemcpyHostToDevice);
    delete host;
    if (e != hipSuccess) { delete env; return fail_hip(e, "task table upload"); }
    DevCtx& c = env->ctx;
    memset(&c, 0, sizeof(c));
    c.b = *buf;
    c.tt = env->tt_dev;
    c.E = t->n_envs; c.K = t->max_blocks; c.max_steps = t->max_steps; c.a_max = t->a_max;
    c.n_groups = t->n_groups; c.n_ground = t->n_ground; c.n_offsets = t->n_offsets; c.n_targets = t->n_targets;
    memcpy(c.group_shape, t->group_shape, sizeof(c.group_shape));
    memcpy(c.group_face, t->group_face, sizeof(c.group_face));
    c.mu = t->mu; c.density = t->density; c.floor_hw = t->floor_half_width; c.floor_depth = t->floor_depth;
    c.xlim0 = t->xlim[0]; c.xlim1 = t->xlim[1]; c.ylim0 = t->ylim[0]; c.ylim1 = t->ylim[1];
    memcpy(c.targets, t->targets, sizeof(c.targets));
    c.seed = t->seed;
    c.debug = t->debug;
    c.env_id_base = t->env_id_base;
    c.n_shapes = t->n_shapes;
    c.img = img;
    env->ev_start = env->ev_stop = nullptr;
    env->ev_cap = env->ev_used = 0;
    env->gate = nullptr;
    env->raster_done = nullptr;
    env->has_tasks = false;
    memset(&env->tasks, 0, sizeof(env->tasks));
    clear_family(env);
    env->fixed_reward_map = buf->reward_map;
    env->fixed_reward_prefix = buf->reward_prefix;
    // mapped, coherent host word: k_scan stores the candidate count of the lock-step straight into it (no copy command
    // in the stream); the host reads it as a hint for the next grid, so a late value costs time, never correctness
    e = hipHostMalloc((void**)&env->h_total, sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&c.h_total, env->h_total, 0);
    if (e != hipSuccess) { (void)hipFree(env->tt_dev); delete env; return fail_hip(e, "hipHostMalloc"); }
    *env->h_total = t->n_envs * 64;        // first guess; replaced after every scan
    env->max_blocks = 1 << 22;
    env->max_faces = 0;
    for (int g = 0; g < t->n_groups; ++g) {
        const int nv = t->shapes[t->group_shape[g]].nv;
        if (nv > env->max_faces) env->max_faces = nv;
    }
    *out = env;
    return BRIDGES_OK;
}

static void free_events(bridges_env* env) {
    for (int i = 0; i < env->ev_cap; ++i) {
        (void)hipEventDestroy(env->ev_start[i]);
        (void)hipEventDestroy(env->ev_stop[i]);
    }
    delete[] env->ev_start;
    delete[] env->ev_stop;
    env->ev_start = env->ev_stop = nullptr;
    env->ev_cap = env->ev_used = 0;
}

int bridges_env_destroy(bridges_env* env) {
    if (!env) return BRIDGES_OK;
    free_events(env);
    if (env->raster_done) (void)hipEventDestroy(env->raster_done);
    (void)hipFree(env->tt_dev);
    (void)hipHostFree(env->h_total);
    delete env;
    return BRIDGES_OK;
}

int bridges_gate_create(bridges_gate** out) {
    if (!out) return fail_arg("gate_create");
    bridges_gate* g = new (std::nothrow) bridges_gate();
    if (!g) return fail_arg("oom");
    g->last = nullptr;
    *out = g;
    return BRIDGES_OK;
}

int bridges_gate_destroy(bridges_gate* gate) {
    delete gate;
    return BRIDGES_OK;
}

int bridges_env_set_gate(bridges_env* env, bridges_gate* gate) {
    if (!env) return fail_arg("set_gate");
    if (gate && !env->raster_done) HIP_TRY(hipEventCreateWithFlags(&env->raster_done, hipEventDisableTiming));
    env->gate = gate;
    return BRIDGES_OK;
}

int bridges_env_timing_begin(bridges_env* env, int32_t max_launches) {
    if (!env || max_launches <= 0 || max_launches > (1 << 16)) return fail_arg("timing_begin");
    free_events(env);
    env->ev_start = new (std::nothrow) hipEvent_t[max_launches];
    env->ev_stop = new (std::nothrow) hipEvent_t[max_launches];
    if (!env->ev_start || !env->ev_stop) {
        delete[] env->ev_start;
        delete[] env->ev_stop;
        env->ev_start = env->ev_stop = nullptr;
        return fail_arg("oom");
    }
    for (int i = 0; i < max_launches; ++i) {
        HIP_TRY(hipEventCreate(&env->ev_start[i]));
        HIP_TRY(hipEventCreate(&env->ev_stop[i]));
        env->ev_cap = i + 1;
    }
    env->ev_used = 0;
    return BRIDGES_OK;
}

int bridges_env_timing_end(bridges_env* env, double* raster_ms_total, int32_t* n_launches) {
    if (!env || !raster_ms_total || !n_launches) return fail_arg("timing_end");
    double total = 0.0;
    for (int i = 0; i < env->ev_used; ++i) {
        HIP_TRY(hipEventSynchronize(env->ev_stop[i]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, env->ev_start[i], env->ev_stop[i]));
        total += ms;
    }
    *raster_ms_total = total;
    *n_launches = env->ev_used;
    free_events(env);
    return BRIDGES_OK;
}

static int refresh(bridges_env* env, hipStream_t s, int after_step) {
    const DevCtx& c = env->ctx;
    if (int rc = launch("k_scan", k_scan, dim3(1), dim3(SCAN_THREADS), 0, s, c, after_step)) return rc;
    if (int rc = launch("k_enumerate", k_enumerate, dim3(c.E), dim3(WAVE), 0, s, c)) return rc;
    // k_scan stores the fresh candidate count into the mapped host word for the next call
    const long long items_est = candidate_estimate(env) + c.E;   // one wave per image (candidates + state rasters)
    long long rblocks = ceil_div(items_est, 4);
    if (rblocks > env->max_blocks) rblocks = env->max_blocks;
    const bool timed = env->ev_cap > 0 && env->ev_used < env->ev_cap;
    if (env->gate && env->gate->last) HIP_TRY(hipStreamWaitEvent(s, env->gate->last, 0));
    if (timed) HIP_TRY(hipEventRecord(env->ev_start[env->ev_used], s));
    // No dynamic LDS, so no cap on the rasteriser's occupancy: 8 workgroups (4 waves each) per CU fill every wave slot.
    // Capping it to leave room for the other env groups' task kernels cost the headline 5-6 % (profiles/r04_kstep_tail.txt).
    if (!env->has_tasks) {
        if (int rc = launch("k_raster", env->max_faces <= 4 ? k_raster<4> : k_raster<MAXV>, dim3((unsigned)rblocks), dim3(256), 0, s, c))
            return rc;
    } else if (env->tasks.n_obstacles == 0) {
        if (int rc = launch("k_raster (per-env tables)", env->max_faces <= 4 ? k_raster<4, true> : k_raster<MAXV, true>,
                            dim3((unsigned)rblocks), dim3(256), 0, s, c))
            return rc;
    } else if (int rc = launch("k_raster (per-env tables and obstacles)", env->max_faces <= 4 ? k_raster<4, true, const uint64_t*> : k_raster<MAXV, true, const uint64_t*>,
                               dim3((unsigned)rblocks), dim3(256), 0, s, c, (const uint64_t*)env->tasks.env_obstacle_bits)) {
        return rc;
    }
    if (timed) { HIP_TRY(hipEventRecord(env->ev_stop[env->ev_used], s)); env->ev_used++; }
    if (env->gate) {
        HIP_TRY(hipEventRecord(env->raster_done, s));
        env->gate->last = env->raster_done;
    }
    return launch("k_select", k_select, dim3(c.E), dim3(WAVE), 0, s, c, 0);
}

static int task_features(bridges_env* env, void* stream, int mode) {
    if (env->family.family != BRIDGES_FAMILY_NONE && env->family_thr)
        return launch("k_task_features (weighted task family)", k_task_features<bridges_task_family, const uint64_t*>, dim3(env->ctx.E),
                      dim3(TASK_THREADS), 0, stream, env->ctx, env->tasks, mode, env->family, env->family_thr);
    if (env->family.family != BRIDGES_FAMILY_NONE)
        return launch("k_task_features (task family)", k_task_features<bridges_task_family>, dim3(env->ctx.E), dim3(TASK_THREADS), 0,
                      stream, env->ctx, env->tasks, mode, env->family);
    return launch("k_task_features", k_task_features<>, dim3(env->ctx.E), dim3(TASK_THREADS), 0, stream, env->ctx, env->tasks, mode);
}

int bridges_env_reset(bridges_env* env, void* stream) {
    if (!env) return fail_arg("null env");
    if (int rc = launch("k_reset", k_reset, dim3(env->ctx.E), dim3(WAVE), 0, stream, env->ctx)) return rc;
    if (env->has_tasks)
        if (int rc = task_features(env, stream, TASK_RESET)) return rc;
    return refresh(env, (hipStream_t)stream, 0);
}

int bridges_env_step(bridges_env* env, void* stream) {
    if (!env) return fail_arg("null env");
    if (!env->has_tasks) {
        if (int rc = launch("k_step", k_step<>, dim3(env->ctx.E), dim3(WAVE), 0, stream, env->ctx)) return rc;
    } else {
        if (int rc = launch("k_step (per-env targets)", k_step<const double*>, dim3(env->ctx.E), dim3(WAVE), 0, stream, env->ctx,
                            (const double*)env->tasks.env_targets))
            return rc;
        // the envs k_step has just reset begin an episode: next task (fixed per-env targets and obstacles: nothing to do)
        if (env->tasks.sample || env->tasks.sample_obstacles || env->family.family != BRIDGES_FAMILY_NONE)
            if (int rc = task_features(env, stream, TASK_STEP)) return rc;
    }
    return refresh(env, (hipStream_t)stream, 1);
}

int bridges_env_set_task_buffers(bridges_env* env, const bridges_task_buffers* tb) {
    if (!env) return fail_arg("null env");
    DevCtx& c = env->ctx;
    if (!tb) {
        clear_family(env);
        env->has_tasks = false;
        memset(&env->tasks, 0, sizeof(env->tasks));
        c.b.reward_map = env->fixed_reward_map;
        c.b.reward_prefix = env->fixed_reward_prefix;
        return BRIDGES_OK;
    }
    if (!tb->env_targets || !tb->target_bits || !tb->reward_map || !tb->reward_prefix || !tb->task_episode || !tb->gauss_k)
        return fail_arg("task buffers: env_targets / target_bits / reward_map / reward_prefix / task_episode / gauss_k not given");
    if (tb->n_obstacles < 0 || tb->n_obstacles > BRIDGES_MAX_OBSTACLES) return fail_arg("task buffers: n_obstacles must be 0..BRIDGES_MAX_OBSTACLES");
    if (tb->env_obstacle_bits && tb->n_obstacles == 0) return fail_arg("task buffers: env_obstacle_bits given but n_obstacles is 0");
    if (tb->n_obstacles > 0 && !tb->env_obstacle_bits) return fail_arg("task buffers: n_obstacles > 0 but env_obstacle_bits not given");
    if (tb->n_obstacles > 0 && !tb->env_obstacles) return fail_arg("task buffers: n_obstacles > 0 but env_obstacles not given");
    if (tb->n_obstacles == 0 && tb->env_obstacles) return fail_arg("task buffers: env_obstacles given but n_obstacles is 0");
    if (tb->sample_obstacles != 0 && tb->sample_obstacles != 1) return fail_arg("task buffers: sample_obstacles must be 0 or 1");
    if (tb->sample_obstacles && tb->n_obstacles == 0) return fail_arg("task buffers: sample_obstacles needs n_obstacles > 0");
    if (tb->sample_obstacles)
        for (int o = 0; o < tb->n_obstacles; ++o)
            if (!(tb->obs_x_range[o][0] <= tb->obs_x_range[o][1] && tb->obs_z_range[o][0] <= tb->obs_z_range[o][1]))
                return fail_arg("task buffers: obs_x_range / obs_z_range");
    if (c.n_targets < 1) return fail_arg("task buffers: the task has no targets");
    if (tb->target_shape < 0 || tb->target_shape >= c.n_shapes) return fail_arg("task buffers: target_shape");
    if (tb->sample != 0 && tb->sample != 1) return fail_arg("task buffers: sample must be 0 or 1");
    if (tb->sample && !(tb->x_range[0] <= tb->x_range[1] && tb->z_range[0] <= tb->z_range[1])) return fail_arg("task buffers: x_range / z_range");
    env->tasks = *tb;
    clear_family(env);      // a family belongs to the buffers it was set on
    env->has_tasks = true;
    c.b.reward_map = tb->reward_map;
    c.b.reward_prefix = tb->reward_prefix;
    return BRIDGES_OK;
}

int bridges_env_set_task_family(bridges_env* env, const bridges_task_family* fam) {
    if (!env) return fail_arg("null env");
    if (!fam || fam->family == BRIDGES_FAMILY_NONE) {
        clear_family(env);
        return BRIDGES_OK;
    }
    if (fam->family != BRIDGES_FAMILY_SPAN && fam->family != BRIDGES_FAMILY_TOWER) return fail_arg("task family: family must be NONE, SPAN or TOWER");
    if (!env->has_tasks) return fail_arg("task family: no task buffers attached");
    if (env->ctx.n_targets != 1) return fail_arg("task family: the task must have n_targets == 1");
    if (fam->n_hi < 1 || fam->n_hi > BRIDGES_MAX_OBSTACLES) return fail_arg("task family: n_hi must be 1..BRIDGES_MAX_OBSTACLES");
    if (fam->n_lo < 0 || fam->n_lo > fam->n_hi) return fail_arg("task family: 0 <= n_lo <= n_hi");
    if (env->tasks.n_obstacles != fam->n_hi) return fail_arg("task family: the task buffers must have n_obstacles == n_hi");
    if (!(fam->size > 0.0)) return fail_arg("task family: size must be > 0");
    if (!fam->task_class) return fail_arg("task family: task_class not given");
    env->family = *fam;
    env->family_thr = nullptr;                         // a table belongs to the family it was set on
    return BRIDGES_OK;
}

int bridges_env_set_family_thresholds(bridges_env* env, const uint64_t* thr_dev) {
    if (!env) return fail_arg("null env");
    if (env->family.family == BRIDGES_FAMILY_NONE) return fail_arg("family thresholds: no task family set");
    env->family_thr = thr_dev;
    return BRIDGES_OK;
}

int bridges_env_load_targets(bridges_env* env, void* stream) {
    if (!env) return fail_arg("null env");
    if (!env->has_tasks) return fail_arg("bridges_env_load_targets: no task buffers attached");
    return task_features(env, stream, TASK_LOAD);
}

int bridges_env_refresh(bridges_env* env, void* stream) {
    if (!env) return fail_arg("null env");
    return refresh(env, (hipStream_t)stream, 0);
}

#define CS_TAB_SMALL 768     // 6 KiB: with carriers, candidates on up to ~4 placed blocks; 9.5 KB of LDS and <= 128 VGPRs per wave: 16 waves per CU
#define CS_COLS_SMALL 92     // its columns; the tableau / column / wave variants measured: profiles/r04_cs_variants.txt
#define CS_TAB_LARGE 4096
int bridges_env_candidate_stability(bridges_env* env, void* stream) {
    if (!env) return fail_arg("null env");
    const DevCtx& c = env->ctx;
    if (!c.b.cand_stable || !c.b.cand_queue || !c.b.cand_counters || !c.b.cand_ws) return fail_arg("cand_stable / cand_queue / cand_counters / cand_ws not given");
    if (c.b.cand_ws_stride < (int64_t)(3 * c.K + 2) * (4 * BRIDGES_MAX_INTERFACES + 3)) return fail_arg("cand_ws_stride");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(c.b.cand_counters, 0, 2 * sizeof(int32_t), s));
    // one wave per raw candidate (masked-out ones leave at once); grid from the last known candidate count, grid-stride beyond
    long long est = candidate_estimate(env);
    if (est > env->max_blocks) est = env->max_blocks;
    if (int rc = launch("k_candidate_stability", k_candidate_stability<CS_TAB_SMALL, CS_COLS_SMALL, false>, dim3((unsigned)est),
                        dim3(WAVE), 0, s, c))
        return rc;
    const int drain = BRIDGES_CAND_WS_SLOTS;          // one cand_ws slot per workgroup
    return launch("k_candidate_stability (queue)", k_candidate_stability<CS_TAB_LARGE, LP_MAX_COLS, true>, dim3(drain), dim3(WAVE),
                  0, s, c);
}

int bridges_env_restrict_to_stable(bridges_env* env, void* stream) {
    if (!env) return fail_arg("null env");
    if (int rc = bridges_env_candidate_stability(env, stream)) return rc;
    return launch("k_restrict_stable", k_restrict_stable, dim3(env->ctx.E), dim3(WAVE), 0, stream, env->ctx);
}

int bridges_env_rebuild_contacts(bridges_env* env, void* stream) {
    if (!env) return fail_arg("null env");
    return launch("k_rebuild_contacts", k_rebuild_contacts, dim3(env->ctx.E), dim3(WAVE), 0, stream, env->ctx);
}

// ---- bridges_env_fork ------------------------------------------------------------------------------------------------
// THE list of per-env state arrays a fork copies: (pointer, bytes per env).  A buffer added to bridges_env_buffers /
// bridges_task_buffers later is forked by adding one line here (and to FORK_* in bridges_hip/abi.py, which
// tests/test_cpu_beam.py holds against this list and against the buffer tables: a per-env buffer that is neither forked nor
// listed as excluded fails there).  A NULL pointer is an optional buffer that is not there: skipped.
static int fork_table(const bridges_env* env, ForkTable* T) {
    const DevCtx& c = env->ctx;
    const bridges_env_buffers& b = c.b;
    const bridges_task_buffers& t = env->tasks;              // all-zero (every pointer NULL) without per-env tasks
    const bridges_task_family& f = env->family;              // likewise without a family
    const int64_t K = c.K, NT = c.n_targets, NO = t.n_obstacles;
    struct Row { const void* p; int64_t bytes; };
#define FORK_ROW(ptr, bytes) {(const void*)(ptr), (int64_t)(bytes)}
    const Row rows[] = {
        FORK_ROW(b.n_blocks, 4),
        FORK_ROW(b.blk_shape, 4 * K),
        FORK_ROW(b.blk_pose, 8 * K * 4),
        FORK_ROW(b.blk_verts, 8 * K * MAXV * 2),
        FORK_ROW(b.blk_occ, K),
        FORK_ROW(b.targets_left, 4),
        FORK_ROW(b.state_bits, 8 * IMG),
        FORK_ROW(b.n_if, 4),
        FORK_ROW(b.if_body, 4 * MAXIF * 2),
        FORK_ROW(b.if_geom, 8 * MAXIF * 8),
        FORK_ROW(b.draw_counter, 8),
        FORK_ROW(b.needs_reset, 1),
        FORK_ROW(b.step_flags, 8),
        FORK_ROW(b.reward, 4),
        FORK_ROW(b.lin_reward, 4),
        FORK_ROW(b.n_reached, 4),
        FORK_ROW(b.n_cand, 4),
        FORK_ROW(b.lp_ws, 8 * b.lp_ws_stride),
        FORK_ROW(b.lp_snap, 8 * b.lp_snap_stride),
        FORK_ROW(t.env_targets, 8 * NT * 3),
        FORK_ROW(t.target_bits, 8 * IMG),
        FORK_ROW(t.reward_map, 4 * IMG * IMG),
        FORK_ROW(t.reward_prefix, 8 * IMG * (IMG + 1)),
        FORK_ROW(t.task_episode, 4),
        FORK_ROW(t.env_obstacles, 8 * NO * 3),
        FORK_ROW(t.env_obstacle_bits, 8 * IMG),
        FORK_ROW(f.task_class, 4),
    };
#undef FORK_ROW
    static_assert(sizeof(rows) / sizeof(rows[0]) <= FORK_MAX_ARRAYS, "fork table too long");
    memset(T, 0, sizeof(*T));
    T->E = c.E;
    int64_t off = 0, blocks = 0;
    for (const Row& r : rows) {
        if (!r.p || r.bytes <= 0) continue;
        ForkArray& a = T->a[T->n++];
        a.base = (char*)r.p;
        a.row_bytes = r.bytes;
        a.scratch_off = off;
        int unit = 16;
        while (unit > 1 && ((((uintptr_t)r.p) | (uintptr_t)r.bytes) & (uintptr_t)(unit - 1))) unit >>= 1;
        a.unit = unit;
        if (r.bytes >= FORK_PIECE / 4) {                     // a long row: pieces of one env's row
            a.rows_per_block = 1;
            a.pieces_per_row = (int32_t)ceil_div(r.bytes, FORK_PIECE);
        } else {                                             // short rows: several envs per workgroup
            a.rows_per_block = (int32_t)(FORK_PIECE / 4 / r.bytes);
            a.pieces_per_row = 1;
        }
        a.block0 = (int32_t)blocks;
        blocks += a.rows_per_block == 1 ? (int64_t)c.E * a.pieces_per_row : ceil_div(c.E, a.rows_per_block);
        off += ceil_div((int64_t)c.E * r.bytes, 16) * 16;
        if (blocks > (int64_t)0x7fffffff) return fail_arg("bridges_env_fork: too many workgroups");
    }
    T->scratch_bytes = off;
    T->n_blocks = (int32_t)blocks;
    return BRIDGES_OK;
}

int bridges_env_fork_scratch(const bridges_env* env, int64_t* bytes) {
    if (!env || !bytes) return fail_arg("bridges_env_fork_scratch: null");
    ForkTable T;
    if (int rc = fork_table(env, &T)) return rc;
    *bytes = T.scratch_bytes;
    return BRIDGES_OK;
}

int bridges_env_fork(bridges_env* env, const int32_t* src, void* scratch, int64_t scratch_bytes, void* stream) {
    if (!env || !src || !scratch) return fail_arg("bridges_env_fork: null env, src or scratch");
    if (!aligned(4, src) || !aligned(16, (const char*)scratch)) return fail_arg("bridges_env_fork: src must be 4-byte, scratch 16-byte aligned");
    ForkTable T;
    if (int rc = fork_table(env, &T)) return rc;
    if (scratch_bytes < T.scratch_bytes) return fail_arg("bridges_env_fork: scratch_bytes below bridges_env_fork_scratch's answer");
    if (T.n_blocks == 0) return BRIDGES_OK;
    if (int rc = launch("k_fork_rows (gather)", k_fork_rows<true>, dim3((unsigned)T.n_blocks), dim3(FORK_THREADS), 0, stream, T, src,
                        (char*)scratch))
        return rc;
    return launch("k_fork_rows (write back)", k_fork_rows<false>, dim3((unsigned)T.n_blocks), dim3(FORK_THREADS), 0, stream, T, src,
                  (char*)scratch);
}

int bridges_env_select_random(bridges_env* env, void* stream) {
    if (!env) return fail_arg("null env");
    return launch("k_select", k_select, dim3(env->ctx.E), dim3(WAVE), 0, stream, env->ctx, 1);
}

int bridges_env_lockstep_random(bridges_env* env, void* stream) {
    if (int rc = bridges_env_select_random(env, stream)) return rc;
    return bridges_env_step(env, stream);
}

int bridges_shapes_upload(const bridges_shape* host, int32_t n, bridges_shape** out_dev) {
    if (!host || n <= 0 || !out_dev) return fail_arg("shapes_upload");
    HIP_TRY(hipMalloc((void**)out_dev, sizeof(bridges_shape) * n));
    HIP_TRY(hipMemcpy(*out_dev, host, sizeof(bridges_shape) * n, hipMemcpyHostToDevice));
    return BRIDGES_OK;
}

int bridges_shapes_free(bridges_shape* dev) {
    if (dev) HIP_TRY(hipFree(dev));
    return BRIDGES_OK;
}

int bridges_place(const bridges_shape* shapes_dev, int32_t n, const double* frame1, const int32_t* shape_id,
                  const int32_t* face, const double* ox, const double* oy, double* pose, double* verts, void* stream) {
    if (n < 0 || !shapes_dev) return fail_arg("bridges_place");
    if (n == 0) return BRIDGES_OK;
    if (!frame1 || !shape_id || !face || !ox || !oy || !pose || !verts) return fail_arg("bridges_place: NULL array with n > 0");
    return launch("k_place", k_place, dim3(ceil_div(n, 256)), dim3(256), 0, stream, shapes_dev, n, frame1, shape_id, face, ox, oy,
                  pose, verts);
}

int bridges_create_block(const bridges_shape* shapes_dev, int32_t n, const double* target_verts,
                         const int32_t* target_shape, const int32_t* target_face, const int32_t* shape_id,
                         const int32_t* face, const double* ox, const double* oy, double* pose, double* verts,
                         double* target_frame_out, void* stream) {
    if (n < 0 || !shapes_dev) return fail_arg("bridges_create_block");
    if (n == 0) return BRIDGES_OK;
    // target_verts / target_shape are read only for items with target_face >= 0, which the host cannot see
    if (!target_face || !shape_id || !face || !ox || !oy || !pose || !verts)
        return fail_arg("bridges_create_block: NULL array with n > 0");
    return launch("k_create_block", k_create_block, dim3(ceil_div(n, 256)), dim3(256), 0, stream, shapes_dev, n, target_verts,
                  target_shape, target_face, shape_id, face, ox, oy, pose, verts, target_frame_out);
}

int bridges_pose_block(const bridges_shape* shapes_dev, int32_t n, const int32_t* shape_id, const double* pose,
                       double* verts, void* stream) {
    if (n < 0 || !shapes_dev) return fail_arg("bridges_pose_block");
    if (n == 0) return BRIDGES_OK;
    if (!shape_id || !pose || !verts) return fail_arg("bridges_pose_block: NULL array with n > 0");
    return launch("k_pose_block", k_pose_block, dim3(ceil_div(n, 256)), dim3(256), 0, stream, shapes_dev, n, shape_id, pose, verts);
}

int bridges_face_frames(const bridges_shape* shapes_dev, int32_t n, const int32_t* shape_id, const double* verts,
                        double* frames, void* stream) {
    if (n < 0 || !shapes_dev) return fail_arg("bridges_face_frames");
    if (n == 0) return BRIDGES_OK;
    if (!shape_id || !verts || !frames) return fail_arg("bridges_face_frames: NULL array with n > 0");
    return launch("k_face_frames", k_face_frames, dim3(ceil_div(n, 256)), dim3(256), 0, stream, shapes_dev, n, shape_id, verts, frames);
}

int bridges_contains_points(const bridges_shape* shapes_dev, int32_t shape_id, const double* verts, int32_t n,
                            const double* points, uint8_t* inside, void* stream) {
    if (n < 0 || !shapes_dev) return fail_arg("bridges_contains_points");
    if (n == 0) return BRIDGES_OK;
    if (shape_id < 0) return fail_arg("bridges_contains_points: shape_id < 0");
    if (!verts || !points || !inside) return fail_arg("bridges_contains_points: NULL array with n > 0");
    return launch("k_contains_points", k_contains_points, dim3(ceil_div(n, 256)), dim3(256), 0, stream, shapes_dev, shape_id, verts,
                  n, points, inside);
}

int bridges_render_blocks(const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                          const double* grid_x, int32_t W, const double* grid_y, int32_t H, uint8_t* out, void* stream) {
    if (!shapes_dev || n < 0 || W < 1 || H < 1 || !grid_x || !grid_y || !out || (n > 0 && (!verts || !shape_id)))
        return fail_arg("bridges_render_blocks");
    const int64_t px = (int64_t)W * H;
    return launch("k_render_blocks", k_render_blocks, dim3((unsigned)ceil_div(px, 256)), dim3(256), 0, stream, shapes_dev, n, verts,
                  shape_id, grid_x, W, grid_y, H, out);
}

// bridges_raster_sized and bridges_raster; `who` is the entry point an argument error names
static int raster_sized(const char* who, const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                        const double* grid_x, const double* grid_y, int32_t size, uint64_t* bits, float* img, void* stream) {
    if (n < 0 || !shapes_dev) return fail_arg(who);
    if (size < 2 || size > IMG) return fail_arg(who, "image size must be 2..64");
    if (n == 0) return BRIDGES_OK;
    if (!verts || !shape_id || !grid_x || !grid_y) return fail_arg(who, "NULL array with n > 0");     // bits / img: either may be NULL
    return launch("k_raster_generic", k_raster_generic, dim3(grid_for_waves(n)), dim3(256), 0, stream, shapes_dev, n, verts, shape_id,
                  grid_x, grid_y, (int)size, bits, img);
}

int bridges_raster_sized(const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                         const double* grid_x, const double* grid_y, int32_t size, uint64_t* bits, float* img,
                         void* stream) {
    return raster_sized("bridges_raster_sized", shapes_dev, n, verts, shape_id, grid_x, grid_y, size, bits, img, stream);
}

int bridges_raster(const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                   const double* grid_x, const double* grid_y, uint64_t* bits, float* img, void* stream) {
    return raster_sized("bridges_raster", shapes_dev, n, verts, shape_id, grid_x, grid_y, IMG, bits, img, stream);
}

int bridges_action_features(const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                            const double* grid_x, const double* grid_y, int32_t size, double xlim0, double xlim1, double ylim0,
                            double ylim1, const uint64_t* state_bits, const uint64_t* obstacle_bits, const double* reward_prefix,
                            uint64_t* bits, float* img, uint8_t* mask, float* lin_reward, void* stream) {
    if (n < 0 || !shapes_dev || !verts || !shape_id || !grid_x || !grid_y) return fail_arg("bridges_action_features");
    if (size < 2 || size > IMG) return fail_arg("bridges_action_features: image size must be 2..64");
    if (lin_reward && !reward_prefix) return fail_arg("bridges_action_features: lin_reward needs reward_prefix");
    if (n == 0) return BRIDGES_OK;
    return launch("k_action_features", k_action_features, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, stream, shapes_dev, n, verts,
                  shape_id, grid_x, grid_y, (int)size, xlim0, xlim1, ylim0, ylim1, state_bits, obstacle_bits, reward_prefix, bits, img,
                  mask, lin_reward);
}

int bridges_bits_or(int32_t n_groups, const int32_t* ranges, const uint64_t* bits, uint64_t* out, void* stream) {
    if (n_groups < 0 || (n_groups > 0 && (!ranges || !bits || !out))) return fail_arg("bridges_bits_or");
    if (n_groups == 0) return BRIDGES_OK;
    return launch("k_bits_or", k_bits_or, dim3(n_groups), dim3(WAVE), 0, stream, n_groups, ranges, bits, out);
}

int bridges_bits_to_f32(int32_t n, const uint64_t* bits, float* img, void* stream) {
    if (n < 0 || (n > 0 && (!bits || !img))) return fail_arg("bridges_bits_to_f32");
    if (n == 0) return BRIDGES_OK;
    // one short-lived wave per image, dispatched in image order (the store structure of k_raster)
    return launch("k_bits_to_f32", k_bits_to_f32, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, stream, n, bits, img);
}

int bridges_conv_input_rows(int32_t n_rows, const uint64_t* block_bits, const int64_t* block_row, const uint64_t* action_bits,
                            const int64_t* action_row, const float* reward, const int64_t* reward_row, int64_t reward_stride,
                            const uint64_t* obstacle_bits, const int64_t* obstacle_row, int64_t obstacle_stride, float* x,
                            void* stream) {
    if (n_rows < 0 || !block_bits || !action_bits || !reward || !obstacle_bits || !x) return fail_arg("bridges_conv_input_rows");
    if (reward_stride != 0 && reward_stride != IMG * IMG) return fail_arg("conv_input_rows: reward_stride must be 0 or 4096");
    if (obstacle_stride != 0 && obstacle_stride != IMG) return fail_arg("conv_input_rows: obstacle_stride must be 0 or 64");
    if (!aligned(16, reward, x)) return fail_arg("conv_input_rows: reward and x must be 16-byte aligned");
    if (n_rows == 0) return BRIDGES_OK;
    // one short-lived wave per (row, channel) image, a workgroup per row, dispatched in row order (the store structure of
    // k_raster)
    return launch("k_conv_input", k_conv_input, dim3((unsigned)n_rows), dim3(256), 0, stream, n_rows, block_bits, block_row, action_bits,
                  action_row, reward, reward_row, reward_stride, obstacle_bits, obstacle_row, obstacle_stride, x);
}

static int stability_launch(const bridges_shape* shapes_dev, int32_t n, int32_t K, const double* pose, const double* verts,
                            const int32_t* shape_id, const int32_t* n_blocks, const uint32_t* fixed_mask, double mu,
                            double density, double floor_half_width, double floor_depth, uint8_t* stable, double* info,
                            double* lp_ws, int64_t lp_ws_stride, double tension_tol, double* forces, void* stream) {
    if (n < 0 || !shapes_dev) return fail_arg("bridges_stability");
    if (K <= 0 || K > BRIDGES_MAX_BLOCKS) return fail_arg("K > BRIDGES_MAX_BLOCKS");
    if (lp_ws_stride < 9 * BRIDGES_MAX_INTERFACES + (int64_t)(3 * K + 2) * (4 * BRIDGES_MAX_INTERFACES + 3))
        return fail_arg("lp_ws_stride");
    if (n == 0) return BRIDGES_OK;
    return launch("k_stability", k_stability, dim3(n), dim3(WAVE), 0, stream, shapes_dev, n, K, pose, verts, shape_id, n_blocks,
                  fixed_mask, mu, density, floor_half_width, floor_depth, stable, info, lp_ws, lp_ws_stride, tension_tol, forces);
}

int bridges_stability(const bridges_shape* shapes_dev, int32_t n, int32_t K, const double* pose, const double* verts,
                      const int32_t* shape_id, const int32_t* n_blocks, const uint32_t* fixed_mask, double mu,
                      double density, double floor_half_width, double floor_depth, uint8_t* stable, double* info,
                      double* lp_ws, int64_t lp_ws_stride, void* stream) {
    return stability_launch(shapes_dev, n, K, pose, verts, shape_id, n_blocks, fixed_mask, mu, density, floor_half_width,
                            floor_depth, stable, info, lp_ws, lp_ws_stride, 0.0, nullptr, stream);
}

int bridges_stability_penalty(const bridges_shape* shapes_dev, int32_t n, int32_t K, const double* pose, const double* verts,
                              const int32_t* shape_id, const int32_t* n_blocks, const uint32_t* fixed_mask, double mu,
                              double density, double floor_half_width, double floor_depth, double tension_tol,
                              uint8_t* stable, double* info, double* forces, double* lp_ws, int64_t lp_ws_stride,
                              void* stream) {
    if (!(tension_tol >= 0.0)) return fail_arg("tension_tol");
    return stability_launch(shapes_dev, n, K, pose, verts, shape_id, n_blocks, fixed_mask, mu, density, floor_half_width,
                            floor_depth, stable, info, lp_ws, lp_ws_stride, tension_tol, forces, stream);
}

int bridges_soft_update(float* target, const float* policy, int64_t n, float tau, float one_minus_tau, void* stream) {
    if (n < 0) return fail_arg("bridges_soft_update");
    if (n == 0) return BRIDGES_OK;
    if (!aligned(16, target, policy)) return fail_arg("soft_update pointers must be 16-byte aligned");
    return launch("k_soft_update", k_soft_update, dim3((int)clamp_grid(ceil_div(n >> 2, 256), 2048)), dim3(256), 0, stream, target,
                  policy, n, tau, one_minus_tau);
}

// The one launch behind the three TD-target entry points (their checks differ, the kernel does not): per-row discounts when
// `discount` is given, the scalar gamma otherwise.
static int td_target_launch(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* select_q, const float* next_q,
                            const float* next_sf, int64_t next_sf_row_stride, const float* action_raster, const float* lin_reward,
                            const uint8_t* done, const float* discount, float gamma, int32_t sf_dim, float* q_target,
                            float* sf_target, int32_t* argmax_row, void* stream) {
    return launch(discount ? "k_td_target<rows>" : "k_td_target", discount ? k_td_target<true> : k_td_target<false>, dim3(n_trans),
                  dim3(256), 0, stream, n_trans, seg_lo, seg_hi, select_q, next_q, next_sf, next_sf_row_stride, action_raster,
                  lin_reward, done, discount, gamma, sf_dim, q_target, sf_target, argmax_row);
}

int bridges_td_target(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* next_q, const float* next_sf,
                      int64_t next_sf_row_stride, const float* action_raster, const float* lin_reward,
                      const uint8_t* done, float gamma, int32_t sf_dim, float* q_target, float* sf_target,
                      int32_t* argmax_row, void* stream) {
    if (n_trans < 0 || sf_dim < 0 || (n_trans > 0 && (!seg_lo || !seg_hi))) return fail_arg("bridges_td_target");
    if (n_trans == 0) return BRIDGES_OK;
    if (sf_dim > 0 && ((next_sf_row_stride & 3) || (sf_dim & 3) || !aligned(16, next_sf, action_raster, sf_target)))
        return fail_arg("td_target: sf rows must be 16-byte aligned");
    return td_target_launch(n_trans, seg_lo, seg_hi, next_q, next_q, next_sf, next_sf_row_stride, action_raster, lin_reward, done,
                            nullptr, gamma, sf_dim, q_target, sf_target, argmax_row, stream);
}

int bridges_td_target_rows(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* next_q, const float* next_sf,
                           int64_t next_sf_row_stride, const float* action_raster, const float* lin_reward,
                           const uint8_t* done, const float* discount, int32_t sf_dim, float* q_target, float* sf_target,
                           int32_t* argmax_row, void* stream) {
    if (n_trans < 0 || sf_dim < 0 || (n_trans > 0 && (!seg_lo || !seg_hi || !discount))) return fail_arg("bridges_td_target_rows");
    if (n_trans == 0) return BRIDGES_OK;
    if (sf_dim > 0 && ((next_sf_row_stride & 3) || (sf_dim & 3) || !aligned(16, next_sf, action_raster, sf_target)))
        return fail_arg("td_target_rows: sf rows must be 16-byte aligned");
    return td_target_launch(n_trans, seg_lo, seg_hi, next_q, next_q, next_sf, next_sf_row_stride, action_raster, lin_reward, done,
                            discount, 0.f, sf_dim, q_target, sf_target, argmax_row, stream);
}

int bridges_td_target_select(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* select_q, const float* next_q,
                             const float* next_sf, int64_t next_sf_row_stride, const float* action_raster, const float* lin_reward,
                             const uint8_t* done, const float* discount, float gamma, int32_t sf_dim, float* q_target,
                             float* sf_target, int32_t* argmax_row, void* stream) {
    if (n_trans < 0 || sf_dim < 0) return fail_arg("bridges_td_target_select: negative count");
    if (n_trans == 0) return BRIDGES_OK;
    if (!seg_lo || !seg_hi || !select_q || !next_q || !lin_reward || !done || !q_target || !argmax_row)
        return fail_arg("bridges_td_target_select: null pointer");
    if (sf_dim > 0 && (!next_sf || !action_raster || !sf_target || next_sf_row_stride < 0))
        return fail_arg("bridges_td_target_select: sf_dim > 0 needs next_sf, action_raster and sf_target");
    if (!aligned(4, seg_lo, seg_hi, select_q, next_q, next_sf, action_raster, lin_reward, discount, q_target, sf_target, argmax_row))
        return fail_arg("bridges_td_target_select: misaligned pointer");
    // (sf rows that are not 16-byte aligned, or an sf_dim that is no multiple of 4, take the kernel's element-wise epilogue)
    return td_target_launch(n_trans, seg_lo, seg_hi, select_q, next_q, next_sf, next_sf_row_stride, action_raster, lin_reward, done,
                            discount, gamma, sf_dim, q_target, sf_target, argmax_row, stream);
}

int bridges_soft_expect(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* select_q, const float* next_q,
                        float temperature, const float* feat, int64_t feat_row_stride, const int64_t* feat_row, int32_t dim,
                        float* value, float* feat_mean, float* entropy, int32_t* argmax_row, void* stream) {
    if (n_trans < 0 || dim < 0) return fail_arg("bridges_soft_expect: negative count");
    if (!(temperature > 0.f && temperature < INFINITY))                           // (a NaN fails the comparison)
        return fail_arg("bridges_soft_expect: the temperature must be finite and > 0");
    if (feat_row_stride < 0) return fail_arg("bridges_soft_expect: negative row stride");
    if (!aligned(4, seg_lo, seg_hi, argmax_row) || !aligned(4, select_q, next_q, feat, value, feat_mean, entropy) || !aligned(8, feat_row))
        return fail_arg("bridges_soft_expect: misaligned pointer");
    if (n_trans == 0) return BRIDGES_OK;
    if (!seg_lo || !seg_hi || !select_q || !next_q || !value || !argmax_row) return fail_arg("bridges_soft_expect: null pointer");
    if (dim > 0 && (!feat || !feat_mean)) return fail_arg("bridges_soft_expect: dim > 0 needs feat and feat_mean");
    // one workgroup per (transition, tile of SOFT_TILE columns); dim == 0 still needs tile 0 for value / entropy / argmax_row
    const unsigned tiles = dim > 0 ? (unsigned)ceil_div(dim, SOFT_TILE) : 1u;
    return launch("k_soft_expect", k_soft_expect, dim3((unsigned)n_trans, tiles), dim3(256), 0, stream, n_trans, seg_lo, seg_hi,
                  select_q, next_q, temperature, feat, feat_row_stride, feat_row, (int)dim, value, feat_mean, entropy, argmax_row);
}

int bridges_soft_expect_rel(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* select_q, const float* next_q,
                            float temperature, float spread_floor, const float* feat, int64_t feat_row_stride, const int64_t* feat_row,
                            int32_t dim, float* value, float* feat_mean, float* entropy, int32_t* argmax_row, double* temp_out,
                            void* stream) {
    if (n_trans < 0 || dim < 0) return fail_arg("bridges_soft_expect_rel: negative count");
    if (!(temperature > 0.f && temperature < INFINITY))                           // (a NaN fails the comparison)
        return fail_arg("bridges_soft_expect_rel: the temperature must be finite and > 0");
    if (!(spread_floor > 0.f && spread_floor < INFINITY))
        return fail_arg("bridges_soft_expect_rel: the spread floor must be finite and > 0");
    if (feat_row_stride < 0) return fail_arg("bridges_soft_expect_rel: negative row stride");
    if (!aligned(4, seg_lo, seg_hi, argmax_row) || !aligned(4, select_q, next_q, feat, value, feat_mean, entropy) || !aligned(8, feat_row))
        return fail_arg("bridges_soft_expect_rel: misaligned pointer");
    if (!aligned(8, temp_out)) return fail_arg("bridges_soft_expect_rel: temp_out must be 8-byte aligned");
    if (n_trans == 0) return BRIDGES_OK;
    if (!seg_lo || !seg_hi || !select_q || !next_q || !value || !argmax_row || !temp_out) return fail_arg("bridges_soft_expect_rel: null pointer");
    if (dim > 0 && (!feat || !feat_mean)) return fail_arg("bridges_soft_expect_rel: dim > 0 needs feat and feat_mean");
    // bridges_soft_expect's grid
    const unsigned tiles = dim > 0 ? (unsigned)ceil_div(dim, SOFT_TILE) : 1u;
    return launch("k_soft_expect_rel", k_soft_expect_rel, dim3((unsigned)n_trans, tiles), dim3(256), 0, stream, n_trans, seg_lo, seg_hi,
                  select_q, next_q, temperature, spread_floor, feat, feat_row_stride, feat_row, (int)dim, value, feat_mean, entropy,
                  argmax_row, temp_out);
}

// What bridges_soft_value and bridges_soft_value_rel refuse alike (bridges_soft_expect's refusals, then their own).
static int soft_value_check(const char* who, int32_t n, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, float temperature,
                            const int32_t* taken_row, float alpha, float clip_lo, const float* value, const float* tlogp,
                            const float* bonus, const uint8_t* miss) {
    if (n < 0) return fail_arg(who, "negative count");
    if (!(temperature > 0.f && temperature < INFINITY))                           // (a NaN fails the comparison)
        return fail_arg(who, "the temperature must be finite and > 0");
    if (!(alpha >= 0.f && alpha <= 1.f)) return fail_arg(who, "alpha must lie in [0, 1]");
    if (!(clip_lo <= 0.f && clip_lo > -INFINITY)) return fail_arg(who, "clip_lo must be finite and <= 0");
    if (!aligned(4, seg_lo, seg_hi, taken_row) || !aligned(4, q, value, tlogp, bonus)) return fail_arg(who, "misaligned pointer");
    if (n == 0) return BRIDGES_OK;
    if (!seg_lo || !seg_hi || !q || !value) return fail_arg(who, "null pointer");
    if (taken_row && (!tlogp || !bonus || !miss)) return fail_arg(who, "taken_row needs tlogp, bonus and miss");
    return BRIDGES_OK;
}

int bridges_soft_value(int32_t n, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, float temperature,
                       const int32_t* taken_row, float alpha, float clip_lo, float* value, float* tlogp, float* bonus, uint8_t* miss,
                       void* stream) {
    if (int rc = soft_value_check("bridges_soft_value", n, seg_lo, seg_hi, q, temperature, taken_row, alpha, clip_lo, value, tlogp,
                                  bonus, miss))
        return rc;
    if (n == 0) return BRIDGES_OK;
    // one wave per segment, four segments per workgroup
    return launch("k_soft_value", k_soft_value, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, stream, (int)n, seg_lo, seg_hi, q,
                  temperature, taken_row, alpha, clip_lo, value, tlogp, bonus, miss);
}

int bridges_soft_value_rel(int32_t n, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, float temperature,
                           float spread_floor, const int32_t* taken_row, float alpha, float clip_lo, float* value, float* tlogp,
                           float* bonus, uint8_t* miss, double* temp_out, void* stream) {
    if (int rc = soft_value_check("bridges_soft_value_rel", n, seg_lo, seg_hi, q, temperature, taken_row, alpha, clip_lo, value,
                                  tlogp, bonus, miss))
        return rc;
    if (!(spread_floor > 0.f && spread_floor < INFINITY))
        return fail_arg("bridges_soft_value_rel: the spread floor must be finite and > 0");
    if (!aligned(8, temp_out)) return fail_arg("bridges_soft_value_rel: temp_out must be 8-byte aligned");
    if (n == 0) return BRIDGES_OK;
    if (!temp_out) return fail_arg("bridges_soft_value_rel: null pointer");
    // bridges_soft_value's grid
    return launch("k_soft_value_rel", k_soft_value_rel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, stream, (int)n, seg_lo, seg_hi,
                  q, temperature, spread_floor, taken_row, alpha, clip_lo, value, tlogp, bonus, miss, temp_out);
}

int bridges_action_row(int32_t n, const int32_t* seg_lo, const int32_t* seg_hi, const int64_t* idx, const int32_t* cand_desc,
                       const double* cand_pose, const double* rec, int64_t rec_stride, int32_t* row, void* stream) {
    if (n < 0) return fail_arg("bridges_action_row: negative count");
    if (rec_stride < BRIDGES_REC_WIDTH) return fail_arg("bridges_action_row: a record has at least BRIDGES_REC_WIDTH columns");
    if (!seg_lo || !seg_hi || !idx || !cand_desc || !cand_pose || !rec || !row) return fail_arg("bridges_action_row: null pointer");
    if (!aligned(4, seg_lo, seg_hi, row) || !aligned(8, idx) || !aligned(8, cand_pose, rec) || !aligned(16, cand_desc))
        return fail_arg("bridges_action_row: misaligned pointer");
    if (n == 0) return BRIDGES_OK;
    // one wave per transition, four per workgroup
    return launch("k_action_row", k_action_row, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, stream, (int)n, seg_lo, seg_hi, idx,
                  cand_desc, cand_pose, rec, rec_stride, row);
}

int bridges_nstep_fold(int32_t E, int32_t W, int32_t n, const double* rec, const uint8_t* valid, double gamma, int32_t* count,
                       double* acc, double* disc, double* stable_s, double* td, double* out, uint8_t* out_valid, void* stream) {
    if (E < 0 || n < 1 || n > BRIDGES_NSTEP_MAX) return fail_arg("bridges_nstep_fold: n must be 1..BRIDGES_NSTEP_MAX");
    if (W < BRIDGES_REC_WIDTH) return fail_arg("bridges_nstep_fold: a record has at least BRIDGES_REC_WIDTH columns");
    if (!rec || !valid || !count || !acc || !disc || !stable_s || !td || !out || !out_valid) return fail_arg("bridges_nstep_fold");
    if (!aligned(8, rec, acc, disc, stable_s, td, out) || !aligned(4, count))
        return fail_arg("bridges_nstep_fold: misaligned pointer");
    if (E == 0) return BRIDGES_OK;
    // one wave per env, four envs per workgroup
    return launch("k_nstep_fold", k_nstep_fold, dim3((unsigned)ceil_div(E, 4)), dim3(256), 0, stream, (int)E, (int)W, (int)n, rec, valid,
                  gamma, count, acc, disc, stable_s, td, out, out_valid);
}

int bridges_priority_sample_scratch(int64_t n_rec, int64_t* doubles) {
    if (!doubles || n_rec < 0 || n_rec > BRIDGES_PRIORITY_MAX_ROWS) return fail_arg("bridges_priority_sample_scratch");
    const int64_t chunks = ceil_div(n_rec, PRIO_CHUNK);
    *doubles = chunks * PRIO_CHUNK + 2 * chunks;          // the masses of whole chunks, the chunk sums, their prefix sums
    return BRIDGES_OK;
}

int bridges_priority_sample(int64_t n_rec, int32_t W, int32_t col, const double* rec, double alpha, int64_t n_draws, const double* u,
                            int64_t* idx, double* scratch, int64_t scratch_doubles, void* stream) {
    if (n_draws < 0) return fail_arg("bridges_priority_sample: negative count");
    if (n_draws == 0) return BRIDGES_OK;
    if (n_rec <= 0 || n_rec > BRIDGES_PRIORITY_MAX_ROWS) return fail_arg("bridges_priority_sample: n_rec must be 1..BRIDGES_PRIORITY_MAX_ROWS");
    if (col < 0 || W <= col) return fail_arg("bridges_priority_sample: the column lies outside the record");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail_arg("bridges_priority_sample: alpha must lie in [0, 1]");
    if (!rec || !u || !idx || !scratch) return fail_arg("bridges_priority_sample: null pointer");
    if (!aligned(8, rec, u, idx, scratch)) return fail_arg("bridges_priority_sample: misaligned pointer");
    int64_t need = 0;
    if (int rc = bridges_priority_sample_scratch(n_rec, &need)) return rc;
    if (scratch_doubles < need) return fail_arg("bridges_priority_sample: scratch too small (bridges_priority_sample_scratch)");
    const int chunks = (int)ceil_div(n_rec, PRIO_CHUNK);
    double* mass = scratch;
    double* chunk_sum = mass + (int64_t)chunks * PRIO_CHUNK;
    double* chunk_cdf = chunk_sum + chunks;
    const int mode = alpha == 0.0 ? 0 : (alpha == 1.0 ? 1 : 2);
    if (int rc = launch("k_priority_mass", k_priority_mass, dim3((unsigned)chunks), dim3(PRIO_CHUNK), 0, stream, n_rec, (int)W, (int)col, rec,
                        alpha, mode, mass, chunk_sum))
        return rc;
    if (int rc = launch("k_priority_scan", k_priority_scan, dim3(1), dim3(256), 0, stream, chunks, (const double*)chunk_sum, chunk_cdf))
        return rc;
    // one wave per draw, four draws per workgroup
    return launch("k_priority_draw", k_priority_draw, dim3((unsigned)ceil_div(n_draws, 4)), dim3(256), 0, stream, n_rec, chunks,
                  (const double*)mass, (const double*)chunk_cdf, n_draws, u, idx);
}

int bridges_hindsight_relabel_scratch(int32_t E, int32_t G, int64_t* bytes) {
    if (!bytes || E < 0 || G < 1 || G > HIND_MAX_GOALS) return fail_arg("bridges_hindsight_relabel_scratch");
    *bytes = (int64_t)sizeof(int32_t) * (E > 0 ? (int64_t)E * G : 1);         // the rows of every (env, slot), then their offsets
    return BRIDGES_OK;
}

int bridges_hindsight_per_step_scratch(int32_t E, int32_t G, int64_t* bytes) {
    if (!bytes || E < 0 || G < 1 || G > HIND_MAX_GOALS) return fail_arg("bridges_hindsight_per_step_scratch");
    *bytes = 2 * (int64_t)sizeof(int32_t) * (E > 0 ? (int64_t)E * G : 1);     // the rows of every (env, slot) (then their offsets), the masks
    return BRIDGES_OK;
}

// What the four hindsight entries check and launch: fold = false stores the one-step rows [., W], fold = true the h-step rows
// [., W + 1]; per_step = false the goals of the final structure, one set per slot, per_step = true one set per step.
static int hindsight_relabel(bool per_step, bool fold, int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                             const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed, int32_t env_id_base,
                             const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape, const double* grid_x,
                             const double* grid_y, int32_t img, const float* gauss_k, int32_t n_step, double gamma, double* out,
                             int32_t* count, void* scratch, int64_t scratch_bytes, void* stream) {
    if (E < 0) return fail_arg("bridges_hindsight_relabel: negative count");
    if (G < 1 || G > HIND_MAX_GOALS) return fail_arg("bridges_hindsight_relabel: G must be 1..4");
    if (K < 1 || K > BRIDGES_MAX_BLOCKS) return fail_arg("bridges_hindsight_relabel: K must be 1..BRIDGES_MAX_BLOCKS");
    if (T < 1 || T > BRIDGES_MAX_TARGETS) return fail_arg("bridges_hindsight_relabel: T must be 1..BRIDGES_MAX_TARGETS");
    if (W < BRIDGES_REC_WIDTH + 3 * T) return fail_arg("bridges_hindsight_relabel: a record ends in its 3 T target values");
    if (n_shapes < 1 || n_shapes > 8 || target_shape < 0 || target_shape >= n_shapes) return fail_arg("bridges_hindsight_relabel: shape table");
    if (img < 1 || img > IMG) return fail_arg("bridges_hindsight_relabel: img must be 1..64");
    if ((int64_t)E * G * K > INT32_MAX) return fail_arg("bridges_hindsight_relabel: more rows than an int32 counts");
    if (fold && (n_step < 1 || n_step > BRIDGES_NSTEP_MAX))
        return fail_arg("bridges_hindsight_relabel_nstep: n_step must be 1..BRIDGES_NSTEP_MAX");
    if (fold && !(gamma - gamma == 0.0)) return fail_arg("bridges_hindsight_relabel_nstep: gamma must be finite");
    if (!buf || !flags || !len || !ended || !episode || !shapes_dev || !grid_x || !grid_y || !gauss_k || !out || !count || !scratch)
        return fail_arg("bridges_hindsight_relabel: null pointer");
    if (!aligned(8, buf, shapes_dev, grid_x, grid_y, out) || !aligned(4, len, episode, gauss_k, count, scratch))
        return fail_arg("bridges_hindsight_relabel: misaligned pointer");
    int64_t need = 0;
    if (int rc = per_step ? bridges_hindsight_per_step_scratch(E, G, &need) : bridges_hindsight_relabel_scratch(E, G, &need)) return rc;
    if (scratch_bytes < need)
        return fail_arg(per_step ? "bridges_hindsight_per_step: scratch too small (bridges_hindsight_per_step_scratch)"
                                 : "bridges_hindsight_relabel: scratch too small (bridges_hindsight_relabel_scratch)");
    if (E == 0) return BRIDGES_OK;
    HindArgs a;
    a.buf = buf; a.flags = flags; a.len = len; a.ended = ended; a.episode = episode; a.shapes = shapes_dev; a.grid_x = grid_x;
    a.grid_y = grid_y; a.gauss_k = gauss_k; a.seed = seed; a.E = E; a.K = K; a.W = W; a.T = T; a.G = G; a.env_id_base = env_id_base;
    a.n_shapes = n_shapes; a.target_shape = target_shape; a.img = img;
    int32_t* cnt = (int32_t*)scratch;
    const int items = E * G;
    if (per_step) {
        // the count and the step mask of every (env, slot): one wave each, four per workgroup; the rows: one workgroup per
        // (env, slot, step), E * G * K <= INT32_MAX of them
        uint32_t* mask = (uint32_t*)(cnt + items);
        const unsigned wgs = (unsigned)items * (unsigned)K;
        if (int rc = launch("k_hindsight_step_count", k_hindsight_step_count, dim3((unsigned)ceil_div(items, 4)), dim3(256), 0, stream, a, cnt,
                            mask))
            return rc;
        if (int rc = launch("k_hindsight_scan", k_hindsight_scan, dim3(1), dim3(HIND_SCAN_THREADS), 0, stream, items, cnt, count)) return rc;
        if (fold)
            return launch("k_hindsight_step_rows_nstep", k_hindsight_step_rows_nstep, dim3(wgs), dim3(TASK_THREADS), 0, stream, a,
                          (const int32_t*)cnt, (const uint32_t*)mask, out, (int)n_step, gamma);
        return launch("k_hindsight_step_rows", k_hindsight_step_rows, dim3(wgs), dim3(TASK_THREADS), 0, stream, a, (const int32_t*)cnt,
                      (const uint32_t*)mask, out);
    }
    // one wave per (env, slot), four per workgroup
    if (int rc = launch("k_hindsight_count", k_hindsight_count, dim3((unsigned)ceil_div(items, 4)), dim3(256), 0, stream, a, cnt)) return rc;
    if (int rc = launch("k_hindsight_scan", k_hindsight_scan, dim3(1), dim3(HIND_SCAN_THREADS), 0, stream, items, cnt, count)) return rc;
    if (fold)
        return launch("k_hindsight_rows_nstep", k_hindsight_rows_nstep, dim3((unsigned)items), dim3(TASK_THREADS), 0, stream, a,
                      (const int32_t*)cnt, (const int32_t*)count, out, (int)n_step, gamma);
    return launch("k_hindsight_rows", k_hindsight_rows, dim3((unsigned)items), dim3(TASK_THREADS), 0, stream, a, (const int32_t*)cnt,
                  (const int32_t*)count, out);
}

int bridges_hindsight_relabel(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                              const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed, int32_t env_id_base,
                              const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape, const double* grid_x,
                              const double* grid_y, int32_t img, const float* gauss_k, double* out, int32_t* count, void* scratch,
                              int64_t scratch_bytes, void* stream) {
    return hindsight_relabel(false, false, E, K, W, T, G, buf, flags, len, ended, episode, seed, env_id_base, shapes_dev, n_shapes, target_shape,
                                    grid_x, grid_y, img, gauss_k, 1, 0.0, out, count, scratch, scratch_bytes, stream);
}

int bridges_hindsight_relabel_nstep(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                                    const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed,
                                    int32_t env_id_base, const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape,
                                    const double* grid_x, const double* grid_y, int32_t img, const float* gauss_k, int32_t n_step,
                                    double gamma, double* out, int32_t* count, void* scratch, int64_t scratch_bytes, void* stream) {
    return hindsight_relabel(false, true, E, K, W, T, G, buf, flags, len, ended, episode, seed, env_id_base, shapes_dev, n_shapes, target_shape,
                                   grid_x, grid_y, img, gauss_k, n_step, gamma, out, count, scratch, scratch_bytes, stream);
}

int bridges_hindsight_per_step(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                               const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed, int32_t env_id_base,
                               const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape, const double* grid_x,
                               const double* grid_y, int32_t img, const float* gauss_k, double* out, int32_t* count, void* scratch,
                               int64_t scratch_bytes, void* stream) {
    return hindsight_relabel(true, false, E, K, W, T, G, buf, flags, len, ended, episode, seed, env_id_base, shapes_dev, n_shapes,
                             target_shape, grid_x, grid_y, img, gauss_k, 1, 0.0, out, count, scratch, scratch_bytes, stream);
}

int bridges_hindsight_per_step_nstep(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                                     const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed,
                                     int32_t env_id_base, const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape,
                                     const double* grid_x, const double* grid_y, int32_t img, const float* gauss_k, int32_t n_step,
                                     double gamma, double* out, int32_t* count, void* scratch, int64_t scratch_bytes, void* stream) {
    return hindsight_relabel(true, true, E, K, W, T, G, buf, flags, len, ended, episode, seed, env_id_base, shapes_dev, n_shapes,
                             target_shape, grid_x, grid_y, img, gauss_k, n_step, gamma, out, count, scratch, scratch_bytes, stream);
}

int bridges_priority_update(int64_t n_rec, int32_t W, int32_t col, double* rec, int64_t n, const int64_t* idx, const float* q_sa,
                            const float* q_target, void* stream) {
    if (n < 0 || n_rec < 0) return fail_arg("bridges_priority_update: negative count");
    if (col < 0 || W <= col) return fail_arg("bridges_priority_update: the column lies outside the record");
    if (n == 0) return BRIDGES_OK;
    if (n > BRIDGES_PRIORITY_MAX_UPDATES) return fail_arg("bridges_priority_update: n > BRIDGES_PRIORITY_MAX_UPDATES");
    if (!rec || !idx || !q_sa || !q_target) return fail_arg("bridges_priority_update: null pointer");
    if (!aligned(8, rec, idx) || !aligned(4, q_sa, q_target)) return fail_arg("bridges_priority_update: misaligned pointer");
    return launch("k_priority_update", k_priority_update, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, stream, n_rec, (int)W, (int)col,
                  rec, n, idx, q_sa, q_target);
}

int bridges_priority_weights(int64_t n_rec, int64_t n_draws, int64_t batch, const int64_t* idx, double beta, const double* scratch,
                             int64_t scratch_doubles, float* weight, void* stream) {
    if (n_draws < 0) return fail_arg("bridges_priority_weights: negative count");
    if (n_draws == 0) return BRIDGES_OK;
    if (n_rec <= 0 || n_rec > BRIDGES_PRIORITY_MAX_ROWS) return fail_arg("bridges_priority_weights: n_rec must be 1..BRIDGES_PRIORITY_MAX_ROWS");
    if (batch <= 0 || batch > INT32_MAX || n_draws % batch != 0) return fail_arg("bridges_priority_weights: n_draws must be a multiple of batch >= 1");
    if (n_draws / batch > INT32_MAX) return fail_arg("bridges_priority_weights: more batches than a grid holds");
    if (!(beta >= 0.0 && beta <= 1.0)) return fail_arg("bridges_priority_weights: beta must lie in [0, 1]");
    if (!idx || !scratch || !weight) return fail_arg("bridges_priority_weights: null pointer");
    if (!aligned(8, idx, scratch) || !aligned(4, weight)) return fail_arg("bridges_priority_weights: misaligned pointer");
    int64_t need = 0;
    if (int rc = bridges_priority_sample_scratch(n_rec, &need)) return rc;
    if (scratch_doubles < need) return fail_arg("bridges_priority_weights: scratch too small (bridges_priority_sample_scratch)");
    const int mode = beta == 0.0 ? 0 : (beta == 1.0 ? 1 : 2);
    // one workgroup per batch; the masses are the first chunks * PRIO_CHUNK doubles of the sampler's scratch
    return launch("k_priority_weights", k_priority_weights, dim3((unsigned)(n_draws / batch)), dim3(256), 0, stream, n_rec, (int)batch, idx,
                  scratch, beta, mode, weight);
}

int bridges_bits_discounted_sum(int32_t n, const uint64_t* bits, int64_t n_rows, const int64_t* first, const int32_t* h, float gamma,
                                float* sum, float* disc, void* stream) {
    if (n < 0 || n_rows < 0 || (n > 0 && (!bits || !first || !h || !disc))) return fail_arg("bridges_bits_discounted_sum");
    if (!aligned(16, sum) || !aligned(8, bits, first) || !aligned(4, h, disc))
        return fail_arg("bits_discounted_sum: misaligned pointer (sum: 16 bytes)");
    if (n == 0) return BRIDGES_OK;
    // one short-lived wave per transition, dispatched in transition order (the store structure of k_raster)
    return launch("k_bits_discounted_sum", k_bits_discounted_sum, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, stream, (int)n, bits,
                  n_rows, first, h, gamma, sum, disc);
}

int bridges_bits_linear(int32_t n_rows, const uint64_t* bits, const int64_t* bits_row, const float* wt, int32_t d,
                        const float* base, const int64_t* base_row, float* out, void* stream) {
    if (n_rows < 0 || d <= 0 || (d & 3) || !bits || !wt || !out) return fail_arg("bridges_bits_linear");
    if (!aligned(16, wt, out, base)) return fail_arg("bits_linear: rows must be 16-byte aligned");
    if (n_rows == 0) return BRIDGES_OK;
    return launch("k_bits_linear", k_bits_linear, dim3(grid_for_waves(n_rows)), dim3(256), 0, stream, n_rows, bits, bits_row, wt, d,
                  base, base_row, out);
}

int bridges_bits_linear2(int32_t n_rows, const uint64_t* bits_a, const int64_t* bits_row_a, const float* wt_a, const uint64_t* bits_b,
                         const int64_t* bits_row_b, const float* wt_b, int32_t d, const float* base, const int64_t* base_row,
                         float* out, void* stream) {
    if (n_rows < 0 || d <= 0 || (d & 3) || !bits_a || !wt_a || !bits_b || !wt_b || !out) return fail_arg("bridges_bits_linear2");
    if (!aligned(16, wt_a, wt_b, out, base)) return fail_arg("bits_linear2: rows must be 16-byte aligned");
    if (n_rows == 0) return BRIDGES_OK;
    return launch("k_bits_linear2", k_bits_linear2, dim3(grid_for_waves(n_rows)), dim3(256), 0, stream, n_rows, bits_a, bits_row_a, wt_a,
                  bits_b, bits_row_b, wt_b, d, base, base_row, out);
}

int bridges_eps_greedy_select(int32_t E, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, const float* join,
                              const float* u, float eps, int32_t greedy, const int64_t* idx, const int32_t* cand_offset,
                              const int32_t* rep, int64_t* sel_compact, int32_t* sel_index, float* q_sel, float* explore_w, void* stream) {
    if (E < 1 || n_rows < 1 || !seg_lo || !seg_hi || !q || !join || !u || !idx || !cand_offset || !sel_compact || !sel_index || !q_sel || !explore_w)
        return fail_arg("bridges_eps_greedy_select");
    return launch("k_eps_greedy_select", k_eps_greedy_select, dim3((unsigned)ceil_div(E, 4)), dim3(256), 0, stream, E, n_rows, seg_lo,
                  seg_hi, q, join, u, eps, (int)greedy, idx, cand_offset, rep, sel_compact, sel_index, q_sel, explore_w);
}

int bridges_boltzmann_select(int32_t E, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, const float* u,
                             float temperature, int32_t greedy, const int64_t* idx, const int32_t* cand_offset, const int32_t* rep,
                             int64_t* sel_compact, int32_t* sel_index, float* q_sel, float* explore_w, float* p_sel, void* stream) {
    if (E < 0) return fail_arg("bridges_boltzmann_select: negative count");
    if (E == 0) return BRIDGES_OK;
    if (n_rows < 1) return fail_arg("bridges_boltzmann_select: n_rows must be >= 1");
    if (!(temperature > 0.f && temperature < INFINITY))                           // (a NaN fails the comparison)
        return fail_arg("bridges_boltzmann_select: the temperature must be finite and > 0");
    if (!seg_lo || !seg_hi || !q || !u || !idx || !cand_offset || !sel_compact || !sel_index || !q_sel || !explore_w || !p_sel)
        return fail_arg("bridges_boltzmann_select: null pointer");
    // one wave per env, four envs per workgroup
    return launch("k_boltzmann_select", k_boltzmann_select, dim3((unsigned)ceil_div(E, 4)), dim3(256), 0, stream, E, n_rows, seg_lo,
                  seg_hi, q, u, temperature, (int)greedy, idx, cand_offset, rep, sel_compact, sel_index, q_sel, explore_w, p_sel);
}

int bridges_boltzmann_select_rel(int32_t E, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, const float* u,
                                 float temperature, float spread_floor, int32_t greedy, const int64_t* idx, const int32_t* cand_offset,
                                 const int32_t* rep, int64_t* sel_compact, int32_t* sel_index, float* q_sel, float* explore_w,
                                 float* p_sel, double* temp_out, void* stream) {
    if (E < 0) return fail_arg("bridges_boltzmann_select_rel: negative count");
    if (E == 0) return BRIDGES_OK;
    if (n_rows < 1) return fail_arg("bridges_boltzmann_select_rel: n_rows must be >= 1");
    if (!(temperature > 0.f && temperature < INFINITY))                           // (a NaN fails the comparison)
        return fail_arg("bridges_boltzmann_select_rel: the temperature must be finite and > 0");
    if (!(spread_floor > 0.f && spread_floor < INFINITY))
        return fail_arg("bridges_boltzmann_select_rel: the spread floor must be finite and > 0");
    if (!seg_lo || !seg_hi || !q || !u || !idx || !cand_offset || !sel_compact || !sel_index || !q_sel || !explore_w || !p_sel)
        return fail_arg("bridges_boltzmann_select_rel: null pointer");
    if (!temp_out || !aligned(8, temp_out)) return fail_arg("bridges_boltzmann_select_rel: temp_out must be an 8-byte aligned array");
    // bridges_boltzmann_select's grid
    return launch("k_boltzmann_select_rel", k_boltzmann_select_rel, dim3((unsigned)ceil_div(E, 4)), dim3(256), 0, stream, E, n_rows,
                  seg_lo, seg_hi, q, u, temperature, spread_floor, (int)greedy, idx, cand_offset, rep, sel_compact, sel_index, q_sel,
                  explore_w, p_sel, temp_out);
}

int bridges_beam_select(int32_t E, int32_t B, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q,
                        const int64_t* idx, const int32_t* cand_offset, const int32_t* rep, const uint8_t* live, const double* ret,
                        const double* disc, int32_t* src, int64_t* sel_compact, int32_t* sel_index, float* q_sel, double* score,
                        uint8_t* live_out, void* stream) {
    if (E < 0) return fail_arg("bridges_beam_select: negative count");
    if (B < 1 || B > BEAM_MAX_WIDTH) return fail_arg("bridges_beam_select: the width must be 1..16");
    if (E % B != 0) return fail_arg("bridges_beam_select: E must be a multiple of the width");
    if (E == 0) return BRIDGES_OK;
    if (n_rows < 1) return fail_arg("bridges_beam_select: n_rows must be >= 1");
    if (!seg_lo || !seg_hi || !q || !idx || !cand_offset || !live || !ret || !disc || !src || !sel_compact || !sel_index || !q_sel ||
        !score || !live_out)
        return fail_arg("bridges_beam_select: null pointer");
    if (!aligned(4, seg_lo, seg_hi, cand_offset, rep, src, sel_index) || !aligned(4, q, q_sel) || !aligned(8, idx, sel_compact) ||
        !aligned(8, ret, disc, score))
        return fail_arg("bridges_beam_select: misaligned pointer");
    // one workgroup per group of B beams
    return launch("k_beam_select", k_beam_select, dim3((unsigned)(E / B)), dim3(BEAM_THREADS), 0, stream, E, B, n_rows, seg_lo, seg_hi, q,
                  idx, cand_offset, rep, live, ret, disc, src, sel_compact, sel_index, q_sel, score, live_out);
}

int bridges_particle_select(int32_t E, int32_t B, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q,
                            const int64_t* idx, const int32_t* cand_offset, const int32_t* rep, const uint8_t* live, const double* ret,
                            const double* disc, const float* u_act, const float* u_res, float temperature,
                            float resample_temperature, int32_t elite, int32_t* src, int64_t* sel_compact, int32_t* sel_index,
                            float* q_sel, double* score, uint8_t* live_out, float* p_sel, double* ess, void* stream) {
    if (E < 0) return fail_arg("bridges_particle_select: negative count");
    if (B < 1 || B > BEAM_MAX_WIDTH) return fail_arg("bridges_particle_select: the width must be 1..16");
    if (E % B != 0) return fail_arg("bridges_particle_select: E must be a multiple of the width");
    if (E == 0) return BRIDGES_OK;
    if (n_rows < 1) return fail_arg("bridges_particle_select: n_rows must be >= 1");
    if (!(temperature > 0.f && temperature < INFINITY))                           // (a NaN fails the comparison)
        return fail_arg("bridges_particle_select: the temperature must be finite and > 0");
    if (!(resample_temperature > 0.f)) return fail_arg("bridges_particle_select: the resampling temperature must be > 0 (+inf allowed)");
    if (!seg_lo || !seg_hi || !q || !idx || !cand_offset || !live || !ret || !disc || !u_act || !u_res || !src || !sel_compact ||
        !sel_index || !q_sel || !score || !live_out || !p_sel || !ess)
        return fail_arg("bridges_particle_select: null pointer");
    if (!aligned(4, seg_lo, seg_hi, cand_offset, rep, src, sel_index) || !aligned(4, q, q_sel, u_act, u_res, p_sel) ||
        !aligned(8, idx, sel_compact) || !aligned(8, ret, disc, score, ess))
        return fail_arg("bridges_particle_select: misaligned pointer");
    // one workgroup per group of B particles
    return launch("k_particle_select", k_particle_select, dim3((unsigned)(E / B)), dim3(BEAM_THREADS), 0, stream, E, B, n_rows, seg_lo,
                  seg_hi, q, idx, cand_offset, rep, live, ret, disc, u_act, u_res, temperature, resample_temperature, (int)elite, src,
                  sel_compact, sel_index, q_sel, score, live_out, p_sel, ess);
}

int bridges_beam_merge(int32_t E, int32_t B, int32_t K, const int32_t* n_blocks, const int32_t* blk_shape, const double* blk_pose,
                       const uint8_t* blk_occ, const int32_t* targets_left, const uint8_t* live, const double* ret, int32_t key_last,
                       int32_t* rep, uint8_t* live_out, int32_t* n_merged, void* stream) {
    if (E < 0) return fail_arg("bridges_beam_merge: negative count");
    if (B < 1 || B > BEAM_MAX_WIDTH) return fail_arg("bridges_beam_merge: the width must be 1..16");
    if (E % B != 0) return fail_arg("bridges_beam_merge: E must be a multiple of the width");
    if (K < 1 || K > BEAM_MAX_SLOTS) return fail_arg("bridges_beam_merge: K must be 1..64");
    if (E == 0) return BRIDGES_OK;
    if (!n_blocks || !blk_shape || !blk_pose || !blk_occ || !targets_left || !live || !ret || !rep || !live_out || !n_merged)
        return fail_arg("bridges_beam_merge: null pointer");
    if (!aligned(4, n_blocks, blk_shape, targets_left, rep, n_merged) || !aligned(8, blk_pose, ret))
        return fail_arg("bridges_beam_merge: misaligned pointer");
    // one workgroup per group of B beams
    return launch("k_beam_merge", k_beam_merge, dim3((unsigned)(E / B)), dim3(BEAM_THREADS), 0, stream, E, B, K, n_blocks, blk_shape,
                  blk_pose, blk_occ, targets_left, live, ret, (int)key_last, rep, live_out, n_merged);
}

int bridges_beam_trace(int32_t E, int32_t B, int32_t D, int32_t n_step, int32_t n_tail, const double* rec, const uint8_t* valid,
                       const int32_t* parent, const int32_t* end_env, const int32_t* end_depth, const double* tail, double gamma,
                       double priority, double* out, int32_t* offset, int32_t* status, void* stream) {
    if (E < 0) return fail_arg("bridges_beam_trace: negative count");
    if (B < 1 || B > BEAM_MAX_WIDTH) return fail_arg("bridges_beam_trace: the width must be 1..16");
    if (E % B != 0) return fail_arg("bridges_beam_trace: E must be a multiple of the width");
    if (D < 1 || D > BRIDGES_REC_K) return fail_arg("bridges_beam_trace: D must be 1..BRIDGES_REC_K");
    if (n_step < 1 || n_step > BRIDGES_NSTEP_MAX) return fail_arg("bridges_beam_trace: n_step must be 1..BRIDGES_NSTEP_MAX");
    if (n_tail < 0) return fail_arg("bridges_beam_trace: negative tail width");
    if (!(gamma - gamma == 0.0)) return fail_arg("bridges_beam_trace: gamma must be finite");
    if (!rec || !valid || !parent || !end_env || !end_depth || !out || !offset || !status || (n_tail > 0 && !tail))
        return fail_arg("bridges_beam_trace: null pointer");
    if (!aligned(8, rec, tail, out) || !aligned(4, parent, end_env, end_depth, offset, status))
        return fail_arg("bridges_beam_trace: misaligned pointer");
    if (E == 0) return BRIDGES_OK;
    BeamTraceArgs a;
    a.rec = rec; a.valid = valid; a.parent = parent; a.end_env = end_env; a.end_depth = end_depth; a.tail = n_tail > 0 ? tail : nullptr;
    a.gamma = gamma; a.priority = priority; a.E = E; a.B = B; a.D = D; a.n_step = n_step; a.n_tail = n_tail;
    // one workgroup per group of B beams, twice: the chains are checked, then the rows of the intact ones are written
    const dim3 grid((unsigned)(E / B));
    if (int rc = launch("k_beam_trace_check", k_beam_trace_check, grid, dim3(BEAM_THREADS), 0, stream, a, status)) return rc;
    return launch("k_beam_trace_rows", k_beam_trace_rows, grid, dim3(BEAM_THREADS), 0, stream, a, (const int32_t*)status, out, offset);
}

int bridges_record_state(int32_t E, int32_t K, const int32_t* n_blocks, const int32_t* blk_shape, const double* blk_pose,
                         const uint8_t* blk_occ, const uint8_t* step_flags, const int64_t* sel_row, const int32_t* cand_desc,
                         const double* cand_pose, double* rec, void* stream) {
    if (E < 0 || K < 1 || K > BRIDGES_REC_K || !n_blocks || !blk_shape || !blk_pose || !blk_occ || !step_flags || !sel_row ||
        !cand_desc || !cand_pose || !rec)
        return fail_arg("bridges_record_state");
    if (E == 0) return BRIDGES_OK;
    return launch("k_record_state", k_record_state, dim3((unsigned)E), dim3(64), 0, stream, E, K, n_blocks, blk_shape, blk_pose,
                  blk_occ, step_flags, sel_row, cand_desc, cand_pose, rec);
}

int bridges_record_result(int32_t E, const float* reward, const float* lin_reward, const uint8_t* step_flags, double* rec,
                          uint8_t* valid, void* stream) {
    if (E < 0 || !reward || !lin_reward || !step_flags || !rec || !valid) return fail_arg("bridges_record_result");
    if (E == 0) return BRIDGES_OK;
    return launch("k_record_result", k_record_result, dim3((unsigned)ceil_div(E, 256)), dim3(256), 0, stream, E, reward, lin_reward,
                  step_flags, rec, valid);
}

int bridges_episode_stats(int32_t E, int32_t K, const double* rec, const uint8_t* valid, const float* gpow, int32_t n_targets,
                          int32_t count_first_only, float* run, int32_t* counted, double* out, void* stream) {
    if (E < 0 || K < 1 || !gpow || !out || (E > 0 && (!rec || !valid || !run || !counted)))
        return fail_arg("bridges_episode_stats");
    if (E == 0) return BRIDGES_OK;
    return launch("k_episode_stats<1>", k_episode_stats<1>, dim3(1), dim3(EPISODE_STATS_THREADS), 0, stream, E, K, rec, valid, gpow,
                  (int)n_targets, (int)(count_first_only != 0), (const int32_t*)nullptr, 1, run, counted, out);
}

int bridges_episode_stats_by_class(int32_t E, int32_t K, const double* rec, const uint8_t* valid, const float* gpow,
                                   int32_t n_targets, int32_t count_first_only, const int32_t* cls, int32_t n_classes, float* run,
                                   int32_t* counted, double* out, void* stream) {
    if (E < 0 || K < 1 || !gpow || !out || (E > 0 && (!rec || !valid || !run || !counted || !cls)))
        return fail_arg("bridges_episode_stats_by_class");
    if (n_classes < 1 || n_classes > EPISODE_STATS_MAX_CLASSES) return fail_arg("bridges_episode_stats_by_class: n_classes must be 1..8");
    if (E == 0) return BRIDGES_OK;
    return launch("k_episode_stats<8>", k_episode_stats<EPISODE_STATS_MAX_CLASSES>, dim3(1), dim3(EPISODE_STATS_THREADS), 0, stream,
                  E, K, rec, valid, gpow, (int)n_targets, (int)(count_first_only != 0), cls, (int)n_classes, run, counted, out);
}

int bridges_family_thresholds(const uint32_t* w_dev, int32_t C, uint64_t* thr_dev, void* stream) {
    if (C < 1 || C > FAMILY_MAX_CLASSES) return fail_arg("bridges_family_thresholds: C must be 1..8");
    if (!w_dev || (C > 1 && !thr_dev)) return fail_arg("bridges_family_thresholds");
    if (C == 1) return BRIDGES_OK;                     // one class: the table has no entry
    return launch("k_family_thresholds", k_family_thresholds, dim3(1), dim3(WAVE), 0, stream, w_dev, (int)C, thr_dev);
}

int bridges_family_draw(uint64_t seed, int32_t env_id_base, int32_t E, const uint32_t* episode, int32_t n_lo, int32_t n_hi,
                        const uint64_t* thr, int32_t* n_out, void* stream) {
    if (E < 0 || (E > 0 && (!episode || !n_out))) return fail_arg("bridges_family_draw");
    if (n_lo < 0 || n_lo > n_hi || n_hi - n_lo + 1 > FAMILY_MAX_CLASSES) return fail_arg("bridges_family_draw: 0 <= n_lo <= n_hi, at most 8 classes");
    if (E == 0) return BRIDGES_OK;
    return launch("k_family_draw", k_family_draw, dim3((E + FAMILY_DRAW_THREADS - 1) / FAMILY_DRAW_THREADS), dim3(FAMILY_DRAW_THREADS), 0,
                  stream, seed, (int)env_id_base, (int)E, episode, (int)n_lo, (int)n_hi, thr, n_out);
}

int bridges_family_curriculum(double* sums, int32_t n_classes, double* state, int32_t n_lo, int32_t n_hi, double beta, uint32_t w_min,
                              int32_t min_episodes, uint32_t* w, uint64_t* thr, void* stream) {
    if (!sums || !state || !w) return fail_arg("bridges_family_curriculum");
    if (n_classes < 1 || n_classes > EPISODE_STATS_MAX_CLASSES) return fail_arg("bridges_family_curriculum: n_classes must be 1..8");
    if (n_lo < 0 || n_lo > n_hi || n_hi >= n_classes) return fail_arg("bridges_family_curriculum: 0 <= n_lo <= n_hi < n_classes");
    if (n_hi > n_lo && !thr) return fail_arg("bridges_family_curriculum: thr not given");
    if (!(beta >= 0.0 && beta <= 1.0)) return fail_arg("bridges_family_curriculum: beta must be in [0, 1]");
    if (w_min < 1 || w_min > FAMILY_MAX_WEIGHT - 65536u) return fail_arg("bridges_family_curriculum: w_min must be 1..2^20 - 2^16");
    if (min_episodes < 1) return fail_arg("bridges_family_curriculum: min_episodes must be >= 1");
    return launch("k_family_curriculum", k_family_curriculum, dim3(1), dim3(WAVE), 0, stream, sums, state, (int)n_lo, (int)n_hi, beta,
                  w_min, (int)min_episodes, w, thr);
}

int bridges_replay_unpack(int32_t E, int32_t n_rec, int32_t K, const double* rec, const int32_t* shape_faces, int32_t n_shapes,
                          int32_t n_groups, int32_t n_ground, int32_t n_off, int32_t* n_blocks, int32_t* blk_shape,
                          double* blk_pose, uint8_t* blk_occ, int32_t* n_cand, int32_t* ranges_next, int32_t* ranges_prev,
                          float* lin, float* stable_s, uint8_t* done, uint8_t* stable_n, void* stream) {
    if (E < 0 || n_rec < 1 || n_rec > E || K < 1 || K > BRIDGES_REC_K || !rec || !shape_faces || n_shapes < 1 || n_groups < 0 ||
        n_ground < 0 || n_off < 0 || !n_blocks || !blk_shape || !blk_pose || !blk_occ || !n_cand || !ranges_next ||
        !ranges_prev || !lin || !stable_s || !done || !stable_n)
        return fail_arg("bridges_replay_unpack");
    return launch("k_replay_unpack", k_replay_unpack, dim3((unsigned)E), dim3(64), 0, stream, E, n_rec, K, rec, shape_faces, n_shapes,
                  n_groups, n_ground, n_off, n_blocks, blk_shape, blk_pose, blk_occ, n_cand, ranges_next, ranges_prev, lin, stable_s,
                  done, stable_n);
}

int bridges_replay_unpack_prev(int32_t E, int32_t n_rec, int32_t K, const double* rec, const int32_t* shape_faces, int32_t n_shapes,
                          int32_t n_groups, int32_t n_ground, int32_t n_off, int32_t* n_blocks, int32_t* blk_shape,
                          double* blk_pose, uint8_t* blk_occ, int32_t* n_cand, int32_t* ranges_next, int32_t* ranges_prev,
                          float* lin, float* stable_s, uint8_t* done, uint8_t* stable_n, void* stream) {
    if (E < 0 || n_rec < 1 || n_rec > E || K < 1 || K > BRIDGES_REC_K || !rec || !shape_faces || n_shapes < 1 || n_groups < 0 ||
        n_ground < 0 || n_off < 0 || !n_blocks || !blk_shape || !blk_pose || !blk_occ || !n_cand || !ranges_next ||
        !ranges_prev || !lin || !stable_s || !done || !stable_n)
        return fail_arg("bridges_replay_unpack_prev");
    return launch("k_replay_unpack_prev", k_replay_unpack_prev, dim3((unsigned)E), dim3(64), 0, stream, E, n_rec, K, rec, shape_faces, n_shapes,
                  n_groups, n_ground, n_off, n_blocks, blk_shape, blk_pose, blk_occ, n_cand, ranges_next, ranges_prev, lin, stable_s,
                  done, stable_n);
}

int bridges_valid_rows(int32_t E, const int32_t* cand_offset, const int32_t* n_cand, const int32_t* n_valid, const uint8_t* cand_mask,
                       const int32_t* rep, int32_t* seg, int32_t* seg_lo, int32_t* seg_hi, int64_t* idx, int64_t* row_env,
                       int32_t* h_total, void* stream) {
    if (E < 1 || !cand_offset || !n_cand || !n_valid || !cand_mask || !seg || !idx || !row_env || !h_total || (rep && (!seg_lo || !seg_hi)) ||
        ((seg_lo == nullptr) != (seg_hi == nullptr)))
        return fail_arg("bridges_valid_rows");
    if (int rc = launch("k_valid_scan", k_valid_scan, dim3(1), dim3(1024), 0, stream, E, n_valid, rep, seg, h_total)) return rc;
    return launch("k_valid_fill", k_valid_fill, dim3((unsigned)ceil_div(E, 4)), dim3(256), 0, stream, E, cand_offset, n_cand, cand_mask,
                  (const int32_t*)seg, rep, seg_lo, seg_hi, idx, row_env);
}

int bridges_env_groups_keyed(int32_t E, int32_t K, const int32_t* n_blocks, const int32_t* blk_shape, const double* blk_pose,
                             const uint8_t* blk_occ, const uint8_t* flag, const uint64_t* extra, int32_t n_extra, uint64_t* hkey,
                             int32_t* rep, void* stream) {
    if (E < 1 || K < 1 || K > 64 || !n_blocks || !blk_shape || !blk_pose || !blk_occ || !hkey || !rep) return fail_arg("bridges_env_groups");
    if (n_extra < 0 || ((extra == nullptr) != (n_extra == 0))) return fail_arg("bridges_env_groups_keyed: extra / n_extra");
    const dim3 grid((unsigned)ceil_div(E, 4));
    if (!extra) {
        if (int rc = launch("k_env_hash", k_env_hash<false>, grid, dim3(256), 0, stream, E, K, n_blocks, blk_shape, blk_pose, blk_occ, flag,
                            extra, 0, hkey))
            return rc;
        return launch("k_env_match", k_env_match<false>, grid, dim3(256), 0, stream, E, K, n_blocks, blk_shape, blk_pose, blk_occ, flag,
                      extra, 0, (const uint64_t*)hkey, rep);
    }
    if (int rc = launch("k_env_hash<keyed>", k_env_hash<true>, grid, dim3(256), 0, stream, E, K, n_blocks, blk_shape, blk_pose, blk_occ,
                        flag, extra, (int)n_extra, hkey))
        return rc;
    return launch("k_env_match<keyed>", k_env_match<true>, grid, dim3(256), 0, stream, E, K, n_blocks, blk_shape, blk_pose, blk_occ, flag,
                  extra, (int)n_extra, (const uint64_t*)hkey, rep);
}

int bridges_env_groups(int32_t E, int32_t K, const int32_t* n_blocks, const int32_t* blk_shape, const double* blk_pose,
                       const uint8_t* blk_occ, const uint8_t* flag, uint64_t* hkey, int32_t* rep, void* stream) {
    return bridges_env_groups_keyed(E, K, n_blocks, blk_shape, blk_pose, blk_occ, flag, nullptr, 0, hkey, rep, stream);
}

// w_row == nullptr: one map w [N] for every row; else w [n_maps, N] and row r takes map w_row[r]
static int head_sigmoid_dot(int32_t n_rows, int32_t K, int32_t N, const float* h, int64_t h_stride, const float* Wd, const float* bd,
                            const float* w, const int32_t* w_row, int32_t n_maps, float* out, float* part, int32_t splits,
                            void* stream) {
    if (n_rows < 0 || N <= 0 || !h || !Wd || !bd || !w || !out || splits < 1 || (splits > 1 && !part))
        return fail_arg("bridges_head_sigmoid_dot");
    if (w_row && (n_maps < 1 || (int64_t)n_maps * N > INT32_MAX)) return fail_arg("bridges_head_sigmoid_dot_rows: n_maps");
    if (K != HEAD_K) return fail_arg("bridges_head_sigmoid_dot: the hidden width must be 256");
    if ((h_stride & 3) || h_stride < K || !aligned(16, h, Wd)) return fail_arg("bridges_head_sigmoid_dot: rows must be 16-byte aligned");
    if (n_rows == 0) return BRIDGES_OK;
    const int tiles = (N + HEAD_BN - 1) / HEAD_BN;
    const int per = (tiles + splits - 1) / splits;
    const int used = (tiles + per - 1) / per;                             // ranges that hold at least one tile
    const dim3 grid((unsigned)ceil_div(n_rows, 128), (unsigned)used);
    if (int rc = w_row ? launch("k_head_sigmoid_dot<rows>", k_head_sigmoid_dot<true>, grid, dim3(256), 0, stream, n_rows, N, h, h_stride, Wd,
                                bd, w, w_row, used > 1 ? part : out, per)
                       : launch("k_head_sigmoid_dot", k_head_sigmoid_dot<false>, grid, dim3(256), 0, stream, n_rows, N, h, h_stride, Wd,
                                bd, w, w_row, used > 1 ? part : out, per))
        return rc;
    if (used <= 1) return BRIDGES_OK;
    return launch("k_head_sum", k_head_sum, dim3((unsigned)ceil_div(n_rows, 256)), dim3(256), 0, stream, n_rows, used, part, out);
}

int bridges_head_sigmoid_dot(int32_t n_rows, int32_t K, int32_t N, const float* h, int64_t h_stride, const float* Wd,
                             const float* bd, const float* w, float* out, float* part, int32_t splits, void* stream) {
    return head_sigmoid_dot(n_rows, K, N, h, h_stride, Wd, bd, w, nullptr, 0, out, part, splits, stream);
}

int bridges_head_sigmoid_dot_rows(int32_t n_rows, int32_t K, int32_t N, const float* h, int64_t h_stride, const float* Wd,
                                  const float* bd, const float* w_all, const int32_t* w_row, int32_t n_maps, float* out, float* part,
                                  int32_t splits, void* stream) {
    if (!w_row) return fail_arg("bridges_head_sigmoid_dot_rows: w_row");
    return head_sigmoid_dot(n_rows, K, N, h, h_stride, Wd, bd, w_all, w_row, n_maps, out, part, splits, stream);
}

int bridges_bits_dot(int32_t n_rows, const uint64_t* bits, const int64_t* bits_row, const float* img, const int64_t* slot,
                     float* out, void* stream) {
    if (n_rows < 0 || !bits || !img || !slot || !out) return fail_arg("bridges_bits_dot");
    if (n_rows == 0) return BRIDGES_OK;
    return launch("k_bits_dot", k_bits_dot, dim3((unsigned)ceil_div(n_rows, 4)), dim3(256), 0, stream, n_rows, bits, bits_row, img, slot,
                  out);
}

int bridges_bits_accumulate(int32_t n_rows, const uint64_t* bits, const int64_t* bits_row, const float* weight,
                            const int64_t* slot, float* img, void* stream) {
    if (n_rows < 0 || !bits || !img || !slot) return fail_arg("bridges_bits_accumulate");
    if (n_rows == 0) return BRIDGES_OK;
    return launch("k_bits_accumulate", k_bits_accumulate, dim3((unsigned)ceil_div(n_rows, 4)), dim3(256), 0, stream, n_rows, bits,
                  bits_row, weight, slot, img);
}

int bridges_sigmoid_dot(int32_t n_rows, const float* d, int64_t row_stride, const float* w, int32_t k, float* out,
                        void* stream) {
    if (n_rows < 0 || k <= 0 || (k & 3) || (row_stride & 3) || !d || !w || !out) return fail_arg("bridges_sigmoid_dot");
    if (!aligned(16, d, w)) return fail_arg("sigmoid_dot: rows must be 16-byte aligned");
    if (n_rows == 0) return BRIDGES_OK;
    return launch("k_sigmoid_dot", k_sigmoid_dot<false>, dim3(grid_for_waves(n_rows)), dim3(256), 0, stream, n_rows, d, row_stride, w,
                  (const int32_t*)nullptr, k, out);
}

int bridges_sigmoid_dot_rows(int32_t n_rows, const float* d, int64_t row_stride, const float* w_all, const int32_t* w_row, int32_t k,
                             float* out, void* stream) {
    if (n_rows < 0 || k <= 0 || (k & 3) || (row_stride & 3) || !d || !w_all || !w_row || !out) return fail_arg("bridges_sigmoid_dot_rows");
    if (!aligned(16, d, w_all)) return fail_arg("sigmoid_dot: rows must be 16-byte aligned");
    if (n_rows == 0) return BRIDGES_OK;
    return launch("k_sigmoid_dot<rows>", k_sigmoid_dot<true>, dim3(grid_for_waves(n_rows)), dim3(256), 0, stream, n_rows, d, row_stride,
                  w_all, w_row, k, out);
}

int bridges_bias_relu(float* x, const float* bias, int64_t n, int32_t C, int32_t hw, void* stream) {
    if (n < 0 || C <= 0 || hw <= 0 || (hw & 3) || !x || !bias) return fail_arg("bridges_bias_relu");
    if (!aligned(16, x)) return fail_arg("bias_relu: x must be 16-byte aligned");
    if (n == 0) return BRIDGES_OK;
    const int64_t n4 = n * C * (hw >> 2);
    return launch("k_bias_relu", k_bias_relu, dim3((unsigned)clamp_grid(ceil_div(n4, 256), 16384)), dim3(256), 0, stream, x, bias, n4,
                  hw >> 2, C);
}

int bridges_bias_relu_pool2(const float* x, const float* bias, float* out, int64_t n, int32_t C, int32_t H, int32_t W,
                            void* stream) {
    if (n < 0 || C <= 0 || H <= 0 || W <= 0 || (W & 3) || (H & 1) || !x || !bias || !out) return fail_arg("bridges_bias_relu_pool2");
    if (!aligned(16, x) || !aligned(8, out)) return fail_arg("bias_relu_pool2: x must be 16-byte, out 8-byte aligned");
    if (n == 0) return BRIDGES_OK;
    const int64_t items = n * C * (H >> 1) * (W >> 2);
    return launch("k_bias_relu_pool2", k_bias_relu_pool2, dim3((unsigned)clamp_grid(ceil_div(items, 256), 16384)), dim3(256), 0, stream,
                  x, bias, out, items, H, W, C);
}

// ---- small-batch MLP training step (mlp_kernels.hip) ------------------------------------------------------------

int bridges_linear_forward(int32_t rows, int32_t K, int32_t N, const float* x, const float* W, const float* bias,
                           int32_t relu, float* y, float* ws, int64_t ws_floats, const int64_t* x_block, void* stream) {
    if (rows <= 0 || (rows & 31) || K <= 0 || N <= 0 || !x || !W || !bias || !y) return fail_arg("bridges_linear_forward: rows must be a positive multiple of 32");
    const int n_tiles = ceil_div(N, 32), m_tiles = rows / 32;
    // enough workgroups to fill the chip; a split holds at least 64 k values and its partial sums must fit in ws
    // (a short K or enough output tiles: one launch, no partial sums)
    int splits = (K <= 512 || n_tiles * m_tiles >= 128) ? 1 : ceil_div(512, n_tiles * m_tiles);
    const int max_by_k = ceil_div(K, 64);
    if (splits > max_by_k) splits = max_by_k;
    const int64_t per_split = (int64_t)rows * N;
    if (!ws || (int64_t)splits * per_split > ws_floats) splits = ws ? (int)(ws_floats / per_split) : 1;
    if (splits < 1) splits = 1;
    int kchunk = ceil_div(ceil_div(K, splits), 32) * 32;
    splits = ceil_div(K, kchunk);
    if (int rc = launch("k_lin_fwd", k_lin_fwd, dim3(n_tiles, splits, m_tiles), dim3(256), 0, stream, K, N, kchunk, x, W, bias, relu, y,
                        splits > 1 ? ws : (float*)nullptr, x_block))
        return rc;
    if (splits <= 1) return BRIDGES_OK;
    return launch("k_lin_fwd_finish", k_lin_fwd_finish, dim3(clamp_grid(ceil_div(rows * N, 256), 1024)), dim3(256), 0, stream, rows, N,
                  splits, ws, bias, relu, y);
}

static int linear_backward_impl(int32_t rows, int32_t K, int32_t N, const float* dz, const float* a_in, const float* W,
                                float* dW, float* db, const float* act_below, float* dz_below, float* ws, int64_t ws_floats,
                                const int64_t* a_block, int32_t a_block_bias, LossLog log, void* stream) {
    if (rows <= 0 || (rows & 31) || K <= 0 || N <= 0 || !dz || !a_in || !W || !dW || !db) return fail_arg("bridges_linear_backward: rows must be a positive multiple of 32");
    const int n_ntiles = ceil_div(N, 32), n_ktiles = ceil_div(K, 32), m_tiles = rows / 32;
    int per_job = ceil_div(n_ntiles * n_ktiles, 1024);           // k tiles per dW job: ~1024 jobs on the big layers
    if (per_job < 4) per_job = 4;                                 // one tile per wave at least
    const int n_dw_jobs = n_ntiles * ceil_div(n_ktiles, per_job);
    int nsplit = 0, nchunk = 0, n_dx_jobs = 0;
    if (dz_below) {
        if (!ws) return fail_arg("bridges_linear_backward: workspace needed for the input gradient");
        nsplit = (N <= 512) ? 1 : ceil_div(256, n_ktiles * m_tiles);
        const int max_by_n = ceil_div(N, 64);
        if (nsplit > max_by_n) nsplit = max_by_n;
        const int64_t per_split = (int64_t)rows * K;
        if ((int64_t)nsplit * per_split > ws_floats) nsplit = (int)(ws_floats / per_split);
        if (nsplit < 1) return fail_arg("bridges_linear_backward: workspace too small");
        nchunk = ceil_div(ceil_div(N, nsplit), 32) * 32;
        nsplit = ceil_div(N, nchunk);
        n_dx_jobs = n_ktiles * nsplit * m_tiles;
    }
    // one split: the input gradient goes straight to dz_below (masked), no partial sums
    if (int rc = launch("k_lin_bwd", k_lin_bwd<false>, dim3(n_dw_jobs + n_dx_jobs), dim3(256), 0, stream, rows, K, N, dz, a_in, W, dW,
                        db, !dz_below ? (float*)nullptr : (nsplit == 1 ? dz_below : ws), nsplit == 1 ? act_below : (const float*)nullptr,
                        n_dw_jobs, per_job, nsplit, nchunk, AdamFold{}, a_block, (int)a_block_bias, log))
        return rc;
    if (!dz_below || nsplit <= 1) return BRIDGES_OK;
    return launch("k_lin_dx_finish", k_lin_dx_finish, dim3(clamp_grid(ceil_div(rows * K, 256), 1024)), dim3(256), 0, stream, rows, K,
                  nsplit, ws, act_below, dz_below);
}

int bridges_linear_backward(int32_t rows, int32_t K, int32_t N, const float* dz, const float* a_in, const float* W,
                            float* dW, float* db, const float* act_below, float* dz_below, float* ws, int64_t ws_floats,
                            const int64_t* a_block, int32_t a_block_bias, void* stream) {
    return linear_backward_impl(rows, K, N, dz, a_in, W, dW, db, act_below, dz_below, ws, ws_floats, a_block, a_block_bias, LossLog{}, stream);
}

int bridges_linear_backward_log(int32_t rows, int32_t K, int32_t N, const float* dz, const float* a_in, const float* W,
                                float* dW, float* db, const float* act_below, float* dz_below, float* ws, int64_t ws_floats,
                                const float* loss_rows, int32_t batch, float* losses, int32_t n_losses, int64_t* counter,
                                float* adam_step, void* stream) {
    if (!loss_rows || batch <= 0 || batch > rows || !counter || (losses && n_losses <= 0)) return fail_arg("bridges_linear_backward_log");
    return linear_backward_impl(rows, K, N, dz, a_in, W, dW, db, act_below, dz_below, ws, ws_floats, nullptr, 0,
                                LossLog{loss_rows, (int)batch, losses, (int)n_losses, counter, adam_step}, stream);
}

// the middle stack the k_mid_* kernels are instantiated for: SuccessorMLP's 256-128-64-128-256 (successor_dqn.py:366)
static bool mid_dims_supported(int32_t n_layers, const int32_t* dims) {
    static const int32_t want[5] = {256, 128, 64, 128, 256};
    if (n_layers != 4 || !dims) return false;
    for (int i = 0; i < 5; ++i) if (dims[i] != want[i]) return false;
    return true;
}
static int mid_ptrs_fill(const char* who, MidPtrs& p, const float* const* W, const float* const* bias, float* const* dW,
                         float* const* db, float* const* acts, float* const* dz) {
    if (!W || !acts) return fail_arg(who);
    for (int l = 0; l < 4; ++l) {
        if (!W[l] || !aligned(16, W[l]) || (bias && !bias[l]) || (dW && !dW[l]) || (db && !db[l])) return fail_arg(who);
        p.W[l] = W[l]; p.bias[l] = bias ? bias[l] : nullptr; p.dW[l] = dW ? dW[l] : nullptr; p.db[l] = db ? db[l] : nullptr;
    }
    for (int l = 0; l < 5; ++l) {
        if (!acts[l] || !aligned(16, acts[l]) || (dz && (l == 0 || l == 4) && (!dz[l] || !aligned(16, dz[l])))) return fail_arg(who);
        p.act[l] = acts[l]; p.dz[l] = dz ? dz[l] : nullptr;
    }
    return BRIDGES_OK;
}

int bridges_mlp_mid_supported(int32_t rows, int32_t n_layers, const int32_t* dims) {
    return (rows == 32 && mid_dims_supported(n_layers, dims)) ? 1 : 0;
}

int bridges_mlp_mid_forward(int32_t rows, int32_t n_layers, const int32_t* dims, const float* const* W, const float* const* bias,
                            float* const* acts, void* stream) {
    if (rows != 32 || !mid_dims_supported(n_layers, dims) || !bias) return fail_arg("bridges_mlp_mid_forward: 32 rows of 256-128-64-128-256 only");
    MidPtrs p{};
    if (int rc = mid_ptrs_fill("bridges_mlp_mid_forward", p, W, bias, nullptr, nullptr, acts, nullptr)) return rc;
    return launch("k_mid_fwd", k_mid_fwd<256, 128, 64, 128, 256>, dim3(256 / 32), dim3(1024), 0, stream, p);
}

int bridges_mlp_mid_rows(int32_t n_rows, int32_t n_layers, const int32_t* dims, const float* const* W, const float* const* bias,
                         const float* x, int64_t x_stride, float* y, int64_t y_stride, float* mid, void* stream) {
    if (n_rows < 0 || !mid_dims_supported(n_layers, dims) || !W || !bias || !x || !y || !mid || x_stride < dims[0] || y_stride < dims[4] ||
        (x_stride & 3) || !aligned(16, x, mid))
        return fail_arg("bridges_mlp_mid_rows: 256-128-64-128-256 only, 16-byte aligned input rows, scratch of n x 64 floats");
    if (n_rows == 0) return BRIDGES_OK;
    for (int l = 0; l < 4; ++l)
        if (!W[l] || !bias[l] || !aligned(16, W[l])) return fail_arg("bridges_mlp_mid_rows");
    const dim3 grid((unsigned)clamp_grid(ceil_div(n_rows, 32), 256));
    if (int rc = launch("k_rows2<256,128,64>", k_rows2<256, 128, 64, true>, grid, dim3(1024), 0, stream, W[0], bias[0], W[1], bias[1],
                        (int)n_rows, x, x_stride, mid, (int64_t)64))
        return rc;
    return launch("k_rows2<64,128,256>", k_rows2<64, 128, 256, false>, grid, dim3(1024), 0, stream, W[2], bias[2], W[3], bias[3],
                  (int)n_rows, (const float*)mid, (int64_t)64, y, y_stride);
}

int bridges_mlp_mid_backward(int32_t rows, int32_t n_layers, const int32_t* dims, const float* const* W, float* const* dW,
                             float* const* db, float* const* acts, float* const* dz, float* rest_param, const float* rest_grad,
                             float* rest_exp_avg, float* rest_exp_avg_sq, int64_t rest_n, const float* step, double lr, double beta1,
                             double beta2, double eps, void* stream) {
    if (rows != 32 || !mid_dims_supported(n_layers, dims) || !dW || !db || !dz) return fail_arg("bridges_mlp_mid_backward: 32 rows of 256-128-64-128-256 only");
    if (rest_n < 0 || (rest_n & 3) || (rest_n > 0 && (!rest_param || !rest_grad || !rest_exp_avg || !rest_exp_avg_sq || !step)))
        return fail_arg("bridges_mlp_mid_backward: the Adam range must be a multiple of 4 floats with all four buffers and the step");
    if (rest_n > 0 && !aligned(16, rest_param, rest_grad, rest_exp_avg, rest_exp_avg_sq))
        return fail_arg("bridges_mlp_mid_backward: Adam buffers must be 16-byte aligned");
    if (rest_n > 0 && (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)))
        return fail_arg("bridges_mlp_mid_backward: hyper-parameters");
    MidPtrs p{};
    if (int rc = mid_ptrs_fill("bridges_mlp_mid_backward", p, W, nullptr, dW, db, acts, dz)) return rc;
    p.rest_p = rest_param; p.rest_g = rest_grad; p.rest_m = rest_exp_avg; p.rest_v = rest_exp_avg_sq; p.rest_n = (long long)rest_n;
    p.step = step; p.lr = lr; p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
    // riders: ~4 float4 groups per thread over the range, at most 248 workgroups (one per CU beside the stack's eight)
    int64_t riders = rest_n > 0 ? ceil_div(rest_n >> 2, 4096) : 0;
    if (riders > 248) riders = 248;
    return launch("k_mid_bwd", k_mid_bwd<256, 128, 64, 128, 256>, dim3(256 / 32 + (unsigned)riders), dim3(1024), 0, stream, p);
}

int bridges_linear_backward_adam(int32_t rows, int32_t K, int32_t N, const float* dz, const float* a_in, float* W, float* bias,
                                 float* exp_avg_w, float* exp_avg_sq_w, float* exp_avg_b, float* exp_avg_sq_b, float* rest_param,
                                 const float* rest_grad, float* rest_exp_avg, float* rest_exp_avg_sq, int64_t rest_n, const float* step,
                                 double lr, double beta1, double beta2, double eps, const int64_t* a_block, int32_t a_block_bias,
                                 void* stream) {
    if (rows != 32 || K <= 0 || N <= 0 || !dz || !a_in || !W || !bias || !exp_avg_w || !exp_avg_sq_w || !exp_avg_b || !exp_avg_sq_b || !step)
        return fail_arg("bridges_linear_backward_adam: one 32-row batch tile, all buffers given");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return fail_arg("bridges_linear_backward_adam: hyper-parameters");
    if (rest_n < 0 || (rest_n & 3) || (rest_n > 0 && (!rest_param || !rest_grad || !rest_exp_avg || !rest_exp_avg_sq)))
        return fail_arg("bridges_linear_backward_adam: rest range must be a multiple of 4 floats with all four buffers");
    if (rest_n > 0 && !aligned(16, rest_param, rest_grad, rest_exp_avg, rest_exp_avg_sq))
        return fail_arg("bridges_linear_backward_adam: rest buffers must be 16-byte aligned");
    const int n_ntiles = ceil_div(N, 32), n_ktiles = ceil_div(K, 32);
    // ~256 weight-gradient jobs (a workgroup then walks ~2 KB of every row of W / m / v) and <= 256 workgroups for the other
    // layers' range: measured 142 us per optimiser step against 156 us with 1024 + 1024 (the update is bound by DRAM locality
    // of six strided streams, not by parallelism; 128 jobs: 146 us, 64: 170 us)
    int per_job = ceil_div(n_ntiles * n_ktiles, 256);             // (128 / 192 / 384 / 512 jobs with 512 threads: 119 / 114 / 115 / 117 us per step, 256: 112-114)
    if (per_job < 4) per_job = 4;
    const int n_dw_jobs = n_ntiles * ceil_div(n_ktiles, per_job);
    int64_t rest_jobs = ceil_div(rest_n >> 2, 256);
    if (rest_jobs > 256) rest_jobs = 256;
    AdamFold ad{W, bias, exp_avg_w, exp_avg_sq_w, exp_avg_b, exp_avg_sq_b, step, lr, beta1, beta2, eps,
                rest_param, rest_grad, rest_exp_avg, rest_exp_avg_sq, (long long)rest_n};
    // 512-thread workgroups: the eight waves of a weight-gradient job walk eight ADJACENT k tiles, 1 KB of every row of W / m / v
    // at a time (two workgroups per CU at the kernel's 247 registers would do the same with 512 B)
    return launch("k_lin_bwd<adam>", k_lin_bwd<true>, dim3(n_dw_jobs + (int)rest_jobs), dim3(512), 0, stream, rows, K, N, dz, a_in,
                  (const float*)W, (float*)nullptr, (float*)nullptr, (float*)nullptr, (const float*)nullptr, n_dw_jobs, per_job, 0, 0, ad,
                  a_block, (int)a_block_bias, LossLog{});
}

// reward_stride: 0 = one map [px] for every transition, px = a map per transition of the per-call arrays ([n, px])
static bool reward_stride_ok(int64_t reward_stride, int32_t px) { return reward_stride == 0 || reward_stride == px; }

int bridges_mlp_input_rows(int32_t batch, int32_t rows, int32_t px, int32_t nf, const int64_t* counter, const float* block_all,
                           const float* action_all, const float* binary_all, const float* reward, int64_t reward_stride,
                           const float* obstacle, float* x, void* stream) {
    if (batch <= 0 || rows < batch || (rows & 31) || px <= 0 || nf < 0 || !counter || !block_all || !action_all || !reward || !obstacle || !x)
        return fail_arg("bridges_mlp_input");
    if (!reward_stride_ok(reward_stride, px)) return fail_arg("bridges_mlp_input_rows: reward_stride must be 0 or px");
    const dim3 grid(clamp_grid(ceil_div(rows * (4 * px + nf), 256), 2048));
    if (reward_stride)
        return launch("k_mlp_input<rows>", k_mlp_input<true>, grid, dim3(256), 0, stream, batch, rows, px, nf, counter, block_all, action_all,
                      binary_all, reward, obstacle, x);
    return launch("k_mlp_input", k_mlp_input<false>, grid, dim3(256), 0, stream, batch, rows, px, nf, counter, block_all, action_all,
                  binary_all, reward, obstacle, x);
}

int bridges_mlp_input(int32_t batch, int32_t rows, int32_t px, int32_t nf, const int64_t* counter, const float* block_all,
                      const float* action_all, const float* binary_all, const float* reward, const float* obstacle,
                      float* x, void* stream) {
    return bridges_mlp_input_rows(batch, rows, px, nf, counter, block_all, action_all, binary_all, reward, 0, obstacle, x, stream);
}

int bridges_mlp_input_batches_rows(int32_t n_batches, int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* block_all,
                                   const float* action_all, const float* binary_all, const float* reward, int64_t reward_stride,
                                   const float* obstacle, float* x_all, void* stream) {
    if (n_batches <= 0 || batch <= 0 || rows < batch || (rows & 31) || px <= 0 || nf < 0 || !block_all || !action_all || !reward || !obstacle || !x_all)
        return fail_arg("bridges_mlp_input_batches");
    if (!reward_stride_ok(reward_stride, px)) return fail_arg("bridges_mlp_input_batches_rows: reward_stride must be 0 or px");
    const dim3 grid(clamp_grid(ceil_div(rows * (4 * px + nf), 256), 2048), n_batches);
    if (reward_stride)
        return launch("k_mlp_input<rows> (all batches)", k_mlp_input<true>, grid, dim3(256), 0, stream, batch, rows, px, nf,
                      (const int64_t*)nullptr, block_all, action_all, binary_all, reward, obstacle, x_all);
    return launch("k_mlp_input (all batches)", k_mlp_input<false>, grid, dim3(256), 0, stream, batch, rows, px, nf, (const int64_t*)nullptr,
                  block_all, action_all, binary_all, reward, obstacle, x_all);
}

int bridges_mlp_input_batches(int32_t n_batches, int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* block_all,
                              const float* action_all, const float* binary_all, const float* reward, const float* obstacle,
                              float* x_all, void* stream) {
    return bridges_mlp_input_batches_rows(n_batches, batch, rows, px, nf, block_all, action_all, binary_all, reward, 0, obstacle, x_all,
                                          stream);
}

// The _rows forms with an obstacle raster per transition, bit-packed ([n, 64] uint64, one word per image row): px must be 64 * 64.
static bool obstacle_bits_ok(int32_t px) { return px == IMG * IMG; }

int bridges_mlp_input_task_rows(int32_t batch, int32_t rows, int32_t px, int32_t nf, const int64_t* counter, const float* block_all,
                                const float* action_all, const float* binary_all, const float* reward, int64_t reward_stride,
                                const uint64_t* obstacle_bits, float* x, void* stream) {
    if (batch <= 0 || rows < batch || (rows & 31) || px <= 0 || nf < 0 || !counter || !block_all || !action_all || !reward || !obstacle_bits || !x)
        return fail_arg("bridges_mlp_input_task_rows");
    if (!reward_stride_ok(reward_stride, px)) return fail_arg("bridges_mlp_input_task_rows: reward_stride must be 0 or px");
    if (!obstacle_bits_ok(px)) return fail_arg("bridges_mlp_input_task_rows: bit-packed obstacle rasters need px == 4096 (64 x 64)");
    const dim3 grid(clamp_grid(ceil_div(rows * (4 * px + nf), 256), 2048));
    if (reward_stride)
        return launch("k_mlp_input<rows, obstacle bits>", k_mlp_input<true, true>, grid, dim3(256), 0, stream, batch, rows, px, nf, counter,
                      block_all, action_all, binary_all, reward, obstacle_bits, x);
    return launch("k_mlp_input<obstacle bits>", k_mlp_input<false, true>, grid, dim3(256), 0, stream, batch, rows, px, nf, counter, block_all,
                  action_all, binary_all, reward, obstacle_bits, x);
}

int bridges_mlp_input_batches_task_rows(int32_t n_batches, int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* block_all,
                                        const float* action_all, const float* binary_all, const float* reward, int64_t reward_stride,
                                        const uint64_t* obstacle_bits, float* x_all, void* stream) {
    if (n_batches <= 0 || batch <= 0 || rows < batch || (rows & 31) || px <= 0 || nf < 0 || !block_all || !action_all || !reward || !obstacle_bits || !x_all)
        return fail_arg("bridges_mlp_input_batches_task_rows");
    if (!reward_stride_ok(reward_stride, px)) return fail_arg("bridges_mlp_input_batches_task_rows: reward_stride must be 0 or px");
    if (!obstacle_bits_ok(px)) return fail_arg("bridges_mlp_input_batches_task_rows: bit-packed obstacle rasters need px == 4096 (64 x 64)");
    const dim3 grid(clamp_grid(ceil_div(rows * (4 * px + nf), 256), 2048), n_batches);
    if (reward_stride)
        return launch("k_mlp_input<rows, obstacle bits> (all batches)", k_mlp_input<true, true>, grid, dim3(256), 0, stream, batch, rows, px, nf,
                      (const int64_t*)nullptr, block_all, action_all, binary_all, reward, obstacle_bits, x_all);
    return launch("k_mlp_input<obstacle bits> (all batches)", k_mlp_input<false, true>, grid, dim3(256), 0, stream, batch, rows, px, nf,
                  (const int64_t*)nullptr, block_all, action_all, binary_all, reward, obstacle_bits, x_all);
}

int bridges_successor_loss(int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* y, const float* reward,
                           const int64_t* counter, const float* q_target_all, const float* sf_target_all, int32_t use_q,
                           int32_t use_sf, float* dy, float* loss_rows, float* q_out, float* losses, int32_t n_losses,
                           int64_t* counter_inc, int32_t* ticket, float* adam_step, void* stream) {
    return bridges_successor_loss_rows(batch, rows, px, nf, y, reward, 0, counter, q_target_all, sf_target_all, use_q, use_sf, dy,
                                       loss_rows, q_out, losses, n_losses, counter_inc, ticket, adam_step, stream);
}

int bridges_successor_loss_rows(int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* y, const float* reward,
                                int64_t reward_stride, const int64_t* counter, const float* q_target_all, const float* sf_target_all,
                                int32_t use_q, int32_t use_sf, float* dy, float* loss_rows, float* q_out, float* losses,
                                int32_t n_losses, int64_t* counter_inc, int32_t* ticket, float* adam_step, void* stream) {
    if (batch <= 0 || rows < batch || px <= 0 || nf < 0 || !y || !reward || !counter || !dy || !loss_rows || !q_out)
        return fail_arg("bridges_successor_loss");
    if ((use_q && !q_target_all) || (use_sf && !sf_target_all)) return fail_arg("bridges_successor_loss: target missing");
    if (ticket && !counter_inc) return fail_arg("bridges_successor_loss: a ticket needs counter_inc");
    if (adam_step && !ticket) return fail_arg("bridges_successor_loss: adam_step is advanced by the ticket holder");
    // with a ticket word (zero before the first call; the kernel re-arms it) the logging happens inside the loss kernel
    if (!reward_stride_ok(reward_stride, px)) return fail_arg("bridges_successor_loss_rows: reward_stride must be 0 or px");
    int64_t* const inc = ticket ? counter_inc : (int64_t*)nullptr;
    if (int rc = reward_stride ? launch("k_successor_loss<rows>", k_successor_loss<true, false>, dim3(rows), dim3(LOSS_THREADS), 0, stream, batch,
                                        px, nf, y, reward, counter, q_target_all, sf_target_all, use_q, use_sf, dy, loss_rows, q_out,
                                        losses, n_losses, inc, ticket, adam_step, (const float*)nullptr)
                               : launch("k_successor_loss", k_successor_loss<false, false>, dim3(rows), dim3(LOSS_THREADS), 0, stream, batch,
                                        px, nf, y, reward, counter, q_target_all, sf_target_all, use_q, use_sf, dy, loss_rows, q_out,
                                        losses, n_losses, inc, ticket, adam_step, (const float*)nullptr))
        return rc;
    if (ticket || !losses || !counter_inc) return BRIDGES_OK;
    return launch("k_loss_log", k_loss_log, dim3(1), dim3(64), 0, stream, batch, loss_rows, losses, n_losses, counter_inc);
}

int bridges_successor_loss_weighted(int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* y, const float* reward,
                                    int64_t reward_stride, const int64_t* counter, const float* q_target_all,
                                    const float* sf_target_all, int32_t use_q, int32_t use_sf, float* dy, float* loss_rows,
                                    float* q_out, float* losses, int32_t n_losses, int64_t* counter_inc, int32_t* ticket,
                                    float* adam_step, const float* weight_all, void* stream) {
    if (batch <= 0 || rows < batch || px <= 0 || nf < 0 || !y || !reward || !counter || !dy || !loss_rows || !q_out)
        return fail_arg("bridges_successor_loss_weighted");
    if (!weight_all) return fail_arg("bridges_successor_loss_weighted: weight missing");
    if ((use_q && !q_target_all) || (use_sf && !sf_target_all)) return fail_arg("bridges_successor_loss_weighted: target missing");
    if (ticket && !counter_inc) return fail_arg("bridges_successor_loss_weighted: a ticket needs counter_inc");
    if (adam_step && !ticket) return fail_arg("bridges_successor_loss_weighted: adam_step is advanced by the ticket holder");
    if (!reward_stride_ok(reward_stride, px)) return fail_arg("bridges_successor_loss_weighted: reward_stride must be 0 or px");
    int64_t* const inc = ticket ? counter_inc : (int64_t*)nullptr;
    if (int rc = reward_stride ? launch("k_successor_loss<rows, weighted>", k_successor_loss<true, true>, dim3(rows), dim3(LOSS_THREADS), 0,
                                        stream, batch, px, nf, y, reward, counter, q_target_all, sf_target_all, use_q, use_sf, dy,
                                        loss_rows, q_out, losses, n_losses, inc, ticket, adam_step, weight_all)
                               : launch("k_successor_loss<weighted>", k_successor_loss<false, true>, dim3(rows), dim3(LOSS_THREADS), 0,
                                        stream, batch, px, nf, y, reward, counter, q_target_all, sf_target_all, use_q, use_sf, dy,
                                        loss_rows, q_out, losses, n_losses, inc, ticket, adam_step, weight_all))
        return rc;
    if (ticket || !losses || !counter_inc) return BRIDGES_OK;
    return launch("k_loss_log", k_loss_log, dim3(1), dim3(64), 0, stream, batch, loss_rows, losses, n_losses, counter_inc);
}

int bridges_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* step,
                      double lr, double beta1, double beta2, double eps, void* stream) {
    if (n < 0 || !param || !grad || !exp_avg || !exp_avg_sq || !step) return fail_arg("bridges_adam_step");
    if (!aligned(16, param, grad, exp_avg, exp_avg_sq)) return fail_arg("bridges_adam_step: buffers must be 16-byte aligned");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return fail_arg("bridges_adam_step: hyper-parameters");
    if (n == 0) return BRIDGES_OK;
    return launch("k_adam_flat", k_adam_flat, dim3((int)clamp_grid(ceil_div(n >> 2, 256), 4096)), dim3(256), 0, stream, param, grad,
                  exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps);
}

int bridges_adam_multi(const bridges_adam_slot* slots, int32_t n_slots, const int32_t* chunk_slot, const int32_t* chunk_off,
                       int32_t n_chunks, const float* step, double lr, double beta1, double beta2, double eps, void* stream) {
    if (n_slots < 0 || n_chunks < 0 || !step || (n_chunks > 0 && (!slots || !chunk_slot || !chunk_off || n_slots < 1))) return fail_arg("bridges_adam_multi");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return fail_arg("bridges_adam_multi: hyper-parameters");
    if (n_chunks == 0) return BRIDGES_OK;
    return launch("k_adam_multi", k_adam_multi, dim3((unsigned)n_chunks), dim3(256), 0, stream, slots, chunk_slot, chunk_off, step, lr,
                  beta1, beta2, eps);
}

// ---- conv3x3 + bias + ReLU [+ pool] for the 64-wide, 16-output-channel layers (conv_kernels.hip) ------------------
int bridges_conv3x3_relu_o16_ex(const float* x, const float* x2, const float* w, const float* bias, float* out, float* out2,
                                const float* proj_w, const float* proj_b, int64_t n, int32_t c_in, int32_t c_in2, int32_t H,
                                int32_t W, int32_t mode, void* stream) {
    if (n < 0 || !x || !w || !bias || !out) return fail_arg("bridges_conv3x3_relu_o16");
    if (W != CONV_W || H <= 0 || (H % CONV_BAND) != 0) return fail_arg("bridges_conv3x3_relu_o16: W must be 64 and H a multiple of 8");
    if (mode < CONV_EPI_PLAIN || mode > CONV_EPI_PROJ) return fail_arg("bridges_conv3x3_relu_o16: mode");
    if (mode == CONV_EPI_BOTH && !out2) return fail_arg("bridges_conv3x3_relu_o16: out2 missing");
    if (mode == CONV_EPI_PROJ && (!proj_w || !proj_b)) return fail_arg("bridges_conv3x3_relu_o16: projection weights missing");
    if (x2) {
        if (c_in != 16 || c_in2 != 16) return fail_arg("bridges_conv3x3_relu_o16: two inputs must hold 16 channels each");
    } else {
        c_in2 = 0;
        if (!(c_in >= 1 && c_in <= 4) && c_in != 16 && c_in != 32) return fail_arg("bridges_conv3x3_relu_o16: C_in must be 1..4, 16 or 32");
    }
    if (!aligned(16, x, out, x2) || !aligned(8, out2)) return fail_arg("bridges_conv3x3_relu_o16: tensors must be 16-byte aligned");
    if (n == 0) return BRIDGES_OK;
    const int64_t blocks = n * (H / CONV_BAND);
    if (blocks > 0x7fffffff) return fail_arg("bridges_conv3x3_relu_o16: too many images");
    typedef void (*o16_fn)(const float*, const float*, const float*, const float*, float*, float*, const float*, const float*, int, int, int);
    // [input channels: two inputs of 16 or 32 in one, 1..4, 16][mode]
    const o16_fn kernels[3][4] = {
        {k_conv3x3_o16<16, 2, CONV_EPI_PLAIN>, k_conv3x3_o16<16, 2, CONV_EPI_POOL>, k_conv3x3_o16<16, 2, CONV_EPI_BOTH>, k_conv3x3_o16<16, 2, CONV_EPI_PROJ>},
        {k_conv3x3_o16<4, 1, CONV_EPI_PLAIN>, k_conv3x3_o16<4, 1, CONV_EPI_POOL>, k_conv3x3_o16<4, 1, CONV_EPI_BOTH>, k_conv3x3_o16<4, 1, CONV_EPI_PROJ>},
        {k_conv3x3_o16<16, 1, CONV_EPI_PLAIN>, k_conv3x3_o16<16, 1, CONV_EPI_POOL>, k_conv3x3_o16<16, 1, CONV_EPI_BOTH>, k_conv3x3_o16<16, 1, CONV_EPI_PROJ>},
    };
    const int layout = (x2 || c_in == 32) ? 0 : c_in <= 4 ? 1 : 2;
    return launch("k_conv3x3_o16", kernels[layout][mode], dim3((unsigned)blocks), dim3(256), 0, stream, x, x2, w, bias,
                  out, out2, proj_w, proj_b, (int)H, (int)c_in, (int)c_in2);
}

int bridges_conv3x3_relu_o16(const float* x, const float* w, const float* bias, float* out, int64_t n, int32_t c_in,
                             int32_t H, int32_t W, int32_t pool, void* stream) {
    return bridges_conv3x3_relu_o16_ex(x, nullptr, w, bias, out, nullptr, nullptr, nullptr, n, c_in, 0, H, W,
                                       pool ? CONV_EPI_POOL : CONV_EPI_PLAIN, stream);
}

int bridges_upconv2x2(const float* x, const float* w, const float* bias, float* out, int64_t n, int32_t c_in, int32_t c_out,
                      int32_t H, int32_t W, void* stream) {
    if (n < 0 || !x || !w || !bias || !out || H <= 0 || W <= 0 || (W % 16) != 0) return fail_arg("bridges_upconv2x2: W must be a multiple of 16");
    if (!((c_in == 32 && c_out == 16) || (c_in == 64 && c_out == 32))) return fail_arg("bridges_upconv2x2: (C_in, C_out) must be (32, 16) or (64, 32)");
    if (!aligned(16, out) || !aligned(8, w)) return fail_arg("bridges_upconv2x2: out must be 16-byte, w 8-byte aligned");
    if (n == 0) return BRIDGES_OK;
    const int64_t tiles = n * H * (W / 16);
    const int64_t blocks = ceil_div(tiles, 4);
    if (blocks > 0x7fffffff) return fail_arg("bridges_upconv2x2: too many images");
    return launch("k_upconv2x2", c_in == 32 ? k_upconv2x2<32, 1> : k_upconv2x2<64, 2>, dim3((unsigned)blocks), dim3(256), 0, stream, x, w,
                  bias, out, (int)H, (int)W, (long)tiles);
}

// ---- K11: ConvBlock training passes (csrc/conv_train_kernels.hip) ---------------------------------------------------------
int bridges_conv3x3(const float* x, const float* in_mask, const float* w, const float* bias, const float* mask, float* out, int64_t n,
                    int32_t c_in, int32_t c_out, int32_t W, int32_t mode, int32_t transposed, void* stream) {
    if (n < 0 || !x || !w || !out || c_in < 1 || c_out < 16 || (c_out & 15)) return fail_arg("bridges_conv3x3: channels (C_out must be a multiple of 16)");
    if (W != 8 && W != 16 && W != 32 && W != 64) return fail_arg("bridges_conv3x3: W must be 8, 16, 32 or 64 (square images)");
    if (mode < C3_EPI_RAW || mode > C3_EPI_MASK || (mode == C3_EPI_BIAS_RELU && !bias) || (mode == C3_EPI_MASK && !mask)) return fail_arg("bridges_conv3x3: mode");
    if (!aligned(16, out, mask, x, in_mask)) return fail_arg("bridges_conv3x3: x / in_mask / out / mask must be 16-byte aligned");
    if (n == 0) return BRIDGES_OK;
    const int bands = W / c3_band_rows(W);
    if (n * bands > 0x7fffffff) return fail_arg("bridges_conv3x3: too many images");
    // forward: w [c_out, c_in, 3, 3]; transposed (input gradient): w [c_in, c_out, 3, 3] of the layer, taps flipped
    const int w_sin = transposed ? c_out * 9 : 9, w_sout = transposed ? 9 : c_in * 9, flip = transposed ? 1 : 0;
    const c3_fn k = W == 64   ? c3_kernel<64>(c_in, mode)
                    : W == 32 ? c3_kernel<32>(c_in, mode)
                    : W == 16 ? c3_kernel<16>(c_in, mode)
                              : c3_kernel<8>(c_in, mode);
    return launch("k_c3", k, dim3((unsigned)(n * bands), (unsigned)(c_out / 16)), dim3(256), 0, stream, x, in_mask, w, bias, mask, out,
                  c_in, c_out, w_sin, w_sout, flip);
}

int bridges_conv3x3_wgrad_scratch(int64_t n, int32_t c_in, int32_t c_out, int32_t W, int64_t* floats) {
    if (!floats || n < 1 || c_in < 1 || c_out < 16 || (c_out & 15) || (W != 8 && W != 16 && W != 32 && W != 64)) return fail_arg("bridges_conv3x3_wgrad_scratch");
    const int64_t units = n * (W / c3_wgrad_rows(W)), tiles = (int64_t)(c_out / 16) * ((c_in + 15) / 16);
    int64_t splits = 512 / tiles;
    if (splits < 1) splits = 1;
    if (splits > units) splits = units;
    const int64_t ups = (units + splits - 1) / splits;
    splits = (units + ups - 1) / ups;
    *floats = splits * ((int64_t)c_out * c_in * 9 + c_out);
    return BRIDGES_OK;
}

int bridges_conv3x3_wgrad(const float* g, const float* g_mask, const float* x, float* dw, float* db, float* scratch, int64_t scratch_floats,
                          int64_t n, int32_t c_in, int32_t c_out, int32_t W, void* stream) {
    if (!g || !x || !scratch || (!dw) != (!db)) return fail_arg("bridges_conv3x3_wgrad");
    if (!aligned(16, g, g_mask, x)) return fail_arg("bridges_conv3x3_wgrad: g / g_mask / x must be 16-byte aligned");
    int64_t need = 0;
    if (int rc = bridges_conv3x3_wgrad_scratch(n, c_in, c_out, W, &need)) return rc;
    if (scratch_floats < need) return fail_arg("bridges_conv3x3_wgrad: scratch too small (bridges_conv3x3_wgrad_scratch)");
    const int64_t units = n * (W / c3_wgrad_rows(W));
    const int tiles = (c_out / 16) * ((c_in + 15) / 16);
    const int64_t n_w = (int64_t)c_out * c_in * 9;
    const int splits = (int)(need / (n_w + c_out));
    const int ups = (int)((units + splits - 1) / splits);
    float* part = scratch;
    float* part_b = scratch + (int64_t)splits * n_w;
    // a table rather than nested ?:, which would name (and instantiate) the innermost kernels first and reorder the device code
    typedef void (*wgrad_fn)(const float*, const float*, const float*, float*, float*, int, int, int, int);
    const wgrad_fn by_width[4] = {k_c3_wgrad<64>, k_c3_wgrad<32>, k_c3_wgrad<16>, k_c3_wgrad<8>};
    const wgrad_fn k = by_width[W == 64 ? 0 : W == 32 ? 1 : W == 16 ? 2 : 3];
    if (int rc = launch("k_c3_wgrad", k, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, stream, g, g_mask, x, part, part_b, (int)n,
                        c_in, c_out, ups))
        return rc;
    if (!dw) return BRIDGES_OK;                                    // partial sums only: the caller reduces them (bridges_reduce_jobs)
    const int64_t tot = n_w + c_out;
    return launch("k_c3_reduce", k_c3_reduce, dim3((unsigned)c3_reduce_blocks(tot, splits)), dim3(256), 0, stream, (const float*)part,
                  (const float*)part_b, dw, db, (int)n_w, c_out, splits);
}

int bridges_maxpool2(const float* a, float* y, int64_t nc, int32_t H, int32_t W, void* stream) {
    if (nc < 0 || !a || !y || H <= 0 || W <= 0 || (W & 3) || (H & 1)) return fail_arg("bridges_maxpool2");
    if (!aligned(16, a) || !aligned(8, y)) return fail_arg("bridges_maxpool2: alignment");
    const int64_t items = nc * (H / 2) * (W / 4);
    if (items == 0) return BRIDGES_OK;
    return launch("k_maxpool2", k_maxpool2, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, stream, a, y, items, H, W);
}

int bridges_maxpool2_relu_backward(const float* a, const float* dy, float* g, int64_t nc, int32_t H, int32_t W, void* stream) {
    if (nc < 0 || !a || !dy || !g || H <= 0 || W <= 0 || (W & 3) || (H & 1)) return fail_arg("bridges_maxpool2_relu_backward");
    if (!aligned(16, a, g) || !aligned(8, dy)) return fail_arg("bridges_maxpool2_relu_backward: alignment");
    const int64_t items = nc * (H / 2) * (W / 4);
    if (items == 0) return BRIDGES_OK;
    return launch("k_maxpool2_relu_bwd", k_maxpool2_relu_bwd, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, stream, a, dy, g, items,
                  H, W);
}

int bridges_bias_grad(const float* g, float* db, float* scratch, int64_t scratch_floats, int64_t n, int32_t C, int32_t hw, void* stream) {
    if (!g || !db || !scratch || n < 1 || C < 1 || hw < 1) return fail_arg("bridges_bias_grad");
    int S = (int)(n < 32 ? n : 32);
    if (scratch_floats < (int64_t)S * C) return fail_arg("bridges_bias_grad: scratch needs min(n, 32) * C floats");
    if (int rc = launch("k_bias_grad_part", k_bias_grad_part, dim3((unsigned)C, (unsigned)S), dim3(256), 0, stream, g, scratch, (int)n, C,
                        hw, S))
        return rc;
    return launch("k_c3_reduce", k_c3_reduce, dim3((unsigned)c3_reduce_blocks(C, S)), dim3(256), 0, stream, (const float*)scratch,
                  (const float*)scratch, db, db, 0, C, S);
}

// ---- backward of the U-Net's transposed / 1x1 convolutions (conv_train_kernels.hip) -----------------------------------------------
int bridges_upconv2x2_backward_scratch(int64_t n, int32_t c_in, int32_t c_out, int32_t H, int32_t W, int64_t* floats) {
    if (!floats || n < 0 || H < 1 || W < 1 || (((int64_t)H * W) & 63)) return fail_arg("bridges_upconv2x2_backward_scratch: H * W must be a multiple of 64");
    if (!((c_in == 32 && c_out == 16) || (c_in == 64 && c_out == 32))) return fail_arg("bridges_upconv2x2_backward_scratch: (C_in, C_out) must be (32, 16) or (64, 32)");
    int tps;
    const int S = up2_splits(n * H * W / 64, &tps);
    *floats = (int64_t)(S < 1 ? 1 : S) * ((int64_t)c_in * c_out * 4 + c_out);
    return BRIDGES_OK;
}

int bridges_upconv2x2_backward(const float* x, const float* g, const float* w, float* dx, float* dw, float* db, float* scratch,
                               int64_t scratch_floats, int64_t n, int32_t c_in, int32_t c_out, int32_t H, int32_t W, void* stream) {
    if (!x || !g || !w || !scratch || (!dw) != (!db)) return fail_arg("bridges_upconv2x2_backward");
    int64_t need = 0;
    if (int rc = bridges_upconv2x2_backward_scratch(n, c_in, c_out, H, W, &need)) return rc;
    if (scratch_floats < need) return fail_arg("bridges_upconv2x2_backward: scratch too small (bridges_upconv2x2_backward_scratch)");
    if (!aligned(8, g)) return fail_arg("bridges_upconv2x2_backward: g must be 8-byte aligned");
    const int64_t tiles = n * H * W / 64;
    if (tiles > 0x7fffffff) return fail_arg("bridges_upconv2x2_backward: too many images");
    const int K = c_out * 4;
    float* part = scratch;
    int tps;
    const int S = up2_splits(tiles, &tps);
    float* part_b = scratch + (size_t)(S < 1 ? 1 : S) * c_in * K;
    if (tiles == 0 && dw) {                                         // no image: zero gradients
        hipStream_t s = (hipStream_t)stream;
        HIP_TRY(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)c_in * K, s));
        HIP_TRY(hipMemsetAsync(db, 0, sizeof(float) * (size_t)c_out, s));
        return BRIDGES_OK;
    }
    if (dx) {
        if (int rc = launch("k_up2_dx", k_up2_dx, dim3((unsigned)tiles, (unsigned)ceil_div(c_in, 16)), dim3(256),
                            (size_t)K * 80 * sizeof(float), stream, g, w, dx, c_in, c_out, H, W))
            return rc;
    }
    if (int rc = launch("k_up2_wgrad", c_in == 64 ? k_up2_wgrad<4, 8> : k_up2_wgrad<2, 4>, dim3((unsigned)S), dim3(256), 0, stream, x, g,
                        part, part_b, c_out, H, W, (int)tiles, tps))
        return rc;
    if (!dw) return BRIDGES_OK;                                    // partial sums only (bridges_reduce_jobs)
    const int n_w = c_in * K;
    return launch("k_c3_reduce", k_c3_reduce, dim3((unsigned)c3_reduce_blocks(n_w + c_out, S)), dim3(256), 0, stream, (const float*)part,
                  (const float*)part_b, dw, db, n_w, c_out, S);
}

int bridges_conv1x1_o1_forward(const float* x, const float* w, const float* bias, float* y, int64_t n, int32_t c_in, int32_t hw, void* stream) {
    if (!x || !w || !bias || !y || n < 0 || c_in < 1 || hw < 4 || (hw & 3)) return fail_arg("bridges_conv1x1_o1_forward: H * W must be a multiple of 4");
    if (!aligned(16, x, y)) return fail_arg("bridges_conv1x1_o1_forward: x / y must be 16-byte aligned");
    const int64_t quads = n * hw / 4;
    if (quads == 0) return BRIDGES_OK;
    return launch("k_pw1_fwd", k_pw1_fwd, dim3((unsigned)ceil_div(quads, 256)), dim3(256), 0, stream, x, w, bias, y, c_in, hw, quads);
}

int bridges_conv1x1_o1_backward(const float* x, const float* g, const float* w, float* dx, float* dw, float* db, float* scratch,
                                int64_t scratch_floats, int64_t n, int32_t c_in, int32_t hw, void* stream) {
    if (!x || !g || !w || !dx || !scratch || (!dw) != (!db) || n < 0 || c_in < 1 || c_in > 32 || hw < 4 || (hw & 3))
        return fail_arg("bridges_conv1x1_o1_backward: C_in <= 32, H * W a multiple of 4");
    if (!aligned(16, x, g, dx)) return fail_arg("bridges_conv1x1_o1_backward: x / g / dx must be 16-byte aligned");
    const int64_t quads = n * hw / 4;
    const int64_t S = clamp_grid(ceil_div(quads, 256), 256);
    if (scratch_floats < S * (c_in + 1)) return fail_arg("bridges_conv1x1_o1_backward: scratch needs min(256, ceil(n * hw / 1024)) * (C_in + 1) floats");
    float* part = scratch;
    float* part_b = scratch + S * c_in;
    if (int rc = launch("k_pw1_bwd", k_pw1_bwd, dim3((unsigned)S), dim3(256), 0, stream, x, g, w, dx, part, part_b, c_in, hw, quads))
        return rc;
    if (!dw) return BRIDGES_OK;                                    // partial sums only (bridges_reduce_jobs)
    return launch("k_c3_reduce", k_c3_reduce, dim3((unsigned)c3_reduce_blocks(c_in + 1, (int)S)), dim3(256), 0, stream, (const float*)part,
                  (const float*)part_b, dw, db, c_in, 1, (int)S);
}

int bridges_reduce_jobs(const bridges_reduce_job* jobs_dev, int32_t n_jobs, int32_t total_blocks, void* stream) {
    if (n_jobs < 0 || total_blocks < 0 || (n_jobs > 0 && (!jobs_dev || total_blocks < 1))) return fail_arg("bridges_reduce_jobs");
    if (n_jobs == 0) return BRIDGES_OK;
    return launch("k_reduce_jobs", k_reduce_jobs, dim3((unsigned)total_blocks), dim3(256), 0, stream, jobs_dev, n_jobs);
}

}  // extern "C"
