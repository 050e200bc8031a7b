// Hindsight goal relabelling of finished episodes (strategy "final", header comment of bridges_hindsight_relabel): every
// episode that ended in this lock-step is written a second time, G times, under T targets that its own final structure reached --
// the centres of the bounding boxes of blocks drawn from it -- with the reward, the linear reward and the done flag the
// environment would have recorded had the same placements been made under those targets.  Nothing of the simulator runs again:
// the stability verdicts are the rollout's (the step_flags kept beside every buffered record), the reached-test is k_step's on
// vertices rebuilt from the recorded poses, and the linear reward comes from the row runs of the block's raster on the float64
// row prefix sums of the hindsight task's reward map, built by the device code of k_task_features (task_map_prefix).
//
// Three launches, no atomics:
//   k_hindsight_count   one wave per (env, slot): draws the goals and walks the reached-test alone -> rows of the slot
//   k_hindsight_scan    one workgroup: exclusive prefix sum of the counts in place (as k_scan), the total -> *count
//   k_hindsight_rows    four waves per (env, slot) with rows: the goals again (same draw, same bits), the raster of the T target
//                       cubes, map and prefix tables in LDS (51 KB, as k_task_features: three workgroups per CU), then wave 0 walks
//                       the episode and stores row offset[slot] + t.  The order of the output is (env, slot, t) by construction.
//   k_hindsight_rows_nstep  the same body for a loop on n-step returns (bridges_hindsight_relabel_nstep): wave 0 keeps the relabelled
//                       lin of every step in LDS and stores, per start t of the walk, the h-step row offset[slot] + t -- when step
//                       t + n_step - 1 is reached, or at the walk's end.  Counts and offsets are the same: one row per walk step.
// The work per finished (env, slot) is that of one k_task_features workgroup -- which the lock-step runs for every finished env
// anyway -- plus K rasters of ~250 wave instructions; envs in mid-episode leave at once.
#include "bridges_device.h"
// (device code of env_kernels.hip -- raster_rows_nv, raster_reward_fetch, task_map_prefix -- is in scope: api.hip includes it first)

namespace bridges {

#define HIND_SALT 0x68696E645F726E67ull     // "hind_rng"
#define HIND_MAX_GOALS 4
#define HIND_SCAN_THREADS 256

struct HindArgs {
    const double* buf;              // [E, K, W] the buffered records of every env's running episode
    const uint8_t* flags;           // [E, K, 8] step_flags of the step of each record
    const int32_t* len;             // [E] records in the buffer
    const uint8_t* ended;           // [E] the episode ended in this lock-step
    const uint32_t* episode;        // [E] task_episode of the episode in the buffer
    const bridges_shape* shapes;    // the task's shape table
    const double* grid_x;           // [img] pixel centres
    const double* grid_y;
    const float* gauss_k;           // [BRIDGES_GAUSS_TAPS]
    uint64_t seed;
    int32_t E, K, W, T, G, env_id_base, n_shapes, target_shape, img;
};

// Lane v < nv: world vertex v of the block that record `row` placed (pos + R(c, s) * local vertex: k_pose_block's and
// k_enumerate's expression, on the recorded pose -- the rollout's bits).  Returns the (clamped) shape id.
__device__ __forceinline__ int hind_block_verts(const HindArgs& a, const double* row, int lane, double& vx, double& vz) {
    int sh = (int)row[BRIDGES_REC_ASHAPE];
    sh = sh < 0 ? 0 : (sh < a.n_shapes ? sh : a.n_shapes - 1);
    const bridges_shape& s = a.shapes[sh];
    const double px = row[BRIDGES_REC_APOSE], pz = row[BRIDGES_REC_APOSE + 1], cs = row[BRIDGES_REC_APOSE + 2], sn = row[BRIDGES_REC_APOSE + 3];
    vx = 0.0; vz = 0.0;
    if (lane < s.nv) {
        double rx, rz;
        rot2(s.vx[lane], s.vz[lane], cs, sn, rx, rz);
        vx = px + rx; vz = pz + rz;
    }
    return sh;
}

// Axis-aligned bounding box of a block's vertices as k_step's reached-test takes it.
struct HindBox { double cx, cz, hx, hz; };
__device__ __forceinline__ HindBox hind_box(double vx, double vz, bool hasv) {
    const double x0 = wave_min_d(hasv ? vx : 1e300), x1 = wave_max_d(hasv ? vx : -1e300);
    const double z0 = wave_min_d(hasv ? vz : 1e300), z1 = wave_max_d(hasv ? vz : -1e300);
    HindBox b;
    b.cx = (x0 + x1) * 0.5; b.cz = (z0 + z1) * 0.5; b.hx = (x1 - x0) * 0.5; b.hz = (z1 - z0) * 0.5;
    return b;
}

// The hindsight targets of slot g of env e's episode of m records: lane 3 q + k holds coordinate k of target q (y = 0), as
// k_step keeps its per-env targets.  Returns m' (the eligible blocks); with m' == 0 there are no targets.
// The choice: idx = 0 .. m' - 1, for i < min(T, m'): j = i + ((u * (m' - i)) >> 32), u = r >> 32, swap(idx[i], idx[j]) with
//   h0 = splitmix64(((seed & 0xFFFFFFFF) << 32 | gid) ^ HIND_SALT);  h1 = splitmix64(h0 ^ episode);  h2 = splitmix64(h1 ^ g);
//   r = splitmix64(h2 ^ i);   target q is the box centre of block idx[q mod m'].  Lane i holds idx[i]; integer arithmetic only.
__device__ __forceinline__ int hind_goals(const HindArgs& a, int e, int g, int m, int lane, double& tgv) {
    const double* rows = a.buf + (size_t)e * a.K * a.W;
    tgv = 0.0;
    int mp = m;
    if (m > 0 && !(rows[(size_t)(m - 1) * a.W + BRIDGES_REC_STABLE_N] > 0.5)) mp = m - 1;     // a collapsed last block is no goal
    if (mp <= 0) return 0;
    const uint64_t h0 = splitmix64((((a.seed & 0xFFFFFFFFull) << 32) | (uint32_t)(a.env_id_base + e)) ^ HIND_SALT);
    const uint64_t h1 = splitmix64(h0 ^ (uint64_t)a.episode[e]);
    const uint64_t h2 = splitmix64(h1 ^ (uint64_t)g);
    int idx = lane;
    const int nd = a.T < mp ? a.T : mp;
    for (int i = 0; i < nd; ++i) {
        const uint64_t u = splitmix64(h2 ^ (uint64_t)i) >> 32;
        const int j = __builtin_amdgcn_readfirstlane(i + (int)((u * (uint64_t)(mp - i)) >> 32));
        const int vi = __builtin_amdgcn_readlane(idx, i), vj = __builtin_amdgcn_readlane(idx, j);
        idx = lane == i ? vj : (lane == j ? vi : idx);
    }
    for (int q = 0; q < a.T; ++q) {
        const int b = __builtin_amdgcn_readlane(idx, q % mp);
        double vx, vz;
        const int sh = hind_block_verts(a, rows + (size_t)b * a.W, lane, vx, vz);
        const HindBox bx = hind_box(vx, vz, lane < a.shapes[sh].nv);
        tgv = lane == 3 * q ? bx.cx : (lane == 3 * q + 2 ? bx.cz : tgv);
    }
    return mp;
}

// k_step's reached-test of one placed block against the open targets `left`, literally: the target after a reached one is
// skipped (env_kernels.hip, "targets"), ty = 0.
__device__ __forceinline__ uint32_t hind_reach(const HindArgs& a, uint32_t left, double tgv, const HindBox& b, double depth) {
    const double hy = depth * 0.5;
    bool skip = false;
    for (int t = 0; t < a.T; ++t) {
        if (!((left >> t) & 1u)) continue;
        if (skip) { skip = false; continue; }
        const double tx = readlane_d(tgv, 3 * t), ty = readlane_d(tgv, 3 * t + 1), tz = readlane_d(tgv, 3 * t + 2);
        const bool in = fabs(tx - b.cx) < b.hx + 1e-6 && fabs(ty) < hy + 1e-6 && fabs(tz - b.cz) < b.hz + 1e-6;
        if (in) { left &= ~(1u << t); skip = true; }
    }
    return left;
}

__device__ __forceinline__ int hind_len(const HindArgs& a, int e) {
    if (!a.ended[e]) return 0;
    const int m = a.len[e];
    return m < 0 ? 0 : (m > a.K ? a.K : m);
}

__global__ __launch_bounds__(256) void k_hindsight_count(HindArgs a, int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int item = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE));
    if (item >= a.E * a.G) return;
    const int e = item / a.G, g = item % a.G;
    const int m = hind_len(a, e);
    double tgv;
    int n = 0;
    if (m > 0 && hind_goals(a, e, g, m, lane, tgv) > 0) {
        const double* rows = a.buf + (size_t)e * a.K * a.W;
        uint32_t left = (1u << a.T) - 1u;
        for (int t = 0; t < m; ++t) {
            double vx, vz;
            const int sh = hind_block_verts(a, rows + (size_t)t * a.W, lane, vx, vz);
            left = hind_reach(a, left, tgv, hind_box(vx, vz, lane < a.shapes[sh].nv), a.shapes[sh].depth);
            n = t + 1;
            if (left == 0u) break;                  // the episode is over under the new targets: later transitions do not exist
        }
    }
    if (lane == 0) cnt[item] = n;
}

// Exclusive prefix sum in place (cnt[i] <- rows in front of slot i), the total -> *total.  One workgroup, as k_scan.
__global__ __launch_bounds__(HIND_SCAN_THREADS) void k_hindsight_scan(int n, int32_t* __restrict__ cnt, int32_t* __restrict__ total) {
    __shared__ int wave_tot[HIND_SCAN_THREADS / WAVE];
    __shared__ int carry_s;
    const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < n; base += HIND_SCAN_THREADS) {
        const int i = base + t;
        const int v = i < n ? cnt[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int up = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += up;
        }
        if (lane == WAVE - 1) wave_tot[wv] = incl;
        __syncthreads();
        int wbase = 0;
        for (int k = 0; k < wv; ++k) wbase += wave_tot[k];
        const int carry = carry_s;
        if (i < n) cnt[i] = carry + wbase + incl - v;
        __syncthreads();
        if (t == HIND_SCAN_THREADS - 1) carry_s = carry + wbase + incl;
        __syncthreads();
    }
    if (t == 0) *total = carry_s;
}

// Raster of a convex outline whose world vertex v sits in lane v: raster_outline's frames (edge_frame on the same vertices) and
// its row runs, without the trip through memory.
__device__ __forceinline__ uint64_t hind_raster(double vx, double vz, const bridges_shape& s, const HindArgs& a, int lane) {
    const int f = lane < s.nv ? lane : 0;
    const int ia = s.fa[f], ib = s.fb[f];
    const double ax = shfl_d(vx, ia), az = shfl_d(vz, ia), bx = shfl_d(vx, ib), bz = shfl_d(vz, ib);
    double cx = 0.0, cz = 0.0, nx = 0.0, nz = 0.0;
    if (lane < s.nv) {
        const Frame2 fr = edge_frame(ax, az, bx, bz);
        cx = fr.cx; cz = fr.cz; nx = fr.nx; nz = fr.nz;
    }
    const int gi = lane < a.img ? lane : a.img - 1;
    return raster_rows_nv(cx, cz, nx, nz, s.nv, a.img, a.grid_x[gi], a.grid_y[gi], lane);
}

// The h-step return of a start from the relabelled lin of its h steps: steps 1-2 of bridges_nstep_fold (binary64, this order, no
// fused multiply-add: the build has -ffp-contract=off).
__device__ __forceinline__ double hind_return(const double* lin, int h, double gamma) {
    double acc = 0.0, disc = 1.0;
    for (int k = 0; k < h; ++k) {
        acc += disc * lin[k];
        disc *= gamma;
    }
    return acc;
}

// One relabelled row: the lane-strided copy of `row` with REWARD, LIN, DONE and the targets of the tail replaced.  FOLD: the h-step
// row of a start (bridges_hindsight_relabel_nstep) -- `lin` is the return, STABLE_S and TD are read from the start's record
// `start`, and h goes into one more column, W.
template <bool FOLD>
__device__ __forceinline__ void hind_store_row(const HindArgs& a, const double* row, const double* start, double reward, double lin,
                                               double done, double h, double tgv, int lane, double* o) {
    const int wout = FOLD ? a.W + 1 : a.W;
    for (int c0 = 0; c0 < wout; c0 += WAVE) {       // (every lane stays for the shuffle)
        const int c = c0 + lane;
        double v = c < a.W ? row[c] : 0.0;
        if (FOLD && (c == BRIDGES_REC_STABLE_S || c == BRIDGES_REC_TD)) v = start[c];
        if (c == BRIDGES_REC_REWARD) v = reward;
        if (c == BRIDGES_REC_LIN) v = lin;
        if (c == BRIDGES_REC_DONE) v = done;
        const int k = c - BRIDGES_REC_WIDTH;
        const bool tail = k >= 0 && k < 3 * a.T;
        const double tk = shfl_d(tgv, tail ? k : 0);
        if (tail) v = tk;
        if (FOLD && c == a.W) v = h;
        if (c < wout) o[c] = v;
    }
}

// FOLD = false: bridges_hindsight_relabel's rows.  FOLD = true: bridges_hindsight_relabel_nstep's -- the same walk, with the
// relabelled lin of every step kept in LDS (K doubles); start t is stored when step t + n_step - 1 is reached, the return folded
// again from the kept values in ascending k, and the end of the walk stores the starts still pending.
template <bool FOLD>
__device__ __forceinline__ void hind_rows(const HindArgs& a, const int32_t* __restrict__ off, const int32_t* __restrict__ total,
                                          double* __restrict__ out, int n_step, double gamma) {
    __shared__ float kz[TASK_KZ];
    __shared__ uint64_t tb_l[IMG];
    __shared__ float map_l[IMG * TASK_ROW];
    __shared__ double pre_l[IMG * TASK_ROW];
    __shared__ double lin_l[FOLD ? BRIDGES_MAX_BLOCKS : 1];
    const int item = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const int e = item / a.G, g = item % a.G;
    const int m = hind_len(a, e);
    if (m == 0) return;                             // mid-episode (the whole workgroup leaves)
    const int first = off[item];
    const int n = (item + 1 < a.E * a.G ? off[item + 1] : *total) - first;
    if (n <= 0) return;                             // no eligible block
    for (int i = tid; i < TASK_KZ; i += TASK_THREADS) {
        const int tap = i - TASK_KZ_PAD;
        kz[i] = (tap >= 0 && tap < BRIDGES_GAUSS_TAPS) ? a.gauss_k[tap] : 0.f;
    }
    double tgv;
    hind_goals(a, e, g, m, lane, tgv);
    // raster of the T target cubes at identity rotation (vertex = target + local vertex: k_task_features), every wave
    const bridges_shape& cube = a.shapes[a.target_shape];
    uint64_t bits = 0ull;
    for (int q = 0; q < a.T; ++q) {
        const double px = readlane_d(tgv, 3 * q), pz = readlane_d(tgv, 3 * q + 2);
        const int v = lane < cube.nv ? lane : 0;
        bits |= hind_raster(px + cube.vx[v], pz + cube.vz[v], cube, a, lane);
    }
    if (wv == 0) tb_l[lane] = bits;
    __syncthreads();
    task_map_prefix<false>(bits, tb_l, kz, map_l, pre_l, a.img, lane, wv, nullptr);
    if (wv != 0) return;
    // ---- wave 0: the episode under the hindsight targets ----
    const double* rows = a.buf + (size_t)e * a.K * a.W;
    const uint8_t* fl = a.flags + (size_t)e * a.K * 8;
    uint32_t left = (1u << a.T) - 1u;
    const int wout = FOLD ? a.W + 1 : a.W;
    double reward_d = 0.0, done_d = 0.0;            // of the last step walked (FOLD: the rows stored at the end are that step's)
    for (int t = 0; t < n; ++t) {
        const double* row = rows + (size_t)t * a.W;
        double vx, vz;
        const int sh = hind_block_verts(a, row, lane, vx, vz);
        const bridges_shape& s = a.shapes[sh];
        left = hind_reach(a, left, tgv, hind_box(vx, vz, lane < s.nv), s.depth);
        const uint64_t rb = hind_raster(vx, vz, s, a, lane);
        double p_hi, p_lo;
        raster_reward_fetch(rb, pre_l, lane, p_hi, p_lo);
        const float base = (float)raster_reward_sum(p_hi, p_lo);                 // k_raster's cand_lin
        const bool st_frozen = fl[t * 8 + F_STABLE_FROZEN], st_free = fl[t * 8 + F_STABLE_UNFROZEN];
        const bool truncated = fl[t * 8 + F_TRUNCATED], no_actions = fl[t * 8 + F_NO_ACTIONS];
        const int n_reached = a.T - __popc(left);
        const bool all_reached = left == 0u;
        const float reward = !st_frozen ? -1.f : (all_reached ? (float)n_reached : (float)(-1 + n_reached));
        const float lin = st_free ? base : (st_frozen ? base / 100.f : 0.f);
        const bool done = !st_frozen || all_reached || truncated || no_actions;
        reward_d = (double)reward; done_d = done ? 1.0 : 0.0;
        if (!FOLD) {
            hind_store_row<false>(a, row, row, reward_d, (double)lin, done_d, 1.0, tgv, lane, out + (size_t)(first + t) * wout);
            continue;
        }
        lin_l[t] = (double)lin;                     // every lane the same value: each reads back what it wrote itself
        if (t + 1 >= n_step) {
            const int st = t + 1 - n_step;
            hind_store_row<true>(a, row, rows + (size_t)st * a.W, reward_d, hind_return(lin_l + st, n_step, gamma), done_d,
                                 (double)n_step, tgv, lane, out + (size_t)(first + st) * wout);
        }
    }
    if (FOLD) {
        // the end of the walk: the starts that never saw n_step steps, with the last step's record -- whether or not it is done
        const double* row = rows + (size_t)(n - 1) * a.W;
        for (int st = n - n_step + 1 > 0 ? n - n_step + 1 : 0; st < n; ++st)
            hind_store_row<true>(a, row, rows + (size_t)st * a.W, reward_d, hind_return(lin_l + st, n - st, gamma), done_d,
                                 (double)(n - st), tgv, lane, out + (size_t)(first + st) * wout);
    }
}

__global__ __launch_bounds__(TASK_THREADS) void k_hindsight_rows(HindArgs a, const int32_t* __restrict__ off, const int32_t* __restrict__ total,
                                                                double* __restrict__ out) {
    hind_rows<false>(a, off, total, out, 1, 0.0);
}

__global__ __launch_bounds__(TASK_THREADS) void k_hindsight_rows_nstep(HindArgs a, const int32_t* __restrict__ off,
                                                                      const int32_t* __restrict__ total, double* __restrict__ out,
                                                                      int n_step, double gamma) {
    hind_rows<true>(a, off, total, out, n_step, gamma);
}

// ---- per-step goals (strategy "per_step", hindsight experience replay's "future"; header comment of bridges_hindsight_per_step) ----
// One work item is (env, slot, step t < m'): its own draw, its own T targets -- block f >= t first, the others from the structure
// after step f -- and at most one row.  Three launches again:
//   k_hindsight_step_count  one wave per (env, slot): the boxes of the K blocks once, one per lane; then for every t the draw, the
//                           targets (lane reads of the boxes) and the reached-test of steps < t -> the rows of the slot and the
//                           32-bit mask of the steps that have one
//   k_hindsight_scan        as above, on the counts
//   k_hindsight_step_rows   four waves per (env, slot, t), a grid of E * G * K of which all but the set bits of the masks leave
//                           after two loads: one pass of the k_hindsight_rows body -- the draw again, the T cube rasters, map and
//                           prefix tables in LDS -- then wave 0 walks steps < t with the reached-test alone, relabels step t
//                           (FOLD: steps t .. last, their lin kept in LDS) and stores row offset[slot] + popcount(mask below t).
//                           (One workgroup per (env, slot) looping over its mask was measured too and was no faster; the loop
//                           around the map build costs SGPR spills: DESIGN.md, "Per-step goals".)

// Lane b < m: box and depth of the block that record b placed (hind_box on hind_block_verts: the bits of the walk of "final").
struct HindLaneBoxes { double cx, cz, hx, hz, depth; };
__device__ __forceinline__ HindLaneBoxes hind_lane_boxes(const HindArgs& a, const double* rows, int m, int lane) {
    HindLaneBoxes lb = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < m; ++b) {
        double vx, vz;
        const int sh = hind_block_verts(a, rows + (size_t)b * a.W, lane, vx, vz);
        const HindBox bx = hind_box(vx, vz, lane < a.shapes[sh].nv);
        if (lane == b) { lb.cx = bx.cx; lb.cz = bx.cz; lb.hx = bx.hx; lb.hz = bx.hz; lb.depth = a.shapes[sh].depth; }
    }
    return lb;
}
__device__ __forceinline__ HindBox hind_box_of(const HindLaneBoxes& lb, int b) {
    HindBox bx;
    bx.cx = readlane_d(lb.cx, b); bx.cz = readlane_d(lb.cz, b); bx.hx = readlane_d(lb.hx, b); bx.hz = readlane_d(lb.hz, b);
    return bx;
}

__device__ __forceinline__ int hind_eligible(const HindArgs& a, const double* rows, int m) {
    return (m > 0 && !(rows[(size_t)(m - 1) * a.W + BRIDGES_REC_STABLE_N] > 0.5)) ? m - 1 : m;
}

__device__ __forceinline__ uint64_t hind_slot_key(const HindArgs& a, int e, int g) {
    const uint64_t h0 = splitmix64((((a.seed & 0xFFFFFFFFull) << 32) | (uint32_t)(a.env_id_base + e)) ^ HIND_SALT);
    const uint64_t h1 = splitmix64(h0 ^ (uint64_t)a.episode[e]);
    return splitmix64(h1 ^ (uint64_t)g);
}

// The targets of work item (slot key h2, step t < mp): h3 = splitmix64(h2 ^ ((t + 1) << 8)), r_i = splitmix64(h3 ^ i), u_i = r_i >> 32;
// f = t + ((u_0 * (mp - t)) >> 32); n = f + 1, idx = 0 .. n - 1, swap(idx[0], idx[f]), for i = 1 .. min(T, n) - 1:
// swap(idx[i], idx[i + ((u_i * (n - i)) >> 32)]); target q = centre of block idx[q mod n] in lanes 3 q, 3 q + 2.  Integers only.
__device__ __forceinline__ void hind_step_goals(const HindArgs& a, uint64_t h2, int t, int mp, int lane, const HindLaneBoxes& lb,
                                                double& tgv) {
    const uint64_t h3 = splitmix64(h2 ^ ((uint64_t)(t + 1) << 8));
    const uint64_t u0 = splitmix64(h3) >> 32;
    const int f = __builtin_amdgcn_readfirstlane(t + (int)((u0 * (uint64_t)(mp - t)) >> 32));
    const int n = f + 1;
    int idx = lane == 0 ? f : (lane == f ? 0 : lane);
    const int nd = a.T < n ? a.T : n;
    for (int i = 1; i < nd; ++i) {
        const uint64_t u = splitmix64(h3 ^ (uint64_t)i) >> 32;
        const int j = __builtin_amdgcn_readfirstlane(i + (int)((u * (uint64_t)(n - i)) >> 32));
        const int vi = __builtin_amdgcn_readlane(idx, i), vj = __builtin_amdgcn_readlane(idx, j);
        idx = lane == i ? vj : (lane == j ? vi : idx);
    }
    tgv = 0.0;
    for (int q = 0; q < a.T; ++q) {
        const int b = __builtin_amdgcn_readlane(idx, q % n);
        const double cx = readlane_d(lb.cx, b), cz = readlane_d(lb.cz, b);
        tgv = lane == 3 * q ? cx : (lane == 3 * q + 2 ? cz : tgv);
    }
}

// The open targets in front of step t under the targets tgv: the reached-test of steps 0 .. t - 1 (0: the episode was over).
__device__ __forceinline__ uint32_t hind_step_prefix(const HindArgs& a, int t, double tgv, const HindLaneBoxes& lb) {
    uint32_t left = (1u << a.T) - 1u;
    for (int s = 0; s < t && left != 0u; ++s) left = hind_reach(a, left, tgv, hind_box_of(lb, s), readlane_d(lb.depth, s));
    return left;
}

__global__ __launch_bounds__(256) void k_hindsight_step_count(HindArgs a, int32_t* __restrict__ cnt, uint32_t* __restrict__ mask) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int item = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) / WAVE));
    if (item >= a.E * a.G) return;
    const int e = item / a.G, g = item % a.G;
    const int m = hind_len(a, e);
    int n = 0;
    uint32_t has = 0u;
    if (m > 0) {
        const double* rows = a.buf + (size_t)e * a.K * a.W;
        const int mp = hind_eligible(a, rows, m);   // t < m': a collapsed last step has no later block to be a goal
        if (mp > 0) {
            const HindLaneBoxes lb = hind_lane_boxes(a, rows, mp, lane);
            const uint64_t h2 = hind_slot_key(a, e, g);
            for (int t = 0; t < mp; ++t) {
                double tgv;
                hind_step_goals(a, h2, t, mp, lane, lb, tgv);
                if (hind_step_prefix(a, t, tgv, lb) != 0u) { has |= 1u << t; ++n; }     // else: over before t, no transition
            }
        }
    }
    if (lane == 0) { cnt[item] = n; mask[item] = has; }
}

template <bool FOLD>
__device__ __forceinline__ void hind_step_rows(const HindArgs& a, const int32_t* __restrict__ off, const uint32_t* __restrict__ mask,
                                               double* __restrict__ out, int n_step, double gamma) {
    __shared__ float kz[TASK_KZ];
    __shared__ uint64_t tb_l[IMG];
    __shared__ float map_l[IMG * TASK_ROW];
    __shared__ double pre_l[IMG * TASK_ROW];
    __shared__ double lin_l[FOLD ? BRIDGES_NSTEP_MAX : 1];
    const int item = blockIdx.x / a.K, t = blockIdx.x % a.K, tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const int e = item / a.G, g = item % a.G;
    const int m = hind_len(a, e);
    if (m == 0) return;                             // mid-episode (the whole workgroup leaves)
    const uint32_t has = mask[item];
    if (!((has >> t) & 1u)) return;                 // no row of this step
    const int first = off[item];
    for (int i = tid; i < TASK_KZ; i += TASK_THREADS) {
        const int tap = i - TASK_KZ_PAD;
        kz[i] = (tap >= 0 && tap < BRIDGES_GAUSS_TAPS) ? a.gauss_k[tap] : 0.f;
    }
    const double* rows = a.buf + (size_t)e * a.K * a.W;
    const uint8_t* fl = a.flags + (size_t)e * a.K * 8;
    const int mp = hind_eligible(a, rows, m);
    const HindLaneBoxes lb = hind_lane_boxes(a, rows, mp, lane);
    const uint64_t h2 = hind_slot_key(a, e, g);
    const bridges_shape& cube = a.shapes[a.target_shape];
    const int wout = FOLD ? a.W + 1 : a.W;
    {
        double tgv;
        hind_step_goals(a, h2, t, mp, lane, lb, tgv);
        // raster of the T target cubes at identity rotation, every wave (as k_hindsight_rows)
        uint64_t bits = 0ull;
        for (int q = 0; q < a.T; ++q) {
            const double px = readlane_d(tgv, 3 * q), pz = readlane_d(tgv, 3 * q + 2);
            const int v = lane < cube.nv ? lane : 0;
            bits |= hind_raster(px + cube.vx[v], pz + cube.vz[v], cube, a, lane);
        }
        if (wv == 0) tb_l[lane] = bits;
        __syncthreads();
        task_map_prefix<false>(bits, tb_l, kz, map_l, pre_l, a.img, lane, wv, nullptr);
        if (wv == 0) {
            // ---- wave 0: steps t .. last under the targets of step t ----
            uint32_t left = hind_step_prefix(a, t, tgv, lb);
            double* o = out + (size_t)(first + __popc(has & ((1u << t) - 1u))) * wout;
            const int hmax = FOLD ? n_step : 1;
            double reward_d = 0.0, done_d = 0.0, lin_d = 0.0;
            int h = 0;
            for (int s = t; s < m && h < hmax; ++s) {
                const double* row = rows + (size_t)s * a.W;
                double vx, vz;
                const int sh = hind_block_verts(a, row, lane, vx, vz);
                const bridges_shape& sp = a.shapes[sh];
                left = hind_reach(a, left, tgv, hind_box(vx, vz, lane < sp.nv), sp.depth);
                const uint64_t rb = hind_raster(vx, vz, sp, a, lane);
                double p_hi, p_lo;
                raster_reward_fetch(rb, pre_l, lane, p_hi, p_lo);
                const float base = (float)raster_reward_sum(p_hi, p_lo);             // k_raster's cand_lin
                const bool st_frozen = fl[s * 8 + F_STABLE_FROZEN], st_free = fl[s * 8 + F_STABLE_UNFROZEN];
                const bool truncated = fl[s * 8 + F_TRUNCATED], no_actions = fl[s * 8 + F_NO_ACTIONS];
                const int n_reached = a.T - __popc(left);
                const bool all_reached = left == 0u;
                const float reward = !st_frozen ? -1.f : (all_reached ? (float)n_reached : (float)(-1 + n_reached));
                const float lin = st_free ? base : (st_frozen ? base / 100.f : 0.f);
                const bool done = !st_frozen || all_reached || truncated || no_actions;
                reward_d = (double)reward; done_d = done ? 1.0 : 0.0; lin_d = (double)lin;
                if (FOLD) lin_l[h] = lin_d;         // every lane the same value: each reads back what it wrote itself
                ++h;
                if (all_reached) break;             // the walk under these targets ends here
            }
            const double* last = rows + (size_t)(t + h - 1) * a.W;
            if (FOLD)
                hind_store_row<true>(a, last, rows + (size_t)t * a.W, reward_d, hind_return(lin_l, h, gamma), done_d, (double)h, tgv, lane, o);
            else
                hind_store_row<false>(a, last, last, reward_d, lin_d, done_d, 1.0, tgv, lane, o);
        }
    }
}

__global__ __launch_bounds__(TASK_THREADS) void k_hindsight_step_rows(HindArgs a, const int32_t* __restrict__ off,
                                                                     const uint32_t* __restrict__ mask, double* __restrict__ out) {
    hind_step_rows<false>(a, off, mask, out, 1, 0.0);
}

__global__ __launch_bounds__(TASK_THREADS) void k_hindsight_step_rows_nstep(HindArgs a, const int32_t* __restrict__ off,
                                                                           const uint32_t* __restrict__ mask, double* __restrict__ out,
                                                                           int n_step, double gamma) {
    hind_step_rows<true>(a, off, mask, out, n_step, gamma);
}

}  // namespace bridges
