// Vectorised assembly_gym lock-step on gfx950: one 64-lane wavefront per environment for the
// task logic (k_step, k_enumerate, k_select) and a persistent wave-per-image rasteriser (k_raster).
//
// Reference semantics (paths relative to the reference root):
//   k_step      AssemblyGym.step + stabilities_freezing + sparse_reward + terminated
//               (assembly_gym/assembly_gym/envs/gym_env.py:11-22, 141-145, 218-253, 325-333),
//               lin_reward rule of rollout_episode (robotoddler/training/successor_dqn.py:397-401)
//   k_enumerate generate_actions (robotoddler/utils/actions.py:7-52) + create_block
//               (gym_env.py:204-216) + the bounds half of collision_on_action (gym_env.py:304-323)
//   k_raster    render_blocks_2d / Shape.contains_2d (assembly_gym/assembly_gym/utils/rendering.py:105-113,
//               assembly_env.py:126-137), the overlap half of filter_actions (actions.py:71-82) and
//               sum(action_features * reward_features) (successor_dqn.py:399-401)
#include "bridges_device.h"
#include "rbe_device.h"

namespace bridges {

// ---------------------------------------------------------------------------------------------
__device__ inline void reset_env(const DevCtx& c, int e, int lane) {
    c.b.state_bits[(size_t)e * IMG + lane] = 0ull;
    if (lane < c.K) c.b.blk_occ[(size_t)e * c.K + lane] = 0;
    if (lane == 0) {
        c.b.n_blocks[e] = 0;
        c.b.n_if[e] = 0;
        c.b.targets_left[e] = (c.n_targets >= 32) ? 0xffffffffu : ((1u << c.n_targets) - 1u);
        c.b.needs_reset[e] = 0;
    }
}

// number of raw candidates of a state: n_groups * (n_ground + n_free_faces * n_offsets).  NOT clamped to the env's capacity
// a_max: k_scan does that for every producer of n_cand (k_reset, k_step, bridges_replay_unpack, a host that loads states),
// raises bit 3 of the env's F_LP_ERROR flag and counts the truncation (stats: cand_overflow) -- a candidate set cut short
// is data loss the reference cannot have (actions.py:7-52 enumerates everything) and must not pass silently.
__device__ inline int count_candidates(const DevCtx& c, int e, int nb, int lane) {
    int nfree = 0;
    for (int i0 = 0; i0 < nb * MAXV; i0 += WAVE) {
        int i = i0 + lane;
        bool fr = false;
        if (i < nb * MAXV) {
            int b = i / MAXV, f = i % MAXV;
            int nv = c.tt->shapes[c.b.blk_shape[(size_t)e * c.K + b]].nv;
            fr = f < nv && !((c.b.blk_occ[(size_t)e * c.K + b] >> f) & 1);
        }
        nfree += __popcll(__ballot(fr));
    }
    return c.n_groups * (c.n_ground + nfree * c.n_offsets);
}

__global__ __launch_bounds__(WAVE) void k_reset(DevCtx c) {
    int e = blockIdx.x, lane = threadIdx.x;
    reset_env(c, e, lane);
    if (lane < 8) c.b.step_flags[(size_t)e * 8 + lane] = 0;
    int nc = count_candidates(c, e, 0, lane);
    if (lane == 0) {
        c.b.reward[e] = 0.f;
        c.b.lin_reward[e] = 0.f;
        c.b.n_reached[e] = 0;
        c.b.draw_counter[e] = 0;
        c.b.n_cand[e] = nc;
    }
}

// ---------------------------------------------------------------------------------------------
// One wave per environment.  The kernel is a chain of dependent steps, and beside another env group's rasteriser
// (which keeps the HBM write queues full) every dependent global-memory round trip costs microseconds, so the loads
// are organised in exactly two levels: (0) everything addressed by the env id alone -- counters, the placed blocks,
// the contact list, the shape table, the persisted tableau's header -- is requested up front and staged in LDS;
// (1) what the selected candidate and the header point to (candidate pose / vertices / raster, tableau cells).
// After that the wave works on LDS and registers only; results leave as stores nobody waits for.
#define STEP_IF_LDS 32      // contacts kept in LDS (the rest of a longer list is read in place from global memory)
#define STEP_TAB_LDS 4096   // doubles of LDS tableau in k_step (32 KiB: carriers included, 12 blocks with 17 contacts still fit;
                            // 4 workgroups per CU, which costs nothing: a 2048-env group needs two rounds at 5 per CU as well)
struct StepStage {          // dead once the contacts are found: shares its storage with the tableau
    bridges_shape shapes[8];
    double pose[MAXK * 4];
    double verts[MAXK * MAXV * 2];
    int32_t shape_id[MAXK];
    int32_t occ[MAXK];
};
struct StepKeep {           // what the LP reads of the assembly
    double if_geom[STEP_IF_LDS * 8];
    int32_t if_body[STEP_IF_LDS * 2];
    double cen[MAXK * 2];
    double vol[MAXK];
};
static_assert(sizeof(StepStage) <= STEP_TAB_LDS * sizeof(double), "staging area must fit into the tableau storage");

// k_step<>(DevCtx): the fixed task, targets in the kernel arguments.  k_step<const double*>(DevCtx, env_targets): every env
// tests its own targets (bridges_task_buffers.env_targets[e]: one value per lane, a level-0 load).  One body for both; the
// optional trailing argument keeps the fixed-task kernel's argument list -- and with it its code, which sits at the register
// limit -- what it is without the feature.
__device__ __forceinline__ const double* step_targets() { return nullptr; }
__device__ __forceinline__ const double* step_targets(const double* p) { return p; }
template <typename... ENV_TARGETS>
__global__ __launch_bounds__(WAVE) void k_step(DevCtx c, ENV_TARGETS... env_targets_arg) {
    constexpr bool PER_ENV = sizeof...(ENV_TARGETS) == 1;
    const double* env_targets = step_targets(env_targets_arg...);
    (void)env_targets;
    __shared__ __attribute__((aligned(16))) double tab[STEP_TAB_LDS];
    __shared__ LpScratch S;
    __shared__ StepKeep Lk;
    StepStage& L = *reinterpret_cast<StepStage*>(tab);
    // latency-bound kernel that usually runs beside another env group's bandwidth-bound rasteriser: take the
    // instruction arbiter's priority so the dependent pivot chain is not stretched by the co-resident store waves
    __builtin_amdgcn_s_setprio(3);
    const int e = blockIdx.x, lane = threadIdx.x;
    const int K = c.K;
    uint8_t* flags = c.b.step_flags + (size_t)e * 8;
    int32_t* shape_id_g = c.b.blk_shape + (size_t)e * K;
    double* pose_g = c.b.blk_pose + (size_t)e * K * 4;
    double* verts_g = c.b.blk_verts + (size_t)e * K * MAXV * 2;
    uint8_t* occ_g = c.b.blk_occ + (size_t)e * K;
    int32_t* if_body_g = c.b.if_body + (size_t)e * MAXIF * 2;
    double* if_geom_g = c.b.if_geom + (size_t)e * MAXIF * 8;
    double* ws = c.b.lp_ws + (size_t)e * c.b.lp_ws_stride;
    const WarmHdr* hdr_g = reinterpret_cast<const WarmHdr*>(ws);

    // ---- level 0: everything the env id addresses ----
    const uint8_t need_reset = c.b.needs_reset[e];
    const int a = c.b.sel_index[e];
    const int off = c.b.cand_offset[e];
    const int nb = c.b.n_blocks[e];                 // index of the new block
    const int n_if_old = c.b.n_if[e];
    uint32_t left = c.b.targets_left[e];
    const uint64_t sbits = c.b.state_bits[(size_t)e * IMG + lane];
    WarmPre W;
    W.magic = hdr_g->magic; W.n_blocks = hdr_g->n_blocks; W.n_if = hdr_g->n_if; W.stride = hdr_g->stride;
    W.half = hdr_g->half; W.m = hdr_g->m;
    W.basis_lane = hdr_g->basis[lane];
    double tgv = 0.0;                               // PER_ENV: lane 3 t + k holds coordinate k of target t
    if constexpr (PER_ENV) {
        if (lane < c.n_targets * 3) tgv = env_targets[(size_t)e * c.n_targets * 3 + lane];
    }
    {
        const double* src = reinterpret_cast<const double*>(c.tt->shapes);
        double* dst = reinterpret_cast<double*>(L.shapes);
        const int nd = c.n_shapes * (int)(sizeof(bridges_shape) / 8);
        for (int i = lane; i < nd; i += WAVE) dst[i] = src[i];
        for (int i = lane; i < nb * 4; i += WAVE) L.pose[i] = pose_g[i];
        for (int i = lane; i < nb * MAXV * 2; i += WAVE) L.verts[i] = verts_g[i];
        if (lane < K) { L.shape_id[lane] = shape_id_g[lane]; L.occ[lane] = occ_g[lane]; }
        const int n0 = n_if_old < STEP_IF_LDS ? n_if_old : STEP_IF_LDS;
        for (int i = lane; i < n0 * 8; i += WAVE) Lk.if_geom[i] = if_geom_g[i];
        for (int i = lane; i < n0 * 2; i += WAVE) Lk.if_body[i] = if_body_g[i];
    }

    if (need_reset) {                               // reset-only lock-step (previous state had no valid action)
        reset_env(c, e, lane);
        if (lane < 8) flags[lane] = 0;
        if (lane == 0) {
            c.b.reward[e] = 0.f;
            c.b.lin_reward[e] = 0.f;
            c.b.n_reached[e] = 0;
        }
        if (lane == 0) c.b.n_cand[e] = c.n_groups * c.n_ground;     // raw count: k_scan clamps to a_max and flags a truncation
        return;
    }

    // ---- level 1: the selected candidate, the cells of the persisted tableau ----
    const size_t ci = (size_t)off + a;
    const int dsc = lane < 4 ? c.b.cand_desc[ci * 4 + lane] : 0;
    const double cpose = lane < 4 ? c.b.cand_pose[ci * 4 + lane] : 0.0;
    const double cvert = lane < MAXV * 2 ? c.b.cand_verts[ci * MAXV * 2 + lane] : 0.0;
    const uint64_t cbits = c.b.cand_bits[ci * IMG + lane];
    const float base = c.b.cand_lin[ci];
    warm_prefetch(W, ws, nb, n_if_old, lane);
    const int tb = __builtin_amdgcn_readlane(dsc, 0), tf = __builtin_amdgcn_readlane(dsc, 1);
    const int sh = __builtin_amdgcn_readlane(dsc, 2), fc = __builtin_amdgcn_readlane(dsc, 3);

    // ---- append the block (gym_env.py:220-232): LDS copy for this step, global copy for the next ones ----
    if (lane < 4) { L.pose[nb * 4 + lane] = cpose; pose_g[nb * 4 + lane] = cpose; }
    if (lane < MAXV * 2) { L.verts[nb * MAXV * 2 + lane] = cvert; verts_g[nb * MAXV * 2 + lane] = cvert; }
    c.b.state_bits[(size_t)e * IMG + lane] = sbits | cbits;
    __syncthreads();                                // level-0 staging and the new block are in LDS
    if (lane == 0) {
        L.shape_id[nb] = sh;
        shape_id_g[nb] = sh;
        L.occ[nb] = (int32_t)(1u << fc);
        occ_g[nb] = (uint8_t)(1u << fc);
        if (tb >= 0) {
            L.occ[tb] |= (int32_t)(1u << tf);
            occ_g[tb] = (uint8_t)L.occ[tb];
        }
        c.b.n_blocks[e] = nb + 1;
    }
    __syncthreads();
    const bridges_shape* shapes = L.shapes;
    const bridges_shape& shn = shapes[sh];
    // per block: world centroid and volume for the LP (the staging area becomes the tableau), free faces for the
    // candidate count of the next state
    int nf = 0;
    if (lane <= nb) {
        const bridges_shape& sb = shapes[L.shape_id[lane]];
        double rgx, rgz;
        rot2(sb.gx, sb.gz, L.pose[4 * lane + 2], L.pose[4 * lane + 3], rgx, rgz);
        Lk.cen[2 * lane] = L.pose[4 * lane] + rgx;
        Lk.cen[2 * lane + 1] = L.pose[4 * lane + 1] + rgz;
        Lk.vol[lane] = sb.volume;
        nf = sb.nv - __popc((uint32_t)L.occ[lane] & ((1u << sb.nv) - 1u));
    }

    // ---- targets (gym_env.py:163-169, compas Box.contains_point tol 1e-6) ----
    double vx = 0.0, vz = 0.0;
    const int nvn = shn.nv;
    bool hasv = lane < nvn;
    if (hasv) { vx = L.verts[nb * MAXV * 2 + 2 * lane]; vz = L.verts[nb * MAXV * 2 + 2 * lane + 1]; }
    double x0 = wave_min_d(hasv ? vx : 1e300), x1 = wave_max_d(hasv ? vx : -1e300);
    double z0 = wave_min_d(hasv ? vz : 1e300), z1 = wave_max_d(hasv ? vz : -1e300);
    {
        double cx = (x0 + x1) * 0.5, cz = (z0 + z1) * 0.5, hx = (x1 - x0) * 0.5, hz = (z1 - z0) * 0.5;
        double hy = shn.depth * 0.5;
        // the reference removes from targets_remaining while iterating over it (gym_env.py:164-168): CPython's list
        // iterator then skips the element that moves into the freed slot, so the open target after a reached one is not
        // tested for this block.  Reproduced literally (oracle/env.py does the same).
        bool skip = false;
        for (int t = 0; t < c.n_targets; ++t) {
            if (!((left >> t) & 1u)) continue;
            if (skip) { skip = false; continue; }
            bool in;
            if constexpr (PER_ENV) {
                const double tx = readlane_d(tgv, 3 * t), ty = readlane_d(tgv, 3 * t + 1), tz = readlane_d(tgv, 3 * t + 2);
                in = fabs(tx - cx) < hx + 1e-6 && fabs(ty) < hy + 1e-6 && fabs(tz - cz) < hz + 1e-6;
            } else {
                in = fabs(c.targets[t][0] - cx) < hx + 1e-6 && fabs(c.targets[t][1]) < hy + 1e-6 &&
                     fabs(c.targets[t][2] - cz) < hz + 1e-6;
            }
            if (in) { left &= ~(1u << t); skip = true; }
        }
    }
    const int n_reached = c.n_targets - __popc(left);

    // ---- contact interfaces of the new block (assembly_env.py:281-304): its faces against the floor and every
    //      older block's faces, frames computed on the fly from the LDS vertices (same pair order and arithmetic as
    //      append_interfaces / oracle/rbe.py face_pair_contact); hits go to the persistent list and its LDS copy ----
    int n_if = n_if_old;
    bool overflow = false;
    {
        const double* nverts = L.verts + nb * MAXV * 2;
        const int totalp = (1 + nb * MAXV) * MAXV;
        for (int p0 = 0; p0 < totalp; p0 += WAVE) {
            const int p = p0 + lane;
            bool hit = false;
            double g[8];
            int bodyA = -1;
            if (p < totalp) {
                const int qa = p / MAXV, fn = p % MAXV;
                if (fn < shn.nv) {
                    const int ia = shn.fa[fn], ib = shn.fb[fn];
                    const double aBx = nverts[2 * ia], aBz = nverts[2 * ia + 1], bBx = nverts[2 * ib], bBz = nverts[2 * ib + 1];
                    const Frame2 fB = edge_frame(aBx, aBz, bBx, bBz);
                    if (qa == 0) {
                        hit = face_pair_contact_v(-c.floor_hw, 0.0, c.floor_hw, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, aBx, aBz, bBx,
                                                  bBz, fB.cx, fB.cz, fB.nx, fB.nz, fmin(c.floor_depth, shn.depth), g);
                    } else {
                        bodyA = (qa - 1) / MAXV;
                        const int f = (qa - 1) % MAXV;
                        const bridges_shape& sa = shapes[L.shape_id[bodyA]];
                        if (f < sa.nv) {
                            const double* v = L.verts + bodyA * MAXV * 2;
                            const double ax = v[2 * sa.fa[f]], az = v[2 * sa.fa[f] + 1], bx = v[2 * sa.fb[f]], bz = v[2 * sa.fb[f] + 1];
                            const Frame2 fr = edge_frame(ax, az, bx, bz);
                            hit = face_pair_contact_v(ax, az, bx, bz, fr.cx, fr.cz, fr.tx, fr.tz, fr.nx, fr.nz, aBx, aBz, bBx, bBz,
                                                      fB.cx, fB.cz, fB.nx, fB.nz, fmin(sa.depth, shn.depth), g);
                        }
                    }
                }
            }
            const uint64_t bal = __ballot(hit);
            const int idx = n_if + __popcll(bal & ((1ull << lane) - 1ull));
            if (hit && idx < MAXIF) {
                if_body_g[2 * idx] = bodyA;
                if_body_g[2 * idx + 1] = nb;
#pragma unroll
                for (int k = 0; k < 8; ++k) if_geom_g[8 * idx + k] = g[k];
                if (idx < STEP_IF_LDS) {
                    Lk.if_body[2 * idx] = bodyA;
                    Lk.if_body[2 * idx + 1] = nb;
#pragma unroll
                    for (int k = 0; k < 8; ++k) Lk.if_geom[8 * idx + k] = g[k];
                }
            }
            n_if += __popcll(bal);
        }
        if (n_if > MAXIF) { overflow = true; n_if = MAXIF; }
    }
    __syncthreads();

    // ---- stability with the last block frozen / nothing frozen (gym_env.py:238-245, 325-333) ----
    bool err = false;
    bool st_frozen = true, st_free = true;
    bool warm_used = false, resolved = false;
    AsmView A;                                      // centroids / volumes / contacts from LDS; the block arrays are gone
    A.pose = nullptr; A.shape_id = nullptr; A.shapes = nullptr; A.n_blocks = nb + 1;
    A.cand_b = -1; A.cand_pose = nullptr; A.cand_shape = 0; A.cen = Lk.cen; A.vol = Lk.vol; A.n_tens = 0; A.tens_coef = 1.0;
    A.n_if = n_if; A.n_if0 = n_if < STEP_IF_LDS ? n_if : STEP_IF_LDS;
    A.if_body0 = Lk.if_body; A.if_geom0 = Lk.if_geom;
    A.if_body1 = if_body_g + 2 * STEP_IF_LDS; A.if_geom1 = if_geom_g + 8 * STEP_IF_LDS;
    rbe_both(tab, STEP_TAB_LDS, ws, c.b.lp_ws_stride, S, A, n_if_old, W, c.mu, c.density, lane, &st_frozen, &st_free, &err,
             &warm_used, c.b.lp_snap ? c.b.lp_snap + (size_t)e * c.b.lp_snap_stride : nullptr, &resolved);

    // ---- reward / termination (gym_env.py:11-22, 141-145) ----
    const bool all_reached = left == 0;
    const bool terminated = !st_frozen || all_reached;
    // gym_env.py:143; a state that fills its K block slots is truncated as well (without a step limit the reference
    // would go on; the arrays here cannot), so slot nb == K is never written
    const bool truncated = (c.max_steps > 0 && (nb + 1) >= c.max_steps) || (nb + 1) >= K;
    const bool done = terminated || truncated;
    float reward = !st_frozen ? -1.f : (all_reached ? (float)n_reached : (float)(-1 + n_reached));
    float lin = st_free ? base : (st_frozen ? base / 100.f : 0.f);          // successor_dqn.py:397-401

    if (lane == 0) {
        flags[F_VALID] = 1; flags[F_STABLE_FROZEN] = st_frozen; flags[F_STABLE_UNFROZEN] = st_free;
        flags[F_TERMINATED] = terminated; flags[F_TRUNCATED] = truncated; flags[F_DONE] = done;
        flags[F_NO_ACTIONS] = 0; flags[F_LP_ERROR] = (uint8_t)((err ? 1 : 0) | (overflow ? 2 : 0) | (resolved ? 4 : 0));   // bit 2: warm verdict re-solved cold
        c.b.reward[e] = reward;
        c.b.lin_reward[e] = lin;
        c.b.n_reached[e] = n_reached;
        c.b.n_if[e] = n_if;
        c.b.targets_left[e] = left;
    }
    int nb_after = nb + 1;
    if (done) {                                     // auto-reset (after the stores above: same lanes, program order)
        reset_env(c, e, lane);
        nb_after = 0;
    }
    int nfree = 0;
    for (int b = 0; b < nb_after; ++b) nfree += __builtin_amdgcn_readlane(nf, b);
    const int nc = c.n_groups * (c.n_ground + nfree * c.n_offsets);     // raw count: k_scan clamps to a_max and flags a truncation
    if (lane == 0) c.b.n_cand[e] = nc;
}

// ---------------------------------------------------------------------------------------------
// exclusive prefix sum of n_cand -> cand_offset[E+1], the clamp of every env's raw candidate count to the capacity a_max
// (a truncated env gets bit 3 of its F_LP_ERROR flag and is counted), plus the per-lock-step statistics (no atomics anywhere:
// 4096 adds on one word cost ~50 us per kernel on this chip).  Single workgroup of only 4 waves: beside another env
// group's rasteriser (28 of a CU's 32 wave slots taken) a 16-wave workgroup waited ~100 us for a CU to place it.
#define SCAN_THREADS 256
#define SCAN_WAVES (SCAN_THREADS / WAVE)
#define SCAN_BATCH 8        // envs per thread whose loads are in flight together (one round trip per 2048 envs)
__global__ __launch_bounds__(SCAN_THREADS) void k_scan(DevCtx c, int after_step) {
    __shared__ int wave_tot[SCAN_WAVES];
    __shared__ int carry_s;
    __shared__ unsigned long long red[SCAN_WAVES][8];
    __builtin_amdgcn_s_setprio(3);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // blocks, env-steps, reset-only, lp errors, if overflow, valid, warm re-solves, truncated candidate sets
    for (int base0 = 0; base0 < c.E; base0 += SCAN_THREADS * SCAN_BATCH) {
        // all loads of the batch first: beside a rasteriser every dependent round trip costs microseconds
        int v[SCAN_BATCH], nbk[SCAN_BATCH], nval[SCAN_BATCH];
        uint64_t fl8[SCAN_BATCH];
#pragma unroll
        for (int u = 0; u < SCAN_BATCH; ++u) {
            const int i = base0 + u * SCAN_THREADS + t;
            const bool in = i < c.E;
            v[u] = in ? c.b.n_cand[i] : 0;              // raw count of the producer
            nbk[u] = in ? c.b.n_blocks[i] : 0;
            nval[u] = (in && after_step) ? c.b.n_valid[i] : 0;
            fl8[u] = (in && after_step) ? *reinterpret_cast<const uint64_t*>(c.b.step_flags + (size_t)i * 8) : 0ull;
        }
#pragma unroll
        for (int u = 0; u < SCAN_BATCH; ++u) {
            const int base = base0 + u * SCAN_THREADS;
            if (base >= c.E) break;
            const int i = base + t;
            if (i < c.E) {
                if (v[u] > c.a_max) {                        // more candidates than the env has room for: cut, flag, count
                    v[u] = c.a_max;
                    c.b.n_cand[i] = c.a_max;
                    c.b.step_flags[(size_t)i * 8 + F_LP_ERROR] |= 8;
                    acc[7] += 1;
                }
                acc[0] += (unsigned long long)nbk[u];
                if (after_step) {
                    const unsigned valid = (unsigned)(fl8[u] >> (8 * F_VALID)) & 0xffu;
                    const unsigned lperr = (unsigned)(fl8[u] >> (8 * F_LP_ERROR)) & 0xffu;
                    acc[1] += valid ? 1 : 0;
                    acc[2] += valid ? 0 : 1;
                    acc[3] += (lperr & 1) ? 1 : 0;
                    acc[4] += (lperr & 2) ? 1 : 0;
                    acc[5] += (unsigned long long)nval[u];             // valid candidates of the state just left
                    acc[6] += (lperr & 4) ? 1 : 0;                     // a warm 'unstable' was solved again from scratch
                }
            }
            int incl = v[u];                                 // inclusive scan inside the wave
#pragma unroll
            for (int o = 1; o < WAVE; o <<= 1) {
                int up = __shfl_up(incl, o, WAVE);
                if (lane >= o) incl += up;
            }
            if (lane == WAVE - 1) wave_tot[wv] = incl;
            __syncthreads();
            int wbase = 0;
            for (int k = 0; k < wv; ++k) wbase += wave_tot[k];
            const int carry = carry_s;
            if (i < c.E) c.b.cand_offset[i] = carry + wbase + incl - v[u];
            __syncthreads();
            if (t == SCAN_THREADS - 1) carry_s = carry + wbase + incl;
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        unsigned long long x = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
        if (lane == 0) red[wv][k] = x;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int w = 0; w < SCAN_WAVES; ++w)
            for (int k = 0; k < 8; ++k) tot[k] += red[w][k];
        c.b.cand_offset[c.E] = carry_s;
        if (c.h_total) *c.h_total = carry_s;
        c.b.stats[ST_SUM_CAND] += (uint64_t)carry_s;
        c.b.stats[ST_SUM_BLOCKS] += tot[0];
        c.b.stats[ST_ENV_STEPS] += tot[1];
        c.b.stats[ST_RESET_ONLY] += tot[2];
        c.b.stats[ST_LP_ERRORS] += tot[3];
        c.b.stats[ST_IF_OVERFLOW] += tot[4];
        c.b.stats[ST_SUM_VALID] += tot[5];
        c.b.stats[ST_WARM_RESOLVED] += tot[6];
        c.b.stats[ST_CAND_OVERFLOW] += tot[7];
        c.b.stats[ST_LOCKSTEPS] += 1;
    }
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_enumerate(DevCtx c) {
    __shared__ uint8_t free_b[MAXK * MAXV], free_f[MAXK * MAXV];
    __shared__ bridges_shape sh_l[8];
    __shared__ double verts_l[MAXK * MAXV * 2];
    __shared__ int32_t shape_l[MAXK], occ_l[MAXK];
    __shared__ double xg_l[32], offs_l[8];
    __builtin_amdgcn_s_setprio(3);
    const int e = blockIdx.x, lane = threadIdx.x;
    const int K = c.K;
    // everything the env id addresses is requested at once and staged in LDS (see k_step)
    if (lane < 32) xg_l[lane] = c.tt->x_ground[lane];
    if (lane < 8) offs_l[lane] = c.tt->offsets[lane];
    const int nb = c.b.n_blocks[e];
    const int ncand = c.b.n_cand[e];
    const size_t off = (size_t)c.b.cand_offset[e];
    {
        const double* src = reinterpret_cast<const double*>(c.tt->shapes);
        double* dst = reinterpret_cast<double*>(sh_l);
        const int nd = c.n_shapes * (int)(sizeof(bridges_shape) / 8);
        for (int i = lane; i < nd; i += WAVE) dst[i] = src[i];
        const double* vg = c.b.blk_verts + (size_t)e * K * MAXV * 2;
        for (int i = lane; i < nb * MAXV * 2; i += WAVE) verts_l[i] = vg[i];
        if (lane < K) { shape_l[lane] = c.b.blk_shape[(size_t)e * K + lane]; occ_l[lane] = c.b.blk_occ[(size_t)e * K + lane]; }
    }
    __syncthreads();
    const bridges_shape* shapes = sh_l;
    const int32_t* shape_id = shape_l;
    const double* verts = verts_l;
    // free (block, face) list in (block, face) order (actions.py:28-45)
    int nfree = 0;
    for (int i0 = 0; i0 < nb * MAXV; i0 += WAVE) {
        int i = i0 + lane;
        bool fr = false;
        int b = i / MAXV, f = i % MAXV;
        if (i < nb * MAXV) {
            int nv = shapes[shape_id[b]].nv;
            fr = f < nv && !((occ_l[b] >> f) & 1);
        }
        uint64_t bal = __ballot(fr);
        if (fr) {
            int idx = nfree + __popcll(bal & ((1ull << lane) - 1ull));
            free_b[idx] = (uint8_t)b;
            free_f[idx] = (uint8_t)f;
        }
        nfree += __popcll(bal);
    }
    __syncthreads();
    const int gsize = c.n_ground + nfree * c.n_offsets;
    for (int a = lane; a < ncand; a += WAVE) {
        int grp = a / gsize, slot = a % gsize;
        int sh = c.group_shape[grp], fc = c.group_face[grp];
        int tb = -1, tf = 0;
        double ox;
        Frame2 f1;
        if (slot < c.n_ground) {
            ox = xg_l[slot];
            f1.cx = 0.0; f1.cz = 0.0; f1.tx = 1.0; f1.tz = 0.0; f1.nx = 0.0; f1.nz = 1.0;   // assembly_env.py:339-340
        } else {
            int k = (slot - c.n_ground) / c.n_offsets;
            ox = offs_l[(slot - c.n_ground) % c.n_offsets];
            tb = free_b[k]; tf = free_f[k];
            const bridges_shape& st = shapes[shape_id[tb]];
            const double* v = verts + (size_t)tb * MAXV * 2;
            f1 = edge_frame(v[2 * st.fa[tf]], v[2 * st.fa[tf] + 1], v[2 * st.fb[tf]], v[2 * st.fb[tf] + 1]);
        }
        const bridges_shape& sn = shapes[sh];
        double px, pz, cs, sn_;
        align_place(f1, sn.fcx[fc], sn.fcz[fc], sn.fnx[fc], sn.fnz[fc], ox, 0.0, px, pz, cs, sn_);
        const size_t ci = off + a;
        bool inb = true;
        const double eps = 1e-6;
        double wx[MAXV], wz[MAXV];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            wx[i] = 0.0; wz[i] = 0.0;
            if (i < sn.nv) {
                double rx, rz;
                rot2(sn.vx[i], sn.vz[i], cs, sn_, rx, rz);
                wx[i] = px + rx; wz[i] = pz + rz;
                if (wx[i] < c.xlim0 - eps || wx[i] > c.xlim1 + eps || wz[i] < c.ylim0 - eps || wz[i] > c.ylim1 + eps) inb = false;
                if (wz[i] < -eps) inb = false;
            }
            c.b.cand_verts[ci * MAXV * 2 + 2 * i] = wx[i];
            c.b.cand_verts[ci * MAXV * 2 + 2 * i + 1] = wz[i];
        }
        // world face frames (oracle: Block.frames) for the rasteriser
        {
#define PICK6(v, k) ((k) == 5 ? v[5] : (k) == 4 ? v[4] : (k) == 3 ? v[3] : (k) == 2 ? v[2] : (k) == 1 ? v[1] : v[0])
#pragma unroll
            for (int f = 0; f < MAXV; ++f) {
                double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0;
                if (f < sn.nv) {
                    const int ia = sn.fa[f], ib = sn.fb[f];
                    const double ax = PICK6(wx, ia), az = PICK6(wz, ia), bx = PICK6(wx, ib), bz = PICK6(wz, ib);
                    Frame2 fr = edge_frame(ax, az, bx, bz);
                    o0 = fr.cx; o1 = fr.cz; o2 = fr.nx; o3 = fr.nz;
                }
                double2* dst = reinterpret_cast<double2*>(c.b.cand_frames + (ci * MAXV + f) * 4);
                dst[0] = make_double2(o0, o1);
                dst[1] = make_double2(o2, o3);
            }
#undef PICK6
            c.b.cand_rows[ci * 2 + 0] = (sn.nv << 16) | ((inb ? 1 : 0) << 24);   // packed for the rasteriser (bits 0-15: unused)
            c.b.cand_rows[ci * 2 + 1] = e;
        }
        c.b.cand_pose[ci * 4 + 0] = px; c.b.cand_pose[ci * 4 + 1] = pz;
        c.b.cand_pose[ci * 4 + 2] = cs; c.b.cand_pose[ci * 4 + 3] = sn_;
        c.b.cand_desc[ci * 4 + 0] = tb; c.b.cand_desc[ci * 4 + 1] = tf;
        c.b.cand_desc[ci * 4 + 2] = sh; c.b.cand_desc[ci * 4 + 3] = fc;
        c.b.cand_ox[ci] = ox;
        c.b.cand_inb[ci] = inb;
        c.b.cand_env[ci] = e;
    }
}

// ---------------------------------------------------------------------------------------------
// f32 expansion of a 64x64 bit raster held one row per lane: 16 wave-wide float4 stores of 1 KiB.
// With nz != nullptr (sparse update) only the row groups that hold pixels now or held pixels the last time this slot
// was written are stored -- the rest of the slot is zero already -- and *nz is replaced by the new group mask.
__device__ __forceinline__ void write_f32_image(float* img, uint64_t rowbits, int lane, int32_t* nz = nullptr) {
    const int sub = lane >> 4, col4 = (lane & 15) * 4;
    const uint64_t nonzero_rows = __ballot(rowbits != 0ull);       // most of a raster is empty rows
    if (nz) {
        uint64_t t = nonzero_rows | (nonzero_rows >> 1);
        t = (t | (t >> 2)) & 0x1111111111111111ull;                // bit 4g = any of rows 4g..4g+3
        uint32_t now = 0u;
#pragma unroll
        for (int g = 0; g < IMG / 4; ++g) now |= (uint32_t)((t >> (4 * g)) & 1ull) << g;
        uint32_t need = (uint32_t)__builtin_amdgcn_readfirstlane(*nz) | now;
        if (lane == 0) *nz = (int32_t)now;
        while (need) {
            const int g = __builtin_ctz(need);
            need &= need - 1u;
            uint32_t nib = 0u;
            if ((now >> g) & 1u) {
                uint64_t m = shfl_u64(rowbits, 4 * g + sub);
                nib = (uint32_t)(m >> col4) & 0xFu;
            }
            float4 v;
            v.x = (nib & 1u) ? 1.f : 0.f;
            v.y = (nib & 2u) ? 1.f : 0.f;
            v.z = (nib & 4u) ? 1.f : 0.f;
            v.w = (nib & 8u) ? 1.f : 0.f;
            *reinterpret_cast<float4*>(img + (size_t)(4 * g + sub) * IMG + col4) = v;
        }
        return;
    }
#pragma unroll
    for (int r0 = 0; r0 < IMG; r0 += 4) {
        uint32_t nib = 0u;
        if ((nonzero_rows >> r0) & 0xFull) {
            uint64_t m = shfl_u64(rowbits, r0 + sub);
            nib = (uint32_t)(m >> col4) & 0xFu;
        }
        float4 v;
        v.x = (nib & 1u) ? 1.f : 0.f;
        v.y = (nib & 2u) ? 1.f : 0.f;
        v.z = (nib & 4u) ? 1.f : 0.f;
        v.w = (nib & 8u) ? 1.f : 0.f;
        *reinterpret_cast<float4*>(img + (size_t)(r0 + sub) * IMG + col4) = v;
    }
}

// Rasterise one convex outline from its world face frames (centre.xz, outward normal.xz per face) WITHOUT visiting
// pixels.  The reference's pixel test (assembly_env.py:126-137 through oracle/raster.py) is, per face,
//     d = ((X[x] - c.x) * n.x) + ((Y[r] - c.z) * n.z) <= 0
// with separately rounded binary64 operations.  With a[x] = fl(fl(X[x] - c.x) * n.x) and b[r] = fl(fl(Y[r] - c.z) * n.z)
// the rounded sum fl(a + b) is <= 0 exactly when the exact sum is (rounding is monotone and never turns a non-zero
// sum of two doubles into zero), i.e. when  a[x] <= -b[r]  -- one comparison, no addition.  X = np.linspace is strictly
// increasing, rounding is monotone, so a[x] is monotone in x (non-decreasing for n.x > 0, non-increasing for n.x < 0,
// constant +-0 for n.x = 0): the pixels of row r that pass face f form a prefix or a suffix of the row, whose length is
// found by a 7-probe binary search over a[.] with exactly the reference's comparison.  The row of the raster is the
// intersection of those runs.  Lane x holds a[x] (column role) and lane r holds -b[r] (row role); every lane searches
// for its own row, so all 64 rows of the image come out at once (row r in lane r) with ~50 wave instructions per face,
// independent of the block's size, instead of ~30 per face-row pair in a loop over the rows.  Bit for bit the same
// raster as the per-pixel test (tests/test_gpu_env_parity.py against oracle/raster.py).
// fr0..fr3: lane f < NF holds centre.x, centre.z, normal.x, normal.z of face f (all-zero frames pass every pixel).
// X / Y: this lane's column / row coordinate (lanes >= n_img repeat the last grid value); n_img = S <= 64.
__device__ __forceinline__ uint64_t low_mask64(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

template <int NF, int F0 = 0>
__device__ __forceinline__ uint64_t raster_rows(double fr0, double fr1, double fr2, double fr3, int n_img, double X, double Y,
                                                int lane) {
    int alo[NF], ahi[NF], pos[NF];
    double t[NF];
    bool rev[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const double cxf = readlane_d(fr0, F0 + f), czf = readlane_d(fr1, F0 + f), nxf = readlane_d(fr2, F0 + f), nzf = readlane_d(fr3, F0 + f);
        const double a = (X - cxf) * nxf;               // column role
        t[f] = -((Y - czf) * nzf);                      // row role: pixel (r, x) passes face f iff a[x] <= t[r]
        alo[f] = __double2loint(a);
        ahi[f] = __double2hiint(a);
        rev[f] = nxf < 0.0;                             // wave-uniform: a[.] non-increasing, the run is a suffix
        pos[f] = 0;
    }
    // probes at pos + s - 1 for s = 32 .. 1 (pos = the largest count <= 63 the run supports), then at pos itself (64)
#define RASTER_PROBE(S_, INC_)                                                                                          \
    _Pragma("unroll") for (int f = 0; f < NF; ++f) {                                                                    \
        const int j = pos[f] + (S_);                                                                                    \
        const int src = rev[f] ? 63 - j : j;                                                                            \
        const double av = __hiloint2double(__shfl(ahi[f], src, WAVE), __shfl(alo[f], src, WAVE));                       \
        if (av <= t[f]) pos[f] += (INC_);                                                                               \
    }
    RASTER_PROBE(31, 32) RASTER_PROBE(15, 16) RASTER_PROBE(7, 8) RASTER_PROBE(3, 4) RASTER_PROBE(1, 2) RASTER_PROBE(0, 1)
    RASTER_PROBE(0, 1)
#undef RASTER_PROBE
    uint64_t bits = low_mask64(n_img);                  // images narrower than the canvas: columns >= S stay empty
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const uint64_t run = low_mask64(pos[f]);
        bits &= rev[f] ? (pos[f] ? ~low_mask64(64 - pos[f]) : 0ull) : run;
    }
    return lane < n_img ? bits : 0ull;                  // rows >= S stay empty
}

// six faces as two batches of three (the searches of a batch run interleaved; one batch of six keeps 30 values per lane
// alive and costs the kernel two of its eight waves per SIMD)
__device__ __forceinline__ uint64_t raster_rows6(double fr0, double fr1, double fr2, double fr3, int n_img, double X, double Y, int lane) {
    return raster_rows<3, 0>(fr0, fr1, fr2, fr3, n_img, X, Y, lane) & raster_rows<3, 3>(fr0, fr1, fr2, fr3, n_img, X, Y, lane);
}

__device__ __forceinline__ uint64_t raster_rows_nv(double fr0, double fr1, double fr2, double fr3, int nv, int n_img, double X,
                                                   double Y, int lane) {
    return nv <= 4 ? raster_rows<4>(fr0, fr1, fr2, fr3, n_img, X, Y, lane) : raster_rows6(fr0, fr1, fr2, fr3, n_img, X, Y, lane);
}

// sum(raster * reward_map) from the row runs: the pixels of a row of a convex outline are one run [lo, hi), so the
// row's sum is prefix[r][hi] - prefix[r][lo] on the float64 row prefix sums of the reward map (reward_prefix, [64][65]).
// Two steps, so that the caller can put the image's 16 KiB of stores between the two gathers and their use (the loads
// are in flight under the stores instead of in front of them).
__device__ __forceinline__ void raster_reward_fetch(uint64_t rowbits, const double* prefix, int lane, double& p_hi, double& p_lo) {
    p_hi = 0.0; p_lo = 0.0;
    if (rowbits) {
        const int lo = __builtin_ctzll(rowbits), hi = 64 - __builtin_clzll(rowbits);
        const double* p = prefix + lane * (IMG + 1);
        p_hi = p[hi]; p_lo = p[lo];
    }
}
__device__ __forceinline__ double raster_reward_sum(double p_hi, double p_lo) { return wave_sum_d(p_hi - p_lo); }

// Same from world vertices (stand-alone operator): frames are derived first (oracle/raster.py contains_2d).
__device__ __forceinline__ uint64_t raster_outline(const double* v /*[6,2]*/, int nv, const int32_t* fa,
                                                   const int32_t* fb, const double* gx, const double* gy, int size, int lane) {
    double cx = 0.0, cz = 0.0, nx = 0.0, nz = 0.0;
    if (lane < nv) {
        Frame2 fr = edge_frame(v[2 * fa[lane]], v[2 * fa[lane] + 1], v[2 * fb[lane]], v[2 * fb[lane] + 1]);
        cx = fr.cx; cz = fr.cz; nx = fr.nx; nz = fr.nz;
    }
    const int g = lane < size ? lane : size - 1;        // lanes beyond the image repeat the last grid value (a[.] stays monotone)
    return raster_rows_nv(cx, cz, nx, nz, nv, size, gx[g], gy[g], lane);
}

// Rasteriser: work item i < total -> candidate i (compact index), else the state raster of env i - total.  One
// wave per image.  The grid is sized by the host from the previous lock-step's candidate count (kept in pinned
// memory) so that a wave sees about one item -- short-lived waves dispatched in item order keep the HBM write
// stream close to linear, which sustains ~14 % more bandwidth than a persistent grid (tools/store_bench.hip) -- and
// the grid-stride loop makes any count correct.  The row runs (raster_rows) cost ~250 wave instructions per image and
// hide behind its 16 KiB of stores.
// NF = 4 when every candidate shape of the task has at most 4 faces (64 VGPRs: 8 waves per SIMD), else MAXV.
// PER_ENV: reward_prefix holds one [64][65] table per env (bridges_task_buffers); the owning env is wave-uniform, so the
// table's base is scalar arithmetic.
// k_raster<NF, true, const uint64_t*>(DevCtx, env_obstacle_bits): per-env obstacles (bridges_task_buffers.env_obstacle_bits,
// [E][64]): the obstacle rows are read per work item beside the state's, from env_obst[e * 64 + lane] (e is wave-uniform: a
// scalar base again), instead of once per wave from the shared raster.  The source is a compile-time choice, made as k_step
// makes its own: the optional trailing argument leaves the two instantiations without per-env obstacles their argument list,
// their hoisted load and their code (compared with the previous build's assembly in docs/MEASUREMENT_LOG.md).
__device__ __forceinline__ const uint64_t* raster_env_obst() { return nullptr; }
__device__ __forceinline__ const uint64_t* raster_env_obst(const uint64_t* p) { return p; }
template <int NF, bool PER_ENV = false, typename... ENV_OBST_ARG>
__global__ __launch_bounds__(256) void k_raster(DevCtx c, ENV_OBST_ARG... env_obst_arg) {
    constexpr bool ENV_OBST = sizeof...(ENV_OBST_ARG) == 1;
    const uint64_t* env_obst = raster_env_obst(env_obst_arg...);
    (void)env_obst;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int nwaves = (gridDim.x * blockDim.x) / WAVE;
    const int total = c.b.cand_offset[c.E];
    const int items = total + (c.b.state_raster ? c.E : 0);
    const double X = c.tt->grid_x[lane], Y = c.tt->grid_y[lane];
    const uint64_t obst = ENV_OBST ? 0ull : c.b.obstacle_bits[lane];
    for (int itv = wave; itv < items; itv += nwaves) {
        const int it = __builtin_amdgcn_readfirstlane(itv);       // wave-uniform: metadata comes through scalar loads
        if (it < total) {
            const size_t ci = (size_t)it;
            const int meta = c.b.cand_rows[ci * 2];
            const int e = c.b.cand_rows[ci * 2 + 1];
            const int nv = (meta >> 16) & 0xff;
            const bool inb = (meta >> 24) & 1;
            (void)nv;
            // everything the descriptor addresses is requested before any of it is used
            double fr0 = 0.0, fr1 = 0.0, fr2 = 0.0, fr3 = 0.0;
            if (lane < MAXV) {
                const double2* p = reinterpret_cast<const double2*>(c.b.cand_frames + (ci * MAXV + lane) * 4);
                const double2 a = p[0], b = p[1];
                fr0 = a.x; fr1 = a.y; fr2 = b.x; fr3 = b.y;
            }
            const uint64_t occ = c.b.state_bits[(size_t)e * IMG + lane] | (ENV_OBST ? env_obst[(size_t)e * IMG + lane] : obst);
            const uint64_t bits = (NF == 4 || nv <= 4) ? raster_rows<4>(fr0, fr1, fr2, fr3, c.img, X, Y, lane)
                                                       : raster_rows6(fr0, fr1, fr2, fr3, c.img, X, Y, lane);
            const bool overlap = __ballot((bits & occ) != 0ull) != 0ull;
            double p_hi, p_lo;
            raster_reward_fetch(bits, PER_ENV ? c.b.reward_prefix + (size_t)e * (IMG * (IMG + 1)) : c.b.reward_prefix, lane, p_hi, p_lo);
            c.b.cand_bits[ci * IMG + lane] = bits;
            if (c.b.cand_raster)
                write_f32_image(c.b.cand_raster + ci * IMG * IMG, bits, lane, c.b.cand_raster_nz ? c.b.cand_raster_nz + ci : nullptr);
            const double lin = raster_reward_sum(p_hi, p_lo);
            if (lane == 0) {
                c.b.cand_lin[ci] = (float)lin;
                c.b.cand_mask[ci] = (uint8_t)(inb && !overlap);
            }
        } else {
            const int e = it - total;
            write_f32_image(c.b.state_raster + (size_t)e * IMG * IMG, c.b.state_bits[(size_t)e * IMG + lane], lane,
                            c.b.state_raster_nz ? c.b.state_raster_nz + e : nullptr);
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Per-env task features (bridges_task_buffers): tower_setup's draw (assembly_gym/assembly_gym/envs/gym_env.py:64-79) and
// get_task_features (robotoddler/training/successor_dqn.py:67-85), one workgroup per env.
//   TASK_LOAD   every env: env_targets were written by the caller; rebuild the features
//   TASK_RESET  every env: task_episode = 0; with the sampler on, draw the targets of episode 0 first
//   TASK_STEP   after k_step, a sampler on: only the envs k_step has just reset -- finished and auto-reset (F_DONE) or a
//               reset-only lock-step (!F_VALID) -- take the next episode: task_episode += 1, new targets and / or new obstacles
//               (whichever sampler is on; with the obstacle sampler alone the target tables are left as they are); the rest
//               leave at once
// The draw (header comment of bridges_env_set_task_buffers): counter-based, keyed by (seed, global env id, episode, target,
// axis) through splitmix64 with a salt that separates it from the policy's stream (k_select).
// The features restate bridges_hip.vec_env.VecAssemblyGym._task_features + gaussian_reward_map operation for operation, so a
// per-env table is bit-identical to the one a fixed-task env of the same targets gets from the host:
//   raster   the T cube06 blocks at identity rotation (vertex = target + local vertex) through raster_outline, rows OR-ed;
//   map      out[y][x] = (float) sum over the set pixels (py, px) of the raster, row-major, of (double)(k[py - y + 50] * k[px - x + 50])
//            -- the float32 product first (the reference's kernel matrix k k^T is float32), a float64 running sum, taps
//            outside the 101-wide kernel contribute nothing, one rounding to float32.  Lane x owns column x and walks rows y: every
//            output pixel is its own sum, so the order is the host's for free;
//   prefix   [r][x + 1] = [r][x] + (double)map[r][x], left to right (np.cumsum), lane r owns row r.
// Work: <= 16 T set pixels x 4096 outputs of float64 adds per env that changes task, a chain of dependent adds per output.
// One workgroup of four waves per env: every wave repeats the (cheap) draw and raster, then wave w takes map rows 16 w ..
// 16 w + 15, four rows at a time per lane -- four independent sums in flight, one LDS read of k per set pixel for the four.
// k sits in LDS between zeros (kz), so a tap outside the 101-wide kernel reads 0: the sum takes (double)(0 * k) = +0.0, which
// changes nothing, exactly what the host adds there.  LDS 51 KB: map and prefix tables are staged so that their 49 KiB leave
// as contiguous stores.
enum { TASK_LOAD = 0, TASK_RESET = 1, TASK_STEP = 2 };
#define TASK_SALT 0x7461736B5F726E67ull     // "task_rng"
#define OBST_SALT 0x6F6273745F726E67ull     // "obst_rng"
#define TASK_ROW (IMG + 1)
#define TASK_WAVES 4
#define TASK_THREADS (TASK_WAVES * WAVE)
#define TASK_ROWS_IN_FLIGHT 4
#define TASK_KZ_PAD 16                      // zeros in front of k: tap index py - y + 50 >= -13 on a 64-pixel canvas
#define TASK_KZ (TASK_KZ_PAD + BRIDGES_GAUSS_TAPS + 16)      // and <= 113
static_assert(IMG - 1 - BRIDGES_GAUSS_TAPS / 2 <= TASK_KZ_PAD && IMG - 1 + BRIDGES_GAUSS_TAPS / 2 < BRIDGES_GAUSS_TAPS + 16,
              "every tap index of a 64 x 64 canvas must fall into the padded table");
static_assert(IMG % (TASK_WAVES * TASK_ROWS_IN_FLIGHT) == 0, "map rows are dealt to the waves in batches");
// Task families (bridges_task_family, header comment of bridges_env_set_task_family): k_task_features<bridges_task_family>
// draws ONE integer n per env and episode -- a stream of its own (FAMI_SALT), integer arithmetic only -- and writes the target
// and the obstacles that n names in place of the uniform draws; unused obstacle slots are parked at z = BRIDGES_PARK_Z, where
// the cube rasterises to nothing.  The optional trailing argument keeps the kernel without a family what it was.
#define FAMI_SALT 0x66616D695F726E67ull     // "fami_rng"
// The class draw of a family, in one place (k_task_features<bridges_task_family...> and the stand-alone k_family_draw): the word
// r of (seed, global env id, episode) on the family's stream, u = r >> 32, and
//   thr == nullptr:  n = n_lo + ((u * C) >> 32)                         C = n_hi - n_lo + 1  (the uniform draw)
//   thr [C - 1]:     n = n_lo + #{k in 0..C-2 : u >= thr[k]}            (weighted: header comment of
//                                                                        bridges_env_set_family_thresholds)
// Integer arithmetic only.  thr is read with plain loads at every draw: a kernel earlier in the stream may have rewritten it.
__device__ __forceinline__ int family_class(uint64_t seed, uint32_t gid, uint32_t ep, int n_lo, int n_hi, const uint64_t* thr) {
    const uint64_t h0 = splitmix64((((seed & 0xFFFFFFFFull) << 32) | gid) ^ FAMI_SALT);
    const uint64_t h1 = splitmix64(h0 ^ (uint64_t)ep);
    const uint64_t r = splitmix64(h1);
    const uint64_t u = r >> 32;
    const int C = n_hi - n_lo + 1;
    if (!thr) return n_lo + (int)((u * (uint64_t)C) >> 32);
    int n = n_lo;
    for (int k = 0; k < C - 1; ++k) n += u >= thr[k] ? 1 : 0;
    return n;
}
__device__ __forceinline__ bridges_task_family task_family() { return bridges_task_family{}; }
__device__ __forceinline__ bridges_task_family task_family(const bridges_task_family& f) { return f; }
__device__ __forceinline__ bridges_task_family task_family(const bridges_task_family& f, const uint64_t*) { return f; }
__device__ __forceinline__ const uint64_t* task_thresholds() { return nullptr; }
__device__ __forceinline__ const uint64_t* task_thresholds(const bridges_task_family&) { return nullptr; }
__device__ __forceinline__ const uint64_t* task_thresholds(const bridges_task_family&, const uint64_t* thr) { return thr; }
// The reward map of a target raster and its row prefix sums, into LDS (the arithmetic above): every thread of the four waves
// calls it with its wave's copy of the raster rows `bits` (row r in lane r) after wave 0 has put them into tb_l and the
// workgroup has met.  STORE_MAP: the map goes to map_g [64][64] as well.  Returns with map_l and pre_l complete and visible.
// k_task_features and the hindsight relabelling (hindsight_kernels.hip) share it, so a relabelled task's tables are an env's.
template <bool STORE_MAP>
__device__ __forceinline__ void task_map_prefix(const uint64_t bits, const uint64_t* tb_l, const float* kz, float* map_l, double* pre_l,
                                                const int S, const int lane, const int wv, float* map_g) {
    // ---- reward map: lane = column x, wave wv = rows 16 wv .. 16 wv + 15 ----
    const uint64_t nzrows = __ballot(bits != 0ull);
    const int half = BRIDGES_GAUSS_TAPS / 2;
    for (int b = 0; b < IMG / (TASK_WAVES * TASK_ROWS_IN_FLIGHT); ++b) {
        const int y0 = (wv * (IMG / TASK_WAVES)) + b * TASK_ROWS_IN_FLIGHT;
        double acc[TASK_ROWS_IN_FLIGHT];
#pragma unroll
        for (int r = 0; r < TASK_ROWS_IN_FLIGHT; ++r) acc[r] = 0.0;
        uint64_t rows = y0 < S ? nzrows : 0ull;
        while (rows) {                              // set pixels in row-major order
            const int py = __builtin_ctzll(rows);
            rows &= rows - 1ull;
            float ki[TASK_ROWS_IN_FLIGHT];
#pragma unroll
            for (int r = 0; r < TASK_ROWS_IN_FLIGHT; ++r) ki[r] = kz[py - (y0 + r) + half + TASK_KZ_PAD];
            const uint64_t row = tb_l[py];
            uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(row >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)row);
            while (m) {
                const int pxl = __builtin_ctzll(m);
                m &= m - 1ull;
                const float kx = kz[pxl - lane + half + TASK_KZ_PAD];
#pragma unroll
                for (int r = 0; r < TASK_ROWS_IN_FLIGHT; ++r) {
                    const float prod = ki[r] * kx;
                    acc[r] = acc[r] + (double)prod;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < TASK_ROWS_IN_FLIGHT; ++r) {
            const int y = y0 + r;
            const float v = (lane < S && y < S) ? (float)acc[r] : 0.f;
            map_l[y * TASK_ROW + lane] = v;
            if constexpr (STORE_MAP) map_g[y * IMG + lane] = v;
        }
    }
    __syncthreads();
    // ---- row prefix sums: lane r of wave 0 = row r ----
    if (wv == 0) {
        double run = 0.0;
        pre_l[lane * TASK_ROW] = 0.0;
        for (int x = 0; x < IMG; ++x) {
            run = run + (double)map_l[lane * TASK_ROW + x];
            pre_l[lane * TASK_ROW + x + 1] = run;
        }
    }
    __syncthreads();
}

// FAMILY... is empty (no family), <bridges_task_family> (the uniform draw) or <bridges_task_family, const uint64_t*> (a threshold
// table attached: the weighted draw); the first two are the kernels they were before the third existed.
template <typename... FAMILY>
__global__ __launch_bounds__(TASK_THREADS) void k_task_features(DevCtx c, bridges_task_buffers t, int mode, FAMILY... family_arg) {
    constexpr bool FAM = sizeof...(FAMILY) >= 1;
    const bridges_task_family fam = task_family(family_arg...);
    const uint64_t* const fam_thr = task_thresholds(family_arg...);
    (void)fam;
    (void)fam_thr;
    const bool draw_obstacles = FAM ? true : t.sample_obstacles != 0, draw_targets = FAM ? true : t.sample != 0;
    __shared__ float kz[TASK_KZ];
    __shared__ uint64_t tb_l[IMG];
    __shared__ double tv_l[TASK_WAVES][MAXV * 2];
    __shared__ float map_l[IMG * TASK_ROW];
    __shared__ double pre_l[IMG * TASK_ROW];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const int T = c.n_targets, S = c.img;
    if (mode == TASK_STEP) {
        const uint8_t* fl = c.b.step_flags + (size_t)e * 8;
        if (fl[F_VALID] && !fl[F_DONE]) return;     // mid-episode: the env keeps its task (the whole workgroup leaves)
    }
    for (int i = tid; i < TASK_KZ; i += TASK_THREADS) {
        const int tap = i - TASK_KZ_PAD;
        kz[i] = (tap >= 0 && tap < BRIDGES_GAUSS_TAPS) ? t.gauss_k[tap] : 0.f;
    }
    double* tg = t.env_targets + (size_t)e * T * 3;
    uint32_t ep = 0u;
    if (mode == TASK_STEP) ep = t.task_episode[e] + 1u;
    __syncthreads();                                // every wave has read the episode before it is replaced
    if (mode != TASK_LOAD && tid == 0) t.task_episode[e] = ep;
    int fam_n = 0;                                  // the env's span / height of this episode (every thread draws it)
    if constexpr (FAM) {
        if (mode != TASK_LOAD) {
            fam_n = family_class(c.seed, (uint32_t)(c.env_id_base + e), ep, fam.n_lo, fam.n_hi, fam_thr);
            if (tid == 0) fam.task_class[e] = fam_n;
        }
    }
    const bridges_shape& cube = c.tt->shapes[t.target_shape];
    const int nv = cube.nv;
    // ---- per-env obstacles (n_obstacles > 0): lane 3 o + k of every wave holds coordinate k of obstacle o; drawn like the
    // targets on a stream of its own (OBST_SALT) with one range pair per obstacle, rasterised exactly as the target blocks ----
    const int O = t.n_obstacles;
    if (O > 0 && (mode != TASK_STEP || draw_obstacles)) {     // fixed obstacles keep their raster over episode boundaries
        double* og = t.env_obstacles + (size_t)e * O * 3;
        double ov = 0.0;
        if (lane < 3 * O) {
            if (draw_obstacles && mode != TASK_LOAD) {
                const int axis = lane % 3, o = lane / 3;
                if constexpr (FAM) {
                    const double half = fam.size / 2.0;
                    if (o >= fam_n) {
                        ov = axis == 2 ? BRIDGES_PARK_Z : 0.0;
                    } else if (fam.family == BRIDGES_FAMILY_SPAN) {
                        const double ox = (double)(o + 1) * fam.size;
                        ov = axis == 0 ? ox : (axis == 2 ? half : 0.0);
                    } else {
                        const double oz = (double)o * fam.size;
                        ov = axis == 0 ? fam.x : (axis == 2 ? oz + half : 0.0);
                    }
                } else if (axis != 1) {
                    const uint64_t h0 = splitmix64((((c.seed & 0xFFFFFFFFull) << 32) | (uint32_t)(c.env_id_base + e)) ^ OBST_SALT);
                    const uint64_t h1 = splitmix64(h0 ^ (uint64_t)ep);
                    const uint64_t r = splitmix64(h1 ^ (uint64_t)lane);
                    const double u = (double)(r >> 11) * 0x1.0p-53;
                    double lo = 0.0, hi = 0.0;
#pragma unroll
                    for (int k = 0; k < BRIDGES_MAX_OBSTACLES; ++k)     // selects: the ranges are kernel arguments
                        if (o == k) {
                            lo = axis == 0 ? t.obs_x_range[k][0] : t.obs_z_range[k][0];
                            hi = axis == 0 ? t.obs_x_range[k][1] : t.obs_z_range[k][1];
                        }
                    const double span = hi - lo;
                    const double step = span * u;
                    ov = lo + step;
                }
                if (wv == 0) og[lane] = ov;
            } else {
                ov = og[lane];
            }
        }
        uint64_t obits = 0ull;
        for (int q = 0; q < O; ++q) {
            const double px = readlane_d(ov, 3 * q), pz = readlane_d(ov, 3 * q + 2);
            __syncthreads();
            if (lane < nv) { tv_l[wv][2 * lane] = px + cube.vx[lane]; tv_l[wv][2 * lane + 1] = pz + cube.vz[lane]; }
            __syncthreads();
            obits |= raster_outline(tv_l[wv], nv, cube.fa, cube.fb, c.tt->grid_x, c.tt->grid_y, S, lane);
        }
        if (wv == 0) t.env_obstacle_bits[(size_t)e * IMG + lane] = obits;
        // obstacle sampler alone: the env begins an episode under its old targets -- target_bits, map and prefix stay
        if (mode == TASK_STEP && !draw_targets) return;
    }
    // ---- targets: lane 3 q + k of every wave holds coordinate k of target q ----
    double tv = 0.0;
    if (lane < 3 * T) {
        if (draw_targets && mode != TASK_LOAD) {
            const int axis = lane % 3;
            if constexpr (FAM) {                    // n_targets == 1: lanes 0..2
                const double half = fam.size / 2.0, run = (double)fam_n * fam.size;
                if (fam.family == BRIDGES_FAMILY_SPAN) {
                    const double lead = 2.5 * fam.size;
                    tv = axis == 0 ? run + lead : (axis == 2 ? half : 0.0);
                } else {
                    tv = axis == 0 ? fam.x : (axis == 2 ? run + half : 0.0);
                }
            } else if (axis != 1) {
                const uint64_t h0 = splitmix64((((c.seed & 0xFFFFFFFFull) << 32) | (uint32_t)(c.env_id_base + e)) ^ TASK_SALT);
                const uint64_t h1 = splitmix64(h0 ^ (uint64_t)ep);
                const uint64_t r = splitmix64(h1 ^ (uint64_t)lane);
                const double u = (double)(r >> 11) * 0x1.0p-53;
                const double lo = axis == 0 ? t.x_range[0] : t.z_range[0], hi = axis == 0 ? t.x_range[1] : t.z_range[1];
                const double span = hi - lo;
                const double step = span * u;
                tv = lo + step;
            }
            if (wv == 0) tg[lane] = tv;
        } else {
            tv = tg[lane];
        }
    }
    // ---- raster of the target blocks (every wave, on its own vertex scratch) ----
    uint64_t bits = 0ull;
    for (int q = 0; q < T; ++q) {
        const double px = readlane_d(tv, 3 * q), pz = readlane_d(tv, 3 * q + 2);
        __syncthreads();
        if (lane < nv) { tv_l[wv][2 * lane] = px + cube.vx[lane]; tv_l[wv][2 * lane + 1] = pz + cube.vz[lane]; }
        __syncthreads();
        bits |= raster_outline(tv_l[wv], nv, cube.fa, cube.fb, c.tt->grid_x, c.tt->grid_y, S, lane);
    }
    if (wv == 0) {
        tb_l[lane] = bits;
        t.target_bits[(size_t)e * IMG + lane] = bits;
    }
    __syncthreads();
    task_map_prefix<true>(bits, tb_l, kz, map_l, pre_l, S, lane, wv, t.reward_map + (size_t)e * IMG * IMG);
    double* pre_g = t.reward_prefix + (size_t)e * IMG * TASK_ROW;
    for (int i = tid; i < IMG * TASK_ROW; i += TASK_THREADS) pre_g[i] = pre_l[i];
}

// ---------------------------------------------------------------------------------------------
// Weighted families and the curriculum (header comments of bridges_family_thresholds / _draw / _curriculum).
// The stand-alone class draw: thread i draws the class of env env_id_base + i in its episode episode[i].
constexpr int FAMILY_MAX_CLASSES = 8;
constexpr uint32_t FAMILY_MAX_WEIGHT = 1u << 20;
constexpr int FAMILY_DRAW_THREADS = 256;
__global__ __launch_bounds__(FAMILY_DRAW_THREADS) void k_family_draw(uint64_t seed, int env_id_base, int E,
                                                                     const uint32_t* __restrict__ episode, int n_lo, int n_hi,
                                                                     const uint64_t* thr, int32_t* __restrict__ n_out) {
    const int i = blockIdx.x * FAMILY_DRAW_THREADS + threadIdx.x;
    if (i >= E) return;
    n_out[i] = family_class(seed, (uint32_t)(env_id_base + i), episode[i], n_lo, n_hi, thr);
}

// thr[k] = ceil((w[0] + .. + w[k]) * 2^32 / sum(w)), k = 0..C-2, in exact integer arithmetic: a weight is at most 2^20 (a larger
// one is taken as 2^20) and C <= 8, so a partial sum is < 2^24 and its product with 2^32 < 2^56.  sum(w) == 0 cannot be refused
// from inside the stream: the table of equal weights is written instead.  One thread: seven 64-bit divisions.
__device__ void family_thresholds_from_weights(const uint32_t* w, int C, uint64_t* thr) {
    uint64_t sum = 0;
    for (int k = 0; k < C; ++k) sum += w[k] < FAMILY_MAX_WEIGHT ? w[k] : FAMILY_MAX_WEIGHT;
    const bool equal = sum == 0;
    if (equal) sum = (uint64_t)C;
    uint64_t cum = 0;
    for (int k = 0; k < C - 1; ++k) {
        cum += equal ? 1u : (w[k] < FAMILY_MAX_WEIGHT ? w[k] : FAMILY_MAX_WEIGHT);
        thr[k] = ((cum << 32) + sum - 1) / sum;
    }
}

__global__ __launch_bounds__(WAVE) void k_family_thresholds(const uint32_t* w, int C, uint64_t* thr) {
    if (blockIdx.x == 0 && threadIdx.x == 0) family_thresholds_from_weights(w, C, thr);
}

// The curriculum update.  ONE workgroup of one wave; lane k < C owns class n = n_lo + k: row n of sums [n_classes, 8] (the
// layout of k_episode_stats: slot 0 = episodes, slot 5 = successes) and row n of state [n_classes, 2] = (ema, seen).
//   e = sums[n][0];  e >= min_episodes:  rate = sums[n][5] / e;  ema = seen ? ema + beta * (rate - ema) : rate  (every operation
//   rounded to binary64 on its own);  seen = 1;  the row of sums is zeroed.  A row below min_episodes stays and accumulates.
//   fail = seen ? min(max(1 - ema, 0), 1) : 1;   w[k] = w_min + (uint32)(fail * 65536.0 + 0.5)
// Then lane 0 builds thr from w (family_thresholds_from_weights).  Rows outside [n_lo, n_hi] are neither read nor written.
// Fixed order, no atomics, no allocation.
__global__ __launch_bounds__(WAVE) void k_family_curriculum(double* __restrict__ sums, double* __restrict__ state, int n_lo, int n_hi,
                                                           double beta, uint32_t w_min, int min_episodes, uint32_t* __restrict__ w,
                                                           uint64_t* __restrict__ thr) {
    __shared__ uint32_t w_l[FAMILY_MAX_CLASSES];
    const int k = threadIdx.x, C = n_hi - n_lo + 1;
    if (k < C) {
        double* row = sums + (size_t)(n_lo + k) * 8;
        double* st = state + (size_t)(n_lo + k) * 2;
        double ema = st[0];
        bool seen = st[1] != 0.0;
        const double e = row[0];
        if (e >= (double)min_episodes) {
            const double rate = __ddiv_rn(row[5], e);
            ema = seen ? __dadd_rn(ema, __dmul_rn(beta, __dsub_rn(rate, ema))) : rate;
            seen = true;
            st[0] = ema;
            st[1] = 1.0;
            for (int s = 0; s < 8; ++s) row[s] = 0.0;
        }
        double fail = 1.0;
        if (seen) {
            fail = __dsub_rn(1.0, ema);
            fail = fail > 0.0 ? fail : 0.0;
            fail = fail < 1.0 ? fail : 1.0;
        }
        const uint32_t wk = w_min + (uint32_t)__dadd_rn(__dmul_rn(fail, 65536.0), 0.5);
        w_l[k] = wk;
        w[k] = wk;
    }
    __syncthreads();
    if (k == 0) family_thresholds_from_weights(w_l, C, thr);
}

// ---------------------------------------------------------------------------------------------
// draw == 0: n_valid + no-action detection (successor_dqn.py:409-411), part of every lock-step;
// draw == 1: the synthetic uniform-random policy over the valid candidates -> sel_index.
__global__ __launch_bounds__(WAVE) void k_select(DevCtx c, int draw) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const int nc = c.b.n_cand[e];
    const size_t off = (size_t)c.b.cand_offset[e];
    int nvalid = 0;
    for (int a0 = 0; a0 < nc; a0 += WAVE) {
        int a = a0 + lane;
        nvalid += __popcll(__ballot(a < nc && c.b.cand_mask[off + a]));
    }
    int sel = 0;
    if (nvalid > 0 && draw) {
        uint64_t ctr = c.b.draw_counter[e];
        uint64_t r = splitmix64(splitmix64(((c.seed & 0xFFFFFFFFull) << 32) | (uint32_t)(c.env_id_base + e)) ^ ctr);
        int rank = (int)(r % (uint64_t)nvalid);
        int seen = 0;
        for (int a0 = 0; a0 < nc; a0 += WAVE) {
            int a = a0 + lane;
            uint64_t bal = __ballot(a < nc && c.b.cand_mask[off + a]);
            int cnt = __popcll(bal);
            if (rank < seen + cnt) {
                int want = rank - seen;            // want-th set bit of bal
                for (int k = 0; k < want; ++k) bal &= bal - 1;
                sel = a0 + (__ffsll((long long)bal) - 1);
                break;
            }
            seen += cnt;
        }
    }
    if (lane == 0) {
        if (draw) {
            c.b.sel_index[e] = sel;
            if (nvalid > 0) c.b.draw_counter[e] += 1;
        } else {
            c.b.n_valid[e] = nvalid;
            if (nvalid == 0) {
                c.b.needs_reset[e] = 1;
                c.b.step_flags[(size_t)e * 8 + F_NO_ACTIONS] = 1;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// is_action_stable_rbe (assembly_gym/assembly_gym/utils/stability.py:122-130) for every valid candidate of every env:
// the candidate block is appended to the assembly (free), the boundary conditions of the placed blocks stay (the last
// placed block is frozen, gym_env.py:238-240) and the RBE feasibility LP decides.  One wave per candidate.  Nothing is
// rebuilt: the env's persistent contact list (k_step) is read in place, only the face pairs between the candidate and
// the older bodies are tested (same pair order as append_interfaces, so the LP is column for column the one k_step
// would build after placing the candidate) and kept in LDS; the candidate's pose / vertices / frames come from the
// candidate arrays k_enumerate wrote.  Result: cand_stable[ci] = 1 stable, 0 unstable (or masked-out candidate),
// 2 = solver error / interface overflow (counts as unstable, stability.py:68 + gym_env.py:182).
//
// Two launches share the code.  QUEUE == false: grid over all raw candidates, a small LDS tableau (high occupancy);
// a candidate whose tableau does not fit is appended to cand_queue (one atomic per such candidate, they are rare).
// QUEUE == true: a small persistent grid drains that queue with the full-size LDS tableau and the env workspace
// lp_ws (one slot per workgroup) behind it; every wave leaves when the queue head passes the count.
#define CS_NEW_IF 16
#define CS_WAVES 4          // waves per SIMD the first pass is compiled for (register cap 512 / CS_WAVES): 4 waves / 13 spills
                            // 87.5 M LPs/s against 80.5 M for 3 spill-free waves and less for 5 or 6 (profiles/r04_cs_variants.txt)
template <int TAB, int MAXCOLS, bool QUEUE>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(QUEUE ? 1 : CS_WAVES, QUEUE ? 2 : CS_WAVES))) void k_candidate_stability(DevCtx c) {
    __shared__ __attribute__((aligned(16))) double tab[TAB];
    __shared__ LpScratchT<MAXCOLS> S;
    __shared__ double new_geom[CS_NEW_IF * 8];
    __shared__ int32_t new_body[CS_NEW_IF * 2];
    const int lane = threadIdx.x;
    const int K = c.K;
    const bridges_shape* shapes = c.tt->shapes;
    const int total = c.b.cand_offset[c.E];
    int32_t* cnt = c.b.cand_counters;                 // [0] queue length, [1] queue head
    const int qlen = QUEUE ? cnt[0] : 0;
    for (int item = blockIdx.x;; item += gridDim.x) {
        int ci;
        if constexpr (QUEUE) {
            int i = 0;
            if (lane == 0) i = atomicAdd(&cnt[1], 1);
            i = __builtin_amdgcn_readfirstlane(i);
            if (i >= qlen) return;
            ci = c.b.cand_queue[i];
        } else {
            if (item >= total) return;
            ci = item;
            if (!c.b.cand_mask[ci]) {
                if (lane == 0) c.b.cand_stable[ci] = 0;
                continue;
            }
        }
        __syncthreads();                               // LDS lists of the previous item are dead
        const int e = c.b.cand_env[ci];
        const int nb = c.b.n_blocks[e];                // index the candidate would take
        const int32_t* shape_id = c.b.blk_shape + (size_t)e * K;
        const double* pose = c.b.blk_pose + (size_t)e * K * 4;
        const double* verts = c.b.blk_verts + (size_t)e * K * MAXV * 2;
        const int csh = c.b.cand_desc[(size_t)ci * 4 + 2];
        const bridges_shape& shn = shapes[csh];
        const double* cverts = c.b.cand_verts + (size_t)ci * MAXV * 2;
        const double* cframes = c.b.cand_frames + (size_t)ci * MAXV * 4;
        const int n_if0 = c.b.n_if[e];
        // ---- interfaces candidate <-> floor and blocks < nb ----
        const int totalp = (1 + nb * MAXV) * MAXV;
        int n_new = 0;
        for (int p0 = 0; p0 < totalp; p0 += WAVE) {
            const int p = p0 + lane;
            bool hit = false;
            double g[8];
            int bodyA = -1;
            if (p < totalp) {
                const int qa = p / MAXV, fn = p % MAXV;
                if (fn < shn.nv) {
                    const int ia = shn.fa[fn], ib = shn.fb[fn];
                    const double aBx = cverts[2 * ia], aBz = cverts[2 * ia + 1], bBx = cverts[2 * ib], bBz = cverts[2 * ib + 1];
                    const double cBx = cframes[4 * fn], cBz = cframes[4 * fn + 1], nBx = cframes[4 * fn + 2], nBz = cframes[4 * fn + 3];
                    if (qa == 0) {
                        hit = face_pair_contact_v(-c.floor_hw, 0.0, c.floor_hw, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, aBx, aBz, bBx,
                                                  bBz, cBx, cBz, nBx, nBz, fmin(c.floor_depth, shn.depth), g);
                    } else {
                        bodyA = (qa - 1) / MAXV;
                        const int f = (qa - 1) % MAXV;
                        const bridges_shape& sa = shapes[shape_id[bodyA]];
                        if (f < sa.nv) {
                            const double* v = verts + (size_t)bodyA * MAXV * 2;
                            const double ax = v[2 * sa.fa[f]], az = v[2 * sa.fa[f] + 1], bx = v[2 * sa.fb[f]], bz = v[2 * sa.fb[f] + 1];
                            const Frame2 fr = edge_frame(ax, az, bx, bz);
                            hit = face_pair_contact_v(ax, az, bx, bz, fr.cx, fr.cz, fr.tx, fr.tz, fr.nx, fr.nz, aBx, aBz, bBx, bBz,
                                                      cBx, cBz, nBx, nBz, fmin(sa.depth, shn.depth), g);
                        }
                    }
                }
            }
            const uint64_t bal = __ballot(hit);
            const int idx = n_new + __popcll(bal & ((1ull << lane) - 1ull));
            if (hit && idx < CS_NEW_IF) {
                new_body[2 * idx] = bodyA;
                new_body[2 * idx + 1] = nb;
#pragma unroll
                for (int k = 0; k < 8; ++k) new_geom[8 * idx + k] = g[k];
            }
            n_new += __popcll(bal);
        }
        __syncthreads();
        uint8_t res;
        if (n_new > CS_NEW_IF || n_if0 + n_new > MAXIF) {
            res = 2;                                   // contact list overflow (k_step would flag the same placement)
        } else {
            AsmView A;
            A.pose = pose; A.shape_id = shape_id; A.shapes = shapes; A.n_blocks = nb + 1;
            A.cand_b = nb; A.cand_pose = c.b.cand_pose + (size_t)ci * 4; A.cand_shape = csh; A.cen = nullptr; A.vol = nullptr; A.n_tens = 0; A.tens_coef = 1.0;
            A.n_if = n_if0 + n_new; A.n_if0 = n_if0;
            A.if_body0 = c.b.if_body + (size_t)e * MAXIF * 2; A.if_geom0 = c.b.if_geom + (size_t)e * MAXIF * 8;
            A.if_body1 = new_body; A.if_geom1 = new_geom;
            const uint32_t fixed = nb > 0 ? (1u << (nb - 1)) : 0u;
            bool err = false, too_big = false;
            double w = 0.0;
            int piv = 0;
            bool st = false, solved = false;
            // continue from the env's snapshot (k_step's "last block frozen" tableau of this very state): ~3 pivots
            // instead of ~2 per row from scratch
            if (c.b.lp_snap && nb > 0) {
                const double* snap = c.b.lp_snap + (size_t)e * c.b.lp_snap_stride;
                WarmPre W;
                warm_header(W, snap, lane);
                W.ok = warm_matches(W, nb, n_if0);
                W.n_pre = 0;
                if (W.ok) {
                    bool fits = false, werr = false;
                    st = rbe_candidate_warm(tab, TAB, MAXCOLS, S, A, n_if0, W, snap, c.mu, c.density, lane, &fits, &werr, &piv);
                    if (!fits) {
                        if constexpr (!QUEUE) {
                            if (lane == 0) c.b.cand_queue[atomicAdd(&cnt[0], 1)] = ci;
                            continue;                  // decided by the second launch
                        }
                    } else if (!werr) {
                        solved = true;
                    }
                    __syncthreads();
                }
            }
            if (!solved) {                             // no snapshot (first block, foreign state) or a failed check: from scratch
                double* ws = QUEUE ? c.b.cand_ws + (size_t)blockIdx.x * c.b.cand_ws_stride : nullptr;
                st = rbe_stable(tab, TAB, MAXCOLS, ws, QUEUE ? c.b.cand_ws_stride : (int64_t)0, S, A, fixed, c.mu, c.density,
                                lane, &w, &piv, &err, &too_big);
                if (too_big) {
                    if constexpr (!QUEUE) {
                        if (lane == 0) c.b.cand_queue[atomicAdd(&cnt[0], 1)] = ci;
                        continue;                      // decided by the second launch
                    }
                    err = true;
                }
            }
            res = err ? 2 : (st ? 1 : 0);
        }
        if (lane == 0) c.b.cand_stable[ci] = res;
    }
}

// ---------------------------------------------------------------------------------------------
// Stable actions only (bridges_env_restrict_to_stable), after k_candidate_stability: filter_actions ∩ {is_action_stable_rbe}.
// One wave per env, the shape of k_select's draw == 0 pass: a valid candidate whose verdict is not 1 (unstable, or a solver
// error, stability.py:68) leaves cand_mask, n_valid is recounted, and an env left without a candidate is marked as k_select
// marks one without a valid candidate (the next lock-step is reset-only, successor_dqn.py:409-411).
__global__ __launch_bounds__(WAVE) void k_restrict_stable(DevCtx c) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const int nc = c.b.n_cand[e];
    const size_t off = (size_t)c.b.cand_offset[e];
    int nvalid = 0;
    for (int a0 = 0; a0 < nc; a0 += WAVE) {
        const int a = a0 + lane;
        bool keep = false;
        if (a < nc && c.b.cand_mask[off + a]) {
            keep = c.b.cand_stable[off + a] == 1;
            if (!keep) c.b.cand_mask[off + a] = 0;
        }
        nvalid += __popcll(__ballot(keep));
    }
    if (lane == 0) {
        c.b.n_valid[e] = nvalid;
        if (nvalid == 0) {
            c.b.needs_reset[e] = 1;
            c.b.step_flags[(size_t)e * 8 + F_NO_ACTIONS] = 1;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The persistent contact list of a state the host wrote (bridges_replay_unpack, load_states), for bridges_env_rebuild_contacts:
// block after block, the faces of block b against the floor and the faces of every block < b -- the pairs k_step tests when
// it places block b, in the same order and with the same arithmetic (append_interfaces on frames staged from the vertices;
// k_step computes them on the fly from the same vertices with the same edge_frame / face_pair_contact_v calls).  One wave
// per env.  The env's persisted tableaux describe some other assembly: both headers are invalidated, so that k_step and
// k_candidate_stability take their cold paths on this state.
__global__ __launch_bounds__(WAVE) void k_rebuild_contacts(DevCtx c) {
    __shared__ FaceLds F;
    __shared__ bridges_shape sh_l[8];
    __shared__ int32_t shape_l[MAXK];
    const int e = blockIdx.x, lane = threadIdx.x;
    const int K = c.K;
    int nb = c.b.n_blocks[e];
    nb = nb < 0 ? 0 : (nb > K ? K : nb);
    {
        const double* src = reinterpret_cast<const double*>(c.tt->shapes);
        double* dst = reinterpret_cast<double*>(sh_l);
        const int nd = c.n_shapes * (int)(sizeof(bridges_shape) / 8);
        for (int i = lane; i < nd; i += WAVE) dst[i] = src[i];
        if (lane < K) shape_l[lane] = c.b.blk_shape[(size_t)e * K + lane];
    }
    __syncthreads();
    stage_faces(F, 0, 1 + nb * MAXV, c.b.blk_verts + (size_t)e * K * MAXV * 2, shape_l, sh_l, c.floor_hw, lane);
    __syncthreads();
    int32_t* if_body_g = c.b.if_body + (size_t)e * MAXIF * 2;
    double* if_geom_g = c.b.if_geom + (size_t)e * MAXIF * 8;
    int n_if = 0;
    bool overflow = false;
    for (int b = 0; b < nb; ++b)
        n_if = append_interfaces(F, b, shape_l, sh_l, c.floor_depth, n_if, if_body_g, if_geom_g, lane, &overflow);
    if (lane == 0) {
        c.b.n_if[e] = n_if;
        uint8_t* fl = c.b.step_flags + (size_t)e * 8 + F_LP_ERROR;
        *fl = (uint8_t)((*fl & ~2u) | (overflow ? 2u : 0u));
        reinterpret_cast<WarmHdr*>(c.b.lp_ws + (size_t)e * c.b.lp_ws_stride)->magic = 0;
        if (c.b.lp_snap) reinterpret_cast<WarmHdr*>(c.b.lp_snap + (size_t)e * c.b.lp_snap_stride)->magic = 0;
    }
}

}  // namespace bridges
