/*
 * bridges_hip.h -- C ABI of libbridges_hip.so (MI355X / gfx950).
 *
 * The reference (syghmon/bridges-with-reinforcement-learning) is pure Python and has
 * no FFI layer; this header is the boundary SURVEY.md §8(b) defines for its hot path.
 * Every entry point names the reference code it replaces (paths relative to the
 * reference root).  Conventions:
 *   - all buffers are DEVICE pointers owned by the caller (PyTorch tensors in the
 *     shipped host code); the library allocates only small constant tables inside
 *     *_create and nothing afterwards;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); all work is
 *     enqueued asynchronously, nothing synchronises;
 *   - return value 0 = ok, negative = BRIDGES_E_*; no exceptions cross the ABI.
 *
 * Reference-side binding: INTEGRATION.md shows the ctypes stub a maintainer adds.
 */
#ifndef BRIDGES_HIP_H
#define BRIDGES_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRIDGES_OK 0
#define BRIDGES_E_ARG (-1)      /* bad argument / size over a compiled limit */
#define BRIDGES_E_HIP (-2)      /* a HIP runtime call failed (bridges_last_error()) */
#define BRIDGES_E_NODEV (-3)    /* no HIP device */

#define BRIDGES_MAX_VERTS 6     /* hexagon */
#define BRIDGES_MAX_BLOCKS 16   /* --max_steps <= 16 */
#define BRIDGES_MAX_GROUPS 24   /* (shape, target face) pairs of one task */
#define BRIDGES_MAX_TARGETS 8
#define BRIDGES_MAX_INTERFACES 64
#define BRIDGES_IMG 64          /* rasters are 64x64 (successor_dqn.py:585 default) */
/* doubles of lp_ws per environment: 64 (header, basis) + 2 halves of (3*MAX_BLOCKS+2) rows x (4*MAX_IF + 2 + 3*MAX_BLOCKS + 1) columns */
#define BRIDGES_LP_WS_DOUBLES (64 + 2 * (3 * BRIDGES_MAX_BLOCKS + 2) * (4 * BRIDGES_MAX_INTERFACES + 2 + 3 * BRIDGES_MAX_BLOCKS + 1))
#define BRIDGES_LP_SNAP_DOUBLES (64 + (3 * BRIDGES_MAX_BLOCKS + 2) * (4 * BRIDGES_MAX_INTERFACES + 2 + 3 * BRIDGES_MAX_BLOCKS + 1))
#define BRIDGES_CAND_WS_SLOTS 1024

/* One block shape: a convex (x,z) outline extruded along y.
 * Replaces Shape.from_urdf / from_mesh / get_face_frame_2d
 * (assembly_gym/assembly_gym/envs/assembly_env.py:45-68, 118-124).  The host
 * fills the derived fields with the arithmetic contract of DESIGN.md. */
typedef struct {
    int32_t nv;                              /* vertices == 2-D faces */
    int32_t pad_;
    double vx[BRIDGES_MAX_VERTS], vz[BRIDGES_MAX_VERTS];
    int32_t fa[BRIDGES_MAX_VERTS], fb[BRIDGES_MAX_VERTS];   /* face f = directed edge fa->fb */
    double fcx[BRIDGES_MAX_VERTS], fcz[BRIDGES_MAX_VERTS];  /* local face centre */
    double fnx[BRIDGES_MAX_VERTS], fnz[BRIDGES_MAX_VERTS];  /* local outward normal */
    double depth;                            /* extent along y */
    double volume;                           /* area * depth */
    double gx, gz;                           /* local centroid */
} bridges_shape;

/* Static description of one vectorised task (all environments share it -- except the targets of an env that has
 * bridges_task_buffers attached, see bridges_env_set_task_buffers: `targets` is then not read, n_targets still is).
 * Replaces the arguments of AssemblyGym.__init__/reset, AssemblyEnv.__init__
 * (gym_env.py:116-139, 255-289; assembly_env.py:164-199) and the constants of
 * successor_dqn.py:611-616. */
typedef struct {
    int32_t n_envs;
    int32_t max_blocks;        /* state capacity K (>= max_steps) */
    int32_t max_steps;         /* 0 = None (gym_env.py:143) */
    int32_t a_max;             /* candidate capacity per env */
    int32_t n_shapes;          /* entries of `shapes` */
    int32_t n_groups;          /* (shape, target_face) pairs in generate_actions order (actions.py:16-19) */
    int32_t group_shape[BRIDGES_MAX_GROUPS];
    int32_t group_face[BRIDGES_MAX_GROUPS];
    int32_t n_ground;          /* len(x_discr_ground) */
    int32_t n_offsets;         /* len(offset_values) */
    int32_t n_targets;
    int32_t debug;             /* 0.  Diagnostic builds (-DBRIDGES_DIAG) read timing-experiment switches from it; the
                                  product library refuses any other value */
    int32_t env_id_base;       /* global id of env 0 (policy RNG stream = seed, env_id_base + e) */
    int32_t img_size;          /* S of the S x S images (--image_size, successor_dqn.py:585); 0 = 64.  S < 64: every
                                  image buffer keeps its 64x64 / 64-word layout and the image is its top-left S x S
                                  corner (the rest is zero) */
    double mu, density;        /* assembly_env.py:164 */
    double floor_half_width;   /* assembly_env.py:290-296 */
    double floor_depth;
    double xlim[2], ylim[2];   /* successor_dqn.py:615-616 */
    double targets[BRIDGES_MAX_TARGETS][3];
    uint64_t seed;             /* synthetic random policy */
    const bridges_shape* shapes;   /* HOST pointer, n_shapes entries (copied) */
    const double* x_ground;        /* HOST, n_ground */
    const double* offsets;         /* HOST, n_offsets */
    const double* grid_x;          /* HOST, S: np.linspace(xlim0, xlim1, S) */
    const double* grid_y;          /* HOST, S: np.linspace(ylim1, ylim0, S) */
} bridges_task;

/* Caller-owned device buffers of a vectorised environment.  E = n_envs,
 * K = max_blocks, C = E * a_max (capacity of the compact candidate arrays:
 * candidate a of env e lives at index cand_offset[e] + a). */
typedef struct {
    /* --- state (struct of arrays) --- */
    int32_t* n_blocks;         /* [E] */
    int32_t* blk_shape;        /* [E,K] */
    double* blk_pose;          /* [E,K,4]  x, z, cos, sin */
    double* blk_verts;         /* [E,K,6,2] world (x,z) */
    uint8_t* blk_occ;          /* [E,K] bit f = face f occupied (gym_env.py:228-232 block_graph) */
    uint32_t* targets_left;    /* [E] bit t = target t not reached yet */
    uint64_t* state_bits;      /* [E,64] row r = 64-pixel mask of the state raster */
    int32_t* n_if;             /* [E] contact interfaces */
    int32_t* if_body;          /* [E,MAX_IF,2] body A, body B (-1 = floor) */
    double* if_geom;           /* [E,MAX_IF,8] p_lo.xz, p_hi.xz, n.xz, t.xz */
    uint64_t* draw_counter;    /* [E] policy draws so far */
    uint8_t* needs_reset;      /* [E] */
    /* --- per-step results --- */
    int32_t* sel_index;        /* [E] in: candidate to place */
    uint8_t* step_flags;       /* [E,8] valid_step, stable_frozen, stable_unfrozen, terminated, truncated, done, no_actions,
                                  lp_error (bit 0 solver error, bit 1 contact-list overflow; bit 2 is not an error: the step's
                                  continued tableau said 'unstable' by a small margin and was solved again from scratch;
                                  bit 3: the state has more raw candidates than a_max -- its candidate set was cut to a_max,
                                  something the reference's generate_actions (actions.py:7-52) never does: treat as an error) */
    float* reward;             /* [E] sparse_reward (gym_env.py:11-22) */
    float* lin_reward;         /* [E] successor_dqn.py:397-401 */
    int32_t* n_reached;        /* [E] */
    /* --- candidates of the current state --- */
    int32_t* n_cand;           /* [E] raw candidates of the state, clamped to a_max by reset / step / refresh (a producer that fills
                                  the state arrays itself writes the unclamped count: the clamp is flagged and counted) */
    int32_t* n_valid;          /* [E] */
    int32_t* cand_offset;      /* [E+1] exclusive prefix sum of n_cand */
    int32_t* cand_env;         /* [C] owning env */
    int32_t* cand_desc;        /* [C,4] target_block, target_face, shape, face */
    double* cand_ox;           /* [C] offset_x */
    double* cand_pose;         /* [C,4] */
    double* cand_verts;        /* [C,6,2] */
    double* cand_frames;       /* [C,6,4] world face frames (centre.xz, normal.xz) of the candidate block */
    int32_t* cand_rows;        /* [C,2] rasteriser work descriptor: row_lo | row_hi<<8 | nv<<16 | in_bounds<<24, owning env */
    uint8_t* cand_inb;         /* [C] inside xlim/ylim (gym_env.py:304-323) */
    uint8_t* cand_mask;        /* [C] filter_actions result (actions.py:71-82) */
    float* cand_lin;           /* [C] sum(action_raster * reward_map) */
    uint64_t* cand_bits;       /* [C,64] bit-packed action rasters */
    float* cand_raster;        /* [C,64,64] f32 action rasters (may be NULL: skip) */
    float* state_raster;       /* [E,64,64] f32 (may be NULL) */
    int32_t* cand_raster_nz;   /* [C] or NULL.  Non-NULL = sparse update of cand_raster: bit g = row group g (rows 4g..4g+3)
                                  of slot i holds non-zero pixels.  The rasteriser then writes only the groups that are
                                  non-zero now or were non-zero before; the buffers must start zeroed with zeroed masks. */
    int32_t* state_raster_nz;  /* [E] or NULL: the same for state_raster (both or neither) */
    /* --- task features --- */
    const uint64_t* obstacle_bits; /* [64] */
    const float* reward_map;       /* [64,64] */
    const double* reward_prefix;   /* [64,65] float64 row prefix sums of reward_map: [r][x] = sum of reward_map[r][0..x-1]
                                      (the rasteriser takes a candidate's sum(raster * reward_map) from its row runs) */
    /* --- scratch --- */
    double* lp_ws;             /* [E, lp_ws_stride] per-env persistent simplex tableau (incremental solve of bridges_env_step):
                                  header + basis + two tableau halves; owned by the library between reset and step calls */
    int64_t lp_ws_stride;      /* >= BRIDGES_LP_WS_DOUBLES */
    uint64_t* stats;           /* [16] sum n_cand, sum n_blocks, env-steps, reset-only steps, lp errors, if overflow, lock-steps,
                                  sum n_valid, continued (warm) 'unstable' verdicts solved again from scratch, candidate sets cut to
                                  a_max (must stay 0: size a_max from the task's bound); rest reserved */
    /* --- candidate stability (bridges_env_candidate_stability; all three may be NULL if it is never called) --- */
    uint8_t* cand_stable;      /* [C] 1 = stable, 0 = unstable or masked-out candidate, 2 = solver error / contact overflow */
    int32_t* cand_queue;       /* [C] scratch: candidates whose tableau needs the large workspace */
    int32_t* cand_counters;    /* [4] scratch: queue length, queue head */
    double* cand_ws;           /* [BRIDGES_CAND_WS_SLOTS, cand_ws_stride] scratch: tableaux too large for LDS */
    int64_t cand_ws_stride;    /* >= (3K+2)*(4*MAX_IF+3) */
    double* lp_snap;           /* [E, lp_snap_stride] or NULL: per env the simplex tableau of "last block frozen" of its
                                  current state, written by bridges_env_step; bridges_env_candidate_stability continues every
                                  candidate's LP from it (NULL: candidates are solved from scratch) */
    int64_t lp_snap_stride;    /* >= BRIDGES_LP_SNAP_DOUBLES */
} bridges_env_buffers;

typedef struct bridges_env bridges_env;

const char* bridges_last_error(void);
int bridges_device_count(void);
/* The stamp the library was compiled with: sha256 over csrc/<every file> and include/<every file> (file names and contents,
 * sorted by name; -DBRIDGES_SRC_HASH=... by __graft_entry__.build()), "unstamped" for a build without it.  The Python
 * binding refuses a library whose stamp is not the hash of the sources lying beside it: a stale .so cannot pass for a build. */
const char* bridges_source_hash(void);

/* --- vectorised environment ------------------------------------------------ */
int bridges_env_create(const bridges_task* task, const bridges_env_buffers* buf, bridges_env** out);
int bridges_env_destroy(bridges_env* env);
/* AssemblyGym.reset for every env + first candidate set. */
int bridges_env_reset(bridges_env* env, void* stream);
/* One lock-step: AssemblyGym.step + stabilities_freezing (gym_env.py:218-253, 325-333),
 * sparse_reward, auto-reset, then generate_actions / get_action_features /
 * filter_actions / linear reward for the new state (successor_dqn.py:392-411).
 * Places sel_index[e] for every env. */
int bridges_env_step(bridges_env* env, void* stream);
/* Synthetic uniform-random policy over the valid candidates -> sel_index. */
int bridges_env_select_random(bridges_env* env, void* stream);
/* select_random + step in one call (the synthetic-rollout inner loop). */
int bridges_env_lockstep_random(bridges_env* env, void* stream);
/* Time the dominant kernel (the rasteriser) of the next <= max_launches lock-steps with HIP events recorded on
 * the launch stream; timing_end synchronises on them and returns the summed duration. */
int bridges_env_timing_begin(bridges_env* env, int32_t max_launches);
int bridges_env_timing_end(bridges_env* env, double* raster_ms_total, int32_t* n_launches);
/* Raster gate: environments that share a gate (one per GPU) never run their rasterisers concurrently -- each
 * rasteriser launch waits (hipStreamWaitEvent) for the previous one of the gate.  With several env groups on several
 * streams this serialises the bandwidth-bound kernels while the latency-bound task kernels of the other groups run
 * beside them.  A gate must outlive the environments attached to it. */
typedef struct bridges_gate bridges_gate;
int bridges_gate_create(bridges_gate** out);
int bridges_gate_destroy(bridges_gate* gate);
int bridges_env_set_gate(bridges_env* env, bridges_gate* gate);
/* Candidate refresh only (used after the host edited the state). */
int bridges_env_refresh(bridges_env* env, void* stream);
/* is_action_stable_rbe (assembly_gym/assembly_gym/utils/stability.py:122-130) for EVERY valid candidate of every
 * environment in one pass -> cand_stable[cand_offset[e] + a].  The candidate block is appended to the env's assembly
 * (free; the last placed block stays frozen, gym_env.py:238-240); its contacts are found against the env's persistent
 * contact list, which must be current (i.e. the state was reached through bridges_env_reset / bridges_env_step). */
int bridges_env_candidate_stability(bridges_env* env, void* stream);
/* Stable actions only: bridges_env_candidate_stability, then one wave per env clears cand_mask[ci] where cand_stable[ci] != 1
 * (a solver error counts as unstable, stability.py:68) and recounts n_valid; an env left without a stable candidate gets
 * needs_reset and F_NO_ACTIONS, as the candidate refresh marks an env without a valid one.  Call it after
 * bridges_env_reset / _step / _refresh on the same stream; everything that reads cand_mask / n_valid afterwards sees the
 * narrowed set.  No host wait. */
int bridges_env_restrict_to_stable(bridges_env* env, void* stream);
/* The persistent contact list (n_if, if_body, if_geom) of every env's current block list, rebuilt as bridges_env_step would
 * hold it had it placed the blocks one by one (same pair order and arithmetic; an overflow sets bit 1 of F_LP_ERROR), for
 * states the host wrote (bridges_replay_unpack / load_states).  Invalidates the env's persisted tableaux (lp_ws, lp_snap):
 * bridges_env_candidate_stability then solves the candidates of these states from scratch.  No host wait. */
int bridges_env_rebuild_contacts(bridges_env* env, void* stream);
/* Fork: env e continues from the state of env src[e] (src int32 [E], device) -- the primitive of beam search, best-of-N with
 * resampling, MCTS and restart distributions.
 * THE RULE: after the call, every per-env row of every STATE array of env e holds the bits that row of env src[e] held before
 * the call, for any src: permutations, duplicates, broadcasts, swaps, chains.  An entry src[e] outside [0, E) means e: the env
 * keeps its own state, and nothing outside the buffers is read.
 * State arrays (the list is the table fork_table() of csrc/api.hip): n_blocks, blk_shape, blk_pose, blk_verts, blk_occ,
 * targets_left, state_bits; n_if, if_body, if_geom; draw_counter, needs_reset; step_flags, reward, lin_reward, n_reached; n_cand;
 * the env's lp_ws row and, when given, its lp_snap row (whole rows: a clone's warm header must never match a tableau of another
 * geometry); with task buffers attached the env's task as well -- env_targets, target_bits, reward_map, reward_prefix,
 * task_episode, env_obstacles / env_obstacle_bits where present, task_class with a family set.  A fork is the whole env.
 * NOT copied: sel_index (an input), the candidate arrays (n_valid, cand_offset, cand_*, state_raster and the *_nz masks, which
 * describe buffer slots) -- the caller refreshes them (bridges_env_refresh, then bridges_env_restrict_to_stable where it
 * narrows the sets) --, stats, and everything all envs share.  The copied contact lists and tableaux are as current as the
 * sources' were.
 * Two launches through the caller's scratch (bridges_env_fork_scratch bytes, 16-byte aligned; about 0.37 MB per env with
 * lp_snap, 0.25 MB without): gather the rows of src into the scratch, then write them back.  No kernel both reads and writes a
 * state array, no atomics, no host wait, the same bits on every call.
 * Refused (BRIDGES_E_ARG, nothing launched): a NULL env, src or scratch, src not 4-byte or scratch not 16-byte aligned,
 * scratch_bytes below the sizing call's answer. */
int bridges_env_fork_scratch(const bridges_env* env, int64_t* bytes);
int bridges_env_fork(bridges_env* env, const int32_t* src /* [E] device */, void* scratch, int64_t scratch_bytes, void* stream);

/* --- per-env tasks ------------------------------------------------------------
 * tower_setup draws three fresh targets each time an episode starts (assembly_gym/assembly_gym/envs/gym_env.py:64-79,
 * env.reset(**setup_fct()), robotoddler/training/successor_dqn.py:371).  With these buffers attached every env owns its
 * targets and everything derived from them; without them nothing changes (same launches, same buffers, same bits).
 * Caller-owned DEVICE buffers, E = n_envs, T = n_targets of the task (a task constant): */
#define BRIDGES_GAUSS_TAPS 101  /* kernel_size of convolve_with_gaussian (successor_dqn.py:80-82) */
#define BRIDGES_MAX_OBSTACLES 4 /* per-env obstacles of one env (bridges_task_buffers.n_obstacles) */
typedef struct {
    double* env_targets;       /* [E,T,3] (x, y, z) of every env's targets; y is compared as the fixed task's is */
    uint64_t* target_bits;     /* [E,64] raster of the env's T cube06 target blocks (get_task_features, successor_dqn.py:73-79) */
    float* reward_map;         /* [E,64,64] its Gaussian blur: convolve_with_gaussian(raster, 101, 16) of the S x S image */
    double* reward_prefix;     /* [E,64,65] float64 row prefix sums of reward_map (bridges_env_buffers.reward_prefix, per env) */
    uint32_t* task_episode;    /* [E] episodes the env has started since bridges_env_reset (the first one is 0) */
    uint64_t* env_obstacle_bits;   /* [E,64] or NULL: raster of the env's O cube06 obstacle blocks, written by the library from
                                      env_obstacles (per-env obstacles, below); NULL with n_obstacles = 0: obstacles stay shared */
    const float* gauss_k;      /* [BRIDGES_GAUSS_TAPS] the normalised float32 Gaussian vector k of the reference's kernel k k^T */
    int32_t target_shape;      /* shape id (in the task's shape table) of a target block: cube06 */
    int32_t sample;            /* 1: an env draws new targets on the device whenever it starts an episode; 0: env_targets stay */
    double x_range[2];         /* sampler: x ~ U[x_range), z ~ U[z_range), y = 0 (tower_setup: [-4, 4], [0, 4]) */
    double z_range[2];
    /* --- per-env obstacles (connecting_setup draws targets AND obstacles per call, gym_env.py:91-99).  Appended: the fields
     * above keep their offsets.  All-zero = obstacles stay bridges_env_buffers.obstacle_bits, one raster for all envs. --- */
    double* env_obstacles;     /* [E,O,3] (x, y, z) of every env's obstacles, O = n_obstacles; NULL when n_obstacles = 0 */
    int32_t n_obstacles;       /* O: 0 = obstacles stay shared, else 1..BRIDGES_MAX_OBSTACLES (env_obstacle_bits and env_obstacles given) */
    int32_t sample_obstacles;  /* 1: an env draws new obstacles on the device whenever it starts an episode; 0: env_obstacles stay */
    double obs_x_range[BRIDGES_MAX_OBSTACLES][2];   /* sampler, per obstacle o: x ~ U[obs_x_range[o]), z ~ U[obs_z_range[o]), y = 0 */
    double obs_z_range[BRIDGES_MAX_OBSTACLES][2];
} bridges_task_buffers;
/* Attach (or replace) the per-env task buffers; NULL detaches them (the env is a fixed-task env again; call bridges_env_reset).
 * From here on the reached-test of bridges_env_step reads env_targets[e], the rasteriser takes cand_lin from reward_prefix[e],
 * and bridges_env_buffers.reward_map / reward_prefix and bridges_task.targets are not read.  Enqueues nothing.
 * bridges_env_reset then sets task_episode = 0 and rebuilds every env's task features (after drawing the targets of episode
 * 0 when sample = 1); bridges_env_step does so, when sample = 1, for the envs that begin an episode in that lock-step: task_episode
 * += 1, new targets.  The step that ends an episode is rewarded against the old targets; the candidates of the fresh state carry
 * the new task's cand_lin.  With sample = 0 a lock-step launches nothing extra.
 * The draw is counter-based (splitmix64 as in the synthetic policy, a stream of its own): with gid = env_id_base + e,
 *   h0 = splitmix64(((seed & 0xFFFFFFFF) << 32 | (uint32)gid) ^ 0x7461736B5F726E67)      ("task_rng")
 *   h1 = splitmix64(h0 ^ task_episode)
 *   r  = splitmix64(h1 ^ (3 * t + axis)),   u = (r >> 11) * 2^-53,   value = lo + ((hi - lo) * u)
 * for target t, axis 0 (x) and 2 (z), every operation rounded to binary64 separately; axis 1 (y) = 0.
 * Per-env obstacles (n_obstacles = O > 0, env_obstacle_bits and env_obstacles given; one without the other is refused): every
 * env owns O cube06 obstacle blocks.  The candidate filter of the rasteriser then tests env e's candidates against
 * state_bits[e] | env_obstacle_bits[e] and bridges_env_buffers.obstacle_bits is not read; nothing else reads obstacles.
 * env_obstacle_bits is rebuilt from env_obstacles wherever target_bits is rebuilt from env_targets; with sample_obstacles = 1
 * the obstacles are drawn first, on the same task_episode counter (targets and obstacles of an episode change together; with
 * sample = 0 and sample_obstacles = 1 a lock-step still advances task_episode for the envs that begin an episode and redraws
 * their obstacles, their targets and maps stay).  The obstacle draw is a stream of its own:
 *   h0 = splitmix64(((seed & 0xFFFFFFFF) << 32 | (uint32)gid) ^ 0x6F6273745F726E67)      ("obst_rng")
 *   h1 = splitmix64(h0 ^ task_episode)
 *   r  = splitmix64(h1 ^ (3 * o + axis)),   u = (r >> 11) * 2^-53,   value = lo + ((hi - lo) * u)
 * for obstacle o with its own ranges obs_x_range[o] / obs_z_range[o], axis 0 (x) and 2 (z), every operation rounded to
 * binary64 separately; axis 1 (y) = 0. */
int bridges_env_set_task_buffers(bridges_env* env, const bridges_task_buffers* tb);
/* The host (or another kernel) has written env_targets: rebuild target_bits, reward_map and reward_prefix of every env -- and,
 * with per-env obstacles attached, env_obstacle_bits from env_obstacles.
 * task_episode and the env states stay; the candidates' cand_lin is stale until bridges_env_reset / _refresh.  No host wait. */
int bridges_env_load_targets(bridges_env* env, void* stream);

/* --- per-env task families ------------------------------------------------------
 * horizontal_bridge_setup(num_obstacles = n) and bridge_setup(num_stories = n) are ONE integer n from which the target and all
 * obstacles follow.  A family draws n per env and episode on the device and writes the task it names into the per-env task
 * buffers; an env then trains across bridge spans (or tower heights).  An obstacle slot the drawn task does not use is parked
 * far below the image, where its cube06 rasterises to nothing: every consumer of [E,O,3] obstacle arrays stays as it is. */
#define BRIDGES_FAMILY_NONE 0
#define BRIDGES_FAMILY_SPAN 1    /* horizontal_bridge_setup(square_size = size, num_obstacles = n), gym_env.py:25-42 */
#define BRIDGES_FAMILY_TOWER 2   /* bridge_setup(H = size, num_stories = n) at x, gym_env.py:46-61 */
#define BRIDGES_PARK_Z (-1000.0) /* z of an obstacle slot the drawn task does not use */
typedef struct {
    int32_t family, n_lo, n_hi, pad_;
    double size, x;              /* x: TOWER only */
    int32_t* task_class;         /* [E] device: n of the env's current task */
} bridges_task_family;
/* Set (or, with NULL or family = BRIDGES_FAMILY_NONE, clear) the task family of an env with per-env task buffers attached.
 * Refused (BRIDGES_E_ARG) unless the buffers have n_targets = 1 and n_obstacles = n_hi, 0 <= n_lo <= n_hi, 1 <= n_hi <=
 * BRIDGES_MAX_OBSTACLES, size > 0 and task_class is given.  A later bridges_env_set_task_buffers clears the family.
 * Enqueues nothing.  With a family set, bridges_env_reset (episode 0) and bridges_env_step for the envs that begin an episode
 * (task_episode += 1) draw n, write env_targets, env_obstacles and task_class[e] = n and rebuild the task features -- in the
 * launch that rebuilds them anyway; sample, sample_obstacles and the ranges of the task buffers are not read.
 * bridges_env_load_targets reads the coordinates as they are written and leaves task_class alone.
 * The draw is a stream of its own, in integer arithmetic only: with gid = env_id_base + e,
 *   h0 = splitmix64(((seed & 0xFFFFFFFF) << 32 | (uint32)gid) ^ 0x66616D695F726E67)      ("fami_rng")
 *   h1 = splitmix64(h0 ^ task_episode)
 *   r  = splitmix64(h1)
 *   n  = n_lo + (int)(((r >> 32) * (uint64)(n_hi - n_lo + 1)) >> 32)
 * Coordinates (binary64, every operation rounded separately, integers converted exactly), y = 0:
 *   SPAN,  s = size:  target ((n*s) + (2.5*s), 0, s/2);     obstacle slot o < n: ((o+1)*s, 0, s/2)
 *   TOWER, H = size:  target (x, 0, (n*H) + (H/2));         obstacle slot o < n: (x, 0, (o*H) + (H/2))
 *   slots o >= n:     (0, 0, BRIDGES_PARK_Z) */
int bridges_env_set_task_family(bridges_env* env, const bridges_task_family* fam);

/* --- weighted families and the curriculum ----------------------------------------
 * A family may carry a threshold table thr: uint64 [C - 1] in device memory, C = n_hi - n_lo + 1.  The draw then uses the
 * family's word r exactly as above (same stream, same salt, same (seed, gid, task_episode)) and, with u = r >> 32,
 *   n = n_lo + #{ k in 0..C-2 : u >= thr[k] }
 * in place of the last line of the uniform draw.  The table of non-negative integer weights w[0..C-1], each <= 2^20, sum > 0:
 *   thr[k] = ceil((w[0] + .. + w[k]) * 2^32 / sum(w))         exact integer arithmetic (the numerator is < 2^56)
 * Class n_lo + k is drawn for thr[k-1] <= u < thr[k] (thr[-1] = 0, thr[C-1] = 2^32): a zero-weight class has an empty interval
 * and is never drawn; a trailing zero weight gives thr = 2^32, above every u.  Equal weights give thr[k] =
 * ceil((k+1) * 2^32 / C), and  u >= ceil(j * 2^32 / C)  <=>  u * C >= j * 2^32  <=>  (u * C) >> 32 >= j:  the uniform draw, for every u.
 *
 * Attach (or, with NULL, detach) a table.  Refused (BRIDGES_E_ARG) without a family set; cleared wherever the family is
 * cleared (bridges_env_set_task_family, bridges_env_set_task_buffers).  Enqueues nothing and reads nothing: the buffer stays
 * the caller's, every draw reads it afresh, so a kernel may rewrite it in-stream and the next lock-step's draw sees the new
 * values.  With no table attached the env launches the kernel it launched before tables existed. */
int bridges_env_set_family_thresholds(bridges_env* env, const uint64_t* thr_dev /* [C-1] or NULL */);

/* --- stand-alone operators (same kernels, caller-shaped batches) ------------ */
/* K1: create_block / align_frames_2d (gym_env.py:204-216, geometry.py:39-50).
 * frame1: [n,6] target frame (c.xz, t.xz, n.xz); shape_id,face: [n]; ox,oy: [n]
 * -> pose [n,4], verts [n,6,2].  A NULL array with n > 0 returns -1 and launches nothing. */
int bridges_place(const bridges_shape* shapes_dev, int32_t n, const double* frame1, const int32_t* shape_id,
                  const int32_t* face, const double* ox, const double* oy, double* pose, double* verts,
                  void* stream);
/* K1 as AssemblyGym.create_block (gym_env.py:204-216): target = floor (target_face[i] < 0) or face target_face[i]
 * of a posed block (target_verts [n,6,2], target_shape [n]; read only for items with target_face[i] >= 0, so they may be
 * NULL when every target is the floor).  target_frame_out [n,6] may be NULL.  A NULL target_face, shape_id, face, ox, oy, pose or
 * verts with n > 0 returns -1 and launches nothing. */
int bridges_create_block(const bridges_shape* shapes_dev, int32_t n, const double* target_verts,
                         const int32_t* target_shape, const int32_t* target_face, const int32_t* shape_id,
                         const int32_t* face, const double* ox, const double* oy, double* pose, double* verts,
                         double* target_frame_out, void* stream);
/* Block.__init__ (assembly_env.py:146-153): world vertices of shapes posed by (x, z, cos, sin): shape_id [n], pose [n,4] ->
 * verts [n,6,2] (slots >= nv are 0).  A NULL array with n > 0 returns -1 and launches nothing. */
int bridges_pose_block(const bridges_shape* shapes_dev, int32_t n, const int32_t* shape_id, const double* pose,
                       double* verts, void* stream);
/* Shape.get_face_frame_2d on posed blocks (assembly_env.py:118-124): frames [n,6,6] = centre.xz, x-axis.xz, normal.xz (slots
 * >= nv are 0).  A NULL array with n > 0 returns -1 and launches nothing. */
int bridges_face_frames(const bridges_shape* shapes_dev, int32_t n, const int32_t* shape_id, const double* verts,
                        double* frames, void* stream);
/* Shape.contains_2d (assembly_env.py:126-137) of ONE posed block for n arbitrary points (x, z):
 * verts [6,2], points [n,2] f64 -> inside [n] u8.  A NULL array with n > 0, or shape_id < 0, returns -1 and launches nothing. */
int bridges_contains_points(const bridges_shape* shapes_dev, int32_t shape_id, const double* verts, int32_t n,
                            const double* points, uint8_t* inside, void* stream);
/* K4: render_blocks_2d (rendering.py:105-113) of n posed outlines, one image each.
 * verts [n,6,2] world vertices in shape-vertex order, shape_id [n], grid_x/grid_y [64] DEVICE
 * -> bits [n,64] and/or f32 [n,64,64] (either may be NULL).  A NULL verts, shape_id, grid_x or grid_y with n > 0 returns -1 and
 * launches nothing. */
int bridges_raster(const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                   const double* grid_x, const double* grid_y, uint64_t* bits, float* img, void* stream);
/* render_blocks_2d (rendering.py:105-113) at any image size (the reference's default is 512 x 512): the UNION of n posed
 * outlines on the pixel grid grid_x [W] x grid_y [H] (DEVICE; row 0 = grid_y[0]) -> out [H, W] u8 {0, 1}.  Same pixel test,
 * operation for operation, as the 64-wide rasterisers. */
int bridges_render_blocks(const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                          const double* grid_x, int32_t W, const double* grid_y, int32_t H, uint8_t* out, void* stream);
/* The same for S x S images, 2 <= S <= 64 (render_blocks_2d's img_size argument, rendering.py:105): grid_x/grid_y
 * hold S values; the outputs keep the 64-word / 64x64 layout, the image is the top-left S x S corner, the rest 0.  A NULL verts,
 * shape_id, grid_x or grid_y with n > 0 returns -1 and launches nothing. */
int bridges_raster_sized(const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                         const double* grid_x, const double* grid_y, int32_t size, uint64_t* bits, float* img,
                         void* stream);
/* get_action_features + filter_actions + the rollout's linear reward, fused, for n posed candidate outlines against one
 * state (successor_dqn.py:84-94, 397-401; actions.py:71-82; gym_env.py:304-323): bits [n,64] u64 and / or img [n,64,64] f32
 * (either may be NULL) = the rasters; mask [n] u8 = every vertex inside [xlim, ylim] and above z = 0 (tolerance 1e-6) and
 * no pixel in common with state_bits | obstacle_bits ([64] u64 each, may be NULL = empty); lin_reward [n] f32 =
 * sum(raster * reward_map) taken from reward_prefix ([64,65] f64 row prefix sums of the map, see bridges_env_buffers).
 * size = S of an S x S image (grid_x / grid_y hold S samples).  The lock-step does the same inside bridges_env_step. */
int bridges_action_features(const bridges_shape* shapes_dev, int32_t n, const double* verts, const int32_t* shape_id,
                            const double* grid_x, const double* grid_y, int32_t size, double xlim0, double xlim1, double ylim0,
                            double ylim1, const uint64_t* state_bits, const uint64_t* obstacle_bits, const double* reward_prefix,
                            uint64_t* bits, float* img, uint8_t* mask, float* lin_reward, void* stream);
/* OR-reduce groups of bit rasters: out[g] = OR bits[ranges[g][0] .. ranges[g][1]);  ranges int32 [n_groups,2]; an empty range
 * gives 64 zero words.  A NULL pointer with n_groups > 0 returns -1 and launches nothing. */
int bridges_bits_or(int32_t n_groups, const int32_t* ranges, const uint64_t* bits, uint64_t* out, void* stream);
/* bit raster -> f32 image.  A NULL pointer with n > 0 returns -1 and launches nothing. */
int bridges_bits_to_f32(int32_t n, const uint64_t* bits, float* img, void* stream);
/* The stacked input of the conv Q-networks (ConvNet / UNet, cv.py's cat([block, action, reward, obstacle], dim=1)) in one pass:
 * x [n_rows, 4, 64, 64] f32, contiguous NCHW, row r =
 *   channel 0: raster(block_bits [*,64] u64 row block_row[r]),  channel 1: raster(action_bits [*,64] u64 row action_row[r])
 *              -- the bit order of bridges_bits_to_f32 / bridges_bits_linear (pixel (y, x) = bit x of word y), exactly 0.0f / 1.0f;
 *   channel 2: the 4096 floats at reward + reward_row[r] * reward_stride, copied bit for bit (NaN payloads, -0.0, denormals);
 *   channel 3: the raster of the 64 words at obstacle_bits + obstacle_row[r] * obstacle_stride.
 * A NULL *_row = row r itself (the convention of bits_row).  reward_stride must be 0 or 4096, obstacle_stride 0 or 64 (0 = one
 * shared map / raster for every row); any other stride, n_rows < 0, a NULL data pointer or NULL x returns -1 and launches
 * nothing; n_rows == 0 succeeds and launches nothing.  reward and x must be 16-byte aligned.  Index values are the caller's
 * contract, as for bridges_bits_linear. */
int bridges_conv_input_rows(int32_t n_rows, const uint64_t* block_bits, const int64_t* block_row, const uint64_t* action_bits,
                            const int64_t* action_row, const float* reward, const int64_t* reward_row, int64_t reward_stride,
                            const uint64_t* obstacle_bits, const int64_t* obstacle_row, int64_t obstacle_stride, float* x,
                            void* stream);
/* K8: linear layer over flattened binary 64x64 rasters, fed with the bit-packed rasters (replaces the product of
 * SuccessorMLP's first layer with the action / block image, robotoddler/models/cv.py:95-97):
 *   out[r, :] = (base ? base[base_row ? base_row[r] : 0, :] : 0) + sum_{p set in bits[bits_row ? bits_row[r] : r]} wt[p, :]
 * bits [*,64] u64 (row y of an image = one word, bit x = pixel (y, x), flattened pixel p = 64*y + x);
 * wt [4096, d] f32 = the transposed weight slice; base [*, d]; out [n_rows, d]; d % 4 == 0; pixels are added in
 * ascending p, so the result is deterministic. */
int bridges_bits_linear(int32_t n_rows, const uint64_t* bits, const int64_t* bits_row, const float* wt, int32_t d,
                        const float* base, const int64_t* base_row, float* out, void* stream);
/* K8 with TWO bit-packed operands in one launch (per-env obstacles: the state raster on W_block and the env's obstacle raster
 * on W_obst):  out[r, :] = base term + sum_{p set in bits_a[bits_row_a ? bits_row_a[r] : r]} wt_a[p, :]
 *                                    + sum_{p set in bits_b[bits_row_b ? bits_row_b[r] : r]} wt_b[p, :]
 * added in that order (base, a's pixels ascending, b's pixels ascending): the float sequence of bridges_bits_linear on a followed by
 * bridges_bits_linear on b with the first result as base, so the output equals the chained calls bit for bit.  Arguments as in
 * bridges_bits_linear (d % 4 == 0, NULL bits_row_* = identity, NULL base = 0; wt_a / wt_b [4096, d]). */
int bridges_bits_linear2(int32_t n_rows, const uint64_t* bits_a, const int64_t* bits_row_a, const float* wt_a, const uint64_t* bits_b,
                         const int64_t* bits_row_b, const float* wt_b, int32_t d, const float* base, const int64_t* base_row,
                         float* out, void* stream);
/* EpsilonGreedy's count-based exploration (successor_dqn.py:112-131) on bit-packed rasters, for many environments at once:
 * bridges_bits_dot: out[r] = sum(img[slot[r]] * raster(bits[bits_row[r]])) -- the overlap of candidate r with the count image of
 * its episode step (img [n_slots,64,64] f32, slot [n] i64; bits_row NULL = identity);
 * bridges_bits_accumulate: img[slot[r]] += weight[r] * raster(bits[bits_row[r]]) (weight NULL = 1; float atomics on the set
 * pixels).  The count images hold small integers, so both are exact whatever the order of the additions. */
int bridges_bits_dot(int32_t n_rows, const uint64_t* bits, const int64_t* bits_row, const float* img, const int64_t* slot,
                     float* out, void* stream);
int bridges_bits_accumulate(int32_t n_rows, const uint64_t* bits, const int64_t* bits_row, const float* weight,
                            const int64_t* slot, float* img, void* stream);
/* The same head with the product inside: out[r] = sum_j w[j] * sigmoid(h[r,:] . Wd[j,:] + bd[j]), h [n, K = 256] (row stride
 * h_stride floats), Wd [N, 256] row-major (= W_out[px:2px] - W_out[:px] of SuccessorMLP), on the f32 matrix cores; the [n, N]
 * product is never written.  splits > 1 cuts the N columns into that many ranges per 128-row workgroup (so that a launch fills
 * the 256 CUs evenly; the ranges' sums go to part [splits, n] and are added in a fixed order: no atomics, deterministic). */
int bridges_head_sigmoid_dot(int32_t n_rows, int32_t K, int32_t N, const float* h, int64_t h_stride, const float* Wd,
                             const float* bd, const float* w, float* out, float* part, int32_t splits, void* stream);
/* The same head with one map PER TASK (per-env tasks: every env owns a reward map): w_all [n_maps, N] row-major, w_row [n_rows]
 * int32 = the map of row r (its env), out[r] = sum_j w_all[w_row[r]][j] * sigmoid(...).  n_maps * N < 2^31; the entries of
 * w_row must lie in [0, n_maps) (not checked on the device).  Same kernel, products, split scheme and summation order: with
 * every w_row naming one map the result equals bridges_head_sigmoid_dot on that map bit for bit. */
int bridges_head_sigmoid_dot_rows(int32_t n_rows, int32_t K, int32_t N, const float* h, int64_t h_stride, const float* Wd,
                                  const float* bd, const float* w_all, const int32_t* w_row, int32_t n_maps, float* out, float* part,
                                  int32_t splits, void* stream);
/* out[r] = sum_j w[j] * sigmoid(d[r * row_stride + j]), j < k: the q head of SuccessorMLP's factored forward
 * (q = sum(softmax(psi)[:, 1] * reward_map), cv.py:101-104, with psi1 - psi0 = d) in one pass.  k % 4 == 0. */
int bridges_sigmoid_dot(int32_t n_rows, const float* d, int64_t row_stride, const float* w, int32_t k, float* out,
                        void* stream);
/* out[r] = sum_j w_all[w_row[r]][j] * sigmoid(d[r * row_stride + j]): w_all [*, k] row-major, w_row [n_rows] int32. */
int bridges_sigmoid_dot_rows(int32_t n_rows, const float* d, int64_t row_stride, const float* w_all, const int32_t* w_row, int32_t k,
                             float* out, void* stream);
/* K2+K3: is_stable_rbe (stability.py:49-71) for n independent assemblies given as
 * padded block lists.  verts [n,K,6,2], shape_id [n,K], n_blocks [n], fixed_mask [n] (bit b = block b
 * is_static)
 * -> stable [n] u8, info [n,8] f64 (phase-1 objective, n_interfaces, pivots, error, shader cycles spent in
 *    interface detection, shader cycles spent in the LP, 0, 0).
 * lp_ws: [n, lp_ws_stride] doubles, lp_ws_stride >= 9*MAX_INTERFACES + (3K+2)*(4*MAX_INTERFACES+3).
 * On return row e of lp_ws begins with the contact list found for assembly e (the rest of the row is the tableau overflow
 * area, scratch): 8*MAX_INTERFACES doubles of if_geom (p_lo.xz, p_hi.xz, n.xz, t.xz per interface, the layout of
 * bridges_env_buffers.if_geom), then MAX_INTERFACES int32 pairs (body A with -1 for the floor, body B), i.e. another
 * MAX_INTERFACES doubles.  Interfaces are ordered by (body B, body A, face of A, face of B); only the first info[1] entries
 * are valid, and when more than MAX_INTERFACES contacts exist the first MAX_INTERFACES are kept and info[3] is set.
 * bridges_stability_penalty leaves the same list. */
int bridges_stability(const bridges_shape* shapes_dev, int32_t n, int32_t K, const double* pose,
                      const double* verts, const int32_t* shape_id, const int32_t* n_blocks,
                      const uint32_t* fixed_mask, double mu, double density, double floor_half_width,
                      double floor_depth, uint8_t* stable, double* info, double* lp_ws, int64_t lp_ws_stride,
                      void* stream);
/* is_stable_rbe_penalty (assembly_gym/assembly_gym/utils/stability.py:75-88; compas_cra rbe_solve(penalty=True) +
 * maximum_tension, assembly_gym/assembly_gym/utils/geometry.py:132-143): contact points may also pull; stable iff some
 * equilibrium keeps the total tension <= tension_tol (> 0; 0 = plain is_stable_rbe).  forces (may be NULL):
 * [n, MAX_INTERFACES, 2, 3] = per contact point (compression c_np, tension c_nn, tangential force) of the equilibrium
 * found, zeros when unstable.  No output of the reference pins this variant ("parity unpinned"). */
int bridges_stability_penalty(const bridges_shape* shapes_dev, int32_t n, int32_t K, const double* pose,
                              const double* verts, const int32_t* shape_id, const int32_t* n_blocks,
                              const uint32_t* fixed_mask, double mu, double density, double floor_half_width,
                              double floor_depth, double tension_tol, uint8_t* stable, double* info, double* forces,
                              double* lp_ws, int64_t lp_ws_stride, void* stream);
/* upload a shape table; returns a device pointer the stand-alone operators take. */
int bridges_shapes_upload(const bridges_shape* shapes_host, int32_t n_shapes, bridges_shape** out_dev);
int bridges_shapes_free(bridges_shape* dev);

/* Environments in the same state: rep[e] = the smallest env index whose state -- n_blocks and the shape id, pose (bit
 * pattern) and face occupancy of its live block slots, plus the caller's flag[e] byte (may be NULL) -- equals env e's word
 * for word (found through a 64-bit hash, hkey [E] scratch, then verified: a hash collision costs the sharing, never
 * correctness).  What a Q-network is asked about a state (its candidate rows, their values) depends on the state alone, so
 * the envs of a group share their representative's rows (bridges_valid_rows with rep).  K = block slots per env (<= 64). */
int bridges_env_groups(int32_t E, int32_t K, const int32_t* n_blocks, const int32_t* blk_shape, const double* blk_pose,
                       const uint8_t* blk_occ, const uint8_t* flag, uint64_t* hkey, int32_t* rep, void* stream);
/* The same with n_extra further 64-bit words per env as part of its identity (extra [E, n_extra]; NULL / 0 = none, which is
 * what bridges_env_groups passes): folded into the hash and compared word for word.  Per-env tasks pass the bit patterns of
 * env_targets[e] (3 T words): what a network is asked about a state then depends on (state, task). */
int bridges_env_groups_keyed(int32_t E, int32_t K, const int32_t* n_blocks, const int32_t* blk_shape, const double* blk_pose,
                             const uint8_t* blk_occ, const uint8_t* flag, const uint64_t* extra, int32_t n_extra, uint64_t* hkey,
                             int32_t* rep, void* stream);

/* The rows a Q-network is fed (filter_actions, actions.py:71-82, for every env at once): compact indices of the candidates
 * with cand_mask != 0, env-major in candidate order, their owning env, and seg[e] .. seg[e + 1] = the rows of env e
 * (seg [E + 1]; n_valid[e] = the env's count, as bridges_env_step leaves it).  idx / row_env need room for every candidate.
 * With rep (bridges_env_groups; may be NULL) only the envs with rep[e] == e get rows; seg_lo[e] .. seg_hi[e] ([E] each; may
 * both be NULL when rep is) is then the row range of env e's representative -- the rows every env of the group reads.
 * The total goes to *h_total, a HOST-visible word (pinned, device-accessible): valid once the stream has passed the call. */
int bridges_valid_rows(int32_t E, const int32_t* cand_offset, const int32_t* n_cand, const int32_t* n_valid, const uint8_t* cand_mask,
                       const int32_t* rep, int32_t* seg, int32_t* seg_lo, int32_t* seg_hi, int64_t* idx, int64_t* row_env,
                       int32_t* h_total, void* stream);

/* EpsilonGreedy.select (successor_dqn.py:98-132) for every env at once.  Rows seg_lo[e] .. seg_hi[e] of q / join / idx belong to
 * env e (bridges_valid_rows; a prefix-sum array seg is passed as seg, seg + 1); rep (may be NULL): the env whose candidates
 * those rows index (bridges_env_groups).  The env explores when u[e] <= eps and greedy == 0: its row is then the FIRST minimum of join (the
 * overlap of the candidate raster with the count image of the env's episode step), else the FIRST maximum of q.
 * -> sel_compact[e] = idx[row], sel_index[e] = max(sel_compact - cand_offset[rep ? rep[e] : e], 0), q_sel[e] = q[row],
 *    explore_w[e] = 1 if the env explored (the weight of its count-image update) -- an env without rows: idx[0], 0, 0. */
int bridges_eps_greedy_select(int32_t E, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, const float* join,
                              const float* u, float eps, int32_t greedy, const int64_t* idx, const int32_t* cand_offset,
                              const int32_t* rep, int64_t* sel_compact, int32_t* sel_index, float* q_sel, float* explore_w, void* stream);

/* Boltzmann exploration for every env at once: env e draws one of its rows lo = seg_lo[e] .. hi - 1 = seg_hi[e] - 1 of q / idx
 * (as for bridges_eps_greedy_select; rep may be NULL) with probability proportional to exp(q / temperature).  The rule, in
 * float64, with T = (double)temperature > 0 and the uniform draw u[e] in [0, 1):
 *   - a row is ELIGIBLE if its q is neither NaN nor -inf; m = the largest eligible q;
 *   - weights: w_j = exp(((double)q_j - m) / T) for an eligible row, 0 for any other; if m is +inf: 1 for the +inf rows, else 0;
 *   - c_j = w_lo + .. + w_j in row order, total = c_{hi-1}, target = (double)u[e] * total;
 *   - the row is the first j with c_j > target (strict); if rounding leaves none, the last row with w_j > 0;
 *   - p_sel[e] = w_row / total, rounded to float32 once;
 *   - no row eligible: row lo, p_sel 0, explore_w 0;  no rows (hi <= lo): row 0, q_sel 0, p_sel 0, explore_w 0;
 *   - explore_w[e] = 1 if the env has rows and the row is not the first maximum among its eligible rows, else 0;
 *   - greedy != 0: the row, sel_* and q_sel of bridges_eps_greedy_select(greedy = 1) on the same q, p_sel 1 (0 without rows),
 *     explore_w 0.
 * sel_compact[e] = idx[row], sel_index[e] = max(sel_compact - cand_offset[rep ? rep[e] : e], 0), q_sel[e] = q[row]; the row is
 * clamped to n_rows - 1.  T -> 0 draws uniformly among the exact ties of the maximum, T -> inf uniformly among the eligible rows,
 * and q / T far above 709 cannot overflow (the exponent is never positive).  Envs that share rows draw each with their own u[e].
 * The order of every sum is fixed: the same inputs give the same bits.  The device's prefix sums are added in another order than
 * c_j above (a scan per 64 rows), so a target within a few ulp of a c_j may fall to the neighbouring row.
 * E == 0: nothing to do.  Refused: n_rows < 1, a temperature that is not finite or not > 0, a NULL array (rep excepted). */
int bridges_boltzmann_select(int32_t E, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, const float* u,
                             float temperature, int32_t greedy, const int64_t* idx, const int32_t* cand_offset, const int32_t* rep,
                             int64_t* sel_compact, int32_t* sel_index, float* q_sel, float* explore_w, float* p_sel, void* stream);

/* RELATIVE TEMPERATURE: bridges_boltzmann_select and bridges_soft_expect at a temperature that is a multiple of each segment's own
 * standard deviation of q, formed on the device in the same launch.  The rule, stated once for both operators; select_q is the
 * array that weighs the rows (q for the select), segment e has its rows lo .. hi - 1:
 *   - SPREAD: the FINITE rows are those whose select_q is neither NaN nor +-inf, n_f their number.  n_f < 2: s = 0.  Otherwise
 *     mean = (sum (double)q_j) / n_f over the finite rows and s = sqrt(sum ((double)q_j - mean)^2 / n_f): the population standard
 *     deviation, in two passes (the mean first, then the squared deviations; never E[x^2] - mean^2), float64 throughout, every sum
 *     in a fixed order of the kernel's own (lane-strided partial sums combined by a fixed tree), so equal inputs give equal bits.
 *   - EFFECTIVE TEMPERATURE: T_e = (double)temperature * fmax(s, (double)spread_floor), written as a double to temp_out[e]; the
 *     floor keeps T_e > 0 where a segment's rows tie.  An empty segment, or one without finite rows, still writes
 *     (double)temperature * (double)spread_floor.
 *   - everything else is the scalar operator's rule at T = T_e, word for word: eligibility, m, the weights and the m = +inf case,
 *     the strict inverse CDF with its fall-back row, p_sel and explore_w; value, feat_mean, entropy, argmax_row and the
 *     nothing-eligible outputs.
 *   - bridges_boltzmann_select_rel with greedy != 0 is bridges_boltzmann_select(greedy = 1) operand for operand; it writes
 *     temp_out[e] = 0 and takes no spread.
 * The argument lists are the scalar siblings' with spread_floor behind temperature and temp_out [E] / [n_trans] f64 before the
 * stream; one launch, no atomics, no scratch, every output word written once.  Refused: whatever the sibling refuses; a
 * spread_floor that is not finite or not > 0; a temp_out that is NULL or not 8-byte aligned. */
int bridges_boltzmann_select_rel(int32_t E, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, const float* u,
                                 float temperature, float spread_floor, int32_t greedy, const int64_t* idx, const int32_t* cand_offset,
                                 const int32_t* rep, int64_t* sel_compact, int32_t* sel_index, float* q_sel, float* explore_w,
                                 float* p_sel, double* temp_out, void* stream);

/* Beam search: the top-B candidates of every group of B beams.  E = G * B envs, group g owns envs gB .. gB + B - 1; rows
 * seg_lo[e] .. seg_hi[e] of q / idx belong to env e exactly as for bridges_eps_greedy_select (rep may be NULL).  Inputs per env:
 * live[e] u8 (the beam is still open), ret[e] f64 (its discounted return so far), disc[e] f64 (the discount of its next reward).
 *   - SCORE of row j of a live env e: S = ret[e] + disc[e] * (double)q[j] -- two binary64 operations, no contraction;
 *   - a row whose q is NaN or -inf is not a candidate (nor is one whose S is NaN); a dead env has no candidates;
 *   - ORDER: S descending, then q descending, then env ascending, then row ascending (with one live beam and B = 1: the first
 *     maximum of q, the choice of bridges_eps_greedy_select(greedy = 1));
 *   - slot i < B of group g takes the i-th candidate of the group in that order: src[gB + i] = its env, sel_compact = idx[row],
 *     sel_index = max(sel_compact - cand_offset[rep ? rep[env] : env], 0), q_sel = q[row], score = S, live_out = 1;
 *   - a slot beyond the group's number of candidates: src = the slot's own env, sel_compact 0, sel_index 0, q_sel 0, score -inf,
 *     live_out 0.
 * src is what bridges_env_fork takes, sel_index what the step after it places.  One workgroup per group, B rounds of an arg-max
 * in a strict total order: no atomics, the same bits on every call.  Rows outside [0, n_rows) are not read.
 * 1 <= B <= 16.  Refused: B outside that, E % B != 0, n_rows < 1, a NULL array other than rep, a misaligned pointer.  E == 0
 * returns 0 and launches nothing. */
int bridges_beam_select(int32_t E, int32_t B, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q,
                        const int64_t* idx, const int32_t* cand_offset, const int32_t* rep, const uint8_t* live, const double* ret,
                        const double* disc, int32_t* src, int64_t* sel_compact, int32_t* sel_index, float* q_sel, double* score,
                        uint8_t* live_out, void* stream);

/* Particle search: best-of-N rollouts with resampling, the sampled sibling of bridges_beam_select.  Layout, seg_lo / seg_hi / q /
 * idx / cand_offset / rep / live / ret / disc and the outputs src .. live_out exactly as there; u_act f32 [E] holds one uniform
 * draw in [0, 1) per slot, u_res f32 [G] one per group.  All arithmetic is binary64 without contraction; T = (double)temperature,
 * T_r = (double)resample_temperature.
 *   - ELIGIBLE row: its q is neither NaN nor -inf (bridges_boltzmann_select's word);
 *   - PARENT: a live env with at least one eligible row whose VALUE S_e = ret[e] + disc[e] * (double)v_e, v_e the env's largest
 *     eligible q, is neither NaN nor -inf (two operations, as bridges_beam_select's score).  A dead env is never a parent;
 *   - RESAMPLING WEIGHTS over the parents of a group, in env order: M = max S, W_p = exp((S_p - M) / T_r); with T_r = +inf every
 *     W_p = 1 (whatever M is); otherwise with M = +inf W_p = 1 for the +inf parents and 0 for the others.  C_p = the inclusive
 *     prefix sum of W in env order, added one by one, total = C_last, ess[g] = total^2 / sum W_p^2 (0 for a group without parents);
 *   - SYSTEMATIC RESAMPLING: slot k = 0 .. B - 1 has the target t_k = ((double)u_res[g] + k) / B * total and takes the first parent
 *     p with C_p > t_k (strict); if rounding leaves none, the last parent with W_p > 0;
 *   - ELITE (elite != 0): slot 0 is overridden after that assignment: its parent is the first parent of maximal S (env
 *     ascending), its row that parent's first maximum of q, its p_sel 1;
 *   - ACTION DRAW of every other slot: the rule of bridges_boltzmann_select word for word -- the weights with their m = +inf case,
 *     the strict inverse CDF, the fall-back row, p_sel -- over the PARENT's rows at T with the draw u_act[gB + k];
 *   - slot gB + k: src = the parent p, sel_compact = idx[row], sel_index = max(sel_compact - cand_offset[rep ? rep[p] : p], 0),
 *     q_sel = q[row], score = ret[p] + disc[p] * (double)q[row], live_out = 1, p_sel as drawn (f32, rounded once);
 *   - a group without parents writes bridges_beam_select's empty slot to every slot (src = the slot's own env, sel_compact 0,
 *     sel_index 0, q_sel 0, score -inf, live_out 0) with p_sel 0.
 * Two exact properties.  With T_r = +inf, elite == 0 and all B envs of a group parents, C_p = p + 1 and t_k = (u + k) / B * B lies
 * in [k, k + 1), so src[gB + k] = gB + k: no particle moves, the group is B independent rollouts (the best-of-N control).  With
 * B = 1 and elite != 0 the outputs src .. live_out equal bridges_beam_select(B = 1)'s wherever ret is finite and disc > 0 (the
 * largest q then has the largest score).
 * One launch, one workgroup per group; no atomics, no scratch; every output word is written exactly once; every sum has a fixed
 * order, so the same inputs give the same bits.  The parent draw adds its prefix sums in the order above; the action draw adds
 * them as bridges_boltzmann_select does, so a target within a few ulp of a c_j may fall to the neighbouring row.  Rows outside
 * [0, n_rows) are never read.  1 <= B <= 16.
 * Refused (-1, nothing launched): whatever bridges_beam_select refuses; a temperature that is not finite or not > 0; a
 * resample_temperature that is NaN or not > 0 (+inf is allowed); a NULL array other than rep; a misaligned pointer.  E == 0
 * returns 0 and launches nothing. */
int bridges_particle_select(int32_t E, int32_t B, int32_t n_rows, const int32_t* seg_lo, const int32_t* seg_hi, const float* q,
                            const int64_t* idx, const int32_t* cand_offset, const int32_t* rep, const uint8_t* live, const double* ret,
                            const double* disc, const float* u_act, const float* u_res, float temperature,
                            float resample_temperature, int32_t elite, int32_t* src, int64_t* sel_compact, int32_t* sel_index,
                            float* q_sel, double* score, uint8_t* live_out, float* p_sel, double* ess, void* stream);

/* Beam search: the beams of a group that hold the same structure, reached by whatever order of placements.  E = G * B envs, group
 * g owns envs gB .. gB + B - 1 as for bridges_beam_select; the caller guarantees that the envs of a group share one task.  The
 * state arrays are the env's own (n_blocks [E], blk_shape [E, K], blk_pose [E, K, 4], blk_occ [E, K], targets_left [E]: the env's
 * 4-byte word, as the fork table copies it); live u8 [E], ret f64 [E] as for bridges_beam_select.
 *   - BLOCK TUPLE of live slot i < nb of env e, nb = n_blocks[e] clamped to [0, K]: the shape id as u32, the occupancy byte, and
 *     the four pose words as 64-bit BIT PATTERNS -- no float comparison, so -0.0 != 0.0 (that costs a merge, never correctness);
 *   - KEY of env e: nb; targets_left[e] (the order of placements can change which targets count as reached); with key_last != 0
 *     the tuple of slot nb - 1 (absent when nb = 0); and the SORTED MULTISET of the tuples of slots 0 .. nb - 1 -- equal tuples
 *     inside one env count with their multiplicity;
 *   - EQUIVALENCE: two LIVE envs of the SAME group are equivalent iff their keys are equal word for word (nothing is accepted on
 *     a hash); a dead env and envs of other groups never match;
 *   - REPRESENTATIVE of a class: its first env by ret descending (a binary64 >; a NaN ret ranks below every number), then env
 *     index ascending;
 *   - rep[e] = the representative of e's class (e itself for a dead env), live_out[e] = live[e] && rep[e] == e, n_merged[g] = the
 *     number of live envs of group g that were closed (live[e] && rep[e] != e).
 * One workgroup per group: every env's tuples are sorted into LDS (ties by slot index, so the order is total), then every env is
 * held against the other live envs of its group.  No atomics, no scratch, every output written exactly once, the same bits on
 * every call; no output may alias an input.  1 <= B <= 16, 1 <= K <= 64.  Refused (-1, nothing launched): E < 0, B or K outside
 * those, E % B != 0, a NULL array, a misaligned pointer.  E == 0 returns 0 and launches nothing. */
int bridges_beam_merge(int32_t E, int32_t B, int32_t K, const int32_t* n_blocks, const int32_t* blk_shape, const double* blk_pose,
                       const uint8_t* blk_occ, const int32_t* targets_left, const uint8_t* live, const double* ret, int32_t key_last,
                       int32_t* rep, uint8_t* live_out, int32_t* n_merged, void* stream);

/* --- transition records of the vectorised loop ------------------------------------------------------------------
 * One float64 row per transition: the compact form of the reference's Transition (successor_dqn.py:27-44) -- the block
 * list of s, the placed block and the scalars; rasters and candidate sets are re-generated when a record is sampled.
 * Integers are stored exactly as float64.  The same rows are what the ranks all-gather per lock-step. */
#define BRIDGES_REC_K 16                                    /* block slots of a record */
#define BRIDGES_REC_NB 0                                    /* n_blocks of s */
#define BRIDGES_REC_SHAPE 1                                 /* [K] shape ids */
#define BRIDGES_REC_POSE (1 + BRIDGES_REC_K)                /* [K][4] (x, z, cos, sin) */
#define BRIDGES_REC_OCC (1 + 5 * BRIDGES_REC_K)             /* [K] face-occupancy bit masks */
#define BRIDGES_REC_ASHAPE (1 + 6 * BRIDGES_REC_K)          /* action: shape id, pose[4], target_block, target_face, face */
#define BRIDGES_REC_APOSE (BRIDGES_REC_ASHAPE + 1)
#define BRIDGES_REC_ATB (BRIDGES_REC_APOSE + 4)
#define BRIDGES_REC_ATF (BRIDGES_REC_APOSE + 5)
#define BRIDGES_REC_AFACE (BRIDGES_REC_APOSE + 6)
#define BRIDGES_REC_REWARD (BRIDGES_REC_AFACE + 1)
#define BRIDGES_REC_LIN (BRIDGES_REC_REWARD + 1)
#define BRIDGES_REC_DONE (BRIDGES_REC_REWARD + 2)           /* terminated | truncated | no next action */
#define BRIDGES_REC_STABLE_S (BRIDGES_REC_REWARD + 3)
#define BRIDGES_REC_STABLE_N (BRIDGES_REC_REWARD + 4)       /* stable(s') with the last block frozen */
#define BRIDGES_REC_TD (BRIDGES_REC_STABLE_N + 1)           /* rollout td_error (successor_dqn.py:413-426), 0 unless prioritised */
#define BRIDGES_REC_WIDTH (BRIDGES_REC_TD + 1)              /* 111 doubles = 888 B */
/* Before the lock-step's step: state s of every env (the env's own arrays, K = its block slots <= 16) and the candidate
 * sel_row[e] (compact row of cand_desc / cand_pose) it is about to place -> rec[e, 0 : REC_REWARD], stable(s); the rest 0. */
int bridges_record_state(int32_t E, int32_t K, const int32_t* n_blocks, const int32_t* blk_shape, const double* blk_pose,
                         const uint8_t* blk_occ, const uint8_t* step_flags, const int64_t* sel_row, const int32_t* cand_desc,
                         const double* cand_pose, double* rec, void* stream);
/* After it: reward, lin_reward, done | no_actions, stable(s') into the same rows; valid[e] = the lock-step was a real
 * env-step of env e (reset-only lock-steps are not transitions). */
int bridges_record_result(int32_t E, const float* reward, const float* lin_reward, const uint8_t* step_flags, double* rec,
                          uint8_t* valid, void* stream);
/* Per-episode statistics (log_episode, successor_dqn.py:479-499) of one lock-step's records rec [E, REC_WIDTH] / valid [E], taken
 * before the all-gather.  gpow [K] = float32(gamma ** i); run [E, 2] (running discounted reward / lin_reward) and counted [E]
 * persist between calls.  Per valid env: i = rec[NB]; i == 0 restarts run; run += gpow[i] * (reward, lin_reward) in float32
 * without fused multiply-add; at REC_DONE, unless count_first_only and counted > 0, out[0..5] += (1, run[0], run[1], i + 1,
 * REC_STABLE_N, reward == n_targets), then counted++.  out [8] float64 is added to in place (slots 6, 7 spare); one workgroup,
 * fixed-order reduction (bitwise reproducible), no allocation; E == 0 is a no-op. */
int bridges_episode_stats(int32_t E, int32_t K, const double* rec, const uint8_t* valid, const float* gpow, int32_t n_targets,
                          int32_t count_first_only, float* run, int32_t* counted, double* out, void* stream);
/* The same fold by class (the spans / heights of a task family): an ended episode of env e is added to row cls[e] of
 * out [n_classes, 8], 1 <= n_classes <= 8; cls [E] is the class the episode was played under (bridges_task_family.task_class as
 * it was BEFORE the step that ended the episode, which redraws it).  A cls[e] outside [0, n_classes) is counted in no row but
 * still advances run and counted.  One workgroup, one fixed-order reduction per row, no atomics; with n_classes = 1 and cls all
 * zero, out, run and counted are bridges_episode_stats' bit for bit (both launch one kernel template: bridges_episode_stats is
 * its instance without classes). */
int bridges_episode_stats_by_class(int32_t E, int32_t K, const double* rec, const uint8_t* valid, const float* gpow,
                                   int32_t n_targets, int32_t count_first_only, const int32_t* cls, int32_t n_classes, float* run,
                                   int32_t* counted, double* out /* [n_classes, 8] */, void* stream);
/* Task-family operators (bridges_env_set_family_thresholds has the formulas).
 * bridges_family_thresholds: thr_dev [C-1] from the weights w_dev [C] on the device, 1 <= C <= 8 (C == 1: nothing to write,
 * nothing is enqueued).  The weights live in device memory, so neither their sum nor their size is knowable here without a
 * host wait: a weight above 2^20 is taken as 2^20, and sum(w) == 0 writes the table of equal weights.  (A caller that holds
 * the weights on the host -- bridges_hip.vec_env.RandomBridges(weights=...) -- refuses both before anything is enqueued.) */
int bridges_family_thresholds(const uint32_t* w_dev, int32_t C, uint64_t* thr_dev, void* stream);
/* The class draw of a family on caller-shaped batches: n_out[i] = the class env env_id_base + i draws in its episode
 * episode[i] under (seed, n_lo, n_hi) and the table thr [n_hi - n_lo] (NULL: the uniform draw) -- the function
 * bridges_env_reset / _step run inside their task kernel.  0 <= n_lo <= n_hi, at most 8 classes. */
int bridges_family_draw(uint64_t seed, int32_t env_id_base, int32_t E, const uint32_t* episode /* [E] */, int32_t n_lo, int32_t n_hi,
                        const uint64_t* thr /* or NULL */, int32_t* n_out /* [E] */, void* stream);
/* Curriculum update: move the draw towards the classes the policy fails on.  sums [n_classes, 8] float64 has the layout of
 * bridges_episode_stats_by_class (row = class n, slot 0 = episodes, slot 5 = successes), state [n_classes, 2] float64 =
 * (ema, seen); rows outside [n_lo, n_hi] are neither read nor written.  For n in n_lo..n_hi, e = sums[n][0]:
 *   e >= min_episodes:  rate = sums[n][5] / e;  ema = seen ? ema + beta * (rate - ema) : rate;  seen = 1;  sums[n][:] = 0
 *                       (binary64, every operation rounded separately, no contraction)
 *   e <  min_episodes:  the row stays and keeps accumulating
 *   fail = seen ? min(max(1 - ema, 0), 1) : 1;      w[n - n_lo] = w_min + (uint32)(fail * 65536.0 + 0.5)
 * and thr [n_hi - n_lo] from w as bridges_family_thresholds builds it.  1 <= w_min <= 2^20 - 2^16 keeps every class drawable
 * and every weight <= 2^20; 0 <= beta <= 1; min_episodes >= 1; 0 <= n_lo <= n_hi < n_classes <= 8.  One workgroup, fixed order,
 * no atomics, no allocation, no host wait. */
int bridges_family_curriculum(double* sums, int32_t n_classes, double* state, int32_t n_lo, int32_t n_hi, double beta, uint32_t w_min,
                              int32_t min_episodes, uint32_t* w /* [C] */, uint64_t* thr /* [C-1] */, void* stream);
/* Sampled records -> the state arrays of a replay env of E >= n_rec envs (envs >= n_rec repeat record 0): s' = s plus the
 * action block with the occupancy update of gym_env.py:228-232, its RAW candidate count
 * n_groups * (n_ground + free faces * n_off) (generate_actions, actions.py:7-52; bridges_env_refresh clamps it to the env's
 * a_max and flags / counts the truncation), the block ranges [e*K, e*K + n) of s' and of s (for bridges_bits_or over the
 * per-block rasters) and the scalars the targets need. */
int bridges_replay_unpack(int32_t E, int32_t n_rec, int32_t K, const double* rec, const int32_t* shape_faces, int32_t n_shapes,
                          int32_t n_groups, int32_t n_ground, int32_t n_off, int32_t* n_blocks, int32_t* blk_shape,
                          double* blk_pose, uint8_t* blk_occ, int32_t* n_cand, int32_t* ranges_next, int32_t* ranges_prev,
                          float* lin, float* stable_s, uint8_t* done, uint8_t* stable_n, void* stream);
/* bridges_replay_unpack for the state s a transition was taken IN (Munchausen targets: the log-policy of the taken action is
 * formed over the candidates of s): n_blocks = NB, the block list as the record stores it (no action block, no occupancy
 * update), the raw candidate count of the free faces of s, ranges_next and ranges_prev both [e*K, e*K + NB).  The argument
 * list, the scalar outputs and the refusals are bridges_replay_unpack's; one kernel body serves both. */
int bridges_replay_unpack_prev(int32_t E, int32_t n_rec, int32_t K, const double* rec, const int32_t* shape_faces, int32_t n_shapes,
                               int32_t n_groups, int32_t n_ground, int32_t n_off, int32_t* n_blocks, int32_t* blk_shape,
                               double* blk_pose, uint8_t* blk_occ, int32_t* n_cand, int32_t* ranges_next, int32_t* ranges_prev,
                               float* lin, float* stable_s, uint8_t* done, uint8_t* stable_n, void* stream);

/* --- K7: DQN ops (robotoddler/training/successor_dqn.py) --------------------- */
/* update_target_net (successor_dqn.py:280-288): target = policy*tau + target*one_minus_tau, the two products and the
 * sum rounded separately in float32 as torch evaluates it (one_minus_tau = (float)(1.0 - tau) from the host). */
int bridges_soft_update(float* target, const float* policy, int64_t n, float tau, float one_minus_tau, void* stream);
/* train_policy_net target construction (successor_dqn.py:197-213, 222, 230):
 * per transition i with rows [seg_lo[i], seg_hi[i]) of the target net's output (a prefix-sum array: seg, seg + 1;
 * transitions whose next states are the same state may share a range, bridges_valid_rows with rep):
 *   j* = argmax next_q (first maximum), q_target[i] = lin_reward[i] + gamma * (done ? 0 : next_q[j*]),
 *   sf_target[i,:] = action_raster[i,:] + gamma * (done ? 0 : next_sf[j*,:])   (sf_dim may be 0).
 * Precondition: a transition that is not done has at least one row (seg_lo[i] < seg_hi[i]); an empty segment belongs to a done
 * transition, whose next rows are never read.  An empty segment that is NOT done is the caller's error and is marked, not
 * followed: q_target[i] = lin_reward[i] + gamma * -inf, argmax_row[i] = 0x7fffffff, and its successor-feature part is taken as
 * zero (sf_target[i,:] = action_raster[i,:]) -- no row of next_sf is read for it.
 * sf_dim > 0 needs sf_dim and next_sf_row_stride to be multiples of 4 and next_sf, action_raster, sf_target 16-byte aligned (-1
 * otherwise).  This is bridges_td_target_select with select_q = next_q behind these stricter checks: one kernel serves both. */
int bridges_td_target(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* next_q, const float* next_sf,
                      int64_t next_sf_row_stride, const float* action_raster, const float* lin_reward,
                      const uint8_t* done, float gamma, int32_t sf_dim, float* q_target, float* sf_target,
                      int32_t* argmax_row, void* stream);
/* bridges_td_target with a discount PER TRANSITION, discount [n_trans] f32, in place of the scalar gamma (n-step returns: the
 * discount of transition i is gamma^h of its horizon):
 *   q_target[i] = lin_reward[i] + discount[i] * (done ? 0 : next_q[j*]),
 *   sf_target[i,:] = action_raster[i,:] + discount[i] * (done ? 0 : next_sf[j*,:]).
 * The first-maximum rule, the empty-segment and done rules, both segment forms, the strided next_sf and argmax_row are those of
 * bridges_td_target, and so are the alignment rules; a discount filled with gamma gives its outputs bit for bit (the same
 * kernel, bridges_td_target_select's with select_q = next_q). */
int bridges_td_target_rows(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* next_q, const float* next_sf,
                           int64_t next_sf_row_stride, const float* action_raster, const float* lin_reward,
                           const uint8_t* done, const float* discount, int32_t sf_dim, float* q_target, float* sf_target,
                           int32_t* argmax_row, void* stream);
/* Double Q-learning: the target with the next row SELECTED by one value vector and VALUED by another.  select_q [R] f32 holds a
 * value for the same rows as next_q (the policy net's q where next_q is the target net's):
 *   j* = the first maximum of select_q over [seg_lo[i], seg_hi[i]) (ties go to the lowest row; NaN-free inputs; a segment that is
 *        all -inf yields its first row),
 *   q_target[i] = lin_reward[i] + d_i * (done ? 0 : next_q[j*]),
 *   sf_target[i,:] = action_raster[i,:] + d_i * (done ? 0 : next_sf[j*,:]),   argmax_row[i] = j*,
 * d_i = discount[i] when discount is not NULL (the per-transition form of bridges_td_target_rows), else the scalar gamma.
 * next_sf is strided (next_sf_row_stride floats between rows); sf_dim may be 0, and need not be a multiple of 4 -- rows that are
 * not 16-byte aligned are handled element by element.  An empty segment is what bridges_td_target states: argmax_row[i] =
 * 0x7fffffff, q_target[i] = lin_reward[i] + d_i * (done ? 0 : -inf), sf_target[i,:] = action_raster[i,:], and nothing of next_q or
 * next_sf is read for it.  With select_q == next_q (the same pointer or equal values) every output equals bridges_td_target's
 * (discount NULL) and bridges_td_target_rows' (discount given) bit for bit: the three entry points launch one kernel.
 * Returns -1 and launches nothing for: n_trans < 0 or sf_dim < 0; with n_trans > 0 a NULL seg_lo, seg_hi, select_q, next_q,
 * lin_reward, done, q_target or argmax_row; sf_dim > 0 with a NULL next_sf, action_raster or sf_target or a negative row stride;
 * a float / int32 pointer that is not 4-byte aligned.  n_trans == 0 returns 0 and launches nothing. */
int bridges_td_target_select(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* select_q, const float* next_q,
                             const float* next_sf, int64_t next_sf_row_stride, const float* action_raster, const float* lin_reward,
                             const uint8_t* done, const float* discount, float gamma, int32_t sf_dim, float* q_target,
                             float* sf_target, int32_t* argmax_row, void* stream);

/* Expected-value targets under the Boltzmann policy (the softmax backup, Expected SARSA for the policy
 * bridges_boltzmann_select draws from): the expectation of next_q and of a feature row over every transition's next rows.
 * select_q, next_q [R] f32 hold a value per row (the same pointer is allowed: the plain, non-double target); feat f32 holds
 * dim floats per row, feat_row_stride floats apart; feat_row [R] i64 (may be NULL) names the row of feat that stands for row j.
 * The rule, for transition i with the rows lo = seg_lo[i] .. seg_hi[i] - 1 and T = (double)temperature, all in float64:
 *   - WEIGHTS: those of bridges_boltzmann_select on select_q, word for word -- a row is ELIGIBLE if its select_q is neither NaN
 *     nor -inf; m = the largest eligible value; w_j = exp(((double)select_q_j - m) / T) for an eligible row, 0 for any other; if
 *     m is +inf: 1 for the +inf rows, else 0.  Z = sum_j w_j, p_j = w_j / Z.
 *   - VALUE: value[i] = (float) sum_j p_j (double)next_q[j].
 *   - FEATURE MEAN: feat_mean[i, c] = (float) sum_j p_j (double)feat[r_j * feat_row_stride + c] for c < dim, r_j = feat_row ?
 *     feat_row[j] : j; the sum over j is taken in ascending row order in float64 (product and sum rounded separately), then
 *     rounded once.
 *   - ENTROPY (entropy may be NULL): entropy[i] = (float)(log Z - sum_j p_j x_j), x_j = ((double)select_q_j - m) / T (taken as 0
 *     on the +inf rows when m is +inf, so the entropy there is the log of their number).
 *   - ARG-MAX ROW: argmax_row[i] = the first maximum of select_q among the eligible rows (for finite inputs the row of
 *     bridges_td_target_select).
 *   - a row whose weight is exactly 0 contributes nothing and is not read in next_q or feat, whatever they hold there;
 *   - NOTHING ELIGIBLE (an empty segment, hi <= lo, or a segment without an eligible row): value[i] = -inf, feat_mean[i, :] = 0,
 *     entropy[i] = 0, argmax_row[i] = 0x7fffffff, and nothing of next_q or feat is read.
 * Both segment forms of bridges_td_target are taken (a prefix-sum array as seg, seg + 1; separate lo / hi arrays); transitions
 * may share or overlap ranges.  dim == 0: feat, feat_row and feat_mean may be NULL.  The caller keeps every r_j * feat_row_stride
 * + c inside feat.  No atomics, every output word is written exactly once, the order of every sum is fixed (value and entropy:
 * lane-strided partial sums combined by a fixed tree): the same inputs give the same bits on every call.
 * Returns -1 and launches nothing for: n_trans < 0 or dim < 0; a temperature that is not finite or not > 0; a negative
 * feat_row_stride; a float / int32 pointer that is not 4-byte aligned or a feat_row that is not 8-byte aligned; with n_trans > 0
 * a NULL seg_lo, seg_hi, select_q, next_q, value or argmax_row, or dim > 0 with a NULL feat or feat_mean.  n_trans == 0 returns 0
 * and launches nothing. */
int bridges_soft_expect(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* select_q, const float* next_q,
                        float temperature, const float* feat, int64_t feat_row_stride, const int64_t* feat_row, int32_t dim,
                        float* value, float* feat_mean, float* entropy, int32_t* argmax_row, void* stream);

/* bridges_soft_expect at the RELATIVE TEMPERATURE of every transition (the rule stands at bridges_boltzmann_select_rel): the
 * spread is that of the transition's rows of select_q -- under double Q-learning the policy net's values, the array that weighs
 * the rows, never next_q --, T_e goes to temp_out[i] as a double, and every other output is bridges_soft_expect's at T = T_e. */
int bridges_soft_expect_rel(int32_t n_trans, const int32_t* seg_lo, const int32_t* seg_hi, const float* select_q, const float* next_q,
                            float temperature, float spread_floor, const float* feat, int64_t feat_row_stride, const int64_t* feat_row,
                            int32_t dim, float* value, float* feat_mean, float* entropy, int32_t* argmax_row, double* temp_out,
                            void* stream);

/* MUNCHAUSEN TARGETS: the entropy-regularised (log-sum-exp) value of a segment of q and the scaled log-policy T ln pi(a) of one
 * of its rows, on top of the rule of bridges_boltzmann_select.  With pi = softmax(q / T) the Munchausen target is
 *   r + alpha * clip(T ln pi(a|s), clip_lo, 0) + gamma * (1 - done) * V_T(s'),   V_T(s) = T ln sum_j exp(q_j / T),
 * and T ln pi(a|s) = q(s, a) - V_T(s): this one operator serves both halves.  The rule, for segment i with the rows
 * lo = seg_lo[i] .. seg_hi[i] - 1 of q (f32) and T = (double)temperature, all in float64:
 *   - ELIGIBILITY, m and the WEIGHTS w_j are those of bridges_boltzmann_select, word for word; Z = sum_j w_j.
 *   - VALUE: value[i] = (float)(m + T * log Z); m = +inf: +inf.  NOTHING ELIGIBLE (an empty segment included): value[i] = -inf and
 *     nothing else of q is read.
 *   - TAKEN ROW (taken_row i32 [n] given, a = taken_row[i]): if a lies in [lo, hi) and is eligible,
 *       L = fmin(((double)q_a - m) - T * log Z, 0);  m = +inf: L = -(T * log Z) on a +inf row (Z is their number), -inf on any other;
 *       tlogp[i] = (float)L,  bonus[i] = (float)((double)alpha * fmax(L, (double)clip_lo)), a zero written as +0.0,  miss[i] = 0.
 *     If a lies outside the segment, is 0x7fffffff (bridges_action_row's no-match), is not eligible, or nothing is eligible:
 *       tlogp[i] = 0, bonus[i] = +0.0, miss[i] = 1.
 *     taken_row == NULL: tlogp, bonus and miss may be NULL and are not written.
 * Both segment forms of bridges_td_target are taken; segments may share or overlap rows.  Every sum has a fixed order
 * (lane-strided partial sums combined by a fixed tree), there are no atomics and every output word is written once: equal inputs
 * give equal bits.  One launch, no scratch.
 * Returns -1 and launches nothing for: what bridges_soft_expect refuses of the arguments they share (n < 0, a temperature that is
 * not finite or not > 0, a float / int32 pointer that is not 4-byte aligned, with n > 0 a NULL seg_lo, seg_hi, q or value); an
 * alpha that is not finite or outside [0, 1]; a clip_lo that is not finite or > 0; with taken_row given, a NULL tlogp, bonus or
 * miss.  n == 0 returns 0 and launches nothing. */
int bridges_soft_value(int32_t n, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, float temperature,
                       const int32_t* taken_row /* i32 [n] or NULL */, float alpha, float clip_lo, float* value, float* tlogp,
                       float* bonus, uint8_t* miss, void* stream);

/* bridges_soft_value at the RELATIVE TEMPERATURE of every segment (the rule stands at bridges_boltzmann_select_rel): the spread
 * is that of the segment's own rows of q, T_e goes to temp_out[i] as a double (nothing eligible: temperature * spread_floor), and
 * every other output is bridges_soft_value's at T = T_e.  Refused: whatever the sibling refuses; a spread_floor that is not
 * finite or not > 0; a temp_out that is not 8-byte aligned or, with n > 0, NULL. */
int bridges_soft_value_rel(int32_t n, const int32_t* seg_lo, const int32_t* seg_hi, const float* q, float temperature,
                           float spread_floor, const int32_t* taken_row, float alpha, float clip_lo, float* value, float* tlogp,
                           float* bonus, uint8_t* miss, double* temp_out /* f64 [n] */, void* stream);

/* The row of a rebuilt candidate set that holds the action a record took.  For transition i with the rows lo = seg_lo[i] ..
 * seg_hi[i] - 1 of idx (i64: compact candidate rows, bridges_valid_rows) and the record rec + i * rec_stride (doubles):
 *   row[i] = the first j in [lo, hi) whose candidate c = idx[j] has cand_desc[c] (i32 [C, 4]: target_block, target_face, shape,
 *   face) equal to the record's (ATB, ATF, ASHAPE, AFACE) and the four words of cand_pose[c] (f64 [C, 4]) equal to the record's
 *   APOSE words as 64-bit patterns -- no float comparison: -0.0 does not match 0.0, a NaN matches its own bits;
 *   0x7fffffff if there is none.
 * The descriptor alone is not unique (ground positions and offsets share it): the pose bits decide.  The caller keeps every
 * idx[j] inside cand_desc / cand_pose.  No atomics, each output written once.  Returns -1 and launches nothing for: n < 0,
 * rec_stride < BRIDGES_REC_WIDTH, a NULL array, an int32 pointer that is not 4-byte, an idx / cand_pose / rec that is not 8-byte
 * or a cand_desc that is not 16-byte aligned.  n == 0 returns 0 and launches nothing. */
int bridges_action_row(int32_t n, const int32_t* seg_lo, const int32_t* seg_hi, const int64_t* idx /* i64 [R] */,
                       const int32_t* cand_desc /* i32 [C,4] */, const double* cand_pose /* f64 [C,4] */, const double* rec,
                       int64_t rec_stride /* doubles */, int32_t* row /* i32 [n] */, void* stream);

/* --- n-step returns of the vectorised loop ------------------------------------------------------------------------
 * The fold of one lock-step's one-step records rec [E, W] f64 (W >= BRIDGES_REC_WIDTH: the record plus its task tail) / valid [E]
 * into h-step records.  Per-env window state that persists between calls: count [E] i32 (pending starts, 0 .. n - 1) and
 * acc, disc, stable_s, td [E, n] f64.  Per env with a valid transition, in this order:
 *   1. a pending start is appended: acc = 0, disc = 1, the record's STABLE_S and TD;
 *   2. every pending start j: acc_j += disc_j * rec[LIN], disc_j *= gamma (float64);
 *   3. rec[DONE] set: every pending start is emitted, oldest first, with horizon h_j = count - j, and the window is emptied;
 *      else count == n: the oldest start is emitted with h = n and the rest shifts down.
 * An env with valid = 0 keeps its window (it is empty then: the transition before a reset-only lock-step was done).
 * out [E * n, W + 1] f64, out_valid [E * n] u8: env e's emissions are rows e * n ..., oldest first, out_valid = 1; the other rows
 * of its block have out_valid = 0 and unspecified content.  An emitted row is rec[e] with LIN = acc_j (the h-step return),
 * STABLE_S and TD = the start's, and h_j in column W; block list, action, DONE, STABLE_N, REWARD and the tail stay the last
 * step's, so the start state is the first rec[NB] - (h - 1) blocks of the row's block list and the start action the block after.
 * n outside 1..BRIDGES_NSTEP_MAX, W < BRIDGES_REC_WIDTH, a NULL or misaligned pointer return -1 and launch nothing. */
#define BRIDGES_NSTEP_MAX 8
int bridges_nstep_fold(int32_t E, int32_t W, int32_t n, const double* rec, const uint8_t* valid, double gamma, int32_t* count,
                       double* acc, double* disc, double* stable_s, double* td, double* out, uint8_t* out_valid, void* stream);
/* Beam search: the transition records of one finished beam per group, traced back through the slots it occupied (it stands here
 * because its rows are the records above, in the h-step form of bridges_nstep_fold).  E = G * B envs, group g owns envs
 * gB .. gB + B - 1 as for bridges_beam_select.  The search keeps per depth t < D and env e: rec [D, E, BRIDGES_REC_WIDTH] f64, the
 * one-step record of the transition e made at depth t; valid [D, E] u8, whether it made one; parent [D, E] i32, the slot it was
 * forked from (the src of that depth's bridges_beam_select; row 0 is never read).  Per group the caller names the end of one
 * episode: end_env [G], end_depth [G] i32.
 *   - end_depth[g] < 0: nothing ended; the group emits no rows, status[g] = 0.
 *   - CHAIN: L = end_depth + 1, e_{L-1} = end_env[g], e_{t-1} = parent[t][e_t] for t = L-1 .. 1.
 *   - BROKEN CHAIN: end_depth >= D, or some e_t outside [gB, gB + B), or some valid[t][e_t] == 0: no rows, status[g] = 1.  No
 *     index outside the given arrays is ever read, whatever they hold.
 *   - ROWS: an intact chain (status[g] = 0) emits L rows, one per start t = 0 .. L-1, ascending.  h = min(n_step, L - t),
 *     last = t + h - 1.  The row is rec[last][e_last], all BRIDGES_REC_WIDTH columns copied as bits; then REC_STABLE_S is that of
 *     rec[t][e_t], REC_TD is `priority`, and for h > 1 REC_LIN is the return  acc = 0, disc = 1; for k = 0 .. h-1:
 *     acc += disc * lin_{t+k}; disc *= gamma  (binary64, in this order: steps 1-2 of bridges_nstep_fold; the same bits on every
 *     call); for h == 1 the column keeps the record's own bits.  The n_tail doubles of tail[end_env[g]] follow (tail [E, n_tail],
 *     or NULL with n_tail = 0; the envs of a group share one task), and with n_step > 1 h as a double in a last column:
 *     out [G * D, W_out], W_out = BRIDGES_REC_WIDTH + n_tail + (n_step > 1).
 *   - OFFSETS: offset [G + 1] i32, the exclusive prefix sum of the groups' row counts: group g's rows are out[offset[g] + t],
 *     offset[G] is the total; rows of out at or beyond the total are not written.
 * A child's block list extends its parent's, so the start state of a row is the first REC_NB - (h - 1) blocks of its block list,
 * as for the rows of bridges_nstep_fold.  Two launches, one workgroup per group, no scratch, no atomics; every output word is
 * written at most once; no output may alias an input.  1 <= B <= 16, 1 <= D <= BRIDGES_REC_K, 1 <= n_step <= BRIDGES_NSTEP_MAX.
 * Refused (-1, nothing launched): E < 0, B, D or n_step outside those, E % B != 0, n_tail < 0, a NULL array (tail excepted when
 * n_tail = 0), a misaligned pointer, a gamma that is not finite.  E == 0 returns 0 and launches nothing. */
int bridges_beam_trace(int32_t E, int32_t B, int32_t D, int32_t n_step, int32_t n_tail, const double* rec, const uint8_t* valid,
                       const int32_t* parent, const int32_t* end_env, const int32_t* end_depth, const double* tail, double gamma,
                       double priority, double* out, int32_t* offset, int32_t* status, void* stream);
/* The discounted sum of consecutive block rasters (the action part of an h-step successor-feature target): bits [n_rows, 64] u64,
 * per transition i a first row first[i] (i64) and a count h[i] (i32, 1..BRIDGES_NSTEP_MAX) ->
 *   sum [n, 64, 64] f32:  sum[i] = sum_{k < h[i]} d_k * image(bits[first[i] + k]),    disc [n] f32:  disc[i] = d_{h[i]},
 * d_0 = 1, d_{k+1} = d_k * gamma in float32 (both outputs from the same sequence), the terms added in ascending k; the
 * bit-to-pixel order is bridges_bits_to_f32's and h = 1 gives its image bit for bit.  sum may be NULL (disc only).
 * h is clamped to 0..BRIDGES_NSTEP_MAX and first[i] + k to the n_rows of the table: nothing outside bits is read. */
int bridges_bits_discounted_sum(int32_t n, const uint64_t* bits, int64_t n_rows, const int64_t* first, const int32_t* h, float gamma,
                                float* sum, float* disc, void* stream);

/* --- prioritised replay of the vectorised loop --------------------------------------------------------------------
 * The inverse-CDF draw over one column of the replay ring.  rec [n_rec, W] f64 holds the live rows (their order is irrelevant),
 * col the priority column (BRIDGES_REC_TD), u [n_draws] f64 uniforms in [0, 1):
 *   m_i = pow(fmin(fmax(rec[i, col], 0), 1e30) + 1e-5, alpha)     (alpha == 1: the sum itself, no pow; alpha == 0: m_i = 1),
 *   idx[j] = the first k with m_0 + .. + m_k > u[j] * (m_0 + .. + m_{n_rec-1}), clamped to n_rec - 1
 * -- torch.searchsorted(cumsum(m), u * sum(m), right=True).clamp(max = n_rec - 1).  A NaN or negative priority counts as 0 and
 * one above 1e30 as 1e30 (fmax / fmin return the operand that is not NaN), so the total is finite and positive whatever a
 * diverged step wrote.  The sums are float64 in a fixed order of the kernels' own (256-row chunks summed by a tree, the chunk
 * sums scanned serially, the masses inside a chunk scanned by a wave): against the exactly rounded prefix sums idx[j] may differ
 * where u[j] * total lies within ~n_rec * 2^-52 * total of a boundary, and nowhere else.  No floating-point atomics: the same
 * inputs give the same idx bit for bit on every call and every device.  Three launches (masses + chunk sums, scan, draws), no
 * host wait; rec is only read.  scratch: bridges_priority_sample_scratch(n_rec) doubles, caller-owned, overwritten.
 * u[j] outside [0, 1) or NaN is not an error: every idx[j] lies in [0, n_rec).
 * Returns -1 and launches nothing for: n_draws < 0; with n_draws > 0: n_rec <= 0 or n_rec > BRIDGES_PRIORITY_MAX_ROWS; col < 0 or
 * W <= col; alpha outside [0, 1] or NaN; a NULL rec, u, idx or scratch; a pointer that is not 8-byte aligned; scratch_doubles
 * below the sizing call's answer.  n_draws == 0 returns 0 and launches nothing. */
#define BRIDGES_PRIORITY_MAX_ROWS (1ll << 30)
#define BRIDGES_PRIORITY_MAX_UPDATES (1ll << 20)
int bridges_priority_sample_scratch(int64_t n_rec, int64_t* doubles);
int bridges_priority_sample(int64_t n_rec, int32_t W, int32_t col, const double* rec, double alpha, int64_t n_draws, const double* u,
                            int64_t* idx, double* scratch, int64_t scratch_doubles, void* stream);
/* The refresh of sampled rows: rec[idx[j], col] = (double)fabsf(q_sa[j] - q_target[j]) for j < n (idx i64, q_sa and q_target f32).
 * A row named by several j takes the value of the LAST of them (the highest j); every row is written by one thread, so equal
 * inputs give equal rings.  An idx[j] outside [0, n_rec) writes nothing; no column but col and no row that idx does not name is
 * written.  One launch; the work grows with n^2 / 2 (n = n_steps * batch_size, hundreds), n <= BRIDGES_PRIORITY_MAX_UPDATES.
 * Returns -1 and launches nothing for: n < 0 or n_rec < 0; col < 0 or W <= col; with n > 0 a NULL rec, idx, q_sa or q_target, an
 * rec / idx that is not 8-byte or a q_sa / q_target that is not 4-byte aligned.  n == 0 returns 0 and launches nothing. */
int bridges_priority_update(int64_t n_rec, int32_t W, int32_t col, double* rec, int64_t n, const int64_t* idx, const float* q_sa,
                            const float* q_target, void* stream);
/* The importance-sampling weights of the draws (Schaul et al.'s beta): idx [n_draws] i64 as bridges_priority_sample returned it,
 * scratch as THAT call left it for the same n_rec (its first ceil(n_rec / 256) * 256 doubles are the masses m_i; only read here),
 * weight [n_draws] f32.  w_j = (n_rec * m_idx[j] / total)^(-beta); every `batch` consecutive draws are one optimiser step and are
 * divided by their own maximum, so the largest weight of a batch is exactly 1 and n_rec and total cancel:
 *   weight[j] = (float)pow(min_k m_idx[k] / m_idx[j], beta),   k over the batch of j
 * in float64, rounded once (beta == 0: 1.0f, no pow; beta == 1: the quotient, no pow).  The masses are those the draws were made
 * from, not the record column: a bridges_priority_update in between does not change the weights, the next
 * bridges_priority_sample on the same scratch does.  An idx[j] outside [0, n_rec) gets weight 0 and takes no part in the minimum.
 * One launch, one workgroup per batch, no atomics: the same bits on every call.
 * Returns -1 and launches nothing for: n_draws < 0; with n_draws > 0: n_rec <= 0 or n_rec > BRIDGES_PRIORITY_MAX_ROWS; batch <= 0
 * or n_draws % batch != 0; beta outside [0, 1] or NaN; a NULL idx, scratch or weight; an idx / scratch that is not 8-byte or a
 * weight that is not 4-byte aligned; scratch_doubles below the sizing call's answer.  n_draws == 0 returns 0, launches nothing. */
int bridges_priority_weights(int64_t n_rec, int64_t n_draws, int64_t batch, const int64_t* idx, double beta, const double* scratch,
                             int64_t scratch_doubles, float* weight, void* stream);

/* --- hindsight goal relabelling of the vectorised loop on per-env tasks ("final" strategy) ---------------------------
 * Every episode that ended in this lock-step is written again, G times, under T targets its own final structure reached.
 * Inputs (device): buf [E, K, W] f64, the records of every env's running episode in step order (W >= BRIDGES_REC_WIDTH + 3 T: a
 * record and its task tail, the T targets first); flags [E, K, 8] u8, the step_flags of the step of each record; len [E] i32,
 * the records held (m); ended [E] u8, set where the record len - 1 has BRIDGES_REC_DONE; episode [E] u32, task_episode of the
 * buffered episode.  shapes_dev (bridges_shapes_upload), target_shape (cube06), grid_x / grid_y [img], img and gauss_k
 * [BRIDGES_GAUSS_TAPS] are the env's.  Per ended env e and slot g < G:
 *   eligible blocks: all m, but the last when its step was not frozen-stable (BRIDGES_REC_STABLE_N == 0): m'; m' == 0: no rows.
 *   choice: idx = 0 .. m' - 1; for i < min(T, m'): swap(idx[i], idx[j]), j = i + ((u * (m' - i)) >> 32), u = r >> 32,
 *     h0 = splitmix64(((seed & 0xFFFFFFFF) << 32 | (uint32)(env_id_base + e)) ^ 0x68696E645F726E67)      ("hind_rng")
 *     h1 = splitmix64(h0 ^ episode[e]);  h2 = splitmix64(h1 ^ g);  r = splitmix64(h2 ^ i)      -- integer arithmetic only
 *   target q = (cx, 0, cz), the centre of the axis-aligned bounding box of block idx[q mod m'], taken over the block's world
 *     vertices (rebuilt from the recorded shape id and pose as bridges_pose_block does) exactly as bridges_env_step's
 *     reached-test takes its box: cx = (x0 + x1) * 0.5.
 *   rows t = 0, 1, ..: record t with REWARD, LIN, DONE and the 3 T target values of the tail replaced by what bridges_env_step
 *     records under the new targets: its reached-test (the target after a reached one is skipped), its sparse reward,
 *     LIN = free-stable ? base : (frozen-stable ? base / 100 : 0) with base the rasteriser's float cand_lin of the block on the
 *     new targets' reward map (the arithmetic of the per-env task features), DONE = !frozen-stable | all targets reached |
 *     truncated | no_actions, the four flags read from flags[e, t].  The walk stops after the first t at which all targets are
 *     reached.  Every other column (TD, the obstacle values of the tail) is copied.
 * out [E * K * G, W] f64: the rows compacted to the front, env ascending, then g, then t; *count (device i32) their number; rows
 * beyond it are not written.  Three launches (count, scan, rows), no atomics, no host wait: the same bits on every call.
 * scratch: bridges_hindsight_relabel_scratch(E, G) bytes, caller-owned, overwritten.
 * Returns -1 and launches nothing for: E < 0; G outside 1..4; K outside 1..BRIDGES_MAX_BLOCKS; T outside 1..BRIDGES_MAX_TARGETS;
 * W < BRIDGES_REC_WIDTH + 3 T; a shape table of no or more than 8 shapes or a target_shape outside it; img outside 1..64; a NULL
 * or misaligned pointer; scratch_bytes below the sizing call's answer.  E == 0 returns 0 and launches nothing. */
int bridges_hindsight_relabel_scratch(int32_t E, int32_t G, int64_t* bytes);
int bridges_hindsight_relabel(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                              const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed, int32_t env_id_base,
                              const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape, const double* grid_x,
                              const double* grid_y, int32_t img, const float* gauss_k, double* out, int32_t* count, void* scratch,
                              int64_t scratch_bytes, void* stream);
/* The same relabelling for a loop on n-step returns: the h-step rows of the relabelled walk, in the form of bridges_nstep_fold.
 * Per ended env e and slot g the eligible blocks, the choice, the targets and the walk are bridges_hindsight_relabel's; let the
 * walk have the L one-step rows r_0 .. r_{L-1} (exactly the rows that entry writes for (e, g)).  The slot emits L rows, one per
 * start t = 0 .. L-1, ascending: h = min(n_step, L - t), last = t + h - 1, and the row is r_last with
 *   REC_LIN = the return  acc = 0, disc = 1; for k = 0 .. h-1: acc += disc * lin(r_{t+k}); disc *= gamma  (binary64, in this order,
 *     no fused multiply-add: steps 1-2 of bridges_nstep_fold on the RELABELLED lin),
 *   REC_STABLE_S and REC_TD = those of r_t, the start's,  and h as an exact double in one more column, W;
 * block list, action, REWARD, DONE, STABLE_N and the whole relabelled tail stay r_last's.  The end of the walk flushes every pending
 * start whether or not r_{L-1} has DONE: under hindsight targets a final step that is not terminal bootstraps like any other, and
 * its tail rows are h-step rows with h < n_step that bootstrap from s_L.  (This is where the rule differs from bridges_nstep_fold,
 * in which only DONE flushes.)  n_step = 1 gives bridges_hindsight_relabel's rows with a column of 1.0 appended, bit for bit: the
 * relabelled lin is a non-negative finite float, so 0 + 1 * lin keeps its bits.
 * out [E * K * G, W + 1] f64: env ascending, then g, then start t; *count the number of rows -- the number the one-step entry
 * reports for the same inputs; rows at or beyond it are not written.  Three launches (the count and the scan are the sibling's),
 * no atomics, no host wait: the same bits on every call.  scratch: bridges_hindsight_relabel_scratch(E, G) bytes, as there.
 * Returns -1 and launches nothing for: whatever bridges_hindsight_relabel refuses (W is the width of the input); n_step outside
 * 1..BRIDGES_NSTEP_MAX; a gamma that is not finite; an out that is not 8-byte aligned.  E == 0 returns 0 and launches nothing. */
int bridges_hindsight_relabel_nstep(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                                    const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed,
                                    int32_t env_id_base, const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape,
                                    const double* grid_x, const double* grid_y, int32_t img, const float* gauss_k, int32_t n_step,
                                    double gamma, double* out /* [E*K*G, W+1] */, int32_t* count, void* scratch,
                                    int64_t scratch_bytes, void* stream);
/* --- hindsight relabelling with per-step goals ("per_step" strategy: hindsight experience replay's "future") ---------
 * Every transition of an episode that ended in this lock-step is written again, G times, under T targets that the episode
 * achieves from that transition onward.  Inputs, shape table, grids and kernel taps are bridges_hindsight_relabel's, and so are
 * m, the eligible blocks m' and the reading of a record.  One work item is (ended env e, slot g < G, step t < m'); it emits at
 * most one row.  (With m' = m - 1 the collapsed last step m - 1 has no later block to be a goal: it emits nothing, the rollout's
 * own record carries the collapse.)
 *   draw: the "hind_rng" stream with one more key -- h2 as there (seed, env_id_base + e, episode[e], g);
 *     h3 = splitmix64(h2 ^ ((t + 1) << 8));  r_i = splitmix64(h3 ^ i);  u_i = r_i >> 32                 -- integer arithmetic only
 *   future block: f = t + ((u_0 * (m' - t)) >> 32), in [t, m' - 1].
 *   goals, from the structure as it stands after step f: n = f + 1, idx = 0 .. n - 1; swap(idx[0], idx[f]); for i = 1 ..
 *     min(T, n) - 1: swap(idx[i], idx[j]), j = i + ((u_i * (n - i)) >> 32).  Target q = (cx, 0, cz), the bounding-box centre of
 *     block idx[q mod n], the box taken as bridges_env_step's reached-test takes it.  Target 0 is always block f's own centre.
 *   existence: bridges_env_step's reached-test (the target after a reached one is skipped) of steps 0 .. t - 1 under these
 *     targets; if it leaves no target open the episode was over before step t, the transition does not exist, nothing is emitted.
 *   row (bridges_hindsight_per_step): record t with REWARD, LIN, DONE and the 3 T target values of the tail replaced by what
 *     bridges_env_step records at step t under these targets -- the expressions of bridges_hindsight_relabel's rows, the open
 *     targets being those the walk 0 .. t leaves.  Every other column is copied.
 *   h-step row (bridges_hindsight_per_step_nstep), in the form of bridges_hindsight_relabel_nstep: the walk under the goals of t
 *     runs from step t to the first step that leaves no target open, or else to step m - 1 (a collapsed last step included);
 *     h = min(n_step, walk_end - t + 1), last = t + h - 1; the row is record last relabelled under the goals of t, with
 *     REC_LIN = acc = 0, disc = 1; for k = 0 .. h-1: acc += disc * lin(step t + k); disc *= gamma (binary64, in this order, no
 *     fused multiply-add), REC_STABLE_S and REC_TD of record t, and h in one more column, W.  An open end flushes: a start
 *     whose walk ends before n_step steps is stored with its shorter h whether or not its last step has DONE.  n_step = 1 gives
 *     the one-step rows with a column of 1.0 appended, bit for bit.
 * out [E * K * G, W] (nstep: [E * K * G, W + 1]) f64: the rows compacted to the front, env ascending, then g, then t; *count
 * (device i32) their number; rows beyond it are not written.  Envs in mid-episode emit nothing; the inputs are only read.
 * Three launches (count with a step mask per (env, slot), scan, rows), no atomics, no host wait: the same bits on every call.
 * scratch: bridges_hindsight_per_step_scratch(E, G) bytes (a count and a mask per (env, slot)), caller-owned, overwritten.
 * Returns -1 and launches nothing for whatever the sibling entry of the "final" strategy refuses.  E == 0 returns 0. */
int bridges_hindsight_per_step_scratch(int32_t E, int32_t G, int64_t* bytes);
int bridges_hindsight_per_step(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                               const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed, int32_t env_id_base,
                               const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape, const double* grid_x,
                               const double* grid_y, int32_t img, const float* gauss_k, double* out, int32_t* count, void* scratch,
                               int64_t scratch_bytes, void* stream);
int bridges_hindsight_per_step_nstep(int32_t E, int32_t K, int32_t W, int32_t T, int32_t G, const double* buf, const uint8_t* flags,
                                     const int32_t* len, const uint8_t* ended, const uint32_t* episode, uint64_t seed,
                                     int32_t env_id_base, const bridges_shape* shapes_dev, int32_t n_shapes, int32_t target_shape,
                                     const double* grid_x, const double* grid_y, int32_t img, const float* gauss_k, int32_t n_step,
                                     double gamma, double* out /* [E*K*G, W+1] */, int32_t* count, void* scratch,
                                     int64_t scratch_bytes, void* stream);

/* Inference epilogues of the conv Q-networks (robotoddler/models/cv.py:5-17, 41-73, 108-170: Conv2d -> ReLU
 * [-> MaxPool2d(2)]), one pass instead of torch's three; bit-identical to relu(conv + bias) / maxpool(relu(conv + bias)).
 * x [n, C, hw] f32 contiguous NCHW output of a bias-free convolution, updated in place (hw % 4 == 0). */
int bridges_bias_relu(float* x, const float* bias, int64_t n, int32_t C, int32_t hw, void* stream);
/* x [n, C, H, W] -> out [n, C, H/2, W/2] (W % 4 == 0, H % 2 == 0). */
int bridges_bias_relu_pool2(const float* x, const float* bias, float* out, int64_t n, int32_t C, int32_t H, int32_t W,
                            void* stream);

/* ---- one optimiser step of SuccessorMLP at replay-batch size (robotoddler/models/cv.py:76-105;
 * train_policy_net, robotoddler/training/successor_dqn.py:157-235: forward, MSE losses, backward) on the f32 matrix
 * cores.  All tensors f32, row-major, contiguous; `rows` = the batch padded to a multiple of 32 (padding rows zero).
 * `ws` = scratch for split partial sums (ws_floats floats; the split count adapts to it). */
/* y [rows,N] = act(x [rows,K] . W [N,K]^T + bias), act = ReLU if relu else identity (nn.Linear [+ nn.ReLU], cv.py:20-38). */
int bridges_linear_forward(int32_t rows, int32_t K, int32_t N, const float* x, const float* W, const float* bias,
                           int32_t relu, float* y, float* ws, int64_t ws_floats, const int64_t* x_block, void* stream);
/* Backward of the same layer from dz [rows,N] (gradient at its pre-activation) and its input a_in [rows,K]:
 * dW [N,K] = dz^T . a_in, db [N] = column sums of dz, and -- unless dz_below is NULL (first layer) --
 * dz_below [rows,K] = (dz . W) masked by act_below > 0 (act_below = the ReLU output that was this layer's input; NULL =
 * no mask). */
int bridges_linear_backward(int32_t rows, int32_t K, int32_t N, const float* dz, const float* a_in, const float* W,
                            float* dW, float* db, const float* act_below, float* dz_below, float* ws, int64_t ws_floats,
                            const int64_t* a_block, int32_t a_block_bias, void* stream);
/* The middle Linear + ReLU layers of the step in ONE launch each way and without traffic between workgroups: a 1024-thread
 * workgroup per 32-column tile of the stack's last layer (backward: of the gradient handed below the stack) computes the
 * layers that tile depends on itself, in full, handing activations / gradients from layer to layer through LDS; every weight
 * fragment is requested before the first MFMA.  Built for the reference's stack (successor_dqn.py:366): n_layers = 4,
 * dims = {256, 128, 64, 128, 256} (layer l: dims[l] -> dims[l + 1]), one 32-row batch tile; bridges_mlp_mid_supported says
 * whether a shape is (1 / 0), anything else is refused by the two calls.
 *   forward:  acts[l + 1] = relu(acts[l] . W[l]^T + bias[l])                      (acts: 5 arrays [32, dims[l]])
 *   backward: dW[l] = dz[l + 1]^T . acts[l], db[l] = column sums of dz[l + 1], dz[0] = the gradient handed below the stack
 *             (dz: 5 pointers like acts; dz[4] given, dz[0] written, dz[1..3] live in LDS only and are not touched)
 * dims and the pointer tables are HOST arrays.  Bit-identical to four calls of bridges_linear_forward / _backward.
 * The backward launch can carry an Adam update of ANOTHER layer's flat range (rest_*, as bridges_linear_backward_adam's; rest_n
 * = 0: none): the head's, whose gradient is complete and whose weights nothing reads any more -- extra workgroups beside the
 * stack's eight, so that traffic is out of the step's last launch. */
int bridges_mlp_mid_supported(int32_t rows, int32_t n_layers, const int32_t* dims);
int bridges_mlp_mid_forward(int32_t rows, int32_t n_layers, const int32_t* dims, const float* const* W, const float* const* bias,
                            float* const* acts, void* stream);
int bridges_mlp_mid_backward(int32_t rows, int32_t n_layers, const int32_t* dims, const float* const* W, float* const* dW,
                             float* const* db, float* const* acts, float* const* dz, float* rest_param, const float* rest_grad,
                             float* rest_exp_avg, float* rest_exp_avg_sq, int64_t rest_n, const float* step, double lr, double beta1,
                             double beta2, double eps, void* stream);
/* The same stack for MANY rows -- the acting / target forward between the first layer and the head (cv.py:20-38 inside
 * SuccessorMLP.forward): y [n, 256] = the four Linear + ReLU layers applied to relu(x), x [n, 256] the pre-activation of the
 * layer in front (row strides in floats); mid = scratch of n x 64 floats (the narrow activation between the two launches).
 * Two launches of two layers each instead of four library GEMMs; the arithmetic of the training step's forward, tile by tile.
 * dims / W / bias as for bridges_mlp_mid_forward. */
int bridges_mlp_mid_rows(int32_t n_rows, int32_t n_layers, const int32_t* dims, const float* const* W, const float* const* bias,
                         const float* x, int64_t x_stride, float* y, int64_t y_stride, float* mid, void* stream);
/* bridges_linear_backward of the LAST layer with the step's book-keeping riding along (one thread of the launch, beside its
 * jobs): losses[*counter] = sum of loss_rows[0 .. batch) in row order, ++*counter, ++*adam_step (adam_step may be NULL).  The
 * loss rows are those bridges_successor_loss (called with ticket = NULL, losses = NULL) has just written; nothing between the
 * two calls may read *counter.  No x_block / a_block indirection (the head's input is the stack's output). */
int bridges_linear_backward_log(int32_t rows, int32_t K, int32_t N, const float* dz, const float* a_in, const float* W,
                                float* dW, float* db, const float* act_below, float* dz_below, float* ws, int64_t ws_floats,
                                const float* loss_rows, int32_t batch, float* losses, int32_t n_losses, int64_t* counter,
                                float* adam_step, void* stream);
/* Backward of a Linear layer that needs no input gradient (the first layer) with the optimiser update inside: W, bias and
 * their moments are updated in place from the weight-gradient tiles in the matrix-core accumulators (that gradient is never
 * written; rows must be 32: one batch tile), and extra workgroups of the same launch apply Adam to `rest_n` further
 * parameters (the other layers: one contiguous, 16-byte-aligned range of flat parameter / gradient / moment buffers, rest_n
 * a multiple of 4; 0 = none) -- valid because this is the last backward launch of a step.  *step as in bridges_adam_step. */
int bridges_linear_backward_adam(int32_t rows, int32_t K, int32_t N, const float* dz, const float* a_in, float* W, float* bias,
                                 float* exp_avg_w, float* exp_avg_sq_w, float* exp_avg_b, float* exp_avg_sq_b, float* rest_param,
                                 const float* rest_grad, float* rest_exp_avg, float* rest_exp_avg_sq, int64_t rest_n, const float* step,
                                 double lr, double beta1, double beta2, double eps, const int64_t* a_block, int32_t a_block_bias,
                                 void* stream);
/* Input rows of replay batch *counter: x [rows, 4 px + nf] = [block | action | reward | obstacle | binary]
 * (cv.py:100-103) from block_all / action_all [n,px], binary_all [n,nf] (row *counter * batch + b), reward / obstacle [px]. */
int bridges_mlp_input(int32_t batch, int32_t rows, int32_t px, int32_t nf, const int64_t* counter, const float* block_all,
                      const float* action_all, const float* binary_all, const float* reward, const float* obstacle,
                      float* x, void* stream);
/* The same rows for ALL n_batches batches of a train_policy_net call in one launch: x_all [n_batches * rows, 4 px + nf], batch c in
 * rows [c * rows, (c + 1) * rows).  bridges_linear_forward / _backward / _backward_adam take a device word `x_block` /
 * `a_block` (may be NULL = 0) that selects the block of such an array (x + *x_block * rows * K; the backward entry points add the
 * host constant a_block_bias to the word: -1 when the step's loss kernel has advanced the counter in between), so a replayed
 * graph of one optimiser step reads batch *counter of the pre-built inputs instead of building its rows first. */
int bridges_mlp_input_batches(int32_t n_batches, int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* block_all,
                              const float* action_all, const float* binary_all, const float* reward, const float* obstacle,
                              float* x_all, void* stream);
/* Both with a reward map PER TRANSITION (replay of per-env tasks): reward_stride = 0 is the one map [px] of the entry points
 * above (which forward here), reward_stride = px makes reward [n, px] and transition row *counter * batch + b read its own row;
 * any other stride is refused.  The obstacle map stays shared. */
int bridges_mlp_input_rows(int32_t batch, int32_t rows, int32_t px, int32_t nf, const int64_t* counter, const float* block_all,
                           const float* action_all, const float* binary_all, const float* reward, int64_t reward_stride,
                           const float* obstacle, float* x, void* stream);
int bridges_mlp_input_batches_rows(int32_t n_batches, int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* block_all,
                                   const float* action_all, const float* binary_all, const float* reward, int64_t reward_stride,
                                   const float* obstacle, float* x_all, void* stream);
/* The _rows forms with an obstacle raster PER TRANSITION as well (replay of per-env obstacles), read BIT-PACKED: obstacle_bits
 * [n, 64] u64, one raster per transition of the per-call arrays in the layout of bridges_bits_to_f32 / bridges_bits_linear --
 * column 3 px + p of transition row src = bit p & 63 of word src * 64 + (p >> 6): 512 B per transition instead of a 16 KiB f32
 * image.  px must be 4096 (64 x 64), anything else returns -1; reward / reward_stride as in the _rows forms. */
int bridges_mlp_input_task_rows(int32_t batch, int32_t rows, int32_t px, int32_t nf, const int64_t* counter, const float* block_all,
                                const float* action_all, const float* binary_all, const float* reward, int64_t reward_stride,
                                const uint64_t* obstacle_bits, float* x, void* stream);
int bridges_mlp_input_batches_task_rows(int32_t n_batches, int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* block_all,
                                        const float* action_all, const float* binary_all, const float* reward, int64_t reward_stride,
                                        const uint64_t* obstacle_bits, float* x_all, void* stream);
/* Head + loss + its gradient (cv.py:104-108; successor_dqn.py:215-232): y [rows, 2 px + 2 nf] = (psi0 | psi1 | binary),
 * q = sum_j softmax(psi)[1][j] * reward[j], loss = [use_q] mean (q - q_target)^2 + [use_sf] mean (psi0 - sf_target)^2
 * with the targets of batch *counter (q_target_all [n], sf_target_all [n,px]).  Writes dy [rows, 2 px + 2 nf],
 * loss_rows [rows] (per-row share of the loss), q_out [rows]; if losses != NULL: losses[*counter_inc] = sum of
 * loss_rows and ++*counter_inc (the step counter that selects the next batch). */
int bridges_successor_loss(int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* y, const float* reward,
                           const int64_t* counter, const float* q_target_all, const float* sf_target_all, int32_t use_q,
                           int32_t use_sf, float* dy, float* loss_rows, float* q_out, float* losses, int32_t n_losses,
                           int64_t* counter_inc, int32_t* ticket, float* adam_step, void* stream);
/* The same with reward_stride as in bridges_mlp_input_rows: q of transition row src is weighed with reward[src * reward_stride + j]. */
int bridges_successor_loss_rows(int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* y, const float* reward,
                                int64_t reward_stride, const int64_t* counter, const float* q_target_all, const float* sf_target_all,
                                int32_t use_q, int32_t use_sf, float* dy, float* loss_rows, float* q_out, float* losses,
                                int32_t n_losses, int64_t* counter_inc, int32_t* ticket, float* adam_step, void* stream);
/* The _rows form with an importance-sampling weight per transition: weight_all [n] f32 (bridges_priority_weights), addressed as the
 * targets are (row *counter * batch + b).  loss = [use_q] mean_b w_b (q - q_target)^2 + [use_sf] mean_b w_b mean_j (psi0 - sf_target)^2:
 * loss_rows[b] is w_b times the row's unweighted share, the two gradient coefficients of row b (2 (q - q_target) / batch and
 * 2 / (batch px)) are each multiplied by w_b once before they meet the per-pixel factors, q_out stays the unweighted q, rows
 * b >= batch stay zero.  With every w_b == 1.0f the outputs are the bits of bridges_successor_loss / _rows.  reward_stride 0 or px
 * as there; ticket, losses, counter_inc and adam_step as there (the logged loss is the in-order f32 sum of the weighted rows,
 * also through bridges_linear_backward_log).  A NULL weight_all returns -1. */
int bridges_successor_loss_weighted(int32_t batch, int32_t rows, int32_t px, int32_t nf, const float* y, const float* reward,
                                    int64_t reward_stride, const int64_t* counter, const float* q_target_all,
                                    const float* sf_target_all, int32_t use_q, int32_t use_sf, float* dy, float* loss_rows,
                                    float* q_out, float* losses, int32_t n_losses, int64_t* counter_inc, int32_t* ticket,
                                    float* adam_step, const float* weight_all, void* stream);
/* `ticket` (device int32, zero before the first call; may be NULL): the logging (losses[*counter_inc] = sum of loss_rows,
 * ++*counter_inc, and ++*adam_step if given) is done inside the loss kernel by the row workgroup that arrives last
 * instead of a second launch; the kernel re-arms the ticket.
 * One Adam step of torch.optim.Adam (successor_dqn.py:640; amsgrad / weight decay / maximize off) over a flat float32
 * buffer of n parameters with their gradients and moments; *step (device float) is the step number of THIS update,
 * already incremented by the caller. */
int bridges_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* step,
                      double lr, double beta1, double beta2, double eps, void* stream);
/* The same update over many tensors in ONE launch (a conv Q-network's 34-60 parameter tensors with their autograd gradients):
 * slots [n_slots] (device) name the tensors; chunk c of the launch updates elements [chunk_off[c] * 1024, + 1024) of tensor
 * chunk_slot[c] (device int32 arrays, n_chunks entries: every tensor cut into 1024-element chunks).  *step (device float) =
 * the number of updates done SO FAR: this update is number *step + 1; the launch does not write *step (advance it after the
 * call), it writes the new count into every slot's own `step` word when that is not NULL (torch.optim.Adam's state['step']). */
typedef struct bridges_adam_slot {
    float* p; const float* g; float* m; float* v; float* step; int64_t n;
} bridges_adam_slot;
int bridges_adam_multi(const bridges_adam_slot* slots, int32_t n_slots, const int32_t* chunk_slot, const int32_t* chunk_off,
                       int32_t n_chunks, const float* step, double lr, double beta1, double beta2, double eps, void* stream);

/* relu(conv3x3(x, w, padding 1) + bias) [then MaxPool2d(2)] for the 64-pixel-wide layers with 16 output channels of
 * the conv Q-networks (cv.py:5-17 ConvBlock(4,16) / (16,16); cv.py:138-254 UNet e11, e12, d41, d42), inference passes:
 * x [n, c_in, H, 64] f32 NCHW contiguous, w [16, c_in, 3, 3], bias [16] -> out [n, 16, H, 64] (pool: [n, 16, H/2, 32]).
 * c_in in {1..4, 16, 32}, H % 8 == 0.  Same function as torch's conv2d + relu (+ max_pool2d) up to f32 summation order. */
int bridges_conv3x3_relu_o16(const float* x, const float* w, const float* bias, float* out, int64_t n, int32_t c_in,
                             int32_t H, int32_t W, int32_t pool, void* stream);
/* The same kernel with the U-Net's neighbours folded in (cv.py:184-197):
 *   x2 != NULL: the 32 input channels are torch.cat([x, x2], dim=1) of two 16-channel tensors (decoder: up-convolution
 *               output + skip tensor), never materialised;
 *   mode 0 plain, 1 pooled, 2 both (out = relu(conv) [n,16,H,64] AND out2 = its MaxPool2d(2) [n,16,H/2,32]: the encoder's
 *        skip tensor and next level), 3 projection (out [n,1,H,64] = sum_c proj_w[c] * relu(conv)_c + proj_b[0]: the
 *        1x1 outconv to one channel behind the last decoder convolution). */
int bridges_conv3x3_relu_o16_ex(const float* x, const float* x2, const float* w, const float* bias, float* out, float* out2,
                                const float* proj_w, const float* proj_b, int64_t n, int32_t c_in, int32_t c_in2, int32_t H,
                                int32_t W, int32_t mode, void* stream);
/* ConvTranspose2d(kernel_size=2, stride=2) + bias of the U-Net decoder (cv.py:176, 179 upconv3 / upconv4), inference:
 * x [n, c_in, H, W] f32 NCHW (W % 16 == 0), w [c_in, c_out, 2, 2], bias [c_out] -> out [n, c_out, 2H, 2W];
 * (c_in, c_out) = (32, 16) or (64, 32). */
int bridges_upconv2x2(const float* x, const float* w, const float* bias, float* out, int64_t n, int32_t c_in, int32_t c_out,
                      int32_t H, int32_t W, void* stream);

/* --- K11: the ConvBlock stacks (robotoddler/models/cv.py:5-17, 41-73) in the TRAINING passes of train_policy_net
 * (successor_dqn.py:157-277), on the f32 matrix cores.  Square W x W float32 NCHW images, W in {8, 16, 32, 64}; C_out a multiple
 * of 16.
 * bridges_conv3x3: out [n, c_out, W, W] = conv3x3(x [n, c_in, W, W], padding 1) with
 *   mode 0: nothing else;  1: + bias, ReLU;  2: x [mask > 0] (mask [n, c_out, W, W]: the ReLU of the layer whose output the
 *   gradient flows into);
 *   transposed 0: w = Conv2d.weight [c_out, c_in, 3, 3];  1: the INPUT GRADIENT of a layer with weight w [c_in, c_out, 3, 3]
 *   (x = the gradient at that layer's output with c_in channels, out = the gradient at its input with c_out channels);
 *   in_mask (may be NULL; shape of x): x counts only where in_mask > 0 -- x = the gradient at a ReLU's output, in_mask = that
 *   ReLU's activation (likewise g_mask of bridges_conv3x3_wgrad).
 * bridges_conv3x3_wgrad: dw [c_out, c_in, 3, 3] and db [c_out] from g [n, c_out, W, W] (gradient at the layer's output, ReLU
 *   mask applied) and the layer's input x [n, c_in, W, W]; partial sums over pixel ranges are added in a fixed order
 *   (deterministic); scratch: bridges_conv3x3_wgrad_scratch floats.
 * Image tensors (x, in_mask, mask, out, g, g_mask) must be 16-byte aligned: rows are read and written as float4.
 * bridges_maxpool2 / bridges_maxpool2_relu_backward: MaxPool2d(2) of a [nc, H, W] and, from dy [nc, H/2, W/2], the gradient at
 *   the pre-pool activation a = relu(.): the first maximum of a window in scan order takes dy (as torch), times [a > 0]. */
int bridges_conv3x3(const float* x, const float* in_mask, const float* w, const float* bias, const float* mask, float* out, int64_t n,
                    int32_t c_in, int32_t c_out, int32_t W, int32_t mode, int32_t transposed, void* stream);
/* bridges_conv3x3_wgrad with dw == db == NULL leaves the partial sums in scratch ([splits][c_out * c_in * 9] then
 * [splits][c_out], splits = scratch floats / (c_out * c_in * 9 + c_out)); bridges_reduce_jobs then adds the partial sums of
 * SEVERAL layers in one launch: job j = workgroups [block_start, block_start + B_j) of total_blocks with B_j = ceil((n_w + n_b) /
 * 256) when splits <= 16 and ceil((n_w + n_b) / 16) otherwise; same arithmetic and order as the single-layer form (jobs_dev:
 * device array, ascending block_start). */
typedef struct bridges_reduce_job {
    const float* part; const float* part_b; float* dw; float* db; int32_t n_w; int32_t n_b; int32_t splits; int32_t block_start;
} bridges_reduce_job;
int bridges_reduce_jobs(const bridges_reduce_job* jobs_dev, int32_t n_jobs, int32_t total_blocks, void* stream);
int bridges_conv3x3_wgrad_scratch(int64_t n, int32_t c_in, int32_t c_out, int32_t W, int64_t* floats);
int bridges_conv3x3_wgrad(const float* g, const float* g_mask, const float* x, float* dw, float* db, float* scratch, int64_t scratch_floats,
                          int64_t n, int32_t c_in, int32_t c_out, int32_t W, void* stream);
int bridges_maxpool2(const float* a, float* y, int64_t nc, int32_t H, int32_t W, void* stream);
/* Backward of the U-Net decoder's ConvTranspose2d(kernel_size=2, stride=2) (cv.py:176, 179; forward: bridges_upconv2x2): from
 * the layer's input x [n, c_in, H, W], the gradient g [n, c_out, 2H, 2W] at its output and w [c_in, c_out, 2, 2] ->
 * dx [n, c_in, H, W] (may be NULL), dw [c_in, c_out, 2, 2], db [c_out]; (c_in, c_out) = (32, 16) or (64, 32), H * W a multiple
 * of 64; partial sums per workgroup added in a fixed order (deterministic).  scratch: bridges_upconv2x2_backward_scratch floats.
 * bridges_conv1x1_o1_*: Conv2d(c_in, 1, kernel_size=1) (cv.py:182 outconv of UNet(1)): y [n, hw] = b + sum_c x[n, c, hw] w[c];
 * backward: dx = g w[c], dw [c_in], db [1]; c_in <= 32, hw a multiple of 4; scratch: min(256, ceil(n * hw / 1024)) * (c_in + 1).
 * Both backward entry points leave the partial sums in scratch ([splits][n_w] then [splits][n_b]) when dw == db == NULL, for
 * bridges_reduce_jobs. */
int bridges_upconv2x2_backward_scratch(int64_t n, int32_t c_in, int32_t c_out, int32_t H, int32_t W, int64_t* floats);
int bridges_upconv2x2_backward(const float* x, const float* g, const float* w, float* dx, float* dw, float* db, float* scratch,
                               int64_t scratch_floats, int64_t n, int32_t c_in, int32_t c_out, int32_t H, int32_t W, void* stream);
int bridges_conv1x1_o1_forward(const float* x, const float* w, const float* bias, float* y, int64_t n, int32_t c_in, int32_t hw, void* stream);
int bridges_conv1x1_o1_backward(const float* x, const float* g, const float* w, float* dx, float* dw, float* db, float* scratch,
                                int64_t scratch_floats, int64_t n, int32_t c_in, int32_t hw, void* stream);
/* db [C] = sum over n and the hw pixels of g [n, C, hw] in a fixed order (deterministic, single-workgroup stages): the bias
 * gradient of a convolution whose weights stay with the library.  scratch: min(n, 32) * C floats. */
int bridges_bias_grad(const float* g, float* db, float* scratch, int64_t scratch_floats, int64_t n, int32_t C, int32_t hw, void* stream);
int bridges_maxpool2_relu_backward(const float* a, const float* dy, float* g, int64_t nc, int32_t H, int32_t W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BRIDGES_HIP_H */
