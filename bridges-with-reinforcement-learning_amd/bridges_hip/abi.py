"""ctypes mirror of include/bridges_hip.h and loader of libbridges_hip.so.

The library is the product: if it is missing or no HIP device is present the
entry points raise ``BridgesHipError`` -- there is no CPU fallback.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libbridges_hip.so")
CSRC_DIR = os.path.join(os.path.dirname(HERE), "csrc")
INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(HERE)), "include")
STAMP_PREFIX = "BRIDGES_SRC_HASH="


def source_hash():
    """sha256 over the library's sources: every file of csrc/ and include/ (relative name + contents, sorted by name).
    __graft_entry__.build() compiles it into the library (bridges_source_hash()); lib() compares."""
    import hashlib
    h = hashlib.sha256()
    for tag, d in (("csrc", CSRC_DIR), ("include", INCLUDE_DIR)):
        for name in sorted(os.listdir(d)):
            path = os.path.join(d, name)
            if os.path.isfile(path) and not name.startswith("."):
                h.update(f"{tag}/{name}\0".encode())
                with open(path, "rb") as fh:
                    h.update(fh.read())
                h.update(b"\0")
    return h.hexdigest()


def library_stamp(path=None):
    """The stamp inside a built library file, read from its bytes without loading it (None: no such file / no stamp)."""
    import re
    path = path or LIB_PATH
    if not os.path.exists(path):
        return None
    with open(path, "rb") as fh:
        m = re.search(rb"BRIDGES_SRC_HASH=([0-9a-f]{64}|unstamped)", fh.read())
    return m.group(1).decode() if m else None

MAX_VERTS = 6
MAX_BLOCKS = 16
MAX_GROUPS = 24
MAX_TARGETS = 8
MAX_INTERFACES = 64


def lp_ws_stride(max_blocks):
    """Doubles of simplex workspace per assembly of the stand-alone stability operator (bridges_stability) and per
    slot of the candidate-stability scratch: interface list + the largest tableau, (3K equilibrium rows + budget +
    cost) x (4*MAX_IF generators + slack + rhs, padded to an odd stride)."""
    return 9 * MAX_INTERFACES + (3 * max_blocks + 2) * (4 * MAX_INTERFACES + 3)


# include/bridges_hip.h: BRIDGES_LP_WS_DOUBLES -- the per-env persistent tableau of the incremental simplex
ENV_LP_WS_DOUBLES = 64 + 2 * (3 * MAX_BLOCKS + 2) * (4 * MAX_INTERFACES + 2 + 3 * MAX_BLOCKS + 1)
CAND_WS_SLOTS = 1024


IMG = 64

FLAG_NAMES = ("valid_step", "stable_frozen", "stable_unfrozen", "terminated", "truncated", "done",
              "no_actions", "lp_error")
STAT_NAMES = ("sum_cand", "sum_blocks", "env_steps", "reset_only", "lp_errors", "if_overflow", "locksteps",
              "sum_valid", "warm_resolved", "cand_overflow")


class BridgesHipError(RuntimeError):
    pass


class Shape(C.Structure):
    _fields_ = [
        ("nv", C.c_int32), ("pad_", C.c_int32),
        ("vx", C.c_double * MAX_VERTS), ("vz", C.c_double * MAX_VERTS),
        ("fa", C.c_int32 * MAX_VERTS), ("fb", C.c_int32 * MAX_VERTS),
        ("fcx", C.c_double * MAX_VERTS), ("fcz", C.c_double * MAX_VERTS),
        ("fnx", C.c_double * MAX_VERTS), ("fnz", C.c_double * MAX_VERTS),
        ("depth", C.c_double), ("volume", C.c_double), ("gx", C.c_double), ("gz", C.c_double),
    ]


class Task(C.Structure):
    _fields_ = [
        ("n_envs", C.c_int32), ("max_blocks", C.c_int32), ("max_steps", C.c_int32), ("a_max", C.c_int32),
        ("n_shapes", C.c_int32), ("n_groups", C.c_int32),
        ("group_shape", C.c_int32 * MAX_GROUPS), ("group_face", C.c_int32 * MAX_GROUPS),
        ("n_ground", C.c_int32), ("n_offsets", C.c_int32), ("n_targets", C.c_int32), ("debug", C.c_int32),
        ("env_id_base", C.c_int32), ("img_size", C.c_int32),
        ("mu", C.c_double), ("density", C.c_double),
        ("floor_half_width", C.c_double), ("floor_depth", C.c_double),
        ("xlim", C.c_double * 2), ("ylim", C.c_double * 2),
        ("targets", (C.c_double * 3) * MAX_TARGETS),
        ("seed", C.c_uint64),
        ("shapes", C.POINTER(Shape)),
        ("x_ground", C.POINTER(C.c_double)), ("offsets", C.POINTER(C.c_double)),
        ("grid_x", C.POINTER(C.c_double)), ("grid_y", C.POINTER(C.c_double)),
    ]


# (field name, torch dtype name, shape expression in E, K, C) -- order == bridges_env_buffers
ENV_BUFFER_FIELDS = [
    ("n_blocks", "int32", "E"),
    ("blk_shape", "int32", "E,K"),
    ("blk_pose", "float64", "E,K,4"),
    ("blk_verts", "float64", "E,K,6,2"),
    ("blk_occ", "uint8", "E,K"),
    ("targets_left", "int32", "E"),          # uint32 on the device
    ("state_bits", "int64", "E,64"),         # uint64 on the device
    ("n_if", "int32", "E"),
    ("if_body", "int32", "E,IF,2"),
    ("if_geom", "float64", "E,IF,8"),
    ("draw_counter", "int64", "E"),
    ("needs_reset", "uint8", "E"),
    ("sel_index", "int32", "E"),
    ("step_flags", "uint8", "E,8"),
    ("reward", "float32", "E"),
    ("lin_reward", "float32", "E"),
    ("n_reached", "int32", "E"),
    ("n_cand", "int32", "E"),
    ("n_valid", "int32", "E"),
    ("cand_offset", "int32", "E1"),
    ("cand_env", "int32", "C"),
    ("cand_desc", "int32", "C,4"),
    ("cand_ox", "float64", "C"),
    ("cand_pose", "float64", "C,4"),
    ("cand_verts", "float64", "C,6,2"),
    ("cand_frames", "float64", "C,6,4"),
    ("cand_rows", "int32", "C,2"),
    ("cand_inb", "uint8", "C"),
    ("cand_mask", "uint8", "C"),
    ("cand_lin", "float32", "C"),
    ("cand_bits", "int64", "C,64"),
    ("cand_raster", "float32", "C,64,64"),
    ("state_raster", "float32", "E,64,64"),
    ("cand_raster_nz", "int32", "C"),
    ("state_raster_nz", "int32", "E"),
    ("obstacle_bits", "int64", "64"),
    ("reward_map", "float32", "64,64"),
    ("reward_prefix", "float64", "64,65"),
    ("lp_ws", "float64", "E,WS"),
]


# buffers that follow lp_ws_stride / stats in bridges_env_buffers
ENV_BUFFER_FIELDS_TAIL = [
    ("cand_stable", "uint8", "C"),
    ("cand_queue", "int32", "C"),
    ("cand_counters", "int32", "4"),
    ("cand_ws", "float64", "CWS,WSC"),
]
ENV_LP_SNAP_DOUBLES = 64 + (3 * MAX_BLOCKS + 2) * (4 * MAX_INTERFACES + 2 + 3 * MAX_BLOCKS + 1)


class EnvBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in ENV_BUFFER_FIELDS] + [
        ("lp_ws_stride", C.c_int64), ("stats", C.c_void_p)] + [(name, C.c_void_p) for name, _, _ in ENV_BUFFER_FIELDS_TAIL] + [
        ("cand_ws_stride", C.c_int64), ("lp_snap", C.c_void_p), ("lp_snap_stride", C.c_int64)]


# (field name, torch dtype name, shape expression in E, T) -- the device buffers of bridges_task_buffers, in header order
GAUSS_TAPS = 101
TASK_BUFFER_FIELDS = [
    ("env_targets", "float64", "E,T,3"),
    ("target_bits", "int64", "E,64"),          # uint64 on the device
    ("reward_map", "float32", "E,64,64"),
    ("reward_prefix", "float64", "E,64,65"),
    ("task_episode", "int32", "E"),            # uint32 on the device
]


# the device buffers of per-env obstacles (shape expression in E, O): env_obstacle_bits sits in the slot the header reserved for
# it, env_obstacles at the end of the struct
MAX_OBSTACLES = 4
OBSTACLE_BUFFER_FIELDS = [
    ("env_obstacles", "float64", "E,O,3"),
    ("env_obstacle_bits", "int64", "E,64"),    # uint64 on the device
]


class TaskBuffers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in TASK_BUFFER_FIELDS] + [
        ("env_obstacle_bits", C.c_void_p), ("gauss_k", C.c_void_p), ("target_shape", C.c_int32), ("sample", C.c_int32),
        ("x_range", C.c_double * 2), ("z_range", C.c_double * 2),
        # per-env obstacles: appended, so the fields above keep their offsets
        ("env_obstacles", C.c_void_p), ("n_obstacles", C.c_int32), ("sample_obstacles", C.c_int32),
        ("obs_x_range", (C.c_double * 2) * MAX_OBSTACLES), ("obs_z_range", (C.c_double * 2) * MAX_OBSTACLES)]


# bridges_task_family: one integer n per env and episode names the task (bridges_env_set_task_family)
FAMILY_NONE, FAMILY_SPAN, FAMILY_TOWER = 0, 1, 2
PARK_Z = -1000.0                               # BRIDGES_PARK_Z: z of an obstacle slot the drawn task does not use
EPISODE_STATS_MAX_CLASSES = 8
FAMILY_MAX_CLASSES = 8                         # classes of a threshold table (bridges_family_thresholds)
FAMILY_MAX_WEIGHT = 1 << 20                    # largest weight of a class
FAMILY_FAIL_SCALE = 65536                      # bridges_family_curriculum: w = w_min + round(fail * 65536)
NSTEP_MAX = 8                                  # BRIDGES_NSTEP_MAX: the longest horizon of an n-step record


class TaskFamily(C.Structure):
    _fields_ = [("family", C.c_int32), ("n_lo", C.c_int32), ("n_hi", C.c_int32), ("pad_", C.c_int32),
                ("size", C.c_double), ("x", C.c_double), ("task_class", C.c_void_p)]


# bridges_env_fork (the table fork_table() of csrc/api.hip, in its order): the per-env STATE arrays a fork copies -- fields of
# bridges_env_buffers, then of bridges_task_buffers, then of bridges_task_family -- and the per-env buffers it deliberately
# leaves alone, each with its reason.  A per-env buffer that stands in neither list fails tests/test_cpu_beam.py.
FORK_ENV_FIELDS = ("n_blocks", "blk_shape", "blk_pose", "blk_verts", "blk_occ", "targets_left", "state_bits", "n_if", "if_body",
                   "if_geom", "draw_counter", "needs_reset", "step_flags", "reward", "lin_reward", "n_reached", "n_cand", "lp_ws",
                   "lp_snap")
FORK_TASK_FIELDS = ("env_targets", "target_bits", "reward_map", "reward_prefix", "task_episode", "env_obstacles", "env_obstacle_bits")
FORK_FAMILY_FIELDS = ("task_class",)
FORK_EXCLUDED = {
    "sel_index": "an input of the next step, written by its caller",
    "n_valid": "candidate array: recounted by the refresh after the fork",
    "cand_offset": "candidate array: the prefix sum of the refresh",
    "state_raster": "rewritten from state_bits by the refresh",
    "state_raster_nz": "describes the buffer slot (what the sparse update left in it), not the env",
}
BEAM_MAX_WIDTH = 16                            # bridges_beam_select, bridges_beam_merge: 1 <= B <= 16
BEAM_MAX_SLOTS = 64                            # bridges_beam_merge: 1 <= K <= 64
REC_WIDTH = 111                                # BRIDGES_REC_WIDTH: the doubles of a transition record
BEAM_TRACE_MAX_DEPTH = 16                      # bridges_beam_trace: 1 <= D <= BRIDGES_REC_K


# put lp_ws_stride right after lp_ws as in the header (fields above are already in header order)
assert [f[0] for f in EnvBuffers._fields_][-10:-7] == ["lp_ws", "lp_ws_stride", "stats"]

# argument types of every entry point that returns an int status (all but the three special symbols below)
vp, i32, i64, f64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_float
SIGNATURES = {
    "bridges_env_create": [C.POINTER(Task), C.POINTER(EnvBuffers), C.POINTER(vp)],
    "bridges_env_destroy": [vp],
    "bridges_env_reset": [vp, vp],
    "bridges_env_step": [vp, vp],
    "bridges_env_select_random": [vp, vp],
    "bridges_env_lockstep_random": [vp, vp],
    "bridges_env_refresh": [vp, vp],
    "bridges_env_candidate_stability": [vp, vp],
    "bridges_env_restrict_to_stable": [vp, vp],
    "bridges_env_rebuild_contacts": [vp, vp],
    "bridges_env_fork_scratch": [vp, C.POINTER(i64)],
    "bridges_env_fork": [vp, vp, vp, i64, vp],
    "bridges_env_set_task_buffers": [vp, C.POINTER(TaskBuffers)],
    "bridges_env_set_task_family": [vp, C.POINTER(TaskFamily)],
    "bridges_env_set_family_thresholds": [vp, vp],
    "bridges_env_load_targets": [vp, vp],
    "bridges_gate_create": [C.POINTER(vp)],
    "bridges_gate_destroy": [vp],
    "bridges_env_set_gate": [vp, vp],
    "bridges_env_timing_begin": [vp, i32],
    "bridges_env_timing_end": [vp, C.POINTER(C.c_double), C.POINTER(i32)],
    "bridges_shapes_upload": [C.POINTER(Shape), i32, C.POINTER(vp)],
    "bridges_shapes_free": [vp],
    "bridges_place": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_create_block": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_pose_block": [vp, i32, vp, vp, vp, vp],
    "bridges_face_frames": [vp, i32, vp, vp, vp, vp],
    "bridges_contains_points": [vp, i32, vp, i32, vp, vp, vp],
    "bridges_raster": [vp, i32, vp, vp, vp, vp, vp, vp, vp],
    "bridges_raster_sized": [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp],
    "bridges_render_blocks": [vp, i32, vp, vp, vp, i32, vp, i32, vp, vp],
    "bridges_bits_or": [i32, vp, vp, vp, vp],
    "bridges_action_features": [vp, i32, vp, vp, vp, vp, i32, f64, f64, f64, f64, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_bits_to_f32": [i32, vp, vp, vp],
    "bridges_conv_input_rows": [i32, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp],
    "bridges_bits_linear": [i32, vp, vp, vp, i32, vp, vp, vp, vp],
    "bridges_bits_linear2": [i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp],
    "bridges_sigmoid_dot": [i32, vp, i64, vp, i32, vp, vp],
    "bridges_sigmoid_dot_rows": [i32, vp, i64, vp, vp, i32, vp, vp],
    "bridges_bits_dot": [i32, vp, vp, vp, vp, vp, vp],
    "bridges_head_sigmoid_dot": [i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, i32, vp],
    "bridges_head_sigmoid_dot_rows": [i32, i32, i32, vp, i64, vp, vp, vp, vp, i32, vp, vp, i32, vp],
    "bridges_linear_backward_log": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i32, vp, i32, vp, vp, vp],
    "bridges_mlp_mid_rows": [i32, i32, vp, vp, vp, vp, i64, vp, i64, vp, vp],
    "bridges_mlp_mid_supported": [i32, i32, vp],
    "bridges_mlp_mid_forward": [i32, i32, vp, vp, vp, vp, vp],
    "bridges_mlp_mid_backward": [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, f64, f64, f64, f64, vp],
    "bridges_eps_greedy_select": [i32, i32, vp, vp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_boltzmann_select": [i32, i32, vp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_boltzmann_select_rel": [i32, i32, vp, vp, vp, vp, C.c_float, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_beam_select": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_particle_select": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                vp],
    "bridges_beam_merge": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp],
    "bridges_beam_trace": [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f64, f64, vp, vp, vp, vp],
    "bridges_valid_rows": [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_env_groups": [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_env_groups_keyed": [i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp],
    "bridges_record_state": [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_record_result": [i32, vp, vp, vp, vp, vp, vp],
    "bridges_episode_stats": [i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp],
    "bridges_episode_stats_by_class": [i32, i32, vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp],
    "bridges_family_thresholds": [vp, i32, vp, vp],
    "bridges_family_draw": [C.c_uint64, i32, i32, vp, i32, i32, vp, vp, vp],
    "bridges_family_curriculum": [vp, i32, vp, i32, i32, f64, C.c_uint32, i32, vp, vp, vp],
    "bridges_replay_unpack": [i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_replay_unpack_prev": [i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_bits_accumulate": [i32, vp, vp, vp, vp, vp, vp],
    "bridges_stability": [vp, i32, i32, vp, vp, vp, vp, vp, f64, f64, f64, f64, vp, vp, vp, i64, vp],
    "bridges_stability_penalty": [vp, i32, i32, vp, vp, vp, vp, vp, f64, f64, f64, f64, f64, vp, vp, vp, vp, i64, vp],
    "bridges_soft_update": [vp, vp, i64, f32, f32, vp],
    "bridges_bias_relu": [vp, vp, i64, i32, i32, vp],
    "bridges_bias_relu_pool2": [vp, vp, vp, i64, i32, i32, i32, vp],
    "bridges_conv3x3_relu_o16": [vp, vp, vp, vp, i64, i32, i32, i32, i32, vp],
    "bridges_conv3x3_relu_o16_ex": [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp],
    "bridges_upconv2x2": [vp, vp, vp, vp, i64, i32, i32, i32, i32, vp],
    "bridges_linear_forward": [i32, i32, i32, vp, vp, vp, i32, vp, vp, i64, vp, vp],
    "bridges_linear_backward": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i32, vp],
    "bridges_mlp_input": [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_mlp_input_batches": [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp],
    "bridges_mlp_input_rows": [i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp],
    "bridges_mlp_input_batches_rows": [i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp],
    "bridges_mlp_input_task_rows": [i32, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp],
    "bridges_mlp_input_batches_task_rows": [i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp],
    "bridges_successor_loss": [i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp],
    "bridges_successor_loss_rows": [i32, i32, i32, i32, vp, vp, i64, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp],
    "bridges_adam_step": [vp, vp, vp, vp, i64, vp, f64, f64, f64, f64, vp],
    "bridges_linear_backward_adam": [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, f64, f64, f64, f64, vp, i32, vp],
    "bridges_conv3x3": [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp],
    "bridges_conv3x3_wgrad_scratch": [i64, i32, i32, i32, C.POINTER(i64)],
    "bridges_conv3x3_wgrad": [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp],
    "bridges_maxpool2": [vp, vp, i64, i32, i32, vp],
    "bridges_bias_grad": [vp, vp, vp, i64, i64, i32, i32, vp],
    "bridges_adam_multi": [vp, i32, vp, vp, i32, vp, f64, f64, f64, f64, vp],
    "bridges_reduce_jobs": [vp, i32, i32, vp],
    "bridges_upconv2x2_backward_scratch": [i64, i32, i32, i32, i32, C.POINTER(i64)],
    "bridges_upconv2x2_backward": [vp, vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, i32, vp],
    "bridges_conv1x1_o1_forward": [vp, vp, vp, vp, i64, i32, i32, vp],
    "bridges_conv1x1_o1_backward": [vp, vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp],
    "bridges_maxpool2_relu_backward": [vp, vp, vp, i64, i32, i32, vp],
    "bridges_td_target": [i32, vp, vp, vp, vp, i64, vp, vp, vp, f32, i32, vp, vp, vp, vp],
    "bridges_td_target_rows": [i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp],
    "bridges_td_target_select": [i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, f32, i32, vp, vp, vp, vp],
    "bridges_soft_expect": [i32, vp, vp, vp, vp, f32, vp, i64, vp, i32, vp, vp, vp, vp, vp],
    "bridges_soft_expect_rel": [i32, vp, vp, vp, vp, f32, f32, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp],
    "bridges_soft_value": [i32, vp, vp, vp, f32, vp, f32, f32, vp, vp, vp, vp, vp],
    "bridges_soft_value_rel": [i32, vp, vp, vp, f32, f32, vp, f32, f32, vp, vp, vp, vp, vp, vp],
    "bridges_action_row": [i32, vp, vp, vp, vp, vp, vp, i64, vp, vp],
    "bridges_nstep_fold": [i32, i32, i32, vp, vp, f64, vp, vp, vp, vp, vp, vp, vp, vp],
    "bridges_bits_discounted_sum": [i32, vp, i64, vp, vp, f32, vp, vp, vp],
    "bridges_priority_sample_scratch": [i64, C.POINTER(i64)],
    "bridges_priority_sample": [i64, i32, i32, vp, f64, i64, vp, vp, vp, i64, vp],
    "bridges_priority_update": [i64, i32, i32, vp, i64, vp, vp, vp, vp],
    "bridges_priority_weights": [i64, i64, i64, vp, f64, vp, i64, vp, vp],
    "bridges_hindsight_relabel_scratch": [i32, i32, C.POINTER(i64)],
    "bridges_hindsight_relabel": [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, C.c_uint64, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp,
                                  i64, vp],
    "bridges_hindsight_relabel_nstep": [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, C.c_uint64, i32, vp, i32, i32, vp, vp, i32, vp, i32,
                                        f64, vp, vp, vp, i64, vp],
    "bridges_hindsight_per_step_scratch": [i32, i32, C.POINTER(i64)],
    "bridges_hindsight_per_step": [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, C.c_uint64, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp,
                                   i64, vp],
    "bridges_hindsight_per_step_nstep": [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, C.c_uint64, i32, vp, i32, i32, vp, vp, i32, vp, i32,
                                         f64, vp, vp, vp, i64, vp],
    "bridges_successor_loss_weighted": [i32, i32, i32, i32, vp, vp, i64, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
}


# every symbol include/bridges_hip.h declares
EXPORTED_SYMBOLS = ("bridges_last_error", "bridges_device_count", "bridges_source_hash", *SIGNATURES)

_lib = None


def lib():
    """Load libbridges_hip.so (once).  Raises BridgesHipError if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BridgesHipError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    try:
        L.bridges_source_hash.restype = C.c_char_p
        stamp = L.bridges_source_hash().decode()[len(STAMP_PREFIX):]
    except AttributeError:
        stamp = "missing"
    want = source_hash()
    if stamp != want:
        raise BridgesHipError(f"{LIB_PATH} is stale: it was built from other sources (stamp {stamp[:16]}, sources {want[:16]}); "
                              "rebuild it with `python __graft_entry__.py build`")
    L.bridges_last_error.restype = C.c_char_p
    L.bridges_device_count.restype = C.c_int
    for name, argtypes in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = lib().bridges_last_error().decode(errors="replace")
        raise BridgesHipError(f"{what} failed (rc={rc}): {msg}")


def require_gpu():
    """Fail loudly when the HIP path cannot run."""
    import torch
    L = lib()
    if not torch.cuda.is_available() or L.bridges_device_count() <= 0:
        raise BridgesHipError("no MI355X / HIP device visible: the assembly_gym hot path runs only on the "
                              "HIP kernels of libbridges_hip.so (no CPU fallback)")
    return L


def current_stream():
    """torch's current stream of the current device as the C ABI's ``void* stream`` (the raw getter: a tenth of the cost of
    building a torch.cuda.Stream object per operator call)."""
    import torch
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
